// rice_walk_check.cpp - stand-alone check of honours_amd/csrc/press_rice_walk.h (host code, no device): streams of known
// length in heap blocks of exactly that length, so that a sanitizer sees any byte read behind the last code.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rice_walk_check.cpp -o rice_walk_check
//   ./rice_walk_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../honours_amd/csrc/press_rice_walk.h"

static void put_bit(std::vector<uint8_t> &b, uint64_t &n, int bit)
{
	if (b.size() <= n / 8)
		b.push_back(0);
	if (bit)
		b[n / 8] |= (uint8_t) (1u << (n % 8));
	n++;
}

// header (2 bytes), nex = 0 for every layout (the section is then the count alone), rice(low) at k
static std::vector<uint8_t> stream_of(const std::vector<uint8_t> &low, uint32_t k)
{
	std::vector<uint8_t> s(6, 0), p;
	s[0] = 0x34, s[1] = 0x12;
	uint64_t n = 0;
	put_bit(p, n, (k >> 2) & 1), put_bit(p, n, (k >> 1) & 1), put_bit(p, n, k & 1);
	for (uint8_t x : low) {
		for (uint32_t q = x >> k; q; q--)
			put_bit(p, n, 1);
		put_bit(p, n, 0);
		for (int j = (int) k - 1; j >= 0; j--)
			put_bit(p, n, (x >> j) & 1);
	}
	s.insert(s.end(), p.begin(), p.end());
	return s;
}

int main()
{
	int bad = 0, cases = 0;
	uint32_t seed = 12345;
	for (uint32_t k = 0; k < 8; k++) {
		for (uint32_t count : { 0u, 1u, 2u, 7u, 8u, 9u, 300u, 5000u }) {
			std::vector<uint8_t> low(count);
			for (auto &x : low) {
				seed = seed * 1664525u + 1013904223u;
				x = (uint8_t) ((seed >> 24) % (count % 3 ? 256u : 20u));
			}
			const std::vector<uint8_t> s = stream_of(low, k);
			for (int layout = 0; layout < 4; layout++) {
				uint8_t *heap = (uint8_t *) malloc(s.size()); // exactly the stream
				memcpy(heap, s.data(), s.size());
				uint64_t len = 0;
				const bool ok = ph::rice_stream_len(layout, heap, (uint64_t) count + 1, &len);
				if (!ok || len != s.size()) {
					printf("k %u count %u layout %d: %d, %llu for %zu\n", k, count, layout, (int) ok, (unsigned long long) len, s.size());
					bad++;
				}
				free(heap);
				cases++;
			}
		}
	}
	// vbe21 with exceptions: 6 bytes each in front of the payload; a count the header contradicts
	{
		std::vector<uint8_t> s = stream_of({ 1, 2, 3 }, 1);
		s[2] = 2;
		s.insert(s.begin() + 6, 12, 0xEE);
		uint64_t len = 0;
		if (!ph::rice_stream_len(0, s.data(), 6, &len) || len != s.size())
			bad++, printf("vbe21 with exceptions: %llu for %zu\n", (unsigned long long) len, s.size());
		if (ph::rice_stream_len(0, s.data(), 2, &len) || ph::rice_stream_len(0, s.data(), 0, &len))
			bad++, printf("a contradicted count was accepted\n");
		cases += 3;
	}
	printf("%d cases, %d bad\n", cases, bad);
	return bad ? 1 : 0;
}
