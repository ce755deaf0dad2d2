// dhuf_walk_check.cpp - stand-alone check of honours_amd/csrc/press_dhuf_walk.h (host code, no device): streams in heap
// blocks of exactly their length, whole and cut at every byte, so that a sanitizer sees any byte read behind the end.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/dhuf_walk_check.cpp -o dhuf_walk_check
//   ./dhuf_walk_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../honours_amd/csrc/press_dhuf_walk.h"

static void put32(std::vector<uint8_t> &s, uint32_t v)
{
	for (int i = 0; i < 4; i++)
		s.push_back((uint8_t) (v >> (8 * i)));
}

// first sample, nex, a section of the layout's shape (the coded blocks: lp and lv bytes), then a table head that
// announces nlow values and `tail` further bytes
static std::vector<uint8_t> stream_of(int layout, uint32_t nex, uint32_t lp, uint32_t lv, uint32_t nlow, uint32_t tail)
{
	std::vector<uint8_t> s = { 0x34, 0x12 };
	put32(s, nex);
	if (layout == 0) {
		s.insert(s.end(), 6 * (size_t) nex, 0xEE);
	} else if (nex == 1) {
		s.insert(s.end(), 6, 0xEE);
	} else if (nex > 1) {
		put32(s, lp);
		s.insert(s.end(), lp, 0xEE);
		put32(s, lv);
		s.insert(s.end(), lv, 0xEE);
	}
	s.push_back(0x01);
	for (int i = 3; i >= 0; i--)
		s.push_back((uint8_t) (nlow >> (8 * i)));
	s.insert(s.end(), tail, 0x55);
	return s;
}

static int check(const std::vector<uint8_t> &s, int layout, size_t len, bool want_ok, uint64_t want_n)
{
	uint8_t *heap = (uint8_t *) malloc(len ? len : 1); // exactly the bytes given
	memcpy(heap, s.data(), len);
	uint64_t n = 0;
	const bool ok = ph::dhuf_stream_samples(layout, heap, len, &n);
	free(heap);
	if (ok != want_ok || (ok && n != want_n)) {
		printf("layout %d len %zu of %zu: %d, %llu (wanted %d, %llu)\n", layout, len, s.size(), (int) ok, (unsigned long long) n,
		       (int) want_ok, (unsigned long long) want_n);
		return 1;
	}
	return 0;
}

int main()
{
	int bad = 0, cases = 0;
	for (int layout = 0; layout < 4; layout++) {
		for (uint32_t nex : { 0u, 1u, 2u, 7u, 300u }) {
			for (uint32_t nlow : { 0u, 1u, 255u, 65536u, 14930351u }) {
				const std::vector<uint8_t> s = stream_of(layout, nex, 3 + nex, 1 + 2 * nex, nlow, 9);
				const size_t head = s.size() - 9;
				// whole, cut right behind the count field, and cut at every byte in front of that
				bad += check(s, layout, s.size(), true, 1ull + nex + nlow), cases++;
				bad += check(s, layout, head, true, 1ull + nex + nlow), cases++;
				for (size_t len = 0; len < head; len += (head > 600 ? 37 : 1))
					bad += check(s, layout, len, false, 0), cases++;
				bad += check(s, layout, head - 1, false, 0), cases++;
			}
		}
	}
	// a stream that says more samples than a count can hold; length fields that point far behind the end
	{
		std::vector<uint8_t> s = stream_of(0, 2, 0, 0, 0xFFFFFFFFu, 0);
		bad += check(s, 0, s.size(), false, 0), cases++;
		s = stream_of(1, 5, 4, 4, 10, 0);
		s[6] = s[7] = s[8] = s[9] = 0xFF; // lp = 2^32 - 1
		bad += check(s, 1, s.size(), false, 0), cases++;
		s = stream_of(2, 5, 4, 4, 10, 0);
		s[14] = s[15] = s[16] = s[17] = 0xFF; // lv = 2^32 - 1
		bad += check(s, 2, s.size(), false, 0), cases++;
		s = stream_of(0, 0, 0, 0, 10, 0);
		s[2] = s[3] = s[4] = s[5] = 0xFF; // nex = 2^32 - 1 under vbe21: the section alone is 24 GiB
		bad += check(s, 0, s.size(), false, 0), cases++;
	}
	printf("%d cases, %d bad\n", cases, bad);
	return bad ? 1 : 0;
}
