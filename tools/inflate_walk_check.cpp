// inflate_walk_check.cpp - stand-alone check of honours_amd/csrc/press_inflate_walk.h (host code, no device): the serial
// walk ph::inflate_serial over the battery of tests/golden/inflate_battery.bin (tests/_inflate.py writes it: every
// malformed stream of the test battery with the status the model gives it, and the small valid ones) and over seeded
// random mutations of the valid streams.  Every stream stands in a heap block of exactly its length and every output in
// one of exactly its capacity, so that a sanitizer sees any byte read or written outside them.  With -DWITH_ZLIB (and
// -lz) every verdict is also held against zlib's uncompress: OK exactly where it succeeds, and then the same bytes.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DWITH_ZLIB tools/inflate_walk_check.cpp -lz -o inflate_walk_check
//   ./inflate_walk_check tests/golden/inflate_battery.bin
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../honours_amd/csrc/press_inflate_walk.h"

#ifdef WITH_ZLIB
#include <zlib.h>
#endif

struct Entry {
	uint8_t status;
	uint64_t n;
	uint32_t hash;
	std::vector<uint8_t> s;
};

static uint32_t fnv1a(const uint8_t *p, size_t n)
{
	uint32_t h = 0x811C9DC5u;
	for (size_t i = 0; i < n; i++)
		h = (h ^ p[i]) * 0x01000193u;
	return h;
}

// the walk on exact heap blocks; out_cap bytes of room
static uint8_t run(const std::vector<uint8_t> &s, size_t len, size_t cap, bool with_out, uint64_t *n, std::vector<uint8_t> *keep)
{
	uint8_t *in = (uint8_t *) malloc(len ? len : 1);
	if (len)
		memcpy(in, s.data(), len);
	uint8_t *out = with_out ? (uint8_t *) malloc(cap ? cap : 1) : nullptr;
	const uint8_t st = ph::inflate_serial(in, len, out, with_out ? cap : 0, n);
	if (keep && out)
		keep->assign(out, out + (st == ph::ifw::OK ? *n : 0));
	free(in);
	free(out);
	return st;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return (uint32_t) (rng_state >> 16);
}

int main(int argc, char **argv)
{
	const char *path = argc > 1 ? argv[1] : "tests/golden/inflate_battery.bin";
	FILE *f = fopen(path, "rb");
	if (!f) {
		printf("cannot open %s\n", path);
		return 2;
	}
	std::vector<uint8_t> file;
	uint8_t buf[65536];
	for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;)
		file.insert(file.end(), buf, buf + k);
	fclose(f);
	if (file.size() < 8 || memcmp(file.data(), "IFB1", 4)) {
		printf("%s is no battery\n", path);
		return 2;
	}
	uint32_t count;
	memcpy(&count, file.data() + 4, 4);
	std::vector<Entry> es;
	size_t p = 8;
	for (uint32_t i = 0; i < count; i++) {
		if (p + 17 > file.size())
			return 2;
		Entry e;
		uint32_t len;
		e.status = file[p];
		memcpy(&e.n, file.data() + p + 1, 8);
		memcpy(&e.hash, file.data() + p + 9, 4);
		memcpy(&len, file.data() + p + 13, 4);
		p += 17;
		if (p + len > file.size())
			return 2;
		e.s.assign(file.begin() + p, file.begin() + p + len);
		p += len;
		es.push_back(e);
	}
	int bad = 0;
	long cases = 0, agree_ok = 0;
	auto fail = [&](const char *what, size_t i, int got, int want) {
		printf("stream %zu: %s: %d (wanted %d)\n", i, what, got, want);
		bad++;
	};
	// the battery: the status, the length and the bytes; the count alone; a slot one byte short; no slot
	for (size_t i = 0; i < es.size(); i++) {
		const Entry &e = es[i];
		uint64_t n = 0;
		std::vector<uint8_t> out;
		const size_t cap = e.status == 0 ? (size_t) e.n : 1000;
		uint8_t st = run(e.s, e.s.size(), cap, true, &n, &out);
		cases++;
		if (st != e.status)
			fail("status", i, st, e.status);
		else if (st == 0 && (n != e.n || fnv1a(out.data(), out.size()) != e.hash))
			fail("bytes", i, (int) n, (int) e.n);
		else if (st != 0 && n != UINT64_MAX && st != ph::ifw::ROOM)
			fail("a failed stream has a length", i, (int) n, -1);
		if (e.status == 0) {
			st = run(e.s, e.s.size(), 0, false, &n, nullptr);
			cases++;
			if (e.n ? (st != ph::ifw::ROOM || n != e.n) : st != 0)
				fail("the count alone", i, st, ph::ifw::ROOM);
			if (e.n) {
				st = run(e.s, e.s.size(), (size_t) e.n - 1, true, &n, nullptr);
				cases++;
				if (st != ph::ifw::ROOM || n != e.n)
					fail("one byte short", i, st, ph::ifw::ROOM);
			}
			// cut at every byte: TRUNCATED (or whole already, with bytes behind its Adler-32)
			for (size_t cut = 0; cut < e.s.size() && e.s.size() < 600; cut++) {
				st = run(e.s, cut, cap, true, &n, nullptr);
				cases++;
				if (st != ph::ifw::TRUNCATED && st != 0)
					fail("cut short", i, st, ph::ifw::TRUNCATED);
			}
		}
	}
	// seeded mutations of the valid streams: nothing but the verdict is asked of them - and zlib's, where it is linked
	for (size_t i = 0; i < es.size(); i++) {
		if (es[i].status != 0)
			continue;
		for (int k = 0; k < 400; k++) {
			std::vector<uint8_t> s = es[i].s;
			const uint32_t kind = rnd() % 4, nmut = 1 + rnd() % 3;
			for (uint32_t j = 0; j < nmut && !s.empty(); j++) {
				const size_t at = kind == 3 ? rnd() % (s.size() < 48 ? s.size() : 48) : rnd() % s.size();
				if (kind == 0)
					s[at] ^= (uint8_t) (1u << (rnd() % 8));
				else if (kind == 1)
					s[at] = (uint8_t) rnd();
				else if (kind == 2)
					s.resize(at);
				else
					s[at] ^= (uint8_t) (1u << (rnd() % 8)); // in the headers
			}
			uint64_t n = 0;
			std::vector<uint8_t> out;
			const size_t cap = (size_t) es[i].n + 70000;
			const uint8_t st = run(s, s.size(), cap, true, &n, &out);
			cases++;
#ifdef WITH_ZLIB
			std::vector<uint8_t> z(cap ? cap : 1);
			unsigned long zn = (unsigned long) cap;
			const int rc = uncompress(z.data(), &zn, s.data(), (unsigned long) s.size());
			if (rc == Z_BUF_ERROR && st == ph::ifw::ROOM)
				continue; // more than the room: zlib has no verdict on the rest
			if ((rc == Z_OK) != (st == 0)) {
				// (Z_BUF_ERROR is also zlib's word for a truncated stream)
				printf("stream %zu mutation %d: status %d, zlib %d\n", i, k, st, rc);
				bad++;
			} else if (st == 0) {
				agree_ok++;
				if (zn != n || (n && memcmp(z.data(), out.data(), n))) {
					printf("stream %zu mutation %d: the bytes differ from zlib's\n", i, k);
					bad++;
				}
			}
#endif
		}
	}
	printf("%ld cases over %zu streams, %ld mutations that zlib and the walk both take, %d bad\n", cases, es.size(), agree_ok, bad);
	return bad ? 1 : 0;
}
