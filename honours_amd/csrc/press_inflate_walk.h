// press_inflate_walk.h - the rules of a zlib stream (RFC 1950 around RFC 1951) as one serial walk, compiled for the host
// and the device: the bounded bit reader, the header check, the block header, the validation of a dynamic block's
// code-length description, the construction of the decode tables and the symbol loop.  The kernels of press_inflate.hip
// run walk() with one wave per record (every lane takes the same steps; the table fill and the byte moves are shared
// out over the lanes by the environment), inflate_serial() below runs it on one host thread, and
// tools/inflate_walk_check.cpp runs that under a sanitizer.  include/press_hip.h section 2zb is the contract,
// tests/_inflate.py the model of the classification.
//
// Safety, whatever the bytes are: the reader never loads a byte at or behind `len` (bits there read as zeros and a field
// that needs one ends the walk with TRUNCATED); every table index is a masked field of the stream or a sum that the
// validation has bounded; every pass of every loop consumes at least one bit or ends the walk, so a walk takes at most
// 8 * len passes.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define IFW_FN __host__ __device__ inline
#else
#define IFW_FN inline
#endif

namespace ph {
namespace ifw {

// the status bytes (PRESS_HIP_INFLATE_* of include/press_hip.h; press_inflate.hip asserts that they agree)
enum : uint8_t { OK = 0, HEADER = 1, TRUNCATED = 2, BTYPE = 3, STORED = 4, CODES = 5, SYMBOL = 6, DISTANCE = 7, ADLER = 8, ROOM = 9, REFUSED = 10 };

constexpr uint32_t LIT_BITS = 10, DIST_BITS = 8, CL_BITS = 7; // widths of the primary tables
constexpr uint32_t NLENS = 320;                               // 288 + 32: the code lengths of one block
constexpr uint32_t ADLER_MOD = 65521;

// ------------------------------------------------------------------ the bit reader

// bytes at .. at + 3 of the stream, zeros at and behind len
IFW_FN uint32_t load32(const uint8_t *p, uint64_t len, uint64_t at)
{
	uint32_t v = 0;
	if (at + 4 <= len) {
		memcpy(&v, p + at, 4);
		return v;
	}
	for (uint32_t i = 0; i < 4; i++)
		if (at + i < len)
			v |= (uint32_t) p[at + i] << (8 * i);
	return v;
}

// Bit i of the stream is bit i % 8 of byte i / 8.  A window of 12 bytes: lo and hi are in use, pre has been loaded for
// the next step (its load is in flight while the bits of lo are consumed).
struct BitIn {
	const uint8_t *p;
	uint64_t len;  // bytes; < 2^32
	uint64_t base; // byte position of lo
	uint32_t lo, hi, pre;
	uint32_t off; // bits of lo | hi consumed; < 32 behind norm()

	IFW_FN void seek(uint64_t byte)
	{
		base = byte;
		lo = load32(p, len, byte);
		hi = load32(p, len, byte + 4);
		pre = load32(p, len, byte + 8);
		off = 0;
	}
	IFW_FN void norm()
	{
		if (off >= 32) {
			lo = hi;
			hi = pre;
			base += 4;
			pre = load32(p, len, base + 8);
			off -= 32;
		}
	}
	IFW_FN uint64_t bitpos() const { return base * 8 + off; }
	IFW_FN bool have(uint32_t n) const { return bitpos() + n <= len * 8; }
	// the next 32 bits, zeros behind the end
	IFW_FN uint32_t peek()
	{
		norm();
		return (uint32_t) ((((uint64_t) hi << 32) | lo) >> off);
	}
	IFW_FN void skip(uint32_t n) { off += n; } // n <= 32, behind a peek()
	IFW_FN uint32_t take(uint32_t n)          // n <= 16
	{
		const uint32_t v = peek() & ((1u << n) - 1);
		off += n;
		return v;
	}
	IFW_FN void align() { off = (off + 7) & ~7u; }
};

// ------------------------------------------------------------------ code sets

// A canonical code over n symbols (RFC 1951 3.2.2): count[l] codes of length l, the symbols sorted by (length, symbol),
// and a primary table over the next `bits` bits of the stream as they stand (first bit lowest): symbol << 4 | length
// for a code of at most `bits` bits, 0 where the canonical walk has to look (a longer code, or no code)
struct Code {
	uint16_t *count;  // [32]: the 16 counts, then code_sort's 16 offsets
	uint16_t *symbol; // [n]
	uint16_t *lut;    // [1 << bits]
	uint32_t bits;
};

// This part is NOT shared out over the lanes: on the device all 64 lanes of the wave run it in lock step on the same LDS
// words, every lane reading and writing the same values (count[l]++ by 64 lanes adds one: they all read the old value
// before any of them writes).  It is right only because the walk is wave-uniform - one wave per workgroup, no divergent
// branch above it - and it costs the n steps once per block; the same holds for the lengths' loop of dynamic_tables.
// code_fill below is the shared part.
// count[] and symbol[] from lens[0 .. n), n <= 288.  -> what is left of the code space: 0 a complete set, > 0 an
// incomplete one, < 0 over-subscribed (then symbol[] is not made).  *ncodes: symbols with a code
IFW_FN int code_sort(const uint8_t *lens, uint32_t n, const Code &c, uint32_t *ncodes)
{
	uint16_t *const offs = c.count + 16;
	for (uint32_t l = 0; l < 16; l++)
		c.count[l] = 0;
	for (uint32_t s = 0; s < n; s++)
		c.count[lens[s] & 15]++;
	*ncodes = n - c.count[0];
	int left = 1;
	for (uint32_t l = 1; l < 16; l++) {
		left <<= 1;
		left -= c.count[l];
		if (left < 0)
			return left;
	}
	offs[1] = 0;
	for (uint32_t l = 1; l < 15; l++)
		offs[l + 1] = (uint16_t) (offs[l] + c.count[l]);
	for (uint32_t s = 0; s < n; s++) {
		const uint32_t l = lens[s] & 15;
		if (l)
			c.symbol[offs[l]++] = (uint16_t) s; // offs[l] < ncodes <= n
	}
	return left;
}

// the canonical walk over the bits of w (first bit lowest), lengths 1 .. maxlen: symbol << 4 | length, 0: no code
IFW_FN uint32_t code_walk(const Code &c, uint32_t w, uint32_t maxlen)
{
	uint32_t code = 0, first = 0, index = 0;
	for (uint32_t l = 1; l <= maxlen; l++) {
		code |= w & 1;
		w >>= 1;
		const uint32_t cnt = c.count[l];
		if (code < first + cnt) // (code >= first: the set is not over-subscribed)
			return (uint32_t) c.symbol[index + (code - first)] << 4 | l;
		index += cnt;
		first = (first + cnt) << 1;
		code <<= 1;
	}
	return 0;
}

// the primary table, entries lane, lane + nlanes, ...
IFW_FN void code_fill(const Code &c, uint32_t lane, uint32_t nlanes)
{
	for (uint32_t j = lane; j < (1u << c.bits); j += nlanes)
		c.lut[j] = (uint16_t) code_walk(c, j, c.bits);
}

// RFC 1951 3.2.5: the extra bits and the first value of a length symbol 257 + li (li <= 28), of a distance symbol (< 30)
IFW_FN uint32_t len_extra(uint32_t li) { return li < 8 || li == 28 ? 0 : (li - 4) >> 2; }
IFW_FN uint32_t len_base(uint32_t li) { return li < 8 ? 3 + li : li == 28 ? 258 : 3 + ((4 + (li & 3)) << ((li - 4) >> 2)); }
IFW_FN uint32_t dist_extra(uint32_t ds) { return ds < 4 ? 0 : (ds - 2) >> 1; }
IFW_FN uint32_t dist_base(uint32_t ds) { return ds < 4 ? 1 + ds : 1 + ((2 + (ds & 1)) << ((ds - 2) >> 1)); }

// ------------------------------------------------------------------ the walk

// What a walk works in.  Env gives:
//   BitIn b; uint8_t *lens /* NLENS */; Code lit /* 288, LIT_BITS */, dist /* 32, DIST_BITS */, cl /* 19, CL_BITS */;
//   uint32_t lane(), nlanes(); void sync() - between the writes of a table and its reads by other lanes;
//   uint32_t u(uint32_t) - a value every lane holds alike (the device keeps it in a scalar register);
//   void literal(uint32_t byte); void match(uint32_t len, uint32_t dist) - dist <= produced();
//   void stored(uint64_t at, uint32_t n) - n bytes of the stream from byte `at`, inside it;
//   uint64_t produced().

// one symbol of code c: -> its value, or -1 with *st TRUNCATED (a bit of it lies behind the end) or SYMBOL (15 bits that
// are no code: only an incomplete distance or literal set has such)
template <class Env>
IFW_FN int symbol(Env &e, const Code &c, uint8_t *st)
{
	const uint32_t w = e.b.peek();
	uint32_t en = e.u(c.lut[w & ((1u << c.bits) - 1)]);
	if (!en)
		en = e.u(code_walk(c, w, 15));
	if (!en) {
		*st = e.b.have(15) ? SYMBOL : TRUNCATED;
		return -1;
	}
	if (!e.b.have(en & 15)) {
		*st = TRUNCATED;
		return -1;
	}
	e.b.skip(en & 15);
	return (int) (en >> 4);
}

// a set zlib takes: complete, or one code of one bit
IFW_FN bool set_ok(int left, const Code &c, uint32_t ncodes) { return left == 0 || (left > 0 && ncodes == 1 && c.count[1] == 1); }

// the tables of a dynamic block from its header (behind BTYPE): 0, or the status
template <class Env>
IFW_FN uint8_t dynamic_tables(Env &e)
{
	BitIn &b = e.b;
	if (!b.have(14))
		return TRUNCATED;
	const uint32_t nlen = e.u(b.take(5)) + 257, ndist = e.u(b.take(5)) + 1, ncode = e.u(b.take(4)) + 4;
	if (nlen > 286 || ndist > 30)
		return CODES;
	const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
	uint64_t packed = 0; // the 19 lengths of the code-length code, 3 bits each, by symbol
	for (uint32_t i = 0; i < ncode; i++) {
		if (!b.have(3))
			return TRUNCATED;
		packed |= (uint64_t) e.u(b.take(3)) << (3 * order[i]);
	}
	e.sync(); // (the block before may still read lens and the tables)
	for (uint32_t s = 0; s < 19; s++)
		e.lens[s] = (uint8_t) ((packed >> (3 * s)) & 7);
	e.sync();
	uint32_t ncodes;
	if (code_sort(e.lens, 19, e.cl, &ncodes) != 0)
		return CODES; // over-subscribed or incomplete: the code-length code must be complete
	e.sync();
	code_fill(e.cl, e.lane(), e.nlanes());
	e.sync();
	const uint32_t total = nlen + ndist; // <= 316
	uint32_t idx = 0;
	while (idx < total) {
		uint8_t st = OK;
		const int s = symbol(e, e.cl, &st);
		if (s < 0)
			return st;
		if (s < 16) {
			e.lens[idx++] = (uint8_t) s;
			continue;
		}
		const uint32_t eb = s == 16 ? 2 : s == 17 ? 3 : 7;
		if (!b.have(eb))
			return TRUNCATED;
		const uint32_t rep = (s == 18 ? 11 : 3) + e.u(b.take(eb));
		if ((s == 16 && idx == 0) || idx + rep > total)
			return CODES; // a repeat with nothing before it, or past the end
		const uint8_t v = s == 16 ? e.lens[idx - 1] : 0;
		for (uint32_t k = 0; k < rep; k++)
			e.lens[idx++] = v;
	}
	e.sync();
	if (e.lens[256] == 0)
		return CODES; // no end-of-block code
	int left = code_sort(e.lens, nlen, e.lit, &ncodes);
	if (!set_ok(left, e.lit, ncodes))
		return CODES;
	left = code_sort(e.lens + nlen, ndist, e.dist, &ncodes);
	if (!(ncodes == 0 || set_ok(left, e.dist, ncodes)))
		return CODES;
	e.sync();
	code_fill(e.lit, e.lane(), e.nlanes());
	code_fill(e.dist, e.lane(), e.nlanes());
	e.sync();
	return OK;
}

// ... of a fixed block (RFC 1951 3.2.6)
template <class Env>
IFW_FN void fixed_tables(Env &e)
{
	e.sync();
	for (uint32_t s = e.lane(); s < 288; s += e.nlanes())
		e.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
	for (uint32_t s = e.lane(); s < 32; s += e.nlanes())
		e.lens[288 + s] = 5;
	e.sync();
	uint32_t ncodes;
	(void) code_sort(e.lens, 288, e.lit, &ncodes);
	(void) code_sort(e.lens + 288, 32, e.dist, &ncodes);
	e.sync();
	code_fill(e.lit, e.lane(), e.nlanes());
	code_fill(e.dist, e.lane(), e.nlanes());
	e.sync();
}

// the symbols of a Huffman block up to its end-of-block: 0, or the status
template <class Env>
IFW_FN uint8_t block_symbols(Env &e)
{
	BitIn &b = e.b;
	for (;;) {
		uint8_t st = OK;
		const int s = symbol(e, e.lit, &st);
		if (s < 0)
			return st;
		if (s < 256) {
			e.literal((uint32_t) s);
			continue;
		}
		if (s == 256)
			return OK;
		if (s >= 286)
			return SYMBOL;
		const uint32_t li = (uint32_t) s - 257, leb = len_extra(li);
		if (!b.have(leb))
			return TRUNCATED;
		const uint32_t len = len_base(li) + e.u(b.take(leb));
		const int ds = symbol(e, e.dist, &st);
		if (ds < 0)
			return st;
		if (ds >= 30)
			return SYMBOL;
		const uint32_t deb = dist_extra((uint32_t) ds);
		if (!b.have(deb))
			return TRUNCATED;
		const uint32_t dist = dist_base((uint32_t) ds) + e.u(b.take(deb));
		if (dist > e.produced())
			return DISTANCE; // (before a single byte is copied)
		e.match(len, dist);
	}
}

// The whole stream: the status - OK with *adler the stored Adler-32 (the caller compares it with the bytes' own, where it
// has them) - and what the environment has taken.  Bytes behind the Adler-32 are not looked at.
template <class Env>
IFW_FN uint8_t walk(Env &e, uint32_t *adler)
{
	BitIn &b = e.b;
	b.seek(0);
	if (!b.have(16))
		return TRUNCATED;
	const uint32_t cmf = e.u(b.take(8)), flg = e.u(b.take(8));
	if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20))
		return HEADER;
	for (;;) {
		if (!b.have(3))
			return TRUNCATED;
		const uint32_t last = e.u(b.take(1)), type = e.u(b.take(2));
		if (type == 3)
			return BTYPE;
		if (type == 0) {
			b.align();
			if (!b.have(32))
				return TRUNCATED;
			const uint32_t n = e.u(b.take(16)), nn = e.u(b.take(16));
			if (n != (nn ^ 0xFFFF))
				return STORED;
			b.norm();
			const uint64_t at = b.bitpos() >> 3;
			if (at + n > b.len)
				return TRUNCATED;
			if (n)
				e.stored(at, n);
			b.seek(at + n);
		} else {
			if (type == 1) {
				fixed_tables(e);
			} else if (const uint8_t st = dynamic_tables(e)) {
				return st;
			}
			if (const uint8_t st = block_symbols(e))
				return st;
		}
		if (last)
			break;
	}
	b.align();
	if (!b.have(32))
		return TRUNCATED;
	uint32_t a = 0;
	for (int i = 0; i < 4; i++)
		a = a << 8 | e.u(b.take(8));
	*adler = a;
	return OK;
}

// ------------------------------------------------------------------ one host thread

struct SerialEnv {
	BitIn b;
	uint8_t lens_[NLENS];
	uint16_t cnt_[3][32], sym_[288 + 32 + 19], lut_[(1 << LIT_BITS) + (1 << DIST_BITS) + (1 << CL_BITS)];
	uint8_t *lens = lens_;
	Code lit = { cnt_[0], sym_, lut_, LIT_BITS }, dist = { cnt_[1], sym_ + 288, lut_ + (1 << LIT_BITS), DIST_BITS },
	     cl = { cnt_[2], sym_ + 320, lut_ + (1 << LIT_BITS) + (1 << DIST_BITS), CL_BITS };
	uint8_t *out;
	uint64_t cap, n = 0;
	uint32_t s1 = 1, s2 = 0;
	bool room = true; // every byte so far has been written
	uint32_t lane() const { return 0; }
	uint32_t nlanes() const { return 1; }
	void sync() {}
	uint32_t u(uint32_t v) const { return v; }
	uint64_t produced() const { return n; }
	void put(uint8_t v)
	{
		if (n < cap) {
			out[n] = v;
			s1 = (s1 + v) % ADLER_MOD;
			s2 = (s2 + s1) % ADLER_MOD;
		} else {
			room = false;
		}
		n++;
	}
	void literal(uint32_t v) { put((uint8_t) v); }
	void match(uint32_t len, uint32_t dist)
	{
		// behind the slot's end only the count goes on (a source at or behind cap was never written)
		for (uint32_t i = 0; i < len; i++)
			put(n - dist < cap ? out[n - dist] : 0);
	}
	void stored(uint64_t at, uint32_t m)
	{
		for (uint32_t i = 0; i < m; i++)
			put(b.p[at + i]);
	}
};

} // namespace ifw

// One zlib stream on one host thread: comp[0 .. comp_len) into out[0 .. cap) (out may be NULL with cap 0: the count
// alone).  -> the status of include/press_hip.h 2zb; *out_len the inflated length when the stream is well formed to its
// end (OK, ROOM - nothing is written behind cap, and the Adler-32 is not judged), else UINT64_MAX.
inline uint8_t inflate_serial(const uint8_t *comp, uint64_t comp_len, uint8_t *out, uint64_t cap, uint64_t *out_len)
{
	*out_len = UINT64_MAX;
	if (comp_len >> 32)
		return ifw::REFUSED;
	ifw::SerialEnv e;
	e.b.p = comp;
	e.b.len = comp_len;
	e.out = out;
	e.cap = cap;
	uint32_t adler = 0;
	const uint8_t st = ifw::walk(e, &adler);
	if (st)
		return st;
	*out_len = e.n;
	if (!e.room)
		return ifw::ROOM;
	if (adler != (e.s2 << 16 | e.s1)) {
		*out_len = UINT64_MAX;
		return ifw::ADLER;
	}
	return ifw::OK;
}

} // namespace ph
