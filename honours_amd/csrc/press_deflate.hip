// press_deflate.hip - zlib streams of BLOW5 records, made on the device (include/press_hip.h section 2z; the serial model is
// tests/_deflate.py).  A record is pre | u64 length | signal | post; it is never put together: rec_byte yields byte i of
// record r from the side arena (pre, post), the length field's value, and the signal field where the press left it.
//
// The stream of a record: 78 01 | one final dynamic-Huffman block over literals, distance-1 matches for the zero runs
// and end-of-block | Adler-32 - or stored blocks where that is not longer.  A record is cut into units of DF_UNIT bytes, a
// wave each, a lane 16 bytes of it; a byte's token follows from its run's first and last position alone, so a unit needs
// of its neighbours only the zeros in front of it and behind it.
//   k_df_plan    one wave: per record its parts checked, its length, its units; the unit count
//   k_df_fill    per record: the record of every unit
//   k_df_lead    per unit: leading and trailing zeros, "all zero", the Adler partial sums
//   k_df_carry   per record, one wave: the zeros in front of and behind every unit, Adler-32
//   k_df_hist    per unit: the token counts in LDS, added to the record's 286 counters
//   k_df_tree    per record, one wave: code lengths (limit 15), canonical codes, the block header's bits, the bit count,
//                dynamic or stored, the exact length
//   k_df_layout  one wave: rec_off from the lengths, raw[]
//   k_df_count   per unit: its bits
//   k_df_place   per record, one wave: the units' first bits; the length field, 78 01, header, end-of-block, Adler-32
//   k_df_write   per unit: the codes through an LDS window into the image; a stored record's bytes and block headers
// The image is zeroed first and every shared dword of it is written with atomicOr, so no kernel depends on a neighbour.
// SIZES: plan .. tree.  BATCH: the sizes, then layout .. write.

#include <algorithm>

#include "press_host.h"
#include "press_wave.h"

namespace ph {

namespace {

constexpr uint32_t DF_UNIT = 1024;        // bytes of a record per wave
constexpr uint32_t DF_NSYM = 286;         // literal / length symbols
constexpr uint32_t DF_TAB = 288;          // words per record of the count and code tables
constexpr uint32_t DF_HDR = 72;           // words per record for the block header's bits (at most 74 + 287 * 7 bits)
constexpr uint32_t DF_MAXN = 320;         // symbols the tree builder takes: five a lane
constexpr uint32_t DF_WIN = 488;          // dwords of a writer's LDS window: DF_UNIT * 15 bits, a last match's 6 more, the ragged ends
__device__ const uint8_t DF_ORDER[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 }; // RFC 1951 3.2.7
constexpr uint32_t DF_STORED = 65535;     // bytes of a stored block
constexpr uint32_t DF_MATCH = 258;
constexpr uint32_t DF_EOB = 256;
constexpr uint32_t DF_MAX_RECORD = 0xFFFF0000u;
constexpr uint8_t DF_REFUSED = 0xFF;

struct DfRec {
	uint64_t pre_off, post_off, sig_off, lenfield;
	uint32_t pre_len, sig_len, post_len, m;
	uint32_t first_unit, nunits;
	uint32_t ok;    // the parts lie inside their arenas and the record is not too long
	uint32_t raw;   // stored blocks
	uint32_t adler, hbits;
	uint32_t eob;   // the end-of-block code as it is written | its length << 16
	uint32_t place; // the stream lies inside the image
	uint64_t tokbits;    // bits of all tokens, end-of-block included
	uint64_t stream_len;
};
static_assert(sizeof(DfRec) == 96, "DfRec");

struct DfCtl {
	uint32_t nunits, bad;
};

struct DfArgs {
	const uint8_t *side, *sig;
	const uint64_t *side_tab, *sig_off, *sig_len;
	uint64_t side_bytes, sig_bytes;
	uint32_t nrec, max_units;
	int signal_method;
	DfRec *rec;
	DfCtl *ctl;
	uint32_t *urec, *uinfo, *us1, *us2, *uzb, *uza, *ubits;
	uint64_t *ustart;
	uint32_t *hist, *code, *hdr;
	uint64_t *need;
	uint32_t *img;
	uint64_t cap;
	uint64_t *rec_off;
	uint8_t *raw;
};

// ------------------------------------------------------------------ a record's bytes

__device__ __forceinline__ uint32_t rec_byte(const DfArgs &a, const DfRec &R, uint32_t i)
{
	if (i < R.pre_len)
		return a.side[R.pre_off + i];
	i -= R.pre_len;
	if (i < 8)
		return (uint32_t) (R.lenfield >> (8 * i)) & 0xFFu;
	i -= 8;
	if (i < R.sig_len)
		return a.sig[R.sig_off + i];
	return a.side[R.post_off + (i - R.sig_len)];
}

__device__ __forceinline__ uint4 ld16_any(const uint8_t *p)
{
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	typedef u32x4 u32x4_u __attribute__((aligned(1)));
	const u32x4 v = *reinterpret_cast<const u32x4_u *>(p);
	return make_uint4(v.x, v.y, v.z, v.w);
}

// the nb bytes of the record from o on; the bytes behind them are 0xFF: not zero, they end a run
__device__ __forceinline__ void load16(const DfArgs &a, const DfRec &R, uint32_t o, uint32_t nb, uint32_t (&w)[4])
{
	w[0] = w[1] = w[2] = w[3] = 0xFFFFFFFFu;
	if (nb == 0)
		return;
	const uint32_t s0 = R.pre_len + 8;
	if (nb == 16 && o >= s0 && o + 16 <= s0 + R.sig_len) {
		const uint4 v = ld16_any(a.sig + R.sig_off + (o - s0));
		w[0] = v.x;
		w[1] = v.y;
		w[2] = v.z;
		w[3] = v.w;
		return;
	}
#pragma unroll
	for (uint32_t i = 0; i < 16; i++) {
		if (i < nb) {
			const uint32_t sh = 8 * (i & 3);
			w[i >> 2] = (w[i >> 2] & ~(0xFFu << sh)) | (rec_byte(a, R, o + i) << sh);
		}
	}
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[4], uint32_t i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xFFu; }

// bit i: byte i is zero
__device__ __forceinline__ uint32_t zero_mask(const uint32_t (&w)[4])
{
	uint32_t zm = 0;
#pragma unroll
	for (uint32_t i = 0; i < 16; i++)
		zm |= (byte_of(w, i) == 0 ? 1u : 0u) << i;
	return zm;
}

// Items in a row, one a lane, each `size` bytes: lead / trail = its leading / trailing zeros, allz = nothing but zeros
// (then it is `size` bytes long); cb / ca = the zeros in front of item 0 / behind item 63.  -> the zeros in front of and
// behind this lane's item.  An item that is cut short or missing is not allz and has lead = 0: it ends the run.
__device__ __forceinline__ void run_context(bool allz, uint32_t lead, uint32_t trail, uint32_t size, uint32_t cb, uint32_t ca,
					    uint32_t lane, uint32_t &zb, uint32_t &za)
{
	const uint64_t nz = __ballot(!allz);
	const uint64_t below = nz & ((1ull << lane) - 1ull);
	const uint64_t above = lane == 63 ? 0ull : nz & ~((2ull << lane) - 1ull);
	const uint32_t p = below ? 63u - (uint32_t) __clzll((long long) below) : 0u;
	const uint32_t q = above ? (uint32_t) __ffsll((unsigned long long) above) - 1u : 63u;
	const uint32_t tp = (uint32_t) __shfl((int) trail, (int) p, 64);
	const uint32_t lq = (uint32_t) __shfl((int) lead, (int) q, 64);
	zb = below ? tp + (lane - p - 1) * size : cb + lane * size;
	za = above ? lq + (q - lane - 1) * size : ca + (63 - lane) * size;
}

// a lane's 16 bytes: the mask of its zeros -> allz, lead, trail
__device__ __forceinline__ void lane_runs(uint32_t zm, bool &allz, uint32_t &lead, uint32_t &trail)
{
	const uint32_t nzm = ~zm & 0xFFFFu;
	allz = nzm == 0;
	lead = allz ? 16u : (uint32_t) __ffs((int) nzm) - 1u;
	trail = allz ? 16u : (uint32_t) __clz((int) nzm) - 16u;
}

// a match length 3 .. 258 -> its symbol, the number of extra bits, their value (RFC 1951 3.2.5)
__device__ __forceinline__ void length_code(uint32_t len, uint32_t &sym, uint32_t &ne, uint32_t &ev)
{
	if (len == DF_MATCH) {
		sym = 285;
		ne = 0;
		ev = 0;
		return;
	}
	const uint32_t l = len - 3;
	if (l < 8) {
		sym = 257 + l;
		ne = 0;
		ev = 0;
		return;
	}
	const uint32_t e = 29u - (uint32_t) __clz((int) l); // floor(log2 l) - 2
	sym = 261 + 4 * e + ((l >> e) & 3u);
	ne = e;
	ev = l & ((1u << e) - 1u);
}
__device__ __forceinline__ uint32_t length_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0u : (sym - 261) >> 2; }

// The tokens of a lane's nb bytes, in order: tok(symbol, bits behind the code, their value).  zb / za: the zeros in front of
// the lane's first byte and behind its last.  A zero at place j of its run, d zeros from it to the run's end (itself
// counted): j == 0 a literal; else with o = (j - 1) % 258: o == 0 opens a piece - a match of min(d, 258) where d >= 3, a
// literal where not -, o == 1 with d == 1 is the second literal of a two-byte tail, and every other byte lies in a match.
template <class F>
__device__ __forceinline__ void walk16(const uint32_t (&w)[4], uint32_t nb, uint32_t zm, uint32_t zb, uint32_t za, F &&tok)
{
	const uint32_t nzm = ~zm & 0xFFFFu;
#pragma unroll
	for (uint32_t i = 0; i < 16; i++) {
		const uint32_t b = byte_of(w, i);
		const uint32_t below = nzm & ((1u << i) - 1u);
		const uint32_t j = below ? i - (32u - (uint32_t) __clz((int) below)) : i + zb;
		const uint32_t above = nzm >> i;
		const uint32_t d = above ? (uint32_t) __ffs((int) above) - 1u : 16u - i + za;
		const uint32_t o = j ? (j - 1) % DF_MATCH : 0u;
		uint32_t sym = b, ne = 0, ev = 0;
		bool emit = i < nb;
		if (b == 0 && j != 0) {
			if (o == 0 && d >= 3) {
				length_code(d < DF_MATCH ? d : DF_MATCH, sym, ne, ev);
				ne++; // (the distance code: one zero bit)
			} else {
				emit = emit && (o == 0 || (o == 1 && d == 1));
			}
		}
		if (emit)
			tok(sym, ne, ev);
	}
}

struct Unit {
	uint32_t u, r;
	uint32_t o;  // the unit's first byte in the record
	uint32_t n;  // its bytes
	uint32_t lo; // the lane's first byte in the record
	uint32_t nb; // the lane's bytes
};

// the wave's unit and its record; false: none
__device__ __forceinline__ bool unit_of(const DfArgs &a, Unit &x, DfRec &R)
{
	const uint32_t lane = threadIdx.x & 63;
	x.u = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (x.u >= uni(a.ctl->nunits))
		return false;
	x.r = uni(a.urec[x.u]);
	R = a.rec[x.r];
	x.o = (x.u - R.first_unit) * DF_UNIT;
	x.n = R.m - x.o < DF_UNIT ? R.m - x.o : DF_UNIT;
	x.lo = x.o + lane * 16;
	x.nb = lane * 16 >= x.n ? 0u : (x.n - lane * 16 < 16 ? x.n - lane * 16 : 16u);
	return true;
}

// the lane's bytes, their zero mask, and the zeros in front of and behind them
__device__ __forceinline__ void unit_bytes(const DfArgs &a, const Unit &x, const DfRec &R, uint32_t (&w)[4], uint32_t &zm, uint32_t &zb,
					   uint32_t &za)
{
	const uint32_t lane = threadIdx.x & 63;
	load16(a, R, x.lo, x.nb, w);
	zm = zero_mask(w);
	bool allz;
	uint32_t lead, trail;
	lane_runs(zm, allz, lead, trail);
	run_context(allz, lead, trail, 16, a.uzb[x.u], a.uza[x.u], lane, zb, za);
}

// OR `n` bits (at most 32) into the image at bit p
__device__ __forceinline__ void or_bits(uint32_t *img, uint64_t p, uint32_t v, uint32_t n)
{
	const uint32_t sh = (uint32_t) p & 31u;
	if (v << sh)
		atomicOr(img + (p >> 5), v << sh);
	if (sh + n > 32 && (v >> (32 - sh)))
		atomicOr(img + (p >> 5) + 1, v >> (32 - sh));
}
__device__ __forceinline__ void or_byte(uint32_t *img, uint64_t at, uint32_t v)
{
	if (v)
		atomicOr(img + (at >> 2), v << (8 * ((uint32_t) at & 3u)));
}

// ------------------------------------------------------------------ the tree of one record (a wave)

struct TreeLds {
	uint32_t org[DF_MAXN];     // the counts as given
	uint32_t cnt[2 * DF_MAXN]; // the nodes' counts: the leaves (the symbols), from DF_MAXN on the parents as they are made
	uint16_t par[2 * DF_MAXN];
	uint16_t lst[DF_MAXN];     // the list, ascending by count
	uint8_t len[DF_MAXN];
};

// Code lengths of the symbols below n (at most DF_MAXN) that have a count in t.org, into t.len; lane l owns the symbols
// 5 l .. 5 l + 4.  The list ascending by (count, symbol); the first two nodes become a parent with the sum of their counts,
// which goes back in front of the first remaining node whose count is not smaller; a symbol's length is its depth, one
// symbol alone has length 1.  A length beyond `limit`: again from max(1, c >> k), k = 1, 2, ...  -> k
__device__ uint32_t build_lengths(TreeLds &t, uint32_t n, uint32_t limit, uint32_t lane)
{
	for (uint32_t k = 0;; k++) {
		uint32_t c[5], nsym = 0;
#pragma unroll
		for (uint32_t j = 0; j < 5; j++) {
			const uint32_t sym = lane * 5 + j;
			c[j] = sym < n ? t.org[sym] : 0u;
			if (c[j]) {
				c[j] >>= k;
				c[j] = c[j] ? c[j] : 1u;
			}
			t.cnt[sym] = c[j];
			nsym += (uint32_t) __popcll(__ballot(c[j] != 0));
		}
		wave_lds_sync();
#pragma unroll 1
		for (uint32_t j = 0; j < 5; j++) {
			if (!c[j])
				continue;
			const uint32_t sym = lane * 5 + j;
			uint32_t rank = 0;
			for (uint32_t s = 0; s < n; s++) {
				const uint32_t cs = t.cnt[s];
				rank += (cs != 0 && (cs < c[j] || (cs == c[j] && s < sym))) ? 1u : 0u;
			}
			t.lst[rank] = (uint16_t) sym;
		}
		wave_lds_sync();
		uint32_t head = 0;
		for (uint32_t step = 0; head + 1 < nsym; step++) {
			const uint32_t m1 = t.lst[head], m2 = t.lst[head + 1];
			const uint32_t pc = t.cnt[m1] + t.cnt[m2];
			const uint32_t pid = DF_MAXN + step;
			uint32_t pos = 0; // nodes behind the two with a smaller count than the parent: it goes behind them
			for (uint32_t base = head + 2; base < nsym; base += 64) {
				const uint32_t i = base + lane;
				const bool lt = i < nsym && t.cnt[t.lst[i]] < pc;
				const uint32_t cnt = (uint32_t) __popcll(__ballot(lt));
				pos += cnt;
				if (cnt < 64)
					break;
			}
			for (uint32_t base = 0; base < pos; base += 64) { // they move down one place
				const uint32_t i = base + lane;
				const uint16_t v = i < pos ? t.lst[head + 2 + i] : (uint16_t) 0;
				wave_lds_sync();
				if (i < pos)
					t.lst[head + 1 + i] = v;
				wave_lds_sync();
			}
			if (lane == 0) {
				t.lst[head + 1 + pos] = (uint16_t) pid;
				t.cnt[pid] = pc;
				t.par[m1] = (uint16_t) pid;
				t.par[m2] = (uint16_t) pid;
			}
			wave_lds_sync();
			head++;
		}
		const uint32_t root = nsym ? t.lst[head] : 0u;
		uint32_t maxlen = 0;
#pragma unroll 1
		for (uint32_t j = 0; j < 5; j++) {
			uint32_t l = 0;
			if (c[j]) {
				uint32_t node = lane * 5 + j;
				while (node != root) {
					node = t.par[node];
					l++;
				}
				l = l ? l : 1u;
			}
			t.len[lane * 5 + j] = (uint8_t) (l < 255 ? l : 255u);
			maxlen = l > maxlen ? l : maxlen;
		}
		maxlen = max32(maxlen);
		wave_lds_sync();
		if (maxlen <= limit)
			return k;
	}
}

} // namespace

// ------------------------------------------------------------------ the kernels

__global__ __launch_bounds__(64) void k_df_plan(DfArgs a)
{
	const uint32_t lane = threadIdx.x;
	uint64_t carry = 0;
	for (uint32_t base = 0; base < a.nrec; base += 64) {
		const uint32_t r = base + lane;
		uint64_t nu = 0;
		DfRec R = {};
		if (r < a.nrec) {
			const uint64_t po = a.side_tab[4 * (size_t) r], pl = a.side_tab[4 * (size_t) r + 1];
			const uint64_t qo = a.side_tab[4 * (size_t) r + 2], ql = a.side_tab[4 * (size_t) r + 3];
			const uint64_t so = a.sig_off[r], sl = a.sig_len[r];
			bool ok = pl <= a.side_bytes && po <= a.side_bytes - pl && ql <= a.side_bytes && qo <= a.side_bytes - ql &&
				  sl <= a.sig_bytes && so <= a.sig_bytes - sl;
			ok = ok && pl < DF_MAX_RECORD && ql < DF_MAX_RECORD && sl < DF_MAX_RECORD && pl + 8 + sl + ql < DF_MAX_RECORD;
			if (ok) {
				R.pre_off = po;
				R.post_off = qo;
				R.sig_off = so;
				R.lenfield = a.signal_method ? sl : sl / 2;
				R.pre_len = (uint32_t) pl;
				R.sig_len = (uint32_t) sl;
				R.post_len = (uint32_t) ql;
				R.m = (uint32_t) (pl + 8 + sl + ql);
				R.nunits = (R.m + DF_UNIT - 1) / DF_UNIT;
				R.ok = 1;
				nu = R.nunits;
			}
		}
		const uint64_t inc = wave_incl_scan64(nu, lane);
		if (r < a.nrec) {
			const uint64_t first = carry + inc - nu;
			R.first_unit = first < 0xFFFFFFFFull ? (uint32_t) first : 0xFFFFFFFFu;
			a.rec[r] = R;
		}
		carry += __shfl(inc, 63, 64);
	}
	if (lane == 0) {
		const bool bad = carry > a.max_units;
		a.ctl->nunits = bad ? 0u : (uint32_t) carry;
		a.ctl->bad = bad ? 1u : 0u;
	}
}

__global__ __launch_bounds__(64) void k_df_fill(DfArgs a)
{
	if (uni(a.ctl->bad))
		return;
	const uint32_t r = blockIdx.x;
	const uint32_t first = uni(a.rec[r].first_unit), nu = uni(a.rec[r].nunits);
	for (uint32_t i = threadIdx.x; i < nu; i += 64)
		a.urec[first + i] = r;
}

__global__ __launch_bounds__(256) void k_df_lead(DfArgs a)
{
	const uint32_t lane = threadIdx.x & 63;
	Unit x;
	DfRec R;
	if (!unit_of(a, x, R))
		return;
	uint32_t w[4];
	load16(a, R, x.lo, x.nb, w);
	const uint32_t zm = zero_mask(w);
	bool allz;
	uint32_t lead, trail;
	lane_runs(zm, allz, lead, trail);
	uint32_t s1 = 0, s2 = 0;
#pragma unroll
	for (uint32_t i = 0; i < 16; i++) {
		const uint32_t b = i < x.nb ? byte_of(w, i) : 0u;
		s1 += b;
		s2 += b * (lane * 16 + i);
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		s1 += (uint32_t) __shfl_xor((int) s1, d, 64);
		s2 += (uint32_t) __shfl_xor((int) s2, d, 64);
	}
	const uint64_t nz = __ballot(!allz);
	const uint32_t f = nz ? (uint32_t) __ffsll((unsigned long long) nz) - 1u : 0u;
	const uint32_t l = nz ? 63u - (uint32_t) __clzll((long long) nz) : 0u;
	const uint32_t lf = (uint32_t) __shfl((int) lead, (int) f, 64), tl = (uint32_t) __shfl((int) trail, (int) l, 64);
	if (lane == 0) {
		const uint32_t ulead = nz ? f * 16 + lf : DF_UNIT, utrail = nz ? tl + (63 - l) * 16 : DF_UNIT;
		a.uinfo[x.u] = ulead | (utrail << 11) | (nz ? 0u : 1u << 22);
		a.us1[x.u] = s1;
		a.us2[x.u] = s2;
	}
}

__global__ __launch_bounds__(64) void k_df_carry(DfArgs a)
{
	if (uni(a.ctl->bad))
		return;
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	DfRec *R = a.rec + r;
	if (!uni(R->ok))
		return;
	const uint32_t first = uni(R->first_unit), nu = uni(R->nunits), m = uni(R->m);
	// forwards: the zeros in front of every unit; and the Adler sums
	uint32_t cb = 0;
	uint64_t sa = 0, sb = 0;
	for (uint32_t base = 0; base < nu; base += 64) {
		const uint32_t i = base + lane;
		const uint32_t info = i < nu ? a.uinfo[first + i] : 0u;
		const bool allz = (info >> 22) & 1u;
		const uint32_t trail = (info >> 11) & 0x7FFu;
		uint32_t zb, za;
		run_context(allz, 0u, trail, DF_UNIT, cb, 0u, lane, zb, za);
		if (i < nu) {
			a.uzb[first + i] = zb;
			const uint64_t s1 = a.us1[first + i], s2 = a.us2[first + i];
			sa += s1;
			sb += ((uint64_t) (m - i * DF_UNIT) * s1 - s2) % 65521u; // byte j of the unit counts m - (o + j) times
		}
		const uint64_t nz = __ballot(!allz);
		const uint32_t l = nz ? 63u - (uint32_t) __clzll((long long) nz) : 0u;
		const uint32_t tl = (uint32_t) __shfl((int) trail, (int) l, 64);
		cb = nz ? tl + (63 - l) * DF_UNIT : cb + 64 * DF_UNIT;
	}
	// backwards: the zeros behind every unit
	uint32_t ca = 0;
	for (uint32_t base = (nu - 1) / 64 * 64;; base -= 64) {
		const uint32_t i = base + lane;
		const uint32_t info = i < nu ? a.uinfo[first + i] : 0u;
		const bool allz = (info >> 22) & 1u;
		const uint32_t lead = info & 0x7FFu;
		uint32_t zb, za;
		run_context(allz, lead, 0u, DF_UNIT, 0u, ca, lane, zb, za);
		if (i < nu)
			a.uza[first + i] = za;
		const uint64_t nz = __ballot(!allz);
		const uint32_t f = nz ? (uint32_t) __ffsll((unsigned long long) nz) - 1u : 0u;
		const uint32_t lf = (uint32_t) __shfl((int) lead, (int) f, 64);
		ca = nz ? lf + f * DF_UNIT : ca + 64 * DF_UNIT;
		if (base == 0)
			break;
	}
	sa = sum64(sa);
	sb = sum64(sb);
	if (lane == 0)
		R->adler = (uint32_t) ((1 + sa) % 65521u) | ((uint32_t) ((m + sb) % 65521u) << 16);
}

__global__ __launch_bounds__(256) void k_df_hist(DfArgs a)
{
	__shared__ uint32_t s_h[4][DF_TAB];
	const uint32_t lane = threadIdx.x & 63;
	uint32_t *h = s_h[threadIdx.x >> 6];
	Unit x;
	DfRec R;
	if (!unit_of(a, x, R))
		return;
	for (uint32_t i = lane; i < DF_TAB; i += 64)
		h[i] = 0;
	wave_lds_sync();
	uint32_t w[4], zm, zb, za;
	unit_bytes(a, x, R, w, zm, zb, za);
	walk16(w, x.nb, zm, zb, za, [&](uint32_t sym, uint32_t, uint32_t) { atomicAdd(&h[sym], 1u); });
	wave_lds_sync();
	uint32_t *g = a.hist + (size_t) x.r * DF_TAB;
	for (uint32_t i = lane; i < DF_NSYM; i += 64) {
		const uint32_t c = h[i];
		if (c)
			atomicAdd(&g[i], c);
	}
}

__global__ __launch_bounds__(64) void k_df_tree(DfArgs a)
{
	__shared__ TreeLds t;
	__shared__ uint16_t s_cls[DF_MAXN]; // the code-length sequence: symbol | extra value << 8
	__shared__ uint32_t s_blc[16], s_next[16], s_hdr[DF_HDR], s_clc[20], s_misc[4];
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	DfRec *R = a.rec + r;
	if (uni(a.ctl->bad) || !uni(R->ok)) {
		if (lane == 0) {
			R->ok = 0;
			a.need[r] = PRESS_HIP_FAILED;
		}
		return;
	}
	const uint32_t m = uni(R->m);
	const uint32_t *hist = a.hist + (size_t) r * DF_TAB;
	uint32_t c[5];
#pragma unroll
	for (uint32_t j = 0; j < 5; j++) {
		const uint32_t sym = lane * 5 + j;
		c[j] = sym < DF_NSYM ? hist[sym] : 0u;
		if (sym == DF_EOB)
			c[j] = 1;
		t.org[sym] = c[j];
	}
	if (lane < 16)
		s_blc[lane] = 0;
	for (uint32_t i = lane; i < DF_HDR; i += 64)
		s_hdr[i] = 0;
	wave_lds_sync();
	build_lengths(t, DF_NSYM, 15, lane);
	// canonical codes (RFC 1951 3.2.2), kept as they are written: the first bit lowest
	uint32_t len[5];
#pragma unroll
	for (uint32_t j = 0; j < 5; j++) {
		len[j] = t.len[lane * 5 + j];
		if (len[j])
			atomicAdd(&s_blc[len[j]], 1u);
	}
	wave_lds_sync();
	if (lane == 0) {
		uint32_t code = 0;
		s_next[0] = 0;
		for (uint32_t b = 1; b < 16; b++) {
			code = (code + (b > 1 ? s_blc[b - 1] : 0u)) << 1;
			s_next[b] = code;
		}
	}
	wave_lds_sync();
	uint32_t *codes = a.code + (size_t) r * DF_TAB;
	uint64_t tokbits = 0;
	uint32_t top = 0;
#pragma unroll 1
	for (uint32_t j = 0; j < 5; j++) {
		const uint32_t sym = lane * 5 + j;
		uint32_t cw = 0;
		if (len[j]) {
			uint32_t rank = 0;
			for (uint32_t s = 0; s < sym; s++)
				rank += t.len[s] == len[j] ? 1u : 0u;
			cw = (__brev(s_next[len[j]] + rank) >> (32 - len[j])) | (len[j] << 16);
			tokbits += (uint64_t) c[j] * (len[j] + (sym > DF_EOB ? length_extra(sym) + 1u : 0u));
			top = sym;
			if (sym == DF_EOB)
				R->eob = cw;
		}
		if (sym < DF_TAB)
			codes[sym] = cw;
	}
	tokbits = sum64(tokbits);
	const uint32_t nlit = max32(top) < 256 ? 257u : max32(top) + 1u;
	wave_lds_sync();
	// the code-length sequence of the nlit lengths and the one distance length, by one lane; the counts of its symbols
	for (uint32_t i = lane; i < DF_MAXN; i += 64)
		t.org[i] = 0;
	wave_lds_sync();
	if (lane == 0) {
		t.len[nlit] = 1;
		const uint32_t nseq = nlit + 1;
		uint32_t ncls = 0;
		for (uint32_t i = 0; i < nseq;) {
			const uint32_t v = t.len[i];
			uint32_t e = i + 1;
			while (e < nseq && t.len[e] == v)
				e++;
			uint32_t run = e - i;
			if (v == 0) {
				while (run >= 11) {
					const uint32_t n = run < 138 ? run : 138u;
					s_cls[ncls++] = (uint16_t) (18u | ((n - 11) << 8));
					t.org[18]++;
					run -= n;
				}
				if (run >= 3) {
					s_cls[ncls++] = (uint16_t) (17u | ((run - 3) << 8));
					t.org[17]++;
					run = 0;
				}
			} else {
				s_cls[ncls++] = (uint16_t) v;
				t.org[v]++;
				run--;
				while (run >= 3) {
					const uint32_t n = run < 6 ? run : 6u;
					s_cls[ncls++] = (uint16_t) (16u | ((n - 3) << 8));
					t.org[16]++;
					run -= n;
				}
			}
			for (; run; run--) {
				s_cls[ncls++] = (uint16_t) v;
				t.org[v]++;
			}
			i = e;
		}
		s_misc[0] = ncls;
	}
	wave_lds_sync();
	build_lengths(t, 19, 7, lane);
	if (lane == 0) {
		const uint32_t ncls = s_misc[0];
		const uint8_t *order = DF_ORDER;
		for (uint32_t b = 0; b < 8; b++)
			s_blc[b] = 0;
		for (uint32_t s = 0; s < 19; s++)
			s_blc[t.len[s] & 7u]++;
		s_blc[0] = 0;
		uint32_t code = 0;
		s_next[0] = 0;
		for (uint32_t b = 1; b < 8; b++) {
			code = (code + s_blc[b - 1]) << 1;
			s_next[b] = code;
		}
		for (uint32_t s = 0; s < 19; s++) {
			const uint32_t l = t.len[s];
			s_clc[s] = l ? (__brev(s_next[l]) >> (32 - l)) | (l << 8) : 0u;
			if (l)
				s_next[l]++;
		}
		uint32_t ncl = 4;
		for (uint32_t i = 4; i < 19; i++)
			if (t.len[order[i]])
				ncl = i + 1;
		uint32_t p = 0;
		auto put = [&](uint32_t v, uint32_t n) {
			const uint32_t sh = p & 31u;
			s_hdr[p >> 5] |= v << sh;
			if (sh + n > 32)
				s_hdr[(p >> 5) + 1] |= v >> (32 - sh);
			p += n;
		};
		put(1, 1);
		put(2, 2);
		put(nlit - 257, 5);
		put(0, 5);
		put(ncl - 4, 4);
		for (uint32_t i = 0; i < ncl; i++)
			put(t.len[order[i]], 3);
		for (uint32_t i = 0; i < ncls; i++) {
			const uint32_t e = s_cls[i], s = e & 0xFFu, cw = s_clc[s];
			put(cw & 0xFFu, cw >> 8);
			if (s >= 16)
				put(e >> 8, s == 16 ? 2u : s == 17 ? 3u : 7u);
		}
		s_misc[1] = p;
	}
	wave_lds_sync();
	const uint32_t hbits = s_misc[1];
	uint32_t *hdr = a.hdr + (size_t) r * DF_HDR;
	for (uint32_t i = lane; i < DF_HDR; i += 64)
		hdr[i] = s_hdr[i];
	if (lane)
		return;
	const uint64_t dyn = (hbits + tokbits + 7) / 8;
	const uint64_t stored = (uint64_t) m + 5ull * (m ? (m + DF_STORED - 1) / DF_STORED : 1u);
	const bool raw = dyn >= stored;
	R->raw = raw ? 1u : 0u;
	R->hbits = hbits;
	R->tokbits = tokbits;
	R->stream_len = 2 + (raw ? stored : dyn) + 4;
	a.need[r] = 8 + R->stream_len;
}

__global__ __launch_bounds__(64) void k_df_layout(DfArgs a)
{
	const uint32_t lane = threadIdx.x;
	uint64_t carry = 0;
	for (uint32_t base = 0; base < a.nrec; base += 64) {
		const uint32_t r = base + lane;
		const bool ok = r < a.nrec && a.rec[r].ok;
		const uint64_t n = ok ? a.need[r] : 0ull;
		const uint64_t inc = wave_incl_scan64(n, lane);
		if (r < a.nrec) {
			const uint64_t at = carry + inc - n;
			const bool fits = ok && at + n <= a.cap;
			a.rec_off[r] = at;
			a.rec[r].place = fits ? 1u : 0u;
			a.raw[r] = fits ? (uint8_t) a.rec[r].raw : DF_REFUSED;
		}
		carry += __shfl(inc, 63, 64);
	}
	if (lane == 0)
		a.rec_off[a.nrec] = carry;
}

__global__ __launch_bounds__(256) void k_df_count(DfArgs a)
{
	__shared__ uint8_t s_len[4][DF_TAB];
	const uint32_t lane = threadIdx.x & 63;
	uint8_t *ln = s_len[threadIdx.x >> 6];
	Unit x;
	DfRec R;
	if (!unit_of(a, x, R))
		return;
	if (!R.place || R.raw)
		return;
	const uint32_t *codes = a.code + (size_t) x.r * DF_TAB;
	for (uint32_t i = lane; i < DF_TAB; i += 64)
		ln[i] = (uint8_t) (codes[i] >> 16);
	wave_lds_sync();
	uint32_t w[4], zm, zb, za;
	unit_bytes(a, x, R, w, zm, zb, za);
	uint32_t bits = 0;
	walk16(w, x.nb, zm, zb, za, [&](uint32_t sym, uint32_t ne, uint32_t) { bits += ln[sym] + ne; });
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		bits += (uint32_t) __shfl_xor((int) bits, d, 64);
	if (lane == 0)
		a.ubits[x.u] = bits;
}

__global__ __launch_bounds__(64) void k_df_place(DfArgs a)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const DfRec *R = a.rec + r;
	if (!uni(R->ok) || !uni(R->place))
		return;
	const uint64_t at = a.rec_off[r];
	const uint64_t slen = R->stream_len;
	const uint32_t adler = uni(R->adler);
	if (lane < 8)
		or_byte(a.img, at + lane, (uint32_t) (slen >> (8 * lane)) & 0xFFu);
	if (lane == 8)
		or_byte(a.img, at + 8, 0x78u);
	if (lane == 9)
		or_byte(a.img, at + 9, 0x01u);
	if (lane >= 10 && lane < 14)
		or_byte(a.img, at + 8 + slen - 4 + (lane - 10), (adler >> (8 * (13 - lane))) & 0xFFu);
	if (uni(R->raw))
		return;
	const uint32_t hbits = uni(R->hbits), first = uni(R->first_unit), nu = uni(R->nunits);
	const uint64_t p0 = (at + 10) * 8;
	const uint32_t *hdr = a.hdr + (size_t) r * DF_HDR;
	for (uint32_t i = lane; i * 32 < hbits; i += 64)
		or_bits(a.img, p0 + 32ull * i, hdr[i], hbits - 32 * i < 32 ? hbits - 32 * i : 32u);
	uint64_t carry = p0 + hbits;
	for (uint32_t base = 0; base < nu; base += 64) {
		const uint32_t i = base + lane;
		const uint64_t b = i < nu ? a.ubits[first + i] : 0ull;
		const uint64_t inc = wave_incl_scan64(b, lane);
		if (i < nu)
			a.ustart[first + i] = carry + inc - b;
		carry += __shfl(inc, 63, 64);
	}
	if (lane == 0)
		or_bits(a.img, carry, R->eob & 0xFFFFu, R->eob >> 16);
}

__global__ __launch_bounds__(256) void k_df_write(DfArgs a)
{
	__shared__ uint32_t s_win[4][DF_WIN];
	__shared__ uint32_t s_code[4][DF_TAB];
	const uint32_t lane = threadIdx.x & 63;
	uint32_t *win = s_win[threadIdx.x >> 6], *code = s_code[threadIdx.x >> 6];
	Unit x;
	DfRec R;
	if (!unit_of(a, x, R))
		return;
	if (!R.place)
		return;
	if (R.raw) { // stored blocks: 78 01 | per block { final, len, ~len } and its bytes
		const uint64_t body = a.rec_off[x.r] + 10;
		const uint32_t nblk = (R.m + DF_STORED - 1) / DF_STORED;
		for (uint32_t i = 0; i < x.nb; i++) {
			const uint32_t pos = x.lo + i, blk = pos / DF_STORED;
			const uint64_t dst = body + 5ull * (blk + 1) + pos;
			if (pos % DF_STORED == 0) {
				const uint32_t len = R.m - pos < DF_STORED ? R.m - pos : DF_STORED;
				or_byte(a.img, dst - 5, blk == nblk - 1 ? 1u : 0u);
				or_byte(a.img, dst - 4, len & 0xFFu);
				or_byte(a.img, dst - 3, len >> 8);
				or_byte(a.img, dst - 2, ~len & 0xFFu);
				or_byte(a.img, dst - 1, (~len >> 8) & 0xFFu);
			}
			or_byte(a.img, dst, rec_byte(a, R, pos));
		}
		return;
	}
	const uint32_t *codes = a.code + (size_t) x.r * DF_TAB;
	for (uint32_t i = lane; i < DF_TAB; i += 64)
		code[i] = codes[i];
	const uint64_t p0 = a.ustart[x.u];
	const uint32_t nbits = uni(a.ubits[x.u]), off = (uint32_t) p0 & 31u;
	const uint32_t ndw = (off + nbits + 31) >> 5;
	for (uint32_t i = lane; i < ndw + 1 && i < DF_WIN; i += 64)
		win[i] = 0;
	wave_lds_sync();
	uint32_t w[4], zm, zb, za;
	unit_bytes(a, x, R, w, zm, zb, za);
	uint32_t bits = 0;
	walk16(w, x.nb, zm, zb, za, [&](uint32_t sym, uint32_t ne, uint32_t) { bits += (code[sym] >> 16) + ne; });
	uint32_t p = off + scan32(bits, lane) - bits;
	walk16(w, x.nb, zm, zb, za, [&](uint32_t sym, uint32_t ne, uint32_t ev) {
		const uint32_t cw = code[sym], l = cw >> 16;
		const uint32_t v = (cw & 0xFFFFu) | (ev << l), n = l + ne; // at most 21 bits
		const uint32_t sh = p & 31u;
		atomicOr(&win[p >> 5], v << sh);
		if (sh + n > 32)
			atomicOr(&win[(p >> 5) + 1], v >> (32 - sh));
		p += n;
	});
	wave_lds_sync();
	uint32_t *dst = a.img + (p0 >> 5);
	for (uint32_t i = lane; i < ndw; i += 64) {
		const uint32_t v = win[i];
		if (i == 0 || i == ndw - 1) { // shared with the neighbours
			if (v)
				atomicOr(dst + i, v);
		} else {
			dst[i] = v;
		}
	}
}

// ------------------------------------------------------------------ the host side

namespace {

uint32_t df_max_units(uint64_t record_bytes, uint32_t nrec) { return (uint32_t) std::min<uint64_t>(record_bytes / DF_UNIT + nrec, 0xFFFFFF00u); }
size_t df_unit_bytes(uint32_t max_units) { return ((size_t) max_units + 8) * (7 * 4 + 8); }
size_t df_rec_bytes(uint32_t nrec) { return (size_t) nrec * sizeof(DfRec) + 64; }
size_t df_tab_bytes(uint32_t nrec) { return (size_t) nrec * (2 * DF_TAB + DF_HDR) * 4; }

int df_bind(DfArgs &a, uint64_t record_bytes)
{
	a.max_units = df_max_units(record_bytes, a.nrec);
	if (g.df_rec.reserve(df_rec_bytes(a.nrec)) || g.df_unit.reserve(df_unit_bytes(a.max_units)) || g.df_tab.reserve(df_tab_bytes(a.nrec)) ||
	    g.df_need.reserve(((size_t) a.nrec + 1) * 8))
		return PRESS_HIP_EHIP;
	a.ctl = (DfCtl *) g.df_rec.p;
	a.rec = (DfRec *) ((uint8_t *) g.df_rec.p + 64);
	const size_t mu = (size_t) a.max_units + 8;
	a.ustart = (uint64_t *) g.df_unit.p;
	a.urec = (uint32_t *) (a.ustart + mu);
	a.uinfo = a.urec + mu;
	a.us1 = a.uinfo + mu;
	a.us2 = a.us1 + mu;
	a.uzb = a.us2 + mu;
	a.uza = a.uzb + mu;
	a.ubits = a.uza + mu;
	a.hist = (uint32_t *) g.df_tab.p;
	a.code = a.hist + (size_t) a.nrec * DF_TAB;
	a.hdr = a.code + (size_t) a.nrec * DF_TAB;
	return 0;
}

void df_launch_sizes(const DfArgs &a, hipStream_t s)
{
	const uint32_t grid = (a.max_units + 3) / 4;
	(void) hipMemsetAsync(a.hist, 0, (size_t) a.nrec * DF_TAB * 4, s);
	hipLaunchKernelGGL(k_df_plan, dim3(1), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_df_fill, dim3(a.nrec), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_df_lead, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_df_carry, dim3(a.nrec), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_df_hist, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_df_tree, dim3(a.nrec), dim3(64), 0, s, a);
}

// behind df_launch_sizes; zero: the bytes of the image to clear (a multiple of 4, at least what is written)
void df_launch_write(const DfArgs &a, uint64_t zero, hipStream_t s)
{
	const uint32_t grid = (a.max_units + 3) / 4;
	(void) hipMemsetAsync(a.img, 0, zero, s);
	hipLaunchKernelGGL(k_df_layout, dim3(1), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_df_count, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_df_place, dim3(a.nrec), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_df_write, dim3(grid), dim3(256), 0, s, a);
}

struct DfIn {
	const uint8_t *side;
	const uint64_t *side_tab;
	uint64_t side_bytes;
	const uint8_t *sig;
	const uint64_t *sig_off, *sig_len;
	uint64_t sig_bytes;
	uint32_t nrec;
	uint64_t record_bytes;
	int signal_method;
};

// image == NULL: the sizes alone, into need
int df_run(const DfIn &in, uint64_t *need, uint8_t *image, uint64_t image_cap, uint64_t *rec_off, uint8_t *raw, int device_resident)
{
	API_LOCK;
	const bool sizes = image == nullptr && rec_off == nullptr;
	if (in.signal_method < 0 || in.signal_method > 1)
		return set_error(PRESS_HIP_EARG, "signal_method = %d: 0 (int16 samples) or 1 (svb-zd)", in.signal_method);
	if (in.nrec && (!in.side_tab || !in.sig_off || !in.sig_len || (!in.side && in.side_bytes) || (!in.sig && in.sig_bytes)))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (sizes ? (in.nrec && !need) : (!rec_off || (in.nrec && !raw) || (!image && image_cap)))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (!sizes && device_resident && (((uintptr_t) image | image_cap) & 3))
		return set_error(PRESS_HIP_EARG, "the image and image_cap must be multiples of 4 bytes");
	if (int rc = ctx_init())
		return rc;
	const hipStream_t s = g.stream();
	if (in.nrec == 0) {
		if (sizes)
			return 0;
		if (device_resident)
			HIPCHK(hipMemsetAsync(rec_off, 0, 8, s));
		else
			rec_off[0] = 0;
		return 0;
	}
	DfArgs a = {};
	a.nrec = in.nrec;
	a.signal_method = in.signal_method;
	a.side_bytes = in.side_bytes;
	a.sig_bytes = in.sig_bytes;
	uint64_t record_bytes = in.record_bytes;
	if (!device_resident) { // the exact figure, and the tables' own check
		record_bytes = 0;
		for (uint32_t r = 0; r < in.nrec; r++) {
			const uint64_t pl = in.side_tab[4 * (size_t) r + 1], ql = in.side_tab[4 * (size_t) r + 3], sl = in.sig_len[r];
			if (pl >= DF_MAX_RECORD || ql >= DF_MAX_RECORD || sl >= DF_MAX_RECORD || pl + 8 + sl + ql >= DF_MAX_RECORD)
				return set_error(PRESS_HIP_EARG, "record %u is longer than %u bytes", r, DF_MAX_RECORD - 1);
			record_bytes += pl + 8 + sl + ql;
		}
	}
	if (record_bytes / DF_UNIT + in.nrec > 0xFFFFFF00ull)
		return set_error(PRESS_HIP_EARG, "record_bytes = %llu: too many for one call", (unsigned long long) record_bytes);
	if (int rc = df_bind(a, record_bytes))
		return rc;
	a.need = sizes && device_resident ? need : (uint64_t *) g.df_need.p;
	a.side = in.side;
	a.side_tab = in.side_tab;
	a.sig = in.sig;
	a.sig_off = in.sig_off;
	a.sig_len = in.sig_len;
	if (device_resident) {
		df_launch_sizes(a, s);
		if (sizes)
			return launch_status();
		a.img = (uint32_t *) image;
		a.cap = image_cap;
		a.rec_off = rec_off;
		a.raw = raw;
		df_launch_write(a, image_cap, s);
		return launch_status();
	}
	// host pointers: the arenas and tables go up, the sizes come back, the image is made at its exact size and comes back
	Staged st(in.nrec, s);
	const size_t n8 = (size_t) in.nrec * 8;
	if (g.df_side.reserve(in.side_bytes + 16) || g.df_sig.reserve(in.sig_bytes + 16) || g.df_tabs.reserve(6 * n8) ||
	    g.df_out.reserve(n8 + 8 + in.nrec + 8))
		return PRESS_HIP_EHIP;
	int rc;
	uint64_t *tabs = (uint64_t *) g.df_tabs.p;
	if ((rc = st.push(g.df_side.p, in.side, in.side_bytes)) || (rc = st.push(g.df_sig.p, in.sig, in.sig_bytes)) ||
	    (rc = st.push(tabs, in.side_tab, 4 * n8)) || (rc = st.push(tabs + 4 * (size_t) in.nrec, in.sig_off, n8)) ||
	    (rc = st.push(tabs + 5 * (size_t) in.nrec, in.sig_len, n8)))
		return rc;
	a.side = (const uint8_t *) g.df_side.p;
	a.sig = (const uint8_t *) g.df_sig.p;
	a.side_tab = tabs;
	a.sig_off = tabs + 4 * (size_t) in.nrec;
	a.sig_len = tabs + 5 * (size_t) in.nrec;
	a.need = (uint64_t *) g.df_need.p;
	df_launch_sizes(a, s);
	if ((rc = launch_status()))
		return rc;
	std::vector<uint64_t> hneed(in.nrec);
	if ((rc = st.fetch_tables({ { hneed.data(), g.df_need.p, n8 } })))
		return rc;
	if (sizes) {
		memcpy(need, hneed.data(), n8);
		return 0;
	}
	uint64_t total = 0;
	for (uint32_t r = 0; r < in.nrec; r++)
		total += hneed[r] == PRESS_HIP_FAILED ? 0 : hneed[r];
	const uint64_t room = total < image_cap ? total : image_cap;
	const uint64_t zero = (room + 3) & ~3ull;
	if (g.df_img.reserve(zero + 16))
		return PRESS_HIP_EHIP;
	a.img = (uint32_t *) g.df_img.p;
	a.cap = room;
	a.rec_off = (uint64_t *) g.df_out.p;
	a.raw = (uint8_t *) g.df_out.p + n8 + 8;
	df_launch_write(a, zero, s);
	if ((rc = launch_status()) || (rc = st.fetch_prefix(image, g.df_img.p, room)))
		return rc;
	return st.fetch_tables({ { rec_off, a.rec_off, n8 + 8 }, { raw, a.raw, in.nrec } });
}

} // namespace

} // namespace ph

using namespace ph;

extern "C" int press_hip_blow5_deflate_sizes(const uint8_t *side, const uint64_t *side_tab, uint64_t side_bytes, const uint8_t *sig,
					     const uint64_t *sig_off, const uint64_t *sig_len, uint64_t sig_bytes, uint32_t nrec,
					     uint64_t record_bytes, int signal_method, uint64_t *need, int device_resident)
{
	const DfIn in = { side, side_tab, side_bytes, sig, sig_off, sig_len, sig_bytes, nrec, record_bytes, signal_method };
	return df_run(in, need, nullptr, 0, nullptr, nullptr, device_resident);
}

extern "C" int press_hip_blow5_deflate_batch(const uint8_t *side, const uint64_t *side_tab, uint64_t side_bytes, const uint8_t *sig,
					     const uint64_t *sig_off, const uint64_t *sig_len, uint64_t sig_bytes, uint32_t nrec,
					     uint64_t record_bytes, int signal_method, uint8_t *image, uint64_t image_cap,
					     uint64_t *rec_off, uint8_t *raw, int device_resident)
{
	if (!rec_off)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	const DfIn in = { side, side_tab, side_bytes, sig, sig_off, sig_len, sig_bytes, nrec, record_bytes, signal_method };
	return df_run(in, nullptr, image, image_cap, rec_off, raw, device_resident);
}

extern "C" uint64_t press_hip_blow5_deflate_workspace_bytes(uint64_t record_bytes, uint32_t nrec)
{
	if (record_bytes / DF_UNIT + nrec > 0xFFFFFF00ull)
		return 0;
	return df_rec_bytes(nrec) + df_unit_bytes(df_max_units(record_bytes, nrec)) + df_tab_bytes(nrec) + ((uint64_t) nrec + 1) * 8;
}
