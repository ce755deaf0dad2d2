// press_rice.hip - entropy stage 6 of the exception-split methods: Golomb-Rice coding of the one-byte values
// (rice_press / rice_depress, press.c:4860-4978, as the reference's rice_*_zd methods call them).
//
// Payload (include/press_hip.h section 2u; pinned by tests/_rice.py and tests/golden/ref_rice.json):
//   bit i of the payload is bit i % 8, from the least significant, of byte i / 8;
//   bits 0, 1, 2 = k >> 2 & 1, k >> 1 & 1, k & 1; then per value x: x >> k one-bits, a zero bit, the low k bits of x
//   from the most significant down;
//   k = the smallest of 0 .. 7 that minimises sum((x >> k) + 1 + k), sums in 64 bits (no value: k = 0);
//   nbits = 3 + that sum, (nbits - 1) / 8 + 1 bytes, the bits behind nbits in the last byte zero.
// Decoder: k from the first three bits; per value the run of ones counted modulo 256 (however long it is), the zero
// bit, k bits; value = (uint8_t) ((q << k) | rem); bits behind the stream's end are zero, nothing outside the stream
// is read.
//
// PRESS.  A read's one-byte values (a.low_tmp, k_low_encode_chunked) are cut into UNITS of RICE_UNIT values, a wave
// each; unit i of a read is entry 32 * first_chunk + i of the unit tables (a chunk of CHUNK samples has room for 32).
//   k_rice_count   per unit the eight sums of x >> k
//   k_rice_pick    per read: the totals, k, nbits, the length and the slot check; the exclusive scan of the units'
//                  bits at the chosen k, so that every unit knows its first bit
//   k_rice_write   per unit: code lengths -> wave scan -> bit positions; the bits of 512 values are assembled in LDS
//                  (windows of 8192 bits: a unary run may be 255 bits long and a unit's span has no useful bound) and
//                  go out as whole dwords to a STAGED payload in scratch (a.ri_pay, dword aligned, zeroed by the
//                  launcher): the first and last dword of a span are shared with the neighbours and merged with
//                  atomic OR, the others are stored
//   k_rice_copy    staged payload -> the slot, behind the section, at whatever byte address that is
// PRESS SIZES (need != NULL): count and pick alone, nothing else is written.
//
// DEPRESS.  A Rice code with a given k is a prefix code: the plan of press_huffman.hip, with arithmetic in the place
// of the tables.  The payload is cut into SUBSEQUENCES of RICE_SUB bits, a lane each, RICE_DT of them a tile.
//   k_rice_dplan   per read: k, the subsequences worth decoding in parallel (those of the payload, at most what nlow
//                  values can take at nine bits each: a pressed payload never has more), the tile table
//   k_rice_sync    a lane guesses the first code of its subsequence by running up through the one in front, then
//                  decodes its own: record = { start, end, codes }, start and end relative to the subsequence's
//                  first bit / the next one's
//   k_rice_fix x 2 a lane whose start is not the end the subsequence in front recorded decodes again from that end
//   k_rice_check   per read the first subsequence whose start is still not that end (hmin); the tiles' code counts
//   k_rice_dscan   per read the exclusive scan of the tiles' counts
//   k_rice_emit    the subsequences in front of hmin: their records chain from bit 3, so they are the true ones;
//                  values to a.low from the true starts, up to nlow
//   k_rice_walk    per read, serially from where the chain ends (bit 3 if nothing settled), until nlow values are out;
//                  behind the stream's end every value is 0
// The number of launches is fixed.  Correctness never depends on synchronisation: a stream whose codes all have one
// length (a forged one can, a pressed one cannot) leaves hmin small and the walk does the work.  A run of more than
// RICE_RUNCAP ones makes sync and fix give the subsequence up (the walk reads it a dword per step), so no lane spends
// more than a bounded time on bits that are not its own.

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

namespace {

constexpr uint64_t RICE_FAIL64 = ~0ull;
constexpr uint32_t RICE_NONE = 0xFFFFFFFFu; // record: the subsequence was given up
constexpr uint32_t RICE_SAT = 0xFFFFFFFEu;  // ... and its end
constexpr uint32_t RICE_RUNCAP = 4096;
constexpr uint32_t RICE_WIN = 256; // dwords of a writer's LDS window

__device__ __forceinline__ uint32_t scan32(uint32_t v, uint32_t lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = (uint32_t) __shfl_up((int) v, d, 64);
		if (lane >= (uint32_t) d)
			v += o;
	}
	return v;
}

__device__ __forceinline__ uint64_t sum64(uint64_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v += __shfl_xor(v, d, 64);
	return v;
}

// the unit a wave works on: false if there is none
struct Unit {
	uint32_t r, u, cnt; // read, unit id, values
	uint64_t v0, soff;  // first value, the read's sample offset
};
__device__ __forceinline__ bool unit_of(const BatchArgs &a, uint32_t u, Unit &x)
{
	const uint32_t t = u / RICE_UPC;
	if (t >= uni(a.ctl->nchunks))
		return false;
	const ChunkDesc *d = a.chunks + t;
	x.r = uni(d->read);
	x.u = u;
	x.soff = uni64(d->sig_off);
	const ReadMeta *m = a.meta + x.r;
	if (uni(m->status))
		return false;
	const uint64_t nlow = (uint64_t) uni(d->n) - 1 - uni(m->nex);
	x.v0 = ((uint64_t) uni(d->j) * RICE_UPC + u % RICE_UPC) * RICE_UNIT;
	if (x.v0 >= nlow)
		return false;
	x.cnt = nlow - x.v0 < RICE_UNIT ? (uint32_t) (nlow - x.v0) : RICE_UNIT;
	return true;
}

// up to eight values of a unit from i on, one per byte of the result; nv: how many there are
__device__ __forceinline__ uint64_t load8(const uint8_t *in, uint32_t i, uint32_t cnt, uint32_t &nv)
{
	uint64_t v = 0;
	nv = i < cnt ? (cnt - i < 8 ? cnt - i : 8u) : 0u;
	if (nv == 8) {
		__builtin_memcpy(&v, in + i, 8); // (8-byte aligned: the read's offset and i are multiples of 8)
	} else {
		for (uint32_t j = 0; j < nv; j++)
			v |= (uint64_t) in[i + j] << (8 * j);
	}
	return v;
}

} // namespace

__global__ __launch_bounds__(256) void k_rice_count(BatchArgs a)
{
	const uint32_t lane = threadIdx.x & 63;
	Unit x;
	if (!unit_of(a, uni(blockIdx.x * 4 + (threadIdx.x >> 6)), x))
		return;
	const uint8_t *in = a.low_tmp + x.soff + x.v0;
	uint32_t s[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	for (uint32_t step = 0; step < RICE_UNIT; step += 512) {
		uint32_t nv;
		const uint64_t v = load8(in, step + lane * 8, x.cnt, nv);
		for (uint32_t j = 0; j < nv; j++) {
			const uint32_t b = (uint32_t) (v >> (8 * j)) & 0xFFu;
#pragma unroll
			for (int k = 0; k < 8; k++)
				s[k] += b >> k;
		}
	}
#pragma unroll
	for (int k = 0; k < 8; k++) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1)
			s[k] += (uint32_t) __shfl_xor((int) s[k], d, 64);
	}
	if (lane == 0) {
		uint32_t *o = a.ri_sum + (size_t) x.u * 8;
#pragma unroll
		for (int k = 0; k < 8; k++)
			o[k] = s[k];
	}
}

// One wave per read.  need == NULL: press (behind k_ex_section: out_len = FAILED and status != 0 for a read it
// refused); else sizes (behind k_ex_sizes, which left header + section in need[r], or FAILED).
__global__ __launch_bounds__(64) void k_rice_pick(BatchArgs a, uint64_t *need)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const ReadMeta *m = a.meta + r;
	const uint32_t n = a.nsamp[r];
	RiceRead *rd = a.ri_rd + r;
	const bool refused = n == 0 || (need ? need[r] == RICE_FAIL64 : m->status != 0);
	if (refused) {
		if (lane == 0) {
			rd->ok = 0;
			rd->nunits = 0;
			if (a.ri_k)
				a.ri_k[r] = 0;
		}
		return;
	}
	const uint64_t nlow = (uint64_t) n - 1 - m->nex;
	const uint32_t nunits = (uint32_t) ((nlow + RICE_UNIT - 1) / RICE_UNIT);
	const size_t u0 = (size_t) a.first_chunk[r] * RICE_UPC;
	uint64_t S[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	for (uint32_t i = lane; i < nunits; i += 64) {
#pragma unroll
		for (int k = 0; k < 8; k++)
			S[k] += a.ri_sum[(u0 + i) * 8 + k];
	}
	uint32_t best = 0;
	uint64_t best_c = RICE_FAIL64;
#pragma unroll
	for (int k = 0; k < 8; k++) {
		const uint64_t c = sum64(S[k]) + nlow * (uint64_t) (1 + k);
		if (c < best_c) { // (press.c:4884: '<', ties go to the lower k)
			best_c = c;
			best = (uint32_t) k;
		}
	}
	const uint64_t nbits = 3 + best_c;
	const uint64_t paylen = (nbits - 1) / 8 + 1;
	uint64_t carry = 3;
	for (uint32_t base = 0; base < nunits; base += 64) {
		const uint32_t i = base + lane;
		uint64_t b = 0;
		if (i < nunits) {
			const uint64_t left = nlow - (uint64_t) i * RICE_UNIT;
			b = a.ri_sum[(u0 + i) * 8 + best] + (left < RICE_UNIT ? left : RICE_UNIT) * (1 + best);
		}
		const uint64_t inc = wave_incl_scan64(b, lane);
		if (i < nunits)
			a.ri_start[u0 + i] = carry + inc - b;
		carry += __shfl(inc, 63, 64);
	}
	if (lane)
		return;
	bool ok = true;
	if (need) {
		need[r] += paylen;
	} else {
		const uint64_t total = (uint64_t) m->hdr + m->seclen + paylen;
		ok = total <= a.out_off[r + 1] - a.out_off[r];
		a.out_len[r] = ok ? total : RICE_FAIL64;
	}
	rd->nbits = nbits;
	rd->paylen = paylen;
	rd->k = best;
	rd->ok = ok ? 1 : 0;
	rd->nlow = (uint32_t) nlow;
	rd->nunits = nunits;
	if (a.ri_k)
		a.ri_k[r] = (uint8_t) best;
}

__global__ __launch_bounds__(256) void k_rice_write(BatchArgs a)
{
	__shared__ uint32_t s_bits[4][RICE_WIN];
	const uint32_t lane = threadIdx.x & 63;
	uint32_t *lds = s_bits[threadIdx.x >> 6];
	Unit x;
	if (!unit_of(a, uni(blockIdx.x * 4 + (threadIdx.x >> 6)), x))
		return;
	const RiceRead *rd = a.ri_rd + x.r;
	if (!uni(rd->ok))
		return;
	const uint32_t k = uni(rd->k);
	const uint8_t *in = a.low_tmp + x.soff + x.v0;
	uint32_t *pay = reinterpret_cast<uint32_t *>(a.ri_pay + 2 * x.soff);
	uint64_t P = uni64(a.ri_start[x.u]);
	if (x.v0 == 0 && lane == 0 && k)
		atomicOr(pay, ((k >> 2) & 1u) | (((k >> 1) & 1u) << 1) | ((k & 1u) << 2));
	for (uint32_t step = 0; step < RICE_UNIT; step += 512) {
		uint32_t nv;
		const uint64_t v = load8(in, step + lane * 8, x.cnt, nv);
		uint32_t L = 0;
		for (uint32_t j = 0; j < nv; j++)
			L += (((uint32_t) (v >> (8 * j)) & 0xFFu) >> k) + 1 + k;
		const uint32_t inc = scan32(L, lane);
		const uint32_t tot = (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
		if (!tot)
			break; // (wave-uniform: the unit's values are used up)
		const uint64_t mine = P + inc - L, mine_end = P + inc;
		const uint64_t firstdw = P >> 5, lastdw = (P + tot - 1) >> 5;
		for (uint64_t wb = firstdw; wb <= lastdw; wb += RICE_WIN) {
			for (uint32_t d = lane; d < RICE_WIN; d += 64)
				lds[d] = 0;
			__builtin_amdgcn_wave_barrier();
			// nb bits (1 .. 32) at stream position pos, cut to the window
			auto put = [&](uint64_t pos, uint32_t bits, uint32_t nb) {
				const uint64_t d = (pos >> 5) - wb; // (wraps for a position in front of the window: then >= RICE_WIN)
				const uint32_t sh = (uint32_t) pos & 31u;
				if (d < RICE_WIN)
					atomicOr(&lds[d], bits << sh);
				if (sh + nb > 32 && d + 1 < RICE_WIN) // (d + 1 == 0: the code's tail is the window's first dword)
					atomicOr(&lds[d + 1], bits >> (32 - sh));
			};
			if (L && mine_end > (wb << 5) && mine < ((wb + RICE_WIN) << 5)) {
				uint64_t p = mine;
				for (uint32_t j = 0; j < nv; j++) {
					const uint32_t b = (uint32_t) (v >> (8 * j)) & 0xFFu;
					uint32_t q = b >> k;
					while (q) { // a run can cross eight dwords
						const uint32_t c = q < 32 ? q : 32u;
						put(p, c == 32 ? ~0u : (1u << c) - 1u, c);
						p += c;
						q -= c;
					}
					p += 1; // the zero bit
					if (k)
						put(p, __brev(b & ((1u << k) - 1u)) >> (32 - k), k);
					p += k;
				}
			}
			__builtin_amdgcn_wave_barrier();
			for (uint32_t d = lane; d < RICE_WIN && wb + d <= lastdw; d += 64) {
				const uint32_t w = lds[d];
				const uint64_t idx = wb + d;
				if (idx == firstdw || idx == lastdw) { // shared with the spans around this one
					if (w)
						atomicOr(pay + idx, w);
				} else {
					pay[idx] = w;
				}
			}
			__builtin_amdgcn_wave_barrier();
		}
		P += tot;
	}
}

// staged payload -> the slot: RICE_COPY bytes per unit index, which covers every payload (at most nine bits a value)
__global__ __launch_bounds__(256) void k_rice_copy(BatchArgs a)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t u = uni(blockIdx.x * 4 + (threadIdx.x >> 6));
	const uint32_t t = u / RICE_UPC;
	if (t >= uni(a.ctl->nchunks))
		return;
	const ChunkDesc *d = a.chunks + t;
	const uint32_t r = uni(d->read);
	const RiceRead *rd = a.ri_rd + r;
	const ReadMeta *m = a.meta + r;
	if (uni(m->status) || !uni(rd->ok))
		return;
	const uint64_t paylen = uni64(rd->paylen);
	const uint64_t b0 = ((uint64_t) uni(d->j) * RICE_UPC + u % RICE_UPC) * RICE_COPY;
	if (b0 >= paylen)
		return;
	const uint32_t len = paylen - b0 < RICE_COPY ? (uint32_t) (paylen - b0) : RICE_COPY;
	const uint8_t *src = a.ri_pay + 2 * uni64(d->sig_off) + b0;
	uint8_t *dst = a.out + a.out_off[r] + uni(m->hdr) + uni(m->seclen) + b0;
	for (uint32_t b = lane * 8; b < len; b += 512) {
		if (b + 8 <= len) {
			uint2 w = *reinterpret_cast<const uint2 *>(src + b);
			__builtin_memcpy(dst + b, &w, 8);
		} else {
			for (uint32_t j = b; j < len; j++)
				dst[j] = src[j];
		}
	}
}

// ------------------------------------------------------------------ depress

namespace {

struct RBits {
	const uint8_t *in; // the payload
	uint64_t len;      // its bytes
};

// 32 bits from bit p on; behind the end: zeros
__device__ __forceinline__ uint32_t peek32(const RBits &b, uint64_t p)
{
	const uint64_t at = p >> 3;
	uint64_t w = 0;
	if (at + 8 <= b.len) {
		__builtin_memcpy(&w, b.in + at, 8);
	} else {
		for (uint32_t i = 0; i < 5; i++)
			if (at + i < b.len)
				w |= (uint64_t) b.in[at + i] << (8 * i);
	}
	return (uint32_t) (w >> (p & 7u));
}

// one code from p on: p moves behind it, v = its value; false: a run longer than cap (p is then inside the run)
__device__ __forceinline__ bool rice_code(const RBits &b, uint32_t k, uint64_t &p, uint32_t &v, uint64_t cap)
{
	uint64_t run = 0;
	uint32_t w, ones;
	for (;;) {
		w = peek32(b, p);
		ones = w == ~0u ? 32u : (uint32_t) __builtin_ctz(~w);
		p += ones;
		run += ones;
		if (ones < 32)
			break;
		if (run > cap)
			return false;
	}
	p += 1;
	uint32_t rem = 0;
	if (k) {
		const uint32_t f = ones + 1 + k <= 32 ? w >> (ones + 1) : peek32(b, p);
		rem = __brev(f & ((1u << k) - 1u)) >> (32 - k);
	}
	p += k;
	v = (((uint32_t) run << k) | rem) & 0xFFu; // (q is a uint8_t in the reference: the run counts modulo 256)
	return true;
}

struct DTile {
	uint32_t r;
	uint32_t s;     // the lane's subsequence of the read
	size_t g;       // ... and its record
	uint64_t begin; // its first bit
	RBits b;
	uint32_t k;
};
// the subsequence of a thread; false: none
__device__ __forceinline__ bool dtile_of(const DecodeArgs &a, DTile &t)
{
	if (blockIdx.x >= uni(a.ri_ctl[0]) || blockIdx.x >= a.ri_max_tiles)
		return false;
	const uint2 e = a.ri_tile[blockIdx.x];
	t.r = uni(e.x);
	if (t.r == RICE_NONE)
		return false; // (a tile id k_rice_dplan took and could not use)
	const RiceDRead *rd = a.ri_drd + t.r;
	t.s = uni(e.y) * RICE_DT + threadIdx.x;
	if (t.s >= uni(rd->nsubs))
		return false;
	t.g = (size_t) blockIdx.x * RICE_DT + threadIdx.x;
	t.begin = (uint64_t) t.s * RICE_SUB;
	const ReadMeta *m = a.meta + t.r;
	t.b.in = a.in + a.in_off[t.r] + uni(m->hdr) + uni(m->seclen);
	t.b.len = uni64(rd->paylen);
	t.k = uni(rd->k);
	return true;
}

// the subsequence from `start` on -> its record
__device__ __forceinline__ void dsub(const DecodeArgs &a, const DTile &t, uint64_t start)
{
	uint32_t *rec = a.ri_rec + 3 * t.g;
	uint64_t p = start;
	uint32_t cnt = 0, v;
	const uint64_t end = t.begin + RICE_SUB;
	while (p < end) {
		if (!rice_code(t.b, t.k, p, v, RICE_RUNCAP)) {
			rec[0] = RICE_NONE;
			rec[1] = RICE_SAT;
			rec[2] = 0;
			return;
		}
		cnt++;
	}
	rec[0] = (uint32_t) (start - t.begin); // (no run beyond RICE_RUNCAP: the offsets are small)
	rec[1] = (uint32_t) (p - end);
	rec[2] = cnt;
}

} // namespace

// One thread per read: its tiles get contiguous ids, taken by one atomic per wave.
__global__ __launch_bounds__(256) void k_rice_dplan(DecodeArgs a)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
	uint32_t nsubs = 0, k = 0, nlow = 0;
	uint64_t paylen = 0;
	bool ok = false;
	if (r < a.nreads && a.meta[r].status == 0) {
		const ReadMeta *m = a.meta + r;
		const uint64_t head = (uint64_t) m->hdr + m->seclen;
		ok = true;
		nlow = m->nlow;
		paylen = a.in_len[r] - head; // (k_ex_parse: the section lies inside the stream)
		if (paylen) {
			const uint32_t b = a.in[a.in_off[r] + head];
			k = ((b & 1u) << 2) | (b & 2u) | ((b >> 2) & 1u);
		}
		const uint64_t budget = 9ull * nlow + 3;
		const uint64_t useful = paylen * 8 < budget ? paylen * 8 : budget;
		nsubs = nlow ? (uint32_t) ((useful + RICE_SUB - 1) / RICE_SUB) : 0u;
	}
	uint32_t nt = (nsubs + RICE_DT - 1) / RICE_DT;
	const uint32_t inc = scan32(nt, lane);
	uint32_t base = 0;
	if (lane == 63 && inc)
		base = atomicAdd(&a.ri_ctl[0], inc);
	base = (uint32_t) __builtin_amdgcn_readlane((int) base, 63);
	const uint32_t first = base + inc - nt;
	if (r >= a.nreads)
		return;
	if ((uint64_t) first + nt > a.ri_max_tiles) { // (the plan's bound covers every batch of disjoint rooms: the walk alone then)
		for (uint32_t j = 0; j < nt && first + j < a.ri_max_tiles; j++)
			a.ri_tile[first + j] = make_uint2(RICE_NONE, 0);
		nt = 0;
		nsubs = 0;
	}
	for (uint32_t j = 0; j < nt; j++)
		a.ri_tile[first + j] = make_uint2(r, j);
	RiceDRead *rd = a.ri_drd + r;
	rd->paylen = paylen;
	rd->wpos = 3;
	rd->widx = 0;
	rd->k = k;
	rd->nsubs = nsubs;
	rd->tile0 = first;
	rd->nlow = nlow;
	rd->hmin = nsubs;
	rd->ok = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_rice_sync(DecodeArgs a)
{
	DTile t;
	if (!dtile_of(a, t))
		return;
	uint64_t start = 3;
	if (t.s) {
		uint64_t p = t.s == 1 ? 3 : t.begin - RICE_SUB;
		uint32_t v;
		while (p < t.begin) {
			if (!rice_code(t.b, t.k, p, v, RICE_RUNCAP)) {
				uint32_t *rec = a.ri_rec + 3 * t.g;
				rec[0] = RICE_NONE;
				rec[1] = RICE_SAT;
				rec[2] = 0;
				return;
			}
		}
		start = p;
	}
	dsub(a, t, start);
}

// A record is written by its own lane alone, and a lane reads of the record in front the one word `end`: whichever
// value it sees, k_rice_check compares what the launches left.
template <int ROUND>
__global__ __launch_bounds__(256) void k_rice_fix(DecodeArgs a)
{
	DTile t;
	if (!dtile_of(a, t) || t.s == 0)
		return;
	const uint32_t want = a.ri_rec[3 * (t.g - 1) + 1];
	if (want >= RICE_SAT || want == a.ri_rec[3 * t.g])
		return;
	atomicAdd(&a.ri_ctl[ROUND], 1u);
	dsub(a, t, t.begin + want);
}

__global__ __launch_bounds__(256) void k_rice_check(DecodeArgs a)
{
	__shared__ uint32_t s_cnt[4];
	DTile t;
	const bool have = dtile_of(a, t);
	if (blockIdx.x >= uni(a.ri_ctl[0]))
		return;
	uint32_t cnt = 0;
	if (have) {
		const uint32_t start = a.ri_rec[3 * t.g];
		const uint32_t want = t.s ? a.ri_rec[3 * (t.g - 1) + 1] : 3u;
		if (start != want || want >= RICE_SAT)
			atomicMin(&a.ri_drd[t.r].hmin, t.s);
		cnt = a.ri_rec[3 * t.g + 2];
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		cnt += (uint32_t) __shfl_xor((int) cnt, d, 64);
	if ((threadIdx.x & 63) == 0)
		s_cnt[threadIdx.x >> 6] = cnt;
	__syncthreads();
	if (threadIdx.x == 0)
		a.ri_tbase[(size_t) a.ri_max_tiles + blockIdx.x] = (uint64_t) s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// one wave per read: ri_tbase[tile] = the codes of the read's tiles in front of it
__global__ __launch_bounds__(64) void k_rice_dscan(DecodeArgs a)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const RiceDRead *rd = a.ri_drd + r;
	const uint32_t nt = (rd->nsubs + RICE_DT - 1) / RICE_DT, t0 = rd->tile0;
	uint64_t carry = 0;
	for (uint32_t base = 0; base < nt; base += 64) {
		const uint32_t i = base + lane;
		const uint64_t c = i < nt ? a.ri_tbase[(size_t) a.ri_max_tiles + t0 + i] : 0;
		const uint64_t inc = wave_incl_scan64(c, lane);
		if (i < nt)
			a.ri_tbase[t0 + i] = carry + inc - c;
		carry += __shfl(inc, 63, 64);
	}
}

__global__ __launch_bounds__(256) void k_rice_emit(DecodeArgs a)
{
	__shared__ uint32_t s_w[4];
	DTile t;
	const bool have = dtile_of(a, t);
	if (blockIdx.x >= uni(a.ri_ctl[0]))
		return;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	if (uni(a.ri_tile[blockIdx.x].x) == RICE_NONE)
		return;
	RiceDRead *rd = a.ri_drd + uni(a.ri_tile[blockIdx.x].x);
	const uint32_t hmin = uni(rd->hmin);
	const bool live = have && t.s < hmin;
	const uint32_t cnt = live ? a.ri_rec[3 * t.g + 2] : 0u;
	const uint32_t inc = scan32(cnt, lane);
	if (lane == 63)
		s_w[w] = inc;
	__syncthreads();
	uint64_t o = a.ri_tbase[blockIdx.x] + inc - cnt;
	for (uint32_t i = 0; i < w; i++)
		o += s_w[i];
	if (!live)
		return;
	const uint64_t nlow = uni(rd->nlow);
	uint8_t *out = a.low + a.off[t.r];
	uint64_t p = t.begin + a.ri_rec[3 * t.g];
	for (uint32_t i = 0; i < cnt; i++) {
		uint32_t v;
		rice_code(t.b, t.k, p, v, ~0ull);
		if (o + i < nlow)
			out[o + i] = (uint8_t) v;
	}
	if (t.s + 1 == hmin) { // where the chain ends: the walk goes on from here
		rd->wpos = p;
		rd->widx = o + cnt;
	}
}

__global__ __launch_bounds__(64) void k_rice_walk(DecodeArgs a)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const RiceDRead *rd = a.ri_drd + r;
	if (!uni(rd->ok))
		return;
	const ReadMeta *m = a.meta + r;
	RBits b;
	b.in = a.in + a.in_off[r] + uni(m->hdr) + uni(m->seclen);
	b.len = uni64(rd->paylen);
	const uint32_t k = uni(rd->k);
	const uint64_t nlow = uni(rd->nlow);
	uint8_t *out = a.low + a.off[r];
	uint64_t idx = uni64(rd->widx), p = uni64(rd->wpos);
	if (idx > nlow)
		idx = nlow;
	if (lane == 0) {
		uint32_t walked = 0;
		while (idx < nlow && p < b.len * 8) {
			uint32_t v;
			rice_code(b, k, p, v, ~0ull);
			out[idx++] = (uint8_t) v;
			walked++;
		}
		if (walked)
			atomicAdd(&a.ri_ctl[3], walked);
	}
	idx = __shfl(idx, 0, 64);
	for (uint64_t i = idx + lane; i < nlow; i += 64) // behind the stream's end every code is a zero bit and k zero bits
		out[i] = 0;
}

// ------------------------------------------------------------------ launchers

// behind k_low_encode_chunked<false>; need != NULL: the sizes alone
void launch_rice_encode(const BatchArgs &a, uint64_t *need, hipStream_t s)
{
	const uint32_t grid = (uint32_t) (((uint64_t) a.max_chunks * RICE_UPC + 3) / 4);
	hipLaunchKernelGGL(k_rice_count, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_pick, dim3(a.nreads), dim3(64), 0, s, a, need);
	if (need)
		return;
	(void) hipMemsetAsync(a.ri_pay, 0, a.ri_pay_bytes, s);
	hipLaunchKernelGGL(k_rice_write, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_copy, dim3(grid), dim3(256), 0, s, a);
}

// behind k_ex_parse: the payloads -> a.low
void launch_rice_decode(const DecodeArgs &a, hipStream_t s)
{
	(void) hipMemsetAsync(a.ri_ctl, 0, RICE_CTL_WORDS * 4, s);
	hipLaunchKernelGGL(k_rice_dplan, dim3((a.nreads + 255) / 256), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_sync, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_fix<1>, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_fix<2>, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_check, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_dscan, dim3(a.nreads), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_rice_emit, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_walk, dim3(a.nreads), dim3(64), 0, s, a);
}

} // namespace ph
