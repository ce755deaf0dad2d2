// press_prefix.h - the prefix-code engine of the entropy stages that code a read's one-byte values one code per value:
// Golomb-Rice (press_rice.hip, stage 6) and a Huffman code per read (press_dhuf.hip, stage 7).  What the two share is
// here once, as device function templates over a small CODE POLICY; the __global__ kernels are wrappers in the two files.
//
// PRESS.  A read's one-byte values (a.low_tmp, k_low_encode_chunked) are cut into UNITS of PFX_UNIT values, a wave
// each; unit i of a read is entry PFX_UPC * first_chunk + i of the unit tables (a chunk of CHUNK samples has room for
// PFX_UPC).
//   prefix_unit_scan  per read: the exclusive scan of the units' bits, so that every unit knows its first bit
//   prefix_write      per unit: code lengths -> wave scan -> bit positions; the bits of 512 values are assembled in LDS
//                     (windows of 8192 bits: a unit's span has no useful bound) and go out as whole dwords to a STAGED
//                     payload in scratch (a.ri_pay, dword aligned, zeroed by the launcher): the first and last dword
//                     of a span are shared with the neighbours and merged with atomic OR, the others are stored
//   prefix_copy       staged payload -> the slot, behind the section and what the family puts between the two
//
// DEPRESS.  The plan of press_huffman.hip.  The payload is cut into SUBSEQUENCES of PFX_SUB bits, a lane each, PFX_DT
// of them a tile.
//   prefix_dplan   per read: the subsequences worth decoding in parallel (those of the payload, at most what nlow values
//                  can take at nine bits each: a pressed payload never has more), the tile table
//   prefix_sync    a lane guesses the first code of its subsequence by running up through the one in front, then
//                  decodes its own: record = { start, end, codes }, start and end relative to the subsequence's
//                  first bit / the next one's
//   prefix_fix     a lane whose start is not the end the subsequence in front recorded decodes again from that end
//   prefix_check   per read the first subsequence whose start is still not that end (hmin); the tiles' code counts
//   prefix_dscan   per read the exclusive scan of the tiles' counts
//   prefix_emit    the subsequences in front of hmin: their records chain from the first code bit, so they are the
//                  true ones; values to a.low from the true starts, up to nlow
//   prefix_walk    per read, serially from where the chain ends, until nlow values are out
// The number of launches is fixed, and correctness never depends on synchronisation: a stream whose codes all have one
// length leaves hmin small and the walk does the work.
//
// A code policy C is a struct of static members, every one resolved at compile time:
//   FIRST_BIT      the first code bit of a payload
//   LDS_STATE      tile_state() is the whole workgroup's work (LDS, a barrier); false: the tile kernels take from the
//                  policy no LDS, no barrier and no pointer
//   KEEP_PARTIAL   a subsequence that stops at bits that are no code keeps { start, PFX_SAT, codes so far }, so that
//                  emit writes those codes and the walk goes on from where it stopped; false: { PFX_NONE, PFX_SAT, 0 }
//   STRICT_END     the walk: a code that fails refuses the read (ReadMeta::status); false: the walk stops at the
//                  payload's end and every value behind it is 0
//   State          what the decoder knows of a read
//   press_extra(rd)                 bytes between section and payload, press
//   takes_part(a, r)                dplan, for a read k_ex_parse accepted: is there a payload to decode?
//   extra(a, r)                     bytes between section and payload, depress
//   plan_k(pay, paylen)             PfxDRead::k
//   tile_state(a, r), read_state(a, r)   the State for a tile kernel / for the walk
//   code<BOUNDED>(b, st, p, v)      one code from bit p on: p moves behind it, v = its value; false: no code.  BOUNDED:
//                                   the caller is sync or fix, whose lanes may spend only a bounded time on bits that
//                                   are not their own
#pragma once

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

// ------------------------------------------------------------------ press

// the unit a wave works on: false if there is none
struct PfxUnit {
	uint32_t r, u, cnt; // read, unit id, values
	uint64_t v0, soff;  // first value, the read's sample offset
};
__device__ __forceinline__ bool unit_of(const BatchArgs &a, uint32_t u, PfxUnit &x)
{
	const uint32_t t = u / PFX_UPC;
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
	x.v0 = ((uint64_t) uni(d->j) * PFX_UPC + u % PFX_UPC) * PFX_UNIT;
	if (x.v0 >= nlow)
		return false;
	x.cnt = nlow - x.v0 < PFX_UNIT ? (uint32_t) (nlow - x.v0) : PFX_UNIT;
	return true;
}
// ... of this wave, four waves a workgroup
__device__ __forceinline__ bool unit_of(const BatchArgs &a, PfxUnit &x)
{
	return unit_of(a, uni(blockIdx.x * 4 + (threadIdx.x >> 6)), x);
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

// One wave per read: ri_start[unit] = first + the bits of the read's units in front of it; bits_of(entry, i): the bits
// of the read's unit i, which is entry `entry` of the unit tables.
template <class F>
__device__ __forceinline__ void prefix_unit_scan(const BatchArgs &a, uint32_t r, uint32_t nunits, uint64_t first, F bits_of)
{
	const uint32_t lane = threadIdx.x;
	const size_t u0 = (size_t) a.first_chunk[r] * PFX_UPC;
	uint64_t carry = first;
	for (uint32_t base = 0; base < nunits; base += 64) {
		const uint32_t i = base + lane;
		const uint64_t b = i < nunits ? bits_of(u0 + i, i) : 0;
		const uint64_t inc = wave_incl_scan64(b, lane);
		if (i < nunits)
			a.ri_start[u0 + i] = carry + inc - b;
		carry += __shfl(inc, 63, 64);
	}
}

// The staged writer: the unit x of a wave, whose window is lds[PFX_WIN].  len_of(b): the bits of the value b's code;
// put_code(put, p, b): the code's bits to position p on, through put(pos, bits, nb): nb bits (1 .. 32) at stream
// position pos; p moves behind the code.
template <class L, class P>
__device__ __forceinline__ void prefix_write(const BatchArgs &a, const PfxUnit &x, uint32_t *lds, L len_of, P put_code)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint8_t *in = a.low_tmp + x.soff + x.v0;
	uint32_t *pay = reinterpret_cast<uint32_t *>(a.ri_pay + 2 * x.soff);
	uint64_t P0 = uni64(a.ri_start[x.u]);
	for (uint32_t step = 0; step < PFX_UNIT; step += 512) {
		uint32_t nv;
		const uint64_t v = load8(in, step + lane * 8, x.cnt, nv);
		uint32_t L0 = 0;
		for (uint32_t j = 0; j < nv; j++)
			L0 += len_of((uint32_t) (v >> (8 * j)) & 0xFFu);
		const uint32_t inc = scan32(L0, lane);
		const uint32_t tot = (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
		if (!tot)
			break; // (wave-uniform: the unit's values are used up, or no code of them has a bit)
		const uint64_t mine = P0 + inc - L0, mine_end = P0 + inc;
		const uint64_t firstdw = P0 >> 5, lastdw = (P0 + tot - 1) >> 5;
		for (uint64_t wb = firstdw; wb <= lastdw; wb += PFX_WIN) {
			for (uint32_t d = lane; d < PFX_WIN; d += 64)
				lds[d] = 0;
			__builtin_amdgcn_wave_barrier();
			// cut to the window
			auto put = [&](uint64_t pos, uint32_t bits, uint32_t nb) {
				const uint64_t d = (pos >> 5) - wb; // (wraps for a position in front of the window: then >= PFX_WIN)
				const uint32_t sh = (uint32_t) pos & 31u;
				if (d < PFX_WIN)
					atomicOr(&lds[d], bits << sh);
				if (sh + nb > 32 && d + 1 < PFX_WIN) // (d + 1 == 0: the code's tail is the window's first dword)
					atomicOr(&lds[d + 1], bits >> (32 - sh));
			};
			if (L0 && mine_end > (wb << 5) && mine < ((wb + PFX_WIN) << 5)) {
				uint64_t p = mine;
				for (uint32_t j = 0; j < nv; j++)
					put_code(put, p, (uint32_t) (v >> (8 * j)) & 0xFFu);
			}
			__builtin_amdgcn_wave_barrier();
			for (uint32_t d = lane; d < PFX_WIN && wb + d <= lastdw; d += 64) {
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
		P0 += tot;
	}
}

// staged payload -> the slot: PFX_COPY bytes per unit index, which covers every payload (at most nine bits a value)
template <class C>
__device__ __forceinline__ void prefix_copy(const BatchArgs &a)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t u = uni(blockIdx.x * 4 + (threadIdx.x >> 6));
	const uint32_t t = u / PFX_UPC;
	if (t >= uni(a.ctl->nchunks))
		return;
	const ChunkDesc *d = a.chunks + t;
	const uint32_t r = uni(d->read);
	const PfxRead *rd = a.ri_rd + r;
	const ReadMeta *m = a.meta + r;
	if (uni(m->status) || !uni(rd->ok))
		return;
	const uint64_t paylen = uni64(rd->paylen);
	const uint64_t b0 = ((uint64_t) uni(d->j) * PFX_UPC + u % PFX_UPC) * PFX_COPY;
	if (b0 >= paylen)
		return;
	const uint32_t len = paylen - b0 < PFX_COPY ? (uint32_t) (paylen - b0) : PFX_COPY;
	const uint8_t *src = a.ri_pay + 2 * uni64(d->sig_off) + b0;
	uint8_t *dst = a.out + a.out_off[r] + uni(m->hdr) + uni(m->seclen) + uni(C::press_extra(*rd)) + b0;
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

struct PfxBits {
	const uint8_t *in; // the payload
	uint64_t len;      // its bytes
};

// 32 bits from bit p on; behind the end: zeros
__device__ __forceinline__ uint32_t peek32(const PfxBits &b, uint64_t p)
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

// 64 bits from bit p on; behind the end: zeros
__device__ __forceinline__ uint64_t peek64(const PfxBits &b, uint64_t p)
{
	const uint64_t at = p >> 3;
	const uint32_t sh = (uint32_t) p & 7u;
	uint64_t w = 0;
	if (at + 8 <= b.len) {
		__builtin_memcpy(&w, b.in + at, 8);
	} else {
		for (uint32_t i = 0; i < 8; i++)
			if (at + i < b.len)
				w |= (uint64_t) b.in[at + i] << (8 * i);
	}
	w >>= sh;
	if (sh && at + 8 < b.len)
		w |= (uint64_t) b.in[at + 8] << (64 - sh);
	return w;
}

// a read's payload
template <class C>
__device__ __forceinline__ PfxBits payload_of(const DecodeArgs &a, uint32_t r)
{
	const ReadMeta *m = a.meta + r;
	PfxBits b;
	b.in = a.in + a.in_off[r] + uni(m->hdr) + uni(m->seclen) + uni(C::extra(a, r));
	b.len = uni64(a.ri_drd[r].paylen);
	return b;
}

template <class C>
struct PfxTile {
	uint32_t r;
	uint32_t s;     // the lane's subsequence of the read
	size_t g;       // ... and its record
	uint64_t begin; // its first bit
	PfxBits b;
	typename C::State st;
};
// the tile of a workgroup, { read, tile of the read }; false (for the whole workgroup): none
__device__ __forceinline__ bool tile_read(const DecodeArgs &a, uint2 &e)
{
	if (blockIdx.x >= uni(a.ri_ctl[0]) || blockIdx.x >= a.ri_max_tiles)
		return false;
	e = a.ri_tile[blockIdx.x];
	e.x = uni(e.x);
	e.y = uni(e.y);
	return e.x != PFX_NONE; // (a tile id prefix_dplan took and could not use)
}
// the subsequence of a thread of that tile, the decoder's state excepted; false: none
template <class C>
__device__ __forceinline__ bool dtile_of(const DecodeArgs &a, uint2 e, PfxTile<C> &t)
{
	t.r = e.x;
	t.s = e.y * PFX_DT + threadIdx.x;
	if (t.s >= uni(a.ri_drd[t.r].nsubs))
		return false;
	t.g = (size_t) blockIdx.x * PFX_DT + threadIdx.x;
	t.begin = (uint64_t) t.s * PFX_SUB;
	t.b = payload_of<C>(a, t.r);
	return true;
}

// the subsequence from `start` on -> its record
template <class C>
__device__ __forceinline__ void dsub(const DecodeArgs &a, const PfxTile<C> &t, uint64_t start)
{
	uint32_t *rec = a.ri_rec + 3 * t.g;
	uint64_t p = start;
	uint32_t cnt = 0, v;
	const uint64_t end = t.begin + PFX_SUB;
	bool whole = true;
	while (p < end) {
		if (!C::template code<true>(t.b, t.st, p, v)) {
			whole = false;
			break;
		}
		cnt++;
	}
	const bool keep = whole || C::KEEP_PARTIAL;
	rec[0] = keep ? (uint32_t) (start - t.begin) : PFX_NONE; // (a code that sync and fix accept is short: the offsets are small)
	rec[1] = whole ? (uint32_t) (p - end) : PFX_SAT;
	rec[2] = keep ? cnt : 0u;
}

// One thread per read: its tiles get contiguous ids, taken by one atomic per wave.
template <class C>
__device__ __forceinline__ void prefix_dplan(const DecodeArgs &a)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
	uint32_t nsubs = 0, k = 0, nlow = 0;
	uint64_t paylen = 0;
	bool ok = false;
	if (r < a.nreads && a.meta[r].status == 0 && C::takes_part(a, r)) {
		const ReadMeta *m = a.meta + r;
		const uint64_t head = (uint64_t) m->hdr + m->seclen + C::extra(a, r);
		ok = true;
		nlow = m->nlow;
		paylen = a.in_len[r] - head; // (k_ex_parse, and whoever checked what C::extra() counts: it lies inside the stream)
		k = C::plan_k(a.in + a.in_off[r] + head, paylen);
		// a pressed payload has at most nine bits a value; what a forged one has beyond them is the walk's
		const uint64_t budget = 9ull * nlow + 3;
		const uint64_t useful = paylen * 8 < budget ? paylen * 8 : budget;
		nsubs = nlow ? (uint32_t) ((useful + PFX_SUB - 1) / PFX_SUB) : 0u;
	}
	uint32_t nt = (nsubs + PFX_DT - 1) / PFX_DT;
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
			a.ri_tile[first + j] = make_uint2(PFX_NONE, 0);
		nt = 0;
		nsubs = 0;
	}
	for (uint32_t j = 0; j < nt; j++)
		a.ri_tile[first + j] = make_uint2(r, j);
	PfxDRead *rd = a.ri_drd + r;
	rd->paylen = paylen;
	rd->wpos = C::FIRST_BIT;
	rd->widx = 0;
	rd->k = k;
	rd->nsubs = nsubs;
	rd->tile0 = first;
	rd->nlow = nlow;
	rd->hmin = nsubs;
	rd->ok = ok ? 1 : 0;
}

template <class C>
__device__ __forceinline__ void prefix_sync(const DecodeArgs &a)
{
	uint2 e;
	if (!tile_read(a, e))
		return;
	const typename C::State st = C::tile_state(a, e.x);
	PfxTile<C> t;
	if (!dtile_of(a, e, t))
		return;
	t.st = st;
	uint64_t start = C::FIRST_BIT;
	if (t.s) {
		uint64_t p = t.s == 1 ? C::FIRST_BIT : t.begin - PFX_SUB;
		uint32_t v;
		while (p < t.begin) {
			if (!C::template code<true>(t.b, t.st, p, v)) {
				uint32_t *rec = a.ri_rec + 3 * t.g;
				rec[0] = PFX_NONE;
				rec[1] = PFX_SAT;
				rec[2] = 0;
				return;
			}
		}
		start = p;
	}
	dsub(a, t, start);
}

// A record is written by its own lane alone, and a lane reads of the record in front the one word `end`: whichever
// value it sees, prefix_check compares what the launches left.  ctr: the word of ri_ctl that counts this round's work.
template <class C>
__device__ __forceinline__ void prefix_fix(const DecodeArgs &a, uint32_t ctr)
{
	uint2 e;
	if (!tile_read(a, e))
		return;
	PfxTile<C> t;
	const bool have = dtile_of(a, e, t) && t.s != 0;
	uint32_t want = PFX_SAT;
	if (have)
		want = a.ri_rec[3 * (t.g - 1) + 1];
	const bool redo = have && want < PFX_SAT && want != a.ri_rec[3 * t.g];
	if constexpr (C::LDS_STATE) { // no lane has work: the state is not loaded
		if (!__syncthreads_or(redo ? 1 : 0))
			return;
	} else if (!redo) {
		return;
	}
	t.st = C::tile_state(a, e.x);
	if (!redo)
		return;
	atomicAdd(&a.ri_ctl[ctr], 1u);
	dsub(a, t, t.begin + want);
}

template <class C>
__device__ __forceinline__ void prefix_check(const DecodeArgs &a)
{
	__shared__ uint32_t s_cnt[4];
	uint2 e;
	if (!tile_read(a, e)) {
		if (blockIdx.x < uni(a.ri_ctl[0]) && blockIdx.x < a.ri_max_tiles && threadIdx.x == 0)
			a.ri_tbase[(size_t) a.ri_max_tiles + blockIdx.x] = 0;
		return;
	}
	PfxTile<C> t;
	const bool have = dtile_of(a, e, t);
	uint32_t cnt = 0;
	if (have) {
		const uint32_t start = a.ri_rec[3 * t.g];
		const uint32_t want = t.s ? a.ri_rec[3 * (t.g - 1) + 1] : C::FIRST_BIT;
		if (start != want || want >= PFX_SAT)
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
__device__ __forceinline__ void prefix_dscan(const DecodeArgs &a)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const PfxDRead *rd = a.ri_drd + r;
	const uint32_t nt = (rd->nsubs + PFX_DT - 1) / PFX_DT, t0 = rd->tile0;
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

template <class C>
__device__ __forceinline__ void prefix_emit(const DecodeArgs &a)
{
	__shared__ uint32_t s_w[4];
	uint2 e;
	if (!tile_read(a, e))
		return;
	const typename C::State st = C::tile_state(a, e.x);
	PfxTile<C> t;
	const bool have = dtile_of(a, e, t);
	t.st = st;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	PfxDRead *rd = a.ri_drd + e.x;
	const uint32_t hmin = uni(rd->hmin);
	// the subsequences in front of hmin chain from the first code bit: their records are the true ones.  (KEEP_PARTIAL: a
	// record in front of hmin may have stopped early, end = PFX_SAT: then hmin is the next subsequence and the walk goes
	// on where it stopped.)
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
		uint32_t v = 0;
		C::template code<false>(t.b, t.st, p, v);
		if (o + i < nlow)
			out[o + i] = (uint8_t) v;
	}
	if (t.s + 1 == hmin) { // where the chain ends: the walk goes on from here
		rd->wpos = p;
		rd->widx = o + cnt;
	}
}

// one wave per read; lane 0 decodes
template <class C>
__device__ __forceinline__ void prefix_walk(const DecodeArgs &a)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const PfxDRead *rd = a.ri_drd + r;
	if (!uni(rd->ok))
		return;
	const PfxBits b = payload_of<C>(a, r);
	const uint64_t nlow = uni(rd->nlow);
	uint8_t *out = a.low + a.off[r];
	uint64_t idx = uni64(rd->widx), p = uni64(rd->wpos);
	if (idx > nlow)
		idx = nlow;
	if (lane == 0) {
		const typename C::State st = C::read_state(a, r);
		uint32_t walked = 0;
		while (idx < nlow && (C::STRICT_END || p < b.len * 8)) {
			uint32_t v;
			if (!C::template code<false>(b, st, p, v)) {
				if constexpr (C::STRICT_END) // bits that are no code, or the payload ends before nlow values are out
					a.meta[r].status = 1;
				break;
			}
			out[idx++] = (uint8_t) v;
			walked++;
		}
		if (walked)
			atomicAdd(&a.ri_ctl[3], walked);
	}
	if constexpr (!C::STRICT_END) { // behind the payload's end every code is a run of no ones and zero bits
		idx = __shfl(idx, 0, 64);
		for (uint64_t i = idx + lane; i < nlow; i += 64)
			out[i] = 0;
	}
}

} // namespace ph
