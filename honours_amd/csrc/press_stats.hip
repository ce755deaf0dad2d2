// press_stats.hip - per-read order statistics of decoded samples: the median and the median absolute deviation.
//
// For a read of c samples s[], with k = c / 2:  med = the k-th smallest (0-based) of s, mad = the k-th smallest of
// d[i] = |s[i] - med| (sigtk stat.h:56-73, mediani16 / medianf: ks_ksmall(n, copy, n / 2); events.c:171-194, madf before
// its factor).  Both are selections among 16-bit keys - s + 32768 for the median, d for the MAD - and are done as a
// radix select in two digits, without sorting:
//
//   k_stat_count<high>   one workgroup per tile of CHUNK samples (k_pa_tiles' table): the high digit of every key is
//                        counted in LDS, the counters that are not zero are added to the read's row in global scratch
//   k_stat_pick          one wave per read scans the row: the digit that holds rank k, the rank that is left within it
//   k_stat_count<low>    the low digit of the keys whose high digit is the chosen one
//   k_stat_pick          the key
//
// four launches for the median, the same four for the MAD (its keys need the median); the last pick writes stats and the
// two floats k_pa_convert normalises with.  Every sum is one of integers: the result does not depend on the order in
// which workgroups finish, and no workgroup waits for another.  A pick clears the row it has read, so one memset per
// call serves all four counting passes.

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

// The digit split: STAT_HI high bits, 16 - STAT_HI low bits (DESIGN.md 6.0.17 has the measurements behind it).
#ifndef PRESS_STAT_HI_BITS
#define PRESS_STAT_HI_BITS 8
#endif
constexpr int STAT_HI = PRESS_STAT_HI_BITS, STAT_LO = 16 - STAT_HI;
static_assert(STAT_HI >= 8 && STAT_HI <= 12, "the high digit's counters and their copies fit LDS");
constexpr uint32_t STAT_ROW = 1u << STAT_HI; // counters of a read's row (the low digit uses the first 2^STAT_LO)
constexpr uint32_t STAT_FAIL = 0xFFFFFFFFu;  // out_n of a refused read
constexpr uint32_t STAT_NONE = 0xFFFFFFFFu;  // no digit: a sample that is not counted

struct StatRead { // per read, between the launches (16 bytes)
	uint32_t c;  // samples (0: empty or refused)
	uint32_t k;  // the rank that is left
	uint32_t hi; // the high digit chosen
	int32_t med;
};
static_assert(sizeof(StatRead) == 16, "StatRead");

// LDS counters of a digit of BITS bits: as many copies as 16 KiB hold, 16 at the most
template <int BITS> struct StatLds {
	static constexpr uint32_t NB = 1u << BITS;
	static constexpr uint32_t COPIES = NB >= 4096 ? 1 : NB >= 256 ? 4096 / NB : 16;
	static constexpr uint32_t STRIDE = NB + 1; // (copies of one counter in different banks)
};

// One workgroup per tile: 8 samples per lane and step, a 16-byte load.  Nanopore levels crowd into a few hundred
// adjacent values and a lane's 8 samples are neighbours in time, so a lane first merges runs of one digit (typically
// all 8) and adds a run with ONE ds_add; lanes pick a copy of the counters by their id, so that a wave's 64 lanes
// spread over all of them.  A tile beyond the decoded count, or of a refused read, ends at once.
//
// RANGED (press_hip_signal_stats_ranged, the trimmed chunk call): only the samples [a', b') of the read take part - range[2r],
// range[2r + 1] clamped as include/press_hip.h 2y says.  The tiles and the aligned 16-byte groups are the room's, as
// without a range: a tile wholly outside the range ends at once, a group in front of a' is not loaded, and the groups at
// the two edges are masked per sample.  The range is a trailing parameter pack - empty, or one `const uint32_t *` - so
// that the kernel without a range keeps its arguments and its code.
template <int BITS, bool LOW, bool MAD, class... R>
__global__ __launch_bounds__(256) void k_stat_count(const int16_t *sig, const uint64_t *off, const uint32_t *out_n,
						     const uint2 *tiles, const uint32_t *ntiles, const StatRead *st, uint32_t *rows, R... range)
{
	constexpr bool RANGED = sizeof...(R) != 0;
	typedef StatLds<BITS> L;
	__shared__ uint32_t s_h[L::COPIES * L::STRIDE];
	if (blockIdx.x >= uni(*ntiles))
		return; // (the grid is an upper bound)
	const uint32_t r = uni(tiles[blockIdx.x].x), j = uni(tiles[blockIdx.x].y);
	const uint32_t on = uni(out_n[r]);
	const uint64_t first = (uint64_t) j * CHUNK;
	if (on == STAT_FAIL || first >= on)
		return;
	uint64_t end = first + CHUNK < on ? first + CHUNK : on;
	uint32_t lo = 0;
	if constexpr (RANGED) {
		const uint2 ab = range_clamp(range..., r, on);
		lo = uni(ab.x);
		const uint32_t hi = uni(ab.y);
		if (lo >= hi || first >= hi || first + CHUNK <= lo)
			return;
		end = first + CHUNK < hi ? first + CHUNK : hi;
	}
	for (uint32_t i = threadIdx.x; i < L::COPIES * L::STRIDE; i += 256)
		s_h[i] = 0;
	__syncthreads();
	const int32_t med = MAD ? (int32_t) uni((uint32_t) st[r].med) : 0;
	const uint32_t hi = LOW ? uni(st[r].hi) : 0;
	uint32_t *my = s_h + (threadIdx.x & (L::COPIES - 1)) * L::STRIDE;
	const int16_t *in = sig + uni64(off[r]);
	for (uint64_t i = first + threadIdx.x * 8; i < end; i += 256 * 8) {
		if (RANGED && i + 8 <= lo)
			continue;
		const uint4 q = ld16_stream(in + i);
		const uint32_t v[4] = { q.x, q.y, q.z, q.w };
		const uint32_t nv = end - i < 8 ? (uint32_t) (end - i) : 8u;
		const uint32_t skip = RANGED && lo > i ? (uint32_t) (lo - i) : 0u; // (the group that holds a')
		uint32_t cur = STAT_NONE, cnt = 0;
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const int32_t s = (e & 1) ? (int32_t) v[e >> 1] >> 16 : (int32_t) (int16_t) (v[e >> 1] & 0xFFFFu);
			const uint32_t key = MAD ? (uint32_t) (s >= med ? s - med : med - s) : (uint32_t) (s + 32768);
			uint32_t d = LOW ? key & (L::NB - 1) : key >> (16 - BITS);
			if ((uint32_t) e >= nv || (LOW && (key >> BITS) != hi) || (RANGED && (uint32_t) e < skip))
				d = STAT_NONE;
			if (d != cur) {
				if (cur != STAT_NONE)
					atomicAdd(&my[cur], cnt);
				cur = d;
				cnt = 0;
			}
			cnt++;
		}
		if (cur != STAT_NONE)
			atomicAdd(&my[cur], cnt);
	}
	__syncthreads();
	uint32_t *row = rows + (size_t) r * STAT_ROW;
	for (uint32_t b = threadIdx.x; b < L::NB; b += 256) {
		uint32_t sum = 0;
#pragma unroll
		for (uint32_t c = 0; c < L::COPIES; c++)
			sum += s_h[c * L::STRIDE + b];
		if (sum)
			atomicAdd(row + b, sum);
	}
}

__device__ __forceinline__ uint32_t stat_rank(uint32_t c, uint32_t num, uint32_t den)
{
	const uint64_t k = (uint64_t) c * num / den;
	return c == 0 ? 0u : k < c ? (uint32_t) k : c - 1;
}

// One wave per read, `stage` 0 .. 3: the median's high and low digit, the MAD's.  The row is scanned 64 counters at a
// time for the digit that holds the rank, and cleared for the next counting pass.  The rank is floor(c * num / den)
// (num / den = 1 / 2: sigtk's n / 2).  Stage 3 writes stats[2r] = med, stats[2r + 1] = mad and cal[2r] = (float) -med,
// cal[2r + 1] = 1 / ((float) mad * 1.4826f), or 1 for mad = 0; an empty or refused read gets {0, 0} and {0, 1}.
// RANGED: the read's count is L = b' - a' of its clamped range.
template <bool RANGED>
__device__ __forceinline__ void stat_pick(int stage, const uint32_t *out_n, const uint32_t *range, uint32_t nreads, StatRead *st, uint32_t *rows,
					  uint32_t num, uint32_t den, int32_t *stats, float *cal)
{
	const uint32_t r = uni(blockIdx.x * 4 + (threadIdx.x >> 6));
	if (r >= nreads)
		return;
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t nb = (stage & 1) ? 1u << STAT_LO : 1u << STAT_HI;
	StatRead t = { 0, 0, 0, 0 };
	if (stage == 0) {
		const uint32_t on = uni(out_n[r]);
		t.c = on == STAT_FAIL ? 0u : on;
		if (RANGED) {
			const uint2 ab = range_clamp(range, r, t.c);
			t.c = uni(ab.y - ab.x);
		}
		t.k = stat_rank(t.c, num, den);
	} else {
		t.c = uni(st[r].c);
		t.k = uni(st[r].k);
		t.hi = uni(st[r].hi);
		t.med = (int32_t) uni((uint32_t) st[r].med);
	}
	uint32_t digit = 0, left = t.k;
	if (t.c) {
		uint32_t *row = rows + (size_t) r * STAT_ROW;
		uint32_t before = 0;
		bool found = false;
		for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
			uint32_t v = 0;
			if (b0 + lane < nb) {
				v = row[b0 + lane];
				row[b0 + lane] = 0;
			}
			if (found)
				continue;
			uint32_t inc = v; // inclusive wave scan (at most c in all: no overflow)
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				const uint32_t u = __shfl_up(inc, d, 64);
				if (lane >= (uint32_t) d)
					inc += u;
			}
			const unsigned long long m = __ballot(before + inc > t.k);
			if (m) {
				const int l = __ffsll(m) - 1;
				digit = b0 + l;
				left = t.k - (before + (uint32_t) __shfl(inc - v, l, 64));
				found = true;
			} else {
				before += (uint32_t) __shfl(inc, 63, 64);
			}
		}
	}
	if (lane != 0)
		return;
	if (stage == 0 || stage == 2) {
		t.hi = digit;
		t.k = left;
		st[r] = t;
		return;
	}
	const uint32_t key = t.c ? (t.hi << STAT_LO) | digit : 0u;
	if (stage == 1) {
		t.med = t.c ? (int32_t) key - 32768 : 0;
		t.k = stat_rank(t.c, num, den);
		st[r] = t;
		return;
	}
	if (stats) {
		stats[2 * (size_t) r] = t.med;
		stats[2 * (size_t) r + 1] = (int32_t) key;
	}
	if (cal) {
		cal[2 * (size_t) r] = (float) -t.med;
		cal[2 * (size_t) r + 1] = key ? __fdiv_rn(1.0f, __fmul_rn((float) key, 1.4826f)) : 1.0f;
	}
}

__global__ __launch_bounds__(256) void k_stat_pick(int stage, const uint32_t *out_n, uint32_t nreads, StatRead *st, uint32_t *rows,
						    uint32_t num, uint32_t den, int32_t *stats, float *cal)
{
	stat_pick<false>(stage, out_n, nullptr, nreads, st, rows, num, den, stats, cal);
}

__global__ __launch_bounds__(256) void k_stat_pick_ranged(int stage, const uint32_t *out_n, const uint32_t *range, uint32_t nreads,
							   StatRead *st, uint32_t *rows, uint32_t num, uint32_t den, int32_t *stats, float *cal)
{
	stat_pick<true>(stage, out_n, range, nreads, st, rows, num, den, stats, cal);
}

uint64_t stat_rows_bytes(uint32_t nreads) { return (uint64_t) nreads * STAT_ROW * sizeof(uint32_t); }
uint64_t stat_state_bytes(uint32_t nreads) { return (uint64_t) nreads * sizeof(StatRead); }

template <bool MAD>
static void stat_round_ranged(const DecodeArgs &a, const uint32_t *range, const uint2 *tiles, const uint32_t *ntiles, StatRead *st,
			      uint32_t *rows, int32_t *stats, float *cal, hipStream_t s)
{
	const dim3 gc(a.max_chunks), gp((a.nreads + 3) / 4), b(256);
	const int16_t *sig = a.sig;
	const uint32_t *on = a.out_n;
	hipLaunchKernelGGL((k_stat_count<STAT_HI, false, MAD, const uint32_t *>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const StatRead *) st, rows, range);
	hipLaunchKernelGGL(k_stat_pick_ranged, gp, b, 0, s, MAD ? 2 : 0, on, range, a.nreads, st, rows, 1u, 2u, (int32_t *) nullptr, (float *) nullptr);
	hipLaunchKernelGGL((k_stat_count<STAT_LO, true, MAD, const uint32_t *>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const StatRead *) st, rows, range);
	hipLaunchKernelGGL(k_stat_pick_ranged, gp, b, 0, s, MAD ? 3 : 1, on, range, a.nreads, st, rows, 1u, 2u, MAD ? stats : nullptr,
			   MAD ? cal : nullptr);
}

template <bool MAD>
static void stat_round(const DecodeArgs &a, const uint2 *tiles, const uint32_t *ntiles, StatRead *st, uint32_t *rows,
		       int32_t *stats, float *cal, hipEvent_t *ev, hipStream_t s)
{
	const dim3 gc(a.max_chunks), gp((a.nreads + 3) / 4), b(256);
	const int16_t *sig = a.sig;
	const uint32_t *on = a.out_n;
	int e = MAD ? 4 : 0;
	hipLaunchKernelGGL((k_stat_count<STAT_HI, false, MAD>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const StatRead *) st, rows);
	if (ev)
		(void) hipEventRecord(ev[++e], s);
	hipLaunchKernelGGL(k_stat_pick, gp, b, 0, s, MAD ? 2 : 0, on, a.nreads, st, rows, 1u, 2u, (int32_t *) nullptr, (float *) nullptr);
	if (ev)
		(void) hipEventRecord(ev[++e], s);
	hipLaunchKernelGGL((k_stat_count<STAT_LO, true, MAD>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const StatRead *) st, rows);
	if (ev)
		(void) hipEventRecord(ev[++e], s);
	hipLaunchKernelGGL(k_stat_pick, gp, b, 0, s, MAD ? 3 : 1, on, a.nreads, st, rows, 1u, 2u, MAD ? stats : nullptr, MAD ? cal : nullptr);
	if (ev)
		(void) hipEventRecord(ev[++e], s);
}

// med and mad of a.out_n[r] samples at a.sig + a.off[r] (tiles / ntiles: launch_pa_tiles' table of the same batch;
// state, rows: stat_state_bytes, stat_rows_bytes).  stats and cal may be NULL.  ev: NULL, or 9 events - ev[0] is
// recorded in front of the first kernel, ev[1 .. 8] behind each of the eight.
void launch_signal_stats(const DecodeArgs &a, const uint2 *tiles, const uint32_t *ntiles, void *state, uint32_t *rows,
			 int32_t *stats, float *cal, hipEvent_t *ev, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	(void) hipMemsetAsync(rows, 0, stat_rows_bytes(a.nreads), s);
	if (ev)
		(void) hipEventRecord(ev[0], s);
	stat_round<false>(a, tiles, ntiles, (StatRead *) state, rows, stats, cal, ev, s);
	stat_round<true>(a, tiles, ntiles, (StatRead *) state, rows, stats, cal, ev, s);
}

// ... of the samples [a', b') of every read alone (range: 2 words per read, device memory, clamped by the kernels)
void launch_signal_stats_ranged(const DecodeArgs &a, const uint32_t *range, const uint2 *tiles, const uint32_t *ntiles, void *state,
				uint32_t *rows, int32_t *stats, float *cal, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	(void) hipMemsetAsync(rows, 0, stat_rows_bytes(a.nreads), s);
	stat_round_ranged<false>(a, range, tiles, ntiles, (StatRead *) state, rows, stats, cal, s);
	stat_round_ranged<true>(a, range, tiles, ntiles, (StatRead *) state, rows, stats, cal, s);
}

} // namespace ph
