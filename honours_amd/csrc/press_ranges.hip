// press_ranges.hip - sigtk's `stat` and `prefix` on the device (sigtk/src/cfunc.c:126-234, stat.h:17-73, misc.c:15-32), bit
// for bit.  include/press_hip.h has the definitions (press_hip_signal_range_stats, press_hip_signal_prefix), DESIGN.md
// 6.0.30 the arguments; in short:
//
//   k_range_stats  ONE WAVE PER RANGE [a, b) of a read, at any sample offset, in tiles of 64 samples, a lane each, four
//                  tiles in flight (seg_tiles), in TWO passes over the samples:
//                    pass 1  S, the float sum of x in the reference's order (seg_chain), and the counts of the high byte
//                            of the 16-bit keys s + 32768 in 256 LDS counters (ds_add); a wave scan finds the byte that
//                            holds the median's rank
//                    pass 2  Q of (x - mean)^2 likewise, and the counts of the low byte among the keys with that high
//                            byte; the same scan finds the key
//                  The counts ride in the two passes the sums need anyway: a ds_add per tile beside 64 dependent adds.
//                  All counting is on integers, so the median is the same from run to run, and nothing is kept per sample.
//   k_prefix       one wave per read behind k_adaptor: the adaptor's pair, m_a = the ordered picoampere mean of
//                  [adapt_start, adapt_end), the thresholds m_a + shift +- half, and seg_walk<FIRST> - the walk k_segments
//                  runs, press_segwalk.h - over the suffix [adapt_end, n) for its first record; it writes the result,
//                  thr, and the two ranges for k_range_stats
//
// A wave walks its range alone: the time of either call is that of its longest range (read), as the segments' and the
// events' is.

#include "press_segwalk.h"

#pragma clang fp contract(off) // every operation below rounds on its own, as the reference's does (x86-64, no FMA)

namespace ph {

struct RangeStat { // press_hip_range_stat
	float mean, stdv, median;
};
struct PrefixRec { // press_hip_prefix
	int32_t adapt_start, adapt_end, polya_start, polya_end;
};

__device__ __forceinline__ float uni_f32(const float *p) { return __int_as_float((int) uni((uint32_t) __float_as_int(*p))); }

// cnt[0 .. 256) = 0 by the wave
__device__ __forceinline__ void rank_clear(uint32_t *cnt, uint32_t lane)
{
	__syncthreads();
#pragma unroll
	for (uint32_t j = 0; j < 4; j++)
		cnt[lane + 64 * j] = 0;
	__syncthreads();
}

// The digit d with (the sum of cnt[0 .. d)) <= rank < (the sum of cnt[0 .. d]); rank becomes the rank among the keys of
// that digit.  The counts must hold more than `rank` keys.  Wave-uniform
__device__ __forceinline__ uint32_t rank_digit(const uint32_t *cnt, uint32_t lane, uint32_t &rank)
{
	__syncthreads();
	uint32_t c[4];
#pragma unroll
	for (uint32_t j = 0; j < 4; j++)
		c[j] = cnt[4 * lane + j];
	const uint32_t sum = c[0] + c[1] + c[2] + c[3];
	uint32_t incl = sum;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = (uint32_t) __shfl_up((int) incl, d, 64);
		if (lane >= (uint32_t) d)
			incl += o;
	}
	const uint64_t m = __ballot(incl > rank);
	const uint32_t f = m ? (uint32_t) __builtin_ctzll(m) : 63u; // the lane whose four counters hold the rank
	uint32_t before = incl - sum, d = 0;
#pragma unroll
	for (uint32_t j = 0; j < 3; j++)
		if (d == j && rank >= before + c[j]) { // (only lane f's choice is used)
			before += c[j];
			d = j + 1;
		}
	const uint32_t digit = uni((uint32_t) __shfl((int) (4 * lane + d), (int) f, 64));
	rank -= uni((uint32_t) __shfl((int) before, (int) f, 64));
	return digit;
}

// Range idx of read idx >> shift (shift 0: a range per read; 1: two, the prefix call's).  range NULL: the whole read
__global__ __launch_bounds__(64) void k_range_stats(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, const float *cal,
						     const uint32_t *range, uint32_t shift, RangeStat *out)
{
	__shared__ uint32_t cnt[256];
	const uint32_t idx = blockIdx.x, lane = threadIdx.x;
	const uint32_t r = idx >> shift;
	const uint32_t n = uni(nsamp[r]);
	uint32_t a = 0, b = n;
	if (range) {
		b = uni(range[2 * (size_t) idx + 1]);
		b = b < n ? b : n;
		a = uni(range[2 * (size_t) idx]);
		a = a < b ? a : b;
	}
	const uint32_t L = b - a;
	const int16_t *in = sig + uni64(off[r]) + a;
	const bool raw = cal == nullptr;
	float c0 = 0.0f, c1 = 0.0f;
	if (!raw) {
		c0 = uni_f32(cal + 2 * (size_t) r);
		c1 = uni_f32(cal + 2 * (size_t) r + 1);
	}
	// x falls as s rises under a negative scale: the L / 2-th largest sample
	uint32_t rank = !raw && c1 < 0.0f ? L - 1 - L / 2 : L / 2;

	// ---- pass 1: meanf / meani16 (stat.h:17-33), the keys' high bytes
	rank_clear(cnt, lane);
	float S = 0.0f, Q = 0.0f;
	seg_tiles(in, L, lane, [&](uint32_t t, int16_t s) {
		const uint64_t i = (uint64_t) t * 64 + lane;
		if (i < L)
			atomicAdd(&cnt[(((uint32_t) (uint16_t) s) ^ 0x8000u) >> 8], 1u);
		S = seg_chain(S, i < L ? seg_plain_x(s, raw, c0, c1) : 0.0f);
		return true;
	});
	const float Lf = (float) L;
	const float mean = S / Lf;
	const uint32_t hi = L ? rank_digit(cnt, lane, rank) : 0u;

	// ---- pass 2: stdvf / stdvi16 (stat.h:36-54), the low bytes of the keys with that high byte
	rank_clear(cnt, lane);
	seg_tiles(in, L, lane, [&](uint32_t t, int16_t s) {
		const uint64_t i = (uint64_t) t * 64 + lane;
		const uint32_t key = ((uint32_t) (uint16_t) s) ^ 0x8000u;
		if (i < L && key >> 8 == hi)
			atomicAdd(&cnt[key & 255u], 1u);
		const float d = seg_plain_x(s, raw, c0, c1) - mean;
		const float q = d * d;
		Q = seg_chain(Q, i < L ? q : 0.0f);
		return true;
	});
	const float stdv = sqrtf(Q / Lf);
	float median = 0.0f;
	if (L) {
		const uint32_t lo = rank_digit(cnt, lane, rank);
		median = seg_plain_x((int16_t) (uint16_t) (((hi << 8) | lo) ^ 0x8000u), raw, c0, c1);
	}
	if (lane == 0)
		out[idx] = { mean, stdv, median };
}

// pair: k_adaptor's.  range: 4 words per read, the adaptor's range and the poly-A's, 0, 0 for a stretch that is absent
__global__ __launch_bounds__(64) void k_prefix(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, const float *cal, SegParams p,
						int32_t rna, float shift, float half, const int32_t *pair, PrefixRec *out, float *thr,
						uint32_t *range)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const uint32_t n = uni(nsamp[r]);
	const int32_t as = (int32_t) uni((uint32_t) pair[2 * (size_t) r]), ae = (int32_t) uni((uint32_t) pair[2 * (size_t) r + 1]);
	int32_t ps = -1, pe = -1;
	float bot = 0.0f, top = 0.0f;
	if (ae > 0 && rna) {
		// the range as k_range_stats clamps it (a start below 0 is beyond every end: an empty range, a NaN mean)
		const uint32_t b = (uint32_t) ae < n ? (uint32_t) ae : n;
		const uint32_t a = (uint32_t) as < b ? (uint32_t) as : b;
		const uint32_t L = b - a;
		const int16_t *in = sig + uni64(off[r]);
		const float c0 = uni_f32(cal + 2 * (size_t) r), c1 = uni_f32(cal + 2 * (size_t) r + 1);
		float S = 0.0f;
		seg_tiles(in + a, L, lane, [&](uint32_t t, int16_t s) {
			const uint64_t i = (uint64_t) t * 64 + lane;
			S = seg_chain(S, i < L ? seg_plain_x(s, false, c0, c1) : 0.0f);
			return true;
		});
		const float m_a = S / (float) L;
		const float t = m_a + shift; // m_a + 30 + 20 and m_a + 30 - 20, as C evaluates them (cfunc.c:191)
		top = t + half;
		bot = t - half;
		uint32_t fs = 0, fe = 0;
		const uint32_t count = seg_walk<true>(in + b, n - b, lane, false, c0, c1, top, bot, p, [&](uint32_t k, uint32_t start, uint32_t end) {
			if (k == 0) {
				fs = start;
				fe = end;
			}
		});
		if (count) {
			ps = (int32_t) (fs + b);
			pe = (int32_t) (fe + b);
		}
	}
	if (lane == 0) {
		out[r] = { as, ae, ps, pe };
		if (thr) {
			thr[2 * (size_t) r] = bot;
			thr[2 * (size_t) r + 1] = top;
		}
		const bool ad = ae > 0, pa = pe > 0;
		reinterpret_cast<uint4 *>(range)[r] = make_uint4(ad ? (uint32_t) as : 0u, ad ? (uint32_t) ae : 0u, pa ? (uint32_t) ps : 0u,
								  pa ? (uint32_t) pe : 0u);
	}
}

// out[i] of range i (range: 2 * nranges words, or NULL: whole reads) of read i >> shift; cal NULL: the raw domain
void launch_range_stats(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nranges, uint32_t shift, const float *cal,
			const uint32_t *range, void *out, hipStream_t s)
{
	ktime_begin(1, s);
	hipLaunchKernelGGL(k_range_stats, dim3(nranges), dim3(64), 0, s, sig, off, n, cal, range, shift, (RangeStat *) out);
	ktime_end(1, s);
}

// behind launch_adaptor on the same stream: out (16 bytes per read), thr (NULL, or 2 * nreads) and range (16 bytes per read)
void launch_prefix(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal, const SegParams &polya,
		   int32_t rna, float shift, float half, const int32_t *pair, void *out, float *thr, uint32_t *range, hipStream_t s)
{
	ktime_begin(1, s);
	hipLaunchKernelGGL(k_prefix, dim3(nreads), dim3(64), 0, s, sig, off, n, cal, polya, rna, shift, half, pair, (PrefixRec *) out, thr,
			   range);
	ktime_end(1, s);
}

} // namespace ph
