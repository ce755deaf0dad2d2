// press_segwalk.h - what the kernels of press_segments.hip and press_ranges.hip share: the tile loader, the sums in the
// reference's order, and jnn_core's walk (sigtk/src/jnn.c:200-268).  Device code only.
//
// A sum starting at +0 is never -0 (a + b = -0 only for a = b = -0), so the +0 that the lanes beyond n add changes nothing.
#pragma once

#include "press_internal.h"
#include "press_wave.h"

#pragma clang fp contract(off) // every operation below rounds on its own, as the reference's does (x86-64, no FMA)

namespace ph {

constexpr uint32_t SEG_NONE = 0xFFFFFFFFu; // launch_segments_first: start of a read without a segment (press_internal.h: STALL_NOSEG)
constexpr uint32_t SEG_AHEAD = 4; // tiles whose loads are in flight while a group of as many is worked on

// carry + v[0] + v[1] + ... + v[63], added in that order
__device__ __forceinline__ float seg_chain(float carry, float v)
{
#pragma unroll
	for (uint32_t j = 0; j < 64; j++)
		carry = carry + lane_f32(v, j);
	return carry;
}

__device__ __forceinline__ int32_t seg_clamp(int16_t s) { return s > 1200 ? 1200 : s < 0 ? 0 : (int32_t) s; }

// rm_outlier / rm_outlierf (jnn.c:60-94): a NaN is in neither branch and stays
__device__ __forceinline__ float seg_x(int16_t s, bool raw, float c0, float c1)
{
	if (raw)
		return (float) seg_clamp(s);
	const float a = (float) s + c0;
	const float p = a * c1;
	return p > 1200.0f ? 1200.0f : p < 0.0f ? 0.0f : p;
}

// the sample as it is (meani16, stat.h:26) or as signal_in_picoamps has it (misc.c:28): no clamp
__device__ __forceinline__ float seg_plain_x(int16_t s, bool raw, float c0, float c1)
{
	if (raw)
		return (float) s;
	const float a = (float) s + c0;
	return a * c1;
}

// f(t, s): tile t of the n samples at in, s the lane's sample (0 beyond n); f returns false to stop.  `in` needs the
// alignment of a sample only, and no load leaves [in, in + n)
template <class F>
__device__ __forceinline__ void seg_tiles(const int16_t *in, uint32_t n, uint32_t lane, F &&f)
{
	const uint32_t ntile = (uint32_t) (((uint64_t) n + 63) / 64);
	int16_t cur[SEG_AHEAD], nxt[SEG_AHEAD];
	auto load = [&](uint32_t t0, int16_t *v) {
#pragma unroll
		for (uint32_t k = 0; k < SEG_AHEAD; k++) {
			const uint64_t i = (uint64_t) (t0 + k) * 64 + lane;
			v[k] = i < n ? in[i] : (int16_t) 0;
		}
	};
	load(0, cur);
	for (uint32_t t0 = 0; t0 < ntile; t0 += SEG_AHEAD) {
		load(t0 + SEG_AHEAD, nxt);
#pragma unroll
		for (uint32_t k = 0; k < SEG_AHEAD; k++) {
			if (t0 + k < ntile && !f(t0 + k, cur[k]))
				return;
			cur[k] = nxt[k];
		}
	}
}

struct SegWalk { // jnn_core's state (jnn.c:200-215) with exact integers, and the last record, which a merge may still change
	bool prev;
	uint32_t c, prev_err, start, count, last_start, last_end;
	uint64_t w;
	int64_t err;
};

// The walk (jnn.c:217-268) over the n samples at in, as x = seg_x(s, raw, c0, c1), with x < top && x > bot in range.
// __ballot of that is the tile as one wave-uniform 64-bit mask, and the state machine is stepped over it in scalar
// registers by uniform branches; the stretches where nothing can happen are jumped with a find-first-set.
// emit(k, start, end), on every lane: record k is [start, end) and no merge can change it any more.  FIRST: the walk stops
// once record 0 is final.  Returns the count (FIRST: 2 where the walk stopped early)
template <bool FIRST, class Emit>
__device__ __forceinline__ uint32_t seg_walk(const int16_t *in, uint32_t n, uint32_t lane, bool raw, float c0, float c1, float top,
					     float bot, const SegParams &p, Emit &&emit)
{
	const uint32_t window = (uint32_t) p.window;
	const float stall = (float) p.window * p.stall_len;
	SegWalk a = { false, 0u, 0u, 0u, 0u, 0u, 0u, (uint64_t) (uint32_t) p.corrector, 0 };
	auto flush = [&]() { emit(a.count - 1, a.last_start, a.last_end); }; // the last record is final
	auto grown = [&]() { // c and w have just been raised
		if (a.c >= window && (uint64_t) a.c >= a.w && a.c % (uint32_t) a.w == 0)
			a.err--;
	};
	seg_tiles(in, n, lane, [&](uint32_t t, int16_t s) {
		const uint32_t base = t * 64;
		const uint64_t i = (uint64_t) base + lane;
		const float x = seg_x(s, raw, c0, c1);
		const uint64_t mask = __ballot(i < n && x < top && x > bot);
		const uint32_t here = n - base < 64 ? n - base : 64;
		uint32_t pos = 0;
		while (pos < here) {
			uint64_t rest = mask >> pos;
			if (!a.prev) { // an out-of-range sample changes nothing
				if (!rest)
					break;
				pos += (uint32_t) __builtin_ctzll(rest);
				rest = mask >> pos;
			}
			if (rest & 1) {
				if (!a.prev) {
					a.start = base + pos;
					a.prev = true;
				}
				a.prev_err = 0;
				if ((uint64_t) a.c < a.w) { // c and w rise together: c >= w at no sample of the run, err stays
					const uint32_t k = ~rest ? (uint32_t) __builtin_ctzll(~rest) : 64u;
					a.c += k;
					a.w += k;
					pos += k;
				} else {
					a.c++;
					a.w++;
					grown();
					pos++;
				}
				continue;
			}
			// out of range behind an in-range sample
			if (a.err < (int64_t) p.error) {
				a.c++;
				a.err++;
				a.prev_err++;
				grown();
			} else {
				if (a.c >= window || (a.count == 0 && (float) a.c >= stall)) {
					const uint32_t end = base + pos - a.prev_err;
					if (a.count && (int64_t) a.start - (int64_t) a.last_end < (int64_t) p.seg_dist) {
						a.last_end = end;
					} else {
						if (a.count)
							flush();
						a.last_start = a.start;
						a.last_end = end;
						a.count++;
					}
				}
				a.prev = false;
				a.c = 0;
				a.err = 0;
				a.prev_err = 0;
			}
			pos++;
		}
		return !(FIRST && a.count >= 2); // (the first record was flushed when the second began)
	});
	if (a.count)
		flush();
	return a.count;
}

} // namespace ph
