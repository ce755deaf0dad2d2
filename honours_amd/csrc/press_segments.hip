// press_segments.hip - sigtk's jnn segmenter (press_hip_signal_segments: jnn_core over jnn_raw / jnn_pa, sigtk/src/jnn.c:185-301)
// and its jnnv2 adaptor finder (press_hip_signal_adaptor, jnn.c:98-178), bit for bit.  DESIGN.md 6.0.28 has the arguments;
// in short:
//
//   k_segments<false>  ONE WAVE PER READ, three passes over the read in tiles of 64 samples, a lane each, four tiles in
//                      flight.  Pass 1: S, the float sum of x in the reference's order - 64 dependent adds per tile on
//                      values read lane by lane into a wave-uniform carry.  Pass 2: Q of (x - mn)^2 likewise.  (Both only
//                      for std_scale > 0.)  Pass 3: the walk.  __ballot of x < top && x > bot is the tile as one
//                      wave-uniform 64-bit mask, and jnn_core's state machine is stepped over it in scalar registers by
//                      uniform branches; the stretches where nothing can happen are jumped with a find-first-set.  This
//                      launch only counts; it leaves the count and the two thresholds per read (16 bytes).
//   k_records_scan     (press_events.hip) one wave: seg_first[] = the exclusive sums of the counts, seg_count[] with the
//                      reads that do not fit
//   k_segments<true>   pass 3 again with the thresholds of the first launch, for the reads that fit, writing the records
//   k_adaptor          one wave per read, the same three passes over t[j], the rolling mean of `window` samples; the
//                      window sums are integers (below 2^24, so the reference's rolling float sum never rounds): the sum
//                      at a tile's first position is carried, the others come from a wave scan of s[j + window] - s[j]
//
// The tile loader, the ordered sums and the walk itself are press_segwalk.h's: press_ranges.hip walks with them too.

#include <stddef.h>

#include "press_segwalk.h"

#pragma clang fp contract(off) // every operation below rounds on its own, as the reference's does (x86-64, no FMA)

namespace ph {

struct SegRec { // press_hip_segment
	uint32_t start, end;
};
struct SegState { // per read, between the launches (16 bytes); the count comes first: launch_records_scan reads it there
	uint32_t count, pad;
	float bot, top;
};
static_assert(offsetof(SegState, count) == 0, "k_records_scan: the count is the first word of a state record");

// One block of 64 lanes per read.  WRITE: the records of a read that fits; else its count and its thresholds.
// FIRST (with !WRITE; the stall methods, press_stall.hip): one launch that keeps segs[0] alone - seg[r] is the read's
// first record once no merge can change it, start = SEG_NONE for a read without one, and the walk stops there
template <bool WRITE, bool FIRST = false>
__global__ __launch_bounds__(64) void k_segments(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, const float *cal,
						  SegParams p, SegState *state, float *thr, SegRec *seg, uint64_t seg_cap,
						  const uint64_t *seg_first)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const uint32_t n = uni(nsamp[r]);
	const bool given = !(p.std_scale > 0.0f);
	uint64_t first = 0, room = 0; // the read's records: seg[first .. first + room)
	if (WRITE) {
		first = uni64(seg_first[r]);
		const uint64_t end = uni64(seg_first[r + 1]);
		if (n == 0 || end > seg_cap || end <= first)
			return;
		room = end - first;
	} else if (n == 0) { // no segment and no thresholds of its own
		if (lane == 0) {
			if (FIRST)
				seg[r] = { SEG_NONE, 0u };
			state[r] = { 0u, 0u, given ? p.bot : 0.0f, given ? p.top : 0.0f };
			if (thr) {
				thr[2 * (size_t) r] = given ? p.bot : 0.0f;
				thr[2 * (size_t) r + 1] = given ? p.top : 0.0f;
			}
		}
		return;
	}
	const int16_t *in = sig + uni64(off[r]);
	const bool raw = cal == nullptr;
	float c0 = 0.0f, c1 = 0.0f;
	if (!raw) {
		c0 = __int_as_float((int) uni((uint32_t) __float_as_int(cal[2 * (size_t) r])));
		c1 = __int_as_float((int) uni((uint32_t) __float_as_int(cal[2 * (size_t) r + 1])));
	}

	float top = p.top, bot = p.bot;
	if (WRITE) {
		bot = __int_as_float((int) uni((uint32_t) __float_as_int(state[r].bot)));
		top = __int_as_float((int) uni((uint32_t) __float_as_int(state[r].top)));
	} else if (!given) { // meanf, stdvf (stat.h:17-44)
		float S = 0.0f, Q = 0.0f;
		seg_tiles(in, n, lane, [&](uint32_t t, int16_t s) {
			const uint64_t i = (uint64_t) t * 64 + lane;
			S = seg_chain(S, i < n ? seg_x(s, raw, c0, c1) : 0.0f);
			return true;
		});
		const float nf = (float) n;
		const float mn = S / nf;
		seg_tiles(in, n, lane, [&](uint32_t t, int16_t s) {
			const uint64_t i = (uint64_t) t * 64 + lane;
			const float d = seg_x(s, raw, c0, c1) - mn;
			const float q = d * d;
			Q = seg_chain(Q, i < n ? q : 0.0f);
			return true;
		});
		const float sd = sqrtf(Q / nf);
		const float k = sd * p.std_scale;
		top = mn + k;
		bot = mn - k;
	}

	// ---- the walk (jnn.c:217-268)
	const uint32_t count = seg_walk<FIRST>(in, n, lane, raw, c0, c1, top, bot, p, [&](uint32_t k, uint32_t start, uint32_t end) {
		if (FIRST && lane == 0 && k == 0)
			seg[r] = { start, end };
		if (WRITE && lane == 0 && (uint64_t) k < room)
			seg[first + k] = { start, end };
	});
	if (FIRST && lane == 0 && count == 0)
		seg[r] = { SEG_NONE, 0u };
	if (!WRITE && lane == 0) {
		state[r] = { count, 0u, bot, top };
		if (thr) {
			thr[2 * (size_t) r] = bot;
			thr[2 * (size_t) r + 1] = top;
		}
	}
}

// ------------------------------------------------------------------ jnnv2

// f(t, tv, valid): tile t of the m = n - window rolling means, tv the lane's (valid: its position is below m); f returns
// false to stop.  W: the integer sum of the window at the tile's first position
template <class F>
__device__ __forceinline__ void adaptor_tiles(const int16_t *in, uint32_t m, uint32_t window, uint32_t W, uint32_t lane, F &&f)
{
	const uint32_t ntile = (uint32_t) (((uint64_t) m + 63) / 64);
	const float wf = (float) window;
	int32_t cur[SEG_AHEAD], nxt[SEG_AHEAD]; // s[j + window] - s[j], clamped each; 0 beyond m
	auto load = [&](uint32_t t0, int32_t *v) {
#pragma unroll
		for (uint32_t k = 0; k < SEG_AHEAD; k++) {
			const uint64_t j = (uint64_t) (t0 + k) * 64 + lane;
			v[k] = j < m ? seg_clamp(in[j + window]) - seg_clamp(in[j]) : 0;
		}
	};
	load(0, cur);
	for (uint32_t t0 = 0; t0 < ntile; t0 += SEG_AHEAD) {
		load(t0 + SEG_AHEAD, nxt);
#pragma unroll
		for (uint32_t k = 0; k < SEG_AHEAD; k++) {
			if (t0 + k < ntile) {
				int32_t inc = cur[k];
#pragma unroll
				for (int d = 1; d < 64; d <<= 1) {
					const int32_t o = __shfl_up(inc, d, 64);
					if (lane >= (uint32_t) d)
						inc += o;
				}
				const uint32_t Wj = W + (uint32_t) (inc - cur[k]); // 0 .. 1200 * window < 2^24: the float is exact
				const uint64_t j = (uint64_t) (t0 + k) * 64 + lane;
				if (!f(t0 + k, (float) Wj / wf, j < m))
					return;
				W += (uint32_t) __builtin_amdgcn_readlane(inc, 63);
			}
			cur[k] = nxt[k];
		}
	}
}

__global__ __launch_bounds__(64) void k_adaptor(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, Seg2Params p,
						 int32_t *pair, float *thr)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const uint32_t n = uni(nsamp[r]);
	const uint32_t window = (uint32_t) p.window;
	if (n <= window) { // (jnn.c:172)
		if (lane == 0) {
			pair[2 * (size_t) r] = pair[2 * (size_t) r + 1] = -1;
			if (thr)
				thr[2 * (size_t) r] = thr[2 * (size_t) r + 1] = 0.0f;
		}
		return;
	}
	const int16_t *in = sig + uni64(off[r]);
	const uint32_t m = n - window;
	uint32_t W0 = 0;
	for (uint32_t i = lane; i < window; i += 64)
		W0 += (uint32_t) seg_clamp(in[i]);
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		W0 += (uint32_t) __shfl_xor((int) W0, d, 64);
	W0 = uni(W0);

	float S = 0.0f, Q = 0.0f;
	adaptor_tiles(in, m, window, W0, lane, [&](uint32_t, float tv, bool valid) {
		S = seg_chain(S, valid ? tv : 0.0f);
		return true;
	});
	const float mf = (float) m;
	const float mn = S / mf;
	adaptor_tiles(in, m, window, W0, lane, [&](uint32_t, float tv, bool valid) {
		const float d = tv - mn;
		const float q = d * d;
		Q = seg_chain(Q, valid ? q : 0.0f);
		return true;
	});
	const float sd = sqrtf(Q / mf);
	const float bot = mn - sd * p.std_scale;

	// ---- the walk (jnn.c:124-151) and the choice (jnn.c:152-166): the first record, once no merge can change it, with
	// lo_thresh <= y - x <= hi_thresh
	bool begin = false, has = false, found = false;
	uint32_t start = 0, end = 0, lx = 0, ly = 0; // lx, ly: the last record
	auto final_ok = [&]() {
		const int64_t d = (int64_t) ly - (int64_t) lx;
		return d <= (int64_t) p.hi_thresh && d >= (int64_t) p.lo_thresh;
	};
	adaptor_tiles(in, m, window, W0, lane, [&](uint32_t t, float tv, bool valid) {
		const uint32_t base = t * 64;
		const uint64_t lt = __ballot(valid && tv < bot), gt = __ballot(valid && tv > bot);
		uint32_t pos = 0;
		while (pos < 64) {
			const uint64_t rl = lt >> pos, rg = gt >> pos;
			if (!begin) { // nothing happens before the next value below bot
				if (!rl)
					break;
				pos += (uint32_t) __builtin_ctzll(rl);
				start = base + pos;
				begin = true;
				pos++;
				continue;
			}
			// end is the last value below bot before the first one above it
			const uint32_t g = rg ? (uint32_t) __builtin_ctzll(rg) : 64u;
			const uint64_t below = g < 64 ? rl & ((1ull << g) - 1) : rl;
			if (below)
				end = base + pos + 63u - (uint32_t) __builtin_clzll(below);
			if (!rg)
				break;
			if (has && (int64_t) start - (int64_t) ly < (int64_t) p.seg_dist) {
				ly = end;
			} else {
				if (has && final_ok()) {
					found = true;
					return false;
				}
				lx = start;
				ly = end;
				has = true;
			}
			start = 0;
			end = 0;
			begin = false;
			pos += g + 1;
		}
		return true;
	});
	if (!found && has && final_ok())
		found = true;
	if (lane == 0) {
		const uint32_t shift = window / 2 - 1;
		pair[2 * (size_t) r] = found ? (int32_t) (lx + shift) : 0;
		pair[2 * (size_t) r + 1] = found ? (int32_t) (ly + shift) : 0;
		if (thr) {
			thr[2 * (size_t) r] = bot;
			thr[2 * (size_t) r + 1] = mn;
		}
	}
}

uint64_t segments_state_bytes(uint32_t nreads) { return (uint64_t) nreads * sizeof(SegState); }

// The counting walk and the layout: seg_first (nreads + 1), seg_count and thr (unless NULL) are written; state:
// segments_state_bytes.  cal NULL: the raw domain
void launch_segments_count(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal,
			   const SegParams &p, void *state, uint64_t seg_cap, uint64_t *seg_first, uint32_t *seg_count, float *thr,
			   hipStream_t s)
{
	ktime_begin(1, s);
	hipLaunchKernelGGL((k_segments<false>), dim3(nreads), dim3(64), 0, s, sig, off, n, cal, p, (SegState *) state, thr,
			   (SegRec *) nullptr, seg_cap, (const uint64_t *) nullptr);
	ktime_end(1, s);
	ktime_begin(1, s);
	launch_records_scan(state, sizeof(SegState), nreads, seg_cap, seg_first, seg_count, s);
	ktime_end(1, s);
}

// The writing walk behind launch_segments_count on the same stream: the records of the reads with seg_first[r + 1] <= seg_cap
void launch_segments_write(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal,
			   const SegParams &p, void *state, void *seg, uint64_t seg_cap, const uint64_t *seg_first, hipStream_t s)
{
	ktime_begin(1, s);
	hipLaunchKernelGGL((k_segments<true>), dim3(nreads), dim3(64), 0, s, sig, off, n, cal, p, (SegState *) state, (float *) nullptr,
			   (SegRec *) seg, seg_cap, seg_first);
	ktime_end(1, s);
}

// The first record of every read in one launch (first: 8 bytes per read, start = 0xFFFFFFFF: none); state as above;
// cal NULL: the raw domain
void launch_segments_first(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const SegParams &p, void *state,
			   void *first, hipStream_t s, const float *cal)
{
	ktime_begin(1, s);
	hipLaunchKernelGGL((k_segments<false, true>), dim3(nreads), dim3(64), 0, s, sig, off, n, cal, p,
			   (SegState *) state, (float *) nullptr, (SegRec *) first, (uint64_t) 0, (const uint64_t *) nullptr);
	ktime_end(1, s);
}

void launch_adaptor(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const Seg2Params &p, int32_t *pair,
		    float *thr, hipStream_t s)
{
	ktime_begin(1, s);
	hipLaunchKernelGGL(k_adaptor, dim3(nreads), dim3(64), 0, s, sig, off, n, p, pair, thr);
	ktime_end(1, s);
}

} // namespace ph
