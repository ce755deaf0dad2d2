// press_events.hip - event detection (press_hip_signal_events): scrappie's detector as sigtk carries it
// (sigtk/src/events.c:293-550, detect_events), on the picoampere floats x[i] = ((float) s[i] + c0) * c1 of the samples,
// bit for bit in the reference's precisions.  DESIGN.md 6.0.26 has the arguments; in short:
//
//   k_events<false>   ONE WAVE PER READ walks the read in tiles of 64 positions, a lane each.  Per tile: the running sums
//                     S, Q (double) of x and of the rounded squares, into an LDS ring of four tiles; the two t-statistics
//                     of the tile BEFORE (a position needs the sums of w <= 64 positions ahead), a lane each; then the two
//                     coupled peak detectors are stepped over those 64 values in order, every lane running the same state
//                     machine on values read with v_readlane.  The doubles never reach memory: a detector keeps S and Q of
//                     its pending peak, and an event is made of the sums at its two boundaries when the peak is emitted.
//                     This launch only counts.
//   k_records_scan    one wave: ev_first[] = the exclusive sums of the counts, ev_count[] with the reads that do not fit
//                     (the segments' layout too: launch_records_scan)
//   k_events<true>    the same walk again, for the reads that fit, writing the records at ev_first[r]
//
// The sums.  The reference adds sequentially (events.c:299-302).  Before the walk the wave looks at the whole read once:
// every non-zero x is a multiple of 2^q, and n * max|x| < 2^(q + 53), likewise for the squares with their own q.  Then
// every partial sum of the read, in any order, is a multiple of 2^q below 2^(q + 53): a double, no add rounds, and a wave
// scan plus the carry of the tiles before IS the sequential sum.  A read that fails the test (NaN, inf, a calibration
// that makes tiny and large values meet) takes sums that add in the reference's order, 64 dependent adds per tile on
// values read lane by lane; it is counted in g_ev_serial (press_hip_events_serial_reads).
//
// The sign of a zero sum: S[0] = +0, and a sum that starts at +0 is never -0 (x + y = -0 only for x = y = -0), in either
// scheme: the carry is +0 or not zero, so carry + (a tile's -0) is +0 as the sequential sum is.

#include <float.h>
#include <stddef.h>

#include "press_internal.h"
#include "press_wave.h"

#pragma clang fp contract(off) // every operation below rounds on its own, as the reference's does (x86-64, no FMA)

namespace ph {

constexpr uint32_t EV_RING = 256; // S, Q of positions [64 (t - 2), 64 (t + 1)] while tile t - 1 is worked on
constexpr uint32_t REC_NOFIT = 0xFFFFFFFFu; // count[r] of a read whose records do not fit (either record call)

struct EvRec { // press_hip_event
	uint32_t start, length;
	float mean, stdv;
};
struct EvState { // per read, between the launches (8 bytes); the count comes first: k_records_scan reads it there
	uint32_t count, serial;
};
static_assert(offsetof(EvState, count) == 0, "k_records_scan: the count is the first word of a state record");

__device__ uint32_t g_ev_serial; // reads whose sums took the serial path, since the library was loaded

__device__ __forceinline__ double wave_incl_f64(double v, uint32_t lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const double o = __shfl_up(v, d, 64);
		if (lane >= (uint32_t) d)
			v = o + v;
	}
	return v;
}

// What the no-rounding test keeps of one float: the largest magnitude (as bits: the order of non-negative floats) and the
// smallest exponent of a lowest set bit, v = odd * 2^low.  Zero takes no part.
__device__ __forceinline__ void exact_fold(float v, uint32_t &top, int32_t &low)
{
	const uint32_t b = (uint32_t) __float_as_int(v) & 0x7FFFFFFFu;
	if (b == 0)
		return;
	const uint32_t e = b >> 23, m = e ? (b & 0x7FFFFFu) | 0x800000u : b;
	const int32_t l = (int32_t) __builtin_ctz(m) + (int32_t) (e ? e : 1u) - 150;
	top = b > top ? b : top;
	low = l < low ? l : low;
}

// |v| < 2^E for every v folded, n <= 2^L: n * max|v| < 2^(E + L) <= 2^(low + 53)?  (inf and NaN: never)
__device__ __forceinline__ bool exact_ok(uint32_t top, int32_t low, uint32_t n)
{
	if (top == 0)
		return true;
	const uint32_t e = top >> 23;
	if (e == 255)
		return false;
	const int32_t E = (int32_t) (e ? e : 1u) - 126;
	const int32_t L = n <= 1 ? 0 : 32 - (int32_t) __builtin_clz(n - 1);
	return E + L <= low + 53;
}

// events.c:338-361 for one position; s0, s1, s2 = S[i - w], S[i], S[i + w], q* likewise
__device__ __forceinline__ float ev_tstat(double s0, double s1, double s2, double q0, double q1, double q2, float wf)
{
	const double sum1 = s1 - s0, sumsq1 = q1 - q0;
	const float sum2 = (float) (s2 - s1), sumsq2 = (float) (q2 - q1);
	const float mean1 = (float) (sum1 / (double) wf);
	const float mean2 = sum2 / wf;
	double cv = sumsq1 / (double) wf;
	cv = cv - (double) (mean1 * mean1);
	cv = cv + (double) (sumsq2 / wf);
	cv = cv - (double) (mean2 * mean2);
	const float var = fmaxf((float) cv, FLT_MIN);
	const float delta = mean2 - mean1;
	return (float) (fabs((double) delta) / sqrt((double) (var / wf)));
}

// events.c:457-473
__device__ __forceinline__ EvRec ev_make(uint32_t start, uint32_t end, double s0, double s1, double q0, double q1)
{
	EvRec e;
	e.start = start;
	e.length = end - start;
	const float len = (float) e.length;
	e.mean = (float) (s1 - s0) / len;
	const float dq = (float) (q1 - q0);
	const float var = dq / len - e.mean * e.mean;
	e.stdv = sqrtf(fmaxf(var, 0.0f));
	return e;
}

struct EvDet { // one detector of events.c:269-280; pos is valid while has (the reference's peak_pos != -1)
	float pval;
	uint32_t pos;
	bool has, valid;
	double s, q; // S, Q at pos once its tile is behind
};

// One block of 64 lanes per read.  WRITE: the records of a read that fits; else its count and whether its sums are serial.
template <bool WRITE>
__global__ __launch_bounds__(64) void k_events(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, const float *cal,
						uint32_t w1, uint32_t w2, float thr1, float thr2, float height, EvState *state,
						EvRec *ev, uint64_t ev_cap, const uint64_t *ev_first)
{
	__shared__ double s_S[EV_RING], s_Q[EV_RING];
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const uint32_t n = uni(nsamp[r]);
	uint64_t first = 0, room = 0; // the read's records: ev[first .. first + room)
	if (WRITE) {
		first = uni64(ev_first[r]);
		const uint64_t end = uni64(ev_first[r + 1]);
		if (n == 0 || end > ev_cap || end < first)
			return;
		room = end - first;
	} else if (n == 0) {
		if (lane == 0)
			state[r] = { 0u, 0u };
		return;
	}
	const int16_t *in = sig + uni64(off[r]);
	const float c0 = __int_as_float((int) uni((uint32_t) __float_as_int(cal[2 * (size_t) r])));
	const float c1 = __int_as_float((int) uni((uint32_t) __float_as_int(cal[2 * (size_t) r + 1])));

	bool serial;
	if (WRITE) {
		serial = uni(state[r].serial) != 0;
	} else {
		uint32_t tx = 0, ty = 0;
		int32_t lx = 1000, ly = 1000;
		for (uint32_t i = lane; i < n; i += 64) {
			const float t = (float) in[i] + c0;
			const float x = t * c1;
			exact_fold(x, tx, lx);
			exact_fold(x * x, ty, ly);
			if (i + 64 < i)
				break; // (n within 64 of 2^32)
		}
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			const uint32_t ox = (uint32_t) __shfl_xor((int) tx, d, 64), oy = (uint32_t) __shfl_xor((int) ty, d, 64);
			const int32_t olx = __shfl_xor(lx, d, 64), oly = __shfl_xor(ly, d, 64);
			tx = ox > tx ? ox : tx;
			ty = oy > ty ? oy : ty;
			lx = olx < lx ? olx : lx;
			ly = oly < ly ? oly : ly;
		}
		serial = uni(exact_ok(tx, lx, n) && exact_ok(ty, ly, n) ? 0u : 1u) != 0;
	}

	if (lane == 0) {
		s_S[0] = 0.0;
		s_Q[0] = 0.0;
	}
	const float wf1 = (float) w1, wf2 = (float) w2;
	const uint32_t ntile = (uint32_t) (((uint64_t) n + 63) / 64);
	double carry_s = 0.0, carry_q = 0.0; // S, Q at the end of the tiles summed so far
	EvDet ds = { FLT_MAX, 0, false, false, 0.0, 0.0 }, dl = ds;
	uint32_t masked = 0;                 // the long detector's masked_to (the short one's stays 0)
	uint32_t prev = 0, count = 0;        // the last boundary, the events so far
	double prev_s = 0.0, prev_q = 0.0;

	for (uint32_t t = 0; t <= ntile; t++) {
		if (t < ntile) { // ---- the sums of tile t
			const uint64_t i = (uint64_t) t * 64 + lane;
			float x = 0.0f;
			if (i < n) {
				const float a = (float) in[i] + c0;
				x = a * c1;
			}
			const double xd = (double) x, yd = (double) (x * x);
			double si, qi;
			if (!serial) {
				si = carry_s + wave_incl_f64(xd, lane);
				qi = carry_q + wave_incl_f64(yd, lane);
				carry_s = lane_f64(si, 63);
				carry_q = lane_f64(qi, 63);
			} else {
				si = qi = 0.0;
				for (uint32_t j = 0; j < 64; j++) {
					carry_s = carry_s + lane_f64(xd, j);
					carry_q = carry_q + lane_f64(yd, j);
					if (lane == j) {
						si = carry_s;
						qi = carry_q;
					}
				}
			}
			// (positions beyond n add +0: S[n] is the carry behind the last tile, and nothing reads S beyond n)
			s_S[(i + 1) & (EV_RING - 1)] = si;
			s_Q[(i + 1) & (EV_RING - 1)] = qi;
		}
		__syncthreads();
		if (t == 0)
			continue;
		// ---- tile t - 1: the t-statistics, a lane each
		const uint32_t base = (t - 1) * 64;
		const uint64_t i = (uint64_t) base + lane;
		const double s1 = s_S[i & (EV_RING - 1)], q1 = s_Q[i & (EV_RING - 1)];
		float t1 = 0.0f, t2 = 0.0f;
		if (n >= 2 * w1 && i >= w1 && i + w1 <= n)
			t1 = ev_tstat(s_S[(i - w1) & (EV_RING - 1)], s1, s_S[(i + w1) & (EV_RING - 1)], s_Q[(i - w1) & (EV_RING - 1)], q1,
				      s_Q[(i + w1) & (EV_RING - 1)], wf1);
		if (n >= 2 * w2 && i >= w2 && i + w2 <= n)
			t2 = ev_tstat(s_S[(i - w2) & (EV_RING - 1)], s1, s_S[(i + w2) & (EV_RING - 1)], s_Q[(i - w2) & (EV_RING - 1)], q1,
				      s_Q[(i + w2) & (EV_RING - 1)], wf2);
		__syncthreads(); // (the next tile's sums overwrite S[64 (t - 2)])

		// ---- the detectors over the tile, in order; every lane holds the same state (events.c:383-440)
		const uint32_t here = n - base < 64 ? n - base : 64;
		auto emit = [&](EvDet &d) {
			double es = d.s, eq = d.q;
			if (d.pos >= base) {
				es = lane_f64(s1, uni(d.pos - base));
				eq = lane_f64(q1, uni(d.pos - base));
			}
			if (WRITE) {
				const EvRec e = ev_make(prev, d.pos, prev_s, es, prev_q, eq);
				if (lane == 0 && count < room)
					ev[first + count] = e;
			}
			count++;
			prev = d.pos;
			prev_s = es;
			prev_q = eq;
		};
		auto step = [&](EvDet &d, float cur, uint32_t pos, float thr, uint32_t w, bool is_short) {
			if (!d.has) {
				if (cur < d.pval) {
					d.pval = cur;
				} else if (cur - d.pval > height) {
					d.pval = cur;
					d.pos = pos;
					d.has = true;
				}
				return;
			}
			if (cur > d.pval) {
				d.pval = cur;
				d.pos = pos;
			}
			if (is_short && d.pval > thr) {
				const uint64_t m = (uint64_t) d.pos + w;
				masked = m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) m;
				dl.has = false;
				dl.pval = FLT_MAX;
				dl.valid = false;
			}
			if (d.pval - cur > height && d.pval > thr)
				d.valid = true;
			if (uni(d.valid && pos - d.pos > w / 2 ? 1u : 0u)) {
				emit(d);
				d.has = false;
				d.pval = cur;
				d.valid = false;
			}
		};
		for (uint32_t j = 0; j < here; j++) {
			const uint32_t pos = base + j;
			const float a = lane_f32(t1, j), b = lane_f32(t2, j);
			if (pos != 0)
				step(ds, a, pos, thr1, w1, true);
			if (masked < pos)
				step(dl, b, pos, thr2, w2, false);
		}
		// a pending peak of this tile: its sums, before the ring moves on
		if (uni(ds.has && ds.pos >= base ? 1u : 0u)) {
			ds.s = lane_f64(s1, uni(ds.pos - base));
			ds.q = lane_f64(q1, uni(ds.pos - base));
		}
		if (uni(dl.has && dl.pos >= base ? 1u : 0u)) {
			dl.s = lane_f64(s1, uni(dl.pos - base));
			dl.q = lane_f64(q1, uni(dl.pos - base));
		}
	}
	// the last event ends at n; a read without a peak is this one event
	if (WRITE) {
		const EvRec e = ev_make(prev, n, prev_s, carry_s, prev_q, carry_q);
		if (lane == 0 && count < room)
			ev[first + count] = e;
	} else if (lane == 0) {
		state[r] = { count + 1, serial ? 1u : 0u };
		if (serial)
			atomicAdd(&g_ev_serial, 1u);
	}
}

// One wave, the layout of either record call (launch_records_scan, press_internal.h): first[0] = 0, first[r + 1] =
// first[r] + count of read r; count[r] = that count where the read fits below cap.  The count is the first word of a
// state record of `stride` bytes (EvState, SegState)
__global__ __launch_bounds__(64) void k_records_scan(const uint8_t *state, uint32_t stride, uint32_t nreads, uint64_t cap, uint64_t *first,
						      uint32_t *count)
{
	const uint32_t lane = threadIdx.x;
	uint64_t before = 0;
	if (lane == 0)
		first[0] = 0;
	for (uint32_t r0 = 0; r0 < nreads; r0 += 64) {
		const uint32_t r = r0 + lane;
		const uint32_t c = r < nreads && r >= r0 ? *reinterpret_cast<const uint32_t *>(state + (size_t) r * stride) : 0u;
		const uint64_t inc = wave_incl_scan64(c, lane);
		if (r < nreads && r >= r0) {
			first[(size_t) r + 1] = before + inc;
			count[r] = before + inc <= cap ? c : REC_NOFIT;
		}
		before += __shfl(inc, 63, 64);
		if (r0 + 64 < r0)
			break;
	}
}

void launch_records_scan(const void *state, uint32_t state_stride, uint32_t nreads, uint64_t cap, uint64_t *first, uint32_t *count,
			 hipStream_t s)
{
	hipLaunchKernelGGL(k_records_scan, dim3(1), dim3(64), 0, s, (const uint8_t *) state, state_stride, nreads, cap, first, count);
}

uint64_t events_state_bytes(uint32_t nreads) { return (uint64_t) nreads * sizeof(EvState); }

// The counting walk and the layout: ev_first (nreads + 1) and ev_count are written; state: events_state_bytes
void launch_events_count(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal,
			 const EvParams &p, void *state, uint64_t ev_cap, uint64_t *ev_first, uint32_t *ev_count, hipStream_t s)
{
	ktime_begin(1, s);
	hipLaunchKernelGGL((k_events<false>), dim3(nreads), dim3(64), 0, s, sig, off, n, cal, p.w1, p.w2, p.thr1, p.thr2, p.height,
			   (EvState *) state, (EvRec *) nullptr, ev_cap, (const uint64_t *) nullptr);
	ktime_end(1, s);
	ktime_begin(1, s);
	launch_records_scan(state, sizeof(EvState), nreads, ev_cap, ev_first, ev_count, s);
	ktime_end(1, s);
}

// The writing walk behind launch_events_count on the same stream: the records of the reads with ev_first[r + 1] <= ev_cap
void launch_events_write(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal,
			 const EvParams &p, void *state, void *ev, uint64_t ev_cap, const uint64_t *ev_first, hipStream_t s)
{
	ktime_begin(1, s);
	hipLaunchKernelGGL((k_events<true>), dim3(nreads), dim3(64), 0, s, sig, off, n, cal, p.w1, p.w2, p.thr1, p.thr2, p.height,
			   (EvState *) state, (EvRec *) ev, ev_cap, ev_first);
	ktime_end(1, s);
}

// g_ev_serial once the stream is idle; 0 where it cannot be read
uint32_t events_serial_reads(hipStream_t s)
{
	uint32_t v = 0;
	if (hipStreamSynchronize(s) != hipSuccess || hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_ev_serial), sizeof v) != hipSuccess)
		return 0;
	return v;
}

} // namespace ph
