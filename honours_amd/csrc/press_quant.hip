// press_quant.hip - per-read quantiles of decoded samples: up to QMAX order statistics of a read in one radix select.
//
// q[nq * r + i] = the k_i-th smallest (0-based) sample of read r, k_i = min(c - 1, floor(c * num_i / den_i)) - press_stats.hip's
// stat_rank.  The select keeps that file's two digits (8 high bits, 8 low bits of s + 32768) and takes four launches
// whatever nq is:
//
//   k_q_count<1, high>    as k_stat_count: the high digit of every key, one row per read - shared by all ranks
//   k_q_pick (stage 0)    one wave per read scans the row once and finds, for every rank, the digit that holds it and the
//                         rank that is left within that digit
//   k_q_count<NQ, low>    the low digit of every key whose high digit is rank i's, into row i of the read's nq rows; two
//                         ranks may share a high digit, so a sample may be counted in several rows
//   k_q_pick (stage 1)    row i gives rank i's key; q[] is written, and with a rule the two floats k_pa_convert's
//                         arithmetic scales the read with
//
// Scratch: nq rows of 256 counters per read, zeroed by one memset per call (stage 0 clears row 0 again, for the low
// pass), and 36 bytes of state.  Every sum is one of integers; no workgroup waits for another.

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

constexpr uint32_t Q_NB = 256;            // counters of a row: one digit of 8 bits
constexpr uint32_t Q_STRIDE = Q_NB + 1;   // (copies of one counter in different banks)
constexpr uint32_t Q_ROWCOPIES = 16;      // LDS: rows x copies, 16 x 257 words - what k_stat_count's 16 copies of one row take
constexpr uint32_t Q_FAIL = 0xFFFFFFFFu;  // out_n of a refused read
constexpr uint32_t Q_NONE = 0xFFFFFFFFu;  // no digit: a sample that is not counted

struct QRead { // per read, between the launches
	uint32_t c;        // samples (0: empty or refused)
	uint32_t k[QMAX];  // the rank that is left
	uint32_t hi[QMAX]; // the high digit chosen
};

// One workgroup per tile of CHUNK samples (k_pa_tiles' table), 8 samples per lane and step, as k_stat_count: a lane merges
// runs of one digit and adds a run with one ds_add per row; lanes pick a copy of the counters by their id.  LOW: NQ rows
// (1, 2 or 4; nq = 3 runs as 4 with a row nobody matches) and 16 / NQ copies of each; a run is one of equal low digit
// AND equal set of matching ranks.
// RANGED (press_hip_signal_quantiles_ranged, the trimmed chunk call): the samples [a', b') of the read alone, as
// k_stat_count's - the room's tiles and groups, the two edge groups masked per sample (the range: a trailing
// parameter pack, empty or one `const uint32_t *`, as there).
template <int NQ, bool LOW, class... R>
__global__ __launch_bounds__(256) void k_q_count(const int16_t *sig, const uint64_t *off, const uint32_t *out_n, const uint2 *tiles,
						  const uint32_t *ntiles, const QRead *st, uint32_t *rows, uint32_t nq, R... range)
{
	constexpr bool RANGED = sizeof...(R) != 0;
	constexpr uint32_t COPIES = Q_ROWCOPIES / NQ;
	__shared__ uint32_t s_h[Q_ROWCOPIES * Q_STRIDE];
	if (blockIdx.x >= uni(*ntiles))
		return; // (the grid is an upper bound)
	const uint32_t r = uni(tiles[blockIdx.x].x), j = uni(tiles[blockIdx.x].y);
	const uint32_t on = uni(out_n[r]);
	const uint64_t first = (uint64_t) j * CHUNK;
	if (on == Q_FAIL || first >= on)
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
	for (uint32_t i = threadIdx.x; i < Q_ROWCOPIES * Q_STRIDE; i += 256)
		s_h[i] = 0;
	__syncthreads();
	uint32_t hi[NQ];
#pragma unroll
	for (int i = 0; i < NQ; i++)
		hi[i] = LOW && (uint32_t) i < nq ? uni(st[r].hi[i]) : Q_NONE; // (no key has the high digit Q_NONE)
	uint32_t *my = s_h + (threadIdx.x & (COPIES - 1)) * NQ * Q_STRIDE;
	const int16_t *in = sig + uni64(off[r]);
	auto flush = [&](uint32_t tok, uint32_t cnt) {
		if (!LOW) {
			atomicAdd(&my[tok], cnt);
			return;
		}
#pragma unroll
		for (int i = 0; i < NQ; i++)
			if (tok >> (8 + i) & 1u)
				atomicAdd(&my[i * Q_STRIDE + (tok & 255u)], cnt);
	};
	for (uint64_t i = first + threadIdx.x * 8; i < end; i += 256 * 8) {
		if (RANGED && i + 8 <= lo)
			continue;
		const uint4 q = ld16_stream(in + i);
		const uint32_t v[4] = { q.x, q.y, q.z, q.w };
		const uint32_t nv = end - i < 8 ? (uint32_t) (end - i) : 8u;
		const uint32_t skip = RANGED && lo > i ? (uint32_t) (lo - i) : 0u; // (the group that holds a')
		uint32_t cur = Q_NONE, cnt = 0;
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const int32_t s = (e & 1) ? (int32_t) v[e >> 1] >> 16 : (int32_t) (int16_t) (v[e >> 1] & 0xFFFFu);
			const uint32_t key = (uint32_t) (s + 32768);
			uint32_t d;
			if (LOW) { // the ranks this sample counts for, above its low digit
				uint32_t m = 0;
#pragma unroll
				for (int i = 0; i < NQ; i++)
					m |= (key >> 8) == hi[i] ? 1u << (8 + i) : 0u;
				d = m ? m | (key & 255u) : Q_NONE;
			} else {
				d = key >> 8;
			}
			if ((uint32_t) e >= nv || (RANGED && (uint32_t) e < skip))
				d = Q_NONE;
			if (d != cur) {
				if (cur != Q_NONE)
					flush(cur, cnt);
				cur = d;
				cnt = 0;
			}
			cnt++;
		}
		if (cur != Q_NONE)
			flush(cur, cnt);
	}
	__syncthreads();
	uint32_t *row = rows + (size_t) r * nq * Q_NB;
	for (uint32_t x = threadIdx.x; x < NQ * Q_NB; x += 256) {
		const uint32_t i = x / Q_NB, b = x % Q_NB;
		if (i >= (LOW ? nq : 1u))
			break;
		uint32_t sum = 0;
#pragma unroll
		for (uint32_t c = 0; c < COPIES; c++)
			sum += s_h[(c * NQ + i) * Q_STRIDE + b];
		if (sum)
			atomicAdd(row + i * Q_NB + b, sum);
	}
}

__device__ __forceinline__ uint32_t q_rank(uint32_t c, uint32_t num, uint32_t den)
{
	const uint64_t k = (uint64_t) c * num / den;
	return c == 0 ? 0u : k < c ? (uint32_t) k : c - 1;
}

// the digit of a row of 256 counters that holds rank k (the wave's 64 lanes, four steps), and the rank left within it
__device__ __forceinline__ void q_scan_row(const uint32_t (&v)[4], uint32_t lane, uint32_t k, uint32_t &digit, uint32_t &left)
{
	uint32_t before = 0;
	bool found = false;
	digit = 0;
	left = k;
#pragma unroll
	for (int s = 0; s < 4; s++) {
		uint32_t inc = v[s]; // inclusive wave scan (at most c in all: no overflow)
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t u = __shfl_up(inc, d, 64);
			if (lane >= (uint32_t) d)
				inc += u;
		}
		const unsigned long long m = __ballot(before + inc > k);
		if (m && !found) {
			const int l = __ffsll(m) - 1;
			digit = s * 64 + l;
			left = k - (before + (uint32_t) __shfl(inc - v[s], l, 64));
			found = true;
		}
		before += (uint32_t) __shfl(inc, 63, 64);
	}
}

struct QRanks {
	uint32_t num[QMAX], den[QMAX];
};

// One wave per read.  Stage 0 reads (and clears) row 0 and leaves every rank's high digit; stage 1 reads all nq rows and
// writes q[nq * r + i] (the memset in front of the next call clears them).  cal (stage 1, nq = 2): press_hip_scale_cal's
// two floats of {q[0], q[1]}, every operation rounded once and none fused.
// RANGED: the read's count is L = b' - a' of its clamped range.
template <bool RANGED>
__device__ __forceinline__ void q_pick(int stage, const uint32_t *out_n, const uint32_t *range, uint32_t nreads, QRead *st, uint32_t *rows,
				       uint32_t nq, const QRanks &rk, int32_t *q, float *cal, const ScaleRule &rule)
{
	const uint32_t r = uni(blockIdx.x * 4 + (threadIdx.x >> 6));
	if (r >= nreads)
		return;
	const uint32_t lane = threadIdx.x & 63;
	uint32_t *row = rows + (size_t) r * nq * Q_NB;
	QRead t;
	if (stage == 0) {
		const uint32_t on = uni(out_n[r]);
		t.c = on == Q_FAIL ? 0u : on;
		if (RANGED) {
			const uint2 ab = range_clamp(range, r, t.c);
			t.c = uni(ab.y - ab.x);
		}
	} else {
		t.c = uni(st[r].c);
	}
	int32_t res[QMAX] = {};
#pragma unroll
	for (uint32_t i = 0; i < QMAX; i++) {
		t.k[i] = t.hi[i] = 0;
		if (i >= nq)
			continue;
		t.k[i] = stage == 0 ? q_rank(t.c, rk.num[i], rk.den[i]) : uni(st[r].k[i]);
		t.hi[i] = stage == 0 ? 0u : uni(st[r].hi[i]);
		if (!t.c)
			continue; // (nothing was counted: the rows are clean)
		const uint32_t *src = row + (stage == 0 ? 0u : i * Q_NB);
		uint32_t v[4];
#pragma unroll
		for (int s = 0; s < 4; s++)
			v[s] = src[s * 64 + lane];
		uint32_t digit, left;
		q_scan_row(v, lane, t.k[i], digit, left);
		if (stage == 0) {
			t.hi[i] = digit;
			t.k[i] = left;
		} else {
			res[i] = (int32_t) ((t.hi[i] << 8) | digit) - 32768;
		}
	}
	if (stage == 0 && t.c) { // every lane's loads are done (the scans' shuffles have used them): the low pass adds into row 0
		for (uint32_t x = lane; x < Q_NB; x += 64)
			row[x] = 0;
	}
	if (lane != 0)
		return;
	if (stage == 0) {
		st[r] = t;
		return;
	}
	if (q) {
#pragma unroll
		for (uint32_t i = 0; i < QMAX; i++)
			if (i < nq)
				q[(size_t) nq * r + i] = res[i];
	}
	if (cal) {
		const float shift = fmaxf(rule.shift_min, __fmul_rn(rule.shift_mul, (float) (res[0] + res[1])));
		const float scale = fmaxf(rule.scale_min, __fmul_rn(rule.scale_mul, (float) (res[1] - res[0])));
		cal[2 * (size_t) r] = -shift;
		cal[2 * (size_t) r + 1] = __fdiv_rn(1.0f, scale);
	}
}

__global__ __launch_bounds__(256) void k_q_pick(int stage, const uint32_t *out_n, uint32_t nreads, QRead *st, uint32_t *rows, uint32_t nq,
						 QRanks rk, int32_t *q, float *cal, ScaleRule rule)
{
	q_pick<false>(stage, out_n, nullptr, nreads, st, rows, nq, rk, q, cal, rule);
}

__global__ __launch_bounds__(256) void k_q_pick_ranged(int stage, const uint32_t *out_n, const uint32_t *range, uint32_t nreads, QRead *st,
							uint32_t *rows, uint32_t nq, QRanks rk, int32_t *q, float *cal, ScaleRule rule)
{
	q_pick<true>(stage, out_n, range, nreads, st, rows, nq, rk, q, cal, rule);
}

uint64_t quant_rows_bytes(uint32_t nreads, uint32_t nq) { return (uint64_t) nreads * nq * Q_NB * sizeof(uint32_t); }
uint64_t quant_state_bytes(uint32_t nreads) { return (uint64_t) nreads * sizeof(QRead); }

// nq quantiles of a.out_n[r] samples at a.sig + a.off[r] (tiles / ntiles: launch_pa_tiles' table of the same batch; state,
// rows: quant_state_bytes, quant_rows_bytes).  q may be NULL; cal: NULL, or (nq == 2) the floats of `rule`.
void launch_signal_quantiles(const DecodeArgs &a, const uint2 *tiles, const uint32_t *ntiles, void *state, uint32_t *rows,
			     const uint32_t *num, const uint32_t *den, uint32_t nq, int32_t *q, float *cal, const ScaleRule *rule,
			     hipStream_t s)
{
	if (!a.nreads || !a.max_chunks || !nq || nq > QMAX)
		return;
	QRanks rk = {};
	for (uint32_t i = 0; i < nq; i++) {
		rk.num[i] = num[i];
		rk.den[i] = den[i];
	}
	const ScaleRule ru = rule ? *rule : ScaleRule{};
	QRead *st = (QRead *) state;
	const dim3 gc(a.max_chunks), gp((a.nreads + 3) / 4), b(256);
	const int16_t *sig = a.sig;
	const uint32_t *on = a.out_n;
	(void) hipMemsetAsync(rows, 0, quant_rows_bytes(a.nreads, nq), s);
	hipLaunchKernelGGL((k_q_count<1, false>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const QRead *) st, rows, nq);
	hipLaunchKernelGGL(k_q_pick, gp, b, 0, s, 0, on, a.nreads, st, rows, nq, rk, (int32_t *) nullptr, (float *) nullptr, ru);
	if (nq == 1)
		hipLaunchKernelGGL((k_q_count<1, true>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const QRead *) st, rows, nq);
	else if (nq == 2)
		hipLaunchKernelGGL((k_q_count<2, true>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const QRead *) st, rows, nq);
	else
		hipLaunchKernelGGL((k_q_count<4, true>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const QRead *) st, rows, nq);
	hipLaunchKernelGGL(k_q_pick, gp, b, 0, s, 1, on, a.nreads, st, rows, nq, rk, q, nq == 2 ? cal : nullptr, ru);
}

// ... of the samples [a', b') of every read alone (range: 2 words per read, device memory, clamped by the kernels)
void launch_signal_quantiles_ranged(const DecodeArgs &a, const uint32_t *range, const uint2 *tiles, const uint32_t *ntiles, void *state,
				    uint32_t *rows, const uint32_t *num, const uint32_t *den, uint32_t nq, int32_t *q, float *cal,
				    const ScaleRule *rule, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks || !nq || nq > QMAX)
		return;
	QRanks rk = {};
	for (uint32_t i = 0; i < nq; i++) {
		rk.num[i] = num[i];
		rk.den[i] = den[i];
	}
	const ScaleRule ru = rule ? *rule : ScaleRule{};
	QRead *st = (QRead *) state;
	const dim3 gc(a.max_chunks), gp((a.nreads + 3) / 4), b(256);
	const int16_t *sig = a.sig;
	const uint32_t *on = a.out_n;
	(void) hipMemsetAsync(rows, 0, quant_rows_bytes(a.nreads, nq), s);
	hipLaunchKernelGGL((k_q_count<1, false, const uint32_t *>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const QRead *) st, rows, nq, range);
	hipLaunchKernelGGL(k_q_pick_ranged, gp, b, 0, s, 0, on, range, a.nreads, st, rows, nq, rk, (int32_t *) nullptr, (float *) nullptr, ru);
	if (nq == 1)
		hipLaunchKernelGGL((k_q_count<1, true, const uint32_t *>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const QRead *) st, rows, nq, range);
	else if (nq == 2)
		hipLaunchKernelGGL((k_q_count<2, true, const uint32_t *>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const QRead *) st, rows, nq, range);
	else
		hipLaunchKernelGGL((k_q_count<4, true, const uint32_t *>), gc, b, 0, s, sig, a.off, on, tiles, ntiles, (const QRead *) st, rows, nq, range);
	hipLaunchKernelGGL(k_q_pick_ranged, gp, b, 0, s, 1, on, range, a.nreads, st, rows, nq, rk, q, nq == 2 ? cal : nullptr, ru);
}

} // namespace ph
