// press_tally.hip - dataset analysis on the device (include/press_hip.h, "Dataset analysis"): what the
// reference's viz/ programs and press/stats.c compute on the host, in one pass over a batch laid out as for
// press_hip_symbol_counts.  With zz(v) = (uint16_t) ((v << 1) ^ (v >> 15)), d[i] = (int16_t) (s[i] - s[i-1]) and
// sym[i] = min(zz(d[i]), 256):
//
//   raw    65536 counters   raw[zz(s[i])]++                       i in [0, c)   viz/freq_slow5.c, tally.h updatetally
//   delta  65536 counters   delta[zz(d[i])]++                     i in [1, c)   viz/freq_delta_slow5.c
//   trans  257 x 257        trans[257 * sym[i-1] + sym[i]]++      i in [2, c)   the order-1 statistic of the coded symbols
//   mom    one per read     sum, sum of squares, min, max, n and the number of d[i] outside [-128, 127]
//                                                                                press/stats.c, viz/get_exceptions.c
//
//   k_tally_prep    the work list (one entry per chunk of CHUNK samples) and the initial moments
//   k_tally<WHAT>   a persistent grid over the chunks, one instance per set of outputs
//
// THE WINDOWS.  No table fits LDS whole (65536 u32 = 256 KiB, 257^2 u32 = 264 KiB; a CU has 160 KiB), so each keeps the
// counters that nanopore data hits in LDS and sends every other increment to the table itself with a 64-bit atomic that
// returns nothing:
//   raw    zz < 8192   samples in [-4096, 4095] (the reference's own TALLY_SZ_EXP)       32 KiB
//   delta  zz < 1024   deltas in [-512, 511], 4 copies                                   16 KiB
//   trans  both symbols below 160 (deltas in [-80, 79]) or the exception class: 161^2   101 KiB
// The window only decides WHERE an increment is counted: the sums are exact for any int16 content.  A workgroup adds its
// LDS counters that are not zero to the tables when it has run out of chunks, one 64-bit atomic each.  149 KiB for all
// four outputs: one workgroup of 16 waves per CU, which walks four chunks at a time; an instance pays only for its own
// tables, and the host asks the runtime how many workgroups of the instance a CU holds (tally_launch).
//
// CONTENTION.  A lane's 8 samples are neighbours in time, so a lane merges runs of one counter (a stall or a constant
// stretch: all 8) and adds a run with ONE ds_add; the lanes of a wave spread over the 4 copies of the delta window by
// lane & 3.  A constant read then costs one ds_add per lane, table and 16-byte load instead of eight.
//
// COUNTER WIDTH.  The LDS counters are 32 bits and are flushed once, at the end.  A counter receives at most one
// increment per sample its workgroup walks, a workgroup walks at most max_chunks / grid + 4 chunks of 2^15 samples, and
// the host chooses the grid so that max_chunks / grid is at most TALLY_WG_CHUNKS = 2^16 (tally_grid): below 2^32 per counter.
//
// All sums are sums of integers: the results do not depend on the order in which workgroups finish.

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

enum { Y_RAW = 1, Y_DELTA = 2, Y_TRANS = 4, Y_MOM = 8 };
// threads per workgroup of an instance: a chunk in flight per 256, four waves each.  With the transition table a CU
// holds one workgroup, so that one is as large as a workgroup gets (16 waves; measured against 8: all four outputs
// 1.70 against 2.52 ms, trans alone 0.84 against 1.19); the instances without it are faster as several of 8 waves
// (raw alone 0.41 against 0.46 ms)
constexpr int tally_wg(int what) { return (what & Y_TRANS) ? 1024 : 512; }
constexpr int YCK = 16;                   // 16-byte loads per lane and chunk (4 waves x 16 x 512 samples = CHUNK)
constexpr uint32_t YSUB = 512;            // samples per wave and load (64 lanes x 8)
constexpr uint32_t YWAVE = YCK * YSUB;    // samples per wave and chunk
static_assert(YWAVE * 4 == CHUNK, "chunk = 4 waves");
constexpr uint32_t RAW_WIN = 8192;        // raw counters in LDS
constexpr uint32_t DEL_WIN = 1024;        // delta counters in LDS ...
constexpr uint32_t DEL_COPIES = 4;        // ... this many times, by lane & 3
constexpr uint32_t DEL_STRIDE = DEL_WIN;
constexpr uint32_t TR_CORE = 160;         // symbols of the transition table's core in LDS ...
constexpr uint32_t TR_SIDE = TR_CORE + 1;  // ... and the exception class (symbol 256) as one more row and column
constexpr uint32_t YNONE = 0xFFFFFFFFu;   // no counter: an element that is not counted
constexpr uint32_t TALLY_WG_CHUNKS = 1u << 16;

struct Moments { // press_hip_moments
	long long sum;
	unsigned long long sumsq;
	int32_t min, max;
	uint32_t n, nex;
};
static_assert(sizeof(Moments) == 32, "press_hip_moments");

// The work list, built on the device (off / n may be device-resident): one thread per read, a wave takes a contiguous
// range of chunk ids with ONE atomic.  A read of one sample has a chunk (raw and mom count it); an empty read has none.
// mom (may be NULL): every read's record before the walk adds to it.
__global__ __launch_bounds__(256) void k_tally_prep(const uint32_t *nsamp, uint32_t nreads, uint2 *chunks, uint32_t *nchunks,
						    uint32_t max_chunks, Moments *mom)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	uint32_t n = 0, nch = 0;
	if (r < nreads) {
		n = nsamp[r];
		nch = n / CHUNK + (n % CHUNK != 0);
	}
	uint32_t inc = nch; // inclusive wave scan
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = __shfl_up(inc, d, 64);
		if (lane >= d)
			inc += t;
	}
	uint32_t base = 0;
	if (lane == 63 && inc)
		base = atomicAdd(nchunks, inc);
	base = (uint32_t) __builtin_amdgcn_readlane((int) base, 63);
	if (r >= nreads)
		return;
	if (mom) {
		Moments m = { 0, 0, 32767, -32768, n, 0 }; // press/stats.c init_stats
		mom[r] = m;
	}
	const uint32_t first = base + inc - nch;
	for (uint32_t j = 0; j < nch && first + j < max_chunks; j++)
		chunks[first + j] = make_uint2(r, j);
}

// runs of one counter among a lane's 8 elements: add(key, run length) once per run; YNONE elements are not counted
template <class Add> __device__ __forceinline__ void tally_runs(const uint32_t key[8], Add add)
{
	uint32_t cur = YNONE, cnt = 0;
#pragma unroll
	for (int e = 0; e < 8; e++) {
		if (key[e] != cur) {
			if (cur != YNONE)
				add(cur, cnt);
			cur = key[e];
			cnt = 0;
		}
		cnt++;
	}
	if (cur != YNONE)
		add(cur, cnt);
}

__device__ __forceinline__ uint32_t zz_pair(uint32_t v)
{
	const s16x2 s = __builtin_bit_cast(s16x2, v);
	return __builtin_bit_cast(uint32_t, (s16x2) ((s << 1) ^ (s >> 15)));
}

// A chunk is 4 waves x 16 loads of 16 bytes per lane (the layout of k_symbol_count); the two samples in front of a wave's
// quarter are one plain load.  No barrier inside the loop: a wave may leave a chunk on its own.
template <int WHAT>
__global__ __launch_bounds__(tally_wg(WHAT)) void k_tally(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, const uint2 *chunks,
					       const uint32_t *nchunks, uint32_t max_chunks, unsigned long long *raw,
					       unsigned long long *delta, unsigned long long *trans, Moments *mom)
{
	constexpr bool RAW = WHAT & Y_RAW, DEL = WHAT & Y_DELTA, TRA = WHAT & Y_TRANS, MOM = WHAT & Y_MOM;
	constexpr uint32_t YWG = tally_wg(WHAT), YPAR = YWG / 256;
	__shared__ uint32_t s_raw[RAW ? RAW_WIN : 1];
	__shared__ uint32_t s_del[DEL ? DEL_COPIES * DEL_STRIDE : 1];
	__shared__ uint32_t s_tr[TRA ? TR_SIDE * TR_SIDE : 1];
	if (RAW)
		for (uint32_t i = threadIdx.x; i < RAW_WIN; i += YWG)
			s_raw[i] = 0;
	if (DEL)
		for (uint32_t i = threadIdx.x; i < DEL_COPIES * DEL_STRIDE; i += YWG)
			s_del[i] = 0;
	if (TRA)
		for (uint32_t i = threadIdx.x; i < TR_SIDE * TR_SIDE; i += YWG)
			s_tr[i] = 0;
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t w = uni((threadIdx.x >> 6) & 3);   // the wave's quarter of its chunk
	const uint32_t half = uni(threadIdx.x >> 8);      // which of the workgroup's chunks in flight
	const uint32_t nch = min(uni(*nchunks), max_chunks);
	uint32_t *my_del = s_del + (DEL ? (lane & (DEL_COPIES - 1)) * DEL_STRIDE : 0);

	auto add_raw = [&](uint32_t key, uint32_t cnt) {
		if (key < RAW_WIN)
			atomicAdd(&s_raw[key], cnt);
		else
			atomicAdd(raw + key, (unsigned long long) cnt);
	};
	auto add_del = [&](uint32_t key, uint32_t cnt) {
		if (key < DEL_WIN)
			atomicAdd(&my_del[key], cnt);
		else
			atomicAdd(delta + key, (unsigned long long) cnt);
	};
	auto add_tr = [&](uint32_t key, uint32_t cnt) { // key = from << 16 | to, both at most 256
		const uint32_t a = key >> 16, b = key & 0xFFFFu;
		const uint32_t ia = a == 256u ? TR_CORE : a, ib = b == 256u ? TR_CORE : b;
		if ((a < TR_CORE || a == 256u) && (b < TR_CORE || b == 256u))
			atomicAdd(&s_tr[ia * TR_SIDE + ib], cnt);
		else
			atomicAdd(trans + 257u * a + b, (unsigned long long) cnt);
	};

	for (uint64_t t = (uint64_t) YPAR * blockIdx.x + half; t < nch; t += (uint64_t) YPAR * gridDim.x) {
		const uint32_t r = uni(chunks[t].x);
		const uint32_t n = uni(nsamp[r]);
		const uint32_t ws = uni(chunks[t].y) * CHUNK + w * YWAVE; // first sample of this wave's quarter
		if (ws >= n)
			continue;
		const int16_t *in = sig + uni64(off[r]);
		uint4 z[YCK];
#pragma unroll
		for (int k = 0; k < YCK; k++) {
			const uint32_t i0 = ws + k * YSUB + lane * 8;
			z[k] = make_uint4(0, 0, 0, 0);
			if (i0 < n)
				z[k] = ld16_stream(in + i0);
		}
		// s[ws - 2], s[ws - 1] (ws is a multiple of 8192: both are samples of the read) and the symbol of d[ws - 1]
		uint32_t carry = ws > 0 ? *reinterpret_cast<const uint32_t *>(in + ws - 2) : 0u;
		uint32_t carry_sym = min(zd_pair(carry, 0) >> 16, 256u);
		int32_t m_sum = 0, m_min = 32767, m_max = -32768;
		uint32_t m_nex = 0;
		uint64_t m_sq = 0;
#pragma unroll
		for (int k = 0; k < YCK; k++) {
			const uint32_t i0 = ws + k * YSUB + lane * 8;
			const uint32_t pw = prev_lane(z[k].w, carry);
			carry = (uint32_t) __builtin_amdgcn_readlane((int) z[k].w, 63);
			const uint32_t zd[4] = { zd_pair(z[k].x, pw), zd_pair(z[k].y, z[k].x), zd_pair(z[k].z, z[k].y),
						 zd_pair(z[k].w, z[k].z) };
			const uint32_t zr[4] = { zz_pair(z[k].x), zz_pair(z[k].y), zz_pair(z[k].z), zz_pair(z[k].w) };
			const uint32_t v[4] = { z[k].x, z[k].y, z[k].z, z[k].w };
			// the symbol in front of the lane's first: the previous lane's last, the previous load's last for lane 0
			const uint32_t my_last = min(zd[3] >> 16, 256u);
			uint32_t before = prev_lane(my_last, carry_sym);
			carry_sym = (uint32_t) __builtin_amdgcn_readlane((int) my_last, 63);
			if (i0 >= n)
				continue; // (per lane: the loads behind the read's end)
			uint32_t kr[8], kd[8], kt[8];
#pragma unroll
			for (int q = 0; q < 8; q++) {
				const uint32_t i = i0 + q;
				const bool in_read = i < n; // i0 < n and i0 + 7 does not wrap: n - i0 > q
				const uint32_t d = (zd[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
				const uint32_t sym = min(d, 256u);
				kr[q] = in_read ? (zr[q >> 1] >> (16 * (q & 1))) & 0xFFFFu : YNONE;
				kd[q] = in_read && i >= 1 ? d : YNONE;
				kt[q] = in_read && i >= 2 ? (before << 16) | sym : YNONE;
				before = sym;
				if (MOM && in_read) {
					const int32_t s = (q & 1) ? (int32_t) v[q >> 1] >> 16 : (int32_t) (int16_t) (v[q >> 1] & 0xFFFFu);
					m_sum += s; // (at most 128 samples per lane and chunk: 2^22)
					m_sq += (uint32_t) (s * s);
					m_min = min(m_min, s);
					m_max = max(m_max, s);
					m_nex += (i >= 1 && d > 255u) ? 1u : 0u;
				}
			}
			if (RAW)
				tally_runs(kr, add_raw);
			if (DEL)
				tally_runs(kd, add_del);
			if (TRA)
				tally_runs(kt, add_tr);
		}
		if (MOM) { // the wave's quarter: at most 8192 samples, |sum| < 2^28
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1) {
				m_sum += __shfl_xor(m_sum, d, 64);
				m_sq += __shfl_xor(m_sq, d, 64);
				m_min = min(m_min, __shfl_xor(m_min, d, 64));
				m_max = max(m_max, __shfl_xor(m_max, d, 64));
				m_nex += __shfl_xor(m_nex, d, 64);
			}
			if (lane == 0) {
				Moments *m = mom + r;
				atomicAdd(reinterpret_cast<unsigned long long *>(&m->sum), (unsigned long long) (long long) m_sum);
				atomicAdd(&m->sumsq, (unsigned long long) m_sq);
				atomicMin(&m->min, m_min);
				atomicMax(&m->max, m_max);
				if (m_nex)
					atomicAdd(&m->nex, m_nex);
			}
		}
	}
	__syncthreads();
	if (RAW)
		for (uint32_t b = threadIdx.x; b < RAW_WIN; b += YWG)
			if (s_raw[b])
				atomicAdd(raw + b, (unsigned long long) s_raw[b]);
	if (DEL)
		for (uint32_t b = threadIdx.x; b < DEL_WIN; b += YWG) {
			uint64_t sum = 0;
#pragma unroll
			for (uint32_t c = 0; c < DEL_COPIES; c++)
				sum += s_del[c * DEL_STRIDE + b];
			if (sum)
				atomicAdd(delta + b, (unsigned long long) sum);
		}
	if (TRA)
		for (uint32_t b = threadIdx.x; b < TR_SIDE * TR_SIDE; b += YWG)
			if (s_tr[b]) {
				const uint32_t ia = b / TR_SIDE, ib = b % TR_SIDE;
				atomicAdd(trans + 257u * (ia == TR_CORE ? 256u : ia) + (ib == TR_CORE ? 256u : ib), (unsigned long long) s_tr[b]);
			}
}

uint64_t tally_scratch_bytes(uint32_t max_chunks) { return (uint64_t) max_chunks * sizeof(uint2); }

// the persistent grid (wg: the workgroups the device holds at once), widened where a workgroup would otherwise walk more
// than TALLY_WG_CHUNKS chunks: the 32-bit LDS counters cannot wrap (COUNTER WIDTH above)
static uint32_t tally_grid(uint32_t max_chunks, uint32_t wg)
{
	const uint32_t need = max_chunks / TALLY_WG_CHUNKS + (max_chunks % TALLY_WG_CHUNKS != 0);
	return wg > need ? wg : need;
}

// a persistent grid: as many workgroups as the device holds of this instance (its LDS decides: one per CU with the
// transition table, more without), at most 4 per CU
template <int WHAT> static void tally_launch(const int16_t *sig, const uint64_t *off, const uint32_t *n, const uint2 *chunks,
					     const uint32_t *nchunks, uint32_t max_chunks, uint64_t *raw, uint64_t *delta,
					     uint64_t *trans, void *mom, uint32_t cus, hipStream_t s)
{
	static int per_cu = 0; // (asked once per instance; the API lock serialises the callers)
	if (per_cu == 0) {
		int nb = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_tally<WHAT>, tally_wg(WHAT), 0) != hipSuccess || nb < 1)
			nb = 1;
		per_cu = nb > 4 ? 4 : nb;
	}
	const uint32_t grid = tally_grid(max_chunks, cus * (uint32_t) per_cu);
	hipLaunchKernelGGL((k_tally<WHAT>), dim3(grid), dim3(tally_wg(WHAT)), 0, s, sig, off, n, chunks, nchunks, max_chunks,
			   (unsigned long long *) raw, (unsigned long long *) delta, (unsigned long long *) trans, (Moments *) mom);
}

// raw, delta, trans, mom: any may be NULL (not all: the caller returns before).  chunks takes tally_scratch_bytes(max_chunks),
// nchunks is one device word (zeroed here); cus: the device's compute units
void launch_signal_tally(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, uint64_t *raw, uint64_t *delta,
			 uint64_t *trans, void *mom, void *chunks, uint32_t *nchunks, uint32_t max_chunks, uint32_t cus, hipStream_t s)
{
	typedef void (*Launch)(const int16_t *, const uint64_t *, const uint32_t *, const uint2 *, const uint32_t *, uint32_t, uint64_t *,
			       uint64_t *, uint64_t *, void *, uint32_t, hipStream_t);
	static const Launch table[16] = { nullptr,          tally_launch<1>,  tally_launch<2>,  tally_launch<3>, tally_launch<4>,  tally_launch<5>,
					  tally_launch<6>,  tally_launch<7>,  tally_launch<8>,  tally_launch<9>, tally_launch<10>, tally_launch<11>,
					  tally_launch<12>, tally_launch<13>, tally_launch<14>, tally_launch<15> };
	const int what = (raw ? Y_RAW : 0) | (delta ? Y_DELTA : 0) | (trans ? Y_TRANS : 0) | (mom ? Y_MOM : 0);
	if (!what)
		return;
	(void) hipMemsetAsync(nchunks, 0, sizeof(uint32_t), s);
	hipLaunchKernelGGL(k_tally_prep, dim3((nreads + 255) / 256), dim3(256), 0, s, n, nreads, (uint2 *) chunks, nchunks, max_chunks,
			   (Moments *) mom);
	table[what](sig, off, n, (const uint2 *) chunks, nchunks, max_chunks, raw, delta, trans, mom, cus, s);
}

} // namespace ph
