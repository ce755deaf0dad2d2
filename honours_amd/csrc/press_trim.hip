// press_trim.hip - the cuts and the row plan of press_hip_depress_chunks_trimmed_batch, on the device: nothing here waits
// for the host, so the rows of a batch can depend on what a detector found in it.
//
//   k_trim_counts   c[r] = min(out_n[r], n[r]), 0 for a refused read: the sample counts the detectors walk
//   k_trim_cut      a', b' of every read from the caller's range (mode RANGE), the adaptor's pair (ADAPTOR) or the first
//                   stall record (SEGMENT), clamped as include/press_hip.h 2y says, min_keep applied; cut[] and the read's
//                   row count press_hip_chunk_plan gives L = b' - a' samples, as a 64-bit word
//   k_pk_scan       (press_packed.hip, launch_pack_scan with no alignment and no cap) the exclusive 64-bit sums of those
//                   counts: row_first[0 .. nreads]

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

constexpr uint32_t TRIM_FAIL = 0xFFFFFFFFu; // out_n of a refused read

__device__ __forceinline__ uint32_t trim_count(const uint32_t *out_n, const uint32_t *nsamp, uint32_t r)
{
	const uint32_t on = out_n[r], c = nsamp[r];
	return on == TRIM_FAIL ? 0u : on < c ? on : c;
}

__global__ __launch_bounds__(256) void k_trim_counts(const uint32_t *out_n, const uint32_t *nsamp, uint32_t nreads, uint32_t *cnt)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r < nreads)
		cnt[r] = trim_count(out_n, nsamp, r);
}

// det: mode ADAPTOR - launch_adaptor's pairs (start, end), int32; mode SEGMENT - launch_segments_first's records
// (start, end), start = STALL_NOSEG: none.  cut and user: 2 words per read (user may be NULL); need: a word of 64 bits
__global__ __launch_bounds__(256) void k_trim_cut(const uint32_t *out_n, const uint32_t *nsamp, uint32_t nreads, int mode,
						   const uint32_t *range, const uint32_t *det, uint32_t min_keep, uint32_t T, uint32_t S,
						   uint32_t *cut, uint32_t *user, uint64_t *need)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= nreads)
		return;
	const uint32_t c = trim_count(out_n, nsamp, r);
	uint2 ab;
	if (mode == PRESS_TRIM_RANGE) {
		ab = range_clamp(range, r, c);
	} else {
		const uint32_t d0 = det[2 * (size_t) r], d1 = det[2 * (size_t) r + 1];
		uint32_t a;
		if (mode == PRESS_TRIM_ADAPTOR)
			a = (int32_t) d1 > 0 ? d1 : 0u;
		else
			a = d0 == STALL_NOSEG ? 0u : d1;
		a = a < c ? a : c;
		if (c - a < min_keep)
			a = 0;
		ab = make_uint2(a, c);
	}
	cut[2 * (size_t) r] = ab.x;
	cut[2 * (size_t) r + 1] = ab.y;
	if (user) {
		user[2 * (size_t) r] = ab.x;
		user[2 * (size_t) r + 1] = ab.y;
	}
	const uint32_t L = ab.y - ab.x; // press_hip_chunk_plan's rows of a read of L samples
	need[r] = L == 0 ? 0ull : L <= T ? 1ull : 1ull + ((uint64_t) (L - T) + S - 1) / S;
}

void launch_trim_counts(const DecodeArgs &a, uint32_t *cnt, hipStream_t s)
{
	if (a.nreads)
		hipLaunchKernelGGL(k_trim_counts, dim3((a.nreads + 255) / 256), dim3(256), 0, s, (const uint32_t *) a.out_n, a.nsamp, a.nreads, cnt);
}

// cut[] (and user[], unless NULL) of a.nreads >= 1 reads, then row_first[0 .. nreads]; need and slot: nreads + 1 words of
// 64 bits each (the scan's tables)
void launch_trim_plan(const DecodeArgs &a, int mode, const uint32_t *range, const void *det, uint32_t min_keep, uint32_t T, uint32_t overlap,
		      uint32_t *cut, uint32_t *user, uint64_t *need, uint64_t *slot, uint64_t *row_first, hipStream_t s)
{
	hipLaunchKernelGGL(k_trim_cut, dim3((a.nreads + 255) / 256), dim3(256), 0, s, (const uint32_t *) a.out_n, a.nsamp, a.nreads, mode, range,
			   (const uint32_t *) det, min_keep, T, T - overlap, cut, user, need);
	// (no alignment, no cap: layout[] is the plain exclusive sum.  The scan also fills slot[], the table of a packed press's
	// writers; nothing here reads it - a by-product of using that kernel as it is, which is why the plan carries pslot)
	const PackArgs pk = { need, row_first, slot, ~0ull - 1, 1u };
	launch_pack_scan(pk, a.nreads, s);
}

} // namespace ph
