// press_degrade.hip - lossy archives: D_b, the rounding of every sample to the nearest multiple of 2^b (include/press_hip.h,
// press_hip_degrade_value), over samples that lie in device memory: the caller's (press_hip_degrade_batch) or the ones a
// recode has just decoded (press_hip_recode_degraded_*, the route that is not fused).
//
// The kernel runs over k_pa_tiles' table as k_pa_convert and k_verify_cmp do: a read's room is cut into tiles of CHUNK
// samples, one workgroup per tile, and a tile at or beyond the read's count ends at once; no workgroup waits for another.
// 8 samples per lane and step: one 16-byte load, four packed 16-bit saturating adds and four ANDs (degrade_pair), one
// 16-byte store.  A lane stores what it has loaded itself, so out == sig needs no care.  The read's last group of fewer
// than 8 samples is stored sample by sample and never past the count; its load stays inside
// [off[r], off[r] + roundup8(count)), as the press kernels' do.

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

namespace {

constexpr uint32_t DG_FAIL = 0xFFFFFFFFu; // out_n of a refused read

__device__ __forceinline__ void st16_plain(void *p, const uint4 v)
{
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	u32x4 w;
	w.x = v.x, w.y = v.y, w.z = v.z, w.w = v.w;
	__builtin_nontemporal_store(w, reinterpret_cast<u32x4 *>(p));
}

__global__ __launch_bounds__(256) void k_degrade(const int16_t *sig, int16_t *out, const uint64_t *off, const uint32_t *out_n,
						  const uint2 *tiles, const uint32_t *ntiles, uint32_t h2, uint32_t m2)
{
	if (blockIdx.x >= uni(*ntiles))
		return; // (the grid is an upper bound)
	const uint32_t r = uni(tiles[blockIdx.x].x), j = uni(tiles[blockIdx.x].y);
	const uint32_t on = uni(out_n[r]);
	if (on == DG_FAIL)
		return;
	const uint64_t first = (uint64_t) j * CHUNK;
	if (first >= on)
		return;
	const uint64_t end = first + CHUNK < on ? first + CHUNK : on;
	const uint64_t o = uni64(off[r]);
	for (uint64_t i = first + threadIdx.x * 8; i < end; i += 256 * 8) {
		const uint4 q = ld16_stream(sig + o + i);
		const uint32_t v[4] = { degrade_pair(q.x, h2, m2), degrade_pair(q.y, h2, m2), degrade_pair(q.z, h2, m2),
					degrade_pair(q.w, h2, m2) };
		if (i + 8 <= end) {
			st16_plain(out + o + i, make_uint4(v[0], v[1], v[2], v[3]));
		} else {
#pragma unroll
			for (uint32_t k = 0; k < 8; k++)
				if (i + k < end)
					out[o + i + k] = (int16_t) (v[k >> 1] >> (16 * (k & 1)));
		}
	}
}

} // namespace

// out[a.off[r] + i] = D_bits(a.sig[a.off[r] + i]) for i < a.out_n[r] (a refused read: nothing), bits in 0 .. 8 (0: a copy),
// over the tile table of a.nsamp (launch_pa_tiles)
void launch_degrade(const DecodeArgs &a, int16_t *out, uint32_t bits, const uint2 *tiles, const uint32_t *ntiles, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	hipLaunchKernelGGL(k_degrade, dim3(a.max_chunks), dim3(256), 0, s, (const int16_t *) a.sig, out, a.off, (const uint32_t *) a.out_n,
			   tiles, ntiles, degrade_h2(bits), degrade_m2(bits));
}

} // namespace ph

// The definition, as host arithmetic in 32-bit integers (an arithmetic shift of a negative value, as every compiler this
// library builds with gives it)
extern "C" int16_t press_hip_degrade_value(int16_t s, uint32_t bits)
{
	if (bits == 0 || bits > 8)
		return s;
	const int32_t b = (int32_t) bits;
	const int32_t r = (((int32_t) s + (1 << (b - 1))) >> b) * (1 << b);
	const int32_t top = 32768 - (1 << b);
	return (int16_t) (r < top ? r : top);
}
