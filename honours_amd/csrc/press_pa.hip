// press_pa.hip - picoamperes of decoded samples, for the methods whose decoder has no float writer of its own.
//
// press_hip_depress_pa_batch for a method whose decoder is not fused: the decoder has left int16 samples in library
// scratch at the caller's off[]; every read is cut into tiles of CHUNK samples, one workgroup per tile.

#include "press_chunk.h"

namespace ph {

// One thread per read: the read's tiles (its ROOM's: out_n is not known on the host, and a tile beyond the decoded
// count ends at once) get contiguous ids, taken by one atomic per wave as in k_chunk_prep; tiles[id] = { read, j }.
__global__ __launch_bounds__(256) void k_pa_tiles(const uint32_t *nsamp, uint32_t nreads, uint2 *tiles, uint32_t *ntiles,
						   uint32_t max_tiles)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	const uint32_t nt = r < nreads ? (uint32_t) (((uint64_t) nsamp[r] + CHUNK - 1) / CHUNK) : 0u;
	const uint32_t inc = scan32(nt, threadIdx.x & 63);
	uint32_t base = 0;
	if ((threadIdx.x & 63) == 63 && inc)
		base = atomicAdd(ntiles, inc);
	base = (uint32_t) __builtin_amdgcn_readlane((int) base, 63);
	const uint32_t first = base + inc - nt;
	for (uint32_t j = 0; j < nt && first + j < max_tiles; j++) // (max_tiles bounds the sum)
		tiles[first + j] = make_uint2(r, j);
}

// One workgroup per tile: [0, out_n[r]) of the read, 8 samples per lane and step - a 16-byte load, two 16-byte stores;
// the read's last, partial group float by float.  The decoder has written out_n[r] samples of the scratch and no more:
// what lies behind them in the group is whatever an earlier call left there, and no float is made of it.  A refused
// read gets nothing.
__global__ __launch_bounds__(256) void k_pa_convert(const int16_t *sig, const uint64_t *off, const uint32_t *out_n,
						     const float *cal, float *pa, const uint2 *tiles, const uint32_t *ntiles)
{
	if (blockIdx.x >= uni(*ntiles))
		return; // (the grid is an upper bound)
	const uint32_t r = uni(tiles[blockIdx.x].x), j = uni(tiles[blockIdx.x].y);
	const uint32_t on = uni(out_n[r]);
	if (on == CFAIL32)
		return;
	const uint64_t cnt = ((uint64_t) on + 7) & ~7ull;
	const uint64_t first = (uint64_t) j * CHUNK;
	const uint64_t end = first + CHUNK < cnt ? first + CHUNK : cnt;
	const uint64_t o = uni64(off[r]);
	const float c0 = __uint_as_float(uni(__float_as_uint(cal[2 * (size_t) r])));
	const float c1 = __uint_as_float(uni(__float_as_uint(cal[2 * (size_t) r + 1])));
	for (uint64_t i = first + threadIdx.x * 8; i < end; i += 256 * 8) {
		const uint4 q = ld16_stream(sig + o + i);
		const uint32_t v[4] = { q.x, q.y, q.z, q.w };
		if (i + 8 <= on) {
			st_pa8(pa + o + i, v, c0, c1);
		} else {
#pragma unroll
			for (uint32_t k = 0; k < 8; k++)
				if (i + k < on)
					pa[o + i + k] = pa_of(v, k, c0, c1);
		}
	}
}

// the two halves of launch_pa_convert, for a caller that reads the tile table between them (press_stats.hip)
void launch_pa_tiles(const DecodeArgs &a, uint2 *tiles, uint32_t *ntiles, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	(void) hipMemsetAsync(ntiles, 0, sizeof(uint32_t), s);
	hipLaunchKernelGGL(k_pa_tiles, dim3((a.nreads + 255) / 256), dim3(256), 0, s, a.nsamp, a.nreads, tiles, ntiles, a.max_chunks);
}

void launch_pa_apply(const DecodeArgs &a, float *pa, const float *cal, const uint2 *tiles, const uint32_t *ntiles, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	hipLaunchKernelGGL(k_pa_convert, dim3(a.max_chunks), dim3(256), 0, s, (const int16_t *) a.sig, a.off, (const uint32_t *) a.out_n,
			   cal, pa, tiles, ntiles);
}

void launch_pa_convert(const DecodeArgs &a, float *pa, const float *cal, uint2 *tiles, uint32_t *ntiles, hipStream_t s)
{
	launch_pa_tiles(a, tiles, ntiles, s);
	launch_pa_apply(a, pa, cal, tiles, ntiles, s);
}

} // namespace ph
