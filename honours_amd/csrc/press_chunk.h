// press_chunk.h - the chunk machinery shared by the svb kernels (press_svb.hip), the exception-split kernels
// (press_exsplit.hip) and the picoampere converter (press_pa.hip).
//
// A read is cut into chunks of CHUNK = 32768 samples; one 256-thread workgroup per chunk,
// handed out in ticket order.  Each of the 4 waves owns a contiguous quarter of the chunk
// (8192 samples = 16 sub-tiles of 512 samples; a lane holds 8 samples = one dwordx4 per
// sub-tile), so
//   * all 16 loads of a lane are issued back to back (64 KiB in flight per workgroup) and
//     the zig-zag-delta values stay in registers as packed 16-bit pairs
//     (v_alignbit + v_pk_sub_i16 + v_pk_lshlrev/ashrrev + v_xor per pair);
//   * a sub-tile without exceptions (98 % of them on NA12878-like data) is written with
//     two v_perm_b32 and ONE 8-byte global store per lane at an unaligned address
//     (unaligned dwordx2 stores run at 0.9x the aligned rate on MI355X,
//     tools/ubench_unaligned.hip); a sub-tile with exceptions takes a wave scan and the
//     few lanes that hold an exception store byte-wise.  No LDS staging, no barrier in
//     the data path;
//   * what chains the chunks of a read is only the NUMBER of exceptions before the chunk
//     (the byte offset of sample i is i + #exceptions before i): a decoupled look-back
//     over 8-byte {status,count} granules, each written by one relaxed agent-scope atomic
//     store (cdna_hip_programming.md Guideline 16, form R2: the data is the flag).
//     Ticket order makes the look-back deadlock free: every predecessor of a chunk was
//     taken by a workgroup that is already running.
#pragma once

#include "press_internal.h"
#include "press_packed.h"
#include "press_wave.h"

namespace ph {

constexpr int CWG = 256;                     // threads per workgroup
constexpr int CK = 16;                       // sub-tiles per wave
constexpr uint32_t SUB = 512;                // samples per sub-tile (64 lanes x 8)
constexpr uint32_t WAVE_SAMPLES = CK * SUB;  // 8192
static_assert(WAVE_SAMPLES * 4 == CHUNK, "chunk = 4 waves");

#ifndef PERSISTENT_GRID_N
#define PERSISTENT_GRID_N 1024 // = what is resident (4 workgroups of ~110 VGPRs per CU); 768-1280 measured equal, 2048 2.5 % slower
#endif
constexpr uint32_t PERSISTENT_GRID = PERSISTENT_GRID_N;   // workgroups of the ticket-loop kernel (k_svb_encode_chunked)
constexpr uint64_t G_A = 1ull << 62;         // granule: aggregate of this chunk only
constexpr uint64_t G_P = 2ull << 62;         // granule: inclusive prefix up to this chunk
constexpr uint64_t G_MASK = (1ull << 62) - 1;
constexpr uint64_t CFAIL64 = ~0ull;
constexpr uint32_t CFAIL32 = 0xFFFFFFFFu;

// 8 bytes at any byte address of a stream that is read once
#ifndef PRESS_NO_NT
__device__ __forceinline__ unsigned long long ld8_stream(const void *p)
{
	typedef unsigned long long __attribute__((aligned(1))) u64_u;
	return __builtin_nontemporal_load(reinterpret_cast<const u64_u *>(p));
}
#else
__device__ __forceinline__ unsigned long long ld8_stream(const void *p)
{
	unsigned long long v;
	__builtin_memcpy(&v, p, 8);
	return v;
}
#endif
// ... and 16 bytes of a stream that is written once and not read again by this call
#if !defined(PRESS_NO_NT) && !defined(PRESS_NO_NT_ST)
__device__ __forceinline__ void st16_stream(void *p, uint4 v)
{
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	__builtin_nontemporal_store((u32x4){ v.x, v.y, v.z, v.w }, reinterpret_cast<u32x4 *>(p));
}
#else
__device__ __forceinline__ void st16_stream(void *p, uint4 v) { *reinterpret_cast<uint4 *>(p) = v; }
#endif

// Picoamperes (press_hip_depress_pa_batch): pa = ((float) s + c0) * c1, the reference's signal_in_picoamps (sigtk
// misc.c:28).  The add and the multiply round one after the other: no contraction into a fused multiply-add here,
// whatever the build's default.
__device__ __forceinline__ float to_pa(int32_t smp, float c0, float c1)
{
#pragma clang fp contract(off)
	const float t = (float) smp + c0;
	return t * c1;
}
// the k-th of the 8 samples a lane holds as packed pairs
__device__ __forceinline__ float pa_of(const uint32_t (&v)[4], int k, float c0, float c1)
{
	return to_pa((k & 1) ? (int32_t) v[k >> 1] >> 16 : (int32_t) (int16_t) (v[k >> 1] & 0xFFFFu), c0, c1);
}
// ... all 8 to p (32-byte aligned): two 16-byte stores
__device__ __forceinline__ void st_pa8(float *p, const uint32_t (&v)[4], float c0, float c1)
{
	uint32_t x[8];
#pragma unroll
	for (int k = 0; k < 8; k++)
		x[k] = __float_as_uint(pa_of(v, k, c0, c1));
	st16_stream(p, make_uint4(x[0], x[1], x[2], x[3]));
	st16_stream(p + 4, make_uint4(x[4], x[5], x[6], x[7]));
}

// the same, and which of the two differences do not fit 16 bits (bit 15 / bit 31 of `ov`): slow5lib
// takes the delta in 32 bits (streamvbyte_zigzag.c:15), so such a value is 17 bits wide.
// If d16 is the wrapped difference and z16 its zig-zag, the true zig-zag is (~z16 & 0xFFFF) | 0x10000.
__device__ __forceinline__ uint32_t zd_pair_ovf(uint32_t cur, uint32_t prevdw, uint32_t &ov)
{
	const uint32_t sh = __builtin_amdgcn_alignbit(cur, prevdw, 16); // [prev.hi, cur.lo]
	const s16x2 d = __builtin_bit_cast(s16x2, cur) - __builtin_bit_cast(s16x2, sh);
	const uint32_t du = __builtin_bit_cast(uint32_t, d);
	ov |= (cur ^ sh) & (cur ^ du) & 0x80008000u; // a - b overflows iff sign(a) != sign(b) and sign(a - b) != sign(a)
	const s16x2 z = (d << 1) ^ (d >> 15);
	return __builtin_bit_cast(uint32_t, z);
}

// relaxed agent-scope granule access (sc1: L2-coherent, bypasses this CU's L1)
__device__ __forceinline__ void gran_store(uint64_t *g, uint64_t v)
{
	__hip_atomic_store(g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t gran_load(uint64_t *g)
{
	return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Decoupled look-back, executed by ONE WAVE (all 64 lanes call it): publish this chunk's
// aggregate, sum the aggregates of the chunks before it in the same read - 64 granules per
// round trip, nearest first - and publish the inclusive prefix.  `t` = this chunk's ticket,
// j = its index in the read (chunk t-j is the read's first and always publishes a prefix).
// Returns the exclusive prefix (same value in every lane).  `last`: no chunk of this read
// follows, nothing needs publishing.
__device__ __forceinline__ uint64_t lookback(uint64_t *gran, uint32_t t, uint32_t j, uint64_t mine, bool last)
{
	const uint32_t lane = threadIdx.x & 63;
	if (j == 0) {
		if (!last && lane == 0)
			gran_store(gran + t, G_P | mine);
		return 0;
	}
	if (!last && lane == 0)
		gran_store(gran + t, G_A | mine);
	uint64_t sum = 0;
	uint32_t done = 0; // predecessors already summed
	for (;;) {
		// lane l looks at predecessor number done + l (0 = the chunk right before this one)
		const uint32_t idx = done + lane;
		const bool want = idx < j;
		uint64_t g = 0;
		if (want)
			g = gran_load(gran + (t - 1 - idx));
		const unsigned long long pmask = __ballot(want && (g >> 62) == 2);
		const unsigned long long zmask = __ballot(want && (g >> 62) == 0);
		// usable lanes: everything nearer than the first unpublished granule, up to and
		// including the first prefix
		uint32_t stop = 64;
		if (zmask)
			stop = (uint32_t) __builtin_ctzll(zmask);
		uint32_t firstp = 64;
		if (pmask)
			firstp = (uint32_t) __builtin_ctzll(pmask);
		const bool have_p = firstp < stop;
		const uint32_t take = have_p ? firstp + 1 : stop; // lanes [0, take) are added
		uint64_t v = (lane < take) ? (g & G_MASK) : 0;
#pragma unroll
		for (int dd = 32; dd >= 1; dd >>= 1) {
			const uint32_t lo = (uint32_t) __shfl_xor((int) (uint32_t) v, dd, 64);
			const uint32_t hi = (uint32_t) __shfl_xor((int) (uint32_t) (v >> 32), dd, 64);
			v += ((uint64_t) hi << 32) | lo;
		}
		sum += v;
		done += take;
		if (have_p || done >= j)
			break;
		if (take == 0)
			__builtin_amdgcn_s_sleep(2);
	}
	if (!last && lane == 0)
		gran_store(gran + t, G_P | (sum + mine));
	return sum;
}

// the fields of a chunk descriptor as wave-uniform (scalar) values
struct ChunkU {
	uint64_t sig_off, out_base;
	uint32_t n, j, read, cap_ok;
};
__device__ __forceinline__ ChunkU load_chunk(const ChunkDesc *dp)
{
	ChunkU c;
	c.sig_off = uni64(dp->sig_off);
	c.out_base = uni64(dp->out_base);
	c.n = uni(dp->n);
	c.j = uni(dp->j);
	c.read = uni(dp->read);
	c.cap_ok = uni(dp->cap_ok);
	return c;
}

// The chunk table of a batch: the control block zeroed, then k_chunk_prep (press_svb.hip, which holds the kernel).  hdr:
// bytes in front of the keys (4: the slow5 svb-zd stream).  Press: meta - ReadMeta cleared as well (the exception-split
// family); pk - the slots are the exact ones of the packed svb press (pk->layout, pk->need, pk->out_cap), not a.out_off.
void launch_chunk_prep(const BatchArgs &a, bool key2bit, uint32_t hdr, bool meta, const PackArgs *pk, hipStream_t s);
void launch_chunk_prep(const DecodeArgs &a, bool key2bit, uint32_t hdr, hipStream_t s);

#ifdef DEC_STAMPS
// diagnostic build only: per-chunk phase timestamps (s_memtime), read back by tools.  Every unit that stamps has a table
// of its own (no relocatable device code): stamps_read adds this unit's to dst where dst holds none
static __device__ uint64_t g_stamps[65536 * 8];
#define STAMP(i)                                                                         \
	do {                                                                             \
		if (threadIdx.x == 0 && t < 65536)                                       \
			g_stamps[t * 8 + (i)] = __builtin_amdgcn_s_memtime();             \
	} while (0)
static int stamps_read(uint64_t *dst, uint32_t nwords)
{
	uint64_t *tmp = new uint64_t[nwords];
	const int rc = (int) hipMemcpyFromSymbol(tmp, HIP_SYMBOL(g_stamps), (size_t) nwords * 8);
	for (uint32_t i = 0; rc == 0 && i < nwords; i++)
		if (!dst[i])
			dst[i] = tmp[i];
	delete[] tmp;
	return rc;
}
int ex_stamps_read(uint64_t *dst, uint32_t nwords); // press_exsplit.hip
#else
#define STAMP(i)
#endif

// 8-bit mask of the samples of a lane that are exceptions (value > 255)
__device__ __forceinline__ uint32_t exc_mask(const uint4 &z, uint32_t i0)
{
	const uint32_t zz[4] = { z.x, z.y, z.z, z.w };
	uint32_t m = 0;
#pragma unroll
	for (int h = 0; h < 4; h++) {
		m |= ((zz[h] & 0x0000FF00u) ? 1u : 0u) << (2 * h);
		m |= ((zz[h] & 0xFF000000u) ? 1u : 0u) << (2 * h + 1);
	}
	if (i0 == 0)
		m &= ~1u; // zd[0] is stored raw in the header
	return m;
}

// which of a lane's 8 samples starting at i0 are one-byte values: inside [1, n), no exception
__device__ __forceinline__ uint32_t low_mask(const uint4 &z, uint32_t i0, uint32_t n)
{
	uint32_t lowm = i0 + 8 <= n ? 0xFFu : (i0 < n ? (1u << (n - i0)) - 1u : 0u);
	if (i0 == 0)
		lowm &= ~1u;
	if ((z.x | z.y | z.z | z.w) & 0xFF00FF00u)
		lowm &= ~exc_mask(z, i0);
	return lowm;
}

} // namespace ph
