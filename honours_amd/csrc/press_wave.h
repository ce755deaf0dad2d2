// press_wave.h - wave-level helpers shared by the kernel files.  Only moves of bits and integer arithmetic: the units that
// compile with fp contract(off) include this header, and a float operation here would escape their pragma.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ph {

typedef short s16x2 __attribute__((ext_vector_type(2)));

// wave-uniform values: tell the compiler (scalar registers, scalar branches)
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t) __builtin_amdgcn_readfirstlane((int) v); }
// uni() of a 64-bit value
__device__ __forceinline__ uint64_t uni64(uint64_t v)
{
	return ((uint64_t) uni((uint32_t) (v >> 32)) << 32) | uni((uint32_t) v);
}

// The clamped range of a read of c samples (include/press_hip.h 2y): b' = min(b, c), a' = min(a, b') of range[2r],
// range[2r + 1]; range NULL: [0, c)
__device__ __forceinline__ uint2 range_clamp(const uint32_t *range, uint32_t r, uint32_t c)
{
	if (!range)
		return make_uint2(0u, c);
	const uint32_t a = range[2 * (size_t) r], b = range[2 * (size_t) r + 1];
	const uint32_t hi = b < c ? b : c;
	return make_uint2(a < hi ? a : hi, hi);
}

// 16 bytes of a stream that is read once: non-temporal policy (tools/ubench_stream.hip: a read-only sweep reaches
// 7.1 TB/s with it against 6.3 TB/s with the default policy, a copy 6.0 against 5.2-5.6)
#ifndef PRESS_NO_NT
__device__ __forceinline__ uint4 ld16_stream(const void *p)
{
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
	return make_uint4(v.x, v.y, v.z, v.w);
}
#else
__device__ __forceinline__ uint4 ld16_stream(const void *p) { return *reinterpret_cast<const uint4 *>(p); }
#endif

// value of the previous lane (lane 0 receives `lane0`)
__device__ __forceinline__ uint32_t prev_lane(uint32_t v, uint32_t lane0)
{
	// DPP wave_shr:1 - lane l reads lane l-1; lane 0 keeps `old`
	return (uint32_t) __builtin_amdgcn_update_dpp((int) lane0, (int) v, 0x138, 0xf, 0xf, false);
}

// v of `lane` (wave-uniform), to every lane
__device__ __forceinline__ float lane_f32(float v, uint32_t lane)
{
	return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int) lane));
}
__device__ __forceinline__ double lane_f64(double v, uint32_t lane)
{
	const uint64_t b = (uint64_t) __double_as_longlong(v);
	const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) b, (int) lane);
	const uint32_t hi = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) (b >> 32), (int) lane);
	return __longlong_as_double((long long) (((uint64_t) hi << 32) | lo));
}

// inclusive sum over the lanes of a wave
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v, uint32_t lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint64_t o = __shfl_up(v, d, 64);
		if (lane >= (uint32_t) d)
			v += o;
	}
	return v;
}

// ... of 32-bit values
__device__ __forceinline__ uint32_t scan32(uint32_t v, uint32_t lane)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = (uint32_t) __shfl_up((int) v, d, 64);
		if (lane >= (uint32_t) d)
			v += o;
	}
	return v;
}

// sum / maximum over the lanes of a wave, to every lane
__device__ __forceinline__ uint64_t sum64(uint64_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v += __shfl_xor(v, d, 64);
	return v;
}
__device__ __forceinline__ uint32_t max32(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const uint32_t o = (uint32_t) __shfl_xor((int) v, d, 64);
		v = o > v ? o : v;
	}
	return v;
}

// make the LDS writes of this wave visible to its other lanes (DS ops of a wave execute in
// order; this only stops the compiler from moving them)
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// zig-zag delta of the two samples packed in `cur`, given the dword holding the two
// samples before them (trans.c:75,215 on packed 16-bit lanes)
__device__ __forceinline__ uint32_t zd_pair(uint32_t cur, uint32_t prevdw)
{
	const uint32_t sh = __builtin_amdgcn_alignbit(cur, prevdw, 16); // [prev.hi, cur.lo]
	const s16x2 d = __builtin_bit_cast(s16x2, cur) - __builtin_bit_cast(s16x2, sh);
	const s16x2 z = (d << 1) ^ (d >> 15);
	return __builtin_bit_cast(uint32_t, z);
}

// D_b (include/press_hip.h, press_hip_degrade_value) of the two samples packed in v, for b = 1 .. 8: round to the nearest
// multiple of 2^b, ties up, saturating.  h2 = 2^(b-1) and m2 = ~(2^b - 1) in both halves (degrade_h2, degrade_m2).  The add
// saturates (v_pk_add_i16 clamp), which is the definition's min: where s + 2^(b-1) passes 32767 the sum becomes 32767,
// whose multiple below is 32768 - 2^b, the top bucket; where it does not, the 16-bit sum is the 32-bit one and its
// multiple below cannot exceed that bucket.  Clearing the low bits is the arithmetic shift down and up again.
__device__ __forceinline__ uint32_t degrade_pair(uint32_t v, uint32_t h2, uint32_t m2)
{
	const s16x2 s = __builtin_elementwise_add_sat(__builtin_bit_cast(s16x2, v), __builtin_bit_cast(s16x2, h2));
	return __builtin_bit_cast(uint32_t, s) & m2;
}
// (b = 0: h2 = 0 and m2 = all ones, the identity)
__host__ __device__ __forceinline__ uint32_t degrade_h2(uint32_t bits) { return bits ? 0x00010001u << (bits - 1) : 0u; }
__host__ __device__ __forceinline__ uint32_t degrade_m2(uint32_t bits) { return ~(((1u << bits) - 1u) * 0x00010001u); }

} // namespace ph
