// press_rows.hip - the writer of press_hip_depress_chunks_batch: decoded int16 samples in library scratch -> the rows a
// basecaller takes, [rows, T] of float32, float16 or bfloat16.
//
// Read r owns rows row_first[r] .. row_first[r + 1) (press_hip_chunk_plan over the ROOMS n[r], so the layout is known
// on the host).  Row j of a read of c = n[r] samples starts at sample j * S, S = T - overlap, except the last row of a
// read longer than T, which starts at c - T.  Column t of the row holds round_to_dtype(((float) s + c0) * c1) of sample
// start + t - k_pa_convert's arithmetic, then one more rounding to nearest even - or +0 where start + t is at or beyond the
// read's decoded count (all of a refused read).
//
// A lane makes 8 columns: 16 bytes of float16 / bfloat16 or 32 of float32, in stores of 16 bytes that are aligned
// because T is a multiple of 8.  A row's source start is any sample, so the 8 samples come from the one or two aligned
// 16-byte groups that hold them, shifted into place in registers; a group is loaded only where it begins inside the
// read's room of roundup8(c) samples.  T >= 2048: a workgroup writes one row, 2048 columns per step, and looks its read up
// once, in scalar registers.  T < 2048: a workgroup writes floor(2048 / T) whole rows and every lane looks up its own row's read.
// The look-up is a binary search in row_first; reads without rows are skipped by it.

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

constexpr uint32_t ROW_COLS = 2048; // columns a workgroup writes: 256 lanes x 8
constexpr uint32_t ROW_FAIL = 0xFFFFFFFFu; // out_n of a refused read

__device__ __forceinline__ float row_scale(int32_t smp, float c0, float c1)
{
#pragma clang fp contract(off)
	const float t = (float) smp + c0;
	return t * c1;
}

// float32 -> bfloat16 bits, to nearest even on the bit pattern; a NaN stays a quiet NaN of its sign
__device__ __forceinline__ uint32_t bf16_bits(float y)
{
	const uint32_t u = __float_as_uint(y);
	if ((u & 0x7FFFFFFFu) > 0x7F800000u)
		return (u >> 16) | 0x40u;
	return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// float32 -> float16 bits: one rounding of the float32 to nearest even, overflow to infinity, subnormals kept
// (v_cvt_f16_f32).  The empty asm keeps y a float32 in a register: without it the compiler folds the multiply that made y
// and this conversion into v_fma_mixlo_f16, which rounds the exact product once - another number in 1 of 10^4 samples.
__device__ __forceinline__ uint32_t f16_bits(float y)
{
	asm volatile("" : "+v"(y));
	const _Float16 h = (_Float16) y;
	return (uint32_t) __builtin_bit_cast(uint16_t, h);
}

// the read that owns `row`: the largest r with row_first[r] <= row, for row < row_first[nreads]
__device__ __forceinline__ uint32_t row_read_of(const uint64_t *row_first, uint32_t nreads, uint64_t row)
{
	uint32_t lo = 0, hi = nreads; // row_first[lo] <= row < row_first[hi]
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (row_first[mid] <= row)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// what the columns of one row are made of: the read's samples from `start` on, `on` of them decoded, its two floats
struct RowSrc {
	const int16_t *in; // the read's room, roundup8 samples of it readable
	uint64_t start;
	uint32_t on, cnt8;
	float c0, c1;
};

__device__ __forceinline__ RowSrc row_src(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, const uint32_t *out_n,
					   const float *cal, const uint64_t *row_first, uint32_t r, uint64_t row, uint32_t T, uint32_t S)
{
	RowSrc s;
	const uint32_t c = nsamp[r];
	const bool last = row + 1 == row_first[r + 1];
	s.start = last && c > T ? (uint64_t) (c - T) : (row - row_first[r]) * S;
	const uint32_t raw = out_n[r];
	s.on = raw == ROW_FAIL ? 0u : raw < c ? raw : c; // (no decoder gives more than the room)
	s.cnt8 = (c + 7u) & ~7u;
	s.in = sig + off[r];
	s.c0 = cal[2 * (size_t) r]; // (a refused read's floats are never used: on = 0)
	s.c1 = cal[2 * (size_t) r + 1];
	return s;
}

// 8 columns from `col` of the row that begins at `out`
template <int DT>
__device__ __forceinline__ void row_cols(const RowSrc &s, uint64_t col, uint8_t *out)
{
	const uint64_t p = s.start + col; // the first sample of this lane's 8
	uint32_t x[8] = {};
	if (p < s.on) {
		// (p < on <= c: the group at g lies in the room; the next one only where g + 8 < roundup8(c))
		const uint64_t g = p & ~7ull;
		const uint32_t sh = (uint32_t) (p & 7u);
		const int16_t *in = s.in + g;
		const uint4 a = ld16_stream(in);
		uint4 b = make_uint4(0, 0, 0, 0);
		if (sh && g + 8 < s.cnt8)
			b = ld16_stream(in + 8);
		// 8 samples from halfword sh of the 16: by whole dwords first (sh >> 1 in 0 .. 3), then by the odd halfword
		// (named values, not arrays: selects between array elements become indexed loads of a private copy)
		const bool s4 = sh & 4u, s2 = sh & 2u, s1 = sh & 1u;
		const uint32_t u0 = s4 ? a.z : a.x, u1 = s4 ? a.w : a.y, u2 = s4 ? b.x : a.z, u3 = s4 ? b.y : a.w, u4 = s4 ? b.z : b.x,
			       u5 = s4 ? b.w : b.y;
		const uint32_t v0 = s2 ? u1 : u0, v1 = s2 ? u2 : u1, v2 = s2 ? u3 : u2, v3 = s2 ? u4 : u3, v4 = s2 ? u5 : u4;
		const uint32_t d[4] = { s1 ? __builtin_amdgcn_alignbit(v1, v0, 16) : v0, s1 ? __builtin_amdgcn_alignbit(v2, v1, 16) : v1,
					s1 ? __builtin_amdgcn_alignbit(v3, v2, 16) : v2, s1 ? __builtin_amdgcn_alignbit(v4, v3, 16) : v3 };
		const uint32_t nv = s.on - p < 8 ? (uint32_t) (s.on - p) : 8u;
#pragma unroll
		for (int e = 0; e < 8; e++) {
			const int32_t smp = (e & 1) ? (int32_t) d[e >> 1] >> 16 : (int32_t) (int16_t) (d[e >> 1] & 0xFFFFu);
			const float y = row_scale(smp, s.c0, s.c1);
			const uint32_t bits = DT == PRESS_ROWS_F32 ? __float_as_uint(y) : DT == PRESS_ROWS_F16 ? f16_bits(y) : bf16_bits(y);
			x[e] = (uint32_t) e < nv ? bits : 0u;
		}
	}
	if (DT == PRESS_ROWS_F32) {
		uint8_t *o = out + col * 4;
		*reinterpret_cast<uint4 *>(o) = make_uint4(x[0], x[1], x[2], x[3]);
		*reinterpret_cast<uint4 *>(o + 16) = make_uint4(x[4], x[5], x[6], x[7]);
	} else {
		*reinterpret_cast<uint4 *>(out + col * 2) = make_uint4(x[0] | x[1] << 16, x[2] | x[3] << 16, x[4] | x[5] << 16, x[6] | x[7] << 16);
	}
}

template <int DT> // PRESS_HIP_F32 / F16 / BF16
__global__ __launch_bounds__(256) void k_chunk_rows(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, const uint32_t *out_n,
						     const float *cal, const uint64_t *row_first, uint32_t nreads, uint8_t *rows,
						     uint64_t nrows_cap, uint32_t T, uint32_t S)
{
	constexpr uint32_t ES = DT == PRESS_ROWS_F32 ? 4 : 2;
	const uint64_t planned = uni64(row_first[nreads]);
	const uint64_t nrows = planned < nrows_cap ? planned : nrows_cap;
	if (T >= ROW_COLS) { // a row per workgroup, ROW_COLS columns per step: one search and one set of the read's values per row
		for (uint64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
			const uint32_t r = uni(row_read_of(row_first, nreads, row));
			const RowSrc s = row_src(sig, off, nsamp, out_n, cal, row_first, r, row, T, S);
			uint8_t *out = rows + row * T * ES;
			for (uint64_t col = threadIdx.x * 8; col < T; col += ROW_COLS) // (64 bits: col + ROW_COLS may pass 2^32)
				row_cols<DT>(s, col, out);
		}
		return;
	}
	const uint32_t rpb = ROW_COLS / T; // rows of a workgroup
	const uint64_t nblocks = (nrows + rpb - 1) / rpb;
	const uint32_t lr = threadIdx.x * 8 / T, col = threadIdx.x * 8 - lr * T;
	if (lr >= rpb)
		return;
	for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
		const uint64_t row = blk * rpb + lr;
		if (row >= nrows)
			continue;
		const uint32_t r = row_read_of(row_first, nreads, row);
		const RowSrc s = row_src(sig, off, nsamp, out_n, cal, row_first, r, row, T, S);
		row_cols<DT>(s, col, rows + row * T * ES);
	}
}

// The rows of press_hip_depress_chunks_trimmed_batch: read r gives the L = b' - a' samples [a', b') of cut[2r], cut[2r + 1]
// (clamped by k_trim_cut: b' is at most the decoded count), row_first is the plan over the L[r] and lies in device memory
// like the cuts.  A row's source start is a' + the plan's start for a read of L samples, its decoded bound b'; the room
// and its groups are the read's, as above.  The lane that makes a row's first columns writes its row_read / row_start.
__device__ __forceinline__ RowSrc row_src_ranged(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, const uint32_t *cut,
						  const float *cal, const uint64_t *row_first, uint32_t r, uint64_t row, uint32_t T, uint32_t S)
{
	RowSrc s;
	const uint32_t a = cut[2 * (size_t) r], b = cut[2 * (size_t) r + 1];
	const uint32_t L = b - a;
	const bool last = row + 1 == row_first[r + 1];
	s.start = a + (last && L > T ? (uint64_t) (L - T) : (row - row_first[r]) * S);
	s.on = b;
	s.cnt8 = (nsamp[r] + 7u) & ~7u;
	s.in = sig + off[r];
	s.c0 = cal[2 * (size_t) r];
	s.c1 = cal[2 * (size_t) r + 1];
	return s;
}

template <int DT>
__global__ __launch_bounds__(256) void k_chunk_rows_ranged(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, const uint32_t *cut,
							    const float *cal, const uint64_t *row_first, uint32_t nreads, uint8_t *rows,
							    uint64_t nrows_cap, uint32_t T, uint32_t S, uint32_t *row_read, uint32_t *row_start)
{
	constexpr uint32_t ES = DT == PRESS_ROWS_F32 ? 4 : 2;
	const uint64_t planned = uni64(row_first[nreads]);
	const uint64_t nrows = planned < nrows_cap ? planned : nrows_cap;
	if (T >= ROW_COLS) {
		for (uint64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
			const uint32_t r = uni(row_read_of(row_first, nreads, row));
			const RowSrc s = row_src_ranged(sig, off, nsamp, cut, cal, row_first, r, row, T, S);
			uint8_t *out = rows + row * T * ES;
			for (uint64_t col = threadIdx.x * 8; col < T; col += ROW_COLS)
				row_cols<DT>(s, col, out);
			if (threadIdx.x == 0) {
				if (row_read)
					row_read[row] = r;
				if (row_start)
					row_start[row] = (uint32_t) s.start;
			}
		}
		return;
	}
	const uint32_t rpb = ROW_COLS / T; // rows of a workgroup
	const uint64_t nblocks = (nrows + rpb - 1) / rpb;
	const uint32_t lr = threadIdx.x * 8 / T, col = threadIdx.x * 8 - lr * T;
	if (lr >= rpb)
		return;
	for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
		const uint64_t row = blk * rpb + lr;
		if (row >= nrows)
			continue;
		const uint32_t r = row_read_of(row_first, nreads, row);
		const RowSrc s = row_src_ranged(sig, off, nsamp, cut, cal, row_first, r, row, T, S);
		row_cols<DT>(s, col, rows + row * T * ES);
		if (col == 0) {
			if (row_read)
				row_read[row] = r;
			if (row_start)
				row_start[row] = (uint32_t) s.start;
		}
	}
}

// ... of the trimmed call: the grid is the same bound, as L[r] <= n[r]
void launch_chunk_rows_ranged(const DecodeArgs &a, const uint32_t *cut, const float *cal, const uint64_t *row_first, void *rows,
			      uint64_t nrows_cap, int dtype, uint32_t T, uint32_t overlap, uint64_t total_samples, uint32_t *row_read,
			      uint32_t *row_start, hipStream_t s)
{
	const uint32_t S = T - overlap;
	uint64_t bound = (uint64_t) a.nreads + total_samples / S;
	if (bound > nrows_cap)
		bound = nrows_cap;
	if (!a.nreads || !bound)
		return;
	const uint64_t nb = T >= ROW_COLS ? bound : (bound + ROW_COLS / T - 1) / (ROW_COLS / T);
	const dim3 g((uint32_t) (nb < 0x7FFFFFFFull ? nb : 0x7FFFFFFFull)), b(256);
	const int16_t *sig = a.sig;
	if (dtype == PRESS_ROWS_F32)
		hipLaunchKernelGGL((k_chunk_rows_ranged<PRESS_ROWS_F32>), g, b, 0, s, sig, a.off, a.nsamp, cut, cal, row_first, a.nreads,
				   (uint8_t *) rows, nrows_cap, T, S, row_read, row_start);
	else if (dtype == PRESS_ROWS_F16)
		hipLaunchKernelGGL((k_chunk_rows_ranged<PRESS_ROWS_F16>), g, b, 0, s, sig, a.off, a.nsamp, cut, cal, row_first, a.nreads,
				   (uint8_t *) rows, nrows_cap, T, S, row_read, row_start);
	else
		hipLaunchKernelGGL((k_chunk_rows_ranged<PRESS_ROWS_BF16>), g, b, 0, s, sig, a.off, a.nsamp, cut, cal, row_first, a.nreads,
				   (uint8_t *) rows, nrows_cap, T, S, row_read, row_start);
}

// rows of the batch: every planned row below nrows_cap.  The grid is what the host knows: no read has more than
// 1 + n[r] / S rows and the rooms lie within total_samples, so nreads + total_samples / S bounds the planned rows.
void launch_chunk_rows(const DecodeArgs &a, const float *cal, const uint64_t *row_first, void *rows, uint64_t nrows_cap, int dtype,
		       uint32_t T, uint32_t overlap, uint64_t total_samples, hipStream_t s)
{
	const uint32_t S = T - overlap;
	uint64_t bound = (uint64_t) a.nreads + total_samples / S;
	if (bound > nrows_cap)
		bound = nrows_cap;
	if (!a.nreads || !bound)
		return;
	const uint64_t nb = T >= ROW_COLS ? bound : (bound + ROW_COLS / T - 1) / (ROW_COLS / T);
	const dim3 g((uint32_t) (nb < 0x7FFFFFFFull ? nb : 0x7FFFFFFFull)), b(256);
	const int16_t *sig = a.sig;
	const uint32_t *on = a.out_n;
	if (dtype == PRESS_ROWS_F32)
		hipLaunchKernelGGL((k_chunk_rows<PRESS_ROWS_F32>), g, b, 0, s, sig, a.off, a.nsamp, on, cal, row_first, a.nreads, (uint8_t *) rows,
				   nrows_cap, T, S);
	else if (dtype == PRESS_ROWS_F16)
		hipLaunchKernelGGL((k_chunk_rows<PRESS_ROWS_F16>), g, b, 0, s, sig, a.off, a.nsamp, on, cal, row_first, a.nreads, (uint8_t *) rows,
				   nrows_cap, T, S);
	else
		hipLaunchKernelGGL((k_chunk_rows<PRESS_ROWS_BF16>), g, b, 0, s, sig, a.off, a.nsamp, on, cal, row_first, a.nreads, (uint8_t *) rows,
				   nrows_cap, T, S);
}

} // namespace ph
