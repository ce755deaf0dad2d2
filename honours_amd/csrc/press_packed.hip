// press_packed.hip - the kernels that only the packed press has (press_hip_press_sizes / press_hip_press_packed):
// the exact size of an svb stream without writing it, the read-level scan that turns sizes into offsets, and the
// patch of the chunk table with those offsets.  The size halves that need a family's static helpers live next to
// them (k_ex_sizes: press_sections.hip, k_zs_plan<true>: press_zstd.hip, k_chunk_prep<.., true>: press_svb.hip).

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

namespace {

constexpr uint64_t PFAIL = ~0ull;
constexpr uint32_t SZ_SEG = 16; // workgroups a read's samples are dealt to

// ------------------------------------------------------------------ svb: the exact stream length
//
// hdr + keys + n + the extra bytes (a value above 255 takes one more byte, slow5's 17-bit values two): what phase 1 of
// k_svb_encode_chunked counts, here over plain 16-byte loads with nothing kept.  need[] is zeroed by the launcher;
// segment 0 of a read adds the part that depends on n alone, every segment one atomic of its extra bytes (integers:
// the same sum in any order).
template <bool KEY2, bool ZD, bool S5>
__global__ __launch_bounds__(256) void k_pk_svb_sizes(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp,
						      unsigned long long *need)
{
	__shared__ uint32_t s_w[4];
	const uint32_t r = blockIdx.x, seg = blockIdx.y;
	const uint32_t n = uni(nsamp[r]);
	const int16_t *in = sig + uni64(off[r]);
	uint32_t extra = 0;
	for (uint64_t i0 = ((uint64_t) seg * 256 + threadIdx.x) * 8; i0 < n; i0 += (uint64_t) SZ_SEG * 256 * 8) {
		int16_t v[8];
		const uint32_t nv = n - i0 < 8 ? (uint32_t) (n - i0) : 8u;
		if (nv == 8) {
			const uint4 q = ld16_stream(in + i0);
			__builtin_memcpy(v, &q, 16);
		} else { // the read's ragged tail: nothing behind its last sample is touched
			for (uint32_t h = 0; h < 8; h++)
				v[h] = h < nv ? in[i0 + h] : (int16_t) 0;
		}
		int32_t prev = ZD && i0 ? (int32_t) in[i0 - 1] : 0;
#pragma unroll
		for (uint32_t h = 0; h < 8; h++) {
			uint32_t z;
			if (!ZD) {
				z = (uint16_t) v[h];
			} else if (!S5) { // the delta wraps in 16 bits (trans.c:75)
				const int32_t d = (int32_t) (int16_t) ((int32_t) v[h] - prev);
				z = (uint32_t) ((d << 1) ^ (d >> 15)) & 0xFFFFu;
			} else { // slow5lib takes it in 32 bits (streamvbyte_zigzag.c:15): up to 17 bits
				const int32_t d = (int32_t) v[h] - prev;
				z = (uint32_t) ((d << 1) ^ (d >> 31));
			}
			if (h < nv)
				extra += (z > 255u ? 1u : 0u) + (z > 65535u ? 1u : 0u);
			prev = v[h];
		}
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		extra += (uint32_t) __shfl_xor((int) extra, d, 64);
	if ((threadIdx.x & 63) == 0)
		s_w[threadIdx.x >> 6] = extra;
	__syncthreads();
	if (threadIdx.x)
		return;
	unsigned long long add = (unsigned long long) s_w[0] + s_w[1] + s_w[2] + s_w[3];
	if (seg == 0) {
		const uint32_t klen = KEY2 ? (n + 3) / 4 : (n >> 3) + (((n & 7) + 7) >> 3);
		add += (unsigned long long) (S5 ? 4u : 0u) + klen + n;
	}
	if (add)
		atomicAdd(need + r, add);
}

// ------------------------------------------------------------------ sizes -> offsets
//
// One workgroup, 1024 reads a round (nreads is thousands).  layout[0] = 0, layout[r + 1] = layout[r] + need[r]
// rounded up to `align` (a refused read: 0 bytes), layout[nreads] = the end of the last stream, not rounded.  Then,
// from the back, slot[]: see PackArgs.  All in 64 bits.

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d)
{
	const uint32_t lo = (uint32_t) __shfl_up((int) (uint32_t) v, d, 64);
	const uint32_t hi = (uint32_t) __shfl_up((int) (uint32_t) (v >> 32), d, 64);
	return ((uint64_t) hi << 32) | lo;
}

// inclusive scan over the 1024 threads of `v` under OP (sum or min); every thread calls it
template <bool MIN>
__device__ __forceinline__ uint64_t wg_incl_scan64(uint64_t v, uint64_t *wsum)
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint64_t t = shfl_up64(v, d);
		if (lane >= d)
			v = MIN ? (t < v ? t : v) : v + t;
	}
	__syncthreads(); // (wsum of the round before has been read)
	if (lane == 63)
		wsum[w] = v;
	__syncthreads();
	for (int k = 0; k < w; k++)
		v = MIN ? (wsum[k] < v ? wsum[k] : v) : v + wsum[k];
	return v;
}

__global__ __launch_bounds__(1024) void k_pk_scan(const uint64_t *need, uint32_t nreads, uint64_t amask, uint64_t out_cap,
						   uint64_t *layout, uint64_t *slot)
{
	__shared__ uint64_t wsum[16];
	__shared__ uint64_t s_total;
	uint64_t carry = 0;
	for (uint32_t base = 0; base < nreads; base += 1024) {
		const uint32_t r = base + threadIdx.x;
		uint64_t sz = 0;
		if (r < nreads) {
			sz = need[r];
			if (sz == PFAIL)
				sz = 0;
		}
		const uint64_t step = r + 1 < nreads ? (sz + amask) & ~amask : sz; // (the last read's end is not rounded)
		const uint64_t inc = wg_incl_scan64<false>(step, wsum);
		if (r < nreads) {
			if (r == 0)
				layout[0] = 0;
			layout[r + 1] = carry + inc;
		}
		if (threadIdx.x == 1023)
			s_total = inc;
		__syncthreads();
		carry += s_total;
	}
	__syncthreads(); // layout[] is read back below by other threads of this workgroup
	// slot[r] = min over j >= r of (read j fits ? layout[j] : inf), at most layout[nreads]; thread t takes the
	// round's read 1023 - t, so that the scan runs towards the front
	uint64_t behind = carry; // = layout[nreads]
	if (threadIdx.x == 0)
		slot[nreads] = carry;
	const uint32_t rounds = (nreads + 1023) / 1024;
	for (uint32_t k = rounds; k-- > 0;) {
		const uint32_t r = k * 1024 + (1023 - threadIdx.x);
		uint64_t v = PFAIL;
		if (r < nreads) {
			const uint64_t sz = need[r], o = layout[r];
			if (sz == PFAIL || (sz <= out_cap && o <= out_cap - sz))
				v = o;
		}
		uint64_t m = wg_incl_scan64<true>(v, wsum);
		m = m < behind ? m : behind;
		if (r < nreads)
			slot[r] = m;
		if (threadIdx.x == 1023)
			s_total = m;
		__syncthreads();
		behind = s_total;
	}
}

// ------------------------------------------------------------------ packed recode: reads the SOURCE refused
//
// The press half of a recode sees such a read as an empty one (launch_recode_counts), for which some destinations have a
// size - 4 bytes of slow5_svb_zd, a frame of zstd over svb.  It takes no byte: need[r] = FAILED before the scan.
__global__ __launch_bounds__(256) void k_pk_refused(const uint32_t *out_n, uint64_t *need, uint32_t nreads)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r < nreads && out_n[r] == 0xFFFFFFFFu)
		need[r] = PFAIL;
}

// ... and no slot: k_pk_scan gives a refused read slot[r] = layout[r], which is a slot of no bytes only while read r + 1
// starts there - not when r + 1 does not fit out_cap and slot[r + 1] is a later read's offset, and a writer that has a
// stream for an empty read would put it into that room.  The slot table is made again from layout[] with the source's
// refusals counted as reads that do not fit (slot[r] = slot[r + 1]); everything else as k_pk_scan's second half.  A
// read in front keeps at least its need[]: the room of a refused read falls to it as that of a read that does not fit.
__global__ __launch_bounds__(1024) void k_pk_refused_slots(const uint64_t *need, const uint32_t *out_n, uint32_t nreads,
							   uint64_t out_cap, const uint64_t *layout, uint64_t *slot)
{
	__shared__ uint64_t wsum[16];
	__shared__ uint64_t s_total;
	uint64_t behind = layout[nreads];
	if (threadIdx.x == 0)
		slot[nreads] = behind;
	const uint32_t rounds = (nreads + 1023) / 1024;
	for (uint32_t k = rounds; k-- > 0;) {
		const uint32_t r = k * 1024 + (1023 - threadIdx.x);
		uint64_t v = PFAIL;
		if (r < nreads && out_n[r] != 0xFFFFFFFFu) {
			const uint64_t sz = need[r], o = layout[r];
			if (sz == PFAIL || (sz <= out_cap && o <= out_cap - sz))
				v = o;
		}
		uint64_t m = wg_incl_scan64<true>(v, wsum);
		m = m < behind ? m : behind;
		if (r < nreads)
			slot[r] = m;
		if (threadIdx.x == 1023)
			s_total = m;
		__syncthreads();
		behind = s_total;
	}
}

// ChunkDesc::out_base of every chunk of a read: k_chunk_prep ran before the offsets existed.  One wave per read.
__global__ __launch_bounds__(256) void k_pk_patch(ChunkDesc *chunks, const uint32_t *first_chunk, const uint32_t *nsamp,
						  const uint64_t *slot, uint32_t nreads, uint32_t max_chunks)
{
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (r >= nreads)
		return;
	const uint32_t nch = (nsamp[r] + CHUNK - 1) / CHUNK;
	const uint32_t first = first_chunk[r];
	const uint64_t base = slot[r];
	for (uint32_t j = threadIdx.x & 63; j < nch && first + j < max_chunks; j += 64)
		chunks[first + j].out_base = base;
}

template <bool KEY2, bool ZD, bool S5>
void run_svb_sizes(const BatchArgs &a, uint64_t *need, hipStream_t s)
{
	hipLaunchKernelGGL((k_pk_svb_sizes<KEY2, ZD, S5>), dim3(a.nreads, SZ_SEG), dim3(256), 0, s, a.sig, a.off, a.nsamp,
			   (unsigned long long *) need);
}

} // namespace

void launch_pack_svb_sizes(const BatchArgs &a, bool key2bit, bool zd, bool slow5, uint64_t *need, hipStream_t s)
{
	(void) hipMemsetAsync(need, 0, (size_t) a.nreads * 8, s);
	if (slow5)
		run_svb_sizes<true, true, true>(a, need, s);
	else if (key2bit)
		run_svb_sizes<true, true, false>(a, need, s);
	else if (zd)
		run_svb_sizes<false, true, false>(a, need, s);
	else
		run_svb_sizes<false, false, false>(a, need, s);
}

void launch_pack_scan(const PackArgs &pk, uint32_t nreads, hipStream_t s)
{
	hipLaunchKernelGGL(k_pk_scan, dim3(1), dim3(1024), 0, s, (const uint64_t *) pk.need, nreads, (uint64_t) pk.align - 1,
			   pk.out_cap, pk.layout, pk.slot);
}

// need[] of the reads the source refused, and - with a layout - the scan and the slot table of a packed recode
void launch_pack_scan_refused(const PackArgs &pk, const uint32_t *out_n, uint32_t nreads, hipStream_t s)
{
	hipLaunchKernelGGL(k_pk_refused, dim3((nreads + 255) / 256), dim3(256), 0, s, out_n, pk.need, nreads);
	if (!pk.layout)
		return;
	launch_pack_scan(pk, nreads, s);
	hipLaunchKernelGGL(k_pk_refused_slots, dim3(1), dim3(1024), 0, s, (const uint64_t *) pk.need, out_n, nreads, pk.out_cap,
			   (const uint64_t *) pk.layout, pk.slot);
}

void launch_pack_patch(const BatchArgs &a, const uint64_t *slot, hipStream_t s)
{
	hipLaunchKernelGGL(k_pk_patch, dim3((a.nreads + 3) / 4), dim3(256), 0, s, a.chunks, (const uint32_t *) a.first_chunk,
			   a.nsamp, slot, a.nreads, a.max_chunks);
}

} // namespace ph
