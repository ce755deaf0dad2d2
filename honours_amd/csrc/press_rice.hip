// press_rice.hip - entropy stage 6 of the exception-split methods: Golomb-Rice coding of the one-byte values
// (rice_press / rice_depress, press.c:4860-4978, as the reference's rice_*_zd methods call them).
//
// Payload (include/press_hip.h section 2u; pinned by tests/_rice.py and tests/golden/ref_rice.json):
//   bit i of the payload is bit i % 8, from the least significant, of byte i / 8;
//   bits 0, 1, 2 = k >> 2 & 1, k >> 1 & 1, k & 1; then per value x: x >> k one-bits, a zero bit, the low k bits of x
//   from the most significant down;
//   k = the smallest of 0 .. 7 that minimises sum((x >> k) + 1 + k), sums in 64 bits (no value: k = 0);
//   nbits = 3 + that sum, (nbits - 1) / 8 + 1 bytes, the bits behind nbits in the last byte zero.
// Decoder: k from the first three bits; per value the run of ones counted modulo 256 (however long it is), the zero
// bit, k bits; value = (uint8_t) ((q << k) | rem); bits behind the stream's end are zero, nothing outside the stream
// is read.
//
// Units, the staged writer, subsequences, tiles, records and the repair scheme are the prefix-code engine's
// (press_prefix.h), which the kernels below wrap with the policy RiceCode.  The family's own:
//   k_rice_count   per unit the eight sums of x >> k
//   k_rice_pick    per read: the totals, k, nbits, the length and the slot check; then the engine's scan of the units'
//                  bits at the chosen k, from bit 3
//   k_rice_write   the three bits of k, and per value the run, the zero bit and the remainder through the engine's writer
//   rice_code      one code by arithmetic: the decoder's state is k alone, from the payload's first byte (k_rice_dplan),
//                  and the tile kernels use no LDS for it
// PRESS: count, pick, write, copy.  PRESS SIZES (need != NULL): count and pick alone, nothing else is written.
// PACKED PRESS: the sizes, and once the arena is laid out k_rice_place (the slot check), write, copy.
// DEPRESS: dplan, sync, fix x 2, check, dscan, emit, walk.  A run of more than RICE_RUNCAP ones makes sync and fix give
// the subsequence up (the walk reads it a dword per step), so no lane spends more than a bounded time on bits that are
// not its own.  The walk stops at the payload's end: behind it every value is 0.

#include "press_prefix.h"

namespace ph {

namespace {

constexpr uint32_t RICE_RUNCAP = 4096;

// one code from p on: p moves behind it, v = its value; false: a run longer than cap (p is then inside the run)
__device__ __forceinline__ bool rice_code(const PfxBits &b, uint32_t k, uint64_t &p, uint32_t &v, uint64_t cap)
{
	uint64_t run = 0;
	uint32_t w, ones;
	for (;;) {
		w = peek32(b, p);
		ones = w == ~0u ? 32u : (uint32_t) __builtin_ctz(~w);
		p += ones;
		run += ones;
		if (ones < 32)
			break;
		if (run > cap)
			return false;
	}
	p += 1;
	uint32_t rem = 0;
	if (k) {
		const uint32_t f = ones + 1 + k <= 32 ? w >> (ones + 1) : peek32(b, p);
		rem = __brev(f & ((1u << k) - 1u)) >> (32 - k);
	}
	p += k;
	v = (((uint32_t) run << k) | rem) & 0xFFu; // (q is a uint8_t in the reference: the run counts modulo 256)
	return true;
}

struct RiceCode {
	static constexpr uint32_t FIRST_BIT = 3;
	static constexpr bool LDS_STATE = false, KEEP_PARTIAL = false, STRICT_END = false;
	struct State {
		uint32_t k;
	};
	static __device__ __forceinline__ uint32_t press_extra(const PfxRead &) { return 0; }
	static __device__ __forceinline__ bool takes_part(const DecodeArgs &, uint32_t) { return true; }
	static __device__ __forceinline__ uint32_t extra(const DecodeArgs &, uint32_t) { return 0; }
	static __device__ __forceinline__ uint32_t plan_k(const uint8_t *pay, uint64_t paylen)
	{
		if (!paylen)
			return 0;
		const uint32_t b = pay[0];
		return ((b & 1u) << 2) | (b & 2u) | ((b >> 2) & 1u);
	}
	static __device__ __forceinline__ State tile_state(const DecodeArgs &a, uint32_t r) { return { uni(a.ri_drd[r].k) }; }
	static __device__ __forceinline__ State read_state(const DecodeArgs &a, uint32_t r) { return tile_state(a, r); }
	template <bool BOUNDED>
	static __device__ __forceinline__ bool code(const PfxBits &b, const State &st, uint64_t &p, uint32_t &v)
	{
		return rice_code(b, st.k, p, v, BOUNDED ? RICE_RUNCAP : ~0ull);
	}
};

} // namespace

__global__ __launch_bounds__(256) void k_rice_count(BatchArgs a)
{
	const uint32_t lane = threadIdx.x & 63;
	PfxUnit x;
	if (!unit_of(a, x))
		return;
	const uint8_t *in = a.low_tmp + x.soff + x.v0;
	uint32_t s[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	for (uint32_t step = 0; step < PFX_UNIT; step += 512) {
		uint32_t nv;
		const uint64_t v = load8(in, step + lane * 8, x.cnt, nv);
		for (uint32_t j = 0; j < nv; j++) {
			const uint32_t b = (uint32_t) (v >> (8 * j)) & 0xFFu;
#pragma unroll
			for (int k = 0; k < 8; k++)
				s[k] += b >> k;
		}
	}
#pragma unroll
	for (int k = 0; k < 8; k++) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1)
			s[k] += (uint32_t) __shfl_xor((int) s[k], d, 64);
	}
	if (lane == 0) {
		uint32_t *o = a.ri_sum + (size_t) x.u * 8;
#pragma unroll
		for (int k = 0; k < 8; k++)
			o[k] = s[k];
	}
}

// One wave per read.  need == NULL: press (behind k_ex_section: out_len = FAILED and status != 0 for a read it
// refused); else sizes (behind k_ex_sizes, which left header + section in need[r], or FAILED).
__global__ __launch_bounds__(64) void k_rice_pick(BatchArgs a, uint64_t *need)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const ReadMeta *m = a.meta + r;
	const uint32_t n = a.nsamp[r];
	PfxRead *rd = a.ri_rd + r;
	const bool refused = n == 0 || (need ? need[r] == PFX_FAIL64 : m->status != 0);
	if (refused) {
		if (lane == 0) {
			rd->ok = 0;
			rd->nunits = 0;
			if (a.ri_k)
				a.ri_k[r] = 0;
		}
		return;
	}
	const uint64_t nlow = (uint64_t) n - 1 - m->nex;
	const uint32_t nunits = (uint32_t) ((nlow + PFX_UNIT - 1) / PFX_UNIT);
	const size_t u0 = (size_t) a.first_chunk[r] * PFX_UPC;
	uint64_t S[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	for (uint32_t i = lane; i < nunits; i += 64) {
#pragma unroll
		for (int k = 0; k < 8; k++)
			S[k] += a.ri_sum[(u0 + i) * 8 + k];
	}
	uint32_t best = 0;
	uint64_t best_c = PFX_FAIL64;
#pragma unroll
	for (int k = 0; k < 8; k++) {
		const uint64_t c = sum64(S[k]) + nlow * (uint64_t) (1 + k);
		if (c < best_c) { // (press.c:4884: '<', ties go to the lower k)
			best_c = c;
			best = (uint32_t) k;
		}
	}
	const uint64_t nbits = 3 + best_c;
	const uint64_t paylen = (nbits - 1) / 8 + 1;
	prefix_unit_scan(a, r, nunits, RiceCode::FIRST_BIT, [&](size_t entry, uint32_t i) {
		const uint64_t left = nlow - (uint64_t) i * PFX_UNIT;
		return a.ri_sum[entry * 8 + best] + (left < PFX_UNIT ? left : PFX_UNIT) * (1 + best);
	});
	if (lane)
		return;
	bool ok = true;
	if (need) {
		need[r] += paylen;
	} else {
		const uint64_t total = (uint64_t) m->hdr + m->seclen + paylen;
		ok = total <= a.out_off[r + 1] - a.out_off[r];
		a.out_len[r] = ok ? total : PFX_FAIL64;
	}
	rd->nbits = nbits;
	rd->paylen = paylen;
	rd->k = best;
	rd->ok = ok ? 1 : 0;
	rd->nlow = (uint32_t) nlow;
	rd->nunits = nunits;
	if (a.ri_k)
		a.ri_k[r] = (uint8_t) best;
}

// The packed press's write half (launch_rice_write_sized), one lane per read: behind k_rice_pick's sizes mode, which left
// k, the lengths and the units' first bits in ri_rd / ri_start, and behind k_ex_section against the laid-out slot.  What
// k_rice_pick's press mode decides last: the slot check, out_len, ok.
__global__ __launch_bounds__(256) void k_rice_place(BatchArgs a)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= a.nreads)
		return;
	const ReadMeta *m = a.meta + r;
	PfxRead *rd = a.ri_rd + r;
	if (!rd->ok)
		return; // (refused by the size half: k_ex_section has refused it too)
	if (m->status != 0) { // a slot of no bytes: the read does not fit out_cap
		rd->ok = 0;
		return;
	}
	const uint64_t total = (uint64_t) m->hdr + m->seclen + rd->paylen;
	const bool ok = total <= a.out_off[r + 1] - a.out_off[r];
	a.out_len[r] = ok ? total : PFX_FAIL64;
	rd->ok = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_rice_write(BatchArgs a)
{
	__shared__ uint32_t s_bits[4][PFX_WIN];
	PfxUnit x;
	if (!unit_of(a, x))
		return;
	const PfxRead *rd = a.ri_rd + x.r;
	if (!uni(rd->ok))
		return;
	const uint32_t k = uni(rd->k);
	if (x.v0 == 0 && (threadIdx.x & 63) == 0 && k)
		atomicOr(reinterpret_cast<uint32_t *>(a.ri_pay + 2 * x.soff), ((k >> 2) & 1u) | (((k >> 1) & 1u) << 1) | ((k & 1u) << 2));
	prefix_write(
		a, x, s_bits[threadIdx.x >> 6], [&](uint32_t b) { return (b >> k) + 1 + k; },
		[&](auto &put, uint64_t &p, uint32_t b) {
			uint32_t q = b >> k;
			while (q) { // a run can cross eight dwords
				const uint32_t c = q < 32 ? q : 32u;
				put(p, c == 32 ? ~0u : (1u << c) - 1u, c);
				p += c;
				q -= c;
			}
			p += 1; // the zero bit
			if (k)
				put(p, __brev(b & ((1u << k) - 1u)) >> (32 - k), k);
			p += k;
		});
}

__global__ __launch_bounds__(256) void k_rice_copy(BatchArgs a) { prefix_copy<RiceCode>(a); }

// ------------------------------------------------------------------ depress

__global__ __launch_bounds__(256) void k_rice_dplan(DecodeArgs a) { prefix_dplan<RiceCode>(a); }
__global__ __launch_bounds__(256) void k_rice_sync(DecodeArgs a) { prefix_sync<RiceCode>(a); }
template <int ROUND> // counts into ri_ctl[ROUND]
__global__ __launch_bounds__(256) void k_rice_fix(DecodeArgs a)
{
	prefix_fix<RiceCode>(a, ROUND);
}
__global__ __launch_bounds__(256) void k_rice_check(DecodeArgs a) { prefix_check<RiceCode>(a); }
__global__ __launch_bounds__(64) void k_rice_dscan(DecodeArgs a) { prefix_dscan(a); }
__global__ __launch_bounds__(256) void k_rice_emit(DecodeArgs a) { prefix_emit<RiceCode>(a); }
__global__ __launch_bounds__(64) void k_rice_walk(DecodeArgs a) { prefix_walk<RiceCode>(a); }

// ------------------------------------------------------------------ launchers

// behind k_low_encode_chunked<false>; need != NULL: the sizes alone
void launch_rice_encode(const BatchArgs &a, uint64_t *need, hipStream_t s)
{
	const uint32_t grid = (uint32_t) (((uint64_t) a.max_chunks * PFX_UPC + 3) / 4);
	ex_stage_sized();
	hipLaunchKernelGGL(k_rice_count, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_pick, dim3(a.nreads), dim3(64), 0, s, a, need);
	if (need)
		return;
	(void) hipMemsetAsync(a.ri_pay, 0, a.ri_pay_bytes, s);
	hipLaunchKernelGGL(k_rice_write, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_copy, dim3(grid), dim3(256), 0, s, a);
}

// the packed press's write half: behind launch_rice_encode(need != NULL) and k_ex_section; no count, no pick
void launch_rice_write_sized(const BatchArgs &a, hipStream_t s)
{
	const uint32_t grid = (uint32_t) (((uint64_t) a.max_chunks * PFX_UPC + 3) / 4);
	hipLaunchKernelGGL(k_rice_place, dim3((a.nreads + 255) / 256), dim3(256), 0, s, a);
	(void) hipMemsetAsync(a.ri_pay, 0, a.ri_pay_bytes, s);
	hipLaunchKernelGGL(k_rice_write, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_copy, dim3(grid), dim3(256), 0, s, a);
}

// behind k_ex_parse: the payloads -> a.low
void launch_rice_decode(const DecodeArgs &a, hipStream_t s)
{
	(void) hipMemsetAsync(a.ri_ctl, 0, PFX_CTL_WORDS * 4, s);
	hipLaunchKernelGGL(k_rice_dplan, dim3((a.nreads + 255) / 256), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_sync, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_fix<1>, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_fix<2>, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_check, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_dscan, dim3(a.nreads), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_rice_emit, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_rice_walk, dim3(a.nreads), dim3(64), 0, s, a);
}

} // namespace ph
