// press_stall.hip - the stall methods rccm_svbbe21_zd, dstall_fz_1500 and dstall_fz (press.c:7716-8148;
// include/press_hip.h, press_hip_stall_*).  A stream is
//
//   [exists u8]  exists: [stall_start u16][stall_len u16][nstall u16][stall piece]   always: [nrest u32][rest piece]
//
// rest piece: rccm_vbbe21_zd of the read without the samples [stall_start, stall_start + stall_len); stall piece:
// rccm_vbbe21_submin of those samples as uint16: [min u16][vbbe21 section of x - min][the one-byte values, range coded].
//
// Nothing here codes a byte.  A read becomes up to three PIECES - rest, stall, and for dstall_fz the whole read -
// and launch_ex_encode_chunked / launch_ex_decode_chunked press and depress them as the reads of a larger batch:
//
//   press    launch_segments_first   segs[0] of jnn_raw per read (press_segments.hip)
//            k_stall_plan            one wave: truncation to 16 bits, threshold, +20 / -40; the piece table by a scan
//            k_stall_gather          one wave per piece: the samples of the piece
//            (the inner press)
//            k_stall_assemble        one wave per read: the form, the header, the pieces' streams into the slot
//   sizes    ... the inner press, then k_stall_sizes: the form's length per read, nothing of the caller's written
//   packed   ... k_stall_sizes, the layout scan (press_packed.hip), k_stall_assemble<PACKED> against the laid-out offsets
//   depress  k_stall_parse           one wave: every header checked before a byte of a piece is read; the piece table
//            (the inner depress)
//            k_stall_scatter         one wave per read: the two spans of the rest and the stall into place
//
// The stall piece goes through the SAME kernels as the rest.  submin's stream is the layout of a zig-zag-delta stream
// of stall_len + 1 samples whose zd[0] is min and whose zd[1 + i] is x[i] - min: a u16 in front, then vbbe21 over
// everything behind it.  So k_stall_gather writes the samples v that HAVE those zig-zag deltas,
//   v[0] = unzz(min), v[1 + i] = v[i] + unzz(x[i] - min)   (mod 2^16: a wave scan),
// and k_stall_scatter takes them apart again, x[i] = zz(v[1 + i] - v[i]) + zz(v[0]).  zz and unzz are bijections of the
// 16-bit values, so this is exact, and the transform kernels need no second form.

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

namespace {

constexpr uint64_t SFAIL64 = ~0ull;
constexpr uint32_t SFAIL32 = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t zz16(uint32_t d) // trans.c:75 on 16 bits
{
	const int32_t s = (int32_t) (int16_t) d;
	return (uint32_t) ((s << 1) ^ (s >> 15)) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t unzz16(uint32_t z) { return ((z >> 1) ^ (0u - (z & 1u))) & 0xFFFFu; }

__device__ __forceinline__ uint64_t up8(uint64_t n) { return (n + 7) & ~7ull; }
// Bytes certain to hold the stream of a piece of np samples: 2 + the section (4 + 8 + 2 + 6 bytes an exception at most:
// 32-bit position deltas, 16-bit values) + a byte per other sample + what the coder adds to a stream it stores raw
__device__ __forceinline__ uint64_t piece_cap(uint64_t np) { return np ? (6 * np + 64 + 15) & ~15ull : 0ull; }

// dst[0, nb) = src[0, nb) by the lanes of a wave: the bytes in front of dst's first 16-byte boundary, 16-byte stores
// fed by loads at whatever address the source has, the last bytes
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, uint64_t nb, uint32_t lane)
{
	uint64_t head = (16 - ((uintptr_t) dst & 15)) & 15;
	if (head > nb)
		head = nb;
	if (lane < head)
		dst[lane] = src[lane];
	dst += head;
	src += head;
	nb -= head;
	const uint64_t n16 = nb / 16;
#pragma unroll 4
	for (uint64_t c = lane; c < n16; c += 64) {
		uint4 v;
		__builtin_memcpy(&v, src + 16 * c, 16);
		*reinterpret_cast<uint4 *>(dst + 16 * c) = v;
	}
	const uint64_t done = 16 * n16;
	if (lane < nb - done)
		dst[done + lane] = src[done + lane];
}

__device__ __forceinline__ void wave_copy16(int16_t *dst, const int16_t *src, uint64_t count, uint32_t lane)
{
	wave_copy(reinterpret_cast<uint8_t *>(dst), reinterpret_cast<const uint8_t *>(src), 2 * count, lane);
}

__device__ __forceinline__ uint32_t ld16u(const uint8_t *p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8); }
__device__ __forceinline__ uint32_t ld32u(const uint8_t *p)
{
	return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}
__device__ __forceinline__ void st16u(uint8_t *p, uint32_t v)
{
	p[0] = (uint8_t) v;
	p[1] = (uint8_t) (v >> 8);
}
__device__ __forceinline__ void st32u(uint8_t *p, uint32_t v)
{
	st16u(p, v);
	st16u(p + 2, v >> 16);
}

} // namespace

// ------------------------------------------------------------------ press

// One wave, 64 reads a round.  find_stall and the head of X_press_16 (press.c:7728-7773): stall_start = (u16) x,
// stall_len = (u16) (y - x + 1), no stall below the threshold, else start += 20 (16 bits) and len -= 40.  A read without
// a segment has no stall (the reference compares an uninitialised length there).
__global__ __launch_bounds__(64) void k_stall_plan(int method, const uint32_t *nsamp, uint32_t nreads, StallBufs b)
{
	const uint32_t lane = threadIdx.x;
	const uint32_t T = method == PRESS_STALL_1500 ? 1500u : 140u;
	uint64_t sbase = 0, obase = 0;
	for (uint64_t r0 = 0; r0 < nreads; r0 += 64) {
		const uint64_t r = r0 + lane;
		const bool act = r < nreads;
		const uint32_t n = act ? nsamp[r] : 0u;
		uint32_t ss = 0, sl = 0, ex = 0;
		if (act && n) {
			const uint2 sg = b.seg[r];
			if (sg.x != STALL_NOSEG) {
				const uint32_t s16 = sg.x & 0xFFFFu, l16 = (sg.y - sg.x + 1u) & 0xFFFFu;
				if (l16 >= T) {
					ex = 1;
					ss = (s16 + 20u) & 0xFFFFu;
					sl = l16 - 40u;
				}
			}
			// (the truncated start lies at or in front of the real one, the truncated length is no longer than
			// the real one: the stall lies inside the read - held to here all the same)
			if (ex && (uint64_t) ss + sl > n)
				ex = ss = sl = 0;
		}
		uint32_t np[STALL_PIECES] = { n - sl, ex ? sl + 1u : 0u, (ex && method == PRESS_STALL_FZ) ? n : 0u };
		uint64_t sa[STALL_PIECES], oa[STALL_PIECES], ssum = 0, osum = 0;
#pragma unroll
		for (uint32_t k = 0; k < STALL_PIECES; k++) {
			sa[k] = ssum;
			oa[k] = osum;
			ssum += up8(np[k]);
			osum += piece_cap(np[k]);
		}
		const uint64_t sinc = wave_incl_scan64(ssum, lane), oinc = wave_incl_scan64(osum, lane);
		const uint64_t s0 = sbase + sinc - ssum, o0 = obase + oinc - osum;
		// what the host sized the scratch for holds every batch whose reads lie inside total_samples; a read beyond
		// that is refused, not written
		const bool fits = s0 + ssum <= b.sig_cap && o0 + osum <= b.arena_cap;
		if (act) {
#pragma unroll
			for (uint32_t k = 0; k < STALL_PIECES; k++) {
				const uint64_t p = STALL_PIECES * r + k;
				b.poff[p] = s0 + sa[k];
				b.pooff[p] = o0 + oa[k];
				b.pn[p] = fits ? np[k] : 0u;
			}
			b.rd[r] = { ss, sl, ex, fits ? 1u : 0u };
		}
		sbase += __shfl(sinc, 63, 64);
		obase += __shfl(oinc, 63, 64);
	}
	if (lane == 0) {
		b.poff[(uint64_t) STALL_PIECES * nreads] = sbase;
		b.pooff[(uint64_t) STALL_PIECES * nreads] = obase;
	}
}

// One wave per piece.  Rest: the two spans of the read joined at stall_start, an arbitrary sample; whole: the read;
// stall: the samples whose zig-zag deltas are min, x[0] - min, x[1] - min ... (the file's head)
__global__ __launch_bounds__(64) void k_stall_gather(const int16_t *sig, const uint64_t *off, const uint32_t *nsamp, StallBufs b)
{
	const uint32_t p = blockIdx.x, lane = threadIdx.x;
	const uint32_t r = p / STALL_PIECES, k = p % STALL_PIECES;
	const uint32_t np = uni(b.pn[p]);
	if (np == 0)
		return;
	const uint32_t n = uni(nsamp[r]);
	const uint32_t ss = uni(b.rd[r].start), sl = uni(b.rd[r].len);
	const int16_t *src = sig + uni64(off[r]);
	int16_t *dst = b.psig + uni64(b.poff[p]);
	if (k == 0) {
		wave_copy16(dst, src, ss, lane);
		wave_copy16(dst + ss, src + ss + sl, (uint64_t) n - ss - sl, lane);
		return;
	}
	if (k == 2) {
		wave_copy16(dst, src, n, lane);
		return;
	}
	const int16_t *x = src + ss;
	uint32_t mn = 0xFFFFu; // get_min_u16
	for (uint32_t i = lane; i < sl; i += 64)
		mn = min(mn, (uint32_t) (uint16_t) x[i]);
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		mn = min(mn, (uint32_t) __shfl_xor((int) mn, d, 64));
	mn = uni(mn);
	// v[j] for j = 0 .. sl, 512 a round, 8 a lane; dst has room for up8(sl + 1) samples: every store is whole
	uint32_t carry = 0;
	for (uint32_t j0 = 0; j0 < np; j0 += 512) {
		const uint32_t j = j0 + lane * 8;
		uint32_t v[8], run = 0;
#pragma unroll
		for (uint32_t h = 0; h < 8; h++) {
			const uint32_t jj = j + h;
			uint32_t d = 0;
			if (jj == 0)
				d = unzz16(mn);
			else if (jj < np)
				d = unzz16(((uint32_t) (uint16_t) x[jj - 1] - mn) & 0xFFFFu);
			run = (run + d) & 0xFFFFu;
			v[h] = run;
		}
		uint32_t inc = run;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t o = (uint32_t) __shfl_up((int) inc, d, 64);
			if (lane >= (uint32_t) d)
				inc += o;
		}
		const uint32_t base = carry + inc - run;
		if (j < np) {
			uint4 w;
			w.x = ((base + v[0]) & 0xFFFFu) | ((base + v[1]) << 16);
			w.y = ((base + v[2]) & 0xFFFFu) | ((base + v[3]) << 16);
			w.z = ((base + v[4]) & 0xFFFFu) | ((base + v[5]) << 16);
			w.w = ((base + v[6]) & 0xFFFFu) | ((base + v[7]) << 16);
			*reinterpret_cast<uint4 *>(dst + j) = w;
		}
		carry = (carry + (uint32_t) __shfl((int) inc, 63, 64)) & 0xFFFFu;
	}
}

// The form of a read's stream, the one definition of it (k_stall_sizes and k_stall_assemble).  Form 1: the stall stream;
// form 0: [0][u32][a bare stream] of piece `bare`.  dstall_fz keeps the stall form only where the WHOLE stall stream is
// strictly shorter than the bare rccm_vbbe21_zd stream of the read (press.c:8006).  A stall piece beyond 65535 bytes (the
// u16 count): the read is refused, dstall_fz takes the other form.  L0, L1, L2: polen[] of the read's three pieces.
struct StallForm {
	bool fail, form1;
	uint32_t bare;
	uint64_t len; // of the stream; form 0: 5 + the bare piece's
};
__device__ __forceinline__ StallForm stall_form(int method, uint32_t n, uint32_t ex, uint32_t ok, uint64_t L0, uint64_t L1, uint64_t L2)
{
	StallForm f;
	f.form1 = ex && L0 != SFAIL64 && L0 <= 0xFFFFFFFFull && L1 != SFAIL64 && L1 <= 65535;
	const uint64_t len1 = 11 + L1 + L0;
	f.bare = 0;
	f.fail = !ok || n == 0;
	if (ex && method == PRESS_STALL_FZ) {
		f.bare = 2;
		if (f.form1 && L2 != SFAIL64 && !(len1 < L2))
			f.form1 = false;
	} else if (ex && !f.form1) {
		f.fail = true;
	}
	const uint64_t Lb = f.bare ? L2 : L0;
	if (!f.form1 && (Lb == SFAIL64 || Lb > 0xFFFFFFFFull))
		f.fail = true;
	f.len = f.form1 ? len1 : 5 + Lb;
	return f;
}

// Grid-stride, 64 reads a wave round: need[r] = the exact length of the read's stream, SFAIL64 for a refused read
__global__ __launch_bounds__(64) void k_stall_sizes(int method, const uint32_t *nsamp, uint32_t nreads, StallBufs b, uint64_t *need)
{
	for (uint64_t r = (uint64_t) blockIdx.x * 64 + threadIdx.x; r < nreads; r += (uint64_t) gridDim.x * 64) {
		const uint64_t p0 = (uint64_t) STALL_PIECES * r;
		const StallRead rd = b.rd[r];
		const StallForm f = stall_form(method, nsamp[r], rd.exists, rd.ok, b.polen[p0], b.polen[p0 + 1], b.polen[p0 + 2]);
		need[r] = f.fail ? SFAIL64 : f.len;
	}
}

// One wave per read: the form, its length against the room, then the bytes.  The room is the caller's slot
// [out_off[r], out_off[r + 1]), or - PACKED, the laid-out arena of press_hip_press_packed, where neither an aligned next
// offset nor the last read's end says how far a stream may go - what lies between out_off[r] and out_cap.
template <bool PACKED>
__global__ __launch_bounds__(64) void k_stall_assemble(int method, const uint32_t *nsamp, StallBufs b, uint8_t *out, const uint64_t *out_off,
							uint64_t *out_len, uint32_t *stall, uint64_t out_cap)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const uint64_t p0 = (uint64_t) STALL_PIECES * r;
	const StallRead rd = b.rd[r];
	const uint32_t ss = uni(rd.start), sl = uni(rd.len), ex = uni(rd.exists), ok = uni(rd.ok);
	const uint64_t L0 = uni64(b.polen[p0]), L1 = uni64(b.polen[p0 + 1]), L2 = uni64(b.polen[p0 + 2]);
	const uint64_t base = uni64(out_off[r]);
	const uint64_t cap = PACKED ? (base < out_cap ? out_cap - base : 0ull) : uni64(out_off[r + 1]) - base;
	uint8_t *o = out + base;
	const StallForm f = stall_form(method, uni(nsamp[r]), ex, ok, L0, L1, L2);
	const bool form1 = f.form1, fail = f.fail || f.len > cap;
	const uint32_t bare = f.bare;
	const uint64_t Lb = bare ? L2 : L0;
	if (lane == 0) {
		out_len[r] = fail ? SFAIL64 : f.len;
		if (stall) {
			stall[2 * (uint64_t) r] = (!fail && form1) ? ss : 0u;
			stall[2 * (uint64_t) r + 1] = (!fail && form1) ? sl : 0u;
		}
	}
	if (fail)
		return;
	if (form1) {
		if (lane == 0) {
			o[0] = 1;
			st16u(o + 1, ss);
			st16u(o + 3, sl);
			st16u(o + 5, (uint32_t) L1);
			st32u(o + 7 + L1, (uint32_t) L0);
		}
		wave_copy(o + 7, b.parena + uni64(b.pooff[p0 + 1]), L1, lane);
		wave_copy(o + 11 + L1, b.parena + uni64(b.pooff[p0]), L0, lane);
	} else {
		if (lane == 0) {
			o[0] = 0;
			st32u(o + 1, (uint32_t) Lb);
		}
		wave_copy(o + 5, b.parena + uni64(b.pooff[p0 + bare]), Lb, lane);
	}
}

// ------------------------------------------------------------------ depress

// One wave, 64 reads a round: the header of every stream against in_len and the room before anything of a piece is
// touched (exists 0 or 1, stall inside the read, both counts inside the stream); a read that fails gets pieces of no
// samples, which the inner decoder refuses without reading them.
__global__ __launch_bounds__(64) void k_stall_parse(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, const uint32_t *nsamp,
						     uint32_t nreads, StallBufs b)
{
	const uint32_t lane = threadIdx.x;
	uint64_t sbase = 0;
	for (uint64_t r0 = 0; r0 < nreads; r0 += 64) {
		const uint64_t r = r0 + lane;
		const bool act = r < nreads;
		uint32_t n = 0, ss = 0, sl = 0, ex = 0;
		uint64_t at0 = 0, l0 = 0, at1 = 0, l1 = 0;
		bool ok = false;
		if (act) {
			n = nsamp[r];
			const uint64_t base = in_off[r], len = in_len[r];
			const uint8_t *h = in + base;
			if (n && len >= 5 && len != SFAIL64 && h[0] <= 1) { // (a press call's PRESS_HIP_FAILED is no length)
				ex = h[0];
				uint64_t pos = 1;
				ok = true;
				if (ex) {
					ok = len >= 11;
					if (ok) {
						ss = ld16u(h + 1);
						sl = ld16u(h + 3);
						l1 = ld16u(h + 5);
						at1 = base + 7;
						pos = 7 + l1;
						ok = (uint64_t) ss + sl <= n && pos + 4 <= len;
					}
				}
				if (ok) {
					l0 = ld32u(h + pos);
					at0 = base + pos + 4;
					ok = pos + 4 + l0 <= len;
				}
			}
			if (!ok)
				ss = sl = ex = 0;
		}
		const uint32_t np0 = ok ? n - sl : 0u, np1 = ok && ex ? sl + 1u : 0u;
		const uint64_t ssum = up8(np0) + up8(np1);
		const uint64_t sinc = wave_incl_scan64(ssum, lane);
		const uint64_t s0 = sbase + sinc - ssum;
		const bool fits = s0 + ssum <= b.sig_cap;
		if (act) {
			const uint64_t p = STALL_DPIECES * r;
			b.poff[p] = s0;
			b.poff[p + 1] = s0 + up8(np0);
			b.pn[p] = fits ? np0 : 0u;
			b.pn[p + 1] = fits ? np1 : 0u;
			b.pooff[p] = ok ? at0 : 0ull;
			b.pooff[p + 1] = ok ? at1 : 0ull;
			b.polen[p] = ok ? l0 : 0ull;
			b.polen[p + 1] = ok && ex ? l1 : 0ull;
			b.rd[r] = { ss, sl, ex, ok && fits ? 1u : 0u };
		}
		sbase += __shfl(sinc, 63, 64);
	}
	if (lane == 0)
		b.poff[(uint64_t) STALL_DPIECES * nreads] = sbase;
}

// One wave per read, behind the inner decoder: a read stands if its header did and the decoder gave both pieces back at
// their full counts; then out[0, start) and out[start + len, n) from the rest, out[start + i] = x[i] from the stall
// piece's samples (the file's head).  A refused read's room is not written.
__global__ __launch_bounds__(64) void k_stall_scatter(int16_t *sig, const uint64_t *off, const uint32_t *nsamp, StallBufs b, uint32_t *out_n)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const uint64_t p0 = (uint64_t) STALL_DPIECES * r;
	const StallRead rd = b.rd[r];
	const uint32_t ss = uni(rd.start), sl = uni(rd.len), ex = uni(rd.exists);
	const uint32_t n = uni(nsamp[r]);
	bool ok = uni(rd.ok) != 0;
	if (ok)
		ok = uni(b.poutn[p0]) == n - sl && (!ex || uni(b.poutn[p0 + 1]) == sl + 1u);
	if (lane == 0)
		out_n[r] = ok ? n : SFAIL32;
	if (!ok)
		return;
	int16_t *dst = sig + uni64(off[r]);
	const int16_t *rest = b.psig + uni64(b.poff[p0]);
	wave_copy16(dst, rest, ss, lane);
	wave_copy16(dst + ss + sl, rest + ss, (uint64_t) n - ss - sl, lane);
	if (!ex)
		return;
	const int16_t *v = b.psig + uni64(b.poff[p0 + 1]);
	const uint32_t mn = zz16((uint32_t) (uint16_t) v[0]);
	for (uint32_t i = lane; i < sl; i += 64) {
		const uint32_t d = ((uint32_t) (uint16_t) v[i + 1] - (uint32_t) (uint16_t) v[i]) & 0xFFFFu;
		dst[ss + i] = (int16_t) (uint16_t) (zz16(d) + mn);
	}
}

// ------------------------------------------------------------------ sizes and launchers

// Samples the pieces of a batch take at most, every piece rounded up to 8: rest + stall are the read and one sample
// (v[0]); dstall_fz adds the whole read of a read with a stall
uint64_t stall_piece_samples(int stall_method, uint64_t total_samples, uint32_t nreads, bool decode)
{
	const bool whole = !decode && stall_method == PRESS_STALL_FZ;
	return (whole ? 2 : 1) * total_samples + (uint64_t) nreads * (whole ? 32 : 24) + 64;
}

uint64_t stall_arena_bytes(uint64_t piece_samples, uint32_t npieces) { return 6 * piece_samples + (uint64_t) npieces * 80 + 64; }

void launch_stall_plan(int stall_method, const uint32_t *n, uint32_t nreads, const StallBufs &b, hipStream_t s)
{
	hipLaunchKernelGGL(k_stall_plan, dim3(1), dim3(64), 0, s, stall_method, n, nreads, b);
}

void launch_stall_gather(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const StallBufs &b, hipStream_t s)
{
	hipLaunchKernelGGL(k_stall_gather, dim3(STALL_PIECES * nreads), dim3(64), 0, s, sig, off, n, b);
}

void launch_stall_assemble(int stall_method, const uint32_t *n, uint32_t nreads, const StallBufs &b, uint8_t *out, const uint64_t *out_off,
			   uint64_t *out_len, uint32_t *stall, hipStream_t s)
{
	hipLaunchKernelGGL(k_stall_assemble<false>, dim3(nreads), dim3(64), 0, s, stall_method, n, b, out, out_off, out_len, stall, 0ull);
}

void launch_stall_sizes(int stall_method, const uint32_t *n, uint32_t nreads, const StallBufs &b, uint64_t *need, hipStream_t s)
{
	const uint32_t rounds = (nreads + 63) / 64;
	hipLaunchKernelGGL(k_stall_sizes, dim3(rounds < 256u ? rounds : 256u), dim3(64), 0, s, stall_method, n, nreads, b, need);
}

void launch_stall_assemble_packed(int stall_method, const uint32_t *n, uint32_t nreads, const StallBufs &b, uint8_t *out, const uint64_t *slot,
				  uint64_t out_cap, uint64_t *out_len, hipStream_t s)
{
	hipLaunchKernelGGL(k_stall_assemble<true>, dim3(nreads), dim3(64), 0, s, stall_method, n, b, out, slot, out_len, (uint32_t *) nullptr, out_cap);
}

void launch_stall_parse(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, const uint32_t *n, uint32_t nreads,
			const StallBufs &b, hipStream_t s)
{
	hipLaunchKernelGGL(k_stall_parse, dim3(1), dim3(64), 0, s, in, in_off, in_len, n, nreads, b);
}

void launch_stall_scatter(int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const StallBufs &b, uint32_t *out_n,
			  hipStream_t s)
{
	hipLaunchKernelGGL(k_stall_scatter, dim3(nreads), dim3(64), 0, s, sig, off, n, b, out_n);
}

} // namespace ph
