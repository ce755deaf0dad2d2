// press_cdf.hip - entropy stage 5 of the exception-split methods: TurboRC's adaptive nibble-CDF range coder
// (rccdfenc / rccdfdec, rccdf.c:178-202, as the reference's rccdf_*_zd methods call it), and k_rcf_raw, which tells a
// stored payload from a coded one for every coder of the range-coder family.
//
// Coder (restated from its behaviour; the variant WITHOUT __AVX2__ - TurboRC's own makefile leaves AVX2 off -: 64-bit
// range, 15-bit CDFs, 32-bit little-endian output words; pinned by tests/_rcf.py and tests/golden/ref_rcf.json):
//   state   range = 2^64 - 1, low = 0; 17 tables m[0..16] of uint16 (one for the high nibble, one for the low nibble
//           after each high nibble), m[j] = j << 11, m[16] = 32768 fixed;
//   nibble s, table m:
//           range >>= 15; low += range * m[s]; range *= m[s + 1] - m[s]; a carry out of low increments the words already
//           written; range < 2^32: emit the top word of low, shift both by 32 (once);
//           m[i] += (mix - m[i]) >> 7 (arithmetic), mix = i for i <= s, else i + 32752, i = 0 .. 15;
//   byte x  nibble x >> 4 with the first table, nibble x & 15 with table 1 + (x >> 4);
//   end     renormalise; range > 2^33 ? (low += 2^32, one word) : (low += 1, two words);
//   give-up (rcutil_.h:161) once the output reaches n*255/256 - 8 bytes the input is stored raw;
//   decode  code = the first two words; per nibble range >>= 15, s = the first i with m[i + 1] * range > code (15 if
//           none), code -= m[s] * range, range = (m[s + 1] - m[s]) * range, renormalise, the same update.
//
// ONE READ PER GROUP OF 16 LANES, four reads per wave: lane i of a group owns column i of the group's tables in LDS
// (544 bytes per read), so the update is one read-modify-write per lane and the decoder's symbol search is 16 products
// compared at once and a ballot cut to the group's 16 bits.  Range and low / code are computed by all 16 lanes alike.
// The two tables of a byte are different ones, so the encoder fetches both nibbles' entries together: one LDS round
// trip per byte on its chain, two (one per nibble) on the decoder's.  Groups are persistent and draw their next read
// from a ticket, each on its own - a group that finishes early does not wait for the other three of its wave.
// Carries walk back over the group's own stores (lane 0 of the group wrote them), as the coders of press_rc.hip do and
// with their code.  This coder carries about once in 30 to 35 bytes of signal data, each time a global read-modify-write;
// holding the last word and a run count of 0xFFFFFFFF words back in registers would keep memory off that path - not
// built, not measured.

#include "press_internal.h"

namespace ph {

namespace {

constexpr uint64_t CDF_TOP = 1ull << 32;
constexpr uint32_t CDF_GROUPS = 4;       // reads per wave
constexpr uint32_t CDF_MAX_BLOCKS = 8192; // persistent waves: what the chip holds at once

struct CdfOut {
	uint8_t *out;
	uint64_t cap;  // bytes the stream may take
	uint64_t pos;  // bytes written
	bool failed;   // the slot is too small (lane 0 of the group knows)
};

__device__ __forceinline__ void cdf_put32(CdfOut &o, uint32_t w)
{
	if (o.pos + 4 > o.cap) {
		o.failed = true;
	} else {
		__builtin_memcpy(o.out + o.pos, &w, 4);
	}
	o.pos += 4;
}

__device__ __forceinline__ void cdf_carry(CdfOut &o)
{
	uint64_t q = o.pos;
	while (q >= 4 && !o.failed) {
		q -= 4;
		uint32_t w;
		__builtin_memcpy(&w, o.out + q, 4);
		w += 1;
		__builtin_memcpy(o.out + q, &w, 4);
		if (w)
			break;
	}
}

__device__ __forceinline__ void cdf_init(uint16_t (*T)[16], uint32_t gl)
{
	for (int t = 0; t < 17; t++)
		T[t][gl] = (uint16_t) (gl << 11);
}

// column i of a table after symbol s
__device__ __forceinline__ uint16_t cdf_step(uint32_t v, uint32_t i, uint32_t s)
{
	const int32_t mix = (int32_t) (i <= s ? i : i + 32752u);
	return (uint16_t) ((int32_t) v + ((mix - (int32_t) v) >> 7));
}

} // namespace

// the one-byte values of read r are a.low_tmp[off[r] ..) (k_low_encode_chunked); the payload goes behind the section
__global__ __launch_bounds__(64) void k_cdf_encode(BatchArgs a)
{
	__shared__ uint16_t tab[CDF_GROUPS][17][16];
	const uint32_t lane = threadIdx.x, gbase = lane & 48u, gl = lane & 15u;
	uint16_t (*T)[16] = tab[lane >> 4];
	bool have = false, done = false, raw = false;
	uint32_t r = 0, head = 0, cur = 0, nxt = 0;
	uint64_t n = 0, i = 0, low = 0, range = 0;
	long long giveup = 0;
	const uint8_t *in = nullptr;
	CdfOut o = { nullptr, 0, 0, false };
	for (;;) {
		if (!have && !done) {
			uint32_t t = 0;
			if (gl == 0)
				t = atomicAdd(&a.ctl->ticket2, 1u);
			t = (uint32_t) __shfl((int) t, (int) gbase, 64);
			if (t >= a.nreads) {
				done = true;
			} else if (a.meta[t].status == 0) { // (else out_len = FAILED was written by k_ex_section)
				const ReadMeta *m = a.meta + t;
				r = t;
				n = m->nlow;
				head = m->hdr + m->seclen;
				in = a.low_tmp + a.off[r];
				o.out = a.out + a.out_off[r] + head;
				o.cap = a.out_off[r + 1] - a.out_off[r] - head;
				o.pos = 0;
				o.failed = false;
				low = 0;
				range = ~0ull;
				giveup = (long long) (n * 255 / 256) - 8;
				raw = false;
				i = 0;
				nxt = gl < n ? in[gl] : 0u; // 16 input bytes, one per lane, one fetch ahead
				cdf_init(T, gl);
				have = true;
			}
		}
		if (__all(done))
			break;
		if (!have)
			continue;
		if (i < n && !raw) {
			if ((i & 15) == 0) {
				cur = nxt;
				nxt = i + 16 + gl < n ? in[i + 16 + gl] : 0u;
			}
			const uint32_t x = (uint32_t) __shfl((int) cur, (int) (gbase | ((uint32_t) i & 15u)), 64);
			const uint32_t h = x >> 4, l = x & 15u;
			uint16_t *th = T[0], *tl = T[1 + h];
			// everything the byte needs of its two tables in one round trip
			const uint32_t ch = th[gl], cl = tl[gl];
			const uint32_t h0 = th[h], h1 = h == 15 ? 32768u : th[(h + 1) & 15u];
			const uint32_t l0 = tl[l], l1 = l == 15 ? 32768u : tl[(l + 1) & 15u];
			th[gl] = cdf_step(ch, gl, h);
			tl[gl] = cdf_step(cl, gl, l);
#pragma unroll
			for (int k = 0; k < 2; k++) {
				const uint32_t m0 = k ? l0 : h0, m1 = k ? l1 : h1;
				const uint64_t before = low;
				range >>= 15;
				low += range * m0;
				range *= (uint64_t) (m1 - m0);
				if (before > low && gl == 0)
					cdf_carry(o);
				if (range < CDF_TOP) {
					if (gl == 0)
						cdf_put32(o, (uint32_t) (low >> 32));
					else
						o.pos += 4;
					range <<= 32;
					low <<= 32;
				}
			}
			i++;
			if ((long long) o.pos >= giveup)
				raw = true; // rcutil_.h:161: stored instead
			__builtin_amdgcn_wave_barrier(); // (the columns the other lanes wrote are read by the next byte: DS operations of one wave, in order)
			continue;
		}
		// the read's end
		if (raw) {
			const bool fail = n > o.cap;
			if (!fail)
				for (uint64_t k = gl; k < n; k += 16)
					o.out[k] = in[k];
			if (gl == 0)
				a.out_len[r] = fail ? ~0ull : (uint64_t) head + n;
		} else if (gl == 0) {
			if (range < CDF_TOP) {
				range <<= 32;
				cdf_put32(o, (uint32_t) (low >> 32));
				low <<= 32;
			}
			const uint64_t before = low;
			if (range > (1ull << 33)) {
				low += 1ull << 32;
				if (before > low)
					cdf_carry(o);
				cdf_put32(o, (uint32_t) (low >> 32));
			} else {
				low += 1;
				if (before > low)
					cdf_carry(o);
				cdf_put32(o, (uint32_t) (low >> 32));
				cdf_put32(o, (uint32_t) low);
			}
			a.out_len[r] = o.failed ? ~0ull : (uint64_t) head + o.pos;
		}
		have = false;
	}
}

// the payload behind the exception section -> a.low[off[r] ..)
__global__ __launch_bounds__(64) void k_cdf_decode(DecodeArgs a)
{
	__shared__ uint16_t tab[CDF_GROUPS][17][16];
	const uint32_t lane = threadIdx.x, gbase = lane & 48u, gl = lane & 15u;
	uint16_t (*T)[16] = tab[lane >> 4];
	bool have = false, done = false;
	uint32_t wn = 0, acc = 0;
	uint64_t n = 0, i = 0, len = 0, pos = 0, range = 0, code = 0;
	const uint8_t *in = nullptr;
	uint8_t *out = nullptr;
	// bytes past the end of the stream read as zeros (the reference reads whatever follows)
	auto get32 = [&]() -> uint32_t {
		uint32_t w = 0;
		if (pos + 4 <= len) {
			__builtin_memcpy(&w, in + pos, 4);
		} else {
			for (int b = 0; b < 4; b++)
				if (pos + b < len)
					w |= (uint32_t) in[pos + b] << (8 * b);
		}
		pos += 4;
		return w;
	};
	// the next word is always in flight before it is needed
	auto next32 = [&]() -> uint32_t {
		const uint32_t w = wn;
		wn = get32();
		return w;
	};
	for (;;) {
		if (!have && !done) {
			uint32_t t = 0;
			if (gl == 0)
				t = atomicAdd(&a.ctl->ticket2, 1u);
			t = (uint32_t) __shfl((int) t, (int) gbase, 64);
			if (t >= a.nreads) {
				done = true;
			} else if (a.meta[t].status == 0) {
				const ReadMeta *m = a.meta + t;
				const uint32_t head = m->hdr + m->seclen;
				n = m->nlow;
				in = a.in + a.in_off[t] + head;
				len = a.in_len[t] - head;
				out = a.low + a.off[t];
				pos = 0;
				range = ~0ull;
				wn = get32();
				code = next32();
				code = (code << 32) | next32();
				i = 0;
				acc = 0;
				cdf_init(T, gl);
				have = n != 0;
			}
		}
		if (__all(done))
			break;
		if (!have)
			continue;
		uint32_t x = 0;
		uint16_t *row = T[0];
#pragma unroll
		for (int k = 0; k < 2; k++) {
			range >>= 15;
			const uint32_t c0 = row[gl], cn = row[(gl + 1) & 15u];
			const uint32_t c1 = gl == 15 ? 32768u : cn;
			const bool above = (uint64_t) c1 * range > code;
			const uint32_t mask = (uint32_t) (__ballot(above) >> gbase) & 0xFFFFu;
			const uint32_t s = mask ? (uint32_t) __builtin_ctz(mask) : 15u;
			// the two entries around the symbol, from the lane that holds them
			const uint32_t pair = (uint32_t) __shfl((int) (c0 | (c1 << 16)), (int) (gbase | s), 64);
			const uint64_t rp = (uint64_t) (pair & 0xFFFFu) * range;
			range = (uint64_t) (pair >> 16) * range - rp;
			code -= rp;
			if (range < CDF_TOP) {
				range <<= 32;
				code = (code << 32) | next32();
			}
			row[gl] = cdf_step(c0, gl, s);
			__builtin_amdgcn_wave_barrier(); // (DS operations of one wave: in order)
			x = (x << 4) | s;
			row = T[1 + s];
		}
		acc |= x << (8 * ((uint32_t) i & 3u));
		if (((uint32_t) i & 3u) == 3u || i + 1 == n) {
			if (gl == 0)
				for (uint32_t b = 0; b <= ((uint32_t) i & 3u); b++)
					out[(i & ~3ull) + b] = (uint8_t) (acc >> (8 * b));
			acc = 0;
		}
		if (++i == n)
			have = false;
	}
}

// One wave per read, behind the encoder of any coder of the family: raw[r] = 1 where the payload has the length of the
// read's one-byte values and equals them byte for byte - the coder gave up (rcutil_.h:161) and stored them -, else 0.
__global__ __launch_bounds__(64) void k_rcf_raw(BatchArgs a, uint8_t *raw)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const ReadMeta *m = a.meta + r;
	const uint64_t olen = a.out_len[r];
	bool same = false;
	if (m->status == 0 && olen != ~0ull) {
		const uint32_t head = m->hdr + m->seclen;
		const uint64_t n = m->nlow;
		if (olen == (uint64_t) head + n) {
			const uint8_t *p = a.out + a.out_off[r] + head, *q = a.low_tmp + a.off[r];
			bool diff = false;
			for (uint64_t k = lane; k < n; k += 64)
				diff |= p[k] != q[k];
			same = !__any(diff);
		}
	}
	if (lane == 0)
		raw[r] = same ? 1 : 0;
}

static uint32_t cdf_blocks(uint32_t nreads)
{
	const uint32_t b = (nreads + CDF_GROUPS - 1) / CDF_GROUPS;
	return b < CDF_MAX_BLOCKS ? b : CDF_MAX_BLOCKS;
}

void launch_cdf_encode(const BatchArgs &a, uint64_t *, hipStream_t s)
{
	(void) hipMemsetAsync(&a.ctl->ticket2, 0, 4, s);
	hipLaunchKernelGGL(k_cdf_encode, dim3(cdf_blocks(a.nreads)), dim3(64), 0, s, a);
}

void launch_cdf_decode(const DecodeArgs &a, hipStream_t s)
{
	(void) hipMemsetAsync(&a.ctl->ticket2, 0, 4, s);
	hipLaunchKernelGGL(k_cdf_decode, dim3(cdf_blocks(a.nreads)), dim3(64), 0, s, a);
}

void launch_rcf_raw(const BatchArgs &a, uint8_t *raw, hipStream_t s)
{
	if (a.nreads)
		hipLaunchKernelGGL(k_rcf_raw, dim3(a.nreads), dim3(64), 0, s, a, raw);
}

} // namespace ph
