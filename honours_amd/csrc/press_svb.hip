// press_svb.hip - the svb16 / svb32 kernels over the chunk machinery of press_chunk.h: the chunk table, the encoder, the
// key scan and the decoder with its FUSE / float / DEG variants, and the launchers of the svb methods and of recode.
//
// Formats: svb16/encode.hpp:11, encode_scalar.hpp:14, decode.hpp:23, decode_scalar.hpp:31;
// streamvbyte_encode.c:70, streamvbyte_decode.c:62; press.c:1573-1611, 1678-1694.

#include "press_chunk.h"

namespace ph {

// ------------------------------------------------------------------ chunk table

// One thread per read: a wave adds up its reads' chunk counts, takes a contiguous range of
// chunk ids with ONE atomic (ids need only be contiguous and ascending within a read),
// writes the descriptors and clears the look-back granules of its chunks.
// EXACT (the packed press of the svb kinds, press_hip_press_packed): slot_off is the layout the library made from the
// streams' own lengths need[], so a slot is not the format's worst case: the read is written iff it lies inside out_cap.
template <bool DEC, bool KEY2, bool EXACT = false>
__global__ __launch_bounds__(256) void k_chunk_prep(const uint64_t *off, const uint32_t *nsamp,
						    const uint64_t *slot_off, const uint64_t *in_len,
						    uint32_t nreads, ChunkDesc *chunks, uint64_t *gran,
						    ChunkCtl *ctl, uint32_t max_chunks, uint64_t *out_len,
						    uint32_t *out_n, uint32_t *first_chunk, ReadMeta *meta = nullptr,
						    const uint8_t *in = nullptr, uint32_t hdr = 0, uint8_t *out = nullptr,
						    const uint64_t *need = nullptr, uint64_t out_cap = 0)
{
	static_assert(!EXACT || !DEC, "the exact slots are press's");
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	uint32_t n = 0, nch = 0;
	if (r < nreads) {
		n = nsamp[r];
		nch = (n + CHUNK - 1) / CHUNK;
	}
	const uint32_t inc = scan32(nch, threadIdx.x & 63);
	uint32_t base = 0;
	if ((threadIdx.x & 63) == 63 && inc)
		base = atomicAdd(&ctl->nchunks, inc);
	base = (uint32_t) __builtin_amdgcn_readlane((int) base, 63);
	const uint32_t first = base + inc - nch;
	if (r >= nreads)
		return;
	if (meta) {
		ReadMeta z;
		z.nex = z.ored = z.zd0 = z.q = z.hdr = z.seclen = z.nlow = 0;
		z.status = 0;
		meta[r] = z;
	}
	const uint32_t klen = KEY2 ? (n + 3) / 4 : (n >> 3) + (((n & 7) + 7) >> 3);
	const uint64_t sbase = slot_off[r];
	// hdr = 4: the slow5 svb-zd stream (u32 sample count in front, values of up to 3 bytes)
	uint32_t ok;
	if (EXACT) {
		ok = need[r] <= out_cap && sbase <= out_cap - need[r];
	} else if (!DEC) {
		ok = (uint64_t) hdr + klen + (hdr ? 3ull : 2ull) * n <= slot_off[r + 1] - sbase;
	} else {
		ok = (uint64_t) hdr + klen <= in_len[r];
		if (ok && hdr) { // slow5_press.c:1086: the count in the stream is what gets decoded
			const uint8_t *h = in + sbase;
			ok = ((uint32_t) h[0] | ((uint32_t) h[1] << 8) | ((uint32_t) h[2] << 16) | ((uint32_t) h[3] << 24)) == n;
		}
	}
	// an empty read has no chunk: its verdict is given here.  With a header (slow5 svb-zd) the stream is the
	// count alone (slow5_press.c:1046), and a stream of any other length is refused (slow5_press.c:1098)
	if (n == 0) {
		if (!DEC) {
			if (hdr) {
				if (!EXACT)
					ok = hdr <= slot_off[r + 1] - sbase;
				for (uint32_t b = 0; ok && b < hdr; b++)
					out[sbase + b] = 0;
			}
			out_len[r] = ok ? hdr : CFAIL64;
		} else {
			out_n[r] = ok && (!hdr || in_len[r] == hdr) ? 0u : CFAIL32;
		}
	}
	const uint64_t o = off[r];
	if (first_chunk)
		first_chunk[r] = first;
	for (uint32_t j = 0; j < nch; j++) {
		if (first + j >= max_chunks)
			break; // cannot happen: max_chunks bounds the sum
		ChunkDesc d;
		d.sig_off = o;
		d.out_base = sbase;
		d.n = n;
		d.j = j;
		d.read = r;
		d.cap_ok = ok;
		d.ebefore = 0;
		d.ecnt[0] = d.ecnt[1] = d.ecnt[2] = d.ecnt[3] = 0;
		d.kmask[0] = d.kmask[1] = d.kmask[2] = d.kmask[3] = 0;
		chunks[first + j] = d;
		gran[first + j] = 0;
	}
}

void launch_chunk_prep(const BatchArgs &a, bool key2bit, uint32_t hdr, bool meta, const PackArgs *pk, hipStream_t s)
{
	const auto k = pk ? (key2bit ? k_chunk_prep<false, true, true> : k_chunk_prep<false, false, true>)
			  : (key2bit ? k_chunk_prep<false, true> : k_chunk_prep<false, false>);
	(void) hipMemsetAsync(a.ctl, 0, sizeof(ChunkCtl), s);
	hipLaunchKernelGGL(k, dim3((a.nreads + 255) / 256), dim3(256), 0, s, a.off, a.nsamp, pk ? pk->layout : a.out_off, nullptr, a.nreads,
			   a.chunks, a.gran, a.ctl, a.max_chunks, a.out_len, nullptr, a.first_chunk, meta ? a.meta : nullptr, nullptr, hdr, a.out,
			   pk ? pk->need : nullptr, pk ? pk->out_cap : 0);
}

void launch_chunk_prep(const DecodeArgs &a, bool key2bit, uint32_t hdr, hipStream_t s)
{
	(void) hipMemsetAsync(a.ctl, 0, sizeof(ChunkCtl), s);
	hipLaunchKernelGGL((key2bit ? k_chunk_prep<true, true> : k_chunk_prep<true, false>), dim3((a.nreads + 255) / 256), dim3(256), 0, s, a.off,
			   a.nsamp, a.in_off, a.in_len, a.nreads, a.chunks, a.gran, a.ctl, a.max_chunks, nullptr, a.out_n, a.first_chunk, nullptr,
			   a.in, hdr, nullptr, nullptr, 0);
}

// ------------------------------------------------------------------ encode

// S5 (with KEY2, ZD): slow5lib's "svb-zd" signal codec (slow5_press.c:1054): a u32 sample count
// in front, and the delta taken in 32 bits - a jump of more than 32767 is a 3-byte value.
// HIST (the zstd compositions, press_zstd.hip): the data bytes are counted per read (BatchArgs::zhist) while a lane
// holds them - the Huffman table of the read's frame needs their histogram, and a kernel of its own read the stream again
// for it (0.36 ms of config 3's press call).  16 copies of the counters in LDS (4 per wave, by lane): nanopore deltas
// are peaked, and lanes that hit one counter in one instruction are served one after the other.
template <bool KEY2, bool ZD, bool S5 = false, bool HIST = false>
__global__ __launch_bounds__(CWG) void k_svb_encode_chunked(BatchArgs a)
{
	static_assert(!S5 || (KEY2 && ZD), "the slow5 variant is svb32 of zig-zag deltas");
	static_assert(!HIST || !S5, "the histogram is for the two-byte formats");
	__shared__ uint32_t s_ticket;
	__shared__ uint32_t s_wtot[4];
	__shared__ uint64_t s_excl;
	__shared__ uint32_t s_hist[HIST ? 16 : 1][256];
	__shared__ uint32_t s_knz[4];
	uint32_t *myhist = s_hist[HIST ? 4 * (threadIdx.x >> 6) + (threadIdx.x & 3) : 0];
	if (HIST)
		for (int i = 0; i < 16; i++)
			s_hist[i][threadIdx.x] = 0; // (the ticket barrier orders this in front of every count)

	// persistent workgroups: chunks are handed out in ticket order (what makes the
	// look-back deadlock free).  (Fetching the next ticket early was measured slower.)
	const uint32_t nchunks = uni(a.ctl->nchunks);
	for (;;) {
	if (threadIdx.x == 0)
		s_ticket = atomicAdd(&a.ctl->ticket, 1u);
	__syncthreads();
	const uint32_t t = uni(s_ticket);
	if (t >= nchunks)
		break;
	const ChunkU d = load_chunk(a.chunks + t);
	const uint32_t n = d.n;
	const uint32_t first = d.j * CHUNK;          // first sample of the chunk within the read
	const bool last = first + CHUNK >= n;
	const int lane = threadIdx.x & 63;
	const int w = (int) uni(threadIdx.x >> 6);

	if (!d.cap_ok) { // slot smaller than the worst case of the format: fail the read
		if (threadIdx.x < 64) {
			(void) lookback(a.gran, t, d.j, 0, last);
			if (last && threadIdx.x == 0)
				a.out_len[d.read] = CFAIL64;
			if (HIST && last && threadIdx.x == 0)
				a.zkcnt[t - d.j] = 0;
		}
		__syncthreads(); // every wave has read s_ticket before thread 0 overwrites it
		continue;
	}

	const int16_t *in = a.sig + d.sig_off;
	uint8_t *out = a.out + d.out_base + (S5 ? 4 : 0);
	if (S5 && first == 0 && threadIdx.x == 0) { // slow5_press.c:1046: the sample count
		uint8_t *h = a.out + d.out_base;
		h[0] = (uint8_t) n;
		h[1] = (uint8_t) (n >> 8);
		h[2] = (uint8_t) (n >> 16);
		h[3] = (uint8_t) (n >> 24);
	}
	const uint32_t klen = KEY2 ? (n + 3) / 4 : (n >> 3) + (((n & 7) + 7) >> 3);
	const uint32_t ws = first + w * WAVE_SAMPLES; // first sample of this wave's quarter

	// ---- phase 1: load everything, zig-zag delta in registers, count exceptions
	uint4 z[CK];
#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		z[k] = make_uint4(0, 0, 0, 0);
		if (i0 < n)
			z[k] = ld16_stream(in + i0);
	}
	uint32_t carry = 0; // dword holding the sample in front of lane 0's first sample
	if (ZD && ws > 0 && ws < n)
		carry = (uint32_t) (uint16_t) in[ws - 1] << 16;

	uint32_t kmask = 0;  // sub-tiles that need the slow path (exceptions or a ragged tail)
	uint32_t omask = 0;  // S5: sub-tiles with a 17-bit value
	uint32_t etot = 0;   // exceptions in this wave's quarter (uniform)
	uint32_t knz1 = 0;   // HIST: key bytes of this wave's quarter that are not zero (uniform)
#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		const uint32_t raw_w = z[k].w;
		uint32_t ov[4] = { 0, 0, 0, 0 };
		if (ZD) {
			const uint32_t pw = prev_lane(raw_w, carry);
			uint32_t z0, z1, z2, z3;
			if (S5) {
				z0 = zd_pair_ovf(z[k].x, pw, ov[0]);
				z1 = zd_pair_ovf(z[k].y, z[k].x, ov[1]);
				z2 = zd_pair_ovf(z[k].z, z[k].y, ov[2]);
				z3 = zd_pair_ovf(z[k].w, z[k].z, ov[3]);
			} else {
				z0 = zd_pair(z[k].x, pw);
				z1 = zd_pair(z[k].y, z[k].x);
				z2 = zd_pair(z[k].z, z[k].y);
				z3 = zd_pair(z[k].w, z[k].z);
			}
			z[k] = make_uint4(z0, z1, z2, z3);
			carry = (uint32_t) __builtin_amdgcn_readlane((int) raw_w, 63);
		}
		// samples at or beyond n must not count: zero them
		if (i0 + 8 > n) {
			const uint32_t nv = i0 < n ? n - i0 : 0;
			uint32_t zz[4] = { z[k].x, z[k].y, z[k].z, z[k].w };
#pragma unroll
			for (int q = 0; q < 4; q++) {
				if (nv <= (uint32_t) (2 * q))
					zz[q] = 0;
				else if (nv == (uint32_t) (2 * q + 1))
					zz[q] &= 0xFFFFu;
			}
			z[k] = make_uint4(zz[0], zz[1], zz[2], zz[3]);
			if (S5) { // ... and their differences cannot overflow
#pragma unroll
				for (int q = 0; q < 4; q++) {
					if (nv <= (uint32_t) (2 * q))
						ov[q] = 0;
					else if (nv == (uint32_t) (2 * q + 1))
						ov[q] &= 0xFFFFu;
				}
			}
		}
		const uint32_t hi = (z[k].x | z[k].y | z[k].z | z[k].w) & 0xFF00FF00u;
		const bool ragged = i0 < n && i0 + 8 > n;
		const unsigned long long bo = S5 ? __ballot((ov[0] | ov[1] | ov[2] | ov[3]) != 0) : 0ull;
		const unsigned long long bx = __ballot(hi != 0) | bo;
		const unsigned long long br = __ballot(ragged);
		if (bx | br)
			kmask |= 1u << k;
		if (bo)
			omask |= 1u << k;
		if (bx) {
			if (HIST) { // key bytes that will not be zero: a lane's eight values are one (svb16) or two (svb32) of them
				if (KEY2)
					knz1 += (uint32_t) (__popcll(__ballot(((z[k].x | z[k].y) & 0xFF00FF00u) != 0)) +
							     __popcll(__ballot(((z[k].z | z[k].w) & 0xFF00FF00u) != 0)));
				else
					knz1 += (uint32_t) __popcll(__ballot(hi != 0));
			}
			// exact count of the extra bytes: one popcount of a ballot per key bit; a 17-bit
			// value has two of them whatever its low half looks like
			const uint32_t zz[4] = { z[k].x, z[k].y, z[k].z, z[k].w };
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const bool o0 = S5 && (ov[q] & 0x00008000u), o1 = S5 && (ov[q] & 0x80000000u);
				etot += (uint32_t) __popcll(__ballot(!o0 && (zz[q] & 0x0000FF00u) != 0));
				etot += (uint32_t) __popcll(__ballot(!o1 && (zz[q] & 0xFF000000u) != 0));
				if (S5 && bo)
					etot += 2u * (uint32_t) (__popcll(__ballot(o0)) + __popcll(__ballot(o1)));
			}
		}
	}

	// ---- exceptions before this wave: within the chunk (LDS) and before the chunk (look-back)
	if (lane == 0) {
		s_wtot[w] = etot;
		if (HIST)
			s_knz[w] = knz1;
	}
	__syncthreads();
	const uint32_t t0 = uni(s_wtot[0]), t1 = uni(s_wtot[1]), t2 = uni(s_wtot[2]), t3 = uni(s_wtot[3]);
	// HIST: the look-back carries two counts - exceptions below bit 40, key bytes that are not zero above (a read has
	// fewer than 2^32 of the first and 2^22 of the second)
	const uint32_t q0 = HIST ? uni(s_knz[0]) : 0u, q1 = HIST ? uni(s_knz[1]) : 0u, q2 = HIST ? uni(s_knz[2]) : 0u,
		       q3 = HIST ? uni(s_knz[3]) : 0u;
	if (w == 0) {
		const uint64_t e = lookback(a.gran, t, d.j, ((uint64_t) t0 + t1 + t2 + t3) | ((uint64_t) (q0 + q1 + q2 + q3) << 40), last);
		if (lane == 0)
			s_excl = e;
	}
	__syncthreads();
	const uint64_t ebefore = uni64(s_excl) & ((1ull << 40) - 1);
	uint32_t kbefore = (uint32_t) (uni64(s_excl) >> 40) + (w > 0 ? q0 : 0u) + (w > 1 ? q1 : 0u) + (w > 2 ? q2 : 0u); // list slot of the wave's next key byte
	uint64_t ebase = ebefore + (w > 0 ? t0 : 0u) + (w > 1 ? t1 : 0u) + (w > 2 ? t2 : 0u);
	if (last && threadIdx.x == 0)
		a.out_len[d.read] = (uint64_t) (S5 ? 4 : 0) + klen + n + ebefore + t0 + t1 + t2 + t3;

	// ---- phase 2: keys and data
	uint8_t *data = out + klen;

#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		if (ws + k * SUB >= n)
			continue; // uniform: nothing left in this wave's quarter
		const uint32_t zz[4] = { z[k].x, z[k].y, z[k].z, z[k].w };
		const uint32_t lo0 = __builtin_amdgcn_perm(zz[1], zz[0], 0x06040200);
		const uint32_t lo1 = __builtin_amdgcn_perm(zz[3], zz[2], 0x06040200);
		if (!((kmask >> k) & 1u)) {
			// fast path: no exception, no ragged tail in the whole sub-tile (lanes are
			// either complete or entirely beyond the end of the read)
			if (i0 < n) {
				if (!KEY2)
					out[i0 >> 3] = 0;
				else
					__builtin_memset(out + (i0 >> 2), 0, 2);
				uint2 v;
				v.x = lo0;
				v.y = lo1;
				__builtin_memcpy(data + ebase + i0, &v, 8);
				if (HIST) {
#pragma unroll
					for (int e = 0; e < 4; e++) {
						atomicAdd(&myhist[(lo0 >> (8 * e)) & 0xFFu], 1u);
						atomicAdd(&myhist[(lo1 >> (8 * e)) & 0xFFu], 1u);
					}
				}
			}
			continue;
		}
		// slow path
		uint32_t key = 0;
#pragma unroll
		for (int q = 0; q < 4; q++) {
			key |= ((zz[q] & 0x0000FF00u) ? 1u : 0u) << (2 * q);
			key |= ((zz[q] & 0xFF000000u) ? 1u : 0u) << (2 * q + 1);
		}
		const uint32_t nv = i0 < n ? min(8u, n - i0) : 0u;
		uint32_t wide = 0; // S5: which of the lane's values are 17 bits wide (from the samples again: rare)
		if (S5 && ((omask >> k) & 1u) && nv) {
			const uint4 raw = ld16_stream(in + i0);
			const uint32_t pv = i0 ? (uint32_t) (uint16_t) in[i0 - 1] << 16 : 0u;
			uint32_t ov[4] = { 0, 0, 0, 0 };
			(void) zd_pair_ovf(raw.x, pv, ov[0]);
			(void) zd_pair_ovf(raw.y, raw.x, ov[1]);
			(void) zd_pair_ovf(raw.z, raw.y, ov[2]);
			(void) zd_pair_ovf(raw.w, raw.z, ov[3]);
#pragma unroll
			for (int q = 0; q < 4; q++) {
				wide |= ((ov[q] >> 15) & 1u) << (2 * q);
				wide |= ((ov[q] >> 31) & 1u) << (2 * q + 1);
			}
			wide &= (1u << nv) - 1u;
			key &= ~wide;
		}
		// the lane's key byte(s)
		uint32_t k0 = key, k1 = 0;
		if (KEY2) {
			k0 = 0;
#pragma unroll
			for (int q = 0; q < 4; q++) {
				k0 |= (((key >> q) & 1u) | (((wide >> q) & 1u) << 1)) << (2 * q);
				k1 |= (((key >> (q + 4)) & 1u) | (((wide >> (q + 4)) & 1u) << 1)) << (2 * q);
			}
		}
		if (!nv)
			k0 = 0;
		if (nv <= 4)
			k1 = 0;
		const uint32_t cnt = __popc(key) + 2u * __popc(wide);
		const uint32_t kc = HIST ? (k0 != 0) + (k1 != 0) : 0u; // (one scan for both: a sub-tile has at most 1536 extra bytes)
		const uint32_t inc2 = scan32(cnt | (kc << 16), (uint32_t) lane);
		const uint32_t inc = inc2 & 0xFFFFu;
		const uint32_t tot2 = (uint32_t) __builtin_amdgcn_readlane((int) inc2, 63);
		const uint32_t tot = tot2 & 0xFFFFu;
		uint8_t *p = data + ebase + i0 + (inc - cnt);
		if (HIST && kc) { // the read's list of key bytes that are not zero (press_zstd.hip: RLE blocks between them)
			uint32_t slot = kbefore + (inc2 >> 16) - kc;
			const uint32_t kpos = KEY2 ? i0 >> 2 : i0 >> 3;
			if (k0) {
				a.ex_pos[d.sig_off + slot] = kpos;
				a.ex_val[d.sig_off + slot] = k0;
				slot++;
			}
			if (k1) {
				a.ex_pos[d.sig_off + slot] = kpos + 1;
				a.ex_val[d.sig_off + slot] = k1;
			}
		}
		if (HIST)
			kbefore += tot2 >> 16;
		if (nv) {
			if (!KEY2) {
				out[i0 >> 3] = (uint8_t) key;
			} else {
				out[i0 >> 2] = (uint8_t) k0;
				if (nv > 4)
					out[(i0 >> 2) + 1] = (uint8_t) k1;
			}
			if (HIST) {
#pragma unroll
				for (int q = 0; q < 8; q++) {
					if ((uint32_t) q < nv) {
						const uint32_t val = (zz[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
						atomicAdd(&myhist[val & 0xFFu], 1u);
						if (val > 255u)
							atomicAdd(&myhist[val >> 8], 1u);
					}
				}
			}
			if (nv == 8 && cnt == 0) {
				uint2 v;
				v.x = lo0;
				v.y = lo1;
				__builtin_memcpy(p, &v, 8);
			} else {
#pragma unroll
				for (int q = 0; q < 8; q++) {
					if ((uint32_t) q < nv) {
						uint32_t val = (zz[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
						if (S5 && ((wide >> q) & 1u))
							val = (~val & 0xFFFFu) | 0x10000u;
						*p++ = (uint8_t) val;
						if (val > 255u)
							*p++ = (uint8_t) (val >> 8);
						if (val > 65535u)
							*p++ = (uint8_t) (val >> 16);
					}
				}
			}
		}
		ebase += tot;
	}
	if (HIST) { // the chunk's counts to its read's; a thread clears what it has read (the next chunk counts behind
		    // three barriers)
		__syncthreads();
		if (last && threadIdx.x == 0) // the read's count of such key bytes (k_zs_table takes it from its first chunk's slot)
			a.zkcnt[t - d.j] = (uint32_t) (uni64(s_excl) >> 40) + q0 + q1 + q2 + q3;
		uint32_t c = 0;
		for (int i = 0; i < 16; i++) {
			c += s_hist[i][threadIdx.x];
			s_hist[i][threadIdx.x] = 0;
		}
		if (c)
			atomicAdd(&a.zhist[(uint64_t) d.read * 256 + threadIdx.x], c);
	}
	} // ticket loop
}

// ------------------------------------------------------------------ decode
//
// Chunk j of a read needs two things from the chunks before it: the number of exceptions
// (its data bytes start at klen + j*CHUNK + E) and the value of the last sample (the
// deltas are a running sum, trans.c:260).  E comes from the key bytes alone, so it is
// published before any data is touched; the sample value is published after the chunk
// has summed its own deltas.  Two look-back chains over the same ticket order.
//
// The payload a lane keeps between the phases is the COMPRESSED form (8 bytes per 8
// samples, 32 VGPRs per chunk quarter) plus one 16-bit base per sub-tile; values are
// expanded twice (once to sum the deltas, once to store) - ALU is cheap, registers are
// what bounds the number of chunks in flight per CU.

// key bits (svb16) / 2-bit codes (svb32) of the 8 samples at i0, masked to the valid ones
template <bool KEY2>
__device__ __forceinline__ uint32_t load_key(const uint8_t *in, uint32_t i0, uint32_t n)
{
	uint32_t kk = 0;
	if (i0 < n) {
		if (!KEY2) {
			kk = in[i0 >> 3];
		} else {
			kk = in[i0 >> 2];
			if (i0 + 4 < n)
				kk |= (uint32_t) in[(i0 >> 2) + 1] << 8;
		}
		const uint32_t nv = n - i0;
		if (nv < 8)
			kk &= KEY2 ? ((1u << (2 * nv)) - 1u) : ((1u << nv) - 1u);
	}
	return kk;
}

template <bool KEY2>
__device__ __forceinline__ uint32_t key_extra_bytes(uint32_t kk)
{
	if (!KEY2)
		return __popc(kk);
	uint32_t c = 0;
#pragma unroll
	for (int q = 0; q < 8; q++)
		c += (kk >> (2 * q)) & 3u;
	return c;
}

// Slow path of one sub-tile (exceptions, a ragged tail, or the end of the stream is near):
// byte-wise, bounds-checked gather of the lane's values into packed 16-bit pairs.
// `eb` = exceptions in front of the sub-tile; returns the sub-tile's exception count.
// S5: values may be 17 bits wide (slow5lib); bit q of `hib` = bit 16 of the lane's value q.
template <bool KEY2, bool S5 = false>
__device__ __forceinline__ uint32_t gather_slow(const uint8_t *in, const uint8_t *data, uint64_t dlen,
						uint32_t i0, uint32_t n, uint64_t eb, uint32_t v[4], uint32_t &hib)
{
	hib = 0;
	const uint32_t kk = load_key<KEY2>(in, i0, n);
	const uint32_t c = key_extra_bytes<KEY2>(kk);
	const uint32_t inc = wave_incl_scan_dpp(c);
	const uint32_t tot = (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
	uint64_t p = eb + i0 + (inc - c);
	const uint32_t nv = i0 < n ? min(8u, n - i0) : 0u;
	v[0] = v[1] = v[2] = v[3] = 0;
#pragma unroll
	for (int q = 0; q < 8; q++) {
		if ((uint32_t) q < nv) {
			const uint32_t code = KEY2 ? ((kk >> (2 * q)) & 3u) : ((kk >> q) & 1u);
			uint32_t val = p < dlen ? data[p] : 0u;
			if (code >= 1)
				val |= (p + 1 < dlen ? (uint32_t) data[p + 1] : 0u) << 8;
			if (S5 && code >= 2)
				hib |= (p + 2 < dlen ? (uint32_t) data[p + 2] & 1u : 0u) << q;
			p += 1 + code;
			v[q >> 1] |= val << (16 * (q & 1));
		}
	}
	return tot;
}

// inverse zig-zag of pair q of a gathered lane; a value's bit 16 ends up in bit 15 of z >> 1
__device__ __forceinline__ uint32_t unzz_pair_hib(uint32_t z, uint32_t hib, int q)
{
	return unzz_pair(z) ^ ((((hib >> (2 * q)) & 1u) << 15) | (((hib >> (2 * q + 1)) & 1u) << 31));
}

// ---- key scan: the exception counts depend on the key bytes only (n/8 bytes, 4 % of the
// stream), so they are settled by two tiny kernels before any data is touched; the main
// kernel then starts its data loads straight from the chunk descriptor.

// One workgroup per chunk: per wave quarter, which sub-tiles are not plain and how many
// extra data bytes (exceptions) the quarter holds.  A wave quarter's key bytes are contiguous
// (1 KiB for svb16, 2 KiB for svb32): each lane takes 16 of them with one (unaligned) 16-byte
// load, the count is one popcount reduction and the per-sub-tile flags come from one ballot.
template <bool KEY2, bool S5 = false>
__global__ __launch_bounds__(CWG) void k_svb_keyscan(DecodeArgs a)
{
	// one WAVE per chunk, its four quarters one after the other (a workgroup per chunk: four times the waves for
	// one 16-byte load per lane each)
	const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (c >= uni(a.ctl->nchunks))
		return;
	ChunkDesc *dp = a.chunks + c;
	if (!uni(dp->cap_ok))
		return;
	const uint32_t n = uni(dp->n);
	const uint8_t *in = a.in + uni64(dp->out_base) + (S5 ? 4 : 0);
	const uint64_t in_len = uni64(a.in_len[uni(dp->read)]) - (S5 ? 4 : 0);
	const uint32_t klen = KEY2 ? (n + 3) / 4 : (n >> 3) + (((n & 7) + 7) >> 3);
	const int lane = threadIdx.x & 63;
	constexpr int NL = KEY2 ? 2 : 1;            // 16-byte loads per lane
	constexpr uint32_t SPB = KEY2 ? 4 : 8;      // samples per key byte
	const uint32_t cj = uni(dp->j);
#pragma unroll 1
	for (int w = 0; w < 4; w++) {
	const uint32_t ws = cj * CHUNK + w * WAVE_SAMPLES;
	if (ws >= n && w)
		break; // (the read ends in an earlier quarter: nothing here - the descriptor's zeros stand)
	uint32_t cnt = 0;
	uint32_t kmask = 0;
	uint32_t bad = 0;
#pragma unroll
	for (int h = 0; h < NL; h++) {
		// key bytes [kb, kb+16) of the stream = samples [kb*SPB, (kb+16)*SPB)
		const uint32_t kb = ws / SPB + h * 1024 + lane * 16;
		uint32_t q[4] = { 0, 0, 0, 0 };
		if (kb < klen) {
			// (the stream's very last key byte may carry bits of samples beyond n: byte path)
			if ((uint64_t) kb + 16 <= in_len && (kb + 16 < klen || (kb + 16 == klen && n % SPB == 0))) {
				uint4 v;
				__builtin_memcpy(&v, in + kb, 16);
				q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
			} else {
				for (uint32_t b = 0; b < 16 && kb + b < klen; b++) {
					uint32_t kk = in[kb + b];
					// bits of samples at or beyond n do not count
					const uint32_t s0 = (kb + b) * SPB;
					if (s0 + SPB > n)
						kk &= (1u << ((n - s0) * (KEY2 ? 2 : 1))) - 1u;
					q[b >> 2] |= kk << (8 * (b & 3));
				}
			}
		}
		uint32_t any = q[0] | q[1] | q[2] | q[3];
		if (!KEY2) {
			cnt += __popc(q[0]) + __popc(q[1]) + __popc(q[2]) + __popc(q[3]);
		} else {
#pragma unroll
			for (int i = 0; i < 4; i++) {
				// sum of the 2-bit codes: low bits + 2 x high bits
				cnt += __popc(q[i] & 0x55555555u) + 2 * __popc(q[i] & 0xAAAAAAAAu);
				bad |= q[i] & 0xAAAAAAAAu;
			}
		}
		// sub-tile k of this wave = key bytes [k*64/NL', ...): svb16: 64 bytes = 4 lanes;
		// svb32: 128 bytes = 8 lanes of this half... lanes are ordered by key byte
		const unsigned long long nz = __ballot(any != 0);
		if (!KEY2) {
#pragma unroll
			for (int k = 0; k < CK; k++)
				if ((nz >> (4 * k)) & 0xFull)
					kmask |= 1u << k;
		} else {
#pragma unroll
			for (int k = 0; k < CK / 2; k++)
				if ((nz >> (8 * k)) & 0xFFull)
					kmask |= 1u << (k + h * (CK / 2));
		}
	}
	// ragged tail: the sub-tile that holds sample n-1 when n is not a multiple of 8
	if ((n & 7) && n > ws && n - ws <= WAVE_SAMPLES)
		kmask |= 1u << ((n - 1 - ws) / SUB);
	const uint32_t inc = wave_incl_scan_dpp(cnt);
	uint64_t etot = (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
	// 3- and 4-byte codes cannot come from a 16-bit signal: poison the count so that the
	// read fails its length check and its offsets fall out of range
	if (KEY2 && !S5 && __ballot(bad != 0))
		etot += 1u << 30;
	if (lane == 0) {
		dp->ecnt[w] = (uint32_t) (etot > 0xFFFFFFFFull ? 0xFFFFFFFFull : etot);
		dp->kmask[w] = (uint16_t) kmask;
	}
	}
}

// One thread per read: exclusive prefix of the chunk counts, and the verdict on the stream
// length (decode.hpp:23 consumes klen + n + #exceptions bytes).
template <bool KEY2, bool S5 = false>
__global__ __launch_bounds__(256) void k_svb_keyprefix(DecodeArgs a)
{
	// one wave per read (see k_ex_prefix)
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63;
	if (r >= a.nreads)
		return;
	const uint32_t n = a.nsamp[r];
	if (n == 0)
		return; // out_n[r] = 0 written by k_chunk_prep
	const uint32_t klen = KEY2 ? (n + 3) / 4 : (n >> 3) + (((n & 7) + 7) >> 3);
	const uint64_t in_len = a.in_len[r] - (S5 ? 4 : 0);
	ChunkDesc *dp = a.chunks + a.first_chunk[r];
	if (a.in_len[r] < (S5 ? 4u : 0u) || klen > in_len || !dp->cap_ok) { // cap_ok: k_chunk_prep (S5: the count in the stream)
		if (lane == 0)
			a.out_n[r] = CFAIL32;
		return;
	}
	const uint32_t nch = (n + CHUNK - 1) / CHUNK;
	uint64_t e = 0;
	for (uint32_t j0 = 0; j0 < nch; j0 += 64) {
		const uint32_t j = j0 + lane;
		// (a chunk's count may carry k_svb_keyscan's poison bit 30: the low 20 bits and the rest are summed apart)
		const uint64_t c = j < nch ? (uint64_t) dp[j].ecnt[0] + dp[j].ecnt[1] + dp[j].ecnt[2] + dp[j].ecnt[3] : 0ull;
		const uint32_t lo = wave_incl_scan_dpp((uint32_t) (c & 0xFFFFFu)), hi = wave_incl_scan_dpp((uint32_t) (c >> 20));
		const uint64_t inc = (uint64_t) lo + ((uint64_t) hi << 20);
		if (j < nch)
			dp[j].ebefore = e + inc - c;
		e += (uint64_t) (uint32_t) __builtin_amdgcn_readlane((int) lo, 63) +
		     ((uint64_t) (uint32_t) __builtin_amdgcn_readlane((int) hi, 63) << 20);
	}
	// slow5_press.c:1098: the decoder must consume exactly the bytes it was given
	if (lane == 0)
		a.out_n[r] = (S5 ? (uint64_t) klen + n + e == in_len : (uint64_t) klen + n + e <= in_len) ? n : CFAIL32;
}

#ifdef DEC_STAMPS
extern "C" int press_hip_debug_stamps(uint64_t *dst, uint32_t nwords)
{
	for (uint32_t i = 0; i < nwords; i++)
		dst[i] = 0;
	const int rc = stamps_read(dst, nwords);
	return rc ? rc : ex_stamps_read(dst, nwords);
}
#endif

// Main decode kernel.  Structure per wave quarter (16 sub-tiles):
//   * the plain sub-tiles (no exception, no ragged tail, not at the end of the stream) are
//     handled by fully unrolled loops that contain no load except their own 8-byte data
//     load - so the compiler needs no conservative s_waitcnt between the 16 stores;
//   * the few other sub-tiles go through ROLLED loops over the set bits of `kmask`
//     (byte-wise gather, one copy of the code);
//   * both write their per-lane and per-sub-tile running sums to a small wave-private LDS
//     table, which also frees the registers a per-sub-tile array would take.
//
// FUSE (recode, press_hip_recode_batch): the samples go on to an exception-split press in the same call, and phase 3
// holds what that press's pass A (k_ex_scan_chunked<false, HUFF>) would read them again for.  So the wave leaves, in the
// PRESS-side descriptor of its chunk (f.first_chunk[read] + j: the two chunk tables hand out their ids by atomics of their
// own), the quarter's exception count and flagged sub-tiles, the OR of the samples and zd[0] in ReadMeta and - FUSE 2, a
// static-Huffman destination - the quarter's code bits; pass A is then not launched.  An exception there is the 16-BIT
// wrapped zig-zag delta above 255, never sample 0: a plain sub-tile holds none (its values are single bytes, which the
// 32-bit delta of slow5's stream is only where the wrapped one is the same byte); the others recompute it from the
// deltas they have undone.
//
// OUT = float (press_hip_depress_pa_batch): the other second consumer.  Phase 3 converts the 8 samples a lane holds to
// picoamperes with the read's two calibration floats (f.cal, loaded once per workgroup) and writes them to f.pa as two
// 16-byte stores; the ragged tail writes its floats one by one and none at or beyond n.  a.sig is not used: no int16
// copy of the samples is made.
//
// DEG (press_hip_recode_degraded_*, with FUSE): the samples are rounded to multiples of 2^b (D_b, degrade_pair: two
// packed 16-bit operations a pair) behind the inverse scan and in front of the store and of the counts, so the stream
// keeps what the press half will read and pass A's results describe the DEGRADED read.  The zig-zag deltas of the
// degraded samples are no longer the stream's: the lane takes them again from its eight degraded samples and the degraded
// value in front of them - the base b16 the scan has just added, which IS the sample in front of the lane (0 in front of
// a read's first) - and a plain sub-tile, whose stream bytes hold no exception, may well hold one afterwards (a step of
// 127 becomes one of up to 127 + 2^b): under DEG the plain sub-tiles count as the others do.  A compile-time variant:
// the instantiations without DEG are what they were.
template <bool KEY2, bool ZD, bool S5 = false, int FUSE = 0, typename OUT = int16_t, bool DEG = false>
__global__ __launch_bounds__(CWG) void k_svb_decode_chunked(DecodeArgs a, FuseArgs f)
{
	static_assert(!FUSE || ZD, "the fused counts are those of the zig-zag delta methods");
	static_assert(!DEG || FUSE, "D_b is applied where the samples go on to a press in the same call");
	constexpr bool PA = sizeof(OUT) == sizeof(float);
	static_assert(!PA || !FUSE, "one second consumer at a time");
#ifdef DEC_STAMPS
	const uint64_t t_start = __builtin_amdgcn_s_memtime();
#endif
	// FUSE 2: code length of every one-byte value, 1 << 16 for a value without a code, [256] = 0 (as k_ex_scan_chunked)
	__shared__ uint32_t s_len[FUSE == 2 ? 257 : 1];
	__shared__ uint32_t s_ticket;
	__shared__ uint32_t s_wsum[4];
	__shared__ uint32_t s_sbase;
	__shared__ uint16_t s_xl[4][CK][64];  // delta sum in front of the lane, within its sub-tile
	__shared__ uint32_t s_sub[4][CK];     // per sub-tile: exception count, later delta total / base
	__shared__ uint32_t s_epre[4][CK];    // exceptions of the wave's earlier sub-tiles

	const int lane = threadIdx.x & 63;
	const int w = (int) uni(threadIdx.x >> 6);
	if (blockIdx.x >= uni(a.ctl->nchunks))
		return; // (the grid is an upper bound: surplus workgroups draw no ticket - blockIdx only COUNTS the workgroups)
	if (FUSE == 2) { // (visible behind the ticket's barrier)
		const uint32_t l = f.huff->enc[threadIdx.x] >> 24;
		s_len[threadIdx.x] = l ? l : 0x10000u;
		if (threadIdx.x == 0)
			s_len[256] = 0;
	}
#ifdef DEC_BLOCKIDX_TICKET
	// DIAGNOSTIC BUILD ONLY (tools/build_variants.sh "tkb:-DDEC_BLOCKIDX_TICKET"): what the ticket in front of every
	// workgroup costs.  Chunk ids from blockIdx rely on workgroups starting in the order of their ids, which HIP does not
	// promise - the look-back can deadlock where they do not.  Measured: 0.58-0.61 instead of 0.66-0.69 ms.
	const uint32_t t = blockIdx.x;
	(void) s_ticket;
	if (FUSE == 2)
		__syncthreads();
#else
	if (threadIdx.x == 0)
		s_ticket = atomicAdd(&a.ctl->ticket, 1u);
	__syncthreads();
	const uint32_t t = uni(s_ticket);
#endif
	if (t >= a.ctl->nchunks)
		return;
#ifdef DEC_STAMPS
	if (threadIdx.x == 0 && t < 65536)
		g_stamps[t * 8 + 0] = t_start;
#endif
	STAMP(1);
	const ChunkDesc *dp = a.chunks + t;
	const ChunkU d = load_chunk(dp);
	const uint32_t n = d.n;
	const uint32_t first = d.j * CHUNK;
	const bool last = first + CHUNK >= n;
	if (!d.cap_ok) { // not even the key bytes are there (out_n: k_svb_keyprefix)
		if (ZD && threadIdx.x < 64)
			(void) lookback(a.gran, t, d.j, 0, last);
		return;
	}
	const uint8_t *in = a.in + d.out_base + (S5 ? 4 : 0);
	const uint64_t in_len = uni64(a.in_len[d.read]) - (S5 ? 4 : 0);
	OUT *out = (PA ? (OUT *) f.pa : (OUT *) a.sig) + d.sig_off;
	const float c0 = PA ? __uint_as_float(uni(__float_as_uint(f.cal[2 * (size_t) d.read]))) : 0.f;
	const float c1 = PA ? __uint_as_float(uni(__float_as_uint(f.cal[2 * (size_t) d.read + 1]))) : 0.f;
	const uint32_t klen = KEY2 ? (n + 3) / 4 : (n >> 3) + (((n & 7) + 7) >> 3);
	const uint64_t dlen = in_len - klen; // bytes in the data section (cap_ok: klen <= in_len)
	const uint8_t *data = in + klen;
	const uint32_t ws = first + w * WAVE_SAMPLES;
	const uint32_t e0 = uni(dp->ecnt[0]), e1 = uni(dp->ecnt[1]), e2 = uni(dp->ecnt[2]), e3 = uni(dp->ecnt[3]);
	const uint32_t ew = w == 0 ? e0 : w == 1 ? e1 : w == 2 ? e2 : e3;
	const uint64_t ebase = uni64(dp->ebefore) + (w > 0 ? e0 : 0u) + (w > 1 ? e1 : 0u) + (w > 2 ? e2 : 0u);
	// sub-tiles of this wave that exist, and those that are not plain; a sub-tile whose
	// 8-byte windows could reach past the end of the stream is not plain either
	const uint32_t nsub = ws >= n ? 0u : min((uint32_t) CK, (n - ws + SUB - 1) / SUB);
	const uint32_t live = nsub >= 32 ? ~0u : ((1u << nsub) - 1u);
	uint32_t kmask = uni(dp->kmask[w]) & live;
#pragma unroll
	for (int k = 0; k < CK; k++)
		if (((live >> k) & 1u) && ebase + ew + ws + k * SUB + SUB + 8 > dlen)
			kmask |= 1u << k;
	const uint32_t plain = live & ~kmask;
	STAMP(2);

	// ---- exceptions of the non-plain sub-tiles -> data offset of every sub-tile
	if (lane < CK)
		s_sub[w][lane] = 0;
	wave_lds_sync();
	for (uint32_t m = kmask; m; m &= m - 1) {
		const uint32_t k = (uint32_t) __builtin_ctz(m);
		const uint32_t kk = load_key<KEY2>(in, ws + k * SUB + lane * 8, n);
		const uint32_t inc = wave_incl_scan_dpp(key_extra_bytes<KEY2>(kk));
		if (lane == 63)
			s_sub[w][k] = inc;
	}
	wave_lds_sync();
	if (lane < CK) {
		const uint32_t v = s_sub[w][lane];
		const uint32_t inc = wave_incl_scan_dpp(v);
		s_epre[w][lane] = inc - v;
	}
	wave_lds_sync();

	// ---- phase 1: data loads of the plain sub-tiles (8 bytes per lane, any alignment)
	uint2 dat[CK];
#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		// (a zeroed register pair of its own for every sub-tile: left to itself the compiler kept the two halves of
		// sub-tile 0 in registers that are no pair, loaded into a third place, copied one half over - and waited for
		// that load before it issued the other fifteen: two memory round trips per chunk instead of one)
		unsigned long long d64;
		asm volatile("v_mov_b64 %0, 0" : "=v"(d64)); // (a register PAIR of its own: the 8-byte load lands in it)
		if ((plain >> k) & 1u) { // uniform
			const uint64_t eb = ebase + uni(s_epre[w][k]);
			if (i0 < n)
				d64 = ld8_stream(data + eb + i0);
		}
		const uint2 dd = make_uint2((uint32_t) d64, (uint32_t) (d64 >> 32));
		dat[k] = dd; // (k_low_decode_chunked's unconditional loads were tried here too: 82 instead of 51 VGPRs, 6 % slower)
	}

	// ---- phase 2: delta sums (16-bit wraparound) - per lane inside its sub-tile, per sub-tile
	if (ZD) {
#pragma unroll
		for (int k = 0; k < CK; k++) {
			if ((plain >> k) & 1u) { // uniform
				uint32_t v[4];
				expand8(dat[k], v);
				uint32_t acc = 0;
#pragma unroll
				for (int q = 0; q < 4; q++)
					acc = pk_add16(acc, unzz_pair(v[q]));
				const uint32_t tot16 = (acc + (acc >> 16)) & 0xFFFFu;
				const uint32_t inc = wave_incl_scan_dpp(tot16);
				s_xl[w][k][lane] = (uint16_t) (inc - tot16);
				if (lane == 63)
					s_sub[w][k] = inc;
			}
		}
		for (uint32_t m = kmask; m; m &= m - 1) {
			const uint32_t k = (uint32_t) __builtin_ctz(m);
			const uint32_t i0 = ws + k * SUB + lane * 8;
			uint32_t v[4], hib;
			(void) gather_slow<KEY2, S5>(in, data, dlen, i0, n, ebase + uni(s_epre[w][k]), v, hib);
			uint32_t acc = 0;
#pragma unroll
			for (int q = 0; q < 4; q++)
				acc = pk_add16(acc, unzz_pair_hib(v[q], hib, q));
			const uint32_t tot16 = (acc + (acc >> 16)) & 0xFFFFu;
			const uint32_t inc = wave_incl_scan_dpp(tot16);
			s_xl[w][k][lane] = (uint16_t) (inc - tot16);
			if (lane == 63)
				s_sub[w][k] = inc;
		}
		wave_lds_sync();
		// exclusive prefix over the sub-tiles of the wave
		uint32_t wtot = 0;
		{
			const uint32_t v = (lane < (int) nsub) ? s_sub[w][lane < CK ? lane : 0] : 0u;
			const uint32_t inc = wave_incl_scan_dpp(v);
			wave_lds_sync();
			if (lane < CK)
				s_sub[w][lane] = inc - v;
			wtot = (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
		}
		wave_lds_sync();
		if (lane == 0)
			s_wsum[w] = wtot & 0xFFFFu;
	}
	STAMP(3);

	// ---- sample value in front of this wave: within the chunk (LDS) and before it (look-back)
	uint32_t sb = 0;
	if (ZD) {
		__syncthreads();
		STAMP(4);
		const uint32_t u0 = uni(s_wsum[0]), u1 = uni(s_wsum[1]), u2 = uni(s_wsum[2]), u3 = uni(s_wsum[3]);
		if (w == 0) {
			const uint32_t sv = (uint32_t) lookback(a.gran, t, d.j, (uint64_t) ((u0 + u1 + u2 + u3) & 0xFFFFu), last);
			if (lane == 0)
				s_sbase = sv;
		}
		__syncthreads();
		sb = uni(s_sbase) + (w > 0 ? u0 : 0u) + (w > 1 ? u1 : 0u) + (w > 2 ? u2 : 0u);
	}
	STAMP(5);

	// Every load has completed by now (the barrier above drains vmcnt).  Re-define the payload
	// registers through an empty asm so that the compiler stops associating them with memory
	// operations: otherwise it puts an s_waitcnt vmcnt(0) in front of every sub-tile of the
	// store loop and each 16-byte store is drained before the next one is issued.
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
	for (int k = 0; k < CK; k++)
		asm volatile("" : "+v"(dat[k].x), "+v"(dat[k].y));

	// FUSE: the read's press-side chunk (none for a read k_svb_keyprefix has refused: its count went to the press as 0)
	const bool fz = FUSE && uni(a.out_n[d.read]) != CFAIL32;
	uint32_t f_kmask = 0, f_etot = 0, f_ored = 0, f_bits = 0, f_s0 = 0;

	// ---- phase 3: expand again, prefix inside the lane, add the bases, store
#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		if ((plain >> k) & 1u) { // uniform; plain sub-tiles hold only complete lanes
			uint32_t v[4];
			expand8(dat[k], v);
			uint32_t front = 0; // DEG: the sample in front of the lane's eight
			if (ZD) {
#pragma unroll
				for (int q = 0; q < 4; q++)
					v[q] = unzz_pair(v[q]);
				(void) lane_prefix8(v);
				const uint32_t b16 = (sb + uni(s_sub[w][k]) + s_xl[w][k][lane]) & 0xFFFFu;
				const uint32_t b2 = b16 | (b16 << 16);
#pragma unroll
				for (int q = 0; q < 4; q++)
					v[q] = pk_add16(v[q], b2);
				if (DEG)
					front = b16;
			}
			uint4 z = make_uint4(0, 0, 0, 0);
			if constexpr (DEG) { // D_b of the samples, and the zig-zag deltas of what is left
				const uint32_t fd = degrade_pair(front, f.deg_h2, f.deg_m2) << 16;
#pragma unroll
				for (int q = 0; q < 4; q++)
					v[q] = degrade_pair(v[q], f.deg_h2, f.deg_m2);
				z = make_uint4(zd_pair(v[0], fd), zd_pair(v[1], v[0]), zd_pair(v[2], v[1]), zd_pair(v[3], v[2]));
			}
			if (i0 < n) {
				if constexpr (PA)
					st_pa8(out + i0, v, c0, c1);
				else
					st16_stream(out + i0, make_uint4(v[0], v[1], v[2], v[3]));
			}
			if constexpr (DEG) { // the counts of a sub-tile that is not plain (below): the degraded values may hold exceptions
				const uint32_t nv = i0 + 8 <= n ? 8u : (i0 < n ? n - i0 : 0u);
				if (k == 0)
					f_s0 = v[0];
#pragma unroll
				for (int h = 0; h < 4; h++)
					f_ored |= nv >= (uint32_t) (2 * h + 2) ? v[h] : nv == (uint32_t) (2 * h + 1) ? (v[h] & 0xFFFFu) : 0u;
				if (nv < 8) { // (a plain sub-tile holds complete lanes; zeros at or beyond n all the same)
					const uint32_t zz[4] = { z.x, z.y, z.z, z.w };
					uint32_t zc[4];
#pragma unroll
					for (uint32_t h = 0; h < 4; h++)
						zc[h] = nv >= 2 * h + 2 ? zz[h] : nv == 2 * h + 1 ? (zz[h] & 0xFFFFu) : 0u;
					z = make_uint4(zc[0], zc[1], zc[2], zc[3]);
				}
				const uint32_t em = exc_mask(z, i0);
				if (__ballot(em != 0)) {
					f_kmask |= 1u << k;
					const uint32_t inc = wave_incl_scan_dpp(__popc(em));
					f_etot += (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
				}
				if (FUSE == 2) {
					const uint32_t zz[4] = { z.x, z.y, z.z, z.w };
					const uint32_t lowm = low_mask(z, i0, n);
#pragma unroll
					for (int h = 0; h < 8; h++)
						f_bits += s_len[((lowm >> h) & 1u) ? ((zz[h >> 1] >> (16 * (h & 1))) & 0xFFu) : 256u];
				}
			} else if (FUSE && i0 < n) { // one-byte values only: no exception; their code lengths straight from the stream's bytes
				f_ored |= v[0] | v[1] | v[2] | v[3];
				if (k == 0)
					f_s0 = v[0];
				if (FUSE == 2) {
#pragma unroll
					for (int h = 0; h < 8; h++) {
						const uint32_t b = ((h < 4 ? dat[k].x : dat[k].y) >> (8 * (h & 3))) & 0xFFu;
						f_bits += s_len[h == 0 && i0 == 0 ? 256u : b]; // (sample 0 is stored raw)
					}
				}
			}
		}
	}
	for (uint32_t m = kmask; m; m &= m - 1) {
		const uint32_t k = (uint32_t) __builtin_ctz(m);
		const uint32_t i0 = ws + k * SUB + lane * 8;
		uint32_t v[4], hib;
		(void) gather_slow<KEY2, S5>(in, data, dlen, i0, n, ebase + uni(s_epre[w][k]), v, hib);
		if (ZD) {
#pragma unroll
			for (int q = 0; q < 4; q++)
				v[q] = unzz_pair_hib(v[q], hib, q);
			uint4 z = make_uint4(0, 0, 0, 0);
			if (FUSE) { // zig-zag of the 16-bit deltas again: what the press side calls zd (zeros at or beyond n: gather_slow)
				const s16x2 d0 = __builtin_bit_cast(s16x2, v[0]), d1 = __builtin_bit_cast(s16x2, v[1]),
					    d2 = __builtin_bit_cast(s16x2, v[2]), d3 = __builtin_bit_cast(s16x2, v[3]);
				z = make_uint4(__builtin_bit_cast(uint32_t, (d0 << 1) ^ (d0 >> 15)), __builtin_bit_cast(uint32_t, (d1 << 1) ^ (d1 >> 15)),
					       __builtin_bit_cast(uint32_t, (d2 << 1) ^ (d2 >> 15)), __builtin_bit_cast(uint32_t, (d3 << 1) ^ (d3 >> 15)));
			}
			(void) lane_prefix8(v);
			const uint32_t b16 = (sb + uni(s_sub[w][k]) + s_xl[w][k][lane]) & 0xFFFFu;
			const uint32_t b2 = b16 | (b16 << 16);
#pragma unroll
			for (int q = 0; q < 4; q++)
				v[q] = pk_add16(v[q], b2);
			if constexpr (DEG) { // D_b, and zd again from the degraded samples (those at or beyond n repeat the last: zeros)
				const uint32_t fd = degrade_pair(b16, f.deg_h2, f.deg_m2) << 16;
#pragma unroll
				for (int q = 0; q < 4; q++)
					v[q] = degrade_pair(v[q], f.deg_h2, f.deg_m2);
				z = make_uint4(zd_pair(v[0], fd), zd_pair(v[1], v[0]), zd_pair(v[2], v[1]), zd_pair(v[3], v[2]));
			}
			if (FUSE) {
				const uint32_t nv = i0 + 8 <= n ? 8u : (i0 < n ? n - i0 : 0u);
				if (k == 0)
					f_s0 = v[0];
#pragma unroll
				for (int h = 0; h < 4; h++) // samples at or beyond n count nothing
					f_ored |= nv >= (uint32_t) (2 * h + 2) ? v[h] : nv == (uint32_t) (2 * h + 1) ? (v[h] & 0xFFFFu) : 0u;
				const uint32_t em = exc_mask(z, i0);
				if (__ballot(em != 0)) {
					f_kmask |= 1u << k;
					const uint32_t inc = wave_incl_scan_dpp(__popc(em));
					f_etot += (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
				}
				if (FUSE == 2) {
					const uint32_t zz[4] = { z.x, z.y, z.z, z.w };
					const uint32_t lowm = low_mask(z, i0, n);
#pragma unroll
					for (int h = 0; h < 8; h++)
						f_bits += s_len[((lowm >> h) & 1u) ? ((zz[h >> 1] >> (16 * (h & 1))) & 0xFFu) : 256u];
				}
			}
		}
		if constexpr (PA) {
			if (i0 + 8 <= n) {
				st_pa8(out + i0, v, c0, c1);
			} else if (i0 < n) {
#pragma unroll
				for (int q = 0; q < 8; q++)
					if ((uint32_t) q < n - i0)
						out[i0 + q] = pa_of(v, q, c0, c1);
			}
		} else if (i0 + 8 <= n) {
			st16_stream(out + i0, make_uint4(v[0], v[1], v[2], v[3]));
		} else if (i0 < n) {
#pragma unroll
			for (uint32_t q = 0; q < 8; q++)
				if (q < n - i0)
					out[i0 + q] = (int16_t) (v[q >> 1] >> (16 * (q & 1)));
		}
	}
	if (FUSE && fz) { // what pass A leaves for this quarter (k_ex_scan_chunked's tail)
		const uint32_t pt = uni(f.first_chunk[d.read]) + d.j;
		if (FUSE == 2) {
			const uint32_t nocode = (f_bits >> 16) ? 0x80000000u : 0u; // a value the table has no code for
			const uint32_t inc = wave_incl_scan_dpp(f_bits & 0xFFFFu);
			if (lane == 63)
				f.cbits[pt].q[w] = inc;
			f_ored = ((f_ored | (f_ored >> 16)) & 0xFFFFu) | nocode;
		} else {
			f_ored = (f_ored | (f_ored >> 16)) & 0xFFFFu;
		}
		if (ws < n) {
#pragma unroll
			for (int dd = 32; dd >= 1; dd >>= 1)
				f_ored |= (uint32_t) __shfl_xor((int) f_ored, dd, 64);
			ReadMeta *m = f.meta + d.read;
			if (lane == 0) {
				atomicOr(&m->ored, f_ored);
				f.chunks[pt].ecnt[w] = f_etot;
				f.chunks[pt].kmask[w] = (uint16_t) f_kmask;
				if (ws == 0) { // zd[0]: the zig-zag of sample 0 itself
					const int32_t s0 = (int16_t) f_s0;
					m->zd0 = (uint32_t) ((s0 << 1) ^ (s0 >> 15)) & 0xFFFFu;
				}
			}
		}
	}
	STAMP(6);
}

// ------------------------------------------------------------------ launchers

// Press: the chunk table, then the persistent encoder.  pk (the packed press, press_hip_press_packed): the counting pass
// has given every stream's length and the scan the offsets; the chunk table is made against them (k_chunk_prep<.., EXACT>)
// and the encoder runs as it is - it stores no byte behind a stream's end, so its neighbour may start there.
template <bool KEY2, bool ZD, bool S5 = false, bool HIST = false>
static void run_encode(const BatchArgs &a, const PackArgs *pk, hipStream_t s)
{
	launch_chunk_prep(a, KEY2, S5 ? 4u : 0u, false, pk, s);
	// persistent grid: as many workgroups as are resident (4 per CU)
	const uint32_t grid = a.max_chunks < PERSISTENT_GRID ? a.max_chunks : PERSISTENT_GRID;
	ktime_begin(0, s);
	hipLaunchKernelGGL((k_svb_encode_chunked<KEY2, ZD, S5, HIST>), dim3(grid), dim3(CWG), 0, s, a);
	ktime_end(0, s);
}

void launch_svb_encode_chunked(const BatchArgs &a, bool key2bit, bool zd, hipStream_t s, bool slow5)
{
	if (!a.nreads || !a.max_chunks)
		return;
	if (slow5)
		run_encode<true, true, true>(a, nullptr, s);
	else if (a.zhist && key2bit)
		run_encode<true, true, false, true>(a, nullptr, s);
	else if (a.zhist)
		run_encode<false, true, false, true>(a, nullptr, s);
	else if (key2bit)
		run_encode<true, true>(a, nullptr, s);
	else if (zd)
		run_encode<false, true>(a, nullptr, s);
	else
		run_encode<false, false>(a, nullptr, s);
}

void launch_svb_encode_packed(const BatchArgs &a, bool key2bit, bool zd, bool slow5, const PackArgs &pk, int phases,
			      hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	if (phases & PACK_SIZE) {
		launch_pack_svb_sizes(a, key2bit, zd, slow5, pk.need, s);
		if (pk.layout)
			launch_pack_scan(pk, a.nreads, s);
	}
	if (!(phases & PACK_WRITE))
		return;
	if (slow5)
		run_encode<true, true, true>(a, &pk, s);
	else if (key2bit)
		run_encode<true, true>(a, &pk, s);
	else if (zd)
		run_encode<false, true>(a, &pk, s);
	else
		run_encode<false, false>(a, &pk, s);
}

// The front of every svb decode: the chunk table, then the exception counts, which the key bytes alone give (surplus
// workgroups - max_chunks bounds the real count from above - exit at once)
template <bool KEY2, bool S5>
static void svb_decode_front(const DecodeArgs &a, hipStream_t s)
{
	launch_chunk_prep(a, KEY2, S5 ? 4u : 0u, s);
	hipLaunchKernelGGL((k_svb_keyscan<KEY2, S5>), dim3((a.max_chunks + 3) / 4), dim3(CWG), 0, s, a);
	hipLaunchKernelGGL((k_svb_keyprefix<KEY2, S5>), dim3((a.nreads + 3) / 4), dim3(256), 0, s, a);
}

template <bool KEY2, bool ZD, bool S5 = false, typename OUT = int16_t>
static void run_decode(const DecodeArgs &a, hipStream_t s, const FuseArgs &f = FuseArgs{})
{
	svb_decode_front<KEY2, S5>(a, s);
	ktime_begin(1, s);
	hipLaunchKernelGGL((k_svb_decode_chunked<KEY2, ZD, S5, 0, OUT>), dim3(a.max_chunks), dim3(CWG), 0, s, a, f);
	ktime_end(1, s);
}

void launch_svb_decode_chunked(const DecodeArgs &a, bool key2bit, bool zd, hipStream_t s, bool slow5)
{
	if (!a.nreads || !a.max_chunks)
		return;
	if (slow5)
		run_decode<true, true, true>(a, s);
	else if (key2bit)
		run_decode<true, true>(a, s);
	else if (zd)
		run_decode<false, true>(a, s);
	else
		run_decode<false, false>(a, s);
}

// the same chain with the float writer (press_hip_depress_pa_batch, the fused methods): a.sig is not used
void launch_svb_decode_pa(const DecodeArgs &a, float *pa, const float *cal, bool key2bit, bool zd, bool slow5, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	FuseArgs f{};
	f.pa = pa;
	f.cal = cal;
	if (slow5)
		run_decode<true, true, true, float>(a, s, f);
	else if (key2bit)
		run_decode<true, true, false, float>(a, s, f);
	else if (zd)
		run_decode<false, true, false, float>(a, s, f);
	else
		run_decode<false, false, false, float>(a, s, f);
}

// n[r] = out_n[r], 0 for a read the decoder refused: the sample counts of the press half of a recode
__global__ __launch_bounds__(256) void k_recode_counts(const uint32_t *out_n, uint32_t *n, uint32_t nreads)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r < nreads)
		n[r] = out_n[r] == CFAIL32 ? 0u : out_n[r];
}
void launch_recode_counts(const uint32_t *out_n, uint32_t *n, uint32_t nreads, hipStream_t s)
{
	hipLaunchKernelGGL(k_recode_counts, dim3((nreads + 255) / 256), dim3(256), 0, s, out_n, n, nreads);
}

// A refused read's slot stays as it was.  The press half sees it as an empty read, for which the formats that store a
// count (slow5_svb_zd, the zstd frames over svb) write a stream of a few bytes: the head of such a slot is kept
// aside (save) and put back, with out_len = PRESS_HIP_FAILED for every refused read (!save).
__global__ __launch_bounds__(256) void k_recode_refused(const uint32_t *out_n, uint8_t *out, const uint64_t *out_off,
							  uint64_t *out_len, uint8_t *keep, uint32_t nreads, int save)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= nreads || out_n[r] != CFAIL32)
		return;
	if (keep) {
		const uint64_t cap = out_off[r + 1] - out_off[r];
		const uint32_t nb = cap < RECODE_KEEP ? (uint32_t) cap : RECODE_KEEP;
		uint8_t *slot = out + out_off[r], *k = keep + (size_t) r * RECODE_KEEP;
		for (uint32_t b = 0; b < nb; b++)
			(save ? k[b] : slot[b]) = save ? slot[b] : k[b];
	}
	if (!save)
		out_len[r] = CFAIL64;
}
void launch_recode_refused(const uint32_t *out_n, const BatchArgs &p, uint8_t *keep, bool save, hipStream_t s)
{
	hipLaunchKernelGGL(k_recode_refused, dim3((p.nreads + 255) / 256), dim3(256), 0, s, out_n, p.out, p.out_off, p.out_len,
			   keep, p.nreads, save ? 1 : 0);
}

// the fused decode kernel of a recode: FUSE 2 leaves the code bits a static-Huffman press needs as well, DEG applies D_bits
template <bool KEY2, bool S5>
static void run_decode_fused(const DecodeArgs &d, const FuseArgs &f, ExEnt ent, uint32_t bits, hipStream_t s)
{
	const bool huff = ent == ENT_SHUFF;
	const auto k = bits ? (huff ? k_svb_decode_chunked<KEY2, true, S5, 2, int16_t, true> : k_svb_decode_chunked<KEY2, true, S5, 1, int16_t, true>)
			    : (huff ? k_svb_decode_chunked<KEY2, true, S5, 2> : k_svb_decode_chunked<KEY2, true, S5, 1>);
	ktime_begin(1, s);
	hipLaunchKernelGGL(k, dim3(d.max_chunks), dim3(CWG), 0, s, d, f);
	ktime_end(1, s);
}

// Recode, fused (press_hip_recode_batch): the svb decode of `d` leaves pass A's results in the chunk table of the press
// `p`, whose sample counts p.nsamp are the decoder's verdicts (0 for a read it refuses) - known before the main kernel
// runs, k_svb_keyprefix gives them.  d.sig == p.sig, d.off == p.off; the two sides have a chunk table, a first-chunk list
// and a control block each.  Pass A is not launched.
// pk (the packed form, press_hip_recode_sizes / press_hip_recode_packed): the press half is cut where
// launch_ex_encode_packed cuts it.  PACK_SIZE: the slot table zeroed, the decode with pass A's results, the exception lists
// and the sizes; the reads the source refused lose their size, the scan lays the arena out and the PRESS half's chunk
// table (p.chunks / p.first_chunk) learns the bases.  PACK_WRITE: the section and the encoder as they are.
template <bool KEY2, bool S5>
static void run_recode(const DecodeArgs &d, const BatchArgs &p, ExFmt fmt, ExEnt ent, const PackArgs *pk, int phases, uint32_t bits,
		       hipStream_t s)
{
	if (phases & PACK_SIZE) {
		svb_decode_front<KEY2, S5>(d, s);
		launch_recode_counts(d.out_n, const_cast<uint32_t *>(p.nsamp), d.nreads, s);
		if (pk)
			(void) hipMemsetAsync(pk->slot, 0, ((size_t) p.nreads + 1) * 8, s);
		ex_encode_prep(p, s);
		const FuseArgs f = { p.chunks, p.first_chunk, p.cbits, p.meta, p.huff, nullptr, nullptr, degrade_h2(bits), degrade_m2(bits) };
		run_decode_fused<KEY2, S5>(d, f, ent, bits, s);
		ex_encode_lists(p, fmt, s);
		if (pk) {
			ex_packed_sizes(p, fmt, ent, pk->need, s);
			launch_pack_scan_refused(*pk, d.out_n, d.nreads, s);
			if (pk->layout)
				launch_pack_patch(p, pk->slot, s);
		}
	}
	if (phases & PACK_WRITE) {
		if (pk)
			ex_packed_streams(p, fmt, ent, s);
		else
			ex_encode_streams(p, fmt, ent, s);
	}
}

static void recode(const DecodeArgs &d, const BatchArgs &p, bool key2bit, bool slow5, ExFmt fmt, ExEnt ent, const PackArgs *pk, int phases,
		   uint32_t bits, hipStream_t s)
{
	if (!d.nreads || !d.max_chunks)
		return;
	if (slow5)
		run_recode<true, true>(d, p, fmt, ent, pk, phases, bits, s);
	else if (key2bit)
		run_recode<true, false>(d, p, fmt, ent, pk, phases, bits, s);
	else
		run_recode<false, false>(d, p, fmt, ent, pk, phases, bits, s);
}

void launch_recode_fused(const DecodeArgs &d, const BatchArgs &p, bool key2bit, bool slow5, ExFmt fmt, ExEnt ent, hipStream_t s, uint32_t bits)
{
	recode(d, p, key2bit, slow5, fmt, ent, nullptr, PACK_SIZE | PACK_WRITE, bits, s);
}

void launch_recode_fused_packed(const DecodeArgs &d, const BatchArgs &p, bool key2bit, bool slow5, ExFmt fmt, ExEnt ent,
				const PackArgs &pk, int phases, hipStream_t s, uint32_t bits)
{
	recode(d, p, key2bit, slow5, fmt, ent, &pk, phases, bits, s);
}

} // namespace ph
