// press_exsplit.hip - the exception-split family over the chunk machinery of press_chunk.h: pass A, the lists, pass B,
// the merge of the depress side, and the launchers that run a stage of the table EX_STAGES between them.
//
// vb1e2 family / ex-zd (press.c:2679-3580, ex_zd.c:9-172): the stream is
//   header || u32 nex || exception section || one-byte values of the non-exceptions.
// The section's size depends on ALL exceptions of the read, so the input is read twice:
//   k_ex_scan_chunked  (ticket order + look-back on the exception count): exception list
//                      (position, value) at its final rank, per-chunk counts, OR of the samples
//   k_ex_section       (press_sections.hip): header + section, one lane per read
//   k_low_encode_chunked: the one-byte stream; every chunk knows its offset from the counts,
//                      so no ordering is needed: one workgroup per chunk, 8-byte stores for
//                      sub-tiles without exceptions exactly as in k_svb_encode_chunked.

#include "press_chunk.h"

namespace ph {

// zig-zag deltas of one wave quarter, as in k_svb_encode_chunked phase 1, with the ex-zd
// shift q applied to the samples first (ex_zd.c:383).  hi[k] != 0 marks lanes with an
// exception in sub-tile k; sample 0 of the read is never one (it is stored raw).
__device__ __forceinline__ void quarter_zd(const int16_t *in, uint32_t n, uint32_t ws, int lane, int q,
					   uint4 (&z)[CK], uint32_t &ored)
{
#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		z[k] = make_uint4(0, 0, 0, 0);
		if (i0 < n)
			z[k] = ld16_stream(in + i0);
	}
	uint32_t carry = 0;
	if (ws > 0 && ws < n)
		carry = (uint32_t) (uint16_t) in[ws - 1] << 16;
	uint32_t o = 0;
	const s16x2 qq = { (short) q, (short) q };
#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		uint32_t r[4] = { z[k].x, z[k].y, z[k].z, z[k].w };
		// samples at or beyond n: zero (they neither count nor contribute to the OR)
		if (i0 + 8 > n) {
			const uint32_t nv = i0 < n ? n - i0 : 0;
#pragma unroll
			for (int h = 0; h < 4; h++) {
				if (nv <= (uint32_t) (2 * h))
					r[h] = 0;
				else if (nv == (uint32_t) (2 * h + 1))
					r[h] &= 0xFFFFu;
			}
		}
		o |= r[0] | r[1] | r[2] | r[3];
		const uint32_t raw_w = r[3];
		if (q) {
#pragma unroll
			for (int h = 0; h < 4; h++)
				r[h] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(s16x2, r[h]) >> qq);
		}
		uint32_t c = carry;
		if (q)
			c = __builtin_bit_cast(uint32_t, __builtin_bit_cast(s16x2, c) >> qq);
		const uint32_t pw = prev_lane(r[3], c);
		uint32_t zz[4];
		zz[0] = zd_pair(r[0], pw);
		zz[1] = zd_pair(r[1], r[0]);
		zz[2] = zd_pair(r[2], r[1]);
		zz[3] = zd_pair(r[3], r[2]);
		carry = (uint32_t) __builtin_amdgcn_readlane((int) raw_w, 63);
		if (i0 + 8 > n) { // deltas of samples beyond n are garbage: zero them again
			const uint32_t nv = i0 < n ? n - i0 : 0;
#pragma unroll
			for (int h = 0; h < 4; h++) {
				if (nv <= (uint32_t) (2 * h))
					zz[h] = 0;
				else if (nv == (uint32_t) (2 * h + 1))
					zz[h] &= 0xFFFFu;
			}
		}
		z[k] = make_uint4(zz[0], zz[1], zz[2], zz[3]);
	}
	ored = (o | (o >> 16)) & 0xFFFFu;
}

// raw samples of a lane's 8 samples of a sub-tile (zeros at or beyond n)
__device__ __forceinline__ uint4 sub_load(const int16_t *in, uint32_t n, uint32_t i0)
{
	uint4 r = make_uint4(0, 0, 0, 0);
	if (i0 < n)
		r = ld16_stream(in + i0);
	return r;
}

// their zig-zag deltas (trans.c:75,215), after the ex-zd shift q (ex_zd.c:383).  carry = the
// (raw) sample in front of the sub-tile in bits 16..31; returns the sub-tile's last sample the
// same way for the next one.  ored |= the raw samples below n (qts, ex_zd.c:358).
__device__ __forceinline__ uint4 sub_zd(uint4 raw, uint32_t n, uint32_t i0, uint32_t &carry, int q = 0,
					uint32_t *ored = nullptr)
{
	uint32_t r[4] = { raw.x, raw.y, raw.z, raw.w };
	const uint32_t nv = i0 + 8 <= n ? 8u : (i0 < n ? n - i0 : 0u);
	if (nv < 8) {
#pragma unroll
		for (int h = 0; h < 4; h++) {
			if (nv <= (uint32_t) (2 * h))
				r[h] = 0;
			else if (nv == (uint32_t) (2 * h + 1))
				r[h] &= 0xFFFFu;
		}
	}
	if (ored)
		*ored |= r[0] | r[1] | r[2] | r[3];
	const uint32_t raw_w = r[3];
	uint32_t c = carry;
	if (q) {
		const s16x2 qq = { (short) q, (short) q };
#pragma unroll
		for (int h = 0; h < 4; h++)
			r[h] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(s16x2, r[h]) >> qq);
		c = __builtin_bit_cast(uint32_t, __builtin_bit_cast(s16x2, c) >> qq);
	}
	const uint32_t pw = prev_lane(r[3], c);
	uint32_t zz[4];
	zz[0] = zd_pair(r[0], pw);
	zz[1] = zd_pair(r[1], r[0]);
	zz[2] = zd_pair(r[2], r[1]);
	zz[3] = zd_pair(r[3], r[2]);
	carry = (uint32_t) __builtin_amdgcn_readlane((int) raw_w, 63);
	if (nv < 8) { // deltas of samples beyond n are garbage
#pragma unroll
		for (int h = 0; h < 4; h++) {
			if (nv <= (uint32_t) (2 * h))
				zz[h] = 0;
			else if (nv == (uint32_t) (2 * h + 1))
				zz[h] &= 0xFFFFu;
		}
	}
	return make_uint4(zz[0], zz[1], zz[2], zz[3]);
}

// ex-zd: does any read of the batch need the second scan (all samples divisible by 2^q, q > 0)?
__global__ __launch_bounds__(256) void k_ex_redo_flag(BatchArgs a)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r < a.nreads && a.nsamp[r] && !(a.meta[r].ored & 1u))
		atomicOr(&a.ctl->pad0[0], 1u);
}

// Pass A.  Nothing chains the chunks here: every workgroup streams its chunk once (four sub-tiles
// in flight per wave) and leaves, per wave quarter, the number of exceptions and the sub-tiles that
// hold one in the chunk descriptor; k_ex_prefix turns the counts into ranks and k_ex_list
// writes the (few) exceptions at their final rank from the flagged sub-tiles alone.
// HUFF: also the number of Huffman code bits of every wave quarter (ChunkBits), which lets
// k_huff_encode_chunked place its bits without any chain either.
// Waves per SIMD the register allocator is asked to leave room for (measured: pass A is slower at 8 - a spill -,
// the Huffman encoder 16 % faster - 38 instead of 76 registers then, 62 now that it holds two groups of HENC_G
// sub-tiles, still without a spill; the svb and one-byte kernels are slower with any hint: they stream, and the
// registers hold their loads in flight).
#ifndef SCAN_WAVES
#define SCAN_WAVES 4
#endif
#ifndef HENC_WAVES
#define HENC_WAVES 8
#endif
// Sub-tiles of the Huffman encoder behind one full vector-memory wait (a divisor of CK; two groups of them are held in
// registers: 62 at 4, and 64 is what HENC_WAVES leaves) - see k_huff_encode_chunked
#ifndef HENC_G
#define HENC_G 4
#endif
template <bool REDO, bool HUFF = false>
__global__ __launch_bounds__(CWG, SCAN_WAVES) void k_ex_scan_chunked(BatchArgs a)
{
	// code length of every one-byte value, 1 << 16 for a value without a code; [256] = 0: what a sample that
	// is no one-byte value (exception, sample 0, outside the read) looks up
	__shared__ uint32_t s_len[HUFF ? 257 : 1];
	if (REDO && uni(a.ctl->pad0[0]) == 0)
		return; // no read of this batch has q > 0 (the common case)
	const uint32_t t = blockIdx.x;
	if (t >= uni(a.ctl->nchunks))
		return;
	const int lane = threadIdx.x & 63;
	const int w = (int) uni(threadIdx.x >> 6);
	if (HUFF) {
		const uint32_t l = a.huff->enc[threadIdx.x] >> 24;
		s_len[threadIdx.x] = l ? l : 0x10000u;
		if (threadIdx.x == 0)
			s_len[256] = 0;
		__syncthreads();
	}
	ChunkDesc *dp = a.chunks + t;
	const ChunkU d = load_chunk(dp);
	const uint32_t n = d.n;
	const uint32_t first = d.j * CHUNK;
	ReadMeta *m = a.meta + d.read;
	int q = 0;
	if (REDO) {
		const uint32_t ored = uni(m->ored);
		// ex_zd.c:358-381: largest q <= 5 with every sample divisible by 2^q
		while (q < 5 && !((ored >> q) & 1u))
			q++;
		if (q == 0)
			return; // nothing to redo for this read
	}
	const int16_t *in = a.sig + d.sig_off;
	const uint32_t ws = first + w * WAVE_SAMPLES;
	if (ws >= n) { // the descriptor's counts are zero already
		if (HUFF && lane == 0)
			a.cbits[t].q[w] = 0;
		return;
	}

	uint32_t kmask = 0, etot = 0, ored32 = 0, zd0 = 0, lbits = 0, nocode = 0;
	uint4 raw[4];
#pragma unroll
	for (int k = 0; k < 4; k++)
		raw[k] = sub_load(in, n, ws + k * SUB + lane * 8);
	// the sample in front of the sub-tile: asked for BEHIND the first sub-tiles (in front of them, its shift made the
	// wave wait for this one load before it issued any of the others: one more memory round trip per quarter)
	uint32_t carry = 0, c16 = 0;
	if (ws > 0)
		c16 = (uint32_t) (uint16_t) in[ws - 1]; // (shifted into place behind the next group's loads)
#pragma unroll 1
	for (int kk = 0; kk < CK; kk += 4) {
		uint4 nxt[4];
#pragma unroll
		for (int k = 0; k < 4; k++)
			nxt[k] = kk + 4 + k < CK ? sub_load(in, n, ws + (kk + 4 + k) * SUB + lane * 8) : make_uint4(0, 0, 0, 0);
		if (kk == 0) {
			asm volatile("" : "+v"(c16)); // (keeps the shift - and the wait for the load - here)
			carry = c16 << 16;
		}
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const uint32_t i0 = ws + (kk + k) * SUB + lane * 8;
			const uint4 z = sub_zd(raw[k], n, i0, carry, q, &ored32);
			if (kk + k == 0)
				zd0 = z.x & 0xFFFFu; // lane 0 of the read's first quarter: zd[0]
			uint32_t hi = (z.x | z.y | z.z | z.w) & 0xFF00FF00u;
			if (i0 == 0)
				hi = ((z.x & 0xFF000000u) | ((z.y | z.z | z.w) & 0xFF00FF00u));
			const bool anyex = __ballot(hi != 0) != 0;
			if (anyex) {
				kmask |= 1u << (kk + k);
				const uint32_t inc = wave_incl_scan_dpp(__popc(exc_mask(z, i0)));
				etot += (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
			}
			if (HUFF) { // code lengths of the one-byte values: samples [1, n) that are no exceptions
				const uint32_t zz[4] = { z.x, z.y, z.z, z.w };
				const uint32_t sub0 = ws + (kk + k) * SUB;
				if (!anyex && sub0 != 0 && sub0 + SUB <= n) {
					// a sub-tile of one-byte values only (nearly all are): no mask, no select per sample
#pragma unroll
					for (int h = 0; h < 8; h++)
						lbits += s_len[(zz[h >> 1] >> (16 * (h & 1))) & 0xFFu];
				} else {
					const uint32_t lowm = low_mask(z, i0, n);
#pragma unroll
					for (int h = 0; h < 8; h++) // (a lane sums 128 values of at most 24 bits: below 1 << 16)
						lbits += s_len[((lowm >> h) & 1u) ? ((zz[h >> 1] >> (16 * (h & 1))) & 0xFFu) : 256u];
				}
			}
		}
#pragma unroll
		for (int k = 0; k < 4; k++)
			raw[k] = nxt[k];
	}
	if (HUFF) {
		if (lbits >> 16)
			nocode = 0x80000000u; // a value the table has no code for: the read fails (k_ex_section)
		lbits &= 0xFFFFu;
		const uint32_t inc = wave_incl_scan_dpp(lbits);
		if (lane == 63)
			a.cbits[t].q[w] = inc;
	}
	if (!REDO) { // OR of the raw samples (qts), one atomic per wave; bit 31: a value without a Huffman code
		uint32_t o = ((ored32 | (ored32 >> 16)) & 0xFFFFu) | (HUFF ? nocode : 0u);
#pragma unroll
		for (int dd = 32; dd >= 1; dd >>= 1)
			o |= (uint32_t) __shfl_xor((int) o, dd, 64);
		if (lane == 0)
			atomicOr(&m->ored, o);
	}
	if (lane == 0) {
		dp->ecnt[w] = etot;
		dp->kmask[w] = (uint16_t) kmask;
		if (ws == 0)
			m->zd0 = zd0;
	}
}

// exceptions in front of every chunk (one thread per read); the read's total and its ex-zd shift
__global__ __launch_bounds__(256) void k_ex_prefix(BatchArgs a, int exzd)
{
	// one wave per read (a thread per read walked the 175 chunks of the longest read one after the other)
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63;
	if (r >= a.nreads)
		return;
	const uint32_t n = a.nsamp[r];
	if (n == 0)
		return;
	ReadMeta *m = a.meta + r;
	ChunkDesc *dp = a.chunks + a.first_chunk[r];
	const uint32_t nch = (n + CHUNK - 1) / CHUNK;
	// exclusive prefix of a 64-bit count over the chunks, 64 at a time; returns the total
	auto scan = [&](auto count_of, auto store) -> uint64_t {
		uint64_t carry = 0;
		for (uint32_t j0 = 0; j0 < nch; j0 += 64) {
			const uint32_t j = j0 + lane;
			const uint64_t c = j < nch ? count_of(j) : 0ull;
			// (two 32-bit scans, of the counts' low 20 bits and of the rest: neither can overflow over 64 chunks)
			const uint32_t lo = wave_incl_scan_dpp((uint32_t) (c & 0xFFFFFu)), hi = wave_incl_scan_dpp((uint32_t) (c >> 20));
			const uint64_t inc = (uint64_t) lo + ((uint64_t) hi << 20);
			if (j < nch)
				store(j, carry + inc - c);
			const uint64_t tot = (uint64_t) (uint32_t) __builtin_amdgcn_readlane((int) lo, 63) +
					     ((uint64_t) (uint32_t) __builtin_amdgcn_readlane((int) hi, 63) << 20);
			carry += tot;
		}
		return carry;
	};
	const uint64_t e = scan([&](uint32_t j) { return (uint64_t) dp[j].ecnt[0] + dp[j].ecnt[1] + dp[j].ecnt[2] + dp[j].ecnt[3]; },
				[&](uint32_t j, uint64_t v) { dp[j].ebefore = v; });
	if (a.cbits) { // Huffman code bits in front of every chunk
		ChunkBits *cb = a.cbits + a.first_chunk[r];
		(void) scan([&](uint32_t j) { return (uint64_t) cb[j].q[0] + cb[j].q[1] + cb[j].q[2] + cb[j].q[3]; },
			    [&](uint32_t j, uint64_t v) { cb[j].before = v; });
	}
	if (lane == 0) {
		m->nex = (uint32_t) e;
		uint32_t q = 0;
		if (exzd) { // ex_zd.c:358-381
			const uint32_t ored = m->ored;
			while (q < 5 && !((ored >> q) & 1u))
				q++;
		}
		m->q = q;
	}
}

// the exception list (position, value) at its final rank: only the flagged sub-tiles are read again
__global__ __launch_bounds__(CWG) void k_ex_list(BatchArgs a)
{
	// one WAVE per chunk (its four quarters one after the other: nearly all of them hold no exception) - a
	// workgroup per chunk meant 150 000 waves that read a descriptor and left
	const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (t >= uni(a.ctl->nchunks))
		return;
	const int lane = threadIdx.x & 63;
	const ChunkDesc *dp = a.chunks + t;
	const uint32_t km[4] = { uni(dp->kmask[0]), uni(dp->kmask[1]), uni(dp->kmask[2]), uni(dp->kmask[3]) };
	if (!(km[0] | km[1] | km[2] | km[3]))
		return;
	const ChunkU d = load_chunk(dp);
	const uint32_t n = d.n;
	const int q = (int) uni(a.meta[d.read].q);
	const int16_t *in = a.sig + d.sig_off;
	uint32_t *lpos = a.ex_pos + d.sig_off;
	uint32_t *lval = a.ex_val + d.sig_off;
	const uint32_t cnt[4] = { uni(dp->ecnt[0]), uni(dp->ecnt[1]), uni(dp->ecnt[2]), uni(dp->ecnt[3]) };
	uint32_t rank = (uint32_t) uni64(dp->ebefore);
#pragma unroll
	for (int w = 0; w < 4; w++) {
		const uint32_t ws = d.j * CHUNK + w * WAVE_SAMPLES;
		uint32_t rk = rank;
		for (uint32_t mm = km[w]; mm; mm &= mm - 1) {
			const uint32_t k = (uint32_t) __builtin_ctz(mm);
			const uint32_t sub0 = ws + k * SUB;
			const uint32_t i0 = sub0 + lane * 8;
			uint32_t carry = sub0 ? (uint32_t) (uint16_t) in[sub0 - 1] << 16 : 0u;
			const uint4 z = sub_zd(sub_load(in, n, i0), n, i0, carry, q);
			const uint32_t em = exc_mask(z, i0);
			const uint32_t c = __popc(em);
			const uint32_t inc = wave_incl_scan_dpp(c);
			uint32_t p = rk + inc - c;
			const uint32_t zz[4] = { z.x, z.y, z.z, z.w };
			if (em) {
#pragma unroll
				for (int h = 0; h < 8; h++) {
					if ((em >> h) & 1u) {
						lpos[p] = i0 + h - 1;
						lval[p] = (zz[h >> 1] >> (16 * (h & 1))) & 0xFFFFu;
						p++;
					}
				}
			}
			rk += (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
		}
		rank += cnt[w];
	}
}

// Pass B, plain one-byte stream (press.c:2717-2725): one workgroup per chunk, any order.
// HIST (zstd_hasgam_vbsse21_zdq, press_zstd.hip): the bytes are counted per read while a lane holds them, as in
// k_svb_encode_chunked<.., HIST> (BatchArgs::zhist).
template <bool HIST = false>
__global__ __launch_bounds__(CWG) void k_low_encode_chunked(BatchArgs a)
{
	__shared__ uint32_t s_hist[HIST ? 16 : 1][256];
	const uint32_t t = blockIdx.x;
	if (t >= a.ctl->nchunks)
		return;
	const ChunkDesc *dp = a.chunks + t;
	const ChunkU d = load_chunk(dp);
	const ReadMeta *m = a.meta + d.read;
	if (uni(m->status))
		return; // out_len = FAILED was written by k_ex_section
	const uint32_t n = d.n;
	const int lane = threadIdx.x & 63;
	const int w = (int) uni(threadIdx.x >> 6);
	const uint32_t ws = d.j * CHUNK + w * WAVE_SAMPLES;
	uint32_t *myhist = s_hist[HIST ? 4 * w + (lane & 3) : 0];
	if (HIST) {
		for (int i = 0; i < 16; i++)
			s_hist[i][threadIdx.x] = 0;
		__syncthreads();
	}
	if (ws < n) {
	const int q = (int) uni(m->q);
	const int16_t *in = a.sig + d.sig_off;
	// one-byte value of sample i (i >= 1) goes to stream[(i - 1) - #exceptions before i]
	uint8_t *stream = a.low_tmp ? a.low_tmp + d.sig_off : a.out + d.out_base + uni(m->hdr) + uni(m->seclen);
	const uint32_t e0 = uni(dp->ecnt[0]), e1 = uni(dp->ecnt[1]), e2 = uni(dp->ecnt[2]);
	uint64_t eb = uni64(dp->ebefore) + (w > 0 ? e0 : 0u) + (w > 1 ? e1 : 0u) + (w > 2 ? e2 : 0u);

	uint4 z[CK];
	uint32_t ored;
	quarter_zd(in, n, ws, lane, q, z, ored);
#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		const uint32_t sub0 = ws + k * SUB;
		if (sub0 >= n)
			continue;
		uint32_t hi = (z[k].x | z[k].y | z[k].z | z[k].w) & 0xFF00FF00u;
		const bool special = (i0 == 0) || (i0 < n && i0 + 8 > n); // sample 0 / ragged tail
		if (!__ballot(hi != 0 || special)) {
			// no exception in the sub-tile: 8 low bytes per lane, one (unaligned) store
			if (i0 < n) {
				uint2 v;
				v.x = __builtin_amdgcn_perm(z[k].y, z[k].x, 0x06040200);
				v.y = __builtin_amdgcn_perm(z[k].w, z[k].z, 0x06040200);
				__builtin_memcpy(stream + (i0 - 1 - eb), &v, 8);
				if (HIST) {
#pragma unroll
					for (int e = 0; e < 4; e++) {
						atomicAdd(&myhist[(v.x >> (8 * e)) & 0xFFu], 1u);
						atomicAdd(&myhist[(v.y >> (8 * e)) & 0xFFu], 1u);
					}
				}
			}
			continue;
		}
		const uint32_t em = exc_mask(z[k], i0);
		const uint32_t c = __popc(em);
		const uint32_t inc = wave_incl_scan_dpp(c);
		const uint32_t nv = i0 < n ? min(8u, n - i0) : 0u;
		const uint32_t zz[4] = { z[k].x, z[k].y, z[k].z, z[k].w };
		// first stream index of this lane: samples before i0 minus sample 0 minus exceptions
		uint64_t p = (uint64_t) (i0 ? i0 - 1 : 0) - (eb + inc - c);
#pragma unroll
		for (int h = 0; h < 8; h++) {
			if ((uint32_t) h < nv && !((em >> h) & 1u) && !(i0 == 0 && h == 0)) {
				const uint32_t b = (zz[h >> 1] >> (16 * (h & 1))) & 0xFFu;
				stream[p++] = (uint8_t) b;
				if (HIST)
					atomicAdd(&myhist[b], 1u);
			}
		}
		eb += (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
	}
	} // (a wave whose quarter lies behind the read's end has nothing to write)
	if (HIST) {
		__syncthreads();
		uint32_t c = 0;
		for (int i = 0; i < 16; i++)
			c += s_hist[i][threadIdx.x];
		if (c)
			atomicAdd(&a.zhist[(uint64_t) d.read * 256 + threadIdx.x], c);
	}
}

// Pass B, static-Huffman stream (huffman.c:1184 + do_memory_encode :848: the codes packed
// from bit 0 of each byte upwards - a little-endian bit stream).  One workgroup per chunk in any
// order, its four waves independent of each other: pass A has counted the code bits of every
// wave quarter (k_ex_scan_chunked<.., true>) and k_ex_prefix has summed them, so a wave knows the
// bit position Bq of its quarter from the start; it stages the codes of one 512-sample sub-tile
// at a time in a private LDS buffer (LDS atomic OR of code << bitpos) and copies the completed
// dwords out.  No ticket, no look-back, one barrier (the table load).
// Who writes a byte shared by two quarters: the quarter that holds the byte's LAST bit; it
// recomputes the few bits its predecessors put into that byte from the samples in front of
// it.  The last, partial byte of a read and out_len are written by wave 0 of its last chunk.
constexpr int HSTG = 400; // dwords per wave: carried bits (< 32) + 512 codes of at most 24 bits + spill

__device__ __forceinline__ uint32_t zz16_dev(int32_t d)
{
	const int32_t s = (int32_t) (int16_t) d;
	return (uint32_t) ((s << 1) ^ (s >> 15)) & 0xFFFFu;
}

// the last nb (1..7) bits of the code stream of samples [1, end) of a read: all 64 lanes call
// it, every lane gets the value.  enc: the code table in LDS.
__device__ __forceinline__ uint32_t huff_tail_bits(const int16_t *in, uint32_t end, uint32_t nb, const uint32_t *enc,
						   int lane)
{
	uint32_t acc = 0, got = 0;
	uint32_t pos = end; // samples [1, pos) are still to be looked at
	while (got < nb && pos > 1) {
		const int64_t i = (int64_t) pos - 64 + lane;
		const bool valid = i >= 1;
		uint32_t zv = 0xFFFFu;
		if (valid)
			zv = zz16_dev((int32_t) in[i] - (int32_t) in[i - 1]);
		unsigned long long mask = __ballot(valid && zv <= 255u);
		while (mask && got < nb) {
			const int l = 63 - __builtin_clzll(mask);
			const uint32_t e = enc[(uint32_t) __builtin_amdgcn_readlane((int) zv, l)];
			const uint32_t len = e >> 24;
			acc = (acc << len) | (e & 0xFFFFFFu); // an earlier value's code sits below the later ones
			got += len;
			mask &= ~(1ull << l);
		}
		pos = pos > 64 ? pos - 64 : 0;
	}
	return got >= nb ? (acc >> (got - nb)) & ((1u << nb) - 1u) : acc;
}


__global__ __launch_bounds__(CWG, HENC_WAVES) void k_huff_encode_chunked(BatchArgs a)
{
	__shared__ uint32_t enc[257]; // [256] = 0: what a sample without a code (exception, outside the read) looks up
	__shared__ uint32_t stg_all[4][HSTG];

	enc[threadIdx.x] = a.huff->enc[threadIdx.x];
	if (threadIdx.x == 0)
		enc[256] = 0;
	for (uint32_t i = threadIdx.x; i < 4u * HSTG; i += CWG)
		(&stg_all[0][0])[i] = 0;
	__syncthreads(); // the only barrier
	const uint32_t t = blockIdx.x;
	if (t >= uni(a.ctl->nchunks))
		return;
	const int lane = threadIdx.x & 63;
	const int w = (int) uni(threadIdx.x >> 6);
	uint32_t *stg = stg_all[w];
	const ChunkDesc *dp = a.chunks + t;
	const ChunkU d = load_chunk(dp);
	const ReadMeta *m = a.meta + d.read;
	if (uni(m->status))
		return; // out_len = FAILED was written by k_ex_section
	const uint32_t n = d.n;
	const uint32_t first = d.j * CHUNK;
	const bool last = first + CHUNK >= n;
	const uint32_t ws = first + w * WAVE_SAMPLES;
	const int16_t *in = a.sig + d.sig_off;
	const uint32_t head = uni(m->hdr) + uni(m->seclen) + 4; // bytes in front of the payload
	uint8_t *payload = a.out + d.out_base + head;
	const uint64_t cap = uni64(a.out_off[d.read + 1]) - d.out_base;
	// code bits of the quarters and in front of the chunk: k_ex_scan_chunked<.., true> + k_ex_prefix
	const ChunkBits *cb = a.cbits + t;
	const uint32_t q0 = uni(cb->q[0]), q1 = uni(cb->q[1]), q2 = uni(cb->q[2]), q3 = uni(cb->q[3]);
	const uint64_t before = uni64(cb->before);
	if (w == 0 && last) { // the read ends here: its length and its last, partial byte (zero padded, huffman.c:878)
		const uint64_t bits = before + q0 + q1 + q2 + q3;
		const uint64_t total = (uint64_t) head + (bits + 7) / 8;
		const uint32_t nbt = (uint32_t) bits & 7u;
		if (total <= cap && nbt) {
			const uint32_t tb = huff_tail_bits(in, n, nbt, enc, lane);
			if (lane == 0)
				payload[bits >> 3] = (uint8_t) tb;
		}
		if (lane == 0)
			a.out_len[d.read] = total <= cap ? total : CFAIL64;
	}
	const uint32_t mybits = w == 0 ? q0 : w == 1 ? q1 : w == 2 ? q2 : q3;
	const uint64_t Bq = before + (w > 0 ? q0 : 0u) + (w > 1 ? q1 : 0u) + (w > 2 ? q2 : 0u);
	// a quarter that would run past the slot writes nothing - the read fails
	if (ws >= n || !mybits || (uint64_t) head + (Bq + mybits + 7) / 8 > cap)
		return;
	// the nb bits in front of Bq that share its byte
	const uint32_t nb = (uint32_t) Bq & 7u;
	if (nb) {
		const uint32_t tb = huff_tail_bits(in, ws, nb, enc, lane);
		if (lane == 0)
			stg[0] = tb;
	}
	uint8_t *g = payload + (Bq >> 3); // byte of staging bit 0
	uint32_t fill = nb;               // bits waiting at the front of the staging buffer
	wave_lds_sync();
	// HENC_G sub-tiles to a group.  Between a sample load and its use lie the copy-out loops with a number of stores
	// the compiler cannot count, so what it puts in front of the samples' first use is s_waitcnt vmcnt(0) - a wait for
	// everything, the stores' acknowledgements included (on gfx950 stores count in vmcnt, in order).  With a sub-tile
	// per wait a wave had 1 KB behind every memory round trip and a prefetch overlapped nothing (3.5 TB/s of samples);
	// now one wait per group covers HENC_G KB, and the other sub-tiles of the group, in front of which no load is
	// issued, wait for no vector memory at all.
	static_assert(CK % HENC_G == 0, "a quarter is a whole number of groups");
	uint4 raw[HENC_G];
#pragma unroll
	for (int gi = 0; gi < HENC_G; gi++)
		raw[gi] = sub_load(in, n, ws + gi * SUB + lane * 8);
	// the sample in front of the sub-tile (behind the loads above: see k_ex_scan_chunked)
	uint32_t carry = ws > 0 ? (uint32_t) (uint16_t) in[ws - 1] << 16 : 0u;
#pragma unroll 1
	for (int kg = 0; kg < CK; kg += HENC_G) {
		if (ws + kg * SUB >= n)
			break;
		uint4 cur[HENC_G];
		// wait first: the empty asm takes the group's samples out of the load registers - they were asked for a group
		// ago and have landed, what the wait pays for is the acknowledgement of the last sub-tile's stores -, then the
		// next group's loads go out and have a whole group's work to arrive.  (The other order - issue the next
		// group's loads, then use this one, as pass A does - makes the same wait cover the loads just issued:
		// measured at this order's time or 20 us above it, never below)
#pragma unroll
		for (int gi = 0; gi < HENC_G; gi++) {
			typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
			u32x4 t = { raw[gi].x, raw[gi].y, raw[gi].z, raw[gi].w };
			asm volatile("" : "+v"(t));
			cur[gi] = make_uint4(t.x, t.y, t.z, t.w);
		}
#pragma unroll
		for (int gi = 0; gi < HENC_G; gi++)
			raw[gi] = kg + HENC_G < CK ? sub_load(in, n, ws + (kg + HENC_G + gi) * SUB + lane * 8) : make_uint4(0, 0, 0, 0);
#pragma unroll
		for (int gi = 0; gi < HENC_G; gi++) {
			const uint32_t sub0 = ws + (kg + gi) * SUB;
			if (sub0 >= n)
				break;
			const uint32_t i0 = sub0 + lane * 8;
			const uint4 z = sub_zd(cur[gi], n, i0, carry);
			const uint32_t zz[4] = { z.x, z.y, z.z, z.w };
			uint32_t e[8];
			uint32_t lb = 0;
			if (sub0 != 0 && sub0 + SUB <= n && !__ballot(((z.x | z.y | z.z | z.w) & 0xFF00FF00u) != 0)) {
				// a sub-tile of one-byte values only (nearly all are): no mask, no select per sample
#pragma unroll
				for (int h = 0; h < 8; h++) {
					e[h] = enc[(zz[h >> 1] >> (16 * (h & 1))) & 0xFFu];
					lb += e[h] >> 24;
				}
			} else {
				const uint32_t lowm = low_mask(z, i0, n);
#pragma unroll
				for (int h = 0; h < 8; h++) {
					e[h] = enc[((lowm >> h) & 1u) ? ((zz[h >> 1] >> (16 * (h & 1))) & 0xFFu) : 256u];
					lb += e[h] >> 24;
				}
			}
			const uint32_t inc = wave_incl_scan_dpp(lb);
			const uint32_t tot = (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
			uint32_t pos = fill + inc - lb;
			if (lb <= 64) {
				// the lane's codes side by side in two registers (8 codes of the NA12878 table: 43 bits on
				// average, more than 64 in one lane of 700), then at most three LDS atomics
				uint64_t acc = 0;
				uint32_t o = 0;
#pragma unroll
				for (int h = 0; h < 8; h++) {
					acc |= (uint64_t) (e[h] & 0xFFFFFFu) << o;
					o += e[h] >> 24;
				}
				const uint32_t sh = pos & 31u;
				const uint64_t lo2 = acc << sh;
				const uint32_t w2 = sh ? (uint32_t) (acc >> 32) >> (32u - sh) : 0u;
				if ((uint32_t) lo2)
					atomicOr(&stg[pos >> 5], (uint32_t) lo2);
				if ((uint32_t) (lo2 >> 32))
					atomicOr(&stg[(pos >> 5) + 1], (uint32_t) (lo2 >> 32));
				if (w2)
					atomicOr(&stg[(pos >> 5) + 2], w2);
			} else {
#pragma unroll
				for (int h = 0; h < 8; h++) {
					if (e[h]) {
						const uint64_t wv = (uint64_t) (e[h] & 0xFFFFFFu) << (pos & 31u);
						if ((uint32_t) wv)
							atomicOr(&stg[pos >> 5], (uint32_t) wv);
						if ((uint32_t) (wv >> 32))
							atomicOr(&stg[(pos >> 5) + 1], (uint32_t) (wv >> 32));
						pos += e[h] >> 24;
					}
				}
			}
			wave_lds_sync();
			// completed dwords out (unaligned 4-byte stores), the partial one to the front
			const uint32_t total = fill + tot;
			const uint32_t nfull = total >> 5;
			for (uint32_t c = (uint32_t) lane; c < nfull; c += 64) {
				const uint32_t v = stg[c];
				stg[c] = 0;
				__builtin_memcpy(g + 4ull * c, &v, 4);
			}
			if (nfull && lane == 0) {
				const uint32_t tl = stg[nfull];
				stg[nfull] = 0;
				stg[0] = tl;
			}
			g += 4ull * nfull;
			fill = total & 31u;
			wave_lds_sync();
		}
	}
	// whole bytes that are left; a partial last byte belongs to whoever holds its last bit
	if (lane == 0) {
		const uint32_t v = stg[0];
		for (uint32_t b = 0; b < (fill >> 3); b++)
			g[b] = (uint8_t) (v >> (8 * b));
	}
}

// ------------------------------------------------------------------ exception split decode, chunked
//
// Second half of vbe21_depress and siblings (press.c:2757-2771) fused with unzigdelta_u16_16
// (trans.c:260), after k_ex_parse has produced the sorted exception list (and, for the
// Huffman variants, k_huff_decode_tiles the one-byte stream).  Sample i >= 1 is exception e
// if pos[e] == i-1, otherwise one-byte value number (i-1) - #exceptions before it; so a
// chunk finds its place in the stream by binary search - only the running sample value
// needs the look-back chain.

// chunk table from the parsed streams: n = 1 + nlow + nex samples per read (hread: the Huffman decoder's
// per-read record - reads it has finished itself get no chunks)
__global__ __launch_bounds__(256) void k_chunk_prep_meta(const uint64_t *off, const uint64_t *in_off,
							 const ReadMeta *meta, uint32_t nreads, ChunkDesc *chunks,
							 uint64_t *gran, ChunkCtl *ctl, uint32_t max_chunks,
							 uint32_t *out_n, const uint32_t *hread, const uint32_t *ex_pos)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	uint32_t n = 0, nch = 0;
	if (r < nreads && !meta[r].status) {
		const uint32_t nex = meta[r].nex;
		n = 1u + meta[r].nlow + nex;
		nch = (n + CHUNK - 1) / CHUNK;
		if (hread && (hread[2 * r + 1] & HUF_FUSED))
			nch = 0; // k_huf_emit wrote this read's samples already
		// a Huffman payload that ran out early delivered fewer values than k_ex_parse tested the positions against:
		// the read stands only if its last exception is still reached, pos[nex - 1] + 1 <= nlow + nex.  (A fused read
		// has passed this very test: k_huf_chain sets HUF_FUSED only under pos[nex - 1] < nlow + nex with the same
		// nlow, so the two branches are complementary - change one and the other has to follow.)
		else if (hread && nex && (uint64_t) ex_pos[off[r] + nex - 1] + 1 > (uint64_t) meta[r].nlow + nex)
			n = nch = 0;
	}
	const uint32_t inc = scan32(nch, threadIdx.x & 63);
	uint32_t base = 0;
	if ((threadIdx.x & 63) == 63 && inc)
		base = atomicAdd(&ctl->nchunks, inc);
	base = (uint32_t) __builtin_amdgcn_readlane((int) base, 63);
	const uint32_t first = base + inc - nch;
	if (r >= nreads)
		return;
	out_n[r] = n ? n : CFAIL32;
	for (uint32_t j = 0; j < nch && first + j < max_chunks; j++) {
		ChunkDesc d;
		d.sig_off = off[r];
		d.out_base = in_off[r];
		d.n = n;
		d.j = j;
		d.read = r;
		d.cap_ok = 1;
		d.ebefore = 0;
		d.ecnt[0] = d.ecnt[1] = d.ecnt[2] = d.ecnt[3] = 0;
		d.kmask[0] = d.kmask[1] = d.kmask[2] = d.kmask[3] = 0;
		chunks[first + j] = d;
		gran[first + j] = 0;
	}
}

__device__ __forceinline__ uint32_t lower_bound_dev(const uint32_t *p, uint32_t n, uint32_t key)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (p[mid] < key)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// Exceptions in front of every wave quarter of every chunk (ChunkDesc::ebefore / ecnt): five
// binary searches of the read's sorted position list per chunk, one lane each - here they
// run a hundred thousand at a time instead of in front of the data loads of
// k_low_decode_chunked (22 dependent round trips per wave).
__global__ __launch_bounds__(256) void k_ex_ranks(DecodeArgs a)
{
	const uint32_t g = blockIdx.x * 256 + threadIdx.x;
	const uint32_t c = g >> 3, l = g & 7u;
	uint32_t b = 0;
	const bool act = c < a.ctl->nchunks && c < a.max_chunks;
	if (act && l < 5) {
		const ChunkDesc *dp = a.chunks + c;
		const uint32_t n = dp->n;
		const uint32_t ws = dp->j * CHUNK + l * WAVE_SAMPLES; // l = 4: the end of the chunk
		const uint32_t upto = ws < n ? ws : n;                // exceptions among samples [1, upto)
		b = lower_bound_dev(a.ex_pos + dp->sig_off, a.meta[dp->read].nex, upto ? upto - 1 : 0);
	}
	const uint32_t nxt = (uint32_t) __shfl_down((int) b, 1, 64);
	if (act && l < 4) {
		ChunkDesc *dp = a.chunks + c;
		dp->ecnt[l] = nxt - b;
		if (l == 0)
			dp->ebefore = b;
	}
}

// slow path of one sub-tile: values of the lane's 8 samples, exceptions merged in.  The
// exceptions of the sub-tile are pos[e_first, e_first + e_cnt): the search stays inside them.
__device__ __forceinline__ void gather_low(const uint8_t *low, uint32_t nlow, const uint32_t *pos,
					   const uint32_t *val, uint32_t nex, uint32_t zd0, uint32_t i0,
					   uint32_t n, uint32_t e_first, uint32_t e_cnt, uint32_t v[4])
{
	v[0] = v[1] = v[2] = v[3] = 0;
	if (i0 >= n)
		return;
	const uint32_t nv = min(8u, n - i0);
	const uint32_t uf = i0 ? i0 - 1 : 0;
	uint32_t e = e_first + lower_bound_dev(pos + e_first, e_cnt, uf);
	uint32_t l = uf - e; // index of the next one-byte value
	uint32_t nextpos = e < nex ? pos[e] : 0xFFFFFFFFu;
#pragma unroll
	for (int h = 0; h < 8; h++) {
		if ((uint32_t) h < nv) {
			const uint32_t i = i0 + h;
			uint32_t z;
			if (i == 0) {
				z = zd0;
			} else if (i - 1 == nextpos) {
				z = val[e] & 0xFFFFu;
				e++;
				nextpos = e < nex ? pos[e] : 0xFFFFFFFFu;
			} else {
				z = l < nlow ? low[l] : 0u;
				l++;
			}
			v[h >> 1] |= z << (16 * (h & 1));
		}
	}
}

// HUFF: the one-byte values come from a.low (entropy decoders); the grid may then be smaller than the
// number of chunks (workgroups keep taking tickets)
template <bool HUFF>
__global__ __launch_bounds__(CWG) void k_low_decode_chunked(DecodeArgs a)
{
	__shared__ uint32_t s_ticket;
	__shared__ uint32_t s_wsum[4];
	__shared__ uint32_t s_sbase;
	__shared__ uint16_t s_xl[4][CK][64];
	__shared__ uint32_t s_sub[4][CK];  // delta total / base per sub-tile
	__shared__ uint32_t s_cnt[4][CK];  // exceptions per sub-tile, then their exclusive prefix
	__shared__ uint32_t s_km[4];

	const int lane = threadIdx.x & 63;
	const int w = (int) uni(threadIdx.x >> 6);
#ifdef DEC_STAMPS
	const uint64_t t_start = __builtin_amdgcn_s_memtime();
#endif
	if (HUFF && uni(a.ctl->nchunks) == 0)
		return; // (every read's samples were written by k_huf_emit: no tickets to draw)
	for (;;) {
	if (threadIdx.x == 0)
		s_ticket = atomicAdd(&a.ctl->ticket, 1u);
	if (lane < CK)
		s_cnt[w][lane] = 0;
	if (lane == 0)
		s_km[w] = 0;
	__syncthreads();
	const uint32_t t = uni(s_ticket);
	if (t >= a.ctl->nchunks)
		return;
#ifdef DEC_STAMPS
	if (threadIdx.x == 0 && t < 65536)
		g_stamps[t * 8 + 0] = t_start;
#endif
	STAMP(1);
	const ChunkU d = load_chunk(a.chunks + t);
	const uint32_t n = d.n;
	const uint32_t first = d.j * CHUNK;
	const bool last = first + CHUNK >= n;
	const ReadMeta *m = a.meta + d.read;
	const uint32_t nex = uni(m->nex), nlow = uni(m->nlow), zd0 = uni(m->zd0);
	const int q = (int) uni(m->q);
	const uint32_t *pos = a.ex_pos + d.sig_off;
	const uint32_t *val = a.ex_val + d.sig_off;
	const uint8_t *low = HUFF ? a.low + d.sig_off : a.in + d.out_base + uni(m->hdr) + uni(m->seclen);
	int16_t *out = a.sig + d.sig_off;
	const uint32_t ws = first + w * WAVE_SAMPLES;
	const uint32_t nsub = ws >= n ? 0u : min((uint32_t) CK, (n - ws + SUB - 1) / SUB);
	const uint32_t live = (1u << nsub) - 1u;

	// ---- exceptions of this wave's quarter (ranks from k_ex_ranks): which sub-tiles hold one,
	// how many before each
	const ChunkDesc *dp = a.chunks + t;
	const uint32_t c0 = uni(dp->ecnt[0]), c1 = uni(dp->ecnt[1]), c2 = uni(dp->ecnt[2]), c3 = uni(dp->ecnt[3]);
	const uint32_t ew = w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
	const uint32_t e_lo = (uint32_t) uni64(dp->ebefore) + (w > 0 ? c0 : 0u) + (w > 1 ? c1 : 0u) + (w > 2 ? c2 : 0u);
	if (nsub) {
		const uint32_t e_hi = e_lo + ew;
		for (uint32_t e = e_lo + lane; e < e_hi; e += 64) {
			const uint32_t k = (pos[e] + 1 - ws) / SUB;
			atomicAdd(&s_cnt[w][k], 1u);
			atomicOr(&s_km[w], 1u << k);
		}
	}
	wave_lds_sync();
	uint32_t kmask = uni(s_km[w]);
	if (ws == 0)
		kmask |= 1u; // sample 0 comes from the header
	if ((n & 7) && n > ws && n - ws <= WAVE_SAMPLES)
		kmask |= 1u << ((n - 1 - ws) / SUB); // ragged tail
	if (lane < CK) {
		const uint32_t c = s_cnt[w][lane];
		const uint32_t inc = wave_incl_scan_dpp(c);
		s_cnt[w][lane] = inc - c;
	}
	wave_lds_sync();
	// sub-tiles whose 8-byte windows could reach past the one-byte stream are not plain
#pragma unroll
	for (int k = 0; k < CK; k++)
		if (((live >> k) & 1u) && (uint64_t) ws + k * SUB + SUB + 8 > (uint64_t) nlow + 1 + e_lo)
			kmask |= 1u << k;
	kmask &= live;
	const uint32_t plain = live & ~kmask;
	STAMP(2);

	// ---- phase 1: one-byte values of the plain sub-tiles (8 per lane, any alignment)
	const uint8_t *zeros8 = reinterpret_cast<const uint8_t *>(a.ctl->pad2); // (zeroed with the control block)
	uint2 dat[CK];
#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		// (every sub-tile loads, the ones that are not plain and the lanes behind the read's end zeros from the
		// control block: with the load under a branch or a lane mask the compiler merges the zero and the loaded
		// value in other registers right behind the load and waits for it - these sixteen loads went out one
		// after the other)
		const uint32_t eb = e_lo + uni(s_cnt[w][k]);
		const uint8_t *src = (((plain >> k) & 1u) && i0 < n) ? low + (i0 - 1 - eb) : zeros8;
		const unsigned long long d64 = ld8_stream(src);
		dat[k] = make_uint2((uint32_t) d64, (uint32_t) (d64 >> 32));
	}

	// ---- phase 2: delta sums
#pragma unroll
	for (int k = 0; k < CK; k++) {
		if ((plain >> k) & 1u) {
			uint32_t v[4];
			expand8(dat[k], v);
			uint32_t acc = 0;
#pragma unroll
			for (int h = 0; h < 4; h++)
				acc = pk_add16(acc, unzz_pair(v[h]));
			const uint32_t tot16 = (acc + (acc >> 16)) & 0xFFFFu;
			const uint32_t inc = wave_incl_scan_dpp(tot16);
			s_xl[w][k][lane] = (uint16_t) (inc - tot16);
			if (lane == 63)
				s_sub[w][k] = inc;
		}
	}
	for (uint32_t mm = kmask; mm; mm &= mm - 1) {
		const uint32_t k = (uint32_t) __builtin_ctz(mm);
		uint32_t v[4];
		const uint32_t ef = uni(s_cnt[w][k]);
		const uint32_t ec = (k + 1 < (uint32_t) CK ? uni(s_cnt[w][k + 1 < (uint32_t) CK ? k + 1 : k]) : ew) - ef;
		gather_low(low, nlow, pos, val, nex, zd0, ws + k * SUB + lane * 8, n, e_lo + ef, ec, v);
		uint32_t acc = 0;
#pragma unroll
		for (int h = 0; h < 4; h++)
			acc = pk_add16(acc, unzz_pair(v[h]));
		const uint32_t tot16 = (acc + (acc >> 16)) & 0xFFFFu;
		const uint32_t inc = wave_incl_scan_dpp(tot16);
		s_xl[w][k][lane] = (uint16_t) (inc - tot16);
		if (lane == 63)
			s_sub[w][k] = inc;
	}
	wave_lds_sync();
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
	STAMP(3);
	__syncthreads();
	STAMP(4);
	const uint32_t u0 = uni(s_wsum[0]), u1 = uni(s_wsum[1]), u2 = uni(s_wsum[2]), u3 = uni(s_wsum[3]);
	if (w == 0) {
		const uint32_t sv = (uint32_t) lookback(a.gran, t, d.j, (uint64_t) ((u0 + u1 + u2 + u3) & 0xFFFFu), last);
		if (lane == 0)
			s_sbase = sv;
	}
	__syncthreads();
	STAMP(5);
	const uint32_t sb = uni(s_sbase) + (w > 0 ? u0 : 0u) + (w > 1 ? u1 : 0u) + (w > 2 ? u2 : 0u);

	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
	for (int k = 0; k < CK; k++)
		asm volatile("" : "+v"(dat[k].x), "+v"(dat[k].y));

	// ---- phase 3: values, prefix inside the lane, bases, ex-zd shift, store
	const u16x2 qq = { (unsigned short) q, (unsigned short) q };
#pragma unroll
	for (int k = 0; k < CK; k++) {
		const uint32_t i0 = ws + k * SUB + lane * 8;
		if ((plain >> k) & 1u) {
			uint32_t v[4];
			expand8(dat[k], v);
#pragma unroll
			for (int h = 0; h < 4; h++)
				v[h] = unzz_pair(v[h]);
			(void) lane_prefix8(v);
			const uint32_t b16 = (sb + uni(s_sub[w][k]) + s_xl[w][k][lane]) & 0xFFFFu;
			const uint32_t b2 = b16 | (b16 << 16);
#pragma unroll
			for (int h = 0; h < 4; h++) {
				v[h] = pk_add16(v[h], b2);
				if (q) // ex_zd.c:396 do_rev_qts_inplace
					v[h] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, v[h]) << qq);
			}
			if (i0 < n)
				st16_stream(out + i0, make_uint4(v[0], v[1], v[2], v[3]));
		}
	}
	for (uint32_t mm = kmask; mm; mm &= mm - 1) {
		const uint32_t k = (uint32_t) __builtin_ctz(mm);
		const uint32_t i0 = ws + k * SUB + lane * 8;
		uint32_t v[4];
		const uint32_t ef = uni(s_cnt[w][k]);
		const uint32_t ec = (k + 1 < (uint32_t) CK ? uni(s_cnt[w][k + 1 < (uint32_t) CK ? k + 1 : k]) : ew) - ef;
		gather_low(low, nlow, pos, val, nex, zd0, i0, n, e_lo + ef, ec, v);
#pragma unroll
		for (int h = 0; h < 4; h++)
			v[h] = unzz_pair(v[h]);
		(void) lane_prefix8(v);
		const uint32_t b16 = (sb + uni(s_sub[w][k]) + s_xl[w][k][lane]) & 0xFFFFu;
		const uint32_t b2 = b16 | (b16 << 16);
#pragma unroll
		for (int h = 0; h < 4; h++) {
			v[h] = pk_add16(v[h], b2);
			if (q)
				v[h] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, v[h]) << qq);
		}
		if (i0 + 8 <= n) {
			st16_stream(out + i0, make_uint4(v[0], v[1], v[2], v[3]));
		} else if (i0 < n) {
#pragma unroll
			for (uint32_t h = 0; h < 8; h++)
				if (h < n - i0)
					out[i0 + h] = (int16_t) (v[h >> 1] >> (16 * (h & 1)));
		}
	}
	STAMP(6);
	if (!HUFF)
		return;
	__syncthreads(); // the ticket and the tables of this chunk are free again
	}
}

// ------------------------------------------------------------------ launchers

static uint64_t n_pass_a = 0; // launches of k_ex_scan_chunked<false, ..> so far (press_hip_debug_pass_a_launches)
extern "C" uint64_t press_hip_debug_pass_a_launches(void) { return n_pass_a; }
static uint64_t n_stage_sized = 0; // launches of a stage's sizing kernels so far: count and pick, or hist and tree
extern "C" uint64_t press_hip_debug_stage_sizing_launches(void) { return n_stage_sized; }
void ex_stage_sized() { n_stage_sized++; }
#ifdef DEC_STAMPS
int ex_stamps_read(uint64_t *dst, uint32_t nwords) { return stamps_read(dst, nwords); }
#endif

// exception-split encode: chunk table and ReadMeta of the batch ...
void ex_encode_prep(const BatchArgs &a, hipStream_t s) { launch_chunk_prep(a, false, 0, true, nullptr, s); }

// pass A (surplus workgroups - max_chunks bounds the real count from above - exit at once)
static void ex_pass_a(const BatchArgs &a, ExEnt ent, hipStream_t s)
{
	n_pass_a++;
	if (ent == ENT_SHUFF)
		hipLaunchKernelGGL((k_ex_scan_chunked<false, true>), dim3(a.max_chunks), dim3(CWG), 0, s, a);
	else
		hipLaunchKernelGGL((k_ex_scan_chunked<false>), dim3(a.max_chunks), dim3(CWG), 0, s, a);
}

// ... chunked scan (pass A), section per read, chunked pass B
void launch_ex_encode_chunked(const BatchArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	ex_encode_prep(a, s);
	ex_pass_a(a, ent, s);
	ex_encode_lists(a, fmt, s);
	ex_encode_streams(a, fmt, ent, s);
}

// Packed press of the exception-split family.  PACK_SIZE: the chain up to the exception lists, with a.out_off = pk.slot
// still all zeros (k_chunk_prep only notes a base it is given; the family's kernels do not look at cap_ok); k_ex_sizes -
// the size half of k_ex_section - then knows every stream's length (the range coders': a bound), the scan lays the
// arena out and the chunks learn their read's base.  PACK_WRITE: the section and the encoder as they are, against
// pk.slot.  Pass A runs once.  A PAY_STAGED stage sizes its own payload: PACK_SIZE ends with pass B into a.low_tmp and
// the stage's sizing kernels, as launch_ex_prefix_sizes runs them, and PACK_WRITE goes on from what they left
// (ExStage::write_sized): the values are counted once.
void ex_packed_sizes(const BatchArgs &a, ExFmt fmt, ExEnt ent, uint64_t *need, hipStream_t s)
{
	const ExStage &st = EX_STAGES[ent];
	launch_ex_sizes(a, fmt, ent, need, s);
	if (st.pay != PAY_STAGED)
		return;
	hipLaunchKernelGGL(k_low_encode_chunked<false>, dim3(a.max_chunks), dim3(CWG), 0, s, a);
	st.press(a, need, s);
}

void ex_packed_streams(const BatchArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s)
{
	const ExStage &st = EX_STAGES[ent];
	if (st.pay != PAY_STAGED)
		return ex_encode_streams(a, fmt, ent, s);
	launch_ex_section(a, fmt, ent, s);
	ktime_begin(0, s);
	st.write_sized(a, s);
	ktime_end(0, s);
}

void launch_ex_encode_packed(const BatchArgs &a, ExFmt fmt, ExEnt ent, const PackArgs &pk, int phases, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	if (phases & PACK_SIZE) {
		(void) hipMemsetAsync(pk.slot, 0, ((size_t) a.nreads + 1) * 8, s);
		ex_encode_prep(a, s);
		ex_pass_a(a, ent, s);
		ex_encode_lists(a, fmt, s);
		ex_packed_sizes(a, fmt, ent, pk.need, s);
		if (pk.layout) {
			launch_pack_scan(pk, a.nreads, s);
			launch_pack_patch(a, pk.slot, s);
		}
	}
	if (phases & PACK_WRITE)
		ex_packed_streams(a, fmt, ent, s);
}

// press_hip_rice_press_sizes, press_hip_huffman_press_sizes (a stage with sizes_only): the chain up to the exception lists
// as the packed press runs it (k_chunk_prep leaves status 0, so k_low_encode_chunked writes every read's one-byte values to
// a.low_tmp without a section in front), k_ex_sizes for header and section, then the stage's own sizes: the Rice count and
// pick, or the per-read Huffman hist and tree.  Nothing of the caller's but need[] is written.
void launch_ex_prefix_sizes(const BatchArgs &a, ExFmt fmt, ExEnt ent, uint64_t *need, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks || !EX_STAGES[ent].sizes_only)
		return;
	ex_encode_prep(a, s);
	ex_pass_a(a, ent, s);
	ex_encode_lists(a, fmt, s);
	launch_ex_sizes(a, fmt, ent, need, s);
	hipLaunchKernelGGL(k_low_encode_chunked<false>, dim3(a.max_chunks), dim3(CWG), 0, s, a);
	EX_STAGES[ent].press(a, need, s);
}

// what follows pass A: the exceptions of every read counted and listed ...
void ex_encode_lists(const BatchArgs &a, ExFmt fmt, hipStream_t s)
{
	if (fmt == EXF_EXZD) {
		// second scan on the shifted samples for reads with q > 0
		hipLaunchKernelGGL(k_ex_redo_flag, dim3((a.nreads + 255) / 256), dim3(256), 0, s, a);
		hipLaunchKernelGGL((k_ex_scan_chunked<true>), dim3(a.max_chunks), dim3(CWG), 0, s, a);
	}
	hipLaunchKernelGGL(k_ex_prefix, dim3((a.nreads + 3) / 4), dim3(256), 0, s, a, fmt == EXF_EXZD ? 1 : 0);
	hipLaunchKernelGGL(k_ex_list, dim3((a.max_chunks + 3) / 4), dim3(CWG), 0, s, a);
}

// the two stages that are pass B itself: the one-byte values, or their static-Huffman codes, straight into the stream
void launch_low_encode(const BatchArgs &a, uint64_t *, hipStream_t s)
{
	if (a.zhist)
		hipLaunchKernelGGL(k_low_encode_chunked<true>, dim3(a.max_chunks), dim3(CWG), 0, s, a);
	else
		hipLaunchKernelGGL(k_low_encode_chunked<false>, dim3(a.max_chunks), dim3(CWG), 0, s, a);
}
void launch_shuff_encode(const BatchArgs &a, uint64_t *, hipStream_t s)
{
	hipLaunchKernelGGL(k_huff_encode_chunked, dim3(a.max_chunks), dim3(CWG), 0, s, a);
}

// ... and the streams: section per read, then the stage (timed as the dominant kernel of the press).  A stage with low_tmp
// codes the one-byte values pass B has left in a temporary: one lane (order 1: one workgroup) per read, or a wave per unit
void ex_encode_streams(const BatchArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s)
{
	const ExStage &st = EX_STAGES[ent];
	launch_ex_section(a, fmt, ent, s);
	if (st.low_tmp)
		hipLaunchKernelGGL(k_low_encode_chunked<false>, dim3(a.max_chunks), dim3(CWG), 0, s, a);
	ktime_begin(0, s);
	st.press(a, nullptr, s);
	ktime_end(0, s);
}

// exception-split decode: parse + the stage's depress (press_sections.hip), then the chunked merge
void launch_ex_decode_chunked(const DecodeArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s)
{
	const bool huff = EX_STAGES[ent].depress != nullptr; // the one-byte stream comes from a.low (Huffman or range decoder)
	if (!a.nreads || !a.max_chunks)
		return;
	launch_ex_parse_huff(a, fmt, ent, s); // (k_ex_parse clears both control blocks)
	hipLaunchKernelGGL(k_chunk_prep_meta, dim3((a.nreads + 255) / 256), dim3(256), 0, s, a.off, a.in_off,
			   a.meta, a.nreads, a.chunks, a.gran, a.ctl, a.max_chunks, a.out_n,
			   ent == ENT_SHUFF ? (const uint32_t *) a.hread : (const uint32_t *) nullptr, a.ex_pos);
	hipLaunchKernelGGL(k_ex_ranks, dim3((a.max_chunks * 8 + 255) / 256), dim3(256), 0, s, a);
	if (!huff)
		ktime_begin(1, s);
	if (ent == ENT_SHUFF) {
		// static Huffman: k_huf_emit has written the samples of every read whose lists interleave cleanly;
		// the chunk table holds the others only (normally none)
		const uint32_t grid = a.max_chunks < 1024u ? a.max_chunks : 1024u;
		hipLaunchKernelGGL((k_low_decode_chunked<true>), dim3(grid), dim3(CWG), 0, s, a);
	} else if (huff) {
		hipLaunchKernelGGL((k_low_decode_chunked<true>), dim3(a.max_chunks), dim3(CWG), 0, s, a);
	} else {
		hipLaunchKernelGGL((k_low_decode_chunked<false>), dim3(a.max_chunks), dim3(CWG), 0, s, a);
	}
	if (!huff)
		ktime_end(1, s);
}

} // namespace ph
