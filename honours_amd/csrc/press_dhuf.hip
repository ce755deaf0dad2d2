// press_dhuf.hip - entropy stage 7 of the exception-split methods: a Huffman code built from each read's own one-byte
// values and written in front of its payload (huffman_encode_memory / huffman_decode_memory, huffman/huffman.c:984-1072,
// as the reference's huffman_*_zd methods call them).
//
// Table and payload (include/press_hip.h section 2v; pinned by tests/_dhuf.py and tests/golden/ref_huffman.json):
//   counts   the symbols present, ascending by count, ties by symbol value
//   tree     until one node is left: the first two nodes of the list become the zero and the one child of a parent with
//            the sum of their counts, which goes back in front of every remaining node whose count is not smaller
//   code     the path from the root, first edge first; code bit k is bit k, from the least significant, of a uint64_t
//   table    (nsym - 1) & 255, nlow as a big-endian u32, then per present symbol in ascending order
//            { symbol, len, ceil(len / 8) code bytes, least significant first }
//   payload  the codes in order, bit i of the payload in bit i % 8 of byte i / 8, the last byte zero padded
//
// PRESS.  The one-byte values (a.low_tmp, k_low_encode_chunked) in UNITS of DH_UNIT values, a wave each, indexed as
// press_rice.hip indexes its units; the buffers of the Rice press serve here too (a.ri_sum: a unit's bits in the first
// of its eight words, a.ri_start, a.ri_pay; a.ri_rd holds DhRead records, a.ri_k the longest codes).
//   k_dh_hist    per unit: the 256 counts in LDS, added to the read's 256 words (a.dh_tab, zeroed by the launcher)
//   k_dh_tree    per read, one wave: the sorted list in LDS, at most 255 merge steps (the insertion point by ballot,
//                the nodes in front of it move down one place), the codes by walking up from every leaf; the table's
//                bytes, nbits, the exact length and the slot check; press writes the table into the slot
//   k_dh_count   per unit the sum of its values' code lengths
//   k_dh_scan    per read the exclusive scan of the units' bits
//   k_dh_write   per unit: code lengths -> wave scan -> bit positions; the bits of 512 values are assembled in LDS
//                windows and go out as whole dwords to the staged payload, seam dwords merged with atomic OR
//   k_dh_copy    staged payload -> the slot, behind section and table
// PRESS SIZES (need != NULL): hist and tree alone.
//
// DEPRESS.  The plan of press_rice.hip with a table in the place of the arithmetic; its scratch serves here too.
//   k_dh_table   per read, one wave: the table's bytes to LDS, the entries parsed and checked (definition 4 of 2v), sorted
//                by their left-aligned codes - neighbours tell whether the code is prefix-free -, then the read's decode
//                table (DhTab): a direct look-up by the next DH_W bits, and the sorted list for a binary search where
//                the direct entry says "longer"
//   k_dh_dplan   per read: the subsequences worth decoding in parallel, the tile table
//   k_dh_sync    the tile's table to LDS; a lane runs up through the subsequence in front, then decodes its own:
//                record = { start, end, codes }; bits that are no code end a record early (end = DH_SAT)
//   k_dh_fix x 4 a lane whose start is not the end the subsequence in front recorded decodes again from that end (the
//                first round counts into ri_ctl[1], the later ones into ri_ctl[2])
//   k_dh_check, k_dh_dscan, k_dh_emit   as the Rice kernels of those names
//   k_dh_walk    per read, serially from where the chain ends until nlow values are out; bits that are no code, or a
//                code that runs past the payload's end, refuse the read (ReadMeta::status, in front of k_chunk_prep_meta)
// The number of launches is fixed, and correctness never depends on synchronisation.

#include "press_internal.h"
#include "press_wave.h"

namespace ph {

namespace {

constexpr uint64_t DH_FAIL64 = ~0ull;
constexpr uint32_t DH_NONE = 0xFFFFFFFFu; // record: no start known
constexpr uint32_t DH_SAT = 0xFFFFFFFEu;  // record: no end (the subsequence stopped at bits that are no code)
constexpr uint32_t DH_WIN = 256;          // dwords of a writer's LDS window
constexpr uint32_t DH_LONG = 0xFFFFu;     // direct entry: the code is longer than DH_W bits
constexpr uint32_t DH_RAW = 2568;         // bytes of the longest table, 5 + 256 * 10, rounded up
constexpr int DH_FIX_ROUNDS = 4;          // launches of k_dh_fix

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

__device__ __forceinline__ uint64_t *press_codes(const BatchArgs &a, uint32_t r)
{
	return reinterpret_cast<uint64_t *>(a.dh_tab + (size_t) r * DH_PRESS_TAB);
}
__device__ __forceinline__ uint32_t *press_hist(const BatchArgs &a, uint32_t r)
{
	return reinterpret_cast<uint32_t *>(a.dh_tab + (size_t) r * DH_PRESS_TAB + 2048);
}
__device__ __forceinline__ DhRead *press_read(const BatchArgs &a, uint32_t r) { return reinterpret_cast<DhRead *>(a.ri_rd) + r; }

// the unit a wave works on: false if there is none
struct Unit {
	uint32_t r, u, cnt; // read, unit id, values
	uint64_t v0, soff;  // first value, the read's sample offset
};
__device__ __forceinline__ bool unit_of(const BatchArgs &a, uint32_t u, Unit &x)
{
	const uint32_t t = u / RICE_UPC;
	if (t >= uni(a.ctl->nchunks))
		return false;
	const ChunkDesc *d = a.chunks + t;
	x.r = uni(d->read);
	x.u = u;
	x.soff = uni64(d->sig_off);
	const ReadMeta *m = a.meta + x.r;
	if (uni(m->status))
		return false;
	const uint64_t nlow = (uint64_t) uni(d->n) - 1 - uni(m->nex);
	x.v0 = ((uint64_t) uni(d->j) * RICE_UPC + u % RICE_UPC) * DH_UNIT;
	if (x.v0 >= nlow)
		return false;
	x.cnt = nlow - x.v0 < DH_UNIT ? (uint32_t) (nlow - x.v0) : DH_UNIT;
	return true;
}

// up to eight values of a unit from i on, one per byte of the result; nv: how many there are
__device__ __forceinline__ uint64_t load8(const uint8_t *in, uint32_t i, uint32_t cnt, uint32_t &nv)
{
	uint64_t v = 0;
	nv = i < cnt ? (cnt - i < 8 ? cnt - i : 8u) : 0u;
	if (nv == 8) {
		__builtin_memcpy(&v, in + i, 8); // (8-byte aligned: the read's offset and i are multiples of 8)
	} else {
		for (uint32_t j = 0; j < nv; j++)
			v |= (uint64_t) in[i + j] << (8 * j);
	}
	return v;
}

} // namespace

__global__ __launch_bounds__(256) void k_dh_hist(BatchArgs a)
{
	__shared__ uint32_t s_h[4][256];
	const uint32_t lane = threadIdx.x & 63;
	uint32_t *h = s_h[threadIdx.x >> 6];
	Unit x;
	if (!unit_of(a, uni(blockIdx.x * 4 + (threadIdx.x >> 6)), x))
		return;
	for (uint32_t i = lane; i < 256; i += 64)
		h[i] = 0;
	__builtin_amdgcn_wave_barrier();
	const uint8_t *in = a.low_tmp + x.soff + x.v0;
	for (uint32_t step = 0; step < DH_UNIT; step += 512) {
		uint32_t nv;
		const uint64_t v = load8(in, step + lane * 8, x.cnt, nv);
		for (uint32_t j = 0; j < nv; j++)
			atomicAdd(&h[(uint32_t) (v >> (8 * j)) & 0xFFu], 1u);
	}
	__builtin_amdgcn_wave_barrier();
	uint32_t *g = press_hist(a, x.r);
	for (uint32_t i = lane; i < 256; i += 64) {
		const uint32_t c = h[i];
		if (c)
			atomicAdd(&g[i], c);
	}
}

// One wave per read; lane l owns the symbols 4 l .. 4 l + 3.  need == NULL: press (behind k_ex_section: status != 0 for a
// read it refused); else sizes (behind k_ex_sizes, which left header + section in need[r], or FAILED).
__global__ __launch_bounds__(64) void k_dh_tree(BatchArgs a, uint64_t *need)
{
	__shared__ uint32_t s_cnt[512]; // the nodes' counts: 0 .. 255 the leaves (the symbols), 256 .. the parents as they are made
	__shared__ uint16_t s_par[512]; // a node's parent | the edge's bit << 15
	__shared__ uint16_t s_lst[256]; // the list, ascending by count
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const ReadMeta *m = a.meta + r;
	const uint32_t n = a.nsamp[r];
	DhRead *rd = press_read(a, r);
	const bool refused = n == 0 || (need ? need[r] == DH_FAIL64 : m->status != 0);
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
	const uint32_t *hist = press_hist(a, r);
	uint32_t c[4];
	uint32_t nsym = 0;
#pragma unroll
	for (uint32_t j = 0; j < 4; j++) {
		c[j] = hist[lane * 4 + j];
		s_cnt[lane * 4 + j] = c[j];
		nsym += (uint32_t) __popcll(__ballot(c[j] != 0));
	}
	__builtin_amdgcn_wave_barrier();
	// the place of every symbol present: the symbols with a smaller count, or the same count and a smaller value
	for (uint32_t j = 0; j < 4; j++) {
		if (!c[j])
			continue;
		const uint32_t sym = lane * 4 + j;
		uint32_t rank = 0;
		for (uint32_t t = 0; t < 256; t++) {
			const uint32_t ct = s_cnt[t];
			rank += (ct != 0 && (ct < c[j] || (ct == c[j] && t < sym))) ? 1u : 0u;
		}
		s_lst[rank] = (uint16_t) sym;
	}
	__builtin_amdgcn_wave_barrier();
	// the merge steps: the list is s_lst[head .. nsym)
	uint32_t head = 0;
	for (uint32_t step = 0; head + 1 < nsym; step++) {
		const uint32_t m1 = s_lst[head], m2 = s_lst[head + 1];
		const uint32_t pc = s_cnt[m1] + s_cnt[m2];
		const uint32_t pid = 256 + step;
		uint32_t pos = 0; // nodes behind the two with a smaller count than the parent: it goes behind them
		for (uint32_t base = head + 2; base < nsym; base += 64) {
			const uint32_t i = base + lane;
			const bool lt = i < nsym && s_cnt[s_lst[i]] < pc;
			const uint32_t k = (uint32_t) __popcll(__ballot(lt));
			pos += k;
			if (k < 64)
				break;
		}
		for (uint32_t base = 0; base < pos; base += 64) { // they move down one place
			const uint32_t k = base + lane;
			const uint16_t v = k < pos ? s_lst[head + 2 + k] : (uint16_t) 0;
			__builtin_amdgcn_wave_barrier();
			if (k < pos)
				s_lst[head + 1 + k] = v;
			__builtin_amdgcn_wave_barrier();
		}
		if (lane == 0) {
			s_lst[head + 1 + pos] = (uint16_t) pid;
			s_cnt[pid] = pc;
			s_par[m1] = (uint16_t) pid;
			s_par[m2] = (uint16_t) (pid | 0x8000u);
		}
		__builtin_amdgcn_wave_barrier();
		head++;
	}
	const uint32_t root = nsym ? s_lst[head] : 0u;
	// the codes: up from every leaf, the last edge first
	uint64_t *codes = press_codes(a, r);
	uint32_t len[4], maxlen = 0, tbytes = 0;
	uint64_t bits[4], nbits = 0;
#pragma unroll
	for (uint32_t j = 0; j < 4; j++) {
		len[j] = 0;
		bits[j] = 0;
		if (c[j]) {
			uint32_t node = lane * 4 + j;
			while (node != root && len[j] < 63) {
				const uint32_t p = s_par[node];
				bits[j] = (bits[j] << 1) | (p >> 15);
				node = p & 0x7FFFu;
				len[j]++;
			}
			tbytes += 2 + (len[j] + 7) / 8;
			nbits += (uint64_t) c[j] * len[j];
			maxlen = len[j] > maxlen ? len[j] : maxlen;
		}
		codes[lane * 4 + j] = bits[j] | ((uint64_t) len[j] << 56);
	}
	maxlen = max32(maxlen);
	nbits = sum64(nbits);
	const uint32_t inc = scan32(tbytes, lane);
	const uint32_t tablen = 5 + (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
	const uint64_t paylen = (nbits + 7) / 8;
	bool ok = true;
	uint64_t total = 0;
	if (!need) {
		total = (uint64_t) m->hdr + m->seclen + tablen + paylen;
		ok = total <= a.out_off[r + 1] - a.out_off[r];
	}
	if (!need && ok) { // the table, behind the section
		uint8_t *t = a.out + a.out_off[r] + m->hdr + m->seclen;
		if (lane == 0) {
			t[0] = (uint8_t) ((nsym - 1) & 255u);
			t[1] = (uint8_t) (nlow >> 24);
			t[2] = (uint8_t) (nlow >> 16);
			t[3] = (uint8_t) (nlow >> 8);
			t[4] = (uint8_t) nlow;
		}
		uint8_t *e = t + 5 + (inc - tbytes);
		for (uint32_t j = 0; j < 4; j++) {
			if (!c[j])
				continue;
			*e++ = (uint8_t) (lane * 4 + j);
			*e++ = (uint8_t) len[j];
			for (uint32_t b = 0; b < (len[j] + 7) / 8; b++)
				*e++ = (uint8_t) (bits[j] >> (8 * b));
		}
	}
	if (lane)
		return;
	if (need)
		need[r] += tablen + paylen;
	else
		a.out_len[r] = ok ? total : DH_FAIL64;
	rd->nbits = nbits;
	rd->paylen = paylen;
	rd->tablen = tablen;
	rd->maxlen = maxlen;
	rd->ok = ok ? 1 : 0;
	rd->nlow = (uint32_t) nlow;
	rd->nunits = (uint32_t) ((nlow + DH_UNIT - 1) / DH_UNIT);
	rd->nsym = nsym;
	if (a.ri_k)
		a.ri_k[r] = ok ? (uint8_t) maxlen : (uint8_t) 0;
}

__global__ __launch_bounds__(256) void k_dh_count(BatchArgs a)
{
	__shared__ uint8_t s_len[4][256];
	const uint32_t lane = threadIdx.x & 63;
	uint8_t *ln = s_len[threadIdx.x >> 6];
	Unit x;
	if (!unit_of(a, uni(blockIdx.x * 4 + (threadIdx.x >> 6)), x))
		return;
	if (!uni(press_read(a, x.r)->ok))
		return;
	const uint64_t *codes = press_codes(a, x.r);
	for (uint32_t i = lane; i < 256; i += 64)
		ln[i] = (uint8_t) (codes[i] >> 56);
	__builtin_amdgcn_wave_barrier();
	const uint8_t *in = a.low_tmp + x.soff + x.v0;
	uint32_t L = 0;
	for (uint32_t step = 0; step < DH_UNIT; step += 512) {
		uint32_t nv;
		const uint64_t v = load8(in, step + lane * 8, x.cnt, nv);
		for (uint32_t j = 0; j < nv; j++)
			L += ln[(uint32_t) (v >> (8 * j)) & 0xFFu];
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		L += (uint32_t) __shfl_xor((int) L, d, 64);
	if (lane == 0)
		a.ri_sum[(size_t) x.u * 8] = L;
}

// one wave per read: ri_start[unit] = the bits of the read's units in front of it
__global__ __launch_bounds__(64) void k_dh_scan(BatchArgs a)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const DhRead *rd = press_read(a, r);
	if (!rd->ok)
		return;
	const uint32_t nunits = rd->nunits;
	const size_t u0 = (size_t) a.first_chunk[r] * RICE_UPC;
	uint64_t carry = 0;
	for (uint32_t base = 0; base < nunits; base += 64) {
		const uint32_t i = base + lane;
		const uint64_t b = i < nunits ? a.ri_sum[(u0 + i) * 8] : 0;
		const uint64_t inc = wave_incl_scan64(b, lane);
		if (i < nunits)
			a.ri_start[u0 + i] = carry + inc - b;
		carry += __shfl(inc, 63, 64);
	}
}

__global__ __launch_bounds__(256) void k_dh_write(BatchArgs a)
{
	__shared__ uint32_t s_bits[4][DH_WIN];
	__shared__ uint64_t s_code[4][256];
	const uint32_t lane = threadIdx.x & 63;
	uint32_t *lds = s_bits[threadIdx.x >> 6];
	uint64_t *code = s_code[threadIdx.x >> 6];
	Unit x;
	if (!unit_of(a, uni(blockIdx.x * 4 + (threadIdx.x >> 6)), x))
		return;
	const DhRead *rd = press_read(a, x.r);
	if (!uni(rd->ok))
		return;
	const uint64_t *codes = press_codes(a, x.r);
	for (uint32_t i = lane; i < 256; i += 64)
		code[i] = codes[i];
	__builtin_amdgcn_wave_barrier();
	const uint8_t *in = a.low_tmp + x.soff + x.v0;
	uint32_t *pay = reinterpret_cast<uint32_t *>(a.ri_pay + 2 * x.soff);
	uint64_t P = uni64(a.ri_start[x.u]);
	for (uint32_t step = 0; step < DH_UNIT; step += 512) {
		uint32_t nv;
		const uint64_t v = load8(in, step + lane * 8, x.cnt, nv);
		uint32_t L = 0;
		for (uint32_t j = 0; j < nv; j++)
			L += (uint32_t) (code[(uint32_t) (v >> (8 * j)) & 0xFFu] >> 56);
		const uint32_t inc = scan32(L, lane);
		const uint32_t tot = (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
		if (!tot)
			break; // (wave-uniform: the unit's values are used up, or the read's one code has no bit)
		const uint64_t mine = P + inc - L, mine_end = P + inc;
		const uint64_t firstdw = P >> 5, lastdw = (P + tot - 1) >> 5;
		for (uint64_t wb = firstdw; wb <= lastdw; wb += DH_WIN) {
			for (uint32_t d = lane; d < DH_WIN; d += 64)
				lds[d] = 0;
			__builtin_amdgcn_wave_barrier();
			// nb bits (1 .. 32) at stream position pos, cut to the window
			auto put = [&](uint64_t pos, uint32_t bits, uint32_t nb) {
				const uint64_t d = (pos >> 5) - wb; // (wraps for a position in front of the window: then >= DH_WIN)
				const uint32_t sh = (uint32_t) pos & 31u;
				if (d < DH_WIN)
					atomicOr(&lds[d], bits << sh);
				if (sh + nb > 32 && d + 1 < DH_WIN) // (d + 1 == 0: the code's tail is the window's first dword)
					atomicOr(&lds[d + 1], bits >> (32 - sh));
			};
			if (L && mine_end > (wb << 5) && mine < ((wb + DH_WIN) << 5)) {
				uint64_t p = mine;
				for (uint32_t j = 0; j < nv; j++) {
					const uint64_t cw = code[(uint32_t) (v >> (8 * j)) & 0xFFu];
					const uint32_t l = (uint32_t) (cw >> 56);
					if (l) // a code of up to 63 bits crosses up to three dwords
						put(p, (uint32_t) cw, l < 32 ? l : 32u);
					if (l > 32)
						put(p + 32, (uint32_t) (cw >> 32) & 0x00FFFFFFu, l - 32);
					p += l;
				}
			}
			__builtin_amdgcn_wave_barrier();
			for (uint32_t d = lane; d < DH_WIN && wb + d <= lastdw; d += 64) {
				const uint32_t w = lds[d];
				const uint64_t idx = wb + d;
				if (idx == firstdw || idx == lastdw) { // shared with the spans around this one
					if (w)
						atomicOr(pay + idx, w);
				} else {
					pay[idx] = w;
				}
			}
			__builtin_amdgcn_wave_barrier();
		}
		P += tot;
	}
}

// staged payload -> the slot: RICE_COPY bytes per unit index, which covers every payload (at most eight bits a value on
// average: the fixed eight-bit code is a prefix code, and the Huffman code is no longer)
__global__ __launch_bounds__(256) void k_dh_copy(BatchArgs a)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t u = uni(blockIdx.x * 4 + (threadIdx.x >> 6));
	const uint32_t t = u / RICE_UPC;
	if (t >= uni(a.ctl->nchunks))
		return;
	const ChunkDesc *d = a.chunks + t;
	const uint32_t r = uni(d->read);
	const DhRead *rd = press_read(a, r);
	const ReadMeta *m = a.meta + r;
	if (uni(m->status) || !uni(rd->ok))
		return;
	const uint64_t paylen = uni64(rd->paylen);
	const uint64_t b0 = ((uint64_t) uni(d->j) * RICE_UPC + u % RICE_UPC) * RICE_COPY;
	if (b0 >= paylen)
		return;
	const uint32_t len = paylen - b0 < RICE_COPY ? (uint32_t) (paylen - b0) : RICE_COPY;
	const uint8_t *src = a.ri_pay + 2 * uni64(d->sig_off) + b0;
	uint8_t *dst = a.out + a.out_off[r] + uni(m->hdr) + uni(m->seclen) + uni(rd->tablen) + b0;
	for (uint32_t b = lane * 8; b < len; b += 512) {
		if (b + 8 <= len) {
			uint2 w = *reinterpret_cast<const uint2 *>(src + b);
			__builtin_memcpy(dst + b, &w, 8);
		} else {
			for (uint32_t j = b; j < len; j++)
				dst[j] = src[j];
		}
	}
}

// ------------------------------------------------------------------ depress

namespace {

struct DBits {
	const uint8_t *in; // the payload
	uint64_t len;      // its bytes
};

// the read's decode table, in scratch or in LDS
struct DTab {
	const uint64_t *lcode;
	const uint16_t *ent;
	const uint16_t *direct;
	uint32_t nent;
};

// 64 bits from bit p on; behind the end: zeros
__device__ __forceinline__ uint64_t peek64(const DBits &b, uint64_t p)
{
	const uint64_t at = p >> 3;
	const uint32_t sh = (uint32_t) p & 7u;
	uint64_t w = 0;
	if (at + 8 <= b.len) {
		__builtin_memcpy(&w, b.in + at, 8);
	} else {
		for (uint32_t i = 0; i < 8; i++)
			if (at + i < b.len)
				w |= (uint64_t) b.in[at + i] << (8 * i);
	}
	w >>= sh;
	if (sh && at + 8 < b.len)
		w |= (uint64_t) b.in[at + 8] << (64 - sh);
	return w;
}

// 32 bits from bit p on; behind the end: zeros
__device__ __forceinline__ uint32_t peek32(const DBits &b, uint64_t p)
{
	const uint64_t at = p >> 3;
	uint64_t w = 0;
	if (at + 8 <= b.len) {
		__builtin_memcpy(&w, b.in + at, 8);
	} else {
		for (uint32_t i = 0; i < 5; i++)
			if (at + i < b.len)
				w |= (uint64_t) b.in[at + i] << (8 * i);
	}
	return (uint32_t) (w >> (p & 7u));
}

// one code from p on: p moves behind it, v = its symbol; false: the bits are no code, or the code ends behind the payload
__device__ __forceinline__ bool dh_code(const DBits &b, const DTab &T, uint64_t &p, uint32_t &v)
{
	const uint64_t endbit = b.len * 8;
	if (p >= endbit)
		return false;
	uint32_t e = T.direct[peek32(b, p) & ((1u << DH_W) - 1u)];
	if (e == 0)
		return false;
	if (e == DH_LONG) {
		const uint64_t key = __brevll(peek64(b, p));
		uint32_t lo = 0, hi = T.nent; // the entries in front of lo are <= key
		while (lo < hi) {
			const uint32_t mid = (lo + hi) >> 1;
			if (T.lcode[mid] <= key)
				lo = mid + 1;
			else
				hi = mid;
		}
		if (lo == 0)
			return false;
		e = T.ent[lo - 1];
		if ((key ^ T.lcode[lo - 1]) >> (64 - (e >> 8)))
			return false;
	}
	const uint32_t ln = e >> 8;
	if (p + ln > endbit)
		return false;
	p += ln;
	v = e & 0xFFu;
	return true;
}

__device__ __forceinline__ DhTab *tab_of(const DecodeArgs &a, uint32_t r) { return reinterpret_cast<DhTab *>(a.dh_tab) + r; }

__device__ __forceinline__ DTab global_tab(const DhTab *t)
{
	DTab T;
	T.lcode = t->lcode;
	T.ent = t->ent;
	T.direct = t->direct;
	T.nent = t->nent;
	return T;
}

struct DTile {
	uint32_t r;
	uint32_t s;     // the lane's subsequence of the read
	size_t g;       // ... and its record
	uint64_t begin; // its first bit
	DBits b;
};
// the tile of a workgroup: false (for the whole workgroup): none
__device__ __forceinline__ bool tile_read(const DecodeArgs &a, uint32_t &r)
{
	if (blockIdx.x >= uni(a.ri_ctl[0]) || blockIdx.x >= a.ri_max_tiles)
		return false;
	r = uni(a.ri_tile[blockIdx.x].x);
	return r != DH_NONE; // (a tile id k_dh_dplan took and could not use)
}
// the subsequence of a thread of that tile; false: none
__device__ __forceinline__ bool dtile_of(const DecodeArgs &a, uint32_t r, DTile &t)
{
	const RiceDRead *rd = a.ri_drd + r;
	t.r = r;
	t.s = uni(a.ri_tile[blockIdx.x].y) * RICE_DT + threadIdx.x;
	if (t.s >= uni(rd->nsubs))
		return false;
	t.g = (size_t) blockIdx.x * RICE_DT + threadIdx.x;
	t.begin = (uint64_t) t.s * RICE_SUB;
	const ReadMeta *m = a.meta + r;
	t.b.in = a.in + a.in_off[r] + uni(m->hdr) + uni(m->seclen) + uni(tab_of(a, r)->tablen);
	t.b.len = uni64(rd->paylen);
	return true;
}

// the read's table -> LDS, by the whole workgroup
struct LdsTab {
	uint64_t lcode[256];
	uint16_t ent[256];
	uint16_t direct[1u << DH_W];
};
__device__ __forceinline__ DTab load_tab(const DhTab *t, LdsTab &l)
{
	const uint32_t nent = uni(t->nent);
	for (uint32_t i = threadIdx.x; i < nent; i += 256) {
		l.lcode[i] = t->lcode[i];
		l.ent[i] = t->ent[i];
	}
	const uint32_t *src = reinterpret_cast<const uint32_t *>(t->direct);
	uint32_t *dst = reinterpret_cast<uint32_t *>(l.direct);
	for (uint32_t i = threadIdx.x; i < (1u << DH_W) / 2; i += 256)
		dst[i] = src[i];
	__syncthreads();
	DTab T;
	T.lcode = l.lcode;
	T.ent = l.ent;
	T.direct = l.direct;
	T.nent = nent;
	return T;
}

// the subsequence from `start` on -> its record
__device__ __forceinline__ void dsub(const DecodeArgs &a, const DTile &t, const DTab &T, uint64_t start)
{
	uint32_t *rec = a.ri_rec + 3 * t.g;
	uint64_t p = start;
	uint32_t cnt = 0, v;
	const uint64_t end = t.begin + RICE_SUB;
	bool whole = true;
	while (p < end) {
		if (!dh_code(t.b, T, p, v)) {
			whole = false;
			break;
		}
		cnt++;
	}
	rec[0] = (uint32_t) (start - t.begin); // (a code has at most 63 bits: the offsets are small)
	rec[1] = whole ? (uint32_t) (p - end) : DH_SAT;
	rec[2] = cnt;
}

} // namespace

// One wave per read.  The checks of definition 4; a read that fails them is refused here.
__global__ __launch_bounds__(64) void k_dh_table(DecodeArgs a)
{
	__shared__ uint8_t s_raw[DH_RAW];
	__shared__ uint16_t s_eoff[256];
	__shared__ uint64_t s_lc[256], s_slc[256];
	__shared__ uint8_t s_ln[256], s_sln[256], s_sym[256];
	__shared__ uint16_t s_direct[1u << DH_W];
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	ReadMeta *m = a.meta + r;
	DhTab *T = tab_of(a, r);
	if (lane == 0) {
		T->nent = 0;
		T->tablen = 0;
		T->mode = 2;
	}
	if (m->status)
		return;
	const uint64_t head = (uint64_t) m->hdr + m->seclen;
	const uint8_t *in = a.in + a.in_off[r] + head;
	const uint64_t len = a.in_len[r] - head; // (k_ex_parse: the section lies inside the stream)
	const uint32_t nlow = m->nlow;
	const uint32_t avail = len < DH_RAW ? (uint32_t) len : DH_RAW;
	for (uint32_t i = lane; i < avail; i += 64)
		s_raw[i] = in[i];
	__builtin_amdgcn_wave_barrier();
	bool bad = avail < 5;
	uint32_t count = 0, nent = 0, tablen = 5;
	if (!bad) {
		count = ((uint32_t) s_raw[1] << 24) | ((uint32_t) s_raw[2] << 16) | ((uint32_t) s_raw[3] << 8) | s_raw[4];
		bad = count != nlow;
	}
	if (!bad && count == 0) { // an empty table, whatever the first byte says
		if (lane == 0) {
			T->tablen = 5;
			T->mode = 1;
		}
		return;
	}
	if (!bad) {
		nent = (uint32_t) s_raw[0] + 1;
		if (lane == 0) { // the entries' places: each one's length decides where the next begins
			uint32_t p = 5;
			for (uint32_t e = 0; e < nent; e++) {
				if (p + 2 > avail) {
					bad = true;
					break;
				}
				const uint32_t ln = s_raw[p + 1], nb = (ln + 7) / 8;
				if (ln > 63 || (ln == 0 && nent != 1) || p + 2 + nb > avail) {
					bad = true;
					break;
				}
				s_eoff[e] = (uint16_t) p;
				p += 2 + nb;
			}
			tablen = p;
		}
		bad = __shfl((int) bad, 0, 64) != 0;
		tablen = (uint32_t) __shfl((int) tablen, 0, 64);
	}
	__builtin_amdgcn_wave_barrier();
	if (bad) {
		if (lane == 0)
			m->status = 1;
		return;
	}
	// the entries: symbol, length, the code left-aligned with its first bit on top
	for (uint32_t e = lane; e < nent; e += 64) {
		const uint32_t p = s_eoff[e], ln = s_raw[p + 1];
		uint64_t c = 0;
		for (uint32_t b = 0; b < (ln + 7) / 8; b++)
			c |= (uint64_t) s_raw[p + 2 + b] << (8 * b);
		if (ln)
			c &= ~0ull >> (64 - ln);
		s_sym[e] = s_raw[p];
		s_ln[e] = (uint8_t) ln;
		s_lc[e] = __brevll(c);
	}
	__builtin_amdgcn_wave_barrier();
	uint8_t *low = a.low + a.off[r];
	if (nent == 1 && s_ln[0] == 0) { // one symbol without a bit: nlow copies of it, no payload
		const uint8_t sym = s_sym[0];
		for (uint32_t i = lane; i < nlow; i += 64)
			low[i] = sym;
		if (lane == 0) {
			T->tablen = tablen;
			T->mode = 1;
		}
		return;
	}
	// sorted by (left-aligned code, length, place): a code that heads another one heads its neighbour
	for (uint32_t e = lane; e < nent; e += 64) {
		const uint64_t lc = s_lc[e];
		const uint32_t ln = s_ln[e];
		uint32_t rank = 0;
		for (uint32_t f = 0; f < nent; f++) {
			const uint64_t lf = s_lc[f];
			const uint32_t nf = s_ln[f];
			rank += (lf < lc || (lf == lc && (nf < ln || (nf == ln && f < e)))) ? 1u : 0u;
		}
		s_slc[rank] = lc;
		s_sln[rank] = (uint8_t) ln;
		T->lcode[rank] = lc;
		T->ent[rank] = (uint16_t) (s_sym[e] | (ln << 8));
	}
	__builtin_amdgcn_wave_barrier();
	bool pre = false;
	for (uint32_t i = 1 + lane; i < nent; i += 64)
		pre |= ((s_slc[i - 1] ^ s_slc[i]) >> (64 - s_sln[i - 1])) == 0;
	if (__ballot(pre)) {
		if (lane == 0)
			m->status = 1;
		return;
	}
	// the direct look-up by the next DH_W bits: a code of at most DH_W bits fills every index that begins with it
	uint32_t *d32 = reinterpret_cast<uint32_t *>(s_direct);
	for (uint32_t i = lane; i < (1u << DH_W) / 2; i += 64)
		d32[i] = 0;
	__builtin_amdgcn_wave_barrier();
	for (uint32_t e = lane; e < nent; e += 64) {
		const uint32_t ln = s_ln[e];
		const uint32_t c = (uint32_t) (__brevll(s_lc[e])) & ((1u << DH_W) - 1u); // the first DH_W bits, the first one lowest
		if (ln > DH_W) {
			s_direct[c] = (uint16_t) DH_LONG;
		} else {
			const uint16_t v = (uint16_t) (s_sym[e] | (ln << 8));
			for (uint32_t j = 0; j < (1u << (DH_W - ln)); j++)
				s_direct[c | (j << ln)] = v;
		}
	}
	__builtin_amdgcn_wave_barrier();
	uint32_t *g32 = reinterpret_cast<uint32_t *>(T->direct);
	for (uint32_t i = lane; i < (1u << DH_W) / 2; i += 64)
		g32[i] = d32[i];
	if (lane == 0) {
		T->nent = nent;
		T->tablen = tablen;
		T->mode = 0;
	}
}

// One thread per read: its tiles get contiguous ids, taken by one atomic per wave.
__global__ __launch_bounds__(256) void k_dh_dplan(DecodeArgs a)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
	uint32_t nsubs = 0, nlow = 0;
	uint64_t paylen = 0;
	bool ok = false;
	if (r < a.nreads && a.meta[r].status == 0 && tab_of(a, r)->mode == 0) {
		const ReadMeta *m = a.meta + r;
		ok = true;
		nlow = m->nlow;
		paylen = a.in_len[r] - ((uint64_t) m->hdr + m->seclen + tab_of(a, r)->tablen); // (k_dh_table: the table lies inside the stream)
		// a pressed payload has at most eight bits a value; what a forged one has beyond nine is the walk's
		const uint64_t budget = 9ull * nlow + 3;
		const uint64_t useful = paylen * 8 < budget ? paylen * 8 : budget;
		nsubs = (uint32_t) ((useful + RICE_SUB - 1) / RICE_SUB);
	}
	uint32_t nt = (nsubs + RICE_DT - 1) / RICE_DT;
	const uint32_t inc = scan32(nt, lane);
	uint32_t base = 0;
	if (lane == 63 && inc)
		base = atomicAdd(&a.ri_ctl[0], inc);
	base = (uint32_t) __builtin_amdgcn_readlane((int) base, 63);
	const uint32_t first = base + inc - nt;
	if (r >= a.nreads)
		return;
	if ((uint64_t) first + nt > a.ri_max_tiles) { // (the plan's bound covers every batch of disjoint rooms: the walk alone then)
		for (uint32_t j = 0; j < nt && first + j < a.ri_max_tiles; j++)
			a.ri_tile[first + j] = make_uint2(DH_NONE, 0);
		nt = 0;
		nsubs = 0;
	}
	for (uint32_t j = 0; j < nt; j++)
		a.ri_tile[first + j] = make_uint2(r, j);
	RiceDRead *rd = a.ri_drd + r;
	rd->paylen = paylen;
	rd->wpos = 0;
	rd->widx = 0;
	rd->k = 0;
	rd->nsubs = nsubs;
	rd->tile0 = first;
	rd->nlow = nlow;
	rd->hmin = nsubs;
	rd->ok = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_dh_sync(DecodeArgs a)
{
	__shared__ LdsTab s_tab;
	uint32_t r;
	if (!tile_read(a, r))
		return;
	const DTab T = load_tab(tab_of(a, r), s_tab);
	DTile t;
	if (!dtile_of(a, r, t))
		return;
	uint64_t start = 0;
	if (t.s) {
		uint64_t p = t.s == 1 ? 0 : t.begin - RICE_SUB;
		uint32_t v;
		while (p < t.begin) {
			if (!dh_code(t.b, T, p, v)) {
				uint32_t *rec = a.ri_rec + 3 * t.g;
				rec[0] = DH_NONE;
				rec[1] = DH_SAT;
				rec[2] = 0;
				return;
			}
		}
		start = p;
	}
	dsub(a, t, T, start);
}

// A record is written by its own lane alone, and a lane reads of the record in front the one word `end`: whichever
// value it sees, k_dh_check compares what the launches left.
template <int ROUND>
__global__ __launch_bounds__(256) void k_dh_fix(DecodeArgs a)
{
	__shared__ LdsTab s_tab;
	uint32_t r;
	if (!tile_read(a, r))
		return;
	DTile t;
	const bool have = dtile_of(a, r, t) && t.s != 0;
	uint32_t want = DH_SAT;
	if (have)
		want = a.ri_rec[3 * (t.g - 1) + 1];
	const bool redo = have && want < DH_SAT && want != a.ri_rec[3 * t.g];
	if (!__syncthreads_or(redo ? 1 : 0))
		return;
	const DTab T = load_tab(tab_of(a, r), s_tab);
	if (!redo)
		return;
	atomicAdd(&a.ri_ctl[ROUND], 1u);
	dsub(a, t, T, t.begin + want);
}

__global__ __launch_bounds__(256) void k_dh_check(DecodeArgs a)
{
	__shared__ uint32_t s_cnt[4];
	uint32_t r;
	if (!tile_read(a, r)) {
		if (blockIdx.x < uni(a.ri_ctl[0]) && blockIdx.x < a.ri_max_tiles && threadIdx.x == 0)
			a.ri_tbase[(size_t) a.ri_max_tiles + blockIdx.x] = 0;
		return;
	}
	DTile t;
	const bool have = dtile_of(a, r, t);
	uint32_t cnt = 0;
	if (have) {
		const uint32_t start = a.ri_rec[3 * t.g];
		const uint32_t want = t.s ? a.ri_rec[3 * (t.g - 1) + 1] : 0u;
		if (start != want || want >= DH_SAT)
			atomicMin(&a.ri_drd[t.r].hmin, t.s);
		cnt = a.ri_rec[3 * t.g + 2];
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		cnt += (uint32_t) __shfl_xor((int) cnt, d, 64);
	if ((threadIdx.x & 63) == 0)
		s_cnt[threadIdx.x >> 6] = cnt;
	__syncthreads();
	if (threadIdx.x == 0)
		a.ri_tbase[(size_t) a.ri_max_tiles + blockIdx.x] = (uint64_t) s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// one wave per read: ri_tbase[tile] = the codes of the read's tiles in front of it
__global__ __launch_bounds__(64) void k_dh_dscan(DecodeArgs a)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const RiceDRead *rd = a.ri_drd + r;
	const uint32_t nt = (rd->nsubs + RICE_DT - 1) / RICE_DT, t0 = rd->tile0;
	uint64_t carry = 0;
	for (uint32_t base = 0; base < nt; base += 64) {
		const uint32_t i = base + lane;
		const uint64_t c = i < nt ? a.ri_tbase[(size_t) a.ri_max_tiles + t0 + i] : 0;
		const uint64_t inc = wave_incl_scan64(c, lane);
		if (i < nt)
			a.ri_tbase[t0 + i] = carry + inc - c;
		carry += __shfl(inc, 63, 64);
	}
}

__global__ __launch_bounds__(256) void k_dh_emit(DecodeArgs a)
{
	__shared__ LdsTab s_tab;
	__shared__ uint32_t s_w[4];
	uint32_t r;
	if (!tile_read(a, r))
		return;
	const DTab T = load_tab(tab_of(a, r), s_tab);
	DTile t;
	const bool have = dtile_of(a, r, t);
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	RiceDRead *rd = a.ri_drd + r;
	const uint32_t hmin = uni(rd->hmin);
	// the subsequences in front of hmin chain from bit 0: their records are the true ones.  (A record in front of hmin
	// may have stopped early, end = DH_SAT: then hmin is the next subsequence and the walk goes on where it stopped.)
	const bool live = have && t.s < hmin;
	const uint32_t cnt = live ? a.ri_rec[3 * t.g + 2] : 0u;
	const uint32_t inc = scan32(cnt, lane);
	if (lane == 63)
		s_w[w] = inc;
	__syncthreads();
	uint64_t o = a.ri_tbase[blockIdx.x] + inc - cnt;
	for (uint32_t i = 0; i < w; i++)
		o += s_w[i];
	if (!live)
		return;
	const uint64_t nlow = uni(rd->nlow);
	uint8_t *out = a.low + a.off[t.r];
	uint64_t p = t.begin + a.ri_rec[3 * t.g];
	for (uint32_t i = 0; i < cnt; i++) {
		uint32_t v = 0;
		dh_code(t.b, T, p, v);
		if (o + i < nlow)
			out[o + i] = (uint8_t) v;
	}
	if (t.s + 1 == hmin) { // where the chain ends: the walk goes on from here
		rd->wpos = p;
		rd->widx = o + cnt;
	}
}

__global__ __launch_bounds__(64) void k_dh_walk(DecodeArgs a)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const RiceDRead *rd = a.ri_drd + r;
	if (!uni(rd->ok) || lane)
		return;
	ReadMeta *m = a.meta + r;
	const DhTab *t = tab_of(a, r);
	const DTab T = global_tab(t);
	DBits b;
	b.in = a.in + a.in_off[r] + m->hdr + m->seclen + t->tablen;
	b.len = rd->paylen;
	const uint64_t nlow = rd->nlow;
	uint8_t *out = a.low + a.off[r];
	uint64_t idx = rd->widx, p = rd->wpos;
	uint32_t walked = 0;
	while (idx < nlow) {
		uint32_t v;
		if (!dh_code(b, T, p, v)) { // bits that are no code, or the payload ends before nlow values are out
			m->status = 1;
			break;
		}
		out[idx++] = (uint8_t) v;
		walked++;
	}
	if (walked)
		atomicAdd(&a.ri_ctl[3], walked);
}

// ------------------------------------------------------------------ launchers

// behind k_low_encode_chunked<false>; need != NULL: the sizes alone
void launch_dhuf_encode(const BatchArgs &a, uint64_t *need, hipStream_t s)
{
	const uint32_t grid = (uint32_t) (((uint64_t) a.max_chunks * RICE_UPC + 3) / 4);
	(void) hipMemsetAsync(a.dh_tab, 0, (size_t) a.nreads * DH_PRESS_TAB, s);
	hipLaunchKernelGGL(k_dh_hist, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_tree, dim3(a.nreads), dim3(64), 0, s, a, need);
	if (need)
		return;
	hipLaunchKernelGGL(k_dh_count, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_scan, dim3(a.nreads), dim3(64), 0, s, a);
	(void) hipMemsetAsync(a.ri_pay, 0, a.ri_pay_bytes, s);
	hipLaunchKernelGGL(k_dh_write, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_copy, dim3(grid), dim3(256), 0, s, a);
}

// behind k_ex_parse: tables and payloads -> a.low
void launch_dhuf_decode(const DecodeArgs &a, hipStream_t s)
{
	(void) hipMemsetAsync(a.ri_ctl, 0, RICE_CTL_WORDS * 4, s);
	hipLaunchKernelGGL(k_dh_table, dim3(a.nreads), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_dh_dplan, dim3((a.nreads + 255) / 256), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_sync, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_fix<1>, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	// (the later rounds share a counter.  Two rounds left 77 158 values of bench.py's batch to the walk, which then set the
	// call's time; a round costs a launch that reads the records)
	for (int round = 2; round <= DH_FIX_ROUNDS; round++)
		hipLaunchKernelGGL(k_dh_fix<2>, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_check, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_dscan, dim3(a.nreads), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_dh_emit, dim3(a.ri_max_tiles), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_walk, dim3(a.nreads), dim3(64), 0, s, a);
}

} // namespace ph
