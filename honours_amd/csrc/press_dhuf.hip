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
// Units, the staged writer, subsequences, tiles, records and the repair scheme are the prefix-code engine's
// (press_prefix.h), which the kernels below wrap with the policy DhufCode; a.ri_sum holds a unit's bits in the first of
// its eight words, a.ri_k the longest codes.  The family's own:
//   k_dh_hist    per unit: the 256 counts in LDS, added to the read's 256 words (a.dh_tab, zeroed by the launcher)
//   k_dh_tree    per read, one wave: the sorted list in LDS, at most 255 merge steps (the insertion point by ballot,
//                the nodes in front of it move down one place), the codes by walking up from every leaf; the table's
//                bytes, nbits, the exact length and the slot check; press writes the table into the slot
//   k_dh_count   per unit the sum of its values' code lengths
//   k_dh_write   the read's codes to LDS, and per value its code of up to 63 bits through the engine's writer
//   k_dh_table   per read, one wave: the table's bytes to LDS, the entries parsed and checked (definition 4 of 2v), sorted
//                by their left-aligned codes - neighbours tell whether the code is prefix-free -, then the read's decode
//                table (DhTab): a direct look-up by the next DH_W bits, and the sorted list for a binary search where
//                the direct entry says "longer"
//   dh_code      one code by look-up: the decoder's state is the read's DhTab, which the workgroup of a tile kernel loads
//                to LDS (k_dh_fix: only if a lane has work); the walk reads it in scratch
// PRESS: hist, tree, count, scan, write, copy (behind section and table).  PRESS SIZES (need != NULL): hist and tree alone.
// PACKED PRESS: the sizes, and once the arena is laid out k_dh_place (the slot check and the table), count, scan, write, copy.
// DEPRESS: table, dplan (the reads whose table says there is a payload to decode), sync, fix x 4 (the first round counts
// into ri_ctl[1], the later ones into ri_ctl[2]), check, dscan, emit, walk.  Bits that are no code end a record early
// (end = PFX_SAT) with the codes in front of them kept; in the walk they, or a code that runs past the payload's end,
// refuse the read (ReadMeta::status, in front of k_chunk_prep_meta).

#include "press_prefix.h"

namespace ph {

namespace {

constexpr uint32_t DH_LONG = 0xFFFFu; // direct entry: the code is longer than DH_W bits
constexpr uint32_t DH_RAW = 2568;     // bytes of the longest table, 5 + 256 * 10, rounded up
constexpr int DH_FIX_ROUNDS = 4;      // launches of k_dh_fix

__device__ __forceinline__ uint64_t *press_codes(const BatchArgs &a, uint32_t r)
{
	return reinterpret_cast<uint64_t *>(a.dh_tab + (size_t) r * DH_PRESS_TAB);
}
__device__ __forceinline__ uint32_t *press_hist(const BatchArgs &a, uint32_t r)
{
	return reinterpret_cast<uint32_t *>(a.dh_tab + (size_t) r * DH_PRESS_TAB + 2048);
}
__device__ __forceinline__ DhTab *tab_of(const DecodeArgs &a, uint32_t r) { return reinterpret_cast<DhTab *>(a.dh_tab) + r; }

// the read's decode table, in scratch or in LDS
struct DTab {
	const uint64_t *lcode;
	const uint16_t *ent;
	const uint16_t *direct;
	uint32_t nent;
};

// one code from p on: p moves behind it, v = its symbol; false: the bits are no code, or the code ends behind the payload
__device__ __forceinline__ bool dh_code(const PfxBits &b, const DTab &T, uint64_t &p, uint32_t &v)
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

struct LdsTab {
	uint64_t lcode[256];
	uint16_t ent[256];
	uint16_t direct[1u << DH_W];
};

struct DhufCode {
	static constexpr uint32_t FIRST_BIT = 0;
	static constexpr bool LDS_STATE = true, KEEP_PARTIAL = true, STRICT_END = true;
	typedef DTab State;
	static __device__ __forceinline__ uint32_t press_extra(const PfxRead &rd) { return rd.tablen; }
	static __device__ __forceinline__ bool takes_part(const DecodeArgs &a, uint32_t r) { return tab_of(a, r)->mode == 0; }
	static __device__ __forceinline__ uint32_t extra(const DecodeArgs &a, uint32_t r) { return tab_of(a, r)->tablen; } // (k_dh_table: the table lies inside the stream)
	static __device__ __forceinline__ uint32_t plan_k(const uint8_t *, uint64_t) { return 0; }
	// the read's table -> LDS, by the whole workgroup
	static __device__ __forceinline__ State tile_state(const DecodeArgs &a, uint32_t r)
	{
		__shared__ LdsTab l;
		const DhTab *t = tab_of(a, r);
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
		return { l.lcode, l.ent, l.direct, nent };
	}
	static __device__ __forceinline__ State read_state(const DecodeArgs &a, uint32_t r)
	{
		const DhTab *t = tab_of(a, r);
		return { t->lcode, t->ent, t->direct, t->nent };
	}
	template <bool BOUNDED> // (a code has at most 63 bits: every caller's time is bounded)
	static __device__ __forceinline__ bool code(const PfxBits &b, const State &T, uint64_t &p, uint32_t &v)
	{
		return dh_code(b, T, p, v);
	}
};

} // namespace

__global__ __launch_bounds__(256) void k_dh_hist(BatchArgs a)
{
	__shared__ uint32_t s_h[4][256];
	const uint32_t lane = threadIdx.x & 63;
	uint32_t *h = s_h[threadIdx.x >> 6];
	PfxUnit x;
	if (!unit_of(a, x))
		return;
	for (uint32_t i = lane; i < 256; i += 64)
		h[i] = 0;
	__builtin_amdgcn_wave_barrier();
	const uint8_t *in = a.low_tmp + x.soff + x.v0;
	for (uint32_t step = 0; step < PFX_UNIT; step += 512) {
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
		a.out_len[r] = ok ? total : PFX_FAIL64;
	rd->nbits = nbits;
	rd->paylen = paylen;
	rd->tablen = tablen;
	rd->maxlen = maxlen;
	rd->ok = ok ? 1 : 0;
	rd->nlow = (uint32_t) nlow;
	rd->nunits = (uint32_t) ((nlow + PFX_UNIT - 1) / PFX_UNIT);
	rd->nsym = nsym;
	if (a.ri_k)
		a.ri_k[r] = ok ? (uint8_t) maxlen : (uint8_t) 0;
}

// The packed press's write half (launch_dhuf_write_sized), one wave per read; lane l owns the symbols 4 l .. 4 l + 3.
// Behind k_dh_tree's sizes mode, which left the codes and counts in dh_tab and the lengths in ri_rd, and behind
// k_ex_section against the laid-out slot.  What k_dh_tree's press mode does last: the slot check, out_len, ok, and the
// table behind the section - from the codes as they lie, no tree is built again.
__global__ __launch_bounds__(64) void k_dh_place(BatchArgs a)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	const ReadMeta *m = a.meta + r;
	PfxRead *rd = a.ri_rd + r;
	if (!uni(rd->ok))
		return; // (refused by the size half: k_ex_section has refused it too)
	if (uni(m->status) != 0) { // a slot of no bytes: the read does not fit out_cap
		if (lane == 0)
			rd->ok = 0;
		return;
	}
	const uint32_t tablen = uni(rd->tablen), nlow = uni(rd->nlow), nsym = uni(rd->nsym);
	const uint64_t total = (uint64_t) m->hdr + m->seclen + tablen + uni64(rd->paylen);
	const bool ok = total <= a.out_off[r + 1] - a.out_off[r];
	if (ok) {
		const uint64_t *codes = press_codes(a, r);
		const uint32_t *hist = press_hist(a, r);
		uint32_t c[4], len[4], tbytes = 0;
		uint64_t bits[4];
#pragma unroll
		for (uint32_t j = 0; j < 4; j++) {
			const uint64_t cw = codes[lane * 4 + j];
			c[j] = hist[lane * 4 + j];
			len[j] = (uint32_t) (cw >> 56);
			bits[j] = cw & 0x00FFFFFFFFFFFFFFull;
			if (c[j])
				tbytes += 2 + (len[j] + 7) / 8;
		}
		const uint32_t inc = scan32(tbytes, lane);
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
	a.out_len[r] = ok ? total : PFX_FAIL64;
	rd->ok = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_dh_count(BatchArgs a)
{
	__shared__ uint8_t s_len[4][256];
	const uint32_t lane = threadIdx.x & 63;
	uint8_t *ln = s_len[threadIdx.x >> 6];
	PfxUnit x;
	if (!unit_of(a, x))
		return;
	if (!uni(a.ri_rd[x.r].ok))
		return;
	const uint64_t *codes = press_codes(a, x.r);
	for (uint32_t i = lane; i < 256; i += 64)
		ln[i] = (uint8_t) (codes[i] >> 56);
	__builtin_amdgcn_wave_barrier();
	const uint8_t *in = a.low_tmp + x.soff + x.v0;
	uint32_t L = 0;
	for (uint32_t step = 0; step < PFX_UNIT; step += 512) {
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

// one wave per read: the units' first bits
__global__ __launch_bounds__(64) void k_dh_scan(BatchArgs a)
{
	const uint32_t r = blockIdx.x;
	const PfxRead *rd = a.ri_rd + r;
	if (!rd->ok)
		return;
	prefix_unit_scan(a, r, rd->nunits, DhufCode::FIRST_BIT, [&](size_t entry, uint32_t) -> uint64_t { return a.ri_sum[entry * 8]; });
}

__global__ __launch_bounds__(256) void k_dh_write(BatchArgs a)
{
	__shared__ uint32_t s_bits[4][PFX_WIN];
	__shared__ uint64_t s_code[4][256];
	const uint32_t lane = threadIdx.x & 63;
	uint64_t *code = s_code[threadIdx.x >> 6];
	PfxUnit x;
	if (!unit_of(a, x))
		return;
	if (!uni(a.ri_rd[x.r].ok))
		return;
	const uint64_t *codes = press_codes(a, x.r);
	for (uint32_t i = lane; i < 256; i += 64)
		code[i] = codes[i];
	__builtin_amdgcn_wave_barrier();
	prefix_write(
		a, x, s_bits[threadIdx.x >> 6], [&](uint32_t b) { return (uint32_t) (code[b] >> 56); },
		[&](auto &put, uint64_t &p, uint32_t b) {
			const uint64_t cw = code[b];
			const uint32_t l = (uint32_t) (cw >> 56);
			if (l) // a code of up to 63 bits crosses up to three dwords
				put(p, (uint32_t) cw, l < 32 ? l : 32u);
			if (l > 32)
				put(p + 32, (uint32_t) (cw >> 32) & 0x00FFFFFFu, l - 32);
			p += l;
		});
}

// (PFX_COPY bytes per unit index cover every payload: at most eight bits a value on average - the fixed eight-bit code
// is a prefix code, and the Huffman code is no longer)
__global__ __launch_bounds__(256) void k_dh_copy(BatchArgs a) { prefix_copy<DhufCode>(a); }

// ------------------------------------------------------------------ depress

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

__global__ __launch_bounds__(256) void k_dh_dplan(DecodeArgs a) { prefix_dplan<DhufCode>(a); }
__global__ __launch_bounds__(256) void k_dh_sync(DecodeArgs a) { prefix_sync<DhufCode>(a); }
template <int CTR> // counts into ri_ctl[CTR]
__global__ __launch_bounds__(256) void k_dh_fix(DecodeArgs a)
{
	prefix_fix<DhufCode>(a, CTR);
}
__global__ __launch_bounds__(256) void k_dh_check(DecodeArgs a) { prefix_check<DhufCode>(a); }
__global__ __launch_bounds__(64) void k_dh_dscan(DecodeArgs a) { prefix_dscan(a); }
__global__ __launch_bounds__(256) void k_dh_emit(DecodeArgs a) { prefix_emit<DhufCode>(a); }
__global__ __launch_bounds__(64) void k_dh_walk(DecodeArgs a) { prefix_walk<DhufCode>(a); }

// ------------------------------------------------------------------ launchers

// behind k_low_encode_chunked<false>; need != NULL: the sizes alone
void launch_dhuf_encode(const BatchArgs &a, uint64_t *need, hipStream_t s)
{
	const uint32_t grid = (uint32_t) (((uint64_t) a.max_chunks * PFX_UPC + 3) / 4);
	ex_stage_sized();
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

// the packed press's write half: behind launch_dhuf_encode(need != NULL) and k_ex_section; no histogram, no tree
void launch_dhuf_write_sized(const BatchArgs &a, hipStream_t s)
{
	const uint32_t grid = (uint32_t) (((uint64_t) a.max_chunks * PFX_UPC + 3) / 4);
	hipLaunchKernelGGL(k_dh_place, dim3(a.nreads), dim3(64), 0, s, a);
	hipLaunchKernelGGL(k_dh_count, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_scan, dim3(a.nreads), dim3(64), 0, s, a);
	(void) hipMemsetAsync(a.ri_pay, 0, a.ri_pay_bytes, s);
	hipLaunchKernelGGL(k_dh_write, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(k_dh_copy, dim3(grid), dim3(256), 0, s, a);
}

// behind k_ex_parse: tables and payloads -> a.low
void launch_dhuf_decode(const DecodeArgs &a, hipStream_t s)
{
	(void) hipMemsetAsync(a.ri_ctl, 0, PFX_CTL_WORDS * 4, s);
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
