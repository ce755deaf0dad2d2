// press_table.hip - the static Huffman table: the device form of the 256 {length, code bits} pairs, the table file, and
// the huffman.h objects (press/huffman/huffman.h) the reference's callers hold.

#include <stdlib.h>

#include <vector>

#include "press_host.h"

using namespace ph;

// ---- static Huffman table -> device form ----
// the delta a one-byte value stands for (zig-zag undone): 0, -1, 1, -2, ... -128
static inline int32_t unzz8(uint32_t z) { return (int32_t) (z >> 1) ^ -(int32_t) (z & 1u); }

int ph::upload_table(const uint32_t len[256], const uint64_t bits[256])
{
	if (g.have_table && !memcmp(len, g.tlen, sizeof g.tlen) && !memcmp(bits, g.tbits, sizeof g.tbits))
		return 0;
	std::vector<HuffDev> hv(1);
	HuffDev &h = hv[0];
	memset(&h, 0xFF, sizeof h); // lut = 0xFFFF, child/leaf = -1
	int nnodes = 1, ncoded = 0;
	bool needs_trie = false;
	for (int s = 0; s < 256; s++) {
		const uint32_t l = len[s];
		if (l > 24) // huffman.c takes codes of up to 255 bits; the device tables stop at 24 (press_hip.h)
			return set_error(PRESS_HIP_EARG, "Huffman table: symbol %d has a code of %u bits (at most 24)", s, l);
		if (l == 0) { // a table file may list fewer than 256 symbols (huffman.c:549): such a symbol
			h.enc[s] = 0; // has no code, and a read fails only if the symbol occurs (k_ex_scan_chunked)
			continue;
		}
		ncoded++;
		h.enc[s] = (uint32_t) (bits[s] & 0xFFFFFFu) | (l << 24);
		int p = 0;
		for (uint32_t k = 0; k < l; k++) {
			const int b = (int) ((bits[s] >> k) & 1);
			if (h.leaf[p] >= 0)
				return set_error(PRESS_HIP_EARG, "Huffman table: not a prefix code");
			if (h.child[p][b] < 0) {
				if (nnodes >= 1024)
					return set_error(PRESS_HIP_EARG, "Huffman table: too many nodes");
				h.child[p][b] = (int16_t) nnodes++;
			}
			p = h.child[p][b];
		}
		if (h.child[p][0] >= 0 || h.child[p][1] >= 0)
			return set_error(PRESS_HIP_EARG, "Huffman table: not a prefix code");
		h.leaf[p] = (int16_t) s;
		if (l <= (uint32_t) HUF_LUT_BITS) {
			const uint32_t step = 1u << l;
			for (uint32_t i = (uint32_t) bits[s] & (step - 1); i < (1u << HUF_LUT_BITS); i += step)
				h.lut[i] = (uint16_t) (s | (l << 8));
		}
	}
	// second-level tables for the long codes, grouped by their first HUF_LUT_BITS bits
	{
		int nid = 0;
		uint32_t used = 0;
		int id_of[1 << HUF_LUT_BITS];
		for (int i = 0; i < (1 << HUF_LUT_BITS); i++)
			id_of[i] = -1;
		uint32_t depth[256] = { 0 };
		int prefix_of[256];
		for (int s = 0; s < 256; s++) {
			if (len[s] <= (uint32_t) HUF_LUT_BITS)
				continue;
			const int pfx = (int) (bits[s] & ((1u << HUF_LUT_BITS) - 1));
			if (id_of[pfx] < 0 && nid < HUF_L2_IDS) {
				prefix_of[nid] = pfx;
				id_of[pfx] = nid++;
			}
			if (id_of[pfx] >= 0 && len[s] - HUF_LUT_BITS > depth[id_of[pfx]])
				depth[id_of[pfx]] = len[s] - HUF_LUT_BITS;
		}
		// deepest first: every table then starts at a multiple of its own size (the first-level
		// entries of the parallel decoder keep offset / 2 in 11 bits)
		for (uint32_t d = 32; d >= 1; d--) {
			for (int id = 0; id < nid; id++) {
				if (depth[id] != d)
					continue;
				if (d > 12 || used + (1u << d) > (uint32_t) HUF_L2_ENTRIES)
					continue; // does not fit: this prefix keeps 0xFFFF and walks the trie
				h.l2off[id] = (uint16_t) used;
				h.l2bits[id] = (uint8_t) d;
				h.lut[prefix_of[id]] = (uint16_t) (0x8000u | (uint32_t) id);
				used += 1u << d;
			}
		}
		for (int s = 0; s < 256; s++) {
			if (len[s] <= (uint32_t) HUF_LUT_BITS)
				continue;
			const int pfx = (int) (bits[s] & ((1u << HUF_LUT_BITS) - 1));
			const int id = id_of[pfx];
			if (id < 0 || h.lut[pfx] != (uint16_t) (0x8000u | (uint32_t) id))
				continue;
			const uint32_t rest = (uint32_t) (bits[s] >> HUF_LUT_BITS), rl = len[s] - HUF_LUT_BITS;
			for (uint32_t i = rest; i < (1u << depth[id]); i += 1u << rl)
				h.lut2[h.l2off[id] + i] = (uint16_t) (s | (len[s] << 8));
		}
		// does any code need the trie (a long code whose prefix got no second-level table)?  If none does, the
		// kernels run without it (their TRIE = false variants) and a prefix that is no code at all points at a
		// second-level slot that says so
		needs_trie = used > HUF_L2_NONE; // (the slot must be free)
		for (int s = 0; s < 256; s++) {
			if (len[s] <= (uint32_t) HUF_LUT_BITS)
				continue;
			const int pfx = (int) (bits[s] & ((1u << HUF_LUT_BITS) - 1));
			const int id = id_of[pfx];
			if (id < 0 || h.lut[pfx] != (uint16_t) (0x8000u | (uint32_t) id))
				needs_trie = true;
		}
		for (int i = 0; i < HUF_L2_ENTRIES; i++) {
			const uint32_t e2 = h.lut2[i];
			h.l2ld[i] = e2 == 0xFFFFu ? (uint16_t) 0xFFFFu : (uint16_t) ((e2 >> 8) | ((unzz8(e2 & 0xFFu) & 0xFFu) << 8));
		}
	}
	// two-symbol table
	for (uint32_t i = 0; i < (1u << HUF_LUT_BITS); i++) {
		const uint16_t e1 = h.lut[i];
		if (e1 == 0xFFFFu) {
			h.lut32[i] = needs_trie ? 0xFFFFFFFFu : (HUF_LONG | HUF_L2_NONE);
		} else if (e1 & 0x8000u) { // a long code's prefix: where its second-level table sits
			const uint32_t id = e1 & 0xFFu;
			h.lut32[i] = HUF_LONG | ((uint32_t) h.l2bits[id] << 12) | h.l2off[id];
		} else {
			// (the parallel decoder stages the delta a symbol stands for, not the symbol)
			const uint32_t s1 = (uint32_t) unzz8(e1 & 0xFFu) & 0xFFu, l1 = e1 >> 8;
			uint32_t v = s1 | (l1 << 8) | (l1 << 24);
			const uint32_t rest = (uint32_t) HUF_LUT_BITS - l1;
			const uint16_t e2 = h.lut[i >> l1]; // the upper bits are zeros, not stream bits:
			if (e2 != 0xFFFFu && !(e2 & 0x8000u) && (uint32_t) (e2 >> 8) <= rest) // only a code that fits counts
				v = s1 | ((l1 + (e2 >> 8)) << 8) | (((uint32_t) unzz8(e2 & 0xFFu) & 0xFFu) << 16) | (l1 << 24) | HUF_TWO;
			h.lut32[i] = v;
		}
	}
	// every whole code that fits in the first HUF_LUT_BITS bits, lengths and deltas (k_huf_sync)
	for (uint32_t i = 0; i < (1u << HUF_LUT_BITS); i++) {
		uint32_t pos = 0, n = 0, len1 = 0;
		int32_t d1 = 0, dsum = 0;
		for (;;) {
			const uint16_t e1 = h.lut[i >> pos]; // the upper bits are zeros, not stream bits:
			if (e1 == 0xFFFFu || (e1 & 0x8000u) || pos + (uint32_t) (e1 >> 8) > (uint32_t) HUF_LUT_BITS)
				break; // only a code that fits counts
			const int32_t d = (int32_t) unzz8(e1 & 0xFFu);
			if (!n) {
				len1 = e1 >> 8;
				d1 = d;
			}
			dsum += d;
			pos += e1 >> 8;
			n++;
			if (pos == (uint32_t) HUF_LUT_BITS || n == HUF_M_MAXN)
				break;
		}
		const uint16_t e0 = h.lut[i];
		if (n)
			h.mlut[i] = pos | (n << 4) | (len1 << 8) | (((uint32_t) d1 & 0xFFu) << 12) | (((uint32_t) dsum & 0x7FFu) << 20);
		else if (e0 != 0xFFFFu && (e0 & 0x8000u)) // long code: second-level table of lengths and deltas
			h.mlut[i] = HUF_MLONG | (uint32_t) h.l2off[e0 & 0xFFu] | ((uint32_t) h.l2bits[e0 & 0xFFu] << 12);
		else
			h.mlut[i] = needs_trie ? 0xFFFFFFFFu : (HUF_MLONG | HUF_L2_NONE);
		// the accumulator form (k_huf_sync's lean loop) and the first code alone (its careful loop)
		h.alut[i] = n ? (pos | (n << HUF_A_CNT) | (((uint32_t) dsum & 0x7FFFu) << HUF_A_SUM)) : h.mlut[i];
		h.flut[i] = n ? (uint16_t) (len1 | (((uint32_t) d1 & 0xFFu) << 8)) : (uint16_t) 0;
	}
	if (!ncoded)
		return set_error(PRESS_HIP_EARG, "Huffman table: no symbol has a code");
	h.minlen = 64;
	h.maxlen = 0;
	for (int s = 0; s < 256; s++) {
		if (!len[s])
			continue;
		h.minlen = len[s] < h.minlen ? len[s] : h.minlen;
		h.maxlen = len[s] > h.maxlen ? len[s] : h.maxlen;
	}
	// Batches already enqueued on the current stream read the table that is on the device now: wait for them before it is
	// overwritten (the copy below is null-stream work, which a non-blocking stream is not ordered against).  The copy is
	// complete when hipMemcpy returns, so whatever is enqueued afterwards, on any stream, sees the new table.
	HIPCHK(hipStreamSynchronize(g.stream()));
	if (g.huff.reserve(sizeof(HuffDev)))
		return PRESS_HIP_EHIP;
	HIPCHK(hipMemcpy(g.huff.p, &h, sizeof h, hipMemcpyHostToDevice));
	memcpy(g.tlen, len, sizeof g.tlen);
	memcpy(g.tbits, bits, sizeof g.tbits);
	g.tmin = h.minlen;
	g.tmax = h.maxlen;
	g.table_trie = needs_trie;
	g.have_table = true;
	return 0;
}

namespace {
int parse_table_file(FILE *fp, uint32_t len[256], uint64_t bits[256]);
}

extern "C" int press_hip_set_table(const uint32_t len[256], const uint64_t bits[256])
{
	API_ENTER;
	return upload_table(len, bits);
}

extern "C" int press_hip_load_table_file(const char *path)
{
	uint32_t len[256];
	uint64_t bits[256];
	FILE *fp = fopen(path, "rb");
	if (!fp)
		return set_error(PRESS_HIP_EARG, "cannot open %s", path);
	int rc = parse_table_file(fp, len, bits);
	fclose(fp);
	if (rc)
		return rc;
	return press_hip_set_table(len, bits);
}

// ------------------------------------------------------------------ huffman.h objects (press/huffman/huffman.h)

namespace {

huffman_node *new_node(bool leaf, unsigned char sym)
{
	huffman_node *p = (huffman_node *) calloc(1, sizeof *p);
	if (!p)
		return nullptr;
	p->isLeaf = leaf ? 1 : 0;
	if (leaf)
		p->symbol = sym;
	return p;
}

// File format (huffman.c:427-439, :549): u32 BE entry count, u32 BE byte count, then per
// entry {u8 symbol, u8 numbits, ceil(numbits/8) code bytes; bit k of the code at bit k%8
// of byte k/8, bit 0 next to the root}.
int parse_table_file(FILE *fp, uint32_t len[256], uint64_t bits[256])
{
	unsigned char hd[8];
	memset(len, 0, 256 * sizeof len[0]);
	memset(bits, 0, 256 * sizeof bits[0]);
	if (fread(hd, 1, 8, fp) != 8)
		return set_error(PRESS_HIP_EARG, "Huffman table: short header");
	uint32_t count = ((uint32_t) hd[0] << 24) | ((uint32_t) hd[1] << 16) | ((uint32_t) hd[2] << 8) | hd[3];
	if (count > 256)
		return set_error(PRESS_HIP_EARG, "Huffman table: %u entries", count);
	for (uint32_t i = 0; i < count; i++) {
		int sym = fgetc(fp), nb = fgetc(fp);
		if (sym == EOF || nb == EOF || nb == 0 || nb > 64)
			return set_error(PRESS_HIP_EARG, "Huffman table: bad entry %u", i);
		unsigned char code[8] = { 0 };
		if (fread(code, 1, (size_t) (nb + 7) / 8, fp) != (size_t) (nb + 7) / 8)
			return set_error(PRESS_HIP_EARG, "Huffman table: truncated");
		uint64_t b = 0;
		for (int k = 0; k < nb; k++)
			if (code[k / 8] & (1u << (k % 8)))
				b |= 1ull << k;
		len[sym] = (uint32_t) nb;
		bits[sym] = b;
	}
	return 0;
}

void collect_codes(const huffman_node *p, uint64_t code, uint32_t depth, uint32_t len[256], uint64_t bits[256])
{
	if (!p || depth > 64)
		return;
	if (p->isLeaf) {
		len[p->symbol] = depth;
		bits[p->symbol] = code;
		return;
	}
	collect_codes(p->zero, code, depth + 1, len, bits);
	collect_codes(p->one, code | (depth < 64 ? 1ull << depth : 0), depth + 1, len, bits);
}

} // namespace

int ph::table_from_encoder(SymbolEncoder *se)
{
	API_LOCK;
	uint32_t len[256];
	uint64_t bits[256];
	if (!se)
		return set_error(PRESS_HIP_EARG, "NULL SymbolEncoder");
	for (int s = 0; s < 256; s++) {
		const huffman_code *c = (*se)[s];
		len[s] = 0;
		bits[s] = 0;
		if (!c)
			continue;
		len[s] = (uint32_t) c->numbits;
		for (unsigned long k = 0; k < c->numbits && k < 64; k++)
			if (c->bits[k / 8] & (1u << (k % 8)))
				bits[s] |= 1ull << k;
	}
	int rc = ctx_init();
	return rc ? rc : upload_table(len, bits);
}

int ph::table_from_tree(huffman_node *root)
{
	API_LOCK;
	uint32_t len[256];
	uint64_t bits[256];
	if (!root)
		return set_error(PRESS_HIP_EARG, "NULL Huffman tree");
	memset(len, 0, sizeof len);
	memset(bits, 0, sizeof bits);
	collect_codes(root, 0, 0, len, bits);
	int rc = ctx_init();
	return rc ? rc : upload_table(len, bits);
}

extern "C" bool read_code_table(FILE *in, huffman_node **rootOut, unsigned int *dataBytesOut)
{
	uint32_t len[256];
	uint64_t bits[256];
	if (!in || !rootOut)
		return false;
	long at = ftell(in);
	unsigned char hd[8];
	if (fread(hd, 1, 8, in) != 8)
		return false;
	if (dataBytesOut)
		*dataBytesOut = ((uint32_t) hd[4] << 24) | ((uint32_t) hd[5] << 16) | ((uint32_t) hd[6] << 8) | hd[7];
	if (fseek(in, at, SEEK_SET) || parse_table_file(in, len, bits))
		return false;
	huffman_node *root = new_node(false, 0);
	if (!root)
		return false;
	for (int s = 0; s < 256; s++) {
		if (!len[s])
			continue;
		huffman_node *p = root;
		for (uint32_t k = 0; k < len[s]; k++) {
			const bool one = (bits[s] >> k) & 1;
			if (p->isLeaf) { // a code runs through another one (huffman.c:643)
				free_huffman_tree(root);
				return false;
			}
			huffman_node **slot = one ? &p->one : &p->zero;
			if (!*slot) {
				*slot = new_node(k + 1 == len[s], (unsigned char) s);
				if (!*slot) {
					free_huffman_tree(root);
					return false;
				}
				(*slot)->parent = p;
			}
			p = *slot;
		}
	}
	*rootOut = root;
	return true;
}

extern "C" void build_symbol_encoder(huffman_node *subtree, SymbolEncoder *pSF)
{
	if (!subtree || !pSF)
		return;
	if (!subtree->isLeaf) {
		build_symbol_encoder(subtree->zero, pSF);
		build_symbol_encoder(subtree->one, pSF);
		return;
	}
	// walk up to the root to get the length, then fill the bits from the root down
	unsigned long nb = 0;
	for (const huffman_node *p = subtree; p->parent; p = p->parent)
		nb++;
	huffman_code *c = (huffman_code *) malloc(sizeof *c);
	c->numbits = nb;
	c->bits = (unsigned char *) calloc((nb + 7) / 8 + 1, 1);
	unsigned long k = nb;
	for (const huffman_node *p = subtree; p->parent; p = p->parent) {
		k--;
		if (p == p->parent->one)
			c->bits[k / 8] |= (unsigned char) (1u << (k % 8));
	}
	(*pSF)[subtree->symbol] = c;
}

extern "C" void free_encoder(SymbolEncoder *pSE)
{
	if (!pSE)
		return;
	for (int s = 0; s < 256; s++) {
		huffman_code *c = (*pSE)[s];
		if (c) {
			free(c->bits);
			free(c);
		}
	}
	free(pSE);
}

extern "C" void free_huffman_tree(huffman_node *subtree)
{
	if (!subtree)
		return;
	if (!subtree->isLeaf) {
		free_huffman_tree(subtree->zero);
		free_huffman_tree(subtree->one);
	}
	free(subtree);
}

