// press_internal.h - shared between the kernel files (press_*.hip) and the C-ABI
// host layer (press_host.h and its units).  Not installed; the public interface is include/press_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ph {

// Exception-section encodings of the "vb1e2" family (press.c:2679-3405) and ex-zd (ex_zd.c:9).
enum ExFmt : int {
	EXF_VBE21 = 0,   // nex x u32 pos, nex x u16 raw value
	EXF_VBBE21 = 1,  // bit-packed position deltas, bit-packed (value-256)
	EXF_VBSBE21 = 2, // svb32 position deltas, bit-packed (value-256)
	EXF_VBSSE21 = 3, // svb32 position deltas, svb16 (value-256)
	EXF_EXZD = 4     // svb32 position deltas, svb32 (value-256); one exception = 2 x u32
};
// The entropy stage of an exception-split method: what codes the one-byte values behind the section.  The numbers stand in
// the rows of METHODS[] (press_host.h) and index EX_STAGES[] below.
enum ExEnt : int {
	ENT_PLAIN, // none: the values themselves
	ENT_SHUFF, // the static Huffman table (press_huffman.hip)
	ENT_RC,    // range coder of order 0 (press_rc.hip)
	ENT_RCC,   // ... of order 1
	ENT_RCM,   // ... mixing orders 1 and 0
	ENT_CDF,   // the adaptive nibble-CDF coder (press_cdf.hip)
	ENT_RICE,  // Golomb-Rice (press_rice.hip)
	ENT_DHUF,  // a Huffman code per read (press_dhuf.hip)
	ENT_COUNT
};
// ... and what k_ex_section, k_ex_sizes and k_ex_parse have to know about that stream
enum ExPayload : int {
	PAY_INLINE, // the one-byte values, behind the section
	PAY_SHUFF,  // u32 symbol count (big endian) + the static-Huffman payload
	PAY_CODER,  // a coder that sizes its own stream and stores no count: the slot's size is a bound, nlow the room's rest
	PAY_STAGED  // staged and sized by the stage (k_rice_pick, k_dh_tree), spliced behind the section; no count either
};

// Per-read record shared by the passes of the exception-split methods (device memory).
struct ReadMeta {
	uint32_t nex;     // exceptions among zd[1..n)
	uint32_t ored;    // OR of all samples (ex-zd qts, ex_zd.c:358-381)
	uint32_t zd0;     // zd[0], stored raw in the header
	uint32_t q;       // ex-zd shift (0 for the other methods)
	uint32_t hdr;     // bytes in front of the "u32 nex" field: 2, or 12 for ex-zd
	uint32_t seclen;  // bytes of "u32 nex || exception section"
	uint32_t nlow;    // one-byte values in the stream (decode side)
	uint32_t status;  // 0 = ok, anything else = this read failed
};

// Static-Huffman tables on the device (built on the host from the 256 {len,bits} pairs).
constexpr int HUF_LUT_BITS = 12;
constexpr int HUF_L2_ENTRIES = 3072; // the NA12878 table needs 2848
constexpr int HUF_L2_IDS = 64;       // long-code prefixes with a second-level table (the rest walk the trie)
struct HuffDev {
	uint32_t enc[256];                 // code bits (bit k = k-th emitted bit) | len << 24
	uint16_t lut[1 << HUF_LUT_BITS];   // sym | len << 8 for codes <= 12 bits, 0xFFFF: walk the trie
	int16_t child[1024][2];            // binary trie, node 0 = root, -1 = none
	int16_t leaf[1024];                // symbol at a leaf, -1 otherwise
	uint32_t minlen, maxlen;           // shortest / longest code
	// second level for codes longer than HUF_LUT_BITS: lut[prefix] = 0x8000 | id, then
	// lut2[l2off[id] + next l2bits[id] stream bits] = sym | len << 8 (0xFFFF: no such code)
	uint16_t lut2[HUF_L2_ENTRIES];
	uint16_t l2off[256];
	uint8_t l2bits[256];
	// two-symbol first level for the parallel decoder:
	//   d1 | adv << 8 | d2 << 16 | len1 << 24 | HUF_TWO,  adv = len1 + len2 with HUF_TWO (two whole
	//   codes fit in HUF_LUT_BITS bits), else adv = len1 and d2 = 0;  d = the delta the symbol stands for
	//   (zig-zag undone, a signed byte)
	// (the two deltas sit in the low bytes of the two register halves: ds_write_b8 / _d16_hi store
	// them without a shift); a long code's prefix: HUF_LONG | l2bits << 12 | l2off of its
	// second-level table; 0xFFFFFFFF: walk the trie
	alignas(16) uint32_t lut32[1 << HUF_LUT_BITS];
	// first level of k_huf_sync (lengths and sample deltas, no symbols): every whole code that fits in
	// HUF_LUT_BITS bits at once (at most HUF_M_MAXN of them):
	//   total bits | codes << 4 | bits of the first code << 8 | d1 << 12 | dsum << 20
	//   d1 = delta the first code's symbol stands for (8 bits, signed: zig-zag undone), dsum = sum of the
	//   deltas of all codes of the entry (11 bits, signed);
	// a long code's prefix: HUF_MLONG | l2off | l2bits << 12 (length and delta of the code in
	// l2ld[l2off + the next l2bits stream bits]); 0xFFFFFFFF: walk the trie
	alignas(16) uint32_t mlut[1 << HUF_LUT_BITS];
	alignas(16) uint16_t l2ld[HUF_L2_ENTRIES]; // bits of the code | delta << 8 (signed), 0xFFFF: no such code
	// the same first level laid out as an INCREMENT of the scan's one accumulator (position | codes << 9 |
	// delta sum << 16): total bits | codes << HUF_A_CNT | (dsum & 0x7FFF) << HUF_A_SUM - one add per look-up moves
	// position, count and sum (a scan covers at most 64 codes: 7 bits of count, 15 bits of signed sum).  Long
	// codes / no code: as in mlut (the sign bit)
	alignas(16) uint32_t alut[1 << HUF_LUT_BITS];
	// ... and the first code alone, for the last steps in front of a limit: its bits | its delta << 8; 0: none
	alignas(16) uint16_t flut[1 << HUF_LUT_BITS];
};
constexpr uint32_t HUF_A_CNT = 9, HUF_A_SUM = 16;
constexpr uint32_t HUF_NEEDS_TRIE = 0x80000000u; // in DecodeArgs::huf_minlen: some code is beyond the second-level tables
constexpr uint32_t HUF_L2_NONE = HUF_L2_ENTRIES - 1; // second-level slot that says "no code" (tables that need no trie)
constexpr uint32_t HUF_MLONG = 1u << 31; // (the sign bit: one compare)
constexpr uint32_t HUF_M_MAXN = 8; // 8 deltas of -128 .. 127 fit the 11-bit sum
constexpr uint32_t HUF_LONG = 1u << 30;
constexpr uint32_t HUF_TWO = 1u << 29;

// parallel Huffman decode (press_huffman.hip): tiles of HUF_HT subsequences
constexpr int HUF_HT = 256;        // subsequences per tile (a lane each)
struct HufUnit {              // what k_huf_chain leaves per unit (a quarter tile: one wave's work in k_huf_emit), 32 bytes
	uint32_t src_lo;     // arena byte offset of the unit's first payload byte, bits 0 .. 31
	uint32_t src_hi_bz;  // ... bits 32 .. 47 (offsets into device memory) | bz << 16: the sample value in front of the
	                     // unit's first sample, mod 2^16 (for the read's first unit, which writes sample 0: zd[0])
	uint64_t roff;       // the read's slot (DecodeArgs::off)
	uint32_t obase;      // codes of the read in front of the unit (clamped to 2^32 - 1)
	uint32_t qnf;        // quota | nby << 14 | q << 26 | fused << 30: the codes the unit delivers (cut at the read's
	                     // count), payload bytes from src on (clamped to HUF_U_NBY: more than a unit reads), the
	                     // ex-zd shift, 1 = k_huf_emit writes the read's samples itself (0: its one-byte values go to
	                     // DecodeArgs::low and k_low_decode_chunked merges them)
	uint32_t ea, ecnt;   // the unit's exceptions [ea, ea + ecnt) of the read (fused reads with a quota; else 0)
};
static_assert(sizeof(HufUnit) == 32, "HufUnit");
constexpr uint32_t HUF_U_QUOTA = 0x3FFFu, HUF_U_NBY = 0xFFFu; // (a unit delivers at most 64 x 255 codes)
constexpr uint32_t HUF_FUSED = 0x80000000u; // in DecodeArgs::hread[2r + 1]: the read needs no k_low_decode_chunked

// ---- chunked (v2) svb kernels: a read is cut into chunks of CHUNK samples, one workgroup
// per chunk; chunks of a read are chained by a decoupled look-back over 8-byte granules.
constexpr uint32_t CHUNK = 32768;           // samples per chunk: 4 waves x 16 sub-tiles x 512
struct ChunkDesc {                          // written by k_chunk_prep, one per chunk (64 bytes)
	uint64_t sig_off;   // sample offset of the READ in sig
	uint64_t out_base;  // byte offset of the read's slot (encode) / stream (decode) in the arena
	uint32_t n;         // samples in the read
	uint32_t j;         // chunk index within the read
	uint32_t read;      // read index
	uint32_t cap_ok;    // slot large enough for the worst case of the format
	// decode only, filled by k_svb_keyscan / k_svb_keyprefix:
	uint64_t ebefore;   // exceptions (extra data bytes) in front of this chunk
	uint32_t ecnt[4];   // exceptions in each wave's quarter of the chunk
	uint16_t kmask[4];  // per wave: sub-tiles that are not plain (exception or ragged tail)
};
static_assert(sizeof(ChunkDesc) == 64, "ChunkDesc is one 64-byte line");
struct ChunkBits {                          // Huffman encode: code bits of a chunk (k_ex_scan_chunked<.., true>, k_ex_prefix)
	uint64_t before;    // bits of the read's payload in front of this chunk
	uint32_t q[4];      // bits of each wave's quarter
	uint32_t pad[2];
};
struct ChunkCtl {                           // device control block; every word on its own 128-B line
	uint32_t ticket;    // next chunk to hand out (atomic)
	uint32_t pad0[31];
	uint32_t nchunks;   // written by k_chunk_prep, read by every workgroup
	uint32_t pad1[31];
	uint32_t ticket2;   // spare second ticket
	uint32_t pad2[31];  // (stays zero: k_low_decode_chunked loads its zeros from here)
	uint32_t lists[32]; // Huffman decode: entries of the list repair round r leaves (the first list's: ticket2)
	uint32_t units;     // Huffman decode: next unit of work k_huf_emit hands out
	uint32_t pad4[31];
	uint32_t sunits;    // ... and k_huf_sync
	uint32_t pad5[31];
};

// The prefix-code engine (press_prefix.h) of the Rice methods (press_rice.hip) and the per-read Huffman methods
// (press_dhuf.hip).  Press: a read's one-byte values in units of PFX_UNIT, a wave each; unit i of a read is entry
// PFX_UPC * first_chunk + i of the unit tables.  Depress: the payload in subsequences of PFX_SUB bits, a lane each, PFX_DT
// of them a tile.  Both families use the buffers BatchArgs::ri_* and DecodeArgs::ri_* and the two records below.
constexpr uint32_t PFX_UNIT = 1024;
constexpr uint32_t PFX_UPC = CHUNK / PFX_UNIT;
constexpr uint32_t PFX_COPY = 1280; // payload bytes per unit index in prefix_copy: more than PFX_UNIT values at nine bits take
constexpr uint32_t PFX_WIN = 256;   // dwords of a writer's LDS window
constexpr uint32_t PFX_SUB = 256;
constexpr uint32_t PFX_DT = 256;
constexpr uint32_t PFX_CTL_WORDS = 16; // DecodeArgs::ri_ctl: tiles; subsequences decoded again by the first fix round, by the later ones; values of the walk
constexpr uint64_t PFX_FAIL64 = ~0ull;
constexpr uint32_t PFX_NONE = 0xFFFFFFFFu; // record: no start known (the subsequence was given up); tile table: an id that is not used
constexpr uint32_t PFX_SAT = 0xFFFFFFFEu;  // record: no end
struct PfxRead {              // press, per read (k_rice_pick / k_dh_tree)
	uint64_t nbits;       // payload bits
	uint64_t paylen;      // ... and bytes
	uint32_t ok;          // 0: refused (k_ex_section), or the slot is too small
	uint32_t nlow, nunits;
	uint32_t k;           // Rice: the parameter
	uint32_t tablen;      // per-read Huffman: bytes of the table in front of the payload
	uint32_t maxlen;      // ... the longest code
	uint32_t nsym;        // ... the symbols present
	uint32_t pad;
};
struct PfxDRead {             // depress, per read (prefix_dplan)
	uint64_t paylen;      // payload bytes
	uint64_t wpos, widx;  // where the serial walk starts: bit, value
	uint32_t k;           // Rice: the parameter (per-read Huffman: 0)
	uint32_t nsubs;       // subsequences decoded in parallel
	uint32_t tile0;       // first tile
	uint32_t nlow;
	uint32_t hmin;        // first subsequence that is not settled (nsubs: none)
	uint32_t ok;          // k_ex_parse accepted the read
};

// The per-read Huffman methods' own (press_dhuf.hip): dh_tab, per read DH_PRESS_TAB bytes for press (256 x { code | len << 56 },
// then the 256 counts), a DhTab for depress.
constexpr uint32_t DH_W = 11;                        // bits of the decoder's direct look-up
constexpr uint32_t DH_PRESS_TAB = 256 * 8 + 256 * 4;
struct DhTab {                // depress, per read (k_dh_table)
	uint64_t lcode[256];  // the codes, first bit on top, ascending
	uint16_t ent[256];    // ... their symbol | len << 8
	uint16_t direct[1u << DH_W]; // by the next DH_W bits: symbol | len << 8, 0: no code, 0xFFFF: a longer code, in lcode
	uint32_t nent;
	uint32_t tablen;      // bytes of the table in front of the payload
	uint32_t mode;        // 0: decode the payload, 1: nothing to decode (no value, or one symbol without a bit), 2: refused
	uint32_t pad;
};
static_assert(sizeof(PfxRead) % 8 == 0 && sizeof(PfxDRead) % 8 == 0 && sizeof(DhTab) % 8 == 0, "arrays of them keep their uint64_t aligned");

// Arguments common to every batch kernel.
struct BatchArgs {
	const int16_t *sig;       // samples of all reads
	const uint64_t *off;      // [nreads] read r starts at sig[off[r]] (multiple of 8 samples)
	const uint32_t *nsamp;    // [nreads] samples in read r
	uint8_t *out;             // compressed arena
	const uint64_t *out_off;  // [nreads+1] slot of read r
	uint64_t *out_len;        // [nreads] bytes produced / UINT64_MAX
	ReadMeta *meta;           // [nreads]
	uint32_t *ex_pos;         // [total samples] exception positions of read r at ex_pos[off[r]..]
	uint32_t *ex_val;         // [total samples] raw exception values
	const HuffDev *huff;
	uint32_t nreads;
	// chunked kernels
	ChunkDesc *chunks;        // [max_chunks]
	uint64_t *gran;           // [max_chunks] look-back granules (zeroed per launch)
	ChunkCtl *ctl;            // zeroed per launch
	uint32_t max_chunks;      // >= sum over reads of ceil(n / CHUNK)
	ChunkBits *cbits;         // [max_chunks] Huffman code-bit counts (NULL for the other methods)
	uint8_t *low_tmp;         // range-coder methods: the one-byte values of read r at low_tmp[off[r]..] (else NULL)
	uint32_t *first_chunk;    // [nreads] id of the first chunk of read r (exception-split encode)
	uint32_t *zhist;          // zstd compositions: [nreads][256] occurrences of the data bytes, counted where the svb
	                          // encoder has them in registers (zeroed by the caller; NULL for the other methods)
	uint32_t *zkcnt;          // ... and [max_chunks] at a read's FIRST chunk: the read's key bytes that are not zero (with zhist;
	                          // their positions and values are listed in ex_pos / ex_val of the read, in order)
	// the Rice and the per-read Huffman methods (press_prefix.h; NULL for the other methods)
	uint32_t *ri_sum;         // [max_chunks * PFX_UPC][8] per unit: Rice: the sums of x >> k; per-read Huffman: its bits, in the first word
	uint64_t *ri_start;       // [max_chunks * PFX_UPC] per unit: its first bit of the read's payload
	PfxRead *ri_rd;           // [nreads]
	uint8_t *ri_pay;          // the staged payloads: read r's at 2 * off[r], ri_pay_bytes in all
	uint64_t ri_pay_bytes;
	uint8_t *ri_k;            // [nreads] the caller's k[] (per-read Huffman: maxlen[]), or NULL
	uint8_t *dh_tab;          // the per-read Huffman methods (press_dhuf.hip): [nreads][DH_PRESS_TAB] codes and counts
};

struct HufTile {             // one tile of a read's Huffman payload (press_huffman.hip), 32 bytes
	uint64_t src;        // byte offset in the compressed arena of the tile's first payload byte
	uint64_t low;        // offset in DecodeArgs::low of the read's one-byte stream
	uint32_t nbits;      // payload bits from the tile's first bit to the end of the payload
	uint32_t t_last;     // tile index in the read | (no tile follows) << 31
	uint32_t read;
	uint32_t want;       // codes the read's header announces
};

struct DecodeArgs {
	const uint8_t *in;        // compressed arena
	const uint64_t *in_off;   // [nreads]
	const uint64_t *in_len;   // [nreads]
	int16_t *sig;             // decoded samples
	const uint64_t *off;      // [nreads] slot of read r starts at sig[off[r]] (multiple of 8 samples)
	const uint32_t *nsamp;    // [nreads] slot capacity in samples (= the sample count for svb streams)
	uint32_t *out_n;          // [nreads] samples decoded / UINT32_MAX
	ReadMeta *meta;
	uint32_t *ex_pos;
	uint32_t *ex_val;
	uint8_t *low;             // [total samples] Huffman- / range-decoded one-byte stream of read r at low[off[r]..]
	const HuffDev *huff;
	uint32_t nreads;
	// chunked kernels
	ChunkDesc *chunks;
	uint64_t *gran;           // [max_chunks] look-back granules of the sample-value chain
	ChunkCtl *ctl;
	uint32_t *first_chunk;    // [nreads] id of the first chunk of read r
	uint32_t max_chunks;
	// Huffman tiles (press_huffman.hip)
	HufTile *htiles;          // [max_htiles]
	HufUnit *hunit;           // [max_htiles * 4] per unit (quarter tile): k_huf_chain's plan for k_huf_emit
	uint32_t *hrec;           // [max_htiles * HUF_HT] one record per subsequence: start | codes << 8 | sum of their deltas << 16
	uint32_t *hlist;          // [2 * hlist_cap] two lists of subsequences to decode again (k_huf_fix)
	uint8_t *hend;            // [max_htiles * HUF_HT] per subsequence: where the next one's first code starts (0 .. 30, 31: none)
	uint32_t *hmin;           // [nreads] first subsequence k_huf_fix's rounds left unsettled (0xFFFFFFFF: none)
	uint32_t *hread;          // [2 * nreads] first tile, number of tiles of read r
	uint2 *hwave;             // [max_htiles * 4] per wave of a tile: its codes, the sum of their deltas (mod 2^16 in the low half)
	unsigned long long *hbits; // [max_htiles * 4] per wave of a tile: the lanes whose guess k_huf_sync found wrong or could not check
	uint32_t max_htiles;
	uint32_t hlist_cap;
	uint32_t huf_minlen;      // shortest code of the table (selects the subsequence size on the host)
	// the Rice and the per-read Huffman methods (press_prefix.h; NULL for the other methods)
	PfxDRead *ri_drd;         // [nreads]
	uint2 *ri_tile;           // [ri_max_tiles] { read, tile of the read }
	uint32_t *ri_rec;         // [ri_max_tiles * PFX_DT][3] per subsequence: start, end, codes
	uint64_t *ri_tbase;       // [2 * ri_max_tiles] per tile: the read's codes in front of it; behind them: the tiles' own counts
	uint32_t *ri_ctl;         // [PFX_CTL_WORDS]; what the last depress of either family left
	uint32_t ri_max_tiles;
	uint8_t *dh_tab;          // the per-read Huffman methods (press_dhuf.hip): [nreads] DhTab
};

// zstd frames on the device (press_zstd.hip, zs_table.h): scratch of one batch
struct ZsRead {               // per read
	uint32_t nk, nd;      // key bytes / data bytes of the svb-zd stream
	uint32_t knz;         // key bytes that are not zero
	uint32_t mode;        // 0: RLE keys + Huffman data, 1: raw blocks, 2: failed
	uint32_t dbase;       // frame offset of the first data block
	uint32_t plen;        // bytes in front of the keys: the count / the ex-zd header and exception section
	uint32_t pad[2];
};
// ZsRead on the decode side: nd = content size of the frame, mode 0 ok / 2 malformed / 3 left to libzstd,
// pad[0] = its first block with sequences + 1 (0: none), knz = 1: the frame's Content_Checksum in pad[1] is yet to be verified
struct ZsCopy {               // content bytes [dst, dst + n) of ztmp: a copy of n bytes at src of the arena, or its byte n times
	uint64_t src, dst;
	uint32_t n, fill;
};
struct ZsHuf {                // Huffman-coded literals of one block
	uint64_t src, dst;    // arena offset of the streams (jump table first) / ztmp offset of the literals
	uint32_t cs, R;       // bytes of the streams, literals
	uint32_t four;        // 4 streams (else 1)
	uint32_t pad;
};
struct ZsUnit {               // up to 8 Huffman blocks of a read with one table: half a wave's work
	uint32_t read, tree, count, pad;
};
struct ZsLong {               // a block with four LONG streams (ZSTD_compress's 128-KiB blocks): a wave of its own, 16 lanes a stream
	ZsHuf h;
	uint32_t tree, read, pad[2];
};
struct ZsTree {
	uint8_t w[256];       // weights (RFC 8878 4.2.1.1)
	uint32_t tl, pad[3];
};
struct ZsSeq {               // one sequence: ll literals, then ml bytes from off bytes back
	uint32_t ll, ml, off;
};
struct ZsXBlk {              // a block with sequences, in the order of its frame
	uint64_t lit;        // ztmp offset of its literals
	uint64_t dst;        // ztmp offset of its content
	uint32_t seq0, nseq; // its sequences in dseq
	uint32_t tail;       // literals behind the last match
	uint32_t next;       // the frame's next such block + 1, 0: none
};
struct ZsDCtl { // every counter on a 4-KB page of its own: they are bumped by all waves of k_zs_walk with returning atomics,
                // which are carried out one after the other per address - and on one cache line, all of them together
	uint32_t ncopy, pad0[1023];
	uint32_t nunits, pad1[1023];
	uint32_t ntrees, pad2[1023]; // trees beyond a read's first (that one is slot r of the tree list)
	uint32_t nseq, pad3[1023];
	uint32_t nxblk, pad4[1023];
	uint32_t nhost, pad5[1023];
	uint32_t nlong, pad6[1023];
};
struct ZsBufs {
	uint8_t *ztmp;        // the svb-zd streams between the two stages: [u32 n][keys][data] of read r at zoff[r]
	uint64_t *zoff;       // [nreads + 1]
	uint64_t *zoff4;      // [nreads + 1] zoff + 4: where the svb kernels write / read
	uint64_t *zlen;       // [nreads] bytes of keys + data
	uint32_t *hist;       // [nreads][256]
	void *tab;            // zs::Table [nreads]
	uint32_t *first_blk;  // [nreads + 1] id of the first data block of read r
	uint32_t *blk_read;   // [max_blocks]
	uint4 *sbits;         // [max_blocks] code bits of the four streams of a block
	uint32_t *bpos;       // [max_blocks] frame offset of the block
	uint8_t *bflag;       // [max_blocks] 1: Huffman, 2: carries the tree, 4: last block of the frame
	uint32_t *kcnt;       // [max_chunks] at a read's first chunk: its key bytes that are not zero (BatchArgs::zkcnt)
	ZsRead *rd;           // [nreads]
	uint32_t *nblocks;    // [1]
	uint32_t max_blocks;
	// decode: what k_zs_walk finds in the frames
	ZsCopy *dcopy;        // [cap_copy] raw / RLE pieces
	ZsHuf *dhuf;          // [cap_units * 8] Huffman blocks, 8 slots per unit
	ZsUnit *dunit;        // [cap_units]
	ZsTree *dtree;        // [cap_trees]
	ZsLong *dlong;        // [cap_long] blocks whose streams are decoded in segments (k_zs_hdecode_long)
	ZsDCtl *dctl;
	uint32_t *zn;         // [nreads] sample count found in the stream
	ZsSeq *dseq;          // [cap_seq] sequences of the frames' blocks
	ZsXBlk *dxblk;        // [cap_xblk]
	uint64_t lit_base;    // ztmp offset of the literals space (read r's at lit_base + zoff[r])
	uint32_t cap_seq, cap_xblk;
	uint32_t cap_copy, cap_units, cap_trees, cap_long;
	uint32_t kdiv;        // samples per key byte of the inner stream: 4 (svb-zd), 8 (svb16-zd), 0: ex-zd (no keys)
};
void launch_zstd_encode(const BatchArgs &a, const ZsBufs &z, hipStream_t s); // press_zstd.hip

// Packed press (press_hip_press_sizes / press_hip_press_packed, press_packed.hip): the library lays the arena out.
// Every family's chain is cut in two: PACK_SIZE runs it up to the point where a read's length is known, writes need[]
// and - with a layout - scans it into the offsets; PACK_WRITE runs the rest against those offsets.  The two halves
// share the batch's scratch (chunk table, ReadMeta, the zstd plan), so nothing else may run between them.
struct PackArgs {
	uint64_t *need;    // [nreads] bytes read r takes (the range coders: an upper bound), PRESS_HIP_FAILED: refused
	uint64_t *layout;  // [nreads + 1] the caller's out_off, written by the scan; NULL: sizes only
	uint64_t *slot;    // [nreads + 1] the slot table the writing kernels see: layout[r] for a read that fits out_cap,
	                   // and for one that does not the next fitting read's offset - a slot of no bytes, which every
	                   // kernel refuses (k_pk_scan)
	uint64_t out_cap;
	uint32_t align;    // a power of two
};
constexpr int PACK_SIZE = 1, PACK_WRITE = 2;
// most a range coder emits beyond the nlow bytes of its input (include/press_hip.h, press_hip_press_sizes)
constexpr uint32_t RC_PACK_SLACK = 32;
void launch_pack_svb_sizes(const BatchArgs &a, bool key2bit, bool zd, bool slow5, uint64_t *need, hipStream_t s); // press_packed.hip
void launch_pack_scan(const PackArgs &pk, uint32_t nreads, hipStream_t s);
void launch_pack_patch(const BatchArgs &a, const uint64_t *slot, hipStream_t s);
// packed recode: need[] = FAILED for the reads the source refused (out_n), then - with pk.layout - the scan, and a slot
// table in which such a read has no byte whatever lies behind it
void launch_pack_scan_refused(const PackArgs &pk, const uint32_t *out_n, uint32_t nreads, hipStream_t s);
void launch_svb_encode_packed(const BatchArgs &a, bool key2bit, bool zd, bool slow5, const PackArgs &pk, int phases, hipStream_t s);
void launch_zstd_encode_packed(const BatchArgs &a, const ZsBufs &z, const PackArgs &pk, int phases, hipStream_t s);
// decode in two steps: frames -> svb-zd streams in ztmp (reads the device leaves to libzstd
// are counted in dctl->nhost and patched in by the caller), then the svb-zd decode
void launch_zstd_decode_frames(const DecodeArgs &a, const ZsBufs &z, hipStream_t s);
void launch_zstd_decode_streams(const DecodeArgs &a, const ZsBufs &z, hipStream_t s);

// Recode (press_hip_recode_batch): where the fused svb decode leaves pass A's results - the chunk table, first-chunk
// list, code-bit counts and ReadMeta of the PRESS half of the call, and its table (k_svb_decode_chunked<.., FUSE>)
struct FuseArgs {
	ChunkDesc *chunks;
	const uint32_t *first_chunk;
	ChunkBits *cbits;
	ReadMeta *meta;
	const HuffDev *huff;
	// k_svb_decode_chunked<.., float> (press_hip_depress_pa_batch): the float arena at the caller's off[], two floats per read
	float *pa;
	const float *cal;
	// k_svb_decode_chunked<.., DEG> (press_hip_recode_degraded_*): degrade_pair's two constants
	uint32_t deg_h2, deg_m2;
};
constexpr uint32_t RECODE_KEEP = 64; // bytes of a refused read's slot kept aside (an empty read's stream is 4 / 16 bytes)
// bits > 0: the decode kernel applies D_bits to the samples it holds, and pass A's results are those of the degraded read
void launch_recode_fused(const DecodeArgs &d, const BatchArgs &p, bool key2bit, bool slow5, ExFmt fmt, ExEnt ent, hipStream_t s,
			 uint32_t bits = 0);
// the packed form (press_hip_recode_sizes / press_hip_recode_packed): phases as launch_ex_encode_packed, p.out_off == pk.slot
void launch_recode_fused_packed(const DecodeArgs &d, const BatchArgs &p, bool key2bit, bool slow5, ExFmt fmt, ExEnt ent,
				 const PackArgs &pk, int phases, hipStream_t s, uint32_t bits = 0);
void launch_recode_counts(const uint32_t *out_n, uint32_t *n, uint32_t nreads, hipStream_t s);
void launch_recode_refused(const uint32_t *out_n, const BatchArgs &p, uint8_t *keep, bool save, hipStream_t s);

// Optional timing of the dominant kernel of a batch call with HIP events recorded on the
// launch stream (bench.py's roofline figure): launchers call these around that kernel.
void ktime_begin(int which, hipStream_t s); // which: 0 = press, 1 = depress
void ktime_end(int which, hipStream_t s);
void ktime_mute(bool m); // a composite launcher times its own kernel instead of the inner one's

// launchers.  All asynchronous on `s`.
void launch_svb_encode_chunked(const BatchArgs &a, bool key2bit, bool zd, hipStream_t s, bool slow5 = false); // chunks + look-back
void launch_svb_decode_chunked(const DecodeArgs &a, bool key2bit, bool zd, hipStream_t s, bool slow5 = false);
// picoamperes (press_hip_depress_pa_batch): the svb decode with the float writer (a.sig unused), and for the other
// methods the converter of the samples their decoder left at a.sig (tiles: max_chunks entries, ntiles: one word)
void launch_svb_decode_pa(const DecodeArgs &a, float *pa, const float *cal, bool key2bit, bool zd, bool slow5, hipStream_t s);
void launch_pa_convert(const DecodeArgs &a, float *pa, const float *cal, uint2 *tiles, uint32_t *ntiles, hipStream_t s);
// ... in two halves: the tile table of a.nsamp, then the converter over it
void launch_pa_tiles(const DecodeArgs &a, uint2 *tiles, uint32_t *ntiles, hipStream_t s);
void launch_pa_apply(const DecodeArgs &a, float *pa, const float *cal, const uint2 *tiles, const uint32_t *ntiles, hipStream_t s);
// press_stats.hip: median and MAD of a.out_n[r] samples at a.sig + a.off[r] over launch_pa_tiles' table (eight launches);
// stats: 2 int32 per read, cal: k_pa_convert's two floats per read, either may be NULL; ev: NULL or 9 events (profiling)
uint64_t stat_rows_bytes(uint32_t nreads);
uint64_t stat_state_bytes(uint32_t nreads);
void launch_signal_stats(const DecodeArgs &a, const uint2 *tiles, const uint32_t *ntiles, void *state, uint32_t *rows,
			 int32_t *stats, float *cal, hipEvent_t *ev, hipStream_t s);
// ... of the samples [a', b') of each read alone: range is 2 words per read in device memory, clamped by the kernels
// (include/press_hip.h 2y); the same eight launches
void launch_signal_stats_ranged(const DecodeArgs &a, const uint32_t *range, const uint2 *tiles, const uint32_t *ntiles, void *state,
				uint32_t *rows, int32_t *stats, float *cal, hipStream_t s);
// press_quant.hip: nq (1 .. QMAX) quantiles of a.out_n[r] samples at a.sig + a.off[r] over launch_pa_tiles' table (four
// launches whatever nq is); q: nq int32 per read, may be NULL; cal (nq == 2, else ignored): NULL, or the two floats per
// read that `rule` makes of {q[0], q[1]} (press_hip_scale_cal)
constexpr uint32_t QMAX = 4;
struct ScaleRule { // the floats of press_hip_scale_rule
	float shift_mul, shift_min, scale_mul, scale_min;
};
uint64_t quant_rows_bytes(uint32_t nreads, uint32_t nq);
uint64_t quant_state_bytes(uint32_t nreads);
void launch_signal_quantiles(const DecodeArgs &a, const uint2 *tiles, const uint32_t *ntiles, void *state, uint32_t *rows,
			     const uint32_t *num, const uint32_t *den, uint32_t nq, int32_t *q, float *cal, const ScaleRule *rule,
			     hipStream_t s);
void launch_signal_quantiles_ranged(const DecodeArgs &a, const uint32_t *range, const uint2 *tiles, const uint32_t *ntiles, void *state,
				    uint32_t *rows, const uint32_t *num, const uint32_t *den, uint32_t nq, int32_t *q, float *cal,
				    const ScaleRule *rule, hipStream_t s);
// press_rows.hip: the planned rows below nrows_cap, [*, T] of dtype, from the samples at a.sig + a.off[r] (a.nsamp: the
// rooms the plan was made of, a.out_n: the decoded counts) and two floats per read
enum { PRESS_ROWS_F32 = 0, PRESS_ROWS_F16 = 1, PRESS_ROWS_BF16 = 2 }; // PRESS_HIP_F32 / F16 / BF16
void launch_chunk_rows(const DecodeArgs &a, const float *cal, const uint64_t *row_first, void *rows, uint64_t nrows_cap, int dtype,
		       uint32_t T, uint32_t overlap, uint64_t total_samples, hipStream_t s);
// ... of press_hip_depress_chunks_trimmed_batch: cut (2 words per read, launch_trim_plan's) and row_first in device memory;
// row_read / row_start: NULL, or nrows_cap words each
void launch_chunk_rows_ranged(const DecodeArgs &a, const uint32_t *cut, const float *cal, const uint64_t *row_first, void *rows,
			      uint64_t nrows_cap, int dtype, uint32_t T, uint32_t overlap, uint64_t total_samples, uint32_t *row_read,
			      uint32_t *row_start, hipStream_t s);
// press_trim.hip: cnt[r] = min(a.out_n[r], a.nsamp[r]), 0 for a refused read; and the cuts, then the row plan over their
// lengths (det: launch_adaptor's pairs or launch_segments_first's records, unused in mode RANGE; need, slot: nreads + 1
// words of 64 bits)
enum { PRESS_TRIM_RANGE = 0, PRESS_TRIM_ADAPTOR = 1, PRESS_TRIM_SEGMENT = 2 }; // PRESS_HIP_TRIM_*
void launch_trim_counts(const DecodeArgs &a, uint32_t *cnt, hipStream_t s);
void launch_trim_plan(const DecodeArgs &a, int mode, const uint32_t *range, const void *det, uint32_t min_keep, uint32_t T, uint32_t overlap,
		      uint32_t *cut, uint32_t *user, uint64_t *need, uint64_t *slot, uint64_t *row_first, hipStream_t s);
// press_verify.hip, over launch_pa_tiles' table of the same batch (a.nsamp: the rooms, a.out_n: the counts):
// crc[r] = zlib's CRC-32 of the a.out_n[r] samples at a.sig + a.off[r], 0 for a refused read; raw: one word per read
void launch_crc(const DecodeArgs &a, const uint2 *tiles, const uint32_t *ntiles, uint32_t *raw, uint32_t *crc, hipStream_t s);
// first_bad[r] of the samples at a.sig + a.off[r] against those at sig + a.off[r] (include/press_hip.h,
// press_hip_verify_batch); *nbad = the reads that are not verified
// bits > 0 (press_hip_verify_degraded_batch): against D_bits of those samples, taken in registers
void launch_verify_cmp(const DecodeArgs &a, const int16_t *sig, const uint2 *tiles, const uint32_t *ntiles, uint32_t *first_bad,
		       uint32_t *nbad, hipStream_t s, uint32_t bits = 0);
// press_degrade.hip, over the same table: out[a.off[r] + i] = D_bits(a.sig[a.off[r] + i]) for i < a.out_n[r], bits in
// 0 .. 8 (0: a copy); out == a.sig is fine
void launch_degrade(const DecodeArgs &a, int16_t *out, uint32_t bits, const uint2 *tiles, const uint32_t *ntiles, hipStream_t s);
// press_events.hip: the events of the n[r] samples at sig + off[r] as picoamperes of cal (include/press_hip.h,
// press_hip_signal_events), a wave per read, in two walks: the count and the layout, then the records of the reads that
// fit ev_cap.  state: events_state_bytes.  The kernels are timed as ring 1 of press_hip_kernel_times: count, scan, write
struct EvParams { // press_hip_event_params
	uint32_t w1, w2;
	float thr1, thr2, height;
};
uint64_t events_state_bytes(uint32_t nreads);
void launch_events_count(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal,
			 const EvParams &p, void *state, uint64_t ev_cap, uint64_t *ev_first, uint32_t *ev_count, hipStream_t s);
void launch_events_write(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal,
			 const EvParams &p, void *state, void *ev, uint64_t ev_cap, const uint64_t *ev_first, hipStream_t s);
uint32_t events_serial_reads(hipStream_t s); // synchronises s
// ... and the layout between the two walks of either record call, one wave: first[0] = 0, first[r + 1] = first[r] + the
// count of read r, count[r] = that count where first[r + 1] <= cap, else 0xFFFFFFFF.  state: nreads records of
// state_stride bytes, the count in the first 32-bit word of each
void launch_records_scan(const void *state, uint32_t state_stride, uint32_t nreads, uint64_t cap, uint64_t *first, uint32_t *count,
			 hipStream_t s);
// press_segments.hip: sigtk's jnn segments of the n[r] samples at sig + off[r] (include/press_hip.h,
// press_hip_signal_segments), a wave per read, in two walks as the events; cal NULL: the raw domain; thr NULL, or 2 * nreads.
// state: segments_state_bytes.  launch_adaptor: jnnv2, one launch, no state.  Timed as ring 1 of press_hip_kernel_times
struct SegParams { // press_hip_jnn_params
	float std_scale;
	int32_t corrector, seg_dist, window;
	float stall_len;
	int32_t error;
	float top, bot;
};
struct Seg2Params { // press_hip_jnn2_params
	float std_scale;
	int32_t seg_dist, window, hi_thresh, lo_thresh;
};
uint64_t segments_state_bytes(uint32_t nreads);
void launch_segments_count(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal,
			   const SegParams &p, void *state, uint64_t seg_cap, uint64_t *seg_first, uint32_t *seg_count, float *thr,
			   hipStream_t s);
void launch_segments_write(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal,
			   const SegParams &p, void *state, void *seg, uint64_t seg_cap, const uint64_t *seg_first, hipStream_t s);
void launch_adaptor(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const Seg2Params &p, int32_t *pair,
		    float *thr, hipStream_t s);
// ... and segs[0] alone, in one launch (the stall methods): first[r] = { start, end }, start = STALL_NOSEG: no segment
void launch_segments_first(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const SegParams &p, void *state,
			   void *first, hipStream_t s, const float *cal = nullptr);
// press_ranges.hip: mean, deviation and median (12 bytes) of range i of read i >> shift, a wave per range (include/press_hip.h,
// press_hip_signal_range_stats); range NULL (whole reads), or 2 * nranges words; cal NULL: the raw domain.  launch_prefix,
// behind launch_adaptor on the same stream (press_hip_signal_prefix): out 16 bytes per read, thr NULL or 2 * nreads, and
// range: 4 words per read, the adaptor's range and the poly-A's for launch_range_stats with shift 1.  Timed as ring 1
void launch_range_stats(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nranges, uint32_t shift, const float *cal,
			const uint32_t *range, void *out, hipStream_t s);
void launch_prefix(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const float *cal, const SegParams &polya,
		   int32_t rna, float shift, float half, const int32_t *pair, void *out, float *thr, uint32_t *range, hipStream_t s);
// press_stall.hip: the stall methods (include/press_hip.h, press_hip_stall_*).  A read becomes up to three PIECES - what
// is left of it without the stall, the stall, and for dstall_fz the whole read - which the rccm_vbbe21_zd kernels press
// and depress as the reads of a larger batch; piece k of read r is entry STALL_PIECES * r + k (depress: STALL_DPIECES)
constexpr int PRESS_STALL_SVBBE21 = 0, PRESS_STALL_1500 = 1, PRESS_STALL_FZ = 2; // PRESS_HIP_STALL_* (press_hip.h)
constexpr uint32_t STALL_NOSEG = 0xFFFFFFFFu;
constexpr uint32_t STALL_PIECES = 3, STALL_DPIECES = 2;
struct StallRead {            // per read: what the stream says (press: what the plan found)
	uint32_t start, len;  // the stall [start, start + len) of the read, 0 and 0 without one
	uint32_t exists;
	uint32_t ok;          // press: the pieces fit the scratch; depress: the header passed every check
};
struct StallBufs {            // the scratch of one call (Ctx::sl_*), np pieces
	uint2 *seg;           // [nreads] launch_segments_first
	StallRead *rd;        // [nreads]
	uint64_t *poff;       // [np + 1] piece p's samples start at psig[poff[p]] (multiples of 8)
	uint32_t *pn;         // [np] its samples, 0: no such piece
	uint64_t *pooff;      // [np + 1] press: its slot in parena; depress: its stream's offset in the caller's arena
	uint64_t *polen;      // [np] its stream's bytes
	uint32_t *poutn;      // [np] depress: the inner decoder's verdict
	int16_t *psig;
	uint8_t *parena;      // press
	uint64_t sig_cap, arena_cap; // samples of psig, bytes of parena
};
uint64_t stall_piece_samples(int stall_method, uint64_t total_samples, uint32_t nreads, bool decode);
uint64_t stall_arena_bytes(uint64_t piece_samples, uint32_t npieces);
// press: segs[0] -> plan and piece table -> pieces' samples (behind it: the inner press of the pieces) -> the streams
void launch_stall_plan(int stall_method, const uint32_t *n, uint32_t nreads, const StallBufs &b, hipStream_t s);
void launch_stall_gather(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const StallBufs &b, hipStream_t s);
void launch_stall_assemble(int stall_method, const uint32_t *n, uint32_t nreads, const StallBufs &b, uint8_t *out, const uint64_t *out_off,
			   uint64_t *out_len, uint32_t *stall, hipStream_t s);
// behind the inner press: need[r] = the exact length of read r's stream (PRESS_HIP_FAILED: refused), and the assemble into
// a laid-out arena: read r at slot[r], written where it ends at or in front of out_cap (PackArgs)
void launch_stall_sizes(int stall_method, const uint32_t *n, uint32_t nreads, const StallBufs &b, uint64_t *need, hipStream_t s);
void launch_stall_assemble_packed(int stall_method, const uint32_t *n, uint32_t nreads, const StallBufs &b, uint8_t *out, const uint64_t *slot,
				  uint64_t out_cap, uint64_t *out_len, hipStream_t s);
// depress: headers -> piece table (behind it: the inner depress of the pieces) -> the samples in place
void launch_stall_parse(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, const uint32_t *n, uint32_t nreads,
			const StallBufs &b, hipStream_t s);
void launch_stall_scatter(int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, const StallBufs &b, uint32_t *out_n,
			  hipStream_t s);
// ---- the exception-split pipeline (press_exsplit.hip, press_sections.hip) and its stages
// A stage's press: the read's one-byte values -> its stream behind the section.  need != NULL (the stages with
// sizes_only, press_hip_{rice, huffman}_press_sizes): the stage's sizing kernels alone, need[r] += the bytes of its
// stream; every other stage is given NULL.  Its depress: the stream -> a.low.
typedef void (*ExPressFn)(const BatchArgs &a, uint64_t *need, hipStream_t s);
typedef void (*ExDepressFn)(const DecodeArgs &a, hipStream_t s);
// The write half of a PAY_STAGED stage in the packed press, behind press(need != NULL) of the size half and k_ex_section
// against the laid-out slots: the slot check, then the stage's writing kernels.  Nothing is counted a second time.
typedef void (*ExWriteFn)(const BatchArgs &a, hipStream_t s);
void launch_low_encode(const BatchArgs &a, uint64_t *need, hipStream_t s);   // press_exsplit.hip: pass B, k_low_encode_chunked
void launch_shuff_encode(const BatchArgs &a, uint64_t *need, hipStream_t s); // ... k_huff_encode_chunked
void launch_huff_decode(const DecodeArgs &a, hipStream_t s);                 // press_huffman.hip (the subsequence size: a.huf_minlen)
void launch_rcs_encode(const BatchArgs &a, uint64_t *need, hipStream_t s);   // press_rc.hip
void launch_rcs_decode(const DecodeArgs &a, hipStream_t s);
void launch_rcc_encode(const BatchArgs &a, uint64_t *need, hipStream_t s);
void launch_rcc_decode(const DecodeArgs &a, hipStream_t s);
void launch_rcm_encode(const BatchArgs &a, uint64_t *need, hipStream_t s);
void launch_rcm_decode(const DecodeArgs &a, hipStream_t s);
void launch_cdf_encode(const BatchArgs &a, uint64_t *need, hipStream_t s);   // press_cdf.hip
void launch_cdf_decode(const DecodeArgs &a, hipStream_t s);
void launch_rice_encode(const BatchArgs &a, uint64_t *need, hipStream_t s);  // press_rice.hip; sizes: k_rice_count and k_rice_pick
void launch_rice_write_sized(const BatchArgs &a, hipStream_t s);            // ... k_rice_place, then write and copy
void launch_rice_decode(const DecodeArgs &a, hipStream_t s);
void launch_dhuf_encode(const BatchArgs &a, uint64_t *need, hipStream_t s);  // press_dhuf.hip; sizes: k_dh_hist and k_dh_tree
void launch_dhuf_write_sized(const BatchArgs &a, hipStream_t s);            // ... k_dh_place, then count, scan, write and copy
void launch_dhuf_decode(const DecodeArgs &a, hipStream_t s);
void ex_stage_sized(); // a stage's sizing kernels are launched once more (press_hip_debug_stage_sizing_launches)
struct ExStage {
	ExEnt id;
	ExPayload pay;
	ExPressFn press;
	ExDepressFn depress; // NULL: the merge reads the values where they lie
	bool low_tmp;        // press: k_low_encode_chunked leaves the one-byte values in a.low_tmp for the stage (else it IS the stage, or
	                     // the stage reads the samples); the scratch plan gives such a method Ctx::low
	bool sizes_only;     // press(need != NULL) exists
	ExWriteFn write_sized; // PAY_STAGED: the packed press's write half; NULL for the others
};
constexpr ExStage EX_STAGES[ENT_COUNT] = {
	{ ENT_PLAIN, PAY_INLINE, launch_low_encode, nullptr, false, false, nullptr },
	{ ENT_SHUFF, PAY_SHUFF, launch_shuff_encode, launch_huff_decode, false, false, nullptr },
	{ ENT_RC, PAY_CODER, launch_rcs_encode, launch_rcs_decode, true, false, nullptr },
	{ ENT_RCC, PAY_CODER, launch_rcc_encode, launch_rcc_decode, true, false, nullptr },
	{ ENT_RCM, PAY_CODER, launch_rcm_encode, launch_rcm_decode, true, false, nullptr },
	{ ENT_CDF, PAY_CODER, launch_cdf_encode, launch_cdf_decode, true, false, nullptr },
	{ ENT_RICE, PAY_STAGED, launch_rice_encode, launch_rice_decode, true, true, launch_rice_write_sized },
	{ ENT_DHUF, PAY_STAGED, launch_dhuf_encode, launch_dhuf_decode, true, true, launch_dhuf_write_sized },
};
constexpr bool ex_stages_in_order()
{
	for (int i = 0; i < ENT_COUNT; i++)
		if (EX_STAGES[i].id != i)
			return false;
	return true;
}
static_assert(ex_stages_in_order(), "EX_STAGES[i].id == i");

// the chain of a press: chunk table and ReadMeta; pass A; the exceptions counted and listed; the section and the stage
void ex_encode_prep(const BatchArgs &a, hipStream_t s);
void ex_encode_lists(const BatchArgs &a, ExFmt fmt, hipStream_t s);
void ex_encode_streams(const BatchArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s);
void launch_ex_encode_chunked(const BatchArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s);
void launch_ex_encode_packed(const BatchArgs &a, ExFmt fmt, ExEnt ent, const PackArgs &pk, int phases, hipStream_t s);
// the two halves of the packed press behind the exception lists: need[] (k_ex_sizes, and for a PAY_STAGED stage pass B into
// a.low_tmp and the stage's sizing kernels); the streams (such a stage: the section, then write_sized)
void ex_packed_sizes(const BatchArgs &a, ExFmt fmt, ExEnt ent, uint64_t *need, hipStream_t s);
void ex_packed_streams(const BatchArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s);
// press_hip_{rice, huffman}_press_sizes: the press chain of a stage with sizes_only as far as the sizes; a.out_off:
// nreads + 1 zeros, a.out_len == need
void launch_ex_prefix_sizes(const BatchArgs &a, ExFmt fmt, ExEnt ent, uint64_t *need, hipStream_t s);
void launch_ex_decode_chunked(const DecodeArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s);
void launch_ex_section(const BatchArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s);               // press_sections.hip
void launch_ex_sizes(const BatchArgs &a, ExFmt fmt, ExEnt ent, uint64_t *need, hipStream_t s);
void launch_ex_parse_huff(const DecodeArgs &a, ExFmt fmt, ExEnt ent, hipStream_t s);           // ... k_ex_parse, then the stage's depress
// behind the encode of a range-coder method (PAY_CODER): raw[r] = 1 where the coder gave up and stored the one-byte values
void launch_rcf_raw(const BatchArgs &a, uint8_t *raw, hipStream_t s);
// symbol counts of a batch for fitting a Huffman table (press_train.hip): adds into counts[257]; chunks takes
// train_scratch_bytes(max_chunks), nchunks is one device word (zeroed here)
uint64_t train_scratch_bytes(uint32_t max_chunks);
void launch_symbol_counts(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, uint64_t *counts,
			  void *chunks, uint32_t *nchunks, uint32_t max_chunks, uint32_t grid, hipStream_t s);

// dataset analysis (press_tally.hip): adds into raw[65536], delta[65536], trans[257 * 257] and sets mom[nreads]; any of the four may
// be NULL.  chunks takes tally_scratch_bytes(max_chunks), nchunks is one device word (zeroed here), cus is the device's
// number of compute units: the launch sizes its persistent grid from it
uint64_t tally_scratch_bytes(uint32_t max_chunks);
void launch_signal_tally(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, uint64_t *raw, uint64_t *delta,
			 uint64_t *trans, void *mom, void *chunks, uint32_t *nchunks, uint32_t max_chunks, uint32_t cus, hipStream_t s);

// sets press_hip_last_error() (press_ctx.hip) and returns code
int set_error(int code, const char *fmt, ...);

} // namespace ph
