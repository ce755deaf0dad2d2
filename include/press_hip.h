/*
 * press_hip.h - C ABI of libpress_hip.so: the MI355X (gfx950) implementation of the
 * per-read transform -> pack -> entropy hot path of sashajenner/honours `press/`.
 *
 * Three groups of entry points:
 *
 *  (1) DROP-IN SYMBOLS.  Exactly the X_bound / X_press / X_depress triples that
 *      press/press.h declares for the hot-path methods (file:line cited on each),
 *      plus the four huffman.h functions press/test.c calls for the static table.
 *      Same names, prototypes, argument meaning and return codes, so the
 *      reference's unmodified harness (press/test.c, TEST() in press/test.h:10-37)
 *      links against this library for these methods.  Host pointers in, host
 *      pointers out; each call is H2D copy -> kernels -> D2H copy on a private
 *      stream, synchronous like the reference.
 *
 *  (2) BATCH API (press_hip_*).  Not in the reference: one call per batch of reads
 *      with device-resident buffers - the throughput path (one read per call is
 *      launch/PCIe-latency bound).  Reads are independent (thesis/probspace/
 *      focus.tex:177-183), so a batch is the natural device unit.
 *
 *  (3) BLOW5 FILES (press_hip_blow5_*, slow5_svb_zd_*).  The data format on the input
 *      side of the path: slow5lib's "svb-zd" signal codec on the
 *      device and a host reader / writer for the record framing, so that signals
 *      travel to and from the GPU as stored.
 *
 * Plain C: pointers and sizes only, no C++ or torch types.
 * Deviation from the reference, on purpose: X_press never writes past the capacity
 * passed in *nout (the reference ignores it and relies on X_bound being large
 * enough, press/test.c:1788).  When the stream does not fit, int methods return -1
 * and void methods set *nout = 0.
 */
#ifndef PRESS_HIP_H
#define PRESS_HIP_H

#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ======================================================================= (1) drop-in symbols */

/* ---- static Huffman table objects: press/huffman/huffman.h:22-51 (layout kept) ---- */
#ifndef HUFFMAN_HUFFMAN_H
#define MAX_SYMBOLS 256
typedef struct huffman_node_tag {
	unsigned char isLeaf;
	unsigned long count;
	struct huffman_node_tag *parent;
	union {
		struct {
			struct huffman_node_tag *zero, *one;
		};
		unsigned char symbol;
	};
} huffman_node;
typedef struct huffman_code_tag {
	unsigned long numbits; /* code length in bits */
	unsigned char *bits;   /* bit k of the code at bit k%8 of bits[k/8]; bit 0 is emitted first */
} huffman_code;
typedef huffman_code *SymbolEncoder[MAX_SYMBOLS];
#endif

/* huffman.h:58 / huffman.c:549 - parse the table file (format: SURVEY.md 8(a) a10) */
bool read_code_table(FILE *in, huffman_node **rootOut, unsigned int *dataBytesOut);
/* huffman.h:65 / huffman.c:353 */
void build_symbol_encoder(huffman_node *subtree, SymbolEncoder *pSF);
/* huffman.h:66 / huffman.c:145 - frees the codes AND *pSE itself, as the reference does */
void free_encoder(SymbolEncoder *pSE);
/* huffman.h:67 / huffman.c:117 */
void free_huffman_tree(huffman_node *subtree);

/* ---- svb16 without zd: press.h:317-320 (press.c:1568-1581) ---- */
uint64_t svb12_bound(uint64_t nin);
void svb12_press(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void svb12_depress(const uint8_t *in, uint64_t nin /* samples */, int16_t *out);

/* ---- svb16-zd: press.h:348-352 (press.c:1678-1694).  nin of depress = samples ---- */
uint64_t svb12_zd_bound(uint64_t nin);
void svb12_zd_press(const int16_t *in, uint64_t nin, uint8_t *out, uint64_t *nout);
void svb12_zd_depress(const uint8_t *in, uint64_t nin, int16_t *out, uint64_t *nout);

/* ---- svb-zd (svb32): press.h:324-328 (press.c:1585-1611) ---- */
uint64_t svb_zd_bound_16(uint64_t nin);
void svb_zd_press_16(const int16_t *in, uint64_t nin, uint8_t *out, uint64_t *nout);
void svb_zd_depress_16(const uint8_t *in, uint64_t nin, int16_t *out, uint64_t *nout);

/* ---- VBZ = zstd-svb-zd: press.h:380-384 (press.c:1860-1910).  The inner stream is
 * produced on the GPU; the zstd stage is the third-party libzstd the reference itself
 * calls (press.c:1464), loaded at run time.  -1 when libzstd is not present. ---- */
uint64_t zstd_svb_zd_bound_16(uint32_t nin);
int zstd_svb_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int zstd_svb_zd_depress_16(const uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ---- zstd-svb16-zd: press.h:404-408 (press.c:2020-2070) ---- */
uint64_t zstd_svb12_zd_bound(uint32_t nin);
int zstd_svb12_zd_press(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int zstd_svb12_zd_depress(const uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ---- exception split: press.h:498-526 (press.c:3411-3580 over :2679-3405).
 * depress: nin = compressed bytes; *nout = decoded samples ---- */
uint64_t vbe21_zd_bound_16(uint32_t nin);
void vbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void vbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t vbbe21_zd_bound_16(uint32_t nin);
void vbbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void vbbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t vbsbe21_zd_bound_16(uint32_t nin);
void vbsbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void vbsbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t vbsse21_zd_bound_16(uint32_t nin);
void vbsse21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void vbsse21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ---- static Huffman over the one-byte stream: press.h:634-662 (press.c:4409-4846).
 * se / root are the caller's table objects (read_code_table / build_symbol_encoder);
 * their codes are flattened and uploaded to the device (cached by content).
 * press returns 0 ok, -1 capacity, 1 Huffman-layer failure (as huffman.c does). ---- */
uint64_t shuffman_vbe21_zd_bound_16(uint32_t nin);
int shuffman_vbe21_zd_press_16(SymbolEncoder *se, const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int shuffman_vbe21_zd_depress_16(huffman_node *root, uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t shuffman_vbbe21_zd_bound_16(uint32_t nin);
int shuffman_vbbe21_zd_press_16(SymbolEncoder *se, const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int shuffman_vbbe21_zd_depress_16(huffman_node *root, uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t shuffman_vbsbe21_zd_bound_16(uint32_t nin);
int shuffman_vbsbe21_zd_press_16(SymbolEncoder *se, const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int shuffman_vbsbe21_zd_depress_16(huffman_node *root, uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t shuffman_vbsse21_zd_bound_16(uint32_t nin);
int shuffman_vbsse21_zd_press_16(SymbolEncoder *se, const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int shuffman_vbsse21_zd_depress_16(huffman_node *root, uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ---- vbe21 + order-0 adaptive range coder (TurboRC rcsenc / rcsdec): press.h:712-716 (press.c:5422-5500).
 * SURVEY 8f-1.  depress: *nout in = the exact sample count (press.c:5464). ---- */
uint64_t rc_vbe21_zd_bound_16(uint32_t nin);
void rc_vbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rc_vbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
/* ---- vbe21 + order-1 adaptive range coder (TurboRC rccsenc / rccsdec, rc_.c:181): press.h (press.c:5510-5580).
 * Same calling shape as rc_vbe21_zd. ---- */
uint64_t rcc_vbe21_zd_bound_16(uint32_t nin);
void rcc_vbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rcc_vbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
/* ---- vbbe21 + order 1-0 context mixing with secondary estimation (TurboRC rcmsenc / rcmsdec, rccm_.c:79,
 * instantiated by rccm_s.c): press.c:6901-7000 (the thesis's "rc01s-vbbe21-zd").  Same calling
 * shape as rc_vbe21_zd: *nout of depress in = the exact sample count (press.c:6986). ---- */
uint64_t rccm_vbbe21_zd_bound_16(uint32_t nin);
void rccm_vbbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rccm_vbbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ---- ex-zd v0: press.h:960-964 (press.c:8461-8500 over ex_zd.c:403,495) ---- */
uint64_t hasgam_vbsse21_zdq_bound_16(uint32_t nin);
int hasgam_vbsse21_zdq_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int hasgam_vbsse21_zdq_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ---- zstd over ex-zd: press.h:976-980 (press.c:8549-8589) ---- */
uint64_t zstd_hasgam_vbsse21_zdq_bound_16(uint32_t nin);
int zstd_hasgam_vbsse21_zdq_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int zstd_hasgam_vbsse21_zdq_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ---- BLOW5's signal codec "svb-zd" (SURVEY 8f-2): slow5lib slow5_press.c:1054 ptr_compress_svb_zd /
 * :1110 ptr_depress_svb_zd, reached through slow5_ptr_compress_solo / slow5_ptr_depress_solo
 * (slow5_press.h:103-105) from slow5_rec_to_mem (slow5.c:3948) and the record parser.
 * Stream: u32 sample count, then streamvbyte (2-bit keys) of the 32-bit zig-zag deltas - the same
 * bytes as the pre-zstd buffer of zstd_svb_zd for signals whose jumps fit 16 bits.
 * press: *nout capacity in / bytes out; depress: *nout room in samples in / samples out. */
uint64_t slow5_svb_zd_bound(uint32_t nin);
int slow5_svb_zd_press(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int slow5_svb_zd_depress(const uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
/* slow5lib's own calling shape: malloc'd result (free() it), counts in bytes; NULL on failure */
void *press_hip_slow5_ptr_compress_svb_zd(const int16_t *ptr, size_t count, size_t *n);
void *press_hip_slow5_ptr_depress_svb_zd(const uint8_t *ptr, size_t count, size_t *n);

/* ======================================================================= (2) batch API */

/* method ids (== oracle/press_methods.h); names are the reference's code names */
enum press_hip_method {
	PRESS_HIP_SVB12            = 0,
	PRESS_HIP_SVB12_ZD         = 1,
	PRESS_HIP_SVB_ZD           = 2,
	PRESS_HIP_ZSTD_SVB_ZD      = 3,  /* "VBZ".  Per-read symbols: libzstd on the host, the reference's bytes.
	                                    Batch API: the zstd frames are made and read ON THE DEVICE (below) */
	PRESS_HIP_ZSTD_SVB12_ZD    = 4,  /* zstd(svb16-zd): as method 3 (per-read: libzstd on the host; batch: frames on the device) */
	PRESS_HIP_VBE21_ZD         = 5,
	PRESS_HIP_VBBE21_ZD        = 6,
	PRESS_HIP_VBSBE21_ZD       = 7,
	PRESS_HIP_VBSSE21_ZD       = 8,
	PRESS_HIP_SHUFF_VBE21_ZD   = 9,
	PRESS_HIP_SHUFF_VBBE21_ZD  = 10,
	PRESS_HIP_SHUFF_VBSBE21_ZD = 11,
	PRESS_HIP_SHUFF_VBSSE21_ZD = 12,
	PRESS_HIP_HASGAM_ZDQ       = 13,
	PRESS_HIP_ZSTD_HASGAM_ZDQ  = 14, /* zstd(ex-zd): as method 3 */
	PRESS_HIP_SLOW5_SVB_ZD     = 15, /* BLOW5's signal codec (section 3) */
	PRESS_HIP_RC_VBE21_ZD      = 16, /* vbe21 + order-0 range coder: one read per lane (serial format) */
	PRESS_HIP_RCC_VBE21_ZD     = 17, /* vbe21 + order-1 range coder: one read per workgroup, its 128 KiB of state in LDS */
	PRESS_HIP_RCCM_VBBE21_ZD   = 18, /* vbbe21 + order 1-0 context mixing + SSE: one read per workgroup, 137 KiB of state in LDS */
	PRESS_HIP_NMETHODS         = 19
};

#define PRESS_HIP_OK        0
#define PRESS_HIP_EARG     (-2)  /* bad argument (method, alignment, NULL) */
#define PRESS_HIP_EHIP     (-3)  /* a HIP runtime call failed */
#define PRESS_HIP_ENOTABLE (-4)  /* static-Huffman method without a table */
#define PRESS_HIP_FAILED   UINT64_MAX /* per-read length on failure (capacity, malformed stream) */
/*
 * Argument checks of the batch calls below (press, packed press, symbol counts, the depress family, the signal
 * statistics, recode).  Every one of them first checks what needs no device: the method ids, a NULL among the pointers
 * a non-empty batch reads or writes, align, dtype, T / overlap, the rule, the ranks, and for device_resident != 0 the
 * 16-byte alignment of its sample / float / row arena.  These are PRESS_HIP_EARG with or without a GPU, and before any
 * scratch is (re)allocated.  Then the device is initialised (PRESS_HIP_EHIP if that fails) and a Huffman method's table
 * looked for (PRESS_HIP_ENOTABLE).  nreads == 0 is PRESS_HIP_OK and touches nothing (the packed calls write
 * out_off[0] = 0).  The layout checks of the host-pointer form (offsets, total_samples, overlaps, out_off, row_first) read
 * the caller's tables and come behind that.
 */

/* last HIP / library error as text (thread local) */
const char *press_hip_last_error(void);

/* select the device for this process (default: current device).  One process per GPU: the
 * library keeps ONE context (device, stream, scratch).  Calls may come from any host thread -
 * every entry point re-selects the device for the calling thread and entry points are
 * serialised by a lock - but two threads cannot run batches concurrently. */
int press_hip_set_device(int device);
/* stream (hipStream_t, as void*) the batch calls enqueue on; NULL is HIP's default
 * (null) stream.  Until this is called the library uses a private non-blocking stream;
 * press_hip_reset_stream() returns to it.  Scratch and the Huffman table belong to the context, not to a
 * stream: a caller who switches streams while batches are in flight orders the two streams itself. */
int press_hip_set_stream(void *stream);
int press_hip_reset_stream(void);
void *press_hip_get_stream(void);
/* block until everything enqueued by batch calls has finished */
int press_hip_synchronize(void);

/* static Huffman table for the batch API: file in the format of press/NA12878_zd.huffman
 * (huffman.c:549; it may list fewer than 256 symbols).
 * A table change is ordered against the current stream: press_hip_load_table_file, press_hip_set_table and the
 * table a shuffman_* drop-in symbol brings along wait on the host for everything enqueued on the current stream
 * before the device table is overwritten, and the new table is in place when they return.  Batches enqueued
 * before the call use the old table, batches enqueued after it the new one.  Setting the table that is already
 * in force (same lengths and bits) is recognised on the host and neither waits nor copies. */
int press_hip_load_table_file(const char *path);
/* or 256 {length, code bits} pairs; bit k of bits[s] is the k-th emitted bit.
 * len[s] == 0: symbol s has no code - a read fails (press: PRESS_HIP_FAILED / return 1) only if that
 * value occurs in it (the reference dereferences a NULL code there, huffman.c:860).
 * Limit of the device tables: codes of at most 24 bits (huffman.c takes up to 255); longer -> EARG,
 * and the shuffman_* drop-in symbols return 1 for such a table. */
int press_hip_set_table(const uint32_t len[256], const uint64_t bits[256]);

/*
 * Fitting a table to the caller's reads (press/gen_huffman.c's job, from the samples).
 * press_hip_symbol_counts ADDS the batch's symbol counts to counts[257]: for each read and i in [1, n[r]),
 * the zig-zag of the 16-bit wrapped delta s[i] - s[i-1] (the values the shuffman_* methods code):
 * counts[0..255] the one-byte values, counts[256] the exceptions (values above 255).  Sample 0 of a read
 * is stored raw and not counted.  Layout and alignment as press_hip_press_batch, except that reads may
 * overlap or repeat (the counter only reads them: a read listed twice is counted twice); device_resident != 0:
 * device pointers (counts too), the call only enqueues; == 0: host pointers, synchronous.  The counts are
 * exact integers: the same on every run.
 */
int press_hip_symbol_counts(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			    uint64_t total_samples, uint64_t *counts, int device_resident);
/* The reference's Huffman construction (huffman.c:373 calculate_huffman_codes as gen_huffman runs it) over
 * counts[0..255]: bit-exact with it whenever its longest code has at most max_bits (8..24) bits; otherwise the
 * construction over max(1, c >> k) for the first k = 0, 1, 2, ... whose codes fit.  Every symbol gets a code.
 * Host code, no GPU needed. */
int press_hip_table_from_counts(const uint64_t counts[256], uint32_t max_bits, uint32_t len[256], uint64_t bits[256]);
/* write_code_table (huffman.c:440): the file format of press/NA12878_zd.huffman, which read_code_table and
 * press_hip_load_table_file read; data_bytes goes into the header's "bytes encoded" field (gen_huffman writes
 * the sum of the counts mod 2^32).  Host code, no GPU needed. */
int press_hip_write_table_file(const char *path, const uint32_t len[256], const uint64_t bits[256], uint32_t data_bytes);

/* X_bound of the reference for `method` (what press/test.c allocates).  For n = 0 the exception, Huffman,
 * ex-zd and range-coder methods give the reference's own n - 1 wrap-around (press.c:3411): 8 589 934 593
 * bytes.  It stays so for the drop-in symbols; it is not a size for an empty read's slot (see below). */
uint64_t press_hip_bound(int method, uint32_t n);

/*
 * Compress nreads reads.
 *   sig      int16 samples; read r = sig[off[r] .. off[r]+n[r]).  off (nreads entries)
 *            must be multiples of 8 samples and sig 16-byte aligned: every sample load
 *            is a coalesced 16-byte access.  Reads may lie anywhere in sig, in any order
 *            and with gaps of anything between them, but their sample ranges must not
 *            overlap: per-read scratch (the exception lists, the range coders' byte
 *            streams) is placed at the read's sample offset off[r].  The host path refuses
 *            overlapping reads (PRESS_HIP_EARG) before anything is launched; the
 *            device-resident path cannot read off[] and takes it as a precondition.
 *            Empty reads (n[r] = 0) overlap nothing.
 *   n        samples per read (nreads entries)
 *   total_samples  extent of sig in samples: max(off[r]+n[r]) rounded up as the caller
 *            likes; sizes the library's scratch (with device-resident offsets the
 *            library cannot read them without a synchronisation)
 *   out      output arena; read r may use out[out_off[r] .. out_off[r+1]) - its
 *            capacity; out_off has nreads+1 entries, non-decreasing, each any byte
 *            offset (no alignment; 64-bit: arenas past 4 GiB are fine).  Nothing outside
 *            the slots is written, and a failed read leaves its neighbours alone.
 *            The smallest slot a read takes:
 *              svb12, svb12_zd, svb_zd, slow5_svb_zd: the format's worst case, checked up
 *                front - h + k + w * n with keys k = ceil(n / 8) (svb12, svb12_zd) or
 *                ceil(n / 4) (svb_zd, slow5_svb_zd), h = 4 and w = 3 for slow5_svb_zd
 *                (the u32 count; a 32-bit delta may take 3 bytes), h = 0 and w = 2 else;
 *              the exception, Huffman, ex-zd and range-coder methods: the stream's own
 *                length (the reference's bytes; a range-coder stream stored raw included);
 *              the zstd kinds: the frame's own length.
 *            press_hip_bound(m, n) is the reference's X_bound: too small for
 *            exception-heavy reads (press.c:2575), and 8 GiB for n = 0 (above).
 *   out_len  per read: bytes produced, or PRESS_HIP_FAILED (capacity too small, ...)
 * An empty read (n[r] = 0) gives, as the reference does:
 *   svb12, svb12_zd, svb_zd: an empty stream (0 bytes);
 *   slow5_svb_zd: its u32 count alone, 00 00 00 00 (slow5_press.c:1046), PRESS_HIP_FAILED
 *     in a slot under 4 bytes;
 *   the zstd kinds over svb: a frame holding the u32 count 0;
 *   the exception, Huffman, ex-zd and range-coder methods, and zstd over ex-zd:
 *     PRESS_HIP_FAILED (the reference refuses n = 0).
 * device_resident != 0: every pointer is a device pointer, the call only enqueues
 * work on the current stream (no synchronisation; scratch is (re)allocated only when a
 * batch is larger than any before it); == 0: host pointers, synchronous.
 */
int press_hip_press_batch(int method, const int16_t *sig, const uint64_t *off, const uint32_t *n,
			  uint32_t nreads, uint64_t total_samples, uint8_t *out,
			  const uint64_t *out_off, uint64_t *out_len, int device_resident);

/*
 * Packed press: the library lays the output arena out itself.  The streams go back to back, no read fails for want of
 * a slot, and the arena is as large as the data - the caller needs no slot table and no bound.
 *
 * press_hip_press_sizes writes nothing but need[r]: the bytes read r takes under `method`.  For the 16 methods with
 * press_hip_packed_exact(method) == 1 that is the exact stream length, the out_len[r] press_hip_press_batch gives in a
 * slot that is large enough; summed, a dataset's compressed size.  PRESS_HIP_FAILED for a read the method refuses
 * whatever the slot: n = 0 for the exception, Huffman, ex-zd and range-coder methods, a value the table has no code
 * for, the uint16_t section length of the entropy-coded b/sb/ss forms, ex-zd's 2n + 1024 rule.  Empty reads of the
 * other methods keep the sizes given above (0; 4 for slow5_svb_zd; a frame for zstd over svb).
 * The three range coders (press_hip_packed_exact == 0): their stream's length is known only by coding it, and
 *     need[r] = hdr + seclen + nlow + S,  S = 32
 * is the smallest slot certain to hold it: hdr + seclen (header and exception section) is exact, nlow (the one-byte
 * values) is the size of the stream stored raw, which the coder falls back to once its output reaches
 * g = nlow * 255 / 256 - 8 bytes (rcutil_.h:161).  That test runs once per input byte, and a byte emits at most one
 * 32-bit word per renormalisation: 4 words (rc, rcc: before bits 7, 5, 3, 1) or 8 (rccm: before every bit).  So the
 * most a coder has written when it gives up is max(g - 1, 0) + 32 <= nlow + 23 bytes, or 32 bytes for the inputs
 * (nlow < 10) whose g is not positive; a coder that never gives up ends below g and flushes at most 12 bytes (one
 * renormalisation and two words).  Every case is at most nlow + 32.  S is derived, not measured.
 *
 * press_hip_press_packed compresses.  out_off (nreads + 1 entries) is WRITTEN:
 *     out_off[0] = 0
 *     out_off[r] = the end of read r-1's stream (its need), rounded up to `align`
 *     out_off[nreads] = the end of the last stream, not rounded
 * Read r's stream is out[out_off[r] .. out_off[r] + out_len[r]); a refused read takes 0 bytes.  The layout does not
 * depend on out_cap, so out_off[nreads] always says what the batch needs.  Read r is written iff
 * out_off[r] + need[r] <= out_cap; otherwise out_len[r] = PRESS_HIP_FAILED and no byte of it is written.  Device
 * resident, nothing at or beyond out_cap and no padding byte is ever written.  The streams are byte for byte those of
 * press_hip_press_batch.  The range coders' arena keeps gaps: out_len[r] <= need[r], and the bytes between a stream's
 * end and out_off[r] + need[r] are unspecified.
 *   align    a power of two, 1 .. 4096; anything else is PRESS_HIP_EARG (as a bad method id: before any device call)
 *   sig / off / n / total_samples / device_resident   as press_hip_press_batch, with its checks
 * device_resident != 0: every pointer is a device pointer, out_off and need included; the call only enqueues, there is
 * no synchronisation and no host wait.  == 0: host pointers, synchronous: the samples are staged and the layout is
 * made, out_off[nreads] is read back - the call's one synchronisation besides the last -, the device arena is reserved
 * at min(out_off[nreads], out_cap) bytes, not at a bound, and after the press that prefix of the arena goes to `out` in
 * ONE contiguous transfer (page-locked `out`, or up to 256 KiB: one DMA; pageable: through the staging buffers); on
 * this path padding, range-coder gaps and the room of a read that did not fit arrive as zeros.
 * press_hip_depress_batch wants 64 readable bytes behind the last stream: allocate out_cap + 64 for an arena that is
 * decoded later.
 * press_hip_packed_workspace_bytes: the device scratch the two calls keep for a batch of this shape, exact as
 * press_hip_workspace_bytes is and never below it; 0 for a method id out of range.
 */
int press_hip_press_sizes(int method, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			  uint64_t total_samples, uint64_t *need, int device_resident);
int press_hip_press_packed(int method, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			   uint64_t total_samples, uint8_t *out, uint64_t out_cap, uint32_t align,
			   uint64_t *out_off, uint64_t *out_len, int device_resident);
int press_hip_packed_exact(int method); /* 1: need == stream length (16 of the 19 methods, Rice and per-read Huffman of
                                         * (2w), the stall methods of (2x)); 0: range coders, bad ids */
uint64_t press_hip_packed_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads);

/*
 * Decompress nreads streams.
 *   in/in_off/in_len  stream r = in[in_off[r] .. in_off[r]+in_len[r]); in_off any byte
 *                     offset, streams in any order, and 64 readable bytes behind the
 *                     last stream (the decoders load whole words)
 *   sig/off/n         output layout as above; n[r] is the room for read r in samples
 *                     AND, for the svb methods, the sample count (their streams do
 *                     not carry it, press.c:1689).  For the formats that carry their
 *                     own count the room may be larger than the read.  The rooms
 *                     [off[r], off[r] + n[r]) must not overlap: the host path refuses
 *                     overlapping rooms (PRESS_HIP_EARG) before anything is launched,
 *                     whatever nreads; device resident, it is a precondition.
 *                     Samples are written to [off[r], off[r] + roundup8(n[r])) at most
 *                     (device resident) or [off[r], off[r] + out_n[r]) (host buffers;
 *                     page-locked ones: see the note on press_hip_host_alloc)
 *   out_n             per read: samples decoded, or UINT32_MAX on a malformed stream.  A refused
 *                     read writes nothing outside its own room and leaves the other reads
 *                     alone.  For the twelve methods with an exception section (the four
 *                     vb*e21_zd forms plain, shuffman_* and rc* / rccm*, and ex-zd) a stream
 *                     is well formed iff: header, nex and the lists or
 *                     the two length-prefixed blocks lie inside the stream, and each block
 *                     holds nex values (bit-packed: 1 + ceil(nex * bits / 8) <= its length,
 *                     bits <= 32; svb32 / svb16: the key bytes and the data bytes they
 *                     announce); the positions are strictly increasing 32-bit numbers and
 *                     every exception is placed, pos[nex - 1] - (nex - 1) <= nlow, nlow
 *                     being the one-byte values the stream holds (plain), announces and
 *                     delivers (Huffman) or n[r] - 1 - nex (range coders); and the read's
 *                     1 + nlow + nex samples fit n[r] - for ex-zd also the header's n, which
 *                     is 1 .. n[r] with version 0 and q <= 5.  Blocks longer than needed,
 *                     widths and svb byte lengths larger than minimal are well formed;
 *                     value + 256 is taken modulo 2^16.  A Huffman payload that ends early
 *                     gives the shorter read if its exceptions are still placed.
 * An empty read: slow5_svb_zd takes exactly the 4-byte count 0 and refuses any other stream
 * for n = 0 (the reference needs the count, slow5_press.c:1086, 1098).  svb12, svb12_zd
 * and svb_zd give 0 samples for n = 0 whatever the stream, as the reference does (their
 * streams carry no count).  The other methods decode what the stream holds, into a room
 * of n[r] samples.
 */
int press_hip_depress_batch(int method, const uint8_t *in, const uint64_t *in_off,
			    const uint64_t *in_len, uint32_t nreads, int16_t *sig,
			    const uint64_t *off, const uint32_t *n, uint64_t total_samples,
			    uint32_t *out_n, int device_resident);

/*
 * Decompress nreads streams straight to current in picoamperes: press_hip_depress_batch with float output.
 *
 * The conversion is the reference's signal_in_picoamps (sigtk misc.c:15-32, the TO_PICOAMPS macro; pyslow5's pA = True),
 * bit for bit.  Read r has two floats of calibration,
 *     cal[2r]     = (float) offset
 *     cal[2r + 1] = (float) range / (float) digitisation       (the casts first, the division in single precision)
 * which press_hip_pa_cal makes of the three doubles a BLOW5 record stores (host arithmetic, no GPU), and
 *     pa[off[r] + i] = ((float) s[i] + cal[2r]) * cal[2r + 1]
 * where s is what press_hip_depress_batch decodes.  The add and the multiply round separately, to nearest, in IEEE
 * single precision - never fused -, so the floats depend on the sample and the two floats alone and are the same for
 * every method.  cal is not validated: NaN and inf propagate.
 *   in/in_off/in_len/off/n/total_samples/out_n   as in press_hip_depress_batch, with its checks, its room rules, its
 *            empty-read rules, PRESS_HIP_ENOTABLE and the zstd kinds' host wait; out_n is what that call gives
 *   pa       takes the place of sig: off[] counts floats.  Device resident it must be 16-byte aligned (PRESS_HIP_EARG),
 *            and a decoded read is written as [off[r], off[r] + out_n[r]) and nothing else, whatever the method: no
 *            float is ever made of a sample the call has not decoded.  Nothing outside the rooms is written.  Host
 *            buffers receive exactly out_n[r] floats per read.  A refused read
 *            (out_n[r] = UINT32_MAX) leaves its neighbours' rooms alone; what its own room holds is unspecified, as
 *            with press_hip_depress_batch.
 *   cal      2 * nreads floats; a device pointer when device resident
 * A bad method id or a NULL argument is PRESS_HIP_EARG before any device call; nreads == 0 is PRESS_HIP_OK.
 * device_resident != 0: the call only enqueues.  == 0: host pointers, synchronous; streams, layout and cal are staged,
 * the floats are decoded into a device arena and the decoded ranges come back as press_hip_depress_batch's samples do.
 * press_hip_depress_pa_fused(method) == 1 (the four svb methods): the decode kernel converts the samples it holds in
 * registers and writes the floats itself - no int16 copy of the samples exists anywhere.  == 0: the method's decoder
 * runs unchanged into library scratch and a second kernel converts [0, out_n[r]) of every decoded read.
 * press_hip_depress_pa_workspace_bytes: the device scratch the device-resident call keeps for a batch of this shape,
 * exact as press_hip_workspace_bytes is and never below it: for a fused method the same, for the others plus the
 * samples (total_samples * 2 + 64 bytes) and the converter's tile table.  0 for a method id out of range.
 */
int press_hip_pa_cal(const double *dor, uint32_t nreads, float *cal); /* dor: nreads x {digitisation, offset, range} */
int press_hip_depress_pa_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
			       uint32_t nreads, float *pa, const uint64_t *off, const uint32_t *n,
			       uint64_t total_samples, const float *cal, uint32_t *out_n, int device_resident);
int press_hip_depress_pa_fused(int method); /* 1: the decode kernel writes the floats itself; 0: via int16 scratch, bad ids */
uint64_t press_hip_depress_pa_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads);

/*
 * Robust normalisation on the device: per-read median and median absolute deviation, and decoding straight to
 * (x - median) / (1.4826 * MAD).
 *
 * Both statistics are the reference's (sigtk stat.h:56-73, mediani16 / medianf: ks_ksmall(n, copy, n / 2) - the k-th
 * smallest value, never an average; events.c:171-194, madf).  For a read of c samples s[0 .. c), k = c / 2:
 *     med  = the k-th smallest (0-based) of s                        an int16 value, as int32
 *     d[i] = |(int32) s[i] - med|   in 0 .. 65535
 *     mad  = the k-th smallest of d                                  an integer, as int32, NOT yet scaled by 1.4826
 *     c0   = (float) (-(int32) med)
 *     c1   = 1.0f / ((float) mad * 1.4826f) for mad > 0, 1.0f for mad == 0     (the product rounded to single
 *            precision, then a correctly rounded division)
 *     norm[i] = ((float) s[i] + c0) * c1                             the add and the multiply rounded separately
 * All of it is exact and the same from run to run: order statistics of 16-bit integers, found by a radix select whose
 * only sums are integer counts, and press_hip_depress_pa_batch's arithmetic with a calibration the device derives.  The
 * calibration of the read cancels in norm[], so none is asked for.  c == 0 and a refused read: med = mad = 0,
 * {c0, c1} = {0.0f, 1.0f}.
 *
 * press_hip_signal_stats: stats[2r] = med, stats[2r + 1] = mad of the n[r] samples at sig + off[r].
 *   sig / off / n / total_samples / device_resident   as press_hip_press_batch: layout, alignment (off[] multiples of 8
 *            samples, a device sig 16-byte aligned: PRESS_HIP_EARG), non-overlap (host pointers: checked)
 *   stats    2 * nreads int32; a device pointer when device resident
 *   device_resident != 0: the call only enqueues.  == 0: samples and layout are staged, the call is synchronous.
 * press_hip_norm_cal: host arithmetic, no GPU: cal[2r], cal[2r + 1] = c0, c1 of stats[2r], stats[2r + 1] -
 *   what press_hip_depress_pa_batch takes as cal to reproduce norm[] from the same samples.
 * press_hip_depress_norm_batch: press_hip_depress_pa_batch without cal.  Every read is decoded, med / mad are taken over
 *   its out_n[r] decoded samples, and norm[] is written into `out`.
 *   in/in_off/in_len/off/n/total_samples/out_n   as in press_hip_depress_batch, with its checks, its room rules, its
 *            empty-read rules, PRESS_HIP_ENOTABLE and the zstd kinds' host wait
 *   out      off[] counts floats.  Device resident it must be 16-byte aligned (PRESS_HIP_EARG); a decoded read is
 *            written as [off[r], off[r] + out_n[r]) and nothing else, nothing outside the rooms is written and a
 *            refused read (out_n[r] = UINT32_MAX) gets no float at all.
 *            Host buffers receive exactly out_n[r] floats per read.
 *   stats    2 * nreads int32 as above ({0, 0} for an empty or refused read), or NULL
 * A bad method id or a NULL argument (stats of this call excepted) is PRESS_HIP_EARG before any device call;
 * nreads == 0 is PRESS_HIP_OK.
 * There is no fused variant: the median needs the whole read before the first float can be written, so all 19 methods
 * decode unchanged into library scratch (as press_hip_depress_pa_fused(method) == 0 does), eight small launches select
 * med and mad from it, and press_hip_depress_pa_batch's converter writes the floats.
 * press_hip_depress_norm_workspace_bytes: the device scratch the device-resident call keeps for a batch of this shape,
 * exact as press_hip_depress_pa_workspace_bytes is and never below it for a method that is not fused: plus a row of
 * counters (1 KiB), 16 bytes of state and two floats per read.  0 for a method id out of range.
 * press_hip_signal_stats_timed: a profiling aid - the device-resident press_hip_signal_stats, synchronous, with a HIP
 * event behind each of its eight kernels: ms[0 .. 8) = count, pick, count, pick of the median, then of the MAD.
 */
int press_hip_signal_stats(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			   uint64_t total_samples, int32_t *stats, int device_resident);
int press_hip_norm_cal(const int32_t *stats, uint32_t nreads, float *cal);
int press_hip_depress_norm_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
				 uint32_t nreads, float *out, const uint64_t *off, const uint32_t *n,
				 uint64_t total_samples, int32_t *stats, uint32_t *out_n, int device_resident);
uint64_t press_hip_depress_norm_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads);
int press_hip_signal_stats_timed(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				 uint64_t total_samples, int32_t *stats, float *ms);

/*
 * Quantile scaling and chunk rows: compressed reads straight to the [rows, T] half-precision tensor a basecaller takes.
 *
 * press_hip_signal_quantiles: up to 4 order statistics per read.
 *     q[nq * r + i] = the k-th smallest (0-based) of the n[r] samples at sig + off[r],
 *                     k = min(c - 1, floor(c * rank_num[i] / rank_den[i])), c = n[r]; 0 for c == 0
 *   sig / off / n / total_samples / device_resident   as press_hip_signal_stats, with its checks
 *   rank_num, rank_den   HOST arrays of nq entries in both modes (parameters, not data).  nq is 1 .. 4, den > 0 and
 *            num <= den, else PRESS_HIP_EARG before any device call.  Ranks may repeat and need not be ordered; 1 / 2 is
 *            press_hip_signal_stats' median, 1 / 1 the maximum.
 *   q        nq * nreads int32; a device pointer when device resident.  Nothing beyond it is written.
 *   Four launches whatever nq is (the radix select of the median, its high digit counted once for all ranks); every sum
 *   is one of integers, so the result is the same on every run.
 *
 * press_hip_scale_cal: host arithmetic, no GPU.  A rule names two ranks and four floats; q holds {q_lo, q_hi} per read:
 *     shift = fmaxf(shift_min, shift_mul * (float) (q_lo + q_hi))      (the integer sum is exact in float)
 *     scale = fmaxf(scale_min, scale_mul * (float) (q_hi - q_lo))
 *     cal[2r] = -shift        cal[2r + 1] = 1.0f / scale               (correctly rounded)
 *     y[i] = ((float) s[i] + cal[2r]) * cal[2r + 1]
 *   Every operation is rounded once, to nearest, in IEEE single precision, and never fused: y is what
 *   press_hip_depress_pa_batch writes with this cal.  A rule is valid when both ranks have den > 0 and num <= den, all four
 *   floats are finite and scale_min > 0; anything else, or a NULL rule, is PRESS_HIP_EARG.  The library has no default
 *   rule.
 *
 * press_hip_chunk_plan: host arithmetic, no GPU: the rows of a batch.  T is a positive multiple of 8 and overlap < T, else
 *   PRESS_HIP_EARG.  With S = T - overlap a read of c = n[r] samples takes 0 rows for c == 0, 1 row starting at sample 0
 *   for c <= T, otherwise 1 + ceil((c - T) / S) rows: row j starts at j * S, except the last, which starts at c - T (so no
 *   row of such a read runs past its end, and the last two may overlap by more than `overlap`).
 *   row_first   nreads + 1 entries: the exclusive sum of the row counts; row_first[nreads] is the number of rows
 *   row_read, row_start   per row the read and the start, for stitching a model's output; either may be NULL (call once
 *            with both NULL to size them by row_first[nreads])
 *
 * press_hip_depress_chunks_batch: decode, calibrate, write rows.
 *   in/in_off/in_len/off/n/total_samples/out_n   as in press_hip_depress_norm_batch: all 19 methods, the same checks, room
 *            and empty-read rules, PRESS_HIP_ENOTABLE and the zstd kinds' host wait.  off[] lays out the library's own
 *            sample scratch; the caller never sees samples.
 *   rule     a HOST pointer in both modes, read before the call returns.  Given (and valid, else PRESS_HIP_EARG):
 *            {q_lo, q_hi} are taken over the out_n[r] decoded samples (four launches) and y is press_hip_scale_cal's.
 *            NULL: the calibration is press_hip_depress_norm_batch's, median and MAD.
 *   q        2 * nreads int32 that receive {q_lo, q_hi}, or {med, mad} without a rule; {0, 0} for an empty or refused
 *            read; may be NULL.  A device pointer when device resident.
 *   dtype    PRESS_HIP_F32, PRESS_HIP_F16 or PRESS_HIP_BF16; T, overlap as in press_hip_chunk_plan.  A bad value is
 *            PRESS_HIP_EARG before any device call.
 *   row_first   press_hip_chunk_plan's over the same n[] (the ROOMS, so the layout is known on the host without a
 *            synchronisation); a device pointer when device resident, where it is a precondition; host pointers: checked
 *            (PRESS_HIP_EARG)
 *   rows     row-major [*, T] of dtype; device resident it must be 16-byte aligned (PRESS_HIP_EARG).  Row
 *            row_first[r] + j holds at column t round_to_dtype(y[start_j + t]); a column whose sample index is at or
 *            beyond out_n[r] is +0, and so is every column of every row of a refused read.  round_to_dtype is one
 *            further rounding of the float32 y to nearest even: overflow goes to infinity, float16 subnormals are
 *            kept; bfloat16 is returned as its 16-bit pattern, a NaN (0 * inf: only with a scale_min so small that
 *            1 / scale overflows) stays a quiet NaN.
 *   nrows_cap   rows the arena has room for.  Never written: rows at or beyond nrows_cap, rows at or beyond
 *            row_first[nreads], any byte outside rows[0 .. min(nrows_cap, row_first[nreads]) * T).  The layout does not
 *            depend on the cap.
 * nreads == 0 is PRESS_HIP_OK.  device_resident != 0: the call only enqueues.  == 0: host pointers, synchronous; it
 * stages as press_hip_depress_norm_batch does and the written prefix of rows comes back in one transfer, with q and out_n.
 * press_hip_depress_chunks_workspace_bytes: the device scratch the device-resident call keeps for a batch of this shape,
 * exact as press_hip_depress_norm_workspace_bytes is and never below it: the count rows are two per read.  0 for a method
 * id out of range or a bad T / overlap.
 */
typedef struct press_hip_scale_rule {
	uint32_t lo_num, lo_den, hi_num, hi_den; /* ranks of q_lo and q_hi */
	float shift_mul, shift_min, scale_mul, scale_min;
} press_hip_scale_rule;
enum { PRESS_HIP_F32 = 0, PRESS_HIP_F16 = 1, PRESS_HIP_BF16 = 2 };
int press_hip_signal_quantiles(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			       uint64_t total_samples, const uint32_t *rank_num, const uint32_t *rank_den, uint32_t nq,
			       int32_t *q, int device_resident);
int press_hip_scale_cal(const int32_t *q /* 2 * nreads: q_lo, q_hi */, uint32_t nreads, const press_hip_scale_rule *rule,
			float *cal /* 2 * nreads */);
int press_hip_chunk_plan(const uint32_t *n, uint32_t nreads, uint32_t T, uint32_t overlap, uint64_t *row_first /* nreads + 1 */,
			 uint32_t *row_read, uint32_t *row_start /* may be NULL */);
int press_hip_depress_chunks_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
				   uint32_t nreads, void *rows, uint64_t nrows_cap, int dtype, uint32_t T, uint32_t overlap,
				   const uint64_t *row_first, const uint64_t *off, const uint32_t *n, uint64_t total_samples,
				   const press_hip_scale_rule *rule, int32_t *q, uint32_t *out_n, int device_resident);
uint64_t press_hip_depress_chunks_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads, uint32_t T,
						  uint32_t overlap);

/*
 * Recode nreads streams of src_method into streams of dst_method: what press_hip_depress_batch(src_method) followed by
 * press_hip_press_batch(dst_method) give on the same buffers - out, out_len, out_n and sig byte for byte - in one call,
 * for every pair of methods.
 *   in/in_off/in_len/n/off/total_samples/out_n   as in press_hip_depress_batch
 *   out/out_off/out_len                          as in press_hip_press_batch; the sample counts of that half are out_n
 *   sig      the decoded samples as press_hip_depress_batch leaves them (decode for the basecaller, archive in the better
 *            format), or NULL: they then live in library scratch, total_samples int16 at the caller's off[]
 * A read whose source stream is refused gets out_n[r] = UINT32_MAX and out_len[r] = PRESS_HIP_FAILED; its slot and its
 * neighbours stay untouched.  Whatever the two calls refuse is refused here (the method checks, PRESS_HIP_ENOTABLE, the
 * alignment rules, overlapping rooms on the host path).  device_resident != 0: the call only enqueues (the zstd sources
 * keep the host wait described below); == 0: host pointers through the page-locked staging, synchronous.
 * press_hip_recode_fused(src, dst) == 1 (svb12_zd, svb_zd, slow5_svb_zd into any exception-split, static-Huffman, ex-zd
 * or range-coder method): the press half's first pass over the samples - its exception and code-bit counts - is left
 * behind by the svb decode kernel, which holds those very values in registers; the other pairs run the two halves as
 * they are.  Host arithmetic, no GPU needed.
 * press_hip_recode_workspace_bytes: the device scratch the call keeps for a batch of this shape, exact as
 * press_hip_workspace_bytes is: every buffer at the larger of what the batch calls of either method ask of it, the press
 * half's counts, the press half's own chunk table for a fused pair, and - keep_samples == 0, i.e. sig == NULL - the
 * samples.  0 for a method id out of range.
 */
int press_hip_recode_batch(int src_method, int dst_method, const uint8_t *in, const uint64_t *in_off,
			   const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
			   uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
			   int16_t *sig, uint32_t *out_n, int device_resident);
uint64_t press_hip_recode_workspace_bytes(int src_method, int dst_method, uint64_t total_samples, uint32_t nreads,
					  int keep_samples);
int press_hip_recode_fused(int src_method, int dst_method);

/*
 * Packed recode: press_hip_recode_batch into an arena the library lays out.  A recoding caller holds compressed bytes and
 * rooms n[r], not the sample counts the destination will be asked to code: it cannot make a slot table, and it needs none.
 *
 * press_hip_recode_packed gives what press_hip_depress_batch(src_method) followed by press_hip_press_packed(dst_method)
 * over the decoded samples with the sample counts out_n give - out_off, out_len, out_n, sig and the arena byte for byte -
 * for every pair of methods; the streams are those of press_hip_recode_batch in slots that are large enough.
 *   in/in_off/in_len/n/off/total_samples/sig/out_n   as in press_hip_recode_batch (sig == NULL: library scratch)
 *   out/out_cap/align/out_off/out_len                as in press_hip_press_packed: out_off is WRITTEN, the layout does not
 *            depend on out_cap, out_off[nreads] is what the batch needs, read r is written iff
 *            out_off[r] + need[r] <= out_cap, nothing at or beyond out_cap and - device resident - no padding byte is written;
 *            the range coders keep need = hdr + seclen + nlow + 32 and their gaps (press_hip_packed_exact(dst_method))
 * What that sequence cannot express - a read whose SOURCE stream is refused: out_n[r] = UINT32_MAX,
 * need[r] = out_len[r] = PRESS_HIP_FAILED, 0 bytes of the layout, and no byte written for it wherever out_cap lies and
 * whether or not the read behind it fits - also under the destinations that have a stream for an empty read
 * (slow5_svb_zd's u32 count, the zstd frames over svb).  A source read that decodes to 0 samples is not refused: it gets
 * the destination's empty-read result (press_hip_press_sizes).  A read the source decodes and the destination refuses
 * keeps its decoded out_n, with need = out_len = PRESS_HIP_FAILED and 0 bytes.
 * press_hip_recode_sizes writes only need[] (as press_hip_press_sizes, with the rule above), out_n[] and - sig given -
 * the samples: "what would this archive weigh under dst_method", with no arena.
 * A bad method id or align is PRESS_HIP_EARG before any device call; whatever the two halves refuse is refused here
 * (PRESS_HIP_ENOTABLE, the alignment of sig, overlapping rooms on the host path).  nreads == 0: PRESS_HIP_OK, and
 * press_hip_recode_packed writes out_off[0] = 0.
 * device_resident != 0: every pointer is a device pointer, out_off and need included; the call only enqueues (the zstd
 * sources keep their host wait, see below, and add no other).  == 0: host pointers, synchronous: streams and layout are
 * staged, the batch is decoded and sized, out_off[nreads] is read back - the one synchronisation besides the last -, the
 * device arena is reserved at min(out_off[nreads], out_cap) + 64 bytes, written, and that prefix goes to `out` in one
 * transfer; padding, range-coder gaps and the room of a read that did not fit arrive as zeros.  out_n and the samples
 * come back as from press_hip_recode_batch.
 * press_hip_recode_packed_workspace_bytes: press_hip_recode_workspace_bytes plus the two per-read tables of the packed
 * plan, (nreads + 1) * 8 bytes each; exact in the same sense, never below it, 0 for a method id out of range.  Host
 * arithmetic, no GPU needed.
 */
int press_hip_recode_sizes(int src_method, int dst_method, const uint8_t *in, const uint64_t *in_off,
			   const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
			   uint64_t total_samples, uint64_t *need, int16_t *sig, uint32_t *out_n, int device_resident);
int press_hip_recode_packed(int src_method, int dst_method, const uint8_t *in, const uint64_t *in_off,
			    const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
			    uint64_t total_samples, uint8_t *out, uint64_t out_cap, uint32_t align,
			    uint64_t *out_off, uint64_t *out_len, int16_t *sig, uint32_t *out_n, int device_resident);
uint64_t press_hip_recode_packed_workspace_bytes(int src_method, int dst_method, uint64_t total_samples,
						 uint32_t nreads, int keep_samples);

/*
 * Verifying on the device: "does what I wrote decode to what I had?" - by comparison while the samples are still there,
 * and by a per-read digest that can be kept and checked on another machine or years later.
 *
 * The digest: crc[r] is zlib's CRC-32 of read r's samples as they lie in memory - 2 * count bytes, little-endian int16;
 * polynomial 0xEDB88320 (reflected), initial value and final xor 0xFFFFFFFF; 0 for an empty read.  It is what
 * zlib.crc32(samples.tobytes()) gives, exactly: the value is an integer and does not depend on the run.
 *
 * press_hip_crc32_combine: host arithmetic, no GPU: crc32(A || B) from crc32(A), crc32(B) and |B| in bytes (any 64-bit
 * length: the exponent is reduced, never truncated), so that digests of pieces make the digest of the whole.
 *
 * press_hip_signal_crc32: crc[r] of the n[r] samples at sig + off[r].
 *   sig / off / n / total_samples / device_resident   as press_hip_press_batch, with its checks: off[] multiples of 8
 *            samples, a device sig 16-byte aligned (PRESS_HIP_EARG), non-overlap (host pointers: checked).  Loads stay
 *            inside [off[r], off[r] + roundup8(n[r])); what lies beyond n[r] does not take part.
 *   crc      nreads words; a device pointer when device resident.  Nothing beyond it is written.
 *
 * press_hip_depress_crc_batch: decode any of the 19 methods into library scratch and digest what was decoded; nothing of
 * the samples reaches the caller.
 *   in/in_off/in_len/off/n/total_samples/out_n   exactly as in press_hip_depress_batch: its checks, room rules, empty-read
 *            rules, PRESS_HIP_ENOTABLE and the zstd kinds' host wait.  off[] and n[] place the reads in the library's
 *            scratch; the rooms must not overlap.
 *   crc      crc[r] is the digest of the out_n[r] decoded samples, and 0 for a refused read (out_n[r] == UINT32_MAX)
 *
 * press_hip_verify_batch: decode into library scratch and compare with the caller's samples.
 *   in/in_off/in_len/out_n   as in press_hip_depress_batch
 *   sig / off / n   the samples the streams are meant to hold, laid out as press_hip_press_batch takes them: 16-byte
 *            aligned, off[] in multiples of 8.  n[r] is the expected count AND the decoder's room.  sig is never written;
 *            loads from it stay inside [off[r], off[r] + roundup8(n[r])), as the press kernels' do, and nothing beyond n[r]
 *            takes part in the comparison.
 *   first_bad   per read, with c = out_n[r]:
 *              0 if the stream is refused (c == UINT32_MAX); a count-carrying stream that holds more samples than n[r]
 *                is refused by the decoder, as in press_hip_depress_batch, and so gives 0;
 *              otherwise the smallest i < min(c, n[r]) with decoded[i] != sig[off[r] + i];
 *              without such an i and with c != n[r]: min(c, n[r]);
 *              otherwise PRESS_HIP_VERIFIED.
 *   nbad     *nbad = the number of reads with first_bad[r] != PRESS_HIP_VERIFIED: written, not accumulated.  Device
 *            resident it is a device word.
 * Such reads exist among the library's own output: the three range coders store tiny or incompressible reads raw
 * (rcutil_.h:161) and nothing tells their decoder - a valid output of press_hip_press_batch that does not round-trip.
 *
 * A bad method id or a NULL argument is PRESS_HIP_EARG before any device call; nreads == 0 is PRESS_HIP_OK (host
 * pointers: with *nbad = 0).  device_resident != 0: the three calls only enqueue on the current stream - no
 * synchronisation and no host wait beyond the zstd decode's.  == 0: host pointers, synchronous: the streams are staged as
 * press_hip_depress_batch stages them, the caller's samples as press_hip_press_batch stages them, the decode goes to the
 * library's sample scratch, and the small per-read tables and nbad come back.
 * press_hip_verify_workspace_bytes: the device scratch the device-resident press_hip_verify_batch and
 * press_hip_depress_crc_batch keep for a batch of this shape, exact as press_hip_workspace_bytes is and never below it:
 * plus the samples (total_samples * 2 + 64 bytes), the tile table and 4 bytes per read.  0 for a method id out of range.
 */
#define PRESS_HIP_VERIFIED 0xFFFFFFFFu
uint32_t press_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
int press_hip_signal_crc32(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			   uint64_t total_samples, uint32_t *crc, int device_resident);
int press_hip_depress_crc_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
				uint32_t nreads, const uint64_t *off, const uint32_t *n, uint64_t total_samples,
				uint32_t *crc, uint32_t *out_n, int device_resident);
int press_hip_verify_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
			   uint32_t nreads, const int16_t *sig, const uint64_t *off, const uint32_t *n,
			   uint64_t total_samples, uint32_t *first_bad, uint32_t *out_n, uint32_t *nbad,
			   int device_resident);
uint64_t press_hip_verify_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads);

/*
 * Events: reads segmented on the device, bit for bit as sigtk's `event` subcommand segments them.
 *
 * The events of a read are detect_events (sigtk/src/events.c:506, scrappie's detector) applied to the read's picoampere
 * floats, which are exactly press_hip_depress_pa_batch's:
 *     x[i] = ((float) s[i] + cal[2r]) * cal[2r + 1]                  the add and the multiply rounded separately
 * getevents (events.c:553) trims the read first and throws the result away, so the detection runs on the whole read; that
 * step is not repeated here.  The definition, every operation rounded on its own in the precision named:
 *   sums     S[0] = Q[0] = 0, S[i+1] = S[i] + (double) x[i], Q[i+1] = Q[i] + (double) (x[i] * x[i]) - the square rounded
 *            to single precision first; sequential double-precision adds (events.c:293)
 *   t-statistic of window w (events.c:315): 0 for i < w, for i > n - w, and everywhere when n < 2w; else with wf = (float) w
 *            sum1 = S[i] - S[i-w], sumsq1 = Q[i] - Q[i-w] (double);  sum2 = (float) (S[i+w] - S[i]), sumsq2 likewise
 *            mean1 = (float) (sum1 / (double) wf);  mean2 = sum2 / wf (single)
 *            var = fmaxf((float) (((sumsq1 / (double) wf - (double) (mean1 * mean1)) + (double) (sumsq2 / wf))
 *                                 - (double) (mean2 * mean2)), FLT_MIN)       products and sumsq2 / wf in single precision
 *            t[i] = (float) (fabs((double) (mean2 - mean1)) / sqrt((double) (var / wf)))
 *   peaks    short_long_peak_detector (events.c:371): two coupled state machines over t of w1 and of w2, stepped in that
 *            order at every sample; the short one masks and resets the long one; differences are taken in single precision
 *            before they are compared with peak_height
 *   events   boundaries 0, peak[0], peak[1], ..., n (events.c:457, 475); per event, with len = (float) (end - start):
 *            mean = (float) (S[end] - S[start]) / len
 *            stdv = sqrtf(fmaxf((float) (Q[end] - Q[start]) / len - mean * mean, 0))
 * The sums are exact, not close: a read whose sums cannot round in any order (every x a multiple of 2^q and
 * n * max|x| < 2^(q + 53), likewise the squares - decided per read on the device) is summed by a wave scan, every other
 * read by adds in the reference's order.  press_hip_events_serial_reads counts the latter.
 *
 * Where the reference does not answer, the library defines:
 *   - the reference aborts (assert, events.c:242, in the discarded trimming) on every read shorter than 100 samples and
 *     on every constant read; such reads get the events the definition above yields
 *   - a read with no peak: the reference reads peaks[-1]; here it is one event [0, n) with the formulas above
 *   - n = 0: no event
 *   - cal is not validated: NaN and inf propagate, nothing faults and nothing outside the caller's rooms is written
 *   - the peak positions strictly increase, so do the starts; records are in emission order
 *   - reads of 2^31 samples and more, where the reference's int peak position wraps: the definition with exact integers
 *
 *   prm      press_hip_event_params_preset(rna, &prm): DNA 3, 6, 1.4, 9.0, 0.2; RNA 7, 14, 2.5, 9.0, 1.0
 *            (events.c:43-54).  w1, w2 must lie in 2 .. 64, else PRESS_HIP_EARG before any device call.
 *   sig / off / n / total_samples / device_resident   as press_hip_signal_stats, with its checks
 *   cal      2 * nreads floats, press_hip_pa_cal's
 *   ev / ev_cap / ev_first / ev_count   the layout of press_hip_press_packed.  ev_first (nreads + 1 entries) is WRITTEN:
 *            ev_first[0] = 0, ev_first[r + 1] = ev_first[r] + the events of read r, whatever ev_cap is: ev_first[nreads]
 *            always says what the batch needs.  Read r's records are ev[ev_first[r] .. ev_first[r + 1]) and
 *            ev_count[r] their number iff ev_first[r + 1] <= ev_cap; otherwise ev_count[r] = UINT32_MAX and no record of
 *            it is written.  Nothing at or beyond ev_cap is ever written.  ev == NULL with ev_cap == 0 is a pure count.
 *            start and length are integers (the reference's length is (float) length, which is what the library uses
 *            inside).
 * device_resident != 0: every pointer but prm is a device pointer; the call only enqueues on the current stream and never
 * waits on the host.  == 0: host pointers, synchronous: the samples are staged and counted, ev_first and ev_count come
 * back - the call's one synchronisation besides the last -, the records' arena is reserved at min(ev_first[nreads],
 * ev_cap) records and comes back in ONE transfer; the room of a read that did not fit arrives as zeros.
 * A NULL argument (other than ev with ev_cap == 0) is PRESS_HIP_EARG before any device call; nreads == 0 is PRESS_HIP_OK
 * (ev_first[0] = 0).
 * One wave walks one read, twice (the count, then the records): the call's time is set by the longest read of the batch,
 * as the range coders' is.
 * press_hip_signal_events_workspace_bytes: the device scratch the device-resident call keeps: 8 bytes per read and 0
 * bytes per sample - the sums never reach memory - so the batch is never cut into slices; exact as
 * press_hip_workspace_bytes is, 0 for an empty batch.
 * press_hip_events_serial_reads: a diagnostic, like press_hip_zstd_host_frames: the reads whose sums took the serial
 * path, in all calls since the library was loaded (it waits for the current stream); 0 without a device.
 */
typedef struct {
	uint32_t w1, w2;
	float threshold1, threshold2, peak_height;
} press_hip_event_params;
typedef struct {
	uint32_t start, length;
	float mean, stdv;
} press_hip_event; /* 16 bytes */
int press_hip_event_params_preset(int rna, press_hip_event_params *prm);
int press_hip_signal_events(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			    uint64_t total_samples, const float *cal, const press_hip_event_params *prm,
			    press_hip_event *ev, uint64_t ev_cap, uint64_t *ev_first, uint32_t *ev_count, int device_resident);
uint64_t press_hip_signal_events_workspace_bytes(uint64_t total_samples, uint32_t nreads);
uint32_t press_hip_events_serial_reads(void);

/*
 * Segments: the stall, homopolymer and poly-A stretches of a read and the end of a dRNA adaptor, found on the device bit
 * for bit as sigtk's `jnn` segmenter and the `jnnv2` adaptor finder behind `prefix` find them (sigtk/src/jnn.c).
 *
 * press_hip_signal_segments is jnn_core (jnn.c:185) over jnn_raw / jnn_pa.  The definition, every operation rounded on
 * its own in single precision, never fused:
 *   signal   cal == NULL, the raw domain (jnn_raw): x[i] = (float) clamp(s[i], 0, 1200)
 *            otherwise (jnn_pa on press_hip_depress_pa_batch's floats): p = ((float) s[i] + cal[2r]) * cal[2r + 1],
 *            x[i] = p > 1200 ? 1200 : p < 0 ? 0 : p - a NaN stays a NaN and is never in range
 *   thresholds   std_scale > 0:  mn = S / (float) n, S the sequential float sum of x from 0 (stat.h:17);
 *            sd = sqrtf(Q / (float) n), Q the sequential float sum of (x[i] - mn) * (x[i] - mn), the difference and the
 *            product each rounded (stat.h:36);  k = sd * std_scale, top = mn + k, bot = mn - k.
 *            Otherwise (NaN included) top and bot are prm's.  The sums are added in the reference's order, nothing else.
 *   walk     jnn.c:200-268 over in = x[i] < top && x[i] > bot, with exact integer counters: w starts at corrector and is
 *            never reset; an in-range sample opens a stretch (start = i) unless one is open, c++, w++, and the run of
 *            errors ends; an out-of-range sample of an open stretch is an error while err < error (c++, err++, run++);
 *            after either, err-- if c >= window && c >= w && c % w == 0.  Any other out-of-range sample closes the
 *            stretch: it is a segment if c >= window, or - only while no segment has been made -
 *            (float) c >= (float) window * stall_len; its end is i - (the run of errors).  A segment whose
 *            start - (the last record's end) < seg_dist is not a new record: it overwrites the last record's end.  A
 *            stretch still open when the read ends is dropped.  n == 0: no segment.
 *   thr      NULL, or 2 * nreads floats: bot, top of read r as the walk used them (prm's when std_scale is not > 0).  A
 *            read of no samples has no thresholds of its own: prm's in that case, else 0, 0.  The segments alone do
 *            not show the order of the sums; thr does.
 *   prm      press_hip_jnn_params_preset(which, &prm): 0 cDNA 0.75, 50, 50, 150, 0.25, 5; 1 dRNA 0.75, 50, 50, 1000, 1.0,
 *            5; 2 poly-A -1, 50, 200, 250, 1.0, 30 (jnn.h:29-61; top = bot = 0, for the caller to set).  window < 1,
 *            corrector < 0, error < 0, seg_dist < 0 and a stall_len that is not finite are PRESS_HIP_EARG before any
 *            device call.
 *   sig / off / n / total_samples / device_resident   as press_hip_signal_events, with its checks, its host-pointer form
 *            (counts, seg_first, seg_count and thr back, then the records in ONE transfer; the room of a read that did
 *            not fit arrives as zeros) and its device-resident form, which only enqueues on the current stream
 *   cal      NULL, or 2 * nreads floats, press_hip_pa_cal's; not validated: NaN and inf propagate, nothing faults
 *   seg / seg_cap / seg_first / seg_count   the layout of press_hip_press_packed, as the events': seg_first (nreads + 1) is
 *            always written in full and seg_first[nreads] is what the batch needs; seg_count[r] = UINT32_MAX for a read
 *            that did not fit, of which nothing is written; nothing at or beyond seg_cap is ever written; seg == NULL
 *            with seg_cap == 0 is a pure count (no writing walk runs).  Records are [start, end), in order.
 * A NULL argument other than cal, thr and seg with seg_cap == 0 is PRESS_HIP_EARG; nreads == 0 is PRESS_HIP_OK
 * (seg_first[0] = 0).
 * Reads of 2^31 samples and more, where the reference's int counters wrap: the definition with exact integers (c and the
 * positions in 32 bits without sign, w and err in 64).  (float) c is then the conversion of the exact count.
 * press_hip_signal_segments_workspace_bytes: the device scratch the device-resident call keeps: 16 bytes per read (the
 * count and the two thresholds) and 0 bytes per sample; exact, 0 for an empty batch.  The adaptor call keeps none.
 *
 * press_hip_signal_adaptor is jnnv2 (jnn.c:98), in the raw domain only, as in sigtk:
 *   a read with n <= window gets the pair (-1, -1) (thr: 0, 0).  Otherwise, with m = n - window:
 *   t[j] = (float) (the sum of clamp(s, 0, 1200) over [j, j + window)) / (float) window for j < m.  The reference keeps a
 *            rolling float sum; it holds integers below 1200 * window, so it is exact while that is below 2^24: window
 *            must lie in 1 .. 8192, else PRESS_HIP_EARG, and the sums are taken as integers
 *   mn, sd   the sequential float formulas above over t[0 .. m);  bot = mn - sd * std_scale
 *   walk     jnn.c:124-151: t < bot opens a dip (start = j) or, in an open one, sets end = j; t > bot closes an open dip
 *            as (start, end) - end is 0 if no second value fell below -, merged into the last record (its end is
 *            overwritten) if start - (its end) < seg_dist, else a new record; t == bot and NaN do nothing; a dip open
 *            at the end is dropped
 *   pair     2 * nreads: of the first record in order with lo_thresh <= end - start <= hi_thresh, AFTER all merging:
 *            start + window / 2 - 1, end + window / 2 - 1 (integer division); (0, 0) if there is none.  Positions of
 *            2^31 and more arrive modulo 2^32.
 *   thr      NULL, or 2 * nreads floats: bot, mn
 *   prm      press_hip_jnn2_params_preset(0, &prm): JNNV2_RNA_ADAPTOR 0.5, 1500, 2000, 200000, 2000 (jnn.h:74-80)
 * One wave walks one read in both calls: their time is that of the batch's longest read.
 */
typedef struct {
	float std_scale;
	int32_t corrector, seg_dist, window;
	float stall_len;
	int32_t error;
	float top, bot;
} press_hip_jnn_params;
typedef struct {
	uint32_t start, end;
} press_hip_segment; /* 8 bytes */
typedef struct {
	float std_scale;
	int32_t seg_dist, window, hi_thresh, lo_thresh;
} press_hip_jnn2_params;
int press_hip_jnn_params_preset(int which, press_hip_jnn_params *prm);
int press_hip_jnn2_params_preset(int which, press_hip_jnn2_params *prm);
int press_hip_signal_segments(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			      uint64_t total_samples, const float *cal, const press_hip_jnn_params *prm,
			      press_hip_segment *seg, uint64_t seg_cap, uint64_t *seg_first, uint32_t *seg_count, float *thr,
			      int device_resident);
uint64_t press_hip_signal_segments_workspace_bytes(uint64_t total_samples, uint32_t nreads);
int press_hip_signal_adaptor(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			     uint64_t total_samples, const press_hip_jnn2_params *prm, int32_t *pair, float *thr,
			     int device_resident);

/*
 * Range statistics and the prefix of a dRNA read: sigtk's `stat` and `prefix` subcommands on the device, bit for bit
 * (sigtk/src/cfunc.c:126-234, stat.h:17-73, misc.c:15-32).
 *
 * press_hip_signal_range_stats: the mean, the deviation and the median of the samples [a, b) of every read, L = b - a of
 * them.  Every operation is rounded on its own in single precision, never fused:
 *   x[i]     cal == NULL, the raw domain (meani16 / stdvi16): (float) s[i], no clamp.  Otherwise picoamperes as
 *            signal_in_picoamps has them: ((float) s[i] + cal[2r]) * cal[2r + 1], no clamp (this is NOT the segmenter's
 *            rm_outlierf)
 *   mean     S / (float) L, S the float sum of x from the range's first sample on, added in that order
 *   stdv     sqrtf(Q / (float) L), Q the float sum in that order of (x[i] - mean) * (x[i] - mean), the difference and the
 *            product each rounded
 *   median   the L / 2-th smallest (0-based) of x, the reference's ks_ksmall(L, copy, L / 2), found as a selection among
 *            the 16-bit keys s + 32768, never among floats: in the raw domain (float) of the selected sample; with cal
 *            and cal[2r + 1] < 0, x of the L / 2-th LARGEST sample, else x of the L / 2-th smallest.  x is monotone in s
 *            for every finite calibration, so this is medianf's value there; for a NaN calibration this formula is the
 *            definition
 *   L == 0   mean and stdv are NaN (what 0 / 0 gives), median is 0; the reference has no value there
 *   range    NULL: the whole read, [0, n[r]).  Otherwise 2 * nreads words a, b in samples from the read's start: b is
 *            clamped to n[r] and a to b.  NO alignment is asked of off[r] + a, and loads stay inside
 *            [off[r] + a, off[r] + b)
 *   cal      NULL, or 2 * nreads floats, press_hip_pa_cal's; not validated: NaN and inf propagate, nothing faults
 *   sig / off / n / total_samples / device_resident   as press_hip_signal_segments, with its checks and its two forms:
 *            host pointers go through the staging layer and the call is synchronous; device resident, the call only
 *            enqueues on the current stream and never waits
 *   out      nreads records
 * A NULL argument other than cal and range is PRESS_HIP_EARG before any device call; nreads == 0 is PRESS_HIP_OK.
 * sigtk's `stat` is this call on whole reads, once with cal == NULL and once with it.
 * One wave takes one range, in two passes over its samples (the sum and the keys' high bytes, the squares and the low
 * bytes); the counting is on integers in LDS, so the result is the same from run to run, and nothing is kept per sample.
 * The call's time is that of its longest range, as the segments' and the events' is that of the longest read.
 *
 * press_hip_signal_prefix is prefix_func (cfunc.c:169-234): where the adaptor ends and where the poly-A tail lies.
 *   adapt_start, adapt_end   press_hip_signal_adaptor's pair under prm->adaptor, unchanged: (-1, -1) for n <= window,
 *            (0, 0) if none was found
 *   only if adapt_end > 0 and prm->rna:  m_a = the range mean above (picoamperes) of [adapt_start, adapt_end),
 *            t = m_a + shift, top = t + half, bot = t - half: three float operations, as C evaluates m_a+30+20.  The
 *            poly-A pair is the FIRST record of press_hip_signal_segments' definition (jnn_pa: clamped picoamperes) over
 *            the suffix [adapt_end, n) under prm->polya with these thresholds whatever its std_scale says, reported as
 *            positions in the read: start + adapt_end, end + adapt_end
 *   in every other case (no adaptor, rna == 0, no segment, a NaN m_a)   polya_start = polya_end = -1
 *   stat     NULL, or 2 * nreads records, the adaptor's then the poly-A's: the range statistics (picoamperes) of
 *            [adapt_start, adapt_end) and [polya_start, polya_end); a stretch that is absent is an empty range (NaN, NaN,
 *            0).  (A start below 0, which only an adaptor window of 1 can give, is beyond every end: an empty range.)
 *   thr      NULL, or 2 * nreads floats: bot, top as the walk used them (NaN for a NaN m_a); 0, 0 where no walk ran
 *   cal      required
 *   prm      press_hip_prefix_params_preset(0, &prm): JNNV2_RNA_ADAPTOR, JNNV1_POLYA, rna 1, shift 30, half 20.  The
 *            parameter checks of press_hip_signal_adaptor (on adaptor) and press_hip_signal_segments (on polya) apply,
 *            before any device call; with stat, nreads is at most 2^31 - 1
 * A NULL argument other than stat and thr is PRESS_HIP_EARG; nreads == 0 is PRESS_HIP_OK.  The two forms are those above.
 * Three launches: the adaptor kernel; a wave per read that adds m_a and walks the suffix for its first record; with stat,
 * the range kernel over 2 * nreads ranges.  The call's time is that of the batch's longest read.
 * press_hip_signal_prefix_workspace_bytes: the device scratch the device-resident call keeps, 24 bytes per read (the
 * adaptor's pairs, the two ranges) and 0 per sample; exact, 0 for an empty batch.  The range call keeps none.
 */
typedef struct {
	float mean, stdv, median;
} press_hip_range_stat; /* 12 bytes */
typedef struct {
	press_hip_jnn2_params adaptor;
	press_hip_jnn_params polya;
	int32_t rna;
	float shift, half;
} press_hip_prefix_params;
typedef struct {
	int32_t adapt_start, adapt_end, polya_start, polya_end;
} press_hip_prefix; /* 16 bytes */
int press_hip_signal_range_stats(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				 uint64_t total_samples, const float *cal, const uint32_t *range,
				 press_hip_range_stat *out, int device_resident);
int press_hip_prefix_params_preset(int which, press_hip_prefix_params *prm);
int press_hip_signal_prefix(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			    uint64_t total_samples, const float *cal, const press_hip_prefix_params *prm,
			    press_hip_prefix *out, press_hip_range_stat *stat, float *thr, int device_resident);
uint64_t press_hip_signal_prefix_workspace_bytes(uint32_t nreads);

/*
 * Dataset analysis: value, delta and transition tallies and per-read moments - what the reference's
 * viz/freq_slow5, viz/freq_delta_slow5, viz/get_exceptions and press/stats.c compute on the host, in ONE pass over a batch.
 *
 * For read r with c = n[r] samples s[0 .. c):
 *     zz(v)  = (uint16_t) ((v << 1) ^ (v >> 15))  for an int16 v: the index of viz/tally.h, trans.c's zig-zag
 *     d[i]   = (int16_t) (s[i] - s[i-1])          for i in [1, c), wrapped to 16 bits
 *     sym[i] = min(zz(d[i]), 256)                 what the shuffman_* and range-coder methods code; 256: the exceptions
 *   raw      NULL, or 65536 counters:    raw[zz(s[i])] += 1                       for i in [0, c)
 *   delta    NULL, or 65536 counters:    delta[zz(d[i])] += 1                     for i in [1, c); delta[0 .. 255] is what
 *            press_hip_symbol_counts adds to its counts[0 .. 255], the sum of delta[256 ..] what it adds to counts[256]
 *   trans    NULL, or 257 * 257 counters: trans[257 * sym[i-1] + sym[i]] += 1     for i in [2, c)
 *   mom      NULL, or nreads records:  sum and sumsq of the samples, min and max (32767 and -32768 for an empty read, as
 *            init_stats leaves them), n = c, and nex = the number of i in [1, c) with d[i] outside [-128, 127]
 *            (zz(d[i]) > 255).  Exact integers; sumsq cannot wrap (2^32 samples of at most 2^30)
 * The three tables are ADDED to, as press_hip_symbol_counts adds: a caller accumulates over batches and zeroes them itself.
 * mom is SET.  Nothing else is written.  All outputs NULL, or nreads == 0, is PRESS_HIP_OK after the checks.
 *   sig / off / n / total_samples / device_resident   as press_hip_symbol_counts, with its checks: off[] multiples of 8;
 *            reads may overlap or repeat and are then counted twice.  Device resident: every pointer is a device pointer
 *            and the call only enqueues on the current stream; the work list has room for total_samples / 32768 + nreads + 1
 *            chunks of 32768 samples, so a batch whose reads overlap passes the sum of n[] where that is larger.
 *            Host pointers: synchronous, through the staging layer; the call adds to the caller's host tables.
 * Every sum is one of integers: the same on every run.
 * press_hip_signal_tally_workspace_bytes: the device scratch the device-resident call keeps, 8 bytes per chunk and 64;
 * exact, 0 for an empty batch.
 */
#define PRESS_HIP_TALLY_BINS 65536                   /* counters of raw and of delta */
#define PRESS_HIP_TALLY_SYMS 257                     /* trans is PRESS_HIP_TALLY_SYMS squared counters */
#define PRESS_HIP_TALLY_WORDS (2 * 65536 + 257 * 257) /* the three tables together */
typedef struct {
	int64_t sum;
	uint64_t sumsq;
	int32_t min, max;
	uint32_t n, nex;
} press_hip_moments; /* 32 bytes */
int press_hip_signal_tally(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			   uint64_t total_samples, uint64_t *raw, uint64_t *delta, uint64_t *trans,
			   press_hip_moments *mom, int device_resident);
uint64_t press_hip_signal_tally_workspace_bytes(uint64_t total_samples, uint32_t nreads);

/*
 * Lossy archives: dropping the low b bits of every sample, on the device.
 *
 * The definition.  For bits = b in 0 .. 8 and a sample s (int16), computed in 32-bit integers:
 *     D_0(s) = s
 *     D_b(s) = min( ((s + 2^(b-1)) >> b) << b ,  32768 - 2^b )          (arithmetic shift)
 * the nearest multiple of 2^b, ties towards +infinity, saturating at the largest multiple of 2^b an int16 holds - it
 * never wraps; -32768 is a multiple of every 2^b and needs no clamp.  D_b is idempotent and monotone, and
 * |D_b(s) - s| <= 2^(b-1), except in the saturated top bucket, where it is below 2^b.  This is believed to be the rounding
 * of slow5tools' `degrade` apart from the saturation; that is from memory and NOT checked: no compatibility is claimed.
 * bits > 8 is PRESS_HIP_EARG in every call below, before the method ids are looked at and before any device call.
 *
 * press_hip_degrade_value: the definition as host arithmetic, no GPU (bits > 8: s as it is).
 *
 * press_hip_degrade_batch: out[off[r] + i] = D_b(sig[off[r] + i]) for i < n[r].
 *   sig / off / n / total_samples / device_resident   as press_hip_press_batch, with its checks (off[] multiples of 8
 *            samples, a device sig 16-byte aligned, non-overlap on the host path).  Loads stay inside
 *            [off[r], off[r] + roundup8(n[r])).
 *   out      laid out as sig; device resident 16-byte aligned (PRESS_HIP_EARG).  out == sig (in place) is allowed.
 *            Nothing outside [off[r], off[r] + n[r]) is written: a read's last group of fewer than 8 samples is stored
 *            sample by sample.  Host buffers receive exactly n[r] samples per read.
 *   device_resident != 0: the call only enqueues.  == 0: the samples are staged, the call is synchronous.
 *
 * press_hip_recode_degraded_batch / _sizes / _packed: press_hip_recode_batch / _sizes / _packed with `bits` behind
 * dst_method.  Meaning: decode src, apply D_b, press with dst - the streams, out_len, need, out_off are byte for byte what
 * press_hip_press_batch / _sizes / _packed (dst_method) give on D_b of the decoded samples.  sig, where the caller asks
 * for samples, receives the DEGRADED samples: what the new streams decode to.  Refused source reads, out_n, the slot
 * rules, the packed layout and align, the range coders' need and every check stay as in the undegraded calls.
 * bits == 0 takes the undegraded calls' code path and gives their bytes.  bits > 0, two routes, chosen as
 * press_hip_recode_fused chooses: where it is 1 the svb decode kernel applies D_b to the samples it holds in registers,
 * behind its inverse scan and in front of its store and of the exception and code-bit counts it leaves for the press half,
 * which therefore describe the degraded read - no further pass over the samples.  Every other pair decodes into the
 * samples (the zstd kinds' host fallback included), press_hip_degrade_batch's kernel runs in place over out_n[r] samples
 * of every decoded read, and the press half follows.
 * press_hip_recode_degraded_sizes answers "how much smaller would this archive be without its b low bits" with no arena.
 * press_hip_recode_degraded_workspace_bytes / _packed_workspace_bytes: press_hip_recode_workspace_bytes /
 * _packed_workspace_bytes unchanged for bits == 0 and for a fused pair; for any other pair with bits > 0 that figure plus
 * the degrade kernel's tile table ((total_samples / 32768 + nreads + 1) * 8 bytes and a 64-byte counter) - never below;
 * 0 for a bad method id or bits.
 *
 * press_hip_verify_degraded_batch: press_hip_verify_batch with `bits` behind method.  sig holds the ORIGINAL samples; the
 * decoded samples are compared with D_b of them, taken in registers inside the compare kernel - no degraded copy of the
 * originals is made.  first_bad, nbad, out_n and PRESS_HIP_VERIFIED keep their meanings; bits == 0 is
 * press_hip_verify_batch.  The workspace is press_hip_verify_workspace_bytes.
 */
int16_t press_hip_degrade_value(int16_t s, uint32_t bits);
int press_hip_degrade_batch(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			    uint64_t total_samples, uint32_t bits, int16_t *out, int device_resident);
int press_hip_recode_degraded_batch(int src_method, int dst_method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
				    const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
				    uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
				    int16_t *sig, uint32_t *out_n, int device_resident);
int press_hip_recode_degraded_sizes(int src_method, int dst_method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
				    const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
				    uint64_t total_samples, uint64_t *need, int16_t *sig, uint32_t *out_n, int device_resident);
int press_hip_recode_degraded_packed(int src_method, int dst_method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
				     const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
				     uint64_t total_samples, uint8_t *out, uint64_t out_cap, uint32_t align,
				     uint64_t *out_off, uint64_t *out_len, int16_t *sig, uint32_t *out_n, int device_resident);
uint64_t press_hip_recode_degraded_workspace_bytes(int src_method, int dst_method, uint32_t bits, uint64_t total_samples,
						   uint32_t nreads, int keep_samples);
uint64_t press_hip_recode_degraded_packed_workspace_bytes(int src_method, int dst_method, uint32_t bits, uint64_t total_samples,
							  uint32_t nreads, int keep_samples);
int press_hip_verify_degraded_batch(int method, uint32_t bits, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
				    uint32_t nreads, const int16_t *sig, const uint64_t *off, const uint32_t *n,
				    uint64_t total_samples, uint32_t *first_bad, uint32_t *out_n, uint32_t *nbad,
				    int device_resident);

/*
 * PRESS_HIP_ZSTD_SVB_ZD, _ZSTD_SVB12_ZD and _ZSTD_HASGAM_ZDQ in the calls above (SURVEY.md 8f-3,
 * replaces the ZSTD_compress / ZSTD_decompress calls of press.c:1860-1910, 2020-2070, 8549-8589 for batches):
 *   press    writes one standard zstd frame (RFC 8878) per read whose content is the buffer
 *            the reference hands to ZSTD_compress ([u32 n][svb stream], or the ex-zd stream): a raw
 *            block with the count (ex-zd: header + exception section), RLE blocks for the svb key
 *            bytes, the one-byte values in Huffman-coded literal blocks of 16 KiB
 *            (one table per read, no sequences).  Any zstd decoder reads it - the reference's
 *            zstd_svb_zd_depress_16 included; the BYTES are not libzstd's (they never were
 *            pinned: they depend on the libzstd version).  Size <= 9 + L + 3 * ceil(L / 128 KiB)
 *            for a content of L bytes, well inside press_hip_bound().
 *   depress  reads any single zstd frame of such a buffer on the device: the frames above and
 *            ZSTD_compress's own (the reference's streams, press.c:1462-1469) - Huffman literals,
 *            FSE-coded sequences with all four table modes, repeat offsets - one wave per frame walks
 *            the blocks, the literals are decoded in parallel, one wave per frame carries out its
 *            sequences.  Only frames with a dictionary, a 12-bit Huffman table, more sequences, trees or
 *            blocks than the batch's scratch takes, several frames in one stream or a skippable frame in
 *            front or behind are decompressed by libzstd on the host inside the call.  NOTE: a zstd depress call waits on the host until the frames have been
 *            walked (the count of such frames comes back through page-locked memory behind an event), also
 *            when device_resident != 0 - the device meanwhile goes on with the rest of the batch, and the
 *            call does not wait for that; only a batch WITH such frames synchronises the stream.
 *            n[r] is the room in samples; the count in the stream decides (press.c:1901).  A frame's
 *            Content_Checksum (XXH64; ZSTD_compress writes none) is verified as libzstd does: on the
 *            device, by one lane per such frame, and a read whose sum is wrong is refused.
 */
/* frames the last zstd depress batch left to libzstd on the host (0 for this library's frames and for
 * ZSTD_compress's) */
uint32_t press_hip_zstd_host_frames(void);

/*
 * Host buffers (device_resident == 0).  Ordinary (pageable) memory is copied through two page-locked
 * staging buffers of 32 MiB (the DMA of one overlaps the host's memcpy into / out of the other);
 * compressed streams cross the link packed back to back, whatever the slots' sizes.  Buffers from
 * press_hip_host_alloc() are page-locked: `sig` is then copied by ONE DMA in press, and in depress the
 * decoded samples are written straight into it (the alignment padding between reads is overwritten).
 * Both calls return when the caller's buffers are complete.
 */
void *press_hip_host_alloc(uint64_t bytes); /* hipHostMalloc; NULL on failure */
void press_hip_host_free(void *p);

/* bytes of device scratch the two calls above keep for a batch of this shape.  Exact: for every buffer the larger of
 * what press and depress request (the buffers are shared and grow-only), plus the device table for the static-Huffman
 * methods (whose decoder's share depends on the table in force) - the requested bytes, before the growth slack of
 * n / 8 + 4096 each allocation adds.  Host arithmetic, no GPU needed; 0 for a method id out of range. */
uint64_t press_hip_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads);

/* Measurement aid (bench.py): when enabled, every batch call brackets its dominant kernel
 * (the svb encode / decode kernel, the one-byte-stream kernels of the exception methods)
 * with HIP events on the launch stream.  press_hip_kernel_times(which, ms, max) returns the
 * elapsed times recorded since timing was (re-)enabled; which: 0 = press, 1 = depress. */
int press_hip_kernel_timing(int enable);
int press_hip_kernel_times(int which, float *ms, int max);

/* release every device and host resource held by the library (all scratch buffers, the device
 * copy of the Huffman table, the private stream).  press_hip_set_device(other) goes through it. */
void press_hip_shutdown(void);
/* number of scratch buffers the library keeps; *bytes (may be NULL) = device bytes they hold now
 * (0 after press_hip_shutdown) */
uint32_t press_hip_scratch_buffers(uint64_t *bytes);
/* Diagnostic (tests; on no hot path): overwrite the library's scratch with `byte` (its low 8 bits), so that a later call
 * shows whether any kernel reads a word that this call has not written.  One hipMemsetAsync over the whole capacity of
 * every scratch buffer that holds memory, enqueued on the library's current stream, then - behind a synchronisation
 * of that stream - a host memset of the two page-locked staging buffers.  Spared: the device copy of the
 * static-Huffman table, the only scratch whose content is meant to outlive a call (it is written by the table calls
 * and read by every shuffman_* batch).  Nothing is allocated, freed or resized: press_hip_scratch_buffers reports
 * the same figures before and after.  PRESS_HIP_EHIP without a device. */
int press_hip_scratch_fill(int byte);

/* ======================================================================= (2s) the stall methods */

/*
 * rccm_svbbe21_zd, dstall_fz_1500 and dstall_fz (press.c:7716-8148): the read is cut at a stall - the first segment
 * (x, y) that sigtk's jnn_raw finds under JNNV1_CDNA_PARAM - and the stall and the rest are coded apart.  A family of
 * its own with ids of its own; enum press_hip_method and PRESS_HIP_NMETHODS do not know them, and the generic batch calls
 * do not accept the family's own ids 0 .. 2 - (2x) gives the method id that they take.
 *
 *   stream   [exists u8]  exists: [stall_start u16][stall_len u16][nstall u16][stall piece]  always: [nrest u32][rest piece]
 *   rest     rccm_vbbe21_zd of the read without the samples [stall_start, stall_start + stall_len)
 *   stall    rccm_vbbe21_submin of those samples as uint16: [min u16][vbbe21 section of x - min][one-byte values, rcms]
 *   where    stall_start = (uint16_t) x, stall_len = (uint16_t) (y - x + 1) - the reference's truncations, kept; with the
 *            threshold T: stall_len < T: no stall; else stall_start += 20 (in 16 bits), stall_len -= 40
 *   T        rccm_svbbe21_zd 140, dstall_fz_1500 1500; dstall_fz makes the T = 140 stream and keeps it only where it is
 *            strictly shorter than the read's bare rccm_vbbe21_zd stream (press.c:8006), else [0][u32][that stream]
 * One decoder reads all three.  As in the svb family its nin carries the SAMPLE count, not the bytes (press.c:7871).
 *
 * Where the reference defines nothing, this library does:
 *   1. No segment from jnn (n = 0 and every read the segmenter yields nothing for): no stall.  (The reference compares
 *      an uninitialised stall_len with T there, press.c:7737, 7763.)
 *   2. A stall piece of more than 65535 bytes - the reference truncates the count to 16 bits and writes a stream that does
 *      not decode: rccm_svbbe21_zd and dstall_fz_1500 refuse the read (PRESS_HIP_FAILED), dstall_fz takes the form
 *      without a stall.
 *   3. A stream the decoder cannot trust is refused for that read before a byte of a piece is touched: exists neither 0
 *      nor 1, stall_start + stall_len > n, a piece length that runs past in_len, an inner stream its own decoder
 *      refuses.  The batch call marks it as every decoder of this library does, out_n[r] = UINT32_MAX; the per-read
 *      symbols give *nout = 0.
 * An empty read is refused, as rccm_vbbe21_zd refuses it.
 */
enum press_hip_stall_method {
	PRESS_HIP_STALL_RCCM_SVBBE21_ZD = 0,
	PRESS_HIP_STALL_DSTALL_FZ_1500  = 1,
	PRESS_HIP_STALL_DSTALL_FZ       = 2,
	PRESS_HIP_NSTALL                = 3
};

/* the reference's per-read symbols (press.h), synchronous; *nout of press: the capacity in, the length out (0: refused).
 * depress: nin = the read's SAMPLE count; the bytes read are those the stream's own header announces. */
uint64_t rccm_svbbe21_zd_bound_16(uint32_t nin);
void rccm_svbbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rccm_svbbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t dstall_fz_1500_bound_16(uint32_t nin);
void dstall_fz_1500_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void dstall_fz_1500_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t dstall_fz_bound_16(uint32_t nin);
void dstall_fz_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void dstall_fz_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* the reference's X_bound_16: rccm_vbbe21_zd_bound_16(n) for all three; 0 for an id out of range */
uint64_t press_hip_stall_bound(int stall_method, uint32_t n);

/*
 * The batch calls: arguments, layout rules and the meaning of device_resident as in press_hip_press_batch /
 * press_hip_depress_batch (device resident: the call only enqueues on the current stream).
 *   stall   NULL, or 2 * nreads words: (stall_start, stall_len) as written into read r's stream, (0, 0) where the stream
 *           has no stall or the read failed
 *   out_len the stream's bytes; PRESS_HIP_FAILED for a read that does not fit its slot (nothing outside a slot is
 *           written, and nothing inside the slot of a read that fails), is empty, or is refused by rule 2
 * depress: n[r] is the read's exact sample count (the range coder's streams do not carry it); out_n[r] = n[r], or
 * UINT32_MAX for a refused read, whose room is not written.
 */
int press_hip_stall_press_batch(int stall_method, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint32_t *stall,
				int device_resident);
int press_hip_stall_depress_batch(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint32_t nreads, int16_t *sig,
				  const uint64_t *off, const uint32_t *n, uint64_t total_samples, uint32_t *out_n, int device_resident);
/* device scratch the two device-resident calls keep for a batch of this shape (the larger of the two per buffer): the
 * inner method's, the pieces' samples (dstall_fz: up to twice the batch) and, for press, 6 bytes per piece sample of
 * streams - the most a stream can take, so that only the caller's slot decides whether a read fits.  0 for a bad id. */
uint64_t press_hip_stall_workspace_bytes(int stall_method, uint64_t total_samples, uint32_t nreads);

/* ======================================================================= (2t) the range-coder family */

/*
 * The reference pairs each of its four range coders with each of its four exception layouts (press.h:712-899): sixteen
 * methods {rc, rcc, rccm, rccdf}_{vbe21, vbbe21, vbsbe21, vbsse21}_zd.  A stream is the layout's header and exception
 * section as the plain method L_zd writes them, then the read's one-byte values through the coder.  Three of the pairs are
 * public methods (rc_vbe21_zd, rcc_vbe21_zd, rccm_vbbe21_zd: the same kernels, the same bytes); the family reaches all
 * sixteen, with ids of its own: enum press_hip_method and PRESS_HIP_NMETHODS do not know them, and the generic batch calls
 * do not accept the family's own ids - (2w) gives the id of every pair that they do take.
 *
 *   rc      TurboRC's order-0 binary coder (rcsenc), rcc its order-1 coder (rccsenc), rccm its order 1-0 context mixing
 *           (rcmsenc) - as in the three public methods
 *   rccdf   TurboRC's adaptive nibble-CDF coder (rccdfenc / rccdfdec): two 16-ary decisions per byte, 17 tables of 16
 *           cumulative frequencies, each moving towards the coded symbol by 1/128.  The stream depends on how rccdf.c was
 *           compiled: with __AVX2__ it uses a 32-bit range, 14-bit frequencies and 16-bit output.  This library writes
 *           and reads the variant WITHOUT __AVX2__ - 64-bit range, 15-bit frequencies, 32-bit little-endian words -
 *           because TurboRC's own makefile leaves AVX2 off; a reference built with -mavx2 or -march=native on such a host
 *           makes other bytes.
 *
 * Raw-stored payloads.  Every one of the four coders gives up once its output reaches nlow * 255 / 256 - 8 bytes (nlow:
 * the read's one-byte values) and stores the nlow bytes verbatim; every read of at most nine one-byte values ends so.
 * Nothing in the stream says that this happened, and the decoder - the reference's and this library's - decodes such a
 * payload like any other: the read does NOT come back.  press reports it instead:
 *   raw     NULL, or nreads bytes: raw[r] = 1 where the payload of read r has nlow bytes and equals the one-byte values
 *           byte for byte (the coder gave up), else 0 (also for a read that failed).  A caller who needs the read back
 *           stores such a read with another method.
 * Slots: a stream needs at most its section plus nlow + 32 bytes; press_hip_rcf_bound, the reference's X_bound_16
 * (that of the plain layouts for all sixteen; 0 for an id out of range), covers it on signal data.
 * A stream that ends early is decoded with zeros behind its end; nothing outside a read's stream is read.
 *
 * The batch calls: arguments, layout rules and the meaning of device_resident as in press_hip_press_batch /
 * press_hip_depress_batch (device resident: the call only enqueues on the current stream; raw is then a device pointer).
 * depress: n[r] is the read's exact sample count (the streams do not carry it).  A bad coder or layout id or a NULL
 * argument (raw excepted) is PRESS_HIP_EARG before any device call; nreads == 0 is PRESS_HIP_OK.
 *
 * The family's own ids (coder, layout) are accepted by these calls alone: the recode, picoampere, normalise, chunk-row,
 * verify, CRC, sizes and packed calls do not learn them - they take the pair's extended method id of (2w) - and
 * neither do the calls of the Rice family (2u), which takes the layout ids alone.  Not built: rccm_svb_zd,
 * rccm_svb12_zd, the range-coder methods without zd, jumps.
 */
enum press_hip_rcf_coder {
	PRESS_HIP_RCF_RC      = 0,
	PRESS_HIP_RCF_RCC     = 1,
	PRESS_HIP_RCF_RCCM    = 2,
	PRESS_HIP_RCF_RCCDF   = 3,
	PRESS_HIP_NRCF_CODERS = 4
};
enum press_hip_rcf_layout {
	PRESS_HIP_RCF_VBE21    = 0,
	PRESS_HIP_RCF_VBBE21   = 1,
	PRESS_HIP_RCF_VBSBE21  = 2,
	PRESS_HIP_RCF_VBSSE21  = 3,
	PRESS_HIP_NRCF_LAYOUTS = 4
};
uint64_t press_hip_rcf_bound(int coder, int layout, uint32_t n);
int press_hip_rcf_press_batch(int coder, int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			      uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint8_t *raw,
			      int device_resident);
int press_hip_rcf_depress_batch(int coder, int layout, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
				uint32_t nreads, int16_t *sig, const uint64_t *off, const uint32_t *n, uint64_t total_samples,
				uint32_t *out_n, int device_resident);

/* the reference's per-read symbols of the thirteen pairs that are not public methods (press.h:752-899), synchronous, as
 * rc_vbe21_zd_press_16 and its kin above: *nout of press the capacity in, the length out (0: refused); *nout of depress
 * the exact sample count in */
uint64_t rc_vbbe21_zd_bound_16(uint32_t nin);
void rc_vbbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rc_vbbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rc_vbsbe21_zd_bound_16(uint32_t nin);
void rc_vbsbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rc_vbsbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rc_vbsse21_zd_bound_16(uint32_t nin);
void rc_vbsse21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rc_vbsse21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rcc_vbbe21_zd_bound_16(uint32_t nin);
void rcc_vbbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rcc_vbbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rcc_vbsbe21_zd_bound_16(uint32_t nin);
void rcc_vbsbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rcc_vbsbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rcc_vbsse21_zd_bound_16(uint32_t nin);
void rcc_vbsse21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rcc_vbsse21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rccm_vbe21_zd_bound_16(uint32_t nin);
void rccm_vbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rccm_vbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rccm_vbsbe21_zd_bound_16(uint32_t nin);
void rccm_vbsbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rccm_vbsbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rccm_vbsse21_zd_bound_16(uint32_t nin);
void rccm_vbsse21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rccm_vbsse21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rccdf_vbe21_zd_bound_16(uint32_t nin);
void rccdf_vbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rccdf_vbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rccdf_vbbe21_zd_bound_16(uint32_t nin);
void rccdf_vbbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rccdf_vbbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rccdf_vbsbe21_zd_bound_16(uint32_t nin);
void rccdf_vbsbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rccdf_vbsbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rccdf_vbsse21_zd_bound_16(uint32_t nin);
void rccdf_vbsse21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rccdf_vbsse21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ======================================================================= (2u) the Rice family */

/*
 * The reference's table-free entropy stage: rice_{vbe21, vbbe21, vbsbe21, vbsse21}_zd (press.h:664-701, press.c:4854-5390),
 * Golomb-Rice coding of the read's one-byte values behind the layout's header and exception section.  No table, no
 * adaptive state: a code's length is a function of the value and of one parameter k per read, so press is a count, a scan
 * and a bit scatter and depress a self-synchronising prefix code, both parallel within a read.  A family with ids of its
 * own like (2t): the layout ids are enum press_hip_rcf_layout; enum press_hip_method and PRESS_HIP_NMETHODS do not know
 * these methods, and the generic batch calls, the recode, picoampere, normalise, chunk-row, verify, CRC and packed calls
 * do not accept the family's own ids: (2w) gives the method id that they take.
 *
 * The stream.  With P(L) the plain stream of L_zd, nex its exception count, nlow = n - 1 - nex and
 * sec(L) = P(L)[: len - nlow], the stream of rice_L_zd is sec(L) + rice(low), low being the read's nlow one-byte values
 * (the same under all four layouts).  rice(low), press.c:4860-4924:
 *   bit order  bit i of the payload is bit i % 8, counted from the least significant, of byte i / 8 (the opposite of the
 *              Huffman stream)
 *   k          bits 0, 1, 2 hold k >> 2 & 1, k >> 1 & 1, k & 1
 *   a value x  x >> k one-bits, a zero bit, the low k bits of x from the most significant down
 *   choice     k is the smallest of 0 .. 7 that minimises the sum of (x >> k) + 1 + k over the values, taken in 64 bits
 *              (the reference compares with '<': ties go to the lower k); without a value, k = 0
 *   length     nbits = 3 + that sum, (nbits - 1) / 8 + 1 bytes: never fewer than one
 *
 * Where the reference leaves a hole, this library defines:
 *   1. padding    The reference builds the payload in an uninitialised block and touches only bits below nbits: the bits
 *                 behind nbits in the last byte are whatever the heap held.  This library writes zeros there; "equal to
 *                 the reference" means equal after clearing those bits of the reference's last byte.
 *   2. decoder    (press.c:4927-4978) the unary run is counted modulo 256 (q is a uint8_t), however long it is; the value
 *                 is (uint8_t) ((q << k) | rem).  The reference reads on behind the stream's end; this library reads
 *                 nothing outside [in_off, in_off + in_len), and bits behind the end are zero (the rule of (2t): a stream
 *                 that ends early is decoded with zeros behind its end).  A stream shorter than its own section is
 *                 refused: out_n[r] = 0.
 *   3. sections   For vbbe21, vbsbe21 and vbsse21 the reference keeps the section length in a uint16_t (press.c:5087 and
 *                 its siblings) and mis-splices a section of 65536 bytes or more.  This library's stream is the splice
 *                 above for any section length; it equals the reference's wherever the section is shorter than that.
 *   4. tiny reads rice_bound(nlow) = nlow * 1.5 is smaller than the payload for nlow == 0 and for some reads with
 *                 nlow == 1: the reference writes a byte past a block.  This library's stream is what the rules above
 *                 give; for n = 1: the 2-byte first sample, the empty section (nex = 0), one payload byte 0x00.
 *   5. bounds     press_hip_rice_bound is the reference's X_bound_16 (vb1e2_zd_bound_16 for all four; 0 for a bad id).
 *                 The exact size is known before a byte is written (press_hip_rice_press_sizes).  A read whose slot is
 *                 too small fails as in press_hip_press_batch (out_len[r] = PRESS_HIP_FAILED); the other reads are
 *                 untouched.
 *
 *   k        NULL, or nreads bytes: the parameter read r was coded with (0 for a read that was refused); a device pointer
 *            when device_resident
 *   need[r]  press_hip_rice_press_sizes: the exact stream length of read r, section plus payload (PRESS_HIP_FAILED for an
 *            empty read); no arena, nothing else is written
 * Everything else - argument and layout rules, PRESS_HIP_EARG for a bad layout id or a NULL argument (k excepted) before
 * any device call, nreads == 0, the host-pointer form, "device resident: the call only enqueues on the current stream",
 * depress: n[r] is the read's exact sample count - is as for press_hip_rcf_press_batch / press_hip_rcf_depress_batch.
 * Depress runs a fixed number of launches: subsequences whose guessed start is wrong are repaired in two rounds, what is
 * still unsettled is decoded by a serial walk per read (slow, right for any stream).  press_hip_rice_repairs: the
 * subsequences the two rounds decoded again and the values the walk decoded in the last depress call (it synchronises).
 */
uint64_t press_hip_rice_bound(int layout, uint32_t n);
int press_hip_rice_press_batch(int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			       uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint8_t *k,
			       int device_resident);
int press_hip_rice_press_sizes(int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
			       uint64_t total_samples, uint64_t *need, uint8_t *k, int device_resident);
int press_hip_rice_depress_batch(int layout, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint32_t nreads,
				 int16_t *sig, const uint64_t *off, const uint32_t *n, uint64_t total_samples, uint32_t *out_n,
				 int device_resident);
int press_hip_rice_repairs(uint32_t *counts);

/* the reference's per-read symbols (press.h:673-701), synchronous, as the range-coder symbols above: *nout of press the
 * capacity in, the length out (0: refused); depress takes the SAMPLE count as nin (press.c:5050), *nout the capacity in */
uint64_t rice_vbe21_zd_bound_16(uint32_t nin);
void rice_vbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rice_vbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rice_vbbe21_zd_bound_16(uint32_t nin);
void rice_vbbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rice_vbbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rice_vbsbe21_zd_bound_16(uint32_t nin);
void rice_vbsbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rice_vbsbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t rice_vbsse21_zd_bound_16(uint32_t nin);
void rice_vbsse21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
void rice_vbsse21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ======================================================================= (2v) the per-read Huffman family */

/*
 * The reference's entropy stage that needs no fitted table and still reaches the static table's ratio:
 * huffman_{vbe21, vbbe21, vbsbe21, vbsse21}_zd (press.h:602-631, press.c:3960-4407, huffman/huffman.c:984-1072).  A Huffman
 * code is built from each read's own one-byte values and written in front of the payload.  No adaptive state: press is a
 * histogram, a tree per read, a scan and a bit scatter, depress a self-synchronising prefix code, both parallel within a
 * read.  A family with ids of its own like (2t) and (2u): the layout ids are enum press_hip_rcf_layout; enum
 * press_hip_method and PRESS_HIP_NMETHODS do not know these methods, and the generic batch calls, the recode, picoampere,
 * normalise, chunk-row, verify, CRC and packed calls do not accept the family's own ids: (2w) gives the method id that
 * they take.
 *
 * The stream.  With P(L), nex, nlow and sec(L) as in (2u), the stream of huffman_L_zd is sec(L) + huffman(low):
 *   counts   the symbols present are ordered ascending by count, ties by ascending symbol value
 *   tree     until one node is left: the first two nodes of the list, m1 and m2, get a parent with count m1 + m2, m1 its
 *            zero child and m2 its one child; the parent goes back in front of every remaining node whose count is not
 *            smaller than its own (so in front of equal leaves and of equal parents made earlier)
 *   codes    a symbol's code is its path from the root, zero or one per edge, first edge first
 *   table    one byte (nsym - 1) & 255; nlow as a big-endian u32; per present symbol in ascending symbol order
 *            { u8 symbol, u8 len, ceil(len / 8) code bytes }, code bit k in bit k % 8, from the least significant, of
 *            code byte k / 8
 *   payload  the codes of the values in order, first code bit first; payload bit i in bit i % 8, from the least
 *            significant, of byte i / 8; the last byte zero padded
 * With nlow < 2^32 no code is longer than about 46 bits (a code of depth d needs F(d + 2) values); 64 bits hold every code
 * press can make, 32 do not (34 symbols with Fibonacci counts: 33 bits).
 *
 * Where the reference leaves a hole, this library defines:
 *   1. one value   One distinct one-byte value (a constant stretch, n = 2): the reference aborts in press.  This library
 *                  writes what the rules give: count byte 0x00, nlow, the one entry { symbol, 0 } without a code byte,
 *                  no payload byte; its decoder gives nlow copies of the symbol.
 *   2. no value    n = 1, or every value an exception: ff 00 00 00 00, as the reference writes it (its own depress
 *                  fails on that stream).  The decoder reads a table whose count field is 0 as empty whatever the first
 *                  byte says, and returns the read.
 *   3. sections    For vbbe21, vbsbe21 and vbsse21 the reference keeps the section length in a uint16_t (press.c:4076);
 *                  this library's stream is the splice above for any section length.
 *   4. decoder     A table is valid when it has 1 to 256 entries, every length is in 1 .. 63 (or it is the single entry
 *                  of length 0), the codes are prefix-free and the table ends inside the stream; a symbol may appear
 *                  twice and the table may be incomplete.  A read is refused, as every decoder of this library marks it
 *                  (out_n[r] = UINT32_MAX), when its table is invalid, when the table's count is not n[r] - 1 - nex,
 *                  when bits inside the payload are no code, or when the payload ends before nlow values are out.  The
 *                  other reads of the batch are untouched, and nothing outside [in_off, in_off + in_len) is read.
 *   5. bounds      press_hip_huffman_bound is the reference's X_bound_16 (vb1e2_zd_bound_16 for all four; 0 for a bad
 *                  id).  The exact size is known before a byte is written (press_hip_huffman_press_sizes).  A read whose
 *                  slot is too small fails alone (out_len[r] = PRESS_HIP_FAILED).
 *
 *   maxlen   NULL, or nreads bytes: the longest code of read r's table (0 for cases 1 and 2 and for a refused read); a
 *            device pointer when device_resident
 *   need[r]  press_hip_huffman_press_sizes: the exact stream length of read r (PRESS_HIP_FAILED for an empty read); no
 *            arena, nothing else is written
 * Everything else - arguments, layouts, PRESS_HIP_EARG, the host-pointer form, "device resident: the call only enqueues
 * on the current stream", depress: n[r] is the read's exact sample count - is as in (2u).  Depress runs a fixed number of
 * launches, with four repair rounds and a serial walk per read for what they leave.  press_hip_huffman_repairs: the
 * subsequences the first round decoded again, those the later rounds did, and the values the walk decoded in the last
 * depress call of this family or of (2u), whose counters these are (it synchronises).
 */
uint64_t press_hip_huffman_bound(int layout, uint32_t n);
int press_hip_huffman_press_batch(int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				  uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint8_t *maxlen,
				  int device_resident);
int press_hip_huffman_press_sizes(int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				  uint64_t total_samples, uint64_t *need, uint8_t *maxlen, int device_resident);
int press_hip_huffman_depress_batch(int layout, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint32_t nreads,
				    int16_t *sig, const uint64_t *off, const uint32_t *n, uint64_t total_samples, uint32_t *out_n,
				    int device_resident);
int press_hip_huffman_repairs(uint32_t *counts);

/* the reference's per-read symbols (press.h:602-631), synchronous: 0, or -1 with *nout = 0.  *nout of press the capacity
 * in, the length out; depress takes the stream's byte count as nin and the capacity in samples in *nout: the sample count
 * is read from the stream (nex and the table's count), and a stream that says more than the capacity is refused */
uint64_t huffman_vbe21_zd_bound_16(uint32_t nin);
int huffman_vbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int huffman_vbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t huffman_vbbe21_zd_bound_16(uint32_t nin);
int huffman_vbbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int huffman_vbbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t huffman_vbsbe21_zd_bound_16(uint32_t nin);
int huffman_vbsbe21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int huffman_vbsbe21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);
uint64_t huffman_vbsse21_zd_bound_16(uint32_t nin);
int huffman_vbsse21_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout);
int huffman_vbsse21_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout);

/* ======================================================================= (2w) the families in the generic calls */

/*
 * Extended method ids.  Every stage_layout_zd method of (2t), (2u) and (2v) has an id that every call taking an `int
 * method` (or src_method / dst_method) accepts beside the ids of enum press_hip_method:
 *   stage    enum press_hip_xstage: the four coders of (2t) with the values of enum press_hip_rcf_coder, then Rice (2u) and
 *            the per-read Huffman code (2v)
 *   layout   enum press_hip_rcf_layout
 *   id       PRESS_HIP_XMETHOD_BASE + 4 * stage + layout, 64 .. 87.  press_hip_xmethod(stage, layout) gives it - for the
 *            three pairs that are public methods (rc_vbe21_zd, rcc_vbe21_zd, rccm_vbbe21_zd) the public id 16 / 17 / 18,
 *            which is the same method; 64, 68 and 73 are accepted as well and mean those three - or -1 for a bad stage or
 *            layout.  press_hip_xmethod_parts is the inverse, for 16 / 17 / 18 too; PRESS_HIP_EARG for any other id.
 *            Both are host arithmetic and need no device.
 * enum press_hip_method and PRESS_HIP_NMETHODS are what they were, every id outside 0 .. 18, 64 .. 87 and 96 .. 98 is
 * PRESS_HIP_EARG (0 from the _workspace_bytes, _fused and _exact questions) as before, and the families' own calls take
 * their own coder / layout ids and nothing else.  The stall methods (2s) have ids of their own, 96 .. 98: (2x).
 *
 * What the calls do with an extended id:
 *   press_hip_bound                  the family's bound (the plain layouts' X_bound_16)
 *   press_hip_press_batch,           out, out_len, sig and out_n byte for byte what the family's own press / depress call
 *   press_hip_depress_batch          gives with its optional table (raw, k, maxlen) NULL.  depress: n[r] is the read's
 *                                    exact sample count, as for the three public range-coder methods
 *   press_hip_press_sizes,           Rice and per-read Huffman: need[r] is the exact length (press_hip_packed_exact = 1),
 *   press_hip_press_packed           the arena has no gaps beyond the alignment, a read is written iff it fits out_cap;
 *                                    the stage's sizes are taken once, the write half goes on from them.  The four coders:
 *                                    need[r] = header + section + nlow + 32 and the gaps of the three public ones
 *                                    (press_hip_packed_exact = 0)
 *   press_hip_recode_*               every pair of the 19 + 21 ids, as source and as destination: byte for byte depress
 *                                    followed by press.  press_hip_recode_fused is 1 for svb12_zd / svb_zd / slow5_svb_zd
 *                                    into any extended id, as into the public exception-split methods
 *   press_hip_recode_degraded_*,     as for the public exception-split methods: a fused source rounds in its decode kernel,
 *   press_hip_verify_degraded_batch  every other pair runs the degrade kernel between the halves
 *   press_hip_depress_pa_batch,      the streams are decoded into library scratch, then the converter, compare and CRC
 *   _norm_batch, _chunks_batch,      kernels of the public methods run: floats, rows, first_bad and CRCs are bit for bit
 *   press_hip_verify_batch,          those of the same reads held in any public method (press_hip_depress_pa_fused = 0)
 *   press_hip_depress_crc_batch
 *   every *_workspace_bytes          the figure of the method's row, by the rules of the public methods
 * A range-coder read whose payload was stored raw (2t) decodes wrongly here as everywhere; press_hip_verify_batch
 * reports it, as it does for the public three.
 */
enum press_hip_xstage {
	PRESS_HIP_XSTAGE_RC      = 0,
	PRESS_HIP_XSTAGE_RCC     = 1,
	PRESS_HIP_XSTAGE_RCCM    = 2,
	PRESS_HIP_XSTAGE_RCCDF   = 3,
	PRESS_HIP_XSTAGE_RICE    = 4,
	PRESS_HIP_XSTAGE_HUFFMAN = 5,
	PRESS_HIP_NXSTAGES       = 6
};
enum { PRESS_HIP_XMETHOD_BASE = 64 };
int press_hip_xmethod(int stage, int layout);
int press_hip_xmethod_parts(int id, int *stage, int *layout);

/* ======================================================================= (2x) the stall methods in the generic calls */

/*
 * The three stall methods of (2s) have a method id that every call taking an `int method` (or src_method / dst_method)
 * accepts beside the ids of enum press_hip_method and the extended ids of (2w):
 *   id       PRESS_HIP_SMETHOD_BASE + stall method: 96 rccm_svbbe21_zd, 97 dstall_fz_1500, 98 dstall_fz.
 *            press_hip_smethod(stall_method) gives it, -1 for a stall method out of range; press_hip_smethod_parts is the
 *            inverse, PRESS_HIP_EARG for every other id or a NULL pointer.  Host arithmetic, no device.
 * 88 .. 95 and everything from 99 on stay PRESS_HIP_EARG before any device call (0 from the _workspace_bytes, _fused and
 * _exact questions), press_hip_xmethod_parts refuses 96 .. 98, and the family's own calls (press_hip_stall_*) keep their
 * ids 0 .. 2 and refuse 96 .. 98.  enum press_hip_method and PRESS_HIP_NMETHODS are what they were.
 *
 * What the calls do with such an id (both device_resident forms; the device-resident form only enqueues on the current
 * stream):
 *   press_hip_bound                  press_hip_stall_bound
 *   press_hip_press_batch            out and out_len byte for byte those of press_hip_stall_press_batch with stall = NULL
 *   press_hip_depress_batch          one decoder reads all three ids; n[r] is the exact sample count; out_n[r] = UINT32_MAX
 *                                    for a stream refused by rule 3 of (2s), whose room is not written
 *   press_hip_press_sizes            need[r] is the EXACT stream length (press_hip_packed_exact = 1), PRESS_HIP_FAILED for
 *                                    a refused read: an empty one, or rule 2 for the two methods that are not dstall_fz.
 *                                    A stall stream's length is known only once its pieces are coded: the call runs the
 *                                    inner range coder, all of a press but the last copy - that is its cost
 *   press_hip_press_packed           the layout rules of (2) unchanged: out_off is written, no gaps beyond align, a read is
 *                                    written iff out_off[r] + need[r] <= out_cap, nothing at or beyond out_cap.  The inner
 *                                    coder runs once per call: the pieces' streams lie in library scratch, their lengths
 *                                    give the layout, and the last kernel copies them to the laid-out offsets
 *   press_hip_recode_*               every pair of the 19 + 24 + 3 ids, as source and as destination, the three among
 *                                    themselves included: byte for byte depress followed by press.  press_hip_recode_fused
 *                                    = 0 in both positions: the pieces are gathered from whole samples
 *   press_hip_recode_degraded_*,     the degrade kernel runs between the halves; the stall is found on the DEGRADED
 *   press_hip_verify_degraded_batch  samples; verify compares with D_bits of the originals, as for every method
 *   press_hip_depress_pa_batch,      the streams are decoded into library scratch, then the converter, compare and CRC
 *   _norm_batch, _chunks_batch,      kernels of the public methods run: floats, rows, first_bad and CRCs are bit for bit
 *   press_hip_verify_batch,          those of the same reads held in any public method (press_hip_depress_pa_fused = 0)
 *   press_hip_depress_crc_batch
 *   every *_workspace_bytes          by the rules of the public methods, exact; press_hip_workspace_bytes(id) is never
 *                                    below press_hip_stall_workspace_bytes(id - 96)
 */
enum { PRESS_HIP_SMETHOD_BASE = 96 };
int press_hip_smethod(int stall_method);
int press_hip_smethod_parts(int id, int *stall_method);

/*
 * (2y) Trimmed chunk rows: a range per read, the scaling statistics over it, the row plan on the device.
 *
 * Range.  press_hip_signal_range_stats' convention: `range` is 2 * nreads uint32 words a, b in samples from the read's
 * start.  With c the read's sample count: b' = min(b, c), a' = min(a, b'), L = b' - a'.  range == NULL is [0, c).  No
 * alignment is asked of off[r] + a.  The SLICED BATCH of a batch and its clamped ranges is the batch whose read r is the
 * L samples [a', b') of read r; every "equals" below means bit for bit against the existing call on the sliced batch.
 *
 * press_hip_signal_quantiles_ranged / press_hip_signal_stats_ranged: q and stats equal press_hip_signal_quantiles /
 * press_hip_signal_stats on the sliced batch - k = min(L - 1, floor(L * num / den)), med and mad at L / 2, 0 and {0, 0}
 * for L == 0.  Checks, forms (host pointers: staged and synchronous; device resident: only enqueued, `range` a device
 * pointer) and launch counts (four and eight) are the unranged calls'.  Loads stay inside the read's room
 * [off[r], off[r] + roundup8(n[r])); what lies outside [a', b') does not take part.
 *
 * press_hip_depress_chunks_trimmed_batch: press_hip_depress_chunks_batch (in / in_off / in_len / off / n / total_samples /
 * out_n / dtype / T / overlap / rule / q mean what they mean there: every method id of the generic calls, the same checks,
 * room rules, PRESS_HIP_ENOTABLE and host wait of the zstd kinds; the WHOLE read is decoded into library scratch) with a
 * range per read.  c = min(out_n[r], n[r]) for a decoded read, 0 for a refused one; out_n reports the full decode.
 *   mode RANGE (and trim == NULL)  the caller's `range`, or the whole read when it is NULL
 *   mode ADAPTOR                   a = the second word (end) of press_hip_signal_adaptor's pair under trim->adaptor over
 *                                  the decoded samples [0, c) where end > 0, else 0 (the pairs (-1, -1), (0, 0)); b = c
 *   mode SEGMENT                   a = the end of the first record press_hip_signal_segments defines for the read under
 *                                  trim->seg with seg_cal as its cal (NULL: the raw domain), 0 without a record; b = c
 * Both detector modes: if b' - a' < min_keep then a' = 0; the two detector calls' parameter checks apply before any device
 * call; reads of 2^31 samples and more are outside their definition.  cut (may be NULL) receives a', b' of every read in
 * every mode, (0, 0) for a refused read.
 *   Scaling: with a rule q = {q_lo, q_hi} over [a', b') and y press_hip_scale_cal's; without one median and MAD over
 * [a', b'); q is {0, 0} for L == 0.
 *   Row plan: row_first (nreads + 1, WRITTEN) is press_hip_chunk_plan over the L[r], computed on the device and always
 * written in full: row_first[nreads] says what the batch needs whatever nrows_cap is; a read with L == 0 takes no row.
 * Row row_first[r] + j holds at column t round_to_dtype(y[a' + start_j + t]), start_j the plan's start for a read of L
 * samples; a column at or beyond L is +0.  row_read[row] = r and row_start[row] = a' + start_j (a position in the read,
 * for stitching a model's output); both may be NULL.  Never written: rows, row_read or row_start entries at or beyond
 * nrows_cap, anything at or beyond row_first[nreads], any byte outside the written prefix.  rows == NULL with
 * nrows_cap == 0 is a pure plan: no row kernel runs.
 *   Equivalence: rows, q and row_first equal what press_hip_chunk_plan and press_hip_depress_chunks_batch give for the
 * sliced batch (pressed by any method that takes it) under the same T, overlap, dtype and rule.
 *   Forms.  Device resident: the call only enqueues on the current stream and never waits; row_first, range, cut,
 * row_read, row_start and seg_cal are device pointers, trim and rule host pointers read before the call returns.  Host
 * pointers: staged, synchronous; the written prefix of rows comes back in one transfer, with the small tables.
 *   Refusals: a bad id, mode, T, overlap, dtype, rule or detector parameter is PRESS_HIP_EARG before any device call, so
 * is a NULL argument other than those named optional.  nreads == 0 is PRESS_HIP_OK and writes row_first[0] = 0.
 * press_hip_depress_chunks_trimmed_workspace_bytes is exact, never below press_hip_depress_chunks_workspace_bytes, and 0
 * for a bad id, T, overlap or mode.
 */
int press_hip_signal_quantiles_ranged(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				      uint64_t total_samples, const uint32_t *range, const uint32_t *rank_num,
				      const uint32_t *rank_den, uint32_t nq, int32_t *q, int device_resident);
int press_hip_signal_stats_ranged(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				  uint64_t total_samples, const uint32_t *range, int32_t *stats, int device_resident);
enum { PRESS_HIP_TRIM_RANGE = 0, PRESS_HIP_TRIM_ADAPTOR = 1, PRESS_HIP_TRIM_SEGMENT = 2 };
typedef struct {
	int32_t mode;
	uint32_t min_keep;             /* detector modes: a cut that leaves fewer samples is not made (a' = 0); 0: off */
	press_hip_jnn2_params adaptor; /* mode ADAPTOR */
	press_hip_jnn_params seg;      /* mode SEGMENT */
} press_hip_trim;
int press_hip_depress_chunks_trimmed_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					   uint32_t nreads, void *rows, uint64_t nrows_cap, int dtype, uint32_t T, uint32_t overlap,
					   uint64_t *row_first /* nreads + 1, WRITTEN */, uint32_t *row_read,
					   uint32_t *row_start /* nrows_cap each, may be NULL */, const uint64_t *off, const uint32_t *n,
					   uint64_t total_samples, const press_hip_trim *trim, const uint32_t *range,
					   const float *seg_cal, uint32_t *cut /* 2 * nreads, may be NULL */,
					   const press_hip_scale_rule *rule, int32_t *q, uint32_t *out_n, int device_resident);
uint64_t press_hip_depress_chunks_trimmed_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads, uint32_t T,
							  uint32_t overlap, int mode);

/* ======================================================================= (2z) BLOW5 records deflated on the device */

/*
 * The write side of a BLOW5 file with record compression zlib (its default): a record is
 *     R = pre | u64 length | signal | post         (press_hip_blow5_write; length = sig_len, or sig_len / 2 samples for
 *                                                   signal method 0)
 * and the file holds, per record, a u64 size and a zlib stream of R.  These calls make the streams on the device; the
 * record is never put together.  A stream need not be what zlib would write, only what it reads: slow5lib, slow5tools and
 * pyslow5 inflate it.  tests/_deflate.py is the serial model of every byte below.
 *
 * The stream of a record of m bytes:  78 01 | one final DEFLATE block (RFC 1951) | Adler-32 of R, big endian (RFC 1950).
 *   Tokens.  A byte that is not zero is a literal.  A maximal run of L zero bytes is the literal 0, then matches at
 * distance 1 over the remaining L - 1 bytes in pieces of min(rest, 258) while rest >= 3, and what is left (0, 1 or 2 bytes)
 * as literal zeros.  Then end-of-block.
 *   Code lengths.  The counts: every literal / length symbol as often as it is a token, end-of-block once.  The symbols
 * with a count stand in a list ascending by (count, symbol); until one node is left the first two nodes become a parent
 * with the sum of their counts, which goes back in front of the first remaining node whose count is not smaller.  A
 * symbol's length is its depth; one symbol alone has length 1.  If a length exceeds 15: the same from max(1, c >> k) for
 * k = 1, 2, ... until none does (the rule of press_hip_table_from_counts).  Codes are the canonical ones of RFC 1951
 * 3.2.2, written first bit first into the stream's bits (bit i of the stream is bit i % 8 of byte i / 8), extra bits
 * lowest bit first.
 *   Block header.  BFINAL 1, BTYPE 2, HLIT = highest symbol with a length - 256 (at least 0), HDIST = 0: one distance
 * code, of length 1, so that a match costs one 0 bit behind its length's extra bits.  The sequence of the HLIT + 257
 * lengths and that 1 is written in runs of equal lengths - zeros: code 18 for min(run, 138) while the run has 11 or more,
 * then code 17 for a rest of 3 .. 10, else the zeros themselves; another length: itself once, then code 16 for
 * min(rest, 6) while the rest has 3 or more, then the rest themselves.  The code over these 19 symbols is built as above
 * with the limit 7; HCLEN drops the trailing symbols without a length of the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2
 * 14 1 15, but keeps four.
 *   Stored.  Where the block's bytes are not fewer than m + 5 * max(1, ceil(m / 65535)), the record is written as stored
 * blocks of 65 535 bytes, the last one shorter and final; raw[r] = 1 says so, 0: the dynamic block.
 *
 * Inputs.  side: an arena with the records' pre and post; side_tab: 4 words per record { pre_off, pre_len, post_off,
 * post_len } into it; sig: the arena of the signal fields (e.g. press_hip_press_packed's out), sig_off / sig_len per
 * record (its out_off / out_len); side_bytes, sig_bytes: the arenas' sizes; record_bytes: the records' bytes together, or
 * more (the device-resident form sizes its launches by it; the host form counts itself).  A record whose part leaves its
 * arena, whose sig_len is PRESS_HIP_FAILED, or that has 0xFFFF0000 bytes or more is REFUSED: need[r] = PRESS_HIP_FAILED,
 * it takes no byte of the image and raw[r] = 0xFF.  With record_bytes too small every record is refused.
 *   press_hip_blow5_deflate_sizes: need[r] = 8 + the stream's exact length, nothing written.
 *   press_hip_blow5_deflate_batch: the file image - per record u64 stream length | stream, back to back in the order given
 * - with rec_off[r] its first byte and rec_off[nrec] the image's size, whatever image_cap is.  A record that ends beyond
 * image_cap is not written and has raw[r] = 0xFF.
 *   Forms.  Device resident: every pointer is device memory; image and image_cap are multiples of 4 and all image_cap
 * bytes are written (zeros where no record lies); the calls only enqueue on the current stream.  Host pointers: staged
 * and synchronous; the image is made at its exact size and min(rec_off[nrec], image_cap) bytes of `image` are written.
 * press_hip_blow5_deflate_workspace_bytes: the scratch of the device-resident form (0: more than a call takes).
 */
int press_hip_blow5_deflate_sizes(const uint8_t *side, const uint64_t *side_tab, uint64_t side_bytes, const uint8_t *sig,
				  const uint64_t *sig_off, const uint64_t *sig_len, uint64_t sig_bytes, uint32_t nrec,
				  uint64_t record_bytes, int signal_method, uint64_t *need, int device_resident);
int press_hip_blow5_deflate_batch(const uint8_t *side, const uint64_t *side_tab, uint64_t side_bytes, const uint8_t *sig,
				  const uint64_t *sig_off, const uint64_t *sig_len, uint64_t sig_bytes, uint32_t nrec,
				  uint64_t record_bytes, int signal_method, uint8_t *image, uint64_t image_cap,
				  uint64_t *rec_off /* nrec + 1, WRITTEN */, uint8_t *raw /* nrec */, int device_resident);
uint64_t press_hip_blow5_deflate_workspace_bytes(uint64_t record_bytes, uint32_t nrec);

/* ======================================================================= (2zb) BLOW5 records inflated on the device */

/*
 * The read side of a BLOW5 file with record compression zlib: the file holds, per record, a u64 size and a zlib stream
 * (press_hip_blow5_next_stored hands them out as they are stored), and these calls inflate the streams on the device, one
 * wave per record.  The decoder reads EVERY zlib stream that zlib's uncompress reads (RFC 1950 around RFC 1951), not only
 * the streams of section 2z:
 *   the header CMF FLG with CM = 8, CINFO <= 7, the FCHECK rule and FDICT = 0; any number of blocks in any order - stored,
 * fixed Huffman, dynamic Huffman - among them the empty stored blocks of a sync or full flush and an empty final block;
 * code lengths 1 .. 15; the repeat codes 16 / 17 / 18, also across the boundary between the literal / length and the
 * distance lengths; up to 286 literal / length and 30 distance codes; a set of codes that is complete or - as zlib allows
 * it - has one code of one bit (the one distance code of 2z; a literal / length set that is end-of-block alone), and no
 * distance code at all; lengths 3 .. 258, 258 also as symbol 284 with extra bits 31; distances 1 .. 32768 whatever CINFO
 * says; a match that overlaps itself; the Adler-32, checked on the device; bytes behind the Adler-32 are ignored.
 *
 * status[r]: PRESS_HIP_INFLATE_OK, or the FIRST failure met in stream order -
 *   HEADER     CM, CINFO, FCHECK or FDICT
 *   TRUNCATED  the stream needs a bit beyond comp_len (a Huffman code counts bit by bit: one that ends behind the end)
 *   BTYPE      block type 3
 *   STORED     LEN is not the complement of NLEN
 *   CODES      more than 286 / 30 codes; a repeat with nothing before it or past the end; an over-subscribed set; an
 *              incomplete set other than the single code of one bit (the code-length code must be complete); no
 *              end-of-block code
 *   SYMBOL     literal / length 286 or 287, distance 30 or 31, 15 bits that are no code of an incomplete set
 *   DISTANCE   a match reaches in front of the record's first byte (found before a byte of it is copied)
 *   ADLER      the Adler-32 of the bytes is not the stored one
 *   ROOM       well formed to its end, but longer than its slot (the packed form: it ends behind out_cap)
 *   REFUSED    comp_off[r] + comp_len[r] leaves comp_bytes, or comp_len[r] is 4 GiB or more
 * tests/_inflate.py is the serial model of this classification; honours_amd/csrc/press_inflate_walk.h holds the rules as
 * plain C++ for the host and the device (ph::inflate_serial: one stream on one host thread).
 *
 *   press_hip_blow5_inflate_batch: the caller's slots, as press_hip_press_batch's - record r into out[out_off[r] ..
 * out_off[r + 1]), any byte offset.  Nothing outside a slot is written and a failed record leaves its neighbours alone.
 * out_len[r] is the record's exact inflated length whenever the stream is well formed to its end: OK, and ROOM - there the
 * walk goes on as a count without writing, and the Adler-32 is not judged.  Otherwise out_len[r] = PRESS_HIP_FAILED.  Of
 * a failed record's slot any byte may have been written.  One walk per record.
 *   press_hip_blow5_inflate_sizes: the counting walk alone - need[r] as out_len[r] above with slots of any size, status[r]
 * OK for a stream that is well formed to its end.  No arena, and NO Adler-32 check: the bytes are never made.
 *   press_hip_blow5_inflate_packed: the sizes walk, the layout (rules and align as press_hip_press_packed: out_off WRITTEN,
 * nrec + 1, whatever out_cap is), then the writing walk.  A failed record takes no byte and has out_len[r] =
 * PRESS_HIP_FAILED, one that ends behind out_cap too, with status ROOM.  One failure is found only by the writing walk:
 * a stream that is well formed to its end but whose Adler-32 is wrong keeps its room in the layout (the sizes walk makes
 * no bytes), its bytes are written there, and it has status ADLER and out_len[r] = PRESS_HIP_FAILED.  A device `out` must
 * be a multiple of 4 bytes.
 *   press_hip_blow5_record_fields: parse_record's rules (the host reader's) over inflated records, one lane per record:
 * sig_off[r] (from the arena's first byte) and sig_len[r] are what the depress / recode / pa / chunk calls take as in_off
 * / in_len, n_samples[r] the read's samples (signal method 1: the svb-zd stream's count), dor[3r ..] digitisation, offset
 * and range (may be NULL), read_ids (may be NULL) nrec x PRESS_HIP_BLOW5_ID_LEN chars, NUL padded.  A record that
 * parse_record refuses, or whose rec_len is PRESS_HIP_FAILED, gets sig_len = PRESS_HIP_FAILED and n_samples = 0.
 *   Forms.  Device resident: every pointer is device memory; the calls only enqueue on the current stream and depend on
 * nothing an earlier call left in scratch.  Host pointers: staged and synchronous; out_off must not descend.  Arguments are
 * checked before the device is asked for (NULL, align, a device `out` of the packed form); nrec == 0 is PRESS_HIP_OK.
 * press_hip_blow5_inflate_workspace_bytes: the scratch of the device-resident forms.
 */
#define PRESS_HIP_INFLATE_OK        0
#define PRESS_HIP_INFLATE_HEADER    1
#define PRESS_HIP_INFLATE_TRUNCATED 2
#define PRESS_HIP_INFLATE_BTYPE     3
#define PRESS_HIP_INFLATE_STORED    4
#define PRESS_HIP_INFLATE_CODES     5
#define PRESS_HIP_INFLATE_SYMBOL    6
#define PRESS_HIP_INFLATE_DISTANCE  7
#define PRESS_HIP_INFLATE_ADLER     8
#define PRESS_HIP_INFLATE_ROOM      9
#define PRESS_HIP_INFLATE_REFUSED   10
#define PRESS_HIP_INFLATE_DRAIN     4096 /* bytes a wave produces between two writes of its LDS window to the slot */
int press_hip_blow5_inflate_batch(const uint8_t *comp, const uint64_t *comp_off, const uint64_t *comp_len, uint64_t comp_bytes,
				  uint32_t nrec, uint8_t *out, const uint64_t *out_off /* nrec + 1 */, uint64_t *out_len,
				  uint8_t *status, int device_resident);
int press_hip_blow5_inflate_sizes(const uint8_t *comp, const uint64_t *comp_off, const uint64_t *comp_len, uint64_t comp_bytes,
				  uint32_t nrec, uint64_t *need, uint8_t *status, int device_resident);
int press_hip_blow5_inflate_packed(const uint8_t *comp, const uint64_t *comp_off, const uint64_t *comp_len, uint64_t comp_bytes,
				   uint32_t nrec, uint8_t *out, uint64_t out_cap, uint32_t align, uint64_t *out_off /* WRITTEN */,
				   uint64_t *out_len, uint8_t *status, int device_resident);
int press_hip_blow5_record_fields(const uint8_t *rec, const uint64_t *rec_off, const uint64_t *rec_len, uint64_t rec_bytes,
				  uint32_t nrec, int signal_method, uint64_t *sig_off, uint64_t *sig_len, uint32_t *n_samples,
				  double *dor /* may be NULL */, char *read_ids /* may be NULL */, int device_resident);
uint64_t press_hip_blow5_inflate_workspace_bytes(uint64_t comp_bytes, uint32_t nrec);

/* ======================================================================= (3) BLOW5 files (host) */

/*
 * Reader for BLOW5 files that hands out the signal fields AS STORED: what the
 * reference's loader decodes on the CPU (slow5_open slow5.h:345, slow5_get_next :446,
 * slow5_rec.raw_signal :274) goes to the device compressed and is decoded there with
 * press_hip_depress_batch(PRESS_HIP_SLOW5_SVB_ZD, ...).  Record compression none / zlib / zstd,
 * signal compression none / svb-zd.  Host code, usable without a GPU.
 */
typedef struct press_hip_blow5 press_hip_blow5;
#define PRESS_HIP_BLOW5_ID_LEN 64 /* bytes per read id handed out (NUL padded) */
int press_hip_blow5_open(const char *path, press_hip_blow5 **out);
void press_hip_blow5_close(press_hip_blow5 *f);
/* record method: 0 none, 1 zlib, 2 zstd; signal method: 0 none (int16 samples), 1 svb-zd */
int press_hip_blow5_methods(const press_hip_blow5 *f, int *record_method, int *signal_method);
/* Next batch: up to max_reads signal fields copied back to back into arena (each starts on a
 * 16-byte boundary), sig_off / sig_len in bytes, n_samples per read, read_ids (may be NULL)
 * max_reads x PRESS_HIP_BLOW5_ID_LEN chars.  *got = reads delivered; 0 at the end of the file. */
int press_hip_blow5_next(press_hip_blow5 *f, uint32_t max_reads, uint8_t *arena, uint64_t arena_cap,
			 uint64_t *sig_off, uint64_t *sig_len, uint32_t *n_samples, char *read_ids, uint32_t *got);
/* ... and the calibration of every read: dor[3k ..] = digitisation, offset, range as record k stores them
 * (three doubles; press_hip_pa_cal turns them into press_hip_depress_pa_batch's cal) */
int press_hip_blow5_next_pa(press_hip_blow5 *f, uint32_t max_reads, uint8_t *arena, uint64_t arena_cap,
			    uint64_t *sig_off, uint64_t *sig_len, uint32_t *n_samples, char *read_ids, double *dor,
			    uint32_t *got);
const char *press_hip_blow5_last_error(void);
/* Whole inflated records (for a transcoder): sig_pos / sig_len locate the signal field in
 * record k, the u64 length field sits 8 bytes in front of it. */
int press_hip_blow5_next_records(press_hip_blow5 *f, uint32_t max_reads, uint8_t *arena, uint64_t arena_cap,
				 uint64_t *rec_off, uint64_t *rec_len, uint64_t *sig_pos, uint64_t *sig_len,
				 uint32_t *n_samples, uint32_t *got);
/* Records AS THE FILE STORES THEM, with no inflate (for press_hip_blow5_inflate_batch, 2zb): up to max_reads records
 * copied into arena, each on a 16-byte boundary; comp_off / comp_len in bytes (the u64 size in front of a record is not
 * copied).  File order and the end marker as the calls above; a record that does not fit arena_cap opens the next batch.
 * Records the calls above have read ahead and inflated are not handed out again: use one kind of call per handle. */
int press_hip_blow5_next_stored(press_hip_blow5 *f, uint32_t max_reads, uint8_t *arena, uint64_t arena_cap,
				uint64_t *comp_off, uint64_t *comp_len, uint32_t *got);
/* Writer (slow5_write / slow5_rec_to_mem, slow5.c:3903-4010): header copied from `like`; records
 * framed and - record_method 1 - deflated; signal_method says what `sig` holds (0: int16 samples,
 * 1: svb-zd, e.g. the output of press_hip_press_batch(PRESS_HIP_SLOW5_SVB_ZD, ...)). */
typedef struct press_hip_blow5_writer press_hip_blow5_writer;
int press_hip_blow5_create(const char *path, const press_hip_blow5 *like, int record_method, int signal_method,
			   press_hip_blow5_writer **out);
int press_hip_blow5_write(press_hip_blow5_writer *w, const uint8_t *pre, uint64_t pre_len, const uint8_t *sig,
			  uint64_t sig_len, const uint8_t *post, uint64_t post_len);
/* n records at once: framed and deflated by a pool of host threads, written in the order given */
int press_hip_blow5_write_batch(press_hip_blow5_writer *w, uint32_t n, const uint8_t *const *pre, const uint64_t *pre_len,
				const uint8_t *const *sig, const uint64_t *sig_len, const uint8_t *const *post,
				const uint64_t *post_len);
/* enable != 0: keep slow5lib's index (read id -> record offset and size, slow5_idx.c:269 slow5_idx_write) while
 * writing; press_hip_blow5_finish leaves it as <path>.idx, so that the reference's slow5_idx_load / slow5_get
 * (slow5.h:375, 423) find the reads of the file without building the index themselves */
int press_hip_blow5_index(press_hip_blow5_writer *w, int enable);
/* host threads that inflate records (reader; 0 = as many as the host offers, at most 32) */
int press_hip_blow5_threads(press_hip_blow5 *f, int threads);
/* n records that are deflated already: the image of press_hip_blow5_deflate_batch (2z) - `bytes` = rec_off[n], every
 * record written - goes to the file in one piece, with the index entries press_hip_blow5_write would add (pre[r]: the
 * record's front part, which holds its read id).  Refused with PRESS_HIP_EARG, and nothing written: a writer whose record
 * method is not zlib, rec_off that does not ascend from 0 to `bytes`, a record whose u64 length is not its extent. */
int press_hip_blow5_write_image(press_hip_blow5_writer *w, const uint8_t *image, uint64_t bytes, uint32_t n,
				const uint64_t *rec_off, const uint8_t *const *pre, const uint64_t *pre_len);
int press_hip_blow5_finish(press_hip_blow5_writer *w); /* end marker, the index if asked for, close, free */

#ifdef __cplusplus
}
#endif
#endif /* PRESS_HIP_H */
