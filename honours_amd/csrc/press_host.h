// press_host.h - shared between the host-side units of libpress_hip.so (press_ctx, press_methods, press_staging,
// press_batch, press_table, press_dropin .hip).  Host only: the kernel files include press_internal.h alone.
#pragma once

#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <mutex>
#include <vector>

#include "../../include/press_hip.h"
#include "press_internal.h"

namespace ph {

// ------------------------------------------------------------------ errors (press_ctx.hip)

#define HIPCHK(call)                                                                             \
	do {                                                                                     \
		hipError_t e_ = (call);                                                          \
		if (e_ != hipSuccess)                                                            \
			return set_error(PRESS_HIP_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
	} while (0)

// ------------------------------------------------------------------ context (press_ctx.hip)

struct DevBuf;
extern DevBuf *g_bufs; // every DevBuf links itself in here: press_hip_shutdown() cannot forget one

struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	DevBuf *next;
	DevBuf() : next(g_bufs) { g_bufs = this; }
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	// grow-only; contents are not preserved
	int reserve(size_t n)
	{
		if (n <= cap)
			return 0;
		release();
		size_t want = n + n / 8 + 4096;
		hipError_t e = hipMalloc(&p, want);
		if (e != hipSuccess)
			return set_error(PRESS_HIP_EHIP, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
		cap = want;
		return 0;
	}
	void release()
	{
		if (p)
			(void) hipFree(p);
		p = nullptr;
		cap = 0;
	}
};

struct Ctx {
	bool ready = false;
	int device = -1;
	hipStream_t own = nullptr;
	hipStream_t user = nullptr;
	bool use_user = false;
	// scratch shared by both modes
	DevBuf meta, ex_pos, ex_val, low, huff, chunks, gran, ctl, first_chunk, htiles, hunit, hrec, hlist, hread, hwave, hbits, hend, hmin, cbits;
	DevBuf ztmp, zoff, zoff4, zlen, zhist, ztab, zfirst, zblk, zsbits, zbpos, zbflag, zkcnt, zrd, znb, zn, zdcopy, zdhuf, zdunit, zdtree, zdlong, zdctl, zdseq, zdxblk; // zstd frames
	DevBuf rsig, rn, rkeep, pchunks, pfirst, pctl; // recode: samples nobody asked for, the press half's counts, refused reads' slot heads, its chunk table
	DevBuf pneed, pslot; // packed press: the reads' sizes, the slot table its writing kernels see (PackArgs)
	DevBuf pa_tile, pa_ctl, pa_cal, pa_out; // picoamperes: the converter's tile table and its count; host path: the staged calibration, the float arena
	DevBuf st_rows, st_read, st_cal, st_stats; // median / MAD: the reads' count rows, the pick state, the normaliser's two floats; host path: stats
	DevBuf ch_rows, ch_first; // chunk rows, host path: the row arena, the staged row_first
	DevBuf tr_cut, tr_cnt, tr_det, tr_first, tr_read, tr_start, tr_user; // trimmed chunk rows: the cuts, the detectors' sample counts and results; host path: row_first, row_read, row_start, the caller's cut
	DevBuf vf_raw, vf_out; // verify / CRC-32: a word per read between the two kernels; host path: the staged crc or first_bad, and nbad
	DevBuf ev_state, ev_cal, ev_first, ev_cnt, ev_out; // events: count and path per read; host path: the staged calibration, ev_first, ev_count, the records
	DevBuf sg_state, sg_cal, sg_first, sg_cnt, sg_thr, sg_out; // jnn segments: count and thresholds per read; host path: the staged calibration, seg_first, seg_count, thr, the records (the adaptor: the pairs)
	DevBuf px_pair, px_range, px_out, px_stat; // range statistics and prefix: the adaptor's pairs, the ranges (host path: the caller's); host path: the prefix records, the statistics (the calibration and thr: sg_cal, sg_thr)
	DevBuf sl_seg, sl_rd, sl_poff, sl_pn, sl_pooff, sl_polen, sl_poutn, sl_psig, sl_parena, sl_stall; // stall methods: first segments, plans, the piece table (StallBufs), the pieces' samples and streams; host path: (start, len) per read
	DevBuf ri_sum, ri_start, ri_rd, ri_pay, ri_drd, ri_tile, ri_rec, ri_tbase, ri_ctl, ri_k; // Rice methods: the units' sums and first bits, the reads' records, the staged payloads; depress: reads, tiles, subsequence records, tile bases, counters; host path: k[]
	DevBuf dh_tab; // per-read Huffman methods: codes and counts (press), decode tables (depress); the other buffers are the Rice methods'
	DevBuf tl_chunks, tl_ctl, tl_tab, tl_mom; // dataset tallies: the chunk list and its count; host path: the three tables in a row, the moments
	DevBuf df_rec, df_unit, df_tab, df_need, df_side, df_sig, df_tabs, df_img, df_out; // BLOW5 record deflate (press_deflate.hip): the records, the units' tables, counts / codes / block headers, the sizes; host path: the side arena, the signal arena, the three tables, the image, rec_off and raw
	DevBuf if_need, if_slot, if_comp, if_tabs, if_out, if_res; // BLOW5 record inflate (press_inflate.hip): the packed form's sizes and slot table; host path: the streams, their tables (and the slots), the arena, out_len and status
	// staging for host-pointer calls
	DevBuf sig, off, nsamp, arena, arena_off, lens, lens2, outn, dense, dense_off;
	DevBuf rin, rin_off; // ... of recode: the source streams
	uint32_t zs_nhost = 0; // frames the last zstd depress batch left to libzstd
	uint32_t *zs_pin = nullptr; // page-locked: that count comes back while the device goes on with the batch
	hipEvent_t zs_ev = nullptr;
	// static Huffman table currently on the device
	bool have_table = false;
	bool table_trie = false; // some code of the table is beyond the second-level tables (HUF_NEEDS_TRIE)
	uint32_t tlen[256];
	uint64_t tbits[256];
	uint32_t tmin = 64, tmax = 1; // its shortest / longest code

	hipStream_t stream() const { return use_user ? user : own; }
};

extern Ctx g;
// One context per process (one process per GPU): calls from several host threads are serialised.
extern std::recursive_mutex g_mu;
#define API_LOCK std::lock_guard<std::recursive_mutex> api_lock_(ph::g_mu)

// Every entry point that touches the device comes through here: HIP's current device is per
// host thread, so it is selected again on every call (cheap), not only by the first caller.
int ctx_init();
#define API_ENTER API_LOCK; if (int rc_ = ph::ctx_init()) return rc_ // head of an entry point that needs the device

// ------------------------------------------------------------------ caller I/O and its staging (press_staging.hip)

// The three kinds of caller I/O of a batch call.  An entry point launches on the caller's own pointers (device
// resident) or on what a Staged call returns for them: the same structs, filled by different plumbing.
struct SamplesIn {
	const int16_t *sig;
	const uint64_t *off;
	const uint32_t *n;
};
struct StreamsIn { // streams in and the rooms of what they decode to
	const uint8_t *in;
	const uint64_t *in_off, *in_len, *off;
	const uint32_t *n;
	uint32_t *out_n;
	int16_t *sig; // the samples' room; NULL where the call has none
};
struct SlotsOut {
	uint8_t *out;
	const uint64_t *out_off;
	uint64_t *out_len;
};

// The layout checks of the host-pointer form (they read the caller's tables): EARG with the text in last_error
int check_disjoint(const uint64_t *off, const uint32_t *n, uint32_t nreads, const char *what, std::vector<uint32_t> &order);
int check_layout(const uint64_t *off, const uint32_t *n, uint32_t nreads, uint64_t total_samples); // off[] multiples of 8, reads inside total_samples
int check_slots(const uint64_t *out_off, uint32_t nreads);                                        // out_off non-decreasing

// One host-pointer call: what it moves to the device before the launch and back behind it, through the context's
// staging DevBufs.  The tables its queued copies read are members: they live until the call's last synchronisation.
struct Staged {
	const uint32_t nreads;
	const hipStream_t s;
	Staged(uint32_t nreads_, hipStream_t s_) : nreads(nreads_), s(s_) {}
	// off and n checked and copied, room for the samples (with_sig); what: the ranges must be disjoint, it names them
	// in the refusal (NULL: reads may overlap)
	int layout(const uint64_t *off, const uint32_t *n, uint64_t total_samples, const char *what, bool with_sig);
	int samples(const SamplesIn &h, uint64_t total_samples, SamplesIn &d); // behind layout(): the samples -> d
	// the two in one, for reads that must not overlap ("the sample range"): the head of a call over samples that are there
	int samples_in(const SamplesIn &h, uint64_t total_samples, SamplesIn &d);
	int slots(const SlotsOut &h, SlotsOut &d);                              // an arena for the slots (checked: check_slots) -> d
	// layout() of the rooms, then the streams dense in `arena`, their table in `offs` -> d; d.sig: g.sig with sig_room,
	// else h.sig as it is
	int streams(const StreamsIn &h, uint64_t total_samples, bool sig_room, DevBuf &arena, DevBuf &offs, StreamsIn &d);
	int push(void *dev, const void *src, size_t bytes); // plain bytes up; returns when src may be reused, unless it is page-locked
	// the tails; all but fetch_prefix end with the stream synchronised
	struct Table { // a per-read result table on its way back; dst NULL: the caller did not ask for it
		void *dst;
		const void *dev;
		size_t bytes;
	};
	int fetch_tables(std::initializer_list<Table> tables);                     // each table in turn
	int fetch_streams(const SlotsOut &h);                                      // out_len, the streams of slots()' arena
	int fetch_elems(void *dst, const void *dev, size_t es, const StreamsIn &h); // out_n, the decoded elements of `dev`
	int fetch_samples(const StreamsIn &h);                                     // ... the samples of g.sig into h.sig
	int fetch_prefix(void *dst, void *dev, uint64_t bytes);                    // a dense arena's first bytes
private:
	std::vector<uint32_t> order;    // the reads in ascending sample offset (check_disjoint)
	std::vector<uint64_t> doff, rel; // dense offsets of the streams; the slots relative to the first
};
void staging_release(); // the page-locked staging buffers
void staging_fill(int byte); // ... set to one byte value (press_hip_scratch_fill); the stream must be idle

// ---- zstd, loaded lazily (third party; the reference links -lzstd, press/Makefile:3) ----
struct Zstd {
	bool tried = false;
	size_t (*compress)(void *, size_t, const void *, size_t, int) = nullptr;
	size_t (*decompress)(void *, size_t, const void *, size_t) = nullptr;
	size_t (*bound)(size_t) = nullptr;
	unsigned (*is_error)(size_t) = nullptr;
};
extern Zstd zstd_fn;
bool zstd_open();
uint64_t zstd_bound_(uint64_t n);

// ------------------------------------------------------------------ methods (dispatch and bounds: press_methods.hip)

enum Family : uint8_t { FAM_SVB, FAM_EX, FAM_ZSTD, FAM_STALL };
struct Method {
	int id;
	Family family;
	bool key2, zd, slow5; // FAM_SVB: 2-bit keys (svb32), zig-zag delta, BLOW5's framing
	ExFmt exfmt;          // FAM_EX: the section's layout ...
	ExEnt ent;            // ... and the entropy stage, a row of EX_STAGES
	int inner;            // FAM_ZSTD: the method whose streams the frames hold ...
	uint32_t kdiv;        // ... and its samples per key byte (ZsBufs::kdiv)
	int stall;            // FAM_STALL: the stall method (press_hip_stall_method); `inner` presses and depresses its pieces
};
#define M_SVB(id, key2, zd, slow5) { id, FAM_SVB, key2, zd, slow5, EXF_VBE21, ENT_PLAIN, 0, 0, 0 }
#define M_EX(id, fmt, ent) { id, FAM_EX, false, false, false, fmt, ent, 0, 0, 0 }
#define M_ZSTD(id, inner, kdiv) { id, FAM_ZSTD, false, false, false, EXF_VBE21, ENT_PLAIN, inner, kdiv, 0 }
constexpr Method METHODS[] = {
	M_SVB(PRESS_HIP_SVB12, false, false, false),
	M_SVB(PRESS_HIP_SVB12_ZD, false, true, false),
	M_SVB(PRESS_HIP_SVB_ZD, true, true, false),
	M_ZSTD(PRESS_HIP_ZSTD_SVB_ZD, PRESS_HIP_SVB_ZD, 4),
	M_ZSTD(PRESS_HIP_ZSTD_SVB12_ZD, PRESS_HIP_SVB12_ZD, 8),
	M_EX(PRESS_HIP_VBE21_ZD, EXF_VBE21, ENT_PLAIN),
	M_EX(PRESS_HIP_VBBE21_ZD, EXF_VBBE21, ENT_PLAIN),
	M_EX(PRESS_HIP_VBSBE21_ZD, EXF_VBSBE21, ENT_PLAIN),
	M_EX(PRESS_HIP_VBSSE21_ZD, EXF_VBSSE21, ENT_PLAIN),
	M_EX(PRESS_HIP_SHUFF_VBE21_ZD, EXF_VBE21, ENT_SHUFF),
	M_EX(PRESS_HIP_SHUFF_VBBE21_ZD, EXF_VBBE21, ENT_SHUFF),
	M_EX(PRESS_HIP_SHUFF_VBSBE21_ZD, EXF_VBSBE21, ENT_SHUFF),
	M_EX(PRESS_HIP_SHUFF_VBSSE21_ZD, EXF_VBSSE21, ENT_SHUFF),
	M_EX(PRESS_HIP_HASGAM_ZDQ, EXF_EXZD, ENT_PLAIN),
	M_ZSTD(PRESS_HIP_ZSTD_HASGAM_ZDQ, PRESS_HIP_HASGAM_ZDQ, 0),
	M_SVB(PRESS_HIP_SLOW5_SVB_ZD, true, true, true),
	M_EX(PRESS_HIP_RC_VBE21_ZD, EXF_VBE21, ENT_RC),
	M_EX(PRESS_HIP_RCC_VBE21_ZD, EXF_VBE21, ENT_RCC),
	M_EX(PRESS_HIP_RCCM_VBBE21_ZD, EXF_VBBE21, ENT_RCM),
};
constexpr bool methods_in_order()
{
	for (int i = 0; i < PRESS_HIP_NMETHODS; i++)
		if (METHODS[i].id != i || (METHODS[i].family == FAM_ZSTD && METHODS[METHODS[i].inner].family == FAM_ZSTD))
			return false;
	return true;
}
static_assert(sizeof METHODS / sizeof METHODS[0] == PRESS_HIP_NMETHODS, "one row per method id");
static_assert(methods_in_order(), "METHODS[i].id == i, and a zstd composition wraps a plain method");
inline bool public_ok(int m) { return m >= 0 && m < PRESS_HIP_NMETHODS; }
inline bool is_shuff(const Method &m) { return m.family == FAM_EX && m.ent == ENT_SHUFF; }
// questions to the method's row of EX_STAGES: a stage codes the one-byte values out of a temporary (Ctx::low); the size the
// packed press announces is a bound, not the stream's length
inline bool uses_low_tmp(const Method &m) { return m.family == FAM_EX && EX_STAGES[m.ent].low_tmp; }
inline bool packed_is_bound(const Method &m) { return m.family == FAM_EX && EX_STAGES[m.ent].pay == PAY_CODER; }

// ---- the range-coder family (press_hip_rcf_*): every coder on every layout.  Rows of its own behind the public ids,
// where public_ok does not reach them; the three pairs that are public methods go through the public rows.
constexpr int RCF_PRIVATE = PRESS_HIP_NMETHODS; // private id = RCF_PRIVATE + 4 * coder + layout
#define M_RCF(coder, ent)                                                                                    \
	M_EX(RCF_PRIVATE + 4 * coder + 0, EXF_VBE21, ent), M_EX(RCF_PRIVATE + 4 * coder + 1, EXF_VBBE21, ent), \
		M_EX(RCF_PRIVATE + 4 * coder + 2, EXF_VBSBE21, ent), M_EX(RCF_PRIVATE + 4 * coder + 3, EXF_VBSSE21, ent)
constexpr Method RCF_METHODS[PRESS_HIP_NRCF_CODERS * PRESS_HIP_NRCF_LAYOUTS] = {
	M_RCF(PRESS_HIP_RCF_RC, ENT_RC), M_RCF(PRESS_HIP_RCF_RCC, ENT_RCC), M_RCF(PRESS_HIP_RCF_RCCM, ENT_RCM), M_RCF(PRESS_HIP_RCF_RCCDF, ENT_CDF),
};
static_assert((int) EXF_VBE21 == (int) PRESS_HIP_RCF_VBE21 && (int) EXF_VBBE21 == (int) PRESS_HIP_RCF_VBBE21 &&
		      (int) EXF_VBSBE21 == (int) PRESS_HIP_RCF_VBSBE21 && (int) EXF_VBSSE21 == (int) PRESS_HIP_RCF_VBSSE21,
	      "the family's layout ids are the exception formats");
inline bool rcf_ok(int coder, int layout)
{
	return coder >= 0 && coder < PRESS_HIP_NRCF_CODERS && layout >= 0 && layout < PRESS_HIP_NRCF_LAYOUTS;
}
inline const Method &rcf_method(int coder, int layout)
{
	const Method &m = RCF_METHODS[4 * coder + layout];
	for (const Method &pub : METHODS)
		if (pub.family == FAM_EX && pub.exfmt == m.exfmt && pub.ent == m.ent)
			return pub;
	return m;
}

// ---- the Rice family (press_hip_rice_*): Golomb-Rice coding of the one-byte values on every layout; rows of its own again
constexpr int RICE_PRIVATE = RCF_PRIVATE + PRESS_HIP_NRCF_CODERS * PRESS_HIP_NRCF_LAYOUTS; // private id = RICE_PRIVATE + layout
constexpr Method RICE_METHODS[PRESS_HIP_NRCF_LAYOUTS] = {
	M_EX(RICE_PRIVATE + 0, EXF_VBE21, ENT_RICE), M_EX(RICE_PRIVATE + 1, EXF_VBBE21, ENT_RICE), M_EX(RICE_PRIVATE + 2, EXF_VBSBE21, ENT_RICE),
	M_EX(RICE_PRIVATE + 3, EXF_VBSSE21, ENT_RICE),
};
inline bool is_rice(const Method &m) { return m.family == FAM_EX && m.ent == ENT_RICE; }
inline bool rice_ok(int layout) { return layout >= 0 && layout < PRESS_HIP_NRCF_LAYOUTS; }

// ---- the per-read Huffman family (press_hip_huffman_*): a Huffman code from each read's own one-byte values, on every layout
constexpr int DHUF_PRIVATE = RICE_PRIVATE + PRESS_HIP_NRCF_LAYOUTS; // private id = DHUF_PRIVATE + layout
constexpr Method DHUF_METHODS[PRESS_HIP_NRCF_LAYOUTS] = {
	M_EX(DHUF_PRIVATE + 0, EXF_VBE21, ENT_DHUF), M_EX(DHUF_PRIVATE + 1, EXF_VBBE21, ENT_DHUF), M_EX(DHUF_PRIVATE + 2, EXF_VBSBE21, ENT_DHUF),
	M_EX(DHUF_PRIVATE + 3, EXF_VBSSE21, ENT_DHUF),
};
inline bool is_dhuf(const Method &m) { return m.family == FAM_EX && m.ent == ENT_DHUF; }

// ---- the ids the generic calls take (include/press_hip.h 2w): the public ids, and PRESS_HIP_XMETHOD_BASE + 4 * stage + layout
// for every row of the three families.  method_row resolves an id once; the calls go on with the row.
static_assert((int) PRESS_HIP_XSTAGE_RC == (int) PRESS_HIP_RCF_RC && (int) PRESS_HIP_XSTAGE_RCC == (int) PRESS_HIP_RCF_RCC &&
		      (int) PRESS_HIP_XSTAGE_RCCM == (int) PRESS_HIP_RCF_RCCM && (int) PRESS_HIP_XSTAGE_RCCDF == (int) PRESS_HIP_RCF_RCCDF &&
		      (int) PRESS_HIP_XSTAGE_RICE == (int) PRESS_HIP_NRCF_CODERS && (int) PRESS_HIP_XSTAGE_HUFFMAN == (int) PRESS_HIP_NRCF_CODERS + 1,
	      "the first four extended stages are the family's coders");
static_assert(PRESS_HIP_XMETHOD_BASE >= DHUF_PRIVATE + PRESS_HIP_NRCF_LAYOUTS, "the extended ids lie behind the private ones");
inline bool xmethod_ok(int m) { return m >= PRESS_HIP_XMETHOD_BASE && m < PRESS_HIP_XMETHOD_BASE + PRESS_HIP_NXSTAGES * PRESS_HIP_NRCF_LAYOUTS; }
// ---- the stall methods (press_hip_stall_*, include/press_hip.h 2x): PRESS_HIP_SMETHOD_BASE + the stall method.  Rows of a
// family of its own: the read's pieces go through `inner`'s kernels as the reads of a larger batch (press_stall.hip)
#define M_STALL(sm) { PRESS_HIP_SMETHOD_BASE + sm, FAM_STALL, false, false, false, EXF_VBBE21, ENT_RCM, PRESS_HIP_RCCM_VBBE21_ZD, 0, sm }
constexpr Method STALL_METHODS[PRESS_HIP_NSTALL] = {
	M_STALL(PRESS_HIP_STALL_RCCM_SVBBE21_ZD), M_STALL(PRESS_HIP_STALL_DSTALL_FZ_1500), M_STALL(PRESS_HIP_STALL_DSTALL_FZ),
};
static_assert(PRESS_HIP_SMETHOD_BASE >= PRESS_HIP_XMETHOD_BASE + PRESS_HIP_NXSTAGES * PRESS_HIP_NRCF_LAYOUTS + 8, "ids 88 .. 95 stay unused");
inline bool smethod_ok(int m) { return m >= PRESS_HIP_SMETHOD_BASE && m < PRESS_HIP_SMETHOD_BASE + PRESS_HIP_NSTALL; }
inline bool method_ok(int m) { return public_ok(m) || xmethod_ok(m) || smethod_ok(m); }
inline const Method &xstage_row(int stage, int layout) // stage and layout in range
{
	return stage < PRESS_HIP_NRCF_CODERS ? rcf_method(stage, layout) : stage == PRESS_HIP_XSTAGE_RICE ? RICE_METHODS[layout] : DHUF_METHODS[layout];
}
inline const Method &method_row(int m) // method_ok(m)
{
	if (smethod_ok(m))
		return STALL_METHODS[m - PRESS_HIP_SMETHOD_BASE];
	return public_ok(m) ? METHODS[m] : xstage_row((m - PRESS_HIP_XMETHOD_BASE) / 4, (m - PRESS_HIP_XMETHOD_BASE) % 4);
}

// ---- bounds: the reference's formulas ----
inline uint32_t svb16_keylen(uint32_t n) { return (n >> 3) + (((n & 7) + 7) >> 3); }
inline uint64_t bound_svb32(uint32_t n) { return (uint64_t) (n + 3) / 4 + (uint64_t) n * 4 + 16; }    // streamvbyte.h:35
inline uint64_t bound_svb16(uint32_t n) { return (uint64_t) svb16_keylen(n) + (uint64_t) n * 4 + 16; } // streamvbyte.h:42
inline uint64_t bound_vb1e2(uint32_t m) { return (uint64_t) (1 + m * 0.2 * 6 + m * 0.8); }            // press.c:2575
inline uint64_t bound_vbzd(uint32_t n) { return 2 + bound_vb1e2(n - 1); }                             // press.c:3411

// ------------------------------------------------------------------ scratch plan (press_methods.hip)

// What one batch call needs of the context's DevBufs, and the counts its kernels are launched with: made once at the top
// of the call, reserved, and then the only source of the pointers and counts in BatchArgs / DecodeArgs / ZsBufs.
struct ScratchPlan {
	const Method *m;
	uint32_t max_chunks;
	uint32_t max_htiles, hlist_cap, huf_minlen; // static-Huffman decode, else 0
	uint32_t ri_max_tiles;                      // Rice decode, else 0
	uint64_t ri_pay_bytes;                      // Rice press, else 0
	ZsBufs z; // zstd frames: kdiv, max_blocks, lit_base and the cap_* (else 0); bind() adds the pointers
	// a stall method (FAM_STALL), else 0: the pieces as a batch of `inner` - their count, their samples, the chunks of that
	// batch (max_chunks is the READS' figure, as for every method: the sample walkers behind a decode are sized by it) -
	// and the bytes of the pieces' streams (press)
	struct {
		uint32_t npieces, max_chunks;
		uint64_t piece_samples, arena_bytes;
	} sl;
	static constexpr int MAXROWS = 64; // a degraded packed recode from a stall method into zstd_svb_zd names 48
	struct Row {
		DevBuf Ctx::*buf;
		size_t bytes;
	} rows[MAXROWS]; // at most one per scratch DevBuf of Ctx
	int nrows;
	ScratchPlan &need(DevBuf Ctx::*buf, size_t bytes); // a buffer named twice keeps the larger size
	ScratchPlan &merge(const ScratchPlan &o);          // every row of o: the larger size of every buffer
	int reserve() const;
	void *ptr(DevBuf Ctx::*buf) const; // the buffer's device pointer; NULL for a buffer the plan has no row for
	void bind(BatchArgs &a) const;      // a zeroed, with every scratch pointer and count of the plan
	void bind(DecodeArgs &a) const;
	ZsBufs zs() const;                 // z with its pointers
};
ScratchPlan make_plan(int method, uint64_t total_samples, uint32_t nreads, bool decode);
ScratchPlan make_plan(const Method &method, uint64_t total_samples, uint32_t nreads, bool decode); // ... or the row itself
// The calls that decode nothing and walk samples by launch_pa_tiles' table: make_plan's max_chunks, and the table
ScratchPlan make_tiles_plan(uint64_t total_samples, uint32_t nreads);

// press_hip_recode_batch: src's streams -> samples -> dst's streams in one call.  d and p are the plans the two batch calls
// would make (their bind()s and counts serve the two halves); `all` is what the call reserves: every buffer at the larger
// of what press and depress of either method ask of it (a caller that mixes the three calls on one batch shape never sees
// a buffer grow), the press half's sample counts, the samples when the caller keeps none, and for a fused pair the press
// half's own chunk table.
struct RecodePlan {
	ScratchPlan d, p, all;
	bool fused;      // pass A's results come from the svb decode kernel (recode_fused)
	uint32_t bits;   // press_hip_recode_degraded_*: D_bits (0: none) - fused: in the decode kernel; else between the
	                 // halves, over the tile table in `all`
	bool keep_heads; // dst writes a stream for an empty read: a refused read's slot head is kept aside
};
bool recode_fused(int src, int dst);
RecodePlan make_recode_plan(int src, int dst, uint64_t total_samples, uint32_t nreads, bool keep_samples, uint32_t bits = 0);

// press_hip_recode_sizes / press_hip_recode_packed: the recode plan and the two per-read tables of PackArgs (the slot heads
// of keep_heads stay in the plan and unused: a refused read of the packed form has no slot)
RecodePlan make_recode_packed_plan(int src, int dst, uint64_t total_samples, uint32_t nreads, bool keep_samples, uint32_t bits = 0);

// press_hip_depress_pa_batch: the decode plan of the method; unless the method is fused (depress_pa_fused) the samples and
// the converter's tile table; host pointers: the staged calibration and the float arena
bool depress_pa_fused(int method);
ScratchPlan make_pa_plan(int method, uint64_t total_samples, uint32_t nreads, bool host);

// press_hip_depress_norm_batch: make_pa_plan of a method that is not fused, for every method, and what the median / MAD
// selection keeps: the count rows, the pick state and the normaliser's floats; host pointers: and stats
ScratchPlan make_norm_plan(int method, uint64_t total_samples, uint32_t nreads, bool host);

// press_hip_depress_chunks_batch: make_norm_plan's rows, the count rows and the pick state at the larger of what the
// median / MAD and the two quantiles keep; host pointers: the staged row_first and the row arena (rows_bytes) in the place
// of the float arena
ScratchPlan make_chunks_plan(int method, uint64_t total_samples, uint32_t nreads, bool host, uint64_t rows_bytes);

// press_hip_depress_chunks_trimmed_batch: make_chunks_plan's rows (never less: the workspace figure rests on it), the cuts,
// the scan's two tables and, in a detector mode, the counts the detector walks, its results and (SEGMENT) its state; host
// pointers: the row arena at rows_bytes, the three row tables at table_rows entries, row_first, the staged range and
// seg_cal, the cuts on their way back
ScratchPlan make_chunks_trimmed_plan(int method, uint64_t total_samples, uint32_t nreads, int mode, bool host, uint64_t rows_bytes,
				     uint64_t table_rows);

// press_hip_verify_batch / press_hip_depress_crc_batch: the decode plan of the method, the samples, the tile table and a
// word per read; host pointers: the staged per-read result and nbad (vf_out: nreads words, then nbad).  method < 0
// (press_hip_signal_crc32): no decode and no samples, the tile table and the words alone
ScratchPlan make_verify_plan(int method, uint64_t total_samples, uint32_t nreads, bool host);

// press_hip_signal_events: 8 bytes per read; host pointers: the staged calibration, ev_first and ev_count (the records'
// arena is reserved by the call at min(need, ev_cap) once the need is known).  Nothing per sample: the sums stay in LDS
ScratchPlan make_events_plan(uint32_t nreads, bool host);

// press_hip_signal_segments: 16 bytes per read; host pointers: the staged calibration (with_cal), seg_first, seg_count and
// thr (the records' arena is reserved by the call, as the events').  Nothing per sample
ScratchPlan make_segments_plan(uint32_t nreads, bool host, bool with_cal);
// press_hip_signal_adaptor: no scratch of its own; host pointers: the pairs and thr
ScratchPlan make_adaptor_plan(uint32_t nreads, bool host);
// press_hip_signal_range_stats: no scratch of its own; host pointers: the staged calibration (with_cal) and ranges
// (with_range), the statistics
ScratchPlan make_range_stats_plan(uint32_t nreads, bool host, bool with_cal, bool with_range);
// press_hip_signal_prefix: 24 bytes per read, the adaptor's pairs and the two ranges; host pointers: the staged calibration,
// the records, thr and the statistics
ScratchPlan make_prefix_plan(uint32_t nreads, bool host);

// press_hip_signal_tally: the chunk list (max_chunks entries of 8 bytes) and its count; host pointers: the tables, the moments
ScratchPlan make_tally_plan(uint64_t total_samples, uint32_t nreads, bool host);

// press_hip_press_sizes / press_hip_press_packed: the press plan of the method and the two per-read tables of PackArgs
ScratchPlan make_packed_plan(int method, uint64_t total_samples, uint32_t nreads);

// press_hip_stall_press_batch / press_hip_stall_depress_batch: `inner` is rccm_vbbe21_zd's plan for the pieces as a batch
// of npieces reads of piece_samples samples (its bind()s serve the inner launch), `all` what the call reserves: that, the
// piece table, the pieces' samples and - press - their streams and the segmenter's state; host pointers: press's stall[]
struct StallPlan {
	ScratchPlan inner, all;
	uint32_t npieces;
	uint64_t piece_samples, arena_bytes;
	StallBufs bufs() const; // the pointers of `all`, behind all.reserve()
};
inline bool stall_ok(int sm) { return sm >= 0 && sm < PRESS_HIP_NSTALL; }
StallPlan make_stall_plan(int stall_method, uint64_t total_samples, uint32_t nreads, bool decode, bool host);
// a.sig / off / nsamp: the caller's samples, a.out / out_off / out_len: its slots; stall: NULL or 2 * nreads words
int launch_stall_press(int stall_method, const StallPlan &p, const BatchArgs &a, uint32_t *stall, hipStream_t s);
int launch_stall_depress(const StallPlan &p, const DecodeArgs &a, hipStream_t s);
// the press in its two halves: the pieces pressed into the library's own arena (segments, plan, gather, the inner press),
// and what reads the finished pieces - the assemble above, or the sizes and the packed assemble of launch_press_packed
void launch_stall_pieces(int stall_method, const StallPlan &p, const BatchArgs &a, hipStream_t s);
// make_plan's ScratchPlan of a FAM_STALL row (the generic calls) as the StallPlan the launchers above take
StallPlan stall_plan_of(const ScratchPlan &p);

int check_method(int method); // EARG / ENOTABLE
int launch_status();          // EHIP if a kernel launch since the last call failed
int launch_press(const ScratchPlan &p, const BatchArgs &a, hipStream_t s);
int launch_depress(const ScratchPlan &p, const DecodeArgs &a, hipStream_t s);
// p from make_pa_plan; a.sig: the samples' scratch of a method that is not fused (unused for a fused one)
int launch_depress_pa(const ScratchPlan &p, const DecodeArgs &a, float *pa, const float *cal, hipStream_t s);
// p from make_norm_plan; a.sig: the samples' scratch; stats may be NULL
int launch_depress_norm(const ScratchPlan &p, const DecodeArgs &a, float *out, int32_t *stats, hipStream_t s);
// p from make_chunks_plan; a.sig: the samples' scratch.  What the caller has checked: dtype, T, overlap, the rule.
struct ChunkArgs {
	void *rows;
	uint64_t nrows_cap;
	int dtype;
	uint32_t T, overlap;
	const uint64_t *row_first;
	uint64_t total_samples;
	const press_hip_scale_rule *rule; // host; NULL: median / MAD
	int32_t *q;                       // 2 per read, or NULL
};
int launch_depress_chunks(const ScratchPlan &p, const DecodeArgs &a, const ChunkArgs &c, hipStream_t s);
// p from make_chunks_trimmed_plan; c.row_first is WRITTEN (device memory, nreads + 1).  What the caller has checked: the
// mode and the detector's parameters.  Every pointer is device memory
struct TrimArgs {
	int mode;             // PRESS_TRIM_*
	uint32_t min_keep;
	Seg2Params adaptor;   // mode ADAPTOR
	SegParams seg;        // mode SEGMENT
	const uint32_t *range; // mode RANGE: 2 per read, or NULL
	const float *seg_cal;  // mode SEGMENT: 2 per read, or NULL (the raw domain)
	uint32_t *cut;         // 2 per read, or NULL
	uint32_t *row_read, *row_start; // c.nrows_cap each, or NULL
};
int launch_depress_chunks_trimmed(const ScratchPlan &p, const DecodeArgs &a, const ChunkArgs &c, const TrimArgs &t, hipStream_t s);
// p from make_verify_plan.  launch_signal_crc: a.sig the caller's samples, a.out_n their counts.  launch_depress_crc and
// launch_verify: a.sig the samples' scratch; sig: the samples the streams are meant to hold, at a.off[]
int launch_signal_crc(const ScratchPlan &p, const DecodeArgs &a, uint32_t *crc, hipStream_t s);
int launch_depress_crc(const ScratchPlan &p, const DecodeArgs &a, uint32_t *crc, hipStream_t s);
// bits > 0: against D_bits of sig (press_hip_verify_degraded_batch)
int launch_verify(const ScratchPlan &p, const DecodeArgs &a, const int16_t *sig, uint32_t *first_bad, uint32_t *nbad, hipStream_t s,
		  uint32_t bits = 0);
bool scale_rule_ok(const press_hip_scale_rule *rule); // ranks and floats as include/press_hip.h asks
uint64_t chunk_rows_of(uint32_t c, uint32_t T, uint32_t S); // rows of a read of c samples in press_hip_chunk_plan, S = T - overlap
// phases: PACK_SIZE | PACK_WRITE (press_internal.h); a.out_off must be pk.slot
int launch_press_packed(const ScratchPlan &p, const BatchArgs &a, const PackArgs &pk, int phases, hipStream_t s);

// ------------------------------------------------------------------ static Huffman table (press_table.hip)

int upload_table(const uint32_t len[256], const uint64_t bits[256]); // -> HuffDev in g.huff, cached by content
int table_from_encoder(SymbolEncoder *se);                           // the caller's huffman.h objects -> upload_table
int table_from_tree(huffman_node *root);

} // namespace ph
