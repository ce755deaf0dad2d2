// press_methods.hip - everything that interprets a row of the method table (press_host.h): the reference's X_bound,
// the scratch plan of a batch and its dispatch to the kernel launchers of press_*.hip.

#include <stdlib.h>

#include <cmath>
#include <vector>

#include "press_host.h"
#include "zs_table.h"

using namespace ph;

extern "C" uint64_t press_hip_bound(int method, uint32_t n)
{
	if (!method_ok(method))
		return 0;
	const Method &m = method_row(method);
	switch (m.family) {
	case FAM_SVB:
		if (m.slow5)
			return (uint64_t) (n + 3) / 4 + (uint64_t) n * 4 + 4; // slow5_press.c:1037 (streamvbyte.h:31) + u32 count
		return m.key2 ? bound_svb32(n) : bound_svb16(n);              // press.c:1585 / press.c:1568,1678
	case FAM_EX:
		if (m.exfmt == EXF_EXZD)
			return bound_svb32((uint32_t) bound_vbzd(n));         // press.c:8461
		return bound_vbzd(n);                                         // press.c:3411,4409
	case FAM_ZSTD: // the inner stream, the svb kinds' behind its u32 count (press.c:1860, 2020, 8549)
		return zstd_bound_((m.kdiv ? 4 : 0) + press_hip_bound(m.inner, n));
	case FAM_STALL: // the inner method's (press.c:7723, 7893, 7981)
		return press_hip_bound(m.inner, n);
	}
	return 0;
}

// ------------------------------------------------------------------ scratch plan
//
// Which of the context's device buffers a batch needs, how large, and the counts derived from its shape.  reserve(),
// the bind()s and press_hip_workspace_bytes() all read the one list of rows make_plan() writes: a buffer cannot be bound
// without being sized, nor sized in two places.

namespace ph {

ScratchPlan &ScratchPlan::need(DevBuf Ctx::*buf, size_t bytes)
{
	int i = 0;
	while (i < nrows && rows[i].buf != buf)
		i++;
	if (i == nrows) {
		if (nrows == MAXROWS) // (a plan is a union of a few calls' buffers: MAXROWS is above every one)
			abort();
		rows[nrows++] = { buf, 0 };
	}
	rows[i].bytes = bytes > rows[i].bytes ? bytes : rows[i].bytes;
	return *this;
}

ScratchPlan &ScratchPlan::merge(const ScratchPlan &o)
{
	for (int i = 0; i < o.nrows; i++)
		need(o.rows[i].buf, o.rows[i].bytes);
	return *this;
}

int ScratchPlan::reserve() const
{
	for (int i = 0; i < nrows; i++)
		if ((g.*rows[i].buf).reserve(rows[i].bytes))
			return PRESS_HIP_EHIP;
	return 0;
}

void *ScratchPlan::ptr(DevBuf Ctx::*buf) const
{
	for (int i = 0; i < nrows; i++)
		if (rows[i].buf == buf)
			return (g.*buf).p;
	return nullptr;
}

// Chunks (and tiles of the sample walkers) a batch can have: CHUNK samples each, and a partial one per read
static inline uint32_t plan_max_chunks(uint64_t total_samples, uint32_t nreads) { return (uint32_t) (total_samples / CHUNK + nreads + 1); }

ScratchPlan make_tiles_plan(uint64_t total_samples, uint32_t nreads)
{
	ScratchPlan p{};
	p.max_chunks = plan_max_chunks(total_samples, nreads);
	p.need(&Ctx::pa_tile, (size_t) p.max_chunks * sizeof(uint2)).need(&Ctx::pa_ctl, 64);
	return p;
}

ScratchPlan make_plan(int method, uint64_t total_samples, uint32_t nreads, bool decode)
{
	return make_plan(method_row(method), total_samples, nreads, decode);
}

// (a row of METHODS, or a private one of RCF_METHODS)
ScratchPlan make_plan(const Method &method, uint64_t total_samples, uint32_t nreads, bool decode)
{
	if (method.family == FAM_STALL) {
		// the family's own plan (make_stall_plan): the inner method's over the pieces and the piece table.  max_chunks is
		// the reads' figure, the pieces' is kept aside for the inner launch (stall_plan_of)
		const StallPlan sp = make_stall_plan(method.stall, total_samples, nreads, decode, false);
		ScratchPlan p = sp.all;
		p.m = &method;
		p.sl = { sp.npieces, sp.inner.max_chunks, sp.piece_samples, sp.arena_bytes };
		p.max_chunks = plan_max_chunks(total_samples, nreads);
		return p;
	}
	ScratchPlan p{};
	p.m = &method;
	const bool zs = p.m->family == FAM_ZSTD;
	const Method &k = zs ? METHODS[p.m->inner] : *p.m; // the method whose kernels make / read the samples
	const size_t nr = (size_t) nreads + 1;
	p.max_chunks = plan_max_chunks(total_samples, nreads);
	const size_t mc = p.max_chunks;
	p.need(&Ctx::meta, nr * sizeof(ReadMeta));
	if (zs) {
		p.z.kdiv = p.m->kdiv;
		p.z.max_blocks = (uint32_t) (total_samples * 2 / zs::BLOCK_LITS + nreads + 1);
		const size_t mb = p.z.max_blocks;
		// what a batch of this library's frames needs, with room for others; a frame that does not
		// fit (tiny blocks, thousands of trees) goes to libzstd on the host
		p.z.cap_copy = p.z.max_blocks + (uint32_t) (total_samples / 256) + 16 * nreads + 64;
		p.z.cap_units = p.z.max_blocks / 8 + 2 * nreads + 64;
		p.z.cap_trees = 4 * nreads + 64;
		p.z.cap_long = (uint32_t) (total_samples / 8192) + nreads + 64; // (blocks of at least 32 KiB of literals)
		// frames with sequences (libzstd's own): their literals in the second half of ztmp.  Bytes per sample the
		// inner stream can take at most: device, zs_content_max
		p.z.lit_base = (p.m->kdiv ? total_samples * 9 / 4 : total_samples * 9) + ((uint64_t) nreads + 1) * 128 + 64;
		// (level 1 on signal data: a handful per block; higher levels: one per ~20 content bytes)
		const uint64_t cs = total_samples / 4 + 64ull * nreads + 1024;
		p.z.cap_seq = cs > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t) cs;
		p.z.cap_xblk = p.z.max_blocks / 4 + 4 * nreads + 64;
		p.need(&Ctx::ztmp, decode ? 2 * p.z.lit_base : p.z.lit_base).need(&Ctx::zoff, nr * 8).need(&Ctx::zoff4, nr * 8)
			.need(&Ctx::zlen, nr * 8).need(&Ctx::zrd, nr * sizeof(ZsRead));
		if (decode)
			p.need(&Ctx::zn, nr * 4).need(&Ctx::zdseq, (size_t) p.z.cap_seq * sizeof(ZsSeq))
				.need(&Ctx::zdxblk, (size_t) p.z.cap_xblk * sizeof(ZsXBlk)).need(&Ctx::zdcopy, (size_t) p.z.cap_copy * sizeof(ZsCopy))
				.need(&Ctx::zdhuf, (size_t) p.z.cap_units * 8 * sizeof(ZsHuf)).need(&Ctx::zdunit, (size_t) p.z.cap_units * sizeof(ZsUnit))
				.need(&Ctx::zdtree, (size_t) p.z.cap_trees * sizeof(ZsTree)).need(&Ctx::zdlong, (size_t) p.z.cap_long * sizeof(ZsLong))
				.need(&Ctx::zdctl, sizeof(ZsDCtl));
		else // (ex_pos / ex_val of the svb kinds: the lists of key bytes that are not zero)
			p.need(&Ctx::zhist, nr * 1024).need(&Ctx::ztab, nr * sizeof(zs::Table)).need(&Ctx::zfirst, nr * 4)
				.need(&Ctx::zblk, mb * 4).need(&Ctx::zsbits, mb * 16).need(&Ctx::zbpos, mb * 4).need(&Ctx::zbflag, mb)
				.need(&Ctx::zkcnt, mc * 4).need(&Ctx::znb, 64)
				.need(&Ctx::ex_pos, (total_samples + 64) * 4).need(&Ctx::ex_val, (total_samples + 64) * 4);
	}
	p.need(&Ctx::chunks, mc * sizeof(ChunkDesc)).need(&Ctx::gran, 2 * mc * sizeof(uint64_t)).need(&Ctx::ctl, 2 * sizeof(ChunkCtl))
		.need(&Ctx::first_chunk, nr * 4);
	if (k.family != FAM_EX)
		return p;
	p.need(&Ctx::ex_pos, (total_samples + 64) * 4).need(&Ctx::ex_val, (total_samples + 64) * 4);
	if (!decode && is_shuff(k))
		p.need(&Ctx::cbits, mc * sizeof(ChunkBits));
	if (uses_low_tmp(k))
		p.need(&Ctx::low, total_samples + 64); // the one-byte values between the two stages
	if ((is_rice(k) || is_dhuf(k)) && !decode) {
		// press_prefix.h: 32 units per chunk; a staged payload never takes more than nine bits a value, the reads' stagings
		// start at twice their sample offsets
		p.ri_pay_bytes = 2 * total_samples + 64;
		p.need(&Ctx::ri_sum, mc * PFX_UPC * 32).need(&Ctx::ri_start, mc * PFX_UPC * 8).need(&Ctx::ri_rd, nr * sizeof(PfxRead))
			.need(&Ctx::ri_pay, p.ri_pay_bytes);
	}
	if ((is_rice(k) || is_dhuf(k)) && decode) {
		// tiles of PFX_DT subsequences of PFX_SUB bits: a read has at most ceil((9 nlow + 3) / PFX_SUB) subsequences
		const uint64_t dt = total_samples * 9 / ((uint64_t) PFX_SUB * PFX_DT) + 2ull * nreads + 2;
		const size_t mt = p.ri_max_tiles = dt > 0xFFFFFFull ? 0xFFFFFFu : (uint32_t) dt;
		p.need(&Ctx::ri_drd, nr * sizeof(PfxDRead)).need(&Ctx::ri_tile, mt * sizeof(uint2)).need(&Ctx::ri_rec, mt * PFX_DT * 12)
			.need(&Ctx::ri_tbase, mt * 16).need(&Ctx::ri_ctl, PFX_CTL_WORDS * 4);
	}
	if (is_dhuf(k)) // press_dhuf.hip: beside the engine's buffers, the reads' tables
		p.need(&Ctx::dh_tab, nr * (decode ? sizeof(DhTab) : (size_t) DH_PRESS_TAB));
	if (decode && is_shuff(k)) {
		// Huffman tiles of a batch (press_huffman.hip, k_huff_tiles): a read of n samples has at most
		// n - 1 codes of at most maxlen bits, cut into tiles of HUF_HT subsequences
		const uint32_t minlen = g.tmin, maxlen = g.tmax;
		const uint64_t tb = (uint64_t) HUF_HT * (minlen >= 4 ? 256u : minlen >= 2 ? 128u : 64u);
		const uint64_t ht = total_samples * maxlen / tb + nreads + 1;
		const size_t mt = p.max_htiles = ht > 0xFFFFFFull ? 0xFFFFFFu : (uint32_t) ht;
		// broken links a repair round can list (3 % of the subsequences on signal data; what does not fit is left to
		// the serial pass): a table that never synchronises lists every subsequence; k_huf_sync's workgroups take
		// slots 1024 at a time
		const size_t hl = mt * HUF_HT + (1u << 20);
		p.hlist_cap = (uint32_t) hl;
		p.huf_minlen = minlen | (g.table_trie ? HUF_NEEDS_TRIE : 0u);
		p.need(&Ctx::low, total_samples + 64).need(&Ctx::htiles, mt * sizeof(HufTile))
			.need(&Ctx::hunit, mt * (HUF_HT / 64) * sizeof(HufUnit)).need(&Ctx::hrec, mt * HUF_HT * 4)
			.need(&Ctx::hlist, hl * 8).need(&Ctx::hread, nr * 8)
			.need(&Ctx::hwave, mt * (HUF_HT / 64) * 8).need(&Ctx::hbits, mt * (HUF_HT / 64) * 8)
			.need(&Ctx::hend, mt * HUF_HT + 64).need(&Ctx::hmin, nr * 4);
	}
	return p;
}

ScratchPlan make_packed_plan(int method, uint64_t total_samples, uint32_t nreads)
{
	ScratchPlan p = make_plan(method, total_samples, nreads, false);
	const size_t nr = (size_t) nreads + 1;
	p.need(&Ctx::pneed, nr * 8).need(&Ctx::pslot, nr * 8);
	return p;
}

// The stall methods: rccm_vbbe21_zd's plan over the pieces, and the piece table.  The pieces' streams are held at the
// most a stream can take (stall_arena_bytes), so that a piece never fails for want of room: the caller's slot decides
StallPlan make_stall_plan(int stall_method, uint64_t total_samples, uint32_t nreads, bool decode, bool host)
{
	StallPlan p{};
	p.npieces = (decode ? STALL_DPIECES : STALL_PIECES) * nreads;
	p.piece_samples = stall_piece_samples(stall_method, total_samples, nreads, decode);
	p.arena_bytes = decode ? 0 : stall_arena_bytes(p.piece_samples, p.npieces);
	p.inner = make_plan(PRESS_HIP_RCCM_VBBE21_ZD, p.piece_samples, p.npieces, decode);
	p.all = p.inner;
	const size_t np = (size_t) p.npieces + 1, nr = (size_t) nreads + 1;
	p.all.need(&Ctx::sl_rd, nr * sizeof(StallRead)).need(&Ctx::sl_poff, np * 8).need(&Ctx::sl_pn, np * 4).need(&Ctx::sl_pooff, np * 8)
		.need(&Ctx::sl_polen, np * 8).need(&Ctx::sl_psig, p.piece_samples * 2 + 64);
	if (decode)
		p.all.need(&Ctx::sl_poutn, np * 4);
	else
		p.all.need(&Ctx::sl_seg, nr * 8).need(&Ctx::sg_state, segments_state_bytes(nreads)).need(&Ctx::sl_parena, p.arena_bytes);
	if (host && !decode)
		p.all.need(&Ctx::sl_stall, nr * 8);
	return p;
}

StallPlan stall_plan_of(const ScratchPlan &p)
{
	StallPlan sp{ p, p, p.sl.npieces, p.sl.piece_samples, p.sl.arena_bytes };
	sp.inner.max_chunks = p.sl.max_chunks;
	return sp;
}

StallBufs StallPlan::bufs() const
{
	StallBufs b{};
	b.seg = (uint2 *) all.ptr(&Ctx::sl_seg);
	b.rd = (StallRead *) all.ptr(&Ctx::sl_rd);
	b.poff = (uint64_t *) all.ptr(&Ctx::sl_poff);
	b.pn = (uint32_t *) all.ptr(&Ctx::sl_pn);
	b.pooff = (uint64_t *) all.ptr(&Ctx::sl_pooff);
	b.polen = (uint64_t *) all.ptr(&Ctx::sl_polen);
	b.poutn = (uint32_t *) all.ptr(&Ctx::sl_poutn);
	b.psig = (int16_t *) all.ptr(&Ctx::sl_psig);
	b.parena = (uint8_t *) all.ptr(&Ctx::sl_parena);
	b.sig_cap = piece_samples;
	b.arena_cap = arena_bytes;
	return b;
}

// The svb family's decode kernel writes picoamperes itself; the zstd compositions over it take the general path (their
// second stage is launched by press_zstd.hip with arguments of its own).
bool depress_pa_fused(int method) { return method_ok(method) && method_row(method).family == FAM_SVB; }

ScratchPlan make_pa_plan(int method, uint64_t total_samples, uint32_t nreads, bool host)
{
	ScratchPlan p = make_plan(method, total_samples, nreads, true);
	if (!depress_pa_fused(method))
		p.need(&Ctx::rsig, total_samples * 2 + 64).need(&Ctx::pa_tile, (size_t) p.max_chunks * sizeof(uint2))
			.need(&Ctx::pa_ctl, 64);
	if (host)
		p.need(&Ctx::pa_cal, (size_t) nreads * 8).need(&Ctx::pa_out, total_samples * 4 + 64);
	return p;
}

// Normalised floats: every method decodes into rsig (the median needs the whole read before the first float)
ScratchPlan make_norm_plan(int method, uint64_t total_samples, uint32_t nreads, bool host)
{
	ScratchPlan p = make_plan(method, total_samples, nreads, true);
	p.need(&Ctx::rsig, total_samples * 2 + 64).need(&Ctx::pa_tile, (size_t) p.max_chunks * sizeof(uint2)).need(&Ctx::pa_ctl, 64)
		.need(&Ctx::st_rows, stat_rows_bytes(nreads)).need(&Ctx::st_read, stat_state_bytes(nreads))
		.need(&Ctx::st_cal, (size_t) nreads * 8);
	if (host)
		p.need(&Ctx::st_stats, (size_t) nreads * 8).need(&Ctx::pa_out, total_samples * 4 + 64);
	return p;
}

// Chunk rows: the normalised call's plan; one set of count rows and state serves either calibration
ScratchPlan make_chunks_plan(int method, uint64_t total_samples, uint32_t nreads, bool host, uint64_t rows_bytes)
{
	ScratchPlan p = make_norm_plan(method, total_samples, nreads, false);
	p.need(&Ctx::st_rows, quant_rows_bytes(nreads, 2)).need(&Ctx::st_read, quant_state_bytes(nreads));
	if (host)
		p.need(&Ctx::st_stats, (size_t) nreads * 8).need(&Ctx::ch_first, ((size_t) nreads + 1) * 8).need(&Ctx::ch_rows, rows_bytes + 64);
	return p;
}

// Trimmed chunk rows: the chunk call's plan, the cuts and the tables of the scan that makes row_first; a detector mode adds
// what its kernel reads and writes
ScratchPlan make_chunks_trimmed_plan(int method, uint64_t total_samples, uint32_t nreads, int mode, bool host, uint64_t rows_bytes,
				     uint64_t table_rows)
{
	ScratchPlan p = make_chunks_plan(method, total_samples, nreads, false, 0);
	const size_t nr = (size_t) nreads + 1;
	p.need(&Ctx::tr_cut, nr * 8).need(&Ctx::pneed, nr * 8).need(&Ctx::pslot, nr * 8);
	if (mode != PRESS_TRIM_RANGE)
		p.need(&Ctx::tr_cnt, nr * 4).need(&Ctx::tr_det, nr * 8);
	if (mode == PRESS_TRIM_SEGMENT)
		p.need(&Ctx::sg_state, segments_state_bytes(nreads));
	if (host)
		p.need(&Ctx::st_stats, (size_t) nreads * 8).need(&Ctx::tr_first, nr * 8).need(&Ctx::ch_rows, rows_bytes + 64)
			.need(&Ctx::tr_read, table_rows * 4 + 4).need(&Ctx::tr_start, table_rows * 4 + 4).need(&Ctx::tr_user, nr * 8)
			.need(&Ctx::px_range, nr * 8).need(&Ctx::sg_cal, nr * 8);
	return p;
}

// Verify and CRC-32: the general picoampere plan (decode, samples, tile table) for every method, and a word per read
ScratchPlan make_verify_plan(int method, uint64_t total_samples, uint32_t nreads, bool host)
{
	const ScratchPlan tiles = make_tiles_plan(total_samples, nreads);
	ScratchPlan p = tiles;
	if (method >= 0) { // (the same max_chunks)
		p = make_plan(method, total_samples, nreads, true);
		p.need(&Ctx::rsig, total_samples * 2 + 64).merge(tiles);
	}
	p.need(&Ctx::vf_raw, (size_t) nreads * 4 + 4);
	if (host)
		p.need(&Ctx::vf_out, (size_t) nreads * 4 + 4);
	return p;
}

// Events: the walk keeps its sums in LDS and registers, so the scratch does not depend on total_samples
ScratchPlan make_events_plan(uint32_t nreads, bool host)
{
	ScratchPlan p{};
	p.need(&Ctx::ev_state, events_state_bytes(nreads));
	if (host)
		p.need(&Ctx::ev_cal, (size_t) nreads * 8).need(&Ctx::ev_first, ((size_t) nreads + 1) * 8).need(&Ctx::ev_cnt, (size_t) nreads * 4);
	return p;
}

// Segments: sums and walk state stay in registers, so the scratch does not depend on total_samples either
ScratchPlan make_segments_plan(uint32_t nreads, bool host, bool with_cal)
{
	ScratchPlan p{};
	p.need(&Ctx::sg_state, segments_state_bytes(nreads));
	if (host) {
		p.need(&Ctx::sg_first, ((size_t) nreads + 1) * 8).need(&Ctx::sg_cnt, (size_t) nreads * 4).need(&Ctx::sg_thr, (size_t) nreads * 8);
		if (with_cal)
			p.need(&Ctx::sg_cal, (size_t) nreads * 8);
	}
	return p;
}

ScratchPlan make_adaptor_plan(uint32_t nreads, bool host)
{
	ScratchPlan p{};
	if (host)
		p.need(&Ctx::sg_out, (size_t) nreads * 8).need(&Ctx::sg_thr, (size_t) nreads * 8);
	return p;
}

ScratchPlan make_range_stats_plan(uint32_t nreads, bool host, bool with_cal, bool with_range)
{
	ScratchPlan p{};
	if (host) {
		p.need(&Ctx::px_stat, (size_t) nreads * 12);
		if (with_cal)
			p.need(&Ctx::sg_cal, (size_t) nreads * 8);
		if (with_range)
			p.need(&Ctx::px_range, (size_t) nreads * 8);
	}
	return p;
}

ScratchPlan make_prefix_plan(uint32_t nreads, bool host)
{
	ScratchPlan p{};
	p.need(&Ctx::px_pair, (size_t) nreads * 8).need(&Ctx::px_range, (size_t) nreads * 16);
	if (host)
		p.need(&Ctx::sg_cal, (size_t) nreads * 8).need(&Ctx::px_out, (size_t) nreads * 16).need(&Ctx::sg_thr, (size_t) nreads * 8)
			.need(&Ctx::px_stat, (size_t) nreads * 24);
	return p;
}

// Tallies: 8 bytes per chunk of the work list, nothing per sample
ScratchPlan make_tally_plan(uint64_t total_samples, uint32_t nreads, bool host)
{
	ScratchPlan p{};
	if (nreads == 0)
		return p;
	p.max_chunks = plan_max_chunks(total_samples, nreads);
	p.need(&Ctx::tl_chunks, tally_scratch_bytes(p.max_chunks)).need(&Ctx::tl_ctl, 64);
	if (host)
		p.need(&Ctx::tl_tab, (size_t) PRESS_HIP_TALLY_WORDS * 8).need(&Ctx::tl_mom, (size_t) nreads * sizeof(press_hip_moments));
	return p;
}

// Fused pairs: BLOW5's and the reference's svb-zd streams into any exception-split method.  (svb12 has no deltas; the zstd
// kinds and the svb destinations take the general path.)
bool recode_fused(int src, int dst)
{
	if (!method_ok(src) || !method_ok(dst))
		return false;
	return method_row(src).family == FAM_SVB && method_row(src).zd && method_row(dst).family == FAM_EX;
}

// bits > 0 (press_hip_recode_degraded_*): a fused pair's decode kernel degrades the samples it holds and the plan is that
// of bits == 0; every other pair runs the degrade kernel between its halves, over a tile table of the rooms
RecodePlan make_recode_plan(int src, int dst, uint64_t total_samples, uint32_t nreads, bool keep_samples, uint32_t bits)
{
	RecodePlan r{};
	r.d = make_plan(src, total_samples, nreads, true);
	r.p = make_plan(dst, total_samples, nreads, false);
	r.fused = recode_fused(src, dst);
	r.bits = bits;
	const Method &m = method_row(dst);
	r.keep_heads = (m.family == FAM_SVB && m.slow5) || (m.family == FAM_ZSTD && m.kdiv);
	r.all = r.d;
	r.all.merge(r.p).merge(make_plan(src, total_samples, nreads, false)).merge(make_plan(dst, total_samples, nreads, true));
	const size_t nr = (size_t) nreads + 1;
	r.all.need(&Ctx::rn, nr * 4);
	if (!keep_samples)
		r.all.need(&Ctx::rsig, total_samples * 2 + 64);
	if (r.keep_heads)
		r.all.need(&Ctx::rkeep, nr * RECODE_KEEP);
	if (r.fused)
		r.all.need(&Ctx::pchunks, (size_t) r.p.max_chunks * sizeof(ChunkDesc)).need(&Ctx::pfirst, nr * 4)
			.need(&Ctx::pctl, 2 * sizeof(ChunkCtl));
	if (bits && !r.fused)
		r.all.need(&Ctx::pa_tile, (size_t) r.d.max_chunks * sizeof(uint2)).need(&Ctx::pa_ctl, 64);
	return r;
}

RecodePlan make_recode_packed_plan(int src, int dst, uint64_t total_samples, uint32_t nreads, bool keep_samples, uint32_t bits)
{
	RecodePlan r = make_recode_plan(src, dst, total_samples, nreads, keep_samples, bits);
	const size_t nr = (size_t) nreads + 1;
	r.all.need(&Ctx::pneed, nr * 8).need(&Ctx::pslot, nr * 8);
	return r;
}

// Most fields of the argument blocks carry the name of the buffer behind them (ZsBufs: without its z)
#define BIND(x, f, buf) x.f = (decltype(x.f)) ptr(&Ctx::buf)
#define B(f) BIND(a, f, f)
#define BZ(f) BIND(z, f, z##f)

void ScratchPlan::bind(BatchArgs &a) const
{
	memset(&a, 0, sizeof a);
	B(meta), B(ex_pos), B(ex_val), B(chunks), B(gran), B(ctl), B(first_chunk), B(cbits);
	BIND(a, low_tmp, low);
	B(ri_sum), B(ri_start), B(ri_rd), B(ri_pay), B(dh_tab);
	a.ri_pay_bytes = ri_pay_bytes;
	a.huff = (const HuffDev *) g.huff.p; // (the table's, not the batch's: upload_table)
	a.max_chunks = max_chunks;
}

void ScratchPlan::bind(DecodeArgs &a) const
{
	memset(&a, 0, sizeof a);
	B(meta), B(ex_pos), B(ex_val), B(low), B(chunks), B(gran), B(ctl), B(first_chunk);
	B(htiles), B(hunit), B(hrec), B(hlist), B(hread), B(hwave), B(hbits), B(hend), B(hmin);
	a.huff = (const HuffDev *) g.huff.p;
	a.max_chunks = max_chunks;
	a.max_htiles = max_htiles;
	a.hlist_cap = hlist_cap;
	a.huf_minlen = huf_minlen;
	B(ri_drd), B(ri_tile), B(ri_rec), B(ri_tbase), B(ri_ctl), B(dh_tab);
	a.ri_max_tiles = ri_max_tiles;
}

ZsBufs ScratchPlan::zs() const
{
	ZsBufs z = this->z;
	BIND(z, ztmp, ztmp), BIND(z, zoff, zoff), BIND(z, zoff4, zoff4), BIND(z, zlen, zlen), BIND(z, zn, zn);
	BZ(hist), BZ(tab), BZ(sbits), BZ(bpos), BZ(bflag), BZ(kcnt), BZ(rd);
	BZ(dcopy), BZ(dhuf), BZ(dunit), BZ(dtree), BZ(dlong), BZ(dctl), BZ(dseq), BZ(dxblk);
	BIND(z, first_blk, zfirst), BIND(z, blk_read, zblk), BIND(z, nblocks, znb);
	return z;
}

} // namespace ph

// The *_workspace_bytes: a call's plan summed, with the device table for a Huffman method.  The buffers are shared and
// grow-only, so each call's figure folds in (merge) the plans of the calls a caller mixes it with on one batch shape: no
// buffer grows then.  Host arithmetic, no device needed.
static uint64_t plan_bytes(const ScratchPlan &p, bool huffman)
{
	uint64_t b = huffman ? sizeof(HuffDev) : 0;
	for (int i = 0; i < p.nrows; i++)
		b += p.rows[i].bytes;
	return b;
}
static bool is_shuff(int method) { return is_shuff(method_row(method)); }

// the larger of what press and depress ask of every buffer
extern "C" uint64_t press_hip_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads)
{
	API_LOCK; // (the Huffman decoder's rows depend on the table in force)
	if (!method_ok(method))
		return 0;
	return plan_bytes(make_plan(method, total_samples, nreads, false).merge(make_plan(method, total_samples, nreads, true)), is_shuff(method));
}

extern "C" uint64_t press_hip_recode_workspace_bytes(int src_method, int dst_method, uint64_t total_samples, uint32_t nreads,
						     int keep_samples)
{
	API_LOCK;
	if (!method_ok(src_method) || !method_ok(dst_method))
		return 0;
	return plan_bytes(make_recode_plan(src_method, dst_method, total_samples, nreads, keep_samples != 0).all,
			  is_shuff(src_method) || is_shuff(dst_method));
}

// as press_hip_workspace_bytes, and the two tables of the packed plan
extern "C" uint64_t press_hip_packed_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads)
{
	API_LOCK;
	if (!method_ok(method))
		return 0;
	return plan_bytes(make_packed_plan(method, total_samples, nreads).merge(make_plan(method, total_samples, nreads, true)), is_shuff(method));
}

// the degraded recode calls: bits > 0 adds the degrade kernel's tile table to the undegraded figure of a pair that is not
// fused; bits == 0, and a fused pair, nothing
extern "C" uint64_t press_hip_recode_degraded_workspace_bytes(int src_method, int dst_method, uint32_t bits, uint64_t total_samples,
							      uint32_t nreads, int keep_samples)
{
	API_LOCK;
	if (!method_ok(src_method) || !method_ok(dst_method) || bits > 8)
		return 0;
	return plan_bytes(make_recode_plan(src_method, dst_method, total_samples, nreads, keep_samples != 0, bits).all,
			  is_shuff(src_method) || is_shuff(dst_method));
}

extern "C" uint64_t press_hip_recode_degraded_packed_workspace_bytes(int src_method, int dst_method, uint32_t bits, uint64_t total_samples,
								     uint32_t nreads, int keep_samples)
{
	API_LOCK;
	if (!method_ok(src_method) || !method_ok(dst_method) || bits > 8)
		return 0;
	return plan_bytes(make_recode_packed_plan(src_method, dst_method, total_samples, nreads, keep_samples != 0, bits).all,
			  is_shuff(src_method) || is_shuff(dst_method));
}

// as press_hip_recode_workspace_bytes, and the two tables of the packed plan
extern "C" uint64_t press_hip_recode_packed_workspace_bytes(int src_method, int dst_method, uint64_t total_samples,
							    uint32_t nreads, int keep_samples)
{
	API_LOCK;
	if (!method_ok(src_method) || !method_ok(dst_method))
		return 0;
	return plan_bytes(make_recode_packed_plan(src_method, dst_method, total_samples, nreads, keep_samples != 0).all,
			  is_shuff(src_method) || is_shuff(dst_method));
}

// as press_hip_workspace_bytes, and what the device-resident press_hip_depress_pa_batch adds for a method that is not fused
extern "C" uint64_t press_hip_depress_pa_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads)
{
	API_LOCK;
	if (!method_ok(method))
		return 0;
	return plan_bytes(make_pa_plan(method, total_samples, nreads, false).merge(make_plan(method, total_samples, nreads, false)), is_shuff(method));
}

// ... and what the device-resident press_hip_depress_norm_batch adds
extern "C" uint64_t press_hip_depress_norm_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads)
{
	API_LOCK;
	if (!method_ok(method))
		return 0;
	return plan_bytes(make_norm_plan(method, total_samples, nreads, false).merge(make_plan(method, total_samples, nreads, false)), is_shuff(method));
}

// ... and what the device-resident press_hip_depress_chunks_batch keeps: the rows are the caller's, so T and overlap
// only have to be valid
extern "C" uint64_t press_hip_depress_chunks_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads, uint32_t T,
							     uint32_t overlap)
{
	API_LOCK;
	if (!method_ok(method) || T == 0 || T % 8 || overlap >= T)
		return 0;
	return plan_bytes(make_chunks_plan(method, total_samples, nreads, false, 0).merge(make_plan(method, total_samples, nreads, false)),
			  is_shuff(method));
}

// ... and what the device-resident press_hip_depress_chunks_trimmed_batch keeps in `mode`
extern "C" uint64_t press_hip_depress_chunks_trimmed_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads, uint32_t T,
								     uint32_t overlap, int mode)
{
	API_LOCK;
	if (!method_ok(method) || T == 0 || T % 8 || overlap >= T || mode < PRESS_TRIM_RANGE || mode > PRESS_TRIM_SEGMENT)
		return 0;
	return plan_bytes(make_chunks_trimmed_plan(method, total_samples, nreads, mode, false, 0, 0).merge(make_plan(method, total_samples, nreads, false)),
			  is_shuff(method));
}

// ... and what the device-resident press_hip_verify_batch and press_hip_depress_crc_batch add
extern "C" uint64_t press_hip_verify_workspace_bytes(int method, uint64_t total_samples, uint32_t nreads)
{
	API_LOCK;
	if (!method_ok(method))
		return 0;
	return plan_bytes(make_verify_plan(method, total_samples, nreads, false).merge(make_plan(method, total_samples, nreads, false)), is_shuff(method));
}

// what the device-resident press_hip_signal_events keeps: 8 bytes per read, nothing per sample, no slices
extern "C" uint64_t press_hip_signal_events_workspace_bytes(uint64_t total_samples, uint32_t nreads)
{
	(void) total_samples;
	return plan_bytes(make_events_plan(nreads, false), false);
}

// what the device-resident press_hip_signal_segments keeps: 16 bytes per read, nothing per sample, no slices
// (press_hip_signal_adaptor keeps nothing)
extern "C" uint64_t press_hip_signal_segments_workspace_bytes(uint64_t total_samples, uint32_t nreads)
{
	(void) total_samples;
	return plan_bytes(make_segments_plan(nreads, false, false), false);
}

// what the device-resident press_hip_signal_prefix keeps: 24 bytes per read (the adaptor's pairs, the two ranges), nothing
// per sample (press_hip_signal_range_stats keeps nothing)
extern "C" uint64_t press_hip_signal_prefix_workspace_bytes(uint32_t nreads)
{
	return plan_bytes(make_prefix_plan(nreads, false), false);
}

// what the device-resident press_hip_signal_tally keeps: the chunk list and its count
extern "C" uint64_t press_hip_signal_tally_workspace_bytes(uint64_t total_samples, uint32_t nreads)
{
	return plan_bytes(make_tally_plan(total_samples, nreads, false), false);
}

// The stall methods' bound is rccm_vbbe21_zd's (press.c:7723, 7893, 7981)
extern "C" uint64_t press_hip_stall_bound(int stall_method, uint32_t n)
{
	return stall_ok(stall_method) ? press_hip_bound(PRESS_HIP_RCCM_VBBE21_ZD, n) : 0;
}

// the larger of what the device-resident press_hip_stall_press_batch and press_hip_stall_depress_batch ask of every buffer
extern "C" uint64_t press_hip_stall_workspace_bytes(int stall_method, uint64_t total_samples, uint32_t nreads)
{
	if (!stall_ok(stall_method))
		return 0;
	ScratchPlan p = make_stall_plan(stall_method, total_samples, nreads, false, false).all;
	return plan_bytes(p.merge(make_stall_plan(stall_method, total_samples, nreads, true, false).all), false);
}

// launches of the inner press of the stall methods: one per press, sizes or packed call, whatever its phases
static uint64_t n_stall_inner;
extern "C" uint64_t press_hip_debug_stall_inner_presses(void) { return n_stall_inner; }

// segs[0] of jnn_raw under JNNV1_CDNA_PARAM (press.c:7734), the plan, the pieces, rccm_vbbe21_zd over them: every piece's
// stream and its length lie in the library's arena (sl_parena, polen[]) before a byte reaches the caller
void ph::launch_stall_pieces(int stall_method, const StallPlan &p, const BatchArgs &a, hipStream_t s)
{
	const StallBufs b = p.bufs();
	const SegParams cdna = { 0.75f, 50, 50, 150, 0.25f, 5, 0.0f, 0.0f }; // jnn.h:40-49 (press_hip_jnn_params_preset(0))
	launch_segments_first(a.sig, a.off, a.nsamp, a.nreads, cdna, p.all.ptr(&Ctx::sg_state), b.seg, s);
	launch_stall_plan(stall_method, a.nsamp, a.nreads, b, s);
	launch_stall_gather(a.sig, a.off, a.nsamp, a.nreads, b, s);
	BatchArgs in;
	p.inner.bind(in);
	in.nreads = p.npieces;
	in.sig = b.psig;
	in.off = b.poff;
	in.nsamp = b.pn;
	in.out = b.parena;
	in.out_off = b.pooff;
	in.out_len = b.polen;
	const Method &m = METHODS[PRESS_HIP_RCCM_VBBE21_ZD];
	launch_ex_encode_chunked(in, m.exfmt, m.ent, s);
	n_stall_inner++;
}

// ... and the streams
int ph::launch_stall_press(int stall_method, const StallPlan &p, const BatchArgs &a, uint32_t *stall, hipStream_t s)
{
	launch_stall_pieces(stall_method, p, a, s);
	launch_stall_assemble(stall_method, a.nsamp, a.nreads, p.bufs(), a.out, a.out_off, a.out_len, stall, s);
	return launch_status();
}

// Packed press of a stall method.  PACK_SIZE: the pieces, k_stall_sizes - the streams' exact lengths out of polen[] - and
// with a layout the scan; PACK_WRITE: the assemble against the laid-out offsets and out_cap.  The inner coder runs in
// PACK_SIZE alone: the write half copies what it left in the library's arena.
static void launch_stall_press_packed(int stall_method, const StallPlan &p, const BatchArgs &a, const PackArgs &pk, int phases, hipStream_t s)
{
	const StallBufs b = p.bufs();
	if (phases & PACK_SIZE) {
		launch_stall_pieces(stall_method, p, a, s);
		launch_stall_sizes(stall_method, a.nsamp, a.nreads, b, pk.need, s);
		if (pk.layout)
			launch_pack_scan(pk, a.nreads, s);
	}
	if (phases & PACK_WRITE)
		launch_stall_assemble_packed(stall_method, a.nsamp, a.nreads, b, a.out, pk.slot, pk.out_cap, a.out_len, s);
}

int ph::launch_stall_depress(const StallPlan &p, const DecodeArgs &a, hipStream_t s)
{
	const StallBufs b = p.bufs();
	launch_stall_parse(a.in, a.in_off, a.in_len, a.nsamp, a.nreads, b, s);
	DecodeArgs in;
	p.inner.bind(in);
	in.nreads = p.npieces;
	in.in = a.in;
	in.in_off = b.pooff;
	in.in_len = b.polen;
	in.sig = b.psig;
	in.off = b.poff;
	in.nsamp = b.pn;
	in.out_n = b.poutn;
	const Method &m = METHODS[PRESS_HIP_RCCM_VBBE21_ZD];
	launch_ex_decode_chunked(in, m.exfmt, m.ent, s);
	launch_stall_scatter(a.sig, a.off, a.nsamp, a.nreads, b, a.out_n, s);
	return launch_status();
}

static bool rank_ok(uint32_t num, uint32_t den) { return den > 0 && num <= den; }

bool ph::scale_rule_ok(const press_hip_scale_rule *rule)
{
	return rank_ok(rule->lo_num, rule->lo_den) && rank_ok(rule->hi_num, rule->hi_den) && std::isfinite(rule->shift_mul) &&
	       std::isfinite(rule->shift_min) && std::isfinite(rule->scale_mul) && std::isfinite(rule->scale_min) && rule->scale_min > 0.0f;
}

// shift = max(shift_min, shift_mul * (float) (q_lo + q_hi)), scale = max(scale_min, scale_mul * (float) (q_hi - q_lo)) in
// single precision, every product rounded before it is compared (volatile: whatever the compiler is told about contraction
// or excess precision); cal = { -shift, 1 / scale }
extern "C" int press_hip_scale_cal(const int32_t *q, uint32_t nreads, const press_hip_scale_rule *rule, float *cal)
{
	if (!rule || (nreads && (!q || !cal)))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (!scale_rule_ok(rule))
		return set_error(PRESS_HIP_EARG, "the scale rule is not valid (ranks num <= den, den > 0; finite floats; scale_min > 0)");
	for (uint32_t r = 0; r < nreads; r++) {
		const int32_t lo = q[2 * (size_t) r], hi = q[2 * (size_t) r + 1];
		volatile float sh = rule->shift_mul * (float) ((int64_t) lo + hi);
		volatile float sc = rule->scale_mul * (float) ((int64_t) hi - lo);
		const float shift = fmaxf(rule->shift_min, sh), scale = fmaxf(rule->scale_min, sc);
		cal[2 * (size_t) r] = -shift;
		cal[2 * (size_t) r + 1] = 1.0f / scale;
	}
	return 0;
}

// rows of a read of c samples: 0, 1, or 1 + ceil((c - T) / S)
uint64_t ph::chunk_rows_of(uint32_t c, uint32_t T, uint32_t S)
{
	return c == 0 ? 0 : c <= T ? 1 : 1 + ((uint64_t) (c - T) + S - 1) / S;
}

extern "C" int press_hip_chunk_plan(const uint32_t *n, uint32_t nreads, uint32_t T, uint32_t overlap, uint64_t *row_first,
				    uint32_t *row_read, uint32_t *row_start)
{
	if (T == 0 || T % 8 || overlap >= T)
		return set_error(PRESS_HIP_EARG, "T must be a positive multiple of 8 and overlap below T");
	if (!row_first || (nreads && !n))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	const uint32_t S = T - overlap;
	uint64_t at = 0;
	for (uint32_t r = 0; r < nreads; r++) {
		row_first[r] = at;
		const uint64_t k = chunk_rows_of(n[r], T, S);
		for (uint64_t j = 0; j < k; j++) {
			if (row_read)
				row_read[at + j] = r;
			if (row_start)
				row_start[at + j] = j + 1 == k && n[r] > T ? n[r] - T : (uint32_t) (j * S);
		}
		at += k;
	}
	row_first[nreads] = at;
	return 0;
}

// c0 = (float) -med, c1 = 1 / ((float) mad * 1.4826f) in single precision, the product rounded before the division
// (volatile: whatever the compiler is told about contraction or excess precision); 1 for mad = 0
extern "C" int press_hip_norm_cal(const int32_t *stats, uint32_t nreads, float *cal)
{
	if (nreads && (!stats || !cal))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	for (uint32_t r = 0; r < nreads; r++) {
		const int32_t med = stats[2 * (size_t) r], mad = stats[2 * (size_t) r + 1];
		volatile float scale = (float) mad * 1.4826f;
		cal[2 * (size_t) r] = (float) -(int64_t) med;
		cal[2 * (size_t) r + 1] = mad > 0 ? 1.0f / scale : 1.0f;
	}
	return 0;
}

extern "C" int press_hip_depress_pa_fused(int method) { return depress_pa_fused(method) ? 1 : 0; }

// cal[2r] = (float) offset, cal[2r + 1] = (float) range / (float) digitisation: the reference's casts and its
// single-precision division (sigtk misc.c:17-26)
extern "C" int press_hip_pa_cal(const double *dor, uint32_t nreads, float *cal)
{
	if (nreads && (!dor || !cal))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	for (uint32_t r = 0; r < nreads; r++) {
		const float dig = (float) dor[3 * (size_t) r], rng = (float) dor[3 * (size_t) r + 2];
		cal[2 * (size_t) r] = (float) dor[3 * (size_t) r + 1];
		cal[2 * (size_t) r + 1] = rng / dig;
	}
	return 0;
}

extern "C" int press_hip_packed_exact(int method) { return method_ok(method) && !packed_is_bound(method_row(method)) ? 1 : 0; }

extern "C" int press_hip_recode_fused(int src_method, int dst_method) { return recode_fused(src_method, dst_method) ? 1 : 0; }

// The id the generic calls take for stage_layout_zd: the public id of the three pairs that have one, else the extended id
extern "C" int press_hip_xmethod(int stage, int layout)
{
	if (stage < 0 || stage >= PRESS_HIP_NXSTAGES || !rice_ok(layout))
		return -1;
	const Method &m = xstage_row(stage, layout);
	return public_ok(m.id) && &m == &METHODS[m.id] ? m.id : PRESS_HIP_XMETHOD_BASE + 4 * stage + layout;
}

extern "C" int press_hip_xmethod_parts(int id, int *stage, int *layout)
{
	if (!stage || !layout)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (!(public_ok(id) || xmethod_ok(id)) || (public_ok(id) && id < PRESS_HIP_RC_VBE21_ZD))
		return set_error(PRESS_HIP_EARG, "method %d is not a stage_layout_zd method of the families", id);
	const Method &m = method_row(id);
	*stage = m.ent == ENT_RC ? PRESS_HIP_XSTAGE_RC : m.ent == ENT_RCC ? PRESS_HIP_XSTAGE_RCC : m.ent == ENT_RCM ? PRESS_HIP_XSTAGE_RCCM
		 : m.ent == ENT_CDF ? PRESS_HIP_XSTAGE_RCCDF : m.ent == ENT_RICE ? PRESS_HIP_XSTAGE_RICE : PRESS_HIP_XSTAGE_HUFFMAN;
	*layout = (int) m.exfmt;
	return 0;
}

// The id the generic calls take for a stall method, and back
extern "C" int press_hip_smethod(int stall_method) { return stall_ok(stall_method) ? PRESS_HIP_SMETHOD_BASE + stall_method : -1; }

extern "C" int press_hip_smethod_parts(int id, int *stall_method)
{
	if (!stall_method)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (!smethod_ok(id))
		return set_error(PRESS_HIP_EARG, "method %d is not a stall method's id", id);
	*stall_method = method_row(id).stall;
	return 0;
}

int ph::check_method(int method)
{
	if (!method_ok(method))
		return set_error(PRESS_HIP_EARG, "method %d is not available in the batch API", method);
	if (is_shuff(method_row(method)) && !g.have_table)
		return set_error(PRESS_HIP_ENOTABLE, "static-Huffman method without a table (press_hip_load_table_file)");
	return 0;
}

int ph::launch_status()
{
	hipError_t e = hipGetLastError();
	return e == hipSuccess ? 0 : set_error(PRESS_HIP_EHIP, "kernel launch: %s", hipGetErrorString(e));
}

int ph::launch_press(const ScratchPlan &p, const BatchArgs &a, hipStream_t s)
{
	const Method &m = *p.m;
	if (m.family == FAM_SVB) {
		launch_svb_encode_chunked(a, m.key2, m.zd, s, m.slow5);
	} else if (m.family == FAM_EX) {
		launch_ex_encode_chunked(a, m.exfmt, m.ent, s);
	} else if (m.family == FAM_STALL) {
		return launch_stall_press(m.stall, stall_plan_of(p), a, nullptr, s);
	} else {
		const ZsBufs z = p.zs();
		launch_zstd_encode(a, z, s);
	}
	return launch_status();
}

int ph::launch_press_packed(const ScratchPlan &p, const BatchArgs &a, const PackArgs &pk, int phases, hipStream_t s)
{
	const Method &m = *p.m;
	if (m.family == FAM_SVB) {
		launch_svb_encode_packed(a, m.key2, m.zd, m.slow5, pk, phases, s);
	} else if (m.family == FAM_EX) {
		launch_ex_encode_packed(a, m.exfmt, m.ent, pk, phases, s);
	} else if (m.family == FAM_STALL) {
		launch_stall_press_packed(m.stall, stall_plan_of(p), a, pk, phases, s);
	} else {
		const ZsBufs z = p.zs();
		launch_zstd_encode_packed(a, z, pk, phases, s);
	}
	return launch_status();
}

// Frames the device walk leaves to libzstd (dictionaries, 12-bit tables, several frames in one stream ...): their
// content is made on the host and put where the device would have put it.  How many there are comes back through a
// page-locked word behind an event (zs_count_host_frames, queued between the two stages of a batch): the host waits for
// that word only, while the device already runs the second stage - a batch of this library's own frames, or of
// ZSTD_compress's, has no such frame and is never waited for; with one, the second stage is run again (*patched).
static int zs_count_host_frames(const ZsBufs &z, hipStream_t s)
{
	if (!g.zs_pin) {
		HIPCHK(hipHostMalloc((void **) &g.zs_pin, 64, hipHostMallocDefault));
		HIPCHK(hipEventCreateWithFlags(&g.zs_ev, hipEventDisableTiming));
	}
	HIPCHK(hipMemcpyAsync(g.zs_pin, &z.dctl->nhost, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	HIPCHK(hipEventRecord(g.zs_ev, s));
	return 0;
}
static int zs_host_frames(const DecodeArgs &a, const ZsBufs &z, hipStream_t s, bool *patched)
{
	*patched = false;
	HIPCHK(hipEventSynchronize(g.zs_ev));
	const uint32_t nhost = *g.zs_pin;
	g.zs_nhost = nhost;
	if (!nhost || !zstd_open())
		return 0; // without libzstd those reads fail
	HIPCHK(hipStreamSynchronize(s)); // (the second stage is running on what the device had)
	*patched = true;
	const uint32_t nr = a.nreads;
	std::vector<ZsRead> rd(nr);
	std::vector<uint64_t> ioff(nr), ilen(nr), zoff(nr + 1);
	std::vector<uint32_t> caps(nr);
	HIPCHK(hipMemcpy(rd.data(), z.rd, (size_t) nr * sizeof(ZsRead), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(ioff.data(), a.in_off, (size_t) nr * 8, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(ilen.data(), a.in_len, (size_t) nr * 8, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(zoff.data(), z.zoff, ((size_t) nr + 1) * 8, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(caps.data(), a.nsamp, (size_t) nr * 4, hipMemcpyDeviceToHost));
	std::vector<uint8_t> frame, buf;
	for (uint32_t r = 0; r < nr; r++) {
		if (rd[r].mode != 3)
			continue;
		uint64_t cap;
		if (z.kdiv) {
			cap = 4ull + (caps[r] + (uint64_t) z.kdiv - 1) / z.kdiv + 2ull * caps[r];
		} else { // device: zs_content_max
			const uint64_t vb = bound_vbzd(caps[r] ? caps[r] : 1);
			cap = (vb + 3) / 4 + vb * 4 + 16;
		}
		frame.resize(ilen[r] + 8);
		buf.resize(cap + 8);
		HIPCHK(hipMemcpy(frame.data(), a.in + ioff[r], ilen[r], hipMemcpyDeviceToHost));
		const size_t got = zstd_fn.decompress(buf.data(), cap, frame.data(), ilen[r]);
		if (zstd_fn.is_error(got)) {
			rd[r].mode = 2;
			continue;
		}
		HIPCHK(hipMemcpy(z.ztmp + zoff[r], buf.data(), got, hipMemcpyHostToDevice));
		rd[r].mode = 0;
		rd[r].nd = (uint32_t) got;
		rd[r].knz = 0; // (a Content_Checksum: libzstd has verified it)
	}
	HIPCHK(hipMemcpy(z.rd, rd.data(), (size_t) nr * sizeof(ZsRead), hipMemcpyHostToDevice));
	return 0;
}

int ph::launch_depress_pa(const ScratchPlan &p, const DecodeArgs &a, float *pa, const float *cal, hipStream_t s)
{
	const Method &m = *p.m;
	if (m.family == FAM_SVB) { // (depress_pa_fused)
		launch_svb_decode_pa(a, pa, cal, m.key2, m.zd, m.slow5, s);
		return launch_status();
	}
	const int rc = launch_depress(p, a, s);
	if (rc)
		return rc;
	launch_pa_convert(a, pa, cal, (uint2 *) p.ptr(&Ctx::pa_tile), (uint32_t *) p.ptr(&Ctx::pa_ctl), s);
	return launch_status();
}

int ph::launch_depress_norm(const ScratchPlan &p, const DecodeArgs &a, float *out, int32_t *stats, hipStream_t s)
{
	const int rc = launch_depress(p, a, s);
	if (rc)
		return rc;
	uint2 *tiles = (uint2 *) p.ptr(&Ctx::pa_tile);
	uint32_t *ntiles = (uint32_t *) p.ptr(&Ctx::pa_ctl);
	float *cal = (float *) p.ptr(&Ctx::st_cal);
	launch_pa_tiles(a, tiles, ntiles, s);
	launch_signal_stats(a, tiles, ntiles, p.ptr(&Ctx::st_read), (uint32_t *) p.ptr(&Ctx::st_rows), stats, cal, nullptr, s);
	launch_pa_apply(a, out, cal, tiles, ntiles, s);
	return launch_status();
}

// The decode, the tile table, the calibration (a rule: two quantiles in four launches; none: median and MAD in eight),
// the row writer.
int ph::launch_depress_chunks(const ScratchPlan &p, const DecodeArgs &a, const ChunkArgs &c, hipStream_t s)
{
	const int rc = launch_depress(p, a, s);
	if (rc)
		return rc;
	uint2 *tiles = (uint2 *) p.ptr(&Ctx::pa_tile);
	uint32_t *ntiles = (uint32_t *) p.ptr(&Ctx::pa_ctl);
	float *cal = (float *) p.ptr(&Ctx::st_cal);
	launch_pa_tiles(a, tiles, ntiles, s);
	if (c.rule) {
		const uint32_t num[2] = { c.rule->lo_num, c.rule->hi_num }, den[2] = { c.rule->lo_den, c.rule->hi_den };
		const ScaleRule ru = { c.rule->shift_mul, c.rule->shift_min, c.rule->scale_mul, c.rule->scale_min };
		launch_signal_quantiles(a, tiles, ntiles, p.ptr(&Ctx::st_read), (uint32_t *) p.ptr(&Ctx::st_rows), num, den, 2, c.q, cal, &ru, s);
	} else {
		launch_signal_stats(a, tiles, ntiles, p.ptr(&Ctx::st_read), (uint32_t *) p.ptr(&Ctx::st_rows), c.q, cal, nullptr, s);
	}
	launch_chunk_rows(a, cal, c.row_first, c.rows, c.nrows_cap, c.dtype, c.T, c.overlap, c.total_samples, s);
	return launch_status();
}

// The decode and the tile table; the detector of the mode over the decoded counts; the cuts and the row plan; the
// calibration over the cuts (launch_depress_chunks' two ways, ranged); the ranged row writer.  Nothing waits for the host
// beyond what launch_depress does for the zstd kinds.
int ph::launch_depress_chunks_trimmed(const ScratchPlan &p, const DecodeArgs &a, const ChunkArgs &c, const TrimArgs &t, hipStream_t s)
{
	const int rc = launch_depress(p, a, s);
	if (rc)
		return rc;
	uint2 *tiles = (uint2 *) p.ptr(&Ctx::pa_tile);
	uint32_t *ntiles = (uint32_t *) p.ptr(&Ctx::pa_ctl);
	float *cal = (float *) p.ptr(&Ctx::st_cal);
	uint32_t *cut = (uint32_t *) p.ptr(&Ctx::tr_cut);
	void *det = p.ptr(&Ctx::tr_det);
	launch_pa_tiles(a, tiles, ntiles, s);
	if (t.mode != PRESS_TRIM_RANGE) {
		uint32_t *cnt = (uint32_t *) p.ptr(&Ctx::tr_cnt);
		launch_trim_counts(a, cnt, s);
		if (t.mode == PRESS_TRIM_ADAPTOR)
			launch_adaptor(a.sig, a.off, cnt, a.nreads, t.adaptor, (int32_t *) det, nullptr, s);
		else
			launch_segments_first(a.sig, a.off, cnt, a.nreads, t.seg, p.ptr(&Ctx::sg_state), det, s, t.seg_cal);
	}
	launch_trim_plan(a, t.mode, t.range, det, t.min_keep, c.T, c.overlap, cut, t.cut, (uint64_t *) p.ptr(&Ctx::pneed),
			 (uint64_t *) p.ptr(&Ctx::pslot), (uint64_t *) c.row_first, s);
	if (c.rule) {
		const uint32_t num[2] = { c.rule->lo_num, c.rule->hi_num }, den[2] = { c.rule->lo_den, c.rule->hi_den };
		const ScaleRule ru = { c.rule->shift_mul, c.rule->shift_min, c.rule->scale_mul, c.rule->scale_min };
		launch_signal_quantiles_ranged(a, cut, tiles, ntiles, p.ptr(&Ctx::st_read), (uint32_t *) p.ptr(&Ctx::st_rows), num, den, 2, c.q, cal,
					       &ru, s);
	} else {
		launch_signal_stats_ranged(a, cut, tiles, ntiles, p.ptr(&Ctx::st_read), (uint32_t *) p.ptr(&Ctx::st_rows), c.q, cal, s);
	}
	launch_chunk_rows_ranged(a, cut, cal, c.row_first, c.rows, c.nrows_cap, c.dtype, c.T, c.overlap, c.total_samples, t.row_read, t.row_start, s);
	return launch_status();
}

// The tile table of the rooms, then the digest of the a.out_n[r] samples at a.sig
int ph::launch_signal_crc(const ScratchPlan &p, const DecodeArgs &a, uint32_t *crc, hipStream_t s)
{
	uint2 *tiles = (uint2 *) p.ptr(&Ctx::pa_tile);
	uint32_t *ntiles = (uint32_t *) p.ptr(&Ctx::pa_ctl);
	launch_pa_tiles(a, tiles, ntiles, s);
	launch_crc(a, tiles, ntiles, (uint32_t *) p.ptr(&Ctx::vf_raw), crc, s);
	return launch_status();
}

int ph::launch_depress_crc(const ScratchPlan &p, const DecodeArgs &a, uint32_t *crc, hipStream_t s)
{
	const int rc = launch_depress(p, a, s);
	return rc ? rc : launch_signal_crc(p, a, crc, s);
}

int ph::launch_verify(const ScratchPlan &p, const DecodeArgs &a, const int16_t *sig, uint32_t *first_bad, uint32_t *nbad, hipStream_t s,
		      uint32_t bits)
{
	const int rc = launch_depress(p, a, s);
	if (rc)
		return rc;
	uint2 *tiles = (uint2 *) p.ptr(&Ctx::pa_tile);
	uint32_t *ntiles = (uint32_t *) p.ptr(&Ctx::pa_ctl);
	launch_pa_tiles(a, tiles, ntiles, s);
	launch_verify_cmp(a, sig, tiles, ntiles, first_bad, nbad, s, bits);
	return launch_status();
}

int ph::launch_depress(const ScratchPlan &p, const DecodeArgs &a, hipStream_t s)
{
	const Method &m = *p.m;
	if (m.family == FAM_SVB) {
		launch_svb_decode_chunked(a, m.key2, m.zd, s, m.slow5);
	} else if (m.family == FAM_EX) {
		launch_ex_decode_chunked(a, m.exfmt, m.ent, s);
	} else if (m.family == FAM_STALL) {
		return launch_stall_depress(stall_plan_of(p), a, s);
	} else {
		const ZsBufs z = p.zs();
		launch_zstd_decode_frames(a, z, s);
		int rc = zs_count_host_frames(z, s);
		if (rc)
			return rc;
		launch_zstd_decode_streams(a, z, s);
		bool patched;
		if ((rc = zs_host_frames(a, z, s, &patched)))
			return rc;
		if (patched)
			launch_zstd_decode_streams(a, z, s);
	}
	return launch_status();
}
