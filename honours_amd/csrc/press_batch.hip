// press_batch.hip - the batch entry points of include/press_hip.h.  Every one reads the same way: the checks that need
// no device, the device and the method's table, the empty batch, the scratch plan, the caller's I/O - its own pointers
// (device resident) or what a Staged call returns for them (press_staging.hip) - ONE launch, and for a staged call the
// copies back and the synchronisation.

#include <limits.h>

#include <algorithm>

#include "press_host.h"

using namespace ph;

// ------------------------------------------------------------------ the head of every entry point

constexpr int NONE = INT_MIN; // in the place of a method id: the call has no (second) method

// The checks that need no device, the same with and without a GPU: the method ids, a NULL among the arguments (the
// caller's test: pointers of a non-empty batch), and for a device-resident call the 16-byte alignment of its sample /
// float / row arena `dev_arena` (NULL for a host-pointer call; an empty batch touches nothing and is not checked).
static int args_ok(int m1, int m2, bool null_arg, uint32_t nreads, const void *dev_arena, const char *arena_name)
{
	if (m2 != NONE && (!method_ok(m1) || !method_ok(m2)))
		return set_error(PRESS_HIP_EARG, "method %d -> %d is not available in the batch API", m1, m2);
	if (m2 == NONE && m1 != NONE && !method_ok(m1))
		return set_error(PRESS_HIP_EARG, "method %d is not available in the batch API", m1);
	if (null_arg)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (nreads && ((uintptr_t) dev_arena & 15))
		return set_error(PRESS_HIP_EARG, "%s must be 16-byte aligned", arena_name);
	return 0;
}

// The parameter checks of the two detectors, for every call that takes their parameters (segments, adaptor, prefix, the
// trimmed chunk rows): 0, or EARG with the text in last_error
static int jnn_params_ok(const press_hip_jnn_params &p)
{
	if (p.window < 1 || p.corrector < 0 || p.error < 0 || p.seg_dist < 0 || !std::isfinite(p.stall_len))
		return set_error(PRESS_HIP_EARG, "jnn parameters: window %d >= 1, corrector %d, error %d, seg_dist %d >= 0, a finite stall_len",
				 p.window, p.corrector, p.error, p.seg_dist);
	return 0;
}

static int jnn2_params_ok(const press_hip_jnn2_params &p)
{
	if (p.window < 1 || p.window > 8192)
		return set_error(PRESS_HIP_EARG, "window = %d: 1 .. 8192 (the window sums stay below 2^24)", p.window);
	return 0;
}

static int align_ok(uint32_t align)
{
	if (align == 0 || align > 4096 || (align & (align - 1)))
		return set_error(PRESS_HIP_EARG, "align = %u is not a power of two in 1 .. 4096", align);
	return 0;
}

// ... then the device, then the methods' tables (ENOTABLE)
static int device_ready(int m1, int m2)
{
	int rc = ctx_init();
	if (!rc && m1 != NONE)
		rc = check_method(m1);
	if (!rc && m2 != NONE)
		rc = check_method(m2);
	return rc;
}

// ------------------------------------------------------------------ the caller's I/O into the argument blocks

static void bind_io(BatchArgs &a, const SamplesIn &i)
{
	a.sig = i.sig;
	a.off = i.off;
	a.nsamp = i.n;
}

static void bind_io(BatchArgs &a, const SlotsOut &o)
{
	a.out = o.out;
	a.out_off = o.out_off;
	a.out_len = o.out_len;
}

static void bind_io(DecodeArgs &a, const StreamsIn &i)
{
	a.in = i.in;
	a.in_off = i.in_off;
	a.in_len = i.in_len;
	a.sig = i.sig;
	a.off = i.off;
	a.nsamp = i.n;
	a.out_n = i.out_n;
}

// samples that a decoder's successor reads in place (the stats calls): every sample of a read counts; nothing is written
static void bind_io(DecodeArgs &a, const SamplesIn &i)
{
	a.sig = const_cast<int16_t *>(i.sig);
	a.off = i.off;
	a.nsamp = i.n;
	a.out_n = const_cast<uint32_t *>(i.n);
}

// ------------------------------------------------------------------ press

extern "C" int press_hip_press_batch(int method, const int16_t *sig, const uint64_t *off, const uint32_t *n,
				     uint32_t nreads, uint64_t total_samples, uint8_t *out,
				     const uint64_t *out_off, uint64_t *out_len, int device_resident)
{
	API_LOCK;
	int rc = args_ok(method, NONE, nreads && (!sig || !off || !n || !out || !out_off || !out_len), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(method, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_plan(method, total_samples, nreads, false);
	if ((rc = plan.reserve()))
		return rc;
	BatchArgs a;
	plan.bind(a);
	a.nreads = nreads;
	const SlotsOut host = { out, out_off, out_len };
	SamplesIn in = { sig, off, n };
	SlotsOut so = host;
	Staged st(nreads, s);
	// host pointers: stage, run, copy back, synchronise (the slots' table goes up before the samples: samples_in in two steps)
	if (!device_resident && ((rc = check_slots(out_off, nreads)) || (rc = st.layout(off, n, total_samples, "the sample range", true)) ||
				 (rc = st.slots(host, so)) || (rc = st.samples(in, total_samples, in))))
		return rc;
	bind_io(a, in);
	bind_io(a, so);
	if ((rc = launch_press(plan, a, s)) || device_resident)
		return rc;
	return st.fetch_streams(host);
}

// ------------------------------------------------------------------ packed press: the library lays the arena out

// An empty packed batch has a layout too
static int packed_empty(uint64_t *out_off, int device_resident)
{
	if (device_resident)
		HIPCHK(hipMemsetAsync(out_off, 0, 8, g.stream()));
	else
		out_off[0] = 0;
	return 0;
}

// Everything a host-pointer packed call does behind its size phase's launch, up to the copy of the arena: the layout
// read back, the arena's size, an arena of that size, the write phase (`write`: the call's launch with PACK_WRITE;
// a.out is the arena by then), out_len, the arena's prefix back in one piece.  Not synchronised at the end.
template <class Write>
static int packed_tail(Staged &st, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *out_len, BatchArgs &a,
		       const PackArgs &pk, Write write)
{
	int rc;
	const uint32_t nreads = st.nreads;
	HIPCHK(hipMemcpyAsync(out_off, pk.layout, ((size_t) nreads + 1) * 8, hipMemcpyDeviceToHost, st.s));
	HIPCHK(hipStreamSynchronize(st.s)); // the one synchronisation besides the last: the arena's size
	const uint64_t bytes = out_off[nreads] < out_cap ? out_off[nreads] : out_cap; // what a read that fits can touch
	if (g.arena.reserve(bytes + 64))
		return PRESS_HIP_EHIP;
	// (padding and the gaps of the range coders travel with the streams: they reach the caller as zeros)
	if (bytes)
		HIPCHK(hipMemsetAsync(g.arena.p, 0, bytes, st.s));
	bind_io(a, SlotsOut{ (uint8_t *) g.arena.p, pk.slot, (uint64_t *) g.lens.p });
	if ((rc = write()))
		return rc;
	HIPCHK(hipMemcpyAsync(out_len, g.lens.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, st.s));
	return st.fetch_prefix(out, g.arena.p, bytes);
}

extern "C" int press_hip_press_sizes(int method, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				     uint64_t total_samples, uint64_t *need, int device_resident)
{
	API_LOCK;
	int rc = args_ok(method, NONE, nreads && (!sig || !off || !n || !need), nreads, device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(method, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_packed_plan(method, total_samples, nreads);
	if ((rc = plan.reserve()))
		return rc;
	BatchArgs a;
	plan.bind(a);
	a.nreads = nreads;
	const PackArgs pk = { device_resident ? need : (uint64_t *) g.pneed.p, nullptr, (uint64_t *) g.pslot.p, 0, 1 };
	SamplesIn in = { sig, off, n };
	Staged st(nreads, s);
	if (!device_resident && (rc = st.samples_in(in, total_samples, in)))
		return rc;
	bind_io(a, in);
	bind_io(a, SlotsOut{ nullptr, pk.slot, pk.need }); // (need: an empty read's verdict of k_chunk_prep; the size kernel has the last word)
	if ((rc = launch_press_packed(plan, a, pk, PACK_SIZE, s)) || device_resident)
		return rc;
	return st.fetch_tables({ { need, pk.need, (size_t) nreads * 8 } });
}

extern "C" int press_hip_press_packed(int method, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				      uint64_t total_samples, uint8_t *out, uint64_t out_cap, uint32_t align,
				      uint64_t *out_off, uint64_t *out_len, int device_resident)
{
	API_LOCK;
	int rc = args_ok(method, NONE, !out_off || (nreads && (!sig || !off || !n || !out_len || (!out && out_cap))), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc || (rc = align_ok(align)) || (rc = device_ready(method, NONE)))
		return rc;
	if (nreads == 0)
		return packed_empty(out_off, device_resident);
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_packed_plan(method, total_samples, nreads);
	if ((rc = plan.reserve()))
		return rc;
	BatchArgs a;
	plan.bind(a);
	a.nreads = nreads;
	PackArgs pk = { (uint64_t *) g.pneed.p, out_off, (uint64_t *) g.pslot.p, out_cap, align };
	SamplesIn in = { sig, off, n };
	SlotsOut so = { out, pk.slot, out_len };
	Staged st(nreads, s);
	if (!device_resident) {
		// host pointers: stage, size and lay out, read the arena's size back, press into an arena of that size, copy its
		// prefix back in one piece
		if (g.arena_off.reserve(((size_t) nreads + 1) * 8) || g.lens.reserve((size_t) nreads * 8))
			return PRESS_HIP_EHIP;
		pk.layout = (uint64_t *) g.arena_off.p;
		so = { nullptr, pk.slot, (uint64_t *) g.lens.p };
		if ((rc = st.samples_in(in, total_samples, in)))
			return rc;
	}
	bind_io(a, in);
	bind_io(a, so);
	if ((rc = launch_press_packed(plan, a, pk, device_resident ? PACK_SIZE | PACK_WRITE : PACK_SIZE, s)) || device_resident)
		return rc;
	if ((rc = packed_tail(st, out, out_cap, out_off, out_len, a, pk, [&] { return launch_press_packed(plan, a, pk, PACK_WRITE, s); })))
		return rc;
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

#ifndef TRAIN_WG_PER_CU
#define TRAIN_WG_PER_CU 2 // workgroups per CU of k_symbol_count's persistent grid
#endif

extern "C" int press_hip_symbol_counts(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				       uint64_t total_samples, uint64_t *counts, int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, nreads && (!sig || !off || !n || !counts), nreads, device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const uint32_t mc = make_tiles_plan(total_samples, nreads).max_chunks; // (the buffers are its own, below)
	int cus = 0;
	HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g.device));
	const uint32_t grid = (uint32_t) std::max(cus, 1) * TRAIN_WG_PER_CU;
	if (g.chunks.reserve(train_scratch_bytes(mc)) || g.ctl.reserve(2 * sizeof(ChunkCtl)))
		return PRESS_HIP_EHIP;
	uint32_t *nchunks = &((ChunkCtl *) g.ctl.p)->nchunks;
	SamplesIn in = { sig, off, n };
	uint64_t *sum = counts;
	uint64_t nch = mc; // chunks with something to count; the host form knows the number
	Staged st(nreads, s);
	if (!device_resident) { // host pointers: stage, run, copy the counts back, synchronise (reads may overlap)
		if ((rc = st.layout(off, n, total_samples, nullptr, true)))
			return rc;
		nch = 0;
		for (uint32_t r = 0; r < nreads; r++)
			nch += n[r] >= 2 ? (n[r] + CHUNK - 1) / CHUNK : 0;
		if (nch == 0)
			return 0;
		if (g.lens.reserve(257 * 8))
			return PRESS_HIP_EHIP;
		sum = (uint64_t *) g.lens.p;
		HIPCHK(hipMemcpyAsync(sum, counts, 257 * 8, hipMemcpyHostToDevice, s));
		if ((rc = st.samples(in, total_samples, in)))
			return rc;
	}
	launch_symbol_counts(in.sig, in.off, in.n, nreads, sum, g.chunks.p, nchunks, mc, (uint32_t) std::min<uint64_t>(grid, nch), s);
	if ((rc = launch_status()) || device_resident)
		return rc;
	return st.fetch_tables({ { counts, sum, 257 * 8 } });
}

// ------------------------------------------------------------------ dataset analysis: tallies and moments

extern "C" int press_hip_signal_tally(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				      uint64_t total_samples, uint64_t *raw, uint64_t *delta, uint64_t *trans,
				      press_hip_moments *mom, int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, nreads && (!sig || !off || !n), nreads, device_resident ? sig : nullptr, "sig");
	if (rc)
		return rc;
	if (!device_resident && nreads && (rc = check_layout(off, n, nreads, total_samples)))
		return rc;
	if (nreads == 0 || (!raw && !delta && !trans && !mom))
		return 0;
	if ((rc = device_ready(NONE, NONE)))
		return rc;
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_tally_plan(total_samples, nreads, !device_resident);
	uint32_t mc = plan.max_chunks;
	if (!device_resident) { // the host form knows the number of chunks: reads that overlap may need more than the plan's
		uint64_t nch = 0;
		for (uint32_t r = 0; r < nreads; r++)
			nch += n[r] / CHUNK + (n[r] % CHUNK != 0);
		if (nch > 0xFFFFFFFFull)
			return set_error(PRESS_HIP_EARG, "%llu chunks of samples: at most 2^32 - 1", (unsigned long long) nch);
		mc = std::max(mc, (uint32_t) nch);
	}
	if ((rc = plan.reserve()) || g.tl_chunks.reserve(tally_scratch_bytes(mc)))
		return rc ? rc : PRESS_HIP_EHIP;
	int cus = 0;
	HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g.device));
	const uint32_t ncu = (uint32_t) std::max(cus, 1);
	uint32_t *nchunks = (uint32_t *) g.tl_ctl.p;
	if (device_resident) {
		launch_signal_tally(sig, off, n, nreads, raw, delta, trans, mom, g.tl_chunks.p, nchunks, mc, ncu, s);
		return launch_status();
	}
	// host pointers: stage the samples and the caller's tables, run, copy the tables and the moments back, synchronise
	uint64_t *const d_raw = (uint64_t *) g.tl_tab.p, *const d_delta = d_raw + PRESS_HIP_TALLY_BINS, *const d_trans = d_delta + PRESS_HIP_TALLY_BINS;
	const size_t bins = (size_t) PRESS_HIP_TALLY_BINS * 8, cells = (size_t) PRESS_HIP_TALLY_SYMS * PRESS_HIP_TALLY_SYMS * 8;
	SamplesIn in = { sig, off, n };
	Staged st(nreads, s);
	if ((rc = st.layout(off, n, total_samples, nullptr, true)))
		return rc;
	if (raw)
		HIPCHK(hipMemcpyAsync(d_raw, raw, bins, hipMemcpyHostToDevice, s));
	if (delta)
		HIPCHK(hipMemcpyAsync(d_delta, delta, bins, hipMemcpyHostToDevice, s));
	if (trans)
		HIPCHK(hipMemcpyAsync(d_trans, trans, cells, hipMemcpyHostToDevice, s));
	if ((rc = st.samples(in, total_samples, in)))
		return rc;
	launch_signal_tally(in.sig, in.off, in.n, nreads, raw ? d_raw : nullptr, delta ? d_delta : nullptr, trans ? d_trans : nullptr,
			    mom ? g.tl_mom.p : nullptr, g.tl_chunks.p, nchunks, mc, ncu, s);
	if ((rc = launch_status()))
		return rc;
	return st.fetch_tables({ { raw, d_raw, bins }, { delta, d_delta, bins }, { trans, d_trans, cells },
				 { mom, g.tl_mom.p, (size_t) nreads * sizeof(press_hip_moments) } });
}

// ------------------------------------------------------------------ depress: samples, picoamperes, normalised floats, chunk rows

// The depress of a method's row, behind the caller's argument check.  ready: the method id the device must be ready for
// (NONE: a row of a family with ids of its own)
static int row_depress(const Method &m, int ready, const StreamsIn &host, uint32_t nreads, uint64_t total_samples, int device_resident)
{
	int rc = device_ready(ready, NONE);
	if (rc)
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_plan(m, total_samples, nreads, true);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;
	StreamsIn io = host;
	Staged st(nreads, s);
	if (!device_resident && (rc = st.streams(host, total_samples, true, g.arena, g.arena_off, io)))
		return rc;
	bind_io(a, io);
	if ((rc = launch_depress(plan, a, s)) || device_resident)
		return rc;
	return st.fetch_samples(host);
}

extern "C" int press_hip_depress_batch(int method, const uint8_t *in, const uint64_t *in_off,
				       const uint64_t *in_len, uint32_t nreads, int16_t *sig,
				       const uint64_t *off, const uint32_t *n, uint64_t total_samples,
				       uint32_t *out_n, int device_resident)
{
	API_LOCK;
	const int rc = args_ok(method, NONE, nreads && (!in || !in_off || !in_len || !sig || !off || !n || !out_n), nreads,
			       device_resident ? sig : nullptr, "sig");
	return rc ? rc : row_depress(method_row(method), method, { in, in_off, in_len, off, n, out_n, sig }, nreads, total_samples, device_resident);
}

// Picoamperes: press_hip_depress_batch with the float arena `pa` in the place of sig.  A fused method's decode kernel
// writes the floats itself; the others decode into g.rsig and k_pa_convert follows (launch_depress_pa).
extern "C" int press_hip_depress_pa_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					  uint32_t nreads, float *pa, const uint64_t *off, const uint32_t *n,
					  uint64_t total_samples, const float *cal, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = args_ok(method, NONE, nreads && (!in || !in_off || !in_len || !pa || !off || !n || !cal || !out_n), nreads,
			 device_resident ? pa : nullptr, "pa");
	if (rc || (rc = device_ready(method, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_pa_plan(method, total_samples, nreads, !device_resident);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;
	// (sig: the samples' scratch; NULL for a fused method: its kernel has no use for it)
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, (int16_t *) plan.ptr(&Ctx::rsig) };
	StreamsIn io = host;
	Staged st(nreads, s);
	if (!device_resident) {
		if ((rc = st.streams(host, total_samples, false, g.arena, g.arena_off, io)))
			return rc;
		HIPCHK(hipMemcpyAsync(g.pa_cal.p, cal, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	}
	bind_io(a, io);
	if ((rc = launch_depress_pa(plan, a, device_resident ? pa : (float *) g.pa_out.p, device_resident ? cal : (const float *) g.pa_cal.p, s)) ||
	    device_resident)
		return rc;
	return st.fetch_elems(pa, g.pa_out.p, sizeof(float), host);
}

// Normalised floats: press_hip_depress_pa_batch's general path for every method, with a calibration the device derives
// between the decoder and the converter (launch_depress_norm).
extern "C" int press_hip_depress_norm_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					    uint32_t nreads, float *out, const uint64_t *off, const uint32_t *n,
					    uint64_t total_samples, int32_t *stats, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = args_ok(method, NONE, nreads && (!in || !in_off || !in_len || !out || !off || !n || !out_n), nreads,
			 device_resident ? out : nullptr, "out");
	if (rc || (rc = device_ready(method, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_norm_plan(method, total_samples, nreads, !device_resident);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, (int16_t *) plan.ptr(&Ctx::rsig) };
	StreamsIn io = host;
	Staged st(nreads, s);
	if (!device_resident && (rc = st.streams(host, total_samples, false, g.arena, g.arena_off, io)))
		return rc;
	bind_io(a, io);
	if ((rc = launch_depress_norm(plan, a, device_resident ? out : (float *) g.pa_out.p, device_resident ? stats : (int32_t *) g.st_stats.p, s)) ||
	    device_resident)
		return rc;
	if (stats)
		HIPCHK(hipMemcpyAsync(stats, g.st_stats.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	return st.fetch_elems(out, g.pa_out.p, sizeof(float), host);
}

// Chunk rows: press_hip_depress_norm_batch's decode and staging; the calibration is the rule's two quantiles or, without a
// rule, median and MAD; the writer of press_rows.hip takes the place of the float converter (launch_depress_chunks).
extern "C" int press_hip_depress_chunks_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					      uint32_t nreads, void *rows, uint64_t nrows_cap, int dtype, uint32_t T, uint32_t overlap,
					      const uint64_t *row_first, const uint64_t *off, const uint32_t *n, uint64_t total_samples,
					      const press_hip_scale_rule *rule, int32_t *q, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = args_ok(method, NONE, nreads && (!in || !in_off || !in_len || !row_first || !off || !n || !out_n || (!rows && nrows_cap)),
			 nreads, device_resident ? rows : nullptr, "rows");
	if (rc)
		return rc;
	if (dtype != PRESS_HIP_F32 && dtype != PRESS_HIP_F16 && dtype != PRESS_HIP_BF16)
		return set_error(PRESS_HIP_EARG, "dtype %d: PRESS_HIP_F32, PRESS_HIP_F16 or PRESS_HIP_BF16", dtype);
	if (T == 0 || T % 8 || overlap >= T)
		return set_error(PRESS_HIP_EARG, "T must be a positive multiple of 8 and overlap below T");
	if (rule && !scale_rule_ok(rule))
		return set_error(PRESS_HIP_EARG, "the scale rule is not valid (ranks num <= den, den > 0; finite floats; scale_min > 0)");
	if ((rc = device_ready(method, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const size_t es = dtype == PRESS_HIP_F32 ? 4 : 2;
	uint64_t written = 0;
	if (!device_resident) { // host pointers: row_first must be the plan of n[] (it decides what is written where)
		const uint32_t S = T - overlap;
		uint64_t at = 0;
		for (uint32_t r = 0; r < nreads; r++) {
			if (row_first[r] != at)
				return set_error(PRESS_HIP_EARG, "row_first[%u] is not press_hip_chunk_plan's", r);
			at += chunk_rows_of(n[r], T, S);
		}
		if (row_first[nreads] != at)
			return set_error(PRESS_HIP_EARG, "row_first[%u] is not press_hip_chunk_plan's", nreads);
		written = at < nrows_cap ? at : nrows_cap;
	}
	const ScratchPlan plan = make_chunks_plan(method, total_samples, nreads, !device_resident, written * T * es);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;
	ChunkArgs c = { rows, nrows_cap, dtype, T, overlap, row_first, total_samples, rule, q };
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, (int16_t *) plan.ptr(&Ctx::rsig) };
	StreamsIn io = host;
	Staged st(nreads, s);
	if (!device_resident) {
		if ((rc = st.streams(host, total_samples, false, g.arena, g.arena_off, io)))
			return rc;
		HIPCHK(hipMemcpyAsync(g.ch_first.p, row_first, ((size_t) nreads + 1) * 8, hipMemcpyHostToDevice, s));
		c.rows = g.ch_rows.p;
		c.nrows_cap = written;
		c.row_first = (const uint64_t *) g.ch_first.p;
		c.q = (int32_t *) g.st_stats.p;
	}
	bind_io(a, io);
	if ((rc = launch_depress_chunks(plan, a, c, s)) || device_resident)
		return rc;
	// one transfer of the written prefix of the rows, q and out_n, synchronise
	if (q)
		HIPCHK(hipMemcpyAsync(q, g.st_stats.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(out_n, g.outn.p, (size_t) nreads * 4, hipMemcpyDeviceToHost, s));
	if (written)
		HIPCHK(hipMemcpyAsync(rows, g.ch_rows.p, written * T * es, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// Trimmed chunk rows (include/press_hip.h 2y): the chunk call with a range per read - the caller's, or one a detector finds
// in the decoded samples - and the row plan made on the device (launch_depress_chunks_trimmed).  Host pointers: the
// rows of the untrimmed plan bound what can be written, so the arena and the row tables are staged at min(that,
// nrows_cap); row_first comes back first and says how much of them to fetch.
static_assert((int) PRESS_HIP_TRIM_RANGE == (int) PRESS_TRIM_RANGE && (int) PRESS_HIP_TRIM_ADAPTOR == (int) PRESS_TRIM_ADAPTOR &&
		      (int) PRESS_HIP_TRIM_SEGMENT == (int) PRESS_TRIM_SEGMENT,
	      "the trim modes");

extern "C" int press_hip_depress_chunks_trimmed_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
						      uint32_t nreads, void *rows, uint64_t nrows_cap, int dtype, uint32_t T, uint32_t overlap,
						      uint64_t *row_first, uint32_t *row_read, uint32_t *row_start, const uint64_t *off,
						      const uint32_t *n, uint64_t total_samples, const press_hip_trim *trim, const uint32_t *range,
						      const float *seg_cal, uint32_t *cut, const press_hip_scale_rule *rule, int32_t *q,
						      uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = args_ok(method, NONE, !row_first || (nreads && (!in || !in_off || !in_len || !off || !n || !out_n)) || (!rows && nrows_cap),
			 nreads, device_resident ? rows : nullptr, "rows");
	if (rc)
		return rc;
	if (dtype != PRESS_HIP_F32 && dtype != PRESS_HIP_F16 && dtype != PRESS_HIP_BF16)
		return set_error(PRESS_HIP_EARG, "dtype %d: PRESS_HIP_F32, PRESS_HIP_F16 or PRESS_HIP_BF16", dtype);
	if (T == 0 || T % 8 || overlap >= T)
		return set_error(PRESS_HIP_EARG, "T must be a positive multiple of 8 and overlap below T");
	if (rule && !scale_rule_ok(rule))
		return set_error(PRESS_HIP_EARG, "the scale rule is not valid (ranks num <= den, den > 0; finite floats; scale_min > 0)");
	TrimArgs t = {};
	t.mode = trim ? trim->mode : PRESS_TRIM_RANGE;
	if (t.mode == PRESS_TRIM_ADAPTOR) {
		const press_hip_jnn2_params &p = trim->adaptor;
		if ((rc = jnn2_params_ok(p)))
			return rc;
		t.adaptor = { p.std_scale, p.seg_dist, p.window, p.hi_thresh, p.lo_thresh };
	} else if (t.mode == PRESS_TRIM_SEGMENT) {
		const press_hip_jnn_params &p = trim->seg;
		if ((rc = jnn_params_ok(p)))
			return rc;
		t.seg = { p.std_scale, p.corrector, p.seg_dist, p.window, p.stall_len, p.error, p.top, p.bot };
	} else if (t.mode != PRESS_TRIM_RANGE) {
		return set_error(PRESS_HIP_EARG, "trim mode %d: PRESS_HIP_TRIM_RANGE, _ADAPTOR or _SEGMENT", t.mode);
	}
	t.min_keep = trim && t.mode != PRESS_TRIM_RANGE ? trim->min_keep : 0;
	if ((rc = device_ready(method, NONE)))
		return rc;
	hipStream_t s = g.stream();
	if (nreads == 0) { // (the plan of no reads: one zero)
		if (device_resident)
			HIPCHK(hipMemsetAsync(row_first, 0, 8, s));
		else
			row_first[0] = 0;
		return 0;
	}
	const size_t es = dtype == PRESS_HIP_F32 ? 4 : 2;
	uint64_t staged = 0; // host pointers: the rows that can be written
	if (!device_resident) {
		for (uint32_t r = 0; r < nreads; r++)
			staged += chunk_rows_of(n[r], T, T - overlap);
		staged = staged < nrows_cap ? staged : nrows_cap;
	}
	const ScratchPlan plan = make_chunks_trimmed_plan(method, total_samples, nreads, t.mode, !device_resident, staged * T * es, staged);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;
	ChunkArgs c = { rows, nrows_cap, dtype, T, overlap, row_first, total_samples, rule, q };
	t.range = t.mode == PRESS_TRIM_RANGE ? range : nullptr;
	t.seg_cal = t.mode == PRESS_TRIM_SEGMENT ? seg_cal : nullptr;
	t.cut = cut;
	t.row_read = row_read;
	t.row_start = row_start;
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, (int16_t *) plan.ptr(&Ctx::rsig) };
	StreamsIn io = host;
	Staged st(nreads, s);
	if (!device_resident) {
		if ((rc = st.streams(host, total_samples, false, g.arena, g.arena_off, io)))
			return rc;
		if (t.range) {
			HIPCHK(hipMemcpyAsync(g.px_range.p, t.range, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
			t.range = (const uint32_t *) g.px_range.p;
		}
		if (t.seg_cal) {
			HIPCHK(hipMemcpyAsync(g.sg_cal.p, t.seg_cal, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
			t.seg_cal = (const float *) g.sg_cal.p;
		}
		c.rows = g.ch_rows.p;
		c.nrows_cap = staged;
		c.row_first = (const uint64_t *) g.tr_first.p;
		c.q = (int32_t *) g.st_stats.p;
		t.cut = (uint32_t *) g.tr_user.p;
		t.row_read = (uint32_t *) g.tr_read.p;
		t.row_start = (uint32_t *) g.tr_start.p;
	}
	bind_io(a, io);
	if ((rc = launch_depress_chunks_trimmed(plan, a, c, t, s)) || device_resident)
		return rc;
	// the plan first: it says how many rows were written; then they, the row tables, the cuts, q and out_n in one go
	HIPCHK(hipMemcpyAsync(row_first, g.tr_first.p, ((size_t) nreads + 1) * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	const uint64_t written = row_first[nreads] < staged ? row_first[nreads] : staged;
	if (q)
		HIPCHK(hipMemcpyAsync(q, g.st_stats.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	if (cut)
		HIPCHK(hipMemcpyAsync(cut, g.tr_user.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(out_n, g.outn.p, (size_t) nreads * 4, hipMemcpyDeviceToHost, s));
	if (written) {
		HIPCHK(hipMemcpyAsync(rows, g.ch_rows.p, written * T * es, hipMemcpyDeviceToHost, s));
		if (row_read)
			HIPCHK(hipMemcpyAsync(row_read, g.tr_read.p, written * 4, hipMemcpyDeviceToHost, s));
		if (row_start)
			HIPCHK(hipMemcpyAsync(row_start, g.tr_start.p, written * 4, hipMemcpyDeviceToHost, s));
	}
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// ------------------------------------------------------------------ statistics of samples that are already there

// What the stats calls share: the scratch of a call that decodes nothing (rows_bytes / state_bytes: its count rows and
// pick state), the samples - staged, with result_bytes of g.st_stats for what comes back, unless device resident - the
// argument block, and the tile table enqueued.
static int stats_begin(const SamplesIn &host, uint64_t total_samples, bool device_resident, size_t rows_bytes, size_t state_bytes,
		       size_t result_bytes, Staged &st, DecodeArgs &a, bool with_range = false)
{
	int rc;
	ScratchPlan plan = make_tiles_plan(total_samples, st.nreads);
	plan.need(&Ctx::st_rows, rows_bytes).need(&Ctx::st_read, state_bytes);
	if (!device_resident)
		plan.need(&Ctx::st_stats, result_bytes);
	if (!device_resident && with_range) // (the ranged forms: the caller's ranges, staged)
		plan.need(&Ctx::px_range, (size_t) st.nreads * 8);
	if ((rc = plan.reserve()))
		return rc;
	plan.bind(a);
	a.nreads = st.nreads;
	SamplesIn in = host;
	if (!device_resident && (rc = st.samples_in(host, total_samples, in)))
		return rc;
	bind_io(a, in);
	launch_pa_tiles(a, (uint2 *) g.pa_tile.p, (uint32_t *) g.pa_ctl.p, st.s);
	return 0;
}

static void stats_launch(const DecodeArgs &a, int32_t *stats, hipEvent_t *ev, hipStream_t s)
{
	launch_signal_stats(a, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, g.st_read.p, (uint32_t *) g.st_rows.p, stats,
			    nullptr, ev, s);
}

extern "C" int press_hip_signal_stats(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				      uint64_t total_samples, int32_t *stats, int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, nreads && (!sig || !off || !n || !stats), nreads, device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	Staged st(nreads, s);
	DecodeArgs a;
	if ((rc = stats_begin({ sig, off, n }, total_samples, device_resident, stat_rows_bytes(nreads), stat_state_bytes(nreads),
			      (size_t) nreads * 8, st, a)))
		return rc;
	stats_launch(a, device_resident ? stats : (int32_t *) g.st_stats.p, nullptr, s);
	if ((rc = launch_status()) || device_resident)
		return rc;
	return st.fetch_tables({ { stats, g.st_stats.p, (size_t) nreads * 8 } });
}

// Quantiles of a batch: press_hip_signal_stats' layout and staging, nq ranks in four launches (press_quant.hip)
extern "C" int press_hip_signal_quantiles(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					  uint64_t total_samples, const uint32_t *rank_num, const uint32_t *rank_den, uint32_t nq,
					  int32_t *q, int device_resident)
{
	API_LOCK;
	if (nq < 1 || nq > QMAX) // (it sizes the ranks' tables: before them)
		return set_error(PRESS_HIP_EARG, "nq = %u: 1 .. %u quantiles", nq, QMAX);
	int rc = args_ok(NONE, NONE, !rank_num || !rank_den || (nreads && (!sig || !off || !n || !q)), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc)
		return rc;
	for (uint32_t i = 0; i < nq; i++)
		if (rank_den[i] == 0 || rank_num[i] > rank_den[i])
			return set_error(PRESS_HIP_EARG, "rank %u: %u / %u is not in [0, 1]", i, rank_num[i], rank_den[i]);
	if ((rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	Staged st(nreads, s);
	DecodeArgs a;
	if ((rc = stats_begin({ sig, off, n }, total_samples, device_resident, std::max(stat_rows_bytes(nreads), quant_rows_bytes(nreads, nq)),
			      std::max(stat_state_bytes(nreads), quant_state_bytes(nreads)), (size_t) nreads * nq * 4, st, a)))
		return rc;
	launch_signal_quantiles(a, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, g.st_read.p, (uint32_t *) g.st_rows.p, rank_num,
				rank_den, nq, device_resident ? q : (int32_t *) g.st_stats.p, nullptr, nullptr, s);
	if ((rc = launch_status()) || device_resident)
		return rc;
	return st.fetch_tables({ { q, g.st_stats.p, (size_t) nreads * nq * 4 } });
}

// The ranged forms (include/press_hip.h 2y): the same checks, staging and launch counts; the kernels clamp the range.
// Host pointers: the range is staged in g.px_range (stats_begin with_range).  *drange: what the kernels read (NULL: whole reads)
static int stage_range(const uint32_t *range, uint32_t nreads, bool device_resident, hipStream_t s, const uint32_t **drange)
{
	*drange = range;
	if (device_resident || !range)
		return 0;
	HIPCHK(hipMemcpyAsync(g.px_range.p, range, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	*drange = (const uint32_t *) g.px_range.p;
	return 0;
}

extern "C" int press_hip_signal_stats_ranged(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					     uint64_t total_samples, const uint32_t *range, int32_t *stats, int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, nreads && (!sig || !off || !n || !stats), nreads, device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	Staged st(nreads, s);
	DecodeArgs a;
	const uint32_t *dr;
	if ((rc = stats_begin({ sig, off, n }, total_samples, device_resident, stat_rows_bytes(nreads), stat_state_bytes(nreads),
			      (size_t) nreads * 8, st, a, range != nullptr)) ||
	    (rc = stage_range(range, nreads, device_resident, s, &dr)))
		return rc;
	int32_t *out = device_resident ? stats : (int32_t *) g.st_stats.p;
	if (dr)
		launch_signal_stats_ranged(a, dr, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, g.st_read.p, (uint32_t *) g.st_rows.p,
					   out, nullptr, s);
	else
		stats_launch(a, out, nullptr, s);
	if ((rc = launch_status()) || device_resident)
		return rc;
	return st.fetch_tables({ { stats, g.st_stats.p, (size_t) nreads * 8 } });
}

extern "C" int press_hip_signal_quantiles_ranged(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
						 uint64_t total_samples, const uint32_t *range, const uint32_t *rank_num,
						 const uint32_t *rank_den, uint32_t nq, int32_t *q, int device_resident)
{
	API_LOCK;
	if (nq < 1 || nq > QMAX) // (it sizes the ranks' tables: before them)
		return set_error(PRESS_HIP_EARG, "nq = %u: 1 .. %u quantiles", nq, QMAX);
	int rc = args_ok(NONE, NONE, !rank_num || !rank_den || (nreads && (!sig || !off || !n || !q)), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc)
		return rc;
	for (uint32_t i = 0; i < nq; i++)
		if (rank_den[i] == 0 || rank_num[i] > rank_den[i])
			return set_error(PRESS_HIP_EARG, "rank %u: %u / %u is not in [0, 1]", i, rank_num[i], rank_den[i]);
	if ((rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	Staged st(nreads, s);
	DecodeArgs a;
	const uint32_t *dr;
	if ((rc = stats_begin({ sig, off, n }, total_samples, device_resident, std::max(stat_rows_bytes(nreads), quant_rows_bytes(nreads, nq)),
			      std::max(stat_state_bytes(nreads), quant_state_bytes(nreads)), (size_t) nreads * nq * 4, st, a, range != nullptr)) ||
	    (rc = stage_range(range, nreads, device_resident, s, &dr)))
		return rc;
	int32_t *out = device_resident ? q : (int32_t *) g.st_stats.p;
	if (dr)
		launch_signal_quantiles_ranged(a, dr, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, g.st_read.p,
					       (uint32_t *) g.st_rows.p, rank_num, rank_den, nq, out, nullptr, nullptr, s);
	else
		launch_signal_quantiles(a, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, g.st_read.p, (uint32_t *) g.st_rows.p,
					rank_num, rank_den, nq, out, nullptr, nullptr, s);
	if ((rc = launch_status()) || device_resident)
		return rc;
	return st.fetch_tables({ { q, g.st_stats.p, (size_t) nreads * nq * 4 } });
}

// Profiling aid: the device-resident press_hip_signal_stats with an event behind every kernel; synchronous.
// ms[0 .. 8): count / pick / count / pick of the median, then of the MAD.
extern "C" int press_hip_signal_stats_timed(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					    uint64_t total_samples, int32_t *stats, float *ms)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, !sig || !off || !n || !stats || !ms || !nreads, nreads, sig, "sig");
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	hipStream_t s = g.stream();
	Staged st(nreads, s);
	DecodeArgs a;
	if ((rc = stats_begin({ sig, off, n }, total_samples, true, stat_rows_bytes(nreads), stat_state_bytes(nreads), 0, st, a)))
		return rc;
	hipEvent_t ev[9] = {};
	for (int i = 0; i < 9 && !rc; i++)
		if (hipEventCreate(&ev[i]) != hipSuccess)
			rc = set_error(PRESS_HIP_EHIP, "hipEventCreate failed");
	if (!rc) {
		stats_launch(a, stats, ev, s);
		if (!(rc = launch_status()) && hipStreamSynchronize(s) != hipSuccess)
			rc = set_error(PRESS_HIP_EHIP, "hipStreamSynchronize failed");
		for (int i = 0; i < 8 && !rc; i++)
			if (hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) != hipSuccess)
				rc = set_error(PRESS_HIP_EHIP, "hipEventElapsedTime failed");
	}
	for (int i = 0; i < 9; i++)
		if (ev[i])
			(void) hipEventDestroy(ev[i]);
	return rc;
}

// ------------------------------------------------------------------ records of samples that are already there: two walks
//
// What press_hip_signal_events and press_hip_signal_segments share behind their checks.  Two walks over the reads: `count`
// with the layout (first, count, and thr where the call has one), then `write` with the records of the reads that fit.
// Host pointers: press_hip_signal_stats' staging; first[nreads] comes back between the walks, the records' arena is
// reserved at min(need, cap) records and comes back in one transfer.

struct RecordsOut { // the caller's results, or what is staged for them
	void *rec;
	uint64_t cap;
	size_t rec_bytes;
	uint64_t *first;
	uint32_t *count;
	float *thr; // NULL: not asked for, or a call without thresholds
};
struct RecordsStage { // the DevBufs of the host-pointer form: the calibration, first, count, the records; thr (NULL: a call without)
	DevBuf &cal, &first, &cnt, &out;
	DevBuf *thr;
};

template <class Count, class Write>
static int two_walks(const SamplesIn &host, uint32_t nreads, uint64_t total_samples, const float *cal, const RecordsOut &out,
		     const ScratchPlan &plan, const RecordsStage &b, int device_resident, Count count, Write write)
{
	int rc;
	hipStream_t s = g.stream();
	if (nreads == 0) { // (the layout of no reads: one zero)
		if (device_resident)
			HIPCHK(hipMemsetAsync(out.first, 0, 8, s));
		else
			out.first[0] = 0;
		return 0;
	}
	if ((rc = plan.reserve()))
		return rc;
	if (device_resident) {
		count(host, cal, out, s);
		if (out.cap)
			write(host, cal, out, s);
		return launch_status();
	}
	SamplesIn in;
	Staged st(nreads, s);
	if ((rc = st.samples_in(host, total_samples, in)))
		return rc;
	const float *dcal = cal ? (const float *) b.cal.p : nullptr; // (NULL: the raw domain of the segments)
	RecordsOut d = { nullptr, out.cap, out.rec_bytes, (uint64_t *) b.first.p, (uint32_t *) b.cnt.p, out.thr ? (float *) b.thr->p : nullptr };
	if (cal)
		HIPCHK(hipMemcpyAsync(b.cal.p, cal, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	count(in, dcal, d, s);
	if ((rc = launch_status()) || (rc = st.fetch_tables({ { out.first, d.first, ((size_t) nreads + 1) * 8 },
							       { out.count, d.count, (size_t) nreads * 4 },
							       { out.thr, d.thr, (size_t) nreads * 8 } })))
		return rc;
	const uint64_t have = out.first[nreads] < out.cap ? out.first[nreads] : out.cap;
	if (!have)
		return 0;
	if (b.out.reserve(have * out.rec_bytes))
		return PRESS_HIP_EHIP;
	HIPCHK(hipMemsetAsync(b.out.p, 0, have * out.rec_bytes, s)); // (the room of a read that did not fit: zeros)
	d.rec = b.out.p;
	write(in, dcal, d, s);
	if ((rc = launch_status()) || (rc = st.fetch_prefix(out.rec, b.out.p, have * out.rec_bytes)))
		return rc;
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// ------------------------------------------------------------------ events of samples that are already there
//
// two_walks over the kernels of press_events.hip.

static_assert(sizeof(press_hip_event) == 16 && sizeof(press_hip_event_params) == sizeof(EvParams), "the event structs");

extern "C" int press_hip_event_params_preset(int rna, press_hip_event_params *prm)
{
	if (!prm)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (rna)
		*prm = { 7, 14, 2.5f, 9.0f, 1.0f }; // events.c:50-54
	else
		*prm = { 3, 6, 1.4f, 9.0f, 0.2f }; // events.c:43-47
	return 0;
}

extern "C" int press_hip_signal_events(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				       uint64_t total_samples, const float *cal, const press_hip_event_params *prm,
				       press_hip_event *ev, uint64_t ev_cap, uint64_t *ev_first, uint32_t *ev_count, int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, !prm || !ev_first || (nreads && (!sig || !off || !n || !cal || !ev_count)) || (!ev && ev_cap), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc)
		return rc;
	if (prm->w1 < 2 || prm->w1 > 64 || prm->w2 < 2 || prm->w2 > 64)
		return set_error(PRESS_HIP_EARG, "window lengths %u, %u: 2 .. 64", prm->w1, prm->w2);
	if ((rc = device_ready(NONE, NONE)))
		return rc;
	const EvParams p = { prm->w1, prm->w2, prm->threshold1, prm->threshold2, prm->peak_height };
	const ScratchPlan plan = make_events_plan(nreads, !device_resident);
	return two_walks(
		{ sig, off, n }, nreads, total_samples, cal, { ev, ev_cap, sizeof(press_hip_event), ev_first, ev_count, nullptr }, plan,
		{ g.ev_cal, g.ev_first, g.ev_cnt, g.ev_out, nullptr }, device_resident,
		[&](const SamplesIn &in, const float *c, const RecordsOut &o, hipStream_t s) {
			launch_events_count(in.sig, in.off, in.n, nreads, c, p, plan.ptr(&Ctx::ev_state), o.cap, o.first, o.count, s);
		},
		[&](const SamplesIn &in, const float *c, const RecordsOut &o, hipStream_t s) {
			launch_events_write(in.sig, in.off, in.n, nreads, c, p, plan.ptr(&Ctx::ev_state), o.rec, o.cap, o.first, s);
		});
}

// ------------------------------------------------------------------ jnn segments and the adaptor of samples that are already there
//
// two_walks over the kernels of press_segments.hip (thr, and a NULL cal for the raw domain); the adaptor is one launch.

static_assert(sizeof(press_hip_segment) == 8 && sizeof(press_hip_jnn_params) == sizeof(SegParams) &&
		      sizeof(press_hip_jnn2_params) == sizeof(Seg2Params),
	      "the segment structs");

extern "C" int press_hip_jnn_params_preset(int which, press_hip_jnn_params *prm)
{
	if (!prm)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	switch (which) {
	case 0: *prm = { 0.75f, 50, 50, 150, 0.25f, 5, 0.0f, 0.0f }; return 0;   // JNNV1_CDNA_PARAM, jnn.h:40-49
	case 1: *prm = { 0.75f, 50, 50, 1000, 1.0f, 5, 0.0f, 0.0f }; return 0;   // JNNV1_DRNA_PARAM, jnn.h:29-38
	case 2: *prm = { -1.0f, 50, 200, 250, 1.0f, 30, 0.0f, 0.0f }; return 0;  // JNNV1_POLYA, jnn.h:52-61
	}
	return set_error(PRESS_HIP_EARG, "preset %d: 0 cDNA, 1 dRNA, 2 poly-A", which);
}

extern "C" int press_hip_jnn2_params_preset(int which, press_hip_jnn2_params *prm)
{
	if (!prm)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (which != 0)
		return set_error(PRESS_HIP_EARG, "preset %d: 0 the dRNA adaptor", which);
	*prm = { 0.5f, 1500, 2000, 200000, 2000 }; // JNNV2_RNA_ADAPTOR, jnn.h:74-80
	return 0;
}

extern "C" int press_hip_signal_segments(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					 uint64_t total_samples, const float *cal, const press_hip_jnn_params *prm,
					 press_hip_segment *seg, uint64_t seg_cap, uint64_t *seg_first, uint32_t *seg_count, float *thr,
					 int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, !prm || !seg_first || (nreads && (!sig || !off || !n || !seg_count)) || (!seg && seg_cap), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc)
		return rc;
	if ((rc = jnn_params_ok(*prm)))
		return rc;
	if ((rc = device_ready(NONE, NONE)))
		return rc;
	const SegParams p = { prm->std_scale, prm->corrector, prm->seg_dist, prm->window, prm->stall_len, prm->error, prm->top, prm->bot };
	const ScratchPlan plan = make_segments_plan(nreads, !device_resident, cal != nullptr);
	return two_walks(
		{ sig, off, n }, nreads, total_samples, cal, { seg, seg_cap, sizeof(press_hip_segment), seg_first, seg_count, thr }, plan,
		{ g.sg_cal, g.sg_first, g.sg_cnt, g.sg_out, &g.sg_thr }, device_resident,
		[&](const SamplesIn &in, const float *c, const RecordsOut &o, hipStream_t s) {
			launch_segments_count(in.sig, in.off, in.n, nreads, c, p, plan.ptr(&Ctx::sg_state), o.cap, o.first, o.count, o.thr, s);
		},
		[&](const SamplesIn &in, const float *c, const RecordsOut &o, hipStream_t s) {
			launch_segments_write(in.sig, in.off, in.n, nreads, c, p, plan.ptr(&Ctx::sg_state), o.rec, o.cap, o.first, s);
		});
}

extern "C" int press_hip_signal_adaptor(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					uint64_t total_samples, const press_hip_jnn2_params *prm, int32_t *pair, float *thr,
					int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, !prm || (nreads && (!sig || !off || !n || !pair)), nreads, device_resident ? sig : nullptr, "sig");
	if (rc)
		return rc;
	if ((rc = jnn2_params_ok(*prm)))
		return rc;
	if ((rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const Seg2Params p = { prm->std_scale, prm->seg_dist, prm->window, prm->hi_thresh, prm->lo_thresh };
	const ScratchPlan plan = make_adaptor_plan(nreads, !device_resident);
	if ((rc = plan.reserve()))
		return rc;
	if (device_resident) {
		launch_adaptor(sig, off, n, nreads, p, pair, thr, s);
		return launch_status();
	}
	SamplesIn in = { sig, off, n };
	Staged st(nreads, s);
	if ((rc = st.samples_in(in, total_samples, in)))
		return rc;
	launch_adaptor(in.sig, in.off, in.n, nreads, p, (int32_t *) g.sg_out.p, thr ? (float *) g.sg_thr.p : nullptr, s);
	if ((rc = launch_status()))
		return rc;
	return st.fetch_tables({ { pair, g.sg_out.p, (size_t) nreads * 8 }, { thr, g.sg_thr.p, (size_t) nreads * 8 } });
}

// ------------------------------------------------------------------ range statistics and sigtk's prefix of samples that are already there
//
// The kernels of press_ranges.hip: one launch for the statistics; the adaptor, the poly-A walk and (with stat) the
// statistics of the two stretches for the prefix.

static_assert(sizeof(press_hip_range_stat) == 12 && sizeof(press_hip_prefix) == 16, "the range and prefix structs");

extern "C" int press_hip_signal_range_stats(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					    uint64_t total_samples, const float *cal, const uint32_t *range,
					    press_hip_range_stat *out, int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, nreads && (!sig || !off || !n || !out), nreads, device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_range_stats_plan(nreads, !device_resident, cal != nullptr, range != nullptr);
	if ((rc = plan.reserve()))
		return rc;
	if (device_resident) {
		launch_range_stats(sig, off, n, nreads, 0, cal, range, out, s);
		return launch_status();
	}
	SamplesIn in = { sig, off, n };
	Staged st(nreads, s);
	if ((rc = st.samples_in(in, total_samples, in)))
		return rc;
	if (cal)
		HIPCHK(hipMemcpyAsync(g.sg_cal.p, cal, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	if (range)
		HIPCHK(hipMemcpyAsync(g.px_range.p, range, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	launch_range_stats(in.sig, in.off, in.n, nreads, 0, cal ? (const float *) g.sg_cal.p : nullptr,
			   range ? (const uint32_t *) g.px_range.p : nullptr, g.px_stat.p, s);
	if ((rc = launch_status()))
		return rc;
	return st.fetch_tables({ { out, g.px_stat.p, (size_t) nreads * 12 } });
}

extern "C" int press_hip_prefix_params_preset(int which, press_hip_prefix_params *prm)
{
	if (!prm)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (which != 0)
		return set_error(PRESS_HIP_EARG, "preset %d: 0 the dRNA prefix", which);
	prm->adaptor = { 0.5f, 1500, 2000, 200000, 2000 };         // JNNV2_RNA_ADAPTOR, jnn.h:74-80
	prm->polya = { -1.0f, 50, 200, 250, 1.0f, 30, 0.0f, 0.0f }; // JNNV1_POLYA, jnn.h:52-61
	prm->rna = 1;
	prm->shift = 30.0f; // m_a+30+20, m_a+30-20 (cfunc.c:191)
	prm->half = 20.0f;
	return 0;
}

extern "C" int press_hip_signal_prefix(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				       uint64_t total_samples, const float *cal, const press_hip_prefix_params *prm,
				       press_hip_prefix *out, press_hip_range_stat *stat, float *thr, int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, !prm || (nreads && (!sig || !off || !n || !cal || !out)), nreads, device_resident ? sig : nullptr, "sig");
	if (rc)
		return rc;
	const press_hip_jnn_params &pa = prm->polya;
	if ((rc = jnn_params_ok(pa)) || (rc = jnn2_params_ok(prm->adaptor)))
		return rc;
	if (stat && nreads > 0x7FFFFFFFu)
		return set_error(PRESS_HIP_EARG, "nreads = %u with stat: at most 2^31 - 1 (two ranges per read)", nreads);
	if ((rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const Seg2Params p2 = { prm->adaptor.std_scale, prm->adaptor.seg_dist, prm->adaptor.window, prm->adaptor.hi_thresh, prm->adaptor.lo_thresh };
	const SegParams p = { pa.std_scale, pa.corrector, pa.seg_dist, pa.window, pa.stall_len, pa.error, pa.top, pa.bot };
	const ScratchPlan plan = make_prefix_plan(nreads, !device_resident);
	if ((rc = plan.reserve()))
		return rc;
	int32_t *pair = (int32_t *) g.px_pair.p;
	uint32_t *range = (uint32_t *) g.px_range.p;
	auto launch = [&](const SamplesIn &in, const float *c, void *o, void *st, float *t) {
		launch_adaptor(in.sig, in.off, in.n, nreads, p2, pair, nullptr, s);
		launch_prefix(in.sig, in.off, in.n, nreads, c, p, prm->rna, prm->shift, prm->half, pair, o, t, range, s);
		if (st)
			launch_range_stats(in.sig, in.off, in.n, 2 * nreads, 1, c, range, st, s);
	};
	if (device_resident) {
		launch({ sig, off, n }, cal, out, stat, thr);
		return launch_status();
	}
	SamplesIn in = { sig, off, n };
	Staged st(nreads, s);
	if ((rc = st.samples_in(in, total_samples, in)))
		return rc;
	HIPCHK(hipMemcpyAsync(g.sg_cal.p, cal, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	launch(in, (const float *) g.sg_cal.p, g.px_out.p, stat ? g.px_stat.p : nullptr, thr ? (float *) g.sg_thr.p : nullptr);
	if ((rc = launch_status()))
		return rc;
	return st.fetch_tables({ { out, g.px_out.p, (size_t) nreads * 16 },
				 { stat, g.px_stat.p, (size_t) nreads * 24 },
				 { thr, g.sg_thr.p, (size_t) nreads * 8 } });
}

// ------------------------------------------------------------------ recode: streams in, streams out
//
// The two halves run one after the other on the stream, inside one call and one lock: the decode of `src` into the
// caller's samples (or the library's own, sig == NULL), the verdicts out_n turned into the sample counts of the press
// half (a refused read: 0), the press of `dst`.  The halves share the chunk table, the granules and the per-read records,
// which is fine in sequence - except for a fused pair (recode_fused), where the svb decode kernel writes the press half's
// chunk descriptors while it reads its own: that press has a table, a first-chunk list and a control block to itself.

// press_hip_recode_degraded_*, a pair that is not fused: D_bits in place over the out_n[r] samples the decode half has left
// (the zstd kinds' host fallback lies inside launch_depress: it is behind us), before the press half reads them.  A fused
// pair's decode kernel degrades the samples it holds (launch_recode_fused).
static void recode_degrade(const RecodePlan &rp, const DecodeArgs &da, hipStream_t s)
{
	if (!rp.bits)
		return;
	launch_pa_tiles(da, (uint2 *) g.pa_tile.p, (uint32_t *) g.pa_ctl.p, s);
	launch_degrade(da, da.sig, rp.bits, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, s);
}

static int launch_recode(const RecodePlan &rp, DecodeArgs &da, BatchArgs &pa, hipStream_t s)
{
	int rc;
	pa.sig = da.sig;
	pa.off = da.off;
	pa.nsamp = (const uint32_t *) g.rn.p;
	const Method &sm = *rp.d.m, &dm = *rp.p.m;
	if (rp.fused) {
		pa.chunks = (ChunkDesc *) g.pchunks.p;
		pa.first_chunk = (uint32_t *) g.pfirst.p;
		pa.ctl = (ChunkCtl *) g.pctl.p;
		launch_recode_fused(da, pa, sm.key2, sm.slow5, dm.exfmt, dm.ent, s, rp.bits);
	} else {
		if ((rc = launch_depress(rp.d, da, s)))
			return rc;
		launch_recode_counts(da.out_n, (uint32_t *) g.rn.p, da.nreads, s);
		recode_degrade(rp, da, s);
		if (rp.keep_heads)
			launch_recode_refused(da.out_n, pa, (uint8_t *) g.rkeep.p, true, s);
		if ((rc = launch_press(rp.p, pa, s)))
			return rc;
	}
	launch_recode_refused(da.out_n, pa, rp.keep_heads ? (uint8_t *) g.rkeep.p : nullptr, false, s);
	return launch_status();
}

// What the three recode calls share between their head and their launch: the plan reserved and bound, the source
// streams and rooms - the caller's or staged (then the checks of press_hip_depress_batch) - in da.  The samples nobody
// keeps go to g.rsig.
static int recode_begin(const RecodePlan &rp, const StreamsIn &host, uint64_t total_samples, bool device_resident, Staged &st,
			DecodeArgs &da, BatchArgs &pa)
{
	int rc;
	if ((rc = rp.all.reserve()))
		return rc;
	rp.d.bind(da);
	rp.p.bind(pa);
	da.nreads = pa.nreads = st.nreads;
	StreamsIn io = host;
	if (!device_resident && (rc = st.streams(host, total_samples, host.sig != nullptr, g.rin, g.rin_off, io)))
		return rc;
	if (!io.sig)
		io.sig = (int16_t *) g.rsig.p;
	bind_io(da, io);
	return 0;
}

// The tail of a staged recode's decode half: the samples the caller keeps with out_n (synchronised), else out_n alone
// (synchronised if this is the call's last copy)
static int recode_fetch_decoded(Staged &st, const StreamsIn &host, bool last)
{
	if (host.sig)
		return st.fetch_samples(host);
	HIPCHK(hipMemcpyAsync(host.out_n, g.outn.p, (size_t) st.nreads * 4, hipMemcpyDeviceToHost, st.s));
	if (last)
		HIPCHK(hipStreamSynchronize(st.s));
	return 0;
}

static int bits_ok(uint32_t bits)
{
	return bits > 8 ? set_error(PRESS_HIP_EARG, "bits = %u: 0 .. 8 low bits can be dropped", bits) : 0;
}

// press_hip_recode_batch (bits == 0) and press_hip_recode_degraded_batch
static int recode_batch(int src_method, int dst_method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
			const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
			uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
			int16_t *sig, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = bits_ok(bits);
	if (rc)
		return rc;
	rc = args_ok(src_method, dst_method, nreads && (!in || !in_off || !in_len || !n || !off || !out || !out_off || !out_len || !out_n),
			 nreads, device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(src_method, dst_method)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const RecodePlan rp = make_recode_plan(src_method, dst_method, total_samples, nreads, sig != nullptr, bits);
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, sig };
	const SlotsOut slots = { out, out_off, out_len };
	SlotsOut so = slots;
	Staged st(nreads, s);
	DecodeArgs da;
	BatchArgs pa;
	// host pointers: both calls' checks, the streams and the layout staged, the two halves, the copies back
	if (!device_resident && (rc = check_slots(out_off, nreads)))
		return rc;
	if ((rc = recode_begin(rp, host, total_samples, device_resident, st, da, pa)) || (!device_resident && (rc = st.slots(slots, so))))
		return rc;
	bind_io(pa, so);
	if ((rc = launch_recode(rp, da, pa, s)) || device_resident || (rc = recode_fetch_decoded(st, host, false)))
		return rc;
	return st.fetch_streams(slots);
}

extern "C" int press_hip_recode_batch(int src_method, int dst_method, const uint8_t *in, const uint64_t *in_off,
				      const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
				      uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
				      int16_t *sig, uint32_t *out_n, int device_resident)
{
	return recode_batch(src_method, dst_method, 0, in, in_off, in_len, n, off, nreads, total_samples, out, out_off, out_len, sig, out_n,
			    device_resident);
}

extern "C" int press_hip_recode_degraded_batch(int src_method, int dst_method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
					       const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
					       uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
					       int16_t *sig, uint32_t *out_n, int device_resident)
{
	return recode_batch(src_method, dst_method, bits, in, in_off, in_len, n, off, nreads, total_samples, out, out_off, out_len, sig,
			    out_n, device_resident);
}

// ------------------------------------------------------------------ packed recode: streams in, a library-made arena out
//
// launch_recode with the press half cut in two (PackArgs, press_internal.h).  PACK_SIZE: the decode, the press half's
// sample counts, the destination's chain up to its sizes WITHOUT its scan; then the reads the source refused lose their
// size and their slot (launch_pack_scan_refused) - only then are the offsets final - and the exception family's chunks
// learn their bases.  PACK_WRITE: the rest of the destination's chain, and out_len = FAILED for the refused reads
// (k_recode_refused without a keep: it touches out_len alone).  pa.out_off must be pk.slot.
static int launch_recode_packed(const RecodePlan &rp, DecodeArgs &da, BatchArgs &pa, PackArgs pk, int phases, hipStream_t s)
{
	int rc;
	pa.sig = da.sig;
	pa.off = da.off;
	pa.nsamp = (const uint32_t *) g.rn.p;
	if (pk.out_cap == PRESS_HIP_FAILED) // (k_chunk_prep<.., EXACT> compares need[r] = FAILED with it)
		pk.out_cap--;
	const Method &sm = *rp.d.m, &dm = *rp.p.m;
	if (rp.fused) {
		pa.chunks = (ChunkDesc *) g.pchunks.p;
		pa.first_chunk = (uint32_t *) g.pfirst.p;
		pa.ctl = (ChunkCtl *) g.pctl.p;
		launch_recode_fused_packed(da, pa, sm.key2, sm.slow5, dm.exfmt, dm.ent, pk, phases, s, rp.bits);
	} else {
		if (phases & PACK_SIZE) {
			if ((rc = launch_depress(rp.d, da, s)))
				return rc;
			launch_recode_counts(da.out_n, (uint32_t *) g.rn.p, da.nreads, s);
			recode_degrade(rp, da, s);
			PackArgs sz = pk;
			sz.layout = nullptr; // (the scan comes behind the refused reads' correction)
			if ((rc = launch_press_packed(rp.p, pa, sz, PACK_SIZE, s)))
				return rc;
			launch_pack_scan_refused(pk, da.out_n, da.nreads, s);
			if (pk.layout && dm.family == FAM_EX)
				launch_pack_patch(pa, pk.slot, s);
		}
		if ((phases & PACK_WRITE) && (rc = launch_press_packed(rp.p, pa, pk, PACK_WRITE, s)))
			return rc;
	}
	if (phases & PACK_WRITE)
		launch_recode_refused(da.out_n, pa, nullptr, false, s);
	return launch_status();
}

static int recode_sizes(int src_method, int dst_method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
			const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
			uint64_t total_samples, uint64_t *need, int16_t *sig, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = bits_ok(bits);
	if (rc)
		return rc;
	rc = args_ok(src_method, dst_method, nreads && (!in || !in_off || !in_len || !n || !off || !need || !out_n), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(src_method, dst_method)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const RecodePlan rp = make_recode_packed_plan(src_method, dst_method, total_samples, nreads, sig != nullptr, bits);
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, sig };
	Staged st(nreads, s);
	DecodeArgs da;
	BatchArgs pa;
	if ((rc = recode_begin(rp, host, total_samples, device_resident, st, da, pa)))
		return rc;
	const PackArgs pk = { device_resident ? need : (uint64_t *) g.pneed.p, nullptr, (uint64_t *) g.pslot.p, 0, 1 };
	bind_io(pa, SlotsOut{ nullptr, pk.slot, pk.need }); // (as press_hip_press_sizes)
	if ((rc = launch_recode_packed(rp, da, pa, pk, PACK_SIZE, s)) || device_resident)
		return rc;
	HIPCHK(hipMemcpyAsync(need, pk.need, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	return recode_fetch_decoded(st, host, true);
}

extern "C" int press_hip_recode_sizes(int src_method, int dst_method, const uint8_t *in, const uint64_t *in_off,
				      const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
				      uint64_t total_samples, uint64_t *need, int16_t *sig, uint32_t *out_n, int device_resident)
{
	return recode_sizes(src_method, dst_method, 0, in, in_off, in_len, n, off, nreads, total_samples, need, sig, out_n, device_resident);
}

extern "C" int press_hip_recode_degraded_sizes(int src_method, int dst_method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
					       const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
					       uint64_t total_samples, uint64_t *need, int16_t *sig, uint32_t *out_n, int device_resident)
{
	return recode_sizes(src_method, dst_method, bits, in, in_off, in_len, n, off, nreads, total_samples, need, sig, out_n,
			    device_resident);
}

static int recode_packed(int src_method, int dst_method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
			 const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
			 uint64_t total_samples, uint8_t *out, uint64_t out_cap, uint32_t align, uint64_t *out_off,
			 uint64_t *out_len, int16_t *sig, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = bits_ok(bits);
	if (rc)
		return rc;
	rc = args_ok(src_method, dst_method,
			 !out_off || (nreads && (!in || !in_off || !in_len || !n || !off || !out_len || !out_n || (!out && out_cap))), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc || (rc = align_ok(align)) || (rc = device_ready(src_method, dst_method)))
		return rc;
	if (nreads == 0)
		return packed_empty(out_off, device_resident);
	hipStream_t s = g.stream();
	const RecodePlan rp = make_recode_packed_plan(src_method, dst_method, total_samples, nreads, sig != nullptr, bits);
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, sig };
	Staged st(nreads, s);
	DecodeArgs da;
	BatchArgs pa;
	// host pointers: stage, decode and size, read the arena's size back, write into an arena of that size, copy its prefix
	// back in one piece
	if (!device_resident && (g.arena_off.reserve(((size_t) nreads + 1) * 8) || g.lens.reserve((size_t) nreads * 8)))
		return PRESS_HIP_EHIP;
	if ((rc = recode_begin(rp, host, total_samples, device_resident, st, da, pa)))
		return rc;
	PackArgs pk = { (uint64_t *) g.pneed.p, out_off, (uint64_t *) g.pslot.p, out_cap, align };
	SlotsOut so = { out, pk.slot, out_len };
	if (!device_resident) {
		pk.layout = (uint64_t *) g.arena_off.p;
		so = { nullptr, pk.slot, (uint64_t *) g.lens.p };
	}
	bind_io(pa, so);
	if ((rc = launch_recode_packed(rp, da, pa, pk, device_resident ? PACK_SIZE | PACK_WRITE : PACK_SIZE, s)) || device_resident)
		return rc;
	if ((rc = packed_tail(st, out, out_cap, out_off, out_len, pa, pk, [&] { return launch_recode_packed(rp, da, pa, pk, PACK_WRITE, s); })))
		return rc;
	return recode_fetch_decoded(st, host, true);
}

extern "C" int press_hip_recode_packed(int src_method, int dst_method, const uint8_t *in, const uint64_t *in_off,
				       const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
				       uint64_t total_samples, uint8_t *out, uint64_t out_cap, uint32_t align, uint64_t *out_off,
				       uint64_t *out_len, int16_t *sig, uint32_t *out_n, int device_resident)
{
	return recode_packed(src_method, dst_method, 0, in, in_off, in_len, n, off, nreads, total_samples, out, out_cap, align, out_off,
			     out_len, sig, out_n, device_resident);
}

extern "C" int press_hip_recode_degraded_packed(int src_method, int dst_method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
						const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
						uint64_t total_samples, uint8_t *out, uint64_t out_cap, uint32_t align, uint64_t *out_off,
						uint64_t *out_len, int16_t *sig, uint32_t *out_n, int device_resident)
{
	return recode_packed(src_method, dst_method, bits, in, in_off, in_len, n, off, nreads, total_samples, out, out_cap, align, out_off,
			     out_len, sig, out_n, device_resident);
}

// ------------------------------------------------------------------ degrade: D_b of samples that are already there
//
// press_hip_signal_stats' layout, staging and tile table; the kernel of press_degrade.hip.  Host pointers: the samples are
// staged, degraded in place there, and exactly n[r] samples per read come back into `out`.

extern "C" int press_hip_degrade_batch(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				       uint64_t total_samples, uint32_t bits, int16_t *out, int device_resident)
{
	API_LOCK;
	int rc = bits_ok(bits);
	if (rc || (rc = args_ok(NONE, NONE, nreads && (!sig || !off || !n || !out), nreads, device_resident ? sig : nullptr, "sig")) ||
	    (rc = args_ok(NONE, NONE, false, nreads, device_resident ? out : nullptr, "out")) || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	ScratchPlan plan = make_tiles_plan(total_samples, nreads);
	if (!device_resident)
		plan.need(&Ctx::outn, (size_t) nreads * 4);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;
	SamplesIn in = { sig, off, n };
	int16_t *dst = out;
	Staged st(nreads, s);
	if (!device_resident) {
		if ((rc = st.samples_in(in, total_samples, in)))
			return rc;
		dst = (int16_t *) g.sig.p;
		HIPCHK(hipMemcpyAsync(g.outn.p, g.nsamp.p, (size_t) nreads * 4, hipMemcpyDeviceToDevice, s)); // (fetch_elems' counts)
	}
	bind_io(a, in);
	launch_pa_tiles(a, (uint2 *) g.pa_tile.p, (uint32_t *) g.pa_ctl.p, s);
	if (bits || dst != in.sig) // (D_0 is the identity: out of place the reads' samples as they are, in place nothing)
		launch_degrade(a, dst, bits, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, s);
	if ((rc = launch_status()) || device_resident)
		return rc;
	std::vector<uint32_t> got(nreads);
	return st.fetch_elems(out, g.sig.p, sizeof(int16_t), StreamsIn{ nullptr, nullptr, nullptr, off, n, got.data(), out });
}

// ------------------------------------------------------------------ verify: the digest of samples, of decoded streams; decode and compare
//
// The three calls share make_verify_plan and the launchers beside launch_depress_pa (press_methods.hip); the decoding
// two write their samples into g.rsig at the caller's off[] and hand nothing of them out.

extern "C" int press_hip_signal_crc32(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				      uint64_t total_samples, uint32_t *crc, int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, nreads && (!sig || !off || !n || !crc), nreads, device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_verify_plan(NONE, total_samples, nreads, !device_resident);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;
	SamplesIn in = { sig, off, n };
	Staged st(nreads, s);
	if (!device_resident && (rc = st.samples_in(in, total_samples, in)))
		return rc;
	bind_io(a, in);
	if ((rc = launch_signal_crc(plan, a, device_resident ? crc : (uint32_t *) g.vf_out.p, s)) || device_resident)
		return rc;
	return st.fetch_tables({ { crc, g.vf_out.p, (size_t) nreads * 4 } });
}

extern "C" int press_hip_depress_crc_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					   uint32_t nreads, const uint64_t *off, const uint32_t *n, uint64_t total_samples,
					   uint32_t *crc, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = args_ok(method, NONE, nreads && (!in || !in_off || !in_len || !off || !n || !crc || !out_n), nreads, nullptr, "");
	if (rc || (rc = device_ready(method, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_verify_plan(method, total_samples, nreads, !device_resident);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, (int16_t *) plan.ptr(&Ctx::rsig) };
	StreamsIn io = host;
	Staged st(nreads, s);
	if (!device_resident && (rc = st.streams(host, total_samples, false, g.arena, g.arena_off, io)))
		return rc;
	bind_io(a, io);
	if ((rc = launch_depress_crc(plan, a, device_resident ? crc : (uint32_t *) g.vf_out.p, s)) || device_resident)
		return rc;
	return st.fetch_tables({ { crc, g.vf_out.p, (size_t) nreads * 4 }, { out_n, g.outn.p, (size_t) nreads * 4 } });
}

// press_hip_verify_batch (bits == 0) and press_hip_verify_degraded_batch
static int verify_batch(int method, uint32_t bits, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
			uint32_t nreads, const int16_t *sig, const uint64_t *off, const uint32_t *n,
			uint64_t total_samples, uint32_t *first_bad, uint32_t *out_n, uint32_t *nbad,
			int device_resident)
{
	API_LOCK;
	int rc = bits_ok(bits);
	if (rc)
		return rc;
	rc = args_ok(method, NONE, !nbad || (nreads && (!in || !in_off || !in_len || !sig || !off || !n || !first_bad || !out_n)), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(method, NONE)))
		return rc;
	if (nreads == 0) {
		if (!device_resident)
			*nbad = 0;
		return 0;
	}
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_verify_plan(method, total_samples, nreads, !device_resident);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, nullptr };
	StreamsIn io = host;
	SamplesIn want = { sig, off, n };
	uint32_t *fb = first_bad, *nb = nbad;
	Staged st(nreads, s);
	if (!device_resident) { // host pointers: the streams as depress stages them, the samples where press stages them
		if ((rc = st.streams(host, total_samples, true, g.arena, g.arena_off, io)) || (rc = st.samples(want, total_samples, want)))
			return rc;
		fb = (uint32_t *) g.vf_out.p;
		nb = fb + nreads;
	}
	io.sig = (int16_t *) plan.ptr(&Ctx::rsig); // the decode goes to the library's samples
	bind_io(a, io);
	if ((rc = launch_verify(plan, a, want.sig, fb, nb, s, bits)) || device_resident)
		return rc;
	return st.fetch_tables({ { first_bad, fb, (size_t) nreads * 4 }, { nbad, nb, 4 }, { out_n, g.outn.p, (size_t) nreads * 4 } });
}

extern "C" int press_hip_verify_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
				      uint32_t nreads, const int16_t *sig, const uint64_t *off, const uint32_t *n,
				      uint64_t total_samples, uint32_t *first_bad, uint32_t *out_n, uint32_t *nbad,
				      int device_resident)
{
	return verify_batch(method, 0, in, in_off, in_len, nreads, sig, off, n, total_samples, first_bad, out_n, nbad, device_resident);
}

extern "C" int press_hip_verify_degraded_batch(int method, uint32_t bits, const uint8_t *in, const uint64_t *in_off,
					       const uint64_t *in_len, uint32_t nreads, const int16_t *sig, const uint64_t *off,
					       const uint32_t *n, uint64_t total_samples, uint32_t *first_bad, uint32_t *out_n,
					       uint32_t *nbad, int device_resident)
{
	return verify_batch(method, bits, in, in_off, in_len, nreads, sig, off, n, total_samples, first_bad, out_n, nbad, device_resident);
}

// ------------------------------------------------------------------ the stall methods (press_stall.hip)
//
// press_hip_press_batch / press_hip_depress_batch with a stall id in the place of the method: the same checks, the same
// staging, one launch chain each (launch_stall_press / launch_stall_depress).

static int stall_args_ok(int stall_method, bool null_arg, uint32_t nreads, const void *dev_arena)
{
	if (!stall_ok(stall_method))
		return set_error(PRESS_HIP_EARG, "stall method %d: 0 rccm_svbbe21_zd, 1 dstall_fz_1500, 2 dstall_fz", stall_method);
	return args_ok(NONE, NONE, null_arg, nreads, dev_arena, "sig");
}

extern "C" int press_hip_stall_press_batch(int stall_method, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					   uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
					   uint32_t *stall, int device_resident)
{
	API_LOCK;
	int rc = stall_args_ok(stall_method, nreads && (!sig || !off || !n || !out || !out_off || !out_len), nreads,
			       device_resident ? sig : nullptr);
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const StallPlan plan = make_stall_plan(stall_method, total_samples, nreads, false, !device_resident);
	if ((rc = plan.all.reserve()))
		return rc;
	BatchArgs a{};
	a.nreads = nreads;
	const SlotsOut host = { out, out_off, out_len };
	SamplesIn in = { sig, off, n };
	SlotsOut so = host;
	Staged st(nreads, s);
	if (!device_resident && ((rc = check_slots(out_off, nreads)) || (rc = st.layout(off, n, total_samples, "the sample range", true)) ||
				 (rc = st.slots(host, so)) || (rc = st.samples(in, total_samples, in))))
		return rc;
	bind_io(a, in);
	bind_io(a, so);
	uint32_t *dstall = device_resident ? stall : stall ? (uint32_t *) g.sl_stall.p : nullptr;
	if ((rc = launch_stall_press(stall_method, plan, a, dstall, s)) || device_resident)
		return rc;
	if (stall)
		HIPCHK(hipMemcpyAsync(stall, dstall, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	return st.fetch_streams(host);
}

extern "C" int press_hip_stall_depress_batch(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint32_t nreads,
					     int16_t *sig, const uint64_t *off, const uint32_t *n, uint64_t total_samples,
					     uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = args_ok(NONE, NONE, nreads && (!in || !in_off || !in_len || !sig || !off || !n || !out_n), nreads,
			 device_resident ? sig : nullptr, "sig");
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const StallPlan plan = make_stall_plan(PRESS_HIP_STALL_DSTALL_FZ, total_samples, nreads, true, !device_resident);
	if ((rc = plan.all.reserve()))
		return rc;
	DecodeArgs a{};
	a.nreads = nreads;
	const StreamsIn host = { in, in_off, in_len, off, n, out_n, sig };
	StreamsIn io = host;
	Staged st(nreads, s);
	if (!device_resident && (rc = st.streams(host, total_samples, true, g.arena, g.arena_off, io)))
		return rc;
	bind_io(a, io);
	if ((rc = launch_stall_depress(plan, a, s)) || device_resident)
		return rc;
	return st.fetch_samples(host);
}

// ------------------------------------------------------------------ the range-coder family: every coder on every layout
//
// press_hip_press_batch / press_hip_depress_batch with a (coder, layout) pair in the place of the method: the same checks,
// the same staging, the same launch through the pair's row (rcf_method); press adds k_rcf_raw where the caller asks.

static int rcf_args_ok(int coder, int layout, bool null_arg, uint32_t nreads, const void *dev_arena)
{
	if (!rcf_ok(coder, layout))
		return set_error(PRESS_HIP_EARG, "range-coder family: coder %d (0 rc, 1 rcc, 2 rccm, 3 rccdf), layout %d (0 vbe21, 1 vbbe21, 2 vbsbe21, 3 vbsse21)",
				 coder, layout);
	return args_ok(NONE, NONE, null_arg, nreads, dev_arena, "sig");
}

extern "C" uint64_t press_hip_rcf_bound(int coder, int layout, uint32_t n)
{
	return rcf_ok(coder, layout) ? bound_vbzd(n) : 0; // press.c:5422 ... 7613: vb1e2_zd_bound_16 for all sixteen
}

extern "C" int press_hip_rcf_press_batch(int coder, int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					 uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint8_t *raw,
					 int device_resident)
{
	API_LOCK;
	int rc = rcf_args_ok(coder, layout, nreads && (!sig || !off || !n || !out || !out_off || !out_len), nreads,
			     device_resident ? sig : nullptr);
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	ScratchPlan plan = make_plan(rcf_method(coder, layout), total_samples, nreads, false);
	if (raw && !device_resident)
		plan.need(&Ctx::vf_raw, nreads);
	if ((rc = plan.reserve()))
		return rc;
	BatchArgs a;
	plan.bind(a);
	a.nreads = nreads;
	const SlotsOut host = { out, out_off, out_len };
	SamplesIn in = { sig, off, n };
	SlotsOut so = host;
	Staged st(nreads, s);
	if (!device_resident && ((rc = check_slots(out_off, nreads)) || (rc = st.layout(off, n, total_samples, "the sample range", true)) ||
				 (rc = st.slots(host, so)) || (rc = st.samples(in, total_samples, in))))
		return rc;
	bind_io(a, in);
	bind_io(a, so);
	uint8_t *draw = device_resident ? raw : raw ? (uint8_t *) g.vf_raw.p : nullptr;
	if ((rc = launch_press(plan, a, s)))
		return rc;
	if (draw) {
		launch_rcf_raw(a, draw, s);
		if ((rc = launch_status()))
			return rc;
	}
	if (device_resident)
		return 0;
	if (raw)
		HIPCHK(hipMemcpyAsync(raw, draw, nreads, hipMemcpyDeviceToHost, s));
	return st.fetch_streams(host);
}

extern "C" int press_hip_rcf_depress_batch(int coder, int layout, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					   uint32_t nreads, int16_t *sig, const uint64_t *off, const uint32_t *n, uint64_t total_samples,
					   uint32_t *out_n, int device_resident)
{
	API_LOCK;
	const int rc = rcf_args_ok(coder, layout, nreads && (!in || !in_off || !in_len || !sig || !off || !n || !out_n), nreads,
				   device_resident ? sig : nullptr);
	return rc ? rc : row_depress(rcf_method(coder, layout), NONE, { in, in_off, in_len, off, n, out_n, sig }, nreads, total_samples, device_resident);
}

// ------------------------------------------------------------------ the Rice family and the per-read Huffman family
//
// As the range-coder family with the layout alone in the place of the pair: the rows of RICE_METHODS (Golomb-Rice on every
// layout) or of DHUF_METHODS (a code per read on every layout).  Press reports a byte of every read where the caller asks -
// the Rice parameter k, the longest code -, and the sizes call runs the chain as far as the sizes.  One function each for
// press, sizes and depress: a family is its rows and its name in the error text.

struct PrefixFamily {
	const Method *rows;
	const char *name;
};
static constexpr PrefixFamily RICE_FAMILY = { RICE_METHODS, "Rice" }, DHUF_FAMILY = { DHUF_METHODS, "per-read Huffman" };

static int prefix_args_ok(const PrefixFamily &f, int layout, bool null_arg, uint32_t nreads, const void *dev_arena)
{
	if (!rice_ok(layout))
		return set_error(PRESS_HIP_EARG, "%s family: layout %d (0 vbe21, 1 vbbe21, 2 vbsbe21, 3 vbsse21)", f.name, layout);
	return args_ok(NONE, NONE, null_arg, nreads, dev_arena, "sig");
}

// byte: k[] or maxlen[]
static int prefix_press(const PrefixFamily &f, int layout, SamplesIn in, const SlotsOut &host, uint32_t nreads, uint64_t total_samples,
			uint8_t *byte, int device_resident)
{
	API_LOCK;
	int rc = prefix_args_ok(f, layout, nreads && (!in.sig || !in.off || !in.n || !host.out || !host.out_off || !host.out_len), nreads,
				device_resident ? in.sig : nullptr);
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	ScratchPlan plan = make_plan(f.rows[layout], total_samples, nreads, false);
	if (byte && !device_resident)
		plan.need(&Ctx::ri_k, nreads);
	if ((rc = plan.reserve()))
		return rc;
	BatchArgs a;
	plan.bind(a);
	a.nreads = nreads;
	SlotsOut so = host;
	Staged st(nreads, s);
	if (!device_resident && ((rc = check_slots(host.out_off, nreads)) || (rc = st.layout(in.off, in.n, total_samples, "the sample range", true)) ||
				 (rc = st.slots(host, so)) || (rc = st.samples(in, total_samples, in))))
		return rc;
	bind_io(a, in);
	bind_io(a, so);
	a.ri_k = device_resident ? byte : byte ? (uint8_t *) g.ri_k.p : nullptr;
	if ((rc = launch_press(plan, a, s)) || device_resident)
		return rc;
	if (byte)
		HIPCHK(hipMemcpyAsync(byte, a.ri_k, nreads, hipMemcpyDeviceToHost, s));
	return st.fetch_streams(host);
}

static int prefix_sizes(const PrefixFamily &f, int layout, SamplesIn in, uint32_t nreads, uint64_t total_samples, uint64_t *need,
			uint8_t *byte, int device_resident)
{
	API_LOCK;
	int rc = prefix_args_ok(f, layout, nreads && (!in.sig || !in.off || !in.n || !need), nreads, device_resident ? in.sig : nullptr);
	if (rc || (rc = device_ready(NONE, NONE)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const size_t nr = (size_t) nreads + 1;
	const Method &m = f.rows[layout];
	ScratchPlan plan = make_plan(m, total_samples, nreads, false);
	plan.need(&Ctx::pslot, nr * 8); // the slot table the chain is run against: all zeros
	if (!device_resident)
		plan.need(&Ctx::pneed, nr * 8).need(&Ctx::ri_k, nreads);
	if ((rc = plan.reserve()))
		return rc;
	BatchArgs a;
	plan.bind(a);
	a.nreads = nreads;
	Staged st(nreads, s);
	if (!device_resident && (rc = st.samples_in(in, total_samples, in)))
		return rc;
	bind_io(a, in);
	uint64_t *dneed = device_resident ? need : (uint64_t *) g.pneed.p;
	HIPCHK(hipMemsetAsync(g.pslot.p, 0, nr * 8, s));
	a.out_off = (const uint64_t *) g.pslot.p;
	a.out_len = dneed;
	a.ri_k = device_resident ? byte : byte ? (uint8_t *) g.ri_k.p : nullptr;
	launch_ex_prefix_sizes(a, m.exfmt, m.ent, dneed, s);
	if ((rc = launch_status()) || device_resident)
		return rc;
	return st.fetch_tables({ { need, dneed, (size_t) nreads * 8 }, { byte, a.ri_k, nreads } });
}

static int prefix_depress(const PrefixFamily &f, int layout, const StreamsIn &host, uint32_t nreads, uint64_t total_samples, int device_resident)
{
	API_LOCK;
	const int rc = prefix_args_ok(f, layout, nreads && (!host.in || !host.in_off || !host.in_len || !host.sig || !host.off || !host.n || !host.out_n),
				      nreads, device_resident ? host.sig : nullptr);
	return rc ? rc : row_depress(f.rows[layout], NONE, host, nreads, total_samples, device_resident);
}

extern "C" uint64_t press_hip_rice_bound(int layout, uint32_t n)
{
	return rice_ok(layout) ? bound_vbzd(n) : 0; // press.c:4985, 5072, 5178, 5284: vb1e2_zd_bound_16 for all four
}

extern "C" int press_hip_rice_press_batch(int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					  uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint8_t *k,
					  int device_resident)
{
	return prefix_press(RICE_FAMILY, layout, { sig, off, n }, { out, out_off, out_len }, nreads, total_samples, k, device_resident);
}

extern "C" int press_hip_rice_press_sizes(int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					  uint64_t total_samples, uint64_t *need, uint8_t *k, int device_resident)
{
	return prefix_sizes(RICE_FAMILY, layout, { sig, off, n }, nreads, total_samples, need, k, device_resident);
}

extern "C" int press_hip_rice_depress_batch(int layout, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					    uint32_t nreads, int16_t *sig, const uint64_t *off, const uint32_t *n, uint64_t total_samples,
					    uint32_t *out_n, int device_resident)
{
	return prefix_depress(RICE_FAMILY, layout, { in, in_off, in_len, off, n, out_n, sig }, nreads, total_samples, device_resident);
}

// what the repair rounds and the serial walk of the last press_hip_rice_depress_batch had to touch
extern "C" int press_hip_rice_repairs(uint32_t counts[3])
{
	API_LOCK;
	if (!counts)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	int rc = device_ready(NONE, NONE);
	if (rc)
		return rc;
	counts[0] = counts[1] = counts[2] = 0;
	if (!g.ri_ctl.p)
		return 0;
	uint32_t w[4];
	HIPCHK(hipStreamSynchronize(g.stream()));
	HIPCHK(hipMemcpy(w, g.ri_ctl.p, sizeof w, hipMemcpyDeviceToHost));
	counts[0] = w[1], counts[1] = w[2], counts[2] = w[3];
	return 0;
}

extern "C" uint64_t press_hip_huffman_bound(int layout, uint32_t n)
{
	return rice_ok(layout) ? bound_vbzd(n) : 0; // press.c:3965, 4061, 4177, 4293: vb1e2_zd_bound_16 for all four
}

extern "C" int press_hip_huffman_press_batch(int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					     uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
					     uint8_t *maxlen, int device_resident)
{
	return prefix_press(DHUF_FAMILY, layout, { sig, off, n }, { out, out_off, out_len }, nreads, total_samples, maxlen, device_resident);
}

extern "C" int press_hip_huffman_press_sizes(int layout, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					     uint64_t total_samples, uint64_t *need, uint8_t *maxlen, int device_resident)
{
	return prefix_sizes(DHUF_FAMILY, layout, { sig, off, n }, nreads, total_samples, need, maxlen, device_resident);
}

extern "C" int press_hip_huffman_depress_batch(int layout, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					       uint32_t nreads, int16_t *sig, const uint64_t *off, const uint32_t *n,
					       uint64_t total_samples, uint32_t *out_n, int device_resident)
{
	return prefix_depress(DHUF_FAMILY, layout, { in, in_off, in_len, off, n, out_n, sig }, nreads, total_samples, device_resident);
}

// what the repair rounds and the serial walk of the last press_hip_huffman_depress_batch had to touch (the counters are
// the Rice family's: the last depress call of either family)
extern "C" int press_hip_huffman_repairs(uint32_t counts[3])
{
	return press_hip_rice_repairs(counts);
}
