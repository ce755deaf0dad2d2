// press_batch.hip - the batch entry points of include/press_hip.h (press, depress, symbol counts) and the page-locked
// staging engine behind their host-pointer form.

#include <algorithm>
#include <thread>
#include <vector>

#include "press_host.h"

using namespace ph;

// ------------------------------------------------------------------ host <-> device staging
//
// The host-pointer form of the batch calls (device_resident = 0) is what a caller like
// press/test.c uses: its buffers are ordinary (pageable) memory.  Copies go through two
// page-locked staging buffers of STAGE_BYTES: while the DMA engine moves one, the host fills
// (or drains) the other, several threads sharing the memcpy.  Buffers obtained from
// press_hip_host_alloc() are page-locked themselves and are copied by ONE DMA, no staging.
// Compressed streams travel densely: a gather kernel packs the slots' contents before the
// D2H (slots are sized by X_bound, several times their content), and the decoder's input is
// packed on the host while it is staged.

namespace {

constexpr size_t STAGE_BYTES = 32u << 20;
constexpr size_t DIRECT_MAX = 256u << 10; // below this a plain hipMemcpyAsync (HIP's own staging) is cheaper

struct Staging {
	void *buf[2] = { nullptr, nullptr };
	hipEvent_t ev[2];
	bool busy[2] = { false, false };
	bool made = false;
} stg;

int staging_init()
{
	if (stg.made)
		return 0;
	for (int k = 0; k < 2; k++) {
		HIPCHK(hipHostMalloc(&stg.buf[k], STAGE_BYTES, hipHostMallocDefault));
		HIPCHK(hipEventCreateWithFlags(&stg.ev[k], hipEventDisableTiming));
	}
	stg.made = true;
	return 0;
}

} // namespace

void ph::staging_release()
{
	if (!stg.made)
		return;
	for (int k = 0; k < 2; k++) {
		(void) hipEventDestroy(stg.ev[k]);
		(void) hipHostFree(stg.buf[k]);
		stg.buf[k] = nullptr;
		stg.busy[k] = false;
	}
	stg.made = false;
}

namespace {

int staging_wait(int k)
{
	if (stg.busy[k]) {
		HIPCHK(hipEventSynchronize(stg.ev[k]));
		stg.busy[k] = false;
	}
	return 0;
}

bool is_pinned(const void *p)
{
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess) {
		(void) hipGetLastError(); // ordinary memory is reported as an error: not one of ours
		return false;
	}
	return a.type == hipMemoryTypeHost;
}

// memcpy shared by a few threads (one core moves ~10 GB/s, the link 50+)
void par_memcpy(void *dst, const void *src, size_t n)
{
	constexpr size_t MIN_PART = 2u << 20;
	unsigned nt = (unsigned) (n / MIN_PART);
	if (nt > 6)
		nt = 6;
	if (nt < 2) {
		memcpy(dst, src, n);
		return;
	}
	const size_t part = (n / nt + 63) & ~(size_t) 63;
	std::vector<std::thread> th;
	for (unsigned t = 1; t < nt; t++) {
		const size_t o = (size_t) t * part;
		if (o >= n)
			break;
		const size_t l = o + part > n ? n - o : part;
		th.emplace_back([=] { memcpy((char *) dst + o, (const char *) src + o, l); });
	}
	memcpy(dst, src, part < n ? part : n);
	for (auto &t : th)
		t.join();
}

// host -> device, asynchronous on s as far as the source allows (returns when src may be reused
// unless src is page-locked)
int h2d(void *dst, const void *src, size_t n, hipStream_t s)
{
	if (!n)
		return 0;
	if (n <= DIRECT_MAX || is_pinned(src)) {
		HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s));
		return 0;
	}
	int rc = staging_init();
	if (rc)
		return rc;
	int k = 0;
	for (size_t o = 0; o < n; o += STAGE_BYTES, k ^= 1) {
		const size_t l = n - o < STAGE_BYTES ? n - o : STAGE_BYTES;
		if ((rc = staging_wait(k)))
			return rc;
		par_memcpy(stg.buf[k], (const char *) src + o, l);
		HIPCHK(hipMemcpyAsync((char *) dst + o, stg.buf[k], l, hipMemcpyHostToDevice, s));
		HIPCHK(hipEventRecord(stg.ev[k], s));
		stg.busy[k] = true;
	}
	return 0;
}

// Pieces of host memory <-> one dense device range, through the staging buffers.
struct Piece {
	uint8_t *host;   // where the piece lives on the host
	uint64_t dense;  // its offset in the dense range
	uint64_t len;
};

// pieces must be sorted by `dense` and must not overlap.  TO_DEV: host pieces -> dev[0, total);
// else dev[0, total) -> host pieces.  Synchronous for the host memory involved.
template <bool TO_DEV>
int staged_pieces(uint8_t *dev, uint64_t total, const std::vector<Piece> &pc, hipStream_t s)
{
	if (!total)
		return 0;
	int rc = staging_init();
	if (rc)
		return rc;
	size_t ip = 0; // first piece that may reach into the current chunk
	auto host_side = [&](int k, uint64_t o, uint64_t l) { // move the pieces' bytes of chunk [o, o + l)
		while (ip < pc.size() && pc[ip].dense + pc[ip].len <= o)
			ip++;
		for (size_t i = ip; i < pc.size() && pc[i].dense < o + l; i++) {
			const uint64_t a = pc[i].dense > o ? pc[i].dense : o;
			const uint64_t b = pc[i].dense + pc[i].len < o + l ? pc[i].dense + pc[i].len : o + l;
			if (b <= a)
				continue;
			uint8_t *h = pc[i].host + (a - pc[i].dense);
			uint8_t *g = (uint8_t *) stg.buf[k] + (a - o);
			if (TO_DEV)
				par_memcpy(g, h, b - a);
			else
				par_memcpy(h, g, b - a);
		}
	};
	int k = 0;
	if (TO_DEV) {
		for (uint64_t o = 0; o < total; o += STAGE_BYTES, k ^= 1) {
			const uint64_t l = total - o < STAGE_BYTES ? total - o : STAGE_BYTES;
			if ((rc = staging_wait(k)))
				return rc;
			host_side(k, o, l);
			HIPCHK(hipMemcpyAsync(dev + o, stg.buf[k], l, hipMemcpyHostToDevice, s));
			HIPCHK(hipEventRecord(stg.ev[k], s));
			stg.busy[k] = true;
		}
		return 0;
	}
	// device -> host: the DMA of chunk i+1 runs while the host drains chunk i
	uint64_t po = 0, pl = 0;
	int pk = -1;
	for (uint64_t o = 0; o < total; o += STAGE_BYTES, k ^= 1) {
		const uint64_t l = total - o < STAGE_BYTES ? total - o : STAGE_BYTES;
		if ((rc = staging_wait(k)))
			return rc;
		HIPCHK(hipMemcpyAsync(stg.buf[k], dev + o, l, hipMemcpyDeviceToHost, s));
		HIPCHK(hipEventRecord(stg.ev[k], s));
		stg.busy[k] = true;
		if (pk >= 0) {
			if ((rc = staging_wait(pk)))
				return rc;
			host_side(pk, po, pl);
		}
		pk = k;
		po = o;
		pl = l;
	}
	if (pk >= 0) {
		if ((rc = staging_wait(pk)))
			return rc;
		host_side(pk, po, pl);
	}
	return 0;
}

// dense[dense_off[r] ..) = arena[slot_off[r] .. + len[r]) - the streams of a batch packed back to back
// (16-byte aligned) for ONE copy to the host.  One workgroup per (read, 1/8 of its 4-KiB pieces).
__global__ __launch_bounds__(256) void k_gather_streams(const uint8_t *arena, const uint64_t *slot_off,
							const uint64_t *len, const uint64_t *dense_off, uint8_t *dense)
{
	const uint32_t r = blockIdx.x;
	const uint64_t l = len[r];
	if (l == PRESS_HIP_FAILED || l == 0)
		return;
	const uint8_t *src = arena + slot_off[r];
	uint8_t *dst = dense + dense_off[r];
	const uint64_t n16 = l / 16;
	for (uint64_t c = (uint64_t) blockIdx.y * 256 + threadIdx.x; c < n16; c += 256ull * gridDim.y) {
		uint4 v;
		__builtin_memcpy(&v, src + 16 * c, 16); // the slot may sit at any byte address
		*reinterpret_cast<uint4 *>(dst + 16 * c) = v;
	}
	if (blockIdx.y == 0 && threadIdx.x < (l & 15))
		dst[16 * n16 + threadIdx.x] = src[16 * n16 + threadIdx.x];
}

} // namespace

// EARG unless the sample ranges [off[r], off[r] + n[r]) of the non-empty reads are pairwise disjoint (host
// pointers only: the check reads off and n).  Press keeps per-read scratch at the read's sample offset, depress
// writes the read's samples there.  `order` returns the reads in ascending offset order.
static int check_disjoint(const uint64_t *off, const uint32_t *n, uint32_t nreads, const char *what,
			  std::vector<uint32_t> &order)
{
	order.resize(nreads);
	bool sorted = true;
	for (uint32_t r = 0; r < nreads; r++) {
		order[r] = r;
		sorted = sorted && (r == 0 || off[r] >= off[r - 1]);
	}
	if (!sorted)
		std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return off[x] < off[y]; });
	uint64_t end = 0;
	for (uint32_t i = 0; i < nreads; i++) {
		const uint32_t r = order[i];
		if (n[r] == 0)
			continue;
		if (off[r] < end)
			return set_error(PRESS_HIP_EARG, "%s of read %u overlaps another read's", what, r);
		end = off[r] + n[r];
	}
	return 0;
}

// The head of every host-pointer call: the sample layout checked, room for sig, off and n on the device, off and n
// on their way there.
static int stage_layout(const uint64_t *off, const uint32_t *n, uint32_t nreads, uint64_t total_samples, hipStream_t s,
			bool with_sig = true)
{
	for (uint32_t r = 0; r < nreads; r++) {
		if (off[r] & 7)
			return set_error(PRESS_HIP_EARG, "off[%u] = %llu is not a multiple of 8 samples", r,
					 (unsigned long long) off[r]);
		if (off[r] + n[r] > total_samples)
			return set_error(PRESS_HIP_EARG, "read %u ends beyond total_samples", r);
	}
	if ((with_sig && g.sig.reserve(total_samples * 2 + 64)) || g.off.reserve((size_t) nreads * 8) || g.nsamp.reserve((size_t) nreads * 4))
		return PRESS_HIP_EHIP;
	HIPCHK(hipMemcpyAsync(g.off.p, off, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(g.nsamp.p, n, (size_t) nreads * 4, hipMemcpyHostToDevice, s));
	return 0;
}

static int fetch_streams(uint8_t *out, const uint64_t *out_off, const std::vector<uint64_t> &rel, uint64_t *out_len,
			 uint32_t nreads, hipStream_t s);
static int fetch_elems(void *dst, const void *dev, size_t es, const uint64_t *off, const uint32_t *n, uint32_t *out_n,
		       uint32_t nreads, const std::vector<uint32_t> &order, hipStream_t s);
static int fetch_samples(int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t *out_n, uint32_t nreads,
			 const std::vector<uint32_t> &order, hipStream_t s)
{
	return fetch_elems(sig, g.sig.p, sizeof(int16_t), off, n, out_n, nreads, order, s);
}
// the source streams of a host-pointer depress packed back to back into `arena` while they are staged (the caller's slots
// may be far apart), their offsets and lengths into `offs` and g.lens2
static int stage_streams(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint32_t nreads, DevBuf &arena,
			 DevBuf &offs, std::vector<uint64_t> &doff, hipStream_t s);

extern "C" int press_hip_press_batch(int method, const int16_t *sig, const uint64_t *off, const uint32_t *n,
				     uint32_t nreads, uint64_t total_samples, uint8_t *out,
				     const uint64_t *out_off, uint64_t *out_len, int device_resident)
{
	API_ENTER;
	int rc = check_method(method);
	if (rc)
		return rc;
	if (nreads == 0)
		return 0;
	if (!sig || !off || !n || !out || !out_off || !out_len)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_plan(method, total_samples, nreads, false);
	if ((rc = plan.reserve()))
		return rc;
	BatchArgs a;
	plan.bind(a);
	a.nreads = nreads;

	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		a.sig = sig;
		a.off = off;
		a.nsamp = n;
		a.out = out;
		a.out_off = out_off;
		a.out_len = out_len;
		return launch_press(plan, a, s);
	}

	// host pointers: stage, run, copy back, synchronise
	for (uint32_t r = 0; r < nreads; r++)
		if (out_off[r + 1] < out_off[r])
			return set_error(PRESS_HIP_EARG, "out_off must be non-decreasing");
	{
		std::vector<uint32_t> order;
		if ((rc = check_disjoint(off, n, nreads, "the sample range", order)))
			return rc;
	}
	if ((rc = stage_layout(off, n, nreads, total_samples, s)))
		return rc;
	const uint64_t a0 = out_off[0], a1 = out_off[nreads];
	if (g.arena.reserve(a1 - a0 + 64) || g.arena_off.reserve(((size_t) nreads + 1) * 8) || g.lens.reserve((size_t) nreads * 8))
		return PRESS_HIP_EHIP;
	std::vector<uint64_t> rel(nreads + 1);
	for (uint32_t r = 0; r <= nreads; r++)
		rel[r] = out_off[r] - a0;
	HIPCHK(hipMemcpyAsync(g.arena_off.p, rel.data(), ((size_t) nreads + 1) * 8, hipMemcpyHostToDevice, s));
	if ((rc = h2d(g.sig.p, sig, total_samples * 2, s)))
		return rc;
	a.sig = (const int16_t *) g.sig.p;
	a.off = (const uint64_t *) g.off.p;
	a.nsamp = (const uint32_t *) g.nsamp.p;
	a.out = (uint8_t *) g.arena.p;
	a.out_off = (const uint64_t *) g.arena_off.p;
	a.out_len = (uint64_t *) g.lens.p;
	if ((rc = launch_press(plan, a, s)))
		return rc;
	return fetch_streams(out, out_off, rel, out_len, nreads, s);
}

// The tail of a host-pointer press: out_len, then the streams of g.arena (slot r at rel[r]) into the caller's slots.
static int fetch_streams(uint8_t *out, const uint64_t *out_off, const std::vector<uint64_t> &rel, uint64_t *out_len,
			 uint32_t nreads, hipStream_t s)
{
	int rc;
	HIPCHK(hipMemcpyAsync(out_len, g.lens.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	if (nreads <= 4) { // per-read calls: one small copy each
		for (uint32_t r = 0; r < nreads; r++) {
			if (out_len[r] == PRESS_HIP_FAILED || out_len[r] == 0)
				continue;
			HIPCHK(hipMemcpyAsync(out + out_off[r], (uint8_t *) g.arena.p + rel[r], out_len[r],
					      hipMemcpyDeviceToHost, s));
		}
		HIPCHK(hipStreamSynchronize(s));
		return 0;
	}
	// the streams packed back to back on the device, ONE pass over the link, scattered into the
	// caller's slots by the host
	std::vector<uint64_t> doff(nreads);
	std::vector<Piece> pc;
	pc.reserve(nreads);
	uint64_t dense = 0;
	for (uint32_t r = 0; r < nreads; r++) {
		doff[r] = dense;
		if (out_len[r] == PRESS_HIP_FAILED || out_len[r] == 0)
			continue;
		pc.push_back({ out + out_off[r], dense, out_len[r] });
		dense += (out_len[r] + 15) & ~15ull;
	}
	if (!dense)
		return 0;
	if (g.dense.reserve(dense + 64) || g.dense_off.reserve((size_t) nreads * 8))
		return PRESS_HIP_EHIP;
	HIPCHK(hipMemcpyAsync(g.dense_off.p, doff.data(), (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(k_gather_streams, dim3(nreads, 8), dim3(256), 0, s, (const uint8_t *) g.arena.p,
			   (const uint64_t *) g.arena_off.p, (const uint64_t *) g.lens.p, (const uint64_t *) g.dense_off.p,
			   (uint8_t *) g.dense.p);
	if ((rc = staged_pieces<false>((uint8_t *) g.dense.p, dense, pc, s)))
		return rc;
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// ------------------------------------------------------------------ packed press: the library lays the arena out

// what both packed calls check before any device call
static int packed_args_ok(int method, uint32_t align)
{
	if (!method_ok(method))
		return set_error(PRESS_HIP_EARG, "method %d is not available in the batch API", method);
	if (align == 0 || align > 4096 || (align & (align - 1)))
		return set_error(PRESS_HIP_EARG, "align = %u is not a power of two in 1 .. 4096", align);
	return 0;
}

// the head of their host-pointer form: the checks of press_hip_press_batch, then samples and layout on the device
static int packed_stage(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, uint64_t total_samples,
			BatchArgs &a, hipStream_t s)
{
	int rc;
	std::vector<uint32_t> order;
	if ((rc = check_disjoint(off, n, nreads, "the sample range", order)))
		return rc;
	if ((rc = stage_layout(off, n, nreads, total_samples, s)))
		return rc;
	if ((rc = h2d(g.sig.p, sig, total_samples * 2, s)))
		return rc;
	a.sig = (const int16_t *) g.sig.p;
	a.off = (const uint64_t *) g.off.p;
	a.nsamp = (const uint32_t *) g.nsamp.p;
	return 0;
}

extern "C" int press_hip_press_sizes(int method, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				     uint64_t total_samples, uint64_t *need, int device_resident)
{
	API_LOCK;
	int rc = packed_args_ok(method, 1);
	if (rc || (rc = ctx_init()) || (rc = check_method(method)))
		return rc;
	if (nreads == 0)
		return 0;
	if (!sig || !off || !n || !need)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_packed_plan(method, total_samples, nreads);
	if ((rc = plan.reserve()))
		return rc;
	BatchArgs a;
	plan.bind(a);
	a.nreads = nreads;
	PackArgs pk = { device_resident ? need : (uint64_t *) g.pneed.p, nullptr, (uint64_t *) g.pslot.p, 0, 1 };
	a.out_off = pk.slot;
	a.out_len = pk.need; // (an empty read's verdict of k_chunk_prep; the size kernel has the last word)
	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		a.sig = sig;
		a.off = off;
		a.nsamp = n;
		return launch_press_packed(plan, a, pk, PACK_SIZE, s);
	}
	if ((rc = packed_stage(sig, off, n, nreads, total_samples, a, s)) || (rc = launch_press_packed(plan, a, pk, PACK_SIZE, s)))
		return rc;
	HIPCHK(hipMemcpyAsync(need, pk.need, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

extern "C" int press_hip_press_packed(int method, const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				      uint64_t total_samples, uint8_t *out, uint64_t out_cap, uint32_t align,
				      uint64_t *out_off, uint64_t *out_len, int device_resident)
{
	API_LOCK;
	int rc = packed_args_ok(method, align);
	if (rc || (rc = ctx_init()) || (rc = check_method(method)))
		return rc;
	if (!out_off)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (nreads == 0) { // an empty batch has a layout too
		if (device_resident)
			HIPCHK(hipMemsetAsync(out_off, 0, 8, g.stream()));
		else
			out_off[0] = 0;
		return 0;
	}
	if (!sig || !off || !n || !out_len || (!out && out_cap))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_packed_plan(method, total_samples, nreads);
	if ((rc = plan.reserve()))
		return rc;
	BatchArgs a;
	plan.bind(a);
	a.nreads = nreads;
	PackArgs pk = { (uint64_t *) g.pneed.p, out_off, (uint64_t *) g.pslot.p, out_cap, align };
	a.out_off = pk.slot;
	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		a.sig = sig;
		a.off = off;
		a.nsamp = n;
		a.out = out;
		a.out_len = out_len;
		return launch_press_packed(plan, a, pk, PACK_SIZE | PACK_WRITE, s);
	}

	// host pointers: stage, size and lay out, read the arena's size back, press into an arena of that size, copy its
	// prefix back in one piece
	if (g.arena_off.reserve(((size_t) nreads + 1) * 8) || g.lens.reserve((size_t) nreads * 8))
		return PRESS_HIP_EHIP;
	pk.layout = (uint64_t *) g.arena_off.p;
	a.out_len = (uint64_t *) g.lens.p;
	if ((rc = packed_stage(sig, off, n, nreads, total_samples, a, s)) || (rc = launch_press_packed(plan, a, pk, PACK_SIZE, s)))
		return rc;
	HIPCHK(hipMemcpyAsync(out_off, pk.layout, ((size_t) nreads + 1) * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s)); // the one synchronisation besides the last: the arena's size
	const uint64_t bytes = out_off[nreads] < out_cap ? out_off[nreads] : out_cap; // what a read that fits can touch
	if (g.arena.reserve(bytes + 64))
		return PRESS_HIP_EHIP;
	// (padding and the gaps of the range coders travel with the streams: they reach the caller as zeros)
	if (bytes)
		HIPCHK(hipMemsetAsync(g.arena.p, 0, bytes, s));
	a.out = (uint8_t *) g.arena.p;
	if ((rc = launch_press_packed(plan, a, pk, PACK_WRITE, s)))
		return rc;
	HIPCHK(hipMemcpyAsync(out_len, g.lens.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	if (bytes <= DIRECT_MAX || is_pinned(out)) { // small, or page-locked: one DMA
		if (bytes)
			HIPCHK(hipMemcpyAsync(out, g.arena.p, bytes, hipMemcpyDeviceToHost, s));
	} else {
		const std::vector<Piece> pc = { { out, 0, bytes } };
		if ((rc = staged_pieces<false>((uint8_t *) g.arena.p, bytes, pc, s)))
			return rc;
	}
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

#ifndef TRAIN_WG_PER_CU
#define TRAIN_WG_PER_CU 2 // workgroups per CU of k_symbol_count's persistent grid
#endif

extern "C" int press_hip_symbol_counts(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				       uint64_t total_samples, uint64_t *counts, int device_resident)
{
	API_ENTER;
	int rc;
	if (nreads == 0)
		return 0;
	if (!sig || !off || !n || !counts)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	hipStream_t s = g.stream();
	const uint32_t mc = (uint32_t) (total_samples / CHUNK + nreads + 1); // (as ScratchPlan::max_chunks)
	int cus = 0;
	HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g.device));
	uint32_t grid = (uint32_t) std::max(cus, 1) * TRAIN_WG_PER_CU;
	if (g.chunks.reserve(train_scratch_bytes(mc)) || g.ctl.reserve(2 * sizeof(ChunkCtl)))
		return PRESS_HIP_EHIP;
	uint32_t *nchunks = &((ChunkCtl *) g.ctl.p)->nchunks;

	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		launch_symbol_counts(sig, off, n, nreads, counts, g.chunks.p, nchunks, mc, std::min(grid, mc), s);
		return launch_status();
	}

	// host pointers: stage, run, copy the counts back, synchronise
	if ((rc = stage_layout(off, n, nreads, total_samples, s)))
		return rc;
	uint64_t nch = 0;
	for (uint32_t r = 0; r < nreads; r++)
		nch += n[r] >= 2 ? (n[r] + CHUNK - 1) / CHUNK : 0;
	if (nch == 0)
		return 0;
	if (g.lens.reserve(257 * 8))
		return PRESS_HIP_EHIP;
	HIPCHK(hipMemcpyAsync(g.lens.p, counts, 257 * 8, hipMemcpyHostToDevice, s));
	if ((rc = h2d(g.sig.p, sig, total_samples * 2, s)))
		return rc;
	launch_symbol_counts((const int16_t *) g.sig.p, (const uint64_t *) g.off.p, (const uint32_t *) g.nsamp.p, nreads,
			     (uint64_t *) g.lens.p, g.chunks.p, nchunks, mc, (uint32_t) std::min<uint64_t>(grid, nch), s);
	if ((rc = launch_status()))
		return rc;
	HIPCHK(hipMemcpyAsync(counts, g.lens.p, 257 * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

extern "C" int press_hip_depress_batch(int method, const uint8_t *in, const uint64_t *in_off,
				       const uint64_t *in_len, uint32_t nreads, int16_t *sig,
				       const uint64_t *off, const uint32_t *n, uint64_t total_samples,
				       uint32_t *out_n, int device_resident)
{
	API_ENTER;
	int rc = check_method(method);
	if (rc)
		return rc;
	if (nreads == 0)
		return 0;
	if (!in || !in_off || !in_len || !sig || !off || !n || !out_n)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	hipStream_t s = g.stream();
	const ScratchPlan plan = make_plan(method, total_samples, nreads, true);
	if ((rc = plan.reserve()))
		return rc;
	DecodeArgs a;
	plan.bind(a);
	a.nreads = nreads;

	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		a.in = in;
		a.in_off = in_off;
		a.in_len = in_len;
		a.sig = sig;
		a.off = off;
		a.nsamp = n;
		a.out_n = out_n;
		return launch_depress(plan, a, s);
	}

	std::vector<uint32_t> order; // the reads in ascending slot order (for the staged copy back)
	if ((rc = check_disjoint(off, n, nreads, "the sample room", order)))
		return rc;
	if ((rc = stage_layout(off, n, nreads, total_samples, s)))
		return rc;
	std::vector<uint64_t> doff;
	if ((rc = stage_streams(in, in_off, in_len, nreads, g.arena, g.arena_off, doff, s)))
		return rc;
	a.in = (const uint8_t *) g.arena.p;
	a.in_off = (const uint64_t *) g.arena_off.p;
	a.in_len = (const uint64_t *) g.lens2.p;
	a.sig = (int16_t *) g.sig.p;
	a.off = (const uint64_t *) g.off.p;
	a.nsamp = (const uint32_t *) g.nsamp.p;
	a.out_n = (uint32_t *) g.outn.p;
	if ((rc = launch_depress(plan, a, s)))
		return rc;
	return fetch_samples(sig, off, n, out_n, nreads, order, s);
}

// The tail of a host-pointer depress: out_n, then the decoded elements (es bytes each: int16 samples of g.sig, floats of
// g.pa_out) of the device arena `dev` into the caller's rooms in `dst` (`order`: the reads in ascending room order,
// check_disjoint).
static int fetch_elems(void *dst, const void *dev, size_t es, const uint64_t *off, const uint32_t *n, uint32_t *out_n,
		       uint32_t nreads, const std::vector<uint32_t> &order, hipStream_t s)
{
	uint8_t *const sig = (uint8_t *) dst;
	const uint8_t *const dsig = (const uint8_t *) dev;
	HIPCHK(hipMemcpyAsync(out_n, g.outn.p, (size_t) nreads * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	if (nreads <= 4) {
		for (uint32_t r = 0; r < nreads; r++) {
			if (out_n[r] == UINT32_MAX || out_n[r] == 0)
				continue;
			HIPCHK(hipMemcpyAsync(sig + off[r] * es, dsig + off[r] * es, (size_t) out_n[r] * es, hipMemcpyDeviceToHost, s));
		}
		HIPCHK(hipStreamSynchronize(s));
		return 0;
	}
	// only the decoded samples of every read reach the caller's buffer (its padding between the
	// reads is left alone); reads in ascending slot order for the staged copy (the rooms are disjoint, and
	// out_n[r] <= n[r])
	std::vector<Piece> pc;
	pc.reserve(nreads);
	uint64_t end = 0;
	int rc;
	for (uint32_t i = 0; i < nreads; i++) {
		const uint32_t r = order[i];
		if (out_n[r] == UINT32_MAX || out_n[r] == 0)
			continue;
		if (out_n[r] > n[r])
			return set_error(PRESS_HIP_EHIP, "read %u decoded %u samples into a room of %u", r, out_n[r], n[r]);
		pc.push_back({ sig + off[r] * es, off[r] * es, (uint64_t) out_n[r] * es });
		end = (off[r] + out_n[r]) * es;
	}
	if (is_pinned(sig)) { // page-locked: the decoded ranges go straight to the caller, one DMA per run of reads
		size_t i = 0;
		while (i < pc.size()) {
			size_t k = i;
			// reads whose gaps are only the alignment padding travel together (the padding is overwritten)
			while (k + 1 < pc.size() && pc[k + 1].dense - (pc[k].dense + pc[k].len) < 128)
				k++;
			const uint64_t b0 = pc[i].dense, b1 = pc[k].dense + pc[k].len;
			HIPCHK(hipMemcpyAsync(sig + b0, dsig + b0, b1 - b0, hipMemcpyDeviceToHost, s));
			i = k + 1;
		}
		HIPCHK(hipStreamSynchronize(s));
		return 0;
	}
	if ((rc = staged_pieces<false>(const_cast<uint8_t *>(dsig), end, pc, s)))
		return rc;
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// Picoamperes: press_hip_depress_batch with the float arena `pa` in the place of sig.  A fused method's decode kernel
// writes the floats itself; the others decode into g.rsig and k_pa_convert follows (launch_depress_pa).
extern "C" int press_hip_depress_pa_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					  uint32_t nreads, float *pa, const uint64_t *off, const uint32_t *n,
					  uint64_t total_samples, const float *cal, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	if (!method_ok(method)) // (before any device call)
		return set_error(PRESS_HIP_EARG, "method %d is not available in the batch API", method);
	if (nreads && (!in || !in_off || !in_len || !pa || !off || !n || !cal || !out_n))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	int rc = ctx_init();
	if (rc || (rc = check_method(method)))
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
	a.sig = (int16_t *) plan.ptr(&Ctx::rsig); // (NULL for a fused method: its kernel has no use for it)

	if (device_resident) {
		if ((uintptr_t) pa & 15)
			return set_error(PRESS_HIP_EARG, "pa must be 16-byte aligned");
		a.in = in;
		a.in_off = in_off;
		a.in_len = in_len;
		a.off = off;
		a.nsamp = n;
		a.out_n = out_n;
		return launch_depress_pa(plan, a, pa, cal, s);
	}

	std::vector<uint32_t> order;
	if ((rc = check_disjoint(off, n, nreads, "the sample room", order)))
		return rc;
	if ((rc = stage_layout(off, n, nreads, total_samples, s, false)))
		return rc;
	std::vector<uint64_t> doff;
	if ((rc = stage_streams(in, in_off, in_len, nreads, g.arena, g.arena_off, doff, s)))
		return rc;
	HIPCHK(hipMemcpyAsync(g.pa_cal.p, cal, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	a.in = (const uint8_t *) g.arena.p;
	a.in_off = (const uint64_t *) g.arena_off.p;
	a.in_len = (const uint64_t *) g.lens2.p;
	a.off = (const uint64_t *) g.off.p;
	a.nsamp = (const uint32_t *) g.nsamp.p;
	a.out_n = (uint32_t *) g.outn.p;
	if ((rc = launch_depress_pa(plan, a, (float *) g.pa_out.p, (const float *) g.pa_cal.p, s)))
		return rc;
	return fetch_elems(pa, g.pa_out.p, sizeof(float), off, n, out_n, nreads, order, s);
}

// Normalised floats: press_hip_depress_pa_batch's general path for every method, with a calibration the device derives
// between the decoder and the converter (launch_depress_norm).
extern "C" int press_hip_depress_norm_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					    uint32_t nreads, float *out, const uint64_t *off, const uint32_t *n,
					    uint64_t total_samples, int32_t *stats, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	if (!method_ok(method)) // (before any device call)
		return set_error(PRESS_HIP_EARG, "method %d is not available in the batch API", method);
	if (nreads && (!in || !in_off || !in_len || !out || !off || !n || !out_n))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	int rc = ctx_init();
	if (rc || (rc = check_method(method)))
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
	a.sig = (int16_t *) plan.ptr(&Ctx::rsig);

	if (device_resident) {
		if ((uintptr_t) out & 15)
			return set_error(PRESS_HIP_EARG, "out must be 16-byte aligned");
		a.in = in;
		a.in_off = in_off;
		a.in_len = in_len;
		a.off = off;
		a.nsamp = n;
		a.out_n = out_n;
		return launch_depress_norm(plan, a, out, stats, s);
	}

	std::vector<uint32_t> order;
	if ((rc = check_disjoint(off, n, nreads, "the sample room", order)))
		return rc;
	if ((rc = stage_layout(off, n, nreads, total_samples, s, false)))
		return rc;
	std::vector<uint64_t> doff;
	if ((rc = stage_streams(in, in_off, in_len, nreads, g.arena, g.arena_off, doff, s)))
		return rc;
	a.in = (const uint8_t *) g.arena.p;
	a.in_off = (const uint64_t *) g.arena_off.p;
	a.in_len = (const uint64_t *) g.lens2.p;
	a.off = (const uint64_t *) g.off.p;
	a.nsamp = (const uint32_t *) g.nsamp.p;
	a.out_n = (uint32_t *) g.outn.p;
	if ((rc = launch_depress_norm(plan, a, (float *) g.pa_out.p, (int32_t *) g.st_stats.p, s)))
		return rc;
	if (stats)
		HIPCHK(hipMemcpyAsync(stats, g.st_stats.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	return fetch_elems(out, g.pa_out.p, sizeof(float), off, n, out_n, nreads, order, s);
}

// the scratch of a stats call that decodes nothing, and its DecodeArgs (sig / off / nsamp / out_n are the caller's)
static int stats_scratch(uint32_t nreads, uint64_t total_samples, DecodeArgs &a)
{
	a = DecodeArgs{};
	a.nreads = nreads;
	a.max_chunks = (uint32_t) (total_samples / CHUNK + nreads + 1); // (as ScratchPlan::max_chunks)
	if (g.pa_tile.reserve((size_t) a.max_chunks * sizeof(uint2)) || g.pa_ctl.reserve(64) || g.st_rows.reserve(stat_rows_bytes(nreads)) ||
	    g.st_read.reserve(stat_state_bytes(nreads)))
		return PRESS_HIP_EHIP;
	return 0;
}

static void stats_launch(const DecodeArgs &a, int32_t *stats, hipEvent_t *ev, hipStream_t s)
{
	launch_pa_tiles(a, (uint2 *) g.pa_tile.p, (uint32_t *) g.pa_ctl.p, s);
	launch_signal_stats(a, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, g.st_read.p, (uint32_t *) g.st_rows.p, stats,
			    nullptr, ev, s);
}

extern "C" int press_hip_signal_stats(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
				      uint64_t total_samples, int32_t *stats, int device_resident)
{
	API_LOCK;
	if (nreads && (!sig || !off || !n || !stats)) // (before any device call)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	int rc = ctx_init();
	if (rc)
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	DecodeArgs a;
	if ((rc = stats_scratch(nreads, total_samples, a)))
		return rc;
	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		a.sig = const_cast<int16_t *>(sig);
		a.off = off;
		a.nsamp = n;
		a.out_n = const_cast<uint32_t *>(n); // (every sample of a read counts; nothing is written)
		stats_launch(a, stats, nullptr, s);
		return launch_status();
	}

	// host pointers: stage, run, copy the stats back, synchronise
	std::vector<uint32_t> order;
	if ((rc = check_disjoint(off, n, nreads, "the sample range", order)))
		return rc;
	if ((rc = stage_layout(off, n, nreads, total_samples, s)))
		return rc;
	if (g.st_stats.reserve((size_t) nreads * 8))
		return PRESS_HIP_EHIP;
	if ((rc = h2d(g.sig.p, sig, total_samples * 2, s)))
		return rc;
	a.sig = (int16_t *) g.sig.p;
	a.off = (const uint64_t *) g.off.p;
	a.nsamp = (const uint32_t *) g.nsamp.p;
	a.out_n = (uint32_t *) g.nsamp.p;
	stats_launch(a, (int32_t *) g.st_stats.p, nullptr, s);
	if ((rc = launch_status()))
		return rc;
	HIPCHK(hipMemcpyAsync(stats, g.st_stats.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// Quantiles of a batch: press_hip_signal_stats' layout and staging, nq ranks in four launches (press_quant.hip)
extern "C" int press_hip_signal_quantiles(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					  uint64_t total_samples, const uint32_t *rank_num, const uint32_t *rank_den, uint32_t nq,
					  int32_t *q, int device_resident)
{
	API_LOCK;
	if (nq < 1 || nq > QMAX) // (before any device call)
		return set_error(PRESS_HIP_EARG, "nq = %u: 1 .. %u quantiles", nq, QMAX);
	if (!rank_num || !rank_den || (nreads && (!sig || !off || !n || !q)))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	for (uint32_t i = 0; i < nq; i++)
		if (rank_den[i] == 0 || rank_num[i] > rank_den[i])
			return set_error(PRESS_HIP_EARG, "rank %u: %u / %u is not in [0, 1]", i, rank_num[i], rank_den[i]);
	int rc = ctx_init();
	if (rc)
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	DecodeArgs a;
	if ((rc = stats_scratch(nreads, total_samples, a)))
		return rc;
	if (g.st_rows.reserve(quant_rows_bytes(nreads, nq)) || g.st_read.reserve(quant_state_bytes(nreads)))
		return PRESS_HIP_EHIP;
	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		a.sig = const_cast<int16_t *>(sig);
		a.off = off;
		a.nsamp = n;
		a.out_n = const_cast<uint32_t *>(n); // (every sample of a read counts; nothing is written)
		launch_pa_tiles(a, (uint2 *) g.pa_tile.p, (uint32_t *) g.pa_ctl.p, s);
		launch_signal_quantiles(a, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, g.st_read.p, (uint32_t *) g.st_rows.p,
					rank_num, rank_den, nq, q, nullptr, nullptr, s);
		return launch_status();
	}

	// host pointers: stage, run, copy the quantiles back, synchronise
	std::vector<uint32_t> order;
	if ((rc = check_disjoint(off, n, nreads, "the sample range", order)))
		return rc;
	if ((rc = stage_layout(off, n, nreads, total_samples, s)))
		return rc;
	if (g.st_stats.reserve((size_t) nreads * nq * 4))
		return PRESS_HIP_EHIP;
	if ((rc = h2d(g.sig.p, sig, total_samples * 2, s)))
		return rc;
	a.sig = (int16_t *) g.sig.p;
	a.off = (const uint64_t *) g.off.p;
	a.nsamp = (const uint32_t *) g.nsamp.p;
	a.out_n = (uint32_t *) g.nsamp.p;
	launch_pa_tiles(a, (uint2 *) g.pa_tile.p, (uint32_t *) g.pa_ctl.p, s);
	launch_signal_quantiles(a, (const uint2 *) g.pa_tile.p, (const uint32_t *) g.pa_ctl.p, g.st_read.p, (uint32_t *) g.st_rows.p, rank_num,
				rank_den, nq, (int32_t *) g.st_stats.p, nullptr, nullptr, s);
	if ((rc = launch_status()))
		return rc;
	HIPCHK(hipMemcpyAsync(q, g.st_stats.p, (size_t) nreads * nq * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// Chunk rows: press_hip_depress_norm_batch's decode and staging; the calibration is the rule's two quantiles or, without a
// rule, median and MAD; the writer of press_rows.hip takes the place of the float converter (launch_depress_chunks).
extern "C" int press_hip_depress_chunks_batch(int method, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
					      uint32_t nreads, void *rows, uint64_t nrows_cap, int dtype, uint32_t T, uint32_t overlap,
					      const uint64_t *row_first, const uint64_t *off, const uint32_t *n, uint64_t total_samples,
					      const press_hip_scale_rule *rule, int32_t *q, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	if (!method_ok(method)) // (before any device call)
		return set_error(PRESS_HIP_EARG, "method %d is not available in the batch API", method);
	if (dtype != PRESS_HIP_F32 && dtype != PRESS_HIP_F16 && dtype != PRESS_HIP_BF16)
		return set_error(PRESS_HIP_EARG, "dtype %d: PRESS_HIP_F32, PRESS_HIP_F16 or PRESS_HIP_BF16", dtype);
	if (T == 0 || T % 8 || overlap >= T)
		return set_error(PRESS_HIP_EARG, "T must be a positive multiple of 8 and overlap below T");
	if (rule && !scale_rule_ok(rule))
		return set_error(PRESS_HIP_EARG, "the scale rule is not valid (ranks num <= den, den > 0; finite floats; scale_min > 0)");
	if (nreads && (!in || !in_off || !in_len || !row_first || !off || !n || !out_n || (!rows && nrows_cap)))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	int rc = ctx_init();
	if (rc || (rc = check_method(method)))
		return rc;
	if (nreads == 0)
		return 0;
	hipStream_t s = g.stream();
	const size_t es = dtype == PRESS_HIP_F32 ? 4 : 2;
	ChunkArgs c = { rows, nrows_cap, dtype, T, overlap, row_first, total_samples, rule, q };
	DecodeArgs a;

	if (device_resident) {
		if ((uintptr_t) rows & 15)
			return set_error(PRESS_HIP_EARG, "rows must be 16-byte aligned");
		const ScratchPlan plan = make_chunks_plan(method, total_samples, nreads, false, 0);
		if ((rc = plan.reserve()))
			return rc;
		plan.bind(a);
		a.nreads = nreads;
		a.sig = (int16_t *) plan.ptr(&Ctx::rsig);
		a.in = in;
		a.in_off = in_off;
		a.in_len = in_len;
		a.off = off;
		a.nsamp = n;
		a.out_n = out_n;
		return launch_depress_chunks(plan, a, c, s);
	}

	// host pointers: row_first must be the plan of n[] (it decides what is written where); stage, run, one transfer of
	// the written prefix of the rows, q and out_n, synchronise
	const uint32_t S = T - overlap;
	uint64_t at = 0;
	for (uint32_t r = 0; r < nreads; r++) {
		if (row_first[r] != at)
			return set_error(PRESS_HIP_EARG, "row_first[%u] is not press_hip_chunk_plan's", r);
		at += chunk_rows_of(n[r], T, S);
	}
	if (row_first[nreads] != at)
		return set_error(PRESS_HIP_EARG, "row_first[%u] is not press_hip_chunk_plan's", nreads);
	const uint64_t written = at < nrows_cap ? at : nrows_cap;
	const ScratchPlan plan = make_chunks_plan(method, total_samples, nreads, true, written * T * es);
	if ((rc = plan.reserve()))
		return rc;
	plan.bind(a);
	a.nreads = nreads;
	a.sig = (int16_t *) plan.ptr(&Ctx::rsig);
	std::vector<uint32_t> order;
	if ((rc = check_disjoint(off, n, nreads, "the sample room", order)))
		return rc;
	if ((rc = stage_layout(off, n, nreads, total_samples, s, false)))
		return rc;
	std::vector<uint64_t> doff;
	if ((rc = stage_streams(in, in_off, in_len, nreads, g.arena, g.arena_off, doff, s)))
		return rc;
	HIPCHK(hipMemcpyAsync(g.ch_first.p, row_first, ((size_t) nreads + 1) * 8, hipMemcpyHostToDevice, s));
	a.in = (const uint8_t *) g.arena.p;
	a.in_off = (const uint64_t *) g.arena_off.p;
	a.in_len = (const uint64_t *) g.lens2.p;
	a.off = (const uint64_t *) g.off.p;
	a.nsamp = (const uint32_t *) g.nsamp.p;
	a.out_n = (uint32_t *) g.outn.p;
	c.rows = g.ch_rows.p;
	c.nrows_cap = written;
	c.row_first = (const uint64_t *) g.ch_first.p;
	c.q = (int32_t *) g.st_stats.p;
	if ((rc = launch_depress_chunks(plan, a, c, s)))
		return rc;
	if (q)
		HIPCHK(hipMemcpyAsync(q, g.st_stats.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(out_n, g.outn.p, (size_t) nreads * 4, hipMemcpyDeviceToHost, s));
	if (written)
		HIPCHK(hipMemcpyAsync(rows, g.ch_rows.p, written * T * es, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// Profiling aid: the device-resident press_hip_signal_stats with an event behind every kernel; synchronous.
// ms[0 .. 8): count / pick / count / pick of the median, then of the MAD.
extern "C" int press_hip_signal_stats_timed(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads,
					    uint64_t total_samples, int32_t *stats, float *ms)
{
	API_LOCK;
	if (!sig || !off || !n || !stats || !ms || !nreads)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	int rc = ctx_init();
	if (rc)
		return rc;
	if ((uintptr_t) sig & 15)
		return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
	hipStream_t s = g.stream();
	DecodeArgs a;
	if ((rc = stats_scratch(nreads, total_samples, a)))
		return rc;
	a.sig = const_cast<int16_t *>(sig);
	a.off = off;
	a.nsamp = n;
	a.out_n = const_cast<uint32_t *>(n);
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


static int stage_streams(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint32_t nreads, DevBuf &arena,
			 DevBuf &offs, std::vector<uint64_t> &doff, hipStream_t s)
{
	int rc;
	uint64_t dense = 0;
	doff.resize(nreads); // (the caller's: it is read by a copy that may still be queued when this returns)
	std::vector<Piece> pc;
	pc.reserve(nreads);
	for (uint32_t r = 0; r < nreads; r++) {
		doff[r] = dense;
		if (in_len[r])
			pc.push_back({ const_cast<uint8_t *>(in) + in_off[r], dense, in_len[r] });
		dense += in_len[r];
	}
	if (arena.reserve(dense + 64) || offs.reserve((size_t) nreads * 8) || g.lens2.reserve((size_t) nreads * 8) ||
	    g.outn.reserve((size_t) nreads * 4))
		return PRESS_HIP_EHIP;
	HIPCHK(hipMemcpyAsync(offs.p, doff.data(), (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(g.lens2.p, in_len, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	if (nreads <= 4) {
		for (const Piece &q : pc)
			HIPCHK(hipMemcpyAsync((uint8_t *) arena.p + q.dense, q.host, q.len, hipMemcpyHostToDevice, s));
	} else if ((rc = staged_pieces<true>((uint8_t *) arena.p, dense, pc, s))) {
		return rc;
	}
	return 0;
}

// ------------------------------------------------------------------ recode: streams in, streams out
//
// The two halves run one after the other on the stream, inside one call and one lock: the decode of `src` into the
// caller's samples (or the library's own, sig == NULL), the verdicts out_n turned into the sample counts of the press
// half (a refused read: 0), the press of `dst`.  The halves share the chunk table, the granules and the per-read records,
// which is fine in sequence - except for a fused pair (recode_fused), where the svb decode kernel writes the press half's
// chunk descriptors while it reads its own: that press has a table, a first-chunk list and a control block to itself.

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
		launch_recode_fused(da, pa, sm.key2, sm.slow5, dm.exfmt, dm.ent, s);
	} else {
		if ((rc = launch_depress(rp.d, da, s)))
			return rc;
		launch_recode_counts(da.out_n, (uint32_t *) g.rn.p, da.nreads, s);
		if (rp.keep_heads)
			launch_recode_refused(da.out_n, pa, (uint8_t *) g.rkeep.p, true, s);
		if ((rc = launch_press(rp.p, pa, s)))
			return rc;
	}
	launch_recode_refused(da.out_n, pa, rp.keep_heads ? (uint8_t *) g.rkeep.p : nullptr, false, s);
	return launch_status();
}

extern "C" int press_hip_recode_batch(int src_method, int dst_method, const uint8_t *in, const uint64_t *in_off,
				      const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
				      uint64_t total_samples, uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
				      int16_t *sig, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	if (!method_ok(src_method) || !method_ok(dst_method)) // (before any device call)
		return set_error(PRESS_HIP_EARG, "method %d -> %d is not available in the batch API", src_method, dst_method);
	int rc = ctx_init();
	if (rc || (rc = check_method(src_method)) || (rc = check_method(dst_method)))
		return rc;
	if (nreads == 0)
		return 0;
	if (!in || !in_off || !in_len || !n || !off || !out || !out_off || !out_len || !out_n)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	hipStream_t s = g.stream();
	const RecodePlan rp = make_recode_plan(src_method, dst_method, total_samples, nreads, sig != nullptr);
	if ((rc = rp.all.reserve()))
		return rc;
	DecodeArgs da;
	BatchArgs pa;
	rp.d.bind(da);
	rp.p.bind(pa);
	da.nreads = pa.nreads = nreads;

	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		da.in = in;
		da.in_off = in_off;
		da.in_len = in_len;
		da.sig = sig ? sig : (int16_t *) g.rsig.p;
		da.off = off;
		da.nsamp = n;
		da.out_n = out_n;
		pa.out = out;
		pa.out_off = out_off;
		pa.out_len = out_len;
		return launch_recode(rp, da, pa, s);
	}

	// host pointers: both calls' checks, the streams and the layout staged, the two halves, the copies back
	for (uint32_t r = 0; r < nreads; r++)
		if (out_off[r + 1] < out_off[r])
			return set_error(PRESS_HIP_EARG, "out_off must be non-decreasing");
	std::vector<uint32_t> order;
	if ((rc = check_disjoint(off, n, nreads, "the sample room", order)))
		return rc;
	if ((rc = stage_layout(off, n, nreads, total_samples, s, sig != nullptr)))
		return rc;
	std::vector<uint64_t> doff;
	if ((rc = stage_streams(in, in_off, in_len, nreads, g.rin, g.rin_off, doff, s)))
		return rc;
	const uint64_t a0 = out_off[0], a1 = out_off[nreads];
	if (g.arena.reserve(a1 - a0 + 64) || g.arena_off.reserve(((size_t) nreads + 1) * 8) || g.lens.reserve((size_t) nreads * 8))
		return PRESS_HIP_EHIP;
	std::vector<uint64_t> rel(nreads + 1);
	for (uint32_t r = 0; r <= nreads; r++)
		rel[r] = out_off[r] - a0;
	HIPCHK(hipMemcpyAsync(g.arena_off.p, rel.data(), ((size_t) nreads + 1) * 8, hipMemcpyHostToDevice, s));
	da.in = (const uint8_t *) g.rin.p;
	da.in_off = (const uint64_t *) g.rin_off.p;
	da.in_len = (const uint64_t *) g.lens2.p;
	da.sig = sig ? (int16_t *) g.sig.p : (int16_t *) g.rsig.p;
	da.off = (const uint64_t *) g.off.p;
	da.nsamp = (const uint32_t *) g.nsamp.p;
	da.out_n = (uint32_t *) g.outn.p;
	pa.out = (uint8_t *) g.arena.p;
	pa.out_off = (const uint64_t *) g.arena_off.p;
	pa.out_len = (uint64_t *) g.lens.p;
	if ((rc = launch_recode(rp, da, pa, s)))
		return rc;
	if (sig) {
		if ((rc = fetch_samples(sig, off, n, out_n, nreads, order, s)))
			return rc;
	} else {
		HIPCHK(hipMemcpyAsync(out_n, g.outn.p, (size_t) nreads * 4, hipMemcpyDeviceToHost, s));
	}
	return fetch_streams(out, out_off, rel, out_len, nreads, s);
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
		launch_recode_fused_packed(da, pa, sm.key2, sm.slow5, dm.exfmt, dm.ent, pk, phases, s);
	} else {
		if (phases & PACK_SIZE) {
			if ((rc = launch_depress(rp.d, da, s)))
				return rc;
			launch_recode_counts(da.out_n, (uint32_t *) g.rn.p, da.nreads, s);
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

// what both packed recodes check before any device call
static int recode_packed_args_ok(int src_method, int dst_method, uint32_t align)
{
	if (!method_ok(src_method) || !method_ok(dst_method))
		return set_error(PRESS_HIP_EARG, "method %d -> %d is not available in the batch API", src_method, dst_method);
	return packed_args_ok(dst_method, align);
}

// the head of their host-pointer form: the checks of press_hip_recode_batch, then the streams and the layout on the device
static int recode_packed_stage(const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, const uint32_t *n,
			       const uint64_t *off, uint32_t nreads, uint64_t total_samples, bool keep_samples, DecodeArgs &da,
			       std::vector<uint32_t> &order, std::vector<uint64_t> &doff, hipStream_t s)
{
	int rc;
	if ((rc = check_disjoint(off, n, nreads, "the sample room", order)))
		return rc;
	if ((rc = stage_layout(off, n, nreads, total_samples, s, keep_samples)))
		return rc;
	if ((rc = stage_streams(in, in_off, in_len, nreads, g.rin, g.rin_off, doff, s)))
		return rc;
	da.in = (const uint8_t *) g.rin.p;
	da.in_off = (const uint64_t *) g.rin_off.p;
	da.in_len = (const uint64_t *) g.lens2.p;
	da.sig = keep_samples ? (int16_t *) g.sig.p : (int16_t *) g.rsig.p;
	da.off = (const uint64_t *) g.off.p;
	da.nsamp = (const uint32_t *) g.nsamp.p;
	da.out_n = (uint32_t *) g.outn.p;
	return 0;
}

extern "C" int press_hip_recode_sizes(int src_method, int dst_method, const uint8_t *in, const uint64_t *in_off,
				      const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
				      uint64_t total_samples, uint64_t *need, int16_t *sig, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = recode_packed_args_ok(src_method, dst_method, 1);
	if (rc || (rc = ctx_init()) || (rc = check_method(src_method)) || (rc = check_method(dst_method)))
		return rc;
	if (nreads == 0)
		return 0;
	if (!in || !in_off || !in_len || !n || !off || !need || !out_n)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	hipStream_t s = g.stream();
	const RecodePlan rp = make_recode_packed_plan(src_method, dst_method, total_samples, nreads, sig != nullptr);
	if ((rc = rp.all.reserve()))
		return rc;
	DecodeArgs da;
	BatchArgs pa;
	rp.d.bind(da);
	rp.p.bind(pa);
	da.nreads = pa.nreads = nreads;
	PackArgs pk = { device_resident ? need : (uint64_t *) g.pneed.p, nullptr, (uint64_t *) g.pslot.p, 0, 1 };
	pa.out_off = pk.slot;
	pa.out_len = pk.need; // (as press_hip_press_sizes)
	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		da.in = in;
		da.in_off = in_off;
		da.in_len = in_len;
		da.sig = sig ? sig : (int16_t *) g.rsig.p;
		da.off = off;
		da.nsamp = n;
		da.out_n = out_n;
		return launch_recode_packed(rp, da, pa, pk, PACK_SIZE, s);
	}
	std::vector<uint32_t> order;
	std::vector<uint64_t> doff;
	if ((rc = recode_packed_stage(in, in_off, in_len, n, off, nreads, total_samples, sig != nullptr, da, order, doff, s)) ||
	    (rc = launch_recode_packed(rp, da, pa, pk, PACK_SIZE, s)))
		return rc;
	HIPCHK(hipMemcpyAsync(need, pk.need, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	if (sig)
		return fetch_samples(sig, off, n, out_n, nreads, order, s);
	HIPCHK(hipMemcpyAsync(out_n, g.outn.p, (size_t) nreads * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

extern "C" int press_hip_recode_packed(int src_method, int dst_method, const uint8_t *in, const uint64_t *in_off,
				       const uint64_t *in_len, const uint32_t *n, const uint64_t *off, uint32_t nreads,
				       uint64_t total_samples, uint8_t *out, uint64_t out_cap, uint32_t align, uint64_t *out_off,
				       uint64_t *out_len, int16_t *sig, uint32_t *out_n, int device_resident)
{
	API_LOCK;
	int rc = recode_packed_args_ok(src_method, dst_method, align);
	if (rc || (rc = ctx_init()) || (rc = check_method(src_method)) || (rc = check_method(dst_method)))
		return rc;
	if (!out_off)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (nreads == 0) { // an empty batch has a layout too
		if (device_resident)
			HIPCHK(hipMemsetAsync(out_off, 0, 8, g.stream()));
		else
			out_off[0] = 0;
		return 0;
	}
	if (!in || !in_off || !in_len || !n || !off || !out_len || !out_n || (!out && out_cap))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	hipStream_t s = g.stream();
	const RecodePlan rp = make_recode_packed_plan(src_method, dst_method, total_samples, nreads, sig != nullptr);
	if ((rc = rp.all.reserve()))
		return rc;
	DecodeArgs da;
	BatchArgs pa;
	rp.d.bind(da);
	rp.p.bind(pa);
	da.nreads = pa.nreads = nreads;
	PackArgs pk = { (uint64_t *) g.pneed.p, out_off, (uint64_t *) g.pslot.p, out_cap, align };
	pa.out_off = pk.slot;
	if (device_resident) {
		if ((uintptr_t) sig & 15)
			return set_error(PRESS_HIP_EARG, "sig must be 16-byte aligned");
		da.in = in;
		da.in_off = in_off;
		da.in_len = in_len;
		da.sig = sig ? sig : (int16_t *) g.rsig.p;
		da.off = off;
		da.nsamp = n;
		da.out_n = out_n;
		pa.out = out;
		pa.out_len = out_len;
		return launch_recode_packed(rp, da, pa, pk, PACK_SIZE | PACK_WRITE, s);
	}

	// host pointers: stage, decode and size, read the arena's size back, write into an arena of that size, copy its prefix
	// back in one piece
	if (g.arena_off.reserve(((size_t) nreads + 1) * 8) || g.lens.reserve((size_t) nreads * 8))
		return PRESS_HIP_EHIP;
	pk.layout = (uint64_t *) g.arena_off.p;
	pa.out_len = (uint64_t *) g.lens.p;
	std::vector<uint32_t> order;
	std::vector<uint64_t> doff;
	if ((rc = recode_packed_stage(in, in_off, in_len, n, off, nreads, total_samples, sig != nullptr, da, order, doff, s)) ||
	    (rc = launch_recode_packed(rp, da, pa, pk, PACK_SIZE, s)))
		return rc;
	HIPCHK(hipMemcpyAsync(out_off, pk.layout, ((size_t) nreads + 1) * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s)); // the one synchronisation besides the last: the arena's size
	const uint64_t bytes = out_off[nreads] < out_cap ? out_off[nreads] : out_cap;
	if (g.arena.reserve(bytes + 64))
		return PRESS_HIP_EHIP;
	if (bytes) // (padding and the gaps of the range coders reach the caller as zeros)
		HIPCHK(hipMemsetAsync(g.arena.p, 0, bytes, s));
	pa.out = (uint8_t *) g.arena.p;
	if ((rc = launch_recode_packed(rp, da, pa, pk, PACK_WRITE, s)))
		return rc;
	HIPCHK(hipMemcpyAsync(out_len, g.lens.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	if (bytes <= DIRECT_MAX || is_pinned(out)) {
		if (bytes)
			HIPCHK(hipMemcpyAsync(out, g.arena.p, bytes, hipMemcpyDeviceToHost, s));
	} else {
		const std::vector<Piece> pc = { { out, 0, bytes } };
		if ((rc = staged_pieces<false>((uint8_t *) g.arena.p, bytes, pc, s)))
			return rc;
	}
	if (sig)
		return fetch_samples(sig, off, n, out_n, nreads, order, s);
	HIPCHK(hipMemcpyAsync(out_n, g.outn.p, (size_t) nreads * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}
