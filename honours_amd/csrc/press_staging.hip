// press_staging.hip - the host-pointer form of the batch calls (device_resident = 0): the page-locked staging engine, the
// layout checks that read the caller's tables, and the data movements of a staged call (struct Staged, press_host.h).
// The entry points of press_batch.hip run the same launch on the caller's pointers or on what this unit returns.

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

// press_hip_scratch_fill: the caller has synchronised the stream, so no DMA has either buffer as its source or target
void ph::staging_fill(int byte)
{
	if (!stg.made)
		return;
	for (int k = 0; k < 2; k++) {
		if (stg.busy[k])
			(void) hipEventSynchronize(stg.ev[k]);
		stg.busy[k] = false;
		memset(stg.buf[k], byte, STAGE_BYTES);
	}
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

// ------------------------------------------------------------------ layout checks (host pointers only: they read the tables)

// EARG unless the sample ranges [off[r], off[r] + n[r]) of the non-empty reads are pairwise disjoint.  Press keeps
// per-read scratch at the read's sample offset, depress writes the read's samples there.  `order` returns the reads in
// ascending offset order.
int ph::check_disjoint(const uint64_t *off, const uint32_t *n, uint32_t nreads, const char *what, std::vector<uint32_t> &order)
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

int ph::check_layout(const uint64_t *off, const uint32_t *n, uint32_t nreads, uint64_t total_samples)
{
	for (uint32_t r = 0; r < nreads; r++) {
		if (off[r] & 7)
			return set_error(PRESS_HIP_EARG, "off[%u] = %llu is not a multiple of 8 samples", r,
					 (unsigned long long) off[r]);
		if (off[r] + n[r] > total_samples)
			return set_error(PRESS_HIP_EARG, "read %u ends beyond total_samples", r);
	}
	return 0;
}

int ph::check_slots(const uint64_t *out_off, uint32_t nreads)
{
	for (uint32_t r = 0; r < nreads; r++)
		if (out_off[r + 1] < out_off[r])
			return set_error(PRESS_HIP_EARG, "out_off must be non-decreasing");
	return 0;
}

// ------------------------------------------------------------------ the movements of a staged call

// The head of every host-pointer call: the sample layout checked, room for sig, off and n on the device, off and n
// on their way there.
int Staged::layout(const uint64_t *off, const uint32_t *n, uint64_t total_samples, const char *what, bool with_sig)
{
	int rc;
	if ((what && (rc = check_disjoint(off, n, nreads, what, order))) || (rc = check_layout(off, n, nreads, total_samples)))
		return rc;
	if ((with_sig && g.sig.reserve(total_samples * 2 + 64)) || g.off.reserve((size_t) nreads * 8) || g.nsamp.reserve((size_t) nreads * 4))
		return PRESS_HIP_EHIP;
	HIPCHK(hipMemcpyAsync(g.off.p, off, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(g.nsamp.p, n, (size_t) nreads * 4, hipMemcpyHostToDevice, s));
	return 0;
}

int Staged::samples(const SamplesIn &h, uint64_t total_samples, SamplesIn &d)
{
	const int rc = h2d(g.sig.p, h.sig, total_samples * 2, s);
	d = { (const int16_t *) g.sig.p, (const uint64_t *) g.off.p, (const uint32_t *) g.nsamp.p };
	return rc;
}

int Staged::samples_in(const SamplesIn &h, uint64_t total_samples, SamplesIn &d)
{
	const int rc = layout(h.off, h.n, total_samples, "the sample range", true);
	return rc ? rc : samples(h, total_samples, d);
}

int Staged::slots(const SlotsOut &h, SlotsOut &d)
{
	const uint64_t a0 = h.out_off[0], a1 = h.out_off[nreads];
	if (g.arena.reserve(a1 - a0 + 64) || g.arena_off.reserve(((size_t) nreads + 1) * 8) || g.lens.reserve((size_t) nreads * 8))
		return PRESS_HIP_EHIP;
	rel.resize((size_t) nreads + 1);
	for (uint32_t r = 0; r <= nreads; r++)
		rel[r] = h.out_off[r] - a0;
	HIPCHK(hipMemcpyAsync(g.arena_off.p, rel.data(), ((size_t) nreads + 1) * 8, hipMemcpyHostToDevice, s));
	d = { (uint8_t *) g.arena.p, (const uint64_t *) g.arena_off.p, (uint64_t *) g.lens.p };
	return 0;
}

// The source streams are packed back to back into `arena` while they are staged (the caller's slots may be far apart),
// their offsets and lengths into `offs` and g.lens2.
int Staged::streams(const StreamsIn &h, uint64_t total_samples, bool sig_room, DevBuf &arena, DevBuf &offs, StreamsIn &d)
{
	int rc;
	if ((rc = layout(h.off, h.n, total_samples, "the sample room", sig_room)))
		return rc;
	uint64_t dense = 0;
	doff.resize(nreads); // (a member: it is read by a copy that may still be queued when this returns)
	std::vector<Piece> pc;
	pc.reserve(nreads);
	for (uint32_t r = 0; r < nreads; r++) {
		doff[r] = dense;
		if (h.in_len[r])
			pc.push_back({ const_cast<uint8_t *>(h.in) + h.in_off[r], dense, h.in_len[r] });
		dense += h.in_len[r];
	}
	if (arena.reserve(dense + 64) || offs.reserve((size_t) nreads * 8) || g.lens2.reserve((size_t) nreads * 8) ||
	    g.outn.reserve((size_t) nreads * 4))
		return PRESS_HIP_EHIP;
	HIPCHK(hipMemcpyAsync(offs.p, doff.data(), (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(g.lens2.p, h.in_len, (size_t) nreads * 8, hipMemcpyHostToDevice, s));
	if (nreads <= 4) {
		for (const Piece &q : pc)
			HIPCHK(hipMemcpyAsync((uint8_t *) arena.p + q.dense, q.host, q.len, hipMemcpyHostToDevice, s));
	} else if ((rc = staged_pieces<true>((uint8_t *) arena.p, dense, pc, s))) {
		return rc;
	}
	d = { (const uint8_t *) arena.p,      (const uint64_t *) offs.p, (const uint64_t *) g.lens2.p, (const uint64_t *) g.off.p,
	      (const uint32_t *) g.nsamp.p,  (uint32_t *) g.outn.p,     sig_room ? (int16_t *) g.sig.p : h.sig };
	return 0;
}

// The tail of a host-pointer call whose results are per-read tables and nothing else
int Staged::push(void *dev, const void *src, size_t bytes) { return h2d(dev, src, bytes, s); }

int Staged::fetch_tables(std::initializer_list<Table> tables)
{
	for (const Table &t : tables)
		if (t.dst)
			HIPCHK(hipMemcpyAsync(t.dst, t.dev, t.bytes, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return 0;
}

// The tail of a host-pointer press: out_len, then the streams of g.arena (slot r at rel[r]) into the caller's slots.
int Staged::fetch_streams(const SlotsOut &h)
{
	int rc;
	uint8_t *const out = h.out;
	uint64_t *const out_len = h.out_len;
	HIPCHK(hipMemcpyAsync(out_len, g.lens.p, (size_t) nreads * 8, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	if (nreads <= 4) { // per-read calls: one small copy each
		for (uint32_t r = 0; r < nreads; r++) {
			if (out_len[r] == PRESS_HIP_FAILED || out_len[r] == 0)
				continue;
			HIPCHK(hipMemcpyAsync(out + h.out_off[r], (uint8_t *) g.arena.p + rel[r], out_len[r],
					      hipMemcpyDeviceToHost, s));
		}
		HIPCHK(hipStreamSynchronize(s));
		return 0;
	}
	// the streams packed back to back on the device, ONE pass over the link, scattered into the
	// caller's slots by the host
	doff.resize(nreads); // (the source streams' table, if any, has long been copied: out_len came back behind it)
	std::vector<Piece> pc;
	pc.reserve(nreads);
	uint64_t dense = 0;
	for (uint32_t r = 0; r < nreads; r++) {
		doff[r] = dense;
		if (out_len[r] == PRESS_HIP_FAILED || out_len[r] == 0)
			continue;
		pc.push_back({ out + h.out_off[r], dense, out_len[r] });
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

// The tail of a host-pointer depress: out_n, then the decoded elements (es bytes each: int16 samples of g.sig, floats of
// g.pa_out) of the device arena `dev` into the caller's rooms in `dst` (`order`: the reads in ascending room order,
// check_disjoint).
int Staged::fetch_elems(void *dst, const void *dev, size_t es, const StreamsIn &h)
{
	uint8_t *const sig = (uint8_t *) dst;
	const uint8_t *const dsig = (const uint8_t *) dev;
	const uint64_t *const off = h.off;
	uint32_t *const out_n = h.out_n;
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
		if (out_n[r] > h.n[r])
			return set_error(PRESS_HIP_EHIP, "read %u decoded %u samples into a room of %u", r, out_n[r], h.n[r]);
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

int Staged::fetch_samples(const StreamsIn &h) { return fetch_elems(h.sig, g.sig.p, sizeof(int16_t), h); }

// The tail of the packed calls: the first `bytes` of a dense device arena into dst.  Small, or page-locked: one DMA;
// else through the staging buffers.  Not synchronised.
int Staged::fetch_prefix(void *dst, void *dev, uint64_t bytes)
{
	if (bytes <= DIRECT_MAX || is_pinned(dst)) {
		if (bytes)
			HIPCHK(hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, s));
		return 0;
	}
	const std::vector<Piece> pc = { { (uint8_t *) dst, 0, bytes } };
	return staged_pieces<false>((uint8_t *) dev, bytes, pc, s);
}
