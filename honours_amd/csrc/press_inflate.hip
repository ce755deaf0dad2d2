// press_inflate.hip - BLOW5 records inflated on the device (include/press_hip.h section 2zb): the read side of a file with
// record compression zlib.  The stream rules are press_inflate_walk.h's, the same code the host runs serially
// (ph::inflate_serial; tools/inflate_walk_check.cpp under a sanitizer); tests/_inflate.py is the model.
//
//   k_if_walk<WRITE>  one wave per record, one record per workgroup.  A DEFLATE stream is serial: every lane takes the
//                     walk's steps alike (bit reader, block headers, symbols), the lanes share the filling of the
//                     primary tables, the copy of a match and of a stored block, and the drain.
//       WRITE          literals and matches go into a ring of 32 KiB in LDS - the whole window, so a match never reads
//                      global memory back.  Output byte q stands at ring[(a0 + q) % 32768] with a0 the slot's address
//                      mod 16: whenever IF_DRAIN bytes have been produced, the ring's 16-byte words are the slot's
//                      16-byte words, and the drain is aligned uint4 loads from LDS and stores to global behind a head
//                      of at most 15 single bytes; what is short of a word waits for the next drain, the last one ends
//                      with single bytes.  The drain sums the Adler-32 of what it writes.  A record longer than its
//                      slot goes on as a count: the ring and the drain stop, nothing behind the slot is written.
//       !WRITE         the count alone: no ring, no output, no Adler-32 (press_hip_blow5_inflate_sizes, and the first
//                      walk of the packed form).
//   k_if_fields       one lane per record: parse_record's rules (blow5_reader.cpp) over inflated records.
//
// Bounds: a stream is read through ifw::BitIn, which loads nothing at or behind comp_len (checked against the arena
// first: REFUSED); a stored block is checked against comp_len before its copy; ring indices are masked; the drain
// writes [f, t) with t <= produced <= the slot's size.  Every pass of the walk's loops consumes a bit or ends it.

#include "press_host.h"
#include "press_inflate_walk.h"
#include "press_wave.h"

namespace ph {

namespace {

static_assert(ifw::OK == PRESS_HIP_INFLATE_OK && ifw::HEADER == PRESS_HIP_INFLATE_HEADER && ifw::TRUNCATED == PRESS_HIP_INFLATE_TRUNCATED &&
		      ifw::BTYPE == PRESS_HIP_INFLATE_BTYPE && ifw::STORED == PRESS_HIP_INFLATE_STORED && ifw::CODES == PRESS_HIP_INFLATE_CODES &&
		      ifw::SYMBOL == PRESS_HIP_INFLATE_SYMBOL && ifw::DISTANCE == PRESS_HIP_INFLATE_DISTANCE && ifw::ADLER == PRESS_HIP_INFLATE_ADLER &&
		      ifw::ROOM == PRESS_HIP_INFLATE_ROOM && ifw::REFUSED == PRESS_HIP_INFLATE_REFUSED,
	      "the walk's status bytes are the header's");

constexpr uint32_t IF_RING = 32768, IF_RM = IF_RING - 1; // the window of RFC 1951
constexpr uint32_t IF_DRAIN = PRESS_HIP_INFLATE_DRAIN;   // bytes produced between two drains
constexpr uint64_t IF_FAIL = PRESS_HIP_FAILED;
static_assert(IF_DRAIN + 1024 + 258 + 16 <= IF_RING - 258, "what waits for a drain is never overwritten");

struct IfArgs {
	const uint8_t *comp;
	const uint64_t *comp_off, *comp_len;
	uint64_t comp_bytes;
	uint32_t nrec;
	uint8_t *out;
	const uint64_t *out_off; // [nrec + 1] the slots (the packed form: PackArgs::slot)
	uint64_t *out_len;       // !WRITE: need
	uint8_t *status;
	const uint64_t *need;    // the packed form's second walk: the first one's result, else NULL
};

template <bool WRITE>
struct DevEnv {
	ifw::BitIn b;
	uint8_t *lens;
	ifw::Code lit, dist, cl;
	uint8_t *ring;
	uint8_t *dst;  // the slot
	uint64_t room; // its bytes
	uint64_t q, f; // bytes produced; bytes drained
	uint32_t a0, ln;
	uint32_t s1, s2; // the Adler-32 of the drained bytes
	bool writing;    // every byte so far has its place in the ring, and the slot holds them all

	__device__ uint32_t lane() const { return ln; }
	__device__ uint32_t nlanes() const { return 64; }
	__device__ void sync() { wave_lds_sync(); }
	__device__ uint32_t u(uint32_t v) const { return uni(v); }
	__device__ uint64_t produced() const { return q; }

	// [f, t) from the ring to the slot, t the last 16-byte boundary of the slot at or below q (last: q itself)
	__device__ void drain(bool last)
	{
		wave_lds_sync();
		const uint64_t t = last ? q : q - ((a0 + (uint32_t) q) & 15);
		if (t <= f)
			return;
		uint64_t sa = 0, sb = 0;
		uint64_t h = f + ((16 - ((a0 + (uint32_t) f) & 15)) & 15);
		h = h < t ? h : t;
		if (ln < h - f) { // the head: single bytes up to the boundary
			const uint64_t c = f + ln;
			const uint32_t v = ring[(a0 + (uint32_t) c) & IF_RM];
			dst[c] = (uint8_t) v;
			sa += v;
			sb += (t - c) * v;
		}
		const uint64_t body_end = h + ((t - h) & ~15ull);
		for (uint64_t c = h + 16 * ln; c < body_end; c += 1024) {
			const uint4 v = *reinterpret_cast<const uint4 *>(ring + ((a0 + (uint32_t) c) & IF_RM));
			*reinterpret_cast<uint4 *>(dst + c) = v;
			const uint32_t w[4] = { v.x, v.y, v.z, v.w };
			uint32_t p1 = 0, p2 = 0; // the sum of the 16 bytes, and of byte j times j
#pragma unroll
			for (uint32_t j = 0; j < 16; j++) {
				const uint32_t d = (w[j >> 2] >> (8 * (j & 3))) & 0xFF;
				p1 += d;
				p2 += j * d;
			}
			sa += p1;
			sb += (t - c) * p1 - p2;
		}
		if (ln < t - body_end) { // the tail of the last drain
			const uint64_t c = body_end + ln;
			const uint32_t v = ring[(a0 + (uint32_t) c) & IF_RM];
			dst[c] = (uint8_t) v;
			sa += v;
			sb += (t - c) * v;
		}
		sa = sum64(sa);
		sb = sum64(sb);
		s2 = uni((uint32_t) ((s2 + ((t - f) % ifw::ADLER_MOD) * s1 + sb) % ifw::ADLER_MOD));
		s1 = uni((uint32_t) ((s1 + sa) % ifw::ADLER_MOD));
		f = t;
	}
	__device__ void after()
	{
		if (WRITE && writing) {
			if (q > room)
				writing = false; // the count goes on; nothing more is written
			else if (q - f >= IF_DRAIN)
				drain(false);
		}
	}
	__device__ void literal(uint32_t v)
	{
		if (WRITE && writing && ln == 0)
			ring[(a0 + (uint32_t) q) & IF_RM] = (uint8_t) v;
		q++;
		after();
	}
	// Byte q + i is byte q - dist + i % dist: every source lies in front of q, where this match writes nothing.  A write
	// can only meet a source's place in the ring when dist + len > 32768, and then it is the place of a byte that the
	// same pass, or an earlier one, has read.
	__device__ void match(uint32_t len, uint32_t dist)
	{
		if (WRITE && writing) {
			wave_lds_sync();
			const uint32_t qq = a0 + (uint32_t) q;
			for (uint32_t i = ln; i < len; i += 64) {
				const uint32_t k = dist >= len ? i : dist == 1 ? 0 : i % dist;
				const uint8_t v = ring[(qq - dist + k) & IF_RM];
				ring[(qq + i) & IF_RM] = v;
			}
		}
		q += len;
		after();
	}
	__device__ void stored(uint64_t at, uint32_t n) // [at, at + n) lies inside the stream
	{
		if (!(WRITE && writing)) {
			q += n;
			return;
		}
		for (uint32_t c = 0; c < n; c += 1024) {
			const uint32_t m = n - c < 1024 ? n - c : 1024;
			if (writing) {
				const uint32_t qq = a0 + (uint32_t) q;
				for (uint32_t i = ln; i < m; i += 64)
					ring[(qq + i) & IF_RM] = b.p[at + c + i];
			}
			q += m;
			after();
		}
	}
};

template <bool WRITE>
__global__ __launch_bounds__(64) void k_if_walk(IfArgs a)
{
	__shared__ uint4 ring4[WRITE ? IF_RING / 16 : 1];
	__shared__ uint16_t tab[32 + 288 + (1 << ifw::LIT_BITS) + 32 + 32 + (1 << ifw::DIST_BITS) + 32 + 32 + (1 << ifw::CL_BITS)];
	__shared__ uint8_t lens[ifw::NLENS];
	const uint32_t r = blockIdx.x, ln = threadIdx.x;
	if (r >= a.nrec)
		return;
	const uint64_t co = uni64(a.comp_off[r]), cl = uni64(a.comp_len[r]);
	uint64_t base = 0, room = 0;
	if (WRITE) {
		const uint64_t o0 = uni64(a.out_off[r]), o1 = uni64(a.out_off[r + 1]);
		base = o0;
		room = o1 > o0 ? o1 - o0 : 0;
		if (a.need) { // the packed form: the first walk has judged the stream and left its length
			const uint64_t need = uni64(a.need[r]);
			if (need == IF_FAIL || need > room) {
				if (ln == 0) {
					a.out_len[r] = IF_FAIL;
					if (need != IF_FAIL)
						a.status[r] = ifw::ROOM; // it ends behind out_cap
				}
				return;
			}
			room = need;
		}
	}
	if ((cl >> 32) || co > a.comp_bytes || cl > a.comp_bytes - co) {
		if (ln == 0) {
			a.out_len[r] = IF_FAIL;
			a.status[r] = ifw::REFUSED;
		}
		return;
	}
	DevEnv<WRITE> e;
	e.b.p = a.comp + co;
	e.b.len = cl;
	e.lens = lens;
	uint16_t *t = tab;
	e.lit = { t, t + 32, t + 32 + 288, ifw::LIT_BITS };
	t += 32 + 288 + (1 << ifw::LIT_BITS);
	e.dist = { t, t + 32, t + 64, ifw::DIST_BITS };
	t += 64 + (1 << ifw::DIST_BITS);
	e.cl = { t, t + 32, t + 64, ifw::CL_BITS };
	e.ring = reinterpret_cast<uint8_t *>(ring4);
	e.dst = WRITE ? a.out + base : nullptr;
	e.room = room;
	e.q = e.f = 0;
	e.a0 = WRITE ? (uint32_t) ((uintptr_t) e.dst & 15) : 0;
	e.ln = ln;
	e.s1 = 1;
	e.s2 = 0;
	e.writing = WRITE;
	uint32_t adler = 0;
	uint8_t st = ifw::walk(e, &adler);
	uint64_t n = IF_FAIL;
	if (st == ifw::OK) {
		n = e.q;
		if (WRITE) {
			if (e.q > room) {
				st = ifw::ROOM; // the exact length; the Adler-32 is not judged
			} else {
				e.drain(true);
				if (adler != (e.s2 << 16 | e.s1)) {
					st = ifw::ADLER;
					n = IF_FAIL;
				}
			}
		}
	}
	if (ln == 0) {
		a.out_len[r] = n;
		a.status[r] = st;
	}
}

// ------------------------------------------------------------------ the fields of inflated records

struct FieldArgs {
	const uint8_t *rec;
	const uint64_t *rec_off, *rec_len;
	uint64_t rec_bytes;
	uint32_t nrec;
	int signal_method;
	uint64_t *sig_off, *sig_len;
	uint32_t *n_samples;
	double *dor;
	char *ids;
};

__device__ uint64_t get_le(const uint8_t *p, uint32_t n)
{
	uint64_t v = 0;
	for (uint32_t i = 0; i < n; i++)
		v |= (uint64_t) p[i] << (8 * i);
	return v;
}

// parse_record (blow5_reader.cpp): u16 id length | id | u32 read group | 4 doubles | u64 length | signal | ...
__global__ __launch_bounds__(256) void k_if_fields(FieldArgs a)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= a.nrec)
		return;
	const uint64_t ro = a.rec_off[r], rl = a.rec_len[r];
	bool ok = rl != IF_FAIL && ro <= a.rec_bytes && rl <= a.rec_bytes - ro && rl >= 2;
	const uint8_t *p = a.rec + ro;
	uint64_t idl = 0, at = 0, bytes = 0;
	uint32_t ns = 0;
	if (ok) {
		idl = get_le(p, 2);
		ok = rl >= 2 + idl + 4 + 32 + 8;
	}
	if (ok) {
		at = 2 + idl + 4 + 32;
		const uint64_t len = get_le(p + at, 8);
		at += 8;
		ok = a.signal_method ? len <= rl - at : len <= 0xFFFFFFFFull && len * 2 <= rl - at;
		bytes = a.signal_method ? len : len * 2;
		if (ok && a.signal_method) {
			ok = bytes >= 4;
			if (ok)
				ns = (uint32_t) get_le(p + at, 4);
		} else {
			ns = (uint32_t) len;
		}
	}
	a.sig_off[r] = ok ? ro + at : 0;
	a.sig_len[r] = ok ? bytes : IF_FAIL;
	a.n_samples[r] = ok ? ns : 0;
	if (a.dor)
		for (uint32_t k = 0; k < 3; k++)
			a.dor[3 * (size_t) r + k] = ok ? __longlong_as_double((long long) get_le(p + 2 + idl + 4 + 8 * k, 8)) : 0.0;
	if (a.ids) {
		char *dst = a.ids + (size_t) r * PRESS_HIP_BLOW5_ID_LEN;
		const uint32_t c = !ok ? 0 : idl < PRESS_HIP_BLOW5_ID_LEN - 1 ? (uint32_t) idl : PRESS_HIP_BLOW5_ID_LEN - 1;
		for (uint32_t i = 0; i < PRESS_HIP_BLOW5_ID_LEN; i++)
			dst[i] = i < c ? (char) p[2 + i] : 0;
	}
}

// ------------------------------------------------------------------ the host side

struct IfIn {
	const uint8_t *comp;
	const uint64_t *comp_off, *comp_len;
	uint64_t comp_bytes;
	uint32_t nrec;
};

void if_launch(bool write, const IfArgs &a, hipStream_t s)
{
	if (write)
		hipLaunchKernelGGL(k_if_walk<true>, dim3(a.nrec), dim3(64), 0, s, a);
	else
		hipLaunchKernelGGL(k_if_walk<false>, dim3(a.nrec), dim3(64), 0, s, a);
}

int if_args(const IfIn &in, const void *status)
{
	if (in.nrec && (!in.comp_off || !in.comp_len || (!in.comp && in.comp_bytes) || !status))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	return 0;
}

// the streams and their two tables on the device (host-pointer form): a.comp, a.comp_off, a.comp_len; `extra` more words
// of 8 bytes behind the tables -> *words
int if_stage(Staged &st, const IfIn &in, IfArgs &a, size_t extra, uint64_t **words)
{
	const size_t n8 = (size_t) in.nrec * 8;
	if (g.if_comp.reserve(in.comp_bytes + 16) || g.if_tabs.reserve(2 * n8 + extra * 8 + 8) || g.if_res.reserve(n8 + in.nrec + 16))
		return PRESS_HIP_EHIP;
	int rc;
	uint64_t *tabs = (uint64_t *) g.if_tabs.p;
	if ((rc = st.push(g.if_comp.p, in.comp, in.comp_bytes)) || (rc = st.push(tabs, in.comp_off, n8)) ||
	    (rc = st.push(tabs + in.nrec, in.comp_len, n8)))
		return rc;
	a.comp = (const uint8_t *) g.if_comp.p;
	a.comp_off = tabs;
	a.comp_len = tabs + in.nrec;
	a.out_len = (uint64_t *) g.if_res.p;
	a.status = (uint8_t *) g.if_res.p + n8;
	*words = tabs + 2 * (size_t) in.nrec;
	return 0;
}

IfArgs if_bind(const IfIn &in)
{
	IfArgs a = {};
	a.comp = in.comp;
	a.comp_off = in.comp_off;
	a.comp_len = in.comp_len;
	a.comp_bytes = in.comp_bytes;
	a.nrec = in.nrec;
	return a;
}

} // namespace

} // namespace ph

using namespace ph;

extern "C" int press_hip_blow5_inflate_sizes(const uint8_t *comp, const uint64_t *comp_off, const uint64_t *comp_len, uint64_t comp_bytes,
					     uint32_t nrec, uint64_t *need, uint8_t *status, int device_resident)
{
	API_LOCK;
	const IfIn in = { comp, comp_off, comp_len, comp_bytes, nrec };
	int rc = if_args(in, status);
	if (!rc && nrec && !need)
		rc = set_error(PRESS_HIP_EARG, "NULL argument");
	if (rc || (rc = ctx_init()) || nrec == 0)
		return rc;
	const hipStream_t s = g.stream();
	IfArgs a = if_bind(in);
	a.out_len = need;
	a.status = status;
	if (device_resident) {
		if_launch(false, a, s);
		return launch_status();
	}
	Staged st(nrec, s);
	uint64_t *words;
	if ((rc = if_stage(st, in, a, 0, &words)))
		return rc;
	if_launch(false, a, s);
	if ((rc = launch_status()))
		return rc;
	return st.fetch_tables({ { need, a.out_len, (size_t) nrec * 8 }, { status, a.status, nrec } });
}

extern "C" int press_hip_blow5_inflate_batch(const uint8_t *comp, const uint64_t *comp_off, const uint64_t *comp_len, uint64_t comp_bytes,
					     uint32_t nrec, uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint8_t *status,
					     int device_resident)
{
	API_LOCK;
	const IfIn in = { comp, comp_off, comp_len, comp_bytes, nrec };
	int rc = if_args(in, status);
	if (!rc && nrec && (!out || !out_off || !out_len))
		rc = set_error(PRESS_HIP_EARG, "NULL argument");
	if (!rc && nrec && !device_resident)
		rc = check_slots(out_off, nrec);
	if (rc || (rc = ctx_init()) || nrec == 0)
		return rc;
	const hipStream_t s = g.stream();
	IfArgs a = if_bind(in);
	if (device_resident) {
		a.out = out;
		a.out_off = out_off;
		a.out_len = out_len;
		a.status = status;
		if_launch(true, a, s);
		return launch_status();
	}
	// host pointers: the streams go up, the slots' span is an arena of the device, and what the records hold comes back
	Staged st(nrec, s);
	uint64_t *words;
	if ((rc = if_stage(st, in, a, (size_t) nrec + 1, &words)))
		return rc;
	const uint64_t a0 = out_off[0], span = out_off[nrec] - a0;
	std::vector<uint64_t> rel((size_t) nrec + 1);
	for (uint32_t r = 0; r <= nrec; r++)
		rel[r] = out_off[r] - a0;
	if (g.if_out.reserve(span + 64))
		return PRESS_HIP_EHIP;
	if ((rc = st.push(words, rel.data(), ((size_t) nrec + 1) * 8)))
		return rc;
	a.out = (uint8_t *) g.if_out.p;
	a.out_off = words;
	if_launch(true, a, s);
	if ((rc = launch_status()))
		return rc;
	std::vector<uint8_t> back(span);
	if (span)
		HIPCHK(hipMemcpyAsync(back.data(), g.if_out.p, span, hipMemcpyDeviceToHost, s));
	if ((rc = st.fetch_tables({ { out_len, a.out_len, (size_t) nrec * 8 }, { status, a.status, nrec } })))
		return rc;
	for (uint32_t r = 0; r < nrec; r++) // a failed record's slot stays as the caller left it
		if (status[r] == PRESS_HIP_INFLATE_OK && out_len[r])
			memcpy(out + out_off[r], back.data() + rel[r], out_len[r]);
	return 0;
}

extern "C" int press_hip_blow5_inflate_packed(const uint8_t *comp, const uint64_t *comp_off, const uint64_t *comp_len, uint64_t comp_bytes,
					      uint32_t nrec, uint8_t *out, uint64_t out_cap, uint32_t align, uint64_t *out_off,
					      uint64_t *out_len, uint8_t *status, int device_resident)
{
	API_LOCK;
	const IfIn in = { comp, comp_off, comp_len, comp_bytes, nrec };
	int rc = if_args(in, status);
	if (!rc && (!out_off || (nrec && (!out_len || (!out && out_cap)))))
		rc = set_error(PRESS_HIP_EARG, "NULL argument");
	if (!rc && (align == 0 || align > 4096 || (align & (align - 1))))
		rc = set_error(PRESS_HIP_EARG, "align = %u is not a power of two in 1 .. 4096", align);
	if (!rc && device_resident && nrec && ((uintptr_t) out & 3))
		rc = set_error(PRESS_HIP_EARG, "out must be a multiple of 4 bytes");
	if (rc || (rc = ctx_init()))
		return rc;
	const hipStream_t s = g.stream();
	if (nrec == 0) {
		if (device_resident)
			HIPCHK(hipMemsetAsync(out_off, 0, 8, s));
		else
			out_off[0] = 0;
		return 0;
	}
	const size_t n8 = (size_t) nrec * 8;
	if (g.if_need.reserve(n8) || g.if_slot.reserve(n8 + 8))
		return PRESS_HIP_EHIP;
	IfArgs a = if_bind(in);
	PackArgs pk = { (uint64_t *) g.if_need.p, out_off, (uint64_t *) g.if_slot.p, out_cap, align };
	Staged st(nrec, s);
	uint64_t *words = nullptr;
	if (device_resident) {
		a.status = status;
	} else {
		if ((rc = if_stage(st, in, a, (size_t) nrec + 1, &words)))
			return rc;
		pk.layout = words;
	}
	uint64_t *const lens = device_resident ? out_len : a.out_len;
	// the counting walk, the layout, the writing walk
	a.out_len = pk.need;
	if_launch(false, a, s);
	launch_pack_scan(pk, nrec, s);
	a.out_off = pk.slot;
	a.out_len = lens;
	a.need = pk.need;
	if (device_resident) {
		a.out = out;
		if_launch(true, a, s);
		return launch_status();
	}
	if ((rc = launch_status()) || (rc = st.fetch_tables({ { out_off, pk.layout, n8 + 8 } })))
		return rc;
	const uint64_t bytes = out_off[nrec] < out_cap ? out_off[nrec] : out_cap;
	if (g.if_out.reserve(bytes + 64))
		return PRESS_HIP_EHIP;
	if (bytes)
		HIPCHK(hipMemsetAsync(g.if_out.p, 0, bytes, s)); // (the padding between the records reaches the caller as zeros)
	a.out = (uint8_t *) g.if_out.p;
	if_launch(true, a, s);
	if ((rc = launch_status()) || (rc = st.fetch_prefix(out, g.if_out.p, bytes)))
		return rc;
	return st.fetch_tables({ { out_len, lens, n8 }, { status, a.status, nrec } });
}

extern "C" int press_hip_blow5_record_fields(const uint8_t *rec, const uint64_t *rec_off, const uint64_t *rec_len, uint64_t rec_bytes,
					     uint32_t nrec, int signal_method, uint64_t *sig_off, uint64_t *sig_len, uint32_t *n_samples,
					     double *dor, char *read_ids, int device_resident)
{
	API_LOCK;
	if (signal_method < 0 || signal_method > 1)
		return set_error(PRESS_HIP_EARG, "signal_method = %d: 0 (int16 samples) or 1 (svb-zd)", signal_method);
	if (nrec && (!rec_off || !rec_len || (!rec && rec_bytes) || !sig_off || !sig_len || !n_samples))
		return set_error(PRESS_HIP_EARG, "NULL argument");
	int rc = ctx_init();
	if (rc || nrec == 0)
		return rc;
	const hipStream_t s = g.stream();
	FieldArgs a = { rec, rec_off, rec_len, rec_bytes, nrec, signal_method, sig_off, sig_len, n_samples, dor, read_ids };
	const dim3 grid((nrec + 255) / 256);
	if (device_resident) {
		hipLaunchKernelGGL(k_if_fields, grid, dim3(256), 0, s, a);
		return launch_status();
	}
	Staged st(nrec, s);
	const size_t n8 = (size_t) nrec * 8;
	// results in one buffer: sig_off, sig_len, dor (8-byte words), then n_samples, then the ids
	const size_t res = 2 * n8 + 3 * n8 + (size_t) nrec * 4 + (size_t) nrec * PRESS_HIP_BLOW5_ID_LEN;
	if (g.if_comp.reserve(rec_bytes + 16) || g.if_tabs.reserve(2 * n8) || g.if_res.reserve(res))
		return PRESS_HIP_EHIP;
	uint64_t *tabs = (uint64_t *) g.if_tabs.p;
	if ((rc = st.push(g.if_comp.p, rec, rec_bytes)) || (rc = st.push(tabs, rec_off, n8)) || (rc = st.push(tabs + nrec, rec_len, n8)))
		return rc;
	uint64_t *w = (uint64_t *) g.if_res.p;
	a.rec = (const uint8_t *) g.if_comp.p;
	a.rec_off = tabs;
	a.rec_len = tabs + nrec;
	a.sig_off = w;
	a.sig_len = w + nrec;
	a.dor = (double *) (w + 2 * (size_t) nrec);
	a.n_samples = (uint32_t *) (w + 5 * (size_t) nrec);
	a.ids = (char *) (a.n_samples + nrec);
	hipLaunchKernelGGL(k_if_fields, grid, dim3(256), 0, s, a);
	if ((rc = launch_status()))
		return rc;
	return st.fetch_tables({ { sig_off, a.sig_off, n8 }, { sig_len, a.sig_len, n8 }, { dor, a.dor, 3 * n8 },
				 { n_samples, a.n_samples, (size_t) nrec * 4 }, { read_ids, a.ids, (size_t) nrec * PRESS_HIP_BLOW5_ID_LEN } });
}

extern "C" uint64_t press_hip_blow5_inflate_workspace_bytes(uint64_t comp_bytes, uint32_t nrec)
{
	(void) comp_bytes; // the walks keep their state in LDS: the packed form's two tables are all the scratch there is
	return 2 * ((uint64_t) nrec + 1) * 8;
}
