// press_dropin.hip - the reference's per-read symbols (press/press.h), each one read through the batch path.

#include <stdlib.h>

#include <vector>

#include "press_host.h"
#include "press_rice_walk.h"
#include "press_dhuf_walk.h"

using namespace ph;

// ------------------------------------------------------------------ drop-in per-read symbols

namespace {

// one read through the batch path; returns 0 and the length, or an error code
int press_one(int method, const int16_t *in, uint32_t n, uint8_t *out, uint64_t cap, uint64_t *len)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ooff[2] = { 0, cap };
	uint64_t l = PRESS_HIP_FAILED;
	if (n == 0)
		return set_error(PRESS_HIP_EARG, "empty read");
	int rc = press_hip_press_batch(method, in, off, &n, 1, n, out, ooff, &l, 0);
	if (rc)
		return rc;
	if (l == PRESS_HIP_FAILED)
		return set_error(-1, "stream does not fit %llu bytes", (unsigned long long) cap);
	*len = l;
	return 0;
}

int depress_one(int method, const uint8_t *in, uint64_t nbytes, int16_t *out, uint32_t cap, uint32_t *n)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ioff[1] = { 0 };
	const uint64_t ilen[1] = { nbytes };
	uint32_t got = UINT32_MAX;
	if (cap == 0)
		return set_error(PRESS_HIP_EARG, "no room for samples");
	int rc = press_hip_depress_batch(method, in, ioff, ilen, 1, out, off, &cap, cap, &got, 0);
	if (rc)
		return rc;
	if (got == UINT32_MAX)
		return set_error(-1, "malformed stream");
	*n = got;
	return 0;
}

// exact length of an svb16 / svb32 stream of n values (its callers do not pass it)
uint64_t svb_stream_len(const uint8_t *in, uint32_t n, bool key2)
{
	uint64_t len;
	if (!key2) {
		const uint32_t klen = svb16_keylen(n);
		len = (uint64_t) klen + n;
		for (uint32_t i = 0; i < n / 8; i++)
			len += (uint64_t) __builtin_popcount(in[i]);
		if (n & 7)
			len += (uint64_t) __builtin_popcount(in[n / 8] & ((1u << (n & 7)) - 1));
	} else {
		len = (uint64_t) (n + 3) / 4 + n;
		for (uint32_t i = 0; i < n; i++)
			len += (in[i >> 2] >> (2 * (i & 3))) & 3u;
	}
	return len;
}

void void_press(int method, const int16_t *in, uint64_t n, uint8_t *out, uint64_t *nout)
{
	uint64_t len = 0;
	if (press_one(method, in, (uint32_t) n, out, *nout, &len)) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		len = 0;
	}
	*nout = len;
}

int int_press_inner(int method, const int16_t *in, uint32_t n, uint8_t *out, uint64_t *nout)
{
	uint64_t len = 0;
	int rc = press_one(method, in, n, out, *nout, &len);
	if (rc)
		return -1;
	*nout = len;
	return 0;
}

void void_depress(int method, const uint8_t *in, uint64_t nbytes, int16_t *out, uint32_t *nout)
{
	uint32_t n = 0;
	if (depress_one(method, in, nbytes, out, *nout, &n)) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		n = 0;
	}
	*nout = n;
}

void stall_press_(int sm, const int16_t *in, uint32_t n, uint8_t *out, uint64_t *nout)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ooff[2] = { 0, *nout };
	uint64_t l = PRESS_HIP_FAILED;
	int rc = n ? press_hip_stall_press_batch(sm, in, off, &n, 1, n, out, ooff, &l, nullptr, 0) : set_error(PRESS_HIP_EARG, "empty read");
	if (!rc && l == PRESS_HIP_FAILED)
		rc = set_error(-1, "the read is refused, or its stream does not fit %llu bytes", (unsigned long long) *nout);
	if (rc) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		l = 0;
	}
	*nout = l;
}

void stall_depress_(const uint8_t *in, uint64_t nsamples, int16_t *out, uint32_t *nout)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ioff[1] = { 0 };
	uint32_t n = (uint32_t) nsamples, got = UINT32_MAX;
	// [exists] ([start u16][len u16][nstall u16][stall piece]) [nrest u32][rest piece]
	uint64_t len = 5;
	int rc = 0;
	if (n == 0 || nsamples > UINT32_MAX || in[0] > 1) {
		rc = set_error(-1, "malformed stream");
	} else {
		uint64_t pos = 1;
		if (in[0]) {
			uint16_t l1;
			memcpy(&l1, in + 5, 2);
			pos = 7 + (uint64_t) l1;
		}
		uint32_t l0;
		memcpy(&l0, in + pos, 4);
		len = pos + 4 + l0;
		const uint64_t ilen[1] = { len };
		rc = press_hip_stall_depress_batch(in, ioff, ilen, 1, out, off, &n, n, &got, 0);
		if (!rc && got == UINT32_MAX)
			rc = set_error(-1, "malformed stream");
	}
	if (rc) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		got = 0;
	}
	*nout = got;
}

// the range-coder family: one read through press_hip_rcf_press_batch / press_hip_rcf_depress_batch
void rcf_press_(int coder, int layout, const int16_t *in, uint32_t n, uint8_t *out, uint64_t *nout)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ooff[2] = { 0, *nout };
	uint64_t l = PRESS_HIP_FAILED;
	int rc = n ? press_hip_rcf_press_batch(coder, layout, in, off, &n, 1, n, out, ooff, &l, nullptr, 0) : set_error(PRESS_HIP_EARG, "empty read");
	if (!rc && l == PRESS_HIP_FAILED)
		rc = set_error(-1, "stream does not fit %llu bytes", (unsigned long long) *nout);
	if (rc) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		l = 0;
	}
	*nout = l;
}

void rcf_depress_(int coder, int layout, const uint8_t *in, uint64_t nbytes, int16_t *out, uint32_t *nout)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ioff[1] = { 0 };
	const uint64_t ilen[1] = { nbytes };
	uint32_t cap = *nout, got = UINT32_MAX;
	int rc = cap ? press_hip_rcf_depress_batch(coder, layout, in, ioff, ilen, 1, out, off, &cap, cap, &got, 0)
		     : set_error(PRESS_HIP_EARG, "no room for samples");
	if (!rc && got == UINT32_MAX)
		rc = set_error(-1, "malformed stream");
	if (rc) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		got = 0;
	}
	*nout = got;
}

// the Rice family: one read through press_hip_rice_press_batch / press_hip_rice_depress_batch
void rice_press_(int layout, const int16_t *in, uint32_t n, uint8_t *out, uint64_t *nout)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ooff[2] = { 0, *nout };
	uint64_t l = PRESS_HIP_FAILED;
	int rc = n ? press_hip_rice_press_batch(layout, in, off, &n, 1, n, out, ooff, &l, nullptr, 0) : set_error(PRESS_HIP_EARG, "empty read");
	if (!rc && l == PRESS_HIP_FAILED)
		rc = set_error(-1, "stream does not fit %llu bytes", (unsigned long long) *nout);
	if (rc) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		l = 0;
	}
	*nout = l;
}

// nsamples: the read's SAMPLE count, as the reference's symbols take it (press.c:5050); the stream's length is found by
// reading it (press_rice_walk.h)
void rice_depress_(int layout, const uint8_t *in, uint64_t nsamples, int16_t *out, uint32_t *nout)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ioff[1] = { 0 };
	uint64_t ilen[1] = { 0 };
	uint32_t n = (uint32_t) nsamples, got = UINT32_MAX;
	int rc;
	if (n == 0 || nsamples > *nout)
		rc = set_error(PRESS_HIP_EARG, "no room for samples");
	else if (!rice_stream_len(layout, in, n, ilen))
		rc = set_error(-1, "malformed stream");
	else
		rc = press_hip_rice_depress_batch(layout, in, ioff, ilen, 1, out, off, &n, n, &got, 0);
	if (!rc && got == UINT32_MAX)
		rc = set_error(-1, "malformed stream");
	if (rc) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		got = 0;
	}
	*nout = got;
}

// the per-read Huffman family: one read through press_hip_huffman_press_batch / press_hip_huffman_depress_batch
int dhuf_press_(int layout, const int16_t *in, uint32_t n, uint8_t *out, uint64_t *nout)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ooff[2] = { 0, *nout };
	uint64_t l = PRESS_HIP_FAILED;
	int rc = n ? press_hip_huffman_press_batch(layout, in, off, &n, 1, n, out, ooff, &l, nullptr, 0) : set_error(PRESS_HIP_EARG, "empty read");
	if (!rc && l == PRESS_HIP_FAILED)
		rc = set_error(-1, "stream does not fit %llu bytes", (unsigned long long) *nout);
	if (rc) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		*nout = 0;
		return -1;
	}
	*nout = l;
	return 0;
}

// nbytes: the stream's length, *nout the capacity in samples (press.c:4011); the sample count the batch call wants is
// read from the stream (press_dhuf_walk.h), and a stream that says more than the capacity is refused
int dhuf_depress_(int layout, const uint8_t *in, uint64_t nbytes, int16_t *out, uint32_t *nout)
{
	const uint64_t off[1] = { 0 };
	const uint64_t ioff[1] = { 0 };
	const uint64_t ilen[1] = { nbytes };
	uint64_t ns = 0;
	uint32_t n = 0, got = UINT32_MAX;
	int rc;
	if (!dhuf_stream_samples(layout, in, nbytes, &ns))
		rc = set_error(-1, "malformed stream");
	else if (ns > *nout)
		rc = set_error(PRESS_HIP_EARG, "no room for samples");
	else {
		n = (uint32_t) ns;
		rc = press_hip_huffman_depress_batch(layout, in, ioff, ilen, 1, out, off, &n, n, &got, 0);
	}
	if (!rc && got == UINT32_MAX)
		rc = set_error(-1, "malformed stream");
	if (rc) {
		fprintf(stderr, "press_hip: %s\n", press_hip_last_error());
		*nout = 0;
		return -1;
	}
	*nout = got;
	return 0;
}

// zstd level 1 (press.h:275) around a GPU-made inner stream (press.c:1865, 2025, 8554)
int zstd_press_(int inner, bool prefix_n, const int16_t *in, uint32_t n, uint8_t *out, uint64_t *nout)
{
	if (!zstd_open())
		return set_error(-1, "libzstd not found"), -1;
	const uint64_t cap = (prefix_n ? 4 : 0) + press_hip_bound(inner, n);
	std::vector<uint8_t> buf(cap + 64);
	uint64_t len = 0;
	if (prefix_n)
		memcpy(buf.data(), &n, 4);
	if (press_one(inner, in, n, buf.data() + (prefix_n ? 4 : 0), cap - (prefix_n ? 4 : 0), &len))
		return -1;
	len += prefix_n ? 4 : 0;
	const size_t r = zstd_fn.compress(out, *nout, buf.data(), len, 1);
	if (zstd_fn.is_error(r))
		return -1;
	*nout = r;
	return 0;
}

int zstd_depress_(int inner, bool prefix_n, const uint8_t *in, uint64_t nbytes, int16_t *out, uint32_t *nout)
{
	if (!zstd_open())
		return set_error(-1, "libzstd not found"), -1;
	const uint64_t cap = zstd_bound_((uint64_t) *nout * 2); // press.c:1897
	std::vector<uint8_t> buf(cap + 64);
	const size_t r = zstd_fn.decompress(buf.data(), cap, in, nbytes);
	if (zstd_fn.is_error(r))
		return -1;
	uint32_t n = 0;
	if (prefix_n) {
		uint32_t cnt;
		if (r < 4)
			return -1;
		memcpy(&cnt, buf.data(), 4);
		if (cnt > *nout)
			return -1;
		if (cnt && depress_one(inner, buf.data() + 4, r - 4, out, cnt, &n))
			return -1;
	} else if (depress_one(inner, buf.data(), r, out, *nout, &n)) {
		return -1;
	}
	*nout = n;
	return 0;
}

} // namespace

extern "C" {

uint64_t svb12_bound(uint64_t nin) { return bound_svb16((uint32_t) nin); }
void svb12_press(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)
{
	void_press(PRESS_HIP_SVB12, in, nin, out, nout);
}
void svb12_depress(const uint8_t *in, uint64_t nin, int16_t *out)
{
	uint32_t n = (uint32_t) nin;
	void_depress(PRESS_HIP_SVB12, in, svb_stream_len(in, (uint32_t) nin, false), out, &n);
}

uint64_t svb12_zd_bound(uint64_t nin) { return bound_svb16((uint32_t) nin); }
void svb12_zd_press(const int16_t *in, uint64_t nin, uint8_t *out, uint64_t *nout)
{
	void_press(PRESS_HIP_SVB12_ZD, in, nin, out, nout);
}
void svb12_zd_depress(const uint8_t *in, uint64_t nin, int16_t *out, uint64_t *nout)
{
	uint32_t n = (uint32_t) nin;
	void_depress(PRESS_HIP_SVB12_ZD, in, svb_stream_len(in, (uint32_t) nin, false), out, &n);
	*nout = n;
}

uint64_t svb_zd_bound_16(uint64_t nin) { return bound_svb32((uint32_t) nin); }
void svb_zd_press_16(const int16_t *in, uint64_t nin, uint8_t *out, uint64_t *nout)
{
	void_press(PRESS_HIP_SVB_ZD, in, nin, out, nout);
}
void svb_zd_depress_16(const uint8_t *in, uint64_t nin, int16_t *out, uint64_t *nout)
{
	uint32_t n = (uint32_t) nin;
	void_depress(PRESS_HIP_SVB_ZD, in, svb_stream_len(in, (uint32_t) nin, true), out, &n);
	*nout = n;
}

uint64_t zstd_svb_zd_bound_16(uint32_t nin) { return press_hip_bound(PRESS_HIP_ZSTD_SVB_ZD, nin); }
int zstd_svb_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)
{
	return zstd_press_(PRESS_HIP_SVB_ZD, true, in, nin, out, nout);
}
int zstd_svb_zd_depress_16(const uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)
{
	return zstd_depress_(PRESS_HIP_SVB_ZD, true, in, nin, out, nout);
}

uint64_t zstd_svb12_zd_bound(uint32_t nin) { return press_hip_bound(PRESS_HIP_ZSTD_SVB12_ZD, nin); }
int zstd_svb12_zd_press(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)
{
	return zstd_press_(PRESS_HIP_SVB12_ZD, true, in, nin, out, nout);
}
int zstd_svb12_zd_depress(const uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)
{
	return zstd_depress_(PRESS_HIP_SVB12_ZD, true, in, nin, out, nout);
}

#define VB_FAMILY(name, id)                                                                      \
	uint64_t name##_zd_bound_16(uint32_t nin) { return bound_vbzd(nin); }                    \
	void name##_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)   \
	{                                                                                        \
		void_press(id, in, nin, out, nout);                                              \
	}                                                                                        \
	void name##_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)       \
	{                                                                                        \
		void_depress(id, in, nin, out, nout);                                            \
	}
VB_FAMILY(vbe21, PRESS_HIP_VBE21_ZD)
VB_FAMILY(vbbe21, PRESS_HIP_VBBE21_ZD)
VB_FAMILY(vbsbe21, PRESS_HIP_VBSBE21_ZD)
VB_FAMILY(vbsse21, PRESS_HIP_VBSSE21_ZD)

// the range coders, same shape (their bound is press.c:3411 too); *nout of depress must be the exact sample count (press.c:5464)
VB_FAMILY(rc_vbe21, PRESS_HIP_RC_VBE21_ZD)     // press.h:712-716
VB_FAMILY(rcc_vbe21, PRESS_HIP_RCC_VBE21_ZD)   // press.c:5510-5580: the order-1 coder
VB_FAMILY(rccm_vbbe21, PRESS_HIP_RCCM_VBBE21_ZD) // press.c:6901-7000: vbbe21 + the order 1-0 context-mixing coder

#define SHUFF_FAMILY(name, id)                                                                           \
	uint64_t shuffman_##name##_zd_bound_16(uint32_t nin) { return bound_vbzd(nin); }                 \
	int shuffman_##name##_zd_press_16(SymbolEncoder *se, const int16_t *in, uint32_t nin,            \
					  uint8_t *out, uint64_t *nout)                                  \
	{                                                                                                \
		if (table_from_encoder(se))                                                              \
			return 1;                                                                        \
		return int_press_inner(id, in, nin, out, nout);                                          \
	}                                                                                                \
	int shuffman_##name##_zd_depress_16(huffman_node *root, uint8_t *in, uint64_t nin, int16_t *out, \
					    uint32_t *nout)                                              \
	{                                                                                                \
		if (table_from_tree(root))                                                               \
			return 1;                                                                        \
		uint32_t n = 0;                                                                          \
		if (depress_one(id, in, nin, out, *nout, &n))                                            \
			return 1;                                                                        \
		*nout = n;                                                                               \
		return 0;                                                                                \
	}
SHUFF_FAMILY(vbe21, PRESS_HIP_SHUFF_VBE21_ZD)
SHUFF_FAMILY(vbbe21, PRESS_HIP_SHUFF_VBBE21_ZD)
SHUFF_FAMILY(vbsbe21, PRESS_HIP_SHUFF_VBSBE21_ZD)
SHUFF_FAMILY(vbsse21, PRESS_HIP_SHUFF_VBSSE21_ZD)

uint64_t hasgam_vbsse21_zdq_bound_16(uint32_t nin) { return press_hip_bound(PRESS_HIP_HASGAM_ZDQ, nin); }
int hasgam_vbsse21_zdq_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)
{
	return int_press_inner(PRESS_HIP_HASGAM_ZDQ, in, nin, out, nout);
}
int hasgam_vbsse21_zdq_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)
{
	uint32_t n = 0;
	if (depress_one(PRESS_HIP_HASGAM_ZDQ, in, nin, out, *nout, &n))
		return -1;
	*nout = n;
	return 0;
}

uint64_t zstd_hasgam_vbsse21_zdq_bound_16(uint32_t nin) { return press_hip_bound(PRESS_HIP_ZSTD_HASGAM_ZDQ, nin); }
int zstd_hasgam_vbsse21_zdq_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)
{
	return zstd_press_(PRESS_HIP_HASGAM_ZDQ, false, in, nin, out, nout);
}
int zstd_hasgam_vbsse21_zdq_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)
{
	return zstd_depress_(PRESS_HIP_HASGAM_ZDQ, false, in, nin, out, nout);
}

// ---- BLOW5's signal codec "svb-zd" (slow5lib slow5_press.c:1054,1110), SURVEY 8f-2
uint64_t slow5_svb_zd_bound(uint32_t nin) { return press_hip_bound(PRESS_HIP_SLOW5_SVB_ZD, nin); }
int slow5_svb_zd_press(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)
{
	if (nin == 0) { // an empty signal is just its count
		if (*nout < 4)
			return -1;
		memset(out, 0, 4);
		*nout = 4;
		return 0;
	}
	return int_press_inner(PRESS_HIP_SLOW5_SVB_ZD, in, nin, out, nout);
}
int slow5_svb_zd_depress(const uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)
{
	uint32_t cnt, n = 0;
	if (nin < 4)
		return -1;
	memcpy(&cnt, in, 4); // slow5_press.c:1086: the count travels in the stream
	if (cnt > *nout)
		return -1;
	if (cnt == 0) {
		*nout = 0;
		return nin == 4 ? 0 : -1;
	}
	if (depress_one(PRESS_HIP_SLOW5_SVB_ZD, in, nin, out, cnt, &n))
		return -1;
	*nout = n;
	return 0;
}
// the shape slow5lib itself uses (slow5_ptr_compress_solo / slow5_ptr_depress_solo with
// SLOW5_COMPRESS_SVB_ZD, slow5_press.h:103-105): malloc'd result, byte counts in and out
void *press_hip_slow5_ptr_compress_svb_zd(const int16_t *ptr, size_t count, size_t *n)
{
	const uint32_t ns = (uint32_t) (count / sizeof *ptr);
	uint64_t len = slow5_svb_zd_bound(ns);
	uint8_t *out = (uint8_t *) malloc(len + 16);
	if (!out || slow5_svb_zd_press(ptr, ns, out, &len)) {
		free(out);
		return nullptr;
	}
	*n = (size_t) len;
	return out;
}
void *press_hip_slow5_ptr_depress_svb_zd(const uint8_t *ptr, size_t count, size_t *n)
{
	uint32_t cnt;
	if (count < 4)
		return nullptr;
	memcpy(&cnt, ptr, 4);
	int16_t *out = (int16_t *) malloc(((size_t) cnt + 8) * sizeof *out);
	uint32_t got = cnt;
	if (!out || slow5_svb_zd_depress(ptr, count, out, &got)) {
		free(out);
		return nullptr;
	}
	*n = (size_t) got * sizeof *out;
	return out;
}

// ---- the stall methods (press.c:7716-8030).  Their depress takes the SAMPLE count in nin (press.c:7871) and no byte
// count: the stream's length is what its own header says, as the reference reads it
#define STALL_FAMILY(name, id)                                                                   \
	uint64_t name##_bound_16(uint32_t nin) { return press_hip_stall_bound(id, nin); }        \
	void name##_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)      \
	{                                                                                        \
		stall_press_(id, in, nin, out, nout);                                            \
	}                                                                                        \
	void name##_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)          \
	{                                                                                        \
		stall_depress_(in, nin, out, nout);                                              \
	}
STALL_FAMILY(rccm_svbbe21_zd, PRESS_HIP_STALL_RCCM_SVBBE21_ZD)
STALL_FAMILY(dstall_fz_1500, PRESS_HIP_STALL_DSTALL_FZ_1500)
STALL_FAMILY(dstall_fz, PRESS_HIP_STALL_DSTALL_FZ)

// ---- the thirteen pairs of the range-coder family that are not public methods (press.h:752-899), VB_FAMILY's shape
#define RCF_FAMILY(name, coder, layout)                                                          \
	uint64_t name##_zd_bound_16(uint32_t nin) { return press_hip_rcf_bound(coder, layout, nin); } \
	void name##_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)   \
	{                                                                                        \
		rcf_press_(coder, layout, in, nin, out, nout);                                   \
	}                                                                                        \
	void name##_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)       \
	{                                                                                        \
		rcf_depress_(coder, layout, in, nin, out, nout);                                 \
	}
RCF_FAMILY(rc_vbbe21, PRESS_HIP_RCF_RC, PRESS_HIP_RCF_VBBE21)
RCF_FAMILY(rc_vbsbe21, PRESS_HIP_RCF_RC, PRESS_HIP_RCF_VBSBE21)
RCF_FAMILY(rc_vbsse21, PRESS_HIP_RCF_RC, PRESS_HIP_RCF_VBSSE21)
RCF_FAMILY(rcc_vbbe21, PRESS_HIP_RCF_RCC, PRESS_HIP_RCF_VBBE21)
RCF_FAMILY(rcc_vbsbe21, PRESS_HIP_RCF_RCC, PRESS_HIP_RCF_VBSBE21)
RCF_FAMILY(rcc_vbsse21, PRESS_HIP_RCF_RCC, PRESS_HIP_RCF_VBSSE21)
RCF_FAMILY(rccm_vbe21, PRESS_HIP_RCF_RCCM, PRESS_HIP_RCF_VBE21)
RCF_FAMILY(rccm_vbsbe21, PRESS_HIP_RCF_RCCM, PRESS_HIP_RCF_VBSBE21)
RCF_FAMILY(rccm_vbsse21, PRESS_HIP_RCF_RCCM, PRESS_HIP_RCF_VBSSE21)
RCF_FAMILY(rccdf_vbe21, PRESS_HIP_RCF_RCCDF, PRESS_HIP_RCF_VBE21)
RCF_FAMILY(rccdf_vbbe21, PRESS_HIP_RCF_RCCDF, PRESS_HIP_RCF_VBBE21)
RCF_FAMILY(rccdf_vbsbe21, PRESS_HIP_RCF_RCCDF, PRESS_HIP_RCF_VBSBE21)
RCF_FAMILY(rccdf_vbsse21, PRESS_HIP_RCF_RCCDF, PRESS_HIP_RCF_VBSSE21)

// ---- the four methods of the Rice family (press.h:673-701); depress: nin is the sample count
#define RICE_FAMILY(name, layout)                                                                \
	uint64_t name##_zd_bound_16(uint32_t nin) { return press_hip_rice_bound(layout, nin); }  \
	void name##_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)   \
	{                                                                                        \
		rice_press_(layout, in, nin, out, nout);                                         \
	}                                                                                        \
	void name##_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)       \
	{                                                                                        \
		rice_depress_(layout, in, nin, out, nout);                                       \
	}
RICE_FAMILY(rice_vbe21, PRESS_HIP_RCF_VBE21)
RICE_FAMILY(rice_vbbe21, PRESS_HIP_RCF_VBBE21)
RICE_FAMILY(rice_vbsbe21, PRESS_HIP_RCF_VBSBE21)
RICE_FAMILY(rice_vbsse21, PRESS_HIP_RCF_VBSSE21)

// ---- the four methods of the per-read Huffman family (press.h:602-631): int results, depress: nin is the stream's length
#define DHUF_FAMILY(name, layout)                                                                  \
	uint64_t name##_zd_bound_16(uint32_t nin) { return press_hip_huffman_bound(layout, nin); } \
	int name##_zd_press_16(const int16_t *in, uint32_t nin, uint8_t *out, uint64_t *nout)      \
	{                                                                                          \
		return dhuf_press_(layout, in, nin, out, nout);                                    \
	}                                                                                          \
	int name##_zd_depress_16(uint8_t *in, uint64_t nin, int16_t *out, uint32_t *nout)          \
	{                                                                                          \
		return dhuf_depress_(layout, in, nin, out, nout);                                  \
	}
DHUF_FAMILY(huffman_vbe21, PRESS_HIP_RCF_VBE21)
DHUF_FAMILY(huffman_vbbe21, PRESS_HIP_RCF_VBBE21)
DHUF_FAMILY(huffman_vbsbe21, PRESS_HIP_RCF_VBSBE21)
DHUF_FAMILY(huffman_vbsse21, PRESS_HIP_RCF_VBSSE21)

} // extern "C"
