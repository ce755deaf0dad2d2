// press_train.hip - fitting a static-Huffman table to the user's reads.
//
//   device  k_train_prep + k_symbol_count: the histogram of what the four shuffman_* methods Huffman-code,
//           over a batch laid out as for press_hip_press_batch.  For read r and i in [1, n[r]):
//           zd[i] = zig-zag of the 16-bit wrapped delta s[i] - s[i-1] (trans.c:215, zigdelta_16_u16); values up to
//           255 are counted in counts[zd], the rest (the exceptions vbe21 stores aside, press.c:2679) in counts[256].
//           Sample 0 is stored raw and is not counted.
//   host    press_hip_table_from_counts: calculate_huffman_codes (huffman.c:373) as gen_huffman runs it
//           (get_freq :1074, print_table_freq :1168), with a length limit; press_hip_write_table_file:
//           write_code_table (huffman.c:440).

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/press_hip.h"
#include "press_internal.h"
#include "press_wave.h"

namespace ph {

constexpr int TWG = 256;                        // threads per workgroup
constexpr int TCK = 16;                         // 16-byte loads per lane and chunk (4 waves x 16 x 512 samples = CHUNK)
constexpr uint32_t TSUB = 512;                  // samples per wave and load (64 lanes x 8)
constexpr uint32_t TWAVE = TCK * TSUB;          // samples per wave and chunk
static_assert(TWAVE * 4 == CHUNK, "chunk = 4 waves");
constexpr int TCOPIES = 16;                     // counter copies in LDS: 4 per wave, by lane & 3
constexpr int TBINS = 257;                      // the 256 one-byte values, then the exceptions

struct TrainChunk { // one per chunk of CHUNK samples, written by k_train_prep (16 bytes)
	uint64_t sig_off; // sample offset of the read in sig
	uint32_t n;       // samples in the read
	uint32_t j;       // chunk index within the read
};
static_assert(sizeof(TrainChunk) == 16, "TrainChunk");

// The work list, built on the device (off / n may be device-resident): one thread per read, a wave takes a
// contiguous range of chunk ids with ONE atomic.  Reads of fewer than 2 samples have no delta and no chunk.
__global__ __launch_bounds__(256) void k_train_prep(const uint64_t *off, const uint32_t *nsamp, uint32_t nreads,
						    TrainChunk *chunks, uint32_t *nchunks, uint32_t max_chunks)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	uint32_t n = 0, nch = 0;
	if (r < nreads) {
		n = nsamp[r];
		nch = n >= 2 ? (n + CHUNK - 1) / CHUNK : 0;
	}
	uint32_t inc = nch; // inclusive wave scan
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = __shfl_up(inc, d, 64);
		if (lane >= d)
			inc += t;
	}
	uint32_t base = 0;
	if (lane == 63 && inc)
		base = atomicAdd(nchunks, inc);
	base = (uint32_t) __builtin_amdgcn_readlane((int) base, 63);
	if (r >= nreads)
		return;
	const uint32_t first = base + inc - nch;
	const uint64_t o = off[r];
	for (uint32_t j = 0; j < nch && first + j < max_chunks; j++) {
		TrainChunk c;
		c.sig_off = o;
		c.n = n;
		c.j = j;
		chunks[first + j] = c;
	}
}

// A persistent grid walks the chunks.  A chunk is 4 waves x 16 loads of 16 bytes per lane (the layout of
// k_svb_encode_chunked); the sample in front of a wave's quarter is one plain load.  Every value is counted
// with one LDS add into one of 16 copies of the counters (4 per wave, by lane): nanopore deltas are peaked,
// and lanes that hit one counter in one ds_add are served one after another.  The copies are summed once
// per workgroup and added to counts[] with one 64-bit atomic per bin: integer sums, the same whatever order
// the workgroups finish in.  (A copy counts 1/16 of its workgroup's samples: 32-bit counters overflow only
// beyond 2^36 samples per workgroup.)
__global__ __launch_bounds__(TWG) void k_symbol_count(const int16_t *sig, const TrainChunk *chunks,
						      const uint32_t *nchunks, uint32_t max_chunks,
						      unsigned long long *counts)
{
	__shared__ uint32_t s_h[TCOPIES][TBINS];
	for (int i = threadIdx.x; i < TCOPIES * TBINS; i += TWG)
		(&s_h[0][0])[i] = 0;
	__syncthreads();
	uint32_t *my = s_h[4 * (threadIdx.x >> 6) + (threadIdx.x & 3)];
	const int lane = threadIdx.x & 63;
	const uint32_t w = uni(threadIdx.x >> 6);
	const uint32_t nch = min(uni(*nchunks), max_chunks);

	for (uint32_t t = blockIdx.x; t < nch; t += gridDim.x) {
		const TrainChunk *cp = chunks + t;
		const uint64_t so = uni64(cp->sig_off);
		const uint32_t n = uni(cp->n);
		const uint32_t ws = uni(cp->j) * CHUNK + w * TWAVE; // first sample of this wave's quarter
		if (ws >= n)
			continue; // (no barrier in the loop: a wave may leave a chunk on its own)
		const int16_t *in = sig + so;
		uint4 z[TCK];
#pragma unroll
		for (int k = 0; k < TCK; k++) {
			const uint32_t i0 = ws + k * TSUB + lane * 8;
			z[k] = make_uint4(0, 0, 0, 0);
			if (i0 < n)
				z[k] = ld16_stream(in + i0);
		}
		uint32_t carry = ws > 0 ? (uint32_t) (uint16_t) in[ws - 1] << 16 : 0u;
#pragma unroll
		for (int k = 0; k < TCK; k++) {
			const uint32_t i0 = ws + k * TSUB + lane * 8;
			const uint32_t pw = prev_lane(z[k].w, carry);
			carry = (uint32_t) __builtin_amdgcn_readlane((int) z[k].w, 63);
			const uint32_t zz[4] = { zd_pair(z[k].x, pw), zd_pair(z[k].y, z[k].x), zd_pair(z[k].z, z[k].y),
						 zd_pair(z[k].w, z[k].z) };
			if (i0 >= 1 && i0 + 8 <= n) { // the common case: all eight are deltas of the read
#pragma unroll
				for (int q = 0; q < 4; q++) {
					atomicAdd(&my[min(zz[q] & 0xFFFFu, 256u)], 1u);
					atomicAdd(&my[min(zz[q] >> 16, 256u)], 1u);
				}
			} else if (i0 < n) { // sample 0 of the read, or the read's last lane
#pragma unroll
				for (int q = 0; q < 8; q++) {
					const uint32_t i = i0 + q;
					if (i >= 1 && i < n)
						atomicAdd(&my[min((zz[q >> 1] >> (16 * (q & 1))) & 0xFFFFu, 256u)], 1u);
				}
			}
		}
	}
	__syncthreads();
	for (int b = threadIdx.x; b < TBINS; b += TWG) {
		uint64_t sum = 0;
#pragma unroll
		for (int c = 0; c < TCOPIES; c++)
			sum += s_h[c][b];
		if (sum)
			atomicAdd(counts + b, (unsigned long long) sum);
	}
}

uint64_t train_scratch_bytes(uint32_t max_chunks) { return (uint64_t) max_chunks * sizeof(TrainChunk); }

void launch_symbol_counts(const int16_t *sig, const uint64_t *off, const uint32_t *n, uint32_t nreads, uint64_t *counts,
			  void *chunks, uint32_t *nchunks, uint32_t max_chunks, uint32_t grid, hipStream_t s)
{
	(void) hipMemsetAsync(nchunks, 0, sizeof(uint32_t), s);
	hipLaunchKernelGGL(k_train_prep, dim3((nreads + 255) / 256), dim3(256), 0, s, off, n, nreads,
			   (TrainChunk *) chunks, nchunks, max_chunks);
	hipLaunchKernelGGL(k_symbol_count, dim3(grid), dim3(TWG), 0, s, sig, (const TrainChunk *) chunks,
			   (const uint32_t *) nchunks, max_chunks, (unsigned long long *) counts);
}

} // namespace ph

using namespace ph;

// ------------------------------------------------------------------ counts -> table (host)

namespace {

// calculate_huffman_codes (huffman.c:373) over 256 leaves, zero counts included, 64-bit node counts.  The
// array is sorted ascending by count with a STABLE sort (glibc's qsort is a merge sort for it), NULLs last;
// each round merges the first two into a node whose zero child is the first, puts the node at slot 0,
// empties slot 1 and sorts again.  Code bit k of a symbol = the k-th branch from the root.
// Returns the longest code.
uint32_t huffman_build(const uint64_t c[256], uint32_t len[256], uint64_t bits[256])
{
	struct Node {
		uint64_t count;
		int zero, one; // children, -1 for a leaf
	};
	std::vector<Node> nodes(256);
	std::vector<int> slot(256);
	for (int s = 0; s < 256; s++) {
		nodes[s] = { c[s], -1, -1 };
		slot[s] = s;
	}
	auto before = [&](int a, int b) { // SFComp: NULLs (-1) last, then ascending count
		if (a < 0 || b < 0)
			return a >= 0 && b < 0;
		return nodes[a].count < nodes[b].count;
	};
	std::stable_sort(slot.begin(), slot.end(), before);
	for (int i = 1; i < 256; i++) {
		const int m1 = slot[0], m2 = slot[1];
		nodes.push_back({ nodes[m1].count + nodes[m2].count, m1, m2 });
		slot[0] = (int) nodes.size() - 1;
		slot[1] = -1;
		std::stable_sort(slot.begin(), slot.end(), before);
	}
	uint32_t maxlen = 0;
	struct Walk {
		int node;
		uint32_t depth;
		uint64_t code;
	};
	std::vector<Walk> st{ { slot[0], 0, 0 } };
	while (!st.empty()) {
		const Walk w = st.back();
		st.pop_back();
		const Node &p = nodes[w.node];
		if (p.zero < 0) {
			len[w.node] = w.depth;
			bits[w.node] = w.code; // (only meaningful up to 64 bits: callers reject longer codes)
			maxlen = std::max(maxlen, w.depth);
			continue;
		}
		const uint64_t one = w.depth < 64 ? 1ull << w.depth : 0;
		st.push_back({ p.zero, w.depth + 1, w.code });
		st.push_back({ p.one, w.depth + 1, w.code | one });
	}
	return maxlen;
}

} // namespace

// The reference's construction; when its longest code exceeds max_bits, the counts max(1, c >> k) for
// k = 0, 1, 2, ... until a tree fits (k = 0 only lifts the zero counts to 1).  It ends: with every count
// at 1 (k = 63 at the latest) the tree is 8 levels deep.
extern "C" int press_hip_table_from_counts(const uint64_t counts[256], uint32_t max_bits, uint32_t len[256], uint64_t bits[256])
{
	if (!counts || !len || !bits)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	if (max_bits < 8 || max_bits > 24)
		return set_error(PRESS_HIP_EARG, "max_bits = %u: the device tables take 8 to 24", max_bits);
	uint64_t sum = 0;
	for (int s = 0; s < 256; s++) {
		if (sum + counts[s] < sum)
			return set_error(PRESS_HIP_EARG, "the counts add up to more than 2^64");
		sum += counts[s];
	}
	uint32_t l[256];
	uint64_t b[256];
	if (huffman_build(counts, l, b) > max_bits) {
		uint64_t c[256];
		for (uint32_t k = 0;; k++) {
			for (int s = 0; s < 256; s++)
				c[s] = std::max<uint64_t>(1, counts[s] >> k);
			if (huffman_build(c, l, b) <= max_bits)
				break;
		}
	}
	memcpy(len, l, sizeof l);
	memcpy(bits, b, sizeof b);
	return PRESS_HIP_OK;
}

// write_code_table (huffman.c:440): u32 BE number of codes, u32 BE "bytes encoded", then per symbol with a
// code {u8 symbol, u8 length, ceil(length / 8) code bytes, bit k of the code at bit k % 8 of byte k / 8}.
extern "C" int press_hip_write_table_file(const char *path, const uint32_t len[256], const uint64_t bits[256], uint32_t data_bytes)
{
	if (!path || !len || !bits)
		return set_error(PRESS_HIP_EARG, "NULL argument");
	std::vector<uint8_t> out(8);
	uint32_t count = 0;
	for (int s = 0; s < 256; s++) {
		if (!len[s])
			continue;
		if (len[s] > 64)
			return set_error(PRESS_HIP_EARG, "symbol %d: a code of %u bits (at most 64)", s, len[s]);
		count++;
		out.push_back((uint8_t) s);
		out.push_back((uint8_t) len[s]);
		for (uint32_t k = 0; k < len[s]; k += 8)
			out.push_back((uint8_t) (bits[s] >> k));
	}
	for (int i = 0; i < 4; i++) {
		out[i] = (uint8_t) (count >> (24 - 8 * i));
		out[4 + i] = (uint8_t) (data_bytes >> (24 - 8 * i));
	}
	FILE *fp = fopen(path, "wb");
	if (!fp)
		return set_error(PRESS_HIP_EARG, "cannot create %s", path);
	const bool ok = fwrite(out.data(), 1, out.size(), fp) == out.size();
	if (fclose(fp) != 0 || !ok)
		return set_error(PRESS_HIP_EARG, "cannot write %s", path);
	return PRESS_HIP_OK;
}
