// press_verify.hip - checking reads on the device: the CRC-32 (zlib's) of a read's samples, and the comparison of decoded
// samples with the samples they are meant to be (press_hip_signal_crc32, press_hip_depress_crc_batch,
// press_hip_verify_batch).
//
// Both passes run over k_pa_tiles' table: a read's room is cut into tiles of CHUNK samples, and a tile at or beyond the
// read's count ends at once.  Samples are read as in k_pa_convert: 8 per lane and step, one coalesced 16-byte load.
//
// The digest.  With raw(M) the CRC register after M from 0 and without the final xor (press_crc.h):
//     crc32(M) = raw(M) ^ mul(0xFFFFFFFF, x^(8 L)) ^ 0xFFFFFFFF,   raw(M) = XOR_k mul(raw(M_k), x^(8 t_k))
// for pieces M_k with t_k bytes of M behind them.  t_k depends on the read's count; counted from the read's START it does
// not: with e_k the byte offset of piece k's end,
//     raw(M) = mul(W, x^(8 L)),   W = XOR_k mul(raw(M_k), x^(-8 e_k))          (x^(2^32 - 1) = 1: x^(-e) exists)
//     crc32(M) = mul(W ^ 0xFFFFFFFF, x^(8 L)) ^ 0xFFFFFFFF
// so a tile's share of W is a function of its samples and its place alone, and x^(8 L) - the one power that depends on the
// count - is taken once per read by k_crc_finish.  The pieces are the 16-byte groups of the loads.  In a tile the group of
// lane t and step s ends 4096 s + 16 (t + 1) bytes behind the tile's start, so
//     W_tile = x^(-8 * 65536 j) * XOR_t x^(-128 (t + 1)) * c_t,   c_t = XOR_s raw16(group s, t) * K^s,   K = x^(-8 * 4096)
// c_t is a Horner chain over the lane's groups from the last to the first, c = mulK(c) ^ raw16(group): multiplying by the
// constant K is linear, four 256-entry tables by the bytes of c, and raw16 is sixteen such look-ups by the bytes of the
// group (tables of raw(b || k zero bytes)) - 20 ds_read_b32 per lane and 16 bytes, no general multiplication.  The lane's
// factor (a table of 256 constants), the tile's (a product over the bits of j; none for a read's first tile) and the wave's
// XOR reduction come once per tile, and each wave adds its share to the read's word with one atomicXor: XOR commutes, so
// the word is the same from run to run, and no workgroup waits for another.  The samples of a read's last group that lie
// beyond the count are zeroed: raw(valid || z zero bytes) = raw(valid) * x^(8 z), which is what the group's nominal end,
// z bytes behind the read's, asks for.
//
// The grid is persistent (workgroups stride over the tiles) so that the 20 KiB of tables are brought into LDS once per
// workgroup, not once per tile.

#include "press_crc.h"
#include "press_internal.h"
#include "press_wave.h"

namespace ph {

namespace {

constexpr uint32_t VF_FAIL = 0xFFFFFFFFu;  // out_n of a refused read
constexpr uint32_t VF_NONE = 0xFFFFFFFFu;  // first_bad: no difference (PRESS_HIP_VERIFIED)
constexpr uint32_t STEP_SAMPLES = 256 * 8; // samples a workgroup takes per step
constexpr uint32_t CRC_GRID = 2048;        // workgroups of the persistent grid at most (8 per CU fit the LDS)

struct alignas(16) CrcTables { // what a workgroup keeps in LDS: 20 tables of 256 words (copied 16 bytes at a time)
	uint32_t grp[16][256];   // grp[k][b] = raw(b || k zero bytes): byte 15 - k of a 16-byte group
	uint32_t step[4][256];   // step[j][b] = (b at byte j of a register) * x^(-8 * 4096)
};
struct CrcConsts {
	uint32_t lane[256];      // x^(-128 (t + 1))
	uint32_t tile[17];       // x^(-8 * 65536 * 2^k): the tile index has 17 bits
	uint32_t x2k[32];        // x^(2^k)
};

constexpr CrcTables make_tables()
{
	CrcTables t{};
	for (uint32_t b = 0; b < 256; b++)
		t.grp[0][b] = crc::byte_raw(b);
	for (int k = 1; k < 16; k++) // one more zero byte behind
		for (uint32_t b = 0; b < 256; b++)
			t.grp[k][b] = (t.grp[k - 1][b] >> 8) ^ t.grp[0][t.grp[k - 1][b] & 0xFFu];
	const uint32_t K = crc::xneg(8 * 4096);
	for (int j = 0; j < 4; j++) {
		uint32_t bit[8] = {};
		for (int i = 0; i < 8; i++)
			bit[i] = crc::mul(1u << (8 * j + i), K);
		for (uint32_t b = 1; b < 256; b++) { // linear: the entry without b's lowest bit, and that bit's
			int low = 0;
			while (!(b >> low & 1u))
				low++;
			t.step[j][b] = t.step[j][b & (b - 1)] ^ bit[low];
		}
	}
	return t;
}

constexpr CrcConsts make_consts()
{
	CrcConsts c{};
	const uint32_t g = crc::xneg(128);
	c.lane[0] = g;
	for (int t = 1; t < 256; t++)
		c.lane[t] = crc::mul(c.lane[t - 1], g);
	c.tile[0] = crc::xneg(8 * 65536);
	for (int k = 1; k < 17; k++)
		c.tile[k] = crc::mul(c.tile[k - 1], c.tile[k - 1]);
	c.x2k[0] = crc::ONE >> 1;
	for (int k = 1; k < 32; k++)
		c.x2k[k] = crc::mul(c.x2k[k - 1], c.x2k[k - 1]);
	return c;
}

__device__ const CrcTables d_crc_tab = make_tables();
__device__ const CrcConsts d_crc_con = make_consts();
static_assert(sizeof(CrcTables) == 20 * 1024, "CrcTables");

// XOR / minimum over the 64 lanes of a wave, in every lane
__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v ^= (uint32_t) __shfl_xor((int) v, d, 64);
	return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const uint32_t o = (uint32_t) __shfl_xor((int) v, d, 64);
		v = o < v ? o : v;
	}
	return v;
}

#ifndef PRESS_CRC_ABLATE
#define PRESS_CRC_ABLATE 0 // measurement builds: 1 no group look-ups, 2 no stride multiply, 3 no lane factor / reduction
#endif

// raw(the 16 bytes of q) from the tables at tab
__device__ __forceinline__ uint32_t crc_raw16(const uint32_t *tab, const uint4 q)
{
	const uint32_t w[4] = { q.x, q.y, q.z, q.w };
	uint32_t c = 0;
#pragma unroll
	for (int d = 0; d < 4; d++)
#pragma unroll
		for (int b = 0; b < 4; b++)
			c ^= tab[(15 - 4 * d - b) * 256 + ((w[d] >> (8 * b)) & 0xFFu)];
	return c;
}

// c * x^(-8 * 4096) from the tables at tab (CrcTables::step)
__device__ __forceinline__ uint32_t crc_step(const uint32_t *tab, uint32_t c)
{
	return tab[c & 0xFFu] ^ tab[256 + ((c >> 8) & 0xFFu)] ^ tab[512 + ((c >> 16) & 0xFFu)] ^ tab[768 + (c >> 24)];
}

// Workgroups stride over the tiles.  raw[r] ^= the tile's share of W (zeroed by the caller); a tile at or beyond the
// read's count, or of a refused read, adds nothing.  Loads stay inside [off[r], off[r] + roundup8(out_n[r])).
__global__ __launch_bounds__(256) void k_crc_tiles(const int16_t *sig, const uint64_t *off, const uint32_t *out_n, const uint2 *tiles,
						    const uint32_t *ntiles, uint32_t max_tiles, uint32_t *raw)
{
	__shared__ uint4 s_tab4[sizeof(CrcTables) / 16];
	{
		const uint4 *src = reinterpret_cast<const uint4 *>(&d_crc_tab);
		for (uint32_t i = threadIdx.x; i < sizeof(CrcTables) / 16; i += 256)
			s_tab4[i] = src[i];
	}
	__syncthreads();
	const uint32_t *s_grp = reinterpret_cast<const uint32_t *>(s_tab4);
	const uint32_t *s_step = s_grp + 16 * 256;
	const uint32_t lane_f = d_crc_con.lane[threadIdx.x];
	uint32_t nt = uni(*ntiles);
	nt = nt < max_tiles ? nt : max_tiles;
	const uint32_t mine = threadIdx.x * 8;
	for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {
		const uint32_t r = uni(tiles[t].x), j = uni(tiles[t].y);
		const uint32_t on = uni(out_n[r]);
		const uint64_t first = (uint64_t) j * CHUNK;
		if (on == VF_FAIL || first >= on)
			continue;
		const uint32_t len = on - first < CHUNK ? (uint32_t) (on - first) : CHUNK; // samples of the tile
		const uint32_t S = (len + STEP_SAMPLES - 1) / STEP_SAMPLES;                // steps, the last one may be ragged
		const int16_t *in = sig + uni64(off[r]) + first;
		uint32_t c = 0;
		// four steps' loads at a time, then their look-ups from the last group to the first (a lane without a group in a
		// step takes zeros: they leave c alone while it is still 0, as it is in front of the lane's last group)
		for (int s0 = (int) ((S - 1) & ~3u); s0 >= 0; s0 -= 4) {
			uint4 q[4];
#pragma unroll
			for (int u = 0; u < 4; u++) {
				const uint32_t i = mine + (uint32_t) (s0 + u) * STEP_SAMPLES;
				q[u] = make_uint4(0, 0, 0, 0);
				if (i < len)
					q[u] = ld16_stream(in + i);
			}
#pragma unroll
			for (int u = 3; u >= 0; u--) {
				if ((uint32_t) (s0 + u) >= S)
					continue; // (uniform)
				const uint32_t i = mine + (uint32_t) (s0 + u) * STEP_SAMPLES;
				const uint32_t nv = i < len ? len - i : 0u; // samples of the group inside the count
				uint32_t w[4] = { q[u].x, q[u].y, q[u].z, q[u].w };
				if (nv < 8) {
#pragma unroll
					for (uint32_t d = 0; d < 4; d++)
						w[d] &= nv >= 2 * d + 2 ? 0xFFFFFFFFu : nv == 2 * d + 1 ? 0xFFFFu : 0u;
				}
#if PRESS_CRC_ABLATE == 1
				c = crc_step(s_step, c) ^ w[0] ^ w[1] ^ w[2] ^ w[3];
#elif PRESS_CRC_ABLATE == 2
				c = (c >> 1) ^ crc_raw16(s_grp, make_uint4(w[0], w[1], w[2], w[3]));
#else
				c = crc_step(s_step, c) ^ crc_raw16(s_grp, make_uint4(w[0], w[1], w[2], w[3]));
#endif
			}
		}
#if PRESS_CRC_ABLATE == 3
		uint32_t v = c ^ lane_f;
		v = (uint32_t) __builtin_amdgcn_readlane((int) v, 0) ^ (uint32_t) __builtin_amdgcn_readlane((int) v, 63);
#else
		uint32_t v = wave_xor(crc::mul(c, lane_f));
#endif
		for (uint32_t k = 0; (j >> k) != 0; k++) // (uniform; nothing to do for a read's first tile)
			if (j >> k & 1u)
				v = crc::mul(v, d_crc_con.tile[k]);
		if ((threadIdx.x & 63) == 0 && v)
			atomicXor(&raw[r], v);
	}
}

// x^e over the table of x^(2^k)
__device__ __forceinline__ uint32_t crc_xpow(uint32_t e)
{
	uint32_t p = crc::ONE;
	for (uint32_t k = 0; (e >> k) != 0; k++)
		if (e >> k & 1u)
			p = crc::mul(p, d_crc_con.x2k[k]);
	return p;
}

// One thread per read: crc = mul(W ^ 0xFFFFFFFF, x^(16 * count)) ^ 0xFFFFFFFF; 0 for a refused read (and, by the formula,
// for an empty one).  16 * count has up to 36 bits: it is reduced mod 2^32 - 1, not truncated.
__global__ __launch_bounds__(256) void k_crc_finish(const uint32_t *out_n, uint32_t nreads, const uint32_t *raw, uint32_t *crc)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= nreads)
		return;
	const uint32_t on = out_n[r];
	uint32_t v = 0;
	if (on != VF_FAIL && on != 0)
		v = crc::mul(raw[r] ^ 0xFFFFFFFFu, crc_xpow(crc::fold((uint64_t) on * 16))) ^ 0xFFFFFFFFu;
	crc[r] = v;
}

// One workgroup per tile: the decoded samples against the caller's over [0, min(out_n[r], nsamp[r])); the smallest index
// that differs goes into first_bad[r] (preset to VF_NONE) with one atomicMin per wave.  Loads of either side stay inside
// [off[r], off[r] + roundup8(that minimum)); sig is only read.  DEG (press_hip_verify_degraded_batch): the caller's
// samples are the originals of a degraded archive, and the decoded ones are compared with D_b of them, taken in registers
// (degrade_pair; h2, m2: its constants) - no degraded copy of the originals exists.
template <bool DEG>
__global__ __launch_bounds__(256) void k_verify_cmp(const int16_t *dec, const int16_t *sig, const uint64_t *off, const uint32_t *nsamp,
						     const uint32_t *out_n, const uint2 *tiles, const uint32_t *ntiles, uint32_t *first_bad,
						     uint32_t h2, uint32_t m2)
{
	if (blockIdx.x >= uni(*ntiles))
		return; // (the grid is an upper bound)
	const uint32_t r = uni(tiles[blockIdx.x].x), j = uni(tiles[blockIdx.x].y);
	const uint32_t on = uni(out_n[r]), room = uni(nsamp[r]);
	if (on == VF_FAIL)
		return;
	const uint64_t lim = on < room ? on : room;
	const uint64_t first = (uint64_t) j * CHUNK;
	if (first >= lim)
		return;
	const uint64_t end = first + CHUNK < lim ? first + CHUNK : lim;
	const uint64_t o = uni64(off[r]);
	uint32_t bad = VF_NONE;
	for (uint64_t i = first + threadIdx.x * 8; i < end; i += STEP_SAMPLES) {
		const uint4 a = ld16_stream(dec + o + i);
		uint4 b = ld16_stream(sig + o + i);
		if (DEG)
			b = make_uint4(degrade_pair(b.x, h2, m2), degrade_pair(b.y, h2, m2), degrade_pair(b.z, h2, m2), degrade_pair(b.w, h2, m2));
		const uint32_t x[4] = { a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w };
		uint32_t m = 0; // bit e: sample e of the group differs
#pragma unroll
		for (int d = 0; d < 4; d++)
			m |= ((x[d] & 0xFFFFu) ? 1u : 0u) << (2 * d) | ((x[d] >> 16) ? 2u : 0u) << (2 * d);
		if (end - i < 8)
			m &= (1u << (uint32_t) (end - i)) - 1u;
		if (m && bad == VF_NONE)
			bad = (uint32_t) i + (uint32_t) __builtin_ctz(m);
	}
	bad = wave_min(bad);
	if ((threadIdx.x & 63) == 0 && bad != VF_NONE)
		atomicMin(&first_bad[r], bad);
}

// One thread per read: 0 for a refused read; the first difference; without one, min(out_n, n) where the counts differ;
// else VF_NONE.  *nbad (zeroed by the caller) += the reads that are not VF_NONE, one atomic per wave.
__global__ __launch_bounds__(256) void k_verify_finish(const uint32_t *nsamp, const uint32_t *out_n, uint32_t nreads, uint32_t *first_bad,
							uint32_t *nbad)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	bool is_bad = false;
	if (r < nreads) {
		const uint32_t on = out_n[r], room = nsamp[r];
		uint32_t fb = first_bad[r];
		if (on == VF_FAIL)
			fb = 0;
		else if (fb == VF_NONE && on != room)
			fb = on < room ? on : room;
		first_bad[r] = fb;
		is_bad = fb != VF_NONE;
	}
	const unsigned long long b = __ballot(is_bad);
	if ((threadIdx.x & 63) == 0 && b)
		atomicAdd(nbad, (uint32_t) __popcll(b));
}

} // namespace

void launch_crc(const DecodeArgs &a, const uint2 *tiles, const uint32_t *ntiles, uint32_t *raw, uint32_t *crc, hipStream_t s)
{
	if (!a.nreads || !a.max_chunks)
		return;
	(void) hipMemsetAsync(raw, 0, (size_t) a.nreads * 4, s);
	const uint32_t grid = a.max_chunks < CRC_GRID ? a.max_chunks : CRC_GRID;
	hipLaunchKernelGGL(k_crc_tiles, dim3(grid), dim3(256), 0, s, (const int16_t *) a.sig, a.off, (const uint32_t *) a.out_n, tiles, ntiles,
			   a.max_chunks, raw);
	hipLaunchKernelGGL(k_crc_finish, dim3((a.nreads + 255) / 256), dim3(256), 0, s, (const uint32_t *) a.out_n, a.nreads,
			   (const uint32_t *) raw, crc);
}

void launch_verify_cmp(const DecodeArgs &a, const int16_t *sig, const uint2 *tiles, const uint32_t *ntiles, uint32_t *first_bad,
		       uint32_t *nbad, hipStream_t s, uint32_t bits)
{
	if (!a.nreads || !a.max_chunks)
		return;
	(void) hipMemsetAsync(first_bad, 0xFF, (size_t) a.nreads * 4, s);
	(void) hipMemsetAsync(nbad, 0, 4, s);
	if (bits)
		hipLaunchKernelGGL(k_verify_cmp<true>, dim3(a.max_chunks), dim3(256), 0, s, (const int16_t *) a.sig, sig, a.off, a.nsamp,
				   (const uint32_t *) a.out_n, tiles, ntiles, first_bad, degrade_h2(bits), degrade_m2(bits));
	else
		hipLaunchKernelGGL(k_verify_cmp<false>, dim3(a.max_chunks), dim3(256), 0, s, (const int16_t *) a.sig, sig, a.off, a.nsamp,
				   (const uint32_t *) a.out_n, tiles, ntiles, first_bad, 0u, 0u);
	hipLaunchKernelGGL(k_verify_finish, dim3((a.nreads + 255) / 256), dim3(256), 0, s, a.nsamp, (const uint32_t *) a.out_n, a.nreads,
			   first_bad, nbad);
}

} // namespace ph
