// press_crc.h - arithmetic of zlib's CRC-32 in GF(2)[x] mod P, shared by the host helper (press_crc.cpp) and the
// kernels of press_verify.hip.  Everything is constexpr: the kernels' tables are made by the compiler.
//
// Reflected 32-bit words: bit 31 is the coefficient of x^0, bit 30 of x^1, ... (0x80000000 is 1, 0x40000000 is x).
// raw(M) is the CRC register after M with initial value 0 and no final xor: M(x) * x^32 mod P; a register c followed by
// t zero bytes becomes mul(c, xpow(8 t)).  P is irreducible, so x^(2^32 - 1) = 1 and exponents count mod 2^32 - 1:
// x^(-e) is x^(2^32 - 1 - e).
#pragma once

#include <stdint.h>

namespace ph {
namespace crc {

constexpr uint32_t POLY = 0xEDB88320u;
constexpr uint32_t ONE = 0x80000000u;

// a * b mod P
constexpr uint32_t mul(uint32_t a, uint32_t b)
{
	uint32_t r = 0;
	for (int i = 0; i < 32; i++) {
		r ^= (a & (ONE >> i)) ? b : 0u;
		b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
	}
	return r;
}

// e mod 2^32 - 1 for an exponent of up to 64 bits (2^32 = 1 there: the halves add up); 2^32 - 1 itself may come out, which is
// as good as 0
constexpr uint32_t fold(uint64_t e)
{
	e = (e & 0xFFFFFFFFull) + (e >> 32);
	e = (e & 0xFFFFFFFFull) + (e >> 32);
	return (uint32_t) e;
}

// x^(2^k)
constexpr uint32_t x2k(int k)
{
	uint32_t p = ONE >> 1;
	for (int i = 0; i < k; i++)
		p = mul(p, p);
	return p;
}

// x^e, square and multiply
constexpr uint32_t xpow(uint32_t e)
{
	uint32_t p = ONE, sq = ONE >> 1;
	for (; e; e >>= 1) {
		if (e & 1u)
			p = mul(p, sq);
		sq = mul(sq, sq);
	}
	return p;
}

constexpr uint32_t xneg(uint32_t e) { return xpow(0xFFFFFFFFu - e); } // x^(-e), e < 2^32 - 1

// the register after the one byte b: the table of the byte-wise CRC
constexpr uint32_t byte_raw(uint32_t b)
{
	for (int i = 0; i < 8; i++)
		b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
	return b;
}

// crc32(A || B) of crc32(A), crc32(B) and |B| in bytes
constexpr uint32_t combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
	// (8 |B| of a 64-bit |B| has up to 67 bits: |B| is reduced before the factor 8, the product again - never truncated)
	const uint32_t l = fold(len_b);
	return mul(crc_a, xpow(fold((uint64_t) l * 8))) ^ crc_b;
}

} // namespace crc
} // namespace ph
