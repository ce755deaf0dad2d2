// press_crc.cpp - press_hip_crc32_combine: the CRC-32 of two pieces put together (include/press_hip.h).  Host
// arithmetic over press_crc.h, no GPU and no HIP header.

#include "../../include/press_hip.h"
#include "press_crc.h"

extern "C" uint32_t press_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
	return ph::crc::combine(crc_a, crc_b, len_b);
}
