// press_dhuf_walk.h - host only: how many samples the stream of a huffman_*_zd read holds.
//
// The reference's per-read depress symbols take the stream's byte count and a capacity in *nout (press.c:4011); the
// batch call wants the exact sample count n = 1 + nex + nlow.  nex is the section's first field and nlow the count
// field of the Huffman table behind the section: this reads those two, through the section's own length fields, and
// nothing outside [in, in + len).  Plain C++ without the device: tools/dhuf_walk_check.cpp runs it under the
// sanitizers.
#pragma once

#include <stdint.h>
#include <string.h>

namespace ph {

// layout: 0 vbe21, 1 vbbe21, 2 vbsbe21, 3 vbsse21 (enum press_hip_rcf_layout).  false: the stream ends before the
// table's count field, or says more than 2^32 - 1 samples
inline bool dhuf_stream_samples(int layout, const uint8_t *in, uint64_t len, uint64_t *n)
{
	if (len < 2 + 4)
		return false;
	uint32_t nex;
	memcpy(&nex, in + 2, 4);
	uint64_t head = 2 + 4;
	if (layout == 0) {
		head += 6ull * nex;
	} else if (nex == 1) {
		head += 6;
	} else if (nex > 1) {
		uint32_t lp, lv;
		if (len < head + 4)
			return false;
		memcpy(&lp, in + head, 4);
		if (len < head + 8 + (uint64_t) lp)
			return false;
		memcpy(&lv, in + head + 4 + lp, 4);
		head += 8ull + lp + lv;
	}
	if (len < head + 5)
		return false;
	const uint8_t *t = in + head;
	const uint64_t nlow = ((uint32_t) t[1] << 24) | ((uint32_t) t[2] << 16) | ((uint32_t) t[3] << 8) | t[4];
	const uint64_t total = 1 + (uint64_t) nex + nlow;
	if (total > 0xFFFFFFFFull)
		return false;
	*n = total;
	return true;
}

} // namespace ph
