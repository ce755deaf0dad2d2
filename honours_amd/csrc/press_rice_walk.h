// press_rice_walk.h - host only: how long the stream of a rice_*_zd read is, given its sample count.
//
// The reference's per-read depress symbols take the SAMPLE count, not the stream's length (press.c:5050): like the
// reference, the per-read symbols of press_dropin.hip find the stream's end by reading it - the section's own length
// fields, then one Rice code per one-byte value.  This reads exactly the bytes the reference's decoder reads and none
// behind the last code's last bit.  Plain C++ without the device: tools/rice_walk_check.cpp runs it under the
// sanitizers.
#pragma once

#include <stdint.h>
#include <string.h>

namespace ph {

// layout: 0 vbe21, 1 vbbe21, 2 vbsbe21, 3 vbsse21 (enum press_hip_rcf_layout).  false: the header contradicts n
inline bool rice_stream_len(int layout, const uint8_t *in, uint64_t n, uint64_t *len)
{
	if (n == 0)
		return false;
	uint32_t nex;
	memcpy(&nex, in + 2, 4);
	if ((uint64_t) nex >= n)
		return false;
	uint64_t head = 2 + 4;
	if (layout == 0) {
		head += 6ull * nex;
	} else if (nex == 1) {
		head += 6;
	} else if (nex > 1) {
		uint32_t lp, lv;
		memcpy(&lp, in + head, 4);
		memcpy(&lv, in + head + 4 + lp, 4);
		head += 8ull + lp + lv;
	}
	const uint64_t nlow = n - 1 - nex;
	const uint8_t *p = in + head;
	if (nlow == 0) { // (the reference reads the three bits of k even so)
		*len = head + 1;
		return true;
	}
	const uint32_t k = ((p[0] & 1u) << 2) | (p[0] & 2u) | ((p[0] >> 2) & 1u);
	uint64_t bit = 3;
	for (uint64_t i = 0; i < nlow; i++) {
		while ((p[bit >> 3] >> (bit & 7)) & 1u)
			bit++;
		bit += 1 + k;
	}
	*len = head + (bit - 1) / 8 + 1;
	return true;
}

} // namespace ph
