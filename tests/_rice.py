"""Yardstick and reads for the Rice family (tests/test_rice_family.py, tests/golden/make_rice_golden.py): the four
methods rice_{vbe21, vbbe21, vbsbe21, vbsse21}_zd of press/press.h.

A numpy restatement of rice(low) (press.c:4860-4924) and of its decoder as include/press_hip.h section (2u) defines it
(the run of ones counted modulo 256, the value cut to a byte, zeros behind the stream's end), proven against
tests/golden/ref_rice.json (the compiled reference) by CPU tests before any GPU test uses it.  The splice - header and
section of the plain layout in front of the payload - goes through _rcf.split.

Nothing here touches a GPU.
"""
import json
import os

import numpy as np

import _libs
import _rcf

LAYOUTS = _rcf.LAYOUTS
sha = _rcf.sha


def name(layout):
    return "rice_%s_zd" % layout


# ------------------------------------------------------------------ rice(low), restated

def pick_k(low):
    """the smallest k of 0 .. 7 that minimises sum((x >> k) + 1 + k); 0 without a value -> (k, that sum)"""
    x = np.frombuffer(bytes(low), dtype=np.uint8).astype(np.int64)
    costs = [int((x >> k).sum()) + len(x) * (1 + k) for k in range(8)]
    k = int(np.argmin(costs))  # (the first minimum: ties go to the lower k)
    return k, costs[k]


def encode(low):
    """-> (payload with zero padding bits, k, nbits)"""
    x = np.frombuffer(bytes(low), dtype=np.uint8).astype(np.int64)
    k, cost = pick_k(low)
    nbits = 3 + cost
    bits = np.zeros(nbits, dtype=np.uint8)
    bits[0], bits[1], bits[2] = (k >> 2) & 1, (k >> 1) & 1, k & 1
    q = x >> k
    lens = q + 1 + k
    starts = 3 + np.cumsum(lens) - lens
    # the runs of ones: value i owns q[i] positions from starts[i] on
    first = np.cumsum(q) - q
    ones = np.repeat(starts - first, q) + np.arange(int(q.sum()))
    bits[ones] = 1
    for j in range(k):  # the low k bits, most significant first
        bits[starts + q + 1 + j] = (x >> (k - 1 - j)) & 1
    payload = np.packbits(bits, bitorder="little").tobytes()
    assert len(payload) == (nbits - 1) // 8 + 1
    return payload, k, nbits


def decode(payload, n):
    """n values out of `payload`: the run counted modulo 256, the value cut to a byte, bits behind the end zero"""
    payload = bytes(payload)
    real = 8 * len(payload)
    bits = np.unpackbits(np.frombuffer(payload + b"\0" * 4, dtype=np.uint8), bitorder="little")
    k = int(bits[0]) << 2 | int(bits[1]) << 1 | int(bits[2])
    zeros = np.flatnonzero(bits == 0)
    nxt = np.searchsorted(zeros, zeros + 1 + k).tolist()  # the zero that ends the code behind the one a zero ends
    zl = zeros.tolist()
    term = []
    start = 3
    j = int(np.searchsorted(zeros, 3))
    while len(term) < n and start < real:
        term.append(j)
        start = zl[j] + 1 + k
        j = nxt[j]
    out = np.zeros(n, dtype=np.uint8)  # behind the end: a zero bit and k zero bits each
    if term:
        t = zeros[np.array(term)]
        s = np.concatenate([[3], t[:-1] + 1 + k])
        rem = np.zeros(len(t), dtype=np.int64)
        for i in range(k):
            rem = rem << 1 | bits[t + 1 + i]
        out[:len(t)] = ((((t - s) & 255) << k) | rem) & 255
    return out.tobytes()


# ------------------------------------------------------------------ the splice

def expected(layout, s):
    """the stream of rice_layout_zd -> (stream, k, nbits)"""
    s = np.ascontiguousarray(s, dtype=np.int16)
    payload, k, nbits = encode(_rcf.split("vbe21", s)[1])
    return _rcf.split(layout, s)[0] + payload, k, nbits


def head_len(layout, s):
    """bytes of header and section"""
    return len(_rcf.split(layout, np.ascontiguousarray(s, dtype=np.int16))[0])


def decoded(layout, stream, head, n):
    """the n samples a stream decodes to, `head` bytes of header and section in front of its payload: the payload through
    decode(), the plain stream through the oracle"""
    nex = int.from_bytes(stream[2:6], "little")
    low = decode(stream[head:], n - 1 - nex)
    ret, back = _libs.oracle().depress(layout + "_zd", stream[:head] + low, n)
    assert ret == 0
    return back


def clear_padding(stream, nbits):
    """the stream with the bits behind nbits in its last byte cleared (what "equal to the reference" compares)"""
    b = bytearray(stream)
    if nbits % 8:
        b[-1] &= (1 << (nbits % 8)) - 1
    return bytes(b)


# ------------------------------------------------------------------ the reads

def uniform_low(U, count=4000):
    """count one-byte values drawn uniformly from [0, U)"""
    return bytes(np.random.default_rng(1000 + U).integers(0, U, size=count).astype(np.uint8))


EVERY_K = [(3, 0), (6, 1), (12, 2), (24, 3), (48, 4), (96, 5), (192, 6)]  # U -> the k it makes win


def long_runs_low():
    """3000 zeros with two values of 255 among them (k = 0: a value is its own run of ones and a zero bit).  Value 1023
    is the last of the writer's first unit: its run of 255 ones ends that unit's span, eight dwords on.  Value 2000 starts
    at bit 3 + 2000 + 255 = 2258 = 8 * 256 + 210: its run crosses the reader's subsequence boundary at bit 2304 (and the
    first one the boundary at 1280)."""
    low = bytearray(3000)
    low[1023] = 255
    low[2000] = 255
    return bytes(low)


def extra_reads():
    """the reads of the fixture beyond _rcf.named_reads()"""
    out = [("single-1", np.array([417], dtype=np.int16))]
    for U, k in EVERY_K:
        out.append(("uniform-U%d" % U, _rcf.from_low(uniform_low(U))))
    out.append(("all-255-x100", _rcf.from_low(bytes([255]) * 100)))
    out.append(("all-1-x1000", _rcf.from_low(bytes([1]) * 1000)))
    out.append(("long-runs", _rcf.from_low(long_runs_low())))
    return out


def named_reads():
    """every read of the fixture"""
    return _rcf.named_reads() + extra_reads()


_fx = {}


def fixture():
    if "f" not in _fx:
        _fx["f"] = json.load(open(os.path.join(_rcf.GOLD, "ref_rice.json")))
    return _fx["f"]
