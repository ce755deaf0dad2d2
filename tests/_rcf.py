"""Yardsticks and reads for the range-coder family (tests/test_rc_family.py, tests/golden/make_rcf_golden.py): the
sixteen methods {rc, rcc, rccm, rccdf}_{vbe21, vbbe21, vbsbe21, vbsse21}_zd of press/press.h.

Two yardsticks, both proven against tests/golden/ref_rcf.json (the compiled reference) by CPU tests before any GPU test
uses them:

* cdf_encode / cdf_decode: a restatement of TurboRC's adaptive nibble-CDF coder (rccdfenc / rccdfdec), the variant
  WITHOUT __AVX2__: 64-bit range, 15-bit cumulative frequencies, 32-bit little-endian output words.
* the splice: the one-byte values are the same under all four layouts, so with P(L) the plain stream L_zd, nlow the
  number of one-byte values and sec(L) = P(L)[: len - nlow], the stream of coder C on layout L is sec(L) + tail(C), where
  tail(C) is what follows the section in the one stream of C that the oracle restates (rc_vbe21_zd and rcc_vbe21_zd
  behind 2 + 4 + 6 nex bytes, rccm_vbbe21_zd behind len(P(vbbe21)) - nlow bytes).

Nothing here touches a GPU.
"""
import hashlib
import json
import os
import struct

import numpy as np

import _libs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CODERS = ("rc", "rcc", "rccm", "rccdf")
LAYOUTS = ("vbe21", "vbbe21", "vbsbe21", "vbsse21")
M64 = (1 << 64) - 1
TOP = 1 << 32


def name(coder, layout):
    return "%s_%s_zd" % (coder, layout)


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


# ------------------------------------------------------------------ the CDF coder, restated

_MIX = np.array([[i if i <= s else i + 32752 for i in range(16)] for s in range(16)], dtype=np.int32)


def _tables():
    return [np.arange(16, dtype=np.int32) << 11 for _ in range(17)]


def _entry(t, j):
    return 32768 if j == 16 else int(t[j])


def cdf_encode(data, trace=None):
    """-> (payload, carries, gave_up, flush_words).  gave_up: the payload is `data` itself (rcutil_.h:161) and
    flush_words is 0; else flush_words is 1 or 2.  trace: a list that receives the bytes written so far at every carry"""
    data = bytes(data)
    n = len(data)
    m = _tables()
    low, rng = 0, M64
    out = bytearray()
    carries = 0
    giveup = n * 255 // 256 - 8

    def carry():
        if trace is not None:
            trace.append(len(out))
        q = len(out)
        while q >= 4:
            q -= 4
            w = (int.from_bytes(out[q:q + 4], "little") + 1) & 0xFFFFFFFF
            out[q:q + 4] = w.to_bytes(4, "little")
            if w:
                break

    for x in data:
        h = x >> 4
        for s, t in ((h, m[0]), (x & 15, m[1 + h])):
            ilow = low
            rng >>= 15
            a, b = _entry(t, s), _entry(t, s + 1)
            low = (low + rng * a) & M64
            rng = (rng * (b - a)) & M64
            if ilow > low:
                carries += 1
                carry()
            if rng < TOP:
                out += (low >> 32).to_bytes(4, "little")
                rng = (rng << 32) & M64
                low = (low << 32) & M64
            t += (_MIX[s] - t) >> 7
        if len(out) >= giveup:
            return data, carries, True, 0
    if rng < TOP:
        out += (low >> 32).to_bytes(4, "little")
        rng = (rng << 32) & M64
        low = (low << 32) & M64
    ilow = low
    if rng > (1 << 33):
        low = (low + TOP) & M64
        if ilow > low:
            carries += 1
            carry()
        out += (low >> 32).to_bytes(4, "little")
        words = 1
    else:
        low = (low + 1) & M64
        if ilow > low:
            carries += 1
            carry()
        out += (low >> 32).to_bytes(4, "little")
        out += (low & 0xFFFFFFFF).to_bytes(4, "little")
        words = 2
    return bytes(out), carries, False, words


def cdf_decode(payload, n):
    """n bytes out of `payload`; bytes beyond its end read as zero"""
    payload = bytes(payload)
    pos = 0

    def word():
        nonlocal pos
        w = int.from_bytes(payload[pos:pos + 4].ljust(4, b"\0"), "little")
        pos += 4
        return w

    m = _tables()
    rng = M64
    code = word() << 32
    code |= word()
    out = bytearray()
    for _ in range(n):
        x = 0
        t = m[0]
        for _k in range(2):
            rng >>= 15
            s = 15
            for j in range(16):
                if _entry(t, j + 1) * rng > code:
                    s = j
                    break
            rp = _entry(t, s) * rng
            rng = _entry(t, s + 1) * rng - rp
            code -= rp
            if rng < TOP:
                rng = (rng << 32) & M64
                code = ((code << 32) | word()) & M64
            t += (_MIX[s] - t) >> 7
            x = (x << 4) | s
            t = m[1 + s]
        out.append(x)
    return bytes(out)


# ------------------------------------------------------------------ the splice yardstick

_cache = {}


def _press(method, s):
    key = (method, s.tobytes())
    if key not in _cache:
        ret, c = _libs.oracle().press(method, s, cap=8 * len(s) + 4096)
        assert ret == 0, (method, len(s))
        _cache[key] = c
    return _cache[key]


def split(layout, s):
    """-> (header and section of layout_zd, the one-byte values)"""
    s = np.ascontiguousarray(s, dtype=np.int16)
    p = _press(layout + "_zd", s)
    nex = struct.unpack_from("<I", p, 2)[0]
    nlow = len(s) - 1 - nex
    return p[:len(p) - nlow], p[len(p) - nlow:]


def _cdf(low):
    key = ("cdf", bytes(low))
    if key not in _cache:
        _cache[key] = cdf_encode(low)
    return _cache[key]


def tail(coder, s):
    """the coder's payload of the read's one-byte values"""
    s = np.ascontiguousarray(s, dtype=np.int16)
    if coder == "rccdf":
        return _cdf(split("vbe21", s)[1])[0]
    if coder == "rccm":
        return _press("rccm_vbbe21_zd", s)[len(split("vbbe21", s)[0]):]
    c = _press(coder + "_vbe21_zd", s)
    nex = struct.unpack_from("<I", c, 2)[0]
    return c[2 + 4 + 6 * nex:]


def expected(coder, layout, s):
    """the stream of coder_layout_zd"""
    return split(layout, s)[0] + tail(coder, s)


def gave_up(coder, s):
    """the definition of press_hip_rcf_press_batch's raw[]: the payload has the length of the one-byte values and equals
    them (for rccdf this is the restatement's own flag: test_rc_family checks that the two agree)"""
    low = split("vbe21", s)[1]
    return len(low) > 0 and tail(coder, s) == low


# ------------------------------------------------------------------ the reads

def signal(seed, n, exr=0.0, spread=12, ex_lo=130, ex_hi=400):
    """n samples of a random walk with steps of about +-spread; a fraction exr of the steps are exceptions (a step of
    ex_lo .. ex_hi either way: its zig-zag value needs two bytes)"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-spread, spread + 1, size=n)
    if exr:
        ex = rng.random(n) < exr
        ex[0] = False
        mag = rng.integers(ex_lo, ex_hi, size=int(ex.sum()))
        # alternate the direction so that the walk stays in 16 bits
        sign = np.where(np.arange(len(mag)) % 2 == 0, 1, -1)
        d[ex] = mag * sign
    return (np.cumsum(d) + 500).astype(np.int64).astype(np.uint16).view(np.int16)


def exact_exceptions(seed, n, nex, spread=12):
    """n samples with exactly nex exceptions, spread evenly"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-spread, spread + 1, size=n)
    pos = 1 + (np.arange(nex) * (n - 1)) // max(nex, 1)
    d[pos] = np.where(np.arange(nex) % 2 == 0, 300, -300)
    return (np.cumsum(d) + 500).astype(np.int64).astype(np.uint16).view(np.int16)


def from_low(low, base=0):
    """the read of len(low) + 1 samples without exceptions whose one-byte values are `low`: sample 0 is `base`, every
    further step is the delta whose zig-zag value is the byte (the caller keeps the walk inside 16 bits)"""
    z = np.frombuffer(bytes(low), dtype=np.uint8).astype(np.int64)
    d = np.where(z & 1, -((z + 1) >> 1), z >> 1)
    s = np.concatenate([[base], base + np.cumsum(d)])
    assert s.min() >= -32768 and s.max() <= 32767
    return s.astype(np.int16)


def carry_read():
    """160 one-byte values whose coding carries while only the first output word is written (found by trying seeds;
    test_rc_family asserts the property with cdf_encode's trace)"""
    return bytes(np.random.default_rng(7).integers(0, 25, size=160).astype(np.uint8))


def real_reads():
    out = []
    flat = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    o = 0
    for r in json.load(open(os.path.join(GOLD, "three_reads.json")))["reads"]:
        out.append(("three_reads/" + r["read_id"], flat[o:o + r["n"]].copy()))
        o += r["n"]
    return out


def named_reads():
    """every read of the fixture"""
    out = real_reads()
    for n in (2, 3, 5, 9, 10, 11, 12, 20, 40, 100):
        out.append(("walk-%d" % n, signal(100 + n, n)))
    out.append(("constant-3000", np.full(3000, 417, dtype=np.int16)))
    # about 14 % exceptions, the other steps uniform over every one-byte value: every coder gives up
    out.append(("uniform-2000", signal(7, 2000, exr=0.14, spread=127)))
    out.append(("sparse-5000", signal(8, 5000, exr=0.015)))
    return out


_fx = {}


def fixture():
    if "f" not in _fx:
        _fx["f"] = json.load(open(os.path.join(GOLD, "ref_rcf.json")))
    return _fx["f"]
