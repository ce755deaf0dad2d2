"""Yardstick and reads for the stall methods (tests/test_stall_methods.py, tests/golden/make_stall_golden.py).

The expected stream of rccm_svbbe21_zd / dstall_fz_1500 / dstall_fz (press.c:7716-8148) is COMPOSED here from parts that
are pinned elsewhere: the jnn yardstick of tests/test_signal_segments.py (equal to sigtk's jnn_raw on sigtk_jnn.json),
the oracle's po_press(rccm_vbbe21_zd), po_uint_pack and po_rcms_encode (equal to the compiled reference on the golden
files of tests/test_oracle_golden.py).  tests/golden/ref_stall.json holds what the REAL reference makes of the reads
below; a CPU test proves yardstick == fixture before any GPU test uses the yardstick.

Nothing here touches a GPU.
"""
import ctypes
import hashlib
import json
import os
import struct

import numpy as np

import _layouts
import _libs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STALL_METHODS = ("rccm_svbbe21_zd", "dstall_fz_1500", "dstall_fz")
THRESHOLD = {"rccm_svbbe21_zd": 140, "dstall_fz_1500": 1500, "dstall_fz": 140}
CDNA = (0.75, 50, 50, 150, 0.25, 5, 0.0, 0.0)  # JNNV1_CDNA_PARAM (jnn.h:40-49)
FAILED = None  # what expected() gives for a read the method refuses


# ------------------------------------------------------------------ the yardstick

def first_segment(s):
    """segs[0] of jnn_raw under JNNV1_CDNA_PARAM, or None"""
    import test_signal_segments as TSS

    if len(s) == 0:
        return None
    segs, _ = TSS.yard_segments(s, None, CDNA)
    return (int(segs[0][0]), int(segs[0][1])) if len(segs) else None


def stall_of(seg, T):
    """find_stall and the head of X_press_16: -> (exists, stall_start, stall_len), the 16-bit truncations kept;
    no segment: no stall (definition 1)"""
    if seg is None:
        return 0, 0, 0
    start, ln = seg[0] & 0xFFFF, (seg[1] - seg[0] + 1) & 0xFFFF
    if ln < T:
        return 0, 0, 0
    return 1, (start + 20) & 0xFFFF, ln - 40


def _pack(vals, width):
    lib = _libs.oracle().lib
    a = np.ascontiguousarray(vals, dtype=np.uint32 if width == 32 else np.uint16)
    out = np.zeros(8 * len(a) + 64, dtype=np.uint8)
    n = lib.po_uint_pack(a.ctypes.data, len(a), width, out.ctypes.data)
    return out[:n].tobytes()


def vbbe21_section(y):
    """'u32 nex || section' and the one-byte values of vbbe21_press over the uint16 values y (press.c:2679-3405)"""
    y = np.asarray(y, dtype=np.uint16)
    pos = np.flatnonzero(y > 255).astype(np.uint32)
    val = y[pos].astype(np.uint32) - 256
    sec = struct.pack("<I", len(pos))
    if len(pos) == 1:
        sec += struct.pack("<IH", int(pos[0]), int(val[0]))
    elif len(pos) > 1:
        d = pos.copy()
        d[1:] = pos[1:] - pos[:-1] - 1
        bp, bv = _pack(d, 32), _pack(val, 16)
        sec += struct.pack("<I", len(bp)) + bp + struct.pack("<I", len(bv)) + bv
    return sec, y[y <= 255].astype(np.uint8)


def rcms(low):
    lib = _libs.oracle().lib
    lib.po_rcms_encode.restype = ctypes.c_uint64
    lib.po_rcms_encode.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    low = np.ascontiguousarray(low, dtype=np.uint8)
    out = np.zeros(2 * len(low) + 1024, dtype=np.uint8)
    n = lib.po_rcms_encode(low.ctypes.data, len(low), out.ctypes.data)
    return out[:n].tobytes()


def submin_stream(x):
    """rccm_vbbe21_submin_press_16 (press.c:8042): [min u16][section of x - min][rcms of the one-byte values]"""
    x = np.asarray(x).view(np.uint16)
    mn = int(x.min())
    sec, low = vbbe21_section((x.astype(np.int64) - mn).astype(np.uint16))
    return struct.pack("<H", mn) + sec + rcms(low)


def zd_stream(s):
    """rccm_vbbe21_zd of s, or None where the oracle refuses it"""
    ret, c = _libs.oracle().press("rccm_vbbe21_zd", s, cap=8 * len(s) + 4096)
    return c if ret == 0 else None


def stall_stream(s, T, seg="find"):
    """X_press_16 with threshold T -> (stream or None, (stall_start, stall_len)); None: the rest is refused (n = 0), or
    the stall piece passes 65535 bytes (definition 2)"""
    s = np.asarray(s, dtype=np.int16)
    if isinstance(seg, str):
        seg = first_segment(s)
    ex, ss, sl = stall_of(seg, T)
    head = bytes([ex])
    if ex:
        piece = submin_stream(s[ss:ss + sl])
        if len(piece) > 65535:
            return None, (0, 0)
        head += struct.pack("<HHH", ss, sl, len(piece)) + piece
    rest = zd_stream(np.concatenate([s[:ss], s[ss + sl:]]))
    if rest is None:
        return None, (0, 0)
    return head + struct.pack("<I", len(rest)) + rest, (ss, sl)


def choose(stall, whole):
    """dstall_fz's choice (press.c:8006): the stall stream only where it is STRICTLY shorter than the bare
    rccm_vbbe21_zd stream of the read; stall None: the other form (definition 2)"""
    if stall is not None and len(stall) < len(whole):
        return stall, True
    return b"\0" + struct.pack("<I", len(whole)) + whole, False


def expected(method, s, seg="find"):
    """-> (stream or FAILED, (stall_start, stall_len) as written into it)"""
    s = np.asarray(s, dtype=np.int16)
    if len(s) == 0:
        return FAILED, (0, 0)
    st, where = stall_stream(s, THRESHOLD[method], seg)
    if method != "dstall_fz":
        return st, where if st is not None else (0, 0)
    whole = zd_stream(s)
    if whole is None:
        return FAILED, (0, 0)
    out, kept = choose(st, whole)
    return out, where if kept and out[0] == 1 else (0, 0)


def parse(stream):
    """-> dict of the header fields and the two pieces of a stall-method stream"""
    ex = stream[0]
    d = {"exists": ex, "stall_start": 0, "stall_len": 0, "nstall": 0, "stall": b""}
    pos = 1
    if ex:
        d["stall_start"], d["stall_len"], d["nstall"] = struct.unpack_from("<HHH", stream, 1)
        d["stall"] = stream[7:7 + d["nstall"]]
        pos = 7 + d["nstall"]
    d["nrest"], = struct.unpack_from("<I", stream, pos)
    d["rest_at"] = pos + 4
    d["rest"] = stream[pos + 4:pos + 4 + d["nrest"]]
    return d


# ------------------------------------------------------------------ the reads

def _outside(rng, n, lo=60, hi=1140, dwell=40):
    """the wide-swinging part of a read: `dwell` samples at lo, a ramp of 40 a sample up to hi, `dwell` there, the ramp
    down ..., starting with a dwell at lo.  The ramps cross any band of mean +- 0.75 sigma around 600 in under 38 samples,
    too few for jnn's first segment, and no step is an exception of the coder"""
    ramp = np.arange(lo, hi, 40)
    cycle = np.concatenate([np.full(dwell, lo), ramp, np.full(dwell, hi), ramp[::-1] + 40])
    w = np.tile(cycle, n // len(cycle) + 1)[:n]
    return np.clip(w + rng.integers(-2, 3, size=n), 0, 1200).astype(np.int16)


def stall_read(seed, before, run, after, values=None, spread=3, **wave):
    """`before` outside samples that end in a dwell at lo, `run` in-band ones around 600 (values: given), `after`
    outside ones that begin with one.  jnn's first segment of such a read is (before, before + run): the five samples
    the walk tolerates behind the run are taken back again, and the end is the first sample behind it -
    y - x + 1 = run + 1"""
    rng = np.random.default_rng(seed)
    mid = (600 + rng.integers(-spread, spread + 1, size=run)).astype(np.int16) if values is None else np.asarray(values, dtype=np.int16)
    assert len(mid) == run
    return np.concatenate([_outside(rng, before, **wave)[::-1], mid, _outside(rng, after, **wave)]).astype(np.int16)


def smooth_read(seed, before, run, after):
    """a slowly wandering read with a flat stretch: the whole read codes well, so the stall form gains little"""
    rng = np.random.default_rng(seed)
    a = 300 + np.cumsum(rng.integers(-2, 3, size=before))
    b = 900 + np.cumsum(rng.integers(-2, 3, size=after))
    mid = 600 + rng.integers(-1, 2, size=run)
    return np.clip(np.concatenate([a, mid, b]), -32768, 32767).astype(np.int16)


def generated_reads():
    """-> list of (name, samples, first segment the design aims at or None): the same on every run"""
    out = []
    for want in (139, 140, 141, 1499, 1500, 1501):  # stall_len of find_stall = run + 1
        out.append(("len-%d" % want, stall_read(want, 300, want - 1, 400), (300, 300 + want - 1)))
    out.append(("at-0", stall_read(11, 0, 400, 700), (0, 400)))
    # five tolerated samples, one in the band again, and the read's last sample closes the segment ON that sample
    tail = stall_read(12, 600, 500, 7)
    tail[-2] = 600
    out.append(("to-end", tail, (600, 1106)))
    out.append(("start-beyond-65535", stall_read(13, 66000, 700, 900), (66000, 66700)))
    out.append(("len-beyond-65536", stall_read(14, 30000, 65536 + 300, 25000), (30000, 30000 + 65836)))
    out.append(("len-truncated-under-140", stall_read(15, 30000, 65536 + 99, 25000), (30000, 30000 + 65635)))
    rng = np.random.default_rng(16)
    out.append(("stall-exceptions", stall_read(16, 2000, 1200, 2000, values=rng.integers(440, 760, size=1200)), (2000, 3200)))
    one = np.full(300, 600)
    one[30] = 590  # (the stall is the run without its first and last 20 samples)
    one[120] = 590 + 300
    out.append(("stall-one-exception", stall_read(17, 900, 300, 900, values=one), (900, 1200)))
    two = one.copy()
    two[250] = 590 + 256
    out.append(("stall-two-exceptions", stall_read(18, 900, 300, 900, values=two), (900, 1200)))
    out.append(("smooth-prefers-whole", smooth_read(19, 500, 180, 500), None))
    # definition 2: a stall of 65000 samples most of which are exceptions of 9 bits - its piece passes 65535 bytes; the
    # read around it swings between 0 and 1200, so that mean +- 0.75 sigma still holds the stall
    # (a walk folded into 320 .. 880 in steps of at most 100: no exception among its DELTAS, so the whole read and the
    # rest stay within the inner coder's 65535-byte section; most of its VALUES minus their minimum pass 255)
    t = np.cumsum(np.random.default_rng(20).integers(-100, 101, size=65000)) % 1120
    big = 320 + np.where(t < 560, t, 1120 - t)
    out.append(("stall-piece-over-65535", stall_read(21, 27000, 65000, 27000, values=big, lo=0, hi=1200, dwell=200), (27000, 92000)))
    return out


def tie_candidates(count=400):
    """small reads for the search of a dstall_fz tie (both forms equally long): (name, samples)"""
    for k in range(count):
        rng = np.random.default_rng(5000 + k)
        run = int(rng.integers(139, 260))
        yield "tie-%d" % k, smooth_read(6000 + k, int(rng.integers(60, 300)), run, int(rng.integers(60, 300)))


def named_reads():
    """every read of the fixture: the three real reads, the battery's non-empty reads, the generated ones and the
    tie read the generator found (if any)"""
    out = []
    flat = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    o = 0
    for r in json.load(open(os.path.join(GOLD, "three_reads.json")))["reads"]:
        out.append(("three_reads/" + r["read_id"], flat[o:o + r["n"]].copy()))
        o += r["n"]
    for name, s in _layouts.battery():
        if len(s):
            out.append(("battery/" + name, s))
    for name, s, _ in generated_reads():
        out.append(("gen/" + name, s))
    tie = fixture().get("tie")
    if tie:
        for name, s in tie_candidates():
            if name == tie:
                out.append(("gen/" + name, s))
    return out


_fx = {}


def fixture():
    if "f" not in _fx:
        path = os.path.join(GOLD, "ref_stall.json")
        _fx["f"] = json.load(open(path)) if os.path.exists(path) else {}
    return _fx["f"]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()
