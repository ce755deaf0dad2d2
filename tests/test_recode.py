"""press_hip_recode_batch (include/press_hip.h): streams of one method in, streams of another out, in one call.

What the call must give is what the ORACLE gives - oracle.press(dst, oracle.depress(src, stream)) - not what the
library's own two calls give; the two-call path is compared once (test_agrees_with_the_two_calls), from the other
side.  Inputs are chosen on the CPU before the GPU sees them: a read is a source stream of `src` only where the oracle
itself presses it with `src` and gets it back (the range coders store tiny reads raw, a static-Huffman stream may hold
no code at all: outside the reference's lossless domain, _layouts.py); a read `src` refuses altogether (an empty read
with the exception methods) goes in as the empty stream, which every decoder refuses by its length.

Layouts are the scattered ones of _layouts.py throughout: streams at odd offsets between noise, slots of any byte size
from an odd offset, rooms in a random order, an empty guard read behind every read.
"""
import ctypes
import hashlib
import json
import os
import struct
import zlib

import numpy as np
import pytest

import _layouts as L
import _libs
from honours_amd import press, synth

gpu = pytest.mark.gpu
METHODS = sorted(press.METHODS, key=lambda m: press.METHODS[m])
FUSED_SRC = ("svb12_zd", "svb_zd", "slow5_svb_zd")
FUSED_DST = tuple(m for m in METHODS if m in L.EX_FAMILY)  # the four vb formats, their shuffman_*, ex-zd, the range coders
EARG = -2
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EMPTY = np.zeros(0, dtype=np.int16)


# ------------------------------------------------------------------ without a GPU

def _api():
    from honours_amd import build
    build.build()
    return press.load_library()


def test_fused_pairs_without_gpu():
    """press_hip_recode_fused is 1 exactly for svb12_zd / svb_zd / slow5_svb_zd into the 12 exception-split methods"""
    lib = _api()
    assert len(FUSED_DST) == 12
    ones = {(s, d) for s in METHODS for d in METHODS if lib.press_hip_recode_fused(press.METHODS[s], press.METHODS[d]) == 1}
    assert ones == {(s, d) for s in FUSED_SRC for d in FUSED_DST}
    for s, d in ((-1, 5), (5, -1), (19, 5), (2, 19), (1 << 20, 5)):
        assert lib.press_hip_recode_fused(s, d) == 0
    assert press.recode_fused("slow5_svb_zd", "shuffman_vbe21_zd") and not press.recode_fused("svb12", "vbe21_zd")


def test_recode_workspace_without_gpu():
    """host arithmetic: monotone in the batch shape, at least what the batch calls of either method keep, the sample
    scratch (2 bytes a sample) on top when the caller keeps no samples, 0 for a bad id"""
    lib = _api()
    ws = lambda s, d, t, r, k: int(lib.press_hip_recode_workspace_bytes(press.METHODS[s], press.METHODS[d], t, r, k))
    one = lambda m, t, r: int(lib.press_hip_workspace_bytes(press.METHODS[m], t, r))
    totals = [1000, 100_000, 10_000_000, 930_000_000]
    reads = [1, 5, 64, 8192]
    for s in METHODS:
        for d in METHODS:
            for keep in (0, 1):
                w = {(t, r): ws(s, d, t, r, keep) for t in totals for r in reads}
                for (t, r), v in w.items():
                    assert v >= one(s, t, r) and v >= one(d, t, r), (s, d, t, r, v)
                    assert all(v <= w[(t2, r)] for t2 in totals if t2 >= t), (s, d, t, r)
                    assert all(v <= w[(t, r2)] for r2 in reads if r2 >= r), (s, d, t, r)
            for t in totals:
                assert ws(s, d, t, 64, 0) >= ws(s, d, t, 64, 1) + 2 * t, (s, d, t)
    for s, d in ((-1, 5), (5, 19), (19, 19), (3, -7)):
        assert lib.press_hip_recode_workspace_bytes(s, d, 100000, 4, 0) == 0


def test_bad_ids_without_gpu():
    """a method id out of range is PRESS_HIP_EARG before any device call: the same with and without a GPU"""
    lib = _api()
    a = np.zeros(64, dtype=np.uint64)
    p = a.ctypes.data
    for s, d in ((-1, 5), (5, -1), (19, 2), (2, 19), (1 << 20, 1 << 20)):
        assert lib.press_hip_recode_batch(s, d, p, p, p, p, p, 1, 8, p, p, p, p, p, 0) == EARG, (s, d)
        assert lib.press_hip_recode_batch(s, d, p, p, p, p, p, 1, 8, p, p, p, None, p, 1) == EARG, (s, d)
        assert "method" in press.last_error()


# ------------------------------------------------------------------ inputs and what the oracle makes of them

class Src:
    """the source streams of a list of (name, samples) for one method, made and checked by the oracle"""

    def __init__(self, oracle, m, reads):
        self.m = m
        self.items = []  # (name, samples the stream holds or EMPTY, stream)
        self.left_out = []
        for name, s in reads:
            ret, st = oracle.press(m, s, cap=L.slot_of(oracle.bound, m, len(s)))
            if ret != 0:
                self.items.append((name, EMPTY, b""))  # the method has no stream for this read: the empty one is refused
                continue
            verdict, back = L.expect_depress(oracle, m, s, st, len(s))
            if verdict != "ok" or not np.array_equal(back, s):
                self.left_out.append(name)  # the oracle does not give the read back: no input
                continue
            self.items.append((name, s, st))
        ret, g = oracle.press(m, EMPTY, cap=64)
        self.guard = g if ret == 0 else b""


_want = {}


def want_press(oracle, dst, s, cap=None):
    """the oracle's `dst` stream of s (zstd kinds: the frame's content), None where it refuses; cached by content"""
    if cap is not None:
        return L.expect_press(oracle, dst, s, cap)
    k = (dst, len(s), zlib.crc32(s.tobytes()))
    if k not in _want:
        _want[k] = L.expect_press(oracle, dst, s, L.slot_of(oracle.bound, dst, len(s)))
    return _want[k]


class Entry:
    def __init__(self, name, stream, room, cap, out_n, samples, want):
        self.name, self.stream, self.room, self.cap = name, stream, int(room), int(cap)
        self.out_n, self.samples, self.want = out_n, samples, want  # FAILED32 / None / None where refused


def entry(oracle, src, dst, name, s, st, rng, guard=False):
    """one read of a batch and what the oracle says about it.  s: the samples st holds (a well-formed stream)"""
    n = len(s)
    # (the svb kinds and the range coders take the sample count from the caller; the others a room that may be larger)
    room = n if src in L.SVB_KINDS or src in _libs.RC_FAMILY or guard else n + int(rng.integers(0, 21))
    if guard:
        w = want_press(oracle, dst, EMPTY, 1 << 20)
        cap = 64 if dst in L.ZSTD_KINDS else (len(w) if w is not None else 0) + 16
    else:
        cap = L.slot_of(oracle.bound, dst, n) + int(rng.integers(0, 16))
    verdict, back = L.expect_depress(oracle, src, s, st, room)
    assert verdict != "skip", (src, name)
    if verdict == "fail":
        return Entry(name, st, room, cap, L.FAILED32, None, None)
    assert np.array_equal(back, s), (src, name)
    return Entry(name, st, room, cap, len(back), back, want_press(oracle, dst, back, (1 << 20) if guard else None))


def batch_of(oracle, srcs, dst, rng, left_out=None):
    """every read of srcs with an empty guard read behind it.  A read of samples that the oracle's `dst` refuses to
    press is no input of this pair (exception-heavy reads beyond a format's 16-bit section length: outside the
    reference's domain, as in test_exception_heavy_sections) and is left out here, on the CPU; what `dst` does with an
    EMPTY read is pinned by the header and stays in."""
    out = []
    for name, s, st in srcs.items:
        e = entry(oracle, srcs.m, dst, name, s, st, rng)
        if e.out_n != L.FAILED32 and e.out_n > 0 and e.want is None:
            if left_out is not None:
                left_out.append(name)
            continue
        out.append(e)
        out.append(entry(oracle, srcs.m, dst, name + " guard", EMPTY, srcs.guard, rng, guard=True))
    return out


# ------------------------------------------------------------------ GPU plumbing

@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.load_table()
    press.use_torch_stream()
    lb.press_hip_host_alloc.restype = ctypes.c_void_p
    lb.press_hip_host_alloc.argtypes = [ctypes.c_uint64]
    lb.press_hip_host_free.argtypes = [ctypes.c_void_p]
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _p(x):
    return None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


class Run:
    """one press_hip_recode_batch call on a scattered layout; mode "dev", "host" or a function that gives
    page-locked copies of numpy arrays"""

    def __init__(self, lib, src, dst, entries, rng, mode="dev", keep_sig=True):
        import torch
        self.src, self.dst, self.entries, self.dev = src, dst, entries, mode == "dev"
        inb, in_off, in_len = L.scatter_streams(rng, [e.stream for e in entries])
        self.rooms = np.array([e.room for e in entries], dtype=np.uint32)
        # (page-locked samples: the copy back covers gaps under 128 bytes between rooms, press_hip.h - keep them apart)
        self.off, self.total = L.scatter_rooms(rng, self.rooms, min_gap=64 if callable(mode) else 0)
        self.out_off = L.slots(rng, [e.cap for e in entries])
        nb = int(self.out_off[-1]) + 4096
        nr = len(entries)
        sid, did = press.METHODS[src], press.METHODS[dst]
        if self.dev:
            t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else a.view(dt)).copy()).cuda()
            d_out = torch.full((nb,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
            d_len = torch.zeros(nr, dtype=torch.int64, device="cuda")
            d_outn = torch.zeros(nr, dtype=torch.int32, device="cuda")
            d_sig = torch.full((self.total,), L.SIG_FILL, dtype=torch.int16, device="cuda") if keep_sig else None
            args = (t(inb), t(in_off, np.int64), t(in_len, np.int64), t(self.rooms, np.int32), t(self.off, np.int64))
            d_oo = t(self.out_off, np.int64)
            rc = lib.press_hip_recode_batch(sid, did, *[_p(a) for a in args], nr, self.total, _p(d_out), _p(d_oo),
                                            _p(d_len), _p(d_sig), _p(d_outn), 1)
            assert rc == 0, (src, dst, press.last_error())
            torch.cuda.synchronize()
            self.arena = d_out.cpu().numpy()
            self.lens = d_len.cpu().numpy().view(np.uint64)
            self.out_n = d_outn.cpu().numpy().view(np.uint32)
            self.sig = d_sig.cpu().numpy() if keep_sig else None
            return
        pin = (lambda a: a) if mode == "host" else mode
        self.arena = pin(np.full(nb, L.ARENA_FILL, dtype=np.uint8))
        self.lens = np.zeros(nr, dtype=np.uint64)
        self.out_n = np.zeros(nr, dtype=np.uint32)
        self.sig = pin(np.full(self.total, L.SIG_FILL, dtype=np.int16)) if keep_sig else None
        rc = lib.press_hip_recode_batch(sid, did, _p(pin(inb)), _p(in_off), _p(in_len), _p(self.rooms), _p(self.off), nr,
                                        self.total, _p(self.arena), _p(self.out_off), _p(self.lens), _p(self.sig),
                                        _p(self.out_n), 0)
        assert rc == 0, (src, dst, press.last_error())

    def slot(self, k):
        return int(self.out_off[k]), int(self.out_off[k + 1])

    def stream(self, k):
        o0, _ = self.slot(k)
        return self.arena[o0:o0 + int(self.lens[k])].tobytes()

    def check(self, oracle):
        """every read as the oracle has it; refused reads' slots, the guards' slack, the arena around the slots and the
        samples outside the rooms untouched"""
        src, dst = self.src, self.dst
        for k, e in enumerate(self.entries):
            tag = (src, dst, k, e.name, e.room)
            o0, o1 = self.slot(k)
            ln = int(self.lens[k])
            assert int(self.out_n[k]) == e.out_n, tag + (int(self.out_n[k]), e.out_n)
            if e.out_n == L.FAILED32:
                assert ln == L.FAILED64, tag
                assert (self.arena[o0:o1] == L.ARENA_FILL).all(), tag + ("a refused read's slot was written",)
                continue
            if self.sig is not None:
                o = int(self.off[k])
                assert np.array_equal(self.sig[o:o + e.out_n], e.samples), tag
            if e.want is None:
                assert ln == L.FAILED64, tag + (ln,)
                if e.room == 0:
                    assert (self.arena[o0:o1] == L.ARENA_FILL).all(), tag
                continue
            assert ln != L.FAILED64 and ln <= o1 - o0, tag + (press.last_error(),)
            st = self.arena[o0:o0 + ln].tobytes()
            if dst in L.ZSTD_KINDS:
                L.check_zstd_frame(oracle, dst, e.samples, st, e.want)
            else:
                assert ln == len(e.want) and st == e.want, tag + (ln, len(e.want))
            if e.room == 0:
                assert (self.arena[o0 + ln:o1] == L.ARENA_FILL).all(), tag
        a0, a1 = int(self.out_off[0]), int(self.out_off[-1])
        assert (self.arena[:a0] == L.ARENA_FILL).all() and (self.arena[a1:] == L.ARENA_FILL).all(), (src, dst)
        if self.sig is not None:
            if self.dev:
                spans = [L.roundup8(r) for r in self.rooms]
            else:
                spans = [0 if int(x) == L.FAILED32 else int(x) for x in self.out_n]
            bad = np.nonzero(self.sig[:self.total][L.outside_rooms(self.total, self.off, spans)] != np.int16(L.SIG_FILL))[0]
            assert bad.size == 0, (src, dst, "samples written outside the rooms", bad[:8])


# ------------------------------------------------------------------ the batteries

def _walk(rng, n, exr=0.0, lo=-60, hi=60, big=30000):
    d = rng.integers(lo, hi + 1, size=n)
    ex = rng.random(n) < exr
    d[ex] = rng.integers(-big, big + 1, size=int(ex.sum()))
    return (np.cumsum(d) + 500).astype(np.int64).astype(np.uint16).view(np.int16)


def small_battery():
    """17 reads, 130 000 samples: every edge once, for all 19 x 19 pairs"""
    rng = np.random.default_rng(20261017)
    out = [("empty", EMPTY)]
    for n in (1, 2, 7, 8, 9, 63, 513, 2049):
        out.append(("walk-%d" % n, _walk(rng, n)))
    out.append(("ex1-32769", _walk(rng, 32769, 0.01)))
    out.append(("ex30-5000", _walk(rng, 5000, 0.30)))
    out.append(("all-exceptions-3000", np.where(np.arange(3000) % 2 == 0, 0, 1000).astype(np.int16)))
    out.append(("wrap-5000", _walk(rng, 5000, 0.05, big=40000)))
    out.append(("q8-10000", ((_walk(rng, 10000, 0.002) >> 3) << 3).astype(np.int16)))
    out.append(("constant-4000", np.full(4000, -1234, dtype=np.int16)))
    n, first = synth.read_lengths(7, 200, 1)
    out.append(("synth", synth.synth_read(7, 200, min(int(n[0]), 40000), int(first[0]))))
    out.append(("spikes-20000", _spikes(rng, 20000)))
    return out


def _spikes(rng, n):
    s = np.cumsum(rng.integers(-30, 31, size=n)).astype(np.int16)
    s[rng.integers(0, n, size=max(1, n // 500))] = rng.choice([-32768, 32767])
    return s


def full_battery():
    """the fused pairs' battery: every granule edge (lane 8, sub-tile 512, wave quarter 8192, chunk 32 768), a read of
    more than 100 chunks, and the value shapes that tell the 16-bit wrapped delta from svb-zd's own"""
    rng = np.random.default_rng(20261018)
    out = []
    for n in (0, 1, 2, 7, 8, 9, 511, 512, 513, 8191, 8192, 8193, 32767, 32768, 32769, 65537, 200000):
        out.append(("walk-%d" % n, _walk(rng, n, 0.004) if n else EMPTY))
    out.append(("chunks-101", _walk(rng, 100 * 32768 + 4321, 0.002)))
    ns, first = synth.read_lengths(7, 300, 4)
    for k in range(4):
        out.append(("synth-%d" % k, synth.synth_read(7, 300 + k, min(int(ns[k]), 150000), int(first[k]))))
    out.append(("pm1-70000", np.cumsum(rng.integers(-1, 2, size=70000)).astype(np.int16)))           # the low-entropy stretch
    out.append(("pm1-8200", (np.cumsum(rng.integers(-1, 2, size=8200)) + 3).astype(np.int16)))
    for n in (9, 513, 4095, 70001):
        out.append(("random-%d" % n, rng.integers(-32768, 32768, size=n).astype(np.int16)))          # most jumps are wide
    for n in (19, 512, 32769, 70001):
        out.append(("spikes-%d" % n, _spikes(rng, n)))
    for s0 in (128, -129, 255, 256, -32768, 32767, 12345):
        s = _walk(rng, 3000, 0.01).copy()
        s[0] = s0
        out.append(("first-%d" % s0, s))
    out.append(("first-only-min", np.array([-32768], dtype=np.int16)))
    for q in (1, 2, 3, 4, 5):
        s = _walk(rng, 40000 + q, 0.002)
        out.append(("q%d" % q, ((s >> q) << q).astype(np.int16)))
    # exception densities, at the sizes of test_exception_heavy_sections
    for n, rate, big in ((70000, 0.0, 0), (260000, 0.0004, 30000), (70000, 0.02, 3000), (3000, 0.3, 300), (40000, 0.3, 32000),
                         (70000, 0.9, 20000), (129, 0.5, 50)):
        d = rng.integers(-40, 41, size=n)
        ex = rng.random(n) < rate
        d[ex] = rng.integers(-big, big + 1, size=int(ex.sum()))
        out.append(("ex%g-%d" % (rate, n), np.cumsum(d).astype(np.int16)))
    return out


_srcs = {}


def sources(oracle, which, m):
    if (which, m) not in _srcs:
        _srcs[(which, m)] = Src(oracle, m, small_battery() if which == "small" else full_battery())
    return _srcs[(which, m)]


def test_batteries_keep_their_power(oracle):
    """what the input filter leaves out (CPU, oracle only): nothing for the svb sources; for the others only reads
    outside the reference's lossless domain - the range coders' raw-stored tiny reads, header-only static-Huffman
    streams, ex-zd's 16-bit section length"""
    for m in METHODS:
        s = sources(oracle, "small", m)
        print(m, "left out:", s.left_out, "refused:", [n for n, x, st in s.items if st == b""])
        assert len(s.items) + len(s.left_out) == 17
        assert len(s.left_out) <= (8 if m in _libs.RC_FAMILY else 2), (m, s.left_out)
        if m in L.SVB_KINDS:
            assert not s.left_out
    rng = np.random.default_rng(0)
    for m in FUSED_SRC:
        s = sources(oracle, "full", m)
        assert not s.left_out and len(s.items) == len(full_battery())
        assert max(len(x) for _, x, _ in s.items) >= 100 * 32768
        for dst in FUSED_DST:  # at most 3 of the 52 reads are beyond a destination's domain, all of them exception-heavy
            out = []
            batch_of(oracle, s, dst, rng, out)
            print(m, "->", dst, "left out:", out)
            assert len(out) <= 3 and all(x.startswith(("random-", "ex0.9-", "ex0.3-")) for x in out), (m, dst, out)
    for m in METHODS:
        for dst in METHODS:
            out = []
            batch_of(oracle, sources(oracle, "small", m), dst, rng, out)
            assert len(out) <= 2, (m, dst, out)


# ------------------------------------------------------------------ 1: golden

@gpu
def test_golden_three_reads(lib):
    """the three signal fields of three-reads.blow5 as stored -> each fused destination: the reference's lengths and
    hashes (three_reads.json)"""
    meta = {r["read_id"]: r for r in json.load(open(os.path.join(GOLD, "three_reads.json")))["reads"]}
    rd = press.Blow5Reader(os.path.join(GOLD, "three-reads.blow5"))
    batch = rd.next_batch()
    rd.close()
    assert len(batch) == 3 and rd.signal_method == 1
    flat = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    gold, o = {}, 0
    for r in json.load(open(os.path.join(GOLD, "three_reads.json")))["reads"]:
        gold[r["read_id"]] = flat[o:o + r["n"]]
        o += r["n"]
    for dst in FUSED_DST:
        assert press.recode_fused("slow5_svb_zd", dst)
        out, sigs = press.recode_batch_host("slow5_svb_zd", dst, [s for _, _, s in batch], [n for _, n, _ in batch],
                                            want_samples=True)
        total = 0
        for (rid, n, _), st in zip(batch, out):
            g = meta[rid]["methods"][dst]
            assert st is not None and len(st) == g["len"], (dst, rid)
            assert hashlib.sha256(st).hexdigest()[:32] == g["sha256_32"], (dst, rid)
            total += len(st)
        if dst == "shuffman_vbe21_zd":
            assert total == 175227
        assert all(np.array_equal(x, gold[rid]) for (rid, _, _), x in zip(batch, sigs)), dst


# ------------------------------------------------------------------ 2: the matrix

@gpu
@pytest.mark.parametrize("src", METHODS)
def test_matrix_every_pair(lib, oracle, src):
    """src -> each of the 19 methods on the small battery, device resident; the samples asked for on every other pair"""
    srcs = sources(oracle, "small", src)
    for i, dst in enumerate(METHODS):
        rng = np.random.default_rng(1000 * press.METHODS[src] + press.METHODS[dst])
        Run(lib, src, dst, batch_of(oracle, srcs, dst, rng), rng, keep_sig=(i + press.METHODS[src]) % 2 == 0).check(oracle)


@gpu
@pytest.mark.parametrize("src", FUSED_SRC)
def test_matrix_fused_full_battery(lib, oracle, src):
    srcs = sources(oracle, "full", src)
    for i, dst in enumerate(FUSED_DST):
        assert press.recode_fused(src, dst)
        rng = np.random.default_rng(77000 + 100 * press.METHODS[src] + press.METHODS[dst])
        Run(lib, src, dst, batch_of(oracle, srcs, dst, rng), rng, keep_sig=i % 2 == 1).check(oracle)


# ------------------------------------------------------------------ 3: layouts, host buffers

LAYOUT_PAIRS = [("slow5_svb_zd", "shuffman_vbe21_zd"), ("svb12_zd", "hasgam_vbsse21_zdq"), ("svb_zd", "rccm_vbbe21_zd"),
                ("vbe21_zd", "slow5_svb_zd"), ("shuffman_vbsse21_zd", "zstd_svb_zd"), ("zstd_svb_zd", "svb12")]


@gpu
@pytest.mark.parametrize("src,dst", LAYOUT_PAIRS)
def test_layouts_host_and_device(lib, oracle, src, dst):
    """pageable host buffers (one staged batch, then calls of at most 4 reads: the direct copies), page-locked ones and
    device-resident ones, each with and without the samples"""
    srcs = sources(oracle, "small", src)
    held = []

    def pinned(a):
        p = lib.press_hip_host_alloc(max(a.nbytes, 1))
        assert p
        held.append(p)
        v = np.frombuffer((ctypes.c_uint8 * a.nbytes).from_address(p), dtype=a.dtype)
        v[:] = a
        return v
    try:
        seed = 5000 + 31 * press.METHODS[src] + press.METHODS[dst]
        for j, (mode, keep) in enumerate((("host", True), ("host", False), (pinned, True), (pinned, False), ("dev", True),
                                          ("dev", False))):
            rng = np.random.default_rng(seed + j)
            ents = batch_of(oracle, srcs, dst, rng)
            Run(lib, src, dst, ents, rng, mode, keep).check(oracle)
            if mode == "host":
                for g0 in range(0, 12, 4):
                    Run(lib, src, dst, ents[g0 + 14:g0 + 18], rng, mode, keep).check(oracle)
    finally:
        for p in held:
            lib.press_hip_host_free(p)


# ------------------------------------------------------------------ 4: failures

def _bad_batch(oracle, dst, rng, reads):
    """slow5 svb-zd streams of `reads` with four bad ones between them -> (entries, indices of the good ones)"""
    src = "slow5_svb_zd"
    ents, good = [], []
    for k, s in enumerate(reads):
        ret, st = oracle.press(src, s)
        assert ret == 0
        good.append(len(ents))
        ents.append(entry(oracle, src, dst, "good-%d" % k, s, st, rng))
        n = len(s)
        bad = None
        if k == 1:
            bad = ("truncated", st[:-1], n)
        elif k == 2:
            bad = ("trailing byte", st + b"\0", n)
        elif k == 3:
            bad = ("wrong count", struct.pack("<I", n + 1) + st[4:], n)
        elif k == 4:
            bad = ("count alone", st[:3], n)
        if bad:
            assert oracle.depress(src, bad[1], bad[2])[0] != 0  # the oracle refuses it (by its length / its count)
            ents.append(Entry(bad[0], bad[1], bad[2], 4096, L.FAILED32, None, None))
        if k == 5:  # a slot one byte short of the stream: the read decodes, its press fails
            e = entry(oracle, src, dst, "small slot", s, st, rng)
            assert e.want is not None
            e.cap, e.want = (len(e.want) - 1 if dst not in L.ZSTD_KINDS else 8), None
            ents.append(e)
    return ents, good


@gpu
@pytest.mark.parametrize("dst", ["vbe21_zd", "shuffman_vbbe21_zd", "hasgam_vbsse21_zdq", "rc_vbe21_zd", "slow5_svb_zd",
                                 "zstd_svb_zd", "svb12_zd"])
def test_failures_stay_with_their_read(lib, oracle, dst):
    """a truncated stream, a trailing byte, a wrong count header, a stream shorter than its count and a slot that is
    too small: those reads fail as the header says - refused streams with out_n = UINT32_MAX, out_len = PRESS_HIP_FAILED
    and an untouched slot - and every other read is byte for byte what the batch without them gives"""
    rng = np.random.default_rng(90 + press.METHODS[dst])
    reads = [_walk(rng, n, 0.01) for n in (700, 32769, 513, 70001, 8, 40000, 9000, 1)]
    ents, good = _bad_batch(oracle, dst, rng, reads)
    a = Run(lib, "slow5_svb_zd", dst, ents, rng)
    a.check(oracle)
    clean = [ents[k] for k in good]
    b = Run(lib, "slow5_svb_zd", dst, clean, rng)
    b.check(oracle)
    if dst not in L.ZSTD_KINDS:
        for j, k in enumerate(good):
            assert a.stream(k) == b.stream(j) and a.out_n[k] == b.out_n[j], (dst, k)


@gpu
@pytest.mark.parametrize("src", ["slow5_svb_zd", "vbe21_zd"])
def test_value_without_a_code_fails_its_read_only(lib, oracle, tmp_path, src):
    """a static-Huffman table that lacks a code for a value one read holds: that read decodes and its press fails, the
    others are the oracle's - through the fused decode kernel (slow5_svb_zd) and through pass A (vbe21_zd)"""
    lens = [4] * 8 + [5] * 16  # 24 symbols, Kraft sum = 1 (test_huffman_table_with_fewer_symbols)
    order = sorted(range(24), key=lambda s: (lens[s], s))
    code, prev, bits = 0, lens[order[0]], [0] * 24
    for sy in order:
        code <<= lens[sy] - prev
        prev = lens[sy]
        bits[sy] = int(format(code, "0%db" % lens[sy])[::-1], 2)
        code += 1
    blob = bytearray((24).to_bytes(4, "big") + bytes(4))
    for sy in range(24):
        blob += bytes([sy, lens[sy]]) + bits[sy].to_bytes((lens[sy] + 7) // 8, "little")
    path = str(tmp_path / "partial.huffman")
    open(path, "wb").write(bytes(blob))
    rng = np.random.default_rng(4)
    good = np.cumsum(rng.integers(-11, 12, size=70000)).astype(np.int16)  # zig-zag deltas 0..22
    bad = good.copy()
    bad[40000:] += 100  # one delta of 100: zig-zag 200, no code
    try:
        oracle.load_table(path)
        press.use_table(path)
        for dst in ("shuffman_vbe21_zd", "shuffman_vbsse21_zd"):
            ents = []
            for name, s in (("good", good), ("no-code", bad), ("good-3000", good[:3000]), ("no-code-tail", bad[39990:40010])):
                ret, st = oracle.press(src, s)
                assert ret == 0
                ents.append(entry(oracle, src, dst, name, s, st, rng))
            assert [e.want is None for e in ents] == [False, True, False, True]
            Run(lib, src, dst, ents, rng).check(oracle)
    finally:
        oracle.load_table()
        press.use_table()
        _want.clear()


# ------------------------------------------------------------------ 5: the two calls

@gpu
@pytest.mark.parametrize("src", FUSED_SRC)
def test_agrees_with_the_two_calls(lib, oracle, src):
    """one 64-read batch per fused pair: press_hip_recode_batch == press_hip_depress_batch + press_hip_press_batch in
    every output array (the arena, out_len, out_n, the samples)"""
    import torch
    ns, first = synth.read_lengths(7, 400, 64)
    reads = [synth.synth_read(7, 400 + k, min(int(ns[k]), 50000), int(first[k])) for k in range(64)]
    streams = []
    for s in reads:
        ret, st = oracle.press(src, s)
        assert ret == 0
        streams.append(st)
    rng = np.random.default_rng(64 + press.METHODS[src])
    inb, in_off, in_len = L.scatter_streams(rng, streams)
    rooms = np.array([len(s) for s in reads], dtype=np.uint32)
    off, total = L.scatter_rooms(rng, rooms)
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else a.view(dt)).copy()).cuda()
    d_in, d_io, d_il, d_n, d_off = t(inb), t(in_off, np.int64), t(in_len, np.int64), t(rooms, np.int32), t(off, np.int64)
    sid = press.METHODS[src]
    for dst in FUSED_DST:
        did = press.METHODS[dst]
        out_off = L.slots(rng, [L.slot_of(oracle.bound, dst, len(s)) for s in reads])
        d_oo = t(out_off, np.int64)
        nb = int(out_off[-1]) + 4096
        res = []
        for fused in (False, True):
            d_out = torch.full((nb,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
            d_len = torch.zeros(64, dtype=torch.int64, device="cuda")
            d_outn = torch.zeros(64, dtype=torch.int32, device="cuda")
            d_sig = torch.full((total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
            if fused:
                rc = lib.press_hip_recode_batch(sid, did, _p(d_in), _p(d_io), _p(d_il), _p(d_n), _p(d_off), 64, total,
                                                _p(d_out), _p(d_oo), _p(d_len), _p(d_sig), _p(d_outn), 1)
            else:
                rc = lib.press_hip_depress_batch(sid, _p(d_in), _p(d_io), _p(d_il), 64, _p(d_sig), _p(d_off), _p(d_n),
                                                 total, _p(d_outn), 1)
                assert rc == 0, press.last_error()
                rc = lib.press_hip_press_batch(did, _p(d_sig), _p(d_off), _p(d_outn), 64, total, _p(d_out), _p(d_oo),
                                               _p(d_len), 1)
            assert rc == 0, (src, dst, press.last_error())
            torch.cuda.synchronize()
            res.append((d_out.cpu().numpy(), d_len.cpu().numpy(), d_outn.cpu().numpy(), d_sig.cpu().numpy()))
        for x, y, what in zip(res[0], res[1], ("arena", "out_len", "out_n", "sig")):
            assert np.array_equal(x, y), (src, dst, what)
        assert np.array_equal(res[1][2].view(np.uint32), rooms)


# ------------------------------------------------------------------ 6: pass A is not launched

@gpu
def test_fused_pairs_skip_pass_a(lib, oracle):
    """the library counts its launches of k_ex_scan_chunked<false, ..>: none in a fused recode, one in a recode whose
    source is no svb-zd stream and one in a plain press"""
    s = _walk(np.random.default_rng(6), 50000, 0.01)
    for dst in ("vbe21_zd", "shuffman_vbe21_zd", "rc_vbe21_zd"):
        for src in FUSED_SRC:
            st = oracle.press(src, s)[1]
            before = press.pass_a_launches()
            got = press.recode_batch_host(src, dst, [st], [len(s)])
            assert press.pass_a_launches() == before, (src, dst)
            assert got[0] == oracle.press(dst, s)[1]
        st = oracle.press("vbbe21_zd", s)[1]
        before = press.pass_a_launches()
        got = press.recode_batch_host("vbbe21_zd", dst, [st], [len(s)])
        assert press.pass_a_launches() == before + 1, dst
        assert got[0] == oracle.press(dst, s)[1]
        before = press.pass_a_launches()
        press.press_batch_host(dst, [s])
        assert press.pass_a_launches() == before + 1, dst
