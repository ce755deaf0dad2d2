"""The batch API on the layouts its header allows (include/press_hip.h, press_hip_press_batch /
press_hip_depress_batch), not only on the packed layouts of press.py's helpers:

* A: the read battery of _layouts.py, every method: reads scattered through `sig` in a random order between
  noise, slots of any byte size from an odd offset, an empty guard read behind every read, streams at odd
  offsets, rooms larger than the reads - device resident, host pageable (staged and direct), host pinned,
  and the symbol counter.  Every read as the oracle has it; nothing written outside a read's slot or room.
* C: arena offsets of 2^32 bytes and more, sample offsets of 2^31 and more.
* D: the argument checks of the host path, the overlap checks included.
* The empty read of slow5 svb-zd (the u32 count alone) in both directions.

The ABI is called through ctypes where press.py's wrappers cannot express a layout.
"""
import ctypes

import numpy as np
import pytest

import _layouts as L
import _libs
from honours_amd import press

gpu = pytest.mark.gpu
METHODS = sorted(press.METHODS, key=lambda m: press.METHODS[m])
EARG = -2
VRAM_LIMIT = 10 * 10 ** 9


# ------------------------------------------------------------------ the battery's power (CPU, oracle only)

def test_battery_keeps_its_power(oracle):
    """On the battery, at the A1 capacities: every method presses at least 24 of the 29 reads; what the oracle
    refuses is the 3 empty reads (exception, Huffman, ex-zd and range-coder methods; the ex-zd ones may refuse
    2 more); at most 2 reads per method are left out of the sample comparison, and those only as header-only
    static-Huffman streams (n = 1, every delta an exception); the range coders store 5 to 8 reads raw, which
    are compared with the oracle's decoder."""
    v = L.battery_verdicts(oracle, oracle.bound)
    empties = ["empty-first", "empty-middle", "empty-last"]
    for m, d in v.items():
        print(m, "refused", d["refused"], "left out", d["skipped"], "raw", len(d["raw"]), "lossless", d["lossless"])
        assert 29 - len(d["refused"]) >= 24, m
        if m in L.EX_FAMILY or m in L.HASGAM:
            assert set(empties) <= set(d["refused"]), m
            assert len(d["refused"]) <= 3 + (2 if m in L.HASGAM else 0), m
        else:
            assert d["refused"] == [], m
        assert len(d["skipped"]) <= 2, m
        if m.startswith("shuffman"):
            assert d["skipped"] == ["walk-1", "all-exceptions-3000"], m
        else:
            assert d["skipped"] == [], m
        if m in _libs.RC_FAMILY:
            assert 5 <= len(d["raw"]) <= 8, m
        assert d["lossless"] + len(d["raw"]) + len(d["skipped"]) + len(d["refused"]) == 29, m


# ------------------------------------------------------------------ GPU plumbing

@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.load_table()
    press.use_torch_stream()
    lb.press_hip_symbol_counts.restype = ctypes.c_int
    lb.press_hip_symbol_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                           ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]
    lb.press_hip_host_alloc.restype = ctypes.c_void_p
    lb.press_hip_host_alloc.argtypes = [ctypes.c_uint64]
    lb.press_hip_host_free.argtypes = [ctypes.c_void_p]
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _p(x):
    """pointer of a numpy array or a torch tensor"""
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def press_call(lib, m, sig, off, n, total, out, out_off, out_len, dev):
    return lib.press_hip_press_batch(press.METHODS[m] if isinstance(m, str) else m, _p(sig), _p(off), _p(n),
                                     len(n), total, _p(out), _p(out_off), _p(out_len), 1 if dev else 0)


def depress_call(lib, m, arena, in_off, in_len, sig, off, n, total, out_n, dev):
    return lib.press_hip_depress_batch(press.METHODS[m] if isinstance(m, str) else m, _p(arena), _p(in_off),
                                       _p(in_len), len(n), _p(sig), _p(off), _p(n), total, _p(out_n),
                                       1 if dev else 0)


def _t(torch, a, dtype=None):
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


class Plan:
    """The A layout of one method: the battery with a guard behind every read, the expected streams and
    the slots"""

    def __init__(self, lib, oracle, m, seed):
        self.m = m
        self.rng = np.random.default_rng(seed * 100 + press.METHODS[m])
        self.reads = [s for _, s in L.battery()]
        self.names = [nm for nm, _ in L.battery()]
        self.sig, roff = L.scatter_reads(self.rng, self.reads)
        self.ns, self.off = L.with_guards(self.reads, roff)
        self.total = self.sig.size
        self.samples = []
        self.want = []   # per entry: expected stream (zstd: its content) or None
        sizes = []
        bound = lambda mm, n: int(lib.press_hip_bound(press.METHODS[mm], n))
        empty = np.zeros(0, dtype=np.int16)
        guard = L.expect_press(oracle, m, empty, 1 << 20)
        gslot = 64 if m in L.ZSTD_KINDS else (len(guard) if guard is not None else 0) + 16
        for s in self.reads:
            cap = L.slot_of(bound, m, len(s)) + int(self.rng.integers(0, 16))
            self.samples += [s, empty]
            self.want += [L.expect_press(oracle, m, s, cap), guard]
            sizes += [cap, gslot]
        self.sizes = sizes
        self.out_off = L.slots(self.rng, sizes)
        self.arena_bytes = int(self.out_off[-1]) + 4096

    def check_streams(self, oracle, arena, lens):
        """streams as the oracle's, guard slots and the arena around the slots untouched -> the streams"""
        m = self.m
        out = []
        for k, (s, w) in enumerate(zip(self.samples, self.want)):
            o0, o1 = int(self.out_off[k]), int(self.out_off[k + 1])
            ln = int(lens[k])
            tag = (m, k, len(s), self.names[k // 2] + ("" if k % 2 == 0 else " guard"))
            if w is None:
                assert ln == L.FAILED64, tag
                out.append(b"")
                if k % 2:
                    assert (arena[o0:o1] == L.ARENA_FILL).all(), tag
                continue
            assert ln != L.FAILED64 and ln <= o1 - o0, tag + (press.last_error(),)
            st = arena[o0:o0 + ln].tobytes()
            if m in L.ZSTD_KINDS:
                L.check_zstd_frame(oracle, m, s, st, w)
            else:
                assert st == w, tag + (len(st), len(w))
            if k % 2:
                assert (arena[o0 + ln:o1] == L.ARENA_FILL).all(), tag
            out.append(st)
        return out

    def rooms(self):
        extra = 0 if self.m in L.SVB_KINDS else 21
        return np.array([int(n) + int(self.rng.integers(0, extra)) if extra else int(n) for n in self.ns],
                        dtype=np.uint32)

    def expect_back(self, oracle, streams, rooms):
        return [L.expect_depress(oracle, self.m, s, st, int(r)) for s, st, r in zip(self.samples, streams, rooms)]


def check_back(m, back, off, rooms, out_n, expect, total, device):
    """the decoded reads as expected; no sample written outside [off, off + roundup8(room)) (device resident)
    or [off, off + out_n) (host buffers)"""
    for k, (verdict, want) in enumerate(expect):
        tag = (m, k, int(rooms[k]))
        if verdict == "skip":
            continue
        if verdict == "fail":
            assert int(out_n[k]) == L.FAILED32, tag
            continue
        assert int(out_n[k]) == len(want), tag + (int(out_n[k]), len(want))
        assert np.array_equal(back[int(off[k]):int(off[k]) + len(want)], want), tag
    if device:
        spans = [L.roundup8(r) for r in rooms]
    else:
        spans = [0 if int(x) == L.FAILED32 else int(x) for x in out_n]
    bad = np.nonzero(back[:total][L.outside_rooms(total, off, spans)] != np.int16(L.SIG_FILL))[0]
    assert bad.size == 0, (m, "samples written outside the rooms", bad[:8])


# ------------------------------------------------------------------ A1: device resident

@gpu
@pytest.mark.parametrize("m", METHODS)
def test_a1_device_resident(lib, oracle, m):
    import torch

    pl = Plan(lib, oracle, m, 1)
    d_sig = _t(torch, pl.sig)
    d_off = _t(torch, pl.off, np.int64)
    d_n = _t(torch, pl.ns, np.int32)
    d_out = torch.full((pl.arena_bytes,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
    d_out_off = _t(torch, pl.out_off, np.int64)
    d_len = torch.zeros(len(pl.ns), dtype=torch.int64, device="cuda")
    assert press_call(lib, m, d_sig, d_off, d_n, pl.total, d_out, d_out_off, d_len, True) == 0, press.last_error()
    torch.cuda.synchronize()
    arena = d_out.cpu().numpy()
    lens = d_len.cpu().numpy().view(np.uint64)
    streams = pl.check_streams(oracle, arena, lens)
    assert (arena[:int(pl.out_off[0])] == L.ARENA_FILL).all() and (arena[int(pl.out_off[-1]):] == L.ARENA_FILL).all()

    rooms = pl.rooms()
    expect = pl.expect_back(oracle, streams, rooms)
    inb, in_off, in_len = L.scatter_streams(pl.rng, streams)
    off, total = L.scatter_rooms(pl.rng, rooms)
    d_back = torch.full((total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    d_outn = torch.zeros(len(rooms), dtype=torch.int32, device="cuda")
    assert depress_call(lib, m, _t(torch, inb), _t(torch, in_off, np.int64), _t(torch, in_len, np.int64), d_back,
                        _t(torch, off, np.int64), _t(torch, rooms, np.int32), total, d_outn, True) == 0, press.last_error()
    torch.cuda.synchronize()
    check_back(m, d_back.cpu().numpy(), off, rooms, d_outn.cpu().numpy().view(np.uint32), expect, total, device=True)


# ------------------------------------------------------------------ A2 / A3: host buffers

def _host_round(lib, oracle, m, groups, pinned=None):
    pl = Plan(lib, oracle, m, 2 if pinned is None else 3)
    out = np.full(pl.arena_bytes, L.ARENA_FILL, dtype=np.uint8)
    lens = np.zeros(len(pl.ns), dtype=np.uint64)
    sig = pl.sig if pinned is None else pinned(pl.sig)
    for g0 in range(0, len(pl.ns), groups):
        g1 = min(g0 + groups, len(pl.ns))
        oo = np.ascontiguousarray(pl.out_off[g0:g1 + 1])
        ln = np.zeros(g1 - g0, dtype=np.uint64)
        assert press_call(lib, m, sig, np.ascontiguousarray(pl.off[g0:g1]), np.ascontiguousarray(pl.ns[g0:g1]),
                          pl.total, out, oo, ln, False) == 0, press.last_error()
        lens[g0:g1] = ln
    streams = pl.check_streams(oracle, out, lens)
    assert (out[:int(pl.out_off[0])] == L.ARENA_FILL).all() and (out[int(pl.out_off[-1]):] == L.ARENA_FILL).all()

    rooms = pl.rooms()
    expect = pl.expect_back(oracle, streams, rooms)
    inb, in_off, in_len = L.scatter_streams(pl.rng, streams)
    off, total = L.scatter_rooms(pl.rng, rooms, min_gap=64 if pinned is not None else 0)
    back = np.full(total, L.SIG_FILL, dtype=np.int16) if pinned is None else \
        pinned(np.full(total, L.SIG_FILL, dtype=np.int16))
    out_n = np.zeros(len(rooms), dtype=np.uint32)
    for g0 in range(0, len(rooms), groups):
        g1 = min(g0 + groups, len(rooms))
        on = np.zeros(g1 - g0, dtype=np.uint32)
        assert depress_call(lib, m, inb, np.ascontiguousarray(in_off[g0:g1]), np.ascontiguousarray(in_len[g0:g1]),
                            back, np.ascontiguousarray(off[g0:g1]), np.ascontiguousarray(rooms[g0:g1]), total, on,
                            False) == 0, press.last_error()
        out_n[g0:g1] = on
    check_back(m, back, off, rooms, out_n, expect, total, device=False)


@gpu
@pytest.mark.parametrize("m", METHODS)
def test_a2_host_pageable(lib, oracle, m):
    """one batch of 58 reads (the staged path), then the same layout in calls of at most 4 reads (the direct
    copies): only [off, off + out_n) of a read is written"""
    _host_round(lib, oracle, m, 1 << 20)
    _host_round(lib, oracle, m, 4)


@gpu
@pytest.mark.parametrize("m", ["svb12_zd", "vbsse21_zd", "shuffman_vbe21_zd", "zstd_svb_zd"])
def test_a3_host_pinned(lib, oracle, m):
    """press_hip_host_alloc buffers: sig by one DMA, the samples straight into the caller's buffer - gaps of
    64 samples and more between the rooms stay untouched (the overwrite covers gaps under 128 bytes only)"""
    held = []

    def pinned(a):
        p = lib.press_hip_host_alloc(a.nbytes)
        assert p
        held.append(p)
        v = np.frombuffer((ctypes.c_uint8 * a.nbytes).from_address(p), dtype=a.dtype)
        v[:] = a
        return v
    try:
        _host_round(lib, oracle, m, 1 << 20, pinned)
    finally:
        for p in held:
            lib.press_hip_host_free(p)


# ------------------------------------------------------------------ A4: symbol counts

def zd_counts(reads):
    c = np.zeros(press.NBINS, dtype=np.uint64)
    for s in reads:
        if len(s) < 2:
            continue
        d = (s[1:].astype(np.int32) - s[:-1].astype(np.int32)).astype(np.int16).astype(np.int32)
        z = ((d << 1) ^ (d >> 15)) & 0xFFFF
        c[:256] += np.bincount(z[z <= 255], minlength=256).astype(np.uint64)
        c[256] += np.uint64(int((z > 255).sum()))
    return c


@gpu
def test_a4_symbol_counts(lib):
    """the A1 layout (noise between the reads, guards) plus one read listed twice at the same offset: counting
    only reads, so it is counted twice"""
    import torch

    rng = np.random.default_rng(44)
    reads = [s for _, s in L.battery()]
    sig, roff = L.scatter_reads(rng, reads)
    ns, off = L.with_guards(reads, roff)
    ns = np.append(ns, ns[2 * 20])
    off = np.append(off, off[2 * 20])
    want = zd_counts(reads + [reads[20]])
    d_counts = torch.zeros(press.NBINS, dtype=torch.int64, device="cuda")
    assert lib.press_hip_symbol_counts(_p(_t(torch, sig)), _p(_t(torch, off, np.int64)), _p(_t(torch, ns, np.int32)),
                                       len(ns), sig.size, _p(d_counts), 1) == 0, press.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint64), want)
    host = np.zeros(press.NBINS, dtype=np.uint64)
    assert lib.press_hip_symbol_counts(_p(sig), _p(off), _p(ns), len(ns), sig.size, _p(host), 0) == 0
    assert np.array_equal(host, want)


# ------------------------------------------------------------------ the empty slow5 svb-zd read (fix 1)

@gpu
@pytest.mark.parametrize("dev", [True, False])
def test_empty_slow5_read(lib, oracle, dev):
    """slow5lib's stream of an empty signal is its u32 count (slow5_press.c:1046), as the oracle and the drop-in
    symbol have it: press writes 00 00 00 00, or fails in a slot under 4 bytes; depress takes exactly that
    stream and refuses any other for n = 0"""
    import torch

    cvt = (lambda a, dt=None: _t(torch, a, dt)) if dev else (lambda a, dt=None: np.ascontiguousarray(a))
    ret, want = oracle.press("slow5_svb_zd", np.zeros(0, dtype=np.int16), cap=64)
    assert ret == 0 and want == b"\0\0\0\0"
    sig = np.zeros(64, dtype=np.int16)
    ns = np.zeros(3, dtype=np.uint32)
    off = np.array([0, 8, 16], dtype=np.uint64)
    out_off = np.array([3, 7, 10, 30], dtype=np.uint64)      # slots of 4, 3 and 20 bytes
    out = np.full(64, L.ARENA_FILL, dtype=np.uint8)
    lens = np.zeros(3, dtype=np.uint64)
    o, ln = cvt(out), cvt(lens, np.int64)
    assert press_call(lib, "slow5_svb_zd", cvt(sig), cvt(off, np.int64), cvt(ns, np.int32), 64, o,
                      cvt(out_off, np.int64), ln, dev) == 0, press.last_error()
    if dev:
        torch.cuda.synchronize()
        o, ln = o.cpu().numpy(), ln.cpu().numpy().view(np.uint64)
    assert list(ln) == [4, L.FAILED64, 4]
    assert o[3:7].tobytes() == want and o[10:14].tobytes() == want
    assert (o[:3] == L.ARENA_FILL).all() and (o[7:10] == L.ARENA_FILL).all() and (o[14:] == L.ARENA_FILL).all()

    streams = [b"\0\0\0\0", b"", b"\0\0\0\0\0", b"\1\0\0\0", b"\0\0\0"]
    for st in streams:
        r, _ = oracle.depress("slow5_svb_zd", st, 0)
        assert (r == 0) == (st == want), st
    inb, in_off, in_len = L.scatter_streams(np.random.default_rng(5), streams)
    k = len(streams)
    back = np.full(64, L.SIG_FILL, dtype=np.int16)
    out_n = np.zeros(k, dtype=np.uint32)
    b, on = cvt(back), cvt(out_n, np.int32)
    assert depress_call(lib, "slow5_svb_zd", cvt(inb), cvt(in_off, np.int64), cvt(in_len, np.int64), b,
                        cvt(np.arange(k, dtype=np.uint64) * 8, np.int64), cvt(np.zeros(k, dtype=np.uint32), np.int32),
                        64, on, dev) == 0, press.last_error()
    if dev:
        torch.cuda.synchronize()
        b, on = b.cpu().numpy(), on.cpu().numpy().view(np.uint32)
    assert list(on) == [0] + [L.FAILED32] * (k - 1)
    assert (b == np.int16(L.SIG_FILL)).all()


# ------------------------------------------------------------------ D: argument checks

def _fresh():
    sig = np.arange(256, dtype=np.int16)
    out = np.full(4096, L.ARENA_FILL, dtype=np.uint8)
    lens = np.full(8, 7, dtype=np.uint64)
    back = np.full(256, L.SIG_FILL, dtype=np.int16)
    out_n = np.full(8, 7, dtype=np.uint32)
    counts = np.full(press.NBINS, 3, dtype=np.uint64)
    return sig, out, lens, back, out_n, counts


def _untouched(out, lens, back, out_n, counts):
    assert (out == L.ARENA_FILL).all() and (lens == 7).all()
    assert (back == np.int16(L.SIG_FILL)).all() and (out_n == 7).all() and (counts == 3).all()


def _earg(rc, why):
    assert rc == EARG, (rc, why)
    assert why in press.last_error(), (press.last_error(), why)


@gpu
def test_d_argument_checks(lib):
    """each bad layout is refused with PRESS_HIP_EARG and a message before anything is written (host pointers;
    the device-resident sig alignment with device pointers).  Nothing overlapping reaches a kernel."""
    import torch

    m = "vbe21_zd"
    ok_n = np.array([16, 16], dtype=np.uint32)
    ok_off = np.array([0, 32], dtype=np.uint64)
    out_off = np.array([0, 1024, 2048], dtype=np.uint64)
    in_off = np.array([0, 16], dtype=np.uint64)
    in_len = np.array([16, 16], dtype=np.uint64)
    cases = [  # (off, n, out_off, what the message says, also for depress and the counter)
        (np.array([0, 36], dtype=np.uint64), ok_n, out_off, "multiple of 8", True),
        (ok_off, np.array([16, 225], dtype=np.uint32), out_off, "beyond total_samples", True),
        (ok_off, ok_n, np.array([0, 1024, 1000], dtype=np.uint64), "non-decreasing", False),
        (np.array([0, 8], dtype=np.uint64), ok_n, out_off, "overlaps", False),     # sample ranges (fix 2)
        (np.array([32, 24], dtype=np.uint64), ok_n, out_off, "overlaps", False),   # ... out of order
    ]
    for off, n, oo, why, all3 in cases:
        sig, out, lens, back, out_n, counts = _fresh()
        _earg(press_call(lib, m, sig, off, n, 256, out, oo, lens, False), why)
        _untouched(out, lens, back, out_n, counts)
        if all3:
            _earg(depress_call(lib, m, out, in_off, in_len, back, off, n, 256, out_n, False), why)
            _earg(lib.press_hip_symbol_counts(_p(sig), _p(off), _p(n), 2, 256, _p(counts), 0), why)
            _untouched(out, lens, back, out_n, counts)

    # depress: rooms [off, off + n) that overlap, with 2 reads and with 6 (the staged path's size)
    for off, n in ((np.array([0, 8], dtype=np.uint64), np.array([9, 4], dtype=np.uint32)),
                   (np.array([0, 32, 64, 96, 128, 40], dtype=np.uint64), np.array([8, 8, 8, 8, 8, 30], dtype=np.uint32))):
        sig, out, lens, back, out_n, counts = _fresh()
        io = np.arange(len(n), dtype=np.uint64) * 16
        il = np.full(len(n), 16, dtype=np.uint64)
        _earg(depress_call(lib, m, out, io, il, back, off, n, 256, out_n[:len(n)], False), "overlaps")
        _untouched(out, lens, back, out_n, counts)

    # a method number one past the last
    sig, out, lens, back, out_n, counts = _fresh()
    nm = press.METHODS["rccm_vbbe21_zd"] + 1
    _earg(press_call(lib, nm, sig, ok_off, ok_n, 256, out, out_off, lens[:2], False), "not available")
    _earg(depress_call(lib, nm, out, in_off, in_len, back, ok_off, ok_n, 256, out_n[:2], False), "not available")
    _untouched(out, lens, back, out_n, counts)

    # a device-resident sig that is not 16-byte aligned
    d_sig = torch.zeros(512, dtype=torch.int16, device="cuda")
    d_out = torch.full((4096,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    d_outn = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    d_counts = torch.full((press.NBINS,), 3, dtype=torch.int64, device="cuda")
    d_off, d_n = _t(torch, ok_off, np.int64), _t(torch, ok_n, np.int32)
    _earg(press_call(lib, m, d_sig[1:], d_off, d_n, 256, d_out, _t(torch, out_off, np.int64), d_len, True), "aligned")
    _earg(depress_call(lib, m, d_out, _t(torch, in_off, np.int64), _t(torch, in_len, np.int64), d_sig[1:], d_off, d_n,
                       256, d_outn, True), "aligned")
    _earg(lib.press_hip_symbol_counts(_p(d_sig[1:]), _p(d_off), _p(d_n), 2, 256, _p(d_counts), 1), "aligned")
    torch.cuda.synchronize()
    assert (d_out == L.ARENA_FILL).all() and (d_len == 7).all() and (d_outn == 7).all() and (d_counts == 3).all()

    # nreads = 0: nothing to do, nothing written
    sig, out, lens, back, out_n, counts = _fresh()
    assert lib.press_hip_press_batch(press.METHODS[m], _p(sig), _p(ok_off), _p(ok_n), 0, 256, _p(out), _p(out_off),
                                     _p(lens), 0) == 0
    assert lib.press_hip_depress_batch(press.METHODS[m], _p(out), _p(in_off), _p(in_len), 0, _p(back), _p(ok_off),
                                       _p(ok_n), 256, _p(out_n), 0) == 0
    assert lib.press_hip_symbol_counts(_p(sig), _p(ok_off), _p(ok_n), 0, 256, _p(counts), 0) == 0
    _untouched(out, lens, back, out_n, counts)


# ------------------------------------------------------------------ B: slots at the limit

def svb_worst(m, n):
    """the svb kinds' up-front worst case (press_svb.hip k_chunk_prep): count + keys + 2 bytes a value
    (slow5: 3, a 32-bit delta may take 17 bits)"""
    hdr = 4 if m == "slow5_svb_zd" else 0
    klen = (n + 3) // 4 if m in ("svb_zd", "slow5_svb_zd") else (n + 7) // 8
    return hdr + klen + (3 if hdr else 2) * n


def _b_batch(lib, torch, m, pl, sizes):
    out_off = L.slots(pl.rng, sizes)
    d_out = torch.full((int(out_off[-1]) + 4096,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(len(sizes), dtype=torch.int64, device="cuda")
    assert press_call(lib, m, _t(torch, pl.sig), _t(torch, pl.off, np.int64), _t(torch, pl.ns, np.int32), pl.total,
                      d_out, _t(torch, out_off, np.int64), d_len, True) == 0, press.last_error()
    torch.cuda.synchronize()
    return out_off, d_out.cpu().numpy(), d_len.cpu().numpy().view(np.uint64)


@gpu
@pytest.mark.parametrize("m", METHODS)
def test_b_smallest_slots(lib, oracle, m):
    """every read in the smallest slot its method takes (include/press_hip.h, out_off): the svb kinds' worst case,
    the stream's own length for the others (zstd kinds: the frame's), adjacent and unaligned, a guard behind each
    -> the oracle's bytes; then every other read one byte short -> it fails, its neighbours and the guards do not
    change"""
    import torch

    pl = Plan(lib, oracle, m, 4)
    big = [int(x) for x in pl.sizes]
    _, arena, lens = _b_batch(lib, torch, m, pl, big)
    need = []
    for k, s in enumerate(pl.samples):
        if k % 2:
            need.append(big[k])  # guards keep their A1 slot: 16 (zstd: 64) bytes of canary
        elif m in L.SVB_KINDS:
            need.append(svb_worst(m, len(s)))
        elif pl.want[k] is None:
            need.append(0)
        elif m in L.ZSTD_KINDS:
            need.append(int(lens[k]))  # the device's frame (its bytes are not pinned)
        else:
            need.append(len(pl.want[k]))
    for short in (False, True):
        sizes = list(need)
        cut = set()
        if short:
            for k in range(0, len(sizes), 4):  # every other real read
                if sizes[k] > 0:
                    sizes[k] -= 1
                    cut.add(k)
        out_off, arena, lens = _b_batch(lib, torch, m, pl, sizes)
        assert (arena[:int(out_off[0])] == L.ARENA_FILL).all() and (arena[int(out_off[-1]):] == L.ARENA_FILL).all()
        for k, (s, w) in enumerate(zip(pl.samples, pl.want)):
            o0, o1 = int(out_off[k]), int(out_off[k + 1])
            ln = int(lens[k])
            tag = (m, short, k, len(s), sizes[k])
            if k in cut or w is None:
                assert ln == L.FAILED64, tag
                if k % 2:
                    assert (arena[o0:o1] == L.ARENA_FILL).all(), tag
                continue
            assert ln != L.FAILED64 and ln <= o1 - o0, tag + (press.last_error(),)
            st = arena[o0:o0 + ln].tobytes()
            if m in L.ZSTD_KINDS:
                L.check_zstd_frame(oracle, m, s, st, w)
            else:
                assert st == w, tag
            if k % 2:
                assert (arena[o0 + ln:o1] == L.ARENA_FILL).all(), tag


# ------------------------------------------------------------------ C: offsets past 32 bits

def _vram_check(lib, m, total, nreads, tensor_bytes):
    ws = int(lib.press_hip_workspace_bytes(press.METHODS[m], total, nreads))
    assert ws + tensor_bytes < VRAM_LIMIT, (m, ws, tensor_bytes)


@pytest.fixture
def vram():
    """frees the C tests' multi-GB tensors before the next test, also after a failure (whose traceback would
    keep the test's frame, and with it its tensors, alive)"""
    import gc
    import sys
    import traceback

    import torch
    yield
    tb = getattr(sys, "last_traceback", None)
    if tb is not None:
        traceback.clear_frames(tb)
    gc.collect()
    torch.cuda.empty_cache()


def _all_fill(d_out, b0, b1, piece=1 << 28):
    """d_out[b0:b1] is all ARENA_FILL, compared in pieces (a mask of the whole arena would double its size)"""
    return all(bool((d_out[p:min(p + piece, b1)] == L.ARENA_FILL).all()) for p in range(b0, b1, piece))


C1_READS = [23, 16, 18, 2, 19, 21, 9, 17]   # battery indices: the 150 000-sample read (synth-1) first


@gpu
@pytest.mark.parametrize("m", METHODS)
def test_c1_arena_past_4gib(lib, oracle, m, vram):
    """one output arena of 2^32 + 2^22 bytes: a 150 000-sample read whose slot starts about 10 KB below 2^32
    (its payload and, for the Huffman methods, its units on both sides of the line), seven more wholly beyond
    it, a guard behind each; then depress from the same arena"""
    import torch

    bat = L.battery()
    reads = [bat[i][1] for i in C1_READS]
    assert len(reads[0]) == 150000
    rng = np.random.default_rng(70 + press.METHODS[m])
    sig, roff = L.scatter_reads(rng, reads)
    ns, off = L.with_guards(reads, roff)
    bound = lambda mm, n: int(lib.press_hip_bound(press.METHODS[mm], n))
    empty = np.zeros(0, dtype=np.int16)
    guard = L.expect_press(oracle, m, empty, 1 << 20)
    gslot = 64 if m in L.ZSTD_KINDS else (len(guard) if guard is not None else 0) + 16
    sizes, want, samples = [], [], []
    for s in reads:
        cap = L.slot_of(bound, m, len(s)) + int(rng.integers(0, 16))
        sizes += [cap, gslot]
        want += [L.expect_press(oracle, m, s, cap), guard]
        samples += [s, empty]
    out_off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    out_off[0] = (1 << 32) - 10001
    out_off[1:] = out_off[0] + np.cumsum(np.asarray(sizes, dtype=np.uint64))
    arena_bytes = (1 << 32) + (1 << 22)
    assert int(out_off[-1]) + 64 <= arena_bytes
    _vram_check(lib, m, sig.size, len(ns), arena_bytes + (1 << 28) + 4 * sig.nbytes)
    d_out = torch.full((arena_bytes,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
    d_off, d_n = _t(torch, off, np.int64), _t(torch, ns, np.int32)
    d_out_off = _t(torch, out_off, np.int64)
    d_len = torch.zeros(len(ns), dtype=torch.int64, device="cuda")
    assert press_call(lib, m, _t(torch, sig), d_off, d_n, sig.size, d_out, d_out_off, d_len, True) == 0, \
        press.last_error()
    torch.cuda.synchronize()
    a0, a1 = int(out_off[0]), int(out_off[-1])
    assert _all_fill(d_out, 0, a0) and _all_fill(d_out, a1, arena_bytes)
    used = d_out[a0:a1].cpu().numpy()
    lens = d_len.cpu().numpy().view(np.uint64)
    for k, (s, w) in enumerate(zip(samples, want)):
        o0, o1 = int(out_off[k]) - a0, int(out_off[k + 1]) - a0
        ln = int(lens[k])
        if w is None:
            assert ln == L.FAILED64, (m, k)
            if k % 2:
                assert (used[o0:o1] == L.ARENA_FILL).all(), (m, k)
            continue
        assert ln != L.FAILED64 and ln <= o1 - o0, (m, k)
        st = used[o0:o0 + ln].tobytes()
        if m in L.ZSTD_KINDS:
            L.check_zstd_frame(oracle, m, s, st, w)
        else:
            assert st == w, (m, k, len(st), len(w))
        if k % 2:
            assert (used[o0 + ln:o1] == L.ARENA_FILL).all(), (m, k)
    assert int(out_off[0]) + int(lens[0]) > (1 << 32), "the first stream does not cross 2^32"

    # depress straight from the arena: in_off across and beyond 2^32
    ok = np.array([int(x) != L.FAILED64 for x in lens])
    in_len = np.where(ok, lens, 0).astype(np.uint64)
    d_back = torch.full((sig.size,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    d_outn = torch.zeros(len(ns), dtype=torch.int32, device="cuda")
    assert depress_call(lib, m, d_out, d_out_off[:-1].contiguous(), _t(torch, in_len, np.int64), d_back, d_off, d_n,
                        sig.size, d_outn, True) == 0, press.last_error()
    torch.cuda.synchronize()
    back = d_back.cpu().numpy()
    out_n = d_outn.cpu().numpy().view(np.uint32)
    del d_out, d_back
    torch.cuda.empty_cache()
    for k, s in enumerate(samples):
        st = used[int(out_off[k]) - a0:int(out_off[k]) - a0 + int(in_len[k])].tobytes()
        verdict, w = L.expect_depress(oracle, m, s, st, len(s))
        if verdict == "skip":
            continue
        if verdict == "fail":
            assert int(out_n[k]) == L.FAILED32, (m, k)
            continue
        assert int(out_n[k]) == len(w), (m, k, int(out_n[k]))
        assert np.array_equal(back[int(off[k]):int(off[k]) + len(w)], w), (m, k)


@gpu
@pytest.mark.parametrize("m", ["svb12", "svb12_zd", "svb_zd", "slow5_svb_zd"])
def test_c2_samples_past_2g(lib, oracle, m, vram):
    """a sig of 2^31 + 2^20 samples, reads below, across and beyond the 2^31-sample line (2^32 bytes): press
    against the oracle, depress into the same tensor, symbol counts against numpy.  The exception, Huffman and
    range-coder methods are left out on purpose: their scratch is 8 to 9 bytes per sample of extent
    (press_methods.hip make_plan), about 19 GB here."""
    import torch

    bat = L.battery()
    line = 1 << 31
    reads = [bat[23][1], bat[18][1], bat[26][1], bat[20][1], bat[9][1]]
    off = np.array([line - 160048, line - 10000, line + 10008, line + (1 << 19), line + (1 << 20) - 70000],
                   dtype=np.uint64)
    ns = np.array([len(r) for r in reads], dtype=np.uint32)
    total = line + (1 << 20)
    assert (off % 8 == 0).all() and all(int(o) + int(n) <= total for o, n in zip(off, ns))
    assert all(int(off[k]) + int(ns[k]) <= int(off[k + 1]) for k in range(len(ns) - 1))  # disjoint
    assert int(off[1]) < line < int(off[1]) + int(ns[1])
    _vram_check(lib, m, total, len(ns), total * 2 + (1 << 24))
    d_sig = torch.empty(total, dtype=torch.int16, device="cuda")
    for o, r in zip(off, reads):
        d_sig[int(o):int(o) + len(r)] = torch.from_numpy(r.copy()).cuda()
    bound = lambda mm, n: int(lib.press_hip_bound(press.METHODS[mm], n))
    sizes = [L.slot_of(bound, m, len(r)) for r in reads]
    out_off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    out_off[0] = 5
    out_off[1:] = 5 + np.cumsum(np.asarray(sizes, dtype=np.uint64))
    d_out = torch.full((int(out_off[-1]) + 64,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
    d_off, d_n = _t(torch, off, np.int64), _t(torch, ns, np.int32)
    d_out_off = _t(torch, out_off, np.int64)
    d_len = torch.zeros(len(ns), dtype=torch.int64, device="cuda")
    assert press_call(lib, m, d_sig, d_off, d_n, total, d_out, d_out_off, d_len, True) == 0, press.last_error()
    torch.cuda.synchronize()
    arena = d_out.cpu().numpy()
    lens = d_len.cpu().numpy().view(np.uint64)
    for k, r in enumerate(reads):
        ret, w = oracle.press(m, r, cap=sizes[k])
        assert ret == 0 and arena[int(out_off[k]):int(out_off[k]) + int(lens[k])].tobytes() == w, (m, k)

    d_counts = torch.zeros(press.NBINS, dtype=torch.int64, device="cuda")
    assert lib.press_hip_symbol_counts(_p(d_sig), _p(d_off), _p(d_n), len(ns), total, _p(d_counts), 1) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint64), zd_counts(reads))

    for o, r in zip(off, reads):
        d_sig[int(o):int(o) + len(r)] = 0
    d_outn = torch.zeros(len(ns), dtype=torch.int32, device="cuda")
    assert depress_call(lib, m, d_out, d_out_off[:-1].contiguous(), d_len, d_sig, d_off, d_n, total, d_outn,
                        True) == 0, press.last_error()
    torch.cuda.synchronize()
    assert list(d_outn.cpu().numpy()) == list(ns.astype(np.int32))
    for o, r in zip(off, reads):
        assert np.array_equal(d_sig[int(o):int(o) + len(r)].cpu().numpy(), r), (m, int(o))
    del d_sig, d_out
    torch.cuda.empty_cache()
