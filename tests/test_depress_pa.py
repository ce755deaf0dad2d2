"""press_hip_depress_pa_batch: compressed reads straight to picoampere floats (include/press_hip.h).

The floats are defined bit for bit: pa = ((float) s + cal0) * cal1 with the add and the multiply rounded one after the
other in IEEE single precision, s being what press_hip_depress_batch decodes.  numpy's float32 arithmetic is that
definition, so every comparison here is one of uint32 bit patterns.

CPU: press_hip_pa_cal against numpy, the fused predicate, the workspace size, the argument checks that come before any
device call.  GPU: the read battery of _layouts.py through all 19 methods on scattered rooms behind a canary, extreme
samples, agreement with the two-call route, refused reads, the host path (pageable and page-locked), the scratch a
fused method keeps, and a BLOW5 file end to end.

Tail of a room, as the header states it: a decoded read is written as [off, off + out_n) and nothing else, whatever the
method - the canary survives at [off + n, off + roundup8(n)).
"""
import ctypes
import json
import os

import numpy as np
import pytest

import _layouts as L
import _libs
from honours_amd import build, press

gpu = pytest.mark.gpu
METHODS = sorted(press.METHODS, key=lambda m: press.METHODS[m])
FUSED = L.SVB_KINDS
ZSTD_OVER_SVB = ("zstd_svb_zd", "zstd_svb12_zd")
EARG = -2
F32 = L.FAILED32
CANARY = 0x7FC12345  # a quiet NaN with a payload: no conversion produces it
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cal_of(dor):
    """the definition: (float) offset, (float) range / (float) digitisation -> float32 (nreads, 2)"""
    dor = np.asarray(dor, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([dor[:, 1].astype(np.float32), dor[:, 2].astype(np.float32) / dor[:, 0].astype(np.float32)], axis=1)


def pa_bits(s, c0, c1):
    """the definition of the floats, as uint32 bit patterns"""
    with np.errstate(all="ignore"):
        return ((np.asarray(s).astype(np.float32) + np.float32(c0)) * np.float32(c1)).view(np.uint32)


def batch_cal(nreads):
    """a calibration of its own for every read: units that are no power of two, offsets of both signs"""
    r = np.arange(nreads, dtype=np.float64)
    dor = np.stack([np.full(nreads, 8192.0), np.where(r % 2 == 0, 3 + 7 * r, -(3 + 7 * r)), 1400.0 * (1 + r / 64)], axis=1)
    return cal_of(dor)


# ------------------------------------------------------------------ CPU

@pytest.fixture(scope="module")
def cpu_lib():
    build.build()
    return press.load_library()


def test_pa_cal_against_numpy(cpu_lib):
    """a few hundred random triples and the edges (zeros, infinities, values beyond float32, denormals): bit for bit;
    where the definition gives a NaN, a NaN (its payload is the divider's, not the definition's)"""
    rng = np.random.default_rng(5)
    dor = np.stack([rng.choice([2048.0, 8192.0, 65536.0, 1000.0, 3.7], size=400) * rng.uniform(0.5, 2.0, size=400),
                    rng.uniform(-5000, 5000, size=400), rng.uniform(1, 5000, size=400)], axis=1)
    dor[:40, 1] = np.round(dor[:40, 1])
    edges = [(8192.0, 23.0, 1437.976), (2048.0, -1.0, 748.58), (0.0, 0.0, 0.0), (0.0, 1.0, 1.0), (1.0, np.inf, 1.0),
             (np.inf, 1.0, np.inf), (1e300, 1e300, 1e300), (1e-300, 1e-300, 1e-300), (1e-40, 1e-40, 1e-40),
             (-8192.0, -0.0, 1400.0), (3.0, 16777217.0, 1.0), (8192.0, 0.1, np.nextafter(1400.0, 2000.0))]
    dor = np.concatenate([dor, np.array(edges, dtype=np.float64)])
    want = cal_of(dor)
    got = press.pa_cal(dor)
    assert got.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert nan.sum() >= 2 and np.isinf(want).sum() >= 3
    # the raw call, and an empty batch
    raw = np.zeros(2 * len(dor), dtype=np.float32)
    assert cpu_lib.press_hip_pa_cal(dor.ctypes.data, len(dor), raw.ctypes.data) == 0
    assert np.array_equal(raw.view(np.uint32)[~nan.reshape(-1)], want.reshape(-1).view(np.uint32)[~nan.reshape(-1)])
    assert cpu_lib.press_hip_pa_cal(None, 0, None) == 0
    assert cpu_lib.press_hip_pa_cal(None, 3, raw.ctypes.data) == EARG


def test_fused_predicate(cpu_lib):
    for m, mid in press.METHODS.items():
        f = cpu_lib.press_hip_depress_pa_fused(mid)
        if m in FUSED:
            assert f == 1, m
        elif m in ZSTD_OVER_SVB:
            assert f in (0, 1), m
        else:
            assert f == 0, m
        assert press.depress_pa_fused(m) == bool(f)
    for bad in (-1, len(press.METHODS), 1000):
        assert cpu_lib.press_hip_depress_pa_fused(bad) == 0


def test_workspace_bytes(cpu_lib):
    t, nr = 1 << 20, 64
    for m, mid in press.METHODS.items():
        base = int(cpu_lib.press_hip_workspace_bytes(mid, t, nr))
        ws = int(cpu_lib.press_hip_depress_pa_workspace_bytes(mid, t, nr))
        assert ws >= base, m
        if cpu_lib.press_hip_depress_pa_fused(mid):
            assert ws - base < t, (m, ws - base)
        else:
            assert ws - base >= 2 * t, (m, ws - base)
    for bad in (-1, len(press.METHODS), 1000):
        assert cpu_lib.press_hip_depress_pa_workspace_bytes(bad, t, nr) == 0


def test_argument_checks_need_no_device(cpu_lib):
    """a bad id, a NULL cal and a NULL pa are PRESS_HIP_EARG before any device call: also where there is no device"""
    a = np.zeros(256, dtype=np.uint8)
    io = np.zeros(1, dtype=np.uint64)
    il = np.full(1, 16, dtype=np.uint64)
    pa = np.zeros(64, dtype=np.float32)
    n = np.full(1, 8, dtype=np.uint32)
    cal = np.ones(2, dtype=np.float32)
    on = np.full(1, 7, dtype=np.uint32)
    p = lambda x: x.ctypes.data
    mid = press.METHODS["slow5_svb_zd"]
    call = lambda mm, pp, cc: cpu_lib.press_hip_depress_pa_batch(mm, p(a), p(io), p(il), 1, pp, p(io), p(n), 64, cc, p(on), 0)
    for bad in (-1, len(press.METHODS)):
        assert call(bad, p(pa), p(cal)) == EARG
        assert "not available" in press.last_error()
    assert call(mid, p(pa), None) == EARG and "NULL" in press.last_error()
    assert call(mid, None, p(cal)) == EARG and "NULL" in press.last_error()
    assert on[0] == 7 and (pa == 0).all()


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
    lb.press_hip_scratch_buffers.restype = ctypes.c_uint32
    lb.press_hip_scratch_buffers.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _p(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


def pa_call(lib, m, arena, in_off, in_len, pa, off, n, total, cal, out_n, dev):
    return lib.press_hip_depress_pa_batch(press.METHODS[m], _p(arena), _p(in_off), _p(in_len), len(n), _p(pa), _p(off),
                                          _p(n), total, _p(cal), _p(out_n), 1 if dev else 0)


def i16_call(lib, m, arena, in_off, in_len, sig, off, n, total, out_n, dev):
    return lib.press_hip_depress_batch(press.METHODS[m], _p(arena), _p(in_off), _p(in_len), len(n), _p(sig), _p(off),
                                       _p(n), total, _p(out_n), 1 if dev else 0)


class Case:
    """reads of one method as streams, in scattered rooms, with what the oracle decodes of them"""

    def __init__(self, oracle, m, reads, seed, min_gap=0):
        self.m, self.reads = m, reads
        rng = np.random.default_rng(seed * 100 + press.METHODS[m])
        st, _ = press.press_packed_host(m, reads)
        self.streams = [b"" if x is None else x for x in st]
        extra = 0 if m in L.SVB_KINDS else 21
        self.rooms = np.array([len(s) + (int(rng.integers(0, extra)) if extra else 0) for s in reads], dtype=np.uint32)
        self.expect = [L.expect_depress(oracle, m, s, x, int(r)) for s, x, r in zip(reads, self.streams, self.rooms)]
        self.inb, self.in_off, self.in_len = L.scatter_streams(rng, self.streams)
        self.off, self.total = L.scatter_rooms(rng, self.rooms, min_gap=min_gap)
        self.cal = batch_cal(len(reads))

    def dev(self):
        return (_t(self.inb), _t(self.in_off, np.int64), _t(self.in_len, np.int64), _t(self.off, np.int64),
                _t(self.rooms, np.int32), _t(self.cal.reshape(-1)))

    def check(self, bits, out_n, device):
        """bits: the float arena as uint32.  out_n as the oracle's verdicts, every decoded read bit for bit, the canary
        everywhere outside [off, off + roundup8(room)) (device) or [off, off + out_n) (host), and behind the read's
        last float"""
        m = self.m
        for k, (verdict, want) in enumerate(self.expect):
            tag = (m, k, int(self.rooms[k]))
            if verdict == "skip":
                continue
            if verdict == "fail":
                assert int(out_n[k]) == F32, tag
                continue
            assert int(out_n[k]) == len(want), tag + (int(out_n[k]), len(want))
            o = int(self.off[k])
            got = bits[o:o + len(want)]
            exp = pa_bits(want, self.cal[k, 0], self.cal[k, 1])
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, tag + ("first mismatch at", int(bad[0]), hex(int(got[bad[0]])), hex(int(exp[bad[0]])))
            if device:
                assert (bits[o + len(want):o + L.roundup8(len(want))] == CANARY).all(), tag + ("tail of the room written",)
        if device:
            spans = [L.roundup8(r) for r in self.rooms]
        else:
            spans = [0 if int(x) == F32 else int(x) for x in out_n]
        bad = np.nonzero(bits[:self.total][L.outside_rooms(self.total, self.off, spans)] != CANARY)[0]
        assert bad.size == 0, (m, "floats written outside the rooms", bad[:8])


_cases = {}


def battery_case(oracle, m):
    if m not in _cases:
        _cases[m] = Case(oracle, m, [s for _, s in L.battery()], 7)
    return _cases[m]


def run_device(lib, c):
    import torch
    d_in, d_io, d_il, d_off, d_n, d_cal = c.dev()
    d_pa = torch.full((c.total,), CANARY, dtype=torch.int32, device="cuda")
    d_on = torch.full((len(c.rooms),), 7, dtype=torch.int32, device="cuda")
    assert pa_call(lib, c.m, d_in, d_io, d_il, d_pa, d_off, d_n, c.total, d_cal, d_on, True) == 0, press.last_error()
    torch.cuda.synchronize()
    return d_pa.cpu().numpy().view(np.uint32), d_on.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ 1: the battery, all methods, device resident

@gpu
@pytest.mark.parametrize("m", METHODS)
def test_battery_device_resident(lib, oracle, m):
    c = battery_case(oracle, m)
    left_out = [k for k, (v, _) in enumerate(c.expect) if v == "skip"]
    assert len(left_out) == (2 if m.startswith("shuffman") else 0), (m, left_out)  # as battery_verdicts reports
    bits, out_n = run_device(lib, c)
    c.check(bits, out_n, device=True)


# ------------------------------------------------------------------ 2: extreme samples, the fused methods

@gpu
@pytest.mark.parametrize("m", FUSED)
def test_extremes_fused(lib, oracle, m):
    """8200 samples each (a wave's quarter of 8192 and a ragged tail): -32768 / 32767 alternating, -32768 throughout,
    a slow ramp; calibrations that cancel to within an ulp, reach 2^16 and run over several binades"""
    i = np.arange(8200)
    reads = [np.where(i % 2 == 0, -32768, 32767).astype(np.int16), np.full(8200, -32768, dtype=np.int16),
             (i // 4 - 1000).astype(np.int16)]
    c = Case(oracle, m, reads, 11)
    c.cal = cal_of([(8192.0, 32767.5, 1400.0), (2048.0, 32768.001, 748.58), (4000.0, 1000.25, 1437.976)])
    assert all(v == "ok" and np.array_equal(w, s) for (v, w), s in zip(c.expect, reads))
    for k in range(3):  # the cases reach what they are meant to reach
        e = np.unique(np.frexp(pa_bits(reads[k], c.cal[k, 0], c.cal[k, 1]).view(np.float32))[1])
        assert len(e) >= (8 if k == 2 else 1), (k, e)
    bits, out_n = run_device(lib, c)
    c.check(bits, out_n, device=True)


# ------------------------------------------------------------------ 3: agreement with the two-call route

@gpu
@pytest.mark.parametrize("m", list(FUSED) + ["zstd_svb_zd", "vbe21_zd", "shuffman_vbe21_zd", "hasgam_vbsse21_zdq", "rc_vbe21_zd"])
def test_equals_depress_then_formula(lib, oracle, m):
    """the floats are the formula applied to what press_hip_depress_batch writes on the same streams and rooms, and
    out_n is the same: no oracle involved"""
    import torch
    c = battery_case(oracle, m)
    d_in, d_io, d_il, d_off, d_n, d_cal = c.dev()
    d_sig = torch.full((c.total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    d_on = torch.full((len(c.rooms),), 7, dtype=torch.int32, device="cuda")
    assert i16_call(lib, m, d_in, d_io, d_il, d_sig, d_off, d_n, c.total, d_on, True) == 0, press.last_error()
    torch.cuda.synchronize()
    sig, on16 = d_sig.cpu().numpy(), d_on.cpu().numpy().view(np.uint32)
    bits, out_n = run_device(lib, c)
    assert np.array_equal(out_n, on16), m
    assert (out_n != F32).sum() >= 24
    for k, cnt in enumerate(out_n):
        if int(cnt) == F32:
            continue
        o = int(c.off[k])
        assert np.array_equal(bits[o:o + int(cnt)], pa_bits(sig[o:o + int(cnt)], c.cal[k, 0], c.cal[k, 1])), (m, k)


# ------------------------------------------------------------------ 4: refused reads stay with themselves

@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "vbe21_zd", "shuffman_vbe21_zd"])
def test_refused_reads(lib, oracle, m):
    """read 2's stream loses its tail, read 4 gets a wrong count (slow5: the count is in the stream) or a room that is
    too small: UINT32_MAX exactly where press_hip_depress_batch says so, the other reads bit for bit, nothing outside
    the rooms.  (Malformed input the decoders refuse by their length checks.)"""
    import torch
    rng = np.random.default_rng(41)
    reads = [L._walk(rng, n, 0.01) for n in (9, 2049, 32769, 65, 5000, 2048)]
    c = Case(oracle, m, reads, 13)
    c.in_len[2] -= 100
    c.rooms[4] = 4999 if m in L.SVB_KINDS else 4000
    d_in, d_io, d_il, d_off, d_n, d_cal = c.dev()
    d_sig = torch.full((c.total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    d_on = torch.full((6,), 7, dtype=torch.int32, device="cuda")
    assert i16_call(lib, m, d_in, d_io, d_il, d_sig, d_off, d_n, c.total, d_on, True) == 0, press.last_error()
    torch.cuda.synchronize()
    sig, on16 = d_sig.cpu().numpy(), d_on.cpu().numpy().view(np.uint32)
    assert int(on16[4]) == F32 and [int(on16[k]) for k in (0, 1, 3, 5)] == [9, 2049, 65, 2048], (m, on16)
    bits, out_n = run_device(lib, c)
    assert np.array_equal(out_n, on16), (m, out_n, on16)
    for k, cnt in enumerate(out_n):
        if int(cnt) == F32:
            continue
        o = int(c.off[k])
        assert np.array_equal(bits[o:o + int(cnt)], pa_bits(sig[o:o + int(cnt)], c.cal[k, 0], c.cal[k, 1])), (m, k)
        if k in (0, 1, 3, 5):
            assert np.array_equal(sig[o:o + int(cnt)], reads[k]), (m, k)
    outside = L.outside_rooms(c.total, c.off, [L.roundup8(r) for r in c.rooms])
    assert (bits[:c.total][outside] == CANARY).all(), m


# ------------------------------------------------------------------ 5: host buffers

HOST_READS = ("empty-first", "walk-7", "walk-9", "ex1-2049", "ex1-32769", "all-exceptions-3000", "wrap-5000", "constant-4000")


@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "rc_vbe21_zd"])
@pytest.mark.parametrize("pinned", [False, True])
def test_host_path(lib, oracle, m, pinned):
    """8 reads (the staged copies): exactly out_n[r] floats arrive per read, everything between them keeps its fill"""
    bat = dict(L.battery())
    held = []

    def alloc(a):
        if not pinned:
            return a
        p = lib.press_hip_host_alloc(a.nbytes)
        assert p
        held.append(p)
        v = np.frombuffer((ctypes.c_uint8 * a.nbytes).from_address(p), dtype=a.dtype)
        v[:] = a
        return v
    try:
        c = Case(oracle, m, [bat[k] for k in HOST_READS], 17, min_gap=64 if pinned else 0)
        pa = alloc(np.full(c.total, CANARY, dtype=np.uint32))
        out_n = np.full(len(c.rooms), 7, dtype=np.uint32)
        assert pa_call(lib, m, c.inb, c.in_off, c.in_len, pa, c.off, c.rooms, c.total, c.cal.reshape(-1), out_n,
                       False) == 0, press.last_error()
        assert sum(1 for v, _ in c.expect if v == "ok") >= 7
        c.check(pa, out_n, device=False)
    finally:
        for p in held:
            lib.press_hip_host_free(p)


@gpu
def test_host_overlap_is_refused(lib):
    """rooms that overlap: PRESS_HIP_EARG before anything is launched, with 2 reads and with 6"""
    for off, n in ((np.array([0, 8], dtype=np.uint64), np.array([9, 4], dtype=np.uint32)),
                   (np.array([0, 32, 64, 96, 128, 40], dtype=np.uint64), np.array([8, 8, 8, 8, 8, 30], dtype=np.uint32))):
        a = np.zeros(4096, dtype=np.uint8)
        io = np.arange(len(n), dtype=np.uint64) * 16
        il = np.full(len(n), 16, dtype=np.uint64)
        pa = np.full(256, CANARY, dtype=np.uint32)
        on = np.full(len(n), 7, dtype=np.uint32)
        cal = np.ones(2 * len(n), dtype=np.float32)
        assert pa_call(lib, "vbe21_zd", a, io, il, pa, off, n, 256, cal, on, False) == EARG
        assert "overlaps" in press.last_error()
        assert (pa == CANARY).all() and (on == 7).all()
    # device resident: an arena that is not 16-byte aligned; an empty batch
    import torch
    d_pa = torch.full((512,), CANARY, dtype=torch.int32, device="cuda")
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert lib.press_hip_depress_pa_batch(press.METHODS["vbe21_zd"], _p(z), _p(z), _p(z), 2, _p(d_pa[1:]), _p(z), _p(z), 256,
                                          _p(z), _p(z), 1) == EARG
    assert "aligned" in press.last_error()
    assert lib.press_hip_depress_pa_batch(press.METHODS["vbe21_zd"], None, None, None, 0, None, None, None, 0, None, None, 0) == 0
    torch.cuda.synchronize()
    assert (d_pa == CANARY).all()


# ------------------------------------------------------------------ 6: no sample-sized scratch on the fused path

@gpu
def test_fused_path_keeps_no_samples(lib, oracle):
    """From a library without scratch: one device-resident call of slow5_svb_zd over T samples leaves less than 2 T
    bytes of scratch (no int16 copy of the samples), the same call of vbe21_zd at least 2 T"""
    import torch
    rng = np.random.default_rng(61)
    reads = [L._walk(rng, 131072 + 8 * k, 0.005) for k in range(8)]
    cs = {m: Case(oracle, m, reads, 19) for m in ("slow5_svb_zd", "vbe21_zd")}
    dev = {m: c.dev() for m, c in cs.items()}
    torch.cuda.synchronize()
    lib.press_hip_shutdown()
    try:
        press.use_torch_stream()
        for m, fused in (("slow5_svb_zd", True), ("vbe21_zd", False)):
            c = cs[m]
            t = c.total
            assert t >= 1 << 20
            d_in, d_io, d_il, d_off, d_n, d_cal = dev[m]
            d_pa = torch.full((t,), CANARY, dtype=torch.int32, device="cuda")
            d_on = torch.full((len(reads),), 7, dtype=torch.int32, device="cuda")
            assert pa_call(lib, m, d_in, d_io, d_il, d_pa, d_off, d_n, t, d_cal, d_on, True) == 0, press.last_error()
            torch.cuda.synchronize()
            held = ctypes.c_uint64()
            lib.press_hip_scratch_buffers(ctypes.byref(held))
            print(m, "T", t, "scratch bytes", held.value)
            assert (held.value < 2 * t) if fused else (held.value >= 2 * t), (m, held.value, t)
            c.check(d_pa.cpu().numpy().view(np.uint32), d_on.cpu().numpy().view(np.uint32), device=True)
    finally:
        press.load_table()
        press.use_torch_stream()


# ------------------------------------------------------------------ 7: a BLOW5 file end to end

@gpu
def test_blow5_end_to_end(lib):
    """three-reads.blow5 -> next_batch_pa -> pa_cal -> depress_pa_batch_host / the device-resident call: the formula on
    the reference's decode of the file (three_reads.i16.bin) with the file's own calibration"""
    import torch
    meta = json.load(open(os.path.join(GOLD, "three_reads.json")))["reads"]
    raw = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    want, at = {}, 0
    for r in meta:
        want[r["read_id"]] = raw[at:at + r["n"]]
        at += r["n"]
    assert at == raw.size
    rd = press.Blow5Reader(os.path.join(GOLD, "three-reads.blow5"))
    batch = rd.next_batch_pa()
    rd.close()
    assert len(batch) == 3 and rd.signal_method == 1
    cal = press.pa_cal([d for _, _, _, d in batch])
    assert np.array_equal(cal.view(np.uint32), cal_of([d for _, _, _, d in batch]).view(np.uint32))
    assert all(d[0] > 0 and d[2] > 0 for _, _, _, d in batch)
    exp = [pa_bits(want[rid], cal[k, 0], cal[k, 1]) for k, (rid, n, _, _) in enumerate(batch)]
    out = press.depress_pa_batch_host("slow5_svb_zd", [s for _, _, s, _ in batch], [n for _, n, _, _ in batch], cal)
    for k, (rid, n, _, _) in enumerate(batch):
        assert out[k] is not None and out[k].dtype == np.float32 and len(out[k]) == n == len(want[rid]), rid
        assert np.array_equal(out[k].view(np.uint32), exp[k]), rid
    # device resident
    ns = np.array([n for _, n, _, _ in batch], dtype=np.uint32)
    inb, in_off, in_len = L.scatter_streams(np.random.default_rng(3), [s for _, _, s, _ in batch])
    off, total = L.scatter_rooms(np.random.default_rng(4), ns)
    d_pa = torch.zeros(total, dtype=torch.float32, device="cuda")
    d_on = torch.zeros(3, dtype=torch.int32, device="cuda")
    press.depress_pa_batch("slow5_svb_zd", _t(inb), _t(in_off, np.int64), _t(in_len, np.int64), d_pa, _t(off, np.int64),
                           _t(ns, np.int32), _t(cal.reshape(-1)), d_on)
    torch.cuda.synchronize()
    got = d_pa.cpu().numpy().view(np.uint32)
    assert list(d_on.cpu().numpy()) == list(ns)
    for k in range(3):
        assert np.array_equal(got[int(off[k]):int(off[k]) + int(ns[k])], exp[k]), k
