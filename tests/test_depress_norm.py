"""press_hip_depress_norm_batch: compressed reads straight to (x - median) / (1.4826 * MAD) (include/press_hip.h).

med and mad are order statistics of the decoded samples (np.partition, pinned to sigtk by
test_signal_stats.py::test_numpy_reference_is_sigtk), the floats are ((float) s + c0) * c1 with one rounding per
operation - numpy's float32 arithmetic.  Every comparison is one of integers or of uint32 bit patterns.

The read battery of _layouts.py through all 19 methods on scattered rooms behind a canary, agreement with the four-call
route (depress, signal_stats, norm_cal, depress_pa), refused reads, stats = NULL, the host path (pageable and
page-locked), overlapping rooms, and a BLOW5 file end to end.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import _layouts as L
from honours_amd import press
from test_signal_stats import GOLD, norm_bits, ref_cal, ref_stats

gpu = pytest.mark.gpu
METHODS = sorted(press.METHODS, key=lambda m: press.METHODS[m])
EARG = -2
F32 = L.FAILED32
CANARY = 0x7FC12345  # a quiet NaN with a payload: no conversion produces it
STAT_FILL = 77


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
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


def norm_call(lib, m, arena, in_off, in_len, out, off, n, total, stats, out_n, dev):
    return lib.press_hip_depress_norm_batch(press.METHODS[m], _p(arena), _p(in_off), _p(in_len), len(n), _p(out), _p(off),
                                            _p(n), total, _p(stats), _p(out_n), 1 if dev else 0)


class Case:
    """reads of one method as streams, in scattered rooms, with what the oracle decodes of them and the statistics
    of that (computed once, shared by the tests of the method)"""

    def __init__(self, oracle, m, reads, seed, min_gap=0):
        self.m, self.reads = m, reads
        rng = np.random.default_rng(seed * 100 + press.METHODS[m])
        st, _ = press.press_packed_host(m, reads)
        self.streams = [b"" if x is None else x for x in st]
        extra = 0 if m in L.SVB_KINDS else 21
        self.rooms = np.array([len(s) + (int(rng.integers(0, extra)) if extra else 0) for s in reads], dtype=np.uint32)
        self.expect = [L.expect_depress(oracle, m, s, x, int(r)) for s, x, r in zip(reads, self.streams, self.rooms)]
        self.stats = [ref_stats(w) if v == "ok" else (0, 0) for v, w in self.expect]
        self.inb, self.in_off, self.in_len = L.scatter_streams(rng, self.streams)
        self.off, self.total = L.scatter_rooms(rng, self.rooms, min_gap=min_gap)

    def dev(self):
        return (_t(self.inb), _t(self.in_off, np.int64), _t(self.in_len, np.int64), _t(self.off, np.int64),
                _t(self.rooms, np.int32))

    def check(self, bits, out_n, stats, device):
        """bits: the float arena as uint32.  out_n as the oracle's verdicts, stats as numpy's over the oracle's samples,
        every decoded read bit for bit, the canary everywhere outside [off, off + roundup8(room)) (device) or
        [off, off + out_n) (host), and in the whole room of a refused read"""
        m = self.m
        for k, (verdict, want) in enumerate(self.expect):
            tag = (m, k, int(self.rooms[k]))
            if verdict == "skip":
                continue
            o = int(self.off[k])
            if verdict == "fail":
                assert int(out_n[k]) == F32, tag
                if stats is not None:
                    assert stats[k].tolist() == [0, 0], tag
                assert (bits[o:o + L.roundup8(self.rooms[k])] == CANARY).all(), tag + ("a refused read got floats",)
                continue
            assert int(out_n[k]) == len(want), tag + (int(out_n[k]), len(want))
            med, mad = self.stats[k]
            if stats is not None:
                assert stats[k].tolist() == [med, mad], tag + (stats[k].tolist(), (med, mad))
            got = bits[o:o + len(want)]
            exp = norm_bits(want, med, mad)
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, tag + ("first mismatch at", int(bad[0]), hex(int(got[bad[0]])), hex(int(exp[bad[0]])))
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


def run_device(lib, c, with_stats=True):
    import torch
    d_in, d_io, d_il, d_off, d_n = c.dev()
    nr = len(c.rooms)
    d_out = torch.full((c.total,), CANARY, dtype=torch.int32, device="cuda")
    d_on = torch.full((nr,), 7, dtype=torch.int32, device="cuda")
    d_st = torch.full((2 * nr + 16,), STAT_FILL, dtype=torch.int32, device="cuda")
    assert norm_call(lib, c.m, d_in, d_io, d_il, d_out, d_off, d_n, c.total, d_st if with_stats else None, d_on, True) == 0, \
        press.last_error()
    torch.cuda.synchronize()
    st = d_st.cpu().numpy()
    assert (st[2 * nr:] == STAT_FILL).all(), "stats written beyond 2 * nreads"
    if not with_stats:
        assert (st == STAT_FILL).all()
    return d_out.cpu().numpy().view(np.uint32), d_on.cpu().numpy().view(np.uint32), st[:2 * nr].reshape(-1, 2) if with_stats else None


# ------------------------------------------------------------------ 1: the battery, all methods, device resident

@gpu
@pytest.mark.parametrize("m", METHODS)
def test_battery_device_resident(lib, oracle, m):
    c = battery_case(oracle, m)
    left_out = [k for k, (v, _) in enumerate(c.expect) if v == "skip"]
    assert len(left_out) == (2 if m.startswith("shuffman") else 0), (m, left_out)  # as battery_verdicts reports
    bits, out_n, stats = run_device(lib, c)
    c.check(bits, out_n, stats, device=True)


# ------------------------------------------------------------------ 2: agreement with the four-call route

@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "vbe21_zd", "shuffman_vbe21_zd", "rc_vbe21_zd"])
def test_equals_the_four_calls(lib, oracle, m):
    """press_hip_depress_batch, press_hip_signal_stats over what it decoded, press.norm_cal, press_hip_depress_pa_batch
    with that calibration: the same out_n, stats and floats - no oracle involved"""
    import torch
    c = battery_case(oracle, m)
    d_in, d_io, d_il, d_off, d_n = c.dev()
    nr = len(c.rooms)
    mid = press.METHODS[m]
    d_sig = torch.full((c.total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    d_on = torch.full((nr,), 7, dtype=torch.int32, device="cuda")
    assert lib.press_hip_depress_batch(mid, _p(d_in), _p(d_io), _p(d_il), nr, _p(d_sig), _p(d_off), _p(d_n), c.total, _p(d_on),
                                       1) == 0, press.last_error()
    torch.cuda.synchronize()
    on16 = d_on.cpu().numpy().view(np.uint32)
    cnt = np.where(on16 == F32, 0, on16).astype(np.uint32)  # a refused read has no samples
    d_st = torch.full((2 * nr,), STAT_FILL, dtype=torch.int32, device="cuda")
    press.signal_stats(d_sig, d_off, _t(cnt, np.int32), d_st)
    torch.cuda.synchronize()
    st4 = d_st.cpu().numpy().reshape(-1, 2)
    cal = press.norm_cal(st4)
    assert np.array_equal(cal.view(np.uint32), ref_cal(st4).view(np.uint32))
    d_pa = torch.full((c.total,), CANARY, dtype=torch.int32, device="cuda")
    assert lib.press_hip_depress_pa_batch(mid, _p(d_in), _p(d_io), _p(d_il), nr, _p(d_pa), _p(d_off), _p(d_n), c.total,
                                          _p(_t(cal.reshape(-1))), _p(d_on), 1) == 0, press.last_error()
    torch.cuda.synchronize()
    pa = d_pa.cpu().numpy().view(np.uint32)
    bits, out_n, stats = run_device(lib, c)
    assert np.array_equal(out_n, on16), m
    assert np.array_equal(stats, st4), m
    assert (out_n != F32).sum() >= 24
    for k, n in enumerate(out_n):
        if int(n) == F32:
            continue
        o = int(c.off[k])
        assert np.array_equal(bits[o:o + int(n)], pa[o:o + int(n)]), (m, k)


# ------------------------------------------------------------------ 3: refused reads stay with themselves

@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "vbe21_zd", "shuffman_vbe21_zd"])
def test_refused_reads(lib, oracle, m):
    """read 2's stream loses its tail, read 4 gets a wrong count (slow5: the count is in the stream) or a room that is
    too small: UINT32_MAX exactly where press_hip_depress_batch says so, stats {0, 0} there, the other reads' floats and
    stats exact, nothing outside the rooms"""
    import torch
    rng = np.random.default_rng(41)
    reads = [L._walk(rng, n, 0.01) for n in (9, 2049, 32769, 65, 5000, 2048)]
    c = Case(oracle, m, reads, 13)
    c.in_len[2] -= 100
    c.rooms[4] = 4999 if m in L.SVB_KINDS else 4000
    d_in, d_io, d_il, d_off, d_n = c.dev()
    d_sig = torch.full((c.total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    d_on = torch.full((6,), 7, dtype=torch.int32, device="cuda")
    assert lib.press_hip_depress_batch(press.METHODS[m], _p(d_in), _p(d_io), _p(d_il), 6, _p(d_sig), _p(d_off), _p(d_n), c.total,
                                       _p(d_on), 1) == 0, press.last_error()
    torch.cuda.synchronize()
    sig, on16 = d_sig.cpu().numpy(), d_on.cpu().numpy().view(np.uint32)
    assert int(on16[4]) == F32 and [int(on16[k]) for k in (0, 1, 3, 5)] == [9, 2049, 65, 2048], (m, on16)
    bits, out_n, stats = run_device(lib, c)
    assert np.array_equal(out_n, on16), (m, out_n, on16)
    for k, cnt in enumerate(out_n):
        o = int(c.off[k])
        if int(cnt) == F32:
            assert stats[k].tolist() == [0, 0], (m, k)
            assert (bits[o:o + L.roundup8(c.rooms[k])] == CANARY).all(), (m, k, "a refused read got floats")
            continue
        s = sig[o:o + int(cnt)]
        if k in (0, 1, 3, 5):
            assert np.array_equal(s, reads[k]), (m, k)
        med, mad = ref_stats(s)
        assert stats[k].tolist() == [med, mad], (m, k)
        assert np.array_equal(bits[o:o + int(cnt)], norm_bits(s, med, mad)), (m, k)
    outside = L.outside_rooms(c.total, c.off, [L.roundup8(r) for r in c.rooms])
    assert (bits[:c.total][outside] == CANARY).all(), m


# ------------------------------------------------------------------ 4: stats = NULL

@gpu
@pytest.mark.parametrize("m", ["svb12_zd", "hasgam_vbsse21_zdq"])
def test_null_stats(lib, oracle, m):
    c = battery_case(oracle, m)
    bits, out_n, stats = run_device(lib, c, with_stats=False)
    assert stats is None
    c.check(bits, out_n, None, device=True)


# ------------------------------------------------------------------ 5: host buffers

HOST_READS = ("empty-first", "walk-7", "walk-9", "ex1-2049", "ex1-32769", "all-exceptions-3000", "wrap-5000", "constant-4000")


@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "rc_vbe21_zd"])
@pytest.mark.parametrize("pinned", [False, True])
def test_host_path(lib, oracle, m, pinned):
    """8 reads (the staged copies): exactly out_n[r] floats arrive per read, everything between them keeps its fill,
    and stats come back"""
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
        out = alloc(np.full(c.total, CANARY, dtype=np.uint32))
        out_n = np.full(len(c.rooms), 7, dtype=np.uint32)
        stats = np.full((len(c.rooms) + 4, 2), STAT_FILL, dtype=np.int32)
        assert norm_call(lib, m, c.inb, c.in_off, c.in_len, out, c.off, c.rooms, c.total, stats, out_n, False) == 0, press.last_error()
        assert sum(1 for v, _ in c.expect if v == "ok") >= 7
        assert (stats[len(c.rooms):] == STAT_FILL).all()
        c.check(out, out_n, stats[:len(c.rooms)], device=False)
        # and without stats
        out2 = np.full(c.total, CANARY, dtype=np.uint32)
        assert norm_call(lib, m, c.inb, c.in_off, c.in_len, out2, c.off, c.rooms, c.total, None, out_n, False) == 0, press.last_error()
        assert np.array_equal(out2, np.asarray(out))
    finally:
        for p in held:
            lib.press_hip_host_free(p)
    # the wrapper
    fl, st = press.depress_norm_batch_host(m, c.streams, c.rooms)
    for k, (v, w) in enumerate(c.expect):
        if v == "ok":
            assert st[k].tolist() == list(c.stats[k]) and np.array_equal(fl[k].view(np.uint32), norm_bits(w, *c.stats[k])), (m, k)


@gpu
def test_host_overlap_is_refused(lib):
    """rooms that overlap: PRESS_HIP_EARG before anything is launched, with 2 reads and with 6"""
    for off, n in ((np.array([0, 8], dtype=np.uint64), np.array([9, 4], dtype=np.uint32)),
                   (np.array([0, 32, 64, 96, 128, 40], dtype=np.uint64), np.array([8, 8, 8, 8, 8, 30], dtype=np.uint32))):
        a = np.zeros(4096, dtype=np.uint8)
        io = np.arange(len(n), dtype=np.uint64) * 16
        il = np.full(len(n), 16, dtype=np.uint64)
        out = np.full(256, CANARY, dtype=np.uint32)
        on = np.full(len(n), 7, dtype=np.uint32)
        st = np.full(2 * len(n), STAT_FILL, dtype=np.int32)
        assert norm_call(lib, "vbe21_zd", a, io, il, out, off, n, 256, st, on, False) == EARG
        assert "overlaps" in press.last_error()
        assert (out == CANARY).all() and (on == 7).all() and (st == STAT_FILL).all()
    # device resident: an arena that is not 16-byte aligned; an empty batch
    import torch
    d_out = torch.full((512,), CANARY, dtype=torch.int32, device="cuda")
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert lib.press_hip_depress_norm_batch(press.METHODS["vbe21_zd"], _p(z), _p(z), _p(z), 2, _p(d_out[1:]), _p(z), _p(z), 256,
                                            _p(z), _p(z), 1) == EARG
    assert "aligned" in press.last_error()
    assert lib.press_hip_depress_norm_batch(press.METHODS["vbe21_zd"], None, None, None, 0, None, None, None, 0, None, None, 0) == 0
    torch.cuda.synchronize()
    assert (d_out == CANARY).all()


# ------------------------------------------------------------------ 6: a BLOW5 file end to end

@gpu
def test_blow5_end_to_end(lib):
    """three-reads.blow5 -> next_batch -> depress_norm_batch_host / the device-resident wrapper: the definition over the
    reference's decode of the file (three_reads.i16.bin), and the reference's own statistics (sigtk_stats.json)"""
    import torch
    meta = json.load(open(os.path.join(GOLD, "three_reads.json")))["reads"]
    gold = {g["name"]: (g["med"], g["mad"]) for g in json.load(open(os.path.join(GOLD, "sigtk_stats.json")))["reads"]}
    raw = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    want, at = {}, 0
    for r in meta:
        want[r["read_id"]] = raw[at:at + r["n"]]
        at += r["n"]
    assert at == raw.size
    rd = press.Blow5Reader(os.path.join(GOLD, "three-reads.blow5"))
    batch = rd.next_batch()
    rd.close()
    assert len(batch) == 3
    fl, st = press.depress_norm_batch_host("slow5_svb_zd", [s for _, _, s in batch], [n for _, n, _ in batch])
    exp = []
    for k, (rid, n, _) in enumerate(batch):
        med, mad = ref_stats(want[rid])
        assert (med, mad) == gold["three_reads/" + rid] and st[k].tolist() == [med, mad], rid
        exp.append(norm_bits(want[rid], med, mad))
        assert fl[k] is not None and fl[k].dtype == np.float32 and len(fl[k]) == n == len(want[rid]), rid
        assert np.array_equal(fl[k].view(np.uint32), exp[k]), rid
    # device resident
    ns = np.array([n for _, n, _ in batch], dtype=np.uint32)
    inb, in_off, in_len = L.scatter_streams(np.random.default_rng(3), [s for _, _, s in batch])
    off, total = L.scatter_rooms(np.random.default_rng(4), ns)
    d_out = torch.zeros(total, dtype=torch.float32, device="cuda")
    d_on = torch.zeros(3, dtype=torch.int32, device="cuda")
    d_st = torch.zeros(6, dtype=torch.int32, device="cuda")
    press.depress_norm_batch("slow5_svb_zd", _t(inb), _t(in_off, np.int64), _t(in_len, np.int64), d_out, _t(off, np.int64),
                             _t(ns, np.int32), d_on, d_st)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32)
    assert list(d_on.cpu().numpy()) == list(ns)
    assert np.array_equal(d_st.cpu().numpy().reshape(-1, 2), st)
    for k in range(3):
        assert np.array_equal(got[int(off[k]):int(off[k]) + int(ns[k])], exp[k]), k
