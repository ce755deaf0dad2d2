"""press_hip_depress_chunks_batch, press_hip_chunk_plan, press_hip_scale_cal: compressed reads straight to scaled
half-precision chunk rows (include/press_hip.h).

The yardstick is built in numpy from the oracle's decode (_layouts.expect_depress): the quantiles are order statistics
(np.partition, test_signal_quantiles.ref_quantiles), the scaling is float32 arithmetic one operation per statement, the
row layout is a Python restatement of the plan, and the half-precision roundings are numpy's astype(float16) and the
integer formula for bfloat16 - both pinned to torch's CPU conversions below.  Every comparison is one of integers or of
bit patterns.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch  # before the library is loaded, as in a run of the whole suite: torch's HIP runtime comes first

import _layouts as L
from honours_amd import build, press
from test_depress_norm import HOST_READS, Case, battery_case
from test_signal_quantiles import ref_quantiles
from test_signal_stats import GOLD, ref_cal, ref_stats

gpu = pytest.mark.gpu
METHODS = sorted(press.METHODS, key=lambda m: press.METHODS[m])
EARG = -2
F32 = L.FAILED32
CANARY = {4: 0x7FC12345, 2: 0x7E57}  # by element size; neither is a zero
Q_FILL = 77
DT = {"float32": 0, "float16": 1, "bfloat16": 2}
ES = {"float32": 4, "float16": 2, "bfloat16": 2}
PLAN_GRID = ((8, 0), (64, 0), (64, 8), (64, 5), (64, 63), (1024, 104))


def make_rule(scale_min=1.0, shift_min=10.0):
    """the documented example: the 0.2 and 0.9 quantiles, factors 0.51 and 0.53, floors 10 and 1"""
    return press.ScaleRule(1, 5, 9, 10, 0.51, shift_min, 0.53, scale_min)


RULE = make_rule()


# ------------------------------------------------------------------ the definitions, restated

def plan_ref(ns, T, overlap):
    """-> (row_first uint64[nreads + 1], row_read, row_start)"""
    S = T - overlap
    first, rr, rs = [0], [], []
    for r, c in enumerate(ns):
        c = int(c)
        if c == 0:
            starts = []
        elif c <= T:
            starts = [0]
        else:
            k = 1 + (c - T + S - 1) // S
            starts = [j * S for j in range(k - 1)] + [c - T]
        rr += [r] * len(starts)
        rs += starts
        first.append(first[-1] + len(starts))
    return np.array(first, dtype=np.uint64), np.array(rr, dtype=np.uint32), np.array(rs, dtype=np.uint32)


def rule_cal_ref(q, rule):
    """(nreads, 2) {q_lo, q_hi} -> (nreads, 2) float32 {-shift, 1 / scale}, one float32 operation per statement"""
    f = np.float32
    q = np.asarray(q, dtype=np.int64).reshape(-1, 2)
    total = (q[:, 0] + q[:, 1]).astype(f)
    spread = (q[:, 1] - q[:, 0]).astype(f)
    shift = f(rule.shift_mul) * total
    shift = np.maximum(f(rule.shift_min), shift)
    scale = f(rule.scale_mul) * spread
    scale = np.maximum(f(rule.scale_min), scale)
    with np.errstate(all="ignore"):
        inv = f(1.0) / scale
    return np.stack([-shift, inv], axis=1).astype(f)


def y_ref(s, cal):
    t = np.asarray(s).astype(np.float32) + np.float32(cal[0])
    with np.errstate(all="ignore"):
        return (t * np.float32(cal[1])).astype(np.float32)


def f16_ref(y):
    with np.errstate(all="ignore"):
        return np.asarray(y, dtype=np.float32).astype(np.float16).view(np.uint16)


def bf16_ref(y):
    u = np.asarray(y, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def to_bits(y, dtype):
    return y.view(np.uint32) if dtype == "float32" else f16_ref(y) if dtype == "float16" else bf16_ref(y)


def calibration(dec, rule):
    """decoded samples of the reads (None: refused or left out) -> (q (nreads, 2) int64, cal (nreads, 2) float32)"""
    if rule is None:
        q = np.array([ref_stats(s) if s is not None else (0, 0) for s in dec], dtype=np.int64).reshape(-1, 2)
        return q, ref_cal(q)
    rk = [(rule.lo_num, rule.lo_den), (rule.hi_num, rule.hi_den)]
    q = np.array([ref_quantiles(s, rk) if s is not None else [0, 0] for s in dec], dtype=np.int64).reshape(-1, 2)
    return q, rule_cal_ref(q, rule)


def rows_ref(dec, rooms, T, overlap, dtype, cal):
    """-> ([rows, T] bit patterns, row_read): zeros at and beyond the decoded count, and in a read without samples"""
    first, rr, rs = plan_ref(rooms, T, overlap)
    out = np.zeros((int(first[-1]), T), dtype=np.uint32 if dtype == "float32" else np.uint16)
    for r, s in enumerate(dec):
        a, b = int(first[r]), int(first[r + 1])
        if a == b or s is None or len(s) == 0:
            continue
        yb = to_bits(y_ref(s, cal[r]), dtype)
        idx = rs[a:b].astype(np.int64)[:, None] + np.arange(T)[None, :]
        out[a:b] = np.where(idx < len(s), yb[np.minimum(idx, len(s) - 1)], 0)
    return out, rr


# ------------------------------------------------------------------ CPU

@pytest.fixture(scope="module")
def cpu_lib():
    build.build()
    return press.load_library()


def test_chunk_plan_against_the_restatement(cpu_lib):
    cs = list(range(300)) + [32767, 32768, 32769, 65537]
    for T, ov in PLAN_GRID:
        S = T - ov
        first, rr, rs = press.chunk_plan(cs, T, ov)
        wf, wr, ws = plan_ref(cs, T, ov)
        assert first.dtype == np.uint64 and rr.dtype == np.uint32 and rs.dtype == np.uint32
        assert np.array_equal(first, wf) and np.array_equal(rr, wr) and np.array_equal(rs, ws), (T, ov)
        for r, c in enumerate(cs):  # the restatement itself: every sample covered, starts increase, no row past the end
            st = ws[int(wf[r]):int(wf[r + 1])].astype(np.int64)
            assert len(st) == (0 if c == 0 else 1 if c <= T else 1 + -(-(c - T) // S)), (T, ov, c)
            if c == 0:
                continue
            assert st[0] == 0 and (np.diff(st) > 0).all() and (np.diff(st) <= S).all() and st[-1] + T >= c, (T, ov, c)
            assert c <= T or st[-1] + T == c, (T, ov, c)
    # row_first alone
    n = np.array([0, 5, 64, 65, 1000], dtype=np.uint32)
    first = np.zeros(6, dtype=np.uint64)
    assert cpu_lib.press_hip_chunk_plan(n.ctypes.data, 5, 64, 8, first.ctypes.data, None, None) == 0
    assert first.tolist() == [0, 0, 1, 2, 4, 4 + 1 + -(-(1000 - 64) // 56)]
    assert cpu_lib.press_hip_chunk_plan(None, 0, 64, 8, first.ctypes.data, None, None) == 0 and first[0] == 0
    for T, ov in ((60, 0), (64, 64), (64, 65), (0, 0), (4, 0)):
        assert cpu_lib.press_hip_chunk_plan(n.ctypes.data, 5, T, ov, first.ctypes.data, None, None) == EARG, (T, ov)
        with pytest.raises(press.PressError):
            press.chunk_plan(n, T, ov)
    assert cpu_lib.press_hip_chunk_plan(n.ctypes.data, 5, 64, 8, None, None, None) == EARG


def test_scale_cal_against_numpy(cpu_lib):
    rng = np.random.default_rng(23)
    pairs = [(100, 100), (500, 400), (-32768, 32767), (32767, -32768), (-32768, -32768), (32767, 32767), (0, 0), (3, 9), (-4, 30),
             (-400, -380), (9, 29)]
    pairs += list(zip(rng.integers(-32768, 32768, size=300).tolist(), rng.integers(-32768, 32768, size=300).tolist()))
    q = np.array(pairs, dtype=np.int32)
    for rule in (RULE, make_rule(scale_min=1e6), make_rule(scale_min=1e-3), make_rule(shift_min=-1e9),
                 press.ScaleRule(1, 2, 1, 1, -0.25, -7.5, 3.0, 0.125)):
        want = rule_cal_ref(q, rule)
        got = press.scale_cal(q, rule)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got = press.scale_cal(q, RULE)
    assert got[0].tolist() == [-np.float32(0.51) * np.float32(200.0), 1.0]      # q_lo == q_hi: the scale is scale_min
    assert got[1, 1] == 1.0                                                      # q_hi < q_lo: it falls to scale_min
    assert got[2].tolist() == [-10.0, float(np.float32(1) / (np.float32(0.53) * np.float32(65535.0)))]  # shift_min wins
    assert got[7, 0] == -10.0 and got[10, 0] == float(-(np.float32(0.51) * np.float32(38.0)))  # ... wins, and loses
    assert got[8, 1] == float(np.float32(1) / (np.float32(0.53) * np.float32(34.0)))
    cal = np.zeros(4, dtype=np.float32)
    assert cpu_lib.press_hip_scale_cal(None, 0, ctypes.addressof(RULE), None) == 0
    assert cpu_lib.press_hip_scale_cal(q.ctypes.data, 2, None, cal.ctypes.data) == EARG
    assert cpu_lib.press_hip_scale_cal(None, 2, ctypes.addressof(RULE), cal.ctypes.data) == EARG
    assert cpu_lib.press_hip_scale_cal(q.ctypes.data, 2, ctypes.addressof(RULE), None) == EARG


def bad_rules():
    inf, nan = float("inf"), float("nan")
    return [press.ScaleRule(1, 0, 9, 10, 0.51, 10.0, 0.53, 1.0), press.ScaleRule(1, 5, 9, 0, 0.51, 10.0, 0.53, 1.0),
            press.ScaleRule(6, 5, 9, 10, 0.51, 10.0, 0.53, 1.0), press.ScaleRule(1, 5, 11, 10, 0.51, 10.0, 0.53, 1.0),
            press.ScaleRule(1, 5, 9, 10, nan, 10.0, 0.53, 1.0), press.ScaleRule(1, 5, 9, 10, 0.51, nan, 0.53, 1.0),
            press.ScaleRule(1, 5, 9, 10, 0.51, 10.0, inf, 1.0), press.ScaleRule(1, 5, 9, 10, 0.51, -inf, 0.53, 1.0),
            press.ScaleRule(1, 5, 9, 10, 0.51, 10.0, 0.53, inf), press.ScaleRule(1, 5, 9, 10, 0.51, 10.0, 0.53, nan),
            press.ScaleRule(1, 5, 9, 10, 0.51, 10.0, 0.53, 0.0), press.ScaleRule(1, 5, 9, 10, 0.51, 10.0, 0.53, -1.0)]


def test_rule_refusals(cpu_lib):
    q = np.array([[1, 2]], dtype=np.int32)
    cal = np.full(2, 5.0, dtype=np.float32)
    for k, rule in enumerate(bad_rules()):
        assert cpu_lib.press_hip_scale_cal(q.ctypes.data, 1, ctypes.addressof(rule), cal.ctypes.data) == EARG, k
        assert "rule" in press.last_error()
    assert (cal == 5.0).all()


def test_argument_checks_need_no_device(cpu_lib):
    """bad method, dtype, T, overlap or rule, NULL arguments: PRESS_HIP_EARG before any device call"""
    p = lambda x: x.ctypes.data
    a = np.zeros(256, dtype=np.uint8)
    io = np.zeros(1, dtype=np.uint64)
    il = np.full(1, 16, dtype=np.uint64)
    rows = np.zeros(64, dtype=np.float32)
    n = np.full(1, 8, dtype=np.uint32)
    first = np.array([0, 1], dtype=np.uint64)
    q = np.full(2, Q_FILL, dtype=np.int32)
    on = np.full(1, 7, dtype=np.uint32)
    mid = press.METHODS["slow5_svb_zd"]
    rule = ctypes.addressof(RULE)

    def call(dev, m=mid, rw=p(rows), dt=0, T=8, ov=0, rf=p(first), off=p(io), nn=p(n), ru=rule, qq=p(q), o=p(on), inb=p(a)):
        return cpu_lib.press_hip_depress_chunks_batch(m, inb, p(io), p(il), 1, rw, 8, dt, T, ov, rf, off, nn, 64, ru, qq, o, dev)
    for dev in (0, 1):
        for bad in (-1, len(press.METHODS)):
            assert call(dev, m=bad) == EARG and "not available" in press.last_error()
        for bad in (-1, 3):
            assert call(dev, dt=bad) == EARG and "dtype" in press.last_error()
        for T, ov in ((0, 0), (12, 0), (8, 8), (8, 9)):
            assert call(dev, T=T, ov=ov) == EARG and "multiple of 8" in press.last_error()
        for bad in bad_rules():
            assert call(dev, ru=ctypes.addressof(bad)) == EARG and "rule" in press.last_error()
        for kw in ("rw", "rf", "off", "nn", "o", "inb"):
            assert call(dev, **{kw: None}) == EARG and "NULL" in press.last_error(), kw
    assert (q == Q_FILL).all() and on[0] == 7 and (rows == 0).all()


def test_workspace_bytes(cpu_lib):
    t, nr = 1 << 20, 64
    ws_fn = cpu_lib.press_hip_depress_chunks_workspace_bytes
    for m, mid in press.METHODS.items():
        norm = int(cpu_lib.press_hip_depress_norm_workspace_bytes(mid, t, nr))
        ws = int(ws_fn(mid, t, nr, 1024, 104))
        assert ws >= norm, (m, ws, norm)
        assert ws - norm >= nr * 1024, (m, ws - norm)  # the second row of counters of every read
        assert ws == int(ws_fn(mid, t, nr, 8, 0))
    for bad in (-1, len(press.METHODS), 1000):
        assert ws_fn(bad, t, nr, 64, 8) == 0
    for T, ov in ((0, 0), (12, 0), (8, 8)):
        assert ws_fn(0, t, nr, T, ov) == 0


def test_half_precision_yardsticks_are_torch():
    """astype(float16) and the bfloat16 formula agree with torch's CPU conversions: 2^20 normal values, the float16
    subnormal range, the overflow edge, signed zeros"""
    rng = np.random.default_rng(99)
    u = rng.integers(0x00800000, 0x7F800000, size=1 << 20, dtype=np.uint32) | (rng.integers(0, 2, size=1 << 20, dtype=np.uint32) << 31)
    sub = np.concatenate([rng.uniform(-7e-5, 7e-5, size=4096), [2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -14, 5.96e-8, 2.98e-8,
                                                                 2.99e-8, -2.0 ** -24, -2.0 ** -25]]).astype(np.float32)
    edge = np.array([65504.0, 65519.0, 65520.0, 65521.0, 70000.0, -65520.0, -70000.0, 0.0, -0.0, 3.3895314e38, 3.4e38, -3.4e38],
                    dtype=np.float32)
    y = np.concatenate([u.view(np.float32), sub, edge])
    t = torch.from_numpy(y.copy())
    assert np.array_equal(f16_ref(y), t.to(torch.float16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(bf16_ref(y), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert f16_ref(edge[:5]).tolist() == [0x7BFF, 0x7BFF, 0x7C00, 0x7C00, 0x7C00] and f16_ref(edge[7:9]).tolist() == [0, 0x8000]
    assert f16_ref(np.array([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25], dtype=np.float32)).tolist() == [1, 0, 1]
    assert bf16_ref(edge[9:]).tolist() == [0x7F7F, 0x7F80, 0xFF80]


# ------------------------------------------------------------------ GPU plumbing

@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.load_table()
    press.use_torch_stream()
    lb.press_hip_host_alloc.restype = ctypes.c_void_p
    lb.press_hip_host_alloc.argtypes = [ctypes.c_uint64]
    lb.press_hip_host_free.argtypes = [ctypes.c_void_p]
    yield lb
    torch.cuda.synchronize()
    press.use_torch_stream()
    torch.cuda.empty_cache()
    while PINNED:  # (freed here, not in the test: the report of a failing test may still print arrays that view them)
        lb.press_hip_host_free(PINNED.pop())


def _p(x):
    if x is None:
        return None
    if isinstance(x, press.ScaleRule):
        return ctypes.addressof(x)
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def _t(a, dtype=None):
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


def chunks_call(lib, m, arena, in_off, in_len, rows, cap, dtype, T, ov, first, off, n, total, rule, q, out_n, dev):
    return lib.press_hip_depress_chunks_batch(press.METHODS[m], _p(arena), _p(in_off), _p(in_len), len(n), _p(rows), cap, DT[dtype], T, ov,
                                              _p(first), _p(off), _p(n), total, _p(rule), _p(q), _p(out_n), 1 if dev else 0)


GUARD = 5  # rows of canary behind the arena's cap
PINNED = []  # page-locked buffers of test_host_path


class Dev:
    """a Case on the device, and the arena of one call"""

    def __init__(self, c):
        self.c = c
        self.d_in, self.d_io, self.d_il, self.d_off, self.d_n = c.dev()

    def run(self, lib, T, ov, dtype, rule, cap=None, with_q=True, enqueue_only=False):
        """-> (rows [cap + GUARD, T] as bit patterns, out_n, q or None, planned rows); cap defaults to planned + 2"""
        c = self.c
        nr = len(c.rooms)
        first, _, _ = plan_ref(c.rooms, T, ov)
        planned = int(first[-1])
        cap = planned + 2 if cap is None else cap
        es = ES[dtype]
        self.d_rows = torch.full(((cap + GUARD) * T,), CANARY[es], dtype=torch.int32 if es == 4 else torch.int16, device="cuda")
        self.d_on = torch.full((nr,), 7, dtype=torch.int32, device="cuda")
        self.d_q = torch.full((2 * nr + 16,), Q_FILL, dtype=torch.int32, device="cuda")
        self.d_first = _t(first, np.int64)
        torch.cuda.synchronize()
        self.shape = (cap + GUARD, T, es, nr, with_q, planned)
        if enqueue_only:
            return self
        self.enqueue(lib, T, ov, dtype, rule, cap, with_q)
        return self.fetch()

    def enqueue(self, lib, T, ov, dtype, rule, cap, with_q=True):
        assert chunks_call(lib, self.c.m, self.d_in, self.d_io, self.d_il, self.d_rows, cap, dtype, T, ov, self.d_first, self.d_off,
                           self.d_n, self.c.total, rule, self.d_q if with_q else None, self.d_on, True) == 0, press.last_error()

    def fetch(self):
        torch.cuda.synchronize()
        nrow, T, es, nr, with_q, planned = self.shape
        q = self.d_q.cpu().numpy()
        assert (q[2 * nr:] == Q_FILL).all(), "q written beyond 2 * nreads"
        if not with_q:
            assert (q == Q_FILL).all()
        rows = self.d_rows.cpu().numpy().view(np.uint32 if es == 4 else np.uint16).reshape(nrow, T)
        return rows, self.d_on.cpu().numpy().view(np.uint32), q[:2 * nr].reshape(-1, 2) if with_q else None, planned


def check(tag, expect, rooms, T, ov, dtype, rule, rows, out_n, q, cap):
    """expect: per read ("ok", samples) / ("fail", None) / ("skip", None).  out_n and q as the yardstick's, every row below
    the cap exact bit for bit (zeros where the rule says), the canary in every row at or beyond min(cap, planned)"""
    dec = [w if v == "ok" else None for v, w in expect]
    wq, cal = calibration(dec, rule)
    want, rr = rows_ref(dec, rooms, T, ov, dtype, cal)
    planned = want.shape[0]
    written = min(cap, planned)
    for k, (v, w) in enumerate(expect):
        if v == "skip":
            continue
        assert int(out_n[k]) == (F32 if v == "fail" else len(w)), tag + (k, int(out_n[k]))
        if q is not None:
            assert q[k].tolist() == wq[k].tolist(), tag + (k, q[k].tolist(), wq[k].tolist())
    keep = np.array([expect[r][0] != "skip" for r in rr[:written]], dtype=bool)
    bad = np.nonzero(((rows[:written] != want[:written]).any(axis=1)) & keep)[0]
    if bad.size:
        b = int(bad[0])
        col = int(np.nonzero(rows[b] != want[b])[0][0])
        assert False, tag + ("row", b, "of read", int(rr[b]), "column", col, hex(int(rows[b, col])), hex(int(want[b, col])))
    can = CANARY[rows.dtype.itemsize]
    assert (rows[written:] == can).all(), tag + ("written at or beyond min(nrows_cap, planned rows)",)
    return want


# ------------------------------------------------------------------ 1: the battery, all methods, float32 with a rule

@gpu
@pytest.mark.parametrize("m", METHODS)
def test_battery_device_resident(lib, oracle, m):
    c = battery_case(oracle, m)
    left_out = [k for k, (v, _) in enumerate(c.expect) if v == "skip"]
    assert len(left_out) == (2 if m.startswith("shuffman") else 0), (m, left_out)  # as battery_verdicts reports
    rows, out_n, q, planned = Dev(c).run(lib, 64, 8, "float32", RULE)
    want = check((m,), c.expect, c.rooms, 64, 8, "float32", RULE, rows, out_n, q, planned + 2)
    assert planned > 5000 and (want == 0).any() and (want != 0).any()


# ------------------------------------------------------------------ 2: the shapes and the three dtypes

def shape_lengths(T, ov):
    S = T - ov
    cs = [0, 1, 7, T - 1, T, T + 1, T + S, T + S + 1, 2 * T, 2049, 32767, 32768, 32769, 65537]
    return [min(c, 2049) for c in cs] if ov == 63 else cs


_shape_cases = {}


def shape_case(oracle, m, T, ov):
    if (m, T, ov) not in _shape_cases:
        rng = np.random.default_rng(T * 100 + ov)
        _shape_cases[(m, T, ov)] = Case(oracle, m, [L._walk(rng, c, 0.01) for c in shape_lengths(T, ov)], 19)
    return _shape_cases[(m, T, ov)]


@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "shuffman_vbe21_zd"])
@pytest.mark.parametrize("T,ov", [(8, 0), (64, 0), (64, 5), (64, 63), (1024, 104), (2048, 104), (10000, 500)])
def test_shapes_and_dtypes(lib, oracle, m, T, ov):
    """(2048, 104) and (10000, 500): the writer's other path, several workgroups of 2048 columns on a row - a whole number
    of them, and a last one that reaches beyond T - also with the row cap inside the longest read"""
    c = shape_case(oracle, m, T, ov)
    d = Dev(c)
    first, _, _ = plan_ref(c.rooms, T, ov)
    big = int(np.argmax(np.diff(first.astype(np.int64))))
    mid = int(first[big]) + 2
    assert T < 2048 or int(first[big]) + 2 < int(first[big + 1]) - 1  # (the cap is inside a read, not at its edge)
    for dtype in ("float32", "float16", "bfloat16"):
        rows, out_n, q, planned = d.run(lib, T, ov, dtype, RULE)
        check((m, T, ov, dtype), c.expect, c.rooms, T, ov, dtype, RULE, rows, out_n, q, planned + 2)
        if T >= 2048:
            rows, out_n, q, planned = d.run(lib, T, ov, dtype, RULE, cap=mid)
            check((m, T, ov, dtype, "cap", mid), c.expect, c.rooms, T, ov, dtype, RULE, rows, out_n, q, mid)


# ------------------------------------------------------------------ 3, 4: the existing calls as yardsticks

@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "rc_vbe21_zd"])
def test_no_rule_is_depress_norm(lib, oracle, m):
    """rule == NULL, float32: every row is the matching slice of press_hip_depress_norm_batch's output, q its stats"""
    from test_depress_norm import run_device
    c = battery_case(oracle, m)
    bits, on_norm, stats = run_device(lib, c)
    rows, out_n, q, planned = Dev(c).run(lib, 64, 8, "float32", None)
    assert np.array_equal(out_n, on_norm) and np.array_equal(q, stats)
    first, rr, rs = plan_ref(c.rooms, 64, 8)
    seen = 0
    for row in range(planned):
        r = int(rr[row])
        if int(out_n[r]) == F32:
            assert (rows[row] == 0).all()
            continue
        o, cnt, st = int(c.off[r]), int(out_n[r]), int(rs[row])
        k = max(0, min(64, cnt - st))
        assert np.array_equal(rows[row, :k], bits[o + st:o + st + k]) and (rows[row, k:] == 0).all(), (m, row, r)
        seen += 1
    assert seen > 5000
    check((m,), c.expect, c.rooms, 64, 8, "float32", None, rows, out_n, q, planned + 2)


@gpu
@pytest.mark.parametrize("m", ["svb12_zd", "vbbe21_zd"])
def test_with_a_rule_is_depress_pa(lib, oracle, m):
    """with a rule, float32: every row is the matching slice of press_hip_depress_pa_batch given press_hip_scale_cal(q)"""
    c = battery_case(oracle, m)
    d = Dev(c)
    rows, out_n, q, planned = d.run(lib, 64, 8, "float32", RULE)
    cal = press.scale_cal(q, RULE)
    nr = len(c.rooms)
    d_pa = torch.full((c.total,), CANARY[4], dtype=torch.int32, device="cuda")
    d_on = torch.full((nr,), 7, dtype=torch.int32, device="cuda")
    assert lib.press_hip_depress_pa_batch(press.METHODS[m], _p(d.d_in), _p(d.d_io), _p(d.d_il), nr, _p(d_pa), _p(d.d_off), _p(d.d_n),
                                          c.total, _p(_t(cal.reshape(-1))), _p(d_on), 1) == 0, press.last_error()
    torch.cuda.synchronize()
    pa = d_pa.cpu().numpy().view(np.uint32)
    assert np.array_equal(d_on.cpu().numpy().view(np.uint32), out_n)
    first, rr, rs = plan_ref(c.rooms, 64, 8)
    for row in range(planned):
        r = int(rr[row])
        o, cnt, st = int(c.off[r]), int(out_n[r]), int(rs[row])
        k = 0 if cnt == F32 else max(0, min(64, cnt - st))
        assert np.array_equal(rows[row, :k], pa[o + st:o + st + k]) and (rows[row, k:] == 0).all(), (m, row, r)


# ------------------------------------------------------------------ 5: float16 at its edges

_flat = {}


def flat_case(oracle):
    """reads that hold one level in 19 samples of 20, so q_lo == q_hi and the scale falls to scale_min"""
    if not _flat:
        rng = np.random.default_rng(55)
        reads = []
        for n in (100, 3000, 40000):
            s = np.full(n, 500, dtype=np.int16)
            k = rng.random(n) < 0.05
            s[k] = rng.integers(-32768, 32768, size=int(k.sum()))
            reads.append(s)
        _flat["c"] = Case(oracle, "slow5_svb_zd", reads, 31)
    return _flat["c"]


@gpu
@pytest.mark.parametrize("scale_min", [1e6, 1e-3])
def test_float16_subnormals_and_overflow(lib, oracle, scale_min):
    """the scale at scale_min (q_lo == q_hi = 500, shift 510).  1e6: the level and everything within 61 of the shift
    fall in float16's subnormal range and are kept; 1e-3: everything beyond 65 of the shift overflows to infinity"""
    c = flat_case(oracle)
    rule = make_rule(scale_min=scale_min)
    rows, out_n, q, planned = Dev(c).run(lib, 64, 5, "float16", rule)
    assert q.tolist() == [[500, 500]] * 3
    want = check((scale_min,), c.expect, c.rooms, 64, 5, "float16", rule, rows, out_n, q, planned + 2)
    mag = want & 0x7FFF
    if scale_min > 1:
        assert ((mag > 0) & (mag < 0x0400)).sum() > 40000 and (mag < 0x3000).all()
    else:
        assert (mag == 0x7C00).sum() > 1000 and (mag <= 0x7C00).all() and (want == 0xF0E2).sum() > 40000  # -10000: the level


# ------------------------------------------------------------------ 6: refused reads stay with themselves

@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "vbe21_zd", "shuffman_vbe21_zd"])
def test_refused_reads(lib, oracle, m):
    """test_depress_norm's refusals: read 2's stream loses its tail, read 4 gets a wrong count or a room too small.  The
    yardstick for what is decoded is press_hip_depress_batch; rows of a refused read are zeros, its q {0, 0}"""
    rng = np.random.default_rng(41)
    reads = [L._walk(rng, n, 0.01) for n in (9, 2049, 32769, 65, 5000, 2048)]
    c = Case(oracle, m, reads, 13)
    c.in_len[2] -= 100
    c.rooms[4] = 4999 if m in L.SVB_KINDS else 4000
    d = Dev(c)
    d_sig = torch.full((c.total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    d_on = torch.full((6,), 7, dtype=torch.int32, device="cuda")
    assert lib.press_hip_depress_batch(press.METHODS[m], _p(d.d_in), _p(d.d_io), _p(d.d_il), 6, _p(d_sig), _p(d.d_off), _p(d.d_n), c.total,
                                       _p(d_on), 1) == 0, press.last_error()
    torch.cuda.synchronize()
    sig, on16 = d_sig.cpu().numpy(), d_on.cpu().numpy().view(np.uint32)
    assert int(on16[4]) == F32 and [int(on16[k]) for k in (0, 1, 3, 5)] == [9, 2049, 65, 2048], (m, on16)
    expect = [("fail", None) if int(k) == F32 else ("ok", sig[int(o):int(o) + int(k)]) for o, k in zip(c.off, on16)]
    for k in (0, 1, 3, 5):
        assert np.array_equal(expect[k][1], reads[k]), (m, k)
    for dtype in ("float32", "bfloat16"):
        rows, out_n, q, planned = d.run(lib, 64, 8, dtype, RULE)
        assert np.array_equal(out_n, on16)
        want = check((m, dtype), expect, c.rooms, 64, 8, dtype, RULE, rows, out_n, q, planned + 2)
        first, _, _ = plan_ref(c.rooms, 64, 8)
        assert first[5] > first[4] and (rows[int(first[4]):int(first[5])] == 0).all() and q[4].tolist() == [0, 0]


# ------------------------------------------------------------------ 7: a room larger than the read

@gpu
@pytest.mark.parametrize("m", ["vbe21_zd", "zstd_hasgam_vbsse21_zdq"])
def test_room_larger_than_the_read(lib, oracle, m):
    """the methods that carry their count: the layout follows n[r], the columns at and beyond out_n[r] are zeros"""
    rng = np.random.default_rng(77)
    reads = [L._walk(rng, n, 0.01) for n in (60, 64, 100, 1000, 33000)]
    c = Case(oracle, m, reads, 29)
    c.rooms = (np.array([len(s) for s in reads]) + np.array([10, 1, 200, 57, 56 * 3 + 1])).astype(np.uint32)
    c.off, c.total = L.scatter_rooms(np.random.default_rng(5), c.rooms)
    c.expect = [("ok", s) for s in reads]
    rows, out_n, q, planned = Dev(c).run(lib, 64, 8, "float16", RULE)
    assert [int(x) for x in out_n] == [len(s) for s in reads]
    want = check((m,), c.expect, c.rooms, 64, 8, "float16", RULE, rows, out_n, q, planned + 2)
    first, _, rs = plan_ref(c.rooms, 64, 8)
    assert planned == int(plan_ref(c.rooms, 64, 8)[0][-1]) > int(plan_ref([len(s) for s in reads], 64, 8)[0][-1])
    assert (want[int(first[5]) - 1] == 0).all()  # the last row of the last read lies wholly behind its samples


# ------------------------------------------------------------------ 8, 9, 10: the cap, q == NULL, alignment

@gpu
def test_cap_in_the_middle_of_a_read(lib, oracle):
    c = shape_case(oracle, "slow5_svb_zd", 64, 5)
    first, _, _ = plan_ref(c.rooms, 64, 5)
    big = int(np.argmax(np.diff(first.astype(np.int64))))
    for cap in (int(first[big]) + 3, 0, 1):
        rows, out_n, q, planned = Dev(c).run(lib, 64, 5, "float16", RULE, cap=cap)
        assert cap < planned
        check((cap,), c.expect, c.rooms, 64, 5, "float16", RULE, rows, out_n, q, cap)


@gpu
def test_null_q(lib, oracle):
    c = shape_case(oracle, "shuffman_vbe21_zd", 64, 5)
    for rule in (RULE, None):
        rows, out_n, q, planned = Dev(c).run(lib, 64, 5, "bfloat16", rule, with_q=False)
        assert q is None
        check((rule is None,), c.expect, c.rooms, 64, 5, "bfloat16", rule, rows, out_n, None, planned + 2)


@gpu
def test_misaligned_rows_and_empty_batch(lib):
    d_rows = torch.full((512,), CANARY[2], dtype=torch.int16, device="cuda")
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    call = lambda rows: lib.press_hip_depress_chunks_batch(press.METHODS["vbe21_zd"], _p(z), _p(z), _p(z), 2, _p(rows), 4, 1, 64, 8, _p(z),
                                                           _p(z), _p(z), 256, _p(RULE), _p(z), _p(z), 1)
    for k in (1, 2, 4):
        assert call(d_rows[k:]) == EARG and "aligned" in press.last_error()
    assert lib.press_hip_depress_chunks_batch(press.METHODS["vbe21_zd"], None, None, None, 0, None, 0, 1, 64, 8, None, None, None, 0,
                                              _p(RULE), None, None, 0) == 0
    torch.cuda.synchronize()
    assert (d_rows.cpu().numpy().view(np.uint16) == CANARY[2]).all()


# ------------------------------------------------------------------ 11: host buffers

@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "rc_vbe21_zd"])
@pytest.mark.parametrize("pinned", [False, True])
def test_host_path(lib, oracle, m, pinned):
    """the written prefix of the rows arrives and nothing behind it; q and out_n come back; a row_first that is not the
    plan's is refused; the wrapper"""
    bat = dict(L.battery())

    def alloc(a):
        if not pinned:
            return a
        p = lib.press_hip_host_alloc(a.nbytes)
        assert p
        PINNED.append(p)
        v = np.frombuffer((ctypes.c_uint8 * a.nbytes).from_address(p), dtype=a.dtype)
        v[:] = a
        return v
    T, ov = 64, 8
    c = Case(oracle, m, [bat[k] for k in HOST_READS], 17)
    first, _, _ = plan_ref(c.rooms, T, ov)
    planned = int(first[-1])
    for dtype, rule, cap in (("float16", RULE, planned + 2), ("float32", None, planned), ("bfloat16", RULE, planned // 2)):
        es = ES[dtype]
        rows = alloc(np.full((cap + GUARD) * T, CANARY[es], dtype=np.uint32 if es == 4 else np.uint16))
        out_n = np.full(len(c.rooms), 7, dtype=np.uint32)
        q = np.full((len(c.rooms) + 4, 2), Q_FILL, dtype=np.int32)
        assert chunks_call(lib, m, c.inb, c.in_off, c.in_len, rows, cap, dtype, T, ov, first, c.off, c.rooms, c.total, rule, q, out_n,
                           False) == 0, press.last_error()
        assert (q[len(c.rooms):] == Q_FILL).all()
        check((m, dtype), c.expect, c.rooms, T, ov, dtype, rule, np.asarray(rows).reshape(-1, T), out_n, q[:len(c.rooms)], cap)
    wrong = first.copy()
    wrong[3] += 1
    rows = np.full(planned * T, CANARY[2], dtype=np.uint16)
    assert chunks_call(lib, m, c.inb, c.in_off, c.in_len, rows, planned, "float16", T, ov, wrong, c.off, c.rooms, c.total, RULE, None,
                       out_n, False) == EARG and "row_first" in press.last_error()
    assert (rows == CANARY[2]).all()
    if pinned:
        return
    rows, q, rr, rs, w_on = press.depress_chunks_batch_host(m, c.streams, c.rooms, T, ov, "bfloat16", RULE)
    assert rows.dtype == np.uint16 and rows.shape == (planned, T) and np.array_equal(rr, plan_ref(c.rooms, T, ov)[1])
    assert np.array_equal(rs, plan_ref(c.rooms, T, ov)[2])
    assert w_on.dtype == np.uint32 and np.array_equal(w_on, out_n)  # (the C call above, on the same batch)
    check((m, "wrapper"), c.expect, c.rooms, T, ov, "bfloat16", RULE, np.concatenate([rows, np.full((1, T), CANARY[2], dtype=np.uint16)]),
          w_on, q, planned)


# ------------------------------------------------------------------ 12: a BLOW5 file end to end

@gpu
def test_blow5_end_to_end(lib):
    """three-reads.blow5 -> next_batch -> depress_chunks_batch_host and the device-resident wrapper: the definition over
    the reference's decode of the file (three_reads.i16.bin)"""
    meta = json.load(open(os.path.join(GOLD, "three_reads.json")))["reads"]
    raw = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    want, at = {}, 0
    for r in meta:
        want[r["read_id"]] = raw[at:at + r["n"]]
        at += r["n"]
    rd = press.Blow5Reader(os.path.join(GOLD, "three-reads.blow5"))
    batch = rd.next_batch()
    rd.close()
    assert len(batch) == 3
    T, ov = 1024, 104
    ns = np.array([n for _, n, _ in batch], dtype=np.uint32)
    expect = [("ok", want[rid]) for rid, _, _ in batch]
    assert [len(w) for _, w in expect] == ns.tolist()
    rows, q, rr, rs, on = press.depress_chunks_batch_host("slow5_svb_zd", [s for _, _, s in batch], ns, T, ov, "float16", RULE)
    assert rows.dtype == np.float16 and rows.shape[1] == T and on.tolist() == ns.tolist()
    wq, cal = calibration([w for _, w in expect], RULE)
    exp, wrr = rows_ref([w for _, w in expect], ns, T, ov, "float16", cal)
    assert np.array_equal(q, wq) and np.array_equal(rr, wrr) and np.array_equal(rows.view(np.uint16), exp)
    # device resident, through the wrapper, bfloat16
    inb, in_off, in_len = L.scatter_streams(np.random.default_rng(3), [s for _, _, s in batch])
    off, total = L.scatter_rooms(np.random.default_rng(4), ns)
    first, _, _ = press.chunk_plan(ns, T, ov)
    d_rows = torch.zeros((int(first[-1]), T), dtype=torch.bfloat16, device="cuda")
    d_on = torch.zeros(3, dtype=torch.int32, device="cuda")
    d_q = torch.zeros(6, dtype=torch.int32, device="cuda")
    press.depress_chunks_batch("slow5_svb_zd", _t(inb), _t(in_off, np.int64), _t(in_len, np.int64), d_rows, _t(first, np.int64),
                               _t(off, np.int64), _t(ns, np.int32), total, d_on, ov, RULE, d_q)
    torch.cuda.synchronize()
    assert list(d_on.cpu().numpy()) == list(ns) and np.array_equal(d_q.cpu().numpy().reshape(-1, 2), wq)
    got = d_rows.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, rows_ref([w for _, w in expect], ns, T, ov, "bfloat16", cal)[0])


# ------------------------------------------------------------------ 13: the call only enqueues

HOLD_MS = 50.0


@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "shuffman_vbe21_zd", "rc_vbe21_zd"])
def test_only_enqueues_behind_a_hold(lib, oracle, m):
    """on a torch side stream that is held for 50 ms (tests/test_stream_contract.py's device): the device-resident call
    returns with the hold still pending, and the results are exact afterwards.  (The zstd kinds wait for the host, as
    documented, and are not asked.)"""
    torch.cuda._sleep(100000)
    torch.cuda.synchronize()
    cycles = 2000000
    for _ in range(3):  # torch.cuda._sleep's unit, measured with two events
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 5.0:
            break
        cycles *= 10
    assert ms >= 5.0
    c = shape_case(oracle, m, 64, 5)
    d = Dev(c)
    d.run(lib, 64, 5, "float16", RULE)  # (scratch is reserved, the table is on the device: what follows allocates nothing)
    first, _, _ = plan_ref(c.rooms, 64, 5)
    planned = int(first[-1])
    d.run(lib, 64, 5, "float16", RULE, enqueue_only=True)
    s = torch.cuda.Stream()
    assert lib.press_hip_set_stream(ctypes.c_void_p(s.cuda_stream)) == 0
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(HOLD_MS * cycles / ms))
            e = torch.cuda.Event()
            e.record(s)
            d.enqueue(lib, 64, 5, "float16", RULE, planned + 2)
            assert not e.query(), "a call that promises only to enqueue waited for the stream (or the delay of %g ms ended early)" % HOLD_MS
        s.synchronize()
        assert e.query()
    finally:
        press.use_torch_stream()
    rows, out_n, q, _ = d.fetch()
    check((m,), c.expect, c.rooms, 64, 5, "float16", RULE, rows, out_n, q, planned + 2)
