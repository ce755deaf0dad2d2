"""Range statistics on the device (include/press_hip.h, "Range statistics and the prefix"):
press_hip_signal_range_stats against the definition - the mean and the deviation by bit pattern, which is what shows the
order of the sums, the median with ==.

The yardstick is a numpy restatement with one dtype per operation (the sequential sums of tests/test_signal_segments.py)
and the median as a selection among the SAMPLES.  It is pinned to the reference: tests/golden/sigtk_prefix.json holds what
sigtk's stat_func and prefix_func, compiled as they are, give for the three real reads and every non-empty read of
_layouts.battery() under two calibrations (tests/golden/make_prefix_golden.py), and the yardstick must reproduce every
number of it.  tests/test_signal_prefix.py holds the prefix call's tests and shares this module's helpers.
"""
import ctypes
import json
import os
import time

import numpy as np
import pytest

import _layouts as L
import test_signal_segments as TSS
from honours_amd import press

gpu = pytest.mark.gpu
GOLD = TSS.GOLD
EARG = -2
F32 = np.float32
bits, bits_f32, one_nan = TSS.bits, TSS.bits_f32, TSS.one_nan
GUARD, CANARY32 = TSS.GUARD, TSS.CANARY32
NAN3 = (F32(np.nan), F32(np.nan), F32(0))


# ------------------------------------------------------------------ the yardstick

def yard_x(s, cal):
    """meani16's (float) s, or signal_in_picoamps' ((float) s + offset) * scale: no clamp"""
    s = np.asarray(s, dtype=np.int16)
    if cal is None:
        return s.astype(F32)
    with np.errstate(all="ignore"):
        return ((s.astype(F32) + F32(cal[0])) * F32(cal[1])).astype(F32)


def clamp_range(n, rg):
    if rg is None:
        return 0, n
    b = min(int(rg[1]), n)
    return min(int(rg[0]), b), b


def seq_sum(v):
    """`float sum = 0; for (...) sum += x[i];` - from +0, so a range of nothing but -0 sums to +0 (a cumsum from x[0] on
    would give -0 there, and the same value everywhere else)"""
    return np.cumsum(np.concatenate([np.zeros(1, dtype=F32), np.asarray(v, dtype=F32)]), dtype=F32)[-1]


def yard_range(s, cal, rg=None, total=seq_sum):
    """-> (mean, stdv, median) of the samples [a, b) of s, float32 each"""
    a, b = clamp_range(len(s), rg)
    if b == a:
        return NAN3
    part = np.asarray(s[a:b], dtype=np.int16)
    mean, sd = TSS.yard_mean_sd(yard_x(part, cal), total)
    srt = np.sort(part)
    k = len(part) // 2
    sel = srt[len(part) - 1 - k] if cal is not None and F32(cal[1]) < 0 else srt[k]
    return mean, sd, yard_x([sel], cal)[0]


def stat_bits(want):
    """[(mean, stdv, median)] -> uint32 [k, 3], every NaN as one pattern"""
    return one_nan(np.array([[bits(v) for v in w] for w in want], dtype=np.uint32).reshape(-1, 3))


def same_stats(got, want, what=""):
    """got: uint32 bits [k, 3]; want: [(mean, stdv, median)].  Mean and deviation by bit pattern; the median with =="""
    got = one_nan(np.asarray(got, dtype=np.uint32).reshape(-1, 3))
    wb = stat_bits(want)
    bad = np.nonzero((got[:, :2] != wb[:, :2]).any(axis=1))[0]
    assert not len(bad), (what, "mean / stdv", bad[:8].tolist(), got[bad[:4]].tolist(), wb[bad[:4]].tolist())
    gm, wm = got[:, 2].view(F32), wb[:, 2].view(F32)
    ok = (gm == wm) | (np.isnan(gm) & np.isnan(wm))
    assert ok.all(), (what, "median", np.nonzero(~ok)[0][:8].tolist(), gm[~ok][:4].tolist(), wm[~ok][:4].tolist())


# ------------------------------------------------------------------ inputs

_doc = {}


def fixture():
    if not _doc:
        _doc.update(json.load(open(os.path.join(GOLD, "sigtk_prefix.json"))))
    return _doc


def fixture_cals():
    """the two calibrations as (offset, scale) float32 pairs, in the fixture's order"""
    return [(F32(c["offset"]), F32(c["range"] / c["digitisation"])) for c in fixture()["calibrations"]]


def entries_of(cal):
    key = [bits(cal[0]), bits(cal[1])]
    return [e for e in fixture()["entries"] if e["cal_bits"] == key]


def f3(b):
    return tuple(bits_f32(v) for v in b)


def rand_read(rng, n, lo=-32768, hi=32768):
    return rng.integers(lo, hi, size=n).astype(np.int16)


L_SHAPES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4097)
STARTS = (0, 1, 3, 5, 8, 13)


def shape_cases():
    """-> (reads, ranges): every L of L_SHAPES at every start of STARTS, the range ending at n or 7 samples before it"""
    rng = np.random.default_rng(630)
    reads, ranges = [], []
    for k, ln in enumerate(L_SHAPES):
        for j, a in enumerate(STARTS):
            tail = 0 if (k + j) % 2 else 7
            reads.append(L._walk(rng, a + ln + tail) if (k + j) % 3 else rand_read(rng, a + ln + tail))
            ranges.append((a, a + ln))
    return reads, ranges


def ex1_read():
    return TSS.named_reads()["battery/ex1-32767"]


# ------------------------------------------------------------------ without a GPU

@pytest.fixture(scope="module")
def cpu_lib():
    from honours_amd import build
    build.build()
    return press.load_library()


def test_yardstick_equals_the_reference():
    """every statistic of sigtk_prefix.json: the whole read in both domains (stat_func), the adaptor's and the poly-A's
    stretch in picoamperes (prefix_func -p) - mean and deviation by bit pattern, medians with =="""
    reads = TSS.named_reads()
    ent = fixture()["entries"]
    assert len(ent) == 29 * 2 and len(reads) == 29
    nranges = 0
    for e in ent:
        s = reads[e["name"]]
        assert len(s) == e["n"]
        cal = f3(e["cal_bits"])
        m, sd, med = yard_range(s, None)
        assert [bits(m), bits(sd)] == e["raw_stat"][:2] and med == F32(e["raw_stat"][2]), e["name"]
        same_stats([e["pa_stat"]], [yard_range(s, cal)], e["name"])
        for pos, st in ((e["adapt"], e["adapt_stat"]), (e["polya"], e["polya_stat"])):
            assert (st is not None) == (pos[1] > 0)
            if st is not None:
                same_stats([st], [yard_range(s, cal, pos)], (e["name"], pos))
                x = yard_x(s[pos[0]:pos[1]], cal)  # the selection among samples is medianf's among floats
                assert np.sort(x)[len(x) // 2] == bits_f32(st[2])
                nranges += 1
    assert nranges == 2 * 13 + 6 + 5


def test_negative_scale_median_is_the_floats():
    """x falls as s rises under a negative scale: the L / 2-th largest sample gives the L / 2-th smallest float"""
    rng = np.random.default_rng(7)
    for n in (1, 2, 5, 64, 257, 1000):
        s = rand_read(rng, n, -3000, 3000)
        for cal in ((F32(12.5), F32(-0.25)), (F32(-40), F32(0.125))):
            x = yard_x(s, cal)
            assert np.sort(x)[n // 2] == yard_range(s, cal)[2]


def test_pairwise_sums_give_other_bits():
    """a pairwise float32 sum (np.sum) gives another mean than the in-order one on fixture ranges of both domains: the
    order of the sums is under test"""
    reads = TSS.named_reads()
    differ = {"raw": 0, "pa": 0}
    pw = lambda v: np.sum(v, dtype=F32)
    for e in fixture()["entries"]:
        s = reads[e["name"]]
        differ["raw"] += bits(yard_range(s, None, None, pw)[0]) != e["raw_stat"][0]
        if e["adapt_stat"] is not None:
            differ["pa"] += bits(yard_range(s, f3(e["cal_bits"]), e["adapt"], pw)[0]) != e["adapt_stat"][0]
    assert differ["raw"] >= 1 and differ["pa"] >= 1, differ
    assert float(np.cumsum(TSS.near_1200_read().astype(np.float64))[-1]) > 2 ** 24


def test_symbols_and_header(cpu_lib):
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "press_hip.h")).read()
    for s in ("press_hip_signal_range_stats", "press_hip_prefix_params_preset", "press_hip_signal_prefix",
              "press_hip_signal_prefix_workspace_bytes"):
        assert hasattr(cpu_lib, s) and s in press.HEADER_SYMBOLS and s + "(" in header, s
    for t in ("press_hip_range_stat;", "press_hip_prefix_params;", "press_hip_prefix;"):
        assert t in header
    assert press.RANGE_STAT_DTYPE.itemsize == 12 and press.PREFIX_DTYPE.itemsize == 16
    assert ctypes.sizeof(press.PrefixParams) == 20 + 32 + 12


def test_bad_arguments(cpu_lib):
    """a NULL argument other than cal and range is PRESS_HIP_EARG before any device call: the same with and without a
    device"""
    a = np.zeros(64, dtype=np.uint64)
    p = a.ctypes.data
    for dr in (0, 1):
        # sig off n nreads total cal range out
        args = [p, p, p, 1, 8, p, p, p]
        for k in (0, 1, 2, 7):
            bad = list(args)
            bad[k] = None
            assert cpu_lib.press_hip_signal_range_stats(*bad, dr) == EARG, (k, dr)
            assert "NULL" in press.last_error()
    assert cpu_lib.press_hip_signal_range_stats(p + 2, p, p, 1, 8, None, None, p, 1) == EARG and "aligned" in press.last_error()


# ------------------------------------------------------------------ GPU plumbing

@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.use_torch_stream()
    yield lb
    torch.cuda.synchronize()
    press.use_torch_stream()
    torch.cuda.empty_cache()


_t = TSS._t


class RDev:
    """a batch on the device in a scattered layout; the outputs of both calls between canaries"""

    def __init__(self, reads, cals=None, seed=1):
        rng = np.random.default_rng(seed)
        self.reads, self.nr = reads, len(reads)
        sig, off = L.scatter_reads(rng, reads)
        self.sig, self.off = _t(sig), _t(off, np.int64)
        self.n = _t(np.array([len(r) for r in reads], dtype=np.uint32), np.int32)
        self.cal = None if cals is None else _t(np.array(cals, dtype=F32).reshape(-1))

    @staticmethod
    def room(words):
        import torch
        return torch.full((words + 2 * GUARD,), CANARY32, dtype=torch.int32, device="cuda")

    @staticmethod
    def inside(t, words, what):
        h = t.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == CANARY32).all() and (h[GUARD + words:] == CANARY32).all(), what
        return h[GUARD:GUARD + words].copy()

    def stats(self, ranges=None, raw=False):
        """-> uint32 bits [nr, 3]; the canaries around out are checked"""
        import torch
        out = self.room(3 * self.nr)
        rg = None if ranges is None else _t(np.array(ranges, dtype=np.uint32).reshape(-1), np.int32)
        press.range_stats(self.sig, self.off, self.n, None if raw else self.cal, rg,
                          out[GUARD:GUARD + 3 * self.nr].view(torch.float32))
        torch.cuda.synchronize()
        return self.inside(out, 3 * self.nr, "out").reshape(-1, 3)


def wants(reads, cals, ranges):
    return [yard_range(s, None if cals is None else cals[r], None if ranges is None else ranges[r]) for r, s in enumerate(reads)]


# ------------------------------------------------------------------ on the GPU

@gpu
def test_fixture_batches(lib):
    """the fixture's reads as one batch per calibration, device resident and with host pointers: the whole reads in both
    domains (sigtk stat's six columns) and the fixture's adaptor and poly-A stretches, against the reference's numbers"""
    named = TSS.named_reads()
    for cal in fixture_cals():
        ent = entries_of(cal)
        reads = [named[e["name"]] for e in ent]
        cals = [cal] * len(reads)
        d = RDev(reads, cals, seed=3)
        raw_want = [(bits_f32(e["raw_stat"][0]), bits_f32(e["raw_stat"][1]), F32(e["raw_stat"][2])) for e in ent]
        pa_want = [f3(e["pa_stat"]) for e in ent]
        same_stats(d.stats(raw=True), raw_want, "raw")
        same_stats(d.stats(), pa_want, "pa")
        same_stats(press.range_stats_host(reads).view(np.uint32), raw_want, "raw, host")
        same_stats(press.range_stats_host(reads, np.array(cals)).view(np.uint32), pa_want, "pa, host")
        table = press.signal_stat_table(d.sig, d.off, d.n, d.cal).cpu().numpy()
        assert table.shape == (len(reads), 6)
        same_stats(table[:, 0::2].copy().view(np.uint32), raw_want, "table, raw")
        same_stats(table[:, 1::2].copy().view(np.uint32), pa_want, "table, pa")
        for key in ("adapt", "polya"):
            ranges = [e[key] if e[key][1] > 0 else [0, 0] for e in ent]
            want = [f3(e[key + "_stat"]) if e[key][1] > 0 else NAN3 for e in ent]
            same_stats(d.stats(ranges), want, key)
            same_stats(press.range_stats_host(reads, np.array(cals), np.array(ranges)).view(np.uint32), want, key + ", host")
    assert len(press.range_stats_host([])) == 0


@gpu
def test_range_shapes(lib):
    """L across the tile (64), the load group (256) and several groups, at starts that are odd and at off[r] + a that is
    no multiple of 8, ranges ending at n and before it, in both domains"""
    reads, ranges = shape_cases()
    assert any(a % 2 for a, _ in ranges) and any(b == len(s) for s, (_, b) in zip(reads, ranges))
    cals = [(F32(-3.5 - r), F32(0.17 + 0.01 * r)) for r in range(len(reads))]
    d = RDev(reads, cals, seed=4)
    assert any((int(o) + a) % 8 for o, (a, _) in zip(d.off.cpu().numpy(), ranges))
    same_stats(d.stats(ranges, raw=True), wants(reads, None, ranges), "raw")
    same_stats(d.stats(ranges), wants(reads, cals, ranges), "pa")
    same_stats(press.range_stats_host(reads, np.array(cals), np.array(ranges)).view(np.uint32), wants(reads, cals, ranges), "host")


@gpu
def test_clamped_ranges_and_empty_reads(lib):
    """b > n and a > b are clamped, a read of 0 samples is an empty range: NaN, NaN, 0"""
    rng = np.random.default_rng(631)
    reads = [rand_read(rng, n) for n in (100, 0, 257, 64, 0, 1, 300)]
    ranges = [(10, 5000), (0, 10), (300, 200), (64, 0xFFFFFFFF), (0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (299, 1 << 31)]
    d = RDev(reads, None, seed=5)
    got = d.stats(ranges, raw=True)
    same_stats(got, wants(reads, None, ranges))
    assert np.isnan(got[[1, 2, 3, 4, 5], :2].view(F32)).all() and not got[[1, 2, 3, 4, 5], 2].any()
    same_stats(d.stats(None, raw=True), wants(reads, None, None), "whole reads")


@gpu
def test_ragged_batch(lib):
    """130 reads of ragged lengths, a range each, and the whole reads: the raw median of a whole read is
    press_hip_signal_stats' median"""
    import torch
    rng = np.random.default_rng(632)
    ns = [int(v) for v in rng.integers(0, 700, size=130)]
    ns[7], ns[99] = 0, 2600
    reads = [L._walk(rng, n, exr=0.02) for n in ns]
    ranges = [(int(rng.integers(0, n + 2)), int(rng.integers(0, n + 9))) for n in ns]
    cals = [(F32(rng.uniform(-300, 50)), F32(rng.uniform(0.1, 0.4) * (-1 if r % 5 == 0 else 1))) for r in range(130)]
    d = RDev(reads, cals, seed=6)
    same_stats(d.stats(ranges), wants(reads, cals, ranges), "pa")
    whole = d.stats(None, raw=True)
    same_stats(whole, wants(reads, None, None), "raw, whole")
    st = torch.zeros(2 * 130, dtype=torch.int32, device="cuda")
    press.signal_stats(d.sig, d.off, d.n, st)
    med = st.cpu().numpy().reshape(-1, 2)[:, 0]
    full = np.array(ns) > 0
    assert np.array_equal(whole[full, 2].view(F32), med[full].astype(F32))


@gpu
def test_median_keys(lib):
    """all keys equal; two values with the rank on either side of their boundary; -32768 and 32767 present; even and odd
    L; a negative and a zero scale"""
    lo, hi = np.int16(-32768), np.int16(32767)
    reads, cals = [], []
    for ln in (1, 2, 7, 64, 129, 1000, 1001):
        reads.append(np.full(ln, -7, dtype=np.int16))
        k = ln // 2
        reads.append(np.array([hi] * k + [lo] * (ln - k), dtype=np.int16))            # the rank is the first of the high value
        reads.append(np.array([hi] * (ln - k - 1) + [lo] * (k + 1), dtype=np.int16))  # ... the last of the low value
        reads.append(np.array([256] * k + [255] * (ln - k), dtype=np.int16))          # keys that differ in both digits
        reads.append(np.array([-1, 0] * ln, dtype=np.int16)[:ln])
    rng = np.random.default_rng(633)
    reads = [rng.permutation(r) for r in reads]
    for r in range(len(reads)):
        cals.append(((F32(3.0), F32(0.25)), (F32(3.0), F32(-0.25)), (F32(-1.5), F32(0.0)), (F32(-1.5), F32(-0.0)))[r % 4])
    d = RDev(reads, cals, seed=7)
    raw = d.stats(raw=True)
    same_stats(raw, wants(reads, None, None), "raw")
    assert {float(v) for v in raw[:, 2].view(F32)} >= {-32768.0, 32767.0, -7.0, 255.0, 256.0, -1.0, 0.0}
    same_stats(d.stats(), wants(reads, cals, None), "pa")
    cals2 = cals[1:] + cals[:1]
    same_stats(RDev(reads, cals2, seed=8).stats(), wants(reads, cals2, None), "pa, the scales shifted by one read")


@gpu
def test_sums_that_round(lib):
    """a raw read whose sample sum passes 2^24, and a picoampere range of an ex1 read (exceptions of +-30000 among small
    values): the in-order sums, which a pairwise sum does not reproduce"""
    reads = [TSS.near_1200_read(), ex1_read()]
    cal = fixture_cals()[0]
    ranges = [(0, len(reads[0])), (6649, 13058)]
    pw = lambda v: np.sum(v, dtype=F32)
    assert bits(yard_range(reads[0], None, ranges[0], pw)[0]) != bits(yard_range(reads[0], None, ranges[0])[0])
    assert bits(yard_range(reads[1], cal, ranges[1], pw)[0]) != bits(yard_range(reads[1], cal, ranges[1])[0])
    d = RDev(reads, [cal, cal], seed=9)
    same_stats(d.stats(ranges, raw=True), wants(reads, None, ranges), "raw")
    same_stats(d.stats(ranges), wants(reads, [cal, cal], ranges), "pa")


@gpu
def test_repeatable_behind_scratch_fill(lib):
    """the results do not depend on what the library's scratch held: equal behind press.scratch_fill of two byte values"""
    import torch
    reads, ranges = shape_cases()
    cals = [(F32(2.0), F32(0.2))] * len(reads)
    d = RDev(reads, cals, seed=10)
    got = []
    for byte in (0x00, 0xFF):
        torch.cuda.synchronize()
        press.scratch_fill(byte)
        got.append((d.stats(ranges), press.range_stats_host(reads, np.array(cals), np.array(ranges)).view(np.uint32).reshape(-1, 3)))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(one_nan(got[0][0]), one_nan(got[0][1]))


@gpu
def test_stream_contract(lib):
    """device resident, on a side stream behind a delay: the call returns while the delay is pending - it only enqueues -
    and its results are those of the same call made with nothing pending (as tests/test_signal_segments.py measures it)"""
    import torch
    reads, ranges = shape_cases()
    cals = [(F32(2.0), F32(0.2))] * len(reads)
    d = RDev(reads, cals, seed=11)
    rg = _t(np.array(ranges, dtype=np.uint32).reshape(-1), np.int32)
    out = torch.zeros((len(reads), 3), dtype=torch.float32, device="cuda")
    raw = torch.zeros((len(reads), 3), dtype=torch.float32, device="cuda")

    def calls():
        press.range_stats(d.sig, d.off, d.n, d.cal, rg, out)
        press.range_stats(d.sig, d.off, d.n, None, None, raw)

    behind_a_delay(lib, calls, (out, raw), "range_stats")
    same_stats(out.cpu().numpy().view(np.uint32), wants(reads, cals, ranges))
    same_stats(raw.cpu().numpy().view(np.uint32), wants(reads, None, None))


def behind_a_delay(lib, calls, outputs, what, hold_ms=50.0):
    """calls() on a side stream behind a delay of hold_ms: it must return while the delay is pending"""
    import torch
    torch.cuda._sleep(100000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(20000000)
    b.record()
    b.synchronize()
    cycles = int(hold_ms * 20000000 / a.elapsed_time(b))
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0 and lib.press_hip_set_stream(ctypes.c_void_p(s.cuda_stream)) == 0
    try:
        with torch.cuda.stream(s):
            calls()  # (scratch reserved: nothing left to allocate)
        s.synchronize()
        for o in outputs:
            o.zero_()
        torch.cuda.synchronize()
        e = torch.cuda.Event()
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            e.record(s)
            calls()
        t1 = time.perf_counter()
        assert not e.query(), "a call that promises only to enqueue waited for the stream (or the delay ended early)"
        assert (t1 - t0) * 1e3 < hold_ms / 2
        s.synchronize()
        assert e.query()
        print("%s: %.3f ms of host time behind a delay of %g ms" % (what, (t1 - t0) * 1e3, hold_ms))
    finally:
        torch.cuda.synchronize()
        press.use_torch_stream()


@gpu
def test_nan_and_inf_calibrations(lib):
    """cal is not validated: NaN and inf go through the definition, nothing faults and nothing outside out is written"""
    rng = np.random.default_rng(634)
    reads = [L._walk(rng, n) for n in (900, 64, 2500, 129, 301, 77)]
    cals = [(F32(np.nan), F32(0.18)), (F32(6.0), F32(np.inf)), (F32(3e38), F32(3e38)), (F32(-np.inf), F32(-1.0)),
            (F32(1.0), F32(np.nan)), (F32(2.0), F32(-np.inf))]
    got = RDev(reads, cals, seed=12).stats()
    same_stats(got, wants(reads, cals, None))
    assert np.isnan(got[0].view(F32)).all() and np.isnan(got[4].view(F32)).all()
