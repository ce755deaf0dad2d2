"""Dataset analysis on the device (include/press_hip.h, "Dataset analysis"): press_hip_signal_tally against
its definition, exactly - the value table, the delta table, the 257 x 257 transition table and the per-read moments.

The yardstick is the definition restated in numpy.  It must reproduce every entry of tests/golden/viz_tally.json, which the
REAL reference wrote (tests/golden/make_tally_golden.py: viz/tally.c's printtally over the loops of freq_slow5.c and
freq_delta_slow5.c, get_exceptions.c's count, press/stats.c's get_stats).  The reference has no counterpart of the
transition table at 257 classes: the restatement here is its definition.

The one tolerance: mean and variance from exact integers are the correctly rounded values, the reference's Welford
recurrence in double is not.  Its error is bounded by a small multiple of n * 2^-53 * sqrt(1 + mean^2 / var); the test asserts
rel <= 4 * n * 2^-53 * sqrt(1 + mean^2 / var) per read and equality where var == 0.
"""
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import _layouts as L
import test_range_stats as TRS
import test_signal_segments as TSS
from honours_amd import press

gpu = pytest.mark.gpu
EARG = -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BINS, SYMS = 65536, 257
CANARY = 0x5AC35AC35AC35AC3
GUARD = 64
EDGES = (0, 1, 2, 7, 8, 9, 511, 512, 513, 8191, 8192, 8193, 32767, 32768, 32769, 65537)


# ------------------------------------------------------------------ the yardstick

def zz(v):
    v = np.asarray(v).astype(np.int16).astype(np.int32)
    return ((v << 1) ^ (v >> 15)) & 0xFFFF


def deltas(s):
    s = np.asarray(s, dtype=np.int16).astype(np.int32)
    return (s[1:] - s[:-1]).astype(np.int16)


def yard_tally(reads):
    """-> dict raw, delta (uint64[65536]), trans (uint64[257, 257]), mom (MOMENTS_DTYPE[nreads])"""
    raw = np.zeros(BINS, dtype=np.uint64)
    delta = np.zeros(BINS, dtype=np.uint64)
    trans = np.zeros(SYMS * SYMS, dtype=np.uint64)
    mom = np.zeros(len(reads), dtype=press.MOMENTS_DTYPE)
    for r, s in enumerate(reads):
        s = np.asarray(s, dtype=np.int16)
        raw += np.bincount(zz(s), minlength=BINS).astype(np.uint64)
        zd = zz(deltas(s))
        delta += np.bincount(zd, minlength=BINS).astype(np.uint64)
        sym = np.minimum(zd, 256)
        trans += np.bincount(257 * sym[:-1] + sym[1:], minlength=SYMS * SYMS).astype(np.uint64)
        w = s.astype(np.int64)
        mom[r] = (int(w.sum()), int((w * w).sum()), int(w.min()) if len(s) else 32767, int(w.max()) if len(s) else -32768, len(s),
                  int((zd > 255).sum()))
    return {"raw": raw, "delta": delta, "trans": trans.reshape(SYMS, SYMS), "mom": mom}


def symbol_counts_of(reads):
    """press_hip_symbol_counts' definition (tests/test_table_training.py pins the device to it)"""
    c = np.zeros(257, dtype=np.uint64)
    for s in reads:
        c += np.bincount(np.minimum(zz(deltas(s)), 256), minlength=257).astype(np.uint64)
    return c


_cache = {}


def fixture():
    if "fx" not in _cache:
        _cache["fx"] = json.load(open(os.path.join(GOLD, "viz_tally.json")))
    return _cache["fx"]


def fixture_set(name):
    st = [s for s in fixture()["sets"] if s["name"] == name][0]
    named = TSS.named_reads()
    reads = [named[e["name"]] if e["n"] else np.zeros(0, dtype=np.int16) for e in st["reads"]]
    return st, reads


def yard_of(key, reads):
    """yard_tally once per key: shared by the tests, never changed"""
    if key not in _cache:
        y = yard_tally(reads)
        for a in y.values():
            a.setflags(write=False)
        _cache[key] = y
    return _cache[key]


def table_of_rows(rows):
    t = np.zeros(BINS, dtype=np.uint64)
    for v, c in rows:
        t[int(zz(np.array([v]))[0])] = c
    return t


def edge_reads(seed=7):
    rng = np.random.default_rng(seed)
    return [L._walk(rng, n, 0.01) for n in EDGES]


def ragged_reads(count=300, seed=11):
    rng = np.random.default_rng(seed)
    ns = rng.integers(0, 3000, size=count)
    ns[::37] = 0
    ns[5], ns[count // 2] = 40000, 33000
    return [L._walk(rng, int(n), 0.02) for n in ns]


def extreme_reads():
    rng = np.random.default_rng(13)
    alt = np.where(np.arange(70001) % 2 == 0, -32768, 32767).astype(np.int16)   # wrapped delta -1 / +1; raw bin 65535
    low = np.full(33001, -32768, dtype=np.int16)
    uni = rng.integers(-32768, 32768, size=100000).astype(np.int16)             # everything outside any window
    const = np.full(100000, 517, dtype=np.int16)                                # every lane on one bin
    walk = (500 + np.cumsum(rng.integers(0, 2, size=100000) * 2 - 1)).astype(np.int16)  # +-1: the core of trans only
    return [alt, low, uni, const, walk]


def same(got, want, what=""):
    for k in want:
        if k in got:
            g, w = np.asarray(got[k]), np.asarray(want[k])
            if k == "mom":
                assert g.tobytes() == w.tobytes(), (what, k, g[:4], w[:4])
            else:
                g, w = g.reshape(-1).view(np.uint64), w.reshape(-1)
                bad = np.flatnonzero(g != w)
                assert bad.size == 0, (what, k, bad[:8], g[bad[:8]], w[bad[:8]])


# ------------------------------------------------------------------ without a GPU

@pytest.fixture(scope="module")
def cpu_lib():
    import torch  # noqa: F401  (before the library, as in a run of the whole suite: the two then share one HIP runtime)
    from honours_amd import build
    build.build()
    lb = press.load_library()
    press._tally_api(lb)
    return lb


def test_yardstick_equals_the_reference():
    """every entry of viz_tally.json: both tables and printtally's text exactly, n, min, max and the exception count exactly,
    mean, var and sd from the exact integers against the reference's Welford values within the bound of the docstring"""
    worst = 0.0
    for st in fixture()["sets"]:
        st, reads = fixture_set(st["name"])
        y = yard_of("fx/" + st["name"], reads)
        assert np.array_equal(y["raw"], table_of_rows(st["raw"])) and np.array_equal(y["delta"], table_of_rows(st["delta"]))
        for k in ("raw", "delta"):
            v, c = press.tally_table(y[k])
            assert [[int(a), int(b)] for a, b in zip(v, c)] == st[k], (st["name"], k)
            assert press.tally_text(y[k]) == st[k + "_text"], (st["name"], k)
        ms = press.moments_stats(y["mom"])
        for r, e in enumerate(st["reads"]):
            m = y["mom"][r]
            assert (int(m["n"]), int(m["min"]), int(m["max"])) == (e["n"], e["min"], e["max"]), e["name"]
            if e["nex"] is not None:
                assert int(m["nex"]) == e["nex"], e["name"]
            if e["n"] == 0:
                assert int(m["nex"]) == 0 and np.isnan(ms["mean"][r]) and np.isnan(ms["var"][r])
                continue
            ref = {k: float(np.array([e[k + "_bits"]], dtype=np.uint64).view(np.float64)[0]) for k in ("mean", "var", "sd")}
            mean, var = ms["mean"][r], ms["var"][r]
            if var == 0:
                assert ref["var"] == 0 and ref["sd"] == 0 and ms["sd"][r] == 0 and mean == ref["mean"], e["name"]
                continue
            bound = 4 * e["n"] * 2.0 ** -53 * math.sqrt(1 + mean * mean / var)
            for k in ("mean", "var", "sd"):
                rel = abs(ms[k][r] - ref[k]) / abs(ref[k])
                print("%s %s: rel %.3g bound %.3g" % (e["name"], k, rel, bound))
                assert rel <= bound, (e["name"], k, rel, bound)
                worst = max(worst, rel / bound)
    print("largest ratio of the measured difference to the bound: %.3g" % worst)
    assert worst <= 1


def test_fixture_conditions():
    """the fixture holds what the issue asks of it: both sets inside the reference's domain, empty reads, a read of one
    sample, reads across a chunk boundary, reads with and without exceptions"""
    three, battery = (fixture_set(n) for n in ("three_reads", "battery"))
    assert len(three[1]) == 3 and [len(s) for s in three[1]] == [e["n"] for e in three[0]["reads"]]
    assert min(v for v, _ in three[0]["raw"]) == 253 and max(v for v, _ in three[0]["raw"]) == 697
    # (within the reads; across the two read boundaries of three_reads.i16.bin the flat file also has a step of 205)
    assert min(v for v, _ in three[0]["delta"]) == -162 and max(v for v, _ in three[0]["delta"]) == 137
    ns = [e["n"] for e in battery[0]["reads"]]
    assert len(ns) == 19 and ns.count(0) == 3 and 1 in ns and 2 in ns and max(ns) > 4 * 32768
    assert all(e["nex"] is None for e in battery[0]["reads"] if e["n"] == 0)
    assert any(e["nex"] == 0 for e in battery[0]["reads"] if e["n"] > 100) and any((e["nex"] or 0) > 100 for e in battery[0]["reads"])
    for st, reads in (three, battery):
        for s in reads:
            assert not len(s) or (-4096 <= int(s.min()) and int(s.max()) <= 4095)
            d = deltas(s)
            assert not len(d) or (-4096 <= int(d.min()) and int(d.max()) <= 4095)


def summary_by_hand(rows):
    """viz/freq_analyse.R restated independently over [(value, count)] rows in ascending value order, with fractions"""
    n = sum(c for _, c in rows)

    def q(f):
        cum = Fraction(0)
        for v, c in rows:
            cum += c
            if cum >= n * f:
                return v

    mean = sum(Fraction(v * c, n) for v, c in rows)
    var = sum((v - mean) ** 2 * c for v, c in rows) / n
    top = max(c for _, c in rows)
    import decimal
    with decimal.localcontext() as ctx:  # 50 digits: a peaked table's entropy is a sum of tiny terms, log2(c / n) near 0
        ctx.prec = 50
        ent = float(-sum(decimal.Decimal(c) / n * ((decimal.Decimal(c) / n).ln() / decimal.Decimal(2).ln()) for _, c in rows))
    return dict(n=n, min=rows[0][0], q1=q(Fraction(1, 4)), mean=float(mean), median=q(Fraction(1, 2)), q3=q(Fraction(3, 4)),
                max=rows[-1][0], mode=[v for v, c in rows if c == top][0], var=float(var), std=math.sqrt(float(var)), entropy=ent)


@pytest.mark.parametrize("rows", [
    [(-3, 5), (-1, 5), (0, 2), (4, 5), (9, 3)],              # a three-way tie for the mode: the smallest value
    [(1, 1), (2, 1), (3, 1), (4, 1)],                        # n * q lands exactly on a cumulative count for all three
    [(-32768, 2), (0, 4), (32767, 2)],                       # the extremes; q1 exactly on the first cumulative count
    [(7, 1000)],                                             # one row: entropy 0, variance 0
    [(-2, 3), (-1, 1), (5, 10 ** 12), (6, 7)],               # counts beyond 2^32
], ids=["mode-tie", "quantile-on-count", "extremes", "one-row", "large-counts"])
def test_tally_summary(rows):
    t = np.zeros(BINS, dtype=np.uint64)
    for v, c in rows:
        t[int(zz(np.array([v]))[0])] = c
    v, c = press.tally_table(t)
    assert [(int(a), int(b)) for a, b in zip(v, c)] == rows
    got, want = press.tally_summary(t), summary_by_hand(rows)
    for k in ("n", "min", "q1", "median", "q3", "max", "mode", "mean", "var"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["std"] == pytest.approx(want["std"], rel=1e-15, abs=0) and got["entropy"] == pytest.approx(want["entropy"], rel=1e-12, abs=1e-15)
    if len(rows) == 1:
        assert got["entropy"] == 0 and got["var"] == 0 and got["std"] == 0
    assert press.tally_summary(np.zeros(BINS, dtype=np.uint64))["n"] == 0


def test_transition_entropy():
    """against H(pairs) - H(rows) and the columns' entropy computed from probabilities as fractions"""
    def h(counts):
        n = sum(counts)
        return -sum(float(Fraction(c, n)) * (math.log2(c) - math.log2(n)) for c in counts if c)

    t = np.zeros((SYMS, SYMS), dtype=np.uint64)
    t[0, 0], t[0, 1], t[1, 0], t[5, 256], t[256, 5], t[256, 256] = 50, 25, 25, 7, 7, 1
    h0, h1 = press.transition_entropy(t)
    cells = [int(x) for x in t.reshape(-1) if x]
    assert h0 == pytest.approx(h([int(x) for x in t.sum(axis=0)]), rel=1e-12)
    assert h1 == pytest.approx(h(cells) - h([int(x) for x in t.sum(axis=1)]), rel=1e-12)
    one = np.zeros((SYMS, SYMS), dtype=np.uint64)
    one[3, 3] = 10 ** 13                                      # a constant stream: nothing to learn at either order
    assert press.transition_entropy(one) == (0.0, 0.0)
    iid = np.zeros((SYMS, SYMS), dtype=np.uint64)
    iid[:4, :4] = 1000                                        # independent and uniform over 4 symbols: H1 == H0 == 2
    assert press.transition_entropy(iid) == (pytest.approx(2.0, abs=1e-12), pytest.approx(2.0, abs=1e-12))
    det = np.zeros((SYMS, SYMS), dtype=np.uint64)
    det[0, 1] = det[1, 0] = 500                               # alternating: one bit at order 0, none at order 1
    assert press.transition_entropy(det) == (pytest.approx(1.0, abs=1e-12), pytest.approx(0.0, abs=1e-12))
    assert press.transition_entropy(np.zeros((SYMS, SYMS), dtype=np.uint64)) == (0.0, 0.0)


def test_moments_stats_pa():
    """the picoampere forms of viz/stats.c from the exact integers"""
    s = np.array([100, 104, 96, 100], dtype=np.int16)
    y = yard_tally([s, np.zeros(0, dtype=np.int16)])
    st = press.moments_stats(y["mom"], [[8192.0, 6.0, 1467.61], [2048.0, -243.0, 748.58]])
    k = 1467.61 / 8192.0
    assert st["mean"][0] == 100.0 and st["var"][0] == 8.0 and st["sd"][0] == math.sqrt(8.0)
    assert st["min_pa"][0] == (96 + 6.0) * k and st["max_pa"][0] == (104 + 6.0) * k and st["mean_pa"][0] == (100.0 + 6.0) * k
    assert st["var_pa"][0] == 8.0 * k ** 2 and st["sd_pa"][0] == math.sqrt(8.0 * k ** 2)
    assert np.isnan(st["mean"][1]) and np.isnan(st["var_pa"][1])


def test_symbols_header_and_mirror(cpu_lib):
    header = open(os.path.join(ROOT, "include", "press_hip.h")).read()
    for s in ("press_hip_signal_tally", "press_hip_signal_tally_workspace_bytes"):
        assert hasattr(cpu_lib, s) and s in press.HEADER_SYMBOLS and s + "(" in header, s
    assert press.MOMENTS_DTYPE.itemsize == 32 and "press_tally.hip" in __import__("honours_amd.build", fromlist=["SOURCES"]).SOURCES


def test_bad_layouts_are_refused(cpu_lib):
    """PRESS_HIP_EARG before any device call, the same with and without a device: NULL sig / off / n, a read start that is
    no multiple of 8, a read beyond total_samples, a device arena that is not 16-byte aligned.  All outputs NULL and an
    empty batch are PRESS_HIP_OK behind the checks."""
    lib = cpu_lib
    a = np.zeros(1024, dtype=np.uint64)
    p = a.ctypes.data
    off = np.array([0, 64], dtype=np.uint64)
    n = np.array([10, 20], dtype=np.uint32)
    for dr in (0, 1):
        for k in range(3):
            args = [p, off.ctypes.data, n.ctypes.data]
            args[k] = None
            assert lib.press_hip_signal_tally(*args, 2, 256, p, p, p, p, dr) == EARG and "NULL" in press.last_error(), (k, dr)
    bad_off = np.array([0, 12], dtype=np.uint64)
    assert lib.press_hip_signal_tally(p, bad_off.ctypes.data, n.ctypes.data, 2, 256, p, p, p, p, 0) == EARG
    far = np.array([0, 248], dtype=np.uint64)
    assert lib.press_hip_signal_tally(p, far.ctypes.data, n.ctypes.data, 2, 256, p, p, p, p, 0) == EARG
    assert lib.press_hip_signal_tally(p, bad_off.ctypes.data, n.ctypes.data, 2, 256, None, None, None, None, 0) == EARG
    assert lib.press_hip_signal_tally(p + 2, off.ctypes.data, n.ctypes.data, 2, 256, p, p, p, p, 1) == EARG and "aligned" in press.last_error()
    assert lib.press_hip_signal_tally(p, off.ctypes.data, n.ctypes.data, 2, 256, None, None, None, None, 0) == 0
    assert lib.press_hip_signal_tally(p, off.ctypes.data, n.ctypes.data, 2, 256, None, None, None, None, 1) == 0
    assert lib.press_hip_signal_tally(None, None, None, 0, 0, p, p, p, p, 0) == 0
    assert (a == 0).all()


def test_workspace(cpu_lib):
    """exact: 8 bytes per chunk the work list can hold and the count's 64; nothing per sample beyond that; 0 for no reads"""
    ws = press.signal_tally_workspace_bytes
    assert ws(0, 0) == 0 and ws(10 ** 6, 0) == 0
    for total, nr in ((1000, 1), (10 ** 6, 64), (930_000_000, 8192), ((1 << 31) + (1 << 20), 5)):
        assert ws(total, nr) == 8 * (total // 32768 + nr + 1) + 64, (total, nr)


# ------------------------------------------------------------------ GPU plumbing

@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press._tally_api(lb)
    press.use_torch_stream()
    yield lb
    torch.cuda.synchronize()
    press.use_torch_stream()
    torch.cuda.empty_cache()


class TDev:
    """a batch on the device in a scattered layout; the four outputs lie between canaries"""

    def __init__(self, reads, seed=1, off=None, ns=None):
        rng = np.random.default_rng(seed)
        sig, o = L.scatter_reads(rng, reads)
        ns = np.array([len(r) for r in reads], dtype=np.uint32) if ns is None else ns(reads)
        self.nr = len(ns)
        self.sig = TSS._t(sig)
        self.off = TSS._t(o if off is None else off(o), np.int64)
        self.n = TSS._t(ns, np.int32)

    def room(self, words, fill=0):
        import torch
        t = torch.full((words + 2 * GUARD,), CANARY, dtype=torch.int64, device="cuda")
        t[GUARD:GUARD + words] = fill
        return t

    def run(self, want=press.TALLY_OUTPUTS, pattern=None, times=1):
        """-> dict of the outputs asked for; the canaries around each are checked.  pattern: tables start as pattern[k]"""
        import torch
        words = {"raw": BINS, "delta": BINS, "trans": SYMS * SYMS, "mom": 4 * self.nr}
        rooms = {k: self.room(words[k], 0x7777777777777777 if k == "mom" else 0) for k in want}
        if pattern:
            for k in want:
                if k != "mom":
                    rooms[k][GUARD:GUARD + words[k]] = torch.from_numpy(pattern[k].reshape(-1).view(np.int64)).cuda()
        arg = {k: (rooms[k][GUARD:GUARD + words[k]] if k in want else None) for k in words}
        for _ in range(times):
            press.signal_tally(self.sig, self.off, self.n, arg["raw"], arg["delta"], arg["trans"], arg["mom"])
        torch.cuda.synchronize()
        out = {}
        for k in want:
            h = rooms[k].cpu().numpy().view(np.uint64)
            assert (h[:GUARD] == CANARY).all() and (h[GUARD + words[k]:] == CANARY).all(), ("canary", k)
            body = h[GUARD:GUARD + words[k]].copy()
            out[k] = body.view(press.MOMENTS_DTYPE) if k == "mom" else body.reshape(SYMS, SYMS) if k == "trans" else body
        return out


def device_symbol_counts(d):
    import torch
    counts = torch.zeros(257, dtype=torch.int64, device="cuda")
    press.symbol_counts(d.sig, d.off, d.n, counts)
    torch.cuda.synchronize()
    return counts.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ on the GPU

@gpu
@pytest.mark.parametrize("name", ["three_reads", "battery"])
def test_fixture_sets(lib, name):
    """the fixture's sets, device resident and with host pointers, against the reference's tables themselves"""
    st, reads = fixture_set(name)
    want = yard_of("fx/" + name, reads)
    got = TDev(reads, seed=31).run()
    same(got, want, name)
    assert np.array_equal(got["raw"], table_of_rows(st["raw"])) and np.array_equal(got["delta"], table_of_rows(st["delta"]))
    assert press.tally_text(got["raw"]) == st["raw_text"] and press.tally_text(got["delta"]) == st["delta_text"]
    assert [int(x) for x in got["mom"]["nex"]] == [e["nex"] or 0 for e in st["reads"]]
    same(press.signal_tally_host(reads), want, name + " host")


@gpu
def test_boundary_lengths(lib):
    """lengths around the lane, sub-tile, wave-quarter and chunk boundaries in one ragged batch"""
    reads = edge_reads()
    same(TDev(reads, seed=32).run(), yard_of("edges", reads), "edges")


@gpu
def test_single_delta_at_each_boundary(lib):
    """a read whose only non-zero delta sits at each boundary index in turn: it is counted once, in the right read, and the
    transitions into and out of it are the only ones off (0, 0)"""
    reads = []
    for i in EDGES:
        if i == 0:
            continue
        s = np.full(65539, 300, dtype=np.int16)
        s[i:] = 340                                           # d[i] = 40: zz 80, inside every window
        reads.append(s)
        t = np.full(65539, 300, dtype=np.int16)
        t[i:] = -3000                                         # d[i] = -3300: an exception, outside every window
        reads.append(t)
    want = yard_of("single", reads)
    got = TDev(reads, seed=33).run()
    same(got, want, "single")
    assert int(got["delta"][80]) == len(reads) // 2 and int(got["delta"][6599]) == len(reads) // 2
    assert [int(x) for x in got["mom"]["nex"]] == [0, 1] * (len(reads) // 2)


@gpu
def test_ragged_batch(lib):
    reads = ragged_reads()
    same(TDev(reads, seed=34).run(), yard_of("ragged", reads), "ragged")


@gpu
def test_extremes(lib):
    """-32768 / 32767 alternating, all -32768, uniform int16 (outside every window), a constant read and a +-1 walk (every
    lane on one counter)"""
    reads = extreme_reads()
    want = yard_of("extremes", reads)
    assert int(want["raw"][65535]) > 0 and int(want["delta"][1]) >= 35000 and int(want["trans"][256, 256]) > 90000
    same(TDev(reads, seed=35).run(), want, "extremes")
    for k, s in enumerate(reads):                             # and each alone: nothing leans on a neighbour in the batch
        same(TDev([s], seed=36 + k).run(), yard_of("extreme-%d" % k, [s]), "extreme-%d" % k)


@gpu
def test_window_boundaries(lib):
    """values on both sides of every LDS window's edge, in random order so that every pair of them follows another: the
    counters' indices 8191 / 8192 (raw), 1023 / 1024 (delta), symbols 159 / 160 / 161 and 255 / 256 (trans)"""
    rng = np.random.default_rng(51)
    unzz = lambda z: (z >> 1) ^ -(z & 1)
    zs = np.array([0, 1, 2, 158, 159, 160, 161, 162, 254, 255, 256, 257, 1022, 1023, 1024, 1025, 8190, 8191, 8192, 8193, 65535])
    steps = unzz(rng.choice(zs, size=50000))
    by_delta = np.cumsum(steps).astype(np.int64).astype(np.uint16).view(np.int16)      # wraps: the deltas are what counts
    by_value = unzz(rng.choice(zs, size=50000)).astype(np.int16)
    reads = [by_delta, by_value]
    want = yard_of("windows", reads)
    assert all(int(want["delta"][z]) > 1000 for z in zs) and all(int(want["raw"][z]) > 1000 for z in zs)
    t = want["trans"]
    assert min(int(t[a, b]) for a in (159, 160, 161, 255, 256) for b in (159, 160, 161, 255, 256)) > 50
    same(TDev(reads, seed=52).run(), want, "windows")


@gpu
def test_every_subset_of_outputs(lib):
    """any subset of the four outputs gives what the full call gives for its members"""
    reads = edge_reads()[:13] + ragged_reads(40, seed=12)
    want = yard_of("subset", reads)
    d = TDev(reads, seed=41)
    for mask in range(1, 16):
        sub = tuple(k for b, k in enumerate(press.TALLY_OUTPUTS) if mask >> b & 1)
        got = d.run(sub)
        assert set(got) == set(sub)
        same(got, want, sub)
    same(press.signal_tally_host(reads, ("delta", "mom")), want, "host subset")
    press.signal_tally(d.sig, d.off, d.n)                     # no output at all: nothing to do, no error


@gpu
def test_tables_are_added_to_and_mom_is_set(lib):
    """tables that start as a pattern come back as pattern + counts; two calls double the counts; mom is overwritten"""
    rng = np.random.default_rng(42)
    reads = ragged_reads(60, seed=14)
    want = yard_of("adds", reads)
    pattern = {k: rng.integers(0, 1 << 62, size=want[k].size, dtype=np.uint64).reshape(want[k].shape) for k in ("raw", "delta", "trans")}
    d = TDev(reads, seed=43)
    got = d.run(pattern=pattern)
    for k in pattern:
        assert np.array_equal(got[k], pattern[k] + want[k]), k
    same({"mom": got["mom"]}, want, "mom set over a fill")
    twice = d.run(times=2)
    for k in pattern:
        assert np.array_equal(twice[k], 2 * want[k]), k
    same({"mom": twice["mom"]}, want, "mom after two calls")
    host = press.signal_tally_host(reads, into=pattern)
    for k in pattern:
        assert np.array_equal(host[k], pattern[k] + want[k]), ("host", k)


@gpu
def test_a_read_listed_twice_counts_twice(lib):
    reads = [L._walk(np.random.default_rng(44), n, 0.01) for n in (40000, 513, 9)]
    once = yard_of("listed-once", reads)
    d = TDev(reads, seed=45, off=lambda o: np.concatenate([o, o[:2]]), ns=lambda r: np.array([len(x) for x in r] + [len(r[0]), len(r[1])], dtype=np.uint32))
    got = d.run()
    extra = yard_of("listed-extra", reads[:2])
    for k in ("raw", "delta", "trans"):
        assert np.array_equal(got[k], once[k] + extra[k]), k
    assert got["mom"][:3].tobytes() == once["mom"].tobytes() and got["mom"][3:].tobytes() == once["mom"][:2].tobytes()


@gpu
def test_agrees_with_symbol_counts(lib):
    """delta[0..255] and the sum of delta[256..] are press_hip_symbol_counts' counts; the rows and columns of trans sum to
    the symbol counts less each read's last and first symbol; the moments' exception counts sum to counts[256]"""
    reads = edge_reads() + extreme_reads()[2:3]
    d = TDev(reads, seed=46)
    got = d.run()
    counts = device_symbol_counts(d)
    assert np.array_equal(counts, symbol_counts_of(reads))
    assert np.array_equal(got["delta"][:256], counts[:256]) and int(got["delta"][256:].sum()) == int(counts[256])
    first, last = np.zeros(257, dtype=np.uint64), np.zeros(257, dtype=np.uint64)
    for s in reads:
        sym = np.minimum(zz(deltas(s)), 256)
        if len(sym):
            first[sym[0]] += 1
            last[sym[-1]] += 1
    assert np.array_equal(got["trans"].sum(axis=1), counts - last) and np.array_equal(got["trans"].sum(axis=0), counts - first)
    assert int(got["mom"]["nex"].astype(np.uint64).sum()) == int(counts[256])


@gpu
def test_repeatable_and_independent_of_scratch(lib):
    """identical results twice, and behind press.scratch_fill(0xA5): the work list and its count are written before they are read"""
    import torch
    reads = ragged_reads(80, seed=15) + edge_reads()[10:]
    want = yard_of("repeat", reads)
    d = TDev(reads, seed=47)
    a = d.run()
    b = d.run()
    torch.cuda.synchronize()
    press.scratch_fill(0xA5)
    c = d.run()
    h = press.signal_tally_host(reads)
    for got, what in ((a, "first"), (b, "second"), (c, "behind the fill"), (h, "host behind the fill")):
        same(got, want, what)


@gpu
def test_host_form_equals_device_form(lib):
    reads = edge_reads() + extreme_reads()[:2]
    want = yard_of("host", reads)
    same(press.signal_tally_host(reads), want, "host")
    same(TDev(reads, seed=48).run(), want, "device")
    empty = press.signal_tally_host([])
    assert not empty["raw"].any() and not empty["trans"].any() and len(empty["mom"]) == 0


@gpu
def test_stream_contract(lib):
    """device resident, on a side stream behind a delay: the call returns while the delay is pending - it only enqueues -
    and its results are those of the same call made with nothing pending"""
    import torch
    reads = ragged_reads(50, seed=16)
    d = TDev(reads, seed=49)
    raw = torch.zeros(BINS, dtype=torch.int64, device="cuda")
    delta = torch.zeros(BINS, dtype=torch.int64, device="cuda")
    trans = torch.zeros(SYMS * SYMS, dtype=torch.int64, device="cuda")
    mom = torch.zeros(4 * d.nr, dtype=torch.int64, device="cuda")
    TRS.behind_a_delay(lib, lambda: press.signal_tally(d.sig, d.off, d.n, raw, delta, trans, mom), (raw, delta, trans, mom), "signal_tally")
    got = {"raw": raw.cpu().numpy(), "delta": delta.cpu().numpy(), "trans": trans.cpu().numpy(), "mom": mom.cpu().numpy().view(press.MOMENTS_DTYPE)}
    same(got, yard_of("stream", reads), "behind a delay")


@gpu
def test_dataset_report(lib, tmp_path):
    """the report over tests/golden/three-reads.blow5 (svb-zd fields, decoded on the device) holds the fixture's tables and
    counts, and the tool's --tsv files are the reference's printtally text byte for byte"""
    st, reads = fixture_set("three_reads")
    want = yard_of("fx/three_reads", reads)
    path = os.path.join(GOLD, "three-reads.blow5")
    rep = press.dataset_report(path)
    same(rep, want, "report")
    assert rep["reads"] == 3 and rep["samples"] == sum(len(s) for s in reads)
    assert ["three_reads/" + i for i in rep["ids"]] == [e["name"] for e in st["reads"]]
    assert rep["raw_summary"] == press.tally_summary(want["raw"]) and rep["delta_summary"] == press.tally_summary(want["delta"])
    assert (rep["h0"], rep["h1"]) == press.transition_entropy(want["trans"]) and 0 < rep["h1"] <= rep["h0"] < 9
    assert rep["ratio"]["delta"] == 16 / rep["bits"]["delta"] and rep["dor"].shape == (3, 3) and (rep["dor"][:, 0] > 0).all()
    again = press.dataset_report(reads, max_reads=2)          # a list of arrays, in two batches
    same(again, want, "report of arrays")
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dataset_report.py"), path, "--tsv", str(tmp_path)], env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert open(tmp_path / "raw.freq").read() == st["raw_text"] and open(tmp_path / "delta.freq").read() == st["delta_text"]
    rows = open(tmp_path / "stats.tsv").read().split("\n")
    assert rows[0].split("\t")[:4] == ["id", "n", "min", "max"] and len(rows) == 5 and rows[-1] == ""
    for e, line in zip(st["reads"], rows[1:]):
        f = line.split("\t")
        assert ["three_reads/" + f[0], int(f[1]), int(f[2]), int(f[3])] == [e["name"], e["n"], e["min"], e["max"]]
    assert "entropy" in run.stdout and "reads\t3" in run.stdout
