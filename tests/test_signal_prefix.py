"""sigtk's prefix on the device (include/press_hip.h, "Range statistics and the prefix"):
press_hip_signal_prefix against the definition - the adaptor's and the poly-A's positions exactly, the thresholds and the
statistics by bit pattern, the medians with ==.

The yardstick composes the ones that are already pinned: jnnv2 and jnn_core's walk of tests/test_signal_segments.py and
the range statistics of tests/test_range_stats.py, as prefix_func (sigtk/src/cfunc.c:169-234) composes them.  It must
reproduce every entry of tests/golden/sigtk_prefix.json (tests/golden/make_prefix_golden.py).
"""
import ctypes

import numpy as np
import pytest

import _layouts as L
import test_range_stats as TRS
import test_signal_segments as TSS
from honours_amd import press

gpu = pytest.mark.gpu
EARG = -2
F32 = np.float32
bits, bits_f32, one_nan = TSS.bits, TSS.bits_f32, TSS.one_nan
GUARD = TSS.GUARD
V2, POLYA = TSS.V2, TSS.PRESETS["polya"]


# ------------------------------------------------------------------ the yardstick

def yard_prefix(key, s, cal, v2=V2, polya=POLYA, rna=1, shift=30.0, half=20.0):
    """prefix_func -> ((adapt_start, adapt_end, polya_start, polya_end), (bot, top), adaptor's statistics, poly-A's)"""
    pair = TSS.yard2(key, s, v2)[0]
    ps = pe = -1
    bot = top = F32(0)
    if pair[1] > 0 and rna:
        m_a = TRS.yard_range(s, cal, pair)[0]
        with np.errstate(all="ignore"):
            t = F32(m_a + F32(shift))
            top, bot = F32(t + F32(half)), F32(t - F32(half))
            x = TSS.yard_signal(s[pair[1]:], cal)
            inr = ((x < top) & (x > bot)).tolist()
        rec = first_record(inr, polya)
        if rec is not None:
            ps, pe = rec[0] + pair[1], rec[1] + pair[1]
    st_a = TRS.yard_range(s, cal, pair if pair[1] > 0 else (0, 0))
    st_p = TRS.yard_range(s, cal, (ps, pe) if pe > 0 else (0, 0))
    return (pair[0], pair[1], ps, pe), (bot, top), st_a, st_p


def first_record(inr, prm):
    """segs[0] of jnn_core: the walk over the flags up to the sample behind which no merge can change the first record"""
    if True not in inr:
        return None
    rec = TSS.yard_walk(inr, prm)
    return None if len(rec) == 0 else (int(rec[0][0]), int(rec[0][1]))


_yard = {}


def yard(key, s, cal, **kw):
    k = (key, bits(cal[0]), bits(cal[1]), tuple(sorted(kw.items())))
    if k not in _yard:
        _yard[k] = yard_prefix(key, s, cal, **kw)
    return _yard[k]


def planted_read(seed, lead=3000, low=2600, flat=400, tail=3000, level=90, drop=45, up=30):
    """a high level, a stretch of `low` samples `drop` pA below it, a flat stretch of `flat` samples `up` pA above that,
    then noise: an adaptor and a poly-A tail, under PLANT_CAL"""
    rng = np.random.default_rng(seed)
    pa = np.concatenate([level + rng.normal(0, 6, lead), level - drop + rng.normal(0, 2, low),
                         level - drop + up + rng.normal(0, 1.5, flat), level + rng.normal(0, 12, tail)])
    return np.round(pa / PLANT_CAL[1] - PLANT_CAL[0]).astype(np.int16)


PLANT_CAL = (F32(6.0), F32(1467.61 / 8192.0))


def mixed_batch():
    """reads with all four outcomes: too short (-1, -1), no adaptor (0, 0), an adaptor without a tail, both"""
    rng = np.random.default_rng(640)
    named = TSS.named_reads()
    reads = [planted_read(1), L._walk(rng, 1500), np.full(4000, 500, dtype=np.int16), planted_read(2, up=-80),
             named["battery/synth-4"], planted_read(3, lead=2100, flat=300), L._walk(rng, 0), planted_read(4, flat=0, tail=800)]
    keys = ["plant-1", "mixed-short", "mixed-flat", "plant-2", "battery/synth-4", "plant-3", "mixed-empty", "plant-4"]
    return reads, keys


# ------------------------------------------------------------------ without a GPU

@pytest.fixture(scope="module")
def cpu_lib():
    from honours_amd import build
    build.build()
    return press.load_library()


def test_yardstick_equals_the_reference():
    """every entry of sigtk_prefix.json: the four positions exactly, the thresholds by bit pattern, the statistics of both
    stretches"""
    reads = TSS.named_reads()
    for e in TRS.fixture()["entries"]:
        s = reads[e["name"]]
        pos, thr, st_a, st_p = yard(e["name"], s, TRS.f3(e["cal_bits"]))
        assert list(pos) == e["adapt"] + e["polya"], e["name"]
        if e["thr_bits"] is None:
            assert e["adapt"][1] <= 0 and (bits(thr[0]), bits(thr[1])) == (0, 0)
        else:
            assert [bits(thr[0]), bits(thr[1])] == e["thr_bits"], e["name"]
        for got, want in ((st_a, e["adapt_stat"]), (st_p, e["polya_stat"])):
            if want is None:
                assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 0
            else:
                TRS.same_stats(TRS.stat_bits([got]), [TRS.f3(want)], e["name"])


def test_fixture_conditions():
    """every branch of prefix_func is in the fixture"""
    c1, c2 = (TRS.entries_of(c) for c in TRS.fixture_cals())
    assert len(c1) == 29 and len(c2) == 29
    short = lambda n: n.split("/", 1)[1]
    with_adaptor = [short(e["name"]) for e in c1 if e["adapt"][1] > 0]
    synth = ["synth-%d" % k for k in range(6)]
    assert len(with_adaptor) == 13 and sum(len(n) == 36 for n in with_adaptor) == 2  # the two long real reads
    assert set(with_adaptor) >= {"ex1-32767", "ex1-32768", "ex1-32769", "ex1-65543", "ex30-20000"} | set(synth)
    tails1 = [short(e["name"]) for e in c1 if e["polya"][1] > 0]
    assert tails1 == synth
    s4 = [e for e in c1 if e["name"] == "battery/synth-4"][0]
    assert s4["polya"][0] == s4["adapt"][1]  # the tail starts at the adaptor's end: suffix position 0
    tails2 = [short(e["name"]) for e in c2 if e["polya"][1] > 0]
    assert len(tails2) == 5 and sum(len(n) == 36 for n in tails2) == 2 and tails2[2:] == ["synth-2", "synth-4", "synth-5"]
    pairs = [tuple(e["adapt"]) for e in c1 + c2]
    assert (0, 0) in pairs and (-1, -1) in pairs
    for e in c1 + c2:  # an adaptor and no tail: m_a is far below zero on the ex1 reads
        if short(e["name"]).startswith("ex1-3") or short(e["name"]) == "ex1-65543":
            assert e["adapt"][1] > 0 and e["polya"] == [-1, -1] and bits_f32(e["adapt_stat"][0]) < -100
        assert (e["polya"][1] > 0) == (e["polya_stat"] is not None) and (e["adapt"][1] > 0) == (e["thr_bits"] is not None)
        assert e["prefix_text"].startswith(e["name"] + "\t%d\t" % e["n"]) and e["stat_text"].startswith(e["name"] + "\t")


def test_planted_reads_have_all_outcomes():
    """the mixed batch of the GPU tests: (-1, -1), (0, 0), an adaptor without a tail, an adaptor with one"""
    reads, keys = mixed_batch()
    got = [yard(k, s, PLANT_CAL)[0] for k, s in zip(keys, reads)]
    kinds = {"short": 0, "none": 0, "adaptor": 0, "tail": 0}
    for p in got:
        kinds["short" if p[1] < 0 else "none" if p[1] == 0 else "tail" if p[3] > 0 else "adaptor"] += 1
    assert min(kinds.values()) >= 1, (kinds, got)
    p = got[0]  # the planted read: the adaptor is the low stretch, the tail the flat stretch behind it
    assert 2500 < p[0] < 3500 and 5200 < p[1] < 5700 and 5500 < p[2] < 5700 and p[3] - p[2] >= 250, p


def test_presets(cpu_lib):
    p = press.prefix_params()
    a, q = p.adaptor, p.polya
    assert (bits(a.std_scale), a.seg_dist, a.window, a.hi_thresh, a.lo_thresh) == (bits(0.5), 1500, 2000, 200000, 2000)
    assert (q.corrector, q.seg_dist, q.window, q.error) == (50, 200, 250, 30)
    assert [bits(q.std_scale), bits(q.stall_len), bits(q.top), bits(q.bot)] == [bits(-1.0), bits(1.0), 0, 0]
    assert (p.rna, bits(p.shift), bits(p.half)) == (1, bits(30.0), bits(20.0))
    assert cpu_lib.press_hip_prefix_params_preset(0, None) == EARG
    assert cpu_lib.press_hip_prefix_params_preset(1, ctypes.addressof(p)) == EARG
    assert cpu_lib.press_hip_prefix_params_preset(-1, ctypes.addressof(p)) == EARG


def test_bad_arguments(cpu_lib):
    """NULL arguments and the parameter checks of both underlying calls are PRESS_HIP_EARG before any device call: the same
    with and without a device"""
    lib = cpu_lib
    a = np.zeros(64, dtype=np.uint64)
    p = a.ctypes.data
    ok = press.prefix_params()
    q = ctypes.addressof(ok)
    for dr in (0, 1):
        # sig off n nreads total cal prm out stat thr
        args = [p, p, p, 1, 8, p, q, p, p, p]
        for k in (0, 1, 2, 5, 6, 7):
            bad = list(args)
            bad[k] = None
            assert lib.press_hip_signal_prefix(*bad, dr) == EARG, (k, dr)
            assert "NULL" in press.last_error()
        for field, v in (("window", 0), ("window", -5), ("corrector", -1), ("error", -1), ("seg_dist", -1),
                         ("stall_len", float("nan")), ("stall_len", float("inf")), ("stall_len", float("-inf"))):
            prm = press.prefix_params()
            setattr(prm.polya, field, v)
            assert lib.press_hip_signal_prefix(*args[:6], ctypes.addressof(prm), *args[7:], dr) == EARG, (field, v, dr)
            assert "jnn parameters" in press.last_error()
        for w in (0, -1, 8193, 1 << 30):
            prm = press.prefix_params()
            prm.adaptor.window = w
            assert lib.press_hip_signal_prefix(*args[:6], ctypes.addressof(prm), *args[7:], dr) == EARG, (w, dr)
            assert "window" in press.last_error()
    assert lib.press_hip_signal_prefix(p + 2, p, p, 1, 8, p, q, p, p, p, 1) == EARG and "aligned" in press.last_error()


def test_workspace(cpu_lib):
    """exact: the adaptor's pair and the two ranges of every read, nothing per sample; 0 for an empty batch"""
    ws = press.signal_prefix_workspace_bytes
    assert ws(0) == 0
    for r in (1, 2, 64, 300, 8192, 100000):
        assert ws(r) == 24 * r


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


def run_prefix(d, prm, want_stat=True, want_thr=True):
    """press.signal_prefix on an RDev -> (out int32 [nr, 4], stat bits [2 nr, 3] or None, thr bits [nr, 2] or None); every
    output lies between guard words, which are checked"""
    import torch
    nr = d.nr
    out, stat, thr = d.room(4 * nr), d.room(6 * nr), d.room(2 * nr)
    press.signal_prefix(d.sig, d.off, d.n, d.cal, prm, out[GUARD:GUARD + 4 * nr],
                        stat[GUARD:GUARD + 6 * nr].view(torch.float32) if want_stat else None,
                        thr[GUARD:GUARD + 2 * nr].view(torch.float32) if want_thr else None)
    torch.cuda.synchronize()
    o = d.inside(out, 4 * nr, "out").view(np.int32).reshape(-1, 4)
    s = d.inside(stat, 6 * nr if want_stat else 0, "stat")
    t = d.inside(thr, 2 * nr if want_thr else 0, "thr")
    return o, s.reshape(-1, 3) if want_stat else None, t.reshape(-1, 2) if want_thr else None


def check(got, want, what=""):
    """got = (out, stat, thr) of run_prefix or of signal_prefix_host (as bits) against [yard_prefix's tuple]"""
    out, stat, thr = got
    assert out.tolist() == [list(w[0]) for w in want], (what, out.tolist(), [w[0] for w in want])
    if thr is not None:
        wt = one_nan(np.array([[bits(w[1][0]), bits(w[1][1])] for w in want], dtype=np.uint32))
        assert np.array_equal(one_nan(thr), wt), (what, "thr")
    if stat is not None:
        TRS.same_stats(stat, [st for w in want for st in (w[2], w[3])], what)


def host_bits(res):
    out, stat, thr = res
    return (out.view(np.int32).reshape(-1, 4), None if stat is None else stat.view(np.uint32).reshape(-1, 3),
            None if thr is None else thr.view(np.uint32).reshape(-1, 2))


# ------------------------------------------------------------------ on the GPU

@gpu
def test_fixture_batches(lib):
    """the fixture's reads as one batch per calibration, device resident and with host pointers, against the reference's
    numbers themselves"""
    named = TSS.named_reads()
    for cal in TRS.fixture_cals():
        ent = TRS.entries_of(cal)
        reads = [named[e["name"]] for e in ent]
        cals = [cal] * len(reads)
        want = []
        for e in ent:
            thr = (F32(0), F32(0)) if e["thr_bits"] is None else TRS.f3(e["thr_bits"])
            st = [TRS.NAN3 if b is None else TRS.f3(b) for b in (e["adapt_stat"], e["polya_stat"])]
            want.append((tuple(e["adapt"] + e["polya"]), thr, st[0], st[1]))
        check(run_prefix(TRS.RDev(reads, cals, seed=21), press.prefix_params()), want, "device resident")
        check(host_bits(press.signal_prefix_host(reads, np.array(cals))), want, "host")
    out0, stat0, thr0 = press.signal_prefix_host([], np.zeros((0, 2), dtype=F32))
    assert len(out0) == 0 and stat0.shape == (0, 2) and thr0.shape == (0, 2)


@gpu
def test_mixed_batch_and_outputs(lib):
    """planted reads and all four outcomes in one batch; stat and thr present and NULL in all four combinations; rna = 0"""
    reads, keys = mixed_batch()
    cals = [PLANT_CAL] * len(reads)
    want = [yard(k, s, PLANT_CAL) for k, s in zip(keys, reads)]
    d = TRS.RDev(reads, cals, seed=22)
    prm = press.prefix_params()
    full = run_prefix(d, prm)
    check(full, want)
    for ws, wt in ((True, False), (False, True), (False, False)):
        got = run_prefix(d, prm, ws, wt)
        check(got, want, (ws, wt))
        assert (got[1] is None) == (not ws) and (got[2] is None) == (not wt)
        check(host_bits(press.signal_prefix_host(reads, np.array(cals), prm, ws, wt)), want, ("host", ws, wt))
    prm.rna = 0
    want0 = [yard(k, s, PLANT_CAL, rna=0) for k, s in zip(keys, reads)]
    assert all(w[0][2:] == (-1, -1) and bits(w[1][1]) == 0 for w in want0) and any(w[0][1] > 0 for w in want0)
    check(run_prefix(d, prm), want0, "rna = 0")


@gpu
def test_other_parameters(lib):
    """another shift and half, a shorter poly-A window and error allowance: per-read thresholds through the shared walk"""
    reads, keys = mixed_batch()
    cals = [(F32(6.0 + r), F32(1467.61 / 8192.0)) for r in range(len(reads))]
    polya = (-1.0, 20, 100, 120, 1.0, 10, 0.0, 0.0)
    prm = press.prefix_params()
    prm.polya = press.JnnParams(*polya)
    prm.shift, prm.half = 28.5, 9.25
    want = [yard_prefix(k, s, c, polya=polya, shift=28.5, half=9.25) for k, s, c in zip(keys, reads, cals)]
    assert len({bits(w[1][0]) for w in want}) >= 4 and any(w[0][3] > 0 for w in want)
    check(run_prefix(TRS.RDev(reads, cals, seed=23), prm), want)


@gpu
def test_repeatable_behind_scratch_fill(lib):
    """the results do not depend on what the library's scratch held (the pairs and the ranges between the launches are
    written before they are read): equal behind press.scratch_fill of two byte values"""
    import torch
    reads, keys = mixed_batch()
    cals = [PLANT_CAL] * len(reads)
    d = TRS.RDev(reads, cals, seed=24)
    got = []
    for byte in (0x00, 0xFF):
        torch.cuda.synchronize()
        press.scratch_fill(byte)
        got.append(run_prefix(d, press.prefix_params()) + host_bits(press.signal_prefix_host(reads, np.array(cals))))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    check(got[0][:3], [yard(k, s, PLANT_CAL) for k, s in zip(keys, reads)])


@gpu
def test_stream_contract(lib):
    """device resident, on a side stream behind a delay: the call returns while the delay is pending - it only enqueues
    its three launches - and its results are those of the same call made with nothing pending"""
    import torch
    reads, keys = mixed_batch()
    nr = len(reads)
    d = TRS.RDev(reads, [PLANT_CAL] * nr, seed=25)
    prm = press.prefix_params()
    out = torch.zeros((nr, 4), dtype=torch.int32, device="cuda")
    stat = torch.zeros((2 * nr, 3), dtype=torch.float32, device="cuda")
    thr = torch.zeros(2 * nr, dtype=torch.float32, device="cuda")
    TRS.behind_a_delay(lib, lambda: press.signal_prefix(d.sig, d.off, d.n, d.cal, prm, out, stat, thr), (out, stat, thr),
                       "signal_prefix")
    check((out.cpu().numpy(), stat.cpu().numpy().view(np.uint32), thr.cpu().numpy().view(np.uint32).reshape(-1, 2)),
          [yard(k, s, PLANT_CAL) for k, s in zip(keys, reads)])


@gpu
def test_nan_and_inf_calibrations(lib):
    """cal is not validated: a NaN m_a gives NaN thresholds and no tail, inf goes through the definition; nothing faults
    and nothing outside the rooms is written"""
    reads = [planted_read(1), planted_read(2), planted_read(3), planted_read(5)]
    keys = ["plant-1", "plant-2b", "plant-3b", "plant-5"]
    cals = [(F32(np.nan), F32(0.18)), (F32(6.0), F32(np.inf)), (F32(6.0), F32(np.nan)), (F32(-np.inf), F32(-1.0))]
    want = [yard_prefix(k, s, c) for k, s, c in zip(keys, reads, cals)]
    assert all(w[0][1] > 0 and w[0][3] == -1 for w in want) and np.isnan(want[0][1][0])
    check(run_prefix(TRS.RDev(reads, cals, seed=26), press.prefix_params()), want)
