"""press_hip_signal_stats / press_hip_norm_cal: per-read median and MAD on the device (include/press_hip.h).

The contract is one of integers: with k = n // 2, med = the k-th smallest sample and mad = the k-th smallest
|sample - med| (sigtk's mediani16 / madf before its factor) - np.partition is that definition, and
tests/golden/sigtk_stats.json pins np.partition to the reference's own selection.  norm_cal is defined in IEEE single
precision, one rounding per operation, which is numpy's float32 arithmetic.  Every comparison is exact.

CPU: norm_cal against numpy, the yardstick against the golden numbers, the argument checks that come before any
device call, the workspace size.  GPU: the read battery on scattered rooms, hand-made reads at the edges of the
radix select (a rank on the first / last sample of a value, pairs of values that differ in one digit only, the extreme
keys, neighbouring rows), 300 short reads, repeatability, a canary around stats, the host path.
"""
import json
import os

import numpy as np
import pytest

import _layouts as L
from honours_amd import build, press

gpu = pytest.mark.gpu
EARG = -2
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONFUSED = [m for m in press.METHODS if m not in L.SVB_KINDS]


def ref_stats(s):
    """the definition -> (med, mad); (0, 0) for an empty read"""
    s = np.asarray(s, dtype=np.int16)
    if s.size == 0:
        return 0, 0
    k = s.size // 2
    med = int(np.partition(s, k)[k])
    mad = int(np.partition(np.abs(s.astype(np.int32) - med), k)[k])
    return med, mad


def ref_cal(stats):
    """the definition of c0, c1 in numpy float32 -> (nreads, 2)"""
    st = np.asarray(stats, dtype=np.int32).reshape(-1, 2)
    c0 = (-st[:, 0].astype(np.int64)).astype(np.float32)
    scale = st[:, 1].astype(np.float32) * np.float32(1.4826)
    with np.errstate(all="ignore"):
        c1 = np.where(st[:, 1] > 0, np.float32(1.0) / scale, np.float32(1.0)).astype(np.float32)
    return np.stack([c0, c1], axis=1)


def norm_bits(s, med, mad):
    """the definition of the normalised floats, as uint32 bit patterns"""
    c = ref_cal([[med, mad]])[0]
    return ((np.asarray(s).astype(np.float32) + c[0]) * c[1]).view(np.uint32)


# ------------------------------------------------------------------ CPU

@pytest.fixture(scope="module")
def cpu_lib():
    build.build()
    return press.load_library()


def test_norm_cal_against_numpy(cpu_lib):
    rng = np.random.default_rng(17)
    pairs = [(med, mad) for mad in (0, 1, 2, 3, 255, 256, 65535) for med in (-32768, -1, 0, 1, 32767)]
    pairs += list(zip(rng.integers(-32768, 32768, size=300).tolist(), rng.integers(0, 65536, size=300).tolist()))
    st = np.array(pairs, dtype=np.int32)
    want = ref_cal(st)
    got = press.norm_cal(st)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    zero = st[:, 1] == 0
    assert zero.sum() >= 5 and (got[zero, 1].view(np.uint32) == np.float32(1.0).view(np.uint32)).all()
    assert got[0, 0] == 32768.0  # -(-32768) has no int16
    # the raw call, an empty batch, NULL arguments
    raw = np.zeros(2 * len(st), dtype=np.float32)
    assert cpu_lib.press_hip_norm_cal(st.ctypes.data, len(st), raw.ctypes.data) == 0
    assert np.array_equal(raw.view(np.uint32), want.reshape(-1).view(np.uint32))
    assert cpu_lib.press_hip_norm_cal(None, 0, None) == 0
    assert cpu_lib.press_hip_norm_cal(None, 3, raw.ctypes.data) == EARG
    assert cpu_lib.press_hip_norm_cal(st.ctypes.data, 3, None) == EARG


def golden_reads():
    """name -> samples of every entry of sigtk_stats.json"""
    meta = json.load(open(os.path.join(GOLD, "three_reads.json")))["reads"]
    raw = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    out, at = {}, 0
    for r in meta:
        out["three_reads/" + r["read_id"]] = raw[at:at + r["n"]]
        at += r["n"]
    for name, s in L.battery():
        if len(s):
            out["battery/" + name] = s
    return out


def test_numpy_reference_is_sigtk():
    """the yardstick of this file and of test_depress_norm.py gives the reference's numbers on all 29 reads"""
    gold = json.load(open(os.path.join(GOLD, "sigtk_stats.json")))["reads"]
    reads = golden_reads()
    assert len(gold) == len(reads) == 29
    for g in gold:
        s = reads[g["name"]]
        assert len(s) == g["n"], g["name"]
        assert ref_stats(s) == (g["med"], g["mad"]), g["name"]
    # the issue's hand example, prefixes of one array
    x = np.array([5, -3, 9, 9, -32768, 32767], dtype=np.int16)
    assert [ref_stats(x[:n]) for n in range(1, 7)] == [(5, 0), (5, 8), (5, 4), (9, 4), (5, 4), (9, 12)]


def test_argument_checks_need_no_device(cpu_lib):
    """NULL arguments and bad ids are PRESS_HIP_EARG before any device call: also where there is no device"""
    p = lambda x: x.ctypes.data
    a = np.zeros(256, dtype=np.uint8)
    io = np.zeros(1, dtype=np.uint64)
    il = np.full(1, 16, dtype=np.uint64)
    out = np.zeros(64, dtype=np.float32)
    sig = np.zeros(64, dtype=np.int16)
    n = np.full(1, 8, dtype=np.uint32)
    st = np.full(2, 77, dtype=np.int32)
    on = np.full(1, 7, dtype=np.uint32)
    ms = np.zeros(8, dtype=np.float32)
    mid = press.METHODS["slow5_svb_zd"]
    for dev in (0, 1):
        assert cpu_lib.press_hip_signal_stats(None, p(io), p(n), 1, 64, p(st), dev) == EARG and "NULL" in press.last_error()
        assert cpu_lib.press_hip_signal_stats(p(sig), None, p(n), 1, 64, p(st), dev) == EARG
        assert cpu_lib.press_hip_signal_stats(p(sig), p(io), None, 1, 64, p(st), dev) == EARG
        assert cpu_lib.press_hip_signal_stats(p(sig), p(io), p(n), 1, 64, None, dev) == EARG
        call = lambda mm, oo, nn: cpu_lib.press_hip_depress_norm_batch(mm, p(a), p(io), p(il), 1, oo, p(io), p(n), 64, p(st), nn, dev)
        for bad in (-1, len(press.METHODS)):
            assert call(bad, p(out), p(on)) == EARG
            assert "not available" in press.last_error()
        assert call(mid, None, p(on)) == EARG and "NULL" in press.last_error()
        assert call(mid, p(out), None) == EARG and "NULL" in press.last_error()
    assert cpu_lib.press_hip_signal_stats_timed(p(sig), p(io), p(n), 1, 64, p(st), None) == EARG
    assert cpu_lib.press_hip_signal_stats_timed(None, p(io), p(n), 1, 64, p(st), p(ms)) == EARG
    assert (st == 77).all() and on[0] == 7 and (out == 0).all()


def test_workspace_bytes(cpu_lib):
    t, nr = 1 << 20, 64
    for m, mid in press.METHODS.items():
        base = int(cpu_lib.press_hip_workspace_bytes(mid, t, nr))
        pa = int(cpu_lib.press_hip_depress_pa_workspace_bytes(mid, t, nr))
        ws = int(cpu_lib.press_hip_depress_norm_workspace_bytes(mid, t, nr))
        if m in NONFUSED:
            assert ws >= pa, (m, ws, pa)
            assert ws - pa >= nr * (16 + 8), (m, ws - pa)  # the state and the two floats of every read, and its row
        assert ws - base >= 2 * t, (m, ws - base)
    assert len(NONFUSED) == 15
    for bad in (-1, len(press.METHODS), 1000):
        assert cpu_lib.press_hip_depress_norm_workspace_bytes(bad, t, nr) == 0


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.use_torch_stream()
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


CANARY = 0x5EEDBEEF


def device_stats(reads, seed=3, guard=16):
    """reads scattered over a noisy arena -> (nreads, 2) int32 of the device, the canaries around stats checked"""
    import torch
    sig, off = L.scatter_reads(np.random.default_rng(seed), reads)
    ns = np.array([len(r) for r in reads], dtype=np.uint32)
    d_stats = torch.full((2 * len(reads) + 2 * guard,), CANARY, dtype=torch.int32, device="cuda")
    press.signal_stats(_t(sig), _t(off, np.int64), _t(ns, np.int32), d_stats[guard:guard + 2 * len(reads)])
    torch.cuda.synchronize()
    got = d_stats.cpu().numpy()
    assert (got[:guard] == CANARY).all() and (got[guard + 2 * len(reads):] == CANARY).all(), "stats written outside [0, 2 nreads)"
    return got[guard:guard + 2 * len(reads)].reshape(-1, 2)


def check_exact(reads, got, names=None):
    want = np.array([ref_stats(r) for r in reads], dtype=np.int32).reshape(-1, 2)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(int(k), names[k] if names else len(reads[k]), got[k].tolist(), want[k].tolist()) for k in bad[:6]]


@gpu
def test_battery_device_resident(lib):
    bat = L.battery()
    reads = [s for _, s in bat]
    got = device_stats(reads)
    check_exact(reads, got, [k for k, _ in bat])
    lens = sorted(len(r) for r in reads)
    assert lens[:3] == [0, 0, 0] and 32767 in lens and 32768 in lens and 32769 in lens and 65543 in lens and lens[-1] == 150000
    k = [n for n, _ in bat].index("constant-4000")
    assert got[k].tolist() == [-1234, 0]


def handmade(n):
    """reads of n samples at the edges of the selection (n = 32769: two tiles, and odd; n = 6)"""
    h = n // 2
    out = {}

    rng = np.random.default_rng(1000 + n)

    def two(a, b, na):  # na samples at a, the rest at b, shuffled
        return rng.permutation(np.concatenate([np.full(na, a), np.full(n - na, b)]).astype(np.int16))
    out["rank-on-first-of-B"] = two(100, 900, h)           # sorted[k] is the first B
    out["rank-on-last-of-A"] = two(100, 900, h + 1)        # sorted[k] is the last A
    for a, b in ((0x1200 - 32768, 0x1201 - 32768), (300, 301), (-1, 0), (255, 256), (0x12FF - 32768, 0x1300 - 32768), (-257, 255), (-32768, -32767)):
        out["pair-%d-%d-lowhalf" % (a, b)] = two(a, b, h)
        out["pair-%d-%d-highhalf" % (a, b)] = two(a, b, h + 1)
    for a, b in ((0x1234 - 32768, 0x5634 - 32768), (-32768 + 52, 52), (0x0034 - 32768, 0x0134 - 32768)):  # the low digit the same
        out["hi-pair-%d-%d-lowhalf" % (a, b)] = two(a, b, h)
        out["hi-pair-%d-%d-highhalf" % (a, b)] = two(a, b, h + 1)
    out["extremes-mostly-min"] = two(-32768, 32767, h + 1)  # med = -32768: d reaches 65535
    out["extremes-mostly-max"] = two(-32768, 32767, h)      # med = 32767
    for lo, mid, hi in ((500 - 0x101, 500, 500 + 0x100), (500 - 0x201, 500, 500 + 0x101), (-2, 0, 3), (-32768, 0, 32767)):
        t = n // 3  # thirds: the MAD's rank falls among the two distances, which differ in one digit or in both
        out["thirds-%d-%d-%d" % (lo, mid, hi)] = rng.permutation(
            np.concatenate([np.full(t, lo), np.full(n - 2 * t, mid), np.full(t, hi)]).astype(np.int16))
    out["all-min"] = np.full(n, -32768, dtype=np.int16)
    out["all-max"] = np.full(n, 32767, dtype=np.int16)
    out["all-min-again"] = np.full(n, -32768, dtype=np.int16)
    s = np.full(n, 20000, dtype=np.int16)                   # a positive majority that does not reach rank k from below
    s[:h + 1] = -5
    out["negative-median"] = np.random.default_rng(n).permutation(s)
    s = np.random.default_rng(n + 1).integers(-32768, 32768, size=n).astype(np.int16)
    out["uniform-noise"] = s
    return out


@gpu
@pytest.mark.parametrize("n", [32769, 6])
def test_handmade_reads(lib, n):
    hm = handmade(n)
    reads = list(hm.values())
    want = {k: ref_stats(s) for k, s in hm.items()}
    # the cases are what they say
    assert want["rank-on-first-of-B"][0] == 900 and want["rank-on-last-of-A"][0] == 100
    # (an odd n leaves the larger half at d = 0; an even n puts rank k on d = 65535)
    assert want["extremes-mostly-min"] == (-32768, 0) and want["extremes-mostly-max"] == (32767, 65535 if n % 2 == 0 else 0)
    assert want["negative-median"][0] == -5
    assert want["all-min"] == (-32768, 0) and want["all-max"] == (32767, 0)
    check_exact(reads, device_stats(reads, seed=n), list(hm.keys()))


@gpu
def test_300_short_reads(lib):
    rng = np.random.default_rng(300)
    reads = [L._walk(rng, n, 0.02) for n in range(1, 301)]
    check_exact(reads, device_stats(reads, seed=9))


@gpu
def test_twice_the_same(lib):
    reads = [s for _, s in L.battery()]
    a = device_stats(reads, seed=5)
    b = device_stats(reads, seed=5)
    assert np.array_equal(a, b)
    check_exact(reads, a)


@gpu
def test_host_path_agrees(lib):
    bat = L.battery()
    reads = [s for _, s in bat]
    host = press.signal_stats_host(reads)
    assert host.dtype == np.int32 and host.shape == (len(reads), 2)
    check_exact(reads, host, [k for k, _ in bat])
    assert np.array_equal(host, device_stats(reads, seed=21))
    # overlapping ranges are refused before anything runs; an empty batch is fine; a misaligned device arena is not
    import torch
    off = np.array([0, 8], dtype=np.uint64)
    n = np.array([9, 4], dtype=np.uint32)
    sig = np.zeros(64, dtype=np.int16)
    st = np.full(4, 77, dtype=np.int32)
    p = lambda x: x.ctypes.data
    assert lib.press_hip_signal_stats(p(sig), p(off), p(n), 2, 64, p(st), 0) == EARG and "overlaps" in press.last_error()
    assert (st == 77).all()
    assert lib.press_hip_signal_stats(None, None, None, 0, 0, None, 0) == 0
    d = torch.zeros(64, dtype=torch.int16, device="cuda")
    z = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert lib.press_hip_signal_stats(d[1:].data_ptr(), z.data_ptr(), z.data_ptr(), 1, 32, z.data_ptr(), 1) == EARG
    assert "aligned" in press.last_error()
