"""press_hip_signal_quantiles_ranged / press_hip_signal_stats_ranged (include/press_hip.h 2y): order statistics over the
samples [a', b') of each read alone.

Two yardsticks, both exact: the unranged call on the sliced batch (reads[r][a':b'] laid out as a batch of its own), and
numpy's np.partition over the same slices.  The read lengths cover one tile of CHUNK = 32768 samples, a tile edge and
three tiles; the ranges cover every start within an 8-sample group, a range inside one group, ranges that start or end on
a tile edge and one that leaves a whole tile out at each end.
"""
import numpy as np
import pytest
import torch  # before the library is loaded, as in a run of the whole suite

from honours_amd import build, press

gpu = pytest.mark.gpu
EARG = -2
CHUNK = 32768
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 2049, 32767, 32768, 32769, 70000)
RANKS = ([(1, 2)], [(1, 5), (9, 10)], [(0, 1), (1, 1), (1, 2)], [(1, 2), (1, 2), (1, 10), (9, 10)])
FILL = 77


def make_reads():
    rng = np.random.default_rng(2024)
    reads = []
    for n in LENGTHS:
        s = np.clip(np.cumsum(rng.integers(-40, 41, size=n)) + 300, -32768, 32767).astype(np.int16)
        if n:  # the two ends of the type, at the read's edges and inside
            s[rng.integers(0, n, size=min(n, 6))] = rng.choice([-32768, 32767], size=min(n, 6))
            s[0], s[-1] = 32767, -32768
        reads.append(s)
    return reads


# name -> (a, b) of a read of n samples
RANGES = {
    "none": None,
    "whole": lambda n: (0, n),
    "empty": lambda n: (5, 5),
    "a>b": lambda n: (10, 3),
    "b>n": lambda n: (2, n + 100),
    "a>n": lambda n: (n + 3, n + 9),
    "in-one-group": lambda n: (9, 14),
    "from-tile-edge": lambda n: (CHUNK, n),
    "to-tile-edge": lambda n: (3, CHUNK),
    "tile-to-tile": lambda n: (CHUNK, 2 * CHUNK),
    "skip-a-tile-each-end": lambda n: (CHUNK + 100, 2 * CHUNK - 100),
    "last-sample": lambda n: (max(n, 1) - 1, n),
    "huge": lambda n: (0xFFFFFFF0, 0xFFFFFFFF),
}
RANGES.update({"a%%8=%d" % k: (lambda n, k=k: (k, max(n - (8 - k), 0))) for k in range(1, 8)})
RANGES.update({"a=8j+%d" % k: (lambda n, k=k: (2040 + k, n - k)) for k in (1, 4, 7)})


def ranges_of(name, reads):
    f = RANGES[name]
    if f is None:
        return None
    return np.array([[min(max(x, 0), 0xFFFFFFFF) for x in f(len(s))] for s in reads], dtype=np.uint32)


def sliced(reads, rng):
    cut = press.clamp_ranges([len(s) for s in reads], rng)
    return [s[int(a):int(b)] for s, (a, b) in zip(reads, cut)]


def quant_ref(s, ranks):
    if len(s) == 0:
        return [0] * len(ranks)
    return [int(np.partition(s, k)[k]) for k in (min(len(s) - 1, len(s) * a // b) for a, b in ranks)]


def stats_ref(s):
    if len(s) == 0:
        return [0, 0]
    k = len(s) // 2
    med = int(np.partition(s, k)[k])
    return [med, int(np.partition(np.abs(s.astype(np.int64) - med), k)[k])]


# ------------------------------------------------------------------ CPU

def test_clamp_and_plan_of_ranges():
    """chunk_plan_ranged is chunk_plan over the clamped lengths: b > n, a > b, a == b, a > n, no range"""
    from test_depress_chunks import plan_ref
    build.build()
    ns = [100, 100, 100, 100, 0, 64, 65, 1000]
    rng = [[10, 200], [60, 20], [7, 7], [300, 400], [0, 5], [0, 64], [0, 65], [3, 1000]]
    cut = press.clamp_ranges(ns, rng)
    assert cut.dtype == np.uint32 and cut.tolist() == [[10, 100], [20, 20], [7, 7], [100, 100], [0, 0], [0, 64], [0, 65], [3, 1000]]
    assert press.clamp_ranges(ns, None).tolist() == [[0, n] for n in ns]
    for T, ov in ((8, 0), (64, 5), (64, 63), (2048, 0)):
        for r in (rng, None):
            L = [int(b) - int(a) for a, b in press.clamp_ranges(ns, r)]
            got = press.chunk_plan_ranged(ns, r, T, ov)
            for g, w in zip(got, plan_ref(L, T, ov)):
                assert g.dtype == w.dtype and np.array_equal(g, w), (T, ov)
    with pytest.raises(press.PressError):
        press.chunk_plan_ranged(ns, rng[:3], 8, 0)


def test_refusals_need_no_device():
    """the unranged calls' checks, PRESS_HIP_EARG before any device call, in both forms"""
    build.build()
    lib = press.load_library()
    sig = np.zeros(64, dtype=np.int16)
    off = np.zeros(1, dtype=np.uint64)
    n = np.full(1, 8, dtype=np.uint32)
    rng = np.array([0, 4], dtype=np.uint32)
    out = np.full(8, FILL, dtype=np.int32)
    num, den = np.array([1, 1], dtype=np.uint32), np.array([2, 2], dtype=np.uint32)
    p = lambda x: None if x is None else x.ctypes.data

    def stats(dev, s=sig, o=off, nn=n, st=out):
        return lib.press_hip_signal_stats_ranged(p(s), p(o), p(nn), 1, 64, p(rng), p(st), dev)

    def quant(dev, s=sig, o=off, nn=n, a=num, b=den, nq=2, q=out):
        return lib.press_hip_signal_quantiles_ranged(p(s), p(o), p(nn), 1, 64, p(rng), p(a), p(b), nq, p(q), dev)
    for dev in (0, 1):
        for kw in ("s", "o", "nn", "st"):
            assert stats(dev, **{kw: None}) == EARG and "NULL" in press.last_error(), kw
        for kw in ("s", "o", "nn", "a", "b", "q"):
            assert quant(dev, **{kw: None}) == EARG and "NULL" in press.last_error(), kw
        for nq in (0, 5):
            assert quant(dev, nq=nq) == EARG and "quantiles" in press.last_error()
        assert quant(dev, b=np.array([2, 0], dtype=np.uint32)) == EARG and "rank" in press.last_error()
        assert quant(dev, a=np.array([3, 1], dtype=np.uint32)) == EARG and "rank" in press.last_error()
    assert stats(1, s=sig[1:]) == EARG and "aligned" in press.last_error()
    assert (out == FILL).all()
    if not torch.cuda.is_available():
        for f, args in ((press.signal_stats_ranged_host, ([sig[:8]], [[0, 4]])),
                        (press.signal_quantiles_ranged_host, ([sig[:8]], [(1, 2)], [[0, 4]]))):
            with pytest.raises(press.PressError) as e:
                f(*args)
            assert "hip" in str(e.value).lower()


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.use_torch_stream()
    yield lb
    torch.cuda.synchronize()
    press.use_torch_stream()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def reads():
    return make_reads()


def _t(a, dtype=None):
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


@gpu
@pytest.mark.parametrize("name", sorted(RANGES))
def test_ranged_is_unranged_on_the_sliced_batch(lib, reads, name):
    rng = ranges_of(name, reads)
    sl = sliced(reads, rng)
    assert name not in ("whole", "none") or all(len(a) == len(b) for a, b in zip(sl, reads))
    # host form
    want_s = press.signal_stats_host(sl)
    got_s = press.signal_stats_ranged_host(reads, rng)
    assert np.array_equal(got_s, want_s), (name, got_s.tolist(), want_s.tolist())
    assert want_s.tolist() == [stats_ref(s) for s in sl], name
    for ranks in RANKS:
        want = press.signal_quantiles_host(sl, ranks)
        got = press.signal_quantiles_ranged_host(reads, ranks, rng)
        assert np.array_equal(got, want), (name, ranks, got.tolist(), want.tolist())
        assert want.tolist() == [quant_ref(s, ranks) for s in sl], (name, ranks)
    # device resident: the same numbers, nothing written beyond the tables
    sig, off, ns, total = press._host_batch(reads)
    d_sig, d_off, d_n = _t(sig), _t(off, np.int64), _t(ns, np.int32)
    d_rng = None if rng is None else _t(rng.reshape(-1), np.int32)
    nr = len(reads)
    d_st = torch.full((2 * nr + 8,), FILL, dtype=torch.int32, device="cuda")
    press.signal_stats_ranged(d_sig, d_off, d_n, d_rng, d_st)
    outs = []
    for ranks in RANKS:
        d_q = torch.full((len(ranks) * nr + 8,), FILL, dtype=torch.int32, device="cuda")
        press.signal_quantiles_ranged(d_sig, d_off, d_n, d_rng, ranks, d_q)
        outs.append(d_q)
    torch.cuda.synchronize()
    st = d_st.cpu().numpy()
    assert np.array_equal(st[:2 * nr].reshape(-1, 2), want_s) and (st[2 * nr:] == FILL).all(), name
    for ranks, d_q in zip(RANKS, outs):
        q = d_q.cpu().numpy()
        k = len(ranks) * nr
        assert q[:k].reshape(nr, -1).tolist() == [quant_ref(s, ranks) for s in sl] and (q[k:] == FILL).all(), (name, ranks)


@gpu
def test_what_lies_outside_the_range_takes_no_part(lib, reads):
    """the same ranges over reads whose samples outside [a', b') are the extremes of the type: the same statistics"""
    rng = ranges_of("a%8=3", reads)
    cut = press.clamp_ranges([len(s) for s in reads], rng)
    loud = []
    for s, (a, b) in zip(reads, cut):
        t = s.copy()
        t[:int(a)] = 32767
        t[int(b):] = -32768
        loud.append(t)
    ranks = RANKS[3]
    assert np.array_equal(press.signal_stats_ranged_host(loud, rng), press.signal_stats_ranged_host(reads, rng))
    assert np.array_equal(press.signal_quantiles_ranged_host(loud, ranks, rng), press.signal_quantiles_ranged_host(reads, ranks, rng))
    assert not np.array_equal(press.signal_stats_host(loud), press.signal_stats_host(reads))  # (the premise)


@gpu
def test_no_reads(lib):
    assert press.signal_stats_ranged_host([], None).shape == (0, 2)
    assert press.signal_quantiles_ranged_host([], [(1, 2)], None).shape == (0, 1)
