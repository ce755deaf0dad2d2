"""press_hip_depress_chunks_trimmed_batch (include/press_hip.h 2y): compressed reads straight to scaled chunk rows that
start behind a range's start, the row plan made on the device.

Everything is pinned by composition.  The yardstick of rows, q and row_first is press_hip_depress_chunks_batch with
press_hip_chunk_plan on the SLICED batch - the samples [a', b') of what press_hip_depress_batch decodes of every read,
pressed again with slow5_svb_zd; the cuts of the detector modes are what press.signal_adaptor_host /
press.signal_segments_host give on the decoded reads.  Every comparison is one of integers or of bit patterns.
"""
import ctypes

import numpy as np
import pytest
import torch  # before the library is loaded, as in a run of the whole suite

import _layouts as L
from honours_amd import build, press
from test_depress_chunks import RULE, bad_rules
from test_ranged_stats import LENGTHS, RANGES
from test_stream_contract import WAITED, cycles_per_ms, hold  # noqa: F401 (cycles_per_ms: a fixture, over this module's lib)

gpu = pytest.mark.gpu
EARG = -2
F32 = 0xFFFFFFFF
GUARD = 5                    # rows, and row-table entries, of canary behind the cap
ROW_CANARY = {4: 0x7FC12345, 2: 0x7E57}  # by element size; neither is a zero
TAB_CANARY = 0x5EED5EED
FILL = 77
GRID = ((8, 0), (64, 5), (64, 63), (2048, 0), (4096, 104))
DTYPES = ("float32", "float16", "bfloat16")
TORCH_DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
WIDE = ("shuffman_vbe21_zd", "zstd_svb_zd", "hasgam_vbsse21_zdq")  # streams with a count of their own: the room may be larger
YARD = "slow5_svb_zd"        # the method the sliced batch is pressed with
METHODS = ("slow5_svb_zd", "svb12_zd", "shuffman_vbe21_zd", "zstd_svb_zd", "hasgam_vbsse21_zdq", "rc_vbe21_zd", "huffman_vbe21_zd",
           "dstall_fz")


def walk(rng, n, level=300):
    s = np.clip(np.cumsum(rng.integers(-40, 41, size=n)) + level, -32768, 32767).astype(np.int16)
    if n > 4:
        s[1], s[n // 2] = 32767, -32768
    return s


class Batch:
    """reads of one method as streams in scattered rooms, and what press_hip_depress_batch decodes of them (the premise of
    the sliced batch): dec[r] the decoded samples, None for a refused read"""

    def __init__(self, m, reads, seed, spoil=(), wide_rooms=False):
        rng = np.random.default_rng(seed)
        self.m = m
        st, _ = press.press_packed_host(m, reads)
        self.streams = [b"" if x is None else x for x in st]
        for k in spoil:  # a stream cut short
            self.streams[k] = self.streams[k][:max(1, len(self.streams[k]) // 3)]
        wide = wide_rooms and m in WIDE
        self.rooms = np.array([len(s) + (int(rng.integers(1, 21)) if wide else 0) for s in reads], dtype=np.uint32)
        self.dec = press.depress_batch_host(m, self.streams, self.rooms)
        self.inb, self.in_off, self.in_len = L.scatter_streams(rng, self.streams)
        self.off, self.total = L.scatter_rooms(rng, self.rooms)
        self.c = np.array([0 if d is None else len(d) for d in self.dec], dtype=np.uint32)
        self.out_n = np.array([F32 if d is None else len(d) for d in self.dec], dtype=np.uint32)
        self.dev = None

    def tensors(self):
        if self.dev is None:
            self.dev = (_t(self.inb), _t(self.in_off, np.int64), _t(self.in_len, np.int64), _t(self.off, np.int64), _t(self.rooms, np.int32))
        return self.dev

    def bound(self, T, ov):
        return int(press.chunk_plan(self.rooms, T, ov)[0][-1])


def _t(a, dtype=None):
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


def bits_of(rows):
    return rows.view(np.uint32) if rows.dtype == np.float32 else rows.view(np.uint16)


def yardstick(b, cut, T, ov, dtype, rule):
    """the existing calls on the sliced batch -> (rows as bits, q, row_first, row_read, row_start in the read)"""
    sl = [np.zeros(0, dtype=np.int16) if d is None else d[int(a):int(e)] for d, (a, e) in zip(b.dec, cut)]
    ns = [len(s) for s in sl]
    st, _ = press.press_packed_host(YARD, sl)
    rows, q, rr, rs, on = press.depress_chunks_batch_host(YARD, st, ns, T, ov, dtype=dtype, rule=rule)
    assert on.tolist() == ns
    first = press.chunk_plan(ns, T, ov)[0]
    return bits_of(rows), q, first, rr, rs + cut[rr.astype(np.int64), 0] if len(rr) else rs


def run(b, T, ov, dtype, rule, trim=None, ranges=None, seg_cal=None, cap=None, enqueue_only=False):
    """the device-resident call over canaries -> dict of numpy arrays; cap defaults to the untrimmed rows + 2"""
    nr = len(b.rooms)
    cap = b.bound(T, ov) + 2 if cap is None else cap
    es = 4 if dtype == "float32" else 2
    raw = torch.full(((cap + GUARD) * T,), ROW_CANARY[es], dtype=torch.int32 if es == 4 else torch.int16, device="cuda")
    rows = raw.view(TORCH_DT[dtype]).view(cap + GUARD, T)
    t = {k: torch.full((cap + GUARD,), TAB_CANARY, dtype=torch.int32, device="cuda") for k in ("row_read", "row_start")}
    t["row_first"] = torch.full((nr + 1 + 4,), FILL, dtype=torch.int64, device="cuda")
    t["cut"] = torch.full((2 * nr + 4,), FILL, dtype=torch.int32, device="cuda")
    t["q"] = torch.full((2 * nr + 4,), FILL, dtype=torch.int32, device="cuda")
    t["out_n"] = torch.full((nr,), 7, dtype=torch.int32, device="cuda")
    d_in, d_io, d_il, d_off, d_n = b.tensors()
    d_rng = None if ranges is None else _t(np.asarray(ranges, dtype=np.uint32).reshape(-1), np.int32)
    d_cal = None if seg_cal is None else _t(np.asarray(seg_cal, dtype=np.float32).reshape(-1))
    torch.cuda.synchronize()

    def enqueue():
        press.depress_chunks_trimmed_batch(b.m, d_in, d_io, d_il, rows[:cap], t["row_first"], d_off, d_n, b.total, t["out_n"], ov, trim=trim,
                                           rng=d_rng, seg_cal=d_cal, cut=t["cut"], row_read=t["row_read"], row_start=t["row_start"],
                                           rule=rule, q=t["q"], T=T)

    def fetch():
        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in t.items()}
        assert (g["row_first"][nr + 1:] == FILL).all() and (g["cut"][2 * nr:] == FILL).all() and (g["q"][2 * nr:] == FILL).all()
        g["rows"] = raw.cpu().numpy().view(np.uint32 if es == 4 else np.uint16).reshape(cap + GUARD, T)
        g["row_first"] = g["row_first"][:nr + 1].view(np.uint64)
        g["cut"] = g["cut"][:2 * nr].view(np.uint32).reshape(-1, 2)
        g["q"] = g["q"][:2 * nr].reshape(-1, 2)
        g["out_n"] = g["out_n"].view(np.uint32)
        g["row_read"], g["row_start"] = g["row_read"].view(np.uint32), g["row_start"].view(np.uint32)
        g["cap"] = cap
        return g
    if enqueue_only:
        return enqueue, fetch
    enqueue()
    return fetch()


def check(tag, b, g, cut, T, ov, dtype, rule):
    """g against the yardstick of the cuts `cut`: the plan in full, everything below min(cap, planned) exact, canaries behind"""
    wrows, wq, wfirst, wrr, wrs = yardstick(b, cut, T, ov, dtype, rule)
    cap = g["cap"]
    assert np.array_equal(g["out_n"], b.out_n), tag
    assert np.array_equal(g["cut"], cut), tag + (g["cut"].tolist(), cut.tolist())
    assert np.array_equal(g["row_first"], wfirst), tag + (g["row_first"].tolist(), wfirst.tolist())
    assert np.array_equal(g["q"], wq), tag + (g["q"].tolist(), wq.tolist())
    w = min(cap, int(wfirst[-1]))
    bad = np.nonzero((g["rows"][:w] != wrows[:w]).any(axis=1))[0]
    if bad.size:
        r0 = int(bad[0])
        col = int(np.nonzero(g["rows"][r0] != wrows[r0])[0][0])
        assert False, tag + ("row", r0, "of read", int(wrr[r0]), "column", col, hex(int(g["rows"][r0, col])), hex(int(wrows[r0, col])))
    assert (g["rows"][w:] == ROW_CANARY[g["rows"].dtype.itemsize]).all(), tag + ("rows written at or beyond min(nrows_cap, planned)",)
    assert np.array_equal(g["row_read"][:w], wrr[:w]) and np.array_equal(g["row_start"][:w], wrs[:w]), tag
    assert (g["row_read"][w:] == TAB_CANARY).all() and (g["row_start"][w:] == TAB_CANARY).all(), tag
    return int(wfirst[-1])


def mixed_ranges(ns, shift, T):
    """a range kind of test_ranged_stats per read of ns[r] samples, rotated by `shift`; and L == T, L == T + 1, L == 0 for the
    three reads shape_reads adds for it"""
    kinds = sorted(k for k in RANGES if RANGES[k] is not None)
    out = []
    for r, n in enumerate(int(n) for n in ns):
        a, e = RANGES[kinds[(r + shift) % len(kinds)]](n)
        out.append([min(max(a, 0), F32), min(max(e, 0), F32)])
        if n == 3 * T + 11:
            out[r] = [[5, 5 + T], [7, 7 + T + 1], [9, 9]][(r + shift) % 3]
    return np.array(out, dtype=np.uint32)


def shape_reads(T, ov):
    rng = np.random.default_rng(T * 100 + ov)
    ns = [min(n, 2049) for n in LENGTHS] if ov == 63 else list(LENGTHS)
    ns = ns[:6] + [3 * T + 11] * 3 + ns[6:]  # the three special ranges, in the middle of the batch
    return [walk(rng, n) for n in ns]


# ------------------------------------------------------------------ CPU

@pytest.fixture(scope="module")
def cpu_lib():
    build.build()
    return press.load_library()


def test_argument_checks_need_no_device(cpu_lib):
    """bad id, mode, T, overlap, dtype, rule or detector parameter, NULL arguments: PRESS_HIP_EARG before any device call"""
    p = lambda x: None if x is None else x.ctypes.data
    a = np.zeros(256, dtype=np.uint8)
    io = np.zeros(1, dtype=np.uint64)
    il = np.full(1, 16, dtype=np.uint64)
    rows = np.zeros(64, dtype=np.float32)
    n = np.full(1, 8, dtype=np.uint32)
    first = np.full(2, FILL, dtype=np.uint64)
    tab = np.full(8, FILL, dtype=np.uint32)
    q = np.full(2, FILL, dtype=np.int32)
    on = np.full(1, 7, dtype=np.uint32)
    mid = press.METHODS["slow5_svb_zd"]
    ad = lambda x: None if x is None else ctypes.addressof(x)

    def call(dev, m=mid, rw=rows, cap=8, dt=0, T=8, ov=0, rf=first, off=io, nn=n, trim=None, ru=RULE, o=on, inb=a, ioff=io, ilen=il):
        return cpu_lib.press_hip_depress_chunks_trimmed_batch(m, p(inb), p(ioff), p(ilen), 1, p(rw), cap, dt, T, ov, p(rf), p(tab), p(tab), p(off),
                                                              p(nn), 64, ad(trim), None, None, p(tab), ad(ru), p(q), p(o), dev)
    bad_trims = []
    for mode in (-1, 3):
        t = press.trim_range()
        t.mode = mode
        bad_trims.append((t, "mode"))
    for w in (0, 8193):
        t = press.trim_adaptor()
        t.adaptor.window = w
        bad_trims.append((t, "window"))
    for field, v in (("window", 0), ("corrector", -1), ("error", -1), ("seg_dist", -1), ("stall_len", float("inf"))):
        t = press.trim_segment()
        setattr(t.seg, field, v)
        bad_trims.append((t, "jnn"))
    for dev in (0, 1):
        for bad in (-1, len(press.METHODS), 88, 99):
            assert call(dev, m=bad) == EARG and "not available" in press.last_error()
        for bad in (-1, 3):
            assert call(dev, dt=bad) == EARG and "dtype" in press.last_error()
        for T, ov in ((0, 0), (12, 0), (8, 8), (8, 9)):
            assert call(dev, T=T, ov=ov) == EARG and "multiple of 8" in press.last_error()
        for bad in bad_rules():
            assert call(dev, ru=bad) == EARG and "rule" in press.last_error()
        for t, word in bad_trims:
            assert call(dev, trim=t) == EARG and word in press.last_error(), (word, press.last_error())
        for kw in ("rw", "rf", "off", "nn", "o", "inb", "ioff", "ilen"):
            assert call(dev, **{kw: None}) == EARG and "NULL" in press.last_error(), kw
        if not torch.cuda.is_available():  # what is optional is no refusal: these reach the device check
            for t in (None, press.trim_range(), press.trim_adaptor(min_keep=3), press.trim_segment()):
                assert call(dev, trim=t, ru=None) == -3 and "hip" in press.last_error().lower()
            assert call(dev, rw=None, cap=0) == -3
    assert (q == FILL).all() and on[0] == 7 and (rows == 0).all() and (first == FILL).all() and (tab == FILL).all()


def test_wrappers_reach_the_library(cpu_lib):
    """the two forms with tiny buffers: without a device they come back with the library's missing-device error"""
    if torch.cuda.is_available():
        pytest.skip("GPU present: the device form would run on host addresses")
    z = lambda k, d: torch.zeros(k, dtype=d)
    comp, i64, n = z(76, torch.uint8), torch.tensor([0, 12], dtype=torch.int64), torch.tensor([9, 0], dtype=torch.int32)
    for trim in (None, press.trim_adaptor(), press.trim_segment(min_keep=4)):
        for rows, T in ((z((2, 8), torch.float16), None), (None, 8)):
            with pytest.raises(press.PressError) as e:
                press.depress_chunks_trimmed_batch("svb_zd", comp, i64, i64, rows, z(3, torch.int64), i64, n, 16, z(2, torch.int32), 2, trim=trim,
                                                   rng=z(4, torch.int32), seg_cal=z(4, torch.float32), cut=z(4, torch.int32),
                                                   row_read=z(2, torch.int32), row_start=z(2, torch.int32), rule=RULE, q=z(4, torch.int32), T=T)
            assert "hip" in str(e.value).lower()
        with pytest.raises(press.PressError) as e:
            press.depress_chunks_trimmed_batch_host("svb_zd", [bytes(12), b""], [9, 0], 8, 2, trim=trim, ranges=[[1, 5], [0, 0]],
                                                    seg_cal=[[0.0, 1.0]] * 2, rule=RULE)
        assert "hip" in str(e.value).lower()
    with pytest.raises(press.PressError, match="needs T"):
        press.depress_chunks_trimmed_batch("svb_zd", comp, i64, i64, None, z(3, torch.int64), i64, n, 16, z(2, torch.int32), 2)


def test_press_hands_out_all_of_trim():
    """honours_amd.trim's __all__ names every public function, class and constant it defines, and each is press.<name>"""
    import inspect

    from honours_amd import trim
    own = {n for n, v in vars(trim).items()
           if not n.startswith("_") and ((inspect.isfunction(v) or inspect.isclass(v)) and v.__module__ == trim.__name__ or n.isupper())}
    assert own == set(trim.__all__), sorted(own ^ set(trim.__all__))
    for n in trim.__all__:
        assert getattr(press, n) is getattr(trim, n), n
    assert not hasattr(press, "trim_nothing")


def test_workspace_bytes(cpu_lib):
    t, nr = 1 << 20, 64
    ws = press.depress_chunks_trimmed_workspace_bytes
    ids = list(press.METHODS) + ["huffman_vbe21_zd", "rice_vbsse21_zd", "rccdf_vbbe21_zd", "dstall_fz"]
    for m in ids:
        plain = int(cpu_lib.press_hip_depress_chunks_workspace_bytes(press._mid(m), t, nr, 1024, 104))
        sizes = [ws(m, t, nr, 1024, 104, mode) for mode in (0, 1, 2)]
        assert plain > 0 and sizes[0] >= plain + 2 * 4 * nr, (m, sizes, plain)       # the cuts, at the least
        assert sizes[1] >= sizes[0] + 3 * 4 * nr and sizes[2] >= sizes[1], (m, sizes)  # the counts and the detector's results
        assert sizes == [ws(m, t, nr, 8, 0, mode) for mode in (0, 1, 2)]
        assert ws(m, 2 * t, nr, 64, 8) >= sizes[0] and ws(m, t, 2 * nr, 64, 8) >= sizes[0]
    for bad in (-1, len(press.METHODS), 88, 1000):
        assert ws(bad, t, nr, 64, 8) == 0
    for T, ov in ((0, 0), (12, 0), (8, 8)):
        assert ws(0, t, nr, T, ov) == 0
    for mode in (-1, 3):
        assert ws(0, t, nr, 64, 8, mode) == 0


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.load_table()
    press.use_torch_stream()
    yield lb
    torch.cuda.synchronize()
    press.use_torch_stream()
    torch.cuda.empty_cache()


_shapes = {}


def shape_batch(T, ov):
    if (T, ov) not in _shapes:
        _shapes[(T, ov)] = Batch(YARD, shape_reads(T, ov), T + ov)
    return _shapes[(T, ov)]


@gpu
@pytest.mark.parametrize("T,ov", GRID)
def test_range_mode_is_the_chunk_call_on_the_sliced_batch(lib, T, ov):
    """both branches of the row writer, the three dtypes, with a rule and without; each call gives every read one range kind
    of test_ranged_stats, rotated from call to call, so a length meets six of the kinds (test_ranged_stats.py has every kind
    on every length for the count kernels); L == T, L == T + 1 and L == 0 in the middle of the batch"""
    b = shape_batch(T, ov)
    assert all(d is not None for d in b.dec)
    seen = set()
    for shift, (dtype, rule) in enumerate((d, r) for d in DTYPES for r in (RULE, None)):
        rng = mixed_ranges(b.c, 5 * shift, T)
        cut = press.clamp_ranges(b.c, rng)
        g = run(b, T, ov, dtype, rule, trim=press.trim_range() if shift % 2 else None, ranges=rng)
        planned = check((T, ov, dtype, rule is not None), b, g, cut, T, ov, dtype, rule)
        assert planned > 3
        seen |= {int(e) - int(a) for a, e in cut}
    assert {0, T, T + 1} <= seen and max(seen) > 3 * T


_methods = {}


def method_batch(m):
    if m not in _methods:
        rng = np.random.default_rng(len(m))
        reads = [walk(rng, n) for n in (2049, 0, 700, 9, 4097, 64, 1300, 33000)]
        _methods[m] = Batch(m, reads, 11 + len(m), spoil=(2, 6), wide_rooms=True)
    return _methods[m]


@gpu
@pytest.mark.parametrize("m", METHODS)
def test_every_decode_path(lib, m):
    """one method per decode path, the two families by their extended ids; rooms larger than the reads; two streams cut short
    among good ones: whatever press_hip_depress_batch makes of them is the premise, and a refused read takes no row"""
    b = method_batch(m)
    assert sum(d is not None and len(d) > 0 for d in b.dec) >= 5, [None if d is None else len(d) for d in b.dec]
    assert m not in WIDE or ((b.rooms[[0, 4, 7]] > b.c[[0, 4, 7]]).all() and b.c[[0, 4, 7]].tolist() == [2049, 4097, 33000])
    rng = np.array([[3, 2000], [0, 5], [13, 650], [2, 8], [64, 5000], [0, 64], [1001, 1002], [100, 32900]], dtype=np.uint32)
    cut = press.clamp_ranges(b.c, rng)
    for dtype, rule in (("float16", RULE), ("float32", None)):
        g = run(b, 64, 5, dtype, rule, ranges=rng)
        check((m, dtype), b, g, cut, 64, 5, dtype, rule)
        for r, d in enumerate(b.dec):
            if d is None:
                assert g["cut"][r].tolist() == [0, 0] and g["row_first"][r] == g["row_first"][r + 1] and g["q"][r].tolist() == [0, 0]


@gpu
def test_a_stream_cut_short_is_refused(lib):
    """the premise of "refused reads among good ones" for the method the other tests use"""
    b = method_batch(YARD)
    assert b.dec[2] is None and b.dec[6] is None and all(b.dec[r] is not None for r in (0, 1, 3, 4, 5, 7))


@gpu
def test_no_range_and_no_trim_is_the_untrimmed_call(lib):
    """range == NULL, trim == NULL: rows, q and out_n of press_hip_depress_chunks_batch, row_first the host plan"""
    T, ov = 64, 5
    b = shape_batch(T, ov)
    nr = len(b.rooms)
    first, rr, rs = press.chunk_plan(b.rooms, T, ov)
    planned = int(first[-1])
    d_in, d_io, d_il, d_off, d_n = b.tensors()
    for dtype, rule in (("bfloat16", RULE), ("float32", None)):
        rows = torch.zeros((planned, T), dtype=TORCH_DT[dtype], device="cuda")
        q = torch.zeros(2 * nr, dtype=torch.int32, device="cuda")
        on = torch.zeros(nr, dtype=torch.int32, device="cuda")
        press.depress_chunks_batch(b.m, d_in, d_io, d_il, rows, _t(first, np.int64), d_off, d_n, b.total, on, ov, rule=rule, q=q)
        g = run(b, T, ov, dtype, rule)
        torch.cuda.synchronize()
        es = 4 if dtype == "float32" else 2
        want = rows.view(torch.int32 if es == 4 else torch.int16).cpu().numpy().view(np.uint32 if es == 4 else np.uint16)
        assert np.array_equal(g["row_first"], first) and np.array_equal(g["rows"][:planned], want)
        assert np.array_equal(g["q"].reshape(-1), q.cpu().numpy()) and np.array_equal(g["out_n"], on.cpu().numpy().view(np.uint32))
        assert np.array_equal(g["row_read"][:planned], rr) and np.array_equal(g["row_start"][:planned], rs)
        assert np.array_equal(g["cut"], press.clamp_ranges(b.rooms, None))
        assert (g["rows"][planned:] == ROW_CANARY[es]).all()


@gpu
@pytest.mark.parametrize("T,ov", [(64, 5), (4096, 104)])
def test_cap_rules(lib, T, ov):
    """nrows_cap inside a read, 0 and above the need: the plan is complete every time, nothing at or beyond the cap is
    touched; rows == NULL with nrows_cap == 0 is the plan alone"""
    b = shape_batch(T, ov)
    rng = mixed_ranges(b.c, 6, T)  # (the rotation that gives the longest read its whole length)
    cut = press.clamp_ranges(b.c, rng)
    first = press.chunk_plan(cut[:, 1] - cut[:, 0], T, ov)[0]
    planned = int(first[-1])
    big = int(np.argmax(np.diff(first.astype(np.int64))))
    inside = int(first[big]) + 2
    assert int(first[big]) < inside < int(first[big + 1]) - 1
    for cap in (inside, 0, planned, planned + 3):
        g = run(b, T, ov, "float16", RULE, ranges=rng, cap=cap)
        assert check((T, ov, cap), b, g, cut, T, ov, "float16", RULE) == planned
    # the pure plan
    d_in, d_io, d_il, d_off, d_n = b.tensors()
    d_first = torch.full((len(b.rooms) + 1,), FILL, dtype=torch.int64, device="cuda")
    d_cut = torch.full((2 * len(b.rooms),), FILL, dtype=torch.int32, device="cuda")
    d_on = torch.zeros(len(b.rooms), dtype=torch.int32, device="cuda")
    press.depress_chunks_trimmed_batch(b.m, d_in, d_io, d_il, None, d_first, d_off, d_n, b.total, d_on, ov, rng=_t(rng.reshape(-1), np.int32),
                                       cut=d_cut, T=T)
    torch.cuda.synchronize()
    assert np.array_equal(d_first.cpu().numpy().view(np.uint64), first)
    assert np.array_equal(d_cut.cpu().numpy().view(np.uint32).reshape(-1, 2), cut)
    assert np.array_equal(d_on.cpu().numpy().view(np.uint32), b.out_n)


# ------------------------------------------------------------------ the detector modes

def dip_read(rng, n, dips, level=500, low=200):
    s = (level + rng.integers(-5, 6, size=n)).astype(np.int16)
    for a, e in dips:
        s[a:e] = (low + rng.integers(-5, 6, size=e - a)).astype(np.int16)
    return s


def stall_read(rng, n, stalls):
    """samples far outside (430, 470) on either side, with stretches inside it"""
    s = np.where(np.arange(n) % 2 == 0, 100, 900).astype(np.int16) + rng.integers(-20, 21, size=n).astype(np.int16)
    for a, e in stalls:
        s[a:e] = (450 + rng.integers(-8, 9, size=e - a)).astype(np.int16)
    return s


def detector_reads():
    rng = np.random.default_rng(77)
    return [dip_read(rng, 3000, [(300, 700)]),            # a dip: the adaptor
            stall_read(rng, 2500, [(50, 350)]),            # a stall at the front
            np.full(1200, 480, dtype=np.int16),            # constant, outside the band: neither finds anything
            dip_read(rng, 10, []),                         # n <= window
            dip_read(rng, 2000, [(1500, 1900)]),           # a dip near the end: min_keep undoes the cut
            stall_read(rng, 2100, [(1700, 2050)]),         # ... and a stall near the end
            dip_read(rng, 4100, [(100, 180), (2000, 2300)]),
            stall_read(rng, 4000, [(0, 200), (215, 400), (3000, 3100)]),
            walk(rng, 1500)]                               # cut short below: refused


def detector_batch():
    if "det" not in _methods:
        _methods["det"] = Batch(YARD, detector_reads(), 5, spoil=(8,))
    return _methods["det"]


ADAPTOR = press.Jnn2Params(0.5, 20, 16, 2000, 8)
SEGMENT = press.JnnParams(-1.0, 10, 20, 16, 1.0, 2, 470.0, 430.0)
MIN_KEEP = 300


def apply_min_keep(a, c, min_keep):
    a = np.minimum(a.astype(np.int64), c.astype(np.int64))
    a = np.where(c.astype(np.int64) - a < min_keep, 0, a)
    return np.stack([a, c.astype(np.int64)], axis=1).astype(np.uint32)


def detector_check(b, trim, cut, seg_cal=None):
    for T, ov, dtype, rule in ((64, 5, "float16", RULE), (2048, 0, "float32", None)):
        g = run(b, T, ov, dtype, rule, trim=trim, seg_cal=seg_cal)
        check((trim.mode, T, dtype), b, g, cut, T, ov, dtype, rule)
        # everything else is mode RANGE with those cuts
        h = run(b, T, ov, dtype, rule, trim=press.trim_range(), ranges=cut)
        for k in ("rows", "row_first", "row_read", "row_start", "cut", "q", "out_n"):
            assert np.array_equal(g[k], h[k]), (trim.mode, T, dtype, k)


@gpu
@pytest.mark.parametrize("min_keep", [0, MIN_KEEP])
def test_adaptor_mode(lib, min_keep):
    b = detector_batch()
    dec = [np.zeros(0, dtype=np.int16) if d is None else d for d in b.dec]
    assert b.dec[8] is None
    pair, _ = press.signal_adaptor_host(dec, ADAPTOR, want_thr=False)
    assert pair[3].tolist() == [-1, -1] and pair[8].tolist() == [-1, -1] and pair[2].tolist() == [0, 0]
    assert 650 < pair[0, 1] < 750 and 1850 < pair[4, 1] < 1950 and pair[6, 1] > 0, pair.tolist()
    a = np.where(pair[:, 1] > 0, pair[:, 1], 0)
    cut = apply_min_keep(a, b.c, min_keep)
    assert (cut[4, 0] == 0) == (min_keep > 0) and cut[0, 0] == pair[0, 1] and cut[8].tolist() == [0, 0]
    detector_check(b, press.trim_adaptor(ADAPTOR, min_keep=min_keep), cut)


@gpu
@pytest.mark.parametrize("domain", ["raw", "cal"])
@pytest.mark.parametrize("min_keep", [0, MIN_KEEP])
def test_segment_mode(lib, domain, min_keep):
    b = detector_batch()
    nr = len(b.dec)
    dec = [np.zeros(0, dtype=np.int16) if d is None else d for d in b.dec]
    prm, cal = SEGMENT, None
    if domain == "cal":  # x = (s + 10) * 0.5, and in read 1 another scale: its stall leaves the band
        cal = np.tile(np.array([10.0, 0.5], dtype=np.float32), (nr, 1))
        cal[5] = [10.0, 0.25]
        prm = press.JnnParams(-1.0, 10, 20, 16, 1.0, 2, 240.0, 220.0)
    seg, first, count, _ = press.signal_segments_host(dec, cal=cal, prm=prm, want_thr=False)
    assert (count != press.SEGMENT_NOFIT).all()
    end = np.array([int(seg["end"][int(first[r])]) if first[r + 1] > first[r] else 0 for r in range(nr)], dtype=np.int64)
    assert 340 <= end[1] <= 360 and end[0] == 0 and end[3] == 0 and end[8] == 0 and end[7] > 0, end.tolist()
    assert (end[5] > 2000) == (domain == "raw"), end.tolist()
    cut = apply_min_keep(end, b.c, min_keep)
    assert cut[1, 0] == end[1] and (domain == "cal" or (cut[5, 0] == 0) == (min_keep > 0))
    detector_check(b, press.trim_segment(prm, min_keep=min_keep), cut, seg_cal=cal)


@gpu
def test_segment_mode_with_thresholds_of_its_own(lib):
    """std_scale > 0: the walk's thresholds come from the read's mean and deviation over the decoded samples"""
    b = detector_batch()
    dec = [np.zeros(0, dtype=np.int16) if d is None else d for d in b.dec]
    prm = press.JnnParams(0.75, 10, 20, 16, 1.0, 2, 0.0, 0.0)
    seg, first, count, _ = press.signal_segments_host(dec, prm=prm, want_thr=False)
    end = np.array([int(seg["end"][int(first[r])]) if first[r + 1] > first[r] else 0 for r in range(len(dec))], dtype=np.int64)
    assert (end > 0).any()
    g = run(b, 64, 5, "float16", RULE, trim=press.trim_segment(prm))
    check(("std",), b, g, apply_min_keep(end, b.c, 0), 64, 5, "float16", RULE)


# ------------------------------------------------------------------ contracts

@gpu
def test_enqueues_behind_a_held_stream(lib, cycles_per_ms):
    """device resident: every mode returns while the stream is still held, and delivers the right rows after release"""
    b = detector_batch()
    T, ov = 64, 5
    s = torch.cuda.current_stream()
    todo = []
    for trim, rng in ((None, mixed_ranges(b.c, 1, T)), (press.trim_adaptor(ADAPTOR), None), (press.trim_segment(SEGMENT), None)):
        todo.append((trim, rng) + run(b, T, ov, "float16", RULE, trim=trim, ranges=rng, enqueue_only=True))
    for _, _, enqueue, _ in todo:  # once before the hold: the scratch of these shapes is there
        enqueue()
    torch.cuda.synchronize()
    e = hold(s, cycles_per_ms)
    for _, _, enqueue, _ in todo:
        enqueue()
        assert not e.query(), WAITED
    got = [fetch() for _, _, _, fetch in todo]
    assert e.query()
    for (trim, rng, _, _), g in zip(todo, got):
        h = run(b, T, ov, "float16", RULE, trim=trim, ranges=rng)
        for k in ("rows", "row_first", "row_read", "row_start", "cut", "q", "out_n"):
            assert np.array_equal(g[k], h[k]), k
    check(("held",), b, got[0], press.clamp_ranges(b.c, todo[0][1]), T, ov, "float16", RULE)


@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "shuffman_vbe21_zd"])
def test_independent_of_what_scratch_held(lib, m):
    b = method_batch(m)
    rng = np.array([[3, 2000], [0, 5], [13, 650], [2, 8], [64, 5000], [0, 64], [1001, 1002], [100, 32900]], dtype=np.uint32)
    det = detector_batch()
    calls = [(b, None, rng), (det, press.trim_adaptor(ADAPTOR, min_keep=MIN_KEEP), None), (det, press.trim_segment(SEGMENT), None)]
    base = [run(bb, 64, 5, "float16", RULE, trim=t, ranges=r) for bb, t, r in calls]
    for byte in (0x00, 0xFF):
        for (bb, t, r), want in zip(calls, base):
            torch.cuda.synchronize()
            press.scratch_fill(byte)
            g = run(bb, 64, 5, "float16", RULE, trim=t, ranges=r)
            for k in ("rows", "row_first", "row_read", "row_start", "cut", "q", "out_n"):
                assert np.array_equal(g[k], want[k]), (m, byte, k)
    check((m, "fill"), b, base[0], press.clamp_ranges(b.c, rng), 64, 5, "float16", RULE)


@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "zstd_svb_zd", "dstall_fz"])
def test_host_form_is_the_device_form(lib, m):
    b = method_batch(m)
    rng = np.array([[3, 2000], [0, 5], [13, 650], [2, 8], [64, 5000], [0, 64], [1001, 1002], [100, 32900]], dtype=np.uint32)
    det = detector_batch()
    cal = np.tile(np.array([0.0, 1.0], dtype=np.float32), (len(det.dec), 1))
    for bb, trim, r, sc in ((b, None, rng, None), (det, press.trim_adaptor(ADAPTOR), None, None), (det, press.trim_segment(SEGMENT), None, cal)):
        for dtype, rule, cap in (("float16", RULE, None), ("float32", None, 7), ("bfloat16", RULE, 0)):
            g = run(bb, 64, 5, dtype, rule, trim=trim, ranges=r, seg_cal=sc, cap=cap)
            rows, first, rr, rs, cut, q, on = press.depress_chunks_trimmed_batch_host(bb.m, bb.streams, bb.rooms, 64, 5, dtype=dtype, trim=trim,
                                                                                      ranges=r, seg_cal=sc, rule=rule, nrows_cap=cap)
            w = min(int(first[-1]), g["cap"])
            assert rows.shape == (w, 64) and len(rr) == w and len(rs) == w
            assert np.array_equal(bits_of(rows), g["rows"][:w]) and np.array_equal(first, g["row_first"])
            assert np.array_equal(rr, g["row_read"][:w]) and np.array_equal(rs, g["row_start"][:w])
            assert np.array_equal(cut, g["cut"]) and np.array_equal(q, g["q"]) and np.array_equal(on, g["out_n"])


@gpu
def test_no_reads(lib):
    d_first = torch.full((2,), FILL, dtype=torch.int64, device="cuda")
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    press.depress_chunks_trimmed_batch(YARD, torch.zeros(64, dtype=torch.uint8, device="cuda"), e, e, None, d_first, e,
                                       torch.zeros(0, dtype=torch.int32, device="cuda"), 0, torch.zeros(0, dtype=torch.int32, device="cuda"), 0, T=8)
    torch.cuda.synchronize()
    assert d_first.cpu().tolist() == [0, FILL]
    rows, first, rr, rs, cut, q, on = press.depress_chunks_trimmed_batch_host(YARD, [], [], 8, 0)
    assert first.tolist() == [0] and rows.shape == (0, 8) and cut.shape == (0, 2)
