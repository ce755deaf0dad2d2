"""The stream contract of the device-resident calls: they only enqueue on the current stream, press_hip_set_stream /
press_hip_reset_stream choose that stream, and a table change is ordered against it (include/press_hip.h).

The other GPU modules run on the null stream behind blocking copies, where work on a wrong stream, a hidden host wait or
context state changed under an enqueued batch all still come out right.  Here the stream under test is HELD: a delay of
HOLD_MS is enqueued on it and an event recorded behind the delay, so whatever is enqueued on that stream afterwards cannot
start before the delay ends, while work that lands on any other stream starts at once.  Every test asserts that the event
is still pending at the moment its premise needs it; a delay that ended early is a failure, never a pass.

The decoy: two batches D and R with the same n[], off[] and slots and different samples (two seeds of _layouts._walk).
Step 0, synchronised, runs the call chain on D, so that every output tensor holds D's valid results.  Step 1, behind the
hold and with no host synchronisation before its end: a torch copy on the stream replaces the inputs by R's, the library
calls follow, torch clones of the outputs follow them, and one stream.synchronize() ends it.  Every output must be R's:
what ran on another stream ran ahead of the delay, on D's data, and shows.  D is valid data in R's layout, so no
misordering takes a kernel out of bounds.

Expected values are the oracle's (_layouts.expect_press / expect_depress / check_zstd_frame) and the numpy definitions of
the picoampere, median / MAD and symbol-count tests; never a second run of the library.  The range coders store the two
reads of 64 and 65 samples raw (TurboRC rcutil_.h:161), outside the reference's lossless domain: their streams are still
the oracle's byte for byte, and their decode is compared with the oracle's decoder, as the layout battery does.

Measured on one MI355X: the longest enqueue sequence takes well under HOLD_MS / 20 of host time.
"""
import ctypes
import time

import numpy as np
import pytest

import _layouts as L
import _libs
import test_gpu_parity as PAR  # TABLES, _canonical_table, _write_table
from honours_amd import press
from test_depress_pa import batch_cal, pa_bits
from test_press_packed import layout_of, rc_need
from test_signal_stats import norm_bits, ref_stats
from test_table_training import zd_counts

HOLD_MS = 50.0  # the delay; at least 20 times the host time of the longest enqueue sequence, at most 250 ms
NS = (64, 65, 2049, 32769, 70001)  # tile and two-tile edges, more than one block; none empty, none under 64 samples
NR = len(NS)
SEEDS = {"D": 1, "R": 3}  # every stream length, decode and {median, MAD} differs between the two (test_decoy_...)
METHODS = sorted(press.METHODS, key=lambda m: press.METHODS[m])
SHUFF = [m for m in METHODS if m.startswith("shuffman_")]
FAMILIES = ("slow5_svb_zd", "vbe21_zd", "shuffman_vbe21_zd", "rc_vbe21_zd", "zstd_svb_zd")
RECODE_PAIRS = (("slow5_svb_zd", "shuffman_vbe21_zd"), ("rc_vbe21_zd", "vbe21_zd"))  # recode_fused: yes, no
ALIGN = 16
STREAM_KINDS = ("private", "torch", "null")


# ------------------------------------------------------------------ the two batches and what the oracle makes of them

def _reads(which):
    rng = np.random.default_rng(SEEDS[which])
    return [L._walk(rng, n, 0.01) for n in NS]


READS = {w: _reads(w) for w in ("D", "R")}
OFF = np.concatenate([[0], np.cumsum([L.roundup8(n) for n in NS])[:-1]]).astype(np.uint64)
TOTAL = int(sum(L.roundup8(n) for n in NS)) + 64  # the extent every call is given
_memo = {}


def host_sig(which):
    sig = np.zeros(TOTAL, dtype=np.int16)
    for s, o in zip(READS[which], OFF):
        sig[int(o):int(o) + len(s)] = s
    return sig


def slot_sizes(oracle, m):
    return [L.slot_of(oracle.bound, m, n) for n in NS]


def slot_table(oracle, m):
    """slots from _layouts.slot_of: they depend on n only, so D and R share them; out_off[0] is odd"""
    return L.slots(np.random.default_rng(5), slot_sizes(oracle, m))


def want(oracle, which, m):
    """the oracle's streams of the batch under the DEFAULT table (the zstd kinds: the frames' content)"""
    key = ("st", which, m)
    if key not in _memo:
        sts = [L.expect_press(oracle, m, s, c) for s, c in zip(READS[which], slot_sizes(oracle, m))]
        assert all(st is not None for st in sts), m
        _memo[key] = sts
    return _memo[key]


def is_raw(m, st, n):
    return m in _libs.RC_FAMILY and _libs.rc_stored_raw(m, st, n)


def decoded(oracle, which, m):
    """what the oracle's decoder makes of those streams: the reads, except for a range-coder stream stored raw"""
    key = ("dec", which, m)
    if key not in _memo:
        out = []
        for s, st in zip(READS[which], want(oracle, which, m)):
            if m in L.ZSTD_KINDS:
                out.append(s)
                continue
            verdict, back = L.expect_depress(oracle, m, s, st, len(s))
            assert verdict == "ok", (m, len(s))
            assert is_raw(m, st, len(s)) or np.array_equal(back, s), (m, len(s))
            out.append(back)
        _memo[key] = out
    return _memo[key]


def want_need(oracle, m, sts, ns):
    """press_hip_press_sizes' figure (include/press_hip.h): the stream's length, the range coders' slot; None for the
    zstd kinds, whose bytes are not pinned"""
    if m in L.ZSTD_KINDS:
        return None
    if m in _libs.RC_FAMILY:
        return [rc_need(m, st, n) for st, n in zip(sts, ns)]
    return [len(st) for st in sts]


def recode_want(oracle, which, src, dst):
    """-> (decoded samples of the source streams, the oracle's dst streams of them)"""
    key = ("rec", which, src, dst)
    if key not in _memo:
        dec = decoded(oracle, which, src)
        sts = [L.expect_press(oracle, dst, s, L.slot_of(oracle.bound, dst, len(s))) for s in dec]
        assert all(st is not None for st in sts), (src, dst)
        _memo[key] = (dec, sts)
    return _memo[key]


# ------------------------------------------------------------------ without a GPU: a stale result cannot pass

def test_decoy_differs_in_every_read(oracle):
    """every read of D and R differs in its samples, its {median, MAD}, and under all 19 methods in its stream's bytes,
    its stream's length and what the oracle decodes; only range-coder reads of 64 and 65 samples are stored raw"""
    for r in range(NR):
        assert len(READS["D"][r]) == len(READS["R"][r]) == NS[r]
        assert not np.array_equal(READS["D"][r], READS["R"][r])
        assert ref_stats(READS["D"][r]) != ref_stats(READS["R"][r]), r
    assert not np.array_equal(zd_counts(READS["D"]), zd_counts(READS["R"]))
    for m in METHODS:
        for r, (a, b) in enumerate(zip(want(oracle, "D", m), want(oracle, "R", m))):
            assert a != b and len(a) != len(b), (m, r)
        for r, (a, b) in enumerate(zip(decoded(oracle, "D", m), decoded(oracle, "R", m))):
            assert len(a) == len(b) == NS[r] and not np.array_equal(a, b), (m, r)
        for which in ("D", "R"):
            raw = [NS[r] for r, st in enumerate(want(oracle, which, m)) if is_raw(m, st, NS[r])]
            assert raw == ([64, 65] if m in _libs.RC_FAMILY else []), (m, which, raw)
        need = [want_need(oracle, m, want(oracle, w, m), NS) for w in ("D", "R")]
        if need[0] is not None:
            assert all(a != b for a, b in zip(*need)), m
            assert not np.array_equal(layout_of(need[0], ALIGN), layout_of(need[1], ALIGN)), m
    for src, dst in RECODE_PAIRS:
        d, r = recode_want(oracle, "D", src, dst)[1], recode_want(oracle, "R", src, dst)[1]
        assert all(a != b and len(a) != len(b) for a, b in zip(d, r)), (src, dst)


@pytest.fixture(scope="module")
def tables(oracle, tmp_path_factory):
    """table A is the default one, table B gives all 256 symbols a code (long_codes: second-level tables and the trie
    walk) -> the oracle's streams of R under either, per shuffman_* method"""
    lens = PAR.TABLES["long_codes"]
    bits = PAR._canonical_table(lens)
    path = str(tmp_path_factory.mktemp("tables") / "long_codes.huffman")
    PAR._write_table(path, lens, bits)
    a_codes = oracle.table()
    t = {"A": {"path": _libs.TABLE, "len": [c[0] for c in a_codes], "bits": [c[1] for c in a_codes]},
         "B": {"path": path, "len": list(lens), "bits": list(bits)}}
    t["A"]["want"] = {m: want(oracle, "R", m) for m in SHUFF}
    try:
        oracle.load_table(path)
        assert oracle.table() == list(zip(lens, bits)) and all(ln > 0 for ln in lens)
        t["B"]["want"] = {m: [L.expect_press(oracle, m, s, c) for s, c in zip(READS["R"], slot_sizes(oracle, m))]
                          for m in SHUFF}
        for m in SHUFF:
            for s, st in zip(READS["R"], t["B"]["want"][m]):
                assert st is not None and L.expect_depress(oracle, m, s, st, len(s))[0] == "ok", m
    finally:
        oracle.load_table()
    return t


def test_tables_differ_in_every_read(tables):
    """a batch coded with the wrong table cannot pass: under A and B every read's stream differs"""
    for m in SHUFF:
        for r, (a, b) in enumerate(zip(tables["A"]["want"][m], tables["B"]["want"][m])):
            assert a != b, (m, r)


# ------------------------------------------------------------------ GPU plumbing

ENQUEUE_MS = {}  # host time of every held enqueue sequence, for DESIGN.md


@pytest.fixture(scope="module")
def lib(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    lb.press_hip_scratch_buffers.restype = ctypes.c_uint32
    lb.press_hip_scratch_buffers.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    lb.press_hip_set_table.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    press.load_table()
    press.use_torch_stream()
    try:
        yield lb
    finally:
        # as the other GPU modules set the library up: torch's default stream, the default table on both sides
        torch.cuda.synchronize()
        press.use_torch_stream()
        press.use_table()
        oracle.load_table()
        if ENQUEUE_MS:
            k = max(ENQUEUE_MS, key=ENQUEUE_MS.get)
            print("\nlongest held enqueue sequence: %s, %.3f ms of host time; the delay is %.0f ms (%.0f times that)"
                  % (k, ENQUEUE_MS[k], HOLD_MS, HOLD_MS / ENQUEUE_MS[k]))
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def cycles_per_ms(lib):
    """torch.cuda._sleep's unit, measured once with two events"""
    import torch
    torch.cuda._sleep(100000)
    torch.cuda.synchronize()
    cycles = 2000000
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 5.0:
            break
        cycles *= 10
    assert ms >= 5.0, "torch.cuda._sleep(%d) took %.3f ms" % (cycles, ms)
    return cycles / ms


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


def use_stream(lib, kind):
    """make a stream of this kind the library's current one -> the torch stream object that stands for it"""
    import torch
    if kind == "private":
        assert lib.press_hip_reset_stream() == 0
        h = lib.press_hip_get_stream()
        assert h, press.last_error()
        return torch.cuda.ExternalStream(h)
    if kind == "torch":
        s = torch.cuda.Stream()
        assert s.cuda_stream != 0
        assert lib.press_hip_set_stream(ctypes.c_void_p(s.cuda_stream)) == 0
        return s
    s = torch.cuda.default_stream()
    assert s.cuda_stream == 0
    assert lib.press_hip_set_stream(None) == 0
    return s


def hold(stream, cycles_per_ms, ms=HOLD_MS):
    """a delay on `stream` and the event behind it"""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms))
        e = torch.cuda.Event()
        e.record(stream)
    return e


EARLY = "the delay of %g ms ended before the premise was checked" % HOLD_MS
WAITED = "a call that promises only to enqueue waited for the stream (or the delay of %g ms ended early)" % HOLD_MS


def decoy_run(name, stream, cycles_per_ms, load, steps, outputs):
    """Step 0 on D, synchronised; step 1 on R behind a hold.  load(which): torch ops that put the batch's inputs in
    place; steps: [(callable, documented_host_wait)], run in order; outputs: tensors that are cloned on the stream.
    -> the clones as numpy arrays.  Every step that is not behind a documented wait must leave the hold pending."""
    import torch
    with torch.cuda.stream(stream):
        load("D")
        for fn, _ in steps:
            fn()
    torch.cuda.synchronize()
    e = hold(stream, cycles_per_ms)
    t0 = time.perf_counter()
    waited = False
    with torch.cuda.stream(stream):
        load("R")
        for fn, documented_wait in steps:
            fn()
            waited = waited or documented_wait
            assert waited or not e.query(), name + ": " + WAITED
        clones = [o.clone() for o in outputs]
        t1 = time.perf_counter()
        assert waited or not e.query(), name + ": " + EARLY
    stream.synchronize()
    assert e.query()
    if not waited:
        ENQUEUE_MS[name] = (t1 - t0) * 1e3
        print("%s: %.3f ms of host time for the held sequence" % (name, ENQUEUE_MS[name]))
    return [c.cpu().numpy() for c in clones]


class Samples:
    """the sample side of the two batches on the device: D, R and the tensor the calls read"""

    def __init__(self):
        import torch
        self.src = {w: _t(host_sig(w)) for w in ("D", "R")}
        self.sig = torch.zeros(TOTAL, dtype=torch.int16, device="cuda")
        self.off = _t(OFF, np.int64)
        self.n = _t(np.array(NS, dtype=np.uint32), np.int32)

    def load(self, which):
        self.sig.copy_(self.src[which], non_blocking=True)


class Slots:
    """an output arena with the slots of method m"""

    def __init__(self, oracle, m):
        import torch
        self.out_off = slot_table(oracle, m)
        self.d_out_off = _t(self.out_off, np.int64)
        self.in_off = self.d_out_off[:-1].contiguous()
        self.arena = torch.full((int(self.out_off[-1]) + 64,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
        self.out_len = torch.full((NR,), -7, dtype=torch.int64, device="cuda")


class Streams:
    """the oracle's streams of both batches in the slots of method m, and the arena / in_len the calls read"""

    def __init__(self, oracle, m):
        import torch
        self.out_off = slot_table(oracle, m)
        self.in_off = _t(self.out_off[:-1], np.int64)
        self.src = {}
        for w in ("D", "R"):
            a = np.zeros(int(self.out_off[-1]) + 64, dtype=np.uint8)
            sts = want(oracle, w, m)
            for st, o in zip(sts, self.out_off):
                a[int(o):int(o) + len(st)] = np.frombuffer(st, dtype=np.uint8)
            self.src[w] = (_t(a), _t(np.array([len(st) for st in sts], dtype=np.uint64), np.int64))
        self.arena = torch.zeros_like(self.src["D"][0])
        self.in_len = torch.zeros_like(self.src["D"][1])

    def load(self, which):
        self.arena.copy_(self.src[which][0], non_blocking=True)
        self.in_len.copy_(self.src[which][1], non_blocking=True)


@pytest.fixture(scope="module")
def samples(lib):
    return Samples()


def check_streams(oracle, m, reads, sts, arena, out_off, out_len):
    """the streams in the arena are the oracle's (the zstd kinds: frames that hold the oracle's content)"""
    out_len = out_len.view(np.uint64)
    for r in range(NR):
        ln, o = int(out_len[r]), int(out_off[r])
        assert ln != L.FAILED64, (m, r)
        got = arena[o:o + ln].tobytes()
        if m in L.ZSTD_KINDS:
            L.check_zstd_frame(oracle, m, reads[r], got, sts[r])
        else:
            assert ln == len(sts[r]) and got == sts[r], (m, r, ln, len(sts[r]))


def check_samples(m, dec, back, out_n):
    out_n = out_n.view(np.uint32)
    for r in range(NR):
        assert int(out_n[r]) == len(dec[r]), (m, r, int(out_n[r]))
        assert np.array_equal(back[int(OFF[r]):int(OFF[r]) + len(dec[r])], dec[r]), (m, r)


# ------------------------------------------------------------------ 1. stream selection

@pytest.mark.gpu
def test_stream_selection(lib):
    import torch
    assert lib.press_hip_reset_stream() == 0
    own = lib.press_hip_get_stream()
    fresh = torch.cuda.Stream()
    assert own and own != fresh.cuda_stream
    assert lib.press_hip_set_stream(ctypes.c_void_p(fresh.cuda_stream)) == 0
    assert lib.press_hip_get_stream() == fresh.cuda_stream
    assert lib.press_hip_set_stream(None) == 0
    assert lib.press_hip_get_stream() is None
    assert lib.press_hip_reset_stream() == 0
    assert lib.press_hip_get_stream() == own


@pytest.mark.gpu
def test_hold_is_as_long_as_asked(lib, cycles_per_ms):
    """the device the other tests rest on: the delay lasts HOLD_MS, give or take a quarter, and at most 250 ms"""
    import torch
    s = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        a.record(s)
        torch.cuda._sleep(int(HOLD_MS * cycles_per_ms))
        b.record(s)
    b.synchronize()
    ms = a.elapsed_time(b)
    print("a delay of %g ms took %.1f ms; %.0f cycles per ms" % (HOLD_MS, ms, cycles_per_ms))
    assert 0.75 * HOLD_MS <= ms <= min(1.25 * HOLD_MS, 250.0), ms


@pytest.mark.gpu
@pytest.mark.parametrize("kind", STREAM_KINDS)
def test_synchronize_waits_for_the_current_stream(lib, cycles_per_ms, kind):
    s = use_stream(lib, kind)
    e = hold(s, cycles_per_ms)
    assert not e.query(), EARLY
    assert lib.press_hip_synchronize() == 0
    assert e.query(), "press_hip_synchronize returned with the current stream still busy"


# ------------------------------------------------------------------ 2. press and depress on the current stream

@pytest.mark.gpu
@pytest.mark.parametrize("kind", STREAM_KINDS)
@pytest.mark.parametrize("m", METHODS)
def test_press_depress_on_the_current_stream(lib, oracle, samples, cycles_per_ms, m, kind):
    """press_batch, then depress_batch of the arena and out_len that press just produced, behind a hold; a zstd
    depress waits on the host for its frame walk (include/press_hip.h), so there the hold is checked after the press"""
    import torch
    s = use_stream(lib, kind)
    x, sl = samples, Slots(oracle, m)
    back = torch.full((TOTAL,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    out_n = torch.full((NR,), -7, dtype=torch.int32, device="cuda")
    steps = [(lambda: press.press_batch(m, x.sig, x.off, x.n, sl.arena, sl.d_out_off, sl.out_len), False),
             (lambda: press.depress_batch(m, sl.arena, sl.in_off, sl.out_len, back, x.off, x.n, out_n), m in L.ZSTD_KINDS)]
    arena, out_len, bk, on = decoy_run("press+depress %s %s" % (m, kind), s, cycles_per_ms, x.load, steps,
                                       [sl.arena, sl.out_len, back, out_n])
    check_streams(oracle, m, READS["R"], want(oracle, "R", m), arena, sl.out_off, out_len)
    check_samples(m, decoded(oracle, "R", m), bk, on)


# ------------------------------------------------------------------ 3. the other device-resident calls

@pytest.mark.gpu
@pytest.mark.parametrize("m", FAMILIES)
def test_press_sizes_on_the_current_stream(lib, oracle, samples, cycles_per_ms, m):
    import torch
    s = use_stream(lib, "torch")
    x = samples
    need = torch.full((NR,), -7, dtype=torch.int64, device="cuda")

    def call():
        rc = lib.press_hip_press_sizes(press.METHODS[m], x.sig.data_ptr(), x.off.data_ptr(), x.n.data_ptr(), NR, TOTAL,
                                       need.data_ptr(), 1)
        assert rc == 0, press.last_error()
    wn = want_need(oracle, m, want(oracle, "R", m), NS)
    if wn is not None:
        got, = decoy_run("press_sizes " + m, s, cycles_per_ms, x.load, [(call, False)], [need])
        assert [int(v) for v in got] == wn, m
        return
    # a frame's bytes are not pinned, so no oracle gives its length: the header defines need[r] as the length of the
    # stream press_batch writes, so a press_batch follows in the same held sequence, its frames are checked to hold the
    # oracle's content, and need[r] must be their lengths
    sl = Slots(oracle, m)
    steps = [(call, False), (lambda: press.press_batch(m, x.sig, x.off, x.n, sl.arena, sl.d_out_off, sl.out_len), False)]
    got, arena, out_len = decoy_run("press_sizes " + m, s, cycles_per_ms, x.load, steps, [need, sl.arena, sl.out_len])
    check_streams(oracle, m, READS["R"], want(oracle, "R", m), arena, sl.out_off, out_len)
    assert np.array_equal(got, out_len), m


@pytest.mark.gpu
@pytest.mark.parametrize("m", FAMILIES)
def test_press_packed_on_the_current_stream(lib, oracle, samples, cycles_per_ms, m):
    import torch
    s = use_stream(lib, "torch")
    x, sl = samples, Slots(oracle, m)
    oo = torch.full((NR + 1,), -7, dtype=torch.int64, device="cuda")
    steps = [(lambda: press.press_packed(m, x.sig, x.off, x.n, sl.arena, oo, sl.out_len, align=ALIGN), False)]
    arena, out_off, out_len = decoy_run("press_packed " + m, s, cycles_per_ms, x.load, steps, [sl.arena, oo, sl.out_len])
    sts = want(oracle, "R", m)
    check_streams(oracle, m, READS["R"], sts, arena, out_off.view(np.uint64), out_len)
    wn = want_need(oracle, m, sts, NS)  # (the zstd kinds: the layout the frames' own lengths give)
    assert np.array_equal(out_off.view(np.uint64), layout_of(wn if wn is not None else out_len.view(np.uint64), ALIGN)), m


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", RECODE_PAIRS)
@pytest.mark.parametrize("call", ["batch", "sizes", "packed"])
def test_recode_on_the_current_stream(lib, oracle, cycles_per_ms, call, src, dst):
    import torch
    assert press.recode_fused(src, dst) == (src == "slow5_svb_zd")
    s = use_stream(lib, "torch")
    st, sl = Streams(oracle, src), Slots(oracle, dst)
    n, off = _t(np.array(NS, dtype=np.uint32), np.int32), _t(OFF, np.int64)
    back = torch.full((TOTAL,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    out_n = torch.full((NR,), -7, dtype=torch.int32, device="cuda")
    oo = torch.full((NR + 1,), -7, dtype=torch.int64, device="cuda")
    need = torch.full((NR,), -7, dtype=torch.int64, device="cuda")

    def sizes():
        rc = lib.press_hip_recode_sizes(press.METHODS[src], press.METHODS[dst], st.arena.data_ptr(), st.in_off.data_ptr(),
                                        st.in_len.data_ptr(), n.data_ptr(), off.data_ptr(), NR, TOTAL, need.data_ptr(),
                                        back.data_ptr(), out_n.data_ptr(), 1)
        assert rc == 0, press.last_error()
    fn = {"batch": lambda: press.recode_batch(src, dst, st.arena, st.in_off, st.in_len, n, off, sl.arena, sl.d_out_off,
                                              sl.out_len, out_n, sig=back),
          "sizes": sizes,
          "packed": lambda: press.recode_packed(src, dst, st.arena, st.in_off, st.in_len, n, off, sl.arena, oo, sl.out_len,
                                                out_n, sig=back, align=ALIGN)}[call]
    arena, out_len, bk, on, out_off, nd = decoy_run("recode_%s %s>%s" % (call, src, dst), s, cycles_per_ms, st.load,
                                                    [(fn, False)], [sl.arena, sl.out_len, back, out_n, oo, need])
    dec, sts = recode_want(oracle, "R", src, dst)
    check_samples(src, dec, bk, on)
    wn = want_need(oracle, dst, sts, [len(d) for d in dec])
    if call == "sizes":
        assert [int(v) for v in nd] == wn
        return
    if call == "packed":
        assert np.array_equal(out_off.view(np.uint64), layout_of(wn, ALIGN))
    check_streams(oracle, dst, dec, sts, arena, sl.out_off if call == "batch" else out_off.view(np.uint64), out_len)


@pytest.mark.gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "vbe21_zd"])
def test_depress_pa_on_the_current_stream(lib, oracle, cycles_per_ms, m):
    import torch
    assert press.depress_pa_fused(m) == (m == "slow5_svb_zd")
    s = use_stream(lib, "torch")
    st = Streams(oracle, m)
    n, off = _t(np.array(NS, dtype=np.uint32), np.int32), _t(OFF, np.int64)
    cal = batch_cal(NR)
    d_cal = _t(cal.reshape(-1))
    pa = torch.zeros(TOTAL, dtype=torch.float32, device="cuda")
    out_n = torch.full((NR,), -7, dtype=torch.int32, device="cuda")
    steps = [(lambda: press.depress_pa_batch(m, st.arena, st.in_off, st.in_len, pa, off, n, d_cal, out_n), False)]
    got, on = decoy_run("depress_pa " + m, s, cycles_per_ms, st.load, steps, [pa, out_n])
    for r, d in enumerate(decoded(oracle, "R", m)):
        assert int(on.view(np.uint32)[r]) == len(d), (m, r)
        bits = got[int(OFF[r]):int(OFF[r]) + len(d)].view(np.uint32)
        assert np.array_equal(bits, pa_bits(d, cal[r, 0], cal[r, 1])), (m, r)


@pytest.mark.gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "shuffman_vbe21_zd"])
def test_depress_norm_on_the_current_stream(lib, oracle, cycles_per_ms, m):
    import torch
    s = use_stream(lib, "torch")
    st = Streams(oracle, m)
    n, off = _t(np.array(NS, dtype=np.uint32), np.int32), _t(OFF, np.int64)
    out = torch.zeros(TOTAL, dtype=torch.float32, device="cuda")
    out_n = torch.full((NR,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((2 * NR,), -7, dtype=torch.int32, device="cuda")
    steps = [(lambda: press.depress_norm_batch(m, st.arena, st.in_off, st.in_len, out, off, n, out_n, stats), False)]
    got, on, sg = decoy_run("depress_norm " + m, s, cycles_per_ms, st.load, steps, [out, out_n, stats])
    for r, d in enumerate(decoded(oracle, "R", m)):
        med, mad = ref_stats(d)
        assert int(on.view(np.uint32)[r]) == len(d) and (int(sg[2 * r]), int(sg[2 * r + 1])) == (med, mad), (m, r)
        bits = got[int(OFF[r]):int(OFF[r]) + len(d)].view(np.uint32)
        assert np.array_equal(bits, norm_bits(d, med, mad)), (m, r)


@pytest.mark.gpu
def test_signal_stats_on_the_current_stream(lib, samples, cycles_per_ms):
    import torch
    s = use_stream(lib, "torch")
    x = samples
    stats = torch.full((2 * NR,), -7, dtype=torch.int32, device="cuda")
    got, = decoy_run("signal_stats", s, cycles_per_ms, x.load, [(lambda: press.signal_stats(x.sig, x.off, x.n, stats), False)],
                     [stats])
    assert [(int(got[2 * r]), int(got[2 * r + 1])) for r in range(NR)] == [ref_stats(d) for d in READS["R"]]


@pytest.mark.gpu
def test_symbol_counts_on_the_current_stream(lib, samples, cycles_per_ms):
    """press_hip_symbol_counts ADDS: the zeroing of the counts is a torch op on the stream, in front of the call"""
    import torch
    s = use_stream(lib, "torch")
    x = samples
    counts = torch.zeros(press.NBINS, dtype=torch.int64, device="cuda")

    def load(which):
        x.load(which)
        counts.zero_()
    got, = decoy_run("symbol_counts", s, cycles_per_ms, load, [(lambda: press.symbol_counts(x.sig, x.off, x.n, counts), False)],
                     [counts])
    assert np.array_equal(got.view(np.uint64), zd_counts(READS["R"]))


# ------------------------------------------------------------------ 5. a table switch behind batches in flight

def switch_table(lib, oracle, how, tab):
    """make `tab` the library's table: by file, by the raw pairs, or as the caller-owned table of a per-read call"""
    if how == "file":
        assert lib.press_hip_load_table_file(tab["path"].encode()) == 0, press.last_error()
    elif how == "raw":
        ln, bits = np.array(tab["len"], dtype=np.uint32), np.array(tab["bits"], dtype=np.uint64)
        assert lib.press_hip_set_table(ln.ctypes.data, bits.ctypes.data) == 0, press.last_error()
    else:
        m, s = "shuffman_vbe21_zd", READS["R"][0]
        t = press.HuffmanTable(tab["path"])
        try:
            cap = len(tab["want"][m][0]) + 64
            out = np.zeros(cap + 64, dtype=np.uint8)
            nout = ctypes.c_uint64(cap)
            fn = lib.shuffman_vbe21_zd_press_16
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
            assert fn(t.se, s.ctypes.data, s.size, out.ctypes.data, ctypes.byref(nout)) == 0, press.last_error()
            assert out[:nout.value].tobytes() == tab["want"][m][0]
        finally:
            t.close()


def table_press(lib, oracle, samples, cycles_per_ms, tables, m, kind, how):
    """A in force, the stream held: press into out1; B by `how`; press into out2 -> (stream, out1, out2), not
    synchronised"""
    import torch
    switch_table(lib, oracle, "file", tables["A"])
    s = use_stream(lib, kind)
    x, o1, o2 = samples, Slots(oracle, m), Slots(oracle, m)
    with torch.cuda.stream(s):
        x.load("R")
    torch.cuda.synchronize()
    e = hold(s, cycles_per_ms)
    with torch.cuda.stream(s):
        press.press_batch(m, x.sig, x.off, x.n, o1.arena, o1.d_out_off, o1.out_len)
    assert not e.query(), EARLY
    switch_table(lib, oracle, how, tables["B"])
    with torch.cuda.stream(s):
        press.press_batch(m, x.sig, x.off, x.n, o2.arena, o2.d_out_off, o2.out_len)
    return s, o1, o2


def check_table_streams(oracle, tables, m, o, name, other):
    arena, out_len = o.arena.cpu().numpy(), o.out_len.cpu().numpy()
    ln = [int(v) for v in out_len.view(np.uint64)]
    got = [arena[int(a):int(a) + k].tobytes() if k != L.FAILED64 else None for a, k in zip(o.out_off, ln)]
    if got == tables[other]["want"][m]:
        pytest.fail("%s: the batch enqueued under table %s carries table %s's bytes" % (m, name, other))
    check_streams(oracle, m, READS["R"], tables[name]["want"][m], arena, o.out_off, out_len)


TABLE_CASES = [(m, kind, how) for kind in ("private", "torch") for m in SHUFF for how in ("file", "raw", "dropin")]


@pytest.mark.gpu
@pytest.mark.parametrize("m,kind,how", TABLE_CASES)
def test_table_switch_behind_a_batch_press(lib, oracle, samples, cycles_per_ms, tables, m, kind, how):
    """a batch enqueued before the table changes is coded with the old table, the batch behind the change with the new"""
    try:
        s, o1, o2 = table_press(lib, oracle, samples, cycles_per_ms, tables, m, kind, how)
        s.synchronize()
        check_table_streams(oracle, tables, m, o1, "A", "B")
        check_table_streams(oracle, tables, m, o2, "B", "A")
    finally:
        import torch
        torch.cuda.synchronize()
        oracle.load_table()
        press.use_table()


@pytest.mark.gpu
@pytest.mark.parametrize("m,kind,how", TABLE_CASES)
def test_table_switch_behind_a_batch_roundtrip(lib, oracle, samples, cycles_per_ms, tables, m, kind, how):
    """... and the same for decoding: out2 is decoded under B with the switch back to A behind it in flight, then out1"""
    import torch
    try:
        s, o1, o2 = table_press(lib, oracle, samples, cycles_per_ms, tables, m, kind, how)
        back1, back2 = (torch.full((TOTAL,), L.SIG_FILL, dtype=torch.int16, device="cuda") for _ in range(2))
        n1, n2 = (torch.full((NR,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        x = samples
        s.synchronize()
        e = hold(s, cycles_per_ms)
        with torch.cuda.stream(s):
            press.depress_batch(m, o2.arena, o2.in_off, o2.out_len, back2, x.off, x.n, n2)
        assert not e.query(), EARLY
        switch_table(lib, oracle, how, tables["A"])
        with torch.cuda.stream(s):
            press.depress_batch(m, o1.arena, o1.in_off, o1.out_len, back1, x.off, x.n, n1)
        s.synchronize()
        check_table_streams(oracle, tables, m, o1, "A", "B")
        check_table_streams(oracle, tables, m, o2, "B", "A")
        check_samples(m, READS["R"], back2.cpu().numpy(), n2.cpu().numpy())
        check_samples(m, READS["R"], back1.cpu().numpy(), n1.cpu().numpy())
    finally:
        torch.cuda.synchronize()
        oracle.load_table()
        press.use_table()


# ------------------------------------------------------------------ 6. scratch growth behind a batch in flight

@pytest.mark.gpu
@pytest.mark.parametrize("m", ["vbe21_zd", "shuffman_vbe21_zd"])
def test_scratch_growth_behind_a_batch(lib, oracle, samples, cycles_per_ms, m):
    """DevBuf::reserve frees a buffer that an enqueued batch may still use and relies on hipFree's documented implicit
    device synchronisation: a small batch in flight, then one of more than four times the samples, both exact"""
    import torch
    big_reads = [L._walk(np.random.default_rng(7), n, 0.01) for n in (200001, 150003, 100001)]
    assert sum(len(r) for r in big_reads) >= 4 * sum(NS)
    boff = np.concatenate([[0], np.cumsum([L.roundup8(len(r)) for r in big_reads])[:-1]]).astype(np.uint64)
    btotal = int(sum(L.roundup8(len(r)) for r in big_reads)) + 64
    bsig = np.zeros(btotal, dtype=np.int16)
    for r, o in zip(big_reads, boff):
        bsig[int(o):int(o) + len(r)] = r
    bcaps = [L.slot_of(oracle.bound, m, len(r)) for r in big_reads]
    bwant = [L.expect_press(oracle, m, r, c) for r, c in zip(big_reads, bcaps)]
    boo = L.slots(np.random.default_rng(9), bcaps)
    d_bsig, d_boff, d_bn = _t(bsig), _t(boff, np.int64), _t(np.array([len(r) for r in big_reads], dtype=np.uint32), np.int32)
    d_boo = _t(boo, np.int64)
    d_bin = d_boo[:-1].contiguous()
    barena = torch.full((int(boo[-1]) + 64,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
    blen = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    bback = torch.full((btotal,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    bn = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    x, sl = samples, Slots(oracle, m)
    back = torch.full((TOTAL,), L.SIG_FILL, dtype=torch.int16, device="cuda")
    out_n = torch.full((NR,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib.press_hip_shutdown()
    try:
        press.load_table()
        s = use_stream(lib, "torch")
        with torch.cuda.stream(s):
            x.load("R")
        torch.cuda.synchronize()
        nbytes = ctypes.c_uint64()
        e = hold(s, cycles_per_ms)
        with torch.cuda.stream(s):
            press.press_batch(m, x.sig, x.off, x.n, sl.arena, sl.d_out_off, sl.out_len)
            press.depress_batch(m, sl.arena, sl.in_off, sl.out_len, back, x.off, x.n, out_n)
        assert not e.query(), EARLY
        lib.press_hip_scratch_buffers(ctypes.byref(nbytes))
        small = nbytes.value
        with torch.cuda.stream(s):
            press.press_batch(m, d_bsig, d_boff, d_bn, barena, d_boo, blen)
            press.depress_batch(m, barena, d_bin, blen, bback, d_boff, d_bn, bn)
        lib.press_hip_scratch_buffers(ctypes.byref(nbytes))
        assert 0 < small < nbytes.value, "the second batch did not make the scratch grow"
        s.synchronize()
        check_streams(oracle, m, READS["R"], want(oracle, "R", m), sl.arena.cpu().numpy(), sl.out_off, sl.out_len.cpu().numpy())
        check_samples(m, READS["R"], back.cpu().numpy(), out_n.cpu().numpy())
        arena, ln = barena.cpu().numpy(), blen.cpu().numpy().view(np.uint64)
        got_back, got_n = bback.cpu().numpy(), bn.cpu().numpy().view(np.uint32)
        for r in range(3):
            assert arena[int(boo[r]):int(boo[r]) + int(ln[r])].tobytes() == bwant[r], (m, r)
            assert int(got_n[r]) == len(big_reads[r]), (m, r)
            assert np.array_equal(got_back[int(boff[r]):int(boff[r]) + len(big_reads[r])], big_reads[r]), (m, r)
    finally:
        torch.cuda.synchronize()
        press.load_table()


# ------------------------------------------------------------------ 7. a host-pointer call on a held user stream

@pytest.mark.gpu
@pytest.mark.parametrize("m", ["svb12_zd", "shuffman_vbe21_zd", "zstd_svb_zd"])
def test_host_pointer_calls_wait_for_a_held_stream(lib, oracle, cycles_per_ms, m):
    """press_batch_host / depress_batch_host are synchronous on the current stream: right, and the hold is over"""
    s = use_stream(lib, "torch")
    reads = READS["R"]
    e = hold(s, cycles_per_ms)
    assert not e.query(), EARLY
    sts = press.press_batch_host(m, reads, caps=slot_sizes(oracle, m))
    assert e.query(), "press_batch_host returned with the stream still held"
    for r, st in enumerate(sts):
        assert st is not None, (m, r)
        if m in L.ZSTD_KINDS:
            L.check_zstd_frame(oracle, m, reads[r], st, want(oracle, "R", m)[r])
        else:
            assert st == want(oracle, "R", m)[r], (m, r)
    e = hold(s, cycles_per_ms)
    assert not e.query(), EARLY
    back = press.depress_batch_host(m, sts, [len(r) for r in reads])
    assert e.query(), "depress_batch_host returned with the stream still held"
    for r, b in enumerate(back):
        assert b is not None and np.array_equal(b, reads[r]), (m, r)
