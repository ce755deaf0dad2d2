"""The stall methods in the generic calls (include/press_hip.h section 2x): the method ids 96 .. 98 of rccm_svbbe21_zd,
dstall_fz_1500 and dstall_fz, and what press, sizes, packed, depress, recode, degrade, verify, CRC, picoampere, normalise and
chunk-row calls do with them.

No tolerance anywhere: bytes, bit patterns and integers.  What the device must give is fixed before the GPU sees anything:
* the streams: tests/_stall.py, the restatement that tests/test_stall_methods.py pins to the reference on
  tests/golden/ref_stall.json;
* floats, rows, first_bad and CRCs: the same call on vbe21_zd streams of the same reads, and zlib.

The reads are the fixture's (the three real reads, the threshold and truncation reads, the reads without a segment) with
an empty read in front, in the middle and at the end, and a read of n = 1.  The press runs add an empty guard read around
every one of them (test_stall_methods.PressRun).
"""
import ctypes
import os
import time
import zlib

import numpy as np
import pytest

import _layouts as L
import _libs
import _stall as S
import test_stall_methods as TS
import test_xmethods as TX
from honours_amd import abi, press

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "press_hip.h")
EARG = -2
F64, F32 = L.FAILED64, L.FAILED32
METHODS = S.STALL_METHODS
IDS = {"rccm_svbbe21_zd": 96, "dstall_fz_1500": 97, "dstall_fz": 98}
FILL8, FILL16, GUARD, CANARY = TS.FILL8, TS.FILL16, TS.GUARD, TS.CANARY
OVER = "gen/stall-piece-over-65535"
EMPTY = np.zeros(0, dtype=np.int16)
T_ROWS, OVERLAP = 4000, 200

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def batch():
    """[(name, samples)]: the fixture's reads, an empty read in front, in the middle and at the end, a read of n = 1"""
    def make():
        fx = list(TS.reads_by_name().items())
        mid = len(fx) // 2
        return [("empty-front", EMPTY)] + fx[:mid] + [("empty-middle", EMPTY)] + fx[mid:] + \
               [("n-1", np.array([-123], dtype=np.int16)), ("empty-end", EMPTY)]
    return memo("batch", make)


def names_of():
    return [n for n, _ in batch()]


def reads_of():
    return [s for _, s in batch()]


def want(method, bits=0):
    """the yardstick's streams of the batch (None: refused), of D_bits of the reads for bits > 0"""
    def make():
        out = []
        for name, s in batch():
            if bits:
                d = press.degrade(s, bits)
                out.append(S.expected(method, d, memo(("seg", bits, name), lambda: S.first_segment(d)))[0])
            elif name in TS.reads_by_name():
                out.append(TS.want(method, name)[0])
            else:
                out.append(S.expected(method, s)[0])
        return out
    return memo(("want", method, bits), make)


def decodable(method, bits=0):
    """the reads of the batch whose stream under `method` the decoder gives back (test_stall_methods.decodable)"""
    return [k for k, (st, s) in enumerate(zip(want(method, bits), reads_of())) if TS.decodable(st, len(s))]


def header_of(s):
    """(exists, stall_start, stall_len) of rccm_svbbe21_zd's stream for the samples s"""
    return S.stall_of(S.first_segment(s), 140)


def degrade_bits():
    """the smallest b in 1 .. 8 for which D_b moves the stall header of at least one fixture read"""
    def make():
        orig = {n: S.stall_of(TS.segment_of(n), 140) for n in TS.reads_by_name()}
        for b in range(1, 9):
            moved = [n for n, s in TS.reads_by_name().items() if header_of(press.degrade(s, b)) != orig[n]]
            if moved:
                return b, moved
        return None, []
    return memo("bits", make)


# ------------------------------------------------------------------ without a GPU

@pytest.fixture(scope="module")
def cpu_lib():
    from honours_amd import build
    build.build()
    return press.load_library()


def test_ids_and_their_inverse(cpu_lib):
    lib = cpu_lib
    for name, sm in press.STALL_METHODS.items():
        assert lib.press_hip_smethod(sm) == 96 + sm == IDS[name] == abi.SMETHODS[name] == press.smethod_id(name) == press.smethod_id(sm)
        got = ctypes.c_int(-9)
        assert lib.press_hip_smethod_parts(96 + sm, ctypes.byref(got)) == 0 and got.value == sm == press.smethod_parts(name)
        assert press._mid(name) == 96 + sm
    for bad in (-1, 3, 96, 1000):
        assert lib.press_hip_smethod(bad) == -1
    got = ctypes.c_int(-9)
    for bad in (95, 99, 88, 0, 1, 2, -1, 18, 64, 87, 1 << 20):
        assert lib.press_hip_smethod_parts(bad, ctypes.byref(got)) == EARG and got.value == -9, bad
    assert lib.press_hip_smethod_parts(96, None) == EARG and "NULL" in press.last_error()
    st, la = ctypes.c_int(-9), ctypes.c_int(-9)
    for mid in (96, 97, 98):
        assert lib.press_hip_xmethod_parts(mid, ctypes.byref(st), ctypes.byref(la)) == EARG
    with pytest.raises(press.PressError):
        press.smethod_parts(95)
    assert press.smethod_names() == list(METHODS) and press.SMETHODS is abi.SMETHODS and abi.SMETHOD_BASE == 96


def test_header_mirror_and_wrappers(cpu_lib):
    import inspect
    from honours_amd import smethod
    header = open(HEADER).read()
    flat = " ".join(header.split())
    assert "PRESS_HIP_SMETHOD_BASE = 96" in flat and "PRESS_HIP_NMETHODS = 19" in flat and "PRESS_HIP_NXSTAGES = 6" in flat
    assert "(2x) the stall methods in the generic calls" in header
    for s in ("press_hip_smethod", "press_hip_smethod_parts"):
        assert hasattr(cpu_lib, s) and s in abi.PROTOS and s in press.HEADER_SYMBOLS and s + "(" in header, s
    assert "press_hip_debug_stall_inner_presses" in abi._UNDECLARED and "press_hip_debug_stall_inner_presses" not in header
    assert hasattr(cpu_lib, "press_hip_debug_stall_inner_presses") and press.smethod_inner_presses() >= 0
    assert len(press.METHODS) == 19 and len(abi.XMETHODS) == 24 and len(abi.SMETHODS) == 3
    assert press.STALL_METHODS == {"rccm_svbbe21_zd": 0, "dstall_fz_1500": 1, "dstall_fz": 2}
    assert not set(press.STALL_METHODS) & set(press.METHODS) and not set(abi.SMETHODS) & set(abi.XMETHODS)
    public = sorted(n for n, f in vars(smethod).items() if not n.startswith("_") and inspect.isfunction(f) and f.__module__ == smethod.__name__)
    assert public == ["smethod_id", "smethod_inner_presses", "smethod_names", "smethod_parts"]
    for w in public:
        assert getattr(press, w) is getattr(smethod, w)


def test_bound_is_the_stall_bound(cpu_lib, oracle):
    for name, mid in IDS.items():
        for n in (1, 2, 7, 8, 9, 1000, 7329, 155185, 5724000):
            b = cpu_lib.press_hip_stall_bound(mid - 96, n)
            assert cpu_lib.press_hip_bound(mid, n) == b == press.bound(name, n) == oracle.bound("rccm_vbbe21_zd", n) > 0, (name, n)
    for bad in (95, 99, 88):
        assert cpu_lib.press_hip_bound(bad, 1000) == 0


def test_every_call_knows_the_stall_ids_and_no_others(cpu_lib):
    """95 and 99 are PRESS_HIP_EARG from every call that takes a method id, 96 .. 98 get past the argument check (an empty
    batch: OK with a device, the context's error without), with device_resident 0 and 1; the family's own calls keep 0 .. 2"""
    import torch
    for name, f in TX._calls(cpu_lib).items():
        for dr in (0, 1):
            for bad in (95, 99):
                assert f(bad, dr) == EARG and "method" in press.last_error(), (name, bad, dr)
            for mid in (96, 97, 98):
                # (with a device, a device-resident empty packed call writes out_off[0] through a device pointer: not these)
                if not (dr and "packed" in name and torch.cuda.is_available()):
                    assert f(mid, dr) != EARG, (name, mid, dr, press.last_error())
    a = np.zeros(64, dtype=np.uint64)
    p = a.ctypes.data
    for dr in (0, 1):
        for mid in (96, 97, 98):
            assert cpu_lib.press_hip_stall_press_batch(mid, p, p, p, 0, 0, p, p, p, p, dr) == EARG and "stall method" in press.last_error()
    assert cpu_lib.press_hip_stall_bound(96, 1000) == 0 and cpu_lib.press_hip_stall_workspace_bytes(98, 1000, 10) == 0


def test_exact_fused_and_workspace_questions(cpu_lib):
    lib = cpu_lib
    others = list(press.METHODS.values()) + list(range(64, 88)) + [96, 97, 98]
    for mid in (96, 97, 98):
        assert lib.press_hip_packed_exact(mid) == 1 and lib.press_hip_depress_pa_fused(mid) == 0 and press.packed_exact(mid)
        for o in others:
            assert lib.press_hip_recode_fused(mid, o) == 0 and lib.press_hip_recode_fused(o, mid) == 0, (mid, o)
    for bad in (95, 99):
        assert lib.press_hip_packed_exact(bad) == 0 and lib.press_hip_depress_pa_fused(bad) == 0
        assert lib.press_hip_recode_fused(bad, 98) == 0 and lib.press_hip_recode_fused(98, bad) == 0
    totals = (0, 1, 1000, 32768, 1 << 20, 1 << 27, (1 << 31) + 4096)
    for name, q in TX._questions(lib).items():
        for bad in (95, 99):
            assert q(bad) == 0, (name, bad)
        for mid in (96, 97, 98):
            assert q(mid) > 0, (name, mid)
    for mid in (96, 97, 98):
        for r in (1, 7, 512, 8192):
            last = None
            for t in totals:
                base = int(lib.press_hip_workspace_bytes(mid, t, r))
                row = [base] + [int(getattr(lib, "press_hip_%sworkspace_bytes" % f)(mid, t, r)) for f in ("packed_", "depress_pa_", "depress_norm_", "verify_")]
                row.append(int(lib.press_hip_depress_chunks_workspace_bytes(mid, t, r, T_ROWS, OVERLAP)))
                for other in (5, 15, 18, 3, 98, 97):
                    for keep in (0, 1):
                        ob = int(lib.press_hip_workspace_bytes(other, t, r))
                        for pair in ((mid, other), (other, mid)):
                            for v in (int(lib.press_hip_recode_workspace_bytes(pair[0], pair[1], t, r, keep)),
                                      int(lib.press_hip_recode_packed_workspace_bytes(pair[0], pair[1], t, r, keep)),
                                      int(lib.press_hip_recode_degraded_packed_workspace_bytes(pair[0], pair[1], 3, t, r, keep))):
                                assert v >= base and v >= ob, (mid, other, t, r)
                                row.append(v)
                assert base >= int(lib.press_hip_stall_workspace_bytes(mid - 96, t, r)) > 0 and min(row) >= base, (mid, t, r)
                if last is not None:
                    assert all(x >= y for x, y in zip(row, last)), (mid, t, r)
                last = row


def test_degrading_moves_a_stall():
    """the condition of the degraded tests: under D_b the stall header of at least one fixture read is not the original's"""
    b, moved = degrade_bits()
    assert b is not None and 1 <= b <= 8 and moved, "no b in 1 .. 8 moves a stall header of the fixture"
    n = moved[0]
    s = TS.reads_by_name()[n]
    assert header_of(press.degrade(s, b)) != S.stall_of(TS.segment_of(n), 140)
    for smaller in range(1, b):
        assert all(header_of(press.degrade(x, smaller)) == S.stall_of(TS.segment_of(k), 140) for k, x in TS.reads_by_name().items())


def test_the_batch():
    names, reads = names_of(), reads_of()
    assert [names[0], names[-1], names[-2]] == ["empty-front", "empty-end", "n-1"] and "empty-middle" in names[10:-10]
    assert len(reads) >= 44 and max(len(s) for s in reads) == 155185 and [len(reads[0]), len(reads[-2])] == [0, 1]
    for m in METHODS:
        refused = {n for n, w in zip(names, want(m)) if w is None}
        assert refused == {"empty-front", "empty-middle", "empty-end"} | (set() if m == "dstall_fz" else {OVER}), m
        assert len(decodable(m)) >= len(reads) // 2


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
    yield lb
    torch.cuda.synchronize()
    press.use_torch_stream()
    for k in [k for k in _memo if k[0] == "dev"]:
        del _memo[k]
    torch.cuda.empty_cache()


_t = TS._t


class PressRun(TS.PressRun):
    """test_stall_methods.PressRun through press_hip_press_batch: canary words around out_len, an empty guard read's slot
    on either side of every slot, every byte outside the streams checked"""

    def enqueue(self, method, want_stall=False):
        press.press_batch(method, self.sig, self.off, self.n, self.out, self.d_out_off, self.out_len[GUARD:GUARD + self.nall])

    def run(self, method):
        self.enqueue(method)
        return self.results(False)[0]

    def want_all(self, streams):
        """the expected streams of all the run's reads, guards included"""
        out = [None] * self.nall
        for k, st in zip(self.real, streams):
            out[int(k)] = st
        return out


class DepressRun(TS.DepressRun):
    def __init__(self, method, streams, ns, seed=2):
        super().__init__(streams, ns, seed)
        self.method = method

    def enqueue(self):
        press.depress_batch(self.method, self.arena, self.in_off, self.in_len, self.sig, self.d_off, self.n, self.out_n[GUARD:GUARD + self.nr])


def the_run():
    return memo(("dev", "run"), lambda: PressRun(reads_of(), seed=7))


def layout_of(need, align):
    return TX.layout_of(need, align)


def need_of(streams):
    return np.array([F64 if st is None else len(st) for st in streams], dtype=np.uint64)


def packed(run, method, align, cap):
    """press_packed of a PressRun's reads, guards included, into a filled arena of `cap` bytes and a tail"""
    import torch
    out = torch.full((cap + 4096,), FILL8, dtype=torch.uint8, device="cuda")
    oo = torch.full((run.nall + 1,), -7, dtype=torch.int64, device="cuda")
    ol = torch.full((run.nall,), -7, dtype=torch.int64, device="cuda")
    press._call("press_hip_press_packed", press._mid(method), run.sig.data_ptr(), run.off.data_ptr(), run.n.data_ptr(), run.nall, run.sig.numel(),
                out.data_ptr(), cap, align, oo.data_ptr(), ol.data_ptr(), 1)
    torch.cuda.synchronize()
    return out.cpu().numpy(), oo.cpu().numpy().view(np.uint64), ol.cpu().numpy().view(np.uint64)


def check_packed(tag, streams, align, cap, arena, out_off, out_len):
    """the layout rule of section 2, the streams of the reads that fit, FAILED for the others, every other byte the fill"""
    need = need_of(streams)
    exp = layout_of(need, align)
    assert np.array_equal(out_off, exp), tag
    touched = np.zeros(arena.size, dtype=bool)
    fits = []
    for r, w in enumerate(streams):
        o = int(exp[r])
        if w is None or o + len(w) > cap:
            assert int(out_len[r]) == F64, (tag, r)
            fits.append(False)
            continue
        assert int(out_len[r]) == len(w) and arena[o:o + len(w)].tobytes() == w, (tag, r)
        touched[o:o + len(w)] = True
        fits.append(True)
    assert (arena[~touched] == FILL8).all(), (tag, "a byte outside the streams was written")
    assert (arena[min(cap, arena.size):] == FILL8).all(), (tag, "a byte at or beyond out_cap was written")
    return fits


# ------------------------------------------------------------------ 1: press

@gpu
@pytest.mark.parametrize("method", METHODS)
def test_press(lib, method):
    run = the_run()
    streams = run.run(method)  # (canaries, guards' slots and every byte outside the streams: PressRun.results)
    exp = want(method)
    for name, g, w in zip(names_of(), streams, exp):
        assert g == w, (method, name, None if g is None else len(g), None if w is None else len(w))
    refused = {n for n, g in zip(names_of(), streams) if g is None}
    assert refused == {"empty-front", "empty-middle", "empty-end"} | (set() if method == "dstall_fz" else {OVER})
    if method == "dstall_fz":
        assert sum(len(g) for n, g in zip(names_of(), streams) if n.startswith("three_reads/")) == 172874
    # byte for byte the family's own call with stall = NULL
    assert TS.PressRun(reads_of(), seed=7).run(method, want_stall=False)[0] == streams
    assert run.run(IDS[method]) == streams  # (the id itself)


# ------------------------------------------------------------------ 2: sizes and packed

@gpu
@pytest.mark.parametrize("method", METHODS)
def test_sizes_and_packed(lib, method):
    run = the_run()
    streams = run.want_all(want(method))
    need = need_of(streams)
    c0 = press.smethod_inner_presses()
    got = press.press_sizes(method, run.sig, run.off, run.n).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, need), method
    assert press.smethod_inner_presses() == c0 + 1
    for align in (1, 8, 64):
        total = int(layout_of(need, align)[-1])
        c0 = press.smethod_inner_presses()
        fits = check_packed((method, align), streams, align, total, *packed(run, method, align, total))
        assert all(f == (st is not None) for f, st in zip(fits, streams))
        assert press.smethod_inner_presses() == c0 + 1, "the inner coder runs once per packed call"
    # out_cap inside the stream of a read in the middle
    mid = int(run.real[len(run.real) // 2])
    while streams[mid] is None or len(streams[mid]) < 100:
        mid += 1
    for align in (1, 64):
        exp = layout_of(need, align)
        cap = int(exp[mid]) + len(streams[mid]) // 2
        arena, out_off, out_len = packed(run, method, align, cap)
        fits = check_packed((method, align, "cut"), streams, align, cap, arena, out_off, out_len)
        assert all(fits[r] == (streams[r] is not None) for r in range(mid)) and not any(fits[mid:])
        assert int(out_off[-1]) == int(exp[-1]) > cap


# ------------------------------------------------------------------ 3: depress

@gpu
@pytest.mark.parametrize("method", METHODS)
def test_depress_reads_every_methods_streams(lib, method):
    reads = reads_of()
    for i, made_by in enumerate(METHODS):
        keep = decodable(made_by)
        got = DepressRun(method, [want(made_by)[k] for k in keep], [len(reads[k]) for k in keep], seed=30 + i).run()
        for k, g in zip(keep, got):
            assert g is not None and np.array_equal(g, reads[k]), (method, made_by, names_of()[k])


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_damaged_streams(lib, method):
    """rule 3 of (2s): exists = 2, stall_start + stall_len > n, a piece length past in_len, a stream cut inside its header
    (and the rest of test_stall_methods.damaged): UINT32_MAX, the room keeps its fill, the neighbours decode"""
    gen = {n: s for n, s, _ in S.generated_reads()}
    a, b = gen["len-1501"], gen["stall-two-exceptions"]
    sa, sb = S.expected("rccm_svbbe21_zd", a)[0], S.expected("dstall_fz", b)[0]
    cases = TS.damaged(sa, len(a))
    kinds = [w for w, _ in cases]
    for must in ("exists = 2", "stall beyond the read", "stall piece beyond in_len", "rest piece beyond in_len", "cut inside the header"):
        assert must in kinds
    streams, ns = [sb], [len(b)]
    for _, c in cases:
        streams += [c, sb]
        ns += [len(a), len(b)]
    got = DepressRun(method, streams, ns, seed=41).run()  # (the refused reads' rooms keep FILL16: DepressRun.results)
    for k, (what, _) in enumerate(cases):
        assert got[2 * k + 1] is None, (method, what)
    for k in range(0, len(got), 2):
        assert got[k] is not None and np.array_equal(got[k], b)


# ------------------------------------------------------------------ 4: recode

def slow5_streams(oracle):
    def make():
        out = []
        for s in reads_of():
            ret, st = oracle.press("slow5_svb_zd", s)
            assert ret == 0
            out.append(st)
        return out
    return memo("slow5", make)


class Recode:
    """streams of `src` on the device, scattered, with the rooms of the samples they hold; refused: the positions whose
    stream the source's decoder refuses"""

    def __init__(self, src, streams, samples, seed, refused=()):
        import torch
        self.torch, self.src, self.samples, self.refused = torch, src, samples, set(refused)
        rng = np.random.default_rng(seed)
        self.nr = len(streams)
        self.rooms = np.array([len(s) for s in samples], dtype=np.uint32)
        arena, in_off, in_len = L.scatter_streams(rng, streams)
        self.off, self.total = L.scatter_rooms(rng, self.rooms)
        self.d = (_t(arena), _t(in_off, np.int64), _t(in_len, np.int64), _t(self.rooms, np.int32), _t(self.off, np.int64))

    def _sig(self, keep):
        return self.torch.full((self.total,), FILL16, dtype=self.torch.int16, device="cuda") if keep else None

    def _check_decoded(self, out_n, sig, bits):
        self.torch.cuda.synchronize()
        on = out_n.cpu().numpy().view(np.uint32)
        for k, s in enumerate(self.samples):
            assert int(on[k]) == (F32 if k in self.refused else len(s)), (self.src, k)
        if sig is not None:
            sg = sig.cpu().numpy()
            spans = []
            for k, s in enumerate(self.samples):
                # (a stall decoder leaves a refused read's room as it was; the other decoders promise nothing about it)
                spans.append(0 if k in self.refused and self.src in IDS else len(s))
                if k not in self.refused:
                    o = int(self.off[k])
                    assert np.array_equal(sg[o:o + len(s)], press.degrade(s, bits) if bits else s), (self.src, k)
            assert (sg[L.outside_rooms(self.total, self.off, spans)] == FILL16).all(), (self.src, "a sample outside the decoded reads")

    def batch(self, dst, exp, keep=False, bits=0):
        torch = self.torch
        caps = [TS.slot_for(int(n)) for n in self.rooms]
        out_off = L.slots(np.random.default_rng(3), np.asarray(caps, dtype=np.uint64))
        out = torch.full((int(out_off[-1]) + 64,), FILL8, dtype=torch.uint8, device="cuda")
        ol = torch.full((self.nr,), -7, dtype=torch.int64, device="cuda")
        on = torch.zeros(self.nr, dtype=torch.int32, device="cuda")
        sig = self._sig(keep)
        press.recode_batch(self.src, dst, *self.d, out, _t(out_off, np.int64), ol, on, sig=sig, total_samples=self.total, degrade_bits=bits)
        self._check_decoded(on, sig, bits)
        a, lens = out.cpu().numpy(), ol.cpu().numpy().view(np.uint64)
        touched = np.zeros(a.size, dtype=bool)
        for k, w in enumerate(exp):
            o = int(out_off[k])
            if w is None:
                assert int(lens[k]) == F64, (self.src, dst, k)
                continue
            assert int(lens[k]) == len(w) and a[o:o + len(w)].tobytes() == w, (self.src, dst, k)
            touched[o:(o + len(w)) if dst in IDS else int(out_off[k + 1])] = True  # (a stall id writes its stream and no byte more)
        assert (a[~touched] == FILL8).all(), (self.src, dst, "a byte outside the streams was written")

    def sizes_and_packed(self, dst, exp, keep=False, bits=0, align=1, exact=True):
        """exact: need is the stream's length (else: whatever the destination announces, at least the length)"""
        torch = self.torch
        on = torch.zeros(self.nr, dtype=torch.int32, device="cuda")
        sig = self._sig(keep)
        need = press.recode_sizes(self.src, dst, *self.d, on, sig=sig, total_samples=self.total, degrade_bits=bits)
        self._check_decoded(on, sig, bits)
        need = need.cpu().numpy().view(np.uint64)
        if exact:
            assert np.array_equal(need, need_of(exp)), (self.src, dst)
        else:
            assert all((int(x) == F64) if w is None else (F64 > int(x) >= len(w)) for x, w in zip(need, exp)), (self.src, dst)
        lay = layout_of(need, align)
        total = int(lay[-1])
        out = torch.full((total + 4096,), FILL8, dtype=torch.uint8, device="cuda")
        oo = torch.full((self.nr + 1,), -7, dtype=torch.int64, device="cuda")
        ol = torch.full((self.nr,), -7, dtype=torch.int64, device="cuda")
        on = torch.zeros(self.nr, dtype=torch.int32, device="cuda")
        sig = self._sig(not keep)
        press.recode_packed(self.src, dst, *self.d, out[:total], oo, ol, on, sig=sig, total_samples=self.total, align=align, degrade_bits=bits)
        self._check_decoded(on, sig, bits)
        a = out.cpu().numpy()
        assert np.array_equal(oo.cpu().numpy().view(np.uint64), lay), (self.src, dst)
        lens = ol.cpu().numpy().view(np.uint64)
        touched = np.zeros(a.size, dtype=bool)
        for k, w in enumerate(exp):
            o = int(lay[k])
            if w is None:
                assert int(lens[k]) == F64 and int(lay[k + 1]) == o, (self.src, dst, k)  # refused: FAILED, no byte of the layout
                continue
            assert int(lens[k]) == len(w) and a[o:o + len(w)].tobytes() == w, (self.src, dst, k)
            touched[o:o + (len(w) if exact else int(need[k]))] = True
        assert (a[~touched] == FILL8).all(), (self.src, dst, "a byte outside the slots was written")


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_recode_from_blow5_fields(lib, oracle, method):
    """slow5_svb_zd -> the id: recode_batch, recode_sizes and recode_packed equal tests 1 and 2; one source stream cut
    short: refused, and no byte of the packed form"""
    reads, exp = reads_of(), list(want(method))
    src = list(slow5_streams(oracle))
    cut = names_of().index("gen/len-1500")
    src[cut] = src[cut][:-1]
    exp[cut] = None
    rc = Recode("slow5_svb_zd", src, reads, seed=60 + METHODS.index(method), refused=[cut])
    rc.batch(method, exp, keep=True)
    c0 = press.smethod_inner_presses()
    rc.sizes_and_packed(method, exp, keep=False, align=8 if method == "dstall_fz" else 1)
    assert press.smethod_inner_presses() == c0 + 2  # one for the sizes call, one for the packed call


def own_press(m, reads):
    """a public or extended method's own press of the reads, on the device"""
    return press.press_batch_host(m, reads, [8 * len(s) + 4096 for s in reads])


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_recode_into_other_methods(lib, method):
    keep = decodable(method)
    sub = [reads_of()[k] for k in keep]
    src = [want(method)[k] for k in keep]
    bad = len(src) // 2
    while src[bad][0] != 1:
        bad += 1
    src[bad] = b"\2" + src[bad][1:]  # exists = 2: refused by rule 3
    for i, dst in enumerate(("vbe21_zd", "shuffman_vbe21_zd", "huffman_vbe21_zd")):
        assert press._mid(dst) == (5, 9, 84)[i]
        exp = own_press(dst, sub)
        assert all(e is not None for e in exp)
        exp[bad] = None
        rc = Recode(method, src, sub, seed=70 + i, refused=[bad])
        rc.batch(dst, exp, keep=i % 2 == 0)
        rc.sizes_and_packed(dst, exp, keep=i % 2 == 1, align=1 if i else 64)


@gpu
def test_recode_pairs_that_share_the_scratch(lib):
    """18 -> 98, 98 -> 18, 97 -> 98 and 98 -> 98 in turn: rccm_vbbe21_zd's plan serves reads in one half and pieces in the
    other, and two piece tables of different shapes"""
    reads = reads_of()
    rccm = memo("rccm", lambda: [None if len(s) == 0 else S.zd_stream(s) for s in reads])
    streams = {"rccm_vbbe21_zd": rccm, "dstall_fz_1500": want("dstall_fz_1500"), "dstall_fz": want("dstall_fz")}
    ok = set(decodable("dstall_fz_1500")) & set(decodable("dstall_fz"))
    keep = [k for k in sorted(ok) if not _libs.rc_stored_raw("rccm_vbbe21_zd", rccm[k], len(reads[k]))]
    assert len(keep) >= len(reads) // 2 and max(len(reads[k]) for k in keep) == 155185
    sub = [reads[k] for k in keep]
    for i, (src, dst) in enumerate((("rccm_vbbe21_zd", "dstall_fz"), ("dstall_fz", "rccm_vbbe21_zd"), ("dstall_fz_1500", "dstall_fz"),
                                    ("dstall_fz", "dstall_fz"))):
        assert (press._mid(src), press._mid(dst)) == ((18, 98), (98, 18), (97, 98), (98, 98))[i]
        rc = Recode(src, [streams[src][k] for k in keep], sub, seed=80 + i)
        exp = [streams[dst][k] for k in keep]
        rc.batch(dst, exp, keep=i % 2 == 0)
        rc.sizes_and_packed(dst, exp, keep=i % 2 == 1, align=8, exact=dst != "rccm_vbbe21_zd")


# ------------------------------------------------------------------ 5: degraded

@gpu
@pytest.mark.parametrize("method", METHODS)
def test_degraded_recode_and_verify(lib, oracle, method):
    bits, moved = degrade_bits()
    assert bits and moved
    reads, exp = reads_of(), want(method, bits)
    assert any(a != b for a, b in zip(exp, want(method)))
    rc = Recode("slow5_svb_zd", slow5_streams(oracle), reads, seed=90)
    rc.batch(method, exp, keep=True, bits=bits)
    rc.sizes_and_packed(method, exp, keep=False, bits=bits, align=8)
    keep = decodable(method, bits)
    assert set(names_of()[k] for k in keep) & set(moved)
    sub = [reads[k] for k in keep]
    fb, on, nbad = press.verify_batch_host(method, [exp[k] for k in keep], sub, degrade_bits=bits)
    assert nbad == 0 and (fb == press.VERIFIED).all() and list(on) == [len(s) for s in sub]
    fb, on, nbad = press.verify_batch_host(method, [exp[k] for k in keep], sub)  # (against the originals as they are: not lossless)
    assert nbad > 0


# ------------------------------------------------------------------ 6: the consumers

class Decode:
    def __init__(self, streams, reads, seed=9):
        import torch
        self.torch = torch
        rng = np.random.default_rng(seed)
        self.reads, self.nr = reads, len(reads)
        self.ns = np.array([len(s) for s in reads], dtype=np.uint32)
        arena, in_off, in_len = L.scatter_streams(rng, streams)
        self.off, self.total = L.scatter_rooms(np.random.default_rng(seed + 1), self.ns)  # (the same rooms whatever the streams are)
        self.comp = (_t(arena), _t(in_off, np.int64), _t(in_len, np.int64))
        self.d_off, self.d_n = _t(self.off, np.int64), _t(self.ns, np.int32)
        self.set_samples(reads)

    def set_samples(self, reads):
        sig = np.zeros(self.total, dtype=np.int16)
        for s, o in zip(reads, self.off):
            sig[int(o):int(o) + len(s)] = s
        self.sig = _t(sig)

    def verify(self, m):
        torch = self.torch
        fb, on, nbad = (torch.zeros(k, dtype=torch.int32, device="cuda") for k in (self.nr, self.nr, 1))
        press.verify_batch(m, *self.comp, self.sig, self.d_off, self.d_n, fb, on, nbad)
        torch.cuda.synchronize()
        return fb.cpu().numpy().view(np.uint32), on.cpu().numpy().view(np.uint32), int(nbad.cpu().numpy()[0])

    def results(self, m):
        """every consumer call on the streams as method m -> a dict of numpy arrays, bit patterns"""
        torch = self.torch
        z32 = lambda k=self.nr: torch.zeros(k, dtype=torch.int32, device="cuda")
        out = {}
        out["first_bad"], out["verify_out_n"], nbad = self.verify(m)
        out["nbad"] = np.array([nbad])
        crc, on = z32(), z32()
        press.depress_crc_batch(m, *self.comp, self.d_off, self.d_n, self.total, crc, on)
        out["crc"], out["crc_out_n"] = crc, on
        cal = torch.from_numpy(np.tile(np.array([3.5, 0.1748], dtype=np.float32), self.nr)).cuda()
        pa, on = torch.zeros(self.total, dtype=torch.float32, device="cuda"), z32()
        press.depress_pa_batch(m, *self.comp, pa, self.d_off, self.d_n, cal, on)
        out["pa"], out["pa_out_n"] = pa.view(torch.int32), on
        nm, on, stats = torch.zeros(self.total, dtype=torch.float32, device="cuda"), z32(), z32(2 * self.nr)
        press.depress_norm_batch(m, *self.comp, nm, self.d_off, self.d_n, on, stats=stats)
        out["norm"], out["norm_out_n"], out["stats"] = nm.view(torch.int32), on, stats
        row_first, _, _ = press.chunk_plan(self.ns, T_ROWS, OVERLAP)
        rows = torch.zeros((int(row_first[-1]), T_ROWS), dtype=torch.float16, device="cuda")
        on, q = z32(), z32(2 * self.nr)
        press.depress_chunks_batch(m, *self.comp, rows, _t(row_first, np.int64), self.d_off, self.d_n, self.total, on, OVERLAP, q=q)
        out["rows"], out["rows_q"], out["rows_out_n"] = rows.view(torch.int16), q, on
        torch.cuda.synchronize()
        return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in out.items()}


@gpu
def test_consumers_match_the_public_methods(lib, oracle):
    name = "dstall_fz"
    keep = decodable(name)
    reads = [reads_of()[k] for k in keep]
    base = []
    for s in reads:
        ret, st = oracle.press("vbe21_zd", s, cap=8 * len(s) + 4096)
        assert ret == 0
        base.append(st)
    ref = Decode(base, reads).results("vbe21_zd")
    dec = Decode([want(name)[k] for k in keep], reads)
    got = dec.results(name)
    assert sorted(ref) == sorted(got)
    for k in ref:
        assert ref[k].dtype == got[k].dtype and np.array_equal(ref[k], got[k]), k
    assert int(got["nbad"][0]) == 0 and (got["first_bad"] == press.VERIFIED).all()
    assert [int(c) for c in got["crc"].view(np.uint32)] == [zlib.crc32(s.tobytes()) for s in reads]
    assert got["rows"].shape[0] > len(reads) and got["rows"].any()
    # one sample flipped in two reads: one inside a stall, one in the rest behind it
    long = sorted(range(len(reads)), key=lambda j: -len(reads[j]))
    a = long[0]
    b = next(j for j in long[1:] if want(name)[keep[j]][0] == 1)
    d = S.parse(want(name)[keep[b]])
    at = {a: len(reads[a]) - 3, b: d["stall_start"] + d["stall_len"] // 2}
    bent = [s.copy() for s in reads]
    for j, i in at.items():
        bent[j][i] = np.int16(int(bent[j][i]) ^ 0x0100)
    dec.set_samples(bent)
    fb, on, nbad = dec.verify(name)
    assert nbad == 2 and {j: int(fb[j]) for j in range(len(reads)) if fb[j] != press.VERIFIED} == at
    assert list(on) == [len(s) for s in reads]


# ------------------------------------------------------------------ 7: host pointers

class HostAlloc:
    """numpy arrays in pageable memory or in press_hip_host_alloc's page-locked memory"""

    def __init__(self, lib, pinned):
        self.lib, self.pinned, self.pins = lib, pinned, []

    def zeros(self, count, dtype):
        count = int(count)
        if not self.pinned:
            return np.zeros(count, dtype=dtype)
        nbytes = max(count * np.dtype(dtype).itemsize, 1)
        q = self.lib.press_hip_host_alloc(nbytes)
        assert q, press.last_error()
        self.pins.append(q)
        v = np.frombuffer((ctypes.c_uint8 * nbytes).from_address(q), dtype=dtype, count=count)
        v[:] = 0
        return v

    def copy(self, a):
        v = self.zeros(a.size, a.dtype)
        v[:] = a
        return v

    def close(self):
        for q in self.pins:
            self.lib.press_hip_host_free(q)
        self.pins = []


def host_samples(al, reads):
    sig, off, ns, total = press._host_batch(reads)
    return al.copy(sig), al.copy(off), al.copy(ns), total


def host_streams(al, streams, ns):
    comp, in_off, in_len, ns, off, total = press._decode_batch(streams, ns)
    return al.copy(comp), al.copy(in_off), al.copy(in_len), al.copy(ns), al.copy(off), total


def packed_host(al, method, reads, align):
    sig, off, ns, total = host_samples(al, reads)
    nr = len(reads)
    need = al.zeros(nr, np.uint64)
    press._call("press_hip_press_sizes", press._mid(method), sig.ctypes.data, off.ctypes.data, ns.ctypes.data, nr, total, need.ctypes.data, 0)
    cap = int(layout_of(need, align)[-1])
    out, oo, ol = al.zeros(cap + 64, np.uint8), al.zeros(nr + 1, np.uint64), al.zeros(nr, np.uint64)
    out[cap:] = FILL8
    press._call("press_hip_press_packed", press._mid(method), sig.ctypes.data, off.ctypes.data, ns.ctypes.data, nr, total, out.ctypes.data,
                cap, align, oo.ctypes.data, ol.ctypes.data, 0)
    assert (out[cap:] == FILL8).all()
    return press._streams_of(out, oo, ol), need.copy(), oo.copy()


def recode_packed_host(al, src, dst, streams, rooms, align):
    comp, in_off, in_len, ns, off, total = host_streams(al, streams, rooms)
    nr = len(streams)
    need, on = al.zeros(nr, np.uint64), al.zeros(nr, np.uint32)
    press._call("press_hip_recode_sizes", press._mid(src), press._mid(dst), comp.ctypes.data, in_off.ctypes.data, in_len.ctypes.data,
                ns.ctypes.data, off.ctypes.data, nr, total, need.ctypes.data, None, on.ctypes.data, 0)
    cap = int(layout_of(need, align)[-1])
    out, oo, ol = al.zeros(cap + 64, np.uint8), al.zeros(nr + 1, np.uint64), al.zeros(nr, np.uint64)
    sig = al.zeros(total + 64, np.int16)
    press._call("press_hip_recode_packed", press._mid(src), press._mid(dst), comp.ctypes.data, in_off.ctypes.data, in_len.ctypes.data,
                ns.ctypes.data, off.ctypes.data, nr, total, out.ctypes.data, cap, align, oo.ctypes.data, ol.ctypes.data, sig.ctypes.data,
                on.ctypes.data, 0)
    return press._streams_of(out, oo, ol), oo.copy(), press._reads_of(sig, off, on)


def depress_host(al, method, streams, rooms):
    comp, in_off, in_len, ns, off, total = host_streams(al, streams, rooms)
    sig, on = al.zeros(total + 64, np.int16), al.zeros(len(streams), np.uint32)
    press._call("press_hip_depress_batch", press._mid(method), comp.ctypes.data, in_off.ctypes.data, in_len.ctypes.data, len(streams),
                sig.ctypes.data, off.ctypes.data, ns.ctypes.data, total, on.ctypes.data, 0)
    return press._reads_of(sig, off, on)


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_host_forms(lib, oracle, method):
    """device_resident = 0 from pageable and from page-locked buffers: the streams, layouts and samples of the
    device-resident tests"""
    reads, exp = reads_of(), want(method)
    need = need_of(exp)
    keep = decodable(method)
    src = slow5_streams(oracle)
    for pinned in (False, True):
        al = HostAlloc(lib, pinned)
        try:
            for align in ((8,) if pinned else (1, 64)):
                streams, got_need, oo = packed_host(al, method, reads, align)
                assert streams == exp and np.array_equal(got_need, need) and np.array_equal(oo, layout_of(need, align)), (method, pinned)
            streams, oo, sam = recode_packed_host(al, "slow5_svb_zd", method, src, [len(s) for s in reads], 8)
            assert streams == exp and np.array_equal(oo, layout_of(need, 8)), (method, pinned)
            assert all(np.array_equal(a, b) for a, b in zip(sam, reads))
            back = depress_host(al, method, [exp[k] for k in keep] + [b"\2" + exp[keep[0]][1:]], [len(reads[k]) for k in keep] + [len(reads[keep[0]])])
            assert back[-1] is None
            for k, g in zip(keep, back):
                assert g is not None and np.array_equal(g, reads[k]), (method, pinned, names_of()[k])
        finally:
            al.close()
    if method == "dstall_fz":  # the module's own wrappers, the names resolved by press._mid
        small = [k for k in keep if len(reads[k]) <= 20000]
        sub = [reads[k] for k in small]
        st, total = press.press_packed_host(method, sub, align=8)
        assert st == [exp[k] for k in small] and total == int(layout_of(need_of(st), 8)[-1])
        st2, total2 = press.recode_packed_host("slow5_svb_zd", method, [src[k] for k in small], [len(s) for s in sub], align=8)
        assert st2 == st and total2 == total
        assert all(np.array_equal(a, b) for a, b in zip(press.depress_batch_host(method, st, [len(s) for s in sub]), sub))
        fb, on, nbad = press.verify_batch_host(method, st, sub)
        assert nbad == 0 and (fb == press.VERIFIED).all()
        crc, on = press.depress_crc_batch_host(method, st, [len(s) for s in sub])
        assert [int(c) for c in crc] == [zlib.crc32(s.tobytes()) for s in sub]


# ------------------------------------------------------------------ 8: scratch and stream

def ragged():
    """test_stall_methods.ragged_reads and their streams under the three methods"""
    def make():
        reads = TS.ragged_reads()
        segs = [S.first_segment(s) for s in reads]
        return reads, {m: [S.expected(m, s, g)[0] for s, g in zip(reads, segs)] for m in METHODS}
    return memo("ragged", make)


@gpu
def test_nothing_depends_on_what_scratch_held(lib):
    import torch
    reads, exp = ragged()
    run = PressRun(reads, seed=51)
    keep = TS.kept(exp["dstall_fz_1500"], reads)
    keep = [k for k in keep if TS.decodable(exp["dstall_fz"][k], len(reads[k]))]
    sub = [reads[k] for k in keep]
    for byte in (0x00, 0xFF, 0xA5):
        for method in ("dstall_fz", "rccm_svbbe21_zd"):
            streams = run.want_all(exp[method])
            total = int(layout_of(need_of(streams), 8)[-1])
            torch.cuda.synchronize()
            press.scratch_fill(byte)
            check_packed((method, byte), streams, 8, total, *packed(run, method, 8, total))
        torch.cuda.synchronize()
        press.scratch_fill(byte)
        rc = Recode("dstall_fz_1500", [exp["dstall_fz_1500"][k] for k in keep], sub, seed=52)
        rc.batch("dstall_fz", [exp["dstall_fz"][k] for k in keep])
        torch.cuda.synchronize()
        press.scratch_fill(byte)
        rc.sizes_and_packed("dstall_fz", [exp["dstall_fz"][k] for k in keep], align=8)


@gpu
def test_stream_contract(lib):
    """device resident, on a side stream behind a delay: press_packed and verify_batch of every id return while the delay
    is pending - they only enqueue - and their results are right after synchronising (test_stall_methods.test_stream_contract)"""
    import torch
    reads, exp = ragged()
    run = PressRun(reads, seed=71)
    torch.cuda._sleep(100000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(20000000)
    b.record()
    b.synchronize()
    hold_ms = 50.0
    cycles = int(hold_ms * 20000000 / a.elapsed_time(b))
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0 and lib.press_hip_set_stream(ctypes.c_void_p(s.cuda_stream)) == 0
    try:
        for method in METHODS:
            streams = run.want_all(exp[method])
            need = need_of(streams)
            total = int(layout_of(need, 8)[-1])
            keep = TS.kept(exp[method], reads)
            dec = Decode([exp[method][k] for k in keep], [reads[k] for k in keep], seed=72)
            out = torch.full((total + 4096,), FILL8, dtype=torch.uint8, device="cuda")
            oo = torch.full((run.nall + 1,), -7, dtype=torch.int64, device="cuda")
            ol = torch.full((run.nall,), -7, dtype=torch.int64, device="cuda")
            fb, on, nbad = (torch.full((k,), 7, dtype=torch.int32, device="cuda") for k in (dec.nr, dec.nr, 1))

            def enqueue():
                press.press_packed(method, run.sig, run.off, run.n, out[:total], oo, ol, align=8)
                press.verify_batch(method, *dec.comp, dec.sig, dec.d_off, dec.d_n, fb, on, nbad)
            with torch.cuda.stream(s):
                enqueue()  # (scratch reserved: nothing left to allocate)
            s.synchronize()
            out.fill_(FILL8)
            torch.cuda.synchronize()
            e = torch.cuda.Event()
            t0 = time.perf_counter()
            with torch.cuda.stream(s):
                torch.cuda._sleep(cycles)
                e.record(s)
                enqueue()
            t1 = time.perf_counter()
            assert not e.query(), "a call that promises only to enqueue waited for the stream (or the delay ended early)"
            assert (t1 - t0) * 1e3 < hold_ms / 2
            s.synchronize()
            assert e.query()
            print("%s: press_packed + verify_batch: %.3f ms of host time behind a delay of %g ms" % (method, (t1 - t0) * 1e3, hold_ms))
            check_packed((method, "stream"), streams, 8, total, out.cpu().numpy(), oo.cpu().numpy().view(np.uint64), ol.cpu().numpy().view(np.uint64))
            assert int(nbad.cpu().numpy()[0]) == 0 and (fb.cpu().numpy().view(np.uint32) == press.VERIFIED).all()
            assert list(on.cpu().numpy().view(np.uint32)) == [len(reads[k]) for k in keep]
    finally:
        torch.cuda.synchronize()
        press.use_torch_stream()
