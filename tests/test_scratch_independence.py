"""No call depends on what an earlier call left in the library's scratch.

The scratch buffers belong to the context and are reused by every method and call kind; what a kernel reads of them
before writing it rests on initialisation contracts (granules, control blocks, tickets and count rows "zeroed per
launch", by a memset, by the call's first kernel or by the previous use clearing up behind itself).  A fresh process on
freshly allocated, mostly zeroed memory cannot see such a contract broken.  press.scratch_fill(byte) overwrites every
scratch buffer but the static-Huffman table, and the page-locked staging buffers; here every call kind runs once (the
warm-up: all buffers at their size, the result checked in full against the oracle, zlib and the numpy restatements of
the modules imported below) and then once behind each fill, and every output buffer - canaries and guard words
included - must be bit for bit the warm-up's.  The comparisons run on the device (torch.equal on integer views); a
buffer is copied back only to name the read of a mismatch.

The fills: 0x00 all unpublished / zero; 0xFF granule status 3, counters and tickets at their maximum; 0x80 every
look-back granule an inclusive prefix (G_P = 2 << 62); 0x40 every granule an aggregate (G_A = 1 << 62); 0xA5 the
arena fill of _layouts, so that stale scratch looks like stale output.

The batch is the 29-read battery of _layouts.py; for the two order-1 range coders (one read per workgroup) every read
is cut to 20 000 samples.  test_rc_second_read sends 700 reads through the three range coders: they launch at most 256
persistent workgroups, so every workgroup takes a second and a third read from the ticket, one of them long.
"""
import ctypes

import numpy as np
import pytest
import torch  # before the library is loaded, as in a run of the whole suite

import _layouts as L
import _libs
import test_depress_chunks as C
import test_depress_norm as N
import test_depress_pa as PA
import test_gpu_parity as G
import test_host_forms as HF
import test_press_packed as P
import test_recode as R
import test_recode_packed as RP
import test_signal_crc as SC
import test_signal_quantiles as Q
import test_signal_stats as S
import test_table_training as T
import test_verify as V
from honours_amd import press

pytestmark = pytest.mark.gpu

METHODS = sorted(press.METHODS, key=lambda m: press.METHODS[m])
FILLS = (0x00, 0xFF, 0x80, 0x40, 0xA5)
SLOW = ("rcc_vbe21_zd", "rccm_vbbe21_zd")  # one read per workgroup at about 1 us per byte
CUT = 20000
NINE = 9  # the battery's first reads: the empty one and the eight short walks
F64, F32 = L.FAILED64, L.FAILED32
CANARY = 256
T_ROWS, OVERLAP = 64, 5
GUARD64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.load_table()
    press.use_torch_stream()
    lb.press_hip_host_alloc.restype = ctypes.c_void_p
    lb.press_hip_host_alloc.argtypes = [ctypes.c_uint64]
    lb.press_hip_host_free.argtypes = [ctypes.c_void_p]
    lb.press_hip_scratch_buffers.restype = ctypes.c_uint32
    lb.press_hip_scratch_buffers.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    lb.press_hip_symbol_counts.restype = ctypes.c_int
    lb.press_hip_symbol_counts.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    _states.clear()
    _srcs.clear()


def _t(a, dtype=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a if dtype is None else a.view(dtype)).copy()).cuda()


def _full(n, value, dtype):
    return torch.full((int(n),), value, dtype=dtype, device="cuda")


def _p(x):
    return None if x is None else x.data_ptr()


def ok(rc, *tag):
    assert rc == 0, tag + (press.last_error(),)


# ------------------------------------------------------------------ the engine: warm-up, then a run behind every fill

def scratch_figures(lib):
    nbytes = ctypes.c_uint64(0)
    return lib.press_hip_scratch_buffers(ctypes.byref(nbytes)), nbytes.value


def by_offset(off, names):
    """index of an output element -> the read whose range starts last at or below it"""
    off = np.asarray(off, dtype=np.int64)
    order = np.argsort(off, kind="stable")

    def where(i):
        k = int(np.searchsorted(off[order], i, side="right")) - 1
        return names[int(order[k])] if k >= 0 else "in front of the first read"
    return where


def same_as_warm(tag, warm, got, where):
    bad = [k for k in warm if not torch.equal(warm[k], got[k])]
    if not bad:
        return
    k = bad[0]  # only now a copy back: which element, whose
    a, b = warm[k].cpu().numpy().reshape(-1), got[k].cpu().numpy().reshape(-1)
    i = int(np.nonzero(a != b)[0][0])
    whose = where[k](i) if where and k in where else "entry %d" % i
    n = int((a != b).sum())
    pytest.fail("%s: the result depends on the scratch contents: %s differ; %s: %d elements, the first at %d (%s): %#x, warm-up %#x"
                % (" ".join(map(str, tag)), bad, k, n, i, whose, int(b[i]) & 0xFFFFFFFFFFFFFFFF, int(a[i]) & 0xFFFFFFFFFFFFFFFF))


def filled(lib, tag, run, check=None, where=None, fills=FILLS):
    """run() -> {name: device tensor of an integer type}: every buffer the call writes, canaries included"""
    warm = run()
    torch.cuda.synchronize()
    if check is not None:
        check({k: v.cpu().numpy() for k, v in warm.items()})
    figures = scratch_figures(lib)
    for byte in fills:
        press.scratch_fill(byte)
        assert scratch_figures(lib) == figures, tag + ("the fill changed the registry",)
        same_as_warm(tag + ("fill 0x%02X" % byte,), warm, run(), where)
    assert scratch_figures(lib) == figures, tag + ("a buffer grew behind the warm-up",)
    return warm


# ------------------------------------------------------------------ one method's batch, on the device, and what is expected of it

def named_reads(cut, which="full"):
    """the battery; cut: every read to at most CUT samples; "nine": its first reads alone"""
    reads = L.battery()
    if which == "nine":
        return reads[:NINE]
    return [(nm, s[:CUT]) for nm, s in reads] if cut else reads


class State:
    def __init__(self, oracle, m, which):
        self.m, self.mid, self.oracle = m, press.METHODS[m], oracle
        named = named_reads(m in SLOW, which)
        self.names, self.reads = [nm for nm, _ in named], [s for _, s in named]
        self.nr = len(named)
        rng = np.random.default_rng(8800 + 31 * self.mid + self.nr)
        # the press side: what the oracle makes of every read (test_press_packed.Expect), scattered samples, slots
        self.want = P.Expect(oracle, named).want(m)
        self.pd = P.Dev(self.reads, 20261017 + self.mid)
        self.out_off = L.slots(rng, [L.slot_of(press.bound, m, len(s)) for s in self.reads])
        self.d_out_off = _t(self.out_off, np.int64)
        self.need = None
        # the decode side: the streams in scattered rooms and what the oracle decodes of them (test_depress_norm.Case,
        # with test_depress_pa's calibration)
        self.nc = N.Case(oracle, m, self.reads, 7)
        self.nc.cal = PA.batch_cal(self.nr)
        self.din = self.nc.dev()
        self.d_cal = _t(self.nc.cal.reshape(-1))
        self.room_where = by_offset(self.nc.off, self.names)
        # verify: n is the expected count and the room, the caller's samples scattered among noise (test_verify)
        self.vsig, self.voff = L.scatter_reads(rng, self.reads)
        self.vn = np.array([len(s) for s in self.reads], dtype=np.uint32)
        self.vc = {"reads": self.reads, "n": self.vn, "rooms": self.nc.rooms, "dec_room": self.nc.expect,
                   "dec_n": [L.expect_depress(oracle, m, s, x, len(s)) for s, x in zip(self.reads, self.nc.streams)]}
        self.d_v = (_t(self.vsig), _t(self.voff, np.int64), _t(self.vn, np.int32))

    def sizes(self):
        if self.need is None:
            self.need = self.pd.sizes(self.m)
            P.check_need(self.m, self.reads, self.want, self.need)
        return self.need


_states = {}


def state(oracle, m, which="full"):
    if (m, which) not in _states:
        _states[(m, which)] = State(oracle, m, which)
    return _states[(m, which)]


# ---- the call kinds: kind -> (run(lib, s) -> tensors, check(s, numpy arrays), where(s) -> {key: index -> read})

def run_press_batch(lib, s):
    out = _full(int(s.out_off[-1]) + CANARY, L.ARENA_FILL, torch.uint8)
    ln = _full(s.nr, 7, torch.int64)
    press.press_batch(s.m, s.pd.d_sig, s.pd.d_off, s.pd.d_n, out, s.d_out_off, ln)
    return {"out": out, "out_len": ln}


def check_slots(oracle, m, reads, want, out_off, arena, lens, tag=()):
    """every stream in its slot as the oracle has it, FAILED exactly where the oracle refuses; nothing outside the slots
    and nothing in the slot of a read without a stream"""
    inside = np.zeros(arena.size, dtype=bool)
    for k, (s, w) in enumerate(zip(reads, want)):
        o0, o1, ln = int(out_off[k]), int(out_off[k + 1]), int(lens[k])
        t = tag + (m, k, len(s))
        if w is None:
            assert ln == F64, t + (ln,)
            if len(s):  # (a read that fails on the way may have written into its slot; an empty one has nothing to write)
                inside[o0:o1] = True
            continue
        assert ln != F64 and ln <= o1 - o0, t + (ln,)
        st = arena[o0:o0 + ln].tobytes()
        if m in L.ZSTD_KINDS:
            L.check_zstd_frame(oracle, m, s, st, w)
        else:
            assert st == w, t + (ln, len(w))
        inside[o0:o1] = True
    bad = np.nonzero(arena[~inside] != L.ARENA_FILL)[0]
    assert bad.size == 0, tag + (m, "bytes written outside the slots of the streams", bad[:8])


def check_press_batch(s, r):
    check_slots(s.oracle, s.m, s.reads, s.want, s.out_off, r["out"], r["out_len"].view(np.uint64))


def run_press_sizes(lib, s):
    need = _full(s.nr + 8, GUARD64, torch.int64)
    ok(lib.press_hip_press_sizes(s.mid, _p(s.pd.d_sig), _p(s.pd.d_off), _p(s.pd.d_n), s.nr, s.pd.sig.size, _p(need), 1), s.m)
    return {"need": need}


def check_press_sizes(s, r):
    need = r["need"].view(np.uint64)
    assert (need[s.nr:] == GUARD64).all(), s.m
    P.check_need(s.m, s.reads, s.want, need[:s.nr])


def press_packed(align):
    def run(lib, s):
        total = int(P.layout_of(s.sizes(), align)[-1])
        out = _full(total + CANARY + 64, L.ARENA_FILL, torch.uint8)
        oo, ln = _full(s.nr + 1, -7, torch.int64), _full(s.nr, -7, torch.int64)
        ok(lib.press_hip_press_packed(s.mid, _p(s.pd.d_sig), _p(s.pd.d_off), _p(s.pd.d_n), s.nr, s.pd.sig.size, _p(out), total,
                                      align, _p(oo), _p(ln), 1), s.m)
        return {"out": out, "out_off": oo, "out_len": ln}

    def check(s, r):
        total = int(P.layout_of(s.sizes(), align)[-1])
        P.check_arena(s.oracle, s.m, s.reads, s.want, s.sizes(), align, total, r["out"], r["out_off"].view(np.uint64),
                      r["out_len"].view(np.uint64))
    return run, check, lambda s: {}


def run_depress_batch(lib, s):
    d_in, d_io, d_il, d_off, d_n = s.din
    sig, on = _full(s.nc.total, L.SIG_FILL, torch.int16), _full(s.nr, 7, torch.int32)
    press.depress_batch(s.m, d_in, d_io, d_il, sig, d_off, d_n, on)
    return {"sig": sig, "out_n": on}


def check_samples(m, expect, off, rooms, total, sig, out_n, tag=()):
    """out_n as the oracle's verdicts, every decoded read bit for bit, the fill everywhere outside the rooms"""
    for k, (verdict, want) in enumerate(expect):
        t = tag + (m, k, int(rooms[k]))
        if verdict == "skip":
            continue
        if verdict == "fail":
            assert int(out_n[k]) == F32, t
            continue
        assert int(out_n[k]) == len(want), t + (int(out_n[k]), len(want))
        o = int(off[k])
        assert np.array_equal(sig[o:o + len(want)], want), t
    spans = [L.roundup8(r) for r in rooms]
    bad = np.nonzero(sig[:total][L.outside_rooms(total, off, spans)] != np.int16(L.SIG_FILL))[0]
    assert bad.size == 0, tag + (m, "samples written outside the rooms", bad[:8])


def check_depress_batch(s, r):
    check_samples(s.m, s.nc.expect, s.nc.off, s.nc.rooms, s.nc.total, r["sig"], r["out_n"].view(np.uint32))


def run_depress_pa(lib, s):
    d_in, d_io, d_il, d_off, d_n = s.din
    pa, on = _full(s.nc.total, PA.CANARY, torch.int32), _full(s.nr, 7, torch.int32)
    ok(PA.pa_call(lib, s.m, d_in, d_io, d_il, pa, d_off, d_n, s.nc.total, s.d_cal, on, True), s.m)
    return {"floats": pa, "out_n": on}


def check_depress_pa(s, r):
    PA.Case.check(s.nc, r["floats"].view(np.uint32), r["out_n"].view(np.uint32), True)


def run_depress_norm(lib, s):
    d_in, d_io, d_il, d_off, d_n = s.din
    out, on = _full(s.nc.total, N.CANARY, torch.int32), _full(s.nr, 7, torch.int32)
    ok(N.norm_call(lib, s.m, d_in, d_io, d_il, out, d_off, d_n, s.nc.total, None, on, True), s.m)
    return {"floats": out, "out_n": on}


def check_depress_norm(s, r):
    s.nc.check(r["floats"].view(np.uint32), r["out_n"].view(np.uint32), None, device=True)


def depress_chunks(rule):
    def plan(s):
        first, _, _ = C.plan_ref(s.nc.rooms, T_ROWS, OVERLAP)
        return first, int(first[-1]) + 2

    def run(lib, s):
        d_in, d_io, d_il, d_off, d_n = s.din
        first, cap = plan(s)
        rows = _full((cap + C.GUARD) * T_ROWS, C.CANARY[2], torch.int16)
        on, q = _full(s.nr, 7, torch.int32), _full(2 * s.nr + 16, C.Q_FILL, torch.int32)
        d_first = _t(first, np.int64)
        ok(C.chunks_call(lib, s.m, d_in, d_io, d_il, rows, cap, "float16", T_ROWS, OVERLAP, d_first, d_off, d_n, s.nc.total, rule, q,
                         on, True), s.m)
        torch.cuda.synchronize()  # (d_first lives until the call is through)
        return {"rows": rows, "out_n": on, "q": q}

    def check(s, r):
        _, cap = plan(s)
        assert (r["q"][2 * s.nr:] == C.Q_FILL).all(), (s.m, "q written beyond 2 * nreads")
        C.check((s.m,), s.nc.expect, s.nc.rooms, T_ROWS, OVERLAP, "float16", rule, r["rows"].view(np.uint16).reshape(-1, T_ROWS),
                r["out_n"].view(np.uint32), r["q"][:2 * s.nr].reshape(-1, 2), cap)
    return run, check, lambda s: {}


def _slots_np(s, r, names):
    out = {}
    for k in names:
        a = r[k].view(np.uint32)
        w = 1 if k == "nbad" else s.nr
        assert (a[:8] == np.uint32(V.GUARD)).all() and (a[8 + w:] == np.uint32(V.GUARD)).all(), (s.m, k, "written outside its slot")
        out[k] = a[8:8 + w]
    return out


def run_verify(lib, s):
    d_in, d_io, d_il, _, _ = s.din
    sl = V.Slots(s.nr, ("first_bad", "out_n", "nbad"))
    press.verify_batch(s.m, d_in, d_io, d_il, s.d_v[0], s.d_v[1], s.d_v[2], sl["first_bad"], sl["out_n"], sl["nbad"])
    return dict(sl.t, sig=s.d_v[0])


def check_verify(s, r):
    assert np.array_equal(r["sig"], s.vsig), (s.m, "the caller's samples were written")
    V.check_verify(s.m, s.vc, _slots_np(s, r, ("first_bad", "out_n", "nbad")))


def run_crc(lib, s):
    d_in, d_io, d_il, d_off, d_n = s.din
    sl = V.Slots(s.nr, ("crc", "out_n"))
    press.depress_crc_batch(s.m, d_in, d_io, d_il, d_off, d_n, s.nc.total, sl["crc"], sl["out_n"])
    return dict(sl.t)


def check_crc(s, r):
    V.check_crc(s.m, s.vc, _slots_np(s, r, ("crc", "out_n")))


def _rooms(key):
    return lambda s: {key: s.room_where}


def _per_read(*keys):
    return lambda s: {k: (lambda i, s=s: s.names[i - 8] if 8 <= i < 8 + s.nr else "guard word") for k in keys}


KINDS = {
    "press_batch": (run_press_batch, check_press_batch, lambda s: {"out": by_offset(s.out_off[:-1], s.names)}),
    "press_sizes": (run_press_sizes, check_press_sizes, lambda s: {}),
    "press_packed-1": press_packed(1),
    "press_packed-16": press_packed(16),
    "depress_batch": (run_depress_batch, check_depress_batch, _rooms("sig")),
    "depress_pa_batch": (run_depress_pa, check_depress_pa, _rooms("floats")),
    "depress_norm_batch": (run_depress_norm, check_depress_norm, _rooms("floats")),
    "depress_chunks_batch-norule": depress_chunks(None),
    "depress_chunks_batch-rule": depress_chunks(C.RULE),
    "verify_batch": (run_verify, check_verify, _per_read("first_bad", "out_n")),
    "depress_crc_batch": (run_crc, check_crc, _per_read("crc", "out_n")),
}


def run_kind(lib, oracle, kind, m, which="full", fills=FILLS):
    s = state(oracle, m, which)
    run, check, where = KINDS[kind]
    filled(lib, (kind, m, which), lambda: run(lib, s), lambda r: check(s, r), where(s), fills)


@pytest.mark.parametrize("m", METHODS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_filled(lib, oracle, kind, m):
    run_kind(lib, oracle, kind, m)


@pytest.mark.parametrize("m", METHODS)
def test_small_after_large(lib, oracle, m):
    """the battery, then its first nine reads behind every fill: the tails of the per-read tables, chunk tables and tile
    tables hold the larger batch's entries or the fill"""
    big = state(oracle, m)
    for kind in sorted(KINDS):
        KINDS[kind][0](lib, big)
        run_kind(lib, oracle, kind, m, "nine")


# ------------------------------------------------------------------ recode: one destination per source, and every fused pair

ROTATION = {m: METHODS[(i + 1) % len(METHODS)] for i, m in enumerate(METHODS)}  # every method into the next one
FUSED_PAIRS = [(a, b) for a in METHODS for b in METHODS if a in R.FUSED_SRC and b in R.FUSED_DST]
PAIRS = sorted(set(ROTATION.items()) | set(FUSED_PAIRS), key=lambda p: (press.METHODS[p[0]], press.METHODS[p[1]]))


def family(m):
    return "svb" if m in L.SVB_KINDS else "zstd" if m in L.ZSTD_KINDS else "ex"


def test_rotation_covers_what_it_must():
    assert {press.recode_fused(a, b) for a, b in FUSED_PAIRS} == {True}
    assert sum(press.recode_fused(a, b) for a in METHODS for b in METHODS) == len(FUSED_PAIRS) == 36
    assert set(ROTATION.values()) == set(METHODS) and all(a != b for a, b in ROTATION.items())
    assert {(family(a), family(b)) for a, b in ROTATION.items()} == {(x, y) for x in ("svb", "zstd", "ex") for y in ("svb", "zstd", "ex")}


_srcs = {}


def sources(oracle, src, cut):
    if (src, cut) not in _srcs:
        _srcs[(src, cut)] = R.Src(oracle, src, named_reads(cut))
    return _srcs[(src, cut)]


@pytest.mark.parametrize("src,dst", PAIRS)
def test_recode_filled(lib, oracle, src, dst):
    sid, did = press.METHODS[src], press.METHODS[dst]
    rng = np.random.default_rng(5000 + 19 * sid + did)
    ents = R.batch_of(oracle, sources(oracle, src, src in SLOW or dst in SLOW), dst, rng)
    assert sum(e.out_n not in (0, F32) for e in ents) >= 15, (src, dst)
    dev = RP.dev_of(oracle, src, dst, ents, rng)
    names = [e.name for e in ents]
    nr, args = dev.nr, [_p(a) for a in dev.d]
    out_off = L.slots(rng, [e.cap for e in ents])
    d_oo = _t(out_off, np.int64)
    align = 16 if (sid + did) % 2 == 0 else 1
    tag = (src, dst)

    def run_batch():
        out, ln = _full(int(out_off[-1]) + 4096, L.ARENA_FILL, torch.uint8), _full(nr, 7, torch.int64)
        sig, on = _full(dev.total, L.SIG_FILL, torch.int16), _full(nr, 7, torch.int32)
        ok(lib.press_hip_recode_batch(sid, did, *args, nr, dev.total, _p(out), _p(d_oo), _p(ln), _p(sig), _p(on), 1), *tag)
        return {"out": out, "out_len": ln, "sig": sig, "out_n": on}

    def check_batch(r):
        run = object.__new__(R.Run)  # its check() on this call's buffers
        run.src, run.dst, run.entries, run.dev = src, dst, ents, True
        run.rooms, run.off, run.total, run.out_off = dev.rooms, dev.off, dev.total, out_off
        run.arena, run.lens, run.out_n, run.sig = r["out"], r["out_len"].view(np.uint64), r["out_n"].view(np.uint32), r["sig"]
        run.check(oracle)

    where = {"out": by_offset(out_off[:-1], names), "sig": by_offset(dev.off, names)}
    filled(lib, ("recode_batch",) + tag, run_batch, check_batch, where)

    need = dev.sizes(lib)  # (the helper's own call: need, out_n against the oracle)

    def run_sizes():
        d_need, on = _full(nr + 8, GUARD64, torch.int64), _full(nr, 7, torch.int32)
        ok(lib.press_hip_recode_sizes(sid, did, *args, nr, dev.total, _p(d_need), None, _p(on), 1), *tag)
        return {"need": d_need, "out_n": on}

    def check_sizes(r):
        got = r["need"].view(np.uint64)
        assert (got[nr:] == GUARD64).all() and np.array_equal(got[:nr], need), tag
        dev.check_samples(r["out_n"].view(np.uint32), None)

    filled(lib, ("recode_sizes",) + tag, run_sizes, check_sizes)

    total = int(P.layout_of(need, align)[-1])

    def run_packed():
        out = _full(total + CANARY + 64, L.ARENA_FILL, torch.uint8)
        oo, ln = _full(nr + 1, -7, torch.int64), _full(nr, -7, torch.int64)
        sig, on = _full(dev.total, L.SIG_FILL, torch.int16), _full(nr, 7, torch.int32)
        ok(lib.press_hip_recode_packed(sid, did, *args, nr, dev.total, _p(out), total, align, _p(oo), _p(ln), _p(sig), _p(on), 1), *tag)
        return {"out": out, "out_off": oo, "out_len": ln, "sig": sig, "out_n": on}

    def check_packed(r):
        P.check_arena(oracle, dst, dev.reads, dev.want, need, align, total, r["out"], r["out_off"].view(np.uint64),
                      r["out_len"].view(np.uint64))
        dev.check_samples(r["out_n"].view(np.uint32), r["sig"])

    filled(lib, ("recode_packed", align) + tag, run_packed, check_packed, {"sig": by_offset(dev.off, names)})


# ------------------------------------------------------------------ the calls without a method

@pytest.fixture(scope="module")
def signals():
    named = L.battery()
    reads = [s for _, s in named]
    return [nm for nm, _ in named], reads, P.Dev(reads, 20261019)


def test_signal_stats_filled(lib, signals):
    names, reads, d = signals
    nr = len(reads)

    def run():
        st = _full(2 * nr + 16, 77, torch.int32)
        press.signal_stats(d.d_sig, d.d_off, d.d_n, st)
        return {"stats": st}

    def check(r):
        assert (r["stats"][2 * nr:] == 77).all()
        assert r["stats"][:2 * nr].reshape(-1, 2).tolist() == [list(S.ref_stats(s)) for s in reads]

    filled(lib, ("signal_stats",), run, check, {"stats": lambda i: names[i // 2] if i < 2 * nr else "guard"})


@pytest.mark.parametrize("ranks", sorted(Q.RANK_SETS))
def test_signal_quantiles_filled(lib, signals, ranks):
    names, reads, d = signals
    rk = Q.RANK_SETS[ranks]
    nr, nq = len(reads), len(rk)

    def run():
        q = _full(nq * nr + 16, 77, torch.int32)
        press.signal_quantiles(d.d_sig, d.d_off, d.d_n, rk, q)
        return {"q": q}

    def check(r):
        assert (r["q"][nq * nr:] == 77).all()
        assert r["q"][:nq * nr].reshape(-1, nq).tolist() == [Q.ref_quantiles(s, rk) for s in reads]

    filled(lib, ("signal_quantiles", ranks), run, check, {"q": lambda i: names[i // nq] if i < nq * nr else "guard"})


def test_signal_crc32_filled(lib, signals):
    names, reads, d = signals
    nr = len(reads)

    def run():
        crc = _full(nr + 16, SC.GUARD, torch.int32)
        press.signal_crc32(d.d_sig, d.d_off, d.d_n, crc[8:8 + nr])
        return {"crc": crc}

    def check(r):
        a = r["crc"].view(np.uint32)
        assert (a[:8] == np.uint32(SC.GUARD)).all() and (a[8 + nr:] == np.uint32(SC.GUARD)).all(), "written outside crc[]"
        assert a[8:8 + nr].tolist() == [SC.crc_of(s) for s in reads]

    filled(lib, ("signal_crc32",), run, check, {"crc": lambda i: names[i - 8] if 8 <= i < 8 + nr else "guard"})


def test_symbol_counts_filled(lib, signals):
    _, reads, d = signals
    base = np.arange(press.NBINS, dtype=np.uint64) * 3 + 1  # (the call adds)

    def run():
        counts = _t(base, np.int64)
        press.symbol_counts(d.d_sig, d.d_off, d.d_n, counts)
        return {"counts": counts}

    def check(r):
        assert np.array_equal(r["counts"].view(np.uint64), base + T.zd_counts(reads))

    filled(lib, ("symbol_counts",), run, check)


# ------------------------------------------------------------------ the host-pointer forms: staging DevBufs and page-locked buffers

def call_verify_host(lib, c, b):
    fb, on, nb = b.fill(c.nr, np.uint32, 7), b.fill(c.nr, np.uint32, 7), b.fill(1, np.uint32, 7)
    HF.ok(lib.press_hip_verify_batch(c.mid, *c.decode_args(b), c.nr, *b.ptrs(c.sig, c.off, c.ns), c.total, fb.ptr, on.ptr, nb.ptr, b.dev))
    return {"first_bad": fb.get(), "out_n": on.get(), "nbad": nb.get()}


def _host_press_batch(c, m, d, h, tag):
    HF.same_streams(m, HF.with_slots(c, d), HF.with_slots(c, h), tag, True)


def _host_press_packed(c, m, d, h, tag):
    HF.same_streams(m, d, h, tag, False)


def _host_depress(c, m, d, h, tag):
    HF.same_elems(c, d, h, "sig", np.int16(L.SIG_FILL), tag)


def _host_recode_packed(c, m, d, h, tag):
    HF.same_streams(HF.RECODE_TO[m], d, h, tag, False)
    HF.same_elems(c, d, h, "sig", np.int16(L.SIG_FILL), tag)


def _host_verify(c, m, d, h, tag):
    HF.same_arrays(d, h, ("first_bad", "out_n", "nbad"), tag)
    assert int(d["first_bad"][c.cut]) == 0 and int(d["out_n"][c.cut]) == F32, tag
    assert (d["first_bad"] == V.VERIFIED).sum() >= 3 and int(d["nbad"][0]) == int((d["first_bad"] != V.VERIFIED).sum()), tag


HOST_CALLS = {
    "press_batch_host": (HF.call_press_batch, _host_press_batch),
    "press_packed_host": (HF.call_press_packed, _host_press_packed),
    "depress_batch_host": (HF.call_depress_batch, _host_depress),
    "recode_packed_host": (HF.call_recode_packed, _host_recode_packed),
    "verify_batch_host": (call_verify_host, _host_verify),
}


@pytest.mark.parametrize("kind", HF.HOST_KINDS)
@pytest.mark.parametrize("m", HF.METHODS)
@pytest.mark.parametrize("name", sorted(HOST_CALLS))
def test_host_forms_filled(lib, name, m, kind):
    """the warm-up's yardstick is the device-resident form of the same call, as in test_host_forms; behind every fill the
    host form must deliver the same bytes again"""
    c = HF.case(lib, m, "staged6")
    call, same = HOST_CALLS[name]

    def run(form):
        b = HF.Bufs(lib, form)
        try:
            return {k: np.array(v, copy=True) for k, v in call(lib, c, b).items()}
        finally:
            b.close()

    tag = (name, m, kind)
    warm = run(kind)
    same(c, m, run("dev"), warm, tag)
    figures = scratch_figures(lib)
    for byte in FILLS:
        press.scratch_fill(byte)
        got = run(kind)
        for k in warm:
            assert np.array_equal(warm[k], got[k]), tag + ("fill 0x%02X" % byte, k, "the result depends on the scratch contents")
    assert scratch_figures(lib) == figures, tag


# ------------------------------------------------------------------ the per-read symbols, a table switch

@pytest.mark.parametrize("m", METHODS)
def test_per_read_symbols_after_fill(lib, oracle, m):
    s = dict(L.battery())["ex1-2049"]
    assert len(s) == 2049 and G.shuff_ok(m, s)
    G.check_read(oracle, m, s)  # (its buffers at their size)
    press.scratch_fill(0xFF)
    G.check_read(oracle, m, s)


def test_table_switch_under_fill(lib, oracle, tmp_path):
    """the fill spares the device's table and nothing else: a new table is uploaded over filled scratch and used, and
    the default table comes back the same way"""
    lens = G.TABLES["long_codes"]
    path = str(tmp_path / "long_codes.huffman")
    G._write_table(path, lens, G._canonical_table(lens))
    rng = np.random.default_rng(len("long_codes"))
    steps = rng.integers(-90, 91, size=70000)
    steps[rng.random(70000) < 0.01] += 400
    sig = np.cumsum(steps).astype(np.int16)
    m = "shuffman_vbe21_zd"
    try:
        press.scratch_fill(0xFF)
        oracle.load_table(path)
        press.use_table(path)
        G.check_read(oracle, m, sig)
        press.scratch_fill(0xFF)
        G.check_read(oracle, m, sig)  # the table outlives a fill
    finally:
        press.scratch_fill(0xFF)
        oracle.load_table()
        press.use_table()
    G.check_read(oracle, m, sig)
    press.scratch_fill(0x00)
    G.check_read(oracle, m, sig)


# ------------------------------------------------------------------ range coders: a workgroup's second read

RC_READS = 700


def rc_reads():
    rng = np.random.default_rng(20261020)
    out = []
    for k in range(RC_READS):
        if k % 50 == 7:
            out.append(np.zeros(0, dtype=np.int16))
        else:
            out.append(L._walk(rng, int(rng.integers(100, 701)), 0.05, lo=-3, hi=4))
    out[300] = L._walk(rng, 40000, 0.05, lo=-3, hi=4)  # one long read among short ones
    return out


@pytest.mark.parametrize("m", _libs.RC_FAMILY)
def test_rc_second_read(lib, oracle, m):
    """700 reads on at most 256 persistent workgroups (rc: lanes): the model is rebuilt for every read a workgroup takes,
    an empty read is skipped (`continue` on the status) and a read that does not fit its slot fails alone"""
    reads = rc_reads()
    names = ["read-%d" % k for k in range(RC_READS)]
    empty = [k for k in range(RC_READS) if k % 50 == 7]
    slots = [L.slot_of(press.bound, m, len(s)) for s in reads]
    want = [L.expect_press(oracle, m, s, c) for s, c in zip(reads, slots)]
    assert [k for k, w in enumerate(want) if w is None] == empty and len(empty) == 14
    assert not any(w is not None and _libs.rc_stored_raw(m, w, len(s)) for s, w in zip(reads, want)), "the test's inputs are wrong"
    rng = np.random.default_rng(700 + press.METHODS[m])
    d = P.Dev(reads, 20261020)

    def pressed(out_off):
        d_oo = _t(out_off, np.int64)

        def run():
            out, ln = _full(int(out_off[-1]) + CANARY, L.ARENA_FILL, torch.uint8), _full(RC_READS, 7, torch.int64)
            press.press_batch(m, d.d_sig, d.d_off, d.d_n, out, d_oo, ln)
            torch.cuda.synchronize()  # (d_oo)
            return {"out": out, "out_len": ln}
        return run

    out_off = L.slots(rng, slots)
    filled(lib, ("rc press_batch", m), pressed(out_off),
           lambda r: check_slots(oracle, m, reads, want, out_off, r["out"], r["out_len"].view(np.uint64)),
           {"out": by_offset(out_off[:-1], names)})

    # the streams back: every sample
    streams = [b"" if w is None else w for w in want]
    rooms = np.array([len(s) for s in reads], dtype=np.uint32)
    expect = [L.expect_depress(oracle, m, s, x, len(s)) for s, x in zip(reads, streams)]
    assert all(v == ("fail" if k in empty else "ok") and (w is None or np.array_equal(w, reads[k])) for k, (v, w) in enumerate(expect))
    inb, in_off, in_len = L.scatter_streams(rng, streams)
    off, total = L.scatter_rooms(rng, rooms)
    din = (_t(inb), _t(in_off, np.int64), _t(in_len, np.int64), _t(off, np.int64), _t(rooms, np.int32))

    def run_back():
        sig, on = _full(total, L.SIG_FILL, torch.int16), _full(RC_READS, 7, torch.int32)
        press.depress_batch(m, din[0], din[1], din[2], sig, din[3], din[4], on)
        return {"sig": sig, "out_n": on}

    filled(lib, ("rc depress_batch", m), run_back,
           lambda r: check_samples(m, expect, off, rooms, total, r["sig"], r["out_n"].view(np.uint32)), {"sig": by_offset(off, names)})

    # every third read in a slot 8 bytes short of its stream: it fails, its neighbours are exact
    short = [len(w) - 8 if (k % 3 == 0 and w is not None) else c for k, (w, c) in enumerate(zip(want, slots))]
    want2 = [L.expect_press(oracle, m, s, c) for s, c in zip(reads, short)]
    cutk = [k for k in range(0, RC_READS, 3) if want[k] is not None]
    assert all(want2[k] is None for k in cutk) and len(cutk) >= 220
    assert all(want2[k] == want[k] for k in range(RC_READS) if k not in cutk)
    off2 = L.slots(rng, short)
    r = pressed(off2)()
    check_slots(oracle, m, reads, want2, off2, r["out"].cpu().numpy(), r["out_len"].cpu().numpy().view(np.uint64), ("short slots",))
