"""press_hip_recode_sizes / press_hip_recode_packed (include/press_hip.h): a recode whose output arena the library lays
out, and the call that only says what the archive would weigh.

As in test_recode.py and test_press_packed.py, what the device must give is fixed on the CPU by the oracle alone, before
the GPU sees anything: the oracle's decode of each source stream (test_recode.entry), the oracle's `dst` stream of those
samples or its refusal, and the layout computed from those sizes (test_press_packed.layout_of).  The frames of the zstd
kinds are not pinned byte for byte: their sizes are the device's, their content is checked as
_layouts.check_zstd_frame does.

The input filter is test_recode.batch_of's: a read the oracle does not give back under `src`, or whose samples the
oracle's `dst` refuses to press, is no input of that pair (at most 2 of the 17 reads, asserted before the GPU part).
"""
import ctypes
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import _layouts as L
import _libs
import test_press_packed as P
import test_recode as R
from honours_amd import press

gpu = pytest.mark.gpu
METHODS = R.METHODS
RC = _libs.RC_FAMILY
F64, F32 = L.FAILED64, L.FAILED32
EARG = -2
CANARY = 256
EMPTY = R.EMPTY
# one fused, one fused into ex-zd, one fused into a range coder, x -> svb, x -> zstd, zstd -> x, svb -> svb
PAIRS = R.LAYOUT_PAIRS + [("svb12", "slow5_svb_zd")]


# ------------------------------------------------------------------ without a GPU

@pytest.fixture(scope="module")
def cpu_lib():
    from honours_amd import build
    build.build()
    return press.load_library()


def test_symbols_are_exported(cpu_lib):
    for s in ("press_hip_recode_sizes", "press_hip_recode_packed", "press_hip_recode_packed_workspace_bytes"):
        assert hasattr(cpu_lib, s), s
        assert s in press.HEADER_SYMBOLS, s
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "press_hip.h")).read()
    for s in ("press_hip_recode_sizes(", "press_hip_recode_packed(", "press_hip_recode_packed_workspace_bytes("):
        assert s in text, s


def test_bad_arguments_are_earg_before_any_device_call(cpu_lib):
    """bad method ids (either side) and bad alignments: PRESS_HIP_EARG, also where there is no device to initialise"""
    a = np.zeros(64, dtype=np.uint64)
    p = a.ctypes.data
    for dr in (0, 1):
        for s, d in ((-1, 5), (5, -1), (19, 2), (2, 19), (1 << 20, 1 << 20)):
            assert cpu_lib.press_hip_recode_sizes(s, d, p, p, p, p, p, 1, 8, p, None, p, dr) == EARG, (s, d)
            assert "method" in press.last_error()
            assert cpu_lib.press_hip_recode_packed(s, d, p, p, p, p, p, 1, 8, p, 256, 1, p, p, None, p, dr) == EARG, (s, d)
            assert "method" in press.last_error()
        for align in (0, 3, 8192):
            assert cpu_lib.press_hip_recode_packed(press.METHODS["svb_zd"], press.METHODS["svb12_zd"], p, p, p, p, p, 1, 8,
                                                   p, 256, align, p, p, None, p, dr) == EARG, align
            assert "align" in press.last_error()


def test_workspace_is_the_recode_figure_and_two_tables(cpu_lib):
    """all 361 pairs, both keep_samples values: press_hip_recode_workspace_bytes + 2 * (nreads + 1) * 8; 0 for bad ids"""
    shapes = [(0, 0), (0, 5), (1000, 0), (1000, 1), (100_000, 64), (930_000_000, 8192), ((1 << 31) + (1 << 20), 5)]
    for s, sid in press.METHODS.items():
        for d, did in press.METHODS.items():
            for keep in (0, 1):
                for t, r in shapes:
                    got = int(cpu_lib.press_hip_recode_packed_workspace_bytes(sid, did, t, r, keep))
                    base = int(cpu_lib.press_hip_recode_workspace_bytes(sid, did, t, r, keep))
                    assert base > 0 and got == base + 2 * (r + 1) * 8, (s, d, keep, t, r, got, base)
    for s, d in ((-1, 5), (5, 19), (19, 19), (3, -7), (1 << 20, 2)):
        for keep in (0, 1):
            assert cpu_lib.press_hip_recode_packed_workspace_bytes(s, d, 100000, 4, keep) == 0


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
    lb.press_hip_scratch_buffers.restype = ctypes.c_uint32
    lb.press_hip_scratch_buffers.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


_p = R._p
GUARD = 0x5A5A5A5A5A5A5A5A


def want_need(dst, e):
    """what the oracle pins of need[r]: F64 for a refusal of either side, the stream's length, the range coders' formula;
    None for the zstd kinds (the frame's bytes are the device's)"""
    if e.out_n == F32 or e.want is None:
        return F64
    if dst in RC:
        return P.rc_need(dst, e.want, e.out_n)
    if dst in L.ZSTD_KINDS:
        return None
    return len(e.want)


class Dev:
    """a batch of source streams on the device, scattered as test_recode.Run places it"""

    def __init__(self, src, dst, entries, rng):
        import torch
        self.torch, self.src, self.dst, self.entries = torch, src, dst, entries
        self.sid, self.did = press.METHODS[src], press.METHODS[dst]
        self.inb, self.in_off, self.in_len = L.scatter_streams(rng, [e.stream for e in entries])
        self.rooms = np.array([e.room for e in entries], dtype=np.uint32)
        self.off, self.total = L.scatter_rooms(rng, self.rooms)
        self.nr = len(entries)
        t = P._t
        self.d = (t(torch, self.inb), t(torch, self.in_off, np.int64), t(torch, self.in_len, np.int64),
                  t(torch, self.rooms, np.int32), t(torch, self.off, np.int64))
        self.reads = [EMPTY if e.samples is None else e.samples for e in entries]
        self.want = [None if e.out_n == F32 else e.want for e in entries]

    def _sig(self, keep):
        return self.torch.full((self.total,), L.SIG_FILL, dtype=self.torch.int16, device="cuda") if keep else None

    def check_samples(self, out_n, sig):
        for k, e in enumerate(self.entries):
            assert int(out_n[k]) == e.out_n, (self.src, self.dst, k, e.name, int(out_n[k]), e.out_n)
            if sig is not None and e.out_n != F32:
                o = int(self.off[k])
                assert np.array_equal(sig[o:o + e.out_n], e.samples), (self.src, self.dst, k, e.name)
        if sig is not None:
            spans = [L.roundup8(r) for r in self.rooms]
            bad = np.nonzero(sig[:self.total][L.outside_rooms(self.total, self.off, spans)] != np.int16(L.SIG_FILL))[0]
            assert bad.size == 0, (self.src, self.dst, "samples written outside the rooms", bad[:8])

    def sizes(self, lib, keep_sig=False):
        """press_hip_recode_sizes behind a guard: need as the oracle has it, out_n and the samples too"""
        torch = self.torch
        d_need = torch.full((self.nr + 8,), GUARD, dtype=torch.int64, device="cuda")
        d_outn = torch.zeros(self.nr, dtype=torch.int32, device="cuda")
        d_sig = self._sig(keep_sig)
        rc = lib.press_hip_recode_sizes(self.sid, self.did, *[_p(a) for a in self.d], self.nr, self.total, _p(d_need),
                                        _p(d_sig), _p(d_outn), 1)
        assert rc == 0, (self.src, self.dst, press.last_error())
        torch.cuda.synchronize()
        need = d_need.cpu().numpy().view(np.uint64)
        assert (need[self.nr:] == GUARD).all(), (self.src, self.dst)
        need = need[:self.nr].copy()
        for k, e in enumerate(self.entries):
            w = want_need(self.dst, e)
            if w is None:
                assert int(need[k]) != F64 and int(need[k]) >= 9, (self.src, self.dst, k, e.name)
            else:
                assert int(need[k]) == w, (self.src, self.dst, k, e.name, int(need[k]), w)
        self.check_samples(d_outn.cpu().numpy().view(np.uint32), None if d_sig is None else d_sig.cpu().numpy())
        return need

    def packed(self, lib, need, align=1, out_cap=None, keep_sig=True):
        """press_hip_recode_packed into an arena of the layout's size + CANARY, pre-filled -> (arena tensor, arena,
        out_off, out_len, streams), everything checked against the oracle"""
        torch = self.torch
        total = int(P.layout_of(need, align)[-1])
        cap = total if out_cap is None else out_cap
        d_out = torch.full((total + CANARY + 64,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
        d_oo = torch.full((self.nr + 1,), -7, dtype=torch.int64, device="cuda")
        d_len = torch.full((self.nr,), -7, dtype=torch.int64, device="cuda")
        d_outn = torch.zeros(self.nr, dtype=torch.int32, device="cuda")
        d_sig = self._sig(keep_sig)
        rc = lib.press_hip_recode_packed(self.sid, self.did, *[_p(a) for a in self.d], self.nr, self.total, _p(d_out), cap,
                                         align, _p(d_oo), _p(d_len), _p(d_sig), _p(d_outn), 1)
        assert rc == 0, (self.src, self.dst, press.last_error())
        torch.cuda.synchronize()
        arena = d_out.cpu().numpy()
        out_off = d_oo.cpu().numpy().view(np.uint64)
        out_len = d_len.cpu().numpy().view(np.uint64)
        streams = P.check_arena(self.oracle, self.dst, self.reads, self.want, need, align, cap, arena,
                                out_off, out_len)
        self.check_samples(d_outn.cpu().numpy().view(np.uint32), None if d_sig is None else d_sig.cpu().numpy())
        return d_out, arena, out_off, out_len, streams


def dev_of(oracle, src, dst, entries, rng):
    d = Dev(src, dst, entries, rng)
    d.oracle = oracle
    return d


# ------------------------------------------------------------------ 1: the matrix

@gpu
@pytest.mark.parametrize("src", METHODS)
def test_matrix_every_pair(lib, oracle, src):
    """src -> each of the 19 methods on the small battery, device resident: align 16 and the samples on every other
    pair"""
    srcs = R.sources(oracle, "small", src)
    batches = []
    for i, dst in enumerate(METHODS):  # the CPU part: what the oracle says, and how much the filter leaves out
        rng = np.random.default_rng(3000 * press.METHODS[src] + press.METHODS[dst])
        left = []
        batches.append((dst, R.batch_of(oracle, srcs, dst, rng, left), rng))
        assert len(left) <= 2 and len(srcs.left_out) <= (8 if src in RC else 2), (src, dst, left, srcs.left_out)
    for i, (dst, ents, rng) in enumerate(batches):
        k = i + press.METHODS[src]
        dev = dev_of(oracle, src, dst, ents, rng)
        need = dev.sizes(lib, keep_sig=k % 2 == 1)
        dev.packed(lib, need, align=16 if k % 2 == 0 else 1, keep_sig=(k // 2) % 2 == 0)


# ------------------------------------------------------------------ 2: fused pairs on granule edges

def edge_battery():
    rng = np.random.default_rng(20261019)
    out = []
    for n in (0, 1, 7, 8, 9, 511, 512, 513, 8191, 8192, 8193, 32767, 32768, 32769, 65537):
        out.append(("walk-%d" % n, R._walk(rng, n, 0.004) if n else EMPTY))
    out.append(("chunks-3", R._walk(rng, 3 * 32768 + 4321, 0.002)))
    return out


_edges = {}


@gpu
@pytest.mark.parametrize("src", R.FUSED_SRC)
def test_fused_pairs_on_granule_edges(lib, oracle, src):
    """every lane, sub-tile, wave-quarter and chunk edge and a read of several chunks through the fused chain; pass A is
    not launched, neither by the sizes call nor by the packed one"""
    if src not in _edges:
        _edges[src] = R.Src(oracle, src, edge_battery())
    srcs = _edges[src]
    assert not srcs.left_out and len(srcs.items) == 16
    for i, dst in enumerate(R.FUSED_DST):
        assert press.recode_fused(src, dst)
        rng = np.random.default_rng(88000 + 100 * press.METHODS[src] + press.METHODS[dst])
        left = []
        ents = R.batch_of(oracle, srcs, dst, rng, left)
        assert not left, (src, dst, left)
        dev = dev_of(oracle, src, dst, ents, rng)
        a0 = press.pass_a_launches()
        need = dev.sizes(lib, keep_sig=i % 2 == 0)
        assert press.pass_a_launches() == a0, (src, dst)
        dev.packed(lib, need, align=16 if i % 2 else 1, keep_sig=i % 2 == 1)
        assert press.pass_a_launches() == a0, (src, dst)


@gpu
def test_general_pair_runs_pass_a_once_per_call(lib, oracle):
    src, dst = "vbe21_zd", "shuffman_vbe21_zd"
    assert not press.recode_fused(src, dst)
    rng = np.random.default_rng(21)
    dev = dev_of(oracle, src, dst, R.batch_of(oracle, R.sources(oracle, "small", src), dst, rng), rng)
    a0 = press.pass_a_launches()
    need = dev.sizes(lib)
    assert press.pass_a_launches() == a0 + 1
    dev.packed(lib, need)
    assert press.pass_a_launches() == a0 + 2


# ------------------------------------------------------------------ 3: every read alone

@gpu
@pytest.mark.parametrize("src,dst", PAIRS)
def test_one_read_batches_end_where_the_stream_ends(lib, oracle, src, dst):
    """every read as a one-read batch with out_cap = need in front of a canary: a store past the stream's end has no
    neighbour to hide under"""
    srcs = R.sources(oracle, "small", src)
    rng = np.random.default_rng(31 * press.METHODS[src] + press.METHODS[dst])
    for name, s, st in srcs.items:
        e = R.entry(oracle, src, dst, name, s, st, rng)
        if e.out_n != F32 and e.out_n > 0 and e.want is None:
            continue  # (outside dst's domain: test_recode.batch_of)
        dev = dev_of(oracle, src, dst, [e], rng)
        need = dev.sizes(lib)
        cap = 0 if int(need[0]) == F64 else int(need[0])
        _, arena, out_off, out_len, streams = dev.packed(lib, need, 1, cap, keep_sig=False)
        assert int(out_off[1]) == cap and (arena[cap:] == L.ARENA_FILL).all(), (src, dst, name)
        assert (streams[0] is None) == (int(need[0]) == F64), (src, dst, name)


# ------------------------------------------------------------------ 4: refused source reads

def bad_batch(oracle, dst, rng):
    """slow5 svb-zd streams with malformed ones (test_recode._bad_batch's kinds) first, two in a row, in front of the
    read `tight` and last -> (entries, index of `tight`)"""
    src = "slow5_svb_zd"
    reads = [R._walk(rng, n, 0.01) for n in (700, 32769, 513, 9000, 8, 40000, 1)]
    good = []
    for k, s in enumerate(reads):
        ret, st = oracle.press(src, s)
        assert ret == 0
        good.append((s, st, R.entry(oracle, src, dst, "good-%d" % k, s, st, rng)))

    def bad(name, k, stream):
        n = len(good[k][0])
        assert oracle.depress(src, stream, n)[0] != 0  # the oracle refuses it (by its length / its count)
        return R.Entry(name, stream, n, 0, F32, None, None)
    st = [g[1] for g in good]
    ents = [bad("truncated", 0, st[0][:-1]), good[0][2], good[1][2],
            bad("trailing byte", 2, st[2] + b"\0"), bad("wrong count", 3, struct.pack("<I", 9001) + st[3][4:]),
            good[2][2], good[3][2], bad("count alone", 4, st[4][:3]), good[5][2], good[4][2], good[6][2],
            bad("truncated last", 6, st[6][:-1])]
    return ents, 8


@gpu
@pytest.mark.parametrize("dst", ["slow5_svb_zd", "zstd_svb_zd", "svb12_zd", "vbe21_zd", "shuffman_vbbe21_zd", "rc_vbe21_zd"])
def test_refused_source_reads_stay_alone(lib, oracle, dst):
    """malformed source streams first, last, two in a row and directly in front of a read that does not fit out_cap:
    out_n = UINT32_MAX, need = out_len = FAILED, 0 bytes of the layout and not a byte written - also where dst has a
    stream for an empty read -; the neighbours are the oracle's"""
    rng = np.random.default_rng(190 + press.METHODS[dst])
    ents, tight = bad_batch(oracle, dst, rng)
    assert ents[tight - 1].out_n == F32 and ents[0].out_n == F32 and ents[-1].out_n == F32
    assert ents[3].out_n == F32 and ents[4].out_n == F32
    assert all(e.want is not None for e in ents if e.out_n != F32), dst
    dev = dev_of(oracle, "slow5_svb_zd", dst, ents, rng)
    need = dev.sizes(lib)
    bad = [k for k, e in enumerate(ents) if e.out_n == F32]
    assert all(int(need[k]) == F64 for k in bad)
    for align in (1, 16):
        exp = P.layout_of(need, align)
        assert all(exp[k + 1] == exp[k] for k in bad)  # no byte of the layout
        full = dev.packed(lib, need, align)[4]
        # one byte short of `tight`: it and everything behind it fails, the refused read in front of it writes nothing
        cap = int(exp[tight]) + int(need[tight]) - 1
        _, arena, out_off, out_len, streams = dev.packed(lib, need, align, cap)
        assert all(int(out_len[k]) == F64 for k in bad)
        assert all(st is None for st in streams[tight:]) and all(st is not None for k, st in enumerate(streams[:tight])
                                                                 if k not in bad)
        assert (arena[int(exp[tight - 2]) + int(need[tight - 2]):] == L.ARENA_FILL).all(), (dst, align)
        if dst not in L.ZSTD_KINDS:
            assert streams[:tight] == full[:tight], (dst, align)
        _, arena, _, out_len, streams = dev.packed(lib, need, align, 0)
        assert (arena == L.ARENA_FILL).all() and all(st is None for st in streams if st != b""), (dst, align)


# ------------------------------------------------------------------ 5: short arena

@gpu
@pytest.mark.parametrize("src,dst", PAIRS)
def test_short_arena(lib, oracle, src, dst):
    rng = np.random.default_rng(500 + 31 * press.METHODS[src] + press.METHODS[dst])
    ents = R.batch_of(oracle, R.sources(oracle, "small", src), dst, rng)
    k = [e.name for e in ents].index("ex1-32769")
    dev = dev_of(oracle, src, dst, ents, rng)
    need = dev.sizes(lib)
    assert int(need[k]) != F64 and int(need[k]) > 0
    for align in (1, 16):
        exp = P.layout_of(need, align)
        for cap in (int(exp[k]) + int(need[k]) - 1, 0):
            # (check_arena: out_off is the layout whatever the capacity)
            _, arena, out_off, out_len, streams = dev.packed(lib, need, align, cap, keep_sig=False)
            first = k if cap else 0
            assert all(st is None for st in streams[first:] if st != b""), (src, dst, align, cap)
            assert all((st is None) == (w is None) for st, w in zip(streams[:first], dev.want)), (src, dst, align, cap)
            assert (arena[int(exp[first]):] == L.ARENA_FILL).all(), (src, dst, align, cap)


# ------------------------------------------------------------------ 6: many reads

_many = {}


@gpu
@pytest.mark.parametrize("src,dst", [("slow5_svb_zd", "shuffman_vbsse21_zd"), ("vbe21_zd", "zstd_svb_zd")])
def test_many_reads(lib, oracle, src, dst):
    """2500 reads of 0 .. 40 samples (the scan's workgroup takes three rounds; vbe21_zd has no stream for the empty
    ones: refused source reads all over the batch), and the batch sizes around one wave"""
    if src not in _many:
        _many[src] = R.Src(oracle, src, P.many_reads())
    srcs = _many[src]
    assert not srcs.left_out and len(srcs.items) == 2500
    rng = np.random.default_rng(60 + press.METHODS[src])
    ents = [R.entry(oracle, src, dst, name, s, st, rng) for name, s, st in srcs.items]
    ents = [e for e in ents if not (e.out_n != F32 and e.out_n > 0 and e.want is None)]
    assert len(ents) >= 2490
    for count, align in ((len(ents), 8), (1, 1), (63, 4), (64, 1), (65, 4096)):
        dev = dev_of(oracle, src, dst, ents[:count], rng)
        need = dev.sizes(lib)
        dev.packed(lib, need, align, keep_sig=count == 64)


# ------------------------------------------------------------------ 7: the existing calls, same library, same buffers

@gpu
@pytest.mark.parametrize("src,dst", PAIRS)
def test_agrees_with_the_existing_calls(lib, oracle, src, dst):
    """the streams are press_hip_recode_batch's in slots of need bytes (align 1); out_off / out_len (and, but for the range coders'
    gaps, the arena) are press_hip_depress_batch + press_hip_press_packed's; press_hip_depress_batch(dst) reads the arena
    back to the source's samples (the oracle's decode of every stream: the range coders' raw-stored tiny reads are not
    given back by the reference either)"""
    import torch
    rng = np.random.default_rng(700 + 31 * press.METHODS[src] + press.METHODS[dst])
    ents = R.batch_of(oracle, R.sources(oracle, "small", src), dst, rng)
    dev = dev_of(oracle, src, dst, ents, rng)
    nr = dev.nr
    need = dev.sizes(lib)
    for align in (1, 16):
        d_out, arena, out_off, out_len, streams = dev.packed(lib, need, align)
        total = int(out_off[-1])
        if align == 1:
            # recode_batch in slots of exactly need bytes; the svb destinations in the slots their writer asks for (it
            # refuses a slot below the format's worst case), so the packed offsets cannot be reused
            sz = [0 if int(x) == F64 else int(x) for x in need]
            if dst in L.SVB_KINDS:
                sz = [max(x, L.slot_of(oracle.bound, dst, len(r))) for x, r in zip(sz, dev.reads)]
            slot_off = np.zeros(nr + 1, dtype=np.uint64)
            slot_off[1:] = np.cumsum(sz)
            b_out = torch.full((int(slot_off[-1]) + CANARY + 64,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
            b_len = torch.zeros(nr, dtype=torch.int64, device="cuda")
            b_outn = torch.zeros(nr, dtype=torch.int32, device="cuda")
            b_oo = P._t(torch, slot_off, np.int64)
            rc = lib.press_hip_recode_batch(dev.sid, dev.did, *[_p(a) for a in dev.d], nr, dev.total, _p(b_out), _p(b_oo),
                                            _p(b_len), None, _p(b_outn), 1)
            assert rc == 0, press.last_error()
            torch.cuda.synchronize()
            bl = b_len.cpu().numpy().view(np.uint64)
            ba = b_out.cpu().numpy()
            assert np.array_equal(bl, out_len), (src, dst)
            for k, st in enumerate(streams):
                if st is not None:
                    assert ba[int(slot_off[k]):int(slot_off[k]) + len(st)].tobytes() == st, (src, dst, k)
        # the two calls: depress, then press_packed with the sample counts out_n
        t_sig = torch.full((dev.total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
        t_outn = torch.zeros(nr, dtype=torch.int32, device="cuda")
        rc = lib.press_hip_depress_batch(dev.sid, _p(dev.d[0]), _p(dev.d[1]), _p(dev.d[2]), nr, _p(t_sig), _p(dev.d[4]),
                                         _p(dev.d[3]), dev.total, _p(t_outn), 1)
        assert rc == 0, press.last_error()
        good = [k for k, e in enumerate(ents) if e.out_n != F32]  # (a refused read: what the sequence cannot express)
        torch.cuda.synchronize()
        assert np.array_equal(t_outn.cpu().numpy().view(np.uint32), [e.out_n for e in ents])
        gi = torch.tensor(good, dtype=torch.int64, device="cuda")
        g_off, g_n = dev.d[4][gi].contiguous(), t_outn[gi].contiguous()
        g_need = need[good]
        t_out = torch.full((total + CANARY + 64,), L.ARENA_FILL, dtype=torch.uint8, device="cuda")
        t_oo = torch.zeros(len(good) + 1, dtype=torch.int64, device="cuda")
        t_len = torch.zeros(len(good), dtype=torch.int64, device="cuda")
        rc = lib.press_hip_press_packed(dev.did, _p(t_sig), _p(g_off), _p(g_n), len(good), dev.total, _p(t_out), total,
                                        align, _p(t_oo), _p(t_len), 1)
        assert rc == 0, press.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(t_len.cpu().numpy().view(np.uint64), out_len[good]), (src, dst, align)
        if len(good) == nr:
            assert np.array_equal(t_oo.cpu().numpy().view(np.uint64), out_off), (src, dst, align)
            if dst not in RC:
                assert np.array_equal(t_out.cpu().numpy(), arena), (src, dst, align)
        else:
            assert np.array_equal(t_oo.cpu().numpy().view(np.uint64), P.layout_of(g_need, align)), (src, dst, align)
        # the arena decodes to the source's samples (header-only static-Huffman streams: _layouts.header_only_huffman)
        in_len = np.array([0 if st is None else len(st) for st in streams], dtype=np.uint64)
        d_back = torch.full((dev.total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
        d_outn = torch.zeros(nr, dtype=torch.int32, device="cuda")
        d_io, d_il = P._t(torch, out_off[:-1], np.int64), P._t(torch, in_len, np.int64)
        d_rooms = P._t(torch, np.array([len(s) for s in dev.reads], dtype=np.uint32), np.int32)
        rc = lib.press_hip_depress_batch(dev.did, _p(d_out), _p(d_io), _p(d_il), nr, _p(d_back), _p(dev.d[4]), _p(d_rooms),
                                         dev.total, _p(d_outn), 1)
        assert rc == 0, press.last_error()
        torch.cuda.synchronize()
        back, outn = d_back.cpu().numpy(), d_outn.cpu().numpy().view(np.uint32)
        compared = 0
        for k, (s, st) in enumerate(zip(dev.reads, streams)):
            if st is None:
                continue
            verdict, wantb = L.expect_depress(oracle, dst, s, st, len(s))
            if verdict == "skip":
                assert L.header_only_huffman(dst, s)
                continue
            # what the oracle's own decoder makes of the stream: the source's samples, except for the tiny reads a
            # range coder stores raw, which the reference itself does not give back (_layouts.battery_verdicts)
            assert verdict == "ok" and int(outn[k]) == len(wantb) == len(s), (src, dst, align, k)
            assert np.array_equal(back[int(dev.off[k]):int(dev.off[k]) + len(s)], wantb), (src, dst, align, k)
            if not np.array_equal(wantb, s):
                assert dst in RC and _libs.rc_stored_raw(dst, st, len(s)), (src, dst, align, k)
                continue
            compared += 1
        # 17 reads: 1 empty, at most 2 left out by the filter, 2 header-only (static Huffman) or at most 6 stored raw (the
        # range coders: walk-1 .. walk-63)
        assert compared >= 17 - 1 - 2 - 6, (src, dst, compared)


# ------------------------------------------------------------------ 8: host pointers

def host_packed(lib, dev, need, align, pin, keep_sig, sizes_first=False):
    """press_hip_recode_packed on host buffers (pin: a function that gives page-locked copies, or None) -> (arena,
    out_off, out_len, out_n, sig)"""
    p = pin if pin else (lambda a: a)
    total = int(P.layout_of(need, align)[-1])
    out = p(np.full(total + CANARY, L.ARENA_FILL, dtype=np.uint8))
    oo = np.zeros(dev.nr + 1, dtype=np.uint64)
    ol = np.zeros(dev.nr, dtype=np.uint64)
    on = np.zeros(dev.nr, dtype=np.uint32)
    sig = p(np.full(dev.total, L.SIG_FILL, dtype=np.int16)) if keep_sig else None
    inb = p(dev.inb)
    if sizes_first:
        nd = np.zeros(dev.nr, dtype=np.uint64)
        rc = lib.press_hip_recode_sizes(dev.sid, dev.did, _p(inb), _p(dev.in_off), _p(dev.in_len), _p(dev.rooms), _p(dev.off),
                                        dev.nr, dev.total, _p(nd), _p(sig), _p(on), 0)
        assert rc == 0, press.last_error()
        assert np.array_equal(nd, need) and np.array_equal(on, [e.out_n for e in dev.entries])
    rc = lib.press_hip_recode_packed(dev.sid, dev.did, _p(inb), _p(dev.in_off), _p(dev.in_len), _p(dev.rooms), _p(dev.off),
                                     dev.nr, dev.total, _p(out), total, align, _p(oo), _p(ol), _p(sig), _p(on), 0)
    assert rc == 0, (dev.src, dev.dst, press.last_error())
    return out, oo, ol, on, sig


@gpu
@pytest.mark.parametrize("src,dst", PAIRS)
def test_host_form(lib, oracle, src, dst):
    """pageable and page-locked buffers, with and without the samples: what the device form gives, with padding and
    gaps as zeros and nothing behind out_cap"""
    rng = np.random.default_rng(800 + 31 * press.METHODS[src] + press.METHODS[dst])
    ents = R.batch_of(oracle, R.sources(oracle, "small", src), dst, rng)
    dev = Dev(src, dst, ents, rng)
    dev.oracle = oracle
    # (page-locked samples: the copy back covers gaps under 128 bytes between rooms, press_hip.h - keep them apart)
    dev.off, dev.total = L.scatter_rooms(rng, dev.rooms, min_gap=64)
    dev.d = dev.d[:4] + (P._t(dev.torch, dev.off, np.int64),)
    need = dev.sizes(lib)
    held = []

    def pinned(a):
        q = lib.press_hip_host_alloc(max(a.nbytes, 1))
        assert q
        held.append(q)
        v = np.frombuffer((ctypes.c_uint8 * a.nbytes).from_address(q), dtype=a.dtype)
        v[:] = a
        return v
    try:
        for j, (pin, keep, align) in enumerate(((None, True, 16), (None, False, 1), (pinned, True, 1), (pinned, False, 16))):
            _, d_arena, d_oo, d_len, d_streams = dev.packed(lib, need, align, keep_sig=False)
            out, oo, ol, on, sig = host_packed(lib, dev, need, align, pin, keep, sizes_first=j == 0)
            total = int(oo[-1])
            assert np.array_equal(oo, d_oo) and np.array_equal(ol, d_len), (src, dst, j)
            assert np.array_equal(on, [e.out_n for e in ents]), (src, dst, j)
            assert (out[total:] == L.ARENA_FILL).all(), (src, dst, j, "bytes written behind out_cap")
            covered = np.zeros(total, dtype=bool)
            for k, st in enumerate(d_streams):
                if st is None:
                    continue
                o = int(oo[k])
                got = out[o:o + len(st)].tobytes()
                if dst in L.ZSTD_KINDS:
                    L.check_zstd_frame(oracle, dst, dev.reads[k], got, dev.want[k])
                else:
                    assert got == st, (src, dst, j, k)
                covered[o:o + (int(need[k]) if dst in RC else len(st))] = True
            assert (out[:total][~covered] == 0).all(), (src, dst, j, "padding does not arrive as zeros")
            if dst in RC:  # the gaps too
                for k, st in enumerate(d_streams):
                    if st is not None:
                        o = int(oo[k])
                        assert (out[o + len(st):o + int(need[k])] == 0).all(), (src, dst, j, k)
            if keep:
                for k, e in enumerate(ents):
                    if e.out_n != F32:
                        assert np.array_equal(sig[int(dev.off[k]):int(dev.off[k]) + e.out_n], e.samples), (src, dst, j, k)
                spans = [0 if e.out_n == F32 else e.out_n for e in ents]
                assert (sig[:dev.total][L.outside_rooms(dev.total, dev.off, spans)] == np.int16(L.SIG_FILL)).all()
            out = sig = None
    finally:
        for q in held:
            lib.press_hip_host_free(q)
    # press.recode_packed_host: the same streams, an arena as large as the layout
    res, arena_bytes, sigs = press.recode_packed_host(src, dst, [e.stream for e in ents], [e.room for e in ents], 16,
                                                      want_samples=True)
    assert arena_bytes == int(P.layout_of(need, 16)[-1]), (src, dst)
    for k, (e, st, x) in enumerate(zip(ents, res, sigs)):
        if dev.want[k] is None:
            assert st is None and (x is None) == (e.out_n == F32), (src, dst, k)
        elif dst in L.ZSTD_KINDS:
            L.check_zstd_frame(oracle, dst, dev.reads[k], st, dev.want[k])
        else:
            assert st == dev.want[k] and np.array_equal(x, e.samples), (src, dst, k)


@gpu
@pytest.mark.parametrize("src,dst", [("slow5_svb_zd", "shuffman_vbe21_zd"), ("vbe21_zd", "slow5_svb_zd"),
                                     ("shuffman_vbsse21_zd", "zstd_svb_zd")])
def test_host_arena_is_sized_by_the_streams(lib, oracle, src, dst):
    """From a library without scratch: what the host packed call allocates beyond the host sizes call is the layout
    (nreads + 1 offsets), out_len and the arena at out_off[nreads] + 64 bytes - each with DevBuf's growth slack of
    n / 8 + 4096, nothing sized by a bound"""
    import torch
    rng = np.random.default_rng(900 + press.METHODS[dst])
    ents = R.batch_of(oracle, R.sources(oracle, "small", src), dst, rng)
    inb, in_off, in_len = L.scatter_streams(rng, [e.stream for e in ents])
    rooms = np.array([e.room for e in ents], dtype=np.uint32)
    off, total = L.scatter_rooms(rng, rooms)
    nr = len(ents)
    sid, did = press.METHODS[src], press.METHODS[dst]
    torch.cuda.synchronize()
    lib.press_hip_shutdown()
    try:
        press.load_table()
        press.use_torch_stream()
        need = np.zeros(nr, dtype=np.uint64)
        on = np.zeros(nr, dtype=np.uint32)
        assert lib.press_hip_recode_sizes(sid, did, _p(inb), _p(in_off), _p(in_len), _p(rooms), _p(off), nr, total, _p(need),
                                          None, _p(on), 0) == 0, press.last_error()
        before = ctypes.c_uint64()
        lib.press_hip_scratch_buffers(ctypes.byref(before))
        cap = int(P.layout_of(need, 1)[-1])
        out = np.zeros(cap + 64, dtype=np.uint8)
        oo = np.zeros(nr + 1, dtype=np.uint64)
        ol = np.zeros(nr, dtype=np.uint64)
        assert lib.press_hip_recode_packed(sid, did, _p(inb), _p(in_off), _p(in_len), _p(rooms), _p(off), nr, total, _p(out),
                                           cap, 1, _p(oo), _p(ol), None, _p(on), 0) == 0, press.last_error()
        after = ctypes.c_uint64()
        lib.press_hip_scratch_buffers(ctypes.byref(after))
        grown = lambda b: b + b // 8 + 4096
        assert int(oo[-1]) == cap
        assert after.value - before.value == grown((nr + 1) * 8) + grown(nr * 8) + grown(cap + 64), \
            (src, dst, after.value - before.value, cap)
        bound = sum(int(lib.press_hip_bound(did, int(e.out_n))) for e in ents if e.out_n not in (0, F32))
        print(src, dst, "arena", cap, "bytes; sum of press_hip_bound", bound)
    finally:
        press.load_table()
        press.use_torch_stream()


# ------------------------------------------------------------------ 9: golden

@gpu
def test_golden_three_reads(lib):
    """the three signal fields of three-reads.blow5 as stored -> each fused destination through
    press.recode_packed_host: the reference's lengths and hashes (three_reads.json)"""
    meta = {r["read_id"]: r for r in json.load(open(os.path.join(R.GOLD, "three_reads.json")))["reads"]}
    rd = press.Blow5Reader(os.path.join(R.GOLD, "three-reads.blow5"))
    batch = rd.next_batch()
    rd.close()
    assert len(batch) == 3 and rd.signal_method == 1
    for dst in R.FUSED_DST:
        out, arena_bytes = press.recode_packed_host("slow5_svb_zd", dst, [s for _, _, s in batch], [n for _, n, _ in batch])
        total = 0
        for (rid, n, _), st in zip(batch, out):
            g = meta[rid]["methods"][dst]
            assert st is not None and len(st) == g["len"], (dst, rid)
            assert hashlib.sha256(st).hexdigest()[:32] == g["sha256_32"], (dst, rid)
            total += len(st)
        if dst == "shuffman_vbe21_zd":
            assert total == 175227
        if dst not in RC:
            assert arena_bytes == total, dst  # out_off[-1] at align 1: the streams and nothing else
        else:
            assert arena_bytes >= total, dst
