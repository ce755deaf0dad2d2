"""The families' methods in the generic calls (include/press_hip.h section 2w): the extended method ids of the sixteen
range-coder pairs, the four rice_*_zd and the four huffman_*_zd, and what press, sizes, packed, depress, recode, degrade,
verify, CRC, picoampere, normalise and chunk-row calls do with them.

What the device must give is fixed before the GPU sees anything:
* the eight staged ids (Rice, per-read Huffman): _rice.expected / _dhuf.expected, the numpy restatements pinned to the
  reference by tests/golden/ref_*.json (Rice's padding bits cleared: _rice.clear_padding);
* the thirteen coder ids: the family's own press_hip_rcf_press_batch, which tests/test_rc_family.py pins;
* floats, rows, first_bad and CRCs: the same call on vbe21_zd streams of the same reads, and zlib.

The reads are _layouts.battery(): 29 reads, the longest 150 000 samples, chunk and unit edges, empty reads at both ends
and in the middle, a read of exceptions alone, a constant read and n = 1.
"""
import ctypes
import re
import os
import zlib

import numpy as np
import pytest

import _dhuf
import _layouts as L
import _prefix_runs as PR
import _rcf
import _rice
from honours_amd import abi, press

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "press_hip.h")
EARG = -2
F64, F32 = L.FAILED64, L.FAILED32
STAGES = ("rc", "rcc", "rccm", "rccdf", "rice", "huffman")
LAYOUTS = _rcf.LAYOUTS
XM = abi.XMETHODS if hasattr(abi, "XMETHODS") else {}
STAGED = ["%s_%s_zd" % (s, l) for s in ("rice", "huffman") for l in LAYOUTS]
CODERS = [_rcf.name(c, l) for c in _rcf.CODERS for l in LAYOUTS if _rcf.name(c, l) not in press.METHODS]
X21 = CODERS + STAGED
BAD_IDS = (-1, 19, 63, 88, 1000, 1 << 20)
RC_SLACK = 32
FILL8 = PR.FILL8


def parts(name):
    stage, layout, _ = name.split("_")
    return stage, layout


# ------------------------------------------------------------------ without a GPU

@pytest.fixture(scope="module")
def cpu_lib():
    from honours_amd import build
    build.build()
    return press.load_library()


def test_xmethod_ids_and_their_inverse(cpu_lib):
    assert len(X21) == 21 and len(XM) == 24
    for si, s in enumerate(STAGES):
        for li, l in enumerate(LAYOUTS):
            name = "%s_%s_zd" % (s, l)
            want = press.METHODS.get(name, 64 + 4 * si + li)
            assert cpu_lib.press_hip_xmethod(si, li) == want == XM[name] == press.xmethod_id(s, l), name
            for mid in {want, 64 + 4 * si + li}:  # (64, 68 and 73 mean the three public pairs)
                st, la = ctypes.c_int(-9), ctypes.c_int(-9)
                assert cpu_lib.press_hip_xmethod_parts(mid, ctypes.byref(st), ctypes.byref(la)) == 0
                assert (st.value, la.value) == (si, li) == press.xmethod_parts(mid), (name, mid)
    assert [XM[n] for n in ("rc_vbe21_zd", "rcc_vbe21_zd", "rccm_vbbe21_zd")] == [16, 17, 18]
    for s, l in ((-1, 0), (6, 0), (0, -1), (0, 4), (1000, 1000)):
        assert cpu_lib.press_hip_xmethod(s, l) == -1
    st, la = ctypes.c_int(0), ctypes.c_int(0)
    for mid in list(range(-2, 16)) + list(range(19, 64)) + [88, 89, 1000, 1 << 20]:
        assert cpu_lib.press_hip_xmethod_parts(mid, ctypes.byref(st), ctypes.byref(la)) == EARG, mid
    assert cpu_lib.press_hip_xmethod_parts(80, None, ctypes.byref(la)) == EARG
    assert press.xmethod_names() == list(XM) and press.XMETHODS is abi.XMETHODS
    assert len(press.METHODS) == 19 and press._mid("huffman_vbe21_zd") == 84 and press._mid("vbe21_zd") == 5


def test_header_mirror_and_wrappers(cpu_lib):
    import inspect
    from honours_amd import xmethod
    header = open(HEADER).read()
    flat = " ".join(header.split())
    for k, s in enumerate(("RC", "RCC", "RCCM", "RCCDF", "RICE", "HUFFMAN")):
        assert "PRESS_HIP_XSTAGE_%s = %d" % (s, k) in flat
        assert abi.XSTAGES[s.lower()] == k
    assert "PRESS_HIP_NXSTAGES = 6" in flat and "PRESS_HIP_XMETHOD_BASE = 64" in flat and "PRESS_HIP_NMETHODS = 19" in flat
    assert abi.XMETHOD_BASE == 64
    for s in ("press_hip_xmethod", "press_hip_xmethod_parts"):
        assert hasattr(cpu_lib, s) and s in abi.PROTOS and s in press.HEADER_SYMBOLS and s + "(" in header, s
    assert "press_hip_debug_stage_sizing_launches" in abi._UNDECLARED and "press_hip_debug_stage_sizing_launches" not in header
    assert "(2w) the families in the generic calls" in header
    public = sorted(n for n, f in vars(xmethod).items() if not n.startswith("_") and inspect.isfunction(f) and f.__module__ == xmethod.__name__)
    assert public == ["xmethod_id", "xmethod_names", "xmethod_parts", "xmethod_sizing_launches"]
    for w in public:
        assert getattr(press, w) is getattr(xmethod, w)
    assert press.xmethod_sizing_launches() >= 0
    enum = re.search(r"enum press_hip_xstage \{(.*?)\}", header, re.S).group(1)
    assert len(re.findall(r"PRESS_HIP_XSTAGE_[A-Z]+\s*=", enum)) == 6


def test_bound_is_the_familys(cpu_lib, oracle):
    assert len(XM) == 24
    for name, mid in XM.items():
        for n in (1, 2, 7, 8, 9, 1000, 7329, 155185, 5724000):
            want = oracle.bound("vbe21_zd", n)  # vb1e2_zd_bound_16 for all of them
            stage, layout = parts(name)
            fam = {"rice": press.rice_bound, "huffman": press.huffman_bound}.get(stage)
            assert (fam(layout, n) if fam else press.rcf_bound(stage, layout, n)) == want
            assert cpu_lib.press_hip_bound(mid, n) == want == press.bound(name, n), (name, n)
    for bad in BAD_IDS:
        assert cpu_lib.press_hip_bound(bad, 1000) == 0


def _calls(lib):
    """every call of the table with one method id left open -> {name: f(mid, device_resident)}; the arguments are valid
    for an empty batch, so that an id the call accepts gets past the argument check (and then needs a device)"""
    a = np.zeros(64, dtype=np.uint64)
    p = a.ctypes.data
    Z = 0  # nreads
    return {
        "press_batch": lambda m, dr: lib.press_hip_press_batch(m, p, p, p, Z, 0, p, p, p, dr),
        "press_sizes": lambda m, dr: lib.press_hip_press_sizes(m, p, p, p, Z, 0, p, dr),
        "press_packed": lambda m, dr: lib.press_hip_press_packed(m, p, p, p, Z, 0, p, 0, 1, p, p, dr),
        "depress_batch": lambda m, dr: lib.press_hip_depress_batch(m, p, p, p, Z, p, p, p, 0, p, dr),
        "depress_pa_batch": lambda m, dr: lib.press_hip_depress_pa_batch(m, p, p, p, Z, p, p, p, 0, p, p, dr),
        "depress_norm_batch": lambda m, dr: lib.press_hip_depress_norm_batch(m, p, p, p, Z, p, p, p, 0, p, p, dr),
        "depress_chunks_batch": lambda m, dr: lib.press_hip_depress_chunks_batch(m, p, p, p, Z, p, 0, 1, 64, 8, p, p, p, 0, None, p, p, dr),
        "depress_crc_batch": lambda m, dr: lib.press_hip_depress_crc_batch(m, p, p, p, Z, p, p, 0, p, p, dr),
        "verify_batch": lambda m, dr: lib.press_hip_verify_batch(m, p, p, p, Z, p, p, p, 0, p, p, p, dr),
        "verify_degraded_batch": lambda m, dr: lib.press_hip_verify_degraded_batch(m, 3, p, p, p, Z, p, p, p, 0, p, p, p, dr),
        "recode_batch src": lambda m, dr: lib.press_hip_recode_batch(m, 5, p, p, p, p, p, Z, 0, p, p, p, None, p, dr),
        "recode_batch dst": lambda m, dr: lib.press_hip_recode_batch(15, m, p, p, p, p, p, Z, 0, p, p, p, None, p, dr),
        "recode_sizes src": lambda m, dr: lib.press_hip_recode_sizes(m, 5, p, p, p, p, p, Z, 0, p, None, p, dr),
        "recode_sizes dst": lambda m, dr: lib.press_hip_recode_sizes(15, m, p, p, p, p, p, Z, 0, p, None, p, dr),
        "recode_packed src": lambda m, dr: lib.press_hip_recode_packed(m, 5, p, p, p, p, p, Z, 0, p, 0, 1, p, p, None, p, dr),
        "recode_packed dst": lambda m, dr: lib.press_hip_recode_packed(15, m, p, p, p, p, p, Z, 0, p, 0, 1, p, p, None, p, dr),
        "recode_degraded_batch dst": lambda m, dr: lib.press_hip_recode_degraded_batch(15, m, 3, p, p, p, p, p, Z, 0, p, p, p, None, p, dr),
        "recode_degraded_sizes dst": lambda m, dr: lib.press_hip_recode_degraded_sizes(15, m, 3, p, p, p, p, p, Z, 0, p, None, p, dr),
        "recode_degraded_packed dst": lambda m, dr: lib.press_hip_recode_degraded_packed(15, m, 3, p, p, p, p, p, Z, 0, p, 0, 1, p, p, None, p, dr),
        "recode_degraded_batch src": lambda m, dr: lib.press_hip_recode_degraded_batch(m, 5, 3, p, p, p, p, p, Z, 0, p, p, p, None, p, dr),
    }


def _questions(lib):
    """the workspace / fused / exact questions with one id left open: 0 for an id that is not a method"""
    T, R = 100000, 16
    return {
        "workspace_bytes": lambda m: lib.press_hip_workspace_bytes(m, T, R),
        "packed_workspace_bytes": lambda m: lib.press_hip_packed_workspace_bytes(m, T, R),
        "depress_pa_workspace_bytes": lambda m: lib.press_hip_depress_pa_workspace_bytes(m, T, R),
        "depress_norm_workspace_bytes": lambda m: lib.press_hip_depress_norm_workspace_bytes(m, T, R),
        "depress_chunks_workspace_bytes": lambda m: lib.press_hip_depress_chunks_workspace_bytes(m, T, R, 64, 8),
        "verify_workspace_bytes": lambda m: lib.press_hip_verify_workspace_bytes(m, T, R),
        "recode_workspace_bytes src": lambda m: lib.press_hip_recode_workspace_bytes(m, 5, T, R, 0),
        "recode_workspace_bytes dst": lambda m: lib.press_hip_recode_workspace_bytes(15, m, T, R, 1),
        "recode_packed_workspace_bytes src": lambda m: lib.press_hip_recode_packed_workspace_bytes(m, 5, T, R, 0),
        "recode_packed_workspace_bytes dst": lambda m: lib.press_hip_recode_packed_workspace_bytes(15, m, T, R, 0),
        "recode_degraded_workspace_bytes dst": lambda m: lib.press_hip_recode_degraded_workspace_bytes(15, m, 3, T, R, 0),
        "recode_degraded_workspace_bytes src": lambda m: lib.press_hip_recode_degraded_workspace_bytes(m, 5, 3, T, R, 0),
        "recode_degraded_packed_workspace_bytes dst": lambda m: lib.press_hip_recode_degraded_packed_workspace_bytes(15, m, 3, T, R, 0),
    }


def test_every_call_knows_the_extended_ids_and_no_others(cpu_lib):
    """-1, 19, 63, 88, 1000 and 1 << 20 are PRESS_HIP_EARG from every call of the table (0 from the questions) and 64 .. 87
    are not, with a device and without: an accepted id gets as far as the device (OK on an empty batch, or EHIP)"""
    for name, f in _calls(cpu_lib).items():
        for dr in (0, 1):
            for bad in BAD_IDS:
                assert f(bad, dr) == EARG and "method" in press.last_error(), (name, bad, dr)
        for mid in range(64, 88):  # (host pointers: what an empty batch writes - out_off[0], nbad - is host memory here)
            assert f(mid, 0) != EARG, (name, mid, press.last_error())
    for name, f in _questions(cpu_lib).items():
        for bad in BAD_IDS:
            assert f(bad) == 0, (name, bad)
        for mid in range(64, 88):
            assert f(mid) > 0, (name, mid)
    for bad in BAD_IDS:
        assert cpu_lib.press_hip_packed_exact(bad) == 0 and cpu_lib.press_hip_depress_pa_fused(bad) == 0
        assert cpu_lib.press_hip_recode_fused(bad, 84) == 0 and cpu_lib.press_hip_recode_fused(15, bad) == 0


def test_exact_and_fused_questions(cpu_lib):
    for name in STAGED:
        assert cpu_lib.press_hip_packed_exact(XM[name]) == 1 and press.packed_exact(name), name
    for name in CODERS:
        assert cpu_lib.press_hip_packed_exact(XM[name]) == 0, name
    fused_src = {press.METHODS[m] for m in ("svb12_zd", "svb_zd", "slow5_svb_zd")}
    for src in list(press.METHODS.values()) + list(range(64, 88)):
        for dst in range(64, 88):
            assert cpu_lib.press_hip_recode_fused(src, dst) == (1 if src in fused_src else 0), (src, dst)
        for dst in press.METHODS.values():
            if src >= 64:
                assert cpu_lib.press_hip_recode_fused(src, dst) == 0, (src, dst)
    for mid in range(64, 88):
        assert cpu_lib.press_hip_depress_pa_fused(mid) == 0


def test_workspace_questions(cpu_lib):
    """every question never shrinks in samples or reads over the grid of test_abi_symbols.py::test_workspace_bytes_without_gpu,
    is never below press_hip_workspace_bytes of the same id and shape, and the recode ones never below either half's"""
    totals = (0, 1, 1000, 32768, 1 << 20, 1 << 27, (1 << 31) + 4096)
    readss = (0, 1, 7, 512, 8192)
    lib = cpu_lib
    single = ("packed_", "depress_pa_", "depress_norm_", "verify_")
    for name in X21:
        m = XM[name]
        grid = {}
        for t in totals:
            for r in readss:
                base = int(lib.press_hip_workspace_bytes(m, t, r))
                row = [base] + [int(getattr(lib, "press_hip_%sworkspace_bytes" % f)(m, t, r)) for f in single]
                row.append(int(lib.press_hip_depress_chunks_workspace_bytes(m, t, r, 64, 8)))
                for other in (5, 15, 9):
                    for keep in (0, 1):
                        ob = int(lib.press_hip_workspace_bytes(other, t, r))
                        for q in (lib.press_hip_recode_workspace_bytes, lib.press_hip_recode_packed_workspace_bytes):
                            for pair in ((m, other), (other, m)):
                                v = int(q(pair[0], pair[1], t, r, keep))
                                assert v >= base and v >= ob, (name, other, t, r)
                                row.append(v)
                        for q in (lib.press_hip_recode_degraded_workspace_bytes, lib.press_hip_recode_degraded_packed_workspace_bytes):
                            v = int(q(other, m, 3, t, r, keep))
                            assert v >= base and v >= ob, (name, other, t, r)
                            row.append(v)
                assert base > 0 and min(row) >= base, (name, t, r)
                grid[t, r] = row
        for i, t in enumerate(totals):
            for j, r in enumerate(readss):
                if i:
                    assert all(x >= y for x, y in zip(grid[t, r], grid[totals[i - 1], r])), (name, t, r)
                if j:
                    assert all(x >= y for x, y in zip(grid[t, r], grid[t, readss[j - 1]])), (name, t, r)


# ------------------------------------------------------------------ GPU plumbing and the expectations

@pytest.fixture(scope="module")
def lib():
    for lb in PR.lib():
        press.load_table()
        yield lb


_memo = {}


def battery():
    if "b" not in _memo:
        _memo["b"] = L.battery()
    return _memo["b"]


def reads_of():
    return [s for _, s in battery()]


def names_of():
    return [n for n, _ in battery()]


def staged_expected(name, s):
    """the stream of a staged method for the samples s (None: an empty read)"""
    if len(s) == 0:
        return None
    stage, layout = parts(name)
    if stage == "rice":
        st, _, nbits = _rice.expected(layout, s)
        return _rice.clear_padding(st, len(_rcf.split(layout, s)[0]) * 8 + nbits)
    return _dhuf.expected(layout, s)[0]


def expected(name, bits=0):
    """the streams of the battery under `name` (the coder ids: the family's own press on the device, and its raw[])"""
    key = (name, bits)
    if key not in _memo:
        reads = reads_of()
        if name in STAGED:
            _memo[key] = [staged_expected(name, press.degrade(s, bits) if bits else s) for s in reads]
        else:
            stage, layout = parts(name)
            caps = [PR.slot_for(len(s)) for s in reads]
            st, raw = press.rcf_press_batch_host(stage, layout, reads, caps, want_raw=True)
            _memo[key] = st
            _memo[name, "raw"] = raw
    return _memo[key]


def raw_reads(name):
    """the reads whose payload the coder stored raw: they do not come back"""
    expected(name)
    return {n for n, f in zip(names_of(), _memo[name, "raw"]) if f}


def head_nlow(layout, s):
    head, low = _rcf.split(layout, s)
    return len(head), len(low)


def want_need(name, reads, streams):
    out = []
    for s, st in zip(reads, streams):
        if st is None:
            out.append(F64)
        elif name in STAGED:
            out.append(len(st))
        else:
            h, nlow = head_nlow(parts(name)[1], s)
            out.append(h + nlow + RC_SLACK)
    return np.array(out, dtype=np.uint64)


def layout_of(need, align):
    off = np.zeros(len(need) + 1, dtype=np.uint64)
    pos = end = 0
    for r, x in enumerate(need):
        off[r] = pos
        end = pos + (0 if int(x) == F64 else int(x))
        pos = (end + align - 1) // align * align
    off[len(need)] = end
    return off


def family(stage):
    """the generic calls as a _prefix_runs.Family: the layout picks the id"""
    def nm(l):
        return "%s_%s_zd" % (stage, l)

    def sizes(l, sig, off, n, need, tab):
        press._call("press_hip_press_sizes", press._mid(nm(l)), sig.data_ptr(), off.data_ptr(), n.data_ptr(), off.numel(), sig.numel(),
                    need.data_ptr(), 1)
    return PR.Family(lambda l, sig, off, n, out, oo, ol, tab: press.press_batch(nm(l), sig, off, n, out, oo, ol), sizes,
                     lambda l, *a: press.depress_batch(nm(l), *a), "no table")


def packed(run, name, align, cap):
    """press_packed of a PressRun's batch into a filled arena of `cap` bytes and a tail -> (arena, out_off, out_len)"""
    import torch
    out = torch.full((cap + 4096,), FILL8, dtype=torch.uint8, device="cuda")
    oo = torch.full((run.nr + 1,), -7, dtype=torch.int64, device="cuda")
    ol = torch.full((run.nr,), -7, dtype=torch.int64, device="cuda")
    press._call("press_hip_press_packed", press._mid(name), run.sig.data_ptr(), run.off.data_ptr(), run.n.data_ptr(), run.nr, run.sig.numel(),
                out.data_ptr(), cap, align, oo.data_ptr(), ol.data_ptr(), 1)
    torch.cuda.synchronize()
    return out.cpu().numpy(), oo.cpu().numpy().view(np.uint64), ol.cpu().numpy().view(np.uint64)


def check_packed(name, want, need, align, cap, arena, out_off, out_len):
    exp = layout_of(need, align)
    assert np.array_equal(out_off, exp), (name, align)
    touched = np.zeros(arena.size, dtype=bool)
    for r, w in enumerate(want):
        o = int(exp[r])
        if w is None or o + int(need[r]) > cap:
            assert int(out_len[r]) == F64, (name, align, r)
            continue
        if name in STAGED:
            assert int(out_len[r]) == len(w) == int(need[r]), (name, align, r)
        else:
            assert int(out_len[r]) == len(w) <= int(need[r]), (name, align, r)
        assert arena[o:o + len(w)].tobytes() == w, (name, align, r)
        touched[o:o + int(need[r])] = True  # (a coder's gap behind its stream is unspecified)
    assert (arena[~touched] == FILL8).all(), (name, align, "a byte outside the slots was written")
    assert (arena[min(cap, arena.size):] == FILL8).all(), (name, align, "a byte at or beyond out_cap was written")


# ------------------------------------------------------------------ 1: press, sizes, packed

@gpu
@pytest.mark.parametrize("stage", STAGES)
def test_press_sizes_and_packed(lib, stage):
    reads = reads_of()
    run = PR.PressRun(family(stage), reads, seed=11 + STAGES.index(stage))
    nonempty = [r for r, s in enumerate(reads) if len(s)]
    for layout in LAYOUTS:
        name = "%s_%s_zd" % (stage, layout)
        if name not in X21:
            continue
        want = expected(name)
        streams, _ = run.run(layout, want_tab=False)
        for r, (g, w) in enumerate(zip(streams, want)):
            assert g == w, (name, r, names_of()[r])
        c0 = press.xmethod_sizing_launches()
        need, _ = run.sizes(layout, want_tab=False)
        assert np.array_equal(need, want_need(name, reads, want)), name
        per_call = 1 if name in STAGED else 0
        assert press.xmethod_sizing_launches() == c0 + per_call, name
        for align in (1, 8):
            total = int(layout_of(need, align)[-1])
            c0 = press.xmethod_sizing_launches()
            check_packed(name, want, need, align, total, *packed(run, name, align, total))
            assert press.xmethod_sizing_launches() == c0 + per_call, (name, "the stage's sizes are taken once per packed call")
        k = nonempty[-3]
        exp = layout_of(need, 1)
        cap = int(exp[k]) + int(need[k]) // 2  # out_cap cut inside the third-last read that is not empty
        arena, out_off, out_len = packed(run, name, 1, cap)
        check_packed(name, want, need, 1, cap, arena, out_off, out_len)
        assert [int(x) == F64 for x in out_len[k:]] == [True] * (run.nr - k), name


# ------------------------------------------------------------------ 2: depress

@gpu
@pytest.mark.parametrize("stage", STAGES)
def test_depress_gives_the_samples_back(lib, stage):
    reads, names = reads_of(), names_of()
    small = {"walk-%d" % n for n in (2, 7, 8, 9, 63, 64, 65)}
    for layout in LAYOUTS:
        name = "%s_%s_zd" % (stage, layout)
        if name not in X21:
            continue
        want = expected(name)
        raw = set()
        if name in CODERS:
            raw = raw_reads(name)
            if stage != "rccdf":  # raw[] against the definition, on the CPU
                assert raw == {n for n, s in battery() if len(s) and _rcf.gave_up(stage, s)}, name
            assert raw <= small | {"walk-1"} and len(raw) <= 8, (name, raw)
            assert all(len(s) < 2047 for n, s in battery() if n in raw)
        keep = [r for r, w in enumerate(want) if w is not None]
        run = PR.DepressRun(family(stage), [want[r] for r in keep], [len(reads[r]) for r in keep], seed=5)
        got = run.run(layout)
        for r, g in zip(keep, got):
            assert g is not None, (name, names[r])
            if names[r] not in raw:
                assert np.array_equal(g, reads[r]), (name, names[r])


# ------------------------------------------------------------------ 3: recode

RECODE_SRC = ("slow5_svb_zd", "svb_zd", "vbe21_zd", "shuffman_vbbe21_zd", "zstd_svb_zd")
RECODE_X = STAGED + ["rccdf_vbe21_zd", "rc_vbbe21_zd"]
RECODE_BACK = ("slow5_svb_zd", "vbe21_zd", "huffman_vbe21_zd")


def public_streams(oracle, m):
    """the battery's streams under a public method from the oracle -> list (None: the oracle does not carry the read)"""
    key = ("pub", m)
    if key not in _memo:
        out = []
        for _, s in battery():
            ret, st = oracle.press(m, s, cap=L.slot_of(oracle.bound, m, len(s)))  # (a zstd kind: the frame itself)
            st = st if ret == 0 else None
            if st is not None:
                verdict, back = L.expect_depress(oracle, m, s, st, len(s))
                if verdict != "ok" or not np.array_equal(back, s):
                    st = None
            out.append(st)
        _memo[key] = out
    return _memo[key]


def source_streams(oracle, m):
    return expected(m) if m in XM and m not in press.METHODS else public_streams(oracle, m)


def dst_expected(oracle, m):
    if m in press.METHODS:
        return public_streams(oracle, m)
    return expected(m)


class Recode:
    """the reads `idx` of the battery as streams of `src` on the device, scattered; forged: {position: stream}"""

    def __init__(self, src, streams, idx, seed, forged=None):
        import torch
        self.torch, self.src, self.idx = torch, src, idx
        reads = reads_of()
        rng = np.random.default_rng(seed)
        sts = [streams[r] for r in idx]
        for k, st in (forged or {}).items():
            sts[k] = st
        self.forged = set(forged or {})
        self.rooms = np.array([len(reads[r]) for r in idx], dtype=np.uint32)
        arena, in_off, in_len = L.scatter_streams(rng, sts)
        self.off, self.total = L.scatter_rooms(rng, self.rooms)
        self.nr = len(idx)
        t = PR._t
        self.d = (t(arena), t(in_off, np.int64), t(in_len, np.int64), t(self.rooms, np.int32), t(self.off, np.int64))

    def _sig(self, keep):
        return self.torch.full((self.total,), L.SIG_FILL, dtype=self.torch.int16, device="cuda") if keep else None

    def _check_decoded(self, out_n, sig):
        torch, reads = self.torch, reads_of()
        torch.cuda.synchronize()
        on = out_n.cpu().numpy().view(np.uint32)
        for k, r in enumerate(self.idx):
            assert int(on[k]) == (F32 if k in self.forged else len(reads[r])), (self.src, k)
        if sig is not None:
            sg = sig.cpu().numpy()
            for k, r in enumerate(self.idx):
                if k not in self.forged:
                    o = int(self.off[k])
                    assert np.array_equal(sg[o:o + len(reads[r])], self.samples(r)), (self.src, k)
        return on

    def samples(self, r):
        s = reads_of()[r]
        return press.degrade(s, self.bits) if self.bits else s

    def batch(self, dst, want, keep, bits=0):
        torch = self.torch
        self.bits = bits
        caps = [PR.slot_for(int(n)) for n in self.rooms]
        out_off = L.slots(np.random.default_rng(3), np.asarray(caps, dtype=np.uint64))
        out = torch.full((int(out_off[-1]) + 64,), FILL8, dtype=torch.uint8, device="cuda")
        ol = torch.full((self.nr,), -7, dtype=torch.int64, device="cuda")
        on = torch.zeros(self.nr, dtype=torch.int32, device="cuda")
        sig = self._sig(keep)
        press.recode_batch(self.src, dst, *self.d, out, PR._t(out_off, np.int64), ol, on, sig=sig, total_samples=self.total, degrade_bits=bits)
        self._check_decoded(on, sig)
        a, lens = out.cpu().numpy(), ol.cpu().numpy().view(np.uint64)
        touched = np.zeros(a.size, dtype=bool)
        for k, r in enumerate(self.idx):
            o = int(out_off[k])
            if k in self.forged or want[r] is None:
                assert int(lens[k]) == F64, (self.src, dst, k)
                continue
            assert int(lens[k]) == len(want[r]) and a[o:o + len(want[r])].tobytes() == want[r], (self.src, dst, k, names_of()[r])
            touched[o:int(out_off[k + 1])] = True
        assert (a[~touched] == FILL8).all(), (self.src, dst, "a byte outside the slots of the recoded reads was written")

    def sizes_and_packed(self, dst, want, need_of, keep, bits=0, align=1):
        torch = self.torch
        self.bits = bits
        on = torch.zeros(self.nr, dtype=torch.int32, device="cuda")
        sig = self._sig(keep)
        need = press.recode_sizes(self.src, dst, *self.d, on, sig=sig, total_samples=self.total, degrade_bits=bits)
        self._check_decoded(on, sig)
        need = need.cpu().numpy().view(np.uint64)
        exp_need = np.array([F64 if k in self.forged or want[r] is None else need_of(r) for k, r in enumerate(self.idx)], dtype=np.uint64)
        assert np.array_equal(need, exp_need), (self.src, dst)
        exp = layout_of(need, align)
        total = int(exp[-1])
        out = torch.full((total + 4096,), FILL8, dtype=torch.uint8, device="cuda")
        oo = torch.full((self.nr + 1,), -7, dtype=torch.int64, device="cuda")
        ol = torch.full((self.nr,), -7, dtype=torch.int64, device="cuda")
        on = torch.zeros(self.nr, dtype=torch.int32, device="cuda")
        sig = self._sig(not keep)
        press._call_degraded("recode_packed", bits, press._mid(self.src), press._mid(dst), *[x.data_ptr() for x in self.d], self.nr, self.total,
                             out.data_ptr(), total, align, oo.data_ptr(), ol.data_ptr(), None if sig is None else sig.data_ptr(),
                             on.data_ptr(), 1)
        self._check_decoded(on, sig)
        a = out.cpu().numpy()
        assert np.array_equal(oo.cpu().numpy().view(np.uint64), exp), (self.src, dst)
        lens = ol.cpu().numpy().view(np.uint64)
        touched = np.zeros(a.size, dtype=bool)
        for k, r in enumerate(self.idx):
            o = int(exp[k])
            if int(need[k]) == F64:
                assert int(lens[k]) == F64 and int(exp[k + 1]) == o, (self.src, dst, k)  # refused: FAILED, no byte of the layout
                continue
            assert int(lens[k]) == len(want[r]) and a[o:o + len(want[r])].tobytes() == want[r], (self.src, dst, k, names_of()[r])
            touched[o:o + int(need[k])] = True
        assert (a[~touched] == FILL8).all(), (self.src, dst, "a byte outside the slots was written")


def need_fn(dst, want):
    reads = reads_of()
    if dst in CODERS or dst in ("rc_vbe21_zd", "rcc_vbe21_zd", "rccm_vbbe21_zd"):
        return lambda r: sum(head_nlow(parts(dst)[1], reads[r])) + RC_SLACK
    return lambda r: len(want[r])


def recode_pair(oracle, src, dst, seed, keep):
    srcs, want = source_streams(oracle, src), dst_expected(oracle, dst)
    skip = raw_reads(src) if src in CODERS else set()
    # (an empty read the source has a stream for stays in: the destination refuses it alone)
    idx = [r for r, st in enumerate(srcs) if st is not None and (want[r] is not None or not len(reads_of()[r])) and names_of()[r] not in skip]
    assert len(idx) >= 17, (src, dst, len(idx))
    rc = Recode(src, srcs, idx, seed)
    fused = press.recode_fused(src, dst)
    a0 = press.pass_a_launches()
    rc.batch(dst, want, keep)
    rc.sizes_and_packed(dst, want, need_fn(dst, want), keep, align=8 if seed % 2 else 1)
    exsplit = dst not in L.SVB_KINDS and dst not in L.ZSTD_KINDS  # (pass A is the exception-split press's)
    assert press.pass_a_launches() == a0 + (3 if exsplit and not fused else 0), (src, dst)


@gpu
@pytest.mark.parametrize("src", RECODE_SRC)
def test_recode_into_the_families(lib, oracle, src):
    for i, dst in enumerate(RECODE_X):
        assert press.recode_fused(src, dst) == (src in ("slow5_svb_zd", "svb_zd"))
        recode_pair(oracle, src, dst, 100 * RECODE_SRC.index(src) + i, keep=i % 2 == 0)


@gpu
@pytest.mark.parametrize("src", RECODE_X)
def test_recode_out_of_the_families(lib, oracle, src):
    for i, dst in enumerate(RECODE_BACK):
        recode_pair(oracle, src, dst, 1000 + 10 * RECODE_X.index(src) + i, keep=i % 2 == 1)


@gpu
@pytest.mark.parametrize("src,dst", [("slow5_svb_zd", "huffman_vbbe21_zd"), ("huffman_vbe21_zd", "rice_vbsse21_zd"), ("slow5_svb_zd", "rccdf_vbe21_zd")])
def test_a_forged_source_read_is_refused_alone(lib, oracle, src, dst):
    """a truncated stream in the middle of the batch: out_n = UINT32_MAX, need = out_len = FAILED, no byte of the layout,
    and the neighbours are what they are without it"""
    srcs, want = source_streams(oracle, src), dst_expected(oracle, dst)
    idx = [r for r, st in enumerate(srcs) if st is not None and want[r] is not None]
    k = len(idx) // 2
    while len(reads_of()[idx[k]]) < 2000:
        k += 1
    st = srcs[idx[k]]
    rc = Recode(src, srcs, idx, 77, forged={k: st[:len(st) - (1 if src == "slow5_svb_zd" else len(st) // 3)]})
    rc.batch(dst, want, True)
    rc.sizes_and_packed(dst, want, need_fn(dst, want), False)


# ------------------------------------------------------------------ 4: degrade

@gpu
@pytest.mark.parametrize("src", ["slow5_svb_zd", "vbe21_zd"])
def test_degraded_recode_and_verify(lib, oracle, src):
    import torch
    srcs = public_streams(oracle, src)
    reads = reads_of()
    for bits, dsts in ((3, STAGED), (8, ["huffman_vbe21_zd"])):
        for i, dst in enumerate(dsts):
            want = expected(dst, bits)
            idx = [r for r, st in enumerate(srcs) if st is not None and want[r] is not None]
            rc = Recode(src, srcs, idx, 40 + i)
            a0 = press.pass_a_launches()
            rc.batch(dst, want, i % 2 == 0, bits=bits)
            assert press.pass_a_launches() == a0 + (0 if src == "slow5_svb_zd" else 1)
            if i % 4 == 0:
                rc.sizes_and_packed(dst, want, need_fn(dst, want), True, bits=bits)
            # the degraded archive against the originals
            sub = [reads[r] for r in idx]
            fb, on, nbad = press.verify_batch_host(dst, [want[r] for r in idx], sub, degrade_bits=bits)
            assert nbad == 0 and (fb == press.VERIFIED).all() and list(on) == [len(s) for s in sub], (src, dst, bits)
            if i == 0:
                k = max(range(len(sub)), key=lambda j: len(sub[j]))
                bent = [s.copy() for s in sub]
                at = len(bent[k]) // 2 + 5
                bent[k][at] = np.int16(int(bent[k][at]) ^ 0x4000)
                fb, on, nbad = press.verify_batch_host(dst, [want[r] for r in idx], bent, degrade_bits=bits)
                assert nbad == 1 and int(fb[k]) == at and sum(int(x) != press.VERIFIED for x in fb) == 1, (dst, bits)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 5: verify, CRC, floats, rows

CONSUMERS = ("rice_vbsse21_zd", "huffman_vbe21_zd", "huffman_vbbe21_zd", "rccdf_vbsbe21_zd")


class Decode:
    def __init__(self, streams, reads, seed=9):
        import torch
        self.torch = torch
        rng = np.random.default_rng(seed)
        self.reads, self.nr = reads, len(reads)
        self.ns = np.array([len(s) for s in reads], dtype=np.uint32)
        arena, in_off, in_len = L.scatter_streams(rng, streams)
        self.off, self.total = L.scatter_rooms(np.random.default_rng(seed + 1), self.ns)  # (the same rooms whatever the streams are)
        t = PR._t
        self.comp = (t(arena), t(in_off, np.int64), t(in_len, np.int64))
        self.d_off, self.d_n = t(self.off, np.int64), t(self.ns, np.int32)
        sig = np.zeros(self.total, dtype=np.int16)
        for s, o in zip(reads, self.off):
            sig[int(o):int(o) + len(s)] = s
        self.sig = t(sig)

    def results(self, m):
        """every consumer call on the streams as method m -> a dict of numpy arrays, bit patterns"""
        torch = self.torch
        z32 = lambda k=self.nr: torch.zeros(k, dtype=torch.int32, device="cuda")
        out = {}
        fb, on, nbad = z32(), z32(), z32(1)
        press.verify_batch(m, *self.comp, self.sig, self.d_off, self.d_n, fb, on, nbad)
        out["first_bad"], out["verify_out_n"], out["nbad"] = fb, on, nbad
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
        row_first, _, _ = press.chunk_plan(self.ns, 64, 8)
        for dt in (torch.float16, torch.float32):
            rows = torch.zeros((int(row_first[-1]), 64), dtype=dt, device="cuda")
            on, q = z32(), z32(2 * self.nr)
            press.depress_chunks_batch(m, *self.comp, rows, PR._t(row_first, np.int64), self.d_off, self.d_n, self.total, on, 8, q=q)
            out["rows-%s" % dt] = rows.view(torch.int16 if dt == torch.float16 else torch.int32)
            out["rows-q-%s" % dt] = q
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}


@gpu
@pytest.mark.parametrize("name", CONSUMERS)
def test_consumers_match_the_public_methods(lib, oracle, name):
    base = public_streams(oracle, "vbe21_zd")
    want = expected(name)
    skip = raw_reads(name) if name in CODERS else set()
    idx = [r for r, (a, b) in enumerate(zip(base, want)) if a is not None and b is not None and names_of()[r] not in skip]
    assert len(idx) >= 18
    reads = [reads_of()[r] for r in idx]
    key = ("consumers", tuple(idx))
    if key not in _memo:
        _memo[key] = Decode([base[r] for r in idx], reads).results("vbe21_zd")
    ref = _memo[key]
    got = Decode([want[r] for r in idx], reads).results(name)
    assert sorted(ref) == sorted(got)
    for k in ref:
        assert ref[k].dtype == got[k].dtype and np.array_equal(ref[k], got[k]), (name, k)
    assert int(got["nbad"][0]) == 0 and (got["first_bad"].view(np.uint32) == press.VERIFIED).all()
    assert [int(c) for c in got["crc"].view(np.uint32)] == [zlib.crc32(s.tobytes()) for s in reads], name


@gpu
def test_a_damaged_table_byte_is_refused_alone(lib):
    name = "huffman_vbe21_zd"
    want = expected(name)
    reads, names = reads_of(), names_of()
    idx = [r for r, w in enumerate(want) if w is not None]
    k = idx.index(names.index("ex1-32768"))
    streams = [want[r] for r in idx]
    head = _rice.head_len("vbe21", reads[idx[k]])
    b = bytearray(streams[k])
    b[head + 6] = 0  # the first entry's code length: 0 in a table of several entries (definition 4)
    streams[k] = bytes(b)
    sub = [reads[r] for r in idx]
    fb, on, nbad = press.verify_batch_host(name, streams, sub)
    assert nbad == 1 and int(fb[k]) == 0 and int(on[k]) == F32
    assert all(int(x) == press.VERIFIED for j, x in enumerate(fb) if j != k)
    crc, on = press.depress_crc_batch_host(name, streams, [len(s) for s in sub])
    assert int(crc[k]) == 0 and int(on[k]) == F32
    assert all(int(crc[j]) == zlib.crc32(sub[j].tobytes()) for j in range(len(sub)) if j != k)


# ------------------------------------------------------------------ 6: host pointers

SIX = ("walk-1", "walk-65", "ex1-2049", "ex1-32769", "all-exceptions-3000", "constant-4000")


@gpu
@pytest.mark.parametrize("name", ["rice_vbbe21_zd", "huffman_vbsbe21_zd", "rccdf_vbsse21_zd"])
def test_host_pointer_forms(lib, oracle, name):
    names = names_of()
    idx = [names.index(n) for n in SIX]
    reads = [reads_of()[r] for r in idx]
    want = [expected(name)[r] for r in idx]
    caps = [PR.slot_for(len(s)) for s in reads]
    assert press.press_batch_host(name, reads, caps) == want
    streams, total = press.press_packed_host(name, reads, align=8)
    assert streams == want
    if name in STAGED:
        assert total == int(layout_of(np.array([len(w) for w in want], dtype=np.uint64), 8)[-1])
    raw = raw_reads(name) if name in CODERS else set()
    back = press.depress_batch_host(name, want, [len(s) for s in reads])
    for n, g, s in zip(SIX, back, reads):
        assert g is not None and (n in raw or np.array_equal(g, s)), (name, n)
    # recode, both ways
    src = public_streams(oracle, "slow5_svb_zd")
    got, sam = press.recode_batch_host("slow5_svb_zd", name, [src[r] for r in idx], [len(s) for s in reads], caps, want_samples=True)
    assert got == want and all(np.array_equal(a, b) for a, b in zip(sam, reads))
    got, total = press.recode_packed_host("slow5_svb_zd", name, [src[r] for r in idx], [len(s) for s in reads])
    assert got == want
    ok = [j for j, n in enumerate(SIX) if n not in raw]
    vb = public_streams(oracle, "vbe21_zd")
    got = press.recode_batch_host(name, "vbe21_zd", [want[j] for j in ok], [len(reads[j]) for j in ok], [caps[j] for j in ok])
    assert got == [vb[idx[j]] for j in ok]
    # the consumers
    sub, st = [reads[j] for j in ok], [want[j] for j in ok]
    ns = [len(s) for s in sub]
    fb, on, nbad = press.verify_batch_host(name, st, sub)
    assert nbad == 0 and (fb == press.VERIFIED).all()
    crc, on = press.depress_crc_batch_host(name, st, ns)
    assert [int(c) for c in crc] == [zlib.crc32(s.tobytes()) for s in sub]
    ref = [vb[idx[j]] for j in ok]
    cals = np.tile(np.array([[3.5, 0.1748]], dtype=np.float32), (len(sub), 1))
    for a, b in zip(press.depress_pa_batch_host(name, st, ns, cals), press.depress_pa_batch_host("vbe21_zd", ref, ns, cals)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    (a, sa), (b, sb) = press.depress_norm_batch_host(name, st, ns), press.depress_norm_batch_host("vbe21_zd", ref, ns)
    assert np.array_equal(sa, sb) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    for dt, view in (("float16", np.uint16), ("float32", np.uint32)):
        a = press.depress_chunks_batch_host(name, st, ns, 64, 8, dtype=dt)
        b = press.depress_chunks_batch_host("vbe21_zd", ref, ns, 64, 8, dtype=dt)
        assert np.array_equal(a[0].view(view), b[0].view(view)) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])


# ------------------------------------------------------------------ 7: nothing depends on what scratch held

@gpu
@pytest.mark.parametrize("src,dst", [("slow5_svb_zd", "huffman_vbe21_zd"), ("huffman_vbe21_zd", "rice_vbe21_zd")])
def test_recode_behind_filled_scratch(lib, oracle, src, dst):
    import torch
    srcs, want = source_streams(oracle, src), dst_expected(oracle, dst)
    idx = [r for r, st in enumerate(srcs) if st is not None and want[r] is not None]
    for byte in (0x00, 0xFF, 0xA5):
        torch.cuda.synchronize()
        press.scratch_fill(byte)
        rc = Recode(src, srcs, idx, 5)
        rc.batch(dst, want, False)
        rc.sizes_and_packed(dst, want, need_fn(dst, want), False)
