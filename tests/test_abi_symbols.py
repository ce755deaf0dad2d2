"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/press_hip.h declares.  No compute calls (no GPU here)."""
import os
import re

import pytest

from honours_amd import build, press

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return press.load_library()


def _declared_symbols():
    """function names declared in include/press_hip.h (incl. the macro-free drop-in list)"""
    src = open(os.path.join(ROOT, "include", "press_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b([a-z_][a-z0-9_]*)\s*\([^;{]*\)\s*;", src))
    return {n for n in names if n not in ("defined",)}


def test_header_symbols_exported(lib):
    decl = _declared_symbols()
    assert len(decl) >= 60
    missing = [s for s in sorted(decl) if not hasattr(lib, s)]
    assert not missing, missing
    # and the python mirror knows the same list
    assert set(press.HEADER_SYMBOLS) == decl


def _declared_prototypes():
    """name -> (return type, [parameter declarations]) of every function include/press_hip.h declares, as C text"""
    src = open(os.path.join(ROOT, "include", "press_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)  # (a return type is not to reach back into a #define)
    decl = re.findall(r"((?:\b[A-Za-z_][A-Za-z0-9_]*\b[\s*]+)+)\b([a-z_][a-z0-9_]*)\s*\(([^;{]*)\)\s*;", src)
    out = {}
    for ret, name, params in decl:
        ret = re.sub(r"\s*\*\s*", " *", " ".join(ret.split())).strip()
        ret = re.sub(r"^(?:extern|static|inline)\s+", "", ret)
        params = " ".join(params.split())
        out[name] = (ret, [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    return out


def _c_class(text, is_return):
    """the ctypes class a C parameter declaration or return type must be bound as"""
    import ctypes

    if "*" in text or "[" in text:
        return ctypes.c_char_p if re.match(r"const char \*[a-z_]*$", text) else ctypes.c_void_p
    scalar = {"int": ctypes.c_int, "int16_t": ctypes.c_int16, "uint32_t": ctypes.c_uint32, "unsigned int": ctypes.c_uint32,
              "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}
    if is_return:
        scalar.update({"void": None, "bool": ctypes.c_bool})
        return scalar[text]
    return scalar[text.rsplit(" ", 1)[0]]  # (every parameter of the header is named)


def test_prototypes_match_header():
    """the table honours_amd/abi.py binds the library with says what the header says: for every declared function the
    same number of parameters, each of the ctypes class of its C type (a pointer or array: c_void_p, `const char *`:
    c_char_p), and the same return type.  A wrong arity, or a uint64_t bound as c_uint32, fails here and not at the first
    large value."""
    from honours_amd import abi

    decl = _declared_prototypes()
    assert set(decl) == _declared_symbols() and len(decl) >= 200
    assert set(abi.PROTOS) == set(decl) and press.HEADER_SYMBOLS == sorted(decl)
    for name, (ret, params) in sorted(decl.items()):
        restype, argtypes = abi.PROTOS[name]
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for k, (got, text) in enumerate(zip(argtypes, params)):
            assert got is _c_class(text, False), (name, k, text, got)
        assert restype is _c_class(ret, True), (name, ret, restype)


def test_bounds_match_oracle(lib, oracle):
    """X_bound is host arithmetic: same values as the oracle"""
    for m in press.METHODS:
        for n in (1, 2, 7, 8, 9, 1000, 7329, 155185, 200000, 5724000):
            assert press.bound(m, n) == oracle.bound(m, n), (m, n)
            assert lib.press_hip_bound(press.METHODS[m], n) == oracle.bound(m, n), (m, n)


def test_huffman_objects_roundtrip(lib, oracle):
    """read_code_table + build_symbol_encoder (press/test.c:3786-3791) reproduce the codes"""
    import ctypes

    t = press.HuffmanTable()
    want = oracle.table()
    se = ctypes.cast(t.se, ctypes.POINTER(ctypes.c_void_p * 256)).contents

    class Code(ctypes.Structure):
        _fields_ = [("numbits", ctypes.c_ulong), ("bits", ctypes.POINTER(ctypes.c_ubyte))]

    for s in range(256):
        c = ctypes.cast(se[s], ctypes.POINTER(Code)).contents
        bits = 0
        for k in range(c.numbits):
            if c.bits[k // 8] & (1 << (k % 8)):
                bits |= 1 << k
        assert (c.numbits, bits) == want[s], s
    t.close()


def test_no_gpu_fails_loudly(lib):
    """without a device the product path reports an error - it never falls back to the CPU"""
    import numpy as np
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ret, out = press.press("hasgam_vbsse21_zdq", np.arange(100, dtype=np.int16))
    assert ret != 0 and out == b""
    assert "HIP" in press.last_error() or "hip" in press.last_error()


def test_scratch_registry_without_gpu():
    """every scratch buffer of the library is on the list press_hip_shutdown() walks (a buffer cannot be
    forgotten: it links itself in when it is constructed); nothing is allocated before the first call"""
    import ctypes

    lib = press.load_library()
    lib.press_hip_scratch_buffers.restype = ctypes.c_uint32
    lib.press_hip_scratch_buffers.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    nbytes = ctypes.c_uint64(1)
    nbuf = lib.press_hip_scratch_buffers(ctypes.byref(nbytes))
    # as many as the context declares (DevBuf a, b, c; lines of struct Ctx)
    src = open(os.path.join(os.path.dirname(build.CSRC), "csrc", "press_host.h")).read()
    declared = sum(len(l.split(";")[0].split(",")) for l in re.findall(r"^\tDevBuf ([a-z][^;]*;)", src, re.M))
    assert nbuf == declared >= 40, (nbuf, declared)
    import torch
    if not torch.cuda.is_available():
        assert nbytes.value == 0
    lib.press_hip_shutdown()  # harmless without a context


def test_scratch_fill_without_gpu():
    """the diagnostic fill needs the device like every entry point that touches scratch: PRESS_HIP_EHIP without one,
    and the registry reports what it reported before"""
    import ctypes

    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = press.load_library()
    lib.press_hip_scratch_buffers.restype = ctypes.c_uint32
    lib.press_hip_scratch_buffers.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    before = ctypes.c_uint64(1)
    nbuf = lib.press_hip_scratch_buffers(ctypes.byref(before))
    assert lib.press_hip_scratch_fill(0xA5) == -3  # PRESS_HIP_EHIP
    assert "HIP" in press.last_error() or "hip" in press.last_error()
    with pytest.raises(press.PressError):
        press.scratch_fill(0xA5)
    after = ctypes.c_uint64(1)
    assert lib.press_hip_scratch_buffers(ctypes.byref(after)) == nbuf and after.value == before.value == 0


def test_workspace_bytes_without_gpu():
    """press_hip_workspace_bytes is the scratch plan summed (host arithmetic, no device): for every buffer the larger
    of what press and depress reserve, plus the device table for the Huffman methods.  It never shrinks when the batch
    grows, holds ReadMeta (32 bytes a read) and the two exception lists (2 x 4 bytes a sample; Huffman: and the
    one-byte values), and for the svb methods stays a few MB at the sample count of test_c2_samples_past_2g."""
    import ctypes

    lib = press.load_library()
    lib.press_hip_workspace_bytes.restype = ctypes.c_uint64
    lib.press_hip_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32]
    totals = [1000, 100_000, 10_000_000, 930_000_000, (1 << 31) + (1 << 20)]
    reads = [1, 5, 64, 8192]
    svb = ("svb12", "svb12_zd", "svb_zd", "slow5_svb_zd")
    for m, mid in press.METHODS.items():
        ws = {(t, r): int(lib.press_hip_workspace_bytes(mid, t, r)) for t in totals for r in reads}
        for (t, r), w in ws.items():
            assert w >= 32 * (r + 1), (m, t, r, w)
            if m.startswith("shuffman_"):
                assert w >= 9 * t, (m, t, r, w)
            elif not m.startswith("zstd_") and m not in svb:  # exception split, ex-zd, range coders
                assert w >= 8 * t, (m, t, r, w)
            assert all(w <= ws[(t2, r)] for t2 in totals if t2 >= t), (m, t, r)
            assert all(w <= ws[(t, r2)] for r2 in reads if r2 >= r), (m, t, r)
        if m in svb:
            assert ws[((1 << 31) + (1 << 20), 5)] < 10 ** 9, (m, ws[((1 << 31) + (1 << 20), 5)])


def test_one_libzstd_per_process():
    """round 2's abort under rocprofv3 ("munmap_chunk(): invalid pointer"): the profiler's tool library had the
    system's libzstd in the global scope and the library / bench.py opened another version by absolute path - the
    second copy's internal calls bound to the first and freed its memory.  With a libzstd preloaded the way the
    profiler does it, both openers must bind to THAT copy and compress without aborting."""
    import glob
    import subprocess
    import sys

    sys_z = [p for p in glob.glob("/usr/lib/x86_64-linux-gnu/libzstd.so.1") + glob.glob("/lib/x86_64-linux-gnu/libzstd.so.1")]
    if not sys_z:
        pytest.skip("no system libzstd to preload")
    code = (
        "import ctypes, numpy as np\n"
        "from honours_amd import press\n"
        "z = press.open_libzstd()\n"
        "src = np.tile(np.arange(50, dtype=np.uint8), 4000); dst = np.zeros(src.size + 1024, dtype=np.uint8)\n"
        "c = z.ZSTD_compress(dst.ctypes.data, dst.size, src.ctypes.data, src.size, 1)\n"
        "assert not z.ZSTD_isError(c) and 0 < c < src.size\n"
        "lib = press.load_library()\n"
        "assert press.bound('zstd_svb_zd', 100000) > 100000\n"   # the library's own dlopen (zstd_open)
        "c = z.ZSTD_compress(dst.ctypes.data, dst.size, src.ctypes.data, src.size, 1)\n"
        "assert not z.ZSTD_isError(c)\n"
        "print('ok')\n")
    env = dict(os.environ, LD_PRELOAD=sys_z[0], PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stderr[-500:])
