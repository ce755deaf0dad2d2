"""Host-side mirror of the reference's per-method interface (press/press.h) over
libpress_hip.so, plus the batch entry points.

Per-read calls go through the DROP-IN C symbols (``svb12_zd_press`` ...) exactly as
press/test.c's ``test_X`` functions call them (test.c:1756-1815): bound -> press ->
depress.  Batch calls take torch CUDA tensors (device memory plumbing only) and enqueue
on torch's current stream.

No fallback: if the library is missing or no GPU is present, calls raise.
"""
import ctypes
import os

import numpy as np

from .abi import (HEADER_SYMBOLS, LIB_PATH, METHODS, RCF_CODERS, RCF_LAYOUTS, SMETHODS, STALL_METHODS, XMETHODS,  # noqa: F401
                  _SYMS, PressError, load_library)
from . import abi

TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "NA12878_zd.huffman")
BATCH_METHODS = [m for m in METHODS if not m.startswith("zstd_")]
FAILED = (1 << 64) - 1


def open_libzstd():
    """ctypes handle to a libzstd for tests and bench.py (never the product path), or None.  The copy the process
    already holds comes first: a second copy of another version frees the first one's allocations and glibc aborts
    ("free(): invalid pointer" - round 2's rocprofv3 run); an absolute path only last, bound
    to itself (RTLD_DEEPBIND)."""
    tries = [("libzstd.so.1", os.RTLD_NOW | os.RTLD_NOLOAD), ("libzstd.so.1", os.RTLD_NOW), ("libzstd.so", os.RTLD_NOW),
             ("/opt/conda/lib/libzstd.so.1", os.RTLD_NOW | os.RTLD_DEEPBIND)]
    for name, mode in tries:
        try:
            return abi.declare(ctypes.CDLL(name, mode=mode), abi.ZSTD)
        except OSError:
            continue
    return None


def last_error():
    return load_library().press_hip_last_error().decode()


def _call(name, *args):
    """the library's `name`, which returns a status: raises what the library reports unless it is 0"""
    if getattr(load_library(), name)(*args):
        raise PressError(last_error())


def _ptr(x):
    """the address of a torch tensor, a numpy array or a ctypes structure; None for None"""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return ctypes.addressof(x) if isinstance(x, ctypes.Structure) else x.data_ptr()


def _mid(method):
    """a method's id: a name of METHODS, of XMETHODS (the families' methods in the generic calls) or of SMETHODS (the stall
    methods there), or the id itself"""
    if isinstance(method, str):
        return METHODS[method] if method in METHODS else SMETHODS[method] if method in SMETHODS else XMETHODS[method]
    return int(method)


class HuffmanTable:
    """The caller-owned table objects of press/test.c:3786-3791: read_code_table on the
    table file, then build_symbol_encoder into a malloc'd SymbolEncoder."""

    def __init__(self, path=TABLE_PATH):
        lib = load_library()
        fp = lib._libc.fopen(path.encode(), b"r")
        if not fp:
            raise PressError("cannot open " + path)
        self.root = ctypes.c_void_p()
        nbytes = ctypes.c_uint()
        ok = lib.read_code_table(fp, ctypes.byref(self.root), ctypes.byref(nbytes))
        lib._libc.fclose(fp)
        if not ok:
            raise PressError("read_code_table failed on " + path)
        self.se = lib._libc.malloc(256 * ctypes.sizeof(ctypes.c_void_p))
        ctypes.memset(self.se, 0, 256 * ctypes.sizeof(ctypes.c_void_p))
        lib.build_symbol_encoder(self.root, self.se)

    def close(self):
        lib = load_library()
        if self.se:
            lib.free_encoder(self.se)
            self.se = None
        if self.root:
            lib.free_huffman_tree(self.root)
            self.root = None


_table = None


def default_table():
    global _table
    if _table is None:
        _table = HuffmanTable()
    return _table


def use_table(path=TABLE_PATH):
    """Make `path` the table of the shuffman_* calls: the caller-owned objects the per-read
    functions receive, and the batch API's table (press_hip_load_table_file)."""
    global _table
    new = HuffmanTable(path)
    if _table is not None:
        _table.close()
    _table = new
    load_table(path)


def _press_16(name, sig, cap, table=None):
    """the per-read symbol `name` (table: the encoder a shuffman_* symbol takes first) on one read, with a canary behind
    the capacity -> (ret, bytes); ret as the reference returns it (void symbols: 0, or -1 when the library reports
    *nout = 0)"""
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    out = np.zeros(cap + 64, dtype=np.uint8)
    out[cap:] = 0xA5  # canary: nothing may be written past the capacity
    nout = ctypes.c_uint64(cap)
    ret = getattr(load_library(), name)(*(() if table is None else (table,)), sig.ctypes.data, sig.size, out.ctypes.data,
                                        ctypes.byref(nout))
    if not np.all(out[cap:] == 0xA5):
        raise PressError("%s wrote past its capacity" % name)
    if ret is None:
        ret = 0 if nout.value else -1
    return ret, (out[: nout.value].tobytes() if ret == 0 else b"")


def _depress_16(name, comp, nin, n, kind="vb", table=None):
    """the per-read symbol `name` of calling convention `kind` (table: the tree a shuffman_* symbol takes first) on one
    stream, nin what it is given as the input's size, with a canary behind the n samples -> (ret, int16 array)"""
    buf = np.frombuffer(bytes(comp) + b"\0" * 64, dtype=np.uint8).copy()
    out = np.zeros(n + 64, dtype=np.int16)
    out[n:] = 0x5A5A
    nout = (ctypes.c_uint64 if kind == "svb" else ctypes.c_uint32)(n)
    args = (() if table is None else (table,)) + (buf.ctypes.data, nin, out.ctypes.data)
    ret = getattr(load_library(), name)(*args, *(() if kind == "svb_nz" else (ctypes.byref(nout),)))
    if not np.all(out[n:] == 0x5A5A):
        raise PressError("%s wrote past the sample capacity" % name)
    if ret is None:
        ret = -1 if kind == "vb" and nout.value == 0 else 0
    return ret, out[:nout.value].copy()


def bound(method, n):
    """X_bound(n): what press/test.c mallocs for the compressed read (a family's method of XMETHODS: press_hip_bound)."""
    if method not in _SYMS and (method in XMETHODS or method in SMETHODS):
        return int(load_library().press_hip_bound(_mid(method), n))
    return int(getattr(load_library(), _SYMS[method][0])(n))


def press(method, sig, cap=None):
    """X_press through the drop-in symbol. -> (ret, bytes); ret as the reference returns it
    (void methods: 0, or -1 when the library reports *nout = 0)."""
    _, pname, _, kind = _SYMS[method]
    cap = bound(method, np.size(sig)) + 1024 if cap is None else int(cap)
    return _press_16(pname, sig, cap, default_table().se if kind == "shuff" else None)


def depress(method, comp, n):
    """X_depress through the drop-in symbol. -> (ret, int16 array)"""
    _, _, dname, kind = _SYMS[method]
    return _depress_16(dname, comp, n if kind in ("svb", "svb_nz") else len(comp), n, kind,
                       default_table().root if kind == "shuff" else None)


# ---------------------------------------------------------------------------- host buffers of the batch calls

def _layout(ns):
    """read starts padded to multiples of 8 samples -> (off uint64[nreads], total)"""
    ns = np.asarray(ns, dtype=np.int64)
    pad = (ns + 7) // 8 * 8
    off = np.zeros(ns.size, dtype=np.uint64)
    if ns.size > 1:
        off[1:] = np.cumsum(pad)[:-1]
    return off, int(pad.sum())


def _host_batch(reads, alloc=np.zeros):
    """a list of int16 arrays laid out by _layout in one arena from alloc(count, dtype), which returns zeros
    -> (sig, off, ns uint32, total)"""
    ns = np.array([len(r) for r in reads], dtype=np.uint32)
    off, total = _layout(ns)
    sig = alloc(total + 64, np.int16)
    for r, o in zip(reads, off):
        sig[int(o): int(o) + len(r)] = r
    return sig, off, ns, total


def _streams_arena(streams):
    """a list of bytes end to end in one arena with 64 zero bytes behind -> (comp uint8, in_off uint64, in_len uint64)"""
    nreads = len(streams)
    in_len = np.array([len(s) for s in streams], dtype=np.uint64)
    in_off = np.zeros(nreads, dtype=np.uint64)
    if nreads > 1:
        in_off[1:] = np.cumsum(in_len)[:-1]
    return np.frombuffer(b"".join(streams) + b"\0" * 64, dtype=np.uint8).copy(), in_off, in_len


def _decode_batch(streams, ns):
    """what every host decode form lays out: the streams' arena and the layout of the samples they decode to
    -> (comp, in_off, in_len, ns uint32, off, total)"""
    ns = np.asarray(ns, dtype=np.uint32)
    return _streams_arena(streams) + (ns,) + _layout(ns)


def _slots(caps):
    """output slots of `caps` bytes, each rounded up to 16 -> out_off uint64[nreads + 1]"""
    out_off = np.zeros(len(caps) + 1, dtype=np.uint64)
    out_off[1:] = np.cumsum((np.asarray(caps, dtype=np.uint64) + 15) // 16 * 16)
    return out_off


def _streams_of(out, out_off, out_len):
    """the streams a press call left in `out` -> list of bytes (None: the read failed)"""
    return [None if int(l) == FAILED else out[int(o): int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)]


def _reads_of(buf, off, out_n):
    """the reads a decode call left in `buf` -> list of array copies (None: the read failed)"""
    return [None if int(k) == 0xFFFFFFFF else buf[int(o): int(o) + int(k)].copy() for o, k in zip(off, out_n)]


def _cal_pairs(cal, nreads, who):
    """calibrations, (nreads, 2) or flat -> float32[2 * nreads]"""
    cal = np.ascontiguousarray(cal, dtype=np.float32).reshape(-1)
    if cal.size != 2 * nreads:
        raise PressError("%s: two calibration floats per read" % who)
    return cal


# ---------------------------------------------------------------------------- batch API (torch CUDA tensors)

def use_torch_stream():
    """Make the batch calls enqueue on torch's current CUDA stream."""
    import torch

    _call("press_hip_set_device", torch.cuda.current_device())
    _call("press_hip_set_stream", torch.cuda.current_stream().cuda_stream)


def load_table(path=TABLE_PATH):
    _call("press_hip_load_table_file", path.encode())


def press_batch(method, sig, off, n, out, out_off, out_len):
    """Enqueue the compression of a batch.  All arguments are CUDA tensors: sig int16,
    off int64 (nreads read starts, multiples of 8), n int32 (nreads sample counts),
    out uint8, out_off int64 (nreads+1 slot bounds), out_len int64 (nreads; -1 = failed)."""
    _call("press_hip_press_batch", _mid(method), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(), _ptr(out),
          _ptr(out_off), _ptr(out_len), 1)


def press_sizes(method, sig, off, n):
    """Enqueue the sizing of a batch (CUDA tensors as in press_batch) -> int64 CUDA tensor of nreads entries: the
    bytes every read takes under `method` (the range coders: the slot that is certain to hold it), -1 = refused.
    Nothing is compressed."""
    import torch

    need = torch.empty(off.numel(), dtype=torch.int64, device=sig.device)
    _call("press_hip_press_sizes", _mid(method), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(), _ptr(need), 1)
    return need


def press_packed(method, sig, off, n, out, out_off, out_len, align=1):
    """Enqueue the compression of a batch into an arena the library lays out (press_hip_press_packed).  CUDA tensors
    as in press_batch, but out_off (int64, nreads+1) is WRITTEN: read r's stream is out[out_off[r] ..
    out_off[r] + out_len[r]), out_off[-1] is what the batch needs; out.numel() is the arena's capacity - a read
    that does not fit it gets out_len = -1 and is not written."""
    _call("press_hip_press_packed", _mid(method), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(), _ptr(out),
          out.numel(), int(align), _ptr(out_off), _ptr(out_len), 1)


def packed_exact(method):
    """True where press_sizes gives the stream's own length (every method but the range coders)"""
    return bool(load_library().press_hip_packed_exact(_mid(method)))


def depress_batch(method, comp, in_off, in_len, sig, off, n, out_n):
    """Enqueue the decompression of a batch (CUDA tensors; out_n int32, -1 = failed)."""
    _call("press_hip_depress_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(), _ptr(sig),
          _ptr(off), _ptr(n), sig.numel(), _ptr(out_n), 1)


def pa_cal(dor):
    """(nreads, 3) float64 {digitisation, offset, range} as BLOW5 stores them -> (nreads, 2) float32 calibration
    {offset, range / digitisation} for depress_pa_batch (press_hip_pa_cal: host arithmetic, no GPU)"""
    dor = np.ascontiguousarray(dor, dtype=np.float64).reshape(-1, 3)
    cal = np.zeros((dor.shape[0], 2), dtype=np.float32)
    _call("press_hip_pa_cal", _ptr(dor), dor.shape[0], _ptr(cal))
    return cal


def depress_pa_batch(method, comp, in_off, in_len, pa, off, n, cal, out_n):
    """Enqueue the decompression of a batch straight to picoamperes (CUDA tensors as in depress_batch; pa float32 in
    the place of sig, cal float32 of 2 * nreads: pa_cal): pa[off[r] + i] = ((float) s[i] + cal[2r]) * cal[2r + 1]."""
    _call("press_hip_depress_pa_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(), _ptr(pa),
          _ptr(off), _ptr(n), pa.numel(), _ptr(cal), _ptr(out_n), 1)


def depress_pa_fused(method):
    """True where the decode kernel writes the floats itself (press_hip_depress_pa_fused)"""
    return bool(load_library().press_hip_depress_pa_fused(_mid(method)))


def signal_stats(sig, off, n, stats):
    """Enqueue the per-read median and MAD of a batch of samples (CUDA tensors: sig int16, off int64 read starts in
    multiples of 8 samples, n int32 sample counts, stats int32 of 2 * nreads): stats[2r] = the n[r] // 2-th smallest
    sample, stats[2r + 1] = the n[r] // 2-th smallest |sample - median| (press_hip_signal_stats)."""
    _f32_pairs(stats, off.numel(), "stats")
    _call("press_hip_signal_stats", _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(), _ptr(stats), 1)


def norm_cal(stats):
    """(nreads, 2) int32 {median, MAD} -> (nreads, 2) float32 {-median, 1 / (MAD * 1.4826f)} ({., 1} for MAD = 0): the
    calibration with which depress_pa_batch writes the normalised signal (press_hip_norm_cal: host arithmetic, no GPU)"""
    stats = np.ascontiguousarray(stats, dtype=np.int32).reshape(-1, 2)
    cal = np.zeros((stats.shape[0], 2), dtype=np.float32)
    _call("press_hip_norm_cal", _ptr(stats), stats.shape[0], _ptr(cal))
    return cal


def depress_norm_batch(method, comp, in_off, in_len, out, off, n, out_n, stats=None):
    """Enqueue the decompression of a batch straight to the normalised signal (CUDA tensors as in depress_pa_batch, out
    float32 in the place of pa): out[off[r] + i] = (s[i] - median) / (1.4826 * MAD) in signal_stats' and norm_cal's
    arithmetic over the read's decoded samples.  stats: int32 of 2 * nreads that receives {median, MAD}, or None."""
    if stats is not None:
        _f32_pairs(stats, off.numel(), "stats")
    _call("press_hip_depress_norm_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(), _ptr(out),
          _ptr(off), _ptr(n), out.numel(), _ptr(stats), _ptr(out_n), 1)


class ScaleRule(ctypes.Structure):
    """press_hip_scale_rule: the ranks num / den of q_lo and q_hi, and
    shift = max(shift_min, shift_mul * (q_lo + q_hi)), scale = max(scale_min, scale_mul * (q_hi - q_lo))"""
    _fields_ = [("lo_num", ctypes.c_uint32), ("lo_den", ctypes.c_uint32), ("hi_num", ctypes.c_uint32), ("hi_den", ctypes.c_uint32),
                ("shift_mul", ctypes.c_float), ("shift_min", ctypes.c_float), ("scale_mul", ctypes.c_float),
                ("scale_min", ctypes.c_float)]


CHUNK_DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}  # PRESS_HIP_F32 / F16 / BF16


def _ranks(ranks):
    ranks = [(int(a), int(b)) for a, b in ranks]
    return (np.array([a for a, _ in ranks], dtype=np.uint32), np.array([b for _, b in ranks], dtype=np.uint32))


def _rule_ptr(rule):
    if rule is not None and not isinstance(rule, ScaleRule):
        raise PressError("rule must be a press.ScaleRule or None")
    return _ptr(rule)


def signal_quantiles(sig, off, n, ranks, q):
    """Enqueue per-read order statistics of a batch of samples (CUDA tensors as in signal_stats; ranks: 1 .. 4 pairs
    (num, den), host values; q int32 of len(ranks) * nreads): q[nq * r + i] = the min(n - 1, n * num_i // den_i)-th
    smallest sample of read r (press_hip_signal_quantiles)."""
    nreads = off.numel()
    num, den = _ranks(ranks)
    if q.numel() < num.size * nreads or q.element_size() != 4 or not q.is_contiguous():
        raise PressError("q must be a contiguous 32-bit tensor of len(ranks) * nreads entries")
    _call("press_hip_signal_quantiles", _ptr(sig), _ptr(off), _ptr(n), nreads, sig.numel(), _ptr(num), _ptr(den), num.size,
          _ptr(q), 1)


def signal_quantiles_host(reads, ranks):
    """quantiles of a list of int16 arrays (host buffers, synchronous) -> (nreads, len(ranks)) int32"""
    sig, off, ns, total = _host_batch(reads)
    num, den = _ranks(ranks)
    q = np.zeros((len(reads), num.size), dtype=np.int32)
    _call("press_hip_signal_quantiles", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(num), _ptr(den), num.size,
          _ptr(q), 0)
    return q


def scale_cal(q, rule):
    """(nreads, 2) int32 {q_lo, q_hi} and a ScaleRule -> (nreads, 2) float32 {-shift, 1 / scale}: the calibration with
    which depress_pa_batch writes the scaled signal (press_hip_scale_cal: host arithmetic, no GPU)"""
    q = np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 2)
    cal = np.zeros((q.shape[0], 2), dtype=np.float32)
    _call("press_hip_scale_cal", _ptr(q), q.shape[0], _rule_ptr(rule), _ptr(cal))
    return cal


def chunk_plan(ns, T, overlap):
    """the rows of reads of ns samples cut into rows of T that overlap by `overlap` (press_hip_chunk_plan: host
    arithmetic, no GPU) -> (row_first uint64[nreads + 1], row_read uint32[rows], row_start uint32[rows])"""
    ns = np.ascontiguousarray(ns, dtype=np.uint32)
    row_first = np.zeros(ns.size + 1, dtype=np.uint64)
    _call("press_hip_chunk_plan", _ptr(ns), ns.size, int(T), int(overlap), _ptr(row_first), None, None)
    row_read = np.zeros(int(row_first[-1]), dtype=np.uint32)
    row_start = np.zeros(int(row_first[-1]), dtype=np.uint32)
    _call("press_hip_chunk_plan", _ptr(ns), ns.size, int(T), int(overlap), _ptr(row_first), _ptr(row_read), _ptr(row_start))
    return row_first, row_read, row_start


def depress_chunks_batch(method, comp, in_off, in_len, rows, row_first, off, n, total_samples, out_n, overlap, rule=None, q=None):
    """Enqueue the decompression of a batch straight to scaled chunk rows (CUDA tensors as in depress_norm_batch; rows
    [nrows_cap, T] float32, float16 or bfloat16, contiguous; row_first int64 of nreads + 1: chunk_plan over n; off / n /
    total_samples lay out the library's sample scratch).  rule: a ScaleRule (quantile scaling) or None (median / MAD);
    q: int32 of 2 * nreads that receives {q_lo, q_hi} or {median, MAD}, or None."""
    import torch
    nreads = off.numel()
    dt = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}.get(rows.dtype)
    if dt is None or rows.dim() != 2 or not rows.is_contiguous():
        raise PressError("rows must be a contiguous [nrows, T] tensor of float32, float16 or bfloat16")
    if q is not None:
        _f32_pairs(q, nreads, "q")
    if row_first.numel() < nreads + 1 or row_first.element_size() != 8:
        raise PressError("row_first must be a 64-bit tensor of nreads + 1 entries")
    _call("press_hip_depress_chunks_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), nreads, _ptr(rows),
          rows.shape[0], dt, rows.shape[1], int(overlap), _ptr(row_first), _ptr(off), _ptr(n), int(total_samples),
          _rule_ptr(rule), _ptr(q), _ptr(out_n), 1)


def degrade(samples, bits):
    """D_bits of int16 samples (include/press_hip.h, press_hip_degrade_value), a numpy mirror: the nearest multiple of
    2^bits, ties up, saturating at the largest multiple an int16 holds.  bits in 0 .. 8."""
    bits = int(bits)
    if not 0 <= bits <= 8:
        raise PressError("degrade: bits = %d is not in 0 .. 8" % bits)
    s = np.asarray(samples, dtype=np.int16)
    if bits == 0:
        return s.copy()
    v = ((s.astype(np.int32) + (1 << (bits - 1))) >> bits) << bits
    return np.minimum(v, 32768 - (1 << bits)).astype(np.int16)


def degrade_value(s, bits):
    """press_hip_degrade_value: the definition as the library's host arithmetic (no GPU)"""
    return int(load_library().press_hip_degrade_value(int(s), int(bits)))


def degrade_batch(sig, off, n, bits, out=None):
    """Enqueue D_bits over a batch of reads (CUDA tensors as in press_batch); out: an int16 tensor laid out as sig, or
    None: in place.  Only [off[r], off[r] + n[r]) of out is written."""
    out = sig if out is None else out
    _call("press_hip_degrade_batch", _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(), int(bits), _ptr(out), 1)


def degrade_batch_host(reads, bits):
    """D_bits with host buffers: reads = list of int16 arrays -> list of int16 arrays"""
    sig, off, ns, total = _host_batch(reads)
    out = np.zeros(total + 64, dtype=np.int16)
    _call("press_hip_degrade_batch", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, int(bits), _ptr(out), 0)
    return _reads_of(out, off, ns)


def _call_degraded(name, bits, *args):
    """_call of press_hip_<name> for bits == 0 - the existing entry point, untouched - else of its degraded form with
    `bits` behind the leading method ids"""
    if int(bits) == 0:
        return _call("press_hip_" + name, *args)
    deg, at = abi.DEGRADED[name]
    _call("press_hip_" + deg, *args[:at], int(bits), *args[at:])


def _recode_total(who, sig, total_samples):
    if sig is None and total_samples is None:
        raise PressError("%s without sig needs total_samples" % who)
    return sig.numel() if total_samples is None else int(total_samples)


def recode_batch(src, dst, comp, in_off, in_len, n, off, out, out_off, out_len, out_n, sig=None, total_samples=None,
                 degrade_bits=0):
    """Enqueue the recoding of a batch of `src` streams into `dst` streams (CUDA tensors as in depress_batch and
    press_batch).  sig: the int16 tensor that also receives the decoded samples, or None - they then stay in library
    scratch and total_samples (the extent of the layout off / n) must be given.  degrade_bits > 0: the streams hold
    D_bits of the decoded samples, and sig receives those (press_hip_recode_degraded_batch)."""
    total = _recode_total("recode_batch", sig, total_samples)
    _call_degraded("recode_batch", degrade_bits, _mid(src), _mid(dst), _ptr(comp), _ptr(in_off), _ptr(in_len), _ptr(n),
                   _ptr(off), off.numel(), total, _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(sig), _ptr(out_n), 1)


def recode_sizes(src, dst, comp, in_off, in_len, n, off, out_n, sig=None, total_samples=None, degrade_bits=0):
    """Enqueue the sizing of a recode (CUDA tensors as in recode_batch) -> int64 CUDA tensor of nreads entries: the
    bytes every read's `dst` stream takes (as press_sizes), -1 for a read either method refuses.  out_n and - if given -
    sig receive what the decode of `src` gives; no stream is written."""
    import torch

    total = _recode_total("recode_sizes", sig, total_samples)
    need = torch.empty(off.numel(), dtype=torch.int64, device=comp.device)
    _call_degraded("recode_sizes", degrade_bits, _mid(src), _mid(dst), _ptr(comp), _ptr(in_off), _ptr(in_len), _ptr(n),
                   _ptr(off), off.numel(), total, _ptr(need), _ptr(sig), _ptr(out_n), 1)
    return need


def recode_packed(src, dst, comp, in_off, in_len, n, off, out, out_off, out_len, out_n, sig=None, total_samples=None,
                  align=1, degrade_bits=0):
    """Enqueue the recoding of a batch into an arena the library lays out (press_hip_recode_packed).  CUDA tensors as
    in recode_batch, but out_off (int64, nreads+1) is WRITTEN, as by press_packed: out_off[-1] is what the batch needs,
    out.numel() the arena's capacity.  A read whose source stream is refused takes no byte."""
    total = _recode_total("recode_packed", sig, total_samples)
    _call_degraded("recode_packed", degrade_bits, _mid(src), _mid(dst), _ptr(comp), _ptr(in_off), _ptr(in_len), _ptr(n),
                   _ptr(off), off.numel(), total, _ptr(out), out.numel(), int(align), _ptr(out_off), _ptr(out_len),
                   _ptr(sig), _ptr(out_n), 1)


def recode_fused(src, dst):
    """True where the press half's first pass comes out of the decode kernel (press_hip_recode_fused)"""
    return bool(load_library().press_hip_recode_fused(_mid(src), _mid(dst)))


def scratch_fill(byte):
    """test aid: set every scratch buffer of the library but the static-Huffman table, and its page-locked staging
    buffers, to `byte` (press_hip_scratch_fill): a later call's result must not depend on it"""
    _call("press_hip_scratch_fill", int(byte) & 0xFF)


def pass_a_launches():
    """test aid: launches of the exception-split press's first pass over the samples so far in this process"""
    return int(load_library().press_hip_debug_pass_a_launches())


def _packed_arena(need, align):
    """what the streams of `need` bytes (FAILED: none) take, each rounded up to `align` -> (cap, a uint8 arena of cap + 64)"""
    step = np.where(need == np.uint64(FAILED), np.uint64(0), need)
    cap = int(((step + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)).sum())
    return cap, np.zeros(cap + 64, dtype=np.uint8)  # (+ 64: what a later depress_batch may read behind the last stream)


def recode_batch_host(src, dst, streams, ns, caps=None, want_samples=False, degrade_bits=0):
    """Recode with host buffers: streams = list of bytes of method `src`, ns = sample counts / rooms ->
    list of bytes of method `dst` (None: the read failed); with want_samples -> (streams, list of int16 arrays)."""
    nreads = len(streams)
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    if caps is None:
        caps = [int(load_library().press_hip_bound(_mid(dst), int(x))) + 1024 if x else 64 for x in ns]
    out_off = _slots(caps)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    out_len = np.zeros(nreads, dtype=np.uint64)
    out_n = np.zeros(nreads, dtype=np.uint32)
    sig = np.zeros(total + 64, dtype=np.int16) if want_samples else None
    _call_degraded("recode_batch", degrade_bits, _mid(src), _mid(dst), _ptr(comp), _ptr(in_off), _ptr(in_len), _ptr(ns),
                   _ptr(off), nreads, total, _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(sig), _ptr(out_n), 0)
    res = _streams_of(out, out_off, out_len)
    return (res, _reads_of(sig, off, out_n)) if want_samples else res


def recode_packed_host(src, dst, streams, ns, align=1, want_samples=False, degrade_bits=0):
    """Packed recode with host buffers: streams = list of bytes of method `src`, ns = sample counts / rooms ->
    (list of bytes of method `dst` / None, arena bytes); with want_samples -> (streams, arena bytes, list of int16
    arrays).  No capacities: press_hip_recode_sizes gives the arena's size, so it is as large as the streams, not as a
    bound.  As with press_packed_host the convenience costs the front of the chain twice (here the decode too)."""
    nreads = len(streams)
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    need = np.zeros(nreads, dtype=np.uint64)
    out_n = np.zeros(nreads, dtype=np.uint32)
    _call_degraded("recode_sizes", degrade_bits, _mid(src), _mid(dst), _ptr(comp), _ptr(in_off), _ptr(in_len), _ptr(ns),
                   _ptr(off), nreads, total, _ptr(need), None, _ptr(out_n), 0)
    cap, out = _packed_arena(need, align)
    out_off = np.zeros(nreads + 1, dtype=np.uint64)
    out_len = np.zeros(nreads, dtype=np.uint64)
    sig = np.zeros(total + 64, dtype=np.int16) if want_samples else None
    _call_degraded("recode_packed", degrade_bits, _mid(src), _mid(dst), _ptr(comp), _ptr(in_off), _ptr(in_len), _ptr(ns),
                   _ptr(off), nreads, total, _ptr(out), cap, int(align), _ptr(out_off), _ptr(out_len), _ptr(sig),
                   _ptr(out_n), 0)
    res = _streams_of(out, out_off, out_len)
    return (res, int(out_off[-1]), _reads_of(sig, off, out_n)) if want_samples else (res, int(out_off[-1]))


def press_batch_host(method, reads, caps=None):
    """Batch call with host buffers: reads = list of int16 arrays -> list of bytes / None."""
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    if caps is None:
        caps = [int(load_library().press_hip_bound(_mid(method), int(x))) + 1024 for x in ns]
    out_off = _slots(caps)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    out_len = np.zeros(nreads, dtype=np.uint64)
    _call("press_hip_press_batch", _mid(method), _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(out), _ptr(out_off),
          _ptr(out_len), 0)
    return _streams_of(out, out_off, out_len)


def press_packed_host(method, reads, align=1):
    """Packed batch call with host buffers: reads = list of int16 arrays -> (list of bytes / None, arena bytes).
    No capacities are needed: the arena is sized by press_hip_press_sizes (the exact lengths; the range coders'
    slots) and the library lays it out.  The convenience costs two passes: the samples are staged and the front of
    the chain (the svb counting pass, pass A, the zstd inner encode) runs in the sizes call and again in the packed call.
    A caller who minds calls press_hip_press_packed once with a guessed out_cap and again only where out_off[nreads]
    exceeds it."""
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    need = np.zeros(nreads, dtype=np.uint64)
    _call("press_hip_press_sizes", _mid(method), _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(need), 0)
    cap, out = _packed_arena(need, align)
    out_off = np.zeros(nreads + 1, dtype=np.uint64)
    out_len = np.zeros(nreads, dtype=np.uint64)
    _call("press_hip_press_packed", _mid(method), _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(out), cap, int(align),
          _ptr(out_off), _ptr(out_len), 0)
    return _streams_of(out, out_off, out_len), int(out_off[-1])


def depress_batch_host(method, streams, ns):
    """Batch decode with host buffers: streams = list of bytes, ns = sample counts / capacities."""
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    sig = np.zeros(total + 64, dtype=np.int16)
    out_n = np.zeros(len(streams), dtype=np.uint32)
    _call("press_hip_depress_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), len(streams), _ptr(sig),
          _ptr(off), _ptr(ns), total, _ptr(out_n), 0)
    return _reads_of(sig, off, out_n)


def depress_pa_batch_host(method, streams, ns, cals):
    """Batch decode to picoamperes with host buffers: streams = list of bytes, ns = sample counts / capacities,
    cals = (nreads, 2) float32 (pa_cal) -> list of float32 arrays (None: the read failed)."""
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    cal = _cal_pairs(cals, len(streams), "depress_pa_batch_host")
    pa = np.zeros(total + 64, dtype=np.float32)
    out_n = np.zeros(len(streams), dtype=np.uint32)
    _call("press_hip_depress_pa_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), len(streams), _ptr(pa),
          _ptr(off), _ptr(ns), total, _ptr(cal), _ptr(out_n), 0)
    return _reads_of(pa, off, out_n)


def depress_norm_batch_host(method, streams, ns):
    """Batch decode to the normalised signal with host buffers: streams = list of bytes, ns = sample counts /
    capacities -> (list of float32 arrays (None: the read failed), (nreads, 2) int32 {median, MAD})."""
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    out = np.zeros(total + 64, dtype=np.float32)
    out_n = np.zeros(len(streams), dtype=np.uint32)
    stats = np.zeros((len(streams), 2), dtype=np.int32)
    _call("press_hip_depress_norm_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), len(streams), _ptr(out),
          _ptr(off), _ptr(ns), total, _ptr(stats), _ptr(out_n), 0)
    return _reads_of(out, off, out_n), stats


def depress_chunks_batch_host(method, streams, ns, T, overlap, dtype="float16", rule=None):
    """Batch decode to scaled chunk rows with host buffers: streams = list of bytes, ns = sample counts / capacities
    (what Blow5Reader.next_batch gives) -> (rows, q, row_read, row_start, out_n): rows a numpy [nrows, T] array of
    float32 / float16, or of uint16 bit patterns for "bfloat16"; q (nreads, 2) int32 {q_lo, q_hi} (rule: a ScaleRule) or
    {median, MAD} (None); row_read / row_start: per row the read and the sample it starts at (chunk_plan); out_n uint32
    per read, the decoded count or 0xFFFFFFFF for a read that failed - its rows are zeros and its q {0, 0}."""
    nreads = len(streams)
    if dtype not in CHUNK_DTYPES:
        raise PressError("dtype: one of %s" % ", ".join(CHUNK_DTYPES))
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    row_first, row_read, row_start = chunk_plan(ns, T, overlap)
    rows = np.zeros((int(row_first[-1]), int(T)), dtype={"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[dtype])
    out_n = np.zeros(nreads, dtype=np.uint32)
    q = np.zeros((nreads, 2), dtype=np.int32)
    _call("press_hip_depress_chunks_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), nreads, _ptr(rows),
          rows.shape[0], CHUNK_DTYPES[dtype], int(T), int(overlap), _ptr(row_first), _ptr(off), _ptr(ns), total,
          _rule_ptr(rule), _ptr(q), _ptr(out_n), 0)
    return rows, q, row_read, row_start, out_n


def signal_stats_host(reads):
    """{median, MAD} of a list of int16 arrays (host buffers, synchronous) -> (nreads, 2) int32"""
    sig, off, ns, total = _host_batch(reads)
    stats = np.zeros((len(reads), 2), dtype=np.int32)
    _call("press_hip_signal_stats", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(stats), 0)
    return stats





# ---------------------------------------------------------------------------- events: sigtk's segmentation

class EventParams(ctypes.Structure):
    """press_hip_event_params: the two window lengths (2 .. 64), their thresholds and the peak height"""
    _fields_ = [("w1", ctypes.c_uint32), ("w2", ctypes.c_uint32), ("threshold1", ctypes.c_float),
                ("threshold2", ctypes.c_float), ("peak_height", ctypes.c_float)]


EVENT_DTYPE = np.dtype([("start", "<u4"), ("length", "<u4"), ("mean", "<f4"), ("stdv", "<f4")])  # press_hip_event
EVENT_NOFIT = 0xFFFFFFFF  # ev_count of a read whose records did not fit ev_cap


def _preset(family, which, prm):
    """press_hip_<family>_params_preset(which) into the structure prm -> prm"""
    _call("press_hip_%s_params_preset" % family, which, _ptr(prm))
    return prm


def event_params(rna=False):
    """sigtk's detector parameters (press_hip_event_params_preset): DNA 3, 6, 1.4, 9.0, 0.2; RNA 7, 14, 2.5, 9.0, 1.0"""
    return _preset("event", 1 if rna else 0, EventParams())


def _i64_first(t, nreads, name):
    if t.numel() < nreads + 1 or t.element_size() != 8 or not t.is_contiguous():
        raise PressError("%s must be a contiguous 64-bit tensor of nreads + 1 entries" % name)


def _f32_pairs(t, nreads, name, kind="32-bit"):
    if t.numel() < 2 * nreads or t.element_size() != 4 or not t.is_contiguous():
        raise PressError("%s must be a contiguous %s tensor of 2 * nreads entries" % (name, kind))


def _record_cap(rec, words, cap, name):
    """rec: None or a contiguous 32-bit tensor of `words` words per record; cap: None (the rows of rec) or a limit within
    them -> the cap to call with"""
    rows = 0
    if rec is not None:
        if rec.element_size() != 4 or not rec.is_contiguous() or rec.numel() % words:
            raise PressError("%s must be a contiguous 32-bit tensor of %d words per record" % (name, words))
        rows = rec.numel() // words
    cap = rows if cap is None else int(cap)
    if cap > rows:
        raise PressError("%s_cap is beyond %s" % (name, name))
    return cap


def _count_then_records(call, first, cap, dtype):
    """The host forms of the record calls: call(rec, cap) fills `first`; cap None: what the batch needs, found with a pure
    count; then the records -> the min(need, cap) of them that were written"""
    if cap is None:
        call(None, 0)
        cap = int(first[-1])
    rec = np.zeros(int(cap), dtype=dtype)
    call(rec, int(cap))
    return rec[:min(int(first[-1]), int(cap))]


def signal_events(sig, off, n, cal, prm, ev, ev_first, ev_count, ev_cap=None):
    """Enqueue the event detection of a batch of samples (CUDA tensors as in signal_stats; cal float32 of 2 * nreads:
    pa_cal; prm an EventParams; ev: 16-byte records as a 32-bit tensor of [cap, 4] - start, length, mean bits, stdv bits -
    or None for a pure count; ev_first int64 of nreads + 1, WRITTEN; ev_count 32-bit of nreads): read r's events are
    ev[ev_first[r]:ev_first[r + 1]] where they fit ev_cap (default: the rows of ev), else ev_count[r] = 0xFFFFFFFF
    (press_hip_signal_events)."""
    nreads = off.numel()
    _u32_table(ev_count, nreads, "ev_count")
    _i64_first(ev_first, nreads, "ev_first")
    _f32_pairs(cal, nreads, "cal", "float32")
    cap = _record_cap(ev, 4, ev_cap, "ev")
    _call("press_hip_signal_events", _ptr(sig), _ptr(off), _ptr(n), nreads, sig.numel(), _ptr(cal), _ptr(prm),
          _ptr(ev) if cap else None, cap, _ptr(ev_first), _ptr(ev_count), 1)


def signal_events_host(reads, cal, prm=None, ev_cap=None):
    """Events of a list of int16 arrays (host buffers, synchronous); cal (nreads, 2) float32 as pa_cal gives it, prm an
    EventParams (default: the DNA preset), ev_cap a limit in records (default: what the batch needs, found with a pure
    count) -> (ev, ev_first, ev_count): ev an EVENT_DTYPE array of min(need, ev_cap) records, ev_first uint64 of
    nreads + 1, ev_count uint32 per read (0xFFFFFFFF: the read did not fit)."""
    prm = event_params() if prm is None else prm
    sig, off, ns, total = _host_batch(reads)
    cal = _cal_pairs(cal, len(reads), "cal")
    ev_first = np.zeros(len(reads) + 1, dtype=np.uint64)
    ev_count = np.zeros(len(reads), dtype=np.uint32)

    def call(ev, cap):
        _call("press_hip_signal_events", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(cal), _ptr(prm),
              _ptr(ev) if cap else None, cap, _ptr(ev_first), _ptr(ev_count), 0)

    return _count_then_records(call, ev_first, ev_cap, EVENT_DTYPE), ev_first, ev_count


def events_serial_reads():
    """diagnostic: the reads whose sums took the serial path so far (press_hip_events_serial_reads)"""
    return int(load_library().press_hip_events_serial_reads())


def signal_events_workspace_bytes(total_samples, nreads):
    return int(load_library().press_hip_signal_events_workspace_bytes(int(total_samples), int(nreads)))


# ---------------------------------------------------------------------------- segments: sigtk's jnn and jnnv2

class JnnParams(ctypes.Structure):
    """press_hip_jnn_params: jnn_param_t of sigtk (top and bot are used when std_scale is not > 0)"""
    _fields_ = [("std_scale", ctypes.c_float), ("corrector", ctypes.c_int32), ("seg_dist", ctypes.c_int32),
                ("window", ctypes.c_int32), ("stall_len", ctypes.c_float), ("error", ctypes.c_int32),
                ("top", ctypes.c_float), ("bot", ctypes.c_float)]


class Jnn2Params(ctypes.Structure):
    """press_hip_jnn2_params: jnnv2_param_t of sigtk without the stall_len it never reads; window 1 .. 8192"""
    _fields_ = [("std_scale", ctypes.c_float), ("seg_dist", ctypes.c_int32), ("window", ctypes.c_int32),
                ("hi_thresh", ctypes.c_int32), ("lo_thresh", ctypes.c_int32)]


SEGMENT_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4")])  # press_hip_segment
SEGMENT_NOFIT = 0xFFFFFFFF  # seg_count of a read whose records did not fit seg_cap
JNN_KINDS = {"cdna": 0, "drna": 1, "polya": 2}


def jnn_params(kind="cdna"):
    """sigtk's segmenter parameters (press_hip_jnn_params_preset): "cdna", "drna" or "polya" (set top and bot yourself)"""
    if kind not in JNN_KINDS:
        raise PressError("jnn_params: one of %s" % ", ".join(JNN_KINDS))
    return _preset("jnn", JNN_KINDS[kind], JnnParams())


def jnn2_params():
    """sigtk's dRNA adaptor parameters (press_hip_jnn2_params_preset): 0.5, 1500, 2000, 200000, 2000"""
    return _preset("jnn2", 0, Jnn2Params())


def signal_segments(sig, off, n, cal, prm, seg, seg_first, seg_count, thr=None, seg_cap=None):
    """Enqueue the jnn segmentation of a batch of samples (CUDA tensors as in signal_events; cal float32 of 2 * nreads or
    None for the raw domain; prm a JnnParams; seg: 8-byte records as a 32-bit tensor of [cap, 2] - start, end - or None
    for a pure count; seg_first int64 of nreads + 1, WRITTEN; seg_count 32-bit of nreads; thr None or float32 of
    2 * nreads: bot, top per read): read r's segments are seg[seg_first[r]:seg_first[r + 1]] where they fit seg_cap
    (default: the rows of seg), else seg_count[r] = 0xFFFFFFFF (press_hip_signal_segments)."""
    nreads = off.numel()
    _u32_table(seg_count, nreads, "seg_count")
    _i64_first(seg_first, nreads, "seg_first")
    if cal is not None:
        _f32_pairs(cal, nreads, "cal")
    if thr is not None:
        _f32_pairs(thr, nreads, "thr")
    cap = _record_cap(seg, 2, seg_cap, "seg")
    _call("press_hip_signal_segments", _ptr(sig), _ptr(off), _ptr(n), nreads, sig.numel(), _ptr(cal), _ptr(prm),
          _ptr(seg) if cap else None, cap, _ptr(seg_first), _ptr(seg_count), _ptr(thr), 1)


def signal_segments_host(reads, cal=None, prm=None, seg_cap=None, want_thr=True):
    """Segments of a list of int16 arrays (host buffers, synchronous); cal None (raw domain) or (nreads, 2) float32, prm a
    JnnParams (default: the cDNA preset), seg_cap a limit in records (default: what the batch needs, found with a pure
    count) -> (seg, seg_first, seg_count, thr): seg a SEGMENT_DTYPE array of min(need, seg_cap) records, seg_first uint64
    of nreads + 1, seg_count uint32 per read (0xFFFFFFFF: the read did not fit), thr float32 (nreads, 2): bot, top - or
    None without want_thr."""
    prm = jnn_params() if prm is None else prm
    sig, off, ns, total = _host_batch(reads)
    if cal is not None:
        cal = _cal_pairs(cal, len(reads), "cal")
    seg_first = np.zeros(len(reads) + 1, dtype=np.uint64)
    seg_count = np.zeros(len(reads), dtype=np.uint32)
    thr = np.zeros((len(reads), 2), dtype=np.float32) if want_thr else None

    def call(seg, cap):
        _call("press_hip_signal_segments", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(cal), _ptr(prm),
              _ptr(seg) if cap else None, cap, _ptr(seg_first), _ptr(seg_count), _ptr(thr), 0)

    return _count_then_records(call, seg_first, seg_cap, SEGMENT_DTYPE), seg_first, seg_count, thr


def signal_segments_workspace_bytes(total_samples, nreads):
    return int(load_library().press_hip_signal_segments_workspace_bytes(int(total_samples), int(nreads)))


def signal_adaptor(sig, off, n, prm, pair, thr=None):
    """Enqueue sigtk's jnnv2 adaptor finder over a batch of samples (CUDA tensors as in signal_events; prm a Jnn2Params;
    pair int32 of 2 * nreads, WRITTEN: the adaptor's start and end, (0, 0) for none, (-1, -1) for a read of at most
    `window` samples; thr None or float32 of 2 * nreads: bot, mean) (press_hip_signal_adaptor)."""
    nreads = off.numel()
    _f32_pairs(pair, nreads, "pair")
    if thr is not None:
        _f32_pairs(thr, nreads, "thr")
    _call("press_hip_signal_adaptor", _ptr(sig), _ptr(off), _ptr(n), nreads, sig.numel(), _ptr(prm), _ptr(pair), _ptr(thr), 1)


def signal_adaptor_host(reads, prm=None, want_thr=True):
    """jnnv2 over a list of int16 arrays (host buffers, synchronous) -> (pair int32 (nreads, 2), thr float32 (nreads, 2):
    bot, mean - or None without want_thr)"""
    prm = jnn2_params() if prm is None else prm
    sig, off, ns, total = _host_batch(reads)
    pair = np.zeros((len(reads), 2), dtype=np.int32)
    thr = np.zeros((len(reads), 2), dtype=np.float32) if want_thr else None
    _call("press_hip_signal_adaptor", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(prm), _ptr(pair), _ptr(thr), 0)
    return pair, thr


# ---------------------------------------------------------------------------- range statistics and sigtk's stat and prefix

class PrefixParams(ctypes.Structure):
    """press_hip_prefix_params: the adaptor finder's and the poly-A walk's parameters, rna, and the thresholds
    m_a + shift +- half"""
    _fields_ = [("adaptor", Jnn2Params), ("polya", JnnParams), ("rna", ctypes.c_int32), ("shift", ctypes.c_float),
                ("half", ctypes.c_float)]


RANGE_STAT_DTYPE = np.dtype([("mean", "<f4"), ("stdv", "<f4"), ("median", "<f4")])  # press_hip_range_stat
PREFIX_DTYPE = np.dtype([("adapt_start", "<i4"), ("adapt_end", "<i4"), ("polya_start", "<i4"), ("polya_end", "<i4")])  # press_hip_prefix


def prefix_params():
    """sigtk prefix's parameters (press_hip_prefix_params_preset): JNNV2_RNA_ADAPTOR, JNNV1_POLYA, rna 1, 30, 20"""
    return _preset("prefix", 0, PrefixParams())


def _f32_rows(t, rows, words, name):
    if t.numel() < rows * words or t.element_size() != 4 or not t.is_contiguous():
        raise PressError("%s must be a contiguous 32-bit tensor of %d words per record" % (name, words))


def range_stats(sig, off, n, cal, rng, out):
    """Enqueue the mean, deviation and median of a sample range of every read (CUDA tensors as in signal_segments; cal
    float32 of 2 * nreads or None for the raw domain; rng None for whole reads, or 32-bit of 2 * nreads: a, b in samples from
    the read's start, clamped, at any offset; out float32 of [nreads, 3], WRITTEN: mean, stdv, median)
    (press_hip_signal_range_stats)."""
    nreads = off.numel()
    if cal is not None:
        _f32_pairs(cal, nreads, "cal")
    if rng is not None:
        _f32_pairs(rng, nreads, "range")
    _f32_rows(out, nreads, 3, "out")
    _call("press_hip_signal_range_stats", _ptr(sig), _ptr(off), _ptr(n), nreads, sig.numel(), _ptr(cal), _ptr(rng), _ptr(out), 1)


def range_stats_host(reads, cal=None, rng=None):
    """Range statistics of a list of int16 arrays (host buffers, synchronous); cal None (raw domain) or (nreads, 2) float32,
    rng None (whole reads) or (nreads, 2) unsigned: a, b -> a RANGE_STAT_DTYPE array of nreads records"""
    sig, off, ns, total = _host_batch(reads)
    if cal is not None:
        cal = _cal_pairs(cal, len(reads), "cal")
    if rng is not None:
        rng = np.ascontiguousarray(rng, dtype=np.uint32).reshape(-1)
        if rng.size != 2 * len(reads):
            raise PressError("rng: two positions per read")
    out = np.zeros(len(reads), dtype=RANGE_STAT_DTYPE)
    _call("press_hip_signal_range_stats", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(cal), _ptr(rng), _ptr(out), 0)
    return out


def signal_prefix(sig, off, n, cal, prm, out, stat=None, thr=None):
    """Enqueue sigtk's prefix over a batch of samples (CUDA tensors as in signal_segments; cal float32 of 2 * nreads,
    required; prm a PrefixParams; out int32 of [nreads, 4], WRITTEN: adapt_start, adapt_end, polya_start, polya_end; stat
    None or float32 of [2 * nreads, 3]: mean, stdv, median of the adaptor, then of the poly-A tail, in picoamperes; thr None
    or float32 of 2 * nreads: bot, top of the poly-A walk) (press_hip_signal_prefix)."""
    nreads = off.numel()
    _f32_pairs(cal, nreads, "cal")
    _f32_rows(out, nreads, 4, "out")
    if stat is not None:
        _f32_rows(stat, 2 * nreads, 3, "stat")
    if thr is not None:
        _f32_pairs(thr, nreads, "thr")
    _call("press_hip_signal_prefix", _ptr(sig), _ptr(off), _ptr(n), nreads, sig.numel(), _ptr(cal), _ptr(prm), _ptr(out),
          _ptr(stat), _ptr(thr), 1)


def signal_prefix_host(reads, cal, prm=None, want_stat=True, want_thr=True):
    """sigtk's prefix over a list of int16 arrays (host buffers, synchronous); cal (nreads, 2) float32; prm a PrefixParams
    (default: the preset) -> (out PREFIX_DTYPE of nreads, stat RANGE_STAT_DTYPE (nreads, 2): adaptor, poly-A - or None
    without want_stat, thr float32 (nreads, 2): bot, top - or None without want_thr)"""
    prm = prefix_params() if prm is None else prm
    sig, off, ns, total = _host_batch(reads)
    cal = _cal_pairs(cal, len(reads), "cal")
    out = np.zeros(len(reads), dtype=PREFIX_DTYPE)
    stat = np.zeros((len(reads), 2), dtype=RANGE_STAT_DTYPE) if want_stat else None
    thr = np.zeros((len(reads), 2), dtype=np.float32) if want_thr else None
    _call("press_hip_signal_prefix", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(cal), _ptr(prm), _ptr(out),
          _ptr(stat), _ptr(thr), 0)
    return out, stat, thr


def signal_prefix_workspace_bytes(nreads):
    return int(load_library().press_hip_signal_prefix_workspace_bytes(int(nreads)))


def signal_stat_table(sig, off, n, cal):
    """sigtk stat's six columns per read as a float32 CUDA tensor of [nreads, 6]: raw_mean, pa_mean, raw_std, pa_std,
    raw_median, pa_median (CUDA tensors as in range_stats; cal float32 of 2 * nreads).  Two range_stats calls over whole
    reads; only enqueues."""
    import torch

    nreads = off.numel()
    raw = torch.empty((nreads, 3), dtype=torch.float32, device=sig.device)
    pa = torch.empty((nreads, 3), dtype=torch.float32, device=sig.device)
    range_stats(sig, off, n, None, None, raw)
    range_stats(sig, off, n, cal, None, pa)
    return torch.stack((raw, pa), dim=2).reshape(nreads, 6)


# ---------------------------------------------------------------------------- verifying: CRC-32 and compare-after-decode

# ---------------------------------------------------------------------------- the stall methods

def _sid(method):
    return STALL_METHODS[method] if isinstance(method, str) else int(method)


def stall_bound(method, n):
    """X_bound_16(n) of a stall method: rccm_vbbe21_zd's for all three"""
    return int(load_library().press_hip_stall_bound(_sid(method), int(n)))


def stall_workspace_bytes(method, total_samples, nreads):
    return int(load_library().press_hip_stall_workspace_bytes(_sid(method), int(total_samples), int(nreads)))


def _stall_name(method):
    return [k for k, v in STALL_METHODS.items() if v == _sid(method)][0]


def stall_press(method, sig, cap=None):
    """X_press_16 of a stall method through the per-read symbol -> (ret, bytes); ret -1: the library reports *nout = 0"""
    cap = stall_bound(method, np.size(sig)) + 1024 if cap is None else int(cap)
    return _press_16(_stall_name(method) + "_press_16", sig, cap)


def stall_depress(method, comp, n):
    """X_depress_16 of a stall method through the per-read symbol: n is the read's SAMPLE count, which the reference
    passes in the place of the byte count (press.c:7871) -> (ret, int16 array)"""
    return _depress_16(_stall_name(method) + "_depress_16", comp, n, n)


def stall_press_batch(method, sig, off, n, out, out_off, out_len, stall=None):
    """Enqueue the compression of a batch under a stall method.  CUDA tensors as in press_batch; stall: None, or int32
    of 2 * nreads: (stall_start, stall_len) as written into every stream, (0, 0) without a stall"""
    _call("press_hip_stall_press_batch", _sid(method), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(), _ptr(out),
          _ptr(out_off), _ptr(out_len), _ptr(stall), 1)


def stall_depress_batch(comp, in_off, in_len, sig, off, n, out_n):
    """Enqueue the decompression of a batch of stall-method streams (one decoder reads all three).  CUDA tensors as in
    depress_batch; n: the reads' exact sample counts"""
    _call("press_hip_stall_depress_batch", _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(), _ptr(sig), _ptr(off),
          _ptr(n), sig.numel(), _ptr(out_n), 1)


def stall_press_batch_host(method, reads, caps=None, want_stall=False):
    """Host buffers: reads = list of int16 arrays -> list of bytes / None (want_stall: and uint32 [nreads, 2])"""
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    if caps is None:
        caps = [stall_bound(method, int(x)) + 1024 if x else 32 for x in ns]
    out_off = _slots(caps)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    out_len = np.zeros(nreads, dtype=np.uint64)
    stall = np.zeros((nreads, 2), dtype=np.uint32)
    _call("press_hip_stall_press_batch", _sid(method), _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(out),
          _ptr(out_off), _ptr(out_len), _ptr(stall) if want_stall else None, 0)
    streams = _streams_of(out, out_off, out_len)
    return (streams, stall) if want_stall else streams


def stall_depress_batch_host(streams, ns):
    """Host buffers: streams = list of bytes, ns = the reads' sample counts -> list of int16 arrays / None"""
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    sig = np.zeros(total + 64, dtype=np.int16)
    out_n = np.zeros(len(streams), dtype=np.uint32)
    _call("press_hip_stall_depress_batch", _ptr(comp), _ptr(in_off), _ptr(in_len), len(streams), _ptr(sig), _ptr(off),
          _ptr(ns), total, _ptr(out_n), 0)
    return _reads_of(sig, off, out_n)


# ---- the range-coder family: every coder on every layout (press_hip_rcf_*)


def _rcf_ids(coder, layout):
    return (RCF_CODERS[coder] if isinstance(coder, str) else int(coder),
            RCF_LAYOUTS[layout] if isinstance(layout, str) else int(layout))


def rcf_name(coder, layout):
    """the reference's name of a pair: rcf_name("rccdf", "vbe21") == "rccdf_vbe21_zd" """
    c, l = _rcf_ids(coder, layout)
    return "%s_%s_zd" % ([k for k, v in RCF_CODERS.items() if v == c][0], [k for k, v in RCF_LAYOUTS.items() if v == l][0])


def rcf_bound(coder, layout, n):
    """X_bound_16(n) of a pair: the plain layouts' for all sixteen; 0 for an id out of range"""
    c, l = _rcf_ids(coder, layout)
    return int(load_library().press_hip_rcf_bound(c, l, int(n)))


def rcf_press(coder, layout, sig, cap=None):
    """X_press_16 of a pair through the per-read symbol -> (ret, bytes); ret -1: the library reports *nout = 0"""
    cap = rcf_bound(coder, layout, np.size(sig)) + 1024 if cap is None else int(cap)
    return _press_16(rcf_name(coder, layout) + "_press_16", sig, cap)


def rcf_depress(coder, layout, comp, n):
    """X_depress_16 of a pair through the per-read symbol; n: the read's exact sample count -> (ret, int16 array)"""
    return _depress_16(rcf_name(coder, layout) + "_depress_16", comp, len(comp), n)


def rcf_press_batch(coder, layout, sig, off, n, out, out_off, out_len, raw=None):
    """Enqueue the compression of a batch under a pair of the family.  CUDA tensors as in press_batch; raw: None, or
    uint8 of nreads: 1 where the coder gave up and the payload is the read's one-byte values as they are"""
    _call("press_hip_rcf_press_batch", *_rcf_ids(coder, layout), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(),
          _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(raw), 1)


def rcf_depress_batch(coder, layout, comp, in_off, in_len, sig, off, n, out_n):
    """Enqueue the decompression of a batch of streams of a pair.  CUDA tensors as in depress_batch; n: the reads' exact
    sample counts"""
    _call("press_hip_rcf_depress_batch", *_rcf_ids(coder, layout), _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(),
          _ptr(sig), _ptr(off), _ptr(n), sig.numel(), _ptr(out_n), 1)


def rcf_press_batch_host(coder, layout, reads, caps=None, want_raw=False):
    """Host buffers: reads = list of int16 arrays -> list of bytes / None (want_raw: and uint8 [nreads])"""
    c, l = _rcf_ids(coder, layout)
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    if caps is None:
        caps = [rcf_bound(c, l, int(x)) + 1024 if x else 32 for x in ns]
    out_off = _slots(caps)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    out_len = np.zeros(nreads, dtype=np.uint64)
    raw = np.zeros(nreads, dtype=np.uint8)
    _call("press_hip_rcf_press_batch", c, l, _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(out), _ptr(out_off),
          _ptr(out_len), _ptr(raw) if want_raw else None, 0)
    streams = _streams_of(out, out_off, out_len)
    return (streams, raw) if want_raw else streams


def rcf_depress_batch_host(coder, layout, streams, ns):
    """Host buffers: streams = list of bytes, ns = the reads' exact sample counts -> list of int16 arrays / None"""
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    sig = np.zeros(total + 64, dtype=np.int16)
    out_n = np.zeros(len(streams), dtype=np.uint32)
    _call("press_hip_rcf_depress_batch", *_rcf_ids(coder, layout), _ptr(comp), _ptr(in_off), _ptr(in_len), len(streams),
          _ptr(sig), _ptr(off), _ptr(ns), total, _ptr(out_n), 0)
    return _reads_of(sig, off, out_n)


# ---- the Rice family (press_hip_rice_*) and the per-read Huffman family (press_hip_huffman_*) have modules of their own,
# honours_amd/rice.py and honours_amd/huffman.py; their wrappers are reachable here too.  The two ABIs differ in the
# symbols' prefix ("rice", "huffman") and in what the per-read byte means (k, the longest code): the wrappers' bodies are
# these helpers.


def _prefix_layout(layout):
    return RCF_LAYOUTS[layout] if isinstance(layout, str) else int(layout)


def _prefix_name(prefix, layout):
    l = _prefix_layout(layout)
    return "%s_%s_zd" % (prefix, [k for k, v in RCF_LAYOUTS.items() if v == l][0])


def _prefix_bound(prefix, layout, n):
    return int(getattr(load_library(), "press_hip_%s_bound" % prefix)(_prefix_layout(layout), int(n)))


def _prefix_press_batch(prefix, layout, sig, off, n, out, out_off, out_len, byte):
    _call("press_hip_%s_press_batch" % prefix, _prefix_layout(layout), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(),
          _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(byte), 1)


def _prefix_press_sizes(prefix, layout, sig, off, n, need, byte):
    _call("press_hip_%s_press_sizes" % prefix, _prefix_layout(layout), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(),
          _ptr(need), _ptr(byte), 1)


def _prefix_depress_batch(prefix, layout, comp, in_off, in_len, sig, off, n, out_n):
    _call("press_hip_%s_depress_batch" % prefix, _prefix_layout(layout), _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(),
          _ptr(sig), _ptr(off), _ptr(n), sig.numel(), _ptr(out_n), 1)


def _prefix_press_batch_host(prefix, slack, layout, reads, caps, want_byte):
    """slack: what a default slot has beyond the bound"""
    l = _prefix_layout(layout)
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    if caps is None:
        caps = [_prefix_bound(prefix, l, int(x)) + slack if x else 32 for x in ns]
    out_off = _slots(caps)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    out_len = np.zeros(nreads, dtype=np.uint64)
    byte = np.zeros(nreads, dtype=np.uint8)
    _call("press_hip_%s_press_batch" % prefix, l, _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(out), _ptr(out_off),
          _ptr(out_len), _ptr(byte) if want_byte else None, 0)
    streams = _streams_of(out, out_off, out_len)
    return (streams, byte) if want_byte else streams


def _prefix_press_sizes_host(prefix, layout, reads, want_byte):
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    need = np.zeros(nreads, dtype=np.uint64)
    byte = np.zeros(nreads, dtype=np.uint8)
    _call("press_hip_%s_press_sizes" % prefix, _prefix_layout(layout), _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(need),
          _ptr(byte) if want_byte else None, 0)
    return (need, byte) if want_byte else need


def _prefix_depress_batch_host(prefix, layout, streams, ns):
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    sig = np.zeros(total + 64, dtype=np.int16)
    out_n = np.zeros(len(streams), dtype=np.uint32)
    _call("press_hip_%s_depress_batch" % prefix, _prefix_layout(layout), _ptr(comp), _ptr(in_off), _ptr(in_len), len(streams),
          _ptr(sig), _ptr(off), _ptr(ns), total, _ptr(out_n), 0)
    return _reads_of(sig, off, out_n)


def _prefix_repairs(prefix):
    c = np.zeros(3, dtype=np.uint32)
    _call("press_hip_%s_repairs" % prefix, _ptr(c))
    return tuple(int(x) for x in c)


def __getattr__(name):
    """press.rice_name, press.huffman_press_batch, press.xmethod_id, press.smethod_id ...: the functions of honours_amd.rice,
    honours_amd.huffman, honours_amd.xmethod and honours_amd.smethod (PEP 562; a module is imported on first use, it imports
    this one)"""
    if name.split("_")[0] in ("rice", "huffman", "xmethod", "smethod") and "_" in name:
        import importlib
        mod = importlib.import_module("." + name.split("_")[0], __package__)
        if hasattr(mod, name):
            return getattr(mod, name)
    if not name.startswith("_"):  # honours_amd.trim's __all__: the ranged statistics and the trimmed chunk rows (header 2y);
        import importlib          # honours_amd.deflate's: BLOW5 records deflated on the device (header 2z);
        for sub in (".trim", ".deflate", ".inflate"):  # honours_amd.inflate's: ... and inflated there (header 2zb)
            mod = importlib.import_module(sub, __package__)
            if name in mod.__all__:
                return getattr(mod, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


VERIFIED = 0xFFFFFFFF  # PRESS_HIP_VERIFIED: first_bad of a read that decodes to the samples it is meant to hold


def crc32_combine(a, b, len_b):
    """zlib.crc32(A + B) from zlib.crc32(A), zlib.crc32(B) and len(B) in bytes (press_hip_crc32_combine: host
    arithmetic, no GPU)"""
    return int(load_library().press_hip_crc32_combine(int(a) & 0xFFFFFFFF, int(b) & 0xFFFFFFFF, int(len_b)))


def _u32_table(t, nreads, name):
    if t.numel() < nreads or t.element_size() != 4 or not t.is_contiguous():
        raise PressError("%s must be a contiguous 32-bit tensor of nreads entries" % name)


def signal_crc32(sig, off, n, crc):
    """Enqueue the per-read CRC-32 of a batch of samples (CUDA tensors as in signal_stats; crc: 32-bit, nreads entries):
    crc[r] = zlib.crc32 of the n[r] int16 samples at sig[off[r]:] as bytes (press_hip_signal_crc32)."""
    _u32_table(crc, off.numel(), "crc")
    _call("press_hip_signal_crc32", _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(), _ptr(crc), 1)


def signal_crc32_host(reads):
    """CRC-32 of a list of int16 arrays (host buffers, synchronous) -> uint32[nreads]"""
    sig, off, ns, total = _host_batch(reads)
    crc = np.zeros(len(reads), dtype=np.uint32)
    _call("press_hip_signal_crc32", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(crc), 0)
    return crc


def depress_crc_batch(method, comp, in_off, in_len, off, n, total_samples, crc, out_n):
    """Enqueue the decompression of a batch into library scratch and the CRC-32 of what was decoded (CUDA tensors as in
    depress_batch; off / n / total_samples lay out the library's sample scratch; crc: 32-bit, nreads entries, 0 for a
    refused read).  No sample reaches the caller (press_hip_depress_crc_batch)."""
    _u32_table(crc, off.numel(), "crc")
    _call("press_hip_depress_crc_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(), _ptr(off),
          _ptr(n), int(total_samples), _ptr(crc), _ptr(out_n), 1)


def depress_crc_batch_host(method, streams, ns):
    """Decode and digest with host buffers: streams = list of bytes, ns = sample counts / rooms ->
    (crc uint32[nreads], out_n uint32[nreads]; 0 and 0xFFFFFFFF for a refused read)"""
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    crc = np.zeros(len(streams), dtype=np.uint32)
    out_n = np.zeros(len(streams), dtype=np.uint32)
    _call("press_hip_depress_crc_batch", _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), len(streams), _ptr(off),
          _ptr(ns), total, _ptr(crc), _ptr(out_n), 0)
    return crc, out_n


def verify_batch(method, comp, in_off, in_len, sig, off, n, first_bad, out_n, nbad, degrade_bits=0):
    """Enqueue decode-and-compare of a batch (CUDA tensors: the streams as in depress_batch; sig / off / n the samples
    they are meant to hold, laid out as press_batch takes them; first_bad, out_n: 32-bit, nreads entries; nbad: one
    32-bit word).  first_bad[r] = VERIFIED, or the first sample that differs (0: the stream is refused; min(out_n, n)
    where only the counts differ); nbad = the reads that are not VERIFIED (press_hip_verify_batch).  degrade_bits > 0:
    sig holds the originals of a degraded archive and the comparison is with D_bits of them
    (press_hip_verify_degraded_batch)."""
    _u32_table(first_bad, off.numel(), "first_bad")
    _u32_table(nbad, 1, "nbad")
    _call_degraded("verify_batch", degrade_bits, _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(),
                   _ptr(sig), _ptr(off), _ptr(n), sig.numel(), _ptr(first_bad), _ptr(out_n), _ptr(nbad), 1)


def verify_batch_host(method, streams, reads, degrade_bits=0):
    """Decode and compare with host buffers: streams = list of bytes, reads = the int16 arrays they are meant to hold
    -> (first_bad uint32[nreads], out_n uint32[nreads], nbad)"""
    nreads = len(streams)
    if len(reads) != nreads:
        raise PressError("verify_batch_host: one stream per read")
    comp, in_off, in_len = _streams_arena(streams)
    sig, off, ns, total = _host_batch(reads)
    first_bad = np.zeros(nreads, dtype=np.uint32)
    out_n = np.zeros(nreads, dtype=np.uint32)
    nbad = ctypes.c_uint32(0)
    _call_degraded("verify_batch", degrade_bits, _mid(method), _ptr(comp), _ptr(in_off), _ptr(in_len), nreads, _ptr(sig),
                   _ptr(off), _ptr(ns), total, _ptr(first_bad), _ptr(out_n), ctypes.byref(nbad), 0)
    return first_bad, out_n, int(nbad.value)


class HostBatch:
    """A batch in HOST memory laid out once, so that press() / depress() are nothing but the C calls
    (press_hip_press_batch / press_hip_depress_batch with device_resident = 0): what a C caller that
    keeps its reads in its own buffers pays - H2D, kernels, D2H - and what bench.py's PCIe-inclusive
    figure times.  pinned=True takes the buffers from press_hip_host_alloc (page-locked memory:
    the library then copies by DMA straight from / to them)."""

    def __init__(self, method, reads, pinned=False):
        lib = load_library()
        self.lib, self.mid, self.nreads = lib, _mid(method), len(reads)
        self.pinned = pinned
        self._held = []
        def zeroed(count, dtype):  # (page-locked memory comes as it is)
            a = self._alloc(count, dtype)
            a[:] = 0
            return a

        self.sig, self.off, self.ns, self.total = _host_batch(reads, zeroed)
        self.out_off = _slots([int(lib.press_hip_bound(self.mid, int(x))) + 1024 for x in self.ns])
        self.out = self._alloc(int(self.out_off[-1]) + 64, np.uint8)
        self.out_len = np.zeros(self.nreads, dtype=np.uint64)
        self.back = self._alloc(self.total + 64, np.int16)
        self.out_n = np.zeros(self.nreads, dtype=np.uint32)
        # the arguments of the two calls, resolved once: press() and depress() are one call into the library each
        self._in_off = np.ascontiguousarray(self.out_off[:-1])
        self._press = (self.mid, _ptr(self.sig), _ptr(self.off), _ptr(self.ns), self.nreads, self.total, _ptr(self.out),
                       _ptr(self.out_off), _ptr(self.out_len), 0)
        self._depress = (self.mid, _ptr(self.out), _ptr(self._in_off), _ptr(self.out_len), self.nreads, _ptr(self.back),
                         _ptr(self.off), _ptr(self.ns), self.total, _ptr(self.out_n), 0)

    def _alloc(self, count, dtype):
        nbytes = int(count) * np.dtype(dtype).itemsize
        if not self.pinned:
            return np.zeros(count, dtype=dtype)
        p = self.lib.press_hip_host_alloc(nbytes)
        if not p:  # (returns the pointer, not a status: not a case for _call)
            raise PressError(last_error())
        self._held.append(p)
        buf = (ctypes.c_uint8 * nbytes).from_address(p)
        return np.frombuffer(buf, dtype=dtype)

    def press(self):
        _call("press_hip_press_batch", *self._press)

    def streams(self):
        return _streams_of(self.out, self.out_off, self.out_len)

    def depress(self):
        """decode the streams press() left in the slots of `out` into `back`"""
        _call("press_hip_depress_batch", *self._depress)

    def lossless(self):
        return bool(np.array_equal(self.out_n, self.ns)) and all(
            np.array_equal(self.back[int(o): int(o) + int(k)], self.sig[int(o): int(o) + int(k)])
            for o, k in zip(self.off, self.ns))

    def close(self):
        self.sig = self.out = self.back = None
        for p in self._held:
            self.lib.press_hip_host_free(p)
        self._held = []





def kernel_timing(enable=True):
    """(re)start / stop the HIP-event timing of the dominant kernel of each batch call"""
    _call("press_hip_kernel_timing", 1 if enable else 0)


def kernel_times(which):
    """elapsed ms of the dominant kernel of every press (which=0) / depress (1) call so far"""
    buf = (ctypes.c_float * 128)()
    n = load_library().press_hip_kernel_times(which, buf, 128)
    return [buf[i] for i in range(n)]


# ---------------------------------------------------------------------------- fitting a Huffman table

NBINS = 257  # the 256 one-byte zd values the shuffman_* methods code, then the exceptions


def _rows(lib, *names):
    """(re)apply the table's rows of `names` to a library handle"""
    return abi.declare(lib, {n: abi.PROTOS[n] for n in names})


def _train_api(lib):
    """load_library() has declared these; kept because tests/test_table_training.py calls it before the raw functions"""
    _rows(lib, "press_hip_symbol_counts", "press_hip_table_from_counts", "press_hip_write_table_file")


def _tally_api(lib):
    """as _train_api, for tests/test_signal_tally.py"""
    _rows(lib, "press_hip_signal_tally", "press_hip_signal_tally_workspace_bytes")


def symbol_counts(sig, off, n, counts):
    """Enqueue the counting of a batch on the device, ADDING into counts (CUDA tensors: sig int16, off int64
    read starts in multiples of 8 samples, n int32 sample counts, counts int64 of NBINS entries holding
    uint64 values)."""
    if counts.numel() != NBINS or counts.element_size() != 8 or not counts.is_contiguous():
        raise PressError("counts must be a contiguous 64-bit tensor of %d entries" % NBINS)
    _call("press_hip_symbol_counts", _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(), _ptr(counts), 1)


def symbol_counts_host(reads, counts=None):
    """Counts of a list of int16 arrays (host buffers, synchronous) -> numpy uint64[NBINS]; added to
    `counts` when it is given."""
    sig, off, ns, total = _host_batch(reads)
    out = np.zeros(NBINS, dtype=np.uint64) if counts is None else np.ascontiguousarray(counts, dtype=np.uint64).copy()
    _call("press_hip_symbol_counts", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(out), 0)
    return out


def table_from_counts(counts, max_bits=24):
    """The reference's Huffman construction over counts[0..255] (a longer counts array: the rest is ignored),
    limited to max_bits -> (len uint32[256], bits uint64[256]); bit k of bits[s] is the k-th emitted bit."""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.uint64)[:256])
    if c.size != 256:
        raise PressError("table_from_counts needs 256 counts")
    ln = np.zeros(256, dtype=np.uint32)
    bits = np.zeros(256, dtype=np.uint64)
    _call("press_hip_table_from_counts", _ptr(c), int(max_bits), _ptr(ln), _ptr(bits))
    return ln, bits


def write_table(path, ln, bits, data_bytes):
    """The table file (the format of NA12878_zd.huffman) that use_table() / press_hip_load_table_file read."""
    ln = np.ascontiguousarray(ln, dtype=np.uint32)
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    _call("press_hip_write_table_file", path.encode(), _ptr(ln), _ptr(bits), int(data_bytes) & 0xFFFFFFFF)





def _blow5_counts(path, counts, max_reads=4096, arena_bytes=1 << 28, degrade_bits=0):
    """Counts of every read of a BLOW5 file, into the device tensor `counts`: the signal fields go to the device
    as stored (svb-zd: decoded there by the slow5_svb_zd depress); the samples stay on the device.  degrade_bits > 0:
    the samples are degraded in place there before they are counted."""
    import torch

    dev = counts.device
    rd = Blow5Reader(path)
    try:
        arena = np.empty(arena_bytes, dtype=np.uint8)
        boff = np.zeros(max_reads, dtype=np.uint64)
        blen = np.zeros(max_reads, dtype=np.uint64)
        bns = np.zeros(max_reads, dtype=np.uint32)
        while True:
            got = rd.next_arena(arena, boff, blen, bns, max_reads)
            if got == 0:
                break
            ns = bns[:got].copy()
            off, total = _layout(ns)
            d_off = torch.from_numpy(off.view(np.int64)).to(dev)
            d_n = torch.from_numpy(ns.view(np.int32)).to(dev)
            end = int(boff[got - 1] + blen[got - 1])
            d_sig = torch.zeros(total + 64, dtype=torch.int16, device=dev)
            if rd.signal_method == 1:
                d_in = torch.from_numpy(arena[:end + 64].copy()).to(dev)
                d_in_off = torch.from_numpy(boff[:got].view(np.int64).copy()).to(dev)
                d_in_len = torch.from_numpy(blen[:got].view(np.int64).copy()).to(dev)
                d_out_n = torch.zeros(got, dtype=torch.int32, device=dev)
                depress_batch("slow5_svb_zd", d_in, d_in_off, d_in_len, d_sig, d_off, d_n, d_out_n)
                if degrade_bits:
                    degrade_batch(d_sig, d_off, d_n, degrade_bits)
                symbol_counts(d_sig, d_off, d_n, counts)
                if not torch.equal(d_out_n, d_n):
                    raise PressError("a signal of %s does not decode" % path)
            elif rd.signal_method == 0:  # int16 samples as stored
                sig = np.zeros(total + 64, dtype=np.int16)
                for k in range(got):
                    sig[int(off[k]):int(off[k]) + int(ns[k])] = arena[int(boff[k]):int(boff[k] + blen[k])].view(np.int16)
                d_sig.copy_(torch.from_numpy(sig))
                if degrade_bits:
                    degrade_batch(d_sig, d_off, d_n, degrade_bits)
                symbol_counts(d_sig, d_off, d_n, counts)
            else:
                raise PressError("%s: signal method %d" % (path, rd.signal_method))
    finally:
        rd.close()


def train_table(src, path, max_bits=24, degrade_bits=0):
    """Fit a static-Huffman table to `src` (a list of int16 arrays, or the path of a BLOW5 file) and write it to
    `path` for use_table() / press_hip_load_table_file / the reference's read_code_table.  -> the counts
    (numpy uint64[NBINS]; counts[256] = the exceptions, which the table does not code).  degrade_bits > 0: the table
    is fitted to D_bits of the reads (degraded on the device, then counted) - the table for a degraded archive."""
    degrade_bits = int(degrade_bits)
    if not 0 <= degrade_bits <= 8:
        raise PressError("train_table: degrade_bits = %d is not in 0 .. 8" % degrade_bits)
    if isinstance(src, (str, os.PathLike)):
        import torch

        use_torch_stream()
        counts = torch.zeros(NBINS, dtype=torch.int64, device="cuda")
        _blow5_counts(os.fspath(src), counts, degrade_bits=degrade_bits)
        counts = counts.cpu().numpy().view(np.uint64)
    else:
        counts = symbol_counts_host(degrade_batch_host(src, degrade_bits) if degrade_bits else src)
    ln, bits = table_from_counts(counts, max_bits)
    write_table(path, ln, bits, int(counts[:256].sum()))
    return counts


# ---------------------------------------------------------------------------- dataset analysis: tallies and moments

TALLY_BINS = 65536   # counters of raw and of delta, indexed by zz(v) = (v << 1) ^ (v >> 15) as uint16
TALLY_SYMS = NBINS   # trans is TALLY_SYMS x TALLY_SYMS: the 256 one-byte symbols, then the exceptions as one class
# include/press_hip.h press_hip_moments
MOMENTS_DTYPE = np.dtype([("sum", "<i8"), ("sumsq", "<u8"), ("min", "<i4"), ("max", "<i4"), ("n", "<u4"), ("nex", "<u4")])
TALLY_OUTPUTS = ("raw", "delta", "trans", "mom")


def signal_tally_workspace_bytes(total_samples, nreads):
    return int(load_library().press_hip_signal_tally_workspace_bytes(int(total_samples), int(nreads)))


def signal_tally(sig, off, n, raw=None, delta=None, trans=None, mom=None):
    """Enqueue press_hip_signal_tally on the device (CUDA tensors: sig int16, off int64 read starts in multiples of 8
    samples, n int32 sample counts).  raw and delta (64-bit, TALLY_BINS entries) and trans (64-bit, TALLY_SYMS squared)
    are ADDED to; mom (32 bytes per read: a contiguous tensor of nreads * 4 64-bit or nreads * 8 32-bit words, read with
    MOMENTS_DTYPE) is set.  Any may be None."""
    nreads = off.numel()
    for name, t, words in (("raw", raw, TALLY_BINS), ("delta", delta, TALLY_BINS), ("trans", trans, TALLY_SYMS * TALLY_SYMS)):
        if t is not None and (t.numel() != words or t.element_size() != 8 or not t.is_contiguous()):
            raise PressError("%s must be a contiguous 64-bit tensor of %d entries" % (name, words))
    if mom is not None and (mom.numel() * mom.element_size() != 32 * nreads or not mom.is_contiguous()):
        raise PressError("mom must be a contiguous tensor of 32 bytes per read")
    _call("press_hip_signal_tally", _ptr(sig), _ptr(off), _ptr(n), nreads, sig.numel(), _ptr(raw), _ptr(delta), _ptr(trans),
          _ptr(mom), 1)


def signal_tally_host(reads, want=TALLY_OUTPUTS, into=None):
    """Tallies of a list of int16 arrays (host buffers, synchronous) -> dict with the members of `want`: raw, delta
    (numpy uint64[TALLY_BINS]), trans (uint64[TALLY_SYMS, TALLY_SYMS]), mom (MOMENTS_DTYPE[nreads]).  into: a dict of
    tables the counts are added to (copies are returned)."""
    sig, off, ns, total = _host_batch(reads)
    shapes = {"raw": (TALLY_BINS,), "delta": (TALLY_BINS,), "trans": (TALLY_SYMS, TALLY_SYMS)}
    out = {}
    for k in want:
        if k == "mom":
            out[k] = np.zeros(len(reads), dtype=MOMENTS_DTYPE)
        elif into is not None and k in into:
            out[k] = np.ascontiguousarray(into[k], dtype=np.uint64).reshape(shapes[k]).copy()
        else:
            out[k] = np.zeros(shapes[k], dtype=np.uint64)
    _call("press_hip_signal_tally", _ptr(sig), _ptr(off), _ptr(ns), len(reads), total, _ptr(out.get("raw")),
          _ptr(out.get("delta")), _ptr(out.get("trans")), _ptr(out.get("mom")), 0)
    return out





def tally_value(index):
    """the int16 value of a counter index of raw / delta: the inverse of zz"""
    index = np.asarray(index, dtype=np.int64)
    return (index >> 1) ^ -(index & 1)


def tally_table(counts):
    """raw or delta counters -> (values ascending, counts) with the zero rows dropped: the rows printtally prints"""
    c = np.asarray(counts, dtype=np.uint64).reshape(-1)
    values = tally_value(np.arange(c.size))
    order = np.argsort(values, kind="stable")
    values, c = values[order], c[order]
    keep = c != 0
    return values[keep], c[keep]


def tally_text(counts):
    """the text viz/freq_slow5 and viz/freq_delta_slow5 print for these counters (tally.c printtally)"""
    v, c = tally_table(counts)
    return "signal\tfreq\n" + "".join("%d\t%d\n" % (int(a), int(b)) for a, b in zip(v, c))


def _entropy_bits(counts, total):
    """- sum p log2 p of integer counts with sum `total`, term by term (no cancellation: a peaked table keeps its digits);
    for p above one half, log2 p = log1p(-(total - c) / total) / ln 2"""
    import math

    def term(c):
        if 2 * c > total:
            return -(c / total) * math.log1p(-((total - c) / total)) / math.log(2.0)
        return -(c / total) * (math.log2(c) - math.log2(total))
    return math.fsum(term(c) for c in counts if c) if total else 0.0


def tally_summary(counts):
    """The eleven numbers of viz/freq_analyse.R over a raw or delta table -> dict of n, min, q1, mean, median, q3, max, mode,
    var (population), std, entropy (bits per value).  Integers and fractions, rounded once to float; a quantile is the
    first value in ascending order whose cumulative count reaches n * q; the mode is the smallest value among ties.  An
    empty table: n = 0 and None for the rest."""
    from fractions import Fraction
    v, c = tally_table(counts)
    v, c = [int(x) for x in v], [int(x) for x in c]
    n = sum(c)
    if n == 0:
        return dict(n=0, min=None, q1=None, mean=None, median=None, q3=None, max=None, mode=None, var=None, std=None, entropy=None)

    def quantile(num, den):
        cum = 0
        for val, cnt in zip(v, c):
            cum += cnt
            if cum * den >= n * num:
                return val
        return v[-1]

    s1 = sum(a * b for a, b in zip(v, c))
    s2 = sum(a * a * b for a, b in zip(v, c))
    var = Fraction(n * s2 - s1 * s1, n * n)
    top = max(c)
    return dict(n=n, min=v[0], q1=quantile(1, 4), mean=float(Fraction(s1, n)), median=quantile(1, 2), q3=quantile(3, 4),
                max=v[-1], mode=v[c.index(top)], var=float(var), std=_sqrt_fraction(var), entropy=_entropy_bits(c, n))


def _sqrt_fraction(q):
    """sqrt of a non-negative Fraction p / q as a float: isqrt(p q 4^64) / (q 2^64), an integer root of at least 64 bits
    (relative error below 2^-63), rounded once"""
    import math
    from fractions import Fraction
    if q <= 0:
        return 0.0
    return float(Fraction(math.isqrt((q.numerator * q.denominator) << 128), q.denominator << 64))


def transition_entropy(trans):
    """(H0, H1) in bits of a transition table: H0 the order-0 entropy of the symbol the transitions arrive at (column
    sums), H1 = H(sym[i] | sym[i-1]) = H(pairs) - H(row sums).  (0, 0) for an empty table."""
    t = np.asarray(trans, dtype=np.uint64).reshape(TALLY_SYMS, TALLY_SYMS)
    cells = [int(x) for x in t.reshape(-1) if x]
    n = sum(cells)
    if n == 0:
        return 0.0, 0.0
    rows = [int(x) for x in t.sum(axis=1, dtype=object)]
    cols = [int(x) for x in t.sum(axis=0, dtype=object)]
    return _entropy_bits(cols, n), max(0.0, _entropy_bits(cells, n) - _entropy_bits(rows, n))


def moments_stats(mom, dor=None):
    """Per read, from the exact integers of MOMENTS_DTYPE records -> dict of float64 arrays mean, var (population) and sd
    (NaN for an empty read): var = (n * sumsq - sum^2) / n^2 as a rational, rounded once.  dor: [nreads, 3] digitisation,
    offset, range -> also min_pa, max_pa, mean_pa = (x + offset) * (range / dig), var_pa = var * (range / dig)^2 and sd_pa
    (viz/stats.c)."""
    import math
    from fractions import Fraction
    mom = np.asarray(mom, dtype=MOMENTS_DTYPE).reshape(-1)
    out = {k: np.full(mom.size, np.nan) for k in ("mean", "var", "sd")}
    for r, m in enumerate(mom):
        n, s1, s2 = int(m["n"]), int(m["sum"]), int(m["sumsq"])
        if n == 0:
            continue
        var = Fraction(n * s2 - s1 * s1, n * n)
        out["mean"][r] = float(Fraction(s1, n))
        out["var"][r] = float(var)
        out["sd"][r] = _sqrt_fraction(var)
    if dor is not None:
        dor = np.asarray(dor, dtype=np.float64).reshape(-1, 3)
        with np.errstate(all="ignore"):
            scale = dor[:, 2] / dor[:, 0]
            out["min_pa"] = (mom["min"] + dor[:, 1]) * scale
            out["max_pa"] = (mom["max"] + dor[:, 1]) * scale
            out["mean_pa"] = (out["mean"] + dor[:, 1]) * scale
            out["var_pa"] = out["var"] * scale ** 2
            out["sd_pa"] = np.sqrt(out["var_pa"])
    return out


def _report_batches(src, max_reads, arena_bytes, dev, inflate="host"):
    """the reads of a BLOW5 file or of a list of int16 arrays as device batches -> (d_sig, d_off, d_n, ids, dor rows)"""
    import torch

    if not isinstance(src, (str, os.PathLike)):
        for k0 in range(0, len(src), max_reads):
            part = src[k0:k0 + max_reads]
            sig, off, ns, _ = _host_batch(part)
            yield (torch.from_numpy(sig).to(dev), torch.from_numpy(off.view(np.int64)).to(dev),
                   torch.from_numpy(ns.view(np.int32)).to(dev), ["read-%08d" % (k0 + k) for k in range(len(part))], None)
        return
    path = os.fspath(src)
    rd = Blow5Reader(path)
    try:
        while inflate == "device" and rd.record_method == 1 and rd.signal_method == 1:
            # zlib records of svb-zd fields: inflated, parsed and decoded on the device; no field exists on the host
            b = rd.next_batch_device(max_reads, arena_bytes, dev)
            if b is None:
                return
            ns = b["n_samples"].cpu().numpy().view(np.uint32)
            off, total = _layout(ns)
            d_off = torch.from_numpy(off.view(np.int64)).to(dev)
            d_sig = torch.zeros(total + 64, dtype=torch.int16, device=dev)
            d_out_n = torch.zeros(ns.size, dtype=torch.int32, device=dev)
            depress_batch("slow5_svb_zd", b["rec"], b["sig_off"], b["sig_len"], d_sig, d_off, b["n_samples"], d_out_n)
            if not torch.equal(d_out_n, b["n_samples"]):
                raise PressError("a signal of %s does not decode" % path)
            yield d_sig, d_off, b["n_samples"], b["ids"], b["dor"].cpu().numpy()
        arena = np.empty(arena_bytes, dtype=np.uint8)
        boff = np.zeros(max_reads, dtype=np.uint64)
        blen = np.zeros(max_reads, dtype=np.uint64)
        bns = np.zeros(max_reads, dtype=np.uint32)
        dor = np.zeros((max_reads, 3), dtype=np.float64)
        idbuf = ctypes.create_string_buffer(max_reads * rd.ID_LEN)
        got = ctypes.c_uint32()
        while True:
            _blow5_call("press_hip_blow5_next_pa", rd._h, max_reads, _ptr(arena), arena.size, _ptr(boff), _ptr(blen), _ptr(bns),
                        idbuf, _ptr(dor), ctypes.byref(got))
            g = got.value
            if g == 0:
                break
            ids = [idbuf.raw[k * rd.ID_LEN:(k + 1) * rd.ID_LEN].split(b"\0")[0].decode() for k in range(g)]
            ns = bns[:g].copy()
            off, total = _layout(ns)
            d_off = torch.from_numpy(off.view(np.int64)).to(dev)
            d_n = torch.from_numpy(ns.view(np.int32)).to(dev)
            if rd.signal_method == 1:  # svb-zd fields: decoded on the device, the samples stay there
                end = int(boff[g - 1] + blen[g - 1])
                d_sig = torch.zeros(total + 64, dtype=torch.int16, device=dev)
                d_in = torch.from_numpy(arena[:end + 64].copy()).to(dev)
                d_in_off = torch.from_numpy(boff[:g].view(np.int64).copy()).to(dev)
                d_in_len = torch.from_numpy(blen[:g].view(np.int64).copy()).to(dev)
                d_out_n = torch.zeros(g, dtype=torch.int32, device=dev)
                depress_batch("slow5_svb_zd", d_in, d_in_off, d_in_len, d_sig, d_off, d_n, d_out_n)
                if not torch.equal(d_out_n, d_n):
                    raise PressError("a signal of %s does not decode" % path)
            elif rd.signal_method == 0:  # int16 samples as stored
                sig = np.zeros(total + 64, dtype=np.int16)
                for k in range(g):
                    sig[int(off[k]):int(off[k]) + int(ns[k])] = arena[int(boff[k]):int(boff[k] + blen[k])].view(np.int16)
                d_sig = torch.from_numpy(sig).to(dev)
            else:
                raise PressError("%s: signal method %d" % (path, rd.signal_method))
            yield d_sig, d_off, d_n, ids, dor[:g].copy()
    finally:
        rd.close()


def dataset_report(src, max_reads=4096, arena_bytes=1 << 28, inflate="host"):
    """What the data looks like, tallied on the device: src is the path of a BLOW5 file or a list of int16 arrays.  The
    reads go through in batches (svb-zd signal fields are decoded on the device), one press_hip_signal_tally per batch
    with all four outputs; only the tables and the moments come back.  -> dict:
      raw, delta, trans      the tables (numpy uint64)
      raw_summary, delta_summary, symbol_summary   tally_summary of raw, of delta, and of the symbol stream (trans' column
                             sums as a table over 0 .. 256)
      h0, h1                 transition_entropy(trans)
      bits                   {"raw", "delta", "symbols", "symbols_order1"}: entropy in bits per sample
      ratio                  16 / bits for each of them (inf where the entropy is 0)
      mom, ids, dor, stats   the per-read moments, the read ids, [nreads, 3] digitisation / offset / range (None for a list
                             of arrays) and moments_stats(mom, dor)
      reads, samples         counts
    inflate="device": a file with record method zlib and signal method svb-zd is inflated on the device too
    (Blow5Reader.next_batch_device), so that no field of a batch exists on the host; record methods none and zstd, and
    files of int16 samples, keep the host path."""
    import torch

    _inflate_mode(inflate)
    use_torch_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    raw = torch.zeros(TALLY_BINS, dtype=torch.int64, device=dev)
    delta = torch.zeros(TALLY_BINS, dtype=torch.int64, device=dev)
    trans = torch.zeros(TALLY_SYMS * TALLY_SYMS, dtype=torch.int64, device=dev)
    moms, ids, dors = [], [], []
    for d_sig, d_off, d_n, batch_ids, dor in _report_batches(src, max_reads, arena_bytes, dev, inflate):
        mom = torch.zeros(4 * d_off.numel(), dtype=torch.int64, device=dev)
        signal_tally(d_sig, d_off, d_n, raw, delta, trans, mom)
        moms.append(mom.cpu().numpy().view(MOMENTS_DTYPE))
        ids += batch_ids
        dors.append(dor)
    rep = {"raw": raw.cpu().numpy().view(np.uint64), "delta": delta.cpu().numpy().view(np.uint64),
           "trans": trans.cpu().numpy().view(np.uint64).reshape(TALLY_SYMS, TALLY_SYMS)}
    rep["mom"] = np.concatenate(moms) if moms else np.zeros(0, dtype=MOMENTS_DTYPE)
    rep["ids"] = ids
    rep["dor"] = np.concatenate(dors) if dors and dors[0] is not None else None
    rep["stats"] = moments_stats(rep["mom"], rep["dor"])
    rep["reads"] = len(ids)
    rep["samples"] = int(rep["mom"]["n"].astype(np.uint64).sum())
    rep["raw_summary"] = tally_summary(rep["raw"])
    rep["delta_summary"] = tally_summary(rep["delta"])
    cols = rep["trans"].sum(axis=0)
    sym = np.zeros(TALLY_BINS, dtype=np.uint64)  # symbol k as the value k: counter index zz(k) = 2 k
    sym[2 * np.arange(TALLY_SYMS)] = cols
    rep["symbol_summary"] = tally_summary(sym)
    rep["h0"], rep["h1"] = transition_entropy(rep["trans"])
    rep["bits"] = {"raw": rep["raw_summary"]["entropy"] or 0.0, "delta": rep["delta_summary"]["entropy"] or 0.0,
                   "symbols": rep["h0"], "symbols_order1": rep["h1"]}
    rep["ratio"] = {k: (16.0 / b if b > 0 else float("inf")) for k, b in rep["bits"].items()}
    return rep


# ---------------------------------------------------------------------------- BLOW5 input (host side)

def _blow5_call(name, *args):
    """as _call, for the press_hip_blow5_* functions: they report through press_hip_blow5_last_error"""
    lib = load_library()
    if getattr(lib, name)(*args):
        raise PressError(lib.press_hip_blow5_last_error().decode())


class Blow5Reader:
    """press_hip_blow5_*: iterate over a BLOW5 file's signal fields as stored (svb-zd streams for
    signal method 1) - what depress_batch_host("slow5_svb_zd", ...) / the device batch API decode."""

    ID_LEN = 64

    def __init__(self, path):
        self._h = ctypes.c_void_p()
        _blow5_call("press_hip_blow5_open", path.encode(), ctypes.byref(self._h))
        rm, sm = ctypes.c_int(), ctypes.c_int()
        load_library().press_hip_blow5_methods(self._h, ctypes.byref(rm), ctypes.byref(sm))
        self.record_method, self.signal_method = rm.value, sm.value

    def next_batch(self, max_reads=4096, arena_bytes=1 << 28):
        """-> list of (read_id, n_samples, signal field bytes); empty at the end of the file"""
        arena = np.empty(arena_bytes, dtype=np.uint8)
        off = np.zeros(max_reads, dtype=np.uint64)
        ln = np.zeros(max_reads, dtype=np.uint64)
        ns = np.zeros(max_reads, dtype=np.uint32)
        ids = ctypes.create_string_buffer(max_reads * self.ID_LEN)
        got = ctypes.c_uint32()
        _blow5_call("press_hip_blow5_next", self._h, max_reads, _ptr(arena), arena_bytes, _ptr(off), _ptr(ln), _ptr(ns), ids,
                    ctypes.byref(got))
        out = []
        for k in range(got.value):
            rid = ids.raw[k * self.ID_LEN:(k + 1) * self.ID_LEN].split(b"\0")[0].decode()
            out.append((rid, int(ns[k]), arena[int(off[k]):int(off[k]) + int(ln[k])].tobytes()))
        return out

    def next_batch_pa(self, max_reads=4096, arena_bytes=1 << 28):
        """-> list of (read_id, n_samples, signal field bytes, (digitisation, offset, range)); empty at the end of the
        file.  The three doubles as the record stores them: pa_cal makes depress_pa_batch's calibration of them."""
        arena = np.empty(arena_bytes, dtype=np.uint8)
        off = np.zeros(max_reads, dtype=np.uint64)
        ln = np.zeros(max_reads, dtype=np.uint64)
        ns = np.zeros(max_reads, dtype=np.uint32)
        dor = np.zeros((max_reads, 3), dtype=np.float64)
        ids = ctypes.create_string_buffer(max_reads * self.ID_LEN)
        got = ctypes.c_uint32()
        _blow5_call("press_hip_blow5_next_pa", self._h, max_reads, _ptr(arena), arena_bytes, _ptr(off), _ptr(ln), _ptr(ns), ids,
                    _ptr(dor), ctypes.byref(got))
        out = []
        for k in range(got.value):
            rid = ids.raw[k * self.ID_LEN:(k + 1) * self.ID_LEN].split(b"\0")[0].decode()
            out.append((rid, int(ns[k]), arena[int(off[k]):int(off[k]) + int(ln[k])].tobytes(),
                        (float(dor[k, 0]), float(dor[k, 1]), float(dor[k, 2]))))
        return out

    def next_stored(self, max_reads=4096, arena_bytes=1 << 28, arena=None):
        """press_hip_blow5_next_stored: the next records AS THE FILE STORES THEM, with no inflate (record method zlib: the
        zlib streams blow5_inflate_batch reads) -> (arena uint8, comp_off uint64, comp_len uint64), the tables `got`
        long: 0 at the end of the file.  Every record starts on a 16-byte boundary.  arena: a numpy uint8 array to fill
        (e.g. page-locked memory) in the place of a new one.  No GPU is needed.  One kind of call per reader: records
        the inflating calls have read ahead are not handed out again."""
        if arena is None:
            arena = np.empty(arena_bytes, dtype=np.uint8)
        off = np.zeros(max_reads, dtype=np.uint64)
        ln = np.zeros(max_reads, dtype=np.uint64)
        got = ctypes.c_uint32()
        _blow5_call("press_hip_blow5_next_stored", self._h, max_reads, _ptr(arena), arena.size, _ptr(off), _ptr(ln), ctypes.byref(got))
        return arena, off[:got.value], ln[:got.value]

    def next_batch_device(self, max_reads=4096, arena_bytes=1 << 28, device="cuda"):
        """The next records of a file with record method zlib, inflated and parsed ON THE DEVICE: the stored records go up
        as they are (next_stored), blow5_inflate_batch inflates them - a first round with slots of 4 * comp_len + 4096
        bytes, the host reader's own first guess, and a second one with the exact length for the records that answer
        ROOM - and blow5_record_fields finds the fields.  -> dict of CUDA tensors rec (uint8: the record arena), rec_off /
        rec_len (int64: the records in it), sig_off
        / sig_len (int64: depress_batch's in_off / in_len over rec), n_samples (int32), dor (float64 (n, 3)), and ids, a
        list of str on the host; None at the end of the file.  A record with any other failure status raises PressError
        with the status name."""
        import importlib

        import torch

        if self.record_method != 1:
            raise PressError("next_batch_device inflates zlib records: this file's record method is %d" % self.record_method)
        ifl = importlib.import_module(".inflate", __package__)
        if getattr(self, "_stored_arena", None) is None or self._stored_arena.size < arena_bytes:
            self._stored_arena = np.empty(arena_bytes, dtype=np.uint8)  # kept: one allocation per reader, not per batch
        arena, off, ln = self.next_stored(max_reads, arena=self._stored_arena[:arena_bytes])
        n = off.size
        if n == 0:
            return None
        used = int(off[-1] + ln[-1])
        comp = torch.from_numpy(arena[:used]).to(device)
        d_off = torch.from_numpy(off.view(np.int64)).to(device)
        d_ln = torch.from_numpy(ln.view(np.int64)).to(device)
        slots = _slots(4 * ln + 4096)
        out_off = torch.from_numpy(slots.view(np.int64)).to(device)
        # the second round's records go behind the first round's slots: a spare eighth is there for them, so that the
        # arena is not copied (only a batch whose ROOM records need more gets a larger arena)
        first = int(slots[-1])
        rec = torch.empty(first + max(first // 8, 1 << 20), dtype=torch.uint8, device=device)
        out_len = torch.empty(n, dtype=torch.int64, device=device)
        status = torch.empty(n, dtype=torch.uint8, device=device)
        ifl.blow5_inflate_batch(comp, d_off, d_ln, rec, out_off, out_len, status)
        st = status.cpu().numpy()
        rec_off = out_off[:n]
        again = np.flatnonzero(st == ifl.INFLATE_STATUS.index("ROOM"))
        if again.size:  # the second round: exact slots behind the first round's
            idx = torch.from_numpy(again).to(device)
            need = out_len[idx].cpu().numpy().astype(np.uint64)
            slots2 = _slots(need) + np.uint64(first)
            if int(slots2[-1]) > rec.numel():
                rec = torch.cat([rec[:first], torch.empty(int(slots2[-1]) - first, dtype=torch.uint8, device=device)])
            len2 = torch.empty(again.size, dtype=torch.int64, device=device)
            st2 = torch.empty(again.size, dtype=torch.uint8, device=device)
            ifl.blow5_inflate_batch(comp, d_off[idx].contiguous(), d_ln[idx].contiguous(), rec,
                                    torch.from_numpy(slots2.view(np.int64)).to(device), len2, st2)
            rec_off = rec_off.clone()
            rec_off[idx] = torch.from_numpy(slots2[:-1].view(np.int64).copy()).to(device)
            out_len[idx] = len2
            st[again] = st2.cpu().numpy()
        if st.any():
            k = int(np.flatnonzero(st)[0])
            raise PressError("next_batch_device: record %d does not inflate: %s" % (k, ifl.INFLATE_STATUS[st[k]]))
        sig_off, sig_len, ns, dor, ids = ifl.blow5_record_fields(rec, rec_off, out_len, self.signal_method)
        if bool((sig_len < 0).any()):
            raise PressError("next_batch_device: record %d is not a BLOW5 record" % int(torch.nonzero(sig_len < 0)[0]))
        names = [bytes(r).split(b"\0")[0].decode() for r in ids.cpu().numpy()]
        return {"rec": rec, "rec_off": rec_off, "rec_len": out_len, "sig_off": sig_off, "sig_len": sig_len, "n_samples": ns, "dor": dor,
                "ids": names}

    def set_threads(self, n):
        """host threads that inflate records (0: as many as the host offers, at most 32)"""
        _blow5_call("press_hip_blow5_threads", self._h, int(n))

    def next_arena(self, arena, off, ln, ns, max_reads):
        """the raw call: signal fields into the caller's arena (numpy uint8; page-locked memory from
        press.host_alloc for a fast copy to the device), offsets / lengths / sample counts into off / ln / ns
        (numpy uint64, uint64, uint32 of >= max_reads).  -> reads delivered (0 at the end of the file)"""
        got = ctypes.c_uint32()
        _blow5_call("press_hip_blow5_next", self._h, max_reads, _ptr(arena), arena.size, _ptr(off), _ptr(ln), _ptr(ns), None,
                    ctypes.byref(got))
        return got.value

    def close(self):
        if self._h:
            load_library().press_hip_blow5_close(self._h)
            self._h = ctypes.c_void_p()


def _blow5_write_batch(w, pres, sigs, posts):
    """press_hip_blow5_write_batch over lists of numpy uint8 arrays (posts may hold empty arrays)"""
    n = len(pres)
    PT = ctypes.c_void_p * n
    LT = ctypes.c_uint64 * n
    pre_p, sig_p, post_p = PT(), PT(), PT()
    pre_l, sig_l, post_l = LT(), LT(), LT()
    for k in range(n):
        pre_p[k], pre_l[k] = pres[k].ctypes.data, pres[k].size
        sig_p[k], sig_l[k] = (sigs[k].ctypes.data if sigs[k].size else None), sigs[k].size
        post_p[k], post_l[k] = (posts[k].ctypes.data if posts[k].size else None), posts[k].size
    _blow5_call("press_hip_blow5_write_batch", w, n, pre_p, pre_l, sig_p, sig_l, post_p, post_l)


# ---------------------------------------------------------------------------- BLOW5 records deflated on the device
# (the calls themselves: honours_amd.deflate, whose names are attributes of this module too - __getattr__ above)

def _deflate():
    import importlib
    return importlib.import_module(".deflate", __package__)


def _blow5_write_image(w, image, rec_off, pres):
    """press_hip_blow5_write_image: image and rec_off as numpy arrays, pres the records' front parts"""
    n = len(pres)
    pre_p, pre_l = (ctypes.c_void_p * n)(), (ctypes.c_uint64 * n)()
    for k in range(n):
        pre_p[k], pre_l[k] = pres[k].ctypes.data, pres[k].size
    rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    _blow5_call("press_hip_blow5_write_image", w, _ptr(image), int(rec_off[n]), n, _ptr(rec_off), pre_p, pre_l)


def _blow5_fields_deflated(src_signal_method, fields, ns, pres, posts, degrade_bits, who):
    """One batch of a transcode with deflate="device": the source's signal fields (svb-zd streams, or int16 samples as
    bytes) become svb-zd fields in a device arena - recoded, or pressed - and the deflate call reads them there; only the
    image comes back.  -> (image, rec_off) as numpy arrays"""
    import torch

    n = len(fields)
    dev = torch.device("cuda")

    def up(a, view=None):
        return torch.from_numpy(a if view is None else a.view(view)).to(dev)
    ns = np.asarray(ns, dtype=np.uint32)
    bound = sum(int(load_library().press_hip_bound(METHODS["slow5_svb_zd"], int(x))) for x in ns)
    arena = torch.empty((bound + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev)
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    if src_signal_method == 1:
        comp, in_off, in_len, ns, off, total = _decode_batch(fields, ns)
        out_n = torch.empty(n, dtype=torch.int32, device=dev)
        recode_packed("slow5_svb_zd", "slow5_svb_zd", up(comp), up(in_off, np.int64), up(in_len, np.int64), up(ns, np.int32),
                      up(off, np.int64), arena, out_off, out_len, out_n, total_samples=total, degrade_bits=degrade_bits)
    else:
        sig, off, ns, total = _host_batch([np.frombuffer(f, dtype=np.int16) for f in fields])
        d_sig, d_off, d_n = up(sig), up(off, np.int64), up(ns, np.int32)
        if degrade_bits:
            degrade_batch(d_sig, d_off, d_n, degrade_bits)
        press_packed("slow5_svb_zd", d_sig, d_off, d_n, arena, out_off, out_len)
    dfl = _deflate()
    side, tab = dfl.side_arena(pres, posts)
    record_bytes = side.size + 8 * n + bound
    image = torch.empty(dfl.blow5_deflate_image_cap(record_bytes, n), dtype=torch.uint8, device=dev)
    rec_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    raw = torch.empty(n, dtype=torch.uint8, device=dev)
    d_side, d_tab = up(side if side.size else np.zeros(4, dtype=np.uint8)), up(tab.reshape(-1), np.int64)
    torch.cuda.current_stream().synchronize()  # (the library may enqueue on a stream of its own)
    dfl.blow5_deflate_batch(d_side, d_tab, arena, out_off[:n], out_len, record_bytes, image, rec_off, raw)
    _call("press_hip_synchronize")
    raw = raw.cpu().numpy()
    if np.any(raw == dfl.DEFLATE_REFUSED):
        raise PressError("%s: the signal of record %d does not press or recode" % (who, int(np.flatnonzero(raw == dfl.DEFLATE_REFUSED)[0])))
    rec_off = rec_off.cpu().numpy().view(np.uint64)
    return image[:int(rec_off[n])].cpu().numpy(), rec_off


def _blow5_batch_deflated(batch, src_signal_method, degrade_bits, who):
    """One batch of a transcode with inflate="device" and deflate="device": what Blow5Reader.next_batch_device made - the
    inflated records in a device arena and their fields - is recoded (svb-zd fields) or pressed (int16 samples) into
    svb-zd fields in another device arena, and the deflate call takes the records' front parts and auxiliary fields out
    of the record arena itself; only the front parts (for the index) and the image come back.
    -> (image, rec_off, pres) as numpy arrays"""
    import torch

    rec, ro, rl, so, sl, d_n = (batch[k] for k in ("rec", "rec_off", "rec_len", "sig_off", "sig_len", "n_samples"))
    n = ro.numel()
    dev = rec.device
    ns = d_n.cpu().numpy().view(np.uint32)
    off, total = _layout(ns)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    bound = sum(int(load_library().press_hip_bound(METHODS["slow5_svb_zd"], int(x))) for x in ns)
    arena = torch.empty((bound + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev)
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    if src_signal_method == 1:
        out_n = torch.empty(n, dtype=torch.int32, device=dev)
        recode_packed("slow5_svb_zd", "slow5_svb_zd", rec, so, sl, d_n, d_off, arena, out_off, out_len, out_n, total_samples=total,
                      degrade_bits=degrade_bits)
    else:  # int16 samples at any byte offset of the record arena: gathered into an aligned sample arena on the device
        d_sig = torch.zeros(total + 64, dtype=torch.int16, device=dev)
        h_so = so.cpu().numpy()
        for k in range(n):
            d_sig[int(off[k]):int(off[k]) + int(ns[k])] = rec[int(h_so[k]):int(h_so[k]) + 2 * int(ns[k])].clone().view(torch.int16)
        if degrade_bits:
            degrade_batch(d_sig, d_off, d_n, degrade_bits)
        press_packed("slow5_svb_zd", d_sig, d_off, d_n, arena, out_off, out_len)
    pre_len = so - 8 - ro
    post_off = so + sl
    d_tab = torch.stack([ro, pre_len, post_off, ro + rl - post_off], dim=1).contiguous().reshape(-1)
    width = int(pre_len.max())
    idx = (ro[:, None] + torch.arange(width, device=dev)[None, :]).clamp_(max=rec.numel() - 1)
    h_pre, h_len = rec[idx].cpu().numpy(), pre_len.cpu().numpy()
    pres = [np.ascontiguousarray(h_pre[k, :int(h_len[k])]) for k in range(n)]
    dfl = _deflate()
    record_bytes = int(rl.sum()) - int(sl.sum()) + bound
    image = torch.empty(dfl.blow5_deflate_image_cap(record_bytes, n), dtype=torch.uint8, device=dev)
    rec_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    raw = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.current_stream().synchronize()  # (the library may enqueue on a stream of its own)
    dfl.blow5_deflate_batch(rec, d_tab, arena, out_off[:n], out_len, record_bytes, image, rec_off, raw)
    _call("press_hip_synchronize")
    raw = raw.cpu().numpy()
    if np.any(raw == dfl.DEFLATE_REFUSED):
        raise PressError("%s: the signal of record %d does not press or recode" % (who, int(np.flatnonzero(raw == dfl.DEFLATE_REFUSED)[0])))
    rec_off = rec_off.cpu().numpy().view(np.uint64)
    return image[:int(rec_off[n])].cpu().numpy(), rec_off, pres


def _inflate_mode(inflate):
    if inflate not in ("host", "device"):
        raise PressError('inflate = %r: "host" or "device"' % (inflate,))
    return inflate == "device"


def _deflate_mode(deflate, record_method):
    if deflate not in ("host", "device"):
        raise PressError('deflate = %r: "host" or "device"' % (deflate,))
    if deflate == "device" and record_method != 1:
        raise PressError('deflate="device" makes zlib streams: it needs record_method 1')
    return deflate == "device"


def blow5_write_like(dst, like, fields, record_method=1, signal_method=1, index=False, ids=None, deflate="host"):
    """A BLOW5 file with the header of `like` and one record per entry of `fields` (signal fields in the given
    signal method: svb-zd streams or int16 samples as bytes); every record takes the fixed fields and auxiliary
    fields of `like`'s first record and a read id of its own (ids, default "read-%08d" padded to the template's
    length).  For benchmarks and tests: a file of any size with realistic framing.  deflate="device": the records'
    zlib streams are made on the device (blow5_deflate_batch_host) instead of by zlib on host threads.  -> the read ids"""
    on_device = _deflate_mode(deflate, record_method)
    lib = load_library()
    rd = Blow5Reader(like)
    cap = 1 << 26
    arena = np.empty(cap, dtype=np.uint8)
    ro, rl, sp, sl = (np.zeros(1, dtype=np.uint64) for _ in range(4))
    ns = np.zeros(1, dtype=np.uint32)
    got = ctypes.c_uint32()
    if lib.press_hip_blow5_next_records(rd._h, 1, _ptr(arena), cap, _ptr(ro), _ptr(rl), _ptr(sp), _ptr(sl), _ptr(ns),
                                        ctypes.byref(got)) or got.value != 1:
        rd.close()
        raise PressError("no template record in " + like)
    rec = arena[int(ro[0]):int(ro[0]) + int(rl[0])].copy()
    idl = int(rec[0]) | (int(rec[1]) << 8)
    fixed = rec[2 + idl:int(sp[0]) - 8].copy()          # read group, digitisation ... sampling rate
    post = rec[int(sp[0]) + int(sl[0]):].copy()         # auxiliary fields
    w = ctypes.c_void_p()
    try:
        _blow5_call("press_hip_blow5_create", dst.encode(), rd._h, record_method, signal_method, ctypes.byref(w))
    finally:
        rd.close()
    out_ids = []
    try:
        if index:
            lib.press_hip_blow5_index(w, 1)
        B = 512
        for k0 in range(0, len(fields), B):
            pres, sigs, posts = [], [], []
            for k in range(k0, min(k0 + B, len(fields))):
                rid = (ids[k] if ids else "read-%08d" % k).encode()
                out_ids.append(rid.decode())
                pres.append(np.frombuffer(bytes([len(rid) & 255, len(rid) >> 8]) + rid + fixed.tobytes(), dtype=np.uint8))
                f = fields[k]
                sigs.append(f if isinstance(f, np.ndarray) else np.frombuffer(f, dtype=np.uint8))
                posts.append(post)
            if on_device:
                image, rec_off, _ = _deflate().blow5_deflate_batch_host(pres, sigs, posts, signal_method)
                _blow5_write_image(w, image, rec_off, pres)
            else:
                _blow5_write_batch(w, pres, sigs, posts)
    finally:
        _blow5_call("press_hip_blow5_finish", w)
    return out_ids


def blow5_transcode(src, dst, record_method=1, signal_method=1, codec=None, passthrough=False, index=False, verify=False,
                    degrade_bits=0, deflate="host", inflate="host"):
    """BLOW5 -> BLOW5 with the signal fields re-coded: codec(list of int16 arrays) -> list of svb-zd
    streams (default: the device, press_batch_host("slow5_svb_zd")); signal_method 0 writes the raw
    samples.  Signals of the source are decoded on the device when it stores them as svb-zd.
    passthrough: keep the signal fields as they are (source and target signal method must agree;
    no GPU involved - only the record framing / record compression changes).
    index: also write slow5lib's <dst>.idx (the reference's slow5_get then works on the transcoded file).
    verify: before a batch is written, its outgoing svb-zd fields are decoded on the device and compared with the
    samples they were made of (verify_batch_host); a field that does not give them back raises PressError with the
    read's id and the first bad sample, and nothing more is written.  Nothing to check with passthrough or
    signal_method 0, which writes the samples themselves.
    degrade_bits > 0: a lossy archive - the signals written decode to D_bits of the source's samples (degrade()); the
    file is still plain BLOW5.  A source that stores svb-zd is decoded, degraded and pressed in one device call
    (recode_batch_host) unless a codec is given; verify then compares the fields with D_bits of the source's samples
    on the device (verify_batch_host(..., degrade_bits)).  Not with passthrough.
    deflate="device" (record_method 1): the records' zlib streams are made on the device and a batch goes to the file as
    one image (press_hip_blow5_write_image).  With signal_method 1, no codec, no verify and no passthrough the fields stay
    on the device between the recode or press call and the deflate call, and only the image comes back; otherwise the
    fields made as above are deflated through blow5_deflate_batch_host.
    inflate="device": a source with record method zlib is inflated and parsed on the device
    (Blow5Reader.next_batch_device).  Together with the conditions under which deflate="device" keeps the fields on the
    device, no field of a batch exists on the host: the records go up as stored and come back as the image.  In every
    other combination the inflated records are copied to the host and go on as above.  Sources with record method none or
    zstd keep the host path whatever `inflate` says.
    Returns the number of reads written."""
    on_device = _deflate_mode(deflate, record_method)
    inflate_device = _inflate_mode(inflate)
    degrade_bits = int(degrade_bits)
    if not 0 <= degrade_bits <= 8:
        raise PressError("blow5_transcode: degrade_bits = %d is not in 0 .. 8" % degrade_bits)
    if passthrough and degrade_bits:
        raise PressError("passthrough keeps the signal fields as they are: it cannot degrade them")
    lib = load_library()
    rd = Blow5Reader(src)
    w = ctypes.c_void_p()
    try:
        _blow5_call("press_hip_blow5_create", dst.encode(), rd._h, record_method, signal_method, ctypes.byref(w))
    except PressError:
        rd.close()
        raise
    total = 0
    try:
        if index:
            lib.press_hip_blow5_index(w, 1)
        maxr, cap = 1024, 1 << 28
        arena = np.empty(cap, dtype=np.uint8)
        ro, rl, sp, sl = (np.zeros(maxr, dtype=np.uint64) for _ in range(4))
        ns = np.zeros(maxr, dtype=np.uint32)
        got = ctypes.c_uint32()
        inflate_device = inflate_device and rd.record_method == 1
        while True:
            if inflate_device:
                batch = rd.next_batch_device(maxr, cap)
                if batch is None:
                    break
                got.value = len(batch["ids"])
                if on_device and signal_method == 1 and codec is None and not passthrough and not verify:
                    image, rec_off, pres = _blow5_batch_deflated(batch, rd.signal_method, degrade_bits, src)
                    _blow5_write_image(w, image, rec_off, pres)
                    total += got.value
                    continue
                arena = batch["rec"].cpu().numpy()  # the other combinations work on the host from here on
                ro[:got.value], rl[:got.value] = batch["rec_off"].cpu().numpy(), batch["rec_len"].cpu().numpy()
                sp[:got.value] = (batch["sig_off"] - batch["rec_off"]).cpu().numpy()
                sl[:got.value], ns[:got.value] = batch["sig_len"].cpu().numpy(), batch["n_samples"].cpu().numpy().view(np.uint32)
            else:
                _blow5_call("press_hip_blow5_next_records", rd._h, maxr, _ptr(arena), cap, _ptr(ro), _ptr(rl), _ptr(sp), _ptr(sl),
                            _ptr(ns), ctypes.byref(got))
            if got.value == 0:
                break
            recs = [arena[int(ro[k]):int(ro[k]) + int(rl[k])] for k in range(got.value)]
            fields = [r[int(sp[k]):int(sp[k]) + int(sl[k])].tobytes() for k, r in enumerate(recs)]
            pres = [r[:int(sp[k]) - 8] for k, r in enumerate(recs)]
            posts = [r[int(sp[k]) + int(sl[k]):] for k, r in enumerate(recs)]
            if on_device and signal_method == 1 and codec is None and not passthrough and not verify:
                image, rec_off = _blow5_fields_deflated(rd.signal_method, fields, ns[:got.value], pres, posts, degrade_bits, src)
                _blow5_write_image(w, image, rec_off, pres)
                total += got.value
                continue
            if passthrough:
                if rd.signal_method != signal_method:
                    raise PressError("passthrough needs the same signal method on both sides")
                out = fields
                sigs = None
            elif rd.signal_method == 1:
                sigs = depress_batch_host("slow5_svb_zd", fields, [int(x) for x in ns[:got.value]])
                if any(s is None for s in sigs):
                    raise PressError("a signal of %s does not decode" % src)
            else:
                sigs = [np.frombuffer(f, dtype=np.int16) for f in fields]
            if passthrough:
                pass
            elif signal_method == 1:
                if degrade_bits and codec is None and rd.signal_method == 1:
                    out = recode_batch_host("slow5_svb_zd", "slow5_svb_zd", fields, [int(x) for x in ns[:got.value]],
                                            degrade_bits=degrade_bits)
                    if any(o is None for o in out):
                        raise PressError("a signal of %s does not recode" % src)
                else:
                    out = (codec or (lambda reads: press_batch_host("slow5_svb_zd", reads)))(
                        degrade_batch_host(sigs, degrade_bits) if degrade_bits else sigs)
                if verify:
                    first_bad, _, nbad = verify_batch_host("slow5_svb_zd", out, sigs, degrade_bits=degrade_bits)
                    if nbad:
                        k = int(np.flatnonzero(first_bad != VERIFIED)[0])
                        idl = int(recs[k][0]) | (int(recs[k][1]) << 8)
                        raise PressError("read %s: the svb-zd field written for it does not decode to its samples (first bad sample %d)"
                                         % (recs[k][2:2 + idl].tobytes().split(b"\0")[0].decode(errors="replace"), int(first_bad[k])))
            else:
                out = [np.ascontiguousarray(s, dtype=np.int16).tobytes()
                       for s in (degrade_batch_host(sigs, degrade_bits) if degrade_bits else sigs)]
            outs = [np.frombuffer(out[k], dtype=np.uint8) for k in range(got.value)]
            if on_device:
                image, rec_off, _ = _deflate().blow5_deflate_batch_host(pres, outs, posts, signal_method)
                _blow5_write_image(w, image, rec_off, pres)
            else:
                _blow5_write_batch(w, pres, outs, posts)
            total += got.value
    finally:
        rd.close()
        _blow5_call("press_hip_blow5_finish", w)
    return total
