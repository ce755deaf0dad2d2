"""Trimmed chunk rows (include/press_hip.h section 2y): per-read statistics over a sample range, and compressed reads
straight to scaled chunk rows that start behind a range's start - the caller's, the jnnv2 adaptor's end or the end of the
first jnn record - with the row plan made on the device.  Every function and name here is also an attribute of
honours_amd.press (press.trim_adaptor, press.depress_chunks_trimmed_batch ...).
"""
import ctypes

import numpy as np

from . import press as _p

# what honours_amd.press hands out as its own attributes (press.__getattr__ reads this list)
__all__ = ["signal_stats_ranged", "signal_stats_ranged_host", "signal_quantiles_ranged", "signal_quantiles_ranged_host", "Trim",
           "TRIM_RANGE", "TRIM_ADAPTOR", "TRIM_SEGMENT", "trim_range", "trim_adaptor", "trim_segment", "clamp_ranges",
           "chunk_plan_ranged", "depress_chunks_trimmed_workspace_bytes", "depress_chunks_trimmed_batch",
           "depress_chunks_trimmed_batch_host"]


def _range_pairs(ranges, nreads):
    """None, or (nreads, 2) uint32 {a, b} for the host forms"""
    if ranges is None:
        return None
    ranges = np.ascontiguousarray(ranges, dtype=np.uint32).reshape(-1, 2)
    if ranges.shape[0] != nreads:
        raise _p.PressError("ranges: one pair (a, b) per read")
    return ranges


def signal_stats_ranged(sig, off, n, rng, stats):
    """signal_stats over the samples [a', b') of each read alone (rng: a 32-bit CUDA tensor of 2 * nreads words a, b,
    clamped as range_stats clamps them, or None for whole reads) (press_hip_signal_stats_ranged)."""
    nreads = off.numel()
    _p._f32_pairs(stats, nreads, "stats")
    if rng is not None:
        _p._f32_pairs(rng, nreads, "rng")
    _p._call("press_hip_signal_stats_ranged", _p._ptr(sig), _p._ptr(off), _p._ptr(n), nreads, sig.numel(), _p._ptr(rng), _p._ptr(stats), 1)


def signal_stats_ranged_host(reads, ranges=None):
    """{median, MAD} of reads[r][a':b'] for a list of int16 arrays and (nreads, 2) ranges (host buffers, synchronous)
    -> (nreads, 2) int32"""
    sig, off, ns, total = _p._host_batch(reads)
    rng = _range_pairs(ranges, len(reads))
    stats = np.zeros((len(reads), 2), dtype=np.int32)
    _p._call("press_hip_signal_stats_ranged", _p._ptr(sig), _p._ptr(off), _p._ptr(ns), len(reads), total, _p._ptr(rng), _p._ptr(stats), 0)
    return stats


def signal_quantiles_ranged(sig, off, n, rng, ranks, q):
    """signal_quantiles over the samples [a', b') of each read alone (rng as in signal_stats_ranged): with L = b' - a',
    q[nq * r + i] = the min(L - 1, L * num_i // den_i)-th smallest of them, 0 for L == 0
    (press_hip_signal_quantiles_ranged)."""
    nreads = off.numel()
    num, den = _p._ranks(ranks)
    if q.numel() < num.size * nreads or q.element_size() != 4 or not q.is_contiguous():
        raise _p.PressError("q must be a contiguous 32-bit tensor of len(ranks) * nreads entries")
    if rng is not None:
        _p._f32_pairs(rng, nreads, "rng")
    _p._call("press_hip_signal_quantiles_ranged", _p._ptr(sig), _p._ptr(off), _p._ptr(n), nreads, sig.numel(), _p._ptr(rng), _p._ptr(num),
          _p._ptr(den), num.size, _p._ptr(q), 1)


def signal_quantiles_ranged_host(reads, ranks, ranges=None):
    """quantiles of reads[r][a':b'] (host buffers, synchronous) -> (nreads, len(ranks)) int32"""
    sig, off, ns, total = _p._host_batch(reads)
    rng = _range_pairs(ranges, len(reads))
    num, den = _p._ranks(ranks)
    q = np.zeros((len(reads), num.size), dtype=np.int32)
    _p._call("press_hip_signal_quantiles_ranged", _p._ptr(sig), _p._ptr(off), _p._ptr(ns), len(reads), total, _p._ptr(rng), _p._ptr(num),
          _p._ptr(den), num.size, _p._ptr(q), 0)
    return q


class Trim(ctypes.Structure):
    """press_hip_trim: where the range of a read comes from - mode 0 the caller's range, 1 the jnnv2 adaptor's end, 2 the
    end of the first jnn record - and min_keep: a detector's cut that leaves fewer samples is not made"""
    _fields_ = [("mode", ctypes.c_int32), ("min_keep", ctypes.c_uint32), ("adaptor", _p.Jnn2Params), ("seg", _p.JnnParams)]


TRIM_RANGE, TRIM_ADAPTOR, TRIM_SEGMENT = 0, 1, 2  # PRESS_HIP_TRIM_*


def _trim(mode, min_keep, adaptor=None, seg=None):
    t = Trim()
    t.mode, t.min_keep = mode, int(min_keep)
    t.adaptor = _p.jnn2_params() if adaptor is None else adaptor
    t.seg = _p.jnn_params() if seg is None else seg
    return t


def trim_range():
    """a Trim of mode RANGE: the caller's ranges (None: whole reads)"""
    return _trim(TRIM_RANGE, 0)


def trim_adaptor(prm=None, min_keep=0):
    """a Trim of mode ADAPTOR: rows start behind the adaptor signal_adaptor finds under prm (default: _p.jnn2_params())"""
    return _trim(TRIM_ADAPTOR, min_keep, adaptor=prm)


def trim_segment(prm=None, min_keep=0):
    """a Trim of mode SEGMENT: rows start behind the first record of signal_segments under prm (default: the cDNA preset)"""
    return _trim(TRIM_SEGMENT, min_keep, seg=prm)


def _trim_ptr(trim):
    if trim is not None and not isinstance(trim, Trim):
        raise _p.PressError("trim must be a press.Trim or None")
    return _p._ptr(trim)


def clamp_ranges(ns, ranges):
    """the clamped ranges of reads of ns samples: b' = min(b, n), a' = min(a, b') -> (nreads, 2) uint32 (None: whole reads)"""
    ns = np.ascontiguousarray(ns, dtype=np.uint32)
    if ranges is None:
        return np.stack([np.zeros_like(ns), ns], axis=1)
    ranges = _range_pairs(ranges, ns.size)
    b = np.minimum(ranges[:, 1], ns)
    return np.stack([np.minimum(ranges[:, 0], b), b], axis=1)


def chunk_plan_ranged(ns, ranges, T, overlap):
    """_p.chunk_plan over the clamped lengths L = b' - a' (numpy; what depress_chunks_trimmed_batch computes on the device)
    -> (row_first, row_read, row_start); row_start counts from a', the start of the read's range"""
    cut = clamp_ranges(ns, ranges)
    return _p.chunk_plan(cut[:, 1] - cut[:, 0], T, overlap)


def depress_chunks_trimmed_workspace_bytes(method, total_samples, nreads, T, overlap, mode=TRIM_RANGE):
    return int(_p.load_library().press_hip_depress_chunks_trimmed_workspace_bytes(_p._mid(method), int(total_samples), int(nreads), int(T),
                                                                                int(overlap), int(mode)))


def depress_chunks_trimmed_batch(method, comp, in_off, in_len, rows, row_first, off, n, total_samples, out_n, overlap, trim=None,
                                 rng=None, seg_cal=None, cut=None, row_read=None, row_start=None, rule=None, q=None, T=None):
    """Enqueue depress_chunks_batch with a range per read and the row plan made on the device (CUDA tensors as there;
    rows may be None for a pure plan of rows of T columns; row_first int64 of nreads + 1, WRITTEN: _p.chunk_plan over the ranges' lengths; trim: a
    Trim or None (the caller's ranges); rng: 32-bit, 2 * nreads words a, b, or None; seg_cal: float32 of 2 * nreads for
    mode SEGMENT, or None; cut: 32-bit of 2 * nreads that receives a', b', or None; row_read / row_start: 32-bit of
    rows.shape[0] entries that receive each row's read and its first sample's position in the read, or None)
    (press_hip_depress_chunks_trimmed_batch)."""
    import torch
    nreads = off.numel()
    cap, dt = 0, 1
    if rows is None:
        if T is None:
            raise _p.PressError("a pure plan (rows None) needs T")
        T = int(T)
    else:
        dt = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}.get(rows.dtype)
        if dt is None or rows.dim() != 2 or not rows.is_contiguous():
            raise _p.PressError("rows must be a contiguous [nrows, T] tensor of float32, float16 or bfloat16")
        cap, T = rows.shape
    for t, name in ((q, "q"), (rng, "rng"), (seg_cal, "seg_cal"), (cut, "cut")):
        if t is not None:
            _p._f32_pairs(t, nreads, name)
    for t, name in ((row_read, "row_read"), (row_start, "row_start")):
        if t is not None and (t.numel() < cap or t.element_size() != 4 or not t.is_contiguous()):
            raise _p.PressError("%s must be a contiguous 32-bit tensor of a word per row" % name)
    _p._i64_first(row_first, nreads, "row_first")
    _p._call("press_hip_depress_chunks_trimmed_batch", _p._mid(method), _p._ptr(comp), _p._ptr(in_off), _p._ptr(in_len), nreads, _p._ptr(rows) if cap else None,
          cap, dt, T, int(overlap), _p._ptr(row_first), _p._ptr(row_read), _p._ptr(row_start), _p._ptr(off), _p._ptr(n), int(total_samples),
          _trim_ptr(trim), _p._ptr(rng), _p._ptr(seg_cal), _p._ptr(cut), _p._rule_ptr(rule), _p._ptr(q), _p._ptr(out_n), 1)


def depress_chunks_trimmed_batch_host(method, streams, ns, T, overlap, dtype="float16", trim=None, ranges=None, seg_cal=None,
                                      rule=None, nrows_cap=None):
    """Batch decode to trimmed, scaled chunk rows with host buffers (streams, ns, T, overlap, dtype, rule as in
    depress_chunks_batch_host; trim: a Trim or None; ranges: (nreads, 2) or None; seg_cal: (nreads, 2) float32 or None;
    nrows_cap: a limit in rows, default: what the batch needs) -> (rows, row_first, row_read, row_start, cut, q, out_n):
    the min(need, nrows_cap) rows that were written, their tables, and per read the plan, a' and b', the scaling
    statistics and the decoded count."""
    nreads = len(streams)
    if dtype not in _p.CHUNK_DTYPES:
        raise _p.PressError("dtype: one of %s" % ", ".join(_p.CHUNK_DTYPES))
    comp, in_off, in_len, ns, off, total = _p._decode_batch(streams, ns)
    row_first = np.zeros(nreads + 1, dtype=np.uint64)
    if int(T) <= 0 or int(T) % 8 or int(overlap) >= int(T):  # (the library refuses; the bound below needs them valid)
        cap = 0
    else:  # no trimmed batch has more rows than the untrimmed one
        cap = int(_p.chunk_plan(ns, T, overlap)[0][-1])
    if nrows_cap is not None:
        cap = min(cap, int(nrows_cap))
    rows = np.zeros((cap, max(int(T), 0)), dtype={"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[dtype])
    row_read = np.zeros(cap, dtype=np.uint32)
    row_start = np.zeros(cap, dtype=np.uint32)
    cut = np.zeros((nreads, 2), dtype=np.uint32)
    out_n = np.zeros(nreads, dtype=np.uint32)
    q = np.zeros((nreads, 2), dtype=np.int32)
    rng = _range_pairs(ranges, nreads)
    if seg_cal is not None:
        seg_cal = _p._cal_pairs(seg_cal, nreads, "seg_cal")
    _p._call("press_hip_depress_chunks_trimmed_batch", _p._mid(method), _p._ptr(comp), _p._ptr(in_off), _p._ptr(in_len), nreads,
          _p._ptr(rows) if cap else None, cap, _p.CHUNK_DTYPES[dtype], int(T), int(overlap), _p._ptr(row_first), _p._ptr(row_read), _p._ptr(row_start),
          _p._ptr(off), _p._ptr(ns), total, _trim_ptr(trim), _p._ptr(rng), _p._ptr(seg_cal), _p._ptr(cut), _p._rule_ptr(rule), _p._ptr(q), _p._ptr(out_n), 0)
    have = min(int(row_first[-1]), cap)
    return rows[:have], row_first, row_read[:have], row_start[:have], cut, q, out_n
