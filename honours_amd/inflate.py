"""BLOW5 records inflated on the device (include/press_hip.h section 2zb): the zlib streams of a file with record
compression zlib, read by press_inflate.hip's kernels - one wave per record - instead of by zlib on host threads.  Every
name of __all__ is also an attribute of honours_amd.press (press.blow5_inflate_batch ...); Blow5Reader.next_batch_device
uses these calls.
"""
import numpy as np

from . import press as _p

# what honours_amd.press hands out as its own attributes (press.__getattr__ reads this list)
__all__ = ["INFLATE_STATUS", "INFLATE_DRAIN", "INFLATE_FAILED", "blow5_inflate_batch", "blow5_inflate_batch_host", "blow5_inflate_sizes",
           "blow5_inflate_sizes_host", "blow5_inflate_packed", "blow5_inflate_packed_host", "blow5_record_fields",
           "blow5_record_fields_host", "blow5_inflate_workspace_bytes"]

# status[r] (PRESS_HIP_INFLATE_*): 0 is the only success
INFLATE_STATUS = ("OK", "HEADER", "TRUNCATED", "BTYPE", "STORED", "CODES", "SYMBOL", "DISTANCE", "ADLER", "ROOM", "REFUSED")
INFLATE_DRAIN = 4096  # bytes a wave produces between two writes of its LDS window to the slot (PRESS_HIP_INFLATE_DRAIN)
INFLATE_FAILED = 0xFFFFFFFFFFFFFFFF  # out_len / need / sig_len of a failed record (-1 in the int64 tensors)


def blow5_inflate_batch(comp, comp_off, comp_len, out, out_off, out_len, status):
    """Enqueue the inflating of a batch of zlib streams into the caller's slots (press_hip_blow5_inflate_batch).  CUDA
    tensors: comp uint8 (the arena of the streams), comp_off / comp_len int64 (nrec), out uint8, out_off int64 (nrec + 1:
    record r into out[out_off[r]:out_off[r + 1]]), out_len int64 (nrec, WRITTEN: the inflated length, -1 = failed; under
    status ROOM the length the record needs), status uint8 (nrec, WRITTEN: an index into INFLATE_STATUS)."""
    _p._call("press_hip_blow5_inflate_batch", _p._ptr(comp), _p._ptr(comp_off), _p._ptr(comp_len), comp.numel(), comp_len.numel(),
             _p._ptr(out), _p._ptr(out_off), _p._ptr(out_len), _p._ptr(status), 1)


def blow5_inflate_sizes(comp, comp_off, comp_len):
    """Enqueue the counting walk alone (press_hip_blow5_inflate_sizes; no Adler-32 check).  -> (need int64, status uint8)
    CUDA tensors: the inflated lengths, -1 = the stream is not well formed"""
    import torch

    nrec = comp_len.numel()
    need = torch.empty(nrec, dtype=torch.int64, device=comp.device)
    status = torch.empty(nrec, dtype=torch.uint8, device=comp.device)
    _p._call("press_hip_blow5_inflate_sizes", _p._ptr(comp), _p._ptr(comp_off), _p._ptr(comp_len), comp.numel(), nrec, _p._ptr(need),
             _p._ptr(status), 1)
    return need, status


def blow5_inflate_packed(comp, comp_off, comp_len, out, out_off, out_len, status, align=16):
    """Enqueue the inflating into an arena the library lays out (press_hip_blow5_inflate_packed): out uint8 CUDA tensor
    (its size: out_cap), out_off int64 (nrec + 1, WRITTEN: gap-free up to `align`, out_off[-1] what the batch needs), out_len
    and status as in blow5_inflate_batch; a failed record takes no byte."""
    _p._call("press_hip_blow5_inflate_packed", _p._ptr(comp), _p._ptr(comp_off), _p._ptr(comp_len), comp.numel(), comp_len.numel(),
             _p._ptr(out), out.numel(), int(align), _p._ptr(out_off), _p._ptr(out_len), _p._ptr(status), 1)


def blow5_record_fields(rec, rec_off, rec_len, signal_method=1, want_dor=True, want_ids=True):
    """Enqueue parse_record's rules over inflated records in a device arena (press_hip_blow5_record_fields): rec uint8,
    rec_off / rec_len int64 CUDA tensors (e.g. blow5_inflate_packed's out_off[:-1] and out_len).  -> (sig_off int64,
    sig_len int64 (-1: refused), n_samples int32 bits of a u32, dor float64 (nrec, 3) or None, ids uint8 (nrec, 64) or None),
    CUDA tensors: sig_off / sig_len are depress_batch's in_off / in_len over `rec`."""
    import torch

    nrec = rec_len.numel()
    dev = rec.device
    sig_off = torch.empty(nrec, dtype=torch.int64, device=dev)
    sig_len = torch.empty(nrec, dtype=torch.int64, device=dev)
    ns = torch.empty(nrec, dtype=torch.int32, device=dev)
    dor = torch.empty((nrec, 3), dtype=torch.float64, device=dev) if want_dor else None
    ids = torch.empty((nrec, _p.Blow5Reader.ID_LEN), dtype=torch.uint8, device=dev) if want_ids else None
    _p._call("press_hip_blow5_record_fields", _p._ptr(rec), _p._ptr(rec_off), _p._ptr(rec_len), rec.numel(), nrec, int(signal_method),
             _p._ptr(sig_off), _p._ptr(sig_len), _p._ptr(ns), _p._ptr(dor) if want_dor else None, _p._ptr(ids) if want_ids else None, 1)
    return sig_off, sig_len, ns, dor, ids


def blow5_inflate_workspace_bytes(comp_bytes, nrec):
    """the scratch the device-resident calls take (host arithmetic)"""
    return int(_p.load_library().press_hip_blow5_inflate_workspace_bytes(int(comp_bytes), int(nrec)))


# ---------------------------------------------------------------------------- host buffers

def _streams(streams):
    comp, off, ln = _p._streams_arena([bytes(s) for s in streams])
    return comp[:comp.size - 64], off, ln


def blow5_inflate_sizes_host(streams):
    """-> (need uint64 (nrec), status uint8 (nrec)) of a list of zlib streams (bytes)"""
    comp, off, ln = _streams(streams)
    n = len(streams)
    need = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    _p._call("press_hip_blow5_inflate_sizes", _p._ptr(comp), _p._ptr(off), _p._ptr(ln), comp.size, n, _p._ptr(need), _p._ptr(status), 0)
    return need, status


def blow5_inflate_batch_host(streams, out, out_off):
    """Inflate a list of zlib streams (bytes) into the caller's slots: out numpy uint8, out_off uint64 (nrec + 1).  ->
    (out_len uint64, status uint8); a failed record's slot is left as it was."""
    comp, off, ln = _streams(streams)
    n = len(streams)
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    out_len = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    _p._call("press_hip_blow5_inflate_batch", _p._ptr(comp), _p._ptr(off), _p._ptr(ln), comp.size, n, _p._ptr(out), _p._ptr(out_off),
             _p._ptr(out_len), _p._ptr(status), 0)
    return out_len, status


def blow5_inflate_packed_host(streams, out_cap=None, align=16):
    """Inflate a list of zlib streams (bytes) into one arena -> (out uint8, out_off uint64 (nrec + 1), out_len uint64,
    status uint8).  out_cap None: as much as the batch needs (two calls: the sizes first)."""
    comp, off, ln = _streams(streams)
    n = len(streams)
    if out_cap is None:
        need, _ = blow5_inflate_sizes_host(streams)
        out_cap = int(sum(((int(v) + align - 1) // align * align) for v in need if v != INFLATE_FAILED))
    out = np.zeros(max(int(out_cap), 1), dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    out_len = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    _p._call("press_hip_blow5_inflate_packed", _p._ptr(comp), _p._ptr(off), _p._ptr(ln), comp.size, n, _p._ptr(out), int(out_cap),
             int(align), _p._ptr(out_off), _p._ptr(out_len), _p._ptr(status), 0)
    return out, out_off, out_len, status


def blow5_record_fields_host(records, signal_method=1):
    """parse_record's rules over a list of inflated records (bytes), on the device -> (sig_off uint64 - the field's
    position in its record - sig_len uint64, n_samples uint32, dor float64 (nrec, 3), ids list of str)"""
    rec, off, ln = _streams(records)
    n = len(records)
    sig_off = np.zeros(n, dtype=np.uint64)
    sig_len = np.zeros(n, dtype=np.uint64)
    ns = np.zeros(n, dtype=np.uint32)
    dor = np.zeros((n, 3), dtype=np.float64)
    ids = np.zeros((n, _p.Blow5Reader.ID_LEN), dtype=np.uint8)
    _p._call("press_hip_blow5_record_fields", _p._ptr(rec), _p._ptr(off), _p._ptr(ln), rec.size, n, int(signal_method), _p._ptr(sig_off),
             _p._ptr(sig_len), _p._ptr(ns), _p._ptr(dor), _p._ptr(ids), 0)
    return sig_off - off, sig_len, ns, dor, [bytes(r).split(b"\0")[0].decode() for r in ids]
