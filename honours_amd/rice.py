"""The Rice family (include/press_hip.h section 2u, press_hip_rice_*): Golomb-Rice coding of the one-byte values on every
exception layout, rice_{vbe21, vbbe21, vbsbe21, vbsse21}_zd.  Layouts go by name or id (abi.RCF_LAYOUTS), as the range-coder
family takes them.  Every function here is also an attribute of honours_amd.press (press.rice_name ...).

Through press's one call path and its shared host buffers: nothing here assigns a prototype or lays out an arena itself.
"""
import numpy as np

from .abi import RCF_LAYOUTS, load_library
from .press import (_call, _decode_batch, _depress_16, _host_batch, _press_16, _ptr, _reads_of, _slots,  # noqa: F401
                    _streams_of)


def _rice_id(layout):
    return RCF_LAYOUTS[layout] if isinstance(layout, str) else int(layout)


def rice_name(layout):
    """the reference's name of a layout's method: rice_name("vbe21") == "rice_vbe21_zd" """
    l = _rice_id(layout)
    return "rice_%s_zd" % [k for k, v in RCF_LAYOUTS.items() if v == l][0]


def rice_bound(layout, n):
    """X_bound_16(n): the plain layouts' for all four; 0 for an id out of range"""
    return int(load_library().press_hip_rice_bound(_rice_id(layout), int(n)))


def rice_press(layout, sig, cap=None):
    """rice_L_zd_press_16 through the per-read symbol -> (ret, bytes); ret -1: the library reports *nout = 0"""
    cap = rice_bound(layout, np.size(sig)) + 1024 if cap is None else int(cap)
    return _press_16(rice_name(layout) + "_press_16", sig, cap)


def rice_depress(layout, comp, n):
    """rice_L_zd_depress_16 through the per-read symbol, which takes the SAMPLE count n as its input size, as the
    reference's does -> (ret, int16 array)"""
    return _depress_16(rice_name(layout) + "_depress_16", comp, int(n), n)


def rice_press_batch(layout, sig, off, n, out, out_off, out_len, k=None):
    """Enqueue the compression of a batch as rice_L_zd.  CUDA tensors as in press_batch; k: None, or uint8 of nreads:
    the Rice parameter every read was coded with"""
    _call("press_hip_rice_press_batch", _rice_id(layout), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(),
          _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(k), 1)


def rice_press_sizes(layout, sig, off, n, need, k=None):
    """Enqueue the exact stream lengths of a batch as rice_L_zd: need uint64 of nreads, k as in rice_press_batch"""
    _call("press_hip_rice_press_sizes", _rice_id(layout), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(),
          _ptr(need), _ptr(k), 1)


def rice_depress_batch(layout, comp, in_off, in_len, sig, off, n, out_n):
    """Enqueue the decompression of a batch of rice_L_zd streams.  CUDA tensors as in depress_batch; n: the reads' exact
    sample counts"""
    _call("press_hip_rice_depress_batch", _rice_id(layout), _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(),
          _ptr(sig), _ptr(off), _ptr(n), sig.numel(), _ptr(out_n), 1)


def rice_press_batch_host(layout, reads, caps=None, want_k=False):
    """Host buffers: reads = list of int16 arrays -> list of bytes / None (want_k: and uint8 [nreads])"""
    l = _rice_id(layout)
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    if caps is None:
        caps = [rice_bound(l, int(x)) + 1024 if x else 32 for x in ns]
    out_off = _slots(caps)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    out_len = np.zeros(nreads, dtype=np.uint64)
    k = np.zeros(nreads, dtype=np.uint8)
    _call("press_hip_rice_press_batch", l, _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(out), _ptr(out_off),
          _ptr(out_len), _ptr(k) if want_k else None, 0)
    streams = _streams_of(out, out_off, out_len)
    return (streams, k) if want_k else streams


def rice_press_sizes_host(layout, reads, want_k=False):
    """Host buffers: reads = list of int16 arrays -> uint64 [nreads], FAILED for an empty read (want_k: and uint8
    [nreads])"""
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    need = np.zeros(nreads, dtype=np.uint64)
    k = np.zeros(nreads, dtype=np.uint8)
    _call("press_hip_rice_press_sizes", _rice_id(layout), _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(need),
          _ptr(k) if want_k else None, 0)
    return (need, k) if want_k else need


def rice_depress_batch_host(layout, streams, ns):
    """Host buffers: streams = list of bytes, ns = the reads' exact sample counts -> list of int16 arrays / None"""
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    sig = np.zeros(total + 64, dtype=np.int16)
    out_n = np.zeros(len(streams), dtype=np.uint32)
    _call("press_hip_rice_depress_batch", _rice_id(layout), _ptr(comp), _ptr(in_off), _ptr(in_len), len(streams),
          _ptr(sig), _ptr(off), _ptr(ns), total, _ptr(out_n), 0)
    return _reads_of(sig, off, out_n)


def rice_repairs():
    """(subsequences decoded again by repair round 1, by round 2, values decoded by the serial walk) of the last
    rice_depress_batch; synchronises"""
    c = np.zeros(3, dtype=np.uint32)
    _call("press_hip_rice_repairs", _ptr(c))
    return tuple(int(x) for x in c)
