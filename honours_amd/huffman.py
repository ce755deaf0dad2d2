"""The per-read Huffman family (include/press_hip.h section 2v, press_hip_huffman_*): a Huffman code built from each read's
own one-byte values, on every exception layout, huffman_{vbe21, vbbe21, vbsbe21, vbsse21}_zd.  Layouts go by name or id
(abi.RCF_LAYOUTS).  Every function here is also an attribute of honours_amd.press (press.huffman_name ...).

Through press's one call path and its shared host buffers: nothing here assigns a prototype or lays out an arena itself.
"""
import numpy as np

from .abi import RCF_LAYOUTS, load_library
from .press import (_call, _decode_batch, _depress_16, _host_batch, _press_16, _ptr, _reads_of, _slots,  # noqa: F401
                    _streams_of)


def _layout_id(layout):
    return RCF_LAYOUTS[layout] if isinstance(layout, str) else int(layout)


def huffman_name(layout):
    """the reference's name of a layout's method: huffman_name("vbe21") == "huffman_vbe21_zd" """
    l = _layout_id(layout)
    return "huffman_%s_zd" % [k for k, v in RCF_LAYOUTS.items() if v == l][0]


def huffman_bound(layout, n):
    """X_bound_16(n): the plain layouts' for all four; 0 for an id out of range"""
    return int(load_library().press_hip_huffman_bound(_layout_id(layout), int(n)))


def huffman_press(layout, sig, cap=None):
    """huffman_L_zd_press_16 through the per-read symbol -> (ret, bytes)"""
    cap = huffman_bound(layout, np.size(sig)) + 4096 if cap is None else int(cap)
    return _press_16(huffman_name(layout) + "_press_16", sig, cap)


def huffman_depress(layout, comp, cap):
    """huffman_L_zd_depress_16 through the per-read symbol, which takes the stream's length and a capacity of `cap`
    samples and finds the sample count in the stream -> (ret, int16 array)"""
    return _depress_16(huffman_name(layout) + "_depress_16", comp, len(comp), int(cap), kind="int")


def huffman_press_batch(layout, sig, off, n, out, out_off, out_len, maxlen=None):
    """Enqueue the compression of a batch as huffman_L_zd.  CUDA tensors as in press_batch; maxlen: None, or uint8 of
    nreads: the longest code of every read's table"""
    _call("press_hip_huffman_press_batch", _layout_id(layout), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(),
          _ptr(out), _ptr(out_off), _ptr(out_len), _ptr(maxlen), 1)


def huffman_press_sizes(layout, sig, off, n, need, maxlen=None):
    """Enqueue the exact stream lengths of a batch as huffman_L_zd: need uint64 of nreads, maxlen as in
    huffman_press_batch"""
    _call("press_hip_huffman_press_sizes", _layout_id(layout), _ptr(sig), _ptr(off), _ptr(n), off.numel(), sig.numel(),
          _ptr(need), _ptr(maxlen), 1)


def huffman_depress_batch(layout, comp, in_off, in_len, sig, off, n, out_n):
    """Enqueue the decompression of a batch of huffman_L_zd streams.  CUDA tensors as in depress_batch; n: the reads'
    exact sample counts"""
    _call("press_hip_huffman_depress_batch", _layout_id(layout), _ptr(comp), _ptr(in_off), _ptr(in_len), off.numel(),
          _ptr(sig), _ptr(off), _ptr(n), sig.numel(), _ptr(out_n), 1)


def huffman_press_batch_host(layout, reads, caps=None, want_maxlen=False):
    """Host buffers: reads = list of int16 arrays -> list of bytes / None (want_maxlen: and uint8 [nreads])"""
    l = _layout_id(layout)
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    if caps is None:
        caps = [huffman_bound(l, int(x)) + 4096 if x else 32 for x in ns]
    out_off = _slots(caps)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    out_len = np.zeros(nreads, dtype=np.uint64)
    maxlen = np.zeros(nreads, dtype=np.uint8)
    _call("press_hip_huffman_press_batch", l, _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(out), _ptr(out_off),
          _ptr(out_len), _ptr(maxlen) if want_maxlen else None, 0)
    streams = _streams_of(out, out_off, out_len)
    return (streams, maxlen) if want_maxlen else streams


def huffman_press_sizes_host(layout, reads, want_maxlen=False):
    """Host buffers: reads = list of int16 arrays -> uint64 [nreads], FAILED for an empty read (want_maxlen: and uint8
    [nreads])"""
    nreads = len(reads)
    sig, off, ns, total = _host_batch(reads)
    need = np.zeros(nreads, dtype=np.uint64)
    maxlen = np.zeros(nreads, dtype=np.uint8)
    _call("press_hip_huffman_press_sizes", _layout_id(layout), _ptr(sig), _ptr(off), _ptr(ns), nreads, total, _ptr(need),
          _ptr(maxlen) if want_maxlen else None, 0)
    return (need, maxlen) if want_maxlen else need


def huffman_depress_batch_host(layout, streams, ns):
    """Host buffers: streams = list of bytes, ns = the reads' exact sample counts -> list of int16 arrays / None"""
    comp, in_off, in_len, ns, off, total = _decode_batch(streams, ns)
    sig = np.zeros(total + 64, dtype=np.int16)
    out_n = np.zeros(len(streams), dtype=np.uint32)
    _call("press_hip_huffman_depress_batch", _layout_id(layout), _ptr(comp), _ptr(in_off), _ptr(in_len), len(streams),
          _ptr(sig), _ptr(off), _ptr(ns), total, _ptr(out_n), 0)
    return _reads_of(sig, off, out_n)


def huffman_repairs():
    """(subsequences decoded again by repair round 1, by the later rounds, values decoded by the serial walk) of the
    last huffman_depress_batch; synchronises"""
    c = np.zeros(3, dtype=np.uint32)
    _call("press_hip_huffman_repairs", _ptr(c))
    return tuple(int(x) for x in c)
