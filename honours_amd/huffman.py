"""The per-read Huffman family (include/press_hip.h section 2v, press_hip_huffman_*): a Huffman code built from each read's
own one-byte values, on every exception layout, huffman_{vbe21, vbbe21, vbsbe21, vbsse21}_zd.  Layouts go by name or id
(abi.RCF_LAYOUTS).  Every function here is also an attribute of honours_amd.press (press.huffman_name ...).

Through press's one call path and its shared host buffers: nothing here assigns a prototype or lays out an arena itself.
The bodies are press's helpers for the two prefix-code families (press._prefix_*), with this family's prefix.
"""
import numpy as np

from . import press as _p

_SLACK = 4096  # a default slot: the bound and this (the table)


def huffman_name(layout):
    """the reference's name of a layout's method: huffman_name("vbe21") == "huffman_vbe21_zd" """
    return _p._prefix_name("huffman", layout)


def huffman_bound(layout, n):
    """X_bound_16(n): the plain layouts' for all four; 0 for an id out of range"""
    return _p._prefix_bound("huffman", layout, n)


def huffman_press(layout, sig, cap=None):
    """huffman_L_zd_press_16 through the per-read symbol -> (ret, bytes)"""
    cap = huffman_bound(layout, np.size(sig)) + _SLACK if cap is None else int(cap)
    return _p._press_16(huffman_name(layout) + "_press_16", sig, cap)


def huffman_depress(layout, comp, cap):
    """huffman_L_zd_depress_16 through the per-read symbol, which takes the stream's length and a capacity of `cap`
    samples and finds the sample count in the stream -> (ret, int16 array)"""
    return _p._depress_16(huffman_name(layout) + "_depress_16", comp, len(comp), int(cap), kind="int")


def huffman_press_batch(layout, sig, off, n, out, out_off, out_len, maxlen=None):
    """Enqueue the compression of a batch as huffman_L_zd.  CUDA tensors as in press_batch; maxlen: None, or uint8 of
    nreads: the longest code of every read's table"""
    _p._prefix_press_batch("huffman", layout, sig, off, n, out, out_off, out_len, maxlen)


def huffman_press_sizes(layout, sig, off, n, need, maxlen=None):
    """Enqueue the exact stream lengths of a batch as huffman_L_zd: need uint64 of nreads, maxlen as in
    huffman_press_batch"""
    _p._prefix_press_sizes("huffman", layout, sig, off, n, need, maxlen)


def huffman_depress_batch(layout, comp, in_off, in_len, sig, off, n, out_n):
    """Enqueue the decompression of a batch of huffman_L_zd streams.  CUDA tensors as in depress_batch; n: the reads'
    exact sample counts"""
    _p._prefix_depress_batch("huffman", layout, comp, in_off, in_len, sig, off, n, out_n)


def huffman_press_batch_host(layout, reads, caps=None, want_maxlen=False):
    """Host buffers: reads = list of int16 arrays -> list of bytes / None (want_maxlen: and uint8 [nreads])"""
    return _p._prefix_press_batch_host("huffman", _SLACK, layout, reads, caps, want_maxlen)


def huffman_press_sizes_host(layout, reads, want_maxlen=False):
    """Host buffers: reads = list of int16 arrays -> uint64 [nreads], FAILED for an empty read (want_maxlen: and uint8
    [nreads])"""
    return _p._prefix_press_sizes_host("huffman", layout, reads, want_maxlen)


def huffman_depress_batch_host(layout, streams, ns):
    """Host buffers: streams = list of bytes, ns = the reads' exact sample counts -> list of int16 arrays / None"""
    return _p._prefix_depress_batch_host("huffman", layout, streams, ns)


def huffman_repairs():
    """(subsequences decoded again by repair round 1, by the later rounds, values decoded by the serial walk) of the
    last huffman_depress_batch; synchronises"""
    return _p._prefix_repairs("huffman")
