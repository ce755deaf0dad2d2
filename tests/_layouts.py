"""Read battery and scattered batch layouts for tests/test_batch_layouts.py.

The battery is a fixed set of 29 reads that covers the edges of every format (empty reads, tile and
chunk boundaries, exception-heavy reads, 16-bit wrap-around, q > 0, constant and NA12878-like reads).
``expect_press`` / ``expect_depress`` give what the oracle does with each of them at a given capacity or
room: that is what the device must do.  The layouts place reads, slots and streams where the header
allows them, not where the packing helpers of press.py put them.

Nothing here touches a GPU.
"""
import struct

import numpy as np

import _libs
from honours_amd import synth

FAILED64 = (1 << 64) - 1
FAILED32 = (1 << 32) - 1
SVB_KINDS = ("svb12", "svb12_zd", "svb_zd", "slow5_svb_zd")  # n of depress is the sample count, not a room
ZSTD_KINDS = ("zstd_svb_zd", "zstd_svb12_zd", "zstd_hasgam_vbsse21_zdq")
EX_FAMILY = tuple(m for m in _libs.METHODS if m not in SVB_KINDS and m not in ZSTD_KINDS)
HASGAM = ("hasgam_vbsse21_zdq", "zstd_hasgam_vbsse21_zdq")
ARENA_FILL = 0xA5     # output arena of press
SIG_FILL = 0x5A5A     # output samples of depress


def _walk(rng, n, exr=0.0, lo=-60, hi=60, exlo=-30000, exhi=30000):
    d = rng.integers(lo, hi, size=n)
    ex = rng.random(n) < exr
    d[ex] = rng.integers(exlo, exhi, size=int(ex.sum()))
    return (np.cumsum(d) + 500).astype(np.int64).astype(np.uint16).view(np.int16)


def battery():
    """-> list of (name, int16 samples): the 29 reads, the same on every run"""
    rng = np.random.default_rng(20261016)
    out = [("empty-first", np.zeros(0, dtype=np.int16))]
    for n in (1, 2, 7, 8, 9, 63, 64, 65):
        out.append(("walk-%d" % n, _walk(rng, n)))
    for n in (2047, 2048, 2049, 32767, 32768, 32769, 65543):
        out.append(("ex1-%d" % n, _walk(rng, n, 0.01)))
    out.append(("empty-middle", np.zeros(0, dtype=np.int16)))
    s = np.where(np.arange(3000) % 2 == 0, 0, 1000).astype(np.int16)   # every delta is an exception
    out.append(("all-exceptions-3000", s))
    out.append(("ex30-20000", _walk(rng, 20000, 0.30)))
    out.append(("wrap-5000", _walk(rng, 5000, 0.05, exlo=-40000, exhi=40000)))
    q = _walk(rng, 10000, 0.002)
    out.append(("q8-10000", ((q >> 3) << 3).astype(np.int16)))
    out.append(("constant-4000", np.full(4000, -1234, dtype=np.int16)))
    n, first = synth.read_lengths(7, 100, 6)
    for k in range(6):
        m = min(int(n[k]), 150000)
        out.append(("synth-%d" % k, synth.synth_read(7, 100 + k, m, int(first[k]))))
    out.append(("empty-last", np.zeros(0, dtype=np.int16)))
    assert len(out) == 29
    return out


def roundup8(x):
    return (int(x) + 7) // 8 * 8


def slot_of(bound, m, n):
    """A1 slot size of a read of n samples: the reference's bound is too small for exception-heavy reads
    (press.c:2575), so 8n + 1024 more; an empty read gets a few bytes - press_hip_bound(m, 0) is the
    reference's n - 1 wrap-around for the exception methods (8 GiB), not a size"""
    if n == 0:
        return 32
    return int(bound(m, n)) + 8 * n + 1024


ZSTD_INNER = {"zstd_svb_zd": "svb_zd", "zstd_svb12_zd": "svb12_zd", "zstd_hasgam_vbsse21_zdq": "hasgam_vbsse21_zdq"}


def zstd_content(oracle, m, s):
    """the buffer the reference hands to ZSTD_compress (press.c:1860, 2020, 8554), or None where the inner
    codec refuses the read"""
    inner = ZSTD_INNER[m]
    ret, c = oracle.press(inner, s, cap=slot_of(oracle.bound, inner, len(s)))
    if ret != 0:
        return None
    return c if inner.startswith("hasgam") else struct.pack("<I", len(s)) + c


def expect_press(oracle, m, s, cap):
    """-> the oracle's stream at capacity cap, or None where the oracle refuses the read.  The zstd kinds:
    the content of the frame (their bytes are not pinned)"""
    if m in ZSTD_KINDS:
        return zstd_content(oracle, m, s)
    ret, st = oracle.press(m, s, cap=cap)
    return st if ret == 0 else None


def check_zstd_frame(oracle, m, s, frame, content):
    """a device frame holds `content`: libzstd (when present) gives it back, and the oracle's decoder gives the
    read back wherever its buffer of 2 bytes per sample takes the content (press.c:1896)"""
    from honours_amd import press
    z = press.open_libzstd()
    if z is not None:
        a = np.frombuffer(frame, dtype=np.uint8).copy()
        out = np.zeros(len(content) + 64, dtype=np.uint8)
        r = z.ZSTD_decompress(out.ctypes.data, out.size, a.ctypes.data, len(frame))
        assert not z.ZSTD_isError(r) and out[:r].tobytes() == content, (m, len(s))
    if len(content) <= 2 * len(s):
        ret, back = oracle.depress(m, frame, len(s))
        assert ret == 0 and np.array_equal(back, s), (m, len(s))


def header_only_huffman(m, s):
    """a static-Huffman stream of s codes nothing (n = 1, or every delta an exception): a header-only stream,
    outside the decoder's domain (test_gpu_parity.py::test_micro_kats)"""
    if not m.startswith("shuffman") or len(s) == 0:
        return False
    d = (s[1:].astype(np.int32) - s[:-1].astype(np.int32)).astype(np.int16).astype(np.int32)
    return not bool((((d << 1) ^ (d >> 15)) & 0xFFFF <= 255).any())


def expect_depress(oracle, m, s, stream, room):
    """What the device must give for `stream` (bytes; b"" for a read whose press failed) with `room` samples:
    -> ("skip", None) for a stream outside the reference's domain, ("fail", None), or ("ok", samples)"""
    if stream and header_only_huffman(m, s):
        return "skip", None
    if m in ZSTD_KINDS and stream:
        # the device's own frame: any zstd decoder gives the read back
        return ("ok", s) if room >= len(s) else ("fail", None)
    ret, back = oracle.depress(m, stream, room)
    return ("ok", back) if ret == 0 else ("fail", None)


def battery_verdicts(oracle, bound):
    """The battery through the oracle at the A1 capacities and rooms: per method -> dict of counts
    (press refusals, reads left out of the sample comparison, range-coder streams stored raw)"""
    out = {}
    reads = battery()
    for m in _libs.METHODS:
        refused, skipped, raw, lossless = [], [], [], 0
        for name, s in reads:
            n = len(s)
            st = expect_press(oracle, m, s, slot_of(bound, m, n))
            if st is None:
                refused.append(name)
                continue
            if m in ZSTD_KINDS:  # the device's frame holds this content; the device's decode is checked on the GPU
                lossless += 1
                continue
            verdict, back = expect_depress(oracle, m, s, st, n)
            if verdict == "skip":
                skipped.append(name)
            elif m in _libs.RC_FAMILY and _libs.rc_stored_raw(m, st, n):
                raw.append(name)
            elif verdict == "ok" and np.array_equal(back, s):
                lossless += 1
        out[m] = {"refused": refused, "skipped": skipped, "raw": raw, "lossless": lossless}
    return out


# ------------------------------------------------------------------ layouts

def scatter_reads(rng, reads, gap_max=40):
    """reads into one int16 arena in a random permutation, each at a multiple of 8 samples behind a gap of
    0..gap_max samples; everything that is not a read is random noise -> (sig, off uint64[nreads])"""
    order = rng.permutation(len(reads))
    off = np.zeros(len(reads), dtype=np.uint64)
    pos = 0
    for k in order:
        pos = roundup8(pos + int(rng.integers(0, gap_max + 1)))
        off[k] = pos
        pos += len(reads[k])
    sig = rng.integers(-32768, 32768, size=roundup8(pos) + 64).astype(np.int16)
    for k, r in enumerate(reads):
        sig[int(off[k]):int(off[k]) + len(r)] = r
    return sig, off


def with_guards(reads, off):
    """after every read an empty guard read (at the read's end, rounded down to 8 samples) -> (ns, off)"""
    ns, offs = [], []
    for r, o in zip(reads, off):
        ns += [len(r), 0]
        offs += [int(o), (int(o) + len(r)) // 8 * 8]
    return np.array(ns, dtype=np.uint32), np.array(offs, dtype=np.uint64)


def slots(rng, sizes, first_odd=True):
    """slots of the given byte sizes back to back; out_off[0] odd -> out_off uint64[len + 1]"""
    out_off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    out_off[0] = 2 * int(rng.integers(0, 8)) + 1 if first_odd else 0
    out_off[1:] = out_off[0] + np.cumsum(np.asarray(sizes, dtype=np.uint64))
    return out_off


def scatter_streams(rng, streams):
    """streams into a fresh byte arena, in a random permutation, each at an odd byte offset behind 0..31
    random bytes, and the 64-byte tail the decoders may read -> (arena uint8, in_off, in_len)"""
    order = rng.permutation(len(streams))
    in_off = np.zeros(len(streams), dtype=np.uint64)
    in_len = np.array([len(s) for s in streams], dtype=np.uint64)
    pos = 0
    for k in order:
        pos += int(rng.integers(0, 32))
        pos |= 1
        in_off[k] = pos
        pos += len(streams[k])
    arena = rng.integers(0, 256, size=pos + 64).astype(np.uint8)
    for k, st in enumerate(streams):
        arena[int(in_off[k]):int(in_off[k]) + len(st)] = np.frombuffer(st, dtype=np.uint8)
    return arena, in_off, in_len


def scatter_rooms(rng, rooms, gap_max=40, min_gap=0):
    """rooms of the given sample counts in a random permutation at multiples of 8 samples, gaps of
    min_gap..min_gap + gap_max samples -> (off uint64, total samples)"""
    order = rng.permutation(len(rooms))
    off = np.zeros(len(rooms), dtype=np.uint64)
    pos = 0
    for k in order:
        pos = roundup8(pos + min_gap + int(rng.integers(0, gap_max + 1)))
        off[k] = pos
        pos += int(rooms[k])
    return off, roundup8(pos) + 64


def outside_rooms(total, off, spans):
    """bool mask of the samples of [0, total) outside every [off, off + span)"""
    mask = np.ones(total, dtype=bool)
    for o, k in zip(off, spans):
        mask[int(o):int(o) + int(k)] = False
    return mask
