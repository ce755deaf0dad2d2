"""The device's zstd frame reader (press_zstd.hip: k_zs_walk, DevSink, k_zs_copy, k_zs_hdecode, k_zs_exec; zs_table.h:
walk_frame, read_tree, seq_table) on the whole frame format of RFC 8878 and on its fallback to libzstd on the host.

* the corpus: byte texts embedded as svb-zd reads and framed by ZSTD_compressStream2 with flushes and parameters, the
  other two kinds' buffers framed the same way, and hand-forged frames for what libzstd does not emit (tests/_zsframes.py)
* a census of the corpus' frames, from their headers, must reach every feature of FEATURES - on the CPU and again for
  exactly the frames the device has decoded without the host
* frames that must go to the host (several frames in a stream, skippable frames, dictionaries, more trees / blocks with
  sequences than the batch's lists hold) among ordinary ones
* damaged frames: the device refuses a read or returns what libzstd makes of the same bytes

Expected contents are ZSTD_decompress's, expected samples the oracle's inner decoder's, digests zlib.crc32's: none comes
from the library under test.
"""
import ctypes
import functools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import _libs
import _zsframes as zf
from test_zstd_frames import KINDS, MODEL_SO, cases, model, prezstd  # noqa: F401 (model: the fixture that builds MODEL_SO)

ROOT = _libs.ROOT
gpu = pytest.mark.gpu


def _zstd():
    from honours_amd import press
    z = press.open_libzstd()
    if z is None:
        pytest.skip("no libzstd")
    if not zf.have_streaming(z):
        pytest.skip("this libzstd has no ZSTD_compressStream2")
    return z


# every part of the format the corpus must hold (census keys of _zsframes.census)
FEATURES = [
    "block_raw", "block_rle", "block_compressed", "block_raw_mid", "block_rle_mid", "block_compressed_mid", "block_empty_last",
    "lit_raw_with_seq", "lit_raw_no_seq", "lit_rle_with_seq", "lit_rle_no_seq", "lit_huf_with_seq", "lit_huf_no_seq",
    "lit_treeless_with_seq", "lit_treeless_no_seq",
    "lit_hdr_raw_1", "lit_hdr_raw_2", "lit_hdr_raw_3", "lit_hdr_rle_1", "lit_hdr_rle_2", "lit_hdr_rle_3",
    "tree_fse", "tree_direct", "huf_one_stream", "huf_four_streams", "long_block", "long_with_seq",
    "seq_count_1_byte", "seq_count_2_byte", "seq_count_3_byte",
    "ll_mode_predefined", "ll_mode_rle", "ll_mode_fse", "ll_mode_repeat",
    "of_mode_predefined", "of_mode_rle", "of_mode_fse", "of_mode_repeat",
    "ml_mode_predefined", "ml_mode_rle", "ml_mode_fse", "ml_mode_repeat",
    "rep_offset_1", "rep_offset_2", "rep_offset_0_minus_1", "new_offset",
    "hdr_single_segment", "hdr_window_descriptor", "hdr_no_content_size", "hdr_content_size_1", "hdr_content_size_2",
    "hdr_content_size_4", "hdr_content_size_8", "hdr_checksum", "hdr_no_checksum",
]

STEPS = (97, 1000, 5000, 40000, None)
PARAMS = (dict(level=1), dict(level=3, checksumFlag=1), dict(level=9, contentSizeFlag=0), dict(level=19, windowLog=10),
          dict(level=5, minMatch=3))


def content_room(kind, n):
    """content bytes the device leaves room for in a read of n samples (press_methods.hip, zs_host_frames): more than any
    corpus frame holds, so that libzstd decodes into it what the device may accept"""
    kdiv = KINDS[kind][1]
    return 4 + (n + kdiv - 1) // kdiv + 2 * n if kdiv else 16 * max(n, 1) + 64


def expect_samples(oracle, kind, cont, room):
    """the samples a content stands for, by the oracle's decoder of the inner stream; None: no read of at most `room` samples"""
    inner, kdiv = KINDS[kind]
    if cont is None:
        return None
    if not kdiv:
        ret, s = oracle.depress(inner, cont, room)
        return None if ret else s
    if len(cont) < 4:
        return None
    n, = struct.unpack("<I", cont[:4])
    if n > room:
        return None
    ret, s = oracle.depress(inner, cont[4:], n)
    return None if ret or len(s) != n else s


class Frame:
    def __init__(self, z, oracle, kind, frame, room, tag):
        self.kind, self.frame, self.room, self.tag = kind, frame, room, tag
        self.content = zf.content(z, frame, content_room(kind, room))
        self.expect = expect_samples(oracle, kind, self.content, room)
        self.census = zf.census(frame) if self.content is not None else None


def texts():
    rng = np.random.default_rng(5)  # (the five of test_zstd_frames.test_model_reader_on_both_kinds_of_frames)
    out = [bytes(rng.integers(0, 4, 70000, dtype=np.uint8)), b"abcabcabd" * 9000, bytes(200000),
           bytes(rng.integers(0, 256, 300, dtype=np.uint8)) * 700, b"x" * 5 + bytes(range(256)) * 600]
    # long blocks (four streams of more than 4096 literals each) that also carry sequences: skewed random bytes with
    # forty copied pieces of 8 to 40 bytes
    rng = np.random.default_rng(6)
    t = bytearray((rng.integers(0, 16, 150000) * rng.integers(0, 16, 150000) // 15).astype(np.uint8).tobytes())
    for _ in range(40):
        k, a, b = int(rng.integers(8, 41)), int(rng.integers(0, 70000)), int(rng.integers(75000, 149000))
        t[b:b + k] = t[a:a + k]
    out.append(bytes(t))
    out.append(bytes(rng.integers(0, 16, 40000, dtype=np.uint8)))  # sixteen equally likely values: every code 4 bits
    out.append(b"x" * 100000)
    return out


def forged_frames():
    """-> [(tag, frame)]: what libzstd does not emit.  Every content is an svb-zd buffer: [u32 n][zero key bytes][n data bytes]"""
    out = []
    rng = np.random.default_rng(8)
    n = 300
    data = bytes(rng.integers(0, 8, n, dtype=np.uint8))
    body = struct.pack("<I", n) + bytes((n + 3) // 4) + data
    size = len(body)
    one = zf.block(0, body, last=True)
    # ---- frame headers
    for single, fcs in ((True, 1), (True, 2), (True, 4), (True, 8), (False, 0), (False, 2), (False, 4), (False, 8)):
        if fcs == 1:  # (one byte of content size: a content below 256 bytes)
            small = struct.pack("<I", 100) + bytes(25) + data[:100]
            out.append(("header single fcs 1", zf.frame_header(len(small), True, 1) + zf.block(0, small, last=True)))
            continue
        out.append(("header %s fcs %d" % ("single" if single else "window", fcs), zf.frame_header(size, single, fcs) + one))
    out.append(("header checksum arbitrary", zf.frame_header(size, True, 2, checksum=True) + one + b"\x12\x34\x56\x78"))
    out.append(("header wrong content size", zf.frame_header(size + 1, True, 2) + one))
    for width in (1, 2, 4):
        out.append(("header dictionary id %d" % width, zf.frame_header(size, True, 2, dict_id=(7, width)) + one))
    # ---- raw and RLE blocks, raw and RLE literals in all size formats (no sequences: the byte 0 behind the literals)
    out.append(("blocks raw rle raw", zf.frame_header(size, True, 2) + zf.svb_head(n) + zf.block(0, data, last=True)))
    for kind in (0, 1):
        for fmt in (1, 2, 3):
            k = 28 if fmt == 1 else 300 if fmt == 2 else 5000
            d = bytes(rng.integers(0, 8, k, dtype=np.uint8))
            lit = zf.literals(0, d, fmt) if kind == 0 else zf.literals(1, (4, k), fmt)
            out.append(("literals %s format %d no sequences" % (("raw", "rle")[kind], fmt),
                        zf.frame_header(4 + (k + 3) // 4 + k, True, 4) + zf.svb_head(k) + zf.block(2, lit + b"\0", last=True)))
    # ---- a compressed block between a raw and an RLE block; an empty last raw block behind a content-carrying one
    k = 600
    d = bytes(rng.integers(0, 8, 200, dtype=np.uint8))
    out.append(("compressed between raw and rle", zf.frame_header(4 + k // 4 + k, False, 0) + zf.block(0, struct.pack("<I", k) + bytes(k // 4))
                + zf.block(0, d) + zf.block(2, zf.literals(0, d, 2) + b"\0") + zf.block(1, b"\x06", last=True, rle_count=200)))
    out.append(("empty last raw block", zf.frame_header(size, True, 2) + zf.block(0, body) + zf.block(0, b"", last=True)))
    # ---- sequences with the three tables in RLE mode.  In front: the count, the keys, 64 varied data bytes (what the
    # matches copy, so that a wrong offset shows)
    seed = bytes(rng.integers(0, 8, 64, dtype=np.uint8))

    def seq_frame(tag, blocks, hdr=(True, 4)):
        # blocks: (literals section, its R, seqs, llc, ofc, mlc, count form); the content size by the sequences' own sums
        nd = 64
        body = b""
        rep = (1, 4, 8)
        for i, (lit, R, seqs, llc, ofc, mlc, form) in enumerate(blocks):
            offs, rep, _ = zf.offsets_history(seqs, rep)
            assert sum(s[0] for s in seqs) <= R and max(offs) <= 64
            nd += R + sum(s[1] for s in seqs)
            body += zf.block(2, lit + zf.sequences_rle(seqs, llc, ofc, mlc, form), last=i == len(blocks) - 1)
        total = 4 + (nd + 3) // 4 + nd
        out.append((tag, zf.frame_header(total, hdr[0], hdr[1]) + zf.svb_head(nd) + zf.block(0, seed) + body))

    def rep_seqs(count, ofc):
        # every literal length 0.  Offset code 0: offset value 1 = rep[1].  Code 1: value 2 = rep[2], 3 = rep[0] - 1
        # (taken whenever rep[0] - 1 is still an offset)
        seqs, rep = [], (1, 4, 8)
        for i in range(count):
            v = 1 if ofc == 0 else 3 if rep[0] > 1 and rng.integers(0, 2) else 2
            seqs.append((0, 3, v))
            _, rep, _ = zf.offsets_history(seqs[-1:], rep)
        return seqs
    for count in (7, 200, 32612, 40000):
        for ofc in (0, 1):
            seq_frame("rle sequences %d offset code %d" % (count, ofc),
                      [(zf.literals(1, (5, 40), 2), 40, rep_seqs(count, ofc), 0, ofc, 0, None)])
    # new offsets (code 5: 29 .. 60 bytes back) with literals between the matches, then the repeat branches in a second
    # block whose history the first one left; raw literals; the 2-byte count form for a count that fits one byte
    s1 = [(2, 4, 32 + int(rng.integers(0, 32))) for _ in range(50)]
    lit1 = bytes(rng.integers(0, 8, 120, dtype=np.uint8))
    s2, rep = [], zf.offsets_history(s1)[1]
    for i in range(60):
        v = 3 if rep[0] > 9 and i % 3 else 2
        s2.append((0, 5, v))
        _, rep, _ = zf.offsets_history(s2[-1:], rep)
    seq_frame("new offsets then repeats", [(zf.literals(0, lit1, 2), 120, s1, 2, 5, 1, 2),
                                           (zf.literals(1, (3, 9), 1), 9, s2, 0, 1, 2, None)], hdr=(False, 0))
    # RLE literals with sequences whose literal lengths take from them
    s3 = [(3, 6, 2 + int(rng.integers(0, 2))) for _ in range(30)]
    seq_frame("rle literals spent by sequences", [(zf.literals(1, (7, 100), 3), 100, s3, 3, 1, 3, None)])
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    z = _zstd()
    oracle = _libs.oracle()
    out = []
    for ti, t in enumerate(texts()):
        s, buf = zf.samples_for_text(oracle, t)
        for step in STEPS:
            for pi, p in enumerate(PARAMS):
                out.append(Frame(z, oracle, "zstd_svb_zd", zf.stream_frames(z, buf, step, p), len(s),
                                 "text %d step %s params %d" % (ti, step, pi)))
    reads = cases()[:20]
    for kind in sorted(KINDS):
        for k, s in enumerate(reads):
            buf = prezstd(oracle, s, KINDS[kind][0])
            if buf is None:
                continue
            for step in (1000, None):
                out.append(Frame(z, oracle, kind, zf.stream_frames(z, buf, step, dict(level=1)), len(s),
                                 "%s case %d step %s" % (kind, k, step)))
    for tag, f in forged_frames():
        # (the room: the count in the content; 300, every such frame's, where libzstd refuses the frame)
        c = zf.content(z, f, 1 << 20)
        room = struct.unpack("<I", c[:4])[0] if c is not None else 300
        out.append(Frame(z, oracle, "zstd_svb_zd", f, room, "forged: " + tag))
    return out


def zsm():
    m = ctypes.CDLL(MODEL_SO)
    m.zsm_decode.restype = ctypes.c_int64
    m.zsm_decode.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]

    def dec(f, cap):
        a = np.frombuffer(f, dtype=np.uint8).copy() if len(f) else np.zeros(1, dtype=np.uint8)
        out = np.zeros(cap + 64, dtype=np.uint8)
        r = int(m.zsm_decode(a.ctypes.data, len(f), out.ctypes.data, cap))
        return r, out[:max(r, 0)].tobytes()
    return dec


def total_census(frames):
    c = zf.collections.Counter()
    for f in frames:
        if f.census is not None:
            c.update(f.census)
    return c


# ------------------------------------------------------------------ CPU


def test_model_reads_the_corpus(model):
    """zs::walk_frame on the host: libzstd's content for every frame; what libzstd refuses is not accepted"""
    dec = zsm()
    refused = 0
    for f in corpus():
        r, b = dec(f.frame, content_room(f.kind, f.room))
        if f.content is None:
            assert r < 0, f.tag + ": libzstd refuses it, the model reads %d bytes" % r
            refused += 1
        else:
            assert r == len(f.content) and b == f.content, (f.tag, r)
            assert f.expect is not None, f.tag
    assert refused >= 4  # the arbitrary checksum, the wrong content size, (the dictionary ids: left to libzstd)


def test_corpus_census():
    """the corpus holds every part of the format named in FEATURES (and stays small)"""
    fs = corpus()
    c = total_census(fs)
    missing = [k for k in FEATURES if c[k] < 1]
    assert not missing, missing
    assert len(fs) < 500 and max(f.room for f in fs) <= 210000
    print({k: c[k] for k in FEATURES})


# ------------------------------------------------------------------ damaged frames (CPU: the sanitizer-built model; GPU: test 5)

# one frame per family of features: the first corpus frame whose census holds the key
FAMILIES = ("lit_treeless_with_seq", "tree_fse", "tree_direct", "long_with_seq", "of_mode_repeat", "ll_mode_rle", "ml_mode_fse",
            "seq_count_2_byte", "seq_count_3_byte", "rep_offset_0_minus_1", "lit_rle_with_seq", "block_raw_mid", "hdr_checksum")


@functools.lru_cache(maxsize=None)
def damaged():
    """-> [(Frame of the damaged bytes, the undamaged Frame)]: five damaged copies of each of a dozen corpus frames - one
    seeded byte inside a sequences section or a tree description changed, or the frame cut at a block boundary"""
    z = _zstd()
    oracle = _libs.oracle()
    rng = np.random.default_rng(44)
    picked = []
    for key in FAMILIES:
        for f in corpus():
            if f.kind == "zstd_svb_zd" and f.census is not None and f.census[key] and f not in picked and len(f.frame) < 150000:
                picked.append(f)
                break
        else:
            raise AssertionError("no corpus frame with " + key)
    out = []
    for f in picked:
        spans = []
        zf.census(f.frame, spans)
        inner = [s for s in spans if s[0] != "block"]
        cuts = [s[1] for s in spans if s[0] == "block"][1:]
        for k in range(5):
            x = bytearray(f.frame)
            if k == 4 and cuts:
                x = x[:cuts[int(rng.integers(0, len(cuts)))]]
            else:
                _, a, b = inner[int(rng.integers(0, len(inner)))] if inner else ("", 4, len(x))
                at = int(rng.integers(a, b))
                x[at] ^= 1 << int(rng.integers(0, 8))
            out.append((Frame(z, oracle, f.kind, bytes(x), f.room, "%s damaged %d" % (f.tag, k)), f))
    return out


def test_sanitized_model_reads_the_damaged_frames(tmp_path):
    """the frames of test 5 through zs::walk_frame built for the host with AddressSanitizer + UBSan (oracle/zsframe_fuzz,
    a program of its own): no finding, so the device is given nothing that leaves the frame or the room"""
    exe = os.path.join(ROOT, "oracle", "zsframe_fuzz")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "zsfuzz"], check=True)
    ds = damaged()
    assert len(ds) >= 60
    for i, (d, _) in enumerate(ds):
        with open(os.path.join(tmp_path, "%03d_%d.bin" % (i, content_room(d.kind, d.room))), "wb") as fh:
            fh.write(d.frame)
    r = subprocess.run([exe, "0", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no finding" in r.stdout
    got = [int(w) for w in r.stdout.replace(",", " ").split() if w.isdigit()]
    assert sum(got[:3]) == len(ds), r.stdout


# ------------------------------------------------------------------ GPU


def plan_caps(nreads, total):
    """The lists of a decode batch that the frames of one batch share (press_methods.hip, make_plan; total: the sum of the
    rooms, each rounded up to 8 samples, as press.depress_batch_host lays them out):
        max_blocks = total * 2 / 16384 + nreads + 1
        cap_copy   = max_blocks + total / 256 + 16 * nreads + 64      raw pieces above ZCOPY_INLINE, taken 8 at a time
        cap_units  = max_blocks / 8 + 2 * nreads + 64                 up to 8 Huffman blocks of one tree
        cap_trees  = 4 * nreads + 64                                  a read's first tree has slot r: 3 * nreads + 64 others
        cap_long   = total / 8192 + nreads + 64                       four-stream blocks of more than 16 384 literals
        cap_seq    = total / 4 + 64 * nreads + 1024
        cap_xblk   = max_blocks / 4 + 4 * nreads + 64                 blocks with sequences
    The tests below aim at these: a change of the caps re-aims them (their own assertions fail), it does not hide."""
    mb = total * 2 // 16384 + nreads + 1
    return dict(copy=mb + total // 256 + 16 * nreads + 64, units=mb // 8 + 2 * nreads + 64, trees=3 * nreads + 64,
                long=total // 8192 + nreads + 64, seq=total // 4 + 64 * nreads + 1024, xblk=mb // 4 + 4 * nreads + 64)


def needs(frames):
    c = total_census(frames)
    return {k: c["need_" + k] for k in ("copy", "units", "trees", "long", "seq", "xblk")}


def total_room(frames, extra=0):
    return sum((f.room + extra + 7) // 8 * 8 for f in frames)


@functools.lru_cache(maxsize=None)
def pad_frame(kind):
    """an ordinary read that takes nothing of the shared lists: 16 samples in one raw block"""
    s = (np.arange(16) * 3 + 500).astype(np.int16)
    buf = prezstd(_libs.oracle(), s, KINDS[kind][0])
    f = Frame(_zstd(), _libs.oracle(), kind, zf.frame_header(len(buf), True, 1) + zf.block(0, buf, last=True), 16, "pad")
    assert np.array_equal(f.expect, s) and not any(needs([f]).values())
    return f


def padded(frames, extra=0):
    """frames + as many pad reads as it takes for the batch's lists to hold what all its frames need"""
    need = needs(frames)
    npad = 0
    while True:
        caps = plan_caps(len(frames) + npad, total_room(frames, extra) + npad * ((16 + extra + 7) // 8 * 8))
        short = [k for k in need if need[k] > caps[k]]
        if not short:
            return list(frames) + [pad_frame(frames[0].kind)] * npad
        npad += max(1, max((need[k] - caps[k]) // 4 for k in short))


def check_reads(frames, back, what=""):
    for f, b in zip(frames, back):
        if f.expect is None:
            assert b is None, "%s%s: libzstd / the oracle refuse it, the device reads %d samples" % (what, f.tag, len(b))
        else:
            assert b is not None, what + f.tag + ": refused"
            assert np.array_equal(b, f.expect), what + f.tag


def on_device(f):
    """decided by the device alone: everything but a dictionary id (left to libzstd, which refuses without the dictionary)"""
    return not (f.frame[4] & 3)


@gpu
@pytest.mark.parametrize("zm", sorted(KINDS))
def test_device_reads_the_corpus(zm):
    """test 3: every corpus frame of the kind in one batch, padded so that no list of the scratch plan overflows
    (plan_caps): each read is what libzstd + the oracle make of it, no frame went to the host, and these frames hold
    every feature of FEATURES (zstd_svb_zd; the other kinds: their share).  Once more with 1000 samples more room."""
    from honours_amd import press
    lib = press.load_library()
    fs = [f for f in corpus() if f.kind == zm and on_device(f)]
    assert len(fs) >= 30
    for extra in (0, 1000):
        batch = padded(fs, extra)
        back = press.depress_batch_host(zm, [f.frame for f in batch], [f.room + extra for f in batch])
        assert lib.press_hip_zstd_host_frames() == 0
        check_reads(batch, back, "room + %d: " % extra)
    c = total_census(fs)
    want = FEATURES if zm == "zstd_svb_zd" else ["block_compressed_mid", "lit_huf_no_seq", "hdr_window_descriptor", "hdr_no_content_size"]
    assert not [k for k in want if c[k] < 1]
    assert press.load_library().press_hip_synchronize() == 0


def host_batch():
    """test 4's batch -> (frames, the number designed for the host).  Ordinary frames - this library's (the model's bytes,
    which test_zstd_frames shows to be the device's) and ZSTD_compress's - take no tree beyond their first and have no
    sequences, so the two overflowing reads cannot starve them; everything else fits (asserted against plan_caps)."""
    z = _zstd()
    oracle = _libs.oracle()
    m = ctypes.CDLL(MODEL_SO)
    m.zsm_frame_p.restype = ctypes.c_uint64
    m.zsm_frame_p.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]

    def ours(buf, plen, nk):
        a = np.frombuffer(buf, dtype=np.uint8).copy()
        out = np.zeros(len(buf) + 65536, dtype=np.uint8)
        r = m.zsm_frame_p(a.ctypes.data, len(buf), out.ctypes.data, out.size, plen, nk)
        assert r
        return out[:r].tobytes()

    def theirs(buf, level=1):
        a = np.frombuffer(buf, dtype=np.uint8).copy()
        out = np.zeros(len(buf) + len(buf) // 100 + 1024, dtype=np.uint8)
        r = z.ZSTD_compress(out.ctypes.data, out.size, a.ctypes.data, len(buf), level)
        assert not z.ZSTD_isError(r)
        return out[:r].tobytes()

    def mk(frame, room, tag):
        return Frame(z, oracle, "zstd_svb_zd", frame, room, tag)
    rng = np.random.default_rng(31)
    ordinary = []
    for k in range(60):
        n = int(rng.integers(500, 30000))
        # (this library's frames of smooth reads: RLE key blocks and Huffman blocks under one tree; ZSTD_compress's of noisy
        # ones: mostly one Huffman block without sequences)
        s = ((np.cumsum(rng.integers(-20, 21, n)) + 500) if k % 2 else rng.integers(300, 700, n)).astype(np.int16)
        buf = prezstd(oracle, s)
        f = mk(ours(buf, 4, (n + 3) // 4) if k % 2 else theirs(buf), n, "ordinary %d" % k)
        assert np.array_equal(f.expect, s)
        nd = needs([f])
        if not (nd["trees"] or nd["xblk"]):
            ordinary.append(f)
    ordinary = ordinary[:30]
    for f in ordinary:  # slots of one size, as a caller who does not know the reads' lengths lays them out (the count in the
        f.room = 150000  # stream decides); the batch's lists grow with the rooms: see the arithmetic at the end
    assert len(ordinary) == 30 and sum(int(f.tag.split()[1]) % 2 == 0 for f in ordinary) >= 10  # (even: ZSTD_compress's)
    host = []
    # two frames in one stream, the buffer split in the middle: all four mixes
    for k, (a, b) in enumerate((("ours", "ours"), ("ours", "theirs"), ("theirs", "ours"), ("theirs", "theirs"))):
        n = 9000 + 1000 * k
        s = (np.cumsum(rng.integers(-20, 21, n)) + 500).astype(np.int16)
        buf = prezstd(oracle, s)
        h = len(buf) // 2
        nk = (n + 3) // 4
        fa = ours(buf[:h], 4, nk) if a == "ours" else theirs(buf[:h])
        fb = ours(buf[h:], 1, 0) if b == "ours" else theirs(buf[h:])
        f = mk(fa + fb, n, "two frames: %s + %s" % (a, b))
        assert np.array_equal(f.expect, s)
        host.append(f)
    s = rng.integers(300, 700, 7000).astype(np.int16)
    skip = struct.pack("<II", 0x184D2A50, 5) + b"hello"
    host.append(mk(theirs(prezstd(oracle, s)) + skip, 7000, "a skippable frame behind"))
    host.append(mk(skip + ours(prezstd(oracle, s), 4, 1750), 7000, "a skippable frame in front"))
    assert np.array_equal(host[-1].expect, s) and np.array_equal(host[-2].expect, s)
    # a new tree in every flushed block: every 600 bytes another alphabet
    t = b"".join(bytes((rng.integers(0, 12, 600) ** 2 // 11 + 16 * (i % 13)).astype(np.uint8)) for i in range(330))
    s, buf = zf.samples_for_text(oracle, t)
    many_trees = mk(zf.stream_frames(z, buf, 600, dict(level=1)), len(s), "many trees")
    host.append(many_trees)
    # sequences in every 97-byte block
    s, buf = zf.samples_for_text(oracle, b"abcabcabd" * 9000)
    many_xblk = mk(zf.stream_frames(z, buf, 97, dict(level=1)), len(s), "many blocks with sequences")
    host.append(many_xblk)
    assert np.array_equal(many_xblk.expect, s)
    # refused on the host: a dictionary id; a second frame whose content does not fit the room
    n = 300
    body = struct.pack("<I", n) + bytes(75) + bytes(rng.integers(0, 8, n, dtype=np.uint8))
    host.append(mk(zf.frame_header(len(body), True, 2, dict_id=(7, 1)) + zf.block(0, body, last=True), n, "dictionary id"))
    s = rng.integers(300, 700, 20000).astype(np.int16)
    buf = prezstd(oracle, s)
    host.append(mk(theirs(buf[:100]) + theirs(buf[100:]), 2000, "two frames, the second beyond the room"))
    assert host[-1].expect is None and host[-2].expect is None
    # scattered: a fallback frame behind every third ordinary one
    frames = []
    left = list(host)
    for i, f in enumerate(ordinary):
        frames.append(f)
        if i % 3 == 2 and left:
            frames.append(left.pop(0))
    frames += left
    # ---- aimed at plan_caps
    caps = plan_caps(len(frames), total_room(frames))
    assert needs([many_trees])["trees"] > caps["trees"], (needs([many_trees]), caps)
    assert needs([many_xblk])["xblk"] > caps["xblk"], (needs([many_xblk]), caps)
    # what the ordinary frames share with the others holds all of them, however far the overflowing reads get (a read
    # that runs out of trees has opened at most one unit per tree it got)
    rest = [f for f in frames if f is not many_trees and f.census is not None]
    need = needs(rest)
    assert need["units"] + caps["trees"] + 1 <= caps["units"], (need, caps)
    mt = needs([many_trees])
    assert need["copy"] + mt["copy"] <= caps["copy"] and need["seq"] + mt["seq"] <= caps["seq"] and need["long"] + mt["long"] <= caps["long"]
    return frames, len(host)


@gpu
def test_frames_that_go_to_the_host():
    """test 4: frames the device leaves to libzstd - two frames in one stream (all four mixes of this library's and
    libzstd's), a skippable frame behind and in front, more new trees than the batch's tree list holds, more blocks with
    sequences than its block list holds, a dictionary id (None), a second frame beyond the room (None) - scattered among
    ordinary frames.  The overflowing reads have queued pieces, units and sequences by the time they give up, and the
    stream stage runs a second time for the whole batch: every read must still be libzstd's + the oracle's.
    (A read whose raw blocks above ZCOPY_INLINE = 2048 bytes outnumber cap_copy is out of reach: a read of 200 000
    samples has at most 450 004 content bytes = 219 such blocks, and cap_copy is at least 16 * nreads + 64 + total / 256.)"""
    from honours_amd import press
    lib = press.load_library()
    oracle = _libs.oracle()
    frames, nhost = host_batch()
    streams = [f.frame for f in frames]
    rooms = [f.room for f in frames]
    for again in range(2):  # (scratch and counters are reused)
        back = press.depress_batch_host("zstd_svb_zd", streams, rooms)
        assert lib.press_hip_zstd_host_frames() == nhost, again
        check_reads(frames, back, "run %d: " % again)
    good = [f.expect is not None for f in frames]
    want = [f.expect if f.expect is not None else np.zeros(f.room, dtype=np.int16) for f in frames]
    # compare-after-decode
    first_bad, out_n, nbad = press.verify_batch_host("zstd_svb_zd", streams, want)
    assert lib.press_hip_zstd_host_frames() == nhost
    assert nbad == good.count(False)
    for f, fb, k in zip(frames, first_bad, out_n):
        if f.expect is None:
            assert int(fb) == 0 and int(k) == 0xFFFFFFFF, f.tag
        else:
            assert int(fb) == press.VERIFIED and int(k) == len(f.expect), f.tag
    # digests
    crc, out_n = press.depress_crc_batch_host("zstd_svb_zd", streams, rooms)
    assert lib.press_hip_zstd_host_frames() == nhost
    for f, c, k in zip(frames, crc, out_n):
        if f.expect is None:
            assert int(c) == 0 and int(k) == 0xFFFFFFFF, f.tag
        else:
            assert int(k) == len(f.expect) and int(c) == zlib.crc32(f.expect.tobytes()), f.tag
    # recode to the inner stream
    out, sig = press.recode_batch_host("zstd_svb_zd", "svb_zd", streams, rooms, want_samples=True)
    assert lib.press_hip_zstd_host_frames() == nhost
    check_reads(frames, sig, "recode: ")
    for f, o in zip(frames, out):
        if f.expect is None:
            assert o is None, f.tag
        else:
            ret, c = oracle.press("svb_zd", f.expect)
            assert ret == 0 and o == c, f.tag
    # a batch of ordinary frames behind it: none for the host
    plain = [f for f in frames if f.tag.startswith("ordinary")]
    back = press.depress_batch_host("zstd_svb_zd", [f.frame for f in plain], [f.room for f in plain])
    assert lib.press_hip_zstd_host_frames() == 0
    check_reads(plain, back, "behind: ")
    assert lib.press_hip_synchronize() == 0


@gpu
def test_device_on_damaged_corpus_frames():
    """test 5: the damaged frames (test_sanitized_model_reads_the_damaged_frames has them through the sanitizer-built
    model) next to their undamaged originals: a read is refused or is what libzstd + the oracle make of the same bytes -
    never the original read unless libzstd says so -, the originals decode"""
    from honours_amd import press
    ds = damaged()
    frames = []
    for d, f in ds:
        frames += [d, f]
    batch = padded(frames)
    back = press.depress_batch_host("zstd_svb_zd", [f.frame for f in batch], [f.room for f in batch])
    refused = 0
    for f, b in zip(batch, back):
        if "damaged" not in f.tag:
            assert b is not None and np.array_equal(b, f.expect), f.tag
        elif b is None:
            refused += 1
        else:
            assert f.expect is not None, f.tag + ": libzstd / the oracle refuse it, the device reads %d samples" % len(b)
            assert np.array_equal(b, f.expect), f.tag
    assert refused >= 10
    assert press.load_library().press_hip_synchronize() == 0


def test_model_leaves_a_leading_skippable_frame_to_libzstd(model):
    """a stream that starts with a skippable frame is valid zstd which the reference never writes: the walk hands it to
    libzstd (W_HOST = -2) instead of refusing it; on the device: test_frames_that_go_to_the_host"""
    dec = zsm()
    f = next(f for f in corpus() if f.tag == "forged: header single fcs 2")
    skip = struct.pack("<II", 0x184D2A50, 5) + b"hello"
    assert dec(skip + f.frame, 1000)[0] == -2
    assert zf.content(_zstd(), skip + f.frame, 1000) == f.content
    assert dec(skip[:7], 1000)[0] == -1  # (cut inside the skippable frame's header: no frame at all)
