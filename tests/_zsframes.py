"""zstd frames for the device reader's tests (tests/test_zstd_reader_format.py).  CPU only.

* samples_for_text(T): any byte text as the data part of an svb-zd stream (all key bytes zero), so that what libzstd
  makes of byte texts - long and overlapping matches, short offsets, RLE tables - reaches the device as a read.
* stream_frames(): ZSTD_compressStream2 with flushes and parameters (treeless blocks, repeated tables, raw and RLE blocks
  in the middle of a frame, frames without content size, checksums).
* a forger for what libzstd does not emit: header variants, raw / RLE literals in every size format, sequence sections
  whose three tables are in RLE mode (the bit stream then holds extra bits only: no FSE encoder needed).
* census(frame): which parts of RFC 8878 a frame holds, from its headers alone, and what it takes of the batch's scratch.

Nothing here decodes a frame: expected contents come from libzstd (content()), expected samples from the oracle.
"""
import collections
import ctypes
import struct

import numpy as np

MAGIC = b"\x28\xB5\x2F\xFD"

# ---------------------------------------------------------------- byte texts as reads


def samples_for_text(oracle, text):
    """-> (int16 samples, the buffer the reference hands to ZSTD_compress): a read whose zig-zag deltas are the bytes of
    `text`.  Where the running sum would leave +-30 000 the delta is negated (another byte value: the text that counts
    is the data part the oracle makes)."""
    b = np.frombuffer(bytes(text), dtype=np.uint8).astype(np.int64)
    d = np.where(b & 1, -((b + 1) >> 1), b >> 1)
    out = np.empty(len(d), dtype=np.int64)
    acc = 0
    for i, x in enumerate(d.tolist()):
        if not -30000 <= acc + x <= 30000:
            x = -x if x != -128 else 127  # (+128 would be the two-byte value 256)
        acc += x
        out[i] = acc
    s = out.astype(np.int16)
    ret, c = oracle.press("svb_zd", s)
    assert ret == 0
    nk = (len(s) + 3) // 4
    assert not any(c[:nk]) and len(c) - nk == len(text), "the text is not the data part of its svb-zd stream"
    return s, struct.pack("<I", len(s)) + c


# ---------------------------------------------------------------- libzstd


def content(z, frame, cap):
    """what ZSTD_decompress makes of `frame` with room for cap bytes; None: refused"""
    a = np.frombuffer(frame, dtype=np.uint8).copy() if len(frame) else np.zeros(1, dtype=np.uint8)
    out = np.zeros(cap + 64, dtype=np.uint8)
    r = z.ZSTD_decompress(out.ctypes.data, cap, a.ctypes.data, len(frame))
    return None if z.ZSTD_isError(r) else out[:r].tobytes()


class _Buf(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("size", ctypes.c_size_t), ("pos", ctypes.c_size_t)]


# ZSTD_cParameter (zstd.h, stable since 1.4.0)
PARAM = {"level": 100, "windowLog": 101, "minMatch": 105, "contentSizeFlag": 200, "checksumFlag": 201}
E_FLUSH, E_END = 1, 2


def have_streaming(z):
    return all(hasattr(z, f) for f in ("ZSTD_createCCtx", "ZSTD_CCtx_setParameter", "ZSTD_compressStream2", "ZSTD_freeCCtx"))


def stream_frames(z, buf, step, params):
    """one frame of `buf` by ZSTD_compressStream2: ZSTD_e_flush every `step` bytes (None: never), ZSTD_e_end at the end"""
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    z.ZSTD_compressStream2.restype = ctypes.c_size_t
    z.ZSTD_compressStream2.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Buf), ctypes.POINTER(_Buf), ctypes.c_int]
    c = z.ZSTD_createCCtx()
    assert c
    try:
        for k, v in params.items():
            assert not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(c, PARAM[k], v)), k
        src = np.frombuffer(bytes(buf), dtype=np.uint8).copy() if len(buf) else np.zeros(1, dtype=np.uint8)
        n = len(buf)
        step = n if not step else step
        dst = np.zeros(2 * n + 8 * (n // step + 2) + 4096, dtype=np.uint8)
        o = _Buf(dst.ctypes.data, dst.size, 0)
        at = 0
        while True:
            end = min(n, at + step)
            i = _Buf(src.ctypes.data, end, at)
            op = E_END if end == n else E_FLUSH
            while True:
                r = z.ZSTD_compressStream2(c, ctypes.byref(o), ctypes.byref(i), op)
                assert not z.ZSTD_isError(r)
                if r == 0:
                    break
                assert o.pos < o.size
            assert i.pos == end
            at = end
            if at == n:
                break
        return dst[:o.pos].tobytes()
    finally:
        z.ZSTD_freeCCtx(c)


# ---------------------------------------------------------------- forged frames (RFC 8878 3.1.1)


def frame_header(size=None, single=True, fcs_bytes=1, checksum=False, dict_id=None):
    """magic + frame header.  fcs_bytes: 0 (no content size: window descriptor only), 1 (single-segment only), 2, 4, 8"""
    assert (fcs_bytes == 1) <= single and (fcs_bytes == 0) <= (not single)
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    did = {None: 0, 1: 1, 2: 2, 4: 3}[None if dict_id is None else dict_id[1]]
    h = bytes([flag << 6 | (0x20 if single else 0) | (4 if checksum else 0) | did])
    if not single:
        h += b"\x50"  # window descriptor: 1 MiB
    if dict_id is not None:
        h += dict_id[0].to_bytes(dict_id[1], "little")
    if fcs_bytes:
        h += (size - 256 if fcs_bytes == 2 else size).to_bytes(fcs_bytes, "little")
    return MAGIC + h


def block(kind, body, last=False, rle_count=None):
    """kind 0 raw (body: the bytes), 1 RLE (body: one byte, rle_count times), 2 compressed (body: the block's content)"""
    size = rle_count if kind == 1 else len(body)
    assert size <= 131072
    return (int(last) | kind << 1 | size << 3).to_bytes(3, "little") + body


def literals(kind, data, fmt):
    """raw (kind 0, data: the bytes) or RLE (kind 1, data: (byte, count)) literals section; fmt: header of 1, 2 or 3 bytes"""
    R = len(data) if kind == 0 else data[1]
    body = data if kind == 0 else bytes([data[0]])
    if fmt == 1:
        assert R < 32
        return bytes([kind | R << 3]) + body
    if fmt == 2:
        assert R < 4096
        return (kind | 1 << 2 | R << 4).to_bytes(2, "little") + body
    assert R < 1 << 20
    return (kind | 3 << 2 | R << 4).to_bytes(3, "little") + body


def seq_count(nseq, form=None):
    """Number_of_Sequences in its 1-, 2- or 3-byte form (the shortest that holds it unless told)"""
    form = form or (1 if nseq < 128 else 2 if nseq < 0x7F00 else 3)
    if form == 1:
        assert 0 < nseq < 128
        return bytes([nseq])
    if form == 2:
        assert nseq < 0x7F00
        return bytes([128 + (nseq >> 8), nseq & 255])
    assert 0x7F00 <= nseq < 0x7F00 + 65536
    return b"\xFF" + (nseq - 0x7F00).to_bytes(2, "little")


def _ll_code(c):  # -> (base, extra bits), RFC 8878 3.1.1.3.2.1.1
    if c < 16:
        return c, 0
    if c < 25:
        return [16, 18, 20, 22, 24, 28, 32, 40, 48][c - 16], [1, 1, 1, 1, 2, 2, 3, 3, 4][c - 16]
    return 1 << (c - 19), c - 19


def _ml_code(c):
    if c < 32:
        return c + 3, 0
    if c < 43:
        return ([35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99][c - 32], [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5][c - 32])
    return (1 << (c - 36)) + 3, c - 36


def sequences_rle(seqs, llc, ofc, mlc, form=None):
    """a sequences section whose three tables are in RLE mode (one code each: llc, ofc, mlc).  seqs: (ll, ml, offset
    value) per sequence, each within what its code reaches - offset value = 2^ofc + extra, RFC 8878 3.1.1.3.2.1.1.
    The bit stream holds the extra bits only (an RLE table's state takes none), read backwards: offset, match length,
    literal length of the first sequence on top."""
    lb, lx = _ll_code(llc)
    mb, mx = _ml_code(mlc)
    ob = 1 << ofc
    acc = nbits = 0
    for ll, ml, ofv in seqs:
        for v, base, bits in ((ofv, ob, ofc), (ml, mb, mx), (ll, lb, lx)):
            assert 0 <= v - base < (1 << bits), (v, base, bits)
            acc = acc << bits | (v - base)
            nbits += bits
    acc |= 1 << nbits  # the end mark
    return seq_count(len(seqs), form) + bytes([0x54, llc, ofc, mlc]) + acc.to_bytes(nbits // 8 + 1, "little")


def offsets_history(seqs, rep=(1, 4, 8)):
    """the offsets the sequences (ll, ml, offset value) stand for, and the repeat offsets behind them (RFC 8878 3.1.1.5)
    -> ([offset], rep, sequences that took rep[0] - 1)"""
    rep = list(rep)
    out, minus1 = [], 0
    for ll, _, ofv in seqs:
        if ofv > 3:
            off = ofv - 3
            rep = [off, rep[0], rep[1]]
        else:
            idx = ofv - (1 if ll else 0)
            if idx == 0:
                off = rep[0]
            else:
                off = rep[0] - 1 if idx == 3 else rep[idx]
                minus1 += idx == 3
                rep = [off, rep[0]] + [rep[1] if idx != 1 else rep[2]]
        assert off > 0
        out.append(off)
    return out, tuple(rep), minus1


def svb_head(n):
    """the blocks in front of an svb-zd buffer's data: a raw block with the count, an RLE block with the zero key bytes"""
    return block(0, struct.pack("<I", n)) + block(1, b"\0", rle_count=(n + 3) // 4)


# ---------------------------------------------------------------- census


def census(frame, spans=None):
    """Counter of what a frame holds, read off its headers (no entropy decoding): frame header variants, block types,
    literals types with / without sequences, tree description kinds, stream counts, sequence count forms, table modes,
    `long_with_seq`; the repeat-offset branches where all three tables are in RLE mode and no extra bits stand between
    the offsets' (so the stream can be read without tables).  `need_*`: what the frame takes of the batch's shared lists
    on the device (blocks with sequences, sequences, trees beyond the first, Huffman units, long blocks, copy slots).
    spans (a list): gets ("block", offset of a block header), ("tree" / "seq", first, one past the last byte) of the tree
    descriptions (as far as a description can reach: its true end takes decoding) and the sequences sections."""
    c = collections.Counter()
    f = frame
    if f[1:4] == b"\x2A\x4D\x18" and f[0] & 0xF0 == 0x50:  # a skippable frame: the device walks no further
        c["skippable_first"] += 1
        return c
    assert f[:4] == MAGIC  # (of several frames in one stream only the first is counted: the device walks no further either)
    fhd = f[4]
    single = bool(fhd & 0x20)
    at = 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3]
    fcs = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    c["hdr_single_segment" if single else "hdr_window_descriptor"] += 1
    c["hdr_content_size_%d" % fcs if fcs else "hdr_no_content_size"] += 1
    c["hdr_checksum" if fhd & 4 else "hdr_no_checksum"] += 1
    if fhd & 3:
        c["hdr_dictionary_id"] += 1
    at += fcs
    nblocks = trees = copies = in_unit = 0
    units_open = False
    rep = (1, 4, 8)
    rep_known = True
    while True:
        h = int.from_bytes(f[at:at + 3], "little")
        if spans is not None:
            spans.append(("block", at))
        at += 3
        last, kind, bs = h & 1, (h >> 1) & 3, h >> 3
        assert kind != 3
        c[("block_raw", "block_rle", "block_compressed")[kind]] += 1
        if nblocks and not last:
            c[("block_raw_mid", "block_rle_mid", "block_compressed_mid")[kind]] += 1
        nblocks += 1
        if kind == 0:
            copies += bs > 2048
            if last and bs == 0:
                c["block_empty_last"] += 1
            at += bs
        elif kind == 1:
            at += 1
        else:
            end = at + bs
            b0 = f[at]
            lt, sf = b0 & 3, (b0 >> 2) & 3
            if lt < 2:
                lh = 2 if sf == 1 else 3 if sf == 3 else 1
                v = int.from_bytes(f[at:at + lh], "little")
                R = v >> 3 if lh == 1 else v >> 4
                cs = R if lt == 0 else 1
                c["lit_hdr_%s_%d" % (("raw", "rle")[lt], lh)] += 1
            else:
                lh = 3 if sf < 2 else 4 if sf == 2 else 5
                kb = 10 if sf < 2 else 14 if sf == 2 else 18
                v = int.from_bytes(f[at:at + lh], "little")
                R = (v >> 4) & ((1 << kb) - 1)
                cs = (v >> (4 + kb)) & ((1 << kb) - 1)
                c["huf_one_stream" if sf == 0 else "huf_four_streams"] += 1
                if lt == 2:
                    c["tree_fse" if f[at + lh] < 128 else "tree_direct"] += 1
                    trees += 1
                    units_open = False
                    if spans is not None:
                        hb = f[at + lh]
                        spans.append(("tree", at + lh, at + lh + 1 + (hb if hb < 128 else (hb - 126) // 2)))
            sq = at + lh + cs
            nseq, form = f[sq], 1
            if nseq >= 128:
                if nseq < 255:
                    nseq, form = ((nseq - 128) << 8) + f[sq + 1], 2
                else:
                    nseq, form = f[sq + 1] + (f[sq + 2] << 8) + 0x7F00, 3
            name = ("lit_raw", "lit_rle", "lit_huf", "lit_treeless")[lt]
            c[name + ("_with_seq" if nseq else "_no_seq")] += 1
            if lt == 0:
                copies += R > 2048
            if lt >= 2 and R:
                if sf and R >= 16385:
                    c["long_block"] += 1
                    c["need_long"] += 1
                    if nseq:
                        c["long_with_seq"] += 1
                else:
                    # (a unit holds up to 8 blocks of one tree: counted as if every tree and every ninth block opened one)
                    if not units_open or in_unit == 8:
                        c["need_units"] += 1
                        in_unit = 0
                        units_open = True
                    in_unit += 1
            if nseq:
                if spans is not None:
                    spans.append(("seq", sq, end))
                c["seq_count_%d_byte" % form] += 1
                c["need_xblk"] += 1
                c["need_seq"] += nseq
                modes = f[sq + form]
                m3 = [(modes >> s) & 3 for s in (6, 4, 2)]
                for which, m in zip(("ll", "of", "ml"), m3):
                    c["%s_mode_%s" % (which, ("predefined", "rle", "fse", "repeat")[m])] += 1
                q = sq + form + 1
                if m3 == [1, 1, 1] and rep_known and _ll_code(f[q])[1] == 0 and _ml_code(f[q + 2])[1] == 0:
                    # extra bits of the offsets only: the stream reads without tables
                    llc, ofc, mlc = f[q], f[q + 1], f[q + 2]
                    bits = int.from_bytes(f[q + 3:end], "little")
                    nb = bits.bit_length() - 1
                    assert nb == ofc * nseq
                    seqs = [(llc, mlc + 3, (1 << ofc) + ((bits >> (nb - ofc * (i + 1))) & ((1 << ofc) - 1))) for i in range(nseq)]
                    for ll, _, ofv in seqs:
                        if ofv <= 3:
                            idx = ofv - (1 if ll else 0)
                            c[("rep_offset_0", "rep_offset_1", "rep_offset_2", "rep_offset_0_minus_1")[idx]] += 1
                        else:
                            c["new_offset"] += 1
                    _, rep, _ = offsets_history(seqs, rep)
                else:
                    rep_known = False
            at = end
        if last:
            break
    c["need_trees"] = max(0, trees - 1)
    c["need_copy"] = (copies + 7) // 8 * 8  # a walking wave takes copy slots eight at a time
    return c
