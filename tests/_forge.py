"""Forged exception-family streams: the corpus of tests/test_forged_oracle.py (CPU) and
tests/test_forged_sections.py (GPU).

Twelve methods share the exception-section decoder: vbe21 / vbbe21 / vbsbe21 / vbsse21 plain, behind the static
Huffman coder and behind the range coders, and ex-zd.  Every stream here is assembled field by field from a
description of a read (Spec), then one field is forged.  A case carries the name of its kind and the verdict its
builder intends - "refused", or "accepted" with the samples - worked out here in Python, not taken from a decoder.
DESIGN.md 6.0.20 is the definition the verdicts follow.

``cases_for(method, oracle)`` is the corpus of one method (the oracle only supplies the Huffman code table and the
range coders' payloads); ``expected_kinds(method)`` is the list of kinds the method must have, from the table KINDS.

Nothing here touches a GPU.
"""
import ctypes
import struct

import numpy as np

import _libs

M32 = 0xFFFFFFFF
REFUSED, ACCEPTED = "refused", "accepted"

# method -> (section format, what carries the one-byte values)
LAYOUT = {
    "vbe21_zd": ("vbe21", "plain"), "vbbe21_zd": ("vbbe21", "plain"), "vbsbe21_zd": ("vbsbe21", "plain"),
    "vbsse21_zd": ("vbsse21", "plain"), "hasgam_vbsse21_zdq": ("exzd", "plain"),
    "shuffman_vbe21_zd": ("vbe21", "huff"), "shuffman_vbbe21_zd": ("vbbe21", "huff"),
    "shuffman_vbsbe21_zd": ("vbsbe21", "huff"), "shuffman_vbsse21_zd": ("vbsse21", "huff"),
    "rc_vbe21_zd": ("vbe21", "rc"), "rcc_vbe21_zd": ("vbe21", "rc"), "rccm_vbbe21_zd": ("vbbe21", "rc"),
}
METHODS = tuple(LAYOUT)
FORMATS = ("vbe21", "vbbe21", "vbsbe21", "vbsse21", "exzd")
DELTA = ("vbbe21", "vbsbe21", "vbsse21", "exzd")
SVB_POS = ("vbsbe21", "vbsse21", "exzd")          # positions as an svb32 block
BIT_VAL = ("vbbe21", "vbsbe21")                   # values bit-packed
SVB_VAL = ("vbsse21", "exzd")                     # values as an svb16 / svb32 block
ALL_F, ALL_C = FORMATS, ("plain", "huff", "rc")
ROOMS = (9, 65, 100, 2049)
BIG = 32768 + 9                                   # a chunk and nine samples

# kind (case names are "<kind>" or "<kind>-<variant>") -> (formats, carriers) it exists for
KINDS = {
    # lengths
    "len": (ALL_F, ALL_C),                        # every stream length 0 .. hdr + 3
    "list-short": (("vbe21",), ALL_C),
    "nex1-short": (DELTA, ALL_C),
    "lp-past-1": (DELTA, ALL_C), "lv-past-1": (DELTA, ALL_C), "lp-fffffff8": (DELTA, ALL_C),
    "pblock-short-1": (DELTA, ALL_C), "vblock-short-1": (DELTA, ALL_C),
    "pblock-long-1": (DELTA, ALL_C), "vblock-long-1": (DELTA, ALL_C),
    "pkeys-1-more": (SVB_POS, ALL_C), "vkeys-1-more": (SVB_VAL, ALL_C),
    # counts
    "nex-room-1-nolow": (ALL_F, ("plain", "rc")),  # (a Huffman stream that codes nothing is outside the decoder's domain)
    "nex-room": (ALL_F, ALL_C), "nex-ffffffff": (ALL_F, ALL_C),
    "count-eq-room": (ALL_F, ALL_C),
    "count-room+1": (ALL_F, ("plain", "huff")),    # (a range coder's count of one-byte values is the room's)
    "short-stream": (ALL_F, ("plain", "huff")),
    # width-0 blocks
    "width0-101": (("vbbe21",), ("plain", "rc")), "width0-101-low50": (("vbbe21",), ALL_C),
    # bit widths
    "pbits-wider": (("vbbe21",), ALL_C), "pbits-32": (("vbbe21",), ALL_C), "pbits-33": (("vbbe21",), ALL_C),
    "pbits-255": (("vbbe21",), ALL_C),
    "vbits-wider": (BIT_VAL, ALL_C), "vbits-32": (BIT_VAL, ALL_C), "vbits-33": (BIT_VAL, ALL_C), "vbits-255": (BIT_VAL, ALL_C),
    # non-minimal svb byte lengths
    "psvb-nonminimal": (SVB_POS, ALL_C), "vsvb-nonminimal": (SVB_VAL, ALL_C),
    # positions
    "pos-last-n-2": (ALL_F, ALL_C),
    "pos-n-1": (ALL_F, ("plain", "huff")), "pos-mid": (ALL_F, ("plain", "huff")), "pos-room-2": (ALL_F, ("plain", "huff")),
    "pos-room-1": (ALL_F, ALL_C), "pos-ffffffff": (ALL_F, ALL_C),
    # order
    "order-equal": (("vbe21",), ALL_C), "order-decreasing": (("vbe21",), ALL_C),
    "delta-ffffffff": (DELTA, ALL_C), "sum-wraps": (DELTA, ALL_C),
    # the carries between rounds of 64 exceptions
    "carry-good": (ALL_F, ALL_C), "carry": (ALL_F, ALL_C),
    # values
    "val-wraps-16": (DELTA, ALL_C),
    # ex-zd header
    "ver-1": (("exzd",), ALL_C), "n-0": (("exzd",), ALL_C), "n-room+1": (("exzd",), ALL_C),
    "n-high-word": (("exzd",), ALL_C), "q-6": (("exzd",), ALL_C), "n-below-count": (("exzd",), ALL_C),
    "n-above-count": (("exzd",), ALL_C),
    # static Huffman: the symbol count in front of the payload
    "huff-count-1": (ALL_F, ("huff",)), "huff-count-half": (ALL_F, ("huff",)), "huff-count-1-reachable": (ALL_F, ("huff",)),
    "huff-count+1": (ALL_F, ("huff",)), "huff-count+1-full-room": (ALL_F, ("huff",)),
    # ... and a payload that ends early: the decoder delivers what is there
    "huff-payload-cut": (ALL_F, ("huff",)), "huff-payload-cut-reachable": (ALL_F, ("huff",)),
    # a read of 32768 + 9 samples
    "big-good": (ALL_F, ALL_C), "big-tail-unreachable": (ALL_F, ("plain", "huff")), "big-pos-room-1": (ALL_F, ALL_C),
}


def kind_of(name):
    """the kind of a case name: the longest key of KINDS the name is, or begins with in front of a "-" """
    return max((k for k in KINDS if name == k or name.startswith(k + "-")), key=len)


def expected_kinds(method):
    fmt, carrier = LAYOUT[method]
    return sorted(k for k, (fs, cs) in KINDS.items() if fmt in fs and carrier in cs)


# ------------------------------------------------------------------ fields

def u16(v):
    return struct.pack("<H", v & 0xFFFF)


def u32(v):
    return struct.pack("<I", v & M32)


def bit_block(vals, bits=None):
    """width byte, then the low `bits` bits of every value, most significant bit first (minimal width by default)"""
    if bits is None:
        bits = max(vals).bit_length() if vals else 0
    acc = nb = 0
    for v in vals:
        acc = (acc << bits) | (v & ((1 << bits) - 1))
        nb += bits
    pad = -nb % 8
    return bytes([bits]) + ((acc << pad).to_bytes((nb + pad) // 8, "big") if nb else b"")


def svb32_block(vals, codes=None):
    """ceil(n / 4) key bytes (2 bits per value: its byte count - 1), then the values' bytes, little endian"""
    if codes is None:
        codes = [max((v.bit_length() + 7) // 8, 1) - 1 for v in vals]
    keys = bytearray((len(vals) + 3) // 4)
    data = b""
    for i, (v, c) in enumerate(zip(vals, codes)):
        keys[i >> 2] |= c << (2 * (i & 3))
        data += v.to_bytes(4, "little")[:c + 1]
    return bytes(keys) + data


def svb16_block(vals, wide=None):
    """ceil(n / 8) key bytes (one bit per value: two bytes), then the values"""
    if wide is None:
        wide = [v > 255 for v in vals]
    keys = bytearray((len(vals) + 7) // 8)
    data = b""
    for i, (v, w) in enumerate(zip(vals, wide)):
        if w:
            keys[i >> 3] |= 1 << (i & 7)
        data += v.to_bytes(2, "little")[:2 if w else 1]
    return bytes(keys) + data


def huff_bits(lows, table):
    return sum(table[x][0] for x in lows)


def huff_payload(lows, table):
    """the codes bit by bit, every byte filled from bit 0 upwards, the last one zero padded"""
    acc = nb = 0
    for x in lows:
        ln, bits = table[x]
        acc |= bits << nb
        nb += ln
    return acc.to_bytes((nb + 7) // 8, "little")


class Spec:
    """A well-formed read: zd[0], exceptions at the sorted positions `pos` of zd[1..], one-byte values elsewhere.
    z: the exceptions' 16-bit values; stored: what the section holds of them (z itself for vbe21, z - 256 elsewhere -
    a case may store a value that only gives z after the 16-bit wrap)."""

    def __init__(self, fmt, pos, nlow, zd0=7, q=0, z=None, stored=None, lows=None):
        self.fmt, self.pos, self.zd0, self.q = fmt, list(pos), zd0, q
        nex = len(self.pos)
        self.z = [300 + 211 * ((nex - 1 - k) % 7) for k in range(nex)] if z is None else list(z)
        self.stored = ([v if fmt == "vbe21" else v - 256 for v in self.z]) if stored is None else list(stored)
        self.lows = [(3 * i + i // 5) % 5 for i in range(nlow)] if lows is None else list(lows)
        self.n = 1 + len(self.lows) + nex

    def zd(self):
        out = np.zeros(self.n, dtype=np.int64)
        out[0] = self.zd0
        isex = np.zeros(self.n - 1, dtype=bool)
        if self.pos:
            assert self.pos == sorted(set(self.pos)) and self.pos[-1] < self.n - 1, "a Spec is well formed"
            isex[self.pos] = True
        body = out[1:]
        body[isex] = self.z
        body[~isex] = self.lows
        return out

    def samples(self, count=None):
        z = self.zd()[:count]
        d = (z >> 1) ^ -(z & 1)
        return ((np.cumsum(d) & 0xFFFF) << self.q).astype(np.uint16).view(np.int16)


def section(fmt, pos, stored, pos_bits=None, val_bits=None, pos_codes=None, val_codes=None):
    """-> [[field name, bytes], ...] of "u32 nex || section" for any position list (mod 2^32)"""
    nex = len(pos)
    parts = [["nex", u32(nex)]]
    if nex == 0:
        return parts
    if fmt == "vbe21":
        return parts + [["plist", b"".join(u32(p) for p in pos)], ["vlist", b"".join(u16(v) for v in stored)]]
    if nex == 1:
        return parts + [["p0", u32(pos[0])], ["v0", u32(stored[0]) if fmt == "exzd" else u16(stored[0])]]
    d = [pos[0] & M32] + [(pos[i] - pos[i - 1] - 1) & M32 for i in range(1, nex)]
    pb = bit_block(d, pos_bits) if fmt == "vbbe21" else svb32_block(d, pos_codes)
    if fmt == "exzd":
        vb = svb32_block(stored, val_codes)
    elif fmt == "vbsse21":
        vb = svb16_block(stored, val_codes)
    else:
        vb = bit_block(stored, val_bits)
    return parts + [["lp", u32(len(pb))], ["pblock", pb], ["lv", u32(len(vb))], ["vblock", vb]]


class Case:
    def __init__(self, name, method, room, stream, verdict, samples=None, canonical=None):
        self.name, self.method, self.room, self.stream, self.verdict = name, method, int(room), bytes(stream), verdict
        self.kind = kind_of(name)
        self.samples = samples
        self.canonical = canonical   # the read whose oracle stream these bytes must be, where the encoding is the minimal one
        assert (verdict == ACCEPTED) == (samples is not None)


class Forge:
    """the corpus of one method"""

    def __init__(self, method, oracle):
        self.m, self.oracle = method, oracle
        self.fmt, self.carrier = LAYOUT[method]
        self.hdr = 12 if self.fmt == "exzd" else 2
        self.table = oracle.table() if self.carrier == "huff" else None
        self.cases = []

    # -------------------------------------------------------------- assembling

    def spec(self, pos, nlow, **kw):
        if self.fmt == "exzd":
            kw.setdefault("q", 1)
        return Spec(self.fmt, pos, nlow, **kw)

    def header(self, sp, hdr_n=None):
        if self.fmt == "exzd":
            return [["ver", b"\0"], ["n", struct.pack("<Q", sp.n if hdr_n is None else hdr_n)], ["q", bytes([sp.q])],
                    ["zd0", u16(sp.zd0)]]
        return [["zd0", u16(sp.zd0)]]

    def payload(self, sp):
        """the one-byte values of the well-formed read sp, as this method carries them"""
        if self.carrier == "plain":
            return [["low", bytes(sp.lows)]]
        if self.carrier == "huff":
            return [["hcount", struct.pack(">I", len(sp.lows))], ["hpay", huff_payload(sp.lows, self.table)]]
        # range coders: the oracle's coder over the one-byte values
        enc = getattr(self.oracle.lib, {"rc_vbe21_zd": "po_rcs_encode", "rcc_vbe21_zd": "po_rccs_encode",
                                        "rccm_vbbe21_zd": "po_rcms_encode"}[self.m])
        enc.restype = ctypes.c_uint64
        enc.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        src = np.array(sp.lows, dtype=np.uint8)
        dst = np.zeros(2 * src.size + 256, dtype=np.uint8)
        return [["rc", dst[:enc(src.ctypes.data, src.size, dst.ctypes.data)].tobytes()]]

    def parts(self, sp, pos=None, stored=None, hdr_n=None, **sec):
        """the stream of sp as fields; pos / stored: a forged list in the section, the rest of the stream sp's"""
        return (self.header(sp, hdr_n) + section(self.fmt, sp.pos if pos is None else pos,
                                                 sp.stored if stored is None else stored, **sec) + self.payload(sp))

    @staticmethod
    def join(parts, **forged):
        names = [n for n, _ in parts]
        assert all(k in names for k in forged), (names, list(forged))
        return b"".join(forged.get(n, b) for n, b in parts)

    @staticmethod
    def behind(parts, name):
        """bytes of the stream behind field `name`"""
        names = [n for n, _ in parts]
        return sum(len(b) for _, b in parts[names.index(name) + 1:])

    def add(self, name, room, stream, verdict, samples=None, canonical=None):
        if verdict == ACCEPTED and self.carrier == "rc":
            assert not _libs.rc_stored_raw(self.m, stream, room), (self.m, name)  # outside the coder's lossless domain
        self.cases.append(Case(name, self.m, room, stream, verdict, samples, canonical))

    def ok(self, name, room, sp, parts=None, count=None, canonical=False, **forged):
        parts = self.parts(sp) if parts is None else parts
        s = sp.samples(count)
        self.add(name, room, self.join(parts, **forged), ACCEPTED, s, s if canonical else None)

    def no(self, name, room, parts, **forged):
        self.add(name, room, self.join(parts, **forged), REFUSED)

    # -------------------------------------------------------------- the kinds

    def base(self, room, nex=3, n=None, last=None):
        """a read of n (default: room) samples: exceptions at 1, 4, .. and the last one at `last` (default n - 2)"""
        n = room if n is None else n
        pos = [1, 4, 6][:nex - 1] + [n - 2 if last is None else last]
        return self.spec(pos, n - 1 - nex)

    def build(self):
        rc, huff, fmt = self.carrier == "rc", self.carrier == "huff", self.fmt
        delta = fmt in DELTA
        rooms = ROOMS[1:] if rc else ROOMS
        small = rooms[0]
        # ---- lengths
        sp = self.base(small)
        whole = self.join(self.parts(sp))
        for k in range(self.hdr + 4):
            self.no("len-%d" % k, small, [["s", whole[:k]]])
        if fmt == "vbe21":
            p = self.parts(sp)
            k = [n for n, _ in p].index("vlist")
            self.no("list-short", small, p[:k + 1], vlist=p[k][1][:-1])
        if delta:
            s1 = self.base(small, nex=1)
            p = self.parts(s1)
            names = [n for n, _ in p]
            k = names.index("v0")
            self.no("nex1-short", small, p[:k + 1], v0=p[k][1][:-1])
            sp = self.base(100)
            p = self.parts(sp)
            d = dict(p)
            self.no("lp-past-1", 100, p, lp=u32(self.behind(p, "lp") + 1))
            self.no("lv-past-1", 100, p, lv=u32(self.behind(p, "lv") + 1))
            self.no("lp-fffffff8", 100, p, lp=u32(0xFFFFFFF8))
            self.no("pblock-short-1", 100, p, lp=u32(len(d["pblock"]) - 1), pblock=d["pblock"][:-1])
            self.no("vblock-short-1", 100, p, lv=u32(len(d["vblock"]) - 1), vblock=d["vblock"][:-1])
            self.ok("pblock-long-1", 100, sp, p, lp=u32(len(d["pblock"]) + 1), pblock=d["pblock"] + b"\xEE")
            self.ok("vblock-long-1", 100, sp, p, lv=u32(len(d["vblock"]) + 1), vblock=d["vblock"] + b"\xEE")
            nex = len(sp.pos)
            if fmt in SVB_POS:  # the last position delta announces one byte more: the data is one byte short of it
                b = bytearray(d["pblock"])
                code = (b[(nex - 1) >> 2] >> (2 * ((nex - 1) & 3))) & 3
                assert code < 3
                b[(nex - 1) >> 2] += 1 << (2 * ((nex - 1) & 3))
                self.no("pkeys-1-more", 100, p, pblock=bytes(b))
            if fmt in SVB_VAL:
                b = bytearray(d["vblock"])
                if fmt == "exzd":
                    assert (b[(nex - 1) >> 2] >> (2 * ((nex - 1) & 3))) & 3 < 3
                    b[(nex - 1) >> 2] += 1 << (2 * ((nex - 1) & 3))
                else:
                    assert not (b[(nex - 1) >> 3] >> ((nex - 1) & 7)) & 1
                    b[(nex - 1) >> 3] |= 1 << ((nex - 1) & 7)
                self.no("vkeys-1-more", 100, p, vblock=bytes(b))
        # ---- counts
        for room in rooms:
            if not huff:
                self.ok("nex-room-1-nolow-room%d" % room, room, self.spec(range(room - 1), 0), canonical=room <= 100)
            # `room` exceptions, listed in full: the count is what is wrong with this stream
            full = self.spec(range(room - 1), 1 if huff else 0)
            self.no("nex-room-room%d" % room, room, self.parts(full, pos=list(range(room)), stored=full.stored + full.stored[:1]))
            sp = self.base(room)
            self.no("nex-ffffffff-room%d" % room, room, self.parts(sp), nex=u32(M32))
            self.ok("count-eq-room-room%d" % room, room, sp, canonical=True)
            if not rc:
                early = self.spec([1, 4, 6], room - 4)  # every position inside a room one sample smaller
                self.no("count-room+1-room%d" % (room - 1), room - 1, self.parts(early))
                self.ok("short-stream-room%d" % (room + 11), room + 11, sp)
        # ---- two blocks of width 0 (s[i] = 128 i: every delta is the exception 256, every position delta 0)
        if fmt == "vbbe21":
            if not huff:
                w0 = Spec(fmt, range(100), 0, zd0=0, z=[256] * 100)
                assert np.array_equal(w0.samples(), (128 * np.arange(101)).astype(np.int16))
                if self.carrier == "plain":
                    assert self.join(self.parts(w0)) == bytes.fromhex("0000" "64000000" "01000000" "00" "01000000" "00")
                self.ok("width0-101", 101, w0, canonical=True)
            self.ok("width0-101-low50", 151, Spec(fmt, range(100), 50, zd0=0, z=[256] * 100), canonical=True)
        # ---- bit widths
        sp = self.base(100)
        if fmt == "vbbe21":
            need = max(sp.pos[0], *(b - a - 1 for a, b in zip(sp.pos, sp.pos[1:]))).bit_length()
            self.ok("pbits-wider", 100, sp, self.parts(sp, pos_bits=need + 3))
            self.ok("pbits-32", 100, sp, self.parts(sp, pos_bits=32))
            self.no("pbits-33", 100, self.parts(sp, pos_bits=33))
            self.no("pbits-255", 100, self.parts(sp, pos_bits=255))
        if fmt in BIT_VAL:
            need = max(sp.stored).bit_length()
            self.ok("vbits-wider", 100, sp, self.parts(sp, val_bits=need + 3))
            self.ok("vbits-32", 100, sp, self.parts(sp, val_bits=32))
            self.no("vbits-33", 100, self.parts(sp, val_bits=33))
            self.no("vbits-255", 100, self.parts(sp, val_bits=255))
        # ---- svb values in more bytes than they need
        if fmt in SVB_POS:
            self.ok("psvb-nonminimal", 100, sp, self.parts(sp, pos_codes=[3, 1, 2]))
        if fmt in SVB_VAL:
            self.ok("vsvb-nonminimal", 100, sp, self.parts(sp, val_codes=[3, 2, 3] if fmt == "exzd" else [True] * 3))
        # ---- positions: the last one at n - 2 (the read's last sample), then where no sample reaches
        for nex in (1, 3):
            tag = "-nex%d" % nex
            self.ok("pos-last-n-2" + tag, 100, self.base(100, nex), canonical=True)
            if not rc:
                # a read of 80 samples in a room of 100: one-byte values run out in front of the position
                sp = self.base(100, nex, n=80)
                for name, last in (("pos-n-1", 79), ("pos-mid", 85), ("pos-room-2", 98)):
                    self.no(name + tag, 100, self.parts(sp, pos=sp.pos[:-1] + [last]))
            sp = self.base(100, nex)
            self.no("pos-room-1" + tag, 100, self.parts(sp, pos=sp.pos[:-1] + [99]))
            self.no("pos-ffffffff" + tag, 100, self.parts(sp, pos=sp.pos[:-1] + [M32]))
        # ---- order
        sp = self.spec([10, 15, 20], 96)
        for name, pos in (("order-equal", [10, 10, 20]), ("order-decreasing", [20, 10, 30])):
            if delta:  # the same lists as deltas: 0xFFFFFFFF, and a running sum that wraps 2^32
                name = {"order-equal": "delta-ffffffff", "order-decreasing": "sum-wraps"}[name]
            self.no(name, 100, self.parts(sp, pos=pos, pos_bits=32 if fmt == "vbbe21" else None))
        # ---- 130 exceptions: three rounds of 64, the offending element on either side of a round's edge
        good = [3 * k + 1 for k in range(130)]
        sp = self.spec(good, 2048 - 130)
        self.ok("carry-good", 2049, sp, canonical=True)
        for k in (0, 63, 64, 65, 129):
            pos = list(good)
            pos[k] = pos[k - 1] if k else M32  # equal to its neighbour in front; element 0: beyond every room
            self.no("carry-%d" % k, 2049, self.parts(sp, pos=pos))
        # ---- value + 256 wraps 16 bits
        if delta:
            for nex in (1, 3):
                z = [0xF0] + [300] * (nex - 1)
                st = [0x1FFF0 if fmt == "exzd" else 0xFFF0] + [44] * (nex - 1)
                b = self.base(100, nex)
                self.ok("val-wraps-16-nex%d" % nex, 100, self.spec(b.pos, len(b.lows), z=z, stored=st))
        # ---- the ex-zd header
        if fmt == "exzd":
            sp = self.base(100)
            p = self.parts(sp)
            self.no("ver-1", 100, p, ver=b"\1")
            self.no("n-0", 100, p, n=struct.pack("<Q", 0))
            self.no("n-room+1", 100, p, n=struct.pack("<Q", 101))
            self.no("n-high-word", 100, p, n=struct.pack("<Q", 100 + (1 << 32)))
            self.no("q-6", 100, p, q=b"\6")
            sp = self.base(100, n=80)
            self.no("n-below-count", 100, self.parts(sp, hdr_n=79))
            self.ok("n-above-count", 100, sp, self.parts(sp, hdr_n=90))
        # ---- static Huffman: the symbol count
        if huff:
            sp = self.base(100)
            nlow = len(sp.lows)
            p = self.parts(sp)
            self.no("huff-count-1", 100, p, hcount=struct.pack(">I", nlow - 1))      # the last exception: out of reach
            self.no("huff-count-half", 100, p, hcount=struct.pack(">I", nlow // 2))
            early = self.spec([1, 4, 6], 96)
            self.ok("huff-count-1-reachable", 100, early, count=99, hcount=struct.pack(">I", 95))
            # one symbol more than the payload holds: the decoder delivers what is there (a payload that ends on a
            # byte's edge has no padding bits that could be one more code)
            full = None
            for tail in range(20 ** 3):
                t = [tail // 400, tail // 20 % 20, tail % 20]
                cand = self.spec([1, 4, 88], 87, lows=[(3 * i + i // 5) % 5 for i in range(84)] + t)
                if huff_bits(cand.lows, self.table) % 8 == 0:
                    full = cand
                    break
            assert full is not None and full.n == 91
            self.ok("huff-count+1", 100, full, hcount=struct.pack(">I", 88))
            # ... but an announced count that does not fit the room with the exceptions is refused
            self.no("huff-count+1-full-room", 91, self.parts(full), hcount=struct.pack(">I", 88))
            # half the payload: about half the values arrive, the last exception is beyond them - or, with every
            # exception in front, the read ends early
            sp = self.base(100)
            p = self.parts(sp)
            self.no("huff-payload-cut", 100, p, hpay=dict(p)["hpay"][:len(dict(p)["hpay"]) // 2])
            lows = [(5 * i) % 3 for i in range(96)]           # 4-bit codes throughout: 48 bytes, 20 of them hold 40 values
            assert {self.table[x][0] for x in lows} == {4}
            early = self.spec([1, 4, 6], 96, lows=lows)
            p = self.parts(early)
            self.ok("huff-payload-cut-reachable", 100, early, p, count=1 + 3 + 40, hpay=dict(p)["hpay"][:20])
        # ---- 32768 + 9 samples: positions on a wave quarter's and a chunk's edge, the unreachable tail behind them
        pos = [8190, 8191, 8192, 16383, 32766, 32767, 32768, BIG - 2]
        sp = self.spec(pos, BIG - 1 - len(pos))
        self.ok("big-good", BIG, sp, canonical=True)
        if not rc:
            self.no("big-tail-unreachable", 32768 + 65, self.parts(sp, pos=pos[:-1] + [BIG - 1]))
        self.no("big-pos-room-1", BIG, self.parts(sp, pos=pos[:-1] + [BIG - 1]))
        return self.cases


def good_reads(oracle, m):
    """four well-formed reads of m in rooms of exactly their size -> [(name, stream, room)]"""
    import _layouts as L
    rng = np.random.default_rng(77)
    out = []
    for n in (100, 2049, 333, 700):
        s = L._walk(rng, n, 0.05, lo=-3, hi=4)  # (small deltas: a range coder stores what it cannot shrink raw)
        ret, st = oracle.press(m, s, cap=L.slot_of(oracle.bound, m, n))
        assert ret == 0, (m, n)
        assert not (m in _libs.RC_FAMILY and _libs.rc_stored_raw(m, st, n)), (m, n)
        verdict, back = L.expect_depress(oracle, m, s, st, n)
        assert verdict == "ok" and np.array_equal(back, s), (m, n)
        out.append(("good-%d" % n, st, n))
    return out


def interleaved(oracle, m):
    """good, forged, good, forged, .. good -> (the good reads, [(name, stream, room)])"""
    good = good_reads(oracle, m)
    items = [good[0]]
    for k, c in enumerate(cases_for(m, oracle)):
        items.append((c.name, c.stream, c.room))
        items.append(good[(k + 1) % len(good)])
    return good, items


_corpus = {}


def cases_for(method, oracle):
    if method not in _corpus:
        _corpus[method] = Forge(method, oracle).build()
    return _corpus[method]


def fnv1a32_samples(s):
    return _libs.fnv1a32(np.ascontiguousarray(s, dtype=np.int16).tobytes())


def write_corpus(path, cases):
    """the file oracle/forged_check.c reads"""
    with open(path, "wb") as f:
        f.write(b"FRG1" + u32(len(cases)))
        for c in cases:
            f.write(u32(_libs.METHODS[c.method]) + u32(c.room) + u32(len(c.stream)) + c.stream)
