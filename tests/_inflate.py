"""Serial model of the device's zlib reader for BLOW5 records (include/press_hip.h section 2zb), and a forge that writes
zlib streams from explicit blocks - the cases zlib itself never writes, and the malformed ones.  Nothing here is
imported by the product package.

inflate(stream, room=None) -> (status, bytes or None, out_len or None) classifies a stream as the header words it: the
first failure met in stream order; a field that needs a bit behind the stream's end is TRUNCATED; a Huffman symbol is
read bit by bit until the bits are a code (15 bits that are none: SYMBOL).  OK exactly where zlib.decompress succeeds.
"""
import zlib

from _deflate import Bits, CL_ORDER, canonical, cl_sequence, huff_lengths

STATUS = ("OK", "HEADER", "TRUNCATED", "BTYPE", "STORED", "CODES", "SYMBOL", "DISTANCE", "ADLER", "ROOM", "REFUSED")
OK, HEADER, TRUNCATED, BTYPE, STORED, CODES, SYMBOL, DISTANCE, ADLER, ROOM, REFUSED = range(11)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _In:
    def __init__(self, data):
        self.d = bytes(data) + b"\0" * 8
        self.nbits = 8 * len(data)
        self.pos = 0

    def peek(self):
        """the next 32 bits at least, zeros behind the end"""
        p = self.pos
        return int.from_bytes(self.d[p >> 3:(p >> 3) + 8], "little") >> (p & 7)

    def need(self, n):
        if self.pos + n > self.nbits:
            raise _Stop(TRUNCATED)

    def take(self, n):
        self.need(n)
        v = self.peek() & ((1 << n) - 1)
        self.pos += n
        return v


def _left(lens):
    """what a set of code lengths leaves of the code space: 0 complete, > 0 incomplete, < 0 over-subscribed"""
    left = 1 << 15
    for l in lens:
        if l:
            left -= 1 << (15 - l)
    return left


def _set_ok(lens):
    """a set zlib takes: complete, or one code of one bit"""
    left = _left(lens)
    return left == 0 or (left > 0 and [l for l in lens if l] == [1])


class _Code:
    """first bit lowest: table[bits] = (symbol, length) over the next 9 bits, `long` {(length, code): symbol} behind it"""
    W = 9

    def __init__(self, lens):
        codes = canonical(list(lens))
        self.table = [None] * (1 << self.W)
        self.long = {}
        self.maxlen = max(lens) if lens else 0
        for s, l in enumerate(lens):
            if not l:
                continue
            rev = int(format(codes[s], "0%db" % l)[::-1], 2)
            if l <= self.W:
                for j in range(rev, 1 << self.W, 1 << l):
                    self.table[j] = (s, l)
            else:
                self.long[(l, rev)] = s

    def read(self, b):
        w = b.peek()
        e = self.table[w & ((1 << self.W) - 1)]
        if e is None:
            for l in range(self.W + 1, self.maxlen + 1):
                s = self.long.get((l, w & ((1 << l) - 1)))
                if s is not None:
                    e = (s, l)
                    break
        if e is None:
            raise _Stop(SYMBOL if b.pos + 15 <= b.nbits else TRUNCATED)
        b.need(e[1])
        b.pos += e[1]
        return e[0]


def _dynamic(b):
    b.need(14)
    nlen, ndist, ncode = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if nlen > 286 or ndist > 30:
        raise _Stop(CODES)
    cll = [0] * 19
    for i in range(ncode):
        cll[CL_ORDER[i]] = b.take(3)
    if _left(cll) != 0:
        raise _Stop(CODES)
    cl = _Code(cll)
    lens = []
    while len(lens) < nlen + ndist:
        s = cl.read(b)
        if s < 16:
            lens.append(s)
            continue
        rep = {16: 3, 17: 3, 18: 11}[s] + b.take({16: 2, 17: 3, 18: 7}[s])
        if (s == 16 and not lens) or len(lens) + rep > nlen + ndist:
            raise _Stop(CODES)
        lens += [lens[-1] if s == 16 else 0] * rep
    if lens[256] == 0:
        raise _Stop(CODES)
    ll, dl = lens[:nlen], lens[nlen:]
    if not _set_ok(ll) or not (not any(dl) or _set_ok(dl)):
        raise _Stop(CODES)
    return _Code(ll), _Code(dl)


_FIXED = None


def _walk(b, out):
    global _FIXED
    cmf, flg = b.take(8), b.take(8)
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or (flg & 0x20):
        raise _Stop(HEADER)
    while True:
        b.need(3)
        last, typ = b.take(1), b.take(2)
        if typ == 3:
            raise _Stop(BTYPE)
        if typ == 0:
            b.pos = (b.pos + 7) & ~7
            b.need(32)
            n, nn = b.take(16), b.take(16)
            if n != nn ^ 0xFFFF:
                raise _Stop(STORED)
            at = b.pos >> 3
            if 8 * (at + n) > b.nbits:
                raise _Stop(TRUNCATED)
            out += b.d[at:at + n]
            b.pos += 8 * n
        else:
            if typ == 1:
                if _FIXED is None:
                    _FIXED = (_Code(FIXED_LIT), _Code(FIXED_DIST))
                lit, dist = _FIXED
            else:
                lit, dist = _dynamic(b)
            while True:
                s = lit.read(b)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s >= 286:
                    raise _Stop(SYMBOL)
                ln = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                ds = dist.read(b)
                if ds >= 30:
                    raise _Stop(SYMBOL)
                d = DIST_BASE[ds] + b.take(DIST_EXTRA[ds])
                if d > len(out):
                    raise _Stop(DISTANCE)
                if d >= ln:
                    out += out[len(out) - d:len(out) - d + ln]
                else:
                    seg = bytes(out[len(out) - d:])
                    out += (seg * (ln // d + 1))[:ln]
        if last:
            break
    b.pos = (b.pos + 7) & ~7
    b.need(32)
    return int.from_bytes(b.d[b.pos >> 3:(b.pos >> 3) + 4], "big")


def inflate(stream, room=None):
    """-> (status, bytes, out_len); bytes is None unless OK, out_len None unless OK or ROOM.  room: the slot's bytes"""
    b = _In(stream)
    out = bytearray()
    try:
        adler = _walk(b, out)
    except _Stop as e:
        return e.status, None, None
    if room is not None and len(out) > room:
        return ROOM, None, len(out)
    if adler != zlib.adler32(bytes(out)):
        return ADLER, None, None
    return OK, bytes(out), len(out)


# ---------------------------------------------------------------------------- the forge

def length_symbol(ln, alt=False):
    """a match length -> (symbol, extra bits, extra value); alt: 258 as symbol 284 with extra bits 31"""
    if ln == 258 and not alt:
        return 285, 0, 0
    for i in range(27, -1, -1):
        if ln >= LEN_BASE[i]:
            return 257 + i, LEN_EXTRA[i], ln - LEN_BASE[i]
    raise ValueError(ln)


def dist_symbol(d):
    for i in range(29, -1, -1):
        if d >= DIST_BASE[i]:
            return i, DIST_EXTRA[i], d - DIST_BASE[i]
    raise ValueError(d)


def apply_tokens(tokens, out):
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "match":
            for _ in range(t[1]):
                out.append(out[len(out) - t[2]] if t[2] <= len(out) else 0)


def lits(data):
    return [("lit", v) for v in bytes(data)]


def _put_tokens(b, tokens, ll, dl, eob):
    lc, dc = canonical(list(ll)), canonical(list(dl))
    for t in tokens:
        if t[0] == "lit":
            b.code(lc[t[1]], ll[t[1]])
        elif t[0] == "match":
            s, eb, ev = length_symbol(t[1], len(t) > 3 and t[3] == "alt")
            b.code(lc[s], ll[s])
            b.put(ev, eb)
            ds, deb, dev = dist_symbol(t[2])
            b.code(dc[ds], dl[ds])
            b.put(dev, deb)
        elif t[0] == "bits":  # (value, count) as they are
            b.put(t[1], t[2])
    if eob:
        b.code(lc[256], ll[256])


def _histograms(tokens):
    lh, dh = [0] * 286, [0] * 30
    for t in tokens:
        if t[0] == "lit":
            lh[t[1]] += 1
        elif t[0] == "match":
            lh[length_symbol(t[1], len(t) > 3 and t[3] == "alt")[0]] += 1
            dh[dist_symbol(t[2])[0]] += 1
    lh[256] += 1
    return lh, dh


def put_block(b, blk, final):
    """One block into the Bits b.  blk: dict with
      type     "stored" | "fixed" | "dynamic"
      tokens   [("lit", byte) | ("match", length, distance[, "alt"]) | ("bits", value, count)]; stored: `data` bytes
      lit_lens, dist_lens   explicit code lengths (dynamic; default: Huffman lengths of the tokens, and [0] without a match)
      cl_lens  explicit lengths of the 19 code-length codes;  cl_syms  the explicit code-length sequence
      hlit, hdist   the header's fields as written (default: what the lengths give);  btype  the BTYPE field as written
      nlen     stored: the NLEN field as written;  eob  False: no end-of-block is written"""
    typ = blk["type"]
    b.put(1 if final else 0, 1)
    b.put(blk.get("btype", {"stored": 0, "fixed": 1, "dynamic": 2}[typ]), 2)
    if typ == "stored":
        data = bytes(blk.get("data", b""))
        b.put(0, -b.n % 8)
        b.put(len(data), 16)
        b.put(blk.get("nlen", len(data) ^ 0xFFFF), 16)
        for v in data:
            b.put(v, 8)
        return
    tokens = blk.get("tokens", [])
    if typ == "fixed":
        _put_tokens(b, tokens, FIXED_LIT, FIXED_DIST, blk.get("eob", True))
        return
    lh, dh = _histograms(tokens)
    ll = list(blk["lit_lens"]) if "lit_lens" in blk else huff_lengths(lh, 15)[0]
    ll = ll + [0] * (286 - len(ll))
    if "dist_lens" in blk:
        dl = list(blk["dist_lens"])
    else:
        dl = huff_lengths(dh, 15)[0] if any(dh) else [0]
    dl = dl + [0] * (30 - len(dl))
    nlen = max(257, max([s for s in range(286) if ll[s]] + [0]) + 1)
    ndist = max(1, max([s for s in range(30) if dl[s]] + [0]) + 1)
    nlen = blk.get("hlit", nlen - 257) + 257
    ndist = blk.get("hdist", ndist - 1) + 1
    seq = (ll + [0] * 8)[:nlen] + (dl + [0] * 8)[:ndist]
    cls = blk["cl_syms"] if "cl_syms" in blk else cl_sequence(seq)
    clh = [0] * 19
    for s, _, _ in cls:
        clh[s] += 1
    if "cl_lens" in blk:
        cll = list(blk["cl_lens"])
    else:
        cll = huff_lengths(clh, 7)[0]
        if sum(1 for l in cll if l) == 1:  # zlib wants this code complete: a second code of one bit
            cll[[s for s in range(19) if not cll[s]][0]] = 1
    clc = canonical(cll)
    ncl = max(4, max(i for i, s in enumerate(CL_ORDER) if cll[s]) + 1)
    b.put(nlen - 257, 5)
    b.put(ndist - 1, 5)
    b.put(ncl - 4, 4)
    for s in CL_ORDER[:ncl]:
        b.put(cll[s], 3)
    for s, eb, ev in cls:
        b.code(clc[s], cll[s])
        b.put(ev, eb)
    _put_tokens(b, tokens, ll, dl, blk.get("eob", True))


def plain_of(blocks):
    out = bytearray()
    for blk in blocks:
        if blk["type"] == "stored":
            out += bytes(blk.get("data", b""))
        else:
            apply_tokens(blk.get("tokens", []), out)
    return bytes(out)


def forge(blocks, head=b"\x78\x01", adler=None, trailing=b"", final=None):
    """blocks -> a zlib stream; head: CMF FLG as written; adler: the value written in the place of the bytes' own (or the
    bytes of the field as they are); final: which blocks carry BFINAL (default: the last)"""
    b = Bits()
    for i, blk in enumerate(blocks):
        put_block(b, blk, (i == len(blocks) - 1) if final is None else (i in final))
    if adler is None:
        adler = zlib.adler32(plain_of(blocks))
    tail = adler if isinstance(adler, bytes) else adler.to_bytes(4, "big")
    return bytes(head) + b.bytes() + tail + bytes(trailing)


# ---------------------------------------------------------------------------- the batteries

def _rng_bytes(n, seed):
    import random

    r = random.Random(seed)
    return bytes(r.getrandbits(8) for _ in range(n))


def inputs():
    """the four plain inputs of the zlib.compressobj cases"""
    import random

    r = random.Random(5)
    geo = bytes(min(255, int(r.expovariate(0.05))) for _ in range(60000))
    text = b"the quick brown fox jumps over the lazy dog; " * 700
    return {"run": b"\x07" * 40000, "text": text, "geo": geo, "random": _rng_bytes(33068, 9)}


def _cobj(data, **kw):
    args = dict(level=6, method=zlib.DEFLATED, wbits=15, memLevel=8, strategy=zlib.Z_DEFAULT_STRATEGY)
    args.update(kw)
    c = zlib.compressobj(args["level"], args["method"], args["wbits"], args["memLevel"], args["strategy"])
    return c.compress(data) + c.flush()


PHASE_LENS = {65: 1, 66: 2, 256: 2}  # a complete set: 'A' in one bit


def _phase_block(k):
    ll = [0] * 257
    for s, l in PHASE_LENS.items():
        ll[s] = l
    return {"type": "dynamic", "tokens": [("lit", 66)] + [("lit", 65)] * k, "lit_lens": ll, "dist_lens": [0]}


def _steps(n):
    """a complete set of n codes with the lengths 1, 2, ..., n - 1, n - 1"""
    return list(range(1, n)) + [n - 1]


def valid_forged():
    """-> [(name, stream, plain)]"""
    out = []

    def add(name, blocks, **kw):
        out.append((name, forge(blocks, **kw), plain_of(blocks)))

    far = _rng_bytes(32768, 1)
    add("dist-32768-32767", [{"type": "dynamic", "tokens": lits(far) + [("match", 150, 32768), ("match", 150, 32767)]}])
    add("match-first-byte", [{"type": "dynamic", "tokens": lits(b"abc") + [("match", 3, 3)]}])
    add("dist1-len258", [{"type": "dynamic", "tokens": lits(b"z") + [("match", 258, 1)]}])
    add("258-as-284+31", [{"type": "dynamic", "tokens": lits(b"yz") + [("match", 258, 2, "alt")]}])
    add("258-as-284+31-fixed", [{"type": "fixed", "tokens": lits(b"q") + [("match", 258, 1, "alt"), ("match", 258, 1)]}])
    ll = [0] * 258
    for s, l in zip(list(range(14)) + [256, 257], _steps(16)):
        ll[s] = l
    dl = _steps(16)
    add("15-bit-codes", [{"type": "dynamic", "lit_lens": ll, "dist_lens": dl,
                          "tokens": lits(bytes(range(14)) * 15) + [("match", 3, 193 + 7), ("lit", 13)]}])
    add("hlit-286-hdist-30", [{"type": "dynamic", "tokens": lits(_rng_bytes(24600, 2)) + [("match", 258, 24577 + 11)]}])
    ll = [0] * 259
    ll[97], ll[98], ll[256], ll[257], ll[258] = 2, 2, 3, 3, 2
    blk = {"type": "dynamic", "lit_lens": ll, "dist_lens": [2, 2, 2, 2], "tokens": lits(b"abba") + [("match", 4, 2), ("match", 3, 4)]}
    assert cl_sequence(ll + [2, 2, 2, 2])[-1] == (16, 2, 1), "the repeat runs from the literal lengths into the distance lengths"
    add("repeat-across-the-boundary", [blk])
    add("zero-run-across-the-boundary", [{"type": "dynamic", "hlit": 29, "dist_lens": [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1],
                                           "tokens": lits(b"hello")}])
    add("no-distance-code", [{"type": "dynamic", "dist_lens": [0], "tokens": lits(b"only literals here")}])
    add("one-code-is-end-of-block", [{"type": "dynamic", "tokens": []}])
    big = _rng_bytes(65535, 3)
    for k in range(8):
        for name, data in (("0", b""), ("65535", big)):
            add("stored-%s-phase-%d" % (name, k),
                [_phase_block(k), {"type": "stored", "data": data}, {"type": "dynamic", "tokens": lits(b"tail") + [("match", 4, 4)]}])
    add("match-into-stored", [{"type": "stored", "data": b"0123456789"}, {"type": "dynamic", "tokens": [("match", 25, 10), ("lit", 33)]}])
    add("match-into-stored-fixed", [{"type": "stored", "data": b"0123456789"}, {"type": "fixed", "tokens": [("match", 10, 7)]}])
    add("trailing-bytes", [{"type": "fixed", "tokens": lits(b"trail")}], trailing=b"\x00\xff junk behind the Adler-32")
    add("empty-final-stored", [{"type": "fixed", "tokens": lits(b"x")}, {"type": "stored", "data": b""}])
    add("empty-final-fixed", [{"type": "stored", "data": b"xy"}, {"type": "fixed", "tokens": []}])
    return out


def valid_zlib():
    """-> [(name, stream, plain)]: what zlib.compressobj writes"""
    out = []
    for name, data in inputs().items():
        for tag, kw in (("l0", dict(level=0)), ("l1", dict(level=1)), ("l6", dict(level=6)), ("l9", dict(level=9)),
                        ("fixed", dict(strategy=zlib.Z_FIXED)), ("huff", dict(strategy=zlib.Z_HUFFMAN_ONLY)),
                        ("rle", dict(strategy=zlib.Z_RLE)), ("w9", dict(wbits=9)), ("m1", dict(memLevel=1))):
            out.append(("%s-%s" % (name, tag), _cobj(data, **kw), data))
    c = zlib.compressobj()
    s = c.compress(b"01234") + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(b"56") + c.flush(zlib.Z_FULL_FLUSH) + c.compress(b"789") + c.flush()
    out.append(("flushes", s, b"0123456789"))
    out.append(("empty", zlib.compress(b""), b""))
    return out


def malformed():
    """-> [(name, stream, status)]"""
    out = []

    def add(name, status, blocks, **kw):
        out.append((name, forge(blocks, **kw) if isinstance(blocks, list) else blocks, status))

    base = [("lit", 1), ("lit", 2), ("lit", 3)]
    add("codes-hlit-287", CODES, [{"type": "dynamic", "tokens": base, "hlit": 30}])
    add("codes-hdist-31", CODES, [{"type": "dynamic", "tokens": base, "hdist": 30}])
    add("codes-repeat-first", CODES, [{"type": "dynamic", "tokens": base, "cl_syms": [(16, 2, 0)] + [(18, 7, 127)] * 2, "cl_lens": [0] * 16 + [1, 0, 1]}])
    ll = [0] * 257
    ll[1], ll[2], ll[3], ll[256] = 2, 2, 2, 2
    add("codes-repeat-past-the-end", CODES, [{"type": "dynamic", "tokens": base, "lit_lens": ll, "dist_lens": [0],
                                              "cl_syms": cl_sequence(ll) + [(17, 3, 0)]}])
    over = list(ll)
    over[4] = 1
    add("codes-over-subscribed", CODES, [{"type": "dynamic", "tokens": base, "lit_lens": over, "dist_lens": [0]}])
    under = list(ll)
    under[3] = 0
    add("codes-incomplete-literals", CODES, [{"type": "dynamic", "tokens": base[:2], "lit_lens": under, "dist_lens": [0]}])
    add("codes-incomplete-distances", CODES, [{"type": "dynamic", "tokens": base, "lit_lens": ll, "dist_lens": [2, 2]}])
    add("codes-one-2-bit-distance", CODES, [{"type": "dynamic", "tokens": base, "lit_lens": ll, "dist_lens": [0, 2]}])
    add("codes-over-subscribed-distances", CODES, [{"type": "dynamic", "tokens": base, "lit_lens": ll, "dist_lens": [1, 1, 1]}])
    add("codes-cl-incomplete", CODES, [{"type": "dynamic", "tokens": base, "lit_lens": ll, "dist_lens": [0],
                                        "cl_lens": [2 if s in (0, 2, 18) else 0 for s in range(19)]}])
    add("codes-cl-over-subscribed", CODES, [{"type": "dynamic", "tokens": base, "lit_lens": ll, "dist_lens": [0],
                                             "cl_lens": [1 if s in (0, 2, 18) else 0 for s in range(19)]}])
    noeob = [0] * 257
    noeob[1], noeob[2] = 1, 1
    add("codes-no-end-of-block", CODES, [{"type": "dynamic", "tokens": base[:2], "lit_lens": noeob, "dist_lens": [0], "eob": False}])
    add("symbol-286", SYMBOL, [{"type": "fixed", "tokens": base + [("bits", 0b01100011, 8), ("bits", 0, 8)]}])
    add("symbol-287", SYMBOL, [{"type": "fixed", "tokens": base + [("bits", 0b11100011, 8), ("bits", 0, 8)]}])
    # fixed: length symbol 257 is 0000001 first bit first; distance symbols 30, 31 are 11110, 11111
    add("symbol-distance-30", SYMBOL, [{"type": "fixed", "tokens": base + [("bits", 0b1000000, 7), ("bits", 0b01111, 5)]}])
    add("symbol-distance-31", SYMBOL, [{"type": "fixed", "tokens": base + [("bits", 0b1000000, 7), ("bits", 0b11111, 5)]}])
    m = [0] * 258
    m[1], m[2], m[256], m[257] = 2, 2, 2, 2
    lc = canonical(m)
    code257 = int(format(lc[257], "02b")[::-1], 2)
    add("symbol-outside-the-1-bit-set", SYMBOL, [{"type": "dynamic", "lit_lens": m, "dist_lens": [1],
                                                 "tokens": [("lit", 1), ("lit", 2), ("lit", 1), ("bits", code257, 2), ("bits", 0x7FFF, 15)]}])
    add("symbol-no-distance-code", SYMBOL, [{"type": "dynamic", "lit_lens": m, "dist_lens": [0],
                                            "tokens": [("lit", 1), ("lit", 2), ("lit", 1), ("bits", code257, 2), ("bits", 0, 15)]}])
    add("distance-one-past-the-start", DISTANCE, [{"type": "dynamic", "tokens": base + [("match", 3, 4)]}])
    add("distance-at-once", DISTANCE, [{"type": "fixed", "tokens": [("match", 3, 1)]}])
    add("distance-behind-a-stored-block", DISTANCE, [{"type": "stored", "data": b"abcd"}, {"type": "fixed", "tokens": [("match", 3, 5)]}])
    s60 = forge([{"type": "dynamic", "tokens": lits(bytes(range(30, 70)) + b"abcabc") + [("match", 9, 3)]}])
    s60 = s60 + b"\0" * 0
    assert 50 <= len(s60) <= 80, len(s60)
    for cut in range(len(s60)):
        out.append(("truncated-60-at-%d" % cut, s60[:cut], TRUNCATED))
    big = forge([{"type": "dynamic", "tokens": lits(_rng_bytes(300, 4)) + [("match", 40, 200)]}])
    for cut in range(2, 40):  # every byte of the dynamic header: HLIT / HDIST / HCLEN, the 3-bit lengths, the sequence
        out.append(("truncated-header-at-%d" % cut, big[:cut], TRUNCATED))
    st = forge([{"type": "stored", "data": b"stored bytes"}])
    for cut in (3, 4, 5, 6, 7, 10, len(st) - 5):
        out.append(("truncated-stored-at-%d" % cut, st[:cut], TRUNCATED))
    add("stored-len-nlen", STORED, [{"type": "stored", "data": b"abc", "nlen": 0xFFFD}])
    add("stored-len-nlen-later", STORED, [{"type": "fixed", "tokens": base}, {"type": "stored", "data": b"", "nlen": 0}])
    add("btype-3", BTYPE, [{"type": "fixed", "tokens": base, "btype": 3}])
    add("btype-3-second", BTYPE, [{"type": "fixed", "tokens": base}, {"type": "fixed", "tokens": base, "btype": 3}])
    ok = forge([{"type": "fixed", "tokens": lits(b"header cases")}])

    def head(cmf, fdict=0):  # FLG with the FCHECK that makes the pair a multiple of 31
        flg = fdict << 5
        return bytes([cmf, flg + (31 - ((cmf << 8) + flg) % 31) % 31])

    out.append(("header-fdict", head(0x78, 1) + ok[2:], HEADER))
    out.append(("header-fcheck", b"\x78\x02" + ok[2:], HEADER))
    out.append(("header-cm-9", head(0x79) + ok[2:], HEADER))
    out.append(("header-cinfo-8", head(0x88) + ok[2:], HEADER))
    out.append(("adler-wrong", ok[:-1] + bytes([ok[-1] ^ 1]), ADLER))
    out.append(("adler-wrong-top", ok[:-4] + bytes([ok[-4] ^ 0x80]) + ok[-3:], ADLER))
    for k in (1, 2, 3, 4):
        out.append(("adler-cut-%d" % k, ok[:-k], TRUNCATED))
    return out


# ---------------------------------------------------------------------------- the battery as a file

def fnv1a(data):
    h = 0x811C9DC5
    for v in bytes(data):
        h = ((h ^ v) * 0x01000193) & 0xFFFFFFFF
    return h


def battery_file(max_stream=4096):
    """The malformed battery and the valid streams of at most max_stream bytes as tools/inflate_walk_check.cpp reads them
    (tests/golden/inflate_battery.bin): "IFB1", u32 count, then per stream u8 status, u64 inflated length (all ones: none),
    u32 FNV-1a of the inflated bytes, u32 length, the stream."""
    rows = [(st, OK, plain) for _, st, plain in valid_forged() + valid_zlib() if len(st) <= max_stream]
    rows += [(st, status, None) for _, st, status in malformed()]
    out = bytearray(b"IFB1" + len(rows).to_bytes(4, "little"))
    for st, status, plain in rows:
        n = len(plain) if plain is not None else 0xFFFFFFFFFFFFFFFF
        out += bytes([status]) + n.to_bytes(8, "little") + fnv1a(plain or b"").to_bytes(4, "little") + len(st).to_bytes(4, "little") + st
    return bytes(out)


if __name__ == "__main__":
    import os
    import sys

    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate_battery.bin")
    with open(path, "wb") as f:
        f.write(battery_file())
    print(path, os.path.getsize(path))
