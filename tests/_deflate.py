"""Serial model of the device's zlib streams for BLOW5 records (include/press_hip.h section 2z): the byte-for-byte
yardstick of press_hip_blow5_deflate_batch.  Nothing here is imported by the product package.

A record R of m bytes becomes  78 01 | one final DEFLATE block | Adler-32(R), big endian.  The block is dynamic
Huffman (BTYPE 2) over literals, distance-1 matches for the zero runs and end-of-block, or - where that would not be
shorter - stored blocks of at most 65 535 bytes."""
import zlib

NLIT = 286
EOB = 256
MATCH_MAX = 258
STORED_MAX = 65535
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5: length code -> (extra bits, first length)
LEN_CODES = ([(257 + i, 0, 3 + i) for i in range(8)] +
             [(265 + i, 1, 11 + 2 * i) for i in range(4)] + [(269 + i, 2, 19 + 4 * i) for i in range(4)] +
             [(273 + i, 3, 35 + 8 * i) for i in range(4)] + [(277 + i, 4, 67 + 16 * i) for i in range(4)] +
             [(281 + i, 5, 131 + 32 * i) for i in range(4)] + [(285, 0, 258)])


def length_code(ln):
    """a match length 3 .. 258 -> (symbol, extra bits, extra value)"""
    if ln == 258:
        return 285, 0, 0
    for sym, eb, base in reversed(LEN_CODES[:-1]):
        if ln >= base:
            return sym, eb, ln - base
    raise ValueError(ln)


def tokens(rec):
    """the record's tokens in order: ("lit", byte) and ("match", length), without end-of-block"""
    out = []
    i, m = 0, len(rec)
    while i < m:
        if rec[i]:
            out.append(("lit", rec[i]))
            i += 1
            continue
        j = i
        while j < m and rec[j] == 0:
            j += 1
        out.append(("lit", 0))
        rest = j - i - 1
        while rest >= 3:
            piece = min(rest, MATCH_MAX)
            out.append(("match", piece))
            rest -= piece
        out.extend([("lit", 0)] * rest)
        i = j
    return out


def _build(counts):
    """Huffman code lengths of the symbols with a count: the list ascending by (count, symbol); the first two nodes
    become a parent with the sum of their counts, which goes back in front of the first remaining node whose count is not
    smaller; a symbol's length is its depth.  One symbol alone: length 1."""
    present = sorted((c, s) for s, c in enumerate(counts) if c)
    lens = [0] * len(counts)
    if len(present) == 1:
        lens[present[0][1]] = 1
        return lens
    nodes = [(c, [s]) for c, s in present]
    while len(nodes) > 1:
        (c1, l1), (c2, l2) = nodes[0], nodes[1]
        for s in l1 + l2:
            lens[s] += 1
        rest = nodes[2:]
        pc = c1 + c2
        pos = 0
        while pos < len(rest) and rest[pos][0] < pc:
            pos += 1
        rest.insert(pos, (pc, l1 + l2))
        nodes = rest
    return lens


def huff_lengths(counts, limit):
    """-> (lengths, k): _build of the counts; longer than `limit`: of max(1, c >> k) for the smallest k that fits"""
    k = 0
    while True:
        lens = _build([max(1, c >> k) if c else 0 for c in counts])
        if max(lens) <= limit:
            return lens, k
        k += 1


def canonical(lens):
    """RFC 1951 3.2.2 -> the codes (first bit on top)"""
    maxl = max(lens) if lens else 0
    bl = [0] * (maxl + 2)
    for l in lens:
        if l:
            bl[l] += 1
    nxt = [0] * (maxl + 2)
    code = 0
    for b in range(1, maxl + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def cl_sequence(seq):
    """the code-length sequence -> [(symbol 0 .. 18, extra bits, extra value)].  A run of equal lengths, zeros: 18 for
    min(run, 138) while the run has 11 or more, then 17 for 3 .. 10, else the zeros themselves; another length: itself
    once, then 16 for min(rest, 6) while the rest has 3 or more, then the rest themselves."""
    out = []
    i = 0
    while i < len(seq):
        v = seq[i]
        j = i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                t = min(run, 138)
                out.append((18, 7, t - 11))
                run -= t
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
            out.extend([(0, 0, 0)] * run)
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                t = min(run, 6)
                out.append((16, 2, t - 3))
                run -= t
            out.extend([(v, 0, 0)] * run)
        i = j
    return out


class Bits:
    """the stream's bits: bit i is bit i % 8 of byte i / 8"""

    def __init__(self):
        self.out, self.acc, self.k, self.n = bytearray(), 0, 0, 0

    def put(self, value, nbits):
        self.acc |= value << self.k
        self.k += nbits
        self.n += nbits
        if self.k >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.k -= 64

    def code(self, code, ln):
        """a Huffman code, its first bit first"""
        self.put(int(format(code, "0%db" % ln)[::-1], 2) if ln else 0, ln)

    def bytes(self):
        return bytes(self.out) + self.acc.to_bytes((self.k + 7) // 8, "little")


def histogram(rec):
    h = [0] * NLIT
    for kind, v in tokens(rec):
        h[v if kind == "lit" else length_code(v)[0]] += 1
    h[EOB] = 1
    return h


def stored_length(m):
    return m + 5 * max(1, (m + STORED_MAX - 1) // STORED_MAX)


def dynamic_block(rec, info=None):
    """-> the block's bytes (the last one zero padded)"""
    hist = histogram(rec)
    lens, k = huff_lengths(hist, 15)
    codes = canonical(lens)
    nlit = max(257, max(s for s in range(NLIT) if lens[s]) + 1)
    cls = cl_sequence(lens[:nlit] + [1])
    clh = [0] * 19
    for s, _, _ in cls:
        clh[s] += 1
    cll, cl_k = huff_lengths(clh, 7)
    clc = canonical(cll)
    ncl = max(4, max(i for i, s in enumerate(CL_ORDER) if cll[s]) + 1)
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(nlit - 257, 5)
    b.put(0, 5)
    b.put(ncl - 4, 4)
    for s in CL_ORDER[:ncl]:
        b.put(cll[s], 3)
    for s, eb, ev in cls:
        b.code(clc[s], cll[s])
        b.put(ev, eb)
    hbits = b.n
    rev = [int(format(codes[s], "0%db" % lens[s])[::-1], 2) if lens[s] else 0 for s in range(NLIT)]  # as written: first bit lowest
    for kind, v in tokens(rec):
        if kind == "lit":
            b.put(rev[v], lens[v])
        else:
            s, eb, ev = length_code(v)
            b.put(rev[s], lens[s])
            b.put(ev, eb)
            b.put(0, 1)  # the one distance code
    b.put(rev[EOB], lens[EOB])
    if info is not None:
        info.update(k=k, maxlen=max(lens), lens=lens, nlit=nlit, header_bits=hbits, hist=hist, cl_k=cl_k, ncl=ncl, cl_hist=clh,
                    cl_syms=cls)
    return b.bytes()


def unit_bits(rec, lens, unit=1024):
    """-> the bits of the tokens of every `unit` bytes of the record under the code lengths `lens`; a token counts for the
    unit in which it opens, a match with its extra bits and its one distance bit; end-of-block counts for none"""
    out = [0] * ((len(rec) + unit - 1) // unit)
    pos = 0
    for kind, v in tokens(rec):
        if kind == "lit":
            out[pos // unit] += lens[v]
            pos += 1
        else:
            s, eb, _ = length_code(v)
            out[pos // unit] += lens[s] + eb + 1
            pos += v
    return out


def unit_starts(rec, lens, header_bits, unit=1024):
    """-> the bit at which every unit's first token stands, counted from the first byte of the record's place in the image:
    80 bits (the u64 length and 78 01), the block header, and the bits of the units before it"""
    out, at = [], 80 + header_bits
    for b in unit_bits(rec, lens, unit):
        out.append(at)
        at += b
    return out


def stored_blocks(rec):
    out = bytearray()
    m = len(rec)
    nb = max(1, (m + STORED_MAX - 1) // STORED_MAX)
    for i in range(nb):
        part = rec[i * STORED_MAX:(i + 1) * STORED_MAX]
        out += bytes([1 if i == nb - 1 else 0]) + len(part).to_bytes(2, "little") + (len(part) ^ 0xFFFF).to_bytes(2, "little") + part
    return bytes(out)


def deflate_record(rec, info=None):
    """-> (stream, raw): the zlib stream of one record, raw = 1 where it took the stored form"""
    rec = bytes(rec)
    dyn = dynamic_block(rec, info)
    raw = len(dyn) >= stored_length(len(rec))
    body = stored_blocks(rec) if raw else dyn
    return b"\x78\x01" + body + zlib.adler32(rec).to_bytes(4, "big"), int(raw)


def frame(pre, sig, post, signal_method):
    """pre | u64 length | signal | post, as press_hip_blow5_write frames a record"""
    lenfield = len(sig) if signal_method else len(sig) // 2
    return bytes(pre) + lenfield.to_bytes(8, "little") + bytes(sig) + bytes(post)


def image(records):
    """-> (image, rec_off, raw): per record u64 stream length | stream, back to back"""
    out = bytearray()
    off, raws = [0], []
    for rec in records:
        st, raw = deflate_record(rec)
        out += len(st).to_bytes(8, "little") + st
        off.append(len(out))
        raws.append(raw)
    return bytes(out), off, raws
