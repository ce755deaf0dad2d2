"""Yardstick and reads for the per-read Huffman family (tests/test_huffman_family.py, tests/golden/make_huffman_golden.py):
the four methods huffman_{vbe21, vbbe21, vbsbe21, vbsse21}_zd of press/press.h.

A numpy restatement of huffman(low) (huffman/huffman.c: calculate_huffman_codes, write_code_table_to_memory,
do_memory_encode) and of the decoder as include/press_hip.h section (2v) defines it, proven against
tests/golden/ref_huffman.json (the compiled reference) by CPU tests before any GPU test uses it.  The splice - header and
section of the plain layout in front of table and payload - goes through _rcf.split.

Nothing here touches a GPU.
"""
import json
import os

import numpy as np

import _libs
import _rcf
import _rice

LAYOUTS = _rcf.LAYOUTS
sha = _rcf.sha


def name(layout):
    return "huffman_%s_zd" % layout


# ------------------------------------------------------------------ huffman(low), restated

def build_code(counts):
    """counts: 256 occurrence counts -> {symbol: (len, bits)}, bit k of `bits` the k-th edge from the root.

    The symbols present ascending by count, ties by symbol; the first two nodes of the list become the zero and the one
    child of a parent that goes back in front of every remaining node whose count is not smaller than its own."""
    lst = [(int(counts[s]), ("L", s)) for s in sorted((s for s in range(256) if counts[s]), key=lambda s: (int(counts[s]), s))]
    if not lst:
        return {}
    while len(lst) > 1:
        m1, m2, rest = lst[0], lst[1], lst[2:]
        c = m1[0] + m2[0]
        i = 0
        while i < len(rest) and rest[i][0] < c:
            i += 1
        rest.insert(i, (c, ("P", m1[1], m2[1])))
        lst = rest
    code = {}
    stack = [(lst[0][1], 0, 0)]
    while stack:
        node, ln, bits = stack.pop()
        if node[0] == "L":
            code[node[1]] = (ln, bits)
        else:
            stack.append((node[1], ln + 1, bits))
            stack.append((node[2], ln + 1, bits | 1 << ln))
    return code


def table_bytes(code, nlow):
    out = bytearray([(len(code) - 1) & 255]) + int(nlow).to_bytes(4, "big")
    for s in sorted(code):
        ln, bits = code[s]
        out += bytes([s, ln]) + bits.to_bytes((ln + 7) // 8, "little")
    return bytes(out)


def encode(low):
    """-> (table + payload, the longest code's length)"""
    x = np.frombuffer(bytes(low), dtype=np.uint8)
    code = build_code(np.bincount(x, minlength=256))
    table = table_bytes(code, len(x))
    lens_s = np.zeros(256, dtype=np.int64)
    bits_s = np.zeros(256, dtype=np.uint64)
    for s, (ln, b) in code.items():
        lens_s[s], bits_s[s] = ln, b
    lens = lens_s[x]
    nbits = int(lens.sum())
    if nbits == 0:
        return table, 0
    starts = np.cumsum(lens) - lens
    codes = bits_s[x]
    bits = np.zeros(nbits, dtype=np.uint8)
    idx = np.arange(len(x))
    for j in range(int(lens_s.max())):
        idx = idx[lens[idx] > j]
        bits[starts[idx] + j] = (codes[idx] >> np.uint64(j)) & np.uint64(1)
    return table + np.packbits(bits, bitorder="little").tobytes(), int(lens_s.max())


def parse_table(buf):
    """-> (entries [(symbol, len, bits)], count, table bytes), or None where definition 4 calls the table invalid; a
    count field of 0 is an empty table whatever the first byte says"""
    buf = bytes(buf)
    if len(buf) < 5:
        return None
    count = int.from_bytes(buf[1:5], "big")
    if count == 0:
        return [], 0, 5
    nent, p, ent = buf[0] + 1, 5, []
    for _ in range(nent):
        if p + 2 > len(buf):
            return None
        s, ln = buf[p], buf[p + 1]
        nb = (ln + 7) // 8
        if ln > 63 or (ln == 0 and nent != 1) or p + 2 + nb > len(buf):
            return None
        bits = int.from_bytes(buf[p + 2:p + 2 + nb], "little") & ((1 << ln) - 1)
        ent.append((s, ln, bits))
        p += 2 + nb
    for i, (_, la, a) in enumerate(ent):  # prefix-free: no code is the head of another, equal codes included
        for j, (_, lb, b) in enumerate(ent):
            if i != j and la <= lb and (b & ((1 << la) - 1)) == a:
                return None
    return ent, count, p


def decode(buf, nlow):
    """nlow values out of table + payload, or None where the library refuses the read (definition 4)"""
    t = parse_table(buf)
    if t is None:
        return None
    ent, count, p = t
    if count != nlow:
        return None
    if count == 0:
        return b""
    if len(ent) == 1 and ent[0][1] == 0:
        return bytes([ent[0][0]]) * nlow
    pay = np.frombuffer(bytes(buf[p:]) + b"\0" * 16, dtype=np.uint8).astype(np.uint64)
    real = 8 * (len(buf) - p)
    word = np.zeros(len(pay) - 8, dtype=np.uint64)
    for k in range(8):
        word |= pay[k:k + len(word)] << np.uint64(8 * k)
    pos = np.arange(real, dtype=np.int64)
    sh = (pos & 7).astype(np.uint64)
    win = word[pos >> 3] >> sh
    hi = pay[(pos >> 3) + 8] << ((np.uint64(64) - sh) & np.uint64(63))
    win |= np.where(sh == 0, np.uint64(0), hi)
    ln_at = np.zeros(real, dtype=np.int64)
    sym_at = np.zeros(real, dtype=np.uint8)
    for s, ln, bits in ent:
        m = (win & np.uint64((1 << ln) - 1)) == np.uint64(bits)
        ln_at[m], sym_at[m] = ln, s
    nxt = ln_at.tolist()
    out, at = [], 0
    while len(out) < nlow:
        if at >= real or nxt[at] == 0 or at + nxt[at] > real:
            return None  # bits that are no code, or the payload ends early
        out.append(at)
        at += nxt[at]
    return sym_at[np.array(out)].tobytes()


# ------------------------------------------------------------------ the splice

def low_of(s):
    return _rcf.split("vbe21", np.ascontiguousarray(s, dtype=np.int16))[1]


def expected(layout, s):
    """the stream of huffman_layout_zd -> (stream, the longest code's length)"""
    s = np.ascontiguousarray(s, dtype=np.int16)
    tail, maxlen = encode(low_of(s))
    return _rcf.split(layout, s)[0] + tail, maxlen


head_len = _rice.head_len


def decoded(layout, stream, head, n):
    """the n samples a stream decodes to (None: refused), `head` bytes of header and section in front of the table"""
    nex = int.from_bytes(stream[2:6], "little")
    low = decode(stream[head:], n - 1 - nex)
    if low is None:
        return None
    ret, back = _libs.oracle().depress(layout + "_zd", stream[:head] + low, n)
    assert ret == 0
    return back


# ------------------------------------------------------------------ the reads

def fib_low(nsym):
    """nsym symbols with Fibonacci counts 1, 1, 2, 3 ...: the deepest code has nsym - 1 bits; shuffled"""
    f = [1, 1]
    while len(f) < nsym:
        f.append(f[-1] + f[-2])
    # the steps the symbols stand for are chosen so that the counts times the steps cancel: from the largest count down,
    # the unused step of -128 .. 127 that leaves the smallest drift; shuffled, the walk then stays inside 16 bits
    # (from_low asserts it)
    free, drift, sym = list(range(-128, 128)), 0, []
    for c in reversed(f):
        d = min(free, key=lambda d: (abs(drift + c * d), abs(d), d))
        free.remove(d)
        drift += c * d
        sym.append(2 * d if d >= 0 else -2 * d - 1)
    low = np.repeat(np.array(sym[::-1], dtype=np.uint8), f)
    np.random.default_rng(nsym).shuffle(low)
    return low.tobytes()


def never_sync_low():
    """eight symbols 500 times each, shuffled: every code has 3 bits, a subsequence boundary is never a code boundary
    for a decoder that starts at the wrong bit"""
    low = np.repeat(np.arange(8, dtype=np.uint8) * 3, 500)
    np.random.default_rng(8).shuffle(low)
    return low.tobytes()


BIG = "fib-34"  # the one large read: 14 930 352 samples, a 33-bit code


def extra_reads():
    """the reads of the fixture beyond _rice.named_reads()"""
    rng = np.random.default_rng(77)
    geo = np.minimum(rng.geometric(0.3, size=6000) - 1, 255).astype(np.uint8)
    return [
        ("two-symbols", _rcf.from_low(bytes([0, 1]) * 700)),
        ("every-byte", _rcf.from_low(bytes(int(v) for v in np.random.default_rng(256).permutation(256)))),
        ("ties-40x7", _rcf.from_low(bytes(np.random.default_rng(40).permutation(np.repeat(np.arange(40, dtype=np.uint8), 7))))),
        ("never-sync", _rcf.from_low(never_sync_low())),
        ("fib-24", _rcf.from_low(fib_low(24))),
        (BIG, _rcf.from_low(fib_low(34))),
        ("geometric", _rcf.from_low(geo.tobytes())),
    ]


_reads = {}


def named_reads():
    """every read of the fixture"""
    if "r" not in _reads:
        _reads["r"] = _rice.named_reads() + extra_reads()
    return _reads["r"]


_fx = {}


def fixture():
    if "f" not in _fx:
        _fx["f"] = json.load(open(os.path.join(_rcf.GOLD, "ref_huffman.json")))
    return _fx["f"]
