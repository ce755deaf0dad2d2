"""The device's deflate (include/press_hip.h section 2z) at the edges its first battery does not reach: 63 to 200 records
in a call, counts that are rescaled twice and three times, the 7-bit limit of the code-length alphabet, every repeat code
of the block header at its run-length edges, a unit whose every byte takes a 15-bit code next to another dense one, stored
blocks at their seams and the dynamic / stored tie, zero runs from every place of a 16-byte grid, record_bytes too small
and too large, and the largest Adler sums.

The yardstick is tests/_deflate.py, byte for byte, as in test_blow5_deflate.py.  Every fixture is made here from a fixed
seed.  The CPU tests assert of every fixture the property it is there for - so that a later edit cannot quietly drain it -
and that zlib inflates the model's stream to the record.  The GPU tests hold image, rec_off, raw and the sizes call against
the model.  U = DEFLATE_UNIT is all this file knows of the kernels.

What a framed record cannot reach: its length field ends in at least five zero bytes for any signal below 2^24 bytes, so a
framed record always holds a match and nlit is 259 at the least (test_header_fields asserts it).  nlit 257 and 258 are
held on the model alone, on bare records; the device sees 259, 260, 261 and 286."""
import functools
import struct
import zlib

import numpy as np
import pytest

import _deflate as D
from honours_amd import deflate, press
from test_blow5_deflate import DeviceBatch, arrays, battery, check_device, first_difference, lib  # noqa: F401  (lib: the fixture)

U = deflate.DEFLATE_UNIT
REFUSED = deflate.DEFLATE_REFUSED


def nzb(n, seed=0):
    """n bytes, none of them zero"""
    return bytes(1 + (seed + 7 * i) % 255 for i in range(n))


@functools.lru_cache(maxsize=None)
def model(rec):
    """-> (stream, raw, info) of one record by the model; every fixture is deflated once per session"""
    info = {}
    stream, raw = D.deflate_record(rec, info)
    return stream, raw, info


def framed(cases, signal_method=1):
    return [D.frame(p, s, q, signal_method) for _, p, s, q in cases]


def model_image(recs):
    """D.image(recs) from the streams that model() keeps"""
    out, off, raws = bytearray(), [0], []
    for rec in recs:
        stream, raw, _ = model(rec)
        out += len(stream).to_bytes(8, "little") + stream
        off.append(len(out))
        raws.append(raw)
    return bytes(out), off, raws


def inflates(cases, signal_method=1):
    for (name, _, _, _), rec in zip(cases, framed(cases, signal_method)):
        stream, raw, _ = model(rec)
        assert stream[:2] == b"\x78\x01" and zlib.decompress(stream) == rec, name


def exact_parts(seq, pre_len, post_len):
    """(pre, sig, post) of a record that holds, next to its length field's zero bytes, exactly the bytes of `seq` (none of
    them zero): the length field's own bytes are taken out of seq.  None where seq does not hold them."""
    for n_lf in (1, 2, 3):
        sig_len = len(seq) - n_lf - pre_len - post_len
        lf = sig_len.to_bytes(8, "little").rstrip(b"\0") if sig_len > 0 else b""
        if len(lf) == n_lf and 0 not in lf:
            break
    else:
        return None
    body = bytearray(seq)
    for v in lf:
        at = body.rfind(bytes([v]))
        if at < 0:
            return None
        del body[at]
    body = bytes(body)
    return body[:pre_len], body[pre_len:pre_len + sig_len], body[pre_len + sig_len:]


def exact_case(name, seq, pre_len, post_len):
    """the first pre_len from the given one on for which exact_parts finds the length field's bytes in seq"""
    for p in range(pre_len, pre_len + 256):
        parts = exact_parts(seq, p, post_len)
        if parts is not None:
            assert sorted(D.frame(*parts, 1).replace(b"\0", b"")) == sorted(seq)
            return (name,) + parts
    raise AssertionError("no pre_len for " + name)


# ------------------------------------------------------------------ the fixtures

@functools.lru_cache(maxsize=None)
def fib_cases():
    """Framed records whose counts - end-of-block, the length field's literal zero and its match, then the byte values -
    are 1, 1, 1, 2, 3, 5, 8, ...: the unlimited tree is a chain.  The byte values are relabelled so that the length field's
    bytes are the two most common ones."""
    out = []
    for limit in (50000, 300000):
        counts, a, b = [], 2, 3
        while sum(counts) + a < limit:
            counts.append(a)
            a, b = b, a + b
        total, pre_len, post_len = sum(counts), 20, 3
        sig_len = total - 2 - pre_len - post_len
        if sig_len >= 65536:
            sig_len -= 1
        lf = sig_len.to_bytes(8, "little").rstrip(b"\0")
        assert 0 not in lf and len(set(lf)) == len(lf) and len(lf) <= 3
        labels = [v for v in range(1, 256) if v not in lf][:len(counts) - len(lf)] + list(lf)
        seq = b"".join(bytes([labels[i]]) * c for i, c in enumerate(counts))
        parts = exact_parts(seq, pre_len, post_len)
        assert parts is not None
        out.append(("fibonacci %d" % limit,) + parts)
    return out


CL_MULT = {1: 1, 2: 1, 3: 1, 4: 1, 9: 9, 10: 32, 11: 13, 13: 27, 14: 30, 15: 72}  # a complete code: lengths -> symbols


@functools.lru_cache(maxsize=None)
def cl_limit_case():
    """A record with the dyadic counts 2^(15 - l) of CL_MULT's lengths: three of the 15s are end-of-block, the length
    field's literal zero and its match, the others the byte values 1 .. 184 in a shuffled order.  -> the first shuffle whose
    code-length alphabet passes 7 bits unlimited, and its number"""
    assert sum(n * 2 ** (15 - l) for l, n in CL_MULT.items()) == 2 ** 15
    lens = [l for l, n in sorted(CL_MULT.items()) for _ in range(n)][:-3]
    assert len(lens) == 184
    for shuffle in range(200):
        rng = np.random.default_rng(1000 + shuffle)
        order = rng.permutation(len(lens))
        seq = np.concatenate([np.full(2 ** (15 - lens[i]), 1 + int(v), dtype=np.uint8) for i, v in zip(order, range(len(lens)))])
        seq = bytes(rng.permutation(seq))
        case = exact_case("code-length limit", seq, 40, 11)
        info = model(framed([case])[0])[2]
        if info["cl_k"] >= 1:
            return case, shuffle
    raise AssertionError("no shuffle reaches the limit of the code-length alphabet")


def _dyadic_header_case(name, runs_and_gaps, sig_len):
    """256 tokens with dyadic counts, so that the lengths are known: value 1 has length 1, value 2 length 3, 22 values in
    runs behind gaps length 6 (each 4 times), zero length 6 (the length field's and three single ones), 255 length 7,
    end-of-block and the length field's match length 8.  runs_and_gaps: (gap of unused values, run of used values) ..."""
    values, v = [], 3
    for gap, run in runs_and_gaps:
        v += gap
        values += list(range(v, v + run))
        v += run
    assert len(values) == 22 and v <= 255 and sig_len in values
    seq = bytearray(b"\x01" * 128 + b"\x02" * 32 + b"\xff" * 2)
    for x in values:
        seq += bytes([x]) * 4
    seq = bytearray(np.random.default_rng(len(name)).permutation(np.frombuffer(bytes(seq), dtype=np.uint8)).tobytes())
    seq.remove(sig_len)  # the length field's one byte that is not zero
    pre, sig, post = bytes(seq[:60]), bytes(seq[60:60 + sig_len]), bytes(seq[60 + sig_len:])
    # three single zeros, none next to another or to the length field
    pre = pre[:10] + b"\0" + pre[10:40] + b"\0" + pre[40:]
    post = post[:5] + b"\0" + post[5:]
    return name, pre, sig, post


@functools.lru_cache(maxsize=None)
def header_cases():
    rng = np.random.default_rng(77)
    out = [_dyadic_header_case("gaps 3 10 11 138, runs 4 5 6 7", ((3, 4), (10, 5), (11, 6), (138, 7)), 40),
           _dyadic_header_case("gaps 3 10 11 139, runs 8 7 4 3", ((3, 8), (10, 7), (11, 4), (139, 3)), 45)]
    out.append(("nlit 286", nzb(33, 1), b"\x05" + bytes(259) + b"\x06" + nzb(300, 2), b"\x07"))
    out.append(("nlit 260", nzb(21, 3), rng.integers(1, 9, 700, dtype=np.uint8).tobytes(), nzb(2, 4)))
    out.append(("nlit 259", nzb(9, 5), rng.integers(1, 17, 0x010101, dtype=np.uint8).tobytes(), b""))
    return out


WANT_PAIRS = {(16, 0), (16, 1), (16, 2), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)}


def code_limit_cases():
    return fib_cases() + [cl_limit_case()[0]] + header_cases()


DENSE_AT = 100  # the unit of the record that is the first dense one
DENSE_PRE = 39  # bytes of the first variant's pre


@functools.lru_cache(maxsize=None)
def dense_cases():
    """Four records of 257 units: eight common values with 1024 << j bytes each, and 240 rare values eight times each,
    which the rescaled code gives 14 or 15 bits.  The rare bytes stand together from a unit boundary on: the 128 values
    with the longest codes fill unit DENSE_AT, the others most of the next one.  The variants' pre differs by 0 .. 3 bytes,
    so the units' first bits stand at other places of their dwords."""
    rng = np.random.default_rng(5)
    common = rng.permutation(np.concatenate([np.full(1024 << j, 1 + j, dtype=np.uint8) for j in range(8)])).tobytes()
    rare = list(range(9, 249))

    def build(v, order):
        pre = bytes([1 + 2 * v]) * (DENSE_PRE + v)
        block = b"".join(bytes(rng.permutation(np.repeat(np.array(part, dtype=np.uint8), 8))) for part in (order[:128], order[128:]))
        head = DENSE_AT * U - len(pre) - 8
        return "dense, pre %d" % len(pre), pre, common[v:head + v] + block + common[head + v:], b"\x07\x08"

    probe = build(0, rare)
    lens = model(framed([probe])[0])[2]["lens"]
    order = sorted(rare, key=lambda x: (-lens[x], x))
    return [build(v, order) for v in range(4)]


def dense_units(cases):
    """-> per record (bits of unit DENSE_AT, bits of the next unit, their first bits in the image modulo 32)"""
    recs = framed(cases)
    _, off, _ = model_image(recs)
    out = []
    for k, rec in enumerate(recs):
        info = model(rec)[2]
        bits = D.unit_bits(rec, info["lens"], U)
        starts = D.unit_starts(rec, info["lens"], info["header_bits"], U)
        out.append((bits[DENSE_AT], bits[DENSE_AT + 1], [(8 * off[k] + starts[DENSE_AT + i]) % 32 for i in (0, 1)]))
    return out


@functools.lru_cache(maxsize=None)
def tie_cases():
    """-> (the first short record whose dynamic block is as long as its stored form, the first one byte shorter, how many
    of each kind the search met)"""
    rng = np.random.default_rng(31)
    found, met = {}, {0: 0, 1: 0}
    for trial in range(4000):
        n = int(rng.integers(20, 401))
        alphabet = int(rng.integers(2, 257))
        pre_len = int(rng.integers(0, min(n - 8, 48) + 1))
        body = rng.integers(0, alphabet, n - 8, dtype=np.uint8).tobytes()
        case = ("tie trial %d" % trial, body[:pre_len], body[pre_len:], b"")
        rec = D.frame(*case[1:], 1)
        assert len(rec) == n
        gap = D.stored_length(n) - len(D.dynamic_block(rec))
        if gap in (0, 1):
            met[gap] += 1
            found.setdefault(gap, case)
    return found.get(0), found.get(1), met


@functools.lru_cache(maxsize=None)
def stored_cases():
    rng = np.random.default_rng(41)
    out = []
    for m in (65535, 65536, 131070, 131071, 65535 + 7):
        for pre_len, post_len in ((1024, 0), (20, 30000)):
            body = rng.integers(0, 256, m - 8, dtype=np.uint8).tobytes()
            sig_end = m - 8 - post_len
            out.append(("stored %d, pre %d post %d" % (m, pre_len, post_len), body[:pre_len], body[pre_len:sig_end], body[sig_end:]))
    return out + list(tie_cases()[:2])


@functools.lru_cache(maxsize=None)
def count_cases():
    """200 small records, 8 to about 3000 bytes: zero-heavy bytes, random bytes that go stored, one value, odd and empty
    parts, and twice the record of the length field alone"""
    rng = np.random.default_rng(200)
    out = []
    for k in range(200):
        kind = k % 5
        n = int(rng.integers(0, 2950)) if k % 7 else int(rng.integers(0, 40))
        if kind in (0, 1):
            sig = (rng.integers(0, 8, n, dtype=np.uint8) * (rng.random(n) < 0.45)).astype(np.uint8).tobytes()
        elif kind == 2:
            sig = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 3:
            sig = bytes([1 + k % 255]) * n
        else:
            sig = rng.integers(0, 3, n, dtype=np.uint8).tobytes()
        pre = b"" if k % 11 == 4 else nzb(1 + (3 * k) % 47, k)
        post = b"" if k % 3 == 0 else nzb(1 + (5 * k) % 23, k + 1) + bytes(k % 4)
        if k in (66, 130):
            pre, sig, post = b"", b"", b""
        out.append(("small %d" % k, pre, sig, post))
    return out


SWEEP_L = tuple(range(1, 21)) + tuple(range(255, 263)) + tuple(range(513, 521)) + tuple(range(771, 777))


def sweep_record(L, s, past):
    """A run of L zeros from byte 48 + s of the record on, and a second one whose last zero is the last byte of a unit
    (past = 0) or the first byte of the next one (past = 1): the first unit boundary behind the first run that leaves room,
    1024 where both runs fit below it.  Bytes that are not zero stand around both."""
    pre = nzb(24 + s, L)
    e1 = 48 + s + L
    end = (e1 + 1 + L + U - 1) // U * U + past
    sig = nzb(16, s) + bytes(L) + nzb(end - L - e1, L + s) + bytes(L) + nzb(5 + L % 7, 3)
    rec = D.frame(pre, sig, nzb(s % 3, 9), 1)
    assert rec[47 + s] and not any(rec[48 + s:e1]) and rec[e1] and rec[end - L - 1] and not any(rec[end - L:end]) and rec[end]
    assert end % U == past and (end - past == U or 2 * L + 49 + s > U)
    return "run %d at %d, to %d" % (L, 48 + s, end), pre, sig, nzb(s % 3, 9)


@functools.lru_cache(maxsize=None)
def sweep_cases():
    return [sweep_record(L, s, past) for L in SWEEP_L for s in range(16) for past in ((0, 1) if s < 4 else (0,))]


SEAM_Z = (0, 1, 2, 3, 8, 15, 16, 17, 33, 40)
SEAM_AC = ((3, 5), (16, 16), (250, 9), (9, 250), (258, 258))


@functools.lru_cache(maxsize=None)
def seam_cases():
    """zeros at the end of pre, a signal of zeros, zeros at the start of post: with an empty signal one run goes through
    the length field's eight bytes; the same without anything in front of the zeros, and with an empty pre"""
    out = []
    for z in SEAM_Z:
        for a, c in SEAM_AC:
            out.append(("seam %d | %d | %d" % (a, z, c), nzb(7 + z, a) + bytes(a), bytes(z), bytes(c) + nzb(3, c)))
            out.append(("seam from byte 0, %d | %d | %d" % (a, z, c), bytes(a), bytes(z), bytes(c) + nzb(3, c)))
        out.append(("seam, no pre | %d | %d" % (z, 3 * z), b"", bytes(z), bytes(3 * z) + nzb(2, z)))
    return out


@functools.lru_cache(maxsize=None)
def seam_cases_method_0():
    """signal method 0: an odd number of zero samples"""
    return [("samples %d | %d | %d" % (a, n, c), nzb(5, n) + bytes(a), bytes(2 * n), bytes(c) + nzb(3, c))
            for n in (1, 3, 5, 129, 511) for a, c in SEAM_AC]


@functools.lru_cache(maxsize=None)
def adler_cases():
    return [("0xFF", nzb(30), b"\xff" * 300000, b""), ("0xFF 0x00", nzb(31), b"\xff\x00" * 150000, nzb(1))]


@functools.lru_cache(maxsize=None)
def record_bytes_cases():
    rng = np.random.default_rng(9)
    out = []
    for k, n in enumerate((100, 5000, 37, 4500, 900, 1, 6100, 2048, 300, 0)):
        sig = (rng.integers(0, 6, n, dtype=np.uint8) * (rng.random(n) < 0.5)).astype(np.uint8).tobytes()
        out.append(("record %d" % k, nzb(11 + k, k), sig, nzb(k % 3, k)))
    return out


# ------------------------------------------------------------------ CPU: the fixtures are what they claim

def test_model_image_is_the_models():
    """model_image puts the kept streams together as D.image does"""
    recs = framed(count_cases()[:70])
    assert model_image(recs) == D.image(recs)


def test_unit_helpers():
    """the units' bits and end-of-block are the block's bits; a match counts where it opens"""
    for case in (battery()[5], battery()[-2], count_cases()[0], dense_cases()[0]):
        rec = D.frame(*case[1:], 1)
        info = {}
        block = D.dynamic_block(rec, info)
        bits = D.unit_bits(rec, info["lens"], U)
        starts = D.unit_starts(rec, info["lens"], info["header_bits"], U)
        assert len(bits) == len(starts) == (len(rec) + U - 1) // U and starts[0] == 80 + info["header_bits"]
        assert [starts[i + 1] - starts[i] for i in range(len(bits) - 1)] == bits[:-1]
        assert len(block) == (info["header_bits"] + sum(bits) + info["lens"][D.EOB] + 7) // 8
    lens = [8] * D.NLIT
    assert D.unit_bits(b"\x01" * 1022 + bytes(300), lens, U) == [8 * 1023 + 8 + 1, 8 + 3 + 1]  # .. 0, match 258 | match 41
    assert D.unit_bits(b"\x01" * 1024 + bytes(2), lens, U) == [8 * 1024, 16]


def test_rescale_depth():
    cases = fib_cases()
    inflates(cases)
    for (name, _, _, _), rec, k, unlimited in zip(cases, framed(cases), (2, 3), (22, 25)):
        stream, raw, info = model(rec)
        print(name, len(rec), "bytes: k", info["k"], "unlimited", max(D._build(info["hist"])), "maxlen", info["maxlen"])
        assert sorted(c for c in info["hist"] if c)[:6] == [1, 1, 1, 2, 3, 5]
        assert max(D._build(info["hist"])) == unlimited
        assert info["k"] == k and info["maxlen"] <= 15 and raw == 0
    assert [len(r) for r in framed(cases)] == [46365 + 6, 196415 + 5]  # the counts and the length field's zeros


def test_code_length_alphabet_limit():
    case, shuffle = cl_limit_case()
    inflates([case])
    rec = framed([case])[0]
    stream, raw, info = model(rec)
    print("shuffle", shuffle, len(rec), "bytes: k", info["k"], "cl_k", info["cl_k"], "unlimited", max(D._build(info["cl_hist"])))
    assert max(D._build(info["cl_hist"])) > 7 and info["cl_k"] >= 1 and raw == 0
    assert info["k"] == 0 and sorted(l for l in info["lens"] if l) == sorted(l for l, n in CL_MULT.items() for _ in range(n))
    cll = D.huff_lengths(info["cl_hist"], 7)[0]
    assert max(cll) == 7


def test_header_fields():
    cases = code_limit_cases()
    inflates(cases)
    infos = {name: model(rec)[2] for (name, _, _, _), rec in zip(cases, framed(cases))}
    for name, info in infos.items():
        print(name, "nlit", info["nlit"], "ncl", info["ncl"], "cl_k", info["cl_k"],
              sorted({(s, ev) for s, _, ev in info["cl_syms"] if s >= 16}))
    # the sequence ends in the distance code's length 1, and 1 is the 18th of the order: ncl is 18, or 19 with a length 15
    everything = [model(rec)[2] for rec in framed(count_cases() + sweep_cases() + seam_cases())] + list(infos.values())
    assert {i["ncl"] for i in everything} == {18, 19}
    assert all((i["ncl"] == 19) == (i["maxlen"] == 15) for i in everything)
    assert infos["nlit 260"]["ncl"] == 18 and infos["fibonacci 300000"]["ncl"] == 19
    # a framed record's length field ends in five zeros or more (a signal below 2^24 bytes): a match, nlit 259 at least
    assert min(i["nlit"] for i in everything) == 259
    assert {infos[n]["nlit"] for n in ("nlit 259", "nlit 260", "nlit 286")} == {259, 260, 286}
    for name in ("gaps 3 10 11 138, runs 4 5 6 7", "gaps 3 10 11 139, runs 8 7 4 3"):
        lens = infos[name]["lens"]
        assert infos[name]["nlit"] == 261 and (lens[0], lens[1], lens[2], lens[255], lens[256], lens[260]) == (6, 1, 3, 7, 8, 8)
        assert sorted(set(lens)) == [0, 1, 3, 6, 7, 8] and lens.count(6) == 23
    pairs = set()
    for info in infos.values():
        pairs |= {(s, ev) for s, _, ev in info["cl_syms"] if s >= 16}
    assert pairs >= WANT_PAIRS, WANT_PAIRS - pairs
    second = [(s, ev) for s, _, ev in infos["gaps 3 10 11 139, runs 8 7 4 3"]["cl_syms"]]
    at = second.index((18, 127))
    assert second[at + 1] == (0, 0) and second[at + 2][0] == 6  # 139 zeros: 138 and one by itself
    # bare records, the model alone: no match at all, and the match of three alone
    for rec, nlit in ((bytes(range(1, 200)) * 3, 257), (b"\x05" + bytes(4) + b"\x06" * 40 + bytes(4) + b"\x07", 258)):
        info = {}
        stream, raw = D.deflate_record(rec, info)
        assert zlib.decompress(stream) == rec and info["nlit"] == nlit


def test_dense_units():
    cases = dense_cases()
    inflates(cases)
    forward, backward = dense_units(cases), dense_units(cases[::-1])
    for (name, _, _, _), rec, d in zip(cases, framed(cases), forward):
        info = model(rec)[2]
        print(name, len(rec), "bytes: k", info["k"], "units of", d[0], "and", d[1], "bits at", d[2])
        assert info["k"] >= 1 and info["maxlen"] == 15 and model(rec)[1] == 0
        assert d[0] >= 14848 and d[1] >= 12000 and d[0] <= 15 * U
    print("in reverse order at", [d[2] for d in backward])
    offsets = [o for d in forward for o in d[2]]
    assert max(offsets) >= 24 and min(offsets) <= 8, offsets
    moved = sum(f[2] != b[2] for f, b in zip(forward, backward[::-1]))
    assert moved >= 3, "in reverse order the records' dense units stand at other bits of their dwords"


def test_tie_records():
    stored, dynamic, met = tie_cases()
    print("met", met)
    assert stored is not None and dynamic is not None
    inflates([stored, dynamic])
    for case, gap, raw in ((stored, 0, 1), (dynamic, 1, 0)):
        rec = D.frame(*case[1:], 1)
        assert 20 <= len(rec) <= 400 and D.stored_length(len(rec)) - len(D.dynamic_block(rec)) == gap
        assert model(rec)[1] == raw


def test_stored_seams_on_the_model():
    cases = stored_cases()
    inflates(cases)
    recs = framed(cases)
    assert [len(r) for r in recs[:10]] == [65535, 65535, 65536, 65536, 131070, 131070, 131071, 131071, 65542, 65542]
    assert [model(r)[1] for r in recs] == [1] * 11 + [0]
    assert [len(model(r)[0]) - len(r) - 6 for r in recs[:10]] == [5, 5, 10, 10, 10, 10, 15, 15, 10, 10]
    seams = {1024: [], 20: []}  # where a block ends and another begins: in the signal, or in post
    for (_, pre, sig, _), rec in zip(cases[:10], recs):
        for at in range(65535, len(rec), 65535):
            seams[len(pre)].append("signal" if len(pre) + 8 <= at < len(pre) + 8 + len(sig) else "post")
    assert seams[1024] == ["signal"] * 5 and seams[20] == ["post", "signal", "signal", "post", "post"]


def test_small_records():
    cases = count_cases()
    inflates(cases)
    sizes = [len(r) for r in framed(cases)]
    raws = [model(r)[1] for r in framed(cases)]
    assert len(cases) == 200 and min(sizes) == 8 and sizes[66] == sizes[130] == 8 and 2900 < max(sizes) < 3100
    assert 20 < sum(raws) < 180 and any(not p for _, p, _, _ in cases) and any(not q for _, _, _, q in cases)
    for lo, hi in ((0, 63), (63, 65), (65, 128), (128, 130), (130, 200)):
        assert {0, 1} == set(raws[lo:hi]) or hi - lo == 2


def test_run_sweep_records():
    cases = sweep_cases()
    assert len(cases) == len(SWEEP_L) * 20 == 840
    inflates(cases)
    inflates(seam_cases())
    inflates(seam_cases_method_0(), 0)
    whole = [c for c in seam_cases() if not c[2]]  # an empty signal: one run through all of the length field
    for name, pre, sig, post in whole:
        rec = D.frame(pre, sig, post, 1)
        run = len(pre) - len(pre.rstrip(b"\0")) + 8 + len(post) - len(post.lstrip(b"\0"))
        first = len(pre.rstrip(b"\0"))
        assert not any(rec[first:first + run]) and rec[first + run] and (first == 0 or rec[first - 1])
    assert any(not c[1] for c in seam_cases()) and len(framed([("", b"", b"", b"")])[0]) == 8
    for name, pre, sig, post in seam_cases_method_0():
        assert len(sig) % 4 == 2 and D.frame(pre, sig, post, 0)[len(pre):len(pre) + 8] == (len(sig) // 2).to_bytes(8, "little")


def test_adler_records():
    cases = adler_cases()
    inflates(cases)
    for rec in framed(cases):
        stream, raw, _ = model(rec)
        assert raw == 0 and stream[-4:] == zlib.adler32(rec).to_bytes(4, "big") and len(rec) > 300000


# ------------------------------------------------------------------ GPU: the device against the model

def names_of(cases):
    return [c[0] for c in cases]


def host_form(cases, signal_method=1):
    """the host-pointer form against the model -> the image"""
    want, want_off, want_raw = model_image(framed(cases, signal_method))
    pres, sigs, posts = arrays(cases)
    image, rec_off, raw = press.blow5_deflate_batch_host(pres, sigs, posts, signal_method)
    assert [int(x) for x in rec_off] == want_off
    assert [int(x) for x in raw] == want_raw
    assert image.tobytes() == want, first_difference(image, want, want_off, names_of(cases))
    return image


def device_form(cases, signal_method=1):
    """the device-resident form against the model: the sizes call, then image, rec_off, raw and the zeros behind"""
    import torch
    want, want_off, want_raw = model_image(framed(cases, signal_method))
    b = DeviceBatch(cases, signal_method)
    b.load()
    need = b.sizes()
    b.run()
    torch.cuda.synchronize()
    assert [int(x) for x in need.cpu().numpy()] == [want_off[k + 1] - want_off[k] for k in range(b.n)]
    check_device(b, want, want_off, want_raw, names_of(cases))
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 200])
def test_gpu_record_counts_host_form(lib, n):
    host_form(count_cases()[:n])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 129, 200])
def test_gpu_record_counts_device_form(lib, n):
    device_form(count_cases()[:n])


@pytest.mark.gpu
def test_gpu_refusals_in_every_group(lib):
    """a failed signal at 5 and 70, a pre that leaves its arena at 63, 64 and 191: they take no byte, the others follow"""
    import torch
    cases = count_cases()
    recs = framed(cases)
    _, full_off, _ = model_image(recs)
    b = DeviceBatch(cases)
    b.load()
    refused = (5, 63, 64, 70, 191)
    for r in (5, 70):
        b.sig_len[r] = -1
    for r in (63, 64, 191):
        b.tab[4 * r + 1] = 1 << 40
    need = b.sizes()
    b.run()
    torch.cuda.synchronize()
    keep = [k for k in range(b.n) if k not in refused]
    want, off, raw = model_image([recs[k] for k in keep])
    want_off, want_raw, at = [], [], 0
    for k in range(b.n):
        want_off.append(off[at])
        if k in refused:
            want_raw.append(REFUSED)
        else:
            want_raw.append(raw[at])
            at += 1
    want_off.append(off[-1])
    assert [int(x) for x in need.cpu().numpy()] == [-1 if k in refused else full_off[k + 1] - full_off[k] for k in range(b.n)]
    assert all(want_off[k + 1] == want_off[k] for k in refused)
    check_device(b, want, want_off, want_raw, names_of(cases))


@pytest.mark.gpu
def test_gpu_image_cap_behind_the_first_group(lib):
    """image_cap at record 100: what ends inside it is the model's, the others are not written, rec_off is complete"""
    import torch
    cases = count_cases()
    want, want_off, want_raw = model_image(framed(cases))
    b = DeviceBatch(cases)
    b.load()
    cap = (want_off[100] + 3) // 4 * 4
    b.image = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    b.run()
    torch.cuda.synchronize()
    fits = [want_off[k + 1] <= cap for k in range(b.n)]
    assert fits[99] and not fits[101] and not any(fits[101:])
    assert [int(x) for x in b.rec_off.cpu().numpy()] == want_off
    assert [int(x) for x in b.raw.cpu().numpy()] == [want_raw[k] if fits[k] else REFUSED for k in range(b.n)]
    end = max(want_off[k + 1] for k in range(b.n) if fits[k])
    img = b.image.cpu().numpy()
    assert img[:end].tobytes() == want[:end], first_difference(img[:end], want[:end], want_off, names_of(cases))
    assert not img[end:].any()


@pytest.mark.gpu
def test_gpu_record_bytes(lib):
    """record_bytes too small: every record refused, nothing written; the same batch at once with the exact figure, and
    with far more, is the model's"""
    import torch
    cases = record_bytes_cases()
    recs = framed(cases)
    assert sum(len(r) > 4096 for r in recs) == 3 and sum((len(r) + U - 1) // U for r in recs) > len(recs)
    want, want_off, want_raw = model_image(recs)
    b = DeviceBatch(cases)
    exact = b.record_bytes
    assert exact == sum(len(r) for r in recs)
    b.load()
    b.record_bytes = 0
    need = b.sizes()
    b.run()
    torch.cuda.synchronize()
    assert [int(x) for x in need.cpu().numpy()] == [-1] * b.n
    assert [int(x) for x in b.raw.cpu().numpy()] == [REFUSED] * b.n
    assert [int(x) for x in b.rec_off.cpu().numpy()] == [0] * (b.n + 1)
    assert not b.image.cpu().numpy().any()
    for figure in (exact, 2 * exact + 1000000):
        b.record_bytes = figure
        need = b.sizes()
        b.run()
        torch.cuda.synchronize()
        assert [int(x) for x in need.cpu().numpy()] == [want_off[k + 1] - want_off[k] for k in range(b.n)]
        check_device(b, want, want_off, want_raw, names_of(cases))


@pytest.mark.gpu
def test_gpu_code_limits(lib):
    """k = 2 and 3, the code-length alphabet at its limit, ncl 18 and 19, nlit 259 .. 286, every repeat code's edges"""
    cases = code_limit_cases()
    host_form(cases)
    device_form(cases)


@pytest.mark.gpu
def test_gpu_dense_units(lib):
    """two nearly full bit windows side by side, at eight places of the image's dwords"""
    cases = dense_cases()
    host_form(cases)
    device_form(cases)
    host_form(cases[::-1])
    device_form(cases[::-1])


def device_streams(image, cases, signal_method=1):
    for k, rec in enumerate(framed(cases, signal_method)):
        ln, = struct.unpack("<Q", image[:8].tobytes())
        assert zlib.decompress(image[8:8 + ln].tobytes()) == rec, cases[k][0]
        yield image[8:8 + ln].tobytes(), rec
        image = image[8 + ln:]
    assert image.size == 0


@pytest.mark.gpu
def test_gpu_stored_seams_and_ties(lib):
    """stored blocks of 65 535 bytes exactly, one more, two exactly, and one more; the seam in the signal and in post; the
    dynamic block as long as the stored form and one byte shorter.  zlib reads the device's streams themselves."""
    cases = stored_cases()
    image = host_form(cases)
    assert len(list(device_streams(image, cases))) == len(cases)
    b = device_form(cases)
    assert [int(x) for x in b.raw.cpu().numpy()] == [1] * 11 + [0]
    assert len(list(device_streams(b.image.cpu().numpy()[:int(b.rec_off[-1])], cases))) == len(cases)


@pytest.mark.gpu
def test_gpu_run_sweep(lib):
    """runs of every length around 1, 258, 516 and 774 from every place of the 16-byte grid, and ending at a unit's end"""
    cases = sweep_cases()
    for lo in range(0, len(cases), 300):
        host_form(cases[lo:lo + 300])
    device_form(cases)


@pytest.mark.gpu
def test_gpu_run_seams(lib):
    """one run through pre, the length field, the signal and post; an empty pre; zero samples under signal method 0"""
    host_form(seam_cases())
    device_form(seam_cases())
    host_form(seam_cases_method_0(), 0)
    device_form(seam_cases_method_0(), 0)


@pytest.mark.gpu
def test_gpu_adler_at_its_largest(lib):
    cases = adler_cases()
    image = host_form(cases)
    for stream, rec in device_streams(image, cases):
        assert stream[-4:] == zlib.adler32(rec).to_bytes(4, "big")
