"""GPU: k_huf_sync's pair loop - a lane takes two subsequences in a row (A, then B), runs up once over the end of B,
scans A from its guess and B from where A ended; a wave's ticket is half a tile (128 subsequences).

The reads sit on the boundaries of that loop: payloads that end inside A, between A and B, inside B, at a pair's and at
a tile's end; subsequences full of the shortest codes; long codes across the seam between A and B; bits that are no
code and payloads cut short in A, in B and in B's run-up; the 128- and 64-bit subsequences of tables with short codes;
a table that never synchronises.  Every read is decoded alone and in one batch and compared with the oracle."""
import numpy as np
import pytest

from honours_amd import press
from test_gpu_parity import TABLES, _canonical_table, _write_table
from test_huffman_emit_waits import LENS, long_deltas, subsequence_counts, table_lens, with_deltas, zd_of
from test_huffman_unit_plan import (check_alone, check_batch, exceptions_of, oracle_stream, payload_bytes,
                                    prefix_with_payload, walk)

pytestmark = pytest.mark.gpu

M = "shuffman_vbe21_zd"
SUB = 32  # payload bytes of a subsequence for the NA12878 table (256 bits); a lane takes 64, a wave 4096, a tile 8192
# subsequences: one, A + B of a lane, one more; around the second unit of a pair, a pair, the second pair's second
# unit, a tile, and half a pair into the next tile
KS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 384, 385)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    press.load_library()
    press.load_table()
    yield


class foreign_table:
    """oracle and device under another code table; the NA12878 table comes back behind it"""

    def __init__(self, oracle, path):
        self.oracle, self.path = oracle, path

    def __enter__(self):
        self.oracle.load_table(self.path)
        press.use_table(self.path)

    def __exit__(self, *exc):
        self.oracle.load_table()
        press.use_table()


def write_partial_table(path, lens):
    """a table file that lists len(lens) < 256 symbols, canonical codes in symbol order (the lengths do not decrease)"""
    assert list(lens) == sorted(lens)
    code, prev, blob = 0, lens[0], bytearray(len(lens).to_bytes(4, "big") + bytes(4))
    for sy, ln in enumerate(lens):
        code <<= ln - prev
        prev = ln
        bits = int(format(code, "0%db" % ln)[::-1], 2)
        blob += bytes([sy, ln]) + bits.to_bytes((ln + 7) // 8, "little")
        code += 1
    assert code <= 1 << prev
    open(path, "wb").write(bytes(blob))
    return code < 1 << prev  # the all-ones pattern of the longest length is no code


def read_with_payload(oracle, lens, base, target):
    """a read whose Huffman payload is `target` bytes: a prefix of `base` (no exceptions), then samples that repeat
    the last value - delta 0, whose code is short, so the payload grows by at most a byte per sample (under a table
    with 9- or 10-bit codes next to 1- or 2-bit ones a prefix of base alone steps over sizes)"""
    assert 0 < lens[0] <= 8
    bits = np.cumsum(lens[zd_of(base.astype(np.int16))[1:]])
    m = int(np.searchsorted(bits, 8 * target - 24))  # codes of the prefix: 24 bits or more below the target
    have = int(bits[m - 1]) if m else 0
    assert m < bits.size and 8 * (target - 1) + 1 > have
    t = -(-(8 * (target - 1) + 1 - have) // int(lens[0]))
    sig = np.concatenate([base[:m + 1], np.full(t, base[m])]).astype(np.int16)
    assert payload_bytes(oracle_stream(oracle, sig)) == target, target
    return sig


def check_all(oracle, sigs):
    streams = [check_alone(oracle, s) for s in sigs]
    check_batch(oracle, streams, [s.size for s in sigs])
    return streams


# ---------------------------------------------------------------- where a payload ends

def test_payload_sizes_around_the_pair_loop(oracle):
    """payloads of k subsequences and a byte less and more: the read ends inside A, exactly between A and B, inside B,
    at a unit's, a pair's and a tile's end; alone, and in one batch, where pairs of different reads share a workgroup"""
    base = walk(24000, 41)
    sigs = [prefix_with_payload(oracle, base, k * SUB + d) for k in KS for d in (-1, 0, 1)]
    check_all(oracle, sigs)


@pytest.mark.parametrize("name", ["min2_incomplete", "min1_incomplete"])
def test_payload_sizes_with_short_subsequences(oracle, tmp_path, name):
    """the same sizes in subsequences of 128 bits (a 2-bit shortest code) and of 64 bits (a 1-bit one): the other
    two instances of the kernel, with 9 and 5 payload dwords per lane"""
    lens = np.array(TABLES[name], dtype=np.int64)
    sub = 16 if lens.min() >= 2 else 8
    path = str(tmp_path / (name + ".huffman"))
    _write_table(path, TABLES[name], _canonical_table(TABLES[name]))
    rng = np.random.default_rng(len(name))
    steps = rng.integers(-1, 2, size=60000) if sub == 16 else np.zeros(60000, dtype=np.int64)
    far = rng.random(steps.size) < (0.05 if sub == 16 else 0.1)
    steps[far] = rng.integers(-9, 10, size=int(far.sum()))  # the 10-bit (9-bit) codes: subsequences of 1 .. 64 codes
    base = (np.cumsum(steps) + 500).astype(np.int64)
    with foreign_table(oracle, path):
        sigs = [read_with_payload(oracle, lens, base, k * sub + d) for k in KS for d in (-1, 0, 1)]
        check_all(oracle, sigs)


# ---------------------------------------------------------------- what A and B hold

def shortest_walk(n):
    """a walk whose deltas all take the table's shortest code (4 bits: 64 codes per subsequence, 128 per lane - more
    than one scan's accumulator counts), kept near 500"""
    short = [(int(z) >> 1) ^ -(int(z) & 1) for z in np.nonzero(LENS == LENS[LENS > 0].min())[0]]
    assert min(short) < 0 < max(short), short
    a, v = np.empty(n, dtype=np.int64), 500
    for i in range(n):
        a[i] = v
        v += min(short) if v > 500 else max(short)
    # (not a plain zig-zag: three steps in ten change places with the next one)
    rng = np.random.default_rng(5)
    steps = np.diff(a, prepend=a[0])
    flip = np.nonzero(rng.random(n) < 0.3)[0]
    for i in flip[(flip > 0) & (flip < n - 1)]:
        steps[i], steps[i + 1] = steps[i + 1], steps[i]
    return np.cumsum(steps) + 500


def test_a_stretch_of_the_shortest_codes(oracle):
    """three and a half pairs of subsequences with 64 codes each; then with an exception inside an A and inside a B"""
    n = 1 + 64 * (3 * 128 + 64) + 7
    base = shortest_walk(n)
    sig = base.astype(np.int16)
    counts = subsequence_counts(sig, LENS, 8 * SUB)
    assert counts.size == 3 * 128 + 65 and (counts[:-1] == 64).all()
    exc = base.copy()
    for at, d in ((1 + 64 * 10 + 20, 700), (1 + 64 * 13 + 20, -700), (1 + 64 * 128 + 5, 700), (1 + 64 * 255 + 60, -700)):
        exc[at:] += d  # (subsequences 10 and 128: an A; 13 and 255: a B)
    exc = exc.astype(np.int16)
    assert exceptions_of(oracle_stream(oracle, exc)) == 4
    check_all(oracle, [sig, exc, sig[:1 + 64 * 129], exc[:1 + 64 * 14]])


def seam_straddles(sig, lens, sub_bits):
    """codes that start in an A and end in its B (the subsequence pairs of a lane: 2 m, 2 m + 1)"""
    ln = lens[zd_of(sig)[1:]]
    start = np.concatenate([[0], np.cumsum(ln)])[:-1]
    sa, sb = start // sub_bits, (start + ln - 1) // sub_bits
    return int(((sa != sb) & (sa % 2 == 0)).sum())


def long_code_reads(lens, n, seed):
    """reads whose deltas take the table's codes of 13 bits and more every other sample (all the time, the stream
    would outgrow the reference's bound), and every fourth"""
    rng = np.random.default_rng(seed)
    zs = np.nonzero(lens >= 13)[0]
    d = np.array([(int(z) >> 1) ^ -(int(z) & 1) for z in zs])
    up, down = d[d > 0], d[d < 0]
    assert up.size and down.size
    sigs = []
    for every in (2, 4):
        steps, v = rng.integers(-3, 4, size=n), 0
        for i in range(1, n, every):
            steps[i] = rng.choice(down if v > 0 else up)
            v += steps[i]
        steps[0] = 500
        sigs.append(np.cumsum(steps).astype(np.int16))
    return sigs


def test_long_codes_across_the_seam(oracle, tmp_path):
    """codes of 13 to 24 bits at high density - many of them start in a lane's A and end in its B, and A's reach
    (the dword both subsequences share) is B's first"""
    sigs = long_code_reads(LENS, 9000, 61)
    assert all(seam_straddles(s, LENS, 8 * SUB) >= 20 for s in sigs)
    for d in long_deltas(LENS):  # a long code alone in B's first bits, and as A's last and B's first
        base = walk(900, 62, spread=3)
        sigs += [with_deltas(base, [i], d) for i in range(60, 76)] + [with_deltas(base, [i, i + 1], d) for i in range(60, 76)]
    check_all(oracle, sigs)
    name = "long_codes"  # (more long prefixes than the second-level tables take: the trie instance)
    lens = np.array(TABLES[name], dtype=np.int64)
    path = str(tmp_path / (name + ".huffman"))
    _write_table(path, TABLES[name], _canonical_table(TABLES[name]))
    with foreign_table(oracle, path):
        sigs = long_code_reads(lens, 9000, 63)
        assert all(seam_straddles(s, lens, 8 * SUB) >= 20 for s in sigs)
        check_all(oracle, sigs)


# ---------------------------------------------------------------- bits that are no code; payloads cut short

# the damage starts in an even subsequence (an A), in an odd one (a B), and in the last 128 bits of an odd one (B's
# run-up: the right neighbour's guess); byte offsets in the payload
DAMAGE_AT = (6 * SUB + 10, 9 * SUB + 3, 21 * SUB + 16 + 5, 128 * SUB + 1, 255 * SUB + 30, 131 * SUB + 20)


def damaged_streams(oracle, tmp_path):
    """a table of 23 symbols whose all-ones pattern is no code, a read under it, and per place of DAMAGE_AT its stream
    with three bytes of ones there: (with the whole count announced, n), (with a count that ends in front of the
    damage, n).  To be used under foreign_table(oracle, path)"""
    lens = [4] * 8 + [5] * 15
    path = str(tmp_path / "partial23.huffman")
    assert write_partial_table(path, lens)
    rng = np.random.default_rng(71)
    sig = (np.cumsum(rng.integers(-11, 12, size=20000)) + 500).astype(np.int16)  # zig-zag deltas 0 .. 22
    oracle.load_table(path)
    try:
        full = oracle_stream(oracle, sig)
    finally:
        oracle.load_table()
    assert exceptions_of(full) == 0 and payload_bytes(full) > 258 * SUB
    pay = 2 + 4 + 4  # header, exception count, the count of one-byte values
    whole, short = [], []
    for at in DAMAGE_AT:
        bad = full[:pay + at] + b"\xff\xff\xff" + full[pay + at + 3:]
        want = 8 * at // 5 - 10  # codes of at most 5 bits: these end in front of the damage
        whole.append((bad, sig.size))
        short.append((bad[:6] + want.to_bytes(4, "big") + bad[10:], want + 1))
    return path, sig, full, whole, short


def test_bits_that_are_no_code_behind_the_count(oracle, tmp_path):
    """the announced count ends in front of the damage: the oracle delivers the read, and the subsequences behind,
    which the scans still run through (an A that ends in bits that are no code, its B listed with the guess 0; a run-up
    that ends in them), must not matter.  Alone and in one batch with the undamaged read"""
    path, sig, full, _, short = damaged_streams(oracle, tmp_path)
    with foreign_table(oracle, path):
        check_alone(oracle, sig)
        for st, n in short:
            assert oracle.depress(M, st, n)[0] == 0
            check_alone(oracle, sig, stream=st, n=n)
        check_batch(oracle, [st for st, _ in short] + [full], [n for _, n in short] + [sig.size])


def test_bits_that_are_no_code_in_front_of_the_count(oracle, tmp_path):
    """the whole count announced: the oracle refuses the read at the first bits that are no code (po_shuff_decode), and
    so does the device (k_huf_chain walks the subsequence the scans stopped in through the trie; before that it ended
    the read there as at the end of its input and delivered the 349 to 14 076 samples in front) - alone, and in one
    batch, where the undamaged read beside them stands"""
    path, sig, full, whole, _ = damaged_streams(oracle, tmp_path)
    with foreign_table(oracle, path):
        for (st, n), at in zip(whole, DAMAGE_AT):
            ro, _ = oracle.depress(M, st, n)
            rg, bg = press.depress(M, st, n)
            print("damage at payload byte %d: device (%d, %s samples), oracle (%d, -)" % (at, rg, None if rg else bg.size, ro))
        for st, n in whole:
            assert oracle.depress(M, st, n)[0] != 0
            check_alone(oracle, sig, stream=st, n=n)
        check_batch(oracle, [st for st, _ in whole] + [full], [n for _, n in whole] + [sig.size])
        # and cut short under this table: the bits in front of the cut are the beginning of a code or of none
        cuts = [full[:2 + 4 + 4 + at] for at in DAMAGE_AT] + [st[:2 + 4 + 4 + at + 2] for (st, _), at in zip(whole, DAMAGE_AT)]
        for st in cuts:
            check_alone(oracle, sig, stream=st)
        check_batch(oracle, cuts + [full], [sig.size] * (len(cuts) + 1))


def test_payloads_cut_short(oracle):
    """a stream that ends inside an A, inside a B and in a B's last 128 bits: the decoder delivers what the oracle does"""
    sig = walk(24000, 72).astype(np.int16)
    full = oracle_stream(oracle, sig)
    assert exceptions_of(full) == 0 and payload_bytes(full) > 258 * SUB
    streams = [full[:2 + 4 + 4 + at] for at in DAMAGE_AT + (2 * SUB, 3 * SUB, 128 * SUB, 1, SUB)]
    for st in streams:
        check_alone(oracle, sig, stream=st)
    check_batch(oracle, streams + [full], [sig.size] * (len(streams) + 1))


# ---------------------------------------------------------------- a table that never synchronises

def test_a_table_that_never_synchronises(oracle, tmp_path):
    """every code length a multiple of 3 and 128-bit subsequences: the repair rounds settle little and k_huf_serial
    walks the reads - payloads of 2, 128 and 129 subsequences (a lane's pair, a pair of units and one more)"""
    lens = [3] * 7 + [6] * 7 + [9] * 7 + [12] * 7 + [15] * 7 + [18] * 7 + [21] * 7 + [24] * 8  # Kraft sum 1
    path = str(tmp_path / "mult3.huffman")
    assert not write_partial_table(path, lens)
    rng = np.random.default_rng(73)
    steps = rng.integers(-3, 4, size=30000)
    far = rng.random(steps.size) < 0.05
    steps[far] = rng.integers(-28, 29, size=int(far.sum()))  # zig-zag values up to 56: the long codes
    base = (np.cumsum(steps) + 500).astype(np.int64)
    with foreign_table(oracle, path):
        tl = table_lens(path)
        sigs = [read_with_payload(oracle, tl, base, k * 16) for k in (2, 128, 129)]
        check_all(oracle, sigs)


# ---------------------------------------------------------------- scratch

def test_two_batches_on_one_context(oracle):
    """two batch calls back to back - a large one, then a small one whose pairs use a part of the same records and
    words - and again behind a fill of every scratch buffer"""
    base = walk(24000, 74)
    big = [prefix_with_payload(oracle, base, k * SUB + 1) for k in (385, 129, 64)]
    small = [prefix_with_payload(oracle, base, k * SUB) for k in (3, 65)]
    calls = [([oracle_stream(oracle, s) for s in sigs], [s.size for s in sigs]) for sigs in (big, small)]
    for fill in (None, 0xA5, 0xFF):
        if fill is not None:
            if not hasattr(press, "scratch_fill"):
                break
            press.scratch_fill(fill)
        for streams, ns in calls:
            check_batch(oracle, streams, ns)
