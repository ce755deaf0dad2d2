"""GPU: what k_huf_emit does between its waits - the sample rounds of a unit (with the unit's exceptions held in the
wave, at most 64, or searched in memory), the tickets that hand out units, and the steps of the decode loop.

Every read is compared with the oracle, alone (press.depress) and in one batch (press.depress_batch_host).  A unit is
2048 payload bytes - about 3 000 samples - of the NA12878 table; `units_of` restates which samples and exceptions a
unit writes, so that the cases can say where they put theirs."""
import numpy as np
import pytest

from honours_amd import press

pytestmark = pytest.mark.gpu

METHODS = ("shuffman_vbe21_zd", "shuffman_vbbe21_zd", "shuffman_vbsbe21_zd", "shuffman_vbsse21_zd")
M = METHODS[0]
UNIT_BITS = 8 * 2048   # payload bits of a unit for the NA12878 table (64 subsequences of 256 bits)
SUB_BITS = 256
ROUND = 1024           # samples a wave writes per round


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    press.load_library()
    press.load_table()
    yield


def table_lens(path=press.TABLE_PATH):
    """code length of every one-byte value (the table file: u32 count, u32, then symbol, bits, the bits' bytes)"""
    d = open(path, "rb").read()
    lens, p = np.zeros(256, dtype=np.int64), 8
    for _ in range(int.from_bytes(d[:4], "big")):
        lens[d[p]] = d[p + 1]
        p += 2 + (d[p + 1] + 7) // 8
    return lens


LENS = table_lens()


def zd_of(sig):
    s = np.asarray(sig).astype(np.int64)
    d = np.diff(s, prepend=0)
    return np.where(d >= 0, 2 * d, -2 * d - 1)


def units_of(sig, lens=LENS, unit_bits=UNIT_BITS):
    """the units of a read as k_huf_chain plans them: a list of (Ia, Ib, ecnt) - the unit writes the samples [Ia, Ib),
    ecnt of them exceptions.  Sample i >= 1 is an exception if its zig-zag delta is above 255, else the next
    one-byte value; a value belongs to the unit its code starts in, an exception to the unit of the value behind it
    (the last unit: also those behind its last value), sample 0 to the first."""
    z = zd_of(sig)[1:]
    exc = z > 255
    start = np.concatenate([[0], np.cumsum(np.where(exc, 0, lens[np.minimum(z, 255)]))])[:-1]  # a value's first bit
    unit = start // unit_bits  # (an exception: the unit of the next value, which starts at the same bit)
    nv = int((~exc).sum())
    last = int(unit[~exc][-1]) if nv else 0
    unit = np.minimum(unit, last)
    out = []
    for u in range(last + 1):
        idx = np.nonzero(unit == u)[0]
        ia = int(idx[0]) + 1 if u else 0
        out.append((ia, int(idx[-1]) + 2, int(exc[idx].sum())))
    return out


def walk(n, seed, spread=12):
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.integers(-spread, spread + 1, size=n)) + 500).astype(np.int64)


def with_exceptions(a, at):
    """exceptions (|delta| >= 128) at the given sample indices (>= 1), every other one up, every other one down"""
    a = a.copy()
    for j, i in enumerate(sorted(at)):
        a[i:] += 700 if j % 2 == 0 else -700
    assert a.min() >= -8000 and a.max() <= 8000  # (room for the shifted variants)
    return a.astype(np.int16)


def exceptions_of(stream):
    return int.from_bytes(stream[2:6], "little")


def oracle_stream(oracle, m, sig):
    ret, st = oracle.press(m, sig)
    assert ret == 0
    return st


def check(oracle, m, sigs, alone=True):
    """every read through press.press / press.depress alone, then all of them through one batch call"""
    streams = []
    for i, sig in enumerate(sigs):
        st = oracle_stream(oracle, m, sig)
        streams.append(st)
        if not alone:
            continue
        ret, got = press.press(m, sig)
        assert ret == 0 and got == st, press.last_error()
        ro, bo = oracle.depress(m, st, sig.size)
        rg, bg = press.depress(m, st, sig.size)
        assert ro == 0 and rg == 0 and np.array_equal(bo, sig), (m, i, sig.size)
        assert np.array_equal(bg, bo), (m, i, sig.size, np.nonzero(bg != bo)[0][:4])
    backs = press.depress_batch_host(m, streams, [s.size for s in sigs])
    for i, (sig, bk) in enumerate(zip(sigs, backs)):
        assert bk is not None and bk.size == sig.size, (m, i, sig.size)
        assert np.array_equal(bk, sig), (m, i, sig.size, np.nonzero(bk != sig)[0][:4])
    return streams


def shifted(sigs):
    """the reads and the same reads with two zero bits below every sample (ex-zd's qts shift undone by the decoder)"""
    return list(sigs) + [(s.astype(np.int32) * 4).astype(np.int16) for s in sigs]


# ---------------------------------------------------------------- rounds

BASE = walk(20000, 1)
UNITS = units_of(BASE.astype(np.int16))
assert len(UNITS) >= 5
IA1, IB1, _ = UNITS[1]   # the second unit of BASE without exceptions
G1 = (IA1 & ~7) + ROUND  # where its second round starts


@pytest.mark.parametrize("m", METHODS)
def test_exception_counts_of_a_unit(oracle, m):
    """units with 0, 1, 2, 63, 64, 65 and about 200 exceptions: none, the list a wave holds, the searched slice"""
    rng = np.random.default_rng(2)
    sigs = []
    for k in (0, 1, 2, 63, 64, 65, 200):
        at = IA1 + 300 + rng.choice(1800, size=k, replace=False) if k else []
        sig = with_exceptions(BASE, at)
        assert units_of(sig)[1][2] == k and sum(u[2] for u in units_of(sig)) == k
        sigs.append(sig)
    check(oracle, m, shifted(sigs))


@pytest.mark.parametrize("m", METHODS)
def test_exceptions_at_round_and_unit_boundaries(oracle, m):
    """exceptions around the start of a unit's second round, around the unit's last sample and the next unit's first,
    at a read's sample 1 and its last sample; one at a time, then as runs of adjacent exceptions across the boundary
    (a run belongs to one unit - that of the value behind it - whose rounds it crosses) and as every other sample"""
    n = BASE.size
    sigs = []
    for b in (G1, IB1):
        for d in (-2, -1, 0, 1):
            sigs.append(with_exceptions(BASE, [b + d]))
        sigs.append(with_exceptions(BASE, range(b - 2, b + 2)))
        sigs.append(with_exceptions(BASE, range(b - 40, b + 41)))  # more than 64 in the unit, across the boundary
        sigs.append(with_exceptions(BASE, range(b - 20, b + 21)))  # at most 64
        sigs.append(with_exceptions(BASE, range(b - 40, b + 121, 2)))  # every other sample (each one moves the unit's end on by two)
    sigs.append(with_exceptions(BASE, [IA1, IA1 + 1]))
    sigs.append(with_exceptions(BASE, [1]))
    sigs.append(with_exceptions(BASE, [n - 1]))
    sigs.append(with_exceptions(BASE, [1, 2, G1 - 1, G1, IB1 - 1, IB1, n - 2, n - 1]))
    u = units_of(sigs[4])
    assert any(ia <= G1 - 2 and G1 + 1 < ib and e == 4 for ia, ib, e in u)  # (the run lies inside one unit)
    assert sorted(e for _, _, e in units_of(sigs[13]))[-2:] == [0, 81]  # (adjacent exceptions share a unit: that of the value behind them)
    u = units_of(sigs[15])
    assert u[1][2] > 0 and u[2][2] > 0 and u[1][2] + u[2][2] == 81  # (exceptions on both sides of a unit's end)
    check(oracle, m, shifted(sigs))


@pytest.mark.parametrize("m", METHODS)
def test_a_wave_switches_between_the_two_sample_loops(oracle, m):
    """a read whose first unit has more than 64 exceptions and whose second has none, the reverse, and both in turn:
    one-unit-at-a-time batches make one wave take the units one behind the other"""
    rng = np.random.default_rng(3)
    first = list(100 + rng.choice(2000, size=90, replace=False))
    second = list(IA1 + 300 + rng.choice(1800, size=90, replace=False))
    fourth = list(UNITS[3][0] + 300 + rng.choice(1800, size=70, replace=False))
    sigs = [with_exceptions(BASE, first), with_exceptions(BASE, second), with_exceptions(BASE, first + fourth),
            with_exceptions(BASE, first[:30] + second + fourth[:5])]
    assert [u[2] for u in units_of(sigs[0])[:2]] == [90, 0]
    assert [u[2] for u in units_of(sigs[1])[:3]] == [0, 90, 0]
    assert [u[2] for u in units_of(sigs[2])[:4]] == [90, 0, 0, 70]
    assert [u[2] for u in units_of(sigs[3])[:4]] == [30, 90, 0, 5]
    check(oracle, m, shifted(sigs))


# ---------------------------------------------------------------- tickets

LONG = walk(900000, 4, spread=10)
LONG_BITS = np.cumsum(LENS[zd_of(LONG.astype(np.int16))[1:]])


def read_of_units(k):
    """a prefix of LONG whose payload ends in its k-th unit"""
    want = (k - 1) * UNIT_BITS + UNIT_BITS // 2
    n = int(np.searchsorted(LONG_BITS, want)) + 2
    sig = LONG[:n].astype(np.int16)
    assert len(units_of(sig)) == k
    return sig


def one_unit_reads(k):
    return [LONG[1000 * j:1000 * j + 1500 + 7 * (j % 50)].astype(np.int16) for j in range(k)]


@pytest.mark.parametrize("k", [1, 15, 16, 17, 127, 128, 129, 257])
def test_unit_counts_around_a_chunk(oracle, k):
    """batches of k units - k around the 16 units a workgroup takes from the global counter at a time, and around
    eight workgroups' worth: as one long read, and as k reads of one unit each"""
    check(oracle, M, [read_of_units(k)], alone=k <= 17)
    sigs = one_unit_reads(k)
    assert all(len(units_of(s)) == 1 for s in sigs[:3])
    check(oracle, M, sigs, alone=False)


def test_fewer_units_than_a_workgroup_has_waves(oracle):
    for k in (1, 2, 3, 5, 7):
        check(oracle, M, one_unit_reads(k), alone=False)
    check(oracle, M, [read_of_units(3)])


def test_two_batches_back_to_back_on_one_stream(oracle):
    """two device-resident calls on one stream with nothing between them: the second call's workgroups start from
    its own cleared control block, whatever chunks the first call handed out"""
    import torch

    dev = torch.device("cuda:0")
    press.use_torch_stream()
    calls = []
    for sigs in ([read_of_units(129)] + one_unit_reads(40), one_unit_reads(17), [read_of_units(2)]):
        streams = [oracle_stream(oracle, M, s) for s in sigs]
        ns = np.array([s.size for s in sigs], dtype=np.int64)
        in_len = np.array([len(s) for s in streams], dtype=np.int64)
        in_off = np.concatenate([[0], np.cumsum(in_len)[:-1]])
        pad = (ns + 7) // 8 * 8
        off = np.concatenate([[0], np.cumsum(pad)[:-1]])
        comp = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
        calls.append(dict(sigs=sigs, off=off, comp=comp, in_off=torch.from_numpy(in_off).to(dev),
                          in_len=torch.from_numpy(in_len).to(dev), d_off=torch.from_numpy(off).to(dev),
                          d_n=torch.from_numpy(ns.astype(np.int32)).to(dev),
                          back=torch.zeros(int(pad.sum()) + 64, dtype=torch.int16, device=dev),
                          outn=torch.zeros(len(sigs), dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    for c in calls + calls[::-1]:  # (every order of a large and a small batch)
        c["back"].zero_()
        press.depress_batch(M, c["comp"], c["in_off"], c["in_len"], c["back"], c["d_off"], c["d_n"], c["outn"])
    torch.cuda.synchronize()
    for c in calls:
        back, outn = c["back"].cpu().numpy(), c["outn"].cpu().numpy()
        for s, o, k in zip(c["sigs"], c["off"], outn):
            assert k == s.size and np.array_equal(back[int(o):int(o) + s.size], s), s.size


# ---------------------------------------------------------------- steps

def long_deltas(lens):
    """one-byte deltas whose codes are the longest and the shortest of those above 12 bits"""
    syms = [s for s in range(256) if lens[s] >= 13]
    assert syms
    zs = (max(syms, key=lambda s: (lens[s], s)), min(syms, key=lambda s: (lens[s], s)))
    return [(z >> 1) ^ -(z & 1) for z in zs]


def with_deltas(a, at, delta):
    """sample at[j]'s delta replaced by `delta`"""
    a = a.copy()
    for i in sorted(at):
        a[i:] += delta - (a[i] - a[i - 1])
    return a.astype(np.int16)


def step_reads(lens, sub_bits):
    """reads for the decode loop: subsequences with every number of codes from none to full, +-1 walks (the shortest
    codes: as many codes as a subsequence takes), a long code at every place of a subsequence - so also as its
    first, its last and, where the read ends behind it, its only code - and two in a row"""
    span = sub_bits // int(lens[lens > 0].min()) + 2
    base = walk(4 * span + 700, 7, spread=3)
    sigs = [base[:n].astype(np.int16) for n in range(2, 2 * span + 2)]  # the last subsequence: 1, 2, 3, ... codes
    rng = np.random.default_rng(8)
    pm = np.cumsum(rng.choice([-1, 1], size=9000)).astype(np.int64) + 300
    sigs += [pm.astype(np.int16), pm[:span + 1].astype(np.int16), np.concatenate([base[:500], pm + base[499] - 300]).astype(np.int16)]
    for d in long_deltas(lens):
        for i in range(span + 4, 2 * span + 4):
            one = with_deltas(base[:i + 1 + span], [i], d)
            sigs += [one, one[:i + 1], with_deltas(base[:i + 2 + span], [i, i + 1], d)]
    return sigs


def subsequence_counts(sig, lens, sub_bits):
    z = zd_of(sig)[1:]
    start = np.concatenate([[0], np.cumsum(lens[z])])[:-1]
    return np.bincount(start // sub_bits)


def test_codes_of_a_subsequence(oracle):
    """0, 1, 2, odd and even numbers of codes in a subsequence, 64 codes, long codes first, last, alone and in pairs"""
    sigs = step_reads(LENS, SUB_BITS)
    counts = np.concatenate([subsequence_counts(s, LENS, SUB_BITS) for s in sigs])
    assert {1, 2, 3, 4, 31, 32, 64} <= set(counts.tolist())
    # (a long code as the first and as the only code of a subsequence)
    z = [zd_of(s)[1:] for s in sigs]
    first = [LENS[zz[np.unique((np.concatenate([[0], np.cumsum(LENS[zz])])[:-1]) // SUB_BITS, return_index=True)[1]]] for zz in z]
    assert any((f >= 13).any() for f in first)
    assert any(f[-1] >= 13 and subsequence_counts(s, LENS, SUB_BITS)[-1] == 1 for f, s in zip(first, sigs))
    for m in (M, "shuffman_vbsse21_zd"):
        check(oracle, m, sigs[::7] + sigs[-3:])
        check(oracle, m, sigs, alone=False)


@pytest.mark.parametrize("name", ["long_codes", "min1_incomplete", "min2_incomplete"])
def test_codes_of_a_subsequence_foreign_tables(oracle, tmp_path, name):
    """the same under the tables of test_gpu_parity.test_huffman_other_tables: 32- and 64-bit subsequences, and codes
    of up to 24 bits behind more long prefixes than second-level tables take (the decoder's trie walk)"""
    from test_gpu_parity import TABLES, _canonical_table, _write_table

    lens = np.array(TABLES[name], dtype=np.int64)
    path = str(tmp_path / (name + ".huffman"))
    _write_table(path, TABLES[name], _canonical_table(TABLES[name]))
    sub_bits = 256 if lens.min() >= 4 else 128 if lens.min() >= 2 else 64
    sigs = step_reads(lens, sub_bits) if (lens >= 13).any() else step_reads_short(lens, sub_bits)
    try:
        oracle.load_table(path)
        press.use_table(path)
        check(oracle, M, sigs[::7] + sigs[-3:])
        check(oracle, M, sigs, alone=False)
    finally:
        oracle.load_table()
        press.use_table()


def step_reads_short(lens, sub_bits):
    """step_reads for a table without long codes: every number of codes in the last subsequence, and long reads"""
    span = sub_bits // int(lens.min()) + 2
    base = walk(4 * span + 700, 9, spread=3)
    sigs = [base[:n].astype(np.int16) for n in range(2, 3 * span + 2)]
    flat = np.full(5000, 300, dtype=np.int64)  # delta 0 throughout: the shortest code, full subsequences
    return sigs + [flat.astype(np.int16), np.concatenate([base, flat + base[-1] - 300]).astype(np.int16)]
