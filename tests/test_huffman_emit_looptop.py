"""GPU: the head of k_huf_emit's unit loop - a wave draws the ticket of the unit after next and asks for its plan
while the stores of the unit before are still on their way, and reads that plan on every path, also where there is
no such unit.  What tests/test_huffman_emit_waits.py and tests/test_huffman_unit_plan.py do not have: batches of few
units, so that the last unit comes up in every position of a workgroup's chunk of 16 and most waves find no unit
behind theirs; the two copies of the sample writer on a batch's last units; a read that k_huf_emit does not write
itself; out_n of every read.  Every read is compared with the oracle."""
import numpy as np
import pytest

from honours_amd import press
from test_huffman_emit_waits import (BASE, IA1, M, one_unit_reads, oracle_stream, read_of_units, units_of,
                                     with_exceptions)

pytestmark = pytest.mark.gpu

UNIT_COUNTS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    press.load_library()
    press.load_table()
    yield


def check_batch(oracle, streams, rooms):
    """one batch call: every read comes back as the oracle decodes it - samples and count - or fails as it does"""
    backs = press.depress_batch_host(M, streams, rooms)
    ok = 0
    for i, (st, n, bk) in enumerate(zip(streams, rooms, backs)):
        ro, bo = oracle.depress(M, st, n)
        assert (bk is not None) == (ro == 0), (i, n, ro)
        if ro == 0:
            assert bk.size == bo.size, (i, bk.size, bo.size)  # (out_n)
            assert np.array_equal(bk, bo), (i, n, np.nonzero(bk != bo)[0][:4])
            ok += 1
    return ok


@pytest.mark.parametrize("k", UNIT_COUNTS)
def test_batches_of_few_units(oracle, k):
    """k units in all: as one read, as k reads of one unit, and as two reads that share them"""
    one = read_of_units(k)
    assert check_batch(oracle, [oracle_stream(oracle, M, one)], [one.size]) == 1
    sigs = one_unit_reads(k)
    assert all(len(units_of(s)) == 1 for s in sigs[:2] + sigs[-1:])
    assert check_batch(oracle, [oracle_stream(oracle, M, s) for s in sigs], [s.size for s in sigs]) == k
    if k >= 2:
        sigs = [read_of_units(k - k // 2), read_of_units(k // 2)]
        assert check_batch(oracle, [oracle_stream(oracle, M, s) for s in sigs], [s.size for s in sigs]) == 2


def last_unit_with(k, seed):
    """BASE cut behind its second unit, k exceptions in that (last) unit"""
    rng = np.random.default_rng(seed)
    at = IA1 + 300 + rng.choice(1800, size=k, replace=False) if k else []
    sig = with_exceptions(BASE, at)
    sig = sig[:units_of(sig)[1][1] - 40]
    u = units_of(sig)
    assert len(u) == 2 and u[1][2] == k and u[0][2] == 0, (k, u)
    return sig


@pytest.mark.parametrize("k", [0, 1, 64, 65])
def test_exceptions_in_the_last_unit(oracle, k):
    """0, 1, 64 and 65 exceptions in a batch's last unit (the sample writer that holds a unit's exceptions in the wave,
    and the one that searches them in memory): alone, behind one-unit reads, and in front of them"""
    sig = last_unit_with(k, 11 + k)
    st = oracle_stream(oracle, M, sig)
    assert int.from_bytes(st[2:6], "little") == k
    assert check_batch(oracle, [st], [sig.size]) == 1
    few = one_unit_reads(5)
    fs = [oracle_stream(oracle, M, s) for s in few]
    assert check_batch(oracle, fs + [st], [s.size for s in few] + [sig.size]) == 6
    assert check_batch(oracle, [st] + fs, [sig.size] + [s.size for s in few]) == 6


def test_a_read_that_is_not_fused(oracle):
    """streams cut short inside the payload between whole ones: with every exception in front of the cut the read
    delivers fewer samples than its header announces; with its last exception behind the values that are delivered
    the lists no longer interleave - k_huf_emit leaves the read to the one-byte path, which refuses it as the
    oracle does - and the reads around it are untouched"""
    early = with_exceptions(BASE, [100, 15000])
    late = with_exceptions(BASE, [100, BASE.size - 5])
    se, sl = oracle_stream(oracle, M, early), oracle_stream(oracle, M, late)
    whole = one_unit_reads(3)
    ws = [oracle_stream(oracle, M, s) for s in whole]
    streams = [ws[0], se[:len(se) - 2500], ws[1], sl[:len(sl) - 2500], ws[2], sl, sl[:len(sl) - 10]]
    rooms = [whole[0].size, early.size, whole[1].size, late.size, whole[2].size, late.size, late.size]
    verdicts = [oracle.depress(M, st, n) for st, n in zip(streams, rooms)]
    assert [r for r, _ in verdicts] == [0, 0, 0, -1, 0, 0, -1]
    assert verdicts[1][1].size < early.size  # (delivers less than announced)
    assert check_batch(oracle, streams, rooms) == 5
    assert check_batch(oracle, streams[3:4], rooms[3:4]) == 0  # (a batch of that read alone)


def test_two_depress_calls_back_to_back(oracle):
    """device-resident calls of 33, 3, 9 and 1 units on one stream with nothing between them, in both orders: out_n
    and the samples of every call"""
    import torch

    dev = torch.device("cuda:0")
    press.use_torch_stream()
    calls = []
    for sigs in ([read_of_units(17)] + one_unit_reads(16), one_unit_reads(3), [read_of_units(9)], one_unit_reads(1)):
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
    for order in (calls, calls[::-1]):
        for c in order:
            c["back"].zero_()
            c["outn"].fill_(-7)
        for c in order:
            press.depress_batch(M, c["comp"], c["in_off"], c["in_len"], c["back"], c["d_off"], c["d_n"], c["outn"])
        torch.cuda.synchronize()
        for c in order:
            back, outn = c["back"].cpu().numpy(), c["outn"].cpu().numpy()
            for s, o, k in zip(c["sigs"], c["off"], outn):
                assert int(k) == s.size, (int(k), s.size)
                assert np.array_equal(back[int(o):int(o) + s.size], s), s.size
