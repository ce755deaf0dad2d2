"""CPU, no library: the host-buffer helpers every *_host form of press.py lays its arenas out with, exactly - offsets,
dtypes, zero fill and the 64 spare entries behind an arena.  Zero-length reads and the off-by-one at the pad of 8 samples
(7 and 9) are where they can go wrong."""
import numpy as np
import pytest

from honours_amd import press

BATCHES = [[], [[5]], [[1, 2, 3, 4, 5, 6, 7], [], [-1, -2, -3, -4, -5, -6, -7, -8, -9]]]
STREAMS = [b"abcde", b"", bytes(range(100, 117))]


def _same(a, want, dtype):
    assert isinstance(a, np.ndarray) and a.dtype == np.dtype(dtype), (a.dtype, dtype)
    assert a.tolist() == list(want), (a.tolist(), want)


@pytest.mark.parametrize("ns,off,total", [([], [], 0), ([1], [0], 8), ([7, 0, 9], [0, 8, 8], 24), ([8, 8], [0, 8], 16)])
def test_layout(ns, off, total):
    got_off, got_total = press._layout(ns)
    _same(got_off, off, np.uint64)
    assert got_total == total and isinstance(got_total, int)


@pytest.mark.parametrize("reads", BATCHES)
def test_host_batch(reads):
    reads = [np.array(r, dtype=np.int16) for r in reads]
    sig, off, ns, total = press._host_batch(reads)
    want_off, want_total = press._layout([len(r) for r in reads])
    _same(off, want_off, np.uint64)
    _same(ns, [len(r) for r in reads], np.uint32)
    assert total == want_total and all(int(o) % 8 == 0 for o in off)
    want = np.zeros(total + 64, dtype=np.int16)  # zero fill between the reads and behind the last one
    for r, o in zip(reads, off):
        want[int(o): int(o) + len(r)] = r
    _same(sig, want, np.int16)


def test_host_batch_takes_its_arena_from_alloc():
    asked = []

    def alloc(count, dtype):
        asked.append((count, dtype))
        return np.zeros(count, dtype=dtype)

    sig, off, ns, total = press._host_batch([np.arange(9, dtype=np.int16)], alloc)
    assert asked == [(16 + 64, np.int16)] and total == 16
    _same(sig[:16], list(range(9)) + [0] * 7, np.int16)


def test_streams_arena():
    comp, in_off, in_len = press._streams_arena(STREAMS)
    _same(in_len, [5, 0, 17], np.uint64)
    _same(in_off, [0, 5, 5], np.uint64)  # the empty stream in the middle starts where the next one does
    _same(comp, list(b"abcde" + bytes(range(100, 117)) + b"\0" * 64), np.uint8)
    assert comp.flags.writeable
    comp, in_off, in_len = press._streams_arena([])
    _same(in_len, [], np.uint64)
    _same(in_off, [], np.uint64)
    _same(comp, [0] * 64, np.uint8)


def test_slots():
    _same(press._slots([1, 16, 17]), [0, 16, 32, 64], np.uint64)
    _same(press._slots([]), [0], np.uint64)
    _same(press._slots(np.array([0, 15], dtype=np.uint32)), [0, 0, 16], np.uint64)


def test_streams_of():
    out = np.arange(64, dtype=np.uint8)
    out_off = np.array([0, 16, 32, 48], dtype=np.uint64)
    out_len = np.array([5, press.FAILED, 0], dtype=np.uint64)
    got = press._streams_of(out, out_off, out_len)
    assert got == [bytes(range(5)), None, b""] and all(s is None or type(s) is bytes for s in got)
    assert press._streams_of(out, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64)) == []


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_reads_of(dtype):
    buf = np.arange(24 + 64, dtype=dtype)
    off = np.array([0, 8, 8], dtype=np.uint64)
    out_n = np.array([7, 0xFFFFFFFF, 9], dtype=np.uint32)
    got = press._reads_of(buf, off, out_n)
    assert got[1] is None
    _same(got[0], range(7), dtype)
    _same(got[2], range(8, 17), dtype)
    buf[:] = 0  # copies, not views
    _same(got[0], range(7), dtype)
    assert got[0].base is None and got[2].base is None
    assert press._reads_of(buf, off[:0], out_n[:0]) == []


def test_cal_pairs():
    pairs = [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]
    _same(press._cal_pairs(pairs, 3, "cal"), [1, 2, 3, 4, 5, 6], np.float32)
    _same(press._cal_pairs(np.arange(6, dtype=np.float64), 3, "cal"), range(6), np.float32)
    _same(press._cal_pairs([], 0, "cal"), [], np.float32)
    assert press._cal_pairs(np.zeros((3, 2), dtype=np.float32)[:, ::-1], 3, "cal").flags.c_contiguous
    for bad, nreads in ((pairs, 2), (pairs, 4), ([1.0], 1), ([], 1)):
        with pytest.raises(press.PressError, match="per read"):
            press._cal_pairs(bad, nreads, "cal")
