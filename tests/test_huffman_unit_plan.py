"""GPU: the per-unit plans of the static-Huffman decoder (k_huf_chain -> HufUnit -> k_huf_emit).

k_huf_chain decides for every unit (a quarter tile, one wave's work in k_huf_emit) which one-byte values it
delivers, which exceptions it merges in and the sample value in front of its first sample.  These reads sit on
the boundaries of those decisions; every one is decoded alone and in batches, and compared with the oracle."""
import numpy as np
import pytest

from honours_amd import press

pytestmark = pytest.mark.gpu

M = "shuffman_vbe21_zd"
UNIT_BYTES = 2048      # payload bytes of a unit for the NA12878 table (64 subsequences of 256 bits)
TILE_BYTES = 4 * UNIT_BYTES


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    press.load_library()
    press.load_table()
    yield


def walk(n, seed, spread=12):
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.integers(-spread, spread + 1, size=n)) + 500).astype(np.int64)


def with_exceptions(a, at):
    """exceptions (|delta| >= 128) at the given sample indices (>= 1), every other one up, every other one down"""
    a = a.copy()
    for j, i in enumerate(sorted(at)):
        a[i:] += 700 if j % 2 == 0 else -700
    return a.astype(np.int16)


def exceptions_of(stream):
    return int.from_bytes(stream[2:6], "little")


def payload_bytes(stream):
    return len(stream) - (2 + 4 + 6 * exceptions_of(stream) + 4)


def oracle_stream(oracle, sig):
    ret, st = oracle.press(M, sig)
    assert ret == 0
    return st


def check_alone(oracle, sig, stream=None, n=None):
    """one read through press.depress (and the oracle's stream back through the GPU)"""
    if stream is None:
        stream = oracle_stream(oracle, sig)
        ret, got = press.press(M, sig)
        assert ret == 0 and got == stream, press.last_error()
    n = sig.size if n is None else n
    ro, bo = oracle.depress(M, stream, n)
    rg, bg = press.depress(M, stream, n)
    assert (rg == 0) == (ro == 0), (rg, ro)
    if ro == 0:
        assert bg.size == bo.size and np.array_equal(bg, bo), (bg.size, bo.size)
    return stream


def check_batch(oracle, streams, ns):
    backs = press.depress_batch_host(M, streams, ns)
    for st, n, bk in zip(streams, ns, backs):
        ro, bo = oracle.depress(M, st, n)
        assert (bk is not None) == (ro == 0), (n, ro)
        if ro == 0:
            assert bk.size == bo.size and np.array_equal(bk, bo), (n, bk.size, bo.size)


def prefix_with_payload(oracle, base, target):
    """the shortest prefix of `base` whose Huffman payload is `target` bytes (no exceptions in base)"""
    lo, hi = 2, base.size
    while lo < hi:  # the payload grows with the prefix
        mid = (lo + hi) // 2
        if payload_bytes(oracle_stream(oracle, base[:mid].astype(np.int16))) < target:
            lo = mid + 1
        else:
            hi = mid
    sig = base[:lo].astype(np.int16)
    assert payload_bytes(oracle_stream(oracle, sig)) == target, target
    return sig


def test_exception_counts(oracle):
    """0, 1, 64, 65 and several hundred exceptions: the ballot-sized and the searched slices"""
    base = walk(40000, 1)
    rng = np.random.default_rng(2)
    sigs = []
    for k in (0, 1, 63, 64, 65, 129, 700):
        at = rng.choice(np.arange(1, base.size), size=k, replace=False) if k else []
        sig = with_exceptions(base, at)
        assert exceptions_of(oracle_stream(oracle, sig)) == k
        sigs.append(sig)
    streams = [check_alone(oracle, s) for s in sigs]
    check_batch(oracle, streams, [s.size for s in sigs])
    check_batch(oracle, streams[4:5], [sigs[4].size])  # a one-read batch


def test_every_key_in_a_range(oracle):
    """an exception at every other sample over several units: key pos[e] - e takes every value of the range, so
    some exception's key falls exactly on the first value of each unit there (and on the one behind its last)"""
    base = walk(60000, 3)
    sig = with_exceptions(base, range(3001, 3001 + 2 * 9000, 2))
    check_alone(oracle, sig)
    # and as runs of exceptions right in front of and behind those values
    sig2 = with_exceptions(base, [i for i in range(5000, 20000) if i % 7 in (0, 1, 2)])
    check_batch(oracle, [oracle_stream(oracle, sig), oracle_stream(oracle, sig2)], [sig.size, sig2.size])


def test_exceptions_at_the_ends(oracle):
    """exceptions in front of the first value and behind the last delivered one (the last delivering unit takes
    them all), alone and together"""
    base = walk(30000, 4)
    sigs = [with_exceptions(base, [1, 2, 3]), with_exceptions(base, [base.size - 3, base.size - 2, base.size - 1]),
            with_exceptions(base, list(range(1, 80)) + list(range(base.size - 80, base.size)))]
    streams = [check_alone(oracle, s) for s in sigs]
    check_batch(oracle, streams, [s.size for s in sigs])


def test_want_below_the_decoded_count(oracle):
    """a header that announces fewer one-byte values than the payload holds: the read delivers `want` values
    (huffman.c:1243); with its exceptions in front it stays on k_huf_emit's own sample writer"""
    base = walk(50000, 5)
    sig = with_exceptions(base, [10, 500, 9000])
    full = oracle_stream(oracle, sig)
    nex = exceptions_of(full)
    at = 2 + 4 + 6 * nex
    nlow = int.from_bytes(full[at:at + 4], "big")
    streams, ns = [], []
    for cut in (1, 7, 3000, 20000):
        st = full[:at] + (nlow - cut).to_bytes(4, "big") + full[at + 4:]
        check_alone(oracle, sig, stream=st, n=sig.size - cut)
        streams.append(st)
        ns.append(sig.size - cut)
    check_batch(oracle, streams + [full], ns + [sig.size])


def test_payload_sizes_at_unit_boundaries(oracle):
    """a payload of exactly one tile, of a whole number of units, and one that ends a few bits / bytes into a new
    unit (whose units then deliver a code or two, or nothing)"""
    base = walk(60000, 6)
    sigs = []
    for target in (TILE_BYTES, UNIT_BYTES, 3 * UNIT_BYTES, TILE_BYTES + 1, UNIT_BYTES + 1, 2 * UNIT_BYTES + 2,
                   TILE_BYTES + 36):
        sigs.append(prefix_with_payload(oracle, base, target))
    streams = [check_alone(oracle, s) for s in sigs]
    check_batch(oracle, streams, [s.size for s in sigs])
    # the same with exceptions early and late
    ex = [with_exceptions(s.astype(np.int64), [5, s.size - 2]) for s in sigs]
    check_batch(oracle, [check_alone(oracle, s) for s in ex], [s.size for s in ex])


def test_fused_and_unfused_reads_with_exceptions(oracle):
    """one batch: reads cut short inside the payload - some with all their exceptions in front of the cut (k_huf_emit
    writes them from fewer values than the header announces), some with exceptions behind it (their lists no longer
    interleave: the one-byte stream and k_low_decode_chunked) - between whole ones.  The reads the oracle decodes
    must come back as it decodes them; those it rejects only have to leave the others alone"""
    streams, ns = [], []
    for i in range(12):
        base = walk(20000 + 5000 * i, 10 + i)
        end = base.size // 2 if i % 4 == 1 else base.size
        sig = with_exceptions(base, list(range(100 * i + 1, end, 997)))
        st = oracle_stream(oracle, sig)
        if i % 2:
            st = st[:len(st) - len(st) // (3 + i)]
        streams.append(st)
        ns.append(sig.size)
    backs = press.depress_batch_host(M, streams, ns)
    decoded = 0
    for st, n, bk in zip(streams, ns, backs):
        ro, bo = oracle.depress(M, st, n)
        if ro == 0:
            assert bk is not None and bk.size == bo.size and np.array_equal(bk, bo), (n, bo.size)
            decoded += 1
    assert decoded >= 8
