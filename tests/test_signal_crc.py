"""CRC-32 of reads on the device (include/press_hip.h: press_hip_signal_crc32, press_hip_crc32_combine) and the checks of
the verify calls that need no device.

The digest is zlib's CRC-32 of a read's samples as bytes: the yardstick everywhere is zlib.crc32(samples.tobytes()), and
every comparison is one of integers.

CPU: press_hip_crc32_combine against zlib over small and random splits and - with no big buffer - over lengths up to 2^36
bytes (a truncated exponent shows there); the argument checks of the three device calls, which come before any device
call; press_hip_verify_workspace_bytes.  GPU: one batch of scattered reads whose counts sit on every edge of the kernel
(a lane's 16-byte group, a workgroup's step of 2048 samples, the tile of 32768, many tiles), with contents that catch a
forgotten initial-value term and a wrong tail exponent; repeatability; many short reads; the host form.
"""
import ctypes
import zlib

import numpy as np
import pytest

import _layouts as L
from honours_amd import build, press

gpu = pytest.mark.gpu
EARG = -2
GUARD = 0x5EEDC0DE


def crc_of(s):
    return zlib.crc32(np.ascontiguousarray(s, dtype=np.int16).tobytes()) & 0xFFFFFFFF


# ------------------------------------------------------------------ CPU

@pytest.fixture(scope="module")
def cpu_lib():
    build.build()
    return press.load_library()


def test_combine_against_zlib(cpu_lib):
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, size=20000, dtype=np.uint8).tobytes()
    lens = (0, 1, 3, 16, 4097)
    for la in lens:
        for lb in lens:
            a, b = data[:la], data[la:la + lb]
            assert press.crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)
    for _ in range(300):
        la, lb = int(rng.integers(0, 9000)), int(rng.integers(0, 9000))
        a, b = data[:la], data[la:la + lb]
        assert press.crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)
    # appending nothing changes nothing
    for la in (0, 1, 777):
        assert press.crc32_combine(zlib.crc32(data[:la]), zlib.crc32(b""), 0) == zlib.crc32(data[:la])
    # the raw symbol
    assert cpu_lib.press_hip_crc32_combine(zlib.crc32(b"hello "), zlib.crc32(b"world"), 5) == zlib.crc32(b"hello world")


def test_combine_large_lengths_without_a_buffer(cpu_lib):
    """z(L) = crc32 of L zero bytes: made directly up to 2^20, doubled by z(2L) = combine(z(L), z(L), L) up to 2^36 and
    checked against the direct value while a buffer is affordable; z(3L) by both groupings at every L - an exponent
    8 * len_b truncated to 32 bits breaks the second grouping from L = 2^28 on."""
    z = {}
    for k in range(0, 21):
        z[k] = zlib.crc32(bytes(1 << k))
    for k in range(0, 36):
        L_ = 1 << k
        z2 = press.crc32_combine(z[k], z[k], L_)
        if k + 1 in z:
            assert z2 == z[k + 1], k
        z[k + 1] = z2
        assert press.crc32_combine(z2, z[k], L_) == press.crc32_combine(z[k], z2, 2 * L_), k
    # ... and an odd split of 2^36 + 5 zero bytes, the long half in front or behind
    five = zlib.crc32(bytes(5))
    assert press.crc32_combine(z[36], five, 5) == press.crc32_combine(five, z[36], 1 << 36)
    # 2^32 - 1 zero bytes: 8 * len_b is a multiple of the group's order, so appending them multiplies by 1
    a = zlib.crc32(b"any prefix")
    assert press.crc32_combine(a, 0, 0xFFFFFFFF) == a


def test_argument_checks_need_no_device(cpu_lib):
    """a bad method id and a NULL argument are PRESS_HIP_EARG before any device call - also where there is no device -
    and the outputs stay as they were"""
    p = lambda x: x.ctypes.data
    arena = np.zeros(256, dtype=np.uint8)
    io = np.zeros(1, dtype=np.uint64)
    il = np.full(1, 16, dtype=np.uint64)
    sig = np.zeros(64, dtype=np.int16)
    n = np.full(1, 8, dtype=np.uint32)
    crc = np.full(1, 7, dtype=np.uint32)
    fb = np.full(1, 7, dtype=np.uint32)
    on = np.full(1, 7, dtype=np.uint32)
    nbad = np.full(1, 7, dtype=np.uint32)
    mid = press.METHODS["slow5_svb_zd"]
    dcrc = lambda mm, cc, oo: cpu_lib.press_hip_depress_crc_batch(mm, p(arena), p(io), p(il), 1, p(io), p(n), 64, cc, oo, 0)
    ver = lambda mm, ss, ff, bb: cpu_lib.press_hip_verify_batch(mm, p(arena), p(io), p(il), 1, ss, p(io), p(n), 64, ff, p(on), bb, 0)
    for bad in (-1, len(press.METHODS), 1000):
        assert dcrc(bad, p(crc), p(on)) == EARG and "not available" in press.last_error()
        assert ver(bad, p(sig), p(fb), p(nbad)) == EARG and "not available" in press.last_error()
    assert dcrc(mid, None, p(on)) == EARG and "NULL" in press.last_error()
    assert dcrc(mid, p(crc), None) == EARG and "NULL" in press.last_error()
    assert ver(mid, None, p(fb), p(nbad)) == EARG and "NULL" in press.last_error()
    assert ver(mid, p(sig), None, p(nbad)) == EARG and "NULL" in press.last_error()
    assert ver(mid, p(sig), p(fb), None) == EARG and "NULL" in press.last_error()
    assert cpu_lib.press_hip_signal_crc32(None, p(io), p(n), 1, 64, p(crc), 0) == EARG and "NULL" in press.last_error()
    assert cpu_lib.press_hip_signal_crc32(p(sig), p(io), p(n), 1, 64, None, 0) == EARG and "NULL" in press.last_error()
    # device resident: a sample arena that is not 16-byte aligned
    assert cpu_lib.press_hip_signal_crc32(p(sig) + 2, p(io), p(n), 1, 64, p(crc), 1) == EARG and "aligned" in press.last_error()
    assert [int(x[0]) for x in (crc, fb, on, nbad)] == [7, 7, 7, 7]


def test_outputs_untouched_by_refusals(cpu_lib):
    p = lambda x: x.ctypes.data
    arena = np.zeros(256, dtype=np.uint8)
    io = np.zeros(1, dtype=np.uint64)
    il = np.full(1, 16, dtype=np.uint64)
    sig = np.zeros(64, dtype=np.int16)
    n = np.full(1, 8, dtype=np.uint32)
    outs = [np.full(1, 7, dtype=np.uint32) for _ in range(4)]
    crc, fb, on, nbad = outs
    assert cpu_lib.press_hip_depress_crc_batch(99, p(arena), p(io), p(il), 1, p(io), p(n), 64, p(crc), p(on), 0) == EARG
    assert cpu_lib.press_hip_verify_batch(99, p(arena), p(io), p(il), 1, p(sig), p(io), p(n), 64, p(fb), p(on), p(nbad), 0) == EARG
    assert cpu_lib.press_hip_verify_batch(1, p(arena), p(io), p(il), 1, None, p(io), p(n), 64, p(fb), p(on), p(nbad), 0) == EARG
    assert cpu_lib.press_hip_depress_crc_batch(1, None, p(io), p(il), 1, p(io), p(n), 64, p(crc), p(on), 0) == EARG
    assert [int(x[0]) for x in outs] == [7, 7, 7, 7]


def test_verify_workspace_bytes(cpu_lib):
    t, nr = 1 << 20, 64
    for m, mid in press.METHODS.items():
        base = int(cpu_lib.press_hip_workspace_bytes(mid, t, nr))
        ws = int(cpu_lib.press_hip_verify_workspace_bytes(mid, t, nr))
        assert ws >= base, m
        assert ws - base >= 2 * t, (m, ws - base)
        assert ws - base < 2 * t + (1 << 16), (m, ws - base)  # the samples, the tile table, a word per read - no more
    for bad in (-1, len(press.METHODS), 1000):
        assert cpu_lib.press_hip_verify_workspace_bytes(bad, t, nr) == 0


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.use_torch_stream()
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


COUNTS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 4095, 4097, 32767, 32768, 32769, 65536 + 5, 300001, 3000000)

_batch = {}


def edge_batch():
    """the reads of the edge batch, their layout and zlib's digests: made once"""
    if not _batch:
        rng = np.random.default_rng(20261019)
        reads = [rng.integers(-32768, 32768, size=n).astype(np.int16) for n in COUNTS]
        for n in (9, 2049, 32769, 300001):
            reads += [np.zeros(n, dtype=np.int16), np.full(n, -1, dtype=np.int16), np.full(n, -32768, dtype=np.int16)]
        for n in (17, 4097, 65536 + 5, 300001):
            last = np.zeros(n, dtype=np.int16)
            last[-1] = 0x1234
            first = np.zeros(n, dtype=np.int16)
            first[0] = -77
            reads += [last, first]
        sig, off = L.scatter_reads(rng, reads)
        _batch.update(reads=reads, sig=sig, off=off, n=np.array([len(r) for r in reads], dtype=np.uint32),
                      want=np.array([crc_of(r) for r in reads], dtype=np.uint32))
    return _batch


def device_crc(lib, sig, off, n):
    """-> crc[nreads] of a device-resident call, its guard words checked"""
    import torch
    nreads = len(n)
    d_sig, d_off, d_n = _t(sig), _t(off, np.int64), _t(n, np.int32)
    d_crc = torch.full((nreads + 16,), GUARD, dtype=torch.int32, device="cuda")
    crc = d_crc[8:8 + nreads]
    press.signal_crc32(d_sig, d_off, d_n, crc)
    torch.cuda.synchronize()
    got = d_crc.cpu().numpy().view(np.uint32)
    assert (got[:8] == np.uint32(GUARD)).all() and (got[8 + nreads:] == np.uint32(GUARD)).all(), "written outside crc[]"
    return got[8:8 + nreads].copy()


@gpu
def test_edges_against_zlib(lib):
    b = edge_batch()
    got = device_crc(lib, b["sig"], b["off"], b["n"])
    bad = [(int(b["n"][k]), k, hex(int(got[k])), hex(int(b["want"][k]))) for k in np.nonzero(got != b["want"])[0]]
    assert not bad, bad[:10]
    assert int(got[0]) == 0  # the empty read
    # the same batch again: the same words
    assert np.array_equal(device_crc(lib, b["sig"], b["off"], b["n"]), got)


@gpu
def test_many_short_reads(lib):
    """300 reads of 1 .. 40 samples, and empty ones among them: many reads per workgroup of the finish kernel, waves
    with empty lanes, workgroups that take several tiles"""
    rng = np.random.default_rng(8)
    reads = [rng.integers(-32768, 32768, size=int(rng.integers(1, 41))).astype(np.int16) for _ in range(300)]
    for k in (0, 63, 64, 150, 299):
        reads[k] = reads[k][:0]
    sig, off = L.scatter_reads(rng, reads)
    n = np.array([len(r) for r in reads], dtype=np.uint32)
    got = device_crc(lib, sig, off, n)
    assert np.array_equal(got, np.array([crc_of(r) for r in reads], dtype=np.uint32))


@gpu
def test_host_form(lib):
    b = edge_batch()
    assert np.array_equal(press.signal_crc32_host(b["reads"]), b["want"])
    # the raw call on the scattered layout, pageable memory
    crc = np.full(len(b["n"]) + 2, GUARD, dtype=np.uint32)
    rc = lib.press_hip_signal_crc32(b["sig"].ctypes.data, b["off"].ctypes.data, b["n"].ctypes.data, len(b["n"]), b["sig"].size - 64,
                                    crc[1:].ctypes.data, 0)
    assert rc == 0, press.last_error()
    assert np.array_equal(crc[1:-1], b["want"]) and crc[0] == GUARD and crc[-1] == GUARD
    assert lib.press_hip_signal_crc32(None, None, None, 0, 0, None, 0) == 0  # an empty batch touches nothing


@gpu
def test_digests_combine(lib):
    """the digests of two reads that lie back to back make the digest of both: what the host helper is for"""
    b = edge_batch()
    k = [i for i, x in enumerate(COUNTS) if x == 32769][0]
    j = [i for i, x in enumerate(COUNTS) if x == 4097][0]
    both = np.concatenate([b["reads"][k], b["reads"][j]])
    assert press.crc32_combine(int(b["want"][k]), int(b["want"][j]), 2 * 4097) == crc_of(both)
