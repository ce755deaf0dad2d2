"""press_hip_blow5_next_pa: press_hip_blow5_next plus the calibration fields of every record (host code, no GPU).

The file is parsed a second time here, independently (zlib + struct on the layout of slow5.c:3903-3965), and the two
must agree on digitisation, offset and range."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest

from honours_amd import build, press

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLD, "three-reads.blow5")


@pytest.fixture(scope="module")
def cpu_lib():
    build.build()
    return press.load_library()


def parse_blow5(path):
    """-> [(read id, (digitisation, offset, range), signal field bytes)] of a BLOW5 file with zlib or no record compression"""
    b = open(path, "rb").read()
    assert b[:6] == b"BLOW5\x01"
    record_method = b[9]
    assert record_method in (0, 1)
    (hs,) = struct.unpack_from("<I", b, 64)
    p = 68 + hs
    out = []
    while b[p:p + 5] != b"5WOLB":
        (size,) = struct.unpack_from("<Q", b, p)
        rec = b[p + 8:p + 8 + size]
        p += 8 + size
        if record_method == 1:
            rec = zlib.decompress(rec)
        (idl,) = struct.unpack_from("<H", rec, 0)
        rid = rec[2:2 + idl].split(b"\0")[0].decode()
        q = 2 + idl + 4  # behind the read group
        dig, off, rng, _rate = struct.unpack_from("<4d", rec, q)
        (ln,) = struct.unpack_from("<Q", rec, q + 32)
        out.append((rid, (dig, off, rng), rec[q + 40:q + 40 + ln]))
    return out


def test_next_pa_matches_next_and_the_file(cpu_lib):
    want = parse_blow5(PATH)
    assert len(want) == 3
    rd = press.Blow5Reader(PATH)
    plain = rd.next_batch()
    rd.close()
    rd = press.Blow5Reader(PATH)
    assert rd.signal_method == 1  # (the signal field's length counts bytes: parse_blow5)
    got = rd.next_batch_pa()
    assert rd.next_batch_pa() == []
    rd.close()
    assert [(rid, n, s) for rid, n, s, _ in got] == plain
    for (rid, n, s, dor), (wid, wdor, ws) in zip(got, want):
        assert rid == wid and s == ws and n == struct.unpack_from("<I", ws, 0)[0]
        assert struct.pack("<3d", *dor) == struct.pack("<3d", *wdor), (rid, dor, wdor)
        assert dor[0] > 0 and dor[2] > 0
    assert len({d for _, _, _, d in got}) >= 1


def test_next_pa_cut_batches_continue(cpu_lib):
    """max_reads = 2: two reads, then the third with ITS calibration, then the end"""
    want = parse_blow5(PATH)
    rd = press.Blow5Reader(PATH)
    a = rd.next_batch_pa(max_reads=2)
    b = rd.next_batch_pa(max_reads=2)
    c = rd.next_batch_pa(max_reads=2)
    rd.close()
    assert len(a) == 2 and len(b) == 1 and c == []
    for (rid, n, s, dor), (wid, wdor, ws) in zip(a + b, want):
        assert rid == wid and s == ws and tuple(dor) == tuple(wdor)


def test_next_pa_null_dor_is_refused(cpu_lib):
    rd = press.Blow5Reader(PATH)
    arena = np.zeros(1 << 20, dtype=np.uint8)
    off = np.zeros(4, dtype=np.uint64)
    ln = np.zeros(4, dtype=np.uint64)
    ns = np.zeros(4, dtype=np.uint32)
    got = ctypes.c_uint32(9)
    cpu_lib.press_hip_blow5_next_pa.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    assert cpu_lib.press_hip_blow5_next_pa(rd._h, 4, arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data,
                                           ns.ctypes.data, None, None, ctypes.byref(got)) == -2
    # nothing was consumed: the whole file is still there
    assert len(rd.next_batch_pa()) == 3
    rd.close()
