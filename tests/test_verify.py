"""press_hip_verify_batch and press_hip_depress_crc_batch: compare-after-decode and the digest of what a stream decodes
to (include/press_hip.h).  Everything here is exact: integers against integers.

What a stream decodes to is the oracle's business (L.expect_depress); the digest of that is zlib.crc32, and first_bad is
the header's rule restated in numpy (first_bad_rule) over the oracle's decode.  Streams are the oracle's (L.expect_press)
and, for the zstd kinds, the library's own frames, as in the neighbouring tests.

A note on "not verified" in the battery: a read whose press is refused (the empty reads of the exception, Huffman, ex-zd
and range-coder methods) has no stream; the empty stream in its place is refused by the decoder and so counts as bad by
the rule (first_bad = 0).  For the 13 methods that are neither zstd kinds nor range coders the battery test therefore
asserts that every read that HAS a stream is VERIFIED and that nbad is exactly the number of reads without one (0 for
the four svb methods).  The two header-only Huffman streams per static-Huffman method are outside the decoder's domain
(L.header_only_huffman) and are only required to be consistent with nbad.
"""
import ctypes
import os
import zlib

import numpy as np
import pytest

import _forge
import _layouts as L
import _libs
from honours_amd import press

gpu = pytest.mark.gpu
METHODS = sorted(press.METHODS, key=lambda m: press.METHODS[m])
F32 = L.FAILED32
VERIFIED = 0xFFFFFFFF
GUARD = 0x5EEDC0DE
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOW5 = os.path.join(GOLD, "three-reads.blow5")
HOLD_MS = 50.0


def crc_of(s):
    return zlib.crc32(np.ascontiguousarray(s, dtype=np.int16).tobytes()) & 0xFFFFFFFF


def first_bad_rule(verdict, dec, s):
    """the header's rule: dec = what the stream decodes to in a room of len(s) samples, s = the caller's samples"""
    if verdict == "fail":
        return 0
    c, n = len(dec), len(s)
    lim = min(c, n)
    d = np.nonzero(np.asarray(dec[:lim]) != np.asarray(s[:lim]))[0]
    if d.size:
        return int(d[0])
    return lim if c != n else VERIFIED


def test_rule_restated():
    s = np.arange(10, dtype=np.int16)
    assert first_bad_rule("fail", None, s) == 0
    assert first_bad_rule("ok", s, s) == VERIFIED
    assert first_bad_rule("ok", s[:7], s) == 7
    t = s.copy()
    t[3] = t[8] = -1
    assert first_bad_rule("ok", t, s) == 3
    assert first_bad_rule("ok", t[:2], s) == 2
    assert press.VERIFIED == VERIFIED


# ------------------------------------------------------------------ GPU plumbing

@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.load_table()
    press.use_torch_stream()
    lb.press_hip_host_alloc.restype = ctypes.c_void_p
    lb.press_hip_host_alloc.argtypes = [ctypes.c_uint64]
    lb.press_hip_host_free.argtypes = [ctypes.c_void_p]
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


class Slots:
    """per-read 32-bit outputs of a device-resident call, each behind and in front of guard words"""

    def __init__(self, nreads, names):
        import torch
        self.nreads, self.names = nreads, names
        self.t = {k: torch.full((nreads + 16,), GUARD, dtype=torch.int32, device="cuda") for k in names}

    def __getitem__(self, k):
        return self.t[k][8:8 + (1 if k == "nbad" else self.nreads)]

    def fetch(self):
        out = {}
        for k in self.names:
            a = self.t[k].cpu().numpy().view(np.uint32)
            w = 1 if k == "nbad" else self.nreads
            assert (a[:8] == np.uint32(GUARD)).all() and (a[8 + w:] == np.uint32(GUARD)).all(), (k, "written outside its slot")
            out[k] = a[8:8 + w].copy()
        return out


def streams_of(oracle, m, reads):
    """the oracle's streams (b"" where it refuses the read); the zstd kinds: the library's own frames"""
    if m in L.ZSTD_KINDS:
        st, _ = press.press_packed_host(m, reads)
    else:
        st = [L.expect_press(oracle, m, s, L.slot_of(oracle.bound, m, len(s))) for s in reads]
    return [b"" if x is None else x for x in st]


def dev_verify(m, inb, in_off, in_len, sig, off, n):
    """one device-resident press_hip_verify_batch -> {first_bad, out_n, nbad}; sig must come back bit for bit"""
    import torch
    sl = Slots(len(n), ("first_bad", "out_n", "nbad"))
    d_sig = _t(sig)
    press.verify_batch(m, _t(inb), _t(in_off, np.int64), _t(in_len, np.int64), d_sig, _t(off, np.int64), _t(n, np.int32),
                       sl["first_bad"], sl["out_n"], sl["nbad"])
    torch.cuda.synchronize()
    assert np.array_equal(d_sig.cpu().numpy(), sig), (m, "the caller's samples were written")
    return sl.fetch()


def dev_crc(m, inb, in_off, in_len, off, rooms, total):
    import torch
    sl = Slots(len(rooms), ("crc", "out_n"))
    press.depress_crc_batch(m, _t(inb), _t(in_off, np.int64), _t(in_len, np.int64), _t(off, np.int64), _t(rooms, np.int32), total,
                            sl["crc"], sl["out_n"])
    torch.cuda.synchronize()
    return sl.fetch()


# ------------------------------------------------------------------ 1: the battery, all 19 methods

_bat = {}


def battery_case(oracle, m):
    if m not in _bat:
        reads = [s for _, s in L.battery()]
        rng = np.random.default_rng(9100 + press.METHODS[m])
        st = streams_of(oracle, m, reads)
        c = {"reads": reads, "streams": st}
        c["inb"], c["in_off"], c["in_len"] = L.scatter_streams(rng, st)
        # the digest call: rooms with some slack where the stream carries its count
        extra = 0 if m in L.SVB_KINDS else 21
        c["rooms"] = np.array([len(s) + (int(rng.integers(0, extra)) if extra else 0) for s in reads], dtype=np.uint32)
        c["room_off"], c["room_total"] = L.scatter_rooms(rng, c["rooms"])
        c["dec_room"] = [L.expect_depress(oracle, m, s, x, int(r)) for s, x, r in zip(reads, st, c["rooms"])]
        # the verify call: n is the expected count and the room; the caller's samples are scattered among noise
        c["n"] = np.array([len(s) for s in reads], dtype=np.uint32)
        c["sig"], c["off"] = L.scatter_reads(rng, reads)
        c["dec_n"] = [L.expect_depress(oracle, m, s, x, len(s)) for s, x in zip(reads, st)]
        _bat[m] = c
    return _bat[m]


def check_crc(m, c, got):
    for k, (verdict, want) in enumerate(c["dec_room"]):
        tag = (m, k, int(c["rooms"][k]))
        if verdict == "skip":
            continue
        if verdict == "fail":
            assert int(got["out_n"][k]) == F32 and int(got["crc"][k]) == 0, tag
            continue
        assert int(got["out_n"][k]) == len(want), tag
        assert int(got["crc"][k]) == crc_of(want), tag + (hex(int(got["crc"][k])), hex(crc_of(want)))


def check_verify(m, c, got):
    fb = got["first_bad"]
    assert int(got["nbad"][0]) == int((fb != VERIFIED).sum()), (m, int(got["nbad"][0]))
    for k, (verdict, want) in enumerate(c["dec_n"]):
        if verdict == "skip":
            continue
        tag = (m, k, int(c["n"][k]))
        assert int(got["out_n"][k]) == (F32 if verdict == "fail" else len(want)), tag
        assert int(fb[k]) == first_bad_rule(verdict, want, c["reads"][k]), tag + (int(fb[k]),)


@gpu
@pytest.mark.parametrize("m", METHODS)
def test_battery(lib, oracle, m):
    c = battery_case(oracle, m)
    check_crc(m, c, dev_crc(m, c["inb"], c["in_off"], c["in_len"], c["room_off"], c["rooms"], c["room_total"]))
    got = dev_verify(m, c["inb"], c["in_off"], c["in_len"], c["sig"], c["off"], c["n"])
    check_verify(m, c, got)
    fb = got["first_bad"]
    has_stream = [k for k, x in enumerate(c["streams"]) if x and c["dec_n"][k][0] != "skip"]
    if m in _libs.RC_FAMILY:
        # the case the call exists for: a valid output of press that does not round-trip
        raw = [k for k in has_stream if _libs.rc_stored_raw(m, c["streams"][k], len(c["reads"][k]))]
        assert raw, m
        assert any(int(fb[k]) != VERIFIED for k in raw), (m, raw, [int(fb[k]) for k in raw])
    elif m not in L.ZSTD_KINDS:
        assert all(int(fb[k]) == VERIFIED for k in has_stream), (m, [(k, int(fb[k])) for k in has_stream if int(fb[k]) != VERIFIED])
        rest = [k for k in range(len(fb)) if k not in has_stream]  # reads without a stream, header-only Huffman streams
        assert int(got["nbad"][0]) == sum(int(fb[k]) != VERIFIED for k in rest), m
        if m in L.SVB_KINDS:
            assert int(got["nbad"][0]) == 0, m


# ------------------------------------------------------------------ 2: the comparison itself

def _changes(n):
    """(indices to change in the caller's samples, first_bad expected) for a read of n samples"""
    singles = [0, 7, 8, 2047, 2048, 32767, 32768, n - 1]
    return [([i], i) for i in singles] + [([n - 2, 2049], 2049), ([], VERIFIED)]


@gpu
@pytest.mark.parametrize("m", ["svb12_zd", "shuffman_vbe21_zd"])
def test_first_difference(lib, oracle, m):
    """the caller's samples - not the stream - change at one index (or two: the smaller wins); the neighbours stay
    VERIFIED; a change at n .. roundup8(n) - 1, beyond the read and inside its last group, is not reported"""
    rng = np.random.default_rng(31)
    base = [L._walk(rng, 40000, 0.01), L._walk(rng, 70001, 0.01)]
    st = streams_of(oracle, m, base)
    reads, streams, want = [], [], []
    for s, x in zip(base, st):
        for idx, fb in _changes(len(s)):
            t = s.copy()
            for i in idx:
                t[i] ^= 0x0100
            reads += [t, s]  # ... and an untouched neighbour
            streams += [x, x]
            want += [fb, VERIFIED]
    inb, in_off, in_len = L.scatter_streams(rng, streams)
    sig, off = L.scatter_reads(rng, reads)
    n = np.array([len(r) for r in reads], dtype=np.uint32)
    for k, r in enumerate(reads):  # the samples behind a read, inside its last group: different from anything decoded
        o, e = int(off[k]) + len(r), int(off[k]) + L.roundup8(len(r))
        sig[o:e] = 0x7A5A
    got = dev_verify(m, inb, in_off, in_len, sig, off, n)
    assert np.array_equal(got["out_n"], n), m
    assert [int(x) for x in got["first_bad"]] == want, m
    assert int(got["nbad"][0]) == sum(w != VERIFIED for w in want)


# ------------------------------------------------------------------ 3: counts that differ, refused streams

@gpu
def test_count_mismatch_and_forged(lib, oracle):
    m = "vbe21_zd"
    rng = np.random.default_rng(32)
    s100 = L._walk(rng, 100, 0.05)
    st100 = streams_of(oracle, m, [s100])[0]
    longer = np.concatenate([s100, L._walk(rng, 20)])
    good = _forge.good_reads(oracle, m)
    good_s = [oracle.depress(m, x, room)[1] for _, x, room in good]
    forged = [c for c in _forge.cases_for(m, oracle) if c.verdict == _forge.REFUSED and c.stream][0]
    reads = [longer, s100[:80], good_s[0], rng.integers(-99, 99, size=forged.room).astype(np.int16), good_s[1]]
    streams = [st100, st100, good[0][1], forged.stream, good[1][1]]
    inb, in_off, in_len = L.scatter_streams(rng, streams)
    sig, off = L.scatter_reads(rng, reads)
    n = np.array([len(r) for r in reads], dtype=np.uint32)
    got = dev_verify(m, inb, in_off, in_len, sig, off, n)
    assert [int(x) for x in got["out_n"]] == [100, F32, len(good_s[0]), F32, len(good_s[1])]
    assert [int(x) for x in got["first_bad"]] == [100, 0, VERIFIED, 0, VERIFIED]
    assert int(got["nbad"][0]) == 3


# ------------------------------------------------------------------ 4: host forms

def _pinned(lib, a, held):
    p = lib.press_hip_host_alloc(max(a.nbytes, 64))
    assert p
    held.append(p)
    b = np.frombuffer((ctypes.c_uint8 * a.nbytes).from_address(p), dtype=a.dtype)
    b[:] = a
    return b


@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "shuffman_vbe21_zd", "rc_vbe21_zd"])
def test_host_forms(lib, oracle, m):
    c = battery_case(oracle, m)
    # the helpers of press.py (pageable, packed layouts)
    fb, out_n, nbad = press.verify_batch_host(m, c["streams"], c["reads"])
    check_verify(m, c, {"first_bad": fb, "out_n": out_n, "nbad": np.array([nbad])})
    crc, out_n = press.depress_crc_batch_host(m, c["streams"], [len(s) for s in c["reads"]])
    rooms0 = dict(c, rooms=c["n"], dec_room=c["dec_n"])
    check_crc(m, rooms0, {"crc": crc, "out_n": out_n})
    # the raw calls on the scattered layouts, pageable and page-locked
    mid = press.METHODS[m]
    nr = len(c["n"])
    for pinned in (False, True):
        held = []
        w = (lambda a: _pinned(lib, a, held)) if pinned else (lambda a: a.copy())
        inb, sig = w(c["inb"]), w(c["sig"])
        p = lambda x: x.ctypes.data
        fb, on, crc, on2 = (np.full(nr + 2, GUARD, dtype=np.uint32) for _ in range(4))
        nbad = np.full(3, GUARD, dtype=np.uint32)
        try:
            assert lib.press_hip_verify_batch(mid, p(inb), p(c["in_off"]), p(c["in_len"]), nr, p(sig), p(c["off"]), p(c["n"]), sig.size - 64,
                                              p(fb[1:]), p(on[1:]), p(nbad[1:]), 0) == 0, press.last_error()
            assert lib.press_hip_depress_crc_batch(mid, p(inb), p(c["in_off"]), p(c["in_len"]), nr, p(c["room_off"]), p(c["rooms"]),
                                                   c["room_total"], p(crc[1:]), p(on2[1:]), 0) == 0, press.last_error()
            assert np.array_equal(sig, c["sig"])
        finally:
            for h in held:
                lib.press_hip_host_free(h)
        for a in (fb, on, crc, on2, nbad):
            assert a[0] == GUARD and a[-1] == GUARD
        check_verify(m, c, {"first_bad": fb[1:-1], "out_n": on[1:-1], "nbad": nbad[1:2]})
        check_crc(m, c, {"crc": crc[1:-1], "out_n": on2[1:-1]})
    one = np.full(1, 7, dtype=np.uint32)
    assert lib.press_hip_verify_batch(mid, None, None, None, 0, None, None, None, 0, None, None, one.ctypes.data, 0) == 0 and one[0] == 0


# ------------------------------------------------------------------ 5: the device-resident calls only enqueue

@gpu
@pytest.mark.parametrize("m", ["slow5_svb_zd", "shuffman_vbe21_zd", "rc_vbe21_zd"])
def test_only_enqueues_behind_a_hold(lib, oracle, m):
    """on a torch side stream that is held for 50 ms (tests/test_depress_chunks.py's device): each of the three
    device-resident calls returns with the hold still pending, and the results are exact afterwards.  (The zstd kinds
    wait for the host, as documented, and are not asked.)"""
    import torch
    torch.cuda._sleep(100000)
    torch.cuda.synchronize()
    cycles = 2000000
    for _ in range(3):  # torch.cuda._sleep's unit, measured with two events
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 5.0:
            break
        cycles *= 10
    assert ms >= 5.0
    c = battery_case(oracle, m)
    nr = len(c["n"])
    d_in, d_io, d_il = _t(c["inb"]), _t(c["in_off"], np.int64), _t(c["in_len"], np.int64)
    d_sig, d_off, d_n = _t(c["sig"]), _t(c["off"], np.int64), _t(c["n"], np.int32)
    d_roff, d_rooms = _t(c["room_off"], np.int64), _t(c["rooms"], np.int32)

    def calls():
        v, d, g = Slots(nr, ("first_bad", "out_n", "nbad")), Slots(nr, ("crc", "out_n")), Slots(nr, ("crc",))
        press.verify_batch(m, d_in, d_io, d_il, d_sig, d_off, d_n, v["first_bad"], v["out_n"], v["nbad"])
        press.depress_crc_batch(m, d_in, d_io, d_il, d_roff, d_rooms, c["room_total"], d["crc"], d["out_n"])
        press.signal_crc32(d_sig, d_off, d_n, g["crc"])
        return v, d, g

    calls()  # (scratch is reserved, the table is on the device: what follows allocates nothing)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert lib.press_hip_set_stream(ctypes.c_void_p(s.cuda_stream)) == 0
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(HOLD_MS * cycles / ms))
            e = torch.cuda.Event()
            e.record(s)
            v, d, g = calls()
            assert not e.query(), "a call that promises only to enqueue waited for the stream (or the delay of %g ms ended early)" % HOLD_MS
        s.synchronize()
        assert e.query()
    finally:
        press.use_torch_stream()
    check_verify(m, c, v.fetch())
    check_crc(m, c, d.fetch())
    assert np.array_equal(g.fetch()["crc"], np.array([crc_of(r) for r in c["reads"]], dtype=np.uint32))


# ------------------------------------------------------------------ 6: BLOW5

def _golden_reads():
    import json
    meta = json.load(open(os.path.join(GOLD, "three_reads.json")))
    sig = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    out, o = {}, 0
    for r in meta["reads"]:
        out[r["read_id"]] = sig[o:o + r["n"]]
        o += r["n"]
    return out


@gpu
def test_blow5_transcode_verifies(lib, tmp_path):
    plain, checked, broken = (str(tmp_path / x) for x in ("plain.blow5", "checked.blow5", "broken.blow5"))
    assert press.blow5_transcode(BLOW5, plain) == 3
    assert press.blow5_transcode(BLOW5, checked, verify=True) == 3
    assert open(plain, "rb").read() == open(checked, "rb").read()
    rd = press.Blow5Reader(BLOW5)
    ids = [rid for rid, _, _ in rd.next_batch()]
    rd.close()

    def flipping(reads):
        out = press.press_batch_host("slow5_svb_zd", reads)
        st = bytearray(out[1])
        st[len(st) // 2] ^= 0x04  # a data byte of the second read's stream
        out[1] = bytes(st)
        return out

    with pytest.raises(press.PressError) as ei:
        press.blow5_transcode(BLOW5, broken, codec=flipping, verify=True)
    assert ids[1] in str(ei.value) and ids[0] not in str(ei.value) and ids[2] not in str(ei.value)
    rd = press.Blow5Reader(broken)  # the writer was finished: a valid file, and no record in it
    assert rd.next_batch() == []
    rd.close()
    # without verify the same codec writes the broken field
    assert press.blow5_transcode(BLOW5, broken, codec=flipping) == 3


@gpu
def test_blow5_stored_fields_digest(lib):
    """the digest of what the file's stored fields decode to, without a sample leaving the device"""
    gold = _golden_reads()
    rd = press.Blow5Reader(BLOW5)
    batch = rd.next_batch()
    rd.close()
    crc, out_n = press.depress_crc_batch_host("slow5_svb_zd", [f for _, _, f in batch], [n for _, n, _ in batch])
    assert [int(x) for x in out_n] == [n for _, n, _ in batch]
    assert [int(x) for x in crc] == [crc_of(gold[rid]) for rid, _, _ in batch]
    back = press.depress_batch_host("slow5_svb_zd", [f for _, _, f in batch], [n for _, n, _ in batch])  # test_blow5.py's route
    assert [int(x) for x in crc] == [crc_of(b) for b in back]
