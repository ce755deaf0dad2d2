"""BLOW5 records deflated on the device (include/press_hip.h section 2z): zlib streams that slow5lib reads.

The yardstick is the serial model tests/_deflate.py.  The CPU tests hold the model itself against zlib - every stream
inflates to its record, the token rules at their edges, the code-length limit, the stored fallback, and the size against
zlib's own deflate on real records.  The GPU tests hold the device against the model, byte for byte: the image, rec_off,
raw and the sizes call, in the host-pointer and the device-resident form, behind two scratch fills, and on a held stream.
The file-level tests read what blow5_transcode(deflate="device") wrote.

The battery is made once per session and never changed; U = 1024 is the device's unit (a wave's bytes of a record)."""
import functools
import json
import os
import struct
import zlib

import numpy as np
import pytest

import _deflate as D
import _libs
from honours_amd import deflate, press, synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOW5 = os.path.join(GOLD, "three-reads.blow5")
U = 1024
RUNS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 1 + 2 * 258 + 2)
NZ = bytes(range(1, 256))


def nz(n, seed=0):
    """n bytes, none of them zero"""
    return bytes(NZ[(seed + 7 * i) % 255] for i in range(n))


def fib_bytes():
    """byte counts 1, 1, 2, 3, 5, ...: unlimited Huffman lengths pass 15"""
    a, b, out, v = 1, 1, bytearray(), 1
    while len(out) + a < 6000:
        out += bytes([v]) * a
        a, b, v = b, a + b, v + 1
    return bytes(out)


def run_at(start, length, pre_len=41, tail=5):
    """(pre, sig, post) of a record whose zero run of `length` bytes begins at byte `start` of the record"""
    assert start >= pre_len + 8 + 1
    return nz(pre_len, 3), nz(start - pre_len - 8, 5) + bytes(length) + nz(tail, 9), nz(13, 11)


@functools.lru_cache(maxsize=None)
def battery():
    """-> [(name, pre, sig, post)] for signal method 1: every case of the issue that is a framed record"""
    rng = np.random.default_rng(20)
    out = []
    for L in RUNS:
        out.append(("run %d" % L, b"\x05\x00id-%03d" % L, b"\x05" + bytes(L) + b"\x06", b"\x09" * (L % 3)))
    out.append(("run at the start", bytes(300), b"\x05\x06\x07", b"\x01"))
    out.append(("run at the end", nz(17), nz(40), bytes(300)))
    out.append(("all zero", bytes(10), b"", bytes(700)))
    out.append(("one value", b"\x07" * 5, b"\x07" * 7, b""))
    out.append(("all values", nz(9), bytes(range(256)) * 3, b""))
    out.append(("fibonacci", nz(20), fib_bytes(), nz(3)))
    out.append(("random 3000", nz(30), rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), b""))
    out.append(("random 70000", nz(31), rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), nz(2)))
    for L in (U - 1, U, U + 1, 2 * U + 259):
        ends = (L + U + U - 1) // U * U  # the first unit boundary the run can end at
        for start in (U - 1, U, U + 1, ends - L, 2 * U - L // 2):
            if start >= 50:
                out.append(("run %d from %d" % (L, start),) + run_at(start, L))
    out.append(("two-byte tail in the next unit",) + run_at(U - 259, 261))
    out.append(("tail split by the unit's end",) + run_at(U - 260, 261))
    for n in (70, 333, U - 8, U, U + 9, 2 * U + 1, 3 * U):  # a mix of sizes, odd offsets in both arenas
        pre = nz(45 + n % 2, n)
        body = bytearray(rng.integers(0, 8, n - len(pre) - 8, dtype=np.uint8))
        out.append(("mixed %d" % n, pre, bytes(body), b""))
    big = np.zeros(1200000, dtype=np.uint8)
    at = rng.integers(0, big.size, 24000)
    big[at] = rng.integers(1, 256, at.size)
    big[300000:700000] = 0  # hundreds of units inside one run
    out.append(("1.2 MB", nz(61), big.tobytes(), nz(40)))
    return out


@functools.lru_cache(maxsize=None)
def battery_model():
    """-> (records, image, rec_off, raw) of the battery by the model"""
    recs = [D.frame(p, s, q, 1) for _, p, s, q in battery()]
    return (recs,) + D.image(recs)


@functools.lru_cache(maxsize=None)
def real_records():
    """the three real reads and six synthetic ones as svb-zd records with a 60-byte front part -> [bytes]"""
    o = _libs.oracle()
    meta = json.load(open(os.path.join(GOLD, "three_reads.json")))
    sig = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    reads, at = [], 0
    for r in meta["reads"]:
        reads.append(sig[at:at + r["n"]])
        at += r["n"]
    s, off = synth.synth_batch(1, 0, 6)
    reads += [s[int(off[k]):int(off[k + 1])] for k in range(6)]
    out = []
    for k, r in enumerate(reads):
        ret, field = o.press("slow5_svb_zd", r)
        assert ret == 0
        out.append(D.frame(b"\x24\x00" + b"%036d" % k + nz(22, k), field, b"", 1))
    return out


# ------------------------------------------------------------------ CPU: the model against zlib

def test_every_fixture_record_inflates():
    recs, image, rec_off, raw = battery_model()
    assert rec_off[0] == 0 and len(image) == rec_off[-1]
    for k, rec in enumerate(recs):
        ln, = struct.unpack("<Q", image[rec_off[k]:rec_off[k] + 8])
        assert ln == rec_off[k + 1] - rec_off[k] - 8
        stream = image[rec_off[k] + 8:rec_off[k + 1]]
        assert stream[:2] == b"\x78\x01" and zlib.decompress(stream) == rec, battery()[k][0]  # (zlib checks the Adler-32)


@pytest.mark.parametrize("L", RUNS)
def test_tokeniser_edges(L):
    """a run of L zeros: the literal, matches of min(rest, 258) while rest >= 3, then 0 .. 2 literals"""
    rec = b"\x05" + bytes(L) + b"\x06"
    toks = D.tokens(rec)
    assert toks[0] == ("lit", 5) and toks[1] == ("lit", 0) and toks[-1] == ("lit", 6)
    body = toks[2:-1]
    matches = [v for k, v in body if k == "match"]
    tail = [t for t in body if t[0] == "lit"]
    assert all(3 <= v <= 258 for v in matches) and all(v == 258 for v in matches[:-1])
    assert body == [("match", v) for v in matches] + tail and tail == [("lit", 0)] * len(tail) and len(tail) <= 2
    assert 1 + sum(matches) + len(tail) == L and (not tail or (L - 1) % 258 == len(tail) or L - 1 == len(tail))
    stream, raw = D.deflate_record(rec)
    assert zlib.decompress(stream) == rec


def test_run_placement():
    for rec in (bytes(300) + b"\x01\x02", b"\x01\x02" + bytes(300), bytes(1), bytes(2), bytes(3), bytes(259), bytes(5000)):
        stream, raw = D.deflate_record(rec)
        assert zlib.decompress(stream) == rec
        assert sum(1 if k == "lit" else v for k, v in D.tokens(rec)) == len(rec)


def test_symbol_counts():
    info = {}
    rec = b"\x07" * 100
    stream, raw = D.deflate_record(rec, info)
    assert zlib.decompress(stream) == rec
    assert [s for s in range(D.NLIT) if info["lens"][s]] == [7, 256] and info["maxlen"] == 1
    rec = bytes(range(256)) * 4
    stream, raw = D.deflate_record(rec, info)
    assert zlib.decompress(stream) == rec and all(info["lens"][s] for s in range(257)) and info["nlit"] == 257


def test_code_length_limit():
    rec = fib_bytes()
    assert 2000 < len(rec) < 8192
    hist = D.histogram(rec)
    assert max(D._build(hist)) > 15  # without the limit
    info = {}
    stream, raw = D.deflate_record(rec, info)
    assert info["k"] >= 1 and info["maxlen"] <= 15 and raw == 0
    assert zlib.decompress(stream) == rec


def test_stored_fallback():
    rng = np.random.default_rng(3)
    for n, blocks in ((3000, 1), (70000, 2), (65535, 1), (65536, 2)):
        rec = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        stream, raw = D.deflate_record(rec)
        assert raw == 1 and len(stream) == 2 + n + 5 * blocks + 4
        assert zlib.decompress(stream) == rec


def test_signal_method_0():
    s = (np.cumsum(np.random.default_rng(4).integers(-20, 21, 5000)) + 400).astype(np.int16)
    rec = D.frame(nz(50), s.tobytes(), nz(4), 0)
    assert struct.unpack("<Q", rec[50:58])[0] == s.size
    stream, raw = D.deflate_record(rec)
    assert zlib.decompress(stream) == rec


def test_size_against_zlib():
    """the condition of the issue: on the three real reads and six synthetic ones, framed as svb-zd records, the model's
    stream is no longer than zlib's at its default level (the estimate: 0.94 to 0.954 of it)"""
    for k, rec in enumerate(real_records()):
        stream, raw = D.deflate_record(rec)
        z = zlib.compress(rec, -1)
        print("record %d: %d bytes, model %d, zlib %d, ratio %.4f" % (k, len(rec), len(stream), len(z), len(stream) / len(z)))
        assert zlib.decompress(stream) == rec and raw == 0
        assert len(stream) <= len(z), (k, len(stream), len(z))


def test_entry_points_exist():
    lib = press.load_library()
    for name in ("press_hip_blow5_deflate_sizes", "press_hip_blow5_deflate_batch", "press_hip_blow5_deflate_workspace_bytes",
                 "press_hip_blow5_write_image"):
        assert hasattr(lib, name)
    from honours_amd import build
    assert "press_deflate.hip" in build.SOURCES
    w1, w2 = (int(lib.press_hip_blow5_deflate_workspace_bytes(b, n)) for b, n in ((1 << 20, 10), (1 << 27, 8192)))
    assert 0 < w1 < w2 < (1 << 27)
    with pytest.raises(press.PressError):
        press.blow5_transcode(BLOW5, os.devnull, record_method=0, deflate="device")
    with pytest.raises(press.PressError):
        press.blow5_transcode(BLOW5, os.devnull, deflate="gpu")


def test_write_image_needs_a_zlib_writer(tmp_path):
    """press_hip_blow5_write_image on a writer with record method none: refused, nothing written"""
    import ctypes
    lib = press.load_library()
    recs = real_records()[:1]
    image, rec_off, raw = D.image(recs)
    pres = [np.frombuffer(recs[0][:60], dtype=np.uint8)]
    img = np.frombuffer(image, dtype=np.uint8)
    sizes = {}
    for method in (0, 1):
        dst = str(tmp_path / ("w%d.blow5" % method))
        rd = press.Blow5Reader(BLOW5)
        w = ctypes.c_void_p()
        press._blow5_call("press_hip_blow5_create", dst.encode(), rd._h, method, 1, ctypes.byref(w))
        rd.close()
        try:
            if method == 0:
                with pytest.raises(press.PressError, match="zlib"):
                    press._blow5_write_image(w, img, np.array(rec_off, dtype=np.uint64), pres)
            else:
                press._blow5_write_image(w, img, np.array(rec_off, dtype=np.uint64), pres)
                with pytest.raises(press.PressError):  # a length field that is not the record's extent
                    bad = img.copy()
                    bad[0] ^= 1
                    press._blow5_write_image(w, bad, np.array(rec_off, dtype=np.uint64), pres)
        finally:
            press._blow5_call("press_hip_blow5_finish", w)
        sizes[method] = os.path.getsize(dst)
    assert sizes[1] == sizes[0] + len(image)  # header | (records) | end marker


# ------------------------------------------------------------------ GPU: the device against the model

@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.use_torch_stream()
    try:
        yield lb
    finally:
        torch.cuda.synchronize()
        press.use_torch_stream()
        torch.cuda.empty_cache()


def arrays(cases):
    return ([np.frombuffer(p, dtype=np.uint8) for _, p, _, _ in cases], [np.frombuffer(s, dtype=np.uint8) for _, _, s, _ in cases],
            [np.frombuffer(q, dtype=np.uint8) for _, _, _, q in cases])


def first_difference(image, want, rec_off, names):
    a, b = np.frombuffer(bytes(image), dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    if a.size != b.size:
        return "the image has %d bytes, the model's %d" % (a.size, b.size)
    i = int(np.flatnonzero(a != b)[0])
    k = int(np.searchsorted(np.asarray(rec_off[:-1], dtype=np.int64), i, side="right")) - 1
    return "%d bytes differ, the first at %d: byte %d of record %d (%s): %#x, the model %#x" % (
        int((a != b).sum()), i, i - int(rec_off[k]), k, names[k], int(a[i]), int(b[i]))


@pytest.mark.gpu
def test_gpu_host_form_equals_the_model(lib):
    recs, want, want_off, want_raw = battery_model()
    names = [c[0] for c in battery()]
    pres, sigs, posts = arrays(battery())
    image, rec_off, raw = press.blow5_deflate_batch_host(pres, sigs, posts, 1)
    assert [int(x) for x in rec_off] == want_off
    assert [int(x) for x in raw] == want_raw
    assert image.tobytes() == want, first_difference(image, want, want_off, names)
    assert 1 in want_raw and 0 in want_raw


class DeviceBatch:
    """a batch for the device-resident form: side and signal arenas with odd offsets, and the outputs"""

    def __init__(self, cases, signal_method=1):
        import torch
        self.n = n = len(cases)
        pres, sigs, posts = arrays(cases)
        side, tab = deflate.side_arena(pres, posts)
        arena, off, ln = press._streams_arena([s.tobytes() for s in sigs])
        self.record_bytes = sum(len(p) + 8 + len(s) + len(q) for _, p, s, q in cases)
        self.signal_method = signal_method
        dev = "cuda"
        self.side = torch.from_numpy(side.copy()).to(dev)
        self.tab = torch.from_numpy(tab.reshape(-1).view(np.int64).copy()).to(dev)
        self.src = torch.from_numpy(arena.copy()).to(dev)
        self.sig = torch.zeros_like(self.src)
        self.sig_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        self.sig_len = torch.from_numpy(ln.view(np.int64).copy()).to(dev)
        cap = press.blow5_deflate_image_cap(self.record_bytes, n)
        self.image = torch.full((cap,), 0xA5, dtype=torch.uint8, device=dev)
        self.rec_off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
        self.raw = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)

    def load(self, src=None):
        self.sig.copy_(self.src if src is None else src, non_blocking=True)

    def run(self):
        press.blow5_deflate_batch(self.side, self.tab, self.sig, self.sig_off, self.sig_len, self.record_bytes, self.image,
                                  self.rec_off, self.raw, self.signal_method)

    def sizes(self):
        return press.blow5_deflate_sizes(self.side, self.tab, self.sig, self.sig_off, self.sig_len, self.record_bytes,
                                         self.signal_method)

    def outputs(self):
        return {"image": self.image, "rec_off": self.rec_off, "raw": self.raw}


def check_device(b, want, want_off, want_raw, names):
    rec_off = b.rec_off.cpu().numpy()
    assert [int(x) for x in rec_off] == want_off
    assert [int(x) for x in b.raw.cpu().numpy()] == want_raw
    image = b.image.cpu().numpy()
    assert image[:len(want)].tobytes() == want, first_difference(image[:len(want)], want, want_off, names)
    assert not image[len(want):].any()  # the rest of the capacity: zeros


@pytest.mark.gpu
def test_gpu_device_form_equals_the_model(lib):
    import torch
    recs, want, want_off, want_raw = battery_model()
    b = DeviceBatch(battery())
    b.load()
    need = b.sizes()
    b.run()
    torch.cuda.synchronize()
    assert [int(x) for x in need.cpu().numpy()] == [want_off[k + 1] - want_off[k] for k in range(b.n)]
    check_device(b, want, want_off, want_raw, [c[0] for c in battery()])
    assert int(lib.press_hip_blow5_deflate_workspace_bytes(b.record_bytes, b.n)) > 0


@pytest.mark.gpu
def test_gpu_signal_method_0_and_real_records(lib):
    """int16 samples as the signal field (the length field counts samples), and the real svb-zd records"""
    s = (np.cumsum(np.random.default_rng(4).integers(-20, 21, 5001)) + 400).astype(np.int16)
    cases = [("samples", nz(50), s.tobytes(), nz(4)), ("short", nz(3), s[:7].tobytes(), b"")]
    pres, sigs, posts = arrays(cases)
    image, rec_off, raw = press.blow5_deflate_batch_host(pres, sigs, posts, 0)
    recs = [D.frame(p, g, q, 0) for _, p, g, q in cases]
    want, want_off, want_raw = D.image(recs)
    assert image.tobytes() == want and [int(x) for x in rec_off] == want_off and [int(x) for x in raw] == want_raw
    real = real_records()
    cases = [("real %d" % k, r[:60], r[68:], b"") for k, r in enumerate(real)]
    pres, sigs, posts = arrays(cases)
    image, rec_off, raw = press.blow5_deflate_batch_host(pres, sigs, posts, 1)
    want, want_off, want_raw = D.image(real)
    assert image.tobytes() == want, first_difference(image, want, want_off, [c[0] for c in cases])
    assert [int(x) for x in rec_off] == want_off and not raw.any()


@pytest.mark.gpu
def test_gpu_refusals(lib):
    """a record that does not fit image_cap is not written; a part outside its arena and a failed signal are refused"""
    import torch
    cases = battery()[:6]
    recs = [D.frame(p, s, q, 1) for _, p, s, q in cases]
    want, want_off, want_raw = D.image(recs)
    b = DeviceBatch(cases)
    b.load()
    cap = (want_off[4] + 3) // 4 * 4  # records 0 .. 3 fit; 4 only if it ends inside the rounding
    b.image = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    b.run()
    torch.cuda.synchronize()
    fits = [want_off[k + 1] <= cap for k in range(b.n)]
    assert [int(x) for x in b.rec_off.cpu().numpy()] == want_off
    assert [int(x) for x in b.raw.cpu().numpy()] == [want_raw[k] if fits[k] else 0xFF for k in range(b.n)]
    end = max(want_off[k + 1] for k in range(b.n) if fits[k])
    img = b.image.cpu().numpy()
    assert img[:end].tobytes() == want[:end] and not img[end:].any()
    b = DeviceBatch(cases)
    b.load()
    b.sig_len[2] = -1           # what a refused read's out_len says
    b.tab[4 * 3 + 1] = 1 << 40  # a front part that leaves the side arena
    need = b.sizes()
    b.run()
    torch.cuda.synchronize()
    keep = [k for k in range(b.n) if k not in (2, 3)]
    w2, off2, raw2 = D.image([recs[k] for k in keep])
    assert [int(x) for x in need.cpu().numpy()] == [-1 if k in (2, 3) else want_off[k + 1] - want_off[k] for k in range(b.n)]
    assert [int(x) for x in b.raw.cpu().numpy()] == [0xFF if k in (2, 3) else want_raw[k] for k in range(b.n)]
    assert b.image.cpu().numpy()[:len(w2)].tobytes() == w2 and int(b.rec_off[-1]) == len(w2)


@pytest.mark.gpu
def test_gpu_same_image_behind_scratch_fills(lib):
    """tests/test_scratch_independence.py's idea on the new call: the outputs behind press.scratch_fill are the warm-up's"""
    import test_scratch_independence as SI
    recs, want, want_off, want_raw = battery_model()
    b = DeviceBatch(battery())

    def run():
        b.image.fill_(0xA5)
        b.rec_off.fill_(-7)
        b.raw.fill_(0x77)
        b.load()
        b.run()
        return {k: v.clone() for k, v in b.outputs().items()}

    def check(warm):
        assert warm["image"][:len(want)].tobytes() == want and [int(x) for x in warm["rec_off"]] == want_off
    SI.filled(lib, ("blow5_deflate_batch",), run, check, fills=(0x00, 0xFF))
    pres, sigs, posts = arrays(battery()[:20])
    first = press.blow5_deflate_batch_host(pres, sigs, posts, 1)
    for byte in (0x00, 0xFF):
        press.scratch_fill(byte)
        again = press.blow5_deflate_batch_host(pres, sigs, posts, 1)
        assert all(np.array_equal(x, y) for x, y in zip(first, again)), "host form behind fill %#x" % byte


from test_stream_contract import cycles_per_ms  # noqa: E402,F401  (the fixture: torch.cuda._sleep's unit)


@pytest.mark.gpu
def test_gpu_device_form_only_enqueues(lib, cycles_per_ms):
    """the stream contract: behind a delay held on the current stream the two device-resident calls return at once, and
    what they then make is the image of the signal fields that were loaded on that stream behind the delay"""
    import test_stream_contract as SC
    cases = [c for c in battery() if len(c[2]) < 5000][:24]
    b = DeviceBatch(cases)
    decoy = b.src.clone()
    decoy[decoy != 0] ^= 0x55  # the same runs, other literals (a byte of 0x55 becomes a zero: the model says what that gives)
    srcs = {"D": decoy, "R": b.src}
    s = SC.use_stream(lib, "torch")
    need = {}
    steps = [(lambda: need.__setitem__("need", b.sizes()), False), (b.run, False)]
    image, rec_off, raw = SC.decoy_run("blow5_deflate", s, cycles_per_ms, lambda which: b.load(srcs[which]), steps,
                                       [b.image, b.rec_off, b.raw])
    recs = [D.frame(p, g, q, 1) for _, p, g, q in cases]
    want, want_off, want_raw = D.image(recs)
    assert [int(x) for x in rec_off] == want_off and [int(x) for x in raw] == want_raw
    assert image[:len(want)].tobytes() == want
    assert [int(x) for x in need["need"].cpu().numpy()] == [want_off[k + 1] - want_off[k] for k in range(b.n)]
    press.use_torch_stream()


# ------------------------------------------------------------------ files

def read_index(path):
    d = open(path, "rb").read()
    assert d[:9] == b"SLOW5IDX\x01" and d[-8:] == b"XDI5WOLS"
    p, out = 64, []
    while p < len(d) - 8:
        idl, = struct.unpack("<H", d[p:p + 2])
        rid = d[p + 2:p + 2 + idl].decode()
        off, size = struct.unpack("<QQ", d[p + 2 + idl:p + 18 + idl])
        out.append((rid, off, size))
        p += 18 + idl
    assert p == len(d) - 8
    return out


def read_all(path):
    rd = press.Blow5Reader(path)
    methods = (rd.record_method, rd.signal_method)
    got = rd.next_batch()
    rd.close()
    return methods, got


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"verify": True}, {"degrade_bits": 3}, {"signal_method": 0}])
def test_gpu_transcode_device_deflate(lib, tmp_path, kw):
    """blow5_transcode(deflate="device", index=True): the file reads back to the ids and signals of the host form's file
    (the reference's slow5lib reads it too, where oracle/_ref is built), and its index points at the records"""
    import subprocess
    import test_blow5 as B
    host, dev = str(tmp_path / "host.blow5"), str(tmp_path / "dev.blow5")
    assert press.blow5_transcode(BLOW5, host, index=True, **kw) == 3
    assert press.blow5_transcode(BLOW5, dev, index=True, deflate="device", **kw) == 3
    mh, gh = read_all(host)
    md, gd = read_all(dev)
    assert md == mh == (1, kw.get("signal_method", 1)) and gd == gh and len(gd) == 3
    if not kw:
        gold = B.golden_reads()
        assert [(i, s) for i, _, s in gd] == B.parse_blow5_py(BLOW5)
        for rid, sig in B.read_blow5_py(dev):
            assert np.array_equal(sig, gold[rid]), rid
        tool = os.path.join(_libs.ORACLE_DIR, "_ref", "ref_dump_blow5")
        if os.path.exists(tool):  # (as the existing BLOW5 tests: only where the reference is built)
            got = B._ref_dump(dev, tmp_path)
            assert set(got) == set(gold) and all(np.array_equal(got[k], gold[k]) for k in gold)
            ids = [i for i, _, _ in gd][::-1]
            got = B._ref_dump(dev, tmp_path, ids)
            assert list(got) == ids and all(np.array_equal(got[k], gold[k]) for k in ids)
    data = open(dev, "rb").read()
    idx = read_index(dev + ".idx")
    assert [i for i, _, _ in idx] == [i for i, _, _ in gd] == [i for i, _, _ in read_index(host + ".idx")]
    end = None
    for rid, off, size in idx:
        ln, = struct.unpack("<Q", data[off:off + 8])
        assert ln == size - 8 and (end is None or off == end)
        rec = zlib.decompress(data[off + 8:off + size])
        idl, = struct.unpack("<H", rec[:2])
        assert rec[2:2 + idl].decode() == rid
        end = off + size
    assert data[end:] == b"5WOLB"


@pytest.mark.gpu
def test_gpu_write_like_device_deflate(lib, tmp_path):
    import test_blow5 as B
    fields = [f for _, f in B.parse_blow5_py(BLOW5)]
    many = [fields[k % 3][: 4 + (len(fields[k % 3]) - 4) // (1 + k % 5)] for k in range(30)]
    dst = str(tmp_path / "many.blow5")
    ids = press.blow5_write_like(dst, BLOW5, many, index=True, deflate="device")
    _, got = read_all(dst)
    assert [g[0] for g in got] == ids and [g[2] for g in got] == [bytes(m) for m in many]
    assert [i for i, _, _ in read_index(dst + ".idx")] == ids
