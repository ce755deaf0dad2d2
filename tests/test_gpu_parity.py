"""GPU: the HIP path (through the C ABI) against the oracle and the golden vectors.

These read like the reference's own test_X functions (press/test.c:1756-1815):
bound -> press -> depress -> compare - but every sample is compared (the reference
stops at n/2, test.c:1804) and the stream bytes are checked too."""
import hashlib
import json
import os

import numpy as np
import pytest

import _libs
from honours_amd import press, synth

pytestmark = pytest.mark.gpu

DET = [m for m in press.METHODS if not m.startswith("zstd_")]
ZSTD = [m for m in press.METHODS if m.startswith("zstd_")]


def sha(b):
    return hashlib.sha256(b).hexdigest()[:32]


def zd_of(sig):
    s = np.asarray(sig, dtype=np.int16).astype(np.uint16)
    d = (s - np.concatenate([[0], s[:-1]]).astype(np.uint16)).astype(np.int16).astype(np.int32)
    return ((d << 1) ^ (d >> 15)).astype(np.uint16)


def shuff_ok(m, sig):
    return (not m.startswith("shuffman")) or int((zd_of(sig)[1:] <= 255).sum()) >= 1


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    press.load_library()
    press.load_table()
    yield


def check_read(oracle, m, sig, want=None):
    """the test_X pattern + byte parity with the oracle"""
    sig = np.ascontiguousarray(sig, dtype=np.int16)
    n = sig.size
    if want is None:
        ret, want = oracle.press(m, sig)
        assert ret == 0
    ret, got = press.press(m, sig, cap=max(len(want) + 64, press.bound(m, n) + 1024))
    assert ret == 0, (m, n, press.last_error())
    if m in DET:
        assert got == want, (m, n, len(got), len(want))
    ret, back = press.depress(m, got, n)
    if m in _libs.RC_FAMILY:
        # reference quirk (TurboRC rcutil_.h:161): once the coder's output reaches n*255/256 - 8 bytes it
        # stores the bytes raw, and nothing tells its decoder - such reads (a few dozen samples) are outside
        # the reference's lossless domain; there the GPU must still do what the reference's decoder does
        ro, oback = oracle.depress(m, want, n)
        assert ro == 0 and ret == 0 and np.array_equal(back, oback), (m, n)
        if not _libs.rc_stored_raw(m, want, n):
            assert np.array_equal(back, sig), (m, n)
        return
    assert ret == 0 and back.size == n and np.array_equal(back, sig), (m, n)
    # and the oracle's stream decodes on the GPU (cross decode)
    ret, back = press.depress(m, want, n)
    assert ret == 0 and np.array_equal(back, sig), (m, n)


def test_three_reads(oracle, golden_dir):
    """config 1 of BASELINE.json: data/three-reads.blow5, every hot-path method"""
    meta = json.load(open(os.path.join(golden_dir, "three_reads.json")))
    sig = np.fromfile(os.path.join(golden_dir, "three_reads.i16.bin"), dtype=np.int16)
    o = 0
    for r in meta["reads"]:
        s = sig[o:o + r["n"]]
        o += r["n"]
        for m, e in r["methods"].items():
            ret, got = press.press(m, s)
            assert ret == 0, (m, press.last_error())
            if m in DET:
                assert len(got) == e["len"] and sha(got) == e["sha256_32"], (m, r["n"])
            else:
                # zstd stage: libzstd-version dependent bytes ("parity unpinned"); the frame
                # must decode to the oracle's pre-zstd buffer and be no larger than +1 %
                assert len(got) <= e["len"] * 1.01 + 16
            ret, back = press.depress(m, got, r["n"])
            assert ret == 0 and np.array_equal(back, s), m


def test_micro_kats(oracle, golden_dir):
    vec = json.load(open(os.path.join(golden_dir, "micro_kats.json")))["vectors"]
    for v in vec:
        s = np.array(v["input"], dtype=np.int16)
        for m, hexs in v["streams"].items():
            want = bytes.fromhex(hexs)
            ret, got = press.press(m, s, cap=max(len(want) + 64, press.bound(m, len(s))))
            assert ret == 0 and got == want, (v["name"], m, got.hex(), hexs)
            if m.startswith("shuffman") and len(want) <= 2 + 4 + 4:
                continue  # header-only Huffman stream: outside the decoder's domain (quirk 2)
            ret, back = press.depress(m, want, len(s))
            assert ret == 0 and np.array_equal(back, s), (v["name"], m)


def test_synth_kats(oracle, golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "synth_kats.json")))["cases"]
    for c in cases:
        s = synth.synth_read(c["seed"], c["read"], c["n"], c["first"])
        for m, e in c["methods"].items():
            ret, got = press.press(m, s)
            assert ret == 0, (m, c["n"], press.last_error())
            if m in DET:
                assert len(got) == e["len"] and sha(got) == e["sha256_32"], (m, c["n"])
            if m.startswith("shuffman") and c["n"] == 1:
                continue
            ret, back = press.depress(m, got, c["n"])
            if m in _libs.RC_FAMILY and _libs.rc_stored_raw(m, got, c["n"]):
                # outside the reference's lossless domain: the GPU does what the reference's decoder does
                ro, oback = oracle.depress(m, got, c["n"])
                assert ret == 0 and ro == 0 and np.array_equal(back, oback), (m, c["n"])
                continue
            assert ret == 0 and np.array_equal(back, s), (m, c["n"])


@pytest.mark.parametrize("m", DET)
def test_random_vs_oracle(oracle, m):
    """randomised reads incl. heavy exceptions, wraparound, q > 0, tile-boundary lengths"""
    rng = np.random.default_rng(abs(hash(m)) % (1 << 31))
    lens = [1, 2, 3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 2047, 2048, 2049, 2055, 4096, 4104, 6000, 20000]
    for it, n in enumerate(lens):
        exr = [0.0, 0.001, 0.02, 0.15][it % 4]
        d = rng.integers(-60, 60, size=n)
        ex = rng.random(n) < exr
        d[ex] = rng.integers(-40000, 40000, size=int(ex.sum()))
        s = (np.cumsum(d) + 500).astype(np.int64).astype(np.uint16).view(np.int16)
        if it % 5 == 0:
            s = ((s >> 3) << 3).astype(np.int16)
        if not shuff_ok(m, s):
            continue
        check_read(oracle, m, s)
    # s[i] = 128 i: every delta is the exception 256 and every position delta 0, so both blocks of the bit-packed
    # forms have width 0 and 100 exceptions cost no byte (vbbe21_zd: 16 bytes)
    s = (128 * np.arange(101)).astype(np.int16)
    if shuff_ok(m, s):
        check_read(oracle, m, s)


@pytest.mark.parametrize("m", DET)
def test_multi_chunk_reads(oracle, m):
    """reads longer than one 32768-sample chunk: exceptions on both sides of chunk and
    wave-quarter boundaries, exception-dense stretches, ragged ends, q > 0"""
    rng = np.random.default_rng(abs(hash("mc" + m)) % (1 << 31))
    for it, n in enumerate([32767, 32768, 32769, 40961, 65536, 65543, 100003, 131072 + 17]):
        exr = [0.0005, 0.0, 0.01, 0.08][it % 4]
        d = rng.integers(-60, 60, size=n)
        ex = rng.random(n) < exr
        # make sure the boundaries themselves are hit
        for b in (8191, 8192, 8193, 32767, 32768, 32769, 65535, 65536):
            if b < n and it % 2 == 0:
                ex[b] = True
        d[ex] = rng.integers(-30000, 30000, size=int(ex.sum()))
        s = (np.cumsum(d) + 500).astype(np.int64).astype(np.uint16).view(np.int16)
        if it == 3:
            s = ((s >> 2) << 2).astype(np.int16)  # q = 2 for ex-zd
        if m.startswith("shuffman") and not shuff_ok(m, s):
            continue
        ret, want = oracle.press(m, s, cap=int(oracle.bound(m, n)) + 6 * n + 1024)
        assert ret == 0
        if m.startswith("shuffman") and m != "shuffman_vbe21_zd" and len(want) > 60000 and exr > 0.005:
            continue  # press.c:4520: the b/sb/ss variants keep the section length in 16 bits
        check_read(oracle, m, s, want)


@pytest.mark.parametrize("m", ZSTD)
def test_zstd_compositions(oracle, m):
    """inner stream on the GPU, libzstd on the host: round trip + the oracle's decoder
    accepts the frame (same inner bytes)"""
    sig, off = synth.synth_batch(5, 0, 3)
    for k in range(3):
        s = sig[int(off[k]):int(off[k + 1])]
        ret, got = press.press(m, s)
        assert ret == 0
        ret, back = oracle.depress(m, got, s.size)
        assert ret == 0 and np.array_equal(back, s)
        ret, back = press.depress(m, got, s.size)
        assert ret == 0 and np.array_equal(back, s)


def test_capacity_is_respected(oracle):
    """the library never writes past *nout (include/press_hip.h: deviation from the reference)"""
    s = np.array([0, 1000] * 50, dtype=np.int16)  # every delta is an exception
    for m in DET:
        if not shuff_ok(m, s):
            continue
        ret, want = oracle.press(m, s, cap=10000)
        assert ret == 0
        ret, got = press.press(m, s, cap=len(want) - 1)  # canaries checked inside press()
        if m in ("svb12", "svb12_zd", "svb_zd", "slow5_svb_zd"):
            # worst case of the format is what is checked up front
            assert ret != 0
        else:
            assert ret != 0, m
        ret, got = press.press(m, s, cap=len(want) + (200 if m.startswith("svb") or m.startswith("slow5") else 0))
        assert ret == 0 and got == want, m


def test_malformed_streams_do_not_crash():
    rng = np.random.default_rng(9)
    for m in DET:
        for n in (8, 100, 3000):
            junk = rng.integers(0, 256, size=int(rng.integers(1, 4000)), dtype=np.uint8).tobytes()
            ret, back = press.depress(m, junk, n)  # canaries checked inside depress()
            assert back.size <= n


@pytest.mark.parametrize("m", ["svb12_zd", "svb_zd", "vbe21_zd", "vbsse21_zd", "hasgam_vbsse21_zdq",
                               "shuffman_vbe21_zd", "shuffman_vbbe21_zd"])
def test_batch_host_matches_per_read(oracle, m):
    """the batch entry (host buffers) == per-read calls, ragged lengths incl. tiny reads"""
    sig, off = synth.synth_batch(11, 100, 12)
    reads = [sig[int(off[k]):int(off[k + 1])] for k in range(12)]
    reads += [reads[0][:5], reads[1][:2048], reads[2][:2049], reads[3][:9]]
    streams = press.press_batch_host(m, reads)
    for r, st in zip(reads, streams):
        ret, want = oracle.press(m, r)
        assert ret == 0 and st == want, (m, len(r))
    back = press.depress_batch_host(m, streams, [len(r) for r in reads])
    for r, b in zip(reads, back):
        assert b is not None and np.array_equal(b, r), (m, len(r))


def _device_batch(m, sig_al, starts, n_np, dev):
    """press_batch + depress_batch with device-resident tensors on torch's stream (what bench.py times)
    -> (streams as bytes per read, decoded tensor, decoded counts)"""
    import torch

    nreads = len(n_np)
    d_off = torch.from_numpy(starts[:-1].astype(np.int64)).to(dev)
    d_n = torch.from_numpy(n_np.astype(np.int32)).to(dev)
    caps = np.array([press.bound(m, int(x)) + 64 for x in n_np], dtype=np.int64)
    caps = (caps + 127) // 128 * 128
    out_off = np.concatenate([[0], np.cumsum(caps)])
    d_out = torch.empty(int(out_off[-1]) + 64, dtype=torch.uint8, device=dev)
    d_out_off = torch.from_numpy(out_off).to(dev)
    d_len = torch.zeros(nreads, dtype=torch.int64, device=dev)
    press.press_batch(m, sig_al, d_off, d_n, d_out, d_out_off, d_len)
    torch.cuda.synchronize()
    lens = d_len.cpu().numpy()
    assert (lens > 0).all() and (lens <= caps).all(), m
    arena = d_out.cpu().numpy()
    streams = [arena[int(out_off[k]):int(out_off[k]) + int(lens[k])].tobytes() for k in range(nreads)]
    d_back = torch.zeros_like(sig_al)
    d_outn = torch.zeros(nreads, dtype=torch.int32, device=dev)
    press.depress_batch(m, d_out, d_out_off[:-1].contiguous(), d_len, d_back, d_off, d_n, d_outn)
    torch.cuda.synchronize()
    return streams, d_back, d_outn.cpu().numpy()


@pytest.mark.parametrize("m", sorted(press.METHODS))
def test_batch_device_resident_roundtrip(oracle, m):
    """device-resident batch (the path bench.py times), EVERY batch method, every read: the stream
    of each read equals the oracle's (zstd frames, whose bytes are not pinned: the oracle's decoder -
    libzstd + the inner codec - reads them back), and the device decodes its own batch losslessly"""
    import torch

    dev = torch.device("cuda:0")
    press.use_torch_stream()
    nreads = 64
    sig_al, starts, n_np = synth.synth_batch_torch(3, 0, nreads, dev, align=8)
    total = int(starts[-1])
    sig_al = torch.cat([sig_al, torch.zeros(64, dtype=torch.int16, device=dev)])
    host = sig_al.cpu().numpy()
    streams, d_back, outn = _device_batch(m, sig_al, starts, n_np, dev)
    for k in range(nreads):
        s = host[int(starts[k]):int(starts[k]) + int(n_np[k])]
        if m in DET:
            ret, w = oracle.press(m, s)
            assert ret == 0 and streams[k] == w, (m, k, len(streams[k]), len(w))
        else:
            ret, back = oracle.depress(m, streams[k], s.size)
            assert ret == 0 and np.array_equal(back, s), (m, k)
    assert np.array_equal(outn, n_np.astype(np.int32)), m
    assert torch.equal(d_back[:total], sig_al[:total]), m


@pytest.mark.parametrize("m", ["shuffman_vbe21_zd", "svb12_zd", "zstd_svb_zd", "hasgam_vbsse21_zdq"])
def test_config5_shape(oracle, m):
    """BASELINE.json config 5's shape: fixed 200 000-sample reads (what bench.py --gpus N > 1 runs on every
    rank), device resident; a few dozen reads against the oracle"""
    import torch

    dev = torch.device("cuda:0")
    press.use_torch_stream()
    nreads = 24
    sig_al, starts, n_np = synth.synth_batch_torch(20261004, 4096, nreads, dev, fixed_len=200000, align=64)
    assert (n_np == 200000).all()
    total = int(starts[-1])
    sig_al = torch.cat([sig_al, torch.zeros(64, dtype=torch.int16, device=dev)])
    host = sig_al.cpu().numpy()
    streams, d_back, outn = _device_batch(m, sig_al, starts, n_np, dev)
    for k in range(nreads):
        s = host[int(starts[k]):int(starts[k]) + 200000]
        # the generator is counter based: the device's reads are the numpy generator's
        if k < 2:
            assert np.array_equal(s, synth.synth_read(20261004, 4096 + k, 200000,
                                                      synth.read_lengths(20261004, 4096 + k, 1, 200000)[1][0]))
        if m in DET:
            ret, w = oracle.press(m, s)
            assert ret == 0 and streams[k] == w, (m, k)
        else:
            ret, back = oracle.depress(m, streams[k], s.size)
            assert ret == 0 and np.array_equal(back, s), (m, k)
    assert (outn == 200000).all()
    assert torch.equal(d_back[:total], sig_al[:total]), m


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("m", ["svb12_zd", "shuffman_vbe21_zd", "zstd_svb_zd", "vbsse21_zd"])
def test_host_batch_staging(oracle, m, pinned):
    """host buffers through the batch API (device_resident = 0): pageable memory goes through the
    page-locked staging buffers (several 32-MiB chunks here), press_hip_host_alloc memory by direct DMA;
    streams land in the caller's slots, samples in the caller's layout, padding untouched (pageable)"""
    sig, off = synth.synth_batch(13, 200, 300)  # ~34 M samples: 68 MB in, > 2 staging chunks
    reads = [sig[int(off[k]):int(off[k + 1])] for k in range(300)]
    reads += [reads[0][:5], reads[1][:2049], reads[2][:9]]
    hb = press.HostBatch(m, reads, pinned=pinned)
    hb.back[:] = 0x5A5A
    hb.press()
    st = hb.streams()
    for k in (0, 1, 2, 150, 299, 300, 301, 302):
        if m in DET:
            ret, w = oracle.press(m, reads[k])
            assert ret == 0 and st[k] == w, (m, k)
        else:
            ret, back = oracle.depress(m, st[k], len(reads[k]))
            assert ret == 0 and np.array_equal(back, reads[k]), (m, k)
    hb.depress()
    assert hb.lossless(), m
    if not pinned:
        for o, k, nxt in zip(hb.off[:-1], hb.ns[:-1], hb.off[1:]):
            assert (hb.back[int(o) + int(k):int(nxt)] == 0x5A5A).all()
    hb.close()


def test_shutdown_releases_every_buffer(oracle):
    """press_hip_shutdown() must free ALL scratch (the zstd buffers were forgotten) so that a
    later press_hip_set_device() cannot leave pointers of the old device behind"""
    import ctypes

    lib = press.load_library()
    lib.press_hip_scratch_buffers.restype = ctypes.c_uint32
    lib.press_hip_scratch_buffers.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    sig, off = synth.synth_batch(2, 0, 6)
    reads = [sig[int(off[k]):int(off[k + 1])] for k in range(6)]
    for m in ("zstd_svb_zd", "shuffman_vbe21_zd", "rc_vbe21_zd"):
        st = press.press_batch_host(m, reads)
        back = press.depress_batch_host(m, st, [len(r) for r in reads])
        assert all(np.array_equal(b, r) for b, r in zip(back, reads))
    nbytes = ctypes.c_uint64()
    nbuf = lib.press_hip_scratch_buffers(ctypes.byref(nbytes))
    assert nbuf >= 40 and nbytes.value > 0
    lib.press_hip_shutdown()
    assert lib.press_hip_scratch_buffers(ctypes.byref(nbytes)) == nbuf and nbytes.value == 0
    # the library comes back by itself (the table has to be loaded again)
    press.load_table()
    st = press.press_batch_host("zstd_svb_zd", reads)
    back = press.depress_batch_host("zstd_svb_zd", st, [len(r) for r in reads])
    assert all(np.array_equal(b, r) for b, r in zip(back, reads))
    ret, got = press.press("shuffman_vbe21_zd", reads[0])
    assert ret == 0 and got == oracle.press("shuffman_vbe21_zd", reads[0])[1]


@pytest.mark.parametrize("m", ["svb12_zd", "vbe21_zd", "shuffman_vbe21_zd", "rc_vbe21_zd", "zstd_svb_zd"])
def test_scratch_plan_is_what_is_allocated(m):
    """press_hip_workspace_bytes() is exact: from an empty library, one device-resident press and one depress of a
    batch leave every scratch buffer at the size the plan asks for plus DevBuf's growth slack (n + n / 8 + 4096 per
    buffer), and nothing else - device-resident calls touch no staging buffer"""
    import ctypes

    import torch

    lib = press.load_library()
    lib.press_hip_scratch_buffers.restype = ctypes.c_uint32
    lib.press_hip_scratch_buffers.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    dev = torch.device("cuda:0")
    nreads = 16
    sig_al, starts, n_np = synth.synth_batch_torch(5, 0, nreads, dev, align=8)
    sig_al = torch.cat([sig_al, torch.zeros(64, dtype=torch.int16, device=dev)])
    torch.cuda.synchronize()
    lib.press_hip_shutdown()
    try:
        if m.startswith("shuffman"):
            press.load_table()
        press.use_torch_stream()
        streams, d_back, outn = _device_batch(m, sig_al, starts, n_np, dev)
        assert np.array_equal(outn, n_np.astype(np.int32)) and torch.equal(d_back, sig_al), m
        nbytes = ctypes.c_uint64()
        nbuf = lib.press_hip_scratch_buffers(ctypes.byref(nbytes))
        ws = int(lib.press_hip_workspace_bytes(press.METHODS[m], sig_al.numel(), nreads))
        print(m, "workspace_bytes", ws, "allocated", nbytes.value, "buffers", nbuf)
        assert ws <= nbytes.value <= ws + ws // 8 + 4096 * nbuf, (m, ws, nbytes.value, nbuf)
    finally:
        press.load_table()  # (the rest of the module runs with the table)


# ---------------------------------------------------------------- static Huffman: tables other than NA12878

def _canonical_table(lens):
    """prefix code with the given lengths (Kraft sum <= 1): canonical codes, emitted MSB first
    -> bit k of `bits` = k-th emitted bit (the table file's order, huffman.c:427-439)"""
    order = sorted(range(256), key=lambda s: (lens[s], s))
    code, prev = 0, lens[order[0]]
    bits = [0] * 256
    for s in order:
        code <<= lens[s] - prev
        prev = lens[s]
        bits[s] = int(format(code, "0%db" % lens[s])[::-1], 2)  # MSB-first emission -> LSB-first integer
        code += 1
    assert code <= 1 << prev
    return bits


def _write_table(path, lens, bits):
    """the reference's table file (huffman.c:549 read_code_table): u32 BE count, u32 (unused here),
    then per symbol: symbol, number of bits, the bits packed from bit 0 of each byte upwards"""
    b = bytearray((256).to_bytes(4, "big") + bytes(4))
    for s in range(256):
        b += bytes([s, lens[s]]) + bits[s].to_bytes((lens[s] + 7) // 8, "little")
    with open(path, "wb") as f:
        f.write(bytes(b))


TABLES = {
    # shortest code 1 bit -> 32-bit subsequences; one 9-bit pattern is no code at all
    "min1_incomplete": [1] + [9] * 255,
    # shortest code 2 bits -> 64-bit subsequences; incomplete as well
    "min2_incomplete": [2, 2, 2] + [10] * 253,
    # long codes: second-level tables and, beyond 64 long prefixes, the trie walk
    "long_codes": [6] * 16 + [7] * 32 + [8] * 64 + [9] * 32 + [10] * 32 + [13] * 16 + [16] * 16 + [20] * 16
                  + [22] * 16 + [24] * 16,
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_huffman_other_tables(oracle, tmp_path, name):
    """shuffman_* with a caller-supplied table (read_code_table + build_symbol_encoder in the
    reference's interface): subsequence sizes 32/64/128, bit patterns that are no code, codes of
    up to 24 bits; multi-tile reads, byte parity with the oracle and lossless both ways"""
    lens = TABLES[name]
    assert len(lens) == 256
    path = str(tmp_path / (name + ".huffman"))
    _write_table(path, lens, _canonical_table(lens))
    rng = np.random.default_rng(len(name))
    try:
        oracle.load_table(path)
        press.use_table(path)
        for n, spread in ((1, 3), (2, 3), (9, 200), (5000, 3), (70000, 90), (150001, 127)):
            # random walk: zig-zag deltas cover [0, 2*spread]; a few exceptions sprinkled in
            steps = rng.integers(-spread, spread + 1, size=n)
            steps[rng.random(n) < 0.01] += 400
            sig = np.cumsum(steps).astype(np.int16)
            for m in ("shuffman_vbe21_zd", "shuffman_vbsse21_zd"):
                if shuff_ok(m, sig):
                    check_read(oracle, m, sig)
    finally:
        oracle.load_table()
        press.use_table()


def test_huffman_table_with_fewer_symbols(oracle, tmp_path):
    """a table file that lists fewer than 256 symbols (huffman.c:549 takes count <= 256): reads that do
    not use the missing values code exactly as with the oracle; a read that does fails (the reference
    dereferences a NULL code there, huffman.c:860) - and only that read"""
    lens = [4] * 8 + [5] * 16  # 24 symbols, Kraft sum = 1
    order = sorted(range(24), key=lambda s: (lens[s], s))
    code, prev, bits = 0, lens[order[0]], [0] * 24
    for sy in order:
        code <<= lens[sy] - prev
        prev = lens[sy]
        bits[sy] = int(format(code, "0%db" % lens[sy])[::-1], 2)
        code += 1
    blob = bytearray((24).to_bytes(4, "big") + bytes(4))
    for sy in range(24):
        blob += bytes([sy, lens[sy]]) + bits[sy].to_bytes((lens[sy] + 7) // 8, "little")
    path = str(tmp_path / "partial.huffman")
    open(path, "wb").write(bytes(blob))
    rng = np.random.default_rng(4)
    try:
        oracle.load_table(path)
        press.use_table(path)
        good = np.cumsum(rng.integers(-11, 12, size=70000)).astype(np.int16)   # zig-zag deltas 0..22
        bad = good.copy()
        bad[40000:] += 100  # one delta of 100: zig-zag 200, no code
        for m in ("shuffman_vbe21_zd", "shuffman_vbbe21_zd"):
            check_read(oracle, m, good)
            assert oracle.press(m, bad)[0] != 0
            assert press.press(m, bad)[0] != 0
            st = press.press_batch_host(m, [good, bad, good[:3000]])
            assert st[1] is None and st[0] == oracle.press(m, good)[1] and st[2] == oracle.press(m, good[:3000])[1]
    finally:
        oracle.load_table()
        press.use_table()


def test_huffman_table_that_never_synchronises(oracle, tmp_path):
    """every code length a multiple of 3, subsequences of 128 bits: a decoder started off a code boundary
    stays off it for ever, so two guesses in three are wrong and no repair round settles more than one
    subsequence per read - the serial walk (k_huf_serial) has to deliver the whole read.  Byte parity with
    the oracle and lossless, single reads and a batch"""
    lens = [3] * 7 + [6] * 7 + [9] * 7 + [12] * 7 + [15] * 7 + [18] * 7 + [21] * 7 + [24] * 8  # Kraft sum 1
    nsym = len(lens)
    code, prev, bits = 0, lens[0], [0] * nsym
    for sy in range(nsym):
        code <<= lens[sy] - prev
        prev = lens[sy]
        bits[sy] = int(format(code, "0%db" % lens[sy])[::-1], 2)
        code += 1
    blob = bytearray(nsym.to_bytes(4, "big") + bytes(4))
    for sy in range(nsym):
        blob += bytes([sy, lens[sy]]) + bits[sy].to_bytes((lens[sy] + 7) // 8, "little")
    path = str(tmp_path / "mult3.huffman")
    open(path, "wb").write(bytes(blob))
    rng = np.random.default_rng(33)
    try:
        oracle.load_table(path)
        press.use_table(path)
        sigs = []
        for n in (2, 3, 50, 5000, 70000, 30011):
            steps = rng.integers(-3, 4, size=n)
            far = rng.random(n) < 0.05
            steps[far] = rng.integers(-28, 29, size=int(far.sum()))  # zig-zag values up to 56: the long codes
            steps[rng.random(n) < 0.002] += 300                      # a few exceptions
            sigs.append(np.cumsum(steps).astype(np.int16))
        sigs = [sig for sig in sigs if shuff_ok("shuffman_vbe21_zd", sig)]
        assert len(sigs) >= 5
        for m in ("shuffman_vbe21_zd", "shuffman_vbbe21_zd"):
            for sig in sigs:
                check_read(oracle, m, sig)
            st = press.press_batch_host(m, sigs)
            assert [x for x in st] == [oracle.press(m, sig)[1] for sig in sigs]
            back = press.depress_batch_host(m, st, [len(sig) for sig in sigs])
            for b, sig in zip(back, sigs):
                assert np.array_equal(b, sig)
    finally:
        oracle.load_table()
        press.use_table()


def test_huffman_batches_repeat_bit_for_bit():
    """the Huffman batch kernels hand out work by tickets and build their repair lists with atomics: whatever the
    order, every run of a batch gives the same streams and the samples back (tools/stress_huff.py, a few batches of
    up to 200 reads, natural and fixed lengths, both exception formats, six runs each)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "stress_huff", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "stress_huff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.stress(5, 200, repeat=4, verbose=False) == 5


def test_huffman_truncated_payload(oracle):
    """a Huffman stream cut short anywhere (tile boundaries included): the decoder delivers what
    the reference's huffman_decode_memory would - it stops when the bytes run out - and never
    writes past the caller's buffer"""
    sig, off = synth.synth_batch(21, 0, 3)
    sig = sig[int(off[0]):int(off[1])][:150000]
    m = "shuffman_vbe21_zd"
    ret, full = oracle.press(m, sig)
    assert ret == 0
    n = sig.size
    for cut in (len(full) - 1, len(full) - 2, len(full) - 4000, 8192 + 600, 8192 * 3 + 9, 700, 20):
        part = full[:cut]
        ro, bo = oracle.depress(m, part, n)
        rg, bg = press.depress(m, part, n)  # canaries checked inside depress()
        assert (rg == 0) == (ro == 0), (cut, rg, ro)
        if ro == 0:
            assert bg.size == bo.size and np.array_equal(bg, bo), (cut, bg.size, bo.size)


def test_huffman_sample_writer_paths(oracle):
    """k_huf_emit writes the samples itself (press_huffman.hip emit_samples): reads built to reach its
    corners - exceptions in front of the first and behind the last one-byte value, runs of more than 64
    exceptions inside one wave's range, reads with more than 64 exceptions, a single one-byte value among
    exceptions, and 4-bit codes throughout (a wave then holds more codes than its staging buffer and
    goes through the one-byte stream's place in memory).  Byte parity and lossless both ways."""
    m = "shuffman_vbe21_zd"
    rng = np.random.default_rng(11)
    reads = []
    base = np.cumsum(rng.integers(-12, 13, size=90000)).astype(np.int64) + 500
    a = base.copy()
    a[1:4] += 3000          # the first samples behind sample 0 are exceptions
    a[-3:] -= 3000          # ... and the last ones
    reads.append(a)
    b = base.copy()
    b[40000:40300:1] += (np.arange(300) % 2) * 900   # 300 exceptions in a row: more than 64 in one wave
    reads.append(b)
    c = base.copy()
    jump = rng.random(c.size) < 0.02                 # ~1800 exceptions all over
    c[jump] += 700
    reads.append(c)
    d = np.array([100, 900, 100, 901, 100, 100, 900, 101], dtype=np.int64)  # little besides exceptions
    reads.append(d)
    for dl in (-2, -1, 1, 2, 0):                     # one of these has a 4-bit code in the NA12878 table
        reads.append(500 + dl * np.arange(70000, dtype=np.int64) % 1500)
    reads.append(np.full(70000, 777, dtype=np.int64))
    for r in reads:
        sig = r.astype(np.int16)
        if shuff_ok(m, sig):
            check_read(oracle, m, sig)
    # and all of them in one batch call
    sigs = [r.astype(np.int16) for r in reads if shuff_ok(m, r.astype(np.int16))]
    streams = press.press_batch_host(m, sigs)
    for sgl, st in zip(sigs, streams):
        ret, want = oracle.press(m, sgl)
        assert ret == 0 and st == want
    backs = press.depress_batch_host(m, streams, [len(x) for x in sigs])
    for sgl, bk in zip(sigs, backs):
        assert bk is not None and np.array_equal(bk, sgl)


@pytest.mark.parametrize("m", ["shuffman_vbe21_zd", "shuffman_vbbe21_zd", "shuffman_vbsse21_zd"])
def test_huffman_batch_of_many_small_reads(oracle, m):
    """four hundred reads of 2 .. 3000 samples (and a few of 40 000) in ONE batch: tiles of a handful of
    subsequences, waves that deliver two values, exceptions at every density up to "every sample" - streams
    equal to the oracle's, samples back exactly"""
    rng = np.random.default_rng(77)
    reads = []
    for i in range(400):
        n = int(rng.integers(2, 3001)) if i % 50 else 40000 + i
        spread = int(rng.choice([1, 3, 20, 127]))
        steps = rng.integers(-spread, spread + 1, size=n)
        pex = float(rng.choice([0.0, 0.001, 0.05, 0.5, 1.0]))
        steps[rng.random(n) < pex] += int(rng.choice([300, -300, 2000]))
        r = np.cumsum(steps).astype(np.int16)
        if shuff_ok(m, r):
            reads.append(r)
    caps = [int(press.bound(m, len(r))) + 8 * len(r) + 1024 for r in reads]  # (the reference's bound is too small
    streams = press.press_batch_host(m, reads, caps=caps)                      # for exception-heavy reads, press.c:2575)
    wants = []
    for r, st, cap in zip(reads, streams, caps):
        ret, want = oracle.press(m, r, cap=cap)
        assert ret == 0 and st == want, (m, len(r), ret, st is None)
        wants.append(want)
    backs = press.depress_batch_host(m, wants, [len(r) for r in reads])
    for r, bk in zip(reads, backs):
        assert bk is not None and np.array_equal(bk, r), (m, len(r))


def test_huffman_batch_mixes_both_decode_ways(oracle):
    """one depress batch in which some reads take k_huf_emit's own sample writer and others (streams cut short:
    their exceptions no longer interleave with what the payload delivers) the two-step way through
    k_low_decode_chunked - every read as the oracle decodes it"""
    m = "shuffman_vbe21_zd"
    sig, off = synth.synth_batch(33, 0, 6)
    reads = [sig[int(off[i]):int(off[i + 1])][:120000] for i in range(6)]
    streams, ns = [], []
    for i, r in enumerate(reads):
        ret, full = oracle.press(m, r)
        assert ret == 0
        if i % 2:  # cut inside the payload: fewer values than the header announces
            full = full[:len(full) - (len(full) // (3 + i))]
        streams.append(full)
        ns.append(len(r))
    backs = press.depress_batch_host(m, streams, ns)
    for st, n, bk in zip(streams, ns, backs):
        ro, bo = oracle.depress(m, st, n)
        assert (bk is not None) == (ro == 0), (n, ro)
        if ro == 0:
            assert bk.size == bo.size and np.array_equal(bk, bo), (n, bk.size, bo.size)


def test_longest_read_in_a_mixed_batch(oracle):
    """a read of NA12878's maximum length (5.7 M samples: 175 chunks, ~420 Huffman tiles - deep
    look-back chains) next to tiny reads in ONE batch call, byte parity with the oracle for the
    chunked kernel families"""
    n_big, first = 5_724_000, 470
    big = synth.synth_read(77, 3, n_big, first)
    rng = np.random.default_rng(3)
    small = [np.cumsum(rng.integers(-20, 21, size=n)).astype(np.int16) for n in (1, 2, 9, 513, 4097)]
    reads = [small[0], big, small[1], small[2], big[:70001], small[3], small[4]]
    for m in ("svb12_zd", "slow5_svb_zd", "hasgam_vbsse21_zdq", "shuffman_vbe21_zd"):
        caps = [int(press.bound(m, len(r))) + 1024 for r in reads]
        streams = press.press_batch_host(m, reads, caps=caps)
        for r, st in zip(reads, streams):
            if not shuff_ok(m, r):
                continue
            ret, want = oracle.press(m, r)
            assert ret == 0 and st == want, (m, len(r))
        ok = [(r, st) for r, st in zip(reads, streams) if st is not None and shuff_ok(m, r)]
        back = press.depress_batch_host(m, [st for _, st in ok], [len(r) for r, _ in ok])
        for (r, _), b in zip(ok, back):
            assert b is not None and np.array_equal(b, r), (m, len(r))


@pytest.mark.parametrize("m", ["shuffman_vbe21_zd", "svb12_zd"])
def test_bench_batch_parity(oracle, m):
    """bench.py's exact batch (seed 20261004, 8192 NA12878-like reads, 0.93 G samples) through press_batch:
    out_len of EVERY read equals the oracle's stream length (oracle on the host's threads), and the bytes of a
    256-read sample that includes the 8 longest reads equal the oracle's; depress_batch gives the samples back."""
    import ctypes
    import sys
    from concurrent.futures import ThreadPoolExecutor

    import torch

    sys.path.insert(0, _libs.ROOT)
    import bench

    dev = torch.device("cuda", 0)
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, 8192, dev, None)
    caps, d_out, d_out_off, d_in_off = b.arena(torch, press, m)
    press.press_batch(m, b.sig, b.d_off, b.d_n, d_out, d_out_off, b.d_len)
    press.depress_batch(m, d_out, d_in_off, b.d_len, b.d_back, b.d_off, b.d_n, b.d_outn)
    torch.cuda.synchronize()
    assert torch.equal(b.d_back, b.sig)
    lens = b.d_len.cpu().numpy()
    host = b.sig.cpu().numpy()
    out_off = d_out_off.cpu().numpy()
    order = np.argsort(-b.n)
    sample = set(int(x) for x in order[:8]) | set(int(x) for x in np.random.default_rng(3).choice(8192, 248, replace=False))
    got_bytes = {}
    dh = d_out.cpu().numpy()
    for r in sample:
        got_bytes[r] = dh[int(out_off[r]): int(out_off[r]) + int(lens[r])].tobytes()
    del dh
    mid = _libs.METHODS[m]
    want_len = np.zeros(8192, dtype=np.int64)
    bad = []

    def work(chunk):
        cap = int(max(oracle.bound(mid, int(b.n[r])) for r in chunk)) + 1024
        out = np.zeros(cap + 64, dtype=np.uint8)
        for r in chunk:
            s = host[int(b.starts[r]): int(b.starts[r]) + int(b.n[r])]
            nout = ctypes.c_uint64(cap)
            ret = oracle._press(mid, s.ctypes.data, s.size, out.ctypes.data, ctypes.byref(nout))
            assert ret == 0
            want_len[r] = nout.value
            if r in sample and out[: nout.value].tobytes() != got_bytes[r]:
                bad.append(r)

    nthr = max(1, min(len(os.sched_getaffinity(0)), 32))
    # longest reads first, dealt out round-robin: the threads finish together
    chunks = [[int(x) for x in order[t::nthr * 8]] for t in range(nthr * 8)]
    with ThreadPoolExecutor(nthr) as ex:
        list(ex.map(work, chunks))
    assert not bad, "stream bytes differ from the oracle's for reads %s" % bad[:8]
    diff = np.nonzero(want_len != lens)[0]
    assert diff.size == 0, "out_len differs from the oracle's for %d reads, first %s" % (diff.size, diff[:8])


@pytest.mark.parametrize("m", ["vbbe21_zd", "vbsbe21_zd", "vbsse21_zd", "hasgam_vbsse21_zdq", "shuffman_vbbe21_zd",
                               "shuffman_vbsse21_zd", "vbe21_zd"])
def test_exception_heavy_sections(oracle, m):
    """sections with hundreds to tens of thousands of exceptions (the whole wave builds and parses them, 64 per
    round): every density, position gaps from 0 to 200 000 samples, values from 256 to 65535 - byte parity with the
    oracle and lossless both ways"""
    rng = np.random.default_rng(len(m) + 11)
    cases = []
    for n, rate, big in ((3000, 0.3, 300), (70000, 0.05, 3000), (70000, 0.9, 20000), (260000, 0.0004, 30000),
                         (1000, 0.065, 100), (129, 0.5, 50), (40000, 0.3, 32000)):
        d = rng.integers(-40, 41, size=n)
        ex = rng.random(n) < rate
        d[ex] = rng.integers(-big, big + 1, size=int(ex.sum()))
        cases.append(np.cumsum(d).astype(np.int16))
    # exactly 64, 65 and 128 exceptions (the rounds' edges)
    for nex in (64, 65, 128, 2):
        d = rng.integers(-20, 21, size=20000)
        at = rng.choice(np.arange(1, 20000), size=nex, replace=False)
        d[at] = 5000
        cases.append(np.cumsum(d).astype(np.int16))
    for sig in cases:
        if not shuff_ok(m, sig):
            continue
        ret, want = oracle.press(m, sig, cap=4 * sig.size + 4096)
        if ret != 0:
            continue  # (outside the reference's domain for this method: e.g. the 16-bit section length)
        check_read(oracle, m, sig, want=want)


def test_huffman_low_entropy_stretches(oracle):
    """a read's low-noise stretches (a nanopore "stall") code every sample with the table's shortest codes: 64 codes per
    256-bit subsequence, 4096 per wave - the emit kernel's staging buffer takes them all (it used to hold 3328 and send
    the rest a slow way).  Byte parity and both decode ways, on reads that are all / partly / not at all low entropy."""
    rng = np.random.default_rng(17)
    lens = oracle.table()
    short = [s for s in range(256) if lens[s][0] == min(l for l, _ in lens)]
    assert short, "the table has a shortest code"
    reads = []
    for n, frac in ((70000, 1.0), (70000, 0.3), (150000, 0.05), (33000, 1.0), (9000, 0.0)):
        d = rng.integers(-30, 31, size=n)
        k = int(n * frac)
        # zig-zag values with the shortest codes only
        z = rng.choice(short, size=k)
        d[:k] = (z >> 1) ^ -(z & 1)
        d[0] = 500
        reads.append(np.cumsum(d).astype(np.int16))
    for sig in reads:
        check_read(oracle, "shuffman_vbe21_zd", sig)
    st = press.press_batch_host("shuffman_vbe21_zd", reads)
    for s, got in zip(reads, st):
        assert got == oracle.press("shuffman_vbe21_zd", s)[1]
    back = press.depress_batch_host("shuffman_vbe21_zd", st, [len(s) for s in reads])
    assert all(b is not None and np.array_equal(b, s) for b, s in zip(back, reads))
