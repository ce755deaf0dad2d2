"""Fitting a static-Huffman table to the user's reads: the device's symbol counts, the reference's tree
construction (huffman.c:373 as gen_huffman runs it) with a length limit, and the table file it writes.

CPU tests: the host builder and writer against the reference's own tables.  GPU tests (marked): the counting
kernel against numpy, and a fitted table through the shuffman_vbe21_zd press / depress."""
import json
import os

import numpy as np
import pytest

import _libs
from honours_amd import press, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FREQ = os.path.join(ROOT, "honours_amd", "data", "NA12878_zd_freq.json")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import torch
    from honours_amd import build
    if torch.cuda.is_available():  # torch initialises the GPU before the library is loaded (as in smoke())
        torch.cuda.set_device(0)
    build.build()
    press.load_library()
    yield


# ---------------------------------------------------------------------------- restatements

def ref_build(counts):
    """calculate_huffman_codes (huffman.c:373): 256 leaves, stable sort ascending, merge the first two into a
    node (zero child = first) at slot 0, slot 1 emptied, stable sort with the empty slots last.
    -> (len[256], bits[256]) with bit k of bits[s] = the k-th branch from the root."""
    nodes = [(int(c), None, None) for c in counts]
    arr = sorted(range(256), key=lambda i: nodes[i][0])
    for _ in range(255):
        a, b = arr[0], arr[1]
        nodes.append((nodes[a][0] + nodes[b][0], a, b))
        arr[0], arr[1] = len(nodes) - 1, None
        arr = sorted(arr, key=lambda i: (1, 0) if i is None else (0, nodes[i][0]))
    ln, bits = [0] * 256, [0] * 256
    st = [(arr[0], 0, 0)]
    while st:
        i, d, b = st.pop()
        if nodes[i][1] is None:
            ln[i], bits[i] = d, b
        else:
            st.append((nodes[i][1], d + 1, b))
            st.append((nodes[i][2], d + 1, b | (1 << d)))
    return ln, bits


def ref_limited(counts, max_bits):
    """the length limit: the reference's tree if it fits, else the tree of max(1, c >> k) for the first k
    (k = 0, 1, ...) that fits"""
    ln, bits = ref_build(counts)
    k = 0
    while max(ln) > max_bits:
        ln, bits = ref_build([max(1, int(c) >> k) for c in counts])
        k += 1
    return ln, bits


def table_bytes(ln, bits, data_bytes):
    """write_code_table (huffman.c:440)"""
    out = bytearray(int(sum(1 for x in ln if x)).to_bytes(4, "big") + (int(data_bytes) & 0xFFFFFFFF).to_bytes(4, "big"))
    for s in range(256):
        if ln[s]:
            out += bytes([s, int(ln[s])]) + int(bits[s]).to_bytes((int(ln[s]) + 7) // 8, "little")
    return bytes(out)


def zd_counts(reads):
    """numpy: counts[257] of the zig-zag deltas zd[1..n) of every read (exceptions in counts[256])"""
    c = np.zeros(press.NBINS, dtype=np.uint64)
    for r in reads:
        r = np.asarray(r, dtype=np.int16)
        if r.size < 2:
            continue
        d = (r[1:].astype(np.uint16) - r[:-1].astype(np.uint16)).astype(np.int16).astype(np.int32)
        z = ((d << 1) ^ (d >> 15)).astype(np.uint16)
        c[:256] += np.bincount(z[z <= 255], minlength=256).astype(np.uint64)
        c[256] += np.uint64(int((z > 255).sum()))
    return c


def scaled(reads, f):
    """the reads with every delta multiplied by f (rounded half away from zero, 16-bit wrap-around): a shifted
    delta distribution - f = 0.5 leaves many values that never occur, f = 1.5 widens the distribution"""
    out = []
    for r in reads:
        d = np.diff(r.astype(np.int64)).astype(np.float64) * f
        h = (np.sign(d) * np.floor(np.abs(d) + 0.5)).astype(np.int64)
        s = np.concatenate([[int(r[0])], int(r[0]) + np.cumsum(h)])
        out.append(s.astype(np.int64).astype(np.uint16).view(np.int16))
    return out


def scaled_batch(nreads, seed, f):
    sig, off = synth.synth_batch(seed, 0, nreads)
    return scaled([sig[int(off[k]):int(off[k + 1])] for k in range(nreads)], f)


def kraft(ln):
    from fractions import Fraction
    return sum(Fraction(1, 1 << int(x)) for x in ln)


# ---------------------------------------------------------------------------- CPU

def test_na12878_table_is_reproduced():
    """gen_huffman's table from its own frequencies, byte for byte (bytes-encoded field = the sum mod 2^32)"""
    freq = json.load(open(FREQ))["freq"]
    ln, bits = press.table_from_counts(freq)
    assert max(ln) <= 24
    want = open(press.TABLE_PATH, "rb").read()
    assert table_bytes(ln, bits, sum(freq)) == want


def test_written_file_equals_na12878(tmp_path):
    freq = json.load(open(FREQ))["freq"]
    ln, bits = press.table_from_counts(freq)
    path = str(tmp_path / "na.huffman")
    press.write_table(path, ln, bits, sum(freq) & 0xFFFFFFFF)
    assert open(path, "rb").read() == open(press.TABLE_PATH, "rb").read()


def test_builder_cases_of_the_reference(tmp_path):
    """ties and zeros: every case of the fixture (the reference's own print_table_freq) byte for byte"""
    fx = json.load(open(os.path.join(GOLD, "huffman_builder_cases.json")))
    assert len(fx["cases"]) >= 8
    for case in fx["cases"]:
        c = case["counts"]
        ln, bits = press.table_from_counts(c, 24)
        path = str(tmp_path / (case["name"] + ".huffman"))
        press.write_table(path, ln, bits, sum(c))
        assert open(path, "rb").read().hex() == case["table_hex"], case["name"]
        # and the restatement agrees with the reference too
        assert table_bytes(*ref_build(c), sum(c)).hex() == case["table_hex"], case["name"]


def _limit_cases():
    freq = json.load(open(FREQ))["freq"]
    rng = np.random.default_rng(3)
    return {
        "halved_batch": [int(x) for x in zd_counts(scaled_batch(16, 7, 0.5))[:256]],
        "geometric": [(1 << (i % 40)) + i for i in range(256)],
        "na12878_tail_zero": [c * 100 if i < 180 else 0 for i, c in enumerate(freq)],
        "sparse": [int(x) if rng.random() < 0.3 else 0 for x in rng.integers(1, 1 << 40, 256)],
    }


@pytest.mark.parametrize("max_bits", [8, 12, 16, 20, 24])
def test_length_limit(max_bits):
    """lengths <= max_bits, a complete prefix code (Kraft sum exactly 1), and the rule as restated here"""
    for name, c in _limit_cases().items():
        ln, bits = press.table_from_counts(c, max_bits)
        assert int(ln.max()) <= max_bits and int(ln.min()) >= 1, name
        assert kraft(ln) == 1, name
        wl, wb = ref_limited(c, max_bits)
        assert [int(x) for x in ln] == wl and [int(x) for x in bits] == wb, (name, max_bits)


def test_length_limit_is_needed():
    """the shifted batch's counts leave values that never occur: the unlimited tree chains them far beyond 24 bits"""
    c = _limit_cases()["halved_batch"]
    assert sum(1 for x in c if x == 0) > 20
    assert max(ref_build(c)[0]) > 24
    ln, _ = press.table_from_counts(c, 24)
    assert int(ln.max()) <= 24


def test_max_bits_range():
    lib = press.load_library()
    press._train_api(lib)
    c = np.ones(256, dtype=np.uint64)
    ln = np.zeros(256, dtype=np.uint32)
    bits = np.zeros(256, dtype=np.uint64)
    for mb in (0, 7, 25, 64):
        assert lib.press_hip_table_from_counts(c.ctypes.data, mb, ln.ctypes.data, bits.ctypes.data) == -2
        assert "max_bits" in press.last_error()
    for mb in (8, 24):
        assert lib.press_hip_table_from_counts(c.ctypes.data, mb, ln.ctypes.data, bits.ctypes.data) == 0
        assert set(ln.tolist()) == {8}
    with pytest.raises(press.PressError):
        press.write_table("/nonexistent-dir/x.huffman", ln, bits, 0)


def test_written_table_loads_everywhere(tmp_path, oracle):
    """a fitted table file: the library's read_code_table + build_symbol_encoder and the oracle's loader give the
    same codes; where the reference is built, its loader takes it and its press equals the oracle's"""
    c = _limit_cases()["halved_batch"]
    ln, bits = press.table_from_counts(c, 24)
    path = str(tmp_path / "fit.huffman")
    press.write_table(path, ln, bits, sum(c))

    import ctypes

    class Code(ctypes.Structure):
        _fields_ = [("numbits", ctypes.c_ulong), ("bits", ctypes.POINTER(ctypes.c_ubyte))]

    t = press.HuffmanTable(path)
    try:
        se = ctypes.cast(t.se, ctypes.POINTER(ctypes.c_void_p * 256)).contents
        for s in range(256):
            code = ctypes.cast(se[s], ctypes.POINTER(Code)).contents
            got = sum(1 << k for k in range(code.numbits) if code.bits[k // 8] & (1 << (k % 8)))
            assert (code.numbits, got) == (int(ln[s]), int(bits[s])), s
    finally:
        t.close()
    reads = scaled_batch(4, 11, 0.5)
    try:
        oracle.load_table(path)
        assert oracle.table() == [(int(ln[s]), int(bits[s])) for s in range(256)]
        if _libs.have_reference():
            ref = _libs.reference()
            ref.load_table(path)
            for r in reads:
                ro, want = oracle.press("shuffman_vbe21_zd", r)
                rr, got = ref.press("shuffman_vbe21_zd", r)
                assert ro == 0 and rr == 0 and got == want
    finally:
        oracle.load_table()
        if _libs.have_reference():
            _libs.reference().load_table()


# ---------------------------------------------------------------------------- GPU

def _count_reads():
    """n in {0, 1, 2, 7, 8, 9}, reads across chunk seams, exception-heavy reads"""
    rng = np.random.default_rng(5)
    reads = []
    for n in (0, 1, 2, 7, 8, 9, 15, 16, 17, 511, 513, 32767, 32768, 32769, 65537, 70001, 100003):
        steps = rng.integers(-40, 41, size=n)
        steps[rng.random(n) < 0.02] *= 300  # exceptions, and 16-bit wrap-around
        reads.append(np.cumsum(steps).astype(np.int64).astype(np.uint16).view(np.int16))
    reads.append(rng.integers(-32768, 32768, size=70000).astype(np.int16))  # every other delta is an exception
    return reads


def _scattered(torch, reads, rng):
    """reads placed in the arena in a shuffled order with gaps of random samples -> device tensors"""
    order = rng.permutation(len(reads))
    off = np.zeros(len(reads), dtype=np.int64)
    pos = 0
    for k in order:
        pos += 8 * int(rng.integers(0, 5))
        off[k] = pos
        pos += (len(reads[k]) + 7) // 8 * 8
    sig = rng.integers(-32768, 32768, size=pos + 64).astype(np.int16)  # gaps hold noise that must not count
    for k, r in enumerate(reads):
        sig[off[k]:off[k] + len(r)] = r
    ns = np.array([len(r) for r in reads], dtype=np.int32)
    return (torch.from_numpy(sig).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(ns).cuda())


@pytest.mark.gpu
def test_device_counts_equal_numpy():
    import torch

    assert torch.cuda.is_available()
    press.use_torch_stream()
    rng = np.random.default_rng(9)
    sig5, off5 = synth.synth_batch(20261004, 0, 512)
    a = _count_reads()
    b = [sig5[int(off5[k]):int(off5[k + 1])] for k in range(512)]
    want_a, want_b = zd_counts(a), zd_counts(b)

    # host form
    assert np.array_equal(press.symbol_counts_host(a), want_a)
    assert np.array_equal(press.symbol_counts_host(b), want_b)
    assert np.array_equal(press.symbol_counts_host(b, counts=want_a), want_a + want_b)

    # device form: two calls accumulate = one call over both
    acc = torch.zeros(press.NBINS, dtype=torch.int64, device="cuda")
    for part in (a, b):
        press.symbol_counts(*_scattered(torch, part, rng), acc)
    one = torch.zeros(press.NBINS, dtype=torch.int64, device="cuda")
    press.symbol_counts(*_scattered(torch, a + b, rng), one)
    torch.cuda.synchronize()
    got = acc.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want_a + want_b)
    assert np.array_equal(one.cpu().numpy().view(np.uint64), want_a + want_b)
    # bit-identical from run to run
    again = torch.zeros(press.NBINS, dtype=torch.int64, device="cuda")
    press.symbol_counts(*_scattered(torch, b, rng), again)
    assert np.array_equal(again.cpu().numpy().view(np.uint64), want_b)

    # counts[256] = the exceptions the existing vbe21_zd press sets aside (u32 nex after the u16 zd[0])
    for part, want in ((a, want_a), (b, want_b)):
        part = [r for r in part if len(r) >= 1]
        streams = press.press_batch_host("vbe21_zd", part, caps=[8 * len(r) + 1024 for r in part])
        assert all(s is not None for s in streams)
        assert sum(int.from_bytes(s[2:6], "little") for s in streams) == int(want[256])


@pytest.mark.gpu
def test_fitted_table_on_shifted_batch(tmp_path, oracle):
    """a table fitted to a batch whose deltas are 1.5 x NA12878-like ones: the device press with it equals the
    oracle's, decodes on the device, and the batch takes at most 0.95 x the bytes it takes with the NA12878 table
    (the counts predict 0.87)"""
    m = "shuffman_vbe21_zd"
    reads = scaled_batch(64, 7, 1.5)
    path = str(tmp_path / "shifted.huffman")
    counts = press.train_table(reads, path)
    assert np.array_equal(counts, zd_counts(reads))
    ln, _ = press.table_from_counts(counts)
    press.load_table()
    base = press.press_batch_host(m, reads)
    assert all(s is not None for s in base)
    try:
        press.use_table(path)
        oracle.load_table(path)
        fitted = press.press_batch_host(m, reads)
        for r, s in zip(reads, fitted):
            ret, want = oracle.press(m, r)
            assert ret == 0 and s == want
        back = press.depress_batch_host(m, fitted, [len(r) for r in reads])
        assert all(np.array_equal(x, r) for x, r in zip(back, reads))
        tot_fit, tot_base = sum(map(len, fitted)), sum(map(len, base))
        assert tot_fit <= 0.95 * tot_base, (tot_fit, tot_base, int(ln.max()))
    finally:
        oracle.load_table()
        press.use_table()


@pytest.mark.gpu
def test_train_table_from_blow5(tmp_path):
    """the BLOW5 path: svb-zd fields decoded and counted on the device; the counts are those of the golden
    samples and the file is table_from_counts of them"""
    import torch

    assert torch.cuda.is_available()
    meta = json.load(open(os.path.join(GOLD, "three_reads.json")))
    sig = np.fromfile(os.path.join(GOLD, "three_reads.i16.bin"), dtype=np.int16)
    reads, o = [], 0
    for r in meta["reads"]:
        reads.append(sig[o:o + r["n"]])
        o += r["n"]
    path = str(tmp_path / "three.huffman")
    counts = press.train_table(os.path.join(GOLD, "three-reads.blow5"), path)
    assert np.array_equal(counts, zd_counts(reads))
    ln, bits = press.table_from_counts(counts)
    assert open(path, "rb").read() == table_bytes(ln, bits, int(counts[:256].sum()))
    # (the file works as a table of the batch API)
    press.use_table(path)
    press.use_table()
