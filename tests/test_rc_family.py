"""The range-coder family (include/press_hip.h, press_hip_rcf_*): the reference's four range coders on its four exception
layouts, sixteen methods, the nibble-CDF coder rccdf among them.

Without a GPU: the two yardsticks of tests/_rcf.py - the restatement of the CDF coder and the splice of oracle streams -
against what the REAL reference made of the fixture's reads (tests/golden/ref_rcf.json); what the fixture holds; header,
symbols and Python mirror; the bound; bad arguments.  On the GPU: the device's streams byte for byte against yardstick
and fixture, and back again.
"""
import ctypes
import os
import time

import numpy as np
import pytest

import _layouts as L
import _rcf as R
from honours_amd import press

gpu = pytest.mark.gpu
EARG = -2
FAILED64 = (1 << 64) - 1
FAILED32 = (1 << 32) - 1
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "press_hip.h")
GUARD = 48
FILL8, FILL16 = 0xA5, 0x5A5A
CANARY = 0x5AC35AC3
PAIRS = [(c, l) for c in R.CODERS for l in R.LAYOUTS]
PUBLIC = {("rc", "vbe21"): "rc_vbe21_zd", ("rcc", "vbe21"): "rcc_vbe21_zd", ("rccm", "vbbe21"): "rccm_vbbe21_zd"}

_cache = {}


def reads_by_name():
    if "reads" not in _cache:
        _cache["reads"] = dict(R.named_reads())
    return _cache["reads"]


def entries():
    return {e["name"]: e for e in R.fixture()["entries"]}


# ------------------------------------------------------------------ without a GPU

@pytest.fixture(scope="module")
def cpu_lib():
    from honours_amd import build
    build.build()
    return press.load_library()


def test_restatement_equals_the_reference():
    """cdf_encode behind the plain layouts' sections reproduces every rccdf_* stream of the fixture, and cdf_decode reads
    every payload back; the fixture's reads are the reads of _rcf.named_reads()"""
    ent = entries()
    assert list(ent) == list(reads_by_name())
    for name, s in reads_by_name().items():
        e = ent[name]
        assert e["n"] == len(s) and e["samples_sha256"] == R.sha(s.tobytes()), name
        low = R.split("vbe21", s)[1]
        payload, _, raw, _ = R._cdf(low)
        if not raw:
            assert R.cdf_decode(payload, len(low)) == low, name
        for l in R.LAYOUTS:
            f = e["methods"][R.name("rccdf", l)]
            got = R.expected("rccdf", l, s)
            assert (len(got), R.sha(got), got[:32].hex()) == (f["len"], f["sha256"], f["first32"]), (name, l)
            # what the reference's own decoder makes of it: a stored payload does not come back, every other does
            assert f["roundtrip"] == (not raw), (name, l)


def test_splice_equals_the_reference():
    """sec(L) + tail(C) reproduces every entry of the twelve methods of the three older coders"""
    ent = entries()
    for name, s in reads_by_name().items():
        for c in ("rc", "rcc", "rccm"):
            for l in R.LAYOUTS:
                f = ent[name]["methods"][R.name(c, l)]
                got = R.expected(c, l, s)
                assert (len(got), R.sha(got), got[:32].hex()) == (f["len"], f["sha256"], f["first32"]), (name, c, l)
                if (c, l) in PUBLIC:
                    assert got == R._press(PUBLIC[(c, l)], s)


def test_fixture_conditions():
    """what the fixture is meant to hold: a carry, the give-up reads, reads of at most ten samples always stored, and on
    the three real reads the bytes the issue quotes"""
    reads = reads_by_name()
    carries = {n: R._cdf(R.split("vbe21", s)[1])[1] for n, s in reads.items()}
    assert max(carries.values()) >= 1, carries
    for n, s in reads.items():
        low = R.split("vbe21", s)[1]
        raw = R._cdf(low)[2]
        assert raw == R.gave_up("rccdf", s), n
        if 2 <= len(s) <= 10:
            assert raw and len(low) <= 9, n
    assert all(R.gave_up(c, reads["uniform-2000"]) for c in R.CODERS)
    nex = len(reads["uniform-2000"]) - 1 - len(R.split("vbe21", reads["uniform-2000"])[1])
    assert 0.10 * 2000 <= nex <= 0.18 * 2000, nex
    nex = len(reads["sparse-5000"]) - 1 - len(R.split("vbe21", reads["sparse-5000"])[1])
    assert 50 <= nex <= 100, nex
    assert not any(R.gave_up(c, reads["constant-3000"]) for c in R.CODERS)
    real = [s for n, s in reads.items() if n.startswith("three_reads/")]
    assert sum(len(R.expected("rccdf", "vbe21", s)) for s in real) == 176884
    assert sum(len(R.expected("rc", "vbe21", s)) for s in real) == 176628
    flushes = {R._cdf(R.split("vbe21", s)[1])[3] for s in reads.values()}
    assert 0 in flushes and flushes & {1, 2}, flushes  # stored reads and flushed ones


SYMBOLS = ["press_hip_rcf_bound", "press_hip_rcf_press_batch", "press_hip_rcf_depress_batch"] + \
          [R.name(c, l) + s for c, l in PAIRS if (c, l) not in PUBLIC for s in ("_bound_16", "_press_16", "_depress_16")]


def test_symbols_header_and_mirror(cpu_lib):
    header = open(HEADER).read()
    assert len(SYMBOLS) == 3 + 39
    for s in SYMBOLS:
        assert hasattr(cpu_lib, s) and s in press.HEADER_SYMBOLS and s + "(" in header, s
    assert press.RCF_CODERS == {"rc": 0, "rcc": 1, "rccm": 2, "rccdf": 3}
    assert press.RCF_LAYOUTS == {"vbe21": 0, "vbbe21": 1, "vbsbe21": 2, "vbsse21": 3}
    flat = " ".join(header.split())
    for k, c in enumerate(("RC", "RCC", "RCCM", "RCCDF")):
        assert "PRESS_HIP_RCF_%s = %d" % (c, k) in flat
    for k, l in enumerate(("VBE21", "VBBE21", "VBSBE21", "VBSSE21")):
        assert "PRESS_HIP_RCF_%s = %d" % (l, k) in flat
    assert "PRESS_HIP_NRCF_CODERS = 4" in flat and "PRESS_HIP_NRCF_LAYOUTS = 4" in flat
    # a family of its own: the method table is what it was
    assert len(press.METHODS) == 19 and "PRESS_HIP_NMETHODS = 19" in flat
    for words in ("WITHOUT __AVX2__", "does NOT come back", "raw[r] = 1", "do not learn them"):
        assert words in header, words
    from honours_amd import build
    assert build.SOURCES[-1] == "press_cdf.hip"


def test_bound_is_the_plain_layouts(cpu_lib, oracle):
    for c, l in PAIRS:
        for n in (1, 2, 7, 8, 9, 1000, 7329, 155185, 5724000):
            b = oracle.bound(l + "_zd", n)
            assert press.rcf_bound(c, l, n) == b and cpu_lib.press_hip_rcf_bound(press.RCF_CODERS[c], press.RCF_LAYOUTS[l], n) == b
            assert getattr(cpu_lib, R.name(c, l) + "_bound_16")(n) == b
    assert press.rcf_bound("rccdf", "vbe21", 7329) == 14659
    for bad in (-1, 4, 1000):
        assert cpu_lib.press_hip_rcf_bound(bad, 0, 100) == 0 and cpu_lib.press_hip_rcf_bound(0, bad, 100) == 0


def test_bad_arguments(cpu_lib):
    """bad coder or layout ids and NULL arguments are PRESS_HIP_EARG before any device call: the same with and without a
    device"""
    lib = cpu_lib
    a = np.zeros(64, dtype=np.uint64)
    p = a.ctypes.data
    for form in (0, 1):
        for bad in (-1, 4, 1000):
            for c, l in ((bad, 0), (0, bad), (bad, bad)):
                assert lib.press_hip_rcf_press_batch(c, l, p, p, p, 1, 8, p, p, p, None, form) == EARG
                assert "coder" in press.last_error()
                assert lib.press_hip_rcf_depress_batch(c, l, p, p, p, 1, p, p, p, 8, p, form) == EARG
                assert lib.press_hip_rcf_press_batch(c, l, p, p, p, 0, 0, p, p, p, None, form) == EARG  # (an empty batch too)
        for k in range(6):
            args = [p] * 6
            args[k] = None
            assert lib.press_hip_rcf_press_batch(3, 0, args[0], args[1], args[2], 1, 8, args[3], args[4], args[5], None, form) == EARG
        for k in range(7):
            args = [p] * 7
            args[k] = None
            assert lib.press_hip_rcf_depress_batch(3, 0, args[0], args[1], args[2], 1, args[3], args[4], args[5], 8, args[6], form) == EARG
    assert lib.press_hip_rcf_press_batch(3, 0, p + 2, p, p, 1, 8, p, p, p, None, 1) == EARG  # a device arena off 16 bytes


# ------------------------------------------------------------------ GPU plumbing

@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.use_torch_stream()
    yield lb
    torch.cuda.synchronize()
    press.use_torch_stream()
    torch.cuda.empty_cache()


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


def slot_for(n):
    return 8 * n + 4096 if n else 32


class PressRun:
    """A batch in a scattered layout, the slots back to back from an odd offset; canaries in front of and behind out_len
    and raw, and every byte of the arena outside the streams and the slots of failed reads must keep its fill"""

    def __init__(self, reads, caps=None, seed=1):
        import torch
        rng = np.random.default_rng(seed)
        self.reads, self.nr = reads, len(reads)
        sig, off = L.scatter_reads(rng, reads)
        caps = [slot_for(len(r)) for r in reads] if caps is None else caps
        self.out_off = L.slots(rng, np.asarray(caps, dtype=np.uint64))
        self.sig, self.off = _t(sig), _t(off.astype(np.uint64), np.int64)
        self.n = _t(np.array([len(r) for r in reads], dtype=np.uint32), np.int32)
        self.d_out_off = _t(self.out_off, np.int64)
        self.out = torch.full((int(self.out_off[-1]) + 64,), FILL8, dtype=torch.uint8, device="cuda")
        self.out_len = torch.full((self.nr + 2 * GUARD,), CANARY, dtype=torch.int64, device="cuda")
        self.raw = torch.full((self.nr + 2 * GUARD,), FILL8, dtype=torch.uint8, device="cuda")

    def enqueue(self, coder, layout, want_raw=True):
        press.rcf_press_batch(coder, layout, self.sig, self.off, self.n, self.out, self.d_out_off, self.out_len[GUARD:GUARD + self.nr],
                              self.raw[GUARD:GUARD + self.nr] if want_raw else None)

    def generic(self, method):
        press.press_batch(method, self.sig, self.off, self.n, self.out, self.d_out_off, self.out_len[GUARD:GUARD + self.nr])

    def results(self, want_raw=True):
        """-> (streams (None: failed), raw uint8 [nr])"""
        import torch
        torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        ol = self.out_len.cpu().numpy().view(np.uint64)
        rw = self.raw.cpu().numpy()
        assert (ol[:GUARD] == CANARY).all() and (ol[GUARD + self.nr:] == CANARY).all(), "out_len"
        assert (rw[:GUARD] == FILL8).all() and (rw[GUARD + (self.nr if want_raw else 0):] == FILL8).all(), "raw"
        ol, rw = ol[GUARD:GUARD + self.nr], rw[GUARD:GUARD + self.nr]
        written = np.zeros(len(out), dtype=bool)
        streams = []
        for k in range(self.nr):
            o, cap = int(self.out_off[k]), int(self.out_off[k + 1] - self.out_off[k])
            if ol[k] == FAILED64:
                streams.append(None)
                assert not want_raw or rw[k] == 0
                written[o:o + cap] = True  # (a read that fails may leave its own slot in any state, as the generic calls do)
            else:
                assert ol[k] <= cap
                written[o:o + int(ol[k])] = True
                streams.append(out[o:o + int(ol[k])].tobytes())
        assert (out[~written] == FILL8).all(), "a byte outside the streams was written"
        self.out.fill_(FILL8)
        self.out_len.fill_(CANARY)
        self.raw.fill_(FILL8)
        return streams, rw.copy()

    def run(self, coder, layout, want_raw=True):
        self.enqueue(coder, layout, want_raw)
        return self.results(want_raw)


class DepressRun:
    def __init__(self, streams, ns, seed=2):
        import torch
        rng = np.random.default_rng(seed)
        self.ns = [int(n) for n in ns]
        self.nr = len(streams)
        arena, in_off, in_len = L.scatter_streams(rng, streams)
        self.off, self.total = L.scatter_rooms(rng, self.ns, min_gap=8)
        self.arena, self.in_off, self.in_len = _t(arena), _t(in_off, np.int64), _t(in_len, np.int64)
        self.d_off, self.n = _t(self.off, np.int64), _t(np.array(self.ns, dtype=np.uint32), np.int32)
        self.sig = torch.full((self.total,), FILL16, dtype=torch.int16, device="cuda")
        self.out_n = torch.full((self.nr + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")

    def enqueue(self, coder, layout):
        press.rcf_depress_batch(coder, layout, self.arena, self.in_off, self.in_len, self.sig, self.d_off, self.n,
                                self.out_n[GUARD:GUARD + self.nr])

    def results(self):
        """-> samples per read (None: refused); nothing outside the rooms of the decoded reads is written"""
        import torch
        torch.cuda.synchronize()
        sig = self.sig.cpu().numpy()
        on = self.out_n.cpu().numpy().view(np.uint32)
        assert (on[:GUARD] == CANARY).all() and (on[GUARD + self.nr:] == CANARY).all(), "out_n"
        on = on[GUARD:GUARD + self.nr]
        got, spans = [], []
        for k in range(self.nr):
            o = int(self.off[k])
            if on[k] == FAILED32:
                got.append(None)
                spans.append(0)
            else:
                assert on[k] == self.ns[k]
                got.append(sig[o:o + self.ns[k]].copy())
                spans.append(self.ns[k])
        assert (sig[L.outside_rooms(self.total, self.off, spans)] == FILL16).all(), "a sample outside the decoded reads was written"
        self.sig.fill_(FILL16)
        self.out_n.fill_(CANARY)
        return got

    def run(self, coder, layout):
        self.enqueue(coder, layout)
        return self.results()


def decoded(oracle, coder, layout, s, stream):
    """what a decoder must make of `stream`, a stream of the read s whose section is intact: the read itself where the
    payload is a coded one; rccdf, any payload: the section with what cdf_decode reads out of the payload, through the
    oracle's decoder of the plain layout; else None (a stored payload under one of the three older coders: some n
    samples)"""
    sec, low = R.split(layout, s)
    payload = stream[len(sec):]
    if stream == R.expected(coder, layout, s) and not R.gave_up(coder, s):
        return s  # (rccdf: test_restatement_equals_the_reference has cdf_decode read such payloads back)
    if coder != "rccdf":
        return None
    ret, back = oracle.depress(layout + "_zd", sec + R.cdf_decode(payload, len(low)), len(s))
    assert ret == 0
    return back


def check_batch(oracle, coder, layout, reads, seed, dec_seed=None):
    """press: streams equal to the yardstick, raw equal to the definition; depress: the device reads them back"""
    streams, raw = PressRun(reads, seed=seed).run(coder, layout)
    for k, s in enumerate(reads):
        if len(s) == 0:
            assert streams[k] is None and raw[k] == 0, k
            continue
        assert streams[k] == R.expected(coder, layout, s), (coder, layout, k, len(s))
        assert raw[k] == R.gave_up(coder, s), (coder, layout, k, len(s))
    keep = [k for k, s in enumerate(reads) if len(s)]
    got = DepressRun([streams[k] for k in keep], [len(reads[k]) for k in keep], seed=dec_seed or seed + 1).run(coder, layout)
    for k, g in zip(keep, got):
        assert g is not None and len(g) == len(reads[k]), k
        want = decoded(oracle, coder, layout, reads[k], streams[k])
        assert want is None or np.array_equal(g, want), (coder, layout, k, len(reads[k]))
    return streams, raw


# ------------------------------------------------------------------ on the GPU

@gpu
@pytest.mark.parametrize("coder", R.CODERS)
def test_fixture_reads(lib, oracle, coder):
    """every layout under the coder on all fixture reads in one batch: stream bytes against restatement or splice, sha256
    against the fixture, raw against the give-up flag, and the device's decoder on those streams"""
    names = list(reads_by_name())
    reads = [reads_by_name()[n] for n in names]
    ent = entries()
    for layout in R.LAYOUTS:
        streams, raw = check_batch(oracle, coder, layout, reads, seed=11)
        for k, name in enumerate(names):
            f = ent[name]["methods"][R.name(coder, layout)]
            assert R.sha(streams[k]) == f["sha256"] and len(streams[k]) == f["len"], (name, layout)
        assert raw[names.index("uniform-2000")] == 1 and raw[names.index("constant-3000")] == 0
        if coder == "rccdf":
            for k, name in enumerate(names):
                assert raw[k] == R._cdf(R.split("vbe21", reads[k])[1])[2], name


def ragged_reads(count, seed, longest_at=None):
    """reads of 0 .. 3000 samples, some with exceptions; longest_at: where the one read of 3000 samples stands"""
    rng = np.random.default_rng(seed)
    ns = [int(x) for x in rng.integers(0, 2900, size=count)]
    if count > 100:  # (the yardstick is Python: most reads of a large batch are short)
        ns = [n if k % 25 == 0 else n % 300 for k, n in enumerate(ns)]
    if longest_at is not None:
        ns[longest_at] = 3000
    return [R.signal(seed * 1000 + k, n, exr=0.01 if k % 3 == 0 else 0.0) if n else np.zeros(0, dtype=np.int16) for k, n in enumerate(ns)]


@gpu
def test_identity_with_the_generic_methods(lib):
    """the three pairs that are public methods: press_hip_rcf_press_batch and press_hip_press_batch write the same bytes"""
    reads = ragged_reads(64, 5, longest_at=40)
    for (c, l), m in PUBLIC.items():
        p = PressRun(reads, seed=21)
        fam = p.run(c, l)[0]
        p.generic(m)
        gen = p.results(want_raw=False)[0]
        assert fam == gen and sum(s is not None for s in fam) >= 60, m


def edge_reads():
    """-> dict name -> read: where k_cdf_encode / k_cdf_decode can go wrong"""
    out = {}
    for nlow in (0, 1, 8, 9, 10, 11):  # the give-up edge: up to nine one-byte values are always stored
        out["nlow-%d" % nlow] = R.signal(300 + nlow, nlow + 1)
    out["one-byte-5000"] = R.from_low(bytes([6]) * 5000, base=-9000)          # a saturated table
    out["every-byte"] = R.from_low(bytes(range(256)) * 3, base=500)
    out["0f-f0"] = R.from_low(bytes([0x0F, 0xF0]) * 250, base=-14000)
    out["carry-in-first-word"] = R.from_low(R.carry_read(), base=0)
    return out


@gpu
def test_cdf_edges(lib, oracle):
    """the give-up edge, a saturated table, every byte value, alternating nibbles, a one-word and a two-word flush, a carry
    inside the first output word, and payloads that start on each of the four byte phases of a 32-bit word.

    A carry that ripples across a whole 0xFFFFFFFF word cannot be provoked (chance 2^-32 per carry): the walk back over
    more than one word is the loop of the three older coders' kernels, and is not faked here."""
    ed = edge_reads()
    for nlow in (0, 1, 8, 9, 10, 11):
        low = R.split("vbe21", ed["nlow-%d" % nlow])[1]
        assert len(low) == nlow
        if nlow <= 9:
            assert R._cdf(low)[2] == (nlow >= 1)  # no byte: a flush of 4 bytes; 1 .. 9 bytes: always stored
    assert len(R._cdf(b"")[0]) == 4
    assert R.split("vbe21", ed["one-byte-5000"])[1] == bytes([6]) * 5000
    assert R.split("vbe21", ed["every-byte"])[1] == bytes(range(256)) * 3
    assert R.split("vbe21", ed["0f-f0"])[1] == bytes([0x0F, 0xF0]) * 250
    trace = []
    R.cdf_encode(R.carry_read(), trace)
    assert 4 in trace, trace
    reads = list(ed.values()) + [R.exact_exceptions(400 + k, 300, k) for k in range(9)]
    flushes, phases = set(), set()
    for s in reads:
        flushes.add(R._cdf(R.split("vbe21", s)[1])[3])
        phases |= {len(R.split(l, s)[0]) % 4 for l in R.LAYOUTS}
    assert {1, 2} <= flushes and phases == {0, 1, 2, 3}, (flushes, phases)
    for layout in R.LAYOUTS:
        check_batch(oracle, "rccdf", layout, reads, seed=31)


@gpu
@pytest.mark.parametrize("count", [1, 3, 4, 5, 63, 64, 65, 300])
def test_cdf_batches(lib, oracle, count):
    """four reads per wave and a ticket: batches that leave groups empty and tails ragged, reads of 0 to 3000 samples, the
    longest read not first"""
    reads = ragged_reads(count, 40 + count, longest_at=count // 2 if count > 1 else None)
    check_batch(oracle, "rccdf", "vbe21" if count % 2 else "vbbe21", reads, seed=41)


@gpu
@pytest.mark.parametrize("coder", R.CODERS)
def test_exception_heavy_reads(lib, oracle, coder):
    """0.04 %, 10 % and 90 % exceptions, and 64, 65 and 128 of them, on every layout against splice or restatement (the
    reference cannot run these; the oracle can)"""
    reads = [R.signal(51, 2500, exr=0.0004), R.signal(52, 1500, exr=0.10), R.signal(53, 600, exr=0.90),
             R.exact_exceptions(54, 900, 64), R.exact_exceptions(55, 900, 65), R.exact_exceptions(56, 900, 128)]
    nex = [len(s) - 1 - len(R.split("vbe21", s)[1]) for s in reads]
    assert nex[0] >= 1 and nex[3:] == [64, 65, 128] and nex[2] > 500, nex
    for layout in R.LAYOUTS:
        check_batch(oracle, coder, layout, reads, seed=51)


@gpu
def test_slot_capacity(lib):
    """the slot is a hard capacity: one byte too few and that read fails, its neighbours and every byte outside the
    streams stay; raw = NULL is accepted"""
    reads = [R.signal(61, 700), R.signal(62, 12), R.signal(63, 2000, exr=0.14, spread=127), R.signal(64, 900, exr=0.02)]
    for c, l in (("rccdf", "vbe21"), ("rccdf", "vbsse21"), ("rc", "vbbe21"), ("rccm", "vbe21")):
        exp = [R.expected(c, l, s) for s in reads]
        assert PressRun(reads, caps=[len(e) for e in exp], seed=61).run(c, l)[0] == exp
        short = PressRun(reads, caps=[len(e) - (k % 2 == 0) for k, e in enumerate(exp)], seed=62).run(c, l, want_raw=False)
        assert short[0] == [None if k % 2 == 0 else e for k, e in enumerate(exp)]
        assert PressRun(reads, caps=[0, 4, 5, 7], seed=63).run(c, l)[0] == [None] * 4


@gpu
def test_decoder_safety(lib, oracle):
    """a stream cut at every length from 0 to 16 bytes, and a payload of 0xFF: the decoder reads zeros behind the end of
    the stream, gives what the restatement gives, and writes nothing outside the read's room"""
    s = R.signal(71, 200)
    full = R.expected("rccdf", "vbe21", s)
    sec = R.split("vbe21", s)[0]
    assert len(sec) == 6 and len(full) > 16
    cuts = [full[:k] for k in range(17)] + [sec + b"\xff" * 150, sec + b"\xff" * 3, full]
    streams, ns = [], []
    for c in cuts:
        streams += [c, full]
        ns += [len(s), len(s)]
    got = DepressRun(streams, ns, seed=71).run("rccdf", "vbe21")
    for k, c in enumerate(cuts):
        assert np.array_equal(got[2 * k + 1], s)
        g = got[2 * k]
        if len(c) >= len(sec):
            assert g is not None and np.array_equal(g, decoded(oracle, "rccdf", "vbe21", s, c)), k
        else:
            assert g is None or len(g) == len(s)
    # the three older coders on the same cuts: something of the right length or a refusal, nothing outside the rooms
    for c, l in (("rc", "vbe21"), ("rcc", "vbsbe21"), ("rccm", "vbe21")):
        full = R.expected(c, l, s)
        got = DepressRun([full[:k] for k in range(17)] + [full], [len(s)] * 18, seed=72).run(c, l)
        assert np.array_equal(got[-1], s) and all(g is None or len(g) == len(s) for g in got)


@gpu
def test_repeatable_and_independent_of_scratch(lib, oracle):
    """the call run twice, and after the scratch was filled with 0xA5, gives identical bytes"""
    import torch
    reads = ragged_reads(37, 8, longest_at=20)
    for c, l in (("rccdf", "vbe21"), ("rccdf", "vbsbe21"), ("rcc", "vbsse21")):
        p = PressRun(reads, seed=81)
        first = p.run(c, l)
        second = p.run(c, l)
        torch.cuda.synchronize()
        press.scratch_fill(0xA5)
        third = p.run(c, l)
        assert first[0] == second[0] == third[0] and np.array_equal(first[1], second[1]) and np.array_equal(first[1], third[1])
        keep = [k for k, s in enumerate(reads) if len(s)]
        d = DepressRun([first[0][k] for k in keep], [len(reads[k]) for k in keep], seed=82)
        one = d.run(c, l)
        press.scratch_fill(0xA5)
        two = d.run(c, l)
        for x, y in zip(one, two):
            assert x is not None and np.array_equal(x, y)


@gpu
def test_host_forms(lib, oracle):
    """host pointers: the same streams, raw and samples as device resident"""
    reads = ragged_reads(19, 9, longest_at=7)
    caps = [slot_for(len(r)) for r in reads]
    for c, l in (("rccdf", "vbe21"), ("rccdf", "vbbe21"), ("rc", "vbsse21"), ("rccm", "vbsbe21")):
        dev = PressRun(reads, seed=91).run(c, l)
        streams, raw = press.rcf_press_batch_host(c, l, reads, caps=caps, want_raw=True)
        assert streams == dev[0] and np.array_equal(raw, dev[1])
        assert press.rcf_press_batch_host(c, l, reads, caps=caps) == streams
        keep = [k for k, s in enumerate(streams) if s is not None and not raw[k]]
        back = press.rcf_depress_batch_host(c, l, [streams[k] for k in keep], [len(reads[k]) for k in keep])
        for k, g in zip(keep, back):
            assert np.array_equal(g, reads[k]), k
    assert press.rcf_press_batch_host("rccdf", "vbe21", []) == [] and press.rcf_depress_batch_host("rccdf", "vbe21", [], []) == []


@gpu
@pytest.mark.parametrize("coder", R.CODERS)
def test_per_read_symbols(lib, coder):
    """X_press_16 and X_depress_16 of every pair on the three real reads: the yardstick's stream, and the read back"""
    for name, s in R.real_reads():
        for l in R.LAYOUTS:
            ret, one = press.rcf_press(coder, l, s)
            assert ret == 0 and one == R.expected(coder, l, s), (name, coder, l)
            ret, back = press.rcf_depress(coder, l, one, len(s))
            assert ret == 0 and np.array_equal(back, s), (name, coder, l)


@gpu
def test_stream_contract(lib, oracle):
    """device resident, on a side stream behind a delay of 50 ms: press and depress return while the delay is pending -
    they only enqueue - and their results are right after synchronising"""
    import torch
    reads = [s for s in ragged_reads(24, 10, longest_at=3) if len(s) > 40]
    c, l = "rccdf", "vbe21"
    exp = [R.expected(c, l, s) for s in reads]
    p = PressRun(reads, seed=101)
    d = DepressRun(exp, [len(s) for s in reads], seed=102)
    torch.cuda._sleep(100000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(20000000)
    b.record()
    b.synchronize()
    hold_ms = 50.0
    cycles = int(hold_ms * 20000000 / a.elapsed_time(b))
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0 and lib.press_hip_set_stream(ctypes.c_void_p(s.cuda_stream)) == 0
    try:
        with torch.cuda.stream(s):
            p.enqueue(c, l)  # (scratch reserved: nothing left to allocate)
            d.enqueue(c, l)
        s.synchronize()
        p.results()
        d.results()
        e = torch.cuda.Event()
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            e.record(s)
            p.enqueue(c, l)
            d.enqueue(c, l)
        t1 = time.perf_counter()
        assert not e.query(), "a call that promises only to enqueue waited for the stream (or the delay ended early)"
        assert (t1 - t0) * 1e3 < hold_ms / 2
        s.synchronize()
        assert e.query()
        print("rcf press + depress: %.3f ms of host time behind a delay of %g ms" % ((t1 - t0) * 1e3, hold_ms))
        assert p.results()[0] == exp
        for g, r in zip(d.results(), reads):
            assert np.array_equal(g, r)
    finally:
        torch.cuda.synchronize()
        press.use_torch_stream()
