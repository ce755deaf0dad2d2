"""The stall methods rccm_svbbe21_zd, dstall_fz_1500 and dstall_fz (include/press_hip.h, press_hip_stall_*).

Without a GPU: header, symbols and Python mirror; the bound; bad arguments; the workspace figure; the yardstick of
tests/_stall.py against what the REAL reference made of the fixture's reads (tests/golden/ref_stall.json); what the
fixture holds.  On the GPU: the device's streams byte for byte against fixture and yardstick, and back again.
"""
import ctypes
import os
import struct
import time

import numpy as np
import pytest

import _layouts as L
import _libs
import _stall as S
from honours_amd import press

gpu = pytest.mark.gpu
EARG = -2
FAILED64 = (1 << 64) - 1
FAILED32 = (1 << 32) - 1
METHODS = S.STALL_METHODS
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "press_hip.h")
GUARD = 48          # bytes of an empty guard read's slot; words around out_len, stall and out_n
FILL8, FILL16 = 0xA5, 0x5A5A
CANARY = 0x5AC35AC3

_cache = {}


def reads_by_name():
    if "reads" not in _cache:
        _cache["reads"] = dict(S.named_reads())
    return _cache["reads"]


def segment_of(name):
    """the yardstick's first segment of a fixture read, computed once"""
    seg = _cache.setdefault("seg", {})
    if name not in seg:
        seg[name] = S.first_segment(reads_by_name()[name])
    return seg[name]


def want(method, name):
    """the yardstick's (stream or None, (stall_start, stall_len)) of a fixture read, computed once"""
    w = _cache.setdefault("want", {})
    if (method, name) not in w:
        w[(method, name)] = S.expected(method, reads_by_name()[name], segment_of(name))
    return w[(method, name)]


# ------------------------------------------------------------------ without a GPU

@pytest.fixture(scope="module")
def cpu_lib():
    from honours_amd import build
    build.build()
    return press.load_library()


SYMBOLS = ["press_hip_stall_bound", "press_hip_stall_press_batch", "press_hip_stall_depress_batch", "press_hip_stall_workspace_bytes"] + \
          [m + s for m in METHODS for s in ("_bound_16", "_press_16", "_depress_16")]


def test_symbols_header_and_mirror(cpu_lib):
    header = open(HEADER).read()
    for s in SYMBOLS:
        assert hasattr(cpu_lib, s) and s in press.HEADER_SYMBOLS and s + "(" in header, s
    assert press.STALL_METHODS == {"rccm_svbbe21_zd": 0, "dstall_fz_1500": 1, "dstall_fz": 2}
    for name, k in (("PRESS_HIP_STALL_RCCM_SVBBE21_ZD", 0), ("PRESS_HIP_STALL_DSTALL_FZ_1500", 1), ("PRESS_HIP_STALL_DSTALL_FZ", 2)):
        assert "%s = %d" % (name, k) in " ".join(header.split())
    # a family of its own: the method table is what it was
    assert len(press.METHODS) == 19 and "PRESS_HIP_NMETHODS = 19" in " ".join(header.split())
    assert not set(press.STALL_METHODS) & set(press.METHODS)
    for text in ("No segment from jnn", "more than 65535 bytes", "SAMPLE count"):  # the definitions are in the header
        assert text in header, text


def test_bound_is_rccm_vbbe21_zd(cpu_lib, oracle):
    for n in (1, 2, 7, 8, 9, 1000, 7329, 155185, 200000, 5724000):
        b = oracle.bound("rccm_vbbe21_zd", n)
        for m, k in press.STALL_METHODS.items():
            assert press.stall_bound(m, n) == b and cpu_lib.press_hip_stall_bound(k, n) == b
            assert getattr(cpu_lib, m + "_bound_16")(n) == b
    assert cpu_lib.press_hip_stall_bound(-1, 100) == 0 and cpu_lib.press_hip_stall_bound(3, 100) == 0


def test_bad_arguments(cpu_lib):
    """ids outside the family and NULL arguments are PRESS_HIP_EARG before any device call: the same with and without a
    device; nreads = 0 needs no pointer"""
    import torch
    lib = cpu_lib
    a = np.zeros(64, dtype=np.uint64)
    p = a.ctypes.data
    for dr in (0, 1):
        # method sig off n nreads total out out_off out_len stall
        args = [0, p, p, p, 1, 8, p, p, p, p]
        for bad_id in (-1, 3, 19):
            assert lib.press_hip_stall_press_batch(bad_id, *args[1:], dr) == EARG and "stall method" in press.last_error()
        for k in (1, 2, 3, 6, 7, 8):
            bad = list(args)
            bad[k] = None
            assert lib.press_hip_stall_press_batch(*bad, dr) == EARG and "NULL" in press.last_error(), (k, dr)
        # in in_off in_len nreads sig off n total out_n
        dargs = [p, p, p, 1, p, p, p, 8, p]
        for k in (0, 1, 2, 4, 5, 6, 8):
            bad = list(dargs)
            bad[k] = None
            assert lib.press_hip_stall_depress_batch(*bad, dr) == EARG and "NULL" in press.last_error(), (k, dr)
        # an empty batch touches nothing and needs no pointer (without a device: the context's error, not an argument's)
        rc0 = lib.press_hip_stall_press_batch(0, None, None, None, 0, 0, None, None, None, None, dr)
        rc1 = lib.press_hip_stall_depress_batch(None, None, None, 0, None, None, None, 0, None, dr)
        assert (rc0, rc1) == (0, 0) if torch.cuda.is_available() else (rc0 != EARG and rc1 != EARG and rc0 and rc1)
        assert lib.press_hip_stall_press_batch(3, None, None, None, 0, 0, None, None, None, None, dr) == EARG
    assert lib.press_hip_stall_press_batch(0, p + 2, p, p, 1, 8, p, p, p, p, 1) == EARG and "aligned" in press.last_error()
    assert lib.press_hip_stall_depress_batch(p, p, p, 1, p + 2, p, p, 8, p, 1) == EARG and "aligned" in press.last_error()


def test_workspace_is_monotone(cpu_lib):
    ws = press.stall_workspace_bytes
    assert ws(-1, 1000, 10) == 0 and ws(3, 1000, 10) == 0
    for m in METHODS:
        last_t = 0
        for t in (0, 1000, 1 << 20, 930_000_000, 1 << 36):
            last_r = 0
            for r in (1, 2, 64, 300, 8192, 100000):
                v = ws(m, t, r)
                assert v > last_r and v >= ws("rccm_svbbe21_zd", t, r)
                last_r = v
            assert ws(m, t, 64) > last_t
            last_t = ws(m, t, 64)
        # at least what the inner method keeps for the same batch
        assert ws(m, 1 << 20, 64) > press.load_library().press_hip_workspace_bytes(press.METHODS["rccm_vbbe21_zd"], 1 << 20, 64)
    assert ws("dstall_fz", 1 << 20, 64) > ws("rccm_svbbe21_zd", 1 << 20, 64)  # the whole read as a third piece


def test_yardstick_equals_the_reference():
    """every entry of ref_stall.json: jnn's first segment, and for a read with one the reference's three streams - length,
    digest, header fields, first 32 bytes.  The dstall_fz streams of the three real reads total 172 874 bytes
    """
    doc = S.fixture()
    reads = reads_by_name()
    assert len(doc["entries"]) == len(reads) >= 40
    defined = total = 0
    for e in doc["entries"]:
        s = reads[e["name"]]
        assert len(s) == e["n"] and S.sha(s.tobytes()) == e["samples_sha256"], e["name"]
        seg = segment_of(e["name"])
        assert (seg is None) == (e["nseg"] == 0) and (seg is None or list(seg) == e["first"]), e["name"]
        if not e["nseg"]:
            assert "methods" not in e  # the reference's streams are undefined there: none recorded
            continue
        for m in METHODS:
            f = e["methods"][m]
            got, where = want(m, e["name"])
            tag = (e["name"], m)
            if f["exists"]:
                piece = S.submin_stream(s[f["stall_start"]:f["stall_start"] + f["stall_len"]])
                if len(piece) > 65535:
                    # definition 2: the reference wrote a truncated count and cannot read its own stream
                    assert not f["roundtrip"] and len(piece) & 0xFFFF == f["nstall"], tag
                    assert (got is not None and got[0] == 0) if m == "dstall_fz" else got is None, tag
                    continue
            assert got is not None, tag
            defined += 1
            assert len(got) == f["len"] and S.sha(got) == f["sha256"] and got[:32].hex() == f["first32"], tag
            d = S.parse(got)
            assert d["exists"] == f["exists"], tag
            if f["exists"]:
                assert (d["stall_start"], d["stall_len"], d["nstall"]) == (f["stall_start"], f["stall_len"], f["nstall"]), tag
                assert where == (f["stall_start"], f["stall_len"]), tag
            else:
                assert where == (0, 0), tag
            if e["name"].startswith("three_reads/") and m == "dstall_fz":
                total += len(got)
                assert f["roundtrip"]
    assert total == 172874
    assert defined >= 80


def test_fixture_conditions():
    """what makes the fixture worth comparing with"""
    doc = S.fixture()
    ent = {e["name"]: e for e in doc["entries"]}
    three = [e for n, e in ent.items() if n.startswith("three_reads/")]
    assert sorted(tuple(e["first"]) for e in three) == [(1, 798), (1, 3249), (28, 281)]
    assert sum(e["nseg"] == 0 for e in ent.values()) >= 10            # no segment: definition 1
    under = [e for e in ent.values() if e["nseg"] and (e["first"][1] - e["first"][0] + 1) & 0xFFFF < 140]
    assert len(under) >= 3                                            # a first segment under the threshold

    def f(name, m="rccm_svbbe21_zd"):
        return ent["gen/" + name]["methods"][m]

    def seglen(name):
        e = ent["gen/" + name]
        return e["first"][1] - e["first"][0] + 1
    assert [seglen("len-%d" % k) for k in (139, 140, 141, 1499, 1500, 1501)] == [139, 140, 141, 1499, 1500, 1501]
    assert [f("len-%d" % k)["exists"] for k in (139, 140, 141)] == [0, 1, 1]
    assert [f("len-%d" % k, "dstall_fz_1500")["exists"] for k in (1499, 1500, 1501)] == [0, 1, 1]
    assert f("len-140")["stall_len"] == 100 and f("len-1500", "dstall_fz_1500")["stall_len"] == 1460
    assert ent["gen/at-0"]["first"][0] == 0 and f("at-0")["stall_start"] == 20
    e = ent["gen/to-end"]
    assert e["first"][1] == e["n"] - 1 and f("to-end")["exists"] == 1
    e = ent["gen/start-beyond-65535"]                                 # stall_start is truncated
    assert e["first"][0] > 65535 and f("start-beyond-65535")["stall_start"] == (e["first"][0] & 0xFFFF) + 20
    assert seglen("len-beyond-65536") > 65536 + 140                   # stall_len is truncated, and still a stall
    assert f("len-beyond-65536")["stall_len"] == (seglen("len-beyond-65536") & 0xFFFF) - 40
    assert seglen("len-truncated-under-140") > 65536 and seglen("len-truncated-under-140") & 0xFFFF < 140
    assert f("len-truncated-under-140")["exists"] == 0
    reads = reads_by_name()

    def nex(name):
        g = f(name)
        x = reads["gen/" + name][g["stall_start"]:g["stall_start"] + g["stall_len"]].view(np.uint16).astype(np.int64)
        return int((x - x.min() > 255).sum())
    assert nex("stall-exceptions") > 20 and nex("stall-one-exception") == 1 and nex("stall-two-exceptions") == 2
    # dstall_fz: both choices occur among reads that have a stall
    kept = [n for n, e in ent.items() if e["nseg"] and e["methods"]["rccm_svbbe21_zd"]["exists"] and e["methods"]["dstall_fz"]["exists"]]
    dropped = [n for n, e in ent.items() if e["nseg"] and e["methods"]["rccm_svbbe21_zd"]["exists"] and not e["methods"]["dstall_fz"]["exists"]]
    assert len(kept) >= 3 and len(dropped) >= 3 and "gen/smooth-prefers-whole" in dropped
    # definition 2
    g = f("stall-piece-over-65535")
    assert g["exists"] == 1 and not g["roundtrip"] and want("rccm_svbbe21_zd", "gen/stall-piece-over-65535")[0] is None
    fz = want("dstall_fz", "gen/stall-piece-over-65535")
    assert fz[0] is not None and fz[0][0] == 0 and fz[1] == (0, 0)
    if doc["tie"]:
        e = ent["gen/" + doc["tie"]]["methods"]
        assert e["rccm_svbbe21_zd"]["exists"] == 1 and e["dstall_fz"]["exists"] == 0 and e["dstall_fz"]["len"] == e["rccm_svbbe21_zd"]["len"] + 5
    else:
        assert "none found" in doc["source"]


def test_tie_rule():
    """dstall_fz keeps the stall stream only where it is STRICTLY shorter than the bare stream of the whole read"""
    whole = bytes(range(100))
    plain = b"\0" + struct.pack("<I", 100) + whole
    assert S.choose(b"\1" + bytes(98), whole) == (b"\1" + bytes(98), True)
    assert S.choose(b"\1" + bytes(99), whole) == (plain, False)        # equally long: the form without a stall
    assert S.choose(b"\1" + bytes(103), whole) == (plain, False)
    assert S.choose(None, whole) == (plain, False)                     # definition 2


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
    """A batch in a scattered layout; in front of the first read and behind every read an EMPTY guard read with a slot of
    GUARD bytes: it fails, so its slot must keep the arena's fill - guard bytes on either side of every real slot"""

    def __init__(self, reads, caps=None, seed=1):
        import torch
        rng = np.random.default_rng(seed)
        self.reads, self.nr = reads, len(reads)
        sig, off = L.scatter_reads(rng, reads)
        ns, offs = L.with_guards(reads, off)
        ns = np.concatenate([[0], ns]).astype(np.uint32)
        offs = np.concatenate([[0], offs]).astype(np.uint64)
        self.real = np.arange(self.nr) * 2 + 1
        caps = [slot_for(len(r)) for r in reads] if caps is None else caps
        sizes = np.full(len(ns), GUARD, dtype=np.uint64)
        sizes[self.real] = caps
        self.out_off = L.slots(rng, sizes)
        self.sig, self.off, self.n = _t(sig), _t(offs, np.int64), _t(ns, np.int32)
        self.d_out_off = _t(self.out_off, np.int64)
        self.nall = len(ns)
        self.out = torch.full((int(self.out_off[-1]) + 64,), FILL8, dtype=torch.uint8, device="cuda")
        self.out_len = torch.full((self.nall + 2 * GUARD,), CANARY, dtype=torch.int64, device="cuda")
        self.stall = torch.full((2 * self.nall + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")

    def enqueue(self, method, want_stall=True):
        press.stall_press_batch(method, self.sig, self.off, self.n, self.out, self.d_out_off, self.out_len[GUARD:GUARD + self.nall],
                                self.stall[GUARD:GUARD + 2 * self.nall] if want_stall else None)

    def results(self, want_stall=True):
        """-> (streams (None: failed), stall uint32 [nr, 2]); every byte and word outside the results is checked"""
        import torch
        torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        ol = self.out_len.cpu().numpy().view(np.uint64)
        st = self.stall.cpu().numpy().view(np.uint32)
        assert (ol[:GUARD] == CANARY).all() and (ol[GUARD + self.nall:] == CANARY).all(), "out_len"
        assert (st[:GUARD] == CANARY).all() and (st[GUARD + (2 * self.nall if want_stall else 0):] == CANARY).all(), "stall"
        ol = ol[GUARD:GUARD + self.nall]
        st = st[GUARD:GUARD + 2 * self.nall].reshape(-1, 2)
        written = np.zeros(len(out), dtype=bool)
        streams = []
        for k in range(self.nall):
            o, cap = int(self.out_off[k]), int(self.out_off[k + 1] - self.out_off[k])
            if k % 2 == 0:
                assert ol[k] == FAILED64, "an empty read"
                continue
            if ol[k] == FAILED64:
                streams.append(None)
            else:
                assert ol[k] <= cap
                written[o:o + int(ol[k])] = True
                streams.append(out[o:o + int(ol[k])].tobytes())
            if want_stall and ol[k] == FAILED64:
                assert tuple(st[k]) == (0, 0)
        assert (out[~written] == FILL8).all(), "a byte outside the streams was written"
        if want_stall:
            assert not st[0::2].any()
        self.out.fill_(FILL8)
        self.out_len.fill_(CANARY)
        self.stall.fill_(CANARY)
        return streams, st[self.real].copy()

    def run(self, method, want_stall=True):
        self.enqueue(method, want_stall)
        return self.results(want_stall)


class DepressRun:
    def __init__(self, streams, ns, seed=2):
        import torch
        rng = np.random.default_rng(seed)
        self.ns = [int(n) for n in ns]
        self.nr = len(streams)
        arena, in_off, in_len = L.scatter_streams(rng, streams)
        self.off, total = L.scatter_rooms(rng, self.ns, min_gap=8)
        self.total = total
        self.arena, self.in_off, self.in_len = _t(arena), _t(in_off, np.int64), _t(in_len, np.int64)
        self.d_off, self.n = _t(self.off, np.int64), _t(np.array(self.ns, dtype=np.uint32), np.int32)
        self.sig = torch.full((total,), FILL16, dtype=torch.int16, device="cuda")
        self.out_n = torch.full((self.nr + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")

    def enqueue(self):
        press.stall_depress_batch(self.arena, self.in_off, self.in_len, self.sig, self.d_off, self.n, self.out_n[GUARD:GUARD + self.nr])

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

    def run(self):
        self.enqueue()
        return self.results()


def decodable(stream, n):
    """False for a refused read, and for a stream one of whose pieces TurboRC stored raw: nothing tells a decoder so
    (_libs.rc_stored_raw), such a read is outside the reference's lossless domain - tiny reads, in practice"""
    if stream is None:
        return False
    d = S.parse(stream)
    if _libs.rc_stored_raw("rccm_vbbe21_zd", d["rest"], n - d["stall_len"]):
        return False
    return not (d["exists"] and _libs.rc_stored_raw("rccm_vbbe21_zd", d["stall"], d["stall_len"] + 1))


def kept(streams, reads):
    return [k for k, s in enumerate(streams) if decodable(s, len(reads[k]))]


def check_back(streams, reads, seed=3):
    """the device's decoder gives every pressed read back"""
    keep = kept(streams, reads)
    assert len(keep) >= len(streams) // 2
    got = DepressRun([streams[k] for k in keep], [len(reads[k]) for k in keep], seed).run()
    for k, g in zip(keep, got):
        assert g is not None and np.array_equal(g, reads[k]), k


# ------------------------------------------------------------------ on the GPU

@gpu
@pytest.mark.parametrize("method", METHODS)
def test_fixture_reads(lib, method):
    """(1) every read of the fixture in one batch: streams, out_len and stall equal to yardstick and fixture; the decoder
    gives the samples back; the per-read symbols make and read the same streams"""
    names = list(reads_by_name())
    reads = [reads_by_name()[n] for n in names]
    ent = {e["name"]: e for e in S.fixture()["entries"]}
    streams, stall = PressRun(reads, seed=11).run(method)
    total = 0
    for k, name in enumerate(names):
        exp, where = want(method, name)
        assert streams[k] == exp, (name, None if streams[k] is None else len(streams[k]), None if exp is None else len(exp))
        assert tuple(stall[k]) == where, name
        f = ent[name].get("methods", {}).get(method)
        if f and exp is not None and S.sha(exp) == f["sha256"]:
            assert S.sha(streams[k]) == f["sha256"] and len(streams[k]) == f["len"]
            total += len(streams[k]) if name.startswith("three_reads/") else 0
    if method == "dstall_fz":
        assert total == 172874
    assert sum(s is None for s in streams) == (0 if method == "dstall_fz" else 1)  # definition 2's read
    check_back(streams, reads, seed=12)
    small = [k for k in range(len(names)) if len(reads[k]) <= 10000 or names[k].startswith("three_reads/")]
    for k in small + [names.index("gen/stall-piece-over-65535")]:
        ret, one = press.stall_press(method, reads[k], cap=slot_for(len(reads[k])))
        assert (one if ret == 0 else None) == streams[k], names[k]
        if ret == 0 and decodable(one, len(reads[k])):
            ret, back = press.stall_depress(method, one, len(reads[k]))
            assert ret == 0 and np.array_equal(back, reads[k]), names[k]


def ragged_reads():
    """the threshold and truncation reads mixed with tiny reads, and a read without a segment between two stall reads"""
    gen = {n: s for n, s, _ in S.generated_reads()}
    rng = np.random.default_rng(77)
    tiny = {k: L._walk(rng, k) for k in (0, 1, 2, 39, 40, 41)}
    order = ["len-139", 0, "len-140", 1, "len-141", 2, "len-1499", 39, "len-1500", "flat", "len-1501", 40, "start-beyond-65535", 41,
             "len-beyond-65536", "at-0", "len-truncated-under-140", "to-end"]
    out = []
    for k in order:
        out.append(np.full(500, 77, dtype=np.int16) if k == "flat" else tiny[k] if isinstance(k, int) else gen[k])
    return out


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_ragged_batch(lib, method):
    """(2) a piece table that slips by one read shows here"""
    reads = ragged_reads()
    streams, stall = PressRun(reads, seed=21).run(method)
    forms = []
    for k, s in enumerate(reads):
        exp, where = S.expected(method, s)
        assert streams[k] == exp and tuple(stall[k]) == where, k
        forms.append(None if exp is None else exp[0])
    assert forms.count(None) == 1 and forms.count(1) >= 2 and forms.count(0) >= 6
    assert S.first_segment(reads[9]) is None and forms[8:11] == [1, 0, 1]
    check_back(streams, reads, seed=22)


@gpu
def test_slot_capacity(lib):
    """(3) the slot is a hard capacity: one byte too few and the read fails, with nothing written anywhere"""
    gen = {n: s for n, s, _ in S.generated_reads()}
    reads = [gen["len-1500"], gen["len-139"], gen["smooth-prefers-whole"], gen["stall-two-exceptions"]]
    for method in METHODS:
        exp = [S.expected(method, s)[0] for s in reads]
        exact = PressRun(reads, caps=[len(e) for e in exp], seed=31).run(method)
        assert exact[0] == exp
        short = PressRun(reads, caps=[len(e) - (k % 2 == 0) for k, e in enumerate(exp)], seed=32).run(method)
        assert short[0] == [None if k % 2 == 0 else e for k, e in enumerate(exp)]
        none = PressRun(reads, caps=[0, 4, 10, 11], seed=33).run(method)
        assert none[0] == [None] * 4


def damaged(stream, n):
    """one stream with a stall, damaged in every way definition 3 names -> list of (what, bytes)"""
    d = S.parse(stream)
    assert d["exists"] == 1
    b = bytearray(stream)
    out = []
    for v in (2, 255):
        c = bytearray(b)
        c[0] = v
        out.append(("exists = %d" % v, bytes(c)))
    c = bytearray(b)
    struct.pack_into("<H", c, 1, n - d["stall_len"] + 1)
    out.append(("stall beyond the read", bytes(c)))
    c = bytearray(b)
    struct.pack_into("<H", c, 3, 65535)
    out.append(("stall_len beyond the read", bytes(c)))
    c = bytearray(b)
    struct.pack_into("<H", c, 5, 65535)
    out.append(("stall piece beyond in_len", bytes(c)))
    c = bytearray(b)
    struct.pack_into("<I", c, 7 + d["nstall"], len(b))
    out.append(("rest piece beyond in_len", bytes(c)))
    out.append(("cut inside the header", bytes(b[:6])))
    out.append(("cut in front of the rest's count", bytes(b[:7 + d["nstall"] + 2])))
    out.append(("cut inside the rest", bytes(b[:-1])))
    out.append(("one byte", bytes(b[:1])))
    out.append(("no byte", b""))
    c = bytearray(b)
    struct.pack_into("<I", c, 7 + 2, 0x7FFFFFFF)  # the stall piece's exception count
    out.append(("stall piece refused by its decoder", bytes(c)))
    c = bytearray(b)
    struct.pack_into("<I", c, d["rest_at"] + 2, 0x7FFFFFFF)
    out.append(("rest piece refused by its decoder", bytes(c)))
    return out


@gpu
def test_damaged_streams(lib):
    """(4) definition 3: the damaged read is refused, its neighbours decode, nothing outside their rooms is written"""
    gen = {n: s for n, s, _ in S.generated_reads()}
    a, b = gen["len-1501"], gen["stall-two-exceptions"]
    sa, sb = S.expected("rccm_svbbe21_zd", a)[0], S.expected("dstall_fz", b)[0]
    cases = damaged(sa, len(a))
    assert len(cases) >= 13
    streams, ns = [sb], [len(b)]
    for _, c in cases:
        streams += [c, sb]
        ns += [len(a), len(b)]
    got = DepressRun(streams, ns, seed=41).run()
    for k, (what, _) in enumerate(cases):
        assert got[2 * k + 1] is None, what
    for k in range(0, len(got), 2):
        assert got[k] is not None and np.array_equal(got[k], b)
    # and the per-read symbol on the forms whose length its header still tells
    for what, c in cases[:4]:
        ret, back = press.stall_depress("rccm_svbbe21_zd", c + bytes(70000), len(a))
        assert ret != 0 and len(back) == 0, what


@gpu
def test_repeatable_and_independent_of_scratch(lib):
    """(5) nothing depends on what an earlier call left in scratch"""
    import torch
    reads = ragged_reads()
    for method in ("rccm_svbbe21_zd", "dstall_fz"):
        p = PressRun(reads, seed=51)
        first = p.run(method)
        torch.cuda.synchronize()
        press.scratch_fill(0x00)
        second = p.run(method)
        torch.cuda.synchronize()
        press.scratch_fill(0xFF)
        third = p.run(method)
        assert first[0] == second[0] == third[0] and np.array_equal(first[1], second[1]) and np.array_equal(first[1], third[1])
        keep = kept(first[0], reads)
        d = DepressRun([first[0][k] for k in keep], [len(reads[k]) for k in keep], seed=52)
        one = d.run()
        press.scratch_fill(0xA5)
        two = d.run()
        for k, x, y in zip(keep, one, two):
            assert np.array_equal(x, reads[k]) and np.array_equal(y, reads[k])


@gpu
def test_host_form(lib):
    """(6) host pointers: the same streams, stall words and samples as device resident"""
    reads = ragged_reads()
    for method in METHODS:
        dev = PressRun(reads, seed=61).run(method)
        streams, stall = press.stall_press_batch_host(method, reads, caps=[slot_for(len(r)) for r in reads], want_stall=True)
        assert streams == dev[0] and np.array_equal(stall, dev[1])
        assert press.stall_press_batch_host(method, reads, caps=[slot_for(len(r)) for r in reads]) == streams
        keep = kept(streams, reads)
        back = press.stall_depress_batch_host([streams[k] for k in keep], [len(reads[k]) for k in keep])
        for k, g in zip(keep, back):
            assert np.array_equal(g, reads[k])
    bad = press.stall_depress_batch_host([b"\2" + streams[keep[0]][1:], streams[keep[1]]], [len(reads[keep[0]]), len(reads[keep[1]])])
    assert bad[0] is None and np.array_equal(bad[1], reads[keep[1]])
    assert press.stall_press_batch_host("dstall_fz", []) == [] and press.stall_depress_batch_host([], []) == []


@gpu
def test_stream_contract(lib):
    """(7) device resident, on a side stream behind a delay: press and depress return while the delay is pending - they
    only enqueue - and their results are right after synchronising"""
    import torch
    reads = ragged_reads()
    method = "dstall_fz"
    exp = [S.expected(method, s) for s in reads]
    p = PressRun(reads, seed=71)
    keep = kept([e[0] for e in exp], reads)
    d = DepressRun([exp[k][0] for k in keep], [len(reads[k]) for k in keep], seed=72)
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
            p.enqueue(method)  # (scratch reserved: nothing left to allocate)
            d.enqueue()
        s.synchronize()
        p.results()
        d.results()
        e = torch.cuda.Event()
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            e.record(s)
            p.enqueue(method)
            d.enqueue()
        t1 = time.perf_counter()
        assert not e.query(), "a call that promises only to enqueue waited for the stream (or the delay ended early)"
        assert (t1 - t0) * 1e3 < hold_ms / 2
        s.synchronize()
        assert e.query()
        print("stall press + depress: %.3f ms of host time behind a delay of %g ms" % ((t1 - t0) * 1e3, hold_ms))
        streams, stall = p.results()
        assert streams == [x[0] for x in exp] and [tuple(w) for w in stall] == [x[1] for x in exp]
        for k, g in zip(keep, d.results()):
            assert np.array_equal(g, reads[k])
    finally:
        torch.cuda.synchronize()
        press.use_torch_stream()


@gpu
def test_oracle_reads_the_rest_piece(lib, oracle):
    """(8) the rest piece of a device-made stream is a plain rccm_vbbe21_zd stream: the oracle's decoder - and the
    compiled reference's - read it"""
    if not _libs.have_reference():
        pytest.skip("oracle/_ref is not built")
    gen = {n: s for n, s, _ in S.generated_reads()}
    names = ["len-1500", "stall-exceptions", "at-0", "len-139"]
    reads = [gen[n] for n in names]
    streams, stall = PressRun(reads, seed=81).run("rccm_svbbe21_zd")
    for s, st, (ss, sl) in zip(reads, streams, stall):
        d = S.parse(st)
        rest = np.concatenate([s[:ss], s[ss + sl:]])
        for codec in (oracle, _libs.reference()):
            ret, back = codec.depress("rccm_vbbe21_zd", d["rest"], len(rest))
            assert ret == 0 and np.array_equal(back, rest)
