"""The host-pointer form of a batch call delivers what its device-resident form delivers.

The two forms are one computation behind different plumbing (press_staging.hip), so this module is differential: every
call runs once device resident and then with host pointers, on pageable buffers and on press_hip_host_alloc buffers, and
the host results must equal the device's - out_len / out_n / need / stats / q / counts as arrays, the bytes, samples,
floats and rows inside what was delivered - with the caller's fill untouched outside it.  The frames of the zstd kinds are
not pinned byte for byte: where two frames differ their lengths and their content must not.
What the device form computes is the business of the oracle tests; nothing here reads the oracle.

The shapes are the smallest that reach every branch of the staging unit:
  direct3   3 reads: the per-read copies of nreads <= 4
  staged6   6 reads of 200 .. 2000 samples in scattered order: the gathered / staged path under the direct-copy limit
  big6      5 reads of 1.8 M smooth samples and an empty one, in room order (svb12_zd; press_batch, press_packed and
            depress_pa_batch only): 18 MB of samples go up through the staging buffers, the packed arena is far above
            the 256-KiB direct limit, and the float arena of 36 MB crosses the 32-MiB staging boundary inside the last read
The 6-read shapes hold an empty read and, for the decoders, a stream cut to 3 bytes - shorter than any header or key
block, so it is refused: FAILED / UINT32_MAX entries go through the piece lists.
"""
import ctypes

import numpy as np
import pytest

import _layouts as L
from honours_amd import press, synth

pytestmark = pytest.mark.gpu

METHODS = ("svb12_zd", "vbbe21_zd", "zstd_svb_zd")  # one per family
RECODE_TO = {"svb12_zd": "vbbe21_zd", "vbbe21_zd": "zstd_svb_zd", "zstd_svb_zd": "svb12_zd"}
SMALL = ("direct3", "staged6")
LENS = {"direct3": [200, 1501, 777], "staged6": [2000, 333, 0, 1999, 200, 1024], "big6": [1_800_000] * 2 + [0] + [1_800_000] * 3}
CUT = 1          # the read of a 6-read shape whose stream is cut ...
CUT_BYTES = 3    # ... to this
F64, F32 = L.FAILED64, L.FAILED32
CANARY = 256
HOST_KINDS = ("pageable", "pinned")
SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
T_ROWS, OVERLAP = 64, 8


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
    lb.press_hip_symbol_counts.restype = ctypes.c_int
    lb.press_hip_symbol_counts.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    _cases.clear()


# ------------------------------------------------------------------ buffers of the three kinds

class Buf:
    def __init__(self, store, dtype):
        self.store, self.dtype = store, dtype

    @property
    def ptr(self):
        return self.store.ctypes.data if isinstance(self.store, np.ndarray) else self.store.data_ptr()

    def get(self):
        if isinstance(self.store, np.ndarray):
            return self.store
        import torch
        torch.cuda.synchronize()
        return self.store.cpu().numpy().view(self.dtype)


class Bufs:
    """the arguments of one call: "dev" (torch tensors; device_resident = 1), "pageable" (numpy) or "pinned"
    (press_hip_host_alloc); every buffer lives until close()"""

    def __init__(self, lib, kind):
        self.lib, self.kind, self.dev, self.held, self.pins = lib, kind, int(kind == "dev"), [], []

    def put(self, a):
        a = np.ascontiguousarray(a)
        if self.kind == "dev":
            import torch
            b = Buf(torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype)).copy()).cuda(), a.dtype)
        elif self.kind == "pinned":
            q = self.lib.press_hip_host_alloc(max(a.nbytes, 1))
            assert q, press.last_error()
            self.pins.append(q)
            v = np.frombuffer((ctypes.c_uint8 * a.nbytes).from_address(q), dtype=a.dtype)
            v[:] = a
            b = Buf(v, a.dtype)
        else:
            b = Buf(a.copy(), a.dtype)
        self.held.append(b)
        return b

    def fill(self, n, dtype, value):
        return self.put(np.full(int(n), value, dtype=dtype))

    def ptrs(self, *arrays):
        return [self.put(a).ptr for a in arrays]

    def close(self):
        self.held = []
        for q in self.pins:
            self.lib.press_hip_host_free(q)
        self.pins = []


def three_forms(lib, call, *args):
    """call(lib, *args, bufs) -> dict of numpy results, once per kind -> (device's, {host kind: host's})"""
    out = {}
    for kind in ("dev",) + HOST_KINDS:
        b = Bufs(lib, kind)
        try:
            out[kind] = {k: (v if v is None else np.array(v, copy=True)) for k, v in call(lib, *args, b).items()}
        finally:
            b.close()
    return out["dev"], {k: out[k] for k in HOST_KINDS}


# ------------------------------------------------------------------ the cases: reads, layouts, streams (made once)

def place(rng, lens, shuffle, min_gap=64):
    """ranges of lens[] samples at multiples of 8, min_gap .. min_gap + 40 samples apart (page-locked rooms: the copy back
    covers gaps under 128 bytes, press_hip.h - they stay apart), in a random or the given order -> (off, total)"""
    order = rng.permutation(len(lens)) if shuffle else np.arange(len(lens))
    off = np.zeros(len(lens), dtype=np.uint64)
    pos = 0
    for k in order:
        pos = L.roundup8(pos + min_gap + int(rng.integers(0, 41)))
        off[k] = pos
        pos += int(lens[k])
    return off, L.roundup8(pos) + 64


class Case:
    def __init__(self, lib, m, shape):
        self.m, self.mid, self.shape = m, press.METHODS[m], shape
        rng = np.random.default_rng(4200 + 17 * self.mid + len(shape))
        lens = LENS[shape]
        if shape == "big6":
            _, first = synth.read_lengths(7, 100, len(lens), fixed_len=lens[0])
            self.reads = [synth.synth_read(7, 100 + k, n, int(first[k])) if n else np.zeros(0, dtype=np.int16) for k, n in enumerate(lens)]
        else:
            self.reads = [L._walk(rng, n, 0.01) for n in lens]
        self.nr = len(lens)
        self.ns = np.array(lens, dtype=np.uint32)
        # the samples: noise between the reads
        self.off, self.total = place(rng, lens, shape != "big6")
        self.sig = rng.integers(-32768, 32768, size=self.total).astype(np.int16)
        for k, r in enumerate(self.reads):
            self.sig[int(self.off[k]):int(self.off[k]) + len(r)] = r
        # slots for their streams: the reference's bound and room for exception-heavy reads (_layouts.slot_of), less for
        # the smooth large reads
        slot = (lambda n: int(press.bound(m, n)) + 1024 if n else 32) if shape == "big6" else (lambda n: L.slot_of(press.bound, m, n))
        self.out_off = L.slots(rng, [slot(n) for n in lens])
        # their streams, pressed once by the device-resident call, scattered; one cut short
        self.streams = self.dev_press(lib)
        self.inb, self.in_off, self.in_len = L.scatter_streams(rng, self.streams)
        self.cut = CUT if self.nr == 6 else None
        if self.cut is not None:
            assert len(self.streams[self.cut]) > CUT_BYTES
            self.in_len[self.cut] = CUT_BYTES
        self.roff, self.rtotal = place(rng, lens, shape != "big6")

    def dev_press(self, lib):
        b = Bufs(lib, "dev")
        try:
            r = call_press_batch(lib, self, b)
        finally:
            b.close()
        return [b"" if int(l) == F64 else r["out"][int(o):int(o) + int(l)].tobytes() for o, l in zip(self.out_off, r["out_len"])]

    def decode_args(self, b):
        return b.ptrs(self.inb, self.in_off, self.in_len)


_cases = {}


def case(lib, m, shape):
    if (m, shape) not in _cases:
        _cases[(m, shape)] = Case(lib, m, shape)
    return _cases[(m, shape)]


# ------------------------------------------------------------------ the calls: (lib, case, bufs) -> results

def ok(rc):
    assert rc == 0, press.last_error()


def call_press_batch(lib, c, b):
    out = b.fill(int(c.out_off[-1]) + CANARY, np.uint8, L.ARENA_FILL)
    ln = b.fill(c.nr, np.uint64, 7)
    ok(lib.press_hip_press_batch(c.mid, *b.ptrs(c.sig, c.off, c.ns), c.nr, c.total, out.ptr, b.put(c.out_off).ptr, ln.ptr, b.dev))
    return {"out": out.get(), "out_len": ln.get()}


def call_press_sizes(lib, c, b):
    need = b.fill(c.nr + 8, np.uint64, 7)
    ok(lib.press_hip_press_sizes(c.mid, *b.ptrs(c.sig, c.off, c.ns), c.nr, c.total, need.ptr, b.dev))
    return {"need": need.get()}


def call_press_packed(lib, c, b, align=16):
    room = int(c.out_off[-1]) + 16 * c.nr  # (slots that take every stream, so the packed arena fits)
    out = b.fill(room + CANARY, np.uint8, L.ARENA_FILL)
    oo, ln = b.fill(c.nr + 1, np.uint64, 7), b.fill(c.nr, np.uint64, 7)
    ok(lib.press_hip_press_packed(c.mid, *b.ptrs(c.sig, c.off, c.ns), c.nr, c.total, out.ptr, room, align, oo.ptr, ln.ptr, b.dev))
    return {"out": out.get(), "out_off": oo.get(), "out_len": ln.get()}


def call_depress_batch(lib, c, b):
    sig, on = b.fill(c.rtotal, np.int16, L.SIG_FILL), b.fill(c.nr, np.uint32, 7)
    ok(lib.press_hip_depress_batch(c.mid, *c.decode_args(b), c.nr, sig.ptr, *b.ptrs(c.roff, c.ns), c.rtotal, on.ptr, b.dev))
    return {"sig": sig.get(), "out_n": on.get()}


def call_depress_pa(lib, c, b):
    cal = (np.arange(2 * c.nr, dtype=np.float32) * 0.37 + 0.11).astype(np.float32)
    pa, on = b.fill(c.rtotal, np.float32, -7.5), b.fill(c.nr, np.uint32, 7)
    ok(lib.press_hip_depress_pa_batch(c.mid, *c.decode_args(b), c.nr, pa.ptr, *b.ptrs(c.roff, c.ns), c.rtotal, b.put(cal).ptr, on.ptr, b.dev))
    return {"floats": pa.get(), "out_n": on.get()}


def call_depress_norm(lib, c, b):
    out, on, st = b.fill(c.rtotal, np.float32, -7.5), b.fill(c.nr, np.uint32, 7), b.fill(2 * c.nr, np.int32, 7)
    ok(lib.press_hip_depress_norm_batch(c.mid, *c.decode_args(b), c.nr, out.ptr, *b.ptrs(c.roff, c.ns), c.rtotal, st.ptr, on.ptr, b.dev))
    return {"floats": out.get(), "out_n": on.get(), "stats": st.get()}


def call_depress_chunks(lib, c, b):
    first = np.zeros(c.nr + 1, dtype=np.uint64)
    ok(lib.press_hip_chunk_plan(c.ns.ctypes.data, c.nr, T_ROWS, OVERLAP, first.ctypes.data, None, None))
    nrows = int(first[-1])
    rows = b.fill((nrows + 2) * T_ROWS, np.uint16, 0x7777)  # float16 patterns
    on, q = b.fill(c.nr, np.uint32, 7), b.fill(2 * c.nr, np.int32, 7)
    ok(lib.press_hip_depress_chunks_batch(c.mid, *c.decode_args(b), c.nr, rows.ptr, nrows, 1, T_ROWS, OVERLAP, b.put(first).ptr,
                                          *b.ptrs(c.roff, c.ns), c.rtotal, None, q.ptr, on.ptr, b.dev))
    return {"rows": rows.get(), "nrows": np.array([nrows]), "out_n": on.get(), "q": q.get()}


def recode_outputs(c, b):
    """the destination's slots (sized for either method of the pair), the kept samples, out_n"""
    dst = RECODE_TO[c.m]
    off = L.slots(np.random.default_rng(77), [L.slot_of(press.bound, dst, int(n)) for n in c.ns])
    return dst, off, b.fill(c.rtotal, np.int16, L.SIG_FILL), b.fill(c.nr, np.uint32, 7)


def call_recode_batch(lib, c, b):
    dst, out_off, sig, on = recode_outputs(c, b)
    out, ln = b.fill(int(out_off[-1]) + CANARY, np.uint8, L.ARENA_FILL), b.fill(c.nr, np.uint64, 7)
    ok(lib.press_hip_recode_batch(c.mid, press.METHODS[dst], *c.decode_args(b), *b.ptrs(c.ns, c.roff), c.nr, c.rtotal, out.ptr,
                                  b.put(out_off).ptr, ln.ptr, sig.ptr, on.ptr, b.dev))
    return {"out": out.get(), "out_off": out_off, "out_len": ln.get(), "sig": sig.get(), "out_n": on.get()}


def call_recode_sizes(lib, c, b):
    dst, _, sig, on = recode_outputs(c, b)
    need = b.fill(c.nr + 8, np.uint64, 7)
    ok(lib.press_hip_recode_sizes(c.mid, press.METHODS[dst], *c.decode_args(b), *b.ptrs(c.ns, c.roff), c.nr, c.rtotal, need.ptr,
                                  None, on.ptr, b.dev))  # (without the samples: the other tail of the decode half)
    return {"need": need.get(), "out_n": on.get()}


def call_recode_packed(lib, c, b, align=16):
    dst, out_off, sig, on = recode_outputs(c, b)
    room = int(out_off[-1]) + 16 * c.nr
    out = b.fill(room + CANARY, np.uint8, L.ARENA_FILL)
    oo, ln = b.fill(c.nr + 1, np.uint64, 7), b.fill(c.nr, np.uint64, 7)
    ok(lib.press_hip_recode_packed(c.mid, press.METHODS[dst], *c.decode_args(b), *b.ptrs(c.ns, c.roff), c.nr, c.rtotal, out.ptr, room,
                                   align, oo.ptr, ln.ptr, sig.ptr, on.ptr, b.dev))
    return {"out": out.get(), "out_off": oo.get(), "out_len": ln.get(), "sig": sig.get(), "out_n": on.get()}


def call_signal_stats(lib, c, b):
    st = b.fill(2 * c.nr + 8, np.int32, 7)
    ok(lib.press_hip_signal_stats(*b.ptrs(c.sig, c.off, c.ns), c.nr, c.total, st.ptr, b.dev))
    return {"stats": st.get()}


def call_signal_quantiles(lib, c, b):
    num, den = np.array([1, 1, 3], dtype=np.uint32), np.array([4, 2, 4], dtype=np.uint32)  # (host pointers in both forms)
    q = b.fill(3 * c.nr + 8, np.int32, 7)
    ok(lib.press_hip_signal_quantiles(*b.ptrs(c.sig, c.off, c.ns), c.nr, c.total, num.ctypes.data, den.ctypes.data, 3, q.ptr, b.dev))
    return {"q": q.get()}


def call_symbol_counts(lib, c, b):
    counts = b.put(np.arange(257, dtype=np.uint64) * 3 + 1)  # (the call adds)
    ok(lib.press_hip_symbol_counts(*b.ptrs(c.sig, c.off, c.ns), c.nr, c.total, counts.ptr, b.dev))
    return {"counts": counts.get()}


# ------------------------------------------------------------------ what must be equal

def zstd_content(frame):
    z = press.open_libzstd()
    assert z is not None, "two frames differ and there is no libzstd to compare their content"
    a = np.frombuffer(frame, dtype=np.uint8).copy()
    out = np.zeros(1 << 16, dtype=np.uint8)
    r = z.ZSTD_decompress(out.ctypes.data, out.size, a.ctypes.data, a.size)
    assert not z.ZSTD_isError(r)
    return out[:r].tobytes()


def same_streams(m, d, h, tag, fill_outside):
    """out_len (and out_off) equal, every delivered stream equal, and outside the streams the host arena as it was"""
    assert np.array_equal(d["out_len"], h["out_len"]), tag
    assert np.array_equal(d["out_off"], h["out_off"]), tag
    assert any(int(l) not in (0, F64) for l in d["out_len"]), tag
    inside = np.zeros(h["out"].size, dtype=bool)
    for r, (o, l) in enumerate(zip(d["out_off"], d["out_len"])):
        if int(l) == F64:
            continue
        o, l = int(o), int(l)
        x, y = d["out"][o:o + l], h["out"][o:o + l]
        if not np.array_equal(x, y):
            assert m in L.ZSTD_KINDS and zstd_content(x.tobytes()) == zstd_content(y.tobytes()), tag + (r,)
        inside[o:o + l] = True
    if fill_outside:
        assert (h["out"][~inside] == L.ARENA_FILL).all(), tag + ("bytes written outside the streams",)
    else:  # a packed arena: the host form delivers its padding and gaps as zeros; behind the arena nothing
        total = int(d["out_off"][-1])
        assert (h["out"][total:] == L.ARENA_FILL).all(), tag + ("bytes written behind the arena",)
        assert (h["out"][:total][~inside[:total]] == 0).all(), tag + ("padding does not arrive as zeros",)


def same_elems(c, d, h, key, fill, tag):
    """out_n equal, the delivered samples / floats equal bit for bit, the host rooms' surroundings as they were"""
    assert np.array_equal(d["out_n"], h["out_n"]), tag
    if c.cut is not None:
        assert int(d["out_n"][c.cut]) == F32, tag + ("the cut stream was not refused",)
    assert any(int(k) not in (0, F32) for k in d["out_n"]), tag
    spans = [0 if int(k) == F32 else int(k) for k in d["out_n"]]
    bits = np.uint32 if d[key].dtype == np.float32 else d[key].dtype
    dv, hv = d[key].view(bits), h[key].view(bits)
    for r, k in enumerate(spans):
        o = int(c.roff[r])
        assert np.array_equal(dv[o:o + k], hv[o:o + k]), tag + (r,)
    outside = L.outside_rooms(c.rtotal, c.roff, spans)
    assert (hv[:c.rtotal][outside] == np.array([fill], dtype=d[key].dtype).view(bits)[0]).all(), tag + ("written outside the delivered ranges",)


def same_arrays(d, h, keys, tag):
    for k in keys:
        assert np.array_equal(d[k], h[k]), tag + (k,)


def with_slots(c, r):
    return dict(r, out_off=c.out_off) if "out_off" not in r else r


# ------------------------------------------------------------------ the tests

def cases_of(calls):
    return [(call, m, s) for call in calls for m in METHODS for s in SMALL]


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL] + [("svb12_zd", "big6")])
def test_press_batch(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_press_batch, c)
    for kind, h in hosts.items():
        same_streams(m, with_slots(c, d), with_slots(c, h), (m, shape, kind), True)


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL])
def test_press_sizes(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_press_sizes, c)
    assert (d["need"][c.nr:] == 7).all() and any(int(x) != F64 for x in d["need"][:c.nr])
    for kind, h in hosts.items():
        same_arrays(d, h, ("need",), (m, shape, kind))


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL] + [("svb12_zd", "big6")])
def test_press_packed(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_press_packed, c)
    if shape == "big6":
        assert int(d["out_off"][-1]) > (256 << 10)
    for kind, h in hosts.items():
        same_streams(m, d, h, (m, shape, kind), False)


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL])
def test_depress_batch(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_depress_batch, c)
    for k, r in enumerate(c.reads):  # (the streams are this module's own: they give the reads back)
        if k != c.cut and len(c.streams[k]):
            assert int(d["out_n"][k]) == len(r) and np.array_equal(d["sig"][int(c.roff[k]):int(c.roff[k]) + len(r)], r), (m, shape, k)
    for kind, h in hosts.items():
        same_elems(c, d, h, "sig", np.int16(L.SIG_FILL), (m, shape, kind))


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL] + [("svb12_zd", "big6")])
def test_depress_pa_batch(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_depress_pa, c)
    if shape == "big6":  # the last room is delivered and the staging boundary lies inside it
        last = int(np.argmax(c.roff))
        assert int(d["out_n"][last]) == c.ns[last] and int(c.roff[last]) * 4 < (32 << 20) < (int(c.roff[last]) + int(c.ns[last])) * 4
    for kind, h in hosts.items():
        same_elems(c, d, h, "floats", np.float32(-7.5), (m, shape, kind))


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL])
def test_depress_norm_batch(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_depress_norm, c)
    for kind, h in hosts.items():
        same_elems(c, d, h, "floats", np.float32(-7.5), (m, shape, kind))
        same_arrays(d, h, ("stats",), (m, shape, kind))


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL])
def test_depress_chunks_batch(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_depress_chunks, c)
    n = int(d["nrows"][0]) * T_ROWS
    assert n and (d["rows"][:n] != 0x7777).any()
    for kind, h in hosts.items():
        same_arrays(d, h, ("out_n", "q"), (m, shape, kind))
        assert np.array_equal(d["rows"][:n], h["rows"][:n]), (m, shape, kind)
        assert (h["rows"][n:] == 0x7777).all(), (m, shape, kind, "rows written behind the plan")


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL])
def test_recode_batch(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_recode_batch, c)
    for kind, h in hosts.items():
        same_streams(RECODE_TO[m], d, h, (m, shape, kind), True)
        same_elems(c, d, h, "sig", np.int16(L.SIG_FILL), (m, shape, kind))


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL])
def test_recode_sizes(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_recode_sizes, c)
    assert (d["need"][c.nr:] == 7).all() and any(int(x) != F64 for x in d["need"][:c.nr])
    for kind, h in hosts.items():
        same_arrays(d, h, ("need", "out_n"), (m, shape, kind))


@pytest.mark.parametrize("m,shape", [(m, s) for m in METHODS for s in SMALL])
def test_recode_packed(lib, m, shape):
    c = case(lib, m, shape)
    d, hosts = three_forms(lib, call_recode_packed, c)
    for kind, h in hosts.items():
        same_streams(RECODE_TO[m], d, h, (m, shape, kind), False)
        same_elems(c, d, h, "sig", np.int16(L.SIG_FILL), (m, shape, kind))


@pytest.mark.parametrize("shape", SMALL)
def test_signal_stats(lib, shape):
    c = case(lib, "svb12_zd", shape)
    d, hosts = three_forms(lib, call_signal_stats, c)
    assert (d["stats"][2 * c.nr:] == 7).all() and (d["stats"][:2 * c.nr] != 7).any()
    for kind, h in hosts.items():
        same_arrays(d, h, ("stats",), (shape, kind))


@pytest.mark.parametrize("shape", SMALL)
def test_signal_quantiles(lib, shape):
    c = case(lib, "svb12_zd", shape)
    d, hosts = three_forms(lib, call_signal_quantiles, c)
    assert (d["q"][3 * c.nr:] == 7).all() and (d["q"][:3 * c.nr] != 7).any()
    for kind, h in hosts.items():
        same_arrays(d, h, ("q",), (shape, kind))


@pytest.mark.parametrize("shape", SMALL)
def test_symbol_counts(lib, shape):
    c = case(lib, "svb12_zd", shape)
    d, hosts = three_forms(lib, call_symbol_counts, c)
    assert int(d["counts"].sum()) - int((np.arange(257) * 3 + 1).sum()) == sum(max(len(r) - 1, 0) for r in c.reads)
    for kind, h in hosts.items():
        same_arrays(d, h, ("counts",), (shape, kind))
