"""CPU: every wrapper of press.py reaches the library with arguments it accepts.

Without a device every entry point checks its arguments, then asks for the device and fails there, before it touches a
pointer (the order press_batch.hip documents).  So each wrapper can be called here with tiny host buffers - the device
forms with CPU torch tensors - and must come back with the library's "no HIP device" error: a TypeError, a
ctypes.ArgumentError or an AttributeError means the wrapper and the prototype table disagree.

The whole module is skipped where a device is present: the device forms would hand host addresses to kernels."""
import hashlib
import inspect

import numpy as np
import pytest
import torch

from honours_amd import build, press

if torch.cuda.is_available():
    pytest.skip("GPU present: the device forms would run on host addresses", allow_module_level=True)

READS = [np.array([3, -2, 7, 7, 0, -9, 400, -400, 1], dtype=np.int16), np.zeros(0, dtype=np.int16)]
NS = [9, 0]
STREAMS = [bytes([9, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]), b""]
CAL = np.array([[10.0, 0.5], [0.0, 1.0]], dtype=np.float32)
RULE = press.ScaleRule(1, 10, 9, 10, 0.5, 0.0, 1.0, 1.0)


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return press.load_library()


def _no_device(fn, *args, **kw):
    with pytest.raises(press.PressError) as e:
        fn(*args, **kw)
    assert "hip" in str(e.value).lower() and str(e.value) == press.last_error(), str(e.value)


# ---------------------------------------------------------------------------- host forms

HOST = {
    "press_batch_host": lambda f: f("svb_zd", READS),
    "press_packed_host": lambda f: f("svb_zd", READS, align=16),
    "depress_batch_host": lambda f: f("svb_zd", STREAMS, NS),
    "depress_pa_batch_host": lambda f: f("svb_zd", STREAMS, NS, CAL),
    "depress_norm_batch_host": lambda f: f("svb_zd", STREAMS, NS),
    "depress_chunks_batch_host": lambda f: [f("svb_zd", STREAMS, NS, 8, 2, dtype=d, rule=r)
                                            for d in press.CHUNK_DTYPES for r in (None, RULE)],
    "depress_crc_batch_host": lambda f: f("svb_zd", STREAMS, NS),
    "recode_batch_host": lambda f: [f("svb_zd", "vbe21_zd", STREAMS, NS, want_samples=w, degrade_bits=b)
                                    for w in (False, True) for b in (0, 3)],
    "recode_packed_host": lambda f: [f("svb_zd", "vbe21_zd", STREAMS, NS, align=8, want_samples=w, degrade_bits=b)
                                     for w in (False, True) for b in (0, 3)],
    "verify_batch_host": lambda f: [f("svb_zd", STREAMS, READS, degrade_bits=b) for b in (0, 3)],
    "degrade_batch_host": lambda f: f(READS, 3),
    "signal_stats_host": lambda f: f(READS),
    "signal_quantiles_host": lambda f: f(READS, [(1, 10), (9, 10)]),
    "signal_crc32_host": lambda f: f(READS),
    "signal_events_host": lambda f: [f(READS, CAL), f(READS, CAL, prm=press.event_params(True), ev_cap=4)],
    "signal_segments_host": lambda f: [f(READS), f(READS, cal=CAL, seg_cap=4, want_thr=False)],
    "signal_adaptor_host": lambda f: [f(READS), f(READS, want_thr=False)],
    "range_stats_host": lambda f: [f(READS), f(READS, cal=CAL, rng=[[0, 4], [0, 0]])],
    "signal_prefix_host": lambda f: [f(READS, CAL), f(READS, CAL, want_stat=False, want_thr=False)],
    "symbol_counts_host": lambda f: [f(READS), f(READS, counts=np.ones(press.NBINS, dtype=np.uint64))],
    "signal_tally_host": lambda f: [f(READS), f(READS, want=("raw", "mom"), into={"raw": np.ones(press.TALLY_BINS)})],
    "stall_press_batch_host": lambda f: [f(m, READS, want_stall=w) for m in press.STALL_METHODS for w in (False, True)],
    "stall_depress_batch_host": lambda f: f(STREAMS, NS),
    "rcf_press_batch_host": lambda f: [f(c, "vbe21", READS, want_raw=w) for c in press.RCF_CODERS for w in (False, True)],
    "rcf_depress_batch_host": lambda f: [f("rc", l, STREAMS, NS) for l in press.RCF_LAYOUTS],
    "scratch_fill": lambda f: f(0xA5),
    "kernel_timing": lambda f: f(True),
    "load_table": lambda f: f(),
    "use_table": lambda f: f(),
    "train_table": lambda f: f(READS, "unwritten.huffman"),
}


@pytest.mark.parametrize("name", sorted(HOST))
def test_host_form_reaches_the_library(name):
    calls = []

    def once(*args, **kw):
        calls.append(1)
        _no_device(getattr(press, name), *args, **kw)

    HOST[name](once)
    assert calls


def test_host_batch_reaches_the_library():
    for pinned in (False, True):
        if pinned:  # page-locked memory needs the device too: the constructor reports it
            _no_device(press.HostBatch, "svb_zd", READS, pinned=True)
            continue
        hb = press.HostBatch("svb_zd", READS)
        _no_device(hb.press)
        _no_device(hb.depress)
        assert hb.streams() == [b"", b""] and not hb.lossless()  # nothing was written: out_len 0, out_n 0 != ns
        hb.close()


def _hip_was_last(call):
    """call() with another error standing in press.last_error() -> its result; the call must have replaced that error
    with the missing device"""
    with pytest.raises(press.PressError, match="multiple of 8"):
        press.chunk_plan(NS, 4, 1)
    assert "hip" not in press.last_error().lower()
    res = call()
    assert "hip" in press.last_error().lower(), press.last_error()
    return res


@pytest.mark.parametrize("method", sorted(press.METHODS))
def test_per_read_press_depress(method):
    ret, out = _hip_was_last(lambda: press.press(method, READS[0]))
    assert ret != 0 and out == b""
    if press._SYMS[method][3] in ("svb", "svb_nz"):
        # svb12_depress, svb12_zd_depress and svb_zd_depress_16 return void and have no count that could say "failed":
        # the wrapper's ret is 0 whatever happened, and the error is all there is
        ret, back = _hip_was_last(lambda: press.depress(method, STREAMS[0], 9))
    else:
        # (some methods read the stream's header on the host first and refuse these arbitrary bytes before they ask for
        # the device: a status of the library's all the same)
        ret, back = press.depress(method, STREAMS[0], 9)
        assert ret != 0
    assert back.dtype == np.int16


def test_per_read_stall_and_rcf():
    for m in press.STALL_METHODS:
        assert _hip_was_last(lambda: press.stall_press(m, READS[0])) == (-1, b"")
        ret, back = press.stall_depress(m, STREAMS[0], 9)
        assert ret == -1 and back.size == 0 and back.dtype == np.int16
    for c in press.RCF_CODERS:
        for l in press.RCF_LAYOUTS:
            assert _hip_was_last(lambda: press.rcf_press(c, l, READS[0])) == (-1, b"")
            ret, back = press.rcf_depress(c, l, STREAMS[0], 9)
            assert ret == -1 and back.size == 0 and back.dtype == np.int16


# ---------------------------------------------------------------------------- device forms, on CPU tensors

def _t(values, dtype):
    return torch.tensor(values, dtype=dtype)


def _z(count, dtype):
    return torch.zeros(count, dtype=dtype)


SIG, OFF, N = _z(16 + 64, torch.int16), _t([0, 16], torch.int64), _t(NS, torch.int32)
COMP, IN_OFF, IN_LEN = _z(12 + 64, torch.uint8), _t([0, 12], torch.int64), _t([12, 0], torch.int64)
OUT, OUT_OFF, OUT_LEN = _z(256 + 64, torch.uint8), _t([0, 128, 256], torch.int64), _z(2, torch.int64)
OUT_N, F32, TCAL = _z(2, torch.int32), _z(16 + 64, torch.float32), torch.from_numpy(CAL.reshape(-1).copy())
I32x2, F32x2, U32 = _z(4, torch.int32), _z(4, torch.float32), _z(2, torch.int32)
FIRST = _z(3, torch.int64)
DECODE = (COMP, IN_OFF, IN_LEN)
RECODE = ("svb_zd", "vbe21_zd", COMP, IN_OFF, IN_LEN, N, OFF)

DEVICE = {
    "press_batch": lambda f: f("svb_zd", SIG, OFF, N, OUT, OUT_OFF, OUT_LEN),
    "press_sizes": lambda f: f("svb_zd", SIG, OFF, N),
    "press_packed": lambda f: f("svb_zd", SIG, OFF, N, OUT, _z(3, torch.int64), OUT_LEN, align=16),
    "depress_batch": lambda f: f("svb_zd", *DECODE, SIG, OFF, N, OUT_N),
    "depress_pa_batch": lambda f: f("svb_zd", *DECODE, F32, OFF, N, TCAL, OUT_N),
    "depress_norm_batch": lambda f: [f("svb_zd", *DECODE, F32, OFF, N, OUT_N), f("svb_zd", *DECODE, F32, OFF, N, OUT_N, stats=I32x2)],
    "depress_chunks_batch": lambda f: [f("svb_zd", *DECODE, _z((2, 8), d), FIRST, OFF, N, 16, OUT_N, 2, rule=r, q=q)
                                       for d in (torch.float32, torch.float16, torch.bfloat16)
                                       for r, q in ((None, None), (RULE, I32x2))],
    "depress_crc_batch": lambda f: f("svb_zd", *DECODE, OFF, N, 16, U32, OUT_N),
    "recode_batch": lambda f: [f(*RECODE, OUT, OUT_OFF, OUT_LEN, OUT_N, sig=SIG, degrade_bits=b) for b in (0, 3)] +
                              [f(*RECODE, OUT, OUT_OFF, OUT_LEN, OUT_N, total_samples=16, degrade_bits=b) for b in (0, 3)],
    "recode_sizes": lambda f: [f(*RECODE, OUT_N, sig=SIG, degrade_bits=b) for b in (0, 3)] +
                              [f(*RECODE, OUT_N, total_samples=16, degrade_bits=b) for b in (0, 3)],
    "recode_packed": lambda f: [f(*RECODE, OUT, _z(3, torch.int64), OUT_LEN, OUT_N, sig=SIG, align=8, degrade_bits=b) for b in (0, 3)] +
                               [f(*RECODE, OUT, _z(3, torch.int64), OUT_LEN, OUT_N, total_samples=16, degrade_bits=b) for b in (0, 3)],
    "verify_batch": lambda f: [f("svb_zd", *DECODE, SIG, OFF, N, U32, OUT_N, _z(1, torch.int32), degrade_bits=b) for b in (0, 3)],
    "degrade_batch": lambda f: [f(SIG, OFF, N, 3), f(SIG, OFF, N, 3, out=_z(16 + 64, torch.int16))],
    "signal_stats": lambda f: f(SIG, OFF, N, I32x2),
    "signal_quantiles": lambda f: f(SIG, OFF, N, [(1, 10), (9, 10)], I32x2),
    "signal_crc32": lambda f: f(SIG, OFF, N, U32),
    "signal_events": lambda f: [f(SIG, OFF, N, TCAL, press.event_params(), _z((4, 4), torch.int32), FIRST, U32),
                                f(SIG, OFF, N, TCAL, press.event_params(), None, FIRST, U32)],
    "signal_segments": lambda f: [f(SIG, OFF, N, TCAL, press.jnn_params(), _z((4, 2), torch.int32), FIRST, U32, thr=F32x2),
                                  f(SIG, OFF, N, None, press.jnn_params(), None, FIRST, U32)],
    "signal_adaptor": lambda f: [f(SIG, OFF, N, press.jnn2_params(), I32x2, thr=F32x2), f(SIG, OFF, N, press.jnn2_params(), I32x2)],
    "range_stats": lambda f: [f(SIG, OFF, N, TCAL, I32x2, _z((2, 3), torch.float32)), f(SIG, OFF, N, None, None, _z((2, 3), torch.float32))],
    "signal_prefix": lambda f: [f(SIG, OFF, N, TCAL, press.prefix_params(), _z((2, 4), torch.int32),
                                  stat=_z((4, 3), torch.float32), thr=F32x2),
                                f(SIG, OFF, N, TCAL, press.prefix_params(), _z((2, 4), torch.int32))],
    "signal_stat_table": lambda f: f(SIG, OFF, N, TCAL),
    "symbol_counts": lambda f: f(SIG, OFF, N, _z(press.NBINS, torch.int64)),
    "signal_tally": lambda f: [f(SIG, OFF, N, mom=_z(16, torch.int32)),  # (no output at all: nothing to do, no device asked for)
                               f(SIG, OFF, N, _z(press.TALLY_BINS, torch.int64), _z(press.TALLY_BINS, torch.int64),
                                 _z(press.TALLY_SYMS ** 2, torch.int64), _z(8, torch.int64))],
    "stall_press_batch": lambda f: [f("dstall_fz", SIG, OFF, N, OUT, OUT_OFF, OUT_LEN), f(0, SIG, OFF, N, OUT, OUT_OFF, OUT_LEN, stall=I32x2)],
    "stall_depress_batch": lambda f: f(*DECODE, SIG, OFF, N, OUT_N),
    "rcf_press_batch": lambda f: [f("rccdf", "vbbe21", SIG, OFF, N, OUT, OUT_OFF, OUT_LEN),
                                  f("rc", "vbe21", SIG, OFF, N, OUT, OUT_OFF, OUT_LEN, raw=_z(2, torch.uint8))],
    "rcf_depress_batch": lambda f: f("rccdf", "vbbe21", *DECODE, SIG, OFF, N, OUT_N),
}


@pytest.mark.parametrize("name", sorted(DEVICE))
def test_device_form_reaches_the_library(name):
    calls = []

    def once(*args, **kw):
        calls.append(1)
        _no_device(getattr(press, name), *args, **kw)

    DEVICE[name](once)
    assert calls


# ---------------------------------------------------------------------------- host arithmetic and small getters

def _fields(s):
    return [_fields(getattr(s, f)) if hasattr(getattr(s, f), "_fields_") else getattr(s, f) for f, _ in s._fields_]


def _table_digest(f):
    ln, bits = f(np.arange(1, 257, dtype=np.uint64))
    return str(ln.dtype), str(bits.dtype), int(ln.sum()), int(ln[0]), int(ln[255]), int(bits[0]), int(bits[255])


def _write_table(f, tmp_path):
    ln, bits = press.table_from_counts(np.arange(1, 257, dtype=np.uint64))
    path = str(tmp_path / "t.huffman")
    f(path, ln, bits, 77)
    press.HuffmanTable(path).close()  # read_code_table and build_symbol_encoder take it
    data = open(path, "rb").read()
    return len(data), hashlib.sha256(data).hexdigest()[:16]


_MOM = np.array([(6, 14, 1, 3, 3, 0)], dtype=press.MOMENTS_DTYPE)
_TRANS = np.zeros((press.TALLY_SYMS, press.TALLY_SYMS), dtype=np.uint64)
_TRANS[0, 0], _TRANS[0, 1], _TRANS[1, 0] = 2, 1, 1
_JNN = [-1.0, 50, 200, 250, 1.0, 30, 0.0, 0.0]
_JNN2 = [0.5, 1500, 2000, 200000, 2000]

# No device and no batch: each is called once with its smallest input, and returns what it returned before the binding
# layer was put on one table (the literals).
PURE = {
    "pa_cal": (lambda f: f([[8192.0, 10.0, 1400.0]]).tolist(), [[10.0, 0.1708984375]]),
    "norm_cal": (lambda f: f([[5, 2]]).tolist(), [[-5.0, 0.337245374917984]]),
    "scale_cal": (lambda f: f([[1, 3]], RULE).tolist(), [[-2.0, 0.5]]),
    "chunk_plan": (lambda f: [(x.tolist(), str(x.dtype)) for x in f(NS, 8, 2)],
                   [([0, 2, 2], "uint64"), ([0, 0], "uint32"), ([0, 1], "uint32")]),
    "crc32_combine": (lambda f: f(1, 2, 3), 29518389),
    "degrade": (lambda f: f([5, -3, 32767], 2).tolist(), [4, -4, 32764]),
    "degrade_value": (lambda f: (f(5, 2), f(-3, 2), f(32767, 2)), (4, -4, 32764)),
    "tally_value": (lambda f: f([0, 1, 2, 3]).tolist(), [0, -1, 1, -2]),
    "tally_table": (lambda f: [x.tolist() for x in f([0, 2, 1])], [[-1, 1], [2, 1]]),
    "tally_text": (lambda f: f([0, 2, 1]), "signal\tfreq\n-1\t2\n1\t1\n"),
    "tally_summary": (lambda f: f([0, 2, 1]),
                      {"n": 3, "min": -1, "q1": -1, "mean": -0.3333333333333333, "median": -1, "q3": 1, "max": 1, "mode": -1,
                       "var": 0.8888888888888888, "std": 0.9428090415820634, "entropy": 0.9182958340544893}),
    "transition_entropy": (lambda f: f(_TRANS), (0.8112781244591328, 0.6887218755408672)),
    "moments_stats": (lambda f: {k: v.tolist() for k, v in f(_MOM, [[8192.0, 10.0, 1400.0]]).items()},
                      {"mean": [2.0], "var": [0.6666666666666666], "sd": [0.816496580927726], "min_pa": [1.8798828125],
                       "max_pa": [2.2216796875], "mean_pa": [2.05078125], "var_pa": [0.019470850626627602],
                       "sd_pa": [0.13953798990464067]}),
    "table_from_counts": (_table_digest, ("uint32", "uint64", 2175, 15, 7, 127, 21)),
    "write_table": (_write_table, (872, "0091ba1ee41b4050")),
    "bound": (lambda f: [f(m, 9) for m in press.METHODS],
              [54, 54, 55, 122, 121, 19, 19, 19, 19, 19, 19, 19, 19, 97, 160, 43, 19, 19, 19]),
    "stall_bound": (lambda f: [f(m, 9) for m in press.STALL_METHODS], [19, 19, 19]),
    "rcf_bound": (lambda f: [f(c, l, 9) for c in press.RCF_CODERS for l in press.RCF_LAYOUTS], [19] * 16),
    "rcf_name": (lambda f: (f("rccdf", "vbe21"), f(0, 3)), ("rccdf_vbe21_zd", "rc_vbsse21_zd")),
    "stall_workspace_bytes": (lambda f: f("dstall_fz", 16, 2), 6572),
    "signal_events_workspace_bytes": (lambda f: f(16, 2), 16),
    "signal_segments_workspace_bytes": (lambda f: f(16, 2), 32),
    "signal_prefix_workspace_bytes": (lambda f: f(2), 48),
    "signal_tally_workspace_bytes": (lambda f: f(16, 2), 88),
    "packed_exact": (lambda f: (f("svb_zd"), f("rc_vbe21_zd")), (True, False)),
    "depress_pa_fused": (lambda f: (f("svb_zd"), f("zstd_svb_zd")), (True, False)),
    "recode_fused": (lambda f: (f("svb_zd", "vbe21_zd"), f("zstd_svb_zd", "svb_zd")), (True, False)),
    "kernel_times": (lambda f: (f(0), f(1)), ([], [])),
    "events_serial_reads": (lambda f: f(), 0),
    "pass_a_launches": (lambda f: f(), 0),
    "event_params": (lambda f: (_fields(f()), _fields(f(True))),
                     ([3, 6, 1.399999976158142, 9.0, 0.20000000298023224], [7, 14, 2.5, 9.0, 1.0])),
    "jnn_params": (lambda f: [_fields(f(k)) for k in press.JNN_KINDS],
                   [[0.75, 50, 50, 150, 0.25, 5, 0.0, 0.0], [0.75, 50, 50, 1000, 1.0, 5, 0.0, 0.0], _JNN]),
    "jnn2_params": (lambda f: _fields(f()), _JNN2),
    "prefix_params": (lambda f: _fields(f()), [_JNN2, _JNN, 1, 30.0, 20.0]),
}


@pytest.mark.parametrize("name", sorted(PURE))
def test_host_arithmetic_is_what_it_was(name, tmp_path):
    call, want = PURE[name]
    got = call(getattr(press, name), tmp_path) if name == "write_table" else call(getattr(press, name))
    assert got == want, (name, got, want)


# Neither a batch nor arithmetic: how the library and its table are opened, and what needs a file or a CUDA device
# before the library is asked anything.
ELSEWHERE = {
    "load_library", "last_error", "default_table", "open_libzstd",  # used by every test above / test_abi_symbols.py
    "use_torch_stream",       # torch.cuda.current_device() raises first; every GPU test starts with it
    "blow5_write_like", "blow5_transcode",  # need a BLOW5 file: tests/test_blow5.py calls both without a GPU
    "dataset_report",         # starts with use_torch_stream(); tests/test_signal_tally.py
}


def test_every_wrapper_is_called():
    public = {n for n, f in vars(press).items()
              if not n.startswith("_") and inspect.isfunction(f) and f.__module__.startswith("honours_amd.")}
    per_read = {"press", "depress", "stall_press", "stall_depress", "rcf_press", "rcf_depress"}
    called = set(HOST) | set(DEVICE) | set(PURE) | per_read
    assert not public - called - ELSEWHERE, sorted(public - called - ELSEWHERE)
    assert not (called | ELSEWHERE) - public, sorted((called | ELSEWHERE) - public)  # the lists name nothing that is gone
    assert not called & ELSEWHERE
