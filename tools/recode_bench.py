#!/usr/bin/env python3
"""press_hip_recode_batch against the two calls it replaces, device resident, on bench.py's 8192-read batch.

    python3 tools/recode_bench.py [--reads 8192] [--baseline-lib PATH] [--seconds 0.5] [--once] [--out FILE]

Legs, per pair (slow5_svb_zd -> shuffman_vbe21_zd, svb_zd -> vbe21_zd), alternated call block by call block within
this one process after a warm-up, HIP events around every whole call, at least --seconds of timed calls per leg:

  baseline   press_hip_depress_batch + press_hip_press_batch of --baseline-lib (a libpress_hip.so built from the parent
             commit: the yardstick), and the same leg a second time (baseline2) for the run-to-run spread
  two_calls  the same two calls of this build (a cross-check, never the yardstick)
  recode     press_hip_recode_batch of this build, the samples kept (sig given)
  recode_ns  ... the samples left in library scratch (sig = NULL)

The recode counts as faster only where it beats the baseline by more than |baseline - baseline2|.  --once: one call per
leg and no timing (for rocprofv3 --kernel-trace --stats and tools/traffic.py, which want few launches).  Every leg's
streams are compared with the first leg's before anything is timed.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIRS = [("slow5_svb_zd", "shuffman_vbe21_zd"), ("svb_zd", "vbe21_zd")]


class Lib:
    """one libpress_hip.so, called through its C ABI on torch's current stream"""

    def __init__(self, path, torch, table):
        self.l = l = ctypes.CDLL(path)
        l.press_hip_last_error.restype = ctypes.c_char_p
        l.press_hip_set_stream.argtypes = [ctypes.c_void_p]
        l.press_hip_load_table_file.argtypes = [ctypes.c_char_p]
        V, U32, U64, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        l.press_hip_press_batch.argtypes = [I, V, V, V, U32, U64, V, V, V, I]
        l.press_hip_depress_batch.argtypes = [I, V, V, V, U32, V, V, V, U64, V, I]
        self.has_recode = hasattr(l, "press_hip_recode_batch")
        if self.has_recode:
            l.press_hip_recode_batch.argtypes = [I, I, V, V, V, V, V, U32, U64, V, V, V, V, V, I]
        self.ok(l.press_hip_set_device(torch.cuda.current_device()))
        self.ok(l.press_hip_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.ok(l.press_hip_load_table_file(table.encode()))

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.l.press_hip_last_error().decode())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--block", type=int, default=16, help="calls of one leg before the next leg's turn")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("recode_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    new = Lib(press.LIB_PATH, torch, press.TABLE_PATH)
    base = Lib(a.baseline_lib, torch, press.TABLE_PATH) if a.baseline_lib else None
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    p = lambda t: None if t is None else t.data_ptr()
    result = {"reads": R, "samples": b.total_samples, "pairs": {}}
    for src, dst in PAIRS:
        sid, did = press.METHODS[src], press.METHODS[dst]
        _, d_src, d_src_off, d_in_off = b.arena(torch, press, src)
        d_src_len = torch.zeros(R, dtype=torch.int64, device=dev)
        new.ok(new.l.press_hip_press_batch(sid, p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_src), p(d_src_off), p(d_src_len), 1))
        caps, d_out, d_out_off, _ = b.arena(torch, press, dst)
        d_len = torch.zeros(R, dtype=torch.int64, device=dev)
        d_outn = torch.zeros(R, dtype=torch.int32, device=dev)
        d_sig = torch.zeros_like(b.sig)

        def two(lib):
            def call():
                lib.ok(lib.l.press_hip_depress_batch(sid, p(d_src), p(d_in_off), p(d_src_len), R, p(d_sig), p(b.d_off), p(b.d_n),
                                                     total, p(d_outn), 1))
                lib.ok(lib.l.press_hip_press_batch(did, p(d_sig), p(b.d_off), p(d_outn), R, total, p(d_out), p(d_out_off),
                                                   p(d_len), 1))
            return call

        def rec(keep):
            def call():
                new.ok(new.l.press_hip_recode_batch(sid, did, p(d_src), p(d_in_off), p(d_src_len), p(b.d_n), p(b.d_off), R, total,
                                                    p(d_out), p(d_out_off), p(d_len), p(d_sig) if keep else None, p(d_outn), 1))
            return call

        legs = ([("baseline", two(base)), ("baseline2", two(base))] if base else []) + \
            [("two_calls", two(new)), ("recode", rec(True)), ("recode_ns", rec(False))]
        # warm-up and agreement: every leg's out_len, out_n and stream bytes as the first leg's
        ref = None
        for name, call in legs:
            d_out.zero_()
            d_len.zero_()
            for _ in range(1 if a.once else 3):
                call()
            torch.cuda.synchronize()
            lens = d_len.cpu().numpy()
            assert (lens > 0).all() and (lens < caps).all(), (name, "a read failed")
            assert bool((d_outn.cpu().numpy() == b.n).all()), name
            got = (lens.copy(), d_out.cpu().numpy().copy())
            if ref is None:
                ref = got
            else:
                assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]), (name, "differs from", legs[0][0])
        assert torch.equal(d_sig, b.sig), "the decoded samples differ"
        rec_pair = {"stream_bytes_in": int(d_src_len.sum().item()), "stream_bytes_out": int(ref[0].sum()), "legs": {}}
        if not a.once:
            times = {name: [] for name, _ in legs}
            spent = {name: 0.0 for name, _ in legs}
            while min(spent.values()) < a.seconds:
                for name, call in legs:
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.block)]
                    for e0, e1 in ev:
                        e0.record()
                        call()
                        e1.record()
                    torch.cuda.synchronize()
                    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
                    times[name] += ms
                    spent[name] += sum(ms) / 1000.0
            for name, ms in times.items():
                ms = np.array(ms)
                rec_pair["legs"][name] = {"calls": int(ms.size), "mean_ms": float(ms.mean()), "median_ms": float(np.median(ms)),
                                          "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
                                          "timed_s": float(ms.sum() / 1000.0)}
            L = rec_pair["legs"]
            if base:
                spread = abs(L["baseline"]["median_ms"] - L["baseline2"]["median_ms"])
                gain = L["baseline"]["median_ms"] - L["recode"]["median_ms"]
                rec_pair["baseline_spread_ms"] = spread
                rec_pair["recode_gain_ms"] = gain
                rec_pair["recode_is_faster"] = bool(gain > spread)
        result["pairs"]["%s->%s" % (src, dst)] = rec_pair
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
