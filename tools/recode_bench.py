#!/usr/bin/env python3
"""press_hip_recode_packed and press_hip_recode_sizes against press_hip_recode_batch, device resident, on bench.py's
8192-read batch.

    python3 tools/recode_bench.py [--reads 8192] [--baseline-lib PATH] [--seconds 0.5] [--once] [--out FILE]

Legs, per pair (slow5_svb_zd -> shuffman_vbe21_zd fused, svb_zd -> vbe21_zd fused, vbe21_zd -> slow5_svb_zd: an svb
destination, vbe21_zd -> zstd_svb_zd: a zstd one), alternated call block by call block within this one process after a
warm-up, HIP events around every whole call, at least --seconds of timed calls per leg:

  baseline    press_hip_recode_batch of --baseline-lib (a libpress_hip.so built from the parent commit: the yardstick),
              and the same leg a second time (baseline2) for the run-to-run spread
  recode      press_hip_recode_batch of this build (the same code: a cross-check of the yardstick)
  packed_a1   press_hip_recode_packed of this build, align 1
  packed_a16  ... align 16
  sizes       press_hip_recode_sizes of this build
All with the samples kept (sig given).  A leg differs from the baseline only where the medians are further apart than
|baseline - baseline2|.  Beside the times: the arena bytes of each layout (out_off[nreads]) against the sum of
press_hip_bound over the reads, which is what a caller's slot table is made of.  --once: one call per leg and no timing
(for rocprofv3 --kernel-trace --stats and tools/traffic.py, which want few launches).  Every leg's streams are compared
with the first leg's before anything is timed.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIRS = [("slow5_svb_zd", "shuffman_vbe21_zd"), ("svb_zd", "vbe21_zd"), ("vbe21_zd", "slow5_svb_zd"), ("vbe21_zd", "zstd_svb_zd")]


class Lib:
    """one libpress_hip.so, called through its C ABI on torch's current stream"""

    def __init__(self, path, torch, table):
        self.l = l = ctypes.CDLL(path)
        from honours_amd import abi

        abi.declare(l, optional=True)  # (an older build lacks some of the table's symbols)
        self.has_recode = hasattr(l, "press_hip_recode_batch")
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

        d_poff = torch.zeros(R + 1, dtype=torch.int64, device=dev)
        d_need = torch.zeros(R, dtype=torch.int64, device=dev)

        def rec(lib):
            def call():
                lib.ok(lib.l.press_hip_recode_batch(sid, did, p(d_src), p(d_in_off), p(d_src_len), p(b.d_n), p(b.d_off), R, total,
                                                    p(d_out), p(d_out_off), p(d_len), p(d_sig), p(d_outn), 1))
            return call

        def packed(align):
            def call():
                new.ok(new.l.press_hip_recode_packed(sid, did, p(d_src), p(d_in_off), p(d_src_len), p(b.d_n), p(b.d_off), R,
                                                     total, p(d_out), d_out.numel() - 64, align, p(d_poff), p(d_len), p(d_sig),
                                                     p(d_outn), 1))
            return call

        def sizes():
            new.ok(new.l.press_hip_recode_sizes(sid, did, p(d_src), p(d_in_off), p(d_src_len), p(b.d_n), p(b.d_off), R, total,
                                                p(d_need), p(d_sig), p(d_outn), 1))

        legs = ([("baseline", rec(base)), ("baseline2", rec(base))] if base and base.has_recode else []) + \
            [("recode", rec(new)), ("packed_a1", packed(1)), ("packed_a16", packed(16)), ("sizes", sizes)]
        # warm-up and agreement: every leg's out_len, out_n and stream bytes as the first leg's
        ref = None
        slot_off = d_out_off.cpu().numpy()
        arena_bytes = {}
        for name, call in legs:
            d_out.zero_()
            d_len.zero_()
            for _ in range(1 if a.once else 3):
                call()
            torch.cuda.synchronize()
            assert bool((d_outn.cpu().numpy() == b.n).all()), name
            if name == "sizes":
                assert np.array_equal(d_need.cpu().numpy(), ref[0]), (name, "differs from", legs[0][0])
                continue
            lens = d_len.cpu().numpy()
            assert (lens > 0).all() and (lens < caps).all(), (name, "a read failed")
            offs = d_poff.cpu().numpy() if name.startswith("packed") else slot_off
            if name.startswith("packed"):
                arena_bytes[name] = int(offs[-1])
            host = d_out.cpu().numpy()
            got = (lens.copy(), np.concatenate([host[int(o):int(o) + int(l)] for o, l in zip(offs[:-1], lens)]))
            if ref is None:
                ref = got
            else:
                assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]), (name, "differs from", legs[0][0])
        assert torch.equal(d_sig, b.sig), "the decoded samples differ"
        bound = int(sum(int(new.l.press_hip_bound(did, int(x))) for x in b.n))
        rec_pair = {"fused": bool(press.recode_fused(src, dst)), "stream_bytes_in": int(d_src_len.sum().item()),
                    "stream_bytes_out": int(ref[0].sum()), "arena_bytes": arena_bytes, "sum_of_press_hip_bound": bound,
                    "legs": {}}
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
            if "baseline" in L:
                spread = abs(L["baseline"]["median_ms"] - L["baseline2"]["median_ms"])
                rec_pair["baseline_spread_ms"] = spread
                for name in ("recode", "packed_a1", "packed_a16", "sizes"):
                    rec_pair[name + "_minus_baseline_ms"] = L[name]["median_ms"] - L["baseline"]["median_ms"]
                    rec_pair[name + "_differs"] = bool(abs(rec_pair[name + "_minus_baseline_ms"]) > spread)
        result["pairs"]["%s->%s" % (src, dst)] = rec_pair
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
