#!/usr/bin/env python3
"""press_hip_signal_prefix and press_hip_signal_range_stats, device resident, on bench.py's 8192-read batch.

    python3 tools/prefix_bench.py [--reads 8192] [--calls 5] [--out FILE]

Legs, each a whole call between two HIP events, alternated (every leg once per round), the median of --calls rounds:
  prefix             press_hip_signal_prefix under its preset, without stat
  prefix_stat        ... with stat and thr
  range_stats_raw    press_hip_signal_range_stats on whole reads, raw domain
  range_stats_pa     ... in picoamperes
  adaptor            press_hip_signal_adaptor alone under JNNV2_RNA_ADAPTOR: the first launch of prefix
  segments_count     press_hip_signal_segments (cDNA preset) as a pure count: the scale of one three-pass walk
Then the longest read of the batch as a batch of its own for prefix_stat and range_stats_pa - one wave's work, the floor of
the call's time -, the kernel times of prefix_stat's three launches (press_hip_kernel_timing) and what prefix found.
One JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ["adaptor", "prefix_walk", "range_stats"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("prefix_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    cal = torch.tensor([6.0, 1467.61 / 8192.0], dtype=torch.float32, device=dev).repeat(R).contiguous()
    out = torch.zeros((R, 4), dtype=torch.int32, device=dev)
    stat = torch.zeros((2 * R, 3), dtype=torch.float32, device=dev)
    rs = torch.zeros((R, 3), dtype=torch.float32, device=dev)
    thr = torch.zeros(2 * R, dtype=torch.float32, device=dev)
    pair = torch.zeros(2 * R, dtype=torch.int32, device=dev)
    first = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(R, dtype=torch.int32, device=dev)
    prm, prm2, cdna = press.prefix_params(), press.jnn2_params(), press.jnn_params("cdna")
    legs = {"prefix": lambda: press.signal_prefix(b.sig, b.d_off, b.d_n, cal, prm, out),
            "prefix_stat": lambda: press.signal_prefix(b.sig, b.d_off, b.d_n, cal, prm, out, stat, thr),
            "range_stats_raw": lambda: press.range_stats(b.sig, b.d_off, b.d_n, None, None, rs),
            "range_stats_pa": lambda: press.range_stats(b.sig, b.d_off, b.d_n, cal, None, rs),
            "adaptor": lambda: press.signal_adaptor(b.sig, b.d_off, b.d_n, prm2, pair),
            "segments_count": lambda: press.signal_segments(b.sig, b.d_off, b.d_n, None, cdna, None, first, count, None)}

    def timed(fns, calls):
        """every leg once per round, `calls` rounds -> the median per leg"""
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(calls):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return {k: float(np.median(np.array(v))) for k, v in ms.items()}

    result = {"reads": R, "samples": b.total_samples, "longest_read": int(b.n.max()),
              "workspace_bytes": press.signal_prefix_workspace_bytes(R), "median_ms": timed(legs, a.calls)}
    result["samples_per_s"] = {k: b.total_samples / (v / 1000.0) for k, v in result["median_ms"].items()}

    # the longest read alone: what one wave needs for it
    k = int(np.argmax(b.n))
    o1, n1 = b.d_off[k:k + 1].contiguous(), b.d_n[k:k + 1].contiguous()
    alone = {"prefix_stat": lambda: press.signal_prefix(b.sig, o1, n1, cal[:2], prm, out[:1], stat[:2], thr[:2]),
             "range_stats_pa": lambda: press.range_stats(b.sig, o1, n1, cal[:2], None, rs[:1])}
    result["longest_read_alone_ms"] = timed(alone, 3)

    press.kernel_timing(True)
    legs["prefix_stat"]()
    torch.cuda.synchronize()
    kt = press.kernel_times(1)
    press.kernel_timing(False)
    assert len(kt) == 3, kt
    result["prefix_stat_kernel_ms"] = {k_: float(kt[i]) for i, k_ in enumerate(KERNELS)}
    oh = out.cpu().numpy()
    result["found"] = {"adaptor": int((oh[:, 1] > 0).sum()), "tail": int((oh[:, 3] > 0).sum()),
                       "none": int((oh[:, 1] == 0).sum()), "too_short": int((oh[:, 1] < 0).sum())}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
