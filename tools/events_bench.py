#!/usr/bin/env python3
"""press_hip_signal_events, device resident, on bench.py's 8192-read batch.

    python3 tools/events_bench.py [--reads 8192] [--calls 5] [--out FILE]

Per preset (DNA, RNA), with the calibration digitisation 8192, offset 6, range 1467.61 for every read: a pure count for
the batch's need, then --calls calls with room for all, each between two HIP events; the kernel times of the call's three
launches (the counting walk, the layout scan, the writing walk) through press_hip_kernel_timing; the events per read; the
reads whose sums took the serial path (press_hip_events_serial_reads, per call); the workspace; the longest read of the
batch as a batch of its own - one wave's walk, the floor of the call's time.  press_hip_signal_stats is timed on the same batch in the same run, as the scale.
One JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ["count_walk", "layout_scan", "write_walk"]


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
        sys.exit("events_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    cal = torch.tensor([6.0, 1467.61 / 8192.0], dtype=torch.float32, device=dev).repeat(R).contiguous()
    first = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(R, dtype=torch.int32, device=dev)
    result = {"reads": R, "samples": b.total_samples, "longest_read": int(b.n.max()),
              "workspace_bytes": press.signal_events_workspace_bytes(total, R), "presets": {}}

    def timed(fn, calls):
        ms = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return np.array(ms)

    for name, rna in (("dna", False), ("rna", True)):
        prm = press.event_params(rna)
        press.signal_events(b.sig, b.d_off, b.d_n, cal, prm, None, first, count)
        need = int(first[-1].item())
        ev = torch.zeros((need, 4), dtype=torch.int32, device=dev)
        call = lambda: press.signal_events(b.sig, b.d_off, b.d_n, cal, prm, ev, first, count)
        call()
        torch.cuda.synchronize()
        s0 = press.events_serial_reads()
        call()
        serial = press.events_serial_reads() - s0
        ms = timed(call, a.calls)
        press.kernel_timing(True)
        call()
        torch.cuda.synchronize()
        kt = press.kernel_times(1)
        press.kernel_timing(False)
        assert len(kt) == 3, kt
        assert int(first[-1].item()) == need and bool((count.cpu().numpy().view(np.uint32) != 0xFFFFFFFF).all())
        result["presets"][name] = {"events": need, "events_per_read": need / R, "samples_per_event": b.total_samples / need,
                                   "serial_reads": serial, "calls": int(ms.size), "median_ms": float(np.median(ms)),
                                   "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                                   "samples_per_s": b.total_samples / (float(np.median(ms)) / 1000.0),
                                   "kernel_ms": {k: float(kt[i]) for i, k in enumerate(KERNELS)}}
        # the longest read alone: what one wave needs for it, twice
        k = int(np.argmax(b.n))
        o1, n1 = b.d_off[k:k + 1].contiguous(), b.d_n[k:k + 1].contiguous()
        f1, c1 = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        one = lambda: press.signal_events(b.sig, o1, n1, cal[:2], prm, ev, f1, c1)
        one()
        torch.cuda.synchronize()
        result["presets"][name]["longest_read_alone_ms"] = float(np.median(timed(one, 3)))
        result["presets"][name]["longest_read_events"] = int(f1[1].item())
        del ev
    st = torch.zeros(2 * R, dtype=torch.int32, device=dev)
    press.signal_stats(b.sig, b.d_off, b.d_n, st)
    torch.cuda.synchronize()
    ms = timed(lambda: press.signal_stats(b.sig, b.d_off, b.d_n, st), 20)
    result["signal_stats_median_ms"] = float(np.median(ms))
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
