#!/usr/bin/env python3
"""press_hip_signal_segments and press_hip_signal_adaptor, device resident, on bench.py's 8192-read batch.

    python3 tools/segments_bench.py [--reads 8192] [--calls 5] [--out FILE]

Raw domain.  Per preset (cDNA, dRNA): the median of --calls pure counts (the three passes of the counting walk and the
layout scan) and of --calls calls with room for all (and the writing walk), each between two HIP events; the kernel times
of the call's three launches through press_hip_kernel_timing; the segments per read; the longest read of the batch as a
batch of its own - one wave's walk, the floor of the call's time.  Then the adaptor call under its preset, likewise.
press_hip_signal_events (DNA preset) and press_hip_signal_stats are timed on the same batch in the same run, as the scale.
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
        sys.exit("segments_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    first = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(R, dtype=torch.int32, device=dev)
    thr = torch.zeros(2 * R, dtype=torch.float32, device=dev)
    result = {"reads": R, "samples": b.total_samples, "longest_read": int(b.n.max()),
              "workspace_bytes": press.signal_segments_workspace_bytes(total, R), "presets": {}}

    def timed(fn, calls):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(np.array(ms)))

    # the longest read alone: what one wave needs for it
    k = int(np.argmax(b.n))
    o1, n1 = b.d_off[k:k + 1].contiguous(), b.d_n[k:k + 1].contiguous()
    f1, c1 = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    for name in ("cdna", "drna"):
        prm = press.jnn_params(name)
        count_only = lambda: press.signal_segments(b.sig, b.d_off, b.d_n, None, prm, None, first, count, thr)
        count_only()
        need = int(first[-1].item())
        seg = torch.zeros((max(need, 1), 2), dtype=torch.int32, device=dev)
        call = lambda: press.signal_segments(b.sig, b.d_off, b.d_n, None, prm, seg, first, count, thr)
        row = {"segments": need, "segments_per_read": need / R, "count_median_ms": timed(count_only, a.calls),
               "records_median_ms": timed(call, a.calls)}
        press.kernel_timing(True)
        call()
        torch.cuda.synchronize()
        kt = press.kernel_times(1)
        press.kernel_timing(False)
        assert len(kt) == 3, kt
        assert int(first[-1].item()) == need and bool((count.cpu().numpy().view(np.uint32) != 0xFFFFFFFF).all())
        row["kernel_ms"] = {k_: float(kt[i]) for i, k_ in enumerate(KERNELS)}
        row["samples_per_s"] = b.total_samples / (row["records_median_ms"] / 1000.0)
        row["longest_read_alone_ms"] = timed(lambda: press.signal_segments(b.sig, o1, n1, None, prm, seg, f1, c1, thr[:2]), 3)
        row["longest_read_segments"] = int(f1[1].item())
        result["presets"][name] = row
        del seg

    prm2 = press.jnn2_params()
    pair = torch.zeros(2 * R, dtype=torch.int32, device=dev)
    adaptor = lambda: press.signal_adaptor(b.sig, b.d_off, b.d_n, prm2, pair, thr)
    result["adaptor"] = {"median_ms": timed(adaptor, a.calls),
                         "longest_read_alone_ms": timed(lambda: press.signal_adaptor(b.sig, o1, n1, prm2, pair[:2], thr[:2]), 3)}
    adaptor()
    torch.cuda.synchronize()
    ph = pair.cpu().numpy().reshape(-1, 2)
    result["adaptor"].update(found=int((ph[:, 1] > 0).sum()), none=int(((ph[:, 0] == 0) & (ph[:, 1] == 0)).sum()),
                             too_short=int((ph[:, 0] < 0).sum()))

    cal = torch.tensor([6.0, 1467.61 / 8192.0], dtype=torch.float32, device=dev).repeat(R).contiguous()
    eprm = press.event_params(False)
    press.signal_events(b.sig, b.d_off, b.d_n, cal, eprm, None, first, count)
    ev = torch.zeros((int(first[-1].item()), 4), dtype=torch.int32, device=dev)
    result["signal_events_median_ms"] = timed(lambda: press.signal_events(b.sig, b.d_off, b.d_n, cal, eprm, ev, first, count), a.calls)
    st = torch.zeros(2 * R, dtype=torch.int32, device=dev)
    result["signal_stats_median_ms"] = timed(lambda: press.signal_stats(b.sig, b.d_off, b.d_n, st), 20)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
