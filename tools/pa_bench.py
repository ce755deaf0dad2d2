#!/usr/bin/env python3
"""press_hip_depress_pa_batch against what a caller could do before it existed, device resident, on bench.py's
8192-read batch.

    python3 tools/pa_bench.py [--reads 8192] [--seconds 1.0] [--out FILE]

Per method (slow5_svb_zd and svb12_zd: the decode kernel writes the floats; vbe21_zd and shuffman_vbe21_zd: decode into
library scratch, then k_pa_convert), two routes from the same compressed streams to the same float32 arena:

  a   press_hip_depress_pa_batch
  b   press_hip_depress_batch into an int16 tensor, then the same formula as torch ops: torch.add(sig, c0, out=pa) and
      pa.mul_(c1) - two element-wise kernels, no temporary, the int16 -> float32 conversion inside the add.  c0 / c1 are
      the per-read calibration expanded to one float per sample by repeat_interleave, outside the timed region.
      This is the yardstick: everything the parent commit offers.

The routes alternate block by block in one process after a warm-up; HIP events around every whole route, at least
--seconds of timed calls and at least 20 steps each; route b is timed a second time (b2) for the run-to-run spread.
Before anything is timed the floats of (a) are compared with those of (b) bit for bit over every read.
One JSON line: per method the two medians, a / b, and the bytes each route moves per sample (counted from the
kernels' loads and stores, the compressed stream's bytes per sample measured).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
METHODS = ["slow5_svb_zd", "svb12_zd", "vbe21_zd", "shuffman_vbe21_zd"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--block", type=int, default=8, help="calls of one route before the next route's turn")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("pa_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lib = press.load_library()
    press.load_table()
    press.use_torch_stream()

    def ok(rc):
        if rc:
            raise RuntimeError(press.last_error())

    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    p = lambda t: t.data_ptr()
    # a calibration of its own for every read, one float per sample of the arena for route b (gaps: the read in front)
    r = np.arange(R, dtype=np.float64)
    dor = np.stack([np.full(R, 8192.0), np.where(r % 2 == 0, 3 + 7 * (r % 97), -(3 + 7 * (r % 97))), 1400.0 * (1 + (r % 64) / 64)], axis=1)
    cal = press.pa_cal(dor)
    d_cal = torch.from_numpy(cal.reshape(-1).copy()).to(dev)
    seg = np.diff(b.starts.astype(np.int64))
    seg[-1] += total - int(b.starts[-1])
    d_seg = torch.from_numpy(seg).to(dev)
    c0 = torch.repeat_interleave(torch.from_numpy(cal[:, 0].copy()).to(dev), d_seg)
    c1 = torch.repeat_interleave(torch.from_numpy(cal[:, 1].copy()).to(dev), d_seg)
    assert c0.numel() == total
    rid = torch.repeat_interleave(torch.arange(R, device=dev), d_seg)
    valid = (torch.arange(total, device=dev) - b.d_off[rid]) < b.d_n[rid]  # the samples of the reads, without the gaps
    del rid
    assert int(valid.sum().item()) == b.total_samples

    result = {"reads": R, "samples": b.total_samples, "methods": {}}
    for m in METHODS:
        mid = press.METHODS[m]
        _, d_src, d_src_off, d_in_off = b.arena(torch, press, m)
        d_len = torch.zeros(R, dtype=torch.int64, device=dev)
        ok(lib.press_hip_press_batch(mid, p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_src), p(d_src_off), p(d_len), 1))
        d_outn = torch.zeros(R, dtype=torch.int32, device=dev)
        d_sig = torch.zeros_like(b.sig)
        pa_a = torch.zeros(total, dtype=torch.float32, device=dev)
        pa_b = torch.zeros(total, dtype=torch.float32, device=dev)

        def route_a():
            ok(lib.press_hip_depress_pa_batch(mid, p(d_src), p(d_in_off), p(d_len), R, p(pa_a), p(b.d_off), p(b.d_n), total,
                                              p(d_cal), p(d_outn), 1))

        def route_b():
            ok(lib.press_hip_depress_batch(mid, p(d_src), p(d_in_off), p(d_len), R, p(d_sig), p(b.d_off), p(b.d_n), total,
                                           p(d_outn), 1))
            torch.add(d_sig, c0, out=pa_b)
            pa_b.mul_(c1)

        legs = [("a", route_a), ("b", route_b), ("b2", route_b)]
        for name, call in legs:  # warm-up, and the routes agree
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            assert bool((d_outn.cpu().numpy() == b.n).all()), (m, name)
        assert torch.equal(d_sig, b.sig), (m, "the decoded samples differ")
        same = bool(torch.equal(pa_a.view(torch.int32)[valid], pa_b.view(torch.int32)[valid]))
        assert same, (m, "route a and route b differ")
        times = {name: [] for name, _ in legs}
        spent = {name: 0.0 for name, _ in legs}
        while min(spent.values()) < a.seconds or min(len(v) for v in times.values()) < 20:
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
        rec = {"fused": bool(press.depress_pa_fused(m)), "bitwise_equal": same, "legs": {}}
        for name, ms in times.items():
            ms = np.array(ms)
            rec["legs"][name] = {"calls": int(ms.size), "median_ms": float(np.median(ms)), "mean_ms": float(ms.mean()),
                                 "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90))}
        L = rec["legs"]
        rec["a_over_b"] = L["a"]["median_ms"] / L["b"]["median_ms"]
        rec["b2_over_b"] = L["b2"]["median_ms"] / L["b"]["median_ms"]
        stream = float(d_len.sum().item()) / b.total_samples
        # loads and stores of sample-sized data per sample (the compressed stream is read once by either route)
        rec["bytes_per_sample"] = {
            "stream": stream,
            "a": 4.0 if rec["fused"] else 2.0 + 2.0 + 4.0,       # floats out; general path: samples out and in again first
            "b": 2.0 + (2.0 + 4.0 + 4.0) + (4.0 + 4.0 + 4.0),   # samples out; add: samples + c0 in, floats out; mul: floats + c1 in, floats out
            "b_least": 2.0 + 2.0 + 4.0}                          # ... a single-pass converter with the calibration in registers
        rec["samples_per_s_a"] = b.total_samples / (L["a"]["median_ms"] / 1000.0)
        result["methods"][m] = rec
        del d_src, d_sig, pa_a, pa_b
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
