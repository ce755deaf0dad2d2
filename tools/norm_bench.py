#!/usr/bin/env python3
"""press_hip_depress_norm_batch against what a caller could do before it existed, device resident, on bench.py's
8192-read batch.

    python3 tools/norm_bench.py [--reads 8192] [--seconds 1.0] [--b-calls 3] [--out FILE]      (--b-calls 0: route a alone)

Per method (slow5_svb_zd and shuffman_vbe21_zd), two routes from the same compressed streams to the same float32 arena
of (x - median) / (1.4826 * MAD):

  a   press_hip_depress_norm_batch
  b   press_hip_depress_batch into an int16 tensor, then per read torch.kthvalue twice (the samples, then
      |samples - median|, rank n // 2 + 1), then the element-wise step as two torch ops over the whole arena
      (torch.add(sig, c0, out=f); f.mul_(c1)) with the two floats of every read expanded by repeat_interleave.
      This is the yardstick: everything the parent commit offers without bringing the samples to the host.

Route a is timed with HIP events around every call, at least --seconds and 20 calls; route b loops over the reads in
Python and takes seconds per call, so it is timed --b-calls times with a wall clock around a synchronised call.  Before
anything is timed the statistics of both routes are compared exactly and the floats bit for bit.
press_hip_signal_stats_timed gives the time of each of the eight new launches on the decoded batch (medians of 20
calls).  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
METHODS = ["slow5_svb_zd", "shuffman_vbe21_zd"]
KERNELS = ["med_count_hi", "med_pick_hi", "med_count_lo", "med_pick_lo", "mad_count_hi", "mad_pick_hi", "mad_count_lo", "mad_pick_lo"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--b-calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("norm_bench needs a GPU")
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
    seg = np.diff(b.starts.astype(np.int64))
    seg[-1] += total - int(b.starts[-1])
    d_seg = torch.from_numpy(seg).to(dev)
    rid = torch.repeat_interleave(torch.arange(R, device=dev), d_seg)
    valid = (torch.arange(total, device=dev) - b.d_off[rid]) < b.d_n[rid]  # the samples of the reads, without the gaps
    del rid
    assert int(valid.sum().item()) == b.total_samples
    offs = [int(x) for x in b.d_off.cpu().numpy()]
    ns = [int(x) for x in b.n]

    result = {"reads": R, "samples": b.total_samples, "methods": {}}
    for m in METHODS:
        mid = press.METHODS[m]
        _, d_src, d_src_off, d_in_off = b.arena(torch, press, m)
        d_len = torch.zeros(R, dtype=torch.int64, device=dev)
        ok(lib.press_hip_press_batch(mid, p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_src), p(d_src_off), p(d_len), 1))
        d_outn = torch.zeros(R, dtype=torch.int32, device=dev)
        d_sig = torch.zeros_like(b.sig)
        f_a = torch.zeros(total, dtype=torch.float32, device=dev)
        f_b = torch.zeros(total, dtype=torch.float32, device=dev)
        st_a = torch.zeros(2 * R, dtype=torch.int32, device=dev)
        med_b = torch.zeros(R, dtype=torch.int32, device=dev)
        mad_b = torch.zeros(R, dtype=torch.int32, device=dev)

        def route_a():
            ok(lib.press_hip_depress_norm_batch(mid, p(d_src), p(d_in_off), p(d_len), R, p(f_a), p(b.d_off), p(b.d_n), total,
                                                p(st_a), p(d_outn), 1))

        def route_b():
            ok(lib.press_hip_depress_batch(mid, p(d_src), p(d_in_off), p(d_len), R, p(d_sig), p(b.d_off), p(b.d_n), total,
                                           p(d_outn), 1))
            for r in range(R):
                if ns[r] == 0:
                    continue
                s = d_sig[offs[r]:offs[r] + ns[r]]
                k = ns[r] // 2 + 1
                med = torch.kthvalue(s, k).values
                med_b[r] = med
                mad_b[r] = torch.kthvalue((s.to(torch.int32) - med.to(torch.int32)).abs(), k).values
            c0 = -med_b.to(torch.float32)
            c1 = torch.where(mad_b > 0, 1.0 / (mad_b.to(torch.float32) * 1.4826), torch.ones((), device=dev))
            torch.add(d_sig, torch.repeat_interleave(c0, d_seg), out=f_b)
            f_b.mul_(torch.repeat_interleave(c1, d_seg))

        for _ in range(3):
            route_a()
        torch.cuda.synchronize()
        assert bool((d_outn.cpu().numpy() == b.n).all()), m
        stats_equal = same = None
        if a.b_calls:
            route_b()
            torch.cuda.synchronize()
            assert torch.equal(d_sig, b.sig), (m, "the decoded samples differ")
            st = st_a.view(R, 2)
            stats_equal = bool(torch.equal(st[:, 0], med_b)) and bool(torch.equal(st[:, 1], mad_b))
            assert stats_equal, (m, "route a and route b differ in median / MAD")
            same = bool(torch.equal(f_a.view(torch.int32)[valid], f_b.view(torch.int32)[valid]))

        ta, spent = [], 0.0
        while spent < a.seconds or len(ta) < 20:
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(8)]
            for e0, e1 in ev:
                e0.record()
                route_a()
                e1.record()
            torch.cuda.synchronize()
            ms = [e0.elapsed_time(e1) for e0, e1 in ev]
            ta += ms
            spent += sum(ms) / 1000.0
        tb = []
        for _ in range(a.b_calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            route_b()
            torch.cuda.synchronize()
            tb.append((time.perf_counter() - t0) * 1000.0)
        # the decode alone (route b's first call), for what the statistics add to it
        td = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ok(lib.press_hip_depress_batch(mid, p(d_src), p(d_in_off), p(d_len), R, p(d_sig), p(b.d_off), p(b.d_n), total, p(d_outn), 1))
            e1.record()
            torch.cuda.synchronize()
            td.append(e0.elapsed_time(e1))
        ta, tb = np.array(ta), np.array(tb)
        rec = {"stats_equal": stats_equal, "floats_bitwise_equal": same,
               "a": {"calls": int(ta.size), "median_ms": float(np.median(ta)), "p10_ms": float(np.percentile(ta, 10)),
                     "p90_ms": float(np.percentile(ta, 90))},
               "depress_batch_median_ms": float(np.median(td))}
        if tb.size:
            rec["b"] = {"calls": int(tb.size), "median_ms": float(np.median(tb)), "min_ms": float(tb.min()), "max_ms": float(tb.max())}
            rec["a_over_b"] = rec["a"]["median_ms"] / rec["b"]["median_ms"]
        rec["samples_per_s_a"] = b.total_samples / (rec["a"]["median_ms"] / 1000.0)
        result["methods"][m] = rec
        del d_src, f_a, f_b

    # the eight launches on the decoded batch
    ms = np.zeros((20, 8), dtype=np.float32)
    st = torch.zeros(2 * R, dtype=torch.int32, device=dev)
    for i in range(ms.shape[0] + 2):
        ok(lib.press_hip_signal_stats_timed(p(b.sig), p(b.d_off), p(b.d_n), R, total, p(st), ms[max(i - 2, 0)].ctypes.data))
    med = np.median(ms, axis=0)
    result["kernel_ms"] = {k: float(v) for k, v in zip(KERNELS, med)}
    result["kernel_ms"]["sum"] = float(med.sum())
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
