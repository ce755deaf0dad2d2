#!/usr/bin/env python3
"""press_hip_depress_chunks_trimmed_batch against the untrimmed call and against the route a caller had, device resident,
on bench.py's 8192-read batch (slow5_svb_zd, float16, a quantile rule).

    python3 tools/trim_bench.py [--reads 8192] [--T 10000] [--overlap 500] [--cut 2000] [--route-calls 1] [--out FILE]

  untrimmed      press_hip_depress_chunks_batch, row_first from the host plan
  range_whole    the trimmed call, mode RANGE, range NULL: the same rows, the plan made on the device
  range_cut      ... with the range [cut, n) for every read
  adaptor        mode ADAPTOR under sigtk's dRNA preset; adaptor_call: press_hip_signal_adaptor alone on the decoded samples
  segment        mode SEGMENT under sigtk's cDNA preset; segment_call: press_hip_signal_segments (count only) alone
  route          what a caller did for trimmed rows before: press_hip_depress_batch, press_hip_signal_adaptor, the pairs
                 copied to the host, per read a slice, two torch.kthvalue, the scaling, unfold and .half() (--route-calls 0:
                 left out).  Its rows are compared bit for bit with mode ADAPTOR's before anything is timed.

Every library call is timed with HIP events around single calls: the median of 5 after 2 warm-up calls, all in one run.
The route loops over the reads in Python and is timed with a wall clock around a synchronised call.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = "slow5_svb_zd"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--overlap", type=int, default=500)
    ap.add_argument("--cut", type=int, default=2000)
    ap.add_argument("--route-calls", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("trim_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lib = press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    T, S = a.T, a.T - a.overlap
    p = lambda t: t.data_ptr()
    rule = press.ScaleRule(1, 5, 9, 10, 0.51, 10.0, 0.53, 1.0)
    ns = np.asarray([int(x) for x in b.n], dtype=np.uint32)
    offs = [int(x) for x in b.d_off.cpu().numpy()]
    first, _, _ = press.chunk_plan(ns, T, a.overlap)
    nrows = int(first[-1])
    d_first = torch.from_numpy(first.view(np.int64).copy()).to(dev)
    _, d_src, d_src_off, d_in_off = b.arena(torch, press, M)
    d_len = torch.zeros(R, dtype=torch.int64, device=dev)
    if lib.press_hip_press_batch(press.METHODS[M], p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_src), p(d_src_off), p(d_len), 1):
        raise RuntimeError(press.last_error())
    z = lambda k, d: torch.zeros(k, dtype=d, device=dev)
    d_outn, q = z(R, torch.int32), z(2 * R, torch.int32)
    rows = torch.zeros((nrows, T), dtype=torch.float16, device=dev)
    t_first, t_cut, t_read, t_start = z(R + 1, torch.int64), z(2 * R, torch.int32), z(nrows, torch.int32), z(nrows, torch.int32)
    rng_cut = torch.from_numpy(np.stack([np.full(R, a.cut, dtype=np.uint32), ns], axis=1).reshape(-1).view(np.int32).copy()).to(dev)
    adaptor, seg = press.jnn2_params(), press.jnn_params("cdna")
    pair, d_sig = z(2 * R, torch.int32), torch.zeros_like(b.sig)
    seg_first, seg_count = z(R + 1, torch.int64), z(R, torch.int32)

    def trimmed(trim=None, rng=None):
        press.depress_chunks_trimmed_batch(M, d_src, d_in_off, d_len, rows, t_first, b.d_off, b.d_n, total, d_outn, a.overlap, trim=trim, rng=rng,
                                           cut=t_cut, row_read=t_read, row_start=t_start, rule=rule, q=q)

    calls = {
        "untrimmed": lambda: press.depress_chunks_batch(M, d_src, d_in_off, d_len, rows, d_first, b.d_off, b.d_n, total, d_outn, a.overlap, rule, q),
        "range_whole": lambda: trimmed(),
        "range_cut": lambda: trimmed(rng=rng_cut),
        "adaptor": lambda: trimmed(trim=press.trim_adaptor(adaptor)),
        "segment": lambda: trimmed(trim=press.trim_segment(seg)),
        "depress_batch": lambda: press.depress_batch(M, d_src, d_in_off, d_len, d_sig, b.d_off, b.d_n, d_outn),
        "adaptor_call": lambda: press.signal_adaptor(b.sig, b.d_off, b.d_n, adaptor, pair),
        "segment_call": lambda: press.signal_segments(b.sig, b.d_off, b.d_n, None, seg, None, seg_first, seg_count),
    }

    def median_of_5(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    result = {"method": M, "reads": R, "samples": b.total_samples, "T": T, "overlap": a.overlap, "cut": a.cut, "rows": nrows, "ms": {}}
    # before anything is timed: the whole-read ranges give the untrimmed rows and the host plan
    calls["untrimmed"]()
    want = rows.clone()
    rows.zero_()
    calls["range_whole"]()
    torch.cuda.synchronize()
    assert torch.equal(rows.view(torch.int16), want.view(torch.int16)) and torch.equal(t_first, d_first), "range NULL differs from the untrimmed call"
    result["range_whole_equals_untrimmed"] = True
    if a.route_calls:
        calls["adaptor"]()
        torch.cuda.synchronize()
        want, want_first = rows.clone(), t_first.cpu().numpy().view(np.uint64).copy()
        rows_b = torch.zeros_like(rows)

        def route():
            calls["depress_batch"]()
            press.signal_adaptor(d_sig, b.d_off, b.d_n, adaptor, pair)
            end = pair.cpu().numpy().reshape(-1, 2)[:, 1]  # (the synchronisation the trimmed call does not need)
            cut = np.where(end > 0, end, 0).astype(np.int64)
            cut = np.minimum(cut, ns)
            f, _, _ = press.chunk_plan(ns - cut, T, a.overlap)
            qs = []
            for r in range(R):
                c = int(ns[r] - cut[r])
                if c == 0:
                    qs.append(None)
                    continue
                s = d_sig[offs[r] + int(cut[r]):offs[r] + int(ns[r])]
                qs.append((torch.kthvalue(s, min(c - 1, c * rule.lo_num // rule.lo_den) + 1).values,
                           torch.kthvalue(s, min(c - 1, c * rule.hi_num // rule.hi_den) + 1).values))
            q_b = np.array([(0, 0) if v is None else (int(v[0]), int(v[1])) for v in qs], dtype=np.int32)
            cal = torch.from_numpy(press.scale_cal(q_b, rule)).to(dev)
            for r in range(R):
                c = int(ns[r] - cut[r])
                if c == 0:
                    continue
                y = (d_sig[offs[r] + int(cut[r]):offs[r] + int(ns[r])].to(torch.float32) + cal[r, 0]) * cal[r, 1]
                r0, r1 = int(f[r]), int(f[r + 1])
                if c <= T:
                    rows_b[r0, :c] = y.half()
                    rows_b[r0, c:] = 0
                    continue
                rows_b[r0:r1 - 1] = y.unfold(0, T, S)[:r1 - r0 - 1].half()
                rows_b[r1 - 1] = y[c - T:].half()
            return f

        f = route()
        torch.cuda.synchronize()
        k = int(f[-1])
        assert np.array_equal(f, want_first) and torch.equal(rows_b[:k].view(torch.int16), want[:k].view(torch.int16)), "the route's rows differ"
        result["route_rows_bitwise_equal"] = True
        result["adaptor_rows"] = k
        tb = []
        for _ in range(a.route_calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            route()
            torch.cuda.synchronize()
            tb.append((time.perf_counter() - t0) * 1000.0)
        result["ms"]["route"] = float(np.median(tb))
        del rows_b, want
    for name, fn in calls.items():
        result["ms"][name] = median_of_5(fn)
    ms = result["ms"]
    result["range_whole_over_untrimmed"] = ms["range_whole"] / ms["untrimmed"]
    result["range_cut_over_untrimmed"] = ms["range_cut"] / ms["untrimmed"]
    result["adaptor_walk_share"] = ms["adaptor_call"] / ms["adaptor"]
    result["segment_walk_share"] = ms["segment_call"] / ms["segment"]
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
