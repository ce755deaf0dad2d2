#!/usr/bin/env python3
"""press_hip_depress_chunks_batch against two yardsticks, device resident, on bench.py's 8192-read batch.

    python3 tools/chunks_bench.py [--reads 8192] [--seconds 1.0] [--b-calls 2] [--T 10000] [--overlap 500] [--out FILE]

Per method (slow5_svb_zd and shuffman_vbe21_zd), from the same compressed streams:

  new  press_hip_depress_chunks_batch: float16 rows [nrows, T], a quantile rule (0.2 / 0.9, 0.51 / 0.53, floors 10 / 1)
  a    press_hip_depress_norm_batch: what the library offered before - float32, flat, median / MAD.  It does not make
       the same tensor; it is the nearest existing call and the byte-count argument compares against it.
  b    the route a caller had: press_hip_depress_batch into an int16 tensor, per read two torch.kthvalue (the ranks of
       the rule), press.scale_cal for the two floats, (s.float() + c0) * c1 as two torch ops, unfold for the full rows,
       the last row and the padding by slices, .half().  (--b-calls 0: left out.)

`new`, `a` and the parts of `new` that the library has as calls of their own (press_hip_depress_batch,
press_hip_signal_quantiles with the rule's two ranks, press_hip_signal_stats) are timed with HIP events around every
call, at least --seconds and 20 calls; route b loops over the reads
in Python and is timed --b-calls times with a wall clock around a synchronised call.  Before anything is timed the
quantiles of `new` and b are compared exactly and the rows bit for bit.  One JSON line.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--b-calls", type=int, default=2)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--overlap", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("chunks_bench needs a GPU")
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
    T, S = a.T, a.T - a.overlap
    rule = press.ScaleRule(1, 5, 9, 10, 0.51, 10.0, 0.53, 1.0)
    ns = [int(x) for x in b.n]
    offs = [int(x) for x in b.d_off.cpu().numpy()]
    first, row_read, row_start = press.chunk_plan(np.asarray(ns, dtype=np.uint32), T, a.overlap)
    nrows = int(first[-1])
    d_first = torch.from_numpy(first.view(np.int64).copy()).to(dev)

    def times(fn):
        t, spent = [], 0.0
        while spent < a.seconds or len(t) < 20:
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(8)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            ms = [e0.elapsed_time(e1) for e0, e1 in ev]
            t += ms
            spent += sum(ms) / 1000.0
        t = np.array(t)
        return {"calls": int(t.size), "median_ms": float(np.median(t)), "p10_ms": float(np.percentile(t, 10)),
                "p90_ms": float(np.percentile(t, 90))}

    result = {"reads": R, "samples": b.total_samples, "T": T, "overlap": a.overlap, "rows": nrows, "dtype": "float16", "methods": {}}
    for m in METHODS:
        mid = press.METHODS[m]
        _, d_src, d_src_off, d_in_off = b.arena(torch, press, m)
        d_len = torch.zeros(R, dtype=torch.int64, device=dev)
        ok(lib.press_hip_press_batch(mid, p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_src), p(d_src_off), p(d_len), 1))
        d_outn = torch.zeros(R, dtype=torch.int32, device=dev)
        rows_new = torch.zeros((nrows, T), dtype=torch.float16, device=dev)
        q_new = torch.zeros(2 * R, dtype=torch.int32, device=dev)
        f_a = torch.zeros(total, dtype=torch.float32, device=dev)
        st_a = torch.zeros(2 * R, dtype=torch.int32, device=dev)

        def route_new():
            press.depress_chunks_batch(m, d_src, d_in_off, d_len, rows_new, d_first, b.d_off, b.d_n, total, d_outn, a.overlap, rule, q_new)

        def route_a():
            ok(lib.press_hip_depress_norm_batch(mid, p(d_src), p(d_in_off), p(d_len), R, p(f_a), p(b.d_off), p(b.d_n), total,
                                                p(st_a), p(d_outn), 1))

        for _ in range(3):
            route_new()
            route_a()
        torch.cuda.synchronize()
        assert bool((d_outn.cpu().numpy() == b.n).all()), m
        rec = {"q_equal": None, "rows_bitwise_equal": None}
        tb = []
        if a.b_calls:
            d_sig = torch.zeros_like(b.sig)
            rows_b = torch.zeros((nrows, T), dtype=torch.float16, device=dev)
            q_b = np.zeros((R, 2), dtype=np.int32)

            def route_b():
                ok(lib.press_hip_depress_batch(mid, p(d_src), p(d_in_off), p(d_len), R, p(d_sig), p(b.d_off), p(b.d_n), total,
                                               p(d_outn), 1))
                qs = []
                for r in range(R):
                    c = ns[r]
                    if c == 0:
                        qs.append(None)
                        continue
                    s = d_sig[offs[r]:offs[r] + c]
                    qs.append((torch.kthvalue(s, min(c - 1, c * rule.lo_num // rule.lo_den) + 1).values,
                               torch.kthvalue(s, min(c - 1, c * rule.hi_num // rule.hi_den) + 1).values))
                for r, v in enumerate(qs):  # (one synchronisation for all of them)
                    q_b[r] = (0, 0) if v is None else (int(v[0]), int(v[1]))
                cal = torch.from_numpy(press.scale_cal(q_b, rule)).to(dev)
                for r in range(R):
                    c = ns[r]
                    if c == 0:
                        continue
                    y = (d_sig[offs[r]:offs[r] + c].to(torch.float32) + cal[r, 0]) * cal[r, 1]
                    r0, r1 = int(first[r]), int(first[r + 1])
                    if c <= T:
                        rows_b[r0, :c] = y.half()
                        rows_b[r0, c:] = 0
                        continue
                    full = y.unfold(0, T, S)[:r1 - r0 - 1]
                    rows_b[r0:r1 - 1] = full.half()
                    rows_b[r1 - 1] = y[c - T:].half()

            route_b()
            torch.cuda.synchronize()
            assert torch.equal(d_sig, b.sig), (m, "the decoded samples differ")
            rec["q_equal"] = bool(np.array_equal(q_new.cpu().numpy().reshape(-1, 2), q_b))
            assert rec["q_equal"], (m, "the quantiles of the two routes differ")
            rec["rows_bitwise_equal"] = bool(torch.equal(rows_new.view(torch.int16), rows_b.view(torch.int16)))
            assert rec["rows_bitwise_equal"], (m, "the rows of the two routes differ")
            for _ in range(a.b_calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                route_b()
                torch.cuda.synchronize()
                tb.append((time.perf_counter() - t0) * 1000.0)
            del d_sig, rows_b
        rec["new"] = times(route_new)
        rec["a"] = times(route_a)
        rec["new_over_a"] = rec["new"]["median_ms"] / rec["a"]["median_ms"]
        # the parts, from calls the library has on their own: the decode, the two quantiles and the median / MAD over the
        # decoded samples; what is left of `new` is the tile table and the row writer
        d_sig2 = torch.zeros_like(b.sig)
        q2 = torch.zeros(2 * R, dtype=torch.int32, device=dev)
        ranks = [(rule.lo_num, rule.lo_den), (rule.hi_num, rule.hi_den)]
        rec["parts"] = {
            "depress_batch": times(lambda: ok(lib.press_hip_depress_batch(mid, p(d_src), p(d_in_off), p(d_len), R, p(d_sig2), p(b.d_off),
                                                                          p(b.d_n), total, p(d_outn), 1))),
            "signal_quantiles_2": times(lambda: press.signal_quantiles(b.sig, b.d_off, b.d_n, ranks, q2)),
            "signal_stats": times(lambda: press.signal_stats(b.sig, b.d_off, b.d_n, q2)),
        }
        torch.cuda.synchronize()
        assert torch.equal(d_sig2, b.sig) and torch.equal(q2, st_a), (m, "the parts' results differ")
        del d_sig2
        if tb:
            tb = np.array(tb)
            rec["b"] = {"calls": int(tb.size), "median_ms": float(np.median(tb)), "min_ms": float(tb.min()), "max_ms": float(tb.max())}
            rec["new_over_b"] = rec["new"]["median_ms"] / rec["b"]["median_ms"]
        rec["samples_per_s_new"] = b.total_samples / (rec["new"]["median_ms"] / 1000.0)
        result["methods"][m] = rec
        del d_src, f_a, rows_new

    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
