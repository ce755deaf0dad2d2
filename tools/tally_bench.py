#!/usr/bin/env python3
"""press_hip_signal_tally, device resident, on bench.py's 8192-read batch and on three synthetic batches of the same shape.

    python3 tools/tally_bench.py [--reads 8192] [--calls 5] [--out FILE] [--hbm-tbps 7.1]

Legs, each a whole call between two HIP events, alternated (every leg once per round), the median of --calls rounds:
  raw, delta, trans, mom   each output alone
  all                      the four together, one call
  symbol_counts            press_hip_symbol_counts on the same batch: the yardstick that is there
and the time one read of the batch's samples takes at the streaming rate of tools/ubench_stream.hip (--hbm-tbps: a read-only
sweep with the non-temporal policy reached 7.1 TB/s).  The batches: bench.py's synthetic nanopore reads; the same layout
filled with one constant (every lane on one counter), with a +-1 walk (two delta counters, four transition cells) and with
uniform int16 (everything outside every LDS window).  The tables of the first batch are checked against torch.bincount of
the same samples before anything is timed.  One JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hbm-tbps", type=float, default=7.1)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("tally_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    raw = torch.zeros(press.TALLY_BINS, dtype=torch.int64, device=dev)
    delta = torch.zeros(press.TALLY_BINS, dtype=torch.int64, device=dev)
    trans = torch.zeros(press.TALLY_SYMS ** 2, dtype=torch.int64, device=dev)
    mom = torch.zeros(4 * R, dtype=torch.int64, device=dev)
    counts = torch.zeros(press.NBINS, dtype=torch.int64, device=dev)

    def batches():
        yield "nanopore", b.sig
        yield "constant", torch.full((total,), 517, dtype=torch.int16, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(20261020)
        blocks = total // 4096
        walk = torch.full((total,), 500, dtype=torch.int16, device=dev)
        for k0 in range(0, blocks, 16384):  # a walk of +-1 steps that starts again at 500 every 4096 samples
            k1 = min(blocks, k0 + 16384)
            steps = torch.randint(0, 2, (k1 - k0, 4096), dtype=torch.int16, device=dev, generator=g) * 2 - 1
            walk[k0 * 4096:k1 * 4096] = (500 + torch.cumsum(steps, dim=1, dtype=torch.int32)).to(torch.int16).reshape(-1)
        yield "walk", walk
        del walk
        yield "uniform", torch.randint(-32768, 32768, (total,), dtype=torch.int16, device=dev, generator=g)

    def check(sig):
        """raw and the moments' n against torch on the whole batch (the reads tile the arena but for the padding)"""
        for t in (raw, delta, trans):
            t.zero_()
        press.signal_tally(sig, b.d_off, b.d_n, raw, delta, trans, mom)
        torch.cuda.synchronize()
        m = mom.cpu().numpy().view(press.MOMENTS_DTYPE)
        assert np.array_equal(m["n"], np.asarray(b.n, dtype=np.uint32)) and int(raw.sum()) == b.total_samples
        assert int(delta.sum()) == b.total_samples - int((np.asarray(b.n) > 0).sum())
        assert int(trans.sum()) == b.total_samples - int(np.minimum(np.asarray(b.n), 2).sum())

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

    result = {"reads": R, "samples": b.total_samples, "workspace_bytes": press.signal_tally_workspace_bytes(total, R),
              "hbm_tbps": a.hbm_tbps, "hbm_floor_ms": 2.0 * b.total_samples / (a.hbm_tbps * 1e12) * 1e3, "calls": a.calls, "median_ms": {}}
    for name, sig in batches():
        check(sig)
        legs = {"raw": lambda: press.signal_tally(sig, b.d_off, b.d_n, raw=raw),
                "delta": lambda: press.signal_tally(sig, b.d_off, b.d_n, delta=delta),
                "trans": lambda: press.signal_tally(sig, b.d_off, b.d_n, trans=trans),
                "mom": lambda: press.signal_tally(sig, b.d_off, b.d_n, mom=mom),
                "all": lambda: press.signal_tally(sig, b.d_off, b.d_n, raw, delta, trans, mom),
                "symbol_counts": lambda: press.symbol_counts(sig, b.d_off, b.d_n, counts)}
        ms = timed(legs, a.calls)
        ms["sum_of_four_alone"] = ms["raw"] + ms["delta"] + ms["trans"] + ms["mom"]
        result["median_ms"][name] = ms
        print(name, json.dumps(ms), file=sys.stderr, flush=True)
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
