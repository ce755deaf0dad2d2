#!/usr/bin/env python3
"""Lossy archives on bench.py's 8192-read batch: what dropping b low bits saves, and what the degraded recode costs.

    python3 tools/degrade_bench.py [--reads 8192] [--baseline-lib PATH] [--seconds 0.5] [--out FILE]

1. Ratios.  The batch as svb_zd streams, recoded with press_hip_recode_degraded_batch at bits 0 .. 5 into
   hasgam_vbsse21_zdq, zstd_svb_zd, rc_vbe21_zd and shuffman_vbe21_zd - the last twice: with the shipped table, and with
   a table fitted to the degraded reads (press_hip_degrade_batch, press_hip_symbol_counts, press_hip_table_from_counts,
   all on the device but the construction).  ratio = 2 * samples / stream bytes.

2. Times, bits = 3, one fused pair (slow5_svb_zd -> shuffman_vbe21_zd) and one that is not (vbe21_zd -> slow5_svb_zd),
   device resident, samples kept, legs alternated call block by call block after a warm-up, HIP events around every whole
   call, at least --seconds of timed calls per leg:
     baseline    press_hip_recode_batch of --baseline-lib, a libpress_hip.so built from the parent commit: yardstick (a);
                 and the same leg a second time (baseline2) for the run-to-run spread
     recode      press_hip_recode_batch of this build (undegraded: a cross-check of the yardstick)
     degraded    press_hip_recode_degraded_batch of this build
     three_call  yardstick (b): press_hip_depress_batch, press_hip_degrade_batch in place, press_hip_press_batch
   The degraded leg's streams are compared with the three-call route's before anything is timed.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = "svb_zd"
DSTS = ["hasgam_vbsse21_zdq", "zstd_svb_zd", "rc_vbe21_zd", "shuffman_vbe21_zd"]
PAIRS = [("slow5_svb_zd", "shuffman_vbe21_zd"), ("vbe21_zd", "slow5_svb_zd")]
BITS = 3


class Lib:
    """one libpress_hip.so, called through its C ABI on torch's current stream"""

    def __init__(self, path, torch, table):
        self.l = l = ctypes.CDLL(path)
        from honours_amd import abi

        abi.declare(l, optional=True)  # (an older build lacks some of the table's symbols)
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("degrade_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    new = Lib(press.LIB_PATH, torch, press.TABLE_PATH)
    press.load_library()
    press.use_torch_stream()
    base = Lib(a.baseline_lib, torch, press.TABLE_PATH) if a.baseline_lib else None
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    p = lambda t: None if t is None else t.data_ptr()
    result = {"reads": R, "samples": b.total_samples, "ratios": {}, "times": {}}

    def source(src):
        """the batch as streams of src -> (arena, in_off, in_len)"""
        _, d_src, d_src_off, d_in_off = b.arena(torch, press, src)
        d_src_len = torch.zeros(R, dtype=torch.int64, device=dev)
        new.ok(new.l.press_hip_press_batch(press.METHODS[src], p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_src), p(d_src_off),
                                           p(d_src_len), 1))
        return d_src, d_in_off, d_src_len

    # ---- 1: ratios
    d_src, d_in_off, d_src_len = source(SRC)
    sid = press.METHODS[SRC]
    d_outn = torch.zeros(R, dtype=torch.int32, device=dev)
    d_deg = torch.zeros_like(b.sig)
    for bits in range(6):
        row = {}
        for dst in DSTS + ["shuffman_vbe21_zd fitted"]:
            m = dst.split()[0]
            if dst.endswith("fitted"):  # a table for the degraded reads: degrade, count, construct, set
                press.degrade_batch(b.sig, b.d_off, b.d_n, bits, d_deg)
                counts = torch.zeros(press.NBINS, dtype=torch.int64, device=dev)
                press.symbol_counts(d_deg, b.d_off, b.d_n, counts)
                ln, cb = press.table_from_counts(counts.cpu().numpy().view(np.uint64))
                new.ok(new.l.press_hip_set_table(ln.ctypes.data, cb.ctypes.data))
                row["fitted_table_longest_code"] = int(ln.max())
            caps, d_out, d_out_off, _ = b.arena(torch, press, m)
            d_len = torch.zeros(R, dtype=torch.int64, device=dev)
            new.ok(new.l.press_hip_recode_degraded_batch(sid, press.METHODS[m], bits, p(d_src), p(d_in_off), p(d_src_len), p(b.d_n),
                                                         p(b.d_off), R, total, p(d_out), p(d_out_off), p(d_len), None, p(d_outn), 1))
            torch.cuda.synchronize()
            lens = d_len.cpu().numpy()
            ok = lens > 0  # (a static-Huffman table need not hold a code for every value: such a read is refused)
            assert (lens[ok] < caps[ok]).all() and ok.any(), (dst, bits)
            row[dst] = {"bytes": int(lens[ok].sum()), "refused_reads": int((~ok).sum()),
                        "ratio": 2.0 * float(b.n[ok].sum()) / float(lens[ok].sum())}
            if dst.endswith("fitted"):
                new.ok(new.l.press_hip_load_table_file(press.TABLE_PATH.encode()))
            del d_out
        result["ratios"][str(bits)] = row

    # ---- 2: times
    for src, dst in PAIRS:
        sid, did = press.METHODS[src], press.METHODS[dst]
        d_src, d_in_off, d_src_len = source(src)
        caps, d_out, d_out_off, _ = b.arena(torch, press, dst)
        d_len = torch.zeros(R, dtype=torch.int64, device=dev)
        d_sig = torch.zeros_like(b.sig)

        def rec(lib):
            def call():
                lib.ok(lib.l.press_hip_recode_batch(sid, did, p(d_src), p(d_in_off), p(d_src_len), p(b.d_n), p(b.d_off), R, total,
                                                    p(d_out), p(d_out_off), p(d_len), p(d_sig), p(d_outn), 1))
            return call

        def degraded():
            new.ok(new.l.press_hip_recode_degraded_batch(sid, did, BITS, p(d_src), p(d_in_off), p(d_src_len), p(b.d_n), p(b.d_off), R,
                                                         total, p(d_out), p(d_out_off), p(d_len), p(d_sig), p(d_outn), 1))

        def three_call():
            new.ok(new.l.press_hip_depress_batch(sid, p(d_src), p(d_in_off), p(d_src_len), R, p(d_sig), p(b.d_off), p(b.d_n), total,
                                                 p(d_outn), 1))
            new.ok(new.l.press_hip_degrade_batch(p(d_sig), p(b.d_off), p(b.d_n), R, total, BITS, p(d_sig), 1))
            new.ok(new.l.press_hip_press_batch(did, p(d_sig), p(b.d_off), p(b.d_n), R, total, p(d_out), p(d_out_off), p(d_len), 1))

        legs = ([("baseline", rec(base)), ("baseline2", rec(base))] if base else []) + \
            [("recode", rec(new)), ("degraded", degraded), ("three_call", three_call)]
        slot_off = d_out_off.cpu().numpy()
        got = {}
        for name, call in legs:  # warm-up and agreement
            d_out.zero_()
            d_len.zero_()
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            assert bool((d_outn.cpu().numpy() == b.n).all()), name
            lens = d_len.cpu().numpy()
            assert (lens > 0).all() and (lens < caps).all(), (name, "a read failed")
            host = d_out.cpu().numpy()
            got[name] = (lens.copy(), np.concatenate([host[int(o):int(o) + int(l)] for o, l in zip(slot_off[:-1], lens)]),
                         d_sig.cpu().numpy().copy())
        for x, y in (("degraded", "three_call"),) + ((("baseline", "recode"),) if base else ()):
            assert all(np.array_equal(u, v) for u, v in zip(got[x], got[y])), (x, "differs from", y)
        pair = {"fused": bool(press.recode_fused(src, dst)), "bits": BITS, "stream_bytes_undegraded": int(got["recode"][0].sum()),
                "stream_bytes_degraded": int(got["degraded"][0].sum()), "legs": {}}
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
            pair["legs"][name] = {"calls": int(ms.size), "mean_ms": float(ms.mean()), "median_ms": float(np.median(ms)),
                                  "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90))}
        lg = pair["legs"]
        pair["degraded_over_three_call"] = lg["degraded"]["median_ms"] / lg["three_call"]["median_ms"]
        if base:
            pair["baseline_spread_ms"] = abs(lg["baseline"]["median_ms"] - lg["baseline2"]["median_ms"])
            pair["degraded_over_baseline"] = lg["degraded"]["median_ms"] / lg["baseline"]["median_ms"]
            pair["recode_over_baseline"] = lg["recode"]["median_ms"] / lg["baseline"]["median_ms"]
        result["times"]["%s->%s" % (src, dst)] = pair
        del d_out
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
