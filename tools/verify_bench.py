#!/usr/bin/env python3
"""The verify calls against what a caller could do before they existed, device resident, on bench.py's 8192-read batch.

    python3 tools/verify_bench.py [--reads 8192] [--seconds 1.0] [--out FILE]

Routes, all from the same samples and the same compressed streams:

  crc      press_hip_signal_crc32 over the batch's samples
  sym      press_hip_symbol_counts over the same samples: the library's other read-once pass over int16 samples
  and per method (slow5_svb_zd, shuffman_vbe21_zd):
  verify   press_hip_verify_batch
  dcrc     press_hip_depress_crc_batch
  dep      press_hip_depress_batch into a caller's int16 tensor
  dep_eq   ... plus one torch.equal over the arena: the cheapest check the parent commit offers - it says yes or no, not
           which read or where, and needs a second full-size int16 arena

The routes alternate block by block in one process after a warm-up; HIP events around every whole call, at least
--seconds of timed calls and at least 20 calls per route.  Before anything is timed the results are compared for
equality: crc[] with zlib.crc32 of every read on the host, dcrc's crc[] with the same numbers, verify's nbad with 0 and
first_bad[] with PRESS_HIP_VERIFIED, the decoded arena with the samples.  One JSON line: per route calls, median, p10, p90,
and for crc the implied GB/s over the samples' bytes.
"""
import argparse
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
METHODS = ["slow5_svb_zd", "shuffman_vbe21_zd"]


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
        sys.exit("verify_bench needs a GPU")
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
    h_sig = b.sig.cpu().numpy()
    h_off = b.d_off.cpu().numpy()
    want_crc = np.array([zlib.crc32(h_sig[int(o):int(o) + int(n)].tobytes()) for o, n in zip(h_off, b.n)], dtype=np.uint32)

    d_crc = torch.zeros(R, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(257, dtype=torch.int64, device=dev)
    legs = [("crc", lambda: press.signal_crc32(b.sig, b.d_off, b.d_n, d_crc)),
            ("sym", lambda: press.symbol_counts(b.sig, b.d_off, b.d_n, d_counts))]
    legs[0][1]()
    torch.cuda.synchronize()
    assert np.array_equal(d_crc.cpu().numpy().view(np.uint32), want_crc), "signal_crc32 differs from zlib.crc32"

    keep = []
    for m in METHODS:
        mid = press.METHODS[m]
        _, d_src, d_src_off, d_in_off = b.arena(torch, press, m)
        d_len = torch.zeros(R, dtype=torch.int64, device=dev)
        ok(lib.press_hip_press_batch(mid, p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_src), p(d_src_off), p(d_len), 1))
        d_outn = torch.zeros(R, dtype=torch.int32, device=dev)
        d_fb = torch.zeros(R, dtype=torch.int32, device=dev)
        d_nbad = torch.zeros(1, dtype=torch.int32, device=dev)
        d_c2 = torch.zeros(R, dtype=torch.int32, device=dev)
        d_sig = torch.zeros_like(b.sig)
        keep.append((d_src, d_len, d_outn, d_fb, d_nbad, d_c2, d_sig))

        def verify(m=m, d_src=d_src, d_in_off=d_in_off, d_len=d_len, d_fb=d_fb, d_outn=d_outn, d_nbad=d_nbad):
            press.verify_batch(m, d_src, d_in_off, d_len, b.sig, b.d_off, b.d_n, d_fb, d_outn, d_nbad)

        def dcrc(m=m, d_src=d_src, d_in_off=d_in_off, d_len=d_len, d_c2=d_c2, d_outn=d_outn):
            press.depress_crc_batch(m, d_src, d_in_off, d_len, b.d_off, b.d_n, total, d_c2, d_outn)

        def dep(m=m, d_src=d_src, d_in_off=d_in_off, d_len=d_len, d_sig=d_sig, d_outn=d_outn):
            press.depress_batch(m, d_src, d_in_off, d_len, d_sig, b.d_off, b.d_n, d_outn)

        def dep_eq(dep=dep, d_sig=d_sig):
            dep()
            if not torch.equal(d_sig, b.sig):
                raise RuntimeError("the decoded arena differs")

        for name, call in (("verify", verify), ("dcrc", dcrc), ("dep", dep), ("dep_eq", dep_eq)):
            legs.append((m + "/" + name, call))
        verify()
        dcrc()
        dep()
        torch.cuda.synchronize()
        assert int(d_nbad.item()) == 0 and bool((d_fb == -1).all()), (m, "verify_batch reports a difference")
        assert np.array_equal(d_c2.cpu().numpy().view(np.uint32), want_crc), (m, "depress_crc_batch differs from zlib.crc32")
        assert bool((d_outn.cpu().numpy() == b.n).all()) and torch.equal(d_sig, b.sig), m

    for _, call in legs:  # warm-up
        for _ in range(3):
            call()
    torch.cuda.synchronize()
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
    result = {"reads": R, "samples": b.total_samples, "legs": {}}
    for name, ms in times.items():
        ms = np.array(ms)
        result["legs"][name] = {"calls": int(ms.size), "median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)),
                                "p90_ms": float(np.percentile(ms, 90))}
    Lg = result["legs"]
    result["crc_GBps"] = 2.0 * b.total_samples / (Lg["crc"]["median_ms"] / 1000.0) / 1e9
    result["crc_over_sym"] = Lg["crc"]["median_ms"] / Lg["sym"]["median_ms"]
    result["crc_over_dep_shuffman"] = Lg["crc"]["median_ms"] / Lg["shuffman_vbe21_zd/dep"]["median_ms"]
    for m in METHODS:
        result[m + "/verify_over_dep_eq"] = Lg[m + "/verify"]["median_ms"] / Lg[m + "/dep_eq"]["median_ms"]
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
