#!/usr/bin/env python3
"""The range-coder family (press_hip_rcf_press_batch / press_hip_rcf_depress_batch), device resident, on bench.py's
8192-read batch.

    python3 tools/rcf_bench.py [--reads 8192] [--calls 5] [--out FILE]

Whole calls between two HIP events, all in one process on one card, the legs alternated (one call of every leg per round,
--calls rounds, the median of each): press and depress of every coder on vbe21, of rccdf and rccm on vbbe21, and - the
adaptive coders are set by the longest read - the batch's longest read alone, per coder, on vbe21.  Per leg also the
compressed total, the ratio, the reads whose payload the coder stored raw (raw[], counted on the device) and the round
trip of every other read, checked.  One JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIRS = [("rc", "vbe21"), ("rcc", "vbe21"), ("rccm", "vbe21"), ("rccdf", "vbe21"), ("rccdf", "vbbe21"), ("rccm", "vbbe21")]


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
        sys.exit("rcf_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R = b.R
    caps, d_out, d_out_off, d_in_off = b.arena(torch, press, "vbe21_zd")
    out_off = d_out_off.cpu().numpy()
    raw = torch.zeros(R, dtype=torch.uint8, device=dev)
    outs = {p: torch.empty_like(d_out) for p in PAIRS}
    lens = {p: torch.zeros(R, dtype=torch.int64, device=dev) for p in PAIRS}

    # the longest read alone: a batch of one read, its samples where they lie
    k = int(np.argmax(b.n))
    one_off, one_n = b.d_off[k:k + 1].contiguous(), b.d_n[k:k + 1].contiguous()
    one_out_off = torch.tensor([0, int(caps[k])], dtype=torch.int64, device=dev)
    one_out = {c: torch.empty(int(caps[k]) + 64, dtype=torch.uint8, device=dev) for c in press.RCF_CODERS}
    one_len = {c: torch.zeros(1, dtype=torch.int64, device=dev) for c in press.RCF_CODERS}
    one_outn = torch.zeros(1, dtype=torch.int32, device=dev)

    legs = {}
    for p in PAIRS:
        c, l = p
        legs["%s_%s_zd/press" % p] = lambda p=p, c=c, l=l: press.rcf_press_batch(c, l, b.sig, b.d_off, b.d_n, outs[p], d_out_off, lens[p], raw)
        legs["%s_%s_zd/depress" % p] = lambda p=p, c=c, l=l: press.rcf_depress_batch(c, l, outs[p], d_in_off, lens[p], b.d_back, b.d_off,
                                                                                     b.d_n, b.d_outn)
    for c in press.RCF_CODERS:
        legs["longest_read/%s/press" % c] = lambda c=c: press.rcf_press_batch(c, "vbe21", b.sig, one_off, one_n, one_out[c], one_out_off,
                                                                              one_len[c], None)
        legs["longest_read/%s/depress" % c] = lambda c=c: press.rcf_depress_batch(c, "vbe21", one_out[c], one_out_off[:1], one_len[c],
                                                                                  b.d_back, one_off, one_n, one_outn)

    result = {"reads": R, "samples": b.total_samples, "raw_bytes": b.raw_bytes, "calls": a.calls, "longest_read_samples": int(b.n[k]),
              "methods": {}}
    # warm-up, and what every leg makes: totals, stored reads, the round trip
    sig = b.sig.cpu().numpy()
    for name, fn in legs.items():
        if name.endswith("depress"):
            b.d_back.zero_()
        fn()
        torch.cuda.synchronize()
        if name.startswith("longest_read"):
            c = name.split("/")[1]
            if name.endswith("press"):
                assert int(one_len[c][0]) != -1, name
            else:
                o, kk = int(b.starts[k]), int(b.n[k])
                assert int(one_outn[0]) == kk and np.array_equal(b.d_back[o:o + kk].cpu().numpy(), sig[o:o + kk]), name
            continue
        m, side = name.split("/")
        p = [q for q in PAIRS if "%s_%s_zd" % q == m][0]
        if side == "press":
            ln = lens[p].cpu().numpy().view(np.uint64)
            assert (ln != np.uint64(press.FAILED)).all(), "%s: a read failed" % m
            stored = raw.cpu().numpy().astype(bool)
            result["methods"][m] = {"compressed_bytes": int(ln.sum()), "ratio": b.raw_bytes / float(ln.sum()),
                                    "reads_stored_raw": int(stored.sum()), "stored": stored}
        else:
            got = b.d_outn.cpu().numpy().view(np.uint32)
            assert (got == b.n).all(), "%s: out_n" % m
            back = b.d_back.cpu().numpy()
            stored = result["methods"][m].pop("stored")
            for r in np.flatnonzero(~stored):
                o, kk = int(b.starts[r]), int(b.n[r])
                assert np.array_equal(back[o:o + kk], sig[o:o + kk]), "%s: read %d does not come back" % (m, r)

    ms = {name: [] for name in legs}
    for _ in range(a.calls):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    result["median_ms"] = {name: float(np.median(np.array(v))) for name, v in ms.items()}
    result["min_ms"] = {name: float(min(v)) for name, v in ms.items()}
    result["max_ms"] = {name: float(max(v)) for name, v in ms.items()}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
