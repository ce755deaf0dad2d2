#!/usr/bin/env python3
"""The per-read Huffman family (press_hip_huffman_press_batch / press_hip_huffman_depress_batch), device resident, on
bench.py's 8192-read batch, beside Rice, the fastest adaptive range coder and the static-Huffman path.

    python3 tools/dhuf_bench.py [--reads 8192] [--calls 5] [--out FILE]

Whole calls between two HIP events, all in one process on one card, the legs alternated (one call of every leg per round,
--calls rounds, the median of each): press and depress of huffman_vbe21_zd, rice_vbe21_zd, rccdf_vbe21_zd
(press_hip_rcf_*) and shuffman_vbe21_zd (the shipped table), press_hip_huffman_press_sizes, and the batch's longest read
alone under the per-read Huffman code and rccdf.  Per method also the compressed total and the ratio, the round trip of
every read, checked; for the per-read Huffman code the longest codes the reads chose and what the two repair rounds and
the serial walk had to touch (press_hip_huffman_repairs); and the ratios of huffman, rice and shuffman (shipped table)
on the same reads with 3 bits dropped (press_hip_degrade_batch), the Huffman round trip checked.
One JSON line.  "huffman_tenth": the per-read Huffman code takes at most a tenth of rccdf's time of the same run, in
both directions.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
METHODS = ("huffman_vbe21_zd", "rice_vbe21_zd", "rccdf_vbe21_zd", "shuffman_vbe21_zd")
REPAIRS = ("fix1_subsequences", "fix2_subsequences", "walk_values")


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
        sys.exit("dhuf_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    press.load_table()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R = b.R
    caps, d_out, d_out_off, d_in_off = b.arena(torch, press, "vbe21_zd")
    outs = {m: torch.empty_like(d_out) for m in METHODS}
    lens = {m: torch.zeros(R, dtype=torch.int64, device=dev) for m in METHODS}
    ml = torch.zeros(R, dtype=torch.uint8, device=dev)
    need = torch.zeros(R, dtype=torch.int64, device=dev)
    raw = torch.zeros(R, dtype=torch.uint8, device=dev)  # rccdf: the reads whose payload the coder stored (they do not come back)

    # the longest read alone: a batch of one read, its samples where they lie
    k = int(np.argmax(b.n))
    one_off, one_n = b.d_off[k:k + 1].contiguous(), b.d_n[k:k + 1].contiguous()
    one_out_off = torch.tensor([0, int(caps[k])], dtype=torch.int64, device=dev)
    ONE = (METHODS[0], METHODS[2])
    one_out = {m: torch.empty(int(caps[k]) + 64, dtype=torch.uint8, device=dev) for m in ONE}
    one_len = {m: torch.zeros(1, dtype=torch.int64, device=dev) for m in ONE}
    one_outn = torch.zeros(1, dtype=torch.int32, device=dev)

    def do_press(m, src, sig_off, n, out, out_off, ln, extra=None):
        if m.startswith("huffman"):
            press.huffman_press_batch("vbe21", src, sig_off, n, out, out_off, ln, extra)
        elif m.startswith("rice"):
            press.rice_press_batch("vbe21", src, sig_off, n, out, out_off, ln)
        elif m.startswith("rccdf"):
            press.rcf_press_batch("rccdf", "vbe21", src, sig_off, n, out, out_off, ln, raw if n is b.d_n else None)
        else:
            press.press_batch(m, src, sig_off, n, out, out_off, ln)

    def do_depress(m, comp, in_off, ln, sig_off, n, outn):
        if m.startswith("huffman"):
            press.huffman_depress_batch("vbe21", comp, in_off, ln, b.d_back, sig_off, n, outn)
        elif m.startswith("rice"):
            press.rice_depress_batch("vbe21", comp, in_off, ln, b.d_back, sig_off, n, outn)
        elif m.startswith("rccdf"):
            press.rcf_depress_batch("rccdf", "vbe21", comp, in_off, ln, b.d_back, sig_off, n, outn)
        else:
            press.depress_batch(m, comp, in_off, ln, b.d_back, sig_off, n, outn)

    legs = {}
    for m in METHODS:
        legs[m + "/press"] = lambda m=m: do_press(m, b.sig, b.d_off, b.d_n, outs[m], d_out_off, lens[m], ml if m.startswith("huffman") else None)
        legs[m + "/depress"] = lambda m=m: do_depress(m, outs[m], d_in_off, lens[m], b.d_off, b.d_n, b.d_outn)
    legs["huffman_vbe21_zd/sizes"] = lambda: press.huffman_press_sizes("vbe21", b.sig, b.d_off, b.d_n, need)
    for m in ONE:
        legs["longest_read/%s/press" % m] = lambda m=m: do_press(m, b.sig, one_off, one_n, one_out[m], one_out_off, one_len[m])
        legs["longest_read/%s/depress" % m] = lambda m=m: do_depress(m, one_out[m], one_out_off[:1], one_len[m], one_off, one_n, one_outn)

    result = {"reads": R, "samples": b.total_samples, "raw_bytes": b.raw_bytes, "calls": a.calls, "longest_read_samples": int(b.n[k]),
              "methods": {}}

    def round_trip(m, src, stored):
        got = b.d_outn.cpu().numpy().view(np.uint32)
        assert (got == b.n).all(), "%s: out_n" % m
        back = b.d_back.cpu().numpy()
        for r in np.flatnonzero(~stored):
            o, n1 = int(b.starts[r]), int(b.n[r])
            assert np.array_equal(back[o:o + n1], src[o:o + n1]), "%s: read %d does not come back" % (m, r)

    # warm-up, and what every leg makes: totals and the round trip
    sig = b.sig.cpu().numpy()
    for name, fn in legs.items():
        if name.endswith("depress"):
            b.d_back.zero_()
        fn()
        torch.cuda.synchronize()
        if name.startswith("longest_read"):
            m = name.split("/")[1]
            if name.endswith("press"):
                assert int(one_len[m][0]) != -1, name
            else:
                o, n1 = int(b.starts[k]), int(b.n[k])
                assert int(one_outn[0]) == n1 and np.array_equal(b.d_back[o:o + n1].cpu().numpy(), sig[o:o + n1]), name
                if m.startswith("huffman"):
                    result["longest_read_repairs"] = dict(zip(REPAIRS, press.huffman_repairs()))
            continue
        m, side = name.split("/")
        if side == "press":
            ln = lens[m].cpu().numpy().view(np.uint64)
            assert (ln != np.uint64(press.FAILED)).all(), "%s: a read failed" % m
            result["methods"][m] = {"compressed_bytes": int(ln.sum()), "ratio": b.raw_bytes / float(ln.sum())}
            if m.startswith("huffman"):
                result["maxlen_histogram"] = np.bincount(ml.cpu().numpy(), minlength=32).tolist()
        elif side == "sizes":
            assert np.array_equal(need.cpu().numpy(), lens[m].cpu().numpy()), "sizes differ from out_len"
        else:
            stored = raw.cpu().numpy().astype(bool) if m.startswith("rccdf") else np.zeros(R, dtype=bool)
            result["methods"][m]["reads_stored_raw"] = int(stored.sum())
            round_trip(m, sig, stored)
            if m.startswith("huffman"):
                result["repairs"] = dict(zip(REPAIRS, press.huffman_repairs()))

    ms = {name: [] for name in legs}
    for _ in range(a.calls):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    med = result["median_ms"] = {name: float(np.median(np.array(v))) for name, v in ms.items()}
    result["min_ms"] = {name: float(min(v)) for name, v in ms.items()}
    result["max_ms"] = {name: float(max(v)) for name, v in ms.items()}
    result["huffman_tenth"] = {side: med["huffman_vbe21_zd/" + side] * 10 <= med["rccdf_vbe21_zd/" + side] for side in ("press", "depress")}

    # the same reads with 3 bits dropped: no timing, the ratios and the per-read Huffman round trip
    dsig = torch.empty_like(b.sig)
    dsig.copy_(b.sig)
    press.degrade_batch(b.sig, b.d_off, b.d_n, 3, out=dsig)
    result["degraded_3_bits"] = {}
    for m in (METHODS[0], METHODS[1], METHODS[3]):
        do_press(m, dsig, b.d_off, b.d_n, outs[m], d_out_off, lens[m])
        torch.cuda.synchronize()
        ln = lens[m].cpu().numpy().view(np.uint64)
        assert (ln != np.uint64(press.FAILED)).all(), "%s: a degraded read failed" % m
        result["degraded_3_bits"][m] = {"compressed_bytes": int(ln.sum()), "ratio": b.raw_bytes / float(ln.sum())}
    b.d_back.zero_()
    do_depress(METHODS[0], outs[METHODS[0]], d_in_off, lens[METHODS[0]], b.d_off, b.d_n, b.d_outn)
    torch.cuda.synchronize()
    round_trip(METHODS[0] + " (degraded)", dsig.cpu().numpy(), np.zeros(R, dtype=bool))

    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
