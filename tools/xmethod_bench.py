#!/usr/bin/env python3
"""The families' methods in the generic calls (include/press_hip.h section 2w), device resident, on bench.py's 8192-read
batch: what one call saves over the two calls a caller needed before.

    python3 tools/xmethod_bench.py [--reads 8192] [--calls 5] [--out FILE]

Whole calls between two HIP events, all in one process on one card, the legs alternated (one call of every leg per round,
--calls rounds, the median of each), every result checked against its counterpart:

  recode/<form>/<dst>      press_hip_recode_batch / _sizes / _packed, slow5_svb_zd into huffman_vbe21_zd and rice_vbe21_zd
  two_calls/<form>/<dst>   press_hip_depress_batch, then the family's press / sizes call (packed: sizes, a scan of the
                           sizes on the device, press): the only route there was
  packed/<dst>             press_hip_press_packed of the samples
  sizes_press/<dst>        press_hip_{huffman, rice}_press_sizes, the scan, press_hip_{huffman, rice}_press_batch
  verify/<m>, chunks/<m>   press_hip_verify_batch and press_hip_depress_chunks_batch (T = 10000, overlap 500, float16) on
                           huffman_vbe21_zd beside shuffman_vbe21_zd (the shipped table): reported, not bounded

One JSON line.  "one_call_not_slower": per recode form and destination, median(recode) <= median(two_calls) + the two-call
route's own max - min; "packed_not_slower": the same for packed against sizes_press.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = "slow5_svb_zd"
DSTS = ("huffman_vbe21_zd", "rice_vbe21_zd")
FORMS = ("batch", "sizes", "packed")
T, OVERLAP = 10000, 500


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
        sys.exit("xmethod_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    press.load_table()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R = b.R
    total = b.sig.numel()

    def i64(k=R):
        return torch.zeros(k, dtype=torch.int64, device=dev)

    # the source streams, and shuffman's for the consumers
    _, s_out, s_out_off, s_in_off = b.arena(torch, press, SRC)
    s_len = i64()
    press.press_batch(SRC, b.sig, b.d_off, b.d_n, s_out, s_out_off, s_len)
    _, d_out, d_out_off, d_in_off = b.arena(torch, press, "vbe21_zd")
    h_out, h_len = torch.empty_like(d_out), i64()
    press.press_batch("shuffman_vbe21_zd", b.sig, b.d_off, b.d_n, h_out, d_out_off, h_len)
    torch.cuda.synchronize()
    assert bool((s_len != -1).all()) and bool((h_len != -1).all())

    family = {"huffman_vbe21_zd": (press.huffman_press_batch, press.huffman_press_sizes),
              "rice_vbe21_zd": (press.rice_press_batch, press.rice_press_sizes)}
    # what every leg writes: name -> (arena, out_off, out_len) or need
    res = {}
    for d in DSTS:
        for route in ("recode", "two_calls"):
            res[route, "batch", d] = (torch.empty_like(d_out), d_out_off, i64())
            res[route, "sizes", d] = i64()
            res[route, "packed", d] = (torch.empty_like(d_out), i64(R + 1), i64())
        res["packed", d] = (torch.empty_like(d_out), i64(R + 1), i64())
        res["sizes_press", d] = (torch.empty_like(d_out), i64(R + 1), i64())
    need_tmp = i64()

    def decode():
        press.depress_batch(SRC, s_out, s_in_off, s_len, b.d_back, b.d_off, b.d_n, b.d_outn)

    def sizes_scan_press(d, sig, slot):
        """the family's sizes, the layout on the device (align 1: an exclusive scan), the family's press"""
        out, out_off, out_len = slot
        fpress, fsizes = family[d]
        fsizes("vbe21", sig, b.d_off, b.d_n, need_tmp)
        out_off[0] = 0
        torch.cumsum(need_tmp, 0, out=out_off[1:])
        fpress("vbe21", sig, b.d_off, b.d_n, out, out_off, out_len)

    legs = {}
    for d in DSTS:
        out, oo, ol = res["recode", "batch", d]
        legs["recode/batch/" + d] = lambda d=d, out=out, oo=oo, ol=ol: press.recode_batch(
            SRC, d, s_out, s_in_off, s_len, b.d_n, b.d_off, out, oo, ol, b.d_outn, total_samples=total)
        out, oo, ol = res["two_calls", "batch", d]
        legs["two_calls/batch/" + d] = lambda d=d, out=out, oo=oo, ol=ol: (
            decode(), family[d][0]("vbe21", b.d_back, b.d_off, b.d_n, out, oo, ol))

        def recode_sizes(d=d):
            res["recode", "sizes", d] = press.recode_sizes(SRC, d, s_out, s_in_off, s_len, b.d_n, b.d_off, b.d_outn, total_samples=total)
        legs["recode/sizes/" + d] = recode_sizes
        legs["two_calls/sizes/" + d] = lambda d=d: (decode(), family[d][1]("vbe21", b.d_back, b.d_off, b.d_n, res["two_calls", "sizes", d]))
        out, oo, ol = res["recode", "packed", d]
        legs["recode/packed/" + d] = lambda d=d, out=out, oo=oo, ol=ol: press.recode_packed(
            SRC, d, s_out, s_in_off, s_len, b.d_n, b.d_off, out, oo, ol, b.d_outn, total_samples=total)
        legs["two_calls/packed/" + d] = lambda d=d: (decode(), sizes_scan_press(d, b.d_back, res["two_calls", "packed", d]))
        out, oo, ol = res["packed", d]
        legs["packed/" + d] = lambda d=d, out=out, oo=oo, ol=ol: press.press_packed(d, b.sig, b.d_off, b.d_n, out, oo, ol)
        legs["sizes_press/" + d] = lambda d=d: sizes_scan_press(d, b.sig, res["sizes_press", d])

    # the consumers: the per-read Huffman archive beside the static-Huffman one
    hx_out, hx_len = res["recode", "batch", DSTS[0]][0], res["recode", "batch", DSTS[0]][2]
    fb, vn, nbad = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (R, R, 1))
    row_first, _, _ = press.chunk_plan(b.n, T, OVERLAP)
    rows = torch.zeros((int(row_first[-1]), T), dtype=torch.float16, device=dev)
    d_row_first = torch.from_numpy(row_first.astype(np.int64)).to(dev)
    for m, (arena, ln) in (("huffman_vbe21_zd", (hx_out, hx_len)), ("shuffman_vbe21_zd", (h_out, h_len))):
        legs["verify/" + m] = lambda m=m, arena=arena, ln=ln: press.verify_batch(m, arena, d_in_off, ln, b.sig, b.d_off, b.d_n, fb, vn, nbad)
        legs["chunks/" + m] = lambda m=m, arena=arena, ln=ln: press.depress_chunks_batch(
            m, arena, d_in_off, ln, rows, d_row_first, b.d_off, b.d_n, total, vn, OVERLAP)

    def streams_equal(x, y, what):
        (xa, xo, xl), (ya, yo, yl) = x, y
        xl_, yl_ = xl.cpu().numpy(), yl.cpu().numpy()
        assert (xl_ != -1).all() and np.array_equal(xl_, yl_), what + ": out_len"
        xa_, ya_, xo_, yo_ = xa.cpu().numpy(), ya.cpu().numpy(), xo.cpu().numpy(), yo.cpu().numpy()
        for r in range(R):
            assert np.array_equal(xa_[xo_[r]:xo_[r] + xl_[r]], ya_[yo_[r]:yo_[r] + yl_[r]]), "%s: read %d" % (what, r)
        return int(xl_.sum())

    # warm-up and the checks
    rows_ref = None
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()
        kind = name.split("/")[0]
        if kind == "verify":
            assert int(nbad[0]) == 0 and bool((fb == -1).all()), name
        elif kind == "chunks":
            assert np.array_equal(vn.cpu().numpy().view(np.uint32), b.n), name
            got = rows.view(torch.int16).clone()
            assert rows_ref is None or bool((got == rows_ref).all()), "the rows differ between the two archives"
            rows_ref = got
    result = {"reads": R, "samples": b.total_samples, "raw_bytes": b.raw_bytes, "calls": a.calls, "compressed_bytes": {}}
    for d in DSTS:
        result["compressed_bytes"][d] = streams_equal(res["recode", "batch", d], res["two_calls", "batch", d], "recode_batch " + d)
        streams_equal(res["recode", "packed", d], res["two_calls", "packed", d], "recode_packed " + d)
        streams_equal(res["recode", "packed", d], res["recode", "batch", d], "recode_packed against recode_batch " + d)
        streams_equal(res["packed", d], res["sizes_press", d], "press_packed " + d)
        streams_equal(res["packed", d], res["recode", "batch", d], "press_packed against recode_batch " + d)
        need = res["recode", "sizes", d].cpu().numpy()
        assert np.array_equal(need, res["two_calls", "sizes", d].cpu().numpy()), "recode_sizes " + d
        assert np.array_equal(need, res["recode", "batch", d][2].cpu().numpy()), "recode_sizes against out_len " + d
        oo = res["recode", "packed", d][1].cpu().numpy()
        assert oo[0] == 0 and np.array_equal(np.diff(oo), need), "the packed arena has a gap " + d

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

    def not_slower(new, old):
        return med[new] <= med[old] + (result["max_ms"][old] - result["min_ms"][old])
    result["one_call_not_slower"] = {"%s/%s" % (f, d): not_slower("recode/%s/%s" % (f, d), "two_calls/%s/%s" % (f, d)) for f in FORMS for d in DSTS}
    result["packed_not_slower"] = {d: not_slower("packed/" + d, "sizes_press/" + d) for d in DSTS}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
