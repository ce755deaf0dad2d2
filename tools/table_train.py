"""Fitting a Huffman table on the GPU: what it costs and what it buys.

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/table_train.py [--out FILE.json]

* the counting pass (press_hip_symbol_counts, device-resident) on bench.py's default 8192-read batch: HIP-event
  time of the call (memset + k_train_prep + k_symbol_count; the kernel's own time is in the rocprofv3 stats) and
  bytes/s against the 2n bytes of samples; the counts must be the same on every run;
* a batch with shifted statistics (the deltas of synthetic reads x 1.5): a table fitted to it against the
  NA12878 table - bytes and press / depress MB/s of shuffman_vbe21_zd (device-resident batch calls);
* whether the fitted table needs the decoder's trie (HUF_NEEDS_TRIE: a long code whose first 12 bits get no
  second-level table, the rule of upload_table in press_table.hip).
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LUT_BITS, L2_IDS, L2_ENTRIES = 12, 64, 3072  # press_internal.h


def needs_trie(ln, bits):
    """HUF_NEEDS_TRIE as upload_table decides it"""
    ids, depth = {}, {}
    for s in range(256):
        if ln[s] <= LUT_BITS:
            continue
        p = int(bits[s]) & ((1 << LUT_BITS) - 1)
        if p not in ids and len(ids) < L2_IDS:
            ids[p] = len(ids)
        if p in ids:
            depth[p] = max(depth.get(p, 0), int(ln[s]) - LUT_BITS)
    if any(s_ln > LUT_BITS and (int(bits[s]) & ((1 << LUT_BITS) - 1)) not in ids for s, s_ln in enumerate(ln)):
        return True
    used, placed = 0, set()
    for d in range(32, 0, -1):
        for p in ids:  # (insertion order = id order)
            if depth[p] != d or d > 12 or used + (1 << d) > L2_ENTRIES:
                continue
            placed.add(p)
            used += 1 << d
    return used > L2_ENTRIES - 1 or len(placed) < len(ids)


def scaled(reads, f):
    """every delta multiplied by f, rounded half away from zero (as tests/test_table_training.py)"""
    out = []
    for r in reads:
        d = np.diff(r.astype(np.int64)).astype(np.float64) * f
        h = (np.sign(d) * np.floor(np.abs(d) + 0.5)).astype(np.int64)
        s = np.concatenate([[int(r[0])], int(r[0]) + np.cumsum(h)])
        out.append(s.astype(np.int64).astype(np.uint16).view(np.int16))
    return out


def timed(torch, fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return ms


def device_batch(torch, reads, dev):
    ns = np.array([len(r) for r in reads], dtype=np.int64)
    pad = (ns + 63) // 64 * 64
    off = np.zeros(len(reads), dtype=np.int64)
    off[1:] = np.cumsum(pad)[:-1]
    sig = np.zeros(int(pad.sum()) + 64, dtype=np.int16)
    for r, o in zip(reads, off):
        sig[o:o + len(r)] = r
    return (torch.from_numpy(sig).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(ns.astype(np.int32)).to(dev),
            int(ns.sum()))


def press_depress(torch, press, m, sig, d_off, d_n, ns, reps):
    caps = np.array([press.bound(m, int(x)) for x in ns], dtype=np.int64)
    caps = (caps + 64 + 127) // 128 * 128
    out_off = np.concatenate([[0], np.cumsum(caps)])
    d_out = torch.empty(int(out_off[-1]) + 64, dtype=torch.uint8, device=sig.device)
    d_out_off = torch.from_numpy(out_off).to(sig.device)
    d_in_off = d_out_off[:-1].contiguous()
    d_len = torch.zeros(len(ns), dtype=torch.int64, device=sig.device)
    back = torch.zeros_like(sig)
    outn = torch.zeros(len(ns), dtype=torch.int32, device=sig.device)
    pf = lambda: press.press_batch(m, sig, d_off, d_n, d_out, d_out_off, d_len)
    df = lambda: press.depress_batch(m, d_out, d_in_off, d_len, back, d_off, d_n, outn)
    for _ in range(2):
        pf()
        df()
    tp = timed(torch, pf, reps)
    td = timed(torch, df, reps)
    lens = d_len.cpu().numpy()
    ok = bool((lens >= 0).all()) and torch.equal(outn, d_n) and torch.equal(back, sig)
    return {"bytes": int(lens.sum()), "press_ms": float(np.median(tp)), "depress_ms": float(np.median(td)),
            "lossless": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261004)  # bench.py's default
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--shifted-reads", type=int, default=1024)
    ap.add_argument("--scale", type=float, default=1.5, help="delta scale of the shifted batch")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from honours_amd import press, synth

    assert torch.cuda.is_available(), "table_train.py needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    press.load_library()
    press.use_torch_stream()
    res = {}

    # ---- counting on bench.py's batch
    sig, starts, n = synth.synth_batch_torch(args.seed, 0, args.reads, dev, align=64)
    sig = torch.cat([sig, torch.zeros(64, dtype=torch.int16, device=dev)])
    d_off = torch.from_numpy(starts[:-1].astype(np.int64)).to(dev)
    d_n = torch.from_numpy(n.astype(np.int32)).to(dev)
    total = int(n.sum())
    counts = torch.zeros(press.NBINS, dtype=torch.int64, device=dev)

    def count():
        counts.zero_()
        press.symbol_counts(sig, d_off, d_n, counts)

    count()
    torch.cuda.synchronize()
    first = counts.clone()
    ms = timed(torch, count, args.reps)
    same = bool(torch.equal(first, counts))
    c = first.cpu().numpy().view(np.uint64)
    res["count"] = {"reads": args.reads, "samples": total, "bytes": 2 * total,
                    "call_ms_median": float(np.median(ms)), "call_ms_min": float(np.min(ms)),
                    "GBps_vs_2n_bytes": 2 * total / (float(np.median(ms)) * 1e-3) / 1e9,
                    "deterministic": same, "deltas_counted": int(c.sum()), "exceptions": int(c[256])}
    del sig, counts

    # ---- the shifted batch: fitted table vs NA12878's
    host, off = synth.synth_batch(args.seed + 1, 0, args.shifted_reads)
    reads = scaled([host[int(off[k]):int(off[k + 1])] for k in range(args.shifted_reads)], args.scale)
    del host
    path = os.path.join(tempfile.mkdtemp(), "fitted.huffman")
    fc = press.train_table(reads, path)
    ln, bits = press.table_from_counts(fc)
    d_sig, d_off2, d_n2, tot2 = device_batch(torch, reads, dev)
    ns = np.array([len(r) for r in reads])
    m = "shuffman_vbe21_zd"
    out = {"reads": len(reads), "samples": tot2, "delta_scale": args.scale, "max_code_bits": int(ln.max()),
           "zero_count_values": int((fc[:256] == 0).sum()), "fitted_needs_trie": needs_trie(ln, bits)}
    for name, p in (("na12878", press.TABLE_PATH), ("fitted", path)):
        press.use_table(p)
        r = press_depress(torch, press, m, d_sig, d_off2, d_n2, ns, args.reps)
        r["press_MBps"] = 2 * tot2 / (r["press_ms"] * 1e-3) / 1e6
        r["depress_MBps"] = 2 * tot2 / (r["depress_ms"] * 1e-3) / 1e6
        out[name] = r
    press.use_table()
    na_ln = np.array([x[0] for x in _na_lengths(press)])
    out["na12878_needs_trie"] = needs_trie(na_ln, [x[1] for x in _na_lengths(press)])
    out["fitted_over_na12878_bytes"] = out["fitted"]["bytes"] / out["na12878"]["bytes"]
    res["shifted"] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


def _na_lengths(press):
    freq = json.load(open(os.path.join(ROOT, "honours_amd", "data", "NA12878_zd_freq.json")))["freq"]
    ln, bits = press.table_from_counts(freq)
    return list(zip(ln.tolist(), bits.tolist()))


if __name__ == "__main__":
    main()
