#!/usr/bin/env python3
"""The stall methods (press_hip_stall_press_batch / press_hip_stall_depress_batch), device resident, on bench.py's
8192-read batch.

    python3 tools/stall_bench.py [--reads 8192] [--calls 5] [--legs all|family|generic] [--out FILE]

Whole calls between two HIP events.  Per stall method: the median press and depress times, the compressed total and ratio,
the share of reads whose stream has a stall, the round trip checked.  In the same process and with the legs alternated
(one call of every leg per round, --calls rounds): press_hip_press_batch / press_hip_depress_batch of rccm_vbbe21_zd, the
coder the stall methods are made of, and press_hip_signal_segments (cDNA preset) as a pure count, the segment pass.
"sums" holds what the parts add up to: rccm_vbbe21_zd + the segment pass for rccm_svbbe21_zd and dstall_fz_1500, twice the
coder + the segment pass for dstall_fz; "spread_ms" is the largest max - min of any leg over the rounds.  One JSON line.

The generic calls with dstall_fz's method id (include/press_hip.h 2x), each against the route a caller had without it
("generic": medians in "median_ms", bytes in "generic"):
  recode_packed         press_hip_recode_packed(slow5_svb_zd -> dstall_fz) into an arena of the streams' own size, against
  route_today           press_hip_depress_batch, press_hip_stall_press_batch into press_hip_stall_bound slots and a torch gather
                        of the streams into a dense arena; arena bytes of both
  press_sizes           press_hip_press_sizes(dstall_fz), against dstall_fz/press (press_hip_stall_press_batch)
  verify_batch          press_hip_verify_batch(dstall_fz), against depress_equal: press_hip_stall_depress_batch and torch.equal
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INNER = "rccm_vbbe21_zd"


def stored_raw(piece, n):
    """a [u16][u32 nex][vbbe21 section][coded one-byte values] piece of n values behind the u16 whose coder gave up and
    stored the one-byte values raw (rcutil_.h:161): nothing tells a decoder so, the reference's included - such a stream
    is outside the format's lossless domain"""
    nex = int.from_bytes(piece[2:6], "little")
    sec = 4
    if nex > 1:
        sec += 4 + int.from_bytes(piece[2 + sec:6 + sec], "little")
        sec += 4 + int.from_bytes(piece[2 + sec:6 + sec], "little")
    elif nex == 1:
        sec += 6
    nlow = n - nex
    return nlow > 0 and len(piece) - 2 - sec == nlow


def raw_piece(stream, n):
    """does a stall-method stream of a read of n samples hold a piece stored raw?"""
    pos, sl = 1, 0
    if stream[0]:
        sl = int.from_bytes(stream[3:5], "little")
        l1 = int.from_bytes(stream[5:7], "little")
        if stored_raw(stream[7:7 + l1], sl):
            return True
        pos = 7 + l1
    l0 = int.from_bytes(stream[pos:pos + 4], "little")
    return stored_raw(stream[pos + 4:pos + 4 + l0], n - sl - 1)


def generic_legs(torch, press, b, legs, outs, lens, d_out_off, d_in_off):
    """the legs of the generic calls with dstall_fz's id and of the routes they replace -> {name: fn}, "_bytes": the arena
    figures, "_check": what the warm-up must have left"""
    m, src = "dstall_fz", "slow5_svb_zd"
    dev, R, total = b.dev, b.R, b.sig.numel()
    # the BLOW5 fields of the batch
    _, s_out, s_off, s_in = b.arena(torch, press, src)
    s_len = torch.zeros(R, dtype=torch.int64, device=dev)
    press.press_batch(src, b.sig, b.d_off, b.d_n, s_out, s_off, s_len)
    # the generic route: the arena is as large as the streams (press_hip_recode_sizes says how large)
    outn = torch.zeros(R, dtype=torch.int32, device=dev)
    need = press.recode_sizes(src, m, s_out, s_in, s_len, b.d_n, b.d_off, outn, total_samples=total)
    torch.cuda.synchronize()
    assert bool((need > 0).all())
    packed_bytes = int(need.sum())
    p_out = torch.empty(packed_bytes, dtype=torch.uint8, device=dev)
    p_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    p_len = torch.zeros(R, dtype=torch.int64, device=dev)
    # the route without it: samples, slots of press_hip_stall_bound bytes, a gather
    caps = np.array([press.stall_bound(m, int(x)) for x in b.n], dtype=np.int64)
    t_off_h = np.concatenate([[0], np.cumsum(caps)])
    t_out = torch.empty(int(t_off_h[-1]) + 64, dtype=torch.uint8, device=dev)
    t_off = torch.from_numpy(t_off_h).to(dev)
    t_len = torch.zeros(R, dtype=torch.int64, device=dev)
    dense = {}

    def route_today():
        press.depress_batch(src, s_out, s_in, s_len, b.d_back, b.d_off, b.d_n, b.d_outn)
        press.stall_press_batch(m, b.d_back, b.d_off, b.d_n, t_out, t_off, t_len, None)
        ends = torch.cumsum(t_len, 0)
        shift = torch.repeat_interleave(t_off[:-1] - (ends - t_len), t_len)  # (the sum of t_len: a device-to-host read)
        dense["out"] = t_out[torch.arange(shift.numel(), device=dev) + shift]
        dense["off"] = ends - t_len

    fb, von, nbad = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (R, R, 1))
    same = {}

    def depress_equal():
        press.stall_depress_batch(outs[m], d_in_off, lens[m], b.d_back, b.d_off, b.d_n, b.d_outn)
        same["ok"] = torch.equal(b.d_back, b.sig) and torch.equal(b.d_outn, b.d_n)

    def check():
        assert int(p_off[-1]) == packed_bytes == dense["out"].numel(), "the two routes' arenas differ"
        assert torch.equal(p_off[:-1], dense["off"]) and torch.equal(p_len, t_len) and torch.equal(p_out, dense["out"])
        assert torch.equal(sizes["need"], lens[m]) and torch.equal(need, p_len)
        assert int(nbad[0]) == 0 and bool((fb == -1).all()) and same["ok"]

    sizes = {}
    return {"recode_packed": lambda: press.recode_packed(src, m, s_out, s_in, s_len, b.d_n, b.d_off, p_out, p_off, p_len, outn,
                                                         total_samples=total),
            "route_today": route_today,
            "press_sizes": lambda: sizes.__setitem__("need", press.press_sizes(m, b.sig, b.d_off, b.d_n)),
            "verify_batch": lambda: press.verify_batch(m, outs[m], d_in_off, lens[m], b.sig, b.d_off, b.d_n, fb, von, nbad),
            "depress_equal": depress_equal,
            "_check": check,
            "_bytes": {"source_bytes": int(s_len.sum()), "recode_packed_arena_bytes": packed_bytes,
                       "route_today_arena_bytes": int(t_off_h[-1]) + packed_bytes, "route_today_slot_bytes": int(t_off_h[-1])}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--legs", choices=("all", "family", "generic"), default="all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("stall_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    # slots of 4 n + 1024 bytes: a stall piece rich in exceptions takes a stream past the reference's bound of 2 n + 3
    caps = (4 * b.n.astype(np.int64) + 1024 + 127) // 128 * 128
    out_off = np.concatenate([[0], np.cumsum(caps)])
    d_out = torch.empty(int(out_off[-1]) + 64, dtype=torch.uint8, device=dev)
    d_out_off = torch.from_numpy(out_off).to(dev)
    d_in_off = d_out_off[:-1].contiguous()
    stall = torch.zeros(2 * R, dtype=torch.int32, device=dev)
    lens = {m: torch.zeros(R, dtype=torch.int64, device=dev) for m in list(press.STALL_METHODS) + [INNER]}
    outs = {m: torch.empty_like(d_out) for m in press.STALL_METHODS}
    outs[INNER] = d_out
    first = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(R, dtype=torch.int32, device=dev)
    prm = press.jnn_params("cdna")

    legs = {"segments_count": lambda: press.signal_segments(b.sig, b.d_off, b.d_n, None, prm, None, first, count, None),
            INNER + "/press": lambda: press.press_batch(INNER, b.sig, b.d_off, b.d_n, d_out, d_out_off, lens[INNER]),
            INNER + "/depress": lambda: press.depress_batch(INNER, d_out, d_in_off, lens[INNER], b.d_back, b.d_off, b.d_n, b.d_outn)}
    for m in press.STALL_METHODS:
        legs[m + "/press"] = lambda m=m: press.stall_press_batch(m, b.sig, b.d_off, b.d_n, outs[m], d_out_off, lens[m], stall)
        legs[m + "/depress"] = lambda m=m: press.stall_depress_batch(outs[m], d_in_off, lens[m], b.d_back, b.d_off, b.d_n, b.d_outn)

    if a.legs == "generic":  # (what the generic legs are compared with stays)
        legs = {k: v for k, v in legs.items() if k in ("dstall_fz/press", "dstall_fz/depress")}
    generic = {}
    if a.legs != "family":
        generic = generic_legs(torch, press, b, legs, outs, lens, d_out_off, d_in_off)

    result = {"reads": R, "samples": b.total_samples, "raw_bytes": b.raw_bytes, "calls": a.calls,
              "workspace_bytes": {m: press.stall_workspace_bytes(m, total, R) for m in press.STALL_METHODS}, "methods": {}}
    result["workspace_bytes"][INNER] = int(press.load_library().press_hip_workspace_bytes(press.METHODS[INNER], total, R))

    # warm-up, and what every leg makes: totals, shares, the round trip.  rccm_svbbe21_zd and dstall_fz_1500 REFUSE a read
    # whose stall piece passes 65535 bytes (include/press_hip.h, definition 2): such reads are counted, left out of the
    # totals, and handed to the decoder as streams of no bytes, which it refuses
    nn = b.n.astype(np.int64)
    for name, fn in legs.items():
        m, _, side = name.partition("/")
        if side == "depress":
            b.d_back.zero_()
        fn()
        torch.cuda.synchronize()
        if side == "press":
            ln = lens[m].cpu().numpy().view(np.uint64)
            ok = ln != np.uint64(press.FAILED)
            assert ok.all() or m in ("rccm_svbbe21_zd", "dstall_fz_1500"), "%s: %d reads failed" % (m, int((~ok).sum()))
            raw = 2 * int(nn[ok].sum())
            row = {"refused_reads": int((~ok).sum()), "raw_bytes": raw, "compressed_bytes": int(ln[ok].sum()),
                   "ratio": raw / float(ln[ok].sum())}
            if m != INNER:
                st = stall.cpu().numpy().view(np.uint32).reshape(-1, 2)
                row["reads_with_stall"] = int((st[:, 1] > 0).sum())
                row["share_with_stall"] = float((st[:, 1] > 0).mean())
                row["stall_samples"] = int(st[:, 1].sum())
            result["methods"][m] = row
            lens[m].masked_fill_(lens[m] == -1, 0)
        elif side == "depress":
            ok = (lens[m] != 0).cpu().numpy()
            got = b.d_outn.cpu().numpy().view(np.uint32)
            assert (got[ok] == b.n[ok]).all() and (got[~ok] == 0xFFFFFFFF).all(), "%s: out_n" % m
            # every read comes back, but for those with a piece the coder stored raw (counted; dstall_fz has none on
            # this batch: a raw piece makes the stall form the longer one)
            back, sig = b.d_back.cpu().numpy(), b.sig.cpu().numpy()
            arena, ln = outs[m].cpu().numpy(), lens[m].cpu().numpy()
            lost = 0
            for r in np.flatnonzero(ok):
                o, k = int(b.starts[r]), int(b.n[r])
                if not np.array_equal(back[o:o + k], sig[o:o + k]):
                    stream = arena[int(out_off[r]):int(out_off[r]) + int(ln[r])].tobytes()
                    assert m != INNER and raw_piece(stream, k), "%s: read %d does not come back" % (m, r)
                    lost += 1
            result["methods"][m]["reads_with_a_raw_piece_not_given_back"] = lost

    if generic:
        result["generic"] = generic.pop("_bytes")
        for name, fn in generic.items():  # warm-up: every buffer reserved, the results checked
            fn()
            torch.cuda.synchronize()
        generic.pop("_check")()
        legs.update(generic)
    ms = {name: [] for name in legs}
    for _ in range(a.calls):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    med = {name: float(np.median(np.array(v))) for name, v in ms.items()}
    result["median_ms"] = med
    result["spread_ms"] = max(float(max(v) - min(v)) for v in ms.values())
    if a.legs != "generic":
        seg = med["segments_count"]
        result["sums"] = {"rccm_svbbe21_zd/press": med[INNER + "/press"] + seg, "dstall_fz_1500/press": med[INNER + "/press"] + seg,
                          "dstall_fz/press": 2 * med[INNER + "/press"] + seg,
                          "depress": med[INNER + "/depress"]}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
