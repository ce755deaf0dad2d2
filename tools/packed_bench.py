#!/usr/bin/env python3
"""press_hip_press_packed / press_hip_press_sizes against press_hip_press_batch, device resident, on bench.py's 8192-read
batch.

    python3 tools/packed_bench.py [--reads 8192] [--baseline-lib PATH] [--seconds 0.5] [--once] [--out FILE]

Legs, per method (svb12_zd, vbe21_zd, shuffman_vbe21_zd, zstd_svb_zd), alternated call block by call block within this
one process after a warm-up, HIP events around every whole call, at least --seconds of timed calls per leg:

  baseline     press_hip_press_batch of --baseline-lib into bench.py's slot arena (a libpress_hip.so built from the
               parent commit: the yardstick), and the same leg a second time (baseline2) for the run-to-run spread
  press_batch  the same call of this build (a cross-check, never the yardstick)
  packed1      press_hip_press_packed, align = 1
  packed16     press_hip_press_packed, align = 16
  sizes        press_hip_press_sizes
  dec_baseline / dec_baseline2   press_hip_depress_batch of the baseline library on the slot arena
  dec_packed1 / dec_packed16     press_hip_depress_batch of this build on the packed arenas

A packed leg "costs nothing" only where |leg - baseline| is inside |baseline - baseline2|.  Also recorded, as exact
counts: the arena bytes of every layout (out_off[nreads]) against the sum of press_hip_bound and against bench.py's
slot arena.  Before anything is timed every packed stream is compared with the slot arena's.  --once: one call per leg
and no timing.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
METHODS = ["svb12_zd", "vbe21_zd", "shuffman_vbe21_zd", "zstd_svb_zd"]


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
    ap.add_argument("--block", type=int, default=8, help="calls of one leg before the next leg's turn")
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("packed_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    new = Lib(press.LIB_PATH, torch, press.TABLE_PATH)
    base = Lib(a.baseline_lib, torch, press.TABLE_PATH) if a.baseline_lib else None
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R, total = b.R, b.sig.numel()
    p = lambda t: t.data_ptr()
    result = {"reads": R, "samples": b.total_samples, "methods": {}}
    for m in a.methods.split(","):
        mid = press.METHODS[m]
        caps, d_slots, d_slot_off, d_slot_in = b.arena(torch, press, m)
        d_len = torch.zeros(R, dtype=torch.int64, device=dev)
        d_need = torch.zeros(R, dtype=torch.int64, device=dev)
        new.ok(new.l.press_hip_press_sizes(mid, p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_need), 1))
        torch.cuda.synchronize()
        need = d_need.cpu().numpy()
        assert (need > 0).all(), "a read was refused"
        packs = {}
        for al in (1, 16):
            cap = int(((need + al - 1) // al * al).sum())  # (room: the layout's last end is not rounded, so it is at most this)
            packs[al] = {"cap": cap, "out": torch.empty(cap + 64, dtype=torch.uint8, device=dev),
                         "off": torch.zeros(R + 1, dtype=torch.int64, device=dev),
                         "len": torch.zeros(R, dtype=torch.int64, device=dev)}
        d_back = torch.zeros_like(b.sig)
        d_outn = torch.zeros(R, dtype=torch.int32, device=dev)

        def slot_press(lib):
            return lambda: lib.ok(lib.l.press_hip_press_batch(mid, p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_slots),
                                                              p(d_slot_off), p(d_len), 1))

        def packed(al):
            q = packs[al]
            return lambda: new.ok(new.l.press_hip_press_packed(mid, p(b.sig), p(b.d_off), p(b.d_n), R, total, p(q["out"]),
                                                               q["cap"], al, p(q["off"]), p(q["len"]), 1))

        def sizes():
            new.ok(new.l.press_hip_press_sizes(mid, p(b.sig), p(b.d_off), p(b.d_n), R, total, p(d_need), 1))

        def slot_dec(lib):
            return lambda: lib.ok(lib.l.press_hip_depress_batch(mid, p(d_slots), p(d_slot_in), p(d_len), R, p(d_back), p(b.d_off),
                                                                p(b.d_n), total, p(d_outn), 1))

        def packed_dec(al):
            q = packs[al]
            return lambda: new.ok(new.l.press_hip_depress_batch(mid, p(q["out"]), p(q["off"]), p(q["len"]), R, p(d_back),
                                                                p(b.d_off), p(b.d_n), total, p(d_outn), 1))

        legs = ([("baseline", slot_press(base)), ("baseline2", slot_press(base))] if base else []) + \
            [("press_batch", slot_press(new)), ("packed1", packed(1)), ("packed16", packed(16)), ("sizes", sizes)] + \
            ([("dec_baseline", slot_dec(base)), ("dec_baseline2", slot_dec(base))] if base else [("dec_slots", slot_dec(new))]) + \
            [("dec_packed1", packed_dec(1)), ("dec_packed16", packed_dec(16))]
        # warm-up and agreement: the packed streams are the slot arena's, and every decode gives the samples back
        for name, call in legs:
            if name.startswith("dec"):
                d_back.zero_()
            for _ in range(1 if a.once else 3):
                call()
            torch.cuda.synchronize()
            if name.startswith("dec"):
                assert bool((d_outn.cpu().numpy() == b.n).all()) and torch.equal(d_back, b.sig), (m, name)
        lens = d_len.cpu().numpy()
        assert np.array_equal(lens, need), (m, "need differs from press_hip_press_batch's out_len")
        slots = d_slots.cpu().numpy()
        soff = d_slot_off.cpu().numpy()
        ref = np.concatenate([slots[int(o):int(o) + int(l)] for o, l in zip(soff[:-1], lens)])
        rec = {"stream_bytes": int(lens.sum()), "slot_arena_bytes": int(soff[-1]),
               "bound_bytes": int(sum(int(new.l.press_hip_bound(mid, int(x))) for x in b.n)), "legs": {}}
        for al in (1, 16):
            q = packs[al]
            off = q["off"].cpu().numpy()
            end = int(off[-1])  # out_off[nreads]: the arena the layout takes, an exact count
            assert np.array_equal(q["len"].cpu().numpy(), lens) and end <= q["cap"], (m, al)
            assert end == int(off[-2]) + int(lens[-1]) and (al > 1 or end == int(lens.sum())), (m, al)
            arena = q["out"].cpu().numpy()
            got = arena[:end] if al == 1 else np.concatenate([arena[int(o):int(o) + int(l)] for o, l in zip(off[:-1], lens)])
            assert np.array_equal(got, ref), (m, al, "packed streams differ from the slot arena's")
            rec["packed%d_arena_bytes" % al] = end
        if not a.once:
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
                rec["legs"][name] = {"calls": int(ms.size), "median_ms": float(np.median(ms)),
                                     "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90))}
            if base:
                L = rec["legs"]
                rec["baseline_spread_ms"] = abs(L["baseline"]["median_ms"] - L["baseline2"]["median_ms"])
                rec["dec_baseline_spread_ms"] = abs(L["dec_baseline"]["median_ms"] - L["dec_baseline2"]["median_ms"])
                for k in ("press_batch", "packed1", "packed16"):
                    rec[k + "_minus_baseline_ms"] = L[k]["median_ms"] - L["baseline"]["median_ms"]
                for k in ("dec_packed1", "dec_packed16"):
                    rec[k + "_minus_baseline_ms"] = L[k]["median_ms"] - L["dec_baseline"]["median_ms"]
        result["methods"][m] = rec
        del d_slots, packs
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
