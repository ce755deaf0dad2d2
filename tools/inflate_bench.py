#!/usr/bin/env python3
"""BLOW5 records inflated on the device against the host reader's zlib pool, on bench.py's 8192-read batch.

    python3 tools/inflate_bench.py [--reads 8192] [--reps 5] [--out FILE]

The batch is pressed once with slow5_svb_zd and framed by blow5_write_like into two files with record compression zlib:
"host" (zlib on the writer's pool) and "device" (deflate="device", the streams of header section 2z).  Legs per file,
each after two warm-up runs, medians of --reps with min - max:

  a_host_reader   press_hip_blow5_next over the whole file, the reader's pool as it sizes itself (at most 32 threads; the
                  CPUs the process may use are reported): wall clock
  b_device_reader next_stored over the whole file, the copy of the stored records to the device,
                  press_hip_blow5_inflate_batch with the first-guess slots of 4 * comp_len + 4096 bytes and
                  press_hip_blow5_record_fields, synchronised: wall clock
  c_first_guess   the inflate call alone between HIP events, slots of 4 * comp_len + 4096 bytes
  c_exact         ... with slots of exactly the records' lengths
  c_sizes         press_hip_blow5_inflate_sizes alone
  d_longest       the longest record as a batch of its own (the call lasts as long as its longest record)

Before anything is timed the device's bytes of the first and last 32 records are compared with zlib.decompress.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIKE = os.path.join(ROOT, "tests", "golden", "three-reads.blow5")


def med(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("inflate_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R = b.R
    need = press.press_sizes("slow5_svb_zd", b.sig, b.d_off, b.d_n)
    torch.cuda.synchronize()
    arena = torch.zeros((int(need.sum()) + 3) // 4 * 4 + 64, dtype=torch.uint8, device=dev)
    out_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    out_len = torch.zeros(R, dtype=torch.int64, device=dev)
    press.press_packed("slow5_svb_zd", b.sig, b.d_off, b.d_n, arena, out_off, out_len)
    torch.cuda.synchronize()
    h_arena, h_off, h_len = arena.cpu().numpy(), out_off.cpu().numpy(), out_len.cpu().numpy()
    fields = [h_arena[int(o):int(o) + int(n)].tobytes() for o, n in zip(h_off[:-1], h_len)]
    del arena, b
    tmp = tempfile.mkdtemp(prefix="inflate_bench_")
    res = {"reads": R, "reps": a.reps, "cpus": len(os.sched_getaffinity(0)), "files": {}}

    def timed(fn, wall):
        ms = []
        for rep in range(a.reps + 2):
            torch.cuda.synchronize()
            if wall:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) * 1e3
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                t = e0.elapsed_time(e1)
            if rep >= 2:
                ms.append(t)
        return med(ms)

    try:
        for tag in ("host", "device"):
            path = os.path.join(tmp, tag + ".blow5")
            press.blow5_write_like(path, LIKE, fields, deflate=tag)
            out = res["files"][tag] = {"file_bytes": os.path.getsize(path)}
            host_arena = np.empty(sum(len(f) for f in fields) + 16 * R + 4096, dtype=np.uint8)
            off, ln = np.zeros(R, dtype=np.uint64), np.zeros(R, dtype=np.uint64)
            ns = np.zeros(R, dtype=np.uint32)

            def host_reader():
                rd = press.Blow5Reader(path)
                got = 0
                while True:
                    k = rd.next_arena(host_arena, off, ln, ns, R)
                    if k == 0:
                        break
                    got += k
                rd.close()
                assert got == R

            stored = np.empty(out["file_bytes"] + 16 * R, dtype=np.uint8)
            state = {}

            def device_reader(keep=False):
                rd = press.Blow5Reader(path)
                _, coff, clen = rd.next_stored(R, arena=stored)
                rd.close()
                assert coff.size == R
                used = int(coff[-1] + clen[-1])
                comp = torch.from_numpy(stored[:used]).to(dev)
                d_off = torch.from_numpy(coff.view(np.int64)).to(dev)
                d_len = torch.from_numpy(clen.view(np.int64)).to(dev)
                slots = press._slots(4 * clen + 4096)
                d_slots = torch.from_numpy(slots.view(np.int64)).to(dev)
                rec = torch.empty(int(slots[-1]), dtype=torch.uint8, device=dev)
                rlen = torch.empty(R, dtype=torch.int64, device=dev)
                st = torch.empty(R, dtype=torch.uint8, device=dev)
                press.blow5_inflate_batch(comp, d_off, d_len, rec, d_slots, rlen, st)
                f = press.blow5_record_fields(rec, d_slots[:R], rlen, 1, want_ids=False)
                if keep:
                    state.update(comp=comp, off=d_off, len=d_len, slots=d_slots, rec=rec, rlen=rlen, st=st, f=f, coff=coff, clen=clen)

            # what is being timed is right
            device_reader(keep=True)
            torch.cuda.synchronize()
            st = state["st"].cpu().numpy()
            out["status_counts"] = {press.INFLATE_STATUS[k]: int((st == k).sum()) for k in np.unique(st)}
            assert not st.any(), out["status_counts"]
            h_rlen, h_slots = state["rlen"].cpu().numpy(), state["slots"].cpu().numpy()
            for k in list(range(min(32, R))) + list(range(max(0, R - 32), R)):
                o, n = int(state["coff"][k]), int(state["clen"][k])
                want = zlib.decompress(stored[o:o + n].tobytes())
                got = state["rec"][int(h_slots[k]):int(h_slots[k]) + int(h_rlen[k])].cpu().numpy().tobytes()
                assert got == want, k
            sig_len = state["f"][1].cpu().numpy()
            assert [int(x) for x in sig_len] == [len(f) for f in fields]
            out["stored_bytes"] = int(state["clen"].sum())
            out["inflated_bytes"] = int(h_rlen.sum())
            out["a_host_reader_ms"] = timed(host_reader, True)
            out["b_device_reader_ms"] = timed(device_reader, True)
            s = state
            out["c_first_guess_ms"] = timed(lambda: press.blow5_inflate_batch(s["comp"], s["off"], s["len"], s["rec"], s["slots"], s["rlen"],
                                                                              s["st"]), False)
            exact = torch.from_numpy(np.concatenate([[0], np.cumsum(h_rlen)]).astype(np.int64)).to(dev)
            out["c_exact_ms"] = timed(lambda: press.blow5_inflate_batch(s["comp"], s["off"], s["len"], s["rec"], exact, s["rlen"], s["st"]), False)
            assert not s["st"].cpu().numpy().any()
            out["c_sizes_ms"] = timed(lambda: press.blow5_inflate_sizes(s["comp"], s["off"], s["len"]), False)
            k = int(np.argmax(h_rlen))
            one = [t[k:k + 1].contiguous() for t in (s["off"], s["len"])]
            slot1 = torch.tensor([0, int(h_rlen[k])], dtype=torch.int64, device=dev)
            out["d_longest_ms"] = timed(lambda: press.blow5_inflate_batch(s["comp"], one[0], one[1], s["rec"], slot1, s["rlen"][:1], s["st"][:1]),
                                        False)
            out["longest_record_bytes"] = int(h_rlen[k])
            out["inflated_GBps"] = {leg: out["inflated_bytes"] / 1e6 / out[leg + "_ms"]["median"]
                                    for leg in ("a_host_reader", "b_device_reader", "c_first_guess", "c_exact", "c_sizes")}
            out["host_over_device_reader_time"] = out["a_host_reader_ms"]["median"] / out["b_device_reader_ms"]["median"]
            state.clear()
            del s
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
