#!/usr/bin/env python3
"""BLOW5 records deflated on the device against the host's zlib pool, on bench.py's 8192-read batch.

    python3 tools/deflate_bench.py [--reads 8192] [--reps 5] [--out FILE]

The batch is pressed once with slow5_svb_zd into a packed device arena (press_hip_press_packed); every read becomes a
record with the fixed fields and auxiliary fields of tests/golden/three-reads.blow5's first record and a read id of its
own, as blow5_write_like frames them.  Legs, each after two warm-up runs, medians of --reps:

  device        press_hip_blow5_deflate_batch, device resident: HIP events around the call
  device_file   that call, the image's way back to the host and press_hip_blow5_write_image into a file: wall clock
  host_file     press_hip_blow5_write_batch on the same records (fields already on the host), record method zlib, the
                writer's pool as it sizes itself (at most 32 threads; the CPUs the process may use are reported): wall clock

and the exact bytes both forms write for the records.  Before anything is timed, the device's streams of the first and
last 32 records are inflated by zlib and compared with the framed records.
"""
import argparse
import ctypes
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


def template(press):
    """the fixed fields and the auxiliary fields of LIKE's first record"""
    rd = press.Blow5Reader(LIKE)
    arena = np.empty(1 << 24, dtype=np.uint8)
    ro, rl, sp, sl = (np.zeros(1, dtype=np.uint64) for _ in range(4))
    ns, got = np.zeros(1, dtype=np.uint32), ctypes.c_uint32()
    press._blow5_call("press_hip_blow5_next_records", rd._h, 1, press._ptr(arena), arena.size, press._ptr(ro), press._ptr(rl),
                      press._ptr(sp), press._ptr(sl), press._ptr(ns), ctypes.byref(got))
    rd.close()
    rec = arena[int(ro[0]):int(ro[0]) + int(rl[0])]
    idl = int(rec[0]) | (int(rec[1]) << 8)
    return rec[2 + idl:int(sp[0]) - 8].copy(), rec[int(sp[0]) + int(sl[0]):].copy()


def writer(press, path):
    rd = press.Blow5Reader(LIKE)
    w = ctypes.c_void_p()
    press._blow5_call("press_hip_blow5_create", path.encode(), rd._h, 1, 1, ctypes.byref(w))
    rd.close()
    return w


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bench
    from honours_amd import deflate, press, synth

    if not torch.cuda.is_available():
        sys.exit("deflate_bench needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, a.reads, dev, None)
    R = b.R
    need = press.press_sizes("slow5_svb_zd", b.sig, b.d_off, b.d_n)
    torch.cuda.synchronize()
    cap = (int(need.sum()) + 3) // 4 * 4
    arena = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
    out_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    out_len = torch.zeros(R, dtype=torch.int64, device=dev)
    press.press_packed("slow5_svb_zd", b.sig, b.d_off, b.d_n, arena, out_off, out_len)
    torch.cuda.synchronize()
    fixed, post = template(press)
    pres = []
    for k in range(R):
        rid = b"read-%08d" % k
        pres.append(np.frombuffer(bytes([len(rid) & 255, len(rid) >> 8]) + rid + fixed.tobytes(), dtype=np.uint8))
    posts = [post] * R
    side, tab = deflate.side_arena(pres, posts)
    h_arena, h_off, h_len = arena.cpu().numpy(), out_off.cpu().numpy(), out_len.cpu().numpy()
    sigs = [h_arena[int(o):int(o) + int(l)] for o, l in zip(h_off[:-1], h_len)]
    record_bytes = int(side.size + 8 * R + h_len.sum())
    d_side = torch.from_numpy(side).to(dev)
    d_tab = torch.from_numpy(tab.reshape(-1).view(np.int64).copy()).to(dev)
    d_sig_off = out_off[:R].contiguous()
    image = torch.empty(press.blow5_deflate_image_cap(record_bytes, R), dtype=torch.uint8, device=dev)
    rec_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
    raw = torch.empty(R, dtype=torch.uint8, device=dev)

    def device_call():
        press.blow5_deflate_batch(d_side, d_tab, arena, d_sig_off, out_len, record_bytes, image, rec_off, raw)

    # what is being timed is right: the streams inflate to the framed records
    device_call()
    torch.cuda.synchronize()
    h_rec_off = rec_off.cpu().numpy().view(np.uint64)
    h_raw = raw.cpu().numpy()
    assert not (h_raw == press.DEFLATE_REFUSED).any(), "a record was refused"
    total = int(h_rec_off[R])
    h_image = image[:total].cpu().numpy()
    for k in list(range(min(32, R))) + list(range(max(0, R - 32), R)):
        rec = pres[k].tobytes() + int(h_len[k]).to_bytes(8, "little") + sigs[k].tobytes() + post.tobytes()
        o, e = int(h_rec_off[k]), int(h_rec_off[k + 1])
        assert int.from_bytes(h_image[o:o + 8].tobytes(), "little") == e - o - 8, k
        assert zlib.decompress(h_image[o + 8:e].tobytes()) == rec, k
    tmp = tempfile.mkdtemp(prefix="deflate_bench_")
    res = {"reads": R, "samples": b.total_samples, "record_bytes": record_bytes, "reps": a.reps,
           "cpus": len(os.sched_getaffinity(0)), "stored_records": int((h_raw == 1).sum()),
           "workspace_bytes": int(press.load_library().press_hip_blow5_deflate_workspace_bytes(record_bytes, R))}
    try:
        # device: HIP events around the call
        ms = []
        for rep in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            device_call()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                ms.append(e0.elapsed_time(e1))
        res["device_ms"] = {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
        # device_file: the call, the image back, one fwrite
        ms, dev_bytes = [], None
        for rep in range(a.reps + 2):
            path = os.path.join(tmp, "dev%d.blow5" % rep)
            w = writer(press, path)
            head = os.path.getsize(path) if os.path.exists(path) else 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device_call()
            off = rec_off.cpu().numpy().view(np.uint64)
            img = image[:int(off[R])].cpu().numpy()
            press._blow5_write_image(w, img, off, pres)
            t1 = time.perf_counter()
            press._blow5_call("press_hip_blow5_finish", w)
            dev_bytes = os.path.getsize(path)
            os.remove(path)
            if rep >= 2:
                ms.append((t1 - t0) * 1e3)
        res["device_file_ms"] = {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
        # host_file: zlib on the writer's pool
        ms, host_bytes = [], None
        for rep in range(a.reps + 2):
            path = os.path.join(tmp, "host%d.blow5" % rep)
            w = writer(press, path)
            t0 = time.perf_counter()
            press._blow5_write_batch(w, pres, sigs, posts)
            t1 = time.perf_counter()
            press._blow5_call("press_hip_blow5_finish", w)
            host_bytes = os.path.getsize(path)
            os.remove(path)
            if rep >= 2:
                ms.append((t1 - t0) * 1e3)
        res["host_file_ms"] = {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
        empty = os.path.join(tmp, "empty.blow5")
        press._blow5_call("press_hip_blow5_finish", writer(press, empty))
        head = os.path.getsize(empty)
        res["device_record_bytes"] = dev_bytes - head
        res["host_record_bytes"] = host_bytes - head
        assert res["device_record_bytes"] == total
        res["device_over_host_bytes"] = res["device_record_bytes"] / res["host_record_bytes"]
        res["host_over_device_file_time"] = res["host_file_ms"]["median"] / res["device_file_ms"]["median"]
        res["record_MBps"] = {k: record_bytes / 1e3 / res[k + "_ms"]["median"] for k in ("device", "device_file", "host_file")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
