#!/usr/bin/env python3
"""Generate tests/golden/sigtk_events.json from the REAL reference: sigtk's event detector (scrappie's, as
press/sigtk/src/events.c carries it) run on picoampere floats.

Run in the build container only (needs /root/reference and gcc):

    python tests/golden/make_events_golden.py

events.c is compiled as it is, with gcc -O2, together with the few lines of DRIVER below (a stub for get_log_level and a
main that reads floats and writes the event table), into a temporary directory.  Nothing of the reference is committed:
the fixture holds DATA - per entry the read's name, n, the two calibration floats as bit patterns, the preset, the event
count, a sha256 over the packed (start, length, mean bits, stdv bits) records and the first and last eight events.

The entries: the three reads of three_reads.i16.bin and the reads of _layouts.battery() named in BATTERY (at least 200
samples and not constant: getevents() asserts on the others, events.c:242), each under both presets and the two
calibrations of CALS.  The floats are what press_hip_depress_pa_batch defines, x = ((float) s + offset) * scale with the
add and the multiply rounded separately, scale = (float) (range / digitisation).
"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import _layouts  # noqa: E402

SIGTK = "/root/reference/press/sigtk"
CALS = ((8192.0, 6.0, 1467.61), (2048.0, -243.0, 748.58))  # digitisation, offset, range
BATTERY = ("ex1-2047", "ex1-2049", "ex30-20000", "wrap-5000", "q8-10000", "synth-0")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "error.h"
#include "sigtk.h"
enum sigtk_log_level_opt get_log_level() { return (enum sigtk_log_level_opt) 0; }
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    size_t n = (size_t) ftell(f) / sizeof(float);
    fseek(f, 0, SEEK_SET);
    float *x = (float *) malloc(n * sizeof(float) + 1);
    if (fread(x, sizeof(float), n, f) != n) return 2;
    fclose(f);
    event_table et = getevents(n, x, (int8_t) atoi(argv[2]));
    FILE *o = fopen(argv[3], "wb");
    if (!o) return 2;
    for (size_t i = 0; i < et.n; i++) {
        unsigned long long start = et.event[i].start;
        float rec[3] = { et.event[i].length, et.event[i].mean, et.event[i].stdv };
        fwrite(&start, 8, 1, o);
        fwrite(rec, 4, 3, o);
    }
    fclose(o);
    return 0;
}
"""


def cal_floats(dig, offset, rng):
    return np.float32(offset), np.float32(rng / dig)


def picoamperes(s, c0, c1):
    return ((s.astype(np.float32) + np.float32(c0)) * np.float32(c1)).astype(np.float32)


def bits(f):
    return int(np.float32(f).view(np.uint32))


def named_reads():
    out = []
    flat = np.fromfile(os.path.join(HERE, "three_reads.i16.bin"), dtype=np.int16)
    o = 0
    for r in json.load(open(os.path.join(HERE, "three_reads.json")))["reads"]:
        out.append(("three_reads/" + r["read_id"], flat[o:o + r["n"]].copy()))
        o += r["n"]
    bat = dict(_layouts.battery())
    for name in BATTERY:
        out.append(("battery/" + name, bat[name]))
    return out


def main():
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.c")
        exe = os.path.join(tmp, "events_ref")
        open(drv, "w").write(DRIVER)
        subprocess.run(["gcc", "-O2", "-I", os.path.join(SIGTK, "src"), "-I", os.path.join(SIGTK, "slow5lib", "include"),
                        os.path.join(SIGTK, "src", "events.c"), drv, "-o", exe, "-lm"], check=True)
        for name, s in named_reads():
            for cal in CALS:
                c0, c1 = cal_floats(*cal)
                fin, fout = os.path.join(tmp, "x.f32"), os.path.join(tmp, "ev.bin")
                picoamperes(s, c0, c1).tofile(fin)
                for rna in (0, 1):
                    subprocess.run([exe, fin, str(rna), fout], check=True)
                    raw = np.fromfile(fout, dtype=np.dtype([("start", "<u8"), ("length", "<f4"), ("mean", "<u4"), ("stdv", "<u4")]))
                    length = raw["length"].astype(np.int64)
                    assert (length.astype(np.float32) == raw["length"]).all() and (length < 1 << 24).all()
                    recs = [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(raw["start"], length, raw["mean"], raw["stdv"])]
                    packed = b"".join(struct.pack("<IIII", *r) for r in recs)
                    entries.append({"name": name, "n": int(len(s)), "cal_bits": [bits(c0), bits(c1)],
                                    "preset": "rna" if rna else "dna", "count": len(recs),
                                    "sha256": hashlib.sha256(packed).hexdigest(),
                                    "first": [list(r) for r in recs[:8]], "last": [list(r) for r in recs[-8:]]})
                    print(name, cal, "rna" if rna else "dna", len(recs), file=sys.stderr)
    doc = {"source": "press/sigtk/src/events.c getevents(), gcc -O2; records packed as <IIII start, length, mean bits, stdv bits",
           "calibrations": [{"digitisation": d, "offset": o, "range": r} for d, o, r in CALS], "entries": entries}
    with open(os.path.join(HERE, "sigtk_events.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
