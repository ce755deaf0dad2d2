#!/usr/bin/env python3
"""Generate tests/golden/sigtk_jnn.json from the REAL reference: sigtk's jnn segmenter and its jnnv2 adaptor finder
(press/sigtk/src/jnn.c).

Run in the build container only (needs /root/reference and gcc):

    python tests/golden/make_jnn_golden.py

jnn.c is compiled as it is, with gcc -O2, together with the few lines of DRIVER below (a stub for get_log_level and a
main that reads samples or floats and writes the segments), into a temporary directory.  Nothing of the reference is
committed: the fixture holds DATA - per entry the read's name, n, the kind of run and its parameters, the segment count, a
sha256 over the packed (start, end) records and the first and last eight of them; for jnnv2 the pair.

The entries: the three reads of three_reads.i16.bin and every non-empty read of _layouts.battery(), each
  raw   jnn_raw under JNNV1_CDNA_PARAM and JNNV1_DRNA_PARAM
  v2    jnnv2 under JNNV2_RNA_ADAPTOR
  pa    jnn_pa under JNNV1_POLYA on the picoampere floats of the two calibrations of CALS (what
        press_hip_depress_pa_batch defines: x = ((float) s + offset) * scale, rounded separately), with top and bot at the
        read's median picoampere value + 15 and - 15 (single precision; their bit patterns are in the entry)
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
CALS = ((8192.0, 6.0, 1467.61), (2048.0, -243.0, 748.58))  # digitisation, offset, range: those of sigtk_events.json
HALF_BAND = 15.0

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "error.h"
#include "jnn.h"
enum sigtk_log_level_opt get_log_level() { return (enum sigtk_log_level_opt) 0; }
static void *slurp(const char *path, size_t es, size_t *n)
{
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    *n = (size_t) ftell(f) / es;
    fseek(f, 0, SEEK_SET);
    void *p = malloc(*n * es + 1);
    if (fread(p, es, *n, f) != *n) exit(2);
    fclose(f);
    return p;
}
/* driver raw|pa|v2 in out [which [top bot]] */
int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    size_t n;
    FILE *o = fopen(argv[3], "wb");
    if (!o) return 2;
    if (!strcmp(argv[1], "v2")) {
        int16_t *s = (int16_t *) slurp(argv[2], 2, &n);
        jnnv2_param_t prm = JNNV2_RNA_ADAPTOR;
        jnn_pair_t p = jnnv2(s, (int64_t) n, prm);
        long long v[2] = { p.x, p.y };
        fwrite(v, 8, 2, o);
    } else {
        jnn_param_t cdna = JNNV1_CDNA_PARAM, drna = JNNV1_DRNA_PARAM, polya = JNNV1_POLYA;
        int which = atoi(argv[4]), k = 0;
        jnn_param_t prm = which == 0 ? cdna : which == 1 ? drna : polya;
        jnn_pair_t *segs;
        if (!strcmp(argv[1], "pa")) {
            unsigned tb = (unsigned) strtoul(argv[5], NULL, 10), bb = (unsigned) strtoul(argv[6], NULL, 10);
            memcpy(&prm.top, &tb, 4);
            memcpy(&prm.bot, &bb, 4);
            float *x = (float *) slurp(argv[2], 4, &n);
            segs = jnn_pa(x, (int64_t) n, prm, &k);
        } else {
            int16_t *s = (int16_t *) slurp(argv[2], 2, &n);
            segs = jnn_raw(s, (int64_t) n, prm, &k);
        }
        for (int i = 0; i < k; i++) {
            long long v[2] = { segs[i].x, segs[i].y };
            fwrite(v, 8, 2, o);
        }
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
    for name, s in _layouts.battery():
        if len(s):
            out.append(("battery/" + name, s))
    return out


def records(path):
    raw = np.fromfile(path, dtype="<i8").reshape(-1, 2)
    assert (raw >= 0).all() and (raw < 1 << 32).all()
    recs = [(int(a), int(b)) for a, b in raw]
    packed = b"".join(struct.pack("<II", *r) for r in recs)
    return {"count": len(recs), "sha256": hashlib.sha256(packed).hexdigest(), "first": [list(r) for r in recs[:8]],
            "last": [list(r) for r in recs[-8:]]}


def main():
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.c")
        exe = os.path.join(tmp, "jnn_ref")
        open(drv, "w").write(DRIVER)
        subprocess.run(["gcc", "-O2", "-I", os.path.join(SIGTK, "src"), "-I", os.path.join(SIGTK, "slow5lib", "include"),
                        os.path.join(SIGTK, "src", "jnn.c"), drv, "-o", exe, "-lm"], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        for name, s in named_reads():
            s.tofile(fin)
            for which, preset in ((0, "cdna"), (1, "drna")):
                subprocess.run([exe, "raw", fin, fout, str(which)], check=True, stderr=subprocess.DEVNULL)
                e = {"kind": "raw", "name": name, "n": int(len(s)), "preset": preset}
                e.update(records(fout))
                entries.append(e)
                print(name, "raw", preset, e["count"], file=sys.stderr)
            subprocess.run([exe, "v2", fin, fout], check=True, stderr=subprocess.DEVNULL)
            pair = np.fromfile(fout, dtype="<i8")
            entries.append({"kind": "v2", "name": name, "n": int(len(s)), "pair": [int(pair[0]), int(pair[1])]})
            print(name, "v2", pair, file=sys.stderr)
        for name, s in named_reads():
            for cal in CALS:
                c0, c1 = cal_floats(*cal)
                x = picoamperes(s, c0, c1)
                x.tofile(fin)
                med = np.float32(np.median(x))
                top, bot = np.float32(med + np.float32(HALF_BAND)), np.float32(med - np.float32(HALF_BAND))
                subprocess.run([exe, "pa", fin, fout, "2", str(bits(top)), str(bits(bot))], check=True, stderr=subprocess.DEVNULL)
                e = {"kind": "pa", "name": name, "n": int(len(s)), "preset": "polya", "cal_bits": [bits(c0), bits(c1)],
                     "top_bits": bits(top), "bot_bits": bits(bot)}
                e.update(records(fout))
                entries.append(e)
                print(name, "pa", cal, e["count"], file=sys.stderr)
    doc = {"source": "press/sigtk/src/jnn.c jnn_raw(), jnn_pa(), jnnv2(), gcc -O2; records packed as <II start, end",
           "calibrations": [{"digitisation": d, "offset": o, "range": r} for d, o, r in CALS],
           "half_band_pa": HALF_BAND, "entries": entries}
    with open(os.path.join(HERE, "sigtk_jnn.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
