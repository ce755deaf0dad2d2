#!/usr/bin/env python3
"""Generate tests/golden/sigtk_prefix.json from the REAL reference: sigtk's `prefix` and `stat` subcommands
(press/sigtk/src/cfunc.c prefix_func and stat_func, with jnn.c, stat.h and misc.c behind them).

Run in the build container only (needs /root/reference and gcc):

    python tests/golden/make_prefix_golden.py

jnn.c, cfunc.c, misc.c, events.c and sigtk.c are compiled as they are (gcc -O2 -ffunction-sections -Wl,--gc-sections, which
links without slow5lib) together with the few lines of DRIVER below, into a temporary directory.  Nothing of the reference
is committed: the fixture holds DATA.  The driver fills a slow5_rec_t by hand and, per read and calibration, writes

  (a) the bit patterns of every number, from its own sequence of jnnv2, meanf, stdvf, medianf, find_polya, meani16,
      stdvi16 and mediani16 - the sequence prefix_func and stat_func run
  (b) the text the reference's own prefix_func (rna = 1, p_stat = 1) and stat_func print

and this script asserts that (b) is (a) formatted with %f / %d / %ld: that pins the driver to the subcommands themselves.

The entries: the three reads of three_reads.i16.bin and every non-empty read of _layouts.battery(), each under the two
calibrations of sigtk_jnn.json.  Per entry: adapt and polya (positions in the read, [-1, -1] for an absent tail), thr_bits
(bot, top of the poly-A walk), adapt_stat / polya_stat (mean, stdv, median bits; null for an absent stretch), raw_stat (mean
and stdv bits, the median sample) and pa_stat of the whole read, and the two texts.
"""
import json
import os
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
CALS = ((8192.0, 6.0, 1467.61), (2048.0, -243.0, 748.58))  # digitisation, offset, range: those of sigtk_jnn.json

DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jnn.h"
#include "sigtk.h"
#include "stat.h"
void prefix_func(slow5_rec_t *rec, opt_t opt);
void stat_func(slow5_rec_t *rec, opt_t opt);
static unsigned fb(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static void three(FILE *o, const char *key, const float *x, int n)
{
    fprintf(o, "%s %u %u %u\n", key, fb(meanf(x, n)), fb(stdvf(x, n)), fb(medianf(x, n)));
}
/* driver in name digitisation offset range bits_out : the two texts go to stdout */
int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    size_t n = (size_t) ftell(f) / 2;
    fseek(f, 0, SEEK_SET);
    int16_t *s = (int16_t *) malloc(n * 2 + 2);
    if (fread(s, 2, n, f) != n) return 2;
    fclose(f);
    slow5_rec_t rec;
    memset(&rec, 0, sizeof rec);
    rec.read_id = argv[2];
    rec.read_id_len = (slow5_rid_len_t) strlen(argv[2]);
    rec.digitisation = atof(argv[3]);
    rec.offset = atof(argv[4]);
    rec.range = atof(argv[5]);
    rec.len_raw_signal = n;
    rec.raw_signal = s;
    FILE *o = fopen(argv[6], "w");
    if (!o) return 2;

    /* (a) */
    float *cur = signal_in_picoamps(&rec);
    float c0 = (float) rec.offset, c1 = (float) rec.range / (float) rec.digitisation;
    fprintf(o, "cal %u %u\n", fb(c0), fb(c1));
    fprintf(o, "raw_stat %u %u %d\n", fb(meani16(s, (int) n)), fb(stdvi16(s, (int) n)), (int) mediani16(s, (int) n));
    three(o, "pa_stat", cur, (int) n);
    jnn_pair_t p = find_adaptor(&rec);
    fprintf(o, "adapt %" PRId64 " %" PRId64 "\n", (int64_t) p.x, (int64_t) p.y);
    if (p.y > 0) {
        float m_a = meanf(&cur[p.x], p.y - p.x);
        three(o, "adapt_stat", &cur[p.x], p.y - p.x);
        float top = m_a + 30 + 20, bot = m_a + 30 - 20;
        fprintf(o, "thr %u %u\n", fb(bot), fb(top));
        jnn_pair_t a = find_polya(&cur[p.y], (int64_t) n - p.y, top, bot);
        if (a.y > 0) {
            fprintf(o, "polya %" PRId64 " %" PRId64 "\n", (int64_t) (a.x + p.y), (int64_t) (a.y + p.y));
            three(o, "polya_stat", &cur[a.x + p.y], a.y - a.x);
        }
    }
    fclose(o);
    free(cur);

    /* (b) */
    opt_t opt;
    memset(&opt, 0, sizeof opt);
    opt.rna = 1;
    opt.p_stat = 1;
    prefix_func(&rec, opt);
    stat_func(&rec, opt);
    return 0;
}
"""


def f32(b):
    return np.array([b], dtype=np.uint32).view(np.float32)[0]


def bits(f):
    return int(np.float32(f).view(np.uint32))


def fmt3(b):
    return "%f\t%f\t%f" % tuple(float(f32(v)) for v in b)


def texts(name, e):
    """what prefix_func (rna, p_stat) and stat_func print for the numbers of (a) (cfunc.c:126-234)"""
    t = "%s\t%d\t" % (name, e["n"])
    if e["adapt"][1] > 0:
        t += "%d\t%d\t" % tuple(e["adapt"])
        t += "%d\t%d" % tuple(e["polya"]) if e["polya"][1] > 0 else ".\t."
        t += "\t" + fmt3(e["adapt_stat"]) + "\t"
        t += "\t" + fmt3(e["polya_stat"]) + "\t" if e["polya"][1] > 0 else "\t.\t.\t."
    else:
        t += ".\t.\t.\t."
    r, p = e["raw_stat"], e["pa_stat"]
    st = "%s\t%d\t" % (name, e["n"])
    st += "%f\t%f\t%f\t%f\t%d\t%f\t" % (float(f32(r[0])), float(f32(p[0])), float(f32(r[1])), float(f32(p[1])), r[2],
                                        float(f32(p[2])))
    return t, st


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


def main():
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.c")
        exe = os.path.join(tmp, "prefix_ref")
        open(drv, "w").write(DRIVER)
        src = [os.path.join(SIGTK, "src", f) for f in ("jnn.c", "cfunc.c", "misc.c", "events.c", "sigtk.c")]
        subprocess.run(["gcc", "-O2", "-ffunction-sections", "-Wl,--gc-sections", "-I", os.path.join(SIGTK, "src"),
                        "-I", os.path.join(SIGTK, "slow5lib", "include")] + src + [drv, "-o", exe, "-lm"], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.txt")
        for name, s in named_reads():
            s.tofile(fin)
            for dig, offset, rng in CALS:
                run = subprocess.run([exe, fin, name, repr(dig), repr(offset), repr(rng), fout], check=True,
                                     stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
                got = {}
                for line in open(fout):
                    k, *v = line.split()
                    got[k] = [int(x) for x in v]
                assert got["cal"] == [bits(offset), bits(np.float32(rng / dig))], (name, got["cal"])
                e = {"name": name, "n": int(len(s)), "cal_bits": got["cal"], "adapt": got["adapt"],
                     "polya": got.get("polya", [-1, -1]), "thr_bits": got.get("thr"), "adapt_stat": got.get("adapt_stat"),
                     "polya_stat": got.get("polya_stat"), "raw_stat": got["raw_stat"], "pa_stat": got["pa_stat"]}
                ptxt, stxt = run.stdout.decode().split("\n")[:2]
                want = texts(name, e)
                assert (ptxt, stxt) == want, (name, ptxt, stxt, want)
                e["prefix_text"], e["stat_text"] = ptxt, stxt
                entries.append(e)
                print(name, (dig, offset, rng), e["adapt"], e["polya"], file=sys.stderr)
    doc = {"source": "press/sigtk/src/cfunc.c prefix_func(rna = 1, p_stat = 1) and stat_func(), gcc -O2; floats as bit patterns",
           "calibrations": [{"digitisation": d, "offset": o, "range": r} for d, o, r in CALS], "entries": entries}
    with open(os.path.join(HERE, "sigtk_prefix.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
