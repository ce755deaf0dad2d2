#!/usr/bin/env python3
"""Generate tests/golden/viz_tally.json from the REAL reference: the frequency tables of viz/ (tally.c with tally.h's
updatetally, as viz/freq_slow5.c and viz/freq_delta_slow5.c drive them), the exception count of viz/get_exceptions.c and
the per-read statistics of press/stats.c.

Run in the build container only (needs /root/reference and gcc):

    python tests/golden/make_tally_golden.py

viz/tally.c, viz/getsig.c and press/stats.c are compiled as they are together with the few lines of DRIVER below, into a
temporary directory.  Nothing of the reference is committed: the fixture holds DATA.  The driver reads a set of reads and

  (a) runs the loops of freq_slow5.c (every sample) and freq_delta_slow5.c (cur - prev as int16, reads of more than one
      sample) over the whole set with updatetally, and prints both tables with the reference's own printtally
  (b) counts, per non-empty read, the differences with diff > 127 || diff < -128 as get_exceptions.c does (it reads
      raw_signal[0] of an empty read: empty reads are left out of this leg and have nex null)
  (c) runs get_stats per read: n, min, max, and the bit patterns of mean, var and sd (Welford's recurrence in double)

Two conditions on the inputs, asserted here: the reference allocates TALLY_SZ_EXP = 8192 counters and indexes them by
zz(x), so every sample and every wrapped delta of a fixture read lies in [-4096, 4095].  The sets: the three reads of
three_reads.i16.bin, and the reads of _layouts.battery() that satisfy the condition.

Per set: the two tables as [value, count] rows (parsed from printtally's text) and the text itself.  Per read: n, min, max,
mean_bits, var_bits, sd_bits, nex.
"""
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

REF = "/root/reference"

DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "stats.h"
#include "tally.h"
static uint64_t db(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
/* driver in : u32 nreads, then per read u32 n and n int16 samples */
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t nreads, r;
    if (fread(&nreads, 4, 1, f) != 1) return 2;
    uint64_t *raw = calloc(TALLY_SZ_EXP, sizeof *raw), *delta = calloc(TALLY_SZ_EXP, sizeof *delta);
    int16_t rmin = INT16_MAX, rmax = INT16_MIN, dmin = INT16_MAX, dmax = INT16_MIN;
    for (r = 0; r < nreads; r++) {
        uint32_t n;
        uint64_t i;
        if (fread(&n, 4, 1, f) != 1) return 2;
        int16_t *s = malloc((size_t) n * 2 + 2);
        if (n && fread(s, 2, n, f) != n) return 2;
        for (i = 0; i < n; i++)                      /* freq_slow5.c gettally_slow5 */
            updatetally(raw, s[i], &rmin, &rmax);
        if (n > 1) {                                 /* freq_delta_slow5.c gettally_delta_slow5 */
            int16_t prev = s[0], cur, x;
            for (i = 1; i < n; i++) {
                cur = s[i];
                x = cur - prev;
                updatetally(delta, x, &dmin, &dmax);
                prev = cur;
            }
        }
        int nex = -1;
        if (n) {                                     /* get_exceptions.c write_exc */
            int16_t prev = s[0], cur, diff;
            nex = 0;
            for (i = 1; i < n; i++) {
                cur = s[i];
                diff = cur - prev;
                prev = cur;
                if (diff > 127 || diff < -128)
                    nex++;
            }
        }
        struct stats st;
        get_stats(s, n, &st);
        printf("read %" PRIu64 " %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", st.n, (int) st.min, (int) st.max, db(st.mean),
               db(st.var), db(st.sd), nex);
        free(s);
    }
    fclose(f);
    printf("== raw\n");
    printtally(raw, rmin, rmax);
    printf("== delta\n");
    printtally(delta, dmin, dmax);
    return 0;
}
"""


def in_domain(s):
    """every sample and every 16-bit wrapped delta in [-4096, 4095]: where the reference's 8192 counters are defined"""
    s = np.asarray(s, dtype=np.int16)
    if s.size and (int(s.min()) < -4096 or int(s.max()) > 4095):
        return False
    d = (s[1:].astype(np.int32) - s[:-1].astype(np.int32)).astype(np.int16)
    return not d.size or (int(d.min()) >= -4096 and int(d.max()) <= 4095)


def sets():
    flat = np.fromfile(os.path.join(HERE, "three_reads.i16.bin"), dtype=np.int16)
    three, o = [], 0
    for r in json.load(open(os.path.join(HERE, "three_reads.json")))["reads"]:
        three.append(("three_reads/" + r["read_id"], flat[o:o + r["n"]].copy()))
        o += r["n"]
    battery = [("battery/" + name, s) for name, s in _layouts.battery() if in_domain(s)]
    return [("three_reads", three), ("battery", battery)]


def parse_table(text):
    lines = text.split("\n")
    assert lines[0] == "signal\tfreq" and lines[-1] == "", lines[:2]
    return [[int(x) for x in ln.split("\t")] for ln in lines[1:-1]]


def main():
    doc = {"source": "viz/tally.c printtally over tally.h updatetally (the loops of viz/freq_slow5.c, viz/freq_delta_slow5.c), "
                     "viz/get_exceptions.c's count, press/stats.c get_stats; gcc -O2; doubles as bit patterns",
           "sets": []}
    with tempfile.TemporaryDirectory() as tmp:
        drv, exe, fin = os.path.join(tmp, "driver.c"), os.path.join(tmp, "tally_ref"), os.path.join(tmp, "in.bin")
        open(drv, "w").write(DRIVER)
        src = [os.path.join(REF, "viz", "tally.c"), os.path.join(REF, "viz", "getsig.c"), os.path.join(REF, "press", "stats.c")]
        subprocess.run(["gcc", "-O2", "-ffunction-sections", "-Wl,--gc-sections", "-I", os.path.join(REF, "press"),
                        "-I", os.path.join(REF, "viz")] + src + [drv, "-o", exe, "-lm"], check=True)
        for name, reads in sets():
            assert reads and all(in_domain(s) for _, s in reads), name
            with open(fin, "wb") as f:
                f.write(struct.pack("<I", len(reads)))
                for _, s in reads:
                    f.write(struct.pack("<I", len(s)))
                    f.write(np.ascontiguousarray(s, dtype="<i2").tobytes())
            out = subprocess.run([exe, fin], check=True, stdout=subprocess.PIPE).stdout.decode()
            head, rest = out.split("== raw\n")
            raw_text, delta_text = rest.split("== delta\n")
            entries = []
            for (rname, s), line in zip(reads, head.strip("\n").split("\n")):
                tag, n, mn, mx, mean, var, sd, nex = line.split()
                assert tag == "read" and int(n) == len(s), (rname, line)
                entries.append({"name": rname, "n": int(n), "min": int(mn), "max": int(mx), "mean_bits": int(mean),
                                "var_bits": int(var), "sd_bits": int(sd), "nex": None if int(nex) < 0 else int(nex)})
            assert len(entries) == len(reads)
            doc["sets"].append({"name": name, "reads": entries, "raw": parse_table(raw_text), "delta": parse_table(delta_text),
                                "raw_text": raw_text, "delta_text": delta_text})
            print(name, len(reads), "reads", len(doc["sets"][-1]["raw"]), "raw rows", len(doc["sets"][-1]["delta"]), "delta rows",
                  file=sys.stderr)
    with open(os.path.join(HERE, "viz_tally.json"), "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
