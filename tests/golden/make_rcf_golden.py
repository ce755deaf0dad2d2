#!/usr/bin/env python3
"""Generate tests/golden/ref_rcf.json from the REAL reference: the sixteen range-coder methods
{rc, rcc, rccm, rccdf}_{vbe21, vbbe21, vbsbe21, vbsse21}_zd (press/press.h:712-899).

Run in the build container only (needs /root/reference, gcc and the objects `make -C oracle ref` leaves in oracle/_ref):

    python tests/golden/make_rcf_golden.py

The few lines of DRIVER below are compiled with Turbo-Range-Coder/rccdf.c as it lies in the reference (gcc -O2, one
translation unit, libc only) and linked with the reference's objects in oracle/_ref, into a temporary directory.  The CDF
coder's stream depends on a build flag: with __AVX2__ rccdf.c:27-30 switches to a 32-bit range, 14-bit frequencies and
16-bit output.  TurboRC's own makefile leaves AVX2 off (makefile:13), so the reference is the variant WITHOUT it: nothing
here passes -march=native or -mavx2, and the driver refuses to compile where __AVX2__ is defined.

Nothing of the reference is committed: the fixture holds DATA - per read its name, n, a sha256 of its samples, and per
method the stream's length, its sha256, its first 32 bytes and whether the reference's own depress gives the read back.
Every read runs in a child process; a read the reference dies on is an error of this generator, not a fixture entry.

The reads are tests/_rcf.named_reads().
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import _rcf  # noqa: E402

PRESS = "/root/reference/press"
REFOBJ = os.path.join(ROOT, "oracle", "_ref")

GUARD = r"""
#ifdef __AVX2__
#error "the reference stream is that of rccdf.c compiled WITHOUT __AVX2__"
#endif
"""

DRIVER = GUARD + r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
typedef void (*press_fn)(const int16_t *, uint32_t, uint8_t *, uint64_t *);
typedef void (*depress_fn)(uint8_t *, uint64_t, int16_t *, uint32_t *);
#define DECL(c, l) void c##_##l##_zd_press_16(const int16_t *, uint32_t, uint8_t *, uint64_t *); \
                   void c##_##l##_zd_depress_16(uint8_t *, uint64_t, int16_t *, uint32_t *);
#define ROW(X, c) X(c, vbe21) X(c, vbbe21) X(c, vbsbe21) X(c, vbsse21)
#define ALL(X) ROW(X, rc) ROW(X, rcc) ROW(X, rccm) ROW(X, rccdf)
ALL(DECL)
#define PFN(c, l) c##_##l##_zd_press_16,
#define DFN(c, l) c##_##l##_zd_depress_16,
static void *slurp(const char *path, size_t es, size_t *n)
{
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    *n = (size_t) ftell(f) / es;
    fseek(f, 0, SEEK_SET);
    void *p = calloc(*n * es + 4096, 1);
    if (fread(p, es, *n, f) != *n) exit(2);
    fclose(f);
    return p;
}
/* driver press k in out | back k in stream (exit 0: the read comes back, 1: it does not) */
int main(int argc, char **argv)
{
    static const press_fn P[16] = { ALL(PFN) };
    static const depress_fn D[16] = { ALL(DFN) };
    if (argc < 5) return 2;
    size_t n;
    int m = atoi(argv[2]);
    int16_t *s = (int16_t *) slurp(argv[3], 2, &n);
    if (!strcmp(argv[1], "press")) {
        uint64_t cap = 8 * (uint64_t) n + 4096, len = cap;
        uint8_t *out = calloc(cap + 4096, 1);
        P[m](s, (uint32_t) n, out, &len);
        FILE *o = fopen(argv[4], "wb");
        if (!o) return 2;
        fwrite(out, 1, len, o);
        fclose(o);
        return 0;
    }
    size_t len;
    uint8_t *in = (uint8_t *) slurp(argv[4], 1, &len);
    int16_t *back = calloc(n + 4096, 2);
    uint32_t got = (uint32_t) n;
    D[m](in, (uint64_t) len, back, &got);
    return got == n && !memcmp(back, s, 2 * n) ? 0 : 1;
}
"""


def build(tmp):
    drv = os.path.join(tmp, "driver.c")
    cdf = os.path.join(tmp, "rccdf.o")
    exe = os.path.join(tmp, "rcf_ref")
    open(drv, "w").write(DRIVER)
    objs = [os.path.join(REFOBJ, f) for f in sorted(os.listdir(REFOBJ))
            if f.endswith(".o") and (f.startswith("top_") or f.startswith("svb_") or f in ("huffman.o", "svb16.o", "rc_s.o", "rccm_s.o"))]
    assert objs, "run `make -C oracle ref` first"
    # (no -march, no -mavx2: see above; the guard goes in front of rccdf.c itself, whose flags decide the stream)
    guard = os.path.join(tmp, "no_avx2.h")
    open(guard, "w").write(GUARD)
    subprocess.run(["gcc", "-O2", "-w", "-fPIC", "-ffunction-sections", "-include", guard, "-c",
                    os.path.join(PRESS, "Turbo-Range-Coder", "rccdf.c"), "-o", cdf], check=True)
    subprocess.run(["gcc", "-O2", "-w", drv, cdf] + objs +
                   ["-o", exe, "-Wl,--gc-sections", "-L/opt/conda/lib", "-Wl,-rpath,/opt/conda/lib", "-lzstd", "-lz", "-lm"], check=True)
    return exe


class Ref:
    def __init__(self, exe, tmp):
        self.exe, self.fin, self.fout = exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")

    def press(self, k, s):
        """-> (stream, the reference's depress gives the read back); a child that dies in press is an error"""
        s.tofile(self.fin)
        subprocess.run([self.exe, "press", str(k), self.fin, self.fout], check=True, stderr=subprocess.DEVNULL)
        stream = open(self.fout, "rb").read()
        back = subprocess.run([self.exe, "back", str(k), self.fin, self.fout], stderr=subprocess.DEVNULL).returncode
        return stream, back == 0


def main():
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        ref = Ref(build(tmp), tmp)
        for rname, s in _rcf.named_reads():
            e = {"name": rname, "n": int(len(s)), "samples_sha256": _rcf.sha(s.tobytes()), "methods": {}}
            k = 0
            for c in _rcf.CODERS:
                for l in _rcf.LAYOUTS:
                    stream, back = ref.press(k, s)
                    e["methods"][_rcf.name(c, l)] = {"len": len(stream), "sha256": _rcf.sha(stream), "first32": stream[:32].hex(),
                                                     "roundtrip": back}
                    k += 1
            entries.append(e)
            print(rname, e["n"], {m: (f["len"], f["roundtrip"]) for m, f in e["methods"].items()}, file=sys.stderr)
    doc = {"source": "press/press.c {rc,rcc,rccm,rccdf}_{vbe21,vbbe21,vbsbe21,vbsse21}_zd_press_16 and their depress; the reference's "
                     "objects as oracle/Makefile builds them, Turbo-Range-Coder/rccdf.c with gcc -O2 and WITHOUT __AVX2__ (64-bit "
                     "range, 15-bit frequencies, 32-bit output words).  roundtrip: the reference's own depress gives the read back "
                     "(a payload stored raw does not come back)",
           "entries": entries}
    with open(os.path.join(HERE, "ref_rcf.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
