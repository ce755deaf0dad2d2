#!/usr/bin/env python3
"""Generate tests/golden/ref_rice.json from the REAL reference: the four Golomb-Rice methods
rice_{vbe21, vbbe21, vbsbe21, vbsse21}_zd (press/press.h:664-701, press.c:4854-5390).

Run in the build container only (needs /root/reference, gcc and the objects `make -C oracle ref` leaves in oracle/_ref):

    python tests/golden/make_rice_golden.py

The few lines of DRIVER below are linked in a temporary directory with the reference's objects in oracle/_ref
(top_press.o holds all four methods) and with Turbo-Range-Coder/rccdf.c as make_rcf_golden.py compiles it, which
top_press.o refers to.

Nothing of the reference is committed: the fixture holds DATA - per read its name, n, a sha256 of its samples, and per
method the stream's length, k (the payload's first three bits), nbits % 8 (nbits = 3 + the sum of the code lengths at that k,
from the read's one-byte values), the sha256 of the stream with the bits behind nbits in its last byte cleared - the
reference leaves there what its uninitialised block held -, whether the reference's own depress gives the read back,
and for reads under 64 samples the cleared stream itself.  Every read runs in a child process; a read the reference
dies on is an error of this generator, not a fixture entry.

The reads are tests/_rice.named_reads().
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

import _rcf  # noqa: E402
import _rice  # noqa: E402

PRESS = "/root/reference/press"
REFOBJ = os.path.join(ROOT, "oracle", "_ref")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
typedef void (*press_fn)(const int16_t *, uint32_t, uint8_t *, uint64_t *);
typedef void (*depress_fn)(uint8_t *, uint64_t, int16_t *, uint32_t *);
#define DECL(l) void rice_##l##_zd_press_16(const int16_t *, uint32_t, uint8_t *, uint64_t *); \
                void rice_##l##_zd_depress_16(uint8_t *, uint64_t, int16_t *, uint32_t *);
#define ALL(X) X(vbe21) X(vbbe21) X(vbsbe21) X(vbsse21)
ALL(DECL)
#define PFN(l) rice_##l##_zd_press_16,
#define DFN(l) rice_##l##_zd_depress_16,
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
/* driver press l in out | back l in stream (exit 0: the read comes back, 1: it does not) */
int main(int argc, char **argv)
{
    static const press_fn P[4] = { ALL(PFN) };
    static const depress_fn D[4] = { ALL(DFN) };
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
    D[m](in, (uint64_t) n, back, &got); /* (the SAMPLE count: press.c:5050) */
    return got == n && !memcmp(back, s, 2 * n) ? 0 : 1;
}
"""


def build(tmp):
    drv = os.path.join(tmp, "driver.c")
    cdf = os.path.join(tmp, "rccdf.o")
    exe = os.path.join(tmp, "rice_ref")
    open(drv, "w").write(DRIVER)
    objs = [os.path.join(REFOBJ, f) for f in sorted(os.listdir(REFOBJ))
            if f.endswith(".o") and (f.startswith("top_") or f.startswith("svb_") or f in ("huffman.o", "svb16.o", "rc_s.o", "rccm_s.o"))]
    assert objs, "run `make -C oracle ref` first"
    subprocess.run(["gcc", "-O2", "-w", "-fPIC", "-ffunction-sections", "-c",
                    os.path.join(PRESS, "Turbo-Range-Coder", "rccdf.c"), "-o", cdf], check=True)
    subprocess.run(["gcc", "-O2", "-w", drv, cdf] + objs +
                   ["-o", exe, "-Wl,--gc-sections", "-L/opt/conda/lib", "-Wl,-rpath,/opt/conda/lib", "-lzstd", "-lz", "-lm"], check=True)
    return exe


class Ref:
    def __init__(self, exe, tmp):
        self.exe, self.fin, self.fout = exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")

    def press(self, l, s):
        """-> (stream, the reference's depress gives the read back); a child that dies in press is an error"""
        s.tofile(self.fin)
        subprocess.run([self.exe, "press", str(l), self.fin, self.fout], check=True, stderr=subprocess.DEVNULL)
        stream = open(self.fout, "rb").read()
        back = subprocess.run([self.exe, "back", str(l), self.fin, self.fout], stderr=subprocess.DEVNULL).returncode
        return stream, back == 0


def main():
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        ref = Ref(build(tmp), tmp)
        for rname, s in _rice.named_reads():
            s = np.ascontiguousarray(s, dtype=np.int16)
            e = {"name": rname, "n": int(len(s)), "samples_sha256": _rcf.sha(s.tobytes()), "methods": {}}
            low = np.frombuffer(_rcf.split("vbe21", s)[1], dtype=np.uint8).astype(np.int64)
            for l, layout in enumerate(_rcf.LAYOUTS):
                stream, back = ref.press(l, s)
                head = _rice.head_len(layout, s)
                b = stream[head]
                k = (b & 1) << 2 | (b & 2) | (b >> 2) & 1
                nbits = 3 + int((low >> k).sum()) + len(low) * (1 + k)
                assert len(stream) == head + (nbits - 1) // 8 + 1, (rname, layout)
                clean = _rice.clear_padding(stream, nbits)
                f = {"len": len(stream), "k": k, "nbits_mod8": nbits % 8, "sha256": _rcf.sha(clean), "roundtrip": back}
                if len(s) < 64:
                    f["stream"] = clean.hex()
                e["methods"][_rice.name(layout)] = f
            entries.append(e)
            print(rname, e["n"], {m: (f["len"], f["k"], f["roundtrip"]) for m, f in e["methods"].items()}, file=sys.stderr)
    doc = {"source": "press/press.c rice_{vbe21,vbbe21,vbsbe21,vbsse21}_zd_press_16 and their depress (given the sample count, "
                     "press.c:5050); the reference's objects as oracle/Makefile builds them, linked with a driver of a few lines "
                     "(tests/golden/make_rice_golden.py).  sha256 and stream: the stream with the bits behind nbits in its last "
                     "byte cleared (the reference leaves heap contents there).  roundtrip: the reference's own depress gives the "
                     "read back",
           "entries": entries}
    with open(os.path.join(HERE, "ref_rice.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
