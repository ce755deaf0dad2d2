#!/usr/bin/env python3
"""Generate tests/golden/ref_huffman.json from the REAL reference: the four per-read Huffman methods
huffman_{vbe21, vbbe21, vbsbe21, vbsse21}_zd (press/press.h:602-631, press.c:3960-4407, huffman/huffman.c:984-1072).

Run in the build container only (needs /root/reference, gcc and the objects `make -C oracle ref` leaves in oracle/_ref):

    python tests/golden/make_huffman_golden.py

The few lines of DRIVER below are linked in a temporary directory with the reference's objects in oracle/_ref and with
Turbo-Range-Coder/rccdf.c as make_rcf_golden.py compiles it, which top_press.o refers to.

Nothing of the reference is committed: the fixture holds DATA - per read its name, n, a sha256 of its samples, and per
method the stream's length, the longest code of its table, the sha256 of the stream, whether the reference's own depress
gives the read back, and for reads under 64 samples the stream itself.  Every read runs in a child process.  A read the
reference dies on in press (one distinct one-byte value: it aborts) is recorded as "reference": "aborts", with the stream
include/press_hip.h section (2v) defines for it, made by tests/_dhuf.py.

The reads are tests/_dhuf.named_reads().
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

import _dhuf  # noqa: E402
import _rcf  # noqa: E402

PRESS = "/root/reference/press"
REFOBJ = os.path.join(ROOT, "oracle", "_ref")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
typedef int (*press_fn)(const int16_t *, uint32_t, uint8_t *, uint64_t *);
typedef int (*depress_fn)(uint8_t *, uint64_t, int16_t *, uint32_t *);
#define DECL(l) int huffman_##l##_zd_press_16(const int16_t *, uint32_t, uint8_t *, uint64_t *); \
                int huffman_##l##_zd_depress_16(uint8_t *, uint64_t, int16_t *, uint32_t *);
#define ALL(X) X(vbe21) X(vbbe21) X(vbsbe21) X(vbsse21)
ALL(DECL)
#define PFN(l) huffman_##l##_zd_press_16,
#define DFN(l) huffman_##l##_zd_depress_16,
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
        if (P[m](s, (uint32_t) n, out, &len)) return 3;
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
    if (D[m](in, (uint64_t) len, back, &got)) return 1;
    return got == n && !memcmp(back, s, 2 * n) ? 0 : 1;
}
"""


def build(tmp):
    drv = os.path.join(tmp, "driver.c")
    cdf = os.path.join(tmp, "rccdf.o")
    exe = os.path.join(tmp, "huffman_ref")
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
        """-> (stream, the reference's depress gives the read back), or (None, False) where press dies on a signal"""
        s.tofile(self.fin)
        rc = subprocess.run([self.exe, "press", str(l), self.fin, self.fout], stderr=subprocess.DEVNULL).returncode
        if rc < 0:
            return None, False
        assert rc == 0, rc
        stream = open(self.fout, "rb").read()
        back = subprocess.run([self.exe, "back", str(l), self.fin, self.fout], stderr=subprocess.DEVNULL).returncode
        return stream, back == 0


def main():
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        ref = Ref(build(tmp), tmp)
        for rname, s in _dhuf.named_reads():
            s = np.ascontiguousarray(s, dtype=np.int16)
            e = {"name": rname, "n": int(len(s)), "samples_sha256": _rcf.sha(s.tobytes()), "methods": {}}
            for l, layout in enumerate(_rcf.LAYOUTS):
                stream, back = ref.press(l, s)
                if stream is None:
                    stream, maxlen = _dhuf.expected(layout, s)
                    f = {"reference": "aborts", "len": len(stream), "maxlen": maxlen, "sha256": _rcf.sha(stream), "roundtrip": False}
                else:
                    table = _dhuf.parse_table(stream[_dhuf.head_len(layout, s):])
                    maxlen = max([ln for _, ln, _ in table[0]] + [0])
                    f = {"reference": "ok", "len": len(stream), "maxlen": maxlen, "sha256": _rcf.sha(stream), "roundtrip": back}
                if len(s) < 64:
                    f["stream"] = stream.hex()
                e["methods"][_dhuf.name(layout)] = f
            entries.append(e)
            print(rname, e["n"], {m: (f["reference"], f["len"], f["maxlen"], f["roundtrip"]) for m, f in e["methods"].items()},
                  file=sys.stderr)
    doc = {"source": "press/press.c huffman_{vbe21,vbbe21,vbsbe21,vbsse21}_zd_press_16 and their depress; the reference's objects as "
                     "oracle/Makefile builds them, linked with a driver of a few lines (tests/golden/make_huffman_golden.py).  "
                     "reference: ok, or aborts (press dies: one distinct one-byte value) - then len, maxlen and sha256 are those "
                     "of the stream include/press_hip.h (2v) defines.  roundtrip: the reference's own depress gives the read back",
           "entries": entries}
    with open(os.path.join(HERE, "ref_huffman.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
