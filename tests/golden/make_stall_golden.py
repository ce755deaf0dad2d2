#!/usr/bin/env python3
"""Generate tests/golden/ref_stall.json from the REAL reference: the stall methods rccm_svbbe21_zd, dstall_fz_1500 and
dstall_fz (press/press.c:7716-8148) over sigtk's jnn_raw (press/sigtk/src/jnn.c).

Run in the build container only (needs /root/reference, gcc and the objects `make -C oracle ref` leaves in oracle/_ref):

    python tests/golden/make_stall_golden.py

The few lines of DRIVER below are compiled with jnn.c (as it is, gcc -O2) and linked with the reference's objects in
oracle/_ref, into a temporary directory.  Nothing of the reference is committed: the fixture holds DATA - per read its
name, n, a sha256 of its samples, the segments jnn_raw finds (count and the first), and per method the stream's length,
its sha256, its header fields, its first 32 bytes and whether the reference's own depress gives the read back.

A read with no segment (nseg = 0) gets NO stall streams: the reference compares an uninitialised stall_len there
(press.c:7737, 7763), so what it writes is no function of the read.  The library's definition 1 (no segment: no stall)
is tested against the yardstick instead, whose inner stream the oracle's rccm_vbbe21_zd pins.

The reads are tests/_stall.named_reads(): the three real reads, the non-empty reads of _layouts.battery() and the
generated ones; each generated read's aimed-at first segment is checked against jnn_raw here, and a read that misses is an
error.  A tie of dstall_fz's two forms is searched for among _stall.tie_candidates() and named in "tie" (null: none found).
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

import _stall  # noqa: E402

PRESS = "/root/reference/press"
SIGTK = PRESS + "/sigtk"
REFOBJ = os.path.join(ROOT, "oracle", "_ref")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "error.h"
#include "jnn.h"
enum sigtk_log_level_opt get_log_level() { return (enum sigtk_log_level_opt) 0; }
typedef void (*press_fn)(const int16_t *, uint32_t, uint8_t *, uint64_t *);
typedef void (*depress_fn)(uint8_t *, uint64_t, int16_t *, uint32_t *);
void rccm_svbbe21_zd_press_16(const int16_t *, uint32_t, uint8_t *, uint64_t *);
void dstall_fz_1500_press_16(const int16_t *, uint32_t, uint8_t *, uint64_t *);
void dstall_fz_press_16(const int16_t *, uint32_t, uint8_t *, uint64_t *);
void rccm_svbbe21_zd_depress_16(uint8_t *, uint64_t, int16_t *, uint32_t *);
void dstall_fz_1500_depress_16(uint8_t *, uint64_t, int16_t *, uint32_t *);
void dstall_fz_depress_16(uint8_t *, uint64_t, int16_t *, uint32_t *);
static void *slurp(const char *path, size_t es, size_t *n)
{
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    *n = (size_t) ftell(f) / es;
    fseek(f, 0, SEEK_SET);
    void *p = calloc(*n * es + 64, 1);
    if (fread(p, es, *n, f) != *n) exit(2);
    fclose(f);
    return p;
}
/* driver seg in out | press k in out | back k in stream (exit 0: the read comes back, 1: it does not) */
int main(int argc, char **argv)
{
    static const press_fn P[3] = { rccm_svbbe21_zd_press_16, dstall_fz_1500_press_16, dstall_fz_press_16 };
    static const depress_fn D[3] = { rccm_svbbe21_zd_depress_16, dstall_fz_1500_depress_16, dstall_fz_depress_16 };
    if (argc < 4) return 2;
    size_t n;
    if (!strcmp(argv[1], "seg")) {
        int16_t *s = (int16_t *) slurp(argv[2], 2, &n);
        jnn_param_t prm = JNNV1_CDNA_PARAM;
        int k = 0;
        jnn_pair_t *segs = jnn_raw(s, (int64_t) n, prm, &k);
        long long v[3] = { k, k ? (long long) segs[0].x : 0, k ? (long long) segs[0].y : 0 };
        FILE *o = fopen(argv[3], "wb");
        if (!o) return 2;
        fwrite(v, 8, 3, o);
        fclose(o);
        return 0;
    }
    int m = atoi(argv[2]);
    int16_t *s = (int16_t *) slurp(argv[3], 2, &n);
    if (!strcmp(argv[1], "press")) {
        uint64_t cap = 8 * (uint64_t) n + 4096, len = cap;
        uint8_t *out = calloc(cap + 64, 1);
        P[m](s, (uint32_t) n, out, &len);
        FILE *o = fopen(argv[4], "wb");
        if (!o) return 2;
        fwrite(out, 1, len, o);
        fclose(o);
        return 0;
    }
    size_t len;
    uint8_t *in = (uint8_t *) slurp(argv[4], 1, &len);
    int16_t *back = calloc(n + 64, 2);
    uint32_t got = (uint32_t) n;
    D[m](in, (uint64_t) n, back, &got);
    return got == n && !memcmp(back, s, 2 * n) ? 0 : 1;
}
"""


def build(tmp):
    drv = os.path.join(tmp, "driver.c")
    exe = os.path.join(tmp, "stall_ref")
    open(drv, "w").write(DRIVER)
    objs = [os.path.join(REFOBJ, f) for f in sorted(os.listdir(REFOBJ))
            if f.endswith(".o") and (f.startswith("top_") or f.startswith("svb_") or f in ("huffman.o", "svb16.o", "rc_s.o", "rccm_s.o"))]
    assert objs, "run `make -C oracle ref` first"
    subprocess.run(["gcc", "-O2", "-w", "-I", os.path.join(SIGTK, "src"), "-I", os.path.join(SIGTK, "slow5lib", "include"),
                    os.path.join(SIGTK, "src", "jnn.c"), drv] + objs +
                   ["-o", exe, "-Wl,--gc-sections", "-L/opt/conda/lib", "-Wl,-rpath,/opt/conda/lib", "-lzstd", "-lz", "-lm"], check=True)
    return exe


class Ref:
    def __init__(self, exe, tmp):
        self.exe, self.fin, self.fout = exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")

    def segs(self, s):
        s.tofile(self.fin)
        subprocess.run([self.exe, "seg", self.fin, self.fout], check=True, stderr=subprocess.DEVNULL)
        k, x, y = (int(v) for v in np.fromfile(self.fout, dtype="<i8"))
        return k, (x, y)

    def press(self, k, s):
        """-> (stream, the reference's depress gives the read back)"""
        s.tofile(self.fin)
        subprocess.run([self.exe, "press", str(k), self.fin, self.fout], check=True, stderr=subprocess.DEVNULL)
        stream = open(self.fout, "rb").read()
        back = subprocess.run([self.exe, "back", str(k), self.fin, self.fout], stderr=subprocess.DEVNULL).returncode == 0
        return stream, back


def entry(ref, name, s):
    k, first = ref.segs(s)
    e = {"name": name, "n": int(len(s)), "samples_sha256": _stall.sha(s.tobytes()), "nseg": k, "first": list(first) if k else None}
    if k:
        e["methods"] = {}
        for i, m in enumerate(_stall.STALL_METHODS):
            stream, back = ref.press(i, s)
            f = {"len": len(stream), "sha256": _stall.sha(stream), "first32": stream[:32].hex(), "roundtrip": back}
            ex = stream[0]
            f["exists"] = ex
            if ex:
                f["stall_start"], f["stall_len"], f["nstall"] = struct.unpack_from("<HHH", stream, 1)
            e["methods"][m] = f
    return e


def main():
    entries = []
    tie = None
    with tempfile.TemporaryDirectory() as tmp:
        ref = Ref(build(tmp), tmp)
        # the generated reads meet their design
        for name, s, aim in _stall.generated_reads():
            k, first = ref.segs(s)
            assert aim is None or (k >= 1 and first == aim), (name, k, first, aim)
        # a tie of dstall_fz's two forms: the T = 140 stream as long as the bare rccm_vbbe21_zd stream
        for name, s in _stall.tie_candidates():
            k, _ = ref.segs(s)
            if not k:
                continue
            st, _ = ref.press(0, s)
            fz, _ = ref.press(2, s)
            if st[0] == 1 and fz[0] == 0 and len(st) == len(fz) - 5:
                tie = name
                print("tie:", name, len(st), file=sys.stderr)
                break
        doc = {"tie": tie}
        _stall._fx["f"] = doc  # (named_reads() reads the tie's name from the fixture)
        for name, s in _stall.named_reads():
            e = entry(ref, name, s)
            entries.append(e)
            print(name, e["n"], e["nseg"], {m: (f["len"], f["exists"], f["roundtrip"]) for m, f in e.get("methods", {}).items()},
                  file=sys.stderr)
    doc.update({"source": "press/press.c rccm_svbbe21_zd_press_16, dstall_fz_1500_press_16, dstall_fz_press_16 and their depress "
                          "over press/sigtk/src/jnn.c jnn_raw(JNNV1_CDNA_PARAM); the reference's objects as oracle/Makefile "
                          "builds them, jnn.c with gcc -O2.  nseg = 0: no streams recorded (the reference reads an "
                          "uninitialised stall_len there).  tie: "
                          + ("the read whose two dstall_fz forms are equally long" if tie else
                             "none found among _stall.tie_candidates(); the tie rule is tested on _stall.choose alone"),
                "entries": entries})
    with open(os.path.join(HERE, "ref_stall.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
