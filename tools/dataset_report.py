#!/usr/bin/env python3
"""What a BLOW5 file's signal data looks like, tallied on the device (press.dataset_report).

    python3 tools/dataset_report.py FILE [--tsv DIR] [--max-reads 4096]

Prints the read and sample counts, the eleven numbers of viz/freq_analyse.R for the raw values, the deltas and the coded
symbols, the order-0 and order-1 entropy of the symbol stream, and bits per sample and 16 / H for each.  With --tsv it
writes into DIR
  raw.freq, delta.freq   the frequency tables in the form viz/freq_slow5 and viz/freq_delta_slow5 print them: a header
                         signal<TAB>freq, ascending values, zero rows omitted - they diff against the reference's output
  stats.tsv              one row per read: id, n, min, max, mean, var, sd, nex and the picoampere forms of viz/stats.c
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUMMARY = ("n", "min", "q1", "mean", "median", "q3", "max", "mode", "var", "std", "entropy")
STATS = ("mean", "var", "sd", "min_pa", "max_pa", "mean_pa", "var_pa", "sd_pa")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file")
    ap.add_argument("--tsv", default=None, metavar="DIR")
    ap.add_argument("--max-reads", type=int, default=4096)
    a = ap.parse_args()
    from honours_amd import press

    rep = press.dataset_report(a.file, max_reads=a.max_reads)
    print("reads\t%d" % rep["reads"])
    print("samples\t%d" % rep["samples"])
    print("exceptions\t%d" % int(rep["mom"]["nex"].astype("u8").sum()))
    for name in ("raw", "delta", "symbol"):
        print("\n# %s" % name)
        for k in SUMMARY:
            print("%s\t%s" % (k, rep[name + "_summary"][k]))
    print("\n# symbol stream (257 classes)")
    print("entropy order 0\t%.6f" % rep["h0"])
    print("entropy order 1\t%.6f" % rep["h1"])
    print("\n# bits per sample, and 16 / H")
    for k, bits in rep["bits"].items():
        print("%s\t%.6f\t%.4f" % (k, bits, rep["ratio"][k]))
    if a.tsv:
        os.makedirs(a.tsv, exist_ok=True)
        for name in ("raw", "delta"):
            with open(os.path.join(a.tsv, name + ".freq"), "w") as f:
                f.write(press.tally_text(rep[name]))
        st, mom = rep["stats"], rep["mom"]
        cols = [k for k in STATS if k in st]
        with open(os.path.join(a.tsv, "stats.tsv"), "w") as f:
            f.write("\t".join(("id", "n", "min", "max") + tuple(cols[:3]) + ("nex",) + tuple(cols[3:])) + "\n")
            for r, rid in enumerate(rep["ids"]):
                m = mom[r]
                row = [rid, "%d" % m["n"], "%d" % m["min"], "%d" % m["max"]] + ["%f" % st[k][r] for k in cols[:3]] + ["%d" % m["nex"]]
                f.write("\t".join(row + ["%f" % st[k][r] for k in cols[3:]]) + "\n")


if __name__ == "__main__":
    main()
