"""Build libpress_hip.so (HIP kernels + C ABI) for gfx950, in-tree.

    python -m honours_amd.build

hipcc cross-compiles without a GPU; the .so is git-ignored but travels to the GPU box.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libpress_hip.so")
SOURCES = ["press_sections.hip", "press_svb.hip", "press_exsplit.hip", "press_pa.hip", "press_huffman.hip", "press_rc.hip", "press_zstd.hip", "press_train.hip", "press_packed.hip", "press_stats.hip", "press_quant.hip", "press_rows.hip", "press_trim.hip", "press_verify.hip", "press_degrade.hip", "press_events.hip", "press_segments.hip", "press_ranges.hip", "press_stall.hip",
           "press_ctx.hip", "press_methods.hip", "press_staging.hip", "press_batch.hip", "press_table.hip", "press_dropin.hip", "blow5_reader.cpp", "press_crc.cpp", "press_tally.hip", "press_rice.hip", "press_dhuf.hip", "press_deflate.hip", "press_inflate.hip", "press_cdf.hip"]
HEADERS = ["press_internal.h", "press_host.h", "press_packed.h", "press_chunk.h", "press_wave.h", "press_segwalk.h", "zs_table.h", "press_crc.h", "press_rice_walk.h", "press_dhuf_walk.h", "press_inflate_walk.h", "press_prefix.h", os.path.join("..", "..", "include", "press_hip.h")]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def build(force=False, verbose=False):
    """Compile the library if it is missing or older than its sources. Returns its path."""
    if not force and not _stale():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall",
           "-Wno-unused-function", "-Wno-cast-align"] + [os.path.join(CSRC, f) for f in SOURCES] + ["-o", LIB, "-ldl"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
