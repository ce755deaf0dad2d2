#!/usr/bin/env python3
"""bench.py's e2e_blow5 leg alone:  python3 tools/e2e_blow5.py [--recode [--packed]] [reads] [reads per batch]

--recode: every batch goes through ONE press_hip_recode_batch call (BLOW5's svb-zd fields in, the target method's
streams out, the samples kept for the check) instead of press_hip_depress_batch + press_hip_press_batch.
--packed (with --recode): that call is press_hip_recode_packed: the leg's slot table is only the room the library lays
the streams out in, back to back, and is overwritten with their offsets."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class RecodeCalls:
    """honours_amd.press as bench.e2e_blow5 uses it, with a depress_batch that only remembers its arguments and a
    press_batch that hands both halves to press.recode_batch"""

    def __init__(self, press, packed=False):
        self._press = press
        self._packed = packed
        self._pending = None

    def __getattr__(self, name):
        return getattr(self._press, name)

    def depress_batch(self, method, comp, in_off, in_len, sig, off, n, out_n):
        self._pending = (method, comp, in_off, in_len, sig, off, n, out_n)

    def press_batch(self, method, sig, off, n, out, out_off, out_len):
        if self._pending is None:  # (the leg's own preparation of the file: samples in)
            return self._press.press_batch(method, sig, off, n, out, out_off, out_len)
        src, comp, in_off, in_len, dsig, doff, dn, out_n = self._pending
        self._pending = None
        assert dsig.data_ptr() == sig.data_ptr() and doff.data_ptr() == off.data_ptr()
        call = self._press.recode_packed if self._packed else self._press.recode_batch
        call(src, method, comp, in_off, in_len, dn, doff, out, out_off, out_len, out_n, sig=dsig)


def main():
    argv = [a for a in sys.argv[1:] if a not in ("--recode", "--packed")]
    recode, packed = "--recode" in sys.argv[1:], "--packed" in sys.argv[1:]
    if packed and not recode:
        sys.exit("--packed needs --recode")
    reads = int(argv[0]) if len(argv) > 0 else 2048
    per = int(argv[1]) if len(argv) > 1 else 512
    import torch

    import bench
    from honours_amd import press, synth

    if not torch.cuda.is_available():
        sys.exit("e2e_blow5 needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    press.load_library()
    press.use_torch_stream()
    b = bench.Batch(torch, press, synth, 20261004, 0, reads, dev, None)
    rec = bench.e2e_blow5(torch, RecodeCalls(press, packed) if recode else press, b, "shuffman_vbe21_zd", nreads=reads, batch_reads=per)
    if rec is not None:
        rec["calls"] = "press_hip_recode_packed" if packed else "press_hip_recode_batch" if recode else "press_hip_depress_batch + press_hip_press_batch"
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
