#!/usr/bin/env python3
"""bench.py's e2e_blow5 leg alone:  python3 tools/e2e_blow5.py [--recode [--packed]] [--inflate device] [reads] [reads per batch]

--recode: every batch goes through ONE press_hip_recode_batch call (BLOW5's svb-zd fields in, the target method's
streams out, the samples kept for the check) instead of press_hip_depress_batch + press_hip_press_batch.
--packed (with --recode): that call is press_hip_recode_packed: the leg's slot table is only the room the library lays
the streams out in, back to back, and is overwritten with their offsets.
--inflate device: the leg's reader hands out the records AS STORED (press_hip_blow5_next_stored) and the device inflates
and parses them (press_hip_blow5_inflate_batch, press_hip_blow5_record_fields; Blow5Reader.next_batch_device): the host
pool's inflate and the copy of the inflated fields are gone, the stored records go up instead."""
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


class DeviceInflate:
    """honours_amd.press as bench.e2e_blow5 uses it, with a Blow5Reader whose next_arena inflates on the device: it leaves
    the leg's page-locked arena alone (the leg copies 64 bytes of it), reports the sample counts, and keeps the record
    arena and the fields' table for the depress_batch that follows, which reads them in the place of the leg's copy"""

    def __init__(self, press):
        import collections

        self._press = press
        self._batches = collections.deque()
        outer = self

        class Reader(press.Blow5Reader):
            def next_arena(self, arena, off, ln, ns, max_reads):
                b = self.next_batch_device(max_reads, arena_bytes=1 << 28)
                if b is None:
                    return 0
                got = len(b["ids"])
                ns[:got] = b["n_samples"].cpu().numpy().view(ns.dtype)  # (synchronises: the batch is whole)
                off[:got] = 0
                ln[:got] = 0
                outer._batches.append(b)
                return got

        self.Blow5Reader = Reader

    def __getattr__(self, name):
        return getattr(self._press, name)

    def depress_batch(self, method, comp, in_off, in_len, sig, off, n, out_n):
        b = self._batches.popleft()
        self._press.depress_batch(method, b["rec"], b["sig_off"], b["sig_len"], sig, off, n, out_n)


def main():
    args = sys.argv[1:]
    inflate = "host"
    if "--inflate" in args:
        k = args.index("--inflate")
        if k + 1 >= len(args) or args[k + 1] not in ("host", "device"):
            sys.exit("--inflate host | device")
        inflate = args[k + 1]
        del args[k:k + 2]
    argv = [a for a in args if a not in ("--recode", "--packed")]
    recode, packed = "--recode" in args, "--packed" in args
    if packed and not recode:
        sys.exit("--packed needs --recode")
    if recode and inflate == "device":
        sys.exit("--inflate device goes with the depress + press calls")
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
    calls = DeviceInflate(press) if inflate == "device" else RecodeCalls(press, packed) if recode else press
    rec = bench.e2e_blow5(torch, calls, b, "shuffman_vbe21_zd", nreads=reads, batch_reads=per)
    if rec is not None:
        rec["inflate"] = inflate
        rec["calls"] = "press_hip_recode_packed" if packed else "press_hip_recode_batch" if recode else "press_hip_depress_batch + press_hip_press_batch"
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
