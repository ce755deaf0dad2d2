"""The GPU harness of the two prefix-code families' tests (test_rice_family.py, test_huffman_family.py): a press batch and
a depress batch in scattered layouts with canaries and fills around everything the device writes.  A family is its three
batch wrappers and the name of the byte it reports per read (the Rice parameter "k", the longest code "maxlen")."""
import collections

import numpy as np

import _layouts as L
from honours_amd import press

FAILED64 = (1 << 64) - 1
FAILED32 = (1 << 32) - 1
GUARD = 48
FILL8, FILL16 = 0xA5, 0x5A5A
CANARY = 0x5AC35AC3

Family = collections.namedtuple("Family", "press_batch press_sizes depress_batch table")


def lib():
    """the body of the test modules' `lib` fixture"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.use_torch_stream()
    yield lb
    torch.cuda.synchronize()
    press.use_torch_stream()
    torch.cuda.empty_cache()


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.view(dtype)
    return torch.from_numpy(a.copy()).cuda()


def slot_for(n):
    return 8 * n + 4096 if n else 32


class PressRun:
    """A batch in a scattered layout, the slots back to back from an odd offset; canaries in front of and behind out_len,
    need and the per-read table, and every byte of the arena outside the streams and the slots of failed reads must keep
    its fill"""

    def __init__(self, family, reads, caps=None, seed=1):
        import torch
        rng = np.random.default_rng(seed)
        self.family = family
        self.reads, self.nr = reads, len(reads)
        sig, off = L.scatter_reads(rng, reads)
        caps = [slot_for(len(r)) for r in reads] if caps is None else caps
        self.out_off = L.slots(rng, np.asarray(caps, dtype=np.uint64))
        self.sig, self.off = _t(sig), _t(off.astype(np.uint64), np.int64)
        self.n = _t(np.array([len(r) for r in reads], dtype=np.uint32), np.int32)
        self.d_out_off = _t(self.out_off, np.int64)
        self.out = torch.full((int(self.out_off[-1]) + 64,), FILL8, dtype=torch.uint8, device="cuda")
        self.out_len = torch.full((self.nr + 2 * GUARD,), CANARY, dtype=torch.int64, device="cuda")
        self.tab = torch.full((self.nr + 2 * GUARD,), FILL8, dtype=torch.uint8, device="cuda")

    def _tables(self, want_tab):
        import torch
        torch.cuda.synchronize()
        ol = self.out_len.cpu().numpy().view(np.uint64)
        tab = self.tab.cpu().numpy()
        assert (ol[:GUARD] == CANARY).all() and (ol[GUARD + self.nr:] == CANARY).all(), "out_len / need"
        assert (tab[:GUARD] == FILL8).all() and (tab[GUARD + (self.nr if want_tab else 0):] == FILL8).all(), self.family.table
        self.out_len.fill_(CANARY)
        self.tab.fill_(FILL8)
        return ol[GUARD:GUARD + self.nr].copy(), tab[GUARD:GUARD + self.nr].copy()

    def run(self, layout, want_tab=True):
        """-> (streams (None: failed), the per-read table uint8 [nr])"""
        self.family.press_batch(layout, self.sig, self.off, self.n, self.out, self.d_out_off, self.out_len[GUARD:GUARD + self.nr],
                                self.tab[GUARD:GUARD + self.nr] if want_tab else None)
        ol, tab = self._tables(want_tab)
        out = self.out.cpu().numpy()
        written = np.zeros(len(out), dtype=bool)
        streams = []
        for r in range(self.nr):
            o, cap = int(self.out_off[r]), int(self.out_off[r + 1] - self.out_off[r])
            if ol[r] == FAILED64:
                streams.append(None)
                written[o:o + cap] = True  # (a read that fails may leave its own slot in any state, as the generic calls do)
            else:
                assert ol[r] <= cap
                written[o:o + int(ol[r])] = True
                streams.append(out[o:o + int(ol[r])].tobytes())
        assert (out[~written] == FILL8).all(), "a byte outside the streams was written"
        self.out.fill_(FILL8)
        return streams, tab

    def sizes(self, layout, want_tab=True):
        """-> (need uint64 [nr], the per-read table); the arena keeps its fill"""
        self.family.press_sizes(layout, self.sig, self.off, self.n, self.out_len[GUARD:GUARD + self.nr],
                                self.tab[GUARD:GUARD + self.nr] if want_tab else None)
        need, tab = self._tables(want_tab)
        assert bool((self.out == FILL8).all())
        return need, tab


class DepressRun:
    def __init__(self, family, streams, ns, seed=2):
        import torch
        rng = np.random.default_rng(seed)
        self.family = family
        self.ns = [int(n) for n in ns]
        self.nr = len(streams)
        arena, in_off, in_len = L.scatter_streams(rng, streams)
        self.off, self.total = L.scatter_rooms(rng, self.ns, min_gap=8)
        self.arena, self.in_off, self.in_len = _t(arena), _t(in_off, np.int64), _t(in_len, np.int64)
        self.d_off, self.n = _t(self.off, np.int64), _t(np.array(self.ns, dtype=np.uint32), np.int32)
        self.sig = torch.full((self.total,), FILL16, dtype=torch.int16, device="cuda")
        self.out_n = torch.full((self.nr + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")

    def run(self, layout):
        """-> samples per read (None: refused); nothing outside the rooms of the decoded reads is written"""
        import torch
        self.family.depress_batch(layout, self.arena, self.in_off, self.in_len, self.sig, self.d_off, self.n,
                                  self.out_n[GUARD:GUARD + self.nr])
        torch.cuda.synchronize()
        sig = self.sig.cpu().numpy()
        on = self.out_n.cpu().numpy().view(np.uint32)
        assert (on[:GUARD] == CANARY).all() and (on[GUARD + self.nr:] == CANARY).all(), "out_n"
        on = on[GUARD:GUARD + self.nr]
        got, spans = [], []
        for r in range(self.nr):
            o = int(self.off[r])
            if on[r] == FAILED32:
                got.append(None)
                spans.append(0)
            else:
                assert on[r] == self.ns[r]
                got.append(sig[o:o + self.ns[r]].copy())
                spans.append(self.ns[r])
        assert (sig[L.outside_rooms(self.total, self.off, spans)] == FILL16).all(), "a sample outside the decoded reads was written"
        self.sig.fill_(FILL16)
        self.out_n.fill_(CANARY)
        return got
