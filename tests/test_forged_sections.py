"""Forged exception sections on the device (include/press_hip.h at out_n of press_hip_depress_batch).

The corpus of tests/_forge.py - every refusal condition of the section parser as the deciding one, each with its
well-formed twin - goes through press_hip_depress_batch in ONE device-resident call per method: every forged read
between two good reads, the streams back to back, the rooms back to back on the 8-sample grid, the samples prefilled.
The oracle is the yardstick (tests/test_forged_oracle.py pins its verdicts to the builders' intentions on the CPU):
out_n is UINT32_MAX exactly where it refuses, elsewhere count and samples are its own, the good neighbours are bit
exact, nothing outside the rooms is written, the call succeeds and the good reads decode alone afterwards.  The same
batch runs once more in reversed order.  One pair per section format goes through press_hip_recode_sizes /
press_hip_recode_packed, and vbe21_zd through press_hip_depress_pa_batch.
"""
import numpy as np
import pytest

import _forge as F
import _layouts as L
import test_depress_pa as PA
import test_recode as R
import test_press_packed as P
import test_recode_packed as RP
from honours_amd import press

gpu = pytest.mark.gpu
F32 = L.FAILED32
FILL = np.int16(L.SIG_FILL)
LEAD = 8  # samples in front of the first room


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lb = press.load_library()
    press.load_table()
    press.use_torch_stream()
    yield lb
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _t(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a if dtype is None else a.view(dtype)).copy()).cuda()


class Batch:
    """reads as one arena of streams back to back and rooms back to back, with what the oracle says of each"""

    def __init__(self, oracle, m, items):
        self.m, self.names = m, [it[0] for it in items]
        self.expect = []
        for name, st, room in items:
            ret, back = oracle.depress(m, st, room)
            self.expect.append(back if ret == 0 else None)
        self.in_len = np.array([len(st) for _, st, _ in items], dtype=np.uint64)
        self.in_off = np.concatenate([[0], np.cumsum(self.in_len)[:-1]]).astype(np.uint64)
        self.inb = np.frombuffer(b"".join(st for _, st, _ in items) + bytes([L.ARENA_FILL]) * 64, dtype=np.uint8)
        self.rooms = np.array([room for _, _, room in items], dtype=np.uint32)
        span = np.array([L.roundup8(r) for r in self.rooms], dtype=np.uint64)
        self.off = (LEAD + np.concatenate([[0], np.cumsum(span)[:-1]])).astype(np.uint64)
        self.total = int(self.off[-1] + span[-1]) + 64
        self.outside = L.outside_rooms(self.total, self.off, span)

    def dev(self):
        return (_t(self.inb), _t(self.in_off, np.int64), _t(self.in_len, np.int64), _t(self.off, np.int64),
                _t(self.rooms, np.int32))

    def decode(self, lib):
        import torch
        d_in, d_io, d_il, d_off, d_n = self.dev()
        d_sig = torch.full((self.total,), L.SIG_FILL, dtype=torch.int16, device="cuda")
        d_on = torch.full((len(self.rooms),), 7, dtype=torch.int32, device="cuda")
        rc = PA.i16_call(lib, self.m, d_in, d_io, d_il, d_sig, d_off, d_n, self.total, d_on, True)
        assert rc == 0, (self.m, press.last_error())
        torch.cuda.synchronize()
        return d_sig.cpu().numpy(), d_on.cpu().numpy().view(np.uint32)

    def check(self, sig, out_n):
        wrong = [(self.names[k], int(out_n[k]), None if e is None else e.size) for k, e in enumerate(self.expect)
                 if int(out_n[k]) != (F32 if e is None else e.size)]
        assert not wrong, (self.m, len(wrong), wrong[:40])
        for k, e in enumerate(self.expect):
            if e is not None:
                o = int(self.off[k])
                assert np.array_equal(sig[o:o + e.size], e), (self.m, self.names[k])
        bad = np.nonzero(sig[self.outside] != FILL)[0]
        assert bad.size == 0, (self.m, "samples written outside the rooms", bad[:8])


@gpu
@pytest.mark.parametrize("m", F.METHODS)
def test_forged_reads_between_good_ones(lib, oracle, m):
    good, items = F.interleaved(oracle, m)
    assert len(items) <= 700
    for order in (items, items[::-1]):
        b = Batch(oracle, m, order)
        refused = sum(e is None for e in b.expect)
        assert refused >= 20 and len(order) - refused >= len(order) // 2 + 10, (m, refused)
        b.check(*b.decode(lib))
    alone = Batch(oracle, m, good)
    assert all(e is not None for e in alone.expect)
    alone.check(*alone.decode(lib))


RECODE_PAIRS = [("vbe21_zd", "svb12_zd"), ("vbbe21_zd", "svb12_zd"), ("vbsbe21_zd", "svb12_zd"), ("vbsse21_zd", "svb12_zd"),
                ("hasgam_vbsse21_zdq", "slow5_svb_zd")]


@gpu
@pytest.mark.parametrize("src,dst", RECODE_PAIRS)
def test_recode_of_forged_sources(lib, oracle, src, dst):
    """a refused source read: need = out_len = FAILED, no byte of the arena (RP.Dev checks the layout, every stream
    against the oracle's `dst` stream of the oracle's samples, and that nothing else is written)"""
    rng = np.random.default_rng(900 + press.METHODS[src])
    _, items = F.interleaved(oracle, src)
    ents = []
    for name, st, room in items:
        ret, back = oracle.depress(src, st, room)
        if ret != 0:
            ents.append(R.Entry(name, st, room, 0, F32, None, None))
        else:
            want = R.want_press(oracle, dst, back)
            assert want is not None, (src, dst, name)
            ents.append(R.Entry(name, st, room, 0, len(back), back, want))
    assert sum(e.out_n == F32 for e in ents) >= 20
    dev = RP.dev_of(oracle, src, dst, ents, rng)
    need = dev.sizes(lib, keep_sig=True)
    assert all(int(need[k]) == L.FAILED64 for k, e in enumerate(ents) if e.out_n == F32)
    exp = P.layout_of(need, 1)
    assert all(exp[k + 1] == exp[k] for k, e in enumerate(ents) if e.out_n == F32)
    dev.packed(lib, need, 1)


@gpu
def test_forged_reads_to_picoamperes(lib, oracle):
    """press_hip_depress_pa_batch, vbe21_zd: a refused read gets no float, an accepted one the floats of the samples
    press_hip_depress_batch gives"""
    import torch
    m = "vbe21_zd"
    _, items = F.interleaved(oracle, m)
    b = Batch(oracle, m, items)
    sig, out_n = b.decode(lib)
    b.check(sig, out_n)
    cal = PA.batch_cal(len(items))
    d_in, d_io, d_il, d_off, d_n = b.dev()
    d_pa = torch.full((b.total,), PA.CANARY, dtype=torch.int32, device="cuda")
    d_on = torch.full((len(items),), 7, dtype=torch.int32, device="cuda")
    rc = PA.pa_call(lib, m, d_in, d_io, d_il, d_pa, d_off, d_n, b.total, _t(cal.reshape(-1)), d_on, True)
    assert rc == 0, press.last_error()
    torch.cuda.synchronize()
    bits, on = d_pa.cpu().numpy().view(np.uint32), d_on.cpu().numpy().view(np.uint32)
    assert np.array_equal(on, out_n)
    for k, cnt in enumerate(on):
        o, span = int(b.off[k]), L.roundup8(int(b.rooms[k]))
        if int(cnt) == F32:
            assert (bits[o:o + span] == PA.CANARY).all(), b.names[k]
        else:
            assert np.array_equal(bits[o:o + int(cnt)], PA.pa_bits(sig[o:o + int(cnt)], cal[k, 0], cal[k, 1])), b.names[k]
    assert (bits[b.outside] == PA.CANARY).all()
