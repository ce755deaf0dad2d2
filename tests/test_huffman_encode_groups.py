"""GPU: the static-Huffman encoder (k_huff_encode_chunked) takes the 16 sub-tiles (512 samples) of a wave's quarter
(8192 samples) in groups, the samples of a whole group behind one wait.  These reads sit on the boundaries of
sub-tiles, groups of two and of four, quarters and chunks (32768 samples); their codes are ordinary, all of the
table's shortest or all of its longest (every lane beyond 64 bits, the staging buffer at its fullest for a whole
group), and their exceptions lie on the first and last samples of those pieces.

Every read is pressed in one device-resident batch into a slot of exactly the stream's length with an empty read's
slot of canary bytes behind it (an empty read fails under these methods and writes nothing); stream bytes and
out_len are the oracle's, and what the device wrote decodes to the read."""
import numpy as np
import pytest

import _layouts as L
from honours_amd import press

pytestmark = pytest.mark.gpu

METHODS = tuple(m for m in press._SYMS if m.startswith("shuff"))
SUB, QUARTER, CHUNK = 512, 8192, 32768
LENGTHS = (1, 2, 7, 8, 9, 511, 512, 513, 2 * SUB - 1, 2 * SUB, 2 * SUB + 1, 4 * SUB - 1, 4 * SUB, 4 * SUB + 1,
           QUARTER - 1, QUARTER, QUARTER + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
CANARY = 32      # bytes of an empty read's slot
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    press.load_library()
    press.load_table()
    press.use_torch_stream()
    yield


def samples_of(deltas, start=500):
    """int16 samples with the given deltas behind sample 0 (16-bit wrap-around, as the formats define it)"""
    s = np.concatenate([[start], start + np.cumsum(np.asarray(deltas, dtype=np.int64))])
    return s.astype(np.uint16).view(np.int16)


def delta_of(z):
    return (z >> 1) ^ -(z & 1)


def ordinary(n, seed):
    rng = np.random.default_rng(seed)
    return samples_of(rng.integers(-12, 13, size=n - 1))


def shortest(n, seed):
    """a +-1 walk: the table's shortest codes"""
    rng = np.random.default_rng(seed)
    return samples_of(rng.choice([-1, 1], size=n - 1))


def longest(n, lens):
    """the one-byte value with the table's longest code, throughout"""
    z = max(range(256), key=lambda s: (lens[s], s))
    return samples_of(np.full(n - 1, delta_of(z)))


def with_exceptions(sig, at):
    """exceptions (|delta| >= 128) at the given sample indices (>= 1), every other one up, every other one down"""
    a = sig.astype(np.int64)
    for j, i in enumerate(sorted(set(at))):
        a[i:] += 700 if j % 2 == 0 else -700
    return a.astype(np.uint16).view(np.int16)


def edges(n):
    """sample 1, the read's last sample, and the first and last samples of every quarter, of a group of four and of
    two sub-tiles and of a sub-tile around each quarter's start"""
    at = {1, n - 1}
    for q in range(0, n, QUARTER):
        for piece in (QUARTER, 4 * SUB, 2 * SUB, SUB):
            at |= {q, q + piece - 1, q + piece}
    return sorted(i for i in at if 1 <= i < n)


_cases = {}


def cases(oracle):
    """-> [(name, samples)], the same for every method"""
    if not _cases:
        lens = [ln for ln, _ in oracle.table()]
        assert max(lens) > 8 and min(lens) >= 1
        out = []
        for k, n in enumerate(LENGTHS):
            out.append(("ordinary-%d" % n, ordinary(n, 100 + k)))
            out.append(("shortest-%d" % n, shortest(n, 200 + k)))
            out.append(("longest-%d" % n, longest(n, lens)))
        # a lane of 8 longest codes is beyond 64 bits, and a sub-tile of them is the staging buffer's worst case
        assert 8 * max(lens) > 64
        n = 2 * CHUNK + 1
        base = ordinary(n, 7)
        out.append(("edges-all", with_exceptions(base, edges(n))))
        one = base[:CHUNK + 2 * SUB + 3]  # one exception at a time
        for i in (1, SUB - 1, SUB, 4 * SUB - 1, 4 * SUB, QUARTER - 1, QUARTER, CHUNK - 1, CHUNK, one.size - 1):
            out.append(("edge-%d" % i, with_exceptions(one, [i])))
        out.append(("edges-longest", with_exceptions(longest(QUARTER + 4 * SUB + 1, lens), edges(QUARTER + 4 * SUB + 1))))
        out.append(("edges-shortest", with_exceptions(shortest(QUARTER + 4 * SUB + 1, 9), edges(QUARTER + 4 * SUB + 1))))
        _cases["c"] = out
    return _cases["c"]


_streams = {}


def streams(oracle, m):
    """the oracle's stream of every case (computed once per method)"""
    if m not in _streams:
        out = []
        for name, s in cases(oracle):
            ret, st = oracle.press(m, s, cap=L.slot_of(oracle.bound, m, len(s)))
            assert ret == 0, (m, name)
            out.append(st)
        _streams[m] = out
    return _streams[m]


class Batch:
    """reads on the device, every read followed by an empty read whose slot holds canary bytes"""

    def __init__(self, reads, caps):
        import torch
        self.reads, self.caps = reads, caps
        ns, slots = [], []
        for r, c in zip(reads, caps):
            ns += [len(r), 0]
            slots += [c, CANARY]
        self.off, total = press._layout(ns)
        sig = np.zeros(total + 64, dtype=np.int16)
        for r, o in zip(reads, self.off[::2]):
            sig[int(o):int(o) + len(r)] = r
        self.out_off = np.concatenate([[0], np.cumsum(slots)]).astype(np.int64)
        dev = torch.device("cuda:0")
        self.d_sig = torch.from_numpy(sig).to(dev)
        self.d_off = torch.from_numpy(self.off.astype(np.int64)).to(dev)
        self.d_n = torch.from_numpy(np.asarray(ns, dtype=np.int32)).to(dev)
        self.d_out_off = torch.from_numpy(self.out_off).to(dev)
        self.d_out = torch.full((int(self.out_off[-1]) + CANARY,), FILL, dtype=torch.uint8, device=dev)
        self.d_len = torch.full((len(ns),), 7, dtype=torch.int64, device=dev)

    def press(self, m):
        press.press_batch(m, self.d_sig, self.d_off, self.d_n, self.d_out, self.d_out_off, self.d_len)

    def check(self, m, want, names):
        """want[r]: the stream read r must give, None: it must fail.  -> the device's streams"""
        import torch
        torch.cuda.synchronize()
        out = self.d_out.cpu().numpy()
        ln = self.d_len.cpu().numpy().astype(np.uint64)
        got = []
        for r, (w, name) in enumerate(zip(want, names)):
            o, end = int(self.out_off[2 * r]), int(self.out_off[2 * r + 1])
            assert int(ln[2 * r + 1]) == press.FAILED, (m, name)  # (the empty read)
            assert (out[end:end + CANARY] == FILL).all(), (m, name, "bytes behind the slot were written")
            if w is None:
                assert int(ln[2 * r]) == press.FAILED, (m, name, int(ln[2 * r]))
                got.append(None)
                continue
            assert int(ln[2 * r]) == len(w), (m, name, int(ln[2 * r]), len(w))
            g = out[o:o + len(w)].tobytes()
            assert g == w, (m, name, [i for i in range(len(w)) if g[i] != w[i]][:4])
            got.append(g)
        assert (out[int(self.out_off[-1]):] == FILL).all()
        return got


def round_trip(m, reads, got):
    keep = [(s, g) for s, g in zip(reads, got) if g is not None and not L.header_only_huffman(m, s)]
    backs = press.depress_batch_host(m, [g for _, g in keep], [s.size for s, _ in keep])
    for (s, _), bk in zip(keep, backs):
        assert bk is not None and bk.size == s.size and np.array_equal(bk, s), (m, s.size)


@pytest.mark.parametrize("m", METHODS)
def test_lengths_contents_and_edges(oracle, m):
    """every case in one batch, each slot exactly as long as its stream"""
    cs, want = cases(oracle), streams(oracle, m)
    reads, names = [s for _, s in cs], [k for k, _ in cs]
    b = Batch(reads, [len(w) for w in want])
    b.press(m)
    got = b.check(m, want, names)
    round_trip(m, reads, got)


@pytest.mark.parametrize("m", METHODS)
def test_a_slot_that_is_too_small(oracle, m):
    """slots one byte, a dword, half a stream and all but a few bytes short, between reads whose slots fit: the short
    ones fail, nothing is written behind any slot, and the neighbours are the oracle's streams"""
    cs, full = cases(oracle), streams(oracle, m)
    pick = [i for i, (k, _) in enumerate(cs) if k.split("-")[1] in ("513", "2049", "8193", "32769", "65537", "all")]
    assert len(pick) >= 16
    reads, names, caps, want = [], [], [], []
    for j, i in enumerate(pick):
        name, s = cs[i]
        short = (1, 4, len(full[i]) // 2, len(full[i]) - 9)[j % 4] if j % 3 != 2 else 0
        cap = len(full[i]) - short
        reads.append(s)
        names.append("%s-short-%d" % (name, short))
        caps.append(cap)
        w = L.expect_press(oracle, m, s, cap)
        assert (w is None) == (short != 0), (m, name, short)
        want.append(w)
    b = Batch(reads, caps)
    b.press(m)
    got = b.check(m, want, names)
    round_trip(m, reads, got)


@pytest.mark.parametrize("m", METHODS[:2])
def test_two_press_calls_back_to_back(oracle, m):
    """two batches of different reads and sizes pressed on one stream with nothing between the calls (they share
    the library's scratch), in both orders"""
    cs, full = cases(oracle), streams(oracle, m)
    names = [k for k, _ in cs]
    big = [i for i, k in enumerate(names) if k.startswith(("longest", "edges"))]
    small = [i for i, k in enumerate(names) if k.startswith("shortest")][::2]
    for order in ((big, small), (small, big), (small, small[::-1])):
        bs = [Batch([cs[i][1] for i in idx], [len(full[i]) for i in idx]) for idx in order]
        for b in bs:
            b.press(m)
        for b, idx in zip(bs, order):
            got = b.check(m, [full[i] for i in idx], [names[i] for i in idx])
            if order[0] is big:
                round_trip(m, b.reads, got)
