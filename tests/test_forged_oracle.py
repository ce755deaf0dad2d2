"""The forged corpus of tests/_forge.py against the oracle (CPU only).

* every case gets exactly the verdict its builder intends - so the corpus cannot decay into streams that all die on
  the first length check, and the oracle implements the definition of DESIGN.md 6.0.20;
* every kind exists for every method it applies to;
* where a case is the minimal encoding of a read, its bytes are the oracle's own stream of that read (the builders
  and the encoder agree on the format);
* oracle/forged_check - the same decoders as a program of its own, linked with AddressSanitizer + UBSan, every
  stream in a block of exactly its size - exits clean with the verdicts of the ctypes oracle.
"""
import os
import subprocess

import numpy as np
import pytest

import _forge as F
import _libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("m", F.METHODS)
def test_kinds_are_all_there(oracle, m):
    cases = F.cases_for(m, oracle)
    assert sorted({c.kind for c in cases}) == F.expected_kinds(m)
    names = [c.name for c in cases]
    assert len(names) == len(set(names)) and len(names) <= 300
    hdr = 12 if F.LAYOUT[m][0] == "exzd" else 2
    assert [c.name for c in cases if c.kind == "len"] == ["len-%d" % k for k in range(hdr + 4)]
    assert {int(c.name.split("-")[1]) for c in cases if c.kind == "carry"} == {0, 63, 64, 65, 129}
    rooms = {c.room for c in cases}
    assert rooms >= {65, 100, 2049, F.BIG} and (F.LAYOUT[m][1] == "rc" or 9 in rooms)
    assert sum(c.verdict == F.ACCEPTED for c in cases) >= 10 and sum(c.verdict == F.REFUSED for c in cases) >= 20


def test_methods_are_the_exception_family():
    import _layouts as L
    assert sorted(F.METHODS) == sorted(m for m in L.EX_FAMILY if m != "zstd_hasgam_vbsse21_zdq")
    assert len(F.METHODS) == 12 and {f for f, _ in F.LAYOUT.values()} == set(F.FORMATS)


@pytest.mark.parametrize("m", F.METHODS)
def test_oracle_gives_the_intended_verdict(oracle, m):
    for c in F.cases_for(m, oracle):
        ret, back = oracle.depress(m, c.stream, c.room)
        if c.verdict == F.REFUSED:
            assert ret != 0, (m, c.name, back.size)
        else:
            assert ret == 0, (m, c.name)
            assert back.size == c.samples.size and np.array_equal(back, c.samples), (m, c.name, back.size, c.samples.size)
        if c.canonical is not None:
            r2, st = oracle.press(m, c.canonical, cap=8 * c.canonical.size + 4096)
            assert r2 == 0 and st == c.stream, (m, c.name)


def test_batches_of_the_gpu_tests_assemble(oracle):
    """what tests/test_forged_sections.py sends to the device: every forged read between two good ones (the good reads
    are ones the oracle gives back, the range coders' not stored raw - asserted where they are made)"""
    for m in F.METHODS:
        good, items = F.interleaved(oracle, m)
        assert len(items) == 2 * len(F.cases_for(m, oracle)) + 1 <= 700 and all(it in good for it in items[::2])


def test_width0_read_round_trips(oracle):
    """s[i] = 128 i, 101 samples: 16 bytes under vbbe21_zd, which the oracle used to refuse (both blocks have width 0,
    so 100 exceptions cost no byte)"""
    s = (128 * np.arange(101)).astype(np.int16)
    for m in ("vbbe21_zd", "rccm_vbbe21_zd"):
        ret, st = oracle.press(m, s)
        assert ret == 0
        if m == "vbbe21_zd":
            assert st.hex() == "0000" "64000000" "01000000" "00" "01000000" "00"
        ret, back = oracle.depress(m, st, 101)
        assert ret == 0 and np.array_equal(back, s), m


def test_sanitizer_build_agrees(oracle, tmp_path):
    exe = os.path.join(ROOT, "oracle", "forged_check")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "forged"], check=True)
    cases = [c for m in F.METHODS for c in F.cases_for(m, oracle)]
    path = str(tmp_path / "forged.bin")
    F.write_corpus(path, cases)
    r = subprocess.run([exe, path, _libs.TABLE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for k, (c, line) in enumerate(zip(cases, lines)):
        ret, back = oracle.depress(c.method, c.stream, c.room)
        want = "%d %d %d %d" % (k, ret, back.size if ret == 0 else 0, F.fnv1a32_samples(back) if ret == 0 else 0)
        assert line == want, (c.method, c.name)
