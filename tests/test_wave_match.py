"""CPU: the wave kernel's hash match (csrc/beam_wave.h: wave_match -- one table round, the losers settled among themselves
in registers, a second round on a cleared table when there are many) and the passes that skip their group work when nobody
joined anybody.
  * the match on its own: a stand-alone program (tests/sim/wave_match_harness.cpp) calls it on the 64-fiber context of
    tests/sim/wave_fibers.h with crafted key sets and compares with brute force; built with AddressSanitizer and UBSan and
    run as a program;
  * whole decodes on the simulator, wave kernel forced, of inputs that merge in most frames, beam for beam against the oracle
    (strict order, scores within 1e-9)."""
import os
import shutil
import subprocess

import pytest

from tests import wave_match_util as U
from tests.sim_util import sim_library  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the simulator and this harness"
    out = str(tmp_path_factory.mktemp("wave_match") / "wave_match_harness")
    src = os.path.join(ROOT, "tests", "sim", "wave_match_harness.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-DCTC_SIM", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function",
                           "-o", out, src])
    return out


def test_match_against_brute_force(harness):
    """Cases (each for one and for two candidates per lane): 1 all keys distinct in one round-one slot (63 losers: the
    cleared-table round); 2 duplicates that lose round one; 3 duplicates that win it; 4 a pair split across the two halves;
    5 exactly as many losers as the loop threshold and one more, and exactly 8 and 9 (the threshold's first value); 6 partly invalid lanes; 7 1 000 seeded random sets
    with 0 - 30 % duplicates."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "all cases ok"
    for a in (1, 2):
        for name in ("1 one-slot", "2 duplicates lose", "2 more duplicates lose", "3 duplicates win", "5 threshold losers", "5 threshold + 1 losers",
                     "5 eight losers", "5 nine losers", "6 invalid lanes", "6 no valid lane"):
            assert any(ln.startswith("%s A=%d: ok" % (name, a)) for ln in lines), (name, a)
        assert "7 random A=%d: 1000 sets done" % a in lines
    assert any(ln.startswith("4 split pair A=2: ok") for ln in lines)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_merging_decodes_on_the_simulator(name, sim_library, monkeypatch):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    monkeypatch.setenv("CTCDEC_BEAM_KERNEL", "wave")
    labels, _, kw = U.CASES[name]
    dec = build_ctcdecoder(labels)
    for u, (x, want) in enumerate(zip(U.inputs(name), U.expected(name))):
        got = U.beams_of(dec.decode_beams(x, **kw))
        assert dec.last_beam_kernel == 1  # (the wave kernel took it)
        U.assert_same_beams(got, want, "%s[%d]" % (name, u))
    if name == "wide100":
        assert max(len(w) for w in U.expected(name)) > 64  # (more than 64 live beams: pass_big)
