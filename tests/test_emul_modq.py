"""CPU statement of the kernels' modulus-dependent lane helpers at the edges of the supported modulus range.

include/rzk.h: q odd, 1073692673 = p0 < q <= 4 p2 - 1 = 4294606851.  q reaches every kernel as a run-time value (about twenty
derived constants, DevTables::crt).  tests/emul/modq_driver.cpp is a stand-alone program over the header the kernels
compile (ring_zk_amd/csrc/rzk_core.h) and checks, for every modulus of MODULI, against 128-bit arithmetic:
  * addq / subq on residue pairs (edges around 0, (q-1)/2, q-1, 2^30, 2^31; random), montq_u / montq on any 32-bit word
    times a residue, center_rounds<3> on |s| < 3q, zq_from_centered / center_from_zq on the centred range;
  * zq_from_i64: every a in [-2^20, 2^20]; every low word past the last multiple of q below 2^32 (from 4q - 8 on where
    4q < 2^32) and next to every multiple of q, under high words 0, +-1, -2 and +-(4.0e18 >> 32); |a| just below 4.0e18
    (where shift_product splits into two 16-bit passes); 10^6 random |a| < 4.0e18, and 10^6 random |a| < 2^62 for q > 2^30
    (below 2^30 the helper needs |a| < q 2^32, which the pass split guarantees);
  * crt_center, the offset chain crt_fold0/1/2 + crt_finish, crt1_zq, and crt2_zq against crt2_zq_short, for np = 1, 2, 3:
    X in {0, +-1, +-(P-1)/2, +-((P-1)/2 - 1), +-h} and 10^5 random X per np, every mix of the two lazy representatives;
  * the lift x + 2p for x in {-h, -h+1, -1, 0, 1, h-1, h}, every prime: inside [0, 4p), below 2^32, congruent to x;
  * the canonical test as rzk_slab32.h states it for host code (the kernels' canon_lo_mx / canon_fail take a wavefront
    vote over the same compare and are device code): +-h pass; +-(h+1), h + 2^32, -h - 2^32 fail, also as int32;
  * make_crt_consts refuses p0, p0 - 2, 4 p2 + 1 and even moduli.
It is built twice, optimised and under -fsanitize=address,undefined as that stand-alone program.  Host logic testing: no
GPU, and the product never loads this program.

With zq_from_i64 as it was before this test (three subtractions of q from the low word), exactly the zq_from_i64 groups
"every a in [-2^20, 2^20]", "low-word edges" (and, at Q_MIN, "seeded random") of Q_MIN and Q_B30 fail, and nothing else.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "modq_driver.cpp")

P0, P2 = 1073692673, 1073651713
Q_MIN = P0 + 2               # smallest accepted; 2^32 - 4q = 196596
Q_B30 = 2 ** 30 - 1          # last modulus with 4q < 2^32
Q_A30 = 1073741827           # first above 2^30: 31-bit sampling mask at acceptance ~ 0.50002
Q_A31 = 2 ** 31 + 1          # first modulus where the sum of two residues wraps 32 bits; (q-1)/2 = 2^30
Q_DEF = 3515337053           # the protocols' modulus
Q_MAX = 4 * P2 - 1           # (q-1)/2 = 2 p2 - 1: the lift x + 2 p2 reaches 1 and 4 p2 - 1
MODULI = {"Q_MIN": Q_MIN, "Q_B30": Q_B30, "Q_A30": Q_A30, "Q_A31": Q_A31, "Q_DEF": Q_DEF, "Q_MAX": Q_MAX}

BUILDS = {
    "O2": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def report(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("modq_" + request.param) / "modq_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + BUILDS[request.param] + ["-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout.splitlines(), p.stderr


def test_modulus_set_is_inside_the_documented_range():
    assert Q_MIN == 1073692675 and Q_MAX == 4294606851
    for q in MODULI.values():
        assert q % 2 == 1 and P0 < q <= 4 * P2 - 1
    assert 4 * Q_B30 < 2 ** 32 < 4 * Q_A30 and 2 ** 32 - 4 * Q_MIN == 196596
    assert 4.0e18 < Q_MIN * 2 ** 32          # the rotation sums' high word stays below every supported modulus


def test_every_case_matches(report):
    code, lines, err = report
    assert code == 0 and lines and lines[-1] == "all cases passed", "\n".join(l for l in lines if not l.startswith("ok")) + err
    assert not [l for l in lines if l.startswith("FAIL")]
    assert "runtime error" not in err and "AddressSanitizer" not in err


def _count(line):
    return int(line.rsplit(":", 1)[1].split()[0])


@pytest.mark.parametrize("name", sorted(MODULI))
def test_the_cases_each_modulus_is_checked_on(report, name):
    _, lines, _ = report
    q = MODULI[name]
    mine = [l for l in lines if l.startswith("ok  ") and f" q={q}:" in l]

    def group(prefix):
        hits = [l for l in mine if l[5:].startswith(prefix)]
        assert len(hits) == 1, (prefix, hits)
        return _count(hits[0])

    assert group("constants accepted") == 1
    assert group("addq / subq") >= 2 * 200 * 200
    assert group("montq_u / montq") >= 2 * 200 * 200
    assert group("center_rounds<3>") >= 100000
    assert group("zq_from_centered / center_from_zq") >= 100007
    assert group("zq_from_i64: every a in [-2^20, 2^20]") == 2 ** 21 + 1
    # every low word in [4q - 8, 2^32) where that interval exists, under eight high words
    gap = 2 ** 32 - (2 ** 32 // q) * q + 8
    assert group("zq_from_i64: low-word edges") >= 8 * min(gap, 400000)
    assert group("zq_from_i64: |a| just below 4.0e18") == 2 * 4096
    assert group("zq_from_i64: seeded random |a| < 4.0e18") == 10 ** 6
    if q > 2 ** 30:
        assert group("zq_from_i64: seeded random |a| < 2^62") == 10 ** 6
    for np_ in (1, 2, 3):
        assert group(f"crt np={np_}: crt_center") >= 100000
    assert group("crt np=2: crt2_zq == crt2_zq_short") >= 100000
    assert group("lift") == 3 * 7
    assert group("canonical test") >= 20


def test_the_range_itself_is_pinned(report):
    _, lines, _ = report
    assert any(l.startswith("ok   constants refused outside") and _count(l) == 8 for l in lines)
