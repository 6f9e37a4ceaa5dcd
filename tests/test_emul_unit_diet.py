"""CPU statement of the unit kernels' shorter lane-level forms (ring_zk_amd/csrc/rzk_core.h): crt2_zq_short and dot2_lazy.

tests/emul/unit_diet_driver.cpp is a stand-alone program over the header the kernels compile:
  * crt2_zq_short against crt_center, the two-reduction crt2_zq and a 128-bit computation, on the digit edges
    d1 in {0, 1, h1-1, h1, h1+1, p1-1} x d0 in {0, h0-1, h0, h0+1, p0-1} with (h1, h0) = divmod((P+1)/2, p0), both lazy
    representatives of the prime-1 residue, and 10^6 seeded random pairs (for the protocols' modulus; the edges and 10^5
    pairs for the smallest and the largest modulus the constants accept);
  * dot2_lazy against the mont_lazy / mac_add / mac_sub steps it replaces: x in {0, 1, 4p-1, 2^32-1, random},
    k in {0, 1, p-1, random}, both signs of both terms, all three primes: equal mod p and inside [0, 2p).
It is built twice, optimised and under -fsanitize=address,undefined as that stand-alone program.  Host logic testing: no
GPU, and the product never loads this program.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "unit_diet_driver.cpp")
BUILDS = {
    "O2": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def report(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unit_diet_" + request.param) / "unit_diet_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + BUILDS[request.param] + ["-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout.splitlines(), p.stderr


def test_every_case_matches(report):
    code, lines, err = report
    assert code == 0 and lines and lines[-1] == "all cases passed", "\n".join(l for l in lines if not l.startswith("ok")) + err
    assert not [l for l in lines if l.startswith("FAIL")]
    assert "runtime error" not in err and "AddressSanitizer" not in err


def test_the_cases_the_forms_are_checked_on(report):
    _, lines, _ = report
    crt = [l for l in lines if l.startswith("ok   crt2 q=3515337053")]
    assert any("digit edges" in l and ": 30 cases" in l for l in crt)
    assert any("seeded random pairs" in l and ": 1000000 cases" in l for l in crt)
    assert sum("digit edges" in l for l in lines) == 3          # three moduli
    dot = [l for l in lines if l.startswith("ok   dot2 p")]
    assert len(dot) == 3                                          # three primes
    for l in dot:
        assert int(l.rsplit(":", 1)[1].split()[0]) >= 4 * 4 * 3 * 3 * 4
