"""CPU statement of the full vector-twiddle image of the N = 1024 unit kernels (TwAllImg, ring_zk_amd/csrc/rzk_core.h; RZK_TW_LDS=2).

tests/emul/tw3_lds_driver.cpp is a stand-alone program over the header the kernels compile:
  * it builds the image of every prime and direction as the kernels' fill loop does with 1024 threads, each in an
    allocation of its own;
  * every index phase 3 forms lies in [256, 1024), the image word it reads holds exactly that table entry, the image holds
    every entry of [256, 1024) once, and its first 256 words are the phase-2 image;
  * no two of sixteen consecutive lanes share a bank in any 16-byte read of either phase;
  * all 64 lanes of the forward and inverse transforms at LOGN = 10, phases 2 and 3 reading the image, equal the run on the
    global table word for word: three primes, seeded random polynomials over the lazy ranges and the all-maximum one.
It is built twice, optimised and under -fsanitize=address,undefined as that stand-alone program.  Host logic testing: no
GPU, and the product never loads this program.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "tw3_lds_driver.cpp")
BUILDS = {
    "O2": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def report(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tw3_lds_" + request.param) / "tw3_lds_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + BUILDS[request.param] + ["-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout.splitlines(), p.stderr


def count(line):
    return int(line.rsplit(":", 1)[1].split()[0])


def test_every_case_matches(report):
    code, lines, err = report
    assert code == 0 and lines and lines[-1] == "all cases passed", "\n".join(lines) + err
    assert not [l for l in lines if l.startswith("FAIL")]
    assert "runtime error" not in err and "AddressSanitizer" not in err


def test_the_cases_the_image_is_checked_on(report):
    _, lines, _ = report
    held = [l for l in lines if l.startswith("ok   image holds the phase-2 image, then entries 256..1023 once each")]
    assert len(held) == 1 and count(held[0]) == 1024
    idx = [l for l in lines if l.startswith("ok   phase-3 indices inside [256, 1024)")]
    assert len(idx) == 1 and count(idx[0]) == 64 * 6 * 12   # lanes x tables x twiddles per lane
    banks = [l for l in lines if l.startswith("ok   sixteen consecutive lanes cover the 64 banks once")]
    assert len(banks) == 1 and count(banks[0]) == 6 * 7 * 4   # tables x 16-byte reads per lane x groups of sixteen lanes
    for pi in range(3):
        for what in ("forward, image against global table", "inverse, image against global table",
                     "inverse(forward(x)) == x through the image"):
            hit = [l for l in lines if l.startswith("ok   prime %d %s" % (pi, what))]
            assert len(hit) == 1 and count(hit[0]) == 5 * 1024
