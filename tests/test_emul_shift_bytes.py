"""CPU statement of shift_row_kernel's packed-byte rotations (ByteGeo, ring_zk_amd/csrc/rzk_core.h).

tests/emul/shift_bytes_driver.cpp is a stand-alone program: it replays the 64 lanes' byte-image build, window fetch,
realign and add through the header the kernel compiles, and compares with the schoolbook negacyclic product — ternary
operands under challenges, the edge of the condition for |v|_inf = 1, 2, 3 with every byte sum at its extreme, every
byte alignment and wrap position, zero operands, and the inputs that must fall back to the word path.  Host logic
testing: no GPU, and the product never loads this program.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "shift_bytes_driver.cpp")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shift_bytes") / "shift_bytes_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout.splitlines()


def test_every_case_matches_the_schoolbook_product(report):
    code, lines = report
    assert code == 0 and lines[-1] == "all cases passed", "\n".join(l for l in lines if not l.startswith("ok"))
    assert not [l for l in lines if l.startswith("FAIL")]


def test_the_cases_cover_both_sizes_and_both_paths(report):
    _, lines = report
    for n in (512, 1024):
        mine = [l for l in lines if f"N={n} " in l]
        assert sum(" bytes " in l for l in mine) >= 60 and sum(" words " in l for l in mine) >= 9, (n, len(mine))
        # the edge: floor(255 / (2 |v|)) non-zeros fit, one more does not
        for m, fit in ((1, 127), (2, 63), (3, 42)):
            assert any(f"bytes edge |v|={m} sign +1: {fit} non-zeros" in l for l in mine)
            assert any(f"words edge |v|={m} sign -1: {fit + 1} non-zeros" in l for l in mine)

