"""CPU tier of the Linear and Sum prover loops: what they add to ring_zk_amd/csrc/rzk_prove_loop.h,
compiled with g++ under -fsanitize=address,undefined into tests/prove_loop/fields_driver.cpp and run as a process.

  * the field-list gather, accept-scatter and zero kernels, emulated through the kernels' own offset function, equal plain
    byte copies for 1 .. 6 fields, entry sizes of V in {1, 2, 3} times k in {3, 5} rows at N in {4, 64, 1024}, the index
    sets first / last / all / ascending subsets and accept all / none / alternating; every destination is compared whole,
    guard bytes included (inside the driver);
  * the live rule for every (ok_commit, wanted, ok_hash) against the Python provers' expressions;
  * the nonce span 2 + 4 max_rounds across every byte carry and its refusal at the 128-bit edge, against Python integers;
  * the quad-count guard at the edges of its two ranges, against Python integers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS, NS, VS, KS, SETS, ACCEPTS = 6, 3, 3, 2, 5, 3


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the field-list driver")
    exe = str(tmp_path_factory.mktemp("prove_loop_fields") / "fields_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "prove_loop", "fields_driver.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, "20261021"], capture_output=True, text=True, env=env)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    return [ln.split() for ln in res.stdout.splitlines()]


def test_field_moves_equal_plain_copies(lines):
    (row,) = [ln for ln in lines if ln[0] == "fields"]
    cases, failures = int(row[1]), int(row[2])
    assert cases == FIELDS * NS * VS * KS * SETS * ACCEPTS
    assert failures == 0


def test_live_rule(lines):
    rows = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "live"]
    assert len(rows) == 4 * 2 * 2 + 1
    seen = set()
    for okc, wanted, okh, live in rows:
        if wanted == 3:       # fiat_shamir.linear_prove_zk: _flag(ok == 3) & okf
            want = int(okc == 3 and okh != 0)
        else:                 # open_prove_zk / sum_prove_zk: (ok & okf) != 0 with one-bit flags; bit 0 is the verdict
            want = int(okc & 1 and okh != 0)
        assert live == want, (okc, wanted, okh)
        seen.add((okc, wanted, okh & 1))
    assert seen == {(c, w, h) for c in range(4) for w in (1, 3) for h in (0, 1)}


def test_nonce_span_across_every_carry_and_at_the_edge(lines):
    (row,) = [ln for ln in lines if ln[0] == "span"]
    assert [int(v) for v in row[1:]] == [2 + 4 * 1, 2 + 4 * 64, 2 + 4 * 255]
    rows = [ln for ln in lines if ln[0] == "edge"]
    assert len(rows) == 16 * 2 + 9
    carried, at_edge = set(), {}
    for _, n0_hex, mr, out_hex, ok in rows:
        n0, out, mr = int.from_bytes(bytes.fromhex(n0_hex), "little"), int.from_bytes(bytes.fromhex(out_hex), "little"), int(mr)
        span = 2 + 4 * mr
        assert out == (n0 + span) % (1 << 128), (n0_hex, mr)
        assert int(ok) == (1 if n0 + span < (1 << 128) else 0), (n0_hex, mr)     # refused: nonce0 + span leaves 128 bits
        for byte in range(16):
            if (n0 % (1 << (8 * byte + 8))) + (span % (1 << (8 * byte + 8))) >= 1 << (8 * byte + 8):
                carried.add(byte)
        if n0 + span in ((1 << 128) - 1, 1 << 128, (1 << 128) + 1):
            at_edge[(mr, n0 + span - (1 << 128))] = int(ok)
    assert carried == set(range(16))
    assert at_edge == {(mr, d): int(d < 0) for mr in (1, 64, 255) for d in (-1, 0, 1)}


def test_quad_count_guard(lines):
    rows = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "quads"]
    assert len(rows) == 12
    verdicts = []
    for n_rows, N, coef, B, ok, quads in rows:
        nbytes = n_rows * N * coef
        q = nbytes // 16
        want = nbytes % 16 == 0 and 0 < q <= 0xFFFFFFFF and B * q * 16 <= (1 << 63) - 1
        assert ok == int(want), (n_rows, N, coef, B)
        if want:
            assert quads == q
        verdicts.append(ok)
    assert verdicts == [1, 1, 1, 0, 0, 1, 0, 0, 1, 0, 1, 0]      # each guard is met from both sides
    assert [15 * 1024 * 8 // 16] == [r[5] for r in rows[:1]]     # zs at V = 3, k = 5, N = 1024: V k N 8 / 16
