"""CPU tier of the in-library prover loop: ring_zk_amd/csrc/rzk_prove_loop.h compiled with g++ under
-fsanitize=address,undefined into tests/prove_loop/prove_loop_driver.cpp and run as a process.

  * the compaction kernel, lane by lane (compact_emulate), equals a plain loop for B in {1, 63, 64, 65, 1023, 1024, 1025,
    4097}, for the patterns all clear / all set / alternating / first only / last only / random, with live masks that
    exclude set entries, and leaves idx past count untouched (checked inside the driver, between guard words);
  * nonce i = nonce0 + i as a 128-bit little-endian integer across every byte carry, and the wrap rule, against Python
    integers;
  * the coin formula at the extremes of the two draws against Python integers (fiat_shamir.draw_coins)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES, PATTERNS, MASKS = 8, 9, 3


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the prove-loop driver")
    exe = str(tmp_path_factory.mktemp("prove_loop") / "prove_loop_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "prove_loop", "prove_loop_driver.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, "20261020"], capture_output=True, text=True, env=env)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    return [ln.split() for ln in res.stdout.splitlines()]


def test_compaction_equals_the_plain_loop(lines):
    (row,) = [ln for ln in lines if ln[0] == "compact"]
    cases, failures = int(row[1]), int(row[2])
    assert cases == SIZES * PATTERNS * MASKS + 1
    assert failures == 0


def test_nonce_addition_across_every_byte_carry(lines):
    rows = [ln for ln in lines if ln[0] == "nonce"]
    assert len(rows) == 16 * 2 + 6
    carried, wrapped = set(), 0
    for _, n0_hex, inc, out_hex, ok in rows:
        n0, out = int.from_bytes(bytes.fromhex(n0_hex), "little"), int.from_bytes(bytes.fromhex(out_hex), "little")
        total = n0 + int(inc)
        assert out == total % (1 << 128), (n0_hex, inc)
        assert int(ok) == (1 if total < (1 << 128) else 0), (n0_hex, inc)
        wrapped += total >= (1 << 128)
        for byte in range(16):                                  # a carry out of `byte` into the next one (or out of the top)
            if (n0 % (1 << (8 * byte + 8))) + (int(inc) % (1 << (8 * byte + 8))) >= 1 << (8 * byte + 8):
                carried.add(byte)
    assert carried == set(range(16))
    assert wrapped >= 3                                         # 2^128 - 1 + 1, and 2^128 - 768 + 768 / + 769


def test_nonce_span_and_the_wrap_rule(lines):
    (row,) = [ln for ln in lines if ln[0] == "span"]
    assert [int(v) for v in row[1:]] == [4, 766]                 # r, then y and two coin draws per round
    top = (1 << 128) - 768
    by_inc = {int(ln[2]): int(ln[4]) for ln in lines if ln[0] == "nonce" and int.from_bytes(bytes.fromhex(ln[1]), "little") == top}
    assert by_inc == {766: 1, 767: 1, 768: 0, 769: 0}            # the sum must stay below 2^128


def test_coin_formula_at_the_extremes(lines):
    from ring_zk_amd import fiat_shamir as FS

    (consts,) = [ln for ln in lines if ln[0] == "consts"]
    R0, half, R = (int(v) for v in consts[1:])
    assert R0 == FS.COIN_R0 == (1 << 31) - 1 and half == (R0 - 1) // 2 == (1 << 30) - 1 and R == R0 * R0 <= 1 << 62
    rows = [ln for ln in lines if ln[0] == "coin"]
    assert len(rows) == 49
    seen = set()
    for _, a, b, coin in rows:
        a, b, coin = int(a), int(b), int(coin)
        assert coin == (a + half) * R0 + (b + half), (a, b)
        assert 0 <= coin < R
        seen.add((a, b))
    assert {(-half, -half), (half, half), (-half, half), (half, -half)} <= seen
    assert (half + half) * R0 + (half + half) == R - 1           # the largest coin is R - 1: uniform over [0, R)
