"""CPU tier of the 32-bit slab format: ring_zk_amd/csrc/rzk_slab32.h (the scalar narrow / widen / canonical rules and the
routing predicate of the 32-bit entry points) and ring_zk_amd/csrc/rzk_coef.h (the coefficient type that carries a slab's
width through the host layer), compiled with g++ under -fsanitize=address,undefined into tests/slab32/slab32_driver.cpp
and run as a process, against Python integers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
Q_DEFAULT = 3515337053
Q_MAX = 4294606851      # the largest modulus rzk_ctx_create takes (odd, below 4 x the smallest auxiliary prime)
Q_MIN = 3               # ... and the smallest
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

(PG_OPEN_COMMIT, PG_RESPONSE, PG_A1_RELATION) = (3, 4, 5)
RECOVER_VAR = 0x40000
PATH_SHIFT, PATH_UNITS = 1, 6
# the four programs of the 32-bit entry points as they ask for them: commit (fused norm predicate), response, verify, recover
PROGRAMS = [(PG_OPEN_COMMIT, 1), (PG_RESPONSE, 1), (PG_A1_RELATION, 1), (PG_A1_RELATION, RECOVER_VAR | 1)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the slab32 driver")
    exe = str(tmp_path_factory.mktemp("slab32") / "slab32_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "slab32", "slab32_driver.cpp")])
    return exe


def run_driver(exe, tmp_path, mode, lines):
    path = tmp_path / ("slab32_%s.txt" % mode)
    path.write_text("".join(line + "\n" for line in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    out = [line.split() for line in res.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def low_word(c):
    """The int32 a two's-complement machine keeps of the integer c."""
    w = c & 0xFFFFFFFF
    return w - 2 ** 32 if w >= 2 ** 31 else w


def check_rules(exe, tmp_path, q, values):
    half = (q - 1) // 2
    got = run_driver(exe, tmp_path, "rules", ["%d %d" % (q, c) for c in values])
    for c, g in zip(values, got):
        canon = -half <= c <= half
        assert int(g[0]) == canon, (q, c)
        assert int(g[1]) == low_word(c), (q, c)
        assert int(g[2]) == (not canon), (q, c)          # narrow reports exactly the non-canonical coefficients
        if canon:
            assert int(g[1]) == c                        # ... and is exact on the canonical ones
        if I32_MIN <= c <= I32_MAX:
            assert int(g[3]) == canon, (q, c)            # the 32-bit test agrees with the 64-bit one on every int32
            assert int(g[4]) == c, (q, c)                # widen is sign extension
            assert int(g[5]) == (c + half) % 2 ** 32     # the word the kernels max before their one compare
            assert (int(g[5]) <= 2 * half) == canon
        else:
            assert g[3:] == ["-", "-", "-"] and not canon


@pytest.mark.parametrize("q", [Q_DEFAULT, Q_MAX, Q_MIN])
def test_rules_at_the_edges(driver, tmp_path, q):
    half = (q - 1) // 2
    assert half < 2 ** 31
    values = [0, 1, -1, half, -half, half + 1, -half - 1, I32_MIN, I32_MAX,
              # beyond int32: what narrow must report, and what the old high-word half of the test was for
              2 ** 31, -2 ** 31 - 1, 2 ** 32, 2 ** 32 + 5, -2 ** 32, 7 * 2 ** 32 - 3, 2 ** 63 - 1, -2 ** 63]
    check_rules(driver, tmp_path, q, values)


@pytest.mark.parametrize("q", [Q_DEFAULT, Q_MAX, Q_MIN])
def test_aliases_of_a_canonical_residue(driver, tmp_path, q):
    """c - q and c + q are the same residue as c, and for some canonical c they are int32 values: the coefficients a
    32-bit slab can hold that a kernel must not read as c.

    c - q >= -2^31 needs c >= q - 2^31, so the canonical c with c - q in int32 are [max(-HALF, q - 2^31), HALF]; by
    symmetry those with c + q in int32 are [-HALF, min(HALF, 2^31 - 1 - q)].  The endpoints of both intervals are tested.
    For the default and the largest modulus 3 q / 2 > 2^31, so c +- 2 q lies outside int32 for every canonical c: c - q and
    c + q are then the ONLY non-canonical int32 values of c's residue, and the interval ends are q - 2^31 and
    2^31 - 1 - q themselves.  (The smallest modulus has many more aliases; every one of them fails |c| <= HALF all the
    same, which is all the test needs.)"""
    half = (q - 1) // 2
    lo = max(-half, q - 2 ** 31)
    hi = min(half, 2 ** 31 - 1 - q)
    if q in (Q_DEFAULT, Q_MAX):
        assert 3 * q > 2 ** 32 and lo == q - 2 ** 31 and hi == 2 ** 31 - 1 - q
        assert half - 2 * q < I32_MIN and -half + 2 * q > I32_MAX
    values = [lo - q, half - q, -half + q, hi + q]
    for v in values:
        assert I32_MIN <= v <= I32_MAX and not -half <= v <= half
        assert -half <= (v + q if v < 0 else v - q) <= half
    assert lo - q == I32_MIN or q == Q_MIN
    assert hi + q == I32_MAX or q == Q_MIN
    check_rules(driver, tmp_path, q, values + [lo, hi, half, -half])


def test_rules_on_a_sweep(driver, tmp_path):
    """Every int32 within a few steps of the edges and a stride over the whole range, default modulus."""
    half = (Q_DEFAULT - 1) // 2
    near = [e + s for e in (0, half, -half, I32_MIN + 8, I32_MAX - 8) for s in range(-8, 9)]
    check_rules(driver, tmp_path, Q_DEFAULT, near + list(range(I32_MIN, I32_MAX, 104729 * 41)))


# the key's classification (KeyClass digits, row-major): a1 = [I | a1'], a2 = [0 | I | a2'], the reference's shape
def ref_key(n, k, l):
    rows = []
    for i in range(n):
        rows.append("".join("1" if j == i else ("0" if j < n else "2") for j in range(k)))
    for i in range(l):
        rows.append("".join("0" if j < n else ("1" if j == n + i else ("0" if j < n + l else "2")) for j in range(k)))
    return "".join(rows)


def route(exe, tmp_path, N, nkl, rot=1, shift_bytes=1, pair_poly=1):
    n, k, l = nkl
    logn = N.bit_length() - 1
    lines = ["%d %d %d %d %d %d %d %d %d %d %s" % (n, k, l, logn, int(N < 512), rot, shift_bytes, pair_poly, pid, var,
                                                   "-" if pid == PG_RESPONSE else ref_key(n, k, l)) for pid, var in PROGRAMS]
    return [(int(st), p, int(nat)) for st, p, nat in run_driver(exe, tmp_path, "route", lines)]


@pytest.mark.parametrize("N", [512, 1024])
def test_routing_native(driver, tmp_path, N):
    got = route(driver, tmp_path, N, (1, 3, 1))
    assert [g[0] for g in got] == [0] * 4
    assert [g[2] for g in got] == [1] * 4, "all four programs run native 32-bit kernels at (1,3,1)"
    assert [int(g[1]) for g in got] == [PATH_UNITS, PATH_SHIFT, PATH_UNITS, PATH_UNITS]


@pytest.mark.parametrize("N,nkl,knobs", [
    (64, (1, 3, 1), {}),                    # small rings: schoolbook kernels
    (2048, (1, 3, 1), {}),                  # two-wavefront teams
    (2048, (1, 3, 1), {"pair_poly": 0}),    # ... and the one-wavefront N = 2048 kernels: no native form either
    (512, (2, 5, 2), {}),                   # n >= 2: groups, the split relation
    (1024, (2, 5, 2), {}),
    (512, (1, 3, 1), {"rot": 0}),           # RZK_SHIFT=0: challenge products as transforms
    (1024, (1, 3, 1), {"rot": 0}),
    (1024, (1, 3, 1), {"shift_bytes": 0}),  # RZK_SHIFT_BYTES=0: the word-only rotation kernel
])
def test_routing_convert(driver, tmp_path, N, nkl, knobs):
    got = route(driver, tmp_path, N, nkl, **knobs)
    assert [g[2] for g in got] == [0] * 4, "every program of such a context takes the convert path"


@pytest.mark.parametrize("N", [4, 512])
def test_typed_byte_count(driver, tmp_path, N):
    """poly_bytes<C>(N, count) = count * N * sizeof(C): the one byte count of the host layer, for both slab types (the
    driver's static_asserts hold that an Op<int32_t> takes no 64-bit slab and an Op<int64_t> no 32-bit one)."""
    counts = [0, 1, 3, 9, 4096 * 9, 2 ** 33 + 5]     # the last: a count whose bytes need more than 32 bits at either width
    got = run_driver(driver, tmp_path, "coef", ["%d %d" % (N, k) for k in counts])
    for k, g in zip(counts, got):
        assert [int(v) for v in g] == [k * N * 8, k * N * 4, 1, 1], (N, k)
