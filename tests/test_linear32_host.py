"""CPU tier of the Linear proof on 32-bit slabs: the routing predicate on the real plans of the
programs a Linear call launches (tests/slab32/slab32_driver.cpp, `route`, built as tests/test_slab32_host.py builds it) and
the per-coefficient arithmetic of the 32-bit norm kernel (tests/linear32/norm32_driver.cpp), both g++ programs under
-fsanitize=address,undefined, run as processes."""
import os
import shutil
import subprocess

import pytest

from test_slab32_host import I32_MAX, I32_MIN, Q_DEFAULT, Q_MAX, Q_MIN, ref_key, run_driver

HERE = os.path.dirname(os.path.abspath(__file__))
(PG_CMUL, PG_RESPONSE, PG_LIN_COMMIT2, PG_LIN_U, PG_LIN_V1, PG_LIN_V2, PG_LIN_V1B, PG_LIN_V2B) = (2, 4, 6, 7, 8, 9, 20, 21)
DKEY_VAR, RECOVER_VAR, MASK_VAR = 0x10000, 0x40000, 2
PATH_SHIFT, PATH_ROWS, PATH_UNITS = 1, 5, 6
GXX_FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"]


def build(tmp_path_factory, sub, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the host drivers")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([gxx] + GXX_FLAGS + ["-o", exe, os.path.join(HERE, sub, name + ".cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory, "slab32", "slab32_driver")


@pytest.fixture(scope="module")
def norm_driver(tmp_path_factory):
    return build(tmp_path_factory, "linear32", "norm32_driver")


def linear_programs(l):
    """(program, variant, launch path at n = 1) of every program the six Linear calls launch on a context that prepares no
    multiplier images, fused and plain forms of the checked ones."""
    return [
        (PG_CMUL, l, PATH_ROWS),                          # gx = g . x
        (PG_LIN_COMMIT2, 0, PATH_UNITS), (PG_LIN_COMMIT2, 1, PATH_UNITS), (PG_LIN_COMMIT2, MASK_VAR, PATH_UNITS),
        (PG_LIN_U, 0, PATH_ROWS),
        (PG_RESPONSE, 2, PATH_SHIFT),
        (PG_LIN_V1B, 0, PATH_UNITS), (PG_LIN_V1B, 1, PATH_UNITS),
        (PG_LIN_V1B, RECOVER_VAR, PATH_UNITS), (PG_LIN_V1B, RECOVER_VAR | 1, PATH_UNITS),
        (PG_LIN_V2B, 0, PATH_ROWS), (PG_LIN_V2B, RECOVER_VAR, PATH_ROWS),
    ]


def route(exe, tmp_path, N, nkl, programs, rot=1, shift_bytes=1, pair_poly=1):
    n, k, l = nkl
    logn = N.bit_length() - 1
    lines = ["%d %d %d %d %d %d %d %d %d %d %s" % (n, k, l, logn, int(N < 512), rot, shift_bytes, pair_poly, pid, var,
                                                   "-" if pid in (PG_RESPONSE, PG_CMUL) else ref_key(n, k, l))
             for pid, var in programs]
    return [(int(st), p, int(nat)) for st, p, nat in run_driver(exe, tmp_path, "route", lines)]


@pytest.mark.parametrize("N", [512, 1024])
def test_linear_programs_native(driver, tmp_path, N):
    progs = linear_programs(1)
    got = route(driver, tmp_path, N, (1, 3, 1), [(p, v) for p, v, _ in progs])
    assert [g[0] for g in got] == [0] * len(progs)
    assert [int(g[1]) for g in got] == [path for _, _, path in progs], "the paths the routing rule was written for"
    assert [g[2] for g in got] == [1] * len(progs), "every program of a Linear call at (1,3,1) has native 32-bit kernels"


@pytest.mark.parametrize("N", [512, 1024])
def test_multiplier_images_convert(driver, tmp_path, N):
    """The dkey variants (RZK_DKEY=2, or enough rows per multiplier) read images made from 64-bit slabs."""
    progs = [(PG_CMUL, 1 | DKEY_VAR), (PG_LIN_U, DKEY_VAR), (PG_LIN_V2B, DKEY_VAR), (PG_LIN_V2B, DKEY_VAR | RECOVER_VAR)]
    got = route(driver, tmp_path, N, (1, 3, 1), progs)
    assert [g[0] for g in got] == [0] * len(progs) and [int(g[1]) for g in got] == [PATH_ROWS] * len(progs)
    assert [g[2] for g in got] == [0] * len(progs)


@pytest.mark.parametrize("N", [512, 1024])
def test_rotation_terms_inside_rows_convert(driver, tmp_path, N):
    """RZK_LIN_E=0: the verifier's pair PG_LIN_V1 / PG_LIN_V2 multiplies by g AND carries rotation terms in row_kernel."""
    got = route(driver, tmp_path, N, (1, 3, 1), [(PG_LIN_V1, 0), (PG_LIN_V1, 1), (PG_LIN_V2, 0)])
    assert [g[0] for g in got] == [0] * 3 and [int(g[1]) for g in got] == [PATH_ROWS] * 3
    assert [g[2] for g in got] == [0] * 3


@pytest.mark.parametrize("N,nkl,knobs", [
    (64, (1, 3, 1), {}),
    (2048, (1, 3, 1), {}),
    (512, (2, 5, 2), {}),
    (1024, (2, 5, 2), {}),
    (512, (1, 3, 1), {"rot": 0}),
    (1024, (1, 3, 1), {"rot": 0}),
    (512, (1, 3, 1), {"shift_bytes": 0}),
    (1024, (1, 3, 1), {"shift_bytes": 0}),
])
def test_linear_programs_convert(driver, tmp_path, N, nkl, knobs):
    progs = linear_programs(nkl[2])
    got = route(driver, tmp_path, N, nkl, [(p, v) for p, v, _ in progs], **knobs)
    planned = [g for g in got if g[0] == 0]
    assert len(planned) >= len(progs) - 4, got          # (a fused form may be uncoverable on a shape: it is not planned)
    assert [g[2] for g in planned] == [0] * len(planned), "every program of such a context takes the convert path"


@pytest.mark.parametrize("q", [Q_DEFAULT, Q_MAX, Q_MIN])
def test_norm_term_at_the_edges(norm_driver, tmp_path, q):
    """What norm_rows<., int32_t> does with one coefficient: the canonical test is exact at +-h and +-(h + 1), |c| is exact
    for every int32 (2^31 for INT32_MIN, which is never canonical), and the halves of its square add up to c^2."""
    half = (q - 1) // 2
    values = [0, 1, -1, half, -half, half + 1, -half - 1, half - q if half - q >= I32_MIN else -half - 2, I32_MAX, I32_MIN,
              I32_MIN + 1, 65535, 65536, -65536]
    path = tmp_path / "norm32.txt"
    path.write_text("".join("%d %d\n" % (q, c) for c in values))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([norm_driver, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    rows = [[int(v) for v in line.split()] for line in res.stdout.splitlines()]
    assert len(rows) == len(values)
    for c, (canon, al, lo, hi) in zip(values, rows):
        assert canon == int(-half <= c <= half), (q, c)
        assert al == abs(c) and lo + (hi << 32) == c * c, (q, c)
        assert lo < 2 ** 32 and hi < 2 ** 32
    assert rows[values.index(I32_MIN)][0] == 0
