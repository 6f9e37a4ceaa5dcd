"""CPU tier of the key planner (ring_zk_amd/csrc/rzk_keyplan.h): the host part of rzk_key_load — range test, classification,
entry indices, the list of general entries, the 2-norm bounds — compiled with g++ into tests/keyplan/keyplan_driver.cpp,
once under -fsanitize=address,undefined and once plain, and compared with a restatement on Python integers.

  * seeded keys of shapes (1,3,1), (2,5,2), (4,9,4) at N = 4, 64, 512 with, besides the reference layout, entries that are
    the constants 0, 1, -1, 2, "1 plus one non-zero at N-1", and +-(q-1)/2 throughout (each asserted to occur at every
    planted position, per shape, N and modulus): class and entry index of every position, the general list (SHA-256) and
    the count equal the restatement's;
  * every kinf, rounded to float32, is not below the exact 2-norm, and is not above (1 + 2e-6) times it: the sum of
    squares in a 64-bit-mantissa long double (N (q/2)^2 < 2^71, relative error below N 2^-64) times 1 + 1e-6;
  * a coefficient +-((q-1)/2 + 1) at the first or last coefficient of the first, a middle or the last entry is refused
    by plan_key_tables, the call of rzk_key.cpp, and neither the output struct nor the sentinel-filled tables that stand
    for the context's previous ones are touched;
  * what a refused load used to leave in the context ("Context walk"): the tables of the refused key
    up to the failing entry, KC_GENERAL / -1 beyond, while the previous key's images and count stay.  The planner
    (tests/plan/plan_driver.cpp) given those tables plans something else than under the previous key."""
import hashlib
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
Q_DEFAULT = 3515337053
Q_MAX = 4294606851      # the largest modulus rzk_ctx_create takes
SHAPES = [(1, 3, 1), (2, 5, 2), (4, 9, 4)]
SIZES = [4, 64, 512]
KC_ZERO, KC_ONE, KC_GENERAL = 0, 1, 2
OK, E_ARG, E_UNSUPPORTED = 0, -1, -4
SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")


def compile_driver(out_dir, source, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the host drivers")
    exe = str(out_dir / os.path.basename(source).replace(".cpp", ""))
    subprocess.check_call([gxx, "-std=c++17", "-O1", *(SANITIZE if sanitize else ()), "-Wall", "-Wextra", "-Werror",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, source)])
    return exe


@pytest.fixture(scope="module", params=[True, False], ids=["sanitized", "plain"])
def driver(request, tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("keyplan"), "keyplan/keyplan_driver.cpp", request.param)


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("keyplan_plan"), "plan/plan_driver.cpp", True)


# ---- keys -------------------------------------------------------------------------------------------------------------
def reference_key(rng, N, n, k, l, q):
    """[a1;a2] with a1 = [I_n | a1'], a2 = [0 | I_l | a2'], general entries uniform over the centred range."""
    half = (q - 1) // 2
    A = np.zeros((n + l, k, N), dtype=np.int64)
    for i in range(n):
        A[i, i, 0] = 1
        A[i, n:] = rng.integers(-half, half + 1, (k - n, N), dtype=np.int64)
    for i in range(l):
        A[n + i, n + i, 0] = 1
        A[n + i, n + l:] = rng.integers(-half, half + 1, (k - n - l, N), dtype=np.int64)
    return A


def special_entries(rng, N, q):
    half = (q - 1) // 2
    const = lambda v: np.array([v] + [0] * (N - 1), dtype=np.int64)   # noqa: E731
    one_tail = const(1)
    one_tail[N - 1] = int(rng.integers(1, half + 1)) * int(rng.choice([-1, 1]))
    return [const(0), const(1), const(-1), const(2), one_tail, np.full(N, half, dtype=np.int64),
            np.full(N, -half, dtype=np.int64), half * np.where(np.arange(N) % 2 == 0, -1, 1).astype(np.int64)]


SPECIAL_NAMES = ["0", "1", "-1", "2", "1 + tail", "+h", "-h", "-h, +h, ..."]


def keys_of(N, shape, q, seed):
    """The reference layout; then one key per special entry j, in which every entry (every second one where the key has
    more entries than there are specials: random general entries stay between them) takes special (position + j) mod 8,
    so that every planted position meets every special; then a key made of 0 / 1 entries only."""
    n, k, l = shape
    rng = np.random.default_rng(seed)
    entries = (n + l) * k
    keys = [reference_key(rng, N, n, k, l, q)]
    spec = special_entries(rng, N, q)
    assert len(spec) == len(SPECIAL_NAMES)
    planted = range(0, entries, 2 if entries > len(spec) else 1)
    for j in range(len(spec)):
        A = reference_key(rng, N, n, k, l, q).reshape(entries, N)
        for pos, e in enumerate(planted):
            A[e] = spec[(pos + j) % len(spec)]
        keys.append(A.reshape(n + l, k, N))
    only01 = np.zeros((entries, N), dtype=np.int64)
    only01[::2, 0] = 1
    keys.append(only01.reshape(n + l, k, N))
    return keys, spec


def count_specials(keys, spec):
    """how often each special entry occurs among the entries of `keys`"""
    polys = np.concatenate([A.reshape(-1, A.shape[-1]) for A in keys])
    return [int((polys == s).all(axis=1).sum()) for s in spec]


# ---- the restatement ----------------------------------------------------------------------------------------------------
def restate(A, q):
    """(classes, entries, general list, sums of squares) on Python integers; None for a key the range test refuses."""
    half = (q - 1) // 2
    classes, entries, general, ssq = [], [], [], []
    for poly in A.reshape(-1, A.shape[-1]):
        p = [int(v) for v in poly]
        if any(v > half or v < -half for v in p):
            return None
        if all(v == 0 for v in p):
            classes.append(KC_ZERO), entries.append(-1)
        elif p[0] == 1 and all(v == 0 for v in p[1:]):
            classes.append(KC_ONE), entries.append(-1)
        else:
            classes.append(KC_GENERAL), entries.append(len(general))
            general.append(p)
            ssq.append(sum(v * v for v in p))
    return classes, entries, general, ssq


def run_driver(exe, tmp_path, keys, q):
    N = keys[0].shape[-1]
    entries = keys[0].size // N
    path = tmp_path / "keys.bin"
    path.write_bytes(b"".join(np.ascontiguousarray(k, dtype="<i8").tobytes() for k in keys))
    res = subprocess.run([exe, str(q), str(N), str(entries), str(len(keys)), str(path)], capture_output=True, text=True, env=SAN_ENV)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    lines = [ln.split() for ln in res.stdout.splitlines()]
    assert len(lines) == len(keys)
    return lines


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d_%d" % s)
def test_classification_entries_and_norm_bounds(driver, tmp_path, shape, N):
    seen = set()
    for q in (Q_DEFAULT, Q_MAX):
        keys, spec = keys_of(N, shape, q, 20261021 + 1000 * N + sum(shape))
        entries = (shape[0] + shape[2]) * shape[1]
        planted = (entries + 1) // 2 if entries > len(spec) else entries
        counts = count_specials(keys[1:1 + len(spec)], spec)
        assert all(c >= planted for c in counts), dict(zip(SPECIAL_NAMES, counts))   # every special at every planted position
        for A, line in zip(keys, run_driver(driver, tmp_path, keys, q)):
            classes, entries, general, ssq = restate(A, q)
            assert line[0] == "ok", line[:3]
            assert int(line[1]) == len(general)
            assert [int(ch) for ch in line[2]] == classes
            assert [int(v) for v in line[3].split(",")] == entries
            flat = np.array(general, dtype="<i8").tobytes()
            assert line[4] == hashlib.sha256(flat).hexdigest()
            kinf = [] if line[5] == "-" else [float.fromhex(v) for v in line[5].split(",")]
            assert len(kinf) == len(general)
            for bound, s in zip(kinf, ssq):
                as_f32 = Fraction(float(np.float32(bound)))
                assert as_f32 * as_f32 >= s, (bound, s)                                   # an upper bound, as the kernels read it
                assert Fraction(bound) ** 2 <= Fraction(1000002, 1000000) ** 2 * s, (bound, s)
            seen.update(classes)
            seen.add(("n_general", len(general) == 0))
    assert seen >= {KC_ZERO, KC_ONE, KC_GENERAL, ("n_general", True), ("n_general", False)}


def test_special_entries_are_what_they_claim():
    """constants 0 / 1 are recognised, -1 and 2 and "1 plus a tail" are general, and the extremes have the largest norm."""
    N, q = 64, Q_DEFAULT
    spec = special_entries(np.random.default_rng(5), N, q)
    classes, _, _, ssq = restate(np.stack(spec)[None], q)
    assert classes == [KC_ZERO, KC_ONE] + [KC_GENERAL] * 6
    assert ssq[-3:] == [N * ((q - 1) // 2) ** 2] * 3 and int(spec[4][0]) == 1 and int(spec[4][N - 1]) != 0


def plants(A, q):
    """A with +-((q-1)/2 + 1) at the first / last coefficient of the first, a middle and the last entry: 12 keys."""
    N = A.shape[-1]
    entries = A.size // N
    out = []
    for e in (0, entries // 2, entries - 1):
        for j in (0, N - 1):
            for sign in (1, -1):
                bad = A.copy().reshape(entries, N)
                bad[e, j] = sign * ((q - 1) // 2 + 1)
                out.append((e, j, bad.reshape(A.shape)))
    return out


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d_%d" % s)
def test_out_of_range_coefficient_is_refused_and_nothing_is_written(driver, tmp_path, shape, N):
    for q in (Q_DEFAULT, Q_MAX):
        A = keys_of(N, shape, q, 77 + N)[0][0]
        bad = plants(A, q)
        assert len(bad) == 12 and all(restate(k, q) is None for _, _, k in bad)
        # the extreme values themselves are accepted at the same places
        edge = [np.clip(k, -((q - 1) // 2), (q - 1) // 2) for _, _, k in bad]
        lines = run_driver(driver, tmp_path, [k for _, _, k in bad] + edge, q)
        for (e, j, _), line in zip(bad, lines):
            assert line == ["refused", str(E_ARG), "1", "1"], (e, j, line)   # neither the KeyPlan nor the context's tables change
        assert [ln[0] for ln in lines[len(bad):]] == ["ok"] * len(edge)


# ---- what a refused load used to leave behind ---------------------------------------------------------------------------
def tables_after_refusal_before_the_fix(bad, q):
    """key_class / key_entry / count as rzk_key_load wrote them up to the entry that failed its range test: every entry
    KC_GENERAL / -1 first, then entry after entry classified — while the image store stayed the previous key's."""
    half = (q - 1) // 2
    polys = bad.reshape(-1, bad.shape[-1])
    classes, entries, count = [KC_GENERAL] * len(polys), [-1] * len(polys), 0
    for e, poly in enumerate(polys):
        if np.any(poly > half) or np.any(poly < -half):
            return classes, entries, count
        sub = restate(poly[None, None], q)
        classes[e] = sub[0][0]
        if classes[e] == KC_GENERAL:
            entries[e], count = count, count + 1
    raise AssertionError("the key is in range")


PG_MATVEC, PG_OPEN_COMMIT, PG_A1_RELATION = 0, 3, 5
TERM_KEY, KIND_MASK = 0, 0x3F


def plan_case(N, shape, classes, entries, pid, var):
    n, k, l = shape
    return " ".join(str(v) for v in (n, k, l, N.bit_length() - 1, int(N < 512), 1, 11, 1, 4, 1, repr(2.0), 1, pid, var,
                                     "".join(str(c) for c in classes), ",".join(str(e) for e in entries)))


def run_plans(exe, tmp_path, lines):
    import json

    path = tmp_path / "cases.txt"
    path.write_text("".join(ln + "\n" for ln in lines))
    res = subprocess.run([exe, "plan", str(path), "full"], capture_output=True, text=True, env=SAN_ENV)
    assert res.returncode == 0, res.stderr[-4000:]
    return [json.loads(ln) for ln in res.stdout.splitlines()]


@pytest.mark.parametrize("N,shape", [(512, (1, 3, 1)), (64, (1, 3, 1)), (1024, (2, 5, 2))])
def test_tables_left_by_a_refused_load_before_the_fix_plan_another_key(plan_driver, tmp_path, N, shape):
    """The refused keys of tests/test_gpu_context_walk.py (one general entry replaced by the constant 1, one identity entry
    made general; the bad coefficient at N-1 of the last entry, or at 0 of the first).  Under the tables the unfixed load
    left, a key product planned after the refusal is not the previous key's: its key terms index the previous key's image
    store with the refused key's numbering, or (an entry not yet visited: index -1) the plan is refused as too large."""
    n, k, l = shape
    q = Q_DEFAULT
    K0 = reference_key(np.random.default_rng(31), N, n, k, l, q)
    c0, e0, g0, _ = restate(K0, q)
    bad = K0.copy()
    bad[0, n] = 0
    bad[0, n, 0] = 1                                                   # a general entry becomes the constant 1
    bad[0, 0] = np.random.default_rng(32).integers(-5, 6, N)            # an identity entry becomes general
    outcomes = []
    for (row, col, j) in ((n + l - 1, k - 1, N - 1), (0, 0, 0)):
        refused = bad.copy()
        refused[row, col, j] = (q - 1) // 2 + 1
        assert restate(refused, q) is None
        c1, e1, count1 = tables_after_refusal_before_the_fix(refused, q)
        assert (c1, e1) != (c0, e0)
        for pid, var in ((PG_MATVEC, 4), (PG_MATVEC, 1), (PG_OPEN_COMMIT, 0), (PG_A1_RELATION, 0)):
            want, got = run_plans(plan_driver, tmp_path, [plan_case(N, shape, c0, e0, pid, var), plan_case(N, shape, c1, e1, pid, var)])
            assert want["status"] == OK
            key_idx = lambda r: [(t[4], t[3], t[5]) for t in r["terms"] if t[0] & KIND_MASK == TERM_KEY]   # noqa: E731  (image, operand polynomial)
            assert all(i < len(g0) for i, _, _ in key_idx(want))
            if got["status"] == OK:
                assert got["sha_program"] != want["sha_program"], (pid, var)
                assert key_idx(got) != key_idx(want)
                outcomes.append("other indices")
            else:
                assert got["status"] == E_UNSUPPORTED and got["overflow"] == 1
                outcomes.append("refused plan")
    print(N, shape, outcomes)
    assert "other indices" in outcomes and "refused plan" in outcomes
