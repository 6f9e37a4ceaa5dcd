"""CPU tier of the row-program planner (ring_zk_amd/csrc/rzk_plan.h), compiled with g++ under
-fsanitize=address,undefined into tests/plan/plan_driver.cpp.

  * Pinned plans: tests/golden/plans.jsonl holds, for every distinct planner input the GPU suite, its random-shape knob
    sets and a few direct calls reached, what the planner computed BEFORE it moved into the header (status, scalar
    facts, SHA-256 of every uploaded table, launch path).  plan_program must reproduce each record exactly.
  * Invariants, over a seeded sweep of shapes, key classifications and knobs, for every ProgId: what the kernels rely on
    when they walk the tables (coverage of rows by units / groups / blocks, slot references, pairs, fused-check marks,
    traffic counts, index bounds).  These do not lean on the pinned records.
"""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "plans.jsonl")

# rzk_plan.h / rzk_dev.h
(PG_MATVEC, PG_POLYMUL, PG_CMUL, PG_OPEN_COMMIT, PG_RESPONSE, PG_A1_RELATION, PG_LIN_COMMIT2, PG_LIN_U, PG_LIN_V1,
 PG_LIN_V2, PG_SUM_XP, PG_SUM_U, PG_SUM_W2, PG_SUM_V3, PG_COMMIT, PG_COMMIT_VERIFY, PG_A1Z, PG_REL_ROT, PG_SUM_D,
 PG_SUM_V4, PG_LIN_V1B, PG_LIN_V2B) = range(22)
NPROG = 22
DKEY_VAR, OIMG_VAR = 0x10000, 0x20000
OK, E_ARG, E_UNSUPPORTED = 0, -1, -4
PATHS = ["Small", "Shift", "Blocks", "Groups", "Slots", "Rows", "Units"]
TERM_KEY, TERM_VEC, TERM_SHIFT, TERM_DKEY, TERM_DD, KIND_MASK = 0, 1, 2, 3, 4, 0x3F
CHECK, CHECK2, ADD_OP_MASK = 0x80, 0x40, 0x3F
MODE_STORE = 0
NONE16 = 0xFFFF
MAX_OPERANDS, MAX_ROWS, MAX_TERMS, MAX_ADDS, MAX_SLOTS, BLOCK_MAX_ROWS, BLOCK_MAX_SLOTS = 12, 48, 640, 128, 512, 16, 9

FACTS = ["nrows", "nunits", "work", "has_vec", "nslots", "np_store", "ngroups", "nblocks", "has_dkey", "has_dd", "shift",
         "has_shift", "two_bit", "polys_out", "polys_in", "paired", "sha_program", "sha_wave", "sha_slots", "sha_blocks",
         "path"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the planner driver")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "plan", "plan_driver.cpp")])
    return exe


SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")


def case_line(c):
    """The driver's input line of a case: a dict with N, n, k, l, the knobs, id, var and the key's classification."""
    logn = c["N"].bit_length() - 1
    return " ".join(str(v) for v in (
        c["n"], c["k"], c["l"], logn, int(c["N"] < 512), c["rot"], c["block_min_logn"], c["use_groups"], c["group_max"],
        c["use_pairs"], repr(float(c["slot_share_min"])), c["vec_rows"], c["id"], c["var"], c["key_class"] or "-"))


def run_plans(exe, tmp_path, cases, full=False):
    path = tmp_path / "cases.txt"
    path.write_text("".join(case_line(c) + "\n" for c in cases))
    res = subprocess.run([exe, "plan", str(path)] + (["full"] if full else []), capture_output=True, text=True, env=SAN_ENV)
    assert res.returncode == 0, res.stderr[-4000:]
    out = [json.loads(line) for line in res.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def test_driver_sha256_is_sha256(driver):
    for text in ["", "abc", "x" * 55, "y" * 56, "z" * 64, "row programs " * 500]:
        got = subprocess.run([driver, "sha", text], capture_output=True, text=True, env=SAN_ENV, check=True).stdout.strip()
        assert got == hashlib.sha256(text.encode()).hexdigest()


# ---- a. plans pinned at the parent ------------------------------------------------------------------------------------
def load_golden():
    """The records as dicts, one per planner input.  The file's first line names the fields.  An "out" line is one distinct
    result (a result whose status is not OK ends after its status; polys_in is written without its trailing zeros); an
    "env" line is one shape, knob set and key with the [id, var, index of the out line] of every plan recorded under it."""
    with open(GOLDEN) as f:
        lines = [json.loads(line) for line in f if line.strip()]
    names, outs, recs = lines[0], [ln["out"] for ln in lines[1:] if "out" in ln], []
    for ln in lines[1:]:
        for pid, var, out in ln.get("plans", []):
            rec = dict(zip(names["env"], ln["env"]), id=pid, var=var, **dict(zip(names["out"], outs[out])))
            if "polys_in" in rec:
                rec["polys_in"] = rec["polys_in"] + [0] * (MAX_OPERANDS - len(rec["polys_in"]))
            recs.append(rec)
    return recs


def test_pinned_plans_cover_the_planner():
    recs = load_golden()
    ok = [r for r in recs if r["status"] == OK]
    assert {r["id"] for r in ok} == set(range(NPROG)), "every ProgId"
    assert {PATHS[r["path"]] for r in ok} == set(PATHS), "every launch path, Small included"
    assert any(r["var"] & DKEY_VAR for r in ok) and any(r["var"] & OIMG_VAR for r in ok)
    assert any(r["two_bit"] for r in ok) and any(r["paired"] for r in ok)
    assert any(r["status"] == E_UNSUPPORTED for r in recs)
    inputs = [case_line(r) for r in recs]
    assert len(set(inputs)) == len(inputs), "one record per distinct planner input"


def test_pinned_plans_replay_exactly(driver, tmp_path):
    recs = load_golden()
    got = run_plans(driver, tmp_path, recs)
    for want, have in zip(recs, got):
        assert have["status"] == want["status"], (case_line(want), have)
        if want["status"] == OK:
            diff = {key: (want[key], have[key]) for key in FACTS if want[key] != have[key]}
            assert not diff, (case_line(want), diff)


# ---- b. invariants ----------------------------------------------------------------------------------------------------
def draw_key(rng, n, k, l, mode):
    """Classification of [a1;a2], (n+l) x k: 0 zero, 1 one, 2 general."""
    kc = np.zeros((n + l, k), dtype=np.int64)
    if mode == "reference":          # a1 = [I_n | a1'], a2 = [0 | I_l | a2'] (commit.rs:33-60)
        for i in range(n):
            kc[i, i], kc[i, n:] = 1, 2
        for i in range(l):
            kc[n + i, n + i], kc[n + i, n + l:] = 1, 2
    elif mode == "dense":
        kc[:] = 2
    elif mode == "banded":           # as many entries in every row, in other columns: equal counts, unequal operand lists
        for i in range(n + l):
            for j in range(min(2, k)):
                kc[i, (i + j) % k] = 2
    elif mode == "mixed":            # zero, one and general entries anywhere
        kc[:] = rng.choice([0, 1, 2], size=kc.shape, p=[0.3, 0.2, 0.5])
    else:                            # "sparse": mostly zero, some columns empty
        kc[:] = rng.choice([0, 1, 2], size=kc.shape, p=[0.6, 0.1, 0.3])
    return "".join(str(v) for v in kc.reshape(-1))


CHECKED = {   # id -> [(operand, CHECK or CHECK2)] of the fused-check variant (var | 1); each operand has k polynomials
    PG_OPEN_COMMIT: [(1, CHECK)], PG_COMMIT: [(1, CHECK)], PG_COMMIT_VERIFY: [(1, CHECK)], PG_A1Z: [(0, CHECK)],
    PG_A1_RELATION: [(0, CHECK)], PG_LIN_COMMIT2: [(2, CHECK), (3, CHECK2)], PG_LIN_V1: [(0, CHECK), (1, CHECK)],
    PG_LIN_V1B: [(0, CHECK), (1, CHECK)],
}
SCALAR = {PG_CMUL, PG_LIN_U, PG_LIN_V1, PG_LIN_V2, PG_LIN_V2B, PG_SUM_XP, PG_SUM_U, PG_SUM_W2, PG_SUM_V3, PG_SUM_D}


def draw_var(rng, pid):
    if pid == PG_MATVEC:
        var = int(rng.integers(0, 6))
    elif pid in (PG_CMUL, PG_SUM_XP, PG_SUM_U, PG_SUM_W2, PG_SUM_V3, PG_SUM_D):
        var = int(rng.integers(1, 6))
    elif pid == PG_RESPONSE:
        var = int(rng.integers(1, 3))
    elif pid == PG_COMMIT_VERIFY:
        var = int(rng.integers(0, 4))
    elif pid in CHECKED:
        var = int(rng.integers(0, 2))
    else:
        var = 0
    if pid in SCALAR and rng.random() < 0.5:
        var |= DKEY_VAR
        if pid == PG_SUM_D and rng.random() < 0.5:
            var |= OIMG_VAR
    return var


def sweep_cases():
    rng = np.random.default_rng(20261017)
    cases = []
    for e in range(48):
        N = int(rng.choice([64, 512, 1024, 2048]))
        n = int(rng.integers(1, 5))
        l = int(rng.integers(1, n + 1))
        k = n + l + int(rng.integers(0, 4))          # 48 rows / 640 terms hold every program up to (4, 11, 4), V = 5
        env = dict(N=N, n=n, k=k, l=l, rot=int(rng.integers(0, 2)) if N >= 512 else 0,
                   block_min_logn=int(rng.choice([10, 11, 12])), use_groups=int(rng.integers(0, 2)),
                   group_max=int(rng.integers(1, 3 if N == 2048 else 5)), use_pairs=int(rng.integers(0, 2)),
                   slot_share_min=float(rng.choice([0.0, 1.0, 1.5, 2.0])), vec_rows=int(rng.integers(0, 2)),
                   key_class=draw_key(rng, n, k, l, ["reference", "reference", "dense", "mixed", "sparse", "banded"][e % 6]))
        for pid in range(NPROG):
            for _ in range(2):
                cases.append(dict(env, id=pid, var=draw_var(rng, pid)))
    return cases


def check_plan(c, r):
    """Every invariant of one plan; c the case, r the driver's full record."""
    rows, terms, adds = r["rows"], r["terms"], r["adds"]
    kind = lambda t: t[0] & KIND_MASK   # noqa: E731
    b_of = lambda t: (t[3], t[5])       # noqa: E731
    a_of = lambda t: (t[2], t[4])       # noqa: E731
    general = c["key_class"].count("2")
    # index bounds; the rows partition the term and addition tables in order
    assert r["nrows"] == len(rows) <= MAX_ROWS and len(terms) <= MAX_TERMS and len(adds) <= MAX_ADDS
    t_at = a_at = 0
    for term0, nterms, add0, nadds, out_op, mode, out_off, nshift in rows:
        assert (term0, add0) == (t_at, a_at) and out_op < MAX_OPERANDS
        t_at, a_at = t_at + nterms + nshift, a_at + nadds
        assert all(kind(t) != TERM_SHIFT for t in terms[term0:term0 + nterms])
        assert all(kind(t) == TERM_SHIFT for t in terms[term0 + nterms:term0 + nterms + nshift])
    assert (t_at, a_at) == (len(terms), len(adds))
    for t in terms:
        assert t[3] < MAX_OPERANDS and t[1] in (1, -1) and kind(t) <= TERM_DD
        assert t[4] < general if kind(t) == TERM_KEY else (t[2] < MAX_OPERANDS or kind(t) in (TERM_DKEY, TERM_DD))
    assert all((a[0] & ADD_OP_MASK) < MAX_OPERANDS for a in adds)
    assert r["polys_out"] == sum(1 for row in rows if row[5] == MODE_STORE)
    row_terms = lambda i: terms[rows[i][0]:rows[i][0] + rows[i][1]]   # noqa: E731
    path = PATHS[r["path"]]
    # units: every row in exactly one, counting a pair's rowB
    if c["N"] >= 512:
        units, items = r["units"], r["items"]
        assert r["nunits"] == len(units) <= MAX_ROWS and len(items) <= MAX_TERMS
        seen = []
        for rowA, rowB, item0, nitems in units:
            seen.append(rowA)
            mine = row_terms(rowA)
            assert nitems == len(mine) and item0 + nitems <= len(items)
            for t, it in zip(mine, items[item0:item0 + nitems]):
                assert (it[2], it[4]) == b_of(t) and it[8] == t[1]
                assert it[0] == (1 if kind(t) == TERM_VEC else 0)
            if rowB != NONE16:
                assert c["use_pairs"]
                seen.append(rowB)
                tb = row_terms(rowB)
                assert len(tb) == 1 and rows[rowB][7] == 0 and kind(tb[0]) == TERM_KEY and b_of(tb[0]) == b_of(mine[-1])
                last = items[item0 + nitems - 1]
                assert (last[7], last[9]) == (tb[0][4], tb[0][1])
            else:
                assert all(it[7] == NONE16 for it in items[item0:item0 + nitems])
        assert sorted(seen) == list(range(len(rows)))
    else:
        assert path == "Small" and "units" not in r
    # groups
    assert r["prog_ngroups"] == r["ngroups"] == len(r["groups"])
    if r["ngroups"]:
        covered = []
        for row0, count in r["groups"]:
            assert 1 <= count <= c["group_max"]
            covered += range(row0, row0 + count)
            lists = [[b_of(t) for t in row_terms(i)] for i in range(row0, row0 + count)]
            assert all(x == lists[0] for x in lists)
        assert covered == list(range(len(rows)))
    # blocks
    if r["nblocks"]:
        assert r["nblocks"] == len(r["blocks"]) and len(r["block_slots"]) <= MAX_SLOTS
        covered = []
        for row0, nrows, slot0, nslots in r["blocks"]:
            assert 1 <= nrows <= BLOCK_MAX_ROWS and 1 <= nslots <= BLOCK_MAX_SLOTS and slot0 + nslots <= len(r["block_slots"])
            covered += range(row0, row0 + nrows)
            for i in range(row0, row0 + nrows):
                assert rows[i][7] == 0
                for j, t in enumerate(row_terms(i)):
                    s = r["term_slot"][rows[i][0] + j]
                    assert s < nslots and tuple(r["block_slots"][slot0 + s][:2]) == b_of(t) and kind(t) == TERM_KEY
        assert covered == list(range(len(rows)))
    # slots
    if r["nslots"]:
        assert r["nslots"] == len(r["slots"]) <= MAX_SLOTS
        for t, (sa, sb) in zip(terms, r["term_ab"]):
            assert sb < r["nslots"] and tuple(r["slots"][sb][:2]) == b_of(t)
            if kind(t) == TERM_VEC:
                assert sa < r["nslots"] and tuple(r["slots"][sa][:2]) == a_of(t)
    # fused checks: one mark per polynomial of the checked vectors, visible to the kernel of the chosen path
    marks = CHECKED.get(c["id"], []) if c["var"] & 1 else []
    assert r["two_bit"] == int(any(m == CHECK2 for _, m in marks))
    for op, mark in marks:
        for j in range(c["k"]):
            on_terms = [i for i, t in enumerate(terms) if b_of(t) == (op, j) and t[0] & mark]
            on_adds = [a for a in adds if (a[0] & ADD_OP_MASK, a[2]) == (op, j) and a[0] & mark]
            assert len(on_terms) + len(on_adds) == 1, (op, j)
            if not on_terms:
                continue   # additions stay in Program::rows on every path
            if path == "Units":
                assert any((it[2], it[4]) == (op, j) and it[1] & mark for it in r["items"])
            elif path == "Slots":
                assert r["slots"][r["term_ab"][on_terms[0]][1]][2] == 1
            elif path == "Blocks":
                blk = next(b for b in r["blocks"] if rows[b[0]][0] <= on_terms[0] < rows[b[0] + b[1] - 1][0] + rows[b[0] + b[1] - 1][1])
                assert r["block_slots"][blk[2] + r["term_slot"][on_terms[0]]][2] == 1
    if not marks:
        assert not any(t[0] & (CHECK | CHECK2) for t in terms) and not any(a[0] & (CHECK | CHECK2) for a in adds)


def test_invariants_over_a_seeded_sweep(driver, tmp_path):
    cases = sweep_cases()
    recs = run_plans(driver, tmp_path, cases, full=True)
    unsupported = 0
    paths, ids = set(), set()
    for c, r in zip(cases, recs):
        if r["status"] == E_UNSUPPORTED:
            unsupported += 1
            continue
        assert r["status"] == OK, (case_line(c), r["status"])
        try:
            check_plan(c, r)
        except AssertionError as exc:
            raise AssertionError("%s: %s" % (case_line(c), exc)) from exc
        paths.add(PATHS[r["path"]])
        ids.add(c["id"])
    print("sweep: %d cases, %d unsupported, paths %s" % (len(cases), unsupported, sorted(paths)))
    assert unsupported * 4 <= len(cases), (unsupported, len(cases))
    assert ids == set(range(NPROG)) and paths == set(PATHS)


def test_unknown_program_is_an_argument_error(driver, tmp_path):
    case = dict(N=512, n=1, k=3, l=1, rot=1, block_min_logn=11, use_groups=1, group_max=4, use_pairs=1,
                slot_share_min=2.0, vec_rows=1, key_class="102012", id=NPROG, var=0)
    assert run_plans(driver, tmp_path, [case])[0]["status"] == E_ARG
