"""CPU tier of the recover ("recompute") variants of the verifier row programs (rzk_plan.h, kRecoverVar),
on the stand-alone tests/plan/plan_driver.cpp build of tests/test_plan.py (g++ -fsanitize=address,undefined).

Over the seeded shape and knob sweep of test_plan.py, for every program that has a recover form: the recover variant has
the status of the compare variant of the same case, and where that is OK the same rows, fused-check marks and launch
facts except that every relation / result row is stored into the operand the compare form subtracts, nothing is left to
test against zero, and no row reads what the program stores.  Programs without a recover form stay argument errors."""
import numpy as np

from test_plan import (ADD_OP_MASK, CHECK, CHECK2, DKEY_VAR, E_ARG, E_UNSUPPORTED, KIND_MASK, MODE_STORE, NPROG, OK, PATHS,
                       PG_A1_RELATION, PG_LIN_V1, PG_LIN_V1B, PG_LIN_V2, PG_LIN_V2B, PG_REL_ROT, PG_SUM_V3, PG_SUM_V4,
                       TERM_SHIFT, TERM_VEC, case_line, check_plan, driver, run_plans, sweep_cases)  # noqa: F401

RECOVER_VAR = 0x40000
# id -> result operands of the recover form, in row order: [(operand the rows are stored into, "n" or "l" rows)]
RESULTS = {
    PG_A1_RELATION: [(1, "n")],
    PG_REL_ROT: [(1, "n")],
    PG_LIN_V1B: [(2, "n"), (3, "n")],      # then the e / e' rows, stored in both forms
    PG_LIN_V2B: [(3, "l")],
    PG_SUM_V3: [(5, "l")],
    PG_SUM_V4: [(3, "l")],
}


def recover_cases():
    """The sweep's cases of the recover-capable programs, plus for each a twin with the Sum / Linear variant knobs the
    sweep draws (V, DKEY, the fused-check bit) so that every id meets both values of its own bits."""
    rng = np.random.default_rng(20261019)
    out = []
    for c in sweep_cases():
        if c["id"] not in RESULTS:
            continue
        out.append(c)
        twin = dict(c)
        if c["id"] in (PG_A1_RELATION, PG_LIN_V1B):
            twin["var"] = c["var"] ^ 1
        elif c["id"] == PG_SUM_V3:
            twin["var"] = int(rng.integers(1, 6)) | (c["var"] & DKEY_VAR ^ DKEY_VAR)
        elif c["id"] == PG_LIN_V2B:
            twin["var"] = c["var"] ^ DKEY_VAR
        else:
            continue
        out.append(twin)
    return out


def reads_of(r):
    """(operand, offset) of everything the program loads: b operands, a operands of non-key products, additions."""
    got = set()
    for t in r["terms"]:
        got.add((t[3], t[5]))
        if (t[0] & KIND_MASK) in (TERM_VEC, TERM_SHIFT):   # (a_op, a_off) is an operand; key / image terms have none
            got.add((t[2], t[4]))
    for a in r["adds"]:
        got.add((a[0] & ADD_OP_MASK, a[2]))
    return got


def marks_of(r):
    """The fused-check marks as (what is marked, operand, offset, mark bits), independent of table positions."""
    out = []
    for t in r["terms"]:
        if t[0] & (CHECK | CHECK2):
            out.append(("term", t[3], t[5], t[0] & (CHECK | CHECK2)))
    for a in r["adds"]:
        if a[0] & (CHECK | CHECK2):
            out.append(("add", a[0] & ADD_OP_MASK, a[2], a[0] & (CHECK | CHECK2)))
    return sorted(out)


def test_recover_variants_over_the_sweep(driver, tmp_path):
    cases = recover_cases()
    rec_cases = [dict(c, var=c["var"] | RECOVER_VAR) for c in cases]
    cmp_recs = run_plans(driver, tmp_path, cases, full=True)
    rec_recs = run_plans(driver, tmp_path, rec_cases, full=True)
    ids, paths, planned = set(), set(), 0
    for c, rc_case, a, b in zip(cases, rec_cases, cmp_recs, rec_recs):
        where = case_line(rc_case)
        assert b["status"] == a["status"], (where, a["status"], b["status"])
        if a["status"] != OK:
            assert a["status"] == E_UNSUPPORTED
            continue
        planned += 1
        try:
            check_plan(rc_case, b)
        except AssertionError as exc:
            raise AssertionError("%s: %s" % (where, exc)) from exc
        dims = {"n": c["n"], "l": c["l"]}
        assert b["nrows"] == a["nrows"], where
        assert marks_of(b) == marks_of(a), where
        # the result rows, in order, store into their operand at their own index; every other row is as it was
        want = [(op, i) for op, which in RESULTS[c["id"]] for i in range(dims[which])]
        assert len(want) <= len(b["rows"]), where
        for i, (ra, rb) in enumerate(zip(a["rows"], b["rows"])):
            if i < len(want):
                assert ra[5] != MODE_STORE and rb[5] == MODE_STORE and (rb[4], rb[6]) == want[i], (where, i)
                # the same products and rotations; one addition less: the operand it is now stored into
                assert (rb[1], rb[7], rb[3]) == (ra[1], ra[7], ra[3] - 1), (where, i)
                sub = [x for x in a["adds"][ra[2]:ra[2] + ra[3]] if (x[0] & ADD_OP_MASK, x[2]) == want[i]]
                assert len(sub) == 1 and sub[0][1] == -1, (where, i)
                terms_a = a["terms"][ra[0]:ra[0] + ra[1] + ra[7]]
                terms_b = b["terms"][rb[0]:rb[0] + rb[1] + rb[7]]
                assert terms_a == terms_b, (where, i)
                adds_a = [x for x in a["adds"][ra[2]:ra[2] + ra[3]] if x is not sub[0]]
                assert adds_a == b["adds"][rb[2]:rb[2] + rb[3]], (where, i)
            else:
                assert ra[5] == MODE_STORE and (rb[0], rb[1], rb[3:]) == (ra[0], ra[1], ra[3:]), (where, i)
                assert a["adds"][ra[2]:ra[2] + ra[3]] == b["adds"][rb[2]:rb[2] + rb[3]], (where, i)
        assert all(row[5] == MODE_STORE for row in b["rows"]), where           # no MODE_ZERO row is left
        stored = {(row[4], row[6]) for row in b["rows"]}
        assert len(stored) == len(b["rows"]), where                            # every row its own polynomial
        assert not (stored & reads_of(b)), where                               # no row reads what the program stores
        assert b["polys_out"] == a["polys_out"] + len(want) == len(b["rows"]), where
        # the launch facts the path depends on are those of the compare form: same kernel, same tables
        for key in ("has_vec", "has_dkey", "has_dd", "shift", "has_shift", "two_bit", "ngroups", "nblocks", "nslots", "nunits",
                    "work", "path", "paired"):
            assert b[key] == a[key], (where, key)
        ids.add(c["id"])
        paths.add(PATHS[b["path"]])
    print("recover sweep: %d cases, %d planned, paths %s" % (len(cases), planned, sorted(paths)))
    assert ids == set(RESULTS)
    assert {"Small", "Shift", "Units", "Rows"} <= paths, paths


def test_programs_without_a_recover_form_are_argument_errors(driver, tmp_path):
    env = dict(N=512, n=1, k=3, l=1, rot=1, block_min_logn=11, use_groups=1, group_max=4, use_pairs=1,
               slot_share_min=2.0, vec_rows=1, key_class="102012")
    cases = [dict(env, id=pid, var=RECOVER_VAR | (1 if pid in (10, 11, 12, 13, 18, 2, 4) else 0))
             for pid in range(NPROG + 1) if pid not in RESULTS]
    assert {PG_LIN_V1, PG_LIN_V2, NPROG} <= {c["id"] for c in cases}   # the non-rearranged Linear pair; id 22
    got = run_plans(driver, tmp_path, cases)
    assert [g["status"] for g in got] == [E_ARG] * len(cases)
    # ... and the same ids without the bit plan as always (id 22 stays an argument error)
    plain = run_plans(driver, tmp_path, [dict(c, var=c["var"] & ~RECOVER_VAR) for c in cases])
    assert [g["status"] for g in plain] == [OK] * (len(cases) - 1) + [E_ARG]
