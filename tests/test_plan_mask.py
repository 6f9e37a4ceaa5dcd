"""CPU tier of the "masks only" variant of PG_LIN_COMMIT2 (rzk_plan.h kMaskVar): the rows of
rzk_linear_mask_batch.  The planner driver of test_plan.py, unchanged, and its invariants (check_plan), imported.

  * the variant over the seeded shapes of test_plan.sweep_cases, at every N in {64, 512, 1024, 2048}: every invariant the
    kernels rely on, and what makes it the masks of the commit program: the rows of t = a1.y, a2.y, t' = a1.y' in the
    order and with the terms of the full program, no commitment row, no operand of x, gx, r, r', c, c';
  * kMaskVar | 1 (a fused norm check of masks, which carry no norm rule) is an argument error;
  * how many cases are E_UNSUPPORTED: the count is printed and capped at a quarter, as in test_plan.
"""
import pytest

import test_plan as TP
from test_plan import driver  # noqa: F401  (the fixture that builds tests/plan/plan_driver.cpp)

MASK_VAR = 2
NS = (64, 512, 1024, 2048)


def mask_cases():
    """One case per distinct environment of the seeded sweep, and the same environment at every N (the sweep draws one N
    per environment; the knobs that depend on N are drawn as test_plan draws them for that N)."""
    seen, cases = set(), []
    for c in TP.sweep_cases():
        env = {key: v for key, v in c.items() if key not in ("id", "var")}
        for N in NS:
            e = dict(env, N=N)
            if N < 512:
                e["rot"] = 0
            if N == 2048:
                e["group_max"] = min(e["group_max"], 2)
            key = TP.case_line(dict(e, id=TP.PG_LIN_COMMIT2, var=MASK_VAR))
            if key not in seen:
                seen.add(key)
                cases.append(dict(e, id=TP.PG_LIN_COMMIT2, var=MASK_VAR))
    return cases


def test_mask_variant_over_the_seeded_sweep(driver, tmp_path):
    cases = mask_cases()
    assert {c["N"] for c in cases} == set(NS) and len(cases) >= 4 * 40
    full = [dict(c, var=0) for c in cases]
    recs = TP.run_plans(driver, tmp_path, cases + full, full=True)
    masks, fulls = recs[:len(cases)], recs[len(cases):]
    unsupported, paths = 0, set()
    for c, r, rf in zip(cases, masks, fulls):
        if r["status"] == TP.E_UNSUPPORTED:
            unsupported += 1
            continue
        assert r["status"] == TP.OK, (TP.case_line(c), r["status"])
        try:
            TP.check_plan(c, r)
        except AssertionError as exc:
            raise AssertionError("%s: %s" % (TP.case_line(c), exc)) from exc
        paths.add(TP.PATHS[r["path"]])
        n, k, l = c["n"], c["k"], c["l"]
        rows, terms, adds = r["rows"], r["terms"], r["adds"]
        # 2n + l rows, all stored: t (operand 8), a2.y (10), t' (9), in the order of the full program
        assert [(row[4], row[6]) for row in rows] == [(8, i) for i in range(n)] + [(10, i) for i in range(l)] + [(9, i) for i in range(n)]
        assert all(row[5] == TP.MODE_STORE for row in rows) and r["polys_out"] == 2 * n + l
        # nothing but key products and plain additions of y (4) and y' (5): none of x, gx, r, r', c, c' is an operand
        assert all((t[0] & TP.KIND_MASK) == TP.TERM_KEY and t[3] in (4, 5) for t in terms)
        assert all((a[0] & TP.ADD_OP_MASK) in (4, 5) for a in adds)
        assert [p for i, p in enumerate(r["polys_in"]) if i not in (4, 5)] == [0] * (TP.MAX_OPERANDS - 2)
        assert not r["two_bit"] and not r["has_vec"] and not r["has_dkey"] and not r["shift"]
        if rf["status"] == TP.OK:   # the same rows as the tail of the full program: terms and additions, row by row
            tail = rf["rows"][2 * (n + l):]
            assert len(tail) == len(rows)
            for row, frow in zip(rows, tail):
                assert (row[1], row[3], row[4], row[5], row[6], row[7]) == (frow[1], frow[3], frow[4], frow[5], frow[6], frow[7])
                assert terms[row[0]:row[0] + row[1]] == rf["terms"][frow[0]:frow[0] + frow[1]]
                assert adds[row[2]:row[2] + row[3]] == rf["adds"][frow[2]:frow[2] + frow[3]]
    print("mask sweep: %d cases, %d unsupported, paths %s" % (len(cases), unsupported, sorted(paths)))
    assert unsupported * 4 <= len(cases), (unsupported, len(cases))
    assert "Small" in paths and len(paths) >= 2


def test_mask_variant_has_no_fused_check(driver, tmp_path):
    case = dict(N=512, n=1, k=3, l=1, rot=1, block_min_logn=11, use_groups=1, group_max=4, use_pairs=1,
                slot_share_min=2.0, vec_rows=1, key_class="102012", id=TP.PG_LIN_COMMIT2, var=MASK_VAR | 1)
    assert TP.run_plans(driver, tmp_path, [case])[0]["status"] == TP.E_ARG
    for var in (0, 1, MASK_VAR):
        assert TP.run_plans(driver, tmp_path, [dict(case, var=var)])[0]["status"] == TP.OK
