"""CPU tier of the slab lists (ring_zk_amd/csrc/rzk_slabs.h): the table every entry point's NULL test,
alignment test, staging plan and convert plan are derived from, held against the declarations of include/rzk.h.  The table is
printed by tests/slabs/slabs_driver.cpp, a g++ program under -fsanitize=address,undefined that includes only that header and
runs as a process; what a parameter's name means is stated here, independent of the C++ header.  No GPU needed."""
import os
import re
import subprocess

import pytest

from test_abi_linear32 import declarations
from test_linear32_host import HERE, build

# (n, k, l, V): the four values differ from each other and from most of their sums and products, so a swapped count shows;
# the second point has n == l, the shape of every protocol context of the GPU suite.  rows: the operand of the Mat calls.
POINTS = [(2, 7, 3, 5), (2, 5, 2, 3)]
ROWS = 11

# entry points that take their slabs from a schema or a caller's rows[], or have one output: not in the table
OWN_PATH = ("rzk_key_load", "rzk_ntt_forward_batch", "rzk_ntt_inverse_batch", "rzk_wire_decode_batch", "rzk_wire_encode_batch",
            "rzk_fs_challenge_batch", "rzk_fs_challenge32_batch", "rzk_reject_batch", "rzk_packed_encode_batch",
            "rzk_packed_decode_batch", "rzk_packed_encode32_batch", "rzk_packed_decode32_batch", "rzk_xof_uniform_batch")
OPTIONAL = {("commit", "ok"), ("open_commit", "ok"), ("linear_commit", "ok"), ("sum_commit", "ok")}   # and every addend, f, E
COMPANION_BYTES = {"ok": 1, "accept": 1, "eq": 1, "rounds": 1, "coin": 8, "E": 8}
# parameters of the ring / Mat calls, whose names say nothing about a proof: polynomials per entry of the batch
MAT = {
    "polymul": {"a": "1", "b": "1", "out": "1"}, "add": {"a": "1", "b": "1", "out": "1"}, "sub": {"a": "1", "b": "1", "out": "1"},
    "canonicalize": {"in": "1", "out": "1"}, "narrow": {"in": "1", "out": "1"}, "widen": {"in": "1", "out": "1"},
    "matvec": {"v": "k", "addend": "rows", "out": "rows"}, "cmul": {"m": "rows", "p": "1", "out": "rows"},
    "norm2_le": {"v": "rows"}, "eq": {"a": "rows", "b": "rows"}, "eq32": {"a": "rows", "b": "rows"},
}


def polynomials(call, name, n, k, l, V):
    """What the header's naming says a coefficient slab holds per proof."""
    if call in MAT:
        return {"1": 1, "k": k, "rows": ROWS}[MAT[call][name]]
    base = name[:-4] if name.endswith("_out") else name
    per = {"x": l, "r": k, "y": k, "z": k, "c": n + l, "t": n, "u": l, "g": 1, "d": 1, "f": 1}
    if base in per:                      # one polynomial vector
        return per[base]
    if base.endswith("p"):               # the primed vector of Linear / Sum: rp, yp, zp, cp, tp
        return per[base[:-1]]
    assert base.endswith("s"), (call, name)   # the V summands of Sum: xs, rs, ys, zs, cs, ts, gs
    return V * per[base[:-1]]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = build(tmp_path_factory, "slabs", "slabs_driver")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = {}
    for n, k, l, V in POINTS:
        res = subprocess.run([exe] + [str(v) for v in (n, k, l, V, ROWS)], capture_output=True, text=True, env=env)
        assert res.returncode == 0, res.stderr[-4000:]
        calls, key_rows = {}, None
        for line in res.stdout.splitlines():
            f = line.split()
            if f[0] == "key_rows":
                key_rows = [int(v) for v in f[1:]]
                continue
            call, both, name, cls, direction, need, count = f
            entry = calls.setdefault(call, {"both": both == "1", "slabs": []})
            assert entry["both"] == (both == "1")
            entry["slabs"].append((name, cls, direction, need, int(count)))
        out[(n, k, l, V)] = (calls, key_rows)
    return out


def pointer_params(decl):
    """(const?, type, name) of every pointer parameter that is a slab or a companion: everything but the context, the nonce,
    aux32 and rounds_run, which are scalars of the call passed by address."""
    got = []
    for a in decl:
        m = re.fullmatch(r"(const )?(int64_t|int32_t|uint8_t)\* (\w+)", a)
        if m and m.group(3) not in ("aux32",):
            got.append((bool(m.group(1)), m.group(2), m.group(3)))
    return got


def symbol(call, wide32=False):
    return "rzk_%s%s_batch" % (call, "32" if wide32 else "")


def test_coverage(table):
    decl = declarations()
    calls = table[POINTS[0]][0]
    listed = {symbol(c) for c in calls} | {symbol(c, True) for c, e in calls.items() if e["both"]}
    for name in listed:
        assert name in decl and name + "_dev" in decl, f"{name}: in the table, not declared as a host / _dev pair"
        assert decl[name] == decl[name + "_dev"], f"{name}: host and device form differ"
    pairs = {n for n in decl if n + "_dev" in decl}
    assert pairs - set(OWN_PATH) == listed, (sorted(pairs - set(OWN_PATH) - listed), sorted(listed - pairs))
    assert not set(OWN_PATH) & listed and set(OWN_PATH) <= pairs
    for point in POINTS[1:]:
        assert set(table[point][0]) == set(calls)


@pytest.mark.parametrize("point", POINTS)
def test_order_roles_and_counts(table, point):
    n, k, l, V = point
    decl = declarations()
    calls, _ = table[point]
    for call, entry in calls.items():
        params = pointer_params(decl[symbol(call)])
        assert [name for name, *_ in entry["slabs"]] == [p[2] for p in params], f"{call}: order or names differ from the header"
        for (name, cls, direction, need, count), (const, ctype, _) in zip(entry["slabs"], params):
            where = f"{call}.{name}"
            assert (direction == "in") == const, f"{where}: const <=> read"
            optional = (call, name) in OPTIONAL or name in ("addend", "f", "E")
            assert (need == "opt") == optional, f"{where}: optional"
            if name in COMPANION_BYTES:
                assert cls == "bytes" and count == COMPANION_BYTES[name], where
                assert ctype == ("int64_t" if count == 8 else "uint8_t"), where
            else:
                assert cls == "coef" and ctype in ("int64_t", "int32_t"), where
                assert count == polynomials(call, name, n, k, l, V), f"{where}: {count} polynomials per proof"


def test_widths(table):
    decl = declarations()
    for call, entry in table[POINTS[0]][0].items():
        if not entry["both"]:
            continue
        wide, narrow = pointer_params(decl[symbol(call)]), pointer_params(decl[symbol(call, True)])
        want = [(c, t if name in COMPANION_BYTES else "int32_t", name) for c, t, name in wide]
        assert narrow == want, f"{call}: the 32-bit sibling has another list"
        assert all(t == "int64_t" for _, t, name in wide if name not in COMPANION_BYTES or COMPANION_BYTES[name] == 8), call


@pytest.mark.parametrize("point", POINTS)
def test_key_rows(table, point):
    n, _, l, _ = point
    assert table[point][1] == [n, l, n + l, 0, 0]   # RZK_KEY_A1, RZK_KEY_A2, RZK_KEY_A, and two values that select nothing


SOURCES = ("rzk_host.cpp", "rzk_protocols.cpp", "rzk_codec.cpp", "rzk_slab32.cpp", "rzk_prove_loop.cpp")


def function_bodies():
    """name -> text of every function defined at column 0 in the five files of the entry points (up to the closing brace at
    column 0)."""
    bodies = {}
    for src in SOURCES:
        code = open(os.path.join(HERE, "..", "ring_zk_amd", "csrc", src)).read()
        for m in re.finditer(r"^(?:int|bool) (\w+)\([^;{]*\) \{\n(.*?)^\}\n", code, flags=re.M | re.S):
            bodies[m.group(1)] = m.group(2)
    return bodies


def lists_used(bodies, name, depth=2):
    """The kSlabs* lists the function names, itself or through the one function of these files its return statement calls."""
    used = set(re.findall(r"\bkSlabs\w+", bodies[name]))
    if not used and depth:
        for callee in re.findall(r"return (\w+)(?:<\w+>)?\(c,", bodies[name]):
            if callee in bodies:
                used |= lists_used(bodies, callee, depth - 1)
    return used


def test_every_symbol_uses_its_own_list(table):
    """The table test above holds each list against its declaration; this one holds each entry point against its list: the
    only list rzk_<call>[32]_batch[_dev] names, directly or through the template it forwards to, is kSlabs<Call>."""
    bodies = function_bodies()
    for call, entry in table[POINTS[0]][0].items():
        want = {"kSlabs" + "".join(w.capitalize() for w in call.split("_"))}
        for wide32 in ([False, True] if entry["both"] else [False]):
            for name in (symbol(call, wide32), symbol(call, wide32) + "_dev"):
                assert name in bodies, f"{name}: no definition found"
                assert lists_used(bodies, name) == want, f"{name} names {sorted(lists_used(bodies, name))}, not {sorted(want)}"
