"""The exact kernel instantiation every branch of the row-program dispatchers starts.

The launchers (rzk_kernels.hip, rzk_slab32_dev.hip, rzk_response_stat_dev.hip) pick a template instantiation from the ring
degree, the planned program's facts and the context's knobs, and report its name (Context.prof_read_kernels).  The other
GPU tests look at a suffix or a family prefix of those names; here a case is (ring and shape, knobs, entry point) -> the
whole list of names of the call, compared for equality with tests/golden/launch_names.json.  The table was recorded with
this module's __main__ on the commit BEFORE the launch layer was folded into rzk_launch.h, so it pins what the dispatch
chose then; re-record it (python tests/test_gpu_launch_names.py > tests/golden/launch_names.json) only with a change that
means to alter the routing.

Batch 3, V = 2, inputs from ring_zk_amd.synth; verdicts are not asserted (the names do not depend on them).  Knobs appear
only where they change the route of some entry point, and a case lists only the entry points they change.

Branches (each `return launch_...` of a dispatcher) and a case that reaches them — "1024/UNIT_IO=1: open_commit" reads
"context 1024-131-UNIT_IO=1, entry point open_commit"; the shape is (1,3,1) unless it is named:
  launch_units, unit_io_kernel
    <9, false> / <9, true>                      512/default: open_commit / open_verify
    <10, false> / <10, true>                    1024/UNIT_IO=1: open_commit / open_verify
    <11, false, PairTeam>                       2048/UNIT_IO=1: open_commit
    <11, false>                                 2048/UNIT_IO=1+PAIR_POLY=0: open_commit
  launch_units, unit_kernel on the teams with the twiddle image (reported under the names of the teams without)
    <10, false, false> / <10, false, true>      1024/default: open_commit / open_verify
    <10, true, false> / <10, true, true>        1024/VEC_ROWS=0: polymul / sum_verify
  launch_units, unit_kernel
    <9, false, false> / <9, false, true>        512/UNIT_IO=0: open_commit / open_verify
    <9, true, false> / <9, true, true>          512/VEC_ROWS=0: polymul / sum_verify
    <10, false, false|true>                     1024/TW_LDS=0: open_commit / open_verify
    <10, true, false|true>                      1024/VEC_ROWS=0+TW_LDS=0: polymul / sum_verify
    <11, false, false|true, PairTeam>           2048/default: open_commit / open_verify
    <11, true, false|true, PairTeam>            2048/VEC_ROWS=0: polymul / sum_verify
    <11, false, false> / <11, true, false>      2048/PAIR_POLY=0: open_commit / 2048/VEC_ROWS=0+PAIR_POLY=0: polymul
  launch_rows, row_kernel
    <9|10, false, WaveTeam, false>              512|1024/default: polymul
    <9|10, true, WaveTeam, false>               512|1024/default: sum_verify
    <11, false|true, PairTeam, false>           2048/default: polymul / sum_verify
    <11, false, WaveTeam, false>                2048/PAIR_POLY=0: polymul
    <9|10, false, WaveTeam, true>               512|1024/SUM_D=1+DKEY=2: sum_commit (rows that read the call's operand images)
    <11, false, PairTeam|WaveTeam, true>        2048/SUM_D=1+DKEY=2 | 2048/SUM_D=1+DKEY=2+PAIR_POLY=0: sum_commit
  launch_shift_rows, shift_row_kernel
    <9|10, false>                               512|1024/default: open_response
    <9|10, false, WaveTeam, false>              512|1024/SHIFT_BYTES=0: open_response
    <11, false, PairTeam>                       2048/default: open_response
  launch_row_blocks, row_block_kernel
    <10>                                        1024-252/BLOCK_MIN_LOGN=10: matvec
    <11, BlockPairTeam> / <11>                  2048-252/default / 2048-252/PAIR_POLY=0: matvec
  launch_response_stat, response_stat_kernel
    <9|10, false>                               512|1024/default: open_response_reject
    <9|10, false, false>                        512|1024/SHIFT_BYTES=0: open_response_reject
  launch_units32
    unit_io_kernel<9, false|true, i32>          512/default: open_commit32 / open_verify32
    unit_io_kernel<10, false|true, i32>         1024/UNIT_IO=1: open_commit32 / open_verify32
    unit_kernel<9, false, false|true, i32>      512/UNIT_IO=0: open_commit32 / open_verify32
    unit_kernel<10, false, false|true, i32>     1024/default (twiddle image), 1024/TW_LDS=0: open_commit32 / open_verify32
  launch_shift_rows32, shift_row_kernel<9|10, false, i32>      512|1024/default: open_response32
  and beside them: row_group_kernel<10, 4> 1024-252/default: matvec; fwd_slots + row_slots 2048-252/BLOCK_MIN_LOGN=12: matvec.
The -1 answers start nothing: N = 64 runs row_kernel_small; the 32-bit calls at N = 64, N = 2048, (2,5,2) and under
SHIFT_BYTES=0 or SHIFT=0 take the convert path (widen_kernel, the 64-bit kernels, narrow_kernel); N = 2048 under
PAIR_POLY=0 keeps its challenge products on the transform kernels.  RZK_UNIT_IO=0 at N >= 1024, RZK_ROW_GROUPS=0 at (1,3,1)
and RZK_BLOCK_MIN_LOGN=12 at N = 1024 change no route and have no case.
"""
import conftest  # noqa: F401  (run as a script: puts the repository root on sys.path)

import json
import os

import numpy as np
import pytest

from ring_zk_amd import synth
from test_gpu_baseline_shapes import make_ctx, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_names.json")
B, V = 3, 2


def make_inputs(ctx, rng):
    N, n, k, l = ctx.N, ctx.n, ctx.k, ctx.l
    sig = ctx.sigma
    U, S, G = synth.uniform, synth.small, synth.gauss
    return dict(
        x=U(rng, (B, l, N)), r=S(rng, (B, k, N)), rp=S(rng, (B, k, N)), y=G(rng, (B, k, N), sig), yp=G(rng, (B, k, N), sig),
        g=U(rng, (B, N)), h=U(rng, (B, N)), d=synth.challenge(rng, (B,), N, ctx.kappa),
        z=G(rng, (B, k, N), sig), zp=G(rng, (B, k, N), sig), t=U(rng, (B, n, N)), tp=U(rng, (B, n, N)),
        c=U(rng, (B, n + l, N)), cp=U(rng, (B, n + l, N)), u=U(rng, (B, l, N)),
        gs=U(rng, (B, V, N)), xs=U(rng, (B, V, l, N)), rs=S(rng, (B, V, k, N)), ys=G(rng, (B, V, k, N), sig),
        zs=G(rng, (B, V, k, N), sig), cs=U(rng, (B, V, n + l, N)), ts=U(rng, (B, V, n, N)),
        coin=rng.integers(0, 2 ** 32, (B,), dtype=np.int64))


def n32(*arrays):
    return [np.ascontiguousarray(a.astype(np.int32)) for a in arrays]


ENTRY_POINTS = {
    "polymul": lambda c, i: c.polymul(i["g"], i["h"]),
    "matvec": lambda c, i: c.matvec(2, i["r"]),
    "open_commit": lambda c, i: c.open_commit(i["x"], i["r"], i["y"]),
    "open_response": lambda c, i: c.open_response(i["y"], i["r"], i["d"]),
    "open_verify": lambda c, i: c.open_verify(i["z"], i["t"], i["c"], i["d"]),
    "open_recover": lambda c, i: c.open_recover(i["z"], i["c"], i["d"]),
    "open_commit32": lambda c, i: c.open_commit32(*n32(i["x"], i["r"], i["y"])),
    "open_response32": lambda c, i: c.open_response32(*n32(i["y"], i["r"], i["d"])),
    "open_verify32": lambda c, i: c.open_verify32(*n32(i["z"], i["t"], i["c"], i["d"])),
    "open_recover32": lambda c, i: c.open_recover32(*n32(i["z"], i["c"], i["d"])),
    "open_response_reject": lambda c, i: c.open_response_reject(i["y"], i["r"], i["d"], i["coin"], 2 ** 32, 1.0),
    "linear_commit": lambda c, i: c.linear_commit(i["g"], i["x"], i["r"], i["rp"], i["y"], i["yp"]),
    "linear_verify": lambda c, i: c.linear_verify(i["z"], i["zp"], i["c"], i["cp"], i["g"], i["t"], i["tp"], i["u"], i["d"]),
    "sum_commit": lambda c, i: c.sum_commit(i["gs"], i["xs"], i["rs"], i["rp"], i["ys"], i["yp"]),
    "sum_verify": lambda c, i: c.sum_verify(i["zs"], i["zp"], i["cs"], i["cp"], i["gs"], i["ts"], i["tp"], i["u"], i["d"]),
}

ALL = list(ENTRY_POINTS)
OPEN32 = ["open_commit32", "open_response32", "open_verify32", "open_recover32"]
KEY_PRODUCTS = ["matvec", "open_commit", "open_verify", "open_recover", "open_commit32", "open_verify32", "open_recover32",
                "linear_commit", "linear_verify", "sum_commit", "sum_verify"]            # programs on the unit kernels
ROTATIONS = ["open_response", "open_verify", "open_recover"] + OPEN32 + ["open_response_reject", "linear_verify", "sum_verify"]
VEC = ["polymul", "linear_commit", "linear_verify", "sum_commit", "sum_verify"]          # vector x vector products
GROUPED = [e for e in KEY_PRODUCTS if e != "linear_verify"]                                # (2,5,2): row groups / blocks
S131, S252 = (1, 3, 1), (2, 5, 2)
IMAGES = {"RZK_SUM_D": 1, "RZK_DKEY": 2}   # V = 2 is below the cost model's threshold for the operand images: force them

# (N, (n, k, l), knobs, entry points)
CASES = [
    (64, S131, {}, ["polymul", "open_verify", "open_verify32", "open_response_reject", "sum_commit"]),
    (512, S131, {}, ALL),
    (512, S131, {"RZK_UNIT_IO": 0}, KEY_PRODUCTS),
    (512, S131, {"RZK_SHIFT_BYTES": 0}, ["open_response", "open_response_reject"] + OPEN32),
    (512, S131, {"RZK_SHIFT": 0}, ROTATIONS),
    (512, S131, {"RZK_VEC_ROWS": 0}, VEC),
    (512, S131, IMAGES, ["sum_commit", "sum_verify"]),
    (1024, S131, {}, ALL),
    (1024, S131, {"RZK_UNIT_IO": 1}, KEY_PRODUCTS),
    (1024, S131, {"RZK_TW_LDS": 0}, ["open_commit", "open_verify", "open_commit32", "open_verify32"]),   # (same names: the image does not show)
    (1024, S131, {"RZK_SHIFT_BYTES": 0}, ["open_response", "open_response_reject"] + OPEN32),
    (1024, S131, {"RZK_SHIFT": 0}, ROTATIONS),
    (1024, S131, {"RZK_VEC_ROWS": 0}, VEC),
    (1024, S131, {"RZK_VEC_ROWS": 0, "RZK_TW_LDS": 0}, ["polymul", "sum_verify"]),
    (1024, S131, IMAGES, ["sum_commit", "sum_verify"]),
    (2048, S131, {}, ALL),
    (2048, S131, {"RZK_UNIT_IO": 1}, ["matvec", "open_commit", "open_commit32", "linear_commit", "sum_commit", "sum_verify"]),
    (2048, S131, {"RZK_SHIFT": 0}, [e for e in ROTATIONS if e != "open_commit32"]),
    (2048, S131, {"RZK_PAIR_POLY": 0}, ALL),
    (2048, S131, {"RZK_VEC_ROWS": 0}, VEC),
    (2048, S131, {"RZK_UNIT_IO": 1, "RZK_PAIR_POLY": 0}, ["matvec", "open_commit"]),
    (2048, S131, {"RZK_VEC_ROWS": 0, "RZK_PAIR_POLY": 0}, ["polymul", "sum_commit"]),
    (2048, S131, IMAGES, ["sum_commit", "sum_verify"]),
    (2048, S131, dict(IMAGES, RZK_PAIR_POLY=0), ["sum_commit", "sum_verify"]),
    (1024, S252, {}, ALL),
    (1024, S252, {"RZK_SHIFT_BYTES": 0}, ["open_response", "open_verify", "open_recover", "open_response_reject", "sum_verify"]),
    (1024, S252, {"RZK_SHIFT": 0}, [e for e in ROTATIONS if e != "open_commit32"]),
    (1024, S252, {"RZK_ROW_GROUPS": 0}, GROUPED),
    (1024, S252, {"RZK_BLOCK_MIN_LOGN": 10}, GROUPED),
    (1024, S252, {"RZK_VEC_ROWS": 0}, ["linear_verify"]),
    # row_block_kernel at N = 2048 needs rows that share operands: the one shape beyond the list above
    (2048, S252, {}, ["matvec", "open_commit", "open_verify"]),
    (2048, S252, {"RZK_PAIR_POLY": 0}, ["matvec", "open_commit", "open_verify"]),
    (2048, S252, {"RZK_BLOCK_MIN_LOGN": 12}, ["matvec", "open_commit", "open_verify"]),
]


def case_id(N, shape, knobs):
    return f"{N}-{''.join(map(str, shape))}-" + ("+".join(f"{k[4:]}={v}" for k, v in knobs.items()) or "default")


def launched(N, shape, knobs, entries):
    """{entry point: [kernel names of the call]} in a fresh context under the knobs."""
    ctx = make_ctx(N, *shape, env=knobs)
    rng = np.random.default_rng(71000 + N + shape[0])
    ctx.load_key(synth.key(rng, N, *shape))
    inputs = make_inputs(ctx, rng)
    out = {}
    ctx.prof_enable(True)
    try:
        for name in entries:
            ctx.prof_reset()
            ENTRY_POINTS[name](ctx, inputs)
            out[name] = [nm for nm, _ in ctx.prof_read_kernels()]
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("N,shape,knobs,entries", CASES, ids=[case_id(*c[:3]) for c in CASES])
def test_launched_names(torch_mod, N, shape, knobs, entries):
    with open(GOLDEN) as fh:
        want = json.load(fh)[case_id(N, shape, knobs)]
    assert sorted(want) == sorted(entries), "the table and CASES list different entry points"
    assert launched(N, shape, knobs, entries) == want


if __name__ == "__main__":
    print(json.dumps({case_id(*c[:3]): launched(*c) for c in CASES}, indent=1))
