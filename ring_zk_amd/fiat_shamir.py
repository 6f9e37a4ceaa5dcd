"""Non-interactive (Fiat-Shamir) form of the three proofs (include/rzk.h "Fiat-Shamir").

The reference's verifier draws the challenge d itself (open.rs:138-145, linear.rs:182-189, sum.rs:226-233), so it has
to be online.  Here d is the hash of the prover's commitment message under the FS1 transcript (SHAKE256 on the GPU,
rzk_fs_challenge_batch[_dev]): a proof is (commitment message, response), and anyone holding the key recomputes d.

  * `challenge` / `key_digest`: the transcript hash itself;
  * `open_prove` / `open_verify`, `linear_*`, `sum_*`: commit -> challenge -> response, and challenge -> verify; with
    torch CUDA tensors nothing leaves the device between the phases;
  * `verify_open_wire`: the same verdict from serialized OpenProofCommitment / OpenProofResponse messages;
  * `open_verify_packed`, `linear_verify_packed`, `sum_verify_packed`: the same verdicts from fixed-width packed records
    (`packed.py`);
  * `challenge32`, `open_prove32`, `open_verify32`, `open_short32`, `open_verify_short32`, `open_verify_packed32`,
    `open_verify_short_packed32`: the Open proof on int32 slabs;
  * `open_short` / `open_verify_short` / `open_verify_short_packed`: the signature form of an Open proof, (c, d, z): the
    verifier recomputes t from the verification equation and accepts iff the transcript of (c, t) gives d again;
  * `linear_short` / `linear_verify_short[_packed]`, `sum_short` / `sum_verify_short[_packed]`: the same for Linear and
    Sum proofs, which drop t, t', u.  A short proof and a full proof are one proof in two encodings;
  * `multipliers`: the public multipliers g / g_i of Linear and Sum proofs derived from seeds;
  * `open_prove_sampled`, `linear_prove_sampled`, `sum_prove_sampled`: the provers with r and y drawn on the device by a
    `backend.KeyedSampler` (ChaCha20) instead of supplied by the caller;
  * `open_prove_zk`, `linear_prove_zk`, `sum_prove_zk`: the sampled provers with the scheme's rejection step
    (Context.reject): a response is released only once it passed, with a fresh y per attempt;
  * `open_prove_sampled32`, `open_prove_zk32`: the sampled and the zero-knowledge Open prover on int32 slabs with a
    `backend.KeyedSampler32`;
  * `linear_prove32`, `linear_verify32`, `linear_short32`, `linear_verify_short32`, `linear_verify_packed32`,
    `linear_verify_short_packed32`, `linear_prove_sampled32`, `linear_prove_zk32`: the Linear proof on int32 slabs
    (DESIGN.md §25);
  * `open_prove_zk_native`: open_prove_zk / open_prove_zk32 with the rejection loop inside the library, one call
    (rzk_open_prove_zk[32]_batch_dev);
  * `linear_prove_zk_native`, `sum_prove_zk_native`: the same for linear_prove_zk / sum_prove_zk
    (rzk_linear_prove_zk_batch_dev, rzk_sum_prove_zk_batch_dev).

`aux` (32 bytes, default zeros) binds the proofs of a call to a session or statement; prover and verifier must agree.
Like the rest of the package every function takes numpy arrays (host entry points) or torch CUDA tensors (device entry
points on torch's current stream).
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple
from typing import Optional

import numpy as np

from . import packed, wire
from ._lib import (KEY_A1, MSG_LINEAR_COMMITMENT, MSG_LINEAR_RESPONSE, MSG_LINEAR_SHORT, MSG_OPEN_COMMITMENT, MSG_OPEN_RESPONSE,
                   MSG_OPEN_SHORT, MSG_SUM_COMMITMENT, MSG_SUM_RESPONSE, MSG_SUM_SHORT)

KINDS = (MSG_OPEN_COMMITMENT, MSG_LINEAR_COMMITMENT, MSG_SUM_COMMITMENT)


def key_digest(ctx) -> bytes:
    """FS1 digest of the loaded key and the context's parameters (rzk_fs_key_digest)."""
    out = (C.c_uint8 * 32)()
    ctx._check(ctx._L.rzk_fs_key_digest(ctx._h, out))
    return bytes(out)


def _aux(aux) -> Optional[C.Array]:
    if aux is None:
        return None
    aux = bytes(aux)
    if len(aux) != 32:
        raise ValueError("aux must be 32 bytes")
    return (C.c_uint8 * 32).from_buffer_copy(aux)


def challenge(ctx, kind: int, *slabs, V: Optional[int] = None, aux=None):
    """Field slabs of B commitment messages (declaration order, as for wire.encode_batch) -> (d, digest, ok).

    d [B][N] int64: the challenges; digest [B][32] uint8: the transcript digests; ok [B] uint8: 0 where a coefficient
    of the proof is not a centred residue mod q (its d and digest are then unspecified)."""
    return _challenge(ctx, kind, slabs, V, aux, np.int64)


def challenge32(ctx, kind: int, *slabs, V: Optional[int] = None, aux=None):
    """challenge for int32 slabs (numpy int32 arrays or torch int32 CUDA tensors, rzk_fs_challenge32_batch[_dev]): the
    same digest and ok as challenge on the widened slabs, and the same d as int32.  The transcript hashes a coefficient
    as its int32, so nothing is converted."""
    return _challenge(ctx, kind, slabs, V, aux, np.int32)


def _challenge(ctx, kind, slabs, V, aux, dt):
    w32 = dt is np.int32
    if kind not in KINDS:
        raise ValueError("challenge: kind must be MSG_OPEN_COMMITMENT, MSG_LINEAR_COMMITMENT or MSG_SUM_COMMITMENT")
    shapes = wire.field_shapes(ctx, kind, V)
    if len(slabs) != len(shapes):
        raise ValueError(f"{len(shapes)} field slabs expected, got {len(slabs)}")
    B = int(slabs[0].shape[0])
    dev = wire._is_torch(slabs[0])
    for (name, sh), s in zip(shapes, slabs):
        if wire._is_torch(s) != dev or tuple(s.shape) != (B,) + sh:
            raise ValueError(f"field {name}: expected {(B,) + sh}, got {tuple(s.shape)}")
    if dev:
        import torch

        slabs = [s.contiguous() for s in slabs]
        if any(s.dtype != (torch.int32 if w32 else torch.int64) or not s.is_cuda for s in slabs):
            raise ValueError("device slabs must be %s CUDA tensors" % ("int32" if w32 else "int64"))
        d = torch.empty((B, ctx.N), dtype=torch.int32 if w32 else torch.int64, device=slabs[0].device)
        digest = torch.empty((B, 32), dtype=torch.uint8, device=slabs[0].device)
        ok = torch.empty(B, dtype=torch.uint8, device=slabs[0].device)
        ctx._bind_torch_stream()
        fn = ctx._L.rzk_fs_challenge32_batch_dev if w32 else ctx._L.rzk_fs_challenge_batch_dev
    else:
        if w32 and any(s.dtype != np.int32 for s in slabs):
            raise ValueError("host slabs must be int32 numpy arrays")
        slabs = [np.ascontiguousarray(s, dtype=dt) for s in slabs]
        d = np.empty((B, ctx.N), dtype=dt)
        digest = np.empty((B, 32), dtype=np.uint8)
        ok = np.empty(B, dtype=np.uint8)
        fn = ctx._L.rzk_fs_challenge32_batch if w32 else ctx._L.rzk_fs_challenge_batch
    fields = (C.c_void_p * len(slabs))(*[wire._ptr(s).value for s in slabs])
    ctx._check(fn(ctx._h, kind, V or 0, fields, _aux(aux), wire._ptr(d), wire._ptr(digest), wire._ptr(ok), B))
    return d, digest, ok


def multipliers(ctx, seeds, V: Optional[int] = None, domain: int = 1):
    """Public multipliers of Linear / Sum proofs as uniform ring elements derived from seeds [B, 32] uint8 (statement
    digests, say) by the XP1 expansion (Context.xof_uniform): g [B, N] for V = None, the shape
    linear_prove takes, or gs [B, V, N] for sum_prove.  Prover and verifier call this with the same seeds and domain."""
    if V is None:
        return ctx.xof_uniform(seeds, 1, domain).reshape(-1, ctx.N)
    if V < 1:
        raise ValueError("multipliers: V must be at least 1")
    return ctx.xof_uniform(seeds, V, domain)


def _same_challenge(ctx, d2, d):
    """d2 (recomputed, canonical) == d per proof; d is foreign, so its canonical copy is compared: a non-canonical d has
    already cleared the verdict of the recompute step and must not fail the call here."""
    return ctx.eq(d2.reshape(-1, 1, ctx.N), ctx.canonicalize(d).reshape(-1, 1, ctx.N))


def _flag(cond):
    """boolean array / tensor -> uint8 flags"""
    if wire._is_torch(cond):
        import torch

        return cond.to(torch.uint8)
    return cond.astype(np.uint8)


# ---- OpenProof (src/prove/open.rs) -------------------------------------------------------------------------------------
# The Open functions exist for int64 and for int32 slabs and are written once, over the record of the
# operations they use at one width.  On int32 slabs every slab is int32 (numpy or torch CUDA): no 64-bit slab and no convert
# launch appears between record and verdict at N = 512 and 1024, n = 1.
def _method(name):
    return lambda ctx, *args: getattr(ctx, name)(*args)


def _same_challenge32(ctx, d2, d):
    """_same_challenge on int32 slabs, word for word (Context.eq32): a canonical d is its own canonical copy, and a
    non-canonical one has already cleared the verdict of open_recover32, so the canonicalize launch of the 64-bit form has
    nothing to do here."""
    return ctx.eq32(d2.reshape(-1, 1, ctx.N), d.reshape(-1, 1, ctx.N))


def draw_coins32(sampler, lead):
    """draw_coins from a sampler that returns int32 tensors: the same two draws and coefficients; the two [*lead] vectors
    are converted to int64 before (a + half) R0 + (b + half) is formed (the product overflows int32).  That is a gather of
    one value per proof, not a pass over a slab.  The coin is int64, as Context.open_response_reject32 takes it."""
    import torch

    half = (COIN_R0 - 1) // 2
    a = sampler.uniform(half, tuple(lead))[..., 0].to(torch.int64)
    b = sampler.uniform(half, tuple(lead))[..., 1].to(torch.int64)
    return ((a + half) * COIN_R0 + (b + half)).contiguous(), COIN_R0 * COIN_R0


# suffix: of the public names ("" on int64 slabs, "32" on int32 slabs); decode: packed records -> slabs; same_challenge: the
# short verifier's final compare; coins: the coin draw of a zero-knowledge round; the others: the Context methods
_OpenOps = namedtuple("_OpenOps", "suffix challenge decode same_challenge coins commit matvec response response_reject verify recover")


def _open_ops(suffix, challenge_, decode, same_challenge, coins):
    names = ("open_commit", "matvec", "open_response", "open_response_reject", "open_verify", "open_recover")
    return _OpenOps(suffix, challenge_, decode, same_challenge, coins, *[_method(m + suffix) for m in names])


def _open_prove(w, ctx, x, r, y, aux):
    c, t, ok = w.commit(ctx, x, r, y)
    d, _, okf = w.challenge(ctx, MSG_OPEN_COMMITMENT, c, t, aux=aux)
    z = w.response(ctx, y, r, d)
    return c, t, z, ok & okf


def _open_verify(w, ctx, c, t, z, aux):
    d, _, okf = w.challenge(ctx, MSG_OPEN_COMMITMENT, c, t, aux=aux)
    return w.verify(ctx, z, t, c, d) & okf


def _open_verify_packed(w, ctx, commitment_records, response_records, aux):
    c, t, ok1 = w.decode(ctx, MSG_OPEN_COMMITMENT, commitment_records)
    (z, ok2) = w.decode(ctx, MSG_OPEN_RESPONSE, response_records)
    return _open_verify(w, ctx, c, t, z, aux) & ok1 & ok2


def _open_short(w, ctx, c, t, z, aux):
    d, _, _ = w.challenge(ctx, MSG_OPEN_COMMITMENT, c, t, aux=aux)
    return d


def _open_verify_short(w, ctx, c, d, z, aux):
    t, acc = w.recover(ctx, z, c, d)
    d2, _, okf = w.challenge(ctx, MSG_OPEN_COMMITMENT, c, t, aux=aux)   # the caller's c: a non-canonical one clears okf
    return acc & okf & w.same_challenge(ctx, d2, d)


def _open_verify_short_packed(w, ctx, records, aux):
    c, d, z, ok = w.decode(ctx, MSG_OPEN_SHORT, records)
    return _open_verify_short(w, ctx, c, d, z, aux) & ok


def open_prove(ctx, x, r, y, aux=None):
    """commit (open.rs:80-103), d = challenge(c, t), response (open.rs:107-117): (c, t, z, ok); ok[b] = 0 where r fails
    the commit constraint (the caller resamples) or an output is not canonical."""
    return _open_prove(_OPEN64, ctx, x, r, y, aux)


def open_verify(ctx, c, t, z, aux=None):
    """OpenProofVerifier::verify (open.rs:162-174) with the recomputed challenge."""
    return _open_verify(_OPEN64, ctx, c, t, z, aux)


def verify_open_wire(ctx, commitment_msgs, response_msgs, aux=None, coef_bytes: int = 8):
    """open_verify from serialized OpenProofCommitment and OpenProofResponse messages (lists of bytes or
    (data, offsets)): decode, recompute d, verify; a message that does not decode rejects its proof."""
    c, t, ok1 = wire.decode_batch(ctx, MSG_OPEN_COMMITMENT, *wire._msgs(commitment_msgs), coef_bytes=coef_bytes)
    (z, ok2) = wire.decode_batch(ctx, MSG_OPEN_RESPONSE, *wire._msgs(response_msgs), coef_bytes=coef_bytes)
    return open_verify(ctx, c, t, z, aux=aux) & ok1 & ok2


def open_verify_packed(ctx, commitment_records, response_records, aux=None):
    """open_verify from packed MSG_OPEN_COMMITMENT and MSG_OPEN_RESPONSE records (packed.encode_batch): decode,
    recompute d, verify; a record that does not decode rejects its own proof."""
    return _open_verify_packed(_OPEN64, ctx, commitment_records, response_records, aux)


def open_short(ctx, c, t, z, aux=None):
    """The short form of the Open proof (c, t, z): (c, d, z) with d = challenge(c, t), as a Fiat-Shamir signature sends
    it.  Returns d; t is dropped, the verifier recomputes it (open_verify_short).  z is left as it is."""
    return _open_short(_OPEN64, ctx, c, t, z, aux)


def open_verify_short(ctx, c, d, z, aux=None):
    """Verifier of the short form: t' = a1.z - c1 (.) d is the only t that satisfies the verification equation
    (open.rs:171-173) for (c, d, z), computed by Context.open_recover together with the norm rule on z; accept iff the
    transcript of (c, t') gives d again, z passes the norm rule and neither step met a non-canonical coefficient
    (foreign data rejects its proof instead of failing the call).  An honest proof has t' = t."""
    return _open_verify_short(_OPEN64, ctx, c, d, z, aux)


def open_verify_short_packed(ctx, records, aux=None):
    """open_verify_short from packed MSG_OPEN_SHORT records; a record that does not decode rejects its own proof."""
    return _open_verify_short_packed(_OPEN64, ctx, records, aux)


def open_prove32(ctx, x, r, y, aux=None):
    """open_prove on int32 slabs: (c, t, z, ok), each the int32 of open_prove's."""
    return _open_prove(_OPEN32, ctx, x, r, y, aux)


def open_verify32(ctx, c, t, z, aux=None):
    """open_verify on int32 slabs."""
    return _open_verify(_OPEN32, ctx, c, t, z, aux)


def open_verify_packed32(ctx, commitment_records, response_records, aux=None):
    """open_verify_packed through int32 slabs: the records are those of packed.encode_batch or encode_batch32."""
    return _open_verify_packed(_OPEN32, ctx, commitment_records, response_records, aux)


def open_short32(ctx, c, t, z, aux=None):
    """open_short on int32 slabs: d = challenge32(c, t) as int32."""
    return _open_short(_OPEN32, ctx, c, t, z, aux)


def open_verify_short32(ctx, c, d, z, aux=None):
    """open_verify_short on int32 slabs.  The recomputed challenge is compared with the caller's d word for word
    (_same_challenge32)."""
    return _open_verify_short(_OPEN32, ctx, c, d, z, aux)


def open_verify_short_packed32(ctx, records, aux=None):
    """open_verify_short_packed through int32 slabs: packed MSG_OPEN_SHORT records -> verdicts."""
    return _open_verify_short_packed(_OPEN32, ctx, records, aux)


# ---- LinearProof (src/prove/linear.rs) ---------------------------------------------------------------------------------
# Written once over the record of operations at one width, as the Open functions: on int32 slabs every slab is
# int32, and at (1, k, 1), N = 512 and 1024 no 64-bit slab and no convert launch appears between record and verdict.
_LinearOps = namedtuple("_LinearOps", "suffix challenge decode same_challenge coins commit response response_reject verify recover")


def _linear_ops(suffix, challenge_, decode, same_challenge, coins):
    names = ("linear_commit", "linear_response", "linear_response_reject", "linear_verify", "linear_recover")
    return _LinearOps(suffix, challenge_, decode, same_challenge, coins, *[_method(m + suffix) for m in names])


def _linear_prove(w, ctx, g, x, r, rp, y, yp, aux):
    c, cp, t, tp, u, ok = w.commit(ctx, g, x, r, rp, y, yp)
    d, _, okf = w.challenge(ctx, MSG_LINEAR_COMMITMENT, c, cp, g, t, tp, u, aux=aux)
    z, zp = w.response(ctx, y, yp, r, rp, d)
    return c, cp, t, tp, u, z, zp, _flag(ok == 3) & okf


def _linear_verify(w, ctx, c, cp, g, t, tp, u, z, zp, aux):
    d, _, okf = w.challenge(ctx, MSG_LINEAR_COMMITMENT, c, cp, g, t, tp, u, aux=aux)
    return w.verify(ctx, z, zp, c, cp, g, t, tp, u, d) & okf


def _linear_verify_packed(w, ctx, commitment_records, response_records, aux):
    c, cp, g, t, tp, u, ok1 = w.decode(ctx, MSG_LINEAR_COMMITMENT, commitment_records)
    z, zp, ok2 = w.decode(ctx, MSG_LINEAR_RESPONSE, response_records)
    return _linear_verify(w, ctx, c, cp, g, t, tp, u, z, zp, aux) & ok1 & ok2


def _linear_short(w, ctx, c, cp, g, t, tp, u, z, zp, aux):
    d, _, _ = w.challenge(ctx, MSG_LINEAR_COMMITMENT, c, cp, g, t, tp, u, aux=aux)
    return d


def _linear_verify_short(w, ctx, c, cp, g, d, z, zp, aux):
    t, tp, u, acc = w.recover(ctx, z, zp, c, cp, g, d)
    d2, _, okf = w.challenge(ctx, MSG_LINEAR_COMMITMENT, c, cp, g, t, tp, u, aux=aux)
    return acc & okf & w.same_challenge(ctx, d2, d)


def _linear_verify_short_packed(w, ctx, records, aux):
    c, cp, g, d, z, zp, ok = w.decode(ctx, MSG_LINEAR_SHORT, records)
    return _linear_verify_short(w, ctx, c, cp, g, d, z, zp, aux) & ok


def linear_prove(ctx, g, x, r, rp, y, yp, aux=None):
    """(c, cp, t, tp, u, z, zp, ok); ok[b] = 1 iff r and rp both pass the commit constraint."""
    return _linear_prove(_LINEAR64, ctx, g, x, r, rp, y, yp, aux)


def linear_verify(ctx, c, cp, g, t, tp, u, z, zp, aux=None):
    """LinearProofVerifier::verify (linear.rs:213-250) with the recomputed challenge."""
    return _linear_verify(_LINEAR64, ctx, c, cp, g, t, tp, u, z, zp, aux)


def linear_verify_packed(ctx, commitment_records, response_records, aux=None):
    """linear_verify from packed MSG_LINEAR_COMMITMENT and MSG_LINEAR_RESPONSE records."""
    return _linear_verify_packed(_LINEAR64, ctx, commitment_records, response_records, aux)


def linear_short(ctx, c, cp, g, t, tp, u, z, zp, aux=None):
    """The short form of the Linear proof: (c, cp, g, d, z, zp) with d = challenge(c, cp, g, t, tp, u).  Returns d; the
    verifier recomputes t, tp, u (linear_verify_short)."""
    return _linear_short(_LINEAR64, ctx, c, cp, g, t, tp, u, z, zp, aux)


def linear_verify_short(ctx, c, cp, g, d, z, zp, aux=None):
    """Verifier of the short Linear proof: Context.linear_recover gives the only (t', tp', u') that satisfy
    linear.rs:224-249 for the rest of the proof, with the norm rule on z and zp; accept iff the transcript of the full
    commitment message with them gives d again."""
    return _linear_verify_short(_LINEAR64, ctx, c, cp, g, d, z, zp, aux)


def linear_verify_short_packed(ctx, records, aux=None):
    """linear_verify_short from packed MSG_LINEAR_SHORT records; a record that does not decode rejects its own proof."""
    return _linear_verify_short_packed(_LINEAR64, ctx, records, aux)


def linear_prove32(ctx, g, x, r, rp, y, yp, aux=None):
    """linear_prove on int32 slabs: every output slab the int32 of linear_prove's, ok the same."""
    return _linear_prove(_LINEAR32, ctx, g, x, r, rp, y, yp, aux)


def linear_verify32(ctx, c, cp, g, t, tp, u, z, zp, aux=None):
    """linear_verify on int32 slabs.  The transcript is the 64-bit one: a proof made in either width verifies in the other
    after narrow / widen."""
    return _linear_verify(_LINEAR32, ctx, c, cp, g, t, tp, u, z, zp, aux)


def linear_verify_packed32(ctx, commitment_records, response_records, aux=None):
    """linear_verify_packed through int32 slabs: the records are those of packed.encode_batch or encode_batch32."""
    return _linear_verify_packed(_LINEAR32, ctx, commitment_records, response_records, aux)


def linear_short32(ctx, c, cp, g, t, tp, u, z, zp, aux=None):
    """linear_short on int32 slabs: d as int32."""
    return _linear_short(_LINEAR32, ctx, c, cp, g, t, tp, u, z, zp, aux)


def linear_verify_short32(ctx, c, cp, g, d, z, zp, aux=None):
    """linear_verify_short on int32 slabs; the recomputed challenge is compared word for word (_same_challenge32)."""
    return _linear_verify_short(_LINEAR32, ctx, c, cp, g, d, z, zp, aux)


def linear_verify_short_packed32(ctx, records, aux=None):
    """linear_verify_short_packed through int32 slabs: packed MSG_LINEAR_SHORT records -> verdicts."""
    return _linear_verify_short_packed(_LINEAR32, ctx, records, aux)


# ---- SumProof (src/prove/sum.rs) ---------------------------------------------------------------------------------------
def sum_prove(ctx, gs, xs, rs, rp, ys, yp, aux=None):
    """(cs, cp, ts, tp, u, zs, zp, ok) for V = gs.shape[-2] summands per proof."""
    V = int(gs.shape[-2])
    cs, cp, ts, tp, u, ok = ctx.sum_commit(gs, xs, rs, rp, ys, yp)
    d, _, okf = challenge(ctx, MSG_SUM_COMMITMENT, cp, cs, gs, tp, ts, u, V=V, aux=aux)
    zs, zp = ctx.sum_response(ys, yp, rs, rp, d)
    return cs, cp, ts, tp, u, zs, zp, ok & okf


def sum_verify(ctx, cs, cp, gs, ts, tp, u, zs, zp, aux=None):
    """SumProofVerifier::verify (sum.rs:257-320) with the recomputed challenge."""
    V = int(gs.shape[-2])
    d, _, okf = challenge(ctx, MSG_SUM_COMMITMENT, cp, cs, gs, tp, ts, u, V=V, aux=aux)
    return ctx.sum_verify(zs, zp, cs, cp, gs, ts, tp, u, d) & okf


def sum_verify_packed(ctx, commitment_records, response_records, V: int, aux=None):
    """sum_verify from packed MSG_SUM_COMMITMENT and MSG_SUM_RESPONSE records of V summands."""
    cp, cs, gs, tp, ts, u, ok1 = packed.decode_batch(ctx, MSG_SUM_COMMITMENT, commitment_records, V=V)
    zp, zs, ok2 = packed.decode_batch(ctx, MSG_SUM_RESPONSE, response_records, V=V)
    return sum_verify(ctx, cs, cp, gs, ts, tp, u, zs, zp, aux=aux) & ok1 & ok2


def sum_short(ctx, cs, cp, gs, ts, tp, u, zs, zp, aux=None):
    """The short form of the Sum proof: (cp, cs, gs, d, zp, zs) with d = challenge(cp, cs, gs, tp, ts, u).  Returns d."""
    V = int(gs.shape[-2])
    d, _, _ = challenge(ctx, MSG_SUM_COMMITMENT, cp, cs, gs, tp, ts, u, V=V, aux=aux)
    return d


def sum_verify_short(ctx, cs, cp, gs, d, zs, zp, aux=None):
    """Verifier of the short Sum proof: Context.sum_recover gives the only (ts', tp', u') that satisfy sum.rs:277-319,
    with the norm rule on every z_i and zp; accept iff the transcript of the full commitment message gives d again."""
    V = int(gs.shape[-2])
    ts, tp, u, acc = ctx.sum_recover(zs, zp, cs, cp, gs, d)
    d2, _, okf = challenge(ctx, MSG_SUM_COMMITMENT, cp, cs, gs, tp, ts, u, V=V, aux=aux)
    return acc & okf & _same_challenge(ctx, d2, d)


def sum_verify_short_packed(ctx, records, V: int, aux=None):
    """sum_verify_short from packed MSG_SUM_SHORT records of V summands."""
    cp, cs, gs, d, zp, zs, ok = packed.decode_batch(ctx, MSG_SUM_SHORT, records, V=V)
    return sum_verify_short(ctx, cs, cp, gs, d, zs, zp, aux=aux) & ok


# ---- provers that draw their own randomness (backend.KeyedSampler: ChaCha20 on the device) ---------------
# r-type vectors are uniform in [-b, b] (commit.rs:101), y-type vectors N(0, sigma) (open.rs:88-91).  x (and g) must be
# torch CUDA tensors: the draws live on the device.  ok is passed through as from *_prove (0: r failed the commit
# constraint, the caller draws again); there is no resampling loop here.
def _lead(x, tail: int):
    if not wire._is_torch(x):
        raise ValueError("the sampled provers take torch CUDA tensors")
    return tuple(x.shape[:-tail])


def _open_prove_sampled(w, ctx, x, sampler, aux):
    lead = _lead(x, 2)
    r = sampler.uniform(ctx.b, lead + (ctx.k,))
    y = sampler.gauss(ctx.sigma, lead + (ctx.k,))
    return _open_prove(w, ctx, x, r, y, aux) + (r,)


def open_prove_sampled(ctx, x, sampler, aux=None):
    """open_prove with r, y from `sampler`: (c, t, z, ok, r)."""
    return _open_prove_sampled(_OPEN64, ctx, x, sampler, aux)


def open_prove_sampled32(ctx, x, sampler, aux=None):
    """open_prove_sampled on int32 slabs, r and y from a KeyedSampler32: (c, t, z, ok, r)."""
    return _open_prove_sampled(_OPEN32, ctx, x, sampler, aux)


def _linear_prove_sampled(w, ctx, g, x, sampler, aux):
    lead = _lead(x, 2)
    r = sampler.uniform(ctx.b, lead + (ctx.k,))
    rp = sampler.uniform(ctx.b, lead + (ctx.k,))
    y = sampler.gauss(ctx.sigma, lead + (ctx.k,))
    yp = sampler.gauss(ctx.sigma, lead + (ctx.k,))
    return _linear_prove(w, ctx, g, x, r, rp, y, yp, aux) + (r, rp)


def linear_prove_sampled(ctx, g, x, sampler, aux=None):
    """linear_prove with r, r', y, y' from `sampler`: (c, cp, t, tp, u, z, zp, ok, r, rp)."""
    return _linear_prove_sampled(_LINEAR64, ctx, g, x, sampler, aux)


def linear_prove_sampled32(ctx, g, x, sampler, aux=None):
    """linear_prove_sampled on int32 slabs, the draws from a KeyedSampler32: (c, cp, t, tp, u, z, zp, ok, r, rp)."""
    return _linear_prove_sampled(_LINEAR32, ctx, g, x, sampler, aux)


def sum_prove_sampled(ctx, gs, xs, sampler, aux=None):
    """sum_prove with rs, r', ys, y' from `sampler`: (cs, cp, ts, tp, u, zs, zp, ok, rs, rp)."""
    lead = _lead(xs, 3)
    V = int(xs.shape[-3])
    rs = sampler.uniform(ctx.b, lead + (V, ctx.k))
    rp = sampler.uniform(ctx.b, lead + (ctx.k,))
    ys = sampler.gauss(ctx.sigma, lead + (V, ctx.k))
    yp = sampler.gauss(ctx.sigma, lead + (ctx.k,))
    return sum_prove(ctx, gs, xs, rs, rp, ys, yp, aux=aux) + (rs, rp)


# ---- zero-knowledge provers: the sampled provers plus the rejection step ------------------------------
# z = y + d r of the provers above is a Gaussian centred at d r: stored proofs under one r average r out.  The scheme
# releases z only with probability min(1, D_sigma(z) / (M D_{dr,sigma}(z))) and starts again with a fresh y otherwise
# (BDLOP Fig. 2); Context.reject is that test, these provers loop over it until every proof of the batch has passed.
COIN_R0 = (1 << 31) - 1


def draw_coins(sampler, lead):
    """(coin, R): one coin per proof, uniform in [0, R), from two uniform(2^30 - 1) draws of one polynomial each:
    a = coefficient 0 of the first, b = coefficient 1 of the second, R0 = 2^31 - 1 values each,
    coin = (a + 2^30 - 1) R0 + (b + 2^30 - 1), R = R0^2 (the largest such square below the 2^62 the entry point allows)."""
    half = (COIN_R0 - 1) // 2
    a = sampler.uniform(half, tuple(lead))[..., 0]
    b = sampler.uniform(half, tuple(lead))[..., 1]
    return ((a + half) * COIN_R0 + (b + half)).contiguous(), COIN_R0 * COIN_R0


def zk_lnm(m: int) -> float:
    """ln M for a proof with m response vectors of k polynomials: sigma = 11 kappa b sqrt(k N) (params.rs:94-98) is
    alpha = 11 for one vector d r, the m vectors together have up to sqrt(m) times its norm: alpha = 11 / sqrt(m)."""
    from .backend import reject_lnm

    return reject_lnm(11.0 / math.sqrt(m))


def _zk_rounds(ctx, sampler, m: int, max_rounds: int, attempt, fresh):
    """attempt(idx, lnM) -> (outputs, ok, accept) proves the whole batch (idx None) or the proofs idx with a fresh y and
    tests the response in the same call (Context.*_response_reject); it draws y and then the coins
    (draw_coins) from the sampler, in that order.  outputs[i] for i in `fresh` depend on y.  Returns (outputs, ok, rounds)."""
    import torch

    if not 1 <= max_rounds <= 255:
        raise ValueError("max_rounds must lie in 1 .. 255")
    lnM = zk_lnm(m)
    outs, ok, acc = attempt(None, lnM)
    outs = list(outs)
    B = int(ok.shape[0])
    live = ok != 0                      # r passed the commit constraint: worth another y
    done = live & (acc != 0)
    rounds = torch.zeros(B, dtype=torch.uint8, device=ok.device)
    for rnd in range(1, max_rounds):
        idx = torch.nonzero(live & ~done).flatten()
        if idx.numel() == 0:
            break
        o2, _, acc = attempt(idx, lnM)
        a = acc != 0
        sel = idx[a]
        for i in fresh:
            outs[i][sel] = o2[i][a]
        rounds[sel] = rnd
        done[sel] = True
    for i in fresh:                     # a rejected attempt never leaves: what is left of round 0 is overwritten
        outs[i][~done] = 0
    return outs, done.to(torch.uint8), rounds


def _batch3(x, tail: int, name: str):
    if not wire._is_torch(x) or x.ndim != tail + 1:
        raise ValueError(f"{name}: the zero-knowledge provers take torch CUDA tensors with one batch dimension")
    return int(x.shape[0])


def _open_prove_zk(w, ctx, x, sampler, aux, max_rounds):
    import torch

    B = _batch3(x, 2, "open_prove_zk" + w.suffix)
    if w is _OPEN32 and x.dtype != torch.int32:
        raise ValueError("open_prove_zk32: x must be an int32 tensor")
    r = sampler.uniform(ctx.b, (B, ctx.k))

    first = {}

    def attempt(idx, lnM):
        xs, rs = (x, r) if idx is None else (x[idx], r[idx])
        nb = int(xs.shape[0])
        y = sampler.gauss(ctx.sigma, (nb, ctx.k))
        coin, R = w.coins(sampler, (nb,))
        if idx is None:
            c, t, ok = w.commit(ctx, xs, rs, y)
            first["c"] = c
        else:               # c = commit(x; r) does not depend on y: a retry computes t = a1.y alone
            c, ok = first["c"][idx], None
            t = w.matvec(ctx, KEY_A1, y)
        d, _, okf = w.challenge(ctx, MSG_OPEN_COMMITMENT, c, t, aux=aux)
        z, acc, _ = w.response_reject(ctx, y, rs, d, coin, R, lnM)
        return (c, t, z), (okf if ok is None else ok & okf), acc

    (c, t, z), ok, rounds = _zk_rounds(ctx, sampler, 1, max_rounds, attempt, fresh=(1, 2))
    return c, t, z, ok, r, rounds


def open_prove_zk(ctx, x, sampler, aux=None, max_rounds: int = 64):
    """open_prove_sampled with the rejection step: (c, t, z, ok, r, rounds).  Round 0 is open_prove_sampled; each later
    round proves the pending proofs again with the same r and a fresh y.  ok[b] = 1 iff r passed the commit constraint
    and the proof was accepted within max_rounds, in round rounds[b]; t and z of the other proofs are zero."""
    return _open_prove_zk(_OPEN64, ctx, x, sampler, aux, max_rounds)


def open_prove_zk32(ctx, x, sampler, aux=None, max_rounds: int = 64):
    """open_prove_zk on int32 slabs: x int32 [B, l, N] (torch CUDA), sampler a KeyedSampler32 /
    ExactKeyedSampler32 -> (c, t, z, ok, r, rounds) with c, t, z, r int32.  The draw order is the same (r; then per round y
    and the two coin draws), so the outputs are bit-identical to narrow() of open_prove_zk's under the same key and nonces;
    ok and rounds are the same."""
    return _open_prove_zk(_OPEN32, ctx, x, sampler, aux, max_rounds)


_OPEN64 = _open_ops("", challenge, packed.decode_batch, _same_challenge, draw_coins)
_OPEN32 = _open_ops("32", challenge32, packed.decode_batch32, _same_challenge32, draw_coins32)
_LINEAR64 = _linear_ops("", challenge, packed.decode_batch, _same_challenge, draw_coins)
_LINEAR32 = _linear_ops("32", challenge32, packed.decode_batch32, _same_challenge32, draw_coins32)


# ---- the same prover with the loop inside the library (include/rzk.h "prover loop") ----------------------
def open_prove_zk_native(ctx, x, sampler, aux=None, max_rounds: int = 64):
    """open_prove_zk (x int64) / open_prove_zk32 (x int32) through Context.open_prove_zk[32]: one library call runs every
    round, and nothing of the loop passes through torch.  Returns the tuple of open_prove_zk, bit for bit, and leaves the
    sampler's counter where open_prove_zk would: the largest number of nonces the call may use (1 + 3 max_rounds) is taken
    up front and the unused ones are given back.  `sampler` is a KeyedSampler of any kind (its GAUSS_KIND and STREAM pick
    the draws); a SeededSampler is a ValueError: Philox has no keyed entry point."""
    import torch

    B = _batch3(x, 2, "open_prove_zk_native")
    if not hasattr(sampler, "take_nonces") or not hasattr(sampler, "GAUSS_KIND"):
        raise ValueError("open_prove_zk_native needs a KeyedSampler: the library draws from the keyed samplers only")
    if not 1 <= max_rounds <= 255:
        raise ValueError("max_rounds must lie in 1 .. 255")
    if x.dtype not in (torch.int64, torch.int32):
        raise ValueError("open_prove_zk_native: x must be an int64 or int32 tensor")
    span = 1 + 3 * max_rounds
    nonce0 = sampler.take_nonces(span)
    ran = 0
    try:
        prove = ctx.open_prove_zk32 if x.dtype == torch.int32 else ctx.open_prove_zk
        c, t, z, ok, r, rounds, ran = prove(x.contiguous(), nonce0, sampler.STREAM, sampler.GAUSS_KIND, aux, max_rounds)
    finally:
        # open_prove_zk draws r and round 0 even for an empty batch; a failed call keeps the nonces it may have drawn under
        used = span if (ran == 0 and B) else 1 + 3 * max(ran, 1)
        sampler.counter -= span - used
    return c, t, z, ok, r, rounds


def _field_prove_zk_native(name, prove, B, sampler, max_rounds):
    """The nonce bookkeeping of linear_prove_zk_native / sum_prove_zk_native around prove(nonce0) -> (..., rounds_run): the
    largest number of nonces the call may use (2 + 4 max_rounds) is taken up front, the unused ones are given back."""
    if not hasattr(sampler, "take_nonces") or not hasattr(sampler, "GAUSS_KIND"):
        raise ValueError(f"{name} needs a KeyedSampler: the library draws from the keyed samplers only")
    if not 1 <= max_rounds <= 255:
        raise ValueError("max_rounds must lie in 1 .. 255")
    span = 2 + 4 * max_rounds
    nonce0 = sampler.take_nonces(span)
    ran = 0
    try:
        out = prove(nonce0)
        ran = out[-1]
    finally:
        # the Python loop draws r, r' and round 0 even for an empty batch; a failed call keeps the nonces it may have drawn under
        used = span if (ran == 0 and B) else 2 + 4 * max(ran, 1)
        sampler.counter -= span - used
    return out[:-1]


def linear_prove_zk_native(ctx, g, x, sampler, aux=None, max_rounds: int = 64):
    """linear_prove_zk through Context.linear_prove_zk: one library call runs every round (rzk_linear_prove_zk_batch_dev,
    DESIGN.md §24).  Returns the tuple of linear_prove_zk, bit for bit, and leaves the sampler's counter where it would.
    `sampler` is a KeyedSampler of any 64-bit kind; a SeededSampler is a ValueError."""
    B = _batch3(x, 2, "linear_prove_zk_native")
    return _field_prove_zk_native(
        "linear_prove_zk_native",
        lambda nonce0: ctx.linear_prove_zk(g.contiguous(), x.contiguous(), nonce0, sampler.STREAM, sampler.GAUSS_KIND, aux, max_rounds),
        B, sampler, max_rounds)


def sum_prove_zk_native(ctx, gs, xs, sampler, aux=None, max_rounds: int = 64):
    """sum_prove_zk through Context.sum_prove_zk (rzk_sum_prove_zk_batch_dev): the tuple of sum_prove_zk, bit
    for bit, and the same sampler counter afterwards."""
    B = _batch3(xs, 3, "sum_prove_zk_native")
    return _field_prove_zk_native(
        "sum_prove_zk_native",
        lambda nonce0: ctx.sum_prove_zk(gs.contiguous(), xs.contiguous(), nonce0, sampler.STREAM, sampler.GAUSS_KIND, aux, max_rounds),
        B, sampler, max_rounds)


def _linear_prove_zk(w, ctx, g, x, sampler, aux, max_rounds):
    B = _batch3(x, 2, "linear_prove_zk" + w.suffix)
    if w is _LINEAR32:
        import torch

        if x.dtype != torch.int32 or g.dtype != torch.int32:
            raise ValueError("linear_prove_zk32: g and x must be int32 tensors")
    r = sampler.uniform(ctx.b, (B, ctx.k))
    rp = sampler.uniform(ctx.b, (B, ctx.k))

    def attempt(idx, lnM):
        gs, xs, rs, rps = (g, x, r, rp) if idx is None else (g[idx], x[idx], r[idx], rp[idx])
        nb = int(xs.shape[0])
        y = sampler.gauss(ctx.sigma, (nb, ctx.k))
        yp = sampler.gauss(ctx.sigma, (nb, ctx.k))
        coin, R = w.coins(sampler, (nb,))
        c, cp, t, tp, u, ok = w.commit(ctx, gs, xs, rs, rps, y, yp)
        d, _, okf = w.challenge(ctx, MSG_LINEAR_COMMITMENT, c, cp, gs, t, tp, u, aux=aux)
        z, zp, acc, _ = w.response_reject(ctx, y, yp, rs, rps, d, coin, R, lnM)
        return (c, cp, t, tp, u, z, zp), _flag(ok == 3) & okf, acc

    outs, ok, rounds = _zk_rounds(ctx, sampler, 2, max_rounds, attempt, fresh=(2, 3, 4, 5, 6))
    return tuple(outs) + (ok, r, rp, rounds)


def linear_prove_zk(ctx, g, x, sampler, aux=None, max_rounds: int = 64):
    """linear_prove_sampled with the rejection step over (z, z'): (c, cp, t, tp, u, z, zp, ok, r, rp, rounds)."""
    return _linear_prove_zk(_LINEAR64, ctx, g, x, sampler, aux, max_rounds)


def linear_prove_zk32(ctx, g, x, sampler, aux=None, max_rounds: int = 64):
    """linear_prove_zk on int32 slabs: g, x int32 (torch CUDA), sampler a KeyedSampler32 / ExactKeyedSampler32.
    The draw order is linear_prove_zk's, so under the same key and nonces every slab is narrow() of its slab, ok and rounds are
    the same, and the sampler's counter ends where the 64-bit loop leaves it."""
    return _linear_prove_zk(_LINEAR32, ctx, g, x, sampler, aux, max_rounds)


def sum_prove_zk(ctx, gs, xs, sampler, aux=None, max_rounds: int = 64):
    """sum_prove_sampled with the rejection step over (zs, z'): (cs, cp, ts, tp, u, zs, zp, ok, rs, rp, rounds).  With
    V summands M = exp(12 sqrt(V+1) / 11 + (V+1) / 242): the acceptance rate 1 / M falls quickly with V."""
    B = _batch3(xs, 3, "sum_prove_zk")
    V = int(xs.shape[-3])
    rs = sampler.uniform(ctx.b, (B, V, ctx.k))
    rp = sampler.uniform(ctx.b, (B, ctx.k))

    def attempt(idx, lnM):
        g_, x_, rs_, rp_ = (gs, xs, rs, rp) if idx is None else (gs[idx], xs[idx], rs[idx], rp[idx])
        nb = int(x_.shape[0])
        ys = sampler.gauss(ctx.sigma, (nb, V, ctx.k))
        yp = sampler.gauss(ctx.sigma, (nb, ctx.k))
        coin, R = draw_coins(sampler, (nb,))
        cs, cp, ts, tp, u, ok = ctx.sum_commit(g_, x_, rs_, rp_, ys, yp)
        d, _, okf = challenge(ctx, MSG_SUM_COMMITMENT, cp, cs, g_, tp, ts, u, V=V, aux=aux)
        zs, zp, acc, _ = ctx.sum_response_reject(ys, yp, rs_, rp_, d, coin, R, lnM)
        return (cs, cp, ts, tp, u, zs, zp), ok & okf, acc

    outs, ok, rounds = _zk_rounds(ctx, sampler, V + 1, max_rounds, attempt, fresh=(2, 3, 4, 5, 6))
    return tuple(outs) + (ok, rs, rp, rounds)
