"""bincode form of the reference's serialized values <-> dense int64 slabs (include/rzk.h "wire format").

The reference derives serde on `Mat` (src/mat.rs:11-14) and on the protocol messages, and round-trips them
with bincode's default options in its own test (src/mat.rs:424-438).

  * `mat_encode` / `mat_decode`: one `Mat` on the host (rzk_wire_mat_*);
  * `decode_batch` / `encode_batch`: whole protocol messages (`MSG_*` kinds), B at a time, on the GPU
    (rzk_wire_{decode,encode}_batch[_dev]); `pack` / `split` convert between a list of `bytes` and the
    `(data, offsets)` form those take;
  * `verify_open` / `verify_linear` / `verify_sum` / `verify_commitment`: decode, verify with the existing batched
    entry point, and reject every proof whose messages do not decode.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import (MSG_CHALLENGE, MSG_COMMITMENT, MSG_LINEAR_COMMITMENT, MSG_OPEN_COMMITMENT,  # noqa: F401
                   MSG_OPEN_RESPONSE, MSG_OPENING, MSG_SUM_COMMITMENT, MSG_SUM_RESPONSE)


def mat_encode(slab: np.ndarray, coef_bytes: int = 8) -> bytes:
    """slab: int64 [rows][cols][N] -> bincode bytes (polynomials trimmed of trailing zeros)."""
    slab = np.ascontiguousarray(slab, dtype=np.int64)
    if slab.ndim != 3:
        raise ValueError("expected a [rows][cols][N] array")
    rows, cols, N = slab.shape
    L = _lib.lib()
    size = L.rzk_wire_mat_size(C.c_void_p(slab.ctypes.data), rows, cols, N, coef_bytes)
    if size == 0:
        raise ValueError("coef_bytes must be 4 or 8")
    out = np.empty(size, dtype=np.uint8)
    written = C.c_size_t(0)
    rc = L.rzk_wire_mat_encode(C.c_void_p(slab.ctypes.data), rows, cols, N, coef_bytes, C.c_void_p(out.ctypes.data),
                               size, C.byref(written))
    if rc != _lib.RZK_OK:
        raise ValueError("a coefficient does not fit the requested width")
    return out[:written.value].tobytes()


def mat_decode(data: bytes, N: int, coef_bytes: int = 8, q: int = 0) -> Tuple[np.ndarray, int]:
    """bincode bytes -> (int64 [rows][cols][N] slab, bytes consumed).  Raises ValueError on malformed input and,
    with q > 0 (a message over ZqI64<q>), on any coefficient outside the centred range mod q."""
    buf = np.frombuffer(data, dtype=np.uint8)
    L = _lib.lib()
    rows, cols, used = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    ptr = C.c_void_p(buf.ctypes.data) if buf.size else C.c_void_p(0)
    rc = L.rzk_wire_mat_decode(ptr, buf.size, N, coef_bytes, q, C.byref(rows), C.byref(cols), None, 0, C.byref(used))
    if rc != _lib.RZK_OK:
        raise ValueError("malformed Mat encoding")
    slab = np.empty((rows.value, cols.value, N), dtype=np.int64)
    rc = L.rzk_wire_mat_decode(ptr, buf.size, N, coef_bytes, q, C.byref(rows), C.byref(cols),
                               C.c_void_p(slab.ctypes.data), rows.value * cols.value, C.byref(used))
    if rc != _lib.RZK_OK:
        raise ValueError("malformed Mat encoding")
    return slab, used.value


# ---- batched codec of the protocol messages (GPU) --------------------------------------------------------------------
_SUM_KINDS = (MSG_SUM_COMMITMENT, MSG_SUM_RESPONSE)


def field_shapes(ctx, kind: int, V: Optional[int] = None) -> List[Tuple[str, tuple]]:
    """[(field name, slab shape of one message)] of a message kind, fields in declaration order (include/rzk.h)."""
    N, n, k, l = ctx.N, ctx.n, ctx.k, ctx.l
    if kind in _SUM_KINDS and not V:
        raise ValueError("the Sum message kinds need V >= 1")
    return {
        MSG_COMMITMENT: [("c", (n + l, N))],
        MSG_OPENING: [("x", (l, N)), ("r", (k, N)), ("f", (N,))],
        MSG_CHALLENGE: [("d", (N,))],
        MSG_OPEN_COMMITMENT: [("c", (n + l, N)), ("t", (n, N))],
        MSG_OPEN_RESPONSE: [("z", (k, N))],
        MSG_LINEAR_COMMITMENT: [("c", (n + l, N)), ("cp", (n + l, N)), ("g", (N,)), ("t", (n, N)), ("tp", (n, N)),
                                ("u", (l, N))],
        MSG_SUM_COMMITMENT: [("cp", (n + l, N)), ("cs", (V, n + l, N)), ("gs", (V, N)), ("tp", (n, N)),
                             ("ts", (V, n, N)), ("u", (l, N))],
        MSG_SUM_RESPONSE: [("zp", (k, N)), ("zs", (V, k, N))],
    }[kind]


def pack(msgs: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """List of messages -> (data uint8, offsets uint64 [B+1]), messages back to back."""
    offsets = np.zeros(len(msgs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    data = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    return data, offsets


def split(data, offsets) -> List[bytes]:
    """(data, offsets) -> list of messages (numpy or torch)."""
    if type(data).__module__.startswith("torch"):
        data, offsets = data.cpu().numpy(), offsets.cpu().numpy()
    raw = np.asarray(data, dtype=np.uint8).tobytes()
    o = [int(v) for v in np.asarray(offsets).astype(np.uint64)]
    return [raw[o[b]:o[b + 1]] for b in range(len(o) - 1)]


def max_bytes(ctx, kind: int, V: Optional[int] = None, coef_bytes: int = 8) -> int:
    """Largest encoding of one message of the kind (rzk_wire_max_bytes)."""
    v = ctx._L.rzk_wire_max_bytes(ctx._h, kind, V or 0, coef_bytes)
    if v == 0:
        raise ValueError("bad message kind, coef_bytes or V")
    return int(v)


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _ptr(a) -> C.c_void_p:
    return C.c_void_p(a.data_ptr() if _is_torch(a) else a.ctypes.data)


def decode_batch(ctx, kind: int, data, offsets, V: Optional[int] = None, coef_bytes: int = 8):
    """B serialized messages -> (slab of every field, in declaration order..., ok).

    data: uint8 bytes (numpy, or a torch CUDA tensor for the device entry point on torch's current stream); offsets:
    [B+1] boundaries (numpy uint64 / torch int64).  ok[b] = 0 marks a message that does not decode (wrong counts, a
    polynomial longer than N, a bad Option tag, a coefficient that is not a centred residue mod q, trailing or missing
    bytes); its slabs are unspecified.  An Opening decoded from None has f = 1 (the same verdict, commit.rs:200-209)."""
    shapes = field_shapes(ctx, kind, V)
    B = int(offsets.shape[0]) - 1
    if B < 0:
        raise ValueError("offsets needs B + 1 entries")
    if _is_torch(data):
        import torch

        if not (data.is_cuda and offsets.is_cuda) or data.dtype != torch.uint8 or offsets.dtype != torch.int64:
            raise ValueError("device messages: uint8 data and int64 offsets, both CUDA tensors")
        data, offsets = data.contiguous(), offsets.contiguous()
        slabs = [torch.empty((B,) + sh, dtype=torch.int64, device=data.device) for _, sh in shapes]
        ok = torch.empty(B, dtype=torch.uint8, device=data.device)
        ctx._bind_torch_stream()
        fn = ctx._L.rzk_wire_decode_batch_dev
    else:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.ctypes.data % 8:
            data = data.copy()
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        slabs = [np.empty((B,) + sh, dtype=np.int64) for _, sh in shapes]
        ok = np.empty(B, dtype=np.uint8)
        fn = ctx._L.rzk_wire_decode_batch
    if data.shape[0] == 0:   # empty messages only: a valid dummy pointer
        data = (np.zeros(8, dtype=np.uint8) if not _is_torch(data) else data.new_zeros(8))[:8]
        total = 0
    else:
        total = int(data.shape[0])
    fields = (C.c_void_p * len(slabs))(*[_ptr(s).value for s in slabs])
    ctx._check(fn(ctx._h, kind, V or 0, coef_bytes, _ptr(data), total, _ptr(offsets), fields, _ptr(ok), B))
    return (*slabs, ok)


def encode_batch(ctx, kind: int, *slabs, V: Optional[int] = None, coef_bytes: int = 8):
    """Field slabs of B messages (declaration order; [B] + the shapes of field_shapes) -> (data, offsets).

    numpy in -> numpy out (uint8, uint64); torch CUDA tensors in -> torch out (uint8, int64) on the current stream.
    For an Opening, f = None encodes every message with f = None.  Polynomials are written trimmed.  Raises RzkError
    (RZK_E_ARG) when a coefficient is not a centred residue mod q."""
    shapes = field_shapes(ctx, kind, V)
    if len(slabs) != len(shapes):
        raise ValueError(f"{len(shapes)} field slabs expected, got {len(slabs)}")
    present = [s for s in slabs if s is not None]
    B = int(present[0].shape[0])
    dev = _is_torch(present[0])
    for (name, sh), s in zip(shapes, slabs):
        if s is None:
            if not (kind == MSG_OPENING and name == "f"):
                raise ValueError(f"field {name} is missing")
            continue
        if _is_torch(s) != dev or tuple(s.shape) != (B,) + sh:
            raise ValueError(f"field {name}: expected {(B,) + sh}, got {tuple(s.shape)}")
    cap = max(B * max_bytes(ctx, kind, V, coef_bytes), 8)
    if dev:
        import torch

        slabs = [s.contiguous() if s is not None else None for s in slabs]
        if any(s is not None and (s.dtype != torch.int64 or not s.is_cuda) for s in slabs):
            raise ValueError("device slabs must be int64 CUDA tensors")
        data = torch.empty(cap, dtype=torch.uint8, device=present[0].device)
        offsets = torch.empty(B + 1, dtype=torch.int64, device=present[0].device)
        ctx._bind_torch_stream()
        fn = ctx._L.rzk_wire_encode_batch_dev
    else:
        slabs = [np.ascontiguousarray(s, dtype=np.int64) if s is not None else None for s in slabs]
        data = np.empty(cap, dtype=np.uint8)
        offsets = np.empty(B + 1, dtype=np.uint64)
        fn = ctx._L.rzk_wire_encode_batch
    fields = (C.c_void_p * len(slabs))(*[_ptr(s).value if s is not None else None for s in slabs])
    ctx._check(fn(ctx._h, kind, V or 0, coef_bytes, fields, _ptr(data), cap, _ptr(offsets), B))
    if dev:
        ctx.synchronize()   # reports a non-canonical coefficient of this call
        total = int(offsets[-1].item()) if B else 0
    else:
        total = int(offsets[-1]) if B else 0
    return data[:total], offsets


def _msgs(m):
    """(data, offsets) or a list of bytes -> (data, offsets)."""
    return pack(m) if isinstance(m, (list, tuple)) and (not m or isinstance(m[0], (bytes, bytearray))) else m


def verify_open(ctx, commitment, challenge, response, coef_bytes: int = 8):
    """OpenProofVerifier::verify (open.rs:162-174) from serialized OpenProofCommitment, OpenProofChallenge and
    OpenProofResponse messages: accept[b] = decoded(b) && rzk_open_verify_batch."""
    c, t, ok1 = decode_batch(ctx, MSG_OPEN_COMMITMENT, *_msgs(commitment), coef_bytes=coef_bytes)
    (d, ok2) = decode_batch(ctx, MSG_CHALLENGE, *_msgs(challenge), coef_bytes=coef_bytes)
    (z, ok3) = decode_batch(ctx, MSG_OPEN_RESPONSE, *_msgs(response), coef_bytes=coef_bytes)
    return ctx.open_verify(z, t, c, d) & ok1 & ok2 & ok3


def verify_linear(ctx, commitment, challenge, z, zp, coef_bytes: int = 8):
    """LinearProofVerifier::verify (linear.rs:213-250) from serialized LinearProofCommitment and LinearProofChallenge
    messages; the response's z, zp (no serde derive, linear.rs:318) come as slabs [B][k][N]."""
    c, cp, g, t, tp, u, ok1 = decode_batch(ctx, MSG_LINEAR_COMMITMENT, *_msgs(commitment), coef_bytes=coef_bytes)
    (d, ok2) = decode_batch(ctx, MSG_CHALLENGE, *_msgs(challenge), coef_bytes=coef_bytes)
    return ctx.linear_verify(z, zp, c, cp, g, t, tp, u, d) & ok1 & ok2


def verify_sum(ctx, V: int, commitment, challenge, response, coef_bytes: int = 8):
    """SumProofVerifier::verify (sum.rs:257-320) from serialized SumProofCommitment, SumProofChallenge and
    SumProofResponse messages of V summands."""
    cp, cs, gs, tp, ts, u, ok1 = decode_batch(ctx, MSG_SUM_COMMITMENT, *_msgs(commitment), V=V, coef_bytes=coef_bytes)
    (d, ok2) = decode_batch(ctx, MSG_CHALLENGE, *_msgs(challenge), coef_bytes=coef_bytes)
    zp, zs, ok3 = decode_batch(ctx, MSG_SUM_RESPONSE, *_msgs(response), V=V, coef_bytes=coef_bytes)
    return ctx.sum_verify(zs, zp, cs, cp, gs, ts, tp, u, d) & ok1 & ok2 & ok3


def verify_commitment(ctx, commitment, opening, coef_bytes: int = 8):
    """Commitment::verify (commit.rs:173-210) from serialized Commitment and Opening messages (f = None decodes to
    f = 1, which gives the verdict of None)."""
    (c, ok1) = decode_batch(ctx, MSG_COMMITMENT, *_msgs(commitment), coef_bytes=coef_bytes)
    x, r, f, ok2 = decode_batch(ctx, MSG_OPENING, *_msgs(opening), coef_bytes=coef_bytes)
    return ctx.commitment_verify(c, x, r, f) & ok1 & ok2
