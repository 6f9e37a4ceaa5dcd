"""Fixed-width packed records "RZKP1" <-> dense int64 slabs (include/rzk.h "fixed-width packed records"),
or dense int32 slabs (`encode_batch32` / `decode_batch32`).

The compact stored form of the protocol messages: every record of a kind has the same size (`record_bytes`), each
coefficient takes the bits its field class needs (`widths`), and both directions are one GPU launch
(rzk_packed_{encode,decode}_batch[_dev]).  `wire.py` remains the reference's bincode form.

Kinds: the MSG_* values of `wire.py` except MSG_OPENING, plus MSG_LINEAR_RESPONSE { z, zp } and the short (signature)
forms of the three proofs, MSG_OPEN_SHORT { c, d, z }, MSG_LINEAR_SHORT { c, cp, g, d, z, zp } and MSG_SUM_SHORT
{ cp, cs, gs, d, zp, zs } (fiat_shamir.*_verify_short).  Inputs are numpy arrays (host entry
points) or torch CUDA tensors (device entry points on torch's current stream), as everywhere in the package.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from . import wire
from ._lib import (MSG_CHALLENGE, MSG_COMMITMENT, MSG_LINEAR_COMMITMENT, MSG_LINEAR_RESPONSE,  # noqa: F401
                   MSG_LINEAR_SHORT, MSG_OPEN_COMMITMENT, MSG_OPEN_RESPONSE, MSG_OPEN_SHORT, MSG_OPENING,
                   MSG_SUM_COMMITMENT, MSG_SUM_RESPONSE, MSG_SUM_SHORT)

KINDS = (MSG_COMMITMENT, MSG_CHALLENGE, MSG_OPEN_COMMITMENT, MSG_OPEN_RESPONSE, MSG_LINEAR_COMMITMENT, MSG_SUM_COMMITMENT,
         MSG_SUM_RESPONSE, MSG_LINEAR_RESPONSE, MSG_OPEN_SHORT)
SHORT_KINDS = (MSG_LINEAR_SHORT, MSG_SUM_SHORT)   # the short Linear and Sum proofs; also packed kinds


def widths(ctx) -> Tuple[int, int]:
    """(W_Q, W_Z): bits per coefficient of the commitment-side fields and of the response fields (rzk_packed_widths)."""
    wq, wz = C.c_uint32(0), C.c_uint32(0)
    ctx._check(ctx._L.rzk_packed_widths(ctx._h, C.byref(wq), C.byref(wz)))
    return int(wq.value), int(wz.value)


def record_bytes(ctx, kind: int, V: Optional[int] = None) -> int:
    """Size of one record of the kind (rzk_packed_record_bytes)."""
    v = ctx._L.rzk_packed_record_bytes(ctx._h, kind, V or 0)
    if v == 0:
        raise ValueError("bad message kind or V (or a context the packed format does not cover)")
    return int(v)


def field_shapes(ctx, kind: int, V: Optional[int] = None) -> List[Tuple[str, tuple]]:
    """wire.field_shapes extended by the kinds of the packed format only; MSG_OPENING is not a packed kind."""
    N, n, k, l = ctx.N, ctx.n, ctx.k, ctx.l
    if kind == MSG_LINEAR_RESPONSE:
        return [("z", (k, N)), ("zp", (k, N))]
    if kind == MSG_OPEN_SHORT:
        return [("c", (n + l, N)), ("d", (N,)), ("z", (k, N))]
    if kind == MSG_LINEAR_SHORT:
        return [("c", (n + l, N)), ("cp", (n + l, N)), ("g", (N,)), ("d", (N,)), ("z", (k, N)), ("zp", (k, N))]
    if kind == MSG_SUM_SHORT:
        if V is None or V < 1:
            raise ValueError("MSG_SUM_SHORT needs V >= 1")
        return [("cp", (n + l, N)), ("cs", (V, n + l, N)), ("gs", (V, N)), ("d", (N,)), ("zp", (k, N)), ("zs", (V, k, N))]
    if kind not in KINDS:
        raise ValueError("not a kind of the packed format")
    return wire.field_shapes(ctx, kind, V)


def _fields(slabs):
    return (C.c_void_p * len(slabs))(*[wire._ptr(s).value for s in slabs])


def encode_batch(ctx, kind: int, *slabs, V: Optional[int] = None):
    """Field slabs of B messages (declaration order; [B] + the shapes of field_shapes) -> (records, ok).

    records: uint8 [B][record_bytes]; ok: uint8 [B], 0 where a coefficient does not fit its field class (outside the
    centred range mod q, or a response coefficient beyond verify_bound): that record holds the all-ones marker in the
    coefficient's place and never decodes as valid."""
    return _encode(ctx, kind, slabs, V, np.int64)


def encode_batch32(ctx, kind: int, *slabs, V: Optional[int] = None):
    """encode_batch for int32 slabs (numpy int32 arrays or torch int32 CUDA tensors, rzk_packed_encode32_batch[_dev]):
    the same records and ok as encode_batch on the widened slabs.  Records carry no width."""
    return _encode(ctx, kind, slabs, V, np.int32)


def decode_batch32(ctx, kind: int, records, V: Optional[int] = None):
    """decode_batch into int32 slabs (rzk_packed_decode32_batch[_dev]): the same ok, and for an accepted record the same
    values as int32."""
    return _decode(ctx, kind, records, V, np.int32)


def _encode(ctx, kind, slabs, V, dt):
    w32 = dt is np.int32
    shapes = field_shapes(ctx, kind, V)
    if len(slabs) != len(shapes):
        raise ValueError(f"{len(shapes)} field slabs expected, got {len(slabs)}")
    B = int(slabs[0].shape[0])
    dev = wire._is_torch(slabs[0])
    for (name, sh), s in zip(shapes, slabs):
        if wire._is_torch(s) != dev or tuple(s.shape) != (B,) + sh:
            raise ValueError(f"field {name}: expected {(B,) + sh}, got {tuple(s.shape)}")
    size = record_bytes(ctx, kind, V)
    if dev:
        import torch

        slabs = [s.contiguous() for s in slabs]
        if any(s.dtype != (torch.int32 if w32 else torch.int64) or not s.is_cuda for s in slabs):
            raise ValueError("device slabs must be %s CUDA tensors" % ("int32" if w32 else "int64"))
        records = torch.empty((B, size), dtype=torch.uint8, device=slabs[0].device)
        ok = torch.empty(B, dtype=torch.uint8, device=slabs[0].device)
        ctx._bind_torch_stream()
        fn = ctx._L.rzk_packed_encode32_batch_dev if w32 else ctx._L.rzk_packed_encode_batch_dev
    else:
        if w32 and any(s.dtype != np.int32 for s in slabs):
            raise ValueError("host slabs must be int32 numpy arrays")
        slabs = [np.ascontiguousarray(s, dtype=dt) for s in slabs]
        records = np.empty((B, size // 8), dtype=np.uint64).view(np.uint8)   # 8-byte aligned
        ok = np.empty(B, dtype=np.uint8)
        fn = ctx._L.rzk_packed_encode32_batch if w32 else ctx._L.rzk_packed_encode_batch
    if B:
        ctx._check(fn(ctx._h, kind, V or 0, _fields(slabs), wire._ptr(records), wire._ptr(ok), B))
    return records, ok


def decode_batch(ctx, kind: int, records, V: Optional[int] = None):
    """records uint8 [B][record_bytes] (or flat, B * record_bytes) -> (slab of every field..., ok).

    ok[b] = 0 marks a record that does not decode (wrong header, a value above its class's limit, a set padding bit);
    its slabs are unspecified."""
    return _decode(ctx, kind, records, V, np.int64)


def _decode(ctx, kind, records, V, dt):
    w32 = dt is np.int32
    shapes = field_shapes(ctx, kind, V)
    size = record_bytes(ctx, kind, V)
    total = int(np.prod(tuple(records.shape), dtype=np.int64))
    if total % size:
        raise ValueError(f"records: {total} bytes is not a multiple of the record size {size}")
    B = total // size
    if wire._is_torch(records):
        import torch

        if not records.is_cuda or records.dtype != torch.uint8:
            raise ValueError("device records: a uint8 CUDA tensor")
        records = records.contiguous()
        if records.data_ptr() % 8:
            records = records.clone()
        slabs = [torch.empty((B,) + sh, dtype=torch.int32 if w32 else torch.int64, device=records.device) for _, sh in shapes]
        ok = torch.empty(B, dtype=torch.uint8, device=records.device)
        ctx._bind_torch_stream()
        fn = ctx._L.rzk_packed_decode32_batch_dev if w32 else ctx._L.rzk_packed_decode_batch_dev
    else:
        records = np.ascontiguousarray(records, dtype=np.uint8)
        if records.ctypes.data % 8:
            aligned = np.empty(total // 8, dtype=np.uint64).view(np.uint8)
            aligned[:] = records.reshape(-1)
            records = aligned
        slabs = [np.empty((B,) + sh, dtype=dt) for _, sh in shapes]
        ok = np.empty(B, dtype=np.uint8)
        fn = ctx._L.rzk_packed_decode32_batch if w32 else ctx._L.rzk_packed_decode_batch
    if B:
        ctx._check(fn(ctx._h, kind, V or 0, wire._ptr(records), _fields(slabs), wire._ptr(ok), B))
    return (*slabs, ok)
