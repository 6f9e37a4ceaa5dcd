"""ctypes binding of include/rzk.h.  Fails loudly when the HIP library is missing: there is no
CPU fallback in this package."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.environ.get("RZK_LIB", os.path.join(HERE, "librzk_hip.so"))  # RZK_LIB: tuning variants (tools/)

RZK_OK, RZK_E_ARG, RZK_E_HIP, RZK_E_STATE, RZK_E_UNSUPPORTED = 0, -1, -2, -3, -4
KEY_A1, KEY_A2, KEY_A = 0, 1, 2
# message kinds of the batched wire codec (include/rzk.h "protocol messages on the wire", v4)
(MSG_COMMITMENT, MSG_OPENING, MSG_CHALLENGE, MSG_OPEN_COMMITMENT, MSG_OPEN_RESPONSE, MSG_LINEAR_COMMITMENT,
 MSG_SUM_COMMITMENT, MSG_SUM_RESPONSE) = range(8)
# kinds of the packed format only (include/rzk.h "fixed-width packed records", v8)
MSG_LINEAR_RESPONSE, MSG_OPEN_SHORT = 8, 9
MSG_LINEAR_SHORT, MSG_SUM_SHORT = 11, 12   # v12; 10 is unassigned

_lib = None

_I64 = C.c_void_p  # int64_t* (host or device pointer, passed as an address)
_I32 = C.c_void_p  # int32_t* (32-bit coefficient slabs, v14)
_U8 = C.c_void_p
_U32P = C.c_void_p
_SZ = C.c_size_t
_CTX = C.c_void_p

# name -> (restype, argtypes); every symbol include/rzk.h declares
SIGNATURES = {
    "rzk_ctx_create": (C.c_int, [C.POINTER(_CTX), C.c_int64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_uint64, C.c_int]),
    "rzk_ctx_destroy": (None, [_CTX]),
    "rzk_abi_version": (C.c_uint32, []),
    "rzk_ctx_trust_device_outputs": (C.c_int, [_CTX, C.c_int]),
    "rzk_ctx_set_stream": (C.c_int, [_CTX, C.c_void_p]),
    "rzk_ctx_use_own_stream": (C.c_int, [_CTX]),
    "rzk_ctx_synchronize": (C.c_int, [_CTX]),
    "rzk_ctx_check_inputs": (C.c_int, [_CTX]),
    "rzk_last_error": (C.c_char_p, [_CTX]),
    "rzk_sigma": (C.c_uint64, [_CTX]),
    "rzk_commit_bound": (C.c_uint64, [_CTX]),
    "rzk_verify_bound": (C.c_uint64, [_CTX]),
    "rzk_key_load": (C.c_int, [_CTX, _I64]),
    "rzk_key_load_dev": (C.c_int, [_CTX, _I64]),
    "rzk_key_generate": (C.c_int, [_CTX, C.c_uint64, _I64]),
    "rzk_key_expand": (C.c_int, [_CTX, _U8, _I64]),   # v10
    "rzk_polymul_batch": (C.c_int, [_CTX, _I64, _I64, _I64, _SZ]),
    "rzk_matvec_batch": (C.c_int, [_CTX, C.c_int, _I64, _I64, _I64, _SZ]),
    "rzk_cmul_batch": (C.c_int, [_CTX, _I64, C.c_uint32, _I64, _I64, _SZ]),
    "rzk_canonicalize_batch": (C.c_int, [_CTX, _I64, _I64, _SZ]),
    "rzk_add_batch": (C.c_int, [_CTX, _I64, _I64, _I64, _SZ]),
    "rzk_sub_batch": (C.c_int, [_CTX, _I64, _I64, _I64, _SZ]),
    "rzk_norm2_le_batch": (C.c_int, [_CTX, _I64, C.c_uint32, C.c_uint64, _U8, _SZ]),
    "rzk_eq_batch": (C.c_int, [_CTX, _I64, _I64, C.c_uint32, _U8, _SZ]),
    "rzk_ntt_forward_batch": (C.c_int, [_CTX, C.c_int, _U32P, _U32P, _SZ]),
    "rzk_ntt_inverse_batch": (C.c_int, [_CTX, C.c_int, _U32P, _U32P, _SZ]),
    "rzk_ntt_prime": (C.c_uint32, [C.c_int]),
    "rzk_ntt_psi": (C.c_uint32, [C.c_int, C.c_uint32]),
    "rzk_ntt_layout_index": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "rzk_commit_batch": (C.c_int, [_CTX, _I64, _I64, _I64, _U8, _SZ]),
    "rzk_commitment_verify_batch": (C.c_int, [_CTX, _I64, _I64, _I64, _I64, _U8, _SZ]),
    "rzk_open_commit_batch": (C.c_int, [_CTX, _I64, _I64, _I64, _I64, _I64, _U8, _SZ]),
    "rzk_open_response_batch": (C.c_int, [_CTX, _I64, _I64, _I64, _I64, _SZ]),
    "rzk_open_verify_batch": (C.c_int, [_CTX, _I64, _I64, _I64, _I64, _U8, _SZ]),
    "rzk_linear_commit_batch": (C.c_int, [_CTX] + [_I64] * 11 + [_U8, _SZ]),
    "rzk_linear_response_batch": (C.c_int, [_CTX] + [_I64] * 7 + [_SZ]),
    "rzk_linear_verify_batch": (C.c_int, [_CTX] + [_I64] * 9 + [_U8, _SZ]),
    "rzk_sum_commit_batch": (C.c_int, [_CTX, C.c_uint32] + [_I64] * 11 + [_U8, _SZ]),
    "rzk_sum_response_batch": (C.c_int, [_CTX, C.c_uint32] + [_I64] * 7 + [_SZ]),
    "rzk_sum_verify_batch": (C.c_int, [_CTX, C.c_uint32] + [_I64] * 9 + [_U8, _SZ]),
    # v12: recompute steps of the short proofs
    "rzk_open_recover_batch": (C.c_int, [_CTX, _I64, _I64, _I64, _I64, _U8, _SZ]),
    "rzk_linear_recover_batch": (C.c_int, [_CTX] + [_I64] * 9 + [_U8, _SZ]),
    "rzk_sum_recover_batch": (C.c_int, [_CTX, C.c_uint32] + [_I64] * 9 + [_U8, _SZ]),
    "rzk_sample_uniform_dev": (C.c_int, [_CTX, C.c_uint64, C.c_uint32, C.c_uint64, _I64, _SZ]),
    "rzk_sample_gauss_dev": (C.c_int, [_CTX, C.c_uint64, C.c_uint32, C.c_double, _I64, _SZ]),
    "rzk_sample_challenge_dev": (C.c_int, [_CTX, C.c_uint64, C.c_uint32, _I64, _SZ]),
    # v6: keyed (ChaCha20) samplers
    "rzk_sampler_set_key": (C.c_int, [_CTX, _U8]),
    "rzk_sample_uniform_keyed_dev": (C.c_int, [_CTX, _U8, C.c_uint32, C.c_uint64, _I64, _SZ]),
    "rzk_sample_gauss_keyed_dev": (C.c_int, [_CTX, _U8, C.c_uint32, C.c_double, _I64, _SZ]),
    "rzk_sample_challenge_keyed_dev": (C.c_int, [_CTX, _U8, C.c_uint32, _I64, _SZ]),
    # v11: the exact discrete Gaussian (count in coefficients)
    "rzk_sample_dgauss_keyed_dev": (C.c_int, [_CTX, _U8, C.c_uint32, C.c_uint32, _I64, _SZ]),
    "rzk_wire_mat_size": (C.c_size_t, [_I64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rzk_wire_mat_encode": (C.c_int, [_I64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _U8, _SZ,
                                      C.POINTER(C.c_size_t)]),
    "rzk_wire_mat_decode": (C.c_int, [_U8, _SZ, C.c_uint32, C.c_uint32, C.c_int64, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32), _I64, _SZ, C.POINTER(C.c_size_t)]),
    # v4: batched codec of the protocol messages
    "rzk_wire_max_bytes": (C.c_size_t, [_CTX, C.c_int, C.c_uint32, C.c_uint32]),
    "rzk_wire_decode_batch": (C.c_int, [_CTX, C.c_int, C.c_uint32, C.c_uint32, _U8, C.c_uint64, C.c_void_p,
                                        C.c_void_p, _U8, _SZ]),
    "rzk_wire_encode_batch": (C.c_int, [_CTX, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, _U8, C.c_uint64,
                                        C.c_void_p, _SZ]),
    # v5: Fiat-Shamir challenges from the FS1 transcript
    "rzk_fs_key_digest": (C.c_int, [_CTX, _U8]),
    "rzk_fs_challenge_batch": (C.c_int, [_CTX, C.c_int, C.c_uint32, C.c_void_p, _U8, _I64, _U8, _U8, _SZ]),
    # v7: rejection sampling of the provers
    "rzk_reject_lnm": (C.c_double, [C.c_double]),
    "rzk_reject_batch": (C.c_int, [_CTX, C.c_uint32, C.c_void_p, C.c_void_p, _U32P, _I64, C.c_uint64, C.c_double, _U8, _I64,
                                   _SZ]),
    # v13: response and rejection test in one call (y.., r.., d, coin, R, lnM, z.., accept, E, B)
    "rzk_open_response_reject_batch": (C.c_int, [_CTX] + [_I64] * 4 + [C.c_uint64, C.c_double, _I64, _U8, _I64, _SZ]),
    "rzk_linear_response_reject_batch": (C.c_int, [_CTX] + [_I64] * 6 + [C.c_uint64, C.c_double, _I64, _I64, _U8, _I64, _SZ]),
    "rzk_sum_response_reject_batch": (C.c_int, [_CTX, C.c_uint32] + [_I64] * 6 + [C.c_uint64, C.c_double, _I64, _I64, _U8, _I64,
                                                                                 _SZ]),
    # v14: 32-bit coefficient slabs (int32_t* where the siblings take int64_t*)
    "rzk_narrow_batch": (C.c_int, [_CTX, _I64, _I32, _SZ]),
    "rzk_widen_batch": (C.c_int, [_CTX, _I32, _I64, _SZ]),
    "rzk_open_commit32_batch": (C.c_int, [_CTX] + [_I32] * 5 + [_U8, _SZ]),
    "rzk_open_response32_batch": (C.c_int, [_CTX] + [_I32] * 4 + [_SZ]),
    "rzk_open_verify32_batch": (C.c_int, [_CTX] + [_I32] * 4 + [_U8, _SZ]),
    "rzk_open_recover32_batch": (C.c_int, [_CTX] + [_I32] * 4 + [_U8, _SZ]),
    # v14, slab32 messages: the transcript hash, the packed codec and the short verifier's compare on int32_t slabs
    "rzk_fs_challenge32_batch": (C.c_int, [_CTX, C.c_int, C.c_uint32, C.c_void_p, _U8, _I32, _U8, _U8, _SZ]),
    "rzk_packed_encode32_batch": (C.c_int, [_CTX, C.c_int, C.c_uint32, C.c_void_p, _U8, _U8, _SZ]),
    "rzk_packed_decode32_batch": (C.c_int, [_CTX, C.c_int, C.c_uint32, _U8, C.c_void_p, _U8, _SZ]),
    "rzk_eq32_batch": (C.c_int, [_CTX, _I32, _I32, C.c_uint32, _U8, _SZ]),
    # v14, slab32 prover: keyed samplers writing int32 slabs, a1.y and the response with its rejection test on int32 slabs
    "rzk_sample_uniform_keyed32_dev": (C.c_int, [_CTX, _U8, C.c_uint32, C.c_uint64, _I32, _SZ]),
    "rzk_sample_gauss_keyed32_dev": (C.c_int, [_CTX, _U8, C.c_uint32, C.c_double, _I32, _SZ]),
    "rzk_sample_challenge_keyed32_dev": (C.c_int, [_CTX, _U8, C.c_uint32, _I32, _SZ]),
    "rzk_sample_dgauss_keyed32_dev": (C.c_int, [_CTX, _U8, C.c_uint32, C.c_uint32, _I32, _SZ]),
    "rzk_matvec32_batch": (C.c_int, [_CTX, C.c_int, _I32, _I32, _I32, _SZ]),
    "rzk_open_response_reject32_batch": (C.c_int, [_CTX] + [_I32] * 3 + [_I64, C.c_uint64, C.c_double, _I32, _U8, _I64, _SZ]),
    # v14, prover loop: the zero-knowledge Open prover with its rejection loop inside the library
    # (x, nonce0, stream, gauss_kind, aux32, max_rounds, c, t, z, r, ok, rounds, rounds_run, B)
    "rzk_open_prove_zk_batch": (C.c_int, [_CTX, _I64, _U8, C.c_uint32, C.c_int, _U8, C.c_uint32] + [_I64] * 4 +
                                [_U8, _U8, C.POINTER(C.c_uint32), _SZ]),
    "rzk_open_prove_zk32_batch": (C.c_int, [_CTX, _I32, _U8, C.c_uint32, C.c_int, _U8, C.c_uint32] + [_I32] * 4 +
                                  [_U8, _U8, C.POINTER(C.c_uint32), _SZ]),
    # v14, additions: the y-only half of the Linear / Sum commit step (g, y, yp, t, tp, u, B), Sum with V in front
    "rzk_linear_mask_batch": (C.c_int, [_CTX] + [_I64] * 6 + [_SZ]),
    "rzk_sum_mask_batch": (C.c_int, [_CTX, C.c_uint32] + [_I64] * 6 + [_SZ]),
    # ... and the zero-knowledge Linear / Sum provers with their rejection loop inside the library
    # (g, x, nonce0, stream, gauss_kind, aux32, max_rounds, c, cp, t, tp, u, z, zp, r, rp, ok, rounds, rounds_run, B)
    "rzk_linear_prove_zk_batch": (C.c_int, [_CTX, _I64, _I64, _U8, C.c_uint32, C.c_int, _U8, C.c_uint32] + [_I64] * 9 +
                                  [_U8, _U8, C.POINTER(C.c_uint32), _SZ]),
    "rzk_sum_prove_zk_batch": (C.c_int, [_CTX, C.c_uint32, _I64, _I64, _U8, C.c_uint32, C.c_int, _U8, C.c_uint32] + [_I64] * 9 +
                               [_U8, _U8, C.POINTER(C.c_uint32), _SZ]),
    # v14, slab32 Linear: the Linear cycle, its recompute step and the norm predicate on int32 slabs (arguments as the siblings')
    "rzk_linear_commit32_batch": (C.c_int, [_CTX] + [_I32] * 11 + [_U8, _SZ]),
    "rzk_linear_mask32_batch": (C.c_int, [_CTX] + [_I32] * 6 + [_SZ]),
    "rzk_linear_response32_batch": (C.c_int, [_CTX] + [_I32] * 7 + [_SZ]),
    "rzk_linear_response_reject32_batch": (C.c_int, [_CTX] + [_I32] * 5 + [_I64, C.c_uint64, C.c_double, _I32, _I32, _U8, _I64, _SZ]),
    "rzk_linear_verify32_batch": (C.c_int, [_CTX] + [_I32] * 9 + [_U8, _SZ]),
    "rzk_linear_recover32_batch": (C.c_int, [_CTX] + [_I32] * 9 + [_U8, _SZ]),
    "rzk_norm2_le32_batch": (C.c_int, [_CTX, _I32, C.c_uint32, C.c_uint64, _U8, _SZ]),
    "rzk_debug_compact_dev": (C.c_int, [_CTX, _U8, _U8, _SZ, _U32P, _U32P]),
    # v8: fixed-width packed records
    "rzk_packed_record_bytes": (C.c_size_t, [_CTX, C.c_int, C.c_uint32]),
    "rzk_packed_widths": (C.c_int, [_CTX, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rzk_packed_encode_batch": (C.c_int, [_CTX, C.c_int, C.c_uint32, C.c_void_p, _U8, _U8, _SZ]),
    "rzk_packed_decode_batch": (C.c_int, [_CTX, C.c_int, C.c_uint32, _U8, C.c_void_p, _U8, _SZ]),
    # v10: seed expansion "XP1"
    "rzk_xof_uniform_batch": (C.c_int, [_CTX, _U8, C.c_uint32, C.c_uint32, _I64, _SZ]),
    "rzk_bench_ntt_forward_dev": (C.c_double, [_CTX, C.c_int, _U32P, _U32P, _SZ, C.c_int]),
    "rzk_debug_read_scratch": (C.c_int, [_CTX, C.c_void_p, _SZ, C.POINTER(C.c_size_t)]),
    "rzk_debug_gauss_map_dev": (C.c_int, [_CTX, C.c_int, C.c_void_p, C.c_double, _I64, _SZ]),
    "rzk_debug_dgauss_trial_dev": (C.c_int, [_CTX, C.c_uint32, C.c_void_p, _I64, _SZ]),   # v11
    "rzk_prof_reset": (C.c_int, [_CTX]),
    "rzk_prof_enable": (C.c_int, [_CTX, C.c_int]),
    "rzk_prof_read": (C.c_int, [_CTX, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "rzk_prof_count": (C.c_uint64, [_CTX]),
    "rzk_prof_read_all": (C.c_int, [_CTX, C.POINTER(C.c_double), _SZ, C.POINTER(C.c_size_t)]),
    "rzk_prof_read_kernels": (C.c_int, [_CTX, C.c_char_p, _SZ, C.POINTER(C.c_size_t)]),
}
ABI_VERSION = 14   # include/rzk.h: RZK_ABI_VERSION
# every batched entry point also exists as a device-pointer variant with the same signature
for _name in list(SIGNATURES):
    if _name.endswith("_batch"):
        SIGNATURES[_name + "_dev"] = SIGNATURES[_name]


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise RuntimeError(
                f"{SO} is missing: build it with `python -m ring_zk_amd.build` (hipcc, gfx950). "
                "The ring-zk MI355X backend has no CPU fallback.")
        # PyTorch bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Device memory and streams
        # are shared with torch, so torch's HIP runtime must be the one this process uses: load it first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(SO)
        # a stale or variant library with another ABI must fail here, not read shifted arguments later
        try:
            L.rzk_abi_version.restype = C.c_uint32
            have = int(L.rzk_abi_version())
        except AttributeError:
            have = None
        if have != ABI_VERSION:
            raise RuntimeError(f"{SO}: C ABI version {have}, this binding needs {ABI_VERSION} (include/rzk.h); rebuild with "
                               "`python -m ring_zk_amd.build`")
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib
