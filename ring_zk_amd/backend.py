"""Thin Python host layer over the C ABI (include/rzk.h).

`Context` mirrors `Params<ZqI64<Q>>` + const generic `N` of the reference (src/params.rs:18-36) and
owns one `rzk_ctx`.  Every method takes either numpy arrays (host pointers -> the synchronous
`rzk_*_batch` entry points) or torch CUDA tensors (device pointers -> the asynchronous `*_dev` entry
points on torch's current stream).  PyTorch is used only for device memory and streams; all
arithmetic happens in the HIP library.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib

Q_DEFAULT = 3515337053  # ZqI64<3515337053>, src/params.rs:121


class RzkError(RuntimeError):
    """Non-zero status from the C ABI (the Rust shim turns it into panic!)."""

    def __init__(self, status: int, msg: str):
        super().__init__(f"rzk status {status}: {msg}")
        self.status = status


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class Context:
    def __init__(self, N: int, n: int = 1, k: int = 3, l: int = 1, kappa: int = 36, b: int = 1,
                 q: int = Q_DEFAULT, device: int = 0):
        self._L = _lib.lib()
        self.N, self.n, self.k, self.l, self.kappa, self.b, self.q = N, n, k, l, kappa, b, q
        self.device = device
        h = C.c_void_p()
        st = self._L.rzk_ctx_create(C.byref(h), q, N, n, k, l, kappa, b, device)
        if st != 0:
            raise RzkError(st, "rzk_ctx_create: " + self._L.rzk_last_error(None).decode())
        self._h = h
        self._stream = None
        self.half = (q - 1) // 2

    # ---- plumbing --------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.rzk_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int):
        if st != 0:
            raise RzkError(st, self._L.rzk_last_error(self._h).decode())

    def synchronize(self):
        self._check(self._L.rzk_ctx_synchronize(self._h))

    @property
    def sigma(self) -> int:
        return self._L.rzk_sigma(self._h)

    @property
    def commit_bound(self) -> int:
        return self._L.rzk_commit_bound(self._h)

    @property
    def verify_bound(self) -> int:
        return self._L.rzk_verify_bound(self._h)

    def _bind_torch_stream(self):
        import torch

        s = torch.cuda.current_stream(self.device).cuda_stream   # 0 = HIP's default stream
        if s != self._stream:
            self._check(self._L.rzk_ctx_set_stream(self._h, C.c_void_p(s)))
            self._stream = s

    def _prep(self, arrs: Sequence, dtypes: Sequence):
        """Validate inputs; returns (is_device, pointers)."""
        present = [a for a in arrs if a is not None]
        dev = _is_torch(present[0])
        ptrs = []
        for a, dt in zip(arrs, dtypes):
            if a is None:
                ptrs.append(None)
                continue
            if _is_torch(a) != dev:
                raise ValueError("mixing host (numpy) and device (torch) buffers in one call")
            if dev:
                import torch

                want = {np.int64: torch.int64, np.int32: torch.int32, np.uint32: torch.int32, np.uint8: torch.uint8}[dt]
                if a.dtype != want or not a.is_cuda or not a.is_contiguous():
                    raise ValueError("device buffers must be contiguous CUDA tensors of the right dtype")
                ptrs.append(C.c_void_p(a.data_ptr()))
            else:
                if a.dtype != dt or not a.flags["C_CONTIGUOUS"]:
                    raise ValueError("host buffers must be C-contiguous numpy arrays of the right dtype")
                ptrs.append(C.c_void_p(a.ctypes.data))
        if dev:
            self._bind_torch_stream()
        return dev, ptrs

    def _empty(self, like, shape, dtype=np.int64):
        if _is_torch(like):
            import torch

            tdt = {np.int64: torch.int64, np.int32: torch.int32, np.uint32: torch.int32, np.uint8: torch.uint8}[dtype]
            return torch.empty(shape, dtype=tdt, device=like.device)
        return np.empty(shape, dtype=dtype)

    def _fn(self, name: str, dev: bool):
        return getattr(self._L, name + ("_dev" if dev else ""))

    def _shape(self, a, *tail):
        if tuple(a.shape[-len(tail):]) != tuple(tail):
            raise ValueError(f"shape mismatch: expected trailing dims {tail}, got {tuple(a.shape)}")
        return int(np.prod(a.shape[:-len(tail)], dtype=np.int64)) if a.ndim > len(tail) else 1

    # ---- key ---------------------------------------------------------------------------------------
    def generate_key(self, seed: int) -> np.ndarray:
        """CommitmentKey::new (commit.rs:33-60) from the device-side sampler; loads the key and returns it."""
        a = np.empty((self.n + self.l, self.k, self.N), dtype=np.int64)
        self._check(self._L.rzk_key_generate(self._h, seed, C.c_void_p(a.ctypes.data)))
        return a

    def expand_key(self, seed: bytes) -> np.ndarray:
        """CommitmentKey::new as a public function of a 32-byte seed (rzk_key_expand): the general entry at
        row i, column j is polynomial i*k + j of the XP1 expansion under domain 0.  Loads the key and returns it."""
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("the key seed must be 32 bytes")
        a = np.empty((self.n + self.l, self.k, self.N), dtype=np.int64)
        self._check(self._L.rzk_key_expand(self._h, (C.c_uint8 * 32).from_buffer_copy(seed), C.c_void_p(a.ctypes.data)))
        return a

    def load_key(self, A):
        """CommitmentKey as the dense matrix [a1;a2] ((n+l) x k polynomials; src/commit.rs:109-114)."""
        self._shape(A, self.n + self.l, self.k, self.N)
        dev, (p,) = self._prep([A], [np.int64])
        self._check(self._fn("rzk_key_load", dev)(self._h, p))

    # ---- Mat seam ------------------------------------------------------------------------------------
    def polymul(self, a, b):
        cnt = self._shape(a, self.N)
        if self._shape(b, self.N) != cnt:
            raise ValueError("polymul: operand counts differ")
        out = self._empty(a, tuple(a.shape))
        dev, p = self._prep([a, b, out], [np.int64] * 3)
        self._check(self._fn("rzk_polymul_batch", dev)(self._h, p[0], p[1], p[2], cnt))
        return out

    def _rows(self, which: int) -> int:
        return {_lib.KEY_A1: self.n, _lib.KEY_A2: self.l, _lib.KEY_A: self.n + self.l}[which]

    # Entry points that exist for int64 and int32 slabs (include/rzk.h "32-bit slabs") share one private body, parametrised
    # by the method's name (for its messages), the dtype of its slabs and the symbol: _prep rejects the other dtype.
    def _matvec(self, name, dt, sym, which, v, addend):
        B = self._shape(v, self.k, self.N)
        rows = self._rows(which)
        if addend is not None and self._shape(addend, rows, self.N) != B:
            raise ValueError(f"{name}: addend batch differs")
        out = self._empty(v, tuple(v.shape[:-2]) + (rows, self.N), dt)
        dev, p = self._prep([v, addend, out], [dt] * 3)
        self._check(self._fn(sym, dev)(self._h, which, p[0], p[1], p[2], B))
        return out

    def matvec(self, which: int, v, addend=None):
        """Mat::dot with the key on the left (src/mat.rs:95-115), optional `.add(&z)` (commit.rs:125)."""
        return self._matvec("matvec", np.int64, "rzk_matvec_batch", which, v, addend)

    def cmul(self, m, p_):
        """Mat::componentwise_mul (src/mat.rs:168-178): m [B, rows, N], p [B, N]."""
        rows = int(m.shape[-2])
        B = self._shape(m, rows, self.N)
        if self._shape(p_, self.N) != B:
            raise ValueError("cmul: batch differs")
        out = self._empty(m, tuple(m.shape))
        dev, p = self._prep([m, p_, out], [np.int64] * 3)
        self._check(self._fn("rzk_cmul_batch", dev)(self._h, p[0], rows, p[1], p[2], B))
        return out

    def _addsub(self, name, a, b):
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError("Mat::add / Mat::sub dimension mismatch (mat.rs:129-130, 154-155)")
        cnt = self._shape(a, self.N)
        out = self._empty(a, tuple(a.shape))
        dev, p = self._prep([a, b, out], [np.int64] * 3)
        self._check(self._fn(name, dev)(self._h, p[0], p[1], p[2], cnt))
        return out

    def add(self, a, b):
        return self._addsub("rzk_add_batch", a, b)

    def sub(self, a, b):
        return self._addsub("rzk_sub_batch", a, b)

    def canonicalize(self, a):
        """Any int64 coefficients -> centred residues mod q (the other calls require canonical inputs)."""
        cnt = self._shape(a, self.N)
        out = self._empty(a, tuple(a.shape))
        dev, p = self._prep([a, out], [np.int64] * 2)
        self._check(self._fn("rzk_canonicalize_batch", dev)(self._h, p[0], p[1], cnt))
        return out

    def _norm2_le(self, dt, sym, v, bound):
        rows = int(v.shape[-2])
        B = self._shape(v, rows, self.N)
        ok = self._empty(v, (B,), np.uint8)
        dev, p = self._prep([v, ok], [dt, np.uint8])
        self._check(self._fn(sym, dev)(self._h, p[0], rows, bound, p[1], B))
        return ok

    def norm2_le(self, v, bound: int):
        return self._norm2_le(np.int64, "rzk_norm2_le_batch", v, bound)

    def eq(self, a, b):
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError("eq: shape mismatch")
        rows = int(a.shape[-2])
        B = self._shape(a, rows, self.N)
        out = self._empty(a, (B,), np.uint8)
        dev, p = self._prep([a, b, out], [np.int64, np.int64, np.uint8])
        self._check(self._fn("rzk_eq_batch", dev)(self._h, p[0], p[1], rows, p[2], B))
        return out

    # ---- transforms -------------------------------------------------------------------------------------
    def ntt_forward(self, prime: int, x):
        cnt = self._shape(x, self.N)
        out = self._empty(x, tuple(x.shape), np.uint32)
        dev, p = self._prep([x, out], [np.uint32] * 2)
        self._check(self._fn("rzk_ntt_forward_batch", dev)(self._h, prime, p[0], p[1], cnt))
        return out

    def ntt_inverse(self, prime: int, x):
        cnt = self._shape(x, self.N)
        out = self._empty(x, tuple(x.shape), np.uint32)
        dev, p = self._prep([x, out], [np.uint32] * 2)
        self._check(self._fn("rzk_ntt_inverse_batch", dev)(self._h, prime, p[0], p[1], cnt))
        return out

    def ntt_prime(self, prime: int) -> int:
        return self._L.rzk_ntt_prime(prime)

    def ntt_psi(self, prime: int) -> int:
        return self._L.rzk_ntt_psi(prime, self.N)

    def ntt_layout(self) -> np.ndarray:
        """perm[j] = position in the library's NTT-domain layout of standard (bit-reversed) element j."""
        return np.array([self._L.rzk_ntt_layout_index(self.N, j) for j in range(self.N)], dtype=np.int64)

    def bench_ntt_forward(self, prime: int, x, out, iters: int) -> float:
        """Average duration (us) of one batched forward-NTT launch, HIP events on the launch stream."""
        cnt = self._shape(x, self.N)
        dev, p = self._prep([x, out], [np.uint32] * 2)
        if not dev:
            raise ValueError("bench_ntt_forward needs device buffers")
        us = self._L.rzk_bench_ntt_forward_dev(self._h, prime, p[0], p[1], cnt, iters)
        if us < 0:
            raise RzkError(int(us), self._L.rzk_last_error(self._h).decode())
        return us

    # ---- profiling of the row kernel (HIP events on the launch stream) ----------------------------------------
    def prof_enable(self, on: bool = True):
        self._check(self._L.rzk_prof_enable(self._h, 1 if on else 0))

    def prof_reset(self):
        self._check(self._L.rzk_prof_reset(self._h))

    def prof_read(self):
        us, cnt = C.c_double(), C.c_uint64()
        self._check(self._L.rzk_prof_read(self._h, C.byref(us), C.byref(cnt)))
        return us.value, cnt.value

    def prof_count(self) -> int:
        """Launches recorded so far (no synchronisation)."""
        return int(self._L.rzk_prof_count(self._h))

    def prof_read_all(self):
        """Durations (us) of the recorded launches, in launch order."""
        n = self.prof_count()
        buf = (C.c_double * max(n, 1))()
        cnt = C.c_size_t(0)
        self._check(self._L.rzk_prof_read_all(self._h, buf, n, C.byref(cnt)))
        return [buf[i] for i in range(min(n, cnt.value))]

    def prof_read_kernels(self):
        """[(kernel template instance, algorithmic bytes)] of the recorded launches, in launch order."""
        need = C.c_size_t(0)
        self._check(self._L.rzk_prof_read_kernels(self._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value + 1)
        self._check(self._L.rzk_prof_read_kernels(self._h, buf, need.value + 1, C.byref(need)))
        out = []
        for line in buf.value.decode().splitlines():
            name, nbytes = line.rsplit("\t", 1)
            out.append((name, int(nbytes)))
        return out

    def trust_device_outputs(self, on=True):
        """Trusted-producer mode (rzk_ctx_trust_device_outputs): skip the canonical test of loaded coefficients."""
        self._check(self._L.rzk_ctx_trust_device_outputs(self._h, 1 if on else 0))

    # ---- device-side samplers (statistical parity with src/polynomial.rs:14-44, src/challenge_space.rs:12-33) ----
    def _sample_out(self, lead, dt=np.int64):
        import torch

        self._bind_torch_stream()
        shape = tuple(lead) + (self.N,)
        tdt = torch.int32 if dt is np.int32 else torch.int64
        out = torch.empty(shape, dtype=tdt, device=torch.device("cuda", self.device))
        return out, int(np.prod(shape[:-1], dtype=np.int64))

    def sample_uniform(self, seed: int, stream: int, bound: int, lead):
        """[*lead][N] coefficients uniform in [-bound, bound] (random_polynomial_within)."""
        out, cnt = self._sample_out(lead)
        self._check(self._L.rzk_sample_uniform_dev(self._h, seed, stream, bound, C.c_void_p(out.data_ptr()), cnt))
        return out

    def sample_gauss(self, seed: int, stream: int, sigma: float, lead):
        """[*lead][N] coefficients (i64) N(0, sigma) (random_polynomial_in_normal_distribution)."""
        out, cnt = self._sample_out(lead)
        self._check(self._L.rzk_sample_gauss_dev(self._h, seed, stream, float(sigma), C.c_void_p(out.data_ptr()), cnt))
        return out

    def sample_challenge(self, seed: int, stream: int, lead):
        """[*lead][N] challenges: kappa coefficients +-1 (random_polynomial_from_challenge_set)."""
        out, cnt = self._sample_out(lead)
        self._check(self._L.rzk_sample_challenge_dev(self._h, seed, stream, C.c_void_p(out.data_ptr()), cnt))
        return out

    def debug_gauss_map(self, f32: bool, words, sigma: float):
        """Diagnostic (rzk_debug_gauss_map_dev): the Gaussian samplers' word-to-pair map on chosen words.
        words: uint32 [pairs][4] (numpy) -> int64 numpy [pairs][2]."""
        import torch

        self._bind_torch_stream()
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if w.ndim != 2 or w.shape[1] != 4:
            raise ValueError("words must be [pairs][4]")
        dev = torch.device("cuda", self.device)
        d_w = torch.from_numpy(w.view(np.int32)).to(dev)
        out = torch.empty((w.shape[0], 2), dtype=torch.int64, device=dev)
        self._check(self._L.rzk_debug_gauss_map_dev(self._h, 1 if f32 else 0, C.c_void_p(d_w.data_ptr()), float(sigma),
                                                    C.c_void_p(out.data_ptr()), w.shape[0]))
        return out.cpu().numpy()

    def debug_dgauss_trial(self, words, sigma: int):
        """Diagnostic (rzk_debug_dgauss_trial_dev): one trial of the exact discrete Gaussian sampler on chosen words.
        words: uint32 [trials][8] (numpy) -> int64 numpy [trials][2] = (accepted, value)."""
        import torch

        self._bind_torch_stream()
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if w.ndim != 2 or w.shape[1] != 8:
            raise ValueError("words must be [trials][8]")
        dev = torch.device("cuda", self.device)
        d_w = torch.from_numpy(w.view(np.int32)).to(dev)
        out = torch.empty((w.shape[0], 2), dtype=torch.int64, device=dev)
        self._check(self._L.rzk_debug_dgauss_trial_dev(self._h, int(sigma), C.c_void_p(d_w.data_ptr()),
                                                       C.c_void_p(out.data_ptr()), w.shape[0]))
        return out.cpu().numpy()

    # ---- keyed samplers: the same distributions from ChaCha20 under a 256-bit key (include/rzk.h "keyed") ----
    def set_sampler_key(self, key: Optional[bytes]):
        """Key of the keyed samplers (32 bytes; None clears it).  The context keeps a copy in host memory and wipes it
        when it is replaced, cleared or the context is closed."""
        if key is None:
            self._check(self._L.rzk_sampler_set_key(self._h, None))
            return
        key = bytes(key)
        if len(key) != 32:
            raise ValueError("the sampler key must be 32 bytes")
        self._check(self._L.rzk_sampler_set_key(self._h, (C.c_uint8 * 32).from_buffer_copy(key)))

    @staticmethod
    def _nonce(nonce: bytes):
        nonce = bytes(nonce)
        if len(nonce) != 16:
            raise ValueError("the nonce must be 16 bytes")
        return (C.c_uint8 * 16).from_buffer_copy(nonce)

    def _sample_keyed(self, dt, sym, nonce, stream, args, lead, per_poly=1):
        """One keyed draw into a fresh [*lead][N] tensor of dtype dt; the symbol counts polynomials, or coefficients
        (per_poly = N)."""
        out, cnt = self._sample_out(lead, dt)
        self._check(getattr(self._L, sym)(self._h, self._nonce(nonce), stream, *args, C.c_void_p(out.data_ptr()), cnt * per_poly))
        return out

    def _sample_dgauss_keyed(self, name, dt, sym, nonce, stream, sigma, lead):
        if int(sigma) != sigma:
            raise ValueError(f"{name}: sigma must be an integer")
        return self._sample_keyed(dt, sym, nonce, stream, (int(sigma),), lead, self.N)

    def sample_uniform_keyed(self, nonce: bytes, stream: int, bound: int, lead):
        """sample_uniform from the keyed generator.  A (key, nonce, stream) triple must never serve two draws."""
        return self._sample_keyed(np.int64, "rzk_sample_uniform_keyed_dev", nonce, stream, (bound,), lead)

    def sample_gauss_keyed(self, nonce: bytes, stream: int, sigma: float, lead):
        """sample_gauss from the keyed generator."""
        return self._sample_keyed(np.int64, "rzk_sample_gauss_keyed_dev", nonce, stream, (float(sigma),), lead)

    def sample_dgauss_keyed(self, nonce: bytes, stream: int, sigma: int, lead):
        """[*lead][N] coefficients from the exact discrete Gaussian D_sigma over the integers (integer sigma in
        [1, 2^26]; rzk_sample_dgauss_keyed_dev), from the keyed generator."""
        return self._sample_dgauss_keyed("sample_dgauss_keyed", np.int64, "rzk_sample_dgauss_keyed_dev", nonce, stream, sigma, lead)

    def sample_challenge_keyed(self, nonce: bytes, stream: int, lead):
        """sample_challenge from the keyed generator."""
        return self._sample_keyed(np.int64, "rzk_sample_challenge_keyed_dev", nonce, stream, (), lead)

    # ---- seed expansion: uniform ring elements from public seeds with SHAKE256 (include/rzk.h "XP1") ----------
    def xof_uniform(self, seeds, rows: int, domain: int):
        """seeds [B, 32] uint8 -> [B, rows, N] int64: out[b][r] is polynomial r of the XP1 expansion under seeds[b] and
        `domain` (not 0, which is the keys').  numpy seeds go through the host entry point, torch CUDA seeds through the
        device one on torch's current stream.  For public data only."""
        if seeds.ndim != 2 or int(seeds.shape[1]) != 32:
            raise ValueError("xof_uniform: seeds must be [B, 32] uint8")
        B = int(seeds.shape[0])
        out = self._empty(seeds, (B, int(rows), self.N))
        dev, p = self._prep([seeds, out], [np.uint8, np.int64])
        self._check(self._fn("rzk_xof_uniform_batch", dev)(self._h, p[0], int(domain), int(rows), p[1], B))
        return out

    # ---- rejection sampling of the provers (include/rzk.h "rejection sampling") ----------------------------
    def reject(self, parts, coin, R: int, lnM: float):
        """The prover's rejection test of B proofs: (accept [B] uint8, E [B] int64).

        parts: 1 .. 4 pairs (z, y) of equally shaped slabs [B][...][N] that together hold every response polynomial of a
        proof and the y it was made from (Open: [(z, y)]; Linear: [(z, y), (zp, yp)]; Sum: [(zs, ys), (zp, yp)]);
        coin [B] int64, uniform in [0, R), 2 <= R <= 2^62; lnM = ln M >= 0 (reject_lnm)."""
        parts = list(parts)
        B = int(coin.shape[0])
        if coin.ndim != 1 or not 1 <= len(parts) <= 4:
            raise ValueError("reject: coin must be [B] and parts 1 .. 4 pairs (z, y)")
        rows = []
        for z, y in parts:
            if tuple(z.shape) != tuple(y.shape) or z.ndim < 2 or int(z.shape[0]) != B or int(z.shape[-1]) != self.N:
                raise ValueError("reject: every pair is two slabs [B][...][N] of one shape")
            rows.append(int(np.prod(z.shape[1:-1], dtype=np.int64)))
        accept = self._empty(coin, (B,), np.uint8)
        E = self._empty(coin, (B,), np.int64)
        zs, ys = [z for z, _ in parts], [y for _, y in parts]
        dev, p = self._prep(zs + ys + [coin, accept, E], [np.int64] * (2 * len(parts) + 1) + [np.uint8, np.int64])
        n = len(parts)
        zp = (C.c_void_p * n)(*[q.value for q in p[:n]])
        yp = (C.c_void_p * n)(*[q.value for q in p[n:2 * n]])
        self._check(self._fn("rzk_reject_batch", dev)(self._h, n, zp, yp, (C.c_uint32 * n)(*rows), p[2 * n], R, float(lnM),
                                                      p[2 * n + 1], p[2 * n + 2], B))
        return accept, E

    # The response and its rejection test in one call (include/rzk.h v13): z as *_response writes it, accept and
    # E as reject returns them for that z; at N = 512 / 1024 the response rows accumulate the statistic themselves.
    def _response_reject(self, name, head, ins, outs, coin, R, lnM, dt=np.int64):
        B = int(coin.shape[0])
        if coin.ndim != 1:
            raise ValueError(f"{name}: coin must be [B]")
        accept = self._empty(coin, (B,), np.uint8)
        E = self._empty(coin, (B,), np.int64)
        dev, p = self._prep(ins + [coin] + outs + [accept, E], [dt] * len(ins) + [np.int64] + [dt] * len(outs) + [np.uint8, np.int64])
        n = len(ins) + 1
        self._check(self._fn(name, dev)(self._h, *head, *p[:n], R, float(lnM), *p[n:], B))
        return accept, E

    def _open_response_reject(self, name, dt, sym, y, r, d, coin, R, lnM):
        B = self._shape(y, self.k, self.N)
        # (a coin that is not [B]: the int32 form says so here, the int64 form in _response_reject, as they always have)
        if (self._shape(r, self.k, self.N) != B or self._shape(d, self.N) != B or int(coin.shape[0]) != B
                or (dt is np.int32 and coin.ndim != 1)):
            raise ValueError(f"{name}: batch / shape mismatch")
        z = self._empty(y, tuple(y.shape), dt)
        accept, E = self._response_reject(sym, (), [y, r, d], [z], coin, R, lnM, dt)
        return z, accept, E

    def open_response_reject(self, y, r, d, coin, R: int, lnM: float):
        """open_response and reject([(z, y)], coin, R, lnM) in one call: (z, accept, E)."""
        return self._open_response_reject("open_response_reject", np.int64, "rzk_open_response_reject_batch", y, r, d, coin, R, lnM)

    def _linear_response_reject(self, name, dt, sym, y, yp, r, rp, d, coin, R, lnM):
        B = self._shape(y, self.k, self.N)
        if any(self._shape(a, self.k, self.N) != B for a in (yp, r, rp)) or self._shape(d, self.N) != B or int(coin.shape[0]) != B:
            raise ValueError(f"{name}: batch / shape mismatch")
        z = self._empty(y, tuple(y.shape), dt)
        zp = self._empty(y, tuple(y.shape), dt)
        accept, E = self._response_reject(sym, (), [y, yp, r, rp, d], [z, zp], coin, R, lnM, dt)
        return z, zp, accept, E

    def linear_response_reject(self, y, yp, r, rp, d, coin, R: int, lnM: float):
        """linear_response and reject([(z, y), (zp, yp)], coin, R, lnM) in one call: (z, zp, accept, E)."""
        return self._linear_response_reject("linear_response_reject", np.int64, "rzk_linear_response_reject_batch", y, yp, r, rp, d,
                                            coin, R, lnM)

    def sum_response_reject(self, ys, yp, rs, rp, d, coin, R: int, lnM: float):
        """sum_response and reject([(zs, ys), (zp, yp)], coin, R, lnM) in one call: (zs, zp, accept, E)."""
        V = int(ys.shape[-3])
        B = self._shape(ys, V, self.k, self.N)
        if (self._shape(rs, V, self.k, self.N) != B or self._shape(yp, self.k, self.N) != B or self._shape(rp, self.k, self.N) != B
                or self._shape(d, self.N) != B or int(coin.shape[0]) != B):
            raise ValueError("sum_response_reject: batch / shape mismatch")
        zs = self._empty(ys, tuple(ys.shape))
        zp = self._empty(yp, tuple(yp.shape))
        accept, E = self._response_reject("rzk_sum_response_reject_batch", (V,), [ys, yp, rs, rp, d], [zs, zp], coin, R, lnM)
        return zs, zp, accept, E

    # ---- commitment scheme (src/commit.rs) --------------------------------------------------------------------
    def commit(self, x, r):
        """CommitmentKey::commit (commit.rs:88-128) with caller-supplied r: (c, ok)."""
        B = self._shape(x, self.l, self.N)
        if self._shape(r, self.k, self.N) != B:
            raise ValueError("commit: batch / shape mismatch (commit.rs:95)")
        lead = tuple(x.shape[:-2])
        c = self._empty(x, lead + (self.n + self.l, self.N))
        ok = self._empty(x, (B,), np.uint8)
        dev, p = self._prep([x, r, c, ok], [np.int64] * 3 + [np.uint8])
        self._check(self._fn("rzk_commit_batch", dev)(self._h, *p, B))
        return c, ok

    def commitment_verify(self, c, x, r, f=None):
        """Commitment::verify (commit.rs:173-210); f = None or one scalar polynomial per opening."""
        B = self._shape(c, self.n + self.l, self.N)
        if self._shape(x, self.l, self.N) != B or self._shape(r, self.k, self.N) != B:
            raise ValueError("commitment_verify: batch / shape mismatch")
        if f is not None and self._shape(f, self.N) != B:
            raise ValueError("commitment_verify: one f per opening")
        ok = self._empty(c, (B,), np.uint8)
        dev, p = self._prep([c, x, r, f, ok], [np.int64] * 4 + [np.uint8])
        self._check(self._fn("rzk_commitment_verify_batch", dev)(self._h, *p, B))
        return ok

    # ---- OpenProof (src/prove/open.rs) -----------------------------------------------------------------------
    def _open_commit(self, name, dt, sym, x, r, y):
        B = self._shape(x, self.l, self.N)
        if self._shape(r, self.k, self.N) != B or self._shape(y, self.k, self.N) != B:
            raise ValueError(f"{name}: batch / shape mismatch (commit.rs:95)")
        lead = tuple(x.shape[:-2])
        c = self._empty(x, lead + (self.n + self.l, self.N), dt)
        t = self._empty(x, lead + (self.n, self.N), dt)
        ok = self._empty(x, (B,), np.uint8)
        dev, p = self._prep([x, r, y, c, t, ok], [dt] * 5 + [np.uint8])
        self._check(self._fn(sym, dev)(self._h, *p, B))
        return c, t, ok

    def _open_response(self, name, dt, sym, y, r, d):
        B = self._shape(y, self.k, self.N)
        if self._shape(r, self.k, self.N) != B or self._shape(d, self.N) != B:
            raise ValueError(f"{name}: batch / shape mismatch")
        z = self._empty(y, tuple(y.shape), dt)
        dev, p = self._prep([y, r, d, z], [dt] * 4)
        self._check(self._fn(sym, dev)(self._h, *p, B))
        return z

    def _open_verify(self, name, dt, sym, z, t, c, d):
        B = self._shape(z, self.k, self.N)
        if (self._shape(t, self.n, self.N) != B or self._shape(c, self.n + self.l, self.N) != B
                or self._shape(d, self.N) != B):
            raise ValueError(f"{name}: batch / shape mismatch")
        acc = self._empty(z, (B,), np.uint8)
        dev, p = self._prep([z, t, c, d, acc], [dt] * 4 + [np.uint8])
        self._check(self._fn(sym, dev)(self._h, *p, B))
        return acc

    def _open_recover(self, name, dt, sym, z, c, d):
        B = self._shape(z, self.k, self.N)
        if self._shape(c, self.n + self.l, self.N) != B or self._shape(d, self.N) != B:
            raise ValueError(f"{name}: batch / shape mismatch")
        t = self._empty(z, tuple(z.shape[:-2]) + (self.n, self.N), dt)
        acc = self._empty(z, (B,), np.uint8)
        dev, p = self._prep([z, c, d, t, acc], [dt] * 4 + [np.uint8])
        self._check(self._fn(sym, dev)(self._h, *p, B))
        return t, acc

    def open_commit(self, x, r, y):
        return self._open_commit("open_commit", np.int64, "rzk_open_commit_batch", x, r, y)

    def open_response(self, y, r, d):
        return self._open_response("open_response", np.int64, "rzk_open_response_batch", y, r, d)

    def open_verify(self, z, t, c, d):
        return self._open_verify("open_verify", np.int64, "rzk_open_verify_batch", z, t, c, d)

    def open_recover(self, z, c, d):
        """The recompute step of a short Open proof (rzk_open_recover_batch): (t, accept) with t = a1.z - c1 (.) d, the
        only t for which open_verify's equation holds; accept[b] = norm rule on z and every coefficient read canonical."""
        return self._open_recover("open_recover", np.int64, "rzk_open_recover_batch", z, c, d)

    # ---- 32-bit coefficient slabs (include/rzk.h "32-bit slabs", v14) ------------------------------------------
    # The same values as int32: numpy int32 arrays or torch int32 tensors.  The methods above keep rejecting int32.
    def narrow(self, a):
        """int64 slab -> int32 slab; a non-canonical coefficient is an input fault of the call (host arrays: raises;
        device tensors: the sticky condition, reported by synchronize())."""
        count = self._shape(a, self.N)
        out = self._empty(a, tuple(a.shape), np.int32)
        dev, p = self._prep([a, out], [np.int64, np.int32])
        self._check(self._fn("rzk_narrow_batch", dev)(self._h, *p, count))
        return out

    def widen(self, a):
        """int32 slab -> int64 slab (sign extension; the consuming call tests the range)."""
        count = self._shape(a, self.N)
        out = self._empty(a, tuple(a.shape), np.int64)
        dev, p = self._prep([a, out], [np.int32, np.int64])
        self._check(self._fn("rzk_widen_batch", dev)(self._h, *p, count))
        return out

    def open_commit32(self, x, r, y):
        return self._open_commit("open_commit32", np.int32, "rzk_open_commit32_batch", x, r, y)

    def open_response32(self, y, r, d):
        return self._open_response("open_response32", np.int32, "rzk_open_response32_batch", y, r, d)

    def open_verify32(self, z, t, c, d):
        return self._open_verify("open_verify32", np.int32, "rzk_open_verify32_batch", z, t, c, d)

    def open_recover32(self, z, c, d):
        return self._open_recover("open_recover32", np.int32, "rzk_open_recover32_batch", z, c, d)

    def eq32(self, a, b):
        """eq[b] = 1 iff the int32 blocks a[b], b[b] ([rows][N]) are equal word for word (rzk_eq32_batch); no range test,
        unlike eq: the verdict of the call that read or wrote the slabs has tested them."""
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError("eq32: shape mismatch")
        rows = int(a.shape[-2])
        B = self._shape(a, rows, self.N)
        out = self._empty(a, (B,), np.uint8)
        dev, p = self._prep([a, b, out], [np.int32, np.int32, np.uint8])
        self._check(self._fn("rzk_eq32_batch", dev)(self._h, p[0], p[1], rows, p[2], B))
        return out

    # ---- the zero-knowledge Open prover on int32 slabs (include/rzk.h "slab32 prover") -----------------
    def sample_uniform_keyed32(self, nonce: bytes, stream: int, bound: int, lead):
        """sample_uniform_keyed as an int32 tensor: the same stream, the same values."""
        return self._sample_keyed(np.int32, "rzk_sample_uniform_keyed32_dev", nonce, stream, (bound,), lead)

    def sample_gauss_keyed32(self, nonce: bytes, stream: int, sigma: float, lead):
        """sample_gauss_keyed as an int32 tensor."""
        return self._sample_keyed(np.int32, "rzk_sample_gauss_keyed32_dev", nonce, stream, (float(sigma),), lead)

    def sample_dgauss_keyed32(self, nonce: bytes, stream: int, sigma: int, lead):
        """sample_dgauss_keyed as an int32 tensor."""
        return self._sample_dgauss_keyed("sample_dgauss_keyed32", np.int32, "rzk_sample_dgauss_keyed32_dev", nonce, stream, sigma, lead)

    def sample_challenge_keyed32(self, nonce: bytes, stream: int, lead):
        """sample_challenge_keyed as an int32 tensor."""
        return self._sample_keyed(np.int32, "rzk_sample_challenge_keyed32_dev", nonce, stream, (), lead)

    def matvec32(self, which: int, v, addend=None):
        """matvec on int32 slabs (rzk_matvec32_batch): narrow() of matvec's output."""
        return self._matvec("matvec32", np.int32, "rzk_matvec32_batch", which, v, addend)

    def open_response_reject32(self, y, r, d, coin, R: int, lnM: float):
        """open_response_reject on int32 slabs y, r, d (coin stays int64): (z int32, accept, E), z = narrow() of the
        sibling's and accept, E byte for byte the sibling's."""
        return self._open_response_reject("open_response_reject32", np.int32, "rzk_open_response_reject32_batch", y, r, d, coin, R, lnM)

    # ---- the prover loop inside the library (include/rzk.h "prover loop") -------------------------------
    def _open_prove_zk(self, name, dt, x, nonce0, stream, gauss_kind, aux, max_rounds):
        B = self._shape(x, self.l, self.N)
        if x.ndim != 3:
            raise ValueError(f"{name}: x must be [B, l, N]")
        if aux is not None:
            aux = bytes(aux)
            if len(aux) != 32:
                raise ValueError("aux must be 32 bytes")
            aux = (C.c_uint8 * 32).from_buffer_copy(aux)
        c = self._empty(x, (B, self.n + self.l, self.N), dt)
        t = self._empty(x, (B, self.n, self.N), dt)
        z = self._empty(x, (B, self.k, self.N), dt)
        r = self._empty(x, (B, self.k, self.N), dt)
        ok = self._empty(x, (B,), np.uint8)
        rounds = self._empty(x, (B,), np.uint8)
        ran = C.c_uint32(0)
        dev, p = self._prep([x, c, t, z, r, ok, rounds], [dt] * 5 + [np.uint8] * 2)
        self._check(self._fn(name, dev)(self._h, p[0], self._nonce(nonce0), int(stream), int(gauss_kind), aux, int(max_rounds),
                                        *p[1:], C.byref(ran), B))
        return c, t, z, ok, r, rounds, int(ran.value)

    def open_prove_zk(self, x, nonce0: bytes, stream: int = 0, gauss_kind: int = 0, aux=None, max_rounds: int = 64):
        """The zero-knowledge Open prover with its rejection loop inside the library (rzk_open_prove_zk_batch[_dev]):
        x [B, l, N] int64 -> (c, t, z, ok, r, rounds, rounds_run).  r, y and the coins are drawn by the keyed samplers under
        the context's sampler key and the nonces nonce0, nonce0 + 1, ... (1 + 3 rounds_run of them); gauss_kind 0 is the
        Box-Muller sampler, 1 the exact discrete Gaussian.  numpy in, numpy out (host form); torch CUDA in, torch out."""
        return self._open_prove_zk("rzk_open_prove_zk_batch", np.int64, x, nonce0, stream, gauss_kind, aux, max_rounds)

    def open_prove_zk32(self, x, nonce0: bytes, stream: int = 0, gauss_kind: int = 0, aux=None, max_rounds: int = 64):
        """open_prove_zk on int32 slabs (rzk_open_prove_zk32_batch[_dev]): c, t, z, r are int32."""
        return self._open_prove_zk("rzk_open_prove_zk32_batch", np.int32, x, nonce0, stream, gauss_kind, aux, max_rounds)

    # ---- Linear and Sum: the y-only half of the commit step and the prover loops -------------------------
    def _linear_mask(self, name, dt, sym, g, y, yp):
        B = self._shape(y, self.k, self.N)
        if self._shape(yp, self.k, self.N) != B or self._shape(g, self.N) != B:
            raise ValueError(f"{name}: batch / shape mismatch")
        lead = tuple(y.shape[:-2])
        t = self._empty(y, lead + (self.n, self.N), dt)
        tp = self._empty(y, lead + (self.n, self.N), dt)
        u = self._empty(y, lead + (self.l, self.N), dt)
        dev, p = self._prep([g, y, yp, t, tp, u], [dt] * 6)
        self._check(self._fn(sym, dev)(self._h, *p, B))
        return t, tp, u

    def linear_mask(self, g, y, yp):
        """The part of linear_commit that depends on y alone (rzk_linear_mask_batch[_dev]): (t, tp, u), byte for byte what
        linear_commit returns for the same g, y, yp."""
        return self._linear_mask("linear_mask", np.int64, "rzk_linear_mask_batch", g, y, yp)

    def sum_mask(self, gs, ys, yp):
        """The part of sum_commit that depends on ys, yp alone (rzk_sum_mask_batch[_dev]): (ts, tp, u)."""
        V = int(gs.shape[-2])
        if V == 0:
            raise ValueError("sum_mask: gs must not be empty (sum.rs:105)")
        B = self._shape(gs, V, self.N)
        if self._shape(ys, V, self.k, self.N) != B or self._shape(yp, self.k, self.N) != B:
            raise ValueError("sum_mask: batch / shape mismatch")
        lead = tuple(gs.shape[:-2])
        ts = self._empty(gs, lead + (V, self.n, self.N))
        tp = self._empty(gs, lead + (self.n, self.N))
        u = self._empty(gs, lead + (self.l, self.N))
        dev, p = self._prep([gs, ys, yp, ts, tp, u], [np.int64] * 6)
        self._check(self._fn("rzk_sum_mask_batch", dev)(self._h, V, *p, B))
        return ts, tp, u

    def _field_prove_zk(self, name, lead_args, ins, shapes, nonce0, stream, gauss_kind, aux, max_rounds):
        """ins: the input slabs; shapes: of the nine int64 outputs, in the C argument order."""
        like = ins[0]
        B = int(like.shape[0])
        if aux is not None:
            aux = bytes(aux)
            if len(aux) != 32:
                raise ValueError("aux must be 32 bytes")
            aux = (C.c_uint8 * 32).from_buffer_copy(aux)
        outs = [self._empty(like, (B,) + tuple(sh)) for sh in shapes]
        ok = self._empty(like, (B,), np.uint8)
        rounds = self._empty(like, (B,), np.uint8)
        ran = C.c_uint32(0)
        dev, p = self._prep(list(ins) + outs + [ok, rounds], [np.int64] * (len(ins) + 9) + [np.uint8] * 2)
        self._check(self._fn(name, dev)(self._h, *lead_args, *p[:len(ins)], self._nonce(nonce0), int(stream), int(gauss_kind), aux,
                                        int(max_rounds), *p[len(ins):], C.byref(ran), B))
        return outs, ok, rounds, int(ran.value)

    def linear_prove_zk(self, g, x, nonce0: bytes, stream: int = 0, gauss_kind: int = 0, aux=None, max_rounds: int = 64):
        """The zero-knowledge Linear prover with its rejection loop inside the library (rzk_linear_prove_zk_batch[_dev]):
        g [B, N], x [B, l, N] -> (c, cp, t, tp, u, z, zp, ok, r, rp, rounds, rounds_run).  The draws use the nonces nonce0,
        nonce0 + 1, ... (2 + 4 rounds_run of them).  numpy in, numpy out (host form); torch CUDA in, torch out."""
        if x.ndim != 3 or self._shape(x, self.l, self.N) != int(x.shape[0]) or tuple(g.shape) != (int(x.shape[0]), self.N):
            raise ValueError("linear_prove_zk: x must be [B, l, N] and g [B, N]")
        n, k, l, N = self.n, self.k, self.l, self.N
        shapes = [(n + l, N), (n + l, N), (n, N), (n, N), (l, N), (k, N), (k, N), (k, N), (k, N)]
        (c, cp, t, tp, u, z, zp, r, rp), ok, rounds, ran = self._field_prove_zk(
            "rzk_linear_prove_zk_batch", (), [g, x], shapes, nonce0, stream, gauss_kind, aux, max_rounds)
        return c, cp, t, tp, u, z, zp, ok, r, rp, rounds, ran

    def sum_prove_zk(self, gs, xs, nonce0: bytes, stream: int = 0, gauss_kind: int = 0, aux=None, max_rounds: int = 64):
        """The zero-knowledge Sum prover with its rejection loop inside the library (rzk_sum_prove_zk_batch[_dev]):
        gs [B, V, N], xs [B, V, l, N] -> (cs, cp, ts, tp, u, zs, zp, ok, rs, rp, rounds, rounds_run)."""
        if xs.ndim != 4 or gs.ndim != 3:
            raise ValueError("sum_prove_zk: xs must be [B, V, l, N] and gs [B, V, N]")
        V = int(xs.shape[1])
        if V == 0:
            raise ValueError("sum_prove_zk: V must be at least 1 (sum.rs:105)")
        if self._shape(xs, V, self.l, self.N) != int(xs.shape[0]) or tuple(gs.shape) != (int(xs.shape[0]), V, self.N):
            raise ValueError("sum_prove_zk: xs must be [B, V, l, N] and gs [B, V, N]")
        n, k, l, N = self.n, self.k, self.l, self.N
        shapes = [(V, n + l, N), (n + l, N), (V, n, N), (n, N), (l, N), (V, k, N), (k, N), (V, k, N), (k, N)]
        (cs, cp, ts, tp, u, zs, zp, rs, rp), ok, rounds, ran = self._field_prove_zk(
            "rzk_sum_prove_zk_batch", (V,), [gs, xs], shapes, nonce0, stream, gauss_kind, aux, max_rounds)
        return cs, cp, ts, tp, u, zs, zp, ok, rs, rp, rounds, ran

    def debug_compact(self, live, done):
        """Diagnostic (rzk_debug_compact_dev): live, done uint8 [B] (torch CUDA) -> (idx uint32-as-int32 [B], count [1]):
        idx[:count] are the ascending b with live[b] and not done[b]; idx[count:] is not written (it keeps the -1 fill)."""
        import torch

        B = int(live.shape[0])
        dev, p = self._prep([live, done], [np.uint8] * 2)
        if not dev:
            raise ValueError("debug_compact takes torch CUDA tensors")
        idx = torch.full((max(B, 1),), -1, dtype=torch.int32, device=live.device)
        count = torch.full((1,), -1, dtype=torch.int32, device=live.device)
        self._check(self._L.rzk_debug_compact_dev(self._h, p[0], p[1], B, C.c_void_p(idx.data_ptr()), C.c_void_p(count.data_ptr())))
        return idx[:B], count

    # ---- LinearProof (src/prove/linear.rs) ------------------------------------------------------------------------
    # (written once over the dtype of the slabs, as the Open methods: the int32 forms are linear_*32 below)
    def _linear_commit(self, name, dt, sym, g, x, r, rp, y, yp):
        B = self._shape(x, self.l, self.N)
        for a, rows in ((r, self.k), (rp, self.k), (y, self.k), (yp, self.k)):
            if self._shape(a, rows, self.N) != B:
                raise ValueError(f"{name}: batch / shape mismatch")
        if self._shape(g, self.N) != B:
            raise ValueError(f"{name}: batch / shape mismatch")
        lead = tuple(x.shape[:-2])
        c = self._empty(x, lead + (self.n + self.l, self.N), dt)
        cp = self._empty(x, lead + (self.n + self.l, self.N), dt)
        t = self._empty(x, lead + (self.n, self.N), dt)
        tp = self._empty(x, lead + (self.n, self.N), dt)
        u = self._empty(x, lead + (self.l, self.N), dt)
        ok = self._empty(x, (B,), np.uint8)
        dev, p = self._prep([g, x, r, rp, y, yp, c, cp, t, tp, u, ok], [dt] * 11 + [np.uint8])
        self._check(self._fn(sym, dev)(self._h, *p, B))
        return c, cp, t, tp, u, ok

    def _linear_response(self, name, dt, sym, y, yp, r, rp, d):
        B = self._shape(y, self.k, self.N)
        z = self._empty(y, tuple(y.shape), dt)
        zp = self._empty(y, tuple(y.shape), dt)
        dev, p = self._prep([y, yp, r, rp, d, z, zp], [dt] * 7)
        self._check(self._fn(sym, dev)(self._h, *p, B))
        return z, zp

    def _linear_verify(self, name, dt, sym, z, zp, c, cp, g, t, tp, u, d):
        B = self._shape(z, self.k, self.N)
        acc = self._empty(z, (B,), np.uint8)
        dev, p = self._prep([z, zp, c, cp, g, t, tp, u, d, acc], [dt] * 9 + [np.uint8])
        self._check(self._fn(sym, dev)(self._h, *p, B))
        return acc

    def _linear_recover(self, name, dt, sym, z, zp, c, cp, g, d):
        B = self._shape(z, self.k, self.N)
        if (self._shape(zp, self.k, self.N) != B or self._shape(c, self.n + self.l, self.N) != B
                or self._shape(cp, self.n + self.l, self.N) != B or self._shape(g, self.N) != B or self._shape(d, self.N) != B):
            raise ValueError(f"{name}: batch / shape mismatch")
        lead = tuple(z.shape[:-2])
        t = self._empty(z, lead + (self.n, self.N), dt)
        tp = self._empty(z, lead + (self.n, self.N), dt)
        u = self._empty(z, lead + (self.l, self.N), dt)
        acc = self._empty(z, (B,), np.uint8)
        dev, p = self._prep([z, zp, c, cp, g, d, t, tp, u, acc], [dt] * 9 + [np.uint8])
        self._check(self._fn(sym, dev)(self._h, *p, B))
        return t, tp, u, acc

    def linear_commit(self, g, x, r, rp, y, yp):
        return self._linear_commit("linear_commit", np.int64, "rzk_linear_commit_batch", g, x, r, rp, y, yp)

    def linear_response(self, y, yp, r, rp, d):
        return self._linear_response("linear_response", np.int64, "rzk_linear_response_batch", y, yp, r, rp, d)

    def linear_verify(self, z, zp, c, cp, g, t, tp, u, d):
        return self._linear_verify("linear_verify", np.int64, "rzk_linear_verify_batch", z, zp, c, cp, g, t, tp, u, d)

    def linear_recover(self, z, zp, c, cp, g, d):
        """The recompute step of a short Linear proof (rzk_linear_recover_batch): (t, tp, u, accept)."""
        return self._linear_recover("linear_recover", np.int64, "rzk_linear_recover_batch", z, zp, c, cp, g, d)

    # ---- LinearProof on int32 slabs (include/rzk.h "slab32 Linear") -------------------------------------------
    # Every slab is int32 (numpy or torch CUDA); outputs are narrow() of the 64-bit methods' on the widened inputs, ok / accept /
    # E are identical.  The methods above keep rejecting int32.
    def linear_commit32(self, g, x, r, rp, y, yp):
        return self._linear_commit("linear_commit32", np.int32, "rzk_linear_commit32_batch", g, x, r, rp, y, yp)

    def linear_mask32(self, g, y, yp):
        return self._linear_mask("linear_mask32", np.int32, "rzk_linear_mask32_batch", g, y, yp)

    def linear_response32(self, y, yp, r, rp, d):
        return self._linear_response("linear_response32", np.int32, "rzk_linear_response32_batch", y, yp, r, rp, d)

    def linear_response_reject32(self, y, yp, r, rp, d, coin, R: int, lnM: float):
        """linear_response_reject on int32 slabs (coin stays int64): (z, zp int32, accept, E)."""
        return self._linear_response_reject("linear_response_reject32", np.int32, "rzk_linear_response_reject32_batch", y, yp, r, rp,
                                            d, coin, R, lnM)

    def linear_verify32(self, z, zp, c, cp, g, t, tp, u, d):
        return self._linear_verify("linear_verify32", np.int32, "rzk_linear_verify32_batch", z, zp, c, cp, g, t, tp, u, d)

    def linear_recover32(self, z, zp, c, cp, g, d):
        return self._linear_recover("linear_recover32", np.int32, "rzk_linear_recover32_batch", z, zp, c, cp, g, d)

    def norm2_le32(self, v, bound: int):
        """norm2_le on an int32 slab (rzk_norm2_le32_batch): the same verdicts as norm2_le on widen(v)."""
        return self._norm2_le(np.int32, "rzk_norm2_le32_batch", v, bound)

    # ---- SumProof (src/prove/sum.rs) --------------------------------------------------------------------------------
    def sum_commit(self, gs, xs, rs, rp, ys, yp):
        V = int(gs.shape[-2])
        if V == 0:
            raise ValueError("sum_commit: gs must not be empty (sum.rs:105)")
        B = self._shape(gs, V, self.N)
        if (self._shape(xs, V, self.l, self.N) != B or self._shape(rs, V, self.k, self.N) != B
                or self._shape(ys, V, self.k, self.N) != B or self._shape(rp, self.k, self.N) != B
                or self._shape(yp, self.k, self.N) != B):
            raise ValueError("sum_commit: gs.len() != xs.len() or shape mismatch (sum.rs:105)")
        lead = tuple(gs.shape[:-2])
        cs = self._empty(gs, lead + (V, self.n + self.l, self.N))
        cp = self._empty(gs, lead + (self.n + self.l, self.N))
        ts = self._empty(gs, lead + (V, self.n, self.N))
        tp = self._empty(gs, lead + (self.n, self.N))
        u = self._empty(gs, lead + (self.l, self.N))
        ok = self._empty(gs, (B,), np.uint8)
        dev, p = self._prep([gs, xs, rs, rp, ys, yp, cs, cp, ts, tp, u, ok], [np.int64] * 11 + [np.uint8])
        self._check(self._fn("rzk_sum_commit_batch", dev)(self._h, V, *p, B))
        return cs, cp, ts, tp, u, ok

    def sum_response(self, ys, yp, rs, rp, d):
        V = int(ys.shape[-3])
        B = self._shape(ys, V, self.k, self.N)
        zs = self._empty(ys, tuple(ys.shape))
        zp = self._empty(yp, tuple(yp.shape))
        dev, p = self._prep([ys, yp, rs, rp, d, zs, zp], [np.int64] * 7)
        self._check(self._fn("rzk_sum_response_batch", dev)(self._h, V, *p, B))
        return zs, zp

    def sum_verify(self, zs, zp, cs, cp, gs, ts, tp, u, d):
        V = int(zs.shape[-3])
        B = self._shape(zs, V, self.k, self.N)
        acc = self._empty(zs, (B,), np.uint8)
        dev, p = self._prep([zs, zp, cs, cp, gs, ts, tp, u, d, acc], [np.int64] * 9 + [np.uint8])
        self._check(self._fn("rzk_sum_verify_batch", dev)(self._h, V, *p, B))
        return acc

    def sum_recover(self, zs, zp, cs, cp, gs, d):
        """The recompute step of a short Sum proof (rzk_sum_recover_batch): (ts, tp, u, accept)."""
        V = int(zs.shape[-3])
        if V == 0:
            raise ValueError("sum_recover: zs must not be empty")
        B = self._shape(zs, V, self.k, self.N)
        if (self._shape(zp, self.k, self.N) != B or self._shape(cs, V, self.n + self.l, self.N) != B
                or self._shape(cp, self.n + self.l, self.N) != B or self._shape(gs, V, self.N) != B
                or self._shape(d, self.N) != B):
            raise ValueError("sum_recover: batch / shape mismatch")
        lead = tuple(zs.shape[:-3])
        ts = self._empty(zs, lead + (V, self.n, self.N))
        tp = self._empty(zs, lead + (self.n, self.N))
        u = self._empty(zs, lead + (self.l, self.N))
        acc = self._empty(zs, (B,), np.uint8)
        dev, p = self._prep([zs, zp, cs, cp, gs, d, ts, tp, u, acc], [np.int64] * 9 + [np.uint8])
        self._check(self._fn("rzk_sum_recover_batch", dev)(self._h, V, *p, B))
        return ts, tp, u, acc


def reject_lnm(alpha: float) -> float:
    """ln M = 12 / alpha + 1 / (2 alpha^2) of the rejection step for sigma = alpha |d r|_2 (rzk_reject_lnm)."""
    return float(_lib.lib().rzk_reject_lnm(float(alpha)))


class SeededSampler:
    """The interface of KeyedSampler over the seeded (Philox) samplers: for tests and benchmarks, NOT for proofs anyone
    relies on.  Every draw takes the next stream id under `seed`, so a sampler made again from the same seed repeats
    the same sequence of draws."""

    def __init__(self, ctx: Context, seed: int, stream0: int = 0):
        self.ctx = ctx
        self.seed = int(seed)
        self.stream = int(stream0)

    def _next_stream(self) -> int:
        if self.stream >= 1 << 32:
            raise OverflowError("the stream counter is exhausted: use another seed")
        self.stream += 1
        return self.stream - 1

    def uniform(self, bound: int, lead):
        return self.ctx.sample_uniform(self.seed, self._next_stream(), bound, lead)

    def gauss(self, sigma: float, lead):
        return self.ctx.sample_gauss(self.seed, self._next_stream(), sigma, lead)

    def challenge(self, lead):
        return self.ctx.sample_challenge(self.seed, self._next_stream(), lead)


class KeyedSampler:
    """Prover / verifier randomness from the keyed (ChaCha20) device samplers, one fresh nonce per draw.

    The nonce is a 128-bit little-endian counter starting at `nonce0`; `uniform`, `gauss` and `challenge` each consume
    its next value, so a program cannot use a (key, nonce) pair twice by accident.  key = None takes 32 bytes from
    os.urandom; a given key plus nonce0 make a run reproducible (tests).  The key is installed in `ctx`: one sampler
    per context at a time."""

    STREAM = 0
    GAUSS_KIND = 0   # what `gauss` draws, as rzk_open_prove_zk_batch names it: the Box-Muller sampler

    def __init__(self, ctx: Context, key: Optional[bytes] = None, nonce0: int = 0):
        import os

        if not 0 <= nonce0 < 1 << 128:
            raise ValueError("nonce0 must fit 128 bits")
        self.ctx = ctx
        self.counter = nonce0
        ctx.set_sampler_key(os.urandom(32) if key is None else key)

    def _next_nonce(self) -> bytes:
        if self.counter >= 1 << 128:
            raise OverflowError("the nonce counter is exhausted: install a new key")
        nonce = self.counter.to_bytes(16, "little")
        self.counter += 1
        return nonce

    def take_nonces(self, n: int) -> bytes:
        """The current counter as 16 bytes, for a call that draws under n consecutive nonces itself (Context.open_prove_zk);
        the counter advances by n.  Every nonce handed out stays below 2^128, as in _next_nonce."""
        if n < 0:
            raise ValueError("take_nonces: n must not be negative")
        if self.counter + max(n, 1) > 1 << 128:
            raise OverflowError("the nonce counter is exhausted: install a new key")
        nonce = self.counter.to_bytes(16, "little")
        self.counter += n
        return nonce

    def uniform(self, bound: int, lead):
        return self.ctx.sample_uniform_keyed(self._next_nonce(), self.STREAM, bound, lead)

    def gauss(self, sigma: float, lead):
        return self.ctx.sample_gauss_keyed(self._next_nonce(), self.STREAM, sigma, lead)

    def challenge(self, lead):
        return self.ctx.sample_challenge_keyed(self._next_nonce(), self.STREAM, lead)


class ExactKeyedSampler(KeyedSampler):
    """KeyedSampler whose `gauss` draws from the exact discrete Gaussian D_sigma (Context.sample_dgauss_keyed, DESIGN
    §15) instead of the truncated Box-Muller normal: the y that the provers' rejection step assumes.  sigma must be
    integral (the library's sigma = 11 kappa beta sqrt(kN) is rounded by rzk_sigma).  Nonces, uniform and challenge
    draws are KeyedSampler's."""

    GAUSS_KIND = 1

    def gauss(self, sigma, lead):
        if int(sigma) != sigma:
            raise ValueError("ExactKeyedSampler.gauss: sigma must be an integer")
        return self.ctx.sample_dgauss_keyed(self._next_nonce(), self.STREAM, int(sigma), lead)


class KeyedSampler32(KeyedSampler):
    """KeyedSampler whose draws are int32 tensors (Context.sample_*_keyed32).  Same key, nonce counter and
    streams: a KeyedSampler32 and a KeyedSampler made with the same key and nonce0 consume nonces identically and
    return the same values in two widths."""

    def uniform(self, bound: int, lead):
        return self.ctx.sample_uniform_keyed32(self._next_nonce(), self.STREAM, bound, lead)

    def gauss(self, sigma: float, lead):
        return self.ctx.sample_gauss_keyed32(self._next_nonce(), self.STREAM, sigma, lead)

    def challenge(self, lead):
        return self.ctx.sample_challenge_keyed32(self._next_nonce(), self.STREAM, lead)


class ExactKeyedSampler32(KeyedSampler32):
    """ExactKeyedSampler on int32 tensors: `gauss` draws from the exact discrete Gaussian (Context.sample_dgauss_keyed32)."""

    GAUSS_KIND = 1

    def gauss(self, sigma, lead):
        if int(sigma) != sigma:
            raise ValueError("ExactKeyedSampler32.gauss: sigma must be an integer")
        return self.ctx.sample_dgauss_keyed32(self._next_nonce(), self.STREAM, int(sigma), lead)
