/*
 * rzk.h — C ABI of the MI355X (gfx950) polynomial-ring backend for ring-zk.
 *
 * The reference crate (AlvinHon/ring-zk, /root/reference) has no plugin / FFI seam: all ring
 * arithmetic of its protocols flows through four crate-private methods of `Mat`
 * (src/mat.rs:95-178), one direct `Polynomial::mul` (src/prove/linear.rs:94) and the norm
 * predicates of `Params` (src/params.rs:102-118).  This header is the boundary a thin Rust shim
 * binds at exactly those places (INTEGRATION.md shows the `extern "C"` block and the replaced
 * function bodies).  Each entry point below cites the reference code it replaces.
 *
 * Conventions
 *   - A polynomial is N int64 coefficients, each the centred representative in
 *     [-(q-1)/2, (q-1)/2] (what ZqI64<Q> stores; src/params.rs:122-126); outputs always are.  The reference's
 *     type guarantees this for its own values (ZqI64::from reduces, src/params.rs:126); data from elsewhere
 *     (the wire, another library) may not be, so EVERY coefficient a kernel loads is tested while it is loaded
 *     (all 64 bits: k*2^32 + s is never read as s).  A violation
 *       - in a verifier-side entry point (rzk_*_verify_batch, rzk_commitment_verify_batch) clears the verdict of
 *         the offending proof (accept / ok = 0) and the call succeeds: a malformed proof is a rejected proof;
 *       - anywhere else (Mat primitives, commit / response phases) makes the call fail with RZK_E_ARG (the
 *         host-pointer variants at return, the *_dev variants at the next rzk_ctx_synchronize /
 *         rzk_ctx_check_inputs); per-proof ok flags of the offending proofs are cleared as well, outputs of
 *         those proofs are unspecified.  rzk_canonicalize_batch reduces foreign data first (= ZqI64::from);
 *         rzk_wire_mat_decode rejects out-of-range coefficients when given q.
 *   - Slabs are dense row-major: [batch][row][N].  A "batch" is B independent proofs that share
 *     only the commitment key.
 *   - Every function returns 0 (RZK_OK) or a negative status; nothing aborts.  The Rust shim turns
 *     a non-zero status into panic!, preserving the reference's assert!/assert_eq! behaviour on
 *     shape mismatch (src/mat.rs:103,129-130,154-155; src/commit.rs:95; src/prove/sum.rs:105).
 *   - `*_dev` variants take device pointers and are asynchronous on the context's HIP stream;
 *     the variants without the suffix take host pointers, copy in/out and are synchronous.
 *   - One context per (GPU, host thread); calls on a context are serialised on its stream.
 *   - The library never falls back to a CPU path: without a usable HIP device rzk_ctx_create fails.
 */
#ifndef RZK_H
#define RZK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RZK_OK 0
#define RZK_E_ARG (-1)         /* bad argument / shape mismatch (reference: assert panic)        */
#define RZK_E_HIP (-2)         /* HIP runtime error, see rzk_last_error                           */
#define RZK_E_STATE (-3)       /* e.g. key not loaded                                             */
#define RZK_E_UNSUPPORTED (-4) /* ring degree / modulus / shape outside what the kernels support */

typedef struct rzk_ctx rzk_ctx;

/* Version of this C ABI: bumped whenever an existing signature changes (rzk_wire_mat_decode gained `q` in 2,
 * version 3 added the entry points marked "v3", version 4 those marked "v4", version 5 those marked "v5", version 6 those marked "v6", version 7 those marked "v7", version 8 those marked "v8", version 9 those marked "v9", version 10 those marked "v10", version 11 those marked "v11", version 12 those marked "v12", version 13 those marked "v13", version 14 those marked "v14").  A binding checks rzk_abi_version() == RZK_ABI_VERSION after loading
 * the library, so that a stale or variant .so fails at load time instead of reading shifted arguments. */
#define RZK_ABI_VERSION 14u
uint32_t rzk_abi_version(void);

/* Which block of the commitment key a matrix-vector product uses (src/commit.rs:19-25). */
#define RZK_KEY_A1 0 /* a1: n x k        (rows 0..n-1 of [a1;a2])  */
#define RZK_KEY_A2 1 /* a2: l x k        (rows n..n+l-1)           */
#define RZK_KEY_A 2  /* [a1;a2]: (n+l) x k, as built at src/commit.rs:109-114 */

/* ---- context ---------------------------------------------------------------------------------- */
/* Mirrors Params<ZqI64<Q>> (src/params.rs:18-36) + const generics N and Q.
 * q: ring modulus Q, NOT Params.q: odd, 1073692673 < q <= 4294606851 (above the first auxiliary NTT prime,
 *    (q-1)/2 below twice the third; the default 3515337053, src/params.rs:121, lies inside), else RZK_E_UNSUPPORTED.
 *    Both ends of the range, the moduli either side of 2^30 and 2^31 + 1 are pinned by tests/test_emul_modq.py (the
 *    lane arithmetic, CPU) and tests/test_gpu_moduli.py (every kernel family against the oracle).
 * N: power of two in [4, 2048].  512 / 1024 / 2048 run the NTT kernels (the BASELINE sizes); 4 .. 256
 * (the sizes of the reference's own tests: src/mat.rs:241 N=4, tests/test.rs:8 N=16) run a schoolbook
 * kernel, same results, for drop-in completeness.  Requires k > n >= 1, l >= 1, n + l <= k
 * (src/params.rs:26-31).
 * device: HIP device ordinal. */
int rzk_ctx_create(rzk_ctx** out, int64_t q, uint32_t N, uint32_t n, uint32_t k, uint32_t l,
                   uint32_t kappa, uint64_t b, int device);
void rzk_ctx_destroy(rzk_ctx* ctx);
/* Run on a caller-owned hipStream_t (e.g. PyTorch's current stream); NULL selects HIP's default
 * (null) stream.  rzk_ctx_use_own_stream goes back to the private stream created with the context. */
int rzk_ctx_set_stream(rzk_ctx* ctx, void* hip_stream);
int rzk_ctx_use_own_stream(rzk_ctx* ctx);
/* v3.  Trusted-producer mode, default OFF.  With on != 0 the caller vouches that every coefficient later calls on this
 * context load is canonical — written by this library on this device (commitments, t, responses, sampler outputs), or
 * validated before (rzk_canonicalize_batch, rzk_wire_mat_decode with q) — and the kernels skip the per-coefficient
 * range test (3 vector instructions per loaded coefficient).  Norm predicates, the norm measurements that fix the
 * prime count, and therefore the results on canonical data are unchanged; on non-canonical data the results are
 * unspecified.  A verifier that receives z, t, c from elsewhere leaves this off (reference: ZqI64::from,
 * src/params.rs:126, makes every value canonical by construction).  Synchronises the stream. */
int rzk_ctx_trust_device_outputs(rzk_ctx* ctx, int on);
/* Waits for the context's stream.  Also the point where the asynchronous *_dev calls report non-canonical input
 * coefficients (see "Conventions"): RZK_E_ARG once, then the condition is cleared.  rzk_ctx_check_inputs is the
 * same call under the name a caller uses when it only wants that verdict. */
int rzk_ctx_synchronize(rzk_ctx* ctx);
int rzk_ctx_check_inputs(rzk_ctx* ctx);
/* Ordering rule for mixed use: a host-pointer call reports only its OWN input faults — it clears the sticky condition
 * when it starts.  A caller of *_dev entry points that wants their verdict must therefore ask for it
 * (rzk_ctx_check_inputs / rzk_ctx_synchronize) before its next host-pointer call on the same context. */
/* Message of the last failure on this context; with ctx == NULL, of the last failed rzk_ctx_create. */
const char* rzk_last_error(const rzk_ctx* ctx);
/* sigma, 4*sigma*floor(sqrt N), 2*sigma*floor(sqrt N)   (src/params.rs:94-98,104,114) */
uint64_t rzk_sigma(const rzk_ctx* ctx);
uint64_t rzk_commit_bound(const rzk_ctx* ctx);
uint64_t rzk_verify_bound(const rzk_ctx* ctx);

/* ---- key ----------------------------------------------------------------------------------------- */
/* CommitmentKey (src/commit.rs:19-25): a = [a1;a2], (n+l)*k polynomials row-major, exactly the
 * matrix commit() assembles at src/commit.rs:109-114 (identity / zero blocks included).  The key is
 * transformed once into the NTT domain of the three auxiliary primes and kept resident in HBM;
 * entries equal to 0 or 1 are recognised and skipped / turned into plain additions.
 * What a failed load leaves behind (rzk_key_load, rzk_key_load_dev, and rzk_key_generate / rzk_key_expand, which load
 * through the same path once their polynomials are drawn):
 *   - a load that returns RZK_E_ARG (a coefficient outside [-(q-1)/2, (q-1)/2], a NULL argument) leaves the previous key
 *     and every later result exactly as if the call had not been made: the key is tested as a whole, on the host, before
 *     anything of the context changes;
 *   - so does a failure before the key has been tested: selecting the device, the device-to-host copy of
 *     rzk_key_load_dev, drawing the polynomials of rzk_key_generate / rzk_key_expand;
 *   - any failure after the key has been accepted (allocation, transform, digest: RZK_E_HIP ...) leaves the context
 *     without a key: every later call that needs one returns RZK_E_STATE until a load succeeds, never a mixture of two
 *     keys. */
int rzk_key_load(rzk_ctx* ctx, const int64_t* a_host);
int rzk_key_load_dev(rzk_ctx* ctx, const int64_t* a_dev);
/* CommitmentKey::new (src/commit.rs:33-60) with the device-side sampler: a1 = [I_n | U], a2 = [0 | I_l | U],
 * U uniform over [-(q-1)/2, (q-1)/2] (src/params.rs:126), drawn from (seed); the key is loaded and, when
 * a_host_out != NULL, also returned ([n+l][k][N], the public key material).  Statistical parity (see samplers). */
int rzk_key_generate(rzk_ctx* ctx, uint64_t seed, int64_t* a_host_out);
/* v10.  CommitmentKey::new (src/commit.rs:33-60) as a public function of a 32-byte seed, the way Dilithium and Kyber derive
 * A = ExpandA(rho): the structure of rzk_key_generate, a1 = [I_n | a1'], a2 = [0 | I_l | a2'], where the general entry at row i,
 * column j of the (n+l) x k matrix is polynomial p = i*k + j of the "XP1" expansion below under domain RZK_XOF_DOMAIN_KEY and
 * `seed`.  The index is the position, so a verifier can recompute one entry alone, and the seed is all that has to be stored,
 * sent or pinned.  The polynomials are produced on the device; the key is loaded through the path of rzk_key_load
 * (classification, transform, FS1 key digest) and, when a_host_out != NULL, also returned ([n+l][k][N]). */
int rzk_key_expand(rzk_ctx* ctx, const uint8_t seed[32], int64_t* a_host_out);

/* ---- ring / Mat primitives (the Mat seam) ------------------------------------------------------------ */
/* Polynomial::mul (src/prove/linear.rs:94; src/mat.rs:110,176): out[i] = a[i] * b[i], count polys */
int rzk_polymul_batch(rzk_ctx* ctx, const int64_t* a, const int64_t* b, int64_t* out, size_t count);
int rzk_polymul_batch_dev(rzk_ctx* ctx, const int64_t* a, const int64_t* b, int64_t* out, size_t count);
/* Mat::dot with the key on the left (src/mat.rs:95-115; call sites src/commit.rs:125,
 * src/prove/open.rs:97,171 ...): out[b] = KEY(which) . v[b] (+ addend[b] when addend != NULL, the
 * `.add(&z)` of src/commit.rs:125).  v: [B][k][N]; out, addend: [B][rows(which)][N]. */
int rzk_matvec_batch(rzk_ctx* ctx, int which, const int64_t* v, const int64_t* addend, int64_t* out,
                     size_t B);
int rzk_matvec_batch_dev(rzk_ctx* ctx, int which, const int64_t* v, const int64_t* addend,
                         int64_t* out, size_t B);
/* Mat::componentwise_mul (src/mat.rs:168-178): out[b][i] = m[b][i] * p[b].  m,out: [B][rows][N]; p: [B][N] */
int rzk_cmul_batch(rzk_ctx* ctx, const int64_t* m, uint32_t rows, const int64_t* p, int64_t* out, size_t B);
int rzk_cmul_batch_dev(rzk_ctx* ctx, const int64_t* m, uint32_t rows, const int64_t* p, int64_t* out,
                       size_t B);
/* Any int64 coefficient -> the centred representative in [-(q-1)/2, (q-1)/2] (what ZqI64::from does,
 * src/params.rs:126).  Every other entry point rejects non-canonical inputs (see Conventions); data that did not
 * pass through a ZqI64 goes through this first.  in, out: [count][N], may alias. */
int rzk_canonicalize_batch(rzk_ctx* ctx, const int64_t* in, int64_t* out, size_t count);
int rzk_canonicalize_batch_dev(rzk_ctx* ctx, const int64_t* in, int64_t* out, size_t count);
/* Mat::add / Mat::sub (src/mat.rs:122-140, 147-165) on `count` polynomials */
int rzk_add_batch(rzk_ctx* ctx, const int64_t* a, const int64_t* b, int64_t* out, size_t count);
int rzk_add_batch_dev(rzk_ctx* ctx, const int64_t* a, const int64_t* b, int64_t* out, size_t count);
int rzk_sub_batch(rzk_ctx* ctx, const int64_t* a, const int64_t* b, int64_t* out, size_t count);
int rzk_sub_batch_dev(rzk_ctx* ctx, const int64_t* a, const int64_t* b, int64_t* out, size_t count);
/* Params::check_{commit,verify}_constraint (src/params.rs:102-118 -> src/polynomial.rs:60-73):
 * ok[b] = 1 iff every one of the `rows` polynomials of proof b has floor(sqrt(sum c^2)) <= bound */
int rzk_norm2_le_batch(rzk_ctx* ctx, const int64_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B);
int rzk_norm2_le_batch_dev(rzk_ctx* ctx, const int64_t* v, uint32_t rows, uint64_t bound, uint8_t* ok,
                           size_t B);
/* derived Mat PartialEq (src/mat.rs:11; `lhs == rhs` at src/prove/open.rs:173): eq[b] = all rows equal */
int rzk_eq_batch(rzk_ctx* ctx, const int64_t* a, const int64_t* b, uint32_t rows, uint8_t* eq, size_t B);
int rzk_eq_batch_dev(rzk_ctx* ctx, const int64_t* a, const int64_t* b, uint32_t rows, uint8_t* eq, size_t B);

/* ---- batched transforms over one auxiliary prime (no reference counterpart) ---------- */
/* in/out: `count` residue polynomials of N uint32 in [0,p).  Forward output / inverse input use the
 * library's NTT-domain layout (rzk_ntt_layout_index).  prime: 0..2. */
int rzk_ntt_forward_batch(rzk_ctx* ctx, int prime, const uint32_t* in, uint32_t* out, size_t count);
int rzk_ntt_forward_batch_dev(rzk_ctx* ctx, int prime, const uint32_t* in, uint32_t* out, size_t count);
int rzk_ntt_inverse_batch(rzk_ctx* ctx, int prime, const uint32_t* in, uint32_t* out, size_t count);
int rzk_ntt_inverse_batch_dev(rzk_ctx* ctx, int prime, const uint32_t* in, uint32_t* out, size_t count);
uint32_t rzk_ntt_prime(int prime);
/* primitive 2N-th root of unity used for ring degree N */
uint32_t rzk_ntt_psi(int prime, uint32_t N);
/* position, in the NTT-domain layout, of element j of the standard bit-reversed-order transform */
uint32_t rzk_ntt_layout_index(uint32_t N, uint32_t j);

/* ---- commitment scheme (src/commit.rs) ------------------------------------------------------------------ */
/* CommitmentKey::commit (commit.rs:88-128) with the randomness supplied by the caller:
 * c = [a1;a2].r + [0_n ; x] (commit.rs:109-125); ok[b] = check_commit_constraint(r_b) — the reference
 * resamples r until it holds (commit.rs:98-107), here the caller resamples the proofs with ok == 0.
 * x:[B][l][N] r:[B][k][N] -> c:[B][n+l][N] ok:[B] (ok may be NULL) */
int rzk_commit_batch(rzk_ctx* ctx, const int64_t* x, const int64_t* r, int64_t* c, uint8_t* ok, size_t B);
int rzk_commit_batch_dev(rzk_ctx* ctx, const int64_t* x, const int64_t* r, int64_t* c, uint8_t* ok, size_t B);
/* Commitment::verify (commit.rs:173-210) of the opening (x, r, f):
 * ok[b] = check_commit_constraint(r) && ( f == NULL ?  [a1;a2].r + [0_n;x] == c
 *                                                   :  c (.) f == [a1;a2].r + [0_n;x] (.) f )
 * c:[B][n+l][N] x:[B][l][N] r:[B][k][N] f:[B][N] or NULL (Opening::f = None) -> ok:[B] */
int rzk_commitment_verify_batch(rzk_ctx* ctx, const int64_t* c, const int64_t* x, const int64_t* r,
                                const int64_t* f, uint8_t* ok, size_t B);
int rzk_commitment_verify_batch_dev(rzk_ctx* ctx, const int64_t* c, const int64_t* x, const int64_t* r,
                                    const int64_t* f, uint8_t* ok, size_t B);

/* ---- OpenProof phases (src/prove/open.rs) --------------------------------------------------------- */
/* OpenProofProver::commit (open.rs:80-103) with the randomness supplied by the caller:
 * c = [a1;a2].r + [0;x] (commit.rs:125), t = a1.y (open.rs:97); ok[b] = check_commit_constraint(r)
 * (commit.rs:98-107: the reference resamples r until it holds; here the caller does).
 * x:[B][l][N] r,y:[B][k][N] -> c:[B][n+l][N] t:[B][n][N] ok:[B] */
int rzk_open_commit_batch(rzk_ctx* ctx, const int64_t* x, const int64_t* r, const int64_t* y,
                          int64_t* c, int64_t* t, uint8_t* ok, size_t B);
int rzk_open_commit_batch_dev(rzk_ctx* ctx, const int64_t* x, const int64_t* r, const int64_t* y,
                              int64_t* c, int64_t* t, uint8_t* ok, size_t B);
/* OpenProofProver::create_response (open.rs:107-117): z = y + r (.) d.   d:[B][N] z:[B][k][N] */
int rzk_open_response_batch(rzk_ctx* ctx, const int64_t* y, const int64_t* r, const int64_t* d,
                            int64_t* z, size_t B);
int rzk_open_response_batch_dev(rzk_ctx* ctx, const int64_t* y, const int64_t* r, const int64_t* d,
                                int64_t* z, size_t B);
/* OpenProofVerifier::verify (open.rs:162-174) on the full commitment c (c1 split as
 * Commitment::c1_c2 does, commit.rs:213-218; requires n == l):
 * accept[b] = check_verify_constraint(z) && a1.z == t + c1 (.) d */
int rzk_open_verify_batch(rzk_ctx* ctx, const int64_t* z, const int64_t* t, const int64_t* c,
                          const int64_t* d, uint8_t* accept, size_t B);
int rzk_open_verify_batch_dev(rzk_ctx* ctx, const int64_t* z, const int64_t* t, const int64_t* c,
                              const int64_t* d, uint8_t* accept, size_t B);

/* ---- LinearProof phases (src/prove/linear.rs) -------------------------------------------------------- */
/* commit (linear.rs:82-140): gx = g*x; cp = commit(gx; rp); c = commit(x; r); t = a1.y; tp = a1.yp;
 * u = (a2.y) (.) g - a2.yp.   ok[b]: bit0 = constraint(r), bit1 = constraint(rp).
 * g:[B][N] x:[B][l][N] r,rp,y,yp:[B][k][N] -> c,cp:[B][n+l][N] t,tp:[B][n][N] u:[B][l][N] */
int rzk_linear_commit_batch(rzk_ctx* ctx, const int64_t* g, const int64_t* x, const int64_t* r,
                            const int64_t* rp, const int64_t* y, const int64_t* yp, int64_t* c,
                            int64_t* cp, int64_t* t, int64_t* tp, int64_t* u, uint8_t* ok, size_t B);
int rzk_linear_commit_batch_dev(rzk_ctx* ctx, const int64_t* g, const int64_t* x, const int64_t* r,
                                const int64_t* rp, const int64_t* y, const int64_t* yp, int64_t* c,
                                int64_t* cp, int64_t* t, int64_t* tp, int64_t* u, uint8_t* ok, size_t B);
/* create_response (linear.rs:144-158): z = y + r(.)d, zp = yp + rp(.)d */
int rzk_linear_response_batch(rzk_ctx* ctx, const int64_t* y, const int64_t* yp, const int64_t* r,
                              const int64_t* rp, const int64_t* d, int64_t* z, int64_t* zp, size_t B);
int rzk_linear_response_batch_dev(rzk_ctx* ctx, const int64_t* y, const int64_t* yp, const int64_t* r,
                                  const int64_t* rp, const int64_t* d, int64_t* z, int64_t* zp, size_t B);
/* verify (linear.rs:213-250) */
int rzk_linear_verify_batch(rzk_ctx* ctx, const int64_t* z, const int64_t* zp, const int64_t* c,
                            const int64_t* cp, const int64_t* g, const int64_t* t, const int64_t* tp,
                            const int64_t* u, const int64_t* d, uint8_t* accept, size_t B);
int rzk_linear_verify_batch_dev(rzk_ctx* ctx, const int64_t* z, const int64_t* zp, const int64_t* c,
                                const int64_t* cp, const int64_t* g, const int64_t* t, const int64_t* tp,
                                const int64_t* u, const int64_t* d, uint8_t* accept, size_t B);

/* ---- SumProof phases (src/prove/sum.rs), V summands per proof ----------------------------------------- */
/* commit (sum.rs:99-178).  gs:[B][V][N] xs:[B][V][l][N] rs,ys:[B][V][k][N] rp,yp:[B][k][N]
 * -> cs:[B][V][n+l][N] cp:[B][n+l][N] ts:[B][V][n][N] tp:[B][n][N] u:[B][l][N]; ok[b] = all constraints */
int rzk_sum_commit_batch(rzk_ctx* ctx, uint32_t V, const int64_t* gs, const int64_t* xs,
                         const int64_t* rs, const int64_t* rp, const int64_t* ys, const int64_t* yp,
                         int64_t* cs, int64_t* cp, int64_t* ts, int64_t* tp, int64_t* u, uint8_t* ok,
                         size_t B);
int rzk_sum_commit_batch_dev(rzk_ctx* ctx, uint32_t V, const int64_t* gs, const int64_t* xs,
                             const int64_t* rs, const int64_t* rp, const int64_t* ys, const int64_t* yp,
                             int64_t* cs, int64_t* cp, int64_t* ts, int64_t* tp, int64_t* u,
                             uint8_t* ok, size_t B);
/* create_response (sum.rs:182-200) */
int rzk_sum_response_batch(rzk_ctx* ctx, uint32_t V, const int64_t* ys, const int64_t* yp,
                           const int64_t* rs, const int64_t* rp, const int64_t* d, int64_t* zs,
                           int64_t* zp, size_t B);
int rzk_sum_response_batch_dev(rzk_ctx* ctx, uint32_t V, const int64_t* ys, const int64_t* yp,
                               const int64_t* rs, const int64_t* rp, const int64_t* d, int64_t* zs,
                               int64_t* zp, size_t B);
/* verify (sum.rs:257-320) */
int rzk_sum_verify_batch(rzk_ctx* ctx, uint32_t V, const int64_t* zs, const int64_t* zp,
                         const int64_t* cs, const int64_t* cp, const int64_t* gs, const int64_t* ts,
                         const int64_t* tp, const int64_t* u, const int64_t* d, uint8_t* accept,
                         size_t B);
int rzk_sum_verify_batch_dev(rzk_ctx* ctx, uint32_t V, const int64_t* zs, const int64_t* zp,
                             const int64_t* cs, const int64_t* cp, const int64_t* gs, const int64_t* ts,
                             const int64_t* tp, const int64_t* u, const int64_t* d, uint8_t* accept,
                             size_t B);

/* ---- recompute steps of the short proofs (v12) -----------------------------------------------------------------------------
 * A short proof sends the challenge d in place of the commitment message's t / tp / ts / u (RZK_MSG_OPEN_SHORT,
 * RZK_MSG_LINEAR_SHORT, RZK_MSG_SUM_SHORT below).  These calls are its verifier's first step: the verifiers' own launches
 * with the compared operands as outputs, i.e. the unique values for which the reference's verification equations hold,
 *   open    (open.rs:171-173)     t  = a1.z - c1 (.) d
 *   linear  (linear.rs:224-249)   t  = a1.z - c1 (.) d,  tp = a1.zp - c1p (.) d,  u = g (.) (a2.z - c2 (.) d) - (a2.zp - c2p (.) d)
 *   sum     (sum.rs:277-319)      ts_i = a1.zs_i - c1_i (.) d,  tp = a1.zp - c1p (.) d,
 *                                 u = sum_i g_i (.) (a2.zs_i) - a2.zp - (sum_i c2_i (.) g_i - c2p) (.) d
 * reduced to centred representatives.  The caller then hashes the full commitment message with the recomputed fields
 * (rzk_fs_challenge_batch) and accepts iff that gives d again; the equations hold by construction, so no *_verify pass follows.
 * accept[b] = 1 iff every response vector of proof b passes check_verify_constraint and every coefficient the recompute reads
 * is canonical.  Verifier-side convention: a non-canonical value clears its own proof's verdict and the call succeeds.  Every
 * input is read except, for Open, the rows c2 of c (they are range-tested by the transcript hash that follows).  d is foreign
 * data: the products with it are exact for any canonical d, not only for challenges.  Outputs of a rejected proof are
 * unspecified (but written inside their own rows).  Requires n == l like the verifiers (RZK_E_ARG); B == 0 is a no-op.
 * z,zp:[B][k][N] zs:[B][V][k][N] c,cp:[B][n+l][N] cs:[B][V][n+l][N] g,d:[B][N] gs:[B][V][N]
 * -> t_out,tp_out:[B][n][N] ts_out:[B][V][n][N] u_out:[B][l][N] accept:[B] */
int rzk_open_recover_batch(rzk_ctx* ctx, const int64_t* z, const int64_t* c, const int64_t* d, int64_t* t_out,
                           uint8_t* accept, size_t B);
int rzk_open_recover_batch_dev(rzk_ctx* ctx, const int64_t* z, const int64_t* c, const int64_t* d, int64_t* t_out,
                               uint8_t* accept, size_t B);
int rzk_linear_recover_batch(rzk_ctx* ctx, const int64_t* z, const int64_t* zp, const int64_t* c, const int64_t* cp,
                             const int64_t* g, const int64_t* d, int64_t* t_out, int64_t* tp_out, int64_t* u_out,
                             uint8_t* accept, size_t B);
int rzk_linear_recover_batch_dev(rzk_ctx* ctx, const int64_t* z, const int64_t* zp, const int64_t* c, const int64_t* cp,
                                 const int64_t* g, const int64_t* d, int64_t* t_out, int64_t* tp_out, int64_t* u_out,
                                 uint8_t* accept, size_t B);
int rzk_sum_recover_batch(rzk_ctx* ctx, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                          const int64_t* cp, const int64_t* gs, const int64_t* d, int64_t* ts_out, int64_t* tp_out,
                          int64_t* u_out, uint8_t* accept, size_t B);
int rzk_sum_recover_batch_dev(rzk_ctx* ctx, uint32_t V, const int64_t* zs, const int64_t* zp, const int64_t* cs,
                              const int64_t* cp, const int64_t* gs, const int64_t* d, int64_t* ts_out, int64_t* tp_out,
                              int64_t* u_out, uint8_t* accept, size_t B);

/* ---- instrumentation (bench.py) ------------------------------------------------------------------------- */
/* Times `iters` launches of the batched forward NTT kernel with HIP events on the context stream and
 * returns the average kernel duration in microseconds (negative status on error). */
double rzk_bench_ntt_forward_dev(rzk_ctx* ctx, int prime, const uint32_t* in, uint32_t* out,
                                 size_t count, int iters);
/* ---- device-side samplers ----------------------------------------------------------------------------------- */
/* The distributions of the reference's host RNG helpers, drawn in HBM by a counter-based generator
 * (Philox4x32-10; output = f(seed, stream, polynomial index, position), reproducible and order-independent).
 * Parity with the reference is statistical, not bit-for-bit (the reference draws from rand's thread RNG).
 * count = number of polynomials written to out:[count][N].
 *   uniform   random_polynomial_within (src/polynomial.rs:14-25): coefficients uniform in [-bound, bound],
 *             1 <= bound <= (q-1)/2  (commit randomness r: bound = b, commit.rs:101; key / message: (q-1)/2)
 *   gauss     random_polynomial_in_normal_distribution (src/polynomial.rs:28-44): (i64) N(0, sigma), truncated
 *             toward zero like I::from_f64; y of the provers: sigma = rzk_sigma(ctx) (open.rs:88-94).  Box-Muller on a
 *             64-bit uniform (tail to 9.4 sigma); evaluated in single precision for sigma < 2^19 (every parameter set of
 *             the reference; error of a sample before the truncation < 2^-24 (1.4 sigma^2 / R + 16 R) at radius R: far
 *             below 1 except for radii below sigma / 1000 or so, where it reaches 0.47 at sigma = 21780 — the word-to-
 *             pair map and its bound: ring_zk_amd/csrc/rzk_gauss.h), in double precision up to 2^26
 *   challenge random_polynomial_from_challenge_set (src/challenge_space.rs:12-33): exactly kappa coefficients
 *             +-1 (kappa of the context) at a uniformly random subset of positions, zeros elsewhere */
int rzk_sample_uniform_dev(rzk_ctx* ctx, uint64_t seed, uint32_t stream, uint64_t bound, int64_t* out, size_t count);
int rzk_sample_gauss_dev(rzk_ctx* ctx, uint64_t seed, uint32_t stream, double sigma, int64_t* out, size_t count);
int rzk_sample_challenge_dev(rzk_ctx* ctx, uint64_t seed, uint32_t stream, int64_t* out, size_t count);

/* ---- keyed device-side samplers (v6) --------------------------------------------------------------------------------
 * The samplers above are keyed by a 64-bit seed through Philox4x32-10: a statistical generator, fine for tests and
 * benchmarks, NOT for proofs anyone relies on (zero knowledge rests on y, hiding on r, interactive soundness on d being
 * unpredictable; the reference draws them from rand's ChaCha-based CSPRNG).  These draw the same three distributions,
 * with the same argument rules, from ChaCha20 (RFC 8439, 20 rounds) under a 256-bit key held by the context:
 *   subkey = HChaCha20(key, nonce)   (XChaCha construction, once per call, on the host)
 *   block(stream, poly, blk) = ChaCha20_block(subkey, words 12..15 = blk, poly lo, poly hi, stream)
 * poly = index of the polynomial within the call, blk = 64-byte block within it; one block serves 8 coefficients or 8
 * steps of the challenge sampler (ring_zk_amd/csrc/rzk_chacha.h restates every map).  Output is a
 * function of (key, nonce, stream, polynomial index) alone — not of count, the launch shape or the alignment of out.
 *
 * A (key, nonce, stream) triple must NEVER be used for two different draws: the second draw repeats the first one's
 * randomness (two responses z = y + d r, z' = y + d' r over the same y reveal r).  Use a fresh nonce per call — a
 * counter is enough — and the stream to separate the vectors of one call site.
 * Not claimed: constant time (Box-Muller runs in floating point, Floyd's walk has data-dependent LDS addresses).
 * Bias of a uniform coefficient / challenge position: <= range / 2^64.
 *
 * rzk_sampler_set_key copies the 32 bytes into the context (host memory; only per-call subkeys travel to the device, as
 * kernel arguments); NULL clears it.  The copy is wiped when it is replaced, cleared, and in rzk_ctx_destroy.
 * The draws return RZK_E_ARG when no key is set or nonce is NULL (and for a bad bound / sigma, as above); count == 0
 * returns RZK_OK.  They are asynchronous on the context's stream; out is a device pointer. */
int rzk_sampler_set_key(rzk_ctx* ctx, const uint8_t key[32]);
int rzk_sample_uniform_keyed_dev(rzk_ctx* ctx, const uint8_t nonce[16], uint32_t stream, uint64_t bound, int64_t* out,
                                 size_t count);
int rzk_sample_gauss_keyed_dev(rzk_ctx* ctx, const uint8_t nonce[16], uint32_t stream, double sigma, int64_t* out,
                               size_t count);
int rzk_sample_challenge_keyed_dev(rzk_ctx* ctx, const uint8_t nonce[16], uint32_t stream, int64_t* out, size_t count);

/* ---- the exact discrete Gaussian (v11) ------------------------------------------------------------------------------
 * rzk_sample_gauss_dev / rzk_sample_gauss_keyed_dev truncate a continuous normal toward zero: 0 carries the mass of
 * (-1, 1), about twice that of +-1, which is not the distribution D_sigma that the provers' rejection step
 * (rzk_reject_batch) assumes of y.  This sampler draws from D_sigma over the integers itself, P(v) proportional to
 * exp(-v^2 / 2 sigma^2), for an INTEGER sigma in [1, 2^26], in integer operations alone: the binary-Gaussian rejection
 * sampler of BLISS (Ducas, Durmus, Lepoint, Lyubashevsky 2013, Alg. 10-12).  The acceptance probability of a trial is
 * within eps_B = 2^-61 of the exact one, the tail is cut at 8k >= 9.4 sigma (mass < 2^-63), and the sigma realised
 * differs from the one asked for by less than 2^-73 relative (ring_zk_amd/csrc/rzk_dgauss.h states the sampler and the
 * error budget, DESIGN.md §15 the argument).  Being integer-only it is the same function of its words on every machine.
 * Stream: the subkey of the other keyed samplers; trial t of coefficient pair j of polynomial p reads
 *   ChaCha20_block(subkey, words 12..15 = 0x80000000 | t << 16 | j, p lo, p hi, stream)
 * (bit 31 of word 12 keeps these blocks apart from the other samplers' under the same key, nonce and stream); a
 * coefficient takes its first accepted trial, t < 160, and is 0 if there is none (probability < 2^-117).  Output is a
 * function of (key, nonce, stream, polynomial index, coefficient) alone.
 * count is the number of COEFFICIENTS written to out and must be a multiple of N (out: [count / N][N]).  RZK_E_ARG for
 * sigma = 0 or sigma > 2^26, no key set, a NULL nonce or out, a count that is no multiple of N; count == 0 returns RZK_OK.
 * Not claimed: constant time — the number of trials of a coefficient, and with it the kernel's queue traffic, depends on
 * the value drawn. */
int rzk_sample_dgauss_keyed_dev(rzk_ctx* ctx, const uint8_t nonce[16], uint32_t stream, uint32_t sigma, int64_t* out,
                                size_t count);

/* ---- wire format of one Mat (host only) ---------------------------------------------------------------------------- */
/* bincode layout of the reference's Mat<I,N> (serde derive at src/mat.rs:11-14; bincode default options as in
 * the reference's own test src/mat.rs:424-438: little-endian, u64 length prefixes):
 *     u64 rows ; rows x { u64 cols ; cols x { u64 len ; len x coefficient } }
 * with every polynomial in the crate's trimmed form (no trailing zero coefficients) <-> dense slabs
 * [rows][cols][N] of int64.  The protocol messages (src/commit.rs:134, src/prove/open.rs:190-228, ...) are NOT
 * concatenations of Mats: most of their fields are Vec<Polynomial>, Polynomial or Option<Polynomial>, whose bincode
 * form differs (an n x 1 Mat carries 8 bytes per row more than a Vec<Polynomial> of n).  Whole messages go through
 * the batched GPU codec below (rzk_wire_decode_batch / rzk_wire_encode_batch).  coef_bytes: 8 (i64) or 4 (i32, the width
 * of the reference's test vector); the width ZqI64 uses on the wire is set by the third-party ring crate and
 * is not pinned by any file of the reference.
 * encode: writes rzk_wire_mat_size() bytes (returned through *written; RZK_E_ARG if cap is too small or a
 *         coefficient does not fit coef_bytes).
 * decode: slab may be NULL to measure / validate only; fails on ragged rows, polynomials longer than N, truncated
 *         input and, with q > 0, on any coefficient outside the centred range [-(q-1)/2, (q-1)/2] of a ZqI64
 *         (src/params.rs:122-127) — q = 0 decodes plain integers, as the reference's i32 test vector needs;
 *         *consumed = bytes read, so consecutive fields of a message can be decoded in turn. */
size_t rzk_wire_mat_size(const int64_t* slab, uint32_t rows, uint32_t cols, uint32_t N, uint32_t coef_bytes);
int rzk_wire_mat_encode(const int64_t* slab, uint32_t rows, uint32_t cols, uint32_t N, uint32_t coef_bytes,
                        uint8_t* out, size_t cap, size_t* written);
int rzk_wire_mat_decode(const uint8_t* in, size_t len, uint32_t N, uint32_t coef_bytes, int64_t q, uint32_t* rows,
                        uint32_t* cols, int64_t* slab, size_t slab_polys, size_t* consumed);

/* ---- protocol messages on the wire (v4; batched, on the GPU) ----------------------------------------------------------
 * bincode with the reference's default options (src/mat.rs:424-438): little-endian, a u64 count before every Vec, struct
 * fields in declaration order without tags, a 1-byte tag (0 None, 1 Some) before an Option value; a Polynomial is its
 * trimmed coefficient Vec (u64 len ; len x coefficient), a Mat is u64 rows ; rows x { u64 cols ; cols x Polynomial }.
 * Each kind lists its fields in declaration order; each field is one dense int64 slab in the layout of the entry point
 * that consumes it (B messages; V = summands of the Sum kinds, ignored by the others):
 *   RZK_MSG_COMMITMENT         Commitment { c: Mat (n+l)x1 }                         (commit.rs:134)   c [B][n+l][N]
 *   RZK_MSG_OPENING            Opening { x: Vec<Poly>, r: Mat kx1, f: Option<Poly> } (commit.rs:222)   x [B][l][N], r [B][k][N], f [B][N]
 *   RZK_MSG_CHALLENGE          {Open,Linear,Sum}ProofChallenge { d: Poly }                             d [B][N]
 *   RZK_MSG_OPEN_COMMITMENT    OpenProofCommitment { c: Commitment, t: Vec<Poly> }   (open.rs:190)     c [B][n+l][N], t [B][n][N]
 *   RZK_MSG_OPEN_RESPONSE      OpenProofResponse { z: Mat kx1 }                      (open.rs:222)     z [B][k][N]
 *   RZK_MSG_LINEAR_COMMITMENT  LinearProofCommitment { c, cp: Commitment, g: Poly, t, tp: Vec<Poly>, u: Mat lx1 }
 *                              (linear.rs:271)   c, cp [B][n+l][N], g [B][N], t, tp [B][n][N], u [B][l][N]
 *   RZK_MSG_SUM_COMMITMENT     SumProofCommitment { cp: Commitment, cs: Vec<Commitment>, gs: Vec<Poly>, tp: Vec<Poly>,
 *                              ts: Vec<Vec<Poly>>, u: Mat lx1 } (sum.rs:342)   cp [B][n+l][N], cs [B][V][n+l][N], gs [B][V][N],
 *                              tp [B][n][N], ts [B][V][n][N], u [B][l][N]
 *   RZK_MSG_SUM_RESPONSE       SumProofResponse { zp: Mat kx1, zs: Vec<Mat kx1> }    (sum.rs:385)      zp [B][k][N], zs [B][V][k][N]
 * (LinearProofResponse has no serde derive, linear.rs:318: its two Mats go through rzk_wire_mat_*.)
 * Option: decoding None writes the constant polynomial 1 into f (Commitment::verify with Some(1) makes the same
 * comparison as with None, commit.rs:200-209); encoding with fields[f] == NULL writes None for every message, otherwise
 * every message gets Some(f).  coef_bytes: 4 or 8, as for the Mat codec.
 *
 * rzk_wire_max_bytes: the largest encoding of one message of the kind (every polynomial at full length); 0 = bad
 * argument.
 * rzk_wire_decode_batch: message b is bytes[offsets[b] .. offsets[b+1]) (offsets: [B+1]); fields[i] is the slab of the
 * kind's i-th field.  Returns RZK_OK on a well-formed call; malformed messages are reported per message: ok[b] = 1 only
 * if every count, row and column count equals the context's n, k, l and V, every len <= N, every Option tag is 0 or 1,
 * every coefficient is the centred residue mod q, and the message ends exactly at offsets[b+1].  That last rule is
 * stricter than bincode::deserialize, which ignores trailing bytes: a batch slot holds one message.  A message with
 * offsets[b] % coef_bytes != 0 (every kind except RZK_MSG_OPENING, whose messages end with the 1-byte tag and may start
 * anywhere), offsets[b] > offsets[b+1] or offsets[b+1] > total_len gets ok[b] = 0 without any of its bytes being read.
 * Slabs of a rejected message are unspecified.  RZK_E_ARG only for a bad kind or width, NULL pointers, V == 0 on a Sum
 * kind or a `bytes` pointer not aligned to coef_bytes; RZK_E_UNSUPPORTED for total_len >= 2^48.
 * rzk_wire_encode_batch: writes the B messages back to back from bytes[0] and their B+1 boundaries into offsets.
 * Requires cap >= B * rzk_wire_max_bytes(...) (checked on the host, RZK_E_ARG otherwise).  A non-canonical input
 * coefficient raises the input-fault condition (see Conventions: RZK_E_ARG at return, or at the next
 * rzk_ctx_synchronize for the _dev variant).
 * The _dev variants take device pointers for bytes, offsets, ok and the slabs; `fields` itself is a host array of
 * device pointers. */
#define RZK_MSG_COMMITMENT 0
#define RZK_MSG_OPENING 1
#define RZK_MSG_CHALLENGE 2
#define RZK_MSG_OPEN_COMMITMENT 3
#define RZK_MSG_OPEN_RESPONSE 4
#define RZK_MSG_LINEAR_COMMITMENT 5
#define RZK_MSG_SUM_COMMITMENT 6
#define RZK_MSG_SUM_RESPONSE 7
size_t rzk_wire_max_bytes(const rzk_ctx* ctx, int kind, uint32_t V, uint32_t coef_bytes);
int rzk_wire_decode_batch(rzk_ctx* ctx, int kind, uint32_t V, uint32_t coef_bytes, const uint8_t* bytes,
                          uint64_t total_len, const uint64_t* offsets, int64_t* const* fields, uint8_t* ok, size_t B);
int rzk_wire_decode_batch_dev(rzk_ctx* ctx, int kind, uint32_t V, uint32_t coef_bytes, const uint8_t* bytes,
                              uint64_t total_len, const uint64_t* offsets, int64_t* const* fields, uint8_t* ok,
                              size_t B);
int rzk_wire_encode_batch(rzk_ctx* ctx, int kind, uint32_t V, uint32_t coef_bytes, const int64_t* const* fields,
                          uint8_t* bytes, uint64_t cap, uint64_t* offsets, size_t B);
int rzk_wire_encode_batch_dev(rzk_ctx* ctx, int kind, uint32_t V, uint32_t coef_bytes, const int64_t* const* fields,
                              uint8_t* bytes, uint64_t cap, uint64_t* offsets, size_t B);

/* ---- Fiat-Shamir: non-interactive challenges (v5) -----------------------------------------------------------------------
 * The reference's protocols are interactive (the verifier draws d: open.rs:138-145, linear.rs:182-189, sum.rs:226-233).
 * Here d is derived from the prover's first message by the "FS1" transcript hash (every byte of the
 * format is restated in ring_zk_amd/csrc/rzk_keccak.h), so that a proof (commitment, response) can be stored, forwarded
 * and batch-verified: the verifier recomputes d from the commitment message it received.
 *   LEAF = min(N, 256), C = N / LEAF; a coefficient is hashed as the little-endian int32 of its centred value
 *   leaf(p,c)  = SHAKE256("RZKFS1\0L" | le32(p) | le32(c) | coefficients c*LEAF .. (c+1)*LEAF-1 of polynomial p)[0:32]
 *   keydigest  = SHAKE256("RZKFS1\0K" | le64(q) | le32(N) | le32(n) | le32(k) | le32(l) | le32(kappa) | le32(0) | le64(b)
 *                         | leaf(p,c) of the (n+l)*k key polynomials row-major)[0:32]
 *   stream     = SHAKE256("RZKFS1\0R" | le32(kind) | le32(V) | keydigest | aux[32] | leaf(p,c) of the message polynomials)
 * with the message polynomials in the order of the RZK_MSG_* table above (fields in declaration order, slabs row-major)
 * and V = 0 for the kinds without summands.  stream[0:32] is the transcript digest; d has exactly kappa coefficients
 * +-1 (uniform over challenge_space.rs:10-33), sampled from stream[32:].
 * rzk_fs_key_digest: keydigest of the loaded key (computed on the device by rzk_key_load[_dev] / rzk_key_generate);
 *   RZK_E_STATE without a key.
 * rzk_fs_challenge_batch: kind is RZK_MSG_OPEN_COMMITMENT, RZK_MSG_LINEAR_COMMITMENT or RZK_MSG_SUM_COMMITMENT
 *   (RZK_E_ARG otherwise); fields as for the wire codec; aux32: 32 HOST bytes binding the call to a session or
 *   statement, NULL = zeros; d: [B][N]; digest: [B][32] or NULL; ok: [B] or NULL.  A coefficient outside the centred
 *   range clears ok[b] of its own proof only, whose d and digest are unspecified; the call succeeds (as in
 *   rzk_wire_decode_batch).  With ok == NULL there is no per-proof verdict to clear, so such a coefficient is an input
 *   fault of the call, as in the phase entry points: the host variant returns RZK_E_ARG, the _dev variant raises the
 *   sticky word that rzk_ctx_check_inputs reports.  It is never hashed as its low 32 bits without a signal.  In
 *   trusted-producer mode the test is skipped (the caller vouches for the range).  Needs kappa <= N and a loaded key. */
int rzk_fs_key_digest(rzk_ctx* ctx, uint8_t* out32);
int rzk_fs_challenge_batch(rzk_ctx* ctx, int kind, uint32_t V, const int64_t* const* fields, const uint8_t* aux32,
                           int64_t* d, uint8_t* digest, uint8_t* ok, size_t B);
int rzk_fs_challenge_batch_dev(rzk_ctx* ctx, int kind, uint32_t V, const int64_t* const* fields, const uint8_t* aux32,
                               int64_t* d, uint8_t* digest, uint8_t* ok, size_t B);

/* ---- rejection sampling: the step that makes a response independent of the secret (v7) ----------------------------------
 * The scheme (BDLOP, eprint 2016/997, Fig. 2; Lyubashevsky 2012, Thm 4.6) releases z = y + d r only with probability
 * min(1, D_sigma(z) / (M D_{v,sigma}(z))), v = d r, and otherwise starts again with a fresh y; the reference's
 * create_response (open.rs:107-117, linear.rs:144-158, sum.rs:182-200) leaves that out, so every z it releases is a
 * Gaussian centred at d r.  This entry point is the test (ring_zk_amd/csrc/rzk_reject.h restates it):
 * a proof's `rows` response polynomials (Open: k, Linear: 2k, Sum: (V+1) k) are given as nparts (1 .. 4) pairs of slabs
 * z[p], y[p]: [B][rows[p]][N], an array of field pointers as for rzk_fs_challenge_batch (a HOST array; the _dev variant's
 * slabs, coin, accept and E are device pointers, the slabs 16-byte aligned).
 *   per coefficient  v = centred((z - y) mod q)
 *   per proof        S1 = sum z v, S2 = sum v^2, E = S2 - 2 S1 in exact integers over all rows and coefficients
 *   fail             a z or y coefficient is not canonical (skipped in trusted-producer mode) | some |v| > kappa b |
 *                    a z polynomial fails check_verify_constraint (sum c^2 < (verify_bound + 1)^2) | coin[b] outside [0, R)
 *   accept[b]        !fail && (double)E >= 2 sigma^2 (lnM + log((coin[b] + 1) / R)), in double precision, sigma = rzk_sigma:
 *                    coin / R < min(1, exp(E / 2 sigma^2) / M) in the log domain; coin[b]: caller-supplied, uniform in [0, R)
 * E (may be NULL) receives E per proof: exact whenever no fail flag is set and for the norm / kappa b failures short of
 * |E| >= 2^63 (then it is E mod 2^64); unspecified for non-canonical input.  A non-canonical coefficient clears accept[b]
 * and is an input fault of the call as in the phase entry points: RZK_E_ARG from the host variant, the sticky word
 * (rzk_ctx_check_inputs) from the _dev variant.  RZK_E_ARG also for nparts outside 1 .. 4, R outside [2, 2^62], lnM < 0 or
 * not finite, NULL pointers, and unless rows N 2^24 kappa b < 2^52 and verify_bound < 2^24 (which keep |E| < 2^53 for
 * every unflagged proof).  B == 0 is a no-op.
 * rzk_reject_lnm(alpha) = 12 / alpha + 1 / (2 alpha^2): ln M for sigma = alpha |v|_2 (Thm 4.6).  sigma = 11 kappa b sqrt(k N)
 * (params.rs:94-98) is alpha = 11 for ONE vector d r of k polynomials; a proof with m such vectors uses alpha = 11 / sqrt(m).
 * Not claimed: constant time. */
double rzk_reject_lnm(double alpha);
int rzk_reject_batch(rzk_ctx* ctx, uint32_t nparts, const int64_t* const* z, const int64_t* const* y, const uint32_t* rows,
                     const int64_t* coin, uint64_t R, double lnM, uint8_t* accept, int64_t* E, size_t B);
int rzk_reject_batch_dev(rzk_ctx* ctx, uint32_t nparts, const int64_t* const* z, const int64_t* const* y, const uint32_t* rows,
                         const int64_t* coin, uint64_t R, double lnM, uint8_t* accept, int64_t* E, size_t B);

/* ---- 32-bit slabs (v14) ---------------------------------------------------------------------------------------
 * A "slab32" is the dense row-major [batch][row][N] layout of every coefficient slab above with int32_t centred residues: the
 * same values, half the bytes.  It exists because (q - 1) / 2 < 2^31 for every modulus rzk_ctx_create accepts.  Opt-in: a caller
 * that keeps data on the device (sampler outputs narrowed once, this library's own outputs fed to the next call) gets the same
 * proofs and verdicts from slabs half the size; nothing about the 64-bit entry points changes.
 *   canonical   still |c| <= (q - 1) / 2: the int32 range is wider than that, so every call tests as its sibling does
 *   alignment   device slabs are 16-byte aligned (RZK_E_ARG otherwise)
 *   width       all slabs of one call have the same width
 * rzk_narrow_batch   out = in as int32 (count polynomials).  A non-canonical coefficient is an input fault of the call, reported
 *                    as the Mat-level calls report theirs (host form: RZK_E_ARG; _dev form: the sticky condition, at the next
 *                    synchronising call / rzk_ctx_check_inputs); its output value is then unspecified.  Trusted-producer mode
 *                    (rzk_ctx_trust_device_outputs): no test.
 * rzk_widen_batch    out = in sign-extended.  No test: the consuming call tests.
 * rzk_open_*32_batch the Open cycle: arguments, verdict bytes, fused norm predicate and fault rules of rzk_open_commit_batch,
 *                    rzk_open_response_batch, rzk_open_verify_batch and rzk_open_recover_batch, every slab int32_t.  Prover side
 *                    (commit32, response32) a non-canonical coefficient fails the call; verifier side (verify32, recover32) it
 *                    clears that proof's verdict and the call succeeds.  Bit-identical to narrow() of the siblings' outputs.
 * Native 32-bit kernels run at N = 512 and N = 1024 with n = 1 and the default rotation knobs; every other context converts
 * inside the call (widen into a grow-only arena, the sibling's launches, narrow): same results, no gain.  The _dev forms make
 * no allocation and no host synchronisation in the steady state.  NULL pointers: RZK_E_ARG (ok of commit32 may be NULL);
 * B == 0 / count == 0 is a no-op. */
int rzk_narrow_batch(rzk_ctx* ctx, const int64_t* in, int32_t* out, size_t count);
int rzk_narrow_batch_dev(rzk_ctx* ctx, const int64_t* in, int32_t* out, size_t count);
int rzk_widen_batch(rzk_ctx* ctx, const int32_t* in, int64_t* out, size_t count);
int rzk_widen_batch_dev(rzk_ctx* ctx, const int32_t* in, int64_t* out, size_t count);
int rzk_open_commit32_batch(rzk_ctx* ctx, const int32_t* x, const int32_t* r, const int32_t* y, int32_t* c, int32_t* t,
                            uint8_t* ok, size_t B);
int rzk_open_commit32_batch_dev(rzk_ctx* ctx, const int32_t* x, const int32_t* r, const int32_t* y, int32_t* c, int32_t* t,
                                uint8_t* ok, size_t B);
int rzk_open_response32_batch(rzk_ctx* ctx, const int32_t* y, const int32_t* r, const int32_t* d, int32_t* z, size_t B);
int rzk_open_response32_batch_dev(rzk_ctx* ctx, const int32_t* y, const int32_t* r, const int32_t* d, int32_t* z, size_t B);
int rzk_open_verify32_batch(rzk_ctx* ctx, const int32_t* z, const int32_t* t, const int32_t* c, const int32_t* d,
                            uint8_t* accept, size_t B);
int rzk_open_verify32_batch_dev(rzk_ctx* ctx, const int32_t* z, const int32_t* t, const int32_t* c, const int32_t* d,
                                uint8_t* accept, size_t B);
int rzk_open_recover32_batch(rzk_ctx* ctx, const int32_t* z, const int32_t* c, const int32_t* d, int32_t* t_out,
                             uint8_t* accept, size_t B);
int rzk_open_recover32_batch_dev(rzk_ctx* ctx, const int32_t* z, const int32_t* c, const int32_t* d, int32_t* t_out,
                                 uint8_t* accept, size_t B);

/* ---- 32-bit slabs: messages (v14, slab32 messages) ------------------------------------------------------------
 * The transcript hash, the packed codec and the compare of the short verifier on int32_t slabs, so that a stored proof goes
 * record -> verdict and operands -> record without a 64-bit slab or a convert launch.  Additions only: RZK_ABI_VERSION stays
 * 14, every earlier signature is unchanged, and a binding that resolves these names fails at load on a library without them.
 * Argument rules, NULL rules, B == 0, fault reporting and trusted-producer mode are those of the 64-bit sibling named below;
 * device slabs (fields, d, a, b) are 16-byte aligned as everywhere in the section above (RZK_E_ARG otherwise).  All kinds
 * the sibling takes are supported (the kernels do not depend on the kind).
 * rzk_fs_challenge32_batch    sibling rzk_fs_challenge_batch.  digest and ok are byte for byte what the sibling returns on
 *                             widen(fields); d is narrow() of its d.  FS1 hashes a coefficient as the little-endian int32 of
 *                             its centred value, so a slab32 is the hash's input as it stands; the range test is made on
 *                             the int32 (|c| <= (q-1)/2), with the sibling's consequences.
 * rzk_packed_encode32_batch   sibling rzk_packed_encode_batch.  records and ok are byte for byte the sibling's on widen(fields).
 * rzk_packed_decode32_batch   sibling rzk_packed_decode_batch.  ok is identical; every field of a record with ok = 1 is
 *                             narrow() of the sibling's (every valid value lies in [-bias, limit - bias], inside [-(q-1)/2,
 *                             (q-1)/2]); slabs of a rejected record are unspecified, as there.
 *                             Records have no width: one written by either encoder decodes with either decoder.
 * rzk_eq32_batch              eq[b] = 1 iff the two [rows][N] blocks of entry b are equal word for word.  Unlike rzk_eq_batch
 *                             there is no range test and no input fault: the verdict of the call that consumes or produced
 *                             the slabs (rzk_open_recover32_batch for the short verifier) has tested them.  rows >= 1. */
int rzk_fs_challenge32_batch(rzk_ctx* ctx, int kind, uint32_t V, const int32_t* const* fields, const uint8_t* aux32,
                             int32_t* d, uint8_t* digest, uint8_t* ok, size_t B);
int rzk_fs_challenge32_batch_dev(rzk_ctx* ctx, int kind, uint32_t V, const int32_t* const* fields, const uint8_t* aux32,
                                 int32_t* d, uint8_t* digest, uint8_t* ok, size_t B);
int rzk_packed_encode32_batch(rzk_ctx* ctx, int kind, uint32_t V, const int32_t* const* fields, uint8_t* records, uint8_t* ok,
                              size_t B);
int rzk_packed_encode32_batch_dev(rzk_ctx* ctx, int kind, uint32_t V, const int32_t* const* fields, uint8_t* records,
                                  uint8_t* ok, size_t B);
int rzk_packed_decode32_batch(rzk_ctx* ctx, int kind, uint32_t V, const uint8_t* records, int32_t* const* fields, uint8_t* ok,
                              size_t B);
int rzk_packed_decode32_batch_dev(rzk_ctx* ctx, int kind, uint32_t V, const uint8_t* records, int32_t* const* fields,
                                  uint8_t* ok, size_t B);
int rzk_eq32_batch(rzk_ctx* ctx, const int32_t* a, const int32_t* b, uint32_t rows, uint8_t* eq, size_t B);
int rzk_eq32_batch_dev(rzk_ctx* ctx, const int32_t* a, const int32_t* b, uint32_t rows, uint8_t* eq, size_t B);

/* The response and its test in one call (v13): "give me z, and tell me whether I may release it".
 * z (z', z_s) is byte for byte what rzk_*_response_batch writes; accept and E (may be NULL) are what rzk_reject_batch
 * returns for the parts [(z, y)] (Open), [(z, y), (z', y')] (Linear), [(z_s, y_s), (z', y')] (Sum) with the same coin, R
 * and lnM.  Argument rules and messages are those of rzk_reject_batch with rows = k, 2k, (V + 1) k; y and z slabs of the
 * _dev variants are 16-byte aligned; B == 0 is a no-op.  At N = 512 and 1024 the response rows accumulate the statistic
 * themselves from the product d r, the addend y and the sum z they hold in registers (response_stat_kernel): z and y are
 * never read back.  At N = 2048 (two wavefronts per polynomial), N <= 256 and under RZK_SHIFT=0 the call runs the
 * response launch and then the statistic kernel of rzk_reject_batch: same outputs.
 * One deliberate tightening where the fused rows run: a non-canonical coefficient of r or d, which the two-call form only
 * reports through the sticky word, also clears accept[b] of its proof.  As there it is an input fault of the call
 * (RZK_E_ARG from the host variant, the sticky word from _dev), and E of such a proof is unspecified. */
int rzk_open_response_reject_batch(rzk_ctx* ctx, const int64_t* y, const int64_t* r, const int64_t* d, const int64_t* coin,
                                   uint64_t R, double lnM, int64_t* z, uint8_t* accept, int64_t* E, size_t B);
int rzk_open_response_reject_batch_dev(rzk_ctx* ctx, const int64_t* y, const int64_t* r, const int64_t* d, const int64_t* coin,
                                       uint64_t R, double lnM, int64_t* z, uint8_t* accept, int64_t* E, size_t B);
int rzk_linear_response_reject_batch(rzk_ctx* ctx, const int64_t* y, const int64_t* yp, const int64_t* r, const int64_t* rp,
                                     const int64_t* d, const int64_t* coin, uint64_t R, double lnM, int64_t* z, int64_t* zp,
                                     uint8_t* accept, int64_t* E, size_t B);
int rzk_linear_response_reject_batch_dev(rzk_ctx* ctx, const int64_t* y, const int64_t* yp, const int64_t* r, const int64_t* rp,
                                         const int64_t* d, const int64_t* coin, uint64_t R, double lnM, int64_t* z, int64_t* zp,
                                         uint8_t* accept, int64_t* E, size_t B);
int rzk_sum_response_reject_batch(rzk_ctx* ctx, uint32_t V, const int64_t* ys, const int64_t* yp, const int64_t* rs,
                                  const int64_t* rp, const int64_t* d, const int64_t* coin, uint64_t R, double lnM, int64_t* zs,
                                  int64_t* zp, uint8_t* accept, int64_t* E, size_t B);
int rzk_sum_response_reject_batch_dev(rzk_ctx* ctx, uint32_t V, const int64_t* ys, const int64_t* yp, const int64_t* rs,
                                      const int64_t* rp, const int64_t* d, const int64_t* coin, uint64_t R, double lnM,
                                      int64_t* zs, int64_t* zp, uint8_t* accept, int64_t* E, size_t B);

/* ---- 32-bit slabs: the zero-knowledge Open prover (v14, slab32 prover) ---------------------------------------
 * What a prover that draws its own r and y and loops over the rejection step needs on int32_t slabs, so that x -> (c, t, z)
 * runs without a 64-bit slab or a convert launch.  Additions only: RZK_ABI_VERSION stays 14 and every earlier signature is
 * unchanged.  Each call has the argument list of the 64-bit sibling named below with int32_t* slabs; argument rules, NULL
 * rules, count == 0 / B == 0, fault reporting and trusted-producer mode are the sibling's; device slabs are 16-byte aligned
 * (RZK_E_ARG otherwise), as everywhere in the 32-bit sections above.
 * rzk_sample_{uniform,gauss,dgauss,challenge}_keyed32_dev
 *                                   siblings rzk_sample_*_keyed_dev (device only).  The same stream: for the same key, nonce,
 *                                   stream and arguments, out is narrow() of the sibling's out, coefficient by coefficient.
 *                                   Every value an accepted argument can produce lies inside int32_t (uniform: |v| <=
 *                                   (q-1)/2 < 2^31; gauss: |v| < 5.8e8 at sigma = 2^26; dgauss: tail cut at 9.4 sigma),
 *                                   so there is no further range rule.
 * rzk_matvec32_batch                sibling rzk_matvec_batch (addend may be NULL): out = narrow() of its out; prover side, a
 *                                   non-canonical coefficient is an input fault of the call.
 * rzk_open_response_reject32_batch  sibling rzk_open_response_reject_batch with y, r, d, z as int32_t slabs; coin and E stay
 *                                   int64_t, accept uint8_t.  z is narrow() of the sibling's z; accept and E are byte for
 *                                   byte the sibling's on widen(y, r, d).
 * Native 32-bit kernels run where those of the Open cycle do (N = 512 and 1024, n = 1, default rotation knobs); every other
 * context converts inside the call. */
int rzk_sample_uniform_keyed32_dev(rzk_ctx* ctx, const uint8_t nonce[16], uint32_t stream, uint64_t bound, int32_t* out,
                                   size_t count);
int rzk_sample_gauss_keyed32_dev(rzk_ctx* ctx, const uint8_t nonce[16], uint32_t stream, double sigma, int32_t* out,
                                 size_t count);
int rzk_sample_challenge_keyed32_dev(rzk_ctx* ctx, const uint8_t nonce[16], uint32_t stream, int32_t* out, size_t count);
int rzk_sample_dgauss_keyed32_dev(rzk_ctx* ctx, const uint8_t nonce[16], uint32_t stream, uint32_t sigma, int32_t* out,
                                  size_t count);
int rzk_matvec32_batch(rzk_ctx* ctx, int which, const int32_t* v, const int32_t* addend, int32_t* out,
                       size_t B);
int rzk_matvec32_batch_dev(rzk_ctx* ctx, int which, const int32_t* v, const int32_t* addend,
                           int32_t* out, size_t B);
int rzk_open_response_reject32_batch(rzk_ctx* ctx, const int32_t* y, const int32_t* r, const int32_t* d, const int64_t* coin,
                                     uint64_t R, double lnM, int32_t* z, uint8_t* accept, int64_t* E, size_t B);
int rzk_open_response_reject32_batch_dev(rzk_ctx* ctx, const int32_t* y, const int32_t* r, const int32_t* d, const int64_t* coin,
                                         uint64_t R, double lnM, int32_t* z, uint8_t* accept, int64_t* E, size_t B);

/* ---- prover loop: the zero-knowledge Open prover in one call (v14, prover loop) ------------------------------
 * x -> (c, t, z, ok, r, rounds) with the rejection loop inside the library: what a caller otherwise writes around
 * rzk_open_commit*, rzk_matvec*, rzk_fs_challenge*, rzk_open_response_reject* and the keyed samplers, including which proofs
 * are pending, under which nonces they are drawn and what must not leave the device.  Additions only: RZK_ABI_VERSION stays 14.
 * One entry point per slab width; the int32_t form is narrow() of the int64_t form, slab for slab.
 *   round 0   r = uniform(b) [B][k][N]; y = Gaussian [B][k][N]; two coin draws; c, t = open_commit(x, r, y);
 *             d = challenge(c, t) under RZK_MSG_OPEN_COMMITMENT and aux32; z, accept = open_response_reject(y, r, d, coin,
 *             R, lnM) with lnM = rzk_reject_lnm(11), R = (2^31 - 1)^2
 *   retry     the proofs with ok_commit & ok_hash and no accepted response yet, in ascending order, as a dense sub-batch
 *             (position = polynomial index of the samplers): fresh y and coins, t = a1.y, d = challenge(c, t), z, accept; the
 *             accepted (t, z) replace the proof's, rounds[b] = the round
 *   coin      (a + 2^30 - 1) (2^31 - 1) + (b + 2^30 - 1) from two uniform(2^30 - 1) draws of one polynomial per proof,
 *             a = coefficient 0 of the first, b = coefficient 1 of the second
 * gauss_kind  0: rzk_sample_gauss_keyed*_dev at rzk_sigma(ctx); 1: rzk_sample_dgauss_keyed*_dev at rzk_sigma(ctx); anything
 *             else RZK_E_ARG.  The key is the one installed by rzk_sampler_set_key: RZK_E_STATE without one.
 * stream      the samplers' stream argument, the same for every draw of the call.
 * max_rounds  1 .. 255 (RZK_E_ARG otherwise); aux32: 32 HOST bytes or NULL, as for rzk_fs_challenge_batch.
 * nonces      nonce i = nonce0 + i as a 128-bit little-endian integer.  The call consumes 1 + 3 * rounds_run of them, in this
 *             order: r; then per round y, coin draw a, coin draw b.  A round with nothing pending does not run and consumes
 *             nothing.  RZK_E_ARG, before anything is launched, when nonce0 + 1 + 3 * max_rounds leaves 128 bits.  The nonces
 *             nonce0 .. nonce0 + 3 * max_rounds belong to the call; the caller continues at nonce0 + 1 + 3 * rounds_run or later.
 * rounds_run  HOST memory (may be NULL): the number of rounds that ran, round 0 included.
 * outputs     c:[B][n+l][N] and r:[B][k][N] are written for every proof.  ok[b] = 1 iff r passed the commit constraint, the
 *             round-0 transcript hash was ok and the proof was accepted in round rounds[b] < max_rounds; t:[B][n][N] and
 *             z:[B][k][N] of every other proof are zero (a rejected response is never released).  x:[B][l][N].
 * Argument, fault and trusted-mode rules are those of the calls above; a non-canonical coefficient of x clears ok[b] and raises
 * the sticky input-error word as in rzk_open_commit_batch_dev (the host form returns RZK_E_ARG).  Device slabs of both widths
 * are 16-byte aligned (RZK_E_ARG).  B == 0 is a no-op; B >= 2^32 is RZK_E_ARG.  The _dev form synchronises the stream once per
 * retry round (it reads the 4-byte pending count) and allocates only when a batch is larger than any before.  Its workspace
 * copies of y, t, z and the coins are zeroed on the stream before it returns; when it fails after round 0 was started, t, z
 * and ok are zeroed too (a failed call releases no response).  Bit-identical to fiat_shamir.open_prove_zk /
 * open_prove_zk32 of the Python layer under the same key, stream and first nonce.
 * Not claimed: constant time (the number of rounds, and the pending sets, depend on the secrets). */
int rzk_open_prove_zk_batch(rzk_ctx* ctx, const int64_t* x, const uint8_t nonce0[16], uint32_t stream, int gauss_kind,
                            const uint8_t* aux32, uint32_t max_rounds, int64_t* c, int64_t* t, int64_t* z, int64_t* r,
                            uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run, size_t B);
int rzk_open_prove_zk_batch_dev(rzk_ctx* ctx, const int64_t* x, const uint8_t nonce0[16], uint32_t stream, int gauss_kind,
                                const uint8_t* aux32, uint32_t max_rounds, int64_t* c, int64_t* t, int64_t* z, int64_t* r,
                                uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run, size_t B);
int rzk_open_prove_zk32_batch(rzk_ctx* ctx, const int32_t* x, const uint8_t nonce0[16], uint32_t stream, int gauss_kind,
                              const uint8_t* aux32, uint32_t max_rounds, int32_t* c, int32_t* t, int32_t* z, int32_t* r,
                              uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run, size_t B);
int rzk_open_prove_zk32_batch_dev(rzk_ctx* ctx, const int32_t* x, const uint8_t nonce0[16], uint32_t stream, int gauss_kind,
                                  const uint8_t* aux32, uint32_t max_rounds, int32_t* c, int32_t* t, int32_t* z, int32_t* r,
                                  uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run, size_t B);

/* ---- the y-only half of the Linear and Sum commit steps ("mask" calls; v14, additions only) -----------------
 * t, t', u are the part of the commitment message that depends on the fresh y alone (linear.rs:118-129, sum.rs:145-160):
 *   Linear   t = a1.y, t' = a1.y', u = (a2.y) (.) g - a2.y'
 *   Sum      t_i = a1.y_i, t' = a1.y', u = sum_i (a2.y_i) (.) g_i - a2.y'
 * c, c' (c_i, c') do not depend on y, so a prover that retries with a fresh y (the rejection step) calls these in place of
 * the commit call.  Layouts are those of rzk_linear_commit_batch / rzk_sum_commit_batch, and t, tp, u (ts, tp, u) are byte
 * for byte what those calls write for the same g, y, yp (gs, ys, yp).  Shape limits, V == 0 (RZK_E_ARG), NULL pointers
 * (RZK_E_ARG) and B == 0 (a no-op) are the commit calls' rules.  There is no ok output: y carries no norm rule in the
 * commit step.  A non-canonical input coefficient is reported as by rzk_matvec_batch[_dev]: RZK_E_ARG from the host form,
 * the sticky input-error word from _dev; trusted-producer mode skips the test as everywhere.
 * Routing: Linear runs the "masks only" form of its commit-row program (y is transformed once for the a1 and the a2 row)
 * and the u rows; Sum runs three or four of the commit call's key-product and multiplier programs, on the side of
 * the a2.(sum_i g_i y_i - y') rearrangement that the commit call takes on the same context. */
int rzk_linear_mask_batch(rzk_ctx* ctx, const int64_t* g, const int64_t* y, const int64_t* yp, int64_t* t, int64_t* tp,
                          int64_t* u, size_t B);
int rzk_linear_mask_batch_dev(rzk_ctx* ctx, const int64_t* g, const int64_t* y, const int64_t* yp, int64_t* t, int64_t* tp,
                              int64_t* u, size_t B);
int rzk_sum_mask_batch(rzk_ctx* ctx, uint32_t V, const int64_t* gs, const int64_t* ys, const int64_t* yp, int64_t* ts,
                       int64_t* tp, int64_t* u, size_t B);
int rzk_sum_mask_batch_dev(rzk_ctx* ctx, uint32_t V, const int64_t* gs, const int64_t* ys, const int64_t* yp, int64_t* ts,
                           int64_t* tp, int64_t* u, size_t B);

/* ---- prover loop: the zero-knowledge Linear and Sum provers in one call (v14, additions only) ---------------
 * The contract of rzk_open_prove_zk_batch[_dev], restated for the other two proofs; 64-bit slabs only.
 *   Linear   (g, x) -> (c, cp, t, tp, u, z, zp, r, rp, ok, rounds)
 *   Sum      (gs, xs), V summands -> (cs, cp, ts, tp, u, zs, zp, rs, rp, ok, rounds)
 *   round 0   r, r' = uniform(b) [B][k][N] each (Sum: rs [B][V][k][N] under ONE nonce, then r'); y, y' Gaussian (Sum: ys
 *             [B][V][k][N] under one nonce, then y'); two coin draws; the full rzk_linear_commit / rzk_sum_commit; d = challenge
 *             of (c, cp, g, t, tp, u) under RZK_MSG_LINEAR_COMMITMENT, of (cp, cs, gs, tp, ts, u) with V under
 *             RZK_MSG_SUM_COMMITMENT, and aux32; rzk_linear_response_reject / rzk_sum_response_reject with R = (2^31 - 1)^2 and
 *             lnM = rzk_reject_lnm(11 / sqrt(m)), m = 2 (Linear), V + 1 (Sum).  live = (ok_commit == 3) & ok_hash (Linear),
 *             (ok_commit != 0) & ok_hash (Sum); done = live & accept
 *   retry     the live proofs without an accepted response, in ascending order, as a dense sub-batch (position = polynomial
 *             index of the samplers): fresh y, y' and coins; r, rp, c, cp, g (rs, rp, cs, cp, gs) gathered; the mask call above
 *             in place of the commit call; the hash; the response with its test; the accepted t, tp, u, z, zp (ts, tp, u, zs,
 *             zp) replace the proof's, rounds[b] = the round.  x is not read again.
 *   coin      as for Open.
 * gauss_kind, stream, max_rounds, aux32, rounds_run: as for rzk_open_prove_zk_batch.
 * nonces      nonce i = nonce0 + i.  The call consumes 2 + 4 * rounds_run of them: r, r'; then per round y, y', coin draw a,
 *             coin draw b.  RZK_E_ARG, before anything is launched, when nonce0 + 2 + 4 * max_rounds leaves 128 bits.
 * outputs     c, cp, r, rp (cs, cp, rs, rp) are written for every proof.  ok[b] = 1 iff the proof was live and accepted in round
 *             rounds[b] < max_rounds; t, tp, u, z, zp (ts, tp, u, zs, zp) of every other proof are zero.
 * Argument rules are Open's: gauss_kind 0 or 1, max_rounds 1 .. 255, V 1 .. 2^20 and an entry size that fits (RZK_E_ARG); no
 * sampler key: RZK_E_STATE; every device slab 16-byte aligned (RZK_E_ARG); B == 0 is a no-op; B >= 2^32 is RZK_E_ARG.  Each
 * refusal comes before the first launch.  A non-canonical coefficient of x or g (xs, gs) clears ok[b] and raises the sticky
 * input-error word as in the commit calls (the host form returns RZK_E_ARG).  The _dev form synchronises the stream once per
 * retry round (the 4-byte pending count).  The workspace's y, y', coin draws and coins, and its retry copies of the five
 * y-dependent outputs, are zeroed on the stream whichever way the loop ends; a call that fails after round 0 was started
 * zeroes the five y-dependent outputs and ok.  Bit-identical to fiat_shamir.linear_prove_zk / sum_prove_zk of the Python layer
 * under the same key, stream and first nonce.  Not claimed: constant time. */
int rzk_linear_prove_zk_batch(rzk_ctx* ctx, const int64_t* g, const int64_t* x, const uint8_t nonce0[16], uint32_t stream,
                              int gauss_kind, const uint8_t* aux32, uint32_t max_rounds, int64_t* c, int64_t* cp, int64_t* t,
                              int64_t* tp, int64_t* u, int64_t* z, int64_t* zp, int64_t* r, int64_t* rp, uint8_t* ok,
                              uint8_t* rounds, uint32_t* rounds_run, size_t B);
int rzk_linear_prove_zk_batch_dev(rzk_ctx* ctx, const int64_t* g, const int64_t* x, const uint8_t nonce0[16], uint32_t stream,
                                  int gauss_kind, const uint8_t* aux32, uint32_t max_rounds, int64_t* c, int64_t* cp, int64_t* t,
                                  int64_t* tp, int64_t* u, int64_t* z, int64_t* zp, int64_t* r, int64_t* rp, uint8_t* ok,
                                  uint8_t* rounds, uint32_t* rounds_run, size_t B);
int rzk_sum_prove_zk_batch(rzk_ctx* ctx, uint32_t V, const int64_t* gs, const int64_t* xs, const uint8_t nonce0[16],
                           uint32_t stream, int gauss_kind, const uint8_t* aux32, uint32_t max_rounds, int64_t* cs, int64_t* cp,
                           int64_t* ts, int64_t* tp, int64_t* u, int64_t* zs, int64_t* zp, int64_t* rs, int64_t* rp, uint8_t* ok,
                           uint8_t* rounds, uint32_t* rounds_run, size_t B);
int rzk_sum_prove_zk_batch_dev(rzk_ctx* ctx, uint32_t V, const int64_t* gs, const int64_t* xs, const uint8_t nonce0[16],
                               uint32_t stream, int gauss_kind, const uint8_t* aux32, uint32_t max_rounds, int64_t* cs, int64_t* cp,
                               int64_t* ts, int64_t* tp, int64_t* u, int64_t* zs, int64_t* zp, int64_t* rs, int64_t* rp,
                               uint8_t* ok, uint8_t* rounds, uint32_t* rounds_run, size_t B);

/* ---- 32-bit slabs: the Linear proof (v14, slab32 Linear) ----------------------------------------------------
 * The Linear cycle, its short verifier's recompute step and the stand-alone norm predicate on int32_t slabs.  Additions only:
 * RZK_ABI_VERSION stays 14 and every earlier signature is unchanged.  Each call has the argument list of the 64-bit sibling
 * named by dropping "32", with every coefficient slab an int32_t* (coin and E of the reject call stay int64_t, ok / accept
 * uint8_t); argument rules, NULL rules, B == 0, verdict bytes (the two-bit ok of the commit call included), fault reporting
 * and trusted-producer mode are the sibling's; device slabs are 16-byte aligned (RZK_E_ARG otherwise).  Every output slab is
 * narrow() of the sibling's output on widen(inputs), bit for bit; ok, accept and E are identical.
 * Native 32-bit kernels run at N = 512 and 1024, n = 1, one-wavefront teams and default rotation knobs, for calls that
 * prepare no multiplier images (RZK_DKEY=2, or l >= 2, converts) and, for rzk_linear_verify32_batch, with the rearranged
 * verifier (RZK_LIN_E=0 converts): row_kernel<., false, i32, false> runs the vector x vector programs, norm_kernel_i32 the
 * norm predicates the commit rows cannot fuse (ok not made of whole aligned 32-bit words).  A call runs natively only when
 * every program it launches does; otherwise the whole call widens its inputs, runs the sibling and narrows the outputs.  The
 * native calls keep their workspace intermediates as int32_t, in half the bytes. */
int rzk_linear_commit32_batch(rzk_ctx* ctx, const int32_t* g, const int32_t* x, const int32_t* r, const int32_t* rp,
                              const int32_t* y, const int32_t* yp, int32_t* c, int32_t* cp, int32_t* t, int32_t* tp, int32_t* u,
                              uint8_t* ok, size_t B);
int rzk_linear_commit32_batch_dev(rzk_ctx* ctx, const int32_t* g, const int32_t* x, const int32_t* r, const int32_t* rp,
                                  const int32_t* y, const int32_t* yp, int32_t* c, int32_t* cp, int32_t* t, int32_t* tp, int32_t* u,
                                  uint8_t* ok, size_t B);
int rzk_linear_mask32_batch(rzk_ctx* ctx, const int32_t* g, const int32_t* y, const int32_t* yp, int32_t* t, int32_t* tp,
                            int32_t* u, size_t B);
int rzk_linear_mask32_batch_dev(rzk_ctx* ctx, const int32_t* g, const int32_t* y, const int32_t* yp, int32_t* t, int32_t* tp,
                                int32_t* u, size_t B);
int rzk_linear_response32_batch(rzk_ctx* ctx, const int32_t* y, const int32_t* yp, const int32_t* r, const int32_t* rp,
                                const int32_t* d, int32_t* z, int32_t* zp, size_t B);
int rzk_linear_response32_batch_dev(rzk_ctx* ctx, const int32_t* y, const int32_t* yp, const int32_t* r, const int32_t* rp,
                                    const int32_t* d, int32_t* z, int32_t* zp, size_t B);
int rzk_linear_response_reject32_batch(rzk_ctx* ctx, const int32_t* y, const int32_t* yp, const int32_t* r, const int32_t* rp,
                                       const int32_t* d, const int64_t* coin, uint64_t R, double lnM, int32_t* z, int32_t* zp,
                                       uint8_t* accept, int64_t* E, size_t B);
int rzk_linear_response_reject32_batch_dev(rzk_ctx* ctx, const int32_t* y, const int32_t* yp, const int32_t* r, const int32_t* rp,
                                           const int32_t* d, const int64_t* coin, uint64_t R, double lnM, int32_t* z, int32_t* zp,
                                           uint8_t* accept, int64_t* E, size_t B);
int rzk_linear_verify32_batch(rzk_ctx* ctx, const int32_t* z, const int32_t* zp, const int32_t* c, const int32_t* cp,
                              const int32_t* g, const int32_t* t, const int32_t* tp, const int32_t* u, const int32_t* d,
                              uint8_t* accept, size_t B);
int rzk_linear_verify32_batch_dev(rzk_ctx* ctx, const int32_t* z, const int32_t* zp, const int32_t* c, const int32_t* cp,
                                  const int32_t* g, const int32_t* t, const int32_t* tp, const int32_t* u, const int32_t* d,
                                  uint8_t* accept, size_t B);
int rzk_linear_recover32_batch(rzk_ctx* ctx, const int32_t* z, const int32_t* zp, const int32_t* c, const int32_t* cp,
                               const int32_t* g, const int32_t* d, int32_t* t_out, int32_t* tp_out, int32_t* u_out,
                               uint8_t* accept, size_t B);
int rzk_linear_recover32_batch_dev(rzk_ctx* ctx, const int32_t* z, const int32_t* zp, const int32_t* c, const int32_t* cp,
                                   const int32_t* g, const int32_t* d, int32_t* t_out, int32_t* tp_out, int32_t* u_out,
                                   uint8_t* accept, size_t B);
int rzk_norm2_le32_batch(rzk_ctx* ctx, const int32_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B);
int rzk_norm2_le32_batch_dev(rzk_ctx* ctx, const int32_t* v, uint32_t rows, uint64_t bound, uint8_t* ok, size_t B);

/* diagnostic: the loop's compaction kernel on flags the caller chose.  idx[0 .. *count) = the ascending b < B with
 * live[b] != 0 && done[b] == 0; entries of idx from *count on are not written.  live, done:[B] uint8, idx:[B] uint32 and
 * count (one uint32) are device pointers; asynchronous on the context's stream.  RZK_E_ARG for NULL pointers or B >= 2^32. */
int rzk_debug_compact_dev(rzk_ctx* ctx, const uint8_t* live, const uint8_t* done, size_t B, uint32_t* idx, uint32_t* count);

/* ---- fixed-width packed records "RZKP1" (v8; batched, on the GPU) ----------------------------------------------------------
 * The bincode form above is the reference's: 8 bytes per coefficient and polynomials of variable length.  For proofs that
 * are stored and verified later this is the compact form: every record of a kind has the same size, known on the host, and
 * each coefficient takes the bits its field needs (ring_zk_amd/csrc/rzk_packed.h restates every rule).
 *   record       8-byte header, then the kind's fields in the declaration order of the RZK_MSG_* table, slabs row-major
 *   header       'R' 'Z' 'K' 'P', u8 version = 1, u8 kind, u16 V little-endian (0 for the kinds without summands)
 *   polynomial   of width W: ceil(N W / 64) little-endian 64-bit words; coefficient i is the unsigned value raw = c + bias at
 *                bits [i W, (i+1) W) of the bit string (bit j = bit j % 64 of word j / 64); bits above N W are zero
 *   class Q      c cp cs t tp ts u g gs    bias (q-1)/2          largest raw q-1               W = bitlen(q-1) = 32
 *   class Z      z zp zs                   bias verify_bound     largest raw 2 verify_bound    W = bitlen(2 verify_bound)
 *   class D      d                         bias 1                largest raw 2                 W = 2
 * Class Z loses nothing for a proof a verifier could accept: norm_2(z_i) <= verify_bound bounds every coefficient.
 * Kinds: RZK_MSG_COMMITMENT, CHALLENGE, OPEN_COMMITMENT, OPEN_RESPONSE, LINEAR_COMMITMENT, SUM_COMMITMENT, SUM_RESPONSE as
 * above, and four that exist here only (the rzk_wire_* entry points reject them):
 *   RZK_MSG_LINEAR_RESPONSE    { z, zp }       z, zp [B][k][N]
 *   RZK_MSG_OPEN_SHORT         { c, d, z }     c [B][n+l][N], d [B][N], z [B][k][N]: the signature form of an Open proof, the
 *                              verifier recomputes t = a1.z - c1 (.) d and accepts iff the transcript of (c, t) gives d again
 *   RZK_MSG_LINEAR_SHORT (v12) { c, cp, g, d, z, zp }       } the same for Linear and Sum (V summands): the full kinds' fields in
 *   RZK_MSG_SUM_SHORT    (v12) { cp, cs, gs, d, zp, zs }    } their order without t / tp / ts / u, d behind the commitment fields;
 *                              the verifier recomputes those (rzk_*_recover_batch) and hashes them under the full kind
 * RZK_MSG_OPENING is not a stored proof and is not supported; kind 10 is unassigned.
 * rzk_packed_record_bytes: size of one record; 0 = bad kind or V, or a context with verify_bound > (q-1)/2.
 * rzk_packed_widths: W of classes Q and Z.
 * rzk_packed_encode_batch: fields as for the wire codec -> records [B][record_bytes].  A coefficient outside its class's
 *   range (a non-canonical one included) is written as the all-ones value 2^W - 1, which is above every class's largest raw,
 *   and clears ok[b] of its message: a per-message verdict, not an input fault of the call, and a failed record never
 *   decodes as valid.  The test is made in trusted-producer mode too: it decides whether the value fits.
 * rzk_packed_decode_batch: ok[b] = 0 for a wrong header (magic, version, kind, V), any raw above its class's largest, or a
 *   set padding bit; slabs of a rejected record are unspecified.  One byte string per message: encoding is canonical.
 * RZK_E_ARG: bad kind (RZK_MSG_OPENING included), V == 0 or V > 65535 on a Sum kind, NULL pointers (ok included), records not
 * 8-byte aligned, _dev slabs not 16-byte aligned.  B == 0 is a no-op.  The _dev variants run on the context's stream without
 * host synchronisation or allocation; `fields` is a host array of device pointers. */
#define RZK_MSG_LINEAR_RESPONSE 8
#define RZK_MSG_OPEN_SHORT 9
#define RZK_MSG_LINEAR_SHORT 11
#define RZK_MSG_SUM_SHORT 12
size_t rzk_packed_record_bytes(const rzk_ctx* ctx, int kind, uint32_t V);
int rzk_packed_widths(const rzk_ctx* ctx, uint32_t* wq, uint32_t* wz);
int rzk_packed_encode_batch(rzk_ctx* ctx, int kind, uint32_t V, const int64_t* const* fields, uint8_t* records, uint8_t* ok,
                            size_t B);
int rzk_packed_encode_batch_dev(rzk_ctx* ctx, int kind, uint32_t V, const int64_t* const* fields, uint8_t* records,
                                uint8_t* ok, size_t B);
int rzk_packed_decode_batch(rzk_ctx* ctx, int kind, uint32_t V, const uint8_t* records, int64_t* const* fields, uint8_t* ok,
                            size_t B);
int rzk_packed_decode_batch_dev(rzk_ctx* ctx, int kind, uint32_t V, const uint8_t* records, int64_t* const* fields,
                                uint8_t* ok, size_t B);

/* ---- seed expansion "XP1": uniform elements of R_q from public seeds with SHAKE256 (v10) ------------------------------------
 * Hash-to-ring for public data: commitment keys (rzk_key_expand) and the public multipliers g / g_i of Linear and Sum proofs
 * when they are random-combination coefficients derived from a statement digest (DESIGN.md §14;
 * ring_zk_amd/csrc/rzk_xof.h restates the format and holds the scalar form).  Never for secrets: those stay with the keyed
 * samplers.
 *   CH = min(N, 256), C = N / CH; W = bitlen(q - 1), mask = 2^W - 1
 *   msg(p, c) = "RZKXP1\0U" | le64(q) | le32(N) | le32(domain) | seed[0:32] | le32(p) | le32(c)                       64 bytes
 *   stream    = SHAKE256(msg(p, c)) read as little-endian 32-bit words; a word w gives the candidate v = w & mask, accepted
 *               iff v < q, with the value v - (q-1)/2 (the centred residue)
 *   chunk c of polynomial p = the first CH accepted values, in order -> coefficients c*CH .. c*CH + CH - 1
 * Every coefficient is exactly uniform over the q residues (acceptance q / 2^W > 1/2 per word).
 * rzk_xof_uniform_batch: seeds [B][32], out [B][rows][N]; out[b][r] is polynomial p = r under seeds[b] and `domain`.
 *   domain RZK_XOF_DOMAIN_KEY (0) is reserved for keys: RZK_E_ARG.  Needs no loaded key.  RZK_E_ARG also for NULL pointers,
 *   rows == 0, and in the _dev variant seeds not 8-byte aligned or out not 16-byte aligned.  B == 0 is a no-op.  The _dev
 *   variant runs on the context's stream without host synchronisation or allocation.  There is no per-proof verdict and no
 *   input fault: every byte string is a valid seed.
 * Not claimed: constant time (the rejection loop has no fixed trip count; every input is public). */
#define RZK_XOF_DOMAIN_KEY 0
int rzk_xof_uniform_batch(rzk_ctx* ctx, const uint8_t* seeds, uint32_t domain, uint32_t rows, int64_t* out, size_t B);
int rzk_xof_uniform_batch_dev(rzk_ctx* ctx, const uint8_t* seeds, uint32_t domain, uint32_t rows, int64_t* out, size_t B);

/* HIP-event timing of the last phase call's dominant kernel is exposed through these counters:
 * accumulated microseconds and launch count of the row kernel since the last reset. */
/* diagnostic: copies the row kernels' per-wave scratch lines to the host (tools/wave_timeline.py; *total = its size) */
int rzk_debug_read_scratch(rzk_ctx* ctx, void* dst, size_t bytes, size_t* total);
/* v9.  diagnostic: the word-to-pair map of the Gaussian samplers (ring_zk_amd/csrc/rzk_gauss.h) on words the caller
 * chose, so that a test reaches the edges of the map that no seed or key produces.  words:[pairs][4] and out:[pairs][2] are
 * device pointers; pair i gets what a sampler draws from a Philox block / ChaCha20 quarter with these four words: the
 * single-precision form for f32 != 0 (sigma < 2^19; it reads three words of the four), else the double-precision form
 * (sigma <= 2^26).  Asynchronous on the context's stream; pairs == 0 returns RZK_OK. */
int rzk_debug_gauss_map_dev(rzk_ctx* ctx, int f32, const uint32_t* words, double sigma, int64_t* out, size_t pairs);
/* v11, diagnostic: one trial of the exact discrete Gaussian sampler (dgauss_trial of rzk_dgauss.h) on words the caller
 * chose.  words: device, [trials][8] (words 6 and 7 are not used); out: device, [trials][2] = (accepted 0 / 1, the
 * candidate's signed value).  sigma as rzk_sample_dgauss_keyed_dev. */
int rzk_debug_dgauss_trial_dev(rzk_ctx* ctx, uint32_t sigma, const uint32_t* words, int64_t* out, size_t trials);
int rzk_prof_reset(rzk_ctx* ctx);
int rzk_prof_enable(rzk_ctx* ctx, int on);
int rzk_prof_read(rzk_ctx* ctx, double* row_kernel_us, uint64_t* row_kernel_launches);
/* launches recorded since the last reset / read (host counter, no synchronisation), and their individual
 * durations in launch order (synchronises; does not clear) */
uint64_t rzk_prof_count(const rzk_ctx* ctx);
int rzk_prof_read_all(rzk_ctx* ctx, double* us, size_t cap, size_t* count);
/* v3.  Which kernel every recorded launch ran and its algorithmic bytes (8 N x (distinct polynomials the row program
 * reads + rows it stores) x batch entries), one "<kernel>\t<bytes>\n" line per launch in launch order; *needed = length
 * of the full text.  bench.py names the dominant kernel of every configuration with this. */
int rzk_prof_read_kernels(rzk_ctx* ctx, char* buf, size_t cap, size_t* needed);

/* ---- environment variables (read once by rzk_ctx_create) ----------------------------------------------------------
 * Testing / tuning switches, NOT part of the API contract: every setting computes the same results; they select which
 * kernel evaluates a row program so that the test-suite can reach every kernel at small shapes and so that A/B
 * measurements need no rebuild.  Defaults are what the measurements in DESIGN.md §6 chose.
 *   RZK_SHIFT=0            challenge products through transforms instead of signed rotations (default 1; at N = 2048 only
 *                          with RZK_PAIR_POLY=1, the default)
 *   RZK_SHIFT_BYTES=0|1    shift_row_kernel at N <= 1024: terms with |multiplier|_1 * 2 |operand|_inf <= 255 (every response row
 *                          z = y + r (.) d) rotate packed bytes instead of 32-bit words (default 1; 0 = words only)
 *   RZK_PAIRS=0            unit_kernel: no pairing of rows that share their last operand (default 1)
 *   RZK_UPT=<u>            unit_kernel: units of a proof per wavefront task (default: all once batch >= 16 x CUs, else 1)
 *   RZK_VEC_ROWS=0         programs with vector x vector products through unit_kernel instead of row_kernel (default 1)
 *   RZK_ROW_GROUPS=0       no row groups (row_group_kernel) for key blocks with n > 1 (default 1)
 *   RZK_GROUP_MAX=<g>      rows per group, 1 .. 4 at N <= 1024, 1 .. 2 at N = 2048 (default 4 at N <= 1024, 1 at N = 2048)
 *   RZK_BLOCK_MIN_LOGN=<L> row blocks (row_block_kernel) from ring degree 2^L on (default 11; 12 = never, 10 = also N = 1024)
 *   RZK_SLOT_SHARE_MIN=<x> shared-operand path when (operand transforms) / (distinct operands) >= x (default 2.0; 0 = never)
 *   RZK_PAIR_POLY=0        N = 2048: one wavefront per polynomial instead of two (default 1)
 *   RZK_OIMG=0             Sum proof: the rows of D = sum_i g_i v_i transform v_{i,c} themselves (default 1: they read the transforms the
 *                          a1.v_i key products of the same call left behind, where those ran on the group / block kernels)
 *   RZK_LIN_E=0            Linear verifier: the reference's grouping (a2.z)(.)g - a2.z' == (c2(.)g - c2')(.)d + u with its two products by g
 *                          (default 1: g(.)(a2.z - c2(.)d) - (a2.z' - c2'(.)d) - u == 0, one product)
 *   RZK_DKEY=0|1|2         the scalar multipliers g / g_i of the Linear / Sum proofs transformed once per proof and call into the
 *                          resident key's form: never / when at least four rows of the call multiply by each (default) / always
 *   RZK_SUM_D=0|1          Sum proof: sum_i g_i (a2.v_i) - a2.v' row by row (0) or as a2.(sum_i g_i v_i - v') (1); default: whichever
 *                          needs fewer transforms for the loaded key and V
 *   RZK_PRESET_IN_KERNEL=0 verdict flags always initialised by a fill launch (default 1: by the unit kernels themselves where one
 *                          team evaluates a whole batch entry)
 *   RZK_UNIT_IO=0|1        key-product programs without vector operands: unit_io_kernel (operands read once, per-prime sums
 *                          parked on chip) instead of unit_kernel (default 1 at N = 512, 0 otherwise)
 *   RZK_ROT_LAST=0         unit_kernel: every row's rotation terms (c1 (.) d of the verifier relation) run before the transforms and
 *                          their sum waits in the wavefront's scratch line (default 1: in single-row units of one-wavefront
 *                          teams, N <= 1024, they run after the last inverse transform and accumulate in registers)
 *   RZK_DOT2=0             unit_kernel: each key product of a row is reduced on its own (default 1: a unit of exactly two key
 *                          products into its first row parks the first transform and reduces x1 k1 + x2 k2 once; one-wavefront
 *                          teams, N <= 1024)
 *   RZK_CRT2_SHORT=0       unit kernels: the two-prime reconstruction with two reductions mod q and a 64-bit sign test
 *                          (default 1: digit compares and one reduction, crt2_zq_short)
 *   RZK_TW_LDS=0|1|2       unit_kernel at N = 1024 (one-wavefront teams, 64- and 32-bit slabs): where the per-lane (vector) twiddles of
 *                          every transform come from.  All three report the same kernel names and give the same bytes.
 *                          0: the global tables.
 *                          1 (default at N = 1024): phase 2 from an LDS image the workgroup's 256 threads copy once at kernel
 *                          entry, entries 16 .. 255 of the 3 x 2 tables in 256 words each, 6 144 bytes behind the four teams'
 *                          4 x 8 320: 39 424 bytes per workgroup, four workgroups = 4 waves per SIMD in 157 696 of a CU's
 *                          163 840 bytes; phase 3 from the global tables, the forward transform asking for them where its
 *                          phase 2 begins.
 *                          2: phases 2 and 3 from LDS.  Sixteen teams per workgroup, one workgroup per CU under the grid cap;
 *                          its 1024 threads copy entries 16 .. 1023 of the six tables once (1024 words each, 24 576 bytes
 *                          behind 16 x 8 320): the same 157 696 bytes per CU and 4 waves per SIMD.  The teams stay independent
 *                          after the one barrier behind the fill.  Measured slower than 1 (the workgroup shape costs more
 *                          than the image gains), so not the default.
 *                          Values above 2 read as 2, negative ones as 0.  No effect at other ring degrees or on the other
 *                          kernels; see DESIGN.md §6
 *   RZK_GRID_CUS=<c>       testing: size every grid cap, and the scratch behind it, for c CUs instead of the device's count
 *                          (clamped to 1 .. multiProcessorCount; 0 or a non-number gives 1), so that small batches make
 *                          several grid-stride trips.  The batch at which RZK_UPT's default switches to all units per
 *                          wavefront (16 x CUs) moves with it, so 1 CU reaches the full-batch path choice at batch >= 16
 * RZK_LIB (ring_zk_amd/_lib.py, Python only) loads another build of the library for A/B runs. */

#ifdef __cplusplus
}
#endif
#endif /* RZK_H */
