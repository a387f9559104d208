/*
 * deig.h - C ABI of libdeig.so, the MI355X (gfx950) hot path of the distributed
 * eigenspace estimator (TimeEscaper/distributed_eigenspaces).
 *
 * Every entry point takes raw device pointers, sizes and leading dimensions (in
 * elements), caller-provided device workspace and a hipStream_t (passed as
 * void*).  The library never allocates or frees device memory.  Its only
 * process-global state is thread-safe: a thread-local error string, a per-device
 * CU-count cache (atomics) and a mutex-protected free list of small pinned host
 * blocks (a few hundred bytes each, allocated on first use and kept) that the
 * eigensolvers read their per-cycle status from.  Work is enqueued on
 * the given stream; entry points that iterate (the eigensolvers) synchronise that
 * stream between sweeps to test convergence, and return when done.
 *
 * Layouts: sample matrices X are row-major n x d (row stride ldx); symmetric
 * matrices S are row-major d x d (full storage, both triangles written); bases V
 * are COLUMN-major d x k (Fortran order, column stride ldv), columns in ASCENDING
 * eigenvalue order, exactly like LAPACK ?syevr / scipy.linalg.eigh.  A stack of m
 * bases is passed as Wt = [V_1^T; ...; V_m^T], i.e. (m*k) x d row-major, which is
 * the byte layout of m column-major d x k bases laid end to end.
 *
 * Return codes: 0 ok; DEIG_NOT_CONVERGED (1) = results written but the residual
 * test did not pass within max_sweeps; negative = error (see deig_last_error()).
 */
#ifndef DEIG_H
#define DEIG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEIG_OK 0
#define DEIG_NOT_CONVERGED 1
#define DEIG_EINVAL (-1)
#define DEIG_EHIP (-2)
#define DEIG_EWORKSPACE (-3)
#define DEIG_ETIMEOUT (-4) /* a resident Oja hand-off timed out (deig_oja_error) */

/* Element types of float inputs (deig_syrk_shift, deig_syrk_centered, deig_colsum,
 * deig_topk_sym_ex). */
#define DEIG_F32 0
#define DEIG_F64 1
/* bf16 samples (deig_colsum, deig_syrk_shift, deig_syrk_centered): an element is the upper 16
 * bits of the fp32 value, as torch.bfloat16 and __bf16 store it; alignment 2 bytes.  Widening
 * is exact, so these entry points return the bits they return for the fp32 copy. */
#define DEIG_BF16 2
/* Raw bytes (uint8), one feature per byte: element type of deig_oja_steps_centered,
 * deig_gram_apply and deig_topk_samples only (the covariance and transform uint8 entry points
 * take their own DEIG_U8_* modes); alignment 4 bytes. */
#define DEIG_U8 3

/* Library version, e.g. 0x000400 for 0.4.0.  A caller built against an older header
 * should compare it with the version it was built for before binding entry points
 * whose signature changed (deig_topk_sym_batch: see below).  The uint8 centred-PCA entry
 * points (deig_colsum_u8, deig_syrk_u8_centered, deig_pca_transform_u8 and their workspace
 * queries) are additive: they came without a version change (0x000600), so probe for the
 * symbols rather than for a version. */
int deig_version(void);

/* Release the library's process-lifetime host resources (the pinned per-cycle status
 * blocks of the eigensolvers) after synchronising the current device.  Optional; call
 * it at process exit BEFORE the HIP runtime is torn down (the Python binding registers
 * it with atexit, which runs before the C runtime's exit handlers).  No solver may be
 * running; later solver calls allocate new blocks. */
void deig_shutdown(void);

/* Thread-local message for the last nonzero return on this thread ("" if none). */
const char* deig_last_error(void);

/* Covariance algorithms (deig_syrk_f32_ex):
 *  DEIG_SYRK_SPLIT3: each fp32 sample split once into bf16 hi + lo; products
 *    from 3 bf16 MFMAs (hi*hi + hi*lo + lo*hi), fp32 accumulation, the dropped
 *    lo*lo term restored exactly on the diagonal.  Per-product error <= ~3*2^-16
 *    relative, zero-mean, so it averages out over rows: max |S - S_f64| / max|S|
 *    ~1e-6 at n = 512, ~2e-7 at n >= 32k (fp32 kernel: ~1e-7..2e-6), at 16/3 x
 *    the f32 MFMA rate.
 *  DEIG_SYRK_FP32: v_mfma_f32_32x32x2_f32 (exact fp32 fma chain).
 *  DEIG_SYRK_AUTO (default): SPLIT3 for n >= DEIG_SYRK_SPLIT_MIN_ROWS, else FP32. */
#define DEIG_SYRK_AUTO 0
#define DEIG_SYRK_SPLIT3 1
#define DEIG_SYRK_FP32 2
#define DEIG_SYRK_DEFAULT DEIG_SYRK_AUTO
#define DEIG_SYRK_SPLIT_MIN_ROWS 1024
/* OR-ed into the algorithm of deig_syrk_f32_ex (SPLIT3 only): S += alpha X^T X -
 * one covariance streamed through in row blocks (e.g. a shard larger than HBM). */
#define DEIG_SYRK_ACCUMULATE 0x100

/* Sigma_hat = alpha * X^T X  (alpha = 1/n reproduces the reference).
 * Replaces SlaveNode.compute_sigma_hat_  distributed.py:59-70
 * (np.zeros((d,d)) += np.dot(x.T, x); /= n  ->  OpenBLAS dsyrk).
 * fp32 in, fp32 accumulate (DEIG_SYRK_DEFAULT); output is bit-exactly symmetric.
 * Requires n >= 1, d % 4 == 0, ldx % 4 == 0, lds % 4 == 0, 16-byte aligned X, S.
 * The workspace query returns the recommended size; SPLIT3 works on row chunks
 * that fit the workspace given (more workspace -> fewer, larger chunks). */
int deig_syrk_f32(const float* X, int64_t n, int64_t d, int64_t ldx, float alpha,
                  float* S, int64_t lds, void* ws, size_t ws_bytes, void* stream);
size_t deig_syrk_workspace(int64_t n, int64_t d);
/* Same with an explicit algorithm (DEIG_SYRK_*). */
int deig_syrk_f32_ex(const float* X, int64_t n, int64_t d, int64_t ldx, float alpha,
                     float* S, int64_t lds, int algo, void* ws, size_t ws_bytes, void* stream);
size_t deig_syrk_workspace_ex(int64_t n, int64_t d, int algo);

/* Covariance of bf16 samples taken as they are:  S = alpha X^T X,  or  S += alpha X^T X  with
 * flags = DEIG_SYRK_ACCUMULATE (any other flag bit: DEIG_EINVAL).  No fp32 copy of X is made:
 * the workspace holds a bf16 image of one row chunk in MFMA operand order and fp32 partials.
 * X: n x d row-major bf16 (DEIG_BF16 elements), 16-byte aligned, n >= 1, d % 8 == 0 (d <=
 * 32768), ldx % 8 == 0, ldx >= d; no element behind column d of a row is read.  S: fp32,
 * 16-byte aligned, lds >= d, lds % 4 == 0; both triangles are written from one value, so S is
 * bit-exactly symmetric (when accumulating, the lower triangle of the incoming S is the one
 * that is read).
 * Contract: a bf16 x bf16 product has 16 significant bits and is exact in fp32, so every
 * product is exact (one v_mfma_f32_16x16x32_bf16 per fragment pair; no hi/lo split, no
 * diagonal correction), and S differs from the exact sum only by the fp32 summation.  That
 * is two-level: an MFMA accumulator takes at most 16384 rows (in K-steps of 32) before it is
 * written out as a partial, and the partials (and the incoming S) are added in a fixed order:
 * about (16384 / 32 + n / 16384) eps in the worst case relative to sum_r |x_ri x_rj|, random
 * walk ~sqrt of that in practice.  Integer data whose partial sums stay below 2^24 give the
 * exact result.  Inputs whose products underflow the fp32 normal range are outside the
 * contract.
 * Workspace: the query returns the recommended size.  Any workspace of at least
 * deig_syrk_bf16_workspace(n', d) bytes for some 1 <= n' <= n is accepted and makes the call
 * run in row chunks; a smaller one is DEIG_EWORKSPACE.  The workspace may hold anything on
 * entry.  Asynchronous on `stream`: no allocation, no synchronisation, no float atomics;
 * repeated calls give identical bits.  Argument errors are DEIG_EINVAL before any GPU work.
 * Additive, like the uint8 entry points: probe for the symbols, deig_version() is unchanged. */
int deig_syrk_bf16(const void* X, int64_t n, int64_t d, int64_t ldx, float alpha,
                   float* S, int64_t lds, int flags, void* ws, size_t ws_bytes, void* stream);
size_t deig_syrk_bf16_workspace(int64_t n, int64_t d);

/* Mean-shifted covariance of float samples, float64 result (the reference's own
 * float64 data flow: distributed.py:169-173 grey values -> compute_sigma_hat_
 * :59-70):  S64 = alpha * X^T X  computed as
 *   alpha [ C^T C + s mu^T + mu s^T + n mu mu^T ],  mu = column means (double),
 *   C = fl32(X - mu), s = sum_r (x_r - mu) (double)
 * with C^T C on the split3 / fp32 SYRK (n >= / < DEIG_SYRK_SPLIT_MIN_ROWS): the
 * SYRK's rounding is then relative to the CENTRED data, not to the mean direction
 * that dominates an uncentered covariance of byte images (see shift.hip for the
 * measured effect on the top-k basis).  X: n x d row-major, element type xtype
 * (DEIG_F32 / DEIG_F64 / DEIG_BF16), row stride ldx elements, aligned to its element size.
 * S64 (float64, lds64) and/or S (its fp32 rounding, lds) may be NULL (not both);
 * both triangles are written (bit-exact symmetry).
 * Workspace: deig_syrk_shift_workspace(n, d, xtype) (holds an fp32 copy of C). */
int deig_syrk_shift(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, double alpha,
                    double* S64, int64_t lds64, float* S, int64_t lds, void* ws, size_t ws_bytes,
                    void* stream);
size_t deig_syrk_shift_workspace(int64_t n, int64_t d, int xtype);

/* Column sums in double: sums[j] = sum_r X[r][j] (the first pass of deig_syrk_shift as an
 * entry point of its own; a multi-GPU centred fit all-reduces these into the pooled mean).
 * X: n x d row-major of element type xtype (DEIG_F32 / DEIG_F64 / DEIG_BF16), row stride ldx, aligned
 * to its element size; sums: d doubles on the device.  The rows are summed in a fixed
 * order (min(n, 128) row groups, then the groups in order), so the result is
 * deterministic.  Asynchronous on `stream`, no allocation, no synchronisation. */
int deig_colsum(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, double* sums, void* ws,
                size_t ws_bytes, void* stream);
size_t deig_colsum_workspace(int64_t n, int64_t d);

/* Centred covariance (opt-in; the reference never centres):
 *   S64 = alpha * sum_r (x_r - c)(x_r - c)^T,
 * c = center (d doubles on the device; NULL = the shard's own mean mu).  It is the
 * deig_syrk_shift pipeline with delta = mu - c where that one uses mu:
 *   alpha [ C^T C + s delta^T + delta s^T + n delta delta^T ],  C = fl32(X - mu),
 * so the SYRK still runs on data centred about the shard's OWN mean (its rounding stays on
 * the centred scale for any c) and the rank-one terms are added in double from symmetric
 * expressions.  deig_syrk_shift is exactly the case c = 0: a zero `center` gives its bits.
 * A pooled mean as c makes the covariances of several shards add up to the pooled centred
 * covariance (weights n_i / N with alpha = 1 / n_i).  mean_out (optional, d doubles on the
 * device): mu.  X, S64, S as for deig_syrk_shift.  Like it, the workspace
 * (deig_syrk_centered_workspace) holds an fp32 copy of the shard.  Asynchronous on `stream`,
 * no allocation, no synchronisation; argument errors are DEIG_EINVAL before any GPU work. */
int deig_syrk_centered(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx,
                       const double* center, double alpha, double* S64, int64_t lds64, float* S,
                       int64_t lds, double* mean_out, void* ws, size_t ws_bytes, void* stream);
size_t deig_syrk_centered_workspace(int64_t n, int64_t d, int xtype);

/* Exact covariance of uint8 samples (fused ingest):
 *   S = alpha * V^T V,  V the n x d feature matrix of
 *   DEIG_U8_RAW:   v = x, the first d bytes of each row (e.g. raw CIFAR rows, d = 3072);
 *   DEIG_U8_GRAY3: v = (r + g + b) / 3 of d interleaved 3-byte pixels (row needs 3d
 *                  bytes) - the reference's grayscale + flatten, distributed.py:170-173
 *                  (data.mean(axis=3), reshape), fused into the covariance.
 * Replaces compute_sigma_hat_ (distributed.py:59-70) on the uint8 CIFAR bytes of
 * load_data.py:18-33 (alpha = 1/n reproduces the reference).  Every product and
 * sum is exact (int8 MFMA with int32 accumulation, int64 combination), so S64 is the
 * reference's float64 result rounded once (alpha = 1/n: one division of the exact
 * integer sum) and S its fp32 rounding (within 1 ulp of the correctly rounded
 * value); either may be NULL (not both); both triangles are
 * written (bit-exact symmetry).  Requires d % 4 == 0, d <= 32768, ldx % 4 == 0 bytes,
 * X 4-byte aligned.  Workspace: deig_syrk_u8_workspace(n, d, mode). */
#define DEIG_U8_RAW 0
#define DEIG_U8_GRAY3 1
int deig_syrk_u8(const uint8_t* X, int64_t n, int64_t d, int64_t ldx, int mode, double alpha,
                 float* S, int64_t lds, double* S64, int64_t lds64, void* ws, size_t ws_bytes,
                 void* stream);
size_t deig_syrk_u8_workspace(int64_t n, int64_t d, int mode);

/* Column sums of the uint8 features in double: sums[j] = sum_r v_rj, v as for deig_syrk_u8
 * (mode, rows, ldx and alignment rules as there; any d % 4 == 0).  The accumulation is in
 * integers (one exact integer add per row, in any order: deterministic): DEIG_U8_RAW gives
 * the exact integer sum, DEIG_U8_GRAY3 the integer sum of r + g + b divided by 3, rounded
 * once.  sums: d doubles on the device.  The input of the pooled-mean all-reduce of a centred
 * fit, as deig_colsum is for floats.  Asynchronous on `stream`, no allocation, no
 * synchronisation; argument errors are DEIG_EINVAL and a short workspace DEIG_EWORKSPACE
 * before any GPU work. */
int deig_colsum_u8(const uint8_t* X, int64_t n, int64_t d, int64_t ldx, int mode, double* sums,
                   void* ws, size_t ws_bytes, void* stream);
size_t deig_colsum_u8_workspace(int64_t n, int64_t d);

/* Centred covariance of uint8 samples (opt-in, as deig_syrk_centered is for floats):
 *   S = alpha * sum_r (v_r - c)(v_r - c)^T,   v as for deig_syrk_u8 (same X, n, d, ldx, mode
 * rules, n <= 2^40), c = center: d doubles on the device in units of v, NULL = the shard's own
 * mean.  mean_out (optional, d doubles on the device) receives the own mean.  S (fp32) and/or
 * S64 may be requested, not neither; both triangles are written from the same lower-triangle
 * value (bit-exact symmetry) and S is S64's double rounded to float.
 * The deig_syrk_u8 pipeline with centred epilogues: from the integers it already holds -
 * A_ij = sum y_i y_j and Y_i = sum y_i of the offset values y (raw: x - 128; gray:
 * r + g + b - 384) -
 *   s^2 sum (v - c)(v - c)^T = (n A_ij - Y_i Y_j) / n + e_i e_j / n,     s = 1 (raw), 3 (gray),
 *   e_i = fma(-s n, c_i, Y_i + off n),  off = 128 (raw), 384 (gray);  e = 0 for center == NULL.
 * The numerator n A_ij - Y_i Y_j is formed exactly in 128-bit integers (either term passes
 * 2^63 from n ~ 2^25 while the difference stays small) and e_i is rounded once, relative to
 * itself (both of the fma's integer operands are exact doubles).
 * Accuracy contract, with u = 2^-53 and B_ij = (n A_ij - Y_i Y_j) / n exactly:
 *   |S64_ij - exact_ij| <= 8 u (alpha / s^2) (|B_ij| + |e_i e_j| / n),
 * "exact" being the rational value for the `center` and `alpha` doubles as given.  The 8
 * counts roundings: the B term sees numerator -> double, / n, the sum, / s^2, * alpha (5); the
 * e term sees e_i, e_j, their product, / n, the sum, / s^2, * alpha (7); (1 + u)^7 - 1 < 8 u.
 * Workspace: deig_syrk_u8_centered_workspace(n, d, mode) (>= deig_syrk_u8_workspace: the d
 * centre terms more).  Asynchronous on `stream`, no allocation, no synchronisation; argument
 * errors are DEIG_EINVAL and a short workspace DEIG_EWORKSPACE before any GPU work. */
int deig_syrk_u8_centered(const uint8_t* X, int64_t n, int64_t d, int64_t ldx, int mode,
                          const double* center, double alpha, float* S, int64_t lds, double* S64,
                          int64_t lds64, double* mean_out, void* ws, size_t ws_bytes, void* stream);
size_t deig_syrk_u8_centered_workspace(int64_t n, int64_t d, int mode);

/* Subspace size the solvers use for a given k when the caller passes p <= 0. */
int deig_default_subspace(int64_t d, int k);

/* Sweep algorithms for the symmetric S*Q product of the eigensolver:
 *  DEIG_SWEEP_BF16X6: S rows and Q split into three bf16 pieces in registers
 *    (x = h + m + l), 6 bf16 MFMA products per fp32 product (every term down to
 *    2^-16 |ab|), fp32 accumulation - fp32-grade products, HBM-bound on the 4 d^2
 *    bytes of S for every p <= 128;
 *  DEIG_SWEEP_FP32: f32 MFMA skinny kernel (exact fp32 fma chain, f32-MFMA-bound
 *    above p ~ 40);
 *  DEIG_SWEEP_AUTO: BF16X6 (the solvers' default; deig_solver_opts.sweep_algo). */
#define DEIG_SWEEP_AUTO 0
#define DEIG_SWEEP_BF16X6 1
#define DEIG_SWEEP_FP32 2
/* OR-ed into the algorithm of deig_sym_apply_f32 (BF16X6 only): the workspace
 * already holds the sweep image of this S from an earlier call with the same
 * S, d, p and workspace, so the re-layout pass is skipped (repeated products
 * with one S, as the solver does). */
#define DEIG_SWEEP_PREPARED 0x100
/* OR-ed into the algorithm of deig_sym_apply_f32 (BF16X6 only): the solver's
 * mode.  Q (then written in place) is rounded to Q' = h + m, its two leading
 * bf16 pieces (16 significant bits, |Q' - Q| <= 2^-17 |Q|), and Y = alpha S Q'
 * is formed to fp32 grade from five bf16 MFMA products instead of six. */
#define DEIG_SWEEP_ROUND_Q 0x200
/* OR-ed into the algorithm of deig_sym_apply_f32 (BF16X6 only; implies ROUND_Q):
 * the solver's early-sweep mode.  S is also taken as its two leading bf16 pieces
 * (from a two-piece image written by the same prepare pass), so Y = alpha S' Q' is
 * three bf16 MFMA products (hh + hm + mh) with no split in the sweep: ~2^-16
 * relative (S' rounding 2^-17, dropped m m 2^-18).  deig_topk_sym_f32 uses it while
 * its residual is above 1e-3 (after the one-product HALF sweeps above 1e-2), ROUND_Q
 * down to 1e-4, the exact product below. */
#define DEIG_SWEEP_FAST 0x400
/* OR-ed into the algorithm of deig_sym_apply_f32 / deig_sym_power_f32 (BF16X6 only;
 * implies FAST): the solver's first sweeps.  S and Q are both taken as their leading
 * bf16 piece alone (the h slots of the two-piece image: half its bytes), one bf16
 * MFMA product per fragment pair, ~2^-9 relative.  Needs p >= 64 (below, the FAST
 * mode runs).  deig_topk_sym_f32 uses it while its residual is above
 * deig_solver_opts.half_until (1e-2). */
#define DEIG_SWEEP_HALF 0x1000
/* OR-ed into the algorithm of deig_sym_apply_f32 (BF16X6 only; measurement):
 * launch the sweep kernel alone on the Q image that the previous call with the
 * same workspace, d, p and mode left - no split of Q, no split-K reduction, Y is
 * not written.  Timing such calls gives the sweep kernel's own duration. */
#define DEIG_SWEEP_KERNEL_ONLY 0x800

/* One subspace-iteration sweep Y = alpha * S Q  (S symmetric d x d row-major, lds;
 * Q d x p row-major, ldq; Y d x p row-major, ldy; p % 16 == 0, 16 <= p <= 128).
 * The S*Q product inside deig_topk_sym_f32, exposed for measurement and reuse.
 * Leading dimensions and alignment, all checked before any GPU work (DEIG_EINVAL):
 *  S: 16-byte aligned, lds >= d, lds % 4 == 0 (both algorithms);
 *  DEIG_SWEEP_BF16X6 / AUTO: any ldq >= p and ldy >= p, element alignment of Q and Y
 *    (ROUND_Q / FAST / HALF write the rounded Q back through ldq);
 *  DEIG_SWEEP_FP32: d % 4 == 0, Q 16-byte aligned with ldq % 4 == 0; any ldy >= p.
 * No element behind column d of an S row or column p of a Q row is read, none behind
 * column p of a Y (or Q) row is written. */
int deig_sym_apply_f32(const float* S, int64_t d, int64_t lds, const float* Q, int p,
                       int64_t ldq, float* Y, int64_t ldy, float alpha, int algo, void* ws,
                       size_t ws_bytes, void* stream);
size_t deig_sym_apply_workspace(int64_t d, int p, int algo);

/* `steps` sweeps of the solver's power chain (the sweeps between two Rayleigh-Ritz
 * steps of deig_topk_sym_f32): for i = 0 .. steps-1:  Y = S Q;  Q_j <- cs_j Y_j
 * for every column with cs_j > 0 (the others keep Q_j).  cs: p floats in device
 * memory.  Each basis step is fused into the sweep's split-K reduction together
 * with the next sweep's Q image, as inside the solver, so the time per step is
 * the solver's cost per sweep.  On return Y = S Q_{steps-1} and Q = Q_steps
 * (ROUND_Q / FAST: every Q rounded to two bf16 pieces as for deig_sym_apply_f32).
 * algo: DEIG_SWEEP_BF16X6 / AUTO with the PREPARED / ROUND_Q / FAST flags; the
 * workspace is deig_sym_apply_workspace's.  Extends the sweep entry point (no
 * reference counterpart: the reference solves with LAPACK, distributed.py:22-29).
 * The fused step moves rows of Q and Y as 16-byte vectors: Q and Y must be 16-byte
 * aligned with ldq % 4 == 0 and ldy % 4 == 0 (ldq, ldy >= p; S as for
 * deig_sym_apply_f32); anything else is DEIG_EINVAL before any GPU work. */
int deig_sym_power_f32(const float* S, int64_t d, int64_t lds, float* Q, int p, int64_t ldq,
                       float* Y, int64_t ldy, const float* cs, int steps, int algo, void* ws,
                       size_t ws_bytes, void* stream);

/* Options of the eigensolvers (deig_topk_sym_ex, deig_projavg_topk_ex).  Fill with
 * deig_solver_opts_init() and change fields; NULL options = the defaults.  These
 * replace the r02 environment knobs: the library reads no environment variables. */
typedef struct deig_solver_opts {
  int size;                  /* sizeof(deig_solver_opts), set by deig_solver_opts_init */
  int sweep_algo;            /* DEIG_SWEEP_AUTO (bf16x6 sweeps over an image of S) or
                                DEIG_SWEEP_FP32 (f32-MFMA skinny products; float32 S only) */
  int rr_every;              /* sweeps per Rayleigh-Ritz step before the Chebyshev filter
                                starts (0: 4 with >= 16 guard columns, else 2) */
  int chebyshev;             /* 1 (default): Chebyshev filter once resid <= cheb_above */
  float cheb_above;          /* < 0 (default): 1.0 - the filter from the first Rayleigh-Ritz
                                step on - for a single-block solve of an explicit S (k <= 128)
                                on a basis without guard columns (p - k < 4), else 1e-2 */
  int deflate;               /* 1 (default): lock dominant pairs (theta_1 >= 64 theta_k) and
                                iterate the rest on the deflated operator */
  int deflate_early;         /* 1 (default): lock them as soon as they are converged */
  int jacobi_early_sweeps;   /* Jacobi sweeps of early Rayleigh-Ritz steps (-1: 2 explicit S,
                                3 projector average; 0: uncapped) */
  float jacobi_early_above;  /* residual above which the cap applies (< 0: 1e-4 / 1e-2) */
  float fast_until;          /* three-product sweeps while resid > this (1e-3; 0: never) */
  float round_until;         /* five-product sweeps while resid > this (1e-4) */
  int debug;                 /* 1: per-Rayleigh-Ritz trace on stderr */
  float half_until;          /* one-product sweeps (DEIG_SWEEP_HALF) while resid > this,
                                for d >= 2048 and p >= 64 (1e-2; 0: never) */
} deig_solver_opts;
void deig_solver_opts_init(deig_solver_opts* opts);

/* Top-k eigenpairs of a dense symmetric S (d x d, row-major, lds), ascending.
 * Replaces Node.top_k_eigenvectors  distributed.py:22-29
 * (scipy.linalg.eigh(S, eigvals=(d-k, d-1))[1]  ->  LAPACK dsyevr), plus the
 * eigenvalues ([0] of the same call) as a side output.
 * Any d >= 1, any 1 <= k <= d and any symmetric S, like ?syevr.  S is read in place
 * when d % 4 == 0, d >= 16 and the subspace fits in d (then lds % 4 == 0 and a 16-byte
 * aligned S are required); otherwise it is staged as a zero-padded copy in the
 * workspace (any lds >= d, element alignment) whose padding never enters the
 * iteration or the result (deig_topk_workspace_ex accounts for it).
 * Block subspace iteration with Rayleigh-Ritz on a p-dimensional subspace
 * (k <= p <= 128, p % 16 == 0, p <= d; k > 128: blocks of p - 16 pairs on a p-column
 * subspace, p = 128 by default, each block's pairs LOCKED and deflated out of S for
 * the blocks below); between Rayleigh-Ritz steps a scaled Chebyshev filter on [0, c]
 * (c from the Ritz values; power steps while the residual is above 1e-2).  An
 * indefinite S is detected by the Ritz values (a negative one of significant size)
 * and solved as S + sigma I (the eigenvalues returned are S's).  When theta_1 >=
 * 64 theta_k (an uncentered covariance's mean direction), the dominant pairs are
 * locked and the others iterated on S - V_D L_D V_D^T (formed in double: fp32
 * products S q would otherwise lose their digits to cancellation).  Q0 (d x k0
 * column-major, ldq0) is an optional warm start for k <= 128 (NULL / k0 = 0 ->
 * deterministic pseudo-random start).  Stops when
 * max_j ||S v_j - lambda_j v_j|| <= tol * |lambda_max| (or the residual stalls
 * within 4 tol / 2e-6 of it, the fp32 floor); returns DEIG_NOT_CONVERGED after
 * max_sweeps sweeps (per block), or earlier when it stalls above that floor.
 * Outputs: V (d x k col-major, ldv), evals (k, ascending), *sweeps_out,
 * *resid_out = final max relative residual (host pointers, may be NULL).
 * Leading dimensions: any ldv >= d and any ldq0 >= d with element alignment of V and Q0
 * (nothing behind row d of a column is read or written; an ldv % 4 != 0 or a V that is
 * not 16-byte aligned only moves the final Rayleigh quotients of a float32 S from the
 * f64-MFMA kernel to the plain one: same accuracy, not the same bits).  That holds for
 * deig_solver_opts.sweep_algo = DEIG_SWEEP_FP32 as well: it has no image of S to deflate,
 * so it iterates on a d x d fp32 copy of S - V_D L_D V_D^T (+ sigma I) in the workspace,
 * formed in double like the image (a float64 S with that option is DEIG_EINVAL before any
 * GPU work). */
int deig_topk_sym_f32(const float* S, int64_t d, int64_t lds, int k, int p,
                      int max_sweeps, float tol, const float* Q0, int k0, int64_t ldq0,
                      float* V, int64_t ldv, float* evals, int* sweeps_out,
                      float* resid_out, void* ws, size_t ws_bytes, void* stream);
size_t deig_topk_workspace(int64_t d, int k, int p);
/* The same for S of element type stype (DEIG_F32 / DEIG_F64: a float64 S - the
 * reference's dtype - is read in double by the image pass and the deflation, so
 * the small eigenvectors of an uncentered covariance keep float64 parity), with
 * options (NULL: defaults). */
int deig_topk_sym_ex(const void* S, int stype, int64_t d, int64_t lds, int k, int p, int max_sweeps,
                     float tol, const float* Q0, int k0, int64_t ldq0, float* V, int64_t ldv,
                     float* evals, int* sweeps_out, float* resid_out, const deig_solver_opts* opts,
                     void* ws, size_t ws_bytes, void* stream);
size_t deig_topk_workspace_ex(int64_t d, int k, int p, int stype, const deig_solver_opts* opts);

/* Server solve: top-k eigenpairs of  scale * sum_i V_i V_i^T  without forming it.
 * Wt = [V_1^T; ...; V_m^T] is (mk) x d row-major (ldw); scale = 1/batches_number.
 * Replaces MasterNode.callback_  distributed.py:126-130 (sigma_tilde += V V^T;
 * /= batches_number) + the notebook's server solve (Online Distributed
 * PCA.ipynb raw line 306: top_k_eigenvectors(segma_bar, k)).  Same solver and
 * outputs as deig_topk_sym_f32; the operator is Q -> scale * Wt^T (Wt Q). */
int deig_projavg_topk_f32(const float* Wt, int64_t d, int64_t mk, int64_t ldw,
                          float scale, int k, int p, int max_sweeps, float tol,
                          const float* Q0, int k0, int64_t ldq0, float* V, int64_t ldv,
                          float* evals, int* sweeps_out, float* resid_out, void* ws,
                          size_t ws_bytes, void* stream);
/* W independent top-k problems (the logical workers of one GPU: same d, k, p and
 * element type; S[i] row-major with leading dimension lds, 16-byte aligned),
 * advanced in lockstep: equivalent to W deig_topk_sym_ex calls with the same
 * options (same kernels, same decisions; V[i] column-major with ldv, evals[i]
 * ascending, sweeps_out[i] / resid_out[i] as there), but each step of all problems
 * is enqueued as batched launches on `stream` (the sweeps of all problems at the same
 * point of their plans in one launch per kernel, one Gram, one small-solve launch of
 * one workgroup per problem, one update) and one stream sync serves every problem's
 * host decisions; for d >= 2048 the problems run as two interleaved groups, the second
 * on an internal stream created for the call that waits for `stream` on entry and
 * that `stream` waits for on return.  All work is ordered on `stream`.  Workspace:
 * deig_topk_batch_workspace(W, ...) bytes.  Returns the first error;
 * DEIG_NOT_CONVERGED if any problem stopped above tol.  status_out[i] (host array,
 * may be NULL): problem i's own return code, the one deig_topk_sym_ex would have
 * returned for it.
 * Replaces W concurrent Node.top_k_eigenvectors calls (distributed.py:22-29, one
 * per SlaveNode shard :42-53). */
size_t deig_topk_batch_workspace(int W, int64_t d, int k, int p, int stype,
                                 const deig_solver_opts* opts);
int deig_topk_sym_batch_ex(int W, const void* const* S, int stype, int64_t d, int64_t lds, int k, int p,
                           int max_sweeps, float tol, float* const* V, int64_t ldv,
                           float* const* evals, int* sweeps_out, float* resid_out, int* status_out,
                           const deig_solver_opts* opts, void* ws, size_t ws_bytes, void* stream);
/* The r03 (0x000300) signature, unchanged: deig_topk_sym_batch_ex with
 * status_out = NULL.  streams: ignored since 0x000400 (r03 ran one stream per
 * problem; may be NULL).  (0x000400 had inserted status_out into THIS signature, an
 * in-place ABI break; 0x000500 restores it and moves status_out to the _ex form.  A
 * binary built against the 0x000400 header links but passes status_out where opts is
 * read: check deig_version() >= 0x000500 before calling, or call the _ex form.) */
int deig_topk_sym_batch(int W, const void* const* S, int stype, int64_t d, int64_t lds, int k, int p,
                        int max_sweeps, float tol, float* const* V, int64_t ldv, float* const* evals,
                        int* sweeps_out, float* resid_out, const deig_solver_opts* opts, void* ws,
                        size_t ws_bytes, void* const* streams, void* stream);

size_t deig_projavg_workspace(int64_t d, int64_t mk, int k, int p);
/* With options (k > 128: block locking with the locked pairs deflated by products
 * with them - the operator stays implicit).  Wt: 16-byte aligned, ldw >= d, ldw % 4 == 0,
 * d % 4 == 0, d >= 16.  V: any ldv >= d and element alignment for k <= 128; for k > 128
 * the products with the locked pairs read V itself, which must then be 16-byte aligned
 * with ldv % 4 == 0 (DEIG_EINVAL before any GPU work otherwise; deig_projavg_topk_f32
 * alike).  Q0: any ldq0 >= d. */
int deig_projavg_topk_ex(const float* Wt, int64_t d, int64_t mk, int64_t ldw, float scale, int k,
                         int p, int max_sweeps, float tol, const float* Q0, int k0, int64_t ldq0,
                         float* V, int64_t ldv, float* evals, int* sweeps_out, float* resid_out,
                         const deig_solver_opts* opts, void* ws, size_t ws_bytes, void* stream);
size_t deig_projavg_workspace_ex(int64_t d, int64_t mk, int k, int p, const deig_solver_opts* opts);

/* Procrustes-aligned average of m bases (Charisopoulos, Benson, Damle: "Communication-
 * efficient distributed eigenspace estimation"), the one-pass alternative to the
 * projector-average server above (not in the reference; deig_projavg_topk stays the
 * reference's aggregator):
 *   V = orth( sum_i w_i V_i Z_i ),  Z_i = argmin_{Z in O(k)} ||V_i Z - R||_F = U W^T
 *   for V_i^T R = U diag(c) W^T (c = cosines of the principal angles, descending).
 * orth is the Loewdin (symmetric) orthonormalisation X (X^T X)^(-1/2), applied twice: the
 * orthonormal basis closest to the average, so V keeps the COLUMNS of the reference R
 * (column-wise eigenvector estimates), not only the span.  No eigensolve: two passes over
 * Wt and m + 2 small k x k Jacobi SVDs per pass.
 * Wt: the stack of deig_projavg_topk_f32, (mk) x d row-major (ldw), m = mk / k bases, read
 * only.  Vref: the reference basis R, d x k column-major (ldref), NULL = V_1.  weights: m
 * HOST floats >= 0, not all zero (only their ratios matter), NULL = equal; they are read
 * before the call returns.  iters in 1..8: pass t > 1 aligns to pass t-1's V.  Outputs
 * (device): V d x k column-major (ldv); Z (m x k x k row-major, Z_i of the last pass) and
 * cosines (m x k, descending, last pass) may be NULL.
 * Degenerate cosines: a singular value below 1e-5 c_max contributes no term to Z_i, which
 * is then a partial isometry - the result stays finite (never NaN) and that worker
 * contributes nothing along a direction of R it does not see.
 * Requires 1 <= k <= 128 (above, the projector-average server remains the way), k <= d,
 * mk a positive multiple of k, d % 4 == 0, ldw % 4 == 0, ldw >= d, 16-byte aligned Wt;
 * anything else is DEIG_EINVAL before any GPU work.  Asynchronous on `stream`: no
 * allocation, no synchronisation; repeated calls give bit-identical results. */
int deig_procrustes_avg_f32(const float* Wt, int64_t d, int64_t mk, int64_t ldw, int k,
                            const float* Vref, int64_t ldref, const float* weights, int iters,
                            float* V, int64_t ldv, float* Z, float* cosines, void* ws,
                            size_t ws_bytes, void* stream);
size_t deig_procrustes_workspace(int64_t d, int64_t mk, int k);

/* Distance of the spans of two orthonormal bases A, B (d x k column-major, lda / ldb):
 * out[0] = ||sin Theta(A,B)||_F, out[1] = ||sin Theta(A,B)||_2 (device, 2 floats), from the
 * residual form R = B - A (A^T B): out[0] = ||R||_F, out[1] = sqrt(lambda_max(R^T R)).
 * Unlike the cosine forms (k - ||A^T B||_F^2, singular values of A^T B) it resolves
 * distances far below 1e-3 in fp32.  ||P_A - P_B||_F = sqrt(2) out[0].
 * Requires 1 <= k <= 128, k <= d, d % 4 == 0, lda % 4 == 0, 16-byte aligned A.
 * Asynchronous on `stream`, no allocation, no synchronisation. */
int deig_subspace_dist_f32(const float* A, int64_t lda, const float* B, int64_t ldb,
                           int64_t d, int k, float* out, void* ws, size_t ws_bytes, void* stream);
size_t deig_subspace_dist_workspace(int64_t d, int k);

/* One mini-batch Oja step (online variant, BASELINE.json config 4; not in the
 * reference - parity unpinned):  V <- orth(V + eta/b * Xb^T (Xb V)).
 * Xb is b x d row-major (ldx), V is d x k column-major (ldv), updated in place.
 * k <= 64.  Orthonormalisation: Cholesky-QR2.
 * Requires d % 4 == 0, Xb 16-byte aligned with ldx >= d, ldx % 4 == 0; any ldv >= d and
 * element alignment of V (the same for deig_oja_steps_f32 / deig_oja_steps_ex).  Nothing
 * behind column d of an Xb row is read, nothing behind row d of a V column is touched. */
int deig_oja_step_f32(const float* Xb, int64_t b, int64_t d, int64_t ldx, float eta,
                      float* V, int k, int64_t ldv, void* ws, size_t ws_bytes,
                      void* stream);
size_t deig_oja_workspace(int64_t b, int64_t d, int k);

/* nb consecutive Oja steps over the batches X[i*b:(i+1)*b] (X: (nb*b) x d row-major,
 * ldx), V updated in place.  The basis is re-orthonormalised (CholQR2) every
 * orth_every batches and after the last one: the update is linear in V, so the
 * span after each batch equals that of per-batch orthonormalisation.  Same
 * workspace as deig_oja_step_f32 (deig_oja_workspace(b, d, k)). */
int deig_oja_steps_f32(const float* X, int64_t nb, int64_t b, int64_t d, int64_t ldx, float eta,
                       float* V, int k, int64_t ldv, int orth_every, void* ws, size_t ws_bytes,
                       void* stream);

/* deig_oja_steps_f32 with the algorithm chosen explicitly.  DEIG_OJA_AUTO (what
 * deig_oja_steps_f32 does): the resident path where its shape allows, else the
 * two-pass path.  DEIG_OJA_TWO_PASS: two launches per batch (Xb V, then Xb^T T: Xb
 * read twice).  DEIG_OJA_RESIDENT: one launch per run of batches between two
 * re-orthonormalisations, each workgroup holding its block of Xb in registers (Xb
 * read once per batch); needs b = 4096, d a multiple of 512 up to 3072, k <= 32 and
 * 256 CUs (DEIG_EINVAL otherwise).  Its 256 workgroups wait on each other, so the
 * grid is checked against the occupancy query (one 512-thread workgroup per CU on
 * >= 256 CUs) before its plain launch: when it does not fit, DEIG_OJA_RESIDENT
 * returns DEIG_EHIP and DEIG_OJA_AUTO runs the two-pass path.  If a hand-off still
 * waits longer than 2 s (CUs held by other persistent work), V comes back all NaN -
 * the call is asynchronous, so NaN in V is how such a timeout shows in the data, and
 * deig_oja_error reports it as an error.  Same workspace as deig_oja_steps_f32. */
#define DEIG_OJA_AUTO 0
#define DEIG_OJA_TWO_PASS 1
#define DEIG_OJA_RESIDENT 2
int deig_oja_steps_ex(const float* X, int64_t nb, int64_t b, int64_t d, int64_t ldx, float eta,
                      float* V, int k, int64_t ldv, int orth_every, int algo, void* ws,
                      size_t ws_bytes, void* stream);

/* Status of the last deig_oja_steps_ex / deig_oja_steps_f32 / deig_oja_step_f32 call
 * on workspace ws (same b, d, k): synchronises `stream`, then returns DEIG_ETIMEOUT if
 * a resident hand-off of that call waited past its 2-s bound (V was written as NaN),
 * else DEIG_OK.  Call it before the next Oja call on the same workspace (each call
 * clears the word). */
int deig_oja_error(const void* ws, size_t ws_bytes, int64_t b, int64_t d, int k, void* stream);

/* deig_oja_steps_f32 on bf16 samples taken as they are (no fp32 copy of X): the two-pass
 * kernels with the sample as the MFMA A operand itself.  A bf16 value is its own hi piece
 * and its lo piece is exactly zero, so each fp32 product takes two bf16 MFMAs (hi hi +
 * hi lo) instead of three, over the same k-steps in the same order, and X is read at 2
 * bytes an element.
 * X: (nb*b) x d row-major bf16 (DEIG_BF16 elements), 16-byte aligned, d % 8 == 0, d >= 8,
 * ldx % 8 == 0, ldx >= d; no element behind column d of a row is read.  V, k, ldv,
 * orth_every as for deig_oja_steps_f32: 1 <= k <= min(64, d), any ldv >= d, element
 * alignment of V, nothing behind row d of a V column touched.  A single step is nb = 1,
 * orth_every = 1.
 * Contract: the result has the bits of deig_oja_steps_ex(widened X, ..., DEIG_OJA_TWO_PASS,
 * ...), widened = each element converted to fp32.  The resident kernel is never launched,
 * whatever the shape.
 * Workspace: deig_oja_workspace(b, d, k), the same layout; it may hold anything on entry.
 * The call clears the workspace's timeout word and never sets it: deig_oja_error on that
 * workspace returns DEIG_OK.  Asynchronous on `stream`: no allocation, no synchronisation, no
 * atomics, no wait between workgroups; repeated calls give identical bits.  Argument errors
 * are DEIG_EINVAL and a short or NULL workspace is DEIG_EWORKSPACE, both before any GPU work.
 * Additive: probe for the symbol, deig_version() is unchanged. */
int deig_oja_steps_bf16(const void* X, int64_t nb, int64_t b, int64_t d, int64_t ldx, float eta,
                        float* V, int k, int64_t ldv, int orth_every, void* ws, size_t ws_bytes,
                        void* stream);

/* Oja steps about a centre, on fp32, bf16 or uint8 samples taken as they are: every sample
 * is staged as t = fl32((double)x - center[j]), formed in double and rounded once (what the
 * staging step of deig_pca_transform_* does), then split into hi / lo bf16 pieces - a
 * centred value has a lo piece whatever the sample type, so every centred call runs three
 * MFMAs per fragment pair.  center == NULL means no centring: fp32 samples then run the
 * two-pass kernels, bf16 samples are deig_oja_steps_bf16, and a byte, exact in bf16, is its
 * own hi piece (two MFMAs, X read at 1 byte an element).
 * X: (nb*b) x d row-major of element type xtype, row stride ldx elements (DEIG_U8: bytes),
 * ldx >= d:
 *   DEIG_F32:  16-byte aligned, d % 4 == 0, d >= 4, ldx % 4 == 0 (deig_oja_steps_f32);
 *   DEIG_BF16: 16-byte aligned, d % 8 == 0, d >= 8, ldx % 8 == 0 (deig_oja_steps_bf16);
 *   DEIG_U8:   4-byte aligned,  d % 4 == 0, d >= 4, ldx % 4 == 0 (deig_syrk_u8, raw);
 * DEIG_F64 or any other xtype is DEIG_EINVAL.  No element behind column d of a row is read.
 * center: d doubles on the device, in units of x, or NULL; nothing behind center[d - 1] is
 * read.  V, k, ldv, orth_every as for deig_oja_steps_f32: 1 <= k <= min(64, d), any ldv >= d,
 * element alignment of V, nothing behind row d of a V column touched.  A single step is
 * nb = 1, orth_every = 1.
 * Contract: the result has the bits of deig_oja_steps_ex(T, ..., DEIG_OJA_TWO_PASS, ...) on
 * the fp32 matrix T[r][j] = fl32((double)x_rj - center_j) (center == NULL: the exact
 * widening of x).  The resident kernel is never launched, whatever the shape.
 * Workspace: deig_oja_workspace(b, d, k), the same layout; it may hold anything on entry.
 * The call clears the workspace's timeout word and never sets it: deig_oja_error on that
 * workspace returns DEIG_OK.  Asynchronous on `stream`: no allocation, no synchronisation, no
 * atomics, no wait between workgroups; repeated calls give identical bits.  Argument errors
 * are DEIG_EINVAL and a short or NULL workspace is DEIG_EWORKSPACE, both before any GPU work.
 * Additive: probe for the symbol, deig_version() is unchanged. */
int deig_oja_steps_centered(const void* X, int xtype, int64_t nb, int64_t b, int64_t d,
                            int64_t ldx, const double* center, float eta, float* V, int k,
                            int64_t ldv, int orth_every, void* ws, size_t ws_bytes, void* stream);

/* Covariance-free worker solve: the top-k eigenpairs of  scale * Xc^T Xc  straight from the
 * samples, without forming a d x d matrix (n << d: wide data with few rows, and d beyond the
 * covariance routes' reach).  Xc[r][j] = fl32((double)x_rj - center[j]), formed in double and
 * rounded once where a value is staged (center == NULL: the exact widening of x).
 *
 * deig_gram_apply is the operator itself,  Y = alpha * Xc^T (Xc Q),  exposed for testing and
 * reuse as deig_sym_apply_f32 is for the sweeps.  Two products per call, X read twice, in
 * chunks of rows: Zt = Xc Q (chunk x p, in the workspace) by the fused transform kernels of
 * deig_pca_transform_*, then Y (+)= alpha Xc^T Zt by a packed-sample TN kernel with split-K
 * partial slabs summed in slice order; the chunks are added in chunk order.
 * X: n x d row-major of element type xtype, row stride ldx elements (DEIG_U8: raw bytes),
 * n >= 1, d >= 16, ldx >= d:
 *   DEIG_F32:  16-byte aligned, d % 4 == 0, ldx % 4 == 0;
 *   DEIG_BF16: 16-byte aligned, d % 8 == 0, ldx % 8 == 0;
 *   DEIG_U8:   4-byte aligned,  d % 4 == 0, ldx % 4 == 0;
 * DEIG_F64 or any other xtype is DEIG_EINVAL.  No element behind column d of a row is read.
 * center: d doubles on the device, in units of x, or NULL.  Q, Y: d x p row-major, 16-byte
 * aligned, ldq % 4 == 0, ldy % 4 == 0, both >= p; p % 16 == 0, 16 <= p <= 128.  Nothing behind
 * column p of a Y row is written.
 * Workspace: deig_gram_apply_workspace(n, d, p, xtype) is the recommended size (0 for shapes
 * the call rejects; it does not decrease in n or p).  Any workspace of at least
 * deig_gram_apply_workspace(n', d, p, xtype) bytes for some 1 <= n' <= n is accepted and sets
 * the chunk (deig_syrk_bf16's rule).  It may hold anything on entry.
 * Asynchronous on `stream`: no allocation, no synchronisation, no atomics; repeated calls give
 * identical bits.  Argument errors are DEIG_EINVAL with a message naming the rule, a short or
 * NULL workspace is DEIG_EWORKSPACE, both before any GPU work.
 *
 * deig_topk_samples runs the solver of deig_projavg_topk_ex on that operator (implicit: no
 * image, exact Rayleigh-Ritz, its jcap defaults): the same outputs, return codes and stopping
 * rule; V d x k column-major (ldv >= d), evals ascending: the eigenvalues of scale * Xc^T Xc.
 * 1 <= k <= min(128, d); p % 16 == 0, 16 <= p <= 128, k <= p <= d.  Single solves only.
 * Implicit operators have no dominant-pair deflation: uncentred data with a large mean keeps
 * the fp32 cancellation of the small directions against the mean direction that the explicit
 * route (deig_topk_sym_ex on a covariance) deflates away - pass `center`, or use that route.
 * Additive: probe for the symbols, deig_version() is unchanged. */
int deig_gram_apply(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx,
                    const double* center, float alpha, const float* Q, int p, int64_t ldq,
                    float* Y, int64_t ldy, void* ws, size_t ws_bytes, void* stream);
size_t deig_gram_apply_workspace(int64_t n, int64_t d, int p, int xtype);
int deig_topk_samples(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx,
                      const double* center, float scale, int k, int p, int max_sweeps, float tol,
                      const float* Q0, int k0, int64_t ldq0, float* V, int64_t ldv, float* evals,
                      int* sweeps_out, float* resid_out, const deig_solver_opts* opts,
                      void* ws, size_t ws_bytes, void* stream);
size_t deig_topk_samples_workspace(int64_t n, int64_t d, int k, int p, int xtype,
                                   const deig_solver_opts* opts);

/* Wide-data worker solve through the sample-space (dual) Gram matrix, for n <= d and d beyond
 * the covariance routes' reach:
 *   K = alpha * Xc Xc^T  (n x n),   K u = lambda u   =>   v = Xc^T u * sqrt(alpha / lambda)
 * is a unit eigenvector of  alpha * Xc^T Xc  with the same lambda.  Xc as for deig_gram_apply:
 * Xc[r][j] = fl32((double)x_rj - center[j]), formed in double and rounded once where a value
 * is staged (center == NULL: the exact widening of x).
 *
 * deig_gram_outer forms K on the bf16 MFMA.  A prep kernel stages a chunk of features of all
 * n rows as bf16 pieces in MFMA operand order (no transpose: the inner dimension is the
 * contiguous one of X): a hi piece bf16(t), round to nearest even, and - for float32 samples
 * and every centred call, where a staged value can have one - a lo piece bf16(t - hi).
 * Uncentred bf16 and uint8 samples are their own hi piece.  The product kernel runs the
 * 128 x 128 tile loop of deig_syrk_bf16 once (hi hi) or three times into the same fp32
 * accumulators (hi hi, hi lo, lo hi; lo lo is dropped); no accumulator takes more than 16384
 * inner elements per pass before it is written out, and the partial slabs are added in a
 * fixed order.  Every bf16 x bf16 product is exact in fp32, so with u = 2^-24,
 * gamma_m = m u / (1 - m u) and T the staged matrix, element by element:
 *   uncentred bf16 / uint8:        |K - K64| <= (gamma_d + 2 u) alpha |T| |T|^T
 *                                  (exact when every sum_f |t_if t_jf| < 2^24 and alpha is a
 *                                  power of two);
 *   float32 and all centred calls: |K - K64| <= (2^-16 + 1.01 gamma_3d + 2 u) alpha |T| |T|^T.
 * X, xtype, ldx, alignment and center: the rules of deig_gram_apply (n >= 1, d >= 16, d and ldx
 * multiples of the type's group, DEIG_F64 is DEIG_EINVAL; no element behind column d of a row
 * and no row behind n is read).  1 <= n <= 32768.  K: n x n fp32 row-major, 16-byte aligned,
 * ldk >= n, ldk % 4 == 0; both triangles are written, bit-exactly symmetric; nothing behind
 * column n of a K row is written.  flags must be 0 (reserved for an accumulate bit).
 * Workspace: deig_gram_outer_workspace(n, d, xtype, centred) (centred: center != NULL) is the
 * recommended size, all features in one chunk up to 2^19 of them (0 for shapes the call
 * rejects; it does not decrease in d).  Any workspace of at least
 * deig_gram_outer_workspace(n, d', xtype, centred) bytes for some d' <= d is accepted and sets
 * the feature chunk (deig_syrk_bf16's rule with the roles of n and d swapped); the chunks are
 * added in order.  It may hold anything on entry.
 * Asynchronous on `stream`: no allocation, no synchronisation, no atomics, no wait between
 * workgroups; repeated calls give identical bits.  Argument errors are DEIG_EINVAL with a
 * message naming the rule, a short or NULL workspace is DEIG_EWORKSPACE, both before any GPU
 * work.
 *
 * deig_topk_dual is host composition on that product:
 *   1. K = scale * Xc Xc^T into the workspace;
 *   2. (U, lambda): the top-k pairs of K by the explicit solver as deig_topk_sym_ex runs it on
 *      an n x n fp32 matrix, subspace deig_default_subspace(n, k), the caller's opts, tol and
 *      max_sweeps (any n >= 1: the solver pads);
 *   3. the pairs with lambda_j > n 2^-23 lambda_max are kept (k0 of them), their vectors
 *      scaled by sqrt(scale / lambda_j);
 *   4. V0 = Xc^T (U diag(sqrt(scale / lambda))) by the second product of deig_gram_apply;
 *   5. the finish: the solver of deig_topk_samples on the real operator scale * Xc^T Xc, warm
 *      started with Q0 = V0, k0, and the caller's p, tol, max_sweeps and opts.
 * Why the finish exists: K is fp32-grade, and the eigenvectors of K carry an error of about
 * eps lambda_max / lambda_j, amplified again by the back-projection for small lambda_j.  The
 * dual solve only supplies the start; the outputs, return codes and stopping rule are exactly
 * deig_topk_samples's:  max_j ||A v_j - lambda_j v_j|| <= tol lambda_max  on A = scale *
 * Xc^T Xc.  *sweeps_out is the finish's sweep count; DEIG_NOT_CONVERGED from step 2 is not an
 * error by itself - the finish decides.  The implicit finish inherits deig_topk_samples's
 * caveat: a dominant mean direction is not deflated, so centre such data (pass `center`).
 * Rules: X, xtype, n, d, ldx, center as above; 1 <= k <= min(128, n, d); p, V, ldv, evals as for
 * deig_topk_samples (p % 16 == 0, 16 <= p <= 128, k <= p <= d); scale > 0; max_sweeps >= 1.
 * n > 32768 is DEIG_EINVAL: deig_topk_samples is the route there.
 * Workspace: deig_topk_dual_workspace (0 for shapes the call rejects; it does not decrease in
 * d): K, U and V0, and one region that the five steps use in turn.  The call synchronises
 * `stream` as the solvers do.  Additive: probe for the symbols, deig_version() is unchanged. */
int deig_gram_outer(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx,
                    const double* center, float alpha, float* K, int64_t ldk, int flags,
                    void* ws, size_t ws_bytes, void* stream);
size_t deig_gram_outer_workspace(int64_t n, int64_t d, int xtype, int centred);
int deig_topk_dual(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx,
                   const double* center, float scale, int k, int p, int max_sweeps, float tol,
                   float* V, int64_t ldv, float* evals, int* sweeps_out, float* resid_out,
                   const deig_solver_opts* opts, void* ws, size_t ws_bytes, void* stream);
size_t deig_topk_dual_workspace(int64_t n, int64_t d, int k, int p, int xtype,
                                const deig_solver_opts* opts);

/* Projection onto an estimated eigenspace: Y = X W.
 * Replaces the notebook's  online_distributed_PCA = lambda X: X @ matrix_w
 * (Online Distributed PCA.ipynb raw line 345).  X: n x d row-major (ldx), W: d x k
 * column-major (ldw, the solvers' V), Y: n x k row-major (ldy).  k <= 256.
 * Requires d % 4 == 0, X 16-byte aligned with ldx >= d, ldx % 4 == 0; any ldw >= d and
 * any ldy >= k with element alignment of W and Y. */
int deig_project_f32(const float* X, int64_t n, int64_t d, int64_t ldx, const float* W, int k,
                     int64_t ldw, float* Y, int64_t ldy, void* ws, size_t ws_bytes,
                     void* stream);
size_t deig_project_workspace(int64_t n, int64_t d, int k);

/* Fused centred transform, one pass over X:
 *   Y         = (X - 1 mean^T) W            (n x k row-major, any ldy >= k, any alignment)
 *   energy[i] = ||x_i - mean||^2            (n floats)
 *   resid[i]  = max(0, energy[i] - ||y_i||^2)
 * Each output may be NULL (not all three).  X: n x d row-major fp32, d % 4 == 0,
 * ldx % 4 == 0, 16-byte aligned (as deig_project_f32); mean: d doubles on the device, NULL
 * = no centring; W: d x k column-major (ldw, the solvers' V), 1 <= k <= 256.
 * The mean is subtracted in double and rounded once to fp32 when X is staged, BEFORE the
 * product (fp32 MFMA fma chain, as deig_project_f32), so Y's error is relative to
 * |X - mean| |W| and not to |mean|.
 * Accuracy of resid: for an orthonormal W it is the squared reconstruction error
 * ||(x_i - mean) - W W^T (x_i - mean)||^2, formed as a difference of two fp32 norms - it
 * is accurate to a multiple of eps * energy[i] (about (d + k) 2^-24 energy[i] at worst),
 * NOT of eps * resid[i]: a sample that the basis reconstructs to better than ~1e-3
 * relative has no correct digits in resid.
 * One workgroup per 64 rows and no split over d: a small n with a large d under-fills the
 * chip.  No atomics: repeated calls give identical bits.  Asynchronous on `stream`, no
 * allocation, no synchronisation; argument errors are DEIG_EINVAL and a short workspace
 * DEIG_EWORKSPACE before any GPU work.  Workspace: the packed W image. */
int deig_pca_transform_f32(const float* X, int64_t n, int64_t d, int64_t ldx, const double* mean,
                           const float* W, int k, int64_t ldw, float* Y, int64_t ldy, float* resid,
                           float* energy, void* ws, size_t ws_bytes, void* stream);
size_t deig_pca_transform_workspace(int64_t n, int64_t d, int k);

/* The same transform from uint8 samples, the bytes read once:
 *   Y = (V - 1 mean^T) W,  energy, resid  as deig_pca_transform_f32 (1 <= k <= 256, any
 * ldy >= k, each output optional but not all three NULL, mean == NULL: no centring), V the
 * features of X as for deig_syrk_u8 (mode, ldx in bytes, d % 4 == 0, X 4-byte aligned);
 * `mean` is in units of v.  Centred when the bytes are staged: t = fl32((double)v - mean),
 * formed in double and rounded once before the product; DEIG_U8_GRAY3 uses
 * v = (r + g + b) / 3.0 in double.  Rows past n and features past d contribute exact zeros;
 * no byte behind column d (3 d for gray) of a row is read.  The accuracy notes, the
 * parallelisation (one workgroup per 64 rows), the determinism and the workspace (the packed
 * W image) are those of deig_pca_transform_f32. */
int deig_pca_transform_u8(const uint8_t* X, int64_t n, int64_t d, int64_t ldx, int mode,
                          const double* mean, const float* W, int k, int64_t ldw, float* Y,
                          int64_t ldy, float* resid, float* energy, void* ws, size_t ws_bytes,
                          void* stream);
size_t deig_pca_transform_u8_workspace(int64_t n, int64_t d, int k);

/* The same transform from bf16 samples (DEIG_BF16 elements), read once and never widened in
 * memory: semantics, argument rules and accuracy notes are those of deig_pca_transform_f32,
 * with X n x d row-major bf16, d % 8 == 0, ldx % 8 == 0 (elements), 16-byte aligned.  Each
 * staged value is t = fl32((double)x - mean), rounded once; without a mean it is the exact
 * widening.  Rows past n and features past d contribute exact zeros; no element behind column
 * d of a row is read.  Workspace: the packed W image and the mean, padded to 64 features. */
int deig_pca_transform_bf16(const void* X, int64_t n, int64_t d, int64_t ldx, const double* mean,
                            const float* W, int k, int64_t ldw, float* Y, int64_t ldy,
                            float* resid, float* energy, void* ws, size_t ws_bytes, void* stream);
size_t deig_pca_transform_bf16_workspace(int64_t n, int64_t d, int k);

/* Building block of the solvers, exposed for direct testing / reuse:
 * C[M x N] = alpha * op(A) * B + beta * C  on fp32 MFMA (16x16x4), N % 16 == 0, N <= 256.
 * trans_a != 0: A is K x M row-major (lda), op(A) = A^T  (S*Q with S symmetric, Gram)
 * trans_a == 0: A is M x K row-major (lda)              (Wt*Q, Xb*V)
 * B is K x N row-major (ldb), C is M x N row-major (ldc).  Deterministic split-K.
 * A and B 16-byte aligned, lda % 4 == ldb % 4 == 0; trans_a: M % 4 == 0, else K % 4 == 0.
 * beta == 0: C is not read.  NULL A, B or C: DEIG_EINVAL; a workspace below the query
 * (or NULL where the query is not 0): DEIG_EWORKSPACE; both before any GPU work. */
int deig_gemm_skinny_f32(int trans_a, const float* A, int64_t lda, const float* B, int64_t ldb,
                         float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, float alpha,
                         float beta, void* ws, size_t ws_bytes, void* stream);
size_t deig_gemm_skinny_workspace(int64_t M, int64_t N, int64_t K);

#ifdef __cplusplus
}
#endif

#endif /* DEIG_H */
