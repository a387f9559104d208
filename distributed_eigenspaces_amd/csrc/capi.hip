// extern "C" boundary of libdeig.so (declared in include/deig.h): argument checks and
// forwarding to the launchers and to the eigensolver driver (solver.hip).  No device
// allocation happens here: all device memory is caller-provided (PyTorch tensors on the
// Python side).  Process-global mutable state of this file: the error string
// (thread-local) and the per-device CU counts (atomics); the solver's pool of pinned
// status blocks lives in solver.hip.  Solver behaviour comes from the caller's options.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "deig_internal.hpp"

namespace deig {

static thread_local char g_err[1024] = "";

const char* last_error() { return g_err; }

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int num_cus() {
  static std::atomic<int> cache[64];  // zero-initialised (static storage)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    return 256;  // MI355X; only reached by workspace queries without a device
  }
  int v = cache[dev].load(std::memory_order_relaxed);
  if (!v) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        v <= 0) {
      (void)hipGetLastError();
      v = 256;
    }
    cache[dev].store(v, std::memory_order_relaxed);  // same value from every thread
  }
  return v;
}

}  // namespace deig

using namespace deig;

extern "C" {

int deig_version(void) { return 0x000600; }

void deig_shutdown(void) {
  // nothing allocated (no solver ran in this process): make no HIP call at all
  if (status_pool_empty()) return;
  (void)hipDeviceSynchronize();
  status_pool_drain();
  (void)hipGetLastError();
}

const char* deig_last_error(void) { return g_err; }

void deig_solver_opts_init(deig_solver_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->size = (int)sizeof(deig_solver_opts);
  o->sweep_algo = DEIG_SWEEP_AUTO;
  o->rr_every = 0;
  o->chebyshev = 1;
  o->cheb_above = -1.f;
  o->deflate = 1;
  o->deflate_early = 1;
  o->jacobi_early_sweeps = -1;
  o->jacobi_early_above = -1.f;
  o->fast_until = 1e-3f;
  o->round_until = 1e-4f;
  o->debug = 0;
  o->half_until = 1e-2f;
}

// An explicit S the solver reads in place needs lds % 4 == 0 and 16-byte alignment;
// a staged one (solver_stages: d % 4 != 0, d < 16, subspace wider than d) only its
// element alignment.
static int check_matrix(const void* S, int stype, int64_t d, int k, int p, int64_t lds,
                        const char* what) {
  if (!S || lds < d) return fail(DEIG_EINVAL, "%s: need S with lds >= d", what);
  if (k < 1 || k > d) return fail(DEIG_EINVAL, "%s: need 1 <= k <= d (k=%d, d=%lld)", what, k, (long long)d);
  const uintptr_t a = reinterpret_cast<uintptr_t>(S);
  if (solver_stages(d, k, p)) {
    if (a % (stype == DEIG_F64 ? 8 : 4))
      return fail(DEIG_EINVAL, "%s: S must be aligned to its element size", what);
  } else if (lds % 4 != 0 || !aligned16(S)) {
    return fail(DEIG_EINVAL, "%s: S must be 16-byte aligned with lds %% 4 == 0", what);
  }
  return DEIG_OK;
}

static int check_opts(const deig_solver_opts* o) {
  if (o && o->size != (int)sizeof(deig_solver_opts))
    return fail(DEIG_EINVAL, "solver options: size %d != %d (call deig_solver_opts_init)", o->size,
                (int)sizeof(deig_solver_opts));
  return DEIG_OK;
}

// The projector average with k > 128 deflates its locked blocks by fp32 skinny products with
// V itself (solver.hip apply_op_plain: the operator is implicit, there is no matrix to fold
// them into), which read V as a 16-byte aligned matrix with ldv % 4 == 0.  k alone decides
// that, so the rule is checked before any GPU work.
static int check_product_basis(const float* V, int64_t ldv, const char* what, const char* why) {
  if (ldv % 4 != 0 || !aligned16(V))
    return fail(DEIG_EINVAL, "%s: %s deflates locked pairs by products with V: V must be 16-byte "
                             "aligned with ldv %% 4 == 0 (ldv=%lld)", what, why, (long long)ldv);
  return DEIG_OK;
}

// The fp32-MFMA solver (sweep_algo = DEIG_SWEEP_FP32) reads S itself: float32 only.
static int check_fp32_solver(const deig_solver_opts* o, int stype, const char* what) {
  if (o && o->sweep_algo == DEIG_SWEEP_FP32 && stype != DEIG_F32)
    return fail(DEIG_EINVAL, "%s: a float64 S needs the bf16x6 sweep (DEIG_SWEEP_AUTO)", what);
  return DEIG_OK;
}

// Shape rules shared by deig_sym_apply_f32 and deig_sym_power_f32 (bf16x6 sweep).
static int check_sweep_shape(int64_t d, int p, int64_t ldq, int64_t ldy, const void* Q,
                             const void* Y, const char* what) {
  if (d < 1 || p < 16 || p > 128 || p % 16 != 0)
    return fail(DEIG_EINVAL, "%s: need d >= 1 and p in {16, 32, ..., 128} (p=%d)", what, p);
  if (ldq < p || ldy < p)
    return fail(DEIG_EINVAL, "%s: need ldq >= p and ldy >= p (ldq=%lld, ldy=%lld)", what,
                (long long)ldq, (long long)ldy);
  if (!Q || !Y) return fail(DEIG_EINVAL, "%s: null Q / Y", what);
  return DEIG_OK;
}

static int syrk_resolve(int64_t n, int algo) {
  if (algo != DEIG_SYRK_AUTO) return algo;
  return n >= DEIG_SYRK_SPLIT_MIN_ROWS ? DEIG_SYRK_SPLIT3 : DEIG_SYRK_FP32;
}

size_t deig_syrk_workspace_ex(int64_t n, int64_t d, int algo) {
  algo = syrk_resolve(n, algo & ~DEIG_SYRK_ACCUMULATE);
  if (algo == DEIG_SYRK_FP32) return syrk_workspace_bytes(n, d);
  if (algo == DEIG_SYRK_SPLIT3) return syrk_split_workspace_bytes(n, d);
  return 0;
}

int deig_syrk_f32_ex(const float* X, int64_t n, int64_t d, int64_t ldx, float alpha, float* S,
                     int64_t lds, int algo, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  const bool acc = (algo & DEIG_SYRK_ACCUMULATE) != 0;
  algo = syrk_resolve(n, algo & ~DEIG_SYRK_ACCUMULATE);
  if (acc && algo != DEIG_SYRK_SPLIT3)
    return fail(DEIG_EINVAL, "syrk: DEIG_SYRK_ACCUMULATE needs the split3 algorithm");
  if (algo == DEIG_SYRK_FP32)
    return syrk_launch(X, n, d, ldx, alpha, S, lds, ws, ws_bytes, (hipStream_t)stream);
  if (algo == DEIG_SYRK_SPLIT3)
    return syrk_split_launch(X, n, d, ldx, alpha, S, lds, ws, ws_bytes, (hipStream_t)stream, acc);
  return fail(DEIG_EINVAL, "syrk: unknown algorithm %d", algo);
}

size_t deig_syrk_workspace(int64_t n, int64_t d) {
  return deig_syrk_workspace_ex(n, d, DEIG_SYRK_DEFAULT);
}

int deig_syrk_f32(const float* X, int64_t n, int64_t d, int64_t ldx, float alpha, float* S,
                  int64_t lds, void* ws, size_t ws_bytes, void* stream) {
  return deig_syrk_f32_ex(X, n, d, ldx, alpha, S, lds, DEIG_SYRK_DEFAULT, ws, ws_bytes, stream);
}

size_t deig_syrk_bf16_workspace(int64_t n, int64_t d) { return syrk_bf16_workspace_bytes(n, d); }

int deig_syrk_bf16(const void* X, int64_t n, int64_t d, int64_t ldx, float alpha, float* S,
                   int64_t lds, int flags, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return syrk_bf16_launch(X, n, d, ldx, alpha, S, lds, flags, ws, ws_bytes, (hipStream_t)stream);
}

size_t deig_syrk_shift_workspace(int64_t n, int64_t d, int xtype) {
  return syrk_shift_workspace_bytes(n, d, xtype);
}

int deig_syrk_shift(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, double alpha,
                    double* S64, int64_t lds64, float* S, int64_t lds, void* ws, size_t ws_bytes,
                    void* stream) {
  g_err[0] = 0;
  return syrk_shift_launch(X, xtype, n, d, ldx, alpha, S64, lds64, S, lds, ws, ws_bytes,
                           (hipStream_t)stream);
}

size_t deig_colsum_workspace(int64_t n, int64_t d) { return colsum_workspace_bytes(n, d); }

int deig_colsum(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, double* sums, void* ws,
                size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return colsum_launch(X, xtype, n, d, ldx, sums, ws, ws_bytes, (hipStream_t)stream);
}

size_t deig_syrk_centered_workspace(int64_t n, int64_t d, int xtype) {
  return syrk_centered_workspace_bytes(n, d, xtype);
}

int deig_syrk_centered(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx,
                       const double* center, double alpha, double* S64, int64_t lds64, float* S,
                       int64_t lds, double* mean_out, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return syrk_centered_launch(X, xtype, n, d, ldx, center, alpha, S64, lds64, S, lds, mean_out, ws,
                              ws_bytes, (hipStream_t)stream);
}

size_t deig_syrk_u8_workspace(int64_t n, int64_t d, int mode) {
  return syrk_u8_workspace_bytes(n, d, mode);
}

int deig_syrk_u8(const uint8_t* X, int64_t n, int64_t d, int64_t ldx, int mode, double alpha,
                 float* S, int64_t lds, double* S64, int64_t lds64, void* ws, size_t ws_bytes,
                 void* stream) {
  g_err[0] = 0;
  return syrk_u8_launch(X, n, d, ldx, mode, alpha, S, lds, S64, lds64, ws, ws_bytes,
                        (hipStream_t)stream);
}

size_t deig_colsum_u8_workspace(int64_t n, int64_t d) { return colsum_u8_workspace_bytes(n, d); }

int deig_colsum_u8(const uint8_t* X, int64_t n, int64_t d, int64_t ldx, int mode, double* sums,
                   void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return colsum_u8_launch(X, n, d, ldx, mode, sums, ws, ws_bytes, (hipStream_t)stream);
}

size_t deig_syrk_u8_centered_workspace(int64_t n, int64_t d, int mode) {
  return syrk_u8_centered_workspace_bytes(n, d, mode);
}

int deig_syrk_u8_centered(const uint8_t* X, int64_t n, int64_t d, int64_t ldx, int mode,
                          const double* center, double alpha, float* S, int64_t lds, double* S64,
                          int64_t lds64, double* mean_out, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return syrk_u8_centered_launch(X, n, d, ldx, mode, center, alpha, S, lds, S64, lds64, mean_out, ws,
                                 ws_bytes, (hipStream_t)stream);
}

int deig_default_subspace(int64_t d, int k) { return default_subspace(d, k); }

static size_t topk_ws(int64_t d, int k, int p, bool implicit, int64_t mk, const deig_solver_opts* o,
                      int stype = DEIG_F32) {
  return solver_workspace_bytes(d, k, p, implicit, mk, make_opts(o), stype);
}

size_t deig_topk_workspace_ex(int64_t d, int k, int p, int stype, const deig_solver_opts* opts) {
  return topk_ws(d, k, p, false, 0, opts, stype);
}

size_t deig_topk_workspace(int64_t d, int k, int p) { return topk_ws(d, k, p, false, 0, nullptr); }

int deig_topk_sym_ex(const void* S, int stype, int64_t d, int64_t lds, int k, int p, int max_sweeps,
                     float tol, const float* Q0, int k0, int64_t ldq0, float* V, int64_t ldv,
                     float* evals, int* sweeps_out, float* resid_out, const deig_solver_opts* opts,
                     void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (int rc = check_opts(opts)) return rc;
  if (stype != DEIG_F32 && stype != DEIG_F64)
    return fail(DEIG_EINVAL, "topk: unknown element type %d", stype);
  if (int rc = check_matrix(S, stype, d, k, p, lds, "topk")) return rc;
  if (int rc = check_fp32_solver(opts, stype, "topk")) return rc;
  SolveProblem pr{};
  pr.op.implicit = false;
  pr.op.S = S;
  pr.op.stype = stype;
  pr.op.lds = lds;
  pr.Q0 = Q0;
  pr.k0 = k0;
  pr.ldq0 = ldq0;
  pr.V = V;
  pr.evals = evals;
  return solve_lockstep(1, &pr, d, k, p, max_sweeps, tol, ldv, sweeps_out, resid_out, nullptr,
                        make_opts(opts), ws, ws_bytes, (hipStream_t)stream);
}

int deig_topk_sym_f32(const float* S, int64_t d, int64_t lds, int k, int p, int max_sweeps,
                      float tol, const float* Q0, int k0, int64_t ldq0, float* V, int64_t ldv,
                      float* evals, int* sweeps_out, float* resid_out, void* ws, size_t ws_bytes,
                      void* stream) {
  return deig_topk_sym_ex(S, DEIG_F32, d, lds, k, p, max_sweeps, tol, Q0, k0, ldq0, V, ldv, evals,
                          sweeps_out, resid_out, nullptr, ws, ws_bytes, stream);
}

size_t deig_topk_batch_workspace(int W, int64_t d, int k, int p, int stype,
                                 const deig_solver_opts* opts) {
  if (W < 1) return 0;
  return (size_t)W * align_up(topk_ws(d, k, p, false, 0, opts, stype), 256);
}

int deig_topk_sym_batch(int W, const void* const* S, int stype, int64_t d, int64_t lds, int k, int p,
                        int max_sweeps, float tol, float* const* V, int64_t ldv, float* const* evals,
                        int* sweeps_out, float* resid_out, const deig_solver_opts* opts, void* ws,
                        size_t ws_bytes, void* const* streams, void* stream) {
  (void)streams;  // r03's per-problem streams: every launch is on `stream` since r04
  return deig_topk_sym_batch_ex(W, S, stype, d, lds, k, p, max_sweeps, tol, V, ldv, evals, sweeps_out,
                                resid_out, nullptr, opts, ws, ws_bytes, stream);
}

int deig_topk_sym_batch_ex(int W, const void* const* S, int stype, int64_t d, int64_t lds, int k, int p,
                           int max_sweeps, float tol, float* const* V, int64_t ldv,
                           float* const* evals, int* sweeps_out, float* resid_out, int* status_out,
                           const deig_solver_opts* opts, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (int rc = check_opts(opts)) return rc;
  if (W < 1 || !S || !V || !evals) return fail(DEIG_EINVAL, "topk_batch: need W >= 1 and S / V / evals arrays");
  if (stype != DEIG_F32 && stype != DEIG_F64)
    return fail(DEIG_EINVAL, "topk_batch: unknown element type %d", stype);
  for (int i = 0; i < W; ++i)
    if (int rc = check_matrix(S[i], stype, d, k, p, lds, "topk_batch")) return rc;
  if (int rc = check_fp32_solver(opts, stype, "topk_batch")) return rc;
  const size_t each = align_up(topk_ws(d, k, p, false, 0, opts, stype), 256);
  if (!ws || ws_bytes < (size_t)W * each)
    return fail(DEIG_EWORKSPACE, "topk_batch: workspace %zu bytes < required %zu", ws_bytes,
                (size_t)W * each);
  std::vector<SolveProblem> prs(W);  // value-initialised: no warm start
  for (int i = 0; i < W; ++i) {
    prs[i].op.implicit = false;
    prs[i].op.S = S[i];
    prs[i].op.stype = stype;
    prs[i].op.lds = lds;
    prs[i].V = V[i];
    prs[i].evals = evals[i];
  }
  return solve_lockstep(W, prs.data(), d, k, p, max_sweeps, tol, ldv, sweeps_out, resid_out,
                        status_out, make_opts(opts), ws, each, (hipStream_t)stream);
}

size_t deig_projavg_workspace_ex(int64_t d, int64_t mk, int k, int p,
                                 const deig_solver_opts* opts) {
  return topk_ws(d, k, p, true, mk, opts);
}

size_t deig_projavg_workspace(int64_t d, int64_t mk, int k, int p) {
  return topk_ws(d, k, p, true, mk, nullptr);
}

int deig_projavg_topk_ex(const float* Wt, int64_t d, int64_t mk, int64_t ldw, float scale, int k,
                         int p, int max_sweeps, float tol, const float* Q0, int k0, int64_t ldq0,
                         float* V, int64_t ldv, float* evals, int* sweeps_out, float* resid_out,
                         const deig_solver_opts* opts, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (int rc = check_opts(opts)) return rc;
  if (!Wt || mk < 1 || ldw < d || ldw % 4 != 0 || !aligned16(Wt))
    return fail(DEIG_EINVAL, "projavg: Wt must be 16-byte aligned, mk >= 1, ldw >= d, ldw %% 4 == 0");
  if (k > 128)  // block locking on the implicit operator
    if (int rc = check_product_basis(V, ldv, "projavg", "k > 128")) return rc;
  SolveProblem pr{};
  pr.op.implicit = true;
  pr.op.stype = DEIG_F32;
  pr.op.Wt = Wt;
  pr.op.mk = mk;
  pr.op.ldw = ldw;
  pr.op.scale = scale;
  pr.Q0 = Q0;
  pr.k0 = k0;
  pr.ldq0 = ldq0;
  pr.V = V;
  pr.evals = evals;
  return solve_lockstep(1, &pr, d, k, p, max_sweeps, tol, ldv, sweeps_out, resid_out, nullptr,
                        make_opts(opts), ws, ws_bytes, (hipStream_t)stream);
}

int deig_projavg_topk_f32(const float* Wt, int64_t d, int64_t mk, int64_t ldw, float scale, int k,
                          int p, int max_sweeps, float tol, const float* Q0, int k0, int64_t ldq0,
                          float* V, int64_t ldv, float* evals, int* sweeps_out, float* resid_out,
                          void* ws, size_t ws_bytes, void* stream) {
  return deig_projavg_topk_ex(Wt, d, mk, ldw, scale, k, p, max_sweeps, tol, Q0, k0, ldq0, V, ldv,
                              evals, sweeps_out, resid_out, nullptr, ws, ws_bytes, stream);
}

size_t deig_gram_apply_workspace(int64_t n, int64_t d, int p, int xtype) {
  return gram_apply_workspace_bytes(n, d, p, xtype);
}

int deig_gram_apply(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, const double* center,
                    float alpha, const float* Q, int p, int64_t ldq, float* Y, int64_t ldy, void* ws,
                    size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return gram_apply_launch(X, xtype, n, d, ldx, center, alpha, Q, p, ldq, Y, ldy, ws, ws_bytes,
                           (hipStream_t)stream);
}

// The shape rules of the covariance-free solve that do not involve pointers.
static bool topk_samples_shape_ok(int64_t n, int64_t d, int k, int p, int xtype) {
  return gram_apply_workspace_bytes(n, d, 16, xtype) > 0 && k >= 1 && k <= 128 && k <= d && p >= 16 &&
         p <= 128 && p % 16 == 0 && p >= k && p <= d;
}

size_t deig_topk_samples_workspace(int64_t n, int64_t d, int k, int p, int xtype,
                                   const deig_solver_opts* opts) {
  if (check_opts(opts) || !topk_samples_shape_ok(n, d, k, p, xtype)) return 0;
  return solver_workspace_bytes(d, k, p, true, 0, make_opts(opts), DEIG_F32, n, xtype);
}

int deig_topk_samples(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, const double* center,
                      float scale, int k, int p, int max_sweeps, float tol, const float* Q0, int k0,
                      int64_t ldq0, float* V, int64_t ldv, float* evals, int* sweeps_out,
                      float* resid_out, const deig_solver_opts* opts, void* ws, size_t ws_bytes,
                      void* stream) {
  g_err[0] = 0;
  const char* what = "topk_samples";
  if (int rc = check_opts(opts)) return rc;
  if (int rc = gram_apply_check(X, xtype, n, d, ldx, center, what)) return rc;
  if (k < 1 || k > 128 || k > d)
    return fail(DEIG_EINVAL, "%s: need 1 <= k <= min(128, d) (k=%d, d=%lld)", what, k, (long long)d);
  if (p < 16 || p > 128 || p % 16 != 0)
    return fail(DEIG_EINVAL, "%s: p must be a multiple of 16 in 16..128 (got %d)", what, p);
  if (p < k || p > d)
    return fail(DEIG_EINVAL, "%s: the subspace needs k <= p <= d (k=%d, p=%d, d=%lld)", what, k, p,
                (long long)d);
  if (max_sweeps < 1) return fail(DEIG_EINVAL, "%s: max_sweeps must be >= 1", what);
  if (!V || !evals || ldv < d) return fail(DEIG_EINVAL, "%s: V and evals must not be NULL, ldv >= d", what);
  if (k0 < 0 || k0 > p || (k0 > 0 && (!Q0 || ldq0 < d)))
    return fail(DEIG_EINVAL, "%s: bad warm start (k0=%d, p=%d)", what, k0, p);
  const size_t need = deig_topk_samples_workspace(n, d, k, p, xtype, opts);
  if (!ws || ws_bytes < need)
    return fail(DEIG_EWORKSPACE, "%s: workspace %zu bytes < required %zu", what, ws ? ws_bytes : (size_t)0,
                need);
  SolveProblem pr{};
  pr.op.implicit = true;
  pr.op.stype = DEIG_F32;
  pr.op.X = X;
  pr.op.xtype = xtype;
  pr.op.n = n;
  pr.op.ldx = ldx;
  pr.op.center = center;
  pr.op.scale = scale;
  pr.Q0 = Q0;
  pr.k0 = k0;
  pr.ldq0 = ldq0;
  pr.V = V;
  pr.evals = evals;
  return solve_lockstep(1, &pr, d, k, p, max_sweeps, tol, ldv, sweeps_out, resid_out, nullptr,
                        make_opts(opts), ws, ws_bytes, (hipStream_t)stream);
}

size_t deig_gram_outer_workspace(int64_t n, int64_t d, int xtype, int centred) {
  return gram_outer_workspace_bytes(n, d, xtype, centred);
}

int deig_gram_outer(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, const double* center,
                    float alpha, float* K, int64_t ldk, int flags, void* ws, size_t ws_bytes,
                    void* stream) {
  g_err[0] = 0;
  return gram_outer_launch(X, xtype, n, d, ldx, center, alpha, K, ldk, flags, ws, ws_bytes,
                           (hipStream_t)stream);
}

// The dual solve's workspace: what outlives a phase (K, then U and lam, then V0) in front, then
// one region that the phases use in turn - the Gram product, the n x n solve, the
// back-projection (Zt, Y, split-K slab), the finish.
namespace {
struct DualWs {
  float *K, *U, *lam, *V0, *Zt, *Y, *slab;
  char* phase;
  int64_t ldk;
  int kp, pn;
  size_t outer_bytes, solve_bytes, finish_bytes, phase_bytes, total;
};
DualWs carve_dual(void* ws, int64_t n, int64_t d, int k, int p, int xtype, const deig_solver_opts* opts) {
  DualWs w{};
  w.ldk = (n + 3) / 4 * 4;
  w.kp = (k + 15) / 16 * 16;
  w.pn = default_subspace(n, k);
  Carve c(ws, 0);
  w.K = c.take<float>((size_t)n * w.ldk);
  w.U = c.take<float>((size_t)n * k);
  w.lam = c.take<float>((size_t)k);
  w.V0 = c.take<float>((size_t)d * k);
  w.phase = c.take<char>(0);
  const size_t front = c.off;
  w.outer_bytes = gram_outer_workspace_bytes(n, d, xtype, 1);
  w.solve_bytes = solver_workspace_bytes(n, k, w.pn, false, 0, make_opts(opts), DEIG_F32);
  w.finish_bytes = solver_workspace_bytes(d, k, p, true, 0, make_opts(opts), DEIG_F32, n, xtype);
  Carve b(w.phase, 0);
  w.Zt = b.take<float>((size_t)n * w.kp);
  w.Y = b.take<float>((size_t)d * w.kp);
  const int ks = gram_tn_split(d, n);
  w.slab = b.take<float>(ks > 1 ? (size_t)ks * d * w.kp : 0);
  w.phase_bytes = std::max(std::max(w.outer_bytes, w.solve_bytes), std::max(w.finish_bytes, b.off));
  w.total = front + align_up(w.phase_bytes, 256);
  return w;
}
bool topk_dual_shape_ok(int64_t n, int64_t d, int k, int p, int xtype) {
  return topk_samples_shape_ok(n, d, k, p, xtype) && n <= 32768 && k <= n;
}
}  // namespace

size_t deig_topk_dual_workspace(int64_t n, int64_t d, int k, int p, int xtype,
                                const deig_solver_opts* opts) {
  if (check_opts(opts) || !topk_dual_shape_ok(n, d, k, p, xtype)) return 0;
  const DualWs w = carve_dual(nullptr, n, d, k, p, xtype, opts);
  if (!w.outer_bytes || !w.solve_bytes || !w.finish_bytes) return 0;
  return w.total;
}

int deig_topk_dual(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, const double* center,
                   float scale, int k, int p, int max_sweeps, float tol, float* V, int64_t ldv,
                   float* evals, int* sweeps_out, float* resid_out, const deig_solver_opts* opts,
                   void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  const char* what = "topk_dual";
  hipStream_t st = (hipStream_t)stream;
  if (int rc = check_opts(opts)) return rc;
  if (int rc = gram_apply_check(X, xtype, n, d, ldx, center, what)) return rc;
  if (n > 32768)
    return fail(DEIG_EINVAL, "%s: n must be <= 32768 (got %lld): the n x n Gram matrix is the route for "
                             "n <= d; use deig_topk_samples", what, (long long)n);
  if (k < 1 || k > 128 || k > n || k > d)
    return fail(DEIG_EINVAL, "%s: need 1 <= k <= min(128, n, d) (k=%d, n=%lld, d=%lld)", what, k,
                (long long)n, (long long)d);
  if (p < 16 || p > 128 || p % 16 != 0)
    return fail(DEIG_EINVAL, "%s: p must be a multiple of 16 in 16..128 (got %d)", what, p);
  if (p < k || p > d)
    return fail(DEIG_EINVAL, "%s: the subspace needs k <= p <= d (k=%d, p=%d, d=%lld)", what, k, p,
                (long long)d);
  if (max_sweeps < 1) return fail(DEIG_EINVAL, "%s: max_sweeps must be >= 1", what);
  if (!V || !evals || ldv < d) return fail(DEIG_EINVAL, "%s: V and evals must not be NULL, ldv >= d", what);
  if (!(scale > 0.f)) return fail(DEIG_EINVAL, "%s: scale must be > 0", what);
  const size_t need = deig_topk_dual_workspace(n, d, k, p, xtype, opts);
  if (!ws || ws_bytes < need || !need)
    return fail(DEIG_EWORKSPACE, "%s: workspace %zu bytes < required %zu", what, ws ? ws_bytes : (size_t)0,
                need);
  const DualWs w = carve_dual(ws, n, d, k, p, xtype, opts);
  const Opts o = make_opts(opts);
  // 1. K = scale Xc Xc^T
  if (int rc = gram_outer_launch(X, xtype, n, d, ldx, center, scale, w.K, w.ldk, 0, w.phase, w.phase_bytes,
                                 st))
    return rc;
  // 2. its top-k pairs (U n x k column-major, lam ascending) by the explicit solver; a start
  // that has not converged is still a start
  {
    SolveProblem pr{};
    pr.op.implicit = false;
    pr.op.S = w.K;
    pr.op.stype = DEIG_F32;
    pr.op.lds = w.ldk;
    pr.V = w.U;
    pr.evals = w.lam;
    const int rc = solve_lockstep(1, &pr, n, k, w.pn, max_sweeps, tol, n, nullptr, nullptr, nullptr, o,
                                  w.phase, w.phase_bytes, st);
    if (rc != DEIG_OK && rc != DEIG_NOT_CONVERGED) return rc;
  }
  // 3. the usable pairs: lam_j > n 2^-23 lam_max (ascending: the last k0 columns); K is
  // fp32-grade, what lies below that is rounding
  float lam_h[128];
  DEIG_HIP_CHECK(hipMemcpyAsync(lam_h, w.lam, sizeof(float) * k, hipMemcpyDeviceToHost, st));
  DEIG_HIP_CHECK(hipStreamSynchronize(st));
  int k0 = 0;
  const float lmax = lam_h[k - 1];
  if (lmax > 0.f) {
    const float thr = (float)n * 1.1920929e-7f * lmax;
    while (k0 < k && lam_h[k - 1 - k0] > thr) ++k0;
  }
  if (k0 > 0) {
    // Zt = U diag(sqrt(scale / lam)), then 4. V0 = Xc^T Zt: unit columns, v = Xc^T u sqrt(scale / lam)
    if (int rc = dual_scale_launch(w.U, n, w.lam, k, w.kp, k0, scale, n, w.Zt, st)) return rc;
    if (int rc = gram_tn_launch(X, xtype, n, d, ldx, center, w.Zt, w.kp, 1.f, w.Y, w.kp, w.slab, st))
      return rc;
    if (int rc = dual_cols_launch(w.Y, w.kp, d, k - k0, k0, w.V0, st)) return rc;
  }
  // 5. the finish on the real operator: deig_topk_samples from Q0 = V0
  g_err[0] = 0;
  SolveProblem pr{};
  pr.op.implicit = true;
  pr.op.stype = DEIG_F32;
  pr.op.X = X;
  pr.op.xtype = xtype;
  pr.op.n = n;
  pr.op.ldx = ldx;
  pr.op.center = center;
  pr.op.scale = scale;
  pr.Q0 = k0 ? w.V0 : nullptr;
  pr.k0 = k0;
  pr.ldq0 = d;
  pr.V = V;
  pr.evals = evals;
  return solve_lockstep(1, &pr, d, k, p, max_sweeps, tol, ldv, sweeps_out, resid_out, nullptr, o, w.phase,
                        w.phase_bytes, st);
}

size_t deig_procrustes_workspace(int64_t d, int64_t mk, int k) {
  return procrustes_workspace_bytes(d, mk, k);
}

int deig_procrustes_avg_f32(const float* Wt, int64_t d, int64_t mk, int64_t ldw, int k,
                            const float* Vref, int64_t ldref, const float* weights, int iters,
                            float* V, int64_t ldv, float* Z, float* cosines, void* ws,
                            size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return procrustes_launch(Wt, d, mk, ldw, k, Vref, ldref, weights, iters, V, ldv, Z, cosines, ws,
                           ws_bytes, (hipStream_t)stream);
}

size_t deig_subspace_dist_workspace(int64_t d, int k) { return subspace_dist_workspace_bytes(d, k); }

int deig_subspace_dist_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t d, int k,
                           float* out, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return subspace_dist_launch(A, lda, B, ldb, d, k, out, ws, ws_bytes, (hipStream_t)stream);
}

int deig_sym_power_f32(const float* S, int64_t d, int64_t lds, float* Q, int p, int64_t ldq,
                       float* Y, int64_t ldy, const float* cs, int steps, int algo, void* ws,
                       size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  DEIG_REQUIRE(steps >= 1 && cs && Q, "sym_power: need steps >= 1, cs and Q");
  const bool prepared = (algo & DEIG_SWEEP_PREPARED) != 0;
  const int smode = (algo & DEIG_SWEEP_HALF)      ? kSweepHalf
                    : (algo & DEIG_SWEEP_FAST)    ? kSweepFast
                    : (algo & DEIG_SWEEP_ROUND_Q) ? kSweepRoundQ
                                                  : kSweepExact;
  algo &= ~(DEIG_SWEEP_PREPARED | DEIG_SWEEP_ROUND_Q | DEIG_SWEEP_FAST | DEIG_SWEEP_HALF);
  if (algo != DEIG_SWEEP_AUTO && algo != DEIG_SWEEP_BF16X6)
    return fail(DEIG_EINVAL, "sym_power: algorithm %d has no fused chain (bf16x6 only)", algo);
  if (int rc = check_sweep_shape(d, p, ldq, ldy, Q, Y, "sym_power")) return rc;
  // the fused basis step (sweep.hip sweep_finish_kernel) moves Q and Y rows as float4
  if (ldq % 4 != 0 || ldy % 4 != 0 || !aligned16(Q) || !aligned16(Y))
    return fail(DEIG_EINVAL, "sym_power: Q and Y must be 16-byte aligned with ldq %% 4 == 0 and "
                             "ldy %% 4 == 0 (ldq=%lld, ldy=%lld)", (long long)ldq, (long long)ldy);
  hipStream_t st = (hipStream_t)stream;
  if (!prepared) {
    const int rc = sweep_prepare(S, DEIG_F32, d, lds, p, ws, ws_bytes, st);
    if (rc) return rc;
  }
  SweepStep step{};
  step.kind = 1;
  step.Q = Q;
  step.ldq = ldq;
  step.cs = cs;
  step.lam = cs;  // liveness |cs_j| >= 0 * |cs_0|: every column with cs_j > 0
  step.tau = 0.f;
  step.next_mode = smode;
  for (int i = 0; i < steps; ++i) {
    step.write_y = i + 1 == steps;  // the contract: on return Y = S Q_{steps-1}
    const int rc = sweep_apply(Q, d, p, ldq, Y, ldy, 1.f, ws, ws_bytes, st, smode, &step, i > 0);
    if (rc) return rc;
  }
  return DEIG_OK;
}

size_t deig_sym_apply_workspace(int64_t d, int p, int algo) {
  algo &= ~(DEIG_SWEEP_PREPARED | DEIG_SWEEP_ROUND_Q | DEIG_SWEEP_FAST | DEIG_SWEEP_HALF |
            DEIG_SWEEP_KERNEL_ONLY);
  if (algo == DEIG_SWEEP_FP32) return skinny_workspace_bytes(d, p, d);
  return sweep_workspace_bytes(d, p);
}

int deig_sym_apply_f32(const float* S, int64_t d, int64_t lds, const float* Q, int p,
                       int64_t ldq, float* Y, int64_t ldy, float alpha, int algo, void* ws,
                       size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (algo == DEIG_SWEEP_FP32) {
    // the skinny product's operand rules (skinny.hip skinny_launch), named for this entry point
    if (d < 4 || d % 4 != 0 || lds < d || lds % 4 != 0 || !S || !aligned16(S))
      return fail(DEIG_EINVAL, "sym_apply: DEIG_SWEEP_FP32 needs d %% 4 == 0 and a 16-byte aligned S "
                               "with lds >= d, lds %% 4 == 0 (d=%lld, lds=%lld)", (long long)d,
                  (long long)lds);
    if (ldq < p || ldq % 4 != 0 || !Q || !aligned16(Q) || ldy < p || !Y)
      return fail(DEIG_EINVAL, "sym_apply: DEIG_SWEEP_FP32 needs a 16-byte aligned Q with ldq >= p, "
                               "ldq %% 4 == 0, and ldy >= p (ldq=%lld, ldy=%lld)", (long long)ldq,
                  (long long)ldy);
    return skinny_launch(true, S, lds, Q, ldq, Y, ldy, d, p, d, alpha, 0.f,
                         static_cast<float*>(ws), ws_bytes, (hipStream_t)stream);
  }
  const bool prepared = (algo & DEIG_SWEEP_PREPARED) != 0;
  const bool kernel_only = (algo & DEIG_SWEEP_KERNEL_ONLY) != 0;
  const int smode = (algo & DEIG_SWEEP_HALF)      ? kSweepHalf
                    : (algo & DEIG_SWEEP_FAST)    ? kSweepFast
                    : (algo & DEIG_SWEEP_ROUND_Q) ? kSweepRoundQ
                                                  : kSweepExact;
  algo &= ~(DEIG_SWEEP_PREPARED | DEIG_SWEEP_ROUND_Q | DEIG_SWEEP_FAST | DEIG_SWEEP_HALF |
            DEIG_SWEEP_KERNEL_ONLY);
  if (algo != DEIG_SWEEP_AUTO && algo != DEIG_SWEEP_BF16X6)
    return fail(DEIG_EINVAL, "sym_apply: unknown algorithm %d", algo);
  if (int rc = check_sweep_shape(d, p, ldq, ldy, Q, Y, "sym_apply")) return rc;
  if (!prepared) {
    const int rc = sweep_prepare(S, DEIG_F32, d, lds, p, ws, ws_bytes, (hipStream_t)stream);
    if (rc) return rc;
  }
  return sweep_apply(Q, d, p, ldq, Y, ldy, alpha, ws, ws_bytes, (hipStream_t)stream, smode,
                     nullptr, kernel_only, kernel_only);
}

size_t deig_oja_workspace(int64_t b, int64_t d, int k) { return oja_workspace_bytes(b, d, k); }

int deig_oja_steps_ex(const float* X, int64_t nb, int64_t b, int64_t d, int64_t ldx, float eta,
                      float* V, int k, int64_t ldv, int orth_every, int algo, void* ws,
                      size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (!X || !V || !aligned16(X)) return fail(DEIG_EINVAL, "oja: X must be 16-byte aligned");
  return oja_steps_launch(X, nb, b, d, ldx, eta, V, k, ldv, orth_every, ws, ws_bytes,
                          (hipStream_t)stream, algo);
}

int deig_oja_error(const void* ws, size_t ws_bytes, int64_t b, int64_t d, int k, void* stream) {
  g_err[0] = 0;
  return oja_error(ws, ws_bytes, b, d, k, (hipStream_t)stream);
}

int deig_oja_steps_f32(const float* X, int64_t nb, int64_t b, int64_t d, int64_t ldx, float eta,
                       float* V, int k, int64_t ldv, int orth_every, void* ws, size_t ws_bytes,
                       void* stream) {
  return deig_oja_steps_ex(X, nb, b, d, ldx, eta, V, k, ldv, orth_every, DEIG_OJA_AUTO, ws,
                           ws_bytes, stream);
}

int deig_oja_steps_bf16(const void* X, int64_t nb, int64_t b, int64_t d, int64_t ldx, float eta,
                        float* V, int k, int64_t ldv, int orth_every, void* ws, size_t ws_bytes,
                        void* stream) {
  g_err[0] = 0;
  return oja_steps_bf16_launch(X, nb, b, d, ldx, eta, V, k, ldv, orth_every, ws, ws_bytes,
                               (hipStream_t)stream);
}

int deig_oja_steps_centered(const void* X, int xtype, int64_t nb, int64_t b, int64_t d, int64_t ldx,
                            const double* center, float eta, float* V, int k, int64_t ldv,
                            int orth_every, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return oja_steps_centered_launch(X, xtype, nb, b, d, ldx, center, eta, V, k, ldv, orth_every, ws,
                                   ws_bytes, (hipStream_t)stream);
}

int deig_oja_step_f32(const float* Xb, int64_t b, int64_t d, int64_t ldx, float eta, float* V,
                      int k, int64_t ldv, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  if (!Xb || !V || !aligned16(Xb)) return fail(DEIG_EINVAL, "oja: Xb must be 16-byte aligned");
  return oja_launch(Xb, b, d, ldx, eta, V, k, ldv, ws, ws_bytes, (hipStream_t)stream);
}

size_t deig_project_workspace(int64_t n, int64_t d, int k) {
  return project_workspace_bytes(n, d, k);
}

int deig_project_f32(const float* X, int64_t n, int64_t d, int64_t ldx, const float* W, int k,
                     int64_t ldw, float* Y, int64_t ldy, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return project_launch(X, n, d, ldx, W, k, ldw, Y, ldy, ws, ws_bytes, (hipStream_t)stream);
}

size_t deig_pca_transform_workspace(int64_t n, int64_t d, int k) {
  return pca_transform_workspace_bytes(n, d, k);
}

int deig_pca_transform_f32(const float* X, int64_t n, int64_t d, int64_t ldx, const double* mean,
                           const float* W, int k, int64_t ldw, float* Y, int64_t ldy, float* resid,
                           float* energy, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return pca_transform_launch(X, n, d, ldx, mean, W, k, ldw, Y, ldy, resid, energy, ws, ws_bytes,
                              (hipStream_t)stream);
}

size_t deig_pca_transform_u8_workspace(int64_t n, int64_t d, int k) {
  return pca_transform_u8_workspace_bytes(n, d, k);
}

int deig_pca_transform_u8(const uint8_t* X, int64_t n, int64_t d, int64_t ldx, int mode,
                          const double* mean, const float* W, int k, int64_t ldw, float* Y,
                          int64_t ldy, float* resid, float* energy, void* ws, size_t ws_bytes,
                          void* stream) {
  g_err[0] = 0;
  return pca_transform_u8_launch(X, n, d, ldx, mode, mean, W, k, ldw, Y, ldy, resid, energy, ws,
                                 ws_bytes, (hipStream_t)stream);
}

size_t deig_pca_transform_bf16_workspace(int64_t n, int64_t d, int k) {
  return pca_transform_bf16_workspace_bytes(n, d, k);
}

int deig_pca_transform_bf16(const void* X, int64_t n, int64_t d, int64_t ldx, const double* mean,
                            const float* W, int k, int64_t ldw, float* Y, int64_t ldy,
                            float* resid, float* energy, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return pca_transform_bf16_launch(X, n, d, ldx, mean, W, k, ldw, Y, ldy, resid, energy, ws,
                                   ws_bytes, (hipStream_t)stream);
}

size_t deig_gemm_skinny_workspace(int64_t M, int64_t N, int64_t K) {
  return skinny_workspace_bytes(M, N, K);
}

int deig_gemm_skinny_f32(int trans_a, const float* A, int64_t lda, const float* B, int64_t ldb,
                         float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, float alpha,
                         float beta, void* ws, size_t ws_bytes, void* stream) {
  g_err[0] = 0;
  return skinny_launch(trans_a != 0, A, lda, B, ldb, C, ldc, M, N, K, alpha, beta,
                       static_cast<float*>(ws), ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
