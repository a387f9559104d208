// Fused centred transform (model use of an estimated basis):
//   Y = (X - 1 mean^T) W,   energy_i = ||x_i - mean||^2,   resid_i = max(0, energy_i - ||y_i||^2)
// X: n x d row-major fp32, mean: d doubles (NULL: no centring), W: d x k column-major (the
// solvers' V), Y: n x k row-major.  For an orthonormal W resid_i is the squared
// reconstruction error ||(x_i - mean) - W W^T (x_i - mean)||^2.
//
// One pass over X and one launch, after a pack of W into a zero-padded row-major d x kp
// image (kp = k rounded up to 16; pack_w_launch, project.hip).  The block tile, the W chunk's
// LDS store, the MFMA chunk product (two accumulators at kp = 16) and the epilogue (energy,
// ||y_i||^2, resid, guarded Y stores) are skinny_tile.hpp's, with the padded A layout that
// skinny_kernel's non-transposed path uses.  This kernel's own is how a chunk of X is staged:
//  * the mean is subtracted WHEN A CHUNK OF X IS STAGED, in double, rounded once to fp32
//    (as center_kernel, shift.hip): the product's rounding is then relative to the centred
//    values.  The post-hoc form X W - mean^T W loses log10(|mean| / spread) digits.
//  * the staging threads accumulate each row's sum of squares of the centred values they
//    hold (8 threads per row): energy.
// No split-K: parallelism comes from n (one workgroup per 64 rows), so a small n with a
// large d under-fills the chip.  No atomics: repeated calls give identical bits.
#include "sample_src.hpp"
#include "skinny_tile.hpp"

namespace deig {
namespace {

constexpr int PBM = tile::kRows, PBK = tile::kChunk;  // PBK: columns of X per chunk
constexpr int PT = tile::kThreads, PAST = tile::kAStridePadded;

template <int NB>
__global__ __launch_bounds__(PT) void pca_transform_kernel(
    const float* __restrict__ X, int64_t ldx, const double* __restrict__ mean,
    const float* __restrict__ Wr, float* __restrict__ Y, int64_t ldy, float* __restrict__ resid,
    float* __restrict__ energy, int64_t n, int64_t d, int k) {
  constexpr int N = NB * 16;
  constexpr int KA = NB == 1 ? 2 : 1;  // accumulators per fragment
  constexpr int BST = tile::bstride(N);
  constexpr int NB4 = PBK * N / 4, BPT = tile::b_per_thread(NB);  // float4s per chunk, per thread
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                    // [2][PBK][PAST]
  float* Bs = smem + 2 * PBK * PAST;   // [2][PBK][BST]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * PBM;
  const int64_t nch = (d + PBK - 1) / PBK;
  // staging map: thread -> rows mm and mm + 32 of the tile, columns 4 kq .. 4 kq + 3 of a chunk
  const int mm = tid >> 3, kq = tid & 7;
  const bool rowlive[2] = {m0 + mm < n, m0 + mm + 32 < n};

  f32x4 acc[NB][KA];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int a = 0; a < KA; ++a) acc[j][a] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 ra[2];
  f32x4 rb[BPT];
  double mu[4] = {0.0, 0.0, 0.0, 0.0};
  float en[2] = {0.f, 0.f};

  auto load = [&](int64_t ch) {
    const int64_t kb = ch * PBK;
    const int64_t kc = kb + 4 * kq;
    const bool kin = kc < d;  // d % 4 == 0: the four columns are in or out together
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (kin && rowlive[u]) v = *reinterpret_cast<const f32x4*>(X + (m0 + mm + 32 * u) * ldx + kc);
      ra[u] = v;
    }
    if (mean) {
#pragma unroll
      for (int e = 0; e < 4; ++e) mu[e] = kin ? mean[kc + e] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      const int f = tid + PT * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (f < NB4) {
        const int row = f / (N / 4), c4 = f % (N / 4);
        const int64_t kr = kb + row;
        if (kr < d) v = *reinterpret_cast<const f32x4*>(Wr + kr * N + 4 * c4);
      }
      rb[u] = v;
    }
  };
  // centring happens here (centre1, sample_src.hpp); rows past n and columns past d stay
  // exactly zero
  auto store = [&](int buf) {
    float* as = As + buf * PBK * PAST;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = ra[u][e];
        if (mean) t = rowlive[u] ? centre1(t, mu[e]) : 0.f;
        en[u] = fmaf(t, t, en[u]);
        as[(4 * kq + e) * PAST + mm + 32 * u] = t;
      }
    }
    tile::store_b<NB>(Bs + buf * PBK * BST, rb, tid);
  };

  const int r = lane & 15, kk = lane >> 4;
  load(0);
  store(0);
  __syncthreads();
  int cur = 0;
  for (int64_t ch = 0; ch < nch; ++ch) {
    const bool more = ch + 1 < nch;
    if (more) load(ch + 1);
    const float* as = As + cur * PBK * PAST + kk * PAST + 16 * wave + r;
    tile::mfma_chunk(acc, Bs + cur * PBK * BST, r, kk, [&](int s) { return as[4 * s * PAST]; });
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  tile::transform_epilogue(acc, en, smem, Y, ldy, resid, energy, m0, n, k, tid, wave, r, kk);
}

}  // namespace

size_t pca_transform_workspace_bytes(int64_t n, int64_t d, int k) {
  if (n < 1 || d < 1 || k < 1 || k > 256) return 0;
  const int64_t kp = cdiv(k, 16) * 16;
  return align_up((size_t)d * kp * sizeof(float), 256);  // the packed W image
}

int pca_transform_launch(const float* X, int64_t n, int64_t d, int64_t ldx, const double* mean,
                         const float* W, int k, int64_t ldw, float* Y, int64_t ldy, float* resid,
                         float* energy, void* ws, size_t ws_bytes, hipStream_t st,
                         bool w_rowmajor) {
  DEIG_REQUIRE(k >= 1 && k <= 256, "pca_transform: k=%d must be in 1..256", k);
  DEIG_REQUIRE(n >= 1 && d >= 4 && d % 4 == 0, "pca_transform: need n >= 1, d >= 4, d %% 4 == 0");
  DEIG_REQUIRE(ldx >= d, "pca_transform: ldx must be >= d");
  DEIG_REQUIRE(ldx % 4 == 0, "pca_transform: ldx %% 4 == 0 required");
  DEIG_REQUIRE(ldw >= (w_rowmajor ? (int64_t)k : d), "pca_transform: ldw must be >= d");
  DEIG_REQUIRE(Y || resid || energy, "pca_transform: need at least one output (Y, resid, energy)");
  DEIG_REQUIRE(!Y || ldy >= k, "pca_transform: ldy must be >= k");
  DEIG_REQUIRE(X && W && aligned16(X), "pca_transform: X (16-byte aligned) and W must not be NULL");
  DEIG_REQUIRE(reinterpret_cast<uintptr_t>(mean) % 8 == 0, "pca_transform: mean must be 8-byte aligned");
  const size_t need = pca_transform_workspace_bytes(n, d, k);
  if (!ws || ws_bytes < need)
    return fail(DEIG_EWORKSPACE, "pca_transform: workspace %zu bytes < required %zu", ws_bytes, need);
  const int kp = (int)cdiv(k, 16) * 16;
  float* Wr = static_cast<float*>(ws);
  if (int rc = pack_w_launch(W, ldw, d, k, kp, Wr, st, w_rowmajor)) return rc;
  const dim3 grid((unsigned)cdiv(n, PBM));
  const int rc = tile::dispatch_nb(kp / 16, [&](auto nb) {
    return tile::launch<pca_transform_kernel<nb()>>(grid, tile::shm_bytes(nb() * 16, PAST), st, X,
                                                    ldx, mean, Wr, Y, ldy, resid, energy, n, d, k);
  });
  if (rc == tile::kNoSuchNb) return fail(DEIG_EINVAL, "pca_transform: unsupported k = %d", k);
  return rc;
}

}  // namespace deig
