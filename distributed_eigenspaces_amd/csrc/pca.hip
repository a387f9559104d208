// Fused centred transform (model use of an estimated basis):
//   Y = (X - 1 mean^T) W,   energy_i = ||x_i - mean||^2,   resid_i = max(0, energy_i - ||y_i||^2)
// X: n x d row-major fp32, mean: d doubles (NULL: no centring), W: d x k column-major (the
// solvers' V), Y: n x k row-major.  For an orthonormal W resid_i is the squared
// reconstruction error ||(x_i - mean) - W W^T (x_i - mean)||^2.
//
// One pass over X and one launch, after a pack of W into a zero-padded row-major d x kp
// image (kp = k rounded up to 16; pack_w_launch, project.hip).  The kernel is
// skinny_kernel's non-transposed path (skinny.hip: block = 4 waves, block tile 64 rows x kp,
// each wave 16 rows x kp on v_mfma_f32_16x16x4_f32, d walked in chunks of 32 staged through
// LDS from registers, double buffered) with three changes:
//  * the mean is subtracted WHEN A CHUNK OF X IS STAGED, in double, rounded once to fp32
//    (as center_kernel, shift.hip): the product's rounding is then relative to the centred
//    values.  The post-hoc form X W - mean^T W loses log10(|mean| / spread) digits.
//  * the staging threads accumulate each row's sum of squares of the centred values they
//    hold (8 threads per row, combined by a fixed shuffle tree): energy.
//  * the epilogue forms ||y_i||^2 from the accumulators (the kp/16 fragments, then the 16
//    column lanes), then resid, and stores Y straight to its destination with guarded
//    scalar stores: any ldy >= k, any alignment, k < kp - no staging buffer, no crop pass.
// No split-K: parallelism comes from n (one workgroup per 64 rows), so a small n with a
// large d under-fills the chip.  No atomics: repeated calls give identical bits.
// kp = 16 has one fragment per wave, so its K chain alternates between two accumulators
// (the 16x16x4 MFMA has a 40-cycle dependent latency on a 32-cycle issue).
#include "deig_internal.hpp"

namespace deig {
namespace {

constexpr int PBM = 64;        // rows of a block tile
constexpr int PBK = 32;        // columns of X per chunk
constexpr int PT = 256;        // threads
constexpr int PAST = PBM + 16;  // 80 == 16 mod 32 (skinny.hip)

__host__ __device__ constexpr int pca_bstride(int N) { return (N % 32 == 0) ? N + 16 : N; }
constexpr size_t pca_shm_bytes(int N) {
  return (size_t)(2 * PBK * PAST + 2 * PBK * pca_bstride(N)) * sizeof(float);
}

template <int NB>
__global__ __launch_bounds__(PT) void pca_transform_kernel(
    const float* __restrict__ X, int64_t ldx, const double* __restrict__ mean,
    const float* __restrict__ Wr, float* __restrict__ Y, int64_t ldy, float* __restrict__ resid,
    float* __restrict__ energy, int64_t n, int64_t d, int k) {
  constexpr int N = NB * 16;
  constexpr int KA = NB == 1 ? 2 : 1;  // accumulators per fragment
  constexpr int BST = pca_bstride(N);
  constexpr int NB4 = PBK * N / 4;         // float4s of a W chunk
  constexpr int BPT = (NB4 + PT - 1) / PT;  // per thread
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                    // [2][PBK][PAST]
  float* Bs = smem + 2 * PBK * PAST;   // [2][PBK][BST]
  // [PBM] row energies, written after the last chunk's products on top of the dead staging
  // buffers: a region of their own (256 B) would take the kernel from 4 to 3 workgroups
  // per CU at kp = 64, where the buffers are exactly a quarter of the 160 KB of LDS
  float* es = smem;

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
  // centring happens here: t = fl32(x - mean) in double, one rounding; rows past n and
  // columns past d stay exactly zero
  auto store = [&](int buf) {
    float* as = As + buf * PBK * PAST;
    float* bs = Bs + buf * PBK * BST;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = ra[u][e];
        if (mean) t = rowlive[u] ? (float)((double)t - mu[e]) : 0.f;
        en[u] = fmaf(t, t, en[u]);
        as[(4 * kq + e) * PAST + mm + 32 * u] = t;
      }
    }
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      const int f = tid + PT * u;
      if (f < NB4) {
        const int row = f / (N / 4), c4 = f % (N / 4);
        *reinterpret_cast<f32x4*>(bs + row * BST + 4 * c4) = rb[u];
      }
    }
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
    const float* bs = Bs + cur * PBK * BST + kk * BST + r;
#pragma unroll
    for (int s = 0; s < PBK / 4; ++s) {
      const float a = as[4 * s * PAST];
#pragma unroll
      for (int j = 0; j < NB; ++j)
        acc[j][s % KA] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs[4 * s * BST + 16 * j],
                                                              acc[j][s % KA], 0, 0, 0);
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // row energies: the 8 staging threads of a row are 8 consecutive lanes
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    float e = en[u];
    e += __shfl_xor(e, 1);
    e += __shfl_xor(e, 2);
    e += __shfl_xor(e, 4);
    if (kq == 0) es[mm + 32 * u] = e;
  }
  __syncthreads();

  // C/D map of 16x16x4: col = lane & 15, row = 4 * (lane >> 4) + reg
  const int lrow = 16 * wave + 4 * kk;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t m = m0 + lrow + e;
    float yn = 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      float v = acc[j][0][e];
      if (KA == 2) v += acc[j][KA - 1][e];
      yn = fmaf(v, v, yn);  // columns >= k are exactly zero (zero-padded W image)
      if (Y && m < n && 16 * j + r < k) Y[m * ldy + 16 * j + r] = v;
    }
    yn += __shfl_xor(yn, 1);
    yn += __shfl_xor(yn, 2);
    yn += __shfl_xor(yn, 4);
    yn += __shfl_xor(yn, 8);
    if (r == 0 && m < n) {
      const float ev = es[lrow + e];
      if (energy) energy[m] = ev;
      if (resid) resid[m] = fmaxf(0.f, ev - yn);
    }
  }
}

template <int NB>
int pca_launch_nb(const float* X, int64_t ldx, const double* mean, const float* Wr, float* Y,
                  int64_t ldy, float* resid, float* energy, int64_t n, int64_t d, int k,
                  hipStream_t st) {
  constexpr size_t shm = pca_shm_bytes(NB * 16);
  // once per instantiation (C++11 thread-safe static initialisation)
  static const hipError_t attr = hipFuncSetAttribute(
      (const void*)pca_transform_kernel<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  DEIG_HIP_CHECK(attr);
  hipLaunchKernelGGL((pca_transform_kernel<NB>), dim3((unsigned)cdiv(n, PBM)), dim3(PT), shm, st,
                     X, ldx, mean, Wr, Y, ldy, resid, energy, n, d, k);
  DEIG_HIP_CHECK(hipGetLastError());
  return DEIG_OK;
}

}  // namespace

size_t pca_transform_workspace_bytes(int64_t n, int64_t d, int k) {
  if (n < 1 || d < 1 || k < 1 || k > 256) return 0;
  const int64_t kp = cdiv(k, 16) * 16;
  return align_up((size_t)d * kp * sizeof(float), 256);  // the packed W image
}

int pca_transform_launch(const float* X, int64_t n, int64_t d, int64_t ldx, const double* mean,
                         const float* W, int k, int64_t ldw, float* Y, int64_t ldy, float* resid,
                         float* energy, void* ws, size_t ws_bytes, hipStream_t st) {
  DEIG_REQUIRE(k >= 1 && k <= 256, "pca_transform: k=%d must be in 1..256", k);
  DEIG_REQUIRE(n >= 1 && d >= 4 && d % 4 == 0, "pca_transform: need n >= 1, d >= 4, d %% 4 == 0");
  DEIG_REQUIRE(ldx >= d, "pca_transform: ldx must be >= d");
  DEIG_REQUIRE(ldx % 4 == 0, "pca_transform: ldx %% 4 == 0 required");
  DEIG_REQUIRE(ldw >= d, "pca_transform: ldw must be >= d");
  DEIG_REQUIRE(Y || resid || energy, "pca_transform: need at least one output (Y, resid, energy)");
  DEIG_REQUIRE(!Y || ldy >= k, "pca_transform: ldy must be >= k");
  DEIG_REQUIRE(X && W && aligned16(X), "pca_transform: X (16-byte aligned) and W must not be NULL");
  DEIG_REQUIRE(reinterpret_cast<uintptr_t>(mean) % 8 == 0, "pca_transform: mean must be 8-byte aligned");
  const size_t need = pca_transform_workspace_bytes(n, d, k);
  if (!ws || ws_bytes < need)
    return fail(DEIG_EWORKSPACE, "pca_transform: workspace %zu bytes < required %zu", ws_bytes, need);
  const int kp = (int)cdiv(k, 16) * 16;
  float* Wr = static_cast<float*>(ws);
  if (int rc = pack_w_launch(W, ldw, d, k, kp, Wr, st)) return rc;
  switch (kp / 16) {
#define DEIG_NB(x) \
  case x:          \
    return pca_launch_nb<x>(X, ldx, mean, Wr, Y, ldy, resid, energy, n, d, k, st);
    DEIG_NB(1) DEIG_NB(2) DEIG_NB(3) DEIG_NB(4) DEIG_NB(5) DEIG_NB(6) DEIG_NB(7) DEIG_NB(8)
    DEIG_NB(9) DEIG_NB(10) DEIG_NB(11) DEIG_NB(12) DEIG_NB(13) DEIG_NB(14) DEIG_NB(15)
    DEIG_NB(16)
#undef DEIG_NB
  }
  return fail(DEIG_EINVAL, "pca_transform: unsupported k = %d", k);
}

}  // namespace deig
