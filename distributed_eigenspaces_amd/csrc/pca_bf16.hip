// Fused centred transform of bf16 samples (deig_pca_transform_bf16):
//   Y = (X - 1 mean^T) W,   energy_i = ||x_i - mean||^2,   resid_i = max(0, energy_i - ||y_i||^2)
// X: n x d row-major bf16 (the upper 16 bits of the fp32 value), read once and never widened in
// memory; mean, W, Y, resid, energy as deig_pca_transform_f32 (pca.hip).
//
// The third kernel on skinny_tile.hpp's block tile, next to pca_transform_kernel (pca.hip) and
// pca_transform_u8_kernel (pca_u8.hip): the W chunk's LDS store, the MFMA chunk product and the
// host-side dispatch and launch are that header's, the epilogue too, as text (see the end of
// the kernel, and pca_u8.hip for why); no atomics.  Only the staging is this kernel's own, and
// it is pca_u8.hip's super-chunk scheme at the width of bf16:
//  * a SUPER-CHUNK is 64 features: 8 threads per row, 8 features per thread - one 16-byte load,
//    128 contiguous bytes per row, a whole cache line - held in registers and consumed by TWO
//    compute chunks;
//  * compute chunk c of a super-chunk takes features 8 q + 4 c .. + 3 of every thread q: LDS
//    slot 4 q + e of the chunk is feature 8 q + 4 c + e, and slot s of the W chunk is row
//    8 (s >> 2) + 4 c + (s & 3) of the super-chunk (the order of a dot product's terms is free
//    as long as W's rows follow);
//  * the staged values sit in pca_u8.hip's XOR-swizzled layout (a_swz there: neither the
//    staging writes nor the MFMA reads conflict on a bank);
//  * W's image and the mean are padded with zeros to whole super-chunks in the workspace, so
//    the per-chunk loads carry no predicate on d; d % 8 == 0, so every super-chunk runs both
//    chunks and the stage buffer of chunk c is c itself;
//  * the loads of super-chunk j + 1 are issued when super-chunk j's first chunk starts.
// Centring at staging: t = fl32((double)x - mean), one rounding; without a mean the exact
// widening bits << 16.  Rows past n and features past d stage exact zeros.
#include "skinny_tile.hpp"

namespace deig {
namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int HBM = tile::kRows, HT = tile::kThreads;
constexpr int HBK = tile::kChunk;  // LDS slots (features) per compute chunk
constexpr int HSK = 2 * HBK;       // features per super-chunk (2 compute chunks)
constexpr int HAST = HBM;          // row stride of a staged slot: no padding, XOR-swizzled rows

// pca_u8.hip's swizzle: slot sl x row at sl * HAST + (row ^ a_swz(sl)).  A staging write has e
// fixed and, per half wave, rows m .. m + 3 with the 8 threads kq of each: sl = 4 kq + e, the
// XOR with 4 kq spreads a row's 8 threads over 8 bank groups of 4.  An MFMA read has s fixed
// and, per half, kk = (0, 1) or (2, 3) with 16 rows each: the XOR with (sl & 1) << 4 sends the
// odd kk to the other 16 banks.
__device__ __forceinline__ int a_swz(int sl) { return (sl & 28) ^ ((sl & 1) << 4); }

template <int NB>
__global__ __launch_bounds__(HT) void pca_transform_bf16_kernel(
    const uint16_t* __restrict__ X, int64_t ldx, const double* __restrict__ mean,
    const float* __restrict__ Wr, float* __restrict__ Y, int64_t ldy, float* __restrict__ resid,
    float* __restrict__ energy, int64_t n, int64_t d, int k) {
  constexpr int N = NB * 16;
  constexpr int KA = NB == 1 ? 2 : 1;  // accumulators per fragment
  constexpr int BST = tile::bstride(N);
  constexpr int NB4 = HBK * N / 4, BPT = tile::b_per_thread(NB);  // float4s per chunk, per thread
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                   // [2][HBK][HAST]
  float* Bs = smem + 2 * HBK * HAST;  // [2][HBK][BST]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * HBM;
  const int64_t nsc = (d + HSK - 1) / HSK;
  // staging map: thread -> rows mm and mm + 32 of the tile, features 8 kq .. 8 kq + 7 of a
  // super-chunk
  const int mm = tid >> 3, kq = tid & 7;
  const bool rowlive[2] = {m0 + mm < n, m0 + mm + 32 < n};

  f32x4 acc[NB][KA];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int a = 0; a < KA; ++a) acc[j][a] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint32_t xa[2][4], xb[2][4];  // this and the next super-chunk's elements, two per dword
  f32x4 rb[BPT];
  double mu[4] = {0.0, 0.0, 0.0, 0.0};
  float en[2] = {0.f, 0.f};

  // 8 features of two rows: one 16-byte load where they lie inside d (d % 8 == 0: in or out
  // together) - nothing past column d of a row is ever read
  auto load_x = [&](int64_t sc, uint32_t (&x)[2][4]) {
    const int64_t kc = sc * HSK + 8 * kq;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (rowlive[u] && kc < d)
        v = *reinterpret_cast<const u32x4*>(X + (m0 + mm + 32 * u) * ldx + kc);
#pragma unroll
      for (int w = 0; w < 4; ++w) x[u][w] = v[w];
    }
  };
  // chunk c of super-chunk sc: this thread's mean entries and its share of the W chunk, both
  // from images padded with zeros to a whole super-chunk (pca_transform_bf16_launch): no
  // predicate on d here, and a feature past d stages fl32(0 - 0) = 0 by itself
  auto load_wm = [&](int64_t sc, int c) {
    const int64_t kb = sc * HSK;
    const int64_t kc = kb + 8 * kq + 4 * c;
    if (mean) {
#pragma unroll
      for (int e = 0; e < 4; ++e) mu[e] = mean[kc + e];
    }
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      const int f = tid + HT * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (f < NB4) {
        const int slot = f / (N / 4), c4 = f % (N / 4);
        const int64_t kr = kb + 8 * (slot >> 2) + 4 * c + (slot & 3);
        v = *reinterpret_cast<const f32x4*>(Wr + kr * N + 4 * c4);
      }
      rb[u] = v;
    }
  };
  // centring happens here: t = fl32(x - mean) in double, one rounding; rows past n are set to
  // zero, features past d are zero elements against a zero mean
  auto store = [&](int buf, const uint32_t (&x)[2][4], int c) {
    float* as = As + buf * HBK * HAST;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t w = x[u][2 * c + (e >> 1)];
        const float v = __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16));  // exact
        float t = mean ? (float)((double)v - mu[e]) : v;
        if (!rowlive[u]) t = 0.f;
        en[u] = fmaf(t, t, en[u]);
        as[(4 * kq + e) * HAST + ((mm + 32 * u) ^ a_swz(4 * kq + e))] = t;
      }
    }
    tile::store_b<NB>(Bs + buf * HBK * BST, rb, tid);
  };

  const int r = lane & 15, kk = lane >> 4;
  const int arow = (16 * wave + r) ^ ((kk & 1) << 4);  // this lane's A row, swizzled but for 4 s
  load_x(0, xa);
  load_wm(0, 0);
  store(0, xa, 0);
  __syncthreads();
  for (int64_t sc = 0; sc < nsc; ++sc) {
    const bool msc = sc + 1 < nsc;
    if (msc) load_x(sc + 1, xb);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const bool within = c == 0;
      const bool more = within || msc;
      if (more) {
        if (within)
          load_wm(sc, 1);
        else
          load_wm(sc + 1, 0);
      }
      const float* as = As + c * HBK * HAST + kk * HAST;
      // a_swz(4 s + kk), kk's bit in arow
      tile::mfma_chunk(acc, Bs + c * HBK * BST, r, kk,
                       [&](int s) { return as[4 * s * HAST + (arow ^ (4 * s))]; });
      if (more) {
        if (within)
          store(1, xa, 1);
        else
          store(0, xb, 0);
      }
      __syncthreads();
    }
    if (msc) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w) xa[u][w] = xb[u][w];
    }
  }

  // The text of tile::transform_epilogue (as in pca_u8.hip: called as the helper, the K loop
  // issues one of the staging's packed energy fmas as two scalar ones).
  float* es = smem;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    float e = en[u];
    e += __shfl_xor(e, 1);
    e += __shfl_xor(e, 2);
    e += __shfl_xor(e, 4);
    if (kq == 0) es[mm + 32 * u] = e;
  }
  __syncthreads();

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

// mean -> a copy padded with zeros to dpad entries
__global__ __launch_bounds__(256) void pad_mean_bf16_kernel(const double* __restrict__ mean,
                                                            int64_t d, int64_t dpad,
                                                            double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < dpad) out[i] = i < d ? mean[i] : 0.0;
}

size_t mean_off(int64_t dpad, int kp) { return align_up((size_t)dpad * kp * sizeof(float), 256); }

}  // namespace

// Workspace: the packed W image and the mean, both padded with zeros to whole super-chunks.
size_t pca_transform_bf16_workspace_bytes(int64_t n, int64_t d, int k) {
  if (n < 1 || d < 1 || k < 1 || k > 256) return 0;
  const int64_t dpad = cdiv(d, HSK) * HSK;
  const int kp = (int)cdiv(k, 16) * 16;
  return mean_off(dpad, kp) + align_up((size_t)dpad * sizeof(double), 256);
}

int pca_transform_bf16_launch(const void* X, int64_t n, int64_t d, int64_t ldx, const double* mean,
                              const float* W, int k, int64_t ldw, float* Y, int64_t ldy,
                              float* resid, float* energy, void* ws, size_t ws_bytes,
                              hipStream_t st) {
  DEIG_REQUIRE(k >= 1 && k <= 256, "pca_transform_bf16: k=%d must be in 1..256", k);
  DEIG_REQUIRE(n >= 1, "pca_transform_bf16: n must be >= 1 (got %lld)", (long long)n);
  DEIG_REQUIRE(d >= 8 && d % 8 == 0 && d <= (int64_t(1) << 31),
               "pca_transform_bf16: d must be a multiple of 8 (got %lld)", (long long)d);
  DEIG_REQUIRE(ldx >= d && ldx % 8 == 0,
               "pca_transform_bf16: ldx must be >= d and a multiple of 8 elements");
  DEIG_REQUIRE(ldw >= d, "pca_transform_bf16: ldw must be >= d");
  DEIG_REQUIRE(Y || resid || energy,
               "pca_transform_bf16: need at least one output (Y, resid, energy)");
  DEIG_REQUIRE(!Y || ldy >= k, "pca_transform_bf16: ldy must be >= k");
  DEIG_REQUIRE(X && aligned16(X) && W,
               "pca_transform_bf16: X (16-byte aligned) and W must not be NULL");
  DEIG_REQUIRE(reinterpret_cast<uintptr_t>(mean) % 8 == 0,
               "pca_transform_bf16: mean must be 8-byte aligned");
  const size_t need = pca_transform_bf16_workspace_bytes(n, d, k);
  if (!ws || ws_bytes < need)
    return fail(DEIG_EWORKSPACE, "pca_transform_bf16: workspace %zu bytes < required %zu", ws_bytes,
                need);
  const int kp = (int)cdiv(k, 16) * 16;
  const int64_t dpad = cdiv(d, HSK) * HSK;
  float* Wr = static_cast<float*>(ws);
  if (int rc = pack_w_launch(W, ldw, d, k, kp, Wr, st)) return rc;
  if (dpad > d)
    DEIG_HIP_CHECK(hipMemsetAsync(Wr + d * kp, 0, sizeof(float) * (size_t)(dpad - d) * kp, st));
  double* mpad = nullptr;
  if (mean) {
    mpad = reinterpret_cast<double*>(static_cast<char*>(ws) + mean_off(dpad, kp));
    hipLaunchKernelGGL(pad_mean_bf16_kernel, dim3((unsigned)cdiv(dpad, 256)), dim3(256), 0, st, mean,
                       d, dpad, mpad);
    DEIG_HIP_CHECK(hipGetLastError());
  }
  const dim3 grid((unsigned)cdiv(n, HBM));
  const int rc = tile::dispatch_nb(kp / 16, [&](auto nb) {
    return tile::launch<pca_transform_bf16_kernel<nb()>>(
        grid, tile::shm_bytes(nb() * 16, HAST), st, static_cast<const uint16_t*>(X), ldx, mpad, Wr, Y,
        ldy, resid, energy, n, d, k);
  });
  if (rc == tile::kNoSuchNb) return fail(DEIG_EINVAL, "pca_transform_bf16: unsupported k = %d", k);
  return rc;
}

}  // namespace deig
