// The sample operator of the covariance-free worker solve (deig_gram_apply):
//   Y = alpha * Xc^T (Xc Q),   Xc[r][j] = fl32((double)x_rj - c_j)   (c == NULL: x widened exactly)
// X: n x d row-major float32, bf16 or raw bytes, Q and Y: d x p row-major, p % 16 == 0, p <= 128.
// No d x d matrix is formed: X is read twice per apply, in row chunks of the workspace's size.
//
// Per chunk of rows:
//  1. Zt = Xc Q (chunk x p) with the fused transform kernels as they are (pca.hip,
//     pca_u8.hip, pca_bf16.hip: Y only, no energy, no residual), their W image packed from the
//     row-major Q;
//  2. Y (+)= alpha Xc^T Zt with gram_tn_kernel below, the packed and centred sibling of
//     skinny_kernel<NB, TRANS = true> on the same tile body (skinny_tile.hpp): the 64 rows of
//     a block tile are FEATURES, the inner dimension runs over the rows of X.  X is row-major,
//     so a chunk of 32 rows x 64 features already lies in memory in the k-major LDS order
//     [slot][feature] and is staged without a transpose, with the padded A layout (row stride
//     80) and float4 LDS stores of skinny_kernel's transposed path.
//     Staging map, the same for the three sources: element group f = tid + 256 u (u = 0, 1)
//     is row f >> 4 of the chunk and features 4 (f & 15) .. + 3 of the tile: a 16-byte load of
//     float32, 8 bytes of bf16, one dword of bytes (SampleGroup, sample_src.hpp).  A thread's
//     features are the same in every chunk, so its four centre entries are loaded once before
//     the K loop.  Centring is a uniform run-time branch where a value is staged (centre1);
//     rows past the chunk and features past d stage exact zeros; d is a multiple of the load
//     group, so nothing behind column d of a row is read.
//     A chunk row of a tile is 256 B of float32, 128 B of bf16 and 64 B of bytes - half a cache
//     line.  The linear block id is relabelled with xcd_logical, so the blocks that one XCD
//     runs hold neighbouring feature tiles of one K slice and the other half of a byte row's
//     line is served by that XCD's L2.
//     Split-K over the chunk's rows: fp32 partial slabs summed in slice order by
//     skinny_reduce_kernel, which also applies alpha and adds the chunks before (beta = 1 from
//     the second chunk on).  Fixed order, no atomics: repeated calls give identical bits.
#include "sample_src.hpp"
#include "skinny_tile.hpp"

namespace deig {
namespace {

constexpr int GBM = tile::kRows, GBK = tile::kChunk;
constexpr int GT = tile::kThreads, GAST = tile::kAStridePadded;

// C[d x N] (ldc) = alpha Xc^T B + beta C for the K rows of X at X (ks == 1), or slice sl's
// partial sums into part[sl][d][N].  B: K x N row-major, row stride N.
template <int NB, class Src>
__global__ __launch_bounds__(GT) void gram_tn_kernel(const typename Src::Elem* __restrict__ X,
                                                     int64_t ldx, const double* __restrict__ center,
                                                     const float* __restrict__ B, float* __restrict__ C,
                                                     int64_t ldc, int64_t d, int64_t K, float alpha,
                                                     float beta, float* __restrict__ part, int G,
                                                     int ks) {
  constexpr int N = NB * 16;
  constexpr int BST = tile::bstride(N);
  constexpr int NB4 = GBK * N / 4, BPT = tile::b_per_thread(NB);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                   // [2][GBK][GAST]
  float* Bs = smem + 2 * GBK * GAST;  // [2][GBK][BST]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // neighbouring feature tiles of one slice on one XCD (G tiles x ks slices, a 1-D grid)
#ifdef DEIG_AB_GRAM_LINEAR_TILES  // measurement builds only (tools/topk_samples_bench.py --ab-lib)
  const int lb = (int)blockIdx.x;
#else
  const int lb = xcd_logical((int)blockIdx.x, G * ks);
#endif
  const int sl = lb / G;
  const int64_t m0 = (int64_t)(lb - sl * G) * GBM;
  const int64_t nch = (K + GBK - 1) / GBK;
  const int64_t c0 = nch * sl / ks, c1 = nch * (sl + 1) / ks;

  f32x4 acc[NB][1];
#pragma unroll
  for (int j = 0; j < NB; ++j) acc[j][0] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging map: rows arow and arow + 16 of a chunk, features m0 + 4 c4 .. + 3
  const int arow = tid >> 4, c4 = tid & 15;
  const int64_t mf = m0 + 4 * c4;
  const bool fin = mf < d;  // d % 4 == 0: the four features are in or out together
  const bool centred = center != nullptr;
  double mu[4] = {0.0, 0.0, 0.0, 0.0};
  if (centred && fin) {
#pragma unroll
    for (int e = 0; e < 4; ++e) mu[e] = center[mf + e];
  }

  typename Src::Raw ra[2];
  bool live[2];
  f32x4 rb[BPT];

  auto load = [&](int64_t ch) {
    const int64_t kb = ch * GBK;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t k = kb + arow + 16 * u;
      live[u] = fin && k < K;
      ra[u] = live[u] ? Src::load(X + k * ldx + mf) : Src::zero();
    }
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      const int f = tid + GT * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (f < NB4) {
        const int row = f / (N / 4), b4 = f % (N / 4);
        const int64_t k = kb + row;
        if (k < K) v = *reinterpret_cast<const f32x4*>(B + k * N + 4 * b4);
      }
      rb[u] = v;
    }
  };
  // centring happens here, one rounding per value; dead rows and features stay exactly zero
  auto store = [&](int buf) {
    float* as = As + buf * GBK * GAST;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      f32x4 t;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = Src::value(ra[u], e);
        t[e] = centred ? (live[u] ? centre1(v, mu[e]) : 0.f) : v;
      }
      *reinterpret_cast<f32x4*>(as + (arow + 16 * u) * GAST + 4 * c4) = t;
    }
    tile::store_b<NB>(Bs + buf * GBK * BST, rb, tid);
  };

  const int r = lane & 15, kk = lane >> 4;
  if (c0 < c1) {
    load(c0);
    store(0);
    __syncthreads();
    int cur = 0;
    for (int64_t ch = c0; ch < c1; ++ch) {
      const bool more = ch + 1 < c1;
      if (more) load(ch + 1);
      const float* as = As + cur * GBK * GAST + kk * GAST + 16 * wave + r;
      tile::mfma_chunk(acc, Bs + cur * GBK * BST, r, kk, [&](int s) { return as[4 * s * GAST]; });
      if (more) store(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }

  const int64_t mrow = m0 + 16 * wave + 4 * kk;
  if (ks == 1) {
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t m = mrow + e;
        if (m < d) {
          float* cp = C + m * ldc + 16 * j + r;
          const float v = alpha * acc[j][0][e];
          *cp = (beta != 0.0f) ? v + beta * *cp : v;
        }
      }
  } else {
    float* pp = part + (int64_t)sl * d * N;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t m = mrow + e;
        if (m < d) pp[m * N + 16 * j + r] = acc[j][0][e];
      }
  }
}

// Split-K of the second product over a chunk of K rows: skinny.hip's rule (about four blocks
// per CU, at least 8 inner chunks per slice).  Does not decrease in K.
int gram_ks(int64_t d, int64_t K) { return skinny_split_k(d, K); }

// The first product Zt = Xc Q (rows x p, Y only) and its workspace, per sample type: the three
// fused transform launchers behind one signature.
size_t transform_ws(SampleGroup<float>, int64_t rows, int64_t d, int p) {
  return pca_transform_workspace_bytes(rows, d, p);
}
size_t transform_ws(SampleGroup<bf16_t>, int64_t rows, int64_t d, int p) {
  return pca_transform_bf16_workspace_bytes(rows, d, p);
}
size_t transform_ws(SampleGroup<uint8_t>, int64_t rows, int64_t d, int p) {
  return pca_transform_u8_workspace_bytes(rows, d, p);
}
int transform(SampleGroup<float>, const void* X, int64_t rows, int64_t d, int64_t ldx, const double* center,
              const float* Q, int p, int64_t ldq, float* Zt, void* ws, size_t ws_bytes, hipStream_t st) {
  return pca_transform_launch(static_cast<const float*>(X), rows, d, ldx, center, Q, p, ldq, Zt, p, nullptr,
                              nullptr, ws, ws_bytes, st, true);
}
int transform(SampleGroup<bf16_t>, const void* X, int64_t rows, int64_t d, int64_t ldx, const double* center,
              const float* Q, int p, int64_t ldq, float* Zt, void* ws, size_t ws_bytes, hipStream_t st) {
  return pca_transform_bf16_launch(X, rows, d, ldx, center, Q, p, ldq, Zt, p, nullptr, nullptr, ws, ws_bytes,
                                   st, true);
}
int transform(SampleGroup<uint8_t>, const void* X, int64_t rows, int64_t d, int64_t ldx, const double* center,
              const float* Q, int p, int64_t ldq, float* Zt, void* ws, size_t ws_bytes, hipStream_t st) {
  return pca_transform_u8_launch(static_cast<const uint8_t*>(X), rows, d, ldx, DEIG_U8_RAW, center, Q, p, ldq,
                                 Zt, p, nullptr, nullptr, ws, ws_bytes, st, true);
}

struct GramWs {
  float* Zt;
  void* tw;
  size_t tw_bytes;
  float* slab;
};

// The workspace of a chunk of `rows` rows; its size does not decrease in rows.
GramWs carve_gram(void* ws, size_t cap, int64_t rows, int64_t d, int p, int xtype, size_t* total) {
  Carve c(ws, cap);
  GramWs g;
  g.Zt = c.take<float>((size_t)rows * p);
  g.tw_bytes = dispatch_sample(xtype, [&](auto s) { return transform_ws(s, rows, d, p); });
  g.tw = c.take<char>(g.tw_bytes);
  const int ks = gram_ks(d, rows);
  g.slab = c.take<float>(ks > 1 ? (size_t)ks * d * p : 0);
  *total = align_up(c.off, 256);
  return g;
}

bool gram_shape_ok(int64_t n, int64_t d, int p, int xtype) {
  if (!sample_type(xtype)) return false;
  const int q = kSampleRules[xtype].group;
  return n >= 1 && d >= 16 && d % q == 0 && d <= (int64_t(1) << 31) - 64 && p >= 16 && p <= 128 &&
         p % 16 == 0;
}

template <class Src>
int launch_tn(const void* X, int64_t ldx, const double* center, const float* Zt, float* Y, int64_t ldy,
              int64_t d, int64_t K, int p, float alpha, float beta, float* slab, int ks,
              hipStream_t st) {
  const int G = (int)cdiv(d, GBM);
  const dim3 grid((unsigned)((int64_t)G * ks));
  const int rc = tile::dispatch_nb(p / 16, [&](auto nb) {
    if constexpr (nb() <= 8)
      return tile::launch<gram_tn_kernel<nb(), Src>>(
          grid, tile::shm_bytes(nb() * 16, GAST), st, static_cast<const typename Src::Elem*>(X), ldx,
          center, Zt, Y, ldy, d, K, alpha, beta, slab, G, ks);
    else
      return (int)tile::kNoSuchNb;
  });
  if (rc == tile::kNoSuchNb) return fail(DEIG_EINVAL, "gram_apply: unsupported p = %d", p);
  if (rc) return rc;
  if (ks > 1) return skinny_reduce_launch(slab, ks, Y, ldy, d, p, alpha, beta, st);
  return DEIG_OK;
}

}  // namespace

// The second product alone, for the dual solve's back-projection (capi.hip deig_topk_dual):
// Y (d x p row-major, ldy) = alpha Xc^T Zt for all n rows of X at once, Zt n x p row-major
// with row stride p.  slab: gram_tn_split(d, n) * d * p floats when that is > 1.
int gram_tn_split(int64_t d, int64_t n) { return gram_ks(d, n); }

int gram_tn_launch(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, const double* center,
                   const float* Zt, int p, float alpha, float* Y, int64_t ldy, float* slab,
                   hipStream_t st) {
  return dispatch_sample(xtype, [&](auto s) {
    return launch_tn<decltype(s)>(X, ldx, center, Zt, Y, ldy, d, n, p, alpha, 0.f, slab, gram_ks(d, n), st);
  });
}

// Rows per chunk that the workspace query recommends: all of them, up to 2^20 (Zt is then at
// most 512 MB at p = 128).  Measured (profiles/topk_samples.json, 65536 x 16384, p = 80): a
// chunk small enough for the 256 MB last-level cache does NOT make the second read of X
// cheaper than what more chunks cost - every chunk packs Q again and launches a transform of
// chunk / 64 blocks, which under-fills the chip; one chunk ran the apply in 4.0 - 4.4 ms,
// sixteen in 14.6 - 17.4 ms.
int64_t gram_recommended_rows(int64_t n, int64_t d, int xtype) {
  (void)d;
  (void)xtype;
  const int64_t cap = int64_t(1) << 20;
  return n < cap ? n : cap;
}

size_t gram_apply_workspace_bytes(int64_t n, int64_t d, int p, int xtype) {
  if (!gram_shape_ok(n, d, p, xtype)) return 0;
  size_t total = 0;
  carve_gram(nullptr, 0, gram_recommended_rows(n, d, xtype), d, p, xtype, &total);
  return total;
}

int gram_apply_check(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, const double* center,
                     const char* what) {
  DEIG_REQUIRE(sample_type(xtype), "%s: xtype must be DEIG_F32, DEIG_BF16 or DEIG_U8 (got %d)", what, xtype);
  const int q = kSampleRules[xtype].group;
  const size_t xalign = kSampleRules[xtype].align;
  DEIG_REQUIRE(n >= 1, "%s: n must be >= 1 (got %lld)", what, (long long)n);
  DEIG_REQUIRE(d >= 16, "%s: d must be >= 16 (got %lld)", what, (long long)d);
  DEIG_REQUIRE(d % q == 0 && d <= (int64_t(1) << 31) - 64, "%s: d must be a multiple of %d (got %lld)",
               what, q, (long long)d);
  DEIG_REQUIRE(ldx >= d, "%s: ldx must be >= d", what);
  DEIG_REQUIRE(ldx % q == 0, "%s: ldx must be a multiple of %d elements", what, q);
  DEIG_REQUIRE(X, "%s: X must not be NULL", what);
  DEIG_REQUIRE(reinterpret_cast<uintptr_t>(X) % xalign == 0, "%s: X must be %zu-byte aligned", what,
               xalign);
  DEIG_REQUIRE(reinterpret_cast<uintptr_t>(center) % sizeof(double) == 0,
               "%s: center must be aligned to its element size", what);
  return DEIG_OK;
}

int gram_apply_launch(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, const double* center,
                      float alpha, const float* Q, int p, int64_t ldq, float* Y, int64_t ldy, void* ws,
                      size_t ws_bytes, hipStream_t st) {
  const char* what = "gram_apply";
  if (int rc = gram_apply_check(X, xtype, n, d, ldx, center, what)) return rc;
  DEIG_REQUIRE(p >= 16 && p <= 128 && p % 16 == 0, "%s: p must be a multiple of 16 in 16..128 (got %d)",
               what, p);
  DEIG_REQUIRE(Q && Y, "%s: Q and Y must not be NULL", what);
  DEIG_REQUIRE(aligned16(Q) && aligned16(Y), "%s: Q and Y must be 16-byte aligned", what);
  DEIG_REQUIRE(ldq >= p && ldq % 4 == 0, "%s: ldq must be >= p and a multiple of 4", what);
  DEIG_REQUIRE(ldy >= p && ldy % 4 == 0, "%s: ldy must be >= p and a multiple of 4", what);
  // the chunk: the most rows (<= n) whose workspace fits; sizes do not decrease in rows
  size_t total = 0;
  carve_gram(nullptr, 0, 1, d, p, xtype, &total);
  if (!ws || ws_bytes < total)
    return fail(DEIG_EWORKSPACE, "%s: workspace %zu bytes < required %zu (a chunk of one row)", what,
                ws ? ws_bytes : (size_t)0, total);
  int64_t lo = 1, hi = n;  // carve(lo) fits
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    carve_gram(nullptr, 0, mid, d, p, xtype, &total);
    if (total <= ws_bytes)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int64_t chunk = lo;
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t rows = n - r0 < chunk ? n - r0 : chunk;
    const GramWs g = carve_gram(ws, ws_bytes, rows, d, p, xtype, &total);
    const char* Xr = static_cast<const char*>(X) + (size_t)r0 * ldx * elem_bytes(xtype);
    const int rc = dispatch_sample(xtype, [&](auto s) {
      if (int e = transform(s, Xr, rows, d, ldx, center, Q, p, ldq, g.Zt, g.tw, g.tw_bytes, st)) return e;
      return launch_tn<decltype(s)>(Xr, ldx, center, g.Zt, Y, ldy, d, rows, p, alpha, r0 ? 1.f : 0.f, g.slab,
                                    gram_ks(d, rows), st);
    });
    if (rc) return rc;
  }
  return DEIG_OK;
}

}  // namespace deig
