// The sample-space (dual) Gram matrix of the wide-data worker solve (deig_gram_outer):
//   K = alpha Xc Xc^T  (n x n),   Xc[r][j] = fl32((double)x_rj - c_j)   (c == NULL: x widened exactly)
// X: n x d row-major float32, bf16 or raw bytes, n <= 32768.  The inner dimension of the
// product is the contiguous one of X, so the operand image of syrk_image_tile.hpp is staged
// without a transpose, its roles swapped: the image's "feature" index is the sample row i and
// the K-steps run over the features of X.
//
// Per chunk of features (the chunk is what the workspace's image holds):
//  * gnt_prep_kernel stages t = Xc as bf16 pieces: a hi plane bf16(t) (round to nearest even)
//    at image indices [0, npad) and - where a staged value can have one: float32 samples and
//    every centred call - a lo plane bf16(t - hi) at [npad, 2 npad); fpad = planes * npad,
//    npad = n rounded up to 128.  Uncentred bf16 and uint8 samples are their own hi piece.
//    One wave stages 16 rows x 32 features (one K-step) at a time: lane (g, r) loads the 8
//    features 32 kb + 8 g .. + 7 of row r as two SampleGroups (32 / 16 / 8 bytes; the four
//    lanes of a row read 128 / 64 / 32 contiguous bytes) and stores one 16-byte entry per
//    plane - the 16 lanes of a g write a 256-byte run.  A wave walks kKpw consecutive K-steps
//    of its rows, so the cache line it has touched is used up by its own next steps.  Rows
//    >= n and features past the chunk stage exact zeros and are not read.
//  * gnt_kernel: one workgroup per (lower 128 x 128 tile of K, K segment) runs
//    itile::k_loop<Bf16Op> as it stands - once (hi, hi), and with a lo plane twice more into
//    the same accumulators, (hi, lo) then (lo, hi), by shifting the item's i0 / j0 into the
//    lo plane with diag = false (B is then read from its own panel).  lo * lo is dropped.
//    The accumulators go to a slab of the item's own; nobody waits on anybody, no atomics.
//  * bf16_reduce_kernel (syrk_bf16_tile.hpp) adds the segments' slabs in order, applies alpha,
//    adds the chunks before (beta) and writes K[i][j] and K[j][i] from one value.
//
// Schedule (gnt_segs).  A segment takes at most kFlushRows = 16384 features (the two-level
// summation rule: no accumulator sums more than 16384 inner elements per pass before it is
// written out).  Beyond that, K is split over features until the grid holds about two
// workgroups per CU (kItemsTarget = 512 items), each segment keeping at least 4 stages: at
// n <= 1024 (at most 36 lower tiles) that asks for cdiv(512, tiles) = 15 .. 512 segments, at
// n >= 4096 (528 tiles and more) for one, so there the flush limit alone splits K.  The
// slabs are sized by the chunk's segment count.
//
// The dual solve's two small kernels stand here too: the scaled transposed start
// Zt = U diag(sqrt(scale / lambda)) and the column-major relayout of Xc^T Zt.
#include "sample_src.hpp"
#include "syrk_bf16_tile.hpp"

namespace deig {
namespace {

constexpr int kKpw = 4;                            // consecutive K-steps per wave of the prep
constexpr int64_t kMaxChunkStages = 32 * kSegStages;  // features per chunk at most: 2^19
constexpr int64_t kMaxN = 1 << 15;

// grid (npad / 16, cdiv(nkb, 4 kKpw)); X, center and dc are the chunk's: X points at its
// first feature, dc features of it are live.
template <class Src, bool LO>
__global__ __launch_bounds__(THR) void gnt_prep_kernel(const typename Src::Elem* __restrict__ X, int64_t n,
                                                       int64_t ldx, int64_t dc,
                                                       const double* __restrict__ center, int64_t npad,
                                                       int64_t nkb, uint8_t* __restrict__ img) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int64_t i = (int64_t)blockIdx.x * 16 + r;  // < npad
  const int64_t fpad = LO ? 2 * npad : npad;
  const bool centred = center != nullptr;
  const int64_t kb0 = ((int64_t)blockIdx.y * 4 + wave) * kKpw;
  for (int q = 0; q < kKpw; ++q) {
    const int64_t kb = kb0 + q;
    if (kb >= nkb) break;
    const int64_t f = kb * KB + 8 * g;
    float t[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t ff = f + 4 * h;
      const bool live = i < n && ff < dc;  // dc % group == 0: the four are in or out together
      const typename Src::Raw raw = live ? Src::load(X + i * ldx + ff) : Src::zero();
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = Src::value(raw, e);
        t[4 * h + e] = centred ? (live ? centre1(v, center[ff + e]) : 0.f) : v;
      }
    }
    u32x4 hi;
#pragma unroll
    for (int w = 0; w < 4; ++w) hi[w] = cvt2(t[2 * w], t[2 * w + 1]);
    *reinterpret_cast<u32x4*>(img + img_off(kb, g, i, fpad)) = hi;
    if (LO) {
      u32x4 lo;
#pragma unroll
      for (int w = 0; w < 4; ++w) lo[w] = cvt2(t[2 * w] - lo_f(hi[w]), t[2 * w + 1] - hi_f(hi[w]));
      *reinterpret_cast<u32x4*>(img + img_off(kb, g, npad + i, fpad)) = lo;
    }
  }
}

struct GntSched {
  const uint8_t* img;
  float* slabs;        // [seg][tile][wave][MFMA block a, b][lane][4]
  int64_t nst, fpad, npad;  // SB-feature stages of the chunk
  int T, nseg;
};

// One item = (lower tile of K, K segment); the tile, its LDS stages and the K loop are
// syrk_image_tile.hpp's.
template <bool LO>
__global__ __launch_bounds__(THR, WGS) void gnt_kernel(GntSched s) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[itile::lds_bytes<Bf16Op>()];
  const int item = blockIdx.x;
  const int tile = item % s.T, seg = item / s.T;
  int ti, tj;
  tile_of(tile, ti, tj);
  const itile::Item it = itile::item_of(ti, tj);
  const int64_t k0 = s.nst * seg / s.nseg, k1 = s.nst * (seg + 1) / s.nseg;
  if (k0 >= k1) return;  // (never: nseg <= nst; whole block)
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  itile::k_loop<Bf16Op>(s.img, s.fpad, it, k0, k1, lds, acc);  // hi_i . hi_j
  if (LO) {
    itile::Item m = it;
    m.diag = false;  // the B panel is another plane's: read it from its own LDS panel
    m.j0 = it.j0 + s.npad;
    itile::k_loop<Bf16Op>(s.img, s.fpad, m, k0, k1, lds, acc);  // hi_i . lo_j
    m.j0 = it.j0;
    m.i0 = it.i0 + s.npad;
    itile::k_loop<Bf16Op>(s.img, s.fpad, m, k0, k1, lds, acc);  // lo_i . hi_j
  }
  if (!it.active) return;
  f32x4* slab = reinterpret_cast<f32x4*>(s.slabs + ((int64_t)seg * s.T + tile) * kTileFloats) +
                it.wave * 16 * 64 + it.lane;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) slab[(a * 4 + b) * 64] = acc[a][b];
}

struct GntLayout {
  int64_t npad, fpad, T;
  bool lo;
};

GntLayout gnt_layout(int64_t n, bool lo) {
  GntLayout L;
  L.npad = cdiv(n, TB) * TB;
  L.fpad = (lo ? 2 : 1) * L.npad;
  const int64_t nt = L.npad / TB;
  L.T = nt * (nt + 1) / 2;
  L.lo = lo;
  return L;
}

// K segments of a chunk of nst stages (the file's header comment); 1 <= result <= nst, and
// it does not decrease in nst.
int64_t gnt_segs(int64_t T, int64_t nst) {
  int64_t nseg = cdiv(kItemsTarget, T);
  if (nseg > nst / 4) nseg = nst / 4;
  if (nseg < cdiv(nst, kSegStages)) nseg = cdiv(nst, kSegStages);
  return nseg < 1 ? 1 : nseg;
}

size_t gnt_off_img(const GntLayout& L, int64_t nst) {
  return align_up(sizeof(float) * (size_t)gnt_segs(L.T, nst) * L.T * kTileFloats, 256);
}
// Workspace of a chunk of nst stages: slabs, then the image.  Does not decrease in nst.
size_t gnt_bytes(const GntLayout& L, int64_t nst) {
  return gnt_off_img(L, nst) + (size_t)nst * (2 * SB) * (size_t)L.fpad;
}

bool outer_shape_ok(int64_t n, int64_t d, int xtype) {
  if (!sample_type(xtype)) return false;
  return n >= 1 && n <= kMaxN && d >= 16 && d % kSampleRules[xtype].group == 0 &&
         d <= (int64_t(1) << 31) - 64;
}

__global__ void dual_scale_kernel(const float* __restrict__ U, int64_t ldu, const float* __restrict__ lam,
                                  int k, int kp, int k0, float scale, int64_t n, float* __restrict__ Zt) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * kp) return;
  const int64_t r = idx / kp;
  const int j = (int)(idx - r * kp);
  float v = 0.f;
  if (j < k && j >= k - k0) v = U[(int64_t)j * ldu + r] * sqrtf(scale / lam[j]);
  Zt[idx] = v;
}

__global__ void dual_cols_kernel(const float* __restrict__ Y, int kp, int64_t d, int c0, int k0,
                                 float* __restrict__ V0) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= d * k0) return;
  const int64_t c = idx / d, i = idx - c * d;
  V0[idx] = Y[i * kp + c0 + c];
}

}  // namespace

size_t gram_outer_workspace_bytes(int64_t n, int64_t d, int xtype, int centred) {
  if (!outer_shape_ok(n, d, xtype)) return 0;
  const GntLayout L = gnt_layout(n, xtype == DEIG_F32 || centred);
  const int64_t nst = cdiv(d, SB);
  return gnt_bytes(L, nst < kMaxChunkStages ? nst : kMaxChunkStages);
}

int gram_outer_launch(const void* X, int xtype, int64_t n, int64_t d, int64_t ldx, const double* center,
                      float alpha, float* K, int64_t ldk, int flags, void* ws, size_t ws_bytes,
                      hipStream_t stream) {
  const char* what = "gram_outer";
  if (int rc = gram_apply_check(X, xtype, n, d, ldx, center, what)) return rc;
  DEIG_REQUIRE(flags == 0, "%s: flags must be 0 (got 0x%x)", what, flags);
  DEIG_REQUIRE(n <= kMaxN, "%s: n must be <= 32768 (got %lld)", what, (long long)n);
  DEIG_REQUIRE(K, "%s: K must not be NULL", what);
  DEIG_REQUIRE(aligned16(K), "%s: K must be 16-byte aligned", what);
  DEIG_REQUIRE(ldk >= n, "%s: ldk must be >= n", what);
  DEIG_REQUIRE(ldk % 4 == 0, "%s: ldk must be a multiple of 4", what);
  const bool lo = xtype == DEIG_F32 || center != nullptr;
  const GntLayout L = gnt_layout(n, lo);
  const size_t least = gnt_bytes(L, 1);
  if (!ws || ws_bytes < least)
    return fail(DEIG_EWORKSPACE, "%s: workspace %zu bytes < required %zu (a chunk of %d features)", what,
                ws ? ws_bytes : (size_t)0, least, SB);
  // the chunk: the most stages (all of d's at most) whose workspace fits; sizes do not
  // decrease in the stage count
  int64_t s_lo = 1, s_hi = cdiv(d, SB) < kMaxChunkStages ? cdiv(d, SB) : kMaxChunkStages;
  while (s_lo < s_hi) {
    const int64_t mid = s_lo + (s_hi - s_lo + 1) / 2;
    if (gnt_bytes(L, mid) <= ws_bytes)
      s_lo = mid;
    else
      s_hi = mid - 1;
  }
  const int64_t chunk = s_lo * SB;
  char* base = static_cast<char*>(ws);
  uint8_t* img = reinterpret_cast<uint8_t*>(base + gnt_off_img(L, s_lo));
  GntSched s;
  s.img = img;
  s.slabs = reinterpret_cast<float*>(base);
  s.fpad = L.fpad;
  s.npad = L.npad;
  s.T = (int)L.T;
  int beta = 0;
  for (int64_t c0 = 0; c0 < d; c0 += chunk) {
    const int64_t dc = d - c0 < chunk ? d - c0 : chunk;
    const int64_t nst = cdiv(dc, SB), nkb = KS * nst;
    s.nst = nst;
    s.nseg = (int)gnt_segs(L.T, nst);  // <= the segments the slabs were sized for
    const dim3 pgrid((unsigned)(L.npad / 16), (unsigned)cdiv(nkb, 4 * kKpw));
    const char* Xc = static_cast<const char*>(X) + (size_t)c0 * elem_bytes(xtype);
    const double* cc = center ? center + c0 : nullptr;
    dispatch_sample(xtype, [&](auto src) {
      using Src = decltype(src);
      const typename Src::Elem* Xe = reinterpret_cast<const typename Src::Elem*>(Xc);
      if (lo)
        hipLaunchKernelGGL((gnt_prep_kernel<Src, true>), pgrid, dim3(THR), 0, stream, Xe, n, ldx, dc, cc,
                           L.npad, nkb, img);
      else
        hipLaunchKernelGGL((gnt_prep_kernel<Src, false>), pgrid, dim3(THR), 0, stream, Xe, n, ldx, dc, cc,
                           L.npad, nkb, img);
      return 0;
    });
    DEIG_HIP_CHECK(hipGetLastError());
    const dim3 grid((unsigned)(L.T * s.nseg));
    if (lo)
      hipLaunchKernelGGL(gnt_kernel<true>, grid, dim3(THR), 0, stream, s);
    else
      hipLaunchKernelGGL(gnt_kernel<false>, grid, dim3(THR), 0, stream, s);
    DEIG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bf16_reduce_kernel, dim3((unsigned)L.T), dim3(THR), 0, stream, s.slabs, s.T, s.nseg,
                       alpha, beta, K, ldk, n);
    DEIG_HIP_CHECK(hipGetLastError());
    beta = 1;
  }
  return DEIG_OK;
}

int dual_scale_launch(const float* U, int64_t ldu, const float* lam, int k, int kp, int k0, float scale,
                      int64_t n, float* Zt, hipStream_t stream) {
  const int64_t total = n * kp;
  hipLaunchKernelGGL(dual_scale_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, U, ldu, lam,
                     k, kp, k0, scale, n, Zt);
  DEIG_HIP_CHECK(hipGetLastError());
  return DEIG_OK;
}

int dual_cols_launch(const float* Y, int kp, int64_t d, int c0, int k0, float* V0, hipStream_t stream) {
  const int64_t total = d * k0;
  hipLaunchKernelGGL(dual_cols_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, Y, kp, d, c0,
                     k0, V0);
  DEIG_HIP_CHECK(hipGetLastError());
  return DEIG_OK;
}

}  // namespace deig
