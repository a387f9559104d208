// The fused centred transform of packed samples, stated once for deig_pca_transform_u8
// (pca_u8.hip: raw bytes, gray pixels) and deig_pca_transform_bf16 (pca_bf16.hip):
//   Y = (V - 1 mean^T) W,   energy_i = ||v_i - mean||^2,   resid_i = max(0, energy_i - ||y_i||^2)
// V the n x d feature matrix held in X's elements, mean: d doubles in units of v (NULL: no
// centring), W, Y, resid, energy as deig_pca_transform_f32 (pca.hip).  The samples are read
// once and never widened in memory.  Here: the kernel, its workspace and its launch; a
// translation unit adds its sample sources (Src below), its shape rules and the two functions
// deig_internal.hpp declares, and compiles its own 16 NB instantiations per source.
//
// The block tile, the W chunk's LDS store and the MFMA chunk product are skinny_tile.hpp's,
// shared with pca_transform_kernel (pca.hip); the epilogue is that header's too, as text (see
// the end of the kernel); no atomics.  This kernel's own is how a chunk is staged (and with it
// which rows of W a chunk loads):
//  * the float kernel gives 8 threads to a row and 16 B (4 floats) to a thread per 32-column
//    chunk.  With bytes that map would load 4 B per thread and 32-B row segments.  Here the
//    unit of loading is a SUPER-CHUNK of 8 F features: 8 threads per row, F features per
//    thread - F = 16 bytes (one 16-B load; three for the 48 B of gray) or F = 8 bf16 (one
//    16-B load), whole cache lines per row - held in registers and consumed by F / 4 compute
//    chunks (four, two);
//  * compute chunk c of a super-chunk takes features F q + 4 c .. + 3 of every thread q:
//    LDS slot 4 q + e of the chunk is feature F q + 4 c + e.  The order in which the d
//    terms of a dot product are added does not matter as long as W's rows follow, and they
//    do: slot s of the W chunk is row F (s >> 2) + 4 c + (s & 3) (each a contiguous kp-float
//    row of the packed image, so the W loads stay coalesced).  Every thread converts one
//    dword of each of its two rows per chunk (bytes) - the float kernel's staging work per
//    chunk, and an LDS budget just below its ((2 * 32 * 64 + 2 * 32 * bstride(kp)) floats:
//    20 KiB at kp = 16, 36 KiB at kp = 64 - four workgroups per CU - 84 KiB at kp = 256).  A
//    128-feature chunk staged whole would need 4 x that (278 KiB of W alone at kp = 256,
//    over the CU's 160 KiB);
//  * the staged values sit in an XOR-swizzled layout (a_swz below) in which neither the
//    staging writes nor the MFMA reads conflict on a bank; the float kernel's padded layout
//    (row stride 80) puts the 8 staging threads of a row on one bank.  Measured in one run,
//    the same kernel with that padded layout: 2.90 / 5.67 ms at k = 16 / 64 against 2.67 /
//    5.22 ms (2^20 x 3072 raw bytes);
//  * W's image and the mean are padded with zeros to whole super-chunks in the workspace, so
//    the per-chunk loads carry no predicate on d, and the stage buffer of a chunk is its
//    index's parity, a constant of the unrolled loop (immediate LDS offsets).  The staging is
//    bound by instruction issue, not by memory (0.15 of HBM at k = 16, raw bytes): dropping
//    those predicates and address updates took the raw call from 3.29 to 2.67 ms at k = 16;
//  * the loads of super-chunk j + 1 are issued when super-chunk j's first chunk starts: the
//    other chunks' MFMA work to land in.
// Centring at staging: t = fl32((double)v - mean), one rounding (Src::value).  Rows past n
// and features past d stage exact zeros.  Where d need not be a multiple of F (bytes: d % 4
// == 0), a last super-chunk with fewer than F - 3 features left runs only the compute chunks
// that hold any (d % 128 in 4 .. 12: 1 .. 3 chunks), so d = 4 costs one chunk; d = 36 costs
// four partly filled ones where the float kernel has two - small d is not this kernel's case.
//
// Src, a sample source:
//   Elem                  element type of X
//   F                     features per thread and super-chunk (a multiple of 8)
//   DW                    dwords a thread holds per row and super-chunk
//   kShortTail            may the last super-chunk hold fewer than F features per thread?
//   kXAlign               alignment X must have, in bytes
//   load(row, live, kc, d, x)   x = features kc .. kc + F - 1 of the row at `row` (its first
//                         element), zeros where !live or past d; reads nothing past column d
//   value(x, c, e, centred, mu) feature 4 c + e of x as a float, minus mu in double if centred
#pragma once

#include "sample_src.hpp"
#include "skinny_tile.hpp"

namespace deig {
namespace ptile {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kAStride = tile::kRows;  // row stride of a staged slot: no padding, XOR-swizzled rows
template <class Src>
constexpr int kSuper = 8 * Src::F;  // features per super-chunk

// Staged values: slot sl (feature of the chunk) x row, at sl * kAStride + (row ^ a_swz(sl)).
// Both sides of the LDS are then free of bank conflicts (32 banks of 4 B per 32-lane half):
//  * a staging write has e fixed and, per half, rows mm = m .. m + 3 with the 8 threads kq of
//    each: sl = 4 kq + e, so the XOR with 4 kq (= sl & 28) spreads the 8 threads of a row over
//    8 bank groups of 4 - 32 distinct banks (the float kernel's stride-80 layout puts those 8
//    on ONE bank: 8-way);
//  * an MFMA read has s fixed and, per half, kk = (0, 1) or (2, 3) with 16 rows r each:
//    sl = 4 s + kk, sl & 28 = 4 s for both, and the XOR with (sl & 1) << 4 sends the odd kk to
//    the other 16 banks.
__device__ __forceinline__ int a_swz(int sl) { return (sl & 28) ^ ((sl & 1) << 4); }

template <int NB, class Src>
__global__ __launch_bounds__(tile::kThreads) void pca_transform_packed_kernel(
    const typename Src::Elem* __restrict__ X, int64_t ldx, const double* __restrict__ mean,
    const float* __restrict__ Wr, float* __restrict__ Y, int64_t ldy, float* __restrict__ resid,
    float* __restrict__ energy, int64_t n, int64_t d, int k) {
  constexpr int QBM = tile::kRows, QT = tile::kThreads, QAST = kAStride;
  constexpr int QBK = tile::kChunk;  // LDS slots (features) per compute chunk
  constexpr int F = Src::F, DW = Src::DW;
  constexpr int NC = F / 4;          // compute chunks per super-chunk
  constexpr int QSK = kSuper<Src>;
  static_assert(NC % 2 == 0 && NC * QBK == QSK, "a chunk's stage buffer is its index's parity");
  constexpr int N = NB * 16;
  constexpr int KA = NB == 1 ? 2 : 1;  // accumulators per fragment
  constexpr int BST = tile::bstride(N);
  constexpr int NB4 = QBK * N / 4, BPT = tile::b_per_thread(NB);  // float4s per chunk, per thread
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                   // [2][QBK][QAST]
  float* Bs = smem + 2 * QBK * QAST;  // [2][QBK][BST]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * QBM;
  const int64_t nsc = (d + QSK - 1) / QSK;
  // staging map: thread -> rows mm and mm + 32 of the tile, features F kq .. F kq + F - 1 of a
  // super-chunk
  const int mm = tid >> 3, kq = tid & 7;
  const bool rowlive[2] = {m0 + mm < n, m0 + mm + 32 < n};

  f32x4 acc[NB][KA];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int a = 0; a < KA; ++a) acc[j][a] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint32_t xa[2][DW], xb[2][DW];  // this and the next super-chunk's elements
  f32x4 rb[BPT];
  double mu[4] = {0.0, 0.0, 0.0, 0.0};
  float en[2] = {0.f, 0.f};

  auto load_x = [&](int64_t sc, uint32_t (&x)[2][DW]) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
      Src::load(X + (m0 + mm + 32 * u) * ldx, rowlive[u], sc * QSK + F * kq, d, x[u]);
  };
  // chunk c of super-chunk sc: this thread's mean entries and its share of the W chunk.
  // Both come from images padded with zeros to a whole super-chunk (launch below): no
  // predicate on d here, and a feature past d stages fl32(0 - 0) = 0 by itself.
  auto load_wm = [&](int64_t sc, int c) {
    const int64_t kb = sc * QSK;
    const int64_t kc = kb + F * kq + 4 * c;
    if (mean) {
#pragma unroll
      for (int e = 0; e < 4; ++e) mu[e] = mean[kc + e];
    }
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      const int f = tid + QT * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (f < NB4) {
        const int slot = f / (N / 4), c4 = f % (N / 4);
        const int64_t kr = kb + F * (slot >> 2) + 4 * c + (slot & 3);
        v = *reinterpret_cast<const f32x4*>(Wr + kr * N + 4 * c4);
      }
      rb[u] = v;
    }
  };
  // centring happens here (Src::value); rows past n are set to zero, features past d are
  // zero elements against a zero mean
  auto store = [&](int buf, const uint32_t (&x)[2][DW], int c) {
    float* as = As + buf * QBK * QAST;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = Src::value(x[u], c, e, mean != nullptr, mu[e]);
        if (!rowlive[u]) t = 0.f;
        en[u] = fmaf(t, t, en[u]);
        as[(4 * kq + e) * QAST + ((mm + 32 * u) ^ a_swz(4 * kq + e))] = t;
      }
    }
    tile::store_b<NB>(Bs + buf * QBK * BST, rb, tid);
  };

  const int r = lane & 15, kk = lane >> 4;
  const int arow = (16 * wave + r) ^ ((kk & 1) << 4);  // this lane's A row, swizzled but for 4 s
  load_x(0, xa);
  load_wm(0, 0);
  store(0, xa, 0);
  __syncthreads();
  // the stage buffer of chunk c is c & 1: every super-chunk but a short last one runs all NC
  // (even) chunks, so the parity is a compile-time constant of the unrolled loop
  for (int64_t sc = 0; sc < nsc; ++sc) {
    const bool msc = sc + 1 < nsc;
    if (msc) load_x(sc + 1, xb);
    // compute chunks of this super-chunk that hold any feature (NC but for a short tail;
    // without one the tests on ncs fold away)
    const int64_t left = d - sc * QSK;
    const int ncs = !Src::kShortTail || left >= F ? NC : (int)(left / 4);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < ncs) {
        const bool within = c + 1 < ncs;
        const bool more = within || msc;
        if (more) {
          if (within)
            load_wm(sc, c + 1);
          else
            load_wm(sc + 1, 0);
        }
        const int cur = c & 1;
        const float* as = As + cur * QBK * QAST + kk * QAST;
        // a_swz(4 s + kk), kk's bit in arow
        tile::mfma_chunk(acc, Bs + cur * QBK * BST, r, kk,
                         [&](int s) { return as[4 * s * QAST + (arow ^ (4 * s))]; });
        if (more) {
          if (within)
            store(cur ^ 1, xa, (c + 1) % NC);
          else
            store(cur ^ 1, xb, 0);
        }
        __syncthreads();
      }
    }
    if (msc) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w = 0; w < DW; ++w) xa[u][w] = xb[u][w];
    }
  }

  // The text of tile::transform_epilogue (its comment there), the one copy beside the helper.
  // Called as the helper - force-inlined, acc and en by reference - the byte sources' K loops
  // issue staging's packed energy fmas as scalar ones: of 32 v_pk_fma_f32, 31 are left for
  // raw bytes and 28 for gray, at every NB (bf16 keeps its 10).
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

// ---------------------------------------------------------------- host side
// Workspace: the packed W image and the mean, both padded with zeros to whole super-chunks
// of sk features.
inline size_t mean_off(int64_t dpad, int kp) { return align_up((size_t)dpad * kp * sizeof(float), 256); }
inline size_t workspace_bytes(int64_t n, int64_t d, int k, int sk) {
  if (n < 1 || d < 1 || k < 1 || k > 256) return 0;
  const int64_t dpad = cdiv(d, sk) * sk;
  const int kp = (int)cdiv(k, 16) * 16;
  return mean_off(dpad, kp) + align_up((size_t)dpad * sizeof(double), 256);
}

namespace {  // one copy per translation unit
// mean -> a copy padded with zeros to dpad entries
__global__ __launch_bounds__(256) void pad_mean_kernel(const double* __restrict__ mean, int64_t d,
                                                       int64_t dpad, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < dpad) out[i] = i < d ? mean[i] : 0.0;
}
}  // namespace

// The call of one source: `what` names the entry point in the messages, check_shape() is its
// rules for n, d and ldx (0, or the failure's code).
template <class Src, class Check>
int launch(const char* what, const typename Src::Elem* X, int64_t n, int64_t d, int64_t ldx,
           const double* mean, const float* W, int k, int64_t ldw, float* Y, int64_t ldy,
           float* resid, float* energy, void* ws, size_t ws_bytes, hipStream_t st,
           Check check_shape, bool w_rowmajor = false) {
  constexpr int SK = kSuper<Src>;
  DEIG_REQUIRE(k >= 1 && k <= 256, "%s: k=%d must be in 1..256", what, k);
  if (int rc = check_shape()) return rc;
  DEIG_REQUIRE(ldw >= (w_rowmajor ? (int64_t)k : d), "%s: ldw must be >= d", what);
  DEIG_REQUIRE(Y || resid || energy, "%s: need at least one output (Y, resid, energy)", what);
  DEIG_REQUIRE(!Y || ldy >= k, "%s: ldy must be >= k", what);
  DEIG_REQUIRE(X && reinterpret_cast<uintptr_t>(X) % Src::kXAlign == 0 && W,
               "%s: X (%d-byte aligned) and W must not be NULL", what, Src::kXAlign);
  DEIG_REQUIRE(reinterpret_cast<uintptr_t>(mean) % 8 == 0, "%s: mean must be 8-byte aligned", what);
  const size_t need = workspace_bytes(n, d, k, SK);
  if (!ws || ws_bytes < need)
    return fail(DEIG_EWORKSPACE, "%s: workspace %zu bytes < required %zu", what, ws_bytes, need);
  const int kp = (int)cdiv(k, 16) * 16;
  const int64_t dpad = cdiv(d, SK) * SK;
  float* Wr = static_cast<float*>(ws);
  if (int rc = pack_w_launch(W, ldw, d, k, kp, Wr, st, w_rowmajor)) return rc;
  if (dpad > d)
    DEIG_HIP_CHECK(hipMemsetAsync(Wr + d * kp, 0, sizeof(float) * (size_t)(dpad - d) * kp, st));
  double* mpad = nullptr;
  if (mean) {
    mpad = reinterpret_cast<double*>(static_cast<char*>(ws) + mean_off(dpad, kp));
    hipLaunchKernelGGL(pad_mean_kernel, dim3((unsigned)cdiv(dpad, 256)), dim3(256), 0, st, mean, d,
                       dpad, mpad);
    DEIG_HIP_CHECK(hipGetLastError());
  }
  const dim3 grid((unsigned)cdiv(n, tile::kRows));
  const int rc = tile::dispatch_nb(kp / 16, [&](auto nb) {
    return tile::launch<pca_transform_packed_kernel<nb(), Src>>(
        grid, tile::shm_bytes(nb() * 16, kAStride), st, X, ldx, mpad, Wr, Y, ldy, resid, energy, n, d, k);
  });
  if (rc == tile::kNoSuchNb) return fail(DEIG_EINVAL, "%s: unsupported k = %d", what, k);
  return rc;
}

}  // namespace ptile
}  // namespace deig
