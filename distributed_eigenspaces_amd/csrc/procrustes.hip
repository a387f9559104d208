// Procrustes-aligned basis averaging and the residual-form subspace distance.
//
//   V = orth( sum_i w_i V_i Z_i ),  Z_i = argmin_{Z in O(k)} ||V_i Z - R||_F = U W^T
//   for G_i = V_i^T R = U diag(c) W^T                    (deig_procrustes_avg_f32)
//   ||sin Theta(A, B)|| from R = B - A (A^T B)           (deig_subspace_dist_f32)
//
// One pass over the gathered stack Wt = [V_1^T; ...; V_m^T] is
//   1. ref_rows_kernel   the reference basis (column-major d x k) as a row-major
//                        d x kp image, kp = ceil(k / 16) * 16, padding columns zero
//   2. skinny_launch     G = Wt R                 (mk x kp; rows i k .. i k + k - 1 = G_i)
//   3. small_svd_kernel  one workgroup per basis: Z_i from a one-sided Jacobi SVD of
//                        G_i held in LDS, written as w_i Z_i into the stack Zs (mk x kp)
//   4. skinny_launch     Vbar = Wt^T Zs           (d x kp)
//   5. Loewdin, twice:   C = Vbar^T Vbar (skinny_launch), M = C^(-1/2) (small_svd_kernel,
//                        one workgroup), Vbar <- Vbar M (apply_kernel); the second
//                        apply writes the column-major result.
// The subspace distance runs 1, 2 (with A in the place of Wt), apply_kernel for the
// residual R = B - A G, C = R^T R and small_svd_kernel for lambda_max(C).
//
// No workgroup waits for another one anywhere here: every kernel is a plain grid of
// independent blocks, so there is no co-residency requirement.  All sums run in a
// fixed order (no atomics on data), so repeated calls are bit-identical.
#include <math.h>

#include <algorithm>
#include <cmath>

#include "deig_internal.hpp"

namespace deig {
namespace {

constexpr int kMaxK = 128;       // widest basis (2 x 128 x 132 floats of LDS)
constexpr int kMaxJSweeps = 30;  // the Jacobi loop always ends
constexpr float kJRel = 2e-7f;   // rotate while |g_p . g_q| > kJRel ||g_p|| ||g_q|| (rr_small_batch_launch's jrel)
constexpr float kDropRel = 1e-5f;     // polar: singular values below this * c_max give no term
constexpr float kDropRelInv = 1e-6f;  // inverse square root: the same guard (C = Vbar^T Vbar)

constexpr int kModePolar = 0;    // Z = sum_j u_j w_j^T
constexpr int kModeInvSqrt = 1;  // M = sum_j c_j^(-1/2) u_j w_j^T  (symmetric PSD input)
constexpr int kModeNorms = 2;    // out[0] = sqrt(trace), out[1] = sqrt(c_max)

inline int pad16(int k) { return (k + 15) / 16 * 16; }
__host__ __device__ inline int pad4(int k) { return (k + 3) / 4 * 4; }
__host__ __device__ inline int lds_stride(int k) { return pad4(k) + 4; }

size_t small_svd_shm(int k) {
  return ((size_t)2 * k * lds_stride(k) + 2 * kMaxK + 4) * sizeof(float);
}
int small_svd_threads(int k) {
  const int pairs = (k + 1) / 2;
  return std::max(64, (16 * pairs + 63) / 64 * 64);
}

// ---------------------------------------------------------------- weights
// The m weights are host values; they reach the device through kernel arguments, a
// chunk per launch (asynchronous, no staging copy, the caller's array is free on return).
constexpr int kWChunk = 512;
struct WeightChunk {
  float w[kWChunk];
};

__global__ __launch_bounds__(256) void set_weights_kernel(float* __restrict__ wdev, int base, int n,
                                                          const WeightChunk c) {
  for (int t = threadIdx.x; t < n; t += 256) wdev[base + t] = c.w[t];
}

__global__ __launch_bounds__(256) void fill_kernel(float* __restrict__ p, int n, float v) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < n) p[t] = v;
}

// ---------------------------------------------------------------- reference image
// dst (d x kp row-major) = src (d x k column-major, column stride ld), padding zero.
__global__ __launch_bounds__(256) void ref_rows_kernel(const float* __restrict__ src, int64_t ld,
                                                       int64_t d, int k, int kp,
                                                       float* __restrict__ dst) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * 32;
  const int j0 = blockIdx.y * 32;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int jj = ty + 8 * u;
    const int j = j0 + jj;
    const int64_t r = r0 + tx;
    tile[jj][tx] = (j < k && r < d) ? src[(int64_t)j * ld + r] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int rr = ty + 8 * u;
    const int64_t r = r0 + rr;
    const int j = j0 + tx;
    if (r < d && j < kp) dst[r * kp + j] = tile[tx][rr];
  }
}

// ---------------------------------------------------------------- small SVD
// Sum over the 16 lanes of a DPP row (lanes 16 g .. 16 g + 15 of the wave) by row
// rotations of 8, 4, 2, 1: no LDS traffic, and every lane of the row ends with the same
// bits (after each step the partial sums are periodic with the step's distance).
template <int N>
__device__ __forceinline__ float row_ror(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 | N, 0xF, 0xF, false));
}
__device__ __forceinline__ float row_sum16(float v) {
  v += row_ror<8>(v);
  v += row_ror<4>(v);
  v += row_ror<2>(v);
  v += row_ror<1>(v);
  return v;
}

// One workgroup per k x k matrix G (row-major, row stride ldg, matrix i at
// G + i * gstride).  One-sided (Hestenes) Jacobi: right rotations W make the columns
// g_j of G W orthogonal, G = U diag(c) W^T with g_j = c_j u_j.  LDS holds the columns
// of G W and of W as contiguous rows (A[j][:] = g_j, Wr[j][:] = w_j, row stride
// pad4(k) + 4 floats), so a rotation of the pair (p, q) touches four rows.  A group of
// 16 lanes owns one pair of a step (each lane 16-byte chunks of the rows, read once and
// kept in registers from the dot products to the rotation); the ceil(k / 2) pairs of a
// round-robin step are disjoint, and one barrier separates the steps.
struct SmallSvdArgs {
  const float* G;
  int64_t gstride;
  int ldg;
  int k, kp;
  int mode;
  const float* wts;  // polar: weight of matrix i (device), NULL = 1
  float* Zw;         // polar / invsqrt: (k rows) x kp row-major per matrix, weight folded in,
                     // columns k .. kp-1 written as zero; matrix i at Zw + i * k * kp
  float* Zout;       // polar: k x k row-major per matrix, unweighted (may be NULL)
  float* cos_out;    // polar: k singular values per matrix, descending (may be NULL)
  float* norms;      // kModeNorms: 2 floats
};

__global__ __launch_bounds__(1024) void small_svd_kernel(const SmallSvdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int k = a.k, S = lds_stride(k), K4 = pad4(k);
  float* A = sm;                       // [k][S]
  float* Wr = sm + (size_t)k * S;      // [k][S]
  float* cn = sm + (size_t)2 * k * S;  // [kMaxK] singular values
  float* sc = cn + kMaxK;              // [kMaxK] per-column scale of the output sum
  int* flag = reinterpret_cast<int*>(sc + kMaxK);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int mat = blockIdx.x;
  const float* G = a.G + (int64_t)mat * a.gstride;

  for (int idx = tid; idx < k * S; idx += nt) {
    const int j = idx / S, e = idx - j * S;
    A[idx] = 0.f;
    Wr[idx] = (e == j) ? 1.f : 0.f;
  }
  if (tid == 0) flag[0] = flag[1] = 0;
  __syncthreads();
  for (int idx = tid; idx < k * k; idx += nt) {
    const int r = idx / k, j = idx - r * k;
    A[j * S + r] = G[(int64_t)r * a.ldg + j];
  }
  __syncthreads();

  const int grp = tid >> 4, gl = tid & 15;
  const int nb = K4 / 4;             // 4 x 4 register blocks per side
  const bool has_item = tid < nb * nb;  // at most one block per thread (small_svd_threads)
  const int rb = has_item ? tid / nb : 0, cb = has_item ? tid - rb * nb : 0;
  const int kp = a.kp;
  float* Zw = a.Zw ? a.Zw + (int64_t)mat * k * kp : nullptr;

  // column norms of A into cn (16 lanes per column)
  auto col_norms = [&]() {
    for (int j = grp; j < k; j += nt >> 4) {
      float s = 0.f;
      for (int e = gl; e < K4; e += 16) s = fmaf(A[j * S + e], A[j * S + e], s);
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o);
      if (gl == 0) cn[j] = sqrtf(s);
    }
    __syncthreads();
  };
  // acc[i][e] = sum_{j < k} X[j][4 rb + i] Y[j][4 cb + e]   (X^T Y, one block per thread)
  auto block_tn = [&](const float* X, const float* Y, f32x4* acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(X + j * S + 4 * rb);
      const f32x4 yv = *reinterpret_cast<const f32x4*>(Y + j * S + 4 * cb);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] += xv[i] * yv;
    }
  };
  // acc[i][e] = sum_c X[4 rb + i][c] Y[4 cb + e][c]   (X Y^T; rows clamped to k - 1, the
  // caller discards those; X rows in LDS, Y rows of stride ldy in LDS or global memory)
  auto block_nt = [&](const float* X, const float* Y, int64_t ldy, f32x4* acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* xr[4];
    const float* yr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xr[i] = X + (size_t)min(4 * rb + i, k - 1) * S;
      yr[i] = Y + (int64_t)min(4 * cb + i, k - 1) * ldy;
    }
    for (int c = 0; c < K4; c += 4) {
      f32x4 xv[4], yv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xv[i] = *reinterpret_cast<const f32x4*>(xr[i] + c);
        yv[i] = *reinterpret_cast<const f32x4*>(yr[i] + c);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[i][e] += xv[i][0] * yv[e][0] + xv[i][1] * yv[e][1] + xv[i][2] * yv[e][2] +
                       xv[i][3] * yv[e][3];
    }
  };
  // rows 4 rb + i < k of a [k][S] LDS matrix <- acc (columns >= k as zero)
  auto store_block = [&](float* M, const f32x4* acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * rb + i;
      if (r >= k) continue;
      f32x4 v = acc[i];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * cb + e >= k) v[e] = 0.f;
      *reinterpret_cast<f32x4*>(M + r * S + 4 * cb) = v;
    }
  };
  // k x kp row-major output block (columns < k), weight folded in; optional k x k copy
  auto write_block = [&](const f32x4* acc, float wgt, float* Zo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * rb + i;
      if (r >= k) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * cb + e;
        if (c >= k) continue;
        Zw[(int64_t)r * kp + c] = wgt * acc[i][e];
        if (Zo) Zo[(int64_t)r * k + c] = acc[i][e];
      }
    }
  };
  // the padding columns k .. kp - 1 of the output, by all threads
  auto write_pad = [&]() {
    const int padc = kp - k;
    for (int idx = tid; idx < k * padc; idx += nt) {
      const int r = idx / padc, c = k + idx - r * padc;
      Zw[(int64_t)r * kp + c] = 0.f;
    }
  };

  // Inverse square root of a matrix already close to I (the second Loewdin pass, or a
  // stack that agrees with its reference): E = C - I, M = I - E/2 + 3/8 E^2 (next term
  // 5/16 E^3 <= 4e-10 for |E| <= 1e-3).  An eigendecomposition of such a C has an
  // arbitrary eigenbasis, and its rounding would cost ~k eps in M; the series does not.
  if (a.mode == kModeInvSqrt) {
    float dev = 0.f;
    for (int idx = tid; idx < k * k; idx += nt) {
      const int j = idx / k, r = idx - j * k;
      dev = fmaxf(dev, fabsf(A[j * S + r] - (r == j ? 1.f : 0.f)));
    }
    if (!(dev <= 1e-3f / (float)k)) flag[1] = 1;  // NaN counts as far (benign race: all write 1)
    __syncthreads();
    if (!flag[1]) {
      for (int idx = tid; idx < k * S; idx += nt) {
        const float e = A[idx] - Wr[idx];  // Wr = I
        A[idx] = e;
      }
      __syncthreads();
      for (int idx = tid; idx < k * S; idx += nt) Wr[idx] = A[idx];
      __syncthreads();
      if (has_item) {
        f32x4 acc[4];
        block_tn(A, Wr, acc);  // E^T E = E^2
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 ev = *reinterpret_cast<const f32x4*>(A + min(4 * rb + i, k - 1) * S + 4 * cb);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[i][e] = ((4 * rb + i == 4 * cb + e) ? 1.f : 0.f) - 0.5f * ev[e] + 0.375f * acc[i][e];
        }
        write_block(acc, 1.f, nullptr);
      }
      write_pad();
      return;
    }
  }

  // columns below tiny (< 3e-7 c_max, since c_max^2 >= ||G||_F^2 / k) are dropped from the
  // output anyway: they are left alone, so a rank-deficient G does not rotate its noise
  col_norms();
  float fro2 = 0.f;
  for (int j = 0; j < k; ++j) fro2 = fmaf(cn[j], cn[j], fro2);
  const float tiny2 = 9e-14f * fro2 / (float)k;
  __syncthreads();

  // round-robin tournament over n players (n even; player k is a bye when k is odd)
  const int n = (k + 1) & ~1;
  // one run of sweeps, until one passes without a rotation; returns the sweeps it took
  auto jacobi = [&](int max_sweeps) {
    int sweep = 0;
    while (sweep < max_sweeps) {
      ++sweep;
      for (int s = 0; s < n - 1; ++s) {
        int p = 0, q = 0;
        bool live = grp < n / 2;
        if (live) {
          const int x = (grp == 0) ? n - 1 : (s + grp) % (n - 1);
          const int y = (grp == 0) ? s : (s + n - 1 - grp) % (n - 1);
          p = x < y ? x : y;
          q = x < y ? y : x;
          if (q >= k) {
            live = false;
            p = q = 0;
          }
        }
        // the lane's part of both columns: 16-byte chunks gl and gl + 16, kept in registers
        // from the dot products to the rotation
        float* ap = A + p * S;
        float* aq = A + q * S;
        f32x4 xa[2], ya[2];
        float aa = 0.f, bb = 0.f, cc = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int ch = gl + 16 * u;
          xa[u] = ya[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (ch < nb) {
            xa[u] = *reinterpret_cast<const f32x4*>(ap + 4 * ch);
            ya[u] = *reinterpret_cast<const f32x4*>(aq + 4 * ch);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            aa = fmaf(xa[u][e], xa[u][e], aa);
            bb = fmaf(ya[u][e], ya[u][e], bb);
            cc = fmaf(xa[u][e], ya[u][e], cc);
          }
        }
        aa = row_sum16(aa);  // all 16 lanes of the group end with the same bits
        bb = row_sum16(bb);
        cc = row_sum16(cc);
        if (live && fabsf(cc) > kJRel * (sqrtf(aa) * sqrtf(bb)) && fminf(aa, bb) > tiny2) {
          const float zeta = (bb - aa) / (2.f * cc);
          const float t = copysignf(1.f, zeta) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
          const float cs = 1.f / sqrtf(1.f + t * t), sn = cs * t;
          float* wp = Wr + p * S;
          float* wq = Wr + q * S;
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int ch = gl + 16 * u;
            if (ch < nb) {
              *reinterpret_cast<f32x4*>(ap + 4 * ch) = cs * xa[u] - sn * ya[u];
              *reinterpret_cast<f32x4*>(aq + 4 * ch) = sn * xa[u] + cs * ya[u];
              const f32x4 wu = *reinterpret_cast<const f32x4*>(wp + 4 * ch);
              const f32x4 wv = *reinterpret_cast<const f32x4*>(wq + 4 * ch);
              *reinterpret_cast<f32x4*>(wp + 4 * ch) = cs * wu - sn * wv;
              *reinterpret_cast<f32x4*>(wq + 4 * ch) = sn * wu + cs * wv;
            }
          }
          if (gl == 0) flag[0] = 1;
        }
        __syncthreads();
      }
      const int rotated = flag[0];
      __syncthreads();
      if (tid == 0) flag[0] = 0;
      __syncthreads();
      if (!rotated) break;
    }
    return sweep;
  };
  // Rounding piles up with the rotations a column has seen (~sqrt(#rotations) eps, 1e-4 in
  // ||Z||_F after ten sweeps at k = 128).  After a long run the right factor is made
  // orthogonal again by one Newton-Schulz step, W <- W (3 I - W^T W) / 2 (it is within
  // ~1e-5 of orthogonal, so one step reaches rounding), the columns G W are formed afresh
  // from G, and the sweeps resume from there - a short run, since the columns are
  // orthogonal to ~1e-5 already.
  auto fresh_start = [&]() {
    f32x4 acc[4];
    if (has_item) {
      block_nt(Wr, Wr, S, acc);  // T = Wr Wr^T = W^T W
      store_block(A, acc);
    }
    __syncthreads();
    if (has_item) {
      block_tn(A, Wr, acc);  // T^T Wr
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(Wr + min(4 * rb + i, k - 1) * S + 4 * cb);
        acc[i] = 1.5f * w - 0.5f * acc[i];
      }
    }
    __syncthreads();
    if (has_item) store_block(Wr, acc);
    __syncthreads();
    if (has_item) {
      block_nt(Wr, G, a.ldg, acc);  // A[j][r] = sum_c Wr[j][c] G[r][c] = (G W)[r][j]
      store_block(A, acc);
    }
    __syncthreads();
  };
  if (k > 1) {
    // a short run has piled up nothing; after a long one, two sweeps from the fresh start
    // (the first takes the ~1e-5 that is left to ~1e-10, below what fp32 dot products see)
    if (jacobi(kMaxJSweeps) > 3) {
      fresh_start();
      jacobi(2);
    }
  }

  // singular values c_j = ||g_j||
  col_norms();
  float cmax = 0.f;
  for (int j = 0; j < k; ++j) cmax = fmaxf(cmax, cn[j]);

  if (a.mode == kModeNorms) {
    if (tid == 0) {
      double tr = 0.0;
      for (int j = 0; j < k; ++j) tr += (double)G[(int64_t)j * a.ldg + j];
      a.norms[0] = (float)sqrt(tr > 0.0 ? tr : 0.0);
      a.norms[1] = sqrtf(cmax);
    }
    return;
  }

  if (a.cos_out) {  // descending, by rank (ties by index)
    for (int j = tid; j < k; j += nt) {
      const float c = cn[j];
      int rank = 0;
      for (int i = 0; i < k; ++i) rank += (cn[i] > c || (cn[i] == c && i < j)) ? 1 : 0;
      a.cos_out[(int64_t)mat * k + rank] = c;
    }
  }
  for (int j = tid; j < k; j += nt) {
    const float c = cn[j];
    float s;
    if (a.mode == kModePolar)
      s = (c > kDropRel * cmax) ? 1.f / c : 0.f;
    else
      s = (c > kDropRelInv * cmax) ? 1.f / (c * sqrtf(c)) : 0.f;
    sc[j] = s;
  }
  __syncthreads();
  for (int idx = tid; idx < k * S; idx += nt) A[idx] *= sc[idx / S];
  __syncthreads();

  // Z[r][c] = sum_j A[j][r] Wr[j][c], 4 x 4 outputs per thread
  if (has_item) {
    f32x4 acc[4];
    block_tn(A, Wr, acc);
    write_block(acc, a.wts ? a.wts[mat] : 1.f, a.Zout ? a.Zout + (int64_t)mat * k * k : nullptr);
  }
  write_pad();
}

int small_svd_launch(const SmallSvdArgs& a, int nmat, hipStream_t st) {
  static const hipError_t attr =
      hipFuncSetAttribute((const void*)small_svd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)small_svd_shm(kMaxK));
  DEIG_HIP_CHECK(attr);
  hipLaunchKernelGGL(small_svd_kernel, dim3((unsigned)nmat), dim3(small_svd_threads(a.k)),
                     small_svd_shm(a.k), st, a);
  DEIG_HIP_CHECK(hipGetLastError());
  return DEIG_OK;
}

// ---------------------------------------------------------------- apply / residual
// out[r][j] = beta * B[r][j] + alpha * sum_{a < k} A(r, a) G[a][j],  r < d, j < ncols
//   A(r, a) = A[r * a_rs + a * a_cs]   (row-major image: a_cs = 1; column-major basis: a_rs = 1)
//   G: k x ncols row-major (ldg);  B: d x ncols row-major (ldb), NULL with beta = 0
//   out(r, j) = out[r * o_rs + j * o_cs]; only the columns j < ocols are stored.
// A block takes 32 rows; the A tile and the output tile pass through LDS so that both
// layouts are read and written along their unit stride.
constexpr int kApplyRows = 32;

struct ApplyArgs {
  const float* A;
  int64_t a_rs, a_cs;
  const float* G;
  int ldg;
  const float* B;
  int64_t ldb;
  float* out;
  int64_t o_rs, o_cs;
  int64_t d;
  int k, ncols, ocols;
  float alpha, beta;
};

__global__ __launch_bounds__(256) void apply_kernel(const ApplyArgs a) {
  __shared__ float As[kApplyRows][kMaxK + 1];
  __shared__ float Os[kApplyRows][kMaxK + 1];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kApplyRows;
  const int k = a.k, nc = a.ncols;
  for (int idx = tid; idx < kApplyRows * k; idx += 256) {
    int rr, c;
    if (a.a_cs == 1) {
      rr = idx / k;
      c = idx - rr * k;
    } else {
      c = idx / kApplyRows;
      rr = idx - c * kApplyRows;
    }
    const int64_t r = r0 + rr;
    As[rr][c] = r < a.d ? a.A[r * a.a_rs + c * a.a_cs] : 0.f;
  }
  __syncthreads();
  for (int item = tid; item < (kApplyRows / 8) * nc; item += 256) {
    const int rg = item / nc, j = item - rg * nc;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int c = 0; c < k; ++c) {
      const float g = a.G[(int64_t)c * a.ldg + j];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(As[8 * rg + e][c], g, acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int rr = 8 * rg + e;
      const int64_t r = r0 + rr;
      float v = a.alpha * acc[e];
      if (a.B && r < a.d) v += a.beta * a.B[r * a.ldb + j];
      Os[rr][j] = v;
    }
  }
  __syncthreads();
  const int oc = a.ocols;
  for (int idx = tid; idx < kApplyRows * oc; idx += 256) {
    int rr, j;
    if (a.o_cs == 1) {
      rr = idx / oc;
      j = idx - rr * oc;
    } else {
      j = idx / kApplyRows;
      rr = idx - j * kApplyRows;
    }
    const int64_t r = r0 + rr;
    if (r < a.d) a.out[r * a.o_rs + j * a.o_cs] = Os[rr][j];
  }
}

int apply_launch(const ApplyArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(apply_kernel, dim3((unsigned)cdiv(a.d, kApplyRows)), dim3(256), 0, st, a);
  DEIG_HIP_CHECK(hipGetLastError());
  return DEIG_OK;
}

int ref_rows_launch(const float* src, int64_t ld, int64_t d, int k, int kp, float* dst,
                    hipStream_t st) {
  hipLaunchKernelGGL(ref_rows_kernel, dim3((unsigned)cdiv(d, 32), (unsigned)cdiv(kp, 32)),
                     dim3(256), 0, st, src, ld, d, k, kp, dst);
  DEIG_HIP_CHECK(hipGetLastError());
  return DEIG_OK;
}

size_t max3(size_t a, size_t b, size_t c) { return std::max(a, std::max(b, c)); }

struct ProcWs {
  float *wdev, *R, *G, *Zs, *Vbar, *Vtmp, *C, *M, *slab;
  size_t slab_bytes, total;
};

ProcWs carve_proc(void* ws, size_t cap, int64_t d, int64_t mk, int k) {
  const int kp = pad16(k);
  Carve c(ws, cap);
  ProcWs w{};
  w.wdev = c.take<float>((size_t)(mk / k));
  w.R = c.take<float>((size_t)d * kp);
  w.G = c.take<float>((size_t)mk * kp);
  w.Zs = c.take<float>((size_t)mk * kp);
  w.Vbar = c.take<float>((size_t)d * kp);
  w.Vtmp = c.take<float>((size_t)d * kp);
  w.C = c.take<float>((size_t)kp * kp);
  w.M = c.take<float>((size_t)kp * kp);
  w.slab_bytes = max3(skinny_workspace_bytes(mk, kp, d), skinny_workspace_bytes(d, kp, mk),
                      skinny_workspace_bytes(kp, kp, d));
  w.slab = c.take<float>(w.slab_bytes / sizeof(float));
  w.total = c.off;
  return w;
}

struct DistWs {
  float *Brow, *G, *R, *C, *slab;
  size_t slab_bytes, total;
};

DistWs carve_dist(void* ws, size_t cap, int64_t d, int k) {
  const int kp = pad16(k);
  Carve c(ws, cap);
  DistWs w{};
  w.Brow = c.take<float>((size_t)d * kp);
  w.G = c.take<float>((size_t)kp * kp);
  w.R = c.take<float>((size_t)d * kp);
  w.C = c.take<float>((size_t)kp * kp);
  w.slab_bytes = std::max(skinny_workspace_bytes(k, kp, d), skinny_workspace_bytes(kp, kp, d));
  w.slab = c.take<float>(w.slab_bytes / sizeof(float));
  w.total = c.off;
  return w;
}

// Vin (d x kp row-major) -> Vin (Vin^T Vin)^(-1/2), written to out with strides (o_rs, o_cs).
int loewdin_step(const float* Vin, int64_t d, int k, int kp, const ProcWs& w, float* out,
                 int64_t o_rs, int64_t o_cs, int ocols, hipStream_t st) {
  int rc = skinny_launch(true, Vin, kp, Vin, kp, w.C, kp, kp, kp, d, 1.f, 0.f, w.slab,
                         w.slab_bytes, st);
  if (rc) return rc;
  SmallSvdArgs s{};
  s.G = w.C;
  s.gstride = 0;
  s.ldg = kp;
  s.k = k;
  s.kp = kp;
  s.mode = kModeInvSqrt;
  s.Zw = w.M;
  rc = small_svd_launch(s, 1, st);
  if (rc) return rc;
  ApplyArgs ap{};
  ap.A = Vin;
  ap.a_rs = kp;
  ap.a_cs = 1;
  ap.G = w.M;
  ap.ldg = kp;
  ap.out = out;
  ap.o_rs = o_rs;
  ap.o_cs = o_cs;
  ap.d = d;
  ap.k = k;
  ap.ncols = kp;
  ap.ocols = ocols;
  ap.alpha = 1.f;
  ap.beta = 0.f;
  return apply_launch(ap, st);
}

}  // namespace

size_t procrustes_workspace_bytes(int64_t d, int64_t mk, int k) {
  if (d < 1 || k < 1 || k > kMaxK || mk < k || mk % k != 0) return 0;
  return carve_proc(nullptr, 0, d, mk, k).total;
}

int procrustes_launch(const float* Wt, int64_t d, int64_t mk, int64_t ldw, int k, const float* Vref,
                      int64_t ldref, const float* weights, int iters, float* V, int64_t ldv,
                      float* Z, float* cosines, void* ws, size_t ws_bytes, hipStream_t st) {
  DEIG_REQUIRE(k >= 1 && k <= kMaxK, "procrustes: k=%d must be 1..%d (above, use deig_projavg_topk)",
               k, kMaxK);
  DEIG_REQUIRE(d >= 1 && k <= d, "procrustes: k=%d must not exceed d=%lld", k, (long long)d);
  DEIG_REQUIRE(mk >= k && mk % k == 0, "procrustes: mk=%lld must be a positive multiple of k=%d",
               (long long)mk, k);
  DEIG_REQUIRE(iters >= 1 && iters <= 8, "procrustes: iters=%d must be 1..8", iters);
  const int64_t m = mk / k;
  DEIG_REQUIRE(m <= (int64_t)1 << 20, "procrustes: %lld bases", (long long)m);
  DEIG_REQUIRE(d % 4 == 0 && ldw % 4 == 0 && ldw >= d, "procrustes: d %% 4, ldw %% 4 and ldw >= d required");
  DEIG_REQUIRE(Wt && aligned16(Wt), "procrustes: Wt must be a 16-byte aligned device pointer");
  DEIG_REQUIRE(V && ldv >= d, "procrustes: V must be given with ldv >= d");
  DEIG_REQUIRE(!Vref || ldref >= d, "procrustes: ldref >= d required");
  double wsum = 0.0;
  if (weights) {
    for (int64_t i = 0; i < m; ++i) {
      DEIG_REQUIRE(weights[i] >= 0.f && std::isfinite(weights[i]),
                   "procrustes: weight %lld is negative or not finite", (long long)i);
      wsum += weights[i];
    }
    DEIG_REQUIRE(wsum > 0.0, "procrustes: the weights are all zero");
  }
  const ProcWs w = carve_proc(ws, ws_bytes, d, mk, k);
  if (!ws || w.total > ws_bytes)
    return fail(DEIG_EWORKSPACE, "procrustes: workspace %zu bytes < required %zu", ws_bytes, w.total);
  const int kp = pad16(k);

  if (weights) {
    for (int64_t base = 0; base < m; base += kWChunk) {
      WeightChunk c;
      const int n = (int)std::min<int64_t>(kWChunk, m - base);
      for (int t = 0; t < n; ++t) c.w[t] = (float)(weights[base + t] / wsum);
      hipLaunchKernelGGL(set_weights_kernel, dim3(1), dim3(256), 0, st, w.wdev, (int)base, n, c);
    }
  } else {
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, st, w.wdev, (int)m,
                       (float)(1.0 / (double)m));
  }
  DEIG_HIP_CHECK(hipGetLastError());

  for (int it = 0; it < iters; ++it) {
    const bool last = it + 1 == iters;
    // reference: pass 1 Vref (or V_1, the first k rows of Wt); later passes the previous V
    const float* ref = it ? V : (Vref ? Vref : Wt);
    const int64_t ldr = it ? ldv : (Vref ? ldref : ldw);
    int rc = ref_rows_launch(ref, ldr, d, k, kp, w.R, st);
    if (rc) return rc;
    rc = skinny_launch(false, Wt, ldw, w.R, kp, w.G, kp, mk, kp, d, 1.f, 0.f, w.slab, w.slab_bytes, st);
    if (rc) return rc;
    SmallSvdArgs s{};
    s.G = w.G;
    s.gstride = (int64_t)k * kp;
    s.ldg = kp;
    s.k = k;
    s.kp = kp;
    s.mode = kModePolar;
    s.wts = w.wdev;
    s.Zw = w.Zs;
    s.Zout = last ? Z : nullptr;
    s.cos_out = last ? cosines : nullptr;
    rc = small_svd_launch(s, (int)m, st);
    if (rc) return rc;
    rc = skinny_launch(true, Wt, ldw, w.Zs, kp, w.Vbar, kp, d, kp, mk, 1.f, 0.f, w.slab, w.slab_bytes, st);
    if (rc) return rc;
    rc = loewdin_step(w.Vbar, d, k, kp, w, w.Vtmp, kp, 1, kp, st);
    if (rc) return rc;
    rc = loewdin_step(w.Vtmp, d, k, kp, w, V, 1, ldv, k, st);
    if (rc) return rc;
  }
  return DEIG_OK;
}

size_t subspace_dist_workspace_bytes(int64_t d, int k) {
  if (d < 1 || k < 1 || k > kMaxK) return 0;
  return carve_dist(nullptr, 0, d, k).total;
}

int subspace_dist_launch(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t d, int k,
                         float* out, void* ws, size_t ws_bytes, hipStream_t st) {
  DEIG_REQUIRE(k >= 1 && k <= kMaxK, "subspace_dist: k=%d must be 1..%d", k, kMaxK);
  DEIG_REQUIRE(d >= 1 && k <= d, "subspace_dist: k=%d must not exceed d=%lld", k, (long long)d);
  DEIG_REQUIRE(d % 4 == 0 && lda % 4 == 0 && lda >= d && ldb >= d,
               "subspace_dist: d %% 4, lda %% 4, lda >= d and ldb >= d required");
  DEIG_REQUIRE(A && B && out && aligned16(A), "subspace_dist: A (16-byte aligned), B and out required");
  const DistWs w = carve_dist(ws, ws_bytes, d, k);
  if (!ws || w.total > ws_bytes)
    return fail(DEIG_EWORKSPACE, "subspace_dist: workspace %zu bytes < required %zu", ws_bytes, w.total);
  const int kp = pad16(k);
  int rc = ref_rows_launch(B, ldb, d, k, kp, w.Brow, st);
  if (rc) return rc;
  // G = A^T B: the column-major A is the row-major k x d image A^T
  rc = skinny_launch(false, A, lda, w.Brow, kp, w.G, kp, k, kp, d, 1.f, 0.f, w.slab, w.slab_bytes, st);
  if (rc) return rc;
  ApplyArgs ap{};
  ap.A = A;
  ap.a_rs = 1;
  ap.a_cs = lda;
  ap.G = w.G;
  ap.ldg = kp;
  ap.B = w.Brow;
  ap.ldb = kp;
  ap.out = w.R;
  ap.o_rs = kp;
  ap.o_cs = 1;
  ap.d = d;
  ap.k = k;
  ap.ncols = kp;
  ap.ocols = kp;
  ap.alpha = -1.f;
  ap.beta = 1.f;
  rc = apply_launch(ap, st);
  if (rc) return rc;
  rc = skinny_launch(true, w.R, kp, w.R, kp, w.C, kp, kp, kp, d, 1.f, 0.f, w.slab, w.slab_bytes, st);
  if (rc) return rc;
  SmallSvdArgs s{};
  s.G = w.C;
  s.gstride = 0;
  s.ldg = kp;
  s.k = k;
  s.kp = kp;
  s.mode = kModeNorms;
  s.norms = out;
  return small_svd_launch(s, 1, st);
}

}  // namespace deig
