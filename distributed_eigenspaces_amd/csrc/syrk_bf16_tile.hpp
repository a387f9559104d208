// What the two bf16 image products share beside the tile K loop (syrk_image_tile.hpp):
// the covariance S = alpha X^T X of bf16 samples (syrk_bf16.hip) and the sample-space Gram
// K = alpha Xc Xc^T (gram_nt.hip).  The loop's operation and stage size, the two-level
// summation rule, the slab layout and the kernel that reduces the slabs.
//
// Slabs: [K segment][lower tile][wave][MFMA block a, b][lane][4] floats, a tile's accumulators
// in fragment order (one 16-byte store per lane and MFMA block, fully coalesced).  Every slab
// entry that the reduce reads was written by the product kernel of the same call (a diagonal
// tile's upper wave block is neither written nor read).
//
// The kernel stands in an unnamed namespace: each translation unit that includes this header
// holds and launches its own copy.
#pragma once

#include "syrk_image_tile.hpp"

namespace deig {
namespace {

constexpr int KB = 32;              // inner elements per MFMA K-step
// Tuning constants; a measurement build overrides them (_build.build_library(defines=...)).
// 32-row stages with a 4-deep ring fit 3 workgroups per CU (166 VGPRs, 32 KiB LDS): 7 %
// faster at 2^20 x 3072, 2.6 % slower at 2^19 x 8192 than the values below (DESIGN Appendix A).
#ifndef DEIG_AB_BF16_STAGE_ROWS
#define DEIG_AB_BF16_STAGE_ROWS 64
#endif
#ifndef DEIG_AB_BF16_PF
#define DEIG_AB_BF16_PF 2
#endif
#ifndef DEIG_AB_BF16_WGS
#define DEIG_AB_BF16_WGS 2
#endif
constexpr int SB = DEIG_AB_BF16_STAGE_ROWS;  // inner elements per LDS stage (a multiple of KB)
constexpr int KS = SB / 32;                  // K-steps per stage
constexpr int WGS = DEIG_AB_BF16_WGS;        // workgroups per CU the kernels are built for
using namespace itile;  // TB, THR, img_off, tile_of, frag_row, frag_col
// The shared K loop's operation; stage st is the K-steps kb = KS st .. KS st + KS - 1.
struct Bf16Op {
  static constexpr int KS = SB / 32, PF = DEIG_AB_BF16_PF;  // PF: stages in the register ring (even)
  typedef bf16x8 Frag;
  typedef f32x4 Acc;
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
constexpr int kFlushRows = 16384;   // inner elements per K segment at most (syrk_split.hip flush_ktiles)
constexpr int kSegStages = kFlushRows / SB;
constexpr int kItemsTarget = 512;   // two workgroups on each of 256 CUs
constexpr int64_t kTileFloats = (int64_t)TB * TB;

// One workgroup per lower tile, one 64-row half of it at a time; slab entries are placed by
// the C/D map (frag_row, frag_col).  v = alpha (sum of the segments in order)
// (+ S[i][j], the lower entry, when accumulating) goes to LDS (row stride 129: both the row
// and the column walk are conflict-free), then to S[i][j] in rows of 128 contiguous floats
// and to S[j][i] in runs of 64: both triangles hold the same bits.
__global__ __launch_bounds__(THR) void bf16_reduce_kernel(const float* __restrict__ slabs, int T,
                                                          int nseg, float alpha, int beta,
                                                          float* __restrict__ S, int64_t lds,
                                                          int64_t d) {
  __shared__ float V[64][TB + 1];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  int ti, tj;
  tile_of(tile, ti, tj);
  const bool diag = ti == tj;
  const int64_t j0 = (int64_t)tj * TB;
  for (int h = 0; h < 2; ++h) {
    const int64_t i0 = (int64_t)ti * TB + 64 * h;
    for (int q = tid; q < 2048; q += THR) {
      const int wj = q >> 10, ab = (q >> 6) & 15, lane = q & 63;
      if (diag && h < wj) continue;  // not computed, and only mirrors
      const int64_t e = ((int64_t)((2 * h + wj) * 16 + ab) * 64 + lane) * 4;
      const float* p = slabs + (int64_t)tile * kTileFloats + e;
      f32x4 v = *reinterpret_cast<const f32x4*>(p);
      for (int sg = 1; sg < nseg; ++sg)
        v += *reinterpret_cast<const f32x4*>(p + (int64_t)sg * T * kTileFloats);
      const int jl = frag_col(wj, ab & 3, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int il = frag_row(0, ab >> 2, lane, r);  // (within the half: wi = h is in i0)
        const int64_t i = i0 + il, j = j0 + jl;
        float x = alpha * v[r];
        if (beta && i < d && j < d && j <= i) x += S[i * lds + j];
        V[il][jl] = x;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < 64 * TB; idx += THR) {
      const int il = idx >> 7, jl = idx & 127;
      const int64_t i = i0 + il, j = j0 + jl;
      if (i < d && j < d && j <= i) S[i * lds + j] = V[il][jl];
    }
    for (int idx = tid; idx < 64 * TB; idx += THR) {
      const int jl = idx >> 6, il = idx & 63;
      const int64_t i = i0 + il, j = j0 + jl;
      if (i < d && j < d && j < i) S[j * lds + i] = V[il][jl];
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace deig
