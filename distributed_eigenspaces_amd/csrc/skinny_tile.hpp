// The block tile shared by skinny_kernel (skinny.hip), pca_transform_kernel (pca.hip) and
// pca_transform_packed_kernel (pca_packed_tile.hpp: uint8 and bf16 samples), stated once: the
// layout and its reasons, the tile constants and LDS sizing, the B chunk store, the MFMA chunk
// product and the host-side dispatch and launch (all three kernels), and the transform
// epilogue (pca_transform_kernel calls it; the packed kernel carries its text, see there).
//
// Tile.  A block of kThreads = 4 waves owns kRows = 64 rows x N = 16 NB columns of the
// output; wave w owns rows 16 w .. 16 w + 15 as NB accumulator fragments of
// v_mfma_f32_16x16x4_f32.  The inner dimension advances in chunks of kChunk = 32 slots.  A
// chunk's two operands are loaded into registers, then written to LDS after the products
// of the chunk before it (two stage buffers), as k-major images:
//   A [slot][row], row stride chosen by the kernel: kAStridePadded (80) in the float
//     kernels, 64 with XOR-swizzled rows in the packed-sample kernel (a_swz,
//     pca_packed_tile.hpp);
//   B [slot][column], row stride bstride(N).
// LDS per block: shm_bytes(N, a_stride).
//
// Strides.  One MFMA step reads slot 4 s + (lane >> 4) at row or column (lane & 15): a
// ds_read_b32 serves its 64 lanes as two groups of 32, and each group holds two slots of
// 16 lanes.  With a row stride == 16 (mod 32) floats the second slot's 16 lanes fall on
// the other 16 banks, so a group touches 32 distinct banks: 80 for A, and N + 16 for B
// when N itself is a multiple of 32 (an odd multiple of 16 already is == 16 mod 32).
//
// C/D map of 16x16x4: lane l, register e of a fragment hold column (l & 15) and row
// 4 (l >> 4) + e of the wave's 16 x 16 block; fragment j is columns 16 j .. 16 j + 15.
//
// Accumulators.  The 16x16x4 MFMA has a 40-cycle dependent latency on a 32-cycle issue.
// With NB >= 2 the fragments of a wave interleave and hide it.  N = 16 has one fragment per
// wave, so the two PCA kernels alternate its K chain between KA = 2 accumulators that the
// epilogue adds; skinny_kernel runs KA = 1 at every N (its sums, and their bits, are those
// of one chain).
#pragma once

#include <type_traits>

#include "deig_internal.hpp"

namespace deig {
namespace tile {

constexpr int kRows = 64;                   // rows of a block tile
constexpr int kChunk = 32;                  // slots of the inner dimension per chunk
constexpr int kThreads = 256;               // 4 waves
constexpr int kAStridePadded = kRows + 16;  // 80 == 16 mod 32

__host__ __device__ constexpr int bstride(int N) { return (N % 32 == 0) ? N + 16 : N; }
constexpr size_t shm_bytes(int N, int a_stride) {
  return (size_t)(2 * kChunk * a_stride + 2 * kChunk * bstride(N)) * sizeof(float);
}
// float4s of a B chunk that one thread stages
__host__ __device__ constexpr int b_per_thread(int NB) {
  return (kChunk * NB * 16 / 4 + kThreads - 1) / kThreads;
}

// ---------------------------------------------------------------- B / W chunk staging
// A chunk of B: kChunk slots x N floats; float4 f = tid + kThreads u of it is slot f / (N/4),
// columns 4 (f % (N/4)) .. + 3, held in rb[u] from its load (each kernel's own: which row of
// B a slot holds is its rule) to this store into the stage buffer bs ([kChunk][bstride(N)]).
template <int NB>
__device__ __forceinline__ void store_b(float* bs, const f32x4 (&rb)[b_per_thread(NB)], int tid) {
  constexpr int N = NB * 16, NB4 = kChunk * N / 4, BST = bstride(N), BPT = b_per_thread(NB);
#pragma unroll
  for (int u = 0; u < BPT; ++u) {
    const int f = tid + kThreads * u;
    if (f < NB4) {
      const int slot = f / (N / 4), c4 = f % (N / 4);
      *reinterpret_cast<f32x4*>(bs + slot * BST + 4 * c4) = rb[u];
    }
  }
}

// ---------------------------------------------------------------- MFMA chunk product
// The wave's products of one staged chunk: step s multiplies slots 4 s .. 4 s + 3.
// With r = lane & 15 and kk = lane >> 4, read_a(s) is this lane's A value of step s (slot
// 4 s + kk, row 16 wave + r, in the kernel's own A layout); bs is the B stage buffer.
template <int NB, int KA, class ReadA>
__device__ __forceinline__ void mfma_chunk(f32x4 (&acc)[NB][KA], const float* bs, int r, int kk,
                                           const ReadA& read_a) {
  constexpr int BST = bstride(NB * 16);
  const float* b = bs + kk * BST + r;
#pragma unroll
  for (int s = 0; s < kChunk / 4; ++s) {
    const float a = read_a(s);
#pragma unroll
    for (int j = 0; j < NB; ++j)
      acc[j][s % KA] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[4 * s * BST + 16 * j],
                                                            acc[j][s % KA], 0, 0, 0);
  }
}

// ---------------------------------------------------------------- transform epilogue
// The end of both PCA transform kernels, after the last chunk's barrier.  en[u]: the sum of
// squares of the centred values this thread staged for rows (tid >> 3) + 32 u of the tile (8
// consecutive lanes per row: one fixed shuffle tree).  The row energies are exchanged through
// es, kRows floats ON the dead stage buffers: 256 B of their own would take the kernels from
// 4 to 3 workgroups per CU at N = 64 (buffers exactly a quarter of the 160 KB of LDS).  Then
// ||y_i||^2 from the accumulators (the NB fragments, then the 16 column lanes), resid, and Y
// straight to its destination with guarded scalar stores: any ldy >= k, any alignment, k < N.
// Y, resid, energy: each may be NULL.  r = lane & 15, kk = lane >> 4.
template <int NB, int KA>
__device__ __forceinline__ void transform_epilogue(
    const f32x4 (&acc)[NB][KA], const float (&en)[2], float* es, float* __restrict__ Y, int64_t ldy,
    float* __restrict__ resid, float* __restrict__ energy, int64_t m0, int64_t n, int k, int tid,
    int wave, int r, int kk) {
  const int mm = tid >> 3, kq = tid & 7;
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
// f(std::integral_constant<int, NB>{}) for nb = NB in 1 .. 16; kNoSuchNb for any other nb.
constexpr int kNoSuchNb = -0x7fffffff;
template <class F>
int dispatch_nb(int nb, F f) {
  switch (nb) {
#define DEIG_NB(x) case x: return f(std::integral_constant<int, x>{});
    DEIG_NB(1) DEIG_NB(2) DEIG_NB(3) DEIG_NB(4) DEIG_NB(5) DEIG_NB(6) DEIG_NB(7) DEIG_NB(8)
    DEIG_NB(9) DEIG_NB(10) DEIG_NB(11) DEIG_NB(12) DEIG_NB(13) DEIG_NB(14) DEIG_NB(15)
    DEIG_NB(16)
#undef DEIG_NB
  }
  return kNoSuchNb;
}

// One kernel instantiation on kThreads-thread blocks with shm bytes of dynamic LDS; the
// attribute is set once per instantiation (C++11 thread-safe static initialisation).
template <auto Kernel, class... Args>
int launch(dim3 grid, size_t shm, hipStream_t st, Args... args) {
  static const hipError_t attr = hipFuncSetAttribute(
      (const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  DEIG_HIP_CHECK(attr);
  hipLaunchKernelGGL(Kernel, grid, dim3(kThreads), shm, st, args...);
  DEIG_HIP_CHECK(hipGetLastError());
  return DEIG_OK;
}

}  // namespace tile
}  // namespace deig
