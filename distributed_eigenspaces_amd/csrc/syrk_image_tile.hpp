// The 128 x 128 tile K loop shared by u8_syrk_kernel (syrk_u8.hip) and bf16_syrk_kernel
// (syrk_bf16.hip), stated once: the operand image and its addressing, the lower-tile index,
// the decode of a workgroup's place in its tile, the C/D map of the accumulators, and the
// loop itself.  The kernels keep what is theirs: item -> (tile, K segment, plane), the
// accumulators' zeroing, the epilogues and the launch bounds.
//
// Image.  A prep kernel relays the samples into MFMA operand order:
//   [kb = K-step][g = row group of the K-step, 4 of them][feature, padded to fpad][16 B],
// the 16 bytes being what lane (g, feature) feeds to one MFMA: 16 rows of int8
// (v_mfma_i32_16x16x64_i8, 64 rows per K-step) or 8 rows of bf16 (v_mfma_f32_16x16x32_bf16,
// 32 rows per K-step).  Several planes (uint8 gray) are whole images one after the other: a
// plane is an offset on the base pointer.
//
// Tile.  A workgroup of THR = 4 waves owns one lower TB x TB tile (ti, tj), tj <= ti, over
// a range of stages; a stage is Op::KS K-steps.  Wave (wi, wj) owns rows 64 wi.. and columns
// 64 wj.. of the tile as 4 x 4 MFMA blocks.  The upper wave block of a diagonal tile is a
// mirror: that wave stages with the others and computes nothing (active == false).
//
// LDS.  2 stages x (A panel, B panel), a panel = 4 KS row groups x 128 features x 16 B (8 KiB
// at KS = 1, 16 KiB at KS = 2), the same bytes as the image's [kb][g][f0 .. f0 + 127] runs.
// Lane l reads the fragment of feature 16 a + (l & 15), row group l >> 4 of a K-step: within
// a ds_read_b128 lane group the 16 addresses cover 64 distinct banks.
//
// C/D map (gfx950, the same for both MFMAs): lane l, register r of block (a, b) of wave
// (wi, wj) is row frag_row = 64 wi + 16 a + 4 (l >> 4) + r and column frag_col = 64 wj + 16 b
// + (l & 15) of the tile.
//
// K loop.  The LDS double buffer is fed from a PF-deep register ring - the loads of stage
// kk + PF are issued while kk's MFMAs run, so each load has PF - 1 stages to land (one
// stage ahead, a c1 worker shard of uint8 samples took 149 us: every step waited out a
// global load latency).  Loads are unpredicated (clamped to the last stage) so that the
// compiler's counted waits keep the ring in flight, and unconditional: a diagonal tile loads
// its panel twice - a branch around the B loads would make those waits conservative.  PF is
// even: LDS buffer = ring slot & 1.  The summation order is fixed: stages in order, the
// K-steps of a stage in order, and per K-step the blocks a-outer, b-inner.
#pragma once

#include "bf16_split.hpp"

namespace deig {
namespace itile {

constexpr int TB = 128;   // output tile edge (features)
constexpr int THR = 256;  // 4 waves, 2 x 2 wave tiles of 64 x 64

__host__ __device__ inline int64_t img_off(int64_t kb, int g, int64_t f, int64_t fpad) {
  return ((kb * 4 + g) * fpad + f) * 16;
}

// Lower tile t (row-major over the triangle) -> (ti, tj), tj <= ti.
__device__ __forceinline__ void tile_of(int t, int& ti, int& tj) {
  int i = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while (i * (i + 1) / 2 > t) --i;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  ti = i;
  tj = t - i * (i + 1) / 2;
}

// A thread's place in the tile (ti, tj) of its workgroup.
struct Item {
  int tid, lane, wave, wi, wj;
  bool diag, active;
  int64_t i0, j0;  // the tile's first row and column (features)
};
__device__ __forceinline__ Item item_of(int ti, int tj) {
  Item it;
  it.tid = threadIdx.x;
  it.lane = it.tid & 63;
  it.wave = it.tid >> 6;
  it.wi = it.wave >> 1;
  it.wj = it.wave & 1;
  it.diag = ti == tj;
  it.active = !(it.diag && it.wi < it.wj);
  it.i0 = (int64_t)ti * TB;
  it.j0 = (int64_t)tj * TB;
  return it;
}

__device__ __forceinline__ int frag_row(int wi, int a, int lane, int r) {
  return 64 * wi + 16 * a + 4 * (lane >> 4) + r;
}
__device__ __forceinline__ int frag_col(int wj, int b, int lane) { return 64 * wj + 16 * b + (lane & 15); }

// Op: KS (K-steps per stage), PF (stages in the register ring, even), Frag, Acc and
// static Acc mfma(Frag, Frag, Acc).
template <class Op>
constexpr int lds_bytes() { return 2 * 2 * Op::KS * 4 * TB * 16; }

// acc += the products of stages k0 .. k1 - 1 (k0 < k1) of the image; lds: lds_bytes<Op>()
// bytes, 16-byte aligned, free again after the loop's last barrier.  Whole workgroup.
// fpad is taken by reference, the kernel's argument itself, as the loop's lambdas held it
// when they stood in the kernels: by value, the compiler keeps the 64 store masks of the
// uint8 direct epilogue in SGPRs across its loops and spills them to VGPR lanes (212 VGPRs
// for 204, 89.0 us for 87.0 us on a c1 worker shard of uint8 samples).
template <class Op>
__device__ __forceinline__ void k_loop(const uint8_t* __restrict__ img, const int64_t& fpad,
                                       const Item& it, int64_t k0, int64_t k1, uint8_t* lds,
                                       typename Op::Acc (&acc)[4][4]) {
  constexpr int KS = Op::KS, PF = Op::PF;
  constexpr int NH = 2 * KS;  // 16-byte pieces per thread, panel and stage
  constexpr int PANEL = KS * 4 * TB * 16;
  static_assert(PF >= 2 && PF % 2 == 0, "ring slot & 1 is the LDS buffer");
  // staging: thread t moves the 16-byte pieces c = t + 256 h of each panel (4 KS row groups
  // x 128 features)
  auto load = [&](int64_t st, u32x4 (&ra)[NH], u32x4 (&rb)[NH]) {
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int c = it.tid + h * THR;
      const int grp = c >> 7, fl = c & 127;
      ra[h] = *reinterpret_cast<const u32x4*>(img + img_off(KS * st + (grp >> 2), grp & 3, it.i0 + fl, fpad));
      rb[h] = *reinterpret_cast<const u32x4*>(img + img_off(KS * st + (grp >> 2), grp & 3, it.j0 + fl, fpad));
    }
  };
  auto put = [&](int b, const u32x4 (&ra)[NH], const u32x4 (&rb)[NH]) {
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int c = it.tid + h * THR;
      *reinterpret_cast<u32x4*>(lds + (2 * b) * PANEL + c * 16) = ra[h];
      *reinterpret_cast<u32x4*>(lds + (2 * b + 1) * PANEL + c * 16) = rb[h];
    }
  };
  u32x4 ra[PF][NH], rb[PF][NH];
  auto clampk = [&](int64_t st) { return st < k1 ? st : k1 - 1; };
#pragma unroll
  for (int u = 0; u < PF; ++u) load(clampk(k0 + u), ra[u], rb[u]);
  put(0, ra[0], rb[0]);
  __syncthreads();
  const int g = it.lane >> 4, c = it.lane & 15;
  auto body = [&](int64_t kk, int u) {
    load(clampk(kk + PF), ra[u], rb[u]);  // slot u's stage is already in LDS
    const int b = u & 1;
    if (it.active) {
      const uint8_t* pa = lds + (2 * b) * PANEL;
      const uint8_t* pb = it.diag ? pa : pa + PANEL;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        typename Op::Frag fa[4], fb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
          fa[a] = *reinterpret_cast<const typename Op::Frag*>(
              pa + ((ks * 4 + g) * TB + 64 * it.wi + 16 * a + c) * 16);
#pragma unroll
        for (int bb = 0; bb < 4; ++bb)
          fb[bb] = *reinterpret_cast<const typename Op::Frag*>(
              pb + ((ks * 4 + g) * TB + 64 * it.wj + 16 * bb + c) * 16);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int bb = 0; bb < 4; ++bb) acc[a][bb] = Op::mfma(fa[a], fb[bb], acc[a][bb]);
      }
    }
    put(b ^ 1, ra[(u + 1) % PF], rb[(u + 1) % PF]);  // stage kk + 1 (a clamped copy past k1)
    __syncthreads();
  };
  int64_t kk = k0;
  for (; kk + PF <= k1; kk += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) body(kk + u, u);
  }
#pragma unroll
  for (int u = 0; u < PF; ++u)
    if (kk + u < k1) body(kk + u, u);
}

}  // namespace itile
}  // namespace deig
