// Covariance of bf16 samples taken as they are (deig_syrk_bf16):  S = alpha X^T X (+ S).
// A bf16 x bf16 product is exact in fp32 (8 x 8 significant bits), so one
// v_mfma_f32_16x16x32_bf16 product per fragment pair gives what the split3 kernel
// (syrk_split.hip) needs three for on a widened copy - whose lo pieces are all zero - and
// there is no split pass, no fp32 copy and no lo*lo diagonal correction.  The only error is
// the fp32 summation, kept two-level: no MFMA accumulator takes more than kFlushRows = 16384
// rows before it is written out as a partial, and the partials are added in a fixed order.
//
// Pipeline, per row chunk (the chunk is what the workspace's image holds):
//  * bf16_prep_kernel relays the chunk of X into an image in MFMA operand order:
//    [k-step of 32 rows][g = 8-row group][feature, padded to 128][8 rows = 16 B], the 16
//    bytes lane (g, feature) feeds to the MFMA.  Rows past n and features past d are zero;
//    no element behind column d of a row is read.
//  * bf16_syrk_kernel: one workgroup per (lower 128 x 128 tile, K segment) runs the tile K
//    loop of syrk_image_tile.hpp with 64-row stages (two MFMA K-steps per barrier) and fp32
//    accumulators, and stores them to a slab of its own (fragment order: one 16-byte store per
//    lane and MFMA block, fully coalesced).  Plain independent workgroups: nobody waits on
//    anybody, no atomics.
//  * bf16_reduce_kernel (syrk_bf16_tile.hpp, with the loop's operation and the slab layout:
//    shared with gram_nt.hip): one workgroup per tile adds the segments' slabs in order, applies
//    alpha, adds S when accumulating (the caller's flag, and every chunk after the first),
//    and writes S[i][j] and, through LDS, the mirror S[j][i] from the same value.
// Every slab entry that is read was written by this call (a diagonal tile's upper wave
// block is neither), so the workspace may hold anything on entry.
#include "syrk_bf16_tile.hpp"

namespace deig {
namespace {

constexpr int kMinSegs = 4, kMaxSegs = 32;

// grid (cdiv(fpad, 512), YB): wave g of a block owns the 8-row group g of K-steps kb =
// by, by + YB, ..., lane l the features 512 bx + 8 l .. + 7: eight 16-byte row loads (1 KiB
// contiguous per row and wave), an 8 x 8 transpose of 16-bit values in registers, eight
// 16-byte stores (128 contiguous bytes per lane, 8 KiB per wave).
__global__ __launch_bounds__(THR) void bf16_prep_kernel(const uint16_t* __restrict__ X, int64_t n,
                                                        int64_t ldx, int64_t d, int64_t fpad,
                                                        int64_t nkb, uint8_t* __restrict__ img) {
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t f = (int64_t)blockIdx.x * 512 + lane * 8;
  if (f >= fpad) return;
  const bool fin = f < d;  // d % 8 == 0: the 8 features are all in or all out
  for (int64_t kb = blockIdx.y; kb < nkb; kb += gridDim.y) {
    u32x4 rows[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int64_t row = kb * KB + g * 8 + r;
      rows[r] = (fin && row < n) ? *reinterpret_cast<const u32x4*>(X + row * ldx + f)
                                 : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {  // features 2 w (low halves) and 2 w + 1 (high halves)
      u32x4 lo, hi;
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // rows 2 q, 2 q + 1
        const uint32_t a = rows[2 * q][w], b = rows[2 * q + 1][w];
        lo[q] = (a & 0xffffu) | (b << 16);
        hi[q] = (a >> 16) | (b & 0xffff0000u);
      }
      *reinterpret_cast<u32x4*>(img + img_off(kb, g, f + 2 * w, fpad)) = lo;
      *reinterpret_cast<u32x4*>(img + img_off(kb, g, f + 2 * w + 1, fpad)) = hi;
    }
  }
}

struct Bf16Sched {
  const uint8_t* img;
  float* slabs;  // [seg][tile][wave][MFMA block a, b][lane][4]
  int64_t nst, fpad;  // SB-row stages of the chunk
  int T, nseg;
};

// One item = (lower tile, K segment); the tile, its LDS stages and the K loop are
// syrk_image_tile.hpp's.
__global__ __launch_bounds__(THR, WGS) void bf16_syrk_kernel(Bf16Sched s) {
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
  itile::k_loop<Bf16Op>(s.img, s.fpad, it, k0, k1, lds, acc);
  if (!it.active) return;
  // the slab of this item, in fragment order: block (a, b) of the wave is 64 lanes x 16 B
  f32x4* slab = reinterpret_cast<f32x4*>(s.slabs + ((int64_t)seg * s.T + tile) * kTileFloats) +
                it.wave * 16 * 64 + it.lane;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) slab[(a * 4 + b) * 64] = acc[a][b];
}

struct Bf16Layout {
  int64_t fpad, T, max_rows;
  int max_segs;
  size_t off_img, row_bytes;
};

// The slabs are sized by d alone (max_segs segments of every lower tile), so what a given
// workspace leaves for the image, and with it the chunk, does not depend on n.
Bf16Layout bf16_layout(int64_t d) {
  Bf16Layout L;
  L.fpad = cdiv(d, TB) * TB;
  const int64_t nt = L.fpad / TB;
  L.T = nt * (nt + 1) / 2;
  int64_t segs = cdiv(kItemsTarget, L.T);
  L.max_segs = (int)(segs < kMinSegs ? kMinSegs : segs > kMaxSegs ? kMaxSegs : segs);
  L.max_rows = (int64_t)L.max_segs * kFlushRows;
  L.off_img = align_up(sizeof(float) * (size_t)L.max_segs * L.T * kTileFloats, 256);
  L.row_bytes = (size_t)L.fpad * 2;
  return L;
}

int64_t pad_rows(int64_t n) { return cdiv(n, SB) * SB; }

}  // namespace

size_t syrk_bf16_workspace_bytes(int64_t n, int64_t d) {
  if (n < 1 || d < 1 || d > (1 << 15)) return 0;
  const Bf16Layout L = bf16_layout(d);
  const int64_t rows = pad_rows(n) < L.max_rows ? pad_rows(n) : L.max_rows;
  return L.off_img + (size_t)rows * L.row_bytes;
}

int syrk_bf16_launch(const void* X, int64_t n, int64_t d, int64_t ldx, float alpha, float* S,
                     int64_t lds, int flags, void* ws, size_t ws_bytes, hipStream_t stream) {
  DEIG_REQUIRE((flags & ~DEIG_SYRK_ACCUMULATE) == 0, "syrk_bf16: unknown flag bits 0x%x", flags);
  DEIG_REQUIRE(n >= 1, "syrk_bf16: n must be >= 1 (got %lld)", (long long)n);
  DEIG_REQUIRE(d >= 8 && d % 8 == 0 && d <= (1 << 15),
               "syrk_bf16: d must be a multiple of 8 in [8, 32768] (got %lld)", (long long)d);
  DEIG_REQUIRE(ldx >= d, "syrk_bf16: ldx must be >= d");
  DEIG_REQUIRE(ldx % 8 == 0, "syrk_bf16: ldx must be a multiple of 8 elements");
  DEIG_REQUIRE(X && S, "syrk_bf16: X and S must not be NULL");
  DEIG_REQUIRE(aligned16(X) && aligned16(S), "syrk_bf16: X and S must be 16-byte aligned");
  DEIG_REQUIRE(lds >= d && lds % 4 == 0, "syrk_bf16: lds must be >= d and a multiple of 4");
  const Bf16Layout L = bf16_layout(d);
  const size_t least = L.off_img + (size_t)SB * L.row_bytes;
  if (!ws || ws_bytes < least)
    return fail(DEIG_EWORKSPACE, "syrk_bf16: workspace %zu bytes < required %zu", ws_bytes, least);
  int64_t chunk = (int64_t)((ws_bytes - L.off_img) / (L.row_bytes * SB)) * SB;
  if (chunk > L.max_rows) chunk = L.max_rows;
  char* base = static_cast<char*>(ws);
  Bf16Sched s;
  s.img = reinterpret_cast<const uint8_t*>(base + L.off_img);
  s.slabs = reinterpret_cast<float*>(base);
  s.fpad = L.fpad;
  s.T = (int)L.T;
  const uint16_t* Xe = static_cast<const uint16_t*>(X);
  int beta = (flags & DEIG_SYRK_ACCUMULATE) ? 1 : 0;
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t rows = n - r0 < chunk ? n - r0 : chunk;
    const int64_t nst = cdiv(rows, SB), nkb = KS * nst;
    // K segments: enough items for two workgroups per CU, each at most kFlushRows rows
    // (the two-level summation) and at least 4 stages (the staging prologue)
    int64_t nseg = cdiv(kItemsTarget, L.T);
    if (nseg > L.max_segs) nseg = L.max_segs;
    if (nseg > nst / 4) nseg = nst / 4;
    if (nseg < cdiv(nst, kSegStages)) nseg = cdiv(nst, kSegStages);
    if (nseg < 1) nseg = 1;
    s.nst = nst;
    s.nseg = (int)nseg;  // <= max_segs: nst <= max_segs * kSegStages
    const int yb = (int)(nkb < 256 ? nkb : 256);
    hipLaunchKernelGGL(bf16_prep_kernel, dim3((unsigned)cdiv(L.fpad, 512), (unsigned)yb), dim3(THR),
                       0, stream, Xe + r0 * ldx, rows, ldx, d, L.fpad, nkb,
                       reinterpret_cast<uint8_t*>(base + L.off_img));
    DEIG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bf16_syrk_kernel, dim3((unsigned)(L.T * nseg)), dim3(THR), 0, stream, s);
    DEIG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bf16_reduce_kernel, dim3((unsigned)L.T), dim3(THR), 0, stream, s.slabs, s.T,
                       s.nseg, alpha, beta, S, lds, d);
    DEIG_HIP_CHECK(hipGetLastError());
    beta = 1;
  }
  return DEIG_OK;
}

}  // namespace deig
