// Fused centred transform of bf16 samples (deig_pca_transform_bf16): pca_packed_tile.hpp's
// kernel on X as n x d row-major bf16 (the upper 16 bits of the fp32 value), read once and
// never widened in memory.  A thread holds 8 features of a row per super-chunk of 64, two per
// dword; d % 8 == 0, so every super-chunk runs both of its compute chunks.
#include "pca_packed_tile.hpp"

namespace deig {
namespace {

struct Bf16Source {
  using Elem = bf16_t;
  static constexpr int F = 8, DW = 4, kXAlign = 16;
  static constexpr bool kShortTail = false;

  // one 16-byte load where the 8 features lie inside d (d % 8 == 0: in or out together)
  static __device__ __forceinline__ void load(const bf16_t* row, bool live, int64_t kc, int64_t d,
                                              uint32_t (&x)[DW]) {
    ptile::u32x4 v = {0u, 0u, 0u, 0u};
    if (live && kc < d) v = *reinterpret_cast<const ptile::u32x4*>(row + kc);
#pragma unroll
    for (int w = 0; w < 4; ++w) x[w] = v[w];
  }
  static __device__ __forceinline__ float value(const uint32_t (&x)[DW], int c, int e, bool centred,
                                                double mu) {
    const float v = bf16_f(x[2 * c + (e >> 1)], e);
    return centred ? centre1(v, mu) : v;
  }
};

}  // namespace

size_t pca_transform_bf16_workspace_bytes(int64_t n, int64_t d, int k) {
  return ptile::workspace_bytes(n, d, k, ptile::kSuper<Bf16Source>);
}

int pca_transform_bf16_launch(const void* X, int64_t n, int64_t d, int64_t ldx, const double* mean,
                              const float* W, int k, int64_t ldw, float* Y, int64_t ldy,
                              float* resid, float* energy, void* ws, size_t ws_bytes,
                              hipStream_t st, bool w_rowmajor) {
  auto check = [&] {
    DEIG_REQUIRE(n >= 1, "pca_transform_bf16: n must be >= 1 (got %lld)", (long long)n);
    DEIG_REQUIRE(d >= 8 && d % 8 == 0 && d <= (int64_t(1) << 31),
                 "pca_transform_bf16: d must be a multiple of 8 (got %lld)", (long long)d);
    DEIG_REQUIRE(ldx >= d && ldx % 8 == 0,
                 "pca_transform_bf16: ldx must be >= d and a multiple of 8 elements");
    return (int)DEIG_OK;
  };
  return ptile::launch<Bf16Source>("pca_transform_bf16", static_cast<const bf16_t*>(X), n, d, ldx,
                                   mean, W, k, ldw, Y, ldy, resid, energy, ws, ws_bytes, st, check,
                                   w_rowmajor);
}

}  // namespace deig
