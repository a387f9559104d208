// Fused centred transform of uint8 samples (deig_pca_transform_u8): pca_packed_tile.hpp's
// kernel on two sources of bytes.  DEIG_U8_RAW: v = x; DEIG_U8_GRAY3: v = (r + g + b) / 3 of
// interleaved 3-byte pixels, in double.  The bytes are read once: a quarter (raw) or three
// quarters (gray) of what the float kernel reads for the same features.  A thread holds 16
// features of a row per super-chunk of 128; d % 4 == 0, so the last one may be short.
#include "pca_packed_tile.hpp"

namespace deig {
namespace {

typedef ptile::u32x4 u32x4_a4 __attribute__((aligned(4)));  // rows are only 4-byte aligned

template <int BPF>  // bytes per feature
struct U8Source {
  using Elem = uint8_t;
  static constexpr int F = 16, DW = 4 * BPF, kXAlign = 4;
  static constexpr bool kShortTail = true;

  // one aligned-to-4 16-B load per BPF when all 16 features lie inside d, else dword by
  // dword for the 4-feature groups that do (d % 4 == 0: in or out together)
  static __device__ __forceinline__ void load(const uint8_t* row, bool live, int64_t kc, int64_t d,
                                              uint32_t (&x)[DW]) {
#pragma unroll
    for (int w = 0; w < DW; ++w) x[w] = 0u;
    if (live && kc < d) {
      const uint8_t* p = row + BPF * kc;
      if (kc + 16 <= d) {
#pragma unroll
        for (int q = 0; q < BPF; ++q) {
          const ptile::u32x4 v = *reinterpret_cast<const u32x4_a4*>(p + 16 * q);
#pragma unroll
          for (int w = 0; w < 4; ++w) x[4 * q + w] = v[w];
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (kc + 4 * g < d) {
#pragma unroll
            for (int w = 0; w < BPF; ++w)
              x[BPF * g + w] = *reinterpret_cast<const uint32_t*>(p + 4 * (BPF * g + w));
          }
      }
    }
  }
};

struct U8Raw : U8Source<1> {
  static __device__ __forceinline__ float value(const uint32_t (&x)[DW], int c, int e, bool centred,
                                                double mu) {
    // byte_f and centre1 (sample_src.hpp) as text, not as calls: through either helper the
    // sixteen NB instantiations schedule their converts in another order (same instructions)
    const float v = (float)((x[c] >> (8 * e)) & 0xffu);
    return centred ? (float)((double)v - mu) : v;
  }
};

struct U8Gray3 : U8Source<3> {
  static __device__ __forceinline__ float value(const uint32_t (&x)[DW], int c, int e, bool centred,
                                                double mu) {
    uint32_t s = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int byte = 3 * e + b;
      s += (x[3 * c + (byte >> 2)] >> (8 * (byte & 3))) & 0xffu;
    }
    // s / 3.0, correctly rounded, without the division's expansion: q = s * fl(1/3) is
    // within an ulp, the residual fma(-3, q, s) is exact, and one correction step lands on
    // the rounded quotient (equal to s / 3.0 for every s in 0 .. 765: checked exhaustively
    // on the host)
    const double sd = (double)s, third = 1.0 / 3.0;
    const double q = sd * third;
    const double v = fma(fma(-3.0, q, sd), third, q);
    return centred ? centre1(v, mu) : (float)v;
  }
};

}  // namespace

size_t pca_transform_u8_workspace_bytes(int64_t n, int64_t d, int k) {
  return ptile::workspace_bytes(n, d, k, ptile::kSuper<U8Raw>);
}

int pca_transform_u8_launch(const uint8_t* X, int64_t n, int64_t d, int64_t ldx, int mode,
                            const double* mean, const float* W, int k, int64_t ldw, float* Y,
                            int64_t ldy, float* resid, float* energy, void* ws, size_t ws_bytes,
                            hipStream_t st, bool w_rowmajor) {
  const char* what = "pca_transform_u8";
  auto check = [&] { return u8_check_shape(what, n, d, ldx, mode, int64_t(1) << 31); };
  if (mode == DEIG_U8_RAW)
    return ptile::launch<U8Raw>(what, X, n, d, ldx, mean, W, k, ldw, Y, ldy, resid, energy, ws,
                                ws_bytes, st, check, w_rowmajor);
  return ptile::launch<U8Gray3>(what, X, n, d, ldx, mean, W, k, ldw, Y, ldy, resid, energy, ws,
                                ws_bytes, st, check, w_rowmajor);  // an unknown mode: check's to report
}

}  // namespace deig
