// A sample as it lies in memory, stated once for every kernel that stages one (oja.hip,
// gram.hip, pca.hip, pca_u8.hip, pca_bf16.hip): float32, bf16 (bf16_t: the upper 16 bits of the
// fp32 value) or a raw byte.  Widening is exact; a centred sample is staged as
//   t = fl32((double)x - mean[j]),
// formed in double and rounded once (centre1).  Device side: the decoders of a packed dword
// and SampleGroup, four consecutive features of a row as one raw load.  Host side: the
// per-type rules of the entry points that take such samples and dispatch_sample.
#pragma once

#include "deig_internal.hpp"

namespace deig {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- decoders
// Byte e (0..3) of a dword as a float: one byte-to-float convert.
__device__ __forceinline__ float byte_f(uint32_t w, int e) { return (float)((w >> (8 * e)) & 0xffu); }
// The bf16 halves of a dword as floats (element 0 in the low half), and half e & 1.
__device__ __forceinline__ float lo_f(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float hi_f(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }
__device__ __forceinline__ float bf16_f(uint32_t w, int e) { return (e & 1) ? hi_f(w) : lo_f(w); }
// Centring where a value is staged: formed in double, rounded once.
__device__ __forceinline__ float centre1(float x, double mu) { return (float)((double)x - mu); }
__device__ __forceinline__ float centre1(double x, double mu) { return (float)(x - mu); }

// ---------------------------------------------------------------- four features of a row
// SampleGroup<Elem>: Raw, the 16 / 8 / 4 bytes that hold four consecutive features, its load
// (p aligned to the group), exact zeros, and feature e of it as a float.  Also the tag that
// dispatch_sample hands to its callee.
template <class E, class R>
struct SampleGroupOf {
  using Elem = E;
  using Raw = R;
  static __device__ __forceinline__ Raw zero() { return Raw{}; }
  static __device__ __forceinline__ Raw load(const Elem* p) { return *reinterpret_cast<const Raw*>(p); }
};
template <class Elem>
struct SampleGroup;
template <>
struct SampleGroup<float> : SampleGroupOf<float, f32x4> {
  static __device__ __forceinline__ float value(const Raw& x, int e) { return x[e]; }
};
template <>
struct SampleGroup<bf16_t> : SampleGroupOf<bf16_t, u32x2> {
  static __device__ __forceinline__ float value(const Raw& x, int e) { return bf16_f(x[e >> 1], e); }
};
template <>
struct SampleGroup<uint8_t> : SampleGroupOf<uint8_t, uint32_t> {
  static __device__ __forceinline__ float value(const Raw& x, int e) { return byte_f(x, e); }
};

// ---------------------------------------------------------------- host-side rules
// Per element type (indexed by DEIG_F32, DEIG_F64, DEIG_BF16, DEIG_U8): bytes of an element,
// elements in the narrowest load group (d and ldx are multiples of it) and the alignment of X
// in bytes.  DEIG_F64 is no packed sample type: group 0.
struct SampleRules {
  int bytes, group, align;
};
constexpr SampleRules kSampleRules[4] = {{4, 4, 16}, {8, 0, 0}, {2, 8, 16}, {1, 4, 4}};
inline bool sample_type(int xtype) { return xtype >= 0 && xtype < 4 && kSampleRules[xtype].group; }

// Bytes of an element of type xtype: its alignment rule.  known_elem: the float types of the
// shifted covariance (shift.hip), which takes no raw bytes.
inline size_t elem_bytes(int xtype) { return kSampleRules[xtype].bytes; }
inline bool known_elem(int xtype) { return xtype == DEIG_F32 || xtype == DEIG_F64 || xtype == DEIG_BF16; }

// f(SampleGroup<Elem>{}) for the element type of a sample_type(xtype).
template <class F>
auto dispatch_sample(int xtype, F&& f) {
  switch (xtype) {
    case DEIG_F32: return f(SampleGroup<float>{});
    case DEIG_BF16: return f(SampleGroup<bf16_t>{});
    default: return f(SampleGroup<uint8_t>{});
  }
}

}  // namespace deig
