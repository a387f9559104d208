// fp32 -> bf16 pieces for the split products (x = hi + lo (+ ...), each piece a bf16):
// the packed conversion (its two halves read back as fp32: lo_f / hi_f, sample_src.hpp) and
// the vector types of the bf16 MFMA operands (syrk_split.hip, sweep.hip, oja.hip).
#pragma once

#include "sample_src.hpp"

namespace deig {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Two fp32 -> packed bf16 (element 0 in the low half), round to nearest even;
// one v_cvt_pk_bf16_f32 (NaN stays NaN).
__device__ __forceinline__ uint32_t cvt2(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}

}  // namespace deig
