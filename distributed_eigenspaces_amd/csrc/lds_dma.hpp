// HBM -> LDS DMA (buffer_load_dwordx4 ... lds) as the covariance kernels issue it
// (syrk.hip, syrk_split.hip): the raw buffer descriptor, the 16-B-per-lane load and the
// counted wait on it.
#pragma once

#include "deig_internal.hpp"

namespace deig {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// Raw buffer descriptor (gfx950): base, stride 0, num_records bytes, dword format.
// Offsets >= nrec are out of range: an out-of-range LDS-DMA writes zeros.
__device__ __forceinline__ i32x4 make_rsrc(const void* base, uint32_t nrec) {
  const uint64_t a = reinterpret_cast<uint64_t>(base);
  i32x4 r;
  r[0] = (int)(uint32_t)a;
  r[1] = (int)((uint32_t)(a >> 32) & 0xffffu);
  r[2] = (int)nrec;
  r[3] = 0x00020000;
  return r;
}

// buffer_load_dwordx4 ... lds: 16 B per lane into LDS at (m0 + 16 * lane).
// Issued from inline asm on purpose: hipcc cannot tell which LDS bytes an
// LDS-DMA writes and would otherwise put vmcnt(0) in front of every ds_read of
// the *other* buffer, serialising the prefetch with the MFMA loop.  The only
// waits on these loads are the explicit ones (wait_vm) before the barrier that
// publishes a buffer.
__device__ __forceinline__ void dma16(i32x4 rsrc, int voff, const void* lds_dst) {
  const unsigned m0v = (unsigned)(uintptr_t)(lds_void*)lds_dst;
  asm volatile("s_mov_b32 m0, %2\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds"
               :
               : "v"(voff), "s"(rsrc), "s"(m0v)
               : "memory", "m0");
}

// At most N of this wave's vector-memory operations still in flight.
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

}  // namespace deig
