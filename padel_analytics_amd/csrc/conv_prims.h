// Device primitives shared by the convolution kernels (fp32 tap, fp16, bf16x3 and h2 families): vector types, raw buffer
// descriptors, the LDS-DMA request, counted waits, the LDS fence.  The index arithmetic that goes with them is conv_index.h.
#pragma once
#include "conv_index.h"
#include <cstdint>

namespace padel {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));

namespace {

// raw buffer descriptor (gfx9 family): base, stride 0, num_records = 2 GiB, 32-bit data format.  Two forms that do NOT compile
// to the same code; a kernel keeps the one it was tuned with.  make_rsrc: the words as an i32x4, the base forced into SGPRs
// with readfirstlane — what the LDS-DMA request's "s" operand wants.  make_buffer_rsrc: the compiler's own descriptor type, for
// the __builtin_amdgcn_raw_buffer_load_* of the register-staged patch kernels.
__device__ __forceinline__ i32x4 make_rsrc(const void* base) {
    const unsigned long long b = (unsigned long long)(uintptr_t)base;
    i32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)b);
    r[1] = __builtin_amdgcn_readfirstlane((int)((unsigned)(b >> 32) & 0xFFFFu));
    r[2] = (int)0x80000000u;
    r[3] = 0x00020000;
    return r;
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_buffer_rsrc(const float* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)0x80000000u, 0x00020000);
}
// a lane offset >= num_records: the load returns zeros (taps outside the image, rows past M: no compare, no select in the loop).
// (kOORh of h2_common.h is a second such value, one that stays out of range under small positive additions.)
constexpr unsigned kOOR = 0xFFFFFFF0u;

// 64 lanes x 16 bytes, buffer (rsrc base + soff + per-lane voff) -> LDS (lds_wave + LDS_IMM + 16 * lane)
template <int LDS_IMM>
__device__ __forceinline__ void lds_dma(unsigned voff, i32x4 rsrc, unsigned soff, unsigned lds_wave) {
    asm volatile("s_add_u32 m0, %[lb], %[imm]\n\ts_nop 0\n\tbuffer_load_dwordx4 %[vo], %[rs], %[so] offen lds"
                 :
                 : [lb] "s"(lds_wave), [imm] "n"(LDS_IMM), [vo] "v"(voff), [rs] "s"(rsrc), [so] "s"(soff)
                 : "memory", "scc");
}
// at most N of this wave's vector-memory requests (LDS-DMA included) still in flight
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// this wave's LDS accesses have completed
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// The sticky "a value did not fit fp16" flag of a model (h2 and fp16 families): each lane brings the OR of its own tests, the wave
// does one ballot and, only when that is non-zero, one atomicOr by its first lane.  Called where the whole wave is active.
__device__ __forceinline__ void range_raise(unsigned* flag, bool bad) {
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

}  // namespace

}  // namespace padel
