// pt_windows.hpp -- the power-of-two windows inside which the optimistic kernel's cheap divisions are exact (pt_numerics.hpp "exact division,
// cheaper"), each bound written once.  Host and device read them here: the ray side in the kernel (pt_trace.hpp ray_guard, num_window,
// den_window), the triangle records as they are prepared (pt_kernels_fused.hip k_prepTriangles), the set's bounds on the host
// (pt_set_guard.hpp).  Nothing beyond <stdint.h>: a plain C++ compiler builds it and tests/test_set_guard.py checks the bits on the CPU.
#pragma once
#include <stdint.h>

namespace pt {

// a DENOMINATOR -- a ray direction component, a slab width, a triangle-plane normal component: |v| in [2^-40, 2^40]
constexpr float kDenLo = 0x1p-40f, kDenHi = 0x1p40f;
// a POSITION -- a ray origin component, a bound of a set, a single cell's forward exit plane: zero, or |v| in [2^-30, 2^20]
constexpr float kPosLo = 0x1p-30f, kPosHi = 0x1p20f;
// a NUMERATOR of the grid walk -- a span hi - lo, x - lo, x_next - o: zero, or |v| in [2^-60, 2^60]
constexpr float kNumLo = 0x1p-60f, kNumHi = 0x1p60f;
// a triangle's vertex and edge components: |v| <= 2^21
constexpr float kTriMax = 0x1p21f;

// ray_guard's integer form compares bit patterns: for |x| the unsigned order of the bits is the order of the values
constexpr uint32_t kDenLoBits = 0x2B800000u, kDenHiBits = 0x53800000u, kPosLoBits = 0x30800000u, kPosHiBits = 0x49800000u;
static_assert(__builtin_bit_cast(uint32_t, kDenLo) == kDenLoBits && __builtin_bit_cast(uint32_t, kDenHi) == kDenHiBits, "bit patterns of 2^-40, 2^40");
static_assert(__builtin_bit_cast(uint32_t, kPosLo) == kPosLoBits && __builtin_bit_cast(uint32_t, kPosHi) == kPosHiBits, "bit patterns of 2^-30, 2^20");

}  // namespace pt
