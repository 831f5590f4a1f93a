// pt_upsample_taps.hpp -- where the four taps of a high-resolution pixel lie in the low-resolution image, and how the two image sizes relate
// (mirt_upsample_guided, include/mirt.h).  Plain integer functions of a pixel coordinate and the factor: no HIP header and no device, so a plain
// C++ compiler builds it and tests/test_upsample_taps.py checks it on the CPU (tests/upsample_taps_dump.cpp).  constexpr: the same functions are
// callable from the kernel (pt_kernels_upsample.hip) and from the ABI's argument checks (mirt_abi.cpp).
//
// Low pixel X covers the high pixels f * X .. f * X + f - 1 of its axis: its centre lies at high coordinate f * X + (f - 1) / 2.  In units of half
// a high pixel the centre of high pixel x is 2x + 1, that of low pixel X is f * (2X + 1), and two low centres are 2f apart.  With e = 2x + 1 - f:
//   X0 = floor(e / 2f)   the low pixel at or left of x's centre; -1 for the x left of the first low centre (e < 0: FLOOR, not truncation)
//   m  = e - 2f * X0     in [0, 2f): how far x's centre lies past X0's, so the bilinear weights are 1 - m / 2f for X0 and m / 2f for X0 + 1
#pragma once
#include <stdint.h>

namespace pt {

constexpr uint32_t kUpsampleMinFactor = 2u, kUpsampleMaxFactor = 4u;

constexpr bool upsample_factor_ok(uint32_t f) { return f >= kUpsampleMinFactor && f <= kUpsampleMaxFactor; }

// the low-resolution extent under a high-resolution one, 0 when the factor does not divide it (the two images would not show the same frustum)
constexpr uint32_t upsample_low_extent(uint32_t high, uint32_t f) { return (f != 0u && high % f == 0u) ? high / f : 0u; }

// floor(a / b) for b > 0: C++ division truncates towards zero, one too high for a negative a that b does not divide
constexpr int32_t upsample_floor_div(int32_t a, int32_t b) { return a / b - ((a % b) < 0 ? 1 : 0); }

struct UpsampleTap {
    int32_t q0;    // X0: -1 .. extent / f - 1; the taps of the axis are q0 and q0 + 1
    int32_t m;     // 0 .. 2f - 1
};
// x < 65536 and f <= 4: nothing here leaves int32
constexpr UpsampleTap upsample_tap(uint32_t x, uint32_t f) {
    const int32_t e = 2 * (int32_t)x + 1 - (int32_t)f;
    const int32_t q0 = upsample_floor_div(e, 2 * (int32_t)f);
    return UpsampleTap{q0, e - 2 * (int32_t)f * q0};
}

// the low pixel that covers high pixel x (the fallback's Q0, and where upsampled.w comes from)
constexpr uint32_t upsample_nearest(uint32_t x, uint32_t f) { return x / f; }

}  // namespace pt
