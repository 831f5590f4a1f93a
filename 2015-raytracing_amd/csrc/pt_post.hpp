// pt_post.hpp -- the arithmetic the post-process stage's kernels share (pt_kernels_filter.hip, pt_kernels_upsample.hip), each piece defined once.
// The stage is defined operation by operation in include/mirt.h (mirt_filter_atrous, mirt_upsample_guided) and restated in numpy by
// tests/filter_common.py and tests/upsample_common.py; the kernels equal those restatements bit for bit, in both libraries.
//
// Numerics.  One fp32 operation at a time, rounded on its own: every translation unit builds with -ffp-contract=off, and nothing here is an fma.
// The reference has no post-process stage, so there is ONE contract for libmirt.so and libmirt_default.so: a plain `/` would be AMD's 2.5-ulp
// sequence in the default-contract build, so every quotient is div_cr() -- the operands widened to fp64, divided there (fp64 division is correctly
// rounded in both builds) and rounded back: 53 >= 2 * 24 + 2 bits make the double rounding harmless, the result IS the correctly rounded fp32
// quotient.  A handful of quotients per pixel beside the taps: their cost does not matter.  No exp, pow or sqrt: the edge terms are hats and
// repeated squaring.
#pragma once
#include "pt_numerics.hpp"

namespace pt {

PT_DEV float div_cr(float n, float d) { return (float)((double)n / (double)d); }
// ... and the correctly rounded fp32 square root the same way, for the same reason (fp64 sqrt is correctly rounded in both builds, 53 >= 2 * 24 + 2).
// The view cameras' ray generator (pt_view.hpp) is its one user: the post-process stage itself takes no root.
PT_DEV float sqrt_cr(float x) { return (float)__builtin_sqrt((double)x); }

// A live pixel's guides, normalised by its hit count: r = 1 / hits, then (n^.x, n^.y, n^.z, z) = (n * r, depth * r) -- the filter's prepared
// guide -- and a = albedo * r.  Two functions of r, because a is wanted only where the image is demodulated.
PT_DEV float post_inv_hits(float hits) { return div_cr(1.0f, hits); }
PT_DEV float4 post_guide(const float4 normal_hits, const float4 albedo_depth, float r) {
    return make_float4(normal_hits.x * r, normal_hits.y * r, normal_hits.z * r, albedo_depth.w * r);
}
struct PostAlbedo { float x, y, z; };
PT_DEV PostAlbedo post_albedo(const float4 albedo_depth, float r) { return {albedo_depth.x * r, albedo_depth.y * r, albedo_depth.z * r}; }

// Demodulation: a channel over its albedo where the albedo is positive.  The empty asm keeps the test a branch: as a select, the compiler runs
// the three quotient sequences of a pixel side by side and k_filterPrepare needs 28 VGPRs instead of 23.
PT_DEV float post_demodulate(float c, float a) {
    if (a > 0.0f) {
        c = div_cr(c, a);
        asm("" : "+v"(c));
    }
    return c;
}
PT_DEV void post_demodulate(float& x, float& y, float& z, const PostAlbedo a) { x = post_demodulate(x, a.x); y = post_demodulate(y, a.y); z = post_demodulate(z, a.z); }
// ... and back
PT_DEV float post_modulate(float c, float a) { return a > 0.0f ? c * a : c; }
PT_DEV void post_modulate(float& x, float& y, float& z, const PostAlbedo a) { x = post_modulate(x, a.x); y = post_modulate(y, a.y); z = post_modulate(z, a.z); }

// the normal term of two prepared guides: max(0, n^p . n^q), squared npow times
PT_DEV float post_normal_weight(const float4 gp, const float4 gq, uint32_t npow) {
    float wn = cl_max(0.0f, (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z);
    for (uint32_t j = 0; j < npow; ++j) wn = wn * wn;
    return wn;
}

// the depth term: a hat over |zp - zq| that reaches 0 at sigma_depth * zp; izp is the centre pixel's, computed once
PT_DEV float post_inv_depth(float sigma_depth, float zp) { return div_cr(1.0f, sigma_depth * zp); }
PT_DEV float post_depth_hat(float zp, float zq, float izp) { return cl_max(0.0f, 1.0f - cl_fabs(zp - zq) * izp); }

// the outputs of a pixel, each where the caller asked for it: (x, y, z, w) as it is and / or tone-mapped to RGBA8
PT_DEV void post_store(void* out, void* pixel, uint32_t p, float x, float y, float z, float w, float tone) {
    if (out) ((float4*)out)[p] = make_float4(x, y, z, w);
    if (pixel) ((uchar4*)pixel)[p] = tone_rgba8(x, y, z, tone);
}

}  // namespace pt
