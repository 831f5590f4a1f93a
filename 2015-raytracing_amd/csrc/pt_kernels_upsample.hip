// pt_kernels_upsample.hip -- guide-driven (joint-bilateral) upsampling of a frame shaded at 1/f resolution (mirt_upsample_guided): the radiance
// of a (W / f) x (H / f) frame, as a pass or the a-trous filter leaves it, rebuilt at W x H from the first-hit guide buffers of BOTH resolutions
// (pt_kernels_guides.hip).  The definition -- every operation, in order -- is the comment of mirt_upsample_guided in include/mirt.h;
// tests/upsample_common.py restates it in numpy and the kernel equals that restatement bit for bit, in both libraries.
//
// Numerics: as pt_kernels_filter.hip.  One fp32 operation at a time (-ffp-contract=off, nothing is an fma), and every quotient is div_cr(): the
// operands widened to fp64, divided there (correctly rounded in both builds) and rounded back, which IS the correctly rounded fp32 quotient --
// one contract for libmirt.so and libmirt_default.so.
//
// Structure: one thread per high pixel, blocks of 64 x 4 pixels like k_filterDirect.  A wave is 64 neighbours of one high row; its tap reads
// touch 64 / f + 1 consecutive low pixels of one low row, each shared by f x f neighbours, so they are served by L1 / L2; the own guides (32 B)
// and the outputs (20 B) are contiguous per wave.  Where the four taps lie: pt_upsample_taps.hpp (host-only, CPU-tested).  A tap's three float4
// are loaded whether it is live or not, so they are in flight together.  No LDS: DESIGN.md section 5 has the measurement that decides it.
#include "pt_launch.hpp"
#include "pt_numerics.hpp"
#include "pt_upsample_taps.hpp"

namespace pt {

namespace {

PT_DEV float div_cr(float n, float d) { return (float)((double)n / (double)d); }

// J(q) of a live low pixel: its radiance over its own albedo, per channel where the albedo is positive
PT_DEV void upsample_tap_value(const UpsampleArgs& A, const float4 R, const float4 ad, float r, float& jx, float& jy, float& jz) {
    jx = R.x; jy = R.y; jz = R.z;
    if (A.demodulate) {
        const float ax = ad.x * r, ay = ad.y * r, az = ad.z * r;
        if (ax > 0.0f) jx = div_cr(R.x, ax);
        if (ay > 0.0f) jy = div_cr(R.y, ay);
        if (az > 0.0f) jz = div_cr(R.z, az);
    }
}

}  // namespace

__global__ void __launch_bounds__(256) k_upsampleGuided(const UpsampleArgs A) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= A.width || y >= A.height) return;
    const uint32_t f = A.factor;
    const int wl = (int)(A.width / f), hl = (int)(A.height / f);
    const float4* const Rl = (const float4*)A.radiance_lo;
    const float4* const NHl = (const float4*)A.normal_hits_lo;
    const float4* const ADl = (const float4*)A.albedo_depth_lo;
    const uint32_t p = y * A.width + x;
    const float4 nh = ((const float4*)A.normal_hits)[p];
    const float4 ad = ((const float4*)A.albedo_depth)[p];
    const uint32_t q0 = upsample_nearest(y, f) * (uint32_t)wl + upsample_nearest(x, f);
    const float4 R0 = Rl[q0];   // Q0 is one of the four taps: upsampled.w, and the fallback's radiance

    const bool live = nh.w > 0.0f;
    float npx = 0.0f, npy = 0.0f, npz = 0.0f, zp = 0.0f, apx = 0.0f, apy = 0.0f, apz = 0.0f, izp = 0.0f;
    if (live) {
        const float r = div_cr(1.0f, nh.w);
        npx = nh.x * r; npy = nh.y * r; npz = nh.z * r;
        zp = ad.w * r;
        apx = ad.x * r; apy = ad.y * r; apz = ad.z * r;
        if (A.depth_on) izp = div_cr(1.0f, A.sigma_depth * zp);
    }

    const UpsampleTap tx = upsample_tap(x, f), ty = upsample_tap(y, f);
    const float den = (float)(2u * f);
    const float fx = div_cr((float)tx.m, den), fy = div_cr((float)ty.m, den);
    const float bx[2] = {1.0f - fx, fx}, by[2] = {1.0f - fy, fy};

    float sumw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int qx = tx.q0 + i, qy = ty.q0 + j;
            if (qx < 0 || qx >= wl || qy < 0 || qy >= hl) continue;
            const uint32_t q = (uint32_t)qy * (uint32_t)wl + (uint32_t)qx;
            const float4 nq = NHl[q];
            const float4 aq = ADl[q];
            const float4 Rq = Rl[q];
            const bool qlive = nq.w > 0.0f;
            if (qlive != live) continue;   // a surface pixel gathers surface taps, a background pixel background taps
            const float b = by[j] * bx[i];
            float w = b, jx = Rq.x, jy = Rq.y, jz = Rq.z;
            if (live) {
                const float r = div_cr(1.0f, nq.w);
                upsample_tap_value(A, Rq, aq, r, jx, jy, jz);
                float wn = cl_max(0.0f, (npx * (nq.x * r) + npy * (nq.y * r)) + npz * (nq.z * r));
                for (uint32_t k = 0; k < A.npow; ++k) wn = wn * wn;
                w = b * wn;
                if (A.depth_on) w = w * cl_max(0.0f, 1.0f - cl_fabs(zp - aq.w * r) * izp);
            }
            if (w > 0.0f) {
                sumw += w;
                sx += jx * w; sy += jy * w; sz += jz * w;
            }
        }
    }

    float ox, oy, oz;
    bool modulate = live;
    if (sumw > 0.0f) {
        ox = div_cr(sx, sumw); oy = div_cr(sy, sumw); oz = div_cr(sz, sumw);
    } else {
        // no tap counted (a surface the low frame does not have, weights that are 0 or NaN): the covering low pixel
        const float4 n0 = NHl[q0];
        ox = R0.x; oy = R0.y; oz = R0.z;
        if (live && n0.w > 0.0f) upsample_tap_value(A, R0, ADl[q0], div_cr(1.0f, n0.w), ox, oy, oz);
        else modulate = false;   // raw radiance: nothing was divided out, nothing is multiplied back
    }
    if (modulate && A.demodulate) {
        if (apx > 0.0f) ox = ox * apx;
        if (apy > 0.0f) oy = oy * apy;
        if (apz > 0.0f) oz = oz * apz;
    }
    if (A.upsampled) ((float4*)A.upsampled)[p] = make_float4(ox, oy, oz, R0.w);
    if (A.pixel) {   // k_copyToPixel's tone map (pt_kernels_granular.hip), as the filter's
        const float sc = 255.0f * A.tone;
        const float r = cl_clamp((ox * sc) * 1.8f, 0.0f, 255.0f);
        const float g = cl_clamp((oy * sc) * 1.8f, 0.0f, 255.0f);
        const float b = cl_clamp((oz * sc) * 1.8f, 0.0f, 255.0f);
        ((uchar4*)A.pixel)[p] = make_uchar4((unsigned char)f2u(r), (unsigned char)f2u(g), (unsigned char)f2u(b), 255);
    }
}

void launch_upsample(hipStream_t s, const UpsampleArgs& a) {
    const dim3 grid((a.width + 63u) / 64u, (a.height + 3u) / 4u);
    hipLaunchKernelGGL(k_upsampleGuided, grid, dim3(256), 0, s, a);
}

}  // namespace pt
