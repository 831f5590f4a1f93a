// pt_kernels_upsample.hip -- guide-driven (joint-bilateral) upsampling of a frame shaded at 1/f resolution (mirt_upsample_guided): the radiance
// of a (W / f) x (H / f) frame, as a pass or the a-trous filter leaves it, rebuilt at W x H from the first-hit guide buffers of BOTH resolutions
// (pt_kernels_guides.hip).  The definition -- every operation, in order -- is the comment of mirt_upsample_guided in include/mirt.h;
// tests/upsample_common.py restates it in numpy and the kernel equals that restatement bit for bit, in both libraries.
//
// Numerics: pt_post.hpp, which also holds the arithmetic this file shares with the a-trous filter (pt_kernels_filter.hip) -- div_cr(), the guide
// normalisation, demodulation and its inverse, the normal and depth terms, the tone map and the final store.  What is the upsampler's own stays
// here: the bilinear tap weights, the surface / background split, and the fallback to the covering low pixel.
//
// Structure: one thread per high pixel, blocks of 64 x 4 pixels like k_filterDirect.  A wave is 64 neighbours of one high row; its tap reads
// touch 64 / f + 1 consecutive low pixels of one low row, each shared by f x f neighbours, so they are served by L1 / L2; the own guides (32 B)
// and the outputs (20 B) are contiguous per wave.  Where the four taps lie: pt_upsample_taps.hpp (host-only, CPU-tested).  A tap's three float4
// are loaded whether it is live or not, so they are in flight together.  No LDS: DESIGN.md section 5 has the measurement that decides it.
#include "pt_launch.hpp"
#include "pt_post.hpp"
#include "pt_upsample_taps.hpp"

namespace pt {

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
    float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // (n^, z) of this pixel, its albedo, 1 / (sigma_depth * z)
    PostAlbedo ap = {0.0f, 0.0f, 0.0f};
    float izp = 0.0f;
    if (live) {
        const float r = post_inv_hits(nh.w);
        gp = post_guide(nh, ad, r);
        ap = post_albedo(ad, r);
        if (A.depth_on) izp = post_inv_depth(A.sigma_depth, gp.w);
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
                const float r = post_inv_hits(nq.w);
                const float4 gq = post_guide(nq, aq, r);
                if (A.demodulate) post_demodulate(jx, jy, jz, post_albedo(aq, r));   // J(q): the tap's radiance over its own albedo
                w = b * post_normal_weight(gp, gq, A.npow);
                if (A.depth_on) w = w * post_depth_hat(gp.w, gq.w, izp);
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
        if (live && n0.w > 0.0f) {
            if (A.demodulate) post_demodulate(ox, oy, oz, post_albedo(ADl[q0], post_inv_hits(n0.w)));
        } else {
            modulate = false;   // raw radiance: nothing was divided out, nothing is multiplied back
        }
    }
    if (modulate && A.demodulate) post_modulate(ox, oy, oz, ap);
    post_store(A.upsampled, A.pixel, p, ox, oy, oz, R0.w, A.tone);
}

// High rows [row0, row0 + nrows) of the same image (mirt_upsample_guided_rows): k_upsampleGuided operation for operation -- the bits are its --
// with the tap geometry worked on the GLOBAL row y = row0 + the band's row and tested against the low IMAGE, the high guides and the outputs indexed
// by the band's row, and the low buffers, which hold the low rows from lo_row0 on, at qy - lo_row0.  Tile borders are not multiples of the factor, so
// none of this reduces to offset pointers.
__global__ void __launch_bounds__(256) k_upsampleGuidedRows(const UpsampleRowsArgs A) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), yb = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= A.width || yb >= A.nrows) return;
    const uint32_t y = A.row0 + yb;
    const uint32_t f = A.factor;
    const int wl = (int)(A.width / f), hl = (int)(A.height / f);
    const float4* const Rl = (const float4*)A.radiance_lo;
    const float4* const NHl = (const float4*)A.normal_hits_lo;
    const float4* const ADl = (const float4*)A.albedo_depth_lo;
    const uint32_t p = yb * A.width + x;
    const float4 nh = ((const float4*)A.normal_hits)[p];
    const float4 ad = ((const float4*)A.albedo_depth)[p];
    const uint32_t q0 = (upsample_nearest(y, f) - A.lo_row0) * (uint32_t)wl + upsample_nearest(x, f);
    const float4 R0 = Rl[q0];

    const bool live = nh.w > 0.0f;
    float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    PostAlbedo ap = {0.0f, 0.0f, 0.0f};
    float izp = 0.0f;
    if (live) {
        const float r = post_inv_hits(nh.w);
        gp = post_guide(nh, ad, r);
        ap = post_albedo(ad, r);
        if (A.depth_on) izp = post_inv_depth(A.sigma_depth, gp.w);
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
            const uint32_t q = ((uint32_t)qy - A.lo_row0) * (uint32_t)wl + (uint32_t)qx;
            const float4 nq = NHl[q];
            const float4 aq = ADl[q];
            const float4 Rq = Rl[q];
            const bool qlive = nq.w > 0.0f;
            if (qlive != live) continue;
            const float b = by[j] * bx[i];
            float w = b, jx = Rq.x, jy = Rq.y, jz = Rq.z;
            if (live) {
                const float r = post_inv_hits(nq.w);
                const float4 gq = post_guide(nq, aq, r);
                if (A.demodulate) post_demodulate(jx, jy, jz, post_albedo(aq, r));
                w = b * post_normal_weight(gp, gq, A.npow);
                if (A.depth_on) w = w * post_depth_hat(gp.w, gq.w, izp);
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
        const float4 n0 = NHl[q0];
        ox = R0.x; oy = R0.y; oz = R0.z;
        if (live && n0.w > 0.0f) {
            if (A.demodulate) post_demodulate(ox, oy, oz, post_albedo(ADl[q0], post_inv_hits(n0.w)));
        } else {
            modulate = false;
        }
    }
    if (modulate && A.demodulate) post_modulate(ox, oy, oz, ap);
    post_store(A.upsampled, A.pixel, p, ox, oy, oz, R0.w, A.tone);
}

void launch_upsample(hipStream_t s, const UpsampleArgs& a) {
    const dim3 grid((a.width + 63u) / 64u, (a.height + 3u) / 4u);
    hipLaunchKernelGGL(k_upsampleGuided, grid, dim3(256), 0, s, a);
}

void launch_upsampleRows(hipStream_t s, const UpsampleRowsArgs& a) {
    const dim3 grid((a.width + 63u) / 64u, (a.nrows + 3u) / 4u);
    hipLaunchKernelGGL(k_upsampleGuidedRows, grid, dim3(256), 0, s, a);
}

}  // namespace pt
