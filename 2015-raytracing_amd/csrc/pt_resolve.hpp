// pt_resolve.hpp -- copyToPixel inside a block (A10 code.cl:1366-1386) with its inputs spelled out: what the fused pass's frame-after-every-pass
// launches (pt_kernels_fused.hip resolve_frame) and the view cameras' pass (pt_kernels_rays.hip k_viewPass) share.  Moved here verbatim from
// pt_kernels_fused.hip, so that both files run the same instructions on the same operands; the single-frame kernels of the pass keep their own
// copy, resolve_block, there.
#pragma once
#include "pt_closest.hpp"

#ifndef PT_RESOLVE_PRIO
#define PT_RESOLVE_PRIO 1
#endif
namespace pt {

// `rows` = the block's parked accumulators, [channel][lane] (rows 0..3 of the park area), final for every lane (the caller's barrier).  The block
// holds the segments of 256 / seg_len whole pixels (FusedArgs::seg_off), lane-contiguous; one lane per (pixel, channel) adds that pixel's seg_len
// samples in the reference's order -- sequential in i, from +0 or, with A.seg_off != 0, from `carry` -- reading them four at a time; the four
// lanes of a pixel (one DPP quad) hand their sums to the first, which writes `radiance` (the sums) and `pixel` (the tone-scaled RGBA8,
// truncating) with the tone factor `res_m`; either may be null.
// (A copy of resolve_block, not a generalisation: the single-frame kernels keep resolve_block's instructions -- routed through this function the
// compiler schedules their resolve differently.)
PT_DEV void resolve_rows(const FusedArgs& A, const float* rows, uint32_t blk, uint64_t n_local, const float* carry, void* radiance, void* pixel, float res_m) {
    const uint32_t rpp = A.rpp, per = A.seg_len, ppb = 256u / per;   // per: the rays of ONE pixel this block holds (FusedArgs::seg_len)
    const uint32_t pix0 = blk * ppb, npix = (uint32_t)(n_local / rpp);
#if PT_RESOLVE_PRIO
    // The sums are chains of dependent additions (256 long at 256 rays per pixel, on four lanes) at the very end of a block whose other waves
    // have left: until the chain ends the block's LDS and this wave's slot are held.  At the top priority the chain's instructions issue as they
    // become ready instead of waiting their turn among the SIMD's other waves.
    __builtin_amdgcn_s_setprio(3);
#endif
    for (uint32_t q = threadIdx.x; q < 4u * ppb; q += 256u) {   // whole quads: 4 ppb is a multiple of 4, and so is every q - threadIdx.x
        const uint32_t j = q >> 2, c = q & 3u;
        const float* r = rows + c * 256u + j * per;
        float s = 0.0f;
        // a later segment of a pixel of more than 256 rays: the chain goes on from the sum over the segments before it (FusedArgs::seg_off)
        if (A.seg_off != 0u && pix0 + j < npix) s = carry[4u * (size_t)(pix0 + j) + c];
        if (per >= 4u) {
            const float4* r4 = (const float4*)r;   // 16-byte aligned: the rows are, and `per` is a multiple of 4 (a power of two)
            for (uint32_t i = 0; i < per / 4u; ++i) { const float4 v = r4[i]; s += v.x; s += v.y; s += v.z; s += v.w; }
        } else {
            for (uint32_t i = 0; i < per; ++i) s += r[i];
        }
        const int si = (int)__float_as_uint(s);
        const float x = __uint_as_float((uint32_t)__builtin_amdgcn_mov_dpp(si, 0x00, 0xf, 0xf, true));   // quad_perm [0,0,0,0]
        const float y = __uint_as_float((uint32_t)__builtin_amdgcn_mov_dpp(si, 0x55, 0xf, 0xf, true));   // [1,1,1,1]
        const float z = __uint_as_float((uint32_t)__builtin_amdgcn_mov_dpp(si, 0xaa, 0xf, 0xf, true));   // [2,2,2,2]
        const float w = __uint_as_float((uint32_t)__builtin_amdgcn_mov_dpp(si, 0xff, 0xf, 0xf, true));   // [3,3,3,3]
        if (c != 0u || pix0 + j >= npix) continue;
        if (radiance) ((float4*)radiance)[pix0 + j] = make_float4(x, y, z, w);
        if (pixel) {
            const float sc = 255.0f * res_m;
            const float cx = cl_clamp((x * sc) * 1.8f, 0.0f, 255.0f), cy = cl_clamp((y * sc) * 1.8f, 0.0f, 255.0f), cz = cl_clamp((z * sc) * 1.8f, 0.0f, 255.0f);
            ((uchar4*)pixel)[pix0 + j] = make_uchar4((unsigned char)f2u(cx), (unsigned char)f2u(cy), (unsigned char)f2u(cz), 255);
        }
    }
}

}  // namespace pt
