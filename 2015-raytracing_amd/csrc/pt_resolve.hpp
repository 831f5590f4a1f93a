// pt_resolve.hpp -- copyToPixel inside a block (A10 code.cl:1366-1386) with its inputs spelled out: what the fused pass's frame-after-every-pass
// launches (pt_kernels_fused.hip resolve_frame) and the view cameras' pass (pt_kernels_rays.hip k_viewPass) share.  Moved here verbatim from
// pt_kernels_fused.hip, so that both files run the same instructions on the same operands; the single-frame kernels of the pass keep their own
// copy, resolve_block, there.  Also here, for the same two files: guides_emit, the lane walk that writes the first-hit guides of a block's pixels
// from the registers of the pass (k_fusedPass GUIDES, k_viewPass GUIDES).
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

// ---- moved here unchanged from pt_kernels_fused.hip, for k_fusedPass GUIDES and k_viewPass GUIDES (pt_kernels_rays.hip) alike.  There rpp is 4, 16
// or 64; the view cameras add rpp 1, where a pixel is one lane and the walk one trip.
// The first-hit guides of the block's pixels (FusedArgs::guide_nh, guide_ad; defined in pt_kernels_guides.hip), from the registers of the pass
// right after segment 0's closest_all -- the point k_guides takes them at, reached here by the same functions on the same ray ids, so the values
// are k_guides's bit for bit.  The block resolves its pixels (rpp 4, 16 or 64, one contiguous segment): a pixel's samples are the rpp consecutive
// lanes [t & ~(rpp - 1), +rpp) of ONE wave, in sample order.  Every lane walks its pixel's lanes in that order by ds_bpermute and adds what each
// holds -- a lane that is not a hit (a dead vertex, an id past the material table, a lane past the end of the tile riding along) holds +0 in all
// eight, and adding +0 leaves a sum that started at +0 unchanged bit for bit (such a sum is never -0), so the result is the sequential fp32 sum
// over the HIT samples only.  The pixel's first lane stores.  One output after the other: four values and four sums are live at a time.  No LDS
// of its own and no barrier: every lane of the wave is here (a resolving block keeps its lanes to the end) and rpp is wave-uniform.
PT_DEV float lane_get(uint32_t lane4, float v) { return __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute((int)lane4, (int)__float_as_uint(v))); }   // v of lane lane4 / 4
PT_DEV void guides_emit(const FusedArgs& A, const Ray& ray, const Poi& poi, bool valid, uint32_t blk) {
    const uint32_t rpp = A.rpp, t = threadIdx.x;
    const bool hit = valid && poi.matId >= 0 && (uint32_t)poi.matId < A.nmat;
    const uint32_t first = (t & 63u) & ~(rpp - 1u);
    const uint32_t pix = blk * (256u / rpp) + t / rpp;   // tile-local
    const bool store = (t & (rpp - 1u)) == 0u && pix < A.nrows * A.width;
    if (A.guide_nh) {
        const float v0 = hit ? poi.n.x : 0.0f, v1 = hit ? poi.n.y : 0.0f, v2 = hit ? poi.n.z : 0.0f, v3 = hit ? 1.0f : 0.0f;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        for (uint32_t i = 0, at = first << 2; i < rpp; ++i, at += 4u) { s0 += lane_get(at, v0); s1 += lane_get(at, v1); s2 += lane_get(at, v2); s3 += lane_get(at, v3); }
        if (store) ((float4*)A.guide_nh)[pix] = make_float4(s0, s1, s2, s3);
    }
    if (A.guide_ad) {
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (hit) c = ((const float4*)A.material)[poi.matId];
        const float v0 = c.x, v1 = c.y, v2 = c.z, v3 = hit ? ray.maxt : 0.0f;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        for (uint32_t i = 0, at = first << 2; i < rpp; ++i, at += 4u) { s0 += lane_get(at, v0); s1 += lane_get(at, v1); s2 += lane_get(at, v2); s3 += lane_get(at, v3); }
        if (store) ((float4*)A.guide_ad)[pix] = make_float4(s0, s1, s2, s3);
    }
}

}  // namespace pt
