// pt_kernels_fused.hip -- one launch per progressive pass.
//
// What the reference does in 44+ launches per pass (A10 code.js:1806-1854: initTrace,
// sphere/triangle/mesh closest hit, lightRender, then per segment initShadowTrace,
// any-hit kernels, sceneRender, bouncePaths ...), with every stage round-tripping
// Ray(48 B) / Poi(64 B) / shadow Ray(48 B) / acu(16 B) through memory, this kernel does
// per ray in registers: one work-item per ray, the whole path walked in one go.  HBM
// traffic is the seed (4 B in, 4 B out) and the accumulator (16 B in, 16 B out) per ray;
// the scene description arrives as kernel arguments (SGPRs) and the geometry, for the
// single-cell grids of loose primitives (n_slabs == 1, A10 code.js:399), through
// wave-uniform loops, i.e. scalar loads shared by the 64 lanes of a wave.
//
// The per-ray order of operations is exactly the order the reference's kernel sequence
// imposes on one ray id, which is what makes the result bit-identical to the granular
// path and to the oracle:
//   primary ray -> closest(spheres, triangles, mesh 0..M-1) -> lightRender(light 0..L-1)
//   -> for each light: shadow ray, any-hit(spheres, triangles, meshes), shade
//   -> `bounces` x { bounce ray, closest(...), per-light shadow + shade }
// including its quirks: lights scale `atte` once EACH (sceneRender runs per light), a
// bounce that misses re-shades the stale vertex (SURVEY 8a hazards 2, 3).
//
// Triangles are read from a PREPARED copy of the host's position buffer (k_prepTriangles):
// {p0, e1 = p1-p0, e2 = p2-p0, n = cross(e2,e1)} -- the ray-independent head of
// Moeller-Trumbore (A10 code.cl:252-256), computed once with the same fp32 operations, so
// every value that reaches a ray-dependent operation has the bits it has in the reference.
#include <stdlib.h>
#include "pt_closest.hpp"
#include "pt_direct.hpp"   // direct_all and the park rows, shared with k_traceRadiance (pt_kernels_rays.hip)
#include "pt_resolve.hpp"  // resolve_rows and PT_RESOLVE_PRIO, shared with k_viewPass (pt_kernels_rays.hip)

namespace pt {

// prepared triangle: 3 x float4 = {p0.xyz, n.x} {e1.xyz, n.y} {e2.xyz, n.z}
// `insane` (one word, zeroed by the caller) is set when a plane-normal component is neither zero nor within [2^-40, 2^40]:
// such a set must not use the fast reciprocal forms (GridArgs::fast_ok).
__global__ void __launch_bounds__(256) k_prepTriangles(const float4* pos, float4* out, uint32_t count, uint32_t* insane) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    f3 p0 = ld3(pos[3u * i]), p1 = ld3(pos[3u * i + 1]), p2 = ld3(pos[3u * i + 2]);
    f3 e1 = sub3(p1, p0);
    f3 e2 = sub3(p2, p0);
    f3 n = cross3(e2, e1);
    out[3u * i] = make_float4(p0.x, p0.y, p0.z, n.x);
    out[3u * i + 1] = make_float4(e1.x, e1.y, e1.z, n.y);
    out[3u * i + 2] = make_float4(e2.x, e2.y, e2.z, n.z);
    auto bad = [](float v) { const float a = __builtin_fabsf(v); return !(v == 0.0f || (a >= kDenLo && a <= kDenHi)); };   // pt_windows.hpp
    // ... and every vertex / edge component within 2^21 in magnitude (NaN fails): the bounds of the set are the caller's word, the
    // finiteness arguments of the optimistic kernel (pt_trace.hpp) are about the triangles themselves
    auto big = [](float v) { return !(__builtin_fabsf(v) <= kTriMax); };
    if (bad(n.x) || bad(n.y) || bad(n.z) || big(p0.x) || big(p0.y) || big(p0.z) || big(e1.x) || big(e1.y) || big(e1.z) || big(e2.x) || big(e2.y) || big(e2.z))
        atomicOr(insane, 1u);
    // One bounding sphere per group of kTriGroup consecutive records, behind the records: {centre, R'^2} with R' the radius inflated by
    // 1 % plus what the centre's own rounding can move it (pt_trace.hpp group_missed).  The frame kernels of Assign04 / 07 skip a group
    // whose sphere the ray's line misses.
    if ((i % kTriGroup) == 0u) {
        const uint32_t last = i + kTriGroup < count ? i + kTriGroup : count;
        f3 lo = p0, hi = p0;
        for (uint32_t k = 3u * i; k < 3u * last; ++k) {
            const f3 v = ld3(pos[k]);
            lo = mk3(__builtin_fminf(lo.x, v.x), __builtin_fminf(lo.y, v.y), __builtin_fminf(lo.z, v.z));
            hi = mk3(__builtin_fmaxf(hi.x, v.x), __builtin_fmaxf(hi.y, v.y), __builtin_fmaxf(hi.z, v.z));
        }
        const f3 c = mk3(0.5f * (lo.x + hi.x), 0.5f * (lo.y + hi.y), 0.5f * (lo.z + hi.z));
        float r2 = 0.0f;
        for (uint32_t k = 3u * i; k < 3u * last; ++k) {
            const f3 v = sub3(ld3(pos[k]), c);
            r2 = __builtin_fmaxf(r2, v.x * v.x + v.y * v.y + v.z * v.z);
        }
        const float cm = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(c.x), __builtin_fabsf(c.y)), __builtin_fabsf(c.z));
        const float r = __builtin_sqrtf(r2) * 1.01f + 1e-5f * cm + 1e-30f;
        // (a NaN coordinate is ignored by min / max: the triangle it belongs to can only produce a NaN t, which the reference's own
        // interval test rejects -- skipping it changes nothing; an infinite one makes the radius infinite: never skipped)
        ((float4*)(out + 3u * (size_t)count))[i / kTriGroup] = make_float4(c.x, c.y, c.z, r * r);
    }
}

// The candidate sweep's plane list of a small set (count <= kLdsTriMax; GridArgs::pnorm), from the prepared records (layout: pt_launch.hpp
// "plane list").  Per chunk of 32 records (one candidate word), one entry per PLANE -- every record of the chunk whose plane is the same bit
// for bit (n = cross(e2, e1) with -0 read as +0, and k = p0 . n; for an axis plane the coordinate and the one non-zero normal component)
// shares it through a 32-bit record mask (record c0 + j at bit 31 - j): the halves of a quad wherever they sit in the list.  A record whose
// plane is the same with the normal REVERSED (-n, -k: the back face of a double-sided triangle) rides in the entry's second mask: the sweep
// gets its verdict from two more fused operations instead of a whole evaluation.  AXIS planes -- n has two zero components and both edges
// are exactly zero along the third axis, so the plane is {x_a = p0_a} exactly -- are listed per axis as {q = p0_a, n_a, mask, back mask}: the
// sweep needs one product for n . d and two operations for n . o - k.  General planes: {n.xyz, k, mask, back mask, 0, 0}.  Entries travel
// in 64-byte groups (one s_load_dwordx16: four axis entries or two general ones), each class padded with zero-mask entries.
// Margin constants (pt_trace.hpp): M = G |o|_1 + H, G = 2^-17 |e1|_1 |e2|_1, H = max(G |p0|_1, 2^-56), every product rounded up; the sweep
// uses the chunk's largest G and H for every plane of the chunk (a wider margin keeps more, never less).  Serial: at most 96 records, once per buffer content.
__global__ void __launch_bounds__(64) k_planeList(const float4* prep, uint32_t count, uint32_t* out) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    uint32_t* hdr = out;
    uint32_t* ent = out + 16;   // the header is 64 bytes; groups of 16 words follow
    const float up = 1.0000002384185791015625f;   // 1 + 2^-22: more than the rounding of the sums and products below
    auto canon = [](float v) { return v == 0.0f ? 0u : __float_as_uint(v); };   // -0 -> +0 (the sign of a zero component cannot change what n . d <= 0 decides)
    uint32_t groups = 0;   // 64-byte groups written so far
    for (uint32_t c = 0; c < 4u; ++c) {
        const uint32_t lo = c * 32u, hi = lo + 32u < count ? lo + 32u : count;
        hdr[c] = 0u; hdr[4u + c] = groups; hdr[8u + c] = 0u; hdr[12u + c] = 0u;
        if (lo >= count) continue;
        float gmax = 0.0f, hmax = 0.0f;
        // class of every record of the chunk: 0 / 1 / 2 = axis plane along x / y / z, 3 = general; and its key
        uint32_t cls[32], key[32][4];
        for (uint32_t i = lo; i < hi; ++i) {
            const float4 A = prep[3u * i], B = prep[3u * i + 1], C = prep[3u * i + 2];
            const float k = (float)((double)A.x * A.w + (double)A.y * B.w + (double)A.z * C.w);
            const float E = ((__builtin_fabsf(B.x) + __builtin_fabsf(B.y) + __builtin_fabsf(B.z)) * up) * ((__builtin_fabsf(C.x) + __builtin_fabsf(C.y) + __builtin_fabsf(C.z)) * up) * up;
            const float G = 0x1p-17f * E;
            const float H = __builtin_fmaxf(G * ((__builtin_fabsf(A.x) + __builtin_fabsf(A.y) + __builtin_fabsf(A.z)) * up) * up, 0x1p-56f);
            gmax = __builtin_fmaxf(gmax, G); hmax = __builtin_fmaxf(hmax, H);
            const float n[3] = {A.w, B.w, C.w}, p0[3] = {A.x, A.y, A.z}, e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
            uint32_t cl = 3u;
            for (uint32_t a = 0; a < 3u; ++a)
                if (n[a] != 0.0f && n[(a + 1u) % 3u] == 0.0f && n[(a + 2u) % 3u] == 0.0f && e1[a] == 0.0f && e2[a] == 0.0f) cl = a;
            cls[i - lo] = cl;
            if (cl < 3u) { key[i - lo][0] = canon(p0[cl]); key[i - lo][1] = __float_as_uint(n[cl]); key[i - lo][2] = 0u; key[i - lo][3] = 0u; }
            else { key[i - lo][0] = canon(n[0]); key[i - lo][1] = canon(n[1]); key[i - lo][2] = canon(n[2]); key[i - lo][3] = canon(k); }
        }
        hdr[8u + c] = __float_as_uint(gmax); hdr[12u + c] = __float_as_uint(hmax);
        uint32_t packed = 0u;
        for (uint32_t cl = 0; cl < 4u; ++cl) {
            const uint32_t per = cl < 3u ? 4u : 2u, words = cl < 3u ? 4u : 8u;   // entries per group, words per entry
            uint32_t n_ent = 0;
            uint32_t* base = ent + 16u * groups;
            uint32_t done = 0u;   // records of this class already in an entry
            for (uint32_t i = 0; i < hi - lo; ++i) {
                if (cls[i] != cl || (done >> i & 1u)) continue;
                uint32_t mask = 0u, back = 0u;
                // the same plane; the same plane reversed: every key word that is a float negated (zeros stay zeros; an axis plane keeps its coordinate)
                for (uint32_t j = i; j < hi - lo; ++j) {
                    if (cls[j] != cl || (done >> j & 1u)) continue;
                    bool same = true, rev = true;
                    for (uint32_t w = 0; w < 4u; ++w) {
                        const uint32_t a = key[i][w], b = key[j][w];
                        same = same && a == b;
                        const bool coord = cl < 3u && w == 0u;   // q: not a signed quantity of the normal
                        rev = rev && (coord || a == 0u ? a == b : (a ^ 0x80000000u) == b);
                    }
                    if (same) { mask |= 0x80000000u >> j; done |= 1u << j; }
                    else if (rev) { back |= 0x80000000u >> j; done |= 1u << j; }
                }
                uint32_t* e = base + words * n_ent;
                for (uint32_t w = 0; w < words; ++w) e[w] = 0u;
                if (cl < 3u) { e[0] = key[i][0]; e[1] = key[i][1]; e[2] = mask; e[3] = back; }
                else { e[0] = key[i][0]; e[1] = key[i][1]; e[2] = key[i][2]; e[3] = key[i][3]; e[4] = mask; e[5] = back; }
                ++n_ent;
            }
            const uint32_t g = (n_ent + per - 1u) / per;
            for (uint32_t w = words * n_ent; w < 16u * g; ++w) base[w] = 0u;   // padding entries: both masks zero
            packed |= g << (8u * cl);
            groups += g;
        }
        hdr[c] = packed;   // groups per class: x | y << 8 | z << 16 | general << 24
    }
}

// copyToPixel inside the pass (A10 code.cl:1366-1386) for block `blk` of the launch: `rows` = the block's parked accumulators, [channel][lane]
// (rows 0..3 of the park area), final for every lane (the caller's barrier).  The block holds the segments of 256 / seg_len whole pixels
// (FusedArgs::seg_off), lane-contiguous; one lane per (pixel, channel) adds that pixel's seg_len samples in the reference's order -- sequential
// in i, from +0 or from the sum the segments before it left: the fp32 sum is order-dependent -- reading them four at a time (a channel's row is
// contiguous in LDS); the four lanes of a pixel (one DPP quad) hand their sums to the first, which writes `radiance` (the sums) and `pixel`
// (the tone-scaled RGBA8, truncating).
// The ray id of lane t of block `blk` of this launch -- the one place it is derived (FusedArgs::seg_off): sample seg_off + t % seg_len of pixel
// blk * (256 / seg_len) + t / seg_len.  SEG = false, a contiguous segment (seg_len == rpp, or 256, and every launch that does not resolve in the
// pass): the block's first id, scalar arithmetic on kernel arguments, plus the lane.  In 64 bits: the caller checks it against the tile's ray
// count (a lane past the last pixel -- its pixel >= the tile's -- rides along on the tile's last sample); a valid id fits 32 bits.
template <bool SEG>
PT_DEV uint64_t seg_ray(const FusedArgs& A, uint32_t blk, uint32_t t) {
    if (!SEG) return (uint64_t)(blk * A.seg_pitch + A.seg_off) + t;
    const uint32_t sh = (uint32_t)__builtin_ctz(A.seg_len);   // wave-uniform
    const uint32_t pix = (blk << (8u - sh)) + (t >> sh);
    return (uint64_t)pix * A.rpp + (A.seg_off + (t & (A.seg_len - 1u)));
}
PT_DEV void resolve_block(const FusedArgs& A, const float* rows, uint32_t blk, uint64_t n_local) {
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
        if (A.seg_off != 0u && pix0 + j < npix) s = ((const float*)A.radiance)[4u * (size_t)(pix0 + j) + c];
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
        if (A.radiance) ((float4*)A.radiance)[pix0 + j] = make_float4(x, y, z, w);
        if (A.pixel) {
            const float sc = 255.0f * A.res_m;
            const float cx = cl_clamp((x * sc) * 1.8f, 0.0f, 255.0f), cy = cl_clamp((y * sc) * 1.8f, 0.0f, 255.0f), cz = cl_clamp((z * sc) * 1.8f, 0.0f, 255.0f);
            ((uchar4*)A.pixel)[pix0 + j] = make_uchar4((unsigned char)f2u(cx), (unsigned char)f2u(cy), (unsigned char)f2u(cz), 255);
        }
    }
}

// resolve_rows -- resolve_block with its inputs spelled out, for a launch that writes a frame after every pass (FusedArgs::every) -- is
// pt_resolve.hpp's: the view cameras' pass (pt_kernels_rays.hip k_viewPass) resolves its blocks with it too.
// Frame p of the launch's `passes` (pixel, radiance and carry hold that many frames of nrows * width pixels).  Its factor is render_pass_impl's res_m for
// pass pass_index + p, the same double operations: the sum of two integers below 2^32 is exact, and so the product and quotient round as the host's.
PT_DEV void resolve_frame(const FusedArgs& A, const float* rows, uint32_t blk, uint64_t n_local, uint32_t p) {
    const size_t at = (size_t)p * A.nrows * A.width;
    const float m = (float)(1.0 / ((double)A.rpp * ((double)A.pass_index + (double)p)));
    resolve_rows(A, rows, blk, n_local, A.carry ? (const float*)A.carry + 4u * at : nullptr, A.radiance ? (void*)((float4*)A.radiance + at) : nullptr,
                 A.pixel ? (void*)((uchar4*)A.pixel + at) : nullptr, m);
}

#ifndef PT_FUSED_WAVES
#define PT_FUSED_WAVES 6   // waves per SIMD the register allocator must leave room for (A/B without SLP packing: 5 -> 182.8 ms, 6 -> 178.3, 7 -> 181.0, 8 -> 192.1)
#endif
// FAST = true : the optimistic kernel.  Every division in the traversal is one of the exact cheap forms; a sample whose rays
//               ever leave the guard window sets its bit in `defer_mask` and leaves seeds[]/acu[] untouched.
// FAST = false: the exact kernel (true divisions).  With `list` it recomputes the deferred samples; with list == nullptr it
//               is the whole pass (geometry outside the guard, or PT_EXACT_FAST_DIV = 0).
#ifndef PT_FUSED_WAVES_FAST
#define PT_FUSED_WAVES_FAST 8   // the optimistic kernel without the grid walk: 64 VGPRs, no scratch, since its body is straight-line (round 3: 7 -> 109.4 ms, 8 -> 107.7;
                                // round 1, same box: 5 -> 216.7 ms, 6 -> 216.6, 7 -> 213.4, 8 -> 213.7 at depth 8)
#endif
// GRIDS = 0    : every set is a single cell (n == 1: the reference's loose spheres and triangles, A10 code.js:399): only the
//                wave-uniform loops are compiled in.  Without the DDA the register allocator needs 72 VGPRs and no scratch
//                (80 + 56 B with it): 157.3 -> 152.6 ms on the headline scene.  launch_fused picks it when every set has n == 1.
// GRIDS = 1, 2 : sets with n > 1 walk their grid per lane (trace_dda); 1: every cell-offset table is staged in LDS, 2: none is
//                (a scene whose tables exceed kLdsOffWords).
// Tried and dropped for GRIDS: packing the rays that hit a mesh's box across the block's four waves through LDS (one wave walks
// 64 packed rays, three wait at a barrier).  It cuts VALU instructions 4x on those walks and was 30 % SLOWER (cornell_teapot3
// 1080p x16: 72.2 -> 93.8 ms): the waiting waves keep their registers, so each SIMD is left with too few runnable waves.
// What pays instead is sharing the TESTS inside each wave, no barrier, no idle wave: pt_trace_coop.hpp (65.4 -> 40.2 ms).
#ifndef PT_FUSED_WAVES_GRIDS
#define PT_FUSED_WAVES_GRIDS 6   // the grid walk is latency-bound: it wants waves.  Round 3, cornell_teapot3 1080p x 16: 4 waves per SIMD 38.2 ms, 5 (96 VGPRs, no
                                // scratch) 31.6, 6 (80 VGPRs, 18 spilled around the walks, 64 B of scratch) 29.3 -- 6 needs a block's LDS within 26 880 B (six
                                // blocks per CU at the 1280-byte granule), which it is since the owner's ray travels by ds_bpermute (pt_trace_coop.hpp)
                                // (round 2, at five blocks per CU whatever this said: 6 -> 48.8 ms, 5 -> 43.0, 4 -> 48.1)
#endif
// WAVES != 0: an occupancy variant of the optimistic grid kernels.  PT_FUSED_WAVES_GRIDS waves per SIMD only exist while a block's LDS lets as
// many blocks share a CU (26 880 B at six); a scene with bigger cell tables gets five blocks at best, and for it the 96-register build --
// no scratch -- is the better kernel: launch_fused picks by the bytes it is about to ask for.
// The kernel arguments through a pointer the compiler cannot see through, made anew by every trip of the MULTI kernel's pass loop.  As
// loop-invariant loads, the arguments the path reads (camera, bounds, lights, sets ...) were hoisted out of the loop and kept alive across the
// whole path: 15 -> 51 spilled SGPRs and 0 -> 10 spilled VGPRs in the headline kernel.  The pointer stays in the kernarg address space, so the
// loads stay scalar.  (k_fusedPass's FusedArgs is its first argument: offset 0 of the kernarg segment.)
PT_DEV const FusedArgs& opaque_args() {
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const FusedArgs*)p;
}
// The arguments for ONE stage of a segment -- the closest hit, lightRender, the shadow stage -- of the kernels without grids: opaque_args() again,
// made anew at the stage.  What a stage reads of the arguments (the light count and the address of the light records, the set count ...) is
// loop-invariant, so it was loaded ahead of the segment loop and kept across the other stages' loops, where the 64-register build has no SGPR
// left for it: 19 v_readlane_b32 / v_writelane_b32 on the straight-line path of every segment of k_fusedPass<true, 0, 0>, VALU issue slots each.
// Re-read at the stage they are scalar loads from the kernarg segment (cached) and nothing crosses a loop: no lane traffic inside the segment
// loop, 21 -> 7 spilled SGPRs, 98.68 -> 96.29 ms on the headline frame (profiles/segment_audit).  The grid kernels keep the plain reference:
// there the extra address registers turned into spilled VGPRs (profiles/segment_audit/README.md has every instance).
template <int GRIDS>
PT_DEV const FusedArgs& stage_args(const FusedArgs& P) {
    if constexpr (GRIDS == 0) return opaque_args();
    else return P;
}
// MULTI: FusedArgs::passes progressive passes in one launch (mirt_render_passes).  Passes interact only through a ray's own seed and its own
// accumulator, so each lane runs its sample through every pass in a row: the seed stays in a register, the accumulator in the park rows, and
// both are written once at the end -- bit-identical to that many separate passes.  The unit of the optimistic / exact pair is the same as in
// one pass (a sample, or with in-pass resolve a block): a sample that left the guard windows in ANY pass is handed over, and the exact kernel
// re-runs all of its passes from the seed and accumulator it started with, which nothing of it has overwritten.
// MULTI 1: the plain loop, every pass walks its path from the primary ray.  MULTI 2: PRIMARY-HIT REUSE -- for rays_per_pixel > 1 segment 0 is the
// same in every pass (the lens grid is un-jittered and initTrace, the closest hit and lightRender draw nothing from the seed), so passes after the
// first take its vertex (p, n, material) and the light lightRender added, if any, from eight LDS rows pass 0 left (kReuseWords) instead of tracing
// the primary ray again.  (Its guard-window verdict is already in `defer`, which every pass ORs into.)
constexpr int kReuseWords = 8;
PT_DEV float* reuse_rows() {   // [word][lane]: p.xyz, n.xyz, material id, the light lightRender added (-1: none)
    __shared__ __attribute__((aligned(16))) float reuse_mem[kReuseWords][256];
    return &reuse_mem[0][threadIdx.x];
}
// (guides_emit, the lane walk that writes the first-hit guides of the block's pixels, is pt_resolve.hpp's: k_viewPass shares it.)
// SEG: the general form of the ray ids of a launch's segment (seg_ray); false for every contiguous one.
// EVERY: a frame after every pass (FusedArgs::every): instantiated for resolving launches of several passes only.
// GUIDES: the pass writes the first-hit guides of its pixels too (guides_emit): instantiated for resolving launches of one contiguous segment only
// (SEG false).  The optimistic kernel learns its block's verdict only at the end of the path and does not carry eight sums that
// far: it writes the guides at segment 0 whatever the verdict.  A block that defers afterwards is re-run whole by the exact kernel's redo mode,
// which writes the same pixels' guides again, later on the same stream: those are the final ones.
// With MULTI (mirt_render_passes_guided) the guides are taken in pass 0 and nowhere else: the k x k lens grid draws nothing from the seeds, so segment
// 0 is the same in every pass.  The verdict may come in any pass, and with EVERY a deferring block leaves at a frame barrier: either way the redo
// re-runs the block from its pass 0.  Instantiated for scenes without grids and the pairing multipass_reuse picks for them by default, MULTI 2, with
// and without EVERY (launch_seg).  The grid kernels' plain loop (MULTI 1) was built too, every pass reaching that point and the first alone emitting,
// and was slower than the guide launches behind the unguided kernel (31 -> 62 spilled VGPRs at 6 waves): the route rule keeps
// grid scenes of several passes on the two launches (pt_pass_plan.hpp fused_guides_in_passes).
template <bool FAST, int GRIDS, int WAVES = 0, int MULTI = 0, bool SEG = false, bool EVERY = false, bool GUIDES = false>
__global__ void __launch_bounds__(256, WAVES ? WAVES : (GRIDS ? PT_FUSED_WAVES_GRIDS : (FAST ? PT_FUSED_WAVES_FAST : PT_FUSED_WAVES))) k_fusedPass(const FusedArgs A, uint32_t* defer_mask, const uint32_t* redo_mask, uint32_t redo_words) {
    static_assert(!EVERY || (MULTI != 0 && PT_PARK_LDS), "a frame after every pass resolves from the park rows of the multi-pass loop");
    static_assert(!GUIDES || !SEG, "the guides are taken from a resolving launch of one contiguous segment");
    static_assert(!GUIDES || MULTI == 0 || (MULTI == 2 && GRIDS == 0), "guided multi-pass kernels exist without grids, for their default reuse pairing only");
    const uint64_t n_local = (uint64_t)A.nrows * A.width * A.rpp;
    stage_block<FAST, GRIDS>(A);
    // Exact kernel in redo mode (`redo_mask`: the bits the optimistic kernel set): one thread per 32-sample word, a loop over its
    // set bits -- no list, no count, no host round trip between the two kernels.  Otherwise: one thread, one sample, one trip.
    // GRIDS: the walk shares its triangle tests across the wave (pt_trace_coop.hpp), so every lane stays in to the end: a lane
    // without a sample of its own (past the end of the tile; no bit left in its redo word) rides along on the tile's last sample
    // and writes nothing.
    // In-pass resolve (A.resolve): the unit of everything is the BLOCK of 256 samples (FusedArgs::seg_off) -- the optimistic kernel hands a whole
    // block over when one of its samples left the guard windows (a bit per block of the launch in `defer_mask`, the launch's own region of the
    // mask; nothing of the block is written), and the exact kernel's redo mode is one block per 32-block word of that region, every thread one
    // sample of each marked block in turn.  Every thread stays in to the block's barrier: a lane past the end of the tile rides along as in the
    // grid kernels.
    uint64_t base = seg_ray<SEG>(A, blockIdx.x, threadIdx.x);   // (every launch of this kernel uses 256-thread blocks: launch_fused)
    uint32_t todo = 1u;
    uint32_t stride = 1u;
    if (!FAST && redo_mask) {
        if (A.resolve) {
            todo = redo_mask[blockIdx.x];   // (the grid is one block per word)
            stride = 256u;
        } else {
            if (GRIDS) todo = base < redo_words ? redo_mask[base] : 0u;
            else {
                if (base >= redo_words) return;
                todo = redo_mask[base];
            }
            base *= 32u;
        }
    }
  for (;; todo &= todo - 1u) {
    bool valid = todo != 0u;
    if (GRIDS) { if (__builtin_amdgcn_ballot_w64(valid) == 0ull) break; }
    else if (!valid) break;
    // the id is checked in 64 bits (the last block of a tile of nearly 2^32 rays reaches past it) and kept in 32.  (Resolving, redo mode: lane
    // threadIdx.x of the marked block of this trip -- wave-uniform todo.)
    const uint64_t lid64 = stride == 256u ? seg_ray<SEG>(A, blockIdx.x * 32u + (valid ? (uint32_t)__builtin_ctz(todo) : 0u), threadIdx.x)
                                          : base + (valid ? (uint32_t)__builtin_ctz(todo) * stride : 0u);
    uint32_t lid = (uint32_t)lid64;
    if (lid64 >= n_local) {
        if (!GRIDS && !A.resolve) return;
        valid = false;
        lid = (uint32_t)(n_local - 1u);
    }
    bool defer = false;
    int32_t seed = A.seeds[lid];
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // initAcu (A10 code.cl:448-456) when the pass is a frame's first
    if (!A.fresh) acc = ((const float4*)A.acu)[lid];
    Park park;
#if PT_PARK_LDS
    __shared__ __attribute__((aligned(16))) float park_mem[PT_PARK_WORDS(GRIDS)][256];
    park.base = &park_mem[0][threadIdx.x];
    park.put(0, acc.x); park.put(1, acc.y); park.put(2, acc.z); park.put(3, acc.w);
    park.put(4, 1.0f); park.put(5, 1.0f); park.put(6, 1.0f);
#endif
  for (uint32_t pass = 0;;) {   // (one trip unless MULTI)
    const FusedArgs& P = MULTI ? opaque_args() : A;
    if (MULTI && FAST) {   // the ray id from the thread index, as at the end of the path (see there): kept across the passes it cost spills
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        const uint64_t again = seg_ray<SEG>(P, blockIdx.x, t), n = (uint64_t)P.nrows * P.width * P.rpp;
        lid = again < n ? (uint32_t)again : (uint32_t)(n - 1u);
    }
    Ray ray = primary_ray(P, lid);
    Poi poi;
    poi.p = mk3(0.0f, 0.0f, 0.0f);
    poi.n = mk3(0.0f, 0.0f, 0.0f);
    poi.atte = mk3(1.0f, 1.0f, 1.0f);
    poi.matId = -1;

    // segment 0 is the primary ray; segments 1..bounces start with bouncePaths (code.js:1829-1846)
    pt_count(PC_WAVES);
    for (uint32_t seg = 0; seg <= P.bounces; ++seg) {
        pt_count(PC_SEGMENTS);
        if (seg > 0) {
            if (poi.matId >= 0) {
                pt_count(PC_BOUNCE); pt_count(PC_BOUNCE_LANES, true);
#if PT_PARK_LDS
                if (PT_PARK_PN_FOR(GRIDS)) park.get_pn(poi);
#endif
                ray = bounce_ray(poi, seed);
            } else {
                ray.mint = PT_INF;
                ray.maxt = PT_INF;
            }
        }
        if (PT_COUNT && !(ray.mint == ray.maxt)) pt_count(PC_SEG_LANES, true);
        bool reused = false;   // MULTI 2, a pass after the first: segment 0 as pass 0 left it (wave-uniform: every lane of the wave skips the walk)
#if PT_PARK_LDS
        if constexpr (MULTI == 2) {
            float* const reuse = reuse_rows();
            if (seg == 0 && pass != 0u) {
                poi.p = mk3(reuse[0], reuse[256], reuse[512]);
                poi.n = mk3(reuse[768], reuse[1024], reuse[1280]);
                poi.matId = (int32_t)__float_as_uint(reuse[1536]);
                const int32_t lit = (int32_t)__float_as_uint(reuse[1792]);
                if (lit >= 0) {
                    const f3 irr = norm3(ld3(P.lights[lit].light + 6));
                    park.acc_add(irr.x, irr.y, irr.z);
                }
                if (PT_PARK_PN_FOR(GRIDS)) park.put_pn(poi);
                reused = true;
            } else if (seg == 0) {
                reuse[1792] = __uint_as_float(0xFFFFFFFFu);   // pass 0: no light added (yet)
            }
        }
#endif
      if (MULTI != 2 || !reused) {
        closest_all<FAST, GRIDS, Park>(stage_args<GRIDS>(P), ray, poi, park, defer);
        if constexpr (GUIDES) if (seg == 0 && pass == 0u) {   // the block of the launch as at the resolve below: blockIdx alone, or the marked block of this trip
            const uint32_t blk = FAST || stride != 256u ? blockIdx.x : blockIdx.x * 32u + (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_ctz(todo));
            guides_emit(A, ray, poi, valid, blk);
        }
        if (seg == 0) {
            const FusedArgs& PL = stage_args<GRIDS>(P);
            for (uint32_t l = 0; l < PL.n_lights; ++l) {  // lightRender (code.cl:600-629), primary segment only
                if (ray.mint == ray.maxt) continue;
                const LightArgs& L = PL.lights[l];
                f3 irr = norm3(ld3(L.light + 6));
                if (!light_visible(ray, ld3(L.light), ld3(L.light + 3), L.light[9])) continue;
                ray.mint = PT_INF;
                ray.maxt = PT_INF;
                poi.matId = -1;
#if PT_PARK_LDS
                park.acc_add(irr.x, irr.y, irr.z);
                if constexpr (MULTI == 2) reuse_rows()[1792] = __uint_as_float(l);
#else
                acc.x += irr.x; acc.y += irr.y; acc.z += irr.z; acc.w += 1.0f;
#endif
            }
        }
#if PT_PARK_LDS
        if constexpr (MULTI == 2) if (seg == 0) {   // pass 0: keep segment 0 for the passes after it
            float* const reuse = reuse_rows();
            reuse[0] = poi.p.x; reuse[256] = poi.p.y; reuse[512] = poi.p.z;
            reuse[768] = poi.n.x; reuse[1024] = poi.n.y; reuse[1280] = poi.n.z;
            reuse[1536] = __uint_as_float((uint32_t)poi.matId);
        }
#endif
      }
        direct_all<FAST, GRIDS, Park>(stage_args<GRIDS>(P), poi, seed, acc, park, defer);
    }
#if PT_PARK_LDS
    if constexpr (EVERY) if (pass + 1u < A.passes) {
        // The frame after this pass, from the park rows as they stand.  The first barrier makes every lane's accumulator final in LDS, and the block's
        // verdict with it: an optimistic block that has deferred leaves now (the exact kernel re-runs it whole from the seeds and accumulators it
        // started with, every frame included) and saves its remaining passes.  Lanes past the end of the tile ride along and the redo loop is
        // block-uniform, so every thread reaches both barriers.  The second keeps the next pass's light out of the rows until the sums have read them.
        if (FAST && defer) pt_blk_defer[0] = 1u;
        __syncthreads();
        if (FAST && pt_blk_defer[0] != 0u) {
            if (threadIdx.x == 0u) atomicOr(&defer_mask[blockIdx.x >> 5], 1u << (blockIdx.x & 31u));
            return;
        }
        const uint32_t blk = FAST || stride != 256u ? blockIdx.x : blockIdx.x * 32u + (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_ctz(todo));
        resolve_frame(P, &park_mem[0][0], blk, n_local, pass);
#if PT_RESOLVE_PRIO
        __builtin_amdgcn_s_setprio(0);   // (resolve_rows raised it for its chain; the next pass's path runs at the usual priority)
#endif
        __syncthreads();
    }
#endif
    if (!MULTI || ++pass == A.passes) break;
#if PT_PARK_LDS
    park.put(4, 1.0f); park.put(5, 1.0f); park.put(6, 1.0f);   // the next pass's path starts unattenuated; the accumulator goes on
#endif
  }

    if (FAST) {
        // the ray id again, from the thread index (one sample per thread in this kernel): re-deriving it here costs a few instructions,
        // keeping it (and the 64-bit addresses made from it) alive across the whole path cost spilled registers in every variant
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        const uint64_t again = seg_ray<SEG>(A, blockIdx.x, t);
        lid = (uint32_t)again;
        if (GRIDS || A.resolve) valid = again < n_local;   // (a lane past the end of the tile rode along on the tile's last sample)
    }
    if (A.resolve) {   // wave-uniform (a kernel argument)
#if !PT_PARK_LDS
        __shared__ __attribute__((aligned(16))) float park_mem[4][256];
        park_mem[0][threadIdx.x] = acc.x; park_mem[1][threadIdx.x] = acc.y; park_mem[2][threadIdx.x] = acc.z; park_mem[3][threadIdx.x] = acc.w;
#endif
        if (FAST && defer) pt_blk_defer[0] = 1u;
        __syncthreads();   // every lane's accumulator is final in LDS, and so is the flag
        if (FAST && pt_blk_defer[0] != 0u) {   // the whole block goes to the exact kernel: its seeds stay as they were, no pixel of it is written
            if (threadIdx.x == 0u) atomicOr(&defer_mask[blockIdx.x >> 5], 1u << (blockIdx.x & 31u));
            return;
        }
        if (valid) {
            A.seeds[lid] = seed;
            if (A.acu) ((float4*)A.acu)[lid] = make_float4(park_mem[0][threadIdx.x], park_mem[1][threadIdx.x], park_mem[2][threadIdx.x], park_mem[3][threadIdx.x]);
        }
        // the block of the launch: wave-uniform (blockIdx alone in the optimistic kernel; the marked block of this trip in the redo loop)
        const uint32_t blk = FAST || stride != 256u ? blockIdx.x : blockIdx.x * 32u + (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_ctz(todo));
        if constexpr (EVERY) resolve_frame(A, &park_mem[0][0], blk, n_local, A.passes - 1u);
        else resolve_block(A, &park_mem[0][0], blk, n_local);
        if (FAST) return;
        __syncthreads();   // the redo loop's next block parks into the same rows
        continue;
    }
    // The optimistic kernel has one sample per thread: it LEAVES here, so the compiler sees a straight-line body and not a loop (the
    // exact kernel's redo mode does loop over the set bits of its word).  As a loop -- its exit in the grid kernels is a wave ballot, opaque
    // to the compiler -- every sample-independent value of the body (the camera set-up, sqrt(rpp), the lens-grid reciprocals ...) was
    // hoisted out and kept alive through the whole path: that was what the grid kernels spilled.
    if (FAST && defer) {   // hand the sample to the exact kernel: its inputs stay as they were
        if (valid) atomicOr(&defer_mask[lid >> 5], 1u << (lid & 31u));
        return;
    }
    if (valid) {
        A.seeds[lid] = seed;
#if PT_PARK_LDS
        acc = make_float4(park.get(0), park.get(1), park.get(2), park.get(3));
#endif
        ((float4*)A.acu)[lid] = acc;
    }
    if (FAST) return;
  }
}


// deferred-sample bookkeeping: count the set bits (only when the host asks, mirt_pass_deferred)
__global__ void __launch_bounds__(256) k_deferCount(const uint32_t* mask, uint32_t words, uint32_t* count) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = (i < words) ? (uint32_t)__builtin_popcount(mask[i]) : 0u;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}
// Several passes in one launch: primary-hit reuse (MULTI 2) where it pays, the plain loop (MULTI 1) elsewhere.  4 passes, device events, medians of
// 5 alternating repetitions (profiles/multipass/multipass_ab.json): cornell 1080p x 256, depth 8 (single-cell sets) 96.66 ms per pass with reuse, 98.45 plain
// (101.94 as ordinary passes); cornell_teapot3 1080p x 16, depth 5 (grid meshes) 24.52 with reuse (27.16 forced to 6 waves: its 8 LDS rows cost the
// grid kernel a block per CU, and it spills 71 VGPRs) against 20.36 plain (19.89 ordinary).  So: reuse for scenes without grids only.
// MIRT_MULTIPASS_REUSE=1 / 0 forces one or the other -- an A/B switch, read per launch so that one process can alternate them (profiles/multipass_bench.py).
static bool multipass_reuse(bool grids) { const char* e = getenv("MIRT_MULTIPASS_REUSE"); return e && e[0] ? e[0] != '0' : !grids; }
// The guided multi-pass kernels (GUIDES with MULTI) exist for the default pairing only: whether a launch of `a` with several passes would run it now.
bool fused_has_grids(const FusedArgs& a) {
    bool grids = false;
    for (uint32_t i = 0; i < a.n_sets; ++i) grids = grids || a.sets[i].n != 1u;   // as fused_lds_slots
    return grids;
}
bool fused_multipass_default(const FusedArgs& a) { const bool grids = fused_has_grids(a); return multipass_reuse(grids) == !grids; }
template <bool FAST, int GRIDS, int WAVES, bool SEG>
static void launch_seg(const dim3& grid, size_t lds, hipStream_t s, const FusedArgs& b, uint32_t* defer_mask, const uint32_t* redo_mask, uint32_t redo_words) {
    const bool every = b.every != 0u && b.resolve != 0u && b.passes > 1u;   // a frame after every pass (FusedArgs::every)
    if constexpr (!SEG && GRIDS == 0) if (b.passes > 1u && (b.guide_nh || b.guide_ad)) {   // the caller kept to the route rule (fused_guides_in_passes): no grids, the default pairing
        if (every) hipLaunchKernelGGL((k_fusedPass<FAST, 0, WAVES, 2, false, true, true>), grid, dim3(256), lds, s, b, defer_mask, redo_mask, redo_words);
        else hipLaunchKernelGGL((k_fusedPass<FAST, 0, WAVES, 2, false, false, true>), grid, dim3(256), lds, s, b, defer_mask, redo_mask, redo_words);
        return;
    }
    if (every && multipass_reuse(GRIDS != 0)) hipLaunchKernelGGL((k_fusedPass<FAST, GRIDS, WAVES, 2, SEG, true>), grid, dim3(256), lds, s, b, defer_mask, redo_mask, redo_words);
    else if (every) hipLaunchKernelGGL((k_fusedPass<FAST, GRIDS, WAVES, 1, SEG, true>), grid, dim3(256), lds, s, b, defer_mask, redo_mask, redo_words);
    else if (b.passes > 1u && multipass_reuse(GRIDS != 0)) hipLaunchKernelGGL((k_fusedPass<FAST, GRIDS, WAVES, 2, SEG>), grid, dim3(256), lds, s, b, defer_mask, redo_mask, redo_words);
    else if (b.passes > 1u) hipLaunchKernelGGL((k_fusedPass<FAST, GRIDS, WAVES, 1, SEG>), grid, dim3(256), lds, s, b, defer_mask, redo_mask, redo_words);
    else if (!SEG && (b.guide_nh || b.guide_ad)) hipLaunchKernelGGL((k_fusedPass<FAST, GRIDS, WAVES, 0, false, false, true>), grid, dim3(256), lds, s, b, defer_mask, redo_mask, redo_words);
    else hipLaunchKernelGGL((k_fusedPass<FAST, GRIDS, WAVES, 0, SEG>), grid, dim3(256), lds, s, b, defer_mask, redo_mask, redo_words);
}
template <bool FAST, int GRIDS, int WAVES = 0>
static void launch_pass(const dim3& grid, size_t lds, hipStream_t s, const FusedArgs& b, uint32_t* defer_mask, const uint32_t* redo_mask, uint32_t redo_words) {
    if (b.resolve && !fused_segment_contiguous(b.rpp, b.seg_len)) launch_seg<FAST, GRIDS, WAVES, true>(grid, lds, s, b, defer_mask, redo_mask, redo_words);
    else launch_seg<FAST, GRIDS, WAVES, false>(grid, lds, s, b, defer_mask, redo_mask, redo_words);
}
void launch_fused(hipStream_t s, const FusedArgs& a, bool fast, uint32_t* defer_mask, const uint32_t* redo_mask, uint32_t redo_words) {
    const uint64_t n = redo_mask ? redo_words : (uint64_t)a.nrows * a.width * a.rpp;
    if (!n) return;
    FusedArgs b = a;
    const FusedLds slots = fused_lds_slots(b, fast);   // pt_closest.hpp
    const bool grids = slots.grids, staged = slots.staged;
    const size_t lds_tri = slots.lds_tri, lds2 = slots.lds2, lds = slots.lds;
    // redo mode: one thread per 32-sample word of the mask, or (in-pass resolve: the mask is per block) one block per 32-block word.  Otherwise a
    // block per 256 samples of the launch's segment: 256 / seg_len pixels each (FusedArgs::seg_off; without in-pass resolve seg_len is rpp)
    const dim3 grid(redo_mask && a.resolve ? (unsigned)redo_words
                  : a.resolve ? (unsigned)(((uint64_t)a.nrows * a.width * a.seg_len + 255) / 256) : (unsigned)((n + 255) / 256));
    if (fast) {
        // LDS is handed out in 1280-byte granules, 128 of them per CU: the blocks per CU this launch can have, and the waves per SIMD worth compiling for
        static const int force_waves = [] { const char* e = getenv("MIRT_GRID_WAVES"); return e ? atoi(e) : 0; }();   // A/B and test switch
        const size_t fixed = sizeof(float) * ((size_t)PT_PARK_WORDS(1) * 256u + kLensTab   // the grid kernels' static LDS: parked state, lens table
                                              + (b.passes > 1u && multipass_reuse(grids) ? (size_t)kReuseWords * 256u : 0u));   // (and segment 0's rows: MULTI 2)
        const size_t want = grids && staged ? lds : lds2, granules = (want + fixed + 1279u) / 1280u;
        // (several passes in one launch pick the same way: the 5-wave build, spill-free, is slower there too -- cornell_teapot3 1080p x 16, 4 passes,
        // plain loop: 21.12 ms per pass against 20.29 at 6 waves with 39 spilled VGPRs, profiles/multipass/multipass_bench_{5,6}waves_grid.json)
        const bool five = force_waves ? force_waves == 5 : (granules ? 128u / granules : 8u) < (unsigned)PT_FUSED_WAVES_GRIDS;
        if (grids && staged && five) launch_pass<true, 1, 5>(grid, lds, s, b, defer_mask, nullptr, 0u);
        else if (grids && staged) launch_pass<true, 1>(grid, lds, s, b, defer_mask, nullptr, 0u);
        else if (grids && five) launch_pass<true, 2, 5>(grid, lds2, s, b, defer_mask, nullptr, 0u);
        else if (grids) launch_pass<true, 2>(grid, lds2, s, b, defer_mask, nullptr, 0u);
        else launch_pass<true, 0>(grid, lds_tri, s, b, defer_mask, nullptr, 0u);
    } else {
        if (grids && staged) launch_pass<false, 1>(grid, lds, s, b, nullptr, redo_mask, redo_words);
        else if (grids) launch_pass<false, 2>(grid, lds2, s, b, nullptr, redo_mask, redo_words);
        else launch_pass<false, 0>(grid, 0, s, b, nullptr, redo_mask, redo_words);
    }
}
bool fused_fast_available() { return PT_EXACT_FAST_DIV != 0; }
#if PT_COUNT
int debug_counters(unsigned long long* out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(pt_counters), sizeof(unsigned long long) * PC_COUNT) != hipSuccess) return -1;
    if (reset) { unsigned long long z[PC_COUNT] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(pt_counters), z, sizeof z) != hipSuccess) return -1; }
    return 0;
}
#endif
void launch_deferCount(hipStream_t s, const uint32_t* mask, uint32_t words, uint32_t* count) {
    if (words) hipLaunchKernelGGL(k_deferCount, dim3((words + 255) / 256), dim3(256), 0, s, mask, words, count);
}

size_t prepared_bytes(uint32_t count) { return prepared_planes_offset(count) + (count <= kLdsTriMax ? prepared_planes_bytes(count) : 0); }
void launch_prepTriangles(hipStream_t s, const void* pos, void* out, uint32_t count, uint32_t* insane_word) {
    if (!count) return;
    hipLaunchKernelGGL(k_prepTriangles, dim3((count + 255) / 256), dim3(256), 0, s, (const float4*)pos, (float4*)out, count, insane_word);
    if (count <= kLdsTriMax) hipLaunchKernelGGL(k_planeList, dim3(1), dim3(64), 0, s, (const float4*)out, count, (uint32_t*)((char*)out + prepared_planes_offset(count)));
}

}  // namespace pt
