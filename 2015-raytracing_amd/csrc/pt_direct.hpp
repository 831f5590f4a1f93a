// pt_direct.hpp -- the per-light stage of a path segment (shadow ray, any-hit over every set, shade) and the LDS rows it parks a lane's cold
// state in: what the fused pass (pt_kernels_fused.hip) and the radiance of caller-supplied rays (pt_kernels_rays.hip k_traceRadiance) share.
// Moved here verbatim from pt_kernels_fused.hip, so that both files run the same instructions on the same operands
// (profiles/radiance/isa_compare.txt: every kernel of the pass compiles to the assembly it had).
#pragma once
#include "pt_closest.hpp"

#ifndef PT_SKIP_DARK_SHADOWS
#define PT_SKIP_DARK_SHADOWS 1   // grid kernels: a shadow ray whose vertex the light cannot light is not traced (direct_all)
#endif
#ifndef PT_SHADOW_GAP
#define PT_SHADOW_GAP 1          // optimistic kernels without grids: a wave whose shadow segments all stay inside a single-cell triangle set's plane-free
                                 // gap skips the set's box test and the axis entries of its plane list (gap_test below; pt_shadow_gap.hpp).  0: the
                                 // shadow stage as it was
#endif
#define PT_SHADOW_GAP_FOR(FAST, GRIDS) (PT_SHADOW_GAP && (GRIDS) == 0 && PT_LANE_LISTS_FOR(FAST, GRIDS))
namespace pt {

// The gap test of one shadow segment against a set's plane-free gap, gap = GridArgs::gap = {qlo[3], qhi[3], Gm[3], Hm[3]} (scalar operands: kernel
// arguments).  Both ends of the segment [0, hi+], hi+ the sweep's own widened window end, lie inside the open interval (qlo_a, qhi_a) on every axis
// by more than m_a = Gm_a |o|_1 + Hm_a; pt_shadow_gap.hpp derives the constants and what a pass implies.  A NaN anywhere compares false: no pass.
PT_DEV bool gap_test(const Ray& r, const float* gap) {
    const float o1 = __builtin_fabsf(r.o.x) + __builtin_fabsf(r.o.y) + __builtin_fabsf(r.o.z);
    const float hi_p = __builtin_fmaxf(r.maxt * 1.00000095367431640625f, 0x1p-100f);
    const float oo[3] = {r.o.x, r.o.y, r.o.z}, dd[3] = {r.d.x, r.d.y, r.d.z};
    int pass = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float e = cl_fma(hi_p, dd[a], oo[a]);
        const float m = cl_fma(gap[6 + a], o1, gap[9 + a]);
        pass &= (int)(__builtin_fminf(oo[a], e) - gap[a] > m) & (int)(gap[3 + a] - __builtin_fmaxf(oo[a], e) > m);
    }
    return pass != 0;
}

// STRIDE: words between the rows of one lane's record ([word][lane] rows of 256 lanes in k_fusedPass).  ATTE_LDS: the attenuation is
// parked too (else it stays in registers and the p / n rows move up).  As closest_all's hooks (pt_closest.hpp) it adds put_pn alone.
template <int STRIDE, bool ATTE_LDS>
struct ParkT : ClosestHooks {
    static constexpr bool kAtteLds = ATTE_LDS;
    static constexpr int kP = ATTE_LDS ? 7 : 4, kN = kP + 3;
    float* base;   // the lane's word 0
    PT_DEV void put(int w, float v) const { base[w * STRIDE] = v; }
    PT_DEV float get(int w) const { return base[w * STRIDE]; }
    PT_DEV void acc_add(float x, float y, float z) const {
        put(0, get(0) + x); put(1, get(1) + y); put(2, get(2) + z); put(3, get(3) + 1.0f);
    }
    PT_DEV void put_pn(const Poi& q) const { put(kP, q.p.x); put(kP + 1, q.p.y); put(kP + 2, q.p.z); put(kN, q.n.x); put(kN + 1, q.n.y); put(kN + 2, q.n.z); }
    PT_DEV void get_pn(Poi& q) const { q.p = mk3(get(kP), get(kP + 1), get(kP + 2)); q.n = mk3(get(kN), get(kN + 1), get(kN + 2)); }
};
typedef ParkT<256, true> Park;

// per light: shadow ray, any-hit over every set, shade (A10 code.js:1817-1826; code.cl:631-673,
// 1073-1321, 1323-1364)
template <bool FAST, int GRIDS, class PARK>
PT_DEV void direct_all(const FusedArgs& A, Poi& poi, int32_t& seed, float4& acc, const PARK& park, bool& defer) {
    const float4* material = (const float4*)A.material;
    for (uint32_t l = 0; l < A.n_lights; ++l) {
        const LightArgs& L = A.lights[l];
        const bool path = poi.matId >= 0;  // initShadowTrace: a dead path draws nothing (code.cl:645-650)
        bool dark = false;
        Ray sh;
        sh.o = mk3(0.0f, 0.0f, 0.0f);
        sh.d = mk3(0.0f, 0.0f, 0.0f);
        sh.mint = PT_INF;
        sh.maxt = PT_INF;
        if (path) {
#if PT_PARK_LDS
            if (PT_PARK_PN_FOR(GRIDS)) park.get_pn(poi);
#endif
            sh = shadow_ray(poi, ld3(L.shadow), ld3(L.shadow + 3), ld3(L.shadow + 6), L.shadow[9], seed);
#if PT_SKIP_DARK_SHADOWS
            if (GRIDS) {
                // A vertex the light cannot light -- cosx * cosy == 0 in sceneRender's term (code.cl:1339-1349): the surface or the
                // emitter faces away -- adds area * (0 / r^2) * E = 0 whether or not the shadow ray is blocked (a blocked one adds the
                // literal 0; the accumulator, a sum of non-negative terms from +0, cannot tell one zero from another).  Nothing else of the
                // shadow ray survives the kernel, so it is not traced.  Needs r^2 > 0 (else 0 / 0) and finite area and irradiance.
                const float cosx = cl_clamp(dot3(sh.d, poi.n), 0.0f, 1.0f);
                const float cosy = cl_clamp(dot3(neg3(sh.d), ld3(L.scene + 3)), 0.0f, 1.0f);
                const float r = len3(sub3(poi.p, ld3(L.scene)));
                const float fin = L.scene[9] * 0.0f + L.scene[6] * 0.0f + L.scene[7] * 0.0f + L.scene[8] * 0.0f;   // 0 iff all four are finite
                dark = (cosx * cosy == 0.0f) & (r * r > 0.0f) & (fin == 0.0f);
            }
            if (FAST && !dark) defer = defer || !ray_guard(sh);
#else
            if (FAST) defer = defer || !ray_guard(sh);
#endif
        }
        const RayRcp rr = ray_rcp<FAST>(sh);
        // (this loop is stated a second time, as rays_any in pt_kernels_rays.hip, and the two are kept in step by hand: no shared form left this
        // kernel's assembly as it is -- profiles/shared_loops/README.md)
        for (uint32_t s = 0; s < A.n_sets; ++s) {
            const GridArgs& S = A.sets[s];
            const bool live = path && !dark && !(sh.mint == sh.maxt);
            Hit ch;
            bool walked = false;
            if (!GRIDS || S.n == 1u) {
                if (live) {
                    bool gap = false;
                    if (PT_SHADOW_GAP_FOR(FAST, GRIDS) && S.gap_ok != 0u && S.lds_off != kNoLds) {   // wave-uniform: kernel arguments
                        const bool pass = gap_test(sh, S.gap);
                        gap = __builtin_amdgcn_ballot_w64(!pass) == 0ull;   // (the live lanes: the others are masked off here)
                        pt_count(PC_GAP_ASKED);
                        if (gap) pt_count(PC_GAP_TAKEN);
                        if (PT_COUNT && !pass) pt_count(PC_GAP_REFUSED_LANES, true);
                    }
                    if (gap) {
                        // every live lane's segment stays inside the set's plane-free gap: the box test would say v, tmin = 0, exit >= maxt
                        BoxHit bh = {};
                        ch = trace_cell1<TRIANGLES, true, TRI_A10, FAST, true, PT_LANE_LISTS_FOR(FAST, GRIDS), true>(sh, rr, bh, S);
                        walked = true;
                    } else {
                        pt_count(PC_BOX_TESTS); pt_count(PC_BOX_LANES, true);
                        const BoxHit bh = cell1_box<FAST>(sh, rr, S);
                        if (bh.v) {
                            ch = (S.kind == KIND_SPHERES) ? trace_cell1<SPHERES, true, TRI_A10, FAST, true>(sh, rr, bh, S) : trace_cell1<TRIANGLES, true, TRI_A10, FAST, true, PT_LANE_LISTS_FOR(FAST, GRIDS)>(sh, rr, bh, S);
                            walked = true;
                        }
                    }
                }
            } else if (S.kind == KIND_TRIANGLES) {
                BoxHit bh = {};
                if (live) bh = inter_aabb_t<FAST, true>(sh, rr, set_box(S));
                walked = live && bh.v;
                ch = trace_dda_coop<COOP_ANY, FAST, GRIDS == 1>(walked, sh, rr, bh, S, defer);
            } else if (live) {
                const BoxHit bh = inter_aabb_t<FAST, true>(sh, rr, set_box(S));
                if (bh.v) {
                    ch = trace_dda<SPHERES, true, TRI_A10, FAST, GRIDS == 1>(sh, bh, S, defer);
                    walked = true;
                }
            }
            if (!walked) continue;
            sh.maxt = ch.t;
            if (ch.idx != UINT32_MAX) sh.mint = ch.t;
        }
        if (!path || (uint32_t)poi.matId >= A.nmat) continue;  // out-of-range id: shade nothing (see k_sceneRender)
        pt_count(PC_SHADE); pt_count(PC_SHADE_LANES, true);
        float4 c4 = material[poi.matId];
#if PT_PARK_LDS
        if (PT_PARK_PN_FOR(GRIDS)) park.get_pn(poi);
        if (PARK::kAtteLds) poi.atte = mk3(park.get(4), park.get(5), park.get(6));
        f3 c = shade_vertex(poi, sh, mk3(c4.x, c4.y, c4.z), ld3(L.scene), ld3(L.scene + 3), ld3(L.scene + 6), L.scene[9]);
        if (PARK::kAtteLds) { park.put(4, poi.atte.x); park.put(5, poi.atte.y); park.put(6, poi.atte.z); }
        park.acc_add(c.x, c.y, c.z);
#else
        f3 c = shade_vertex(poi, sh, mk3(c4.x, c4.y, c4.z), ld3(L.scene), ld3(L.scene + 3), ld3(L.scene + 6), L.scene[9]);
        acc.x += c.x; acc.y += c.y; acc.z += c.z; acc.w += 1.0f;
#endif
    }
}

}  // namespace pt
