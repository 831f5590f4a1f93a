// pt_closest.hpp -- what the fused pass (pt_kernels_fused.hip), the guide-buffer kernel (pt_kernels_guides.hip) and the ray queries
// (pt_kernels_rays.hip) share: the block prologue (staged single-cell sets and cell tables, the lens table), the primary ray, the closest-hit
// query over every set -- the ONE definition of that loop: each kernel adds what is its own through ClosestHooks -- and the LDS slots a launch
// gives the sets, with the kernel instance they call for.  Moved here verbatim from pt_kernels_fused.hip, so that all three files run the same
// instructions on the same operands.  Also here, each once: the rules of the optimistic / exact pair that every query kernel of the guides and
// the rays file follows (fresh_poi .. defer_wave behind stage_block) and the launch of such a pair (query_dispatch, at the end).
#pragma once
#include <type_traits>
#include "pt_trace_coop.hpp"

#ifndef PT_AABB_UNSIGNED_ZERO
#define PT_AABB_UNSIGNED_ZERO 1   // single-cell sets only (their tmin / tmax / exits are compare-only): see slab1_fast
#endif

#ifndef PT_LANE_LISTS
#define PT_LANE_LISTS 1          // optimistic kernel: single-cell triangle sets through per-lane candidate lists (pt_trace.hpp trace_cell1, LANES)
#endif
#ifndef PT_LANE_LISTS_GRIDS
#define PT_LANE_LISTS_GRIDS 1    // ... in the grid kernels as well (cornell_teapot3 35.8 -> 33.4 ms, cornell_teapot 24.0 -> 22.7, own_gems 12.4 -> 12.8)
#endif
#define PT_LANE_LISTS_FOR(FAST, GRIDS) ((FAST) && PT_LANE_LISTS && ((GRIDS) == 0 || PT_LANE_LISTS_GRIDS))

#ifndef PT_STAGE_TABLES
#define PT_STAGE_TABLES 1
#endif

namespace pt {

// Cold per-ray state parked in LDS instead of registers: the accumulator (touched once per shading event) and the
// path attenuation (once per shade).  Seven dwords per lane = 7 KB per 256-thread block, [word][lane] so a wave's
// access is one conflict-free row.  It buys the register allocator seven VGPRs on a kernel that is held at
// 6 waves/SIMD by an 80-register budget.
#ifndef PT_PARK_LDS
#define PT_PARK_LDS 1
#endif
#ifndef PT_PARK_PN
#define PT_PARK_PN 0   // A/B: parking p and n as well is slower (199.9 vs 196.2 ms): the reloads sit on the critical path
#endif
#ifndef PT_PARK_PN_GRIDS
#define PT_PARK_PN_GRIDS 1   // the same for the grid kernels only: their walks hold far more state (38 -> 22 spilled VGPRs; cornell_teapot3 859 -> 880
                             // Msamples/s, own_gems 2399 -> 2541)
#endif
#define PT_PARK_PN_FOR(GRIDS) (PT_PARK_PN || (PT_PARK_PN_GRIDS && (GRIDS) != 0))
#define PT_PARK_WORDS(GRIDS) (PT_PARK_PN_FOR(GRIDS) ? 13 : 7)

PT_DEV Box set_box(const GridArgs& S) { return set_box_of(S); }


// What a kernel adds to closest_all's loop: four members, called where the loop names them.
//   guard   optimistic kernel only, once, ahead of the ray's reciprocals: asks the ray-side guard and notes a refusal in `defer`
//   top     at the head of every trip of the loop over the sets
//   won     set s has just delivered the closest hit so far
//   put_pn  (kernels that park p and n: PT_PARK_PN_FOR) the vertex as the trip leaves it
// These are the camera kernels': k_guides takes them as they stand, the pass's Park (pt_kernels_fused.hip) replaces put_pn, and k_traceRays
// (pt_kernels_rays.hip RayHooks) the other three.
struct ClosestHooks {
    PT_DEV void guard(Ray& ray, bool& defer) const { if (!(ray.mint == ray.maxt)) defer = defer || !ray_guard(ray); }   // a dead ray divides nothing
    PT_DEV void top(Ray&) const {}
    PT_DEV void won(uint32_t) const {}
    PT_DEV void put_pn(const Poi&) const {}
};

// closest hit over every set in upload order, z-buffered through ray.maxt
// (A10 code.cl:675-800, 802-935, 937-1070; order A10 code.js:1809-1813)
template <bool FAST, int GRIDS, class HOOKS>
PT_DEV void closest_all(const FusedArgs& A, Ray& ray, Poi& poi, const HOOKS& hooks, bool& defer) {
    if (FAST) hooks.guard(ray, defer);
    const RayRcp rr = ray_rcp<FAST>(ray);
    for (uint32_t s = 0; s < A.n_sets; ++s) {
        const GridArgs& S = A.sets[s];
        hooks.top(ray);
        const bool live = !(ray.mint == ray.maxt);
        Hit ch;
        ch.idx = UINT32_MAX;
        if (!GRIDS || S.n == 1u) {
            if (live) {
                pt_count(PC_BOX_TESTS); pt_count(PC_BOX_LANES, true);
                const BoxHit bh = cell1_box<FAST>(ray, rr, S);
                if (bh.v) ch = (S.kind == KIND_SPHERES) ? trace_cell1<SPHERES, false, TRI_A10, FAST>(ray, rr, bh, S) : trace_cell1<TRIANGLES, false, TRI_A10, FAST, false, PT_LANE_LISTS_FOR(FAST, GRIDS)>(ray, rr, bh, S);
            }
        } else if (S.kind == KIND_TRIANGLES) {   // every lane of the wave enters: the tests of the walk are shared (pt_trace_coop.hpp)
            BoxHit bh = {};
            if (live) bh = inter_aabb_t<FAST, true>(ray, rr, set_box(S));
            ch = trace_dda_coop<COOP_CLOSEST, FAST, GRIDS == 1>(live && bh.v, ray, rr, bh, S, defer);
        } else if (live) {
            const BoxHit bh = inter_aabb_t<FAST, true>(ray, rr, set_box(S));
            if (bh.v) ch = trace_dda<SPHERES, false, TRI_A10, FAST, GRIDS == 1>(ray, bh, S, defer);
        }
        if (ch.idx == UINT32_MAX) continue;
        hooks.won(s);
        ray.maxt = ch.t;
        poi.p = fma3(ch.t, ray.d, ray.o);   // getPoint, code.cl:87
        if (S.kind == KIND_SPHERES) {
            poi.n = norm3(sub3(poi.p, ld3(((const float4*)S.prims)[ch.idx])));
            poi.matId = (int32_t)((const uint32_t*)S.matid)[ch.idx];
        } else {
            float w = 1.0f - ch.beta - ch.gamma;  // code.cl:409-411
            if (PT_LANE_LISTS_FOR(FAST, GRIDS) && S.n == 1u && S.lds_off != kNoLds) {
                // a set staged for the candidate loops carries its vertex normals and material ids in LDS too: three ds_read_b128 and a
                // ds_read_b32 instead of four dependent global loads between the hit and the bounce
                const uint32_t base = S.lds_off + 12u * S.nslots;
                const float4* nn = (const float4*)&pt_lds_dyn[base + __umul24(ch.idx, 12u)];
                poi.n = norm3(fma3(ch.gamma, ld3(nn[2]), fma3(w, ld3(nn[0]), scl3(ch.beta, ld3(nn[1])))));
                poi.matId = (int32_t)pt_lds_dyn[base + 12u * S.nslots + ch.idx];
            } else {
                const float4* nn = (const float4*)S.normals + 3u * (size_t)ch.idx;
                poi.n = norm3(fma3(ch.gamma, ld3(nn[2]), fma3(w, ld3(nn[0]), scl3(ch.beta, ld3(nn[1])))));
                poi.matId = (int32_t)(S.matid ? ((const uint32_t*)S.matid)[ch.idx] : S.mesh_matid);
            }
        }
#if PT_PARK_LDS
        if (PT_PARK_PN_FOR(GRIDS)) hooks.put_pn(poi);
#endif
    }
}

// Block prologue of the fused kernels.  GRIDS: the cell-offset tables of the grid sets (uint[n^3 + 1] each) are copied into LDS once
// per block, before any thread leaves: launch_fused gave every set that fits a slot (GridArgs::lds_off).  The primitives of a grid stay
// in memory.  PT_LANE_LISTS: likewise the prepared records of the single-cell triangle sets launch_fused gave a slot (the candidate
// loops fetch them per lane by ds_read_b128).
// The k x k lens grid's coordinates (code.cl:482-509): coord = delta / 2 and then `+= delta` per step -- sample (i, j) of every pixel needs
// the i-th and the j-th partial sum of that chain.  One thread walks the chain once per block and leaves the k values in LDS (as
// every lane walking it to its own i and j it cost up to 2 (k - 1) dependent additions per sample: 30 of them at 256 rays per pixel, 62 at
// 1024).  k > kLensTab: the lanes walk.
constexpr uint32_t kLensTab = 64;
static_assert(kLensTab % 4u == 0u, "the static LDS ahead of pt_lds_dyn stays a multiple of 16 bytes");
__shared__ float pt_lens_tab[kLensTab];
__shared__ uint32_t pt_blk_defer[4];   // in-pass resolve: "a sample of this block left the guard windows" (word 0; four words keep what follows 16-byte aligned)
// (the ray count is laundered through an SGPR: as a common subexpression of the block prologue and of every sample's set-up, the float made from it
// stayed alive in a VGPR between the two -- the one register the 64-register build had to spill)
PT_DEV uint32_t lens_side(const FusedArgs& A) {
    uint32_t rpp = A.rpp;
    asm volatile("" : "+s"(rpp));
    return f2u_uniform(cl_sqrt((float)rpp));
}

template <bool FAST, int GRIDS>
PT_DEV void stage_block(const FusedArgs& A) {
    if (threadIdx.x == 0u) pt_blk_defer[0] = 0u;
    if (A.rpp > 1u && threadIdx.x == 0u) {
        const uint32_t side = lens_side(A);
        if (side <= kLensTab) {
            const float delta = 1.0f / (float)side;
            float c = delta / 2.0f;
            for (uint32_t k = 0; k < side; ++k) { pt_lens_tab[k] = c; c += delta; }
        }
    }
    if (!(GRIDS == 1 || PT_LANE_LISTS_FOR(FAST, GRIDS))) __syncthreads();
    if (GRIDS == 1 || PT_LANE_LISTS_FOR(FAST, GRIDS)) {
        for (uint32_t s = 0; s < A.n_sets; ++s) {
            const GridArgs& S = A.sets[s];
            if (S.lds_off == kNoLds) continue;
            if (S.n == 1u) {
                if (!PT_LANE_LISTS_FOR(FAST, GRIDS)) continue;
                // [records 12 words each][vertex normals 12 words each][material ids, one word each: a mesh's single id repeated]
                const uint32_t words = S.nslots * 12u;
                const uint32_t* src = (const uint32_t*)S.prims;
                const uint32_t* nrm = (const uint32_t*)S.normals;
                const uint32_t* mid = (const uint32_t*)S.matid;
                for (uint32_t k = threadIdx.x; k < words; k += 256u) { pt_lds_dyn[S.lds_off + k] = src[k]; pt_lds_dyn[S.lds_off + words + k] = nrm[k]; }
                for (uint32_t k = threadIdx.x; k < S.nslots; k += 256u) pt_lds_dyn[S.lds_off + 2u * words + k] = mid ? mid[k] : S.mesh_matid;
            } else if (GRIDS == 1) {
                const uint32_t words = S.n * S.n * S.n + 1u;
                const uint32_t* src = (const uint32_t*)S.off;
                for (uint32_t k = threadIdx.x; k < words; k += 256u) pt_lds_dyn[S.lds_off + k] = src[k];
            }
        }
        __syncthreads();
    }
}

// ---- The rules of the optimistic / exact pair that every QUERY kernel restates (k_guides, k_traceRays, k_ao, k_traceRadiance, k_viewPass,
// k_viewGuides, k_viewAo), each defined once.  A unit is what the kernel's mask holds a bit for: a ray or a pixel, a lane each.

// a Poi as initTrace resets it (A10 code.cl:538-541)
PT_DEV Poi fresh_poi() {
    Poi poi;
    poi.p = mk3(0.0f, 0.0f, 0.0f);
    poi.n = mk3(0.0f, 0.0f, 0.0f);
    poi.atte = mk3(1.0f, 1.0f, 1.0f);
    poi.matId = -1;
    return poi;
}

// what a lane without a ray rides along with: dead (mint == maxt), so it enters the shared walks and tests nothing of its own
PT_DEV Ray dead_ray() {
    Ray ray;
    ray.o = mk3(0.0f, 0.0f, 0.0f); ray.d = mk3(0.0f, 0.0f, 0.0f); ray.mint = 0.0f; ray.maxt = 0.0f;
    return ray;
}

// The work-item prologue, in two steps (as ONE function with a `bool& valid` the exact kernels' instructions came out reordered:
// profiles/query_helpers/README.md).  Has lane `id` a unit of its own?  It has when the id is inside the launch and -- exact kernel only --
// when redo_mask is null (every unit) or holds the unit's bit (the units the optimistic kernel handed over).
template <bool FAST>
PT_DEV bool unit_valid(uint32_t id, uint32_t count, const uint32_t* redo_mask) {
    bool valid = id < count;
    if (!FAST && redo_mask && valid) valid = (redo_mask[id >> 5] >> (id & 31u) & 1u) != 0u;
    return valid;
}
// ... and may the lane leave?  With grids the walk shares its tests across the wave (pt_trace_coop.hpp): a wave without work leaves at the
// ballot, and in a wave with work a lane without a unit of its own STAYS -- it rides along dead and writes nothing.  Without grids a lane
// without work leaves.
template <int GRIDS>
PT_DEV bool nothing_to_do(bool valid) {
    if (GRIDS) return __builtin_amdgcn_ballot_w64(valid) == 0ull;
    return !valid;
}

// The deferred hand-over of the optimistic kernel: the unit's bit in defer_mask, and nothing of the unit is written -- the exact kernel redoes
// it whole.  Per unit: one atomic (the pixel kernels, where deferral is the exception).
PT_DEV void defer_unit(uint32_t* defer_mask, uint32_t id) { atomicOr(&defer_mask[id >> 5], 1u << (id & 31u)); }
// Per wave (the ray kernels; EVERY lane of the wave calls it: k_traceRadiance does, k_traceRays keeps the same lines as its own lambda, which
// is the only form that leaves its code as it was).  A wave holds 64 consecutive ids from a multiple of 64 on: two whole words of
// the mask, which no other wave touches -- so lanes 0 and 32 store the wave's ballot, a word each (a zero word stays as the host cleared it),
// instead of one atomic per ray: a batch the guard refuses whole made 32 atomics on every word of the mask, and they cost more than tracing
// the batch.
PT_DEV void defer_wave(uint32_t* defer_mask, uint32_t id, bool valid, bool defer) {
    const unsigned long long dm = __builtin_amdgcn_ballot_w64(valid && defer);
    const uint32_t lane = threadIdx.x & 63u;
    if (valid && (lane & 31u) == 0u) {
        const uint32_t w = (uint32_t)(dm >> lane);
        if (w) defer_mask[id >> 5] = w;
    }
}

// initTrace (code.cl:458-543) for one ray id of the tile: thin-lens ray through its pixel, clipped to the scene box
// (tile-local ray ids fit 32 bits: mirt_render_pass refuses a tile of more than 2^32 - 256 rays)
PT_DEV Ray primary_ray(const FusedArgs& A, uint32_t lid) {
    // (the host makes rays_per_pixel k x k; when k is a power of two -- 1, 4, 16, 64, 256, 1024 -- the pixel and the sample are a shift and a mask)
    const bool pow2 = (A.rpp & (A.rpp - 1u)) == 0u;   // wave-uniform
    const uint32_t lpix = pow2 ? lid >> (uint32_t)__builtin_ctz(A.rpp) : lid / A.rpp;
    const uint32_t smp = pow2 ? lid & (A.rpp - 1u) : lid - lpix * A.rpp;
    const uint32_t lrow = lpix / A.width;
    const uint32_t col = lpix - lrow * A.width;
    const uint32_t row = A.row0 + lrow;
    Cam cam;
    cam.eye = ld3(A.cam); cam.U = ld3(A.cam + 3); cam.V = ld3(A.cam + 6); cam.W = ld3(A.cam + 9);
    cam.width = A.cam[12]; cam.height = A.cam[13];
    cam.cols = f2u_uniform(A.cam[14]); cam.rows = f2u_uniform(A.cam[15]);
    Box bound;
    bound.lo = mk3(A.bound[0], A.bound[1], A.bound[2]);
    bound.hi = mk3(A.bound[4], A.bound[5], A.bound[6]);
    const f3 fp = focal_point(cam, (float)col, (float)row, A.focal_length);
    float cx, cy;
    if (A.rpp > 1) {
        // un-jittered k x k lens grid; coordinates accumulate by repeated addition in the
        // reference (coord += delta), so they are rebuilt the same way
        const uint32_t side = lens_side(A);
        const uint32_t i = smp / side, j = smp - i * side;
        if (side <= kLensTab) {   // the chain's partial sums, left in LDS by stage_block
            cy = pt_lens_tab[i];
            cx = pt_lens_tab[j];
        } else {
            const float delta = 1.0f / (float)side;
            cy = delta / 2.0f;
            for (uint32_t k = 0; k < i; ++k) cy += delta;
            cx = delta / 2.0f;
            for (uint32_t k = 0; k < j; ++k) cx += delta;
        }
    } else {
        float2 c = ((const float2*)A.uv)[lpix];
        cx = c.x;
        cy = c.y;
    }
    Ray ray = thin_lens_ray(cam, fp, A.lens_rad, cx, cy);
    clip_to(ray, bound);
    return ray;
}

// The LDS slots of a launch (GridArgs::lds_off of every set of `b`) and the dynamic LDS its kernel asks for: `lds` with the cell tables staged
// (GRIDS == 1), `lds2` without (GRIDS == 2), `lds_tri` for a scene without grids (GRIDS == 0).  launch_fused, launch_guides and launch_rays all call it, so
// a set is staged for the guide and ray kernels exactly where it is staged for the pass.
struct FusedLds { bool grids, staged; size_t lds_tri, lds2, lds; };
inline FusedLds fused_lds_slots(FusedArgs& b, bool fast) {
    bool grids = false;
    for (uint32_t i = 0; i < b.n_sets; ++i) grids = grids || b.sets[i].n != 1u;
    // LDS slots for the cell-offset tables: all of them or none (the walk's table reads are compiled for one address space)
    uint64_t used = 0;
    for (uint32_t i = 0; i < b.n_sets; ++i) {
        b.sets[i].lds_off = kNoLds;
        if (b.sets[i].n > 1u) { b.sets[i].lds_off = kCoopWordsPerBlock + (uint32_t)(used < kLdsOffWords ? used : kLdsOffWords); used += (uint64_t)b.sets[i].n * b.sets[i].n * b.sets[i].n + 1u; }
    }
    const bool staged = PT_STAGE_TABLES && used <= kLdsOffWords;
    if (grids && !staged)
        for (uint32_t i = 0; i < b.n_sets; ++i) b.sets[i].lds_off = kNoLds;
    // ... then the prepared records of the single-cell triangle sets, for the candidate loops of the optimistic kernel: all that fit
    // kLdsTriMax records, in upload order (a set without a slot runs the wave-uniform loop)
    uint32_t tri_words = 0;
    const uint32_t tri_base = grids ? kCoopWordsPerBlock + (staged ? (uint32_t)used : 0u) : 0u;   // multiples of 4 words: kCoopWordsPerBlock is, `used` is rounded up below
    const uint32_t tri_base4 = (tri_base + 3u) & ~3u;
    if (fast && PT_LANE_LISTS_FOR(true, grids ? 1 : 0)) {
        uint32_t tris = 0;
        for (uint32_t i = 0; i < b.n_sets; ++i) {
            GridArgs& S = b.sets[i];
            if (S.n != 1u || S.kind != KIND_TRIANGLES || !S.pnorm || S.nslots == 0u || tris + S.nslots > kLdsTriMax) continue;
            S.lds_off = tri_base4 + tri_words;
            tri_words += S.nslots * 28u;   // records, vertex normals, material ids (stage_block), rounded up to whole float4s
            tris += S.nslots;
        }
    }
    // dynamic LDS: the waves' exchange areas, then the staged tables (what the scene needs, not the 16 KB cap: occupancy), then the staged triangles
    const size_t lds_tri = tri_words ? (size_t)(tri_base4 - tri_base + tri_words) * 4u : 0u;
    const size_t lds2 = (size_t)kCoopWordsPerBlock * 4u + lds_tri, lds = (size_t)kCoopWordsPerBlock * 4u + (staged ? (size_t)used * 4u : 0u) + lds_tri;
    return FusedLds{grids, staged, lds_tri, lds2, lds};
}
// ... and the kernel those slots call for: launch(std::integral_constant<int, GRIDS>, the dynamic LDS bytes of that GRIDS)
template <class LAUNCH>
inline void fused_lds_dispatch(const FusedLds& L, const LAUNCH& launch) {
    if (L.grids && L.staged) launch(std::integral_constant<int, 1>{}, L.lds);
    else if (L.grids) launch(std::integral_constant<int, 2>{}, L.lds2);
    else launch(std::integral_constant<int, 0>{}, L.lds_tri);
}
// ... and the launch of a query kernel's optimistic / exact pair, either half of it.  `b`: the launch's own copy of the arguments, the fields
// that are the caller's already set; it gets its LDS slots here.  fast: the optimistic kernel, which sets the bits of the units it hands over
// in defer_mask (the host cleared it) and has no redo mask; !fast: the exact kernel, over the units of redo_mask or over every unit when it
// is null, and with no defer mask.  launch(std::bool_constant<FAST>, std::integral_constant<int, GRIDS>, the dynamic LDS bytes, the defer mask
// and the redo mask THAT kernel gets).
template <class LAUNCH>
inline void query_dispatch(FusedArgs& b, bool fast, uint32_t* defer_mask, const uint32_t* redo_mask, const LAUNCH& launch) {
    const FusedLds L = fused_lds_slots(b, fast);
    if (fast) fused_lds_dispatch(L, [&](auto G, size_t lds) { launch(std::true_type{}, G, lds, defer_mask, (const uint32_t*)nullptr); });
    else fused_lds_dispatch(L, [&](auto G, size_t lds) { launch(std::false_type{}, G, lds, (uint32_t*)nullptr, redo_mask); });
}

}  // namespace pt
