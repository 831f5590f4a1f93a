// pt_kernels_rays.hip -- ray queries (mirt_trace_closest, mirt_trace_occluded): the closest hit, or whether anything is hit at all, for rays
// the CALLER supplies -- picking, autofocus, visibility between two points, ambient occlusion, baking -- where every other kernel of the library
// starts at the Assign10 camera.
//
// Definition.  Ray i is the record {o, mint, d, maxt} (32 bytes) as given: d is not normalised, t is in units of |d|.
//   closest   the state the kernel-by-kernel path leaves in Ray.maxt and Poi when Ray{o, d, mint, maxt} and a Poi reset as initTrace resets it
//             (A10 code.cl:538-541) run through sphereTrace, triangleTrace and every meshTrace in upload order (code.js:1809-1813):
//             hits[i] = {Poi.normal, Ray.maxt, Poi.p, Poi.matId}, 32 bytes; a miss is (0, 0, 0, the input maxt, 0, 0, 0, -1), and a dead ray
//             (mint == maxt) is a miss.  sets[i] = the index, in that stage order, of the set whose primitive won, or 0xFFFFFFFF.
//   occluded  sceneRender's own test (code.cl:1350): occluded[i] = 1 iff mint == maxt after sphereShadowTrace, triangleShadowTrace and a
//             triangleShadowTrace per mesh have run on the ray in that order -- a ray that enters dead is reported 1.  No t is delivered, so the
//             sets run the fused pass's cheap any-hit forms (COOP_ANY, the blocked-flag cell loops).
//
// The bits are the fused pass's: stage_block and the closest-hit loop are the pass's own functions (pt_closest.hpp: closest_all, to which this
// kernel adds its guard and the winning set's index through RayHooks), the sets get the LDS slots the pass gives them and the kernel instance
// those call for (fused_lds_slots, fused_lds_dispatch), and the optimistic / exact pair is the pass's -- here per RAY: a ray the ray-side guard
// refuses, or whose walk defers, sets its bit and writes nothing, and the exact kernel redoes the marked rays.
// The rules of that pair which every kernel of this file follows are stated ONCE, in pt_closest.hpp, and the kernels call them: which lane has
// a unit of its own and which lane may leave (unit_valid, nothing_to_do), what a lane without one rides along with (dead_ray), the vertex a ray
// starts from (fresh_poi), how a deferred unit is handed over (defer_unit per pixel, defer_wave per wave of rays), and which mask each kernel
// of the pair is launched with (query_dispatch).  Every kernel's code is the parent's, symbol for symbol; where a call would have changed it the
// lines stay hand-written and say so: k_traceRays' prologue and hand-over, and the lightRender loop, which k_traceRadiance and k_viewPass
// still state twice -- a change to one is a change to both (profiles/query_helpers/README.md has the forms tried and the figures).
// The any-hit loop (rays_any) is still stated twice, here and in the shadow stage of direct_all (pt_direct.hpp): every shared form that was
// tried re-allocated registers in k_fusedPass, whose rule is identical assembly (profiles/shared_loops/README.md).  A change to one is a change to both.
//
// Structure: one lane per ray, two float4 loads, the query, two float4 stores (and the optional uint32), or one byte.
//
// A caller's rays are not the camera's: they need not be coherent, and axis-parallel directions are common -- a zero component of d fails the
// guard's |d_k| >= 2^-40, as does a zero-length, infinite or NaN one.  Such batches run mostly in the EXACT kernel (mirt_trace_deferred counts
// them; profiles/rays/timing.json has the measured cost).  The guard windows are what makes the optimistic kernel's divisions exact and are not
// widened for this.
//
// Also here, because it runs rays_any: k_ao, ambient occlusion of the first hit (mirt_render_ao); and because it starts at a caller's ray:
// k_traceRadiance, the pass's path from that ray on (mirt_trace_radiance); and because they are k_traceRadiance with the ray made in registers:
// k_viewRays and k_viewPass, the panoramic, fisheye and orthographic cameras (mirt_view_rays, mirt_render_view), k_viewGuides, their
// first-hit guides (mirt_view_guides), and k_viewAo, their ambient occlusion (mirt_view_ao) -- at the end of the file.
#include "pt_direct.hpp"
#include "pt_rays_guard.hpp"   // keep_in_loop, guard_or_retire, RadiancePark
#include "pt_resolve.hpp"   // resolve_rows: k_viewPass resolves its blocks' pixels as the pass does; guides_emit: its GUIDES instances write the guides
#include "pt_view.hpp"      // view_ray: a sample's ray

namespace pt {

// keep_in_loop, guard_or_retire: pt_rays_guard.hpp

// What this kernel adds to closest_all's loop (pt_closest.hpp ClosestHooks): its own guard, the division kept in the loop, and the index of the
// last set that won
struct RayHooks : ClosestHooks {
    uint32_t& set;
    PT_DEV void guard(Ray& ray, bool& defer) const { guard_or_retire(ray, defer); }
    PT_DEV void top(Ray& ray) const { keep_in_loop(ray); }
    PT_DEV void won(uint32_t s) const { set = s; }
};

// rays_any, the any-hit loop: pt_rays_any.inc, one text for this file and for the batch's translation unit
#include "pt_rays_any.inc"

// rays: two float4 per ray {o, mint} {d, maxt}.  ANY: `occluded` (a byte per ray); else `hits` (two float4 per ray) and / or `sets`.
// defer_mask (optimistic kernel): a bit per ray.  redo_mask (exact kernel only): the rays the optimistic kernel handed over; null: every ray.
template <bool FAST, int GRIDS, bool ANY>
__global__ void __launch_bounds__(256) k_traceRays(const FusedArgs A, const float4* __restrict__ rays, uint32_t count, float4* __restrict__ hits,
                                                   uint32_t* __restrict__ sets, uint8_t* __restrict__ occluded, uint32_t* defer_mask, const uint32_t* redo_mask) {
    stage_block<FAST, GRIDS>(A);
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;   // (count <= 2^32 - 256: mirt_trace_closest)
    // (the prologue and the hand-over are hand-written here: called as unit_valid / nothing_to_do and defer_wave, pt_closest.hpp, whose rules they
    // follow word for word, six instances of this kernel came out as other code and missed the timing rule -- profiles/query_helpers/README.md)
    bool valid = id < count;
    if (!FAST && redo_mask && valid) valid = (redo_mask[id >> 5] >> (id & 31u) & 1u) != 0u;
    if (GRIDS) { if (__builtin_amdgcn_ballot_w64(valid) == 0ull) return; }
    else if (!valid) return;
    Ray ray = dead_ray();
    if (valid) {
        const float4 a = rays[2u * (size_t)id], b = rays[2u * (size_t)id + 1u];
        ray.o = mk3(a.x, a.y, a.z); ray.mint = a.w;
        ray.d = mk3(b.x, b.y, b.z); ray.maxt = b.w;
    }
    bool defer = false;
    const auto hand_over = [&]() {
        const unsigned long long dm = __builtin_amdgcn_ballot_w64(valid && defer);
        const uint32_t lane = threadIdx.x & 63u;
        if (valid && (lane & 31u) == 0u) {
            const uint32_t w = (uint32_t)(dm >> lane);
            if (w) defer_mask[id >> 5] = w;
        }
    };
    if (ANY) {
        rays_any<FAST, GRIDS>(A, ray, defer);
        if (FAST) hand_over();
        if (!valid || (FAST && defer)) return;   // the exact kernel redoes a deferred ray: nothing of it is written
        occluded[id] = ray.mint == ray.maxt ? (uint8_t)1 : (uint8_t)0;
    } else {
        Poi poi = fresh_poi();
        uint32_t won = UINT32_MAX;
        closest_all<FAST, GRIDS>(A, ray, poi, RayHooks{{}, won}, defer);
        if (FAST) hand_over();
        if (!valid || (FAST && defer)) return;
        if (hits) {
            hits[2u * (size_t)id] = make_float4(poi.n.x, poi.n.y, poi.n.z, ray.maxt);
            hits[2u * (size_t)id + 1u] = make_float4(poi.p.x, poi.p.y, poi.p.z, __int_as_float(poi.matId));
        }
        if (sets) sets[id] = won;
    }
}

// fast / defer_mask / redo_mask: query_dispatch's (pt_closest.hpp), a bit per ray.  occluded != null: the occlusion query; else the closest hit
// into hits and / or sets.
void launch_rays(hipStream_t s, const FusedArgs& a, bool fast, const void* rays, uint32_t count, void* hits, uint32_t* sets, uint8_t* occluded,
                 uint32_t* defer_mask, const uint32_t* redo_mask) {
    if (!count) return;
    FusedArgs b = a;
    b.rpp = 1u;   // stage_block: no lens table
    const dim3 grid((unsigned)(((uint64_t)count + 255u) / 256u));
    if (occluded) {
        query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
            hipLaunchKernelGGL((k_traceRays<decltype(F)::value, decltype(G)::value, true>), grid, dim3(256), lds, s, b, (const float4*)rays, count, nullptr, nullptr, occluded, dm, rm);
        });
    } else {
        query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
            hipLaunchKernelGGL((k_traceRays<decltype(F)::value, decltype(G)::value, false>), grid, dim3(256), lds, s, b, (const float4*)rays, count, (float4*)hits, sets, nullptr, dm, rm);
        });
    }
}

// ---- ambient occlusion of the first hit (mirt_render_ao): the guides' primary ray and closest-hit stage, then `samples` hemisphere rays per
// casting sample through the any-hit loop above -- in one launch, nothing per ray in memory.  The definition is include/mirt.h's; the pieces are
// the pass's (primary_ray, closest_all with ClosestHooks as they stand, bounce_ray) and this file's rays_any, which is why the kernel lives here.
//
// Structure: k_guides' -- one lane per pixel, walking its samples in order, so every k x k count works with no segment plan -- and behind each
// sample's closest hit a loop of `samples` trips, a kernel argument and so WAVE-UNIFORM: in the grid variants every lane of the wave enters each
// shared-test walk of rays_any together (pt_trace_coop.hpp).  A lane whose sample did not cast rides along with a dead ray and counts nothing,
// like a lane without a pixel (nothing_to_do).  The optimistic / exact pair is per PIXEL (defer_unit): a pixel defers when the guard refuses one
// of its primary or AO rays or one of its walks defers.
// seeds: int32 per tile-local ray, read for the casting samples and never written.  ao_out: {open, cast} per tile-local pixel, one 8-byte store.
// Waves per SIMD the register allocator is held to (A/B switches; profiles/ao/README.md has the measurement).  Left alone the grid kernels take 126 to
// 129 VGPRs (the optimistic one 3 waves, a register over the fourth) and the single-cell ones 81 to 94 (5 waves); a lane here runs rpp * (1 + samples)
// rays back to back with nothing to overlap them but other waves, and more waves paid at every step tried, a few spilled registers included:
// cornell_teapot3 7.25 -> 5.99 (4 waves) -> 5.63 ms (5), cornell 2.29 -> 2.19 (6) -> 2.15 ms (7) at 1920 x 1080 x 16 with 4 AO rays.
// (PT_AO_GRID_WAVES 5, PT_AO_CELL_WAVES 7: pt_rays_guard.hpp, where the batch's translation unit finds them too)
#define PT_AO_BOUNDS(GRIDS) __launch_bounds__(256, (GRIDS) ? PT_AO_GRID_WAVES : PT_AO_CELL_WAVES)
template <bool FAST, int GRIDS>
__global__ void PT_AO_BOUNDS(GRIDS) k_ao(const FusedArgs A, uint32_t samples, float radius, float bias, uint2* __restrict__ ao_out, uint32_t* defer_mask,
                                            const uint32_t* redo_mask) {
    stage_block<FAST, GRIDS>(A);
    const uint32_t npix = A.nrows * A.width;   // (a tile holds fewer than 2^32 rays: mirt_render_ao)
    uint32_t pix = blockIdx.x * 256u + threadIdx.x;
    const bool valid = unit_valid<FAST>(pix, npix, redo_mask);
    if (nothing_to_do<GRIDS>(valid)) return;
    if (pix >= npix) pix = npix - 1u;
    const int32_t* __restrict__ seeds = A.seeds;
    uint32_t open = 0u, cast = 0u;
    bool defer = false;
    const uint32_t first = pix * A.rpp;
    for (uint32_t i = 0; i < A.rpp; ++i) {
        Ray ray = primary_ray(A, first + i);
        if (!valid) { ray.mint = 0.0f; ray.maxt = 0.0f; }   // rides along dead: hits nothing, casts nothing
        Poi poi = fresh_poi();
        closest_all<FAST, GRIDS>(A, ray, poi, ClosestHooks{}, defer);
        const bool casts = poi.matId >= 0;   // bouncePaths' own test (code.cl:592): no material is read
        int32_t seed = 0;
        if (casts) seed = seeds[first + i];
        for (uint32_t j = 0; j < samples; ++j) {
            Ray sh = dead_ray();
            if (casts) {
                sh = bounce_ray(poi, seed);   // getHemisphereRay (code.cl:545-579): the seed advances, in its register only
                if (bias != 0.0f) sh.o = add3(poi.p, scl3(bias, poi.n));   // two fp32 operations, each rounded on its own (-ffp-contract=off)
                sh.maxt = radius;
            }
            rays_any<FAST, GRIDS>(A, sh, defer);
            if (casts) {
                cast += 1u;
                if (!(sh.mint == sh.maxt)) open += 1u;
            }
        }
    }
    if (!valid) return;
    if (FAST && defer) { defer_unit(defer_mask, pix); return; }
    ao_out[pix] = make_uint2(open, cast);
}

// fast / defer_mask / redo_mask: query_dispatch's (pt_closest.hpp), a bit per pixel of the tile
void launch_ao(hipStream_t s, const FusedArgs& a, bool fast, uint32_t samples, float radius, float bias, void* ao_out, uint32_t* defer_mask, const uint32_t* redo_mask) {
    if (!a.nrows || !a.width) return;
    FusedArgs b = a;
    const dim3 grid((unsigned)(((uint64_t)b.nrows * b.width + 255u) / 256u));
    query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
        hipLaunchKernelGGL((k_ao<decltype(F)::value, decltype(G)::value>), grid, dim3(256), lds, s, b, samples, radius, bias, (uint2*)ao_out, dm, rm);
    });
}

// ---- path radiance of caller-supplied rays (mirt_trace_radiance): the pass's path -- closest hit, lightRender, then per segment the per-light
// shadow stage and shade, bouncePaths between the segments -- started at the CALLER's ray instead of initTrace's, `samples` times per ray, in one
// launch.  The definition is include/mirt.h's: executeRender (A10 code.js:1806-1854) without initTrace and copyToPixel.  The pieces are the pass's:
// closest_all (with this file's guard and the division kept in the loop: a caller's d is not of unit length), the lightRender loop as k_fusedPass
// states it (and k_viewPass below, verbatim), direct_all with the park rows (pt_direct.hpp), bounce_ray.
//
// Structure: one lane per ray; two float4 loads per sample for the ray (they hit the cache after the first; held in registers across the path they
// were eight more live VGPRs), the seed and, with MIRT_RADIANCE_ACCUMULATE, the accumulator once; one float4 store and one seed store.  `samples`,
// the bounce count and the flags are kernel arguments and so WAVE-UNIFORM: in the grid variants every lane of a wave enters every shared-test walk
// together (pt_trace_coop.hpp).  A lane that rides along dead (nothing_to_do) hits nothing, so it shades and bounces nothing.  The optimistic /
// exact pair is per RAY (defer_wave): a ray defers when the guard refuses its primary, a shadow or a bounce ray in any sample or one of its
// walks defers; neither its seed nor its accumulator is written, and the exact kernel redoes it from the start, all samples.
// Not built: samples after the first reusing the primary ray's closest hit and lightRender verdict (k_fusedPass's MULTI 2 does it for the camera).
// Waves per SIMD the register allocator is held to, A/B switches like k_ao's (profiles/radiance/README.md has the registers per instance and the
// measurement).  A lane runs samples * (1 + bounces) segments back to back with nothing to overlap them but other waves, and more waves paid at
// every step measured, the spilled registers included: at 1920 x 1080 x 4 rays, bounces 5, cornell_teapot3 6.44 (4 waves, 107 VGPRs) -> 5.49 (5,
// 96 VGPRs) -> 5.08 ms (6, 80 VGPRs, 16 to 20 spilled), cornell 1.29 (5 waves) -> 1.21 (6) -> 1.14 (7, 72 VGPRs, 2 to 8 spilled) -> 1.15 ms (8).
// (PT_RADIANCE_GRID_WAVES, PT_RADIANCE_CELL_WAVES, PT_RADIANCE_BOUNDS and RadiancePark: pt_rays_guard.hpp)
constexpr uint32_t kRadianceAccumulate = 1u, kRadianceNoEmitters = 2u;   // MIRT_RADIANCE_ACCUMULATE, MIRT_RADIANCE_NO_EMITTERS (include/mirt.h)
template <bool FAST, int GRIDS>
__global__ void PT_RADIANCE_BOUNDS(GRIDS) k_traceRadiance(const FusedArgs A, const float4* __restrict__ rays, uint32_t count, uint32_t samples, uint32_t flags,
                                                           int32_t* __restrict__ seeds, float4* __restrict__ radiance, uint32_t* defer_mask, const uint32_t* redo_mask) {
    stage_block<FAST, GRIDS>(A);
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;   // (count <= 2^32 - 256: mirt_trace_radiance)
    const bool valid = unit_valid<FAST>(id, count, redo_mask);
    if (nothing_to_do<GRIDS>(valid)) return;
    int32_t seed = 0;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // initAcu (A10 code.cl:448-456)
    if (valid) {
        seed = seeds[id];
        if (flags & kRadianceAccumulate) acc = radiance[id];
    }
    RadiancePark park;
#if PT_PARK_LDS
    __shared__ __attribute__((aligned(16))) float park_mem[PT_PARK_WORDS(GRIDS)][256];
    park.base = &park_mem[0][threadIdx.x];
    park.put(0, acc.x); park.put(1, acc.y); park.put(2, acc.z); park.put(3, acc.w);
#endif
    bool defer = false;
    for (uint32_t j = 0; j < samples; ++j) {
        Ray ray = dead_ray();
        if (valid) {
            const float4 a = rays[2u * (size_t)id], b = rays[2u * (size_t)id + 1u];
            ray.o = mk3(a.x, a.y, a.z); ray.mint = a.w;
            ray.d = mk3(b.x, b.y, b.z); ray.maxt = b.w;
        }
        Poi poi = fresh_poi();
#if PT_PARK_LDS
        park.put(4, 1.0f); park.put(5, 1.0f); park.put(6, 1.0f);   // every sample's path starts unattenuated; the accumulator goes on
#endif
        // segment 0 is the caller's ray; segments 1..bounces start with bouncePaths (code.js:1829-1846)
        for (uint32_t seg = 0; seg <= A.bounces; ++seg) {
            if (seg > 0) {
                if (poi.matId >= 0) {
#if PT_PARK_LDS
                    if (PT_PARK_PN_FOR(GRIDS)) park.get_pn(poi);
#endif
                    ray = bounce_ray(poi, seed);
                } else {
                    ray.mint = PT_INF;
                    ray.maxt = PT_INF;
                }
            }
            closest_all<FAST, GRIDS>(A, ray, poi, park, defer);
            if (seg == 0 && !(flags & kRadianceNoEmitters)) {
                for (uint32_t l = 0; l < A.n_lights; ++l) {  // lightRender (code.cl:600-629), on the caller's ray only
                    if (ray.mint == ray.maxt) continue;
                    const LightArgs& L = A.lights[l];
                    f3 irr = norm3(ld3(L.light + 6));
                    if (!light_visible(ray, ld3(L.light), ld3(L.light + 3), L.light[9])) continue;
                    ray.mint = PT_INF;
                    ray.maxt = PT_INF;
                    poi.matId = -1;
#if PT_PARK_LDS
                    park.acc_add(irr.x, irr.y, irr.z);
#else
                    acc.x += irr.x; acc.y += irr.y; acc.z += irr.z; acc.w += 1.0f;
#endif
                }
            }
            direct_all<FAST, GRIDS>(A, poi, seed, acc, park, defer);
        }
    }
    if (FAST) defer_wave(defer_mask, id, valid, defer);
    if (!valid || (FAST && defer)) return;   // the exact kernel redoes a deferred ray: nothing of it is written
    seeds[id] = seed;
#if PT_PARK_LDS
    acc = make_float4(park.get(0), park.get(1), park.get(2), park.get(3));
#endif
    radiance[id] = acc;
}

// fast / defer_mask / redo_mask: query_dispatch's (pt_closest.hpp), a bit per ray
void launch_radiance(hipStream_t s, const FusedArgs& a, bool fast, const void* rays, uint32_t count, uint32_t samples, uint32_t flags, int32_t* seeds, void* radiance,
                     uint32_t* defer_mask, const uint32_t* redo_mask) {
    if (!count) return;
    FusedArgs b = a;
    b.rpp = 1u;   // stage_block: no lens table
    const dim3 grid((unsigned)(((uint64_t)count + 255u) / 256u));
    query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
        hipLaunchKernelGGL((k_traceRadiance<decltype(F)::value, decltype(G)::value>), grid, dim3(256), lds, s, b, (const float4*)rays, count, samples, flags, seeds,
                           (float4*)radiance, dm, rm);
    });
}

// ---- panoramic, fisheye and orthographic cameras (mirt_view_rays, mirt_render_view): the ray of a sample is pt_view.hpp's view_ray, the one
// definition both kernels call; include/mirt.h defines it operation by operation.
}  // namespace pt
#include "pt_view_pass.hpp"   // the launch bounds and set-up that k_viewRays / k_viewPass share with the batch's translation unit
namespace pt {
// k_viewRays, k_viewPass: the single calls' kernels -- the text of pt_view_kernels.inc at BATCH false (the batch calls' are in
// pt_kernels_view_batch.hip)
#define PT_VIEW_BATCH false
#define PT_VIEW_ARGS ViewArgs
#define PT_VIEW_RAYS_KERNEL k_viewRays
#define PT_VIEW_PASS_TEMPLATE template <bool FAST, int GRIDS, bool GUIDES = false>
#define PT_VIEW_PASS_KERNEL k_viewPass
#include "pt_view_kernels.inc"
void launch_viewRays(hipStream_t s, const ViewArgs& v, void* rays) {
    const uint64_t count = view_pass_rays(v);
    if (!count) return;
    hipLaunchKernelGGL(k_viewRays, dim3((unsigned)((count + 255u) / 256u)), dim3(256), 0, s, v, (uint32_t)count, (float4*)rays);
}

// fast / defer_mask / redo_mask: query_dispatch's (pt_closest.hpp), a bit per BLOCK of the launch.  a.guide_nh / a.guide_ad (either given): the
// GUIDES instances, which the caller asks for at rpp 1, 4, 16 or 64 only.
void launch_viewPass(hipStream_t s, const FusedArgs& a, const ViewArgs& v, bool fast, bool accumulate, int32_t* seeds, void* radiance, void* pixel, float tone,
                     uint32_t* defer_mask, const uint32_t* redo_mask) {
    const uint64_t count = view_pass_rays(v);
    if (!count) return;
    FusedArgs b = view_pass_args(a, v, accumulate);
    const dim3 grid((unsigned)((count + 255u) / 256u));
    query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
        constexpr bool FAST = decltype(F)::value;
        constexpr int GRIDS = decltype(G)::value;
        if (b.guide_nh || b.guide_ad) hipLaunchKernelGGL((k_viewPass<FAST, GRIDS, true>), grid, dim3(256), lds, s, b, v, (uint32_t)count, seeds, (float4*)radiance, (uchar4*)pixel, tone, dm, rm);
        else hipLaunchKernelGGL((k_viewPass<FAST, GRIDS>), grid, dim3(256), lds, s, b, v, (uint32_t)count, seeds, (float4*)radiance, (uchar4*)pixel, tone, dm, rm);
    });
}

// ---- first-hit guides of a view camera's tile (mirt_view_guides): k_guides (pt_kernels_guides.hip) with the ray of a sample made by view_ray
// instead of primary_ray.  The definition is include/mirt.h's: pixel p has the rays p * rpp + i in sample order, exactly as k_viewRays writes
// them; each runs through closest_all as k_traceRays runs a caller's ray (this file's guard, the division kept in the loop: a view ray's d is the
// caller's basis as given, not of unit length); a sample is a hit iff 0 <= Poi.matId < A.nmat.
// Structure: k_guides' -- one lane per pixel walking its samples in order, the eight sums in registers, no barrier behind the prologue.  V is a
// kernel argument: the model's branch is WAVE-UNIFORM, and a DEAD fisheye sample (r > 1) rides through the shared walk as a dead ray and is never
// a hit.  In the grid variants a lane past the end of the tile rides along (nothing_to_do) on the last pixel (clamped).  The optimistic / exact
// pair is per PIXEL (defer_unit): a pixel defers when the ray-side guard refuses one of its samples (it goes on dead, guard_or_retire) or one of
// its walks defers.
// k_viewGuides, k_viewAo: the single calls' kernels -- the text of pt_view_aov_kernels.inc at BATCH false (the batch calls' are in
// pt_kernels_view_batch.hip)
#define PT_VIEW_RAY view_ray
#define PT_VIEW_GUIDES_KERNEL k_viewGuides
#define PT_VIEW_AO_KERNEL k_viewAo
#include "pt_view_aov_kernels.inc"

// fast / defer_mask / redo_mask: query_dispatch's (pt_closest.hpp), a bit per pixel of the tile.  Either output may be null.
// blocks: ceil(pixels / 256), the plan's (pt_view_plan.hpp).
void launch_viewGuides(hipStream_t s, const FusedArgs& a, const ViewArgs& v, uint32_t blocks, bool fast, void* normal_hits, void* albedo_depth, uint32_t* defer_mask,
                       const uint32_t* redo_mask) {
    if (!blocks) return;
    FusedArgs b = a;
    b.width = v.width; b.nrows = v.nrows;
    b.rpp = v.k * v.k;   // stage_block, as launch_viewPass sets it (the lens table of it is k words nobody reads)
    query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
        hipLaunchKernelGGL((k_viewGuides<decltype(F)::value, decltype(G)::value>), dim3(blocks), dim3(256), lds, s, b, v, (float4*)normal_hits, (float4*)albedo_depth, dm, rm);
    });
}

// ---- ambient occlusion of a view camera's tile (mirt_view_ao): k_ao with the ray of a sample made by view_ray instead of primary_ray, and so
// through closest_all with ViewGuideHooks (a view ray's d is not of unit length); behind each sample's closest hit k_ao's own `samples` trips of
// bounce_ray + rays_any, stated here a second time: a device function shared with k_ao re-allocated k_ao's registers (spill offsets and
// scalar loads moved in all six instances), and that kernel's rule is identical code.  A change to one is a change to both.  The definition is
// include/mirt.h's.
// Structure: k_ao's and k_viewGuides' -- one lane per pixel walking its samples in order; V and `samples` are kernel arguments, so the model's
// branch and the trip count are WAVE-UNIFORM.  A DEAD fisheye sample, a sample the guard retired and a lane that rides along (nothing_to_do; on
// the clamped last pixel when it is past the tile) go on with a dead ray: they hit nothing, cast nothing and count nothing.  The optimistic /
// exact pair is per PIXEL (defer_unit): a pixel defers when the guard refuses one of its view or AO rays or one of its walks defers.
// seeds: int32 per tile-local ray, read for the casting samples and never written.  ao_out: {open, cast} per tile-local pixel, one 8-byte store.
// Waves per SIMD the register allocator is held to: A/B switches of this kernel's own, starting from k_ao's (profiles/view_ao/README.md has the
// registers per instance and the measurement).  At 1920 x 1080 x 4 with 4 AO rays on cornell_teapot3, equirect / oblique orthographic: 2.39 / 1.79 ms
// (4 waves) -> 2.22 / 1.77 (5) -> 2.22 / 1.85 (6): the bounds stay k_ao's.
// fast / defer_mask / redo_mask: query_dispatch's (pt_closest.hpp), a bit per pixel of the tile.  blocks: ceil(pixels / 256), the plan's
// (pt_view_plan.hpp).
void launch_viewAo(hipStream_t s, const FusedArgs& a, const ViewArgs& v, uint32_t blocks, bool fast, uint32_t samples, float radius, float bias, const int32_t* seeds,
                   void* ao_out, uint32_t* defer_mask, const uint32_t* redo_mask) {
    if (!blocks) return;
    FusedArgs b = a;
    b.width = v.width; b.nrows = v.nrows;
    b.rpp = v.k * v.k;   // stage_block, as launch_viewGuides sets it
    query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
        hipLaunchKernelGGL((k_viewAo<decltype(F)::value, decltype(G)::value>), dim3(blocks), dim3(256), lds, s, b, v, samples, radius, bias, seeds, (uint2*)ao_out, dm, rm);
    });
}

}  // namespace pt
