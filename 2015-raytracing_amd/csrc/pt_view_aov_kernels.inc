// pt_view_aov_kernels.inc -- the view cameras' first-hit guides and ambient occlusion kernels, ONE text for two translation units, as
// pt_view_kernels.inc is for the ray and frame kernels.  The includer defines, beside that file's PT_VIEW_ARGS (ViewArgs / ViewBatchArgs),
//   PT_VIEW_RAY             view_ray / view_ray<true>: a sample's ray (a name, so that the single calls' text keeps its tokens)
//   PT_VIEW_GUIDES_KERNEL   k_viewGuides / k_viewGuidesBatch
//   PT_VIEW_AO_KERNEL       k_viewAo / k_viewAoBatch
// and has included pt_rays_any.inc.  pt_kernels_rays.hip includes it with the first of each (mirt_view_guides, mirt_view_ao) and gets, token for
// token, the kernels it had before there was a batch of them; pt_kernels_view_batch.hip includes it with the second (mirt_view_guides_batch,
// mirt_view_ao_batch).  Text and not a shared device function, for pt_view_kernels.inc's reason and k_viewAo's own (below).
// BATCH: V.nrows = n_frames * height rows of stacked frames are ONE image -- one lane and one mask bit per pixel of it, a pixel's rpp samples
// all in one frame, each sample's camera loaded from the table by view_ray<true>.  Nothing else differs.
// The comments of the two kernels are at their launchers in pt_kernels_rays.hip.
struct ViewGuideHooks : ClosestHooks {
    PT_DEV void guard(Ray& ray, bool& defer) const { guard_or_retire(ray, defer); }
    PT_DEV void top(Ray& ray) const { keep_in_loop(ray); }
};
template <bool FAST, int GRIDS>
__global__ void __launch_bounds__(256) PT_VIEW_GUIDES_KERNEL(const FusedArgs A, const PT_VIEW_ARGS V, float4* normal_hits, float4* albedo_depth, uint32_t* defer_mask,
                                                    const uint32_t* redo_mask) {
    stage_block<FAST, GRIDS>(A);
    const uint32_t npix = V.nrows * V.width;   // (a tile holds at most 2^32 - 256 rays: pt_view_plan.hpp)
    uint32_t pix = blockIdx.x * 256u + threadIdx.x;
    const bool valid = unit_valid<FAST>(pix, npix, redo_mask);
    if (nothing_to_do<GRIDS>(valid)) return;
    if (pix >= npix) pix = npix - 1u;
    const float4* material = (const float4*)A.material;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, hits = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, depth = 0.0f;
    bool defer = false;
    const uint32_t rpp = V.k * V.k, first = pix * rpp;
    for (uint32_t i = 0; i < rpp; ++i) {
        Ray ray = PT_VIEW_RAY(V, first + i);
        Poi poi = fresh_poi();
        closest_all<FAST, GRIDS>(A, ray, poi, ViewGuideHooks{}, defer);
        if (poi.matId < 0 || (uint32_t)poi.matId >= A.nmat) continue;
        const float4 c = material[poi.matId];
        nx += poi.n.x; ny += poi.n.y; nz += poi.n.z; hits += 1.0f;
        ar += c.x; ag += c.y; ab += c.z; depth += ray.maxt;
    }
    if (!valid) return;
    if (FAST && defer) { defer_unit(defer_mask, pix); return; }
    if (normal_hits) normal_hits[pix] = make_float4(nx, ny, nz, hits);
    if (albedo_depth) albedo_depth[pix] = make_float4(ar, ag, ab, depth);
}

#ifndef PT_VIEW_AO_GRID_WAVES
#define PT_VIEW_AO_GRID_WAVES PT_AO_GRID_WAVES
#endif
#ifndef PT_VIEW_AO_CELL_WAVES
#define PT_VIEW_AO_CELL_WAVES PT_AO_CELL_WAVES
#endif
#define PT_VIEW_AO_BOUNDS(GRIDS) __launch_bounds__(256, (GRIDS) ? PT_VIEW_AO_GRID_WAVES : PT_VIEW_AO_CELL_WAVES)
template <bool FAST, int GRIDS>
__global__ void PT_VIEW_AO_BOUNDS(GRIDS) PT_VIEW_AO_KERNEL(const FusedArgs A, const PT_VIEW_ARGS V, uint32_t samples, float radius, float bias, const int32_t* __restrict__ seeds,
                                                    uint2* __restrict__ ao_out, uint32_t* defer_mask, const uint32_t* redo_mask) {
    stage_block<FAST, GRIDS>(A);
    const uint32_t npix = V.nrows * V.width;   // (a tile holds at most 2^32 - 256 rays: pt_view_plan.hpp)
    uint32_t pix = blockIdx.x * 256u + threadIdx.x;
    const bool valid = unit_valid<FAST>(pix, npix, redo_mask);
    if (nothing_to_do<GRIDS>(valid)) return;
    if (pix >= npix) pix = npix - 1u;
    uint32_t open = 0u, cast = 0u;
    bool defer = false;
    const uint32_t rpp = V.k * V.k, first = pix * rpp;
    for (uint32_t i = 0; i < rpp; ++i) {
        Ray ray = PT_VIEW_RAY(V, first + i);
        if (!valid) { ray.mint = 0.0f; ray.maxt = 0.0f; }   // rides along dead: hits nothing, casts nothing
        Poi poi = fresh_poi();
        closest_all<FAST, GRIDS>(A, ray, poi, ViewGuideHooks{}, defer);
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

