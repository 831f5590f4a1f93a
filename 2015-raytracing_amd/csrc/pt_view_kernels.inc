// pt_view_kernels.inc -- the view cameras' ray and frame kernels, ONE text for two translation units.  The includer defines
//   PT_VIEW_BATCH          false / true: the compile-time flag of both kernels (view_ray<PT_VIEW_BATCH>)
//   PT_VIEW_ARGS           ViewArgs / ViewBatchArgs
//   PT_VIEW_RAYS_KERNEL    k_viewRays / k_viewRaysBatch
//   PT_VIEW_PASS_TEMPLATE  template <bool FAST, int GRIDS, bool GUIDES = false>, in both
//   PT_VIEW_PASS_KERNEL    k_viewPass / k_viewPassBatch
// pt_kernels_rays.hip includes it with the first of each (the single calls: mirt_view_rays, mirt_render_view, mirt_render_view_guided) and gets,
// token for token, the kernels it had before there was a batch; pt_kernels_view_batch.hip includes it with the second.  Text and not a shared
// device function: a kernel that only calls a force-inlined body came out of hipcc with other code than the kernel itself (k_viewPass's twelve
// instances by -36 to +136 bytes each), and the single calls' kernels keep theirs byte for byte -- and, in a code object without the batch's
// kernels, their addresses (profiles/view_batch/README.md).
// k_viewRays: the rays as 32-byte records, one lane per ray, two float4 stores -- memory-bound, nothing else to it.
// BATCH (mirt_view_rays_batch): the rays of V.nrows / V.frame_rows stacked frames, each lane's camera from the table (pt_view.hpp view_ray).
__global__ void __launch_bounds__(256) PT_VIEW_RAYS_KERNEL(const PT_VIEW_ARGS V, uint32_t count, float4* __restrict__ rays) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;   // (count <= 2^32 - 256: pt_view_plan.hpp)
    if (id >= count) return;
    const Ray r = view_ray<PT_VIEW_BATCH>(V, id);
    rays[2u * (size_t)id] = make_float4(r.o.x, r.o.y, r.o.z, r.mint);
    rays[2u * (size_t)id + 1u] = make_float4(r.d.x, r.d.y, r.d.z, r.maxt);
}

// k_viewPass: k_traceRadiance's body at one sample per ray with the ray made in registers by view_ray instead of loaded, and behind the block's
// barrier the pass's own resolve (pt_resolve.hpp resolve_rows) -- in one launch; neither the rays nor the per-ray accumulators reach memory.
// A.rpp = A.seg_len = k * k (1, 4, 16, 64 or 256: it divides 256, so a block of 256 consecutive ray ids holds 256 / rpp WHOLE pixels) and
// A.seg_off != 0 iff the sums go on from `radiance` (MIRT_VIEW_ACCUMULATE: resolve_rows' carry); A.width / A.nrows are the tile's.
//
// Structure: one lane per ray.  The generator's registers are dead before the segment loop; the four accumulator words are parked as
// [channel][lane] rows from the start (they begin at +0: ACCUMULATE is the resolve's business, not the ray's) and read by the resolve where they
// lie.  Every lane stays to the barrier, so the prologue is the block's own, not unit_valid / nothing_to_do: a lane past the end of the tile
// rides along dead (dead_ray) -- it hits nothing, shades nothing, draws nothing.
// The model, the bounce count and the sizes are kernel arguments and so WAVE-UNIFORM: in the grid variants every lane of a wave enters every
// shared-test walk together (pt_trace_coop.hpp).
// The optimistic / exact pair is per BLOCK, as in the pass's in-block resolve: a block one of whose primary, shadow or bounce rays the guard
// refuses, or one of whose walks defers, writes neither its seeds nor its pixels and sets its bit (a bit per block of the launch); the exact
// kernel runs the same grid and every block without its bit leaves at once.  An ORTHOGRAPHIC camera whose `forward` has a zero component is
// outside the ray-side guard for EVERY ray (|d_k| >= 2^-40): every block is handed over and the frame comes from the exact kernel, same bits.
// Waves per SIMD the register allocator is held to: A/B switches of this kernel's own, starting from k_traceRadiance's (profiles/view/README.md
// has the registers per instance and the measurement).  At 1920 x 1080 x 4 rays, bounces 5, equirect: cornell_teapot3 5.57 (5 waves, 96 VGPRs, no
// spill) -> 5.20 (6, 80 VGPRs, 17 spilled) -> 5.47 (7) -> 6.90 ms (8 waves, 64 VGPRs, 51 spilled), cornell 1.01 (5 waves) -> 1.00 (6) -> 0.97 (7) -> 0.97 ms (8):
// the bounds stay k_traceRadiance's.
// GUIDES (mirt_render_view_guided, the one-launch route: pt_view_plan.hpp view_guides_in_pass): the frame writes the first-hit guides of its
// pixels too, A.guide_nh / A.guide_ad, by the pass's own lane walk (pt_resolve.hpp guides_emit) right after segment 0's closest_all -- the state
// k_viewGuides takes them at, reached by the same functions on the same ray ids.  rpp is 1, 4, 16 or 64: a pixel's samples are consecutive lanes
// of one wave.  As in the pass, the optimistic kernel writes a block's guides before its verdict; a block that defers is re-run whole by the
// exact kernel, which writes the same pixels' guides again, later on the same stream.  The default, false, keeps the unguided instances' code.
// BATCH (mirt_render_view_batch): N cameras' frames of one size stacked into one image of N * height rows.  Only the ray differs -- each lane
// loads its frame's camera from the table V.cameras (view_ray<true>), twelve registers that are dead before the segment loop like the rest of
// the generator's.  A frame's rays are a multiple of rpp, so a block still holds whole pixels, possibly of two frames: the resolve, the
// per-block verdict and the redo pass see an image of width x (N * height) and need nothing new -- nor does GUIDES (mirt_render_view_guided_batch):
// guides_emit's pixel index is tile-local in the stacked image.
PT_VIEW_PASS_TEMPLATE
__global__ void PT_VIEW_BOUNDS(GRIDS) PT_VIEW_PASS_KERNEL(const FusedArgs A, const PT_VIEW_ARGS V, uint32_t count, int32_t* __restrict__ seeds, float4* radiance,
                                                   uchar4* __restrict__ pixel, float tone, uint32_t* defer_mask, const uint32_t* redo_mask) {
    const uint32_t blk = blockIdx.x;
    if (!FAST && redo_mask && (redo_mask[blk >> 5] >> (blk & 31u) & 1u) == 0u) return;   // block-uniform: nothing of the block has begun
    stage_block<FAST, GRIDS>(A);
    const uint32_t id = blk * 256u + threadIdx.x;   // (count <= 2^32 - 256: pt_view_plan.hpp)
    const bool valid = id < count;
    int32_t seed = 0;
    Ray ray = dead_ray();
    if (valid) {
        seed = seeds[id];
        ray = view_ray<PT_VIEW_BATCH>(V, id);
    }
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // initAcu (A10 code.cl:448-456)
    RadiancePark park;
#if PT_PARK_LDS
    __shared__ __attribute__((aligned(16))) float park_mem[PT_PARK_WORDS(GRIDS)][256];
    park.base = &park_mem[0][threadIdx.x];
    park.put(0, 0.0f); park.put(1, 0.0f); park.put(2, 0.0f); park.put(3, 0.0f);
    park.put(4, 1.0f); park.put(5, 1.0f); park.put(6, 1.0f);
#else
    __shared__ __attribute__((aligned(16))) float park_mem[4][256];
#endif
    bool defer = false;
    Poi poi = fresh_poi();
    // segment 0 is the camera's ray; segments 1..bounces start with bouncePaths (code.js:1829-1846)
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
        if constexpr (GUIDES) if (seg == 0) guides_emit(A, ray, poi, valid, blk);   // every lane of the block is here: none leaves before the barrier
        if (seg == 0) {
            for (uint32_t l = 0; l < A.n_lights; ++l) {  // lightRender (code.cl:600-629), on the camera's ray only
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
#if !PT_PARK_LDS
    park_mem[0][threadIdx.x] = acc.x; park_mem[1][threadIdx.x] = acc.y; park_mem[2][threadIdx.x] = acc.z; park_mem[3][threadIdx.x] = acc.w;
#endif
    if (FAST && valid && defer) pt_blk_defer[0] = 1u;
    __syncthreads();   // every lane's accumulator is final in LDS, and so is the flag (stage_block cleared it)
    if (FAST && pt_blk_defer[0] != 0u) {   // the whole block goes to the exact kernel: its seeds stay as they were, no pixel of it is written
        if (threadIdx.x == 0u) defer_unit(defer_mask, blk);
        return;
    }
    if (valid) seeds[id] = seed;
    resolve_rows(A, &park_mem[0][0], blk, count, (const float*)radiance, radiance, pixel, tone);
}
