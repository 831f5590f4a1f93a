// pt_kernels_guides.hip -- first-hit guide buffers of the Assign10 pass (mirt_render_guides): per pixel, the sums over its primary rays of the
// surface normal, the material colour and the hit distance, and the number of rays that hit -- what a denoiser or an a-trous filter behind a
// few-rays-per-pixel frame is guided by.
//
// Definition.  Pixel p of the row tile has the rays pixel * rpp + i, i = 0 .. rpp - 1, the order copyToPixel adds them in (A10 code.cl:1377-1380).
// Each is taken as initTrace (code.cl:458-543) and the closest-hit stage leave it -- sphereTrace, triangleTrace, every meshTrace in upload order
// (code.js:1809-1813) -- BEFORE lightRender and before any shading.  A sample is a HIT when that stage leaves a live vertex, by the reference's own
// test: initTrace resets every Poi to matId = -1 (code.cl:538-541), only a closest-hit kernel that found a primitive stores an id (code.cl:797,
// 932, 1067), and sceneRender shades a vertex iff poi.matId >= 0 (code.cl:1336).  An id past the material table is not a hit and nothing is read
// for it (hazard 6: material[matId] would be a foreign read).
//   normal_hits [p] = (sum Poi.normal.x, sum .y, sum .z, hits)                     hits: the number of hit samples, as a float
//   albedo_depth[p] = (sum material[matId].x, sum .y, sum .z, sum Ray.maxt)
// each a sequential fp32 sum from +0 over the HIT samples in sample order, un-normalised like `radiance`.  The guides describe SURFACES: an
// emitter in front of the surface (lightRender, code.cl:600-629, kills such a ray afterwards) is not considered.
//
// The bits are the fused pass's by construction: primary_ray, stage_block and closest_all are the pass's own functions (pt_closest.hpp; the loop over
// the sets is defined there once, and this kernel adds nothing to it: ClosestHooks as they stand), the sets get the LDS slots the pass gives them
// and the kernel instance those call for (fused_lds_slots, fused_lds_dispatch), and the optimistic / exact pair is the pass's -- here per PIXEL: a pixel one of whose
// samples left the guard windows sets its bit and writes nothing, the exact kernel redoes the marked pixels whole.
//
// Structure: one lane per pixel, walking its samples in order.  Every k x k count works the same way -- no segment plan, no carried sums, no
// barrier behind the prologue -- and the sum's order is the loop's.  The 64 lanes of a wave are 64 neighbouring pixels on the same lens sample: as
// coherent as the pass's 64 samples of one pixel for the shared-test walk.
#include "pt_closest.hpp"

namespace pt {

// defer_mask / redo_mask: a bit per pixel of the tile.  Which lane has a pixel of its own, which lane may leave and how a deferred pixel is handed
// over are the query kernels' common rules (pt_closest.hpp: unit_valid, nothing_to_do, defer_unit); a lane that rides along does so on the
// clamped last pixel.
template <bool FAST, int GRIDS>
__global__ void __launch_bounds__(256) k_guides(const FusedArgs A, float4* normal_hits, float4* albedo_depth, uint32_t* defer_mask, const uint32_t* redo_mask) {
    stage_block<FAST, GRIDS>(A);
    const uint32_t npix = A.nrows * A.width;   // (a tile holds fewer than 2^32 rays: mirt_render_guides)
    uint32_t pix = blockIdx.x * 256u + threadIdx.x;
    const bool valid = unit_valid<FAST>(pix, npix, redo_mask);
    if (nothing_to_do<GRIDS>(valid)) return;
    if (pix >= npix) pix = npix - 1u;
    const float4* material = (const float4*)A.material;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, hits = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, depth = 0.0f;
    bool defer = false;
    const uint32_t first = pix * A.rpp;
    for (uint32_t i = 0; i < A.rpp; ++i) {
        Ray ray = primary_ray(A, first + i);
        Poi poi = fresh_poi();
        closest_all<FAST, GRIDS>(A, ray, poi, ClosestHooks{}, defer);   // the pass parks the vertex for its shadow stage: nothing comes after it here
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

// fast / defer_mask / redo_mask: query_dispatch's (pt_closest.hpp), a bit per pixel of the tile.  Either output may be null.
void launch_guides(hipStream_t s, const FusedArgs& a, bool fast, void* normal_hits, void* albedo_depth, uint32_t* defer_mask, const uint32_t* redo_mask) {
    if (!a.nrows || !a.width) return;
    FusedArgs b = a;
    const dim3 grid((unsigned)(((uint64_t)b.nrows * b.width + 255u) / 256u));
    query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
        hipLaunchKernelGGL((k_guides<decltype(F)::value, decltype(G)::value>), grid, dim3(256), lds, s, b, (float4*)normal_hits, (float4*)albedo_depth, dm, rm);
    });
}

}  // namespace pt
