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

// redo_mask (exact kernel only): a bit per pixel of the tile, the pixels the optimistic kernel handed over; null: every pixel.
// GRIDS: the walk shares its tests across the wave (pt_trace_coop.hpp), so a lane without a pixel of its own rides along and writes nothing.
template <bool FAST, int GRIDS>
__global__ void __launch_bounds__(256) k_guides(const FusedArgs A, float4* normal_hits, float4* albedo_depth, uint32_t* defer_mask, const uint32_t* redo_mask) {
    stage_block<FAST, GRIDS>(A);
    const uint32_t npix = A.nrows * A.width;   // (a tile holds fewer than 2^32 rays: mirt_render_guides)
    uint32_t pix = blockIdx.x * 256u + threadIdx.x;
    bool valid = pix < npix;
    if (!FAST && redo_mask && valid) valid = (redo_mask[pix >> 5] >> (pix & 31u) & 1u) != 0u;
    if (GRIDS) { if (__builtin_amdgcn_ballot_w64(valid) == 0ull) return; }
    else if (!valid) return;
    if (pix >= npix) pix = npix - 1u;
    const float4* material = (const float4*)A.material;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, hits = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f, depth = 0.0f;
    bool defer = false;
    const uint32_t first = pix * A.rpp;
    for (uint32_t i = 0; i < A.rpp; ++i) {
        Ray ray = primary_ray(A, first + i);
        Poi poi;
        poi.p = mk3(0.0f, 0.0f, 0.0f);
        poi.n = mk3(0.0f, 0.0f, 0.0f);
        poi.atte = mk3(1.0f, 1.0f, 1.0f);
        poi.matId = -1;
        closest_all<FAST, GRIDS>(A, ray, poi, ClosestHooks{}, defer);   // the pass parks the vertex for its shadow stage: nothing comes after it here
        if (poi.matId < 0 || (uint32_t)poi.matId >= A.nmat) continue;
        const float4 c = material[poi.matId];
        nx += poi.n.x; ny += poi.n.y; nz += poi.n.z; hits += 1.0f;
        ar += c.x; ag += c.y; ab += c.z; depth += ray.maxt;
    }
    if (!valid) return;
    if (FAST && defer) {   // the exact kernel redoes the pixel: nothing of it is written
        atomicOr(&defer_mask[pix >> 5], 1u << (pix & 31u));
        return;
    }
    if (normal_hits) normal_hits[pix] = make_float4(nx, ny, nz, hits);
    if (albedo_depth) albedo_depth[pix] = make_float4(ar, ag, ab, depth);
}

template <bool FAST>
static void launch_guides_t(hipStream_t s, const FusedArgs& b, const FusedLds& L, float4* nh, float4* ad, uint32_t* defer_mask, const uint32_t* redo_mask) {
    const dim3 grid((unsigned)(((uint64_t)b.nrows * b.width + 255u) / 256u));
    fused_lds_dispatch(L, [&](auto G, size_t lds) { hipLaunchKernelGGL((k_guides<FAST, decltype(G)::value>), grid, dim3(256), lds, s, b, nh, ad, defer_mask, redo_mask); });
}
// fast: the optimistic kernel (sets the deferred pixels' bits in defer_mask, one per pixel of the tile); !fast: the exact kernel over the pixels
// of redo_mask, or over every pixel when it is null.  Either output may be null.
void launch_guides(hipStream_t s, const FusedArgs& a, bool fast, void* normal_hits, void* albedo_depth, uint32_t* defer_mask, const uint32_t* redo_mask) {
    if (!a.nrows || !a.width) return;
    FusedArgs b = a;
    const FusedLds L = fused_lds_slots(b, fast);
    if (fast) launch_guides_t<true>(s, b, L, (float4*)normal_hits, (float4*)albedo_depth, defer_mask, nullptr);
    else launch_guides_t<false>(s, b, L, (float4*)normal_hits, (float4*)albedo_depth, nullptr, redo_mask);
}

}  // namespace pt
