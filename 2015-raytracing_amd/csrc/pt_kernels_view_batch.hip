// pt_kernels_view_batch.hip -- the batched view cameras (mirt_view_rays_batch, mirt_render_view_batch, mirt_view_guides_batch,
// mirt_render_view_guided_batch, mirt_view_ao_batch; include/mirt.h): the text of pt_view_kernels.inc and of pt_view_aov_kernels.inc at
// BATCH true and k_viewCameras, which fills the camera table.  A translation unit of its own: its kernels
// go into a code object of their own and leave that of pt_kernels_rays.hip as it was.
#include "pt_view_pass.hpp"
#include <string.h>

namespace pt {

// k_viewCameras: a chunk of the batch's camera table from the kernel's own arguments to device memory, lane i the words i, i + 256, ...
struct ViewCameraChunk {
    float v[kViewCameraChunk * 12u];
};
__global__ void __launch_bounds__(256) k_viewCameras(const ViewCameraChunk c, uint32_t words, float* __restrict__ table) {
    for (uint32_t i = threadIdx.x; i < words; i += 256u) table[i] = c.v[i];   // (words <= kViewCameraChunk * 12: the launcher's)
}
void launch_viewCameras(hipStream_t s, const float* host_cameras, uint32_t n, float* table) {
    for (uint32_t first = 0; first < n; first += kViewCameraChunk) {
        const uint32_t count = n - first < kViewCameraChunk ? n - first : kViewCameraChunk;
        ViewCameraChunk c;
        memset(&c, 0, sizeof c);
        memcpy(c.v, host_cameras + (size_t)first * 12u, (size_t)count * 48u);
        hipLaunchKernelGGL(k_viewCameras, dim3(1), dim3(256), 0, s, c, count * 12u, table + (size_t)first * 12u);
    }
}
// k_viewRaysBatch, k_viewPassBatch: the text of pt_view_kernels.inc at BATCH true -- the rays and the frames of V.nrows / V.frame_rows stacked
// frames, each lane's camera from the table
#define PT_VIEW_BATCH true
#define PT_VIEW_ARGS ViewBatchArgs
#define PT_VIEW_RAYS_KERNEL k_viewRaysBatch
#define PT_VIEW_PASS_TEMPLATE template <bool FAST, int GRIDS, bool GUIDES = false>
#define PT_VIEW_PASS_KERNEL k_viewPassBatch
#include "pt_view_kernels.inc"
void launch_viewRaysBatch(hipStream_t s, const ViewBatchArgs& v, void* rays) {
    const uint64_t count = view_pass_rays(v);
    if (!count) return;
    hipLaunchKernelGGL(k_viewRaysBatch, dim3((unsigned)((count + 255u) / 256u)), dim3(256), 0, s, v, (uint32_t)count, (float4*)rays);
}

// fast / defer_mask / redo_mask: query_dispatch's, a bit per BLOCK of the launch.  a.guide_nh / a.guide_ad (either given): the GUIDES instances,
// which the caller asks for at rpp 1, 4, 16 or 64 only -- launch_viewPass's rule.
void launch_viewPassBatch(hipStream_t s, const FusedArgs& a, const ViewBatchArgs& v, bool fast, bool accumulate, int32_t* seeds, void* radiance, void* pixel, float tone,
                          uint32_t* defer_mask, const uint32_t* redo_mask) {
    const uint64_t count = view_pass_rays(v);
    if (!count) return;
    FusedArgs b = view_pass_args(a, v, accumulate);
    const dim3 grid((unsigned)((count + 255u) / 256u));
    query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
        constexpr bool FAST = decltype(F)::value;
        constexpr int GRIDS = decltype(G)::value;
        if (b.guide_nh || b.guide_ad) hipLaunchKernelGGL((k_viewPassBatch<FAST, GRIDS, true>), grid, dim3(256), lds, s, b, v, (uint32_t)count, seeds, (float4*)radiance, (uchar4*)pixel, tone, dm, rm);
        else hipLaunchKernelGGL((k_viewPassBatch<FAST, GRIDS>), grid, dim3(256), lds, s, b, v, (uint32_t)count, seeds, (float4*)radiance, (uchar4*)pixel, tone, dm, rm);
    });
}

// k_viewGuidesBatch, k_viewAoBatch: the text of pt_view_aov_kernels.inc at BATCH true -- the guides and the ambient occlusion of the stacked
// frames, one lane and one mask bit per pixel of the image of V.nrows = n_frames * height rows
#include "pt_rays_any.inc"
#define PT_VIEW_RAY view_ray<true>
#define PT_VIEW_GUIDES_KERNEL k_viewGuidesBatch
#define PT_VIEW_AO_KERNEL k_viewAoBatch
#include "pt_view_aov_kernels.inc"
// fast / defer_mask / redo_mask: query_dispatch's, a bit per pixel of the stacked image.  Either output may be null.  blocks: ceil(n_frames *
// pixels / 256), the plan's (pt_view_plan.hpp view_batch_pixel_plan).
void launch_viewGuidesBatch(hipStream_t s, const FusedArgs& a, const ViewBatchArgs& v, uint32_t blocks, bool fast, void* normal_hits, void* albedo_depth, uint32_t* defer_mask,
                            const uint32_t* redo_mask) {
    if (!blocks) return;
    FusedArgs b = a;
    b.width = v.width; b.nrows = v.nrows;
    b.rpp = v.k * v.k;   // stage_block, as launch_viewGuides sets it
    query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
        hipLaunchKernelGGL((k_viewGuidesBatch<decltype(F)::value, decltype(G)::value>), dim3(blocks), dim3(256), lds, s, b, v, (float4*)normal_hits, (float4*)albedo_depth, dm, rm);
    });
}
void launch_viewAoBatch(hipStream_t s, const FusedArgs& a, const ViewBatchArgs& v, uint32_t blocks, bool fast, uint32_t samples, float radius, float bias, const int32_t* seeds,
                        void* ao_out, uint32_t* defer_mask, const uint32_t* redo_mask) {
    if (!blocks) return;
    FusedArgs b = a;
    b.width = v.width; b.nrows = v.nrows;
    b.rpp = v.k * v.k;   // stage_block, as launch_viewAo sets it
    query_dispatch(b, fast, defer_mask, redo_mask, [&](auto F, auto G, size_t lds, uint32_t* dm, const uint32_t* rm) {
        hipLaunchKernelGGL((k_viewAoBatch<decltype(F)::value, decltype(G)::value>), dim3(blocks), dim3(256), lds, s, b, v, samples, radius, bias, seeds, (uint2*)ao_out, dm, rm);
    });
}

}  // namespace pt
