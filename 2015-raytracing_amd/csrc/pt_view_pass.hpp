// pt_view_pass.hpp -- what the two translation units of the view cameras' ray and frame kernels share beside the kernels' text
// (pt_view_kernels.inc): the headers that text needs, the launch bounds, and the launch set-up of a frame's pair.  pt_kernels_rays.hip has the
// single calls' kernels, pt_kernels_view_batch.hip the batch calls'.
#pragma once
#include "pt_rays_guard.hpp"
#include "pt_resolve.hpp"   // resolve_rows: k_viewPass resolves its blocks' pixels as the pass does; guides_emit: its GUIDES instances write the guides
#include "pt_view.hpp"      // view_ray: a sample's ray

namespace pt {

// Waves per SIMD the register allocator is held to in k_viewPass: the measurement is at the kernel (pt_view_kernels.inc)
#ifndef PT_VIEW_GRID_WAVES
#define PT_VIEW_GRID_WAVES PT_RADIANCE_GRID_WAVES
#endif
#ifndef PT_VIEW_CELL_WAVES
#define PT_VIEW_CELL_WAVES PT_RADIANCE_CELL_WAVES
#endif
#define PT_VIEW_BOUNDS(GRIDS) __launch_bounds__(256, (GRIDS) ? PT_VIEW_GRID_WAVES : PT_VIEW_CELL_WAVES)

// The launch of a frame's pair, the part both translation units share: the rays of the launch, and the pass's arguments as resolve_rows reads them
inline uint64_t view_pass_rays(const ViewArgs& v) { return (uint64_t)v.nrows * v.width * v.k * v.k; }
inline FusedArgs view_pass_args(const FusedArgs& a, const ViewArgs& v, bool accumulate) {
    FusedArgs b = a;
    b.width = v.width; b.nrows = v.nrows;
    b.rpp = v.k * v.k;            // resolve_rows: the rays of a pixel (stage_block's lens table of it is k words nobody reads)
    b.seg_len = b.rpp;            // ... all of them in one block
    b.seg_off = accumulate ? 1u : 0u;   // ... and whether the chain goes on from the carry
    return b;
}

}  // namespace pt
