// pt_rays_guard.hpp -- what the kernels that start at a ray of any length share (pt_kernels_rays.hip, and the batched view cameras of
// pt_kernels_view_batch.hip): the division kept in the loop, the ray-side guard that retires a refused ray, and k_traceRadiance's park rows and
// launch bounds, which k_viewPass (pt_view_pass.hpp) takes over.  Inline device code only: a translation unit that includes it emits nothing.
#pragma once
#include "pt_direct.hpp"

namespace pt {

// The default contract only (libmirt_default.so).  The sphere stage's 1 / (2 d.d) depends on the ray alone, so the compiler moves it out of the
// loop over the sets -- and a division it moves loses the 2.5-ulp licence the build gives every division: it comes out correctly rounded, one
// ulp off the kernel-by-kernel path's (and the reference's default build's) v_rcp_f32 form wherever the two differ.  A camera's unit-length d
// never showed it (d.d is within an ulp of 1); a caller's d does.  An empty statement that "changes" d at the top of every trip keeps the
// division where it is written.  Not a run-time cost: the values stay in their registers.
PT_DEV void keep_in_loop(Ray& r) {
#if PT_PLAIN_DIV
    asm volatile("" : "+v"(r.d.x), "+v"(r.d.y), "+v"(r.d.z));
#endif
}

// The optimistic kernel's ray-side guard (a dead ray divides nothing and is not asked).  A refused ray is the exact kernel's whatever this kernel
// would compute for it, and nothing of it is written here: it goes on DEAD, riding along in the shared walks like a lane without a ray, so a batch
// the guard refuses whole -- axis-parallel rays -- costs the optimistic kernel next to nothing.
PT_DEV void guard_or_retire(Ray& r, bool& defer) {
    if (r.mint == r.maxt || ray_guard(r)) return;
    defer = true;
    r.mint = 0.0f;
    r.maxt = 0.0f;
}

// Waves per SIMD of k_traceRadiance (the measurement is at the kernel, pt_kernels_rays.hip) and of k_viewPass, which starts from them
#ifndef PT_RADIANCE_GRID_WAVES
#define PT_RADIANCE_GRID_WAVES 6
#endif
#ifndef PT_RADIANCE_CELL_WAVES
#define PT_RADIANCE_CELL_WAVES 7
#endif
#define PT_RADIANCE_BOUNDS(GRIDS) __launch_bounds__(256, (GRIDS) ? PT_RADIANCE_GRID_WAVES : PT_RADIANCE_CELL_WAVES)
// Waves per SIMD of k_ao (the measurement is at the kernel, pt_kernels_rays.hip) and of k_viewAo / k_viewAoBatch, which start from them
#ifndef PT_AO_GRID_WAVES
#define PT_AO_GRID_WAVES 5
#endif
#ifndef PT_AO_CELL_WAVES
#define PT_AO_CELL_WAVES 7
#endif
// the pass's park rows as closest_all's hooks, with this file's guard and kept division in place of the camera kernels'
struct RadiancePark : Park {
    PT_DEV void guard(Ray& ray, bool& defer) const { guard_or_retire(ray, defer); }
    PT_DEV void top(Ray& ray) const { keep_in_loop(ray); }
};

}  // namespace pt
