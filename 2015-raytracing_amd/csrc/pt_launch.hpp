// pt_launch.hpp -- host-callable launchers of the kernel families (C++ linkage; the C ABI
// in mirt_abi.cpp is the only caller).  All launches are asynchronous on `s`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_pass_plan.hpp"   // fused_resolves, fused_segment and the launch plan of a fused pass (host-only)

namespace pt {

enum { KIND_SPHERES = 0, KIND_TRIANGLES = 1 };

// ---- reference-shaped kernels (pt_kernels_granular.hip) ------------------------------------
void launch_sizeof(hipStream_t s, bool ray, uint32_t* out);
void launch_initAcu(hipStream_t s, void* acu, uint32_t total, uint32_t gsz);
void launch_lensDraws(hipStream_t s, void* seeds, void* uv, uint32_t cols, uint32_t rows, uint32_t gx, uint32_t gy,
                      uint32_t row0, uint32_t nrows);
void launch_initTrace(hipStream_t s, void* rays, void* pois, const void* uv, const float* bound, const float* cam,
                      float focal, float lens_rad, uint32_t rpp, uint32_t gx, uint32_t gy);
void launch_bouncePaths(hipStream_t s, const void* pois, void* rays, void* seeds, uint32_t total, uint32_t gsz);
void launch_lightRender(hipStream_t s, void* pois, void* rays, void* acu, const float* light, uint32_t total, uint32_t gsz);
void launch_initShadowTrace(hipStream_t s, void* shadow, const void* pois, uint32_t total, const float* light, void* seeds, uint32_t gsz);
void launch_closest(hipStream_t s, int kind, uint32_t total, void* pois, void* rays, const void* prims, const void* normals,
                    const void* matid, uint32_t mesh_matid, const void* off, const float* bound, uint32_t n, uint32_t exit_far, uint32_t gsz);
void launch_anyhit(hipStream_t s, int kind, uint32_t total, void* shadow, const void* prims, const void* off, const float* bound,
                   uint32_t n, uint32_t exit_far, uint32_t gsz);
void launch_sceneRender(hipStream_t s, void* acu, void* pois, const void* shadow, const void* material, uint32_t nmat,
                        const float* light, uint32_t total, uint32_t gsz);
void launch_copyToPixel(hipStream_t s, void* pixel, const void* acu, float m, uint32_t pixels, uint32_t rpp, uint32_t gsz, void* radiance);
void launch_numerics(hipStream_t s, int op, const void* a, const void* b, void* out, uint64_t n);
void launch_divCheck(hipStream_t s, int mode, uint64_t seed, uint64_t count, void* out16);
void launch_seedFill(hipStream_t s, void* seeds, uint64_t first, uint64_t count, uint32_t base);

// ---- fused pass (pt_kernels_fused.hip) -------------------------------------------------------
constexpr int kMaxLights = 8;
constexpr int kMaxMeshes = 16;

constexpr uint32_t kNoLds = 0xFFFFFFFFu;
constexpr uint32_t kLdsOffWords = 4096;   // 16 KB of LDS per block for cell-offset tables (n <= 15 for a single grid)
constexpr uint32_t kLdsTriMax = 96;       // single-cell triangle sets staged in LDS for the per-lane candidate loops (records, vertex normals, material ids:
                                          // 112 B per triangle): 10.5 KB per block at most
struct GridArgs {            // one cell-sorted primitive set, device pointers
    const void* prims;       // float4 per sphere (c, r^2) | 3 x float4 per PREPARED triangle (launch_prepTriangles)
    const void* pnorm;       // triangles, at most kLdsTriMax records: the candidate sweep's PLANE LIST behind the records and group spheres
                             // (prepared_planes_offset; k_planeList writes it).  A 64-byte header, one slot per chunk of 32 records:
                             // {groups[4], first[4], Gmax[4], Hmax[4]} -- groups = 64-byte groups per class (x | y << 8 | z << 16 | general << 24),
                             // first = the chunk's first group, Gmax / Hmax = the chunk's largest margin constants (M = G |o|_1 + H).  Then the
                             // groups: axis planes {q, n_a, mask, back mask} four to a group, general planes {n.xyz, k = p0 . n, mask, back
                             // mask, 0, 0} two to a group; mask = the chunk's records in that plane (record c0 + j at bit 31 - j), back mask = those
                             // in the same plane with the normal reversed.  Read by scalar loads in the sweep (pt_trace.hpp trace_cell1).
                             // Null: no list (the set runs the wave-uniform loop)
    const void* normals;     // 3 x float4 per triangle (null for spheres)
    const void* matid;       // uint per primitive (null: use `mesh_matid`)
    const void* off;         // uint[n^3 + 1]
    float bound[8];          // (min,1,max,1)
    uint32_t n;              // cells per axis
    uint32_t mesh_matid;
    uint32_t kind;           // KIND_SPHERES | KIND_TRIANGLES
    uint32_t fast_ok;        // geometry-side guard of the exact 3-operation divisions (pt_trace.hpp ray_recip): every bound is 0 or
                             // in [2^-30, 2^20]; for triangles every plane-normal component is 0 or in [2^-40, 2^40].  The host's verdict:
                             // this field and delta, rdelta, exit_far_axes, exit_up, exit_above_axes, walk_ok, exit_is_far_face below are pt_set_guard.hpp's
                             // SetGuard, copied (mirt_abi.cpp fill_grid)
    uint32_t lds_off;        // fused pass (launch_fused assigns it).  n > 1: dword index of this set's cell-offset table inside the block's
                             // LDS copy, or kNoLds when the tables of the scene do not fit.  n == 1, triangles: dword index (a multiple of
                             // 4) of the set's `nslots` prepared records staged in LDS for the per-lane candidate loops, or kNoLds
    float delta[3], rdelta[3]; // n > 1, optimistic kernel: the cell width per axis (hi - lo) / n and its reciprocal, both correctly rounded --
    uint32_t nslots;         // off[n^3], the number of (cell, primitive) slots, when the host knows it (0: the walk reads it from the table)
    uint32_t exit_far_axes;  // n == 1, optimistic kernel: bit k set where the cell's forward exit plane x_up = lo + 1*((hi-lo)/1) (A10 code.cl:699-707)
                             // equals hi, so a ray with d_k >= 0 leaves the cell where it leaves the box (pt_trace.hpp cell1_exit)
    float exit_up[3];        // ... and x_up itself per axis, for the axes whose bit is clear (the backward plane lo + 0*((hi-lo)/1) is lo: host-checked)
    uint32_t exit_gap_max;   // (the BITS of a float: the kernel asks "is it 0" as a scalar compare.)  n == 1, optimistic kernel, the one slab pass (pt_trace.hpp
                             // box_exit1; pt_box_exit.hpp: the derivation and the constant).  Where x_up lies ABOVE hi, "tmin <= exit" may hold for a ray the
                             // box's far face drops; a lane whose window is shorter than this constant times its largest reciprocal sends its wave to the
                             // box's own comparison.  The largest (x_up - hi) (1 + 2^-20) of the three axes, 0 when no axis has x_up > hi (then nothing is
                             // tested); it sits behind exit_up so that one scalar load brings both
    uint32_t exit_above_axes; // ... bit k set where x_up > hi (pt_set_guard.hpp)
    uint32_t walk_ok;      // what every lane would compute for itself from wave-uniform inputs (pt_trace.hpp axis_setup_t).  walk_ok: the
                             // widths and spans sit inside the windows in which the kernel's 3-operation divisions are exact; a lane that
                             // walks a set without it hands its sample to the exact kernel
    uint32_t exit_is_far_face; // n == 1 only: lo + 1*((hi-lo)/1) == hi and lo + 0*((hi-lo)/1) == lo hold bitwise on all three
                             // axes (checked on the host: pt_set_guard.hpp set_exit_is_far_face), so the single cell's exit t equals the AABB slab's far t
    uint32_t gap_ok;         // n == 1, triangles with a plane list, optimistic kernel: `gap` holds the set's PLANE-FREE GAP (pt_shadow_gap.hpp; the host
                             // makes it from its copy of the plane list and these bounds).  A wave whose shadow segments all pass the gap test skips the
                             // set's box test and the axis entries of the list (pt_direct.hpp direct_all).  0: no gap, every query runs the box test
    float gap[12];           // {qlo[3], qhi[3], Gm[3], Hm[3]}: per axis the open interval between the neighbouring axis planes / box faces / exit planes
                             // around the box centre, and the margin constants m_a = Gm_a |o|_1 + Hm_a.  Kernel arguments: scalar operands where they are used
};
struct LightArgs {           // the three float16 packings of one light (A10 code.js:323-352)
    float shadow[16];        // pos, T, B, radius
    float scene[16];         // pos, normal, irradiance, area
    float light[16];         // pos, normal, irradiance, radius
};
struct FusedArgs {
    float cam[16];
    float bound[8];
    float focal_length, lens_rad;
    uint32_t width, height, rpp;
    uint32_t row0, nrows;    // row tile this launch renders; per-ray buffers are tile-local
    uint32_t bounces;        // 5 in the reference (A10 code.js:1829)
    uint32_t n_sets, n_lights;
    GridArgs sets[2 + kMaxMeshes];   // upload order: spheres, loose triangles, mesh 0..M-1 (A10 code.js:1809-1813)
    LightArgs lights[kMaxLights];
    const void* material;    // float4[nmat]
    uint32_t nmat;
    int32_t* seeds;          // [nrows*width*rpp], read-modify-write
    void* acu;               // float4[nrows*width*rpp], accumulated into
    const void* uv;          // rpp == 1: float2[nrows*width] lens draws from launch_lensDraws
    uint32_t fresh;          // 1: the accumulator starts at zero and is not read (initAcu folded into the pass, mirt_render_first_pass)
    // copyToPixel INSIDE the pass (A10 code.cl:1366-1386; `resolve` != 0): a block of 256 lanes holds whole SEGMENTS of pixels (seg_off, seg_len below)
    // and the pass is a frame's first, so every accumulator of a segment is final in the block's LDS when its last sample ends: the block sums them in
    // the reference's order and writes `pixel` (RGBA8) and / or `radiance` (the un-scaled sums); `acu` may then be null -- nothing per ray but the seed
    // touches memory: 8 B per sample + 20 B per pixel.  The pass's plan decides (pt_pass_plan.hpp pass_plan: `resolves`).
    void* pixel;             // uchar4[nrows*width] or null
    void* radiance;          // float4[nrows*width] or null
    float res_m;             // 1 / (rpp * passes), A10 code.js:1412
    uint32_t resolve;
    // The launch's SEGMENT (pt_pass_plan.hpp pass_segment, fused_segment): samples [seg_off, seg_off + seg_len) of EVERY pixel of the tile, seg_len a power of two <= 256.  A block
    // holds 256 / seg_len pixels' segments: lane t of block b is sample seg_off + t % seg_len of pixel b * (256 / seg_len) + t / seg_len (k_fusedPass
    // seg_ray).  A pixel of more than 256 rays resolves in several launches, in ray order, each continuing the pixel's chain of additions from what
    // `radiance` holds -- the sums over the segments before it -- so the reference's one chain (A10 code.cl:1377-1380) is cut at segment boundaries
    // and carried through memory, 16 B per pixel and launch instead of 16 B per ray.  `pixel` is given to the last launch only.
    uint32_t seg_off;        // 0 unless resolving a pixel of more than 256 rays
    uint32_t seg_len;        // rpp when the pass is one segment (rpp <= 256, or not resolving in the pass)
    uint32_t seg_pitch;      // a CONTIGUOUS segment (seg_len == rpp, or 256): the ray ids from one block's first to the next's -- 256, or rpp when a
                             // block is 256 samples of one pixel (then block b's first ray is b * rpp + seg_off)
    // Progressive passes in ONE launch (mirt_render_passes): every sample runs `passes` passes in a row, its seed and accumulator carried in the
    // kernel, and is written once at the end; `fresh` applies to the first of them, `res_m` to the frame after the last.  > 1 picks the MULTI
    // instantiations of k_fusedPass; 0 and 1 run the single-pass kernels, which never read it.
    uint32_t passes;
    // A frame after EVERY pass of such a launch (mirt_render_passes with MIRT_PASSES_EVERY_FRAME; `every` != 0 in resolving launches with passes > 1
    // only): `pixel` and `radiance` then hold `passes` frames of nrows * width pixels back to back, frame p the one after pass p, tone-scaled by
    // 1 / (rpp * (pass_index + p)) -- worked out in the kernel in double, as the host works out res_m.  A later segment of a pixel of more than 256
    // rays goes on from `carry` (`passes` frames of the sums the segments before it left) instead of from `radiance`: the optimistic and the redo
    // launch of a segment read the same carry, which neither of them writes.
    uint32_t every;
    uint32_t pass_index;     // the 1-based index of the launch's first pass
    const void* carry;       // float4[passes * nrows * width]; read only by a launch with seg_off != 0
    // The first-hit guides written BY the pass (mirt_render_first_pass_guided and mirt_render_passes_guided, the one-launch route: pt_pass_plan.hpp
    // fused_guides_in_pass, fused_guides_in_passes): float4 per pixel of the tile each, as launch_guides writes them; either may be null.  Both null:
    // the pass's ordinary kernels.  One given picks the GUIDES instantiations of k_fusedPass, which exist for resolving launches of one contiguous
    // segment only, and with passes > 1 for scenes without grids and their default reuse pairing only (fused_has_grids, fused_multipass_default) --
    // the caller keeps to the route rule.
    void* guide_nh;          // normal_hits
    void* guide_ad;          // albedo_depth
};
// the optimistic kernel may run the launch: every set passed its geometry-side guard (pt_set_guard.hpp)
inline bool all_sets_fast_ok(const FusedArgs& a) { for (uint32_t i = 0; i < a.n_sets; ++i) if (!a.sets[i].fast_ok) return false; return true; }
// fast: the optimistic kernel (writes deferred samples' bits into defer_mask); !fast: the exact kernel over `list` (or everything)
void launch_fused(hipStream_t s, const FusedArgs& a, bool fast, uint32_t* defer_mask, const uint32_t* redo_mask, uint32_t redo_words);
bool fused_fast_available();   // compiled with PT_EXACT_FAST_DIV
bool fused_has_grids(const FusedArgs& a);           // a set of `a` has more than one cell: the launch runs the grid kernels
bool fused_multipass_default(const FusedArgs& a);   // a multi-pass launch of `a` would pick the default MULTI pairing (MIRT_MULTIPASS_REUSE unset, or forcing what the default is)
void launch_deferCount(hipStream_t s, const uint32_t* mask, uint32_t words, uint32_t* count);
// First-hit guide buffers (pt_kernels_guides.hip): float4 per pixel of the tile, normal_hits = (sum of the hit samples' normals, hits),
// albedo_depth = (sum of their material colours, sum of their Ray.maxt).  One lane per pixel; the optimistic / exact pair as in launch_fused, the
// mask one bit per pixel: (nrows * width + 31) / 32 words.  Reads the camera, bounds, sets and material of `a`; either output may be null.
void launch_guides(hipStream_t s, const FusedArgs& a, bool fast, void* normal_hits, void* albedo_depth, uint32_t* defer_mask, const uint32_t* redo_mask);
// Ray queries (pt_kernels_rays.hip): `count` caller-supplied rays of 32 bytes {o, mint, d, maxt}, one lane per ray.  occluded != null: a byte per
// ray, 1 iff the any-hit stage leaves mint == maxt; else the closest hit, hits = {normal, t, p, matId} (32 bytes per ray) and / or sets = the index
// of the winning set (uint32 per ray).  The optimistic / exact pair as in launch_guides, the mask one bit per ray: (count + 31) / 32 words.  Reads
// the sets of `a` and nothing else of it.
void launch_rays(hipStream_t s, const FusedArgs& a, bool fast, const void* rays, uint32_t count, void* hits, uint32_t* sets, uint8_t* occluded,
                 uint32_t* defer_mask, const uint32_t* redo_mask);
// Ambient occlusion of the first hit (pt_kernels_rays.hip k_ao; the definition is mirt_render_ao's comment in include/mirt.h): uint32[2] per pixel
// of the tile, {open, cast}.  One lane per pixel; the optimistic / exact pair as in launch_guides, the mask one bit per pixel.  Reads the camera,
// bounds and sets of `a` and a.seeds (int32 per tile-local ray, never written); not its material or lights.
void launch_ao(hipStream_t s, const FusedArgs& a, bool fast, uint32_t samples, float radius, float bias, void* ao_out, uint32_t* defer_mask, const uint32_t* redo_mask);
// Path radiance of caller-supplied rays (pt_kernels_rays.hip k_traceRadiance; the definition is mirt_trace_radiance's comment in include/mirt.h):
// `samples` runs of the pass's path per ray, from the caller's ray on.  rays: two float4 per ray; seeds: int32 per ray, read and written; radiance:
// float4 per ray, the accumulator (read first with flags & 1).  The optimistic / exact pair as in launch_rays, the mask one bit per ray.  Reads the
// sets, lights, material, nmat and bounces of `a` and nothing else of it.
void launch_radiance(hipStream_t s, const FusedArgs& a, bool fast, const void* rays, uint32_t count, uint32_t samples, uint32_t flags, int32_t* seeds, void* radiance,
                     uint32_t* defer_mask, const uint32_t* redo_mask);
// Panoramic, fisheye and orthographic cameras (pt_kernels_rays.hip k_viewRays, k_viewPass; the definition is mirt_view_rays's comment in
// include/mirt.h, the ray of a sample pt_view.hpp's view_ray).  The caller has checked everything (pt_view_plan.hpp).
struct ViewArgs {
    uint32_t model;              // MIRT_VIEW_ORTHOGRAPHIC / _EQUIRECT / _FISHEYE
    uint32_t width, height;      // the WHOLE image
    uint32_t k;                  // samples per axis: 1, 2, 4, 8 or 16
    uint32_t row0, nrows;        // the row tile; ray ids are tile-local
    float eye[3], right[3], up[3], forward[3];
    float half_w, half_h, half_angle, t_min, t_max;
};
// The batch calls (mirt_view_rays_batch, mirt_render_view_batch): n frames of frame_rows = height rows each, stacked into one image of nrows =
// n * frame_rows rows, row0 = 0; `cameras` is the device table of 12 floats per frame (eye, right, up, forward), which the batch kernels read
// INSTEAD of the four arrays of ViewArgs.  A struct of its own, handed to those kernels only: a member more in ViewArgs moves the kernel
// arguments behind it, and the single calls' instances keep their code (profiles/view_batch/README.md).
struct ViewBatchArgs : ViewArgs {
    const float* cameras;
    uint32_t frame_rows;
};
// n cameras of 12 floats from HOST memory into the device table (n * 12 floats), in stream order: launches of k_viewCameras whose kernel arguments
// carry kViewCameraChunk cameras each, so the host array is read before this returns and no staging memory outlives the call
constexpr uint32_t kViewCameraChunk = 64u;   // 3072 bytes of arguments a launch
void launch_viewCameras(hipStream_t s, const float* host_cameras, uint32_t n, float* table);
// the tile's nrows * width * k * k rays as 32-byte records, one lane per ray; the batch's n * height * width * k * k likewise
void launch_viewRays(hipStream_t s, const ViewArgs& v, void* rays);
void launch_viewRaysBatch(hipStream_t s, const ViewBatchArgs& v, void* rays);
// mirt_render_view: those rays through k_traceRadiance's path at one sample each and the block's resolve, in one launch.  seeds: int32 per tile
// ray, read and written; radiance (float4) / pixel (uchar4) per tile pixel, either may be null; accumulate: the sums go on from `radiance`.  The
// optimistic / exact pair per BLOCK of 256 ray ids: the mask is one bit per block, (blocks + 31) / 32 words.  Reads the sets, lights, material,
// nmat and bounces of `a` and nothing else of it -- but a.guide_nh / a.guide_ad: either given, the frame writes the first-hit guides of its
// pixels too (k_viewPass GUIDES; mirt_render_view_guided's one-launch route, which the caller takes at k * k = 1, 4, 16 or 64 only).
void launch_viewPass(hipStream_t s, const FusedArgs& a, const ViewArgs& v, bool fast, bool accumulate, int32_t* seeds, void* radiance, void* pixel, float tone,
                     uint32_t* defer_mask, const uint32_t* redo_mask);
// mirt_render_view_batch, mirt_render_view_guided_batch: the same of the stacked frames (k_viewPassBatch, pt_kernels_view_batch.hip), a.guide_nh /
// a.guide_ad included
void launch_viewPassBatch(hipStream_t s, const FusedArgs& a, const ViewBatchArgs& v, bool fast, bool accumulate, int32_t* seeds, void* radiance, void* pixel, float tone,
                          uint32_t* defer_mask, const uint32_t* redo_mask);
// mirt_view_guides: the first-hit guides of those rays (k_viewGuides), float4 per tile pixel each as launch_guides writes them; either may be
// null.  One lane per pixel, `blocks` blocks of 256; the optimistic / exact pair per PIXEL, the mask one bit per pixel: both are the plan's
// (pt_view_plan.hpp view_guides_plan).  Reads the sets, material and nmat of `a` and nothing else of it.
void launch_viewGuides(hipStream_t s, const FusedArgs& a, const ViewArgs& v, uint32_t blocks, bool fast, void* normal_hits, void* albedo_depth, uint32_t* defer_mask,
                       const uint32_t* redo_mask);
// mirt_view_ao: ambient occlusion of those rays' first hits (k_viewAo: k_ao with the ray made by view_ray), uint32[2] per tile pixel, {open, cast}.
// One lane per pixel, `blocks` blocks of 256; the optimistic / exact pair per PIXEL, the mask one bit per pixel: both are view_guides_plan's.
// seeds: int32 per tile ray, never written.  Reads the sets of `a` and nothing else of it.
void launch_viewAo(hipStream_t s, const FusedArgs& a, const ViewArgs& v, uint32_t blocks, bool fast, uint32_t samples, float radius, float bias, const int32_t* seeds,
                   void* ao_out, uint32_t* defer_mask, const uint32_t* redo_mask);
// mirt_view_guides_batch, mirt_view_ao_batch: the two above of the stacked frames (k_viewGuidesBatch, k_viewAoBatch, pt_kernels_view_batch.hip);
// blocks and the mask are of the image of n_frames * height rows (pt_view_plan.hpp view_batch_pixel_plan)
void launch_viewGuidesBatch(hipStream_t s, const FusedArgs& a, const ViewBatchArgs& v, uint32_t blocks, bool fast, void* normal_hits, void* albedo_depth, uint32_t* defer_mask,
                            const uint32_t* redo_mask);
void launch_viewAoBatch(hipStream_t s, const FusedArgs& a, const ViewBatchArgs& v, uint32_t blocks, bool fast, uint32_t samples, float radius, float bias, const int32_t* seeds,
                        void* ao_out, uint32_t* defer_mask, const uint32_t* redo_mask);
// Edge-avoiding a-trous filter (pt_kernels_filter.hip; the definition is mirt_filter_atrous's comment in include/mirt.h).  The caller has checked
// every extent: each input and output holds width * height elements, work[0], work[1] and guide width * height float4 each.
struct FilterArgs {
    uint32_t width, height;
    uint32_t demodulate;         // MIRT_FILTER_DEMODULATE
    uint32_t npow;               // normal_power_log2: the normal term is squared that many times
    uint32_t depth_on, colour_on;
    float tone, sigma_depth;
    const void* radiance;        // float4 per pixel
    const void* normal_hits;
    const void* albedo_depth;
    void* filtered;              // float4 per pixel, or null
    void* pixel;                 // uchar4 per pixel, or null
    void* work[2];               // (I.xyz, live ? 1 : 0): iteration i reads work[i & 1] and writes the other
    void* guide;                 // (n^.xyz, z), zero where the pixel is not live
};
// I_0 into work[0] and the prepared guide; last (no iteration follows): the outputs instead
void launch_filterPrepare(hipStream_t s, const FilterArgs& a, bool last);
// iteration step_log2 (step 2^step_log2) from work[src] into work[src ^ 1], or -- last -- into the outputs.  inv_colour: 1 / (k_i * k_i), IEEE fp32,
// from the host.  tiled: the decimated LDS tiles, else one thread per pixel reading its taps directly; the bits are the same.
void launch_filterStep(hipStream_t s, const FilterArgs& a, uint32_t src, uint32_t step_log2, float inv_colour, bool last, bool tiled);
// The same filter in row tiles (mirt_filter_atrous_rows): the inputs, work[] and guide hold the rows of a WINDOW of the image, `height` of them, and
// filtered / pixel the own rows alone.  A launch computes the rows [band_row0, band_row0 + band_nrows) of the window (pt_rows_plan.hpp's filter_band);
// the last launch's band is the own rows, which it stores from the outputs' first element on.
struct FilterRowsArgs : FilterArgs {
    uint32_t band_row0, band_nrows;
};
void launch_filterPrepareRows(hipStream_t s, const FilterRowsArgs& a, bool last);
void launch_filterStepRows(hipStream_t s, const FilterRowsArgs& a, uint32_t src, uint32_t step_log2, float inv_colour, bool last, bool tiled);
// which structure an iteration of step 2^step_log2 runs as unless the caller forces one: bit step_log2 set = tiled.  Measured at 1080p
// (profiles/filter/timing.json, step_direct_ms against step_tiled_ms): the LDS tiles win at steps 1 and 2, direct reads at 4, 8 and 16.
constexpr uint32_t kFilterTiledSteps = 0x03u;
// Guide-driven upsampling (pt_kernels_upsample.hip; the definition is mirt_upsample_guided's comment in include/mirt.h): a frame shaded at
// (width / factor) x (height / factor) rebuilt at width x height from the guides of both resolutions.  The caller has checked every extent: the
// three low inputs hold (width / factor) * (height / factor) float4, the high guides and outputs width * height elements, factor divides both sizes.
struct UpsampleArgs {
    uint32_t width, height;      // HIGH resolution
    uint32_t factor;             // 2 .. 4
    uint32_t demodulate;         // MIRT_UPSAMPLE_DEMODULATE
    uint32_t npow;               // normal_power_log2
    uint32_t depth_on;
    float tone, sigma_depth;
    const void* radiance_lo;     // float4 per low pixel
    const void* normal_hits_lo;
    const void* albedo_depth_lo;
    const void* normal_hits;     // float4 per high pixel
    const void* albedo_depth;
    void* upsampled;             // float4 per high pixel, or null
    void* pixel;                 // uchar4 per high pixel, or null
};
void launch_upsample(hipStream_t s, const UpsampleArgs& a);
// The same upsampler on high rows [row0, row0 + nrows) (mirt_upsample_guided_rows): width / height are the whole high image's, the high guides and
// the outputs hold those rows alone, the three low inputs the low rows from lo_row0 on (the caller has checked that they contain every tap).
struct UpsampleRowsArgs : UpsampleArgs {
    uint32_t row0, nrows, lo_row0;
};
void launch_upsampleRows(hipStream_t s, const UpsampleRowsArgs& a);
// {p0,e1,e2,n} records from the host's 3 x float4 position buffer (see pt_kernels_fused.hip); `out` holds count records of 48 B,
// behind them ceil(count / kTriGroup) float4 {centre, R'^2}: the bounding spheres of groups of consecutive records, and behind those, for
// count <= kLdsTriMax, the candidate sweep's plane list (GridArgs::pnorm)
void launch_prepTriangles(hipStream_t s, const void* pos, void* out, uint32_t count, uint32_t* insane_word);
size_t prepared_bytes(uint32_t count);   // what `out` must hold for `count` triangles
#ifndef PT_TRI_GROUP
#define PT_TRI_GROUP 16
#endif
constexpr uint32_t kTriGroup = PT_TRI_GROUP;   // prepared records per bounding sphere (pt_trace.hpp group_missed)
// byte offset of the candidate sweep's plane list inside it (64-byte aligned), and its size: the header, then per chunk of 32 records at
// most 32 general entries of 32 bytes (or 32 axis entries of 16) plus one partly filled 64-byte group per class
inline size_t prepared_planes_bytes(uint32_t count) { return 64 + ((size_t)count + 31) / 32 * (32 * 32 + 4 * 64); }
__host__ __device__ inline size_t prepared_planes_offset(uint32_t count) { return ((size_t)count * 48 + ((size_t)count + kTriGroup - 1) / kTriGroup * 16 + 63) & ~(size_t)63; }

// ---- uniform-grid build on the device (pt_grid_build.hip) -------------------------------------------
constexpr uint32_t kMaxCellSlots = 1u << 24;        // slots ONE cell of a grid with n > 1 may hold: the shared-test walk packs a slot's place in its cell into 24 bits (pt_trace_coop.hpp)
constexpr uint64_t kMaxGridSlots = 0x7FFFFFFFull;   // (cell, primitive) slots one grid may hold: the sort and every consumer index them with 31 bits
hipError_t grid_build(hipStream_t s, int kind, const double* prims, uint32_t count, const double bounds6[6], uint32_t n,
                      uint32_t* offsets, uint32_t** order_out, uint32_t* total, uint64_t* slots_needed);
void launch_gatherTriangles(hipStream_t s, const uint32_t* order, uint32_t total, const double* pos9, const double* nor9,
                            int nsteps, const int* ops, const double* vecs, float pad_w, void* pos_out, void* nor_out);
void launch_gatherSpheres(hipStream_t s, const uint32_t* order, uint32_t total, const double* sph4, void* out);
// parseMeshJSON for one (node, mesh) pair: corners de-indexed + transformed into the fp64 soups, bounds6 (fp32 min xyz, max xyz) merged.
// scratch8: 8 device words (6 encoded bounds, a flag word set to 1 by an out-of-range index, one spare); the caller zeroes word 6 first.
void launch_meshIngest(hipStream_t s, const double* P, const double* N, const uint32_t* idx, uint32_t n_vertices, uint32_t n_corners,
                       const float* m16, const float* nm9, double* pos_out, double* nor_out, float* bounds6, uint32_t* scratch8);
void launch_gatherU32(hipStream_t s, const uint32_t* order, uint32_t total, const uint32_t* in, uint32_t* out);

// ---- single-frame kernels of Assign01 / 04 / 07 (pt_kernels_frame.hip) -----------------------------
void launch_a01_raytrace(hipStream_t s, void* pixels, const float* cam, uint32_t gx, uint32_t gy);
void launch_frame_initTrace(hipStream_t s, bool clip, void* pixels, const float* cam, void* rays, const float* bound, uint32_t gx, uint32_t gy);

// What the Assign04 / Assign07 trace stages read, for both frame paths.  The caller has checked every extent (mirt_abi.cpp frame_a04_mesh,
// frame_a07_mesh, frame_a07_mol, which also fill the stages' fields).
struct FrameArgs {
    float cam[16];
    float bound[8];          // assign 7: the one box of initTrace's clip and of both grids
    void* pixels;            // uchar4 per pixel
    void* rays;              // 48 B per pixel; launch_frame_fused: or null
    uint32_t assign;         // launch_frame_fused: 4 or 7
    uint32_t mesh, mol;      // launch_frame_fused, assign 7: which stages run
    uint32_t gx, gy;         // the NDRange; pixels outside it or outside cam.cols x cam.rows stay untouched
    uint32_t t_size;         // assign 4
    const void* prep;        // prepared records (launch_prepTriangles) of the t_size triangles | of the n_slots grid slots, behind them one
                             // bounding sphere per kTriGroup records
    const void* normals;
    const void* mindex;      // assign 4
    const void* mcolor;
    uint32_t ncolors;
    uint32_t n_slabs;        // assign 7, both grids
    const void* slab_size;   // the mesh's cell table
    uint32_t n_slots;
    uint32_t group_slots;    // (launch_frame_fused sets it)
    const void* atoms;       // float4 {c, r*r} per slot
    const void* mol_slab_size;
};
// the whole frame in one launch (k_frame_fused): initTrace and the trace stage(s) on one thread per pixel, the ray in registers.  assign 4: the brute
// force; assign 7: the molecule stage when `mol` is set, then the mesh stage when `mesh` is, the mesh starting from the maxt the molecule left
// (A07 code.js:629-661 computeBoth).  rays null: nothing per ray touches memory.
void launch_frame_fused(hipStream_t s, FrameArgs a);
// one stage as a launch of its own (k_a04_meshTrace, k_a07_meshTrace, k_a07_molTrace) over the rays initTrace or the stage before left in a.rays
enum FrameStage : uint32_t { FS_A04 = 1u, FS_MESH = 2u, FS_MOL = 4u };
void launch_frame_stage(hipStream_t s, const FrameArgs& a, FrameStage stage);
// the anti-aliased frame in one launch (k_frame_aa_lanes): `a` is launch_frame_fused's for the FINE frame -- a.cam says aa*ow x aa*oh, a.rays is
// unused -- and a.pixels holds ow x oh pixels, each the box average of its aa x aa fine samples.  aa: 2, 3 or 4.
void launch_frame_aa(hipStream_t s, FrameArgs a, uint32_t aa, uint32_t ow, uint32_t oh);

}  // namespace pt
