// pt_view_plan.hpp -- the host side of the panoramic, fisheye and orthographic cameras (mirt_view_rays, mirt_render_view, mirt_view_guides,
// mirt_render_view_guided, mirt_view_ao; include/mirt.h): the descriptor checks that need no device, the launch plan -- the tile's rays, its blocks of 256
// consecutive ray ids, the whole pixels a block holds and those of the ragged last block -- the route rule of the guided frame, and the checks and
// the plan of the batch calls (mirt_view_rays_batch, mirt_render_view_batch; tests/view_batch_plan_dump.cpp -- mirt_view_guides_batch,
// mirt_render_view_guided_batch, mirt_view_ao_batch; tests/view_batch_aov_plan_dump.cpp).  Plain
// integers and floats: no HIP header and no device, so a plain C++ compiler builds it and tests/test_view_plan.py,
// tests/test_view_guides_plan.py and tests/test_view_ao_plan.py check it on the CPU (tests/view_plan_dump.cpp, tests/view_guides_plan_dump.cpp,
// tests/view_ao_plan_dump.cpp).  mirt_abi.cpp is the caller and owns the messages.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace pt {

constexpr uint32_t kViewOrthographic = 0u, kViewEquirect = 1u, kViewFisheye = 2u;   // MIRT_VIEW_ORTHOGRAPHIC, _EQUIRECT, _FISHEYE
constexpr uint32_t kViewAccumulate = 1u;                                            // MIRT_VIEW_ACCUMULATE
constexpr uint32_t kViewMaxExtent = 65535u;
constexpr uint64_t kViewMaxRays = 0xFFFFFF00ull;   // 2^32 - 256: the kernels index a tile's rays with 32 bits, and a block reaches 255 ids past the last
constexpr int kViewStatusArg = -1;                 // MIRT_E_ARG
constexpr uint32_t kViewAoMaxSamples = 64u;        // MIRT_AO_MAX_SAMPLES

// mirt_view_desc, field for field (mirt_abi.cpp asserts the size and copies the bytes)
struct ViewDesc {
    uint32_t struct_size, model, width, height;
    uint32_t k;
    uint32_t row0, nrows;
    uint32_t flags;
    float eye[3], right[3], up[3], forward[3];
    float half_w, half_h;
    float half_angle;
    float t_min, t_max;
    float tone;
};
// mirt_ao_desc, field for field
struct ViewAoDesc {
    uint32_t struct_size, samples;
    float radius, bias;
};

enum ViewVerdict {
    VIEW_OK,
    VIEW_STRUCT_SIZE,     // struct_size is not sizeof(mirt_view_desc)
    VIEW_MODEL,           // not one of the three models
    VIEW_FLAGS,           // a flag nobody defined
    VIEW_SAMPLES,         // k not in {1, 2, 4, 8, 16}
    VIEW_EXTENT,          // width or height 0 or above 65535
    VIEW_TILE,            // the row tile reaches outside the image
    VIEW_TILE_RAYS,       // the tile holds more than 2^32 - 256 rays
    VIEW_BASIS,           // a non-finite component of eye, right, up or forward
    VIEW_ORTHO_WINDOW,    // ORTHOGRAPHIC: half_w or half_h not finite or <= 0
    VIEW_FISHEYE_ANGLE,   // FISHEYE: half_angle not finite, <= 0 or > pi
    VIEW_T_MIN,           // t_min negative or not finite
    VIEW_T_MAX,           // t_max NaN or <= t_min
    VIEW_TONE,            // a pixel buffer is given and tone is not finite or <= 0
    VIEW_NO_SEEDS,        // mirt_render_view without seeds
    VIEW_NO_OUTPUT,       // mirt_render_view with neither radiance nor pixel
    VIEW_ACCUMULATE_NEEDS_RADIANCE,
    VIEW_NO_GUIDE,        // mirt_view_guides, mirt_render_view_guided with neither normal_hits nor albedo_depth
    VIEW_AO_STRUCT_SIZE,  // mirt_view_ao: struct_size is not sizeof(mirt_ao_desc)
    VIEW_AO_SAMPLES,      // samples 0 or above MIRT_AO_MAX_SAMPLES
    VIEW_AO_RADIUS,       // radius NaN or <= 0
    VIEW_AO_BIAS,         // bias negative, NaN or infinite
    VIEW_AO_NO_SEEDS,     // mirt_view_ao without seeds
    VIEW_AO_NO_OUTPUT,    // mirt_view_ao without ao_out
    VIEW_BATCH_TILE,      // mirt_view_rays_batch, mirt_render_view_batch: row0 != 0, or nrows neither 0 nor height (whole frames only)
    VIEW_BATCH_NO_CAMERAS,   // cameras NULL with n_frames > 0
    VIEW_BATCH_CAMERA,    // a non-finite component of a camera (view_check_batch reports which frame)
    VIEW_BATCH_RAYS       // n_frames * width * height * k * k above 2^32 - 256
};
// the status every refusal above is reported with: 0, or MIRT_E_ARG
inline int view_status(ViewVerdict v) { return v == VIEW_OK ? 0 : kViewStatusArg; }

inline bool view_samples_ok(uint32_t k) { return k == 1u || k == 2u || k == 4u || k == 8u || k == 16u; }
// the rows of the tile: nrows 0 means the whole image, as in mirt_pass_desc
inline uint32_t view_tile_rows(const ViewDesc& v) { return v.nrows ? v.nrows : v.height; }

// what both calls ask of the descriptor (mirt_view_rays reads neither flags' meaning nor tone, but refuses an unknown flag all the same)
inline ViewVerdict view_check_desc(const ViewDesc& v) {
    if (v.struct_size != sizeof(ViewDesc)) return VIEW_STRUCT_SIZE;
    if (v.model > kViewFisheye) return VIEW_MODEL;
    if (v.flags & ~kViewAccumulate) return VIEW_FLAGS;
    if (!view_samples_ok(v.k)) return VIEW_SAMPLES;
    if (!v.width || !v.height || v.width > kViewMaxExtent || v.height > kViewMaxExtent) return VIEW_EXTENT;
    const uint32_t nrows = view_tile_rows(v);
    if (v.row0 >= v.height || nrows > v.height - v.row0) return VIEW_TILE;
    if ((uint64_t)nrows * v.width * (v.k * v.k) > kViewMaxRays) return VIEW_TILE_RAYS;
    for (int c = 0; c < 3; ++c)
        if (!isfinite(v.eye[c]) || !isfinite(v.right[c]) || !isfinite(v.up[c]) || !isfinite(v.forward[c])) return VIEW_BASIS;
    if (v.model == kViewOrthographic && !(isfinite(v.half_w) && isfinite(v.half_h) && v.half_w > 0.0f && v.half_h > 0.0f)) return VIEW_ORTHO_WINDOW;
    if (v.model == kViewFisheye && !(isfinite(v.half_angle) && v.half_angle > 0.0f && v.half_angle <= 0x1.921fb6p+1f)) return VIEW_FISHEYE_ANGLE;
    if (!(isfinite(v.t_min) && v.t_min >= 0.0f)) return VIEW_T_MIN;
    if (!(v.t_max > v.t_min)) return VIEW_T_MAX;   // a NaN compares false; +inf passes
    return VIEW_OK;
}
// ... and what mirt_render_view asks on top, of the descriptor and of which buffers were given
inline ViewVerdict view_check_render(const ViewDesc& v, bool seeds, bool radiance, bool pixel) {
    const ViewVerdict d = view_check_desc(v);
    if (d != VIEW_OK) return d;
    if (pixel && !(isfinite(v.tone) && v.tone > 0.0f)) return VIEW_TONE;
    if (!seeds) return VIEW_NO_SEEDS;
    if (!radiance && !pixel) return VIEW_NO_OUTPUT;
    if ((v.flags & kViewAccumulate) && !radiance) return VIEW_ACCUMULATE_NEEDS_RADIANCE;
    return VIEW_OK;
}
// what mirt_view_guides asks: the descriptor as mirt_view_rays reads it (tone and the meaning of flags are not looked at), and an output
inline ViewVerdict view_check_guides(const ViewDesc& v, bool normal_hits, bool albedo_depth) {
    const ViewVerdict d = view_check_desc(v);
    if (d != VIEW_OK) return d;
    return normal_hits || albedo_depth ? VIEW_OK : VIEW_NO_GUIDE;
}
// what mirt_view_ao asks: the descriptor as mirt_view_rays reads it, then mirt_render_ao's rules for the AO descriptor, then both buffers.  Its
// grid and mask are view_guides_plan's: one lane and one bit per pixel
inline ViewVerdict view_check_ao(const ViewDesc& v, const ViewAoDesc& ao, bool seeds, bool ao_out) {
    const ViewVerdict d = view_check_desc(v);
    if (d != VIEW_OK) return d;
    if (ao.struct_size != sizeof(ViewAoDesc)) return VIEW_AO_STRUCT_SIZE;
    if (!ao.samples || ao.samples > kViewAoMaxSamples) return VIEW_AO_SAMPLES;
    if (!(ao.radius > 0.0f)) return VIEW_AO_RADIUS;   // a NaN compares false; +inf passes
    if (!(ao.bias >= 0.0f) || isinf(ao.bias)) return VIEW_AO_BIAS;
    if (!seeds) return VIEW_AO_NO_SEEDS;
    if (!ao_out) return VIEW_AO_NO_OUTPUT;
    return VIEW_OK;
}
// ... and mirt_render_view_guided: both calls' rules, the frame's first
inline ViewVerdict view_check_render_guided(const ViewDesc& v, bool seeds, bool radiance, bool pixel, bool normal_hits, bool albedo_depth) {
    const ViewVerdict d = view_check_render(v, seeds, radiance, pixel);
    if (d != VIEW_OK) return d;
    return normal_hits || albedo_depth ? VIEW_OK : VIEW_NO_GUIDE;
}

// The batch calls (mirt_view_rays_batch, mirt_render_view_batch): n_frames cameras' frames of one descriptor, stacked -- for the kernels one image
// of n_frames * height rows.  mirt_view_camera, field for field: the twelve floats view_ray reads of a camera.
struct ViewCamera {
    float eye[3], right[3], up[3], forward[3];
};
inline bool view_camera_ok(const ViewCamera& c) {
    for (int i = 0; i < 3; ++i)
        if (!isfinite(c.eye[i]) || !isfinite(c.right[i]) || !isfinite(c.up[i]) || !isfinite(c.forward[i])) return false;
    return true;
}
// What both batch calls ask, in view_check_desc's order with the batch's rules where the single call has its own: whole frames where it checks
// the tile, the batch's ray count where it checks the tile's, the cameras where it checks the descriptor's basis -- which is neither read nor
// checked.  *bad_frame (may be null): the first frame whose camera is refused, with VIEW_BATCH_CAMERA.  n_frames 0 asks nothing of `cameras`.
inline ViewVerdict view_check_batch(const ViewDesc& v, const ViewCamera* cameras, uint32_t n_frames, uint32_t* bad_frame = nullptr) {
    if (v.struct_size != sizeof(ViewDesc)) return VIEW_STRUCT_SIZE;
    if (v.model > kViewFisheye) return VIEW_MODEL;
    if (v.flags & ~kViewAccumulate) return VIEW_FLAGS;
    if (!view_samples_ok(v.k)) return VIEW_SAMPLES;
    if (!v.width || !v.height || v.width > kViewMaxExtent || v.height > kViewMaxExtent) return VIEW_EXTENT;
    if (v.row0 != 0u || (v.nrows != 0u && v.nrows != v.height)) return VIEW_BATCH_TILE;
    if ((uint64_t)v.height * v.width * (v.k * v.k) > kViewMaxRays / (n_frames ? n_frames : 1u)) return VIEW_BATCH_RAYS;   // R <= 2^32: the quotient's floor decides n * R <= max
    if (n_frames && !cameras) return VIEW_BATCH_NO_CAMERAS;
    for (uint32_t f = 0; f < n_frames; ++f)
        if (!view_camera_ok(cameras[f])) {
            if (bad_frame) *bad_frame = f;
            return VIEW_BATCH_CAMERA;
        }
    if (v.model == kViewOrthographic && !(isfinite(v.half_w) && isfinite(v.half_h) && v.half_w > 0.0f && v.half_h > 0.0f)) return VIEW_ORTHO_WINDOW;
    if (v.model == kViewFisheye && !(isfinite(v.half_angle) && v.half_angle > 0.0f && v.half_angle <= 0x1.921fb6p+1f)) return VIEW_FISHEYE_ANGLE;
    if (!(isfinite(v.t_min) && v.t_min >= 0.0f)) return VIEW_T_MIN;
    if (!(v.t_max > v.t_min)) return VIEW_T_MAX;
    return VIEW_OK;
}
// ... and what mirt_render_view_batch asks on top: view_check_render's rules
inline ViewVerdict view_check_render_batch(const ViewDesc& v, const ViewCamera* cameras, uint32_t n_frames, bool seeds, bool radiance, bool pixel, uint32_t* bad_frame = nullptr) {
    const ViewVerdict d = view_check_batch(v, cameras, n_frames, bad_frame);
    if (d != VIEW_OK) return d;
    if (pixel && !(isfinite(v.tone) && v.tone > 0.0f)) return VIEW_TONE;
    if (!seeds) return VIEW_NO_SEEDS;
    if (!radiance && !pixel) return VIEW_NO_OUTPUT;
    if ((v.flags & kViewAccumulate) && !radiance) return VIEW_ACCUMULATE_NEEDS_RADIANCE;
    return VIEW_OK;
}

// What mirt_view_guides_batch, mirt_view_ao_batch and mirt_render_view_guided_batch ask: the batch's rules first (view_check_batch, in its order),
// then the single call's own in the single call's order -- view_check_guides', view_check_ao's, view_check_render_guided's
inline ViewVerdict view_check_guides_batch(const ViewDesc& v, const ViewCamera* cameras, uint32_t n_frames, bool normal_hits, bool albedo_depth, uint32_t* bad_frame = nullptr) {
    const ViewVerdict d = view_check_batch(v, cameras, n_frames, bad_frame);
    if (d != VIEW_OK) return d;
    return normal_hits || albedo_depth ? VIEW_OK : VIEW_NO_GUIDE;
}
inline ViewVerdict view_check_ao_batch(const ViewDesc& v, const ViewCamera* cameras, uint32_t n_frames, const ViewAoDesc& ao, bool seeds, bool ao_out, uint32_t* bad_frame = nullptr) {
    const ViewVerdict d = view_check_batch(v, cameras, n_frames, bad_frame);
    if (d != VIEW_OK) return d;
    if (ao.struct_size != sizeof(ViewAoDesc)) return VIEW_AO_STRUCT_SIZE;
    if (!ao.samples || ao.samples > kViewAoMaxSamples) return VIEW_AO_SAMPLES;
    if (!(ao.radius > 0.0f)) return VIEW_AO_RADIUS;   // a NaN compares false; +inf passes
    if (!(ao.bias >= 0.0f) || isinf(ao.bias)) return VIEW_AO_BIAS;
    if (!seeds) return VIEW_AO_NO_SEEDS;
    if (!ao_out) return VIEW_AO_NO_OUTPUT;
    return VIEW_OK;
}
inline ViewVerdict view_check_render_guided_batch(const ViewDesc& v, const ViewCamera* cameras, uint32_t n_frames, bool seeds, bool radiance, bool pixel, bool normal_hits,
                                                  bool albedo_depth, uint32_t* bad_frame = nullptr) {
    const ViewVerdict d = view_check_render_batch(v, cameras, n_frames, seeds, radiance, pixel, bad_frame);
    if (d != VIEW_OK) return d;
    return normal_hits || albedo_depth ? VIEW_OK : VIEW_NO_GUIDE;
}

// The launch plan of a descriptor that passed view_check_desc.  A block is 256 consecutive tile-local ray ids; rpp = k * k is 1, 4, 16, 64 or 256
// and divides 256, so a block holds pixels_per_block WHOLE pixels -- the unit the in-block resolve and the optimistic / exact pair work in.
struct ViewPlan {
    uint32_t nrows;               // the tile's rows
    uint32_t rpp;                 // k * k
    uint64_t pixels, rays;        // of the tile
    uint32_t blocks;              // ceil(rays / 256): the grid of k_viewRays and k_viewPass
    uint32_t pixels_per_block;    // 256 / rpp
    uint32_t last_block_pixels;   // the pixels of the last block: pixels_per_block unless it is ragged
    uint32_t mask_words;          // the optimistic kernel's mask, a bit per block
};
inline ViewPlan view_plan(const ViewDesc& v) {
    ViewPlan p;
    p.nrows = view_tile_rows(v);
    p.rpp = v.k * v.k;
    p.pixels = (uint64_t)p.nrows * v.width;
    p.rays = p.pixels * p.rpp;
    p.blocks = (uint32_t)((p.rays + 255u) / 256u);
    p.pixels_per_block = 256u / p.rpp;
    const uint32_t rest = (uint32_t)(p.pixels % p.pixels_per_block);
    p.last_block_pixels = rest ? rest : p.pixels_per_block;
    p.mask_words = (p.blocks + 31u) / 32u;
    return p;
}

// The batch's plan, of a descriptor that passed view_check_batch: view_plan of the stacked image.  Its row count n_frames * height may pass 65535
// (and 2^16 * 65535 passes 2^31: nrows is the one product here that needs care); every other product is 64 bits wide as in view_plan.
struct ViewBatchPlan {
    uint32_t frame_rows;               // height: the rows of a frame
    uint64_t frame_pixels, frame_rays; // P and R of include/mirt.h: a frame's share of radiance / pixel and of rays / seeds
    ViewPlan all;                      // nrows = n_frames * height; pixels, rays, blocks, mask words of the whole batch
};
inline ViewBatchPlan view_batch_plan(const ViewDesc& v, uint32_t n_frames) {
    ViewBatchPlan b;
    b.frame_rows = v.height;
    b.frame_pixels = (uint64_t)v.height * v.width;
    b.frame_rays = b.frame_pixels * (v.k * v.k);
    ViewDesc s = v;
    s.row0 = 0u;
    s.nrows = (uint32_t)((uint64_t)n_frames * v.height);   // n_frames * R <= 2^32 - 256 and width, rpp >= 1: it fits
    b.all = view_plan(s);
    if (!n_frames) { b.all.nrows = 0u; b.all.pixels = b.all.rays = 0u; b.all.blocks = b.all.mask_words = 0u; b.all.last_block_pixels = b.all.pixels_per_block; }
    return b;
}

// mirt_view_guides and mirt_view_ao run one lane per PIXEL (k_viewGuides, k_viewAo): the grid, which the launcher is handed, and the optimistic
// kernel's mask of a bit per pixel of the tile, which mirt_abi.cpp allocates
struct ViewGuidesPlan {
    uint32_t blocks;       // ceil(pixels / 256)
    uint32_t mask_words;   // ceil(pixels / 32)
};
inline ViewGuidesPlan view_guides_plan(const ViewPlan& p) {
    ViewGuidesPlan g;
    g.blocks = (uint32_t)((p.pixels + 255u) / 256u);
    g.mask_words = (uint32_t)((p.pixels + 31u) / 32u);
    return g;
}

// ... and of the batch (k_viewGuidesBatch, k_viewAoBatch): the same of the stacked image's n_frames * P pixels, 0 and 0 without frames
inline ViewGuidesPlan view_batch_pixel_plan(const ViewBatchPlan& b) { return view_guides_plan(b.all); }

// Whether mirt_render_view_guided writes the guides from the frame's own launch (k_viewPass GUIDES) instead of queueing k_viewGuides behind it:
// a pixel's samples must be consecutive lanes of ONE wave, which the kernel sums by lane shuffles -- rpp 1, 4, 16 or 64.  Not at 256 rays (a
// pixel spans four waves), and nowhere with MIRT_GUIDED_VIEW=0 (env_on false).  has_grids (a set of more than one cell: the grid kernels run)
// does not bear on it: measured at 1920 x 1080 x 4, the guided grid kernels beat the two launches by 0.34 to 0.41 ms in 5.7 to 6.4
// (cornell_teapot3) as the single-cell ones do by 0.07 ms in 0.98 to 1.18 (cornell), far beyond the spread of the two runs
// (profiles/view_guided/timing.json).  A family that stops doing so goes to the two launches HERE.
inline bool view_guides_in_pass(uint32_t rpp, bool has_grids, bool env_on) {
    (void)has_grids;
    return env_on && (rpp == 1u || rpp == 4u || rpp == 16u || rpp == 64u);
}
// The same decision for mirt_render_view_guided_batch (k_viewPassBatch GUIDES against k_viewPassBatch then k_viewGuidesBatch), made on the batch's
// own measurement: 1024 frames of 32 x 16 x 4, the one launch beats the two by 0.069 to 0.076 ms in 0.51 (cornell, single-cell sets) and by 0.30 ms
// in 2.57 (cornell_teapot3, grids), against a spread of 0.007 ms between the two runs (profiles/view_batch_aov/timing.json).  Both families keep
// the one launch; a family that stops beating the two launches by more than the runs' spread goes to them HERE.
inline bool view_batch_guides_in_pass(uint32_t rpp, bool has_grids, bool env_on) {
    return view_guides_in_pass(rpp, has_grids, env_on);
}

}  // namespace pt
