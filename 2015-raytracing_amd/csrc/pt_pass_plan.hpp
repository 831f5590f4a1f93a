// pt_pass_plan.hpp -- how one fused pass is launched, worked out once: whether it resolves its pixels in the kernel, the segments of a pixel's
// rays and their launches, the deferred-block mask, the scratch buffer's layout, and the route mirt_render_passes takes.  Integer arithmetic on a
// handful of inputs: no HIP header and no device, so a plain C++ compiler builds it and tests/test_pass_plan.py checks it on the CPU.
// mirt_abi.cpp (render_pass_impl, mirt_render_passes) is the caller; pt_kernels_fused.hip reads fused_segment_contiguous.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pt {

// Whether a pass with these arguments can resolve inside the kernel: rpp divides 256 (whole pixels per block), or rpp > 256 -- any count: the
// segment plan below covers it -- and somewhere to put the result.  A frame's first pass may then do without `acu`.
inline bool fused_resolves(uint32_t rpp, bool want_out) {
    if (!want_out || rpp == 0u) return false;
    return rpp > 256u || 256u % rpp == 0u;
}
// Whether a pass that KEEPS `acu` resolves in the kernel too: only at the counts that resolved in the pass before the segment plan -- rpp divides
// 256, or is 256 times a power of two up to 32.  At the other counts above 256 such a pass writes `acu` and runs the separate copyToPixel: resolving
// there beside a kept accumulator was not measured against it.  The block's LDS holds the accumulators as the pass leaves them, which is what copyToPixel would read back.
inline bool fused_resolves_with_acu(uint32_t rpp, bool want_out) {
    if (!fused_resolves(rpp, want_out)) return false;
    if (rpp <= 256u) return true;
    const uint32_t c = rpp / 256u;
    return rpp % 256u == 0u && c <= 32u && (c & (c - 1u)) == 0u;
}
// The segment plan: a pixel's rays [0, rpp) cut in ray order into power-of-two segments of at most 256 -- floor(rpp / 256) of 256, then one per
// set bit of rpp % 256, largest first (289: 256, 32, 1).  The length of the segment that starts at sample `off` is the largest power of two that
// is at most 256 and at most the rays left.  rpp <= 256 (dividing 256): one segment, the whole pixel.
inline uint32_t fused_segment(uint32_t rpp, uint32_t off) {
    if (rpp <= 256u) return rpp;
    const uint32_t left = rpp - off;
    return left >= 256u ? 256u : 1u << (31 - __builtin_clz(left));
}
// the contiguous form of a segment's ray ids (FusedArgs::seg_pitch) applies: the segment is the whole pixel, or 256 of its rays
inline bool fused_segment_contiguous(uint32_t rpp, uint32_t len) { return len == rpp || len == 256u; }

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------
struct PassRequest {
    uint32_t rpp;            // rays per pixel
    uint64_t npix;           // pixels in the row tile
    uint32_t passes;         // progressive passes the launch runs (mirt_render_passes: the call's n_passes)
    bool fresh;              // the first of them is a frame's first pass
    bool has_acu, has_pixel, has_radiance;   // which buffers the caller gave
    bool every;              // a frame after every pass (MIRT_PASSES_EVERY_FRAME)
    bool inpass_resolve;     // the context's switch (MIRT_INPASS_RESOLVE)
};
// what mirt_render_passes does with its n_passes
enum PassRoute {
    ROUTE_ONE_LAUNCH,        // one multi-pass launch, the frame after the last pass
    ROUTE_ONE_LAUNCH_EVERY,  // one multi-pass launch that resolves in the kernel and writes every pass's frame
    ROUTE_ORDINARY_PASSES,   // n_passes ordinary passes, each writing its own frame slot when every frame is asked for
};
struct ScratchRegion { uint64_t off, bytes; };   // bytes == 0: the pass does not use it
struct PassPlan {
    uint32_t rpp;
    uint64_t npix;
    bool resolves;           // copyToPixel runs inside the pass (FusedArgs::resolve)
    bool null_acu_ok;        // ... of one pass (mirt_render_pass, mirt_render_first_pass)
    bool null_acu_ok_passes; // ... of mirt_render_passes
    PassRoute route;
    uint32_t n_segments;     // launches (or optimistic + redo pairs) of the pass, in ray order: pass_segment(plan, 0 .. n_segments - 1)
    uint32_t mask_words;     // the deferred-block mask of all of them, and what one of its bits stands for:
    uint32_t mask_unit;      // a block of 256 samples resolving in the pass (the exact kernel re-runs whole blocks), else 1 sample
    bool carries;            // every frame, more than 256 rays per pixel: the segments' sums alternate between two carry arrays (pass_segment)
    // The context's scratch buffer, asked for ONCE per pass (growing it frees the old one, so an earlier pointer into it would dangle): one size, the
    // regions side by side.  lens: float2 per pixel from launch_lensDraws (1 ray per pixel).  sums: float4 per pixel, the sums a pixel of more than
    // 256 rays carries from launch to launch where the caller gave no radiance buffer (FusedArgs::seg_off).  carry[0 / 1]: `passes` frames of such
    // sums each; carry[0] is the caller's radiance where there is one (its bytes are 0 then).
    ScratchRegion lens, sums, carry[2];
    uint64_t scratch_bytes;
};
struct PassSegment {
    uint32_t off, len, pitch;            // FusedArgs::seg_off, seg_len, seg_pitch
    uint32_t mask_first, mask_words;     // its own region of the mask
    bool writes_pixel;                   // resolving, the last segment: the one launch that is given `pixel`
    uint32_t carry_write, carry_read;    // plan.carries: the carry array its launches write (as `radiance`) and the one they go on from (`carry`)
};

// mask words of one launch over `len` samples of every pixel
inline uint32_t pass_mask_words(const PassPlan& p, uint32_t len) {
    const uint64_t samples = p.npix * len;
    return (uint32_t)(((p.mask_unit == 256u ? (samples + 255u) / 256u : samples) + 31u) / 32u);
}

// Segment i < n_segments, from the plan alone (nothing is stored per segment: 2^24 rays per pixel are 65 536 of them).  Resolving in the pass a
// pixel of more than 256 rays: the segments of fused_segment, each launch going on from the sums the one before left; every launch has its own
// region of the mask, one bit per block, the regions back to back.  Otherwise one segment, the whole pass.
inline PassSegment pass_segment(const PassPlan& p, uint32_t i) {
    PassSegment s;
    s.off = 0u; s.len = p.rpp; s.mask_first = 0u;
    if (p.n_segments > 1u) {
        const uint32_t n256 = p.rpp / 256u, k = i < n256 ? i : n256;   // the first n256 segments are alike; behind them at most 8, walked
        s.off = k * 256u;
        s.mask_first = k * pass_mask_words(p, 256u);
        for (uint32_t j = k;; ++j) {
            s.len = fused_segment(p.rpp, s.off);
            if (j == i) break;
            s.off += s.len;
            s.mask_first += pass_mask_words(p, s.len);
        }
    }
    s.pitch = s.len == 256u && p.rpp > 256u ? p.rpp : 256u;
    s.mask_words = pass_mask_words(p, s.len);
    s.writes_pixel = p.resolves && i + 1u == p.n_segments;
    // Every frame, a pixel of more than 256 rays: segment i of every pass goes on from the sums segment i - 1 left for that pass.  An optimistic block
    // may write pass p's sums and defer in a later pass, and the redo launch must read what the optimistic one read: so the sums alternate between
    // the two arrays, no launch reading the one it writes, and the last segment writes carry[0] -- the caller's radiance or scratch.
    s.carry_write = (p.n_segments - 1u - i) & 1u;
    s.carry_read = (p.n_segments - i) & 1u;
    return s;
}

inline PassPlan pass_plan(const PassRequest& r) {
    PassPlan p;
    p.rpp = r.rpp; p.npix = r.npix;
    // copyToPixel inside the pass: a frame's first pass at a ray count that divides 256 or is above 256 (fused_resolves: the segment plan).  Then
    // -- and only then -- `acu` is optional: without it nothing per ray but the seed touches memory.  With `acu`, only at the counts of
    // fused_resolves_with_acu; elsewhere the accumulator is written and the separate copyToPixel reads it back.
    const bool want_out = r.has_pixel || r.has_radiance;
    p.resolves = r.inpass_resolve && (r.has_acu ? fused_resolves_with_acu(r.rpp, want_out) : r.fresh && fused_resolves(r.rpp, want_out));
    p.null_acu_ok = r.has_acu || p.resolves;
    // rays_per_pixel 1 couples the rows of a pass through seeds[col] (A10 code.cl:429): a lane cannot run its ray on alone, so mirt_render_passes
    // queues n_passes ordinary passes -- and those need the accumulator between them
    const bool single = r.rpp == 1u;
    p.null_acu_ok_passes = r.has_acu || (p.resolves && !single);
    p.route = single                                         ? ROUTE_ORDINARY_PASSES
              : !r.every                                     ? ROUTE_ONE_LAUNCH
              : r.passes > 1u && p.resolves                  ? ROUTE_ONE_LAUNCH_EVERY
                                                             : ROUTE_ORDINARY_PASSES;
    const bool cut = p.resolves && r.rpp > 256u;
    p.n_segments = cut ? r.rpp / 256u + (uint32_t)__builtin_popcount(r.rpp % 256u) : 1u;
    p.mask_unit = p.resolves ? 256u : 1u;
    const PassSegment last = pass_segment(p, p.n_segments - 1u);
    p.mask_words = last.mask_first + last.mask_words;
    p.carries = cut && r.every;
    const uint64_t frames = (uint64_t)r.passes * r.npix * 16u;
    uint64_t end = 0;
    const auto take = [&end](uint64_t bytes) { const ScratchRegion g = {end, bytes}; end += bytes; return g; };
    p.lens = take(single ? r.npix * 8u : 0u);
    p.sums = take(cut && !r.every && !r.has_radiance ? r.npix * 16u : 0u);
    p.carry[0] = take(p.carries && !r.has_radiance ? frames : 0u);
    p.carry[1] = take(p.carries ? frames : 0u);
    p.scratch_bytes = end;
    return p;
}

// Whether mirt_render_first_pass_guided writes the first-hit guides from the pass's own launch (k_fusedPass GUIDES) instead of queueing
// launch_guides behind it: the pass resolves its pixels in the kernel, as one segment and one pass, at 4, 16 or 64 rays per pixel -- a pixel's
// samples are then rays_per_pixel consecutive lanes of ONE wave, which the kernel sums by lane shuffles.  Not at 256 rays (a pixel spans four
// waves), not at a count that does not divide 256 or is above it, not beside a separate copyToPixel, not for several passes in one launch.
inline bool fused_guides_in_pass(const PassPlan& p, uint32_t passes) {
    return p.resolves && p.n_segments == 1u && passes == 1u && (p.rpp == 4u || p.rpp == 16u || p.rpp == 64u);
}
// The same question for mirt_render_passes_guided, any passes >= 1: the launch is one of mirt_render_passes's one-launch routes (with or without a
// frame after every pass) -- the guides are taken in its pass 0, which is the same whichever pass_index the batch starts at -- and the multi-pass
// kernels are the default pairing (default_pairing: MIRT_MULTIPASS_REUSE does not force the other one; the guided kernels are built for the default
// only; one pass runs the one-pass kernel, which has no pairing, so the flag does not bear on it).  With one pass and no frame after every pass this is
// fused_guides_in_pass, whatever the two flags; one pass WITH a frame after every pass is ROUTE_ORDINARY_PASSES, an ordinary pass that the guide
// launches follow.  Several passes of a scene with grids (`grids`: a set of more than
// one cell) stay on the guide launches: measured, the grid kernels' multi-pass loop with the guides in it was slower than the two launches (4 passes of
// cornell_teapot3 1080p x 16: 128.94 and 128.48 ms against 127.59 and 127.83), while scenes without grids gained.
inline bool fused_guides_in_passes(const PassPlan& p, uint32_t passes, bool default_pairing, bool grids) {
    return p.resolves && p.n_segments == 1u && (p.rpp == 4u || p.rpp == 16u || p.rpp == 64u) &&
           (p.route == ROUTE_ONE_LAUNCH || p.route == ROUTE_ONE_LAUNCH_EVERY) && (passes == 1u || (default_pairing && !grids));
}

}  // namespace pt
