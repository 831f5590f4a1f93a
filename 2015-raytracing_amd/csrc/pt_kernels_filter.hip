// pt_kernels_filter.hip -- the edge-avoiding a-trous filter behind a few-rays-per-pixel frame (mirt_filter_atrous), guided by the first-hit
// guide buffers of pt_kernels_guides.hip.  The definition -- every operation, in order -- is the comment of mirt_filter_atrous in include/mirt.h;
// tests/filter_common.py restates it in numpy and the kernels equal that restatement bit for bit, in both libraries.
//
// Numerics: pt_post.hpp, which also holds the arithmetic this file shares with the upsampler (pt_kernels_upsample.hip) -- div_cr(), the guide
// normalisation, demodulation and its inverse, the normal and depth terms, the tone map and the final store.  The colour term is the filter's own.
//
// Working set (the context's scratch buffer, FilterArgs::work / guide): two float4 images (I.x, I.y, I.z, live ? 1 : 0) that the iterations
// alternate between, and the prepared guide (n^.x, n^.y, n^.z, z).  A tap is 32 B: its colour and, when it is live, its guide.
//
// Two structures of an iteration, the same filter_pixel() behind both (DESIGN.md section 5 has the comparison, profiles/filter/timing.json the numbers):
//   k_filterDirect  one thread per pixel, blocks of 64 x 4 pixels; a wave is 64 neighbours of one row, so each of its 24 tap reads is one
//                   contiguous 1 KB row segment served by L1 / L2 whatever the step is.
//   k_filterTiled   for step s the pixels with equal (x mod s, y mod s) form an image of their own whose 5 x 5 neighbours are the taps: a block
//                   stages a 20 x 20 tile of that lattice in LDS (colour + guide, 12.8 KB) and filters its inner 16 x 16.  Coalesced at s = 1,
//                   strided loads beyond.
// Measured at 1080p (MI355X): the tiles win at steps 1 and 2 (0.053 / 0.072 ms against 0.096 / 0.093), direct reads at 4, 8 and 16 (0.098 / 0.093 /
// 0.086 ms against 0.106 / 0.189 / 0.130): kFilterTiledSteps in pt_launch.hpp.
#include "pt_launch.hpp"
#include "pt_post.hpp"

namespace pt {

// Row tiles (mirt_filter_atrous_rows; the row arithmetic is pt_rows_plan.hpp's): the same kernels instantiated for FilterRowsArgs.  The image they
// see is the WINDOW -- every index, and every edge test, is the window's, which is wrong only in rows nobody needs -- a launch computes the rows of
// its band alone, and the last one, whose band is the own rows, stores them where the outputs, which hold no other row, have them.  For FilterArgs
// both functions fold away: the kernels behind mirt_filter_atrous are the kernels they were.
PT_DEV bool filter_in_band(const FilterArgs&, uint32_t) { return true; }
PT_DEV bool filter_in_band(const FilterRowsArgs& A, uint32_t p) { return p - A.band_row0 * A.width < A.band_nrows * A.width; }
// a block of k_filterTiled whose rows, first .. last, all lie outside the band: it stages nothing
PT_DEV bool filter_rows_outside(const FilterArgs&, int, int) { return false; }
PT_DEV bool filter_rows_outside(const FilterRowsArgs& A, int first, int last) { return last < (int)A.band_row0 || first >= (int)(A.band_row0 + A.band_nrows); }
PT_DEV uint32_t filter_out_index(const FilterArgs&, uint32_t p) { return p; }
PT_DEV uint32_t filter_out_index(const FilterRowsArgs& A, uint32_t p) { return p - A.band_row0 * A.width; }

// out = I_n (times the albedo where the image was demodulated) -> filtered, pixel
template <class ARGS>
PT_DEV void filter_finish(const ARGS& A, uint32_t p, float ox, float oy, float oz, bool live) {
    if (A.demodulate && live) {
        const float r = post_inv_hits(((const float4*)A.normal_hits)[p].w);
        post_modulate(ox, oy, oz, post_albedo(((const float4*)A.albedo_depth)[p], r));
    }
    post_store(A.filtered, A.pixel, filter_out_index(A, p), ox, oy, oz, ((const float4*)A.radiance)[p].w, A.tone);
}

// I_0 and the prepared guide of every pixel.  LAST (iterations == 0): the outputs, straight from I_0.
template <bool LAST, class ARGS = FilterArgs>
__global__ void __launch_bounds__(256) k_filterPrepare(const ARGS A) {
    const uint32_t npix = A.width * A.height;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix || !filter_in_band(A, p)) return;
    const float4 R = ((const float4*)A.radiance)[p];
    const float4 nh = ((const float4*)A.normal_hits)[p];
    const bool live = nh.w > 0.0f;
    float ix = R.x, iy = R.y, iz = R.z;
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) {
        const float4 ad = ((const float4*)A.albedo_depth)[p];
        const float r = post_inv_hits(nh.w);
        g = post_guide(nh, ad, r);
        if (A.demodulate) post_demodulate(ix, iy, iz, post_albedo(ad, r));
    }
    if (LAST) { filter_finish(A, p, ix, iy, iz, live); return; }
    ((float4*)A.work[0])[p] = make_float4(ix, iy, iz, live ? 1.0f : 0.0f);
    ((float4*)A.guide)[p] = g;
}

// One iteration of one live centre pixel.  tap(dx, dy, c, g): the colour of the tap into c, false when it is outside the image or not live,
// else its guide into g.  Returns I_{i+1}(p).
template <class Tap>
PT_DEV float4 filter_pixel(const FilterArgs& A, float inv_colour, const float4 cp, const float4 gp, const Tap& tap) {
    const float h[3] = {0.375f, 0.25f, 0.0625f};
    float izp = 0.0f;
    if (A.depth_on) izp = post_inv_depth(A.sigma_depth, gp.w);
    float sumw = 0.140625f;
    float sx = cp.x * 0.140625f, sy = cp.y * 0.140625f, sz = cp.z * 0.140625f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) continue;
            float4 cq, gq;
            if (!tap(dx, dy, cq, gq)) continue;
            const float k = h[dy < 0 ? -dy : dy] * h[dx < 0 ? -dx : dx];
            float w = k * post_normal_weight(gp, gq, A.npow);
            if (A.depth_on) w = w * post_depth_hat(gp.w, gq.w, izp);
            if (A.colour_on) {
                const float ex = (cp.x - cq.x) * A.tone, ey = (cp.y - cq.y) * A.tone, ez = (cp.z - cq.z) * A.tone;
                const float c = (ex * ex + ey * ey) + ez * ez;
                w = w * cl_max(0.0f, 1.0f - c * inv_colour);
            }
            if (w > 0.0f) {
                sumw += w;
                sx += cq.x * w; sy += cq.y * w; sz += cq.z * w;
            }
        }
    }
    return make_float4(div_cr(sx, sumw), div_cr(sy, sumw), div_cr(sz, sumw), 1.0f);
}

template <bool LAST, class ARGS>
PT_DEV void filter_store(const ARGS& A, uint32_t dst, uint32_t p, const float4 v) {
    if (LAST) filter_finish(A, p, v.x, v.y, v.z, v.w != 0.0f);
    else ((float4*)A.work[dst])[p] = v;
}

// (a) direct reads
template <bool LAST, class ARGS = FilterArgs>
__global__ void __launch_bounds__(256) k_filterDirect(const ARGS A, uint32_t src, int step, float inv_colour) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    const int W = (int)A.width, H = (int)A.height;
    if (x >= W || y >= H) return;
    const float4* const col = (const float4*)A.work[src];
    const float4* const gd = (const float4*)A.guide;
    const uint32_t p = (uint32_t)y * A.width + (uint32_t)x;
    if (!filter_in_band(A, p)) return;
    float4 v = col[p];
    if (v.w != 0.0f) {
        v = filter_pixel(A, inv_colour, v, gd[p], [&](int dx, int dy, float4& c, float4& g) {
            const int qx = x + dx * step, qy = y + dy * step;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) return false;
            const uint32_t q = (uint32_t)qy * A.width + (uint32_t)qx;
            c = col[q];
            g = gd[q];   // read whether the tap is live or not: both loads of a tap are then in flight together
            return c.w != 0.0f;
        });
    }
    filter_store<LAST>(A, src ^ 1u, p, v);
}

// (b) decimated LDS tiles.  blockIdx.x = tile column * step + (x mod step), blockIdx.y likewise.
// kTilePitch: float4 between rows of the LDS tile.  The dense tile (20: 12.8 KB); rows 32 float4 apart (20 KB) measured the same at every step
// (profiles/filter/timing_pitch32.json against timing.json)
constexpr int kTileIn = 16, kTileHalo = 2, kTileSide = kTileIn + 2 * kTileHalo, kTilePitch = kTileSide;
template <bool LAST, class ARGS = FilterArgs>
__global__ void __launch_bounds__(256) k_filterTiled(const ARGS A, uint32_t src, int step, float inv_colour) {
    __shared__ float4 s_col[kTileSide * kTilePitch];
    __shared__ float4 s_gd[kTileSide * kTilePitch];
    const int W = (int)A.width, H = (int)A.height;
    const int cx = (int)blockIdx.x % step, cy = (int)blockIdx.y % step;
    const int lx0 = ((int)blockIdx.x / step) * kTileIn - kTileHalo, ly0 = ((int)blockIdx.y / step) * kTileIn - kTileHalo;   // lattice coordinates of the tile's corner
    if (filter_rows_outside(A, (ly0 + kTileHalo) * step + cy, (ly0 + kTileHalo + kTileIn - 1) * step + cy)) return;
    const float4* const col = (const float4*)A.work[src];
    const float4* const gd = (const float4*)A.guide;
    for (int i = (int)threadIdx.x; i < kTileSide * kTileSide; i += 256) {
        const int ty = i / kTileSide, tx = i % kTileSide;
        const int lx = lx0 + tx, ly = ly0 + ty;
        const int qx = lx * step + cx, qy = ly * step + cy;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = c;   // outside the image: not live
        if (lx >= 0 && ly >= 0 && qx < W && qy < H) {
            const uint32_t q = (uint32_t)qy * A.width + (uint32_t)qx;
            c = col[q];
            g = gd[q];
        }
        s_col[ty * kTilePitch + tx] = c;
        s_gd[ty * kTilePitch + tx] = g;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 15u) + kTileHalo, ty = (int)(threadIdx.x >> 4) + kTileHalo;
    const int x = (lx0 + tx) * step + cx, y = (ly0 + ty) * step + cy;
    if (x >= W || y >= H) return;
    const uint32_t p = (uint32_t)y * A.width + (uint32_t)x;
    if (!filter_in_band(A, p)) return;
    const int at = ty * kTilePitch + tx;
    float4 v = s_col[at];
    if (v.w != 0.0f) {
        v = filter_pixel(A, inv_colour, v, s_gd[at], [&](int dx, int dy, float4& c, float4& g) {
            c = s_col[at + dy * kTilePitch + dx];
            if (c.w == 0.0f) return false;
            g = s_gd[at + dy * kTilePitch + dx];
            return true;
        });
    }
    filter_store<LAST>(A, src ^ 1u, p, v);
}

template <class ARGS>
static void launch_prepare(hipStream_t s, const ARGS& a, bool last) {
    const dim3 grid((unsigned)(((uint64_t)a.width * a.height + 255u) / 256u));
    if (last) hipLaunchKernelGGL((k_filterPrepare<true, ARGS>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_filterPrepare<false, ARGS>), grid, dim3(256), 0, s, a);
}

template <class ARGS>
static void launch_step(hipStream_t s, const ARGS& a, uint32_t src, uint32_t step_log2, float inv_colour, bool last, bool tiled) {
    const int step = 1 << step_log2;
    if (tiled) {
        const uint32_t lw = (a.width + (uint32_t)step - 1u) / (uint32_t)step, lh = (a.height + (uint32_t)step - 1u) / (uint32_t)step;
        const dim3 grid((lw + kTileIn - 1u) / kTileIn * (uint32_t)step, (lh + kTileIn - 1u) / kTileIn * (uint32_t)step);
        if (last) hipLaunchKernelGGL((k_filterTiled<true, ARGS>), grid, dim3(256), 0, s, a, src, step, inv_colour);
        else hipLaunchKernelGGL((k_filterTiled<false, ARGS>), grid, dim3(256), 0, s, a, src, step, inv_colour);
    } else {
        const dim3 grid((a.width + 63u) / 64u, (a.height + 3u) / 4u);
        if (last) hipLaunchKernelGGL((k_filterDirect<true, ARGS>), grid, dim3(256), 0, s, a, src, step, inv_colour);
        else hipLaunchKernelGGL((k_filterDirect<false, ARGS>), grid, dim3(256), 0, s, a, src, step, inv_colour);
    }
}

void launch_filterPrepare(hipStream_t s, const FilterArgs& a, bool last) { launch_prepare(s, a, last); }
void launch_filterStep(hipStream_t s, const FilterArgs& a, uint32_t src, uint32_t step_log2, float inv_colour, bool last, bool tiled) {
    launch_step(s, a, src, step_log2, inv_colour, last, tiled);
}
void launch_filterPrepareRows(hipStream_t s, const FilterRowsArgs& a, bool last) { launch_prepare(s, a, last); }
void launch_filterStepRows(hipStream_t s, const FilterRowsArgs& a, uint32_t src, uint32_t step_log2, float inv_colour, bool last, bool tiled) {
    launch_step(s, a, src, step_log2, inv_colour, last, tiled);
}

}  // namespace pt
