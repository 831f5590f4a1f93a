// pt_rows_plan.hpp -- the row arithmetic of the post-process stage in row tiles (mirt_filter_atrous_rows, mirt_upsample_guided_rows,
// mirt_exchange_rows; include/mirt.h): which rows of its input a band of output rows depends on, the argument rules of the two _rows calls, and
// the plan of a halo exchange -- which copies fill every context's window from the tiles that own its rows.  Plain integers: no HIP header and
// no device, so a plain C++ compiler builds it and tests/test_rows_plan.py checks it on the CPU (tests/rows_plan_dump.cpp).  mirt_abi.cpp is the
// caller and owns the messages.
//
// Why a window is enough.  Neither kernel depends on a pixel's absolute row except at the image's top and bottom edges.  Iteration i of the
// filter reads rows within 2 * 2^i of the row it writes, so rows [row0, row0 + nrows) after n iterations depend on the input rows within
// H = 2 * (2^n - 1) of them and on nothing else: filtering the window [row0 - H, row0 + nrows + H), clamped to the image, as if it were an image
// gives the frame's rows bit for bit (a clamped edge IS the image's edge; at an edge that is not, the wrong rows are rows nobody needs).  High row
// y of the upsampler reads low rows Y0(y), Y0(y) + 1 and y div f, the last always one of the first two inside the image.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pt_upsample_taps.hpp"

namespace pt {

constexpr uint32_t kRowsMaxIterations = 5u;   // MIRT_FILTER_MAX_ITERATIONS

struct RowRange {
    uint32_t row0, nrows;
};

// H: how far, in rows, n iterations reach
constexpr uint32_t filter_halo_rows(uint32_t iterations) { return 2u * ((1u << iterations) - 1u); }

// [row0 - H, row0 + nrows + H) clamped to the image; {0, 0} for rows that are empty or not the image's, or more iterations than the filter has
inline RowRange filter_window(uint32_t image_height, uint32_t row0, uint32_t nrows, uint32_t iterations) {
    if (!nrows || iterations > kRowsMaxIterations || (uint64_t)row0 + nrows > image_height) return RowRange{0u, 0u};
    const uint32_t h = filter_halo_rows(iterations);
    const uint32_t lo = row0 > h ? row0 - h : 0u;
    const uint64_t end = (uint64_t)row0 + nrows + h;
    const uint32_t hi = end < image_height ? (uint32_t)end : image_height;
    return RowRange{lo, hi - lo};
}

// the rows iteration i of n has to compute, so that the iterations behind it find what they read: the own rows and 2 * (2^n - 2^(i + 1)) around
// them, inside the window [win_row0, win_row0 + win_nrows).  i == n (the prepare): every row the first iteration reads, filter_window itself.
inline RowRange filter_band(uint32_t win_row0, uint32_t win_nrows, uint32_t row0, uint32_t nrows, uint32_t iterations, uint32_t i) {
    const uint32_t reach = i >= iterations ? filter_halo_rows(iterations) : 2u * ((1u << iterations) - (1u << (i + 1u)));
    const uint32_t lo = row0 > win_row0 + reach ? row0 - reach : win_row0;
    const uint64_t end = (uint64_t)row0 + nrows + reach, win_end = (uint64_t)win_row0 + win_nrows;
    return RowRange{lo, (uint32_t)(end < win_end ? end : win_end) - lo};
}

// the low rows that high rows [row0, row0 + nrows) of a `height`-row image read: max(0, Y0(row0)) up to min(hl, Y0(row0 + nrows - 1) + 2)
inline RowRange upsample_low_window(uint32_t height, uint32_t factor, uint32_t row0, uint32_t nrows) {
    if (!upsample_factor_ok(factor) || !nrows || height > 65535u || (uint64_t)row0 + nrows > height) return RowRange{0u, 0u};
    const uint32_t hl = upsample_low_extent(height, factor);
    if (!hl) return RowRange{0u, 0u};
    const int32_t first = upsample_tap(row0, factor).q0, last = upsample_tap(row0 + nrows - 1u, factor).q0 + 2;
    const uint32_t lo = first < 0 ? 0u : (uint32_t)first;
    const uint32_t hi = (uint32_t)last < hl ? (uint32_t)last : hl;
    return RowRange{lo, hi - lo};
}

// ---- the argument rules of the two _rows calls
inline bool rows_inside(uint32_t extent, uint32_t row0, uint32_t nrows) { return (uint64_t)row0 + nrows <= extent; }
inline bool rows_contain(uint32_t row0, uint32_t nrows, const RowRange& need) {
    return row0 <= need.row0 && (uint64_t)need.row0 + need.nrows <= (uint64_t)row0 + nrows;
}

enum RowsVerdict {
    ROWS_OK,
    ROWS_EMPTY,            // no rows asked for, or an empty window
    ROWS_OUTSIDE_IMAGE,    // the rows asked for, or the window, reach outside the image
    ROWS_WINDOW_SHORT      // the window does not contain every row the rows asked for depend on
};
// mirt_filter_atrous_rows: rows [row0, row0 + nrows) of an image_height-row image from the input rows [win_row0, win_row0 + win_nrows)
inline RowsVerdict filter_rows_check(uint32_t image_height, uint32_t win_row0, uint32_t win_nrows, uint32_t row0, uint32_t nrows, uint32_t iterations) {
    if (!nrows || !win_nrows) return ROWS_EMPTY;
    if (!rows_inside(image_height, row0, nrows) || !rows_inside(image_height, win_row0, win_nrows)) return ROWS_OUTSIDE_IMAGE;
    return rows_contain(win_row0, win_nrows, filter_window(image_height, row0, nrows, iterations)) ? ROWS_OK : ROWS_WINDOW_SHORT;
}
// mirt_upsample_guided_rows: high rows [row0, row0 + nrows) of a `height`-row image (a multiple of the factor) from the low rows [lo_row0, lo_row0 + lo_nrows)
inline RowsVerdict upsample_rows_check(uint32_t height, uint32_t factor, uint32_t row0, uint32_t nrows, uint32_t lo_row0, uint32_t lo_nrows) {
    if (!nrows || !lo_nrows) return ROWS_EMPTY;
    if (!rows_inside(height, row0, nrows) || !rows_inside(upsample_low_extent(height, factor), lo_row0, lo_nrows)) return ROWS_OUTSIDE_IMAGE;
    return rows_contain(lo_row0, lo_nrows, upsample_low_window(height, factor, row0, nrows)) ? ROWS_OK : ROWS_WINDOW_SHORT;
}

// ---- the exchange plan.  Context i owns image rows [src_row0[i], + src_nrows[i]) -- the first rows of its source buffer -- and wants image rows
// [dst_row0[i], + dst_nrows[i]) in its destination buffer; 0 rows: it owns nothing / wants nothing.  Every wanted row is copied from the context
// that owns it, the context's own rows included; a window may span several owners (tiles can be shorter than the halo).
struct RowCopy {
    uint32_t src_ctx, src_row;   // the row of the SOURCE BUFFER the copy starts at (image row - src_row0[src_ctx])
    uint32_t dst_ctx, dst_row;   // the row of the DESTINATION BUFFER (image row - dst_row0[dst_ctx])
    uint32_t nrows;
};
enum ExchangeVerdict {
    EXCHANGE_OK,
    EXCHANGE_OWNERS_OVERLAP,   // two contexts own the same image row: *at = the higher of the two contexts
    EXCHANGE_ROW_UNOWNED       // a wanted row that nobody owns: *at = the context that wants it
};
// the copies, by destination context and then by image row, appended to `out` (left empty on a refusal)
inline ExchangeVerdict exchange_plan(const uint32_t* src_row0, const uint32_t* src_nrows, const uint32_t* dst_row0, const uint32_t* dst_nrows, size_t n,
                                     std::vector<RowCopy>* out, size_t* at) {
    out->clear();
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < i; ++j)
            if (src_nrows[i] && src_nrows[j] && src_row0[i] < (uint64_t)src_row0[j] + src_nrows[j] && src_row0[j] < (uint64_t)src_row0[i] + src_nrows[i]) {
                if (at) *at = i;
                return EXCHANGE_OWNERS_OVERLAP;
            }
    for (size_t d = 0; d < n; ++d) {
        uint64_t row = dst_row0[d];
        const uint64_t end = row + dst_nrows[d];
        while (row < end) {
            size_t s = 0;
            while (s < n && !(src_nrows[s] && src_row0[s] <= row && row < (uint64_t)src_row0[s] + src_nrows[s])) ++s;
            if (s == n) {
                out->clear();
                if (at) *at = d;
                return EXCHANGE_ROW_UNOWNED;
            }
            const uint64_t owner_end = (uint64_t)src_row0[s] + src_nrows[s], stop = owner_end < end ? owner_end : end;
            out->push_back(RowCopy{(uint32_t)s, (uint32_t)(row - src_row0[s]), (uint32_t)d, (uint32_t)(row - dst_row0[d]), (uint32_t)(stop - row)});
            row = stop;
        }
    }
    return EXCHANGE_OK;
}

}  // namespace pt
