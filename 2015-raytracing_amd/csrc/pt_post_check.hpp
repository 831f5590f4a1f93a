// pt_post_check.hpp -- the argument rules the post-process stage's two entry points share (mirt_filter_atrous, mirt_upsample_guided; include/mirt.h),
// each stated once.  Plain values -- extents, the two scalars, byte ranges as (address, length, present) -- and no HIP header and no device, so a
// plain C++ compiler builds it and tests/test_post_check.py checks it on the CPU (tests/post_check_dump.cpp).  mirt_abi.cpp is the caller and
// owns the messages; what is one entry point's own (iterations and structure flags, the factor) stays there.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace pt {

constexpr uint32_t kPostMaxExtent = 65535u;             // a side of the image: the kernels' grids and their int pixel coordinates rely on it
constexpr uint32_t kPostMaxNormalPowerLog2 = 7u;        // MIRT_FILTER_MAX_NORMAL_POWER_LOG2

enum PostExtent { POST_EXTENT_OK, POST_EXTENT_EMPTY, POST_EXTENT_TOO_LARGE };
inline PostExtent post_extent(uint32_t width, uint32_t height) {
    if (!width || !height) return POST_EXTENT_EMPTY;
    return width > kPostMaxExtent || height > kPostMaxExtent ? POST_EXTENT_TOO_LARGE : POST_EXTENT_OK;
}
inline bool post_normal_power_ok(uint32_t normal_power_log2) { return normal_power_log2 <= kPostMaxNormalPowerLog2; }
// Finite and positive (a NaN fails both comparisons).  `tone` must be; a sigma is a width -- its edge term is on -- iff it is.
inline bool post_finite_positive(float v) { return v > 0.0f && v <= 3.402823466e+38f; }

// Aliasing.  An output is read by nobody and no input is written: no present output's bytes meet an input's, and no two outputs' meet.
struct PostRange {
    uint64_t addr, bytes;
    bool present;            // false: an output the caller did not ask for
};
inline bool post_ranges_meet(const PostRange& a, const PostRange& b) {
    return a.present && b.present && a.addr < b.addr + b.bytes && b.addr < a.addr + a.bytes;
}
inline bool post_any_output(const PostRange* out, size_t n_out) {
    for (size_t o = 0; o < n_out; ++o)
        if (out[o].present) return true;
    return false;
}
enum PostAlias { POST_ALIAS_NONE, POST_ALIAS_OUTPUT_INPUT, POST_ALIAS_OUTPUTS };
inline PostAlias post_alias(const PostRange* in, size_t n_in, const PostRange* out, size_t n_out) {
    for (size_t o = 0; o < n_out; ++o)
        for (size_t i = 0; i < n_in; ++i)
            if (post_ranges_meet(out[o], in[i])) return POST_ALIAS_OUTPUT_INPUT;
    for (size_t o = 0; o < n_out; ++o)
        for (size_t p = o + 1; p < n_out; ++p)
            if (post_ranges_meet(out[o], out[p])) return POST_ALIAS_OUTPUTS;
    return POST_ALIAS_NONE;
}

}  // namespace pt
