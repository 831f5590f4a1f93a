// tests/upsample_taps_dump.cpp -- compiled by tests/test_upsample_taps.py with a plain C++ compiler: prints what csrc/pt_upsample_taps.hpp
// computes, one line per (factor, width, x): "f width x X0 m nearest", for every x of every width f * 1 .. f * 9 of every factor 2 .. 4, then one
// line per (factor, extent) "low f extent low_extent" for extents 0 .. 40, then "factor_ok f ok" for f = 0 .. 6.
#include <stdio.h>

#include "pt_upsample_taps.hpp"

int main() {
    for (uint32_t f = pt::kUpsampleMinFactor; f <= pt::kUpsampleMaxFactor; ++f)
        for (uint32_t wl = 1; wl <= 9; ++wl)
            for (uint32_t x = 0; x < wl * f; ++x) {
                const pt::UpsampleTap t = pt::upsample_tap(x, f);
                printf("%u %u %u %d %d %u\n", f, wl * f, x, t.q0, t.m, pt::upsample_nearest(x, f));
            }
    for (uint32_t f = pt::kUpsampleMinFactor; f <= pt::kUpsampleMaxFactor; ++f)
        for (uint32_t n = 0; n <= 40; ++n) printf("low %u %u %u\n", f, n, pt::upsample_low_extent(n, f));
    for (uint32_t f = 0; f <= 6; ++f) printf("factor_ok %u %d\n", f, pt::upsample_factor_ok(f) ? 1 : 0);
    return 0;
}
