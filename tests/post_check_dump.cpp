// tests/post_check_dump.cpp -- compiled by tests/test_post_check.py with a plain C++ compiler: answers questions about csrc/pt_post_check.hpp, one
// per line of standard input, one line of output each:
//   extent W H                     -> the PostExtent code (0 ok, 1 empty, 2 too large)
//   power P                        -> 1 when post_normal_power_ok
//   positive BITS                  -> 1 when the float with these bits (hex) is post_finite_positive
//   alias NIN NOUT (ADDR LEN PRESENT) x (NIN + NOUT)   -> "<PostAlias code> <post_any_output>", addresses and lengths in hex
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "pt_post_check.hpp"

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "extent")) {
            uint32_t w, h;
            if (scanf("%" SCNu32 " %" SCNu32, &w, &h) != 2) return 1;
            printf("%d\n", (int)pt::post_extent(w, h));
        } else if (!strcmp(what, "power")) {
            uint32_t p;
            if (scanf("%" SCNu32, &p) != 1) return 1;
            printf("%d\n", pt::post_normal_power_ok(p) ? 1 : 0);
        } else if (!strcmp(what, "positive")) {
            uint32_t bits;
            float v;
            if (scanf("%" SCNx32, &bits) != 1) return 1;
            memcpy(&v, &bits, sizeof v);
            printf("%d\n", pt::post_finite_positive(v) ? 1 : 0);
        } else if (!strcmp(what, "alias")) {
            size_t n_in, n_out;
            pt::PostRange r[16];
            if (scanf("%zu %zu", &n_in, &n_out) != 2 || n_in + n_out > 16) return 1;
            for (size_t i = 0; i < n_in + n_out; ++i) {
                int present;
                if (scanf("%" SCNx64 " %" SCNx64 " %d", &r[i].addr, &r[i].bytes, &present) != 3) return 1;
                r[i].present = present != 0;
            }
            printf("%d %d\n", (int)pt::post_alias(r, n_in, r + n_in, n_out), pt::post_any_output(r + n_in, n_out) ? 1 : 0);
        } else {
            return 1;
        }
    }
    return 0;
}
