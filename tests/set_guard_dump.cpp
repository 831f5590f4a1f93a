// tests/set_guard_dump.cpp -- compiled by tests/test_set_guard.py with a plain C++ compiler: answers questions about csrc/pt_set_guard.hpp and
// csrc/pt_windows.hpp, one per line of standard input, one line of output each, every number in hex (floats as their bit patterns):
//   guard B0 .. B7 N SANE   -> fast_ok walk_ok exit_is_far_face set_exit_is_far_face(B, N) exit_far_axes exit_up[3] delta[3] rdelta[3]
//   windows                 -> kDenLo kDenHi kPosLo kPosHi kNumLo kNumHi kTriMax kDenLoBits kDenHiBits kPosLoBits kPosHiBits
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "pt_set_guard.hpp"

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "guard")) {
            uint32_t u[8], n, sane;
            float b[8];
            for (int k = 0; k < 8; ++k)
                if (scanf("%" SCNx32, &u[k]) != 1) return 1;
            if (scanf("%" SCNx32 " %" SCNx32, &n, &sane) != 2) return 1;
            memcpy(b, u, sizeof b);
            const pt::SetGuard g = pt::set_guard(b, n, sane != 0);
            printf("%x %x %x %x %x", g.fast_ok, g.walk_ok, g.exit_is_far_face, pt::set_exit_is_far_face(b, n), g.exit_far_axes);
            for (int k = 0; k < 3; ++k) printf(" %x", bits_of(g.exit_up[k]));
            for (int k = 0; k < 3; ++k) printf(" %x", bits_of(g.delta[k]));
            for (int k = 0; k < 3; ++k) printf(" %x", bits_of(g.rdelta[k]));
            printf("\n");
        } else if (!strcmp(what, "windows")) {
            printf("%x %x %x %x %x %x %x %x %x %x %x\n", bits_of(pt::kDenLo), bits_of(pt::kDenHi), bits_of(pt::kPosLo), bits_of(pt::kPosHi), bits_of(pt::kNumLo),
                   bits_of(pt::kNumHi), bits_of(pt::kTriMax), pt::kDenLoBits, pt::kDenHiBits, pt::kPosLoBits, pt::kPosHiBits);
        } else {
            return 1;
        }
    }
    return 0;
}
