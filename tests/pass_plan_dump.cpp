// tests/pass_plan_dump.cpp -- prints the launch plan of a fused pass (csrc/pt_pass_plan.hpp) as text, for tests/test_pass_plan.py.  Host only.
//   g++ -std=c++17 -I 2015-raytracing_amd/csrc tests/pass_plan_dump.cpp -o pass_plan_dump
// Requests on stdin, one per line: rpp npix passes fresh has_acu has_pixel has_radiance every inpass_resolve (the flags 0 / 1).  Per request one
// "plan" line, then one "seg" line per segment, in order.
#include <inttypes.h>
#include <stdio.h>

#include "pt_pass_plan.hpp"

int main() {
    uint32_t rpp, passes;
    uint64_t npix;
    int fresh, acu, pixel, radiance, every, inpass;
    while (scanf("%" SCNu32 " %" SCNu64 " %" SCNu32 " %d %d %d %d %d %d", &rpp, &npix, &passes, &fresh, &acu, &pixel, &radiance, &every, &inpass) == 9) {
        pt::PassRequest r;
        r.rpp = rpp; r.npix = npix; r.passes = passes;
        r.fresh = fresh != 0; r.has_acu = acu != 0; r.has_pixel = pixel != 0; r.has_radiance = radiance != 0;
        r.every = every != 0; r.inpass_resolve = inpass != 0;
        const pt::PassPlan p = pt::pass_plan(r);
        printf("plan rpp=%" PRIu32 " npix=%" PRIu64 " resolves=%d null_acu_ok=%d null_acu_ok_passes=%d route=%d n_segments=%" PRIu32 " mask_words=%" PRIu32
               " mask_unit=%" PRIu32 " carries=%d scratch=%" PRIu64 " lens=%" PRIu64 "+%" PRIu64 " sums=%" PRIu64 "+%" PRIu64 " carry0=%" PRIu64 "+%" PRIu64
               " carry1=%" PRIu64 "+%" PRIu64 "\n",
               p.rpp, p.npix, (int)p.resolves, (int)p.null_acu_ok, (int)p.null_acu_ok_passes, (int)p.route, p.n_segments, p.mask_words, p.mask_unit,
               (int)p.carries, p.scratch_bytes, p.lens.off, p.lens.bytes, p.sums.off, p.sums.bytes, p.carry[0].off, p.carry[0].bytes, p.carry[1].off,
               p.carry[1].bytes);
        for (uint32_t i = 0; i < p.n_segments; ++i) {
            const pt::PassSegment s = pt::pass_segment(p, i);
            printf("seg %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %d %" PRIu32 " %" PRIu32 "\n", s.off, s.len, s.pitch, s.mask_first,
                   s.mask_words, (int)s.writes_pixel, s.carry_write, s.carry_read);
        }
    }
    return 0;
}
