// tests/pass_guided_plan_dump.cpp -- prints the route mirt_render_first_pass_guided takes (csrc/pt_pass_plan.hpp fused_guides_in_pass) for
// tests/test_pass_guided_plan.py.  Host only.
//   g++ -std=c++17 -I 2015-raytracing_amd/csrc tests/pass_guided_plan_dump.cpp -o pass_guided_plan_dump
// Requests on stdin, one per line: rpp npix passes fresh has_acu has_pixel has_radiance every inpass_resolve (the flags 0 / 1).  Per request one
// line: "<resolves> <n_segments> <guides in the pass>".
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
        printf("%d %" PRIu32 " %d\n", (int)p.resolves, p.n_segments, (int)pt::fused_guides_in_pass(p, passes));
    }
    return 0;
}
