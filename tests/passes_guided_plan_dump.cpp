// tests/passes_guided_plan_dump.cpp -- prints the route mirt_render_passes_guided takes (csrc/pt_pass_plan.hpp fused_guides_in_passes) for
// tests/test_passes_guided_plan.py.  Host only.
//   g++ -std=c++17 -I 2015-raytracing_amd/csrc tests/passes_guided_plan_dump.cpp -o passes_guided_plan_dump
// Requests on stdin, one per line: rpp npix passes fresh has_acu has_pixel has_radiance every inpass_resolve default_pairing grids (the flags 0 / 1).
// Per request one line: "<resolves> <n_segments> <route> <fused_guides_in_pass> <fused_guides_in_passes>".
#include <inttypes.h>
#include <stdio.h>

#include "pt_pass_plan.hpp"

int main() {
    uint32_t rpp, passes;
    uint64_t npix;
    int fresh, acu, pixel, radiance, every, inpass, pairing, grids;
    while (scanf("%" SCNu32 " %" SCNu64 " %" SCNu32 " %d %d %d %d %d %d %d %d", &rpp, &npix, &passes, &fresh, &acu, &pixel, &radiance, &every, &inpass, &pairing, &grids) == 11) {
        pt::PassRequest r;
        r.rpp = rpp; r.npix = npix; r.passes = passes;
        r.fresh = fresh != 0; r.has_acu = acu != 0; r.has_pixel = pixel != 0; r.has_radiance = radiance != 0;
        r.every = every != 0; r.inpass_resolve = inpass != 0;
        const pt::PassPlan p = pt::pass_plan(r);
        printf("%d %" PRIu32 " %d %d %d\n", (int)p.resolves, p.n_segments, (int)p.route, (int)pt::fused_guides_in_pass(p, passes),
               (int)pt::fused_guides_in_passes(p, passes, pairing != 0, grids != 0));
    }
    return 0;
}
