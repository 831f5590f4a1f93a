// tests/view_ao_plan_dump.cpp -- compiled by tests/test_view_ao_plan.py with a plain C++ compiler: what csrc/pt_view_plan.hpp decides for
// mirt_view_ao.  Reads one case per line from stdin, "key=value" tokens that change a valid base (ORTHOGRAPHIC, 13 x 7, k = 2, 4 AO rays of
// unbounded length, bias 0.001, both buffers given); for each prints
//   "verdict status pixels rays blocks mask_words"
// -- view_check_ao, view_status, and view_plan / view_guides_plan, the one-lane-per-pixel grid and mask the call uses (zeros where the view
// descriptor itself is refused).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "pt_view_plan.hpp"

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        pt::ViewDesc d;
        memset(&d, 0, sizeof d);
        d.struct_size = sizeof d; d.model = pt::kViewOrthographic; d.width = 13; d.height = 7; d.k = 2;
        d.right[0] = 1.0f; d.up[1] = 1.0f; d.forward[2] = -1.0f;
        d.half_w = 1.0f; d.half_h = 1.0f; d.half_angle = 1.5f; d.t_min = 0.0f; d.t_max = 10.0f; d.tone = 0.25f;
        pt::ViewAoDesc a = {(uint32_t)sizeof(pt::ViewAoDesc), 4u, INFINITY, 0.001f};
        bool seeds = true, ao_out = true;
        for (char* tok = strtok(line, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) {
            char* eq = strchr(tok, '=');
            if (!eq) continue;
            const std::string key(tok, eq - tok);
            const char* val = eq + 1;
            const uint32_t u = (uint32_t)strtoull(val, nullptr, 0);
            const float f = strtof(val, nullptr);
            if (key == "struct_size") d.struct_size = u;
            else if (key == "model") d.model = u;
            else if (key == "width") d.width = u;
            else if (key == "height") d.height = u;
            else if (key == "k") d.k = u;
            else if (key == "row0") d.row0 = u;
            else if (key == "nrows") d.nrows = u;
            else if (key == "flags") d.flags = u;
            else if (key == "half_w") d.half_w = f;
            else if (key == "half_angle") d.half_angle = f;
            else if (key == "t_min") d.t_min = f;
            else if (key == "t_max") d.t_max = f;
            else if (key == "tone") d.tone = f;
            else if (key == "forward0") d.forward[0] = f;
            else if (key == "ao_size") a.struct_size = u;
            else if (key == "samples") a.samples = u;
            else if (key == "radius") a.radius = f;
            else if (key == "bias") a.bias = f;
            else if (key == "seeds") seeds = u != 0;
            else if (key == "ao_out") ao_out = u != 0;
            else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        const pt::ViewVerdict v = pt::view_check_ao(d, a, seeds, ao_out);
        pt::ViewPlan p;
        pt::ViewGuidesPlan g;
        memset(&p, 0, sizeof p);
        memset(&g, 0, sizeof g);
        if (pt::view_check_desc(d) == pt::VIEW_OK) { p = pt::view_plan(d); g = pt::view_guides_plan(p); }
        printf("%d %d %llu %llu %u %u\n", (int)v, pt::view_status(v), (unsigned long long)p.pixels, (unsigned long long)p.rays, g.blocks, g.mask_words);
    }
    return 0;
}
