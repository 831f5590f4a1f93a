// tests/view_guides_plan_dump.cpp -- compiled by tests/test_view_guides_plan.py with a plain C++ compiler: what csrc/pt_view_plan.hpp decides for
// mirt_view_guides and mirt_render_view_guided.  Reads one case per line from stdin, "key=value" tokens that change a valid base (ORTHOGRAPHIC,
// 13 x 7, k = 2, every buffer given, no grids, the switch on); for each prints
//   "guides_verdict guides_status guided_verdict guided_status in_pass blocks mask_words"
// -- view_check_guides, view_check_render_guided, view_guides_in_pass(k * k, grids, env) and view_guides_plan (zeros where the descriptor itself
// is refused).
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
        bool seeds = true, radiance = true, pixel = true, nh = true, ad = true, grids = false, env = true;
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
            else if (key == "seeds") seeds = u != 0;
            else if (key == "radiance") radiance = u != 0;
            else if (key == "pixel") pixel = u != 0;
            else if (key == "nh") nh = u != 0;
            else if (key == "ad") ad = u != 0;
            else if (key == "grids") grids = u != 0;
            else if (key == "env") env = u != 0;
            else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        const pt::ViewVerdict a = pt::view_check_guides(d, nh, ad), b = pt::view_check_render_guided(d, seeds, radiance, pixel, nh, ad);
        pt::ViewGuidesPlan g;
        memset(&g, 0, sizeof g);
        if (pt::view_check_desc(d) == pt::VIEW_OK) g = pt::view_guides_plan(pt::view_plan(d));
        printf("%d %d %d %d %d %u %u\n", (int)a, pt::view_status(a), (int)b, pt::view_status(b), pt::view_guides_in_pass(d.k * d.k, grids, env) ? 1 : 0, g.blocks,
               g.mask_words);
    }
    return 0;
}
