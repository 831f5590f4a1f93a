// tests/view_plan_dump.cpp -- compiled by tests/test_view_plan.py with a plain C++ compiler: what csrc/pt_view_plan.hpp decides.  Reads one
// case per line from stdin, "key=value" tokens that change a valid base descriptor (ORTHOGRAPHIC, 13 x 7, k = 2, seeds, radiance and pixel all
// given); for each prints "verdict status nrows rpp pixels rays blocks pixels_per_block last_block_pixels mask_words" -- the plan only where the
// descriptor itself passed (zeros otherwise).  Floats are strtof's: inf, nan and hexadecimal forms work.
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
        bool seeds = true, radiance = true, pixel = true, rays_call = false;
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
            else if (key == "half_h") d.half_h = f;
            else if (key == "half_angle") d.half_angle = f;
            else if (key == "t_min") d.t_min = f;
            else if (key == "t_max") d.t_max = f;
            else if (key == "tone") d.tone = f;
            else if (key == "seeds") seeds = u != 0;
            else if (key == "radiance") radiance = u != 0;
            else if (key == "pixel") pixel = u != 0;
            else if (key == "rays_call") rays_call = u != 0;
            else if (key.size() > 1 && key[key.size() - 1] >= '0' && key[key.size() - 1] <= '2') {
                const int c = key[key.size() - 1] - '0';
                const std::string v = key.substr(0, key.size() - 1);
                if (v == "eye") d.eye[c] = f;
                else if (v == "right") d.right[c] = f;
                else if (v == "up") d.up[c] = f;
                else if (v == "forward") d.forward[c] = f;
                else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
            } else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        const pt::ViewVerdict v = rays_call ? pt::view_check_desc(d) : pt::view_check_render(d, seeds, radiance, pixel);
        pt::ViewPlan p;
        memset(&p, 0, sizeof p);
        if (pt::view_check_desc(d) == pt::VIEW_OK) p = pt::view_plan(d);
        printf("%d %d %u %u %llu %llu %u %u %u %u\n", (int)v, pt::view_status(v), p.nrows, p.rpp, (unsigned long long)p.pixels, (unsigned long long)p.rays, p.blocks,
               p.pixels_per_block, p.last_block_pixels, p.mask_words);
    }
    return 0;
}
