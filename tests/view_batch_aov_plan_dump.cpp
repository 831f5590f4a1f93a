// tests/view_batch_aov_plan_dump.cpp -- compiled by tests/test_view_batch_aov_plan.py with a plain C++ compiler: what csrc/pt_view_plan.hpp
// decides for mirt_view_guides_batch, mirt_view_ao_batch and mirt_render_view_guided_batch.  Reads one case per line from stdin, "key=value"
// tokens that change a valid base (EQUIRECT, 13 x 7, k = 2, three finite cameras, every buffer given, AO of 4 samples, radius 1, bias 0.001);
// for each prints
//   "guides_verdict guides_status ao_verdict ao_status guided_verdict guided_status bad_guides bad_ao bad_guided nrows pixels blocks mask_words route"
// -- view_check_guides_batch, view_check_ao_batch, view_check_render_guided_batch, the frame each names (-1: none) and view_batch_pixel_plan of
// view_batch_plan (zeros where the batch itself is refused).  n=N: N cameras; cameras=0: the pointer is null; camF.S=V: slot S (0 .. 11) of
// frame F's camera; basisS=V: slot S of the DESCRIPTOR's eye, right, up, forward, which the batch calls do not read; nh / ad / seeds / radiance
// / pixel / ao_seeds / ao_out = 0: that buffer is not given; ao_size, ao_samples, ao_radius, ao_bias: the AO descriptor's fields.  route:
// view_batch_guides_in_pass(k * k, grids, env) -- grids=1: a set of more than one cell; env=0: MIRT_GUIDED_VIEW=0.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pt_view_plan.hpp"

int main() {
    static_assert(sizeof(pt::ViewCamera) == 48, "mirt_view_camera is 48 bytes");
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        pt::ViewDesc d;
        memset(&d, 0, sizeof d);
        d.struct_size = sizeof d; d.model = pt::kViewEquirect; d.width = 13; d.height = 7; d.k = 2;
        d.right[0] = 1.0f; d.up[1] = 1.0f; d.forward[2] = -1.0f;
        d.half_w = 1.0f; d.half_h = 1.0f; d.half_angle = 1.5f; d.t_min = 0.0f; d.t_max = 10.0f; d.tone = 0.25f;
        pt::ViewAoDesc ao;
        ao.struct_size = sizeof ao; ao.samples = 4; ao.radius = 1.0f; ao.bias = 0.001f;
        bool seeds = true, radiance = true, pixel = true, have_cameras = true, nh = true, ad = true, ao_seeds = true, ao_out = true;
        uint32_t n = 3;
        bool grids = false, env = true;
        struct Edit { uint32_t frame, slot; float v; };
        std::vector<Edit> edits;
        for (char* tok = strtok(line, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) {
            char* eq = strchr(tok, '=');
            if (!eq) continue;
            const std::string key(tok, eq - tok);
            const char* val = eq + 1;
            const uint32_t u = (uint32_t)strtoull(val, nullptr, 0);
            const float f = strtof(val, nullptr);
            unsigned fr = 0, slot = 0;
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
            else if (key == "seeds") seeds = u != 0;
            else if (key == "radiance") radiance = u != 0;
            else if (key == "pixel") pixel = u != 0;
            else if (key == "nh") nh = u != 0;
            else if (key == "ad") ad = u != 0;
            else if (key == "ao_seeds") ao_seeds = u != 0;
            else if (key == "ao_out") ao_out = u != 0;
            else if (key == "ao_size") ao.struct_size = u;
            else if (key == "ao_samples") ao.samples = u;
            else if (key == "ao_radius") ao.radius = f;
            else if (key == "ao_bias") ao.bias = f;
            else if (key == "grids") grids = u != 0;
            else if (key == "env") env = u != 0;
            else if (key == "n") n = u;
            else if (key == "cameras") have_cameras = u != 0;
            else if (sscanf(key.c_str(), "cam%u.%u", &fr, &slot) == 2 && slot < 12) edits.push_back({fr, slot, f});
            else if (sscanf(key.c_str(), "basis%u", &slot) == 1 && slot < 12) (&d.eye[0])[slot] = f;
            else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        // the table is not read beyond the refusal that precedes it: a batch over the ray limit is tested with a short one
        const uint32_t held = n < 4096u ? n : 4096u;
        std::vector<pt::ViewCamera> cams(held);
        for (uint32_t f = 0; f < held; ++f) {
            memset(&cams[f], 0, sizeof cams[f]);
            cams[f].eye[0] = (float)f; cams[f].right[0] = 1.0f; cams[f].up[1] = 1.0f; cams[f].forward[2] = -1.0f;
        }
        for (const Edit& e : edits)
            if (e.frame < held) (&cams[e.frame].eye[0])[e.slot] = e.v;
        const pt::ViewCamera* table = have_cameras ? cams.data() : nullptr;
        uint32_t bad_g = 0xFFFFFFFFu, bad_a = 0xFFFFFFFFu, bad_r = 0xFFFFFFFFu;
        if (n > held && pt::view_check_batch(d, nullptr, n) == pt::VIEW_BATCH_NO_CAMERAS) { fprintf(stderr, "case would read %u cameras\n", n); return 2; }
        const pt::ViewVerdict g = pt::view_check_guides_batch(d, table, n, nh, ad, &bad_g);
        const pt::ViewVerdict a = pt::view_check_ao_batch(d, table, n, ao, ao_seeds, ao_out, &bad_a);
        const pt::ViewVerdict r = pt::view_check_render_guided_batch(d, table, n, seeds, radiance, pixel, nh, ad, &bad_r);
        pt::ViewBatchPlan p;
        memset(&p, 0, sizeof p);
        pt::ViewGuidesPlan q = {0u, 0u};
        if (pt::view_check_batch(d, table, n) == pt::VIEW_OK) { p = pt::view_batch_plan(d, n); q = pt::view_batch_pixel_plan(p); }
        printf("%d %d %d %d %d %d %d %d %d %u %llu %u %u %d\n", (int)g, pt::view_status(g), (int)a, pt::view_status(a), (int)r, pt::view_status(r), (int)bad_g, (int)bad_a,
               (int)bad_r, p.all.nrows, (unsigned long long)p.all.pixels, q.blocks, q.mask_words, (int)pt::view_batch_guides_in_pass(d.k * d.k, grids, env));
    }
    return 0;
}
