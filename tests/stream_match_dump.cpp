// tests/stream_match_dump.cpp -- runs the enqueue-stream recogniser (csrc/pt_stream_match.hpp) on streams given as text, for
// tests/test_stream_match.py.  Host only.
//   g++ -std=c++17 -I 2015-raytracing_amd/csrc tests/stream_match_dump.cpp -o stream_match_dump
// First the kernel table, one "kernel NAME TYPE..." line per row (b u f v a: buffer, uint, float, float16, AABB), and a "limits" line.  Then, for
// every stream on stdin -- one enqueue per line, "NAME DIM GLOBAL... ARG...", an argument either b<id> (a buffer) or the value's bytes in hex, and
// a line "end" after the last enqueue -- "pass 0", or "pass 1 ..." followed by one "set" line per primitive set and one "light" line per light.
// A malformed line (unknown kernel, wrong argument count, size or kind) ends the program with status 2: the test builds well-formed streams only.
#include <inttypes.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "pt_stream_match.hpp"

static mirt_buf* handle(unsigned long id) { return reinterpret_cast<mirt_buf*>((uintptr_t)(id + 1) * 64); }   // distinct, never null, never dereferenced
static std::string name_of(const mirt_buf* b) { return b ? "b" + std::to_string((uintptr_t)b / 64 - 1) : "-"; }
static std::string hex(const void* p, size_t n) {
    static const char d[] = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += d[((const uint8_t*)p)[i] >> 4]; s += d[((const uint8_t*)p)[i] & 15]; }
    return s;
}
static int bad(const std::string& line, const char* why) { fprintf(stderr, "stream_match_dump: %s: %s\n", why, line.c_str()); return 2; }

int main() {
    for (const pt::KernelSpec& k : pt::kKernels) {
        printf("kernel %s", k.name);
        for (size_t j = 0; j < k.args.size(); ++j) printf(" %c", "bufva"[k.args[j]]);
        printf("\n");
    }
    printf("limits lights=%d meshes=%d\n", MIRT_MAX_LIGHTS, MIRT_MAX_MESHES);
    std::vector<pt::Enqueue> P;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name, tok;
        if (!(in >> name)) continue;
        if (name != "end") {
            pt::Enqueue e;
            e.spec = nullptr;
            for (const pt::KernelSpec& k : pt::kKernels) if (name == k.name) e.spec = &k;
            if (!e.spec || !(in >> e.dim) || e.dim < 1 || e.dim > 3) return bad(line, "unknown kernel or bad dim");
            for (unsigned d = 0; d < 3; ++d) { e.g[d] = 1; if (d < e.dim && !(in >> e.g[d])) return bad(line, "missing global size"); }
            e.args.resize(e.spec->args.size());
            for (size_t j = 0; j < e.args.size(); ++j) {
                if (!(in >> tok)) return bad(line, "too few arguments");
                const size_t bytes = pt::arg_size(e.spec->args[j]);
                if (e.spec->args[j] == pt::A_BUF) {
                    if (tok[0] != 'b') return bad(line, "buffer expected");
                    e.args[j].buf = handle(std::stoul(tok.substr(1)));
                } else {
                    if (tok.size() != 2 * bytes) return bad(line, "wrong argument size");
                    uint8_t* out = reinterpret_cast<uint8_t*>(&e.args[j].val);
                    for (size_t b = 0; b < bytes; ++b) out[b] = (uint8_t)std::stoul(tok.substr(2 * b, 2), nullptr, 16);
                }
                e.args[j].set = true;
            }
            if (in >> tok) return bad(line, "too many arguments");
            P.push_back(e);
            continue;
        }
        pt::PassMatch m;
        const bool ok = pt::match_pass(P, &m);
        P.clear();
        if (!ok) { printf("pass 0\n"); continue; }
        printf("pass 1 width=%" PRIu32 " height=%" PRIu32 " rpp=%" PRIu32 " bounces=%" PRIu32 " spheres=%d triangles=%d cam=%s bounds=%s focal_length=%s lens_rad=%s tone=%s",
               m.width, m.height, m.rpp, m.bounces, (int)m.spheres, (int)m.triangles, hex(m.cam, 64).c_str(), hex(m.scene_bounds, 32).c_str(),
               hex(&m.focal_length, 4).c_str(), hex(&m.lens_rad, 4).c_str(), hex(&m.tone, 4).c_str());
        printf(" seeds=%s rays=%s pois=%s shadow=%s acu=%s material=%s pixel=%s\n", name_of(m.seeds).c_str(), name_of(m.rays).c_str(), name_of(m.pois).c_str(),
               name_of(m.shadow).c_str(), name_of(m.acu).c_str(), name_of(m.material).c_str(), name_of(m.pixel).c_str());
        for (const mirt_grid& g : m.sets)
            printf("set prims=%s normals=%s matid=%s off=%s bounds=%s n_slabs=%s mesh_matid=%s\n", name_of(g.prims).c_str(), name_of(g.normals).c_str(),
                   name_of(g.matid).c_str(), name_of(g.cell_offsets).c_str(), hex(g.bounds, 32).c_str(), hex(&g.n_slabs, 4).c_str(), hex(&g.mesh_matid, 4).c_str());
        for (const mirt_light& l : m.lights)
            printf("light light=%s shadow=%s scene=%s\n", hex(l.light, 64).c_str(), hex(l.shadow, 64).c_str(), hex(l.scene, 64).c_str());
    }
    return 0;
}
