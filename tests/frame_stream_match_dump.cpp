// tests/frame_stream_match_dump.cpp -- runs the frame recogniser (csrc/pt_stream_match.hpp match_frame) on streams given as text, for
// tests/test_frame_stream_match.py.  Host only.  Input as tests/stream_match_dump.cpp takes it: one enqueue per line, "NAME DIM GLOBAL... ARG...",
// an argument either b<id> (a buffer) or the value's bytes in hex, and a line "end" after the last enqueue of a stream.  Output: the kernel table
// ("kernel NAME TYPE..."), then per stream "frame 0", or "frame 1 key=value ..." with everything a recognised frame is made of.
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
static int bad(const std::string& line, const char* why) { fprintf(stderr, "frame_stream_match_dump: %s: %s\n", why, line.c_str()); return 2; }

int main() {
    for (const pt::KernelSpec& k : pt::kKernels) {
        printf("kernel %s", k.name);
        for (size_t j = 0; j < k.args.size(); ++j) printf(" %c", "bufva"[k.args[j]]);
        printf("\n");
    }
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
        pt::FrameMatch m;
        const bool ok = pt::match_frame(P, &m);
        P.clear();
        if (!ok) { printf("frame 0\n"); continue; }
        printf("frame 1 assign=%" PRIu32 " width=%" PRIu32 " height=%" PRIu32 " mesh=%d mol=%d cam=%s bounds=%s pixels=%s rays=%s", m.assign, m.width, m.height,
               (int)m.mesh, (int)m.mol, hex(m.cam, 64).c_str(), hex(m.bounds, 32).c_str(), name_of(m.pixels).c_str(), name_of(m.rays).c_str());
        printf(" t_size=%s s_size=%s n_slabs=%s t_pos=%s t_normal=%s t_mindex=%s t_mcolor=%s t_slab_size=%s s_atoms=%s s_mindex=%s s_mcolor=%s s_slab_size=%s\n",
               hex(&m.t_size, 4).c_str(), hex(&m.s_size, 4).c_str(), hex(&m.n_slabs, 4).c_str(), name_of(m.t_pos).c_str(), name_of(m.t_normal).c_str(),
               name_of(m.t_mindex).c_str(), name_of(m.t_mcolor).c_str(), name_of(m.t_slab_size).c_str(), name_of(m.s_atoms).c_str(), name_of(m.s_mindex).c_str(),
               name_of(m.s_mcolor).c_str(), name_of(m.s_slab_size).c_str());
    }
    return 0;
}
