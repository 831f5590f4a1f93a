// pt_stream_match.hpp -- the reference's kernels as the host sees them (names, argument lists, named argument indices), an enqueue as the runtime
// holds it back, and the recogniser of command-stream fusion: is a held stream exactly executeRender's pass (A10 code.js:1806-1854) over one
// consistent set of buffers?  A wrong "yes" changes what the caller's buffers hold -- the fused launch never writes rays, pois or the shadow rays --
// so this is a pure function of the stream: buffer handles are compared, never dereferenced, there is no HIP header and no device, a plain C++
// compiler builds it and tests/test_stream_match.py checks it on the CPU against the reference host's own recorded streams.
// mirt_abi.cpp is the caller: mirt_kernel_* and launch_kernel read the table and the indices, try_fuse_pass runs what match_pass accepts.
#pragma once
#include "../../include/mirt.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pt {

enum ArgType { A_BUF, A_U32, A_F32, A_F16, A_AABB };
enum KernelId {
    K_sizeofRay, K_sizeofPoi, K_initAcu, K_initTrace, K_sphereTrace, K_triangleTrace, K_meshTrace, K_lightRender,
    K_initShadowTrace, K_sphereShadowTrace, K_triangleShadowTrace, K_sceneRender, K_bouncePaths, K_copyToPixel,
    K_a01_raytrace, K_a04_sizeofRay, K_a04_initTrace, K_a04_meshTrace, K_a07_sizeofRay, K_a07_initTrace, K_a07_meshTrace, K_a07_molTrace, K_COUNT
};

constexpr size_t arg_size(ArgType t) { return t == A_U32 || t == A_F32 ? 4 : t == A_F16 ? 64 : t == A_AABB ? 32 : 0; }

constexpr size_t kMaxArgs = 11;   // the longest list: A07 meshTrace
struct ArgList {
    ArgType type[kMaxArgs];
    size_t n;
    constexpr size_t size() const { return n; }
    constexpr ArgType operator[](size_t i) const { return type[i]; }
};
struct KernelSpec { const char* name; KernelId id; ArgList args; };

// One argument of a kernel by name: its position, and its type in the C++ type.  A kernel's ArgList is MADE of its named arguments (args(), which
// does not compile unless they count 0, 1, 2 ... in order), and arg() below reads a value through the overload its type selects -- so a name
// cannot point at another position than the table says, and a buffer cannot be read as a number.
template <ArgType T> struct Idx { unsigned i; };
template <ArgType... T> constexpr ArgList args(Idx<T>... a) {
    static_assert(sizeof...(T) <= kMaxArgs, "raise kMaxArgs");
    const unsigned at[] = {a.i...};
    for (unsigned k = 0; k < sizeof...(T); ++k)
        if (at[k] != k) throw "named arguments are not in the order of their positions";
    return ArgList{{T...}, sizeof...(T)};
}

// The argument lists, named as the .cl signatures name them: A10 code.cl:440-1386 as bound by A10 code.js.
namespace sizeofRay { constexpr Idx<A_BUF> size{0}; constexpr ArgList list = args(size); }   // sizeofPoi and the A04 / A07 sizeofRay: the same
namespace initAcu { constexpr Idx<A_BUF> acu{0}; constexpr Idx<A_U32> total{1}; constexpr ArgList list = args(acu, total); }
namespace initTrace {
constexpr Idx<A_BUF> seeds{0}, rays{1}, pois{2}; constexpr Idx<A_AABB> bound{3}; constexpr Idx<A_F16> fcam{4}; constexpr Idx<A_F32> focal_length{5}, lens_rad{6};
constexpr Idx<A_U32> rays_per_pixel{7};
constexpr ArgList list = args(seeds, rays, pois, bound, fcam, focal_length, lens_rad, rays_per_pixel);
}
namespace sphereTrace {
constexpr Idx<A_U32> total{0}; constexpr Idx<A_BUF> pois{1}, rays{2}, prims{3}, matid{4}, off{5}; constexpr Idx<A_AABB> bounds{6}; constexpr Idx<A_U32> n_slabs{7};
constexpr ArgList list = args(total, pois, rays, prims, matid, off, bounds, n_slabs);
}
namespace triangleTrace {
constexpr Idx<A_U32> total{0}; constexpr Idx<A_BUF> pois{1}, rays{2}, prims{3}, normals{4}, matid{5}, off{6}; constexpr Idx<A_AABB> bounds{7}; constexpr Idx<A_U32> n_slabs{8};
constexpr ArgList list = args(total, pois, rays, prims, normals, matid, off, bounds, n_slabs);
}
namespace meshTrace {
constexpr Idx<A_U32> total{0}; constexpr Idx<A_BUF> pois{1}, rays{2}, prims{3}, normals{4}, off{5}; constexpr Idx<A_U32> matid{6}; constexpr Idx<A_AABB> bounds{7};
constexpr Idx<A_U32> n_slabs{8};
constexpr ArgList list = args(total, pois, rays, prims, normals, off, matid, bounds, n_slabs);
}
namespace lightRender {
constexpr Idx<A_BUF> pois{0}, rays{1}, acu{2}; constexpr Idx<A_F16> light_info{3}; constexpr Idx<A_U32> total{4};
constexpr ArgList list = args(pois, rays, acu, light_info, total);
}
namespace initShadowTrace {
constexpr Idx<A_BUF> shadow_rays{0}, pois{1}; constexpr Idx<A_U32> total{2}; constexpr Idx<A_F16> light_info{3}; constexpr Idx<A_BUF> seeds{4};
constexpr ArgList list = args(shadow_rays, pois, total, light_info, seeds);
}
namespace shadowTrace {   // sphereShadowTrace and triangleShadowTrace
constexpr Idx<A_U32> total{0}; constexpr Idx<A_BUF> shadow_rays{1}, prims{2}, off{3}; constexpr Idx<A_AABB> bounds{4}; constexpr Idx<A_U32> n_slabs{5};
constexpr ArgList list = args(total, shadow_rays, prims, off, bounds, n_slabs);
}
namespace sceneRender {
constexpr Idx<A_BUF> acu{0}, pois{1}, shadow_rays{2}, material{3}; constexpr Idx<A_F16> light_info{4}; constexpr Idx<A_U32> total{5};
constexpr ArgList list = args(acu, pois, shadow_rays, material, light_info, total);
}
namespace bouncePaths {
constexpr Idx<A_BUF> pois{0}, rays{1}, seeds{2}; constexpr Idx<A_U32> total{3};
constexpr ArgList list = args(pois, rays, seeds, total);
}
namespace copyToPixel {
constexpr Idx<A_BUF> pixel{0}, acu{1}; constexpr Idx<A_F32> m{2}; constexpr Idx<A_U32> pixels{3}, rays_per_pixel{4};
constexpr ArgList list = args(pixel, acu, m, pixels, rays_per_pixel);
}
// earlier assignments, selected with a dialect prefix (their kernel names collide with A10's): A01 code.cl:116; A04 code.cl:200-315; A07 code.cl:307-626.
// Every one of them begins (pixels, fcam), the A04 / A07 ones (pixels, fcam, rays).
namespace frame { constexpr Idx<A_BUF> pixels{0}; constexpr Idx<A_F16> fcam{1}; constexpr Idx<A_BUF> rays{2}; }
namespace a01_raytrace { constexpr ArgList list = args(frame::pixels, frame::fcam); }
namespace a04_initTrace { constexpr ArgList list = args(frame::pixels, frame::fcam, frame::rays); }
namespace a04_meshTrace {
constexpr Idx<A_U32> t_size{3}; constexpr Idx<A_BUF> t_pos{4}, t_normal{5}, t_mindex{6}, m_color{7};
constexpr ArgList list = args(frame::pixels, frame::fcam, frame::rays, t_size, t_pos, t_normal, t_mindex, m_color);
}
namespace a07_initTrace { constexpr Idx<A_AABB> bound{3}; constexpr ArgList list = args(frame::pixels, frame::fcam, frame::rays, bound); }
namespace a07_meshTrace {
constexpr Idx<A_U32> t_size{3}; constexpr Idx<A_BUF> t_pos{4}, t_normal{5}, t_mindex{6}, m_color{7}; constexpr Idx<A_AABB> bound{8}; constexpr Idx<A_U32> n_slabs{9};
constexpr Idx<A_BUF> slab_size{10};
constexpr ArgList list = args(frame::pixels, frame::fcam, frame::rays, t_size, t_pos, t_normal, t_mindex, m_color, bound, n_slabs, slab_size);
}
namespace a07_molTrace {   // A07 code.cl:337-344
constexpr Idx<A_U32> s_size{3}; constexpr Idx<A_BUF> s_atoms{4}, s_mindex{5}, m_color{6}; constexpr Idx<A_AABB> bound{7}; constexpr Idx<A_U32> n_slabs{8};
constexpr Idx<A_BUF> slab_size{9};
constexpr ArgList list = args(frame::pixels, frame::fcam, frame::rays, s_size, s_atoms, s_mindex, m_color, bound, n_slabs, slab_size);
}

inline constexpr KernelSpec kKernels[] = {
    {"sizeofRay", K_sizeofRay, sizeofRay::list},
    {"sizeofPoi", K_sizeofPoi, sizeofRay::list},
    {"initAcu", K_initAcu, initAcu::list},
    {"initTrace", K_initTrace, initTrace::list},
    {"sphereTrace", K_sphereTrace, sphereTrace::list},
    {"triangleTrace", K_triangleTrace, triangleTrace::list},
    {"meshTrace", K_meshTrace, meshTrace::list},
    {"lightRender", K_lightRender, lightRender::list},
    {"initShadowTrace", K_initShadowTrace, initShadowTrace::list},
    {"sphereShadowTrace", K_sphereShadowTrace, shadowTrace::list},
    {"triangleShadowTrace", K_triangleShadowTrace, shadowTrace::list},
    {"sceneRender", K_sceneRender, sceneRender::list},
    {"bouncePaths", K_bouncePaths, bouncePaths::list},
    {"copyToPixel", K_copyToPixel, copyToPixel::list},
    {"A01:raytrace", K_a01_raytrace, a01_raytrace::list},
    {"A04:sizeofRay", K_a04_sizeofRay, sizeofRay::list},
    {"A04:initTrace", K_a04_initTrace, a04_initTrace::list},
    {"A04:meshTrace", K_a04_meshTrace, a04_meshTrace::list},
    {"A07:sizeofRay", K_a07_sizeofRay, sizeofRay::list},
    {"A07:initTrace", K_a07_initTrace, a07_initTrace::list},
    {"A07:meshTrace", K_a07_meshTrace, a07_meshTrace::list},
    {"A07:molTrace", K_a07_molTrace, a07_molTrace::list},
};
static_assert(sizeof kKernels / sizeof kKernels[0] == K_COUNT, "as many rows as KernelIds (rows are found by name)");

struct KArg {
    bool set = false;
    mirt_buf* buf = nullptr;
    union { uint32_t u; float f; float v[16]; } val;
};
inline mirt_buf* arg(const std::vector<KArg>& a, Idx<A_BUF> j) { return a[j.i].buf; }
inline uint32_t arg(const std::vector<KArg>& a, Idx<A_U32> j) { return a[j.i].val.u; }
inline float arg(const std::vector<KArg>& a, Idx<A_F32> j) { return a[j.i].val.f; }
inline const float* arg(const std::vector<KArg>& a, Idx<A_F16> j) { return a[j.i].val.v; }
inline const float* arg(const std::vector<KArg>& a, Idx<A_AABB> j) { return a[j.i].val.v; }

// an enqueue as mirt_enqueue holds it back: the kernel, a snapshot of its arguments, the NDRange (g[d] = 1 beyond dim)
struct Enqueue { const KernelSpec* spec; std::vector<KArg> args; unsigned dim; size_t g[3]; };

// OpenCL's convert_uint_sat of the image size the camera block carries as floats (fcam[14], fcam[15])
inline uint32_t f2u_host(float f) {
    if (!(f == f)) return 0u;
    if (f >= 4294967296.0f) return UINT32_MAX;
    if (f <= 0.0f) return 0u;
    return (uint32_t)f;
}

// What a recognised pass is made of -- enough to write the stream out again, NDRange sizes aside.
struct PassMatch {
    uint32_t width = 0, height = 0, rpp = 0, bounces = 0;
    float cam[16], scene_bounds[8], focal_length = 0.0f, lens_rad = 0.0f;   // initTrace's scalars
    // the primitive sets in enqueue order, which is the upload order the fused pass assumes: the sphere set if `spheres`, then the loose-triangle set
    // if `triangles`, then the meshes
    std::vector<mirt_grid> sets;
    bool spheres = false, triangles = false;
    std::vector<mirt_light> lights;
    mirt_buf *seeds = nullptr, *rays = nullptr, *pois = nullptr, *shadow = nullptr, *acu = nullptr, *material = nullptr, *pixel = nullptr;
    float tone = 0.0f;   // copyToPixel's factor as the host passed it
};

// Is the stream exactly one pass -- initTrace, the closest-hit kernels, lightRender per light, per light {initShadowTrace, one any-hit kernel per
// set, sceneRender}, any number of {bouncePaths, closest-hit kernels, per-light block}, copyToPixel -- with every stage reading what the stage before
// wrote, the same geometry and light blocks in every segment, and every NDRange covering its work?  Fills *m when it is.
inline bool match_pass(const std::vector<Enqueue>& P, PassMatch* m) {
    size_t i = 0;
    auto id = [&](size_t k) { return k < P.size() ? P[k].spec->id : K_COUNT; };
    auto same_f = [](const float* x, const float* y, int n) { return memcmp(x, y, (size_t)n * 4) == 0; };
    if (id(0) != K_initTrace || P[0].dim != 2) return false;
    mirt_buf *seeds = arg(P[0].args, initTrace::seeds), *rays = arg(P[0].args, initTrace::rays), *pois = arg(P[0].args, initTrace::pois);
    const uint32_t rpp = arg(P[0].args, initTrace::rays_per_pixel);
    const float* cam = arg(P[0].args, initTrace::fcam);
    const uint32_t cols = f2u_host(cam[14]), rows = f2u_host(cam[15]);
    if (!rpp || !cols || !rows || P[0].g[0] < cols || P[0].g[1] < rows) return false;
    const uint64_t total64 = (uint64_t)cols * rows * rpp;
    if (total64 > 0xFFFFFFFFull) return false;
    const uint32_t total = (uint32_t)total64;
    i = 1;
    auto closest_group = [&](std::vector<mirt_grid>& out, std::vector<KernelId>& kinds) -> bool {
        for (;; ++i) {
            const KernelId k = id(i);
            if (k != K_sphereTrace && k != K_triangleTrace && k != K_meshTrace) return true;
            const std::vector<KArg>& a = P[i].args;
            static_assert(triangleTrace::total.i == sphereTrace::total.i && triangleTrace::pois.i == sphereTrace::pois.i && triangleTrace::rays.i == sphereTrace::rays.i &&
                          meshTrace::total.i == sphereTrace::total.i && meshTrace::pois.i == sphereTrace::pois.i && meshTrace::rays.i == sphereTrace::rays.i,
                          "total, pois and rays sit at the same positions in all three");
            if (arg(a, sphereTrace::total) != total || arg(a, sphereTrace::pois) != pois || arg(a, sphereTrace::rays) != rays || P[i].g[0] < total) return false;
            mirt_grid r;
            memset(&r, 0, sizeof r);
            if (k == K_sphereTrace) {
                namespace S = sphereTrace;
                r.prims = arg(a, S::prims); r.matid = arg(a, S::matid); r.cell_offsets = arg(a, S::off); memcpy(r.bounds, arg(a, S::bounds), 32); r.n_slabs = arg(a, S::n_slabs);
            } else if (k == K_triangleTrace) {
                namespace T = triangleTrace;
                r.prims = arg(a, T::prims); r.normals = arg(a, T::normals); r.matid = arg(a, T::matid); r.cell_offsets = arg(a, T::off);
                memcpy(r.bounds, arg(a, T::bounds), 32); r.n_slabs = arg(a, T::n_slabs);
            } else {
                namespace M = meshTrace;
                r.prims = arg(a, M::prims); r.normals = arg(a, M::normals); r.cell_offsets = arg(a, M::off); r.mesh_matid = arg(a, M::matid);
                memcpy(r.bounds, arg(a, M::bounds), 32); r.n_slabs = arg(a, M::n_slabs);
            }
            out.push_back(r);
            kinds.push_back(k);
        }
    };
    std::vector<mirt_grid> sets;
    std::vector<KernelId> kinds;
    if (!closest_group(sets, kinds)) return false;
    // upload order the fused pass assumes: at most one sphere set, then at most one loose-triangle set, then the meshes
    bool spheres = false, triangles = false;
    {
        size_t k = 0;
        if (k < sets.size() && kinds[k] == K_sphereTrace) { spheres = true; ++k; }
        if (k < sets.size() && kinds[k] == K_triangleTrace) { triangles = true; ++k; }
        for (; k < sets.size(); ++k) if (kinds[k] != K_meshTrace) return false;
        if (sets.size() > 2u + MIRT_MAX_MESHES) return false;
    }
    std::vector<mirt_light> lights;
    mirt_buf *acu = nullptr, *shadow = nullptr, *material = nullptr;
    for (; id(i) == K_lightRender; ++i) {
        namespace L = lightRender;
        const std::vector<KArg>& a = P[i].args;
        if (arg(a, L::pois) != pois || arg(a, L::rays) != rays || arg(a, L::total) != total || P[i].g[0] < total) return false;
        if (acu && arg(a, L::acu) != acu) return false;
        acu = arg(a, L::acu);
        mirt_light l;
        memset(&l, 0, sizeof l);
        memcpy(l.light, arg(a, L::light_info), 64);
        lights.push_back(l);
    }
    if (lights.size() > MIRT_MAX_LIGHTS) return false;
    auto direct_block = [&](bool first) -> bool {
        for (size_t l = 0; l < lights.size(); ++l) {
            {
                namespace I = initShadowTrace;
                if (id(i) != K_initShadowTrace) return false;
                const std::vector<KArg>& a = P[i].args;
                if (arg(a, I::pois) != pois || arg(a, I::total) != total || arg(a, I::seeds) != seeds || P[i].g[0] < total) return false;
                if (shadow && arg(a, I::shadow_rays) != shadow) return false;
                shadow = arg(a, I::shadow_rays);
                if (first) memcpy(lights[l].shadow, arg(a, I::light_info), 64); else if (!same_f(lights[l].shadow, arg(a, I::light_info), 16)) return false;
                ++i;
            }
            for (size_t k = 0; k < sets.size(); ++k) {   // one any-hit kernel per set, same order, same geometry
                namespace H = shadowTrace;
                const mirt_grid& r = sets[k];
                if (id(i) != (kinds[k] == K_sphereTrace ? K_sphereShadowTrace : K_triangleShadowTrace)) return false;
                const std::vector<KArg>& a = P[i].args;
                if (arg(a, H::total) != total || arg(a, H::shadow_rays) != shadow || arg(a, H::prims) != r.prims || arg(a, H::off) != r.cell_offsets ||
                    !same_f(arg(a, H::bounds), r.bounds, 8) || arg(a, H::n_slabs) != r.n_slabs || P[i].g[0] < total) return false;
                ++i;
            }
            {
                namespace R = sceneRender;
                if (id(i) != K_sceneRender) return false;
                const std::vector<KArg>& a = P[i].args;
                if (arg(a, R::acu) != acu || arg(a, R::pois) != pois || arg(a, R::shadow_rays) != shadow || arg(a, R::total) != total || P[i].g[0] < total) return false;
                if (material && arg(a, R::material) != material) return false;
                material = arg(a, R::material);
                if (first) memcpy(lights[l].scene, arg(a, R::light_info), 64); else if (!same_f(lights[l].scene, arg(a, R::light_info), 16)) return false;
                ++i;
            }
        }
        return true;
    };
    if (lights.empty() || !direct_block(true)) return false;     // a scene without lights has no sceneRender to take acu / material from: not fused
    uint32_t bounces = 0;
    while (id(i) == K_bouncePaths) {
        namespace B = bouncePaths;
        const std::vector<KArg>& a = P[i].args;
        if (arg(a, B::pois) != pois || arg(a, B::rays) != rays || arg(a, B::seeds) != seeds || arg(a, B::total) != total || P[i].g[0] < total) return false;
        ++i;
        std::vector<mirt_grid> again;
        std::vector<KernelId> again_kinds;
        if (!closest_group(again, again_kinds) || again.size() != sets.size()) return false;
        for (size_t k = 0; k < sets.size(); ++k)
            if (again_kinds[k] != kinds[k] || again[k].prims != sets[k].prims || again[k].normals != sets[k].normals || again[k].matid != sets[k].matid ||
                again[k].cell_offsets != sets[k].cell_offsets || again[k].n_slabs != sets[k].n_slabs || again[k].mesh_matid != sets[k].mesh_matid ||
                !same_f(again[k].bounds, sets[k].bounds, 8)) return false;
        if (!direct_block(false)) return false;
        ++bounces;
    }
    if (id(i) != K_copyToPixel || i + 1 != P.size()) return false;
    namespace C = copyToPixel;
    const std::vector<KArg>& last = P[i].args;
    if (arg(last, C::acu) != acu || arg(last, C::pixels) != cols * rows || arg(last, C::rays_per_pixel) != rpp || P[i].g[0] < cols * rows) return false;
    {   // the fused pass takes k x k rays per pixel only (see render_pass_impl)
        const uint32_t k = (uint32_t)std::sqrt((double)rpp);
        const uint32_t kk = (k + 1) * (k + 1) == rpp ? k + 1 : k;
        if (kk * kk != rpp) return false;
    }
    m->width = cols; m->height = rows; m->rpp = rpp; m->bounces = bounces;
    memcpy(m->cam, cam, 64);
    memcpy(m->scene_bounds, arg(P[0].args, initTrace::bound), 32);
    m->focal_length = arg(P[0].args, initTrace::focal_length); m->lens_rad = arg(P[0].args, initTrace::lens_rad);
    m->sets = std::move(sets); m->spheres = spheres; m->triangles = triangles;
    m->lights = std::move(lights);
    m->seeds = seeds; m->rays = rays; m->pois = pois; m->shadow = shadow; m->acu = acu; m->material = material;
    m->pixel = arg(last, C::pixel); m->tone = arg(last, C::m);
    return true;
}

// ---- the frame dialects (Assign04 / Assign07): is a held stream exactly one frame as the pages issue it -- compute (A07 code.js:571-600: initTrace,
// molTrace), computeTri (A04 code.js:553-577, A07 code.js:603-628: initTrace, meshTrace) or computeBoth (A07 code.js:629-661: initTrace, molTrace,
// meshTrace) -- over one pixel buffer, one ray buffer, one camera block, one box and one NDRange that covers the image?  The fused frame
// (mirt_render_frame) writes pixels only, so a wrong "yes" loses a ray buffer somebody reads or renders over the wrong box: everything is compared.
struct FrameMatch {
    uint32_t assign = 0, width = 0, height = 0;
    float cam[16], bounds[8];                       // bounds: Assign07 only (zero for Assign04)
    mirt_buf *pixels = nullptr, *rays = nullptr;
    bool mesh = false, mol = false;
    uint32_t t_size = 0, s_size = 0, n_slabs = 0;   // n_slabs: of both grids
    mirt_buf *t_pos = nullptr, *t_normal = nullptr, *t_mindex = nullptr, *t_mcolor = nullptr, *t_slab_size = nullptr;
    mirt_buf *s_atoms = nullptr, *s_mindex = nullptr, *s_mcolor = nullptr, *s_slab_size = nullptr;
};

inline bool is_frame_init(KernelId k) { return k == K_a04_initTrace || k == K_a07_initTrace; }
inline bool is_frame_trace(KernelId k) { return k == K_a04_meshTrace || k == K_a07_meshTrace || k == K_a07_molTrace; }

inline bool match_frame(const std::vector<Enqueue>& P, FrameMatch* m) {
    if (P.size() < 2 || P.size() > 3 || !is_frame_init(P[0].spec->id) || P[0].dim != 2) return false;
    const bool a07 = P[0].spec->id == K_a07_initTrace;
    const std::vector<KArg>& a0 = P[0].args;
    mirt_buf *pixels = arg(a0, frame::pixels), *rays = arg(a0, frame::rays);
    const float* cam = arg(a0, frame::fcam);
    const uint32_t cols = f2u_host(cam[14]), rows = f2u_host(cam[15]);
    if (!cols || !rows || P[0].g[0] < cols || P[0].g[1] < rows) return false;
    FrameMatch r;
    memset(r.bounds, 0, sizeof r.bounds);
    if (a07) memcpy(r.bounds, arg(a0, a07_initTrace::bound), 32);
    for (size_t i = 1; i < P.size(); ++i) {
        const Enqueue& e = P[i];
        const std::vector<KArg>& a = e.args;
        // every stage over the same pixels, camera block and rays, with the global size of the initTrace
        if (!is_frame_trace(e.spec->id) || e.dim != 2 || e.g[0] != P[0].g[0] || e.g[1] != P[0].g[1]) return false;
        if (arg(a, frame::pixels) != pixels || arg(a, frame::rays) != rays || memcmp(arg(a, frame::fcam), cam, 64) != 0) return false;
        if (e.spec->id == K_a04_meshTrace) {
            namespace M = a04_meshTrace;
            if (a07 || r.mesh) return false;
            r.mesh = true; r.t_size = arg(a, M::t_size);
            r.t_pos = arg(a, M::t_pos); r.t_normal = arg(a, M::t_normal); r.t_mindex = arg(a, M::t_mindex); r.t_mcolor = arg(a, M::m_color);
        } else if (e.spec->id == K_a07_molTrace) {
            namespace M = a07_molTrace;
            if (!a07 || r.mol || r.mesh) return false;                      // the molecule comes first, once
            if (memcmp(arg(a, M::bound), r.bounds, 32) != 0) return false;
            r.mol = true; r.s_size = arg(a, M::s_size); r.n_slabs = arg(a, M::n_slabs);
            r.s_atoms = arg(a, M::s_atoms); r.s_mindex = arg(a, M::s_mindex); r.s_mcolor = arg(a, M::m_color); r.s_slab_size = arg(a, M::slab_size);
        } else {
            namespace M = a07_meshTrace;
            if (!a07 || r.mesh) return false;
            if (memcmp(arg(a, M::bound), r.bounds, 32) != 0) return false;
            if (r.mol && arg(a, M::n_slabs) != r.n_slabs) return false;    // computeBoth bins both models with the page's one n_slabs
            r.mesh = true; r.t_size = arg(a, M::t_size); r.n_slabs = arg(a, M::n_slabs);
            r.t_pos = arg(a, M::t_pos); r.t_normal = arg(a, M::t_normal); r.t_mindex = arg(a, M::t_mindex); r.t_mcolor = arg(a, M::m_color);
            r.t_slab_size = arg(a, M::slab_size);
        }
    }
    r.assign = a07 ? 7u : 4u; r.width = cols; r.height = rows;
    memcpy(r.cam, cam, 64);
    r.pixels = pixels; r.rays = rays;
    *m = r;
    return true;
}

}  // namespace pt
