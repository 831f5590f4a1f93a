// pt_kernels_frame.hip -- the single-frame kernels of the reference's earlier assignments that
// BASELINE.json lists as parity configurations:
//   Assign01  raytrace                       (A01 code.cl:116-147)  one hard-coded sphere
//   Assign04  initTrace, meshTrace           (A04 code.cl:204-215, 262-315)  brute-force ray / triangle
//   Assign07  initTrace, meshTrace, molTrace (A07 code.cl:311-335, 475-626, 337-473)  3-D uniform grid DDA over triangles / atoms,
//                                            cell-parity shading
// Same launch shape as the reference (2-D NDRange, one work-item per pixel), same buffers
// (Ray 48 B, uchar4 pixels, float4-padded triangles).  Triangles are read from the prepared copy
// (pt_trace.hpp).  Assign04's molTrace (brute force over atoms) is not built: its molecule mode is subsumed by Assign07's.
#include "pt_trace.hpp"

namespace pt {

PT_DEV void store_ray48(RayAoS* p, const Ray& r) {
    float4* q = reinterpret_cast<float4*>(p);
    q[0] = make_float4(r.o.x, r.o.y, r.o.z, 0.0f);
    q[1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
    *reinterpret_cast<float2*>(q + 2) = make_float2(r.mint, r.maxt);
}
PT_DEV Ray load_ray48(const RayAoS* p) {
    const float4* q = reinterpret_cast<const float4*>(p);
    float4 a = q[0], b = q[1];
    float2 c = *reinterpret_cast<const float2*>(q + 2);
    Ray r;
    r.o = mk3(a.x, a.y, a.z); r.d = mk3(b.x, b.y, b.z); r.mint = c.x; r.maxt = c.y;
    return r;
}
// getRay of A02..A10 (A04 code.cl:86-97): pinhole ray through the pixel centre
PT_DEV Ray pinhole_ray(const Cam& c, float col, float row) {
    float sx = (-0.5f + (col + 0.5f) / (float)c.cols) * c.width;
    float sy = (0.5f - (row + 0.5f) / (float)c.rows) * c.height;
    f3 cop = add3(fma3(sx, c.U, scl3(sy, c.V)), scl3(-1.0f, c.W));
    Ray r;
    r.d = norm3(cop);
    r.o = c.eye;
    r.mint = 0.0f;
    r.maxt = PT_INF;
    return r;
}
// (uchar) of a float the way the compiled reference does it: truncate to int32, keep the low byte
PT_DEV unsigned char f2u8(float f) { return (unsigned char)(f2i(f) & 0xFF); }

// ---- Assign01 -----------------------------------------------------------------------------------
// Camera packs rows, cols in .sE, .sF as floats (A01 code.cl:44-46; swapped w.r.t. A02+), getRay uses
// normalize(cop - eye), interSphere is the textbook quadratic with `/ 2*a` (sic) and an open interval.
__global__ void __launch_bounds__(256) k_a01_raytrace(uchar4* pixels, F16 cam, uint32_t gx, uint32_t gy) {
    uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t row = blockIdx.y * blockDim.y + threadIdx.y;
    const float rows = cam.v[14], cols = cam.v[15];
    // the reference has no range check (it is launched on exactly cols x rows); we add one so a padded
    // NDRange cannot write outside the image
    if (col >= gx || row >= gy || !((float)col < cols) || !((float)row < rows)) return;
    f3 eye = ld3(cam.v), U = ld3(cam.v + 3), V = ld3(cam.v + 6), W = ld3(cam.v + 9);
    float sx = (-0.5f + ((float)col + 0.5f) / cols) * cam.v[12];
    float sy = (0.5f - ((float)row + 0.5f) / rows) * cam.v[13];
    f3 cop = add3(fma3(sx, U, scl3(sy, V)), scl3(-1.0f, W));
    f3 o = eye;
    f3 d = norm3(sub3(cop, o));
    const f3 sc = mk3(0.0f, 0.0f, 1.0f);
    const float sr = 0.5f;
    f3 omc = sub3(o, sc);
    float a = dot3(d, d);
    float b = 2.0f * dot3(omc, d);
    float c = cl_fma(-sr, sr, dot3(omc, omc));              // A01 code.cl:68, contracted
    float dis = cl_fma(b, b, -((4.0f * a) * c));            // A01 code.cl:69: the LEFT product fuses
    bool v = false;
    float t = PT_INF;
    if (!(dis < 0.0f)) {
        float sq = cl_sqrt(dis);
        float t0 = (-b - sq) / 2 * a;
        float t1 = (-b + sq) / 2 * a;
        if (t0 > 0.0f && t0 < PT_INF) { t = t0; v = true; }
        else if (t1 > 0.0f && t1 < PT_INF) { t = t1; v = true; }
    }
    unsigned char base = v ? f2u8((1.0f - t) * 255.0f) : 0;
    pixels[f2u_uniform(cols) * row + col] = make_uchar4(base, base, base, 255);
}

// ---- Assign04 / Assign07 initTrace ---------------------------------------------------------------
template <bool CLIP>
__global__ void __launch_bounds__(256) k_frame_initTrace(uchar4* pixels, F16 cam16, RayAoS* rays, Box8 bound8, uint32_t gx, uint32_t gy) {
    const Cam cam = mk_cam(cam16);
    uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t row = blockIdx.y * blockDim.y + threadIdx.y;
    if (col >= gx || row >= gy || col >= cam.cols || row >= cam.rows) return;
    Ray r = pinhole_ray(cam, (float)col, (float)row);
    if (CLIP) clip_to(r, mk_box(bound8));   // A07 code.cl:321-328
    store_ray48(&rays[(size_t)cam.cols * row + col], r);
    pixels[(size_t)cam.cols * row + col] = make_uchar4(0, 0, 0, 255);
}

PT_DEV uchar4 parity_colour(int hx, int hy, int hz, float shade) {   // A07 code.cl:463-469, 616-622
    const float k = shade * 127.0f;
    return make_uchar4(f2u8((float)((hx % 2) + 1) * k), f2u8((float)((hy % 2) + 1) * k), f2u8((float)((hz % 2) + 1) * k), 255);
}

// ---- Assign04 meshTrace: every pixel against every triangle, wave-uniform loop --------------------
__global__ void __launch_bounds__(256) k_a04_meshTrace(uchar4* pixels, F16 cam16, RayAoS* rays, uint32_t t_size, const float4* prep,
                                                        const float4* normals, const uint32_t* mindex, const float4* mcolor,
                                                        uint32_t ncolors, uint32_t gx, uint32_t gy) {
    const Cam cam = mk_cam(cam16);
    uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t row = blockIdx.y * blockDim.y + threadIdx.y;
    if (col >= gx || row >= gy || col >= cam.cols || row >= cam.rows) return;
    const size_t pix = (size_t)cam.cols * row + col;
    Ray ray = load_ray48(&rays[pix]);
    float champ_t = PT_INF, cb = 0.0f, cg = 0.0f;
    uint32_t champ_i = t_size;
    // interTriangle (A04 code.cl:146-184) on the prepared triangle, staged: the 64 lanes of a wave are 2 x 32 adjacent pixels, and
    // almost every one of a mesh's small triangles is missed by all of them at an early rejection.  After each of the reference's
    // early-outs a wave ballot asks whether ANY lane is still in; if none is, the rest of the test is skipped for the wave.  Lanes
    // that are still in compute exactly the values the straight-line test computes, so nothing changes but the work.
    const float4* __restrict__ p = prep;
    const float4* __restrict__ groups = prep + 3u * (size_t)t_size;   // one bounding sphere per kTriGroup records (k_prepTriangles)
    const float dd = ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z;
    for (uint32_t i = 0; i < t_size; ++i, p += 3) {
        // a whole group none of the wave's 64 rays can reach (pt_trace.hpp group_missed) is skipped
        if ((i % kTriGroup) == 0u && i + kTriGroup <= t_size && __builtin_amdgcn_ballot_w64(!group_missed(ray, dd, groups[i / kTriGroup])) == 0ull) {
            i += kTriGroup - 1u;
            p += 3u * (kTriGroup - 1u);
            continue;
        }
        const float4 A = p[0], B = p[1], C = p[2];
        const f3 p0 = mk3(A.x, A.y, A.z), e1 = mk3(B.x, B.y, B.z), e2 = mk3(C.x, C.y, C.z), n = mk3(A.w, B.w, C.w);
        const float div = dot3(n, ray.d);
        bool in = !(div <= 0);                                                   // code.cl:153
        if (__builtin_amdgcn_ballot_w64(in) == 0ull) continue;
        const float idiv = rcp_exact(div, !in);                                  // 1.0f / div, bit for bit (pt_numerics.hpp)
        const f3 s = sub3(ray.o, p0);
        const float beta = dot3(cross3(s, ray.d), e2) * idiv;
        in = in & !(beta < 0.0f) & !(beta > 1.0f);                               // :161
        if (__builtin_amdgcn_ballot_w64(in) == 0ull) continue;
        const float gamma = dot3(cross3(s, e1), ray.d) * idiv;
        const float gb = gamma + beta;
        in = in & !(gamma < 0.0f) & !(gamma > 1.0f) & !(gb < 0.0f) & !(gb > 1.0f);   // :169-170 (A04 also rejects gamma > 1)
        if (__builtin_amdgcn_ballot_w64(in) == 0ull) continue;
        const float t = dot3(cross3(s, e2), e1) * -idiv;
        in = in & (t > ray.mint) & (t < ray.maxt);                               // open interval, :177
        if (in && t < champ_t) { champ_t = t; champ_i = i; cb = beta; cg = gamma; }
    }
    if (champ_i >= t_size) return;
    rays[pix].maxt = champ_t;
    f3 n = interp_normal(normals + 3u * (size_t)champ_i, cb, cg);
    float shade = cl_clamp(dot3(cam.W, n), 0.0f, 1.0f);
    uint32_t m = mindex[champ_i];
    if (m >= ncolors) return;  // foreign-memory guard (the reference would read out of bounds)
    float4 mc = mcolor[m];
    pixels[pix] = make_uchar4(f2u8((mc.x * 255.0f) * shade), f2u8((mc.y * 255.0f) * shade), f2u8((mc.z * 255.0f) * shade), 255);
}

// ---- Assign07 meshTrace: 3-D grid DDA, colour = parity of the hit cell x fake shade -------------------
// GROUPS: coarse grids (see the loop); a template parameter so that fine grids run the plain loop, untouched
template <bool GROUPS>
__global__ void __launch_bounds__(256) k_a07_meshTrace(uchar4* pixels, F16 cam16, RayAoS* rays, const float4* prep, const float4* normals,
                                                        Box8 bound8, uint32_t n_slabs, const uint32_t* slab_size, uint32_t group_slots, uint32_t gx, uint32_t gy) {
    const Cam cam = mk_cam(cam16);
    uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t row = blockIdx.y * blockDim.y + threadIdx.y;
    if (col >= gx || row >= gy || col >= cam.cols || row >= cam.rows) return;
    const size_t pix = (size_t)cam.cols * row + col;
    Ray ray = load_ray48(&rays[pix]);
    if (ray.mint == ray.maxt) return;
    const Box bound = mk_box(bound8);
    BoxHit bh = inter_aabb(ray, bound);
    if (!bh.v) return;
    // per-lane DDA; the hit cell is needed for the colour, so the walk is spelled out here
    Axis ax = axis_setup(ray.o.x, ray.d.x, bh.tmin, bound.lo.x, bound.hi.x, n_slabs);
    Axis ay = axis_setup(ray.o.y, ray.d.y, bh.tmin, bound.lo.y, bound.hi.y, n_slabs);
    Axis az = axis_setup(ray.o.z, ray.d.z, bh.tmin, bound.lo.z, bound.hi.z, n_slabs);
    float champ_t = ray.maxt, cb = 0.0f, cg = 0.0f;
    uint32_t champ_i = UINT32_MAX;
    int hx = 0, hy = 0, hz = 0;
    const uint32_t zs = n_slabs * n_slabs, ys = n_slabs;
    // phase A / phase B as in trace_dda (pt_trace.hpp): close and open cells until every live lane holds a triangle, then one test each
    float t = bh.tmin, cmin = t, cmax = cl_min(cl_min(ax.tnext, ay.tnext), az.tnext);
    uint32_t cell = __umul24((uint32_t)az.slab, zs) + __umul24((uint32_t)ay.slab, ys) + (uint32_t)ax.slab;
    uint32_t i = slab_size[cell], end = slab_size[cell + 1];
    const float dd = GROUPS ? ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z : 0.0f;
    for (;;) {
        bool alive = true;
        while (i == end) {
            if (champ_i != UINT32_MAX) { alive = false; break; }
            t = cmax;
            if (t == ax.tnext) {
                ax.tnext += ax.dt;
                ax.slab += ax.dslab;
                if (t >= bh.tmax || ax.slab == ax.limit) { alive = false; break; }
            } else if (t == ay.tnext) {
                ay.tnext += ay.dt;
                ay.slab += ay.dslab;
                if (t >= bh.tmax || ay.slab == ay.limit) { alive = false; break; }
            } else {
                az.tnext += az.dt;
                az.slab += az.dslab;
                if (t >= bh.tmax || az.slab == az.limit) { alive = false; break; }
            }
            cmin = t;
            cmax = cl_min(cl_min(ax.tnext, ay.tnext), az.tnext);
            cell = __umul24((uint32_t)az.slab, zs) + __umul24((uint32_t)ay.slab, ys) + (uint32_t)ax.slab;
            i = slab_size[cell];
            end = slab_size[cell + 1];
        }
        if (!alive) break;
        // Coarse grids (the page's n_slabs = 2: a thousand slots per cell): when every lane still in has at least a whole group of
        // kTriGroup slots ahead in its list and none of their rays can reach its own group's bounding sphere (pt_trace.hpp group_missed),
        // all step over that group together -- per lane the skip is exact on its own, the ballot only keeps the wave in step.
        if (GROUPS) {
            const bool whole = ((i % kTriGroup) == 0u) & (end - i >= kTriGroup);
            if (__builtin_amdgcn_ballot_w64(!whole) == 0ull &&
                __builtin_amdgcn_ballot_w64(!group_missed(ray, dd, (prep + 3u * (size_t)group_slots)[i / kTriGroup])) == 0ull) {
                i += kTriGroup;
                continue;
            }
        }
        float ti, b, g;
        const float4* __restrict__ p = prep + 3u * (size_t)i;
        // adjacent pixels walk the same cells in nearly the same order: staged rejection with wave ballots (tri_test_staged)
        const bool hit = tri_test_staged<TRI_A07>(true, ray.o, ray.d, cmin, cmax, p[0], p[1], p[2], ti, b, g);
        if (hit && ti < champ_t) { champ_t = ti; champ_i = i; cb = b; cg = g; hx = ax.slab; hy = ay.slab; hz = az.slab; }
        ++i;
    }
    if (champ_i == UINT32_MAX) return;
    rays[pix].maxt = champ_t;
    f3 n = interp_normal(normals + 3u * (size_t)champ_i, cb, cg);
    float shade = cl_clamp(dot3(cam.W, n), 0.0f, 1.0f);
    pixels[pix] = parity_colour(hx, hy, hz, shade);
}

// ---- the trace stages on a ray in registers ------------------------------------------------------------------------------------------------
// A stage is a trace kernel's work on a ray it is handed instead of one it loads.  A hit sets ray.maxt and returns true; a miss -- mint == maxt, a
// ray outside the box, no champion -- returns false and changes nothing.  A hit that shades sets `colour`, alpha 255; a miss, and an Assign04 hit
// whose mindex names no colour, leave it as it was (black, or what the stage before left).  The one-launch kernel (k_frame_fused) runs its stages
// in a row; k_a07_molTrace is the molecule stage between a load and two stores.  The two mesh kernels above keep a text of their own -- the same
// loop and the same walk, line for line: as wrappers of these stages they compile to a few instructions more and measured 2 - 4 % slower on
// parliament (profiles/frame_stages/README.md).

// k_a04_meshTrace on `ray`
PT_DEV bool frame_stage_a04(const Cam& cam, Ray& ray, uint32_t t_size, const float4* prep, const float4* normals, const uint32_t* mindex,
                            const float4* mcolor, uint32_t ncolors, uchar4& colour) {
    float champ_t = PT_INF, cb = 0.0f, cg = 0.0f;
    uint32_t champ_i = t_size;
    const float4* __restrict__ p = prep;
    const float4* __restrict__ groups = prep + 3u * (size_t)t_size;
    const float dd = ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z;
    for (uint32_t i = 0; i < t_size; ++i, p += 3) {
        if ((i % kTriGroup) == 0u && i + kTriGroup <= t_size && __builtin_amdgcn_ballot_w64(!group_missed(ray, dd, groups[i / kTriGroup])) == 0ull) {
            i += kTriGroup - 1u;
            p += 3u * (kTriGroup - 1u);
            continue;
        }
        const float4 A = p[0], B = p[1], C = p[2];
        const f3 p0 = mk3(A.x, A.y, A.z), e1 = mk3(B.x, B.y, B.z), e2 = mk3(C.x, C.y, C.z), n = mk3(A.w, B.w, C.w);
        const float div = dot3(n, ray.d);
        bool in = !(div <= 0);
        if (__builtin_amdgcn_ballot_w64(in) == 0ull) continue;
        const float idiv = rcp_exact(div, !in);
        const f3 s = sub3(ray.o, p0);
        const float beta = dot3(cross3(s, ray.d), e2) * idiv;
        in = in & !(beta < 0.0f) & !(beta > 1.0f);
        if (__builtin_amdgcn_ballot_w64(in) == 0ull) continue;
        const float gamma = dot3(cross3(s, e1), ray.d) * idiv;
        const float gb = gamma + beta;
        in = in & !(gamma < 0.0f) & !(gamma > 1.0f) & !(gb < 0.0f) & !(gb > 1.0f);
        if (__builtin_amdgcn_ballot_w64(in) == 0ull) continue;
        const float t = dot3(cross3(s, e2), e1) * -idiv;
        in = in & (t > ray.mint) & (t < ray.maxt);
        if (in && t < champ_t) { champ_t = t; champ_i = i; cb = beta; cg = gamma; }
    }
    if (champ_i >= t_size) return false;
    ray.maxt = champ_t;
    const f3 n = interp_normal(normals + 3u * (size_t)champ_i, cb, cg);
    const float shade = cl_clamp(dot3(cam.W, n), 0.0f, 1.0f);
    const uint32_t m = mindex[champ_i];
    if (m >= ncolors) return true;   // a hit that leaves the colour alone
    const float4 mc = mcolor[m];
    colour = make_uchar4(f2u8((mc.x * 255.0f) * shade), f2u8((mc.y * 255.0f) * shade), f2u8((mc.z * 255.0f) * shade), 255);
    return true;
}

// The grid walk of k_a07_meshTrace (MOL false: triangles, GROUPS as there) and of Assign07's molTrace (MOL true: atoms {c, r*r}; A07
// code.cl:337-473) on `ray`: phase A closes and opens cells until the lane holds a primitive, phase B tests it.  The hit record keeps the CELL of the
// champion (champ_slab, code.cl:402, 425-429): the walk ends once any cell produced one.  prims: the prepared records (+ group spheres at record
// group_slots) | the atoms.
template <bool MOL, bool GROUPS>
PT_DEV bool frame_stage_grid(const Cam& cam, Ray& ray, const Box& bound, const float4* prims, const float4* normals, uint32_t n_slabs,
                             const uint32_t* slab_size, uint32_t group_slots, uchar4& colour) {
    if (ray.mint == ray.maxt) return false;
    const BoxHit bh = inter_aabb(ray, bound);
    if (!bh.v) return false;
    Axis ax = axis_setup(ray.o.x, ray.d.x, bh.tmin, bound.lo.x, bound.hi.x, n_slabs);
    Axis ay = axis_setup(ray.o.y, ray.d.y, bh.tmin, bound.lo.y, bound.hi.y, n_slabs);
    Axis az = axis_setup(ray.o.z, ray.d.z, bh.tmin, bound.lo.z, bound.hi.z, n_slabs);
    SphereRay sr = {0.0f, 0.0f};
    if (MOL) sr = sphere_ray<false>(ray.d);
    float champ_t = ray.maxt, cb = 0.0f, cg = 0.0f;
    uint32_t champ_i = UINT32_MAX;
    int hx = 0, hy = 0, hz = 0;
    const uint32_t zs = n_slabs * n_slabs, ys = n_slabs;
    float t = bh.tmin, cmin = t, cmax = cl_min(cl_min(ax.tnext, ay.tnext), az.tnext);
    uint32_t cell = __umul24((uint32_t)az.slab, zs) + __umul24((uint32_t)ay.slab, ys) + (uint32_t)ax.slab;
    uint32_t i = slab_size[cell], end = slab_size[cell + 1];
    const float dd = !MOL && GROUPS ? ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z : 0.0f;
    for (;;) {
        bool alive = true;
        while (i == end) {
            if (champ_i != UINT32_MAX) { alive = false; break; }
            t = cmax;
            if (t == ax.tnext) {
                ax.tnext += ax.dt;
                ax.slab += ax.dslab;
                if (t >= bh.tmax || ax.slab == ax.limit) { alive = false; break; }
            } else if (t == ay.tnext) {
                ay.tnext += ay.dt;
                ay.slab += ay.dslab;
                if (t >= bh.tmax || ay.slab == ay.limit) { alive = false; break; }
            } else {
                az.tnext += az.dt;
                az.slab += az.dslab;
                if (t >= bh.tmax || az.slab == az.limit) { alive = false; break; }
            }
            cmin = t;
            cmax = cl_min(cl_min(ax.tnext, ay.tnext), az.tnext);
            cell = __umul24((uint32_t)az.slab, zs) + __umul24((uint32_t)ay.slab, ys) + (uint32_t)ax.slab;
            i = slab_size[cell];
            end = slab_size[cell + 1];
        }
        if (!alive) break;
        if (!MOL && GROUPS) {
            const bool whole = ((i % kTriGroup) == 0u) & (end - i >= kTriGroup);
            if (__builtin_amdgcn_ballot_w64(!whole) == 0ull &&
                __builtin_amdgcn_ballot_w64(!group_missed(ray, dd, (prims + 3u * (size_t)group_slots)[i / kTriGroup])) == 0ull) {
                i += kTriGroup;
                continue;
            }
        }
        float ti, b = 0.0f, g = 0.0f;
        bool hit;
        if (MOL) {
            hit = sph_test(ray.o, ray.d, sr, cmin, cmax, prims[i], ti);
        } else {
            const float4* __restrict__ p = prims + 3u * (size_t)i;
            hit = tri_test_staged<TRI_A07>(true, ray.o, ray.d, cmin, cmax, p[0], p[1], p[2], ti, b, g);
        }
        if (hit && ti < champ_t) { champ_t = ti; champ_i = i; cb = b; cg = g; hx = ax.slab; hy = ay.slab; hz = az.slab; }
        ++i;
    }
    if (champ_i == UINT32_MAX) return false;
    ray.maxt = champ_t;
    f3 n;
    if (MOL) n = norm3(sub3(fma3(champ_t, ray.d, ray.o), ld3(prims[champ_i])));   // A07 code.cl:455-457
    else n = interp_normal(normals + 3u * (size_t)champ_i, cb, cg);
    colour = parity_colour(hx, hy, hz, cl_clamp(dot3(cam.W, n), 0.0f, 1.0f));
    return true;
}

// ---- Assign07 molTrace: the molecule stage on the ray initTrace left.  A hit stores the ray's new maxt (those 4 bytes, not the ray) and the
// pixel; a miss stores nothing, so the pixel keeps what initTrace wrote.
__global__ void __launch_bounds__(256) k_a07_molTrace(uchar4* pixels, F16 cam16, RayAoS* rays, const float4* atoms, Box8 bound8, uint32_t n_slabs,
                                                       const uint32_t* slab_size, uint32_t gx, uint32_t gy) {
    const Cam cam = mk_cam(cam16);
    uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t row = blockIdx.y * blockDim.y + threadIdx.y;
    if (col >= gx || row >= gy || col >= cam.cols || row >= cam.rows) return;
    const size_t pix = (size_t)cam.cols * row + col;
    Ray ray = load_ray48(&rays[pix]);
    uchar4 colour;
    if (!frame_stage_grid<true, false>(cam, ray, mk_box(bound8), atoms, nullptr, n_slabs, slab_size, 0u, colour)) return;
    rays[pix].maxt = ray.maxt;
    pixels[pix] = colour;
}

// ---- the whole Assign04 / Assign07 frame in one launch (mirt_render_frame) ---------------------------------------------------------------
// initTrace + the stage(s) on one thread per pixel, the ray in registers: no 48-byte ray goes out to memory and comes back between two launches.
// The colour starts as initTrace's black and every stage that shades overwrites it, as the launches' pixel stores do in `pixels`.  The kernel
// stores the pixel once, and the finished ray once when a ray buffer is given (RAYS): the same 40 bytes the launches leave there.  Which stages
// run is the template parameter STAGES (FrameStage bits, pt_launch.hpp); the walks have no run-time switch.
template <uint32_t STAGES, bool GROUPS, bool RAYS>
__global__ void __launch_bounds__(256) k_frame_fused(FrameArgs a) {
    const Cam cam = mk_cam(*reinterpret_cast<const F16*>(a.cam));
    const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t row = blockIdx.y * blockDim.y + threadIdx.y;
    if (col >= a.gx || row >= a.gy || col >= cam.cols || row >= cam.rows) return;
    const size_t pix = (size_t)cam.cols * row + col;
    Ray ray = pinhole_ray(cam, (float)col, (float)row);
    const Box bound = mk_box(*reinterpret_cast<const Box8*>(a.bound));
    if (!(STAGES & FS_A04)) clip_to(ray, bound);   // A07 code.cl:321-328
    uchar4 colour = make_uchar4(0, 0, 0, 255);
    if (STAGES & FS_A04)
        frame_stage_a04(cam, ray, a.t_size, (const float4*)a.prep, (const float4*)a.normals, (const uint32_t*)a.mindex, (const float4*)a.mcolor, a.ncolors, colour);
    // computeBoth (A07 code.js:629-661): the molecule, then the mesh from the maxt the molecule left
    if (STAGES & FS_MOL) frame_stage_grid<true, false>(cam, ray, bound, (const float4*)a.atoms, nullptr, a.n_slabs, (const uint32_t*)a.mol_slab_size, 0u, colour);
    if (STAGES & FS_MESH)
        frame_stage_grid<false, GROUPS>(cam, ray, bound, (const float4*)a.prep, (const float4*)a.normals, a.n_slabs, (const uint32_t*)a.slab_size, a.group_slots, colour);
    if (RAYS) store_ray48(&((RayAoS*)a.rays)[pix], ray);
    ((uchar4*)a.pixels)[pix] = colour;
}

// ---- the anti-aliased frame: AA x AA samples a pixel in one launch (mirt_render_frame_aa) ---------------------------------------------------
// FrameArgs is the FINE frame's: a.cam says AA*ow x AA*oh, so pinhole_ray puts sample (AA*x + i, AA*y + j) exactly where k_frame_fused puts that
// pixel of the fine frame, and the stages below are k_frame_fused's, in its order.  An output pixel is the integer box average of its AA*AA
// samples' bytes, (S + AA*AA/2) / (AA*AA) per channel, alpha 255 (include/mirt.h); a.pixels is ow x oh.
// One lane per SAMPLE (k_frame_aa_lanes): a pixel's samples sit in adjacent lanes of one wave, the wave covers a compact fine tile, the sums cross
// lanes (DPP for AA 2 and 4, ds_bpermute for 3) and the pixel's first lane stores.  The other structure that gives these bits -- one thread per OUTPUT
// pixel looping over its samples -- fills the device with 1 / (AA*AA) of the waves and measured 3.5 to 17 times slower
// (profiles/frame_aa/README.md, where it is kept as a patch).
template <uint32_t STAGES, bool GROUPS>
PT_DEV uchar4 frame_sample(const FrameArgs& a, const Cam& cam, const Box& bound, uint32_t col, uint32_t row) {
    Ray ray = pinhole_ray(cam, (float)col, (float)row);
    if (!(STAGES & FS_A04)) clip_to(ray, bound);
    uchar4 colour = make_uchar4(0, 0, 0, 255);
    if (STAGES & FS_A04)
        frame_stage_a04(cam, ray, a.t_size, (const float4*)a.prep, (const float4*)a.normals, (const uint32_t*)a.mindex, (const float4*)a.mcolor, a.ncolors, colour);
    if (STAGES & FS_MOL) frame_stage_grid<true, false>(cam, ray, bound, (const float4*)a.atoms, nullptr, a.n_slabs, (const uint32_t*)a.mol_slab_size, 0u, colour);
    if (STAGES & FS_MESH)
        frame_stage_grid<false, GROUPS>(cam, ray, bound, (const float4*)a.prep, (const float4*)a.normals, a.n_slabs, (const uint32_t*)a.slab_size, a.group_slots, colour);
    return colour;
}
// the sums of R and B ride in the halves of one register (16 * 255 < 65536), G in another
template <uint32_t AA>
PT_DEV uchar4 aa_average(uint32_t rb, uint32_t g) {
    constexpr uint32_t N = AA * AA;
    return make_uchar4((unsigned char)(((rb & 0xFFFFu) + N / 2u) / N), (unsigned char)((g + N / 2u) / N), (unsigned char)(((rb >> 16) + N / 2u) / N), 255);
}

// the output pixels of one wave in k_frame_aa_lanes: W x H of them, lane = pixel * AA*AA + sample.  AA 2: 16 DPP quads, an 8 x 8 fine tile; AA 4:
// four 16-lane DPP rows, 8 x 8 fine; AA 3: 7 pixels in 63 lanes, 21 x 3 fine, lane 63 idle.
template <uint32_t AA> struct AaWave;
template <> struct AaWave<2> { static constexpr uint32_t W = 4, H = 4; };
template <> struct AaWave<3> { static constexpr uint32_t W = 7, H = 1; };
template <> struct AaWave<4> { static constexpr uint32_t W = 2, H = 2; };
template <int CTRL>
PT_DEV uint32_t dpp_get(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true); }
// v summed over the AA*AA lanes of the caller's pixel; the pixel's FIRST lane holds the whole sum (for AA 2 and 4 every lane does).  Every lane
// of the wave must enter.
template <uint32_t AA>
PT_DEV uint32_t aa_lane_sum(uint32_t v, uint32_t lane, uint32_t s) {
    if (AA == 3) {
        // lanes s .. 8 of the pixel fold down on lane s: after the steps 1, 2, 4, 8 lane 0 holds all nine
#pragma unroll
        for (uint32_t d = 1; d < 16u; d *= 2u) {
            const uint32_t o = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((lane + d) & 63u) * 4u), (int)v);
            if (s + d < 9u) v += o;
        }
        return v;
    }
    v += dpp_get<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_get<0x4E>(v);   // quad_perm [2,3,0,1]
    if (AA == 4) {
        v += dpp_get<0x124>(v);   // row_ror:4
        v += dpp_get<0x128>(v);   // row_ror:8
    }
    return v;
}

template <uint32_t STAGES, bool GROUPS, uint32_t AA>
__global__ void __launch_bounds__(256) k_frame_aa_lanes(FrameArgs a, uint32_t ow, uint32_t oh) {
    constexpr uint32_t N = AA * AA, TW = AaWave<AA>::W, TH = AaWave<AA>::H;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t p = lane / N, s = lane % N;
    const uint32_t x = (blockIdx.x * 4u + wave) * TW + p % TW, y = blockIdx.y * TH + p / TW;
    // a lane without a sample (outside the image, or AA 3's lane 63) traces nothing and rides along to the cross-lane sums with zeros
    const bool live = p < TW * TH && x < ow && y < oh;
    uint32_t rb = 0u, g = 0u;
    if (live) {
        const Cam cam = mk_cam(*reinterpret_cast<const F16*>(a.cam));
        const Box bound = mk_box(*reinterpret_cast<const Box8*>(a.bound));
        const uchar4 c = frame_sample<STAGES, GROUPS>(a, cam, bound, AA * x + s % AA, AA * y + s / AA);
        rb = (uint32_t)c.x | ((uint32_t)c.z << 16);
        g = c.y;
    }
    rb = aa_lane_sum<AA>(rb, lane, s);
    g = aa_lane_sum<AA>(g, lane, s);
    if (live && s == 0u) ((uchar4*)a.pixels)[(size_t)ow * y + x] = aa_average<AA>(rb, g);
}

static F16 mk16f(const float* f) { F16 r; for (int i = 0; i < 16; ++i) r.v[i] = f[i]; return r; }
static Box8 mk8f(const float* f) { Box8 r; for (int i = 0; i < 8; ++i) r.v[i] = f ? f[i] : 0.0f; return r; }
static dim3 grid2(uint32_t gx, uint32_t gy) { return dim3((gx + 31) / 32, (gy + 7) / 8); }

void launch_a01_raytrace(hipStream_t s, void* pixels, const float* cam, uint32_t gx, uint32_t gy) {
    if (!gx || !gy) return;
    hipLaunchKernelGGL(k_a01_raytrace, grid2(gx, gy), dim3(32, 8), 0, s, (uchar4*)pixels, mk16f(cam), gx, gy);
}
void launch_frame_initTrace(hipStream_t s, bool clip, void* pixels, const float* cam, void* rays, const float* bound, uint32_t gx, uint32_t gy) {
    if (!gx || !gy) return;
    if (clip) hipLaunchKernelGGL(k_frame_initTrace<true>, grid2(gx, gy), dim3(32, 8), 0, s, (uchar4*)pixels, mk16f(cam), (RayAoS*)rays, mk8f(bound), gx, gy);
    else hipLaunchKernelGGL(k_frame_initTrace<false>, grid2(gx, gy), dim3(32, 8), 0, s, (uchar4*)pixels, mk16f(cam), (RayAoS*)rays, mk8f(nullptr), gx, gy);
}
// the group spheres behind a grid's n_slots prepared records are consulted only where cells are long on average (coarse grids): where they
// start, in records, or 0 for the plain loop
static uint32_t frame_group_slots(uint32_t n_slabs, uint32_t n_slots) {
    const uint64_t cells = (uint64_t)n_slabs * n_slabs * n_slabs;
    return (uint64_t)n_slots >= cells * 4u * kTriGroup ? n_slots : 0u;
}
void launch_frame_stage(hipStream_t s, const FrameArgs& a, FrameStage stage) {
    if (!a.gx || !a.gy) return;
    const dim3 grid = grid2(a.gx, a.gy), block(32, 8);
    uchar4* pixels = (uchar4*)a.pixels;
    RayAoS* rays = (RayAoS*)a.rays;
    const float4 *prep = (const float4*)a.prep, *normals = (const float4*)a.normals;
    const uint32_t group_slots = stage == FS_MESH ? frame_group_slots(a.n_slabs, a.n_slots) : 0u;
    if (stage == FS_A04)
        hipLaunchKernelGGL(k_a04_meshTrace, grid, block, 0, s, pixels, mk16f(a.cam), rays, a.t_size, prep, normals, (const uint32_t*)a.mindex,
                           (const float4*)a.mcolor, a.ncolors, a.gx, a.gy);
    else if (stage == FS_MOL)
        hipLaunchKernelGGL(k_a07_molTrace, grid, block, 0, s, pixels, mk16f(a.cam), rays, (const float4*)a.atoms, mk8f(a.bound), a.n_slabs,
                           (const uint32_t*)a.mol_slab_size, a.gx, a.gy);
    else if (group_slots)
        hipLaunchKernelGGL(k_a07_meshTrace<true>, grid, block, 0, s, pixels, mk16f(a.cam), rays, prep, normals, mk8f(a.bound), a.n_slabs,
                           (const uint32_t*)a.slab_size, group_slots, a.gx, a.gy);
    else
        hipLaunchKernelGGL(k_a07_meshTrace<false>, grid, block, 0, s, pixels, mk16f(a.cam), rays, prep, normals, mk8f(a.bound), a.n_slabs,
                           (const uint32_t*)a.slab_size, 0u, a.gx, a.gy);
}

template <uint32_t STAGES, bool GROUPS>
static void launch_frame_fused_t(hipStream_t s, const FrameArgs& a) {
    if (a.rays) hipLaunchKernelGGL((k_frame_fused<STAGES, GROUPS, true>), grid2(a.gx, a.gy), dim3(32, 8), 0, s, a);
    else hipLaunchKernelGGL((k_frame_fused<STAGES, GROUPS, false>), grid2(a.gx, a.gy), dim3(32, 8), 0, s, a);
}
void launch_frame_fused(hipStream_t s, FrameArgs a) {
    if (!a.gx || !a.gy) return;
    if (a.assign == 4) { launch_frame_fused_t<FS_A04, false>(s, a); return; }
    a.group_slots = a.mesh ? frame_group_slots(a.n_slabs, a.n_slots) : 0u;
    const bool mesh = a.mesh != 0u, mol = a.mol != 0u;
    if (mesh && mol) { if (a.group_slots) launch_frame_fused_t<FS_MOL | FS_MESH, true>(s, a); else launch_frame_fused_t<FS_MOL | FS_MESH, false>(s, a); }
    else if (mesh) { if (a.group_slots) launch_frame_fused_t<FS_MESH, true>(s, a); else launch_frame_fused_t<FS_MESH, false>(s, a); }
    else if (mol) launch_frame_fused_t<FS_MOL, false>(s, a);
}

template <uint32_t STAGES, bool GROUPS, uint32_t AA>
static void launch_frame_aa_t(hipStream_t s, const FrameArgs& a, uint32_t ow, uint32_t oh) {
    // four waves a block, side by side: (4 * W) x H output pixels
    const dim3 grid((ow + 4u * AaWave<AA>::W - 1u) / (4u * AaWave<AA>::W), (oh + AaWave<AA>::H - 1u) / AaWave<AA>::H);
    hipLaunchKernelGGL((k_frame_aa_lanes<STAGES, GROUPS, AA>), grid, dim3(256), 0, s, a, ow, oh);
}
template <uint32_t STAGES, bool GROUPS>
static void launch_frame_aa_s(hipStream_t s, const FrameArgs& a, uint32_t aa, uint32_t ow, uint32_t oh) {
    if (aa == 2u) launch_frame_aa_t<STAGES, GROUPS, 2>(s, a, ow, oh);
    else if (aa == 3u) launch_frame_aa_t<STAGES, GROUPS, 3>(s, a, ow, oh);
    else if (aa == 4u) launch_frame_aa_t<STAGES, GROUPS, 4>(s, a, ow, oh);
}
void launch_frame_aa(hipStream_t s, FrameArgs a, uint32_t aa, uint32_t ow, uint32_t oh) {
    if (!ow || !oh) return;
    if (a.assign == 4) { launch_frame_aa_s<FS_A04, false>(s, a, aa, ow, oh); return; }
    a.group_slots = a.mesh ? frame_group_slots(a.n_slabs, a.n_slots) : 0u;
    const bool mesh = a.mesh != 0u, mol = a.mol != 0u;
    if (mesh && mol) { if (a.group_slots) launch_frame_aa_s<FS_MOL | FS_MESH, true>(s, a, aa, ow, oh); else launch_frame_aa_s<FS_MOL | FS_MESH, false>(s, a, aa, ow, oh); }
    else if (mesh) { if (a.group_slots) launch_frame_aa_s<FS_MESH, true>(s, a, aa, ow, oh); else launch_frame_aa_s<FS_MESH, false>(s, a, aa, ow, oh); }
    else if (mol) launch_frame_aa_s<FS_MOL, false>(s, a, aa, ow, oh);
}

}  // namespace pt
