/* tests/shadow_gap_check.c -- TEST INFRASTRUCTURE, a stand-alone program (tests/test_shadow_gap.py compiles and runs it; no GPU).
 *
 * The claim the shadow stage's early-out rests on (2015-raytracing_amd/csrc/pt_direct.hpp gap_test, pt_shadow_gap.hpp):
 *
 *      a shadow segment passes the gap test of a single-cell triangle set
 *          ==>  the reference's box test says v, tmin == 0, and neither the box's tmax nor the cell's exit is below maxt
 *          and  every axis-plane triangle of the set, in either winding, is rejected by the reference's test or has t >= maxt
 *          and  the sweep's own verdict (pt_trace.hpp trace_cell1, restated below) on every axis entry, front and back, is "drop"
 *
 * The third line is the mechanism the margin is made for: the early-out steps past exactly the entries the sweep would have dropped.  It is
 * also the line that can tell a margin that is too small.  The first two cannot, for AXIS planes: both edges of such a triangle are exactly
 * zero along the axis, so every term of the reference's numerator of t is a product with s_a = o_a - q and its sign is exact -- it is the
 * sweep's fused evaluation, whose margin M is made for general planes, that keeps a plane nearer than M; and end_a, a float strictly inside
 * the gap, has the exact end strictly inside too.
 *
 * Restated here in C with fmaf under the numerics contract (correctly rounded division): the reference's box test (A10 code.cl:340-390) and
 * cell exit (code.cl:699-707), the reference's interTriangle (code.cl:250-288), and the kernel's gap test with the HOST'S constants -- this file
 * includes pt_shadow_gap.hpp itself and feeds it a plane list in the layout of pt_launch.hpp, so the parser and the constants are the product's.
 *
 * usage: shadow_gap_check SEED CASES SHRINK     SHRINK: the margins are cut by 2^-SHRINK (0: the product's)
 * prints one line: cases passes violations box_violations triangle_violations sweep_keeps interior interior_passes skipped
 *   cases: segments inside the guard windows; passes: of those, the gap test passed; interior: segments of the cornell-like room from an origin
 *   0.001 off a surface to a point of the light's disk. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pt_shadow_gap.hpp"

typedef struct { float x, y, z; } v3;
static float comp(v3 a, int k) { return k == 0 ? a.x : (k == 1 ? a.y : a.z); }
static v3 mk(float x, float y, float z) { v3 r = {x, y, z}; return r; }
static v3 with(v3 a, int k, float v) { if (k == 0) a.x = v; else if (k == 1) a.y = v; else a.z = v; return a; }
static v3 sub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static float dot(v3 a, v3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static v3 cross(v3 a, v3 b) { return mk(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x))); }
static float l1(v3 a) { return (fabsf(a.x) + fabsf(a.y)) + fabsf(a.z); }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static uint64_t mix64(uint64_t* s) {
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static float urand(uint64_t* s) { return (float)((mix64(s) >> 40) * (1.0 / 16777216.0)); }
static float range(uint64_t* s, float lo, float hi) { return lo + (hi - lo) * urand(s); }
static uint32_t pick(uint64_t* s, uint32_t n) { return (uint32_t)(mix64(s) % n); }

/* ---- the reference ---------------------------------------------------------------------------------------------------------------- */
/* interTriangle on (p0, e1, e2), A10 rule, window [cmin, cmax] and t < maxt */
static int ref_tri(v3 o, v3 d, float cmin, float cmax, float maxt, v3 p0, v3 e1, v3 e2) {
    const v3 n = cross(e2, e1);
    const float div = dot(n, d);
    if (div <= 0.0f) return 0;
    const float idiv = 1.0f / div;
    const v3 s = sub(o, p0);
    const float beta = dot(cross(s, d), e2) * idiv;
    if (beta < 0.0f || beta > 1.0f) return 0;
    const float gamma = dot(cross(s, e1), d) * idiv;
    const float gb = gamma + beta;
    if (gamma < 0.0f || gb < 0.0f || gb > 1.0f) return 0;
    const float t = dot(cross(s, e2), e1) * -idiv;
    return t >= cmin && t <= cmax && t < maxt;
}
/* the box test: v, tmin, tmax; and the single cell's exit t */
static int ref_box(v3 o, v3 d, const float* b8, float* tmin, float* tmax, float* exit_t) {
    float mn = 0.0f, mx = INFINITY, ex = INFINITY;
    int v = 1;
    for (int k = 0; k < 3; ++k) {
        const float lo = b8[k], hi = b8[4 + k], ok = comp(o, k), dk = comp(d, k);
        const float t0 = (lo - ok) / dk, t1 = (hi - ok) / dk;
        const float tn = dk < 0 ? t1 : t0, tf = dk < 0 ? t0 : t1;
        mn = fmaxf(tn, mn);
        mx = fminf(tf, mx);
        if (mn > mx) v = 0;
        const float delta = (hi - lo) / 1.0f;
        const float xnext = lo + (float)(dk >= 0 ? 1 : 0) * delta;
        ex = fminf(ex, (xnext - ok) / dk);
    }
    *tmin = mn; *tmax = mx; *exit_t = ex;
    return v;
}
/* the kernel's gap test (pt_direct.hpp gap_test), operation for operation */
static int gap_test(v3 o, v3 d, float maxt, const struct ShadowGap* g) {
    const float o1 = (fabsf(o.x) + fabsf(o.y)) + fabsf(o.z);
    const float hi_p = fmaxf(maxt * 1.00000095367431640625f, 0x1p-100f);
    int pass = 1;
    for (int a = 0; a < 3; ++a) {
        const float e = fmaf(hi_p, comp(d, a), comp(o, a));
        const float m = fmaf(g->gm[a], o1, g->hm[a]);
        pass &= (fminf(comp(o, a), e) - g->qlo[a] > m) & (g->qhi[a] - fmaxf(comp(o, a), e) > m);
    }
    return pass;
}
/* the sweep's verdicts on an axis entry {q, n_a} (pt_trace.hpp trace_cell1: verdict, PT_AXIS_GROUPS) in the window of a gap query: cmin = 0,
   cmax = maxt.  1: some record of the entry, front or back, stays a candidate */
static int sweep_keeps_axis(v3 o, v3 d, float maxt, int a, float q, float na, float gmax, float hmax) {
    const float o1 = (fabsf(o.x) + fabsf(o.y)) + fabsf(o.z);
    const float hi_p = fmaxf(maxt * 1.00000095367431640625f, 0x1p-100f), lo_m = 0.0f * 0.99999904632568359375f;
    const float M = fmaf(gmax, o1, hmax);
    const float div = na * comp(d, a), sn = na * (comp(o, a) - q);
    const float sp = sn + M, sm = sn - M;
    const float w = fminf(fminf(div, fmaf(hi_p, div, sp)), -fmaf(lo_m, div, sm));
    const float wb = fminf(fminf(-div, -fmaf(hi_p, div, sm)), fmaf(lo_m, div, sp));
    return (bits(w) >> 31) == 0u || (bits(wb) >> 31) == 0u;
}
/* the ray-side guard (pt_trace.hpp ray_guard): a ray outside it is the exact kernel's, whatever the optimistic one computes */
static int ray_guard(v3 o, v3 d) {
    for (int k = 0; k < 3; ++k) {
        const float a = fabsf(comp(d, k)), p = fabsf(comp(o, k));
        if (!(a >= 0x1p-40f && a <= 0x1p40f)) return 0;
        if (!(p == 0.0f || (p >= 0x1p-30f && p <= 0x1p20f))) return 0;
    }
    return 1;
}

/* ---- a set: at most 32 records (one chunk), its box, its plane list in the product's layout ------------------------------------------- */
enum { MAXT = 32 };
typedef struct {
    uint32_t n;
    v3 p0[MAXT], e1[MAXT], e2[MAXT];
    int axis[MAXT];          /* 0..2: an axis-plane record; 3: general */
    float b8[8], exit_up[3];
    uint32_t words[16 + 16 * (MAXT + 4)];
    struct GapPlanes planes;
    struct ShadowGap gap;
} Set;

static void add_tri(Set* S, v3 a, v3 b, v3 c) {
    if (S->n >= MAXT) return;
    S->p0[S->n] = a; S->e1[S->n] = sub(b, a); S->e2[S->n] = sub(c, a);
    S->n++;
}
/* a rectangle in the plane {x_ax = q}, cut in two, winding by `flip` */
static void add_axis_quad(Set* S, int ax, float q, float u0, float u1, float w0, float w1, int flip) {
    const int ua = (ax + 1) % 3, wa = (ax + 2) % 3;
    v3 p[4];
    for (int i = 0; i < 4; ++i) {
        p[i] = with(mk(0, 0, 0), ax, q);
        p[i] = with(p[i], ua, (i == 1 || i == 2) ? u1 : u0);
        p[i] = with(p[i], wa, (i >= 2) ? w1 : w0);
    }
    if (flip) { add_tri(S, p[0], p[2], p[1]); add_tri(S, p[0], p[3], p[2]); }
    else { add_tri(S, p[0], p[1], p[2]); add_tri(S, p[0], p[2], p[3]); }
}
/* the plane list (pt_launch.hpp), one entry per record (merging records of one plane is an optimisation of k_planeList, not part of the layout),
   the chunk's largest margin constants as k_planeList forms them; then the host's parser and constants */
static int finish(Set* S, double scale) {
    const float up = 1.0000002384185791015625f;
    float gmax = 0.0f, hmax = 0.0f;
    uint32_t cnt[4] = {0, 0, 0, 0};
    memset(S->words, 0, sizeof S->words);
    for (uint32_t i = 0; i < S->n; ++i) {
        const v3 n = cross(S->e2[i], S->e1[i]);
        const float nn[3] = {n.x, n.y, n.z};
        int cl = 3;
        for (int a = 0; a < 3; ++a)
            if (nn[a] != 0.0f && nn[(a + 1) % 3] == 0.0f && nn[(a + 2) % 3] == 0.0f && comp(S->e1[i], a) == 0.0f && comp(S->e2[i], a) == 0.0f) cl = a;
        S->axis[i] = cl;
        cnt[cl]++;
        const float E = (l1(S->e1[i]) * up) * (l1(S->e2[i]) * up) * up;
        const float G = 0x1p-17f * E;
        const float H = fmaxf(G * (l1(S->p0[i]) * up) * up, 0x1p-56f);
        gmax = fmaxf(gmax, G); hmax = fmaxf(hmax, H);
    }
    uint32_t groups = 0, packed = 0;
    for (int cl = 0; cl < 4; ++cl) {
        const uint32_t per = cl < 3 ? 4u : 2u, nw = cl < 3 ? 4u : 8u;
        uint32_t k = 0;
        for (uint32_t i = 0; i < S->n; ++i) {
            if (S->axis[i] != cl) continue;
            uint32_t* e = S->words + 16 + 16 * groups + nw * k++;
            const v3 n = cross(S->e2[i], S->e1[i]);
            if (cl < 3) { float q = comp(S->p0[i], cl) + 0.0f, na = comp(n, cl); memcpy(e, &q, 4); memcpy(e + 1, &na, 4); e[2] = 0x80000000u >> i; }
            else { memcpy(e, &n.x, 4); memcpy(e + 1, &n.y, 4); memcpy(e + 2, &n.z, 4); e[4] = 0x80000000u >> i; }
        }
        const uint32_t g = (cnt[cl] + per - 1u) / per;
        packed |= g << (8 * cl);
        groups += g;
    }
    S->words[0] = packed; S->words[4] = 0u;
    memcpy(&S->words[8], &gmax, 4); memcpy(&S->words[12], &hmax, 4);
    for (int k = 0; k < 3; ++k) {   /* pt_set_guard.hpp exit_planes */
        const float delta = (S->b8[4 + k] - S->b8[k]) / 1.0f;
        S->exit_up[k] = S->b8[k] + 1.0f * delta;
    }
    if (!gap_planes_from_list(S->words, 16u + 16u * groups, S->n, &S->planes)) return 0;
    S->gap = shadow_gap(S->b8, S->exit_up, &S->planes, scale);
    return (int)S->gap.ok;
}

/* a coordinate on axis a for an end of a segment: inside the gap, or at 0.5 / 1 / 2 margins or 1e-3 of the scale from either end of it */
static float place(uint64_t* s, const Set* S, int a, float m, float scale) {
    const float lo = S->gap.qlo[a], hi = S->gap.qhi[a];
    const uint32_t w = pick(s, 12);
    static const float f[3] = {0.5f, 1.0f, 2.0f};
    if (w < 3) return lo + f[w] * m;
    if (w < 6) return hi - f[w - 3] * m;
    if (w == 6) return lo + 1e-3f * scale;
    if (w == 7) return hi - 1e-3f * scale;
    return range(s, lo, hi);
}

/* ADVERSARIAL: a segment aimed at an axis-plane record that lies in one end of the gap.  P: a point of the record; h: 0.5 / 1 / 2 margins or one to four
   representable steps off the plane, on the gap's side.  Either the segment STARTS at height h over P and leads away (the plane is behind the origin by
   h: the reference's t is negative by a few roundings only), or it ENDS at height h over P (it stops that short of the plane: the reference's t is
   beyond maxt by as little), the origin anywhere in the gap -- nearly in the plane included, where an error of the numerator is worth the most t. */
static int aim(uint64_t* s, const Set* S, float scale, v3* o, v3* e) {
    uint32_t found[MAXT], nf = 0;
    for (uint32_t i = 0; i < S->n; ++i) {
        const int a = S->axis[i];
        if (a < 3 && (comp(S->p0[i], a) == S->gap.qlo[a] || comp(S->p0[i], a) == S->gap.qhi[a])) found[nf++] = i;
    }
    if (!nf) return 0;
    const uint32_t i = found[pick(s, nf)];
    const int a = S->axis[i];
    const float q = comp(S->p0[i], a);
    const float sgn = q == S->gap.qlo[a] ? 1.0f : -1.0f;
    float b = urand(s), g = urand(s);
    if (b + g > 1.0f) { b = 1.0f - b; g = 1.0f - g; }
    v3 P = mk(S->p0[i].x + b * S->e1[i].x + g * S->e2[i].x, S->p0[i].y + b * S->e1[i].y + g * S->e2[i].y, S->p0[i].z + b * S->e1[i].z + g * S->e2[i].z);
    v3 other = mk(0, 0, 0);
    const float o1 = l1(P);
    for (int k = 0; k < 3; ++k) other = with(other, k, place(s, S, k, fmaf(S->gap.gm[k], o1, S->gap.hm[k]), scale));
    const float m = fmaf(S->gap.gm[a], o1, S->gap.hm[a]);
    const uint32_t w = pick(s, 8);
    static const float f[4] = {0.5f, 1.0f, 1.0625f, 2.0f};
    float x = q + sgn * f[w & 3] * m;
    if (w >= 4) { x = q; for (uint32_t k = 0; k <= (w & 3); ++k) x = nextafterf(x, sgn * INFINITY); }
    P = with(P, a, x);
    if (pick(s, 2)) { *o = P; *e = other; if (pick(s, 2)) *e = with(*e, a, x + sgn * ldexpf(fabsf(x) + scale, -(int)pick(s, 30))); }
    else { *e = P; *o = other; if (pick(s, 2)) *o = with(*o, a, x + sgn * ldexpf(fabsf(x) + scale, -(int)pick(s, 30))); }
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: shadow_gap_check SEED CASES SHRINK\n"); return 2; }
    uint64_t seed = strtoull(argv[1], 0, 10) * 0xD1B54A32D192ED03ull + 0x8CB92BA72F3D8DD7ull;
    uint64_t rng = mix64(&seed);   /* (the generator steps by a constant: seeds must not be a step apart) */
    const uint64_t want = strtoull(argv[2], 0, 10);
    const double shrink = ldexp(1.0, -atoi(argv[3]));
    uint64_t cases = 0, passes = 0, viol = 0, box_viol = 0, tri_viol = 0, sweep_viol = 0, interior = 0, interior_pass = 0, skipped = 0;
    static Set S;
    while (cases < want) {
        /* ---- a set, at one of forty octaves of scale ---- */
        const float sc = ldexpf(1.0f, (int)pick(&rng, 40) - 20);
        const uint32_t kind = pick(&rng, 4);   /* 0, 1: a room like cornell.xml's; 2: an axis-plane soup; 3: no axis planes */
        memset(&S, 0, sizeof S);
        float blo[3], bhi[3];
        for (int k = 0; k < 3; ++k) { blo[k] = -sc; bhi[k] = sc; }
        if (kind >= 2) for (int k = 0; k < 3; ++k) { blo[k] = range(&rng, -2.0f, 0.5f) * sc; bhi[k] = blo[k] + range(&rng, 0.25f, 2.0f) * sc; }
        for (int k = 0; k < 3; ++k) { S.b8[k] = blo[k]; S.b8[4 + k] = bhi[k]; }
        S.b8[3] = S.b8[7] = 1.0f;
        if (kind < 2) {
            const float w = 0.99f * sc;
            add_axis_quad(&S, 0, -w, -w, w, -w, w, (int)pick(&rng, 2));
            add_axis_quad(&S, 0, w, -w, w, -w, w, (int)pick(&rng, 2));
            add_axis_quad(&S, 1, -w, -w, w, -w, w, (int)pick(&rng, 2));
            add_axis_quad(&S, 1, w, -w, w, -w, w, (int)pick(&rng, 2));
            add_axis_quad(&S, 2, -w, -w, w, -w, w, (int)pick(&rng, 2));
            if (kind == 1) add_axis_quad(&S, 2, bhi[2], -w, w, -w, w, (int)pick(&rng, 2));   /* a plane on the box's face */
        }
        if (kind == 2) {
            const uint32_t quads = 1 + pick(&rng, 12);
            for (uint32_t i = 0; i < quads; ++i) {
                const int ax = (int)pick(&rng, 3), ua = (ax + 1) % 3, wa = (ax + 2) % 3;
                const uint32_t where = pick(&rng, 8);
                const float q = where == 0 ? blo[ax] : where == 1 ? bhi[ax] : where == 2 ? blo[ax] - 0.1f * sc : where == 3 ? range(&rng, -0.03f, 0.03f) * sc : range(&rng, blo[ax], bhi[ax]);
                const float u0 = range(&rng, blo[ua] - 0.2f * sc, bhi[ua]), w0 = range(&rng, blo[wa] - 0.2f * sc, bhi[wa]);
                add_axis_quad(&S, ax, q, u0, u0 + range(&rng, 0.05f, 2.5f) * sc, w0, w0 + range(&rng, 0.05f, 2.5f) * sc, (int)pick(&rng, 2));
            }
        }
        for (uint32_t i = 0, n = 1 + pick(&rng, 3); i < n; ++i) {   /* general triangles: listed, never part of the claim */
            v3 a = mk(range(&rng, -0.5f, 0.5f) * sc, range(&rng, -0.5f, 0.5f) * sc, range(&rng, -0.5f, 0.5f) * sc);
            add_tri(&S, a, mk(a.x + 0.3f * sc, a.y + range(&rng, 0.01f, 0.2f) * sc, a.z), mk(a.x, a.y + 0.1f * sc, a.z + 0.3f * sc));
        }
        if (!finish(&S, shrink)) { skipped++; if (skipped > 100 * (want + 1000)) break; continue; }
        /* ---- segments against it ---- */
        for (uint32_t it = 0; it < 64 && cases < want; ++it) {
            v3 o = mk(0, 0, 0), e = mk(0, 0, 0);
            const int room_interior = kind < 2 && it < 16;
            if (room_interior) {
                /* an origin 0.001 off a wall, the floor or the ceiling (or anywhere inside), an end point on the light's disk */
                const float w = 0.99f * sc, off = 0.001f * sc;
                o = mk(range(&rng, -w + off, w - off), range(&rng, -w + off, w - off), range(&rng, -w + off, (kind == 1 ? w : sc) - off));
                const uint32_t face = pick(&rng, 8);
                if (face < 5) o = with(o, (int)(face % 3), (face == 3 || face == 4) ? w - off : -w + off);
                const float r = 0.2f * sc * sqrtf(urand(&rng)), ph = 6.2831853f * urand(&rng);
                e = mk(r * cosf(ph), 0.75f * sc, r * sinf(ph));
            } else if (it % 3 == 0 && aim(&rng, &S, sc, &o, &e)) {
                /* (aimed at an axis-plane record of the gap's own end: below) */
            } else {
                v3 guess =mk(range(&rng, S.gap.qlo[0], S.gap.qhi[0]), range(&rng, S.gap.qlo[1], S.gap.qhi[1]), range(&rng, S.gap.qlo[2], S.gap.qhi[2]));
                const float o1 = l1(guess);
                for (int a = 0; a < 3; ++a) {
                    const float m = fmaf(S.gap.gm[a], o1, S.gap.hm[a]);
                    o = with(o, a, place(&rng, &S, a, m, sc));
                    e = with(e, a, place(&rng, &S, a, m, sc));
                }
            }
            const v3 v = sub(e, o);
            const float len = sqrtf(dot(v, v));
            if (!(len > 0.0f)) continue;
            v3 d = mk(v.x / len, v.y / len, v.z / len);
            float maxt = len;
            if (!room_interior) {
                const uint32_t w = pick(&rng, 8);
                if (w == 0) d = with(d, (int)pick(&rng, 3), (pick(&rng, 2) ? 1.0f : -1.0f) * ldexpf(1.0f, -40 + (int)pick(&rng, 12)));   /* |d_a| at the guard window's edge */
                if (w == 1) maxt = len * range(&rng, 0.25f, 4.0f);
            }
            if (!ray_guard(o, d)) { skipped++; continue; }
            cases++;
            if (room_interior) interior++;
            if (!gap_test(o, d, maxt, &S.gap)) continue;
            passes++;
            if (room_interior) interior_pass++;
            float tmin, tmax, ex;
            const int bv = ref_box(o, d, S.b8, &tmin, &tmax, &ex);
            int bad = 0;
            if (!(bv && tmin == 0.0f && tmax >= maxt && ex >= maxt)) { box_viol++; bad = 1; }
            for (uint32_t i = 0; i < S.n; ++i) {
                if (S.axis[i] == 3) continue;
                /* the window the product would compare with (cmin = 0, cmax = maxt), and the reference's own (tmin, the cell's exit) */
                if (ref_tri(o, d, 0.0f, maxt, maxt, S.p0[i], S.e1[i], S.e2[i]) || ref_tri(o, d, 0.0f, maxt, maxt, S.p0[i], S.e2[i], S.e1[i]) ||
                    ref_tri(o, d, tmin, ex, maxt, S.p0[i], S.e1[i], S.e2[i]) || ref_tri(o, d, tmin, ex, maxt, S.p0[i], S.e2[i], S.e1[i])) { tri_viol++; bad = 1; }
                float gmax, hmax;
                memcpy(&gmax, &S.words[8], 4); memcpy(&hmax, &S.words[12], 4);
                const v3 n = cross(S.e2[i], S.e1[i]);
                if (sweep_keeps_axis(o, d, maxt, S.axis[i], comp(S.p0[i], S.axis[i]) + 0.0f, comp(n, S.axis[i]), gmax, hmax)) { sweep_viol++; bad = 1; }
            }
            viol += (uint64_t)bad;
        }
    }
    printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)cases, (unsigned long long)passes, (unsigned long long)viol, (unsigned long long)box_viol,
           (unsigned long long)tri_viol, (unsigned long long)sweep_viol, (unsigned long long)interior, (unsigned long long)interior_pass, (unsigned long long)skipped);
    return 0;
}
