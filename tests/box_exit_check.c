/* tests/box_exit_check.c -- stand-alone check of the one slab pass of a single-cell set (csrc/pt_trace.hpp box_exit1; constants and derivation:
   csrc/pt_box_exit.hpp, which this file includes) against the two functions it replaces (inter_aabb_t<FAST, false> and cell1_exit<FAST>), on the CPU.
   tests/test_box_exit.py compiles and runs it:   box_exit_check SEED CASES [SHRINK]   (SHRINK: the host's bound times 2^-SHRINK)

   Boxes: lo and hi with random mantissas over forty octaves of scale, or on a coarse lattice, or cornell.xml's sphere box; the exit plane is the
   reference's up = lo + 1*((hi - lo)/1), which lands below, on or above hi by an ulp or two -- all 27 combinations over the three axes occur and are
   counted.  Rays, per box: (0) random origins and directions; (1) aimed at a point of an edge or a corner of the box or of the exit planes, moved by
   zero to three representable steps either way; (2) starting within three steps of a far face or exit plane; (3) as (0) with direction components
   down to 2^-40.  A ray outside the ray-side guard windows (pt_trace.hpp ray_guard) is skipped: such a lane defers before it divides.

   The two-function form divides with `/` (the reference's correctly rounded quotient), the one pass with the kernel's three-operation quotient on the
   correctly rounded reciprocal; printed, in this order:
     cases skipped both_true  differ overruled  bit_mismatches violations  close ordinary ordinary_overruled  combos
   differ: the two final verdicts disagree.  close: lanes whose window is shorter than the host's bound, which take the box's own comparison on the
   axes with up > hi.  overruled: close lanes which that comparison drops.  bit_mismatches: tmin or the exit differ as floats (a zero of either sign
   is one value).  violations: the final verdicts disagree and the reference's window [tmin, exit] is not empty -- a lane that was not close and needed
   the box's comparison.  ordinary: rays of kind (0) that pass tmin <= exit on cornell.xml's sphere box, ordinary_overruled those of them the box's
   comparison drops.  combos: how many of the 27 relations occurred. */
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

#include "pt_box_exit.hpp"

static uint64_t rng_state;
static uint64_t rnd64(void) {   /* splitmix64 */
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t rnd(uint32_t n) { return (uint32_t)(rnd64() % n); }
static float unit(void) { return (float)((double)(rnd64() >> 11) * 0x1p-53); }          /* [0, 1) */
static float sym(void) { return (float)((double)(rnd64() >> 11) * 0x1p-52 - 1.0); }     /* [-1, 1) */
static float steps(float v, int n) {
    for (; n > 0; --n) v = nextafterf(v, INFINITY);
    for (; n < 0; ++n) v = nextafterf(v, -INFINITY);
    return v;
}

/* the windows of the optimistic kernel (csrc/pt_windows.hpp): |d| in [2^-40, 2^40]; o, bounds and exit planes zero or in [2^-30, 2^20] */
static int den_ok(float d) { return fabsf(d) >= 0x1p-40f && fabsf(d) <= 0x1p40f; }
static int pos_ok(float p) { return p == 0.0f || (fabsf(p) >= 0x1p-30f && fabsf(p) <= 0x1p20f); }

/* the kernel's quotient (pt_trace.hpp box_exit1 `quo`, pt_numerics.hpp div_exact3_anyzero) */
static float quo(float num, float d, float r) {
    const float q0 = num * r;
    return fmaf(fmaf(-d, q0, num), r, q0);
}

typedef struct Box1 { float lo[3], hi[3], up[3]; uint32_t far_axes; BoxExit e; int cornell; } Box1;

static int make_box(Box1* b, int shrink) {
    float b8[8];
    const int kind = (int)rnd(8);
    const float scale = ldexpf(1.0f, (int)rnd(41) - 24);   /* 2^-24 .. 2^16 */
    int k;
    for (k = 0; k < 3; ++k) {
        float lo, hi;
        if (kind == 0) {          /* cornell.xml's sphere box, as the fixture has it */
            static const float L[3] = {-0.4f, -1.0f, -0.4f}, H[3] = {0.7f, -0.4f, 0.5f};   /* up above hi on x and y, below it on z */
            lo = L[k]; hi = H[k];
        } else if (kind == 1) {   /* a coarse lattice: up == hi mostly */
            lo = ((float)rnd(64) - 32.0f) * 0.125f * scale;
            hi = lo + (float)(1 + rnd(32)) * 0.125f * scale;
        } else {                  /* random mantissas, either sign, independent or within a sixty-fourth of each other */
            lo = sym() * scale;                                  /* (hi made as lo + width would make hi - lo exact and up == hi) */
            hi = rnd(2) ? sym() * scale : lo * (1.0f + unit() * 0x1p-6f);
            if (hi < lo) { const float t = lo; lo = hi; hi = t; }
            if (hi == lo) hi = lo + scale;
        }
        b->lo[k] = lo; b->hi[k] = hi;
    }
    b->far_axes = 0u;
    b->cornell = kind == 0;
    for (k = 0; k < 3; ++k) {
        const float delta = (b->hi[k] - b->lo[k]) / 1.0f;
        b->up[k] = b->lo[k] + 1.0f * delta;                 /* A10 code.cl:699-707 (pt_set_guard.hpp exit_planes) */
        if (b->up[k] == b->hi[k]) b->far_axes |= 1u << k;
        if (!(b->lo[k] <= b->hi[k]) || !pos_ok(b->lo[k]) || !pos_ok(b->hi[k]) || !pos_ok(b->up[k])) return 0;   /* not fast_ok (pt_set_guard.hpp) */
        b8[k] = b->lo[k]; b8[4 + k] = b->hi[k];
    }
    b8[3] = b8[7] = 1.0f;
    b->e = box_exit_consts(b8, b->up);
    for (k = 0; k < 3; ++k) b->e.gap[k] = ldexpf(b->e.gap[k], -shrink);
    b->e.gap_max = ldexpf(b->e.gap_max, -shrink);
    return 1;
}
static int combo_of(const Box1* b) {
    int c = 0, k;
    for (k = 0; k < 3; ++k) c = c * 3 + (b->up[k] < b->hi[k] ? 0 : b->up[k] == b->hi[k] ? 1 : 2);
    return c;
}

/* a coordinate of interest on axis k: a face, the exit plane, or somewhere between */
static float plane_of(const Box1* b, int k, int which) {
    switch (which) { case 0: return b->lo[k]; case 1: return b->hi[k]; case 2: return b->up[k]; default: return b->lo[k] + unit() * (b->hi[k] - b->lo[k]); }
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    rng_state = strtoull(argv[1], 0, 10) * 0x2545F4914F6CDD1Dull + 1u;
    const uint64_t cases = strtoull(argv[2], 0, 10);
    const int shrink = argc > 3 ? atoi(argv[3]) : 0;
    uint64_t n = 0, skipped = 0, both = 0, differ = 0, deferred = 0, mismatches = 0, violations = 0, close_n = 0, ordinary = 0, ordinary_deferred = 0;
    uint32_t combos[27];
    Box1 b;
    int have = 0, k;
    memset(combos, 0, sizeof combos);
    while (n < cases) {
        if (!have || (n & 1023u) == 0u) {
            have = make_box(&b, shrink);
            if (!have) continue;
            combos[combo_of(&b)]++;
        }
        ++n;
        const float ext = fmaxf(fmaxf(b.hi[0] - b.lo[0], b.hi[1] - b.lo[1]), b.hi[2] - b.lo[2]);
        const int kind = (int)rnd(4);
        float o[3], d[3];
        for (k = 0; k < 3; ++k) {   /* kinds 0 and 3: an origin within a few extents of the box, a direction of any orientation */
            o[k] = 0.5f * (b.lo[k] + b.hi[k]) + sym() * ext * (rnd(4) ? 2.0f : 0.4f);
            d[k] = sym();
        }
        if (kind == 1) {            /* aimed at a point of an edge or a corner, a few representable steps off */
            float t[3];
            const int free_axis = rnd(4) == 0 ? -1 : (int)rnd(3);
            for (k = 0; k < 3; ++k) t[k] = steps(plane_of(&b, k, k == free_axis ? 3 : (int)rnd(3)), (int)rnd(7) - 3);
            for (k = 0; k < 3; ++k) d[k] = t[k] - o[k];
            if (rnd(2)) { const float s = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); for (k = 0; k < 3; ++k) d[k] *= s; }
        } else if (kind == 2) {     /* starting within three steps of a far face or an exit plane, inside the box on the other axes or near them too */
            const int a = (int)rnd(3);
            for (k = 0; k < 3; ++k) o[k] = rnd(4) ? plane_of(&b, k, 3) : steps(plane_of(&b, k, 1 + (int)rnd(2)), (int)rnd(7) - 3);
            o[a] = steps(plane_of(&b, a, 1 + (int)rnd(2)), (int)rnd(7) - 3);
        } else if (kind == 3) {
            for (k = 0; k < 3; ++k) if (rnd(2)) d[k] = ldexpf(d[k], -(int)rnd(40));
        }
        if (!(den_ok(d[0]) && den_ok(d[1]) && den_ok(d[2]) && pos_ok(o[0]) && pos_ok(o[1]) && pos_ok(o[2]))) { ++skipped; continue; }

        /* the two functions, the reference's divisions (pt_trace.hpp inter_aabb_t<FAST, false>, cell1_exit<FAST>) */
        float tn[3], tf[3], ex[3];
        for (k = 0; k < 3; ++k) {
            const float q0 = (b.lo[k] - o[k]) / d[k], q1 = (b.hi[k] - o[k]) / d[k], qu = (b.up[k] - o[k]) / d[k];
            tn[k] = fminf(q0, q1); tf[k] = fmaxf(q0, q1);
            ex[k] = (((b.far_axes >> k) & 1u) != 0u || !(d[k] >= 0.0f)) ? tf[k] : qu;
        }
        const float tmin0 = fmaxf(fmaxf(tn[0], tn[1]), fmaxf(tn[2], 0.0f)), tmax0 = fminf(fminf(tf[0], tf[1]), tf[2]);
        const float exit0 = fminf(fminf(ex[0], ex[1]), ex[2]);
        const int v0 = !(tmin0 > tmax0);

        /* the one pass (pt_trace.hpp box_exit1) */
        float r[3], nr[3], fr[3];
        for (k = 0; k < 3; ++k) {
            r[k] = 1.0f / d[k];
            const float nl = b.lo[k] - o[k], nh = b.hi[k] - o[k], nu = b.up[k] - o[k];
            const int fwd = d[k] >= 0.0f;
            nr[k] = quo(fwd ? nl : nh, d[k], r[k]);
            fr[k] = quo(fwd ? nu : nl, d[k], r[k]);
        }
        const float tmin1 = fmaxf(fmaxf(nr[0], nr[1]), fmaxf(nr[2], 0.0f)), cmax1 = fminf(fminf(fr[0], fr[1]), fr[2]);
        int v1 = !(tmin1 > cmax1), overruled = 0;
        if (b.e.gap_max != 0.0f) {
            const float room = fmaf(cmax1, 0.99999904632568359375f, -tmin1);
            const float rmax = fmaxf(fmaxf(fabsf(r[0]), fabsf(r[1])), fabsf(r[2]));
            const int close = v1 && !(room >= b.e.gap_max * rmax);
            if (close) {   /* (the kernel lets the whole wave take this comparison; a lane that is not close must not need it: that is the check) */
                float tmax1 = cmax1;
                for (k = 0; k < 3; ++k)
                    if (((b.e.above >> k) & 1u) && d[k] >= 0.0f) tmax1 = fminf(tmax1, quo(b.hi[k] - o[k], d[k], r[k]));
                overruled = tmin1 > tmax1;
                v1 = !overruled;
                ++close_n;
            }
        }
        if (!(tmin1 == tmin0) || !(cmax1 == exit0)) ++mismatches;
        if (v0 && v1) ++both;
        if (overruled) ++deferred;
        if (v0 != v1) {
            ++differ;
            const int empty = tmin0 > exit0;          /* the reference asks for tmin <= t <= exit: nothing can answer */
            if (!(v0 && empty)) ++violations;
        }
        if (b.cornell && kind == 0 && !(tmin1 > cmax1)) { ++ordinary; if (overruled) ++ordinary_deferred; }
    }
    int seen = 0;
    for (k = 0; k < 27; ++k) seen += combos[k] != 0u;
    printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", n, skipped, both,
           differ, deferred, mismatches, violations, close_n, ordinary, ordinary_deferred, seen);
    return 0;
}
