// pt_shadow_gap.hpp -- the PLANE-FREE GAP of a single-cell triangle set: what the host works out once per set so that the optimistic kernel's
// shadow stage (pt_direct.hpp direct_all) may skip the set's box test and every axis-plane entry of its plane list for a wave whose shadow
// SEGMENTS all stay between the set's axis planes.  Plain C arithmetic on the host's copy of the plane list (k_planeList's words, pt_launch.hpp
// "plane list") and the set's bounds -- no HIP header, no context and no buffer; written in the common subset of C and C++ so that
// tests/shadow_gap_check.c includes this very file.  mirt_abi.cpp is the caller (ensure_prepared reads the list back once per buffer content;
// fill_grid makes the gap for the bounds of the launch) and copies the result into GridArgs::gap / gap_ok.
//
// The gap, per axis a: the open interval (qlo_a, qhi_a) between two neighbouring values of { box lo_a, top_a = min(box hi_a, the cell's forward exit
// plane exit_up[a]), every axis-plane coordinate q of class a in any chunk } that contains the box centre.  So every axis plane of the set, the box's
// faces and the cell's exit planes lie at or outside the gap's ends.
//
// The kernel's test (direct_all, per live lane; o, d, maxt the shadow ray's):
//     hi+   = max(maxt * (1 + 2^-20), 2^-100)                       the sweep's own widened window end (pt_trace.hpp trace_cell1)
//     end_a = fma(hi+, d_a, o_a)
//     m_a   = fma(Gm_a, |o|_1, Hm_a)
//     pass  = for all a:  min(o_a, end_a) - qlo_a > m_a  and  qhi_a - max(o_a, end_a) > m_a          (a NaN anywhere: no pass)
// and when every live lane of the wave passes, the wave enters the candidate loops with cmin = 0, cmax = maxt and steps past the axis entries.
//
// Why nothing changes (u = 2^-24; Q_a = max(|qlo_a|, |qhi_a|); mu_a = the largest sweep margin M / |n_a| of an axis entry on a, M = G |o|_1 + H
// with the chunk's largest G and H, exactly what the sweep itself allows that entry):
//   * what the test establishes.  A passing end_a lies inside the gap, so |end_a| <= Q_a and the exact end o_a + hi+ d_a is within u Q_a of it; the
//     difference and m_a carry one rounding each and |o|_1 two.  With Gm_a = 17/16 mu's G (1 + 2^-19) and Hm_a = (17/16 mu's H + 2^-23 Q_a)(1 + 2^-19),
//     rounded up:
//         exact end - qlo_a  >=  fl(end_a - qlo_a)(1 - u) - u Q_a  >  m_a (1 - u) - u Q_a  >=  (Gm_a |o|_1 + Hm_a)(1 - u)^4 - u Q_a  >=  17/16 mu_a
//     and the same at qhi_a and for the origin (which has no rounding of its own).  In words: both ends of the segment [0, hi+] lie inside the gap,
//     farther than 17/16 mu_a from either end of it, in exact arithmetic.
//   * the sixteenth.  The sweep evaluates its two inequalities in fp32: sn = fl(n_a fl(o_a - q)), div = fl(n_a d_a), one sum and one fused operation,
//     each rounding relative to at most |n_a| (|o_a| + |q|) <= E (|o|_1 + |p0|_1) = M / 128 u -- together under 6 u of that, M / 21.  A segment
//     farther than 17/16 M / |n_a| from the plane in exact arithmetic is therefore dropped by the sweep AS COMPUTED: the early-out skips exactly
//     verdicts that say "drop" (tests/shadow_gap_check.c counts the ones that would not).
//   * box.  lo_a <= qlo_a < o_a < qhi_a <= hi_a: the near numerators lo - o (d > 0) or hi - o (d < 0) are non-zero with the sign opposite to d, every
//     near quotient is negative or a zero, tmin = max(.., 0) = 0 under either division contract.  The exact end lies below top_a <= hi_a, exit_up[a]
//     and above lo_a: hi+ |d_a| < the exact far numerator, whose rounding and the quotient's (<= 2.5 ulp under the default contract) are covered by
//     the 2^-20 = 16 u in hi+: every far and exit quotient is >= maxt, so v holds, cmax >= maxt, and "t <= cmax and t < maxt" is "t <= maxt and t < maxt".
//   * axis planes.  A triangle in the plane {x_a = q}, q <= qlo_a, with normal n_a e_a: the reference's div = fl(n_a d_a) is <= 0 (reject, code.cl:259)
//     or the ray faces it.  Facing it from above with d_a > 0: the reference's numerator N of t is within delta = 14 u E (|o|_1 + |p0|_1) of
//     n_a (o_a - q) >= M = 128 u E (..) (pt_trace.hpp's term-by-term bound), so N > 0 and t = N * -(1 / div) < 0 = cmin: rejected.  With d_a < 0:
//     |n_a| (o_a - q) - hi+ |n_a d_a| = |n_a| (exact end - q) > M, so -N > hi+ div and t > maxt: no hit.  The planes at or above qhi_a mirror this.
//     These are the two inequalities the sweep's verdict evaluates (pt_trace.hpp PLANE WINDOW), taken at the innermost plane of each side; a plane
//     farther out only adds to the left-hand sides.  Both windings are covered: the argument never used the sign of n_a but through div > 0.
// tests/test_shadow_gap.py checks the claim on the CPU against the reference's box and triangle tests (tests/shadow_gap_check.c).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
namespace pt {
#endif

enum { kGapMaxPlanes = 96 };   /* kLdsTriMax: no list holds more records, so no axis more planes */

/* the axis planes of one plane list: per axis the coordinates, and the largest G / |n_a| and H / |n_a| over its entries (G, H: the entry's chunk's) */
typedef struct GapPlanes {
    uint32_t n[3];
    float q[3][kGapMaxPlanes];
    double g[3], h[3];
} GapPlanes;

/* what the kernel reads: GridArgs::gap = {qlo[3], qhi[3], Gm[3], Hm[3]}, GridArgs::gap_ok = ok */
typedef struct ShadowGap {
    float qlo[3], qhi[3], gm[3], hm[3];
    uint32_t ok;
} ShadowGap;

static inline float gap_word_float(uint32_t w) { float f; memcpy(&f, &w, 4); return f; }

/* words: the host's copy of a plane list of `count` records (header and groups), n_words of them.  Returns 0 when the list does not parse inside
   n_words (the caller then offers no gap). */
static inline int gap_planes_from_list(const uint32_t* words, uint32_t n_words, uint32_t count, GapPlanes* out) {
    memset(out, 0, sizeof *out);
    if (n_words < 16u || count == 0u || count > (uint32_t)kGapMaxPlanes) return 0;
    for (uint32_t c = 0; c < (count + 31u) / 32u; ++c) {
        const uint32_t groups = words[c], first = words[4u + c];
        const float G = gap_word_float(words[8u + c]), H = gap_word_float(words[12u + c]);
        uint32_t g = 16u + 16u * first;
        for (uint32_t cl = 0; cl < 3u; ++cl) {
            for (uint32_t i = 0; i < ((groups >> (8u * cl)) & 255u); ++i, g += 16u) {
                if (g + 16u > n_words) return 0;
                for (uint32_t k = 0; k < 4u; ++k) {
                    const uint32_t* e = words + g + 4u * k;
                    if ((e[2] | e[3]) == 0u) continue;   /* a padding entry */
                    const float na = fabsf(gap_word_float(e[1]));
                    if (out->n[cl] >= (uint32_t)kGapMaxPlanes || !(na > 0.0f)) return 0;
                    out->q[cl][out->n[cl]++] = gap_word_float(e[0]);
                    out->g[cl] = fmax(out->g[cl], (double)G / (double)na);
                    out->h[cl] = fmax(out->h[cl], (double)H / (double)na);
                }
            }
        }
    }
    return 1;
}

static inline float gap_round_up(double v) {   /* the smallest float >= v (v finite, >= 0) */
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}

/* b8: the set's bounds (min, 1, max, 1); exit_up: the single cell's forward exit planes (pt_set_guard.hpp SetGuard::exit_up).  scale: 1 in the
   product; the CPU check cuts the margins with it to show that it can tell a margin that is too small. */
static inline ShadowGap shadow_gap(const float* b8, const float* exit_up, const GapPlanes* P, double scale) {
    ShadowGap s;
    memset(&s, 0, sizeof s);
    int ok = 1;
    for (int a = 0; a < 3; ++a) {
        const float lo = b8[a], top = fminf(b8[4 + a], exit_up[a]);
        const float c = 0.5f * lo + 0.5f * b8[4 + a];
        float qlo = lo, qhi = top;   /* the neighbours of the centre among lo, top and the planes: the largest value <= c, the smallest > c */
        for (uint32_t i = 0; i < P->n[a]; ++i) {
            const float q = P->q[a][i];
            if (q <= c && q > qlo) qlo = q;
            if (q > c && q < qhi) qhi = q;
        }
        ok = ok && lo <= c && c < top && qlo < qhi && b8[4 + a] >= top && exit_up[a] >= top;   /* (a NaN fails) */
        const double Q = fmax(fabs((double)qlo), fabs((double)qhi));
        s.qlo[a] = qlo;
        s.qhi[a] = qhi;
        s.gm[a] = gap_round_up(P->g[a] * 1.0625 * 1.0000019073486328125 * scale);
        s.hm[a] = gap_round_up((P->h[a] * 1.0625 + 0x1p-23 * Q) * 1.0000019073486328125 * scale);
        /* every constant finite, the margin positive and normal (no product below can be flushed), the gap wider than twice its smallest margin */
        ok = ok && isfinite(s.qlo[a]) && isfinite(s.qhi[a]) && isfinite(s.gm[a]) && isfinite(s.hm[a]) && s.hm[a] >= 0x1p-120f &&
             (double)qhi - (double)qlo > 2.0 * (double)s.hm[a];
    }
    s.ok = ok ? 1u : 0u;
    return s;
}

#ifdef __cplusplus
}  // namespace pt
#endif
