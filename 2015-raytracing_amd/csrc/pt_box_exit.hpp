// pt_box_exit.hpp -- ONE SLAB PASS for a single-cell set whose exit planes are not the box's far faces: what the host works out once per set so
// that the optimistic kernels (pt_trace.hpp box_exit1, called by closest_all, direct_all and rays_any) take the box verdict and the cell's exit t
// from six quotients instead of nine.  Plain C arithmetic on the set's bounds and exit planes -- no HIP header, no context and no buffer; written in
// the common subset of C and C++ so that tests/box_exit_check.c includes this very file.  mirt_abi.cpp is the caller (fill_grid, with the exit planes
// pt_set_guard.hpp made) and copies gap_max into GridArgs::exit_gap_max; GridArgs::exit_above_axes is pt_set_guard.hpp's own.
//
// The two functions this replaces for such a set (pt_trace.hpp inter_aabb_t<FAST, false> and cell1_exit<FAST>), per axis k, every quotient the
// correctly rounded one (div_exact3_anyzero on the ray's refined reciprocal, inside the guard windows):
//     q_lo = (lo - o) / d,  q_hi = (hi - o) / d,  q_up = (up - o) / d          up = lo + 1*((hi - lo)/1), the reference's forward exit plane
//     tmin = max(0, max_k min(q_lo, q_hi)),  tmax = min_k max(q_lo, q_hi),  v = !(tmin > tmax)
//     exit = min_k (d >= 0 ? q_up : q_lo)                                        (the backward exit plane is lo: host-checked, set_guard)
// and the set's primitives are asked for t with tmin <= t <= exit when v holds.
//
// The one pass, per axis k:
//     near_k = ((d >= 0 ? lo : hi) - o) / d,  far_k = ((d >= 0 ? up : lo) - o) / d        -- the numerators selected, two quotients
//     tmin = max(0, max_k near_k),  cmax = min_k far_k,  v' = !(tmin > cmax)
// Same bits (the sign of a zero aside, which comparisons cannot see -- pt_trace.hpp slab1_fast): near_k is the reference's own choice (code.cl's
// d < 0 ? t1 : t0), which the box test takes as min(q_lo, q_hi) because rounding to nearest and the division by one d are monotonic and lo <= hi
// (part of fast_ok); far_k is cell1_exit's choice, whose far slab quotient max(q_lo, q_hi) is q_lo for d < 0.  Hence tmin is the box test's tmin and
// cmax is cell1_exit's exit.
//
// The verdict v' = (tmin <= cmax) against the reference's v = (tmin <= tmax), u = 2^-24:
//   * an axis with up <= hi, or with d < 0: far_k <= max(q_lo, q_hi) (monotonic again, or the same quotient), so tmin <= far_k gives tmin <= the
//     box's far quotient of that axis.
//   * an axis with up > hi (GridArgs::exit_above_axes) and d > 0.  eps = up - hi > 0, T = (up - o) / d and E = eps / d in exact arithmetic.  far_k
//     carries the rounding of its numerator and of the quotient: far_k <= T (1 + u)^2 when T >= 0, and the box's q_hi >= T (1 - u)^2 - E (1 + u)^2
//     whichever sign T - E has:
//         q_hi  >=  far_k (1 - u)^2 / (1 + u)^2 - E (1 + u)^2  >=  far_k (1 - 4u) - E (1 + 3u)                                            (1)
//     (T < 0 makes far_k and cmax <= 0: then v' needs tmin = cmax = 0, room is a zero and the lane is close below, the gaps being positive.)
//   So: v false and v' true needs an axis of the second kind, and v true with v' false means tmin > exit -- the reference's window is empty and it
//   finds nothing, which is what not asking finds.  Where v may be false and v' true the lane takes the BOX's comparison.  The kernel's test,
//   compiled in only for a set with exit_above_axes != 0, in two steps.  With c = 1 - 2^-20 = 1 - 16u, r_k the ray's refined reciprocal of d_k
//   (RayRcp: |r_k| >= (1 - 2u) / |d_k|) and exit_gap_max = the largest eps (1 + 2^-20), rounded up:
//     every lane:   room = fma(cmax, c, -tmin),  close = v' and not room >= fl(exit_gap_max * max_k |r_k|)
//     a wave with a close lane:   tmax = min(cmax, q_hi on the axes of exit_above_axes with d >= 0),  v' = !(tmin > tmax)
//   The product rounds once: fl(exit_gap_max max|r|) >= E (1 + 16u)(1 - 2u)(1 - u) >= E (1 + 12u) for the E of every axis.  A lane that is not close:
//   room >= that product > 0, room <= (cmax c - tmin)(1 + u), so on every axis of the second kind
//         tmin  <=  cmax (1 - 16u) - E (1 + 12u) / (1 + u)  <=  far_k (1 - 4u) - E (1 + 3u)  <=  q_hi                                     by (1),
//   and tmin <= far_k <= the box's far quotient on the others: tmin <= tmax, v holds as v' does.  In a wave with a close lane every lane compares
//   tmin with the smaller of cmax and the q_hi of those axes -- the quotients the box test forms there, by the same three operations.  v' true then
//   says tmin <= every far quotient of the box (the others are no smaller than far_k >= cmax): v.  v' false says tmin > cmax, an empty window, or
//   tmin > some q_hi: not v.  The lanes that were not close keep the verdict they had (just shown).  Nothing underflows: eps >= 2^-54 (an ulp of a
//   bound of at least 2^-30), |d| in [2^-40, 2^40].  No lane defers on account of this pass.
//   * how often the second step runs: when some lane's whole window [tmin, cmax] is shorter than 2^-20 cmax plus the largest gap over the smallest
//     |d_k| -- a ray that grazes an edge of the cell, or runs nearly parallel to an axis.  tests/box_exit_check.c counts the close lanes.
// tests/test_box_exit.py checks all of this on the CPU (tests/box_exit_check.c) against the two-function form.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __cplusplus
namespace pt {
#endif

/* what the kernel reads: GridArgs::exit_gap_max = gap_max (GridArgs::exit_above_axes is pt_set_guard.hpp's and equals `above`) */
typedef struct BoxExit {
    uint32_t above;   /* bit k: up[k] > hi[k] */
    float gap[3];     /* (up[k] - hi[k]) (1 + 2^-20), rounded up, on the axes of `above`; 0 elsewhere */
    float gap_max;    /* the largest of the three */
} BoxExit;

/* b8: the set's bounds (min, 1, max, 1); up: its forward exit planes (pt_set_guard.hpp exit_planes) */
static inline BoxExit box_exit_consts(const float* b8, const float* up) {
    BoxExit e;
    int k;
    e.above = 0u;
    e.gap_max = 0.0f;
    for (k = 0; k < 3; ++k) {
        e.gap[k] = 0.0f;
        if (up[k] > b8[4 + k]) {   /* (a NaN plane is above nothing; such a set is not fast_ok) */
            const double eps = ((double)up[k] - (double)b8[4 + k]) * (1.0 + 0x1p-20);   /* exact difference, one rounding of the product */
            float g = (float)eps;
            if ((double)g < eps) g = nextafterf(g, INFINITY);
            e.gap[k] = g;
            if (g > e.gap_max) e.gap_max = g;
            e.above |= 1u << k;
        }
    }
    return e;
}

#ifdef __cplusplus
}  // namespace pt
#endif
