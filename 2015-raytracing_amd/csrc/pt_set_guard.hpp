// pt_set_guard.hpp -- the geometry side of "may this launch be optimistic": what the host works out once per primitive set from its bounds and
// slab count, before launch, because no lane can catch it (a ray outside the windows defers itself in the kernel; a SET outside them would be wrong
// for every ray).  The result is copied into GridArgs (pt_launch.hpp: fast_ok, walk_ok, exit_is_far_face, exit_far_axes, exit_up, exit_above_axes, delta, rdelta).
// Plain fp32 arithmetic on eight floats -- no HIP header, no context and no buffer, so a plain C++ compiler builds it and tests/test_set_guard.py
// checks it on the CPU (tests/set_guard_dump.cpp) against the same rules in numpy.float32.  mirt_abi.cpp is the caller (fill_grid; launch_kernel's
// single-cell launches for set_exit_is_far_face alone).
//
// Every quotient and sum below is the reference's own fp32 operation, correctly rounded.  A compiler that contracts a*b + c changes nothing here:
// the only products are 1*x and 0*x, which are exact, so the fused and the unfused sum round the same value.
#pragma once
#include <stdint.h>
#include <math.h>
#include "pt_windows.hpp"

namespace pt {

inline bool guard_within(float v, float lo, float hi) { const float a = fabsf(v); return a >= lo && a <= hi; }   // a NaN fails
inline bool guard_zero_or_within(float v, float lo, float hi) { return v == 0.0f || guard_within(v, lo, hi); }

// The two exit planes of the single cell of an n == 1 set, as the reference forms them (A10 code.cl:699-707):
// x_next = lo + (0 + (d >= 0)) * ((hi - lo) / 1), i.e. forward up = lo + 1*delta, backward dn = lo + 0*delta.
struct ExitPlanes {
    float up[3];             // the forward plane per axis
    uint32_t up_is_hi;       // bit k: up[k] == hi (a NaN plane equals nothing)
    bool dn_is_lo;           // on all three axes the backward plane equals lo (a zero of either sign; false when 0*delta is a NaN)
};
inline ExitPlanes exit_planes(const float* b8) {
    ExitPlanes p = {{0.0f, 0.0f, 0.0f}, 0u, true};
    for (int k = 0; k < 3; ++k) {
        const float lo = b8[k], hi = b8[4 + k];
        const float delta = (hi - lo) / 1.0f;
        const float dn = lo + 0.0f * delta;
        p.up[k] = lo + 1.0f * delta;
        if (p.up[k] == hi) p.up_is_hi |= 1u << k;
        p.dn_is_lo = p.dn_is_lo && dn == lo;
    }
    return p;
}
inline bool planes_are_far_face(const ExitPlanes& p) { return p.up_is_hi == 7u && p.dn_is_lo; }

// n == 1 only: both exit planes reproduce the box's faces on all three axes, so the single cell's exit t is the very quotient the box test
// already formed for the far slab plane (pt_trace.hpp cell1_exit, every kernel that walks a single cell).
inline uint32_t set_exit_is_far_face(const float* b8, uint32_t n) { return n == 1u && planes_are_far_face(exit_planes(b8)) ? 1u : 0u; }

struct SetGuard {
    uint32_t fast_ok;            // the optimistic kernel may run this set; 0 sends the whole launch to the exact kernel
    uint32_t walk_ok;            // n > 1: delta / rdelta sit inside the windows of the walk's 3-operation divisions; 0: a lane that walks the set defers
    uint32_t exit_is_far_face;   // set_exit_is_far_face
    uint32_t exit_far_axes;      // n == 1: bit k where the forward exit plane is hi (7 otherwise)
    float exit_up[3];            // n == 1: the forward exit plane per axis (hi otherwise)
    uint32_t exit_above_axes;    // n == 1: bit k where the forward exit plane lies ABOVE hi (0 otherwise).  There the one slab pass of the optimistic kernel
                                 // (pt_trace.hpp box_exit1) asks the box's far face as well when a lane's window is shorter than a constant made from
                                 // exit_up and the bounds: pt_box_exit.hpp box_exit_consts, a header of its own in the common subset of C and C++ (its CPU
                                 // check is a C program), which the caller of set_guard includes
    float delta[3], rdelta[3];   // the slab width (hi - lo) / n and its reciprocal
};

// b8: the set's bounds (min, 1, max, 1).  n: slabs per axis, 1..1024 (check_grid).  records_sane: what k_prepTriangles found (true for spheres).
inline SetGuard set_guard(const float* b8, uint32_t n, bool records_sane) {
    SetGuard g = {};
    // fast_ok: every bound is a position inside its window ...
    bool fast = records_sane;
    for (int k = 0; k < 8; ++k)
        if ((k & 3) != 3) fast = fast && guard_zero_or_within(b8[k], kPosLo, kPosHi);
    // ... the optimistic kernel's box test takes min / max of the two plane quotients as near / far: that needs lo <= hi on every axis
    // (an inverted box is a miss in the reference; here it goes to the exact kernel; a NaN fails) ...
    for (int k = 0; k < 3; ++k) fast = fast && b8[k] <= b8[4 + k];
    g.exit_far_axes = 7u;
    for (int k = 0; k < 3; ++k) g.exit_up[k] = b8[4 + k];
    if (n == 1u) {
        // ... and a single cell's forward exit planes are positions like the bounds, its backward planes are lo: the kernel subtracts the ray's
        // origin from the first and takes the box's far quotient for the second (pt_trace.hpp cell1_exit)
        const ExitPlanes p = exit_planes(b8);
        for (int k = 0; k < 3; ++k) {
            g.exit_up[k] = p.up[k];
            fast = fast && guard_zero_or_within(p.up[k], kPosLo, kPosHi);
        }
        fast = fast && p.dn_is_lo;
        g.exit_far_axes = p.up_is_hi;
        g.exit_is_far_face = planes_are_far_face(p) ? 1u : 0u;
        for (int k = 0; k < 3; ++k)
            if (p.up[k] > b8[4 + k]) g.exit_above_axes |= 1u << k;
    }
    g.fast_ok = fast ? 1u : 0u;
    // the walk's wave-uniform quotients, once, in the arithmetic the kernel would use: fp32, correctly rounded.  The span is a numerator of the
    // walk (pt_trace.hpp num_window), the width a denominator (den_window).
    bool walk = true;
    for (int k = 0; k < 3; ++k) {
        const float span = b8[4 + k] - b8[k];
        g.delta[k] = span / (float)n;
        g.rdelta[k] = 1.0f / g.delta[k];
        walk = walk && guard_zero_or_within(span, kNumLo, kNumHi) && guard_within(g.delta[k], kDenLo, kDenHi);
    }
    g.walk_ok = walk ? 1u : 0u;
    return g;
}

}  // namespace pt
