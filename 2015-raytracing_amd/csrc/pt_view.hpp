// pt_view.hpp -- the ray of one sample of a panoramic, fisheye or orthographic camera: the ONE device definition, used by k_viewRays (the rays
// as records) and k_viewPass (the rays in registers) of pt_kernels_rays.hip.  The definition is include/mirt.h's (mirt_view_rays), restated in
// numpy by tests/view_common.py; the kernels equal that restatement bit for bit, in both libraries.
//
// Numerics.  One fp32 operation at a time, rounded on its own, in the order the header writes them: every translation unit builds with
// -ffp-contract=off, and nothing here is an fma except inside cl_sincos.  The reference has no such camera, so there is ONE contract for
// libmirt.so and libmirt_default.so: every quotient is div_cr() and the one root sqrt_cr() (pt_post.hpp), sin and cos are cl_sincos
// (pt_numerics.hpp).  1 / k is a power of two and is built from its exponent, so (sx + 0.5) / k and the sum with x are exact.
#pragma once
#include "pt_device.hpp"
#include "pt_launch.hpp"
#include "pt_post.hpp"

namespace pt {

// d.c = (right.c * lx + up.c * ly) + forward.c * lz: the local direction (lx, ly, lz) in the caller's basis, used as given
PT_DEV f3 view_dir(const ViewArgs& V, float lx, float ly, float lz) {
    return mk3((V.right[0] * lx + V.up[0] * ly) + V.forward[0] * lz, (V.right[1] * lx + V.up[1] * ly) + V.forward[1] * lz,
               (V.right[2] * lx + V.up[2] * ly) + V.forward[2] * lz);
}

// tile-local ray id -> the sample's ray.  id = ((y - row0) * width + x) * rpp + i, i = sy * k + sx; positions use the global y.
// (V is a kernel argument: the model's branch, the shifts and the masks are wave-uniform.)
PT_DEV Ray view_ray(const ViewArgs& V, uint32_t id) {
    const uint32_t lk = (uint32_t)__builtin_ctz(V.k);   // k is 1, 2, 4, 8 or 16
    const uint32_t pix = id >> (2u * lk), i = id & ((1u << (2u * lk)) - 1u);
    const uint32_t sy = i >> lk, sx = i & (V.k - 1u);
    const uint32_t lrow = pix / V.width;
    const uint32_t x = pix - lrow * V.width, y = V.row0 + lrow;
    const float ik = __uint_as_float((127u - lk) << 23);   // 1 / k
    const float fx = (float)x + ((float)sx + 0.5f) * ik, fy = (float)y + ((float)sy + 0.5f) * ik;
    const float u = div_cr(fx, (float)V.width), v = div_cr(fy, (float)V.height);
    const float a = (u + u) - 1.0f, b = 1.0f - (v + v);   // row 0 is the top
    Ray r;
    r.o = ld3(V.eye);
    r.mint = V.t_min;
    r.maxt = V.t_max;
    if (V.model == 0u) {   // MIRT_VIEW_ORTHOGRAPHIC
        const float ta = a * V.half_w, tb = b * V.half_h;
        r.o = mk3((V.eye[0] + V.right[0] * ta) + V.up[0] * tb, (V.eye[1] + V.right[1] * ta) + V.up[1] * tb, (V.eye[2] + V.right[2] * ta) + V.up[2] * tb);
        r.d = ld3(V.forward);
    } else if (V.model == 1u) {   // MIRT_VIEW_EQUIRECT
        const float phi = a * 0x1.921fb6p+1f, th = b * 0x1.921fb6p+0f;
        float sp, cp, st, ct;
        cl_sincos(phi, sp, cp);
        cl_sincos(th, st, ct);
        r.d = view_dir(V, sp * ct, st, cp * ct);
    } else {   // MIRT_VIEW_FISHEYE
        const float rad = sqrt_cr(a * a + b * b);
        if (!(rad <= 1.0f)) {   // outside the circle: a DEAD sample
            r.d = ld3(V.forward);
            r.mint = 0.0f;
            r.maxt = 0.0f;
        } else {
            const float ang = rad * V.half_angle;
            float sa, ca;
            cl_sincos(ang, sa, ca);
            const float q = rad > 0.0f ? div_cr(sa, rad) : 0.0f;
            r.d = view_dir(V, a * q, b * q, ca);
        }
    }
    return r;
}

}  // namespace pt
