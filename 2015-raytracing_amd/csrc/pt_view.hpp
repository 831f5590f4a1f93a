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
#include <type_traits>

namespace pt {

// d.c = (right.c * lx + up.c * ly) + forward.c * lz: the local direction (lx, ly, lz) in the caller's basis, used as given
PT_DEV f3 view_dir(const float* right, const float* up, const float* forward, float lx, float ly, float lz) {
    return mk3((right[0] * lx + up[0] * ly) + forward[0] * lz, (right[1] * lx + up[1] * ly) + forward[1] * lz, (right[2] * lx + up[2] * ly) + forward[2] * lz);
}

// tile-local ray id -> the sample's ray.  id = ((y - row0) * width + x) * rpp + i, i = sy * k + sx; positions use the global y.
// (V is a kernel argument: the model's branch, the shifts and the masks are wave-uniform.)
// BATCH (mirt_view_rays_batch, mirt_render_view_batch): the tile is V.nrows / V.frame_rows frames stacked, row0 = 0.  The tile-local row gives
// the frame f = row div frame_rows and the frame's own y = row - f * frame_rows, and the camera is the table's entry f, loaded PER LANE: a wave
// may hold lanes of several frames (64 of them at 1 x 1, k = 1).  Everything from fx on is the one code; the default keeps the single
// instances' code, which read the camera from the kernel arguments.
template <bool BATCH>
using ViewArgsOf = typename std::conditional<BATCH, ViewBatchArgs, ViewArgs>::type;
template <bool BATCH = false>
PT_DEV Ray view_ray(const ViewArgsOf<BATCH>& V, uint32_t id) {
    const uint32_t lk = (uint32_t)__builtin_ctz(V.k);   // k is 1, 2, 4, 8 or 16
    const uint32_t pix = id >> (2u * lk), i = id & ((1u << (2u * lk)) - 1u);
    const uint32_t sy = i >> lk, sx = i & (V.k - 1u);
    const uint32_t lrow = pix / V.width;
    const uint32_t x = pix - lrow * V.width;
    uint32_t y;
    float cam[12];
    const float *eye = V.eye, *right = V.right, *up = V.up, *forward = V.forward;
    if constexpr (BATCH) {
        const uint32_t f = lrow / V.frame_rows;
        y = lrow - f * V.frame_rows;
        const float4* c = (const float4*)(V.cameras + (size_t)f * 12u);   // 48 bytes an entry: three aligned 16-byte loads
        const float4 c0 = c[0], c1 = c[1], c2 = c[2];
        cam[0] = c0.x; cam[1] = c0.y; cam[2] = c0.z; cam[3] = c0.w; cam[4] = c1.x; cam[5] = c1.y; cam[6] = c1.z; cam[7] = c1.w;
        cam[8] = c2.x; cam[9] = c2.y; cam[10] = c2.z; cam[11] = c2.w;
        eye = cam; right = cam + 3; up = cam + 6; forward = cam + 9;
    } else {
        y = V.row0 + lrow;
    }
    const float ik = __uint_as_float((127u - lk) << 23);   // 1 / k
    const float fx = (float)x + ((float)sx + 0.5f) * ik, fy = (float)y + ((float)sy + 0.5f) * ik;
    const float u = div_cr(fx, (float)V.width), v = div_cr(fy, (float)V.height);
    const float a = (u + u) - 1.0f, b = 1.0f - (v + v);   // row 0 is the top
    Ray r;
    r.o = ld3(eye);
    r.mint = V.t_min;
    r.maxt = V.t_max;
    if (V.model == 0u) {   // MIRT_VIEW_ORTHOGRAPHIC
        const float ta = a * V.half_w, tb = b * V.half_h;
        r.o = mk3((eye[0] + right[0] * ta) + up[0] * tb, (eye[1] + right[1] * ta) + up[1] * tb, (eye[2] + right[2] * ta) + up[2] * tb);
        r.d = ld3(forward);
    } else if (V.model == 1u) {   // MIRT_VIEW_EQUIRECT
        const float phi = a * 0x1.921fb6p+1f, th = b * 0x1.921fb6p+0f;
        float sp, cp, st, ct;
        cl_sincos(phi, sp, cp);
        cl_sincos(th, st, ct);
        r.d = view_dir(right, up, forward, sp * ct, st, cp * ct);
    } else {   // MIRT_VIEW_FISHEYE
        const float rad = sqrt_cr(a * a + b * b);
        if (!(rad <= 1.0f)) {   // outside the circle: a DEAD sample
            r.d = ld3(forward);
            r.mint = 0.0f;
            r.maxt = 0.0f;
        } else {
            const float ang = rad * V.half_angle;
            float sa, ca;
            cl_sincos(ang, sa, ca);
            const float q = rad > 0.0f ? div_cr(sa, rad) : 0.0f;
            r.d = view_dir(right, up, forward, a * q, b * q, ca);
        }
    }
    return r;
}

}  // namespace pt
