"""Shared by tests/test_guides.py and tests/guides_default_child.py: what mirt_render_guides is checked against.

The guides are defined on the state initTrace and the closest-hit stage leave (include/mirt.h): this module drives those kernels of a checker
(oracle/liboracle.so, or the reference binary on the device through oracle/ref_gpu.py) the way oracle/a10_pass.py::run_pass does up to its
closest(), and reduces Ray.maxt, Poi.normal and Poi.matId per pixel in sample order with one np.float32 addition at a time."""
import numpy as np

import a10_pass as A


def first_hit_state(k, sc, rows=None):
    """initTrace, then sphereTrace, triangleTrace and every meshTrace in upload order (run_pass up to closest()): returns the PassState"""
    h = sc.height if rows is None else rows
    n = sc.width * h * sc.rpp
    g1 = A._ceil(n, A.WAVE)
    st = A.PassState(sc, A.make_seeds(sc.total_rays))
    B = k.buf
    bp, _b = A._f(sc.bounds)
    cp, _c = A._f(sc.cam)
    k.initTrace(B(st.seeds), B(st.rays), B(st.pois), bp, cp, sc.focal_length, sc.lens_rad, sc.rpp, A._ceil(sc.width, 8), A._ceil(h, 8))
    if sc.has_spheres:
        p, _k = A._f(sc.sphere_bounds)
        k.sphereTrace(n, B(st.pois), B(st.rays), B(sc.spheres), B(sc.s_matid), B(sc.s_box), p, sc.n_slabs, g1)
    if sc.has_triangles:
        p, _k = A._f(sc.triangle_bounds)
        k.triangleTrace(n, B(st.pois), B(st.rays), B(sc.t_pos), B(sc.t_normal), B(sc.t_matid), B(sc.t_box), p, sc.n_slabs, g1)
    for m in sc.meshes:
        p, _k = A._f(m["bounds"])
        k.meshTrace(n, B(st.pois), B(st.rays), B(m["pos"]), B(m["normal"]), B(m["box"]), m["matid"], p, m["nslabs"], g1)
    k.flush()
    return st


def reduce_guides(maxt, normal, mat_id, materials, rpp):
    """(normal_hits, albedo_depth), float32 [pixels, 4]: sequential fp32 sums from +0 over the hit samples of each pixel, in sample order.
    A hit: 0 <= matId < number of materials."""
    mats = np.asarray(materials, np.float32).reshape(-1, 4)
    maxt = np.asarray(maxt, np.float32).reshape(-1, rpp)
    normal = np.asarray(normal, np.float32).reshape(-1, rpp, 3)
    mat_id = np.asarray(mat_id, np.int32).reshape(-1, rpp)
    npix = maxt.shape[0]
    nh = np.zeros((npix, 4), np.float32)
    ad = np.zeros((npix, 4), np.float32)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        for i in range(rpp):
            hit = (mat_id[:, i] >= 0) & (mat_id[:, i] < mats.shape[0])
            col = mats[np.where(hit, mat_id[:, i], 0)]
            add_n = np.concatenate([normal[:, i, :], np.full((npix, 1), one, np.float32)], axis=1)
            add_a = np.concatenate([col[:, :3], maxt[:, i:i + 1]], axis=1)
            nh[hit] = (nh[hit] + add_n[hit]).astype(np.float32)
            ad[hit] = (ad[hit] + add_a[hit]).astype(np.float32)
    return nh, ad


def expected_guides(k, sc, rows=None):
    st = first_hit_state(k, sc, rows)
    n = sc.width * (sc.height if rows is None else rows) * sc.rpp
    return reduce_guides(st.rays["maxt"][:n], st.pois["normal"][:n], st.pois["matId"][:n], sc.materials, sc.rpp)


def difference(tag, got, want):
    """None when equal bit for bit (every NaN equal to every NaN), else a sentence naming the first difference"""
    g = np.ascontiguousarray(got, np.float32).reshape(-1).view(np.uint32).copy()
    w = np.ascontiguousarray(want, np.float32).reshape(-1).view(np.uint32).copy()
    if g.size != w.size:
        return f"{tag}: {g.size} words against {w.size}"
    for u in (g, w):
        u[(u & 0x7FFFFFFF) > 0x7F800000] = 0x7FC00000
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return None
    i = int(bad[0])
    return f"{tag}: {bad.size} of {g.size} words differ; first at pixel {i // 4} channel {i % 4}: got 0x{int(g[i]):08x}, want 0x{int(w[i]):08x}"
