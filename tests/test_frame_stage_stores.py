"""GPU: what an Assign04 / Assign07 trace stage stores, on both frame paths (pt_kernels_frame.hip: the kernel-by-kernel kernels and k_frame_fused run
the same stage).  A hit writes the ray's maxt -- 4 bytes -- and the pixel; a hit on an Assign04 triangle whose mindex names no colour writes maxt and
leaves the pixel; a miss, and a work-item outside the NDRange, write nothing."""
import numpy as np
import pytest

from conftest import bits
import a10_pass as A
from test_frames import fixture
from test_frame_one_launch import SENTINEL, packed, rays40

BLACK = np.array([0, 0, 0, 255], np.uint8)


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 2], ids=["every triangle", "every other triangle"])
def test_a_mindex_out_of_range_keeps_maxt_and_leaves_the_pixel(ctx, every):
    from raytracing_amd.pyhost import render
    fx, d = fixture("frame_a04_own_icosphere_96x64")   # the unmodified job: its pixels and maxt are the fixture's (test_frames.py)
    ncolors = len(d["mcolor"]) // 4
    mindex = np.asarray(d["mindex"], np.uint32).copy()
    assert (mindex < ncolors).all()
    mindex[::every] = ncolors                           # the first index out of range ...
    mindex[::2 * every] = 0xFFFFFFFF                     # ... and the last
    p = packed(dict(d, mindex=mindex.tolist()))
    px, rays = render.render_frame_stream(ctx, p, rays_fill=0)
    px1, rays1 = render.render_frame_one_launch(ctx, p, keep_rays=True)
    assert np.array_equal(px1, px) and np.array_equal(rays40(rays1)[0], rays40(rays)[0])
    assert np.array_equal(bits(rays.view(A.RAY_DT)["maxt"]), bits(fx["rays_maxt"]))
    black = (px == BLACK).all(axis=1)
    kept = (px == fx["pixel"]).all(axis=1)
    if every == 1:
        assert black.all()
    else:
        assert (black | kept).all() and (black & ~kept).any() and (kept & ~black).any()


def enqueue_stream(ctx, p, gws):
    """initTrace and the job's trace kernel, each over the NDRange gws, on pixel and ray buffers filled with SENTINEL.  Returns (pixels [H, W, 4],
    rays [H, W, 48]) as bytes."""
    u32 = lambda v: np.array([v], np.uint32)   # noqa: E731
    w, h = p.width, p.height
    pixels, rays = ctx.buffer(w * h * 4), ctx.buffer(w * h * 48)
    for b in (pixels, rays):
        b.write(np.full(b.nbytes, SENTINEL, np.uint8))
    if p.mol:
        geo = [ctx.buffer_from(a) for a in (p.atoms, p.mindex, p.mcolor, p.slab_size)]
        tr = ctx.kernel("A07:molTrace").set_args(pixels, p.cam, rays, u32(p.s_size), geo[0], geo[1], geo[2], p.bounds, u32(p.n_slabs), geo[3])
    else:
        geo = [ctx.buffer_from(a) for a in (p.pos, p.normal, p.mindex, p.mcolor, p.slab_size)]
        tr = ctx.kernel("A07:meshTrace").set_args(pixels, p.cam, rays, u32(p.t_size), geo[0], geo[1], geo[2], geo[3], p.bounds, u32(p.n_slabs), geo[4])
    it = ctx.kernel("A07:initTrace").set_args(pixels, p.cam, rays, p.bounds)
    it.enqueue(gws, [8, 8])
    tr.enqueue(gws, [8, 8])
    ctx.finish()
    out = pixels.read(np.uint8).reshape(h, w, 4), rays.read(np.uint8).reshape(h, w, 48)
    for k in (it, tr):
        k.release()
    for b in [pixels, rays] + geo:
        b.release()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["frame_a07_own_terrain_n5_96x64", "frame_a07_own_mol_lattice_n6_96x64"])
def test_a_short_ndrange_writes_nothing_outside_it(ctx, name):
    fx, d = fixture(name)
    p = packed(d)
    w, h = p.width, p.height
    gx, gy = w - 7, h - 5
    full_px, full_rays = enqueue_stream(ctx, p, [w, h])
    assert np.array_equal(full_px.reshape(-1, 4), fx["pixel"]) and (full_px[:gy, :gx, :3] != 0).any()
    px, rays = enqueue_stream(ctx, p, [gx, gy])
    inside = np.zeros((h, w), bool)
    inside[:gy, :gx] = True
    assert np.array_equal(px[inside], full_px[inside])
    assert np.array_equal(rays[inside][:, :40], full_rays[inside][:, :40])
    assert (rays[inside][:, 40:] == SENTINEL).all(), "the 8 bytes of padding of a ray are never written"
    assert (px[~inside] == SENTINEL).all() and (rays[~inside] == SENTINEL).all()
