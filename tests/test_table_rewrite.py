"""GPU (and one CPU test of what the steps are made of): cell tables and primitive arrays that change IN PLACE, in the same buffers of one
DeviceScene on one context.  The runtime caches what it derives from a table and from triangle positions -- the validation verdict and off[n^3] (off_version / off_n / off_last), the prepared
copy and its plane list, and with them what is staged in LDS -- keyed on the buffer's version.  After every step the ray queries and a fused pass
are compared with the CPU oracle's result for the scene the buffers NOW hold (tests/table_edits_common.py), at tolerance 0.

  1. mirt_buf_write: a single-cell set from 96 slots (staged) to 97 (it leaves LDS, the sets behind it enter) and back; a grid from the
     `drop` table back to the builder's -- each a valid table with another off[n^3];
  2. mirt_buf_invalidate: the same changes made through a wrapped view over the owner's device_ptr, then mirt_buf_invalidate(owner) on each
     buffer: the next launch gives the new scene's result;
  3. wrapped geometry: the table and the arrays are mirt_buf_wrap views; they change through a SECOND wrapped view of the same memory and the
     runtime is told nothing: the next launch re-validates (include/mirt.h at mirt_buf_wrap) and gives the new result; a rewrite to a
     decreasing table is MIRT_E_DATA, and the context works afterwards."""
import numpy as np
import pytest

import a10_pass as A
import random_scenes_common as S
import rays_common as R
import table_edits_common as T

E_DATA = -8


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def variant(cid):
    """(scene, rays, set, the batch's name for table_edits_common.expected)"""
    ed = T.case(cid)
    return ed.scene, ed.rays(), ed.sid, None


def builder(cid):
    """the base scene of a case, with the case's ray batch"""
    ed = T.case(cid)
    return ed.base, ed.rays(), ed.sid, cid


def dev_set(dev, sid):
    return dev.sph if sid == "spheres" else dev.tri if sid == "triangles" else dev.meshes[sid[1]]


def arrays_of(sc, sid):
    """{key of DeviceScene's set dict: the array the scene holds for it}"""
    s = T._get(sc.d, sid)
    out = {"off": s["off"], "prims": s["arrs"]["prims"]}
    if "normals" in s["arrs"]:
        out["normals"] = s["arrs"]["normals"]
    if "matid" in s["arrs"]:
        out["matid"] = s["arrs"]["matid"]
    return out


class Bench:
    """one DeviceScene (a rays_common.Tracer's) and the buffers of a fused pass on it"""

    def __init__(self, ctx, sc, cap):
        self.ctx, self.t = ctx, R.Tracer(ctx, sc, cap=cap)
        self.dev = self.t.dev
        n, npix = sc.total_rays, sc.width * sc.height
        self.seeds, self.acu, self.pixel, self.radiance = ctx.buffer(n * 4), ctx.buffer(n * 16), ctx.buffer(npix * 4), ctx.buffer(npix * 16)
        self.views = []

    def check(self, tag, sc, rays, batch=None):
        """the ray queries and a fresh fused pass against the oracle's result for `sc`"""
        from test_rays import check_closest, check_occluded
        hits, sets, occ = T.expected(sc, rays, batch)
        self.t.desc = self.dev.pass_desc(None, None)
        check_closest(tag, self.t, rays, hits, sets)
        check_occluded(tag, self.t, rays, occ)
        seeds = A.make_seeds(sc.total_rays, seed_base=sc.key[1])
        want = S.expected(sc, seeds, 1)[0]
        self.seeds.write(seeds)
        self.acu.write(np.full(sc.total_rays * 4, np.nan, np.float32))
        self.ctx.render_pass(self.dev.pass_desc(self.seeds, self.acu, self.pixel, self.radiance, pass_index=1), fresh=True)
        d = S.words_differ(f"{tag} acu", self.acu.read(np.float32), want.acu)
        assert d is None, d
        assert np.array_equal(self.seeds.read(np.int32), want.seeds), f"{tag}: seeds"
        assert np.array_equal(self.pixel.read(np.uint8).reshape(-1, 4), want.pixel), f"{tag}: pixel"

    def view(self, buf):
        v = self.ctx.wrap(buf.device_ptr, buf.nbytes)
        self.views.append(v)
        return v

    def release(self):
        for b in self.views + [self.seeds, self.acu, self.pixel, self.radiance]:
            b.release()
        self.t.release()


def rewrite(bench, sc, sid, how):
    """the set's table and arrays of `sc` into the DeviceScene's buffers.  how: "write" -- mirt_buf_write on the buffers themselves;
    "invalidate" -- through a wrapped view of each, then mirt_buf_invalidate on the owner; "behind" -- through a wrapped view, nothing said"""
    g = dev_set(bench.dev, sid)
    for key, arr in arrays_of(sc, sid).items():
        assert arr.nbytes <= g[key].nbytes, f"{key}: the buffer is too small for this variant"
        if how == "write":
            g[key].write(arr)
        else:
            bench.view(bench.owner.get(id(g[key]), g[key]) if how == "behind" else g[key]).write(arr)
            if how == "invalidate":
                g[key].invalidate()


# (cell set 96 -> 97 -> 96: the 60-record loose set of the 60 / 40 / 7 scene behind 36 and 37 poison slots; grid: the room of `staged` 3003)
STEPS = {"cell_96_97_96": (variant("lead97"), [variant("lead96"), variant("lead97"), variant("lead96")]),
         "grid_drop_builder": (builder("staged_grid-drop"), [variant("staged_grid-drop"), builder("staged_grid-drop"), variant("staged_grid-drop")])}


def test_the_steps_change_off_last_and_the_staging():
    """CPU: what the steps are made of"""
    a, b = T.case("lead96").scene, T.case("lead97").scene
    assert int(a.t_box[-1]) == 96 and int(b.t_box[-1]) == 97 and int(a.t_box[0]) == 36 and int(b.t_box[0]) == 37
    assert S.kernel_choice(a)["tri_staged"] == [True, False, False] and S.kernel_choice(b)["tri_staged"] == [False, True, True]
    d, base = T.case("staged_grid-drop"), T.case("staged_grid-drop").base
    assert int(d.set()["off"][-1]) < int(T._get(base.d, d.sid)["off"][-1])
    for first, steps in STEPS.values():     # every variant fits the buffers of the first: the DeviceScene is made from the largest
        for sc, _, sid, _ in steps:
            for key, arr in arrays_of(sc, sid).items():
                assert arr.nbytes <= arrays_of(first[0], sid)[key].nbytes


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["write", "invalidate"])
@pytest.mark.parametrize("name", list(STEPS))
def test_a_table_rewritten_in_its_buffers_gives_the_new_scene(ctx, name, how):
    (sc0, rays0, sid, batch0), steps = STEPS[name]
    bench = Bench(ctx, sc0, cap=len(rays0))
    bench.owner = {}
    try:
        bench.check(f"{name} as uploaded", sc0, rays0, batch0)
        for i, (sc, rays, _, batch) in enumerate(steps):
            rewrite(bench, sc, sid, how)
            bench.check(f"{name} {how} step {i + 1} ({sc.key[-2] if len(sc.key) > 5 else 'builder'})", sc, rays, batch)
    finally:
        bench.release()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEPS))
def test_wrapped_geometry_is_validated_again_at_every_launch(ctx, name):
    from raytracing_amd.pyhost import mirt
    (sc0, rays0, sid, batch0), steps = STEPS[name]
    bench = Bench(ctx, sc0, cap=len(rays0))
    g = dev_set(bench.dev, sid)
    bench.owner = {}
    for key in arrays_of(sc0, sid):          # the set's table and arrays become views of memory the runtime does not own
        v = bench.view(g[key])
        bench.owner[id(v)] = g[key]
        g[key] = v
    try:
        bench.check(f"{name} wrapped, as uploaded", sc0, rays0, batch0)
        for i, (sc, rays, _, batch) in enumerate(steps):
            rewrite(bench, sc, sid, "behind")
            bench.check(f"{name} behind the runtime, step {i + 1}", sc, rays, batch)
        # a decreasing table: refused, nothing written, and the context goes on
        sc, rays, _, batch = steps[-1]
        good = arrays_of(sc, sid)["off"]
        bad = good.copy()
        bad[0], bad[1] = good[-1], 0
        behind = bench.view(bench.owner[id(g["off"])])
        behind.write(bad)
        bench.t.fill()
        with pytest.raises(mirt.MirtError) as e:
            ctx.trace_closest(bench.dev.pass_desc(None, None), bench.t.rays, len(rays), bench.t.hits, bench.t.sets)
        assert e.value.code == E_DATA, str(e.value)
        assert R.untouched(bench.t.hits.read(np.uint8)) and R.untouched(bench.t.sets.read(np.uint8))
        with pytest.raises(mirt.MirtError) as e:
            ctx.render_pass(bench.dev.pass_desc(bench.seeds, bench.acu, bench.pixel, bench.radiance, pass_index=1), fresh=True)
        assert e.value.code == E_DATA, str(e.value)
        behind.write(good)
        bench.check(f"{name} after the refusal", sc, rays, batch)
    finally:
        bench.release()
