"""GPU: the refusals of the query entry points, word for word.  A fixed table of refused calls goes through ctypes; each case's (status,
mirt_last_error text) is compared with tests/golden/query_refusals.json, recorded once from the library as it stood before the entry points' host
scaffolding was shared (`python tests/test_query_refusals.py --record` rewrites it).  Every case is refused before anything is queued, so the
file runs in moments: the `guard` stratum scene of tests/rays_common.py (37 x 21 x 4), a standard 13 x 7 k = 2 view camera, 64 rays.

Entry points: mirt_render_guides, mirt_render_ao, mirt_trace_closest, mirt_trace_occluded, mirt_trace_radiance, mirt_view_rays, mirt_render_view,
mirt_view_guides, mirt_render_view_guided, mirt_view_ao, mirt_render_first_pass_guided, mirt_render_passes_guided and the six mirt_*_deferred.
Per entry point: an unknown context; every pointer argument NULL, one at a time; every descriptor with a wrong struct_size; every buffer -- the
descriptor's own seeds / acu / pixel / material where the call has rules for them -- one byte short, released, and of another context; every
output aliasing an input (seeds, rays, a geometry buffer, the material) where the call reads one, and two outputs aliasing each other; the call
inside mirt_capture_begin / mirt_capture_end; and calls with two faults at once, which pin the order of the checks.  (mirt_render_guides has no
aliasing rule, so no such case.)  Messages of device errors quote source text and are not part of the table: no case reaches the device.
"""
import ctypes as C
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_refusals.json")
E_ARG, E_HANDLE, E_RANGE = -1, -2, -5
N_RAYS = 64
SAMPLES, RADIUS, BIAS = 3, 16.0, 0.001
DEFERRED = ("mirt_pass_deferred", "mirt_ao_deferred", "mirt_trace_deferred", "mirt_radiance_deferred", "mirt_view_deferred", "mirt_view_ao_deferred")


class Table:
    """the cases, in a fixed order: name -> (expected status or None, thunk that makes the call and returns its status)"""

    def __init__(self, ctx, other):
        import rays_common as R
        import view_common as V
        from raytracing_amd.pyhost import mirt
        self.mirt, self.L, self.ctx, self.other = mirt, mirt.lib(), ctx, other
        sc = R.scene("guard")
        self.dev = mirt.DeviceScene(ctx, sc)
        self.npix, self.nrays = sc.width * sc.height, sc.width * sc.height * sc.rpp
        self.row_pix = sc.width
        self.view = V.standard_view(sc, "equirect")
        self.vr, self.vp = self.view.n_rays, self.view.n_pixels
        self.cases = {}
        self.made = []
        self.shorts = {}
        not_a_handle = C.create_string_buffer(256)
        self.keep = [not_a_handle]
        self.fake = C.c_void_p(C.addressof(not_a_handle))
        # a buffer of this context that holds any output whole (two outputs aliasing each other; a descriptor's buffer an output meets), a second
        # one, a material table of that size, the largest geometry buffer, a buffer of the other context
        self.big_bytes = max(self.nrays * 16, self.vr * 4, N_RAYS * 32)
        self.big, self.big2, self.big_material = self.buf(self.big_bytes), self.buf(self.big_bytes), self.buf(self.big_bytes)
        self.geo = max((b for b in self.dev.bufs if b is not self.dev.material), key=lambda b: b.nbytes)
        assert self.geo.nbytes >= max(self.row_pix * 16, self.view.width * 16, 32), "no geometry buffer holds a row of guides"
        self.foreign = other.buffer(self.big_bytes)
        # a handle that was live once: released behind every other allocation, so that none of them can take its address
        gone = ctx.buffer(self.big_bytes)
        self.released = C.c_void_p(gone.h.value)
        self.build()
        gone.release()

    # ---- pieces --------------------------------------------------------------------------------------------------------------------------------
    def buf(self, nbytes):
        b = self.ctx.buffer(nbytes)
        self.made.append(b)
        return b

    def short(self, nbytes):
        """a buffer one byte short of nbytes"""
        if nbytes not in self.shorts:
            self.shorts[nbytes] = self.buf(nbytes - 1)
        return self.shorts[nbytes]

    def scene_desc(self, **fields):
        d = self.dev.pass_desc(None, None)
        for k, v in fields.items():
            setattr(d, k, v.h if isinstance(v, self.mirt.Buffer) else v)
        return d

    def view_desc(self, **fields):
        d = self.view.desc()
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    def ao_desc(self, size=None):
        return self.mirt._AoDesc(C.sizeof(self.mirt._AoDesc) if size is None else size, SAMPLES, RADIUS, BIAS)

    def radiance_desc(self, size=None):
        return self.mirt._RadianceDesc(C.sizeof(self.mirt._RadianceDesc) if size is None else size, 1, 0, 0)

    def arg(self, v):
        if isinstance(v, C.Structure):
            return C.byref(v)
        if isinstance(v, self.mirt.Buffer):
            return v.h
        return self.released if isinstance(v, str) and v == "released" else v

    def add(self, name, want, fn, args, c=None):
        assert name not in self.cases, name
        f, argv = getattr(self.L, fn), [self.arg(v) for v in args]
        self.keep.append(args)   # (the descriptors the pointers of argv point into)
        self.cases[name] = (want, lambda: f(self.ctx.h if c is None else c, *argv))

    def entry(self, fn, params, descs=(), bufs=(), inner=(), aliases=(), two_faults=()):
        """params: [(name, default)] behind the context.  descs: {name: its variant with a wrong struct_size}.  bufs: {name: the bytes the call needs
        of it}.  inner: {case name: (descriptor parameter, a function of a buffer -> that descriptor with the buffer in the field, bytes)} -- a
        buffer the call reaches through a descriptor.  aliases, two_faults: {case name: {parameter: value}}."""
        names = [n for n, _ in params]
        base = dict(params)

        def args(**over):
            assert set(over) <= set(names), over
            return [over.get(n, base[n]) for n in names]
        self.add(f"{fn}/unknown_context", E_HANDLE, fn, args(), c=self.fake)
        for n in list(descs) + list(bufs):
            self.add(f"{fn}/{n}_null", None, fn, args(**{n: None}))
        for n, wrong in dict(descs).items():
            self.add(f"{fn}/{n}_struct_size", E_ARG, fn, args(**{n: wrong}))
        for n, nbytes in dict(bufs).items():
            self.add(f"{fn}/{n}_short", E_RANGE, fn, args(**{n: self.short(nbytes)}))
            self.add(f"{fn}/{n}_released", E_HANDLE, fn, args(**{n: "released"}))
            self.add(f"{fn}/{n}_other_context", E_ARG, fn, args(**{n: self.foreign}))
        for n, (param, make, nbytes) in dict(inner).items():
            self.add(f"{fn}/{n}_null", None, fn, args(**{param: make(None)}))
            self.add(f"{fn}/{n}_short", E_RANGE, fn, args(**{param: make(self.short(nbytes))}))
            self.add(f"{fn}/{n}_released", E_HANDLE, fn, args(**{param: make("released")}))
            self.add(f"{fn}/{n}_other_context", E_ARG, fn, args(**{param: make(self.foreign)}))
        for n, over in dict(aliases).items():
            self.add(f"{fn}/alias_{n}", E_ARG, fn, args(**over))
        for n, over in dict(two_faults).items():
            c = over.pop("ctx", None) if isinstance(over, dict) else None
            self.add(f"{fn}/both_{n}", None, fn, args(**over), c=c)
        self.add(f"{fn}/capturing", "capturing", fn, args())

    # ---- the table -----------------------------------------------------------------------------------------------------------------------------
    def build(self):
        m, buf, sd, vd = self.mirt, self.buf, self.scene_desc, self.view_desc
        npix, nrays, vr, vp, n = self.npix, self.nrays, self.vr, self.vp, N_RAYS
        big, big2, geo, bigmat = self.big, self.big2, self.geo, self.big_material
        scene = sd()
        wrong_scene = sd(struct_size=C.sizeof(m._PassDesc) - 4)
        wrong_view = vd(struct_size=C.sizeof(m._ViewDesc) + 4)
        row_scene, row_view = sd(nrows=1), vd(nrows=1)          # a tile of one row: its outputs fit the largest geometry buffer
        too_many = sd(n_meshes=17)                                # MIRT_MAX_MESHES is 16
        no_meshes = sd(n_meshes=1, meshes=None)
        too_many_lights = sd(n_lights=9)                          # MIRT_MAX_LIGHTS is 8

        def released_field(field):
            def make(b):
                return sd(**{field: self.arg(b)})
            return make

        nh, ad = buf(npix * 16), buf(npix * 16)
        self.entry("mirt_render_guides", [("desc", scene), ("normal_hits", nh), ("albedo_depth", ad)],
                   descs={"desc": wrong_scene}, bufs={"normal_hits": npix * 16, "albedo_depth": npix * 16},
                   inner={"material": ("desc", released_field("material"), 16)},
                   two_faults={"no_guides_and_rpp_1": dict(desc=sd(rays_per_pixel=1), normal_hits=None, albedo_depth=None),
                               "short_guide_and_too_many_meshes": dict(desc=too_many, normal_hits=self.short(npix * 16)),
                               "released_guide_and_short_guide": dict(normal_hits="released", albedo_depth=self.short(npix * 16))})
        self.cases.pop("mirt_render_guides/normal_hits_null")      # either guide may be NULL
        self.cases.pop("mirt_render_guides/albedo_depth_null")
        self.add("mirt_render_guides/both_guides_null", E_ARG, "mirt_render_guides", [scene, None, None])

        ao_seeds, ao_out = buf(nrays * 4), buf(npix * 8)
        ao_scene = sd(seeds=ao_seeds)
        self.entry("mirt_render_ao", [("desc", ao_scene), ("ao", self.ao_desc()), ("ao_out", ao_out)],
                   descs={"desc": sd(seeds=ao_seeds, struct_size=8), "ao": self.ao_desc(size=12)}, bufs={"ao_out": npix * 8},
                   inner={"seeds": ("desc", released_field("seeds"), nrays * 4)},
                   aliases={"ao_out_is_seeds": dict(ao_out=ao_seeds), "ao_out_is_geometry": dict(desc=sd(seeds=ao_seeds, nrows=1), ao_out=geo)},
                   two_faults={"no_output_and_no_seeds": dict(desc=scene, ao_out=None), "short_seeds_and_short_output": dict(desc=sd(seeds=self.short(nrays * 4)), ao_out=self.short(npix * 8)),
                               "short_output_and_aliased": dict(ao_out=self.short(nrays * 4), desc=sd(seeds=self.short(nrays * 4))),
                               "bad_ao_and_bad_scene": dict(desc=wrong_scene, ao=self.ao_desc(size=12))})

        rays, hits, sets, occ = buf(n * 32), buf(n * 32), buf(n * 4), buf(n)
        self.entry("mirt_trace_closest", [("desc", scene), ("rays", rays), ("count", n), ("hits", hits), ("sets", sets)],
                   descs={"desc": wrong_scene}, bufs={"rays": n * 32, "hits": n * 32, "sets": n * 4},
                   aliases={"hits_is_rays": dict(hits=rays), "sets_is_rays": dict(sets=rays), "hits_is_geometry": dict(hits=geo, count=1),
                            "sets_is_geometry": dict(sets=geo, count=1), "hits_is_sets": dict(hits=big, sets=big)},
                   two_faults={"no_rays_and_too_many_meshes": dict(rays=None, desc=too_many), "no_rays_and_no_mesh_array": dict(rays=None, desc=no_meshes),
                               "no_rays_and_no_outputs": dict(rays=None, hits=None, sets=None), "short_rays_and_short_hits": dict(rays=self.short(n * 32), hits=self.short(n * 32)),
                               "short_sets_and_aliased_hits": dict(hits=rays, sets=self.short(n * 4)), "aliased_input_and_outputs": dict(hits=rays, sets=rays),
                               "too_many_rays_and_no_outputs": dict(count=0xFFFFFF01, hits=None, sets=None)})
        self.cases.pop("mirt_trace_closest/hits_null")             # either output may be NULL
        self.cases.pop("mirt_trace_closest/sets_null")
        self.add("mirt_trace_closest/both_outputs_null", E_ARG, "mirt_trace_closest", [scene, rays, n, None, None])
        self.entry("mirt_trace_occluded", [("desc", scene), ("rays", rays), ("count", n), ("occluded", occ)],
                   descs={"desc": wrong_scene}, bufs={"rays": n * 32, "occluded": n},
                   aliases={"occluded_is_rays": dict(occluded=rays), "occluded_is_geometry": dict(occluded=geo, count=1)},
                   two_faults={"no_rays_and_no_output": dict(rays=None, occluded=None), "no_rays_and_too_many_meshes": dict(rays=None, desc=too_many),
                               "released_rays_and_short_output": dict(rays="released", occluded=self.short(n))})

        rseeds, rad = buf(n * 4), buf(n * 16)
        self.entry("mirt_trace_radiance", [("desc", scene), ("rd", self.radiance_desc()), ("rays", rays), ("count", n), ("seeds", rseeds), ("radiance", rad)],
                   descs={"desc": wrong_scene, "rd": self.radiance_desc(size=12)}, bufs={"rays": n * 32, "seeds": n * 4, "radiance": n * 16},
                   inner={"material": ("desc", released_field("material"), 16)},
                   aliases={"seeds_is_rays": dict(seeds=rays), "radiance_is_rays": dict(radiance=rays), "radiance_is_geometry": dict(radiance=geo, count=1),
                            "seeds_is_geometry": dict(seeds=geo, count=1), "radiance_is_material": dict(desc=sd(material=bigmat), radiance=bigmat),
                            "seeds_is_radiance": dict(seeds=big, radiance=big)},
                   two_faults={"no_rays_and_too_many_lights": dict(rays=None, desc=too_many_lights), "no_rays_and_no_seeds": dict(rays=None, seeds=None),
                               "no_seeds_and_no_radiance": dict(seeds=None, radiance=None), "short_radiance_and_no_material": dict(radiance=self.short(n * 16), desc=sd(material=None)),
                               "no_material_and_aliased": dict(desc=sd(material=None), seeds=rays), "aliased_input_and_outputs": dict(seeds=rays, radiance=rays)})

        vrays = buf(vr * 32)
        self.entry("mirt_view_rays", [("view", vd()), ("rays", vrays)], descs={"view": wrong_view}, bufs={"rays": vr * 32},
                   two_faults={"bad_view_and_no_rays": dict(view=vd(k=3), rays=None), "unknown_context_and_no_view": dict(ctx=self.fake, view=None)})

        vseeds, vrad, vpix, vnh, vad = buf(vr * 4), buf(vp * 16), buf(vp * 4), buf(vp * 16), buf(vp * 16)
        self.entry("mirt_render_view", [("desc", scene), ("view", vd()), ("seeds", vseeds), ("radiance", vrad), ("pixel", vpix)],
                   descs={"desc": wrong_scene, "view": wrong_view}, bufs={"seeds": vr * 4, "radiance": vp * 16, "pixel": vp * 4},
                   inner={"material": ("desc", released_field("material"), 16)},
                   aliases={"radiance_is_geometry": dict(view=row_view, radiance=geo), "seeds_is_geometry": dict(view=row_view, seeds=geo),
                            "pixel_is_material": dict(desc=sd(material=bigmat), pixel=bigmat), "seeds_is_radiance": dict(seeds=big, radiance=big),
                            "radiance_is_pixel": dict(radiance=big, pixel=big)},
                   two_faults={"bad_view_and_too_many_lights": dict(view=vd(k=3), desc=too_many_lights), "no_seeds_and_too_many_meshes": dict(seeds=None, desc=too_many),
                               "short_pixel_and_no_material": dict(pixel=self.short(vp * 4), desc=sd(material=None)), "no_material_and_aliased": dict(desc=sd(material=None), seeds=big, radiance=big),
                               "aliased_input_and_outputs": dict(view=row_view, radiance=geo, pixel=geo)})
        for name in ("radiance_null", "pixel_null"):               # either output may be NULL
            self.cases.pop("mirt_render_view/" + name)
        self.add("mirt_render_view/both_outputs_null", E_ARG, "mirt_render_view", [scene, vd(), vseeds, None, None])
        self.entry("mirt_view_guides", [("desc", scene), ("view", vd()), ("normal_hits", vnh), ("albedo_depth", vad)],
                   descs={"desc": wrong_scene, "view": wrong_view}, bufs={"normal_hits": vp * 16, "albedo_depth": vp * 16},
                   inner={"material": ("desc", released_field("material"), 16)},
                   aliases={"normal_hits_is_geometry": dict(view=row_view, normal_hits=geo), "albedo_depth_is_material": dict(desc=sd(material=bigmat), albedo_depth=bigmat),
                            "normal_hits_is_albedo_depth": dict(normal_hits=big, albedo_depth=big)},
                   two_faults={"no_guides_and_too_many_meshes": dict(normal_hits=None, albedo_depth=None, desc=too_many),
                               "aliased_input_and_outputs": dict(view=row_view, normal_hits=geo, albedo_depth=geo)})
        for name in ("normal_hits_null", "albedo_depth_null"):
            self.cases.pop("mirt_view_guides/" + name)
        self.add("mirt_view_guides/both_guides_null", E_ARG, "mirt_view_guides", [scene, vd(), None, None])
        self.entry("mirt_render_view_guided", [("desc", scene), ("view", vd()), ("seeds", vseeds), ("radiance", vrad), ("pixel", vpix), ("normal_hits", vnh), ("albedo_depth", vad)],
                   descs={"desc": wrong_scene, "view": wrong_view},
                   bufs={"seeds": vr * 4, "radiance": vp * 16, "pixel": vp * 4, "normal_hits": vp * 16, "albedo_depth": vp * 16},
                   inner={"material": ("desc", released_field("material"), 16)},
                   aliases={"normal_hits_is_geometry": dict(view=row_view, normal_hits=geo), "radiance_is_material": dict(desc=sd(material=bigmat), radiance=bigmat),
                            "normal_hits_is_seeds": dict(normal_hits=big, seeds=big), "normal_hits_is_albedo_depth": dict(normal_hits=big, albedo_depth=big),
                            "albedo_depth_is_radiance": dict(albedo_depth=big, radiance=big)},
                   two_faults={"no_guides_and_no_outputs": dict(radiance=None, pixel=None, normal_hits=None, albedo_depth=None),
                               "short_seeds_and_short_guide": dict(seeds=self.short(vr * 4), albedo_depth=self.short(vp * 16))})
        for name in ("radiance_null", "pixel_null", "normal_hits_null", "albedo_depth_null"):
            self.cases.pop("mirt_render_view_guided/" + name)
        self.add("mirt_render_view_guided/both_outputs_null", E_ARG, "mirt_render_view_guided", [scene, vd(), vseeds, None, None, vnh, vad])
        self.add("mirt_render_view_guided/both_guides_null", E_ARG, "mirt_render_view_guided", [scene, vd(), vseeds, vrad, vpix, None, None])

        vao_seeds, vao_out = buf(vr * 4), buf(vp * 8)
        self.entry("mirt_view_ao", [("desc", scene), ("view", vd()), ("ao", self.ao_desc()), ("seeds", vao_seeds), ("ao_out", vao_out)],
                   descs={"desc": wrong_scene, "view": wrong_view, "ao": self.ao_desc(size=12)}, bufs={"seeds": vr * 4, "ao_out": vp * 8},
                   aliases={"ao_out_is_seeds": dict(ao_out=vao_seeds), "ao_out_is_geometry": dict(view=row_view, ao_out=geo)},
                   two_faults={"no_seeds_and_no_output": dict(seeds=None, ao_out=None), "no_output_and_too_many_meshes": dict(ao_out=None, desc=too_many),
                               "short_seeds_and_short_output": dict(seeds=self.short(vr * 4), ao_out=self.short(vp * 8)),
                               "short_output_and_aliased": dict(seeds=self.short(vr * 4), ao_out=self.short(vr * 4))})

        pseeds, acu, pixel = buf(nrays * 4), buf(nrays * 16), buf(npix * 4)

        def pd(**fields):
            return sd(seeds=fields.pop("seeds", pseeds), acu=fields.pop("acu", acu), pixel=fields.pop("pixel", pixel), **fields)

        def pass_field(field):
            def make(b):
                return pd(**{field: self.arg(b)})
            return make
        for fn, extra in (("mirt_render_first_pass_guided", []), ("mirt_render_passes_guided", [("n_passes", 2), ("flags", m.PASSES_FRESH)])):
            self.entry(fn, [("desc", pd())] + extra + [("normal_hits", nh), ("albedo_depth", ad)],
                       descs={"desc": pd(struct_size=C.sizeof(m._PassDesc) - 4)}, bufs={"normal_hits": npix * 16, "albedo_depth": npix * 16},
                       inner={"seeds": ("desc", pass_field("seeds"), nrays * 4), "acu": ("desc", pass_field("acu"), nrays * 16),
                              "pixel": ("desc", pass_field("pixel"), npix * 4), "material": ("desc", pass_field("material"), 16)},
                       aliases={"normal_hits_is_seeds": dict(desc=pd(seeds=big), normal_hits=big), "albedo_depth_is_acu": dict(albedo_depth=acu),
                                "normal_hits_is_pixel": dict(desc=pd(pixel=big), normal_hits=big), "albedo_depth_is_radiance": dict(desc=pd(radiance=big2), albedo_depth=big2),
                                "normal_hits_is_material": dict(desc=pd(material=bigmat), normal_hits=bigmat), "normal_hits_is_geometry": dict(desc=pd(nrows=1), normal_hits=geo),
                                "normal_hits_is_albedo_depth": dict(normal_hits=big, albedo_depth=big)},
                       two_faults={"no_guides_and_rpp_1": dict(desc=pd(rays_per_pixel=1), normal_hits=None, albedo_depth=None),
                                   "short_seeds_and_short_guide": dict(desc=pd(seeds=self.short(nrays * 4)), normal_hits=self.short(npix * 16)),
                                   "short_guide_and_aliased": dict(normal_hits=self.short(npix * 16), albedo_depth=acu),
                                   "aliased_input_and_outputs": dict(normal_hits=acu, albedo_depth=acu)})
            for name in ("normal_hits_null", "albedo_depth_null", "acu_null", "pixel_null"):   # optional, or NULL under conditions of the pass's own
                self.cases.pop(f"{fn}/{name}")
            tail = [v for _, v in extra]
            self.add(f"{fn}/both_guides_null", E_ARG, fn, [pd()] + tail + [None, None])
        self.add("mirt_render_passes_guided/both_unknown_flags_and_no_guides", None, "mirt_render_passes_guided", [pd(), 2, 0x10, None, None])
        self.add("mirt_render_passes_guided/both_no_passes_and_short_guide", None, "mirt_render_passes_guided", [pd(), 0, m.PASSES_FRESH, self.arg(self.short(npix * 16)), ad])

        out = C.c_uint64()
        for fn in DEFERRED:
            self.add(f"{fn}/unknown_context", E_HANDLE, fn, [C.byref(out)], c=self.fake)
            self.add(f"{fn}/out_null", E_ARG, fn, [None])
            self.add(f"{fn}/both_unknown_context_and_out_null", E_HANDLE, fn, [None], c=self.fake)
            self.add(f"{fn}/capturing", "capturing", fn, [C.byref(out)])

    # ---- running -------------------------------------------------------------------------------------------------------------------------------
    def run(self):
        """-> ({name: [status, text]}, the cases whose status is not the one the table expects); the `capturing` cases run last, inside one
        empty recording"""
        got, unexpected = {}, []

        def one(name, want, call):
            status = call()
            text = self.L.mirt_last_error(None).decode()
            ok = status != 0 and (want is None or (status == E_ARG and "mirt_capture_begin/end" in text if want == "capturing" else status == want))
            if not ok:
                unexpected.append(f"{name}: status {status} ({text}), the table expects {want}")
            got[name] = [status, text]
        for name, (want, call) in self.cases.items():
            if want != "capturing":
                one(name, want, call)
        self.ctx.finish()
        self.ctx.capture_begin()
        try:
            for name, (want, call) in self.cases.items():
                if want == "capturing":
                    one(name, want, call)
        finally:
            self.ctx.graph_release(self.ctx.capture_end())
        return got, unexpected

    def release(self):
        self.foreign.release()
        for b in self.made:
            b.release()
        self.dev.release()


def record_or_run():
    from raytracing_amd.pyhost import mirt
    ctx, other = mirt.Context(0), mirt.Context(0)
    try:
        t = Table(ctx, other)
        try:
            return t.run()
        finally:
            t.release()
    finally:
        other.destroy()
        ctx.destroy()


def test_every_refusal_is_the_recorded_one(pkg):
    with open(GOLDEN_FILE) as f:
        want = json.load(f)["cases"]
    got, unexpected = record_or_run()
    assert not unexpected, "\n".join(unexpected)
    assert sorted(got) == sorted(want), "the table and the golden file list different cases: " + str(sorted(set(got) ^ set(want)))
    different = [f"{name}: got {got[name]}, recorded {want[name]}" for name in got if got[name] != want[name]]
    assert not different, "\n".join(different)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_query_refusals.py --record   (rewrites tests/golden/query_refusals.json from the library as built)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle"), os.path.join(root, "tests")]
    import __graft_entry__ as g
    g.load_package()
    cases, unexpected = record_or_run()
    print("\n".join(unexpected))
    with open(GOLDEN_FILE, "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(cases)} refusals in {GOLDEN_FILE}")
    sys.exit(1 if unexpected else 0)
