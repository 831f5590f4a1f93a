"""Shared by tests/test_ray_guard.py and tests/test_ray_edges.py: the ray-side guard of the optimistic kernel (csrc/pt_trace.hpp ray_guard) stated in
numpy, and the EDGE JOBS -- packed A10 scenes derived from two committed fixtures by edits of the packed dictionary, each built so that the rays
the reference makes sit on a stated side of one edge of that guard: origins at 2^20, 2^-30, -0 and a denormal, direction components that are
exactly 0 or straddle 2^-40, a ray that starts on a bound plane with a zero direction along that axis (the reference's 0 / 0 in the slab test),
degenerate lenses, lights of radius 0, facing away, in a wall's plane, far away or with a non-finite irradiance or area, and the whole scene scaled
to the top of every window at once.

Each job carries a predicate over the CPU oracle's own rays (oracle/a10_pass.py run_pass with checkpoints: primary -> rays, shadow) that says on
which side of its edge it sits, and the counts measured with the oracle when the job was written, so that a change of either shows.  The camera
block, like the bounds, is the caller's word: no kernel checks it."""
import copy

import numpy as np

import a10_pass as A
from conftest import load_fixture

F = np.float32
CORNELL, TEAPOT3 = "cornell_32x24_r4", "cornell_teapot3_32x24_r4"


def P(p):
    return F(2.0) ** F(p)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------
def window_constants(ask):
    """(kDenLo, kDenHi, kPosLo, kPosHi) of csrc/pt_windows.hpp as float32, through tests/set_guard_dump.cpp (`ask`: the fixture of
    tests/test_set_guard.py), not as decimal copies"""
    (got,) = ask(["windows"])
    return np.asarray(got[:4], dtype=np.uint32).view(F)


def accepted(o, d, win):
    """the rule csrc/pt_trace.hpp documents above ray_guard, on float32 arrays [..., 3]: every |d_k| in [kDenLo, kDenHi] and every o_k a zero of
    either sign or |o_k| in [kPosLo, kPosHi].  NaN and infinities fail (every comparison with a NaN is false)."""
    den_lo, den_hi, pos_lo, pos_hi = win
    o, d = np.asarray(o, dtype=F), np.asarray(d, dtype=F)
    with np.errstate(invalid="ignore"):
        ad, ao = np.abs(d), np.abs(o)
        d_ok = (ad >= den_lo) & (ad <= den_hi)
        o_ok = (o == 0) | ((ao >= pos_lo) & (ao <= pos_hi))
    return d_ok.all(axis=-1) & o_ok.all(axis=-1)


# ---- edits of the packed dictionary -----------------------------------------------------------------------------------------------------------
def _variant(sc0, **kw):
    """the same packed scene with fields replaced; a change of the image size re-packs the camera the way Camera.lookAt does
    (as tests/test_gpu_parity.py _variant)"""
    d = dict(sc0.d)
    w, h = kw.pop("width", d["width"]), kw.pop("height", d["height"])
    cam = list(kw.pop("cam", d["cam"]))
    cam[12] = float(F(cam[13] * (w / h)))
    cam[14], cam[15] = float(w), float(h)
    d.update(cam=cam, width=w, height=h, **kw)
    return A.Scene(d)


def _f32_list(v):
    return [float(x) for x in np.asarray(v, dtype=F).ravel()]


def _moved(values, index, t):
    """values[index] + t, the sum formed in fp64 and narrowed to fp32"""
    a = np.asarray(values, dtype=F).astype(np.float64).ravel()
    a[index] = a[index] + t
    return _f32_list(a.astype(F))


def _scaled(values, index, s):
    a = np.asarray(values, dtype=F).astype(np.float64).ravel()
    a[index] = a[index] * s
    out = a.astype(F)
    assert np.array_equal(out.astype(np.float64), a), "the scaling is exact"
    return _f32_list(out)


def _xyz(length, stride):
    """indices of the x, y, z components of records `stride` floats apart"""
    return np.concatenate([np.arange(k, length, stride) for k in range(3)])


def with_eye(d, **axes):
    cam = list(d["cam"])
    for k, v in axes.items():
        cam["xyz".index(k)] = float(F(v))
    return dict(d, cam=cam)


def translated(d, axis, t):
    """every position of the job moved by t along one axis: the eye, the scene bounds, each set's bounds, sphere centres, triangle vertices, and the
    position in all three packed blocks of every light"""
    d = dict(d)
    d["cam"] = _moved(d["cam"], [axis], t)
    for key in ("bounds", "sphere_bounds", "triangle_bounds"):
        if key in d:
            d[key] = _moved(d[key], [axis, 4 + axis], t)
    if d.get("n_spheres", 0):
        d["spheres"] = _moved(d["spheres"], np.arange(axis, len(d["spheres"]), 4), t)
    if d.get("n_triangles", 0):
        d["t_pos"] = _moved(d["t_pos"], np.arange(axis, len(d["t_pos"]), 4), t)
    d["meshes"] = [dict(m, pos=_moved(m["pos"], np.arange(axis, len(m["pos"]), 4), t), bounds=_moved(m["bounds"], [axis, 4 + axis], t))
                   for m in d.get("meshes", [])]
    d["lights"] = [{k: _moved(v, [axis], t) for k, v in l.items()} for l in d["lights"]]
    return d


def scaled(d, s):
    """every length of the scene multiplied by s (a power of two: exact), every area and squared radius by s * s.  Directions -- the camera's
    U, V, W, its window in units of |W|, normals, the lights' tangents -- and the irradiance stay."""
    d = dict(d)
    d["cam"] = _scaled(d["cam"], [0, 1, 2], s)
    d["focal_length"], d["lens_rad"] = float(F(d["focal_length"] * s)), float(F(d["lens_rad"] * s))
    for key in ("bounds", "sphere_bounds", "triangle_bounds"):
        if key in d:
            d[key] = _scaled(d[key], [0, 1, 2, 4, 5, 6], s)
    if d.get("n_spheres", 0):
        d["spheres"] = _scaled(_scaled(d["spheres"], _xyz(len(d["spheres"]), 4), s), np.arange(3, len(d["spheres"]), 4), s * s)
    if d.get("n_triangles", 0):
        d["t_pos"] = _scaled(d["t_pos"], _xyz(len(d["t_pos"]), 4), s)
    d["meshes"] = [dict(m, pos=_scaled(m["pos"], _xyz(len(m["pos"]), 4), s), bounds=_scaled(m["bounds"], [0, 1, 2, 4, 5, 6], s)) for m in d.get("meshes", [])]
    d["lights"] = [dict(shadow=_scaled(l["shadow"], [0, 1, 2, 9], s), light=_scaled(l["light"], [0, 1, 2, 9], s),
                        scene=_scaled(_scaled(l["scene"], [0, 1, 2], s), [9], s * s)) for l in d["lights"]]
    return d


def with_lights(d, edit, only=None):
    """edit(block name, list of 16 floats) -> list, applied to the three packed blocks of every light (or of light `only`)"""
    lights = []
    for i, l in enumerate(d["lights"]):
        lights.append({k: (_f32_list(edit(k, list(v))) if only in (None, i) else list(v)) for k, v in l.items()})
    return dict(d, lights=lights)


def _set(block, index, value):
    block = list(block)
    for i in np.atleast_1d(index):
        block[int(i)] = float(value)
    return block


def _negated(block, index):
    block = list(block)
    for i in index:
        block[i] = -block[i]
    return block


def _scaled_u(d, s):
    cam = list(d["cam"])
    cam[3:6] = _f32_list(np.asarray(cam[3:6], dtype=np.float64) * s)
    return dict(d, cam=cam)


# ---- the jobs ---------------------------------------------------------------------------------------------------------------------------------
class Job:
    """base: the fixture; make(d) -> (d', size and ray-count overrides); outside: what the rule says of the oracle's alive primary rays -- "none",
    "all", "some" (both kinds) or None (no claim); refused: the sets pt_set_guard.hpp refuses (the job's fast_ok table: every other set is
    accepted); at_edge: a value sits ON a bound of the window, so the guard must not defer every alive primary ray; nan_rule: accumulator words
    are equal when their bits are or both are NaN; dark: everything is dark by design (an accumulator with w > 0 instead of a lit pixel);
    measured: counts the oracle gave when the job was written; holds(state): the job's own predicate."""

    def __init__(self, name, base, make, outside=None, refused=(), at_edge=False, nan_rule=False, dark=False, measured=None, holds=None, **size):
        self.name, self.base, self.make, self.outside, self.refused = name, base, make, outside, tuple(refused)
        self.at_edge, self.nan_rule, self.dark, self.measured, self.holds, self.size = at_edge, nan_rule, dark, dict(measured or {}), holds, size

    def scene(self):
        _, base = load_fixture(self.base)
        return _variant(A.Scene(self.make(copy.deepcopy(base.d))), **self.size)


PINHOLE = dict(lens_rad=0.0)
ODD = dict(width=33, height=25)


def _eye_is(state, axis, value):
    o = state.primary["rays"]["o"][state.alive]
    assert len(o) and (o[:, axis].view(np.uint32) == np.asarray(value, dtype=F).view(np.uint32)).all(), "every primary origin is the eye bit for bit"


def _holds_minus_zero(state):
    """o.x = fma(0 * lens sample, U.x, -0): a zero whose sign is the lens sample's -- both zeros in one frame, neither outside the window"""
    assert state.sc.d["cam"][0] == 0.0 and np.signbit(state.sc.d["cam"][0])
    x = state.primary["rays"]["o"][:, 0].view(np.uint32)
    assert ((x & 0x7FFFFFFF) == 0).all() and (x == 0x80000000).any() and (x == 0).any()


def _holds_2p20(past):
    def holds(state):
        d = state.sc.d
        _eye_is(state, 0, P(20) + F(0.125) if past else P(20))
        assert d["triangle_bounds"][4] == float(P(20)) and d["bounds"][4] == float(P(20))
    return holds


def _holds_zero_components(state):
    d = state.primary["rays"]["d"]
    assert ((d[:, 0] == 0).sum(), (d[:, 1] == 0).sum()) == (state.job.measured["dx_zero"], state.job.measured["dy_zero"])


def _holds_zero_on_a_face(state):
    """at least one alive primary ray has d_k == 0 and o_k equal to a bound of the scene box or of a set on axis k"""
    r, d = state.primary["rays"], state.sc.d
    hit = np.zeros(len(r), bool)
    for key in ("bounds", "sphere_bounds", "triangle_bounds"):
        b = np.asarray(d[key], dtype=F)
        for k in range(3):
            hit |= (r["d"][:, k] == 0) & ((r["o"][:, k] == b[k]) | (r["o"][:, k] == b[4 + k]))
    assert (hit & state.alive).any()


def _holds_lens_wide(state):
    """every origin is outside the scene box sideways (the lens samples sit 5 from the axis); the rays still aim at the focal plane inside the
    box, so most are alive -- the oracle shows 326 of 3072 dead, not most of them"""
    r, b = state.primary["rays"], np.asarray(state.sc.d["bounds"], dtype=F)
    out = ((r["o"][:, :2] < b[0:2]) | (r["o"][:, :2] > b[4:6])).any(axis=1)
    assert out.all() and state.alive.any() and not state.alive.all()


def _holds_focal_zero_pinhole(state):
    """every direction is norm3(0), which AMD's normalize() returns as the zero vector itself (not a NaN): six quotients by zero in the scene
    box's slab test, every ray dead, nothing accumulated"""
    r = state.primary["rays"]
    assert (r["d"].view(np.uint32) == 0).all() and not state.alive.any() and not state.st.acu.any()


def _holds_rpp9(state):
    """the NaN centre sample (sample 4 of 9) beside in-window samples in one block"""
    d = state.primary["rays"]["d"].reshape(-1, 9, 3)
    assert np.isnan(d[:, 4]).all() and not np.isnan(d[:, [0, 1, 2, 3, 5, 6, 7, 8]]).any()
    ok = accepted(state.primary["rays"]["o"], state.primary["rays"]["d"], state.win).reshape(-1, 9)
    assert ok[:, 0].any() and not ok[:, 4].any()


def _holds_facing_away(state):
    """the emitters face away from most of the scene, not from all of it (a disc below the ceiling that looks up still lights the ceiling): cosy
    is 0 at most primary vertices -- the shadow skip's branch -- and positive at some -- the traced branch -- in one frame"""
    pois, sh = state.primary["pois"], state.primary["shadow"]
    lnor = np.asarray(state.sc.d["lights"][-1]["scene"][3:6], dtype=np.float64)     # the primary checkpoint holds the LAST light's shadow rays
    live = (pois["matId"] >= 0) & (sh["mint"] != sh["maxt"])
    away = (-sh["d"][live].astype(np.float64)) @ lnor <= 0
    assert (int(live.sum()), int(away.sum())) == (state.job.measured["unblocked"], state.job.measured["cosy_zero"])
    assert 0.5 < away.mean() < 1.0


def _floor_y(d):
    """the height of the floor: the triangles whose vertex normals are (0, 1, 0) and whose three vertices share one y"""
    t, n = np.asarray(d["t_pos"], dtype=F).reshape(-1, 3, 4), np.asarray(d["t_normal"], dtype=F).reshape(-1, 3, 4)
    k = np.flatnonzero((n[:, 0, 1] == 1) & (t[:, 0, 1] == t[:, 1, 1]) & (t[:, 0, 1] == t[:, 2, 1]))
    return float(t[k[0], 0, 1])


def _holds_in_the_floor_plane(state):
    d, pois = state.sc.d, state.primary["pois"]
    y = _floor_y(d)
    assert all(d["lights"][0][k][1] == y for k in ("shadow", "scene", "light"))
    assert d["lights"][0]["shadow"][4] == 0.0 and d["lights"][0]["shadow"][7] == 0.0, "the disc's tangents lie in the plane: every sample has the floor's y"
    # the primary checkpoint holds the LAST light's shadow rays: the floor vertices are checked against the moved light through their position
    floor = (pois["matId"] >= 0) & (pois["normal"][:, 1] == 1.0) & (np.abs(pois["p"][:, 1] - F(y)) < 1e-5)
    assert floor.any()
    assert (pois["p"][floor, 1].astype(np.float64) + 0.001 > y).all(), "every floor vertex looks DOWN at the light: cosx clamps to exactly 0"


def _holds_nonfinite(state):
    acu = state.st.acu
    assert np.isnan(acu).any() and (np.isfinite(acu) & (acu != 0)).any()


def _holds_light_far(state):
    assert all(l[k][1] == float(P(19)) for l in state.sc.d["lights"] for k in ("shadow", "scene", "light"))
    sh, made = state.primary["shadow"], state.primary["pois"]["matId"] >= 0      # (the ceiling blocks every one of them)
    assert made.any() and accepted(sh["o"][made], sh["d"][made], state.win).all(), "the far light's shadow rays are inside the window"
    assert (np.abs(sh["d"][made][:, [0, 2]]) < P(-18)).all()


def _holds_scaled(power):
    def holds(state):
        d = state.sc.d
        assert d["cam"][2] == float(P(power + 1)) and d["bounds"][4:7] == [float(P(power))] * 3 and d["triangle_bounds"][0] == -float(P(power))
        t = np.asarray(d["t_pos"], dtype=np.float64).reshape(-1, 3, 4)[:, :, :3]
        n = np.cross(t[:, 2] - t[:, 0], t[:, 1] - t[:, 0])
        assert np.abs(n).max() == 2.0 ** (2 * power + 2), "the triangle-plane normals"
    return holds


def _nonfinite(block_index):
    def edit(k, b):
        if k == "scene":
            return _set(b, block_index, np.inf)
        if k == "light" and block_index != 9:     # the irradiance is packed into both blocks; the area into `scene` alone
            return _set(b, block_index, np.inf)
        return b
    return edit


JOBS = {j.name: j for j in [
    # ---- origin edges: lens_rad = 0, every primary origin is the eye bit for bit
    Job("eye_at_2p20", CORNELL, lambda d: translated(dict(with_eye(d, x=1.0), **PINHOLE), 0, 2.0 ** 20 - 1.0), outside="some",
        holds=_holds_2p20(False), measured=dict(alive=1608, outside=96, lit=384)),
    Job("eye_past_2p20", CORNELL, lambda d: translated(dict(with_eye(d, x=1.125), **PINHOLE), 0, 2.0 ** 20 - 1.0), outside="all",
        holds=_holds_2p20(True), measured=dict(alive=1396, outside=1396, lit=344)),
    Job("eye_at_2m30", CORNELL, lambda d: dict(with_eye(d, x=P(-30)), **PINHOLE), outside="none", at_edge=True,
        holds=lambda s: _eye_is(s, 0, P(-30)), measured=dict(alive=3048, outside=0, lit=765)),
    Job("eye_below_2m30", CORNELL, lambda d: dict(with_eye(d, x=np.nextafter(P(-30), F(0.0))), **PINHOLE), outside="all",
        holds=lambda s: _eye_is(s, 0, np.nextafter(P(-30), F(0.0))), measured=dict(alive=3048, outside=3048, lit=765)),
    Job("eye_denormal", CORNELL, lambda d: dict(with_eye(d, x=F(1e-40)), **PINHOLE), outside="all",
        holds=lambda s: _eye_is(s, 0, F(1e-40)), measured=dict(alive=3048, outside=3048, lit=762)),
    Job("eye_minus_zero", CORNELL, lambda d: dict(with_eye(d, x=F(-0.0)), **PINHOLE), outside="none", at_edge=True,
        holds=_holds_minus_zero, measured=dict(alive=3048, outside=0, lit=762)),
    # ---- direction edges
    Job("zero_components", CORNELL, lambda d: dict(d, **PINHOLE), outside="some", holds=_holds_zero_components,
        measured=dict(dx_zero=100, dy_zero=132), **ODD),
    Job("zero_on_a_face", CORNELL, lambda d: dict(with_eye(d, x=1.0), **PINHOLE), outside="some", holds=_holds_zero_on_a_face, **ODD),
    # (1040 of all 3072 rays are outside; 256 rays end on the emitter, which leaves 944 of 2816 alive ones)
    Job("tiny_dx_mixed", CORNELL, lambda d: dict(_scaled_u(d, 2.0 ** -38), **PINHOLE), outside="some", measured=dict(alive=2816, outside=944, lit=768)),
    Job("tiny_dx_all", CORNELL, lambda d: dict(_scaled_u(d, 2.0 ** -45), **PINHOLE), outside="all", measured=dict(alive=2816, outside=2816, lit=768)),
    # ---- lens and ray-count edges
    Job("lens_wide", CORNELL, lambda d: dict(d, lens_rad=10.0), holds=_holds_lens_wide, measured=dict(alive=2746)),
    Job("lens_negative", CORNELL, lambda d: dict(d, lens_rad=float(F(-0.1)))),
    # focal_zero as stated: from the fixture's eye, outside the scene box, every ray runs in the lens plane and misses the box -- nothing alive,
    # nothing accumulated; with the eye INSIDE the box the same rays (d.z exactly 0, all outside the window) hit the side walls
    Job("focal_zero", CORNELL, lambda d: dict(d, focal_length=0.0), dark=True, measured=dict(alive=0, lit=0)),
    Job("focal_zero_eye_inside", CORNELL, lambda d: dict(with_eye(d, z=0.5), focal_length=0.0), outside="all",
        holds=lambda s: (s.primary["rays"]["d"][:, 2] == 0).all()),
    Job("focal_zero_pinhole", CORNELL, lambda d: dict(d, focal_length=0.0, **PINHOLE), dark=True, holds=_holds_focal_zero_pinhole),
    Job("rpp1_pinhole", CORNELL, lambda d: dict(d, **PINHOLE), rays_per_pixel=1, **ODD),
    Job("rpp1_lens", CORNELL, lambda d: d, rays_per_pixel=1, **ODD),
    Job("rpp9_lens_at_edge", CORNELL, lambda d: with_eye(d, x=P(-30)), holds=_holds_rpp9, rays_per_pixel=9),
    # ---- light edges
    Job("light_radius_zero", CORNELL, lambda d: with_lights(d, lambda k, b: _set(b, 9, 0.0)), dark=True),
    Job("light_facing_away", TEAPOT3, lambda d: with_lights(d, lambda k, b: b if k == "shadow" else _negated(b, [3, 4, 5])), holds=_holds_facing_away,
        measured=dict(unblocked=2753, cosy_zero=2489)),
    Job("light_in_the_floor_plane", TEAPOT3, lambda d: with_lights(d, lambda k, b: _set(b, 1, _floor_y(d)), only=0), holds=_holds_in_the_floor_plane),
    Job("light_nonfinite_irradiance", TEAPOT3, lambda d: with_lights(d, _nonfinite(6), only=0), nan_rule=True, holds=_holds_nonfinite),
    Job("light_nonfinite_area", TEAPOT3, lambda d: with_lights(d, _nonfinite(9), only=0), nan_rule=True, holds=_holds_nonfinite),
    Job("light_far", CORNELL, lambda d: with_lights(d, lambda k, b: _set(b, 1, P(19))), dark=True, holds=_holds_light_far),
    # ---- everything at once
    Job("scaled_2p19", CORNELL, lambda d: scaled(d, 2.0 ** 19), outside="none", at_edge=True, holds=_holds_scaled(19), measured=dict(outside=0, lit=764)),
    Job("scaled_2p20", CORNELL, lambda d: scaled(d, 2.0 ** 20), refused=("triangle_bounds",), holds=_holds_scaled(20), measured=dict(lit=764)),
]}
NAMES = sorted(JOBS)


# ---- the oracle's pass of a job, computed once --------------------------------------------------------------------------------------------------
class State:
    pass


_STATES = {}


def state(name, win):
    """the job's scene, seeds, the CPU oracle's finished pass (st) and its checkpoint after the primary segment, with the masks the tests share:
    alive (mint != maxt of the primary rays), outside (alive and refused by the rule).  Read-only for every test."""
    if name not in _STATES:
        s = State()
        s.job, s.win = JOBS[name], win
        s.sc = s.job.scene()
        s.seeds = A.make_seeds(s.sc.total_rays)
        s.st = A.PassState(s.sc, s.seeds)
        cp = {}
        A.run_pass(A.load_oracle(), s.sc, s.st, checkpoints=cp)
        s.primary = cp["primary"]
        r = s.primary["rays"]
        with np.errstate(invalid="ignore"):
            s.alive = ~(r["mint"] == r["maxt"])
        s.outside = s.alive & ~accepted(r["o"], r["d"], win)
        s.n_out = int(s.outside.sum())
        s.lit = int(s.st.pixel[:, :3].any(axis=1).sum())
        _STATES[name] = s
    return _STATES[name]


def sets_of(sc):
    """(name, bounds, slabs per axis, is a triangle set, positions) of every primitive set of a packed scene, in upload order"""
    d, out = sc.d, []
    if d.get("n_spheres", 0):
        out.append(("sphere_bounds", d["sphere_bounds"], d.get("n_slabs", 1), False, None))
    if d.get("n_triangles", 0):
        out.append(("triangle_bounds", d["triangle_bounds"], d.get("n_slabs", 1), True, d["t_pos"]))
    for i, m in enumerate(d.get("meshes", [])):
        out.append((f"mesh{i}", m["bounds"], m["nslabs"], True, m["pos"]))
    return out


def records_sane(pos, win):
    """what k_prepTriangles (csrc/pt_kernels_fused.hip) reports of a triangle set, in float32: every plane-normal component cross(e2, e1) zero or in
    [kDenLo, kDenHi], every vertex and edge component at most 2^21 in magnitude.  The cross product is evaluated in fp64 and narrowed: the test
    scenes' normals are far from the windows' edges or exact."""
    t = np.asarray(pos, dtype=F).reshape(-1, 3, 4)[:, :, :3]
    with np.errstate(all="ignore"):
        e1, e2 = (t[:, 1] - t[:, 0]).astype(F), (t[:, 2] - t[:, 0]).astype(F)
        n = np.abs(np.cross(e2.astype(np.float64), e1.astype(np.float64)).astype(F))
        bad = ~((n == 0) | ((n >= win[0]) & (n <= win[1])))
        big = ~(np.abs(np.concatenate([t[:, 0], e1, e2], axis=1)) <= P(21))
    return not (bad.any() or big.any())


def equal_words(got, want, nan_rule):
    """bit for bit; with nan_rule two words are also equal when both are NaN (an x86 NaN and a gfx950 NaN differ in sign and payload)"""
    g = np.ascontiguousarray(got, dtype=F).reshape(-1).view(np.uint32)
    w = np.ascontiguousarray(want, dtype=F).reshape(-1).view(np.uint32)
    if g.size != w.size:
        return False
    same = g == w
    if nan_rule:
        same |= ((g & 0x7FFFFFFF) > 0x7F800000) & ((w & 0x7FFFFFFF) > 0x7F800000)
    return bool(same.all())
