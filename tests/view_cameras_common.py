"""Shared by tests/test_view_cameras_conditions.py (CPU), tests/test_view_cameras.py and tests/view_cameras_default_child.py (GPU): a catalogue of
view cameras (mirt_view_rays, mirt_render_view) on the stratified random scenes, and the CPU oracle's frame for each.

Scenes: rays_common.scene(stratum) for every stratum of random_scenes_common.STRATA -- the seeds the ray queries use, 37 x 21 x 4; their image
size and lens play no part here.  The `guard` scene is the one scaled by 16: every length below is a multiple of scale(sc), half the largest
extent of the scene box.

Cameras: view_common.View objects made by the named functions of CAMERAS; catalogue(stratum) makes them all.  Every expectation comes from
view_common.view_rays and radiance_common.expected_radiance (oracle/liboracle.so) through frame() below, never from a GPU route, and is cached
per (stratum, camera, bounces).  The same oracle run notes, through expected_radiance's `watch`, which ray ids had a live primary, bounce or
shadow ray that rays_common.guard_accepts refuses: refused_blocks().

  oblique_*     view_common.standard_view at 37 x 21, k = 2: the three models.
  axis_*        right = x, up = y, forward = -z, k = 1 (256 pixels a block), 601 x 4 and 601 x 3, EQUIRECT and FISHEYE with half_angle = pi.  The
                centre column has a == 0 and so d.x == 0 exactly; at 601 x 3 the middle row has b == 0 as well, and the centre pixel of the
                FISHEYE frame r == 0.  The guard refuses a primary ray in 4 of 10 and 5 of 8 blocks.
  mixed_k*      EQUIRECT, an axis-parallel basis turned by pi / 4 about y and scaled by 2^-37: a component of d is below 2^-40 where the
                local direction's is below 1/8, which depends on the column.  Rows [1, +2) of a frame 8 rows high -- the band of latitudes
                without the equator or a pole -- at k = 2 (1000 wide: 64 pixels a block), k = 4 (250 wide: 16) and k = 16 (20 wide: one
                pixel a block).  At k = 2 and 4 the width is no multiple of the block, so the second row does not start one.
  all_refused   the standard EQUIRECT basis scaled by 2^41: one component of every d is above 2^40, the whole frame is the exact kernel's.
  scaled_up     ... by 2^38: no primary ray is refused.  t is in units of |d|, so t_max stays +inf.
  sheared_*     right' = 3 (right + forward / 2), up' = -up / 3 (left-handed), forward as it is: used as given, nothing is normalised.
  rim_*         FISHEYE at 39 x 44, k = 2 (four samples with r == 1.0f exactly, live) and at 17 x 40, k = 4 (two at exactly 1.0f, live, and two
                at nextafter(1.0f), dead), each with half_angle = pi, pi / 2 and 2^-12.
  clipped_*     t_min = 0.4, t_max = 0.9 times scale(sc), the eye CLIPPED_EYE scale(sc) off the centre, where t_max cuts some first hits and
                leaves others; clipped_thin has t_max = nextafter(t_min).  (t_min is a ray word and the dead test's operand, no lower limit.)
  outside       ORTHOGRAPHIC from 3 scale(sc) behind the box's centre along -forward, looking in.
  on_face       EQUIRECT with eye.x the scene box's upper x bound, as the float the bound is.
  k*_*          every_k: EQUIRECT and FISHEYE at 37 x 21 with k = 1, 13 x 7 with k = 4, 7 x 5 with k = 8 and 5 x 3 with k = 16.
  extent_*      65535 x 1 at k = 1 (mirt_view_rays only) and rows [65530, +5) of 1 x 65535 at k = 2.

SHARES, measured on the oracle when the cameras were chosen (bounces 2, seeds a10_pass.make_seeds(n_rays)), per (stratum, camera) the GPU
renders: the share of pixels with w > 0, of pixels not black after the tone map, of seeds that advance.
  camera              single_cell       staged            unstaged          many_sets         open              guard
  oblique_ortho       1.00 0.96 1.00    1.00 0.99 1.00    1.00 1.00 1.00    1.00 0.99 1.00    0.38 0.13 0.34    1.00 0.99 1.00
  oblique_equirect    0.99 0.70 0.97    1.00 0.92 0.99    0.91 0.91 0.86    0.97 0.96 0.92    0.94 0.16 0.90    1.00 0.92 0.99
  oblique_fisheye     0.82 0.61 0.78    0.82 0.77 0.78    0.82 0.82 0.78    0.82 0.80 0.78    0.76 0.10 0.71    0.82 0.77 0.78
  axis_equirect_601x4 0.98 0.42 0.97    1.00 0.71 1.00    0.88 0.87 0.87    0.95 0.80 0.95    -                 1.00 0.64 1.00
  axis_equirect_601x3 1.00 0.43 1.00    1.00 0.68 1.00    0.92 0.91 0.92    0.95 0.77 0.95    -                 1.00 0.66 1.00
  axis_fisheye_601x4  0.76 0.29 0.76    0.81 0.45 0.81    0.39 0.39 0.38    0.59 0.50 0.58    -                 0.81 0.56 0.81
  axis_fisheye_601x3  0.79 0.34 0.79    0.83 0.49 0.83    0.47 0.46 0.47    0.63 0.53 0.63    -                 0.83 0.56 0.83
  mixed_k2            0.95 0.70 0.94    1.00 0.90 1.00    0.89 0.89 0.88    0.96 0.94 0.94    -                 1.00 0.88 1.00
  mixed_k4            0.97 0.82 0.94    1.00 0.99 1.00    0.93 0.92 0.89    0.98 0.98 0.94    -                 1.00 0.98 1.00
  mixed_k16           1.00 0.93 0.95    1.00 1.00 1.00    1.00 0.97 0.89    1.00 1.00 0.94    -                 1.00 1.00 1.00
  all_refused         0.99 0.70 0.97    1.00 0.92 0.99    -                 -                 -                 1.00 0.92 0.99
  scaled_up           0.99 0.70 0.97    1.00 0.92 0.99    -                 -                 -                 1.00 0.92 0.99
  sheared_ortho       0.46 0.45 0.44    0.46 0.45 0.44    -                 -                 -                 0.46 0.46 0.44
  sheared_equirect    1.00 0.78 0.98    1.00 0.98 1.00    -                 -                 -                 1.00 0.96 1.00
  sheared_fisheye     0.82 0.74 0.78    0.82 0.81 0.78    -                 -                 -                 0.82 0.77 0.78
  rim_39x44_pi        0.78 0.54 0.73    0.81 0.70 0.78    -                 -                 -                 0.81 0.77 0.78
  rim_39x44_half_pi   0.81 0.62 0.77    0.81 0.77 0.77    -                 -                 -                 0.81 0.75 0.77
  rim_39x44_tiny      0.81 0.81 0.79    0.81 0.76 0.79    -                 -                 -                 0.81 0.81 0.79
  rim_17x40_pi        0.82 0.72 0.73    0.83 0.80 0.78    -                 -                 -                 0.83 0.82 0.78
  rim_17x40_half_pi   0.83 0.72 0.77    0.83 0.82 0.77    -                 -                 -                 0.83 0.81 0.77
  rim_17x40_tiny      0.83 0.83 0.79    0.83 0.83 0.79    -                 -                 -                 0.83 0.83 0.79
  clipped_equirect    0.56 0.53 0.50    0.48 0.47 0.43    -                 -                 -                 0.49 0.48 0.42
  clipped_ortho       0.48 0.41 0.40    0.37 0.35 0.31    -                 -                 -                 0.42 0.41 0.35
  clipped_thin        0.44 0.20 0.36    0.82 0.77 0.78    -                 -                 -                 0.54 0.45 0.41
  outside             1.00 0.94 1.00    1.00 0.99 1.00    -                 -                 -                 1.00 0.99 1.00
  on_face             0.47 0.45 0.43    0.45 0.45 0.41    -                 -                 -                 0.45 0.45 0.41
  k1_equirect         0.98 0.41 0.97    1.00 0.71 0.98    0.88 0.87 0.85    0.95 0.79 0.92    -                 -
  k1_fisheye          0.79 0.43 0.78    0.79 0.62 0.78    0.79 0.79 0.78    0.79 0.66 0.78    -                 -
  k4_equirect         1.00 0.92 0.97    1.00 0.99 0.98    0.96 0.96 0.86    1.00 0.99 0.92    -                 -
  k4_fisheye          0.91 0.79 0.78    0.91 0.89 0.78    0.91 0.91 0.78    0.91 0.90 0.78    -                 -
  k8_equirect         1.00 0.97 0.97    1.00 1.00 0.98    1.00 1.00 0.86    1.00 1.00 0.92    -                 -
  k8_fisheye          1.00 0.89 0.78    1.00 0.94 0.78    1.00 1.00 0.78    1.00 0.97 0.78    -                 -
  k16_equirect        1.00 1.00 0.97    1.00 1.00 0.98    1.00 1.00 0.85    1.00 1.00 0.92    -                 -
  k16_fisheye         1.00 0.87 0.78    1.00 1.00 0.78    1.00 1.00 0.78    1.00 1.00 0.78    -                 -
  extent_tall         1.00 0.60 1.00    1.00 1.00 1.00    -                 -                 -                 1.00 1.00 1.00
Blocks of 256 ray ids with a refused PRIMARY ray: axis_*_601x4 4 of 10, axis_*_601x3 5 of 8, mixed_k2 14 of 32, mixed_k4 15 of 32, mixed_k16 24
of 40, on every enclosed stratum; all_refused 13 of 13; every other camera 0.  Bounce and shadow rays add blocks on `guard` only.
Floors (tests/test_view_cameras_conditions.py): w > 0 in 0.10 of the pixels, 0.25 outside `open` and clipped_*; 0.05 non-black and 0.05 of the
seeds outside `open` and clipped_*.

The wrong restatements (MISTAKES): view_rays_as(view, mistake) is view_common.view_rays with ONE deliberate mistake in it; the conditions show
that each edge camera tells the definition from its nearest mistake in at least one word, without a GPU."""
import numpy as np

import a10_pass as A
import radiance_common as RC
import rays_common as R
import view_common as V
from random_scenes_common import ENCLOSED, STRATA  # noqa: F401  (re-exported for the tests)

f32 = np.float32
BOUNCES = 2
TWO_M12 = 2.0 ** -12

_CACHE = {}


# ---- the scene's box ------------------------------------------------------------------------------------------------------------------------------
def box(sc):
    b = np.asarray(sc.bounds, np.float64)
    return b[0:3], b[4:7]


def scale(sc):
    lo, hi = box(sc)
    return float((hi - lo).max() / 2)


def centre(sc):
    lo, hi = box(sc)
    return (lo + hi) / 2


# ---- the cameras ----------------------------------------------------------------------------------------------------------------------------------
def oblique(sc, model, width=37, height=21, k=2, **kw):
    kw.setdefault("tone", 1.0 / (k * k))
    return V.standard_view(sc, model, width=width, height=height, k=k, **kw)


def axis(sc, model, height):
    return V.View(model, 601, height, 1, centre(sc), (1, 0, 0), (0, 1, 0), (0, 0, -1), half_angle=float(V.PI), tone=1.0)


def mixed(sc, k, width, height, exponent, rows=None):
    """EQUIRECT; the basis x, y, -z turned by pi / 4 about y and scaled by 2^exponent"""
    c = float(f32(np.sqrt(0.5))) * 2.0 ** exponent
    s = 2.0 ** exponent
    v = V.View("equirect", width, height, k, centre(sc), (c, 0, -c), (0, s, 0), (-c, 0, -c), tone=1.0 / (k * k))
    return v if rows is None else v.tile(*rows)


def scaled(sc, model, exponent, **kw):
    v = oblique(sc, model, **kw)
    m = 2.0 ** exponent
    return v.with_(right=v.right * f32(m), up=v.up * f32(m), forward=v.forward * f32(m))


def sheared(sc, model):
    v = oblique(sc, model)
    right, up, fwd = (np.asarray(x, np.float64) for x in (v.right, v.up, v.forward))
    return v.with_(right=(3.0 * (right + 0.5 * fwd)).astype(f32), up=(-up / 3.0).astype(f32))


def rim(sc, width, height, k, half_angle):
    return oblique(sc, "fisheye", width=width, height=height, k=k).with_(half_angle=half_angle)


# from the box's centre every first hit of these scenes is nearer than 0.4 scale(sc); from here t_max = 0.9 scale(sc) cuts a quarter to a half
CLIPPED_EYE = (0.5, 0.3, 0.6)


def clipped(sc, model, thin=False):
    t_min = f32(0.4 * scale(sc))
    t_max = np.nextafter(t_min, f32(np.inf)) if thin else f32(0.9 * scale(sc))
    # (thin: from the centre, where every first hit is nearer than t_min -- the ray is live, one ulp long in [t_min, t_max), and still hits)
    eye = centre(sc) + (0.0 if thin else scale(sc)) * np.array(CLIPPED_EYE)
    return oblique(sc, model, t_min=float(t_min), t_max=float(t_max)).with_(eye=eye.astype(f32))


def outside(sc):
    v = oblique(sc, "ortho")
    eye = centre(sc) - 3.0 * scale(sc) * np.asarray(v.forward, np.float64)
    return v.with_(eye=eye.astype(f32))


def on_face(sc):
    v = oblique(sc, "equirect")
    eye = v.eye.copy()
    eye[0] = f32(sc.bounds[4])          # the bound's own float
    return v.with_(eye=eye)


EVERY_K = ((37, 21, 1), (13, 7, 4), (7, 5, 8), (5, 3, 16))
RIMS = ((39, 44, 2), (17, 40, 4))
RIM_ANGLES = (("pi", float(V.PI)), ("half_pi", float(V.HALF_PI)), ("tiny", TWO_M12))
# what the rim frames hold: (samples with r == 1.0f exactly, samples with r == nextafter(1.0f)) -- the first live, the second dead
RIM_COUNTS = {(39, 44, 2): (4, 0), (17, 40, 4): (2, 2)}

CAMERAS = {}
for _m in V.MODELS:
    CAMERAS[f"oblique_{_m}"] = lambda sc, m=_m: oblique(sc, m)
for _m in ("equirect", "fisheye"):
    for _h in (4, 3):
        CAMERAS[f"axis_{_m}_601x{_h}"] = lambda sc, m=_m, h=_h: axis(sc, m, h)
CAMERAS["mixed_k2"] = lambda sc: mixed(sc, 2, 1000, 8, -37, rows=(1, 2))
CAMERAS["mixed_k4"] = lambda sc: mixed(sc, 4, 250, 8, -37, rows=(1, 2))
CAMERAS["mixed_k16"] = lambda sc: mixed(sc, 16, 20, 8, -37, rows=(1, 2))
CAMERAS["all_refused"] = lambda sc: scaled(sc, "equirect", 41)
CAMERAS["scaled_up"] = lambda sc: scaled(sc, "equirect", 38)
for _m in V.MODELS:
    CAMERAS[f"sheared_{_m}"] = lambda sc, m=_m: sheared(sc, m)
for _w, _h, _k in RIMS:
    for _tag, _ang in RIM_ANGLES:
        CAMERAS[f"rim_{_w}x{_h}_{_tag}"] = lambda sc, w=_w, h=_h, k=_k, a=_ang: rim(sc, w, h, k, a)
CAMERAS["clipped_equirect"] = lambda sc: clipped(sc, "equirect")
CAMERAS["clipped_ortho"] = lambda sc: clipped(sc, "ortho")
CAMERAS["clipped_thin"] = lambda sc: clipped(sc, "fisheye", thin=True)
CAMERAS["outside"] = outside
CAMERAS["on_face"] = on_face
for _w, _h, _k in EVERY_K:
    for _m in ("equirect", "fisheye"):
        CAMERAS[f"k{_k}_{_m}"] = lambda sc, m=_m, w=_w, h=_h, k=_k: oblique(sc, m, width=w, height=h, k=k)
CAMERAS["extent_tall"] = lambda sc: oblique(sc, "equirect", width=1, height=65535, k=2).tile(65530, 5)
# mirt_view_rays only: 65535 rays are too many for an oracle frame in a quick test
RAYS_ONLY = {"extent_wide": lambda sc: oblique(sc, "fisheye", width=65535, height=1, k=1, t_min=0.03125, t_max=1000.0)}

OBLIQUE = tuple(n for n in CAMERAS if n.startswith("oblique_"))
AXIS = tuple(n for n in CAMERAS if n.startswith("axis_"))
MIXED_K = tuple(n for n in CAMERAS if n.startswith("mixed_"))
MIXED = AXIS + MIXED_K
EVERY_K_NAMES = tuple(n for n in CAMERAS if n[0] == "k" and n[1].isdigit())
RIM = tuple(n for n in CAMERAS if n.startswith("rim_"))
CLIPPED = tuple(n for n in CAMERAS if n.startswith("clipped_"))
EDGE = (("all_refused", "scaled_up") + tuple(n for n in CAMERAS if n.startswith("sheared_")) + RIM + CLIPPED + ("outside", "on_face", "extent_tall"))
# where each group runs on the GPU (tests/test_view_cameras.py)
EDGE_STRATA = ("staged", "single_cell", "guard")
EVERY_K_STRATA = ("single_cell", "staged", "unstaged", "many_sets")


def used_on_the_gpu():
    """every (stratum, camera) tests/test_view_cameras.py renders"""
    out = [(s, n) for s in STRATA for n in OBLIQUE]
    out += [(s, n) for s in EVERY_K_STRATA for n in EVERY_K_NAMES]
    out += [(s, n) for s in EDGE_STRATA for n in EDGE]
    out += [(s, n) for s in ENCLOSED for n in MIXED]
    return out


def view(stratum, name):
    key = ("view", stratum, name)
    if key not in _CACHE:
        _CACHE[key] = (CAMERAS.get(name) or RAYS_ONLY[name])(R.scene(stratum))
    return _CACHE[key]


def seeds_of(n):
    return A.make_seeds(n)


# ---- the oracle's frame ------------------------------------------------------------------------------------------------------------------------------
class Frame:
    """the oracle's answer for one (scene, view, seeds, bounces): seeds [n_rays], acc [n_rays, 4] (the per-ray accumulators before the fold),
    sums [n_pixels, 4] and pixel [n_pixels, 4] from +0, and per ray whether the guard refuses its primary ray / any of its rays; read-only"""

    def __init__(self, sc, v, seeds, bounces):
        rays = V.view_rays(v)
        n = len(rays)
        self.view = v
        self.primary = R.live(rays) & ~R.guard_accepts(rays)
        bad = self.primary.copy()

        def watch(kind, buf):
            r = np.zeros((n, 8), f32)
            r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = buf["o"][:n], buf["mint"][:n], buf["d"][:n], buf["maxt"][:n]
            bad[:] |= R.live(r) & ~R.guard_accepts(r)
        self.acc, self.seeds = RC.expected_radiance(sc, rays, seeds, 1, bounces, watch=watch)
        self.refused = bad
        self.sums = V.fold(self.acc, v.rpp)
        self.pixel = V.tone_rgba8(self.sums, v.tone)
        for a in (self.acc, self.seeds, self.sums, self.pixel, self.primary, self.refused):
            a.setflags(write=False)

    def triple(self, carry=None, tone=None):
        """(seeds, sums, pixel) as view_common.expected_view returns them, from +0 or from `carry`, with the view's tone or another"""
        if carry is None and tone is None:
            return self.seeds, self.sums, self.pixel
        sums = V.fold(self.acc, self.view.rpp, carry)
        return self.seeds, sums, V.tone_rgba8(sums, self.view.tone if tone is None else tone)

    def rows(self, row0, nrows):
        """the triple of rows [row0, +nrows) of the frame's own rows (tile-local), from +0"""
        w, rpp = self.view.width, self.view.rpp
        px, ry = slice(row0 * w, (row0 + nrows) * w), slice(row0 * w * rpp, (row0 + nrows) * w * rpp)
        return self.seeds[ry], self.sums[px], self.pixel[px]


def frame(stratum, name, bounces=BOUNCES):
    """the oracle's Frame of a catalogue camera with seeds_of(n_rays), computed once and shared"""
    key = ("frame", stratum, name, bounces)
    if key not in _CACHE:
        v = view(stratum, name)
        _CACHE[key] = Frame(R.scene(stratum), v, seeds_of(v.n_rays), bounces)
    return _CACHE[key]


def blocks_of(flags):
    """bool per ray id -> the blocks of 256 ray ids that hold a set one"""
    return np.unique(np.flatnonzero(flags) // 256)


def refused_blocks(sc, v, seeds, bounces):
    """the blocks of 256 ray ids that hold any live primary, bounce or shadow ray rays_common.guard_accepts refuses"""
    return blocks_of(Frame(sc, v, seeds, bounces).refused)


def clean_tile(fr):
    """(row0, nrows) among the frame's own rows, row0 > 0: the lowest rows of it whose first block of 256 ray ids holds no refused ray"""
    v = fr.view
    per = v.width * v.rpp
    for row0 in range(1, v.rows):
        if not fr.refused[row0 * per:row0 * per + 256].any():
            return row0, v.rows - row0
    raise AssertionError("every row of the frame starts with a refused block")


def n_blocks(v):
    return -(-v.n_rays // 256)


def shares(fr):
    """(share of pixels with w > 0, share of pixels not black after the tone map, share of seeds that advance)"""
    return (float((fr.sums[:, 3] > 0).mean()), float((fr.pixel[:, 0:3] != 0).any(axis=1).mean()),
            float((fr.seeds != seeds_of(len(fr.seeds))).mean()))


# ---- the wrong restatements ---------------------------------------------------------------------------------------------------------------------------
MISTAKES = ("r_below_1", "local_row", "q_unguarded", "normalised_basis", "t_min_ignored")


def view_rays_as(v, mistake=None):
    """view_common.view_rays with one deliberate mistake (None: none, the same words):
      r_below_1         a FISHEYE sample is live when r < 1, not r <= 1
      local_row         positions from the tile-local row, not the global y
      q_unguarded       q = sa / r at r == 0 as well (0 / 0).  (q = 1 there is NOT a mistake an input can show: lx = a * q and ly = b * q with
                        a == b == +0, so every finite q gives the same +0 -- test_q_at_r_0_matters_only_when_it_is_not_finite)
      normalised_basis  right, up and forward normalised before use
      t_min_ignored     every live ray starts at mint = 0"""
    assert mistake is None or mistake in MISTAKES, mistake
    if mistake == "local_row":
        w = v.tile(0, v.rows)
        return V.view_rays(w)
    if mistake == "normalised_basis":
        def unit(x):
            x = np.asarray(x, np.float64)
            return (x / np.linalg.norm(x)).astype(f32)
        return V.view_rays(v.with_(right=unit(v.right), up=unit(v.up), forward=unit(v.forward)))
    if mistake == "t_min_ignored":
        return V.view_rays(v.with_(t_min=0.0))
    rays = V.view_rays(v)
    if mistake is None or v.model != V.FISHEYE:
        return rays
    a, b = window(v)
    r = np.sqrt(a * a + b * b)
    if mistake == "r_below_1":
        on = r == f32(1.0)
        rays[on, 4:7] = v.forward
        rays[on, 3] = 0.0
        rays[on, 7] = 0.0
    elif mistake == "q_unguarded":
        rays[r == 0, 4:7] = np.nan          # (right.c * (0 * NaN) + up.c * (0 * NaN)) + forward.c * ca
    return rays


def window(v):
    """(a, b) float32 per ray of the tile: the sample's position in the window, as view_common.view_rays computes it"""
    k, W = v.k, v.width
    ys, xs, sy, sx = (g.reshape(-1) for g in np.meshgrid(np.arange(v.row0, v.row0 + v.rows), np.arange(W), np.arange(k), np.arange(k), indexing="ij"))
    ik = f32(1.0) / f32(k)
    fx = xs.astype(f32) + (sx.astype(f32) + f32(0.5)) * ik
    fy = ys.astype(f32) + (sy.astype(f32) + f32(0.5)) * ik
    u, w = fx / f32(W), fy / f32(v.height)
    return (u + u) - f32(1.0), f32(1.0) - (w + w)


def fold_pairwise(acc, rpp, carry=None):
    """the WRONG fold: a pixel's accumulators summed as a balanced tree, then added to +0 or the carry"""
    a = np.ascontiguousarray(acc, f32).reshape(-1, rpp, 4)
    while a.shape[1] > 1:
        a = (a[:, 0::2, :] + a[:, 1::2, :]).astype(f32)
    s = np.zeros((a.shape[0], 4), f32) if carry is None else np.array(carry, f32).reshape(-1, 4)
    return (s + a[:, 0, :]).astype(f32)
