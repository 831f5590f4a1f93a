"""Generated cameras for the single-frame kernels (csrc/pt_kernels_frame.hip): the camera generator, the jobs and the guards of
tests/test_frame_cameras.py.  Every other frame test takes the camera block of a committed fixture: Camera.set (A07 code.js:55-71) -- U, V, W the
identity, the eye outside the box at centre + diag * z, every ray's d.z < 0.

page_camera restates Camera.set followed by Camera.rotate (A04 / A07 code.js:73-99, the pages' Rotate button) in float64 and narrows where
toFloat32Array narrows; tests/golden/frame_rot_*.npz (oracle/gen/gen_golden_frame.py ROT_CASES: the reference's own host code run with its own
rotate) hold four such camera blocks and the reference's frames, so the restatement is checked against the page, bit for bit.  CAMERAS adds the
views the page cannot reach: the eye inside the box, on a grid vertex, on a face, along y, a rolled / sheared / mirrored basis, a zero window, far
eyes, and the degenerate blocks (DEGENERATE).

Which lanes share a wave (checked against the code): k_a04_meshTrace, k_a07_meshTrace, k_a07_molTrace and k_frame_fused launch blocks of (32, 8)
(grid2 / launch_frame_fused_t), the linear thread id is 32 * threadIdx.y + threadIdx.x, so a wave is 32 x 2 pixels at x = 0 mod 32, y = 0 mod 2.
k_frame_aa_lanes: lane = pixel * AA * AA + sample, a wave covers an 8 x 8 tile of the FINE frame for AA 2 (4 x 4 pixels of 2 x 2 samples) and a
21 x 3 tile for AA 3 (7 x 1 pixels of 3 x 3 samples), at multiples of those sizes (AaWave, launch_frame_aa_t).

Why the DEGENERATE cameras (zero_W, zero_basis, nan_eye, inf_eye, huge_eye) may run on the device -- every table and record index stays in range
whatever the ray holds:
  * the pixel / ray index is cols * row + col with col < cols, row < rows from cam[14], cam[15], which no camera here changes;
  * clip_to / inter_aabb (pt_device.hpp) only compare and select floats; a NaN quotient loses every cl_max / cl_min or compares false; they index
    nothing;
  * axis_setup: slab = f2i(...) is v_cvt_i32_f32 (NaN -> 0, +-inf and 1e30 saturate), then `slab < 0 -> 0` and `(uint32_t)slab >= n -> n - 1`:
    0 <= slab <= n - 1 for every input; dslab, limit are +1, n or -1, -1 (a NaN d compares `d >= 0` false: backwards);
  * both walks (k_a07_meshTrace, frame_stage_grid) read slab_size[cell], slab_size[cell + 1] with cell = z * n * n + y * n + x built from the three
    slabs.  A step moves exactly ONE axis' slab by its dslab and leaves the loop before the next read when that slab equals its limit, so every slab
    that forms a cell index is in 0 .. n - 1; if t equals neither ax.tnext nor ay.tnext (NaN included) the z axis steps.  Each step brings one axis
    nearer its limit, so at most 3 n cells are opened: the walk ends whatever dt and tnext are (inf, NaN);
  * inside a cell i runs from slab_size[cell] to slab_size[cell + 1]: `++i`, or `i += 16` only when end - i >= 16; the group sphere read is
    [i / 16] behind the records, in range for any in-range i; prims[i], normals[3 * champ_i] with champ_i one of those i; tests that see NaN reject
    (`t > cmin` is false) and would at worst keep an in-range i;
  * the Assign04 loop runs i over 0 .. t_size - 1 whatever the ray is; mcolor[m] is guarded by m < ncolors;
  * k_a01_raytrace has its own range check and indexes nothing but the pixel.
So these frames are ordinary launches whose floats are odd; what they compute is compared with the oracle like any other frame.

Observed on the oracle (the guards below assert the bounds, these are the figures): lit share of the orbit / roll / shear / mirror / above /
below / telephoto frames over all jobs and both sizes: lowest 3.5 % (soup_n1 tele_30 at 67 x 45; lowest orbit frame 4.8 %, parliament orbit_180
at 160 x 100), highest 47.8 % (lattice, sheared); far_4 lights 5 to 156 pixels (0.17 % to 0.97 %), far_8 1 to 36 pixels (0.03 % to 0.30 %), and
in the Assign07 jobs they leave 98.4 % to 99.9 % of the rays dead (Assign04's initTrace does not clip: no ray of such a job is ever dead);
inside and at_vertex_* leave no ray dead in any job; from inside the teapot `inside` lights 3.8 % and at_vertex_px 5.9 % while at_vertex_mz
sees back faces only.  Each Assign07 job reaches all six direction signs with whole lit waves (z forwards from orbit_89 on, y by from_above /
from_below and by the upper and lower halves of most frames).
Tiny components (0 < |d_k| < 2^-40) exist in the orbit_90 / 180 / 270 frames at 67 x 45 only: Math.cos / Math.sin leave 6.1e-17 (1.2e-16, 1.8e-16)
in W and U, and only the CENTRE column of an odd-width frame has sx == 0, where that component is all of d_k; an even width has no such column.
"""
import math

import numpy as np

import frame_pass as F
from test_frames import _random_mesh_job, fixture, resized

SIZES = ((67, 45), (160, 100))
ORBIT_ANGLES = (0, 1, 45, 89, 90, 91, 135, 180, 225, 270, 359)
FAR = (4, 8)                                   # of the orbit distance.  Chosen on the CPU: these objects are a pixel wide from 30 distances, and from 9 on
                                               # some 67 x 45 frame of some job is black (the guard: every far frame lights a pixel); tele_30 goes farther
DEGENERATE = ("zero_W", "zero_basis", "nan_eye", "inf_eye", "huge_eye")
SOUP_SEEDS = {0: 100, 1: 122, 2: 124}          # test_frames._random_mesh_job draws T = 2500 for these seeds
FOV = 60


# ---- the page's camera --------------------------------------------------------------------------------------------------------------------------
def box64(job):
    """(min, max) as the page holds them: doubles -- the molecule reader's own (pdb) or the float32 bounds of the job"""
    if "pdb" in job:
        return np.asarray(job["pdb"]["min"], np.float64), np.asarray(job["pdb"]["max"], np.float64)
    b = np.asarray(job["bounds"], np.float32).astype(np.float64)
    return b[:3], b[4:7]


def centre_diag(job):
    lo, hi = box64(job)
    c = [(lo[k] + hi[k]) / 2 for k in range(3)]                          # Bounds.center, lib/utilities.js:395-401
    e = [hi[k] - lo[k] for k in range(3)]
    return c, math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])         # Bounds.diagonal, :402-408


def block(job, eye, U=(1.0, 0.0, 0.0), V=(0.0, 1.0, 0.0), W=(0.0, 0.0, 1.0)):
    """toFloat32Array (A07 code.js:104-112) of a camera with Camera.set's window for the job's size"""
    cols, rows = int(job["width"]), int(job["height"])
    height = 2.0 * math.tan(0.5 * FOV * math.pi / 180.0)
    width = height * (cols / rows)
    return [float(np.float32(v)) for v in (*eye, *U, *V, *W, width, height, cols, rows)]


def page_camera(job, angle=None):
    """Camera.set(bounds, cols, rows) on a defaultInit camera and, for an angle (whole degrees), Camera.rotate(bounds, angle)"""
    c, diag = centre_diag(job)
    eye = [c[0], c[1], c[2] + diag]
    U, V, W = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
    if angle is not None:
        rad = angle * math.pi / 180.0
        eye = [c[0] + math.sin(rad) * diag, c[1], c[2] + math.cos(rad) * diag]
        W = [eye[0] - c[0], eye[1] - c[1], eye[2] - c[2]]
        ln = math.sqrt(W[0] * W[0] + W[1] * W[1] + W[2] * W[2])
        W = [W[0] / ln, W[1] / ln, W[2] / ln]
        U = [V[1] * W[2] - V[2] * W[1], V[2] * W[0] - V[0] * W[2], V[0] * W[1] - V[1] * W[0]]   # V.cross(W)
    return block(job, eye, U, V, W)


# ---- the other cameras ----------------------------------------------------------------------------------------------------------------------------
def _vertex(job):
    """a vertex of the job's own grid (an Assign04 job has none: n = 2, the middle of the box) as axis_setup forms cell faces: fma(k, delta, lo) in
    float32 with delta = (hi - lo) / n; None where the grid has no vertex inside the box (n = 1)"""
    n = int(job.get("n_slabs", 2))
    if n < 2:
        return None
    b = np.asarray(job["bounds"], np.float32)
    lo, hi = b[:3], b[4:7]
    delta = (hi - lo) / np.float32(n)
    k = (n // 2, (n + 1) // 2, n // 2)
    return [float(np.float32(float(k[a]) * float(delta[a]) + float(lo[a]))) for a in range(3)]


def _at_vertex_mz(job):
    v = _vertex(job)
    return None if v is None else block(job, v)


def _at_vertex_px(job):
    v = _vertex(job)
    return None if v is None else block(job, v, U=(0.0, 0.0, 1.0), W=(-1.0, 0.0, 0.0))


def _on_face(job, side):
    c, _ = centre_diag(job)
    b = np.asarray(job["bounds"], np.float32)
    return block(job, [c[0], c[1], float(b[6] if side else b[2])])


def _along_y(job, sign):
    """from above (sign +1): eye = centre + diag * y, W = +y, V = -z; from below: all three negated.  U = V x W = +x in both"""
    c, diag = centre_diag(job)
    return block(job, [c[0], c[1] + sign * diag, c[2]], V=(0.0, 0.0, -float(sign)), W=(0.0, float(sign), 0.0))


def _rolled(job, degrees=33):
    c, diag = centre_diag(job)
    co, si = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    return block(job, [c[0], c[1], c[2] + diag], U=(co, si, 0.0), V=(-si, co, 0.0))


def _far(job, k):
    c, diag = centre_diag(job)
    return block(job, [c[0], c[1], c[2] + k * diag])


def _tele(job, k=30):
    """k orbit distances away with the window narrowed k times: the frame of orbit_0 in nearly parallel rays"""
    cam = _far(job, k)
    cam[12], cam[13] = float(np.float32(cam[12] / k)), float(np.float32(cam[13] / k))
    return cam


def _with(cam, **at):
    cam = list(cam)
    for k, v in at.items():
        cam[int(k[1:])] = v
    return cam


def _cameras():
    cams = [(f"orbit_{a}", (lambda job, a=a: page_camera(job, a))) for a in ORBIT_ANGLES]
    cams += [
        ("inside", lambda job: block(job, [centre_diag(job)[0][0], centre_diag(job)[0][1], centre_diag(job)[0][2] + 0.1 * centre_diag(job)[1]])),
        ("at_vertex_mz", _at_vertex_mz),
        ("at_vertex_px", _at_vertex_px),
        ("on_max_face_in", lambda job: _on_face(job, 1)),
        ("on_min_face_out", lambda job: _on_face(job, 0)),
        ("from_above", lambda job: _along_y(job, +1)),
        ("from_below", lambda job: _along_y(job, -1)),
        ("rolled_33", _rolled),
        ("sheared", lambda job: block(job, page_camera(job)[:3], U=(2.5, 0.3, 0.0), V=(0.0, 0.4, 0.0), W=(0.2, 0.0, 3.0))),
        ("mirrored", lambda job: block(job, page_camera(job)[:3], U=(-1.0, 0.0, 0.0))),
        ("zero_window", lambda job: _with(page_camera(job), _12=0.0, _13=0.0)),
    ]
    cams += [(f"far_{k}", (lambda job, k=k: _far(job, k))) for k in FAR]
    cams.append(("tele_30", _tele))
    cams += [
        ("zero_W", lambda job: _with(page_camera(job), _9=0.0, _10=0.0, _11=0.0)),
        ("zero_basis", lambda job: _with(page_camera(job), **{f"_{i}": 0.0 for i in range(3, 12)})),
        ("nan_eye", lambda job: _with(page_camera(job), _1=float("nan"))),
        ("inf_eye", lambda job: _with(page_camera(job), _2=float("inf"))),
        ("huge_eye", lambda job: _with(page_camera(job), _0=1e30)),
    ]
    return cams


CAMERAS = _cameras()                           # [(name, job -> cam[16] | None where the job has no such camera)]
CAMERA = dict(CAMERAS)
LIT_2_PERCENT = tuple(n for n, _ in CAMERAS if n.startswith("orbit_") or n in ("rolled_33", "sheared", "mirrored", "from_above", "from_below", "tele_30"))
NO_DEAD_RAY = ("inside", "at_vertex_mz", "at_vertex_px")
PARLIAMENT_CAMERAS = ("orbit_45", "orbit_180", "orbit_270")   # its 9144 triangles make the host side slow


# ---- jobs -----------------------------------------------------------------------------------------------------------------------------------------
FIXTURE_JOBS = ("frame_a07_teapot_n2_160x120", "frame_a07_teapot_n8_160x120", "frame_a04_teapot_160x120", "frame_a07_own_octahedra_n3_96x64",
                "frame_a07_mol_c60_n4_160x120", "frame_a07_own_mol_lattice_n6_96x64")
JOBS = FIXTURE_JOBS + ("soup_n0", "soup_n1", "soup_n2", "both_models", "frame_a07_parliament_n16_160x120")
REF_JOBS = ("frame_a04_teapot_160x120", "frame_a07_teapot_n8_160x120", "frame_a07_mol_c60_n4_160x120")   # oracle against the compiled reference

_jobs, _frames = {}, {}


def _arrays(d):
    """the job with its lists as arrays of the types the packers ask for, made once: np.asarray of a long list is what a frame's host side costs"""
    kinds = dict(pos=np.float32, normal=np.float32, atoms=np.float32, mcolor=np.float32, mindex=np.uint32, slab_size=np.uint32)
    out = {k: (np.asarray(v, kinds[k]) if k in kinds else v) for k, v in d.items()}
    if isinstance(out.get("mol"), dict):
        out["mol"] = {k: (np.asarray(v, kinds[k]) if k in kinds else v) for k, v in out["mol"].items()}
    return out


def job_named(name):
    if name not in _jobs:
        if name.startswith("soup_n"):
            n = int(name[len("soup_n"):])
            _, a04 = fixture("frame_a04_parliament_96x64")
            _, a07 = fixture("frame_a07_parliament_n16_160x120")
            d = _random_mesh_job(a04, a07, SOUP_SEEDS[n], n)
            assert d["t_size"] == 2500
        elif name == "both_models":
            from test_random_molecules import BOTH_SEEDS, both_models_job
            d = both_models_job(BOTH_SEEDS[0])[0]
        else:
            d = fixture(name)[1]
        _jobs[name] = _arrays(d)
    return _jobs[name]


def cameras_of(name):
    return [c for c, _ in CAMERAS if name != "frame_a07_parliament_n16_160x120" or c in PARLIAMENT_CAMERAS]


def with_camera(job, camera, size):
    """the job at `size` under the named camera (or a cam[16] itself); None where the job has no such camera"""
    d = resized(job, *size)
    cam = CAMERA[camera](d) if isinstance(camera, str) else camera
    return None if cam is None else dict(d, cam=cam)


def expected(name, camera, size):
    """(job, oracle pixels, oracle rays) of a named job under a named camera, computed once and read-only; None where there is no such camera"""
    key = (name, camera, tuple(size))
    if key not in _frames:
        d = with_camera(job_named(name), camera, size)
        if d is None:
            _frames[key] = None
        else:
            fr = F.Frame(d)
            px, rays = F.run_frame_both("oracle", fr) if fr.both is not None else F.run_frame("oracle", fr)
            px.flags.writeable = False
            rays.flags.writeable = False
            _frames[key] = (d, px, rays)
    return _frames[key]


# ---- what a frame reached (on the oracle's frame) -------------------------------------------------------------------------------------------------
def lit(px):
    return px[:, :3].max(axis=1) > 0


def dead(rays):
    return rays["mint"] == rays["maxt"]


def uniform_lit_tiles(px, rays, size, tile=(32, 2)):
    """{(axis, sign)}: the signs of d that a whole wave tile (its pixels inside the image) shares while one of its pixels is lit"""
    w, h = size
    tw, th = tile
    d = rays["d"][:, :3].reshape(h, w, 3)
    on = lit(px).reshape(h, w)
    out = set()
    for y in range(0, h, th):
        for x in range(0, w, tw):
            if on[y:y + th, x:x + tw].any():
                t = d[y:y + th, x:x + tw].reshape(-1, 3)
                out |= {(k, +1) for k in range(3) if (t[:, k] > 0).all()} | {(k, -1) for k in range(3) if (t[:, k] < 0).all()}
    return out


def tiny_components(rays):
    a = np.abs(rays["d"][:, :3])
    return int(((a > 0) & (a < 2.0 ** -40)).sum())


# ---- Assign01 --------------------------------------------------------------------------------------------------------------------------------------
A01_RADII = (0.25, 1.0, 6.0)                  # 0.25: inside the sphere c = (0, 0, 1), r = 0.5 -- the second root; 6: (1 - t) * 255 < 0, the byte wraps
A01_ANGLES = (0, 90, 180)


def a01_job(radius, angle, size):
    """the eye on a circle about the hard-coded sphere's centre, W from the centre to the eye, V = y, U = V x W; rows, cols ride swapped
    (cam[14] = rows; A01 code.cl:44-46), the window is compute()'s 2.66 x 2.0 (A01 code.js:180-185)"""
    w, h = size
    rad = angle * math.pi / 180.0
    W = [math.sin(rad), 0.0, math.cos(rad)]
    eye = [radius * W[0], 0.0, 1.0 + radius * W[2]]
    U = [W[2], 0.0, -W[0]]
    cam = [float(np.float32(v)) for v in (*eye, *U, 0.0, 1.0, 0.0, *W, 2.66, 2.0, h, w)]
    return dict(assign=1, width=w, height=h, cam=cam)
