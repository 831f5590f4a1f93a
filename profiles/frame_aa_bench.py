#!/usr/bin/env python3
"""profiles/frame_aa_bench.py [out.json] -- the anti-aliased frame (mirt_render_frame_aa) against the fine frame a user had to render without it, on one
device.  Per configuration and aa = 2, 3, 4 three variants, HIP-event time around the one call, buffers resident:
  fine_frame   mirt_render_frame at aa*W x aa*H: the same rays, aa*aa times the pixels written (and then read back and averaged on the host, which is
               NOT in this number)
  lanes        mirt_render_frame_aa as it ships: one lane per sample, the sums reduced across lanes
  pixel        mirt_render_frame_aa, one thread per output pixel looping over its samples: not in the shipped library.  With
               profiles/frame_aa/pixel_structure.patch applied the library has both and reads MIRT_FRAME_AA_STRUCTURE=pixel|lanes at every call;
               this script measures `pixel` when the library it loads knows that switch, and says so when it does not.
Configurations: BASELINE config 2 (Assign04 parliament, fine 1024 x 1024), config 3 (Assign07 parliament n16), the 3IZ4 molecule, Assign07 teapot n2 (the
GROUPS walk); the Assign07 ones at fine 1920 x 1080; at aa 3 the fine size is rounded down to multiples of 3.  Medians of REPEATS calls after WARMUP, the
three variants alternating inside one loop.  Target: the structure that ships for the aa is no slower than fine_frame by more than the min..max spread
of fine_frame's own calls in that run (`within_spread`).  Every aa frame is also checked against the box average of the fine frame, bit for bit.
  frame_aa_bench.py --relabel FILE   recompute the derived fields (shipped, faster, within_spread) of FILE from its recorded times and SHIPPED below."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import __graft_entry__ as graft  # noqa: E402
import bench  # noqa: E402

WARMUP, REPEATS = 3, 20
SHIPPED = {2: "lanes", 3: "lanes", 4: "lanes"}   # csrc/pt_kernels_frame.hip launch_frame_aa


def fixture(name):
    fx = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return json.loads(bytes(fx["frame_json"]).decode())


def stats(v):
    v = np.sort(np.asarray(v, np.float64))
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "calls": len(v)}


def box(fine, W, H, aa):
    f = fine.reshape(H, aa, W, aa, 4).astype(np.uint32)
    out = np.full((H, W, 4), 255, np.uint8)
    out[..., :3] = ((f[..., :3].sum(axis=(1, 3)) + aa * aa // 2) // (aa * aa)).astype(np.uint8)
    return out.reshape(-1, 4)


def label(rec):
    """the derived fields, from the recorded times"""
    rec["shipped"] = {str(k): v for k, v in SHIPPED.items()}
    for r in rec["runs"]:
        ms = r["ms"]
        r["shipped"] = SHIPPED[r["aa"]]
        if "pixel" in ms:
            r["faster"] = "pixel" if ms["pixel"]["median"] < ms["lanes"]["median"] else "lanes"
        r["fine_frame_spread_ms"] = ms["fine_frame"]["max"] - ms["fine_frame"]["min"]
        r["shipped_minus_fine_frame_ms"] = ms[r["shipped"]]["median"] - ms["fine_frame"]["median"]
        r["within_spread"] = bool(r["shipped_minus_fine_frame_ms"] <= r["fine_frame_spread_ms"])
    return rec


def main():
    out = os.path.join(ROOT, "profiles", "frame_aa", "timing.json")
    if len(sys.argv) > 2 and sys.argv[1] == "--relabel":
        rec = label(json.load(open(sys.argv[2])))
        with open(sys.argv[2], "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
        return
    if len(sys.argv) > 1:
        out = sys.argv[1]
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render
    both = b"MIRT_FRAME_AA_STRUCTURE" in open(mirt.LIB_PATH, "rb").read()
    if not both:
        print("this library has the shipped structure only: `pixel` is not measured (profiles/frame_aa/pixel_structure.patch)", flush=True)
    VARIANTS = ("fine_frame", "pixel", "lanes") if both else ("fine_frame", "lanes")
    ctx = mirt.Context(0)
    configs = [("config2_a04_parliament", fixture("frame_a04_parliament_96x64"), (1024, 1024)),
               ("config3_a07_parliament_n16", fixture("frame_a07_parliament_n16_160x120"), (1920, 1080)),
               ("a07_mol_3IZ4_n16", fixture("frame_a07_mol_3IZ4_n16_96x64"), (1920, 1080)),
               ("a07_teapot_n2_groups", fixture("frame_a07_teapot_n2_160x120"), (1920, 1080))]
    runs = []
    for name, d, (fw, fh) in configs:
        for aa in (2, 3, 4):
            W, H = fw // aa, fh // aa
            fine_d = render.frame_resized(d, aa * W, aa * H)
            cam = list(fine_d["cam"])
            cam[14], cam[15] = float(W), float(H)
            coarse_d = dict(fine_d, width=W, height=H, cam=cam)   # the same window on the coarser lattice
            fine = render.FrameOneLaunch(ctx, render.FramePacked(fine_d))
            coarse = render.FrameOneLaunch(ctx, render.FramePacked(coarse_d), aa=aa)

            def call(variant):
                if variant == "fine_frame":
                    os.environ.pop("MIRT_FRAME_AA_STRUCTURE", None)
                else:
                    os.environ["MIRT_FRAME_AA_STRUCTURE"] = variant
                f = fine if variant == "fine_frame" else coarse
                ctx.timer_start()
                f.render()
                return ctx.timer_stop_ms()
            call("fine_frame")
            want = box(fine.pixels.read(np.uint8), W, H, aa)
            for v in VARIANTS[1:]:
                call(v)
                assert np.array_equal(coarse.pixels.read(np.uint8).reshape(-1, 4), want), (name, aa, v)
            t = {v: [] for v in VARIANTS}
            for i in range(WARMUP + REPEATS):
                for v in VARIANTS:
                    ms = call(v)
                    if i >= WARMUP:
                        t[v].append(ms)
            os.environ.pop("MIRT_FRAME_AA_STRUCTURE", None)
            runs.append({"config": name, "aa": aa, "output": [W, H], "fine": [aa * W, aa * H], "ms": {v: stats(t[v]) for v in VARIANTS},
                         "lit_fraction": float((want[:, :3].max(axis=1) > 0).mean())})
            print(json.dumps(runs[-1]), flush=True)
            fine.release(); coarse.release()
    rec = label({"csrc_sha256": bench.csrc_sha256(), "device": mirt.lib().mirt_version().decode(), "warmup": WARMUP, "repeats": REPEATS,
                 "what": "HIP-event ms of one call: mirt_render_frame at the fine size vs mirt_render_frame_aa in both structures of its kernel", "runs": runs})
    ctx.destroy()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
