"""CPU: the frame recogniser of command-stream fusion (csrc/pt_stream_match.hpp match_frame), run by tests/frame_stream_match_dump.cpp on streams
given as text.  The streams are the four a page issues for one frame -- Assign04 computeTri (initTrace, meshTrace), Assign07 computeTri (initTrace,
meshTrace), Assign07 compute (initTrace, molTrace), Assign07 both models (initTrace, molTrace, meshTrace) -- built from the kernels' argument tables
as the header prints them.  What is checked:
  - each well-formed stream is recognised and ROUND-TRIPS: written out again from what the recogniser reports, in the .cl signatures' argument
    order (A04 code.cl:204, 262; A07 code.cl:311, 337, 475), it equals the stream that went in, argument by argument;
  - every argument of every enqueue changed on its own is refused or still round-trips -- and the accepted ones are exactly the values a frame uses
    once (so nothing else in the stream could vouch for them);
  - the mutants a fused frame must never swallow are refused: another pixels / rays / cam between stages, mesh before molecule, a second initTrace,
    a smaller global size, an Assign10 kernel in between, mixed dialects, a box or n_slabs that differs between stages;
  - the existing entry points (match_pass through tests/stream_match_dump.cpp) answer the reference host's recorded passes as before.
No device: the header compares handles and bytes."""
import os
import shutil
import struct
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
BYTES = {"u": 4, "f": 4, "v": 64, "a": 32}
W, H = 96, 64
G = [96, 64]     # getLocalWS(2, 64) = 8 x 8: the image size rounded up


def u32(v):
    return struct.pack("<I", v).hex()


def f32s(*v):
    return struct.pack("<%df" % len(v), *v).hex()


CAM = f32s(0, 0, 5, 1, 0, 0, 0, 1, 0, 0, 0, 1, 3.0, 2.0, W, H)
BOUND = f32s(-1, -2, -3, 1, 1, 2, 3, 1)


def compile_dump(tmp, src):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile the dump program with")
    exe = os.path.join(tmp, os.path.splitext(src)[0])
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", src), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = compile_dump(str(tmp_path_factory.mktemp("frame_stream_match")), "frame_stream_match_dump.cpp")

    def run(streams):
        text = "".join("".join(f"{n} {len(g)} {' '.join(map(str, g))} {' '.join(a)}\n" for n, g, a in s) + "end\n" for s in streams)
        out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        table = {l.split()[1]: l.split()[2:] for l in out if l.startswith("kernel ")}
        res = [dict(kv.split("=") for kv in l.split()[2:]) if l.split()[1] == "1" else None for l in out if l.startswith("frame ")]
        assert len(res) == len(streams)
        return table, res
    return run


# ---- a frame written out from its parts: the argument order of the .cl signatures ------------------------------------------------------------
def frame_stream(assign, mesh, mol, r):
    """[(kernel, global sizes, [(field, token), ...])] of one frame from the fields `r` (the recogniser's report, or the values a test chose)"""
    pre = f"A0{assign}:"
    head = [("pixels", r["pixels"]), ("cam", r["cam"]), ("rays", r["rays"])]
    out = [(pre + "initTrace", G, head + ([("bounds", r["bounds"])] if assign == 7 else []))]
    if mol:
        out.append((pre + "molTrace", G, head + [("s_size", r["s_size"]), ("s_atoms", r["s_atoms"]), ("s_mindex", r["s_mindex"]), ("s_mcolor", r["s_mcolor"]),
                                                 ("bounds", r["bounds"]), ("n_slabs", r["n_slabs"]), ("s_slab_size", r["s_slab_size"])]))
    if mesh:
        tail = [("bounds", r["bounds"]), ("n_slabs", r["n_slabs"]), ("t_slab_size", r["t_slab_size"])] if assign == 7 else []
        out.append((pre + "meshTrace", G, head + [("t_size", r["t_size"]), ("t_pos", r["t_pos"]), ("t_normal", r["t_normal"]), ("t_mindex", r["t_mindex"]),
                                                  ("t_mcolor", r["t_mcolor"])] + tail))
    return out


def tokens(stream):
    return [(n, list(g), [t for _, t in a]) for n, g, a in stream]


VALUES = dict(pixels="b0", cam=CAM, rays="b1", bounds=BOUND, t_size=u32(9144), t_pos="b2", t_normal="b3", t_mindex="b4", t_mcolor="b5", t_slab_size="b6",
              s_size=u32(8900), s_atoms="b7", s_mindex="b8", s_mcolor="b9", s_slab_size="b10", n_slabs=u32(16))
FRAMES = {"a04_mesh": (4, True, False), "a07_mesh": (7, True, False), "a07_mol": (7, False, True), "a07_both": (7, True, True)}


def well_formed(name):
    return frame_stream(*FRAMES[name], VALUES)


def round_trips(stream, r, assign, mesh, mol):
    return r is not None and (int(r["assign"]), r["mesh"] == "1", r["mol"] == "1") == (assign, mesh, mol) and \
        tokens(frame_stream(assign, mesh, mol, r)) == tokens(stream) and (int(r["width"]), int(r["height"])) == (W, H)


def test_streams_are_built_from_the_argument_tables(dump):
    table, _ = dump([])
    for name in FRAMES:
        for kernel, _, args in well_formed(name):
            types = table[kernel]
            assert len(types) == len(args), kernel
            for ty, (_, tok) in zip(types, args):
                assert (tok[0] == "b") if ty == "b" else (len(tok) == 2 * BYTES[ty]), (kernel, ty, tok)


@pytest.mark.parametrize("name", list(FRAMES))
def test_well_formed_frames_are_recognised_and_round_trip(dump, name):
    s = well_formed(name)
    _, (r,) = dump([tokens(s)])
    assert round_trips(s, r, *FRAMES[name])
    if FRAMES[name][0] == 4:
        assert r["bounds"] == "00" * 32 and r["t_slab_size"] == "-"
    if not FRAMES[name][2]:
        assert r["s_atoms"] == "-" and r["s_slab_size"] == "-"
    if not FRAMES[name][1]:
        assert r["t_pos"] == "-" and r["t_slab_size"] == "-"


def other(tok):
    """the same kind of argument with another value"""
    if len(tok) < 8:   # a buffer, "b<id>" (a value is at least four bytes in hex)
        return "b99"
    return ("01" if tok[:2] != "01" else "02") + tok[2:]


@pytest.mark.parametrize("name", list(FRAMES))
def test_every_single_argument_change_is_refused_or_round_trips(dump, name):
    """One argument of one enqueue changed at a time.  Accepted mutants must round-trip (the change is IN the report), and they are exactly the
    fields that occur once in the frame; a field that occurs in several enqueues (pixels, cam, rays, the box, n_slabs of both grids) changed in one of
    them is refused."""
    s = well_formed(name)
    count = {}
    for _, _, args in s:
        for f, _ in args:
            count[f] = count.get(f, 0) + 1
    mutants, where = [], []
    for i, (_, _, args) in enumerate(s):
        for j, (f, tok) in enumerate(args):
            m = tokens(s)
            m[i][2][j] = other(tok)
            mutants.append(m)
            where.append(f)
    _, res = dump(mutants)
    for m, f, r in zip(mutants, where, res):
        if count[f] > 1:
            assert r is None, f"{f} changed in one stage only was accepted"
        else:
            assert r is not None and tokens(frame_stream(*FRAMES[name], r)) == m, f


def test_mutants_a_fused_frame_must_not_swallow_are_refused(dump):
    both, mesh7, mol7, mesh4 = (tokens(well_formed(n)) for n in ("a07_both", "a07_mesh", "a07_mol", "a04_mesh"))
    mutants = {}
    for what, j in (("pixels", 0), ("cam", 1), ("rays", 2)):   # another pixels / cam / rays between stages
        for stage in (1, 2):
            m = tokens(well_formed("a07_both"))
            m[stage][2][j] = other(m[stage][2][j])
            mutants[f"{what} differs in stage {stage}"] = m
    mutants["mesh before molecule"] = [both[0], both[2], both[1]]
    mutants["a second initTrace"] = [both[0], both[1], both[0], both[2]]
    mutants["a second initTrace at the end"] = [mesh7[0], mesh7[1], mesh7[0]]
    mutants["two meshTraces"] = [mesh7[0], mesh7[1], mesh7[1]]
    mutants["two molTraces"] = [mol7[0], mol7[1], mol7[1]]
    mutants["initTrace alone"] = [mesh7[0]]
    mutants["no initTrace"] = [mesh7[1]]
    for stage in (1, 2):
        m = tokens(well_formed("a07_both"))
        m[stage] = (m[stage][0], [G[0] - 8, G[1]], m[stage][2])
        mutants[f"a smaller global size in stage {stage}"] = m
    m = tokens(well_formed("a07_mesh"))
    mutants["an NDRange that does not cover the image"] = [(n, [G[0] - 8, G[1]], a) for n, _, a in m]
    mutants["a larger global size in the trace"] = [m[0], (m[1][0], [G[0] + 8, G[1]], m[1][2])]
    acu = ("initAcu", [64], ["b20", u32(64)])
    mutants["an Assign10 kernel in between"] = [both[0], both[1], acu, both[2]]
    mutants["an Assign10 kernel after the initTrace"] = [mesh7[0], acu, mesh7[1]]
    mutants["Assign04 initTrace, Assign07 meshTrace"] = [mesh4[0], mesh7[1]]
    mutants["Assign07 initTrace, Assign04 meshTrace"] = [mesh7[0], mesh4[1]]
    mutants["Assign04 initTrace, Assign07 molTrace"] = [mesh4[0], mol7[1]]
    for stage, j in ((1, 7), (2, 8)):   # the box of molTrace (argument 7) / meshTrace (argument 8)
        m = tokens(well_formed("a07_both"))
        m[stage][2][j] = other(m[stage][2][j])
        mutants[f"another box in stage {stage}"] = m
    m = tokens(well_formed("a07_both"))
    m[2][2][9] = u32(8)
    mutants["the mesh binned with another n_slabs than the molecule"] = m
    m = tokens(well_formed("a07_mesh"))
    m[0] = (m[0][0], [G[0]], m[0][2])
    mutants["a 1-D initTrace"] = m
    names = list(mutants)
    _, res = dump([mutants[n] for n in names] + [both, mesh7, mol7, mesh4])
    for n, r in zip(names, res):
        assert r is None, n + ": accepted"
    assert all(r is not None for r in res[len(names):])


def test_a_padded_ndrange_is_recognised(dump):
    """the pages round the global size up to the work-group shape: 100 x 70 runs on 104 x 72"""
    v = dict(VALUES, cam=f32s(0, 0, 5, 1, 0, 0, 0, 1, 0, 0, 0, 1, 3.0, 2.0, 100, 70))
    s = [(n, [104, 72], a) for n, _, a in tokens(frame_stream(7, True, True, v))]
    _, (r,) = dump([s])
    assert r is not None and (int(r["width"]), int(r["height"])) == (100, 70)


def test_the_pass_recogniser_answers_as_before(tmp_path):
    """tests/test_stream_match.py's own entry points, once: its dump program built from the same header recognises every recorded executeRender pass
    with the sizes the recording shows, and refuses a frame stream."""
    import test_stream_match as T
    exe = compile_dump(str(tmp_path), "stream_match_dump.cpp")
    streams, want = [], []
    for name in T.TRACES:
        meta, _, _, passes = T.RECORDED[name]
        assert len(passes) == T.PASSES[name]
        for p in passes:
            streams.append(p)
            want.append(p[0][1])
    streams.append(tokens(well_formed("a07_mesh")))
    text = "".join("".join(f"{n} {len(g)} {' '.join(map(str, g))} {' '.join(a)}\n" for n, g, a in s) + "end\n" for s in streams)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    table = [l for l in out if l.startswith("kernel ")]
    assert len(table) == 22 and "kernel A07:molTrace b v b u b b b a u b" in table
    verdicts = [l.split() for l in out if l.startswith("pass ")]
    assert len(verdicts) == len(streams) == 10
    for v, g in zip(verdicts[:-1], want):
        assert v[1] == "1"
        r = dict(kv.split("=") for kv in v[2:])
        assert -(-int(r["width"]) // 8) * 8 == g[0] and -(-int(r["height"]) // 8) * 8 == g[1]
    assert verdicts[-1][1] == "0"
