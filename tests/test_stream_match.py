"""CPU: the enqueue-stream recogniser of command-stream fusion (csrc/pt_stream_match.hpp), run by tests/stream_match_dump.cpp on streams given as
text.  The streams are the reference host's own: tests/golden/calltrace_*.json records every setArg and enqueue of the unmodified page script, four
traces with nine executeRender passes between them.  What is checked:
  - the kernel table and its named argument indices against what the reference host binds;
  - all nine recorded passes are recognised, with the sizes, sets and lights the recording shows;
  - ROUND TRIP: a recognised pass, written out again as executeRender's sequence (initTrace, the closest-hit kernels,
    lightRender per light, per light {initShadowTrace, one any-hit kernel per set, sceneRender}, bounces x {bouncePaths, closest-hit kernels,
    per-light block}, copyToPixel; argument order as the .cl signatures have it), equals the stream that went in -- kernel by
    kernel, argument by argument, NDRange sizes aside.  Whatever is accepted without round-tripping would be fused over the wrong buffers or constants;
  - mutants of a recorded pass (every argument of every enqueue changed, enqueues dropped / duplicated / swapped, short NDRanges) are refused or still
    round-trip, and the accepted ones are exactly those that touch a value the sequence uses once;
  - the limits (lights, sets, set order, square ray counts, 32-bit ray ids).
No device: the header compares handles and bytes."""
import glob
import json
import os
import shutil
import struct
import subprocess
import time
from collections import Counter

import pytest

from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
HEADER = os.path.join(CSRC, "pt_stream_match.hpp")
TRACES = sorted(os.path.basename(p)[len("calltrace_"):-len(".json")] for p in glob.glob(os.path.join(GOLDEN, "calltrace_*.json")))
PASSES = {"cornell_320x240_k1_p2": 2, "cornell_320x240_k2_p2": 2, "cornell_teapot3_320x240_k1_p2": 2, "threeLights_160x120_k3_p3": 3}
BYTES = {"u": 4, "f": 4, "v": 64, "a": 32}
CLOSEST = ("sphereTrace", "triangleTrace", "meshTrace")


def u32(v):
    return struct.pack("<I", v).hex()


# ---- the dump program -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile tests/stream_match_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("stream_match") / "stream_match_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "stream_match_dump.cpp"), "-o", exe],
                   check=True)

    def run(streams):
        """streams: lists of enqueues (name, global sizes, argument tokens).  Returns (table, limits, one result or None per stream)."""
        text = "".join("".join(f"{n} {len(g)} {' '.join(map(str, g))} {' '.join(a)}\n" for n, g, a in s) + "end\n" for s in streams)
        out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        table, limits, results = {}, {}, []
        for line in out:
            head, *rest = line.split()
            if head == "kernel":
                table[rest[0]] = rest[1:]
            elif head == "limits":
                limits = {k: int(v) for k, v in (kv.split("=") for kv in rest)}
            elif head == "pass":
                results.append(dict(kv.split("=") for kv in rest[1:]) if rest[0] == "1" else None)
                if results[-1] is not None:
                    results[-1].update(sets=[], lights=[])
            else:
                results[-1][head + "s"].append(dict(kv.split("=") for kv in rest))
        assert len(results) == len(streams)
        for r in results:
            if r is not None:
                for k in ("width", "height", "rpp", "bounces", "spheres", "triangles"):
                    r[k] = int(r[k])
        return table, limits, results
    return run


# ---- the recorded streams -------------------------------------------------------------------------------------------------------------------
def recorded(name):
    """(meta, setArg events with their kernel's name, passes): walks the events keeping each kernel object's current arguments, snapshots them at
    every enqueueNDRangeKernel -- which is what mirt_enqueue does -- and cuts at initTrace ... copyToPixel."""
    tr = json.load(open(os.path.join(GOLDEN, f"calltrace_{name}.json")))
    kname, kargs, setargs, created, passes, cur = {}, {}, [], [], [], None
    for ev in tr["events"]:
        op = ev["op"]
        if op == "createKernel":
            kname[ev["id"]] = ev["name"]
            kargs[ev["id"]] = {}
            created.append(ev["name"])
        elif op == "setArg":
            kargs[ev["kernel"]][ev["index"]] = f"b{ev['buffer']}" if "buffer" in ev else ev["hex"]
            setargs.append((kname[ev["kernel"]], ev))
        elif op == "enqueueNDRangeKernel":
            a = kargs[ev["kernel"]]
            assert sorted(a) == list(range(len(a))), "every argument was set"
            assert ev["name"] == kname[ev["kernel"]] and ev["dim"] == len(ev["global"])
            if ev["name"] == "initTrace":
                assert cur is None
                cur = []
            if cur is not None:
                cur.append((ev["name"], list(ev["global"]), [a[i] for i in range(len(a))]))
            if ev["name"] == "copyToPixel":
                passes.append(cur)
                cur = None
        else:
            assert cur is None or op == "finish", f"{op} between the enqueues of a pass"
    assert cur is None
    return tr["meta"], created, setargs, passes


RECORDED = {name: recorded(name) for name in TRACES}


# ---- a pass written out again: executeRender's sequence, from the prose -----------------------------------------------------------------------
def set_kinds(r):
    n = len(r["sets"])
    kinds = (["sphere"] if r["spheres"] else []) + (["triangle"] if r["triangles"] else [])
    return kinds + ["mesh"] * (n - len(kinds))


def expand(r, kinds=None):
    """The enqueues of one pass as [(kernel, global sizes, [(field, token), ...])].  A field names where in the result a value comes from; a field
    that occurs once is a value nothing else in the stream can vouch for.  The ray count and the pixel count are one field, "size": both follow from
    the image size in the camera block and the rays per pixel."""
    kinds = kinds or set_kinds(r)
    total = r["width"] * r["height"] * r["rpp"]
    T = ("size", u32(total & 0xFFFFFFFF))
    G = [-(-total // 64) * 64]
    B = lambda k: (k, r[k])   # noqa: E731
    out = []

    def closest():
        for i, (kind, s) in enumerate(zip(kinds, r["sets"])):
            F = lambda k: ((f"set{i}", k), s[k])   # noqa: E731
            if kind == "sphere":
                out.append(("sphereTrace", G, [T, B("pois"), B("rays"), F("prims"), F("matid"), F("off"), F("bounds"), F("n_slabs")]))
            elif kind == "triangle":
                out.append(("triangleTrace", G, [T, B("pois"), B("rays"), F("prims"), F("normals"), F("matid"), F("off"), F("bounds"), F("n_slabs")]))
            else:
                out.append(("meshTrace", G, [T, B("pois"), B("rays"), F("prims"), F("normals"), F("off"), F("mesh_matid"), F("bounds"), F("n_slabs")]))

    def per_light_block():
        for j, l in enumerate(r["lights"]):
            out.append(("initShadowTrace", G, [B("shadow"), B("pois"), T, ((f"light{j}", "shadow"), l["shadow"]), B("seeds")]))
            for i, (kind, s) in enumerate(zip(kinds, r["sets"])):
                F = lambda k: ((f"set{i}", k), s[k])   # noqa: E731
                out.append(("sphereShadowTrace" if kind == "sphere" else "triangleShadowTrace", G, [T, B("shadow"), F("prims"), F("off"), F("bounds"), F("n_slabs")]))
            out.append(("sceneRender", G, [B("acu"), B("pois"), B("shadow"), B("material"), ((f"light{j}", "scene"), l["scene"]), T]))

    out.append(("initTrace", [-(-r["width"] // 8) * 8, -(-r["height"] // 8) * 8],
                [B("seeds"), B("rays"), B("pois"), B("bounds"), B("cam"), B("focal_length"), B("lens_rad"), ("rpp", u32(r["rpp"]))]))
    closest()
    for j, l in enumerate(r["lights"]):
        out.append(("lightRender", G, [B("pois"), B("rays"), B("acu"), ((f"light{j}", "light"), l["light"]), T]))
    per_light_block()
    for _ in range(r["bounces"]):
        out.append(("bouncePaths", G, [B("pois"), B("rays"), B("seeds"), T]))
        closest()
        per_light_block()
    npix = r["width"] * r["height"]
    out.append(("copyToPixel", [-(-npix // 64) * 64], [B("pixel"), B("acu"), B("tone"), ("size", u32(npix & 0xFFFFFFFF)), ("rpp", u32(r["rpp"]))]))
    return out


def stream_of(expansion):
    return [(n, g, [tok for _, tok in a]) for n, g, a in expansion]


def round_trips(stream, r):
    return [(n, a) for n, _, a in stream] == [(n, a) for n, _, a in stream_of(expand(r))]


# ---- 1. the header is host-only ---------------------------------------------------------------------------------------------------------------
def test_header_is_host_only():
    """the C++ standard library and include/mirt.h (plain C, <stddef.h> / <stdint.h>): it compiles alone, without a HIP header"""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-x", "c++", HEADER], check=True)
    includes = [l.split()[1] for l in open(HEADER).read().splitlines() if l.startswith("#include")]
    assert sorted(includes) == ['"../../include/mirt.h"', "<cmath>", "<cstdint>", "<cstring>", "<vector>"]
    mirt_h = [l.split()[1] for l in open(os.path.join(ROOT, "include", "mirt.h")).read().splitlines() if l.startswith("#include")]
    assert sorted(mirt_h) == ["<stddef.h>", "<stdint.h>"]


# ---- 2. the table against the reference host --------------------------------------------------------------------------------------------------
def test_table_matches_what_the_reference_host_binds(dump):
    """The rows the program prints are made of the header's named indices (args() does not compile unless each list names positions 0, 1, 2 ... in
    order, and arg() reads a value through the overload its type selects), so a row that agrees with the recording is the names agreeing with it."""
    table, _, _ = dump([])
    for name in TRACES:
        _, created, setargs, _ = RECORDED[name]
        assert set(created) <= set(table), name
        for kernel, ev in setargs:
            row = table[kernel]
            assert ev["index"] < len(row), (name, ev)
            t = row[ev["index"]]
            if t == "b":
                assert "buffer" in ev, (name, ev)
            else:
                assert "buffer" not in ev and ev["bytes"] == BYTES[t] == len(ev["hex"]) // 2, (name, ev)
                assert ev["type"] == ("Uint32Array" if t == "u" else "Float32Array"), (name, ev)


# ---- 3. + 4. the recorded passes ----------------------------------------------------------------------------------------------------------------
def test_every_recorded_pass_is_recognised_and_round_trips(dump):
    assert TRACES == sorted(PASSES)
    streams = [(name, p) for name in TRACES for p in RECORDED[name][3]]
    assert Counter(n for n, _ in streams) == PASSES and len(streams) == 9
    assert {n: len(p) for n, p in streams} == {"cornell_320x240_k1_p2": 44, "cornell_320x240_k2_p2": 44, "cornell_teapot3_320x240_k1_p2": 105,
                                               "threeLights_160x120_k3_p3": 70}
    _, _, results = dump([p for _, p in streams])
    for (name, p), r in zip(streams, results):
        meta = RECORDED[name][0]
        assert r is not None, f"{name}: a recorded pass was refused"
        assert (r["width"], r["height"], r["rpp"]) == (meta["width"], meta["height"], meta["raysPerPixel"]), name
        assert r["bounces"] == 5 == sum(n == "bouncePaths" for n, _, _ in p), name
        names = [n for n, _, _ in p]
        first = names[1:names.index("lightRender")]     # the closest-hit kernels of the primary segment
        assert [k + "Trace" for k in set_kinds(r)] == first and set(first) <= set(CLOSEST), name
        assert len(r["lights"]) == names.count("lightRender") == {"cornell_320x240_k1_p2": 1, "cornell_320x240_k2_p2": 1,
                                                                  "cornell_teapot3_320x240_k1_p2": 2, "threeLights_160x120_k3_p3": 3}[name]
        if name.startswith("cornell_teapot3"):
            assert names.count("meshTrace") == 12
        assert round_trips(p, r), name
        assert [g for _, g, _ in stream_of(expand(r))] == [g for _, g, _ in p], f"{name}: the NDRanges the reference host pads to"


# ---- 5. mutations -----------------------------------------------------------------------------------------------------------------------------
def flip(tok, word, bit):
    b = bytearray(bytes.fromhex(tok))
    b[4 * word + bit // 8] ^= 1 << (bit % 8)
    return b.hex()


def with_arg(p, e, j, tok):
    q = list(p)
    n, g, a = q[e]
    q[e] = (n, g, a[:j] + [tok] + a[j + 1:])
    return q


def needed(r, name, d):
    """the work an enqueue's NDRange must cover in dimension d"""
    if name == "initTrace":
        return (r["width"], r["height"])[d]
    return r["width"] * r["height"] * (1 if name == "copyToPixel" else r["rpp"])


@pytest.mark.parametrize("name", TRACES)
def test_mutants_are_refused_or_round_trip(dump, name):
    t0 = time.time()
    p = RECORDED[name][3][0]
    _, _, (r,) = dump([p])
    ex = expand(r)
    assert stream_of(ex) == p
    uses = Counter(f for _, _, a in ex for f, _ in a)
    once = {f for f, c in uses.items() if c == 1}
    # what the sequence uses once: the camera, the scene bounds, focal length, lens radius, the frame buffer, the tone factor, each light's lightRender block
    assert once == {"cam", "bounds", "focal_length", "lens_rad", "pixel", "tone"} | {(f"light{j}", "light") for j in range(len(r["lights"]))}

    # -- one mutant per argument of every enqueue: a buffer nobody else names, or one bit of one word flipped (the lowest of a vector's word, so that
    # the image size the camera block carries as floats stays what it is)
    single, fields = [], []
    for e, (n, g, a) in enumerate(p):
        for j, tok in enumerate(a):
            if tok[0] == "b":
                new = "b9999"
            elif len(tok) == 8:
                new = flip(tok, 0, (3 * e + j) % 32)
            else:
                new = flip(tok, (e + j) % (len(tok) // 8), 0)
            single.append(with_arg(p, e, j, new))
            fields.append(ex[e][2][j][0])
    # -- structural mutants
    dropped = [p[:e] + p[e + 1:] for e in range(len(p))]
    doubled = [p[:e] + [p[e]] + p[e:] for e in range(len(p))]
    swapped = [p[:e] + [p[e + 1], p[e]] + p[e + 2:] for e in range(len(p) - 1)]
    short = []
    for e, (n, g, a) in enumerate(p):
        for d in range(len(g)):
            q = list(p)
            q[e] = (n, g[:d] + [needed(r, n, d) - 1] + g[d + 1:], a)
            short.append(q)
    flat = [[(p[0][0], p[0][1][:1], p[0][2])] + p[1:], [(p[0][0], [p[0][1][0] * p[0][1][1]], p[0][2])] + p[1:]]   # initTrace as a 1-D NDRange
    structural = dropped + doubled + swapped

    _, _, res = dump(single + structural + short + flat)
    res_single, res_struct, res_rest = res[:len(single)], res[len(single):len(single) + len(structural)], res[len(single) + len(structural):]
    accepted = set()
    for q, got, f in zip(single, res_single, fields):
        if got is not None:
            assert round_trips(q, got), f"accepted, and not the stream that went in: {f}"
            accepted.add(f)
    assert accepted == once
    assert all(got is None for got, f in zip(res_single, fields) if f not in once)
    for q, got in zip(structural, res_struct):
        assert got is None or round_trips(q, got)
    assert all(got is None for got in res_rest), "an NDRange that does not cover the work, or a 1-D initTrace"
    print(f"{name}: {len(single)} single-argument mutants ({sum(g is not None for g in res_single)} accepted, all round-trip), "
          f"{len(structural)} dropped / doubled / swapped ({sum(g is not None for g in res_struct)} accepted), {len(short) + len(flat)} NDRange mutants, "
          f"{time.time() - t0:.2f} s")


def segments(p):
    """index of every bouncePaths: the stream is p[:s[0]] (the primary segment), the bounce segments, and the copyToPixel"""
    return [i for i, (n, _, _) in enumerate(p) if n == "bouncePaths"]


@pytest.mark.parametrize("name", TRACES)
def test_the_streams_test_fusion_refuses_are_refused(dump, name):
    """tests/test_fusion.py::STREAMS, restated on a recorded pass"""
    p = RECORDED[name][3][0]
    names = [n for n, _, _ in p]
    s = segments(p)
    light0 = names.index("lightRender")
    first_closest = p[1:light0]
    fresh = "b9999"
    streams = {
        # the host reads after the primary segment: the runtime flushes what it holds there, and the rest no longer begins with an initTrace
        "read_in_the_middle": p[:s[0]],
        "read_in_the_middle, the rest": p[s[0]:],
        "bounce_before_the_light_block": p[:light0] + [p[s[0]]] + first_closest + p[light0:s[0]] + [p[-1]],
        "short_ndrange": [(n, g if len(g) == 2 else [64], a) for n, g, a in p],
        "no_copy_to_pixel": p[:s[2]],
        "light_block_differs_in_a_bounce": p[:s[0]] + [(n, g, a[:3] + [flip(a[3], 0, 23)] + a[4:]) if n == "initShadowTrace" else (n, g, a) for n, g, a in p[s[0]:]],
        "bounce_rays_into_another_buffer": [(n, g, [a[0], fresh] + a[2:]) if n == "bouncePaths" else (n, g, a) for n, g, a in p],
    }
    _, _, res = dump(list(streams.values()))
    assert {k: got is None for k, got in zip(streams, res)} == {k: True for k in streams}


# ---- 6. limits --------------------------------------------------------------------------------------------------------------------------------
def test_limits(dump):
    _, limits, (r,) = dump([RECORDED["cornell_teapot3_320x240_k1_p2"][3][0]])
    assert limits == {"lights": 8, "meshes": 16}
    kinds = set_kinds(r)
    assert "mesh" in kinds and "sphere" in kinds
    mesh = r["sets"][kinds.index("mesh")]
    sphere = r["sets"][kinds.index("sphere")]
    others = [s for k, s in zip(kinds, r["sets"]) if k != "mesh"]

    def variant(**kw):
        return dict(r, **kw)

    def lights(n):
        return variant(lights=[r["lights"][i % len(r["lights"])] for i in range(n)])

    def meshes(n):
        return variant(sets=others + [mesh] * n)

    def sized(w, h, rpp):
        cam = bytearray(bytes.fromhex(r["cam"]))
        cam[56:64] = struct.pack("<ff", w, h)
        return variant(width=w, height=h, rpp=rpp, cam=cam.hex())

    no_sphere = [k for k in kinds if k != "sphere"]
    cases = [
        ("as many lights as fit", lights(limits["lights"]), None, True),
        ("one light too many", lights(limits["lights"] + 1), None, False),
        ("as many sets as fit", meshes(limits["meshes"] + 2 - len(others)), None, True),
        ("one set too many", meshes(limits["meshes"] + 3 - len(others)), None, False),
        ("a sphere set after a mesh", variant(sets=[s for s in r["sets"] if s is not sphere] + [sphere]), no_sphere + ["sphere"], False),
        ("a sphere set after a mesh, between meshes", variant(sets=[mesh, sphere, mesh]), ["mesh", "sphere", "mesh"], False),
        ("4 rays per pixel", sized(320, 240, 4), None, True),
        ("a ray count that is no square", sized(320, 240, 2), None, False),
        ("a ray count that is no square: 8", sized(320, 240, 8), None, False),
        ("the last ray id that fits 32 bits", sized(65535, 65536, 1), None, True),
        ("2^32 rays", sized(65536, 65536, 1), None, False),
        ("2^32 rays, by rays per pixel", sized(32768, 32768, 4), None, False),
    ]
    streams = []
    for _, v, k, _ in cases:
        if k is None:   # the kinds follow from the flags: a variant that drops a kind says so
            ks = set_kinds(v)
            v["spheres"], v["triangles"] = int("sphere" in ks), int("triangle" in ks)
        streams.append(stream_of(expand(v, k)))
    _, _, res = dump(streams)
    for (what, v, k, want), s, got in zip(cases, streams, res):
        assert (got is not None) == want, what
        if got is not None:
            assert round_trips(s, got), what
