"""CPU: the argument rules mirt_filter_atrous and mirt_upsample_guided share (csrc/pt_post_check.hpp), asked through tests/post_check_dump.cpp:
the extent, normal_power_log2, tone and sigma rules at their edges, and the aliasing rule -- no present output's byte range meets an input's, no
two outputs' meet -- over generated ranges against Python's own interval arithmetic, every (input, output) position of the filter's 3 + 2 and the
upsampler's 5 + 2 buffers included.  No device: the header is plain integer and float comparisons."""
import os
import random
import shutil
import struct
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
HEADER = os.path.join(CSRC, "pt_post_check.hpp")
OK, EMPTY, TOO_LARGE = 0, 1, 2
NONE, OUTPUT_INPUT, OUTPUTS = 0, 1, 2
BASE = 0x7F3A00000000           # device addresses lie above 2^32
NPIX = 83 * 47
SHAPES = {"filter": ([NPIX * 16] * 3, [NPIX * 16, NPIX * 4]),
          "upsampler": ([29 * 17 * 16] * 3 + [NPIX * 16] * 2, [NPIX * 16, NPIX * 4])}


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile tests/post_check_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("post_check") / "post_check_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "post_check_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        """one answer (a list of ints) per question"""
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True)
        out = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def test_header_is_host_only():
    """nothing beyond <stddef.h> and <stdint.h>: it compiles alone, without a HIP header"""
    text = open(HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>"], includes
    assert "__device__" not in text and "__host__" not in text


def test_extent_edges(ask):
    sides = (0, 1, 65535, 65536, 2 ** 32 - 1)
    cases = [(w, h) for w in sides for h in sides]
    got = ask([f"extent {w} {h}" for w, h in cases])
    for (w, h), (code,) in zip(cases, got):
        want = EMPTY if w == 0 or h == 0 else TOO_LARGE if w > 65535 or h > 65535 else OK
        assert code == want, (w, h)


def test_normal_power_edges(ask):
    cases = (0, 1, 7, 8, 9, 2 ** 31, 2 ** 32 - 1)
    got = ask([f"power {p}" for p in cases])
    assert [g[0] for g in got] == [1 if p <= 7 else 0 for p in cases]


def test_tone_and_sigma_are_finite_and_positive(ask):
    bits = lambda v: struct.unpack("<I", struct.pack("<f", v))[0]
    denormal_min, float_max = 0x00000001, 0x7F7FFFFF
    cases = [   # (bits, accepted)
        (bits(0.0), 0), (bits(-0.0), 0), (bits(-0.25), 0), (0x7FC00000, 0), (0xFFC00000, 0), (0x7F800001, 0), (bits(float("inf")), 0), (bits(float("-inf")), 0),
        (denormal_min, 1), (denormal_min | 0x80000000, 0), (float_max, 1), (float_max | 0x80000000, 0), (bits(0.25), 1),      # tone
        (bits(-1.0), 0), (bits(0.1), 1), (bits(2.0), 1)]                                                                        # sigma: 0, NaN and inf are above
    got = ask([f"positive {b:x}" for b, _ in cases])
    for (b, want), (g,) in zip(cases, got):
        assert g == want, hex(b)


# ---- aliasing ---------------------------------------------------------------------------------------------------------------------------------
def meet(a, b):
    """Python's own interval arithmetic on (addr, bytes, present): the half-open ranges share a byte"""
    return bool(a[2] and b[2]) and max(a[0], b[0]) < min(a[0] + a[1], b[0] + b[1])


def expected(ins, outs):
    if any(meet(o, i) for o in outs for i in ins):
        return OUTPUT_INPUT
    if any(meet(outs[a], outs[b]) for a in range(len(outs)) for b in range(a + 1, len(outs))):
        return OUTPUTS
    return NONE


def question(ins, outs):
    return f"alias {len(ins)} {len(outs)} " + " ".join(f"{a:x} {n:x} {int(p)}" for a, n, p in ins + outs)


def apart(sizes, first=BASE, gap=1 << 20):
    """ranges of these sizes, one behind the other with a gap between that is wider than any of them"""
    out, at = [], first
    for n in sizes:
        out.append((at, n, True))
        at += n + gap
    return out


def placements(target, n):
    """(tag, address, meets) of a range of n bytes against `target`: every way the issue names"""
    a, m = target[0], target[1]
    yield "same start", a, True
    yield "one byte over its low end", a - n + 1, True
    yield "one byte over its high end", a + m - 1, True
    yield "ends where it begins", a - n, False
    yield "begins where it ends", a + m, False
    yield "inside it or around it", a + (m - n) // 2, True


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_output_against_every_input(ask, shape):
    in_sizes, out_sizes = SHAPES[shape]
    ins = apart(in_sizes)
    far = apart(out_sizes, first=BASE + (1 << 30))
    cases, hit = [], set()
    for o, n in enumerate(out_sizes):
        for i, target in enumerate(ins):
            for tag, addr, meets in placements(target, n):
                for present in (True, False):
                    outs = list(far)
                    outs[o] = (addr, n, present)
                    want = OUTPUT_INPUT if meets and present else NONE
                    assert expected(ins, outs) == want, "the test's own arithmetic"
                    cases.append((f"{shape}: output {o} {tag} of input {i}, present={present}", ins, outs, want))
                    if want == OUTPUT_INPUT:
                        hit.add((i, o))
    assert hit == {(i, o) for i in range(len(ins)) for o in range(2)}
    got = ask([question(i, o) for _, i, o, _ in cases])
    for (tag, _, outs, want), (code, any_out) in zip(cases, got):
        assert code == want, tag
        assert any_out == int(any(p for _, _, p in outs)), tag


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_outputs_against_each_other_and_absent_outputs(ask, shape):
    in_sizes, out_sizes = SHAPES[shape]
    ins = apart(in_sizes)
    first = (BASE + (1 << 30), out_sizes[0], True)
    cases = []
    for tag, addr, meets in placements(first, out_sizes[1]):
        for p0 in (True, False):
            for p1 in (True, False):
                outs = [(first[0], first[1], p0), (addr, out_sizes[1], p1)]
                want = OUTPUTS if meets and p0 and p1 else NONE
                assert expected(ins, outs) == want, "the test's own arithmetic"
                cases.append((f"{shape}: pixel {tag} of the other output, present=({p0}, {p1})", outs, want))
    # an output over an input AND over the other output: the input is reported, as the entry points' messages have it
    both = [(ins[0][0], out_sizes[0], True), (ins[0][0] + 16, out_sizes[1], True)]
    cases.append((f"{shape}: both over input 0", both, OUTPUT_INPUT))
    got = ask([question(ins, outs) for _, outs, _ in cases])
    for (tag, outs, want), (code, any_out) in zip(cases, got):
        assert code == want, tag
        assert any_out == int(outs[0][2] or outs[1][2]), tag


def test_generated_ranges(ask):
    """any number of inputs and outputs of any sizes, placed at random in a window a few ranges wide so that most cases have an overlap somewhere"""
    rng = random.Random(20260)
    cases = []
    for _ in range(2000):
        n_in, n_out = rng.randint(0, 6), rng.randint(0, 4)
        pick = lambda present: (BASE + rng.randint(0, 4000), rng.randint(1, 700), present)
        ins = [pick(True) for _ in range(n_in)]
        outs = [pick(rng.random() < 0.75) for _ in range(n_out)]
        cases.append((ins, outs))
    got = ask([question(i, o) for i, o in cases])
    seen = set()
    for (ins, outs), (code, any_out) in zip(cases, got):
        assert code == expected(ins, outs), (ins, outs)
        assert any_out == int(any(p for _, _, p in outs)), outs
        seen.add(code)
    assert seen == {NONE, OUTPUT_INPUT, OUTPUTS}
