"""CPU, oracle only: the edits of tests/table_edits_common.py do to the ORACLE what their names say, and no GPU test built on them can pass on
emptiness.

  1. identities: lead, tail and dup leave the base scene's closest hits, sets, occlusion flags and one pass's acu and seeds as they are, bit for
     bit (the nonfinite lead cases too); empty gives the scene without that set;
  2. floors (table_edits_common.FLOOR = 32 rays of the batch of N_RAYS + AIMED, per edited set): the MUTANT tables -- the lead scene read from
     slot 0, the tail scene read to the end of the arrays -- change at least that many rays, so a reader that leans on off[0] == 0 or on
     arrays without slack cannot equal the oracle; drop and hollow change at least that many against the base scene; shuffle changes a ray in
     some single-cell case (ties on t);
  3. the coverage table: every edit on every table shape, the shape asserted with random_scenes_common.kernel_choice.
Each test prints what it measured."""
import numpy as np
import pytest

import a10_pass as A
import random_scenes_common as S
import table_edits_common as T

CASES = T.case_ids()
IDENTITY = [c for c in CASES if T.case(c).name.startswith(("lead", "tail", "dup"))]
MUTANTS = [c for c in CASES if T.case(c).name.startswith(("lead", "tail")) and "nonfinite" not in T.case(c).name]
EFFECT = [c for c in CASES if T.case(c).name in ("drop", "hollow") and not T.case(c).identity]


def _seeds(sc):
    return A.make_seeds(sc.total_rays, seed_base=sc.key[1])


def _same_pass(a, b):
    return S.words_differ("acu", a.acu, b.acu) is None and np.array_equal(a.seeds, b.seeds) and np.array_equal(a.pixel, b.pixel)


@pytest.mark.parametrize("cid", IDENTITY)
def test_lead_tail_and_dup_leave_the_oracle_where_it_was(cid):
    ed = T.case(cid)
    rays = ed.rays()
    ch = T.changed(T.expected(ed.scene, rays), T.expected(ed.base, rays, cid))
    assert not ch.any(), f"{cid}: {int(ch.sum())} rays of {len(rays)} differ from the base scene's"
    seeds = _seeds(ed.base)
    assert _same_pass(S.expected(ed.scene, seeds, 1)[0], S.expected(ed.base, seeds, 1)[0]), f"{cid}: the pass differs from the base scene's"


@pytest.mark.parametrize("cid", [c for c in CASES if T.case(c).name == "empty"])
def test_an_empty_set_is_no_set(cid):
    ed = T.case(cid)
    rays = ed.rays()
    wo = T.without_set(ed.base, ed.sid)
    (h0, s0, o0), (h1, s1, o1) = T.expected(ed.scene, rays), T.expected(wo, rays, cid)
    i = T.set_ids(ed.base).index(ed.sid)
    assert not (s0 == i).any(), "the empty set won a ray"
    back = np.where((s1 != 0xFFFFFFFF) & (s1 >= i), s1 + 1, s1).astype(np.uint32)     # the sets behind the missing one, renumbered
    ch = T.changed((h0, s0, o0), (h1, back, o1))
    assert not ch.any(), f"{cid}: {int(ch.sum())} rays differ from the scene without the set"
    seeds = _seeds(ed.base)
    assert _same_pass(S.expected(ed.scene, seeds, 1)[0], S.expected(wo, seeds, 1)[0])


@pytest.mark.parametrize("cid", MUTANTS)
def test_a_reader_that_leans_on_the_builders_shape_is_caught(cid):
    ed = T.case(cid)
    rays = ed.rays()
    ch = T.changed(T.expected(T.mutant(ed), rays), T.expected(ed.scene, rays))
    print(f"{cid} {ed.name}: the mutant table changes {int(ch.sum())} rays of {len(rays)}, {int(ch[-T.AIMED:].sum())} of the {T.AIMED} aimed ones")
    assert ch.sum() >= T.FLOOR


@pytest.mark.parametrize("cid", EFFECT)
def test_drop_and_hollow_change_the_picture(cid):
    ed = T.case(cid)
    rays = ed.rays()
    ch = T.changed(T.expected(ed.scene, rays), T.expected(ed.base, rays, cid))
    print(f"{cid}: changes {int(ch.sum())} rays of {len(rays)} against the base scene, {int(ch[-T.AIMED:].sum())} of the {T.AIMED} aimed ones")
    assert ch.sum() >= T.FLOOR


def test_shuffle_moves_a_tie_in_some_single_cell_case():
    seen = {}
    for cid in CASES:
        ed = T.case(cid)
        if ed.name.startswith("shuffle") and ed.set()["n"] == 1:
            rays = ed.rays()
            seen[cid] = int(T.changed(T.expected(ed.scene, rays), T.expected(ed.base, rays, cid)).sum())
    print("rays a shuffle changes:", seen)
    assert seen and max(seen.values()) >= 1


def test_every_edit_occurs_on_every_table_shape():
    """the shape is that of the BASE set (an edit may move it: 97 records less one are staged; an empty set is never staged); the edited
    scene's own choice is printed next to it.  hollow on a single cell is the identity (one slab) and is listed as such."""
    rows, have = [], set()
    for cid in CASES:
        ed = T.case(cid)
        shape, before = T.shape_of(ed.base, ed.sid)
        after_shape, after = T.shape_of(ed.scene, ed.sid)
        name = ed.name.split("(")[0]
        have.add((shape, name))
        rows.append(f"{cid:22s} {ed.name:18s} {shape:15s} -> {after_shape:15s} GRIDS {before['GRIDS']} -> {after['GRIDS']}  slots {int(ed.set()['off'][-1]):6d}"
                    f"  staged {''.join('x' if t else '.' for t in after['tri_staged'])}{'  (identity)' if ed.identity else ''}")
    print("\n".join(rows))
    for shape, stratum, seed, sid in T.SHAPES:
        got, choice = T.shape_of(T.base_scene(stratum, seed), sid)
        assert got == shape, (shape, got)
        assert choice["GRIDS"] == {"staged_cell": 0, "unstaged_cell": 0, "spheres": 1, "staged_grid": 1, "memory_grid": 2, "many_sets_mesh": 2}[shape]
        for name, _ in T.EDITS:
            assert (shape, name) in have, f"no {name} on a {shape}"
    # the edges of lead and tail on staged single cells (kLdsTriMax = 96; the 60 / 40 / 7 and the 97 / 96 / 95 scenes)
    staged = lambda cid: S.kernel_choice(T.case(cid).scene)["tri_staged"]
    assert staged("staged_cell-lead") == [True, False, True]
    assert staged("lead96") == [True, False, False] and int(T.case("lead96").set()["off"][-1]) == 96
    assert staged("lead97") == [False, True, True] and int(T.case("lead97").set()["off"][-1]) == 97
    assert staged("lead_mesh7") == [True, False, True] and 60 + int(T.case("lead_mesh7").set()["off"][-1]) == 96
    assert staged("tail_mesh96") == [False, False, True, False]          # (the 97 / 96 / 95 scene has spheres in front)
    assert staged("lead_mesh96") == [False, False, False, True]
    assert staged("unstaged_cell-drop") == [False, True, False, False]


@pytest.mark.parametrize("name", T.FRAME_EDITS)
@pytest.mark.parametrize("job", T.FRAME_JOBS)
def test_the_frame_job_edits_show_in_the_a07_oracle(job, name):
    """lead leaves the frame as it was and its mutant does not; drop and hollow change it (FRAME_FLOOR pixels of 37 x 21)"""
    c = T.frame_case(job, name)
    diff = lambda a, b: int((a[1] != b[1]).any(axis=1).sum())
    if name == "lead":
        print(f"{job} lead: the mutant table changes {diff(c['mutant'], c['edited'])} pixels of {len(c['base'][1])}")
        assert diff(c["edited"], c["base"]) == 0 and int(c["edited"][0]["slab_size"][0]) == 5
        assert np.array_equal(c["edited"][2]["maxt"].view(np.uint32), c["base"][2]["maxt"].view(np.uint32))
        assert diff(c["mutant"], c["edited"]) >= T.FRAME_FLOOR
    else:
        print(f"{job} {name}: changes {diff(c['edited'], c['base'])} pixels of {len(c['base'][1])}")
        assert diff(c["edited"], c["base"]) >= T.FRAME_FLOOR
