"""The oracle's per-ray entry points (OracleScene.trace / .occluded / .shoot) against the REAL reference's own intersect,
checkForIntersection and shootRay for the ray sets of tests/reference_ray_sets.py: the fixtures tests/golden/query_<scene>.npz, made by
`python tests/golden/make_golden.py queries` from oracle/_ref/ref_render --rays.  Bit for bit, every ray of every class, no GPU.  (The
same sets at another seed against the live reference: tests/test_oracle_vs_reference.py.)"""
import numpy as np
import pytest

import query_sets as qs
import reference_ray_sets as rrs
from helpers import assert_same_floats, assert_same_hits, blob_to_scene

_answers = {}


def oracle_side(oracle, name):
    """the oracle's answers for the fixture's rays, computed once per scene"""
    if name not in _answers:
        blob, rs, _ = rrs.load_fixture(name)
        o = oracle.OracleScene(blob)
        _answers[name] = rrs.oracle_answers(o, blob_to_scene(blob), rs, lambda origin, direction, d: o.occluded(origin, direction, d, gi=True), name)
    return _answers[name]


def class_rows(rs, cls):
    return np.flatnonzero(rs["labels"] == rrs.CLASSES.index(cls))


@pytest.mark.parametrize("name", rrs.SCENES)
def test_fixture_is_not_vacuous(name):
    blob, rs, ans = rrs.load_fixture(name)
    c = rrs.census(blob_to_scene(blob), rs, ans)
    print(name, c)
    rrs.check_census(name, c)
    for cls in rrs.CLASSES:
        if name in rrs.FULL_SCENES or cls not in ("inside", "through_glass"):
            assert c["class_rays"][cls] > 0, cls
    assert ans["shoot_skip"].any() == (name in rrs.DEEP_SCENES)
    for t in rrs.RAY_TYPES:      # where the reference reports no hit, every field of the record is 0
        h = ans["hits"][t]
        assert not h[h["hit"] == 0].view(np.uint8).any()


def test_the_tie_is_decided_between_the_meshes():
    """two coincident quads of two meshes: the winner is the mesh the walk collects first, in either scene order -- and it differs"""
    (_, rs_ab, ab), (_, rs_ba, ba) = rrs.load_fixture("tie_ab"), rrs.load_fixture("tie_ba")
    assert np.array_equal(rs_ab["rays"].view(np.uint32), rs_ba["rays"].view(np.uint32))
    h_ab, h_ba = ab["hits"][qs.RAY_REFLECTION], ba["hits"][qs.RAY_REFLECTION]
    hit = h_ab["hit"] == 1
    assert np.array_equal(hit, h_ba["hit"] == 1) and hit.sum() >= 100
    assert np.array_equal(h_ab["mesh"][hit], h_ba["mesh"][hit]), "the first collected mesh wins in both orders"
    assert len(np.unique(h_ab["mesh"][hit])) == 1
    # the same index is the diffuse quad in one order and the mirror in the other: the colours differ
    differ = (rrs.bits(ab["shoot"][(qs.RAY_REFLECTION, 5)]) != rrs.bits(ba["shoot"][(qs.RAY_REFLECTION, 5)])).any(axis=1)
    assert differ[hit].sum() >= 50


@pytest.mark.parametrize("ray_type", rrs.RAY_TYPES, ids=["primary", "shadow", "reflection", "refraction"])
@pytest.mark.parametrize("cls", rrs.CLASSES)
@pytest.mark.parametrize("name", rrs.SCENES)
def test_trace_equals_the_reference(oracle, name, cls, ray_type):
    _, rs, ans = rrs.load_fixture(name)
    rows = class_rows(rs, cls)
    assert_same_hits(oracle_side(oracle, name)["hits"][ray_type][rows], ans["hits"][ray_type][rows], "%s %s type %d" % (name, cls, ray_type))


@pytest.mark.parametrize("kind", rrs.OCC_KINDS)
@pytest.mark.parametrize("name", rrs.SCENES)
def test_occlusion_equals_the_reference(oracle, name, kind):
    _, rs, ans = rrs.load_fixture(name)
    rows = np.flatnonzero(rs["occ_kind"] == rrs.OCC_KINDS.index(kind))
    assert len(rows) >= 20
    for rule in ("occ", "occ_gi"):      # occ_gi: the GI build's rule, no mesh skipped; the oracle has it, the ABI does not offer it
        bad = rows[oracle_side(oracle, name)[rule][rows] != ans[rule][rows]]
        assert bad.size == 0, "%s %s %s: %d of %d pairs differ, first: ray %d (class %s) distance %r" % (
            name, kind, rule, bad.size, len(rows), rs["occ_index"][bad[0]], rrs.CLASSES[rs["labels"][rs["occ_index"][bad[0]]]], rs["occ_dist"][bad[0]])


@pytest.mark.parametrize("depth", rrs.DEPTHS)
@pytest.mark.parametrize("cls", rrs.CLASSES)
@pytest.mark.parametrize("name", rrs.SCENES)
def test_shoot_equals_the_reference(oracle, name, cls, depth):
    _, rs, ans = rrs.load_fixture(name)
    got = oracle_side(oracle, name)
    assert np.array_equal(got["shoot_skip"], ans["shoot_skip"])
    for t in rrs.RAY_TYPES:
        rows = class_rows(rs, cls)
        if t != qs.RAY_PRIMARY:      # reference_ray_sets.DEEP_SCENES: not evaluated for the non-finite winners of the two deep scenes
            rows = rows[~ans["shoot_skip"][rows]]
        assert_same_floats(got["shoot"][(t, depth)][rows], ans["shoot"][(t, depth)][rows],
                           "%s %s type %d depth %d" % (name, cls, t, depth))
