"""The GI mode against the REAL reference, bit for bit, on the CPU: the fixtures tests/golden/gi_pairs_<scene>.npz hold the reference's
shootRay colours and getRay rays under seeded engines, each with the key whose draws are the same floats (tests/gi_reference_sets.py).
The oracle's GI restatement (oracle/cpu_ref.c: shade_diffuse, render_pixel) must give the same bits for those keys: one diffuse bounce's
direction, bias, shadow rule and normalisation, the pixel jitter, the key hand-over below a mirror and from (seed, pixel, sample) to a
ray.  Nothing but tests/golden/ is read; no GPU, no reference binary."""
import numpy as np
import pytest

import gi_reference_sets as grs
import query_sets as qs
import reference_ray_sets as rrs
from helpers import assert_same_floats, blob_to_scene, same_bits
from test_gi import crt_test_gi

_oracles = {}


def loaded(oracle, name):
    """(fixture arrays, scene dict, OracleScene, the oracle's answers) of a scene: made once"""
    if name not in _oracles:
        blob, fx = grs.load_fixture(name)
        o = oracle.OracleScene(blob)
        _oracles[name] = (fx, blob_to_scene(blob), o, grs.oracle_answers(oracle, o, fx))
    return _oracles[name]


def test_gi_mix_inverse_inverts_gi_mix(oracle):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    b = np.concatenate([rng.integers(0, 1 << 32, 500_000, dtype=np.uint64), rng.integers(0, 10_000, 250_000),
                        oracle.GI_CHILD + rng.integers(0, 66, 250_000)]).astype(np.uint32)
    mixed = oracle.gi_array(a, b)[0]
    assert np.array_equal(oracle.gi_mix_inverse(mixed, b), a)
    assert np.array_equal(oracle.gi_array(oracle.gi_mix_inverse(a, b), b)[0], a)      # and the other way round: a bijection
    assert int(oracle.gi_mix_inverse(oracle.gi_mix(5, 7), 7)) == 5


@pytest.mark.parametrize("name", grs.SCENES)
def test_fixture_keys_draw_the_references_floats(pkg, oracle, name):
    """Every matched key gives, through the oracle's generator AND through the host build of the product's (csrc/gi_random.h), the two
    floats the reference drew under the pair's seed; and the derived seeds and parent keys put the keys where the cases say."""
    fx = grs.load_fixture(name)[1]
    for kind, d0 in (("hit", 2), ("jitter", 0)):
        keys, draws = fx[kind + "_keys"], fx[kind + "_draws"]
        assert len(keys) >= grs.MIN_PAIRS and len(np.unique(keys)) == len(keys)
        assert ((fx[kind + "_seeds"] >= grs.SEED_FIRST) & (fx[kind + "_seeds"] < grs.SEED_FIRST + grs.SEED_COUNT)).all()
        for j in (0, 1):
            d = np.full(len(keys), d0 + j, dtype=np.uint32)
            same_bits(oracle.gi_array(keys, d)[1], draws[:, j], "%s pairs, draw %d: the oracle's generator" % (kind, d0 + j))
            # crt_test_gi what = 2: the d-th uniform number of a key by the product's header (csrc/gi_random.h), compiled for the host
            assert np.array_equal(crt_test_gi(pkg, -1, 2, keys, d), draws[:, j]), (kind, d0 + j)
        values = draws.view(np.float32)
        assert ((values >= 0) & (values < 1)).all() and len(np.unique(draws, axis=0)) > len(draws) * 0.9
    W = int(loaded(oracle, name)[1]["settings"]["image_settings"]["width"])
    mix = lambda a, b: oracle.gi_array(np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32))[0]
    pixel = fx["p_row"] * np.uint32(W) + fx["p_col"]
    assert np.array_equal(mix(mix(fx["p_seed"], pixel), np.zeros_like(pixel)), fx["hit_keys"][fx["p_pair"]])
    pixel = fx["j_row"] * np.uint32(W) + fx["j_col"]
    assert (fx["j_k"] >= 1).all() and np.array_equal(mix(mix(fx["j_seed"], pixel), fx["j_k"]), fx["jitter_keys"][fx["j_pair"]])
    assert np.array_equal(mix(fx["m_keys"], np.full(len(fx["m_keys"]), oracle.GI_CHILD, dtype=np.uint32)), fx["hit_keys"][fx["m_pair"]])


@pytest.mark.parametrize("name", grs.SCENES)
def test_oracle_gi_shoot_equals_the_reference(oracle, name):
    fx, _, _, ans = loaded(oracle, name)
    assert len(fx["q_rays"]) >= grs.MIN_QUERY
    for k, cls in enumerate(grs.CLASSES):                 # compared class by class so that a failure names the class
        rows = np.flatnonzero(fx["q_label"] == k)
        assert_same_floats(ans["q_rgb"][rows], fx["q_rgb"][rows], "%s %s: shootRay, N = 1, MAX_DEPTH = 1" % (name, cls))


@pytest.mark.parametrize("name", grs.SCENES)
def test_oracle_gi_shoot_below_a_mirror_equals_the_reference(oracle, name):
    fx, _, _, ans = loaded(oracle, name)
    assert len(fx["m_rays"]) >= (grs.MIN_MIRROR if name in grs.MIRROR_SCENES else 0)
    assert_same_floats(ans["m_rgb"], fx["m_rgb"], "%s: shootRay below a mirror, N = 1, MAX_DEPTH = 2" % name)


@pytest.mark.parametrize("name", grs.SCENES)
def test_oracle_jittered_camera_rays_equal_the_references(oracle, name):
    fx, _, o, ans = loaded(oracle, name)
    assert len(fx["j_rays"]) >= grs.MIN_JITTER
    same_bits(ans["j_rays"], fx["j_rays"], "%s: getRay(row, col, true)" % name)
    centre = np.array([np.concatenate(o.camera_ray(int(r), int(c))) for r, c in zip(fx["j_row"], fx["j_col"])], dtype=np.float32)
    assert (centre[:, 3:] != fx["j_rays"][:, 3:]).any(axis=1).all(), "a jittered ray that is the centre ray"


@pytest.mark.parametrize("name", grs.SCENES)
def test_oracle_gi_frame_pixel_equals_the_reference(oracle, name):
    """render_pixel at the derived gi_seed: the reference's getRay(row, col, false) and its shootRay colour under the pair's seed, folded
    as renderRectangle folds one colour; and the same pixel of a whole oracle frame, for the first pixels."""
    fx, _, o, ans = loaded(oracle, name)
    assert len(fx["p_row"]) >= grs.MIN_PIXELS
    same_bits(ans["p_ray"], fx["p_ray"], "%s: getRay(row, col, false)" % name)
    assert_same_floats(ans["p_rgb"], grs.frame_pixel(fx["p_rgb"]), "%s: frame pixels" % name)
    for i in range(3):
        frame, _ = o.render(options=grs.gi_options(oracle, grs.Q_DEPTH, gi_seed=int(fx["p_seed"][i])))
        assert_same_floats(frame[fx["p_row"][i], fx["p_col"][i]], grs.frame_pixel(fx["p_rgb"][i]), "%s: pixel %d of a whole frame" % (name, i))


@pytest.mark.parametrize("name", grs.SCENES)
def test_fixture_meets_its_conditions(oracle, name):
    fx, scene, o, _ = loaded(oracle, name)
    c = grs.census(oracle, scene, o, lambda rays, t: qs.oracle_hits(o, scene, rays, t, rrs.HIT_DTYPE), fx)
    print(name, c)
    grs.check_census(name, scene, c)
