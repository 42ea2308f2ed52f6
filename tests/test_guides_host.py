"""The chain guides' rule on the CPU (tests/guide_sets.py restates include/crt_hip.h, "Chain guides"): the restated child ray is held to
the oracle, the scenes of tests/test_gpu_guides.py have the pixels those tests rely on, and the restatements of the filter say what the
chain guides are worth on the mirror-wall scene BEFORE any GPU run.  No GPU here."""
import numpy as np

import adaptive_sets as ads
import denoise_sets as dns
import guide_sets as g
import shoot_gi_sets as gs
from query_sets import RAY_PRIMARY

_walks = {}


def walks(scenes, oracle, which, bounces, camera=None):
    key = (which, bounces, camera)
    if key not in _walks:
        o = g.oracle_scene(scenes, oracle, which)
        scene = {"white": g.white_mirror_scene, "wall": g.mirror_wall_scene}[which](scenes)
        if camera:
            o.set_camera(camera[0], gs.look_at(*camera))
        rays, fixed = g.fixed_point(gs.camera_rays(o)) if which == "white" else (gs.camera_rays(o), None)
        _walks[key] = dict(o=o, scene=scene, rays=rays, fixed=fixed, walk=g.walk_all(o, scene, rays, RAY_PRIMARY, bounces))
    return _walks[key]


def pinned_rays(w):
    """1 or more bounces, all reflective, not cut, terminal DIFFUSE -- and a ray normalize3 leaves as it is (guide_sets.fixed_point)"""
    k = w["walk"]
    return w["fixed"] & (k["status"] >= 1) & (k["status"] < g.CUT) & k["all_reflective"] & (k["kinds"] == g.DIFFUSE)


def test_the_restated_reflection_is_the_oracles(scenes, oracle):
    """on the white-mirror copy of hw11 a mirror returns 0 + 1 * (its child's colour): shootRay of the camera's ray is shootRay of the
    chain's terminal ray at its depth, in every bit -- one ulp in a restated child ray moves the terminal hit and with it the colour"""
    w = walks(scenes, oracle, "white", 8, g.MIRROR_CAMERA)
    sel = np.flatnonzero(pinned_rays(w))
    assert len(sel) >= 30, len(sel)
    o, k = w["o"], w["walk"]
    for i in sel:
        whole = o.shoot(w["rays"][i, :3], w["rays"][i, 3:], RAY_PRIMARY, 0, 8)
        last = o.shoot(k["last_rays"][i, :3], k["last_rays"][i, 3:], int(k["last_types"][i]), int(k["status"][i]), 8)
        assert np.array_equal(whole.view(np.uint32), last.view(np.uint32)), (i, whole, last)


def test_the_restated_transmission_obeys_snell(scenes):
    """the transmission ray against Snell's law in float64, entering and leaving glass, and total internal reflection"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        p = rng.uniform(-2, 2, size=3)
        origin, direction, kind = g.child_ray(True, 1.5, d.astype(np.float32), p.astype(np.float32), n.astype(np.float32), 1e-4, 1e-4)
        cos_i = -float(d @ n)
        m, eta = (n, 1.0 / 1.5) if cos_i > 0 else (-n, 1.5)
        cos_i = abs(cos_i)
        sin2 = eta * eta * (1.0 - cos_i * cos_i)
        if sin2 < 1.0 - 1e-6:
            want = eta * d + (eta * cos_i - np.sqrt(1.0 - sin2)) * m
            assert kind == g.RAY_REFRACTION and np.allclose(direction, want / np.linalg.norm(want), atol=2e-5)
            assert np.allclose(origin, p - m * 1e-4, atol=1e-6)
        elif sin2 > 1.0 + 1e-6:
            want = d - 2.0 * float(d @ m) * m
            assert kind == g.RAY_REFLECTION and np.allclose(direction, want, atol=2e-5)
            assert np.allclose(origin, p + m * 1e-4, atol=1e-6)


def test_zero_bounces_is_the_first_hit(scenes, oracle):
    import query_sets as qs
    w = walks(scenes, oracle, "wall", 0)
    want = qs.oracle_hits(w["o"], w["scene"], w["rays"], RAY_PRIMARY, g.HIT_DTYPE)
    assert w["walk"]["records"].tobytes() == want.tobytes()
    specular = np.array([g.material_of(w["scene"], int(m))["type"] in ("reflective", "refractive") for m in want["mesh"]]) & (want["hit"] != 0)
    assert np.array_equal(w["walk"]["status"], np.where(specular, g.CUT, 0).astype(np.uint8))


def wall_pixels(scenes, oracle):
    """the pixels whose first hit is the mirror quad and whose chain ends on a diffuse mesh, and those chains' terminal meshes"""
    first, chain = walks(scenes, oracle, "wall", 0), walks(scenes, oracle, "wall", 4)
    n_meshes = len(first["scene"]["objects"])
    records = first["walk"]["records"]
    where = (records["hit"] != 0) & (records["mesh"] == n_meshes - 1) & (chain["walk"]["kinds"] == g.DIFFUSE)
    return where, chain["walk"]["records"]["mesh"][where] % n_meshes, first["walk"]["records"], chain["walk"]["records"]


def test_the_mirror_wall_has_the_pixels(scenes, oracle):
    where, terminal, _, _ = wall_pixels(scenes, oracle)
    assert where.sum() >= 150, where.sum()
    shares = sorted((float((terminal == m).mean()) for m in np.unique(terminal)), reverse=True)
    assert len(shares) >= 2 and shares[1] >= 0.2, shares


_measured = {}


def restated_measure(scenes, oracle):
    """(RMSE of the unfiltered mean, A: the default filter under first-hit guides, B: under chain guides) over wall_pixels, against the
    oracle's 64-sample frame; the 4 samples a pixel are the oracle's, the chain guides the host walk's.  Made once."""
    if not _measured:
        where, _, first, chain = wall_pixels(scenes, oracle)
        o = g.oracle_scene(scenes, oracle, "wall")
        colours = g.oracle_sample_colours(o, oracle, g.FRAME["samples"])
        state = ads.run(colours, (g.FRAME["samples"], g.FRAME["samples"], 0.05, 1e-4))
        mean, var = dns.variance(state["total"], state["sq"], state["counts"])
        truth, _ = o.render(options=oracle.make_options(g.FRAME["depth"], use_gi=1, gi_sample_size=g.FRAME["gi_samples"], rays_per_pixel=g.FRAME["truth"],
                                                        gi_seed=gs.SEED))
        a = dns.denoise(mean, var, first, gs.H, gs.W, dns.DEFAULTS)[0]
        b = dns.denoise(mean, var, chain, gs.H, gs.W, dns.DEFAULTS)[0]
        _measured.update(where=where, truth=truth, mean=mean, var=var, chain=chain,
                         rmse=(dns.rmse(mean, truth, where), dns.rmse(a, truth, where), dns.rmse(b, truth, where)))
    return _measured


def test_the_restatements_keep_what_the_mirror_shows(scenes, oracle):
    """measured here: the mean 0.03592, A 0.04117, B 0.03285, B / A 0.798 over 296 pixels"""
    noisy, a, b = restated_measure(scenes, oracle)["rmse"]
    print("mirror wall, 4 samples: RMSE the mean %.5f, first-hit guides A %.5f, chain guides B %.5f, B / A %.4f" % (noisy, a, b, b / a))
    assert b < a
