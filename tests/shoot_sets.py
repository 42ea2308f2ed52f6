"""Ray sets of the radiance-query tests (tests/test_shoot_rays_host.py, tests/test_gpu_shoot_rays.py) and the oracle's answers for
them.  No GPU here: numpy and OracleScene.shoot / .trace per ray.

The expected colour of a ray is OracleScene.shoot(origin, direction, ray_type, depth=0, max_depth): shoot_ray normalises the direction
on entry and so does crt_shoot_rays, so the sets hold directions as a caller has them -- unit vectors rounded to float32, and (the
aimed rays) differences of two points, of any length."""
import numpy as np

import query_sets as qs
import shade_sets as ss
from helpers import make, small_case

F32 = np.float32
RECURSING = ("reflective", "refractive")


def aimed_rays(scene, per_mesh=192, seed=23):
    """Rays from points in and around the room (query_sets.ROOM_LO / ROOM_HI) AT the mirror and glass meshes: for each such mesh,
    `per_mesh` times, a triangle of it drawn at random, the direction = its centroid - the origin, NOT normalised.  Most of them reach
    the triangle they aim at (some meet a wall or another object first), so their first hit recurses."""
    rng = np.random.default_rng(seed)
    types = ss.mesh_material_types(scene)
    rays = []
    for ob, t in zip(scene["objects"], types):
        if t not in RECURSING:
            continue
        v = np.asarray(ob["vertices"], dtype=np.float64).reshape(-1, 3)
        tri = np.asarray(ob["triangles"], dtype=np.int64).reshape(-1, 3)
        centroids = v[tri].mean(axis=1)
        pick = rng.integers(0, len(tri), per_mesh)
        origins = rng.uniform(qs.ROOM_LO, qs.ROOM_HI, (per_mesh, 3))
        rays.append(np.concatenate([origins, centroids[pick] - origins], axis=1))
    if not rays:
        return np.zeros((0, 6), dtype=F32)
    return np.concatenate(rays).astype(F32)


def rays_for(name, scene):
    """The set a scene is shot with: query_sets.random_rays() (4096 rays); on hw14, whose mirror and glass objects are small -- 67 of
    the random rays meet one first --, also the aimed rays (the union: the random rays come first)."""
    rays = qs.random_rays()
    if name == "hw14":
        rays = np.concatenate([rays, aimed_rays(scene)])
    return np.ascontiguousarray(rays, dtype=F32)


def shaped_rays(scene):
    """4096 rays for the launch-shape prefixes: the aimed rays FIRST (a prefix of 63 rays already recurses), then random ones."""
    return np.ascontiguousarray(np.concatenate([aimed_rays(scene), qs.random_rays()])[:4096], dtype=F32)


def normalized_rays(rays):
    """The rays as shoot_ray walks them: origin, Vector::normalize of the direction in float32 (a zero direction stays zero)."""
    rays = np.ascontiguousarray(rays, dtype=F32)
    with np.errstate(all="ignore"):
        d = ss.normalized_like_shoot_ray(rays)
    d = np.where((rays[:, 3:] == 0).all(axis=1)[:, None], rays[:, 3:], d)
    return np.ascontiguousarray(np.concatenate([rays[:, :3], d], axis=1), dtype=F32)


def first_hit_types(pkg, oracle_scene, scene, rays, ray_type=qs.RAY_REFLECTION):
    """per ray: 'miss' or the material type of the mesh shoot_ray's closest hit lies on"""
    hits = qs.oracle_hits(oracle_scene, scene, normalized_rays(rays), ray_type, pkg.HIT_DTYPE)
    types = np.array(ss.mesh_material_types(scene))
    hit = hits["hit"] != 0
    return np.where(hit, types[np.where(hit, hits["mesh"], 0)], "miss")


def recursing_first_hits(pkg, oracle_scene, scene, rays):
    t = first_hit_types(pkg, oracle_scene, scene, rays)
    return int(np.isin(t, RECURSING).sum())


def oracle_colours(oracle_scene, rays, max_depth, ray_type=qs.RAY_REFLECTION):
    return np.array([oracle_scene.shoot(r[:3], r[3:], ray_type, depth=0, max_depth=max_depth) for r in rays], dtype=F32).reshape(-1, 3)


def level_two_matters(oracle_scene, rays):
    """Does any ray's colour change between max_depth 1 and 2?  Then some ray of level 1 met a mirror or glass again: level 2 holds rays."""
    a, b = oracle_colours(oracle_scene, rays, 1), oracle_colours(oracle_scene, rays, 2)
    with np.errstate(all="ignore"):
        return bool(np.any((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))))


_CASES = {}


def case(pkg, scenes, oracle, name, tmp_path_factory):
    """A scene's tracer, oracle, its ray set (shoot_sets.rays_for) and the oracle's colours at the scene's depth: made once."""
    if name not in _CASES:
        scene, depth, folder = small_case(scenes, name, tmp_path_factory.mktemp(name))
        tracer, o = make(pkg, scenes, oracle, scene, folder)
        rays = rays_for(name, scene)
        rays.setflags(write=False)
        want = oracle_colours(o, rays, depth)
        want.setflags(write=False)
        _CASES[name] = dict(scene=scene, depth=depth, folder=folder, tracer=tracer, oracle=o, rays=rays, want=want)
    return _CASES[name]
