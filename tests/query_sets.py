"""Ray sets of the ray-query tests (tests/test_query_rays_host.py, tests/test_gpu_query_rays.py) and the oracle's answers for
them in the layout of crt_hit.  No GPU here: the builders are numpy, the answers are OracleScene.trace / .occluded per ray."""
import numpy as np

RAY_PRIMARY, RAY_SHADOW, RAY_REFLECTION, RAY_REFRACTION = range(4)   # enum RayType, Ray.h:14
ROOM_LO, ROOM_HI = [-3.5, -2.0, -8.5], [3.5, 3.0, 1.5]               # tests/test_bvh_filter.py: in and around the room


def random_rays(n=4096, seed=11):
    """tests/test_bvh_filter.py:_random_rays with default_rng(11) and the same box: origins in and around the room, any direction."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(ROOM_LO, ROOM_HI, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(np.float32)


def scene_bounds(scene):
    v = np.concatenate([np.asarray(o["vertices"], dtype=np.float64).reshape(-1, 3) for o in scene["objects"]])
    return v.min(axis=0), v.max(axis=0)


def in_plane_rays(scene, n=300, seed=7):
    """Rays that start ON a bounding plane of the scene and run IN it: d . n is exactly 0 for every triangle in that plane, the
    reference divides by it (Ray.cpp:19), and a non-primary ray gets hits at t = NaN / inf -- the rays whose filter miss the miss
    check refutes.  6 n rays (1800): for each axis, for each of lo[axis], hi[axis], n times."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(scene)
    rays = []
    for axis in range(3):
        for plane in (lo[axis], hi[axis]):
            for _ in range(n):
                o = rng.uniform(lo - 2, hi + 2)
                o[axis] = plane
                d = rng.normal(size=3)
                d[axis] = 0.0
                d /= np.linalg.norm(d)
                rays.append(np.concatenate([o, d]))
    return np.array(rays).astype(np.float32)


def triangle_bases(scene):
    """First global triangle index of every object: the flattened scene lists the objects' triangles in scene order
    (host/AccelerationStructure.cpp: flattenScene, triBase)."""
    counts = [len(np.asarray(o["triangles"]).reshape(-1, 3)) for o in scene["objects"]]
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)


def oracle_hits(oracle_scene, scene, rays, ray_type, hit_dtype):
    """OracleScene.trace for every ray, as crt_hit records (triangle index global; every field 0 where there is no hit)."""
    bases = triangle_bases(scene)
    out = np.zeros(len(rays), dtype=hit_dtype)
    for i, r in enumerate(rays):
        hit, v = oracle_scene.trace(r[:3], r[3:], ray_type)
        if hit:
            mesh = int(v[9])
            out[i] = (v[0], v[1:4], v[4:7], v[7], v[8], mesh, int(bases[mesh]) + int(v[10]), 1)
    return out


def oracle_occluded(oracle_scene, rays, max_distance):
    dist = np.broadcast_to(np.asarray(max_distance, dtype=np.float32), (len(rays),))
    return np.array([oracle_scene.occluded(r[:3], r[3:], d) for r, d in zip(rays, dist)], dtype=bool)


def non_finite_winners(hits):
    return int((hits["hit"].astype(bool) & ~np.isfinite(hits["t"])).sum())
