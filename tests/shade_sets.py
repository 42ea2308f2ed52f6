"""Record sets of the direct-lighting tests (tests/test_shade_hits_host.py, tests/test_gpu_shade_hits.py) and the oracle's answers
for them.  No GPU here: numpy and OracleScene.trace / .shoot / .occluded per ray.

The expected colour of a ray's record is OracleScene.shoot(origin, direction, RAY_REFLECTION, depth=0, max_depth=0).  shoot_ray
normalises its direction on entry and crt_trace_rays walks the direction as given, so the tests use only rays whose direction is a
FIXED POINT of that normalisation: in float32, with s = (dx*dx + dy*dy) + dz*dz, sqrt(s) == 1.0 (the factor 1 / length is then 1)."""
import copy

import numpy as np

import query_sets as qs

F32 = np.float32


def is_fixed_point(rays):
    d = np.ascontiguousarray(rays, dtype=F32)[:, 3:]
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]          # Vector.cpp:114-117, evaluated in float32
    assert s.dtype == F32
    return np.sqrt(s) == F32(1.0)


def fixed_point_rays(rays):
    return np.ascontiguousarray(rays[is_fixed_point(rays)])


def normalized_like_shoot_ray(rays):
    """Vector::normalize (Vector.cpp:97-106) in float32: what shoot_ray makes of the directions."""
    d = np.ascontiguousarray(rays, dtype=F32)[:, 3:]
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    inv = (F32(1.0) / length).astype(F32)
    return (d * inv[:, None]).astype(F32)


def white_scene(scene):
    """The same geometry and lights with every diffuse albedo [1, 1, 1] and no textures: what crt_light_points computes is one
    channel of this scene's diffuse colours."""
    s = copy.deepcopy(scene)
    s.pop("textures", None)
    for m in s["materials"]:
        if m["type"] == "diffuse" or isinstance(m["albedo"], str):
            m["albedo"] = [1.0, 1.0, 1.0]
    return s


def with_lights(scene, lights):
    s = copy.deepcopy(scene)
    s["lights"] = copy.deepcopy(list(lights))
    return s


def with_material_type(scene, material, mtype):
    s = copy.deepcopy(scene)
    s["materials"][material]["type"] = mtype
    return s


def mesh_material_types(scene):
    """per mesh (object): the type name of its material"""
    return [scene["materials"][o["material_index"]]["type"] for o in scene["objects"]]


def expected_status(pkg, scene, hits):
    """CRT_SHADE_* of every record by shootRay's switch (RayTracer.cpp:430-450)."""
    by_type = {"diffuse": pkg.SHADE_DIFFUSE, "reflective": pkg.SHADE_RECURSES, "refractive": pkg.SHADE_RECURSES, "constant": pkg.SHADE_BACKGROUND}
    per_mesh = np.array([by_type[t] for t in mesh_material_types(scene)], dtype=np.uint8)
    status = np.full(len(hits), pkg.SHADE_BACKGROUND, dtype=np.uint8)
    h = hits["hit"] != 0
    status[h] = per_mesh[hits["mesh"][h]]
    return status


def oracle_colours(oracle_scene, rays):
    """shootRay without recursion: depth 0 of max_depth 0, so a reflective or refractive hit's children return the background at
    once -- those records are not compared --, a diffuse hit is calculateDiffusion and a miss the background."""
    return np.array([oracle_scene.shoot(r[:3], r[3:], qs.RAY_REFLECTION, depth=0, max_depth=0) for r in rays], dtype=F32).reshape(-1, 3)


def lights_occluded(oracle_scene, scene, hits, shadow_bias=1e-4):
    """bool [n, lights]: is light l occluded at record i (light_setup's shadow ray in float32; used to COUNT the partly and wholly
    shadowed records of a set, not to compute colours)."""
    lights = scene["lights"]
    out = np.zeros((len(hits), len(lights)), dtype=bool)
    p, n = hits["point"].astype(F32), hits["normal"].astype(F32)
    origin = (p + n * F32(shadow_bias)).astype(F32)
    for l, light in enumerate(lights):
        ld = (np.asarray(light["position"], dtype=F32)[None, :] - p).astype(F32)
        dist = np.sqrt((ld[:, 0] * ld[:, 0] + ld[:, 1] * ld[:, 1]) + ld[:, 2] * ld[:, 2])
        with np.errstate(all="ignore"):
            d = (ld * (F32(1.0) / dist)[:, None]).astype(F32)
        for i in range(len(hits)):
            out[i, l] = oracle_scene.occluded(origin[i], d[i], dist[i])
    return out


def census(pkg, oracle_scene, scene, hits):
    """The row of the issue's table for a record set: misses, diffuse / reflective / refractive hits, partly and wholly shadowed."""
    types = np.array(mesh_material_types(scene))
    hit = hits["hit"] != 0
    t = np.where(hit, types[np.where(hit, hits["mesh"], 0)], "miss")
    diffuse = np.flatnonzero(t == "diffuse")
    occ = lights_occluded(oracle_scene, scene, hits[diffuse])
    k = occ.sum(axis=1)
    return dict(misses=int((~hit).sum()), diffuse=len(diffuse), reflective=int((t == "reflective").sum()), refractive=int((t == "refractive").sum()),
                partly=int(((k > 0) & (k < occ.shape[1])).sum()), wholly=int((k == occ.shape[1]).sum()) if occ.shape[1] else 0)
