"""Scenes and ray sets of the scale tests (tests/test_scale_filter.py, tests/test_gpu_scale.py): the room of every other test, moved
and resized.  Every bound of the candidate filter (csrc/crt_bvh.cpp: triangle_margin; csrc/kernel_bvh.h: rho, the +-1e-12 direction
components; overlap_eps; the shadow walk's end) depends on the absolute size and position of the scene and on where a ray starts,
and at unit scale around the origin rho hides all the others.  No GPU here: numpy, and OracleScene per ray for the answers.

A CASE is (base scene, scale s, offset): `transformed` maps every position x to float32(s * x + offset).  The grid, per base scene:

    s1        the control
    s53, s1e3, s3.7e-2                      non-powers of two: every coordinate rounds anew
    hi, lo    the two scales that bracket the loss of the filter (tests/golden/scale_cases.json: found by bisection on the library's
              own verdict, tests/golden/make_golden.py: scale_cases)
    offset    s = 1 at (1000, -2000, 500): coordinates lose eleven low bits
    combined  s = 3.7e-2 at (40, -80, 20): rho comes from the offset, the margins from the triangles

and, on hw11 only, `s1e6`: beyond what kernel_bvh.h's analysis of the +-1e-12 replacement covers ("< 1e7").
"""
import copy
import json
import os

import numpy as np

import query_sets as qs

F32 = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)
HERE = os.path.dirname(os.path.abspath(__file__))
CASES_JSON = os.path.join(HERE, "golden", "scale_cases.json")

# base scenes: detail no higher than helpers.small_case's, lower for hw11 (346 and 1714 triangles)
BASES = {"hw11": dict(width=64, height=36, detail=0.15), "hw14": dict(width=64, height=36, detail=0.04)}
FAR_OFFSET, NEAR_OFFSET = (1000.0, -2000.0, 500.0), (40.0, -80.0, 20.0)
GRID = ["s1", "s53", "s1e3", "s3.7e-2", "hi", "lo", "offset", "combined"]
FIXTURE_CASES = ["hi", "lo", "s1e3", "offset"]           # tests/golden/scale_<case>.npz, on hw11
EXCLUDED = ("hw11", "s1e6")
RIM_K = (0.25, 0.5, 1.0, 2.0, 4.0)
FAR_EXTENTS = (1e2, 1e4, 1e6)
LIMIT_STEPS = (0, -1, -2, -8, 1, 2, 8)                    # float32 neighbours of L


def bracket(base):
    with open(CASES_JSON) as f:
        return json.load(f)[base]


def case_params(base, case):
    """(s, offset) of a case"""
    if case in ("hi", "lo"):
        return float(bracket(base)["S_" + case]), (0.0, 0.0, 0.0)
    return {"s1": (1.0, (0.0, 0.0, 0.0)), "s53": (53.0, (0.0, 0.0, 0.0)), "s1e3": (1.0e3, (0.0, 0.0, 0.0)),
            "s3.7e-2": (3.7e-2, (0.0, 0.0, 0.0)), "s1e6": (1.0e6, (0.0, 0.0, 0.0)),
            "offset": (1.0, FAR_OFFSET), "combined": (3.7e-2, NEAR_OFFSET)}[case]


def all_cases():
    return [(b, c) for b in BASES for c in GRID]


def base_scene(scenes, base, width=None, height=None):
    p = dict(BASES[base])
    if width:
        p.update(width=width, height=height)
    return scenes.make(base, **p)


def move(x, s, offset):
    """float32(s * x + offset), computed in float64: rounded once"""
    return (np.asarray(x, dtype=np.float64) * float(s) + np.asarray(offset, dtype=np.float64)).astype(F32)


def transformed(scene, s, offset=(0.0, 0.0, 0.0)):
    """Every vertex, the camera position and every light position become float32(s * x + offset); normals (recomputed by the
    readers from the vertices), uvs, materials and the camera matrix stay.  A light's intensity is multiplied by s * s, so that
    intensity / (4 pi r^2) stays what it was -- but the schema holds it as an unsigned integer (SceneParser.cpp:139-142), so it is
    rounded, and never below 1: at small scales the frames are brighter than the control's, which the comparisons of floats do not
    mind."""
    out = copy.deepcopy(scene)
    out["camera"]["position"] = move(scene["camera"]["position"], s, offset)
    for l, light in zip(out["lights"], scene["lights"]):
        l["position"] = move(light["position"], s, offset)
        l["intensity"] = int(min(max(1, round(light["intensity"] * float(s) * float(s))), 2 ** 31 - 1))
    for o, ob in zip(out["objects"], scene["objects"]):
        o["vertices"] = move(ob["vertices"], s, offset)
    return out


def make_case(scenes, base, case, width=None, height=None):
    s, offset = case_params(base, case)
    return transformed(base_scene(scenes, base, width, height), s, offset)


def scene_extent(scene):
    lo, hi = qs.scene_bounds(scene)
    return float((hi - lo).max())


def shortest_edge(scene):
    best = np.inf
    for o in scene["objects"]:
        v = np.asarray(o["vertices"], dtype=np.float64).reshape(-1, 3)[np.asarray(o["triangles"], dtype=np.int64).reshape(-1, 3)]
        for k in range(3):
            best = min(best, float(np.linalg.norm(v[:, (k + 1) % 3] - v[:, k], axis=1).min()))
    return best


def _unit32(v):
    """float32-rounded unit vectors (the filter path takes them: kernel_query.h, QUERY_UNIT_TOL)"""
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def _rays(origins, directions):
    rays = np.ascontiguousarray(np.concatenate([origins.astype(F32), directions.astype(F32)], axis=1), dtype=F32)
    rays.setflags(write=False)
    return rays


# ---- the ray sets
def room_rays(s, offset, n=2048):
    """query_sets.random_rays through the transform: origins in and around the room, any direction"""
    base = qs.random_rays(n)
    return _rays(move(base[:, :3], s, offset), base[:, 3:])


def far_rays(scene, n=2046, seed=31):
    """Origins 1e2, 1e4 and 1e6 scene extents from the scene's centre, in random directions, aimed at points drawn uniformly inside
    the scene's bounds: rho grows with the origin, and the walk must still find the hit.  The direction is computed from the ROUNDED
    origin, in float64."""
    rng = np.random.default_rng(seed)
    lo, hi = qs.scene_bounds(scene)
    centre, extent = 0.5 * (lo + hi), float((hi - lo).max())
    per = n // len(FAR_EXTENTS)
    origins, dirs = [], []
    for k in FAR_EXTENTS:
        u = rng.normal(size=(per, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = (centre + u * (k * extent)).astype(F32)
        target = rng.uniform(lo, hi, (per, 3))
        origins.append(o)
        dirs.append(_unit32(target - o.astype(np.float64)))
    return _rays(np.concatenate(origins), np.concatenate(dirs))


def all_triangles(scene):
    """float64 [n, 3, 3]: the corners of every triangle in the scene's (global) order"""
    return np.concatenate([np.asarray(o["vertices"], dtype=np.float64).reshape(-1, 3)[np.asarray(o["triangles"], dtype=np.int64).reshape(-1, 3)]
                           for o in scene["objects"]])


def rim_rays(scene, n_triangles=200, seed=41):
    """Rays aimed at the rim of a triangle's acceptance region (Triangle.cpp:37-57 accepts a point while each edge function is not
    below -FLT_EPSILON, i.e. up to about FLT_EPSILON / |edge| outside the edge).  200 triangles drawn at random; from an origin 1 to 3
    scene extents away on the triangle's front side, TEN rays per triangle (2000 rays: a set holds 2048 at the most, so not every edge
    of every triangle gets every kind; the edge j rotates with the triangle's number):
        0-2  at the three vertices
        3-4  at the midpoints of edges j and j + 1
        5-9  at the midpoint of edge j displaced OUTWARD, in the triangle's plane, by k * FLT_EPSILON / |edge|, k in RIM_K
    Targets in float64, then the direction rounded.  Returns (rays, triangle [n] = the global index aimed at, outside [n] = k of
    the displacement (0: the target is on the triangle's boundary))."""
    rng = np.random.default_rng(seed)
    tris = all_triangles(scene)
    extent = scene_extent(scene)
    pick = rng.choice(len(tris), n_triangles, replace=len(tris) < n_triangles)
    origins, dirs, which, outside = [], [], [], []
    for i, t in enumerate(pick):
        v = tris[t]
        normal = np.cross(v[1] - v[0], v[2] - v[0])
        normal /= np.linalg.norm(normal)
        tilt = rng.normal(size=3) * 0.3
        tilt -= normal * np.dot(tilt, normal)
        o = (v.mean(axis=0) + (normal + tilt) / np.linalg.norm(normal + tilt) * rng.uniform(1.0, 3.0) * extent).astype(F32)
        j = i % 3
        a, b = v[j], v[(j + 1) % 3]
        edge = b - a
        out_dir = np.cross(edge, normal)                  # in the plane, away from the third corner
        out_dir /= np.linalg.norm(out_dir)
        assert np.dot(out_dir, v[(j + 2) % 3] - a) < 0
        targets = [v[0], v[1], v[2], 0.5 * (a + b), 0.5 * (b + v[(j + 2) % 3])]
        ks = [0.0] * 5
        for k in RIM_K:
            targets.append(0.5 * (a + b) + out_dir * (k * FLT_EPSILON / np.linalg.norm(edge)))
            ks.append(k)
        for target, k in zip(targets, ks):
            origins.append(o)
            dirs.append(_unit32(target - o.astype(np.float64)))
            which.append(t)
            outside.append(k)
    return _rays(np.array(origins), np.array(dirs)), np.array(which, dtype=np.int64), np.array(outside)


def float32_neighbour(x, steps):
    x = F32(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, F32(np.inf) if steps > 0 else F32(-np.inf))
    return x


def reference_length(point, origin):
    """Vector::length of point - origin in float32 (Vector.cpp:114-117): what AccelerationStructure.cpp:56-94 compares with the limit"""
    d = (np.asarray(point, dtype=F32) - np.asarray(origin, dtype=F32)).astype(F32)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def limit_rays(scene, rays, hits, n=146):
    """The occlusion query's boundary length(point - origin) <= max_distance: the first `n` of `rays` whose closest hit (`hits`: the
    oracle's records) lies on an occluding mesh -- one that is not refractive.  Each ray comes FOURTEEN times, in two groups of seven
    limits: L and its 1, 2 and 8 float32 neighbours below and above, first for L = length(point - origin) evaluated as the
    reference evaluates it, then for L = the hit's distance t.  (With the first L alone every ray flips at L itself: the occluding
    hit IS that hit, and the comparison is with the very number.  t is what a caller holds who asks "is there anything before this
    hit"; it lies within a few neighbours of the length, on either side.)
    Returns (rays [14 n, 6], limits [14 n], step [14 n])."""
    refractive = np.array([scene["materials"][o["material_index"]]["type"] == "refractive" for o in scene["objects"]])
    ok = (hits["hit"] != 0) & ~refractive[hits["mesh"]] & np.isfinite(hits["t"])
    idx = np.flatnonzero(ok)[:n]
    L = reference_length(hits["point"][idx], rays[idx, :3])
    out_rays = np.repeat(rays[idx], 2 * len(LIMIT_STEPS), axis=0)
    limits = np.array([float32_neighbour(b, k) for l, t in zip(L, hits["t"][idx]) for b in (l, t) for k in LIMIT_STEPS], dtype=F32)
    steps = np.tile(np.array(LIMIT_STEPS), 2 * len(idx))
    return _rays(out_rays[:, :3], out_rays[:, 3:]), limits, steps


def flip_histogram(occluded, steps):
    """Per ray of a limit set: the smallest step at which the oracle says "occluded" (None: at none of the seven); a ray FLIPS when it
    is occluded at some limits and not at others.  Returns {step: rays whose first occluded limit it is} over the flipping rays."""
    order = np.argsort(np.array(LIMIT_STEPS))
    occ = occluded.reshape(-1, len(LIMIT_STEPS))[:, order]
    sorted_steps = np.array(LIMIT_STEPS)[order]
    flips = occ.any(axis=1) & ~occ.all(axis=1)
    first = sorted_steps[occ[flips].argmax(axis=1)]
    return {int(k): int((first == k).sum()) for k in sorted_steps if (first == k).any()}


# ---- a case with its ray sets and the oracle's answers, made once per session and shared (read-only) by the tests
_CASES = {}


def case_data(pkg, scenes, oracle, base, case):
    key = (base, case)
    if key not in _CASES:
        s, offset = case_params(base, case)
        scene = make_case(scenes, base, case)
        o = oracle.OracleScene(scenes.to_blob(scene))
        d = dict(base=base, case=case, s=s, offset=offset, scene=scene, oracle=o, extent=scene_extent(scene))
        d["room"] = room_rays(s, offset)
        d["far"] = far_rays(scene)
        d["rim"], d["rim_triangle"], d["rim_outside"] = rim_rays(scene)
        for name in ("room", "far", "rim"):
            for ray_type in (qs.RAY_PRIMARY, qs.RAY_REFLECTION):
                hits = qs.oracle_hits(o, scene, d[name], ray_type, pkg.HIT_DTYPE)
                hits.setflags(write=False)
                d[name, ray_type] = hits
        d["limit"], d["limit_dist"], d["limit_step"] = limit_rays(scene, d["room"], d["room", qs.RAY_REFLECTION])
        d["limit_occluded"] = qs.oracle_occluded(o, d["limit"], d["limit_dist"])
        for k in ("limit_dist", "limit_step", "limit_occluded", "rim_triangle", "rim_outside"):
            d[k].setflags(write=False)
        _CASES[key] = d
    return _CASES[key]


def rim_census(d, ray_type=qs.RAY_PRIMARY):
    """(rays the oracle answers with the triangle aimed at although the float64 target lies OUTSIDE it, rays that miss that triangle)"""
    hits = d["rim", ray_type]
    on_target = (hits["hit"] != 0) & (hits["triangle"] == d["rim_triangle"])
    return int((on_target & (d["rim_outside"] > 0)).sum()), int((~on_target).sum())
