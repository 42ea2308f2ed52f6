"""Ray sets that pin the ray, lighting and radiance queries to the REAL reference (tests/golden/query_<scene>.npz, made by
tests/golden/make_golden.py queries; read by tests/test_query_reference_host.py and tests/test_gpu_query_reference.py), and the answers
of a backend -- the reference binary or the oracle -- for them.  numpy only, fixed seeds, no GPU.

A set is built FROM the reference's own answers (origins at its hit points, midpoints between its entry and exit hits, occlusion
distances at the length of its own hit), so the builder takes the backend's trace function.  Classes (label = index into CLASSES):
  random         query_sets.random_rays: origins in and around the room, any direction
  outside        origins outside the scene's box: aimed at it, past it, away from it
  on_surface     origins exactly at the reference's hit points of the random set, at triangle vertices and at edge midpoints; directions
                 +n, -n and in the triangle's plane: t == 0, -0, and a zero denominator (Ray.cpp:19-20)
  inside         origins inside the mirror and the glass meshes (midpoint of the reference's entry and exit hit), any direction
  through_glass  from behind the glass mesh through it and out of the room's open side: rays whose only blocker is the glass
  in_plane       query_sets.in_plane_rays: winners at t = NaN / inf
  axis_tie       axis-parallel rays in the split planes of the top-level tree and of one mesh tree, and through vertices and edge
                 midpoints shared by triangles
  scaled         the first rays of the random set with directions times 0.5, 3, 1e-3 and 1e3
The occlusion set pairs every blocked ray of the random and scaled classes (and the through_glass rays) with eight distances: L =
|hitPoint - origin| of the reference's shadow-type hit in float32 (AccelerationStructure.cpp:74), its two float32 neighbours, 0, -1,
inf, NaN and one distance between the first and the second surface."""
import os

import numpy as np

import query_sets as qs

F32 = np.float32
CLASSES = ["random", "outside", "on_surface", "inside", "through_glass", "in_plane", "axis_tie", "scaled"]
SCALES = [0.5, 3.0, 1e-3, 1e3]
RAY_TYPES = [qs.RAY_PRIMARY, qs.RAY_SHADOW, qs.RAY_REFLECTION, qs.RAY_REFRACTION]
DEPTHS = [0, 1, 5]
OCC_KINDS = ["L", "below_L", "above_L", "zero", "minus_one", "inf", "nan", "between"]
SCENES = ["hw11", "hw14", "hw12", "mixed", "tie_ab", "tie_ba"]
FULL_SCENES = SCENES[:4]              # the tie scenes are two quads: no glass, no mirror, no depth
# A winner at t = NaN / inf has a non-finite point; every ray shootRay sends on from it has NaN coordinates, passes every box test
# (BoundingBox.h:85-108) and is tested against every triangle of every leaf of every tree.  In the deep trees of these two scenes that
# is seconds per ray on the CPU and on the GPU alike (hw14: about 6 s a walk, five walks per winner and depth), so THERE shootRay and
# shade_hits are not evaluated for the non-primary rays with such a winner; their hit records are compared like all others, and the
# shading of non-finite winners is pinned on hw11, mixed and the tie scenes (several hundred of them).
DEEP_SCENES = ["hw14", "hw12"]
FIXTURE_SEED, LIVE_SEED = 20250101, 77
COUNTS = dict(random=300, outside=180, surface_hits=40, surface_vertices=25, surface_edges=25, inside=80, through_glass=60, in_plane=40,
              axis=30, shared=30, scaled=100)
HIT_DTYPE = np.dtype([("t", F32), ("point", F32, 3), ("normal", F32, 3), ("u", F32), ("v", F32), ("mesh", np.uint32), ("triangle", np.uint32),
                      ("hit", np.uint32)])   # crt_hit (include/crt_hip.h)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------------------------------ scenes
def tie_scene(order):
    """Two coincident quads of two meshes (one diffuse, one a mirror) and a light in front of them: every hit is an exact tie between
    the meshes, decided by the order in which the top-level walk collects them (KDTree.cpp:156-166).  order: "ab" or "ba"."""
    quad = np.array([[-1, -1, -3], [1, -1, -3], [1, 1, -3], [-1, 1, -3]], dtype=F32)
    tris = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32)
    a = {"material_index": 0, "vertices": quad.copy(), "triangles": tris.copy()}
    b = {"material_index": 1, "vertices": quad.copy(), "triangles": tris.copy()}
    return {"settings": {"background_color": [0.1, 0.2, 0.3], "image_settings": {"width": 32, "height": 24, "bucket_size": 8}},
            "camera": {"matrix": [1, 0, 0, 0, 1, 0, 0, 0, 1], "position": [0, 0, 0]},
            "lights": [{"intensity": 200, "position": [0.3, 0.4, -1.0]}],
            "materials": [{"type": "diffuse", "albedo": [0.9, 0.2, 0.1], "smooth_shading": False},
                          {"type": "reflective", "albedo": [0.8, 0.8, 0.8], "smooth_shading": False}],
            "objects": [a, b] if order == "ab" else [b, a]}


def make_scene(scenes, name):
    if name == "hw11":
        return scenes.make("hw11", width=128, height=72, detail=0.2)
    if name == "hw14":
        return scenes.make("hw14", width=112, height=63, detail=0.03)
    if name == "hw12":
        return scenes.make("hw12", width=96, height=54, detail=0.06, bitmap_size=32)
    if name == "mixed":
        import degenerate_sets
        return degenerate_sets.build(scenes, "mixed")[0]
    return tie_scene(name[4:])


def material_kinds(scene):
    return np.array([scene["materials"][o["material_index"]]["type"] for o in scene["objects"]])


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _mesh(scene, m):
    o = scene["objects"][m]
    return np.asarray(o["vertices"], dtype=F32).reshape(-1, 3), np.asarray(o["triangles"], dtype=np.int64).reshape(-1, 3)


def _face_normal(p):
    n = np.cross((p[1] - p[0]).astype(np.float64), (p[2] - p[0]).astype(np.float64))
    length = np.linalg.norm(n)
    return n / length if length > 0 else np.array([0.0, 0.0, 1.0])


def _in_plane_direction(n, rng):
    d = np.cross(n, rng.normal(size=3))
    return _unit(d)


# ------------------------------------------------------------------------------------------------------------------------ the rays
def build(scene, oracle_scene, trace, seed):
    """-> dict(rays float32 [n, 6], labels uint8 [n], occ_index int32 [m], occ_kind uint8 [m], occ_dist float32 [m]).
    trace(rays, ray_type) -> hit records with fields hit, point, normal (the reference's); oracle_scene: for tree() only."""
    rng = np.random.default_rng(seed)
    lo, hi = qs.scene_bounds(scene)
    flat = bool(np.any(hi - lo == 0))                      # a tie scene
    kinds = material_kinds(scene)
    parts = {}

    # random
    if flat:
        o = rng.uniform([-2, -2, -5], [2, 2, -1], (COUNTS["random"], 3))
        parts["random"] = np.concatenate([o, _unit(rng.normal(size=(COUNTS["random"], 3)))], axis=1).astype(F32)
    else:
        parts["random"] = qs.random_rays(COUNTS["random"], seed=seed)
    random_hits = trace(parts["random"], qs.RAY_REFLECTION)

    # outside: on a shell around the box
    n = COUNTS["outside"]
    size = np.maximum(hi - lo, 1.0)
    o = rng.uniform(lo - size, hi + size, (n, 3))
    face = rng.integers(0, 6, n)
    for i in range(n):
        axis, side = face[i] % 3, face[i] // 3
        o[i, axis] = (hi[axis] + rng.uniform(0.5, 3.0)) if side else (lo[axis] - rng.uniform(0.5, 3.0))
    inside_point = rng.uniform(lo, hi, (n, 3))
    third = n // 3
    d = inside_point - o                                                    # at the box
    d[third:2 * third] = (inside_point + (hi - lo) * rng.choice([-1.5, 1.5], (n, 3)) - o)[third:2 * third]   # past it
    d[2 * third:] = -d[2 * third:]                                          # away from it
    parts["outside"] = np.concatenate([o, _unit(d)], axis=1).astype(F32)

    # on the surface
    surf = []
    hit_idx = np.flatnonzero(random_hits["hit"] & np.isfinite(random_hits["point"]).all(axis=1))
    for i in rng.choice(hit_idx, min(COUNTS["surface_hits"], len(hit_idx)), replace=False):
        p, nrm = random_hits["point"][i].astype(np.float64), random_hits["normal"][i].astype(np.float64)
        for d in (nrm, -nrm, _in_plane_direction(nrm, rng)):
            surf.append(np.concatenate([p, d]))
    for what, count in (("vertex", COUNTS["surface_vertices"]), ("edge", COUNTS["surface_edges"])):
        for _ in range(count):
            v, t = _mesh(scene, rng.integers(len(scene["objects"])))
            p = v[t[rng.integers(len(t))]]
            nrm = _face_normal(p)
            k = rng.integers(3)
            at = p[k].astype(np.float64) if what == "vertex" else ((p[k] + p[(k + 1) % 3]) * F32(0.5)).astype(np.float64)
            edge = (p[(k + 1) % 3] - p[k]).astype(np.float64)
            along = _unit(edge) if np.linalg.norm(edge) > 0 else _in_plane_direction(nrm, rng)
            for d in (nrm, -nrm, along):
                surf.append(np.concatenate([at, d]))
    parts["on_surface"] = np.array(surf).astype(F32)

    # inside the mirror and the glass meshes
    inner, glass = [], [m for m in range(len(kinds)) if kinds[m] == "refractive"]
    closed = [m for m in range(len(kinds)) if kinds[m] in ("reflective", "refractive")] if not flat else []
    for m in closed:
        v, _ = _mesh(scene, m)
        blo, bhi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
        centre, radius = (blo + bhi) / 2, np.linalg.norm(bhi - blo) / 2
        k = COUNTS["inside"] // len(closed)
        aim = centre + rng.uniform(-0.25, 0.25, (k, 3)) * (bhi - blo)
        start = aim + _unit(rng.normal(size=(k, 3))) * (radius + 0.05)
        entry_rays = np.concatenate([start, _unit(aim - start)], axis=1).astype(F32)
        entry = trace(entry_rays, qs.RAY_REFLECTION)
        step = entry["point"] + entry_rays[:, 3:] * F32(1e-3)
        leave = trace(np.concatenate([step, entry_rays[:, 3:]], axis=1).astype(F32), qs.RAY_REFLECTION)
        ok = (entry["hit"] == 1) & (entry["mesh"] == m) & (leave["hit"] == 1) & (leave["mesh"] == m)
        mid = ((entry["point"] + leave["point"]) * F32(0.5))[ok]
        inner.append(np.concatenate([mid, _unit(rng.normal(size=(len(mid), 3)))], axis=1))
    parts["inside"] = np.concatenate(inner).astype(F32) if inner else np.zeros((0, 6), dtype=F32)

    # through the glass and out of the open side (+z)
    through = []
    for m in glass if not flat else []:
        v, _ = _mesh(scene, m)
        blo, bhi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
        k = COUNTS["through_glass"] // len(glass)
        q = (blo + bhi) / 2 + rng.uniform(-0.3, 0.3, (k, 3)) * (bhi - blo)
        p = np.stack([rng.uniform(lo[0] * 0.6, hi[0] * 0.6, k), rng.uniform(lo[1] * 0.4, hi[1] * 0.6, k), np.full(k, hi[2] + 1.5)], axis=1)
        back = q + _unit(q - p) * (np.linalg.norm(bhi - blo) / 2 + 0.1)
        through.append(np.concatenate([back, _unit(p - back)], axis=1))
    parts["through_glass"] = np.concatenate(through).astype(F32) if through else np.zeros((0, 6), dtype=F32)

    # in a bounding plane of the scene
    parts["in_plane"] = qs.in_plane_rays(scene, COUNTS["in_plane"], seed=seed + 1)

    # axis-parallel rays in split planes, and through shared vertices and edge midpoints
    axis_rays = []
    biggest = int(np.argmax([len(o["triangles"]) for o in scene["objects"]]))
    for tree in (-1, biggest):
        boxes, links, _ = oracle_scene.tree(tree)
        inner_nodes = np.flatnonzero((links[:, 3] == 0) & (links[:, 0] != 0xFFFFFFFF) & (links[:, 1] != 0xFFFFFFFF))
        for node in (rng.choice(inner_nodes, COUNTS["axis"], replace=True) if len(inner_nodes) else []):
            c0 = boxes[links[node, 0]]
            split = int(np.flatnonzero(c0[3:] != boxes[node, 3:])[0]) if np.any(c0[3:] != boxes[node, 3:]) else 0
            run = (split + 1 + rng.integers(2)) % 3                      # the axis the ray runs along: in the split plane
            o = rng.uniform(boxes[node, :3], boxes[node, 3:]).astype(np.float64)
            o[split] = c0[3 + split]
            sign = rng.choice([-1.0, 1.0])
            o[run] = (lo[run] - 1.0) if sign > 0 else (hi[run] + 1.0)
            d = np.zeros(3)
            d[run] = sign
            axis_rays.append(np.concatenate([o, d]))
    for k in range(COUNTS["shared"]):
        v, t = _mesh(scene, rng.integers(len(scene["objects"])) if k % 2 else biggest)
        p = v[t[rng.integers(len(t))]]
        j = rng.integers(3)
        at = p[j].astype(np.float64) if k % 4 < 2 else ((p[j] + p[(j + 1) % 3]) * F32(0.5)).astype(np.float64)
        run = int(rng.integers(3))
        sign = rng.choice([-1.0, 1.0])
        o = at.copy()
        o[run] = (lo[run] - 1.0) if sign > 0 else (hi[run] + 1.0)
        d = np.zeros(3)
        d[run] = sign
        axis_rays.append(np.concatenate([o, d]))
    parts["axis_tie"] = np.array(axis_rays).astype(F32)

    # scaled directions
    base = parts["random"][:COUNTS["scaled"]]
    scaled = []
    for s in SCALES:
        r = base.copy()
        r[:, 3:] *= F32(s)
        scaled.append(r)
    parts["scaled"] = np.concatenate(scaled)

    rays = np.concatenate([parts[c] for c in CLASSES]).astype(F32)
    labels = np.concatenate([np.full(len(parts[c]), k, dtype=np.uint8) for k, c in enumerate(CLASSES)])

    # occlusion distances
    cand = np.flatnonzero(np.isin(labels, [CLASSES.index("random"), CLASSES.index("scaled"), CLASSES.index("through_glass")]))
    first = trace(rays[cand], qs.RAY_SHADOW)
    blocked = first["hit"] == 1
    cand, first = cand[blocked], first[blocked]
    with np.errstate(all="ignore"):
        L = length32(first["point"] - rays[cand, :3])
        unit = rays[cand, 3:] / length32(rays[cand, 3:])[:, None]
        second = trace(np.concatenate([first["point"] + unit * F32(1e-3), rays[cand, 3:]], axis=1).astype(F32), qs.RAY_SHADOW)
        gap = np.where(second["hit"] == 1, length32(second["point"] - first["point"]), L)
        between = (L + F32(0.5) * gap).astype(F32)
    dist = np.stack([L, np.nextafter(L, F32(0)), np.nextafter(L, F32(np.inf)), np.zeros_like(L), np.full_like(L, -1), np.full_like(L, np.inf),
                     np.full_like(L, np.nan), between], axis=1).astype(F32)
    return {"rays": rays, "labels": labels, "occ_index": np.repeat(cand, len(OCC_KINDS)).astype(np.int32),
            "occ_kind": np.tile(np.arange(len(OCC_KINDS), dtype=np.uint8), len(cand)), "occ_dist": dist.reshape(-1)}


def length32(v):
    """Vector::length in float32 (Vector.cpp: sqrtf(x x + y y + z z), summed left to right)"""
    v = np.asarray(v, dtype=F32)
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2], dtype=F32)


# ------------------------------------------------------------------------------------------------------------------------ answers
def crt_hits(scene, ref_hits, dtype=HIT_DTYPE):
    """The reference driver's records as crt_hit records: the triangle index global (query_sets.triangle_bases), and u, v as the ABI
    defines them -- Triangle::getBarycentricCoordinates for a smooth or textured material, otherwise 0 (include/crt_hip.h; the
    reference's textured build computes them for every hit, KDTree.cpp:172-190, its other build has no such members)."""
    bases = qs.triangle_bases(scene)
    uses_uv = np.array([bool(scene["materials"][o["material_index"]].get("smooth_shading")) or
                        isinstance(scene["materials"][o["material_index"]]["albedo"], str) for o in scene["objects"]])
    out = np.zeros(len(ref_hits), dtype=dtype)
    hit = ref_hits["hit"] == 1
    for f in ("t", "point", "normal", "mesh", "hit"):
        out[f][hit] = ref_hits[f][hit]
    out["triangle"][hit] = bases[ref_hits["mesh"][hit]] + ref_hits["triangle"][hit]
    keep = hit & uses_uv[np.where(hit, ref_hits["mesh"], 0)]
    out["u"][keep], out["v"][keep] = ref_hits["u"][keep], ref_hits["v"][keep]
    return out


def shoot_skip(name, hits):
    """bool [n]: the rays for which shootRay is not evaluated as a non-primary ray (see DEEP_SCENES); hits: of a non-primary type"""
    skip = (hits["hit"] == 1) & ~np.isfinite(hits["t"])
    return skip if name in DEEP_SCENES else np.zeros_like(skip)


def _shoot_all(shoot, rays, skip):
    """shoot(rays, types) -> [len(types), len(DEPTHS), n, 3]: primary for every ray, the other types for the rays not skipped (0 there)"""
    out = {}
    keep = np.flatnonzero(~skip)
    primary, others = shoot(rays, [qs.RAY_PRIMARY]), shoot(rays[keep], RAY_TYPES[1:])
    for j, d in enumerate(DEPTHS):
        out[(qs.RAY_PRIMARY, d)] = np.ascontiguousarray(primary[0, j])
        for i, t in enumerate(RAY_TYPES[1:]):
            full = np.zeros((len(rays), 3), dtype=F32)
            full[keep] = others[i, j]
            out[(t, d)] = full
    return out


def reference_answers(oracle_api, blob, scene, rs, name, check_plain=True):
    """The real reference's answers for a ray set, in the fixture's layout: hits[type] as crt_hit records, occ / occ_gi bool [m],
    shoot[(type, depth)] float32 [n, 3]."""
    out = {"hits": {}, "shoot": {}}
    tex = oracle_api.reference_trace(blob, rs["rays"], RAY_TYPES, textured=True)
    if check_plain and not scene.get("textures"):      # the build without textures answers the same, and has no u, v
        plain = oracle_api.reference_trace(blob, rs["rays"], RAY_TYPES, textured=False)
        for f in ("t", "point", "normal", "mesh", "triangle", "hit"):
            assert np.array_equal(plain[f].view(np.uint32), tex[f].view(np.uint32)), f
    for i, t in enumerate(RAY_TYPES):
        out["hits"][t] = crt_hits(scene, tex[i])
    out["shoot_skip"] = shoot_skip(name, out["hits"][qs.RAY_REFLECTION])
    out["shoot"] = _shoot_all(lambda rays, types: oracle_api.reference_shoot(blob, rays, types, DEPTHS), rs["rays"], out["shoot_skip"])
    occ_rays = rs["rays"][rs["occ_index"]]
    out["occ"] = oracle_api.reference_occluded(blob, occ_rays, rs["occ_dist"])
    out["occ_gi"] = oracle_api.reference_occluded(blob, occ_rays, rs["occ_dist"], gi=True)
    return out


def oracle_answers(oracle_scene, scene, rs, gi_occluded, name):
    """The oracle's answers in the same layout.  gi_occluded(origin, direction, distance): the oracle's no-mesh-skipped rule."""
    out = {"hits": {}, "shoot": {}}
    for t in RAY_TYPES:
        out["hits"][t] = qs.oracle_hits(oracle_scene, scene, rs["rays"], t, HIT_DTYPE)
    out["shoot_skip"] = shoot_skip(name, out["hits"][qs.RAY_REFLECTION])

    def shoot(rays, types):
        return np.array([[[oracle_scene.shoot(r[:3], r[3:], t, 0, d) for r in rays] for d in DEPTHS] for t in types], dtype=F32).reshape(
            len(types), len(DEPTHS), len(rays), 3)
    out["shoot"] = _shoot_all(shoot, rs["rays"], out["shoot_skip"])
    occ_rays = rs["rays"][rs["occ_index"]]
    out["occ"] = qs.oracle_occluded(oracle_scene, occ_rays, rs["occ_dist"])
    out["occ_gi"] = np.array([gi_occluded(r[:3], r[3:], d) for r, d in zip(occ_rays, rs["occ_dist"])], dtype=bool)
    return out


# ------------------------------------------------------------------------------------------------------------------------ conditions
def census(scene, rs, ans):
    """What makes a set worth having, counted from the reference's answers."""
    labels, background = rs["labels"], np.asarray(scene["settings"]["background_color"], dtype=F32)
    cls = lambda name: labels == CLASSES.index(name)
    refl = ans["hits"][qs.RAY_REFLECTION]
    kind = rs["occ_kind"].reshape(-1, len(OCC_KINDS))[0]
    occ = ans["occ"].reshape(-1, len(OCC_KINDS))
    assert np.array_equal(kind, np.arange(len(OCC_KINDS)))
    differs = np.zeros(len(labels), dtype=bool)
    for f in HIT_DTYPE.names:
        a, b = ans["hits"][qs.RAY_PRIMARY][f], refl[f]
        differs |= (a != b).reshape(len(labels), -1).any(axis=1) & ~(np.isnan(a) & np.isnan(b)).reshape(len(labels), -1).all(axis=1)
    return {
        "hits": {t: int(ans["hits"][t]["hit"].sum()) for t in RAY_TYPES},
        "misses": {t: int((ans["hits"][t]["hit"] == 0).sum()) for t in RAY_TYPES},
        "class_hits": {c: int(refl["hit"][cls(c)].sum()) for c in CLASSES},
        "class_rays": {c: int(cls(c).sum()) for c in CLASSES},
        "non_finite_in_plane": int((refl["hit"].astype(bool) & ~np.isfinite(refl["t"]) & cls("in_plane")).sum()),
        "non_finite": int((refl["hit"].astype(bool) & ~np.isfinite(refl["t"])).sum()),
        "flips_at_L": int((~occ[:, OCC_KINDS.index("below_L")] & occ[:, OCC_KINDS.index("L")]).sum()),
        "glass_skip": int((~occ[:, OCC_KINDS.index("inf")] & (refl["hit"][rs["occ_index"].reshape(-1, len(OCC_KINDS))[:, 0]] == 1)).sum()),
        "inside_not_background": int((ans["shoot"][(qs.RAY_REFLECTION, 5)][cls("inside")] != background).any(axis=1).sum()),
        "depth_1_vs_5": int((bits(ans["shoot"][(qs.RAY_REFLECTION, 1)]) != bits(ans["shoot"][(qs.RAY_REFLECTION, 5)])).any(axis=1).sum()),
        "types_differ": int(differs.sum()),
        "occlusion_pairs": int(len(rs["occ_index"])),
    }


def check_census(name, c):
    """The conditions a fixture has to meet (the generator asserts them before it writes, tests/test_query_reference_host.py on the
    committed files).  The tie scenes are two quads without glass, mirror recursion or a room: the conditions on those do not apply."""
    for t in RAY_TYPES:
        assert c["hits"][t] >= 100 and c["misses"][t] >= 100, (name, t, c)
    assert c["types_differ"] >= 50, (name, c)
    assert c["flips_at_L"] >= 20, (name, c)
    assert c["non_finite_in_plane"] >= 20, (name, c)
    if name in FULL_SCENES:
        assert c["glass_skip"] >= 20, (name, c)
        assert c["inside_not_background"] >= 20, (name, c)
        if name == "hw11":
            assert c["depth_1_vs_5"] >= 20, (name, c)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------ fixtures
def _rows_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1)


def save_fixture(path, blob, rs, ans):
    """One array in full per family (hits: reflection type; colours: reflection type at the deepest depth), the others as the rows in
    which they differ from it -- most rows are the same for every non-primary type and every depth."""
    out = {"blob": np.frombuffer(blob, dtype=np.uint8), "class_names": np.array(CLASSES), "occ_kind_names": np.array(OCC_KINDS),
           "occ": ans["occ"], "occ_gi": ans["occ_gi"], "shoot_skip": ans["shoot_skip"]}
    out.update({k: rs[k] for k in ("rays", "labels", "occ_index", "occ_kind", "occ_dist")})
    base = ans["hits"][qs.RAY_REFLECTION]
    out["hits_base"] = base
    for t in RAY_TYPES:
        rows = np.flatnonzero(_rows_differ(ans["hits"][t], base))
        out["hits_rows_%d" % t], out["hits_diff_%d" % t] = rows.astype(np.int32), ans["hits"][t][rows]
    cbase = ans["shoot"][(qs.RAY_REFLECTION, DEPTHS[-1])]
    out["shoot_base"] = cbase
    for (t, d), rgb in ans["shoot"].items():
        rows = np.flatnonzero(_rows_differ(rgb, cbase))
        out["shoot_rows_%d_%d" % (t, d)], out["shoot_diff_%d_%d" % (t, d)] = rows.astype(np.int32), rgb[rows]
    np.savez_compressed(path, **out)


def fixture_path(name):
    return os.path.join(GOLDEN, "query_%s.npz" % name)


_loaded = {}


def load_fixture(name):
    """-> (blob bytes, ray set dict, answers dict) of tests/golden/query_<name>.npz; loaded once, never written to."""
    if name not in _loaded:
        z = np.load(fixture_path(name))
        assert list(z["class_names"]) == CLASSES and list(z["occ_kind_names"]) == OCC_KINDS
        rs = {k: z[k] for k in ("rays", "labels", "occ_index", "occ_kind", "occ_dist")}
        ans = {"hits": {}, "shoot": {}, "occ": z["occ"], "occ_gi": z["occ_gi"], "shoot_skip": z["shoot_skip"]}
        for t in RAY_TYPES:
            h = z["hits_base"].copy()
            h[z["hits_rows_%d" % t]] = z["hits_diff_%d" % t]
            ans["hits"][t] = h
            for d in DEPTHS:
                c = z["shoot_base"].copy()
                c[z["shoot_rows_%d_%d" % (t, d)]] = z["shoot_diff_%d_%d" % (t, d)]
                ans["shoot"][(t, d)] = c
        for a in list(rs.values()) + list(ans["hits"].values()) + list(ans["shoot"].values()) + [ans["occ"], ans["occ_gi"]]:
            a.setflags(write=False)
        _loaded[name] = (z["blob"].tobytes(), rs, ans)
    return _loaded[name]
