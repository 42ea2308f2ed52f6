"""Scenes and ray sets for the filter's rarely taken routes (tests/test_gpu_filter_rare.py, tests/test_bvh_filter.py): walks whose
stack outgrows its LDS part, hits verified by the pruned tree walk (BVH_TRI_WALK), exact ties in distance.  No GPU here: the builders
are numpy, the answers come from OracleScene, and every property a test relies on is measured by a census function below."""
import numpy as np

from query_sets import RAY_PRIMARY, RAY_REFLECTION, triangle_bases

F32 = np.float32
U = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)            # the diagonal
E1 = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)          # ... and two unit vectors across it
E2 = np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0)


def _settings(width, height, bg=(0.0, 0.5, 0.0)):
    return {"background_color": list(bg), "image_settings": {"width": width, "height": height, "bucket_size": 48}}


def _mesh(material_index, vertices, triangles):
    return {"material_index": int(material_index), "vertices": np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3),
            "triangles": np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)}


def _unit32(d):
    """float32 directions of unit length (within the queries' 2^-20: normalised in float64, rounded once)."""
    d = np.asarray(d, dtype=np.float64)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ deep stack
DEEP_SPACING = 0.05          # s: card i is centred at (DEEP_FIRST + i) s (1, 1, 1)
DEEP_FIRST = 4
DEEP_RADIUS = 0.225 * DEEP_SPACING   # r: a card lies within r of its centre, so its extent on every axis is below s
DEEP_N = 8192                # see test_gpu_filter_rare.py: the smallest count whose filter has four children at each of six levels on every path


def deep_stack_cameras(n):
    """Two cameras on the diagonal looking along it through every card's box: A before the first card looking up the diagonal, B
    behind the last one looking back.  The matrix rows are scaled so that the 32x24 frame is as wide as a card at the far end."""
    length = (n + 2 * DEEP_FIRST) * DEEP_SPACING * np.sqrt(3.0)
    k = 0.9 * DEEP_RADIUS / (length * (32.0 / 24.0))
    a = {"position": [0.0, 0.0, 0.0], "matrix": list(np.concatenate([E1 * k, E2 * k, -U]))}
    end = (n + 2 * DEEP_FIRST) * DEEP_SPACING
    b = {"position": [end, end, end], "matrix": list(np.concatenate([-E1 * k, E2 * k, U]))}
    return a, b


def deep_stack_scene(n=DEEP_N, seed=5):
    """n small cards strung along the diagonal, each one triangle roughly perpendicular to it (normal -(1,1,1)), rotated in its plane
    by a seeded angle and pushed off the axis so that it covers only part of its bounding square and never the axis itself: a ray
    along the diagonal passes every card's box and is stopped by some card only, at any depth of the stack.  Cards are smaller than
    their spacing on every axis, so each axis split of the reference's spatial-median trees separates them (no duplication).  Every
    fourth card is reflective (a second mesh: the reflection runs back through the stack)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    centre = ((DEEP_FIRST + i) * DEEP_SPACING)[:, None] * np.array([1.0, 1.0, 1.0])
    theta = rng.uniform(0.0, 2.0 * np.pi, n)
    rho = DEEP_RADIUS * rng.uniform(0.2, 0.45, n)            # circumradius: below the 0.5 r by which the card is pushed off the axis
    push = 0.5 * DEEP_RADIUS
    mid = centre + push * (np.cos(theta)[:, None] * E1 + np.sin(theta)[:, None] * E2)
    verts = np.empty((n, 3, 3))
    for k in range(3):   # corners in the order that makes the normal (v1 - v0) x (v2 - v0) point along -U
        ang = theta + 1.0 - k * 2.0 * np.pi / 3.0
        verts[:, k] = mid + rho[:, None] * (np.cos(ang)[:, None] * E1 + np.sin(ang)[:, None] * E2)
    n0 = np.cross(verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0])
    assert (n0 @ U < 0).all()
    mirror = (i % 4) == 3
    objects = []
    for sel, material in ((~mirror, 0), (mirror, 1)):
        v = verts[sel].reshape(-1, 3)
        objects.append(_mesh(material, v, np.arange(len(v)).reshape(-1, 3)))
    cam_a, _ = deep_stack_cameras(n)
    return {"settings": _settings(32, 24),
            "camera": cam_a,
            # one light beside camera A: its shadow rays run back through the stack (and mostly end in it); one far to the side and
            # before the first card: it lights every card's front, and its shadow rays leave the stack at once, so a hit's colour says which card was hit
            "lights": [{"intensity": 400000, "position": list(3.0 * DEEP_RADIUS * E1 - 0.5 * DEEP_SPACING * U)},
                       {"intensity": 4000000, "position": list(150.0 * E1 - 40.0 * U)}],
            "materials": [{"type": "diffuse", "albedo": [0.8, 0.6, 0.3], "smooth_shading": False},
                          {"type": "reflective", "albedo": [0.9, 0.9, 0.9], "smooth_shading": False}],
            "objects": objects}


def camera_rays(oracle_scene, camera=None):
    """The rays a frame walks for the pixels' centres: RayTracer::getRay, normalised once more as shootRay does (float32)."""
    if camera is not None:
        oracle_scene.set_camera(camera["position"], camera["matrix"])
    rays = []
    for row in range(oracle_scene.height):
        for col in range(oracle_scene.width):
            o, d = oracle_scene.camera_ray(row, col)
            d = d / np.sqrt(np.sum(d * d, dtype=F32), dtype=F32)
            rays.append(np.concatenate([o, d]))
    return np.array(rays, dtype=F32)


def deep_stack_bundle(n=DEEP_N, per_direction=1024, seed=9):
    """A thin bundle around the diagonal, both ways: parallel rays from a disc of 0.9 r around the axis before the first card (up the
    diagonal) and behind the last card (down it)."""
    rng = np.random.default_rng(seed)
    rays = []
    end = (n + 2 * DEEP_FIRST) * DEEP_SPACING
    for start, direction in ((np.zeros(3), U), (np.full(3, end), -U)):
        rad = 0.9 * DEEP_RADIUS * np.sqrt(rng.uniform(0.0, 1.0, per_direction))
        phi = rng.uniform(0.0, 2.0 * np.pi, per_direction)
        o = start + rad[:, None] * (np.cos(phi)[:, None] * E1 + np.sin(phi)[:, None] * E2)
        rays.append(np.concatenate([o.astype(F32), np.tile(_unit32(direction), (per_direction, 1))], axis=1))
    return np.concatenate(rays).astype(F32)


def deep_stack_rays(oracle_scene, n=DEEP_N):
    """The query tests' ray set: both cameras' frame rays (the walks whose stack mark the frames measure) and the parallel bundle."""
    cam_a, cam_b = deep_stack_cameras(n)
    rays = np.concatenate([camera_rays(oracle_scene, cam_a), camera_rays(oracle_scene, cam_b), deep_stack_bundle(n)])
    oracle_scene.set_camera(cam_a["position"], cam_a["matrix"])
    return rays


def first_hit_cards(scene, hits):
    """Index along the diagonal of the card each hit record names (-1: no hit)."""
    bases = triangle_bases(scene)
    n = sum(len(o["triangles"]) for o in scene["objects"])
    card_of = np.empty(n, dtype=np.int64)
    i = np.arange(n)
    mirror = (i % 4) == 3
    card_of[bases[0]:bases[0] + int((~mirror).sum())] = i[~mirror]
    card_of[bases[1]:bases[1] + int(mirror.sum())] = i[mirror]
    return np.where(hits["hit"].astype(bool), card_of[hits["triangle"]], -1)


# ------------------------------------------------------------------------------------------------------------------- leaf walk
LEAF_LO, LEAF_HI = np.array([-1.0, -1.0, -6.0]), np.array([1.0, 1.0, -4.0])


def _scattered(rng, count, lo, hi, size):
    c = rng.uniform(lo + size, hi - size, (count, 3))
    v = c[:, None, :] + rng.uniform(-size, size, (count, 3, 3))
    return v


def _large_pair(lo, hi):
    """Two triangles lying obliquely across the whole box: each has a corner on every face, so its bounding box is the box."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    t0 = [(x0, y0, z1), (x1, y0, z0), (x0, y1, z0)]
    t1 = [(x1, y1, z0), (x1, y0, z1), (x0, y1, z1)]
    out = []
    for t in (t0, t1):
        t = np.array(t)
        if np.cross(t[1] - t[0], t[2] - t[0])[2] < 0:   # facing the camera at the origin (which looks down -z): primary rays cull back faces
            t = t[[0, 2, 1]]
        out.append(t)
    return np.array(out)


def _leaf_walk_mesh(rng, lo, hi, small, material, large_copies=1):
    v = _scattered(rng, small, lo, hi, 0.13 * float(np.min(hi - lo)))
    large = _large_pair(lo, hi)
    large = np.concatenate([large[:1]] * large_copies + [large[1:]])   # (the FIRST large triangle is the one a tie scene duplicates)
    # the large ones in the middle of the index range: neither first nor last in any leaf by position alone
    allv = np.concatenate([v[:small // 2], large, v[small // 2:]])
    return _mesh(material, allv.reshape(-1, 3), np.arange(3 * len(allv)).reshape(-1, 3)), np.arange(small // 2, small // 2 + len(large))


def leaf_walk_scene(seed=21):
    """One mesh of 300 small triangles scattered in a box plus two large ones across the whole box -- listed by every leaf of the
    mesh's tree, far more than BVH_LIST_MAX: verified by bvh_leaf_walk --, and a second small mesh inside the same box, so that a
    ray's candidates change mesh (cache_mesh / cache_k2)."""
    rng = np.random.default_rng(seed)
    m0, large = _leaf_walk_mesh(rng, LEAF_LO, LEAF_HI, 300, 0)
    v1 = _scattered(rng, 40, LEAF_LO + 0.3, LEAF_HI - 0.3, 0.15)
    m1 = _mesh(1, v1.reshape(-1, 3), np.arange(3 * len(v1)).reshape(-1, 3))
    scene = {"settings": _settings(48, 36),
             "camera": {"matrix": [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], "position": [0.0, 0.0, 0.0]},
             "lights": [{"intensity": 300, "position": [1.5, 2.0, -1.0]}],
             "materials": [{"type": "diffuse", "albedo": [0.8, 0.6, 0.3], "smooth_shading": False},
                           {"type": "diffuse", "albedo": [0.2, 0.4, 0.9], "smooth_shading": False}],
             "objects": [m0, m1]}
    return scene, large   # (large: triangle indices within mesh 0 == global indices, mesh 0 being first)


def box_rays(lo, hi, count, seed):
    """Rays from a sphere around the box towards points inside it."""
    rng = np.random.default_rng(seed)
    mid, rad = 0.5 * (lo + hi), 1.5 * np.linalg.norm(hi - lo)
    o = rng.normal(size=(count, 3))
    o = mid + rad * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = rng.uniform(lo, hi, (count, 3))
    o32 = o.astype(F32)
    return np.concatenate([o32, _unit32(target - o32)], axis=1).astype(F32)


def leaf_walk_rays():
    return box_rays(LEAF_LO, LEAF_HI, 1500, 33)


def ray_triangle_t(rays, tri):
    """float64 distance along each ray to the triangle's plane where the point lies inside the triangle (any facing), else inf:
    geometry for the census only -- which rays pass a large triangle BEHIND their winner -- never an expected value."""
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    a, b, c = (np.asarray(p, dtype=np.float64) for p in tri)
    nrm = np.cross(b - a, c - a)
    den = d @ nrm
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((a - o) @ nrm) / den
    p = o + d * t[:, None]
    inside = np.ones(len(rays), dtype=bool)
    for p0, p1 in ((a, b), (b, c), (c, a)):
        inside &= np.cross(p1 - p0, p - p0) @ nrm >= 0
    return np.where(inside & (t > 0) & np.isfinite(t), t, np.inf)


def leaf_walk_census(scene, large, rays, hits):
    """(share of winners that are a large triangle, share that are a small triangle in front of a large one)"""
    won = hits["hit"].astype(bool)
    is_large = won & np.isin(hits["triangle"], large) & (hits["mesh"] == 0)
    v = scene["objects"][0]["vertices"].reshape(-1, 3, 3)
    behind = np.minimum(ray_triangle_t(rays, v[large[0]]), ray_triangle_t(rays, v[large[1]]))
    in_front = won & ~is_large & (behind > hits["t"].astype(np.float64) * (1.0 + 1e-6)) & np.isfinite(behind)
    return is_large.sum() / max(1, won.sum()), in_front.sum() / max(1, won.sum())


# ------------------------------------------------------------------------------------------------------------------------ ties
TIE_A_LO, TIE_A_HI = np.array([-3.2, -0.6, -5.6]), np.array([-2.0, 0.6, -4.4])     # kind A: one triangle twice in one mesh
TIE_B_LO, TIE_B_HI = np.array([-0.6, -0.6, -5.6]), np.array([0.6, 0.6, -4.4])      # kind B: one mesh twice, two albedos
TIE_C_LO, TIE_C_HI = np.array([2.0, -0.6, -5.6]), np.array([3.2, 0.6, -4.4])       # kind C: a BVH_TRI_WALK triangle twice


def tie_scene(reverse=False, drop=None, seed=41):
    """Coincident geometry of three kinds, side by side in the camera's view:
      A  a mesh of small triangles in which 12 facing triangles appear TWICE (other indices, equal vertices): decided by k3;
      B  one small mesh as TWO objects with different diffuse albedos: decided by k2, visible in the frame's colour;
      C  a leaf-walk mesh (leaf_walk_scene's) whose first large triangle appears twice: a tie through bvh_leaf_walk.
    reverse: the objects in the opposite order (and each mesh's triangles too).  drop = 0 / 1: the scene WITHOUT the first / second
    copy of everything duplicated (vertices and the order of what remains unchanged), from which the census reads each copy's own
    distance.  Returns (scene, info): info[kind] = the object indices and, for A and C, the duplicated triangles' local indices."""
    rng = np.random.default_rng(seed)
    # A: 60 scattered triangles, then 12 larger ones facing +z, then the same 12 again
    va = _scattered(rng, 60, TIE_A_LO, TIE_A_HI, 0.08)
    ca = rng.uniform(TIE_A_LO + 0.25, TIE_A_HI - 0.25, (12, 3))
    dup = ca[:, None, :] + np.array([[-0.2, -0.15, 0.0], [0.2, -0.15, 0.02], [0.0, 0.2, -0.02]])
    parts = [va, dup, dup.copy()]
    if drop is not None:
        parts.pop(1 + (drop == 1))
        parts.insert(1 + (drop == 1), np.empty((0, 3, 3)))
    allv = np.concatenate(parts)
    mesh_a = _mesh(0, allv.reshape(-1, 3), np.arange(3 * len(allv)).reshape(-1, 3))
    dup_a = (np.arange(60, 60 + len(parts[1])), np.arange(60 + len(parts[1]), 60 + len(parts[1]) + len(parts[2])))
    # B: 30 facing triangles, as two objects
    cb = rng.uniform(TIE_B_LO + 0.2, TIE_B_HI - 0.2, (30, 3))
    vb = cb[:, None, :] + np.array([[-0.18, -0.12, 0.0], [0.18, -0.12, 0.03], [0.0, 0.18, -0.03]])
    mesh_b = [_mesh(1 + k, vb.reshape(-1, 3), np.arange(3 * len(vb)).reshape(-1, 3)) for k in range(2)]
    if drop is not None:
        mesh_b = [mesh_b[1 - drop]]
    # C
    mesh_c, large_c = _leaf_walk_mesh(rng, TIE_C_LO, TIE_C_HI, 120, 3, large_copies=2)
    if drop is not None:
        keep = np.ones(len(mesh_c["triangles"]), dtype=bool)
        keep[large_c[drop]] = False
        vc = mesh_c["vertices"].reshape(-1, 3, 3)[keep]
        mesh_c = _mesh(3, vc.reshape(-1, 3), np.arange(3 * len(vc)).reshape(-1, 3))
        large_c = large_c[:2]
    objects = [mesh_a] + mesh_b + [mesh_c]
    kinds = ["A"] + ["B"] * len(mesh_b) + ["C"]
    if reverse:
        objects = objects[::-1]
        kinds = kinds[::-1]
        for o in objects:
            o["triangles"] = np.ascontiguousarray(o["triangles"][::-1])
    scene = {"settings": _settings(64, 24),
             "camera": {"matrix": [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], "position": [0.0, 0.0, 0.0]},
             "lights": [{"intensity": 300, "position": [0.5, 2.0, -1.0]}],
             "materials": [{"type": "diffuse", "albedo": [0.8, 0.6, 0.3], "smooth_shading": False},
                           {"type": "diffuse", "albedo": [0.9, 0.1, 0.1], "smooth_shading": False},
                           {"type": "diffuse", "albedo": [0.1, 0.1, 0.9], "smooth_shading": False},
                           {"type": "diffuse", "albedo": [0.3, 0.8, 0.3], "smooth_shading": False}],
             "objects": objects}
    info = {"kinds": kinds, "dup_a": dup_a, "large_c": large_c}
    return scene, info


def tie_rays():
    """Rays towards each of the three groups from in front of them (+z side), 700 per group."""
    out = []
    for k, (lo, hi) in enumerate(((TIE_A_LO, TIE_A_HI), (TIE_B_LO, TIE_B_HI), (TIE_C_LO, TIE_C_HI))):
        rng = np.random.default_rng(50 + k)
        o = np.stack([rng.uniform(lo[0], hi[0], 700), rng.uniform(lo[1], hi[1], 700), rng.uniform(-2.5, -1.0, 700)], axis=1).astype(F32)
        target = rng.uniform(lo, hi, (700, 3))
        out.append(np.concatenate([o, _unit32(target - o)], axis=1))
    return np.concatenate(out).astype(F32)


def tie_census(oracle, scenes, rays, ray_type=RAY_REFLECTION):
    """Per kind, the rays on which BOTH copies are the closest hit of their own scene at the same bit pattern of t: traced in the
    scene without the second copies and in the scene without the first copies.  Returns {kind: boolean mask over the rays}."""
    from query_sets import oracle_hits
    import importlib
    hit_dtype = importlib.import_module("course-assignment-danielhalachev_amd").HIT_DTYPE
    res = []
    for drop in (1, 0):
        scene, info = tie_scene(drop=drop)
        h = oracle_hits(oracle.OracleScene(scenes.to_blob(scene)), scene, rays, ray_type, hit_dtype)
        res.append((h, info))
    (h0, i0), (h1, i1) = res
    same = h0["hit"].astype(bool) & h1["hit"].astype(bool) & (h0["t"].view(np.uint32) == h1["t"].view(np.uint32)) & (h0["mesh"] == h1["mesh"])
    out = {}
    # in a scene with one copy the mesh indices are A = 0, B = 1, C = 2; the copy is the duplicated triangle itself
    out["A"] = same & (h0["mesh"] == 0) & np.isin(h0["triangle"], np.arange(60, 72)) & np.isin(h1["triangle"], np.arange(60, 72))   # (with one copy left it sits at 60 .. 71)
    out["B"] = same & (h0["mesh"] == 1)
    base_c = int(triangle_bases(tie_scene(drop=0)[0])[2])
    out["C"] = same & (h0["mesh"] == 2) & (h0["triangle"] == base_c + i0["large_c"][0]) & (h1["triangle"] == base_c + i1["large_c"][0])
    return out
