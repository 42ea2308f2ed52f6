"""Scenes with ill-formed triangles, and a ray set for the queries on them (tests/test_degenerate_host.py, tests/test_gpu_degenerate.py,
tests/golden/make_golden.py degenerate).  No GPU here: the builders are numpy, the route predicates walk the oracle's own trees.

The reference accepts any triangle (Triangle.cpp:13-16, Ray.cpp:9-31):
  zero    two identical vertices: the cross product is exactly (0,0,0), Vector::normalize returns early (Vector.cpp:97-106) and the
          stored normal is (0,0,0).  A primary ray is rejected (0 >= 0); every other ray that tests the triangle gets a hit at
          t = -0/0 = NaN, which wins where no finite hit replaces it (KDTree.cpp:75-86, :156-166) and never occludes
          (AccelerationStructure.cpp:73-74).
  plane   e1 = (1,0,0), e2 = (2,1e-25,0): the cross product (0,0,1e-25) has a squared length that underflows, normalize returns early
          and the stored normal is that tiny vector.  t is finite and every pointIsInTriangle term is far above -FLT_EPSILON: the
          triangle is its whole plane for every ray that reaches a leaf listing it.
  needle  1 m x 0.1 mm with a unit normal: well defined.
None of them has a usable margin (crt_bvh.cpp: triangle_margin), so these scenes render without the candidate filter."""
import numpy as np

import query_sets as qs
from shoot_gi_sets import camera_rays, look_at

F32 = np.float32
W, H = 48, 32
DETAIL = 0.15
DEPTH = 3
CASES = ["zero", "plane", "needle", "mixed"]

# the hw11-like room: objects 0 .. 4 are floor, ceiling, back, left and right wall, 5 the mirror sphere, 6 the glass sphere; it is open at z = 1
FLOOR, MIRROR, GLASS = 0, 5, 6
# from inside the room, 0.65 m in front of the mirror sphere on the line from its centre to the open side, looking at it: the mirror rays of
# the middle of its near side leave the room
CAMERA = ((-0.95, -0.3, -3.55), (-1.25, -0.65, -5.0))
# the zero-area triangle is (A, A, B): a segment whose box reaches from the floor in front of the spheres out through the open side and
# holds the light at (0.1, 1.5, -0.4)
ZERO_A, ZERO_B = (-0.9, -1.45, -2.6), (0.9, 2.3, 1.7)
# mixed: two more beside the open side, left and right of the first one's box, in the textured meshes
CHECKER_A, CHECKER_B = (-2.9, -1.4, 0.2), (-0.95, 2.4, 1.8)
BITMAP_A, BITMAP_B = (0.95, -1.4, 0.2), (2.9, 2.4, 1.8)
# the plane triangle: in the floor's mesh, whose box then reaches up to y = 0 -- the plane z = PLANE_Z for every ray that enters that box
PLANE_Z = -6.5
PLANE = ((-1.0, 0.0, PLANE_Z), (0.0, 0.0, PLANE_Z), (1.0, 1e-25, PLANE_Z))
# the needle: 1 m long, 0.1 mm wide, NEEDLE_DISTANCE in front of the camera and square to it, along the plane in which the centre rays of pixel row
# NEEDLE_ROW lie, which cuts it a fifth of its width above its long edge: about a dozen of that row's primary rays hit it
NEEDLE_ROW = 6
NEEDLE_DISTANCE = 0.6

_scenes, _oracles, _frames, _rays = {}, {}, {}, {}


def append_triangle(obj, points, uvs=None):
    """the object with three more vertices and the triangle over them"""
    o = dict(obj)
    n = len(obj["vertices"])
    o["vertices"] = np.concatenate([np.asarray(obj["vertices"], dtype=F32).reshape(-1, 3), np.asarray(points, dtype=F32).reshape(3, 3)])
    o["triangles"] = np.concatenate([np.asarray(obj["triangles"], dtype=np.uint32).reshape(-1, 3), np.array([[n, n + 1, n + 2]], dtype=np.uint32)])
    if "uvs" in obj:
        o["uvs"] = np.concatenate([np.asarray(obj["uvs"], dtype=F32).reshape(-1, 3), np.asarray(uvs, dtype=F32).reshape(3, 3)])
    return o


def zero_points(a, b):
    return (a, a, b)


def lone_triangle(material, points):
    return {"material_index": int(material), "vertices": np.asarray(points, dtype=F32).reshape(3, 3), "triangles": np.array([[0, 1, 2]], dtype=np.uint32)}


def needle_points():
    """RayTracer::getRay (RayTracer.cpp:61-80): the centre ray of (row, col) is x right + y up + forward with y = 1 - 2 (row + 0.5) / H"""
    right, up, back = look_at(*CAMERA).astype(np.float64)
    y = 1.0 - 2.0 * (NEEDLE_ROW + 0.5) / H
    centre = NEEDLE_DISTANCE * (y * up - back)
    across = np.cross(right, centre / np.linalg.norm(centre))       # in the needle's plane, square to its long edge and to the row's plane
    p0 = np.asarray(CAMERA[0], dtype=np.float64) + centre - 0.5 * right - 2e-5 * across
    pts = np.array([p0, p0 + right, p0 + 1e-4 * across])
    if np.dot(np.cross(pts[1] - pts[0], pts[2] - pts[0]), centre) > 0:   # face the camera: a primary ray needs n . d < 0 (Ray.cpp:13)
        pts = pts[[1, 0, 2]]
        pts[2] = pts[1] + 1e-4 * across
    return pts.astype(F32)


def base_scene(scenes):
    scene = scenes.make("hw11", width=W, height=H, detail=DETAIL)
    scene["settings"]["image_settings"]["bucket_size"] = 16      # every pixel is rendered (tests/shoot_gi_sets.py: scene_of)
    scene["camera"] = {"position": [float(x) for x in CAMERA[0]], "matrix": [float(x) for x in look_at(*CAMERA).ravel()]}
    return scene


def build(scenes, case, bad=True):
    """The named case; bad=False: the same scene without its ill-formed triangles (the meshes of their own stay away too).  Returns
    (scene, marks): marks maps a name to (object index, triangle index within the object) of an ill-formed triangle."""
    scene = base_scene(scenes)
    objects = [dict(o) for o in scene["objects"]]
    floor_material = objects[FLOOR]["material_index"]
    where = {}                                            # name -> (the object, as it is in `objects`, and the triangle's index in it)

    def add(name, index, points, uvs=None):
        if bad:
            objects[index] = append_triangle(objects[index], points, uvs)
            where[name] = (objects[index], len(objects[index]["triangles"]) - 1)

    def own(name, points, front=False):
        if bad:
            o = lone_triangle(floor_material, points)
            objects.insert(0, o) if front else objects.append(o)
            where[name] = (o, 0)

    if case in ("zero", "mixed"):
        add("zero_mirror", MIRROR, zero_points(ZERO_A, ZERO_B))                       # the mirror sphere is smooth-shaded
    if case in ("plane", "mixed"):
        add("plane", FLOOR, PLANE)
    if case in ("needle", "mixed"):
        own("needle", needle_points())
    if case == "mixed":
        n_mat = len(scene["materials"])
        scene["textures"] = [{"name": "checker", "type": "checker", "color_A": [0.9, 0.9, 0.9], "color_B": [0.15, 0.15, 0.15], "square_size": 0.125},
                             {"name": "noise", "type": "bitmap", "file_path": "/degenerate_noise.ppm", "_pixels": scenes.noise_bitmap(16, 16, seed=3)}]
        scene["materials"] = scene["materials"] + [{"type": "diffuse", "albedo": "checker", "smooth_shading": False},
                                                   {"type": "diffuse", "albedo": "noise", "smooth_shading": True}]
        uv = [(0.1, 0.2, 0.0), (0.1, 0.2, 0.0), (0.9, 0.7, 0.0)]
        # the textured meshes come before the room's: in a top-level leaf that lists both, their NaN hit is the first one
        for k, (name, centre, a, b) in enumerate([("zero_bitmap", (2.3, -1.0, -2.9), BITMAP_A, BITMAP_B), ("zero_checker", (-2.3, -1.0, -3.2), CHECKER_A, CHECKER_B)]):
            objects.insert(0, scenes.uv_sphere(n_mat + 1 - k, centre, 0.4, 8, 4))
            add(name, 0, zero_points(a, b), uv)
    if case in ("zero", "mixed"):
        own("zero_own", zero_points(ZERO_A, ZERO_B), front=True)                      # listed first in `objects`
    marks = {name: (next(i for i, o in enumerate(objects) if o is obj), tri) for name, (obj, tri) in where.items()}
    scene["objects"] = objects
    if case != "mixed":
        for o in scene["objects"]:
            o.pop("uvs", None)
    return scene, marks


def floor_mesh(scene):
    """the floor's object index: the first object with the floor's material (the room's first) that is no lone triangle"""
    return next(i for i, o in enumerate(scene["objects"]) if o["material_index"] == 0 and len(o["triangles"]) >= 2)


def scene_of(scenes, case, bad=True):
    key = (case, bad)
    if key not in _scenes:
        _scenes[key] = build(scenes, case, bad)
    return _scenes[key]


def oracle_of(scenes, oracle, case, bad=True):
    key = (case, bad)
    if key not in _oracles:
        _oracles[key] = oracle.OracleScene(scenes.to_blob(scene_of(scenes, case, bad)[0]))
    return _oracles[key]


def frame_of(scenes, oracle, case, bad=True):
    """the oracle's frame at DEPTH, made once and never written to"""
    key = (case, bad)
    if key not in _frames:
        rgb, counters = oracle_of(scenes, oracle, case, bad).render(DEPTH)
        rgb.setflags(write=False)
        _frames[key] = (rgb, counters)
    return _frames[key]


# ------------------------------------------------------------------------------------------------------------ route predicates
def nan_pixels(rgb):
    return np.isnan(np.asarray(rgb)).any(axis=-1)


def walk_reaches(oracle, tree, ray, element):
    """Does the reference's walk (KDTree.cpp:53-74: the box test at every node, both children pushed) reach a leaf that lists `element`?"""
    boxes, links, idx = tree
    start = np.concatenate([[0], np.cumsum(links[:, 3])]).astype(np.int64)
    stack = [0]
    while stack:
        n = stack.pop()
        if not oracle.box_hit(boxes[n, :3], boxes[n, 3:], ray[:3], ray[3:]):
            continue
        if links[n, 3]:
            if element in idx[start[n]:start[n + 1]]:
                return True
        else:
            stack += [int(c) for c in links[n, :2] if c != 0xFFFFFFFF]
    return False


def ray_tests_triangle(oracle, o, trees, ray, mesh, triangle):
    """The reference intersects `triangle` of `mesh` with this ray: the top-level walk reaches a leaf listing the mesh, and the mesh's a
    leaf listing the triangle.  trees: {-1: o.tree(-1), mesh: o.tree(mesh)}"""
    return walk_reaches(oracle, trees[-1], ray, mesh) and walk_reaches(oracle, trees[mesh], ray, triangle)


def trees_of(o, meshes):
    return {m: o.tree(m) for m in [-1] + list(meshes)}


def primary_hits(o):
    """OracleScene.trace of every camera ray: (rays [n,6], hit bool [n], values [n,11] = t, point, normal, u, v, mesh, triangle)"""
    rays = camera_rays(o)
    hit = np.zeros(len(rays), dtype=bool)
    vals = np.zeros((len(rays), 11), dtype=F32)
    for i, r in enumerate(rays):
        hit[i], vals[i] = o.trace(r[:3], r[3:], qs.RAY_PRIMARY)
    return rays, hit, vals


def normalized(v):
    """Vector::normalize (Vector.cpp:97-106) in float32"""
    v = np.asarray(v, dtype=F32)
    length = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    with np.errstate(all="ignore"):
        out = (v * (F32(1.0) / length)[..., None]).astype(F32)
    return np.where((length == 0)[..., None], v, out)


def reflection_rays(rays, vals, bias=1e-4):
    """RayTracer.cpp:358-374 in float32: origin = point + normal * bias, direction = normalize(d - 2 (d . n) n).  (The glass sphere's
    reflected ray is the same one: a camera ray meets it from outside.)"""
    d, p, n = rays[:, 3:].astype(F32), vals[:, 1:4].astype(F32), vals[:, 4:7].astype(F32)
    dn = ((d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]).astype(F32)
    direction = normalized((d - (F32(2) * dn)[:, None] * n).astype(F32))
    return np.concatenate([(p + n * F32(bias)).astype(F32), direction], axis=1).astype(F32)


def shadow_segments(scene, points, normals, bias=1e-4):
    """RayTracer.cpp:300-330 in float32: for every point and light the shadow ray and the distance to the light: ([n, lights, 6], [n, lights])"""
    p, n = np.asarray(points, dtype=F32), np.asarray(normals, dtype=F32)
    origin = (p + n * F32(bias)).astype(F32)
    rays = np.zeros((len(p), len(scene["lights"]), 6), dtype=F32)
    dist = np.zeros((len(p), len(scene["lights"])), dtype=F32)
    for l, light in enumerate(scene["lights"]):
        ld = (np.asarray(light["position"], dtype=F32)[None, :] - p).astype(F32)
        dist[:, l] = np.sqrt((ld[:, 0] * ld[:, 0] + ld[:, 1] * ld[:, 1]) + ld[:, 2] * ld[:, 2])
        rays[:, l, :3], rays[:, l, 3:] = origin, normalized(ld)
    return rays, dist


def mirror_pixels(scene, hit, vals):
    """pixels whose primary hit is on a reflective or refractive mesh"""
    kinds = np.array([scene["materials"][o["material_index"]]["type"] for o in scene["objects"]])
    return np.flatnonzero(hit & np.isin(kinds[np.where(hit, vals[:, 9], 0).astype(int)], ["reflective", "refractive"]))


def route_census(scenes, oracle, case):
    """The route conditions of a case, from the oracle alone:
      nan_pixels        pixels of the frame with a NaN component
      nan_winners       {mesh: level-1 reflection rays of the camera's mirror pixels whose closest hit is a NaN hit on that mesh}
      plane_pixels      pixels whose primary hit is the plane triangle at a point outside that triangle's own box
      shadow_crossings  floor pixels with a shadow ray that tests a zero-area triangle, is not occluded, and whose colour is the
                        colour of the same pixel in the scene without the ill-formed triangles"""
    scene, marks = scene_of(scenes, case)
    o = oracle_of(scenes, oracle, case)
    rgb = frame_of(scenes, oracle, case)[0]
    rays, hit, vals = primary_hits(o)
    out = {"nan_pixels": int(nan_pixels(rgb).sum()), "nan_winners": {}, "plane_pixels": 0, "shadow_crossings": 0}
    mirrors = mirror_pixels(scene, hit, vals)
    for r in reflection_rays(rays[mirrors], vals[mirrors]):
        h, v = o.trace(r[:3], r[3:], qs.RAY_REFLECTION)
        if h and np.isnan(v[0]):
            out["nan_winners"][int(v[9])] = out["nan_winners"].get(int(v[9]), 0) + 1
    if "plane" in marks:
        mesh, tri = marks["plane"]
        obj = scene["objects"][mesh]
        pts = np.asarray(obj["vertices"], dtype=F32)[obj["triangles"][tri]]
        on = hit & (vals[:, 9] == mesh) & (vals[:, 10] == tri)
        outside = np.any((vals[:, 1:4] < pts.min(axis=0)) | (vals[:, 1:4] > pts.max(axis=0)), axis=1)
        out["plane_pixels"] = int((on & outside).sum())
    zeros = [marks[k] for k in sorted(marks) if k.startswith("zero")]
    if zeros:
        clean = frame_of(scenes, oracle, case, bad=False)[0].reshape(-1, 3)
        floor = floor_mesh(scene)
        px = np.flatnonzero(hit & (vals[:, 9] == floor) & (vals[:, 10] < 2))
        segs, dist = shadow_segments(scene, vals[px, 1:4], vals[px, 4:7])
        trees = trees_of(o, [m for m, _ in zeros])
        same = (clean[px].view(np.uint32) == rgb.reshape(-1, 3)[px].view(np.uint32)).all(axis=1)
        for k in range(len(px)):
            if not same[k]:
                continue
            for l in range(segs.shape[1]):
                s = segs[k, l]
                if any(ray_tests_triangle(oracle, o, trees, s, m, t) for m, t in zeros) and not o.occluded(s[:3], s[3:], dist[k, l]):
                    out["shadow_crossings"] += 1
                    break
    return out


# ------------------------------------------------------------------------------------------------------------ the queries' ray set
def query_rays(scenes, oracle, case="mixed", n_random=300):
    """dict of float32 [n, 6] ray arrays, made once and never written to:
      camera      the camera's rays
      reflection  the level-1 reflection rays of the pixels with a NaN component
      random      rays from query_sets.random_rays
      shadow      shadow rays from floor points towards a light that test a zero-area triangle; shadow_distance: the light's distance"""
    if case not in _rays:
        scene, marks = scene_of(scenes, case)
        o = oracle_of(scenes, oracle, case)
        rays, hit, vals = primary_hits(o)
        bad = np.flatnonzero(nan_pixels(frame_of(scenes, oracle, case)[0]).reshape(-1) & hit)
        zeros = [marks[k] for k in sorted(marks) if k.startswith("zero")]
        trees = trees_of(o, [m for m, _ in zeros])
        floor = floor_mesh(scene)
        px = np.flatnonzero(hit & (vals[:, 9] == floor) & (vals[:, 10] < 2))
        segs, dist = shadow_segments(scene, vals[px, 1:4], vals[px, 4:7])
        segs, dist = segs.reshape(-1, 6), dist.reshape(-1)
        keep = [k for k in range(len(segs)) if any(ray_tests_triangle(oracle, o, trees, segs[k], m, t) for m, t in zeros)][:256]
        out = {"camera": rays.copy(), "reflection": reflection_rays(rays[bad], vals[bad]), "random": qs.random_rays(n_random, seed=23),
               "shadow": np.ascontiguousarray(segs[keep]), "shadow_distance": np.ascontiguousarray(dist[keep])}
        for a in out.values():
            a.setflags(write=False)
        _rays[case] = out
    return _rays[case]


def all_rays(rays):
    return np.ascontiguousarray(np.concatenate([rays["camera"], rays["reflection"], rays["random"], rays["shadow"]]))
