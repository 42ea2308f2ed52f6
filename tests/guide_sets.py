"""What the tests of the chain guides (crt_guide_rays*, crt_set_guide_bounces) share: the rule of include/crt_hip.h ("Chain guides")
restated in numpy float32 -- the child ray of a mirror or glass hit, one operation and one rounding at a time, as the -ffp-contract=off
build of mirror_glass_children (csrc/kernel_common.h) rounds it, and the host walk of a chain over OracleScene.trace --, the scenes of
these tests, and the oracle's sample colours of a frame.  No GPU here."""
import copy

import numpy as np

import shoot_gi_sets as gs
from query_sets import RAY_PRIMARY, RAY_REFLECTION, RAY_REFRACTION, triangle_bases

F = np.float32
CUT = 0x80
HIT_DTYPE = np.dtype([("t", np.float32), ("point", np.float32, 3), ("normal", np.float32, 3), ("u", np.float32), ("v", np.float32),
                      ("mesh", np.uint32), ("triangle", np.uint32), ("hit", np.uint32)])
# how a chain ended
MISS, DIFFUSE, CONSTANT, SPECULAR = range(4)


def normalize3(v):
    """Vector::normalize (Vector.cpp:97-106) in float32; a zero vector stays"""
    x, y, z = (F(c) for c in v)
    with np.errstate(all="ignore"):
        length = np.sqrt(F(F(F(x * x) + F(y * y)) + F(z * z)))
        if length == 0:
            return np.array([x, y, z], dtype=F)
        inv = F(F(1.0) / length)
        return np.array([F(x * inv), F(y * inv), F(z * inv)], dtype=F)


def fixed_point(rays):
    """rays float32 [n, 6] with every direction normalised until normalize3 leaves it as it is, four times at most, and where it does:
    -> (rays, fixed bool [n]).  A fixed ray is one in the form in which shootRay holds it: crt_shoot_rays* normalises on entry,
    crt_guide_rays* and crt_trace_rays* walk a ray as given, and for a fixed ray the two are the same ray.  (A few directions never
    settle: normalize3 moves them between two neighbouring floats.)"""
    out = np.array(rays, dtype=F)
    fixed = np.zeros(len(out), dtype=bool)
    for i in range(len(out)):
        d = out[i, 3:]
        for _ in range(4):
            e = normalize3(d)
            if np.array_equal(e.view(np.uint32), d.view(np.uint32)):
                fixed[i] = True
                break
            d = e
        out[i, 3:] = d
    return out, fixed


def dot3(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def child_ray(refractive, ior, d, p, n, reflection_bias, refraction_bias):
    """The ray a chain continues with behind a mirror (refractive False) or glass hit: calculateReflection's ray, or calculateRefraction's
    transmission ray and, under total internal reflection, its reflection ray (RayTracer.cpp:358-417) -- normalised once where the
    reference builds the Ray and once more at the child's shootRay entry.  -> (origin, direction, ray_type)"""
    d, p, n = (np.array(a, dtype=F) for a in (d, p, n))
    rb, fb = F(reflection_bias), F(refraction_bias)
    with np.errstate(all="ignore"):
        if refractive:
            eta1, eta2 = F(1.0), F(ior)
            idn = dot3(d, n)
            if idn > 0:
                eta1, eta2 = eta2, eta1
                n = np.array([F(F(-1.0) * c) for c in n], dtype=F)
                idn = F(-idn)
            cos_a = F(-idn)
            s = F(F(1.0) - F(cos_a * cos_a))
            sin_a = np.sqrt(s if F(0.0) < s else F(0.0))
            eta_ratio = F(eta1 / eta2)
            sin_b = F(eta_ratio * sin_a)
            if sin_b < F(1.0):
                c = F(F(1.0) - F(sin_b * sin_b))
                cos_b = np.sqrt(c if F(0.0) < c else F(0.0))
                t = np.array([F(F(eta_ratio * F(d[k] + F(cos_a * n[k]))) - F(cos_b * n[k])) for k in range(3)], dtype=F)
                origin = np.array([F(p[k] - F(n[k] * fb)) for k in range(3)], dtype=F)
                return origin, normalize3(normalize3(t)), RAY_REFRACTION
        k2 = F(F(2.0) * dot3(d, n))
        r = np.array([F(d[k] - F(k2 * n[k])) for k in range(3)], dtype=F)
        origin = np.array([F(p[k] + F(n[k] * rb)) for k in range(3)], dtype=F)
        return origin, normalize3(normalize3(r)), RAY_REFLECTION


def material_of(scene, mesh):
    return scene["materials"][scene["objects"][mesh]["material_index"]]


def walk(o, scene, ray, ray_type, max_bounces, reflection_bias=1e-4, refraction_bias=1e-4, bases=None):
    """The rule for one ray over OracleScene.trace -> dict(record (a HIT_DTYPE scalar), status, last_ray [6], last_type, kind (how it
    ended), types (the ray type of every segment after segment 0))"""
    bases = triangle_bases(scene) if bases is None else bases
    n_meshes = len(scene["objects"])
    origin, direction, kind_of_ray = np.array(ray[:3], dtype=F), np.array(ray[3:], dtype=F), ray_type
    record = np.zeros((), dtype=HIT_DTYPE)
    t_sum, first_mesh, types = F(0.0), 0, []
    k = 0
    while True:
        hit, v = o.trace(origin, direction, kind_of_ray)
        last = dict(last_ray=np.concatenate([origin, direction]).astype(F), last_type=kind_of_ray)
        if not hit:
            return dict(record=record, status=k, kind=MISS, types=types, **last)
        mesh = int(v[9])
        with np.errstate(all="ignore"):
            t_sum = F(v[0]) if k == 0 else F(t_sum + F(v[0]))
        if k == 0:
            first_mesh = mesh
        material = material_of(scene, mesh)
        specular = material["type"] in ("reflective", "refractive")
        if not specular or k == max_bounces:
            tag = mesh if k == 0 else mesh + n_meshes * (1 + first_mesh)
            record[()] = (t_sum, v[1:4], v[4:7], v[7], v[8], tag, int(bases[mesh]) + int(v[10]), 1)
            kind = SPECULAR if specular else (DIFFUSE if material["type"] == "diffuse" else CONSTANT)
            return dict(record=record, status=k | (CUT if specular else 0), kind=kind, types=types, **last)
        origin, direction, kind_of_ray = child_ray(material["type"] == "refractive", material.get("ior", 1.0), direction, v[1:4], v[4:7],
                                                   reflection_bias, refraction_bias)
        types.append(kind_of_ray)
        k += 1


def walk_all(o, scene, rays, ray_type, max_bounces, reflection_bias=1e-4, refraction_bias=1e-4):
    """walk for every ray -> dict of arrays: records, status uint8, last_rays [n, 6], last_types, kinds, all_reflective bool"""
    bases = triangle_bases(scene)
    n = len(rays)
    out = dict(records=np.zeros(n, dtype=HIT_DTYPE), status=np.zeros(n, dtype=np.uint8), last_rays=np.zeros((n, 6), dtype=F),
               last_types=np.zeros(n, dtype=np.int64), kinds=np.zeros(n, dtype=np.int64), all_reflective=np.zeros(n, dtype=bool))
    for i, ray in enumerate(rays):
        w = walk(o, scene, ray, ray_type, max_bounces, reflection_bias, refraction_bias, bases)
        out["records"][i], out["status"][i], out["last_rays"][i] = w["record"], w["status"], w["last_ray"]
        out["last_types"][i], out["kinds"][i] = w["last_type"], w["kind"]
        out["all_reflective"][i] = all(t == RAY_REFLECTION for t in w["types"])
    for a in out.values():
        a.setflags(write=False)
    return out


def untagged(records, n_meshes):
    """guide records with the mesh tag removed: the terminal hit as crt_shade_hits takes it (t stays the path length: it is not read)"""
    out = np.array(records, dtype=HIT_DTYPE)
    out["mesh"] = np.where(out["hit"] != 0, out["mesh"] % np.uint32(n_meshes), out["mesh"])
    return out


# ---- scenes (48x32, tests/shoot_gi_sets.py's sizes)
_made = {}


def white_mirror_scene(scenes):
    """hw11 with every reflective albedo (1, 1, 1): a mirror then returns its child's colour, 0 + 1 * c"""
    if "white" not in _made:
        scene = copy.deepcopy(gs.scene_of(scenes, "hw11"))
        for m in scene["materials"]:
            if m["type"] == "reflective":
                m["albedo"] = [1.0, 1.0, 1.0]
        _made["white"] = scene
    return _made["white"]


# the camera of the pinned test: near the mirror sphere, which then covers enough pixels at 48x32
MIRROR_CAMERA = ((-0.9, 0.2, -2.8), (-1.25, -0.65, -5.0))
# the camera of the mirror-wall scene: between the two spheres, facing the back wall
WALL_CAMERA = ((0.0, 0.5, -4.4), (0.0, 0.5, -8.0))


def mirror_wall_scene(scenes):
    """the hw11 room with a flat reflective quad on the back wall (1 cm in front of it, facing the room)"""
    if "wall" not in _made:
        scene = copy.deepcopy(gs.scene_of(scenes, "hw11"))
        scene["materials"].append({"type": "reflective", "albedo": [0.9, 0.9, 0.92], "smooth_shading": False})
        z = -7.99
        quad = scenes.quad(len(scene["materials"]) - 1, (-2.6, -1.1, z), (2.6, -1.1, z), (2.6, 2.1, z), (-2.6, 2.1, z))
        quad.pop("uvs", None)
        scene["objects"].append(quad)
        scene["camera"] = {"position": [float(c) for c in WALL_CAMERA[0]], "matrix": [float(c) for c in gs.look_at(*WALL_CAMERA).reshape(-1)]}
        _made["wall"] = scene
    return _made["wall"]


def facing_mirrors_scene(scenes):
    """two mirror quads that face each other across x = -1 .. 1, and nothing else: a ray between them bounces for ever, a ray along them leaves"""
    if "facing" not in _made:
        materials = [{"type": "reflective", "albedo": [0.9, 0.9, 0.9], "smooth_shading": False}]
        objects = [scenes.quad(0, (-1.0, -1.0, 1.0), (-1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, 1.0, 1.0)),    # at x = -1, facing +x
                   scenes.quad(0, (1.0, -1.0, -1.0), (1.0, -1.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, -1.0))]       # at x = +1, facing -x
        for q in objects:
            q.pop("uvs", None)
        scene = {"settings": {"background_color": [0.0, 0.5, 0.0], "image_settings": {"width": gs.W, "height": gs.H, "bucket_size": 16}},
                 "camera": {"matrix": [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], "position": [0.0, 0.0, 3.0]},
                 "lights": [{"intensity": 40, "position": [0.0, 0.5, 0.0]}], "materials": materials, "objects": objects}
        _made["facing"] = scene
    return _made["facing"]


def oracle_scene(scenes, oracle, which):
    key = ("oracle", which)
    if key not in _made:
        scene = {"white": white_mirror_scene, "wall": mirror_wall_scene, "facing": facing_mirrors_scene}[which](scenes)
        _made[key] = oracle.OracleScene(scenes.to_blob(scene))
    return _made[key]


# ---- the frame of "it keeps what the mirror shows": depth 3, 2 GI samples, 4 samples a pixel; the truth has 64
FRAME = dict(depth=3, gi_samples=2, samples=4, truth=64)


def oracle_sample_colours(o, oracle, n_samples, depth=FRAME["depth"], gi_samples=FRAME["gi_samples"], seed=gs.SEED):
    """colours float32 [n_samples, H * W, 3]: sample s of every pixel as the frame shoots it -- key mix(mix(seed, p), s), sample 0 through
    the pixel centre, the others jittered -- from the oracle"""
    pixels = o.width * o.height
    rows, cols = np.divmod(np.arange(pixels, dtype=np.uint32), np.uint32(o.width))
    pixel_key = oracle.gi_array(np.full(pixels, seed, dtype=np.uint32), np.arange(pixels, dtype=np.uint32))[0]
    options = oracle.make_options(depth, use_gi=1, gi_sample_size=gi_samples, rays_per_pixel=1, gi_seed=seed)
    out = np.zeros((n_samples, pixels, 3), dtype=F)
    centre = gs.camera_rays(o)
    for s in range(n_samples):
        keys = oracle.gi_array(pixel_key, np.full(pixels, s, dtype=np.uint32))[0]
        rays = centre if s == 0 else o.camera_sample_rays(rows, cols, keys)
        out[s] = o.shoot_gi(rays, keys, RAY_PRIMARY, options)
    out.setflags(write=False)
    return out
