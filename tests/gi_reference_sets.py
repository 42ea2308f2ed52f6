"""Cases that pin the GI mode to the REAL reference bit for bit (tests/golden/gi_pairs_<scene>.npz, made by tests/golden/make_golden.py
gi_pairs; read by tests/test_gi_reference_host.py and tests/test_gpu_gi_reference.py).  numpy only, fixed seeds, no GPU.

The reference draws from std::default_random_engine, seeded from clock() ^ thread id; its driver (oracle/ref_driver.cpp) seeds that
engine instead, so its draws are a known stream.  This project draws gi_uniform(key, d).  A MATCHED PAIR is (key K, engine seed s) whose
two draws are the same two floats on both sides -- found by search, see make_golden.py:
  hit pair      gi_uniform(K, 2), gi_uniform(K, 3) == the first two draws after engine.seed(s): the two angles of GI sample 0 of the
                shootRay invocation with key K, and of the first diffuse hit the reference shades after the seeding;
  jitter pair   gi_uniform(K, 0), gi_uniform(K, 1) == those two draws: offsetX, offsetY of a jittered camera ray.
With GI_SAMPLE_SIZE = 1 and MAX_DEPTH = 1 a ray whose first hit is diffuse has a colour that depends on those two draws only: what the
depth-1 hit draws steers rays of depth 2, which return the background whatever their direction (RayTracer.cpp:427); mirrors and glass
draw nothing.  So shootRay under seed s and this project's GI shoot with key K are the same computation, and must agree in every bit.

gi_mix(a, b) is a bijection in a (oracle_api.gi_mix_inverse), so a matched key can be put anywhere: on sample k of pixel p of a frame
(gi_seed = inverse(inverse(K, k), p)) and below a mirror (the parent key whose child 0 is K).

Case families of a scene's fixture:
  q_*   query rays whose first hit is diffuse, classes CLASSES, each with a hit pair; colour at N = 1, MAX_DEPTH = 1
  m_*   rays whose first hit is a mirror and whose reflected ray hits diffuse, key = parent of K; colour at N = 1, MAX_DEPTH = 2
        (no glass first hits: two subtrees draw there, in the reference's order)
  p_*   frame pixels whose centre ray hits diffuse, with the gi_seed that puts a hit pair's key on the pixel's sample 0; the reference's
        centre ray and its shootRay colour under the seed
  j_*   jittered camera rays: a jitter pair, a pixel, a sample index k >= 1, the gi_seed that puts the key there; the reference's
        getRay(row, col, true)"""
import os

import numpy as np

import query_sets as qs
import reference_ray_sets as rrs

F32 = np.float32
SCENES = ["hw11", "hw14", "hw12"]             # reference_ray_sets.make_scene: 128x72, 112x63, 96x54 (hw12: 32x32 bitmap, textured build)
MIRROR_SCENES = ["hw11", "hw14"]
CLASSES = ["camera", "random", "smooth", "textured", "grazing"]
COUNTS = dict(camera=40, random=40, smooth=48, textured=20, grazing=24, mirror=24, pixels=32, jitter=64)
MIN_QUERY, MIN_MIRROR, MIN_PIXELS, MIN_JITTER, MIN_PAIRS = 96, 24, 32, 64, 128
SEED_FIRST, SEED_COUNT = 1, 1 << 25           # the engine seeds whose draw pairs are tabulated (seed 0 is seed 1 to minstd_rand0)
Q_DEPTH, M_DEPTH, SAMPLES = 1, 2, 1
FIXTURE_SEED = 20250301
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARRAYS = ["hit_keys", "hit_seeds", "hit_draws", "jitter_keys", "jitter_seeds", "jitter_draws",
          "q_rays", "q_type", "q_label", "q_pair", "q_rgb", "m_rays", "m_type", "m_pair", "m_keys", "m_rgb",
          "p_row", "p_col", "p_pair", "p_seed", "p_ray", "p_rgb", "j_row", "j_col", "j_pair", "j_k", "j_seed", "j_rays"]


# ------------------------------------------------------------------------------------------------------------------------ keys
def parent_key(oa, key, child=0):
    """the key whose child `child` (0 reflection, 1 transmission, 2 + i GI sample i) is `key`"""
    return oa.gi_mix_inverse(key, np.uint32(oa.GI_CHILD + child))


def seed_for(oa, key, pixel, sample):
    """the gi_seed under which sample `sample` of pixel `pixel` (row-major index) has `key`: key = mix(mix(seed, pixel), sample)"""
    return oa.gi_mix_inverse(oa.gi_mix_inverse(key, np.asarray(sample, dtype=np.uint32)), np.asarray(pixel, dtype=np.uint32))


def find_pairs(oa, first=SEED_FIRST, count=SEED_COUNT, first_key=0, n_keys=1 << 32):
    """-> {"hit": (keys, seeds, draws), "jitter": (...)}: every key of the range whose draws 2, 3 (hit) or 0, 1 (jitter) are, as float
    bit patterns, the two draws of an engine seed of [first, first + count); draws uint32 [n, 2]"""
    table = oa.reference_gi_draws(first, count)
    out = {}
    for kind, d0 in (("hit", 2), ("jitter", 0)):
        keys, index = oa.gi_pair_search(table, d0, first_key, n_keys)
        out[kind] = (keys, (index.astype(np.uint64) + first).astype(np.uint32), table[index])
    return out


# ------------------------------------------------------------------------------------------------------------------------ scenes
def diffuse_meshes(scene):
    return rrs.material_kinds(scene) == "diffuse"


def smooth_meshes(scene):
    return np.array([bool(scene["materials"][o["material_index"]].get("smooth_shading")) for o in scene["objects"]])


def textured_meshes(scene):
    """meshes whose albedo is a texture that varies over the surface (edges, checker, bitmap; not the constant `albedo` kind)"""
    kind = {t["name"]: t["type"] for t in scene.get("textures", [])}
    return np.array([isinstance(scene["materials"][o["material_index"]]["albedo"], str) and
                     kind[scene["materials"][o["material_index"]]["albedo"]] != "albedo" for o in scene["objects"]])


def covered_pixels(oa, scene):
    """bool [H, W]: the pixels RayTracer::render's bucket grid reaches (the others keep the buffer's zero in every frame)"""
    im = scene["settings"]["image_settings"]
    covered = np.zeros((im["height"], im["width"]), dtype=bool)
    for row, col, w, h in oa.bucket_grid(im["width"], im["height"], im["bucket_size"]):
        covered[row:row + h, col:col + w] = True
    return covered


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _aimed(rng, scene, meshes, n):
    """rays from inside the room at vertices of the given meshes"""
    verts = np.concatenate([np.asarray(scene["objects"][m]["vertices"], dtype=np.float64).reshape(-1, 3) for m in meshes])
    target = verts[rng.integers(len(verts), size=n)]
    origin = rng.uniform([-2.5, -0.9, -7.0], [2.5, 2.2, 0.5], (n, 3))
    return np.concatenate([origin, _unit(target - origin)], axis=1).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------ the cases
def build(oa, scene, blob, pairs, seed=FIXTURE_SEED):
    """The cases of one scene, chosen from the reference's own answers (its trace decides what a ray hits), with the reference's colours
    and rays.  pairs: find_pairs' result."""
    rng = np.random.default_rng(seed)
    im = scene["settings"]["image_settings"]
    W, H = im["width"], im["height"]
    diffuse, smooth, textured = diffuse_meshes(scene), smooth_meshes(scene), textured_meshes(scene)
    kinds = rrs.material_kinds(scene)
    trace = lambda rays, t: oa.reference_trace(blob, rays, t, textured=True)
    hit_keys, hit_seeds, hit_draws = pairs["hit"]
    jit_keys, jit_seeds, jit_draws = pairs["jitter"]
    assert len(hit_keys) >= MIN_PAIRS and len(jit_keys) >= MIN_PAIRS, (len(hit_keys), len(jit_keys))
    order = rng.permutation(len(hit_keys))                       # a scene's hit cases take the pairs in this order, each once if they last
    taken = [0]

    def next_pairs(n):
        idx = order[(taken[0] + np.arange(n)) % len(order)]
        taken[0] += n
        return idx.astype(np.int32)

    # every pixel's centre ray, from the reference (the seed is not read by getRay(.., false))
    rows, cols = (a.reshape(-1).astype(np.uint32) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    centre = oa.reference_camera_rays(blob, rows, cols, np.ones(W * H, dtype=np.uint32), centre=True, max_depth=0)[0]
    centre_hits = trace(centre, qs.RAY_PRIMARY)
    centre_diffuse = (centre_hits["hit"] == 1) & diffuse[np.where(centre_hits["hit"] == 1, centre_hits["mesh"], 0)]

    def first_diffuse(rays, ray_type, want=None, count=0):
        """indices of the first `count` rays whose first hit is diffuse (and on a mesh of `want`), with the hit records"""
        hits = trace(rays, ray_type)
        mesh = np.where(hits["hit"] == 1, hits["mesh"], 0)
        ok = (hits["hit"] == 1) & diffuse[mesh] & np.isfinite(hits["t"])
        if want is not None:
            ok &= want[mesh]
        idx = np.flatnonzero(ok)[:count]
        return idx, hits

    q_rays, q_type, q_label = [], [], []

    def add(cls, rays, ray_type):
        q_rays.append(rays)
        q_type.append(np.full(len(rays), ray_type, dtype=np.uint8))
        q_label.append(np.full(len(rays), CLASSES.index(cls), dtype=np.uint8))

    # camera: centre rays of pixels all over the frame
    pick = rng.permutation(np.flatnonzero(centre_diffuse))[:COUNTS["camera"]]
    add("camera", centre[pick], qs.RAY_PRIMARY)
    # random: origins in and around the room, any direction
    cand = qs.random_rays(600, seed=seed)
    idx, random_hits = first_diffuse(cand, qs.RAY_REFLECTION, None, COUNTS["random"])
    add("random", cand[idx], qs.RAY_REFLECTION)
    # smooth-shaded and textured diffuse meshes: camera rays that reach them and rays aimed at them
    for cls, flags in (("smooth", smooth), ("textured", textured)):
        meshes = np.flatnonzero(flags & diffuse)
        if len(meshes) == 0:
            continue
        on = np.flatnonzero(centre_diffuse & flags[np.where(centre_hits["hit"] == 1, centre_hits["mesh"], 0)])
        from_camera = centre[rng.permutation(on)[:COUNTS[cls] // 2]]
        add(cls, from_camera, qs.RAY_PRIMARY)
        cand = _aimed(rng, scene, meshes, 400)
        idx, _ = first_diffuse(cand, qs.RAY_REFLECTION, flags, COUNTS[cls] - len(from_camera))
        add(cls, cand[idx], qs.RAY_REFLECTION)
    # grazing: towards the reference's own hit points of the random set, one to three degrees above the surface
    ok = np.flatnonzero((random_hits["hit"] == 1) & diffuse[np.where(random_hits["hit"] == 1, random_hits["mesh"], 0)] &
                        np.isfinite(random_hits["point"]).all(axis=1))
    p, nrm = random_hits["point"][ok].astype(np.float64), random_hits["normal"][ok].astype(np.float64)
    tangent = _unit(np.cross(nrm, rng.normal(size=nrm.shape)))
    angle = rng.uniform(np.radians(1.0), np.radians(3.0), (len(ok), 1))
    d = tangent * np.cos(angle) - nrm * np.sin(angle)
    cand = np.concatenate([p - d * rng.uniform(0.2, 0.6, (len(ok), 1)), d], axis=1).astype(F32)
    idx, hits = first_diffuse(cand, qs.RAY_REFLECTION, None, len(cand))
    cosine = np.abs(np.einsum("ij,ij->i", cand[idx, 3:].astype(np.float64), hits["normal"][idx].astype(np.float64)))
    idx = idx[cosine < np.sin(np.radians(4.0))][:COUNTS["grazing"]]
    add("grazing", cand[idx], qs.RAY_REFLECTION)

    out = {"hit_keys": hit_keys, "hit_seeds": hit_seeds, "hit_draws": hit_draws,
           "jitter_keys": jit_keys, "jitter_seeds": jit_seeds, "jitter_draws": jit_draws}
    out["q_rays"], out["q_type"], out["q_label"] = np.concatenate(q_rays).astype(F32), np.concatenate(q_type), np.concatenate(q_label)
    out["q_pair"] = next_pairs(len(out["q_rays"]))
    out["q_rgb"] = shoot_by_type(lambda rays, seeds, t: oa.reference_shoot_gi(blob, rays, seeds, t, Q_DEPTH, SAMPLES),
                                 out["q_rays"], hit_seeds[out["q_pair"]], out["q_type"])

    # below a mirror: the first hit reflective, the reflected ray's hit diffuse
    mirrors = np.flatnonzero(kinds == "reflective")
    m_rays, m_type = np.zeros((0, 6), dtype=F32), np.zeros(0, dtype=np.uint8)
    if len(mirrors):
        on = np.flatnonzero((centre_hits["hit"] == 1) & np.isin(centre_hits["mesh"], mirrors))
        cand = np.concatenate([centre[rng.permutation(on)[:COUNTS["mirror"] // 2 * 3]], _aimed(rng, scene, mirrors, 300)])
        types = np.concatenate([np.full(len(cand) - 300, qs.RAY_PRIMARY), np.full(300, qs.RAY_REFLECTION)]).astype(np.uint8)
        keep = np.zeros(len(cand), dtype=bool)
        for t in (qs.RAY_PRIMARY, qs.RAY_REFLECTION):
            sel = np.flatnonzero(types == t)
            first = trace(cand[sel], t)
            on_mirror = (first["hit"] == 1) & np.isin(first["mesh"], mirrors) & np.isfinite(first["t"])
            n64, d64 = first["normal"].astype(np.float64), _unit(cand[sel, 3:].astype(np.float64))
            refl = d64 - 2.0 * np.einsum("ij,ij->i", d64, n64)[:, None] * n64
            with np.errstate(all="ignore"):
                second_rays = np.concatenate([first["point"] + first["normal"] * F32(1e-4), _unit(refl)], axis=1).astype(F32)
            second_rays[~on_mirror] = cand[sel][~on_mirror]
            second = trace(second_rays, qs.RAY_REFLECTION)
            keep[sel] = on_mirror & (second["hit"] == 1) & diffuse[np.where(second["hit"] == 1, second["mesh"], 0)] & np.isfinite(second["t"])
        half = COUNTS["mirror"] // 2
        from_camera = np.flatnonzero(keep & (types == qs.RAY_PRIMARY))[:half]
        aimed = np.flatnonzero(keep & (types == qs.RAY_REFLECTION))[:COUNTS["mirror"] - len(from_camera)]
        pick = np.concatenate([from_camera, aimed])
        m_rays, m_type = cand[pick], types[pick]
    out["m_rays"], out["m_type"] = m_rays, m_type
    out["m_pair"] = next_pairs(len(m_rays))
    out["m_keys"] = parent_key(oa, hit_keys[out["m_pair"]], 0)
    out["m_rgb"] = shoot_by_type(lambda rays, seeds, t: oa.reference_shoot_gi(blob, rays, seeds, t, M_DEPTH, SAMPLES),
                                 m_rays, hit_seeds[out["m_pair"]], m_type)

    # frame pixels
    pick = rng.permutation(np.flatnonzero(centre_diffuse & covered_pixels(oa, scene).reshape(-1)))[:COUNTS["pixels"]]
    out["p_row"], out["p_col"] = rows[pick], cols[pick]
    out["p_pair"] = next_pairs(len(pick))
    out["p_seed"] = seed_for(oa, hit_keys[out["p_pair"]], pick, 0)
    out["p_ray"], out["p_rgb"] = oa.reference_camera_rays(blob, rows[pick], cols[pick], hit_seeds[out["p_pair"]], centre=True,
                                                          max_depth=Q_DEPTH, gi_sample_size=SAMPLES)

    # jittered camera rays
    n = COUNTS["jitter"]
    pick = rng.integers(W * H, size=n)
    pick[:4] = [0, W - 1, (H - 1) * W, H * W - 1]                  # the frame's corners
    out["j_row"], out["j_col"] = rows[pick], cols[pick]
    out["j_pair"] = rng.permutation(len(jit_keys))[np.arange(n) % len(jit_keys)].astype(np.int32)
    out["j_k"] = rng.integers(1, 8, size=n).astype(np.uint32)
    out["j_seed"] = seed_for(oa, jit_keys[out["j_pair"]], pick, out["j_k"])
    out["j_rays"] = oa.reference_camera_rays(blob, rows[pick], cols[pick], jit_seeds[out["j_pair"]])
    return out


def shoot_by_type(shoot, rays, extra, types):
    """shoot(rays, extra, ray_type) -> [n, 3], called once per ray type present; the colours in ray order"""
    rgb = np.zeros((len(rays), 3), dtype=F32)
    for t in np.unique(types):
        sel = np.flatnonzero(types == t)
        rgb[sel] = shoot(np.ascontiguousarray(rays[sel]), np.ascontiguousarray(extra[sel]), int(t))
    return rgb


def gi_options(oa, depth, **more):
    return oa.make_options(depth, use_gi=1, gi_sample_size=SAMPLES, rays_per_pixel=1, **more)


def oracle_answers(oa, oracle_scene, fx, key_xor=0, depth_less=0):
    """The oracle's answers for a fixture's cases, in the fixture's layout (q_rgb, m_rgb, p_rgb, p_ray, j_rays).  key_xor: the hit cases
    with the keys K ^ key_xor in place of K; depth_less: with MAX_DEPTH lowered by it (the census uses both)."""
    keys = fx["hit_keys"] ^ np.uint32(key_xor)
    out = {}
    out["q_rgb"] = shoot_by_type(lambda r, k, t: oracle_scene.shoot_gi(r, k, t, gi_options(oa, Q_DEPTH - depth_less)),
                                 fx["q_rays"], keys[fx["q_pair"]], fx["q_type"])
    out["m_rgb"] = shoot_by_type(lambda r, k, t: oracle_scene.shoot_gi(r, k, t, gi_options(oa, M_DEPTH - depth_less)),
                                 fx["m_rays"], parent_key(oa, keys[fx["m_pair"]], 0), fx["m_type"])
    pixel = fx["p_row"].astype(np.int64) * oracle_scene.width + fx["p_col"]
    out["p_rgb"] = oracle_scene.render_pixels(fx["p_row"], fx["p_col"], seed_for(oa, keys[fx["p_pair"]], pixel, 0), gi_options(oa, Q_DEPTH - depth_less))
    out["p_ray"] = np.array([np.concatenate(oracle_scene.camera_ray(int(r), int(c))) for r, c in zip(fx["p_row"], fx["p_col"])], dtype=F32)
    out["j_rays"] = oracle_scene.camera_sample_rays(fx["j_row"], fx["j_col"], fx["jitter_keys"][fx["j_pair"]])
    return out


def with_pairs(oa, blob, fx, pairs, width):
    """A fixture's rays and pixels with OTHER matched pairs (dealt out cyclically), the derived keys and seeds, and the live reference's
    answers for them: what tests/test_oracle_vs_reference.py compares the oracle with, so that the committed pairs are not the only
    witness."""
    out = dict(fx)
    out["hit_keys"], out["hit_seeds"], out["hit_draws"] = pairs["hit"]
    out["jitter_keys"], out["jitter_seeds"], out["jitter_draws"] = pairs["jitter"]
    n_hit, n_jit = len(pairs["hit"][0]), len(pairs["jitter"][0])
    for f, start in (("q_pair", 0), ("m_pair", 1), ("p_pair", 2)):
        out[f] = ((np.arange(len(fx[f])) + start) % n_hit).astype(np.int32)
    out["j_pair"] = (np.arange(len(fx["j_pair"])) % n_jit).astype(np.int32)
    keys, seeds = out["hit_keys"], out["hit_seeds"]
    out["m_keys"] = parent_key(oa, keys[out["m_pair"]], 0)
    out["p_seed"] = seed_for(oa, keys[out["p_pair"]], fx["p_row"].astype(np.int64) * width + fx["p_col"], 0)
    out["j_seed"] = seed_for(oa, out["jitter_keys"][out["j_pair"]], fx["j_row"].astype(np.int64) * width + fx["j_col"], fx["j_k"])
    out["q_rgb"] = shoot_by_type(lambda r, s, t: oa.reference_shoot_gi(blob, r, s, t, Q_DEPTH, SAMPLES), fx["q_rays"], seeds[out["q_pair"]], fx["q_type"])
    out["m_rgb"] = shoot_by_type(lambda r, s, t: oa.reference_shoot_gi(blob, r, s, t, M_DEPTH, SAMPLES), fx["m_rays"], seeds[out["m_pair"]], fx["m_type"])
    out["p_ray"], out["p_rgb"] = oa.reference_camera_rays(blob, fx["p_row"], fx["p_col"], seeds[out["p_pair"]], centre=True, max_depth=Q_DEPTH,
                                                          gi_sample_size=SAMPLES)
    out["j_rays"] = oa.reference_camera_rays(blob, fx["j_row"], fx["j_col"], out["jitter_seeds"][out["j_pair"]])
    return out


def frame_pixel(colour):
    """RayTracer::renderRectangle's fold of one colour (RayTracer.cpp:102-104): (Color(0, 0, 0) + colour) * (1.0f / 1) -- a -0 becomes +0"""
    return ((F32(0) + np.asarray(colour, dtype=F32)) * (F32(1.0) / F32(1))).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------ conditions
def _differs(a, b):
    """rows whose colours differ as floats, NaN equal to NaN"""
    return (~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=1)


def census(oa, scene, oracle_scene, blob_trace, fx):
    """What makes a fixture worth having.  Evaluated with the oracle and, for the meshes hit, a trace function (the reference's in the
    generator, the oracle's in the host test) -- never with the kernels.  The hit cases are the q, m and p families."""
    diffuse, smooth, textured = diffuse_meshes(scene), smooth_meshes(scene), textured_meshes(scene)
    base = oracle_answers(oa, oracle_scene, fx)
    other = oracle_answers(oa, oracle_scene, fx, key_xor=1)
    shallow = oracle_answers(oa, oracle_scene, fx, depth_less=1)        # the sample ray is the background there, whatever it would hit
    fams = ("q_rgb", "m_rgb", "p_rgb")
    n_hit = sum(len(base[f]) for f in fams)
    # the mesh of the diffuse hit: the first hit of the q rays and the pixels' centre rays (below a mirror it is a room wall or
    # another mesh, not looked up: those cases count as neither smooth nor textured)
    mesh = []
    for rays, types in ((fx["q_rays"], fx["q_type"]), (fx["p_ray"], np.zeros(len(fx["p_ray"]), dtype=np.uint8))):
        m = np.zeros(len(rays), dtype=np.int64)
        for t in np.unique(types):
            sel = np.flatnonzero(types == t)
            hits = blob_trace(np.ascontiguousarray(rays[sel]), int(t))
            assert (hits["hit"] == 1).all() and diffuse[hits["mesh"]].all(), "a first hit that is not diffuse"
            m[sel] = hits["mesh"]
        mesh.append(m)
    mesh = np.concatenate(mesh)
    return {"hit_cases": n_hit, "query": len(fx["q_rays"]), "mirror": len(fx["m_rays"]), "pixels": len(fx["p_row"]), "jitter": len(fx["j_row"]),
            "hit_pairs": len(fx["hit_keys"]), "jitter_pairs": len(fx["jitter_keys"]),
            "classes": {c: int((fx["q_label"] == k).sum()) for k, c in enumerate(CLASSES)},
            "sample_hits_geometry": int(sum(_differs(base[f], shallow[f]).sum() for f in fams)),
            "other_key_other_colour": int(sum(_differs(base[f], other[f]).sum() for f in fams)),
            "smooth": int(smooth[mesh].sum()), "textured": int(textured[mesh].sum()),
            "nan": int(sum(np.isnan(fx[f]).any(axis=1).sum() for f in fams)),
            "distinct_pairs_used": len(np.unique(np.concatenate([fx["q_pair"], fx["m_pair"], fx["p_pair"]])))}


def check_census(name, scene, c):
    """The conditions a fixture has to meet (the generator asserts them before it writes, tests/test_gi_reference_host.py on the committed
    files).  The smooth-shaded share is asked of the scenes that have a smooth-shaded DIFFUSE mesh: hw11's smooth meshes are its mirror
    and its glass, which its m cases reach as first hits."""
    assert c["hit_pairs"] >= MIN_PAIRS and c["jitter_pairs"] >= MIN_PAIRS, (name, c)
    assert c["query"] >= MIN_QUERY and c["pixels"] >= MIN_PIXELS and c["jitter"] >= MIN_JITTER, (name, c)
    if name in MIRROR_SCENES:
        assert c["mirror"] >= MIN_MIRROR, (name, c)
    assert 2 * c["sample_hits_geometry"] >= c["hit_cases"], (name, c)
    assert 10 * c["other_key_other_colour"] >= 9 * c["hit_cases"], (name, c)
    if (smooth_meshes(scene) & diffuse_meshes(scene)).any():
        assert 5 * c["smooth"] >= c["hit_cases"], (name, c)
    if name == "hw12":
        assert 5 * c["textured"] >= c["hit_cases"], (name, c)
    for cls in ("camera", "random", "grazing"):
        assert c["classes"][cls] >= 12, (name, cls, c)


# ------------------------------------------------------------------------------------------------------------------------ fixtures
def fixture_path(name):
    return os.path.join(GOLDEN, "gi_pairs_%s.npz" % name)


def save_fixture(path, blob, fx):
    options = np.array([Q_DEPTH, M_DEPTH, SAMPLES, SEED_FIRST, SEED_COUNT], dtype=np.int64)   # and the default biases, 1e-4 each
    np.savez_compressed(path, blob=np.frombuffer(blob, dtype=np.uint8), class_names=np.array(CLASSES), options=options, **{k: fx[k] for k in ARRAYS})


_loaded = {}


def load_fixture(name):
    """-> (blob bytes, dict of the arrays ARRAYS) of tests/golden/gi_pairs_<name>.npz; loaded once, never written to."""
    if name not in _loaded:
        z = np.load(fixture_path(name))
        assert list(z["class_names"]) == CLASSES and list(z["options"]) == [Q_DEPTH, M_DEPTH, SAMPLES, SEED_FIRST, SEED_COUNT]
        fx = {k: z[k] for k in ARRAYS}
        for a in fx.values():
            a.setflags(write=False)
        _loaded[name] = (z["blob"].tobytes(), fx)
    return _loaded[name]
