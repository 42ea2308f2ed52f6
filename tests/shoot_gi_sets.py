"""What the tests of the GI radiance queries (crt_shoot_rays_gi*) share: the small scenes, their cameras, the camera's rays and the
keys of a frame's pixels, and the oracle's GI frames -- each made once and never written to."""
import numpy as np

W, H = 48, 32
DEPTH = 3
# scene -> scenes.make's arguments (hw12 as tests/test_gi.py uses it)
SCENES = {"hw11": dict(detail=0.15), "hw08": dict(detail=0.3), "hw14": dict(detail=0.04), "hw12": dict(detail=0.08, bitmap_size=32)}
# (max_depth, gi_sample_size)
TUPLES = [(3, 2), (3, 3), (0, 2), (2, 0), (1, 1)]
SEED = 9
# hw11 from two more places: inside the room looking at the glass sphere, outside the open front looking in (position, target)
GLASS_SPHERE = (1.15, -0.55, -3.9)
CAMERAS = {"inside": ((-1.0, 0.9, -1.6), GLASS_SPHERE), "outside": ((0.8, 0.7, 1.8), (0.0, 0.3, -4.0))}

_scenes, _oracles, _frames = {}, {}, {}


def look_at(position, target):
    """The camera matrix whose rows are right, up and backward (RayTracer::getRay multiplies (x, y, -1) by it as a row vector)."""
    p, t = np.asarray(position, dtype=np.float64), np.asarray(target, dtype=np.float64)
    f = (t - p) / np.linalg.norm(t - p)
    right = np.cross(f, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, f)
    return np.array([right, up, -f], dtype=np.float32)


def scene_of(scenes, name):
    """16 buckets: RayTracer::render's grid then covers all 48x32 pixels (the scenes' own 48 make 6x5 rectangles, which leave the last two
    rows of a frame unrendered -- zero -- in the reference, the oracle and the library alike: no ray's colour)"""
    if name not in _scenes:
        scene = scenes.make(name, width=W, height=H, **SCENES[name])
        scene["settings"]["image_settings"]["bucket_size"] = 16
        _scenes[name] = scene
    return _scenes[name]


def oracle_of(scenes, oracle, name, camera=None):
    """The scene's OracleScene, with the named camera of CAMERAS (None: the scene's own)"""
    key = (name, camera)
    if key not in _oracles:
        o = oracle.OracleScene(scenes.to_blob(scene_of(scenes, name)))
        if camera:
            o.set_camera(CAMERAS[camera][0], look_at(*CAMERAS[camera]))
        _oracles[key] = o
    return _oracles[key]


def camera_rays(o):
    """RayTracer::getRay at every pixel centre, row-major: float32 [H * W, 6]"""
    rays = np.zeros((o.height * o.width, 6), dtype=np.float32)
    for row in range(o.height):
        for col in range(o.width):
            origin, direction = o.camera_ray(row, col)
            rays[row * o.width + col, :3], rays[row * o.width + col, 3:] = origin, direction
    rays.setflags(write=False)
    return rays


def pixel_keys(oracle, seed, n):
    """The keys of a frame's pixels 0 .. n - 1, sample 0: mix(mix(seed, p), 0)"""
    pixel = oracle.gi_array(np.full(n, seed, dtype=np.uint32), np.arange(n, dtype=np.uint32))[0]
    keys = oracle.gi_array(pixel, np.zeros(n, dtype=np.uint32))[0]
    keys.setflags(write=False)
    return keys


def gi_frame(scenes, oracle, name, depth, samples, seed=SEED, camera=None):
    """The oracle's GI frame with one ray per pixel: pixel p is (0 + shootRay(centre ray, key p)) * (1 / 1)"""
    key = (name, depth, samples, seed, camera)
    if key not in _frames:
        o = oracle_of(scenes, oracle, name, camera)
        rgb, _ = o.render(options=oracle.make_options(depth, use_gi=1, gi_sample_size=samples, rays_per_pixel=1, gi_seed=seed))
        rgb.setflags(write=False)
        _frames[key] = rgb
    return _frames[key]


def plain_frame(scenes, oracle, name, depth):
    key = (name, depth, "plain")
    if key not in _frames:
        rgb, _ = oracle_of(scenes, oracle, name).render(max_depth=depth)
        rgb.setflags(write=False)
        _frames[key] = rgb
    return _frames[key]


def differing_pixels(a, b):
    return int(np.any(np.asarray(a).reshape(-1, 3) != np.asarray(b).reshape(-1, 3), axis=1).sum())


def assert_same_values(got, want, what):
    """equal as float VALUES, NaNs equal: the frame's `0 + colour` turns a -0 into +0 and changes nothing else"""
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, "%s: %d of %d floats differ, first at %d: got %r want %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


_CASES = {}


def case(pkg, scenes, oracle, name, tmp_path_factory, camera=None, tuning=None):
    """A scene's tracer (with the named camera and tuning), its oracle, the camera's rays and the keys of a frame's pixels: made once"""
    key = (name, camera, tuple(sorted((tuning or {}).items())))
    if key not in _CASES:
        scene = scene_of(scenes, name)
        folder = ""
        if scene.get("textures"):
            folder = str(tmp_path_factory.mktemp(name))
            scenes.write_bitmaps(scene, folder)
        tracer = pkg.Tracer(pkg.Scene(json_text=scenes.to_json(scene), folder=folder), tuning=pkg.make_tuning(**tuning) if tuning else None)
        o = oracle_of(scenes, oracle, name, camera)
        if camera:
            tracer.set_camera(CAMERAS[camera][0], look_at(*CAMERAS[camera]))
        _CASES[key] = dict(scene=scene, tracer=tracer, oracle=o, rays=camera_rays(o), keys=pixel_keys(oracle, SEED, W * H))
    return _CASES[key]


def gi_options(pkg, depth, samples, seed=SEED, **more):
    return pkg.make_options(depth, use_gi=True, gi_sample_size=samples, rays_per_pixel=1, gi_seed=seed, **more)
