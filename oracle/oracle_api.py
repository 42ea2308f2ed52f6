"""TEST INFRASTRUCTURE -- ctypes wrapper around oracle/liboracle.so (cpu_ref.c) and the prebuilt
real-reference binaries under oracle/_ref/.  Only tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg may import this module; nothing in the product package does.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboracle.so")
REF_PLAIN = os.path.join(HERE, "_ref", "ref_render")
REF_TEX = os.path.join(HERE, "_ref", "ref_render_tex")

COUNTER_NAMES = ["box_tests", "tri_tests", "leaf_index_reads", "shaded_hits", "light_evals", "texel_fetches",
                 "primary_rays", "secondary_rays", "shadow_rays"]


class Options(C.Structure):
    _fields_ = [("max_depth", C.c_uint32), ("shadow_bias", C.c_float), ("reflection_bias", C.c_float),
                ("refraction_bias", C.c_float), ("use_gi", C.c_uint32), ("gi_sample_size", C.c_uint32),
                ("rays_per_pixel", C.c_uint32), ("monte_carlo_bias", C.c_float), ("gi_seed", C.c_uint32)]


def make_options(max_depth=5, shadow_bias=1e-4, reflection_bias=1e-4, refraction_bias=1e-4, use_gi=0, gi_sample_size=2,
                 rays_per_pixel=1, monte_carlo_bias=1e-4, gi_seed=0):
    """RenderOptions (RayTracer.h:25-50); use_gi=1 selects the GI / multi-sample mode with the counter-based generator
    cpu_ref.c defines (gi_seed = the frame's seed)."""
    return Options(max_depth, shadow_bias, reflection_bias, refraction_bias, use_gi, gi_sample_size, rays_per_pixel,
                   monte_carlo_bias, gi_seed)


def build(force=False):
    """(Re)build liboracle.so with gcc; also the real-reference binaries when /root/reference exists."""
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(
            os.path.join(HERE, "cpu_ref.c")):
        subprocess.check_call(["make", "-C", HERE, "oracle"], stdout=subprocess.DEVNULL)
    if os.path.exists("/root/reference/SourceCode/src/RayTracer.cpp"):
        subprocess.check_call(["make", "-C", HERE, "-j4", "ref"], stdout=subprocess.DEVNULL)


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        L.oracle_scene_load.restype = C.c_void_p
        L.oracle_scene_load.argtypes = [C.c_char_p, C.c_size_t]
        L.oracle_scene_free.argtypes = [C.c_void_p]
        L.oracle_scene_dims.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint32)] * 3
        L.oracle_set_camera.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_render.argtypes = [C.c_void_p, C.POINTER(Options), C.c_void_p, C.c_void_p, C.c_int]
        L.oracle_bucket_grid.restype = C.c_uint32
        L.oracle_bucket_grid.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
        L.oracle_box_hit.argtypes = [C.c_void_p] * 4
        L.oracle_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.oracle_occluded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
        L.oracle_occluded_gi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int]
        L.oracle_shoot.argtypes = [C.c_void_p, C.POINTER(Options), C.c_void_p, C.c_void_p, C.c_int, C.c_uint,
                                   C.c_void_p]
        L.oracle_camera_ray.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
        L.oracle_mesh_count.restype = C.c_uint32
        L.oracle_mesh_count.argtypes = [C.c_void_p]
        L.oracle_tree_node_count.restype = C.c_uint32
        L.oracle_tree_node_count.argtypes = [C.c_void_p, C.c_int]
        L.oracle_tree_index_total.restype = C.c_uint64
        L.oracle_tree_index_total.argtypes = [C.c_void_p, C.c_int]
        L.oracle_tree_dump.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_mesh_sizes.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.oracle_mesh_normals.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.oracle_quantize.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.oracle_write_ppm.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.oracle_powf.restype = C.c_float
        L.oracle_powf.argtypes = [C.c_float, C.c_float]
        for name in ("oracle_sinf", "oracle_cosf"):
            getattr(L, name).restype = C.c_float
            getattr(L, name).argtypes = [C.c_float]
        L.oracle_gi_uniform.restype = C.c_float
        L.oracle_gi_uniform.argtypes = [C.c_uint32, C.c_uint32]
        L.oracle_gi_mix.restype = C.c_uint32
        L.oracle_gi_mix.argtypes = [C.c_uint32, C.c_uint32]
        L.oracle_sincos_array.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.oracle_gi_array.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.oracle_sincos_vs_libm.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.oracle_shoot_gi.argtypes = [C.c_void_p, C.POINTER(Options), C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.oracle_camera_sample_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.oracle_render_pixels.argtypes = [C.c_void_p, C.POINTER(Options), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.oracle_gi_pair_search.restype = C.c_uint64
        L.oracle_gi_pair_search.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class OracleScene:
    """A scene loaded into the CPU restatement (trees built exactly as the reference builds them)."""

    def __init__(self, blob: bytes):
        self._L = lib()
        self._h = self._L.oracle_scene_load(blob, len(blob))
        if not self._h:
            raise ValueError("oracle: bad scene blob")
        w, h, b = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._L.oracle_scene_dims(self._h, C.byref(w), C.byref(h), C.byref(b))
        self.width, self.height, self.bucket_count = w.value, h.value, b.value

    def close(self):
        if self._h:
            self._L.oracle_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_camera(self, position, matrix):
        p = np.ascontiguousarray(position, dtype=np.float32)
        m = np.ascontiguousarray(matrix, dtype=np.float32).reshape(9)
        self._L.oracle_set_camera(self._h, _p(p), _p(m))

    def render(self, max_depth=5, threads=0, buffer=None, options=None):
        """Returns (rgb float32 [H,W,3], counters dict)."""
        o = options or make_options(max_depth)
        rgb = buffer if buffer is not None else np.zeros((self.height, self.width, 3), dtype=np.float32)
        cnt = np.zeros(16, dtype=np.uint64)
        self._L.oracle_render(self._h, C.byref(o), _p(rgb), _p(cnt), threads)
        return rgb, {k: int(cnt[i]) for i, k in enumerate(COUNTER_NAMES)}

    def trace(self, origin, direction, ray_type=0):
        o = np.ascontiguousarray(origin, dtype=np.float32)
        d = np.ascontiguousarray(direction, dtype=np.float32)
        out = np.zeros(16, dtype=np.float32)
        hit = self._L.oracle_trace(self._h, _p(o), _p(d), ray_type, _p(out))
        return bool(hit), out[:11].copy()

    def occluded(self, origin, direction, distance, gi=False):
        """checkForIntersection for a shadow ray; gi=True: the GI build's rule, under which no mesh is skipped"""
        o = np.ascontiguousarray(origin, dtype=np.float32)
        d = np.ascontiguousarray(direction, dtype=np.float32)
        if gi:
            return bool(self._L.oracle_occluded_gi(self._h, _p(o), _p(d), float(distance), 1))
        return bool(self._L.oracle_occluded(self._h, _p(o), _p(d), float(distance)))

    def shoot(self, origin, direction, ray_type=0, depth=0, max_depth=5):
        o = np.ascontiguousarray(origin, dtype=np.float32)
        d = np.ascontiguousarray(direction, dtype=np.float32)
        out = np.zeros(3, dtype=np.float32)
        opt = make_options(max_depth)
        self._L.oracle_shoot(self._h, C.byref(opt), _p(o), _p(d), ray_type, depth, _p(out))
        return out

    def camera_ray(self, row, col):
        out = np.zeros(6, dtype=np.float32)
        self._L.oracle_camera_ray(self._h, row, col, _p(out))
        return out[:3].copy(), out[3:].copy()

    def shoot_gi(self, rays, keys, ray_type=0, options=None):
        """shoot_ray(ray i with key keys[i], depth 0) in the GI mode: rays float32 [n, 6], keys uint32 [n] -> float32 [n, 3]"""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        assert rays.shape == (len(keys), 6)
        rgb = np.zeros((len(rays), 3), dtype=np.float32)
        o = options or make_options(use_gi=1)
        self._L.oracle_shoot_gi(self._h, C.byref(o), _p(rays), _p(keys), len(rays), ray_type, _p(rgb))
        return rgb

    def camera_sample_rays(self, rows, cols, keys):
        """the jittered camera ray of the sample with key keys[i] at pixel (rows[i], cols[i]) -> float32 [n, 6]"""
        rows, cols, keys = (np.ascontiguousarray(a, dtype=np.uint32) for a in (rows, cols, keys))
        rays = np.zeros((len(keys), 6), dtype=np.float32)
        self._L.oracle_camera_sample_rays(self._h, _p(rows), _p(cols), _p(keys), len(keys), _p(rays))
        return rays

    def render_pixels(self, rows, cols, seeds, options):
        """pixel (rows[i], cols[i]) of the frame of `options` with gi_seed = seeds[i] -> float32 [n, 3]"""
        rows, cols, seeds = (np.ascontiguousarray(a, dtype=np.uint32) for a in (rows, cols, seeds))
        rgb = np.zeros((len(seeds), 3), dtype=np.float32)
        self._L.oracle_render_pixels(self._h, C.byref(options), _p(rows), _p(cols), _p(seeds), len(seeds), _p(rgb))
        return rgb

    @property
    def mesh_count(self):
        return self._L.oracle_mesh_count(self._h)

    def tree(self, mesh_index=-1):
        """(boxes [n,6], links [n,4] = child0, child1, parent, index count, indexes [total])"""
        n = self._L.oracle_tree_node_count(self._h, mesh_index)
        total = self._L.oracle_tree_index_total(self._h, mesh_index)
        boxes = np.zeros((n, 6), dtype=np.float32)
        links = np.zeros((n, 4), dtype=np.uint32)
        idx = np.zeros(max(total, 1), dtype=np.uint32)
        self._L.oracle_tree_dump(self._h, mesh_index, _p(boxes), _p(links), _p(idx))
        return boxes, links, idx[:total]

    def mesh_normals(self, mesh_index):
        nv, nt = C.c_uint32(), C.c_uint32()
        self._L.oracle_mesh_sizes(self._h, mesh_index, C.byref(nv), C.byref(nt))
        fn = np.zeros((nt.value, 3), dtype=np.float32)
        vn = np.zeros((nv.value, 3), dtype=np.float32)
        self._L.oracle_mesh_normals(self._h, mesh_index, _p(fn), _p(vn))
        return fn, vn


def box_hit(lo, hi, origin, direction) -> bool:
    a = [np.ascontiguousarray(x, dtype=np.float32) for x in (lo, hi, origin, direction)]
    return bool(lib().oracle_box_hit(*[_p(x) for x in a]))


def bucket_grid(width, height, bucket_count):
    rects = np.zeros((65536, 4), dtype=np.uint32)
    n = lib().oracle_bucket_grid(width, height, bucket_count, _p(rects), 65536)
    return rects[:n].copy()


def quantize(rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.zeros(rgb.shape, dtype=np.uint16)
    lib().oracle_quantize(_p(rgb), rgb.size, _p(out))
    return out


def write_ppm(path, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    if lib().oracle_write_ppm(path.encode(), _p(rgb), w, h) != 0:
        raise OSError("oracle: cannot write " + path)


def powf(x, y):
    return float(lib().oracle_powf(x, y))


def sinf(x):
    return float(lib().oracle_sinf(x))


def cosf(x):
    return float(lib().oracle_cosf(x))


def sincos_array(y):
    """(sinf, cosf) of a float32 array by the oracle's restatement of glibc's routines."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    s, c = np.empty_like(y), np.empty_like(y)
    lib().oracle_sincos_array(_p(y), y.size, _p(s), _p(c))
    return s, c


def gi_array(a, b):
    """(mix(a, b), u(a, b)) elementwise for uint32 arrays: the GI generator of cpu_ref.c."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    m, u = np.empty_like(a), np.empty(a.shape, dtype=np.float32)
    lib().oracle_gi_array(_p(a), _p(b), a.size, _p(m), _p(u))
    return m, u


def sincos_vs_libm(first=0.0, last=6.2831860, stride=1):
    """Compares the restated sinf / cosf with this machine's libm over every stride-th float of [first, last] (both >= 0):
    returns (values tested, sinf mismatches, cosf mismatches)."""
    lo = int(np.float32(first).view(np.uint32))
    hi = int(np.float32(last).view(np.uint32))
    out = np.zeros(3, dtype=np.uint64)
    lib().oracle_sincos_vs_libm(lo, hi, stride, _p(out))
    return int(out[0]), int(out[1]), int(out[2])


def gi_uniform(key, d):
    return float(lib().oracle_gi_uniform(key, d))


def gi_mix(a, b):
    return int(lib().oracle_gi_mix(a, b))


# ---- the generator's inverse, in numpy (nothing of cpu_ref.c is used, so that gi_mix can check it).  gi_mix(a, b) =
# fmix32(fmix32(a ^ C1) + (b ^ C2) * C3) is a bijection in a for fixed b: fmix32 is xor-shifts and multiplications by odd constants.
_M32 = np.uint64(0xFFFFFFFF)
_C1, _C2, _C3 = 0x9E3779B9, 0x7F4A7C15, 0x9E3779B1
_INV_M1, _INV_M2 = pow(0x85EBCA6B, -1, 1 << 32), pow(0xC2B2AE35, -1, 1 << 32)
GI_CHILD, GI_DRAW = 0x40000000, 0x80000000       # gi_child_key(K, c) = gi_mix(K, GI_CHILD + c); gi_uniform(K, d) reads gi_mix(K, GI_DRAW + d)


def _fmix32_inverse(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(_INV_M2)) & _M32
    h = h ^ (h >> np.uint64(13)) ^ (h >> np.uint64(26))
    h = (h * np.uint64(_INV_M1)) & _M32
    return h ^ (h >> np.uint64(16))


def gi_mix_inverse(value, b):
    """The a with gi_mix(a, b) == value, elementwise (uint32 arrays or scalars -> uint32 array).  For a key K: the pixel key that puts K
    on sample k is gi_mix_inverse(K, k), the frame seed that puts that pixel key on pixel p is gi_mix_inverse(pixel key, p), and the
    parent key whose child c is K is gi_mix_inverse(K, GI_CHILD + c)."""
    v = np.asarray(value, dtype=np.uint32).astype(np.uint64)
    bb = np.asarray(b, dtype=np.uint32).astype(np.uint64)
    inner = (_fmix32_inverse(v) + np.uint64(1 << 32) - (((bb ^ np.uint64(_C2)) * np.uint64(_C3)) & _M32)) & _M32
    return (_fmix32_inverse(inner) ^ np.uint64(_C1)).astype(np.uint32)


def gi_pair_search(table_bits, d0, first_key=0, n_keys=1 << 32, cap=1 << 16):
    """Every key K of [first_key, first_key + n_keys) whose draws (gi_uniform(K, d0), gi_uniform(K, d0 + 1)) are, as float bit patterns,
    a row of table_bits (uint32 [n, 2]) -> (keys uint32 [m], row indices uint32 [m]), in key order."""
    table = np.ascontiguousarray(table_bits, dtype=np.uint32)
    assert table.ndim == 2 and table.shape[1] == 2
    keys, index = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
    m = int(lib().oracle_gi_pair_search(_p(table), len(table), d0, first_key, n_keys, _p(keys), _p(index), cap))
    if m > cap:
        raise ValueError("gi_pair_search: %d matches, room for %d" % (m, cap))
    return keys[:m].copy(), index[:m].copy()


# ----------------------------------------------------------------------------- the REAL reference
def reference_available(textured=False) -> bool:
    return os.path.exists(REF_TEX if textured else REF_PLAIN)


def reference_render(blob: bytes, max_depth=5, mode="bvhpool", textured=None, ppm_path=None, repeat=1,
                     cpus=None, gi=None, all_frames=False):
    """Run the real reference (oracle/_ref/ref_render[_tex]) on a CRTS blob.
    Returns (rgb float32 [H,W,3], info dict with render_s/build_s/threads).  gi=(GI_SAMPLE_SIZE, RAYS_PER_PIXEL) selects
    the reference's GI mode (every render differs); all_frames=True returns all `repeat` frames as [repeat,H,W,3]."""
    if textured is None:
        textured = blob[80:84] != b"\x00\x00\x00\x00"  # n_textures field (after the 80-byte header)
    exe = REF_TEX if textured else REF_PLAIN
    if not os.path.exists(exe):
        raise FileNotFoundError(exe)
    with tempfile.TemporaryDirectory() as td:
        sp = os.path.join(td, "scene.crts")
        op = os.path.join(td, "out.f32")
        with open(sp, "wb") as f:
            f.write(blob)
        cmd = [exe, sp, op, "--depth", str(max_depth), "--mode", mode, "--repeat", str(repeat)]
        if ppm_path:
            cmd += ["--ppm", ppm_path]
        if gi:
            cmd += ["--gi", str(int(gi[0])), str(int(gi[1]))]
        if all_frames:
            cmd += ["--all-frames"]
        if cpus:
            cmd = ["taskset", "-c", cpus] + cmd
        r = subprocess.run(cmd, capture_output=True, text=True, check=True)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        rgb = np.fromfile(op, dtype=np.float32)
        rgb = rgb.reshape(-1, info["height"], info["width"], 3) if all_frames else rgb.reshape(info["height"], info["width"], 3)
    return rgb, info


# ---- single rays through the real reference (oracle/ref_driver.cpp --rays): its own intersect, checkForIntersection and shootRay
REF_HIT_DTYPE = np.dtype([("t", np.float32), ("point", np.float32, 3), ("normal", np.float32, 3), ("u", np.float32), ("v", np.float32),
                          ("mesh", np.uint32), ("triangle", np.uint32), ("hit", np.uint32)])   # triangle: index within its mesh


def _reference_rays(blob, payload, what, ray_types, textured, extra, dtype, seeds=None):
    """one run of the driver's ray mode; ray_types: a list (its trees take longer to build than a few thousand rays to answer);
    seeds: uint32 per ray, handed over as --seeds (the GI variants)"""
    if textured is None:
        textured = blob[80:84] != b"\x00\x00\x00\x00"
    exe = REF_TEX if textured else REF_PLAIN
    if not os.path.exists(exe):
        raise FileNotFoundError(exe)
    with tempfile.TemporaryDirectory() as td:
        sp, rp, op = (os.path.join(td, n) for n in ("scene.crts", "rays.bin", "out.bin"))
        with open(sp, "wb") as f:
            f.write(blob)
        with open(rp, "wb") as f:
            for a in payload:
                f.write(np.ascontiguousarray(a, dtype="<u4" if a.dtype == np.uint32 else "<f4").tobytes())
        if seeds is not None:
            with open(os.path.join(td, "seeds.bin"), "wb") as f:
                f.write(np.ascontiguousarray(seeds, dtype="<u4").tobytes())
            extra = extra + ["--seeds", os.path.join(td, "seeds.bin")]
        subprocess.run([exe, "--rays", sp, rp, op, "--what", what, "--type", ",".join(str(int(t)) for t in ray_types)] + extra,
                       capture_output=True, text=True, check=True, timeout=900)
        return np.fromfile(op, dtype=dtype)


def _rays6(rays):
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    if rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError("rays: expected shape [n, 6], got %r" % (rays.shape,))
    return rays


def reference_trace(blob: bytes, rays, ray_type, textured=None):
    """AccelerationStructure(scene).intersect(Ray(origin, direction, ray_type)) of the real reference for every ray (float32 [n, 6],
    directions as given) -> REF_HIT_DTYPE [n]; no hit: every field 0.  u, v come from the USE_TEXTURES build only (textured=True runs
    that build on a scene without textures too: its materials become constant-albedo textures, Texture.cpp:14-16).  ray_type may be
    a list: -> [len(ray_type), n] from one run."""
    rays = _rays6(rays)
    types = list(ray_type) if np.ndim(ray_type) else [ray_type]
    out = _reference_rays(blob, [rays], "trace", types, textured, [], REF_HIT_DTYPE).reshape(len(types), len(rays))
    return out if np.ndim(ray_type) else out[0]


def reference_occluded(blob: bytes, rays, distances, gi=False):
    """checkForIntersection(ray, distances[i], useGI=gi) of the real reference for every ray as a ShadowRay -> bool [n]."""
    rays = _rays6(rays)
    dist = np.ascontiguousarray(np.broadcast_to(np.asarray(distances, dtype=np.float32), (len(rays),)))
    out = _reference_rays(blob, [rays, dist], "occluded", [1], None, ["--gi-occlusion"] if gi else [], np.uint8)
    assert out.shape == (len(rays),)
    return out.astype(bool)


def reference_shoot(blob: bytes, rays, ray_type, max_depth):
    """RayTracer::shootRay(Ray(origin, direction, ray_type), 0) of the real reference with MAX_DEPTH = max_depth and the tracer's state
    as render() leaves it for the default tree mode -> float32 [n, 3].  ray_type and max_depth may both be lists:
    -> [len(ray_type), len(max_depth), n, 3] from one run."""
    rays = _rays6(rays)
    lists = bool(np.ndim(ray_type))
    types, depths = (list(ray_type), list(max_depth)) if lists else ([ray_type], [max_depth])
    out = _reference_rays(blob, [rays], "shoot", types, None, ["--depth", ",".join(str(int(d)) for d in depths)], np.float32)
    out = out.reshape(len(types), len(depths), len(rays), 3)
    return out if lists else out[0, 0]


# ---- the GI mode of the real reference on a known stream: the driver seeds RayTracer::engine (the reference's own thread_local member)
# before every ray, so shootRay's and getRay's draws are the reference's distribution(engine) for that seed
def reference_gi_draws(first, count):
    """For every seed of [first, first + count): the engine seeded with it, then distribution(engine) twice -> uint32 [count, 2], the
    float32 bit patterns of the two draws."""
    if not os.path.exists(REF_PLAIN):
        raise FileNotFoundError(REF_PLAIN)
    with tempfile.TemporaryDirectory() as td:
        op = os.path.join(td, "draws.bin")
        subprocess.run([REF_PLAIN, "--gi-draws", str(int(first)), str(int(count)), op], capture_output=True, text=True, check=True, timeout=900)
        return np.fromfile(op, dtype="<u4").reshape(int(count), 2)


def _gi_extra(gi_sample_size, max_depth, monte_carlo_bias):
    return ["--gi", str(int(gi_sample_size)), "--depth", str(int(max_depth)), "--monte-carlo-bias", repr(float(monte_carlo_bias))]


def reference_shoot_gi(blob: bytes, rays, seeds, ray_type, max_depth, gi_sample_size=1, monte_carlo_bias=1e-4):
    """RayTracer::shootRay(Ray(origin, direction, ray_type), 0) of the real reference in the GI mode (USE_GI, GI_SAMPLE_SIZE, MAX_DEPTH,
    MONTE_CARLO_BIAS as given), the engine seeded with seeds[i] before ray i -> float32 [n, 3]."""
    rays = _rays6(rays)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    assert seeds.shape == (len(rays),)
    out = _reference_rays(blob, [rays], "shoot", [ray_type], None, _gi_extra(gi_sample_size, max_depth, monte_carlo_bias), np.float32, seeds=seeds)
    return out.reshape(len(rays), 3)


def reference_camera_rays(blob: bytes, rows, cols, seeds, centre=False, max_depth=1, gi_sample_size=1, monte_carlo_bias=1e-4):
    """centre=False: the Ray RayTracer::getRay(row, col, true) returns with the engine seeded with seeds[i] -> float32 [n, 6].
    centre=True: getRay(row, col, false) and, the engine seeded, shootRay of that ray in the GI mode -> (float32 [n, 6], float32 [n, 3])."""
    pixels = np.ascontiguousarray(np.stack([rows, cols], axis=1), dtype=np.uint32)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    assert seeds.shape == (len(pixels),)
    extra = _gi_extra(gi_sample_size, max_depth, monte_carlo_bias) + (["--centre"] if centre else [])
    out = _reference_rays(blob, [pixels], "camera", [0], None, extra, np.float32, seeds=seeds).reshape(len(pixels), 9 if centre else 6)
    return (np.ascontiguousarray(out[:, :6]), np.ascontiguousarray(out[:, 6:])) if centre else out
