"""The probe volume's visibility term, what needs no GPU: the contract in include/crt_hip.h ("Probe visibility"), the exported symbols, the
numpy restatement of the rule (tests/probe_depth_sets.py) held to the host build of csrc/probe_depth_rule.h -- the header the kernels
compile --, the octahedral wrap, the known answers, the identity with the plain lookup, the hits of the pinned and the partition volume's
rays against tests/golden/probe_depth.npz, which records what the real reference answered (tests/golden/make_probe_depth.py), and the
quality numbers of DESIGN.md section 8r."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import probe_depth_sets as pd
import probe_sets as ps

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "course-assignment-danielhalachev_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "probe_depth.npz")
SYMBOLS = ["crt_probe_visibility_defaults", "crt_probe_depth_device", "crt_probe_irradiance_visible_device", "crt_probe_irradiance_visible",
           "crt_bake_probes_visible"]
F32, U32 = np.float32, np.uint32


def running_text(path, margin):
    return re.sub(r"\s+", " ", re.sub(margin, " ", open(path).read()))


def test_header_states_the_rule_and_the_limits():
    text = running_text(os.path.join(ROOT, "include", "crt_hip.h"), r"\n \*")
    src = open(os.path.join(CSRC, "probe_depth_rule.h")).read().split("\n")
    first = next(i for i, l in enumerate(src) if l.startswith("// Depth record."))
    last = next(i for i, l in enumerate(src) if l.startswith("#pragma once"))
    rule = " ".join(" ".join(l[2:] for l in src[first:last]).split())
    assert "Probe visibility" in text and rule in text                       # the rule's comment stands in the header verbatim
    assert text.index("Irradiance probes") < text.index("Probe visibility") < text.index("one scene on several devices")
    for line in ["crt_probe_depth is 512 bytes", "qx = (((float)col + 0.5f) / 8.0f) * 2.0f - 1.0f", "sgn(v) = v >= 0 ? 1.0f : -1.0f",
                 "r = (h.hit != 0 && h.t < max_distance) ? h.t : max_distance", "w = c^16 by four squarings",
                 "W = W + w; S1 = S1 + w * r; S2 = S2 + w * (r * r)", "g = (p * 0.5f + 0.5f) * 8.0f - 0.5f", "tx < 0: tx = 0, ty = 7 - ty",
                 "dist = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z)", "ch = var / (var + e * e); ch = (ch * ch) * ch",
                 "vis = ch > min_weight ? ch : min_weight", "max_distance = 1.5f * diag", "normal_bias = 0.02f * the smallest spacing",
                 "variance_floor = 1e-6f * (max_distance * max_distance)", "min_weight = 0.01f", "The map's side is fixed at 8",
                 "There is no direction factor", "Back-face hits count with their own distance", "One max_distance per volume", "Static scenes",
                 "Single-device contexts only"]:
        assert line in rule, line
    # the plain lookup's section still says what it lacks, and the new one says which calls lift it
    assert "There is no visibility (Chebyshev) term, so light leaks through thin walls." in text
    assert "the calls of this section lift that limit" in text
    for banned in ("pow", "exp"):
        code = "\n".join(l for l in src[last:] if not l.lstrip().startswith("//"))
        assert not re.search(r"\b%sf?\(" % banned, code), banned


def test_the_symbols_are_exported_and_declared(pkg):
    L = pkg.lib()
    plain = C.CDLL(os.path.join(os.path.dirname(pkg.LIB_PATH), "libcrt_hip.so"))
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for name in SYMBOLS:
        assert name in pkg.DEVICE_SYMBOLS and hasattr(L, name) and hasattr(plain, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert hasattr(L, "crt_debug_set_probe_chunk") and not hasattr(plain, "crt_debug_set_probe_chunk")
    hooks = re.search(r"Test hooks: exported by libcrt_hip_test.so only.*?---- \*/", header, re.S).group(0)
    assert not any(name in hooks for name in SYMBOLS)                         # no new test hook
    for name in ("bake_probes_visible", "probe_depth_device", "probe_irradiance_visible", "probe_irradiance_visible_device"):
        assert callable(getattr(pkg.Tracer, name)), name
    assert C.sizeof(pkg.ProbeVisibility) == 20 and pkg.PROBE_DEPTH_DTYPE.itemsize == 512 and pkg.PROBE_DEPTH_DTYPE == pd.DEPTH_DTYPE
    assert C.sizeof(pkg.ProbeStats) == 48
    text = open(os.path.join(CSRC, "crt_probes.hip")).read()
    assert "sizeof(crt_probe_depth) == 512" in text and "sizeof(crt_probe_visibility) == 20" in text
    # no context is an error, not a crash
    v = pkg.make_probe_volume()
    p = pkg.make_probe_visibility(v)
    assert L.crt_probe_depth_device(None, None, None, 1, 1, 1.0, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_irradiance_visible_device(None, C.byref(v), C.byref(p), None, None, None, None, 1, None, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_irradiance_visible(None, C.byref(v), C.byref(p), None, None, None, None, 1, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_bake_probes_visible(None, C.byref(v), C.byref(p), None, None, None, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_visibility_defaults(None, C.byref(p)) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_visibility_defaults(C.byref(v), None) == pkg.CRT_ERR_INVALID
    assert L.crt_probe_visibility_defaults(C.byref(pkg.make_probe_volume(nx=0)), C.byref(p)) == pkg.CRT_ERR_INVALID


def test_the_defaults_are_the_documented_values(pkg):
    for spacing in ((1, 1, 1), (0.75, 1.3, 0.4), (4.0, 2.0, 4.0)):
        vol = pkg.make_probe_volume(spacing=spacing, nx=2, ny=2, nz=2)
        p = pkg.make_probe_visibility(vol)
        s = np.array(spacing, dtype=F32)
        diag = np.sqrt(F32(F32(s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
        mx = F32(1.5) * diag
        assert p.size == 20
        assert [F32(p.max_distance), F32(p.normal_bias), F32(p.variance_floor), F32(p.min_weight)] == \
            [mx, F32(0.02) * s.min(), F32(1e-6) * F32(mx * mx), F32(0.01)], spacing
        want = pd.Visibility(ps.Volume(spacing=spacing))
        assert [F32(p.max_distance), F32(p.normal_bias), F32(p.variance_floor), F32(p.min_weight)] == \
            [want.max_distance, want.normal_bias, want.variance_floor, want.min_weight]
    assert pkg.make_probe_visibility(vol, min_weight=0.5).min_weight == 0.5


class Grid(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("n", C.c_uint32 * 3), ("rays", C.c_uint32), ("gi_seed", C.c_uint32),
                ("backface_limit", C.c_float)]


class Vis(C.Structure):
    _fields_ = [("size", C.c_uint32), ("max_distance", C.c_float), ("normal_bias", C.c_float), ("variance_floor", C.c_float), ("min_weight", C.c_float)]


def grid_of(v):
    return Grid((C.c_float * 3)(*v.origin), (C.c_float * 3)(*v.spacing), (C.c_uint32 * 3)(*v.n), v.rays, v.gi_seed, float(v.backface_limit))


def vis_of(p):
    return Vis(20, float(p.max_distance), float(p.normal_bias), float(p.variance_floor), float(p.min_weight))


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.gettempdir(), "crt_probe_depth_rule_shim_%d.so" % os.getuid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", os.path.join(HERE, "probe_depth_rule_shim.cpp"), "-o", out])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.shim_depth_directions.argtypes = [vp]
    lib.shim_depth_defaults.argtypes = [C.POINTER(Grid), C.POINTER(Vis)]
    lib.shim_depth_vis_valid.argtypes = [C.POINTER(Vis)]
    lib.shim_depth_project.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_float, vp]
    lib.shim_depth_tap.argtypes = [vp, C.c_uint64, vp, vp, vp, vp]
    lib.shim_depth_lookup.argtypes = [C.POINTER(Grid), C.POINTER(Vis), vp, vp, vp, vp, C.c_uint64, vp, vp]
    for f in (lib.shim_depth_directions, lib.shim_depth_defaults, lib.shim_depth_project, lib.shim_depth_tap, lib.shim_depth_lookup):
        f.restype = None
    return lib


PLACE = dict(origin=(-1.25, 0.3, -4.0), spacing=(0.75, 1.3, 0.4), gi_seed=77)
VOLUMES = [dict(nx=1, ny=1, nz=1), dict(nx=2, ny=3, nz=1), dict(nx=3, ny=2, nz=4), dict(nx=1, ny=4, nz=1)]


def test_the_numpy_texel_directions_are_the_headers(shim):
    got = np.zeros((64, 3), dtype=F32)
    shim.shim_depth_directions(got.ctypes.data)
    e = pd.texel_directions()
    assert np.array_equal(got.view(U32), e.view(U32))
    d = e.astype(np.float64)
    assert np.abs((d * d).sum(axis=1) - 1).max() < 2.0 ** -22 and (e[:, 2] > 0).sum() == 24 and (e[:, 2] < 0).sum() == 24 and len(np.unique(e, axis=0)) == 64
    # a texel's own direction taps its own texel with the whole weight (to rounding)
    for k in range(64):
        ks, ws = pd.taps(e[k])
        assert ks[int(np.argmax(ws))] == k and max(ws) > 0.999, k


def test_the_defaults_and_the_validity_are_the_headers(shim):
    for spacing in ((1, 1, 1), (0.75, 1.3, 0.4)):
        v = ps.Volume(spacing=spacing)
        got = Vis()
        g = grid_of(v)
        shim.shim_depth_defaults(C.byref(g), C.byref(got))
        want = pd.Visibility(v)
        assert (got.size, F32(got.max_distance), F32(got.normal_bias), F32(got.variance_floor), F32(got.min_weight)) == \
            (20, want.max_distance, want.normal_bias, want.variance_floor, want.min_weight)
        assert shim.shim_depth_vis_valid(C.byref(got)) == 1
    for change in INVALID_VISIBILITY:
        bad = vis_of(pd.Visibility(ps.Volume()))
        for k, val in change.items():
            setattr(bad, k, val)
        assert shim.shim_depth_vis_valid(C.byref(bad)) == 0, change


INVALID_VISIBILITY = [dict(size=0), dict(size=16), dict(size=24), dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=float("inf")),
                      dict(max_distance=float("nan")), dict(normal_bias=-1e-3), dict(normal_bias=float("inf")), dict(normal_bias=float("nan")),
                      dict(variance_floor=0.0), dict(variance_floor=-1.0), dict(variance_floor=float("inf")), dict(variance_floor=float("nan")),
                      dict(min_weight=0.0), dict(min_weight=-0.5), dict(min_weight=1.5), dict(min_weight=float("nan")), dict(min_weight=float("inf"))]


@pytest.mark.parametrize("R", ps.RAY_COUNTS)
def test_the_numpy_projection_is_the_header(shim, R):
    rng = np.random.default_rng(R)
    for count, mx in ((1, 2.5), (3, 0.75)):
        v = ps.Volume(rays=R, nx=count, **PLACE)
        rays, _ = ps.rays_and_keys(v, 0, count)
        hit, t = pd.special_hits(rng, count * R, mx)
        got = np.zeros((count, 64, 2), dtype=F32)
        shim.shim_depth_project(rays.ctypes.data, hit.ctypes.data, t.ctypes.data, count, R, mx, got.ctypes.data)
        want = pd.project(rays, hit, t, count, R, mx)
        pd.same_depth(got, want, "R = %d, %d probes" % (R, count))
        assert np.isfinite(want).all() and (want[:, :, 0] >= 0).all() and (want[:, :, 0] <= F32(mx)).all()
    # the special distances one by one: what a ray counts with
    mx = F32(2.5)
    t = np.array(pd.SPECIAL_T + [mx, np.nextafter(mx, F32(np.inf)), np.nextafter(mx, F32(0.0)), 1.0, 1.0], dtype=F32)
    hit = np.ones(len(t), dtype=U32)
    hit[-1] = 0
    want = [0.0, 0.0, 1e-42, 0.0, mx, 0.0, mx, mx, mx, np.nextafter(mx, F32(0.0)), 1.0, mx]
    assert np.array_equal(pd.distances(hit, t, mx).view(U32), np.array(want, dtype=F32).view(U32))


def tap_directions(rng):
    """random directions, the six axes, the map's four corners (all -z) and edge midpoints, directions on the seams, zeros and non-finite"""
    u = rng.normal(size=(300, 3))
    u = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F32)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(F32)
    s = F32(np.sqrt(0.5))
    mids = np.array([(s, 0, -s), (-s, 0, -s), (0, s, -s), (0, -s, -s), (s, s, 0), (-s, s, 0), (s, -s, 0), (-s, -s, 0)], dtype=F32)
    near = np.array([(1e-7, -1e-7, -1), (-1e-7, 1e-7, -1), (1e-7, 1e-7, -1), (-1e-7, -1e-7, -1), (-0.0, 0.0, -1.0), (0.0, -0.0, 1.0)], dtype=F32)
    odd = np.array([(0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 1), (0, -np.inf, -1), (3e38, 3e38, 3e38), (1e-40, 0, -1e-40), (2, -3, 0.5)], dtype=F32)
    return np.concatenate([u, axes, mids, near, odd])


def test_the_numpy_tap_is_the_header(shim):
    rng = np.random.default_rng(12)
    u = tap_directions(rng)
    pairs = rng.uniform(0.1, 3.0, (64, 2)).astype(F32)
    k, w, m = np.zeros((len(u), 4), dtype=U32), np.zeros((len(u), 4), dtype=F32), np.zeros((len(u), 2), dtype=F32)
    shim.shim_depth_tap(u.ctypes.data, len(u), pairs.ctypes.data, k.ctypes.data, w.ctypes.data, m.ctypes.data)
    assert (k < 64).all()
    for i, d in enumerate(u):
        ks, ws = pd.taps(d)
        assert ks == k[i].tolist(), (i, d)
        pd.same_depth(w[i], np.array(ws, dtype=F32), "weights of %r" % (d,))
        pd.same_depth(m[i], np.array(pd.tap(d, pairs), dtype=F32), "moments of %r" % (d,))
    # every wrapped index of the whole [-1, 8]^2 range is a texel, and an interior one is itself
    for ty in range(-1, 9):
        for tx in range(-1, 9):
            assert 0 <= pd.wrap(tx, ty) < 64
            if 0 <= tx < 8 and 0 <= ty < 8:
                assert pd.wrap(tx, ty) == ty * 8 + tx
    assert (pd.wrap(-1, 3), pd.wrap(8, 3), pd.wrap(3, -1), pd.wrap(3, 8), pd.wrap(-1, -1), pd.wrap(8, 8)) == (4 * 8, 4 * 8 + 7, 4, 7 * 8 + 4, 63, 0)


def lookup_cases(rng, v):
    """on probes (dist == 0 without a bias), on the far faces, outside on every side, random ones, non-finite ones"""
    n = np.array(v.n)
    span = v.spacing * (n - 1)
    on = ps.positions(v, np.arange(v.count))
    far = v.origin + span
    outside = np.array([v.origin - 1.5, far + 1.5] + [np.where(np.arange(3) == k, side, v.origin + span / 2) for k in range(3)
                                                      for side in ((v.origin - 2.0)[k], (far + 2.0)[k])], dtype=F32)
    inside = (v.origin + rng.uniform(-0.2, 1.2, (120, 3)) * np.maximum(span, 1.0)).astype(F32)
    pts = np.concatenate([on, far[None, :], outside, inside]).astype(F32)
    nrm = rng.normal(size=pts.shape).astype(F32)
    huge = np.array([(3e38, -3e38, 3e38)], dtype=F32)
    bad_p, bad_n = np.tile(inside[:6], (1, 1)), rng.normal(size=(6, 3)).astype(F32)
    for k, value in enumerate([np.nan, np.inf, -np.inf]):
        bad_p[k, k] = value
        bad_n[3 + k, k] = value
    return np.concatenate([pts, huge, bad_p]), np.concatenate([nrm, np.array([(3e38, 3e38, -3e38)], dtype=F32), bad_n])


def synthetic(rng, v, invalid):
    rec = np.zeros(v.count, dtype=ps.PROBE_DTYPE)
    rec["coef"] = rng.uniform(-0.5, 2.0, (v.count, 9, 3)).astype(F32)
    rec["rays"] = v.rays
    rec["state"] = ps.VALID
    rec["state"][invalid] = ps.INVALID
    mean = rng.uniform(0.05, 1.5, (v.count, 64)).astype(F32)
    depth = np.stack([mean, mean * mean + rng.uniform(0.0, 0.2, (v.count, 64)).astype(F32)], axis=2).astype(F32)
    return rec, depth


def test_the_numpy_lookup_is_the_header(shim):
    rng = np.random.default_rng(8)
    seen = set()
    for dims in VOLUMES:
        v = ps.Volume(rays=64, **dict(PLACE, **dims))
        rec, depth = synthetic(rng, v, rng.uniform(size=v.count) < 0.3)
        rec["state"][rng.integers(v.count)] = 7                          # neither state: taken as INVALID
        depth[0, 5] = (np.nan, 1.0)
        depth[-1, 9] = (np.inf, np.inf)
        pts, nrm = lookup_cases(rng, v)
        for bias in (None, 0.0):                                         # 0: a point AT a probe has dist == 0
            vis = pd.Visibility(v, normal_bias=bias)
            weights = []
            want_rgb, want_status = pd.lookup(v, vis, rec, depth, pts, nrm, weights=weights)
            rgb, status = np.full((len(pts), 3), 9, dtype=F32), np.full(len(pts), 9, dtype=np.uint8)
            g, p = grid_of(v), vis_of(vis)
            shim.shim_depth_lookup(C.byref(g), C.byref(p), rec.ctypes.data, depth.ctypes.data, pts.ctypes.data, nrm.ctypes.data, len(pts), rgb.ctypes.data,
                                   status.ctypes.data)
            ps.same_colours(rgb, want_rgb, repr(dims))
            assert np.array_equal(status, want_status), dims
            assert (status[-6:] == 0).all() and not rgb[-6:].any()
            w = np.array([x[2] for x in weights])
            assert (w >= float(vis.min_weight)).all() and (w <= 1.0).all()
            seen |= {"floor" if x == float(vis.min_weight) else ("one" if x == 1.0 else "between") for x in w}
    assert seen == {"floor", "one", "between"}


def test_the_rule_runs_clean_under_sanitizers(tmp_path):
    """a stand-alone program around the header's host build, with -fsanitize=address,undefined"""
    exe = str(tmp_path / "probe_depth_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DPROBE_DEPTH_RULE_MAIN", os.path.join(HERE, "probe_depth_rule_shim.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.strip().splitlines()) == 18


# ------------------------------------------------------------------------------------------------------------------------ the wrap
def smooth_map():
    """a map whose texel k holds a smooth function of e_k"""
    e = pd.texel_directions().astype(np.float64)
    f = 2.0 + e[:, 0] + 0.5 * e[:, 1] * e[:, 2] - 0.7 * e[:, 2]
    return np.stack([f, f * f], axis=1)


def test_the_wrap_is_continuous_across_the_maps_edges():
    """Across an edge of the octahedral square the sphere goes on: a direction half a step inside an edge and the direction half a step
    beyond it -- which lies inside the map again, mirrored along that edge -- are a step apart, and their taps, in float64 on a map filled
    with a smooth function of e_k, may differ by no more than two taps the same step apart differ in the map's interior.  The bound is the
    largest interior difference measured here for that step over 2 000 random pairs along either axis, times 1.25: the margin is for what
    random pairs miss of the map's true largest slope (the function's gradient varies by less than that between neighbouring texels).  A
    wrap that clamps at the edge, restated in tests/probe_depth_sets.py for this test only, is measured on the same seam pairs: it reads
    the wrong neighbours, must exceed the bound, and so shows that this test can see a wrong wrap."""
    rng = np.random.default_rng(4)
    pairs = smooth_map()
    step = 0.02                                                             # in map units: a texel is 0.25 wide
    interior = seam = clamped = 0.0
    T = np.float64
    # the measurement proper, in map coordinates: the lower sheet (z < 0) fills the square's four corner triangles up to its edges
    for _ in range(2000):
        axis = int(rng.integers(2))
        side = 1.0 if rng.uniform() < 0.5 else -1.0
        along = rng.uniform(-0.95, 0.95)
        # a point half a step inside the edge `axis = side`, and the point half a step beyond it: mirrored back in along the edge
        p_in = np.zeros(2)
        p_in[axis], p_in[1 - axis] = side * (1.0 - step / 2), along
        p_out = np.zeros(2)
        p_out[axis], p_out[1 - axis] = side * (1.0 - step / 2), -along
        a, b = pd.tap(folded_direction(p_in), pairs, T), pd.tap(folded_direction(p_out), pairs, T)
        seam = max(seam, abs(a[0] - b[0]))
        ca, cb = pd.tap(folded_direction(p_in), pairs, T, pd.clamp_wrap), pd.tap(folded_direction(p_out), pairs, T, pd.clamp_wrap)
        clamped = max(clamped, abs(ca[0] - cb[0]))
        # an interior pair the same step apart, anywhere at least a texel from the edges, along either axis
        q = rng.uniform(-0.7, 0.7, 2)
        q2 = q.copy()
        q2[axis] += step
        if (np.abs(q).sum() < 1.0) != (np.abs(q2).sum() < 1.0):
            continue                                                        # (the pair straddles the fold: it is a seam of its own kind)
        a, b = pd.tap(folded_direction(q), pairs, T), pd.tap(folded_direction(q2), pairs, T)
        interior = max(interior, abs(a[0] - b[0]))
    bound = 1.25 * interior
    print("step %.3f: largest interior difference %.5f, across the seam %.5f (bound %.5f), a clamping wrap's error at the edge %.5f"
          % (step, interior, seam, bound, clamped))
    assert interior > 0 and seam <= bound
    assert clamped > bound


def folded_direction(p):
    """the unit direction whose octahedral encoding is the map point p (|p.x|, |p.y| <= 1)"""
    p = np.asarray(p, dtype=np.float64)
    z = 1.0 - np.abs(p).sum()
    if z >= 0:
        d = np.array([p[0], p[1], z])
    else:
        f = (1.0 - np.abs(p[::-1])) * np.where(p >= 0, 1.0, -1.0)
        d = np.array([f[0], f[1], z])
    return d / np.linalg.norm(d)


# ------------------------------------------------------------------------------------------------------------------------ known answers
def test_known_answers_of_the_projection():
    for R in (1, 64, 100):
        v = ps.Volume(rays=R)
        rays, _ = ps.rays_and_keys(v, 0, 1)
        mx, a = F32(4.0), F32(1.3)          # (a power of two: w * max and w * max^2 are exact, so S1 == max * W in every bit)
        # every ray at distance a < max: S1 / W is a weighted mean of equal values.  Each of the 2 R fold steps of S1 (a product, a sum)
        # and the R of W and the division round once, each by at most 2^-24 relative to a partial sum that is at most the final one (all
        # terms are >= 0): |mean - a| <= (3 R + 1) * 2^-24 * a, and likewise mean2 with one more product per ray: (4 R + 1) * 2^-24 * a^2
        got = pd.project(rays, np.ones(R, dtype=U32), np.full(R, a, dtype=F32), 1, R, mx)[0].astype(np.float64)
        seen = got[:, 0] != float(mx)
        assert np.abs(got[seen, 0] - float(a)).max() <= (3 * R + 1) * 2.0 ** -24 * float(a)
        assert np.abs(got[seen, 1] - float(a) ** 2).max() <= (4 * R + 1) * 2.0 ** -24 * float(a) ** 2
        if R >= 64:
            assert seen.all()
        # all misses, and all hits beyond max: (max, max^2) exactly
        for hit, t in ((np.zeros(R, dtype=U32), np.full(R, a, dtype=F32)), (np.ones(R, dtype=U32), np.full(R, 7.0, dtype=F32))):
            got = pd.project(rays, hit, t, 1, R, mx)[0]
            assert np.array_equal(got.view(U32), np.tile(np.array([mx, mx * mx], dtype=F32), (64, 1)).view(U32))
    # R = 1: the single ray points to -z (z = 1 - 1 / 1 = 0 ... the set's one direction); the texels with c = 0 take the fallback
    v = ps.Volume(rays=1)
    rays, _ = ps.rays_and_keys(v, 0, 1)
    got = pd.project(rays, np.ones(1, dtype=U32), np.array([0.5], dtype=F32), 1, 1, 3.0)[0]
    c = pd.sum3(np.tile(rays[0, 3:], (64, 1)), pd.texel_directions())
    w = np.maximum(c, F32(0.0)) ** 16
    away = ~(w > 0)
    assert away.sum() >= 16 and (~away).sum() >= 16
    assert np.array_equal(got[away].view(U32), np.tile(np.array([3.0, 9.0], dtype=F32), (int(away.sum()), 1)).view(U32))
    assert np.abs(got[~away, 0].astype(np.float64) - 0.5).max() <= 4 * 2.0 ** -24


def test_with_nothing_hidden_the_lookup_is_the_plain_one():
    """every pair (max, max^2), every corner within max of the biased point: vis == 1 at every corner, and 1.0f * wc is wc"""
    rng = np.random.default_rng(31)
    for dims in VOLUMES:
        v = ps.Volume(rays=64, **dict(PLACE, **dims))
        rec, _ = synthetic(rng, v, rng.uniform(size=v.count) < 0.3)
        vis = pd.Visibility(v)
        mx = vis.max_distance
        depth = np.tile(np.array([mx, mx * mx], dtype=F32), (v.count, 64, 1))
        span = v.spacing * (np.array(v.n) - 1)
        pts = np.concatenate([(v.origin + rng.uniform(-0.05, 1.05, (150, 3)) * span).astype(F32), ps.positions(v, np.arange(v.count))])
        nrm = rng.normal(size=pts.shape).astype(F32)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        weights = []
        got_rgb, got_status = pd.lookup(v, vis, rec, depth, pts, nrm, weights=weights)
        assert all(w[2] == 1.0 for w in weights) and len(weights) >= len(pts) // 2
        want_rgb, want_status = ps.lookup(v, rec, pts, nrm)
        ps.same_colours(got_rgb, want_rgb, repr(dims))
        assert np.array_equal(got_status, want_status)


# ------------------------------------------------------------------------------------------------------------------------ the reference
def oracle_hit_t(o, rays):
    hit, t = np.zeros(len(rays), dtype=U32), np.zeros(len(rays), dtype=F32)
    for i, r in enumerate(rays):
        h, rec = o.trace(r[:3], r[3:], 2)
        hit[i], t[i] = h, rec[0] if h else 0
    return hit, t


def cases(scenes):
    return (("pin", ps.room(scenes), ps.PIN_VOLUME), ("part", pd.partition_room(scenes), pd.PARTITION_VOLUME))


def test_golden_hits_are_the_oracles(scenes, oracle):
    z = np.load(GOLDEN)
    for name, scene, fields in cases(scenes):
        v = ps.Volume(**fields)
        rays, _ = ps.rays_and_keys(v, 0, v.count)
        o = oracle.OracleScene(scenes.to_blob(scene))
        hit, t = oracle_hit_t(o, rays)
        assert len(rays) == 512 and np.array_equal(hit, z[name + "_hit"]), name
        assert np.array_equal(t.view(U32), z[name + "_t"].view(U32)), name
        assert 400 < int(hit.sum()) < 512                                    # hits and misses both
        if name == "part":
            ps.same_colours(ps.oracle_shoot(o, rays), z["part_rgb"], "the oracle's colours against the recorded reference")


def test_golden_hits_are_the_live_references(scenes, oracle):
    if not oracle.reference_available():
        pytest.skip("the real reference is not built")
    z = np.load(GOLDEN)
    for name, scene, fields in cases(scenes):
        v = ps.Volume(**fields)
        rays, _ = ps.rays_and_keys(v, 0, v.count)
        blob = scenes.to_blob(scene)
        hits = oracle.reference_trace(blob, rays, 2)
        assert np.array_equal(hits["hit"].astype(U32), z[name + "_hit"]) and np.array_equal(hits["t"].view(U32), z[name + "_t"].view(U32)), name
        if name == "part":
            ps.same_colours(oracle.reference_shoot(blob, rays, 2, 5), z["part_rgb"], "the live reference against the recording")


# ------------------------------------------------------------------------------------------------------------------------ the partition scene
def partition_world():
    z = np.load(GOLDEN)
    v = ps.Volume(**pd.PARTITION_VOLUME)
    rays, _ = ps.rays_and_keys(v, 0, v.count)
    vis = pd.Visibility(v)
    rec = ps.project(rays, z["part_rgb"], v.count, v.rays)
    depth = pd.project(rays, z["part_hit"], z["part_t"], v.count, v.rays, vis.max_distance)
    return v, vis, rec, depth


def test_the_partition_scene_is_what_the_tests_need(scenes):
    v = ps.Volume(**pd.PARTITION_VOLUME)
    pos = ps.positions(v, np.arange(v.count)).astype(np.float64)
    assert (np.abs(pos[:, 0] - pd.PARTITION_X) > 10 * pd.PARTITION_HALF).all()                 # no probe in the partition
    assert (pos[:, 0] < pd.PARTITION_X).sum() == 4 and (pos[:, 0] > pd.PARTITION_X).sum() == 4   # a column on each side
    assert (np.abs(pos[:, 0] - pd.PARTITION_X) <= float(v.spacing[0])).all()                   # within one cell of it
    for centre, radius in (((-1.25, -0.65, -5.0), 0.85), ((1.15, -0.55, -3.9), 0.8)):          # no probe in a sphere
        assert (np.linalg.norm(pos - np.array(centre), axis=1) > radius + 0.05).all()
    scene = pd.partition_room(scenes)
    assert len(scene["lights"]) == 1 and all(l["position"][0] > pd.PARTITION_X for l in scene["lights"])
    assert v.backface_limit == 1.0


def test_visibility_shrinks_the_leak_through_the_partition():
    """CPU: the recorded reference's colours and hits, the restatement.  At a fixed grid of dark-side points facing away from the partition,
    inside the cell that straddles it, the plain lookup is > 0 in every channel -- the leak exists -- and the visible lookup is strictly
    below it in every channel at every point.  The remaining leak and the lit side's change are measurements."""
    v, vis, rec, depth = partition_world()
    dark, dark_n = pd.side_points(v, True)
    lit, lit_n = pd.side_points(v, False)
    assert len(dark) == 18 and (dark[:, 0] < pd.PARTITION_X).all() and (lit[:, 0] > pd.PARTITION_X).all()
    plain_d, status = ps.lookup(v, rec, dark, dark_n)
    vis_d, status_v = pd.lookup(v, vis, rec, depth, dark, dark_n)
    assert (status == 8).all() and np.array_equal(status, status_v)
    assert (plain_d > 0).all()
    assert (vis_d < plain_d).all()
    plain_l, _ = ps.lookup(v, rec, lit, lit_n)
    vis_l, _ = pd.lookup(v, vis, rec, depth, lit, lit_n)
    leak = float(vis_d.astype(np.float64).sum() / plain_d.astype(np.float64).sum())
    ratios = vis_d.astype(np.float64) / plain_d.astype(np.float64)
    lit_change = float(vis_l.astype(np.float64).sum() / plain_l.astype(np.float64).sum()) - 1.0
    print("dark side: the leak that remains, sum(visible) / sum(plain) = %.4f (per value: mean %.4f, least %.4f, most %.6f); lit side: relative change %+.4f"
          % (leak, ratios.mean(), ratios.min(), ratios.max(), lit_change))
    assert leak < 1
    # the defaults are wrong if the lit side darkens by more than the dark side's leak shrinks
    assert -lit_change < 1 - leak
    # the float64 variant of the lookup agrees with the float32 one to float32 rounding of an 8-corner blend of 27-term sums
    vis64, _ = pd.lookup(v, vis, rec, depth, dark, dark_n, float64=True)
    assert np.abs(vis64 - vis_d).max() <= 1e-4 * float(np.abs(vis64).max())
