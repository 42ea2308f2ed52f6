"""What the tests of the probe-lit radiance queries (crt_probe_light_hits_device, crt_shoot_rays_lit*, crt_render_probe_lit) share: the rule
of include/crt_hip.h ("Probe-lit radiance"; csrc/probe_lit_rule.h) restated in numpy -- every line one float32 operation, in the header's
order --, a numpy restatement of gi_sample_direction (csrc/kernel_lane.h) in binary64 for the test of the three constants, and the random
volumes the primitive runs on.  numpy only, no GPU.  The lookup's shared parts are tests/probe_sets.py's and tests/probe_depth_sets.py's."""
import numpy as np

import probe_depth_sets as pd
import probe_sets as ps

F32, U32 = np.float32, np.uint32
ZONAL = np.array([1.0, 0.63661975, 0.63661975, 0.63661975, 0.25, 0.25, 0.25, 0.25, 0.25], dtype=F32)
LAMBDA = (1.0, 2.0 / np.pi, 0.25)                       # the band factors the table rounds
SAMPLES = [0, 1, 2, 7]
BACKGROUND, DIFFUSE, RECURSES, INVALID = range(4)      # CRT_SHADE_*
PLACE = dict(origin=(-1.25, 0.3, -4.0), spacing=(0.75, 1.3, 0.4), gi_seed=77)


def lbar(v, vis, rec, depth, points, normals):
    """-> (Lbar float32 [n, 3], status uint8 [n]): the zonal resolve of the plain (vis None) or the Chebyshev-weighted lookup"""
    rec = np.asarray(rec).reshape(-1)
    if vis is not None:
        depth = np.asarray(depth, dtype=F32).reshape(-1, pd.TEXELS, 2)
    points, normals = np.asarray(points, dtype=F32), np.asarray(normals, dtype=F32)
    out = np.zeros((len(points), 3), dtype=F32)
    status = np.zeros(len(points), dtype=np.uint8)
    for i, (x, n) in enumerate(zip(points, normals)):
        if not (np.isfinite(x).all() and np.isfinite(n).all()):
            continue
        ax = [ps.axis(x[k], v.origin[k], v.spacing[k], v.n[k]) for k in range(3)]
        W, S, used = F32(0.0), np.zeros((9, 3), dtype=F32), 0
        with np.errstate(all="ignore"):
            for dz in range(ax[2][2]):
                for dy in range(ax[1][2]):
                    for dx in range(ax[0][2]):
                        wc = (F32(ax[0][1][dx]) * F32(ax[1][1][dy])) * F32(ax[2][1][dz])
                        if wc == 0:
                            continue
                        p = ((ax[2][0] + dz) * v.n[1] + (ax[1][0] + dy)) * v.n[0] + (ax[0][0] + dx)
                        if p >= len(rec) or rec["state"][p] != ps.VALID:
                            continue
                        w = wc
                        if vis is not None:
                            P = ps.positions(v, [p])[0]
                            vv = (x + n * F32(vis.normal_bias)) - P
                            dist = np.sqrt((vv[0] * vv[0] + vv[1] * vv[1]) + vv[2] * vv[2])
                            visible = F32(1.0)
                            if dist > 0:
                                m1, m2 = pd.tap(vv / dist, depth[p], F32)
                                visible = pd.weight(vis, dist, m1, m2, F32)
                            w = wc * visible
                        W = W + w
                        S = S + w * rec["coef"][p]
                        used += 1
            if not used:
                continue
            Y = ps.basis(n)
            e = np.zeros(3, dtype=F32)
            for c in range(9):
                e = e + (ZONAL[c] * Y[c]) * S[c]
            q = e / W
            out[i] = np.where(q > 0, q, F32(0.0))
        status[i] = used
    return out, status


def combine(direct, lb, S):
    """float32 [..., 3]: (direct + (float)S * Lbar) * (1.0f / (float)(S + 1))"""
    with np.errstate(all="ignore"):
        ind = F32(S) * np.asarray(lb, dtype=F32)
        inv = F32(1.0) / F32(S + 1)
        return ((np.asarray(direct, dtype=F32) + ind) * inv).astype(F32)


def light(v, vis, rec, depth, hits, status, S, rgb):
    """the primitive: -> (rgb float32 [n, 3], lit, unlit); hits a record array with "point" and "normal", status uint8 [n]"""
    rgb = np.array(rgb, dtype=F32).reshape(-1, 3)
    idx = np.flatnonzero(np.asarray(status) == DIFFUSE)
    lb, used = lbar(v, vis, rec, depth, hits["point"][idx], hits["normal"][idx])
    rgb[idx] = combine(rgb[idx], lb, S)
    return rgb, int((used != 0).sum()), int((used == 0).sum())


def random_volume(rng, dims):
    """a volume with random records and depth maps; for 3 x 2 x 4: a cell with eight and one with seven invalid corners"""
    v = ps.Volume(rays=64, **dict(PLACE, **dims))
    rec = np.zeros(v.count, dtype=ps.PROBE_DTYPE)
    rec["coef"] = rng.uniform(-0.5, 2.0, (v.count, 9, 3)).astype(F32)
    rec["rays"] = 64
    rec["state"] = ps.VALID
    if v.n == (3, 2, 4):
        rec["state"][[(iz * 2 + iy) * 3 + ix for iz in (0, 1) for iy in (0, 1) for ix in (0, 1)]] = ps.INVALID
        rec["state"][[(iz * 2 + iy) * 3 + 2 for iz in (0, 1) for iy in (0, 1)]] = [ps.VALID, ps.INVALID, ps.INVALID, ps.INVALID]
        rec["state"][-1] = 7
    mean = rng.uniform(0.05, 1.5, (v.count, 64)).astype(F32)
    depth = np.stack([mean, mean * mean + rng.uniform(0.0, 0.2, (v.count, 64)).astype(F32)], axis=2).astype(F32)
    return v, rec, depth


def random_points(rng, v, n):
    """n points and normals: on probes, in the cells of invalid corners, outside, inside, non-finite"""
    span = v.spacing * (np.array(v.n) - 1)
    cells = np.array([v.origin + v.spacing * np.array([0.4, 0.3, 0.6]), v.origin + v.spacing * np.array([1.4, 0.3, 0.6])], dtype=F32)
    fixed = np.concatenate([cells, ps.positions(v, np.arange(v.count)), np.array([v.origin - 1.5, v.origin + span + 1.5], dtype=F32)]).astype(F32)
    if n < len(fixed):
        pts = fixed[:n].copy()
    else:
        pts = np.concatenate([fixed, (v.origin + rng.uniform(-0.2, 1.2, (n - len(fixed), 3)) * np.maximum(span, 1.0)).astype(F32)])
    nrm = rng.normal(size=pts.shape).astype(F32)
    if n >= 63:
        for k, value in enumerate([np.nan, np.inf, -np.inf]):
            pts[-1 - k, k] = value
            nrm[-4 - k, k] = value
    return pts, nrm


def mixed_status(rng, n):
    """diffuse, recursing, constant (background's byte) and invalid records mixed; record 0 is diffuse"""
    s = rng.choice([DIFFUSE, DIFFUSE, DIFFUSE, RECURSES, BACKGROUND, INVALID], size=n).astype(np.uint8)
    s[0] = DIFFUSE
    return s


# ------------------------------------------------------------------------------------------------------------------------ gi_sample_direction
def gi_sample_direction(d, n, u1, u2):
    """csrc/kernel_lane.h's gi_sample_direction in binary64 for arrays u1, u2: right = cross(d, n), forward = cross(right, n), the vector
    (cos angle1, sin angle1, 0) of the (right, normal, forward) frame, rotated about the normal by angle2 -> float64 [len(u1), 3]"""
    d, n = np.asarray(d, dtype=np.float64), np.asarray(n, dtype=np.float64)
    right = np.cross(d, n)
    right = right / np.linalg.norm(right)
    forward = np.cross(right, n)
    a1, a2 = np.pi * np.asarray(u1, dtype=np.float64), 2.0 * np.pi * np.asarray(u2, dtype=np.float64)
    local = np.stack([np.cos(a1), np.sin(a1), np.zeros_like(a1)], axis=1)            # (right, normal, forward) coordinates
    x = local[:, 0] * np.cos(a2) + local[:, 2] * np.sin(a2)                            # a rotation about the second axis, the normal
    z = -local[:, 0] * np.sin(a2) + local[:, 2] * np.cos(a2)
    return x[:, None] * right[None, :] + local[:, 1, None] * n[None, :] + z[:, None] * forward[None, :]


def basis64(w):
    """float64 [n, 9]: tests/probe_sets.py's basis64 for directions float64 [n, 3]"""
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    return np.stack([np.full(len(w), 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * (x * y), 1.092548 * (y * z),
                     0.315392 * (3.0 * (z * z) - 1.0), 1.092548 * (x * z), 0.546274 * (x * x - y * y)], axis=1)


def legendre(l, c):
    return [np.ones_like(c), c, 0.5 * (3.0 * c * c - 1.0)][l]


BAND_OF = [0, 1, 1, 1, 2, 2, 2, 2, 2]


# ------------------------------------------------------------------------------------------------------------------------ the quality case
# the HW11 room of tests/shoot_gi_sets.py (48 x 32, 16 buckets), gi_sample_size 2, depth 2.  The volume stands inside
# the room (x -3 .. 3, y -1.5 .. 2.5, z -8 .. 1), its spacing about a third of it, no probe in a sphere.
QUALITY = dict(depth=2, samples=2, truth_rays_per_pixel=128, seed=9)
QUALITY_VOLUME = dict(origin=(-2.0, -0.9, -6.5), spacing=(2.0, 1.3, 2.5), nx=3, ny=3, nz=3, rays=256, gi_seed=11, backface_limit=1.0)


def quality_answers(scenes, oracle):
    """what the oracle answers for the quality case (tests/golden/make_probe_lit.py records it): the GI frame at many rays per pixel
    ("truth") and at one, the camera's centre rays' first hits, their S = 0 GI colours at the case's depth (a diffuse hit's direct light),
    and the depth - 1 GI colours of the volume's rays"""
    import shoot_gi_sets as gs
    import shoot_sets as sh
    q = QUALITY
    o = gs.oracle_of(scenes, oracle, "hw11")
    scene = gs.scene_of(scenes, "hw11")
    opt = lambda **kw: oracle.make_options(q["depth"], use_gi=1, **kw)  # noqa: E731
    truth, _ = o.render(options=opt(gi_sample_size=q["samples"], rays_per_pixel=q["truth_rays_per_pixel"], gi_seed=q["seed"]))
    one, _ = o.render(options=opt(gi_sample_size=q["samples"], rays_per_pixel=1, gi_seed=q["seed"]))
    rays = sh.normalized_rays(gs.camera_rays(o))
    n = len(rays)
    point, normal, diffuse = np.zeros((n, 3), dtype=F32), np.zeros((n, 3), dtype=F32), np.zeros(n, dtype=bool)
    for i, r in enumerate(rays):
        hit, h = o.trace(r[:3], r[3:], 0)
        if hit:
            point[i], normal[i] = h[1:4], h[4:7]
            diffuse[i] = scene["materials"][scene["objects"][int(h[9])]["material_index"]]["type"] == "diffuse"
    direct = o.shoot_gi(rays, gs.pixel_keys(oracle, q["seed"], n), 0, opt(gi_sample_size=0, gi_seed=q["seed"]))
    v = ps.Volume(**QUALITY_VOLUME)
    prays, pkeys = ps.rays_and_keys(v, 0, v.count)
    pcol = o.shoot_gi(prays, pkeys, 2, oracle.make_options(q["depth"] - 1, use_gi=1, gi_sample_size=q["samples"]))
    return dict(truth=truth.reshape(n, 3).copy(), one=one.reshape(n, 3).copy(), point=point, normal=normal, diffuse=diffuse, direct=direct,
                probe_colours=pcol)


def quality_rmse(a):
    """-> (RMSE of the probe-lit frame, of the same frame with Lbar = 0, of the one-ray-per-pixel GI frame), against the truth, over the
    pixels whose first hit is diffuse; the volume is the restatement's projection of the recorded probe colours"""
    v = ps.Volume(**QUALITY_VOLUME)
    prays, _ = ps.rays_and_keys(v, 0, v.count)
    rec = ps.project(prays, a["probe_colours"], v.count, v.rays)
    m = np.asarray(a["diffuse"], dtype=bool)
    S = QUALITY["samples"]
    lb, status = lbar(v, None, rec, None, a["point"][m], a["normal"][m])
    assert (status > 0).all()
    lit = combine(a["direct"][m], lb, S).astype(np.float64)
    dark = combine(a["direct"][m], np.zeros_like(lb), S).astype(np.float64)
    truth = a["truth"][m].astype(np.float64)
    rmse = lambda x: float(np.sqrt(np.mean((x - truth) ** 2)))  # noqa: E731
    return rmse(lit), rmse(dark), rmse(a["one"][m].astype(np.float64))
