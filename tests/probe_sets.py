"""What the tests of the irradiance probe volume (crt_probe_rays_device, crt_probe_project_device, crt_probe_validity_device,
crt_probe_irradiance_device, crt_bake_probes) share: the rule of include/crt_hip.h ("Irradiance probes"; csrc/probe_rule.h) restated in numpy
-- every line one float32 operation, in the header's order, so a float32 numpy expression rounds it as the -ffp-contract=off build rounds it
--, and the small cases it runs on.  numpy only, no GPU.  Sine and cosine are this machine's libm sinf / cosf, which csrc/glibc_sincosf.h
equals on [0, 2 pi] (tests/test_gi.py)."""
import ctypes as C
import ctypes.util

import numpy as np

import bake_sets as bs

F32 = np.float32
U32 = np.uint32
INVALID, VALID = 0, 1
PROBE_DTYPE = np.dtype([("coef", F32, (9, 3)), ("rays", U32), ("back", U32), ("miss", U32), ("state", U32), ("pad", U32)])
RAY_COUNTS = [1, 63, 64, 65, 100]            # below, at and above a wave's 64 lanes
BAND = np.array([1.0, 0.6666667, 0.6666667, 0.6666667, 0.25, 0.25, 0.25, 0.25, 0.25], dtype=F32)
SCENE_PARAMS = {k: v for k, v in bs.SCENE_PARAMS.items() if k != "bitmap_size"}
# the pinned volume: 2 x 2 x 2 probes of 64 rays in the HW11-like room, none inside a sphere
PIN_VOLUME = dict(origin=(-2.0, -0.9, -6.5), spacing=(4.0, 2.0, 4.0), nx=2, ny=2, nz=2, rays=64, gi_seed=0, backface_limit=1.0)
# the validity case: 3 x 1 x 1 probes, the middle one inside a closed box
BOX = ((-0.4, -0.4, -3.4), (0.4, 0.4, -2.6))
BOX_VOLUME = dict(origin=(-1.5, 0.0, -3.0), spacing=(1.5, 1.0, 1.0), nx=3, ny=1, nz=1, rays=64, gi_seed=0, backface_limit=0.25)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.argtypes = _libm.cosf.argtypes = [C.c_float]
_libm.sinf.restype = _libm.cosf.restype = C.c_float


class Volume:
    """crt_probe_volume as the restatement reads it"""

    def __init__(self, origin=(0, 0, 0), spacing=(1, 1, 1), nx=1, ny=1, nz=1, rays=64, gi_seed=0, backface_limit=1.0):
        self.origin = np.array(origin, dtype=F32)
        self.spacing = np.array(spacing, dtype=F32)
        self.n = (int(nx), int(ny), int(nz))
        self.rays, self.gi_seed, self.backface_limit = int(rays), int(gi_seed), F32(backface_limit)

    @property
    def count(self):
        return self.n[0] * self.n[1] * self.n[2]

    def fields(self):
        return dict(origin=[float(x) for x in self.origin], spacing=[float(x) for x in self.spacing], nx=self.n[0], ny=self.n[1], nz=self.n[2],
                    rays=self.rays, gi_seed=self.gi_seed, backface_limit=float(self.backface_limit))


def room(scenes):
    return scenes.make("hw11", **SCENE_PARAMS)


def box_room(scenes):
    """the room with a closed diffuse box, outward-facing, six quads"""
    scene = room(scenes)
    scene["materials"].append({"type": "diffuse", "albedo": [0.6, 0.6, 0.2], "smooth_shading": False})
    m = len(scene["materials"]) - 1
    (x0, y0, z0), (x1, y1, z1) = BOX
    q = scenes.quad
    faces = [q(m, (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)), q(m, (x1, y0, z0), (x0, y0, z0), (x0, y1, z0), (x1, y1, z0)),
             q(m, (x1, y0, z1), (x1, y0, z0), (x1, y1, z0), (x1, y1, z1)), q(m, (x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)),
             q(m, (x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0)), q(m, (x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1))]
    for f in faces:
        f.pop("uvs", None)
    scene["objects"] += faces
    return scene


# ------------------------------------------------------------------------------------------------------------------------ the rule
def positions(v, p):
    """float32 [len(p), 3]: where the probes p stand"""
    p = np.asarray(p, dtype=np.int64)
    ix, rest = p % v.n[0], p // v.n[0]
    i = np.stack([ix, rest % v.n[1], rest // v.n[1]], axis=1).astype(F32)
    step = i * v.spacing[None, :]
    return v.origin[None, :] + step


def directions(R):
    """float32 [R, 3]: the spherical Fibonacci set"""
    j = np.arange(R, dtype=np.int64)
    q = (2 * j + 1).astype(F32) / F32(R)
    z = F32(1.0) - q
    zz = z * z
    m = F32(1.0) - zz
    r = np.sqrt(np.where(m > 0, m, F32(0.0)).astype(F32))
    t = j.astype(F32) * F32(0.618034)
    t = t - t.astype(np.int32).astype(F32)
    phi = t * F32(6.2831855)
    cos = np.array([_libm.cosf(float(a)) for a in phi], dtype=F32)
    sin = np.array([_libm.sinf(float(a)) for a in phi], dtype=F32)
    return np.stack([r * cos, r * sin, z], axis=1).astype(F32)


def rays_and_keys(v, first, count):
    """the rays float32 [count * R, 6] and keys uint32 [count * R] of the probes [first, first + count)"""
    p = np.arange(first, first + count)
    pos = positions(v, p)
    d = directions(v.rays)
    rays = np.concatenate([np.repeat(pos, v.rays, axis=0), np.tile(d, (count, 1))], axis=1).astype(F32)
    pp = np.repeat(p, v.rays).astype(U32)
    jj = np.tile(np.arange(v.rays), count).astype(U32)
    keys = bs.gi_mix(bs.gi_mix(np.full(len(pp), v.gi_seed, dtype=U32), pp), jj)
    return rays, keys


def basis(d):
    """float32 [..., 9] of directions [..., 3]"""
    d = np.asarray(d, dtype=F32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        xy, yz, xz, xx, yy, zz = x * y, y * z, x * z, x * x, y * y, z * z
        z3 = F32(3.0) * zz
        zm = z3 - F32(1.0)
        xmy = xx - yy
        return np.stack([np.full(x.shape, F32(0.282095)), F32(0.488603) * y, F32(0.488603) * z, F32(0.488603) * x, F32(1.092548) * xy,
                         F32(1.092548) * yz, F32(0.315392) * zm, F32(1.092548) * xz, F32(0.546274) * xmy], axis=-1).astype(F32)


def project(rays, rgb, count, R):
    """the records PROBE_DTYPE [count] of rays float32 [count * R, 6] and colours float32 [count * R, 3]"""
    d = np.asarray(rays, dtype=F32).reshape(count, R, 6)[:, :, 3:]
    L = np.asarray(rgb, dtype=F32).reshape(count, R, 3)
    turns = (R + 63) // 64
    with np.errstate(all="ignore"):
        terms = L[:, :, None, :] * basis(d)[:, :, :, None]                       # [count, R, 9, 3]
        padded = np.zeros((count, turns * 64, 9, 3), dtype=F32)
        padded[:, :R] = terms
        padded = padded.reshape(count, turns, 64, 9, 3)
        live = (np.arange(turns * 64) < R).reshape(turns, 64)
        part = np.zeros((count, 64, 9, 3), dtype=F32)
        for k in range(turns):
            part = np.where(live[k][None, :, None, None], part + padded[:, k], part)
        for step in (32, 16, 8, 4, 2, 1):
            part[:, :step] = part[:, :step] + part[:, step:2 * step]
        coef = part[:, 0] * (F32(12.566371) / F32(R))
    rec = np.zeros(count, dtype=PROBE_DTYPE)
    rec["coef"] = coef
    rec["rays"] = R
    rec["state"] = VALID
    return rec


def state_of(back, R, limit):
    return INVALID if F32(back) > F32(limit) * F32(R) else VALID


def validity(rec, rays, hit, normals, R, limit):
    """rec with back, miss and state of the hits: hit bool [count * R], normals float32 [count * R, 3]"""
    rec = rec.copy()
    count = len(rec)
    d = np.asarray(rays, dtype=F32)[:, 3:]
    n = np.asarray(normals, dtype=F32)
    with np.errstate(all="ignore"):
        dot = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    hit = np.asarray(hit, dtype=bool)
    back = (hit & (dot > 0)).reshape(count, R).sum(axis=1)
    miss = (~hit).reshape(count, R).sum(axis=1)
    rec["back"], rec["miss"] = back, miss
    rec["state"] = [state_of(b, R, limit) for b in back]
    return rec


def axis(x, origin, spacing, n):
    """-> (i0, [w0, w1], corners) for one finite coordinate"""
    with np.errstate(all="ignore"):
        g = (F32(x) - origin) / spacing
    hi = F32(n - 1)
    g = F32(0.0) if g < 0 else (hi if g > hi else g)
    if n == 1:
        return 0, [F32(1.0), F32(0.0)], 1
    i = min(int(g), n - 2)
    f = g - F32(i)
    return i, [F32(1.0) - f, f], 2


def lookup(v, rec, points, normals, float64=False):
    """-> (rgb float32 [n, 3], status uint8 [n]); float64: the same rule evaluated in binary64 on the same records (-> float64 colours)"""
    T = np.float64 if float64 else F32
    rec = np.asarray(rec).reshape(-1)
    points, normals = np.asarray(points, dtype=F32), np.asarray(normals, dtype=F32)
    out = np.zeros((len(points), 3), dtype=T)
    status = np.zeros(len(points), dtype=np.uint8)
    band = BAND.astype(T)
    for i, (x, n) in enumerate(zip(points, normals)):
        if not (np.isfinite(x).all() and np.isfinite(n).all()):
            continue
        ax = [axis(x[k], v.origin[k], v.spacing[k], v.n[k]) for k in range(3)]
        W, S, used = T(0.0), np.zeros((9, 3), dtype=T), 0
        with np.errstate(all="ignore"):
            for dz in range(ax[2][2]):
                for dy in range(ax[1][2]):
                    for dx in range(ax[0][2]):
                        w = (T(ax[0][1][dx]) * T(ax[1][1][dy])) * T(ax[2][1][dz])
                        if w == 0:
                            continue
                        p = ((ax[2][0] + dz) * v.n[1] + (ax[1][0] + dy)) * v.n[0] + (ax[0][0] + dx)
                        if p >= len(rec) or rec["state"][p] != VALID:
                            continue
                        W = W + w
                        S = S + w * rec["coef"][p].astype(T)
                        used += 1
            if not used:
                continue
            Y = basis(n).astype(T) if not float64 else basis64(n)
            e = np.zeros(3, dtype=T)
            for c in range(9):
                e = e + (band[c] * Y[c]) * S[c]
            q = e / W
            out[i] = np.where(q > 0, q, T(0.0))
        status[i] = used
    return out, status


def basis64(d):
    x, y, z = (np.float64(a) for a in d)
    return np.array([0.282095, 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * (x * y), 1.092548 * (y * z), 0.315392 * (3.0 * (z * z) - 1.0),
                     1.092548 * (x * z), 0.546274 * (x * x - y * y)], dtype=np.float64)


def project64(d, L):
    """coefficients float64 [9, 3] of one probe: the rule in binary64 on the float32 directions d [R, 3] and colours L [R, 3]"""
    Y = np.array([basis64(a) for a in d])
    return (Y[:, :, None] * np.asarray(L, dtype=np.float64)[:, None, :]).sum(axis=0) * (4.0 * np.pi / len(d))


def same_records(got, want, what):
    """every field bit for bit; two NaNs count as the same coefficient"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    g, w = np.ascontiguousarray(got["coef"]), np.ascontiguousarray(want["coef"])
    same = (g.view(U32) == w.view(U32)) | (np.isnan(g) & np.isnan(w))
    assert same.all(), "%s: %d coefficients differ, first at %s: got %r want %r" % (what, int((~same).sum()), np.argwhere(~same)[0].tolist(),
                                                                                  g[tuple(np.argwhere(~same)[0])], w[tuple(np.argwhere(~same)[0])])
    for field in ("rays", "back", "miss", "state", "pad"):
        assert np.array_equal(got[field], want[field]), "%s: %s: got %r want %r" % (what, field, got[field][:8], want[field][:8])


def same_colours(got, want, what):
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    same = (got.view(U32) == want.view(U32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ" % (what, int((~same).sum()), same.size)


def special_colours(rng, n):
    """random colours float32 [n, 3] with negative zeros, infinities and NaNs among them (where n allows)"""
    c = rng.uniform(-1, 3, (n, 3)).astype(F32)
    flat = c.reshape(-1)
    for k, value in enumerate([-0.0, np.inf, -np.inf, np.nan, 0.0]):
        if 7 * k + 2 < len(flat) and n > 8:
            flat[7 * k + 2] = value
    return c


# ------------------------------------------------------------------------------------------------------------------------ the oracle
def oracle_shoot(o, rays, max_depth=5):
    return bs.oracle_shoot(o, rays, max_depth)


def oracle_hits(o, rays):
    """OracleScene.trace of every ray as a REFLECTION ray -> (hit bool [n], normals float32 [n, 3])"""
    hit = np.zeros(len(rays), dtype=bool)
    normals = np.zeros((len(rays), 3), dtype=F32)
    for i, r in enumerate(rays):
        h, rec = o.trace(r[:3], r[3:], 2)
        hit[i] = h
        normals[i] = rec[4:7] if h else 0
    return hit, normals


def brute_force(d, L, n):
    """float64 [3]: (4 / R) * sum_j L_j max(0, n . d_j)"""
    cos = np.maximum(np.asarray(d, dtype=np.float64) @ np.asarray(n, dtype=np.float64), 0.0)
    return (np.asarray(L, dtype=np.float64) * cos[:, None]).sum(axis=0) * (4.0 / len(d))
