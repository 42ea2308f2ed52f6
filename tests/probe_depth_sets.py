"""What the tests of the probe volume's visibility term (crt_probe_depth_device, crt_probe_irradiance_visible_device, crt_bake_probes_visible)
share: the rule of include/crt_hip.h ("Probe visibility"; csrc/probe_depth_rule.h) restated in numpy -- every line one float32 operation, in the
header's order, so a float32 numpy expression rounds it as the -ffp-contract=off build rounds it --, a float64 variant of the lookup, and the
partition scene.  numpy only, no GPU.  The lookup's shared part is tests/probe_sets.py's."""
import numpy as np

import probe_sets as ps

F32, U32 = np.float32, np.uint32
SIDE, TEXELS = 8, 64
DEPTH_DTYPE = np.dtype([("moments", F32, (64, 2))])
SPECIAL_T = [0.0, -0.0, 1e-42, -1.0, np.inf, -np.inf, np.nan]      # a zero, a denormal, a negative, the non-finite ones


class Visibility:
    """crt_probe_visibility as the restatement reads it; the defaults are crt_probe_visibility_defaults'"""

    def __init__(self, volume, max_distance=None, normal_bias=None, variance_floor=None, min_weight=None):
        s = volume.spacing
        diag = np.sqrt(F32(F32(s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
        self.max_distance = F32(F32(1.5) * diag) if max_distance is None else F32(max_distance)
        self.normal_bias = F32(F32(0.02) * min(s)) if normal_bias is None else F32(normal_bias)
        self.variance_floor = F32(F32(1e-6) * F32(self.max_distance * self.max_distance)) if variance_floor is None else F32(variance_floor)
        self.min_weight = F32(0.01) if min_weight is None else F32(min_weight)

    def fields(self):
        return dict(max_distance=float(self.max_distance), normal_bias=float(self.normal_bias), variance_floor=float(self.variance_floor),
                    min_weight=float(self.min_weight))


# ------------------------------------------------------------------------------------------------------------------------ the rule
def sgn(v):
    return np.where(v >= 0, F32(1.0), F32(-1.0)).astype(F32)


def sum3(a, b):
    with np.errstate(all="ignore"):
        return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F32)


def texel_directions():
    """float32 [64, 3]: e_k"""
    k = np.arange(TEXELS)
    col, row = (k % SIDE).astype(F32), (k // SIDE).astype(F32)
    qx = ((col + F32(0.5)) / F32(8.0)) * F32(2.0) - F32(1.0)
    qy = ((row + F32(0.5)) / F32(8.0)) * F32(2.0) - F32(1.0)
    ax, ay = np.abs(qx), np.abs(qy)
    z = (F32(1.0) - ax) - ay
    x = np.where(z < 0, (F32(1.0) - ay) * sgn(qx), qx).astype(F32)
    y = np.where(z < 0, (F32(1.0) - ax) * sgn(qy), qy).astype(F32)
    d = np.stack([x, y, z], axis=1).astype(F32)
    length = np.sqrt(sum3(d, d))
    return (d / length[:, None]).astype(F32)


def distances(hit, t, max_distance):
    """float32 [n]: what every ray counts with"""
    t = np.asarray(t, dtype=F32)
    mx = F32(max_distance)
    with np.errstate(all="ignore"):
        r = np.where((np.asarray(hit) != 0) & (t < mx), t, mx).astype(F32)
        return np.where(r > 0, r, F32(0.0)).astype(F32)


def project(rays, hit, t, count, R, max_distance):
    """the depth records float32 [count, 64, 2] of rays float32 [count * R, 6], hit [count * R] and t float32 [count * R]"""
    d = np.asarray(rays, dtype=F32).reshape(count, R, 6)[:, :, 3:]
    r = distances(hit, t, max_distance).reshape(count, R)
    e = texel_directions()
    mx = F32(max_distance)
    W, S1, S2 = (np.zeros((count, TEXELS), dtype=F32) for _ in range(3))
    with np.errstate(all="ignore"):
        for j in range(R):
            dj = d[:, j, None, :]                                                   # [count, 1, 3]
            c = ((dj[..., 0] * e[None, :, 0] + dj[..., 1] * e[None, :, 1]) + dj[..., 2] * e[None, :, 2]).astype(F32)
            c = np.where(c > 0, c, F32(0.0)).astype(F32)
            w = c * c
            w = w * w
            w = w * w
            w = w * w
            rj = r[:, j, None]
            W = W + w
            S1 = S1 + w * rj
            S2 = S2 + w * (rj * rj)
        seen = W > 0
        safe = np.where(seen, W, F32(1.0))
        mean = np.where(seen, S1 / safe, mx)
        mean2 = np.where(seen, S2 / safe, mx * mx)
    return np.stack([mean, mean2], axis=2).astype(F32)


def tap_axis(p, T=F32):
    """-> (i int [-1, 7], f) of one octahedral coordinate"""
    with np.errstate(all="ignore"):
        g = (T(p) * T(0.5) + T(0.5)) * T(8.0) - T(0.5)
    g = g if g > T(-0.5) else T(-0.5)
    g = g if g < T(7.5) else T(7.5)
    i = int(g)
    if T(i) > g:
        i -= 1
    return i, g - T(i)


def wrap(tx, ty):
    if tx < 0:
        tx, ty = 0, 7 - ty
    elif tx > 7:
        tx, ty = 7, 7 - ty
    if ty < 0:
        ty, tx = 0, 7 - tx
    elif ty > 7:
        ty, tx = 7, 7 - tx
    return ty * SIDE + tx


def clamp_wrap(tx, ty):
    """NOT the rule: a wrap that clamps at the map's edge, for the test that must see a wrong wrap"""
    return min(max(ty, 0), 7) * SIDE + min(max(tx, 0), 7)


def taps(u, T=F32, wrap_fn=wrap):
    """-> ([k0..k3], [w0..w3]) of one direction"""
    u = [T(a) for a in u]
    with np.errstate(all="ignore"):
        s = (abs(u[0]) + abs(u[1])) + abs(u[2])
        px, py = u[0] / s, u[1] / s
        if u[2] < 0:
            fx, fy = T(1.0) - abs(py), T(1.0) - abs(px)
            px, py = fx * (T(1.0) if px >= 0 else T(-1.0)), fy * (T(1.0) if py >= 0 else T(-1.0))
        ix, fx = tap_axis(px, T)
        iy, fy = tap_axis(py, T)
        wx, wy = [T(1.0) - fx, fx], [T(1.0) - fy, fy]
        return [wrap_fn(ix + a, iy + b) for b in (0, 1) for a in (0, 1)], [wx[a] * wy[b] for b in (0, 1) for a in (0, 1)]


def tap(u, pairs, T=F32, wrap_fn=wrap):
    """the moments (m1, m2) of one direction in one map pairs [64, 2]"""
    k, w = taps(u, T, wrap_fn)
    m1, m2 = T(0.0), T(0.0)
    with np.errstate(all="ignore"):
        for kk, ww in zip(k, w):
            m1 = m1 + ww * T(pairs[kk][0])
            m2 = m2 + ww * T(pairs[kk][1])
    return m1, m2


def weight(vis, dist, m1, m2, T=F32):
    with np.errstate(all="ignore"):
        var = abs(m2 - m1 * m1)
        floor = T(vis.variance_floor)
        var = var if var > floor else floor
        ch = T(1.0)
        if not dist <= m1:
            e = dist - m1
            ch = var / (var + e * e)
            ch = (ch * ch) * ch
        low = T(vis.min_weight)
        return ch if ch > low else low


def lookup(v, vis, rec, depth, points, normals, float64=False, weights=None):
    """-> (rgb float32 [n, 3], status uint8 [n]); float64: the same rule in binary64 on the same records (-> float64 colours).
    weights: a list that takes every used corner's (point, probe, vis)"""
    T = np.float64 if float64 else F32
    rec = np.asarray(rec).reshape(-1)
    depth = np.asarray(depth, dtype=F32).reshape(-1, TEXELS, 2)
    points, normals = np.asarray(points, dtype=F32), np.asarray(normals, dtype=F32)
    out = np.zeros((len(points), 3), dtype=T)
    status = np.zeros(len(points), dtype=np.uint8)
    band = ps.BAND.astype(T)
    bias = T(vis.normal_bias)
    for i, (x, n) in enumerate(zip(points, normals)):
        if not (np.isfinite(x).all() and np.isfinite(n).all()):
            continue
        ax = [ps.axis(x[k], v.origin[k], v.spacing[k], v.n[k]) for k in range(3)]
        W, S, used = T(0.0), np.zeros((9, 3), dtype=T), 0
        with np.errstate(all="ignore"):
            for dz in range(ax[2][2]):
                for dy in range(ax[1][2]):
                    for dx in range(ax[0][2]):
                        wc = (T(ax[0][1][dx]) * T(ax[1][1][dy])) * T(ax[2][1][dz])
                        if wc == 0:
                            continue
                        p = ((ax[2][0] + dz) * v.n[1] + (ax[1][0] + dy)) * v.n[0] + (ax[0][0] + dx)
                        if p >= len(rec) or rec["state"][p] != ps.VALID:
                            continue
                        P = ps.positions(v, [p])[0].astype(T)
                        vv = (x.astype(T) + n.astype(T) * bias) - P
                        dist = np.sqrt((vv[0] * vv[0] + vv[1] * vv[1]) + vv[2] * vv[2])
                        visible = T(1.0)
                        if dist > 0:
                            m1, m2 = tap(vv / dist, depth[p], T)
                            visible = weight(vis, dist, m1, m2, T)
                        if weights is not None:
                            weights.append((i, p, float(visible)))
                        w = wc * visible
                        W = W + w
                        S = S + w * rec["coef"][p].astype(T)
                        used += 1
            if not used:
                continue
            Y = ps.basis(n).astype(T) if not float64 else ps.basis64(n)
            e = np.zeros(3, dtype=T)
            for c in range(9):
                e = e + (band[c] * Y[c]) * S[c]
            q = e / W
            out[i] = np.where(q > 0, q, T(0.0))
        status[i] = used
    return out, status


def same_depth(got, want, what):
    """bit for bit; two NaNs count as the same"""
    got, want = np.ascontiguousarray(got, dtype=F32).reshape(-1), np.ascontiguousarray(want, dtype=F32).reshape(-1)
    assert got.shape == want.shape, what
    same = (got.view(U32) == want.view(U32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%s: %d of %d floats differ, first at %d: got %r want %r" % (what, int((~same).sum()), same.size, int(np.argmax(~same)),
                                                                                  got[np.argmax(~same)], want[np.argmax(~same)])


def special_hits(rng, n, max_distance):
    """(hit uint32 [n], t float32 [n]): random distances around max_distance with misses, and the special distances among them"""
    t = rng.uniform(0.0, 1.6 * float(max_distance), n).astype(F32)
    hit = (rng.uniform(size=n) < 0.8).astype(U32)
    mx = F32(max_distance)
    for k, value in enumerate(SPECIAL_T + [mx, np.nextafter(mx, F32(np.inf)), np.nextafter(mx, F32(0.0))]):
        if 3 * k + 1 < n:
            t[3 * k + 1] = value
            hit[3 * k + 1] = 1
    return hit, t


# ------------------------------------------------------------------------------------------------------------------------ the partition scene
# tests/probe_sets.py's room (x in [-3, 3], y in [-1.5, 2.5], z in [-8, 1], open to the front) with a thin two-sided diffuse wall across it
# at x = PARTITION_X +- 0.01, between the two spheres, reaching half a unit beyond the floor, the ceiling, the back wall and the open front,
# and the lights of the x > PARTITION_X side only (one of the room's four).  The volume has one probe column on each side, 0.75 from the
# wall, no probe in a sphere or in the wall: its one cell straddles the wall.
PARTITION_X, PARTITION_HALF = 0.0, 0.01
PARTITION_VOLUME = dict(origin=(-0.75, -0.5, -3.0), spacing=(1.5, 1.5, 1.5), nx=2, ny=2, nz=2, rays=64, gi_seed=0, backface_limit=1.0)


def partition_room(scenes):
    scene = ps.room(scenes)
    lo = np.array([np.min([np.min(np.asarray(o["vertices"], dtype=np.float64).reshape(-1, 3), axis=0) for o in scene["objects"]], axis=0)]).reshape(3)
    hi = np.array([np.max([np.max(np.asarray(o["vertices"], dtype=np.float64).reshape(-1, 3), axis=0) for o in scene["objects"]], axis=0)]).reshape(3)
    scene["materials"].append({"type": "diffuse", "albedo": [0.7, 0.7, 0.7], "smooth_shading": False})
    m = len(scene["materials"]) - 1
    q = scenes.quad
    (y0, z0), (y1, z1) = (float(lo[1]) - 0.5, float(lo[2]) - 0.5), (float(hi[1]) + 0.5, float(hi[2]) + 0.5)
    xa, xb = PARTITION_X - PARTITION_HALF, PARTITION_X + PARTITION_HALF
    faces = [q(m, (xa, y0, z0), (xa, y0, z1), (xa, y1, z1), (xa, y1, z0)),          # faces -x
             q(m, (xb, y0, z1), (xb, y0, z0), (xb, y1, z0), (xb, y1, z1))]          # faces +x
    for f in faces:
        f.pop("uvs", None)
    scene["objects"] += faces
    scene["lights"] = [l for l in scene["lights"] if l["position"][0] > PARTITION_X + 0.25]
    return scene


def side_points(v, dark):
    """a fixed grid of points in the cells that straddle the partition, on the dark (x < PARTITION_X) or the lit side, with normals that
    face away from the partition"""
    xs = [PARTITION_X - s for s in (0.15, 0.3, 0.45)] if dark else [PARTITION_X + s for s in (0.15, 0.3, 0.45)]
    ys = [float(v.origin[1] + v.spacing[1] * f) for f in (0.25, 0.6)]
    zs = [float(v.origin[2] + v.spacing[2] * f) for f in (0.2, 0.5, 0.8)]
    pts = np.array([(x, y, z) for z in zs for y in ys for x in xs], dtype=F32)
    nrm = np.tile(np.array([(-1.0 if dark else 1.0, 0.0, 0.0)], dtype=F32), (len(pts), 1))
    return pts, nrm
