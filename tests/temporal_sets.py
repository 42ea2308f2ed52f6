"""What the tests of the temporal accumulation (crt_temporal_device, crt_render_accumulated) share: the rule of include/crt_hip.h ("Temporal
accumulation") restated in numpy float32 -- one operation and one astype at a time, so that every intermediate is rounded to float32 once, as
the -ffp-contract=off build of csrc/temporal_rule.h rounds it --, and a synthetic set to run it on: a previous pose, a previous history and
current hits whose world points are made by un-projecting chosen previous-pixel coordinates in float64 and rounding once."""
import numpy as np

import denoise_sets as dns

F = np.float32
MISS = dns.MISS
HIT_DTYPE = dns.HIT_DTYPE
# crt_history_pixel (64 bytes), as the package's HISTORY_DTYPE has it
HISTORY_DTYPE = np.dtype([("n", np.float32, 3), ("t", np.float32), ("x", np.float32, 3), ("mesh", np.uint32), ("c", np.float32, 3),
                          ("m2", np.float32), ("weight", np.float32), ("pad", np.float32, 3)])
DEFAULTS = (64.0, 0.9, 0.02)
# max_history, normal_min, sigma_plane
SETTINGS = [DEFAULTS, (2.5, 0.5, 0.0), (1e-3, -1.0, 10.0), (3e38, 0.999, 0.005)]
SHAPES = [(37, 29), (1, 1), (5, 1), (1, 7), (64, 3), (33, 9)]   # (the last crosses a 32x8 tile edge on both axes)
ROUTES = ("fx_integral", "fx_half", "fx_negative", "fx_beyond", "fy_integral", "fy_half", "fy_negative", "fy_beyond", "behind", "nan_point", "inf_t",
          "miss", "outside", "weight0", "nonfinite", "mesh", "normal", "plane", "count0", "clamped", "no_valid", "all_valid")


def settings(temporal):
    """(max_history, normal_min, sigma_plane) of a crt_temporal or of a tuple"""
    if isinstance(temporal, tuple):
        return temporal
    return (float(temporal.max_history), float(temporal.normal_min), float(temporal.sigma_plane))


def project(points, pose, width, height):
    """the rule's `reproject` lines up to fx, fy: points float32 [P, 3] -> (depth, fx, fy), float32 [P] each"""
    o, m = np.asarray(pose[0], dtype=F).reshape(3), np.asarray(pose[1], dtype=F).reshape(9)
    with np.errstate(all="ignore"):
        w = [(points[:, j] - o[j]).astype(F) for j in range(3)]
        v = []
        for i in range(3):
            a = (w[0] * m[3 * i]).astype(F)
            b = (w[1] * m[3 * i + 1]).astype(F)
            c = (w[2] * m[3 * i + 2]).astype(F)
            ab = (a + b).astype(F)
            v.append((ab + c).astype(F))
        depth = (F(0.0) - v[2]).astype(F)
        sx = (v[0] / depth).astype(F)
        sy = (v[1] / depth).astype(F)
        fw, fh = F(width), F(height)
        aspect = F(fw / fh)
        sx = (sx / aspect).astype(F)
        ux = (sx + F(1.0)).astype(F)
        uy = (F(1.0) - sy).astype(F)
        hx = (ux * F(0.5)).astype(F)
        hy = (uy * F(0.5)).astype(F)
        px = (hx * fw).astype(F)
        py = (hy * fh).astype(F)
        fx = (px - F(0.5)).astype(F)
        fy = (py - F(0.5)).astype(F)
    return depth, fx, fy


def frame(temporal, width, height, pose, prev, total, sq, counts, hits, tally=None):
    """One frame of the rule.  pose: (position [3], matrix [9]) of the previous frame, prev: its HISTORY_DTYPE records [H * W], or None and None;
    total float32 [P, 3], sq float32 [P], counts uint32 [P], hits crt_hit records [P] -> (records HISTORY_DTYPE [P], colour float32 [P, 3],
    V float32 [P], valid uint8 [P]).  tally: a dict that receives how often each route of ROUTES was taken."""
    max_history, normal_min, sigma_plane = (F(v) for v in settings(temporal))
    n = width * height
    total, sq, counts = np.asarray(total, dtype=F).reshape(n, 3), np.asarray(sq, dtype=F).reshape(n), np.asarray(counts).reshape(n)
    hits = np.asarray(hits).reshape(n)
    n_p, x_p, t_p = np.ascontiguousarray(hits["normal"]), np.ascontiguousarray(hits["point"]), np.ascontiguousarray(hits["t"])
    mesh_p = np.where(hits["hit"] != 0, hits["mesh"], MISS).astype(np.uint32)
    count = dict.fromkeys(ROUTES, 0)
    with np.errstate(all="ignore"):
        # current
        n_c = counts.astype(F)
        inv = (F(1.0) / np.maximum(counts, 1).astype(F)).astype(F)
        c_c = np.stack([(total[:, k] * inv).astype(F) for k in range(3)], axis=1)
        q_c = (sq * inv).astype(F)
        c_c[counts == 0] = F(0.0)
        q_c[counts == 0] = F(0.0)
        count["count0"] = int((counts == 0).sum())
        # reproject
        c_h, q_h, n_h = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F)
        valid = np.zeros(n, np.uint32)
        count["miss"] = int((mesh_p == MISS).sum())
        if prev is not None:
            prev = np.asarray(prev).reshape(n)
            live = mesh_p != MISS
            count["nan_point"] = int((live & np.isnan(x_p).any(axis=1)).sum())
            count["inf_t"] = int((live & np.isinf(t_p)).sum())
            depth, fx, fy = project(x_p, pose, width, height)
            front = depth > F(0.0)
            count["behind"] = int((live & (depth <= F(0.0))).sum())
            live = live & front
            fw, fh = F(width), F(height)
            for name, f, size in (("fx", fx, fw), ("fy", fy, fh)):
                count[name + "_integral"] += int((live & (f == np.floor(f)) & (f >= 0) & (f < size)).sum())
                count[name + "_half"] += int((live & ((f - np.floor(f)).astype(F) == F(0.5)) & (f > 0) & (f < size)).sum())
                count[name + "_negative"] += int((live & (f > F(-1.0)) & (f < F(0.0))).sum())
                count[name + "_beyond"] += int((live & (f >= size)).sum())
            live = live & (fx > F(-1.0)) & (fx < fw) & (fy > F(-1.0)) & (fy < fh)
            x0, y0 = np.floor(fx).astype(F), np.floor(fy).astype(F)
            ax, ay = (fx - x0).astype(F), (fy - y0).astype(F)
            bx, by = (F(1.0) - ax).astype(F), (F(1.0) - ay).astype(F)
            ix, iy = np.where(live, x0, 0).astype(np.int64), np.where(live, y0, 0).astype(np.int64)
            tol = (sigma_plane * t_p).astype(F)
            weights = [(by * bx).astype(F), (by * ax).astype(F), (ay * bx).astype(F), (ay * ax).astype(F)]
            acc, accq, accn, wsum = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
            for k in range(4):
                qx, qy = ix + (k & 1), iy + (k >> 1)
                inside = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
                count["outside"] += int((live & ~inside).sum())
                take = live & inside
                q = prev[np.clip(qy, 0, height - 1) * width + np.clip(qx, 0, width - 1)]
                w_q, c_q, m2_q = q["weight"], q["c"], q["m2"]
                heavy = w_q > F(0.0)
                count["weight0"] += int((take & ~heavy).sum())
                take = take & heavy
                good = dns.usable(c_q, m2_q, w_q)                 # heavy and all finite
                count["nonfinite"] += int((take & ~good).sum())
                take = take & good
                count["mesh"] += int((take & (q["mesh"] != mesh_p)).sum())
                take = take & (q["mesh"] == mesh_p)
                d = dns.normal_dot(n_p, q["n"])
                facing = d >= normal_min
                count["normal"] += int((take & ~facing).sum())
                take = take & facing
                near = dns.plane_distance(n_p, x_p, q["x"]) <= tol
                count["plane"] += int((take & ~near).sum())
                take = take & near
                b = weights[k]
                wsum = np.where(take, (wsum + b).astype(F), wsum)
                for c in range(3):
                    bc = (b * c_q[:, c]).astype(F)
                    acc[:, c] = np.where(take, (acc[:, c] + bc).astype(F), acc[:, c])
                bq = (b * m2_q).astype(F)
                accq = np.where(take, (accq + bq).astype(F), accq)
                bn = (b * w_q).astype(F)
                accn = np.where(take, (accn + bn).astype(F), accn)
                valid = valid + take.astype(np.uint32)
            some = wsum > F(0.0)
            inv = (F(1.0) / wsum).astype(F)
            c_h = np.where(some[:, None], (acc * inv[:, None]).astype(F), F(0.0)).astype(F)
            q_h = np.where(some, (accq * inv).astype(F), F(0.0)).astype(F)
            n_h = np.where(some, (accn * inv).astype(F), F(0.0)).astype(F)
            count["no_valid"] = int((live & (valid == 0)).sum())
            count["all_valid"] = int((valid == 4).sum())
        # merge
        count["clamped"] = int((~(n_h < max_history)).sum())
        n_h = np.where(n_h < max_history, n_h, max_history).astype(F)
        merged = ~(n_h == F(0.0))
        n_m = (n_h + n_c).astype(F)
        inv = (F(1.0) / n_m).astype(F)
        a_h, a_c = (n_h * inv).astype(F), (n_c * inv).astype(F)
        c_m = np.zeros((n, 3), F)
        for c in range(3):
            h = (a_h * c_h[:, c]).astype(F)
            u = (a_c * c_c[:, c]).astype(F)
            c_m[:, c] = (h + u).astype(F)
        h = (a_h * q_h).astype(F)
        u = (a_c * q_c).astype(F)
        q_m = (h + u).astype(F)
        colour = np.where(merged[:, None], c_m, c_c).astype(F)
        q = np.where(merged, q_m, q_c).astype(F)
        weight = np.where(merged, n_m, n_c).astype(F)
        none = weight == F(0.0)
        colour[none] = F(0.0)
        q[none] = F(0.0)
        v = dns.variance_of_mean(colour, q, weight)
        v[none] = F(0.0)
    records = np.zeros(n, dtype=HISTORY_DTYPE)
    records["n"], records["t"], records["x"], records["mesh"] = n_p, t_p, x_p, mesh_p
    records["c"], records["m2"], records["weight"] = colour, q, weight
    if tally is not None:
        for k in ROUTES:
            tally[k] = tally.get(k, 0) + count[k]
    return records, colour, v, valid.astype(np.uint8)


def same_records(got, want, what):
    """two HISTORY_DTYPE arrays, field by field, bit for bit (a NaN is a NaN)"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    for name in HISTORY_DTYPE.names:
        dns.same(np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]), "%s: records' %s" % (what, name))


def rotation(pan_degrees, tilt_degrees):
    """a product of two rotations, row-major float64 [3, 3]: about y, then about x"""
    a, b = np.radians(pan_degrees), np.radians(tilt_degrees)
    ry = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return ry @ rx


def unproject(fx, fy, depth, pose, width, height):
    """float64: the world point that the pose's camera sees at pixel coordinates (fx, fy) (a pixel's centre is its integer coordinates) at
    camera-space depth `depth` -- getRay's arithmetic, with the rule's v = M w inverted by the transpose"""
    o, m = np.asarray(pose[0], dtype=np.float64), np.asarray(pose[1], dtype=np.float64).reshape(3, 3)
    aspect = np.float64(F(F(width) / F(height)))
    sx = ((fx + 0.5) / width * 2.0 - 1.0) * aspect
    sy = 1.0 - (fy + 0.5) / height * 2.0
    v = np.stack([sx * depth, sy * depth, -depth * np.ones_like(sx)], axis=-1)
    return o + v @ m        # w = M^T v: row vector x matrix, as getRay's


def plane_depth(fx, width, height):
    """the set's geometry: the plane z = -(5 + 0.05 x) of the previous camera's space (normal (0.05, 0, 1)), as the depth along the ray
    through pixel coordinate fx"""
    sx = ((fx + 0.5) / width * 2.0 - 1.0) * np.float64(F(F(width) / F(height)))
    return 5.0 / (1.0 - 0.05 * sx)


def exact(point, pose, width, height, axis, want, fraction):
    """a float32 point a few ulps from `point` whose projected coordinate on `axis` (0: fx, 1: fy) has exactly the fraction `fraction` at
    floor `want`; `point` itself when none of the candidates has"""
    cand = np.repeat(np.asarray(point, dtype=F).reshape(1, 3), 3 * 4001, axis=0)
    for j in range(3):      # (neighbouring bit patterns are neighbouring floats while the sign holds)
        bits = cand[j * 4001:(j + 1) * 4001, j].view(np.int32)
        if abs(int(bits[0])) > 4000:
            bits += np.arange(-2000, 2001, dtype=np.int32)
    f = project(cand, pose, width, height)[1 + axis]
    good = np.flatnonzero((np.floor(f) == F(want)) & ((f - np.floor(f)).astype(F) == F(fraction)))
    return cand[good[0]] if len(good) else np.asarray(point, dtype=F)


_sets = {}


def synthetic(width, height, seed=9):
    """-> dict(pose (position [3], matrix [9]), prev HISTORY_DTYPE [P], total, sq, counts, hits), made once per shape and read-only.
    The previous frame saw a slanted plane carrying three meshes side by side (and miss pixels); the current hits lie on that plane at
    chosen previous-pixel coordinates -- the pixel's own plus (1.37, -0.62), and the special ones the routes need."""
    if (width, height, seed) in _sets:
        return _sets[(width, height, seed)]
    rng = np.random.default_rng(seed)
    n = width * height
    ys, xs = np.divmod(np.arange(n), width)
    r = rotation(10.0, -5.0)
    pose = (np.array([0.3, -0.2, 1.0], dtype=F), r.astype(F).reshape(9))
    normal = (np.array([0.05, 0.0, 1.0]) / np.sqrt(1.0025)) @ pose[1].astype(np.float64).reshape(3, 3)   # the plane's normal, to the world
    region = lambda fx: np.clip((3 * np.floor(fx + 0.5)) // max(width, 1), 0, 2).astype(np.uint32)
    # the previous history: the plane at every pixel centre
    prev = np.zeros(n, dtype=HISTORY_DTYPE)
    centre = unproject(xs.astype(np.float64), ys.astype(np.float64), plane_depth(xs.astype(np.float64), width, height), pose, width, height)
    prev["x"], prev["n"] = centre.astype(F), normal.astype(F)
    prev["t"] = np.linalg.norm(centre - pose[0].astype(np.float64), axis=1).astype(F)
    prev["mesh"] = region(xs.astype(np.float64))
    prev["c"] = (rng.random((n, 3), dtype=F) * F(0.8)).astype(F)
    prev["m2"] = ((prev["c"] * prev["c"]).sum(axis=1) + rng.random(n, dtype=F) * F(0.2)).astype(F)
    prev["weight"] = rng.choice(np.array([1.0, 4.0, 7.5, 32.0, 100.0], dtype=F), n)
    prev_miss = (xs * 7 + ys * 5) % 23 == 0
    for name in ("x", "n", "t"):
        prev[name][prev_miss] = 0
    prev["mesh"][prev_miss] = MISS
    prev["weight"][rng.random(n) < 0.05] = 0.0
    prev["weight"][rng.random(n) < 0.01] = -2.0
    special = np.array([np.inf, -np.inf, np.nan], dtype=F)
    pick = rng.random(n) < 0.03
    prev["c"][pick, rng.integers(0, 3, int(pick.sum()))] = rng.choice(special, int(pick.sum()))
    pick = rng.random(n) < 0.02
    prev["m2"][pick] = rng.choice(special, int(pick.sum()))
    pick = rng.random(n) < 0.01
    prev["weight"][pick] = np.inf
    # the current hits
    fx, fy = xs + 1.37, ys - 0.62
    kind = rng.integers(0, 40, n)
    kind[:min(n, 16)] = np.arange(16)[:min(n, 16)]        # (the small shapes have the first kinds by position)
    fx = np.where(kind == 4, -0.4, np.where(kind == 5, width + 0.3, np.where(kind == 6, float(width), fx)))
    fy = np.where(kind == 7, -0.7, np.where(kind == 8, height + 1.5, np.where(kind == 9, float(height), fy)))
    depth = plane_depth(fx, width, height)
    depth = np.where(kind == 10, -depth, depth)          # behind the camera
    points = unproject(fx, fy, depth, pose, width, height)
    points = np.where((kind == 11)[:, None], points + 0.8 * normal, points)      # off the plane
    hits = np.zeros(n, dtype=HIT_DTYPE)
    hits["point"], hits["normal"] = points.astype(F), normal.astype(F)
    for i in np.flatnonzero(kind < 4):                   # fx, fy exactly integral and exactly half-way
        axis, fraction = int(kind[i]) & 1, 0.5 * (int(kind[i]) >> 1)
        target = (min(int(xs[i]) + 1, width - 1), max(int(ys[i]) - 1, 0))
        coords = [target[0] + (fraction if axis == 0 else 0.37), target[1] + (fraction if axis == 1 else 0.41)]
        p = unproject(np.float64(coords[0]), np.float64(coords[1]), plane_depth(coords[0], width, height), pose, width, height)
        hits["point"][i] = exact(p.astype(F), pose, width, height, axis, target[axis], fraction)
        fx[i] = coords[0]
    tilted = (np.array([0.7, 0.0, 0.714]) / np.linalg.norm([0.7, 0.0, 0.714])) @ pose[1].astype(np.float64).reshape(3, 3)
    hits["normal"][kind == 12] = tilted.astype(F)
    hits["t"] = np.linalg.norm(hits["point"].astype(np.float64) - pose[0].astype(np.float64), axis=1).astype(F)
    hits["mesh"], hits["triangle"], hits["hit"] = region(fx), rng.integers(0, 50, n), 1
    hits["mesh"][kind == 13] = 7                           # a mesh the previous frame did not see
    hits["u"], hits["v"] = rng.random(n, dtype=F), rng.random(n, dtype=F)
    hits["point"][kind == 14, 1] = np.nan
    hits["t"][kind == 15] = np.inf
    hits[(kind == 16) | ((xs * 3 + ys * 11) % 17 == 0)] = np.zeros(1, dtype=HIT_DTYPE)   # hit == 0: every other field is 0
    state = dns.synthetic(width, height)                  # the fold's state: noisy colours of 0..8 samples, with the special values
    s = dict(pose=pose, prev=prev, total=state["total"], sq=state["sq"], counts=state["counts"], hits=hits)
    for a in (pose[0], pose[1], prev, s["total"], s["sq"], s["counts"], hits):
        a.setflags(write=False)
    _sets[(width, height, seed)] = s
    return s
