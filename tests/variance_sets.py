"""What the tests of the variance estimate (crt_variance_estimate_device, crt_set_variance_estimate) share: the rule of include/crt_hip.h
("Variance estimate") restated in numpy float32 -- one operation and one astype at a time, so that every intermediate is rounded to float32
once, as the -ffp-contract=off build of csrc/variance_rule.h rounds it --, and synthetic moment records, guides and variances to run it on."""
import numpy as np

import denoise_sets as dns
import temporal_sets as ts

F = np.float32
MISS = dns.MISS
HIT_DTYPE = dns.HIT_DTYPE
HISTORY_DTYPE = ts.HISTORY_DTYPE
RADIUS = 3
DEFAULTS = (4.0, 5, 0.02)
# min_history, normal_squarings, sigma_plane
SETTINGS = [DEFAULTS, (2.0, 0, 0.0), (1e30, 16, 10.0), (3.5, 2, 0.005)]
SHAPES = [(1, 1), (5, 3), (33, 9), (70, 20)]   # smaller than the window both ways; one past a 32x8 tile both ways; several tiles
PASS_ROUTES = ("centre_unusable", "centre_miss", "centre_long", "no_tap")
SKIP_ROUTES = ("outside", "unusable", "mesh", "plane")
ROUTES = PASS_ROUTES + SKIP_ROUTES + ("flagged", "estimated")


def settings(estimate):
    """(min_history, normal_squarings, sigma_plane) of a crt_variance_estimate or of a tuple"""
    if isinstance(estimate, tuple):
        return estimate
    return (float(estimate.min_history), int(estimate.normal_squarings), float(estimate.sigma_plane))


usable = dns.usable


def estimate(setting, width, height, records, hits, var, tally=None):
    """The rule on a width x height image: records HISTORY_DTYPE [P] (c, m2 and weight are read), hits crt_hit records [P] (the guides), var
    float32 [P] -> V' float32 [P].  tally: a dict that receives how many centres took each pass-through route and how many taps each skip
    route skipped (ROUTES)."""
    min_history, squarings, sigma_plane = settings(setting)
    min_history, sigma_plane = F(min_history), F(sigma_plane)
    records = np.asarray(records).reshape(height, width)
    c, m2, weight = np.ascontiguousarray(records["c"]), np.ascontiguousarray(records["m2"]), np.ascontiguousarray(records["weight"])
    guides = dns.guides_of(hits, height, width)
    n_p, x_p, t_p, mesh_p = guides["n"], guides["x"], guides["t"], guides["mesh"]
    v_in = np.asarray(var, dtype=F).reshape(height, width)
    count = dict.fromkeys(ROUTES, 0)
    with np.errstate(all="ignore"):
        good = usable(c, m2, weight)
        is_hit = mesh_p != MISS
        short = weight < min_history
        flagged = good & is_hit & short
        count["centre_unusable"] = int((~good).sum())
        count["centre_miss"] = int((good & ~is_hit).sum())
        count["centre_long"] = int((good & is_hit & ~short).sum())
        count["flagged"] = int(flagged.sum())
        tol = (sigma_plane * t_p).astype(F)
        acc = np.zeros((height, width, 3), F)
        accq, wsum = np.zeros((height, width), F), np.zeros((height, width), F)
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                inside, ys, xs = dns.tap(height, width, dy, dx)
                count["outside"] += int((flagged & ~inside).sum())
                take = flagged & inside
                count["unusable"] += int((take & ~good[ys, xs]).sum())
                take = take & good[ys, xs]
                count["mesh"] += int((take & (mesh_p[ys, xs] != mesh_p)).sum())
                take = take & (mesh_p[ys, xs] == mesh_p)
                n_q, x_q, c_q, m2_q = n_p[ys, xs], x_p[ys, xs], c[ys, xs], m2[ys, xs]
                near, w = dns.geometry_weight(n_p, x_p, tol, squarings, n_q, x_q)
                count["plane"] += int((take & ~near).sum())
                take = take & near
                for k in range(3):
                    wc = (w * c_q[..., k]).astype(F)
                    acc[..., k] = np.where(take, (acc[..., k] + wc).astype(F), acc[..., k])
                wq = (w * m2_q).astype(F)
                accq = np.where(take, (accq + wq).astype(F), accq)
                wsum = np.where(take, (wsum + w).astype(F), wsum)
        weighs = flagged & (wsum > F(0.0))
        count["no_tap"] = int((flagged & ~(wsum > F(0.0))).sum())
        count["estimated"] = int(weighs.sum())
        inv = (F(1.0) / wsum).astype(F)
        cb = (acc * inv[..., None]).astype(F)
        qb = (accq * inv).astype(F)
        new_v = dns.variance_of_mean(cb, qb, weight)
    if tally is not None:
        for k in ROUTES:
            tally[k] = tally.get(k, 0) + count[k]
    return np.where(weighs, new_v, v_in).astype(F).reshape(-1)


def records_of(colour, q, weight, hits=None):
    """HISTORY_DTYPE records with the given moments; the guide fields are hits' (as the temporal rule writes them) or zero"""
    n = len(np.asarray(weight).reshape(-1))
    records = np.zeros(n, dtype=HISTORY_DTYPE)
    records["c"], records["m2"], records["weight"] = np.asarray(colour, dtype=F).reshape(n, 3), np.asarray(q, dtype=F).reshape(n), np.asarray(weight, dtype=F).reshape(n)
    if hits is not None:
        hits = np.asarray(hits).reshape(n)
        records["n"], records["t"], records["x"] = hits["normal"], hits["t"], hits["point"]
        records["mesh"] = np.where(hits["hit"] != 0, hits["mesh"], MISS)
    return records


_sets = {}


def synthetic(width, height, clean=False, short=None, seed=11):
    """-> dict(records HISTORY_DTYPE [P], hits [P], var float32 [P]), made once and read-only.  The guides are denoise_sets.synthetic's: three
    meshes side by side, misses, NaN normals, hits with infinite t and point.  The records' guide fields are garbage (the rule must not read
    them); their moments are noisy colours with weights on both sides of 4.0 and exactly at it, weight 0 and below, and non-finite colour,
    m2 and weight.  clean: every pixel is a usable hit of the three meshes, with no special value.  short: a bool mask [P] -- weight 1 where
    it is set and 32 elsewhere."""
    key = (width, height, clean, None if short is None else np.asarray(short).tobytes(), seed)
    if key in _sets:
        return _sets[key]
    rng = np.random.default_rng(seed)
    n = width * height
    ys, xs = np.divmod(np.arange(n), width)
    hits = dns.synthetic(width, height)["hits"].copy()
    if clean:   # the flat plane's geometry under every pixel, three meshes side by side
        hits = np.zeros(n, dtype=HIT_DTYPE)
        hits["point"][:, 0], hits["point"][:, 1], hits["point"][:, 2] = (xs * 0.1).astype(F), (-(ys * 0.1)).astype(F), F(-5.0)
        hits["normal"][:, 2] = F(1.0)
        hits["t"] = np.sqrt((hits["point"].astype(np.float64) ** 2).sum(axis=1)).astype(F)
        hits["mesh"], hits["hit"] = np.minimum((3 * xs) // max(width, 1), 2), 1
    records = np.zeros(n, dtype=HISTORY_DTYPE)
    for name in ("n", "t", "x", "pad"):
        records[name] = rng.random(records[name].shape, dtype=F) * F(100.0)
    records["mesh"] = rng.integers(0, 5, n)
    base = np.array([[0.8, 0.3, 0.2], [0.2, 0.7, 0.3], [0.3, 0.4, 0.9]], dtype=F)[np.minimum((3 * xs) // max(width, 1), 2)]
    records["c"] = (base + rng.normal(0.0, 0.3, (n, 3)).astype(F)).astype(F)
    records["m2"] = ((records["c"] * records["c"]).sum(axis=1) + rng.random(n, dtype=F) * F(0.3)).astype(F)
    records["weight"] = rng.choice(np.array([1.0, 2.0, 3.5, 4.0, 4.0, 7.5, 32.0], dtype=F), n)
    var = (rng.random(n, dtype=F) * F(0.05)).astype(F)
    if short is not None:
        records["weight"] = np.where(np.asarray(short).reshape(n), F(1.0), F(32.0))
    if not clean:
        records["weight"][rng.random(n) < 0.05] = 0.0
        records["weight"][rng.random(n) < 0.02] = -2.0
        special = np.array([np.inf, -np.inf, np.nan, 3.4e38], dtype=F)
        pick = rng.random(n) < 0.03
        records["c"][pick, rng.integers(0, 3, int(pick.sum()))] = rng.choice(special, int(pick.sum()))
        pick = rng.random(n) < 0.02
        records["m2"][pick] = rng.choice(special, int(pick.sum()))
        pick = rng.random(n) < 0.02
        records["weight"][pick] = rng.choice(np.array([np.inf, np.nan], dtype=F), int(pick.sum()))
        pick = rng.random(n) < 0.03
        var[pick] = rng.choice(special, int(pick.sum()))
    s = dict(records=records, hits=hits, var=var)
    for a in s.values():
        a.setflags(write=False)
    _sets[key] = s
    return s
