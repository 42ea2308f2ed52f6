"""What the tests of the denoiser (crt_sample_variance_device, crt_denoise_device, crt_render_denoised) share: the rule of include/crt_hip.h
("Denoising") restated in numpy float32 -- one operation and one astype at a time, so that every intermediate is rounded to float32 once, as
the -ffp-contract=off build of csrc/denoise_rule.h rounds it --, a synthetic image with guides to run it on, and the bit-for-bit comparison."""
import numpy as np

F = np.float32
MISS = np.uint32(0xFFFFFFFF)
H5 = [F(1.0 / 16.0), F(1.0 / 4.0), F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0)]
G3 = [[F(1), F(2), F(1)], [F(2), F(4), F(2)], [F(1), F(2), F(1)]]
# crt_hit (48 bytes), as the package's HIT_DTYPE has it
HIT_DTYPE = np.dtype([("t", np.float32), ("point", np.float32, 3), ("normal", np.float32, 3), ("u", np.float32), ("v", np.float32),
                      ("mesh", np.uint32), ("triangle", np.uint32), ("hit", np.uint32)])
DEFAULTS = (4, 5, 2.0, 0.02, 1e-6)
# (iterations is the caller's: the tests run 0..5 of each)  normal_squarings, sigma_colour, sigma_plane, floor
SETTINGS = [(5, 4.0, 0.02, 1e-6), (0, 4.0, 0.0, 1e-6), (16, 0.0, 0.02, 1e-6), (2, 1.0, 0.5, 1e-38), (5, 4.0, 0.02, 3e38), (1, 100.0, 0.005, 1e-3),
            (3, 0.5, 10.0, 1e-45)]
ROUTES = ("outside", "unusable", "mesh", "plane", "centre_unusable", "no_weight")


def settings(denoise):
    """(iterations, normal_squarings, sigma_colour, sigma_plane, floor) of a crt_denoise or of a tuple"""
    if isinstance(denoise, tuple):
        return denoise
    return (int(denoise.iterations), int(denoise.normal_squarings), float(denoise.sigma_colour), float(denoise.sigma_plane), float(denoise.floor))


def same(got, want, what):
    """bit for bit; a NaN is a NaN (which payload an addition of two NaNs keeps is the instruction's choice, not the rule's)"""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %r %r against %r %r" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype == np.float32:
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    assert not bad.any(), "%s: %d differ, first at %d: %r against %r" % (what, int(bad.sum()), int(np.flatnonzero(bad)[0]), got[bad][0], want[bad][0])


def finite(x):
    with np.errstate(all="ignore"):
        return (x - x).astype(F) == F(0.0)


# ---- what the stages' rules share (csrc/filter_rule.h), restated once: tests/temporal_sets.py and tests/variance_sets.py call these too

def sum3(a, b):
    """(a0*b0 + a1*b1) + a2*b2 over the last axis: three products, then two sums in this association"""
    p0 = (a[..., 0] * b[..., 0]).astype(F)
    p1 = (a[..., 1] * b[..., 1]).astype(F)
    p2 = (a[..., 2] * b[..., 2]).astype(F)
    p01 = (p0 + p1).astype(F)
    return (p01 + p2).astype(F)


def normal_dot(n_p, n_q):
    """d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z"""
    return sum3(n_p, n_q)


def plane_distance(n_p, x_p, x_q):
    """ae = fabsf(e), e = (n_p.x*(x_q.x - x_p.x) + n_p.y*(x_q.y - x_p.y)) + n_p.z*(x_q.z - x_p.z)"""
    o0 = (x_q[..., 0] - x_p[..., 0]).astype(F)
    o1 = (x_q[..., 1] - x_p[..., 1]).astype(F)
    o2 = (x_q[..., 2] - x_p[..., 2]).astype(F)
    e = sum3(n_p, np.stack([o0, o1, o2], axis=-1))
    return np.abs(e).astype(F)


def geometry_weight(n_p, x_p, tol, squarings, n_q, x_q):
    """the denoiser's and the variance estimate's weight of a tap -> (near, g): near is False where the tap is skipped (either side NaN too)"""
    d = normal_dot(n_p, n_q)
    d = np.where(d > F(0.0), d, F(0.0)).astype(F)
    for _k in range(squarings):
        d = (d * d).astype(F)
    ae = plane_distance(n_p, x_p, x_q)
    near = ae <= tol
    r = (ae / tol).astype(F)
    wz = np.where(tol > F(0.0), (F(1.0) - r).astype(F), F(1.0)).astype(F)
    return near, (d * wz).astype(F)


def usable(c, m2, weight):
    """weight > 0 and c[0..2], m2, weight all finite"""
    with np.errstate(all="ignore"):
        return (weight > F(0.0)) & finite(c[..., 0]) & finite(c[..., 1]) & finite(c[..., 2]) & finite(m2) & finite(weight)


def variance_of_mean(c, q, n):
    """V = (var > 0 ? var : 0) * (1.0f / n), var = q - ((C_r*C_r + C_g*C_g) + C_b*C_b)"""
    mm = sum3(c, c)
    var = (q - mm).astype(F)
    inv = (F(1.0) / n).astype(F)
    return (np.where(var > F(0.0), var, F(0.0)).astype(F) * inv).astype(F)


def variance(total, sq, counts):
    """From the fold's state: total float32 [P, 3], sq float32 [P], counts uint32 [P] -> (mean [P, 3], V [P], the variance of the mean)."""
    total, sq, counts = np.asarray(total, dtype=F).reshape(-1, 3), np.asarray(sq, dtype=F).reshape(-1), np.asarray(counts).reshape(-1)
    with np.errstate(all="ignore"):
        n = np.maximum(counts, 1).astype(F)
        inv = (F(1.0) / n).astype(F)
        c0 = (total[:, 0] * inv).astype(F)
        c1 = (total[:, 1] * inv).astype(F)
        c2 = (total[:, 2] * inv).astype(F)
        q = (sq * inv).astype(F)
        mean = np.stack([c0, c1, c2], axis=1)
        v = variance_of_mean(mean, q, n)
    none = counts == 0
    mean[none] = F(0.0)
    v[none] = F(0.0)
    return mean, v


def guides_of(hits, height, width):
    """crt_hit records [H * W] -> the guide's fields as [H, W, ...] arrays; mesh = 0xFFFFFFFF when hit == 0"""
    hits = np.asarray(hits).reshape(height, width)
    return dict(n=np.ascontiguousarray(hits["normal"]), x=np.ascontiguousarray(hits["point"]), t=np.ascontiguousarray(hits["t"]),
                mesh=np.where(hits["hit"] != 0, hits["mesh"], MISS).astype(np.uint32))


def tap(height, width, oy, ox):
    """the tap at offset (oy, ox) of every pixel: (inside [H, W], the clipped row and column indices to read through)"""
    ys = np.arange(height, dtype=np.int64)[:, None] + oy
    xs = np.arange(width, dtype=np.int64)[None, :] + ox
    inside = (ys >= 0) & (ys < height) & (xs >= 0) & (xs < width)
    return inside, np.broadcast_to(np.clip(ys, 0, height - 1), inside.shape), np.broadcast_to(np.clip(xs, 0, width - 1), inside.shape)


def iteration(colour, var, guides, step, denoise, tally=None):
    """One iteration of the rule: colour float32 [H, W, 3], var float32 [H, W] -> (colour', var').  tally: a dict that receives how many
    taps each skip route skipped and how many centres each pass-through route took (ROUTES)."""
    _, squarings, sigma_colour, sigma_plane, floor = settings(denoise)
    sigma_colour, sigma_plane, floor = F(sigma_colour), F(sigma_plane), F(floor)
    height, width = var.shape
    n_p, x_p, t_p, mesh_p = guides["n"], guides["x"], guides["t"], guides["mesh"]
    count = dict.fromkeys(ROUTES, 0)
    with np.errstate(all="ignore"):
        usable = finite(colour[..., 0]) & finite(colour[..., 1]) & finite(colour[..., 2]) & finite(var)
        vnum, vden = np.zeros((height, width), F), np.zeros((height, width), F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inside, ys, xs = tap(height, width, dy, dx)
                vq = var[ys, xs]
                take = inside & finite(vq)
                gv = (G3[dy + 1][dx + 1] * vq).astype(F)
                vnum = np.where(take, (vnum + gv).astype(F), vnum)
                vden = np.where(take, (vden + G3[dy + 1][dx + 1]).astype(F), vden)
        vp = (vnum / vden).astype(F)
        s2 = F(sigma_colour * sigma_colour)
        s2v = (s2 * vp).astype(F)
        den = (s2v + floor).astype(F)
        tol = (sigma_plane * t_p).astype(F)
        is_hit = mesh_p != MISS
        acc = np.zeros((height, width, 3), F)
        accv, wsum = np.zeros((height, width), F), np.zeros((height, width), F)
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                inside, ys, xs = tap(height, width, dy * step, dx * step)
                take = usable & inside
                count["outside"] += int((usable & ~inside).sum())
                count["unusable"] += int((take & ~usable[ys, xs]).sum())
                take = take & usable[ys, xs]
                count["mesh"] += int((take & (guides["mesh"][ys, xs] != mesh_p)).sum())
                take = take & (guides["mesh"][ys, xs] == mesh_p)
                n_q, x_q, c_q, v_q = n_p[ys, xs], x_p[ys, xs], colour[ys, xs], var[ys, xs]
                near, g = geometry_weight(n_p, x_p, tol, squarings, n_q, x_q)
                count["plane"] += int((take & is_hit & ~near).sum())
                take = take & (~is_hit | near)
                g = np.where(is_hit, g, F(1.0)).astype(F)
                dc = (c_q - colour).astype(F)
                d2 = sum3(dc, dc)
                dd = (den + d2).astype(F)
                wl = (den / dd).astype(F)
                hh = F(H5[dy + 2] * H5[dx + 2])
                hg = (hh * g).astype(F)
                w = (hg * wl).astype(F)
                for c in range(3):
                    wc = (w * c_q[..., c]).astype(F)
                    acc[..., c] = np.where(take, (acc[..., c] + wc).astype(F), acc[..., c])
                ww = (w * w).astype(F)
                wv = (ww * v_q).astype(F)
                accv = np.where(take, (accv + wv).astype(F), accv)
                wsum = np.where(take, (wsum + w).astype(F), wsum)
        weighs = usable & (wsum > F(0.0))
        count["centre_unusable"] += int((~usable).sum())
        count["no_weight"] += int((usable & ~(wsum > F(0.0))).sum())
        inv = (F(1.0) / wsum).astype(F)
        new_c = (acc * inv[..., None]).astype(F)
        i2 = (inv * inv).astype(F)
        new_v = (accv * i2).astype(F)
    if tally is not None:
        for k in ROUTES:
            tally[k] = tally.get(k, 0) + count[k]
    return np.where(weighs[..., None], new_c, colour).astype(F), np.where(weighs, new_v, var).astype(F)


def denoise(colour, var, hits, height, width, denoise_settings, tally=None):
    """settings[0] iterations of the rule on a height x width image: colour [H * W, 3] (any shape of that size), var [H * W], hits crt_hit
    records [H * W] -> (colour' [H, W, 3], var' [H, W]); 0 iterations copy."""
    colour = np.array(colour, dtype=F).reshape(height, width, 3)
    var = np.array(var, dtype=F).reshape(height, width)
    guides = guides_of(hits, height, width)
    for k in range(settings(denoise_settings)[0]):
        colour, var = iteration(colour, var, guides, 1 << k, denoise_settings, tally)
    return colour, var


def synthetic(width, height, seed=5):
    """A fold's state and first-hit records for a width x height image: three meshes side by side (a plane facing the camera, a slanted
    plane, a sphere patch whose normals turn), miss pixels (a band at the top and a sprinkle), noisy colours of 0..8 samples a pixel, and the
    special pixels: non-finite sums and second moments, normals with a NaN, hits with infinite t and point, counts 0 and 1, denormal
    variances.  -> dict(total [P, 3], sq [P], counts [P], hits [P])."""
    rng = np.random.default_rng(seed)
    n = width * height
    ys, xs = np.divmod(np.arange(n), width)
    hits = np.zeros(n, dtype=HIT_DTYPE)
    region = np.minimum((3 * xs) // max(width, 1), 2)
    px, py = (xs * 0.1).astype(F), (-(ys * 0.1)).astype(F)
    point, normal = np.zeros((n, 3), F), np.zeros((n, 3), F)
    point[:, 0], point[:, 1] = px, py
    flat, slant, ball = region == 0, region == 1, region == 2
    point[flat, 2], normal[flat] = F(-5.0), (0.0, 0.0, 1.0)
    slope = np.array([0.3, 0.0, 1.0]) / np.sqrt(1.09)
    point[slant, 2] = (-5.0 - 0.3 * px[slant]).astype(F)
    normal[slant] = slope.astype(F)
    centre = np.array([0.1 * width * 5.0 / 6.0, -0.05 * height, -9.0])
    off = np.stack([px[ball] - centre[0], py[ball] - centre[1]], axis=1).astype(np.float64)
    rz = np.sqrt(np.maximum(16.0 - (off ** 2).sum(axis=1), 1.0))
    point[ball, 2] = (centre[2] + rz).astype(F)
    nb = np.concatenate([off, rz[:, None]], axis=1)
    normal[ball] = (nb / np.linalg.norm(nb, axis=1, keepdims=True)).astype(F)
    hits["point"], hits["normal"] = point, normal
    hits["t"] = np.sqrt((point.astype(np.float64) ** 2).sum(axis=1)).astype(F)
    hits["mesh"], hits["triangle"], hits["hit"] = region, rng.integers(0, 50, n), 1
    hits["u"], hits["v"] = rng.random(n, dtype=F), rng.random(n, dtype=F)
    miss = (ys < height // 8) | ((xs * 5 + ys * 3) % 13 == 0)
    hits[miss] = np.zeros(1, dtype=HIT_DTYPE)   # hit == 0: every other field is 0
    # colours: a truth per region with a gradient, sigma 0.3 noise, 0..8 samples a pixel
    base = np.array([[0.8, 0.3, 0.2], [0.2, 0.7, 0.3], [0.3, 0.4, 0.9]], dtype=F)[region]
    truth = (base * (F(0.6) + F(0.4) * (ys / max(height, 1)).astype(F))[:, None]).astype(F)
    truth[miss] = (0.05, 0.1, 0.2)
    counts = rng.integers(0, 9, n).astype(np.uint32)
    counts[rng.random(n) < 0.6] = 4
    total, sq = np.zeros((n, 3), F), np.zeros(n, F)
    for s in range(8):
        c = (truth + rng.normal(0.0, 0.3, (n, 3)).astype(F)).astype(F)
        on = counts > s
        total[on] = (total[on] + c[on]).astype(F)
        sq[on] = (sq[on] + (c[on] * c[on]).sum(axis=1).astype(F)).astype(F)
    # the special pixels (a fixed few by position as well, so that the small shapes have some)
    special = np.array([np.inf, -np.inf, np.nan, 3.4e38, -3.4e38], dtype=F)
    pick = rng.random(n) < 0.02
    total[pick, rng.integers(0, 3, int(pick.sum()))] = rng.choice(special, int(pick.sum()))
    pick = rng.random(n) < 0.02
    sq[pick] = rng.choice(special, int(pick.sum()))
    pick = (rng.random(n) < 0.02) & ~miss
    hits["normal"][pick, 1] = np.nan
    pick = (rng.random(n) < 0.02) & ~miss
    hits["t"][pick] = np.inf
    hits["point"][pick] = np.inf
    pick = rng.random(n) < 0.03
    total[pick], sq[pick], counts[pick] = 0.0, rng.choice(np.array([1e-44, 3e-42, 1e-39], dtype=F), int(pick.sum())), 2
    pick = rng.random(n) < 0.02
    counts[pick] = rng.integers(0, 2, int(pick.sum()))
    return dict(total=total, sq=sq, counts=counts, hits=hits)


def rmse(a, b, where=None):
    d = np.asarray(a, dtype=np.float64).reshape(-1, 3) - np.asarray(b, dtype=np.float64).reshape(-1, 3)
    if where is not None:
        d = d[np.asarray(where).reshape(-1)]
    return float(np.sqrt(np.mean(d * d)))
