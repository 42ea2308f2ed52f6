"""What the tests of the split GI frames (crt_shoot_rays_gi_split*, crt_split_fold_device, crt_split_recombine_device, crt_render_*_split)
share: the rule of include/crt_hip.h ("Split GI frames") restated in numpy float32 -- one operation and one astype at a time, so that every
intermediate is rounded to float32 once, as the -ffp-contract=off build of csrc/split_rule.h rounds it --, the frame's loop over it, and a
synthetic set with the special values."""
import numpy as np

import adaptive_sets as ads
import denoise_sets as dns

F = np.float32
BACKGROUND, DIFFUSE, RECURSES, INVALID = 0, 1, 2, 3      # CRT_SHADE_*


def direct_of(status, light, gi_sample_size):
    """the direct part of a sample: status uint8 [n] (level 0's CRT_SHADE_*), light float32 [n, 3] (level 0's colours behind its lighting)"""
    status, light = np.asarray(status).reshape(-1), np.asarray(light, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        gi_inv = F(F(1.0) / F(gi_sample_size + 1))
        scaled = (light * gi_inv).astype(F)
    out = np.zeros_like(light)
    out[status == DIFFUSE] = scaled[status == DIFFUSE]
    out[status == BACKGROUND] = light[status == BACKGROUND]
    return out


def fold(sample, rgb, direct, dsum, rsum, rsq):
    """One step for the entries' pixels: rgb, direct, dsum, rsum float32 [P, 3], rsq float32 [P] -> (dsum, rsum, rsq); the state is not read
    when sample == 0."""
    rgb, direct = np.asarray(rgb, dtype=F).reshape(-1, 3), np.asarray(direct, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r = (rgb - direct).astype(F)
        dsum = ((np.zeros_like(direct) if sample == 0 else dsum) + direct).astype(F)
        rsum = ((np.zeros_like(r) if sample == 0 else rsum) + r).astype(F)
        rr = (r[:, 0] * r[:, 0]).astype(F)
        gg = (r[:, 1] * r[:, 1]).astype(F)
        bb = (r[:, 2] * r[:, 2]).astype(F)
        r2 = (rr + gg).astype(F)
        r2 = (r2 + bb).astype(F)
        rsq = ((np.zeros_like(r2) if sample == 0 else rsq) + r2).astype(F)
    return dsum, rsum, rsq


def fold_listed(sample, rgb, direct, pixels, n_pixels, dsum, rsum, rsq):
    """crt_split_fold_device: entry i is pixel pixels[i] (None: pixel i); an index outside the frame is skipped -> copies of the state"""
    dsum, rsum, rsq = np.array(dsum, dtype=F).reshape(-1, 3), np.array(rsum, dtype=F).reshape(-1, 3), np.array(rsq, dtype=F).reshape(-1)
    rgb, direct = np.asarray(rgb, dtype=F).reshape(-1, 3), np.asarray(direct, dtype=F).reshape(-1, 3)
    pixels = np.arange(len(rgb), dtype=np.int64) if pixels is None else np.asarray(pixels).astype(np.int64)
    inside = pixels < n_pixels
    p = pixels[inside]
    dsum[p], rsum[p], rsq[p] = fold(sample, rgb[inside], direct[inside], dsum[p], rsum[p], rsq[p])
    return dsum, rsum, rsq


def recombine(filtered, dsum, counts):
    filtered, dsum, counts = np.asarray(filtered, dtype=F).reshape(-1, 3), np.asarray(dsum, dtype=F).reshape(-1, 3), np.asarray(counts).reshape(-1)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / np.maximum(counts, 1).astype(F)).astype(F)
        dmean = (dsum * inv[:, None]).astype(F)
        out = (filtered + dmean).astype(F)
    return np.where((counts == 0)[:, None], filtered, out).astype(F)


def run(colours, directs, adaptive, passes=None):
    """The split frame's loop: adaptive_sets.run's loop over colours float32 [S, P, 3] with the split's fold beside it over each pass's own list
    -> adaptive_sets.run's dict and dsum [P, 3], rsum [P, 3], rsq [P]."""
    colours, directs = np.asarray(colours, dtype=F), np.asarray(directs, dtype=F)
    n_pixels = colours.shape[1]
    passes = len(colours) if passes is None else passes
    total, sq, mean = np.zeros((n_pixels, 3), F), np.zeros(n_pixels, F), np.zeros((n_pixels, 3), F)
    dsum, rsum, rsq = np.zeros((n_pixels, 3), F), np.zeros((n_pixels, 3), F), np.zeros(n_pixels, F)
    counts = np.zeros(n_pixels, np.uint32)
    listed = np.arange(n_pixels)
    active = [n_pixels]
    for s in range(passes):
        if len(listed):
            t, q, m, c, keep = ads.step(s, colours[s, listed], total[listed], sq[listed], adaptive)
            total[listed], sq[listed], mean[listed], counts[listed] = t, q, m, c
            dsum[listed], rsum[listed], rsq[listed] = fold(s, colours[s, listed], directs[s, listed], dsum[listed], rsum[listed], rsq[listed])
            listed = listed[keep]
        active.append(len(listed))
    return dict(total=total, sq=sq, mean=mean, counts=counts, active=active, listed=listed.astype(np.uint32), dsum=dsum, rsum=rsum, rsq=rsq)


def denoised(state, hits, height, width, denoise):
    """crt_render_denoised_split: the denoiser's rule on the rest's mean and variance, then the direct part's mean back"""
    mean, var = dns.variance(state["rsum"], state["rsq"], state["counts"])
    filtered = dns.denoise(mean, var, hits, height, width, denoise)[0]
    return recombine(filtered, state["dsum"], state["counts"]).reshape(height, width, 3)


_sets = {}


def synthetic(n, seed=3):
    """n entries of samples: rgb and direct float32 [3, n, 3] (sample 0, 1, 2) with NaN, +-inf, denormals and -0 among them, and poison for
    the state; read-only"""
    if (n, seed) in _sets:
        return _sets[(n, seed)]
    rng = np.random.default_rng(seed)
    rgb = (rng.random((3, n, 3), dtype=F) * F(1.5)).astype(F)
    direct = (rgb * rng.random((3, n, 3), dtype=F)).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, 1e-42, -1e-45, -0.0, 3e38, -3e38, 0.0], dtype=F)
    for a in (rgb, direct):
        flat = a.reshape(-1)
        pick = rng.random(flat.size) < 0.08
        pick[:min(flat.size, len(special))] = True
        flat[pick] = np.resize(special, int(pick.sum()))
    both = rng.random((3, n)) < 0.03          # an infinite channel in both parts: inf - inf
    rgb[both, 0] = np.inf
    direct[both, 0] = np.inf
    poison = dict(dsum=np.full((n, 3), np.nan, F), rsum=np.full((n, 3), -np.inf, F), rsq=np.full(n, 7e37, F))
    out = dict(rgb=rgb, direct=direct, **poison)
    for a in out.values():
        a.setflags(write=False)
    _sets[(n, seed)] = out
    return out
