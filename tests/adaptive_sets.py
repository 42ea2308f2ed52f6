"""What the tests of adaptive sampling (crt_adaptive_step_device, crt_render_adaptive) share: the stopping rule of include/crt_hip.h
("The rule") restated in numpy float32 -- one operation and one astype at a time, so that every intermediate is rounded to float32 once,
as the -ffp-contract=off build of csrc/adaptive_rule.h rounds it -- and the frame's pass loop over it."""
import numpy as np

F = np.float32


def settings(adaptive):
    """(min_samples, max_samples, threshold, floor) of a crt_adaptive or of a tuple"""
    if isinstance(adaptive, tuple):
        return adaptive
    return int(adaptive.min_samples), int(adaptive.max_samples), float(adaptive.threshold), float(adaptive.floor)


def moments(total, sq, n):
    """(mean, |mean|^2, var) of a state after n samples, as the rule computes them"""
    with np.errstate(all="ignore"):
        inv = F(F(1.0) / F(n))
        mean = (total * inv).astype(F)
        q = (sq * inv).astype(F)
        m0 = (mean[:, 0] * mean[:, 0]).astype(F)
        m1 = (mean[:, 1] * mean[:, 1]).astype(F)
        m2 = (mean[:, 2] * mean[:, 2]).astype(F)
        mm = (m0 + m1).astype(F)
        mm = (mm + m2).astype(F)
        var = (q - mm).astype(F)
    return mean, mm, var


def step(s, colour, total, sq, adaptive):
    """One step of the rule for sample s: colour, total float32 [P, 3], sq float32 [P] -> (total, sq, mean, count, keep)."""
    lo, hi, threshold, floor = settings(adaptive)
    threshold, floor = F(threshold), F(floor)
    colour = np.asarray(colour, dtype=F)
    n = s + 1
    with np.errstate(all="ignore"):
        total = ((np.zeros_like(total) if s == 0 else total) + colour).astype(F)
        r, g, b = colour[:, 0], colour[:, 1], colour[:, 2]
        rr = (r * r).astype(F)
        gg = (g * g).astype(F)
        bb = (b * b).astype(F)
        c2 = (rr + gg).astype(F)
        c2 = (c2 + bb).astype(F)
        sq = ((np.zeros_like(sq) if s == 0 else sq) + c2).astype(F)
        mean, mm, var = moments(total, sq, n)
        t2 = F(threshold * threshold)
        t2n = F(t2 * F(n))
        bound = (t2n * np.where(mm > floor, mm, floor).astype(F)).astype(F)
        converged = var <= bound                       # False when either side is NaN
    count = np.full(len(colour), n, dtype=np.uint32)
    keep = (n < hi) & ~((n >= lo) & converged)
    return total, sq, mean, count, keep


def run(colours, adaptive, passes=None):
    """The frame's loop over colours float32 [S, P, 3] (sample s of every pixel): pass s steps the active pixels, the kept ones are the
    next pass's.  -> dict(total [P, 3], sq [P], mean [P, 3], counts [P], active = [len(A_0), len(A_1), ...], one more than passes run)."""
    colours = np.asarray(colours, dtype=F)
    n_pixels = colours.shape[1]
    passes = len(colours) if passes is None else passes
    total, sq, mean = np.zeros((n_pixels, 3), F), np.zeros(n_pixels, F), np.zeros((n_pixels, 3), F)
    counts = np.zeros(n_pixels, np.uint32)
    listed = np.arange(n_pixels)
    active = [n_pixels]
    for s in range(passes):
        if len(listed):
            t, q, m, c, keep = step(s, colours[s, listed], total[listed], sq[listed], adaptive)
            total[listed], sq[listed], mean[listed], counts[listed] = t, q, m, c
            listed = listed[keep]
        active.append(len(listed))
    return dict(total=total, sq=sq, mean=mean, counts=counts, active=active, listed=listed.astype(np.uint32))


def shares(counts, adaptive):
    """the three classes of a frame's pixels: stopped at min_samples, strictly between, ran to max_samples"""
    lo, hi = settings(adaptive)[:2]
    counts = np.asarray(counts).reshape(-1)
    return (float(np.mean(counts == lo)), float(np.mean((counts > lo) & (counts < hi))), float(np.mean(counts == hi)))
