"""What the tests of the progressive GI frames (crt_render_progressive and its two primitives) share: the oracle's multi-sample frames of
tests/shoot_gi_sets.py's scenes, made once, and the pixel fold restated in numpy."""
import numpy as np

import shoot_gi_sets as gs

_frames = {}


def oracle_frame(scenes, oracle, name, depth, samples, rays_per_pixel, seed=gs.SEED):
    """The oracle's GI frame with `rays_per_pixel` rays per pixel (bucket_size 16: every pixel of the 48x32 frame is covered)"""
    key = (name, depth, samples, rays_per_pixel, seed)
    if key not in _frames:
        o = gs.oracle_of(scenes, oracle, name)
        rgb, _ = o.render(options=oracle.make_options(depth, use_gi=1, gi_sample_size=samples, rays_per_pixel=rays_per_pixel, gi_seed=seed))
        rgb.setflags(write=False)
        _frames[key] = rgb
    return _frames[key]


def frame_options(pkg, depth, samples, rays_per_pixel, seed=gs.SEED):
    """the library's options of that frame (render_progressive does not read rays_per_pixel; Tracer.render does)"""
    return pkg.make_options(depth, use_gi=True, gi_sample_size=samples, rays_per_pixel=rays_per_pixel, gi_seed=seed)


def fold(colours):
    """The frame's rule for a pixel (include/crt_hip.h, "The fold"): colours float32 [n, ...] -> (sum, mean) with
    sum = ((0 + c0) + c1) + ... in float32 and mean = sum * float32(1 / float32(n)) -- one rounding per operation, NaN and inf as IEEE has them."""
    colours = np.asarray(colours, dtype=np.float32)
    total = np.zeros(colours.shape[1:], dtype=np.float32)
    with np.errstate(all="ignore"):
        for c in colours:
            total = (total + c).astype(np.float32)
        scale = np.float32(1.0) / np.float32(len(colours))
        return total, (total * scale).astype(np.float32)
