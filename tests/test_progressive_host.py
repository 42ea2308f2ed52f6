"""Progressive GI frames, what needs no GPU: the contract in include/crt_hip.h, the exported symbols, and the numpy restatement of the
pixel fold that tests/test_gpu_progressive.py's list test compares the device's sums with."""
import ctypes as C
import os
import re

import numpy as np

import progressive_sets as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["crt_camera_sample_rays_device", "crt_accumulate_samples_device", "crt_render_progressive", "crt_progressive_samples"]


def header_text():
    """the header as running text: a comment's line breaks and its ` * ` margins are blanks"""
    return re.sub(r"\s+", " ", re.sub(r"\n \*", " ", open(os.path.join(ROOT, "include", "crt_hip.h")).read()))


def test_header_states_the_fold_and_the_two_invalid_rules():
    text = header_text()
    # the fold
    assert "d_sum[3p + c] = (sample == 0 ? 0.0f : d_sum[3p + c]) + d_rgb[3i + c]" in text
    assert "d_mean[3p + c] = d_sum[3p + c] * (1.0f / (float)(sample + 1))" in text
    assert "crt_gi_mix(crt_gi_mix(gi_seed, p), sample)" in text and "sum * (1 / (float)n)" in text
    assert "THE PIXELS OF ONE CALL MUST BE DISTINCT" in text
    # the two INVALID rules
    assert "With d_pixels == NULL, n must be width * height: anything else is CRT_ERR_INVALID" in text
    assert "first_sample != crt_progressive_samples(ctx)" in text and "use_gi == 0" in text
    # what the frame call covers
    assert "EVERY pixel of the frame" in text and "rays_per_pixel is NOT read" in text


def test_the_four_symbols_are_exported(pkg):
    L = pkg.lib()
    plain = C.CDLL(os.path.join(os.path.dirname(pkg.LIB_PATH), "libcrt_hip.so"))
    for name in SYMBOLS:
        assert name in pkg.DEVICE_SYMBOLS and hasattr(L, name) and hasattr(plain, name), name
    for name in ("camera_sample_rays_device", "accumulate_samples_device", "render_progressive", "progressive_samples"):
        assert callable(getattr(pkg.Tracer, name)), name
    # no context is an error (a count of zero), not a crash
    assert L.crt_progressive_samples(None) == 0
    assert L.crt_render_progressive(None, None, 0, 1, None) == pkg.CRT_ERR_INVALID
    assert L.crt_camera_sample_rays_device(None, 0, 0, None, 0, None, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_accumulate_samples_device(None, None, None, 0, 0, None, None, None) == pkg.CRT_ERR_INVALID


def documented(colours):
    """The documented formula, one scalar at a time: sum = 0; sum = sum + c_s in order; mean = sum * (1 / (float)n)"""
    n = len(colours)
    flat = colours.reshape(n, -1)
    total = np.zeros(flat.shape[1], dtype=np.float32)
    mean = np.zeros(flat.shape[1], dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(flat.shape[1]):
            acc = np.float32(0.0)
            for s in range(n):
                acc = np.float32(acc + flat[s, j])
            total[j] = acc
            mean[j] = np.float32(acc * np.float32(np.float32(1.0) / np.float32(n)))
    return total.reshape(colours.shape[1:]), mean.reshape(colours.shape[1:])


def test_the_numpy_fold_is_the_documented_formula():
    rng = np.random.default_rng(11)
    special = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, 1e-45, 3.4e38, -3.4e38, 1.0, 0.1], dtype=np.float32)
    for n in (1, 2, 3, 5, 16):
        colours = (rng.random((n, 40, 3), dtype=np.float32) * np.float32(4.0) - np.float32(1.0)).astype(np.float32)
        where = rng.random((n, 40, 3)) < 0.2
        colours[where] = rng.choice(special, size=int(where.sum()))
        colours[:, 0, 0] = np.float32(-0.0)              # a pixel of -0 samples alone: `0 + (-0)` is +0, and stays +0
        total, mean = ps.fold(colours)
        want_total, want_mean = documented(colours)
        assert total.dtype == np.float32 and mean.dtype == np.float32
        for got, want in ((total, want_total), (mean, want_mean)):
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), n
        assert total[0, 0].view(np.uint32) == 0 and mean[0, 0].view(np.uint32) == 0
    # not the mean numpy would compute: a division, or a sum in another order, rounds differently somewhere
    colours = rng.random((3, 4096, 3), dtype=np.float32)
    _, mean = ps.fold(colours)
    assert np.any(mean != (colours.sum(axis=0, dtype=np.float32) / np.float32(3)))
