"""The variance estimate, what needs no GPU: the contract in include/crt_hip.h, the exported symbols, the numpy restatement of the rule
(tests/variance_sets.py) held to the host build of csrc/variance_rule.h -- the header the kernel compiles --, and what the estimate is worth
on a one-sample frame, from the restatements alone."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_sets as ads
import denoise_sets as dns
import guide_sets as g
import progressive_sets as ps
import query_sets as qs
import shoot_gi_sets as gs
import temporal_sets as ts
import variance_sets as vs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "course-assignment-danielhalachev_amd", "csrc")
SYMBOLS = ["crt_variance_estimate_defaults", "crt_variance_estimate_device", "crt_set_variance_estimate", "crt_get_variance_estimate"]
RULE = ["finite(x) is (x - x) == 0.0f",
        "A moment record is M = {c[3], m2, weight}, the fields of a crt_history_pixel (the record's own guide fields are not read)",
        "usable(M): weight > 0 and c[0..2], m2, weight all finite",
        "A guide is G = {n[3], x[3], t, mesh}, taken from a crt_hit as the denoiser takes it",
        "mesh = 0xFFFFFFFF when hit == 0",
        "V_in is the incoming variance of the mean",
        "The window radius is 3 and is not a setting",
        "It passes through, V' = V_in, when !usable(M_p), or mesh_p is a miss, or !(weight_p < min_history)",
        "Otherwise the centre is FLAGGED:",
        "tol = sigma_plane * t_p",
        "acc = {0,0,0}; accq = 0; wsum = 0",
        "for dy in -3..3, dx in -3..3 (row-major), q = (y+dy, x+dx); the offsets are compared with the room the centre has before a coordinate is formed:",
        "skip q outside the frame",
        "skip q with !usable(M_q)",
        "skip q with mesh_q != mesh_p",
        "d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z",
        "d = d > 0 ? d : 0",
        "d = d * d, normal_squarings times",
        "e = (n_p.x*(x_q.x - x_p.x) + n_p.y*(x_q.y - x_p.y)) + n_p.z*(x_q.z - x_p.z)",
        "ae = fabsf(e)",
        "skip unless ae <= tol",
        "a NaN skips",
        "wz = tol > 0 ? 1.0f - ae / tol : 1.0f",
        "w = d * wz",
        "acc_c = acc_c + w * c_q,c",
        "accq = accq + w * m2_q",
        "wsum = wsum + w",
        "if wsum > 0:",
        "inv = 1.0f / wsum",
        "Cb_c = acc_c * inv",
        "qb = accq * inv",
        "mm = (Cb_r*Cb_r + Cb_g*Cb_g) + Cb_b*Cb_b",
        "var = qb - mm",
        "iw = 1.0f / weight_p",
        "V' = (var > 0 ? var : 0) * iw",
        "else: V' = V_in",
        "a flagged centre with no surviving tap, or a NaN weight sum",
        "The centre is its own tap (dy = dx = 0)",
        "a NaN w makes wsum NaN, and the centre passes through"]
LIMITS = ["A miss pixel is never estimated",
          "The estimate is spatial: where the neighbourhood is a texture or a shadow edge inside one mesh and plane, the detail counts as variance and the filter smooths it more",
          "The window is 7x7 and dense; it does not widen where few taps survive"]


def running_text(path, margin):
    """a file as running text: line breaks, the comments' margins and the alignment of the rule's lines are blanks"""
    return re.sub(r"\s+", " ", re.sub(margin, " ", open(path).read()))


def test_header_states_the_rule_and_the_invalid_rules():
    text = running_text(os.path.join(ROOT, "include", "crt_hip.h"), r"\n \*")
    rule = running_text(os.path.join(CSRC, "variance_rule.h"), r"\n//")
    for line in RULE + LIMITS:
        assert line in text, line
        assert line in rule, line
    assert "/* ---- Variance estimate:" in open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    assert ("size must be sizeof(crt_variance_estimate) = 16, min_history > 0 and finite, normal_squarings <= 16, sigma_plane >= 0 and finite: "
            "anything else is CRT_ERR_INVALID, with nothing enqueued") in text
    assert "crt_variance_estimate_defaults: 4.0f, 5, 0.02f" in text
    assert "d_out_var may be d_var, because a pixel reads only its own V_in" in text
    assert ("an invalid crt_variance_estimate (above), width * height >= 2^31, a NULL array, d_moments not aligned to 16 bytes") in text
    assert "one launch, no wait, no allocation, no readback; it can be captured into a graph" in text
    assert "whose d_next is its d_moments and whose d_out_var is its d_var" in text
    assert "off by default; NULL turns it off" in text
    assert "Changing it drops nothing: not the guides, not the history, not the frame's serial" in text
    assert "chain guides when crt_guide_bounces(ctx) > 0, first hits otherwise" in text
    assert "with denoise == NULL they skip the estimate, since there is no spatial stage to serve" in text
    assert "That touches neither history: no ledger, slot or frame count" in text
    # the denoiser's sentences stand where they stood, with a pointer behind them
    assert "With count == 1 every variance is 0, so the filter hardly smooths: use at least 2 samples -- or crt_set_variance_estimate" in text
    denoise = running_text(os.path.join(CSRC, "denoise_rule.h"), r"\n//")
    assert "With count == 1 every variance is 0, so the filter hardly smooths. Use at least 2 samples -- or the variance estimate (csrc/variance_rule.h)" in denoise
    # the kernel is a translation unit of its own, and says how its LDS tile is laid out
    kernel = running_text(os.path.join(CSRC, "kernel_variance.h"), r"\n//")
    assert "three planes of 16-byte vectors" in kernel and "EVERY thread reaches" in kernel
    assert '#include "kernel_variance.h"' in open(os.path.join(CSRC, "crt_variance.hip")).read()


def test_the_symbols_are_exported_and_declared(pkg):
    L = pkg.lib()
    plain = C.CDLL(os.path.join(os.path.dirname(pkg.LIB_PATH), "libcrt_hip.so"))
    header = open(os.path.join(ROOT, "include", "crt_hip.h")).read()
    for name in SYMBOLS:
        assert name in pkg.DEVICE_SYMBOLS and hasattr(L, name) and hasattr(plain, name), name
        assert re.search(r"\b%s\(" % name, header), name
    for name in ("variance_estimate_device", "set_variance_estimate", "variance_estimate"):
        assert callable(getattr(pkg.Tracer, name)), name
    e = pkg.make_variance_estimate()
    assert (e.size, C.sizeof(pkg.VarianceEstimate), e.normal_squarings) == (16, 16, 5)
    assert (np.float32(e.min_history), np.float32(e.sigma_plane)) == (np.float32(4.0), np.float32(0.02))
    assert vs.DEFAULTS == (4.0, 5, 0.02)
    assert pkg.make_variance_estimate(min_history=2.0).min_history == 2.0
    with pytest.raises(KeyError):
        pkg.make_variance_estimate(size=3)
    assert "sizeof(crt_variance_estimate) == 16" in open(os.path.join(CSRC, "crt_variance.hip")).read()
    # the invalid-argument table's first row -- no context is an error, not a crash; the other rows need a context: tests/test_gpu_variance.py
    assert L.crt_variance_estimate_device(None, C.byref(e), 1, 1, None, None, None, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_variance_estimate_device(None, None, 0, 0, None, None, None, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_set_variance_estimate(None, C.byref(e)) == pkg.CRT_ERR_INVALID and L.crt_set_variance_estimate(None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_get_variance_estimate(None, C.byref(e)) == 0 and L.crt_get_variance_estimate(None, None) == 0
    L.crt_variance_estimate_defaults(None)


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.gettempdir(), "crt_variance_rule_shim_%d.so" % os.getuid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", os.path.join(HERE, "variance_rule_shim.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.shim_variance.argtypes = [C.c_float, C.c_uint32, C.c_float, C.c_int32, C.c_int32] + [C.c_void_p] * 8
    lib.shim_variance.restype = None
    return lib


def shim_estimate(shim, setting, width, height, s):
    n = width * height
    h = s["hits"]
    fields = [np.ascontiguousarray(h[k]) for k in ("t", "point", "normal", "mesh", "hit")]
    held = np.zeros(n + 1, dtype=ts.HISTORY_DTYPE)        # (one record more: room to start at a 16-byte boundary)
    off = (-held.ctypes.data) % 16
    held = np.frombuffer(held.view(np.uint8)[off:off + 64 * n], dtype=ts.HISTORY_DTYPE)
    held[:] = s["records"]
    out = np.full(n, 7.0, np.float32)
    shim.shim_variance(setting[0], setting[1], setting[2], width, height, held.ctypes.data, *[f.ctypes.data for f in fields], s["var"].ctypes.data,
                       out.ctypes.data)
    return out


@pytest.mark.parametrize("width,height", vs.SHAPES)
def test_the_numpy_rule_is_the_header(shim, width, height):
    assert vs.SHAPES == [(1, 1), (5, 3), (33, 9), (70, 20)] and len(vs.SETTINGS) == 4
    rows = (height, width)
    short = np.zeros(rows, bool)
    short[height - 1, width - 1] = True
    sets = [("the synthetic set", vs.synthetic(width, height)), ("every pixel flagged", vs.synthetic(width, height, clean=True, short=np.ones(rows, bool))),
            ("the last pixel alone flagged", vs.synthetic(width, height, clean=True, short=short))]
    for name, s in sets:
        for setting in vs.SETTINGS:
            what = "%dx%d, %s, %r" % (width, height, name, setting)
            dns.same(shim_estimate(shim, setting, width, height, s), vs.estimate(setting, width, height, s["records"], s["hits"], s["var"]), what)


def test_the_set_is_not_vacuous():
    """from the restatement alone: every pass-through route and every skip route is taken, and the set holds what it says"""
    width, height = vs.SHAPES[-1]
    s = vs.synthetic(width, height)
    r, h = s["records"], s["hits"]
    kinds = set(np.unique(np.where(h["hit"] != 0, h["mesh"], 99)).tolist())
    assert kinds == {0, 1, 2, 99}, "three meshes and misses"
    with np.errstate(all="ignore"):
        assert (~np.isfinite(r["c"])).any() and (~np.isfinite(r["m2"])).any() and (~np.isfinite(r["weight"])).any() and (r["weight"] == 0).any()
        assert np.isnan(h["normal"]).any() and np.isinf(h["t"]).any()
        assert (r["weight"] < 4.0).any() and (r["weight"] == 4.0).any() and (r["weight"] > 4.0).any()
    tally = {}
    got = vs.estimate(vs.DEFAULTS, width, height, r, h, s["var"], tally)
    print("routes at the defaults:", tally)
    for route in vs.ROUTES:
        assert tally[route] > 0, route
    flat = vs.estimate((2.0, 0, 0.0), width, height, r, h, s["var"], tally := {})
    print("routes with tol == 0:", tally)
    assert tally["estimated"] > 0 and tally["plane"] > 0, "tol == 0 keeps the taps exactly in the centre's plane"
    # a centre at exactly min_history passes through; only flagged centres change, and what they get is a variance
    changed = got.view(np.uint32) != s["var"].view(np.uint32)
    good = vs.usable(r["c"], r["m2"], r["weight"])
    with np.errstate(all="ignore"):
        flagged = good & (h["hit"] != 0) & (r["weight"] < np.float32(4.0))
    assert not (changed & ~flagged).any() and not changed[r["weight"] == 4.0].any()
    assert changed.sum() * 2 > flagged.sum()
    assert np.all(got[changed] >= 0) and np.all(np.isfinite(got[changed]))
    # the small shapes take the routes their size allows
    for width, height in vs.SHAPES[:3]:
        one = {}
        vs.estimate(vs.DEFAULTS, width, height, *[vs.synthetic(width, height, clean=True, short=np.ones(width * height, bool))[k] for k in ("records", "hits", "var")], one)
        assert one["flagged"] == width * height == one["estimated"] and one["outside"] > 0, (width, height, one)


# ---- what it is worth.  hw11 at 48x32, depth 3, 2 GI samples, min = max = 1: ONE sample a pixel, so every variance is 0.  Truth: the oracle's
# frame with rays_per_pixel = 64; RMSE over the hit pixels.  A: crt_denoise_defaults' filter on the sample and V = 0.  B: the same filter
# behind the estimate at crt_variance_estimate_defaults.  The sample, the first hits and the truth are the oracle's: no GPU.
_measured = {}


def restated_measure(scenes, oracle):
    if not _measured:
        o = gs.oracle_of(scenes, oracle, "hw11")
        colours = g.oracle_sample_colours(o, oracle, 1, depth=3, gi_samples=2)
        state = ads.run(colours, (1, 1, 0.05, 1e-4))
        assert np.all(state["counts"] == 1)
        mean, var = dns.variance(state["total"], state["sq"], state["counts"])
        assert not var.any(), "one sample: every variance is 0"
        hits = qs.oracle_hits(o, gs.scene_of(scenes, "hw11"), gs.camera_rays(o), qs.RAY_PRIMARY, vs.HIT_DTYPE)
        truth = ps.oracle_frame(scenes, oracle, "hw11", 3, 2, 64)
        hit = hits["hit"] != 0
        records = ts.frame(ts.DEFAULTS, gs.W, gs.H, None, None, state["total"], state["sq"], state["counts"], hits)[0]
        dns.same(records["c"], mean, "the temporal rule without history: the denoiser's mean")
        tally = {}
        estimated = vs.estimate(vs.DEFAULTS, gs.W, gs.H, records, hits, var, tally)
        a = dns.denoise(mean, var, hits, gs.H, gs.W, dns.DEFAULTS)[0]
        b = dns.denoise(mean, estimated, hits, gs.H, gs.W, dns.DEFAULTS)[0]
        _measured.update(hit=hit, tally=tally, rmse=(dns.rmse(mean, truth, hit), dns.rmse(a, truth, hit), dns.rmse(b, truth, hit)))
    return _measured


def test_the_estimate_lets_a_one_sample_frame_be_filtered(scenes, oracle):
    """measured here: the sample 0.07936, A 0.07933, B 0.05365, B / A 0.6763 over 1536 pixels"""
    m = restated_measure(scenes, oracle)
    noisy, a, b = m["rmse"]
    print("hw11, 1 sample: RMSE over %d hit pixels: the sample %.5f, the filter alone A %.5f, behind the estimate B %.5f, B / A %.4f; routes %r"
          % (int(m["hit"].sum()), noisy, a, b, b / a, m["tally"]))
    assert m["tally"]["flagged"] == m["tally"]["estimated"] + m["tally"]["no_tap"] and m["tally"]["estimated"] * 10 >= int(m["hit"].sum()) * 9
    assert b < a
