"""Radiance queries with no host wait (include/crt_hip.h: crt_shoot_rays*_enqueue), what needs no GPU: the contract in the header, the
report's layout against a C program compiled from the header, the bindings, and the calls' capacity and chunk arithmetic
(csrc/shoot_caps.h) in a stand-alone host program built with the host sanitizers (tests/shoot_caps_check.cpp)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest


HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ["crt_shoot_rays_enqueue", "crt_shoot_rays_gi_enqueue", "crt_get_shoot_report", "crt_query_scratch_generation"]


def header():
    return open(os.path.join(ROOT, "include", "crt_hip.h")).read()


@pytest.fixture(scope="module")
def check_program(pkg):
    """tests/shoot_caps_check.cpp, compiled for the host alone with AddressSanitizer and UndefinedBehaviorSanitizer"""
    out = os.path.join(tempfile.gettempdir(), "crt_shoot_caps_check_%d" % os.getuid())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc"),
                           os.path.join(HERE, "shoot_caps_check.cpp"), "-o", out])
    return out


def test_the_header_carries_the_contract():
    text = header()
    for phrase in ("no hipStreamSynchronize", "level_cap", "crt_query_scratch_generation", "hipStreamIsCapturing", "single chain"):
        assert phrase in text, phrase
    # the existing calls' sentences are still theirs
    assert "ONCE PER LEVEL" in text and "CANNOT BE CAPTURED INTO A hipGraph" in text


def test_report_layout_matches_a_c_probe_of_the_header(pkg, check_program):
    r = subprocess.run([check_program, "--layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    probe = [int(x) for x in r.stdout.split()]
    R = pkg.ShootReport
    assert probe == [C.sizeof(R), R.levels.offset, R.overflow.offset, R.dropped.offset, R.level_rays.offset, R.hits.offset,
                     R.shadow_records.offset, R.rerouted.offset]
    assert probe == [552, 0, 4, 8, 16, 528, 536, 544]
    m = re.search(r"typedef struct crt_shoot_report \{(.*?)\} crt_shoot_report;", header(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.split("[")[0] for f in body.split(";") if f.strip() for n in re.sub(r"^\s*\w+\s+", "", f.strip()).replace(" ", "").split(",")]
    assert names == [n for n, _ in R._fields_]


def test_symbols_are_declared_exported_and_bound(pkg):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    plain = C.CDLL(os.path.join(os.path.dirname(pkg.LIB_PATH), "libcrt_hip.so"))
    L = pkg.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name + " is not declared"
        assert name in pkg.DEVICE_SYMBOLS and hasattr(L, name) and hasattr(plain, name), name
    vp = C.c_void_p
    assert L.crt_shoot_rays_enqueue.argtypes == [vp, vp, C.c_uint64, C.c_uint32, C.POINTER(pkg.Options), vp, vp, vp, vp]
    assert L.crt_shoot_rays_gi_enqueue.argtypes == [vp, vp, vp, C.c_uint64, C.c_uint32, C.POINTER(pkg.Options), vp, vp, vp, vp]
    assert L.crt_get_shoot_report.argtypes == [vp, C.POINTER(pkg.ShootReport)]
    assert L.crt_query_scratch_generation.restype == C.c_uint64
    # what needs no device: no context, no rays
    assert L.crt_shoot_rays_enqueue(None, None, 8, 2, None, None, None, None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_get_shoot_report(None, None) == pkg.CRT_ERR_INVALID
    assert L.crt_query_scratch_generation(None) == 0


def test_multi_device_tracer_refuses_the_enqueue_calls(pkg):
    """(Tracer._single looks at the device list alone: no device is needed to be refused)"""
    tracer = pkg.Tracer.__new__(pkg.Tracer)
    tracer.devices = [0, 0]
    tracer.ctx = None
    try:
        for call in (lambda: tracer.shoot_rays_enqueue(0, 8, 0), lambda: tracer.shoot_rays_gi_enqueue(0, 8, 0), tracer.shoot_report,
                     tracer.query_scratch_generation):
            with pytest.raises(RuntimeError, match="multi-device"):
                call()
    finally:
        tracer.devices = []
    with pytest.raises(ValueError, match="level_cap"):
        pkg.Tracer._level_cap([0, 1, 2], 5)
    assert pkg.Tracer._level_cap(None, 5) is None
    caps = pkg.Tracer._level_cap(range(6), 5)
    assert caps.dtype == np.uint32 and caps.tolist() == [0, 1, 2, 3, 4, 5]


def test_capacity_and_chunk_arithmetic_under_the_host_sanitizers(check_program):
    r = subprocess.run([check_program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 10000 and not r.stderr.strip(), r.stderr


def test_recorded_enqueue_times_are_complete():
    """profiles/shoot_enqueue.json (tools/shoot_enqueue_time.py on an MI355X; no threshold: DESIGN.md section 8f reads the figures and says
    that the enqueue call is not faster): per depth the synchronous call, the enqueue call and its graph replay, measured in one session
    with the frame of the same camera, and each with the synchronous call's colours and numbers."""
    import json
    doc = json.load(open(os.path.join(ROOT, "profiles", "shoot_enqueue.json")))
    assert doc["repeats"] >= 20 and doc["warmup"] >= 5 and doc["rays"] == 1920 * 1080 and doc["commit"]
    for depth in (0, 5, 8):
        row = doc["depths"][str(depth)]
        assert row["frame_ms"] > 0
        for column in ("device", "enqueue", "graph"):
            c = row[column]
            assert 0 < c["ms_min"] <= c["ms"] <= c["ms_max"], (depth, column)
            assert c["levels"] <= depth + 1 and c["level_rays"] == row["device"]["level_rays"] and c["level_rays"][0] == doc["rays"]
        for column in ("enqueue", "graph"):
            assert row[column]["equals_device"] is True and row[column]["overflow"] == 0 and row[column]["dropped"] == 0
        assert row["graph"]["scratch_generation_unchanged"] is True
