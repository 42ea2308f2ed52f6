"""bench.py reads per-launch counters from the committed rocprofv3 passes (profiles/r04_pmc.json, hbm_traffic.json) and must refuse them
when they were collected from other kernel sources than the ones that are running (round 3's review, weak #8)."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_counters_of_other_kernel_sources_are_refused(tmp_path):
    bench = load_bench()
    key = "hw14_1920x1080_d8_n1"
    json.dump({"csrc_sha256": "a" * 64, key: {"kernel": "k", "per_launch": {}}}, open(tmp_path / "r04_pmc.json", "w"))
    json.dump({key: {"csrc_sha256": "a" * 64, "hbm_bytes_per_launch": 123}}, open(tmp_path / "hbm_traffic.json", "w"))
    pmc, traffic, why = bench.committed_evidence(str(tmp_path), key, "a" * 64)
    assert pmc is not None and traffic == 123 and why is None
    pmc, traffic, why = bench.committed_evidence(str(tmp_path), key, "b" * 64)
    assert pmc is None and traffic is None and "other kernel sources" in why and "aaaaaaaaaaaa" in why and "bbbbbbbbbbbb" in why
    # the traffic file alone may be stale too
    json.dump({key: {"csrc_sha256": "c" * 64, "hbm_bytes_per_launch": 123}}, open(tmp_path / "hbm_traffic.json", "w"))
    pmc, traffic, why = bench.committed_evidence(str(tmp_path), key, "a" * 64)
    assert pmc is not None and traffic is None and why is None
    os.remove(tmp_path / "r04_pmc.json")
    pmc, traffic, why = bench.committed_evidence(str(tmp_path), key, "a" * 64)
    assert pmc is None and traffic is None and "not usable" in why


def test_committed_counters_are_of_this_tree(pkg):
    """What is committed under profiles/ was collected from the kernel sources of this very tree (after a kernel change:
    `bash tools/final_numbers.sh r04` on the GPU box, copy its summaries into profiles/ -- bench.py refuses the old ones until then)."""
    bench = load_bench()
    pmc, traffic, why = bench.committed_evidence(os.path.join(ROOT, "profiles"), "hw14_1920x1080_d8_n1", pkg.csrc_sha256())
    assert why is None, why
    assert pmc["hw14_1920x1080_d8_n1"]["kernel"].startswith("bvh_trace_shadow<0") and traffic and traffic > 0


def test_dump_outputs_writes_the_frame_or_a_fixed_sample(tmp_path):
    """bench.py --dump-outputs: the whole frame as frame.npy (float32) while it fits the limit; beyond it, a sample of its pixels
    drawn with a fixed seed (the same pixels in every run of the same size), colours and exact row-major indices, within the limit."""
    import numpy as np
    bench = load_bench()
    h, w = 24, 40
    frame = np.arange(h * w * 3, dtype=np.float32) * np.float32(0.25)
    assert bench.dump_outputs(str(tmp_path / "whole"), frame, h, w) == ["frame"]
    got = np.load(str(tmp_path / "whole" / "frame.npy"))
    assert got.dtype == np.float32 and got.shape == (h, w, 3) and np.array_equal(got.reshape(-1), frame)
    limit = 4000                                        # smaller than the frame's 11520 bytes
    names = [bench.dump_outputs(str(tmp_path / d), frame, h, w, limit=limit) for d in ("a", "b")]
    assert names[0] == names[1] == ["frame_sample", "frame_sample_pixels"]
    sample = [np.load(str(tmp_path / d / "frame_sample.npy")) for d in ("a", "b")]
    pixels = [np.load(str(tmp_path / d / "frame_sample_pixels.npy")) for d in ("a", "b")]
    assert sample[0].dtype == np.float32 and pixels[0].dtype == np.float64
    assert np.array_equal(sample[0], sample[1]) and np.array_equal(pixels[0], pixels[1])
    assert sample[0].nbytes + pixels[0].nbytes <= limit and len(np.unique(pixels[0])) == len(pixels[0]) > 0
    assert np.array_equal(sample[0], frame.reshape(-1, 3)[pixels[0].astype(np.int64)])
