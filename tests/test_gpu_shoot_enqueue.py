"""Radiance queries with no host wait on the GPU (include/crt_hip.h: crt_shoot_rays_enqueue, crt_shoot_rays_gi_enqueue): the colours and
numbers of the synchronous device calls, bit for bit, from a call that only enqueues -- called directly, and captured into a graph and
replayed.  The scenes, ray sets and the oracle's colours are those of tests/test_gpu_shoot_rays.py (tests/shoot_sets.py: made once, shared with it)."""
import ctypes as C

import numpy as np
import pytest

import query_sets as qs
import shoot_sets as sh
from helpers import assert_same_floats, level_rays, make, same_bits
from shoot_gi_sets import case as gi_case, gi_options
from shoot_sets import case

pytestmark = pytest.mark.gpu
SCENES = ["hw08", "hw11", "hw12", "hw14"]


def numbers(st):
    """(levels, level_rays, shadow_records, rerouted) of a ShootStats or a ShootReport"""
    return (st.levels, level_rays(st), st.shadow_records, st.rerouted)


class Device:
    """The device arrays of n rays: rays, colours (one row more, which must stay untouched) and a report"""

    def __init__(self, pkg, rays, keys=None):
        import torch
        self.pkg, self.torch, self.n = pkg, torch, len(rays)
        self.rays = torch.from_numpy(np.array(rays)).cuda()
        self.keys = torch.from_numpy(np.array(keys).view(np.int32)).cuda() if keys is not None else None
        self.rgb = torch.full((self.n + 1, 3), float("nan"), dtype=torch.float32, device="cuda")
        self.rep = torch.full((C.sizeof(pkg.ShootReport),), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def colours(self):
        self.torch.cuda.synchronize()
        rgb = self.rgb.cpu().numpy()
        assert np.all(np.isnan(rgb[self.n:])), "written past the end"
        return rgb[:self.n]

    def report(self):
        self.torch.cuda.synchronize()
        return self.pkg.ShootReport.from_buffer_copy(self.rep.cpu().numpy().tobytes())

    def clear(self):
        self.rgb.fill_(float("nan"))
        self.rep.fill_(0xEE)
        self.torch.cuda.synchronize()


def synchronous(tracer, d, depth, **more):
    """crt_shoot_rays_device: colours, shoot_stats and query_stats -- the yardstick, and the call that sizes the context"""
    d.clear()
    tracer.shoot_rays_device(d.rays.data_ptr(), d.n, d.rgb.data_ptr(), max_depth=depth, **more)
    rgb = d.colours().copy()
    return rgb, tracer.shoot_stats(), tracer.query_stats()


def enqueue(tracer, d, depth, level_cap=None, **more):
    """crt_shoot_rays_enqueue on the default stream: colours and the device's report"""
    d.clear()
    tracer.shoot_rays_enqueue(d.rays.data_ptr(), d.n, d.rgb.data_ptr(), max_depth=depth, level_cap=level_cap, d_report_ptr=d.rep.data_ptr(), **more)
    return d.colours().copy(), d.report()


def check_equal_to_synchronous(pkg, tracer, rays, depth, what, want=None):
    d = Device(pkg, rays)
    sync, st, qst = synchronous(tracer, d, depth)
    got, rep = enqueue(tracer, d, depth)
    print("%s: levels %d level_rays %s hits %d shadow_records %d rerouted %d overflow %d dropped %d" % (
        what, rep.levels, level_rays(rep)[:rep.levels], rep.hits, rep.shadow_records, rep.rerouted, rep.overflow, rep.dropped))
    same_bits(got, sync, what + ": the synchronous call's colours")
    if want is not None:
        assert_same_floats(got, want, what + ": the oracle's colours")
    assert numbers(rep) == numbers(st) and rep.hits == qst.hits and (rep.overflow, rep.dropped) == (0, 0), what
    st2, qst2, host = tracer.shoot_stats(), tracer.query_stats(), tracer.shoot_report()
    assert (st2.rays,) + numbers(st2) == (len(rays),) + numbers(st) and st2.kernel_ms > 0, what + ": shoot_stats after the enqueue call"
    assert (qst2.rays, qst2.hits, qst2.rerouted) == (qst.rays, qst.hits, qst.rerouted), what + ": query_stats after the enqueue call"
    assert bytes(host) == bytes(rep), what + ": crt_get_shoot_report is the device's report"
    return st


# ---- 1. equals the synchronous call
@pytest.mark.parametrize("name", SCENES)
def test_equals_the_synchronous_call(pkg, scenes, oracle, name, tmp_path_factory):
    c = case(pkg, scenes, oracle, name, tmp_path_factory)
    st = check_equal_to_synchronous(pkg, c["tracer"], c["rays"], c["depth"], name, c["want"])
    if name in ("hw11", "hw14"):   # condition on the input: the levels below level 0 must not be empty
        assert level_rays(st)[1] > 0


# ---- 2. launch shapes
def test_launch_shapes(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw14", tmp_path_factory)
    rays = sh.shaped_rays(c["scene"])
    for n in (1, 63, 64, 65, 257, 4096):
        check_equal_to_synchronous(pkg, c["tracer"], rays[:n], c["depth"], "first %d rays" % n)


# ---- 3. the chunk loop: a level in several launches, the last one partly filled
def test_chunk_loop(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw14", tmp_path_factory)
    tracer = c["tracer"]
    try:
        tracer.set_query_chunks(launch_rays=256)
        st = check_equal_to_synchronous(pkg, tracer, c["rays"], c["depth"], "hw14, 256 rays a launch", c["want"])
        lr = level_rays(st)
        assert any(lr[g] > 256 and lr[g] % 256 for g in range(1, st.levels)), "no level below level 0 spans two launches: %s" % lr[:st.levels]
    finally:
        tracer.set_query_chunks()


# ---- 4. levels that run dry: every deeper launch is made, for no ray
def test_levels_run_dry(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw08", tmp_path_factory)
    tracer, rays = c["tracer"], c["rays"]
    d = Device(pkg, rays)
    sync, st, _ = synchronous(tracer, d, 8)
    got, rep = enqueue(tracer, d, 8, level_cap=[0] + [4096] * 8)
    assert st.levels == 1 and numbers(rep) == numbers(st) and (rep.overflow, rep.dropped) == (0, 0)
    same_bits(got, sync, "hw08 at max_depth 8")
    assert_same_floats(got, c["want"], "hw08 at max_depth 8: no ray recurses, so the colours are those of the scene's depth")


# ---- 5. overflow is reported, bounded and harmless
def test_overflow_is_reported_bounded_and_harmless(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw14", tmp_path_factory)
    tracer, depth = c["tracer"], c["depth"]
    rays = sh.aimed_rays(c["scene"])
    assert np.array_equal(rays, c["rays"][4096:])
    want = c["want"][4096:]
    d = Device(pkg, rays)
    sync, st, _ = synchronous(tracer, d, depth)
    lr = level_rays(st)
    assert lr[1] > 64, "condition on the input: level 1 must be wider than the capacity"
    got, rep = enqueue(tracer, d, depth, level_cap=[0, 64] + [1 << 20] * (depth - 1))   # (no exception: the return code is CRT_OK)
    print("overflow: synchronous level_rays %s; with 64 rays at level 1: %s dropped %d overflow %d" % (
        lr[:st.levels], level_rays(rep)[:rep.levels], rep.dropped, rep.overflow))
    assert rep.overflow == 1 and rep.dropped >= lr[1] - 64 and level_rays(rep)[1] == 64 and level_rays(rep)[0] == len(rays)
    final = ~np.isin(sh.first_hit_types(pkg, c["oracle"], c["scene"], rays), sh.RECURSING)
    assert 10 < int(final.sum()) < len(rays)
    assert_same_floats(got[final], want[final], "rays whose first hit does not recurse")
    assert tracer.shoot_stats().levels == rep.levels and tracer.shoot_report().overflow == 1
    again, rep = enqueue(tracer, d, depth)
    same_bits(again, sync, "NULL capacities after the overflow")
    assert numbers(rep) == numbers(st) and (rep.overflow, rep.dropped) == (0, 0)


# ---- 6. a fresh context has no room below level 0
def test_a_fresh_context_has_no_room(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer = make(pkg, scenes, oracle, c["scene"], c["folder"])[0]
    assert tracer.query_scratch_generation() == 0
    d = Device(pkg, c["rays"])
    got, rep = enqueue(tracer, d, c["depth"])
    assert rep.overflow == 1 and rep.dropped > 0 and rep.levels == 1 and level_rays(rep)[:2] == [len(c["rays"]), 0]
    final = ~np.isin(sh.first_hit_types(pkg, c["oracle"], c["scene"], c["rays"]), sh.RECURSING)
    assert_same_floats(got[final], c["want"][final], "rays whose first hit does not recurse")
    assert tracer.query_scratch_generation() > 0


# ---- 7. graph capture and replay: one capture, two replays
def test_graph_capture_and_replay(pkg, scenes, oracle, tmp_path_factory):
    import torch
    c = case(pkg, scenes, oracle, "hw14", tmp_path_factory)
    tracer, depth, rays = c["tracer"], c["depth"], c["rays"]
    sets = [np.ascontiguousarray(rays[:2048]), np.ascontiguousarray(rays[-2048:])]
    synchronous(tracer, Device(pkg, rays), depth)   # sizes the context for every subset of the rays
    refs = []
    for s in sets:
        host = tracer.shoot_rays(s, max_depth=depth)
        refs.append((host, tracer.shoot_stats()))
    assert level_rays(refs[0][1])[1] != level_rays(refs[1][1])[1] and min(level_rays(r[1])[1] for r in refs) > 0, "the sets' level-1 widths must differ"
    d = Device(pkg, sets[0])
    generation = tracer.query_scratch_generation()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tracer.shoot_rays_enqueue(d.rays.data_ptr(), d.n, d.rgb.data_ptr(), max_depth=depth, d_report_ptr=d.rep.data_ptr(),
                                  stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for s, (host, st) in zip(sets, refs):
        d.rays.copy_(torch.from_numpy(s.copy()))
        d.clear()
        graph.replay()
        torch.cuda.synchronize()
        rep = d.report()
        print("replay: levels %d level_rays %s" % (rep.levels, level_rays(rep)[:rep.levels]))
        same_bits(d.colours(), host, "a replay's colours are the host variant's")
        assert numbers(rep) == numbers(st) and (rep.overflow, rep.dropped) == (0, 0)
    assert tracer.query_scratch_generation() == generation, "the graph's pointers are still the context's"
    del graph


# ---- 8. a capture refuses what it cannot do, and stays valid
def test_capture_refuses_what_it_cannot_do(pkg, scenes, oracle, tmp_path_factory):
    import torch
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer = make(pkg, scenes, oracle, c["scene"], c["folder"])[0]
    depth = c["depth"]
    rays = np.ascontiguousarray(c["rays"][:1024])
    small = Device(pkg, rays[:64])
    synchronous(tracer, small, depth)   # a context whose scratch holds 64 rays, and no open call
    d = Device(pkg, rays)
    caps = [0] + [2048] * depth
    x = torch.zeros(8, device="cuda")
    generation = tracer.query_scratch_generation()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = x + 1
        with pytest.raises(pkg.CrtError) as e:
            tracer.shoot_rays_enqueue(d.rays.data_ptr(), d.n, d.rgb.data_ptr(), max_depth=depth, level_cap=caps, d_report_ptr=d.rep.data_ptr(),
                                      stream_ptr=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert e.value.code == pkg.CRT_ERR_INVALID and "grow" in str(e.value) and "captured" in str(e.value), str(e.value)
    graph.replay()   # the capture ended normally: the graph holds the tensor operation alone
    torch.cuda.synchronize()
    assert y.cpu().tolist() == [1.0] * 8 and tracer.query_scratch_generation() == generation
    assert np.all(np.isnan(d.rgb.cpu().numpy())), "a refused call enqueues nothing"
    sync, st, _ = synchronous(tracer, Device(pkg, rays), depth)
    generation = tracer.query_scratch_generation()
    got, rep = enqueue(tracer, d, depth, level_cap=caps)
    grown = tracer.query_scratch_generation()
    assert grown > generation, "the same call outside a capture grows the scratch"
    same_bits(got, sync, "explicit capacities")
    assert numbers(rep) == numbers(st) and rep.overflow == 0
    got, _ = enqueue(tracer, d, depth, level_cap=caps)
    same_bits(got, sync, "the same call again")
    assert tracer.query_scratch_generation() == grown, "two identical calls allocate nothing"


# ---- 9. the GI mode
def test_gi(pkg, scenes, oracle, tmp_path_factory):
    c = gi_case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, rays, keys = c["tracer"], c["rays"], c["keys"]
    opt = gi_options(pkg, 2, 2)
    d = Device(pkg, rays, keys)
    tracer.shoot_rays_gi_device(d.rays.data_ptr(), d.n, d.rgb.data_ptr(), None, qs.RAY_PRIMARY, opt)
    sync, st, qst = d.colours().copy(), tracer.shoot_stats(), tracer.query_stats()
    assert st.levels >= 2 and level_rays(st)[1] > 0
    for d_keys in (None, d.keys.data_ptr()):
        d.clear()
        tracer.shoot_rays_gi_enqueue(d.rays.data_ptr(), d.n, d.rgb.data_ptr(), d_keys, qs.RAY_PRIMARY, opt, d_report_ptr=d.rep.data_ptr())
        same_bits(d.colours(), sync, "GI colours, keys %s" % ("given" if d_keys else "NULL"))
        rep = d.report()
        assert numbers(rep) == numbers(st) and rep.hits == qst.hits and (rep.overflow, rep.dropped) == (0, 0)
        assert numbers(tracer.shoot_stats()) == numbers(st)


# ---- 10. a context without the filter
def test_without_the_filter(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer = make(pkg, scenes, oracle, c["scene"], c["folder"], tuning=dict(bvh=0))[0]
    st = check_equal_to_synchronous(pkg, tracer, c["rays"], c["depth"], "hw11 bvh=0", c["want"])
    assert st.rerouted >= st.rays and tracer.shoot_report().rerouted >= st.rays


# ---- 11. nothing else moved
def test_nothing_else_moved(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, depth = c["tracer"], c["depth"]
    frame = tracer.render(max_depth=depth).copy()
    s0 = tracer.stats()
    d = Device(pkg, c["rays"])
    sync, st, qst = synchronous(tracer, d, depth)
    for _ in range(2):
        got, _ = enqueue(tracer, d, depth)
        same_bits(got, sync, "enqueue")
    assert_same_floats(tracer.render(max_depth=depth), frame, "the frame rendered again")
    s1 = tracer.stats()
    assert (s1.fallback_frames, s1.queue_bytes, s1.queue_regrows) == (s0.fallback_frames, s0.queue_bytes, s0.queue_regrows)
    again, st2, qst2 = synchronous(tracer, d, depth)
    same_bits(again, sync, "crt_shoot_rays_device after the enqueue calls")
    assert (st2.rays,) + numbers(st2) == (st.rays,) + numbers(st) and (qst2.rays, qst2.hits) == (qst.rays, qst.hits)


# ---- 12. arguments
def test_arguments(pkg, scenes, oracle, tmp_path_factory):
    c = case(pkg, scenes, oracle, "hw11", tmp_path_factory)
    tracer, L = c["tracer"], pkg.lib()
    d = Device(pkg, c["rays"][:64])
    rays, rgb = C.c_void_p(d.rays.data_ptr()), C.c_void_p(d.rgb.data_ptr())
    opt, gi = pkg.make_options(2), pkg.make_options(2, use_gi=True)
    assert L.crt_shoot_rays_enqueue(tracer.ctx, None, 0, 9, None, None, None, None, None) == pkg.CRT_OK, "n == 0 touches nothing"
    assert L.crt_shoot_rays_gi_enqueue(tracer.ctx, None, None, 0, 9, None, None, None, None, None) == pkg.CRT_OK
    bad = [(lambda: L.crt_shoot_rays_enqueue(tracer.ctx, rays, (1 << 22) + 1, 2, C.byref(opt), rgb, None, None, None), b"2^22"),
           (lambda: L.crt_shoot_rays_gi_enqueue(tracer.ctx, rays, None, (1 << 22) + 1, 2, C.byref(gi), rgb, None, None, None), b"2^22"),
           (lambda: L.crt_shoot_rays_enqueue(tracer.ctx, rays, 64, 2, C.byref(gi), rgb, None, None, None), b"use_gi"),
           (lambda: L.crt_shoot_rays_gi_enqueue(tracer.ctx, rays, None, 64, 2, C.byref(opt), rgb, None, None, None), b"use_gi"),
           (lambda: L.crt_shoot_rays_enqueue(tracer.ctx, None, 64, 2, C.byref(opt), rgb, None, None, None), b"NULL"),
           (lambda: L.crt_shoot_rays_enqueue(tracer.ctx, rays, 64, 7, C.byref(opt), rgb, None, None, None), b"ray_type"),
           (lambda: L.crt_shoot_rays_enqueue(tracer.ctx, rays, 64, 2, C.byref(pkg.make_options(64)), rgb, None, None, None), b"max_depth")]
    for k, (call, word) in enumerate(bad):
        assert call() == pkg.CRT_ERR_INVALID, k
        assert word in L.crt_last_error(tracer.ctx), (k, L.crt_last_error(tracer.ctx))
    assert np.all(np.isnan(d.colours())), "a refused call writes nothing"
    with pytest.raises(ValueError, match="level_cap"):
        tracer.shoot_rays_enqueue(d.rays.data_ptr(), 64, d.rgb.data_ptr(), max_depth=2, level_cap=[0, 64])
