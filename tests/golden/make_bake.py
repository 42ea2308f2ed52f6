"""Writes tests/golden/bake_maps.npz: what the REAL reference (oracle/_ref, built by __graft_entry__.build()) answers for the probe rays of
the lightmap cases of tests/bake_sets.py on the 13x7 and 33x70 maps.  For every case and map: the covered texels' indices (row-major), their
probe rays (the numpy restatement of csrc/bake_rule.h), shootRay's colours for them as REFLECTION rays at MAX_DEPTH 5, and the count of
probes whose closest hit (the reference's intersect) is the texel's owner.  Run from the repository root: python tests/golden/make_bake.py"""
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import bake_sets as bs  # noqa: E402
from oracle import oracle_api as oa  # noqa: E402


def main():
    pkg = importlib.import_module("course-assignment-danielhalachev_amd")
    scenes = pkg.scenes
    scene = bs.make_scene(scenes)
    blob = scenes.to_blob(scene)
    out = {}
    with tempfile.TemporaryDirectory() as folder:
        hs = bs.host_scene(pkg, scenes, scene, folder)
        for name, mesh in bs.CASES.items():
            md = bs.MeshData(pkg, hs, mesh)
            for width, height in bs.MAPS[:2]:
                key = "%s_%dx%d" % (name, width, height)
                ids, rays, rec = bs.probe_rays(md, width, height)
                rgb = oa.reference_shoot(blob, rays, 2, 5)
                hits = oa.reference_trace(blob, rays, 2, textured=True)   # triangle: the index within its mesh
                own = (hits["hit"] != 0) & (hits["mesh"] == mesh) & (hits["triangle"].astype(np.int64) + int(md.tris[0]) == rec["triangle"].astype(np.int64))
                out[key + "_ids"], out[key + "_rays"], out[key + "_rgb"] = ids, rays, rgb.astype(np.float32)
                out[key + "_self"] = np.int64(own.sum())
                print(key, len(ids), "probes,", int(own.sum()), "meet their owner")
    np.savez_compressed(os.path.join(HERE, "bake_maps.npz"), **out)


if __name__ == "__main__":
    main()
