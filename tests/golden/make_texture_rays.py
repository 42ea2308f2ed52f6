"""Writes tests/golden/texture_rays.npz from the REAL reference (oracle/_ref, built by oracle/Makefile): for the texture-card scenes of
tests/texture_sets.py the scene blob, the rays and the card each is aimed at, and what the reference's textured build answered --
intersect's records (u and v included), shootRay's colours at depths 1 and 3, one 40x24 frame at depth 3 -- with the census of the
classes those rays reach, which has to meet texture_sets.check_census before anything is written.  Recorded results only.  The file is
written without timestamps, so the same reference gives the same bytes.

    python tests/golden/make_texture_rays.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import texture_sets as ts                # noqa: E402
from make_random_scenes import npz_bytes  # noqa: E402
from oracle import oracle_api as oa      # noqa: E402


def rows_differ(a, b):
    return np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))


def fixture_arrays():
    """(name -> array, census over the scenes)"""
    arrays = {"scenes": np.array(ts.SCENES), "depths": np.array(ts.DEPTHS, dtype=np.int32)}
    total = {}
    for name in ts.SCENES:
        scene = ts.make(name)
        rays, card = ts.rays(scene)
        ans = ts.reference_answers(oa, scene, rays)
        ts.add_census(total, ts.full_census(scene, card, ans))
        first, deep = ans["shoot"][ts.DEPTHS[0]], ans["shoot"][ts.DEPTHS[1]]
        rows = rows_differ(first, deep)
        for key, a in (("blob", np.frombuffer(ts.blob(scene), dtype=np.uint8)), ("rays", rays), ("card", card.astype(np.int16)), ("hits", ans["hits"]),
                       ("shoot", first), ("deep_rows", rows.astype(np.int32)), ("deep_diff", deep[rows]), ("frame", ans["frame"])):
            arrays["%s_%s" % (name, key)] = a
    ts.check_census(total)
    arrays["census"] = np.array(json.dumps(total, sort_keys=True, default=list))
    return arrays, total


def fixture_bytes():
    return npz_bytes(fixture_arrays()[0])


if __name__ == "__main__":
    oa.build()
    arrays, total = fixture_arrays()
    data = npz_bytes(arrays)
    with open(ts.GOLDEN, "wb") as f:
        f.write(data)
    print("texture_rays.npz: %d bytes; census %s" % (len(data), json.dumps(total, sort_keys=True, default=list)))
