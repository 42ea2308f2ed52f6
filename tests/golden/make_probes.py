"""Writes tests/golden/probe_volume.npz: what the REAL reference (oracle/_ref, built by __graft_entry__.build()) answers for the rays of the
pinned probe volume of tests/probe_sets.py -- 2 x 2 x 2 probes of 64 rays in the HW11-like room, 512 rays: the rays (the numpy restatement
of csrc/probe_rule.h) and shootRay's colours for them as REFLECTION rays at MAX_DEPTH 5.  Data only.
Run from the repository root: python tests/golden/make_probes.py"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import probe_sets as ps  # noqa: E402
from oracle import oracle_api as oa  # noqa: E402


def main():
    pkg = importlib.import_module("course-assignment-danielhalachev_amd")
    scenes = pkg.scenes
    blob = scenes.to_blob(ps.room(scenes))
    v = ps.Volume(**ps.PIN_VOLUME)
    rays, _ = ps.rays_and_keys(v, 0, v.count)
    rgb = oa.reference_shoot(blob, rays, 2, 5).astype(np.float32)
    print(len(rays), "rays; mean colour", rgb.mean(axis=0))
    np.savez_compressed(os.path.join(HERE, "probe_volume.npz"), rays=rays, rgb=rgb)


if __name__ == "__main__":
    main()
