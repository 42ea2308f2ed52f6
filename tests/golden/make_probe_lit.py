"""Writes tests/golden/probe_lit.npz: what the oracle answers for the quality case of the probe-lit radiance queries (tests/probe_lit_sets.py:
quality_answers) -- the GI frame of the 48 x 32 HW11 room at 128 rays per pixel and at one, the centre rays' first
hits, their direct light, and the depth-1 GI colours of the volume's rays.  tests/test_probe_lit_host.py reads it.
usage: python tests/golden/make_probe_lit.py"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import probe_lit_sets as pl
from oracle import oracle_api

scenes = importlib.import_module("course-assignment-danielhalachev_amd").scenes
a = pl.quality_answers(scenes, oracle_api)
np.savez_compressed(os.path.join(HERE, "probe_lit.npz"), **a)
print("diffuse pixels %d of %d; RMSE probe-lit %.5f, Lbar = 0 %.5f, one ray per pixel %.5f" % ((int(a["diffuse"].sum()), len(a["diffuse"])) + pl.quality_rmse(a)))
