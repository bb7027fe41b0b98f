#!/usr/bin/env python3
"""Records the REFERENCE's own ORBmatcher::SearchByBoW (both overloads, src/ORBmatcher.cc:155-281 and :715-850, through
oracle/_ref/libref_orbmatcher.so: the reference translation unit compiled where it lies against plain-data stand-ins) on the scenes of
tests/bow_rows_scenes.py -> tests/golden/bow_ref_<name>.npz.  Needs the reference tree (build container only); re-run only on purpose.
Procedure and contents: tests/golden/bow_ref.md."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bow_rows_scenes as bs
import test_ref_pin_matcher as rp            # its ctypes prototypes of the reference wrappers

P = lambda a: a.ctypes.data
HERE = os.path.dirname(os.path.abspath(__file__))
for name, form, check, ratio in bs.SCENES:
    r1, r2 = bs.scene(bs.scene_seed(name))
    (n1_, o1, f1), (n2_, o2, f2) = r1["fv"], r2["fv"]
    n1, n2 = len(r1["desc"]), len(r2["desc"])
    if form == "f":
        res = np.zeros(n2, np.int32)
        n = rp.ref().ref_search_by_bow(ratio, check, P(n1_), P(o1), P(f1), len(n1_), P(r1["desc"]), P(r1["angle"]), P(r1["state"]), n1,
                                       P(n2_), P(o2), P(f2), len(n2_), P(r2["desc"]), P(r2["angle"]), n2, P(res))
    else:
        res = np.zeros(n1, np.int32)
        n = rp.ref().ref_search_by_bow_kf(ratio, check, P(n1_), P(o1), P(f1), len(n1_), P(r1["desc"]), P(r1["angle"]), P(r1["state"]), n1,
                                          P(n2_), P(o2), P(f2), len(n2_), P(r2["desc"]), P(r2["angle"]), P(r2["state"]), n2, P(res))
    bs.save_scene(os.path.join(HERE, "bow_ref_%s.npz" % name), name, r1, r2, res, n)
    print(name, form, check, ratio, n1, n2, "matches", n)
