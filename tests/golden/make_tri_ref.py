#!/usr/bin/env python3
"""Records the REFERENCE's own ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:852-1014, through ref_search_for_triangulation of
oracle/_ref/libref_orbmatcher.so: the reference translation unit compiled where it lies against plain-data stand-ins) on the scenes of
tests/tri_rows_scenes.py -> tests/golden/tri_ref_<name>.npz.  Needs the reference tree (build container only); re-run only on purpose.
Procedure and contents: tests/golden/tri_ref.md."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import tri_rows_scenes as ts
import test_ref_pin_matcher as rp            # its ctypes prototypes of the reference wrappers

P = lambda a: a.ctypes.data
HERE = os.path.dirname(os.path.abspath(__file__))
for name, check in ts.SCENES:
    r1, r2, F = ts.scene(ts.scene_seed(name))
    (n1_, o1, f1), (n2_, o2, f2) = r1["fv"], r2["fv"]
    n1, n2 = len(r1["desc"]), len(r2["desc"])
    q2t = np.zeros(n1, np.int32)
    n = rp.ref().ref_search_for_triangulation(0.6, check, P(F), P(ts.SIGMA2), len(ts.SIGMA2), P(n1_), P(o1), P(f1), len(n1_), P(r1["kps"]), P(r1["desc"]),
                                              P(r1["has_mp"]), n1, P(n2_), P(o2), P(f2), len(n2_), P(r2["kps"]), P(r2["desc"]), P(r2["has_mp"]), n2, P(q2t))
    assert n >= 0, n
    ts.save_scene(os.path.join(HERE, "tri_ref_%s.npz" % name), name, r1, r2, F, q2t, n)
    print(name, check, n1, n2, "unsorted nodes", ts.unsorted_nodes(r1["fv"]), ts.unsorted_nodes(r2["fv"]), "matches", n)
