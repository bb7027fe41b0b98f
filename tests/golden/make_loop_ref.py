"""Records tests/golden/loop_ref_*.npz from the reference's own ORBmatcher::SearchByProjection(pKF, Scw, ...) and Fuse(pKF, Scw, ...)
(tests/golden/loop_ref.md).  Needs oracle/_ref/libref_orbmatcher.so, which the build makes only where the reference tree is present; run from
the repository root:
    python tests/golden/make_loop_ref.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import loop_ref as lr  # noqa: E402
import test_ref_pin_matcher as rpm  # noqa: E402


def main():
    L = rpm.load(rpm.PATH)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for name, args in lr.REF_SCENES.items():
        sc = lr.ref_scene(*args)
        t2q, n = lr.ref_search(L, sc)
        fused = lr.ref_fuse_each(L, sc)
        # the restatement agreed when the file was made; the file holds the reference's
        w = lr.restate_search(sc)
        got = t2q.copy(); got[got == -2] = -1
        assert n == w["nmatches"] and np.array_equal(got, w["t2pos"]), name
        assert np.array_equal(fused, lr.restate_fuse(sc)["best_idx"]), name
        v, p, b = sc["view"], sc["pts"], sc["b"]
        np.savez_compressed(os.path.join(HERE, "loop_ref_%s.npz" % name), Scw=bits(sc["Scw"]), intr=bits([v["fx"], v["fy"], v["cx"], v["cy"]]),
                            bounds=np.array([b.min_x, b.max_x, b.min_y, b.max_y], np.int32), grid_inv=bits([b.inv_w, b.inv_h]),
                            th=np.array([lr.TH_SEARCH], np.int32), th_fuse=bits([lr.TH_FUSE]), factors=bits(sc["factors"]),
                            kps=sc["kps"].view(np.uint8).reshape(-1, 28), desc=sc["desc"], cell_off=sc["off"], cell_feat=sc["feat"], pos=bits(p["pos"]),
                            min_dist=bits(p["dmin"]), qdesc=p["desc"], qstate=sc["qstate"], claimed=sc["claimed"], t2q=t2q, nmatches=np.array([n], np.int32),
                            fused=fused)
        print(name, "points", len(fused), "matched", n, "fused", int((fused >= 0).sum()), "statuses", np.bincount(w["status"], minlength=9).tolist())


if __name__ == "__main__":
    main()
