"""Records tests/golden/fuse_ref_*.npz from the reference's own ORBmatcher::Fuse (tests/golden/fuse_ref.md).  Needs
oracle/_ref/libref_orbmatcher.so, which the build makes only where the reference tree is present; run from the repository root:
    python tests/golden/make_fuse_ref.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import fuse_scenes as fs  # noqa: E402
import test_ref_pin_matcher as rpm  # noqa: E402


def main():
    L = rpm.load(rpm.PATH)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for name, args in fs.REF_SCENES.items():
        sc = fs.ref_scene(*args)
        fused = fs.ref_fuse_each(L, sc)
        want = fs.restate(sc)
        assert np.array_equal(fused, want["best_idx"]), name            # the restatement agreed when the file was made; the file holds the reference's
        v, p, b = sc["view"], sc["pts"], sc["b"]
        np.savez_compressed(os.path.join(HERE, "fuse_ref_%s.npz" % name), Rcw=bits(v["Rcw"]), tcw=bits(v["tcw"]), Ow=bits(v["Ow"]),
                            intr=bits([v["fx"], v["fy"], v["cx"], v["cy"]]), bounds=np.array([b.min_x, b.max_x, b.min_y, b.max_y], np.int32),
                            grid_inv=bits([b.inv_w, b.inv_h]), th=bits([sc["th"]]), factors=bits(sc["factors"]), kps=sc["kps"].view(np.uint8).reshape(-1, 28),
                            desc=sc["desc"], cell_off=sc["off"], cell_feat=sc["feat"], pos=bits(p["pos"]), min_dist=bits(p["dmin"]), qdesc=p["desc"],
                            qstate=sc["qstate"], fused=fused)
        print(name, "points", len(fused), "fused", int((fused >= 0).sum()), "statuses", np.bincount(want["status"], minlength=8).tolist())


if __name__ == "__main__":
    main()
