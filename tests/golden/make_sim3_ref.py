"""Records tests/golden/sim3_ref_*.npz from the reference's own ORBmatcher::SearchBySim3 (tests/golden/sim3_ref.md).  Needs
oracle/_ref/libref_orbmatcher.so, which the build makes only where the reference tree is present; run from the repository root, on the CPU:
    python tests/golden/make_sim3_ref.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import sim3_ref as sr  # noqa: E402
import test_ref_pin_matcher as rpm  # noqa: E402


def main():
    L = rpm.load(rpm.PATH)
    bits = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)
    for name, args in sr.REF_SCENES.items():
        sc = sr.ref_scene(*args)
        match12, n = sr.ref_search(L, sc)
        # the restatement agreed when the file was made; the file holds the reference's
        w = sr.restate(sc)
        assert n == w["nfound"] and np.array_equal(match12, w["match12"]), name
        d, b = sc["dirs"][0], sc["b"]
        side = {}
        for s, k in (("1", sc["kf1"]), ("2", sc["kf2"])):
            side.update({"kps" + s: k["kps"].view(np.uint8).reshape(-1, 28), "desc" + s: k["desc"], "cell_off" + s: k["off"], "cell_feat" + s: k["feat"],
                         "state" + s: k["state"], "pos" + s: bits(k["pos"]), "min_dist" + s: bits(k["dmin"])})
        np.savez_compressed(os.path.join(HERE, "sim3_ref_%s.npz" % name), Rt=bits(sc["Rt"]), simRt=bits(np.concatenate([sc["R12"].reshape(9), sc["t12"]])),
                            s12=bits([sc["s12"]]), th=bits([sc["th"]]), intr=bits([d["fx"], d["fy"], d["cx"], d["cy"]]),
                            bounds=np.array([b.min_x, b.max_x, b.min_y, b.max_y], np.int32), grid_inv=bits([b.inv_w, b.inv_h]), factors=bits(sc["factors"]),
                            match12=match12, nfound=np.array([n], np.int32), **side)
        print(name, "features", len(sc["kf1"]["kps"]), len(sc["kf2"]["kps"]), "found", n, "statuses 1->2", np.bincount(w["d12"]["status"], minlength=8).tolist(),
              "2->1", np.bincount(w["d21"]["status"], minlength=8).tolist())


if __name__ == "__main__":
    main()
