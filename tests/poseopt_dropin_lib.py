"""Drives the drop-in ORB_SLAM::PoseOptimizer through tests/poseopt_dropin/harness (the GPU) or harness_host (the same class over
tools/libposeopt_host.so) and states what it is held to: the class adds no arithmetic of its own past `1 / mvLevelSigma2[octave]`, so every frame must
come back with what tests/poseopt_checks.py holds the C ABI to for the scene's edges: the return value, mTcw, and mvbOutlier carried from the compact
edges back to the key points past the NULL map points interleaved among them (whose flags the call must leave alone)."""
import os
import struct
import subprocess

import numpy as np

import poseopt_checks as ck
import poseopt_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEVELS = 8


def frame_blob(s, seed):
    """-> (bytes of one frame for the harness, `where`: the key point of every edge, nkeys)"""
    rng = np.random.RandomState(seed + 5)
    n = s["n"]
    nkeys = n + n // 2 + 3
    where = np.sort(rng.permutation(nkeys)[:n])
    T = np.eye(4, dtype=np.float32)
    T[:3] = s["Tcw"]
    out = [T.tobytes(), struct.pack("<i", nkeys)]
    edge_of = {int(k): i for i, k in enumerate(where)}
    for k in range(nkeys):
        i = edge_of.get(k)
        if i is None:
            out.append(struct.pack("<ffiifff", rng.uniform(0, 640), rng.uniform(0, 480), int(rng.randint(0, NLEVELS)), 0, 0.0, 0.0, 0.0))
        else:
            out.append(np.asarray(s["uv"][i], np.float32).tobytes() + struct.pack("<ii", int(s["level"][i]), 1) + np.asarray(s["xyz"][i], np.float32).tobytes())
    return b"".join(out), where, nkeys


def run(harness, names, mode, tmp_path):
    scenes = [sc.named(nm) for nm in names]
    lv = (np.float32(1.2) ** np.arange(NLEVELS, dtype=np.float32)).astype(np.float32)
    sigma2 = (lv * lv).astype(np.float32)
    blobs = [frame_blob(s, p) for p, s in enumerate(scenes)]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<iii", len(scenes), mode, NLEVELS) + np.asarray(sc.CAM, np.float32).tobytes() + sigma2.tobytes() + b"".join(b[0] for b in blobs))
    r = subprocess.run([os.path.join(ROOT, "tests", "poseopt_dropin", harness), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    raw = open(dst, "rb").read()
    off, out = 0, []
    for s, (blob, where, nkeys) in zip(scenes, blobs):
        head = struct.unpack_from("<5i", raw, off); off += 20
        T = np.frombuffer(raw, np.float32, 16, off).reshape(4, 4); off += 64
        fl = np.frombuffer(raw, np.uint8, nkeys, off); off += nkeys
        out.append((s, head, T, fl, where))
    assert off == len(raw)
    return out


def scenario(harness, tmp_path, names=("n10", "n65", "n130")):
    """three scenes one by one and as one batched call: both against the restatement, and the batched call equal to the single ones"""
    single = run(harness, names, 0, tmp_path)
    batched = run(harness, names, 1, tmp_path)
    for (s, head, T, fl, where), (s2, head2, T2, fl2, where2) in zip(single, batched):
        r = s["ref"]
        assert np.array_equal((np.float32(1.0) / s["sigma2"]).astype(np.float32), s["inv_sigma2"])      # what the class computes from mvLevelSigma2
        good, ninit, nbad, rounds, calls = head
        assert good == r["ninitial"] - r["nbad"] and ninit == s["n"] and nbad == r["nbad"] and rounds == r["rounds"] and calls == 1
        assert np.array_equal(fl[where].astype(bool), r["outlier"])              # mvbOutlier back at the key points of the edges
        rest = np.ones(len(fl), bool)
        rest[where] = False
        assert fl[rest].all()                                                     # a key point without a map point keeps its flag
        assert ck.ulp_distance(T[:3], r["Tcw"][:3]).max() <= 1.0 and list(T[3]) == [0.0, 0.0, 0.0, 1.0]
        assert head2[0] == good and T2.tobytes() == T.tobytes() and fl2.tobytes() == fl.tobytes() and head2[4] == 1
