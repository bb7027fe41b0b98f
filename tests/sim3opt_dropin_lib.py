"""Drives the drop-in ORB_SLAM::Sim3Optimizer through tests/sim3opt_dropin/harness (the GPU) or harness_host (the same class over
tools/libsim3opt_host.so) and states what it is held to.  The class adds the walk of Optimizer.cc:844-923 on the host: the pairs are the matches that
pass the NULL, isBad and GetIndexInKeyFrame tests, their points are R*Pw + t in float as a cv::Mat product accumulates it (restated here in
float32), side 1's weight is GetInvSigma2 and side 2's is GetSigma2.  So every candidate must come back with what tests/sim3opt_checks.py holds the C
ABI to for those pairs: the return value, the similarity, and vpMatches1 cleared exactly at the removed pairs, every other entry (a NULL match, a
NULL or bad point on either side, a point key frame 2 does not observe) left as it was.  ToCvMat and Compose are held to numpy."""
import os
import struct
import subprocess

import numpy as np

import sim3opt_checks as ck
import sim3opt_ref as ref
import sim3opt_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA2 = np.array(sc.LEVEL_SIGMA2, np.float32)


def pose(rng):
    a = rng.randn(3)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = sc.rodrigues(0.2 * a / np.linalg.norm(a)).astype(np.float32)
    T[:3, 3] = rng.uniform(-1, 1, 3).astype(np.float32)
    return T


def to_camera(T, Xw):
    """R*Xw + t as cv::Mat computes it in float: s = 0; s += R[y][k]*X[k] in k order; s + t[y]"""
    out = np.zeros((len(Xw), 3), np.float32)
    for y in range(3):
        s = np.zeros(len(Xw), np.float32)
        for k in range(3):
            s = (s + (T[y, k] * Xw[:, k]).astype(np.float32)).astype(np.float32)
        out[:, y] = (s + T[y, 3]).astype(np.float32)
    return out


def world(T, Pc):
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    return ((Pc.astype(np.float64) - t) @ R).astype(np.float32)


class Case:
    """one key frame 1 with the candidates built from variants of ONE scene (they share its points and its key points)"""

    def __init__(self, s, variants, seed):
        rng = np.random.RandomState(seed + 11)
        n = s["n"]
        self.s, self.n = s, n
        self.T1 = pose(rng)
        self.nkeys1 = n + 8
        self.where = np.sort(rng.permutation(self.nkeys1)[:n])
        self.Xw1 = world(self.T1, s["P1c"])
        rest = [k for k in range(self.nkeys1) if k not in set(self.where.tolist())]
        # the eight other key points: what the walk must skip and leave alone (has1, bad1, match, idx2 >= 0, bad2)
        kinds = [(1, 0, 0, 1, 0), (0, 0, 1, 1, 0), (1, 1, 1, 1, 0), (1, 0, 1, 1, 1), (1, 0, 1, 0, 0), (0, 0, 0, 1, 0), (1, 0, 0, 1, 0), (1, 1, 1, 0, 1)]
        self.other = dict(zip(rest, kinds))
        self.cands = []
        for th2, start_seed in variants:
            T2 = pose(rng)
            S12 = s["S12"] if start_seed is None else self._start(s, start_seed)
            perm = rng.permutation(n + 5)[:n]
            self.cands.append(dict(T2=T2, th2=th2, S12=np.asarray(S12, np.float32), perm=perm, Xw2=world(T2, s["P2c"])))

    @staticmethod
    def _start(s, seed):
        rng = np.random.RandomState(seed)
        a = rng.randn(3)
        R0 = sc.rodrigues(0.015 * a / np.linalg.norm(a)) @ s["R"]
        return np.concatenate([R0.astype(np.float32).reshape(9), (s["t"] + 0.01 * rng.randn(3)).astype(np.float32), [np.float32(s["s"] * 1.01)]])

    def blob(self, mode):
        s, n = self.s, self.n
        edge_of = {int(k): i for i, k in enumerate(self.where)}
        out = [struct.pack("<iii", len(self.cands), mode, len(SIGMA2)), SIGMA2.tobytes(), np.asarray(s["cam1"], np.float32).tobytes(), self.T1.tobytes(),
               struct.pack("<i", self.nkeys1)]
        for k in range(self.nkeys1):
            i = edge_of.get(k)
            if i is None:
                has1, bad1 = self.other[k][0], self.other[k][1]
                out.append(struct.pack("<ffiiifff", 100.0 + k, 50.0 + k, 1, has1, bad1, 0.5, 0.5, 4.0))
            else:
                out.append(np.asarray(s["obs1"][i, :2], np.float32).tobytes() + struct.pack("<iii", int(s["oct1"][i]), 1, 0) + self.Xw1[i].tobytes())
        for c in self.cands:
            out.append(np.asarray(s["cam2"], np.float32).tobytes() + c["T2"].tobytes() + struct.pack("<f", c["th2"]) + c["S12"].tobytes())
            nkeys2 = n + 5
            uv2 = np.zeros((nkeys2, 2), np.float32)
            oct2 = np.ones(nkeys2, np.int32)
            uv2[c["perm"]] = s["obs2"][:, :2]
            oct2[c["perm"]] = s["oct2"]
            out.append(struct.pack("<i", nkeys2))
            for j in range(nkeys2):
                out.append(uv2[j].tobytes() + struct.pack("<i", int(oct2[j])))
            for k in range(self.nkeys1):
                i = edge_of.get(k)
                if i is None:
                    _, _, match, seen, bad2 = self.other[k]
                    out.append(struct.pack("<iiifff", match, 0 if seen else -1, bad2, 0.4, 0.4, 5.0))
                else:
                    out.append(struct.pack("<iii", 1, int(c["perm"][i]), 0) + c["Xw2"][i].tobytes())
        return b"".join(out)

    def expected(self, c, narrowed=False):
        """the restatement on the pairs the walk must produce; narrowed: the start the template overload hands over (toRotationMatrix(q), t, s to float)"""
        s = self.s
        P1, P2 = to_camera(self.T1, self.Xw1), to_camera(c["T2"], c["Xw2"])
        S12 = c["S12"]
        if narrowed:
            q, t, sc_ = ref.sim3_from_float(S12)
            S12 = np.concatenate([np.array(ref.po.to_rotation_matrix(q)).astype(np.float32).reshape(9), np.array(t, np.float32), [np.float32(sc_)]])
        r = ref.optimize_sim3(s["cam1"], s["cam2"], c["th2"], P1, P2, s["obs1"], s["obs2"], S12)
        if r["ret0"]:                                       # g2oS12 untouched: the state the harness built from the ORIGINAL floats
            q, t, sc_ = ref.sim3_from_float(c["S12"])
            r.update(q=np.array(q), t=np.array(t), s=sc_, S12=ref.to_cvmat((q, t, sc_)))
        return r


def run(harness, case, mode, tmp_path):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(case.blob(mode))
    r = subprocess.run([os.path.join(ROOT, "tests", "sim3opt_dropin", harness), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    raw = open(dst, "rb").read()
    off, out = 0, []
    for c in case.cands:
        head = struct.unpack_from("<5i", raw, off); off += 20
        sim = np.frombuffer(raw, np.float64, 8, off); off += 64
        M = np.frombuffer(raw, np.float32, 16, off).reshape(4, 4); off += 64
        C = np.frombuffer(raw, np.float32, 16, off).reshape(4, 4); off += 64
        fl = np.frombuffer(raw, np.uint8, case.nkeys1, off); off += case.nkeys1
        out.append(dict(head=head, q=sim[:4], t=sim[4:7], s=sim[7], M=M, C=C, kept=fl.astype(bool), raw=raw))
    assert off == len(raw)
    return out


def check(case, c, got, r, batched=False):
    nIn, ncorr, nbad, ret0, ncalls = got["head"]
    assert nIn == r["nin"] and ncalls == 1, (got["head"], r["nin"])                           # the batched form is ONE call for every candidate
    if not batched:                                                                           # the report is that of a call's first candidate
        assert ncorr == r["ncorr"] == case.n and nbad == r["nbad"] and ret0 == r["ret0"], (got["head"], r["nbad"])
    assert np.array_equal(~got["kept"][case.where], r["removed"])                              # vpMatches1 cleared exactly at the removed pairs
    for k, (has1, bad1, match, seen, bad2) in case.other.items():
        assert got["kept"][k] == bool(match), k                                               # everything the walk skips stays as it was
    d = max(np.abs(got["q"] - r["q"]).max(), np.abs(got["t"] - r["t"]).max(), abs(got["s"] - r["s"]))
    assert d <= ck.TOL_SIM, d
    assert ck.ulp_distance(got["M"][:3], r["S12"][:3]).max() <= 1.0 and list(got["M"][3]) == [0.0, 0.0, 0.0, 1.0]     # ToCvMat
    S = (list(got["q"]), list(got["t"]), float(got["s"]))
    Smw = ref.sim3_from_float(np.concatenate([c["T2"][:3, :3].reshape(9), c["T2"][:3, 3], [np.float32(1.0)]]))
    assert ck.ulp_distance(got["C"][:3], ref.to_cvmat(ref.sim3_mul(S, Smw))[:3]).max() <= 1.0                         # Compose (LoopClosing.cc:328-330)


def scenario(harness, tmp_path, name="n65"):
    """three candidates of one key frame (th2 = 10, th2 = 5, another start): one by one, through the template overload, and as one batched call"""
    s = sc.named(name)
    case = Case(s, [(10.0, None), (5.0, None), (10.0, 4242)], seed=s["seed_used"])
    single = run(harness, case, 0, tmp_path)
    for c, got in zip(case.cands, single):
        check(case, c, got, case.expected(c))
    templ = run(harness, case, 2, tmp_path)
    for c, got in zip(case.cands, templ):
        check(case, c, got, case.expected(c, narrowed=True))
    batched = run(harness, case, 1, tmp_path)
    for c, got, one in zip(case.cands, batched, single):
        check(case, c, got, case.expected(c), batched=True)
        assert got["head"][0] == one["head"][0] and got["q"].tobytes() == one["q"].tobytes() and got["t"].tobytes() == one["t"].tobytes()
        assert got["s"] == one["s"] and got["kept"].tobytes() == one["kept"].tobytes() and got["M"].tobytes() == one["M"].tobytes()
    return case, single
