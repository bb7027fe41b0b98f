"""Runs tests/init_dropin/harness (the drop-in ORB_SLAM::Initializer on the GPU) or harness_host (the same class over the host route) on one scene and
reads its answer; the angles between two motions; which recordings of the reference's decision are clear.  Test infrastructure."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU, HOST = (os.path.join(ROOT, "tests", "init_dropin", n) for n in ("harness", "harness_host"))


def run(exe, workdir, k1, k2, vMatches12, intr, sigma, iters, sets=None, reps=0):
    """-> dict(ok, model, bestH, bestF, nInliers, chosen, nhyp, SH, SF, RH, nGood, parallax, R21, t21, vbTriangulated, vP3D, sets[, timing])"""
    n1, n2 = len(k1), len(k2)
    fin, fout = os.path.join(str(workdir), "init_in.bin"), os.path.join(str(workdir), "init_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([*intr, sigma], np.float32).tobytes())
        f.write(np.array([iters, n1, n2, 0 if sets is None else 1], np.int32).tobytes())
        f.write(np.ascontiguousarray(k1).tobytes()); f.write(np.ascontiguousarray(k2).tobytes())
        f.write(np.ascontiguousarray(vMatches12, np.int32).tobytes())
        if sets is not None:
            f.write(np.ascontiguousarray(sets, np.int32).tobytes())
    p = subprocess.run([exe, fin, fout] + ([str(reps)] if reps else []), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-2000:]
    b = open(fout, "rb").read()
    o = [0]

    def take(dt, n):
        a = np.frombuffer(b, dt, n, o[0]); o[0] += a.nbytes
        return a.copy()
    head, sc, ng, pl, Rt = take(np.int32, 7), take(np.float32, 3), take(np.int32, 8), take(np.float32, 8), take(np.float32, 12)
    tri, P, used = take(np.uint8, n1), take(np.float32, n1 * 3).reshape(n1, 3), take(np.int32, iters * 8).reshape(iters, 8)
    assert o[0] == len(b)
    r = dict(ok=int(head[0]), model=chr(head[1]) if head[1] else "", bestH=int(head[2]), bestF=int(head[3]), nInliers=int(head[4]), chosen=int(head[5]),
             nhyp=int(head[6]), SH=sc[0], SF=sc[1], RH=sc[2], nGood=ng, parallax=pl, R21=Rt[:9].reshape(3, 3), t21=Rt[9:], vbTriangulated=tri, vP3D=P, sets=used)
    if reps:
        w = p.stdout.split()
        r["timing"] = {w[i]: float(w[i + 1]) for i in range(0, len(w) - 1, 2)}
    return r


def angles(R_a, t_a, R_b, t_b):
    """(the rotation angle of R_a R_b', the angle between the directions t_a and t_b), in degrees"""
    Ra, Rb = np.asarray(R_a, np.float64).reshape(3, 3), np.asarray(R_b, np.float64).reshape(3, 3)
    c = (np.trace(Ra @ Rb.T) - 1) / 2
    ta, tb = np.asarray(t_a, np.float64).ravel(), np.asarray(t_b, np.float64).ravel()
    d = ta @ tb / (np.linalg.norm(ta) * np.linalg.norm(tb))
    return float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.degrees(np.arccos(np.clip(d, -1, 1))))


def unclear(z, min_parallax=1.0, min_triangulated=50):
    """why the recorded decision of one scene could turn on a last bit (empty: the recording is clear): RH within 0.02 of 0.40, an nGood comparison
    within 2 counts of its threshold, the parallax within 0.05 degrees of minParallax"""
    why = []
    if abs(float(z["RH"]) - 0.40) <= 0.02:
        why.append("RH")
    n, N = int(z["nhyp"]), int(z["nInliers"])
    g, p = z["nGood"][:n].astype(int), z["parallax"][:n]
    if n == 0:
        return why
    if chr(int(z["model"])) == "F":
        mx = g.max()
        if abs(mx - max(int(0.9 * N), min_triangulated)) <= 2:
            why.append("maxGood against nMinGood")
        if any(abs(x - 0.7 * mx) <= 2 for x in g if x != mx) or (g == mx).sum() > 1:
            why.append("nsimilar")
        if abs(float(p[int(np.argmax(g))]) - min_parallax) <= 0.05:
            why.append("parallax")
    else:
        order = np.sort(g)[::-1]
        best, second = order[0], order[1]
        if abs(second - 0.75 * best) <= 2:
            why.append("secondBestGood")
        if abs(best - min_triangulated) <= 2 or abs(best - 0.9 * N) <= 2:
            why.append("bestGood")
        if abs(float(p[int(np.argmax(g))]) - min_parallax) <= 0.05:
            why.append("parallax")
    return why
