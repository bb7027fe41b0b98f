"""Pins the numpy restatement tests/sim3solver_ref.py to recordings of the reference's own src/Sim3Solver.cc (tests/golden/sim3solver_ref.md): fed the
logged eigenvectors and rotations (the two steps include/orbh.h does not pin to OpenCV) it must match the recording bit for bit on the constructor's
arrays, the SetRansacParameters table, the truncated max errors, the drawn sets from the seeded rand(), M, N, s, t, T12, T21, every flag and count, and
the whole course of iterate over several calls."""
import numpy as np
import pytest

import sim3solver_dropin_lib as dl
import sim3solver_ref as ref

NAMES = sorted(dl.RECORDED)


def bits(a):
    """the bytes of a, every NaN as the canonical quiet NaN: which NaN an operation hands out (its sign, its payload) is the processor's choice, and
    include/orbh.h writes the canonical one"""
    a = np.ascontiguousarray(a).copy()
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a.tobytes()


@pytest.fixture(scope="module", params=NAMES)
def rec(request):
    name = request.param
    s, blob, where, nm, rseed, calls = dl.recorded_scene(name)
    return name, s, where, nm, calls, dl.load_recording(name)


def test_at_least_six_scenes_with_the_kinds_asked_for():
    assert len(NAMES) >= 6
    found = {n: not dl.load_recording(n)["call_empty"].all() for n in NAMES}
    assert found["general_1"] and found["general_04"] and found["general_27"] and found["late"]
    assert not found["all_outliers"] and not found["equal_triples"]
    z = dl.load_recording("late")
    assert z["call_empty"][0] == 1                                  # a late success: not in the first iterate(5)
    assert int(dl.load_recording("n_equals_min")["max_its"]) == 1 and 20 < int(dl.load_recording("few")["N"]) < 25


def test_constructor_arrays(rec):
    name, s, where, nm, calls, z = rec
    assert int(z["N"]) == s["N"] and int(z["mN1"]) == nm and np.array_equal(z["indices1"], where)
    for k in ("x3dc1", "x3dc2", "p1im1", "p2im2"):
        assert bits(z[k]) == bits(s[k]), k
    assert np.array_equal(z["maxerr1"], s["maxerr1"].astype(np.int64)) and np.array_equal(z["maxerr2"], s["maxerr2"].astype(np.int64))
    assert bits(z["maxerr1"].astype(np.float32)) == bits(ref.max_errors(s["sigma2_1"]))


def test_ransac_table(rec):
    name, s, where, nm, calls, z = rec
    assert len(z["ransac"]) == 45
    for p, mi, mx, want in z["ransac"]:
        assert ref.ransac_parameters(s["N"], p, int(mi), int(mx)) == int(want), (name, p, mi, mx)
    assert ref.ransac_parameters(s["N"], *dl.PARAMS) == int(z["max_its"])


def drawn_sets(z, N):
    values = iter(z["rand"][:, 0].tolist())
    return ref.draw_sets(N, len(z["count"]), lambda: next(values))


def test_the_draw(rec):
    name, s, where, nm, calls, z = rec
    for r, mx, randi in z["rand"]:
        assert ref.random_int(int(r), 0, int(mx)) == int(randi)
    assert np.array_equal(z["rand"][:, 1].reshape(-1, 3), np.tile([s["N"] - 1, s["N"] - 2, s["N"] - 3], (len(z["count"]), 1)))
    sets = drawn_sets(z, s["N"])
    assert sets.min() >= 0 and sets.max() < s["N"]
    # the seeded rand() itself: the C library's sequence after srand
    assert np.array_equal(dl.glibc_rand_sets(s["N"], len(sets), int(z["srand"])), sets)


def test_every_iteration_bit_for_bit(rec):
    name, s, where, nm, calls, z = rec
    sets = drawn_sets(z, s["N"])
    worst = 0.0
    for it in range(len(sets)):
        r = ref.fit(s["x3dc1"], s["x3dc2"], sets[it], R=z["R"][it])
        assert bits(r["M"]) == bits(z["M"][it].reshape(3, 3)), (name, it, "M")
        assert bits(r["N"]) == bits(z["Nmat"][it].reshape(4, 4)), (name, it, "N")
        for k in ("t", "T12", "T21"):
            assert bits(r[k]) == bits(z[k][it].reshape(r[k].shape)), (name, it, k)
        assert bits(r["s"]) == bits(z["s"][it]), (name, it, "s")
        fl, c = ref.check_inliers(z["T12"][it], z["T21"][it], s)
        assert c == z["count"][it] and np.array_equal(fl, z["flags"][it]), (name, it)
        # the unpinned steps, for the record: the logged quaternion rounds to the logged eigenvector; the closed form from the double quaternion against
        # the logged Rodrigues of the FLOAT axis-angle vector differs by the float rounding of the quaternion, a few 2^-24
        assert bits(z["q"][it].astype(np.float32)) == bits(z["evec"][it])
        if np.isfinite(z["R"][it]).all():
            worst = max(worst, float(np.abs(ref.rotation(z["q"][it]).astype(np.float64).reshape(9) - z["R"][it]).max()))
        else:
            assert np.isnan(ref.rotation(z["q"][it])).all() and c == 0          # norm(vec) == 0: NaN in the recording, NaN here
    print("%s: closed form against the logged Rodrigues: %.3g" % (name, worst))
    assert worst <= 16 * 2.0 ** -24
    if name == "equal_triples":
        assert np.isnan(z["R"]).all() and not z["count"].any()


def test_the_course_of_iterate(rec):
    name, s, where, nm, calls, z = rec
    N, mx, mi = s["N"], int(z["max_its"]), dl.PARAMS[1]
    hyp = dict(count=z["count"], T12=z["T12"], R=z["R"], t=z["t"], s=z["s"])
    st = ref.fresh_state(N)
    found_rows = 0
    for call in range(calls):
        done = st["iterations"]
        iters = min(5, len(z["count"]) - done)
        sub = {k: v[done:done + iters] for k, v in hyp.items()}
        res = ref.walk(N, iters, mi, mx, sub, z["flags"][done:done + iters], st)
        got = (int(z["call_empty"][call]), int(z["call_no_more"][call]), int(z["call_ninliers"][call]), int(z["call_iterations"][call]),
               int(z["call_best_inliers"][call]))
        assert got == (1 - res["found"], res["no_more"], res["ninliers"], st["iterations"], st["best_inliers"]), (name, call, got, res)
        want_fl = np.zeros(nm, np.uint8)
        want_fl[where] = res["flags"]
        assert np.array_equal(z["call_inliers"][call], want_fl), (name, call)
        if res["found"]:
            assert bits(z["call_T"][call]) == bits(res["T12"])
        if st["iterations"] and len(z["call_bestR"]):
            assert bits(z["call_bestR"][call]) == bits(st["best_R"]) and bits(z["call_bestt"][call]) == bits(st["best_t"])
            assert bits(z["call_bests"][call]) == bits(np.float32(st["best_s"]))
        found_rows += res["found"]
    assert found_rows == int((1 - z["call_empty"]).sum())
