"""tests/cull_ref.py against the recordings of the reference's own text (tests/golden/cull_ref_*.npz; golden/cull_ref.md says what they hold and
golden/make_cull_ref.md how they were made), without a GPU: the restatement and the definition over the columns both equal them in every stored
quantity, and every named case occurs."""
import collections
import functools
import os

import numpy as np
import pytest

import cull_ref as cr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_SETS = ["small", "wide"]


@functools.lru_cache(maxsize=None)
def load_set(name):
    """-> [(Scene, dict(records [(key frame, nMPs, nRed, SetBadFlag called)], kf_bad, mp_bad, mvp) as the reference left them)]"""
    z = np.load(os.path.join(GOLDEN, "cull_ref_%s.npz" % name))
    out = []
    for i in range(int(z["n"])):
        sc = cr.from_arrays({k: z["%d_s_%s" % (i, k)] for k in ("kf", "mvp", "oct", "mp", "covis", "dims")})
        g = dict(records=[(int(r[0]), int(r[1]), int(r[2]), bool(r[3])) for r in z["%d_g_records" % i]],
                 kf_bad=[bool(x) for x in z["%d_g_kf_bad" % i]], mp_bad=[bool(x) for x in z["%d_g_mp_bad" % i]],
                 mvp=[[int(x) for x in row[:len(kf.mvp)]] for row, kf in zip(z["%d_g_mvp" % i], sc.kfs)])
        out.append((sc, g))
    return out


def same(e, g):
    for key in ("records", "kf_bad", "mp_bad", "mvp"):
        assert e[key] == g[key], key


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_restatement_equals_the_recordings(name):
    scenes = load_set(name)
    assert len(scenes) >= 30
    for sc, g in scenes:
        same(cr.expected(sc), g)


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_column_definition_equals_the_recordings(name):
    """what the GPU computes and what a caller does around it for mbNotErase, stated over the columns, against the reference directly"""
    for sc, g in load_set(name):
        d = cr.dropin_by_columns(sc)
        same(d, g)
        stuck = sum(1 for k, _, _, called in g["records"] if called and not g["kf_bad"][k])     # flagged, protected by mbNotErase
        again = sum(1 for k, _, _, called in g["records"][:-1] if called and not g["kf_bad"][k])   # ... with candidates behind it: the call runs again
        assert d["calls"] == (1 + again if g["records"] else 0)
        if stuck == 0 and g["records"]:
            # then ONE call of the definition is the whole answer
            kf_slot, kf_oct, kf_nt, live = cr.columns(sc)
            nmps, nred, cull = cr.cull_by_columns(cr.candidates(sc), kf_slot, kf_oct, kf_nt, live, sc.capacity, sc.nlevels)
            assert [(n, r, bool(c)) for n, r, c in zip(nmps.tolist(), nred.tolist(), cull.tolist())] == [r[1:] for r in g["records"]]


def test_every_case_occurs():
    n = collections.Counter(c for name in GOLDEN_SETS for sc, _ in load_set(name) for c in cr.classify(sc))
    print(dict(n))
    for c in cr.CASES:
        assert n[c] >= 10, (c, dict(n))
