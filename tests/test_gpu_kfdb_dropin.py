"""The drop-in ORB_SLAM::KeyFrameDatabase (orb_slam_amd/cpp/KeyFrameDatabase.cc) driven through tests/kfdb_dropin/harness
against the restatement (tests/kfdb_ref.py): the recorded reference scenarios, 10,000 random operations, three threads
querying one map, and add / erase racing queries."""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import kfdb_ref as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "kfdb_dropin", "harness")


def _run(tmp_path, lines, scoring=K.L1_NORM, mode="serial", k=4, L=3):
    voc = str(tmp_path / "voc.txt")
    K.write_vocabulary(voc, k, L, scoring)
    script = str(tmp_path / "script.txt")
    with open(script, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([HARNESS, voc, script, mode], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.split("\n")[:-1]


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "kfdb_ref_*.json"))),
                         ids=lambda p: os.path.basename(p)[9:-5])
def test_recorded_scenarios(tmp_path, path):
    doc = json.load(open(path))
    assert _run(tmp_path, doc["script"], doc["scoring"]) == doc["output"]


@pytest.mark.parametrize("scoring", [K.L1_NORM, K.L2_NORM, K.CHI_SQUARE, K.BHATTACHARYYA, K.DOT_PRODUCT])
def test_random_operations(tmp_path, scoring):
    """5 x 2,000 operations: adds, erases (absent ones too), clears, both searches with repeated and fresh ids, field edits"""
    rng = np.random.default_rng(100 + scoring)
    lines = K.random_script(rng, 64, 40, 2000, dump_every=10)
    got = _run(tmp_path, lines, scoring)
    want = K.run_script(lines, scoring)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g[:300], w[:300])


def _map(rng, n_kf=120, n_words=64):
    """key frames and covisibility only (the script's final dump dropped)"""
    return K.random_script(rng, n_words, n_kf, 0, dump_every=0)[:-1]


def test_three_threads_get_the_serial_results(tmp_path):
    """loop searches with distinct query ids do not depend on each other, so any interleaving gives the serial answers"""
    rng = np.random.default_rng(3)
    lines = _map(rng) + ["add %d" % i for i in range(1, 121)]
    searches = ["loop %d %s" % (i, K.fmt_f32(rng.choice([0.0, 0.02, 0.05]))) for i in rng.permutation(np.arange(1, 121))[:90]]
    want = K.run_script(lines + searches, K.L1_NORM)
    got = _run(tmp_path, lines + searches, K.L1_NORM, mode="threads")
    assert got == ["Q %d%s" % (i, w[1:]) for i, w in enumerate(want)]
    assert sum(len(w) > 1 for w in want) > 30


def test_adds_and_erases_racing_queries_reach_the_serial_state(tmp_path):
    rng = np.random.default_rng(4)
    lines = _map(rng) + ["add %d" % i for i in range(1, 61)]       # key frames 61..120 are added while searches run
    racing = []
    for i in range(61, 121):
        racing.append("add %d" % i)
        if i % 4 == 0:
            racing.append("erase %d" % (i - 30))
        racing.append("loop %d 0" % int(rng.integers(1, 121)))
        ids = np.sort(rng.choice(64, size=12, replace=False))
        racing.append("reloc %d %s" % (5000 + i, K.bow_text(ids, np.full(12, 1 / 12))))
    final = ["loop %d 0" % (1000 + i) for i in range(1, 121)]
    kfs = ["kf %d %s" % (1000 + i, l.split(" ", 2)[2]) for i, l in enumerate(lines[:120], start=1)]   # fresh ids, same bags
    serial = lines + [l for l in racing if l.startswith(("add", "erase"))] + kfs + final
    got = _run(tmp_path, lines + ["parallel"] + racing + ["join"] + kfs + final, K.L1_NORM, mode="churn")
    want = K.run_script(serial, K.L1_NORM)
    assert got == want and sum(len(w) > 1 for w in want) > 30
