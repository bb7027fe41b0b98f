"""The launch plan of the extractor, without a GPU: every stage picks its kernel variant (template instantiation) with a pure host function
(orbx_launch.h: plan_*), which orbx_debug_plan evaluates for a described launch group.  Checked here: each row of VARIANT_CASES
(tests/variant_cases.py) plans the kernels it names, and the rows together plan EVERY variant of every stage — an instantiation added to a
launch site without a row fails test_the_table_covers_every_variant, on the CPU.  tests/test_gpu_variants.py runs the rows.

The three launches that ask for more than 64 KiB of dynamic LDS are all within reach of small frames, and each has a row: the FAST launch
from one cell column 3718 px wide (the smallest frame found by a search over the planning call: 3750 x 104 = 390 000 px, 200 features, one
level), k_quota from 6554 cells on a level (450 x 450 = 202 500 px, 36 000 features, one level: 7056 cells), k_cell_select in any small
launch group whose lists may reach 2048 entries."""
import numpy as np
import pytest

from orb_slam_amd import capi
import oracle_lib as orc
import variant_cases as vc

ROWS = vc.VARIANT_CASES
IDS = [r["id"] for r in ROWS]
TILED, STRIP, FUSED = 0, 1, 2
RZS_LDS_BUDGET, RZS_ROWS_MIN, RZS_ROWS_CAP, RZS_SLACK = 160 * 1024 // 8, 12, 48, 16       # k_resize_strip.h


def test_ids_are_unique_and_stage_tables_are_named():
    assert len(set(IDS)) == len(IDS)
    assert capi.variant_count(capi.VS_COUNT) == -1 and capi.variant_count(-1) == -1
    for s in range(capi.VS_COUNT):
        n = capi.variant_count(s)
        assert n >= 1
        names = [capi.variant_name(s, v) for v in range(n)]
        assert len(set(names)) == n and "?" not in names, (s, names)          # one name per instantiation
        assert capi.variant_name(s, n) == "?" and capi.variant_name(s, -1) == "?"


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_row_plans_what_it_targets(row):
    assert vc.names_of(vc.plan_of(row)) == row["targets"]


def test_the_table_covers_every_variant():
    seen = {s: set() for s in range(capi.VS_COUNT)}
    flags = {s: 0 for s in range(capi.VS_COUNT)}
    for row in ROWS:
        for s, (vid, fl, mask) in enumerate(vc.plan_of(row)):
            assert (vid < 0) == (mask == 0) and (vid < 0 or mask >> vid & 1)
            seen[s] |= {v for v in range(64) if mask >> v & 1}
            flags[s] |= fl
    for s in range(capi.VS_COUNT):
        missing = sorted(set(range(capi.variant_count(s))) - seen[s])
        assert seen[s] == set(range(capi.variant_count(s))), "stage %s: no row for %s" % (capi.VS_NAMES[s], [capi.variant_name(s, v) for v in missing])
    # the launch modes: blur inside the FAST launch, on the side stream, per keypoint window; XCD renumbering; the three launches above 64 KiB of LDS
    assert flags[capi.VS_FAST] & capi.VF_FUSE_BLUR and flags[capi.VS_BLUR] & capi.VF_OVERLAP and flags[capi.VS_DESCRIBE] & capi.VF_ON_DEMAND
    assert all(flags[s] & capi.VF_XCD_AFFINITY for s in range(capi.VS_PYRAMID, capi.VS_COUNT) if s != capi.VS_BLUR)      # (the 64-frame row blurs on demand)
    assert all(flags[s] & capi.VF_LDS_OVER_64K for s in (capi.VS_FAST, capi.VS_QUOTA, capi.VS_CELL_SELECT))


def test_on_demand_requested_but_not_supported_takes_the_plane_path():
    """describe_od_supported wants every level >= 64 x 44: with the blur on demand requested in a full launch group, six levels of 160 x 120
    (the deepest 64 x 48) take k_describe_od and no blur launch, seven (54 x 40) the stand-alone blur on the side stream and k_describe"""
    by_id = {r["id"]: r for r in ROWS}
    for rid, blur, desc in (("s7_F33_od1_dev_fails_od_rule", "k_blur_mfma", "k_describe<false>"),
                            ("s7_F33_od1_gat_fails_od_rule", "k_blur_gather<true, BLUR_ROWS>", "k_describe_gather<false>"),
                            ("s6_F33_od1_dev_passes_od_rule", None, "k_describe_od<false>")):
        row = by_id[rid]
        assert row["on_demand"] == 1 and row["F"] >= capi.OD_MIN_FRAMES_DEFAULT
        g = capi.geometry(row["w"], row["h"], **row["ctor"])
        assert all(l["w"] >= 64 and l["h"] >= 44 for l in g) == (blur is None), g[-1]
        p = vc.plan_of(row)
        assert vc.names_of(p)["blur"] == blur and vc.names_of(p)["describe"] == desc
        assert bool(p[capi.VS_BLUR][1] & capi.VF_OVERLAP) == (blur is not None) and bool(p[capi.VS_DESCRIBE][1] & capi.VF_ON_DEMAND) == (blur is None)


def _resize_tables(sw, sh, dw, dh):
    """cv::resize's INTER_LINEAR taps of a level dw x dh from sw x sh (the float sequence of the library's host geometry): first / second source
    column of every output column, first / second source row of every output row"""
    fx = ((np.arange(dw) + 0.5) * (1.0 / (float(dw) / sw)) - 0.5).astype(np.float32)
    sx = np.clip(np.floor(fx).astype(np.int64), 0, sw - 1)
    fy = ((np.arange(dh) + 0.5) * (1.0 / (float(dh) / sh)) - 0.5).astype(np.float32)
    sy = np.floor(fy).astype(np.int64)
    return sx, np.minimum(sx + 1, sw - 1), np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)


def _expected_resize_kernel(g, l, stride0, bits0, gather):
    """orbx_debug_resize_form's rule for level l of a launch group of 32 frames or more, restated: a strip when the four output pixels of a lane
    read at most 8 adjacent source bytes (the windowed arithmetic), the source rows are 4-byte aligned, and strips of at least 12 output rows
    (the largest multiple of 4 up to 48) fit the strip's LDS budget; the tiled kernel otherwise.  Level 1 reads the caller's frames (their
    pitch and alignment; the gather kernels), deeper levels pyramid planes of pitch w rounded up to 64."""
    (sw, sh), (dw, dh) = (g[l - 1]["w"], g[l - 1]["h"]), (g[l]["w"], g[l]["h"])
    sx, sx1, sy0, sy1 = _resize_tables(sw, sh, dw, dh)
    window = max(sx1[min(x0 + 3, dw - 1)] - sx[x0] + 1 for x0 in range(0, dw, 4)) <= 8
    stride = stride0 if l == 1 else (sw + 63) // 64 * 64
    aligned = l > 1 or ((bits0 | stride0) & 3) == 0
    ga = "_gather" if gather and l == 1 else ""
    tiled = "k_resize%s<%s, %s>" % (ga, "true" if aligned else "false", "true" if window else "false")
    if not window or not aligned or stride > RZS_LDS_BUDGET:
        return tiled
    readable = stride if l > 1 else min(stride, (sw + 15) & ~15)
    for rows in range(RZS_ROWS_CAP, RZS_ROWS_MIN - 1, -4):
        lds = 0
        for by0 in range(0, dh, rows):
            by1 = min(by0 + rows - 1, dh - 1)
            lds = max(lds, (((sy1[by1] - sy0[by0]) * stride + readable + 15) & ~15) + RZS_SLACK)
        if lds <= RZS_LDS_BUDGET:
            ng = ((dw + 3) // 4 + 63) // 64
            return "k_resize%s<%d>" % (ga, ng if ng <= 4 else 0)
    return tiled


def test_pyramid_rows_agree_with_the_resize_form_rules():
    """fewer than 32 frames: the fused cones and nothing else (the first of them in the caller's alignment and form, the others aligned);
    32 and more: per level exactly the kernel the restated rule gives.  Between them the rows have levels on both sides of every clause."""
    reasons = set()
    for row in ROWS:
        kernels, g = row["targets"]["pyramid_all"], capi.geometry(row["w"], row["h"], **{k: v for k, v in row["ctor"].items() if k != "fp_contract"})
        if len(g) == 1:
            assert kernels == [] and row["targets"]["pyramid"] is None, row["id"]
            continue
        p = vc.plan_of(row)
        # what the pipeline reads as level 0 (variant_cases.plan_of): only the gray DEVICE / GATHER forms hand over the caller's own rows
        own = row["form"] in (vc.DEVICE, vc.GATHER)
        stride0 = row.get("stride", row["w"]) if own else (row["gray_stride"] if row["form"] == vc.COLOR_GRAY else
                                                       (row["w"] + 63) // 64 * 64 if row["form"] in (vc.ONE, vc.COLOR_ONE) else (row["w"] + 15) & ~15)
        bits0 = row.get("offset", 0) if own else 0
        gather = row["form"] == vc.GATHER
        al0 = ((bits0 | stride0) & 3) == 0
        cones = row["ctor"].get("scaleFactor", 1.2) <= 2.0          # (the fused launches exist for scale factors up to 2)
        assert cones or not any(k.startswith("k_pyramid") for k in kernels), row["id"]
        if row["F"] < 32 and cones:
            first ="k_pyramid<%s, %s>" % ("true" if al0 else "false", "true" if gather else "false")
            assert row["targets"]["pyramid"] == first and set(kernels) <= {first, "k_pyramid<true, false>"}, (row["id"], kernels)
            continue
        want = [_expected_resize_kernel(g, l, stride0, bits0, gather) for l in range(1, len(g))]
        assert row["targets"]["pyramid"] == want[0] and sorted(set(want)) == sorted(kernels), (row["id"], want, kernels)
        assert p[capi.VS_PYRAMID][2] == sum(1 << v for v in range(capi.variant_count(capi.VS_PYRAMID)) if capi.variant_name(capi.VS_PYRAMID, v) in want)
        reasons |= {k.split("<")[1] for k in want}
    assert {"true, true>", "false, true>", "true, false>", "false, false>", "0>", "1>", "2>", "3>", "4>"} <= reasons


def test_early_stops_plan_only_the_stages_in_front():
    row = next(r for r in ROWS if r["form"] == vc.DEVICE and r["F"] >= 32)
    full = vc.plan_of(row)
    for stop, live in ((0, [capi.VS_PYRAMID]), (1, [capi.VS_PYRAMID, capi.VS_FAST]), (4, [capi.VS_PYRAMID, capi.VS_FAST, capi.VS_QUOTA, capi.VS_CELL_SELECT, capi.VS_LEVEL_SELECT])):
        p = vc.plan_of(row, stop_after=stop)
        for s in range(capi.VS_PYRAMID, capi.VS_COUNT):
            assert (p[s][0] >= 0) == (s in live), (stop, s, p[s])
            if s in live and s != capi.VS_BLUR:
                assert p[s][0] == full[s][0]
    assert vc.plan_of(row, stop_after=5)[capi.VS_BLUR][0] >= 0 and vc.plan_of(row, stop_after=5)[capi.VS_DESCRIBE][0] < 0


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_oracle_finds_key_points_in_every_row(row):
    """a row whose frames give no key points would compare empty outputs: the first frame of each gives the oracle at least MIN_KEYPOINTS"""
    kw = dict(row["ctor"])
    if "scoreType" in kw:
        kw["scoreType"] = orc.HARRIS_SCORE if kw["scoreType"] == capi.HARRIS_SCORE else orc.FAST_SCORE
    k, _ = orc.OracleExtractor(**kw)(vc.gray_frames(row)[0])
    assert len(k) >= vc.MIN_KEYPOINTS, len(k)
