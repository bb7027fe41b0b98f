"""Every kernel variant of the extractor, run: one call per row of VARIANT_CASES (tests/variant_cases.py; tests/test_launch_plan_host.py shows on
the CPU that the rows reach every instantiation of every stage).  Each row's outputs are compared with the CPU oracle byte for byte — key
points, descriptors, counts, status — and the handle must report, stage by stage, the kernels the row names (orbx_debug_launch_variant).
One plain gray row per FAST variant (all sixteen, small launch groups and full ones) also stops after the stages and compares the pyramid,
the blurred planes, the NMS map and the band table with the oracle, so that a wrong halo shows in the plane where it happens."""
import numpy as np
import pytest
import torch

from orb_slam_amd import capi
import color_ref as cr
import oracle_lib as orc
import variant_cases as vc
from test_gpu_parity import _check_band_lists

pytestmark = pytest.mark.gpu

ROWS = vc.VARIANT_CASES
TILED, STRIP, FUSED = 0, 1, 2          # orbx_debug_resize_form
IDS = [r["id"] for r in ROWS]


def _outputs(F, cap):
    return (torch.zeros((F, cap, 28), dtype=torch.uint8, device="cuda"), torch.zeros((F, cap, 32), dtype=torch.uint8, device="cuda"),
            torch.full((F,), -7, dtype=torch.int32, device="cuda"), torch.full((F,), -7, dtype=torch.int32, device="cuda"))


def _pitched(arr, stride, offset):
    """a device copy of an (H, W) or (H, W, C) frame whose rows lie `stride` bytes apart, `offset` bytes into its own allocation"""
    a = arr if arr.ndim == 3 else arr[:, :, None]
    h, w, c = a.shape
    buf = torch.full((offset + stride * h + 64,), 0xA5, dtype=torch.uint8, device="cuda")      # (not zero: a tap that strays shows)
    view = torch.as_strided(buf, (h, w, c), (stride, c, 1), offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return view if arr.ndim == 3 else view[:, :, 0]


def _buffer(frames, stride, offset):
    """one device buffer holding (F, H, W[, C]) frames, rows `stride` bytes apart, frames stride * H apart, the first `offset` bytes in"""
    a = frames if frames.ndim == 4 else frames[..., None]
    F, h, w, c = a.shape
    buf = np.full(offset + F * stride * h + 64, 0xA5, np.uint8)
    for f in range(F):
        np.lib.stride_tricks.as_strided(buf[offset + f * stride * h:], (h, w, c), (stride, c, 1))[...] = a[f]
    return torch.from_numpy(buf).cuda()


def _run(ex, row, gray, colour):
    """the row's call; -> host (kps, desc, n, status) per frame"""
    w, h, F, form = row["w"], row["h"], row["F"], row["form"]
    cap = ex.max_keypoints
    fmt = row.get("fmt", capi.PIX_GRAY8)
    ch = capi.PIX_CHANNELS[fmt]
    stride, offset = row.get("stride", w * ch), row.get("offset", 0)
    if form in (vc.ONE, vc.COLOR_ONE):
        k, d = ex(gray[0]) if form == vc.ONE else ex.extract_color(colour[0], fmt)
        kk, dd = np.zeros((1, cap, 28), np.uint8), np.zeros((1, cap, 32), np.uint8)
        kk[0, :len(k)] = k.view(np.uint8).reshape(-1, 28)
        dd[0, :len(k)] = d
        return kk, dd, np.array([len(k)], np.int32), np.zeros(1, np.int32)
    out = _outputs(F, cap)
    p = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), cap, out[3].data_ptr())
    keep = None
    if form == vc.DEVICE:
        keep = _buffer(gray, stride, offset)
        ex.extract_batch_device(keep.data_ptr() + offset, F, w, h, stride, stride * h, *p)
    elif form == vc.GATHER:
        keep = [_pitched(gray[f], stride, offset) for f in range(F)]
        ex.extract_batch(keep, *p)
    elif form == vc.HOST:
        ex.extract_batch([gray[f] for f in range(F)], *p)
    elif form == vc.COLOR_DEVICE:
        keep = _buffer(colour, stride, offset)
        ex.extract_batch_device_color(keep.data_ptr() + offset, F, w, h, stride, stride * h, fmt, *p)
    elif form == vc.COLOR_GRAY:
        keep = _buffer(colour, stride, offset)
        gs = row["gray_stride"]
        dg = torch.zeros(F * gs * h + 64, dtype=torch.uint8, device="cuda")
        ex.extract_batch_device_color(keep.data_ptr() + offset, F, w, h, stride, stride * h, fmt, *p, dg.data_ptr(), gs, gs * h)
        keep = (keep, dg)
    elif form == vc.COLOR_GATHER:
        keep = [_pitched(colour[f], stride, offset) for f in range(F)]
        ex.extract_batch_color(keep, fmt, *p)
    else:
        raise ValueError(form)
    torch.cuda.synchronize()
    del keep
    return tuple(t.cpu().numpy() for t in out)


def _oracle(row, **kw):
    c = dict(row["ctor"])
    if "scoreType" in c:
        c["scoreType"] = orc.HARRIS_SCORE if c["scoreType"] == capi.HARRIS_SCORE else orc.FAST_SCORE
    return orc.OracleExtractor(**c, **kw)


def _assert_variants(ex, row):
    got, flags = {}, 0
    for s in range(capi.VS_COUNT):
        vid, fl, mask, name = ex.launch_variant(s)
        assert name == (capi.variant_name(s, vid) if vid >= 0 else "")
        got[capi.VS_NAMES[s]] = name or None
        flags |= fl
        if s in (capi.VS_PYRAMID, capi.VS_CELL_SELECT):
            got[capi.VS_NAMES[s] + "_all"] = [capi.variant_name(s, v) for v in range(64) if mask >> v & 1]
    got["flags"] = flags
    assert got == row["targets"]
    # ... and orbx_debug_resize_form tells the same story level by level
    kinds = set()
    for l in range(1, row["ctor"].get("nlevels", 8)):
        form, rows = ex.resize_form(l)
        ng = ((ex.level_size(l)[0] + 3) // 4 + 63) // 64
        kinds.add("cone" if form == FUSED else "strip%d" % (ng if ng <= 4 else 0) if form == STRIP else "tiled")
    assert kinds == {"cone" if k.startswith("k_pyramid") else "tiled" if "," in k else "strip" + k[-2] for k in got["pyramid_all"]}, (kinds, got["pyramid_all"])


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_row_matches_the_oracle_and_runs_the_variants_it_names(gpu_extractor_factory, row):
    gray = vc.gray_frames(row)
    fmt = row.get("fmt", capi.PIX_GRAY8)
    colour = None
    if row["form"] in (vc.COLOR_ONE, vc.COLOR_DEVICE, vc.COLOR_GRAY, vc.COLOR_GATHER):
        colour = cr.colorize(gray, fmt, 1)
        gray = cr.to_gray(colour if colour.ndim == 4 else colour[..., None], fmt)      # what the conversion must hand to the pipeline
    ex = gpu_extractor_factory(device=0, max_batch=row["F"], **row["ctor"])
    ex.set_blur_on_demand(row.get("on_demand", 1))
    k, d, n, st = _run(ex, row, gray, colour)
    _assert_variants(ex, row)
    oracle, cache = _oracle(row), {}
    assert (st == 0).all()
    for f in range(row["F"]):
        key = gray[f].tobytes()
        if key not in cache:
            cache[key] = oracle(gray[f])
        ok, od = cache[key]
        assert n[f] == len(ok) and k[f, :n[f]].tobytes() == ok.tobytes() and np.array_equal(d[f, :n[f]], od), f


# the first row of every FAST variant among the plain gray rows (DEVICE / GATHER: the forms whose level 0 the dumps can be compared with; the
# default score type, as in test_stage_parity_vga): all sixteen have one, small launch groups and full ones
def _stage_rows():
    seen, rows = set(), []
    for r in ROWS:
        key = r["targets"]["fast"]
        if key not in seen and r["form"] in (vc.DEVICE, vc.GATHER) and r["ctor"].get("scoreType") is None:
            seen.add(key)
            rows.append(r)
    return rows


def test_every_fast_variant_has_a_stage_row():
    assert sorted(r["targets"]["fast"] for r in _stage_rows()) == sorted(capi.variant_name(capi.VS_FAST, v) for v in range(capi.variant_count(capi.VS_FAST)))


def test_the_parts_of_a_phased_call_add_to_one_record(gpu_extractor_factory):
    row = next(r for r in ROWS if r["form"] == vc.DEVICE and r["F"] >= 32 and r.get("on_demand") == 0)
    gray = vc.gray_frames(row)
    w, h, F, stride = row["w"], row["h"], row["F"], row["stride"]
    ex = gpu_extractor_factory(device=0, max_batch=F, **row["ctor"])
    ex.set_blur_on_demand(0)
    buf = _buffer(gray, stride, 0)
    out = _outputs(F, ex.max_keypoints)
    args = (buf.data_ptr(), F, w, h, stride, stride * h, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ex.max_keypoints, out[3].data_ptr())
    ex.extract_batch_device(*args)
    whole = [ex.launch_variant(s) for s in range(capi.VS_COUNT)]
    ex.extract_batch_device(*args, phases=capi.PHASE_PYRAMID)
    assert [ex.launch_variant(s)[0] >= 0 for s in range(capi.VS_PYRAMID, capi.VS_COUNT)] == [True] + [False] * 6
    ex.extract_batch_device(*args, phases=capi.PHASE_DETECT)
    assert ex.launch_variant(capi.VS_DESCRIBE)[0] < 0 and ex.launch_variant(capi.VS_PYRAMID) == whole[capi.VS_PYRAMID]
    ex.extract_batch_device(*args, phases=capi.PHASE_DESCRIBE)
    torch.cuda.synchronize()
    assert [ex.launch_variant(s) for s in range(capi.VS_COUNT)] == whole
    _assert_variants(ex, row)


@pytest.mark.parametrize("row", _stage_rows(), ids=lambda r: r["id"])
def test_stage_planes_of_the_fast_variants(gpu_extractor_factory, row):
    gray = vc.gray_frames(row)
    nl = row["ctor"].get("nlevels", 8)
    ex = gpu_extractor_factory(device=0, max_batch=row["F"], **row["ctor"])
    ex.set_blur_on_demand(0)                                       # (the blurred planes exist only in this mode)
    frames = sorted({0, row["F"] - 1})
    ex.set_stop_after(capi.ST_BLUR)
    try:
        _run(ex, row, gray, None)
        assert ex.launch_variant(capi.VS_FAST)[3] == row["targets"]["fast"]
        dumps = {}
        for f in frames:
            o = _oracle(row, dumps=True)
            o(gray[f])
            dumps[f] = o
            for l in range(nl):
                assert ex.level_size(l) == o.level_size(l)
                np.testing.assert_array_equal(ex.fetch_plane(capi.DBG_PLANE, l, f), o.level_plane(l, 0), err_msg="frame %d pyramid level %d" % (f, l))
                np.testing.assert_array_equal(ex.fetch_plane(capi.DBG_BLUR, l, f), orc.gaussian_blur7(o.level_plane(l, 0)), err_msg="frame %d blur level %d" % (f, l))
        ex.set_stop_after(capi.ST_FAST_CELLS)
        _run(ex, row, gray, None)
        assert ex.launch_variant(capi.VS_FAST)[3] == row["targets"]["fast"]
        for f in frames:
            _check_band_lists(dumps[f], nl, [ex.fetch_bands(l, f) for l in range(nl)], [ex.fetch_plane(capi.DBG_NMS, l, f) for l in range(nl)])
    finally:
        ex.set_stop_after(-1)
