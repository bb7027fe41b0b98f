"""Call descriptions that between them reach every kernel variant of the extractor (orbx_launch.h: one enum per stage), shared by
tests/test_launch_plan_host.py (no GPU: the plan of every row, and that the table covers every variant) and tests/test_gpu_variants.py (the
calls themselves against the oracle, and that each stage ran the variant the row names).

A row is one call:
  ctor      constructor arguments of the extractor and of the oracle (nfeatures, scaleFactor, nlevels, scoreType, fp_contract)
  w, h, F   frame size and frames in the call (= max_batch: one launch group)
  form      DEVICE        orbx_extract_batch_device on one buffer: rows `stride` bytes apart, first frame `offset` bytes into the allocation
            GATHER        orbx_extract_batch, device frames: each its own allocation, rows `stride` apart, `offset` bytes in
            HOST          orbx_extract_batch, host frames (uploaded into a buffer of pitch w rounded up to 16)
            ONE           orbx_extract (one host frame; F = 1)
            COLOR_ONE     orbx_extract_color (one host frame of format fmt)
            COLOR_DEVICE  orbx_extract_batch_device_color on one buffer (stride / offset in bytes of the colour rows), gray ring inside
            COLOR_GRAY    ... with the caller's gray planes (pitch gray_stride) as level 0
            COLOR_GATHER  orbx_extract_batch_color, device frames
  on_demand the handle's blur-on-demand mode
  family    synthetic frame family (orb_slam_amd.synth)
  targets   per stage the kernel the row is there for, by name (None: the stage launches nothing); pyramid_all / cell_select_all: every
            kernel the stage launches; flags: the VF_* bits of all stages OR-ed
The shapes were chosen on the CPU with capi.plan(): the smallest frames that select the variant and still give the oracle key points."""
from orb_slam_amd import capi, synth

DEVICE, GATHER, HOST, ONE, COLOR_ONE, COLOR_DEVICE, COLOR_GRAY, COLOR_GATHER = "device", "gather", "host", "one", "color_one", "color_device", "color_gray", "color_gather"
MIN_KEYPOINTS = 12        # what the oracle must find in the first frame of every row (checked on the CPU): a row that extracts nothing checks nothing


def _pitch16(n):
    return (n + 15) & ~15


def plan_of(row, stop_after=-1):
    """capi.plan for the launch group the row's call queues: [(id, flags, mask)] per stage"""
    w, h, F, form = row["w"], row["h"], row["F"], row["form"]
    ch = capi.PIX_CHANNELS[row.get("fmt", capi.PIX_GRAY8)]
    stride, offset = row.get("stride", w * ch), row.get("offset", 0)
    kw = dict(on_demand=row.get("on_demand", 1), stop_after=stop_after, **row["ctor"])
    gp = _pitch16(w)
    if form == DEVICE:
        kw.update(row_stride=stride, frame_stride=stride * h, base_bits=offset)
    elif form == GATHER:
        kw.update(row_stride=stride, base_bits=offset, gather=True)
    elif form == HOST:
        kw.update(row_stride=gp, frame_stride=gp * h)
    elif form in (ONE, COLOR_ONE):
        ds = (w + 63) // 64 * 64
        kw.update(row_stride=ds, frame_stride=ds * h)
        if form == ONE:
            kw.update(one_frame=True, one_frame_bytes=ds * h)
        else:
            kw.update(color_fmt=row["fmt"], color_bits=_pitch16(w * ch) | ds)
    elif form == COLOR_DEVICE:
        kw.update(row_stride=gp, frame_stride=gp * h, color_fmt=row["fmt"], color_bits=offset | stride | (stride * h) | gp | (gp * h))
    elif form == COLOR_GRAY:
        gs = row["gray_stride"]
        kw.update(row_stride=gs, frame_stride=gs * h, color_fmt=row["fmt"], color_bits=offset | stride | (stride * h) | gs | (gs * h))
    elif form == COLOR_GATHER:
        kw.update(row_stride=gp, frame_stride=gp * h, color_fmt=row["fmt"], color_gather=True, color_bits=offset | stride | gp | (gp * h))
    else:
        raise ValueError(form)
    return capi.plan(w, h, F, **kw)


def names_of(plan):
    """the plan in the words of a row's targets"""
    t = {}
    flags = 0
    for s, (vid, fl, mask) in enumerate(plan):
        t[capi.VS_NAMES[s]] = capi.variant_name(s, vid) if vid >= 0 else None
        flags |= fl
        if s in (capi.VS_PYRAMID, capi.VS_CELL_SELECT):
            t[capi.VS_NAMES[s] + "_all"] = [capi.variant_name(s, v) for v in range(64) if mask >> v & 1]
    t["flags"] = flags
    return t


def gray_frames(row):
    """the row's gray frames (F, h, w): three families in turn unless the row names one"""
    import numpy as np
    fam = row.get("family")
    fams = [fam] if fam is not None else [synth.BLOCKS, synth.NOISE, synth.MIDTEX]
    distinct = min(row["F"], 4)
    pix = [synth.frame(row["w"], row["h"], fams[i % len(fams)], 40 + i) for i in range(distinct)]
    return np.stack([pix[f % distinct] for f in range(row["F"])])


def R(id, form, w, h, F, targets, **kw):
    ctor = {k: kw.pop(k) for k in ("nfeatures", "scaleFactor", "nlevels", "scoreType", "fp_contract") if k in kw}
    return dict(id=id, form=form, w=w, h=h, F=F, ctor=ctor, targets=targets, **kw)


VARIANT_CASES = [
    R('s_F4_od1_host', HOST, 160, 120, 4,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F33_od0_dev_s164_o0', DEVICE, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<1>', 'pyramid_all': ['k_resize<1>'], 'fast': 'k_fast_cells<true, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': 'k_blur<true, BLUR_ROWS>', 'describe': 'k_describe<false>', 'flags': 4},
      stride=164, offset=0, on_demand=0, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F33_od0_dev_s176_o0', DEVICE, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<1>', 'pyramid_all': ['k_resize<1>'], 'fast': 'k_fast_cells<true, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': 'k_blur_mfma', 'describe': 'k_describe<false>', 'flags': 4},
      stride=176, offset=0, on_demand=0, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('w6_F64_od1_gat_s600_o0', GATHER, 600, 120, 64,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<2>', 'pyramid_all': ['k_resize<2>', 'k_resize_gather<2>'], 'fast': 'k_fast_cells_gather<true, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od_gather<false>', 'flags': 24},
      stride=600, offset=0, on_demand=1, nfeatures=100, nlevels=3),      # oracle: 100 key points in frame 0
    R('x_F33_od0_gat_s320_o0', GATHER, 320, 240, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<true, false>', 'pyramid_all': ['k_resize<true, false>', 'k_resize_gather<true, false>'], 'fast': 'k_fast_cells_gather<true, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': 'k_blur_gather<true, BLUR_ROWS>', 'describe': 'k_describe_gather<false>', 'flags': 4},
      stride=320, offset=0, on_demand=0, nfeatures=100, scaleFactor=2.2, nlevels=3),      # oracle: 100 key points in frame 0
    R('w3_F1_od1_fma_gat_s300_o0', GATHER, 300, 120, 1,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<true, true>', 'pyramid_all': ['k_pyramid<true, true>'], 'fast': 'k_fast_blur_gather<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe_gather<true>', 'flags': 3},
      stride=300, offset=0, on_demand=1, nfeatures=100, nlevels=3, scoreType=0, fp_contract=True),      # oracle: 95 key points in frame 0
    R('s_F33_od1_gray_g161', COLOR_GRAY, 160, 120, 33,
      {'color': 'k_to_gray<1, false, false, false>', 'ingest': None, 'pyramid': 'k_resize<false, true>', 'pyramid_all': ['k_resize<false, true>', 'k_resize<1>'], 'fast': 'k_fast_cells<false, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od<false>', 'flags': 8},
      fmt=0, stride=160, gray_stride=161, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_fma_dev_s161_o1', DEVICE, 160, 120, 1,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<false, false>', 'pyramid_all': ['k_pyramid<false, false>'], 'fast': 'k_fast_blur<false, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<true>', 'flags': 2},
      stride=161, offset=1, on_demand=1, nfeatures=150, nlevels=4, scoreType=0, fp_contract=True),      # oracle: 104 key points in frame 0
    R('s_F33_od1_fma_gat_s161_o1', GATHER, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<false, true>', 'pyramid_all': ['k_resize_gather<false, true>', 'k_resize<1>'], 'fast': 'k_fast_cells_gather<false, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od_gather<true>', 'flags': 8},
      stride=161, offset=1, on_demand=1, nfeatures=150, nlevels=4, scoreType=0, fp_contract=True),      # oracle: 104 key points in frame 0
    R('l_F33_od1_fma_dev_s1408_o0', DEVICE, 288, 216, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<true, true>', 'pyramid_all': ['k_resize<true, true>', 'k_resize<1>'], 'fast': 'k_fast_cells<true, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od<true>', 'flags': 8},
      stride=1408, offset=0, on_demand=1, nfeatures=200, scoreType=0, fp_contract=True),      # oracle: 200 key points in frame 0
    R('s_F1_od1_gat_s161_o1', GATHER, 160, 120, 1,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<false, true>', 'pyramid_all': ['k_pyramid<false, true>'], 'fast': 'k_fast_blur_gather<false, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe_gather<false>', 'flags': 2},
      stride=161, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('l_F1_od1_one', ONE, 288, 216, 1,
      {'color': None, 'ingest': 'k_ingest', 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, false>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 3},
      on_demand=1, nfeatures=200),      # oracle: 200 key points in frame 0
    R('l_F33_od0_dev_s289_o1', DEVICE, 288, 216, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<false, true>', 'pyramid_all': ['k_resize<false, true>', 'k_resize<1>'], 'fast': 'k_fast_cells<false, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': 'k_blur<false, BLUR_ROWS>', 'describe': 'k_describe<false>', 'flags': 4},
      stride=289, offset=1, on_demand=0, nfeatures=200),      # oracle: 200 key points in frame 0
    R('l_F33_od0_gat_s289_o1', GATHER, 288, 216, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<false, true>', 'pyramid_all': ['k_resize_gather<false, true>', 'k_resize<1>'], 'fast': 'k_fast_cells_gather<false, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': 'k_blur_gather<false, BLUR_ROWS>', 'describe': 'k_describe_gather<false>', 'flags': 4},
      stride=289, offset=1, on_demand=0, nfeatures=200),      # oracle: 200 key points in frame 0
    R('s_F1_od1_c1_f1', COLOR_ONE, 160, 120, 1,
      {'color': 'k_to_gray<3, false, true, false>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cg_f1_s480', COLOR_GATHER, 160, 120, 1,
      {'color': 'k_to_gray<3, false, true, true>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=1, stride=480, offset=0, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cd_f1_s481', COLOR_DEVICE, 160, 120, 1,
      {'color': 'k_to_gray<3, false, false, false>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=1, stride=481, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cg_f1_s481', COLOR_GATHER, 160, 120, 1,
      {'color': 'k_to_gray<3, false, false, true>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=1, stride=481, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_c1_f2', COLOR_ONE, 160, 120, 1,
      {'color': 'k_to_gray<3, true, true, false>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=2, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cg_f2_s480', COLOR_GATHER, 160, 120, 1,
      {'color': 'k_to_gray<3, true, true, true>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=2, stride=480, offset=0, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cd_f2_s481', COLOR_DEVICE, 160, 120, 1,
      {'color': 'k_to_gray<3, true, false, false>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=2, stride=481, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cg_f2_s481', COLOR_GATHER, 160, 120, 1,
      {'color': 'k_to_gray<3, true, false, true>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=2, stride=481, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_c1_f3', COLOR_ONE, 160, 120, 1,
      {'color': 'k_to_gray<4, false, true, false>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=3, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cg_f3_s640', COLOR_GATHER, 160, 120, 1,
      {'color': 'k_to_gray<4, false, true, true>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=3, stride=640, offset=0, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cd_f3_s641', COLOR_DEVICE, 160, 120, 1,
      {'color': 'k_to_gray<4, false, false, false>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=3, stride=641, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cg_f3_s641', COLOR_GATHER, 160, 120, 1,
      {'color': 'k_to_gray<4, false, false, true>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=3, stride=641, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_c1_f4', COLOR_ONE, 160, 120, 1,
      {'color': 'k_to_gray<4, true, true, false>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=4, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cg_f4_s640', COLOR_GATHER, 160, 120, 1,
      {'color': 'k_to_gray<4, true, true, true>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=4, stride=640, offset=0, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cd_f4_s641', COLOR_DEVICE, 160, 120, 1,
      {'color': 'k_to_gray<4, true, false, false>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=4, stride=641, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_cg_f4_s641', COLOR_GATHER, 160, 120, 1,
      {'color': 'k_to_gray<4, true, false, true>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=4, stride=641, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F1_od1_gray_g160', COLOR_GRAY, 160, 120, 1,
      {'color': 'k_to_gray<1, false, true, false>', 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      fmt=0, stride=160, gray_stride=160, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('l_F1_od1_gat_s288_o0', GATHER, 288, 216, 1,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<true, true>', 'pyramid_all': ['k_pyramid<true, false>', 'k_pyramid<true, true>'], 'fast': 'k_fast_blur_gather<true, false>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe_gather<false>', 'flags': 3},
      stride=288, offset=0, on_demand=1, nfeatures=200),      # oracle: 200 key points in frame 0
    R('l_F1_od1_dev_s289_o1', DEVICE, 288, 216, 1,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<false, false>', 'pyramid_all': ['k_pyramid<false, false>', 'k_pyramid<true, false>'], 'fast': 'k_fast_blur<false, false>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 3},
      stride=289, offset=1, on_demand=1, nfeatures=200),      # oracle: 200 key points in frame 0
    R('l_F1_od1_gat_s289_o1', GATHER, 288, 216, 1,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<false, true>', 'pyramid_all': ['k_pyramid<true, false>', 'k_pyramid<false, true>'], 'fast': 'k_fast_blur_gather<false, false>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe_gather<false>', 'flags': 3},
      stride=289, offset=1, on_demand=1, nfeatures=200),      # oracle: 200 key points in frame 0
    R('x_F1_od1_dev_s321_o1', DEVICE, 320, 240, 1,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<false, false>', 'pyramid_all': ['k_resize<false, false>', 'k_resize<true, false>'], 'fast': 'k_fast_blur<false, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      stride=321, offset=1, on_demand=1, nfeatures=100, scaleFactor=2.2, nlevels=3),      # oracle: 100 key points in frame 0
    R('x_F1_od1_gat_s321_o1', GATHER, 320, 240, 1,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<false, false>', 'pyramid_all': ['k_resize<true, false>', 'k_resize_gather<false, false>'], 'fast': 'k_fast_blur_gather<false, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe_gather<false>', 'flags': 2},
      stride=321, offset=1, on_demand=1, nfeatures=100, scaleFactor=2.2, nlevels=3),      # oracle: 100 key points in frame 0
    R('s_F33_od1_gat_s160_o0', GATHER, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<1>', 'pyramid_all': ['k_resize<1>', 'k_resize_gather<1>'], 'fast': 'k_fast_cells_gather<true, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od_gather<false>', 'flags': 8},
      stride=160, offset=0, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F33_od1_gat_s1408_o0', GATHER, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<true, true>', 'pyramid_all': ['k_resize_gather<true, true>', 'k_resize<1>'], 'fast': 'k_fast_cells_gather<true, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od_gather<false>', 'flags': 8},
      stride=1408, offset=0, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('w9_F33_od1_dev_s900_o0', DEVICE, 900, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<3>', 'pyramid_all': ['k_resize<3>'], 'fast': 'k_fast_cells<true, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od<false>', 'flags': 8},
      stride=900, offset=0, on_demand=1, nfeatures=200, nlevels=2),      # oracle: 190 key points in frame 0
    R('w9_F33_od1_gat_s900_o0', GATHER, 900, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<3>', 'pyramid_all': ['k_resize_gather<3>'], 'fast': 'k_fast_cells_gather<true, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od_gather<false>', 'flags': 8},
      stride=900, offset=0, on_demand=1, nfeatures=200, nlevels=2),      # oracle: 190 key points in frame 0
    R('w10_F33_od1_dev_s1000_o0', DEVICE, 1000, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<4>', 'pyramid_all': ['k_resize<4>'], 'fast': 'k_fast_cells<true, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od<false>', 'flags': 8},
      stride=1000, offset=0, on_demand=1, nfeatures=200, nlevels=2),      # oracle: 200 key points in frame 0
    R('w10_F33_od1_gat_s1000_o0', GATHER, 1000, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<4>', 'pyramid_all': ['k_resize_gather<4>'], 'fast': 'k_fast_cells_gather<true, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od_gather<false>', 'flags': 8},
      stride=1000, offset=0, on_demand=1, nfeatures=200, nlevels=2),      # oracle: 200 key points in frame 0
    R('w12b_F33_od1_dev_s1280_o0', DEVICE, 1280, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<0>', 'pyramid_all': ['k_resize<0>'], 'fast': 'k_fast_cells<true, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od<false>', 'flags': 8},
      stride=1280, offset=0, on_demand=1, nfeatures=200, scaleFactor=1.1, nlevels=2),      # oracle: 200 key points in frame 0
    R('w12b_F33_od1_gat_s1280_o0', GATHER, 1280, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<0>', 'pyramid_all': ['k_resize_gather<0>'], 'fast': 'k_fast_cells_gather<true, FAST_LARGE>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od_gather<false>', 'flags': 8},
      stride=1280, offset=0, on_demand=1, nfeatures=200, scaleFactor=1.1, nlevels=2),      # oracle: 200 key points in frame 0
    # the rule of describe_od_supported just failing (level 6 is 54 x 40) and just holding (level 5 is 64 x 48) with the blur on demand requested;
    # plain gray rows for the stage planes of the FAST variants the rows above reach only through host, colour or Harris calls; the smallest
    # frames that plan more than 64 KiB of LDS for the FAST launch (one cell column 3718 px wide) and for k_quota (7056 cells on the level)
    R('s7_F33_od1_dev_fails_od_rule', DEVICE, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<1>', 'pyramid_all': ['k_resize<1>'], 'fast': 'k_fast_cells<true, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': 'k_blur_mfma', 'describe': 'k_describe<false>', 'flags': 4},
      stride=160, offset=0, on_demand=1, nfeatures=150, nlevels=7),      # oracle: 119 key points in frame 0
    R('s7_F33_od1_gat_fails_od_rule', GATHER, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<1>', 'pyramid_all': ['k_resize<1>', 'k_resize_gather<1>'], 'fast': 'k_fast_cells_gather<true, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': 'k_blur_gather<true, BLUR_ROWS>', 'describe': 'k_describe_gather<false>', 'flags': 4},
      stride=160, offset=0, on_demand=1, nfeatures=150, nlevels=7),      # oracle: 119 key points in frame 0
    R('s6_F33_od1_dev_passes_od_rule', DEVICE, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<1>', 'pyramid_all': ['k_resize<1>'], 'fast': 'k_fast_cells<true, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od<false>', 'flags': 8},
      stride=160, offset=0, on_demand=1, nfeatures=150, nlevels=6),      # oracle: 121 key points in frame 0
    R('s_F4_od1_dev_s160_o0', DEVICE, 160, 120, 4,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 2},
      stride=160, offset=0, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F4_od1_gat_s160_o0', GATHER, 160, 120, 4,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<true, true>', 'pyramid_all': ['k_pyramid<true, true>'], 'fast': 'k_fast_blur_gather<true, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe_gather<false>', 'flags': 2},
      stride=160, offset=0, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('l_F4_od1_dev_s288_o0', DEVICE, 288, 216, 4,
      {'color': None, 'ingest': None, 'pyramid': 'k_pyramid<true, false>', 'pyramid_all': ['k_pyramid<true, false>'], 'fast': 'k_fast_blur<true, false>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 3},
      stride=288, offset=0, on_demand=1, nfeatures=200),      # oracle: 200 key points in frame 0
    R('s_F33_od1_dev_s161_o1', DEVICE, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize<false, true>', 'pyramid_all': ['k_resize<false, true>', 'k_resize<1>'], 'fast': 'k_fast_cells<false, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select', 'k_cell_select_long'], 'level_select': 'k_level_select', 'blur': None, 'describe': 'k_describe_od<false>', 'flags': 8},
      stride=161, offset=1, on_demand=1, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('s_F33_od0_gat_s161_o1', GATHER, 160, 120, 33,
      {'color': None, 'ingest': None, 'pyramid': 'k_resize_gather<false, true>', 'pyramid_all': ['k_resize_gather<false, true>', 'k_resize<1>'], 'fast': 'k_fast_cells_gather<false, FAST_SMALL>', 'quota': 'k_quota', 'cell_select': 'k_cell_select_gather', 'cell_select_all': ['k_cell_select_gather', 'k_cell_select_long_gather'], 'level_select': 'k_level_select', 'blur': 'k_blur_gather<false, BLUR_ROWS>', 'describe': 'k_describe_gather<false>', 'flags': 4},
      stride=161, offset=1, on_demand=0, nfeatures=150, nlevels=4),      # oracle: 104 key points in frame 0
    R('fastlds_F1_3750x104', DEVICE, 3750, 104, 1,
      {'color': None, 'ingest': None, 'pyramid': None, 'pyramid_all': [], 'fast': 'k_fast_blur<false, false>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 3},
      stride=3750, offset=0, on_demand=1, nfeatures=200, nlevels=1),      # oracle: 200 key points in frame 0
    R('quotalds_F1_450x450', DEVICE, 450, 450, 1,
      {'color': None, 'ingest': None, 'pyramid': None, 'pyramid_all': [], 'fast': 'k_fast_blur<false, true>', 'quota': 'k_quota', 'cell_select': 'k_cell_select', 'cell_select_all': ['k_cell_select'], 'level_select': 'k_level_select_one', 'blur': None, 'describe': 'k_describe<false>', 'flags': 3},
      stride=450, offset=0, on_demand=1, nfeatures=36000, nlevels=1),      # oracle: 753 key points in frame 0
]
