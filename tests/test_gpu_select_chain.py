"""The selection chain (k_quota, k_cell_select, k_cell_select_long, k_level_select) through its plumbing: block -> (frame, item) maps with and
without the frame -> XCD renumbering, the per-cell constant record and k_quota's per-frame record, the staging area k_level_select shares by
list length.  Every case compares the product byte for byte with the CPU oracle (key points, descriptors, counts, status) and first asserts
on the CPU — from the host geometry and the oracle's stage dumps — that its frames really take the path it names.

Launch forms (orbx_launch.h, orbx_internal.h): fewer than 32 frames = the small-group form (one selection class, one wave per level),
32 and more = the throughput form (short lists of at most 384 entries first, k_cell_select_long for the rest, shared level staging), 64 and
more = the same with a frame's blocks renumbered onto one XCD and the grid padded to a multiple of 8 frames."""
import math

import numpy as np
import pytest
import torch

from orb_slam_amd import capi, synth
import oracle_lib as orc

pytestmark = pytest.mark.gpu

SEL_SMALL = 384          # k_select.hip: staging entries of a k_cell_select wave in the throughput form
REC_BANDS = 8            # orbx_internal.h: CELL_REC_BANDS


def _level_totals(o, g):
    """per level: (level total = sum of the cells' nToRetain, longest cell list, cells that retain nothing, cells that fell back to threshold 7,
    cells dumped), from the oracle's cell dumps of its last frame by the reference's quota rule (src/ORBextractor.cc:622-670)"""
    cells = o.cells()
    out = []
    for lvl, l in enumerate(g):
        cols, nc = l["grid_cols"], l["grid_cols"] * l["grid_rows"]
        nk, present, fb = np.zeros(nc, int), np.zeros(nc, bool), 0
        for info, k in cells:
            if info[0] == lvl:
                nk[info[1] * cols + info[2]], present[info[1] * cols + info[2]] = len(k), True
                fb += info[5]
        nfc = math.ceil(l["quota"] / nc)
        nret, done, dist, nomore = np.zeros(nc, int), np.zeros(nc, bool), 0, 0
        for c in range(nc):
            if not present[c]:
                continue
            if nk[c] > nfc:
                nret[c] = nfc
            else:
                nret[c], done[c] = nk[c], True
                dist += nfc - nk[c]
                nomore += 1
        while dist > 0 and nomore < nc:
            nnew, dist = nfc + int(math.ceil(np.float32(dist) / np.float32(nc - nomore))), 0
            for c in range(nc):
                if done[c]:
                    continue
                if nk[c] > nnew:
                    nret[c] = nnew
                else:
                    nret[c], done[c] = nk[c], True
                    dist += nnew - nk[c]
                    nomore += 1
        total = int(nret.sum())
        assert min(total, l["quota"]) == len(o.level_keypoints(lvl))          # the rule restated here is the oracle's
        out.append((total, int(nk.max()), int((nret == 0).sum()), fb, int(present.sum())))
    return out


def _bands_per_cell(g):
    return [l["n_bands"] // (l["grid_cols"] * l["grid_rows"]) for l in g]


def _staging_entries(g):
    """DevGeom::sel_lds_entries (orbx_geometry.hip): the longest list a cell or a level can have, at most 2048"""
    max_cell = max_level = 1
    for l, nb in zip(g, _bands_per_cell(g)):
        cw, ch, nc = l["cell_w"], l["cell_h"], l["grid_cols"] * l["grid_rows"]
        rb = -(-ch // nb)
        cap = ((cw + 1) // 2) * sum((min(ch, (k + 1) * rb) - k * rb + 1) // 2 for k in range(nb))
        max_cell = max(max_cell, cap)
        max_level = max(max_level, min(nc * cap, nc * math.ceil(l["quota"] / nc) + nc * nc + l["quota"] + 64))
    return min(max(max_cell, max_level), 2048)


def _extract(ex, pix, cap, rows=None, gather=None):
    """pix (F, h, w) through orbx_extract_batch_device (or, gather = list of device frames, orbx_extract_batch); outputs have `rows` >= F frames"""
    F, h, w = pix.shape
    rows = rows or F
    k = torch.full((rows, cap, 28), 0xAB, dtype=torch.uint8, device="cuda")
    d = torch.full((rows, cap, 32), 0xAB, dtype=torch.uint8, device="cuda")
    n = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    st = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    if gather is None:
        dev = torch.from_numpy(np.ascontiguousarray(pix)).cuda()
        ex.extract_batch_device(dev.data_ptr(), F, w, h, w, w * h, k.data_ptr(), d.data_ptr(), n.data_ptr(), cap, st.data_ptr())
    else:
        ex.extract_batch(gather, k.data_ptr(), d.data_ptr(), n.data_ptr(), cap, st.data_ptr())
    torch.cuda.synchronize()
    return k.cpu().numpy(), d.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()


def _check(got, want, pick):
    """got: host outputs; want[i] = the oracle's (key points, descriptors) of distinct frame i; frame f shows distinct frame pick[f]"""
    k, d, n, st = got
    for f, i in enumerate(pick):
        ok, od = want[i]
        assert st[f] == 0 and n[f] == len(ok), f
        assert k[f, :n[f]].tobytes() == ok.tobytes() and np.array_equal(d[f, :n[f]], od), f


def _oracle(distinct, g, **kw):
    o = orc.OracleExtractor(dumps=True, **kw)
    want, stats = [], []
    for img in distinct:
        want.append(o(img))
        stats.append(_level_totals(o, g))
    return want, stats


@pytest.fixture(scope="module")
def qvga_blocks():
    """six S-blocks frames of 320x240 and their oracle results (cases a and b)"""
    g = capi.geometry(320, 240, nfeatures=1000)
    distinct = [synth.frame(320, 240, synth.BLOCKS, 900 + i) for i in range(6)]
    want, stats = _oracle(distinct, g, nfeatures=1000)
    return g, distinct, want, stats


@pytest.mark.parametrize("F", [1, 33])
def test_a_small_group_form_and_throughput_form_without_affinity(gpu_extractor_factory, qvga_blocks, F):
    g, distinct, want, stats = qvga_blocks
    assert len(g) == 8 and F < 64 and (F < 32) == (F == 1)
    assert all(sum(t[0] for t in s) > 0 for s in stats)
    pick = np.arange(F) % len(distinct)
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=F)
    _check(_extract(ex, np.stack([distinct[i] for i in pick]), 1000), want, pick)


def test_b_affinity_with_a_padded_group_of_frames(gpu_extractor_factory, qvga_blocks):
    g, distinct, want, stats = qvga_blocks
    F, rows = 67, 72
    assert F >= 64 and F % 8 != 0 and (F + 7) // 8 * 8 == rows                 # blocks of frames 67 .. 71 exist and must do nothing
    pick = (np.arange(F) * 5) % len(distinct)
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=F)
    got = _extract(ex, np.stack([distinct[i] for i in pick]), 1000, rows=rows)
    _check(got, want, pick)
    k, d, n, st = got
    assert (n[F:] == -7).all() and (st[F:] == -7).all() and (k[F:] == 0xAB).all() and (d[F:] == 0xAB).all()


@pytest.mark.parametrize("F", [2, 34])
def test_c_cells_of_several_bands_listed_in_the_record_and_beyond_it(gpu_extractor_factory, F):
    """640x480 with 100 features needs fewer than 8 levels (with 8 the reference's own grid is empty: ORBX_ERR_GEOMETRY); with 3 its four cells
    per level are cut into 10, 7 and 5 bands: levels 1 and 2 take the record's band list, level 0 the generic walk"""
    kw = dict(nfeatures=100, nlevels=3)
    g = capi.geometry(640, 480, **kw)
    bands = _bands_per_cell(g)
    assert any(2 <= nb <= REC_BANDS for nb in bands) and any(nb > REC_BANDS for nb in bands), bands
    distinct = [synth.frame(640, 480, fam, 910 + i) for i, fam in enumerate((synth.BLOCKS, synth.MIDTEX, synth.NOISE))]
    want, stats = _oracle(distinct, g, **kw)
    listed = [l for l, nb in enumerate(bands) if 2 <= nb <= REC_BANDS]
    assert all(s[l][0] > 0 for s in stats for l in listed)                      # those cells do retain key points
    assert any(s[l][1] > SEL_SMALL for s in stats for l in listed) and any(s[l][1] <= SEL_SMALL for s in stats for l in listed)
    pick = np.arange(F) % len(distinct)
    ex = gpu_extractor_factory(device=0, max_batch=F, **kw)
    _check(_extract(ex, np.stack([distinct[i] for i in pick]), 100), want, pick)


def test_d_long_cell_lists_of_a_noise_batch(gpu_extractor_factory):
    g = capi.geometry(640, 480, nfeatures=1000)
    distinct = [synth.frame(640, 480, synth.NOISE, 920 + i) for i in range(4)]
    want, stats = _oracle(distinct, g, nfeatures=1000)
    assert all(s[0][1] > SEL_SMALL for s in stats)                              # level-0 lists for k_cell_select_long ...
    assert all(s[7][1] <= SEL_SMALL for s in stats)                             # ... and short ones beside them
    F = 64
    pick = (np.arange(F) * 3) % len(distinct)
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=F)
    _check(_extract(ex, np.stack([distinct[i] for i in pick]), 1000), want, pick)


def test_d_level_totals_in_all_four_classes_of_the_shared_area(gpu_extractor_factory):
    """With 1000 features no level total of any family leaves the lowest class (a total is about ncells * nfeaturesCell, 240 on level 0, against
    a quarter area of 512 entries): the classes need more features per level.  6000 features on S-noise give totals from about 390 to 1330."""
    kw = dict(nfeatures=6000)
    g = capi.geometry(640, 480, **kw)
    E = _staging_entries(g)
    assert E == 2048
    quarter, third, half = -(-E // 4), -(-E // 3), -(-E // 2)
    distinct = [synth.frame(640, 480, synth.NOISE, 930 + i) for i in range(3)]
    want, stats = _oracle(distinct, g, **kw)
    for s in stats:                                                             # every frame, and inside both chunks of four levels
        work = [t[0] for l, t in enumerate(s) if t[0] > g[l]["quota"] > 0]
        assert any(t <= quarter for t in work) and any(quarter < t <= third for t in work)
        assert any(third < t <= half for t in work) and any(half < t <= E for t in work)
    F = 64
    pick = np.arange(F) % len(distinct)
    ex = gpu_extractor_factory(device=0, max_batch=F, **kw)
    _check(_extract(ex, np.stack([distinct[i] for i in pick]), 6000), want, pick)


@pytest.mark.parametrize("F", [2, 34])
def test_e_empty_lists_nothing_to_retain_and_every_cell_at_the_fallback_threshold(gpu_extractor_factory, F):
    g = capi.geometry(640, 480, nfeatures=1000)
    distinct = [synth.frame(640, 480, synth.FLAT, 0), synth.frame(640, 480, synth.LOWTEX, 940)]
    want, stats = _oracle(distinct, g, nfeatures=1000)
    flat, low = stats
    assert len(want[0][0]) == 0 and all(t[0] == 0 and t[1] == 0 and t[3] == t[4] > 0 for t in flat)     # no corner anywhere: every cell fell back, every list is empty
    assert any(t[2] > 0 and t[0] > 0 for t in low) and any(t[0] == 0 for t in low)                     # cells with nretain = 0 beside cells that retain; empty levels
    assert any(0 < t[0] <= g[l]["quota"] for l, t in enumerate(low))                                  # a level within its quota: k_level_select only stores its count
    pick = np.arange(F) % 2
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=F)
    _check(_extract(ex, np.stack([distinct[i] for i in pick]), 1000), want, pick)


@pytest.mark.parametrize("F", [2, 34])
def test_f_harris_reads_the_level_plane_named_by_the_record(gpu_extractor_factory, F):
    kw = dict(nfeatures=1000, scoreType=orc.HARRIS_SCORE)
    g = capi.geometry(640, 480, nfeatures=1000, scoreType=capi.HARRIS_SCORE)
    distinct = [synth.frame(640, 480, synth.BLOCKS, 950), synth.frame(640, 480, synth.MIDTEX, 951)]
    want, stats = _oracle(distinct, g, **kw)
    assert all(t[0] > 0 for s in stats for t in s)                              # key points on level 0 (the caller's frame) and on every pyramid level
    pick = np.arange(F) % 2
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=F, scoreType=capi.HARRIS_SCORE)
    _check(_extract(ex, np.stack([distinct[i] for i in pick]), 1000), want, pick)


@pytest.mark.parametrize("F,harris", [(3, True), (34, True), (66, False)])
def test_g_pointer_array_form(gpu_extractor_factory, F, harris):
    """k_cell_select_gather / k_cell_select_long_gather: frames in separate allocations of different row strides (Harris reads level 0 there)"""
    w, h = 640, 480
    okw = dict(nfeatures=1000, scoreType=orc.HARRIS_SCORE if harris else orc.FAST_SCORE)
    g = capi.geometry(w, h, nfeatures=1000, scoreType=capi.HARRIS_SCORE if harris else capi.FAST_SCORE)
    distinct = [synth.frame(w, h, fam, 960 + i) for i, fam in enumerate((synth.BLOCKS, synth.NOISE, synth.LOWTEX))]
    want, stats = _oracle(distinct, g, **okw)
    assert any(s[0][1] > SEL_SMALL for s in stats) and any(s[0][1] <= SEL_SMALL for s in stats)
    pick = np.arange(F) % len(distinct)
    frames = []
    for f, i in enumerate(pick):
        stride = w + 16 * (f % 3)
        buf = torch.zeros(stride * h + 64, dtype=torch.uint8, device="cuda")
        view = buf[:stride * h].view(h, stride)[:, :w]
        view.copy_(torch.from_numpy(distinct[i]).cuda())
        frames.append(view)
    ex = gpu_extractor_factory(nfeatures=1000, device=0, max_batch=F, scoreType=capi.HARRIS_SCORE if harris else capi.FAST_SCORE)
    _check(_extract(ex, np.stack([distinct[i] for i in pick]), 1000, gather=frames), want, pick)
