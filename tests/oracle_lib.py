"""ctypes front for oracle/liborb_oracle.so (TEST INFRASTRUCTURE — never imported by the product)."""
import ctypes
import os
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28
HARRIS_SCORE, FAST_SCORE = 0, 1
_LIB = None
c_int, c_float, c_double, c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(ROOT, "oracle", "liborb_oracle.so")
        if not os.path.exists(path):
            raise RuntimeError("oracle/liborb_oracle.so missing: run `make`")
        L = ctypes.CDLL(path)
        L.orc_create.restype = c_void_p
        L.orc_create.argtypes = [c_int, c_float, c_int, c_int, c_int, c_int]
        L.orc_destroy.argtypes = [c_void_p]
        L.orc_keep_dumps.argtypes = [c_void_p, c_int]
        L.orc_extract.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int]
        L.orc_features_per_level.argtypes = [c_void_p, c_int]
        L.orc_scale_factor.argtypes = [c_void_p, c_int]
        L.orc_scale_factor.restype = c_float
        L.orc_inv_scale_factor.argtypes = [c_void_p, c_int]
        L.orc_inv_scale_factor.restype = c_float
        L.orc_umax.argtypes = [c_void_p, c_int]
        L.orc_level_size.argtypes = [c_void_p, c_int, c_void_p, c_void_p]
        L.orc_level_plane.argtypes = [c_void_p, c_int, c_int, c_void_p]
        L.orc_level_keypoints.argtypes = [c_void_p, c_int, c_void_p, c_int]
        L.orc_num_cells.argtypes = [c_void_p]
        L.orc_cell.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int]
        L.orc_cvRound.argtypes = [c_double]
        L.orc_cvFloor.argtypes = [c_double]
        L.orc_cvCeil.argtypes = [c_double]
        L.orc_fastAtan2.argtypes = [c_float, c_float]
        L.orc_fastAtan2.restype = c_float
        L.orc_reflect101.argtypes = [c_int, c_int]
        L.orc_gaussian_kernel_q8.argtypes = [c_void_p]
        L.orc_resize_linear_8u.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int]
        L.orc_fast.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]
        L.orc_gaussian_blur7.argtypes = [c_void_p, c_int, c_int, c_int]
        L.orc_retain_best.argtypes = [c_void_p, c_int, c_int, c_void_p]
        L.orc_sincosf.argtypes = [c_float, c_void_p, c_void_p]
        L.orc_nth_element_perm.argtypes = [c_void_p, c_int, c_int, c_void_p]
        L.orc_hamming256.argtypes = [c_void_p, c_void_p]
        L.orc_match_top2.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
        L.orc_match_top2_popcountll.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
        L.orc_count_accepted.argtypes = [c_void_p, c_void_p, c_int, c_int, c_float]
        L.orc_match_top2_segments.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        L.orc_frame_bounds.argtypes = [c_void_p, c_void_p]
        L.orc_frame_undistort.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
        L.orc_frame_grid.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
        L.orc_frame_features_in_area.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_int, c_int, c_void_p]
        L.orc_search_by_bow.argtypes = [c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                        c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
        L.orc_distinctive.argtypes = [c_void_p, c_int, c_void_p]
        L.orc_search_by_bow_kf.argtypes = [c_int, c_float, c_int] + [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int] * 2 + [c_void_p, c_void_p]
        L.orc_check_dist_epipolar_line.argtypes = [c_float, c_float, c_float, c_float, c_void_p, c_float]
        L.orc_search_for_triangulation.argtypes = [c_int, c_int, c_void_p, c_void_p] + [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int] * 2 + [c_void_p] * 4
        L.orc_sim3_agreement.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p]
        L.orc_three_maxima.argtypes = [c_void_p, c_int, c_void_p]
        L.orc_window_search.argtypes = [c_void_p, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
        L.orc_voc_load_text.restype = c_void_p
        L.orc_voc_load_text.argtypes = [ctypes.c_char_p]
        L.orc_voc_create.restype = c_void_p
        L.orc_voc_create.argtypes = [c_int] * 5 + [c_void_p] * 4
        L.orc_voc_destroy.argtypes = [c_void_p]
        L.orc_voc_info.argtypes = [c_void_p] * 7
        L.orc_forb_distance.argtypes = [c_void_p, c_void_p]
        L.orc_voc_descend.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
        L.orc_voc_transform.argtypes = [c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 7
        L.orc_voc_score.restype = c_double
        L.orc_voc_score.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int]
        _LIB = L
    return _LIB


class OracleExtractor:
    """Mirror of the reference constructor ORBextractor(nfeatures, scaleFactor, nlevels, scoreType, fastTh)."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, scoreType=FAST_SCORE, fastTh=20, blur_mode=0, dumps=False, fp_contract=False):
        self.L = lib()
        self.nfeatures, self.nlevels = nfeatures, nlevels
        self.h = self.L.orc_create(nfeatures, scaleFactor, nlevels, scoreType, fastTh, blur_mode)
        assert self.h
        self.L.orc_keep_dumps(self.h, 1 if dumps else 0)
        self.L.orc_set_fp_contract.argtypes = [c_void_p, c_int]
        self.L.orc_set_fp_contract(self.h, 1 if fp_contract else 0)     # the float expressions as the reference's own build flags contract them

    def __del__(self):
        if getattr(self, "h", None):
            self.L.orc_destroy(self.h)
            self.h = None

    def __call__(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        hh, w = img.shape
        cap = max(2 * self.nfeatures, 16)
        kps = np.zeros(cap, dtype=KP_DTYPE)
        desc = np.zeros((cap, 32), dtype=np.uint8)
        n = self.L.orc_extract(self.h, img.ctypes.data, w, hh, img.strides[0], kps.ctypes.data, desc.ctypes.data, cap)
        if n < 0:
            raise RuntimeError("oracle extract error %d" % n)
        return kps[:n].copy(), desc[:n].copy()

    def features_per_level(self):
        return [self.L.orc_features_per_level(self.h, l) for l in range(self.nlevels)]

    def scale_factors(self):
        return np.array([self.L.orc_scale_factor(self.h, l) for l in range(self.nlevels)], dtype=np.float32)

    def umax(self):
        return [self.L.orc_umax(self.h, v) for v in range(16)]

    def level_size(self, level):
        w, hh = c_int(), c_int()
        self.L.orc_level_size(self.h, level, ctypes.byref(w), ctypes.byref(hh))
        return w.value, hh.value

    def level_plane(self, level, which=0):
        w, hh = self.level_size(level)
        shape = (hh + 32, w + 32) if which == 2 else (hh, w)
        out = np.empty(shape, dtype=np.uint8)
        self.L.orc_level_plane(self.h, level, which, out.ctypes.data)
        return out

    def level_keypoints(self, level):
        cap = 4 * self.nfeatures + 16
        out = np.zeros(cap, dtype=KP_DTYPE)
        n = self.L.orc_level_keypoints(self.h, level, out.ctypes.data, cap)
        assert n >= 0
        return out[:n].copy()

    def cells(self):
        res = []
        for i in range(self.L.orc_num_cells(self.h)):
            info = (c_int * 8)()
            n = self.L.orc_cell(self.h, i, info, None, 0)
            out = np.zeros(max(n, 1), dtype=KP_DTYPE)
            self.L.orc_cell(self.h, i, info, out.ctypes.data, max(n, 1))
            res.append((tuple(info), out[:n].copy()))
        return res


def hamming256(a, b):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    return lib().orc_hamming256(a.ctypes.data, b.ctypes.data)


def match_top2(Q, T):
    Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 32)
    nq, nt = len(Q), len(T)
    idx = np.empty(nq, np.int32); best = np.empty(nq, np.int32); sec = np.empty(nq, np.int32)
    lib().orc_match_top2(Q.ctypes.data, nq, T.ctypes.data, nt, idx.ctypes.data, best.ctypes.data, sec.ctypes.data)
    return idx, best, sec


def match_top2_popcountll(Q, T):
    """the CPU-baseline variant of match_top2 (one popcount instruction per 64-bit word); same integers"""
    Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 32)
    nq, nt = len(Q), len(T)
    idx = np.empty(nq, np.int32); best = np.empty(nq, np.int32); sec = np.empty(nq, np.int32)
    lib().orc_match_top2_popcountll(Q.ctypes.data, nq, T.ctypes.data, nt, idx.ctypes.data, best.ctypes.data, sec.ctypes.data)
    return idx, best, sec


def fast(img, threshold, want_scores=False):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    hh, w = img.shape
    cap = w * hh // 4 + 16
    out = np.zeros(cap, dtype=KP_DTYPE)
    sc = np.zeros((hh, w), dtype=np.uint8) if want_scores else None
    n = lib().orc_fast(img.ctypes.data, w, hh, img.strides[0], threshold, out.ctypes.data, cap,
                       sc.ctypes.data if want_scores else None)
    assert n >= 0
    return (out[:n].copy(), sc) if want_scores else out[:n].copy()


def resize_linear(src, dw, dh):
    src = np.ascontiguousarray(src, dtype=np.uint8)
    sh, sw = src.shape
    dst = np.empty((dh, dw), dtype=np.uint8)
    lib().orc_resize_linear_8u(src.ctypes.data, sw, sh, src.strides[0], dst.ctypes.data, dw, dh, dw)
    return dst


def gaussian_blur7(img, blur_mode=0):
    out = np.ascontiguousarray(img, dtype=np.uint8).copy()
    lib().orc_gaussian_blur7(out.ctypes.data, out.shape[1], out.shape[0], blur_mode)
    return out


def retain_best(responses, n):
    r = np.ascontiguousarray(responses, dtype=np.float32)
    out = np.empty(max(n, 1), dtype=np.int32)
    m = lib().orc_retain_best(r.ctypes.data, len(r), n, out.ctypes.data)
    return out[:m].copy()


def nth_element_perm(responses, nth):
    r = np.ascontiguousarray(responses, dtype=np.float32)
    out = np.empty(len(r), dtype=np.int32)
    lib().orc_nth_element_perm(r.ctypes.data, len(r), nth, out.ctypes.data)
    return out


def match_top2_segments(Q, T, seg_off, cand):
    Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 32)
    seg = np.ascontiguousarray(seg_off, dtype=np.int32)
    cd = np.ascontiguousarray(cand, dtype=np.int32)
    nq = len(Q)
    idx = np.empty(nq, np.int32); best = np.empty(nq, np.int32); sec = np.empty(nq, np.int32)
    lib().orc_match_top2_segments(Q.ctypes.data, nq, T.ctypes.data, len(T), seg.ctypes.data, cd.ctypes.data if len(cd) else None,
                                  idx.ctypes.data, best.ctypes.data, sec.ctypes.data)
    return idx, best, sec


class _VocBase:
    """shared marshalling for the oracle vocabulary (prefix 'orc_') and the compiled reference (prefix 'ref_')"""
    PFX = "orc_"

    def _f(self, name):
        return getattr(self.L, self.PFX + name)

    def descend(self, desc, levelsup=4):
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        n = len(desc)
        word = np.zeros(n, np.uint32); weight = np.zeros(n, np.float64); node = np.zeros(n, np.uint32)
        self._f("voc_descend")(self.h, desc.ctypes.data, n, levelsup, word.ctypes.data, weight.ctypes.data, node.ctypes.data)
        return word, weight, node

    def transform(self, desc, levelsup=4):
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        bid = np.zeros(m, np.uint32); bval = np.zeros(m, np.float64)
        fnode = np.zeros(m, np.uint32); foff = np.zeros(m + 1, np.int32); ffeat = np.zeros(m, np.uint32)
        nb, nf = ctypes.c_int(), ctypes.c_int()
        self._f("voc_transform")(self.h, desc.ctypes.data, n, levelsup, bid.ctypes.data, bval.ctypes.data, ctypes.byref(nb),
                                 fnode.ctypes.data, foff.ctypes.data, ffeat.ctypes.data, ctypes.byref(nf))
        return bid[:nb.value], bval[:nb.value], fnode[:nf.value], foff[:nf.value + 1], ffeat[:foff[nf.value]]

    def score(self, ids1, vals1, ids2, vals2):
        a = np.ascontiguousarray(ids1, dtype=np.uint32); av = np.ascontiguousarray(vals1, dtype=np.float64)
        b = np.ascontiguousarray(ids2, dtype=np.uint32); bv = np.ascontiguousarray(vals2, dtype=np.float64)
        return self._f("voc_score")(self.h, a.ctypes.data, av.ctypes.data, len(a), b.ctypes.data, bv.ctypes.data, len(b))

    def __del__(self):
        if getattr(self, "h", None):
            self._f("voc_destroy")(self.h)
            self.h = None


class OracleVocabulary(_VocBase):
    def __init__(self, path=None, voc=None, scoring=0, weighting=0):
        self.L = lib()
        if path is not None:
            self.h = self.L.orc_voc_load_text(os.fsencode(path))
        else:
            p = np.ascontiguousarray(voc["parent"], dtype=np.int32)
            lf = np.ascontiguousarray(voc["is_leaf"], dtype=np.uint8)
            d = np.ascontiguousarray(voc["desc"], dtype=np.uint8)
            w = np.ascontiguousarray(voc["weight"], dtype=np.float64)
            self.h = self.L.orc_voc_create(voc["k"], voc["L"], scoring, weighting, len(p), p.ctypes.data, lf.ctypes.data, d.ctypes.data, w.ctypes.data)
        assert self.h, "vocabulary load failed"

    def info(self):
        vals = [ctypes.c_int() for _ in range(6)]
        self.L.orc_voc_info(self.h, *[ctypes.byref(x) for x in vals])
        return dict(zip(("k", "L", "scoring", "weighting", "n_words", "n_nodes"), [x.value for x in vals]))


REF_DIR = os.path.join(ROOT, "oracle", "_ref")


def ref_available():
    return os.path.exists(os.path.join(REF_DIR, "libref_orbextractor.so")) and os.path.exists(os.path.join(REF_DIR, "libref_dbow2.so"))


_REF = {}


NATIVE_DIR = os.path.join(REF_DIR, "native")


def native_available():
    return os.path.exists(os.path.join(NATIVE_DIR, "libref_orbextractor.so"))


def ref_lib(name, native=False):
    """the reference's own sources compiled against oracle/cvstub (oracle/Makefile → oracle/_ref/; native: → oracle/_ref/native/, the
    extractor built with the reference's own optimisation flags, i.e. with GCC's default FMA contraction)"""
    key = ("native:" if native else "") + name
    if key in _REF:
        return _REF[key]
    if True:
        lib()     # liborb_oracle.so first: the stand-in cv primitives resolve into it
        R = ctypes.CDLL(os.path.join(NATIVE_DIR if native else REF_DIR, name), mode=ctypes.RTLD_LOCAL if native else ctypes.RTLD_GLOBAL)
        if name == "libref_orbextractor.so":
            R.ref_orb_create.restype = c_void_p
            R.ref_orb_create.argtypes = [c_int, c_float, c_int, c_int, c_int]
            R.ref_orb_destroy.argtypes = [c_void_p]
            R.ref_orb_levels.argtypes = [c_void_p]
            R.ref_orb_scale_factor.argtypes = [c_void_p]
            R.ref_orb_scale_factor.restype = c_float
            R.ref_orb_extract.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int]
            R.cvstub_set_blur_mode.argtypes = [c_int]
        else:
            R.ref_voc_load_text.restype = c_void_p
            R.ref_voc_load_text.argtypes = [ctypes.c_char_p]
            R.ref_voc_destroy.argtypes = [c_void_p]
            R.ref_voc_info.argtypes = [c_void_p] * 6
            R.ref_forb_distance.argtypes = [c_void_p, c_void_p]
            R.ref_voc_descend.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
            R.ref_voc_transform.argtypes = [c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 7
            R.ref_voc_score.restype = c_double
            R.ref_voc_score.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int]
        _REF[key] = R
    return _REF[key]


class RefExtractor:
    """ORB_SLAM::ORBextractor compiled from /root/reference/src/ORBextractor.cc (OpenCV primitives = the oracle's)"""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, scoreType=FAST_SCORE, fastTh=20, blur_mode=0, native=False):
        self.R = ref_lib("libref_orbextractor.so", native=native)
        self.blur_mode = blur_mode
        self.nfeatures = nfeatures
        self.h = self.R.ref_orb_create(nfeatures, scaleFactor, nlevels, scoreType, fastTh)

    def __del__(self):
        if getattr(self, "h", None):
            self.R.ref_orb_destroy(self.h)
            self.h = None

    def __call__(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        hh, w = img.shape
        cap = max(2 * self.nfeatures, 16)
        kps = np.zeros(cap, dtype=KP_DTYPE)
        desc = np.zeros((cap, 32), dtype=np.uint8)
        self.R.cvstub_set_blur_mode(self.blur_mode)
        n = self.R.ref_orb_extract(self.h, img.ctypes.data, w, hh, img.strides[0], kps.ctypes.data, desc.ctypes.data, cap)
        assert n >= 0, "reference extractor failed: %d" % n
        return kps[:n].copy(), desc[:n].copy()


class RefVocabulary(_VocBase):
    """ORB_SLAM::ORBVocabulary compiled from the reference's vendored DBoW2 sources"""
    PFX = "ref_"

    def __init__(self, path):
        self.L = ref_lib("libref_dbow2.so")
        self.h = self.L.ref_voc_load_text(os.fsencode(path))
        assert self.h, "reference loadFromTextFile failed"

    def info(self):
        vals = [ctypes.c_int() for _ in range(5)]
        self.L.ref_voc_info(self.h, *[ctypes.byref(x) for x in vals])
        return dict(zip(("k", "L", "scoring", "weighting", "n_words"), [x.value for x in vals]))


# ---- Frame-side steps (oracle/frame_oracle.cpp).  cam / bounds are ctypes structs with the layout of orbf_camera /
# orbf_bounds (tests pass orb_slam_amd.capi.Camera / Bounds: plain data carriers, no product code runs here).
def frame_bounds(cam, bounds_cls):
    b = bounds_cls()
    lib().orc_frame_bounds(ctypes.addressof(cam), ctypes.addressof(b))
    return b


def frame_undistort(cam, kps):
    kps = np.ascontiguousarray(kps, dtype=KP_DTYPE)
    out = np.zeros(len(kps), dtype=KP_DTYPE)
    lib().orc_frame_undistort(ctypes.addressof(cam), kps.ctypes.data, len(kps), out.ctypes.data)
    return out


def frame_grid(bounds, kps_un):
    kps_un = np.ascontiguousarray(kps_un, dtype=KP_DTYPE)
    off = np.zeros(64 * 48 + 1, np.int32)
    feat = np.zeros(max(len(kps_un), 1), np.int32)
    lib().orc_frame_grid(ctypes.addressof(bounds), kps_un.ctypes.data, len(kps_un), off.ctypes.data, feat.ctypes.data)
    return off, feat[:off[-1]]


def frame_features_in_area(bounds, kps_un, cell_off, cell_feat, x, y, r, min_level, max_level):
    kps_un = np.ascontiguousarray(kps_un, dtype=KP_DTYPE)
    out = np.zeros(max(len(kps_un), 1), np.int32)
    n = lib().orc_frame_features_in_area(ctypes.addressof(bounds), kps_un.ctypes.data, cell_off.ctypes.data, cell_feat.ctypes.data,
                                         x, y, r, min_level, max_level, out.ctypes.data)
    return out[:n]


def three_maxima(sizes):
    sz = np.ascontiguousarray(sizes, dtype=np.int32)
    out = np.zeros(3, np.int32)
    lib().orc_three_maxima(sz.ctypes.data, len(sz), out.ctypes.data)
    return tuple(int(v) for v in out)


def window_search(bounds, rule, th, ratio, check_orientation, kps_un, desc, cell_off, cell_feat, claimed, qxyr, qlev, qdesc, qangle, qvalid):
    """one greedy grid-window search problem (oracle/search_oracle.cpp): -> (nmatches, q2t, t2q, best, second)"""
    kps_un = np.ascontiguousarray(kps_un, dtype=KP_DTYPE)
    desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
    qxyr = np.ascontiguousarray(qxyr, dtype=np.float32).reshape(-1, 3)
    qlev = np.ascontiguousarray(qlev, dtype=np.int32).reshape(-1, 2)
    qdesc = np.ascontiguousarray(qdesc, dtype=np.uint8).reshape(-1, 32)
    nt, nq = len(kps_un), len(qxyr)
    cell_off = np.ascontiguousarray(cell_off, dtype=np.int32)
    cell_feat = np.ascontiguousarray(cell_feat, dtype=np.int32)
    cl = None if claimed is None else np.ascontiguousarray(claimed, dtype=np.uint8)
    qa = None if qangle is None else np.ascontiguousarray(qangle, dtype=np.float32)
    qv = None if qvalid is None else np.ascontiguousarray(qvalid, dtype=np.uint8)
    q2t = np.zeros(max(nq, 1), np.int32); t2q = np.zeros(max(nt, 1), np.int32)
    best = np.zeros(max(nq, 1), np.int32); second = np.zeros(max(nq, 1), np.int32)
    n = lib().orc_window_search(ctypes.addressof(bounds), rule, th, ratio, 1 if check_orientation else 0, kps_un.ctypes.data, desc.ctypes.data,
                                cell_off.ctypes.data, cell_feat.ctypes.data, nt, cl.ctypes.data if cl is not None else None,
                                qxyr.ctypes.data, qlev.ctypes.data, qdesc.ctypes.data, qa.ctypes.data if qa is not None else None,
                                qv.ctypes.data if qv is not None else None, nq, q2t.ctypes.data, t2q.ctypes.data, best.ctypes.data, second.ctypes.data)
    return n, q2t[:nq], t2q[:nt], best[:nq], second[:nq]


def distinctive(desc):
    """one map point's observed descriptors -> (BestIdx, BestMedian)"""
    desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
    med = ctypes.c_int32()
    idx = lib().orc_distinctive(desc.ctypes.data if len(desc) else None, len(desc), ctypes.byref(med))
    return idx, med.value


def search_by_bow(th, ratio, check_orientation, kf_fv, kf_desc, kf_angle, kf_valid, f_fv, f_desc, f_angle):
    """ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) on flattened arrays; *_fv = (nodes, off, feat) FeatureVector CSR.
    -> (nmatches, q2t[nKF], t2q[nF], best[nKF], second[nKF])"""
    kn, ko, kf = (np.ascontiguousarray(kf_fv[0], dtype=np.uint32), np.ascontiguousarray(kf_fv[1], dtype=np.int32), np.ascontiguousarray(kf_fv[2], dtype=np.uint32))
    fn, fo, ff = (np.ascontiguousarray(f_fv[0], dtype=np.uint32), np.ascontiguousarray(f_fv[1], dtype=np.int32), np.ascontiguousarray(f_fv[2], dtype=np.uint32))
    kd = np.ascontiguousarray(kf_desc, dtype=np.uint8).reshape(-1, 32); fd = np.ascontiguousarray(f_desc, dtype=np.uint8).reshape(-1, 32)
    ka = np.ascontiguousarray(kf_angle, dtype=np.float32); fa = np.ascontiguousarray(f_angle, dtype=np.float32)
    kv = np.ascontiguousarray(kf_valid, dtype=np.uint8)
    nK, nF = len(kd), len(fd)
    q2t = np.zeros(max(nK, 1), np.int32); t2q = np.zeros(max(nF, 1), np.int32); best = np.zeros(max(nK, 1), np.int32); second = np.zeros(max(nK, 1), np.int32)
    n = lib().orc_search_by_bow(th, ratio, 1 if check_orientation else 0, kn.ctypes.data, ko.ctypes.data, kf.ctypes.data, len(kn), kd.ctypes.data,
                                ka.ctypes.data, kv.ctypes.data, nK, fn.ctypes.data, fo.ctypes.data, ff.ctypes.data, len(fn), fd.ctypes.data, fa.ctypes.data, nF,
                                q2t.ctypes.data, t2q.ctypes.data, best.ctypes.data, second.ctypes.data)
    return n, q2t[:nK], t2q[:nF], best[:nK], second[:nK]


def _fv(fv):
    return (np.ascontiguousarray(fv[0], dtype=np.uint32), np.ascontiguousarray(fv[1], dtype=np.int32), np.ascontiguousarray(fv[2], dtype=np.uint32))


def search_by_bow_kf(th_low, ratio, check_orientation, fv1, desc1, angle1, valid1, fv2, desc2, angle2, valid2):
    """ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) -> (nmatches, q2t[n1], t2q[n2])"""
    n1_, o1, f1 = _fv(fv1); n2_, o2, f2 = _fv(fv2)
    d1 = np.ascontiguousarray(desc1, dtype=np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(desc2, dtype=np.uint8).reshape(-1, 32)
    a1 = np.ascontiguousarray(angle1, dtype=np.float32); a2 = np.ascontiguousarray(angle2, dtype=np.float32)
    v1 = np.ascontiguousarray(valid1, dtype=np.uint8); v2 = np.ascontiguousarray(valid2, dtype=np.uint8)
    N1, N2 = len(d1), len(d2)
    q2t = np.zeros(max(N1, 1), np.int32); t2q = np.zeros(max(N2, 1), np.int32)
    n = lib().orc_search_by_bow_kf(th_low, ctypes.c_float(ratio), 1 if check_orientation else 0, n1_.ctypes.data, o1.ctypes.data, f1.ctypes.data, len(n1_),
                                   d1.ctypes.data, a1.ctypes.data, v1.ctypes.data, N1, n2_.ctypes.data, o2.ctypes.data, f2.ctypes.data, len(n2_),
                                   d2.ctypes.data, a2.ctypes.data, v2.ctypes.data, N2, q2t.ctypes.data, t2q.ctypes.data)
    return n, q2t[:N1], t2q[:N2]


def check_dist_epipolar_line(x1, y1, x2, y2, F12, sigma2):
    F = np.ascontiguousarray(F12, dtype=np.float32).reshape(9)
    f = ctypes.c_float
    return bool(lib().orc_check_dist_epipolar_line(f(x1), f(y1), f(x2), f(y2), F.ctypes.data, f(sigma2)))


def search_for_triangulation(th_low, check_orientation, F12, level_sigma2, fv1, kps1, desc1, has_mp1, fv2, kps2, desc2, has_mp2):
    """ORBmatcher::SearchForTriangulation -> (nmatches, q2t[n1] (= vMatches12), t2q[n2], best[n1], second[n1])"""
    n1_, o1, f1 = _fv(fv1); n2_, o2, f2 = _fv(fv2)
    F = np.ascontiguousarray(F12, dtype=np.float32).reshape(9)
    s2 = np.ascontiguousarray(level_sigma2, dtype=np.float32)
    k1 = np.ascontiguousarray(kps1); k2 = np.ascontiguousarray(kps2)
    d1 = np.ascontiguousarray(desc1, dtype=np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(desc2, dtype=np.uint8).reshape(-1, 32)
    m1 = np.ascontiguousarray(has_mp1, dtype=np.uint8); m2 = np.ascontiguousarray(has_mp2, dtype=np.uint8)
    N1, N2 = len(d1), len(d2)
    q2t = np.zeros(max(N1, 1), np.int32); t2q = np.zeros(max(N2, 1), np.int32); best = np.zeros(max(N1, 1), np.int32); second = np.zeros(max(N1, 1), np.int32)
    n = lib().orc_search_for_triangulation(th_low, 1 if check_orientation else 0, F.ctypes.data, s2.ctypes.data, n1_.ctypes.data, o1.ctypes.data, f1.ctypes.data,
                                           len(n1_), k1.ctypes.data, d1.ctypes.data, m1.ctypes.data, N1, n2_.ctypes.data, o2.ctypes.data, f2.ctypes.data,
                                           len(n2_), k2.ctypes.data, d2.ctypes.data, m2.ctypes.data, N2, q2t.ctypes.data, t2q.ctypes.data, best.ctypes.data,
                                           second.ctypes.data)
    return n, q2t[:N1], t2q[:N2], best[:N1], second[:N1]


def sim3_agreement(m12, m21):
    a = np.ascontiguousarray(m12, dtype=np.int32); b = np.ascontiguousarray(m21, dtype=np.int32)
    out = np.zeros(max(len(a), 1), np.int32)
    n = lib().orc_sim3_agreement(a.ctypes.data, len(a), b.ctypes.data, len(b), out.ctypes.data)
    return n, out[:len(a)]
