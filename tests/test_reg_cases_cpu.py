"""The designed sheet of tests/reg_cases.py on the CPU: the oracle's fill-holes, regulariser and updateKeyframe passes decide every pixel
as reg_cases.census predicts (so the sheet reaches the decision classes it claims to: both K5 thresholds, the blacklist clause, the
un-blacklisting, K6's keep threshold and occlusion test, a created pixel rejected in the same pass, Frame::setDepth's -0.05 rule, the codes
of the re-activation variance plane), the class x position table has no empty cell that can be filled, and — where oracle/_ref has been
built — the oracle equals the compiled reference bit for bit on the same sheets."""
import numpy as np
import pytest

import reg_cases as rc
from test_gpu_parity import assert_hyp_equal

SIZES = [(176, 144), (320, 240)]
IDENT8 = np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0])


def camera(w, h):
    return np.array([0.8 * w, 0.8 * w, 0.5 * w - 0.5, 0.5 * h - 0.5], np.float32)


def image(w, h, seed=0):
    return np.random.default_rng(1234 + seed).integers(0, 256, (h, w)).astype(np.uint8)


class Side:
    """one library's keyframe + map holding a sheet (L = None: the oracle, else the compiled reference)"""

    def __init__(self, oracle, w, h, hyp, mg, L=None, min_use_grad=None):
        self.o, self.L, self.w, self.h = oracle, L, w, h
        self.K = camera(w, h)
        self.op = oracle.default_params(L) if L is not None else oracle.default_params()
        assert self.op.minUseGrad == rc.MIN_USE_GRAD
        if min_use_grad is not None:          # a sheet built for a moved threshold (rc.build(..., min_use_grad=))
            self.op.minUseGrad = min_use_grad
        self.kf = oracle.Frame(0, image(w, h), self.K, L=L)
        self.kf.set_maxgrad(mg)
        none = np.full((h, w), -1, np.float32)
        self.kf.set_depth_planes(none, none)
        self.dm = oracle.DepthMap(w, h, self.K, params=self.op, L=L, threads=1)
        self.dm.init_gt(self.kf)          # (makes the map cache the keyframe's image, which a raw overwrite alone does not)
        self.hyp = hyp
        self.reset()

    def reset(self):
        self.dm.set(self.kf, self.hyp)

    def tracked(self, id_=1):
        """a frame tracked on the keyframe whose refPixelWasGood mask is all zero: observeDepth looks at no pixel of the sheet"""
        f = self.o.Frame(id_, image(self.w, self.h, id_), self.K, L=self.L)
        f.set_pose(IDENT8, self.kf, 0.3)
        f.set_wasgood(np.zeros((self.h >> 1, self.w >> 1), np.uint8))
        return f

    def run(self, entry):
        if entry in ("fillholes", "regularize", "regularize_occ"):
            self.dm.stage(entry)
        elif entry == "update":
            self.kf.set_counters(7, 3, 3, 0)       # due for Frame::setDepth
            self.dm.update([self.tracked()])
        elif entry == "finalize":
            self.dm.finalize()
        return self.dm.get()


ENTRIES = [("fillholes", "fillholes"), ("regularize", "regularize"), ("regularize_occ", "regularize_occ"), ("update", "fill_regularize"),
           ("finalize", "fill_regularize")]


def test_hyp_dtype_is_the_oracles(oracle):
    assert rc.HYP_DTYPE == oracle.HYP_DTYPE


def assert_cells_keep_apart(cl):
    c = np.array([(cx, cy) for cx, cy, _, _ in cl])
    for i in range(0, len(c), 512):
        d = np.maximum(np.abs(c[i:i + 512, None, 0] - c[None, :, 0]), np.abs(c[i:i + 512, None, 1] - c[None, :, 1]))
        d[np.arange(len(d)), np.arange(i, i + len(d))] = 99
        assert d.min() >= rc.PITCH


@pytest.mark.parametrize("w,h", SIZES)
def test_class_position_table_has_no_empty_cell(w, h):
    """a condition on the inputs: over the VARIANTS sheets of a size every decision class stands at every position class it can stand at.
    Fails if an edit of the sheet loses a case."""
    lists = [rc.cells(w, h, v) for v in range(rc.VARIANTS)]
    t = rc.table(lists)
    print(rc.format_table(t, w, h))
    assert rc.empty_cells(t, w, h) == []
    for cl in lists:       # no two centres closer than PITCH in both axes
        assert_cells_keep_apart(cl)


def test_class_position_table_1024x512_one_sheet():
    """the single-map size with 32x16 tiles runs ONE sheet: it holds every class at every position except the image-edge lines (x = 1, 2, 3,
    w - 3, w - 2 and the same in y are one lattice line each, shorter than the list of classes; 176x144 covers them under the same tile code)"""
    w, h = 1024, 512
    cl = rc.cells(w, h, 0)
    t = rc.table(cl)
    print(rc.format_table(t, w, h))
    assert [e for e in rc.empty_cells(t, w, h) if e[1] not in rc.EDGE_TAGS] == []
    assert_cells_keep_apart(cl)


@pytest.mark.parametrize("variant", range(rc.VARIANTS))
@pytest.mark.parametrize("w,h", SIZES)
def test_oracle_decides_as_the_census_predicts(oracle, w, h, variant):
    oracle_decides_as_the_census_predicts(oracle, w, h, variant)


def oracle_decides_as_the_census_predicts(oracle, w, h, variant, min_use_grad=None):
    """min_use_grad: None = the default threshold, else the sheet, the oracle's map and the census all at that value"""
    th = rc.MIN_USE_GRAD if min_use_grad is None else float(np.float32(min_use_grad))
    hyp, mg = rc.build(w, h, variant, th)
    cl = rc.cells(w, h, variant)
    s = Side(oracle, w, h, hyp, mg, min_use_grad=min_use_grad)
    assert s.op.minUseGrad == np.float32(th)
    for entry, stage in ENTRIES:
        what = "oracle %dx%d variant %d minUseGrad %g %s" % (w, h, variant, th, entry)
        s.reset()
        after = s.run(entry)
        want = rc.census(hyp, mg, s.op.minUseGrad, stage)
        assert rc.assert_expectations(want, cl, stage, what) > 0
        rc.assert_decisions(rc.decisions_from_maps(hyp, after, stage), want, cl, what)
        if entry in ("update", "finalize"):
            sd = rc.setdepth_from_planes(s.kf.plane("idepth", 0), s.kf.plane("idepthVar", 0), hyp["idepth_smoothed"])
            rc.assert_decisions({"setdepth": sd}, want, cl, what + " Frame::setDepth", keys=("setdepth",))
            assert s.kf.stats()["numPoints"] == int((want["setdepth"] != rc.SD_NOT_COUNTED).sum())
        if entry == "finalize":
            # the re-activation planes, read through setFromExistingKF's own reading of them on a map of their own (K6 there changes no
            # blacklisted counter of a pixel without a hypothesis, and every hypothesis it sees was one)
            dm2 = oracle.DepthMap(w, h, s.K, params=s.op, threads=1)
            dm2.set_from_existing(s.kf)
            back = dm2.get()
            # a pixel of the planes that held a hypothesis is valid now, or setFromExistingKF's own K6 rejected it (blacklisted 0 - 1 = -1);
            # one that held none has blacklisted -2 or 0
            held = (back["isValid"] > 0) | (back["blacklisted"] == -1)
            code = np.where(held, 1, np.where(back["blacklisted"] == rc.MIN_BLACKLIST - 1, -2, -1))
            v = back["isValid"] > 0
            assert np.array_equal(back["validity_counter"][v], after["validity_counter"][v]), what + ": validity_reAct"
            assert int(back["validity_counter"][v].max()) == 255, what + ": no validity counter of 255 came back"
            rc.assert_decisions({"react": code}, want, cl, what + " re-activation planes", keys=("react",))
            assert (want["react"] == -2).sum() > 0 and (want["react"] == -1).sum() > 0


@pytest.mark.parametrize("variant", range(rc.VARIANTS))
@pytest.mark.parametrize("w,h", SIZES)
def test_oracle_equals_the_compiled_reference_on_the_sheet(oracle, w, h, variant):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref not built (make -C oracle ref, where the reference sources are)")
    R = oracle.lib(ref="sse")
    hyp, mg = rc.build(w, h, variant)
    a, b = Side(oracle, w, h, hyp, mg), Side(oracle, w, h, hyp, mg, L=R)
    for entry, stage in ENTRIES:
        what = "oracle vs reference %dx%d variant %d %s" % (w, h, variant, entry)
        a.reset()
        b.reset()
        ga, gb = a.run(entry), b.run(entry)
        assert_hyp_equal(ga, gb, what)
        # ... and what both leave in the pixels that hold no hypothesis: K5's stores under a K6 rejection in the same pass
        inv = gb["isValid"] == 0
        for k in ("validity_counter", "idepth", "idepth_var"):
            assert np.array_equal(ga[k][inv], gb[k][inv]), what + ": " + k + " of the pixels without a hypothesis"
        if entry in ("update", "finalize"):
            for lvl in range(5):
                for p in ("idepth", "idepthVar"):
                    assert np.array_equal(a.kf.plane(p, lvl).view(np.uint32), b.kf.plane(p, lvl).view(np.uint32)), "%s keyframe %s L%d" % (what, p, lvl)
            assert a.kf.stats()["numPoints"] == b.kf.stats()["numPoints"]
