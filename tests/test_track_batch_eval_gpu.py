"""The batched SE3 evaluation forms entry by entry against float64 sums of the oracle's per-point float32 terms (tests/se3_terms.py, pinned
to the oracle by test_se3_terms_cpu.py), through lsdhip_tracker_evaluate_batch: one evalOnly job per (keyframe, frame, pose, affine pair)
in the launches lsdhip_tracker_track_batch runs.  The whole-trackFrame checks of test_gpu_parity.py (pose, evaluation count, residual,
mask within 0.2 %) cannot see small errors the LM loop absorbs; here every job of every batch must give

  * exactly the oracle's warped_size, goodCount, badCount, num_constraints and (level 1) refPixelWasGood plane;
  * every entry of A and b, lsError, weightedError and retval within

        |device - sum64| <= gamma * EPS * sum|terms| + 1e-30,      EPS = 2^-24,

    sum64 over the first (M // 4) * 4 in-image points (the SSE tail drop; retval: the good points of all M), sum|terms| also over the
    tail the device adds and subtracts again;
  * pointUsage, meanRes and the affine estimate at the single-path test's tolerances, and the same record bits on a second call.

gamma = depth of one term on its way into the total + the record's division (1) + per-term roundings.  The depth per form:
  small batch (k_track_step<256, true>, fewer than 8 jobs): P sequential additions in a lane, P = pixels per lane of the grid-stride loop
    = ceil(w h / (256 nb)), min(16, ceil(w h / 256)) <= nb <= ceil(w h / 256) rounded up to 8 workgroups (batch_shape: at least 16); the LDS fold: a run of
    RRUN = ceil(256 / RSLICE) = 43 lanes (RSLICE = 256 / RS_END = 6 slices of the 41 columns, CPP = RS_END), then the 6 slices (5); the
    finishing launch: K = ceil(nb / 16) rows per row slot (K), the 16 slots (15); the subtraction of up to 3 tail points (3).
    nb is not reported, so P + K is taken at its largest over the nb the rule allows.
  throughput-mode strips (from 8 jobs): P = tilePx / 256 points per lane at most (a strip's list holds at most tilePx points), the same
    fold (43 + 5), K = ceil(nb / 16) with nb = ceil(w h / tilePx) strips (15 for the slots), the tail (3).  The tail points' rows are
    re-evaluated by the strip that holds them with the same arithmetic.
  k_track_solo (coarse levels): at most 9 points per lane (LSD_SOLO_TRIPS), the upper half folded onto the lower (1), a run of
    RRUN = ceil(256 / 12) = 22 (RSLICE = 512 / 41 = 12), the 12 slices (11), the tail (3).
Per-term roundings (the device forms its own terms, with fused multiply-adds and 1-ulp reciprocals; the oracle with separate roundings and
exact reciprocals): the weight w = wh w_p carries at most 47 unit roundings (w_p: 27 — drpdd's 11 doubled by the square, and 5 of its own;
the Huber factor: 18.5 — half of w_p's through the square root, then 5), a Jacobian entry 7, the products 2: per side 63 for an A term,
56 for a b term (r is exact), 49 for lsError's (r w) r, 48 for the weighted error wh (r sqrt(w_p))^2; both sides: 126, 112, 98, 96.
retval's r r: 1.

The test's own power is asserted: the forms ran (`form`), the levels k_track_solo must not take went to the strips, M % 4 took every value
in each form, and a wrong tail (no drop, or the first M % 4 points dropped) violates the bound in each form."""
import numpy as np
import pytest

from common import assert_bit_equal, sequence
from se3_terms import EPS, point_terms, sums64

pytestmark = pytest.mark.gpu

IDENT7 = np.array([1.0, 0, 0, 0, 0, 0, 0], np.float32)
C_TERM = {"A": 126, "b": 112, "err": 98, "werr": 96}


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def ceil_div(a, b):
    return -(-a // b)


def depth_of(form, px, tilePx):
    """the summation depth of one term (module docstring) at a level of px pixels"""
    if form == "solo":
        return 9 + 1 + 22 + 11 + 3
    if form == "strips":
        nb = ceil_div(px, tilePx)
        return tilePx // 256 + 43 + 5 + ceil_div(nb, 16) + 15 + 3
    hi = ceil_div(px, 256)
    lo = min(16, hi)
    hi = max(lo, ceil_div(hi, 8) * 8)        # (fill_level: multiples of 8 from 16 blocks on, at most one block per 256 pixels before that)
    pk = max(ceil_div(px, 256 * nb) + ceil_div(nb, 16) for nb in range(lo, hi + 1))
    return pk + 43 + 5 + 15 + 3


class Scene:
    """one image size: its sequence, a HIP context, keyframes of each kind on both sides"""

    def __init__(self, oracle, hip, w, h, params=None):
        """params: overrides of the context's settings, handed to the oracle's tracker as well (tests/test_settings_gpu.py)"""
        self.w, self.h = w, h
        self.frames, self.depth0, self.K, self.gt = sequence(w, h, 4, 0)
        self.ctx = hip.Context(w, h, self.K, params=params)
        self.op = oracle.default_params()
        for k, v in (params or {}).items():
            setattr(self.op, k, v)
        self.oracle, self.hip = oracle, hip
        self.kfs = {}

    def planes(self, kind, lvl):
        d = self.depth0.copy()
        if kind == "gt":
            return d, None
        if kind == "ragged":
            d[::2, 1::3] = 0
            return d, None
        if kind == "dense":          # a hypothesis on every pixel
            d[~(d > 0)] = np.median(self.depth0[self.depth0 > 0])
            return 1.0 / d, np.full_like(d, 1e-4)
        if kind == "sparse":         # 5 x 7 reference points at level lvl
            s = 1 << lvl
            x0, y0 = (self.w // 2 // s) * s, (self.h // 2 // s) * s
            m = np.zeros_like(d, bool)
            m[y0:y0 + 7 * s, x0:x0 + 5 * s] = True
            d[~m] = 0
            return d, None
        raise ValueError(kind)

    def keyframe(self, kind, lvl):
        key = (kind, lvl if kind == "sparse" else 0)
        if key not in self.kfs:
            d, var = self.planes(kind, lvl)
            kfo = self.oracle.Frame(0, self.frames[0], self.K)
            kfg = self.hip.Frame(self.ctx, 1000 + len(self.kfs), self.frames[0])
            if var is None:
                kfo.set_depth_gt(d, minUseGrad=self.op.minUseGrad)
                kfg.setDepthFromGroundTruth(d)
            else:
                kfo.set_depth_planes(d.astype(np.float32), var.astype(np.float32))
                kfg.setDepthPlanes(d.astype(np.float32), var.astype(np.float32))
            ro = self.oracle.TrackingReference()
            ro.import_frame(kfo)
            rg = self.hip.TrackingReference()
            rg.importFrame(kfg)
            self.kfs[key] = (ro, rg)
        return self.kfs[key]

    def poses(self):
        o = self.oracle
        return [IDENT7, o.se3_inv(self.gt[3]).astype(np.float32),
                o.se3_exp(np.array([0.05, -0.03, 0.02, 0.01, -0.02, 0.03])).astype(np.float32),
                o.se3_inv(self.gt[2]).astype(np.float32)]


OUT_OF_IMAGE = np.array([0.9, 0.1, 0.0, 0.0, 0.35, 0.0])     # most points leave the image
KINDS = ["gt", "ragged", "dense"]
AFFINE = [(1.0, 0.0), (1.03, -2.5), (0.97, 1.5)]


def run_batch(oracle, hip, sc, n, lvl, coarse, stats, form_name, witness=None):
    """n jobs at level lvl; checks every job; returns the forms the device reported.  witness (a list, or None): per checked job
    (form, (oracle reference, oracle frame, pose, level, a, b), float64 sums, the weighted error's bound), for a caller that wants to
    evaluate the same job again under other settings"""
    tr = hip.SE3Tracker(sc.ctx)
    if coarse is not None:
        tr.set_batch_coarse_min_jobs(coarse)
    poses = sc.poses()
    refs_o, refs_g, frs_o, frs_g, Ts, ab, kinds = [], [], [], [], [], [], []
    for j in range(n):
        if j == 1:
            kind = "sparse"                  # a level with fewer than 64 reference points
        else:
            kind = KINDS[(j + lvl) % 3]
        ro, rg = sc.keyframe(kind, lvl)
        kinds.append(kind)
        T = oracle.se3_exp(OUT_OF_IMAGE).astype(np.float32) if j == 2 else poses[(j + lvl) % len(poses)]
        fi = 1 + (j % 3)
        refs_o.append(ro); refs_g.append(rg)
        frs_o.append(oracle.Frame(10 + j, sc.frames[fi], sc.K))
        frs_g.append(hip.Frame(sc.ctx, 10 + j, sc.frames[fi]))
        Ts.append(np.asarray(T, np.float32))
        ab.append(AFFINE[(j + lvl) % 3])
    recs, form = tr.evaluateBatch(refs_g, frs_g, np.array(Ts), lvl, np.array(ab, np.float32))
    recs2, form2 = tr.evaluateBatch(refs_g, frs_g, np.array(Ts), lvl, np.array(ab, np.float32))
    assert np.array_equal(form, form2)
    masks = [f.refPixelWasGoodNoCreate() for f in frs_g] if lvl == 1 else None
    tro = oracle.SE3Tracker(sc.w, sc.h, sc.K, params=sc.op, mode=oracle.SSE_EXACT_RCP)
    px = (sc.w >> lvl) * (sc.h >> lvl)
    for j in range(n):
        tag = "%s %dx%d n=%d level %d job %d" % (form_name, sc.w, sc.h, n, lvl, j)
        g, g2 = recs[j], recs2[j]
        assert bytes(g) == bytes(g2), tag + ": two calls differ"
        solo, tilePx = int(form[j, 0]), int(form[j, 1])
        fname = "solo" if solo else ("strips" if tilePx > 0 else "small")
        a, b = ab[j]
        r_o = tro.evaluate(refs_o[j], frs_o[j], Ts[j], lvl, a, b)
        assert g.warped_size == r_o.warped_size, tag
        assert g.goodCount == r_o.goodCount and g.badCount == r_o.badCount, tag
        if lvl == 1:
            assert_bit_equal(masks[j], frs_o[j].wasgood(), "refPixelWasGood " + tag)
        if r_o.warped_size < 8:
            continue
        assert g.num_constraints == r_o.num_constraints, tag
        # (the oracle adds its M usage terms in float32, one after the other: beyond the single-path test's sizes its own error, M EPS
        # relative, is the larger one)
        assert g.pointUsage == pytest.approx(r_o.pointUsage, rel=max(2e-5, 2 * r_o.warped_size * EPS)), tag
        assert g.meanRes == pytest.approx(r_o.meanRes, rel=max(1e-3, 2 * r_o.warped_size * EPS), abs=1e-4), tag
        if kinds[j] in ("gt", "ragged"):
            # (syy - sy^2 / sw is ill-conditioned; the single-path tolerances hold for the scenes they were set on, not for the flat
            # image regions the dense keyframe adds)
            assert g.affine_a_lastIt == pytest.approx(r_o.affine_a_lastIt, rel=5e-4), tag
            assert g.affine_b_lastIt == pytest.approx(r_o.affine_b_lastIt, abs=0.08), tag
        P = point_terms(tro, frs_o[j], lvl, Ts[j])
        S = sums64(P)
        M, n4, nc = P["M"], S["n4"], r_o.num_constraints
        depth = depth_of(fname, px, tilePx) + 1
        dev = {"A": np.array([np.float64(g.A[6 * i + k]) * nc for i in range(6) for k in range(i, 6)]),
               "b": np.array(g.b, np.float64) * nc, "err": np.float64(g.lsError) * nc, "werr": np.float64(g.weightedError) * n4}
        st = stats.setdefault(fname, {"ratio": 0.0, "mod4": set(), "wrong_tail": False, "levels": set()})
        st["mod4"].add(M % 4)
        st["levels"].add((sc.w, sc.h, lvl))
        for k in ("A", "b", "err", "werr"):
            bound = (depth + C_TERM[k]) * EPS * S[k + "_abs"] + 1e-30
            ratio = np.max(np.abs(dev[k] - S[k]) / bound)
            st["ratio"] = max(st["ratio"], float(ratio))
            assert ratio <= 1, (tag, k, ratio, dev[k], S[k])
            if M % 4:
                for wrong in ("none", "first"):
                    if np.any(np.abs(dev[k] - sums64(P, wrong)[k]) > bound):
                        st["wrong_tail"] = True
        G = S["good"]
        if witness is not None:
            witness.append((fname, (refs_o[j], frs_o[j], Ts[j], lvl, a, b), S, (depth + C_TERM["werr"]) * EPS * S["werr_abs"] + 1e-30))
        bound = (depth + 1) * EPS * S["res2_abs"] + EPS * abs(S["res2"])     # + retval's division
        assert abs(np.float64(g.retval) * G - S["res2"]) <= bound, tag
        sbound = (depth + 1) * EPS * S["signed_abs"] + EPS * abs(S["signed"]) + 1e-30     # meanRes: the signed residuals of the good points
        assert abs(np.float64(g.meanRes) * G - S["signed"]) <= sbound, tag
        st["ratio"] = max(st["ratio"], float(abs(np.float64(g.retval) * G - S["res2"]) / bound))
    return form


@pytest.fixture(scope="module")
def scenes(oracle, hip):
    cache = {}

    def get(w, h):
        if (w, h) not in cache:
            cache[(w, h)] = Scene(oracle, hip, w, h)
        return cache[(w, h)]
    return get


def report(stats, name):
    st = stats[name]
    print("form %s: worst |device - sum64| / bound = %.3f, M %% 4 seen %s, levels %s" % (name, st["ratio"], sorted(st["mod4"]), sorted(st["levels"])))
    assert st["mod4"] == {0, 1, 2, 3}, (name, st["mod4"])
    assert st["wrong_tail"], name + ": no case where a wrong tail breaks the bound"


def test_small_batch(oracle, hip, scenes):
    stats = {}
    for (w, h) in [(176, 144), (640, 480)]:
        for lvl in (4, 3, 2, 1):
            form = run_batch(oracle, hip, scenes(w, h), 3, lvl, None, stats, "small")
            assert np.all(form == 0), form                      # fewer than 8 jobs: no strips, no solo
    report(stats, "small")


def test_throughput_strips_at_the_floor(oracle, hip, scenes):
    stats = {}
    for (w, h) in [(320, 240), (752, 480)]:                      # 752: strips straddle rows
        for lvl in (4, 3, 2, 1):
            form = run_batch(oracle, hip, scenes(w, h), 8, lvl, 0, stats, "strips")
            assert np.all(form[:, 0] == 0) and np.all(form[:, 1] >= 1024), form
            if lvl >= 3:
                assert np.all(form[:, 1] == 1024), form            # the 1024-pixel floor
    report(stats, "strips")


def test_coarse_levels_in_one_workgroup(oracle, hip, scenes):
    stats = {}
    for (w, h) in [(320, 240), (640, 480)]:
        for lvl in (4, 3, 2, 1):
            form = run_batch(oracle, hip, scenes(w, h), 8, lvl, 1, stats, "solo")
            fits = (w >> lvl) * (h >> lvl) <= 4800 and lvl > 1
            assert np.all(form[:, 1] > 0), form
            assert np.all(form[:, 0] == (1 if fits else 0)), (w, h, lvl, form)   # 640x480 level 2 (19200 px), any level 1: strips
    # 320x240 level 2 is 80x60: the dense keyframe puts 78 x 58 = 4524 points in the 4544 LDS slots
    assert (320, 240, 2) in stats["solo"]["levels"]
    report(stats, "solo")
    st = stats.pop("strips", None)
    if st:
        print("form strips (levels k_track_solo does not take): worst ratio %.3f" % st["ratio"])


def test_large_frames_clamp_the_strip(oracle, hip, scenes):
    stats = {}
    sc = scenes(1280, 1024)
    form = run_batch(oracle, hip, sc, 19, 1, 1, stats, "strips")
    assert np.all(form[:, 0] == 0) and np.all(form[:, 1] == 8192), form    # the 8192-pixel clamp
    form = run_batch(oracle, hip, sc, 19, 4, 1, stats, "strips")
    assert np.all(form[:, 0] == 0), form                         # level 4 is 80 x 64 = 5120 pixels: not for k_track_solo
    st = stats["strips"]
    print("form strips 1280x1024: worst ratio %.3f, M %% 4 seen %s" % (st["ratio"], sorted(st["mod4"])))


def test_hook_refuses_bad_arguments(hip, scenes):
    sc = scenes(176, 144)
    tr = hip.SE3Tracker(sc.ctx)
    _, rg = sc.keyframe("gt", 0)
    fr = hip.Frame(sc.ctx, 99, sc.frames[1])
    for lvl in (0, 5):
        with pytest.raises(hip.LsdHipError):
            tr.evaluateBatch([rg], [fr], IDENT7[None], lvl)
