"""The explicit-point-list arm of k_track_step and the overlap kernels, entry by entry against the oracle: trackFrameOnPermaref's
evaluation through lsdhip_tracker_evaluate_points / _points_batch / _points_bank (one evalOnly job per list in the launches the
trackFrameOnPermaref entries run), checkPermaRefOverlap through lsdhip_tracker_check_overlap / _check_overlap_bank.  Inputs and
restatements: tests/permaref_cases.py (pinned to the oracle, and shown able to expose a wrong kernel, by tests/test_permaref_cases_cpu.py).

Evaluation.  Every job of every form (permaref_cases.form_batches: the single job; batches of 2, 3, 5, 16 and 24 lists; bank slots at
n = 1 and n > 1) must give

  * exactly the oracle's warped_size, goodCount, badCount and num_constraints;
  * every entry of A and b, lsError, weightedError and retval within |device - sum64| <= gamma EPS sum|terms| + 1e-30, sum64 over the
    first (M // 4) * 4 in-image points IN LIST ORDER (se3_terms.sums64 on the oracle's buffers after evaluate_points);
  * pointUsage and meanRes at the tolerances of tests/test_track_batch_eval_gpu.py; the affine estimate at that file's tolerances (rel
    5e-4, abs 0.08) on every job with 8 or more points in the image, against the same formulas in float64 (check_job says why not
    against the oracle's float32 pair);
  * the same record bits on a second call; the bank's records the bits of the host-cloud call on the downloaded clouds.

gamma = depth + the record's division (1) + the per-term roundings C_TERM of tests/test_track_batch_eval_gpu.py.  The depth of a list of n
points, from the code (permaref_cases.depth_for):
  tiles: fill_level tiles a list by its point count (lsd_level_tiling): nb = ceil(n / 256), rounded up to a multiple of 8 from 16 on,
    capped at grid_cap = 304 for the single job and at max(16, (304 / jobs) & ~7) per job of a batch (lsd_batch_shape): 152, 96, 56 for 2,
    3, 5 jobs, 16 for 16 and 24.  The hooks report nb; the test asserts its restatement (permaref_cases.tiles_for) equals it.
  a lane of tile b walks points b 256 + tid, + 256 nb, ... (eval_plain): P = ceil(n / (256 nb)) sequential additions — 1 while the list
    fits one pass (tiles above ceil(n / 256) are empty: 4097 points in 24 tiles), 2 for 4836 points in 16 tiles, 7 for 25000 in 16;
  the LDS fold of reduce_and_store: a run of RRUN = 43 lanes, then the 6 slices (5);
  the finishing launch: K = ceil(nb / 16) rows per row slot, the 16 slots (15);
  the tail: up to 3 points subtracted again (3) — on multi-pass lists re-evaluated from the list index (the tail key of a point list),
    with the same arithmetic.
  depth = P + 43 + 5 + K + 15 + 3.
The worst |device - sum64| / bound is printed per form (on an MI355X: 0.03 .. 0.05 in every form, the overlap at 0.14 of its bound;
the affine estimate within 2.1e-4 (a, relative) and 0.013 (b) of the float64 formulas).

Overlap.  |usage n - sum64 of the restatement's float32 terms| <= (ceil(n / 256) + 6 + 3 + 2) EPS sum|terms| on every cloud and pose: the
lane-strided run, the wave sum, the four wave totals, the 1-ulp reciprocal of a term plus the final division.  At the
pure-approach pose every term is exactly 1, the sum is the integer count of in-image points and the usage is count / n to the bit.  The
bank launch equals the single call bit for bit, a slot listed twice included."""
import numpy as np
import pytest

import permaref_cases as pc
from common import assert_bit_equal
from se3_terms import EPS

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(scope="module")
def orc(oracle):
    return pc.Oracle(oracle)


class Device:
    """per image size: context, the tracked frames 1..3, a tracker; the keyframes of a bank on demand"""

    def __init__(self, hip, orc):
        self.hip, self.orc, self.worlds = hip, orc, {}

    def world(self, size):
        if size not in self.worlds:
            sc = self.orc.scene(size)
            ctx = self.hip.Context(sc.w, sc.h, sc.K)
            frames = {i: self.hip.Frame(ctx, i, sc.frames[i]) for i in (1, 2, 3)}
            self.worlds[size] = dict(sc=sc, ctx=ctx, frames=frames, tr=self.hip.SE3Tracker(ctx), bank=None)
        return self.worlds[size]

    def bank(self, size):
        """a bank with the "gt" and the "dense" keyframe; their downloaded clouds are the oracle's, bit for bit"""
        wd = self.world(size)
        if wd["bank"] is None:
            sc = wd["sc"]
            bank = self.hip.KeyFrameBank(wd["ctx"], 2)
            slots, kfs = {}, []
            for k, kind in enumerate(("gt", "dense")):
                kf = self.hip.Frame(wd["ctx"], 100 + k, sc.frames[0])
                d, var = sc.keyframe_planes(kind)
                if var is None:
                    kf.setDepthFromGroundTruth(d)
                else:
                    kf.setDepthPlanes(d, var)
                slots[kind] = bank.put(kf)
                kfs.append(kf)
                pos, cv = bank.download(slots[kind])
                opos, ocv = self.orc.cloud(size, "bank:" + kind)
                assert_bit_equal(pos, opos, "%s keyframe cloud" % kind)
                assert_bit_equal(cv, ocv, "%s keyframe colours" % kind)
            wd["bank"], wd["slots"], wd["kfs"] = bank, slots, kfs
        return wd["bank"], wd["slots"]


@pytest.fixture(scope="module")
def dev(hip, orc):
    return Device(hip, orc)


def check_job(tag, g, orc, size, job, jobs, tiles, st):
    """one device record against the oracle's job"""
    r_o, P, S, n = orc.job(size, job)
    assert tuple(tiles) == pc.tiles_for(n, jobs), (tag, tiles, n, jobs)
    assert g.warped_size == r_o.warped_size, (tag, g.warped_size, r_o.warped_size)
    assert g.goodCount == r_o.goodCount and g.badCount == r_o.badCount, (tag, g.goodCount, g.badCount, r_o.goodCount, r_o.badCount)
    assert g.num_constraints == r_o.num_constraints, tag
    M = r_o.warped_size
    st["jobs"] += 1
    st["multipass"] += tiles[1] == 0
    if M < 4:
        return                                   # no group of four: the record's sums are divided by zero on both sides
    st["mod4"].add(M % 4)
    n4, nc, G = S["n4"], r_o.num_constraints, S["good"]
    depth = pc.depth_for(n, jobs) + 1
    dev = {"A": np.array([np.float64(g.A[6 * i + k]) * nc for i in range(6) for k in range(i, 6)]), "b": np.array(g.b, np.float64) * nc,
           "err": np.float64(g.lsError) * nc, "werr": np.float64(g.weightedError) * n4}
    for k in ("A", "b", "err", "werr"):
        bound = (depth + pc.C_TERM[k]) * EPS * S[k + "_abs"] + 1e-30
        ratio = float(np.max(np.abs(dev[k] - S[k]) / bound))
        st["ratio"] = max(st["ratio"], ratio)
        assert ratio <= 1, (tag, k, ratio, dev[k], S[k])
    if G > 0:
        bound = (depth + 1) * EPS * S["res2_abs"] + EPS * abs(S["res2"]) + 1e-30
        ratio = float(abs(np.float64(g.retval) * G - S["res2"]) / bound)
        st["ratio"] = max(st["ratio"], ratio)
        assert ratio <= 1, (tag, "retval", ratio)
        sbound = (depth + 1) * EPS * S["signed_abs"] + EPS * abs(S["signed"]) + 1e-30
        assert abs(np.float64(g.meanRes) * G - S["signed"]) <= sbound, (tag, "meanRes")
    if M < 8:
        return
    st["checked"] += 1
    # (the oracle adds its M usage terms in float32, one after the other: its own error, M EPS relative, is the larger one on long lists)
    assert g.pointUsage == pytest.approx(r_o.pointUsage, rel=max(2e-5, 2 * M * EPS)), tag
    if G > 0:
        assert g.meanRes == pytest.approx(r_o.meanRes, rel=max(1e-3, 2 * M * EPS), abs=1e-4), tag
    # The affine estimate a = sqrt((syy - sy^2 / sw) / (sxx - sx^2 / sw)), b = (sy - a sx) / sw at that file's tolerances (rel 5e-4 for a,
    # 0.08 for b) on every job in which it is defined, against the same formulas in float64 over the oracle's per-point c1, c2 and
    # weights.  (Not against the oracle's own float32 pair: on these low-contrast level-4 images each difference cancels several
    # hundredfold, and the oracle's sequential float32 sums are off from float64 by up to 2.7e-3, more than the tolerance.)
    sc = orc.scene(size)
    pos, cv = orc.cloud(size, job[0])
    m = pc.in_image_eval(sc, pos, sc.poses()[job[1]])
    a, b = pc.AFFINE[job[3]]
    c1 = (f32(a) * cv[m, 0] + f32(b)).astype(np.float64)
    c2 = c1 - P["r"].astype(np.float64)
    wt = np.where(np.abs(P["r"]) < 5, 1.0, 5.0 / np.maximum(np.abs(P["r"].astype(np.float64)), 1e-30))
    sw, sx, sy, sxx, syy = wt.sum(), (c1 * wt).sum(), (c2 * wt).sum(), (c1 * c1 * wt).sum(), (c2 * c2 * wt).sum()
    N, D = syy - sy * sy / sw, sxx - sx * sx / sw
    if N > 0 and D > 0:
        a64 = np.sqrt(N / D)
        b64 = (sy - a64 * sx) / sw
        st["affine"] += 1
        st["affine_a"] = max(st["affine_a"], abs(g.affine_a_lastIt - a64) / a64)
        st["affine_b"] = max(st["affine_b"], abs(g.affine_b_lastIt - b64))
        assert g.affine_a_lastIt == pytest.approx(a64, rel=5e-4), (tag, g.affine_a_lastIt, a64)
        assert g.affine_b_lastIt == pytest.approx(b64, abs=0.08), (tag, g.affine_b_lastIt, b64)


def new_stats():
    return {"ratio": 0.0, "mod4": set(), "jobs": 0, "multipass": 0, "affine": 0, "affine_a": 0.0, "affine_b": 0.0, "checked": 0}


def report(form, st):
    print("form %s: %d jobs (%d multi-pass), worst |device - sum64| / bound = %.3f, M %% 4 seen %s; affine estimate held on %d of the %d jobs "
          "with 8 points or more in the image, worst error %.2e (rel, a) and %.2e (b)" % (
              form, st["jobs"], st["multipass"], st["ratio"], sorted(st["mod4"]), st["affine"], st["checked"], st["affine_a"], st["affine_b"]))
    assert st["mod4"] == {0, 1, 2, 3}, (form, st["mod4"])
    assert st["affine"] == st["checked"] > 0, (form, st["affine"], st["checked"])      # the estimate is defined, and held, on every such job


def job_inputs(wd, orc, size, jobs):
    sc = wd["sc"]
    clouds = [orc.cloud(size, j[0]) for j in jobs]
    frames = [wd["frames"][j[2]] for j in jobs]
    T = np.array([sc.poses()[j[1]] for j in jobs], f32)
    ab = np.array([pc.AFFINE[j[3]] for j in jobs], f32)
    return clouds, frames, T, ab


def test_single_job(orc, dev):
    st = new_stats()
    for size, jobs in pc.form_batches("single"):
        wd = dev.world(size)
        (cloud,), (frame,), T, ab = job_inputs(wd, orc, size, jobs)
        g, tiles = wd["tr"].evaluatePoints(cloud[0], cloud[1], frame, T[0], float(ab[0, 0]), float(ab[0, 1]))
        g2, _ = wd["tr"].evaluatePoints(cloud[0], cloud[1], frame, T[0], float(ab[0, 0]), float(ab[0, 1]))
        tag = "single %dx%d %s" % (size + (jobs[0],))
        assert bytes(g) == bytes(g2), tag + ": two calls differ"
        check_job(tag, g, orc, size, jobs[0], 1, tiles, st)
    report("single", st)


@pytest.mark.parametrize("form", ["batch2", "batch3", "batch5", "batch16", "batch24"])
def test_batches(orc, dev, form):
    st = new_stats()
    for size, jobs in pc.form_batches(form):
        wd = dev.world(size)
        clouds, frames, T, ab = job_inputs(wd, orc, size, jobs)
        recs, tiles = wd["tr"].evaluatePointsBatch(clouds, frames, T, ab)
        recs2, _ = wd["tr"].evaluatePointsBatch(clouds, frames, T, ab)
        for j, job in enumerate(jobs):
            tag = "%s %dx%d job %d %s" % ((form,) + size + (j, job))
            assert bytes(recs[j]) == bytes(recs2[j]), tag + ": two calls differ"
            check_job(tag, recs[j], orc, size, job, len(jobs), tiles[j], st)
    report(form, st)
    if form in ("batch16", "batch24"):
        assert st["multipass"] >= 2, st                                      # 16 tiles per job: the lists above 4096 points


@pytest.mark.parametrize("form", ["bank1", "bankN"])
def test_bank_slots(orc, dev, form):
    st = new_stats()
    for size, jobs in pc.BANK_BATCHES[form]:
        wd = dev.world(size)
        bank, slots = dev.bank(size)
        named = [("bank:" + k, p, fi, ai) for (k, p, fi, ai) in jobs]
        clouds, frames, T, ab = job_inputs(wd, orc, size, named)
        sl = [slots[j[0]] for j in jobs]
        recs, tiles = wd["tr"].evaluatePointsBank(bank, sl, frames, T, ab)
        recs2, _ = wd["tr"].evaluatePointsBank(bank, sl, frames, T, ab)
        if len(jobs) == 1:
            host, htiles = wd["tr"].evaluatePoints(clouds[0][0], clouds[0][1], frames[0], T[0], float(ab[0, 0]), float(ab[0, 1]))
            host, htiles = [host], [htiles]
        else:
            host, htiles = wd["tr"].evaluatePointsBatch(clouds, frames, T, ab)
        for j, job in enumerate(named):
            tag = "%s %dx%d job %d %s" % ((form,) + size + (j, job))
            assert bytes(recs[j]) == bytes(recs2[j]), tag + ": two calls differ"
            assert bytes(recs[j]) == bytes(host[j]), tag + ": the bank's record is not the host-cloud call's"
            assert np.array_equal(tiles[j], htiles[j]), tag
            check_job(tag, recs[j], orc, size, job, len(jobs), tiles[j], st)
    report(form, st)


def test_hooks_refuse_bad_arguments(hip, orc, dev):
    wd = dev.world((320, 240))
    pos, cv = orc.cloud((320, 240), "syn5")
    tr = wd["tr"]
    T = np.array([1, 0, 0, 0, 0, 0, 0], f32)
    with pytest.raises(hip.LsdHipError):
        tr.evaluatePoints(pos[:0], cv[:0], wd["frames"][1], T)
    bank, slots = dev.bank((320, 240))
    with pytest.raises(hip.LsdHipError):
        tr.evaluatePointsBank(bank, [7], [wd["frames"][1]], T[None])


def test_overlap(orc, dev):
    worst, approach_checked = 0.0, 0
    for size in pc.SCENES:
        wd = dev.world(size)
        sc = wd["sc"]
        for cname in pc.CLOUD_NAMES[size]:
            pos = orc.cloud(size, cname)[0]
            n = len(pos)
            for pname, T in sc.poses().items():
                T64 = T.astype(np.float64)
                u = f32(wd["tr"].checkPermaRefOverlap(pos, T64))
                term, m = pc.overlap_terms(pos, T64, sc.intr, sc.w4, sc.h4)
                s64 = float(term.astype(np.float64).sum())
                bound = pc.overlap_bound(term, n)
                tag = "overlap %dx%d %s %s" % (size + (cname, pname))
                if bound > 0:
                    worst = max(worst, abs(float(u) * n - s64) / bound)
                assert abs(float(u) * n - s64) <= bound, (tag, float(u) * n, s64, bound)
                if pname == "approach" and np.all(pos[:, 2] > 0):
                    count = int(m.sum())
                    assert np.all(term[m] == 1)
                    assert u.tobytes() == (f32(count) / f32(n)).tobytes(), (tag, u, count, n)
                    approach_checked += 1
    print("overlap: worst |usage n - sum64| / bound = %.3f; integer counts at the approach pose on %d clouds" % (worst, approach_checked))
    assert approach_checked >= 20


def test_overlap_bank_equals_the_single_call(orc, dev):
    worst = 0.0
    for size in pc.SCENES:
        wd = dev.world(size)
        sc = wd["sc"]
        bank, slots = dev.bank(size)
        names = list(sc.poses())
        pairs = [("gt", names[0]), ("dense", names[1]), ("gt", names[2]), ("dense", names[3]), ("dense", names[4]), ("gt", names[4]), ("dense", names[1])]
        T64 = np.array([sc.poses()[p] for _, p in pairs], np.float64)
        got = wd["tr"].checkPermaRefOverlapBank(bank, [slots[k] for k, _ in pairs], T64)
        assert got[1].tobytes() == got[6].tobytes()                           # the same (slot, pose) listed twice
        for j, (kind, pname) in enumerate(pairs):
            pos = orc.cloud(size, "bank:" + kind)[0]
            single = f32(wd["tr"].checkPermaRefOverlap(pos, T64[j]))
            assert got[j].tobytes() == single.tobytes(), (size, kind, pname, got[j], single)
            term, m = pc.overlap_terms(pos, T64[j], sc.intr, sc.w4, sc.h4)
            bound = pc.overlap_bound(term, len(pos))
            err = abs(float(got[j]) * len(pos) - float(term.astype(np.float64).sum()))
            assert err <= bound, (size, kind, pname, err, bound)
            worst = max(worst, err / bound if bound > 0 else 0.0)
    print("overlap over the bank: worst |usage n - sum64| / bound = %.3f" % worst)
