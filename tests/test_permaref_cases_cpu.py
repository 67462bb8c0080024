"""The explicit-point-list tests' inputs and restatements (tests/permaref_cases.py), checked on the oracle alone:

  * pins: SE3Tracker::evaluatePoints on a keyframe's own level-4 cloud equals `evaluate` of that keyframe at level 4 on every record field,
    bit for bit; the float32 restatement of checkPermaRefOverlap, summed as the reference sums it, equals the oracle's check_overlap bit for
    bit on every cloud and pose; the evaluation's in-image mask and weights restated from the buffers are the oracle's;
  * the crafted points are where they should be: on and next to every border, behind the camera and inside the image, on Wz == 0;
  * the inputs can expose a wrong kernel: in every form's case list M % 4 takes every value and each wrong tail (no drop, the first M % 4
    dropped, the tail taken in the column order of a pixel grid instead of list order) misses the evaluation test's bound by more than the
    bound itself; each border comparison loosened to >= / <= changes an exact count or breaks the overlap bound — or cannot differ on this
    camera at all (border_attainable) —; a usage divided by warped_size instead of n and a warped-point minimum taken from another level
    show;
  * the LM loop's cases: at most a quarter unclear, and the clear ones reach every branch of trackFrameOnPermaref."""
import numpy as np
import pytest

import permaref_cases as pc
from se3_terms import EPS, sums64

f32 = np.float32


@pytest.fixture(scope="module")
def orc(oracle):
    return pc.Oracle(oracle)


def test_evaluate_points_equals_evaluate_on_the_keyframes_own_cloud(oracle, orc):
    for size in [(320, 240), (640, 480)]:
        sc = orc.scene(size)
        tr = sc.tracker()
        for kind in ("gt", "dense"):
            pos, cv, ro = sc.keyframe_cloud(kind, permute=False)
            for k, (name, T) in enumerate(sc.poses().items()):
                a, b = pc.AFFINE[k % 3]
                fo = sc.fo[1 + k % 3]
                r_kf = tr.evaluate(ro, fo, T, pc.LEVEL, a, b)
                bufs_kf = [tr.buffer(n) for n in ("x", "y", "z", "dx", "dy", "residual", "d", "idepthVar", "weight_p")]
                r_pts = tr.evaluate_points(pos, cv, fo, T, pc.LEVEL, a, b)
                for field, _ in r_kf._fields_:
                    x, y = np.array(getattr(r_kf, field)), np.array(getattr(r_pts, field))
                    assert x.tobytes() == y.tobytes(), (size, kind, name, field, x, y)
                for n, x in zip(("x", "y", "z", "dx", "dy", "residual", "d", "idepthVar", "weight_p"), bufs_kf):
                    assert x.tobytes() == tr.buffer(n).tobytes(), (size, kind, name, n)
                assert r_kf.warped_size > 0 or name in ("leaves", "behind")


def test_a_list_longer_than_the_image_fits_the_buffers(oracle, orc):
    sc = orc.scene((320, 240))
    pos, cv = sc.synthetic(257)
    tr = oracle.SE3Tracker(32, 16, sc.K, mode=oracle.SSE_EXACT_RCP)           # buffers of 512 floats
    big = (np.tile(pos, (3, 1)), np.tile(cv, (3, 1)))
    r = tr.evaluate_points(big[0], big[1], sc.fo[1], sc.poses()["identity"], pc.LEVEL)
    r1 = sc.tracker().evaluate_points(pos, cv, sc.fo[1], sc.poses()["identity"], pc.LEVEL)
    assert r.warped_size == 3 * r1.warped_size and r.goodCount == 3 * r1.goodCount


def test_overlap_restatement_equals_check_overlap(oracle, orc):
    worst = 0.0
    for size in pc.SCENES:
        sc = orc.scene(size)
        tr = sc.tracker()
        for cname in pc.CLOUD_NAMES[size]:
            pos = orc.cloud(size, cname)[0]
            for pname, T in sc.poses().items():
                T64 = T.astype(np.float64)
                if pname == "twist":
                    T64[:4] *= 1.0000003                                      # an unnormalised quaternion: the cast re-normalises
                term, m = pc.overlap_terms(pos, T64, sc.intr, sc.w4, sc.h4)
                mine = pc.overlap_usage_f32(term, m, len(pos))
                ref = f32(tr.check_overlap(pos, sc.fo[0], T64))
                assert mine.tobytes() == ref.tobytes(), (size, cname, pname, mine, ref)
                if pname == "approach" and np.all(pos[:, 2] > 0):
                    assert np.all(term[m] == 1), (size, cname)                # every term exactly 1: the sum is the count
                    assert float(ref) * len(pos) == pytest.approx(int(m.sum()), abs=len(pos) * EPS * 2)
                # the oracle's own sequential float32 sum lies within the test's bound of the float64 sum only up to n EPS: it is not the yardstick
                worst = max(worst, abs(float(mine) * len(pos) - float(term.astype(np.float64).sum())) / (pc.overlap_bound(term, len(pos)) + 1e-30))
    print("oracle's float32 overlap sum against the float64 sum: worst %.2f of the device's bound" % worst)


def test_restated_mask_and_weights_are_the_oracles(oracle, orc):
    for form in ("single",):
        for size, job, _ in pc.form_jobs(form):
            r, P, S, n = orc.job(size, job)
            sc = orc.scene(size)
            pos, _ = orc.cloud(size, job[0])
            m = pc.in_image_eval(sc, pos, sc.poses()[job[1]])
            assert int(m.sum()) == r.warped_size, (size, job)
            if P is None:
                continue
            assert P["M"] == r.warped_size and int(P["good"].sum()) == r.goodCount, (size, job)
    # weights bit for bit, the record's sums within their own rounding, on one large and one small list
    for job in [("syn4097", "twist", 1, 1), ("syn65", "behind", 2, 2)]:
        sc = orc.scene((320, 240))
        tr = sc.tracker()
        pos, cv = orc.cloud((320, 240), job[0])
        a, b = pc.AFFINE[job[3]]
        r, P, S = pc.evaluate_case(sc, tr, pos, cv, sc.fo[job[2]], sc.poses()[job[1]], a, b)
        n4 = S["n4"]
        assert tr.buffer("weight_p")[:n4].tobytes() == P["w"][:n4].tobytes()
        assert abs(np.float64(r.weightedError) * n4 - S["werr"]) <= (n4 + 2) * EPS * S["werr_abs"]
        assert abs(np.float64(r.lsError) * r.num_constraints - S["err"]) <= (n4 + 2) * EPS * S["err_abs"]


def test_crafted_points_sit_on_and_beside_every_border(oracle, orc):
    for size in [(320, 240), (640, 480)]:
        sc = orc.scene(size)
        pos, cv, founds = sc.crafted_cloud()
        assert len(np.unique(pos, axis=0)) < len(pos)                          # duplicates
        zero_seen = False
        for pname, T in sc.poses().items():
            found = founds[pname]
            for axis, borders in ((0, (0, 1, sc.w4 - 2, sc.w4 - 1)), (1, (0, 1, sc.h4 - 2, sc.h4 - 1))):
                for b in borders:
                    want = {-1, 1} | ({0} if pc.border_attainable(sc.intr, axis, b) else set())
                    assert found[(axis, b)] == want, (size, pname, axis, b, found[(axis, b)])
            zero_seen = zero_seen or found["Wz==0"]
            q, t = np.asarray(T[:4], f32), np.asarray(T[4:7], f32)
            _, _, Wz, u, v = pc.project(pos, q, t, sc.intr)
            behind_inside = (Wz < 0) & pc.inside(u, v, sc.w4, sc.h4, 1, 2)
            assert behind_inside.sum() >= 6, (size, pname)
            if found["Wz==0"]:
                assert np.any(Wz == 0)
        assert zero_seen


def bound_of(S, k, n, jobs):
    return (pc.depth_for(n, jobs) + 1 + pc.C_TERM[k]) * EPS * S[k + "_abs"] + 1e-30


@pytest.mark.parametrize("form", pc.FORMS + ["bank1", "bankN"])
def test_every_form_sees_every_tail_and_would_catch_a_wrong_one(oracle, orc, form):
    mod4, caught, multipass = set(), {"none": 0, "first": 0, "column order": 0}, 0
    for size, job, jobs in pc.form_jobs(form):
        r, P, S, n = orc.job(size, job)
        if P is None or r.warped_size < 8:
            continue
        M = P["M"]
        mod4.add(M % 4)
        multipass += pc.tiles_for(n, jobs)[1] == 0
        if M % 4 == 0:
            continue
        sc = orc.scene(size)
        pos, _ = orc.cloud(size, job[0])
        m = pc.in_image_eval(sc, pos, sc.poses()[job[1]])
        wrong = {"none": sums64(P, "none"), "first": sums64(P, "first"), "column order": pc.sums_with_keep(P, pc.column_order_tail(sc, pos[m], M))}
        for name, W in wrong.items():
            if any(np.any(np.abs(W[k] - S[k]) > 2 * bound_of(S, k, n, jobs)) for k in ("A", "b", "err", "werr")):
                caught[name] += 1
    print("%s: M %% 4 seen %s, cases on which a wrong tail misses the bound: %s, multi-pass jobs %d" % (form, sorted(mod4), caught, multipass))
    assert mod4 == {0, 1, 2, 3}, (form, mod4)
    assert caught["none"] and caught["first"], (form, caught)
    if form not in ("bank1", "bankN"):          # (a keyframe's own order IS the column order of its grid: only permuted lists tell the two apart)
        assert caught["column order"], (form, caught)
    if form in ("batch16", "batch24"):
        assert multipass >= 2, form


def test_tiling_of_the_sizes():
    assert pc.tiles_for(4097) == (24, 1) and pc.tiles_for(4836) == (24, 1) and pc.tiles_for(25000) == (104, 1)
    assert pc.tiles_for(4097, 16) == (16, 0) and pc.tiles_for(4836, 24) == (16, 0) and pc.tiles_for(4096, 16) == (16, 1)
    assert pc.tiles_for(4836, 5) == (24, 1) and pc.tiles_for(25000, 2) == (104, 1) and pc.tiles_for(25000, 5) == (56, 0)
    assert pc.tiles_for(4836, cap=8) == (8, 0) and pc.tiles_for(2048, cap=8) == (8, 1) and pc.tiles_for(2049, cap=8) == (8, 0)
    assert [pc.tiles_for(n)[0] for n in (1, 256, 257, 1064)] == [1, 1, 2, 5]
    # a single job under the three speculation policies: the table tests/cpp/track_plan_test.cpp holds lsd_single_plan to
    table = {255: ((1, 1), (1, 1), (1, 1)), 2048: ((8, 1), (8, 1), (8, 1)), 2049: ((9, 1), (9, 1), (8, 0)), 4097: ((24, 1), (24, 1), (8, 0)),
             4836: ((24, 1), (24, 1), (8, 0)), 24576: ((96, 1), (96, 1), (8, 0)), 25000: ((80, 0), (104, 1), (8, 0))}
    for n, want in table.items():
        assert tuple(pc.single_tiles(n, p) for p in (None, (1, 0), (6, 8))) == want, n


def test_a_loosened_border_comparison_shows(oracle, orc):
    """per comparison: the exact in-image count of the evaluation (warped_size) changes on some case, and the overlap's usage moves by more
    than its bound — unless the border cannot be hit on this camera"""
    seen_eval, seen_overlap = [0] * 4, [0] * 4
    attainable_eval, attainable_overlap = [False] * 4, [False] * 4
    for size in [(320, 240), (640, 480)]:
        sc = orc.scene(size)
        for i, (axis, b) in enumerate(((0, 1), (1, 1), (0, sc.w4 - 2), (1, sc.h4 - 2))):
            attainable_eval[i] |= pc.border_attainable(sc.intr, axis, b)
        for i, (axis, b) in enumerate(((0, 0), (1, 0), (0, sc.w4 - 1), (1, sc.h4 - 1))):
            attainable_overlap[i] |= pc.border_attainable(sc.intr, axis, b)
        pos = sc.crafted_cloud()[0]
        for pname, T in sc.poses().items():
            m = pc.in_image_eval(sc, pos, T)
            term, mo = pc.overlap_terms(pos, T.astype(np.float64), sc.intr, sc.w4, sc.h4)
            s64 = term.astype(np.float64).sum()
            for i in range(4):
                seen_eval[i] += int(pc.in_image_eval(sc, pos, T, loose=i).sum()) != int(m.sum())
                t2, _ = pc.overlap_terms(pos, T.astype(np.float64), sc.intr, sc.w4, sc.h4, loose=i)
                seen_overlap[i] += abs(t2.astype(np.float64).sum() - s64) > 2 * pc.overlap_bound(term, len(pos))
    print("loosened comparisons seen (evaluation %s, overlap %s); attainable (%s, %s)" % (seen_eval, seen_overlap, attainable_eval, attainable_overlap))
    for i in range(4):
        assert bool(seen_eval[i]) == attainable_eval[i], (pc.BORDERS_EVAL[i], seen_eval, attainable_eval)
        assert bool(seen_overlap[i]) == attainable_overlap[i], (pc.BORDERS_OVERLAP[i], seen_overlap, attainable_overlap)
    assert sum(attainable_eval) >= 3 and sum(attainable_overlap) >= 3


def test_a_usage_over_the_warped_count_shows(oracle, orc):
    n_seen = 0
    for size, job, _ in pc.form_jobs("single"):
        r, P, S, n = orc.job(size, job)
        if r.warped_size >= 8 and r.pointUsage != 0:
            wrong = r.pointUsage * n / r.warped_size
            n_seen += abs(wrong - r.pointUsage) > 10 * max(2e-5, 2 * r.warped_size * EPS) * abs(r.pointUsage)
    assert n_seen > 50, n_seen


@pytest.fixture(scope="module")
def loops(oracle, orc):
    return pc.loop_results(orc)


def test_loop_cases_are_clear_and_reach_every_branch(oracle, orc, loops):
    o = oracle
    sc = orc.scene((320, 240))
    unclear, largest = [], 0.0
    reached = dict.fromkeys(["reject chain ends on stepSizeMin", "stop on convergenceEps", "maxIts runs out", "diverged at the first evaluation",
                             "bad through good / all", "bad through good / (good + bad)", "another level's minimum would decide otherwise",
                             "multi-pass under set_speculation(6, 8)", "retries", "accepted after a reject"], 0)
    for case, clear, m, least, (ra, rb), (ta, tb) in loops:
        print("%-36s %s m = %.2e (least margin %.2e): %d evaluations, %d warp updates, diverged %d, good %d" % (
            case[0], "clear  " if clear else "UNCLEAR", m, least, ra.numEvaluations, ra.numWarpUpdates, ra.diverged, ra.trackingWasGood))
        if not clear:
            unclear.append(case[0])
            continue
        largest = max(largest, m)
        br = list(ta["branch"])
        st = case[4]
        reached["reject chain ends on stepSizeMin"] += len(br) >= 2 and br[-1] == o.REJECTED_STEP_MIN and br[-2] == o.REJECTED
        reached["stop on convergenceEps"] += o.ACCEPTED_CONVERGED in br
        reached["maxIts runs out"] += len(br) > 0 and br[-1] == o.ACCEPTED and br.count(o.ACCEPTED) == st["maxIts"]
        reached["diverged at the first evaluation"] += bool(ra.diverged) and ra.numEvaluations == 1
        reached["retries"] += o.REJECTED in br
        reached["accepted after a reject"] += any(x == o.REJECTED and y in (o.ACCEPTED, o.ACCEPTED_CONVERGED) for x, y in zip(br, br[1:]))
        reached["multi-pass under set_speculation(6, 8)"] += len(case[1][0]) > 2048 and len(br) > 0
        if not ra.diverged:
            g, b = float(ra.lastGoodCount), float(ra.lastBadCount)
            all_ok = g / (sc.w4 * sc.h4) > pc.MIN_GOODPERALL_PIXEL
            gb_ok = g / (g + b) > pc.MIN_GOODPERGOODBAD_PIXEL
            assert bool(ra.trackingWasGood) == (all_ok and gb_ok)
            reached["bad through good / all"] += (not all_ok) and gb_ok
            reached["bad through good / (good + bad)"] += all_ok and not gb_ok
            # the warped count of every evaluation against the minimum of level 3 (0.01 x 40 x 30) and of level 5 (0.01 x 10 x 7)
            counts = [int(x) for x in ta["buf_warped_size"]]
            lo, own, hi = [pc.MIN_GOODPERALL_PIXEL_ABSMIN * (sc.w >> l) * (sc.h >> l) for l in (5, 4, 3)]
            reached["another level's minimum would decide otherwise"] += any(own <= c < hi for c in counts)
    print("largest m over the clear cases: %.2e; unclear: %s" % (largest, unclear))
    assert len(unclear) * 4 <= len(loops), unclear
    print("reached by clear cases: %s" % reached)
    for k, v in reached.items():
        assert v, "no clear case reaches: " + k
