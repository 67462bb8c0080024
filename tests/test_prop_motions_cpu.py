"""DepthMap::propagateDepth under general camera motion (tests/prop_motions.py), on the CPU: the inputs are shown to reach every branch,
the census is held to the oracle, and the oracle is pinned to the reference's own DepthMap.cpp under these motions and start states.

POWER OF THE INPUTS, from the census alone (a float64 classification held to the oracle below).  Over motion x {mask, no mask} x {plain,
planted start state} every census class holds at least 100 pixels in at least one case at 176x144; a target with exactly PROP_SLOT_CAP = 8
sources and one with 9 or 10 exist at one of the two sizes; the photometric test rejects at least 1000 sources where the new keyframe
shows another scene and carries no mask.  These are conditions on the inputs: a class that falls short is met by adjusting a recipe of
prop_motions, never by lowering a floor.

The floors are met by the recipes as they stand (start state: _noisy_hyp with sigma 0.02, seed 33, regularised once; planted(.., 7) on
top).  Census figures at 176x144, for orientation: "forward" with the mask 605 / 579 / 547 / 835 sources leave at the four borders;
"forward-big" planted 651 behind-in-image; "x-" planted with the mask occ-keep-old 535, occ-replace 25; "wide" planted with the mask
occ-replace 854, occ-keep-old 0; "other-scene" without a mask 3368 photo-reject; validity-capped 1525 under "far-back-roll" planted;
"far-back-roll" plain 170 targets over the cap with up to 14 sources (320x240: 636, up to 17); "back-1.5" plain: fullest target 8 sources
at 176x144 and 9 at 320x240, planted 9 - 10 and 11.

CENSUS HELD TO THE ORACLE.  Every target with a candidate ends valid, so the census's target count must equal the oracle's valid count
after propagateDepth; 0.1 % is left for pixels where float64 and float32 fall on different sides of a threshold.

ORACLE PINNED TO THE REFERENCE.  propagateDepth alone and the whole createKeyFrame, bit for bit against oracle/_ref, for every motion, both
mask settings and both start states.  Skipped where oracle/_ref cannot be built, as in test_ref_pin_cpu.py."""
import numpy as np
import pytest

import prop_motions as pm
from test_ref_pin_cpu import assert_hyp_bits

SIZES = [(176, 144), (320, 240)]
CASES = [(name, use_mask, plant) for name in pm.NAMES for use_mask in (True, False) for plant in (False, True)]


def label(name, use_mask, plant):
    return "%s %s %s" % (name, "mask" if use_mask else "nomask", "planted" if plant else "plain")


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.have_ref() and not oracle.build_ref():
        pytest.skip("oracle/_ref not available (needs /root/reference to build)")
    oracle.build_ref()          # rebuild if the stand-in headers changed
    return {"sse": oracle.lib(ref="sse")}


@pytest.fixture(scope="module")
def censuses(oracle):
    """{(w, h): {(motion, mask, planted): census}}"""
    return {(w, h): {c: pm.case_census(oracle, w, h, *c) for c in CASES} for w, h in SIZES}


def test_census_table_every_class_is_reached(censuses):
    for (w, h), cs in censuses.items():
        print("\n%dx%d\n" % (w, h) + pm.census_table([(label(*c), v) for c, v in cs.items()]))
    small = censuses[SIZES[0]]
    best = {k: max(v["counts"][k] for v in small.values()) for k in pm.CLASSES}
    edge = ("targets-eq-cap", "targets-cap+1..2")
    short = {k: v for k, v in best.items() if v < 100 and k not in edge}
    assert not short, "census classes that no case at 176x144 reaches with 100 pixels: %r" % short
    for k in edge:
        assert max(v["counts"][k] for cs in censuses.values() for v in cs.values()) >= 1, k
    assert small[("other-scene", False, False)]["counts"]["photo-reject"] >= 1000
    # what today's two motions could not give: every border, both directions of the occlusion branch and the cap, each on ONE case
    for k in ("out-left", "out-top", "out-right", "out-bottom"):
        assert small[("forward", True, False)]["counts"][k] >= 100, k
    assert small[("x-", True, True)]["counts"]["occ-keep-old"] >= 100 and small[("wide", True, True)]["counts"]["occ-replace"] >= 100
    assert small[("far-back-roll", True, True)]["counts"]["validity-capped"] >= 100
    assert small[("forward-big", True, True)]["counts"]["behind-in-image"] >= 100
    # chains: many sources under a rotation, and the 8 / 9 edge
    assert small[("far-back-roll", True, False)]["counts"]["targets-over-cap"] > 0
    assert censuses[SIZES[1]][("far-back-roll", True, False)]["max_sources"] > pm.PROP_SLOT_CAP + 2
    assert censuses[SIZES[1]][("back-1.5", True, False)]["counts"]["targets-over-cap"] > 0


@pytest.mark.parametrize("w,h", SIZES)
def test_census_target_count_agrees_with_the_oracle(oracle, censuses, w, h):
    worst = 0.0
    for name, use_mask, plant in CASES:
        if not use_mask:
            continue
        kf, dm = pm.oracle_map(oracle, w, h, pm.start_state(w, h, plant))
        dm.stage("propagate", [pm.oracle_frame(oracle, w, h, name, kf)])
        n_o = int((dm.get()["isValid"] > 0).sum())
        n_c = censuses[(w, h)][(name, use_mask, plant)]["counts"]["targets"]
        worst = max(worst, abs(n_o - n_c) / max(n_o, 1))
        assert abs(n_o - n_c) <= 0.001 * n_o, "%s: census %d targets, oracle %d valid" % (label(name, use_mask, plant), n_c, n_o)
        assert n_o >= 1000, (label(name, use_mask, plant), n_o)
    print("%dx%d: largest relative difference census / oracle: %.2e" % (w, h, worst))


@pytest.mark.parametrize("plant", [False, True], ids=["plain", "planted"])
@pytest.mark.parametrize("use_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("name", pm.NAMES)
def test_oracle_pinned_to_reference_under_motion(oracle, ref, name, use_mask, plant):
    w, h = SIZES[0]
    L = ref["sse"]
    hyp = pm.start_state(w, h, plant)
    opr = oracle.default_params(L)
    for whole in (False, True):
        kfo, dmo = pm.oracle_map(oracle, w, h, hyp)
        kfr, dmr = pm.oracle_map(oracle, w, h, hyp, params=opr, L=L)
        fo, fr = pm.oracle_frame(oracle, w, h, name, kfo, mask=use_mask), pm.oracle_frame(oracle, w, h, name, kfr, L=L, mask=use_mask)
        if not whole:
            dmo.stage("propagate", [fo])
            dmr.stage("propagate", [fr])
            assert_hyp_bits(dmo.get(), dmr.get(), "%s: propagateDepth" % name)
            continue
        s_o, s_r = dmo.create_keyframe(fo), dmr.create_keyframe(fr)
        assert s_o == s_r or (np.isnan(s_o) and np.isnan(s_r)), (name, s_o, s_r)
        assert_hyp_bits(dmo.get(), dmr.get(), "%s: createKeyFrame" % name)
        assert np.array_equal(fo.pose(), fr.pose()), name
        assert fo.stats() == fr.stats(), name
        for lvl in range(5):
            assert np.array_equal(fo.plane("idepth", lvl).view(np.uint32), fr.plane("idepth", lvl).view(np.uint32)), (name, lvl)
            assert np.array_equal(fo.plane("idepthVar", lvl).view(np.uint32), fr.plane("idepthVar", lvl).view(np.uint32)), (name, lvl)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("use_mask", [True, False], ids=["mask", "nomask"])
def test_oracle_stays_finite_with_sources_behind_the_camera(oracle, w, h, use_mask):
    """createKeyFrame from the planted state under "forward-big": negative inverse depths enter the map as candidates, pass the
    regulariser and the rescale sums; the map stays finite, holds valid hypotheses and the rescale sum stays positive"""
    hyp = pm.start_state(w, h, True)
    kf, dm = pm.oracle_map(oracle, w, h, hyp)
    dm.stage("propagate", [pm.oracle_frame(oracle, w, h, "forward-big", kf, mask=use_mask)])
    after = dm.get()
    v = after["isValid"] > 0
    neg_prop = int((after["idepth"][v] < 0).sum())
    kf, dm = pm.oracle_map(oracle, w, h, hyp)
    nk = pm.oracle_frame(oracle, w, h, "forward-big", kf, mask=use_mask)
    s = dm.create_keyframe(nk)
    m = dm.get()
    v = m["isValid"] > 0
    neg = int((m["idepth_smoothed"][v] < 0).sum())
    print("%dx%d %s: %d negative targets after propagateDepth, rescale factor %.4f, %d valid, %d negative after createKeyFrame"
          % (w, h, "mask" if use_mask else "nomask", neg_prop, s, int(v.sum()), neg))
    assert neg_prop >= 100
    assert int(v.sum()) >= 1000
    assert np.isfinite(s) and s > 0
    for k in ("idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed"):
        assert np.isfinite(m[k][v]).all(), k
    assert nk.pose()[7] == s
    for lvl in range(5):
        assert np.isfinite(nk.plane("idepth", lvl)).all() and np.isfinite(nk.plane("idepthVar", lvl)).all(), lvl
