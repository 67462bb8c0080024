"""The epipolar search under general camera motion (tests/epl_motions.py), on the CPU: the inputs are shown to reach every branch, the
device's reads are shown to stay inside the image, and the oracle is pinned to the reference's own DepthMap.cpp under these motions.

POWER OF THE INPUTS, from the oracle and the census alone.  Over the union of the motions every census class holds at least 50
pixels; from the oracle's line_stereo on a pixel lattice every motion but the near-zero baseline searches at least 1000 pixels, returns
-1 and -2 on at least 50 each, and its observe pass changes at least 1000 hypotheses; the near-zero baseline searches nothing; -3 reaches
50 on the wide baseline and on the motion whose second image shows another scene.  Status -4 is EXEMPT: it needs eplLength == 0 or a
NaN, which no finite pose here produces.  These are conditions on the inputs: a class that falls short is met by adding or adjusting a
motion, never by lowering a threshold.

READS STAY INSIDE.  For every motion and every pixel the census sends into the walk, the extreme taps of stereo_walk_serial (pFar - 2 inc
behind, the last loop position + 4 inc ahead, + 1 for the bilinear tap) lie in [0, w-1] x [0, h-1] — at both test sizes, with and without
the keyframe-gradient tests (the superset).

ORACLE PINNED TO THE REFERENCE.  observe, fillholes, regularize and a second observe per motion, and line_stereo per lattice pixel,
bit for bit against oracle/_ref, for the default switches and for ros-all0.  Skipped where oracle/_ref cannot be built, as in
test_ref_pin_cpu.py."""
import numpy as np
import pytest

import epl_motions as em
from test_ref_pin_cpu import assert_hyp_bits, params_of

W, H = 320, 240
SWITCHES = [pytest.param({}, id="defaults"), pytest.param({"allowNegativeIdepths": 0, "useSubpixelStereo": 0}, id="ros-all0")]


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.have_ref() and not oracle.build_ref():
        pytest.skip("oracle/_ref not available (needs /root/reference to build)")
    oracle.build_ref()          # rebuild if the stand-in headers changed
    return {"sse": oracle.lib(ref="sse"), "scalar": oracle.lib(ref="scalar")}


def _census(oracle, w, h, name, gradients=True):
    kf, dm, hyp = em.noisy_map(oracle, w, h)
    _, sim3, _ = em.pose_of(oracle, w, h, name)
    if gradients:
        return em.census(kf.K, w, h, hyp, sim3, oracle.default_params(), image=kf.plane("image", 0), max_grad=kf.plane("maxGradients", 0))
    return em.census(kf.K, w, h, hyp, sim3, oracle.default_params())


@pytest.fixture(scope="module")
def censuses(oracle):
    return {name: _census(oracle, W, H, name) for name in em.NAMES}


@pytest.fixture(scope="module")
def lattice_codes(oracle):
    """per motion: ({status code: count}, pixels the observe pass changed), from the oracle alone"""
    out = {}
    pts = em.lattice(W, H, 1)      # every interior pixel: -2 is rare (1 in 500 searches)
    for name in em.NAMES:
        kf, dm, hyp = em.noisy_map(oracle, W, H)
        fo = em.oracle_frame(oracle, W, H, name, kf, mask=False)
        dm.stage("observe", [fo])            # (runs prepareForStereoWith on the frame)
        after = dm.get()
        changed = np.zeros(hyp.shape, bool)
        for k in ("isValid", "blacklisted", "nextStereoFrameMinID", "validity_counter", "idepth", "idepth_var"):
            changed |= after[k] != hyp[k]
        dm.set(kf, hyp)
        lo, prior, hi = em.search_intervals(hyp)
        codes = {}
        for x, y in pts:
            c = em.code_of(dm.line_stereo(fo, x, y, lo[y, x], prior[y, x], hi[y, x]))
            codes[c] = codes.get(c, 0) + 1
        out[name] = (codes, int(changed.sum()))
    return out


def test_census_table_every_class_is_reached(censuses):
    rows = [(n, c["counts"], int(c["searched"].sum())) for n, c in censuses.items()]
    print("\n" + em.census_table(rows))
    total = {k: sum(c["counts"][k] for c in censuses.values()) for k in em.CLASSES}
    short = {k: v for k, v in total.items() if v < 50}
    assert not short, "census classes with fewer than 50 pixels over all motions: %r" % short
    # what the circle's frames could not give: both signs of both increments and both dominances, each on one motion alone
    for k in ("incx+", "incx-", "incy+", "incy-", "x-dominant", "y-dominant"):
        assert max(c["counts"][k] for c in censuses.values()) >= 1000, k
    assert int(censuses[em.TINY]["candidates"].sum()) == 0


def test_oracle_status_codes_per_motion(lattice_codes):
    for name, (codes, changed) in lattice_codes.items():
        print("%-12s codes %s, observe changed %d" % (name, dict(sorted(codes.items())), changed))
    for name, (codes, changed) in lattice_codes.items():
        searched = sum(v for k, v in codes.items() if k != 0)
        if name == em.TINY:
            assert searched == 0 and changed == 0, (name, codes, changed)
            continue
        assert searched >= 1000, (name, codes)
        assert codes.get(-1, 0) >= 50 and codes.get(-2, 0) >= 50, (name, codes)
        assert changed >= 1000, (name, changed)
        assert codes.get(-4, 0) == 0, (name, codes)
    for name in ("wide", "other-scene"):
        assert lattice_codes[name][0].get(-3, 0) >= 50, (name, lattice_codes[name][0])


@pytest.mark.parametrize("w,h", [(320, 240), (176, 144)])
@pytest.mark.parametrize("gradients", [True, False])
def test_walk_reads_stay_inside_the_image(oracle, w, h, gradients):
    worst = None
    for name in em.NAMES:
        c = _census(oracle, w, h, name, gradients)
        xmin, xmax, ymin, ymax = c["reads"]
        if len(xmin) == 0:
            assert name == em.TINY, name
            continue
        m = min(int(xmin.min()), int(ymin.min()), w - 1 - int(xmax.max()), h - 1 - int(ymax.max()))
        worst = m if worst is None else min(worst, m)
        assert xmin.min() >= 0 and ymin.min() >= 0 and xmax.max() <= w - 1 and ymax.max() <= h - 1, \
            "%s: the walk would read outside the image: x %d..%d, y %d..%d" % (name, xmin.min(), xmax.max(), ymin.min(), ymax.max())
        assert 1 <= c["steps"].min() and c["steps"].max() < 1000, (name, c["steps"].min(), c["steps"].max())
    print("%dx%d: smallest distance of a tap from the image border: %d" % (w, h, worst))
    assert worst >= 1       # one pixel to spare: float64 here and float32 there may disagree on a step


@pytest.mark.parametrize("ov", SWITCHES)
@pytest.mark.parametrize("name", em.NAMES)
def test_oracle_pinned_to_reference_under_motion(oracle, ref, name, ov):
    L = ref["sse"]
    op, opr = params_of(oracle, None, ov), params_of(oracle, L, ov)
    kfo, dmo, hyp = em.noisy_map(oracle, W, H, params=op)
    kfr, dmr, _ = em.noisy_map(oracle, W, H, params=opr, L=L, hyp=hyp)
    fo, fr = em.oracle_frame(oracle, W, H, name, kfo), em.oracle_frame(oracle, W, H, name, kfr, L=L)
    for st in ("observe", "fillholes", "regularize", "observe"):
        dmo.stage(st, [fo] if st == "observe" else [])
        dmr.stage(st, [fr] if st == "observe" else [])
        assert np.array_equal(fo.stereo_precomp().view(np.uint32), fr.stereo_precomp().view(np.uint32)), name
        assert_hyp_bits(dmo.get(), dmr.get(), "%s: %s" % (name, st))
    dmo.set(kfo, hyp)
    dmr.set(kfr, hyp)
    lo, prior, hi = em.search_intervals(hyp)
    for x, y in em.lattice(W, H):
        args = (lo[y, x], prior[y, x], hi[y, x])
        a, b = dmo.line_stereo(fo, x, y, *args), dmr.line_stereo(fr, x, y, *args)
        assert a.tobytes() == b.tobytes(), (name, x, y, a, b)
