"""tests/se3_terms.py against the oracle it stands in for: the per-point terms it rebuilds are the oracle's (weights and the gradient
taps bit for bit, isGood point for point through goodCount), and the oracle's own float32 sums of them (sequential SSE loops over N
points) lie within N * EPS * sum|terms| of the float64 sums.  The GPU tests of the SE3 evaluation (test_gpu_parity.py,
test_track_batch_eval_gpu.py) hold the device to these sums."""
import numpy as np
import pytest

from common import sequence
from se3_terms import EPS, point_terms, sums64

IDENT7 = np.array([1.0, 0, 0, 0, 0, 0, 0], np.float32)


@pytest.mark.parametrize("w,h", [(176, 144), (320, 240)])
def test_terms_rebuild_the_oracles_evaluation(oracle, w, h):
    frames, depth0, K, gt = sequence(w, h, 4)
    kfo = oracle.Frame(0, frames[0], K)
    depth = depth0.copy()
    depth[::2, 1::3] = 0
    kfo.set_depth_gt(depth)
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    tro = oracle.SE3Tracker(w, h, K, mode=oracle.SSE_EXACT_RCP)
    poses = [IDENT7, oracle.se3_inv(gt[3]).astype(np.float32),
             oracle.se3_exp(np.array([0.05, -0.03, 0.02, 0.01, -0.02, 0.03])).astype(np.float32)]
    seen = set()
    for pi, T in enumerate(poses):
        for lvl in (4, 3, 2, 1):
            fo = oracle.Frame(3, frames[3], K)
            a, b = (1.0, 0.0) if pi % 2 == 0 else (1.03, -2.5)
            r = tro.evaluate(ro, fo, T, lvl, a, b)
            tag = "pose %d level %d" % (pi, lvl)
            P = point_terms(tro, fo, lvl, T)
            assert P["M"] == r.warped_size and P["M"] >= 8, tag
            seen.add(P["M"] % 4)
            n4 = (P["M"] // 4) * 4          # (the SSE loop leaves the tail's weights unset)
            assert np.array_equal(P["w"][:n4].view(np.uint32), tro.buffer("weight_p")[:n4].view(np.uint32)), tag
            assert np.array_equal(P["dx"].view(np.uint32), tro.buffer("dx").view(np.uint32)), tag
            assert np.array_equal(P["dy"].view(np.uint32), tro.buffer("dy").view(np.uint32)), tag
            S = sums64(P)
            assert S["good"] == int(r.goodCount) and P["M"] - S["good"] == int(r.badCount), tag
            nc = r.num_constraints
            assert nc == 6 * (P["M"] // 4), tag
            N = S["n4"]
            # the oracle: sequential float32 sums over N points, then one division by nc (by N for the weighted error)
            bound = lambda k: (N + 2) * EPS * S[k + "_abs"] + 1e-30
            A = np.array(r.A, np.float64).reshape(6, 6)
            for k, (i, j) in enumerate([(i, j) for i in range(6) for j in range(i, 6)]):
                assert abs(A[i, j] * nc - S["A"][k]) <= bound("A")[k], (tag, i, j)
            assert np.all(np.abs(np.array(r.b, np.float64) * nc - S["b"]) <= bound("b")), tag
            assert abs(r.lsError * nc - S["err"]) <= bound("err"), tag
            assert abs(r.weightedError * N - S["werr"]) <= bound("werr"), tag
            G = S["good"]
            M = P["M"]
            assert abs(r.retval * G - S["res2"]) <= (M + 2) * EPS * S["res2_abs"], tag
            assert abs(r.meanRes * G - S["signed"]) <= (M + 2) * EPS * S["signed_abs"] + 1e-30, tag
            # the wrong tails are different sums wherever the tail is not empty
            if M % 4:
                assert not np.allclose(sums64(P, "none")["A"], S["A"], rtol=0, atol=0), tag
    assert len(seen) >= 2, seen
