"""The Levenberg-Marquardt step the trackers run on the device, against float64.

Every LM iteration of the SE3 tracker solves the damped 6x6 system in one wave (gj6_solve_wave), maps the increment through
SE3f::exp (se3f_exp_wave, sincos_small) and left-multiplies the pose (se3f_mul_wave, q_normalize_wave); the Sim3 tracker does the
same with gj7_solve_wave and the double-precision sim3_exp / sim3_mul (track_device.hpp, sim3.hip).  The end-to-end parity tests
cannot see a subtly wrong step — LM corrects itself and only the iteration count moves — so these tests run exactly those inline
routines through the lsdhip_devtest_* hooks (one 64-lane workgroup per case, no image) and hold them to:

  solves   normwise backward error |M x - r| / (|M| |x| + |r|) <= BWD * eps32 (M the damped float32 matrix as the device forms it,
           r = -b), forward error <= FWD * cond(M) * eps32 against numpy.linalg in float64, the same bound against the host LDL^T
           (lsdhip_host_ldlt6 / ldlt7) and the oracle's orc_ldlt6_solve; b = 0 gives x = 0 exactly; an exactly zero row and column
           leaves its unknown at exactly 0 and the rest solves the reduced system (Eigen's LDLT on a zero pivot);
  exp      the pose against oracle.se3_exp / oracle.sim3_exp and the quaternion product in float64, at theta = 0, either side of the
           small-angle branch (1e-5), of the two sincos_small switches (half angle 0.5 <-> theta 1.0, theta 0.5 <-> 1.0), near pi,
           translations 1e-6 ... 10 and random input poses; |q| = 1 within 2 eps32 (rsq).  Sim3 (double on the device): 1e-12.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)     # 2^-23
# Backward error of the unpivoted elimination of an n x n SPD system: each of the n steps rounds the multiplier (1-ulp reciprocal and
# a product) and the update (a product and a difference), and the last division another 1-ulp reciprocal and a product: about 4 n + 2
# roundings of at most eps on a path, no growth on SPD matrices (Higham, Accuracy and Stability, 2nd ed., thm 10.5).  n = 7: 30.
BWD = 32
FWD = 32                                  # forward error <= cond(M) * backward error, same constant


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(scope="module")
def ctx(hip):
    from lsd_slam_amd import synth
    return hip.Context(160, 128, synth.intrinsics(160, 128))


# ---- the hooks ---------------------------------------------------------------------------------------------------------------------
def se3_step(ctx, A, b, damp, T):
    """-> (inc n x 6, Tn n x 7) from the device"""
    A = np.ascontiguousarray(A, np.float32).reshape(-1, 36)
    n = len(A)
    b = np.ascontiguousarray(b, np.float32).reshape(n, 6)
    damp = np.ascontiguousarray(np.broadcast_to(np.asarray(damp, np.float32), (n,)))
    T = np.ascontiguousarray(np.broadcast_to(np.asarray(T, np.float32), (n, 7)))
    inc, Tn = np.zeros((n, 6), np.float32), np.zeros((n, 7), np.float32)
    rc = ctx.L.lsdhip_devtest_se3f_lm_step(ctx.h_, n, A.ctypes.data, b.ctypes.data, damp.ctypes.data, T.ctypes.data,
                                           inc.ctypes.data, Tn.ctypes.data)
    assert rc == 0, ctx.L.lsdhip_last_error()
    return inc, Tn


def sim3_step(ctx, A, b, nc, lam, T):
    """-> (inc n x 7, Tn n x 8) from the device"""
    A = np.ascontiguousarray(A, np.float32).reshape(-1, 49)
    n = len(A)
    b = np.ascontiguousarray(b, np.float32).reshape(n, 7)
    nc = np.ascontiguousarray(np.broadcast_to(np.asarray(nc, np.float64), (n,)))
    lam = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, np.float32), (n,)))
    T = np.ascontiguousarray(np.broadcast_to(np.asarray(T, np.float64), (n, 8)))
    inc, Tn = np.zeros((n, 7), np.float32), np.zeros((n, 8), np.float64)
    rc = ctx.L.lsdhip_devtest_sim3_lm_step(ctx.h_, n, A.ctypes.data, b.ctypes.data, nc.ctypes.data, lam.ctypes.data, T.ctypes.data,
                                           inc.ctypes.data, Tn.ctypes.data)
    assert rc == 0, ctx.L.lsdhip_last_error()
    return inc, Tn


def host_ldlt(L, M32, r32):
    n = len(r32)
    x = np.zeros(n, np.float32)
    M = np.ascontiguousarray(M32, np.float32)
    r = np.ascontiguousarray(r32, np.float32)
    fn = L.lsdhip_host_ldlt6 if n == 6 else L.lsdhip_host_ldlt7
    assert fn(M.ctypes.data, r.ctypes.data, x.ctypes.data) == 0
    return x


# ---- the systems ------------------------------------------------------------------------------------------------------------------
def damped(A32, damp32):
    """the matrix the device factorises: the diagonal times damp, rounded to float32 (gj6: m *= damp)"""
    M = np.array(A32, np.float32, copy=True)
    n = len(M)
    M[np.arange(n), np.arange(n)] = M[np.arange(n), np.arange(n)] * np.float32(damp32)
    return M


def random_systems(n, count, seed, scaled):
    """J^T J of a random 40 x n J (SPD), b random; `scaled`: columns of J scaled by 0.01 ... 100 (what the host tests use)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        J = rng.normal(size=(40, n))
        if scaled:
            J = J * rng.uniform(0.01, 100.0, n)
        A = (J.T @ J).astype(np.float32)
        b = rng.normal(size=n).astype(np.float32)
        out.append((A, b))
    return out


DAMPS = [1.0, 1.0 + 1e-6, 2.0, 1e3]


def check_solution(M32, r32, x, what, others=()):
    """normwise backward error, forward error against float64, and the same forward bound against other solvers' x"""
    M = M32.astype(np.float64)
    r = r32.astype(np.float64)
    x64 = x.astype(np.float64)
    assert np.all(np.isfinite(x)), (what, x)
    nM = np.linalg.norm(M, 2)
    eta = np.linalg.norm(M @ x64 - r) / (nM * np.linalg.norm(x64) + np.linalg.norm(r))
    assert eta <= BWD * EPS, (what, eta / EPS)
    want = np.linalg.solve(M, r)
    cond = np.linalg.cond(M)
    bound = FWD * cond * EPS * np.linalg.norm(want)
    assert np.linalg.norm(x64 - want) <= bound, (what, np.linalg.norm(x64 - want) / np.linalg.norm(want), cond)
    for name, xo in others:
        assert np.linalg.norm(x64 - xo.astype(np.float64)) <= 2 * bound, (what, name, x, xo)
    return eta


def se3_systems_from_evaluations(oracle):
    """LGS6 after finish() from the reference's own evaluation (the oracle's SE3Tracker.evaluate) on a synthetic sequence, levels 4 ... 1,
    at the identity, the true pose and a perturbed one"""
    from lsd_slam_amd import synth
    w, h = 320, 240
    frames, depth0, K, gt = synth.make_sequence(w, h, 4)
    kf = oracle.Frame(0, frames[0], K)
    kf.set_depth_gt(depth0)
    ref = oracle.TrackingReference()
    ref.import_frame(kf)
    tr = oracle.SE3Tracker(w, h, K, mode=oracle.SSE)
    out = []
    for i in (1, 3):
        f = oracle.Frame(i, frames[i], K)
        T_true = oracle.se3_inv(np.asarray(gt[i], np.float64))        # gt: frame -> frame 0; evaluate takes referenceToFrame
        poses = [np.array([1, 0, 0, 0, 0, 0, 0], np.float64), T_true,
                 oracle.se3_mul(oracle.se3_exp([0.004, -0.003, 0.002, 0.003, -0.002, 0.001]), T_true)]
        for lvl in (4, 3, 2, 1):
            for T in poses:
                ev = tr.evaluate(ref, f, T.astype(np.float32), lvl)
                out.append((np.array(ev.A, np.float32).reshape(6, 6), np.array(ev.b, np.float32), "frame %d level %d" % (i, lvl)))
    return out


# ---- solves --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["spd", "scaled-columns"])
def test_gj6_solves_like_float64(ctx, oracle, scaled):
    L, OL = ctx.L, oracle.lib()
    systems = random_systems(6, 12, 11 + scaled, scaled)
    A = np.stack([damped(a, 1.0) for a, _ in systems for _ in DAMPS])          # the undamped matrices, one per (system, damp)
    b = np.stack([bb for _, bb in systems for _ in DAMPS])
    damps = np.array([d for _ in systems for d in DAMPS], np.float32)
    inc, _ = se3_step(ctx, A, b, damps, [1, 0, 0, 0, 0, 0, 0])
    worst = 0.0
    for k in range(len(A)):
        M32, r32 = damped(A[k], damps[k]), (-b[k]).astype(np.float32)
        xo = np.zeros(6, np.float32)
        OL.orc_ldlt6_solve(np.ascontiguousarray(M32).ravel(), r32, xo)
        worst = max(worst, check_solution(M32, r32, inc[k], (k, float(damps[k])),
                                          [("host ldlt6", host_ldlt(L, M32, r32)), ("orc_ldlt6_solve", xo)]))
    print("gj6 %s: worst normwise backward error %.2f eps" % ("scaled" if scaled else "spd", worst / EPS))


def test_gj6_solves_the_reference_normal_equations(ctx, oracle):
    L = ctx.L
    cases = se3_systems_from_evaluations(oracle)
    A = np.stack([a for a, _, _ in cases for _ in DAMPS])
    b = np.stack([bb for _, bb, _ in cases for _ in DAMPS])
    damps = np.array([d for _ in cases for d in DAMPS], np.float32)
    inc, _ = se3_step(ctx, A, b, damps, [1, 0, 0, 0, 0, 0, 0])
    for k in range(len(A)):
        M32, r32 = damped(A[k], damps[k]), (-b[k]).astype(np.float32)
        check_solution(M32, r32, inc[k], (cases[k // len(DAMPS)][2], float(damps[k])), [("host ldlt6", host_ldlt(L, M32, r32))])


def test_gj6_zero_right_hand_side_gives_zero(ctx):
    systems = random_systems(6, 4, 21, True)
    A = np.stack([a for a, _ in systems])
    inc, Tn = se3_step(ctx, A, np.zeros((len(A), 6), np.float32), 1.5, [1, 0, 0, 0, 0, 0, 0])
    assert np.all(inc == 0), inc
    assert np.array_equal(Tn, np.tile(np.array([1, 0, 0, 0, 0, 0, 0], np.float32), (len(A), 1)))


def zero_rows_cases(n, seed):
    """every single index and a few pairs: row and column exactly zero (b there zero, as when the column of J is zero, or not)"""
    sets = [(k,) for k in range(n)] + [(0, 1), (2, 4), (1, n - 1), (3, 5)]
    systems = random_systems(n, len(sets), seed, True)
    out = []
    for (A, b), z in zip(systems, sets):
        A = A.copy()
        b = b.copy()
        A[list(z), :] = 0
        A[:, list(z)] = 0
        b_zero = b.copy()
        b_zero[list(z)] = 0
        out.append((A, b_zero, z))
        out.append((A, b, z))
    return out


def check_zero_rows(M32, r32, x, z, what):
    assert np.all(np.isfinite(x)), (what, z, x)
    assert np.all(x[list(z)] == 0), (what, z, x)
    keep = [i for i in range(len(x)) if i not in z]
    check_solution(M32[np.ix_(keep, keep)], r32[keep], x[keep], (what, z))


@pytest.mark.parametrize("damp", [1.0, 2.0])
def test_gj6_zero_row_and_column_leaves_its_unknown_at_zero(ctx, damp):
    """A degree of freedom without any constraint (gx = 0 everywhere: the tx column of J is zero) gives an exactly zero row and column;
    the reference's A.ldlt().solve(b) returns 0 in that unknown and the reduced system's solution in the others"""
    L = ctx.L
    cases = zero_rows_cases(6, 31)
    A = np.stack([a for a, _, _ in cases])
    b = np.stack([bb for _, bb, _ in cases])
    inc, Tn = se3_step(ctx, A, b, damp, [1, 0, 0, 0, 0, 0, 0])
    for k, (a, bb, z) in enumerate(cases):
        M32, r32 = damped(a, damp), (-bb).astype(np.float32)
        check_zero_rows(M32, r32, inc[k], z, k)
        xh = host_ldlt(L, M32, r32)
        assert np.all(xh[list(z)] == 0)
        keep = [i for i in range(6) if i not in z]
        want = np.linalg.solve(M32[np.ix_(keep, keep)].astype(np.float64), r32[keep].astype(np.float64))
        bound = 2 * FWD * np.linalg.cond(M32[np.ix_(keep, keep)].astype(np.float64)) * EPS * np.linalg.norm(want)
        assert np.linalg.norm(inc[k][keep].astype(np.float64) - xh[keep]) <= bound, (k, z)
        assert np.all(np.isfinite(Tn[k])), (k, Tn[k])


@pytest.mark.parametrize("scaled", [False, True], ids=["spd", "scaled-columns"])
def test_gj7_solves_like_float64(ctx, scaled):
    L = ctx.L
    systems = random_systems(7, 12, 41 + scaled, scaled)
    rng = np.random.default_rng(42)
    A, b, ncs, lams = [], [], [], []
    for a, bb in systems:
        for lam in (0.0, 1e-6, 1.0, 999.0):
            nc = float(rng.integers(1, 5000))
            A.append((a.astype(np.float64) * nc).astype(np.float32))   # the raw sums: the device divides by nc
            b.append((bb.astype(np.float64) * nc).astype(np.float32))
            ncs.append(nc)
            lams.append(lam)
    A, b = np.stack(A), np.stack(b)
    inc, _ = sim3_step(ctx, A, b, ncs, lams, [1, 0, 0, 0, 0, 0, 0, 1])
    for k in range(len(A)):
        M32, r32 = sim3_damped(A[k], b[k], ncs[k], lams[k])
        check_solution(M32, r32, inc[k], (k, ncs[k], lams[k]), [("host ldlt7", host_ldlt(L, M32, r32))])


def sim3_damped(A, b, nc, lam):
    """sim3_damped_entry in float32: A / nc with the diagonal * (1 + lambda), -b / nc"""
    ncf = np.float32(nc)
    M = (np.asarray(A, np.float32).reshape(7, 7) / ncf).astype(np.float32)
    d = np.arange(7)
    M[d, d] = M[d, d] * (np.float32(1) + np.float32(lam))
    r = (-np.asarray(b, np.float32) / ncf).astype(np.float32)
    return M, r


def test_gj7_solves_the_reference_normal_equations(ctx, oracle):
    from lsd_slam_amd import synth
    L = ctx.L
    w, h = 320, 240
    sc = synth.Scene(0)
    K = synth.intrinsics(w, h)
    imgA, depthA = sc.render(0, w, h)
    imgB, depthB = sc.render(2, w, h)
    fa, fb = oracle.Frame(0, imgA, K), oracle.Frame(2, imgB, K)
    fa.set_depth_gt(depthA)
    fb.set_depth_gt((depthB / 1.05).astype(np.float32))
    ra = oracle.TrackingReference()
    ra.import_frame(fa)
    tr = oracle.Sim3Tracker(w, h, K, mode=oracle.SSE_EXACT_RCP)
    R, t = sc.frame_to_ref(2, 0)
    T_true = oracle.sim3_inv(np.concatenate([synth.rot_to_quat(R), t, [1.05]]))
    cases = []
    for lvl in (4, 3, 2, 1):
        for T in (np.array([1, 0, 0, 0, 0, 0, 0, 1.0]), T_true):
            ev = tr.evaluate(ra, fb, T, lvl)
            for lam in (0.0, 1e-6, 1.0, 999.0):
                cases.append((np.array(ev.A, np.float32), np.array(ev.b, np.float32), ev.num_constraints, lam))
    inc, _ = sim3_step(ctx, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), [c[2] for c in cases],
                       [c[3] for c in cases], [1, 0, 0, 0, 0, 0, 0, 1])
    for k, (A, b, nc, lam) in enumerate(cases):
        M32, r32 = sim3_damped(A, b, nc, lam)
        check_solution(M32, r32, inc[k], (k, nc, lam), [("host ldlt7", host_ldlt(L, M32, r32))])


def test_gj7_zero_row_and_column_leaves_its_unknown_at_zero(ctx):
    cases = zero_rows_cases(7, 51)
    A = np.stack([a for a, _, _ in cases])
    b = np.stack([bb for _, bb, _ in cases])
    inc, Tn = sim3_step(ctx, A, b, 1.0, 0.0, [1, 0, 0, 0, 0, 0, 0, 1])
    for k, (a, bb, z) in enumerate(cases):
        M32, r32 = sim3_damped(a, bb, 1.0, 0.0)
        check_zero_rows(M32, r32, inc[k], z, k)
        assert np.all(np.isfinite(Tn[k]))


# ---- exp and product -----------------------------------------------------------------------------------------------------------------
def unit_quats(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def tangents(dim, seed):
    """rotation vectors of the angles where the branches switch, each with translations 1e-6 ... 10"""
    rng = np.random.default_rng(seed)
    thetas = [0.0, 1e-7, 9.9e-6, 1.01e-5, 3e-5, 2e-4, 1e-3, 0.499, 0.501, 0.999, 1.001, 1.998, 2.002, 3.0, np.pi - 1e-3, np.pi - 1e-6]
    out = []
    for th in thetas:
        for tn in (0.0, 1e-6, 1e-3, 0.1, 10.0):
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            v = rng.normal(size=3)
            v *= tn / np.linalg.norm(v)
            a = np.zeros(dim)
            a[:3] = v
            a[3:6] = th * u
            out.append(a)
    return out


def quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2, w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2])


def test_se3f_exp_and_product_against_float64(ctx, oracle):
    """Bounds, derived from the float32 arithmetic of Sophus SE3Group<float>::exp and operator* (pose_math.hpp / se3f_exp_wave):
      q: sin / cos of the half angle (polynomial: truncation < 2e-10, a few roundings; library beyond: ~1 ulp), one division,
         rsq normalisation (1 ulp), the 16-term quaternion product, another normalisation: QB = 16 eps on components of magnitude <= 1;
      |q|: 1 within 2 eps (the 1-ulp rsq and the rounding of each scaled component);
      t: V upsilon + rotate(q, t_T): TB = 16 eps (|upsilon| + |t_T|) of rounding, plus what the float formula itself cannot resolve —
         (1 - cos theta) / theta^2 loses eps / theta^2 to the rounding of cos theta near 1, i.e. eps / theta relative on V upsilon
         (theta >= 1e-5); below 1e-5, V is taken as R(q), off by theta / 2 (Sophus' own approximation)."""
    tans = tangents(6, 61)
    Ts = [np.array([1, 0, 0, 0, 0, 0, 0], np.float64)]
    for q in unit_quats(3, 62):
        Ts.append(np.concatenate([q, np.random.default_rng(63).normal(0, 2.0, 3)]))
    A = np.tile(np.eye(6, dtype=np.float32), (len(tans) * len(Ts), 1, 1))
    b = np.stack([-np.asarray(a, np.float32) for _ in Ts for a in tans])   # (I) inc = -b: the increment itself
    T32 = np.stack([T.astype(np.float32) for T in Ts for _ in tans])
    inc, Tn = se3_step(ctx, A, b, 1.0, T32)
    assert np.array_equal(inc, -b)
    worst_q = 0.0
    for k in range(len(inc)):
        a64 = inc[k].astype(np.float64)
        T64 = T32[k].astype(np.float64)
        want = oracle.se3_mul(oracle.se3_exp(a64), T64)
        got = Tn[k].astype(np.float64)
        theta = np.linalg.norm(a64[3:])
        nu, nt = np.linalg.norm(a64[:3]), np.linalg.norm(T64[4:])
        assert abs(np.linalg.norm(got[:4]) - 1.0) <= 2 * EPS, (k, np.linalg.norm(got[:4]) - 1)
        dq = np.abs(got[:4] - want[:4]).max()
        worst_q = max(worst_q, dq)
        assert dq <= 16 * EPS, (k, theta, dq / EPS, got, want)
        formula = (EPS / theta) if theta >= 1e-5 else theta
        tb = 16 * EPS * (nu + nt) + formula * nu
        assert np.abs(got[4:] - want[4:]).max() <= tb + 1e-30, (k, theta, nu, nt, got, want)
    print("se3f exp * T: worst quaternion error %.1f eps over %d cases" % (worst_q / EPS, len(inc)))


def test_sim3_exp_and_product_against_float64(ctx, oracle):
    """double on the device: 1e-12 of the magnitudes involved"""
    tans = tangents(7, 71)
    rng = np.random.default_rng(72)
    for a in tans:
        a[6] = rng.choice([0.0, 1e-12, 1e-3, -0.2, 0.7])
    Ts = [np.array([1, 0, 0, 0, 0, 0, 0, 1.0])]
    for q in unit_quats(3, 73):
        Ts.append(np.concatenate([q, rng.normal(0, 2.0, 3), [rng.uniform(0.5, 2.0)]]))
    A = np.tile(np.eye(7, dtype=np.float32), (len(tans) * len(Ts), 1, 1))
    b = np.stack([-np.asarray(a, np.float32) for _ in Ts for a in tans])
    T = np.stack([T for T in Ts for _ in tans])
    inc, Tn = sim3_step(ctx, A, b, 1.0, 0.0, T)
    assert np.array_equal(inc, -b)
    for k in range(len(inc)):
        E = oracle.sim3_exp(inc[k].astype(np.float64))
        q = quat_mul(E[:4], T[k][:4])
        q /= np.linalg.norm(q)
        t = E[4:7] + E[7] * (oracle.quat_to_rot(E[:4]) @ T[k][4:7])
        got = Tn[k]
        assert np.abs(got[:4] - q).max() <= 1e-12, (k, got, q)
        mag = np.linalg.norm(E[4:7]) + E[7] * np.linalg.norm(T[k][4:7]) + 1.0
        assert np.abs(got[4:7] - t).max() <= 1e-12 * mag, (k, got, t)
        assert abs(got[7] - E[7] * T[k][7]) <= 1e-12 * abs(E[7] * T[k][7]), k
        assert abs(np.linalg.norm(got[:4]) - 1.0) <= 1e-12
