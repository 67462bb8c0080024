"""Per-point terms of one Sim3 evaluation (calcSim3Buffers + calcSim3WeightsAndResidualSSE + calcSim3LGSSSE), shared by
tests/test_sim3_terms_cpu.py and tests/test_sim3_eval_gpu.py.

sse_terms() forms, from the oracle's float32 buffers, the float32 products the SSE loops add up (same operation order, exact
reciprocals), for the first (M // 4) * 4 points; sums64() adds them up in float64, beside the sums of their magnitudes.  The bounds
that use them are `n * EPS * sum|terms|`, n a count of roundings on the path of one term into the total."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)     # 2^-23
f32 = np.float32
REMAP = (2, 3, 4, 6)                      # LGS7::initializeFrom: the 4x4 depth system on rows / columns 2, 3, 4, 6


def scene_pair(oracle, w, h, k, scale, holes=False):
    """keyframe = synthetic frame 0 with its depth, tracked frame = frame k with its depth divided by `scale`; Sim3 frame -> keyframe"""
    from lsd_slam_amd import synth
    sc = synth.Scene(0)
    K = synth.intrinsics(w, h)
    imgA, depthA = sc.render(0, w, h)
    imgB, depthB = sc.render(k, w, h)
    depthB = (depthB / scale).astype(np.float32)
    if holes:
        rng = np.random.default_rng(5)
        depthA = depthA.copy(); depthB = depthB.copy()
        depthA[rng.uniform(size=depthA.shape) < 0.5] = 0
        depthB[rng.uniform(size=depthB.shape) < 0.5] = 0
    R, t = sc.frame_to_ref(k, 0)
    exp = np.concatenate([synth.rot_to_quat(R), t, [scale]])
    return dict(K=K, imgA=imgA, imgB=imgB, depthA=depthA, depthB=depthB, exp=exp)


def sim3_mul(a, b):
    """(qw,qx,qy,qz,tx,ty,tz,s) product a * b in float64 (Sophus: t = t_a + s_a R_a t_b, q = q_a q_b, s = s_a s_b)"""
    from oracle.pyoracle import quat_to_rot
    qa, qb = np.asarray(a[:4], float), np.asarray(b[:4], float)
    q = np.array([qa[0] * qb[0] - qa[1] * qb[1] - qa[2] * qb[2] - qa[3] * qb[3],
                  qa[0] * qb[1] + qa[1] * qb[0] + qa[2] * qb[3] - qa[3] * qb[2],
                  qa[0] * qb[2] - qa[1] * qb[3] + qa[2] * qb[0] + qa[3] * qb[1],
                  qa[0] * qb[3] + qa[1] * qb[2] - qa[2] * qb[1] + qa[3] * qb[0]])
    t = np.asarray(a[4:7], float) + a[7] * quat_to_rot(qa) @ np.asarray(b[4:7], float)
    return np.concatenate([q / np.linalg.norm(q), t, [a[7] * b[7]]])


def roll_matrix64(R):
    """The ESM roll of the reference gradients (Sim3Tracker.cpp:455-464) from its definition: the shortest rotation taking R (0,0,-1)
    to (0,0,-1) (axis a x b, angle acos(a . b), Rodrigues), times R — not the quaternion recipe the oracle and the device share."""
    a = R @ np.array([0.0, 0.0, -1.0])
    a = a / np.linalg.norm(a)
    b = np.array([0.0, 0.0, -1.0])
    k = np.cross(a, b)
    s, c = np.linalg.norm(k), float(a @ b)
    if s == 0.0:
        return R.copy()
    k = k / s
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + s * Kx + (1 - c) * Kx @ Kx) @ R


def sse_terms(tr):
    """float32 per-point products of calcSim3LGSSSE / calcSim3WeightsAndResidualSSE from the buffers of oracle Sim3Tracker `tr`'s last
    evaluation, first (M // 4) * 4 points.  -> dict of (n,) float32 arrays: A7[(i, j)] (i <= j, the 6x6 and 4x4 parts separately as
    ('p', i, j) / ('d', i, j) in 7x7 indices), b7 parts ('p', i) / ('d', i) (the -sign of LGS b left out), resP, resD; and J6, J4"""
    B = {k: tr.buffer(k) for k in tr.BUFFERS}
    n = (len(B["x"]) // 4) * 4
    px, py, pzb = B["x"][:n], B["y"][:n], B["z"][:n]
    gx, gy = B["dx"][:n], B["dy"][:n]
    rp, rd, wp, wd = B["residual_p"][:n], B["residual_d"][:n], B["weight_p"][:n], B["weight_d"][:n]
    pz = f32(1.0) / pzb
    J4 = [None, None, None, pz]
    J6 = [pz * gx, pz * gy, None, None, None, None]
    J6[5] = ((px * gy) * pz) - ((py * gx) * pz)
    pz2 = pz * pz
    J4[0] = pz2
    J4[1] = pz2 * py
    J4[2] = f32(0) - (pz2 * px)
    v1 = (px * gx) * pz2
    v2 = (py * gy) * pz2
    J6[2] = f32(0) - (v1 + v2)
    J6[3] = f32(0) - ((v2 * py) + (gy + v1 * py))
    J6[4] = (gx + v1 * px) + v2 * px
    T = {}
    for i in range(6):
        Jw = J6[i] * wp
        for j in range(i, 6):
            T[("p", i, j)] = Jw * J6[j]
    resw = rp * wp
    for i in range(6):
        T[("p", i)] = resw * J6[i]
    T["resP"] = resw * rp
    for i in range(4):
        Jw = J4[i] * wd
        for j in range(i, 4):
            T[("d", REMAP[i], REMAP[j])] = Jw * J4[j]
    resw4 = rd * wd
    for i in range(4):
        T[("d", REMAP[i])] = resw4 * J4[i]
    T["resD"] = resw4 * rd
    T["J6"], T["J4"], T["n"], T["bufs"] = J6, J4, n, B
    return T


def sums64(T):
    """float64 sums of the terms -> (A 7x7, |A| 7x7, b 7, |b| 7, sumResP, |.|, sumResD, |.|) with the LGS7 sign of b (b -= J r w)"""
    A, Aa, b, ba = np.zeros((7, 7)), np.zeros((7, 7)), np.zeros(7), np.zeros(7)
    for key, v in T.items():
        if not isinstance(key, tuple):
            continue
        v = v.astype(np.float64)
        if len(key) == 3:
            _, i, j = key
            s, sa = v.sum(), np.abs(v).sum()
            A[i, j] += s; Aa[i, j] += sa
            if i != j:
                A[j, i] += s; Aa[j, i] += sa
        else:
            b[key[1]] -= v.sum(); ba[key[1]] += np.abs(v).sum()
    rP, rD = T["resP"].astype(np.float64), T["resD"].astype(np.float64)
    return A, Aa, b, ba, rP.sum(), np.abs(rP).sum(), rD.sum(), np.abs(rD).sum()
