"""The oracle's per-point Sim3 terms (oracle/orc_sim3.cpp: calcSim3Buffers, calcSim3WeightsAndResidualSSE with exact reciprocals,
calcSim3LGSSSE) against float64 formulas written from their definitions, point by point.

The oracle is pinned bit for bit to the reference's own Sim3Tracker.cpp (test_ref_pin_cpu.py), but both compile against the same
stand-in algebra: rxso3().matrix() and Quaternionf::setFromTwoVectors(...).toRotationMatrix() are restated identically there and on the
device.  Here that algebra is computed independently in float64 — the roll as the shortest rotation taking R (0,0,-1) to (0,0,-1), by
Rodrigues' formula, times R — and so are the warp, the ESM gradients, the residuals, w_p, w_d and the Huber weight, J6 and J4.

Branch decisions are taken from the float32 values (in-image test, |rp| < 2, Huber, var > 0, the rounding of idx_rounded): a float32
replica of the warp, bit-equal to the oracle's buffers, decides them.  Every bound is n * EPS * M: n a count of the roundings on the
longest path of the float32 computation, M the same expression evaluated on the magnitudes of its operands (the sum of the magnitudes
of what cancels), relative where the path goes through a reciprocal or a square root.  The counts:

  warp       Wx = ((sR00 px + sR01 py) + sR02 pz) + tx: cast of sR (1), product (1), two additions, the translation (1)       n = 5
  ESM grad   fx * 0.5 * (interp + roll . g): bilinear weights (dxdy 1, w00 3), product, three additions (8), the sum and fx (2);
             roll entries: cast of R, norm and division (3), half-angle quaternion (3), toRotationMatrix (3), the product with R
             (3) — 12 absolute on entries of size <= 1 — then product, sum, fx (3)                                             10 / 15
  residual   (a I + b) - interp_z: the affine product and sum (2), interp (8), the difference (1)                              n = 11
  depth      1 / Wz - idepth: reciprocal (1), difference (1)                                                                    n = 2
  weights    g0 = (pz tx - px tz) / (pz^2 d): 6; drpdd = g0 gx + g1 gy: 8; D_p = s2 + drpdd^2 s: 2 * 8 + 4; w_p = 1 / D_p: + 1,
             relative to kappa = D_p(|.|) / D_p; w_d the same with g2 = (pz - tz) / (pz^2 d): 5 -> 15; sqrt halves, the weighted
             residuals add 2, their sum 1, the Huber reciprocal and product 2, weight = wh * w: 1
  J6 / J4    1 / pz (1), z^2 (3), the products and sums of calcSim3LGSSSE: at most 8 (J6[3], J6[4])
  A, b       the oracle's own float32 sums against float64 sums of the same float32 terms: the SSE loops add M / 4 terms per lane in
             sequence, then the four lanes (3) and LGS7::initializeFrom (1)
"""
import numpy as np
import pytest

from sim3_terms import EPS, f32, roll_matrix64, scene_pair, sim3_mul, sse_terms, sums64

ROLL_POSE = np.array([np.cos(0.15), 0.03 * np.sin(0.15), -0.02 * np.sin(0.15), np.sin(0.15), 0, 0, 0, 1.0])   # ~0.3 rad about z, tilted


def _q_normalized(q):
    q = np.asarray(q, float)
    return q / np.linalg.norm(q)


def poses(oracle, exp):
    """name -> referenceToFrame: near the optimum; a 0.3 rad roll about the optical axis with a tilt; far enough off for Huber"""
    T0 = oracle.sim3_inv(exp)
    near = T0.copy(); near[4:7] += [0.004, -0.003, 0.002]; near[7] *= 1.03
    roll = np.concatenate([_q_normalized(ROLL_POSE[:4]), ROLL_POSE[4:]])
    huber = T0.copy(); huber[4:7] += [0.03, -0.025, 0.02]; huber[7] *= 0.97
    return {"near": near, "roll": sim3_mul(roll, near), "huber": huber}


def check(name, got, want, bound, worst):
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    ratio = err / np.maximum(bound, 1e-300)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d points outside the bound, first %d: got %r want %r bound %r" % (
        name, bad.sum(), np.argmax(bad), got[bad][:3], want[bad][:3], bound[bad][:3])
    worst[name] = max(worst.get(name, 0.0), float(ratio.max()) if len(ratio) else 0.0)


def _huber(B32, dr32, s32, g232, sigma2, wabs):
    """the Huber branch as calcSim3WeightsAndResidualSSE takes it (float32), and the float64 weight on that branch"""
    wp32 = f32(1) / (f32(sigma2) + dr32 * (dr32 * s32))
    wd32 = f32(1) / (B32["warped_idepthVar"] + g232 * (g232 * s32))
    wab32 = np.where(B32["warped_idepthVar"] > 0, np.abs(B32["residual_d"] * np.sqrt(wd32)), f32(0)) + np.abs(B32["residual_p"] * np.sqrt(wp32))
    hub = ~(wab32 < f32(3.0))                # settings.huber_d
    wh = np.where(hub, 3.0 / wabs, 1.0)
    return wp32, wab32, hub, wh


def check_evaluation(oracle, P, w, h, T, level, a, b, worst):
    from oracle.pyoracle import quat_to_rot
    fa, fb = oracle.Frame(0, P["imgA"], P["K"]), oracle.Frame(1, P["imgB"], P["K"])
    fa.set_depth_gt(P["depthA"]); fb.set_depth_gt(P["depthB"])
    ra = oracle.TrackingReference(); ra.import_frame(fa)
    tr = oracle.Sim3Tracker(w, h, P["K"], mode=oracle.SSE_EXACT_RCP)
    rec = tr.evaluate(ra, fb, T, level, a, b)
    pos, colvar, gref, _ = ra.pointcloud(level)
    wl, hl = fb.dims(level)
    fx, fy, cx, cy = [f32(v) for v in fb.intrinsics(level)[:4]]
    grad = fb.plane("gradients", level)
    idepth, ivar = fb.plane("idepth", level).ravel(), fb.plane("idepthVar", level).ravel()
    R = quat_to_rot(T[:4])
    sR, t = T[7] * R, np.asarray(T[4:7], float)
    # ---- the warp: float32 replica (decisions), float64 formula (values)
    R32, t32 = sR.astype(np.float32), t.astype(np.float32)
    W32 = []
    for i in range(3):
        acc = R32[i, 0] * pos[:, 0]
        acc = acc + R32[i, 1] * pos[:, 1]
        acc = acc + R32[i, 2] * pos[:, 2]
        W32.append(acc + t32[i])
    u32 = (W32[0] / W32[2]) * fx + cx
    v32 = (W32[1] / W32[2]) * fy + cy
    inside = (u32 > 1) & (v32 > 1) & (u32 < f32(wl - 2)) & (v32 < f32(hl - 2))
    M = int(inside.sum())
    assert rec.warped_size == M
    if M < 8:
        return M
    B = {k: tr.buffer(k) for k in tr.BUFFERS}
    for i, k in enumerate("xyz"):
        assert np.array_equal(B[k].view(np.uint32), W32[i][inside].view(np.uint32)), "float32 replica of the warp (%s)" % k
    p, cv, g = pos[inside].astype(np.float64), colvar[inside].astype(np.float64), gref[inside].astype(np.float64)
    W64 = p @ sR.T + t
    Wmag = np.abs(p) @ np.abs(sR).T + np.abs(t)
    for i, k in enumerate("xyz"):
        check("warp", B[k], W64[:, i], 5 * EPS * Wmag[:, i], worst)
    # ---- interpolation at the float32 (u, v), ESM gradients with the float64 roll
    u, v = u32[inside].astype(np.float64), v32[inside].astype(np.float64)
    ix, iy = u.astype(np.int64), v.astype(np.int64)
    dx, dy = u - ix, v - iy
    wts = [(1 - dx) * (1 - dy), dx * (1 - dy), (1 - dx) * dy, dx * dy]
    taps = [grad[iy, ix], grad[iy, ix + 1], grad[iy + 1, ix], grad[iy + 1, ix + 1]]
    interp = sum(wk[:, None] * tk.astype(np.float64) for wk, tk in zip(wts, taps))
    imag = sum(np.abs(wk)[:, None] * np.abs(tk.astype(np.float64)) for wk, tk in zip(wts, taps))
    Q = roll_matrix64(R)
    for c, (k, f) in enumerate((("dx", fx), ("dy", fy))):
        rot = Q[c, 0] * g[:, 0] + Q[c, 1] * g[:, 1]
        want = float(f) * 0.5 * (interp[:, c] + rot)
        bound = abs(float(f)) * 0.5 * (10 * EPS * imag[:, c] + 15 * EPS * (np.abs(g[:, 0]) + np.abs(g[:, 1])))
        check("esm " + k, B[k], want, bound, worst)
    c1 = float(f32(a)) * cv[:, 0] + float(f32(b))
    check("residual_p", B["residual_p"], c1 - interp[:, 2],
          11 * EPS * (abs(a) * np.abs(cv[:, 0]) + abs(b) + imag[:, 2]), worst)
    # ---- depth: idx_rounded from the float32 (u, v), the branch on the float32 variance
    uu, vv = u32[inside], v32[inside]
    idx = (uu + f32(0.5)).astype(np.int64) + wl * (vv + f32(0.5)).astype(np.int64)
    var_f = ivar[idx]
    valid = var_f > 0
    assert np.array_equal(B["warped_idepthVar"][valid], var_f[valid]) and np.all(B["warped_idepthVar"][~valid] == -1)
    assert np.all(B["residual_d"][~valid] == -1)
    zb = B["z"].astype(np.float64)
    check("residual_d", B["residual_d"][valid], 1 / zb[valid] - idepth[idx][valid],
          2 * EPS * (1 / np.abs(zb[valid]) + np.abs(idepth[idx][valid])), worst)
    check("d", B["d"], 1 / p[:, 2], EPS * np.abs(1 / p[:, 2]), worst)
    assert np.array_equal(B["idepthVar"], colvar[inside][:, 1])
    # ---- weights, from the oracle's float32 buffers (inputs of calcSim3WeightsAndResidualSSE), the first (M // 4) * 4 points
    n = (M // 4) * 4
    px, py, pz, d = [B[k][:n].astype(np.float64) for k in ("x", "y", "z", "d")]
    gx, gy, rp, rd = [B[k][:n].astype(np.float64) for k in ("dx", "dy", "residual_p", "residual_d")]
    s = 1.0 * B["idepthVar"][:n].astype(np.float64)
    sv = B["warped_idepthVar"][:n].astype(np.float64)
    tx, ty, tz = [float(v) for v in t32]
    pz2d = 1 / (pz * pz * d)
    g0, g1, g2 = (pz * tx - px * tz) * pz2d, (pz * ty - py * tz) * pz2d, (pz - tz) * pz2d
    m0, m1, m2 = (np.abs(pz * tx) + np.abs(px * tz)) * np.abs(pz2d), (np.abs(pz * ty) + np.abs(py * tz)) * np.abs(pz2d), \
        (np.abs(pz) + abs(tz)) * np.abs(pz2d)
    drpdd = g0 * gx + g1 * gy
    mdr = m0 * np.abs(gx) + m1 * np.abs(gy)
    sigma2 = float(tr.params.cameraPixelNoise2)
    Dp, Dpm = sigma2 + s * drpdd * drpdd, sigma2 + s * mdr * mdr
    Dd, Ddm = sv + s * g2 * g2, np.abs(sv) + s * m2 * m2
    w_p, w_d = 1 / Dp, 1 / Dd
    kp, kd = Dpm / Dp, np.where(sv > 0, Ddm / np.abs(Dd), 0)
    rel_wp, rel_wd = (2 * 8 + 4 + 1) * kp, (2 * 5 + 4 + 1) * kd
    valid = sv > 0
    wrp, wrd = np.abs(rp) * np.sqrt(w_p), np.where(valid, np.abs(rd) * np.sqrt(np.where(valid, w_d, 1)), 0)
    rel_wabs = np.maximum(rel_wp / 2 + 2, np.where(valid, rel_wd / 2 + 2, 0)) + 1
    wabs = wrp + wrd
    # the Huber branch as the float32 computation takes it
    B32 = {k: B[k][:n] for k in B}
    pz2d32 = f32(1) / ((B32["z"] * B32["z"]) * B32["d"])
    g032 = (B32["z"] * t32[0] - B32["x"] * t32[2]) * pz2d32
    g132 = (B32["z"] * t32[1] - B32["y"] * t32[2]) * pz2d32
    g232 = (B32["z"] - t32[2]) * pz2d32
    dr32 = g032 * B32["dx"] + g132 * B32["dy"]
    s32 = f32(1.0) * B32["idepthVar"]
    with np.errstate(all="ignore"):        # (square roots of the weights of points without depth: masked out below)
        wp32, wab32, hub, wh = _huber(B32, dr32, s32, g232, sigma2, wabs)
    rel_wh = np.where(hub, rel_wabs + 2, 0)
    worst["huber share"] = max(worst.get("huber share", 0.0), float(hub.mean()))
    check("weight_p", B["weight_p"][:n], wh * w_p, (rel_wh + rel_wp + 1) * EPS * wh * w_p, worst)
    check("weight_d", B["weight_d"][:n][valid], (wh * w_d)[valid], ((rel_wh + rel_wd + 1) * EPS * wh * w_d)[valid], worst)
    assert np.all(B["weight_d"][:n][~valid] == 0)
    # ---- J6 / J4 as the float32 helper forms them, against the float64 formulas
    Tm = sse_terms(tr)
    z = 1 / pz
    J6 = [z * gx, z * gy, -(px * gx + py * gy) * z * z, -(gy + (px * gx * py + py * gy * py) * z * z),
          gx + (px * gx * px + py * gy * px) * z * z, (px * gy - py * gx) * z]
    ax, ay, agx, agy = np.abs(px), np.abs(py), np.abs(gx), np.abs(gy)
    J6m = [z * agx, z * agy, (ax * agx + ay * agy) * z * z, agy + (ax * agx * ay + ay * agy * ay) * z * z,
           agx + (ax * agx * ax + ay * agy * ax) * z * z, (ax * agy + ay * agx) * np.abs(z)]
    for i, nop in enumerate((2, 2, 6, 8, 8, 4)):
        check("J6[%d]" % i, Tm["J6"][i], J6[i], nop * EPS * J6m[i], worst)
    J4 = [z * z, z * z * py, -z * z * px, z]
    for i, nop in enumerate((3, 4, 4, 1)):
        check("J4[%d]" % i, Tm["J4"][i], J4[i], nop * EPS * np.abs(J4[i]), worst)
    # ---- the oracle's float32 system against float64 sums of these float32 terms
    A64, Aa, b64, ba, rP, rPa, rD, rDa = sums64(Tm)
    gam = n // 4 + 3 + 1
    A32, b32 = np.array(rec.A, np.float64).reshape(7, 7), np.array(rec.b, np.float64)
    check("A (oracle sums)", A32.ravel(), A64.ravel(), gam * EPS * Aa.ravel() + 1e-30, worst)
    check("b (oracle sums)", b32, b64, gam * EPS * ba + 1e-30, worst)
    # the residual sums add wh * (|r| sqrt(w))^2, the terms (r w) r: 6 more roundings per term
    check("sumResP (oracle)", [rec.sumResP], rP, (gam + 6) * EPS * rPa + 1e-30, worst)
    check("sumResD (oracle)", [rec.sumResD], rD, (gam + 6) * EPS * rDa + 1e-30, worst)
    assert rec.numTermsD == int((B["warped_idepthVar"][:n] > 0).sum()) and rec.numTermsP == n
    return M


@pytest.mark.parametrize("w,h,holes,pose,aff,scale", [
    (160, 128, True, "near", (1.0, 0.0), 1.1),
    (176, 144, False, "roll", (0.97, 1.5), 0.8),
    (320, 240, False, "roll", (0.97, 1.5), 1.1),
    (320, 240, True, "huber", (1.0, 0.0), 1.25),
])
def test_sim3_terms_against_float64(oracle, w, h, holes, pose, aff, scale):
    P = scene_pair(oracle, w, h, 2, scale, holes)
    T = poses(oracle, P["exp"])[pose]
    worst, seen = {}, []
    for level in range(5):
        seen.append(check_evaluation(oracle, P, w, h, T, level, aff[0], aff[1], worst))
    assert max(seen) > 200
    print("%dx%d %s: points per level %s; worst |err| / bound: %s" % (
        w, h, pose, seen, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    if pose == "huber":
        assert worst["huber share"] > 0.1


def test_roll_pose_moves_the_gradients():
    """the roll pose of these tests is far from identity in the image plane: the in-plane part of Q R turns the gradients by ~0.3 rad"""
    from oracle.pyoracle import quat_to_rot
    R = quat_to_rot(_q_normalized(ROLL_POSE[:4]))
    QR = roll_matrix64(R)
    assert np.allclose(QR[:, 2], [0, 0, 1], atol=1e-12)          # Q R (0,0,-1) = (0,0,-1): the optical axis is fixed
    assert np.allclose(QR @ QR.T, np.eye(3), atol=1e-12)
    ang = np.arctan2(QR[1, 0], QR[0, 0])
    assert 0.25 < abs(ang) < 0.35
