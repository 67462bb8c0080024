"""float64 sums of the oracle's per-point float32 terms of one SE3 evaluation (SE3Tracker::evaluate in SSE_EXACT_RCP mode), for every sum
an lsdhip_residual_record carries.

The per-point terms are rebuilt in float32 from the oracle's buffers in the operation order of the reference's SSE loops
(calcWeightsAndResidualSSE, calculateWarpUpdateSSE with exact reciprocals, calcResidualAndBuffers for isGood); tests/test_se3_terms_cpu.py
pins them to the oracle (weight_p and dx / dy bit for bit, the oracle's own float32 sums within their rounding).

The SSE loops leave out the last M % 4 in-image points (reference order): A, b, lsError and the weighted error sum the first (M // 4) * 4.
Their sums of absolute values also take the tail points, which the device adds and subtracts again.  retval's squared residuals and
meanRes's signed residuals come from calcResidualAndBuffers, which visits every in-image point: they sum the good ones of all M.
"""
import numpy as np

f32 = np.float32
EPS = 2.0 ** -24          # unit roundoff of float32
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]    # the 21 upper entries of A, in the device's order


def point_terms(tro, fo, lvl, T7, huber_d=3.0, var_weight=1.0, cameraPixelNoise2=None):
    """per-point float32 terms of the oracle's last evaluation (tro = oracle SE3Tracker after evaluate(ref, fo, T7, lvl, ...)).
    Returns a dict of arrays over the M in-image points in reference order."""
    x, y, z = tro.buffer("x"), tro.buffer("y"), tro.buffer("z")
    gx, gy, r = tro.buffer("dx"), tro.buffer("dy"), tro.buffer("residual")
    d, var = tro.buffer("d"), tro.buffer("idepthVar")
    M = len(x)
    if cameraPixelNoise2 is None:
        cameraPixelNoise2 = tro.params.cameraPixelNoise2
    tx, ty, tz = [f32(v) for v in np.asarray(T7, np.float32)[4:7]]
    # calcWeightsAndResidualSSE (exact reciprocals)
    pz2d = f32(1) / ((z * z) * d)
    g0 = (z * tx - x * tz) * pz2d
    g1 = (z * ty - y * tz) * pz2d
    drpdd = g0 * gx + g1 * gy
    w_p = f32(1) / (f32(cameraPixelNoise2) + drpdd * (drpdd * (f32(var_weight) * var)))
    wr = r * np.sqrt(w_p)
    wr = np.maximum(wr, f32(0) - wr)
    hh = f32(huber_d / 2)
    with np.errstate(divide="ignore"):
        wh = np.where(wr < hh, f32(1), hh * (f32(1) / wr)).astype(np.float32)
    werr = wh * (wr * wr)
    w = wh * w_p
    # calculateWarpUpdateSSE
    iz = f32(1) / z
    J = [None] * 6
    J[0] = iz * gx
    J[1] = iz * gy
    J[5] = (x * gy) * iz - (y * gx) * iz
    iz2 = iz * iz
    v1 = (x * gx) * iz2
    v2 = (y * gy) * iz2
    J[2] = f32(0) - (v1 + v2)
    J[3] = f32(0) - ((v2 * y) + (gy + v1 * y))
    J[4] = (gx + v1 * x) + v2 * x
    A = np.stack([(J[i] * w) * J[j] for i, j in UPPER])          # 21 x M
    resw = r * w
    b = np.stack([resw * J[i] for i in range(6)])               # 6 x M (b = -sum)
    err = resw * r
    # calcResidualAndBuffers: isGood needs the gradient taps, re-interpolated from the tracked frame's plane at the warped point
    intr = fo.intrinsics(lvl)
    fx, fy, cx, cy = [f32(v) for v in intr[:4]]
    u = (x / z) * fx + cx
    v = (y / z) * fy + cy
    grad = fo.plane("gradients", lvl)
    wl = grad.shape[1]
    flat = grad.reshape(-1, 4)
    ix, iy = u.astype(np.int32), v.astype(np.int32)
    ddx, ddy = u - ix.astype(np.float32), v - iy.astype(np.float32)
    dxdy = ddx * ddy
    w11, w01, w10, w00 = dxdy, ddy - dxdy, ddx - dxdy, ((f32(1) - ddx) - ddy) + dxdy
    base = ix + iy * wl
    tap = [w11[:, None] * flat[base + 1 + wl], w01[:, None] * flat[base + wl], w10[:, None] * flat[base + 1], w00[:, None] * flat[base]]
    interp = ((tap[0] + tap[1]) + tap[2]) + tap[3]
    rx, ry = interp[:, 0], interp[:, 1]
    good = (r * r) / (f32(40.0 * 40.0) + f32(0.5 * 0.5) * (rx * rx + ry * ry)) < f32(1)
    return dict(M=M, A=A, b=b, err=err, werr=werr, w=w, good=good, r=r, dx=fx * rx, dy=fy * ry)


def oracle_terms64(oracle, tr):
    """float64 accumulation of the oracle's per-point float32 terms of A, b and lsError in SSE operation order (exact reciprocal), the
    weights as the oracle stored them: (A, sum|A terms|, b, sum|b terms|, lsError sum, (M // 4) * 4)."""
    x, y, z = tr.buffer("x"), tr.buffer("y"), tr.buffer("z")
    gx, gy, r, wgt = tr.buffer("dx"), tr.buffer("dy"), tr.buffer("residual"), tr.buffer("weight_p")
    n = (len(x) // 4) * 4
    x, y, z, gx, gy, r, wgt = [a[:n] for a in (x, y, z, gx, gy, r, wgt)]
    pz = f32(1.0) / z
    J = [pz * gx, pz * gy, None, None, None, (x * gy) * pz - (y * gx) * pz]
    pz2 = pz * pz
    v1 = (x * gx) * pz2
    v2 = (y * gy) * pz2
    J[2] = f32(0) - (v1 + v2)
    J[3] = f32(0) - ((v2 * y) + (gy + v1 * y))
    J[4] = (gx + v1 * x) + v2 * x
    A = np.zeros((6, 6))
    Aabs = np.zeros((6, 6))
    for i in range(6):
        Jw = J[i] * wgt
        for j in range(i, 6):
            t = (Jw * J[j]).astype(np.float64)
            A[i, j] = A[j, i] = t.sum()
            Aabs[i, j] = Aabs[j, i] = np.abs(t).sum()
    resw = r * wgt
    b = np.array([-(resw * J[i]).astype(np.float64).sum() for i in range(6)])
    babs = np.array([np.abs((resw * J[i]).astype(np.float64)).sum() for i in range(6)])
    err = (resw * r).astype(np.float64).sum()
    return A, Aabs, b, babs, err, n


def sums64(P, tail="last"):
    """float64 sums and sums of |terms| of every record sum.  tail: which points the SSE drop removes from A, b, lsError and the weighted
    error — "last" (the reference: the last M % 4), "none" (no drop) or "first" (the first M % 4: a wrong tail, for the tests' own power)."""
    M = P["M"]
    n4 = (M // 4) * 4
    keep = np.zeros(M, bool)
    if tail == "last":
        keep[:n4] = True
    elif tail == "none":
        keep[:] = True
    elif tail == "first":
        keep[M - n4:] = True
    else:
        raise ValueError(tail)
    out = {"M": M, "n4": n4}
    for k in ("A", "b", "err", "werr"):
        t = P[k].astype(np.float64)
        out[k] = (t * keep).sum(axis=-1)
        out[k + "_abs"] = np.abs(t).sum(axis=-1)
    out["b"] = -out["b"]
    g = P["good"]
    r = P["r"].astype(np.float64)
    rr = (P["r"] * P["r"]).astype(np.float64)
    out["res2"], out["res2_abs"] = rr[g].sum(), rr[g].sum()
    out["signed"], out["signed_abs"] = r[g].sum(), np.abs(r[g]).sum()
    out["good"] = int(g.sum())
    return out


def terms64(oracle, tro, fo, lvl, T7, tail="last"):
    """sums64(point_terms(...)) in one call"""
    return sums64(point_terms(tro, fo, lvl, T7), tail)
