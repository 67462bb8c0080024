"""float32 numpy restatement of include/lsd_slam_hip_io.hpp's keyframe export — the payload fill loop of makeKeyframeMsg and
flushPointCloud (KeyFrameDisplay::flushPC) — with every intermediate an explicit np.float32, in the header's operation order.
tests/test_cloud_ref_cpu.py pins it to the header bit for bit; tests/test_cloud_gpu.py holds the device export to it.
Also the test maps both files use."""
import numpy as np

F = np.float32
POINT_DTYPE = np.dtype([("idepth", "<f4"), ("idepth_var", "<f4"), ("color", "u1", 4)])

IDENTITY_POSE = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


def wire_pose(axis, angle, scale, t):
    """camToWorld in the message's wire form: quaternion (x, y, z, w) with norm = scale, then the translation"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    q = np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]]) * scale
    return np.concatenate([q, np.asarray(t, np.float64)]).astype(np.float32)


POSE_ROT1 = wire_pose([0.3, -0.5, 0.8], 0.7, 1.0, [0.25, -1.5, 3.0])     # scale 1, non-trivial rotation
POSE_ROT2 = wire_pose([-0.6, 0.2, 0.7], 1.1, 2.0, [1.0, -2.0, 0.5])      # scale 2


def pack_ref(idepth, var, image):
    """makeKeyframeMsg's fill loop: (idepth, idepth_var, (unsigned char)image four times) per pixel"""
    out = np.zeros(idepth.shape, POINT_DTYPE)
    out["idepth"] = idepth.astype(F)
    out["idepth_var"] = var.astype(F)
    out["color"] = image.astype(F).astype(np.int32).astype(np.uint8)[..., None]
    return out


def cloud_constants(K4, c2w):
    fx, fy, cx, cy = (F(v) for v in K4)
    c2w = np.asarray(c2w, F)
    qx, qy, qz, qw = c2w[0], c2w[1], c2w[2], c2w[3]
    n = np.sqrt(F(F(F(F(qx * qx) + F(qy * qy)) + F(qz * qz)) + F(qw * qw)))
    return dict(fxi=F(F(1) / fx), fyi=F(F(1) / fy), cxi=F(F(-cx) / fx), cyi=F(F(-cy) / fy), scale=F(n),
                ux=F(qx / n), uy=F(qy / n), uz=F(qz / n), uw=F(qw / n), t=c2w[4:7].copy())


def flush_ref(points, K4, c2w, scaledTH=1.0, absTH=1.0, minNearSupport=5):
    """flushPointCloud on a [h, w] POINT_DTYPE array -> (xyzi float32 [n, 4] in pixel order, info).  info: the keep mask and the
    number of candidates and of rejections by each of the three filters."""
    h, w = points.shape
    k = cloud_constants(K4, c2w)
    idp = points["idepth"].astype(F)
    var = points["idepth_var"].astype(F)
    scaledTH, absTH = F(scaledTH), F(absTH)
    interior = np.zeros((h, w), bool)
    interior[1:h - 1, 1:w - 1] = True
    with np.errstate(all="ignore"):
        cand = interior & ~(idp <= F(0))
        depth = F(1) / idp
        depth4 = depth * depth
        depth4 = depth4 * depth4
        a = var * depth4
        r1 = cand & (a > scaledTH)
        r2 = cand & ~r1 & ((a * k["scale"]) * k["scale"] > absTH)
        ok = cand & ~r1 & ~r2
        r3 = np.zeros((h, w), bool)
        if minNearSupport > 1:
            ref = F(1) / depth
            pad = np.zeros((h + 2, w + 2), F)
            pad[1:-1, 1:-1] = idp
            near = np.zeros((h, w), np.int32)
            two_var = F(2) * var
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                    diff = q - ref
                    near += ((q > F(0)) & (diff * diff < two_var)).astype(np.int32)
            r3 = ok & (near < minNearSupport)
        keep = ok & ~r3
        ys, xs = np.nonzero(keep)                      # row-major: the host loop's order
        d = depth[ys, xs]
        s = k["scale"]
        v0 = ((xs.astype(F) * k["fxi"] + k["cxi"]) * d) * s
        v1 = ((ys.astype(F) * k["fyi"] + k["cyi"]) * d) * s
        v2 = d * s
        ux, uy, uz, uw = k["ux"], k["uy"], k["uz"], k["uw"]
        tx = F(2) * (uy * v2 - uz * v1)
        ty = F(2) * (uz * v0 - ux * v2)
        tz = F(2) * (ux * v1 - uy * v0)
        out = np.zeros((len(ys), 4), F)
        out[:, 0] = ((v0 + uw * tx) + (uy * tz - uz * ty)) + k["t"][0]
        out[:, 1] = ((v1 + uw * ty) + (uz * tx - ux * tz)) + k["t"][1]
        out[:, 2] = ((v2 + uw * tz) + (ux * ty - uy * tx)) + k["t"][2]
        out[:, 3] = points["color"][ys, xs, 2].astype(F) / F(255)
    assert out.dtype == F and depth.dtype == F and a.dtype == F
    info = dict(keep=keep, candidates=int(cand.sum()), rej_scaled=int(r1.sum()), rej_abs=int(r2.sum()), rej_support=int(r3.sum()), kept=len(ys))
    return out, info


def make_map(w, h, seed):
    """A semi-dense test map (idepth, var) on which every branch of flushPC both fires and passes:
    a smooth slanted surface (neighbours support each other); ~15 % invalid pixels as idepth <= 0 (zeros and negative values) — which also
    starve the 3x3 support count of their neighbours; isolated outliers nobody supports; variances over six decades, the largest beyond
    var * depth^4 = 1 and a band in between that only the absolute threshold of a scale-2 pose (or a tighter absTH) cuts; a border band
    three pixels deep that is valid, smooth and well supported — so rows / columns 1 and w - 2 / h - 2 keep points and row / column 0 and
    the last ones hold valid pixels that must never come out; valid smooth patches across every chunk boundary (multiples of 1024
    pixels), including those where the boundary falls near a row end."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    idepth = (0.6 + 0.2 * xx / w + 0.1 * yy / h).astype(F)
    var = (10.0 ** rng.uniform(-6.5, -1.5, (h, w))).astype(F)
    u = rng.random((h, w))
    var[u < 0.06] = (10.0 ** rng.uniform(-0.4, 0.4, (h, w))).astype(F)[u < 0.06]                  # around and beyond var * depth^4 = 1
    var[(u >= 0.06) & (u < 0.12)] = rng.uniform(0.06, 0.12, (h, w)).astype(F)[(u >= 0.06) & (u < 0.12)]   # var * depth^4 in (0.25, 1): absolute only
    out = rng.random((h, w)) < 0.04                                                               # outliers with a tight variance
    idepth[out] *= F(1.6)
    var[out] = F(1e-6)
    inv = rng.random((h, w))
    idepth[inv < 0.05] = F(0)
    idepth[(inv >= 0.05) & (inv < 0.10)] = F(-1)
    idepth[(inv >= 0.10) & (inv < 0.15)] = -rng.uniform(0.01, 3.0, (h, w)).astype(F)[(inv >= 0.10) & (inv < 0.15)]
    smooth = (0.6 + 0.2 * xx / w + 0.1 * yy / h).astype(F)
    band = (xx < 3) | (xx >= w - 3) | (yy < 3) | (yy >= h - 3)
    for b in range(1024, w * h, 1024):                  # pixels b - 1 | b sit in different chunks
        y, x = divmod(b, w)
        band |= (np.abs(yy - y) <= 2) & (np.abs(xx - x) <= 6)
        if x < 8:                                       # the boundary lies at a row end: the support crosses both
            band |= ((np.abs(yy - (y - 1)) <= 1) & (xx >= w - 4)) | ((np.abs(yy - y) <= 1) & (xx <= 3))
    idepth[band] = smooth[band]
    var[band] = F(1e-3)
    return idepth, var


def dense_map(w, h):
    return np.full((h, w), 0.5, F), np.full((h, w), 1e-3, F)


def invalid_map(w, h):
    idepth = np.zeros((h, w), F)
    idepth[::2] = F(-1)
    return idepth, np.full((h, w), 1e-3, F)
