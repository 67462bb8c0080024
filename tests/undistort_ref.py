"""UndistorterPTAM (util/Undistorter.cpp:91-411, the FOV camera model) restated in numpy, twice:

  * float64 throughout (`build(..., dtype=np.float64)`): the geometry itself, the yardstick of the C++ table builder
    (lsd_slam_hip::Undistorter, include/lsd_slam_hip_io.hpp), which computes in float32 like the reference;
  * `undistort_f32`: the bilinear gather of :384-410 in float32, operation by operation (numpy rounds every float32 operation on its
    own: no fused multiply-add), truncated to a byte with the range clamped — what Undistorter::undistort is held to, byte for byte,
    on the SAME tables.

Also the forward FOV model (`distort_points`), with which the GPU tests render raw images of a rectified scene."""
import os
import subprocess

import numpy as np

from lsd_slam_amd import synth

FOV_EXAMPLE = (0.527334, 0.827306, 0.473568, 0.499436, 0.93)   # the camera of the reference's calib/FOV_example_calib.cfg, dist as the tests use it


EXPLICIT = (0.6, 0.9, 0.5, 0.5, 0.0)      # the five numbers of line 3 in the "explicit" cases


def cfg_text(in5, in_size, line3, out_size):
    """the four lines of a calibration file"""
    return "%s\n%d %d\n%s\n%d %d\n" % (" ".join(repr(float(v)) for v in in5), in_size[0], in_size[1], line3, out_size[0], out_size[1])


def line3_of(mode):
    return "%g %g %g %g %g" % EXPLICIT if mode == "explicit" else mode


def compile_cpp(root, out_dir):
    """tests/cpp/undistort_test.cpp (lsd_slam_hip::Undistorter, plain host C++) -> path of the program"""
    exe = os.path.join(str(out_dir), "undistort_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "undistort_test.cpp"), "-o", exe, "-L" + os.path.join(root, "lsd_slam_amd"), "-llsdhip",
                           "-Wl,-rpath," + os.path.join(root, "lsd_slam_amd")])
    return exe


def cpp_tables(exe, case_dir, text, out_size):
    """the C++ builder on calibration `text` -> dict(dir, cfg, K, outcal, passthrough, same_K[, remapX, remapY float32 [oh, ow]])"""
    os.makedirs(str(case_dir), exist_ok=True)
    cfg = os.path.join(str(case_dir), "calib.cfg")
    with open(cfg, "w") as f:
        f.write(text)
    txt = subprocess.check_output([exe, "tables", cfg, str(case_dir)]).decode()
    rows = {l.split()[0]: l.split()[1:] for l in txt.splitlines()}
    r = {"dir": str(case_dir), "cfg": cfg, "K": np.array(rows["K"], np.float64), "outcal": np.array(rows["outcal"], np.float64),
         "passthrough": rows["passthrough"] == ["1"], "same_K": rows["rectified_cfg_same_K"] == ["1"]}
    if not r["passthrough"]:
        ow, oh = out_size
        r["remapX"] = np.fromfile(os.path.join(str(case_dir), "remapX.f32"), np.float32).reshape(oh, ow)
        r["remapY"] = np.fromfile(os.path.join(str(case_dir), "remapY.f32"), np.float32).reshape(oh, ow)
    return r


def cpp_undistort(exe, tables, imgs, out_size):
    """Undistorter::undistort of the C++ program on uint8 images [n, in_h, in_w] -> [n, oh, ow]"""
    raw, out = os.path.join(tables["dir"], "raw.bin"), os.path.join(tables["dir"], "out.bin")
    np.ascontiguousarray(imgs, dtype=np.uint8).tofile(raw)
    txt = subprocess.check_output([exe, "undistort", tables["cfg"], raw, out]).decode()
    assert "images %d" % len(imgs) in txt, txt
    return np.fromfile(out, np.uint8).reshape(len(imgs), out_size[1], out_size[0])


def random_images(n, w, h, seed):
    """uint8 noise with runs of 0 and of 255 (the values at which the clamp and the truncation act)"""
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    for k in range(n):
        for _ in range(12):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w - 24))
            imgs[k, y:y + int(rng.integers(1, 9)), x:x + int(rng.integers(4, 24))] = 255 if rng.integers(0, 2) else 0
    imgs[0, :, : w // 3] = 255
    imgs[0, :, w // 3: 2 * (w // 3)] = 0
    return imgs


def build(in5, in_w, in_h, mode, out_w, out_h, out5=None, dtype=np.float64):
    """-> dict(K=(fx, fy, cx, cy), out_cal=(5 relative values), remapX, remapY [out_h, out_w] (-1 outside), valid mask).
    mode: "crop" | "full" | "none" | "explicit"."""
    T = dtype
    ic = [T(v) for v in in5]
    dist = ic[4]
    d2t = T(2) * np.tan(dist / T(2))
    fx, fy = ic[0] * T(in_w), ic[1] * T(in_h)
    cx, cy = ic[2] * T(in_w) - T(0.5), ic[3] * T(in_h) - T(0.5)
    if dist == 0:
        ofx, ofy = ic[0] * T(out_w), ic[1] * T(out_h)
        ocx, ocy = ic[2] * T(out_w) - T(0.5), ic[3] * T(out_h) - T(0.5)
    elif mode == "crop":
        l, r, t, b = cx / fx, (T(in_w - 1) - cx) / fx, cy / fy, (T(in_h - 1) - cy) / fy
        tl, tr, tt, tb = (np.tan(v * dist) / d2t for v in (l, r, t, b))
        ofy = fy * ((t + b) / (tt + tb)) * (T(out_h) / T(in_h))
        ocy = (tt / t) * ofy * cy / fy
        ofx = fx * ((l + r) / (tl + tr)) * (T(out_w) / T(in_w))
        ocx = (tl / l) * ofx * cx / fx
    elif mode == "full":
        l, r, t, b = cx / fx, (T(in_w - 1) - cx) / fx, cy / fy, (T(in_h - 1) - cy) / fy
        rtl, rtr, rbl, rbr = np.sqrt(l * l + t * t), np.sqrt(r * r + t * t), np.sqrt(l * l + b * b), np.sqrt(r * r + b * b)
        ttl, ttr, tbl, tbr = (np.tan(v * dist) / d2t for v in (rtl, rtr, rbl, rbr))
        hor = max(rbr, rtr) + max(rbl, rtl)
        vert = max(rtr, rtl) + max(rbl, rbr)
        thor = max(tbr, ttr) + max(tbl, ttl)
        tvert = max(ttr, ttl) + max(tbl, tbr)
        ofy = fy * (vert / tvert) * (T(out_h) / T(in_h))
        ocy = max(ttl / rtl, ttr / rtr) * ofy * cy / fy
        ofx = fx * (hor / thor) * (T(out_w) / T(in_w))
        ocx = max(tbl / rbl, ttl / rtl) * ofx * cx / fx
    elif mode == "explicit":
        oc = [T(v) for v in out5]
        ofx, ofy = oc[0] * T(out_w), oc[1] * T(out_h)
        ocx, ocy = oc[2] * T(out_w) - T(0.5), oc[3] * T(out_h) - T(0.5)
    else:
        raise ValueError("'none' needs dist == 0")
    out_cal = (ofx / T(out_w), ofy / T(out_h), (ocx + T(0.5)) / T(out_w), (ocy + T(0.5)) / T(out_h), T(0))
    K = (out_cal[0] * T(out_w), out_cal[1] * T(out_h), out_cal[2] * T(out_w) - T(0.5), out_cal[3] * T(out_h) - T(0.5))
    x = np.arange(out_w, dtype=T)[None, :]
    y = np.arange(out_h, dtype=T)[:, None]
    ix = np.broadcast_to((x - ocx) / ofx, (out_h, out_w)).astype(T)
    iy = np.broadcast_to((y - ocy) / ofy, (out_h, out_w)).astype(T)
    r = np.sqrt(ix * ix + iy * iy)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = np.where((r == 0) | (dist == 0), T(1), np.arctan(r * d2t) / (dist * r)).astype(T)
    ix = fx * fac * ix + cx
    iy = fy * fac * iy + cy
    ix = np.where(ix == 0, T(0.01), ix)
    iy = np.where(iy == 0, T(0.01), iy)
    ix = np.where(ix == T(in_w - 1), T(in_w - 1.01), ix)
    ix = np.where(iy == T(in_h - 1), T(in_h - 1.01), ix)     # sic (Undistorter.cpp:302); the pixel is invalid either way
    valid = (ix > 0) & (iy > 0) & (ix < in_w - 1) & (iy < in_h - 1)
    return {"K": K, "out_cal": out_cal, "coordX": ix, "coordY": iy, "valid": valid,
            "remapX": np.where(valid, ix, T(-1)), "remapY": np.where(valid, iy, T(-1))}


def undistort_f32(raw, remapX, remapY):
    """Undistorter.cpp:384-410 in float32; raw uint8 [in_h, in_w], tables float32 [out_h, out_w] -> uint8 [out_h, out_w]"""
    f = np.float32
    in_h, in_w = raw.shape
    xx = remapX.astype(f)
    yy = remapY.astype(f)
    valid = ~(xx < 0)
    xs = np.where(valid, xx, f(0))
    ys = np.where(valid, yy, f(0))
    xi = xs.astype(np.int32)
    yi = ys.astype(np.int32)
    xx = xs - xi.astype(f)
    yy = ys - yi.astype(f)
    xxyy = xx * yy
    flat = raw.reshape(-1)
    base = xi + yi * in_w
    lim = flat.size - 1
    s00 = flat[np.minimum(base, lim)].astype(f)
    s10 = flat[np.minimum(base + 1, lim)].astype(f)
    s01 = flat[np.minimum(base + in_w, lim)].astype(f)
    s11 = flat[np.minimum(base + in_w + 1, lim)].astype(f)
    v = ((xxyy * s11 + (yy - xxyy) * s01) + (xx - xxyy) * s10) + (((f(1) - xx) - yy) + xxyy) * s00
    assert v.dtype == np.float32
    b = np.where(v > 0, np.where(v >= 255, f(255), np.trunc(v)), f(0)).astype(np.uint8)
    return np.where(valid, b, np.uint8(0)).astype(np.uint8)


def distort_points(xu, yu, K_rect, in5, in_w, in_h):
    """Forward FOV model in float64: pixel (xu, yu) of the rectified camera K_rect -> pixel of the raw camera
    (r_d = atan(r_u * 2 tan(dist / 2)) / dist), the inverse direction of the table's."""
    fx, fy = in5[0] * in_w, in5[1] * in_h
    cx, cy = in5[2] * in_w - 0.5, in5[3] * in_h - 0.5
    dist = in5[4]
    d2t = 2.0 * np.tan(dist / 2.0)
    ix = (np.asarray(xu, np.float64) - K_rect[2]) / K_rect[0]
    iy = (np.asarray(yu, np.float64) - K_rect[3]) / K_rect[1]
    r = np.sqrt(ix * ix + iy * iy)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = np.where((r == 0) | (dist == 0), 1.0, np.arctan(r * d2t) / (dist * r))
    return fx * fac * ix + cx, fy * fac * iy + cy


def undistort_points(xd, yd, K_rect, in5, in_w, in_h):
    """Inverse of distort_points: pixel of the raw camera -> pixel of the rectified camera (r_u = tan(r_d * dist) / (2 tan(dist / 2)))."""
    fx, fy = in5[0] * in_w, in5[1] * in_h
    cx, cy = in5[2] * in_w - 0.5, in5[3] * in_h - 0.5
    dist = in5[4]
    d2t = 2.0 * np.tan(dist / 2.0)
    ix = (np.asarray(xd, np.float64) - cx) / fx
    iy = (np.asarray(yd, np.float64) - cy) / fy
    r = np.sqrt(ix * ix + iy * iy)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = np.where((r == 0) | (dist == 0), 1.0, np.tan(r * dist) / (d2t * r))
    return K_rect[0] * fac * ix + K_rect[2], K_rect[1] * fac * iy + K_rect[3]


# ---- raw images of the synthetic scene -------------------------------------------------------------------------------------------
def cast_rays(scene, i, dx, dy):
    """lsd_slam_amd.synth.Scene.render for arbitrary viewing rays (dx, dy, 1) of camera i, in float64: grey values (not yet rounded) and depth"""
    R, C = scene.cam_to_world(i)
    d = np.stack([dx, dy, np.ones_like(dx)], axis=-1)
    dw = d @ R.T
    lam = np.full(dx.shape, 2.0)
    for _ in range(6):
        X = C[0] + lam * dw[..., 0]
        Y = C[1] + lam * dw[..., 1]
        f = C[2] + lam * dw[..., 2] - synth._surface(X, Y)
        gx, gy = synth._surface_grad(X, Y)
        lam = lam - f / (dw[..., 2] - gx * dw[..., 0] - gy * dw[..., 1])
    T = scene.texture(C[0] + lam * dw[..., 0], C[1] + lam * dw[..., 1])
    return T, lam


def raw_sequence(seq_index, n, K_rect, in5, in_size, out_size):
    """The synth.py scene as the raw FOV camera sees it: every raw pixel is taken back to the rectified camera K_rect through the FOV model
    (r_u = tan(r_d dist) / (2 tan(dist / 2)), the inverse of r_d = atan(r_u 2 tan(dist / 2)) / dist) and the scene is rendered along that
    ray, in float64 — the rectified images then show the scene as a pinhole camera K_rect sees it, consistent with the depth of frame 0
    rendered at K_rect.  -> raw uint8 [n, in_h, in_w], depth0 float32 [out_h, out_w]"""
    sc = synth.Scene(seq_index, "S1", n)
    K = [float(v) for v in K_rect]
    xd, yd = np.meshgrid(np.arange(in_size[0], dtype=np.float64), np.arange(in_size[1], dtype=np.float64))
    xu, yu = undistort_points(xd, yd, K, in5, in_size[0], in_size[1])
    bx, by = distort_points(xu, yu, K, in5, in_size[0], in_size[1])
    assert np.abs(bx - xd).max() < 1e-9 and np.abs(by - yd).max() < 1e-9          # the forward model takes them back
    raws = np.zeros((n, in_size[1], in_size[0]), np.uint8)
    for i in range(n):
        T, _ = cast_rays(sc, i, (xu - K[2]) / K[0], (yu - K[3]) / K[1])
        raws[i] = np.clip(np.rint(T), 0, 255).astype(np.uint8)
    u, v = np.meshgrid(np.arange(out_size[0], dtype=np.float64), np.arange(out_size[1], dtype=np.float64))
    _, depth0 = cast_rays(sc, 0, (u - K[2]) / K[0], (v - K[3]) / K[1])
    return raws, depth0.astype(np.float32)
