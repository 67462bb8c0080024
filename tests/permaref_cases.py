"""Inputs of the explicit-point-list tests (trackFrameOnPermaref, checkPermaRefOverlap: tests/test_permaref_eval_gpu.py,
tests/test_permaref_loop_gpu.py) and the host-side restatements they are held to; tests/test_permaref_cases_cpu.py pins the restatements to
the oracle and asserts, on the oracle alone, that these inputs can expose a wrong kernel.

Clouds.  The C ABI takes any list of (pos[3], colour, variance), so besides keyframe-derived level-4 clouds there are synthetic ones, which
reach what no keyframe reaches: random sub-pixel level-4 positions over [-2, w4 + 2] x [-2, h4 + 2] back-projected at depths 0.5 .. 5,
colours from the level-4 image plus noise (small for most points, large for a fifth of them: Huber inliers and outliers, good and bad
points), variances 1e-4 .. 1e-1 (log-uniform), the order permuted (the SSE tail drop follows LIST order; a keyframe's own order would be
the column order of its pixel grid as well).  SIZES are the list lengths at which the tiling changes (track_plan.hpp lsd_level_tiling:
one tile per 256 points, multiples of 8 tiles from 16 on — 4097 points: 17 tiles rounded up to 24, seven of them empty; 4836 = 78 x 62, the
level-4 bound at 1280x1024, 19 -> 24 tiles, 16 in a batch of 16 or more jobs: multi-pass; 25000: above LSD_SPEC_CAP_ABOVE_PX).

Crafted points (crafted_block, per pose): points whose float32 u_new / v_new, as calcResidualAndBuffers and checkPermaRefOverlap compute
them, lie ON and within a few ulps on either side of every border either function compares with (1, w4 - 2, h4 - 2; 0, w4 - 1, h4 - 1),
points with Wz < 0 that project inside the image, one point with Wz == 0, and duplicates.

Poses (referenceToFrame): identity, a small general twist, one at which most points leave the image, one with t_z < 0 that puts the near
points behind the camera, and a pure approach (every depthChange >= 1: every overlap term is exactly 1).

Restatements: project() is the float32 projection both functions share (Eigen's coefficient order); overlap_terms() is
checkPermaRefOverlap per point; the evaluation's per-point terms are se3_terms.point_terms on the oracle's buffers after evaluate_points.

The LM-loop cases (loop_cases) and their margins: see loop_margin().  tests/test_permaref_cases_cpu.py::
test_loop_cases_are_clear_and_reach_every_branch prints m per case and the largest m over the clear cases: 9.08e-2 where this was recorded
("syn16 near", a sixteen-point list; 4.03e-2 among the lists of 63 points or more, "kf-dense near").  The SSE mode's _mm_rcp_ps
differs between processors, so m and the set of clear cases differ a little from host to host; the test holds the unclear cases to a
quarter and asserts that every branch is reached by at least one clear case, the case list giving each branch three or more."""
import numpy as np

from common import sequence
from se3_terms import EPS, sums64

f32 = np.float32
LEVEL = 4                      # QUICK_KF_CHECK_LVL
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1064, 4097, 4836, 25000]
GRID_CAP, BLOCK = 304, 256     # lsdhip_tracker::grid_cap (lsd_grid_cap(304, 256, 41) = 304), the step kernel's workgroup
C_TERM = {"A": 126, "b": 112, "err": 98, "werr": 96}     # per-term roundings, both sides (tests/test_track_batch_eval_gpu.py)


def ceil_div(a, b):
    return -(-a // b)


# ---- tiling and summation depth of a point list (track_plan.hpp, tracker.hip) --------------------------------------------------------------
def tiles_for(n, jobs=1, cap=None):
    """(workgroups, single pass) of a list of n points in a batch of `jobs` jobs (1: the single job): lsd_level_tiling with
    lsd_batch_shape's cap — one tile per 256 points, multiples of 8 from 16 tiles on, at most the cap: grid_cap for one job, grid_cap / jobs
    rounded down to a multiple of 8 and at least 16 in a batch.  cap: a workgroup cap of its own (speculation under
    lsdhip_tracker_set_speculation)."""
    nb = ceil_div(n, BLOCK)
    if nb >= 16:
        nb = (nb + 7) & ~7
    if cap is None:
        cap = GRID_CAP if jobs <= 1 else max(16, (GRID_CAP // jobs) & ~7)
    nb = max(1, min(nb, cap))
    return nb, int(nb * BLOCK >= n)


def single_tiles(n, policy):
    """the tiling of a single job's list under a speculation policy (lsd_single_plan): None = the default policy, which caps lists above
    LSD_SPEC_CAP_ABOVE_PX = 24576 points at 80 tiles; (6, 8) = lsdhip_tracker_set_speculation(t, 6, 8), 8 tiles at most; (1, 0): no cap.
    tests/cpp/track_plan_test.cpp holds lsd_single_plan to the same table test_permaref_cases_cpu.py holds this to."""
    if policy == (1, 0):
        return tiles_for(n)
    if policy == (6, 8):
        return tiles_for(n, cap=8)
    return tiles_for(n, cap=80 if n > 24576 else None)


def depth_for(n, jobs=1):
    """summation depth of one term of a list of n points (tests/test_permaref_eval_gpu.py states the derivation)"""
    nb, _ = tiles_for(n, jobs)
    return ceil_div(n, BLOCK * nb) + 43 + 5 + ceil_div(nb, 16) + 15 + 3


# ---- poses ------------------------------------------------------------------------------------------------------------------------------
def pose_cast_f32(T7):
    """SE3d::cast<float>() (the quaternion re-normalised in float, oracle/orc_math.hpp) -> (q wxyz, t) in float32"""
    T7 = np.asarray(T7, np.float64)
    w, x, y, z = [f32(v) for v in T7[:4]]
    n = np.sqrt(((x * x + y * y) + z * z) + w * w)
    return np.array([w / n, x / n, y / n, z / n], f32), np.array(T7[4:7], f32)


def rot_f32(q):
    """Eigen QuaternionBase::toRotationMatrix in float32 (q = w x y z)"""
    w, x, y, z = [f32(v) for v in q]
    two = f32(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = f32(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], f32)


def project(pos, q, t, intr):
    """Wxp = R p + t and (u_new, v_new) as calcResidualAndBuffers / checkPermaRefOverlap compute them, in float32"""
    pos = np.asarray(pos, f32)
    R = rot_f32(q)
    px, py, pz = pos[:, 0], pos[:, 1], pos[:, 2]
    W = [((R[i, 0] * px + R[i, 1] * py) + R[i, 2] * pz) + f32(t[i]) for i in range(3)]
    fx, fy, cx, cy = [f32(v) for v in intr[:4]]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = (W[0] / W[2]) * fx + cx
        v = (W[1] / W[2]) * fy + cy
    return W[0], W[1], W[2], u, v


BORDERS_EVAL = ("u>1", "v>1", "u<w-2", "v<h-2")
BORDERS_OVERLAP = ("u>0", "v>0", "u<w-1", "v<h-1")


def inside(u, v, w4, h4, lo, hi, loose=None):
    """lo < u < w4 - hi and lo < v < h4 - hi (lo, hi = 1, 2: the evaluation; 0, 1: the overlap).  loose: index 0..3 of the one comparison
    taken as >= / <= instead (a wrong kernel, for the tests' own power)"""
    lo_, wu, hv = f32(lo), f32(w4 - hi), f32(h4 - hi)
    with np.errstate(invalid="ignore"):
        c = [u > lo_, v > lo_, u < wu, v < hv]
        if loose is not None:
            c[loose] = [u >= lo_, v >= lo_, u <= wu, v <= hv][loose]
    return c[0] & c[1] & c[2] & c[3]


def border_attainable(intr, axis, border):
    """can u_new (axis 0) or v_new (axis 1) = r f + c equal `border` for any float32 ratio r = W / Wz?  The product r f steps by
    f ulp(r), which may be coarser than the ulp of border - c: then some borders are never hit, and on such a camera `>` and `>=` are the
    same function.  Exhaustive over the ratios around (border - c) / f (the product is monotonic in r)."""
    f, c = f32(intr[axis]), f32(intr[2 + axis])
    r0 = f32((float(border) - float(c)) / float(f))
    r = r0 + np.arange(-4096, 4097).astype(f32) * np.spacing(np.abs(r0))
    val = r.astype(f32) * f + c
    assert val[0] < f32(border) < val[-1] or val[-1] < f32(border) < val[0]
    return bool(np.any(val == f32(border)))


def overlap_terms(pos, T7, intr, w4, h4, loose=None):
    """checkPermaRefOverlap per point: (float32 terms, in-image mask); terms are 0 outside the image"""
    q, t = pose_cast_f32(T7)
    _, _, Wz, u, v = project(pos, q, t, intr)
    m = inside(u, v, w4, h4, 0, 1, loose)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dc = np.asarray(pos, f32)[:, 2] / Wz
    term = np.where(dc < f32(1), dc, f32(1)).astype(f32)
    term[~m] = 0
    return term, m


def overlap_usage_f32(term, m, n):
    """the reference's own sum: float32, one in-image point after the other, then the division by the list length"""
    s = np.cumsum(term[m], dtype=f32)[-1] if m.any() else f32(0)
    return f32(s) / f32(n)


def overlap_bound(term, n):
    """|usage n - sum64| <= (ceil(n / 256) + 6 + 3 + 2) EPS sum|terms|: the lane-strided run, the wave sum, the four wave totals, the
    1-ulp reciprocal and the final division"""
    return (ceil_div(n, 256) + 6 + 3 + 2) * EPS * float(np.abs(term.astype(np.float64)).sum())


# ---- scenes and clouds --------------------------------------------------------------------------------------------------------------------
class Scene:
    """one image size: the synthetic sequence, the oracle's frames, the level-4 intrinsics and image"""

    def __init__(self, oracle, w, h):
        self.oracle, self.w, self.h = oracle, w, h
        self.w4, self.h4 = w >> LEVEL, h >> LEVEL
        self.frames, self.depth0, self.K, self.gt = sequence(w, h, 4, 0)
        self.fo = [oracle.Frame(i, self.frames[i], self.K) for i in range(4)]
        self.intr = self.fo[0].intrinsics(LEVEL)
        self.image4 = self.fo[0].plane("image", LEVEL)
        self._clouds = {}

    def tracker(self, mode=None):
        o = self.oracle
        return o.SE3Tracker(self.w, self.h, self.K, mode=o.SSE_EXACT_RCP if mode is None else mode)

    def backproject(self, u, v, z):
        fx, fy, cx, cy = [float(x) for x in self.intr[:4]]
        return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)

    def colours(self, rng, u, v):
        """level-4 image at the nearest pixel plus noise: sigma 2 for most points, sigma 60 for a fifth"""
        ix = np.clip(np.rint(u).astype(int), 0, self.w4 - 1)
        iy = np.clip(np.rint(v).astype(int), 0, self.h4 - 1)
        sigma = np.where(rng.uniform(size=len(u)) < 0.2, 60.0, 2.0)
        return self.image4[iy, ix] + rng.normal(0, 1, len(u)) * sigma

    def synthetic(self, n, seed=0, crafted=None):
        """n points (crafted: a block of points placed among them, n unchanged)"""
        key = ("syn", n, seed, crafted is not None)
        if key in self._clouds:
            return self._clouds[key]
        rng = np.random.default_rng(1000 * seed + n + self.w)
        u = rng.uniform(-2, self.w4 + 2, n)
        v = rng.uniform(-2, self.h4 + 2, n)
        z = rng.uniform(0.5, 5.0, n)
        pos = self.backproject(u, v, z).astype(f32)
        cv = np.stack([self.colours(rng, u, v), 10.0 ** rng.uniform(-4, -1, n)], axis=1).astype(f32)
        if crafted is not None:
            cpos, ccv = crafted
            assert len(cpos) <= n
            pos[:len(cpos)], cv[:len(cpos)] = cpos, ccv
        order = rng.permutation(n)
        self._clouds[key] = (np.ascontiguousarray(pos[order]), np.ascontiguousarray(cv[order]))
        return self._clouds[key]

    def keyframe_planes(self, kind):
        d = self.depth0.copy()
        if kind == "gt":
            return d, None
        d[~(d > 0)] = np.median(self.depth0[self.depth0 > 0])      # dense: a hypothesis on every pixel
        return (1.0 / d).astype(f32), np.full_like(d, 1e-4, dtype=f32)

    def keyframe_cloud(self, kind, permute=True):
        """the level-4 cloud of keyframe 0 with ground-truth depth ("gt") or a hypothesis on every pixel ("dense": (w4 - 2)(h4 - 2) points)"""
        key = ("kf", kind, permute)
        if key in self._clouds:
            return self._clouds[key]
        o = self.oracle
        kfo = o.Frame(100, self.frames[0], self.K)
        d, var = self.keyframe_planes(kind)
        if var is None:
            kfo.set_depth_gt(d)
        else:
            kfo.set_depth_planes(d, var)
        ro = o.TrackingReference()
        ro.import_frame(kfo)
        pos, cv, _, _ = ro.pointcloud(LEVEL)
        if permute:
            order = np.random.default_rng(7).permutation(len(pos))
            pos, cv = np.ascontiguousarray(pos[order]), np.ascontiguousarray(cv[order])
        self._clouds[key] = (pos, cv, ro)
        return self._clouds[key]

    # -- poses (referenceToFrame as float32[7]: q w x y z, t) -----------------------------------------------------------------------------
    def poses(self):
        o = self.oracle
        e = lambda a: o.se3_exp(np.array(a, np.float64)).astype(f32)          # noqa: E731
        return {"identity": np.array([1, 0, 0, 0, 0, 0, 0], f32),
                "twist": e([0.05, -0.03, 0.02, 0.01, -0.02, 0.03]),
                "leaves": e([0.9, 0.1, 0.0, 0.0, 0.35, 0.0]),
                "behind": e([0.02, 0.01, -1.2, 0.0, 0.01, 0.0]),             # t_z < 0: points nearer than 1.2 end up behind the camera
                "approach": np.array([1, 0, 0, 0, 0, 0, -0.2], f32)}          # Wz = pz - 0.2 < pz: every depthChange > 1

    # -- crafted points ---------------------------------------------------------------------------------------------------------------
    def crafted_block(self, T7, seed=0):
        """points next to every border either function compares u_new / v_new with, at the pose T7 (float32[7], unit quaternion as
        given: the evaluation takes it as it is, the overlap's float re-normalisation is pinned separately), found by a search over
        float32 neighbours of an exact back-projection; Wz < 0 points that project inside, one Wz == 0 point, duplicates.
        Returns (pos, colvar, found) with found[(axis, border value)] = the set of {-1, 0, +1} sides reached."""
        rng = np.random.default_rng(77 + seed)
        q, t = np.asarray(T7[:4], f32), np.asarray(T7[4:7], f32)
        R64 = rot_f32(q).astype(np.float64)
        w4, h4 = self.w4, self.h4
        pts, found = [], {}

        def back(u, v, z):       # frame coordinates -> reference coordinates, in float64
            Wp = self.backproject(np.atleast_1d(u), np.atleast_1d(v), np.atleast_1d(z))
            return (Wp - t.astype(np.float64)) @ R64          # R^T (Wp - t), row vectors

        for axis, borders in ((0, (0, 1, w4 - 2, w4 - 1)), (1, (0, 1, h4 - 2, h4 - 1))):
            for bval in borders:
                # u_new = (Wx / Wz) fx + cx: the values it can take next to the border are spaced by the ulp of the larger of the border
                # and the principal point, the operands of its last addition.  "Next to" = within 4 such steps; ON the border where the
                # product (Wx / Wz) fx can take the value border - cx at all.
                b32 = f32(bval)
                step = float(np.spacing(max(abs(b32), abs(f32(self.intr[2 + axis])))))
                sides = set()
                for attempt in range(6):
                    other = rng.uniform(3, (h4 if axis == 0 else w4) - 4)
                    z = rng.uniform(1.5, 4.0)
                    uv = (bval, other) if axis == 0 else (other, bval)
                    p0 = back(uv[0], uv[1], z)[0].astype(f32)
                    # float32 neighbours of p0: steps of a few ulps in every coordinate
                    k = rng.integers(-60, 61, (20000, 3))
                    cand = (p0[None, :] + k.astype(f32) * np.spacing(np.abs(p0))[None, :]).astype(f32)
                    _, _, _, u, v = project(cand, q, t, self.intr)
                    val = (u if axis == 0 else v)
                    off = (val.astype(np.float64) - float(b32)) / step
                    for side, sel in ((-1, (off < 0) & (off >= -4)), (0, val == b32), (1, (off > 0) & (off <= 4))):
                        idx = np.flatnonzero(sel)
                        if len(idx) and side not in sides:
                            pts.extend(cand[idx[:2]])
                            sides.add(side)
                    if len(sides) == 3:
                        break
                found[(axis, bval)] = sides
        # Wz < 0, projecting inside the image: the mirror image of an inside point through the camera centre
        for _ in range(6):
            u, v, z = rng.uniform(3, w4 - 4), rng.uniform(3, h4 - 4), -rng.uniform(0.5, 3.0)
            pts.append(back(u, v, z)[0].astype(f32))
        # Wz == 0: search the float32 neighbours of a point on the plane Wz = 0
        p0 = back(rng.uniform(3, w4 - 4), rng.uniform(3, h4 - 4), 1.0)[0]
        p0 = (p0 - R64[2] * (R64[2] @ p0 + float(t[2]))).astype(f32)         # projected onto the plane (R p + t)_z = 0
        k = rng.integers(-200, 201, (40000, 3))
        cand = (p0[None, :] + k.astype(f32) * np.spacing(np.abs(p0) + f32(1e-6))[None, :]).astype(f32)
        cand[0] = p0
        Wz = project(cand, q, t, self.intr)[2]
        zero = np.flatnonzero(Wz == 0)
        found["Wz==0"] = len(zero) > 0
        if len(zero):
            pts.append(cand[zero[0]])
        pts = np.array(pts, f32)
        pts = np.concatenate([pts, pts[::3]])                                  # duplicates
        _, _, _, u, v = project(pts, q, t, self.intr)
        with np.errstate(invalid="ignore"):
            uu = np.where(np.isfinite(u), u, 0)
            vv = np.where(np.isfinite(v), v, 0)
        cv = np.stack([self.colours(rng, uu, vv), 10.0 ** rng.uniform(-4, -1, len(pts))], axis=1).astype(f32)
        return pts, cv, found

    def crafted_cloud(self):
        """the crafted blocks of every pose, and random points between them, permuted"""
        if "crafted" in self._clouds:
            return self._clouds["crafted"]
        blocks, founds = [], {}
        for i, (name, T) in enumerate(self.poses().items()):
            p, c, fnd = self.crafted_block(T, i)
            blocks.append((p, c))
            founds[name] = fnd
        cpos = np.concatenate([b[0] for b in blocks])
        ccv = np.concatenate([b[1] for b in blocks])
        n = len(cpos) + 101
        pos, cv = self.synthetic(n, seed=5, crafted=(cpos, ccv))
        self._clouds["crafted"] = (pos, cv, founds)
        return self._clouds["crafted"]


# ---- the evaluation cases ------------------------------------------------------------------------------------------------------------------
def eval_clouds(sc):
    """name -> (pos, colvar) of one scene"""
    out = {}
    if (sc.w, sc.h) == (320, 240):
        for n in SIZES:
            out["syn%d" % n] = sc.synthetic(n)
        out["crafted"] = sc.crafted_cloud()[:2]
        out["kf-gt"] = sc.keyframe_cloud("gt")[:2]
        out["kf-dense-in-order"] = sc.keyframe_cloud("dense", permute=False)[:2]
    elif (sc.w, sc.h) == (640, 480):
        for n in (5, 257, 1064, 4097):
            out["syn%d" % n] = sc.synthetic(n)
        out["crafted"] = sc.crafted_cloud()[:2]
        out["kf-dense"] = sc.keyframe_cloud("dense")[:2]            # 38 x 28 = 1064 points
    else:
        out["kf-dense"] = sc.keyframe_cloud("dense")[:2]            # 1280x1024: 78 x 62 = 4836 points
        out["syn1"] = sc.synthetic(1)
    return out


AFFINE = [(1.0, 0.0), (1.03, -2.5), (0.97, 1.5)]
POSES = ["identity", "twist", "leaves", "behind", "approach"]
SCENES = [(320, 240), (640, 480), (1280, 1024)]


def form_batches(form):
    """The evaluation test's case list of one form: a list of batches (scene size, [job, ...]), job = (cloud name, pose name, tracked
    frame 1..3, index into AFFINE).  Forms: "single" (every cloud at every pose), "batch2" / "batch3" / "batch5" (mixed counts, a 1-point
    list beside the 4836-point one), "batch16" / "batch24" (16 tiles per job: lists above 4096 points are multi-pass)."""
    out = []
    if form == "single":
        for size in SCENES:
            k = 0
            for name in CLOUD_NAMES[size]:
                for pose in (POSES if size != (1280, 1024) else POSES[:3]):
                    out.append((size, [(name, pose, 1 + k % 3, k % 3)]))
                    k += 1
        return out
    mixes = {"batch2": [["kf-dense", "syn1"]], "batch3": [["syn4", "syn1064", "syn65"], ["syn5", "crafted", "syn257"]],
             "batch5": [["syn1", "syn4836", "syn63", "crafted", "kf-gt"], ["syn3", "syn4097", "syn256", "syn64", "syn255"]]}
    if form in mixes:
        for pi, pose in enumerate(POSES):
            for mix in mixes[form]:
                size = (1280, 1024) if form == "batch2" else (320, 240)
                out.append((size, [(name, POSES[(pi + j) % 5] if j % 2 else pose, 1 + (pi + j) % 3, (pi + j) % 3) for j, name in enumerate(mix)]))
        if form == "batch2":
            for pi, pose in enumerate(POSES):
                out.append(((320, 240), [("syn4836", pose, 1 + pi % 3, pi % 3), ("syn1", POSES[(pi + 1) % 5], 2, 1)]))
        return out
    n = {"batch16": 16, "batch24": 24}[form]
    cyc = ["syn4836", "syn4097", "syn257", "crafted", "syn1064", "syn3", "kf-dense-in-order", "syn25000", "syn4836", "syn65", "syn1"]
    out.append(((320, 240), [(cyc[j % len(cyc)], POSES[(j + j // 5) % 5], 1 + j % 3, j % 3) for j in range(n)]))
    out.append(((1280, 1024), [("kf-dense" if j % 4 else "syn1", POSES[j % 5], 1 + j % 3, (j + 1) % 3) for j in range(1, n + 1)]))
    return out


CLOUD_NAMES = {(320, 240): ["syn%d" % n for n in SIZES] + ["crafted", "kf-gt", "kf-dense-in-order"],
               (640, 480): ["syn5", "syn257", "syn1064", "syn4097", "crafted", "kf-dense"],
               (1280, 1024): ["kf-dense", "syn1"]}
FORMS = ["single", "batch2", "batch3", "batch5", "batch16", "batch24"]
# the bank's forms read keyframes' own clouds (in the keyframe's order): (scene size, [(keyframe kind, pose, frame, affine), ...])
BANK_BATCHES = {"bank1": [(size, [(kind, pose, 1 + (i + j) % 3, (i + j) % 3)]) for size in SCENES for i, kind in enumerate(("gt", "dense"))
                          for j, pose in enumerate(POSES) if size != (1280, 1024) or j < 3],
                "bankN": [((320, 240), [("gt", "twist", 1, 0), ("dense", "identity", 2, 1), ("gt", "behind", 3, 2)]),
                          ((640, 480), [("dense", "approach", 1, 1), ("gt", "leaves", 2, 2)]),
                          ((640, 480), [("dense" if j % 2 else "gt", POSES[j % 5], 1 + j % 3, j % 3) for j in range(5)]),
                          ((1280, 1024), [("dense" if j % 3 else "gt", POSES[j % 5], 1 + j % 3, j % 3) for j in range(16)])]}


class Oracle:
    """the oracle's side of the evaluation cases, each computed once: records, per-point terms, float64 sums"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.scenes, self.trackers, self.cache = {}, {}, {}

    def scene(self, size):
        if size not in self.scenes:
            self.scenes[size] = Scene(self.oracle, *size)
            self.trackers[size] = self.scenes[size].tracker()
        return self.scenes[size]

    def cloud(self, size, name):
        sc = self.scene(size)
        if name.startswith("bank:"):
            return sc.keyframe_cloud(name[5:], permute=False)[:2]
        return eval_clouds(sc)[name]

    def job(self, size, job):
        """(record, terms, sums, n) of one job; terms and sums are None when no point is in the image"""
        key = (size,) + tuple(job)
        if key not in self.cache:
            sc = self.scene(size)
            name, pose, fi, ai = job
            pos, cv = self.cloud(size, name)
            a, b = AFFINE[ai]
            self.cache[key] = evaluate_case(sc, self.trackers[size], pos, cv, sc.fo[fi], sc.poses()[pose], a, b) + (len(pos),)
        return self.cache[key]


def form_jobs(form):
    """(scene size, job, jobs in its batch) over a form's batches; the bank's jobs name their cloud "bank:<kind>" """
    if form in BANK_BATCHES:
        return [(size, ("bank:" + k, p, fi, ai), len(jobs)) for size, jobs in BANK_BATCHES[form] for (k, p, fi, ai) in jobs]
    return [(size, job, len(jobs)) for size, jobs in form_batches(form) for job in jobs]


def sums_with_keep(P, keep):
    """sums64's A, b, err, werr with an explicit set of kept points (a wrong tail)"""
    out = {}
    for k in ("A", "b", "err", "werr"):
        out[k] = (P[k].astype(np.float64) * keep).sum(axis=-1)
    out["b"] = -out["b"]
    return out


def column_order_tail(sc, pos_in_image, M):
    """the keep mask of a kernel that drops the M % 4 in-image points with the largest COLUMN-ORDER pixel key (x h4 + y of the point's own
    level-4 pixel: the order of a keyframe's grid) instead of the last M % 4 of the list"""
    fx, fy, cx, cy = [float(v) for v in sc.intr[:4]]
    p = pos_in_image.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.floor(p[:, 0] / p[:, 2] * fx + cx + 0.5)
        y = np.floor(p[:, 1] / p[:, 2] * fy + cy + 0.5)
    key = np.nan_to_num(x * sc.h4 + y, nan=-1.0, posinf=1e9, neginf=-1e9)
    keep = np.ones(M, bool)
    if M % 4:
        keep[np.argsort(key, kind="stable")[-(M % 4):]] = False
    return keep


def evaluate_case(sc, tro, pos, cv, fo, T7, a, b):
    """the oracle's record, per-point terms and float64 sums of one evaluation; None for the sums when nothing is in the image"""
    from se3_terms import point_terms
    r = tro.evaluate_points(pos, cv, fo, T7, LEVEL, a, b)
    if r.warped_size == 0:
        return r, None, None
    P = point_terms(tro, fo, LEVEL, T7)
    return r, P, sums64(P)


def in_image_eval(sc, pos, T7, loose=None):
    """the evaluation's in-image mask of a list at the float32 pose T7 (taken as it is)"""
    _, _, _, u, v = project(pos, np.asarray(T7[:4], f32), np.asarray(T7[4:7], f32), sc.intr)
    return inside(u, v, sc.w4, sc.h4, 1, 2, loose)


# ---- the LM loop's cases ---------------------------------------------------------------------------------------------------------------------
DEFAULT_SETTINGS = dict(lambdaInitial=0.0, stepSizeMin=1e-3, convergenceEps=0.98, maxIts=5)


def loop_cases(sc):
    """(name, pos, colvar, frame index, referenceToFrame double[7], settings) of the 320x240 scene"""
    o = sc.oracle
    e = lambda a: o.se3_exp(np.array(a, np.float64))                              # noqa: E731
    near = e([0.01, 0.0, 0.0, 0, 0, 0.002])
    gtpose = lambda i: o.se3_inv(sc.gt[i])                                       # noqa: E731
    kf = sc.keyframe_cloud("gt")[:2]
    kfo = sc.keyframe_cloud("gt", permute=False)[:2]
    dense = sc.keyframe_cloud("dense")[:2]
    D = DEFAULT_SETTINGS
    S = lambda **kw: dict(D, **kw)                                               # noqa: E731
    cases = [
        ("kf-gt near", kf, 3, near, D),
        ("kf-gt in order identity", kfo, 1, e([0, 0, 0, 0, 0, 0]), D),
        ("kf-gt at the true pose", kf, 2, gtpose(2), D),
        ("kf-gt twenty iterations", kf, 3, near, S(maxIts=20, convergenceEps=0.9999)),
        ("kf-gt one iteration", kf, 3, near, S(maxIts=1)),
        ("kf-gt two iterations, tight eps", kf, 3, e([0.03, -0.02, 0.0, 0, 0.01, 0.0]), S(maxIts=2, convergenceEps=0.99999)),
        ("kf-gt large lambda", kf, 3, near, S(lambdaInitial=5.0, maxIts=8)),
        ("kf-gt loose eps", kf, 2, e([0.02, 0.01, 0.0, 0, 0, 0.0]), S(convergenceEps=0.5)),
        ("kf-gt large step minimum", kf, 2, gtpose(2), S(stepSizeMin=10.0, maxIts=20, convergenceEps=0.999999)),
        ("kf-gt step minimum, from lambda 0", kf, 1, gtpose(1), S(stepSizeMin=1e-9, maxIts=30, convergenceEps=0.9999999)),
        ("kf-dense near", dense, 3, near, D),
        ("kf-dense far", dense, 3, e([0.08, -0.05, 0.03, 0.01, -0.02, 0.03]), S(maxIts=10)),
        ("syn255 near", sc.synthetic(255), 1, near, D),
        ("syn1064 near", sc.synthetic(1064), 1, near, S(maxIts=10)),
        ("syn4097 twist", sc.synthetic(4097), 2, e([0.02, -0.01, 0.01, 0.005, -0.01, 0.01]), D),
        ("syn4836 near", sc.synthetic(4836), 2, near, S(maxIts=8)),
        ("syn25000 near", sc.synthetic(25000), 1, near, D),
        ("crafted near", sc.crafted_cloud()[:2], 1, near, D),
        ("syn63 near", sc.synthetic(63), 1, near, D),
        ("syn5 diverges at once", sc.synthetic(5, seed=3), 1, e([0.9, 0.1, 0.0, 0.0, 0.35, 0.0]), D),
        ("kf-gt leaves the image", kf, 1, e([0.9, 0.1, 0.0, 0.0, 0.6, 0.0]), D),
        ("syn256 bright outliers", bad_colours(sc.synthetic(256), 0.7, 90.0), 1, near, D),
        ("syn257 few in the image", sc.synthetic(257), 1, e([0.55, 0.0, 0.0, 0.0, 0.3, 0.0]), D),
        # ten-odd points in the image: above the level's minimum of 0.01 x 20 x 15 = 3 warped points, below level 3's 12, and fewer good
        # points than 0.04 x 20 x 15 = 12
        ("syn65 behind the camera", sc.synthetic(65), 1, e([0.02, 0.01, -1.2, 0.0, 0.01, 0.0]), D),
        ("syn64 behind the camera", sc.synthetic(64), 2, e([0.02, 0.01, -1.2, 0.0, 0.01, 0.0]), D),
        ("syn63 behind the camera", sc.synthetic(63), 3, e([0.02, 0.01, -1.2, 0.0, 0.01, 0.0]), D),
        ("syn64 behind the camera, nearer", sc.synthetic(64), 1, e([0.0, 0.0, -1.0, 0.0, 0.0, 0.0]), D),
        ("syn255 bright outliers", bad_colours(sc.synthetic(255), 0.8, -90.0), 2, near, D),
        ("syn64 behind the camera, frame 1", sc.synthetic(64), 1, e([0.02, 0.01, -1.2, 0.0, 0.01, 0.0]), D),
        ("syn64 behind the camera, frame 3", sc.synthetic(64), 3, e([0.0, 0.01, -1.2, 0.0, 0.0, 0.0]), D),
        ("syn3 diverges at once", sc.synthetic(3), 2, e([0, 0, 0, 0, 0, 0]), D),
        ("kf-gt three damped iterations", kf, 3, near, S(lambdaInitial=5.0, maxIts=3, convergenceEps=0.99999)),
        # further cases per branch, so that no branch rests on two cases
        ("kf-gt loose eps, frame 3", kf, 3, near, S(convergenceEps=0.5)),
        ("kf-dense loose eps", dense, 2, e([0.02, 0.01, 0.0, 0, 0, 0.0]), S(convergenceEps=0.3)),
        ("kf-gt one iteration, frame 2", kf, 2, e([0.02, 0.01, 0.0, 0, 0, 0.0]), S(maxIts=1)),
        ("kf-dense two damped iterations", dense, 3, near, S(lambdaInitial=5.0, maxIts=2, convergenceEps=0.99999)),
        ("syn4 diverges at once", sc.synthetic(4), 1, e([0, 0, 0, 0, 0, 0]), D),
        ("syn1 diverges at once", sc.synthetic(1), 3, near, D),
        ("syn16 near", sc.synthetic(16), 1, near, D),
        ("syn18 near", sc.synthetic(18, seed=2), 2, near, D),
        ("syn20 identity", sc.synthetic(20, seed=4), 3, e([0, 0, 0, 0, 0, 0]), D),
        ("syn1064 bright outliers", bad_colours(sc.synthetic(1064), 0.8, 90.0), 3, near, D),
        ("kf-gt step minimum, frame 3", kf, 3, gtpose(3), S(stepSizeMin=1e-9, maxIts=30, convergenceEps=0.9999999)),
        ("kf-gt step minimum, frame 2", kf, 2, near, S(stepSizeMin=1e-9, maxIts=30, convergenceEps=0.9999999)),
        ("kf-dense in order near", sc.keyframe_cloud("dense", permute=False)[:2], 3, near, S(maxIts=10)),
        ("kf-gt in order twist", kfo, 2, e([0.03, -0.02, 0.01, 0.005, -0.01, 0.01]), D),
    ]
    return cases


# the loop cases whose list is a keyframe's own cloud in the keyframe's order: what a bank slot holds
BANK_KIND = {"kf-gt in order identity": "gt", "kf-gt in order twist": "gt", "kf-dense in order near": "dense"}


def loop_results(orc):
    """[(case, clear, m, least margin, (result SSE_EXACT_RCP, result SSE), (trace, trace))] of the 320x240 scene's loop cases, m taken
    with the evaluation test's relative weightedError bound for the case's list at its starting pose, in the form that tiles it deepest"""
    if "loops" in orc.cache:
        return orc.cache["loops"]
    sc = orc.scene((320, 240))
    out = []
    for case in loop_cases(sc):
        name, (pos, cv), fi, T0, st = case
        q, t = pose_cast_f32(T0)
        r, P, S = evaluate_case(sc, sc.tracker(), pos, cv, sc.fo[fi], np.concatenate([q, t]), 1.0, 0.0)
        rel = 0.0
        if S is not None and S["werr"] > 0:
            depth = max(depth_for(len(pos), jobs) for jobs in (1, 2, 16)) + 1
            rel = (depth + C_TERM["werr"]) * EPS * S["werr_abs"] / S["werr"]
        out.append((case,) + loop_margin(sc, case, rel, r.warped_size))
    orc.cache["loops"] = out
    return out


def bad_colours(cloud, fraction, offset):
    """the cloud with `fraction` of its colours moved by `offset`: isGood fails for them (more bad than good points)"""
    pos, cv = cloud
    cv = cv.copy()
    k = np.random.default_rng(3).uniform(size=len(cv)) < fraction
    cv[k, 0] += f32(offset)
    return pos, cv


MIN_GOODPERGOODBAD_PIXEL, MIN_GOODPERALL_PIXEL, MIN_GOODPERALL_PIXEL_ABSMIN = 0.5, 0.04, 0.01


def run_loop_oracle(sc, case, mode):
    name, (pos, cv), fi, T0, st = case
    tr = sc.tracker(mode)
    tr.set_testtrack(st["lambdaInitial"], st["stepSizeMin"], st["convergenceEps"], st["maxIts"])
    return tr.track_permaref(pos, cv, sc.fo[fi], T0, trace=True)


def rel_margin(a, b):
    """how far a is from b, relative to the larger"""
    a, b = float(a), float(b)
    if not (np.isfinite(a) and np.isfinite(b)):
        return 0.0
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def loop_margin(sc, case, werr_rel_bound, first_count=None):
    """(clear, m, least margin, results of the two oracle modes, traces).  A case is clear when every comparison — per traced trial
    error < lastErr, error / lastErr > convergenceEps or incdot > stepSizeMin, and the warped count against the level's minimum; the two
    trackingWasGood ratios at the end — keeps a relative margin m from its threshold.  The trace has a record per inner-loop trial and
    none for the first evaluation: first_count is that evaluation's warped count (from evaluate_points at the starting pose), held
    against the minimum like the trials' (a count is an integer the device must match exactly — tests/test_permaref_eval_gpu.py — so a
    case that diverges at once, with no trial and m from the weightedError bound alone, is clear unless the count sits on the minimum).
    m = max(10 x the largest relative difference of the trial errors between the oracle's SSE_EXACT_RCP and SSE modes over the trials on which their decisions agree, 10 x the relative weightedError bound of the
    evaluation test for this cloud)."""
    o = sc.oracle
    st = case[4]
    (ra, ta), (rb, tb) = run_loop_oracle(sc, case, o.SSE_EXACT_RCP), run_loop_oracle(sc, case, o.SSE)
    diff = 0.0
    for x, y in zip(ta, tb):
        if x["branch"] != y["branch"]:
            break
        if x["branch"] != o.DIVERGED:
            diff = max(diff, rel_margin(x["error"], y["error"]), rel_margin(x["lastErr"], y["lastErr"]))
    m = max(10 * diff, 10 * werr_rel_bound)
    least = np.inf
    for x in ta:
        if x["branch"] == o.DIVERGED:
            continue
        least = min(least, rel_margin(x["error"], x["lastErr"]))
        if x["branch"] in (o.ACCEPTED, o.ACCEPTED_CONVERGED):
            least = min(least, rel_margin(x["error"] / x["lastErr"], st["convergenceEps"]))
        else:
            least = min(least, rel_margin(x["incdot"], st["stepSizeMin"]))
    if not ra.diverged:
        g, b = float(ra.lastGoodCount), float(ra.lastBadCount)
        least = min(least, rel_margin(g / (sc.w4 * sc.h4), MIN_GOODPERALL_PIXEL), rel_margin(g / (g + b), MIN_GOODPERGOODBAD_PIXEL))
    minWarped = MIN_GOODPERALL_PIXEL_ABSMIN * sc.w4 * sc.h4
    for count in ([] if first_count is None else [first_count]) + [x["buf_warped_size"] for x in ta]:
        least = min(least, rel_margin(count, minWarped))
    same = (len(ta) == len(tb) and np.array_equal(ta["branch"], tb["branch"]) and ra.diverged == rb.diverged
            and ra.trackingWasGood == rb.trackingWasGood)
    clear = bool(same and least > m)
    return clear, m, least, (ra, rb), (ta, tb)
