#!/usr/bin/env python
"""The re-activating keyframe change, fused against split, in one build and one process.

  fused   lsdhip_depth_reactivate_keyframe_batch(n maps): three launches for all maps, no host wait on an asynchronous context
  split   per map lsdhip_depth_finalize + lsdhip_depth_set_from_existing: the launches of the two single calls, the second of which
          ends in a stream synchronisation

n maps of 640 x 480 stand on keyframe B with keyframe A banked (finalised once); a call takes all of them back to A, the next one back to
B, and so on — every call finalises the keyframe the maps stand on and restores the other from its re-activation planes, so both arms do
the same work on the same kind of data call after call.  Per arm and n: WARMUP calls, then REGIONS regions of CALLS calls; a region's
host time is the wall time of its calls (the time the calling thread is held), its GPU time the span between two events on the mapping
stream around the region.  Regions of the two arms alternate; the median over a leg's regions is reported with its extremes.
Usage: tools/bench_reactivate.py [--ns 1,8,32] [--regions 7] [--calls 10] [--md out.md]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsd_slam_amd as la  # noqa: E402
from lsd_slam_amd import synth  # noqa: E402

W, H = 640, 480
WARMUP = 4
IDENT7 = np.array([1.0, 0, 0, 0, 0, 0, 0])
ITS = [5, 20, 50, 100, 0]


def build_maps(ctx, n, frames, depth0):
    """n maps on keyframe B (frame 3) with two updates on it, keyframe A (frame 0) finalised after two updates"""
    tr = la.SE3Tracker(ctx)
    tr.set_maxItsPerLvl(ITS)
    maps, A, B, keep = [], [], [], []
    for s in range(n):
        kf = la.Frame(ctx, 100 * s, frames[0])
        kf.setDepthFromGroundTruth(depth0)
        dm = la.DepthMap(ctx)
        dm.initializeFromGTDepth(kf)
        ref = la.TrackingReference()
        ref.importFrame(kf)
        pose = IDENT7.copy()
        cur = kf
        for t in range(1, 6):
            fr = la.Frame(ctx, 100 * s + t, frames[t])
            pose = tr.trackFrame(ref, fr, pose)
            if t == 3:
                dm.finalizeKeyFrame()
                dm.createKeyFrame(fr)
                cur, pose = fr, IDENT7.copy()
            else:
                dm.updateKeyframe([fr])
            keep.append(fr)
            ref.importFrame(cur)
            cur.clearDepthHasBeenUpdatedFlag()
        maps.append(dm)
        A.append(kf)
        B.append(cur)
    return maps, A, B, keep


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1,8,32")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    frames, depth0, K, _ = synth.make_sequence(W, H, 6, 0, "S1")
    rows = []
    for n in [int(v) for v in a.ns.split(",")]:
        ctx = la.Context(W, H, K)
        ctx.set_async(True)
        maps, A, B, keep = build_maps(ctx, n, frames, depth0)
        stream = torch.cuda.ExternalStream(ctx.stream())
        target = [A, B]
        state = {"k": 0}

        def fused():
            la.DepthMap.reactivateKeyframeBatch(maps, target[state["k"] % 2])
            state["k"] += 1

        def split():
            olds = target[state["k"] % 2]
            for dm, old in zip(maps, olds):
                dm.finalizeKeyFrame()
                dm.setFromExistingKF(old)
            state["k"] += 1

        legs = {"fused": fused, "split": split}
        host = {k: [] for k in legs}
        gpu = {k: [] for k in legs}
        for name, fn in legs.items():
            for _ in range(WARMUP):
                fn()
        ctx.synchronize()
        for r in range(a.regions):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ctx.synchronize()
                e0.record(stream)
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                t1 = time.perf_counter()
                e1.record(stream)
                e1.synchronize()
                host[name].append((t1 - t0) * 1e3 / a.calls)
                gpu[name].append(e0.elapsed_time(e1) / a.calls)
        row = {"n": n}
        for name in legs:
            hs, gs = sorted(host[name]), sorted(gpu[name])
            row[name] = {"host_ms": round(statistics.median(hs), 4), "host_min": round(hs[0], 4), "host_max": round(hs[-1], 4),
                         "gpu_ms": round(statistics.median(gs), 4), "gpu_min": round(gs[0], 4), "gpu_max": round(gs[-1], 4)}
        rows.append(row)
        del maps, A, B, keep
        ctx.close()
    md = ["| n maps | fused host ms/call | split host ms/call | fused GPU ms/call | split GPU ms/call | GPU ratio split / fused |", "|---|---|---|---|---|---|"]
    for r in rows:
        f, s = r["fused"], r["split"]
        md.append("| %d | %.3f (%.3f – %.3f) | %.3f (%.3f – %.3f) | %.3f (%.3f – %.3f) | %.3f (%.3f – %.3f) | %.2f |"
                  % (r["n"], f["host_ms"], f["host_min"], f["host_max"], s["host_ms"], s["host_min"], s["host_max"],
                     f["gpu_ms"], f["gpu_min"], f["gpu_max"], s["gpu_ms"], s["gpu_min"], s["gpu_max"], s["gpu_ms"] / f["gpu_ms"]))
    print("\n".join(md))
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("\n".join(md) + "\n")
    print(json.dumps({"rows": rows, "regions": a.regions, "calls": a.calls, "size": [W, H]}))


if __name__ == "__main__":
    main()
