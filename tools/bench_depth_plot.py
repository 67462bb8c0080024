"""Times the depth map's debug image at 640x480 on a map of a synth sequence (recorded, not gated):
  (a) today's path without the device plot: lsdhip_depth_download (32 bytes per pixel to the host and a wait for the mapping stream) +
      plotDepthMap on the host, in C++ — tools/bench_depth_plot_host.cpp, built by this tool with g++ -O2 next to it
      (tools/bench_depth_plot_host.bin) and run on the same frames; host wall time;
  (b) the device plot of one map: HIP events on the mapping stream around REPS queued launches, and the host wall time of the queued call;
  (c) 32 maps in one launch (lsdhip_depth_debug_plot_batch): HIP events;
  (d) the host-output call (launch + copy of 3 bytes per pixel + wait): host wall time.
Median of REGIONS regions, per mode.  Algorithmic bytes per pixel: 5 + 4 * planes read, 3 written.  The event
brackets hold REPS queued calls each, so (b) is the time per queued call (argument copy + launch), not the kernel's own duration: for that,
run this tool under rocprofv3 --kernel-trace.  Back-to-back launches re-read the same planes: the bytes of (b) come from L2, those of (c) —
32 maps, 118 MB per launch — from the Infinity Cache, not from HBM (profiles/r07_depth_plot.md).  Prints one JSON object."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PLANES = {0: 1, 1: 1, 2: 2, 3: 1, 4: 1, 5: 1}


def main():
    import torch
    import lsd_slam_amd as la
    from lsd_slam_amd import synth
    from lsd_slam_amd.capi import check
    w, h, REGIONS, REPS, NB = 640, 480, 7, 50, 32
    frames, depth0, K, gt = synth.make_sequence(w, h, 12)
    ctx = la.Context(w, h, K)
    kf = la.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    dm = la.DepthMap(ctx)
    dm.initializeFromGTDepth(kf)
    tracker, ref = la.SE3Tracker(ctx), la.TrackingReference()
    ref.importFrame(kf)
    tracker.set_maxItsPerLvl([5, 20, 50, 100, 0])
    for i in range(1, 11):
        f = la.Frame(ctx, i, frames[i])
        tracker.trackFrame(ref, f, la.IDENTITY)
        dm.updateKeyframe([f])
    hyp = dm.currentDepthMap()
    stream = torch.cuda.ExternalStream(ctx.L.lsdhip_ctx_map_stream(ctx.h_))
    res = {"size": [w, h], "regions": REGIONS, "reps": REPS, "device": torch.cuda.get_device_name(0),
           "valid_fraction": float((hyp["isValid"] != 0).mean())}

    def alloc(n):
        out = []
        for _ in range(n):
            p = ctypes.c_void_p()
            check(ctx.L.lsdhip_ctx_alloc_dev(ctx.h_, 3 * w * h, ctypes.byref(p)), False)
            out.append(p.value)
        return out

    def events(fn, reps):
        out = []
        for _ in range(REGIONS):
            ctx.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(reps):
                fn()
            b.record(stream)
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e-3 / reps)
        return float(np.median(out)), float(min(out)), float(max(out))

    # (a) + the host clock of the device plot, in C++ on the same sequence
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, src = os.path.join(root, "tools", "bench_depth_plot_host.bin"), os.path.join(root, "tools", "bench_depth_plot_host.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe, "-L" + os.path.join(root, "lsd_slam_amd"), "-llsdhip",
                               "-Wl,-rpath,$ORIGIN/../lsd_slam_amd"])
    with tempfile.NamedTemporaryFile(suffix=".bin") as tf:
        tf.write(np.array([w, h, 11], np.int32).tobytes())
        tf.write(np.asarray(K, np.float32).tobytes())
        tf.write(np.ascontiguousarray(depth0, np.float32).tobytes())
        tf.write(np.ascontiguousarray(frames[:11]).tobytes())
        tf.flush()
        res["a_cpp"] = {m: json.loads(subprocess.check_output([exe, tf.name, str(REGIONS), "10", str(m)], timeout=200).decode()) for m in (0, 3)}

    # the other maps of the batch: copies of this one's hypotheses on keyframes of their own (distinct memory: 32 maps do not fit one L2)
    others = []
    for k in range(NB - 1):
        kfk = la.Frame(ctx, 100 + k, frames[0])
        dmk = la.DepthMap(ctx)
        dmk.setCurrentDepthMap(kfk, hyp)
        others.append((dmk, kfk))
    maps = [dm] + [o[0] for o in others]
    bufs = alloc(NB)
    ctx.synchronize()
    per_mode = {}
    for mode in range(7):
        planes = PLANES.get(mode, 0)
        nbytes = (5 + 4 * planes + 3) * w * h
        for _ in range(3):      # warm-up: code object, argument ring
            dm.debugPlotDepthMap(mode, out_dev_ptr=bufs[0])
            la.DepthMap.debugPlotDepthMapBatch(maps, bufs, mode)
        g1 = events(lambda: dm.debugPlotDepthMap(mode, out_dev_ptr=bufs[0]), REPS)
        g32 = events(lambda: la.DepthMap.debugPlotDepthMapBatch(maps, bufs, mode), 10)
        wall = []
        for _ in range(REGIONS):
            for _ in range(REPS):
                t0 = time.perf_counter()
                dm.debugPlotDepthMap(mode, out_dev_ptr=bufs[0])
                wall.append(time.perf_counter() - t0)
            ctx.synchronize()
        sync = []
        for _ in range(REGIONS):
            t0 = time.perf_counter()
            for _ in range(10):
                dm.debugPlotDepthMap(mode)
            sync.append((time.perf_counter() - t0) / 10)
        per_mode[mode] = {"bytes": nbytes, "b_single_gpu_s": g1[0], "b_single_gpu_min_max_s": g1[1:], "b_queued_call_host_s": float(np.median(wall)),
                          "b_single_bytes_per_s": nbytes / g1[0], "c_batch32_gpu_s": g32[0], "c_batch32_gpu_min_max_s": g32[1:],
                          "c_bytes_per_s": NB * nbytes / g32[0],
                          "d_host_output_call_s": float(np.median(sync))}
    res["modes"] = per_mode
    print(json.dumps(res))


if __name__ == "__main__":
    main()
