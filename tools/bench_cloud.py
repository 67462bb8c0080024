"""Times the keyframe export per keyframe at 640x480 on a finalised map of a synth sequence (recorded, not gated):
  (a) the existing host path: makeKeyframeMsg (its three plane downloads, each draining the context, and the fill loop) + flushPointCloud,
      in C++ — tools/bench_cloud_host.cpp, built by this tool with g++ -O2 next to it (tools/bench_cloud_host.bin) and run on the same frames;
  (b) PointCloud.appendKeyframe: HIP events on the mapping stream and host wall time of the call;
  (c) PointCloud.appendBatch of 32 keyframes;
  (d) Frame.keyframePoints (payload pack + copy), and the pack launch's share from HIP events.
Median of REGIONS regions.  Every timed append has room in its cloud, so the write pass does all its work; bytes per launch set from
DESIGN.md: payload 12 read + 12 written per pixel; append 12 read per pixel + 16 written per kept point.  Prints one JSON object."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK = 8.0e12      # bytes/s, MI355X


def main():
    import torch
    import lsd_slam_amd as la
    from lsd_slam_amd import synth
    w, h, REGIONS, REPS = 640, 480, 7, 20
    frames, depth0, K, gt = synth.make_sequence(w, h, 12)
    ctx = la.Context(w, h, K)
    kf = la.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    dm = la.DepthMap(ctx)
    dm.initializeFromGTDepth(kf)
    tracker, ref = la.SE3Tracker(ctx), la.TrackingReference()
    ref.importFrame(kf)
    for i in range(1, 11):
        f = la.Frame(ctx, i, frames[i])
        tracker.trackFrame(ref, f, la.IDENTITY)
        dm.updateKeyframe([f])
    dm.finalizeKeyFrame()
    pose = np.array([0.1, -0.2, 0.05, 0.97, 0.5, -1.0, 2.0], np.float32)
    stream = torch.cuda.ExternalStream(ctx.L.lsdhip_ctx_map_stream(ctx.h_))

    def med(fn):
        out = []
        for _ in range(REGIONS):
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            ctx.synchronize()
            out.append((time.perf_counter() - t0) / REPS)
        return float(np.median(out))

    res = {"size": [w, h], "regions": REGIONS, "reps": REPS, "device": torch.cuda.get_device_name(0)}
    # (a) the C++ host path on the same sequence
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, src = os.path.join(root, "tools", "bench_cloud_host.bin"), os.path.join(root, "tools", "bench_cloud_host.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe, "-L" + os.path.join(root, "lsd_slam_amd"), "-llsdhip",
                               "-Wl,-rpath,$ORIGIN/../lsd_slam_amd"])
    with tempfile.NamedTemporaryFile(suffix=".bin") as tf:
        tf.write(np.array([w, h, 11], np.int32).tobytes())
        tf.write(np.asarray(K, np.float32).tobytes())
        tf.write(np.ascontiguousarray(depth0, np.float32).tobytes())
        tf.write(np.ascontiguousarray(frames[:11]).tobytes())
        tf.flush()
        host = json.loads(subprocess.check_output([exe, tf.name, str(REGIONS), str(REPS)], timeout=100).decode())
    res["a_host_path_s"] = host["host_path_s"]
    res["a_makeKeyframeMsg_s"] = host["makeKeyframeMsg_s"]
    res["a_flushPointCloud_s"] = host["flushPointCloud_s"]
    res["a_kept_points"] = host["kept_points"]
    probe = la.PointCloud(ctx, w * h, 2)
    probe.appendKeyframe(kf, pose)
    kept = probe.total()
    probe.close()
    bytes_append = 12 * w * h + 16 * kept
    res["kept_points"] = kept
    res["b_bytes"] = bytes_append
    # (b) REPS appends per region into a cloud with room for all of them; the reset lies outside the bracket
    cloud = la.PointCloud(ctx, max(kept, 1) * REPS, REPS)

    def region(fn, reset, reps):
        out = []
        for _ in range(REGIONS):
            reset()
            ctx.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(reps):
                fn()
            b.record(stream)
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e-3 / reps)
        return float(np.median(out))

    res["b_append_gpu_s"] = region(lambda: cloud.appendKeyframe(kf, pose), cloud.reset, REPS)
    assert cloud.total() == cloud.stored() == kept * REPS          # nothing was dropped: the write pass did all its work
    wall = []
    for _ in range(REGIONS):
        cloud.reset()
        for _ in range(REPS):
            t0 = time.perf_counter()
            cloud.appendKeyframe(kf, pose)
            wall.append(time.perf_counter() - t0)
        ctx.synchronize()
    res["b_append_host_call_s"] = float(np.median(wall))
    res["b_fraction_of_hbm_peak"] = bytes_append / res["b_append_gpu_s"] / HBM_PEAK
    cloud.close()
    # (c) 32 keyframes per call, REPS_C calls per region, room for all of them
    REPS_C = 5
    clouds = [la.PointCloud(ctx, max(kept, 1) * REPS_C, REPS_C) for _ in range(32)]
    poses32 = np.tile(pose, (32, 1))
    res["c_batch32_gpu_s"] = region(lambda: la.PointCloud.appendBatch(clouds, [kf] * 32, poses32), lambda: [c.reset() for c in clouds], REPS_C)
    assert all(c.total() == c.stored() == kept * REPS_C for c in clouds)
    res["c_bytes"] = 32 * bytes_append
    res["c_fraction_of_hbm_peak"] = 32 * bytes_append / res["c_batch32_gpu_s"] / HBM_PEAK
    # (d) the payload: the synchronous call (launch + copy of 12 B/px to the host)
    res["d_payload_pack_and_copy_s"] = med(kf.keyframePoints)
    res["d_bytes_device"] = 24 * w * h
    res["d_bytes_copied"] = 12 * w * h
    print(json.dumps(res))


if __name__ == "__main__":
    main()
