"""Times the rectification of raw FOV-camera images at 752x480 -> 640x480 (the reference's FOV example calibration), recorded, not gated:
  (a) per frame, host wall time (tools/bench_undistort_host.cpp, built here with g++ -O3 as tools/bench_undistort_host.bin): the host
      gather Undistorter::undistort on one core followed by lsdhip_frame_create_async — what the library's users had to do before — against
      lsdhip_frame_create_undistorted_async of the raw bytes; every region ends with a context synchronise inside the timed window;
  (b) the pipelined lsd_slam_hip::SlamLoop (C++ driver loop, images resident on the device, keyframe every 10 frames) fed raw images
      against the same loop fed the pre-rectified images of the same frames: RUNS alternating runs of FRAMES frames each, wall time around
      lsdloop_run plus the final synchronise; reported per run, with the median and the spread.
  --loop-only raw|rect runs one loop of (b) and nothing else: the form to put under `rocprofv3 --kernel-trace --stats -- python
  tools/bench_undistort.py --loop-only raw` for the launch count (two frame-creation launches per frame either way).
The raw frames are the synth.py scene seen through the FOV camera (tests/undistort_ref.py raw_sequence); the loop's depth of frame 0 is
rendered at the rectified camera.  Prints one JSON object."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FOV = (0.527334, 0.827306, 0.473568, 0.499436, 0.928161)
IN, OUT = (752, 480), (640, 480)


def host_program():
    src, exe = os.path.join(ROOT, "tools", "bench_undistort_host.cpp"), os.path.join(ROOT, "tools", "bench_undistort_host.bin")
    deps = [src, os.path.join(ROOT, "include", "lsd_slam_hip_io.hpp"), os.path.join(ROOT, "include", "lsd_slam_hip.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        lib = os.path.join(ROOT, "lsd_slam_amd")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L" + lib, "-llsdhip", "-Wl,-rpath," + lib])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--loop-only", choices=["raw", "rect"])
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    exe = host_program()
    if a.build_only:
        return
    import torch
    import undistort_ref as ur
    from lsd_slam_amd import capi
    from lsd_slam_amd.driver import DriverLoop
    d = tempfile.mkdtemp()
    cfg = os.path.join(d, "fov.cfg")
    with open(cfg, "w") as f:
        f.write(ur.cfg_text(FOV, IN, "crop", OUT))
    res = {"device": torch.cuda.get_device_name(0), "in": list(IN), "out": list(OUT)}
    if not a.loop_only:
        res["per_frame"] = json.loads(subprocess.check_output([exe, cfg, str(a.regions), str(a.reps)]).decode())
    # (b) the loop
    cam = ur.cpp_tables(ur.compile_cpp(ROOT, d), os.path.join(d, "cam"), ur.cfg_text(FOV, IN, "crop", OUT), OUT)
    K = cam["K"].astype(np.float32)
    period = 50                                    # the synthetic camera closes its circle after 50 frames
    raws, depth0 = ur.raw_sequence(0, period, K, FOV, IN, OUT)
    rect = np.stack([ur.undistort_f32(r, cam["remapX"], cam["remapY"]) for r in raws])      # == Undistorter::undistort (tests/test_undistort_cpu.py)
    dev = {"raw": torch.from_numpy(raws).cuda(), "rect": torch.from_numpy(rect).cuda()}
    torch.cuda.synchronize()

    def run(kind):
        imgs = dev[kind]
        drv = DriverLoop(OUT[0], OUT[1], K, imgs[0].data_ptr(), depth0, kf_every=10, images_on_device=True,
                         undistort=(IN[0], IN[1], cam["remapX"], cam["remapY"]) if kind == "raw" else None)
        drv.set_pipeline(True)
        ptrs = [imgs[t % period].data_ptr() for t in range(1, a.frames + 1)]
        drv.run(ptrs[:20])                            # warm-up
        capi.check(capi.lib().lsdhip_ctx_synchronize(drv.ctx_handle()))
        t0 = time.perf_counter()
        done, _ = drv.run(ptrs[20:])
        capi.check(capi.lib().lsdhip_ctx_synchronize(drv.ctx_handle()))
        dt = time.perf_counter() - t0
        st = drv.stats()
        good = int(st.tracked_good)
        drv.close()
        return dt / done * 1e3, done, good

    if a.loop_only:
        ms, done, good = run(a.loop_only)
        res["loop"] = {"kind": a.loop_only, "frames": done, "tracked_good": good, "ms_per_frame": ms}
    else:
        out = {"raw": [], "rect": []}
        for _ in range(a.runs):
            for kind in ("rect", "raw"):
                ms, done, good = run(kind)
                out[kind].append(ms)
        res["loop"] = {"frames_per_run": a.frames - 20, "runs": a.runs, "tracked_good_last_run": good,
                       "rect_ms_per_frame": out["rect"], "raw_ms_per_frame": out["raw"],
                       "rect_median": float(np.median(out["rect"])), "raw_median": float(np.median(out["raw"])),
                       "rect_spread": [min(out["rect"]), max(out["rect"])], "raw_spread": [min(out["raw"]), max(out["raw"])]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
