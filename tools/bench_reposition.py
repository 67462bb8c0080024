#!/usr/bin/env python3
"""Wall time of one TrackableKeyFrameSearch::findRePositionCandidate (C/GlobalMapping/TrackableKeyFrameSearch.cpp:103-172) over K banked
640x480 keyframes that all pass the prefilter and the overlap score, i.e. K overlap checks and K permaref trackings per search:

  serial  what a caller had before the bank: per candidate lsdhip_tracker_check_overlap + lsdhip_tracker_track_permaref on host clouds
          (an upload and a wait each)
  batch   the K overlap checks as above, then the existing host-cloud batch entry lsdhip_tracker_track_permaref_batch (one upload of
          all clouds)
  bank    lsdhip_tracker_find_reposition_candidate: prefilter on the host, one overlap launch, one tracking batch, nothing uploaded but
          the job records

The legs run in alternating rounds in one process (serial, batch, bank, serial, ...), the median per leg is reported with the spread of
the rounds.  The bank leg's two device stages are also timed on their own (lsdhip_tracker_check_overlap_bank /
lsdhip_tracker_track_permaref_bank: wall time of the call, launch + wait).  Last line: the cost of banking a keyframe (lsdhip_kfbank_put)
against Frame::setPermaRef's host path (lsdhip_ref_pointcloud at level 4).

GPU time of the bank search's two launches: a kernel trace in a run of its own (tracing slows the host, so no wall time is taken from it),
with the bank leg alone so that every traced launch belongs to a search:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_reposition.py --legs bank --ks 32 --rounds 25
    python tools/bench_reposition.py --kernel-trace DIR --ks 32 --rounds 25
The second command reads the trace and prints, per search, the time inside k_overlap_bank and inside the tracking batch's k_track_step
launches (those that still had work and the empty ones of the launch budget behind the last job's finishing step), and the span from the
first tracking launch's start to the last one's end.

The keyframes are views 30 .. 42 of synth.Scene(0, "S1", radius=0.3) with their ground-truth depth, taken round robin; the query is view 41
at its ground-truth pose; five far fillers take the slots of the initialisation phase.  Usage: tools/bench_reposition.py [--rounds 25]
[--ks 1,8,32,128] [--legs serial,batch,bank,bank_overlap,bank_track] [--md out.md]"""
import argparse
import csv
import glob
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
VIEWS = (30, 33, 36, 39, 42)
QUERY = 41


def pose8(R, t, s=1.0):
    return np.concatenate([synth.rot_to_quat(R), t, [s]])


def med(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[0], xs[-1]


WARMUP_ROUNDS = 2     # allocations of the batch buffers, launch budgets


def kernel_trace_summary(directory, ks, rounds):
    """per search of a `--legs bank` run traced by rocprofv3: time inside the overlap launch and inside the tracking batch's launches"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % directory
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    searches, cur = [], None
    for r in rows:         # a search = one k_overlap_bank launch and the k_track_step launches up to the next one
        name, t0, t1 = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if "k_overlap_bank" in name:
            cur = {"overlap": (t1 - t0) / 1e3, "track": 0.0, "launches": 0, "first": None, "last": None}
            searches.append(cur)
        elif "k_track_step" in name and cur is not None:
            cur["track"] += (t1 - t0) / 1e3
            cur["launches"] += 1
            cur["first"] = t0 if cur["first"] is None else cur["first"]
            cur["last"] = t1
    per_k = 1 + WARMUP_ROUNDS + rounds       # the search that sets the leg up, the warm-up rounds, the timed rounds
    assert len(searches) == per_k * len(ks), (len(searches), per_k, ks)
    print("| K | k_overlap_bank us | tracking batch: sum of its k_track_step launches us | launches | first start to last end us |")
    print("|---|---|---|---|---|")
    for i, kk in enumerate(ks):
        timed = searches[i * per_k + 1 + WARMUP_ROUNDS:(i + 1) * per_k]
        print("| %d | %.1f | %.1f | %d | %.1f |" % (kk, statistics.median(x["overlap"] for x in timed), statistics.median(x["track"] for x in timed),
                                                 statistics.median(x["launches"] for x in timed), statistics.median((x["last"] - x["first"]) / 1e3 for x in timed)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--ks", default="1,8,32,128")
    ap.add_argument("--legs", default="serial,batch,bank,bank_overlap,bank_track")
    ap.add_argument("--kernel-trace", default=None, help="summarise a rocprofv3 kernel trace of a `--legs bank` run with the same --ks / --rounds")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(",")]
    if a.kernel_trace:
        return kernel_trace_summary(a.kernel_trace, ks, a.rounds)
    sc = synth.Scene(0, "S1", radius=0.3)
    K = synth.intrinsics(W, H)
    ctx = la.Context(W, H, K)
    views = {i: sc.render(i, W, H) + sc.cam_to_world(i) for i in VIEWS + (QUERY,)}
    frame = la.Frame(ctx, 1000, views[QUERY][0])
    framePose = pose8(views[QUERY][2], views[QUERY][3])
    rows, put_ms, ref_ms = [], [], []
    for kk in ks:
        bank = la.KeyFrameBank(ctx, kk + 5)
        kfs = []
        for j in range(kk + 5):
            i = VIEWS[j % len(VIEWS)]
            img, depth, R, C = views[i]
            f = la.Frame(ctx, j, img)
            f.setDepthFromGroundTruth(depth)
            ref = la.TrackingReference()
            ref.keyframe = f
            t0 = time.perf_counter()
            ref.makePointCloud(4)
            t1 = time.perf_counter()
            bank.put(f)
            t2 = time.perf_counter()
            ref_ms.append((t1 - t0) * 1e3)
            put_ms.append((t2 - t1) * 1e3)
            bank.setMeta(j, pose8(R, C + (np.array([50.0, 0, 0]) if j < 5 else 0.0)), 0.5)
            kfs.append(f)
        search = la.TrackableKeyFrameSearch(ctx, bank)
        assert search.findRePositionCandidate(frame, framePose, -1, 1.0) is not None
        r = search.last
        assert (r.numChecked, r.numTracked) == (kk, kk), (r.numChecked, r.numTracked)
        recs = search.records()[5:]
        slots = [x.slot for x in recs]
        poses = [list(x.refToFrame) for x in recs]
        clouds = [bank.download(s) for s in slots]
        tr = search.tracker

        def serial():
            for (pos, cv), T in zip(clouds, poses):
                tr.checkPermaRefOverlap(pos, T)
                tr.trackFrameOnPermaref(pos, cv, frame, T)

        def batch():
            for (pos, cv), T in zip(clouds, poses):
                tr.checkPermaRefOverlap(pos, T)
            tr.trackFrameOnPermarefBatch(clouds, [frame] * kk, poses)

        def banked():
            search.findRePositionCandidate(frame, framePose, -1, 1.0)

        def stage_overlap():
            tr.checkPermaRefOverlapBank(bank, slots, poses)

        def stage_track():
            tr.trackFrameOnPermarefBank(bank, slots, [frame] * kk, poses)

        legs = {"serial": serial, "batch": batch, "bank": banked, "bank_overlap": stage_overlap, "bank_track": stage_track}
        legs = {k: v for k, v in legs.items() if k in a.legs.split(",")}
        times = {k: [] for k in legs}
        for rnd in range(a.rounds + WARMUP_ROUNDS):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if rnd >= WARMUP_ROUNDS:
                    times[name].append(dt)
        row = {"K": kk}
        for name in legs:
            m, lo, hi = med(times[name])
            row[name + "_ms"], row[name + "_min"], row[name + "_max"] = round(m, 4), round(lo, 4), round(hi, 4)
        if "serial" in legs and "bank" in legs:
            row["serial_over_bank"] = round(row["serial_ms"] / row["bank_ms"], 2)
        rows.append(row)
        del search, kfs
        bank.close()
    out = {"rows": rows, "put_ms": round(statistics.median(put_ms), 4), "setPermaRef_host_ms": round(statistics.median(ref_ms), 4), "rounds": a.rounds}
    md = ["| K | serial ms (min - max) | batch ms | bank ms (min - max) | serial / bank | bank: overlap launch ms | bank: tracking batch ms |",
          "|---|---|---|---|---|---|---|"]
    for r in rows if set(a.legs.split(",")) >= {"serial", "batch", "bank", "bank_overlap", "bank_track"} else []:
        md.append("| %d | %.3f (%.3f - %.3f) | %.3f | %.3f (%.3f - %.3f) | %.2f | %.3f | %.3f |" % (
            r["K"], r["serial_ms"], r["serial_min"], r["serial_max"], r["batch_ms"], r["bank_ms"], r["bank_min"], r["bank_max"],
            r["serial_over_bank"], r["bank_overlap_ms"], r["bank_track_ms"]))
    md.append("")
    md.append("lsdhip_kfbank_put: %.3f ms per keyframe; Frame::setPermaRef's host path (lsdhip_ref_pointcloud, level 4): %.3f ms (medians over %d keyframes)"
              % (out["put_ms"], out["setPermaRef_host_ms"], len(put_ms)))
    print("\n".join(md))
    if a.md:
        with open(a.md, "w") as fh:
            fh.write("\n".join(md) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
