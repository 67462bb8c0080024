"""Row-band decomposition on the GPU: N windows on one MI355X (LocalComm) reproduce the full-frame HIP regulariser and
the full-frame oracle bit for bit over several passes (BASELINE.json configs[4] arithmetic at a test-sized map)."""
import numpy as np
import pytest

from lsd_slam_amd.bands import BandPlan, BandRegularizer, HipBandEngine, LocalComm, synth_s3

pytestmark = pytest.mark.gpu


def _rows_equal(got, ref, what):
    for k in ("isValid", "blacklisted", "validity_counter"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    v = ref["isValid"] > 0
    for k in ("idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed"):
        assert np.array_equal(got[k][v].view(np.uint32), ref[k][v].view(np.uint32)), (what, k)


@pytest.mark.parametrize("world", [2, 4])
def test_banded_hip_equals_full_frame_hip_and_oracle(oracle, world):
    from band_engines import OracleBandEngine
    w, H, passes = 320, 256, 3
    hyp, maxgrad = synth_s3(w, H)
    full = HipBandEngine(w, H)
    full.load(hyp, maxgrad)
    orc = OracleBandEngine(w, H)
    orc.load(hyp, maxgrad)
    for _ in range(passes):
        full.run_pass()
        orc.run_pass()
    ref = full.get()
    _rows_equal(ref, orc.get(), "full-frame HIP vs oracle")
    plan = BandPlan(H, world)
    engines = [HipBandEngine(w, plan.window_rows) for _ in range(world)]
    br = BandRegularizer(plan, engines, LocalComm(), list(range(world)))
    br.load(hyp, maxgrad)
    br.run(passes)
    for r, rows in br.owned_rows().items():
        y0, y1 = plan.owned[r]
        _rows_equal(rows, ref[y0:y1], "band %d of %d" % (r, world))


def test_full_size_3840x2160_hip_vs_oracle_and_8_bands(oracle):
    """BASELINE.json configs[4] at its real size: two fill-holes + regularise passes over the 3840x2160 scene-S3 map, full
    frame HIP vs full-frame oracle, then 8 row bands (LocalComm on one GPU) vs the full frame — all bit-exact."""
    from band_engines import OracleBandEngine
    w, H, passes = 3840, 2160, 2
    hyp, maxgrad = synth_s3(w, H)
    full = HipBandEngine(w, H)
    full.load(hyp, maxgrad)
    orc = OracleBandEngine(w, H)
    orc.load(hyp, maxgrad)
    for _ in range(passes):
        full.run_pass()
        orc.run_pass()
    ref = full.get()
    _rows_equal(ref, orc.get(), "3840x2160 full-frame HIP vs oracle")
    assert int((ref["isValid"] > 0).sum()) > 1_000_000
    del orc
    world = 8
    plan = BandPlan(H, world)
    engines = [HipBandEngine(w, plan.window_rows) for _ in range(world)]
    br = BandRegularizer(plan, engines, LocalComm(), list(range(world)))
    br.load(hyp, maxgrad)
    br.run(passes)
    for r, rows in br.owned_rows().items():
        y0, y1 = plan.owned[r]
        _rows_equal(rows, ref[y0:y1], "3840x2160 band %d of %d" % (r, world))


@pytest.mark.parametrize("world", [2, 5, 8])
def test_native_band_loop_equals_full_frame(world):
    """The C++ loop (liblsdhip_driver.so lsdband_*): same decomposition, everything queued on the context's stream, one map -> map
    copy launch per exchange — bit-exact against the full-frame HIP pass after several passes."""
    from lsd_slam_amd.bands import NativeBandRegularizer
    w, H, passes = 320, 256 if world < 8 else 384, 4
    hyp, maxgrad = synth_s3(w, H)
    full = HipBandEngine(w, H)
    full.load(hyp, maxgrad)
    for _ in range(passes):
        full.run_pass()
    ref = full.get()
    nb = NativeBandRegularizer(w, H, world, list(range(world)))
    nb.load(hyp, maxgrad)
    # two calls, split after the first pass (far from the regulariser's fixed point): the second call starts with the halo refresh
    nb.run(1)
    nb.run(passes - 1)
    assert nb.halo_bytes_per_pass() == nb.plan.halo_bytes_per_pass(w)
    for r, rows in nb.owned_rows().items():
        y0, y1 = nb.plan.owned[r]
        _rows_equal(rows, ref[y0:y1], "native band %d of %d" % (r, world))
    nb.close()


@pytest.mark.parametrize("world", [3, 8])
def test_native_band_loop_packed_wire_format(world):
    """The multi-GPU exchange without the wire: rows are packed (29 B per pixel, plane after plane), copied buffer to buffer in
    place of ncclSend / ncclRecv, and unpacked — everything of the RCCL path except the two RCCL calls (RCCL refuses two ranks on
    the one GPU of this box; the 8-GPU run is the driver's).  Bit-exact against the full frame."""
    from lsd_slam_amd.bands import NativeBandRegularizer
    w, H, passes = 320, 384, 3
    hyp, maxgrad = synth_s3(w, H)
    full = HipBandEngine(w, H)
    full.load(hyp, maxgrad)
    for _ in range(passes):
        full.run_pass()
    ref = full.get()
    nb = NativeBandRegularizer(w, H, world, list(range(world)))
    nb.set_packed_exchange(True)
    nb.load(hyp, maxgrad)
    nb.run(passes)
    for r, rows in nb.owned_rows().items():
        y0, y1 = nb.plan.owned[r]
        _rows_equal(rows, ref[y0:y1], "packed band %d of %d" % (r, world))
    nb.close()


@pytest.mark.parametrize("bands,overlap", [(2, 1), (8, 1), (8, 0)])
def test_native_band_loop_two_processes_over_ipc(tmp_path, bands, overlap):
    """The multi-process wire path of the C++ band loop, executed: TWO processes on this one GPU (RCCL refuses two ranks on one
    device, so the loop's second transport carries the rows: IPC-mapped mailboxes, pack straight into the peer's buffer, ready /
    consumed flags on the stream — the same pack -> transfer -> unpack schedule per pass as the RCCL path), 2 x 1 and 2 x 4 bands,
    several passes over two lsdband_run calls.  overlap = 1 (the default): every pass is issued as edge tile rows + interior tile rows
    and the exchange runs on the transport stream under the interior part; 0: exchange after the pass on one stream.  Owned rows of
    both processes == the full-frame result, bit for bit."""
    import json, os, socket, subprocess, sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = tmp_path / "ipc.json"
    env = dict(os.environ)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "band_ipc_worker.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           worker, "640", "512", str(bands), "4", str(out), str(overlap)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.load(open(out))
    assert res["ok"] and res["flag_waits_failed"] == [0, 0] and res["valid"] > 10000, res


def test_native_band_loop_one_launch_of_32x16_tiles_1024x512():
    """1024x512 in two bands with the exchange after the pass (set_overlap(False)): the parts of a pass go into ONE k_reg_rows_batch launch,
    and 32 tile columns x at least 64 tile rows in all = 2048 workgroups of 32x8 pixels is where lsd_reg_py takes the 32x16 tile
    (k_reg_rows_batch<2>; every other shape of this file stays below it).  Bit-exact against the full-frame pass."""
    from lsd_slam_amd.bands import NativeBandRegularizer
    w, H, world, passes = 1024, 512, 2, 2
    assert ((w + 31) // 32) * (H // 8) >= 2048
    hyp, maxgrad = synth_s3(w, H)
    full = HipBandEngine(w, H)
    full.load(hyp, maxgrad)
    for _ in range(passes):
        full.run_pass()
    ref = full.get()
    assert int((ref["isValid"] > 0).sum()) > 50_000
    nb = NativeBandRegularizer(w, H, world, list(range(world)))
    nb.set_overlap(False)
    nb.load(hyp, maxgrad)
    nb.run(passes)
    for r, rows in nb.owned_rows().items():
        y0, y1 = nb.plan.owned[r]
        _rows_equal(rows, ref[y0:y1], "1024x512 band %d of %d" % (r, world))
    nb.close()
