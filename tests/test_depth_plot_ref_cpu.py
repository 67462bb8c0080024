"""tests/depth_plot_ref.py (the numpy restatement the device's debug image is held to) against three yardsticks, without a GPU:
the reference's own compiled DepthMapPixelHypothesis::getVisualizationColor (oracle/_ref, called through ctypes), a committed fixture of
that function's output, and plotDepthMap of include/lsd_slam_hip_io.hpp on whole images (a small program built with plain g++ -O1).
Every comparison is == on the bytes.  Also the condition on the inputs of modes 3 / 4 that lets the GPU test ask for equality."""
import os
import subprocess

import numpy as np
import pytest

import depth_plot_ref as dp
from common import ROOT, synth
from lsd_slam_amd.capi import HYP_DTYPE

ALL_MODES = dp.MODES + (dp.WHITE_MODE,)
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_plot_colors.npz")
CPU_SIZES = [(48, 32), (176, 144)]

_IMG = {}


def image_of(w, h):
    if (w, h) not in _IMG:
        _IMG[(w, h)] = synth.make_sequence(w, h, 1)[0][0].astype(np.float32)
    return _IMG[(w, h)]


def map_seed(w, h):
    return w * 1000 + h


@pytest.fixture(scope="module")
def ref_lib(oracle):
    if not oracle.have_ref() and not oracle.build_ref():
        pytest.skip("oracle/_ref not available (it is built from the reference sources, which are not here)")
    oracle.build_ref()          # rebuild if the stand-in headers changed
    return os.path.join(oracle.REF_DIR, "liblsd_ref_sse.so")


@pytest.mark.parametrize("last_frame_id", [0, 1234])
def test_restatement_equals_the_compiled_reference_function(ref_lib, last_frame_id):
    n = 100000 if last_frame_id == 0 else 110000
    hyp = dp.random_hypotheses(n, 7 + last_frame_id, last_frame_id)
    # the inputs cover what they claim to
    assert (hyp["idepth"] < 0).sum() > 1000 and (hyp["validity_counter"] < 0).sum() > 100 and (hyp["validity_counter"] > 255).sum() > 1000
    frac = hyp["nextStereoFrameMinID"] != np.rint(hyp["nextStereoFrameMinID"])
    assert frac.sum() > n // 4 and (~frac).sum() > n // 4
    for v in dp.PLANTED_IDEPTH:
        assert (hyp["idepth"].view(np.uint32) == np.float32(v).view(np.uint32)).any()
    for v in dp.PLANTED_VAR:
        assert (hyp["idepth_var"] == np.float32(v)).any() and (hyp["idepth_var_smoothed"] == np.float32(v)).any()
    for mode in ALL_MODES:
        got = dp.color_ref(hyp, mode, last_frame_id)
        want = dp.reference_colors(ref_lib, hyp, mode, last_frame_id)
        ne = np.flatnonzero((got != want).any(axis=1))
        assert len(ne) == 0, "mode %d: %d of %d colours differ, first %r: %r vs %r" % (mode, len(ne), n, hyp[ne[0]], got[ne[0]], want[ne[0]])
    # the planted variance of exactly 1 takes the logarithm of exactly 0
    one = hyp[hyp["idepth_var"] == np.float32(1.0)][:1]
    assert dp.color_ref(one, 4, last_frame_id).tolist() == [[255, 0, 0]]


def test_restatement_equals_the_committed_fixture():
    g = np.load(GOLDEN)
    hyp = np.ascontiguousarray(g["hypotheses"]).view(HYP_DTYPE).reshape(-1)
    assert 0 < len(hyp) <= 2048 and os.path.getsize(GOLDEN) < 150 * 1024
    assert g["colors"].shape == (len(dp.MODES), len(hyp), 3)
    last = int(g["last_frame_id"])
    for k, mode in enumerate(dp.MODES):
        assert np.array_equal(dp.color_ref(hyp, mode, last), g["colors"][k]), "mode %d" % mode
    assert len(np.unique(g["colors"].reshape(-1, 3), axis=0)) > 500      # (a fixture of one colour would pin nothing)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from lsd_slam_amd import build
    build.build()
    d = tmp_path_factory.mktemp("depthplot")
    out = str(d / "depth_plot_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "depth_plot_test.cpp"),
                           "-o", out, "-L" + os.path.join(ROOT, "lsd_slam_amd"), "-llsdhip", "-Wl,-rpath," + os.path.join(ROOT, "lsd_slam_amd")])
    return out


def read_ppm(path, w, h):
    raw = open(path, "rb").read()
    head = ("P6\n%d %d\n255\n" % (w, h)).encode()
    assert raw.startswith(head) and len(raw) == len(head) + w * h * 3
    return np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)


@pytest.mark.parametrize("size", CPU_SIZES)
def test_restatement_equals_the_header_on_whole_images(exe, tmp_path, size):
    w, h = size
    ref_id = 37
    m = dp.make_map(w, h, map_seed(w, h), last_frame_id=ref_id)
    image = image_of(w, h).copy()
    m["isValid"][0, :8] = 0
    image[0, :8] = [-3.0, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0, 127.49]         # ties go to the even byte, both ends saturate
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w, h, ref_id], np.int32).tobytes())
        f.write(m.tobytes())
        f.write(image.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out")])
    valid = m["isValid"] != 0
    assert 0.3 < valid.mean() < 0.4
    for mode in ALL_MODES:
        got = read_ppm(tmp_path / ("out.%d.ppm" % mode), w, h)
        want = dp.plot_ref(m, image, mode, ref_id)
        assert np.array_equal(got, want), "mode %d: %d pixels differ" % (mode, int((got != want).any(axis=2).sum()))
        grey = np.clip(np.rint(image), 0, 255).astype(np.uint8)
        if mode == 2:       # blacklisted pixels are painted whether valid or not; a valid one then takes its colour
            bl = m["blacklisted"] < dp.MIN_BLACKLIST
            assert (bl & ~valid).any() and (bl & valid).any() and (want[bl & ~valid] == (0, 0, 255)).all()
            assert (want[~valid & ~bl] == grey[~valid & ~bl][:, None]).all()
        else:
            assert (want[~valid] == grey[~valid][:, None]).all()
    assert dp.plot_ref(m, image, 0, ref_id)[0, :8, 0].tolist() == [0, 0, 2, 2, 254, 255, 255, 127]


def test_modes_3_and_4_do_not_depend_on_the_last_bits_of_the_logarithm():
    """The condition on the inputs (see depth_plot_ref.log_condition_holds) for the maps of this file and for every map of
    test_depth_plot_gpu.py.  If a seed ever fails it, change the seed, not the condition."""
    for w, h in CPU_SIZES:
        assert dp.log_condition_holds(dp.make_map(w, h, map_seed(w, h)), image_of(w, h)), (w, h)
    for w, h in dp.GPU_SIZES:
        assert dp.log_condition_holds(dp.gpu_map(w, h), image_of(w, h)), (w, h)
    w, h = dp.GPU_BATCH_SIZE
    for k in range(dp.GPU_BATCH_MAPS):
        assert dp.log_condition_holds(dp.gpu_map(w, h, k), image_of(w, h)), (w, h, k)
