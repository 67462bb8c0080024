"""Writes tests/golden/depth_plot_colors.npz: 2048 hypotheses and the colours the reference's own compiled
DepthMapPixelHypothesis::getVisualizationColor (oracle/_ref/liblsd_ref_sse.so, built from the reference's DepthMapPixelHypothesis.cpp and
settings.cpp) gives them in debugDisplay modes 0 .. 5, called through tests/depth_plot_ref.reference_colors.  Recorded results only.
Run from the repository root where oracle/_ref exists:  python tests/golden/make_depth_plot_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import depth_plot_ref as dp  # noqa: E402
from oracle import pyoracle  # noqa: E402

LAST_FRAME_ID = 37
N = 2048

if __name__ == "__main__":
    assert pyoracle.have_ref() or pyoracle.build_ref(), "oracle/_ref is needed"
    lib = os.path.join(pyoracle.REF_DIR, "liblsd_ref_sse.so")
    hyp = dp.random_hypotheses(N, 20260, LAST_FRAME_ID)
    colors = np.stack([dp.reference_colors(lib, hyp, mode, LAST_FRAME_ID) for mode in dp.MODES])
    out = os.path.join(HERE, "depth_plot_colors.npz")
    np.savez_compressed(out, hypotheses=hyp.view(np.uint8).reshape(N, 32), colors=colors, last_frame_id=np.int32(LAST_FRAME_ID))
    print(out, os.path.getsize(out), "bytes")
