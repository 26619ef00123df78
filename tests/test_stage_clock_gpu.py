"""The frame step's half of the stage clock (csrc/host_util.hpp StageClock, owned by dms_fusion): launches counted per stage name
through dms_fusion_get_kernel_time with profiling on.  The tracker's half is pinned by tests/test_tracking_gpu.py."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_stage_launches.json")

# every name a StageTimer of fusion_frame.hip carries
STAGES = ("ingest", "preprocess", "live_pyramids", "initialise", "predict", "fill_in", "odom_init", "track", "predict_old", "loop_init",
          "loop_track", "nid", "index_map", "fuse", "synth_depth", "clean", "global_loop")
FRAMES = 5
SIZES = [(40, 40), (77, 47)]  # the frame step's minimum and a ragged size (test_process_frame_ragged_resolutions)
# the default frame, and one that also runs the local-loop block, the NID gate and the separate fill-in launch
OPTIONS = {"default": {}, "loops": dict(local_loop_closure=1, nid_keyframing=1, fused_fill_in=0)}


@pytest.fixture(scope="module")
def fus():
    from densemonoslam_amd import capi, fusion

    assert capi.device_count() >= 1, "no MI355X visible"
    return fusion


@pytest.fixture(scope="module")
def synth():
    from densemonoslam_amd import synth as s

    return s


def launches(g):
    return {name: g.kernel_time(name)[1] for name in STAGES}


def run_profiled(fus, synth, size, frames, opts):
    """`frames` free-running frames with profiling on: (context, launches per stage, tracked frames that fused)"""
    Wr, Hr = size
    Kr = (0.825 * Wr, 0.825 * Wr, Wr / 2.0 - 0.25, Hr / 2.0 + 0.25)
    g = fus.ElasticFusion(Wr, Hr, Kr, model_capacity=600000, **opts)
    g.set_profiling(True)
    fused = 0
    for k in range(frames):
        d, rgb, _ = synth.frame(k, width=Wr, height=Hr, K=Kr, noise=True)
        r = g.processFrame(rgb, d)
        if k > 0:
            fused += int(bool(r.fused))
    return g, launches(g), fused


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("form", sorted(OPTIONS))
def test_frame_step_stage_launches(fus, synth, size, form):
    g, got, fused = run_profiled(fus, synth, size, FRAMES, OPTIONS[form])
    print("%dx%d %s: %d tracked frames fused, launches %s" % (size[0], size[1], form, fused, json.dumps(got, sort_keys=True)))
    # what the code enqueues: one bootstrap, the live half once per frame, two index maps around every fuse, one clean per fuse,
    # a tracking and a final prediction per tracked frame and a final one for the bootstrap frame
    assert got["initialise"] == 1
    assert got["ingest"] == got["preprocess"] == FRAMES
    assert got["fuse"] == got["clean"] == fused
    assert got["index_map"] == 2 * got["fuse"]
    assert got["predict"] >= FRAMES
    # the same run on the library built from the commit before the clocks were merged
    with open(GOLDEN) as f:
        want = json.load(f)["%dx%d %s" % (size[0], size[1], form)]
    assert got == want
    # a second context keeps a clock of its own
    g2, got2, _ = run_profiled(fus, synth, size, 2, OPTIONS[form])
    assert got2["ingest"] == got2["preprocess"] == 2 and got2["initialise"] == 1
    assert launches(g) == got
    assert g.kernel_time("host_wait")[1] == FRAMES and g2.kernel_time("host_wait")[1] == 2
    g2.close()
    g.close()
