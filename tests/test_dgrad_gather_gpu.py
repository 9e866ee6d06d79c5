"""conv3's / conv2's data gradients in the f32 and f32x3 modes (csrc/learner_common.hip: ProbDgrad3, ProbDgrad2 on gemm_lds):
the transposed convolutions as gather-form GEMMs over the layer's input pixels, 64 rows per block; conv2's four parity
classes are the four N tiles of one launch, each over the 100 pixels per frame of its class.

Through rela_debug_trunk_backward on the integer data of tests/trunk_bwd_ref.py, exactly as tests/test_trunk_backward_gpu.py
runs it (preconditions asserted on the reference, NaN-initialised outputs, the launch census): all eight outputs EQUAL the
float64 reference, at the frame counts where the tiling can go wrong --
  64 frames: conv3's 81 * 64 rows are a whole number of tiles;  65: one frame more, the last tile is ragged
  16 frames: conv2's 100 * 16 rows per class fill their tiles exactly;  17: the last tile of every class is ragged, its
             surplus rows must neither load nor store
  1 frame: fewer rows than two tiles, a class ends inside its second tile (no frame count makes a class smaller than a
           tile of 64 rows)
Every term of the "dense" data set counts, so a dropped tap, a wrong border or a tile that reads another class's weights
shows.  The column-buffer form is gone: a call's timing labels must not contain learner_col2im."""
import ctypes as C
import json

import pytest

import trunk_bwd_ref as R
from test_trunk_backward_gpu import exact_case, expected_census, run_tap

pytestmark = pytest.mark.gpu

BM = 64  # csrc/learner_common.hip: TileDgrad3::BM and TileDgrad2::BM
FRAMES = (1, 16, 17, 64, 65)
assert (81 * 64) % BM == 0 and (100 * 16) % BM == 0
CASES = [(mode, lanes, n) for n in FRAMES for mode in ("f32", "f32x3") for lanes in (0, 1)]


@pytest.mark.parametrize("mode,lanes,frames", CASES, ids=["%s-lanes%d-%d" % c for c in CASES])
def test_gather_form_counts_every_term_once(mode, lanes, frames):
    import torch

    for name in sorted(R.DATA_SETS):
        inp, want = exact_case(name, frames)
        got, counts = run_tap(inp, mode, lanes, 0)
        assert counts == expected_census(mode, frames, 0), (name, counts)
        for key, exp in want.items():
            g = got[key]
            if not torch.equal(g, exp):
                bad = (g != exp).nonzero()
                first = tuple(int(i) for i in bad[0])
                raise AssertionError("%s, %d frames, lanes %d, data set %s: %s differs in %d of %d elements; first at %s: got "
                                     "%r, expected %r" % (mode, frames, lanes, name, key, bad.shape[0], g.numel(), first,
                                                          float(g[first]), float(exp[first])))


@pytest.mark.parametrize("mode", ["f32", "f32x3"])
def test_one_launch_per_layer_and_no_col2im(mode):
    from rela_amd import _capi as capi

    inp, _ = exact_case("dense", 17)
    buf = C.create_string_buffer(1 << 16)
    capi.check(capi.lib.rela_prof_summary_json(buf, len(buf)), "rela_prof_summary_json")  # (drops what came before)
    capi.lib.rela_prof_set_filter(None)
    capi.lib.rela_prof_enable(1)
    try:
        run_tap(inp, mode, 0, 0)
    finally:
        capi.lib.rela_prof_enable(0)
    capi.check(capi.lib.rela_prof_summary_json(buf, len(buf)), "rela_prof_summary_json")
    labels = json.loads(buf.value.decode())
    assert labels["learner_dgrad_conv2"]["count"] == 1 and labels["learner_dgrad_conv3"]["count"] == 1, labels
    assert "learner_col2im" not in labels, labels
