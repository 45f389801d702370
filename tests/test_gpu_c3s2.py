"""conv_c3s2.hip: darknet-53's cfg layers 3-5 (conv3 32 -> 64, its shortcut, the 64 -> 128 stride-2 conv) in one launch, the layer-4
tensor in LDS only.  The fusion keeps every rounding point and K order of conv_halo_c32_c64 + conv_s2_c64_c128, so every comparison
here is np.array_equal.  The plans are told apart by Engine.conv_bytes: the fused plan does not count layer 4's write and read."""
import numpy as np
import pytest
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu

HEAD = """
[convolutional]
size=1
stride=1
pad=1
filters=18
activation=linear

[yolo]
mask=0,1,2
anchors=10,13, 16,30, 33,23
classes=1
num=3
"""


def _sections(text):
    """cfg text -> its sections as text blocks ([net] first)."""
    blocks = ("\n" + text).split("\n[")
    return ["[" + b.strip("\n") + "\n" for b in blocks[1:]]


def _first_stage(size, extra="", filters5=128):
    """The YOLOv3 cfg cut behind cfg layer 5, a 1x1 head on it: layer 5's buffer outlives the forward in every plan, so
    Engine.layer_output serves it without keep_layers."""
    secs = _sections(IO.with_input_size(IO.cfg_text("yolov3"), size))[:7]           # [net] + layers 0-5
    assert [s.split("]")[0] for s in secs[4:7]] == ["[convolutional", "[shortcut", "[convolutional"]
    if filters5 != 128:
        secs[6] = secs[6].replace("filters=128", "filters=%d" % filters5)
    return "\n".join(secs) + extra + HEAD


def _engine(hiplib, monkeypatch, txt, flat, batch, dtype, keep=False, no_c3s2=False):
    if no_c3s2: monkeypatch.setenv("YOLO_NO_C3S2", "1")
    else: monkeypatch.delenv("YOLO_NO_C3S2", raising=False)
    eng = hiplib.Engine(txt, max_batch=batch, dtype=dtype, keep_layers=keep)
    monkeypatch.delenv("YOLO_NO_C3S2", raising=False)
    eng.set_weights(flat)
    return eng


def _l4_bytes(size, batch):
    return 2.0 * batch * (size // 2) * (size // 2) * 64 * 2          # layer 4 written once, read once, 16-bit


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("size", [32, 64, 96])
def test_fused_conv3_s2_equals_layer_by_layer_plan(hiplib, monkeypatch, size, dtype_name):
    """YOLOv3 at 32 / 64 / 96 (the stride-2 output is 8 / 16 / 24 pixels: one 4 x 8 tile column that touches both side borders; 2 columns,
    every tile on a seam and a border; 3 columns with fully interior tiles), batch 3 (the tile walk of a workgroup crosses image boundaries
    with an odd count): detections of the fused plan against keep_layers=True and against the plan with YOLO_NO_C3S2 set; layer 5's
    tensor, on the network cut behind it, against both as well."""
    dtype = hiplib.BF16 if dtype_name == "bf16" else hiplib.FP16
    img = np.random.default_rng(size).integers(0, 256, (3, size, size, 3), dtype=np.uint8)
    txt = IO.with_input_size(IO.cfg_text("yolov3"), size)
    flat = IO.synth_weights(IO.parse_cfg(txt), seed=11)
    dets, nbytes = [], []
    for keep, off in ((False, False), (True, False), (False, True)):
        eng = _engine(hiplib, monkeypatch, txt, flat, 3, dtype, keep=keep, no_c3s2=off)
        dets.append(eng.forward(img)); nbytes.append(eng.conv_bytes(3))
        eng.close()
    assert np.abs(dets[0]).max() > 0 and np.array_equal(dets[0], dets[1]) and np.array_equal(dets[0], dets[2])
    assert nbytes[2] - nbytes[0] == _l4_bytes(size, 3)               # the first plan is the fused one, the switch turns it off
    cut = _first_stage(size)
    cflat = IO.synth_weights(IO.parse_cfg(cut), seed=12)
    outs = []
    for keep, off in ((False, False), (True, False), (False, True)):
        eng = _engine(hiplib, monkeypatch, cut, cflat, 3, dtype, keep=keep, no_c3s2=off)
        eng.forward(img); outs.append(eng.layer_output(5, 3))
        eng.close()
    assert outs[0].shape == (3, size // 4, size // 4, 128) and np.abs(outs[0]).max() > 0.1
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_layer4_padding_is_zero_not_conv3_of_padding(hiplib, monkeypatch):
    """The stride-2 conv pads LAYER 4.  With conv3's bias at 4.0 (batch norm folded: beta = 4, mean = 0), 'conv3 of the zero-padded
    window' is far from zero, so a layer-4 tile that is not masked by position shows on every border output.  Size 32, batch 1: one tile
    column, every tile on a border."""
    cut = _first_stage(32)
    secs = IO.parse_cfg(cut)
    flat = IO.synth_weights(secs, seed=13).copy()
    off = 0
    for c in IO.conv_specs(secs):
        n = c["filters"]
        if c["index"] == 3:
            assert c["bn"] and n == 64
            flat[off:off + n] = 4.0                                  # darknet order: beta, gamma, mean, variance, filters
            flat[off + 2 * n:off + 3 * n] = 0.0
        off += n * (4 if c["bn"] else 1) + n * c["cin"] * c["size"] ** 2
    assert off == flat.size
    img = np.random.default_rng(5).integers(0, 256, (1, 32, 32, 3), dtype=np.uint8)
    outs = []
    for keep in (False, True):
        eng = _engine(hiplib, monkeypatch, cut, flat, 1, hiplib.BF16, keep=keep)
        eng.forward(img); outs.append(eng.layer_output(5, 1))
        if keep:
            assert float(eng.layer_output(3, 1).mean()) > 1.0        # the bias took: conv3 alone sits near 4
        eng.close()
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0][0, 0], outs[1][0, 0]) and np.array_equal(outs[0][0, :, 0], outs[1][0, :, 0])      # (the border rows, named)


@pytest.mark.parametrize("kind", ["route", "filters"])
def test_other_readers_or_shapes_fall_back_to_the_two_kernels(hiplib, monkeypatch, kind):
    """A second reader of layer 4 (a [route] to it behind layer 5) or another stride-2 shape (64 -> 256 filters): the plan is today's two
    launches -- it counts layer 4's traffic whether or not the switch is set -- and gives the bits of keep_layers=True."""
    size = 64
    if kind == "route":
        # layers 6-8: route to layer 4, a stride-2 pool to layer 5's grid, route [5, 7] -> 192 channels into the head
        extra = "\n[route]\nlayers=4\n\n[maxpool]\nsize=2\nstride=2\n\n[route]\nlayers=5,7\n"
        cut = _first_stage(size, extra=extra)
    else:
        cut = _first_stage(size, filters5=256)
    flat = IO.synth_weights(IO.parse_cfg(cut), seed=14)
    img = np.random.default_rng(6).integers(0, 256, (3, size, size, 3), dtype=np.uint8)
    dets, nbytes = [], []
    for keep, off in ((False, False), (True, False), (False, True)):
        eng = _engine(hiplib, monkeypatch, cut, flat, 3, hiplib.BF16, keep=keep, no_c3s2=off)
        dets.append(eng.forward(img)); nbytes.append(eng.conv_bytes(3))
        eng.close()
    assert nbytes[0] == nbytes[2]                                    # not fused: the switch changes nothing
    assert np.abs(dets[0]).max() > 0 and np.array_equal(dets[0], dets[1]) and np.array_equal(dets[0], dets[2])
