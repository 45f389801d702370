"""Rectangular network inputs (width != height), the part that needs no device: the planner (yolo_plan_table), what it still refuses,
darknet_io.with_input_size, and the goldens of the compiled reference at 64 x 96 / 96 x 64 against the project's own numpy oracle."""
import numpy as np
import pytest
from conftest import golden
from oracle import yolo_ref as R
from yolo_tensorflow_amd import hip, darknet_io as IO

DTYPES = {"bf16": hip.BF16, "fp16": hip.FP16, "fp16x2": hip.FP16X2, "fp32": hip.FP32, "fp8": hip.FP8}
# height, width.  Half of 416 would be 208, but YOLOv3 cannot be planned there by anybody: 208 / 32 = 6.5, so the stride-32 grid has 7 rows,
# its 2x upsample 14, and the stride-16 tensor it is concatenated with 13 (darknet's route layer gives up the same way;
# test_yolov3_needs_multiples_of_32 pins the refusal).  192 x 416 is the nearest size at which the topology closes and every fusion of the
# headline plan still fires: 48 x 104 at the 128-channel stage (the resblock launch's 13 x 13 blocks cover it within 15 %), 13 x 13 halo
# blocks on ragged 12 x 26 / 6 x 13 grids.
RECT = (192, 416)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_plan_table_of_a_rectangular_yolov3(dtype):
    rc, text = hip.plan_table(IO.with_input_size(IO.cfg_text("yolov3"), RECT), dtype=DTYPES[dtype], max_batch=3)
    assert rc == 0, text
    last = text.strip().splitlines()[-1]
    assert last.startswith("input 192x416 ")
    assert last.endswith(" rows %d" % (3 * (13 * 6 + 26 * 12 + 52 * 24)))
    assert "grid 6x13 anchors 3" in last and "grid 12x26 anchors 3" in last and "grid 24x52 anchors 3" in last
    if dtype == "bf16":
        rows = text.splitlines()
        assert "fused=stem launcher=1" in rows[0] and "fused=stem launcher=1" in rows[1] and "fused=stem" in rows[2]
        assert "kernel=halo fused=c3s2 launcher=5" in rows[3] and "kernel=s2 fused=c3s2 launcher=5" in rows[5]
        assert sum("fused=resblock" in r for r in rows) == 4          # the two blocks of the 128-channel stage, two layers each


def test_yolov3_needs_multiples_of_32():
    for hw in ((208, 416), (416, 208)):
        rc, msg = hip.plan_table(IO.with_input_size(IO.cfg_text("yolov3"), hw))
        assert rc != 0 and "route spatial mismatch" in msg


def test_square_tables_print_no_rectangular_line():
    rc, text = hip.plan_table(IO.with_input_size(IO.cfg_text("yolov3"), 96))
    assert rc == 0 and text.strip().splitlines()[-1].startswith("buffers ") and "input " not in text


@pytest.mark.parametrize("key,value", [("height", 0), ("width", -32), ("channels", 1)])
def test_still_refused(key, value):
    txt = IO.with_input_size(IO.cfg_text("yolov3"), RECT)
    out = [("%s=%d" % (key, value)) if line.split("=")[0].strip() == key else line for line in txt.splitlines()]
    rc, msg = hip.plan_table("\n".join(out))
    assert rc != 0 and "square" not in msg and "3 channels" in msg


def test_with_input_size():
    base = IO.cfg_text("yolov3")
    legacy = "\n".join(("%s=%d" % (l.split("=")[0].strip(), 320)) if l.split("=")[0].strip() in ("width", "height") else l for l in base.splitlines())
    assert IO.with_input_size(base, 320) == legacy == IO.with_input_size(base, (320, 320))
    net = IO.parse_cfg(IO.with_input_size(base, (352, 608)))[0]
    assert int(net["height"]) == 352 and int(net["width"]) == 608


@pytest.mark.parametrize("name", ["mini_v3_rect.npz", "mini_v2_rect.npz"])
def test_oracle_forward_matches_compiled_darknet_every_layer(name):
    """The form and tolerance of tests/test_oracle_golden.py's square twin."""
    g = golden(name)
    secs = R.parse_cfg(str(g["cfg"]))
    params = R.unflatten_weights(g["weights"], secs)
    x = g["image_u8"].astype(np.float32)[None] / np.float32(255.0)
    assert x.shape[1] != x.shape[2]
    heads, outs = R.forward(secs, params, x, semantics="darknet", bn_mode="darknet_cpu", collect=True)
    for i, o in enumerate(outs):
        ref = g["layer_%02d" % i]
        if o is None:
            continue
        assert o.shape == ref.shape, (i, o.shape, ref.shape)
        np.testing.assert_allclose(o, ref, rtol=2e-5, atol=2e-5, err_msg="layer %d" % i)


@pytest.mark.parametrize("name,classes", [("mini_v3_rect.npz", 4), ("mini_v2_rect.npz", 5)])
def test_fixture_conditions(name, classes):
    """Every head has a box above thresh, at least 8 boxes in all, do_nms_sort suppresses at least one and leaves at least one."""
    g = golden(name)
    secs = R.parse_cfg(str(g["cfg"]))
    thresh = float(g["thresh"])
    for i, s in enumerate(secs[1:]):
        if s["type"] in ("yolo", "region"):
            assert (g["layer_%02d" % i][..., 4::5 + classes] > thresh).sum() >= 1, "head at layer %d" % i
    assert len(g["boxes_raw"]) >= 8
    assert 0 < (g["prob_nms"] > 0).sum() < (g["prob_raw"] > 0).sum()


def test_letterbox_fixture_conditions():
    g, net = golden("mini_v3_rect_letterbox.npz"), golden("mini_v3_rect.npz")
    nh, nw = net["image_u8"].shape[:2]
    for k, (ih, iw) in enumerate(((37, 80), (50, 37), (32, 48))):
        assert g["src_%d" % k].shape == (3, ih, iw) and g["input_%d" % k].shape == (3, nh, nw)
        assert len(g["boxes_%d" % k]) >= 8 and 0 < (g["prob_nms_%d" % k] > 0).sum() < (g["prob_%d" % k] > 0).sum()
    # 37 x 80 is wider than 64 x 96: the width binds, grey bars above and below; 50 x 37: the height binds, bars left and right
    assert np.all(g["input_0"][:, 0, :] == 0.5) and not np.all(g["input_0"][:, :, 0] == 0.5)
    assert np.all(g["input_1"][:, :, 0] == 0.5) and not np.all(g["input_1"][:, 0, :] == 0.5)
    assert not np.any(np.all(g["input_2"] == 0.5, axis=0))
