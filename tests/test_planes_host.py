"""Image networks of any channel count behind [net] yolo_input=planes, without a device: the key's range and refusals, what the planner chooses for layer 0
when the image is not three channels (never a fused first-stage kernel), that the key changes nothing for a three-channel cfg, the weight count, and the
helper that adds the key.  The fixtures tests/golden/mini_planes_*.npz come from the compiled reference (tools/make_golden.py planes): their cfg text is
darknet's own and carries no yolo_input key."""
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import hip, darknet_io as IO

FIXTURES = ["mini_planes_grey", "mini_planes_rgbd", "mini_planes_nine", "mini_planes_17"]
INVALID, UNSUPPORTED = -1, -6


def planes_cfg(n, height=12, width=10, extra=""):
    """a small classifier over n planes: a 3x3 conv, a 1x1 conv to four classes, [avgpool], [softmax]"""
    return ("[net]\nyolo_input=planes\nheight=%d\nwidth=%d\nchannels=%d\n%s\n" % (height, width, n, extra) +
            "[convolutional]\nbatch_normalize=1\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"
            "[convolutional]\nfilters=4\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n")


def _fixture_cfg(name):
    return IO.with_planes_input(str(golden(name + ".npz")["cfg"]))


@pytest.mark.parametrize("dtype", [hip.BF16, hip.FP16, hip.FP32])
@pytest.mark.parametrize("n", [1, 2, 4, 5, 8, 9, 17])
def test_plans_in_the_three_served_configurations(n, dtype):
    rc, msg = hip.plan_check(planes_cfg(n), dtype=dtype)
    assert rc == 0, msg


@pytest.mark.parametrize("dtype", [hip.BF16, hip.FP16, hip.FP32])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_cfgs_plan(name, dtype):
    rc, msg = hip.plan_check(_fixture_cfg(name), dtype=dtype)
    assert rc == 0, msg


@pytest.mark.parametrize("dtype,name", [(hip.FP8, "fp8"), (hip.FP16X2, "split-fp16")])
def test_fp8_and_split_fp16_are_refused_by_name(dtype, name):
    rc, msg = hip.plan_check(planes_cfg(4), dtype=dtype)
    assert rc == UNSUPPORTED and "yolo_input=planes with channels=4 is not served in the %s configuration" % name in msg, msg
    # three planes are the cfg without the key: planned as before
    rc, msg = hip.plan_check(IO.with_input_size(IO.cfg_text("yolov3"), 96).replace("[net]", "[net]\nyolo_input=planes", 1), dtype=dtype)
    assert rc == 0, msg


def test_range_and_size_are_checked():
    for n in (0, 1025, -3):
        rc, msg = hip.plan_check(planes_cfg(n))
        assert rc == INVALID and "yolo_input=planes" in msg and "channels=%d" % n in msg, msg
    assert hip.plan_check(planes_cfg(1024))[0] == 0
    for bad in ("height=0", "height=-2"):
        rc, msg = hip.plan_check(planes_cfg(4).replace("height=12", bad))
        assert rc == INVALID and "yolo_input=planes" in msg and bad in msg, msg
    rc, msg = hip.plan_check(planes_cfg(4).replace("width=10\n", ""))
    assert rc == INVALID and "yolo_input=planes" in msg and "width=0" in msg, msg
    rc, msg = hip.plan_check("[net]\nyolo_input=planes\ninputs=64\nchannels=4\n\n[connected]\noutput=8\nactivation=linear\n\n[softmax]\n")
    assert rc == INVALID and "yolo_input=planes" in msg and "inputs=64" in msg, msg
    rc, msg = hip.plan_check(planes_cfg(4).replace("yolo_input=planes", "yolo_input=image"))
    assert rc == INVALID and "yolo_input=image" in msg, msg


def test_without_the_key_nothing_changes():
    rc, msg = hip.plan_check(planes_cfg(4).replace("yolo_input=planes\n", ""))
    assert rc == UNSUPPORTED and "3 channels" in msg and "yolo_input=planes" in msg and "yolo_input=vector" in msg, msg


def test_three_planes_are_the_cfg_without_the_key():
    """yolov3 at 96 x 96: byte-identical dump, fused stem included; one plane: layers 0 and 1 through the tiled kernel, 32 * 9 * 2 fewer weights"""
    txt = IO.with_input_size(IO.cfg_text("yolov3"), 96)
    keyed = txt.replace("[net]", "[net]\nyolo_input=planes", 1)
    assert "yolo_input=planes" in keyed
    for dtype in (hip.BF16, hip.FP16, hip.FP32, hip.FP16X2, hip.FP8):
        for keep in (False, True):
            assert hip.plan_dump(keyed, dtype, 2, keep) == hip.plan_dump(txt, dtype, 2, keep)
    rc, table = hip.plan_table(txt)
    assert rc == 0 and "fused=stem" in table.splitlines()[0] and "fused=stem" in table.splitlines()[1]
    grey = keyed.replace("channels=3", "channels=1")
    rc, table = hip.plan_table(grey)
    assert rc == 0, table
    for line in table.splitlines()[:2]:
        assert "kernel=tiled fused=none" in line, line
    count = lambda text: int(hip.plan_dump(text)[1].split("weights_count=")[1].split()[0])
    assert count(txt) - count(grey) == 32 * 9 * 2


def _layer_fields(dump, i):
    line = [ln for ln in dump.splitlines() if ln.startswith("layer %d " % i)][0]
    return dict(f.split("=", 1) for f in line.split()[3:])


@pytest.mark.parametrize("dtype", [hip.BF16, hip.FP16, hip.FP32])
def test_no_first_stage_fusion_reads_another_channel_count(dtype):
    """each fixture opens with the shape of one fused first-stage kernel of the RGB path; none of them may be chosen"""
    rc, dump = hip.plan_dump(_fixture_cfg("mini_planes_rgbd"), dtype)
    assert rc == 0 and _layer_fields(dump, 0)["s2d7"] == "0" and _layer_fields(dump, 0)["cin"] == "4" and _layer_fields(dump, 0)["cin_pad"] == "8"
    rc, dump = hip.plan_dump(_fixture_cfg("mini_planes_grey"), dtype)
    for i in (0, 1):
        f = _layer_fields(dump, i)
        assert rc == 0 and f["kernel"] == "0" and f["fused"] == "0" and f["launcher"] == "-1", f
    assert " in_c=1 " in dump
    # the same cfg over three channels IS the fused stem's shape (16 bits)
    rc, rgb = hip.plan_dump(str(golden("mini_planes_grey.npz")["cfg"]).replace("channels=1", "channels=3"), dtype)
    assert rc == 0 and (_layer_fields(rgb, 0)["fused"] != "0") == (dtype != hip.FP32)
    rc, dump = hip.plan_dump(_fixture_cfg("mini_planes_17"), dtype)
    assert rc == 0 and _layer_fields(dump, 0)["cin"] == "17" and _layer_fields(dump, 0)["cin_pad"] == "24"
    rc, dump = hip.plan_dump(_fixture_cfg("mini_planes_nine"), dtype)
    assert rc == 0 and _layer_fields(dump, 0)["C"] == "9" and _layer_fields(dump, 1)["cin"] == "9" and _layer_fields(dump, 1)["cin_pad"] == "16"


def test_layer_zero_keeps_its_refusals():
    grouped = planes_cfg(4).replace("filters=8\n", "filters=8\ngroups=2\n", 1)
    rc, msg = hip.plan_check(grouped)
    assert rc == UNSUPPORTED and "groups=2" in msg and "first layer" in msg, msg
    crnn = "[net]\nyolo_input=planes\nheight=8\nwidth=8\nchannels=4\n\n[crnn]\nhidden_filters=8\noutput_filters=8\n\n" + planes_cfg(4).split("\n\n", 1)[1]
    rc, msg = hip.plan_check(crnn)
    assert rc == UNSUPPORTED and "[crnn]" in msg and "first layer" in msg, msg


@pytest.mark.parametrize("first", ["[maxpool]\nsize=2\nstride=2\n\n", "[reorg]\nstride=2\n\n", "[crop]\ncrop_height=10\ncrop_width=8\n\n",
                                   "[connected]\noutput=12\nactivation=leaky\n\n", "[local]\nfilters=4\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"])
def test_a_first_layer_that_is_no_conv_reads_the_planes(first):
    """eight planes (whole granules: what [connected] and [local] ask of any producer)"""
    tail = "[convolutional]\nfilters=4\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n"
    if first.startswith("[connected]"):
        tail = "[connected]\noutput=4\nactivation=linear\n\n[softmax]\n"
    rc, msg = hip.plan_check("[net]\nyolo_input=planes\nheight=12\nwidth=10\nchannels=8\n\n" + first + tail, dtype=hip.BF16)
    assert rc == 0, msg


def test_with_planes_input():
    grey = str(golden("mini_planes_grey.npz")["cfg"])
    assert "yolo_input" not in grey
    keyed = IO.with_planes_input(grey)
    assert keyed.count("yolo_input=planes") == 1 and IO.parse_cfg(keyed)[0]["yolo_input"] == "planes"
    assert IO.with_planes_input(keyed) == keyed
    assert [s for s in IO.parse_cfg(keyed)[1:]] == [s for s in IO.parse_cfg(grey)[1:]]
    rgb = IO.with_input_size(IO.cfg_text("yolov3"), 96)
    assert IO.with_planes_input(rgb) == rgb
    vec = "[net]\ninputs=37\nyolo_input=vector\n\n[connected]\noutput=37\nactivation=linear\n\n[softmax]\n"
    assert IO.with_planes_input(vec) == vec
    unsized = "[net]\ninputs=37\nchannels=1\n\n[connected]\noutput=37\nactivation=linear\n\n[softmax]\n"
    assert IO.with_planes_input(unsized) == unsized


@pytest.mark.parametrize("name", FIXTURES)
def test_weight_streams(name):
    """the fixture's stream, darknet_io's count and the planner's count agree: layer 0 holds filters x N x size^2 values; synth_weights gives a stream of
    that length for the cfg"""
    g = golden(name + ".npz")
    cfg = _fixture_cfg(name)
    secs = IO.parse_cfg(cfg)
    assert IO.weights_count(secs) == g["weights"].size
    rc, dump = hip.plan_dump(cfg)
    assert rc == 0 and int(dump.split("weights_count=")[1].split()[0]) == g["weights"].size
    assert IO.synth_weights(secs, seed=1).size == g["weights"].size
    h, w, ch = g["image_u8"].shape
    assert (int(secs[0]["height"]), int(secs[0]["width"]), int(secs[0]["channels"])) == (h, w, ch) and ch != 3


def test_pack_images_channels():
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 256, (5, 7), dtype=np.uint8), rng.integers(0, 256, (3, 4, 1), dtype=np.uint8)
    buf, descs = hip.pack_images([a, b], channels=1)
    assert buf.size == 35 + 12 and [int(d["offset"]) for d in descs] == [0, 35] and np.array_equal(buf[:35], a.reshape(-1))
    with pytest.raises(ValueError, match="3 channels, the network reads 4"):
        hip.pack_images([np.zeros((4, 4, 3), np.uint8)], channels=4)
    with pytest.raises(hip.YoloError):
        hip.pack_images([np.zeros((4, 4, 4), np.uint8)])
