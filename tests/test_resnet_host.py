"""ResNet / VGG classifiers, planner side (no device): the general [shortcut] (a `from` tensor with other channels or another size, any
activation) and darknet's thirteen activations are planned in every configuration that serves them, and refused, naming the layer,
where they are not."""
import os
import re
import numpy as np
import pytest
from conftest import golden
from oracle import darknet_ref as DR
from yolo_tensorflow_amd import hip, darknet_io as IO

ACTS = ("logistic", "loggy", "relu", "elu", "relie", "ramp", "linear", "tanh", "plse", "leaky", "stair", "hardtan", "lhtan")      # DN/activations.c get_activation


def raised(cfg, mul=2):
    """the mini cfg with every conv but the class conv `mul` times as wide (16 -> 32: whole 32-channel groups, what split-fp16 pairs need)"""
    return re.sub(r"filters=(\d+)", lambda m: "filters=%d" % (int(m.group(1)) * (1 if m.group(1) == "24" else mul)), cfg)


MINI = [str(golden(n)["cfg"]) for n in ("mini_resnet.npz", "mini_resnet_30.npz")]


def _ok(cfg, dtype):
    rc, msg = hip.plan_check(cfg, dtype=dtype)
    assert rc == 0, msg


@pytest.mark.parametrize("name", ["resnet18", "resnet50", "vgg-16"])
def test_shipped_cfgs_plan(name):
    for dtype in (hip.FP32, hip.BF16, hip.FP16):
        _ok(IO.cfg_text(name), dtype)


@pytest.mark.parametrize("dtype", [hip.FP32, hip.BF16, hip.FP16])
def test_mini_cfgs_plan(dtype):
    for cfg in MINI:
        _ok(cfg, dtype)


def test_split_fp16_plans():
    for name in ("resnet18", "resnet50"):
        _ok(IO.cfg_text(name), hip.FP16X2)
    for cfg in MINI:
        _ok(raised(cfg), hip.FP16X2)


def test_generated_depths_plan():
    """ResNet-34 / 101 / 152 are generated on request, not shipped: the generator's block tables give the published conv counts"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_cfgs", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_cfgs.py"))
    M = importlib.util.module_from_spec(spec); spec.loader.exec_module(M)
    for depth in (18, 34, 50, 101, 152):
        txt = M.resnet(depth)
        assert sum(s["type"] == "convolutional" for s in IO.parse_cfg(txt)) == depth          # stem + blocks + the class conv: darknet's ResNets have no projection convs
        _ok(txt, hip.BF16)
    assert M.resnet(18) == IO.cfg_text("resnet18").split("\n", 1)[1] and M.resnet(50) == IO.cfg_text("resnet50").split("\n", 1)[1]
    assert M.vgg16() == IO.cfg_text("vgg-16").split("\n", 1)[1]


def test_every_activation_name_plans_and_maps():
    base = MINI[0]
    for k, name in enumerate(hip.ACTIVATIONS):
        assert hip.activation_code(name) == k
        _ok(base.replace("activation=tanh", "activation=" + name), hip.BF16)
        _ok(base.replace("activation=elu", "activation=" + name), hip.BF16)
    assert sorted(hip.ACTIVATIONS) == sorted(ACTS)
    with pytest.raises(hip.YoloError):
        hip.activation_code("swish")


def test_refusals_name_the_layer():
    base = MINI[0]
    rc, msg = hip.plan_check(base.replace("activation=tanh", "activation=swish"))
    assert rc != 0 and "layer 15" in msg and "swish" in msg
    rc, msg = hip.plan_check(base.replace("activation=elu", "activation=mish"))
    assert rc != 0 and "layer 17" in msg and "mish" in msg
    rc, msg = hip.plan_check(base, dtype=hip.FP8)
    assert rc != 0 and "fp8" in msg and "layer" in msg
    fp8_ok = "[net]\nwidth=32\nheight=32\nchannels=3\n\n" + "[convolutional]\nbatch_normalize=1\nfilters=16\nsize=3\nstride=1\npad=1\nactivation=relu\n\n" * 2 + "[shortcut]\nfrom=-2\nactivation=%s\n\n" + \
             "[convolutional]\nfilters=6\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[yolo]\nmask=0\nanchors=10,14\nclasses=1\nnum=1\n"
    _ok(fp8_ok % "linear", hip.FP8)          # today's matched, linear shortcut stays served in fp8 (and relu rides in the conv epilogue)
    rc, msg = hip.plan_check(fp8_ok % "leaky", dtype=hip.FP8)
    assert rc != 0 and "layer 2" in msg and "not served in the fp8 configuration" in msg
    rc, msg = hip.plan_check(fp8_ok.replace("activation=relu", "activation=logistic") % "linear", dtype=hip.FP8)
    assert rc != 0 and "layer 0" in msg and "not served in the fp8 configuration" in msg
    for cfg in MINI:          # 16- and 8-channel tensors as pairs: not whole 32-channel groups
        rc, msg = hip.plan_check(cfg, dtype=hip.FP16X2)
        assert rc != 0 and "layer 5" in msg and "multiples of 32" in msg


def test_shortcut_size_assertion_is_refused():
    """DN/blas.c:72-73.  A square network keeps w1 / w2 == h1 / h2, so the planner's check is reached through the geometry the library
    shares with the single operator: yolo_op_shortcut refuses before it touches a device"""
    x = np.zeros((1, 8, 4, 8), np.float32); f = np.zeros((1, 16, 16, 8), np.float32)          # 16 / 4 = 4 but 16 / 8 = 2
    with pytest.raises(hip.YoloError, match="w1 / w2 == h1 / h2"):
        hip.op_shortcut(x, f)


def test_reference_activations_are_correctly_rounded():
    """What test_gpu_resnet.py's bound for the exp-based activations rests on: the reference's C code (a one-layer network, identity
    1 x 1 conv, that activation) stands off from the float64 formula by 0.5 u max(1, |y|) -- it evaluates in double and rounds once."""
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")
    from test_gpu_resnet import act64, act_inputs, EXP_ACTS, K_REF, U
    x = act_inputs()
    pad = np.concatenate([x, np.zeros(-x.size % 24, np.float32)]).reshape(-1, 8, 3)
    for name in EXP_ACTS:
        cfg = "[net]\nbatch=1\nwidth=8\nheight=%d\nchannels=3\n\n[convolutional]\nfilters=3\nsize=1\nstride=1\npad=0\nactivation=%s\n" % (pad.shape[0], name)
        net = DR.RefNet(cfg, np.concatenate([np.zeros(3), np.eye(3).reshape(-1)]).astype(np.float32), 0, 2)
        net.predict(pad)
        got = net.layer_output_nhwc(0)[0].reshape(-1)[:x.size].astype(np.float64)
        net.close()
        y = act64(name, x)
        k = float((np.abs(got - y) / (U * np.maximum(1, np.abs(y)))).max())
        print("%s: the reference stands off from float64 by %.3f u max(1, |y|)" % (name, k))
        assert k <= K_REF
