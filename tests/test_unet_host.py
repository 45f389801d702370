"""Dense-prediction networks, host side (no device): the planner accepts [deconvolutional], [logistic], [activation], [l2norm], darknet's
[upsample] and the declared map kind in every configuration that serves them and refuses, with a message of its own, what it does
not; the weight stream's length; the native-pixel -> map-pixel rule; and the numpy restatements the GPU tests (test_gpu_unet.py)
compare the device against, checked here against the compiled reference's recorded layer outputs."""
import numpy as np
import pytest
from conftest import golden
from oracle import darknet_ref as DR
from yolo_tensorflow_amd import hip, darknet_io as IO

FIXTURES = ("mini_unet.npz", "mini_deconv_odd.npz")
SLOPES = {"linear": 1.0, "leaky": 0.1, "relu": 0.0, "relie": 0.01}


# ---- restatements shared with test_gpu_unet.py ----
def deconv_ref(x, w_iohw, bias, stride, pad, dtype=np.float64):
    """DN/deconvolutional_layer.c as the issue states it: out[f, iy*s - p + kh, ix*s - p + kw] += sum_ci w[ci, f, kh, kw] * in[ci, iy, ix],
    plus bias; x [n, h, w, cin], w [cin, cout, k, k] -> [n, (h-1)s + k - 2p, (w-1)s + k - 2p, cout]"""
    x = np.asarray(x, dtype=dtype); w = np.asarray(w_iohw, dtype=dtype)
    n, h, wd, cin = x.shape; cout, k = w.shape[1], w.shape[2]
    full = np.zeros((n, (h - 1) * stride + k, (wd - 1) * stride + k, cout), dtype=dtype)
    for kh in range(k):
        for kw in range(k):
            full[:, kh:kh + (h - 1) * stride + 1:stride, kw:kw + (wd - 1) * stride + 1:stride, :] += x @ w[:, :, kh, kw]
    ho, wo = (h - 1) * stride + k - 2 * pad, (wd - 1) * stride + k - 2 * pad
    out = full[:, pad:pad + ho, pad:pad + wo, :]
    return out + (0 if bias is None else np.asarray(bias, dtype=dtype))


def tap_counts(h, w, k, stride, pad):
    """how many (kh, kw, iy, ix) land on each output pixel: deconv_ref of ones with one input and one output channel"""
    return deconv_ref(np.ones((1, h, w, 1)), np.ones((1, 1, k, k)), None, stride, pad)[0, :, :, 0]


def letterbox_dims(net_w, net_h, w, h):
    """darknet's letterbox_image integers (DN/image.c:960-966), float32 comparison included"""
    if np.float32(net_w) / np.float32(w) < np.float32(net_h) / np.float32(h):
        return net_w, (h * net_w) // w
    return (w * net_h) // h, net_h


def map_coord(x, w, new_w, dx, net_w, map_w):
    """the rule of include/yolo_hip.h (yolo_segment_images_u8) in Python integers (unbounded, so the 64-bit device form cannot differ)"""
    x = np.asarray(x).astype(object)
    m = ((2 * x + 1) * int(new_w) + 2 * int(w) * int(dx)) * int(map_w) // (2 * int(w) * int(net_w))
    return np.minimum(m.astype(np.int64), map_w - 1)


def native_to_map(h, w, fit_letterbox, net_hw, map_hw):
    """(my [h], mx [w]): the map row / column every native row / column of an h x w image takes"""
    net_h, net_w = net_hw
    new_w, new_h = letterbox_dims(net_w, net_h, w, h) if fit_letterbox else (net_w, net_h)
    dx, dy = (net_w - new_w) // 2, (net_h - new_h) // 2
    return map_coord(np.arange(h), h, new_h, dy, net_h, map_hw[0]), map_coord(np.arange(w), w, new_w, dx, net_w, map_hw[1])


def _ok(cfg, dtype):
    rc, msg = hip.plan_check(cfg, dtype=dtype)
    assert rc == 0, msg


def _refused(cfg, *needles, dtype=hip.BF16):
    rc, msg = hip.plan_check(cfg, dtype=dtype)
    assert rc != 0, "planned: " + cfg
    for n in needles:
        assert n in msg, (n, msg)
    return msg


# ---- the planner ----
@pytest.mark.parametrize("dtype", [hip.FP32, hip.BF16, hip.FP16])
@pytest.mark.parametrize("name", FIXTURES)
def test_mini_cfgs_plan(name, dtype):
    _ok(str(golden(name)["cfg"]), dtype)


def test_refusals_are_distinct():
    unet = str(golden("mini_unet.npz")["cfg"]); odd = str(golden("mini_deconv_odd.npz")["cfg"])
    msgs = []
    for cfg, layer in ((unet, "layer 3"), (odd, "layer 2")):
        msgs.append(_refused(cfg, layer, "[deconvolutional]", "fp8", dtype=hip.FP8))
        msgs.append(_refused(cfg, layer, "[deconvolutional]", "split-fp16", dtype=hip.FP16X2))
    assert msgs[0] != msgs[1]
    one = "[net]\nwidth=8\nheight=6\nchannels=3\nyolo_output=map\n\n[deconvolutional]\nfilters=8\nsize=%d\nstride=%d\npadding=%d\nactivation=linear\n"
    _ok(one % (7, 4, 6), hip.BF16)
    msgs.append(_refused(one % (3, 5, 1), "layer 0", "stride 5"))
    msgs.append(_refused(one % (8, 2, 1), "layer 0", "size 8"))
    msgs.append(_refused(one % (3, 1, 3), "layer 0", "padding 3"))
    msgs.append(_refused("[net]\nwidth=1\nheight=1\nchannels=3\nyolo_output=map\n\n[deconvolutional]\nfilters=8\nsize=2\nstride=1\npadding=1\nactivation=linear\n", "layer 0", "not positive"))
    head = "[convolutional]\nfilters=6\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[yolo]\nmask=0\nanchors=10,14\nclasses=1\nnum=1\n"
    msgs.append(_refused("[net]\nwidth=32\nheight=32\nchannels=3\nyolo_output=map\n\n" + head, "yolo_output=map", "head"))
    msgs.append(_refused(unet.replace("stride=2\nscale=0.5", "stride=0\nscale=0.5"), "layer 9", "upsample stride 0"))
    msgs.append(_refused(unet.replace("yolo_output=map", "yolo_output=heat"), "yolo_output=heat"))
    assert len(set(msgs)) == len(msgs), msgs
    with pytest.raises(hip.YoloError, match="300 channels"):          # refused before a device is touched
        hip.op_label_map(np.zeros((1, 2, 2, 300), np.float32))
    with pytest.raises(hip.YoloError, match="stride"):
        hip.op_upsample(np.zeros((1, 2, 2, 8), np.float32), stride=0)
    with pytest.raises(hip.YoloError, match="served are"):
        hip.op_deconv2d(np.zeros((1, 2, 2, 8), np.float32), np.zeros((8, 8, 3, 3), np.float32), stride=5)
    with pytest.raises(hip.YoloError, match="fp8 and split-fp16"):
        hip.op_deconv2d(np.zeros((1, 2, 2, 8), np.float32), np.zeros((8, 8, 3, 3), np.float32), dtype=hip.FP8)


def test_headless_cfg_without_the_key_is_still_refused():
    for name in FIXTURES:
        cfg = str(golden(name)["cfg"]).replace("yolo_output=map\n", "")
        rc, msg = hip.plan_check(cfg)
        assert rc != 0 and msg == "cfg has no [yolo] / [region] / [detection] head"


def test_upsample_keeps_the_stride_2_rule_for_tf_semantics():
    """plan_check plans with the TF semantics: any stride but 2 is refused there with the message it always had"""
    base = "[net]\nwidth=16\nheight=16\nchannels=3\nyolo_output=map\n\n[convolutional]\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n[upsample]\nstride=%d\n"
    _ok(base % 2, hip.BF16)
    for st in (1, 3, 8):
        rc, msg = hip.plan_check(base % st)
        assert rc != 0 and msg == "layer 1: upsample stride %d" % st


# ---- the weight stream ----
@pytest.mark.parametrize("name", FIXTURES)
def test_weights_count_is_what_the_reference_loader_consumes(name):
    """darknet_io counts a [deconvolutional] section as DN/parser.c:1169 loads it: biases / scales / mean / variance, then cin * filters *
    size^2 filters -- the length of the stream the reference loaded when the fixture was made"""
    g = golden(name); cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg)
    flat = g["weights"]
    assert IO.weights_count(secs) == flat.size
    want = sum(s_["filters"] * (4 if s_["bn"] else 1) + s_["cin"] * s_["filters"] * s_["size"] ** 2 for s_ in IO.conv_specs(secs))
    assert want == flat.size and IO.synth_weights(secs, seed=3).size == flat.size


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_loader_reads_the_stream_to_its_last_float_and_no_further(name):
    """the compiled reference on the fixture's stream: floats appended to it change nothing (it reads no further) and the last float
    changes the last layer's output (it reads that far)"""
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")
    g = golden(name); cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg)
    flat = g["weights"]
    x = g["images_u8"][0].astype(np.float32) / np.float32(255)
    last = len(secs) - 2

    def run(stream):
        net = DR.RefNet(cfg, stream, 0, 2); net.predict(x); out = net.layer_output_nhwc(last).copy(); net.close(); return out
    base = run(flat)
    assert np.array_equal(base[0], g["layer_%02d" % last][0])
    assert np.array_equal(run(np.concatenate([flat, np.full(64, 1e9, np.float32)])), base)
    changed = flat.copy(); changed[-1] += np.float32(1.0)
    assert not np.array_equal(run(changed), base)


# ---- the native pixel -> map pixel rule ----
@pytest.mark.parametrize("letterbox", [False, True])
def test_native_pixels_map_inside_the_map(letterbox):
    net_hw, map_hw = (48, 80), (24, 40)
    for h, w in ((37, 91), (200, 50)):
        my, mx = native_to_map(h, w, letterbox, net_hw, map_hw)
        assert my.min() >= 0 and my.max() <= map_hw[0] - 1 and mx.min() >= 0 and mx.max() <= map_hw[1] - 1
        assert (np.diff(my) >= 0).all() and (np.diff(mx) >= 0).all()
        if not letterbox:          # a stretch reaches both edges of the map
            assert my[0] == 0 and my[-1] == map_hw[0] - 1 and mx[0] == 0 and mx[-1] == map_hw[1] - 1
    my, mx = native_to_map(48, 80, letterbox, (48, 80), (48, 80))          # image, input and map of one size: the identity
    assert np.array_equal(my, np.arange(48)) and np.array_equal(mx, np.arange(80))


def test_letterboxed_pixels_stay_inside_the_fitted_window():
    """a 200 x 50 image in a 48 x 80 input is 12 columns wide at offset 34: its pixels read only the map columns that window covers"""
    net_hw, map_hw = (48, 80), (24, 40)
    new_w, new_h = letterbox_dims(80, 48, 50, 200)
    assert (new_w, new_h) == (12, 48)
    _, mx = native_to_map(200, 50, True, net_hw, map_hw)
    assert mx.min() == 34 * 40 // 80 and mx.max() == (34 + 12) * 40 // 80 - 1


# ---- the restatement against the reference's recorded layers ----
def _bn_fold_ref(p, x):
    """DN/blas.c normalize_cpu + scale + bias in float64: (x - mean) / (sqrt(var) + 1e-6) * gamma + beta"""
    return (x - p["mean"]) / (np.sqrt(p["var"]) + 1e-6) * p["gamma"] + p["beta"]


def stream_params(cfg, flat):
    """{layer index: dict(w, and bias or beta / gamma / mean / var)} of every [convolutional] / [deconvolutional] section"""
    secs = IO.parse_cfg(cfg); out = {}; at = 0
    flat = np.asarray(flat, dtype=np.float64)
    for spec in IO.conv_specs(secs):
        n, k, cin = spec["filters"], spec["size"], spec["cin"]; p = {}
        if spec["bn"]:
            for key in ("beta", "gamma", "mean", "var"):
                p[key] = flat[at:at + n]; at += n
        else:
            p["bias"] = flat[at:at + n]; at += n
        deconv = secs[spec["index"] + 1]["type"] == "deconvolutional"
        p["w"] = flat[at:at + n * cin * k * k].reshape((cin, n, k, k) if deconv else (n, cin, k, k)); at += n * cin * k * k
        out[spec["index"]] = p
    assert at == flat.size
    return out


def deconv_layer_ref(sec, p, x):
    """one [deconvolutional] section of a cfg in float64: scatter, batch norm or bias, a slope-family activation (others: the caller's)"""
    k, st = int(sec.get("size", 1)), int(sec.get("stride", 1))
    pad = k // 2 if int(sec.get("pad", 0)) else int(sec.get("padding", 0))
    y = deconv_ref(x, p["w"], None, st, pad)
    y = _bn_fold_ref(p, y) if "beta" in p else y + p["bias"]
    act = sec.get("activation", "logistic")
    if act in SLOPES:
        y = np.where(y > 0, y, SLOPES[act] * y)
    elif act == "tanh":
        y = np.tanh(y)
    else:
        raise ValueError(act)
    return y


@pytest.mark.parametrize("name", FIXTURES)
def test_deconv_restatement_matches_the_reference_layers(name):
    """every [deconvolutional] layer of both fixtures -- 4/2/1 with batch norm, 2/2/0 with tanh, 3/1/1, 3/2/1, 5/3/2, 1/2/0 --, float64 on
    the reference's own input of that layer: 5e-4 of the tensor's scale (measured: a few 1e-7, the reference's fp32 summation)"""
    g = golden(name); cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    params = stream_params(cfg, g["weights"])
    seen = 0
    for i, s in enumerate(secs):
        if s["type"] != "deconvolutional":
            continue
        want = g["layer_%02d" % i].astype(np.float64)
        got = deconv_layer_ref(s, params[i], g["layer_%02d" % (i - 1)])
        assert got.shape == want.shape
        r = float(np.abs(got - want).max() / np.abs(want).max())
        print("%s layer %d (%s/%s): relmax %.3e" % (name, i, s["size"], s["stride"], r))
        assert r < 5e-4
        seen += 1
    assert seen == 3


def test_small_layers_restated_match_the_reference_layers():
    """[l2norm], [upsample] stride 2 scale 0.5, [logistic] and [activation] elu as the GPU tests restate them, against the fixtures"""
    g = golden("mini_unet.npz")
    x = g["layer_07"].astype(np.float64)
    l2 = x / np.sqrt((x * x).sum(axis=-1, keepdims=True))
    assert np.abs(l2 - g["layer_08"]).max() <= 4 * 2.0 ** -24
    assert np.array_equal(np.repeat(np.repeat(g["layer_08"], 2, axis=1), 2, axis=2) * np.float32(0.5), g["layer_09"])
    assert np.abs(1 / (1 + np.exp(-g["layer_10"].astype(np.float64))) - g["layer_11"]).max() <= 2.0 ** -24
    o = golden("mini_deconv_odd.npz")
    x = o["layer_02"].astype(np.float64)
    assert np.abs(np.where(x >= 0, x, np.exp(x) - 1) - o["layer_03"]).max() <= 2.0 ** -24 * max(1.0, float(np.abs(o["layer_03"]).max()))


def test_fixture_margins():
    """what the label tests lean on: the recorded margins are the recorded outputs' own, and at most 2 % of the pixels are near-ties"""
    for name in FIXTURES:
        g = golden(name); n_layers = len(IO.parse_cfg(str(g["cfg"]))) - 1
        out = g["layer_%02d" % (n_layers - 1)]
        top2 = np.sort(out, axis=-1)[..., -2:]
        assert np.array_equal(g["margin"], top2[..., 1] - top2[..., 0]) and np.array_equal(g["argmax"], np.argmax(out, axis=-1))
        assert float(g["scale"]) == float(np.abs(out).max())
        share = (g["margin"] < 2 * 5e-4 * float(g["scale"])).reshape(3, -1).mean(axis=1)
        assert np.allclose(share, g["tight_share"]) and share.max() <= 0.02
        assert len(np.unique(g["argmax"])) >= 4


def test_tap_counts_restatement():
    """4/2/1 on 5 x 7: interior pixels see 2 x 2 taps, the border rows and columns one fewer; 1/2/0: three of four phases see none"""
    t = tap_counts(5, 7, 4, 2, 1)
    assert t.shape == (10, 14) and t[1:-1, 1:-1].min() == 4 and t[0, 0] == 1 and t[0, 1] == 2
    e = tap_counts(5, 7, 1, 2, 0)
    assert e.shape == (9, 13) and (e[::2, ::2] == 1).all() and e.sum() == 35
