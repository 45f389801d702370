"""[convolutional] with groups=, host side (no device): the weight stream's length and conv_specs against darknet's formula
(DN/convolutional_layer.c:201: filters * (c / groups) * size^2), the planner's acceptance in the three configurations that serve the key and
its refusals -- each with its status and a message that names the layer --, and the float64 restatement the GPU tests (test_gpu_grouped.py)
compare the device against, checked here against the compiled reference's recorded layer outputs: the fixture is pinned to a second
derivation.  (tests/test_plan_table.py already pins the plan of every committed cfg without the key.)"""
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import hip, darknet_io as IO

FIXTURES = ("mini_grouped.npz", "mini_dw_v3.npz")
INVALID, UNSUPPORTED = -1, -6          # YOLO_ERR_INVALID, YOLO_ERR_UNSUPPORTED (include/yolo_hip.h)
ACTS = {"linear": lambda v: v, "leaky": lambda v: np.where(v > 0, v, 0.1 * v), "relu": lambda v: np.maximum(v, 0), "tanh": np.tanh}


# ---- the restatement shared with test_gpu_grouped.py ----
def gconv_ref(x, w_oihw, bias, groups, stride, pad):
    """DN/convolutional_layer.c:458-471 in float64: group g reads the input channels g * cg .., its m filters write the output channels
    g * m ..; x [n, h, w, cin], w [cout, cin / groups, k, k] -> [n, (h + 2p - k) // s + 1, (w + 2p - k) // s + 1, cout]"""
    x = np.asarray(x, dtype=np.float64); w = np.asarray(w_oihw, dtype=np.float64)
    n, h, wd, cin = x.shape; cout, cg, k = w.shape[0], w.shape[1], w.shape[2]
    assert cin == cg * groups and cout % groups == 0
    m = cout // groups
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    xp = np.zeros((n, h + 2 * pad, wd + 2 * pad, cin)); xp[:, pad:pad + h, pad:pad + wd] = x
    out = np.zeros((n, ho, wo, cout))
    for g in range(groups):
        for ky in range(k):
            for kx in range(k):
                win = xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride, g * cg:(g + 1) * cg]
                out[..., g * m:(g + 1) * m] += win @ w[g * m:(g + 1) * m, :, ky, kx].T
    return out + (0 if bias is None else np.asarray(bias, dtype=np.float64))


def taps_inside(h, w, k, stride, pad):
    """how many taps of a k x k window lie inside the image, per output pixel: [ho, wo]"""
    return gconv_ref(np.ones((1, h, w, 1)), np.ones((1, 1, k, k)), None, 1, stride, pad)[0, :, :, 0]


def layer_params(secs, flat):
    """layer index -> (params [filters] or [4][filters], filters [cout][cin / groups][k][k]) of every [convolutional] section of the stream"""
    out, p = {}, 0
    for c in IO.conv_specs(secs):
        nb = c["filters"] * (4 if c["bn"] else 1)
        nw = c["filters"] * (c["cin"] // c["groups"]) * c["size"] ** 2
        out[c["index"]] = (flat[p:p + nb].reshape(-1, c["filters"]), flat[p + nb:p + nb + nw].reshape(c["filters"], c["cin"] // c["groups"], c["size"], c["size"]))
        p += nb + nw
    assert p == flat.size
    return out


def darknet_formula(secs):
    """sum over the [convolutional] sections of l.nweights + biases (+ three batch-norm vectors), from the section's own keys"""
    shapes, n = IO.layer_shapes(secs), 0
    for i, s in enumerate(secs[1:]):
        if s["type"] == "convolutional":
            f, k, g = int(s["filters"]), int(s["size"]), int(s.get("groups", 1))
            n += f * (4 if int(s.get("batch_normalize", 0)) else 1) + f * (shapes[i][4] // g) * k * k
    return n


def _refused(cfg, code, *needles, dtype=hip.BF16):
    rc, msg = hip.plan_check(cfg, dtype=dtype)
    assert rc == code, (rc, msg)
    for n in needles:
        assert n in msg, (n, msg)
    return msg


def _cfgs():
    return [str(golden(n)["cfg"]) for n in FIXTURES] + [IO.cfg_text("resnext50")]


# ---- counts ----
def test_weight_counts_follow_darknets_formula():
    for cfg in _cfgs():
        secs = IO.parse_cfg(cfg)
        assert IO.weights_count(secs) == darknet_formula(secs)
        for c in IO.conv_specs(secs):
            s = secs[1 + c["index"]]
            assert c["groups"] == int(s.get("groups", 1)) and c["cin"] % c["groups"] == 0 and c["filters"] % c["groups"] == 0
    for name in FIXTURES:
        g = golden(name)
        assert g["weights"].size == IO.weights_count(IO.parse_cfg(str(g["cfg"])))


def test_resnext50_layer_list_and_total():
    """the 7x7/2 stem, 3-4-6-3 bottlenecks of 1x1 / 3x3 groups=32 / 1x1 at widths 128/256 .. 1024/2048, a 1x1 conv to 1000: the stream's
    length summed here from that list"""
    secs = IO.parse_cfg(IO.cfg_text("resnext50"))
    convs = IO.conv_specs(secs)
    total, cin, k = 64 * 4 + 64 * 3 * 49, 64, 1
    assert (convs[0]["filters"], convs[0]["size"], convs[0]["groups"]) == (64, 7, 1)
    for stage, blocks in enumerate((3, 4, 6, 3)):
        f = 128 << stage
        for _ in range(blocks):
            for filters, size, groups in ((f, 1, 1), (f, 3, 32), (2 * f, 1, 1)):
                c = convs[k]; k += 1
                assert (c["filters"], c["size"], c["groups"], c["cin"], c["bn"]) == (filters, size, groups, cin, 1)
                total += filters * 4 + filters * (cin // groups) * size * size
                cin = filters
    assert (convs[k]["filters"], convs[k]["size"], convs[k]["cin"], convs[k]["bn"]) == (1000, 1, 2048, 0) and k + 1 == len(convs)
    total += 1000 + 1000 * 2048
    assert IO.weights_count(secs) == total
    assert [s["type"] for s in secs[-2:]] == ["avgpool", "softmax"]
    assert IO.synth_weights(secs, seed=0).size == total


def test_synth_weights_unchanged_without_the_key():
    """fan-in c / groups leaves the stream of a cfg without the key as it was: digests recorded from the commit before groups= was read"""
    import hashlib
    for name, stats, want in (("yolov3-tiny", "benign", "70a146a4dcc2bd9f"), ("yolov3-tiny", "log", "acad8b6221b8a44f"), ("resnet18", "benign", "5e821150c7dea129")):
        secs = IO.parse_cfg(IO.cfg_text(name))
        assert all(c["groups"] == 1 for c in IO.conv_specs(secs))
        flat = IO.synth_weights(secs, seed=3, stats=stats)
        assert hashlib.sha256(np.asarray(flat, np.float32).tobytes()).hexdigest()[:16] == want, (name, stats)
    # and with the key: the log-statistics stream of a grouped cfg has the right length too
    secs = IO.parse_cfg(str(golden("mini_dw_v3.npz")["cfg"]))
    assert IO.synth_weights(secs, seed=3, stats="log").size == IO.weights_count(secs)


# ---- the planner ----
@pytest.mark.parametrize("dtype", [hip.FP32, hip.BF16, hip.FP16])
def test_grouped_cfgs_plan(dtype):
    for cfg in _cfgs():
        rc, msg = hip.plan_check(cfg, dtype=dtype)
        assert rc == 0, msg


def test_grouped_layers_print_as_their_own_kind():
    rc, text = hip.plan_table(str(golden("mini_grouped.npz")["cfg"]))
    assert rc == 0
    rows = text.splitlines()
    for i in (3, 7, 10, 12, 13, 15):
        assert rows[i].startswith("%d convolutional kernel=- fused=none launcher=-1 residual_from=-2 tail_layer=-1 " % i), rows[i]
    assert rows[2].startswith("2 convolutional kernel=tiled ")
    # the two grouped convs the [route] concatenates write windows of its buffer
    st = lambda row: next(v for v in row.split() if v.startswith("storage="))
    assert st(rows[12]) == st(rows[13]) == st(rows[14])


def test_refusals_name_the_layer():
    mini = str(golden("mini_grouped.npz")["cfg"]); dw = str(golden("mini_dw_v3.npz")["cfg"])
    msgs = [_refused(mini, UNSUPPORTED, "layer 3", "groups=4", "fp8", dtype=hip.FP8),
            _refused(mini, UNSUPPORTED, "layer 3", "groups=4", "split-fp16", dtype=hip.FP16X2),
            _refused(dw, UNSUPPORTED, "layer 1", "groups=8", "fp8", dtype=hip.FP8),
            _refused(IO.cfg_text("resnext50"), UNSUPPORTED, "layer 3", "groups=32", "split-fp16", dtype=hip.FP16X2)]
    net = "[net]\nwidth=16\nheight=16\nchannels=3\n\n"
    conv = "[convolutional]\nfilters=%d\nsize=%d\nstride=%d\npad=1\ngroups=%d\nactivation=leaky\n\n"
    dense = "[convolutional]\nfilters=%d\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"
    tail = "[convolutional]\nfilters=8\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n"
    head = "[yolo]\nmask=0\nanchors=10,14\nclasses=1\nnum=1\n"
    rc, msg = hip.plan_check(net + dense % 12 + conv % (20, 3, 1, 4) + tail)
    assert rc == 0, msg
    msgs.append(_refused(net + dense % 12 + conv % (20, 3, 1, 8) + tail, INVALID, "layer 1", "groups=8", "12 input channels"))
    msgs.append(_refused(net + dense % 12 + conv % (20, 3, 1, 3) + tail, INVALID, "layer 1", "groups=3", "filters=20"))
    msgs.append(_refused(net + dense % 12 + conv % (20, 3, 1, 0) + tail, INVALID, "layer 1", "groups=0"))
    msgs.append(_refused(net + dense % 12 + conv % (20, 3, 1, -2) + tail, INVALID, "layer 1", "groups=-2"))
    msgs.append(_refused(net + conv % (6, 3, 1, 3) + tail, UNSUPPORTED, "layer 0", "groups=3", "first layer"))
    msgs.append(_refused(net + dense % 12 + conv % (6, 1, 1, 2) + head, UNSUPPORTED, "layer 1", "groups=2", "[yolo]"))
    msgs.append(_refused(net + dense % 12 + conv % (12, 3, 1, 4) + "[detection]\nclasses=1\nnum=1\nside=2\n", UNSUPPORTED, "layer 1", "groups=4", "[detection]"))
    msgs.append(_refused(net + dense % 12 + conv % (12, 3, 5, 4) + tail, UNSUPPORTED, "layer 1", "stride 5"))
    msgs.append(_refused(net + dense % 12 + conv % (12, 9, 1, 4) + tail, UNSUPPORTED, "layer 1", "size 9"))
    assert len(set(msgs)) == len(msgs), msgs
    with pytest.raises(hip.YoloError, match="divide"):            # refused before a device is touched
        hip.op_conv2d_grouped(np.zeros((1, 4, 4, 12), np.float32), np.zeros((6, 3, 3, 3), np.float32), groups=4)
    with pytest.raises(hip.YoloError, match="fp8 and split-fp16"):
        hip.op_conv2d_grouped(np.zeros((1, 4, 4, 8), np.float32), np.zeros((8, 4, 3, 3), np.float32), groups=2, dtype=hip.FP8)
    with pytest.raises(hip.YoloError, match="served are"):
        hip.op_conv2d_grouped(np.zeros((1, 4, 4, 8), np.float32), np.zeros((8, 4, 3, 3), np.float32), groups=2, stride=5)


def test_groups_1_keeps_the_dense_plan():
    """groups=1 spelled out plans exactly as no key"""
    cfg = IO.cfg_text("yolov3-tiny")
    with_key = cfg.replace("[convolutional]\n", "[convolutional]\ngroups=1\n")
    assert with_key != cfg
    assert hip.plan_table(with_key, max_batch=4) == hip.plan_table(cfg, max_batch=4)


# ---- the fixture against a second derivation ----
def test_restatement_reproduces_every_grouped_layer_of_the_fixture():
    """each grouped layer of mini_grouped.npz from its producer's STORED output: float64 grouped conv, darknet's batch norm
    ((x - mean) / (sqrt(var) + 1e-6) * gamma + beta), the activation -- within 5e-4 of the layer's scale"""
    g = golden("mini_grouped.npz")
    secs = IO.parse_cfg(str(g["cfg"]))
    params = layer_params(secs, g["weights"])
    seen = []
    for i, s in enumerate(secs[1:]):
        if s["type"] != "convolutional" or int(s.get("groups", 1)) == 1:
            continue
        prm, w = params[i]
        k, st, groups = int(s["size"]), int(s["stride"]), int(s["groups"])
        y = gconv_ref(g["layer_%02d" % (i - 1)], w, None, groups, st, k // 2)
        if int(s.get("batch_normalize", 0)):
            beta, gamma, mean, var = prm.astype(np.float64)
            y = (y - mean) / (np.sqrt(var) + 1e-6) * gamma + beta
        else:
            y = y + prm[0].astype(np.float64)
        y = ACTS[s["activation"]](y)
        ref = g["layer_%02d" % i]
        assert y.shape == ref.shape
        err = float(np.abs(y - ref).max() / np.abs(ref).max())
        assert err < 5e-4, "layer %d (groups=%d): %.3e" % (i, groups, err)
        seen.append((k, st, groups))
    assert seen == [(3, 1, 4), (3, 2, 8), (3, 1, 64), (3, 2, 32), (5, 1, 2), (1, 1, 2)]
    # the fixture's own claims
    pooled = g["layer_%02d" % (len(secs) - 3)]
    assert float(np.abs(g["layer_%02d" % int(g["logit_layer"])]).max()) > 4.5
    top2 = np.sort(pooled, axis=-1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) > 2 * 3e-2 * np.abs(pooled).max()).all()
