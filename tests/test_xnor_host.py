"""[convolutional] with xnor=1 (XNOR-Net layers), host side (no device): the float64 restatement the GPU tests (test_gpu_xnor.py) compare the
device against, tied here to the compiled reference's recorded layers (tests/golden/mini_xnor.npz, xnor_layer_cases.npz, written by
tools/make_golden.py --xnor) under a derived bound; alpha_f bit for bit; the condition of the fixtures that makes an end-to-end comparison
meaningful; and the planner: an L_XCONV row, each refusal with its status and a message that names the layer, and unchanged plans for
cfgs without the key and for binary=1 alone."""
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import hip, darknet_io as IO

FIXTURES = ("mini_xnor.npz", "xnor_layer_cases.npz")
INVALID, UNSUPPORTED = -1, -6          # YOLO_ERR_INVALID, YOLO_ERR_UNSUPPORTED (include/yolo_hip.h)
L_XCONV = 20                           # LType (yolo_ctx.h) as yolo_plan_dump prints it
MARGIN_TOL = 5e-4                      # the fp32 bound of the network tests, as a share of the tensor's largest value
ACTS = {"linear": lambda v: v, "leaky": lambda v: np.where(v > 0, v, np.float64(np.float32(0.1)) * v), "relu": lambda v: np.maximum(v, 0), "tanh": np.tanh,
        "logistic": lambda v: 1.0 / (1.0 + np.exp(-v))}


# ---- the restatement shared with test_gpu_xnor.py ----
def xnor_alpha(w_oihw):
    """binarize_weights' magnitude per filter (DN/convolutional_layer.c:28-41), mean |w_f| in float32, in the order the reference's build adds: the
    source reads as a running sum in index order and one division, but under -Ofast (the reference's own OPTS) the compiler keeps four partial
    sums (element j in sum j % 4), adds them as (s0 + s2) + (s1 + s3), then the elements past the last whole four in order, and multiplies by the
    float32 reciprocal of the count.  Measured on the fixtures' 128 filters: this order matches every one bit for bit; the plain running sum with
    a division differs by 1 .. 9 ulp in most of them (test_alpha_matches_the_references_bit_for_bit prints both counts)"""
    w = np.abs(np.asarray(w_oihw, dtype=np.float32).reshape(w_oihw.shape[0], -1))
    n = w.shape[1]; whole = n // 4 * 4
    lane = np.zeros((w.shape[0], 4), np.float32)
    for j in range(0, whole, 4):
        lane = lane + w[:, j:j + 4]          # (float32 + float32: one rounding each)
    s = (lane[:, 0] + lane[:, 2]) + (lane[:, 1] + lane[:, 3])
    for j in range(whole, n):
        s = s + w[:, j]
    assert s.dtype == np.float32
    return s * (np.float32(1) / np.float32(n))


def running_sum_alpha(w_oihw):
    """the source's order taken literally: a float32 running sum in index order, one float32 division (not what the reference's build gives)"""
    w = np.abs(np.asarray(w_oihw, dtype=np.float32).reshape(w_oihw.shape[0], -1))
    return np.cumsum(w, axis=1, dtype=np.float32)[:, -1] / np.float32(w.shape[1])


def sign_sums(x, w_oihw, stride, pad):
    """the integer part: sum over the taps inside the image and the channels of sign(x) * sign(w), signs +1 where > 0 else -1 (so +0, -0 and
    NaN give -1); taps outside the image contribute 0 (im2col pads after the binarisation).  [n, ho, wo, cout] float64, exact"""
    x = np.asarray(x); w = np.asarray(w_oihw)
    n, h, wd, cin = x.shape; cout, k = w.shape[0], w.shape[2]
    assert w.shape[1] == cin
    xs = np.where(x > 0, 1.0, -1.0); ws = np.where(w > 0, 1.0, -1.0)
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    xp = np.zeros((n, h + 2 * pad, wd + 2 * pad, cin)); xp[:, pad:pad + h, pad:pad + wd] = xs
    out = np.zeros((n, ho, wo, cout))
    for ky in range(k):
        for kx in range(k):
            out += xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride] @ ws[:, :, ky, kx].T
    return out


def xnor_ref(x, w_oihw, b_or_bn, stride, pad, act="linear"):
    """DN/convolutional_layer.c:451-485 with l.xnor, in float64: (1) alpha_f = mean |w_f| as xnor_alpha forms it, the filters +-alpha_f; (2) the
    input +-1; (3) the convolution of the two, zero outside the image; (4) b_or_bn None: nothing, [cout]: a bias, [4][cout] (beta, gamma,
    rolling mean, rolling variance): darknet's batch norm (x - mean) / (sqrt(var) + 1e-6) * gamma + beta; then the activation"""
    y = sign_sums(x, w_oihw, stride, pad) * xnor_alpha(w_oihw).astype(np.float64)
    if b_or_bn is not None:
        p = np.asarray(b_or_bn, dtype=np.float64)
        if p.ndim == 2 and p.shape[0] == 4:
            beta, gamma, mean, var = p
            y = (y - mean) / (np.sqrt(var) + 1e-6) * gamma + beta
        else:
            y = y + p.reshape(-1)
    return ACTS[act](y)


def taps_inside(h, w, k, stride, pad):
    """how many taps of a k x k window lie inside the image, per output pixel: [ho, wo]"""
    return sign_sums(np.ones((1, h, w, 1)), np.ones((1, 1, k, k)), stride, pad)[0, :, :, 0]


def layer_params(secs, flat):
    """layer index -> (params [1][filters] or [4][filters], filters [cout][cin][k][k]) of every [convolutional] section of the stream"""
    out, p = {}, 0
    for c in IO.conv_specs(secs):
        nb, nw = c["filters"] * (4 if c["bn"] else 1), c["filters"] * c["cin"] * c["size"] ** 2
        out[c["index"]] = (flat[p:p + nb].reshape(-1, c["filters"]), flat[p + nb:p + nb + nw].reshape(c["filters"], c["cin"], c["size"], c["size"]))
        p += nb + nw
    assert p == flat.size
    return out


def conv_geometry(s):
    """(size, stride, padding) of a [convolutional] section as DN/parser.c reads them: pad=1 means size / 2, else padding= literally"""
    k = int(s.get("size", 1))
    return k, int(s.get("stride", 1)), (k // 2 if int(s.get("pad", 0)) else int(s.get("padding", 0)))


def xnor_layers(secs):
    return [i for i, s in enumerate(secs[1:]) if s["type"] == "convolutional" and int(s.get("xnor", 0))]


def restate_layer(secs, params, i, x):
    """layer i of the cfg from the tensor x that enters it"""
    s = secs[1 + i]; prm, w = params[i]; k, st, pad = conv_geometry(s)
    return xnor_ref(x, w, prm if prm.shape[0] == 4 else prm[0], st, pad, s.get("activation", "logistic"))


# ---- the fixtures against the restatement ----
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_every_xnor_layer_of_the_reference(name):
    """The restatement applied to the reference's own recorded input of every xnor layer reproduces its recorded output.

    The bound, per filter f with K = cin * size^2 terms: the reference's gemm adds K terms of magnitude alpha_f in fp32; every partial sum is at
    most K * alpha_f, so every addition errs by at most 2^-24 * K * alpha_f and the K of them by K * 2^-24 * K * alpha_f.  Batch norm multiplies that
    by |gamma / (sqrt(var) + 1e-6)| (its own four roundings are each 2^-24 of a value no larger than K * alpha_f * that factor: with K >= 8 they fit
    the slack of the first term, which counts every partial sum as the largest possible); the activations served have slope <= 1.  On top, the
    result's own rounding and the activation's: 2 ulp of the result."""
    g = golden(name)
    secs = IO.parse_cfg(str(g["cfg"]))
    params = layer_params(secs, g["weights"])
    seen = []
    for i in xnor_layers(secs):
        s = secs[1 + i]; prm, w = params[i]; k, st, pad = conv_geometry(s)
        K = w.shape[1] * k * k
        assert K >= 8
        y = restate_layer(secs, params, i, g["layer_%02d" % (i - 1)])
        ref = g["layer_%02d" % i]
        assert y.shape == ref.shape
        scale = np.abs(prm[1].astype(np.float64) / (np.sqrt(prm[3].astype(np.float64)) + 1e-6)) if prm.shape[0] == 4 else np.ones(w.shape[0])
        bound = K * 2.0 ** -24 * K * xnor_alpha(w).astype(np.float64) * scale + 2 * 2.0 ** -23 * np.abs(ref.astype(np.float64))
        err = np.abs(y - ref)
        print("%s layer %d (k %d s %d p %d, K %d, %s): max err / bound %.3f, max err %.3e" % (name, i, k, st, pad, K, s["activation"], float((err / bound).max()), float(err.max())))
        assert (err <= bound).all(), "layer %d: %g over" % (i, float((err - bound).max()))
        seen.append((k, st, pad, w.shape[1], w.shape[0], int(s.get("batch_normalize", 0)), s["activation"]))
    want = {"mini_xnor.npz": [(3, 1, 1, 8, 16, 1, "leaky"), (3, 1, 1, 16, 24, 1, "leaky"), (1, 1, 0, 24, 16, 1, "leaky")],
            "xnor_layer_cases.npz": [(3, 1, 1, 8, 12, 1, "leaky"), (5, 1, 1, 12, 20, 1, "leaky"), (3, 2, 1, 20, 16, 0, "leaky"), (1, 1, 0, 16, 24, 1, "tanh")]}
    assert seen == want[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_alpha_matches_the_references_bit_for_bit(name):
    """alpha_NN of the fixture is what the reference's own binarize_weights wrote for each filter"""
    g = golden(name)
    secs = IO.parse_cfg(str(g["cfg"]))
    params = layer_params(secs, g["weights"])
    for i in xnor_layers(secs):
        a = xnor_alpha(params[i][1]); ref = g["alpha_%02d" % i]
        assert a.dtype == np.float32 and ref.dtype == np.float32 and a.shape == ref.shape
        assert np.array_equal(a.view(np.uint32), ref.view(np.uint32)), "layer %d" % i
        r = running_sum_alpha(params[i][1])
        ulp = np.abs(r.view(np.int32).astype(np.int64) - ref.view(np.int32))
        print("%s layer %d: %d filters; the literal running sum differs in %d of them, by at most %d ulp" % (name, i, a.size, int((ulp > 0).sum()), int(ulp.max())))


@pytest.mark.parametrize("name", FIXTURES)
def test_no_input_of_an_xnor_layer_is_near_zero(name):
    """A condition of the fixture: in the reference's run no value entering an xnor layer is non-zero and within MARGIN_TOL * max|tensor| of
    zero, and none is an exact zero either (leaky in front of every xnor layer).  Without it an fp32 device run may legitimately flip a
    sign and the end-to-end comparison of test_gpu_xnor.py means nothing."""
    g = golden(name)
    secs = IO.parse_cfg(str(g["cfg"]))
    for i in xnor_layers(secs):
        x = np.abs(g["layer_%02d" % (i - 1)])
        assert not ((x > 0) & (x <= MARGIN_TOL * x.max())).any(), "layer %d" % i
        assert (x > 0).all(), "layer %d reads an exact zero" % i
        p = i - 1
        while secs[1 + p]["type"] == "maxpool":
            p -= 1
        assert secs[1 + p]["activation"] == "leaky"
    if "obj_raw" in g.files:          # ... and no candidate's objectness sits on the box threshold
        assert 3 <= len(g["obj_raw"]) <= 60 and g["obj_raw"].min() > float(g["thresh"]) * (1 + 1e-3)


def test_the_reference_binarised():
    """the recorded xnor layers are not what a full-precision conv of the same filters gives (the key was not ignored when the fixture was made)"""
    g = golden("mini_xnor.npz")
    secs = IO.parse_cfg(str(g["cfg"]))
    prm, w = layer_params(secs, g["weights"])[2]
    x = g["layer_01"].astype(np.float64)
    xp = np.zeros((1, 8, 8, 8)); xp[:, 1:7, 1:7] = x
    y = sum(xp[:, ky:ky + 6, kx:kx + 6] @ w[:, :, ky, kx].astype(np.float64).T for ky in range(3) for kx in range(3))
    beta, gamma, mean, var = prm.astype(np.float64)
    y = ACTS["leaky"]((y - mean) / (np.sqrt(var) + 1e-6) * gamma + beta)
    assert np.abs(y - g["layer_02"]).max() > 0.1 * np.abs(g["layer_02"]).max()


# ---- the planner ----
NET = "[net]\nwidth=16\nheight=16\nchannels=3\n\n"
DENSE = "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"
XNOR = "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=%d\nstride=%d\npad=1\nxnor=1\n%sactivation=leaky\n\n"
TAIL = "[convolutional]\nfilters=8\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n"


def _refused(cfg, code, *needles, dtype=hip.BF16):
    rc, msg = hip.plan_check(cfg, dtype=dtype)
    assert rc == code, (rc, msg)
    for n in needles:
        assert n in msg, (n, msg)
    return msg


@pytest.mark.parametrize("dtype", [hip.FP32, hip.BF16, hip.FP16])
def test_xnor_cfgs_plan_an_xconv_row(dtype):
    for name in FIXTURES:
        cfg = str(golden(name)["cfg"])
        secs = IO.parse_cfg(cfg)
        rc, dump = hip.plan_dump(cfg, dtype=dtype)
        assert rc == 0, dump
        rc, table = hip.plan_table(cfg, dtype=dtype)
        assert rc == 0, table
        rows, lines = table.splitlines(), dump.splitlines()
        for i, s in enumerate(secs[1:]):
            if s["type"] != "convolutional":
                continue
            if int(s.get("xnor", 0)):
                assert lines[i].startswith("layer %d convolutional type=%d " % (i, L_XCONV)), lines[i]
                assert rows[i].startswith("%d convolutional kernel=- fused=none launcher=-1 residual_from=-2 tail_layer=-1 " % i), rows[i]
            else:
                assert lines[i].startswith("layer %d convolutional type=0 " % i), lines[i]
                assert rows[i].startswith("%d convolutional kernel=tiled " % i) or " fused=" in rows[i], rows[i]
        # the same cfg without the key: dense convs throughout, and not the plan with it
        rc, plain = hip.plan_dump(cfg.replace("xnor=1\n", ""), dtype=dtype)
        assert rc == 0 and "type=%d " % L_XCONV not in plain and plain != dump


def test_refusals_name_the_layer():
    mini = str(golden("mini_xnor.npz")["cfg"])
    msgs = [_refused(mini, UNSUPPORTED, "layer 2", "xnor=1", "fp8", dtype=hip.FP8),
            _refused(mini, UNSUPPORTED, "layer 2", "xnor=1", "split-fp16", dtype=hip.FP16X2)]
    rc, msg = hip.plan_check(NET + DENSE % 12 + XNOR % (20, 3, 1, "") + TAIL)
    assert rc == 0, msg
    msgs.append(_refused(NET + DENSE % 12 + XNOR % (20, 3, 1, "groups=4\n") + TAIL, UNSUPPORTED, "layer 1", "xnor=1", "groups=4"))
    msgs.append(_refused(NET + XNOR % (8, 3, 1, "") + TAIL, UNSUPPORTED, "layer 0", "xnor=1", "first layer"))
    head = "[yolo]\nmask=0\nanchors=10,14\nclasses=1\nnum=1\n"
    xhead = "[convolutional]\nfilters=6\nsize=1\nstride=1\npad=1\nxnor=1\nactivation=linear\n\n"
    msgs.append(_refused(NET + DENSE % 12 + xhead + head, UNSUPPORTED, "layer 1", "xnor=1", "[yolo]"))
    msgs.append(_refused(NET + DENSE % 12 + xhead + "[region]\nanchors=1,1\nclasses=1\nnum=1\n", UNSUPPORTED, "layer 1", "xnor=1", "[region]"))
    msgs.append(_refused(NET + DENSE % 12 + XNOR % (12, 3, 1, "") + "[detection]\nclasses=1\nnum=1\nside=2\n", UNSUPPORTED, "layer 1", "xnor=1", "[detection]"))
    msgs.append(_refused(NET + DENSE % 12 + XNOR % (12, 13, 1, "") + TAIL, UNSUPPORTED, "layer 1", "size 13"))
    assert len(set(msgs)) == len(msgs), msgs
    with pytest.raises(hip.YoloError, match="fp8 and split-fp16"):          # refused before a device is touched
        hip.op_conv2d_xnor(np.zeros((1, 4, 4, 8), np.float32), np.zeros((8, 8, 3, 3), np.float32), dtype=hip.FP8)
    with pytest.raises(hip.YoloError, match="served are"):
        hip.op_conv2d_xnor(np.zeros((1, 4, 4, 8), np.float32), np.zeros((8, 8, 13, 13), np.float32), padding=6)
    with pytest.raises(hip.YoloError, match="filters must be"):
        hip.op_conv2d_xnor(np.zeros((1, 4, 4, 8), np.float32), np.zeros((8, 4, 3, 3), np.float32))


@pytest.mark.parametrize("key", ["xnor=0", "binary=1", "flipped=1"])
def test_cfgs_without_xnor_plan_as_before(key):
    """xnor=0 spelled out, binary=1 alone and flipped=1 are read by nobody: the plan is the plan of the cfg without the key, which
    tests/test_plan_dump.py pins"""
    for name in ("yolov3-tiny", "yolov2-tiny-voc"):
        cfg = IO.cfg_text(name)
        with_key = cfg.replace("[convolutional]\n", "[convolutional]\n%s\n" % key)
        assert with_key != cfg
        for dtype in (hip.BF16, hip.FP32, hip.FP8):
            assert hip.plan_dump(with_key, dtype=dtype, max_batch=4) == hip.plan_dump(cfg, dtype=dtype, max_batch=4)
            assert hip.plan_table(with_key, dtype=dtype, max_batch=4) == hip.plan_table(cfg, dtype=dtype, max_batch=4)


def test_weight_stream_is_a_convs():
    """xnor=1 changes nothing in the weight file: the same floats in the same order"""
    for name in FIXTURES:
        g = golden(name)
        cfg = str(g["cfg"])
        assert IO.weights_count(IO.parse_cfg(cfg)) == IO.weights_count(IO.parse_cfg(cfg.replace("xnor=1\n", ""))) == g["weights"].size
