"""The YOLOv1 family -- [local], [connected], [detection], the 7x7 / 2 first conv -- host side (no device): the float64 restatements of
[local] (DN/local_layer.c:91-120) and [connected] (DN/connected_layer.c:151-166, CHW flatten, batch norm) and the float32 restatement of the
[detection] rows (DN/detection_layer.c:225-254) that tests/test_gpu_v1_edges.py compares the device against, tied here to the compiled
reference's recorded layers: tests/golden/mini_v1_edges.npz and mini_v1_stem.npz (tools/make_golden.py v1_edges), mini_v1.npz and
mini_local.npz.  Also what the fixtures and the device-only networks of the GPU tests must have for those tests to mean anything (a
second pass of k_local's lane loop, a filter count that is no multiple of 4, a K that is no multiple of 64, ...), read from the cfg's
arithmetic and the planner's dump."""
import os
import sys
import numpy as np
import pytest
from conftest import golden
from oracle import darknet_ref as DR
from oracle import yolo_ref as R
from yolo_tensorflow_amd import hip, darknet_io as IO
from test_edges_host import conv_geometry, conv_ref, mover_ref
from test_gpu_resnet import act64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mini_v1_edges.npz", "mini_v1_stem.npz")
OLD = ("mini_v1.npz", "mini_local.npz")
DTYPES = {"fp32": hip.FP32, "bf16": hip.BF16, "fp16": hip.FP16}


# ---- restatements shared with test_gpu_v1_edges.py ----
def layer_params(cfg, flat):
    """{layer index: parameters} of every parameterised layer, from the flat stream in file order (DN/parser.c load_weights_upto):
    [convolutional]  bias or beta / gamma / mean / var, then w [k, k, cin, cout] (from the file's [cout][cin][k][k])
    [local]          bias [filter][location], w [location][filter][cin][kh][kw]
    [connected]      bias, w [output][input], then gamma / mean / var when batch-normalised"""
    secs = IO.parse_cfg(cfg); flat = np.asarray(flat, dtype=np.float32); out = {}; at = [0]

    def take(*shape):
        n = int(np.prod(shape)); v = flat[at[0]:at[0] + n].reshape(shape).copy(); at[0] += n
        return v
    for spec in IO.conv_specs(secs):
        i, n, k, cin = spec["index"], spec["filters"], spec["size"], spec["cin"]
        t = secs[1 + i]["type"]
        if t == "local":
            out[i] = dict(bias=take(n, spec["locations"]), w=take(spec["locations"], n, cin, k, k))
        elif t == "connected":
            p = dict(bias=take(n), w=take(n, cin))
            if spec["bn"]:
                p.update(gamma=take(n), mean=take(n), var=take(n))
            out[i] = p
        else:
            assert t == "convolutional" and spec.get("groups", 1) == 1
            p = {key: take(n) for key in (("beta", "gamma", "mean", "var") if spec["bn"] else ("bias",))}
            p["w"] = np.ascontiguousarray(take(n, cin, k, k).transpose(2, 3, 1, 0))
            out[i] = p
    assert at[0] == flat.size
    return out


def flatten_params(cfg, params):
    """layer_params backwards: the flat stream of {layer index: parameters}"""
    secs = IO.parse_cfg(cfg); parts = []
    for spec in IO.conv_specs(secs):
        p, t = params[spec["index"]], secs[1 + spec["index"]]["type"]
        if t == "local":
            parts += [p["bias"], p["w"]]
        elif t == "connected":
            parts += [p["bias"], p["w"]] + ([p["gamma"], p["mean"], p["var"]] if spec["bn"] else [])
        else:
            parts += [p[key] for key in (("beta", "gamma", "mean", "var") if spec["bn"] else ("bias",))] + [p["w"].transpose(3, 2, 0, 1)]
    return np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for a in parts])


def local_geometry(sec, h, w):
    """(size, stride, pad, Ho, Wo) of a [local] section over an h x w producer (DN/local_layer.c:10-24: `pad` is a flag for the output size
    and the amount for im2col)"""
    k, st, pad = int(sec["size"]), int(sec.get("stride", 1)), int(sec.get("pad", 0))
    return k, st, pad, ((h - 1) if pad else (h - k)) // st + 1, ((w - 1) if pad else (w - k)) // st + 1


def local64(sec, p, x):
    """[local] before its activation, float64: out[n, oy, ox, f] = bias[f][loc] + sum_{c, kh, kw} w[loc][f][c][kh][kw] x[n, oy s - p + kh, ox s - p + kw, c],
    loc = oy Wo + ox.  -> (y, mag): mag = bias's magnitude + sum |x w|, what the accumulation bound is taken of"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64); w = np.asarray(p["w"], dtype=np.float32).astype(np.float64)
    n, h, wd, c = x.shape
    k, st, pad, ho, wo = local_geometry(sec, h, wd)
    assert w.shape[0] == ho * wo and w.shape[2:] == (c, k, k)
    xp = np.pad(x, ((0, 0), (pad, pad + k), (pad, pad + k), (0, 0)))
    y = np.zeros((n, ho, wo, w.shape[1])); mag = np.zeros_like(y)
    for oy in range(ho):
        for ox in range(wo):
            loc = oy * wo + ox
            patch = xp[:, oy * st:oy * st + k, ox * st:ox * st + k, :]          # [n, kh, kw, c]
            wl = w[loc].transpose(0, 2, 3, 1)                                   # [f, kh, kw, c]
            b = np.asarray(p["bias"], dtype=np.float64)[:, loc]
            y[:, oy, ox] = np.einsum("nhwc,fhwc->nf", patch, wl) + b
            mag[:, oy, ox] = np.einsum("nhwc,fhwc->nf", np.abs(patch), np.abs(wl)) + np.abs(b)
    return y, mag


def connected_fold(p):
    """(w [output][input], bias) of a [connected] layer in float64 with its batch norm folded in as DN/connected_layer.c:161 applies it:
    (x - mean) / (sqrt(var) + .000001f) * gamma + bias, the scale evaluated in float32 as the reference's and the packer's C code do"""
    w = np.asarray(p["w"], dtype=np.float32).astype(np.float64); b = np.asarray(p["bias"], dtype=np.float32).astype(np.float64)
    if "gamma" not in p:
        return w, b
    s = (p["gamma"] / (np.sqrt(p["var"]) + np.float32(.000001))).astype(np.float32).astype(np.float64)
    return w * s[:, None], b - p["mean"].astype(np.float64) * s


def connected64(p, x, w=None, b=None):
    """[connected] before its activation, float64, over x [n, h, w, c] flattened CHW as darknet stores it: input index c * h * w + (y * w + x).
    -> (y [n, 1, 1, output], mag).  w / b: folded filters and bias to use instead of connected_fold(p) (pre-rounded to a storage type)"""
    if w is None:
        w, b = connected_fold(p)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    flat = np.ascontiguousarray(x.transpose(0, 3, 1, 2)).reshape(x.shape[0], -1)
    assert flat.shape[1] == w.shape[1]
    y = flat @ w.T + b
    mag = np.abs(flat) @ np.abs(w).T + np.abs(b)
    return y.reshape(x.shape[0], 1, 1, -1), mag.reshape(x.shape[0], 1, 1, -1)


def v1_rows32(pred, side, num, classes, sqrt):
    """oracle/yolo_ref.py: v1_rows for any (side, num, classes, sqrt), every step a float32 operation in the order of DN/detection_layer.c:225-254 (and of
    k_decode_v1), so that a bit comparison means something: [side^2 * num, 5 + classes] = (cx, cy, w, h, confidence, class scores)"""
    f = np.float32
    p = np.asarray(pred, dtype=f).reshape(-1)
    cells = side * side
    assert p.size == cells * (classes + 5 * num)
    cls = p[:cells * classes].reshape(cells, classes); conf = p[cells * classes:cells * (classes + num)].reshape(cells, num)
    box = p[cells * (classes + num):].reshape(cells, num, 4)
    col = (np.arange(cells) % side).astype(f)[:, None]; row = (np.arange(cells) // side).astype(f)[:, None]
    out = np.zeros((cells, num, 5 + classes), f)
    out[..., 0] = (box[..., 0] + col).astype(f) / f(side); out[..., 1] = (box[..., 1] + row).astype(f) / f(side)
    out[..., 2] = (box[..., 2] * box[..., 2]).astype(f) if sqrt else box[..., 2]
    out[..., 3] = (box[..., 3] * box[..., 3]).astype(f) if sqrt else box[..., 3]
    out[..., 4] = conf; out[..., 5:] = cls[:, None, :]
    return out.reshape(cells * num, 5 + classes)


def detection_of(sec):
    return int(sec.get("side", 7)), int(sec.get("num", 1)), int(sec.get("classes", 1)), int(sec.get("sqrt", 0))


def near_threshold(scores, thresh):
    """the (box, class) scores a comparison of `score > thresh` between two programs leaves out: within 1e-3 of the threshold"""
    return np.abs(np.asarray(scores, np.float32) - np.float32(thresh)) <= 1e-3


def fixture_input(name, g):
    """the float32 tensor the reference was handed, [n, h, w, 3]"""
    if "images_u8" in g.files:
        return g["images_u8"].astype(np.float32) / np.float32(255)
    x = g["image_u8"].astype(np.float32)[None] / np.float32(255)
    return x * np.float32(2) - np.float32(1) if name == "mini_v1.npz" else x


def layer_fields(dump, i):
    line = [ln for ln in dump.splitlines() if ln.startswith("layer %d " % i)][0]
    return dict(f.split("=", 1) for f in line.split()[3:])


def storage_fields(dump, k):
    line = [ln for ln in dump.splitlines() if ln.startswith("storage %d " % k)][0]
    return dict(f.split("=", 1) for f in line.split()[2:])


def local_k8(secs, i):
    """8-channel granules of one filter row of [local] layer i: what k_local's 64 lanes stride over"""
    sh = IO.layer_shapes(secs)[i]
    return int(secs[1 + i]["size"]) ** 2 * (-(-sh[4] // 8))


# ---- device-only networks of test_gpu_v1_edges.py, planned here on the CPU ----
def _net(h, w, c, planes=True):
    return "[net]\n%sbatch=1\nheight=%d\nwidth=%d\nchannels=%d\n\n" % ("yolo_input=planes\n" if planes else "", h, w, c)


def _local(filters, size, stride, pad, act="linear"):
    return "[local]\nsize=%d\nstride=%d\npad=%d\nfilters=%d\nactivation=%s\n\n" % (size, stride, pad, filters, act)


def _fc(output, act="linear", bn=False):
    return "[connected]\n%soutput=%d\nactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", output, act)


def _det(side, num, classes, sqrt):
    return "[detection]\nclasses=%d\ncoords=4\nrescore=1\nside=%d\nnum=%d\nsoftmax=0\nsqrt=%d\n" % (classes, side, num, sqrt)


# (c) 64 planes of 3 x 5 straight into a [local] of each geometry of mini_v1_edges' layers 3 / 5 / 6, then a 1x1 conv to 8 channels (which reads every stored
# channel of the [local] layer's pixel, the zero fill behind 13 filters included), a [connected] head and [detection]
LOCAL_FIRST = {"3x3_s1_p1_f13": (13, 3, 1, 1), "3x3_s2_p1_f8": (8, 3, 2, 1), "2x2_s1_p0_f24": (24, 2, 1, 0)}


def local_first_cfg(key):
    f, k, st, pad = LOCAL_FIRST[key]
    return _net(3, 5, 64) + _local(f, k, st, pad) + "[convolutional]\nfilters=8\nsize=1\nstride=1\npad=0\nactivation=linear\n\n" + _fc(7) + _det(1, 1, 2, 1)


# (c) the plan that pools its buffers (keep_layers=False): a [local] of 16 filters that nothing reads, then a [local] of 13 filters over the same producer.
# The second takes over the first one's buffer (asserted from the dump), so within ONE forward its channels 13 .. 15 hold what the first left there
def _conv1(filters):
    return "[convolutional]\nfilters=%d\nsize=1\nstride=1\npad=0\nactivation=linear\n\n" % filters


RECYCLED = _net(3, 5, 64) + _conv1(64) + _local(16, 3, 1, 1) + "[route]\nlayers=0\n\n" + _local(13, 3, 1, 1) + _conv1(8) + _fc(7) + _det(1, 1, 2, 1)


def recycled_buffers(dump):
    """(the physical buffer of the 16-filter [local] layer, that of the 13-filter one, its pixel stride) from a dump of RECYCLED"""
    s1 = storage_fields(dump, int(layer_fields(dump, 1)["storage"])); s3 = storage_fields(dump, int(layer_fields(dump, 3)["storage"]))
    return int(s1["phys"]), int(s3["phys"]), int(s3["stride"])


# (c) 72 planes of 6 x 10 straight into a batch-normalised [connected] of 264 outputs, then 37, 5 and [softmax]
FC_FIRST = _net(6, 10, 72) + _fc(264, bn=True) + _fc(37) + _fc(5) + "[softmax]\ngroups=1\n"


# (d) conv -> 16, [local] 8 over it, [route] of both, a 1x1 [local] over the 24-channel concatenation, [connected], [detection]; and the same without the
# first [local] (the route names the conv alone), whose conv output must be what the concatenation's second window holds
def window_cfg(with_local=True):
    conv = "[convolutional]\nfilters=16\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"
    if not with_local:
        return _net(4, 6, 3, planes=False) + conv + _local(8, 1, 1, 0, "leaky") + _fc(7) + _det(1, 1, 2, 1)
    return (_net(4, 6, 3, planes=False) + conv + _local(8, 3, 1, 1, "leaky") + "[route]\nlayers=-1,-2\n\n" + _local(8, 1, 1, 0, "leaky") + _fc(7) + _det(1, 1, 2, 1))


# (e) [detection] heads behind a linear [connected] over 8 planes of 1 x 1: (side, num, classes, sqrt)
HEADS = [(1, 1, 1, 0), (2, 3, 2, 0), (5, 3, 2, 1), (3, 2, 20, 1)]


def head_cfg(side, num, classes, sqrt):
    return _net(1, 1, 8) + _fc(side * side * (classes + 5 * num)) + _det(side, num, classes, sqrt)


# (f) the 7x7 / 2 / pad 3 first conv alone: a map network
STEM_SIZES = [(2, 2), (4, 6), (10, 14), (6, 30)]


def stem_cfg(h, w, filters=20):
    return "[net]\nbatch=1\nheight=%d\nwidth=%d\nchannels=3\nyolo_output=map\n\n[convolutional]\nfilters=%d\nsize=7\nstride=2\npad=1\nactivation=linear\n" % (h, w, filters)


# ---- the fixtures are what the issue's table says ----
def test_fixtures_have_the_edges():
    g = golden("mini_v1_edges.npz"); cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg); shapes = IO.layer_shapes(secs); L = secs[1:]
    assert (int(secs[0]["height"]), int(secs[0]["width"])) == (6, 10) and g["images_u8"].shape == (3, 6, 10, 3)
    assert [s["type"] for s in L] == ["convolutional", "convolutional", "maxpool", "local", "convolutional", "local", "local", "connected", "connected", "detection"]
    assert [sh[1:4] for sh in shapes[:9]] == [(6, 10, 64), (6, 10, 64), (3, 5, 64), (3, 5, 13), (3, 5, 16), (2, 3, 8), (1, 2, 24), (1, 1, 37), (1, 1, 68)]
    # layer 3: a ragged second pass of the 64 lanes, a rectangular location grid, one real filter in the last workgroup of four waves
    assert local_k8(secs, 3) == 72 and 64 < 72 < 128 and shapes[3][1] != shapes[3][2] and int(L[3]["filters"]) % 4 == 1
    assert (int(L[5]["stride"]), int(L[5]["pad"]), L[5]["activation"]) == (2, 1, "relu")
    assert (int(L[6]["size"]), int(L[6]["pad"]), L[6]["activation"]) == (2, 0, "tanh")
    assert "activation" not in L[7] and shapes[7][4] == 48 and shapes[7][4] % 64 and int(L[7]["output"]) % 8
    assert detection_of(L[9]) == (2, 3, 2, 0) and int(L[8]["output"]) == 2 * 2 * (2 + 3 * 5)
    # the reference's workspace: every [local]'s im2col buffer (sized in elements, used in floats) fits in layer 1's
    ws1 = 60 * 9 * 64 * 4
    for i in (3, 5, 6):
        assert shapes[i][1] * shapes[i][2] * int(L[i]["size"]) ** 2 * shapes[i][4] * 4 < ws1
    g2 = golden("mini_v1_stem.npz"); secs2 = IO.parse_cfg(str(g2["cfg"])); sh2 = IO.layer_shapes(secs2)
    assert g2["images_u8"].shape == (3, 10, 14, 3) and conv_geometry(secs2[1]) == (7, 2, 3)
    assert sh2[0][1:4] == (5, 7, 20) and sh2[0][1] % 2 and sh2[0][2] % 2 and sh2[2][4] == 280 and 280 % 64
    assert detection_of(secs2[4]) == (1, 1, 2, 1)
    for name in NEW:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) < 974396
        gg = golden(name); n = len(IO.parse_cfg(str(gg["cfg"]))) - 1
        for i in range(n):
            assert gg["layer_%02d" % i].shape[0] == 3 and np.isfinite(gg["layer_%02d" % i]).all()
        # the three images differ, and so do their heads
        assert not np.array_equal(gg["layer_%02d" % (n - 1)][0], gg["layer_%02d" % (n - 1)][1])
        side, num, classes, sqrt = detection_of(IO.parse_cfg(str(gg["cfg"]))[-1])
        rows = np.stack([v1_rows32(h, side, num, classes, sqrt) for h in gg["layer_%02d" % (n - 1)]])
        pr = rows[..., 4:5] * rows[..., 5:]
        assert pr.shape == gg["prob_raw"].shape and near_threshold(pr, gg["thresh"]).sum() * 20 <= pr.size      # the GPU test's exclusion is a cap: 5 % of the (box, class) pairs


# ---- the restatements against the reference's recorded layers ----
@pytest.mark.parametrize("name", NEW + OLD)
def test_restatements_reproduce_every_recorded_layer(name):
    """every layer of the fixture on the fixture's own recorded input of that layer, float64 rounded once to float32, within the fp32 bound these fixtures
    have in test_oracle_golden.py (4e-6 of max(1, the tensor's scale): summation order between two programs); [detection] copies its input"""
    g = golden(name); cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    params = layer_params(cfg, g["weights"])
    x0 = fixture_input(name, g); n = x0.shape[0]
    shapes = IO.layer_shapes(IO.parse_cfg(cfg))
    rec = lambda j: x0 if j < 0 else g["layer_%02d" % j].reshape((n,) + tuple(shapes[j][1:4]))
    seen = set()
    for i, s in enumerate(secs):
        x, t = rec(i - 1), s["type"]
        want = g["layer_%02d" % i].reshape(n, -1)
        if t == "convolutional":
            got = conv_ref(s, params[i], x)
        elif t == "maxpool":
            got = mover_ref(s, i, [x])
        elif t in ("dropout", "detection"):
            got = x
        elif t == "local":
            got = act64(s.get("activation", "logistic"), local64(s, params[i], x)[0].astype(np.float32))
        elif t == "connected":
            got = act64(s.get("activation", "logistic"), connected64(params[i], x)[0].astype(np.float32))
        else:
            raise AssertionError(t)
        got = np.asarray(got, dtype=np.float32).reshape(n, -1)
        assert got.shape == want.shape, "layer %d (%s)" % (i, t)
        err = float(np.abs(got - want).max()); scale = max(1.0, float(np.abs(want).max()))
        print("%s layer %d (%s): max err %.3e of scale %.3f" % (name, i, t, err, scale))
        assert err <= 4e-6 * scale, "layer %d (%s)" % (i, t)
        seen.add((t, s.get("activation", "logistic")) if t in ("local", "connected") else t)
    if name == "mini_v1_edges.npz":
        assert {("local", "leaky"), ("local", "relu"), ("local", "tanh"), ("connected", "logistic"), ("connected", "linear")} <= seen


@pytest.mark.parametrize("name", NEW + OLD)
def test_row_restatement_reproduces_the_reference_boxes(name):
    """v1_rows32 on the recorded [detection] input == get_network_boxes -> get_detection_detections of the reference (boxes in network pixels: x and w times
    the width, y and h times the height), under the bounds of test_v1_restatement_matches_compiled_reference; equal to oracle/yolo_ref.py: v1_rows"""
    g = golden(name); secs = IO.parse_cfg(str(g["cfg"])); n = len(secs) - 1
    side, num, classes, sqrt = detection_of(secs[-1])
    H, W = np.float32(secs[0]["height"]), np.float32(secs[0]["width"])
    heads = g["layer_%02d" % (n - 1)].reshape(-1, side * side * (classes + 5 * num))
    many = "images_u8" in g.files
    for b in range(heads.shape[0]):
        rows = v1_rows32(heads[b], side, num, classes, sqrt)
        assert np.array_equal(rows, R.v1_rows(heads[b], side, num, classes, sqr=bool(sqrt)))
        bb, obj, pr = (g[k][b] if many else g[k] for k in ("boxes_raw", "obj_raw", "prob_raw"))
        if name == "mini_local.npz":
            bb, pr = bb[:, :4], pr[:, :classes]
        assert rows.shape == (len(obj), 5 + classes)
        np.testing.assert_allclose(rows[:, :4] * np.array([W, H, W, H], np.float32), bb, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(rows[:, 4], obj, rtol=1e-6, atol=1e-7)
        sc = rows[:, 4:5] * rows[:, 5:]
        np.testing.assert_allclose(np.where(sc > g["thresh"], sc, 0), pr, rtol=1e-5, atol=1e-6)


def test_row_restatement_edges():
    """sqrt=0 leaves w and h alone (negative ones too), num=3 orders the boxes inside the cell, side=1 has column and row 0"""
    rng = np.random.default_rng(5)
    p = rng.standard_normal(1 * (2 + 5 * 3)).astype(np.float32)
    rows = v1_rows32(p, 1, 3, 2, 0)
    assert np.array_equal(rows[:, :4], p[5:].reshape(3, 4)) and np.array_equal(rows[:, 4], p[2:5]) and np.array_equal(rows[:, 5:], np.broadcast_to(p[:2], (3, 2)))
    rows = v1_rows32(p, 1, 3, 2, 1)
    assert np.array_equal(rows[:, 2:4], p[5:].reshape(3, 4)[:, 2:] ** 2) and (rows[:, 2:4] >= 0).all()
    q = rng.standard_normal(4 * (2 + 5 * 3)).astype(np.float32)
    rows = v1_rows32(q, 2, 3, 2, 0).reshape(4, 3, 7)
    assert np.array_equal(rows[3, 1, 0], (q[20 + (3 * 3 + 1) * 4] + np.float32(1)) / np.float32(2)) and np.array_equal(rows[2, 0, 1], (q[20 + (2 * 3) * 4 + 1] + np.float32(1)) / np.float32(2))


# ---- the planner ----
@pytest.mark.parametrize("dname", sorted(DTYPES))
def test_plans_show_what_the_tests_rely_on(dname):
    dt = DTYPES[dname]
    tanh, logistic = hip.activation_code("tanh"), hip.activation_code("logistic")
    rc, dump = hip.plan_dump(str(golden("mini_v1_edges.npz")["cfg"]), dt, 3, True)
    assert rc == 0, dump
    f = [layer_fields(dump, i) for i in range(10)]
    assert [f[i]["post_act"] for i in (3, 5, 6)] == ["0", "0", str(tanh)] and f[3]["cin"] == "64" and f[3]["C"] == "13"
    assert (f[7]["fc"], f[7]["fc_h"], f[7]["fc_w"], f[7]["fc_c"], f[7]["cin"], f[7]["kpad"], f[7]["post_act"]) == ("1", "1", "2", "24", "48", "64", str(logistic))
    assert (f[8]["fc_h"], f[8]["fc_w"], f[8]["cin"], f[8]["cin_pad"], f[8]["head"], f[8]["post_act"]) == ("1", "1", "37", "40", "1", "0")
    assert (f[9]["side"], f[9]["na"], f[9]["classes"], f[9]["sqr"]) == ("2", "3", "2", "0")
    assert storage_fields(dump, int(f[3]["storage"]))["stride"] == "16"          # 13 filters stored in two granules: channels 13 .. 15 are k_local's zero fill
    rc, dump = hip.plan_dump(str(golden("mini_v1_stem.npz")["cfg"]), dt, 3, True)
    assert rc == 0, dump
    f = [layer_fields(dump, i) for i in range(4)]
    assert (f[0]["s2d7"], f[0]["H"], f[0]["W"], f[0]["C"], f[0]["cin_pad"], f[0]["kpad"]) == ("1", "5", "7", "20", "32", "512")
    assert (f[2]["fc_h"], f[2]["fc_w"], f[2]["fc_c"], f[2]["cin"], f[2]["kpad"]) == ("5", "7", "8", "280", "320") and 280 % 64
    assert (f[3]["side"], f[3]["na"], f[3]["sqr"]) == ("1", "1", "1")
    # the device-only networks
    for key, (nf, k, st, pad) in LOCAL_FIRST.items():
        cfg = local_first_cfg(key); rc, dump = hip.plan_dump(cfg, dt, 3, True)
        assert rc == 0, dump
        f0 = layer_fields(dump, 0)
        assert f0["in"] == "[-1]" and f0["cin"] == "64" and local_k8(IO.parse_cfg(cfg), 0) == k * k * 8
    assert local_k8(IO.parse_cfg(local_first_cfg("3x3_s1_p1_f13")), 0) == 72
    rc, dump = hip.plan_dump(RECYCLED, dt, 3, False)
    assert rc == 0, dump
    a, b, stride = recycled_buffers(dump)
    assert a == b and stride == 16 and layer_fields(dump, 3)["C"] == "13" and layer_fields(dump, 1)["C"] == "16" and layer_fields(dump, 4)["cin_pad"] == "16"
    rc, dump = hip.plan_dump(FC_FIRST, dt, 3, True)
    assert rc == 0, dump
    f0 = layer_fields(dump, 0)
    assert (f0["in"], f0["fc_h"], f0["fc_w"], f0["fc_c"], f0["cin"], f0["kpad"], f0["bn"], f0["filters"]) == ("[-1]", "6", "10", "72", "4320", "4352", "1", "264")
    assert 4352 // 64 == 68 and 264 > 256 and layer_fields(dump, 1)["cin"] == "264" and layer_fields(dump, 2)["filters"] == "5"
    for side, num, classes, sqrt in HEADS:
        rc, dump = hip.plan_dump(head_cfg(side, num, classes, sqrt), dt, 3, True)
        assert rc == 0, dump
        f1 = layer_fields(dump, 1)
        assert (f1["side"], f1["na"], f1["classes"], f1["sqr"]) == (str(side), str(num), str(classes), str(sqrt))
    for h, w in STEM_SIZES:
        rc, dump = hip.plan_dump(stem_cfg(h, w), dt, 3, True)
        assert rc == 0, dump
        f0 = layer_fields(dump, 0)
        assert f0["s2d7"] == "1" and (f0["H"], f0["W"]) == (str(h // 2), str(w // 2))
    for with_local in (True, False):
        rc, dump = hip.plan_dump(window_cfg(with_local), dt, 3, True)
        assert rc == 0, dump
        if with_local:          # both producers live in the route's buffer: k_local reads at pixel stride 24 (channel offset 8) and writes at stride 24 (offset 0)
            f = [layer_fields(dump, i) for i in range(4)]
            assert f[0]["storage"] == f[1]["storage"] == f[2]["storage"] and storage_fields(dump, int(f[2]["storage"]))["stride"] == "24"
            assert (f[0]["ch_off"], f[1]["ch_off"], f[1]["in"], f[2]["in"], f[3]["cin"]) == ("8", "0", "[0]", "[1,0]", "24")


def test_stream_splitter_counts():
    for cfg in [str(golden(n)["cfg"]) for n in NEW + OLD] + [FC_FIRST, RECYCLED, window_cfg(), local_first_cfg("3x3_s1_p1_f13")]:
        secs = IO.parse_cfg(cfg)
        flat = IO.synth_weights(secs, seed=3)
        assert flat.size == IO.weights_count(secs)
        p = layer_params(cfg, flat)
        assert sorted(p) == [c["index"] for c in IO.conv_specs(secs)] and np.array_equal(flatten_params(cfg, p), flat)
    p = layer_params(FC_FIRST, np.arange(IO.weights_count(IO.parse_cfg(FC_FIRST)), dtype=np.float32))
    assert p[0]["bias"][0] == 0 and p[0]["w"][0, 0] == 264 and p[0]["gamma"][0] == 264 + 264 * 4320 and p[0]["var"][-1] == 264 * 4324 - 1 and p[1]["bias"][0] == 264 * 4324


# ---- the fixtures regenerate ----
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    """tools/make_golden.py v1_edges, run afresh against oracle/_ref: the cfg, weights and images byte for byte, every recorded tensor to 1e-6 of its scale
    (the reference is built with -Ofast, and its libm may pick other code on another CPU)"""
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden as MG
    finally:
        sys.path.pop(0)
    paths = MG.gen_mini_v1_edges(out_dir=str(tmp_path))
    assert sorted(os.path.basename(p) for p in paths) == sorted(NEW)
    for path in paths:
        new = np.load(path, allow_pickle=False); old = golden(os.path.basename(path))
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            if k in ("cfg", "weights", "images_u8", "thresh"):
                assert np.array_equal(new[k], old[k]), k
            else:
                assert new[k].shape == old[k].shape and np.abs(new[k] - old[k]).max() <= 1e-6 * max(1.0, float(np.abs(old[k]).max())), k
