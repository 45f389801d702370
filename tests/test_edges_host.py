"""The layers that move data and the dense conv's geometry keys at the edges the planner accepts, host side (no device): the numpy
restatements the GPU tests (test_gpu_edges.py) compare the device against, checked here against the compiled reference's recorded
layer outputs (tests/golden/mini_edges.npz: channel counts that are no multiples of 8, pad=0 / padding= / stride 3, five max-pool
geometries, a concatenation at channel offset 20); and the planner: what yolo_plan_check accepts runs, what is not served is refused at
plan time with a message that names the layer."""
import numpy as np
import pytest
from conftest import golden
from oracle import yolo_ref as R
from yolo_tensorflow_amd import hip, darknet_io as IO

FIXTURE = "mini_edges.npz"
SLOPES = {"linear": 1.0, "leaky": 0.1, "relu": 0.0}
MOVERS = ("maxpool", "upsample", "route", "shortcut", "reorg")


# ---- restatements shared with test_gpu_edges.py ----
def conv_geometry(sec):
    """(size, stride, pad) of a [convolutional] section as DN/parser.c reads it: pad=1 means size / 2, else padding= literally"""
    k, st = int(sec.get("size", 1)), int(sec.get("stride", 1))
    return k, st, (k // 2 if int(sec.get("pad", 0)) else int(sec.get("padding", 0)))


def pool_geometry(sec):
    st = int(sec.get("stride", 1)); k = int(sec.get("size", st))
    return k, st, int(sec.get("padding", (k - 1) // 2))


def stream_params(cfg, flat):
    """{layer index: dict(w [k, k, cin, cout] fp32, and bias or beta / gamma / mean / var)} of every [convolutional] section"""
    secs = IO.parse_cfg(cfg); out = {}; at = 0
    flat = np.asarray(flat, dtype=np.float32)
    for spec in IO.conv_specs(secs):
        n, k, cin = spec["filters"], spec["size"], spec["cin"]; p = {}
        for key in (("beta", "gamma", "mean", "var") if spec["bn"] else ("bias",)):
            p[key] = flat[at:at + n]; at += n
        p["w"] = np.ascontiguousarray(flat[at:at + n * cin * k * k].reshape(n, cin, k, k).transpose(2, 3, 1, 0)); at += n * cin * k * k
        out[spec["index"]] = p
    assert at == flat.size
    return out


def route_inputs(sec, i):
    return [l if l >= 0 else i + l for l in (int(v) for v in sec["layers"].split(","))]


def layer_inputs(secs, i):
    """indices of the tensors layer i reads (-1: the network input)"""
    s = secs[i]
    if s["type"] == "route":
        return route_inputs(s, i)
    if s["type"] == "shortcut":
        f = int(s["from"])
        return [i - 1, f if f >= 0 else i + f]
    return [i - 1]


def conv_ref(sec, p, x):
    """one [convolutional] section in fp32: cross-correlation, darknet's batch norm or the bias, a slope-family activation"""
    k, st, pad = conv_geometry(sec)
    y = R.conv2d_nhwc(x, p["w"], st, pad)
    y = R.batch_norm(y, p, mode="darknet_cpu") if "beta" in p else y + p["bias"]
    slope = np.float32(SLOPES[sec.get("activation", "logistic")])
    return np.where(y > 0, y, slope * y).astype(np.float32)


def mover_ref(sec, i, ins, semantics="darknet"):
    """a layer that moves data, on the tensors it reads (`ins`, in the order of layer_inputs)"""
    t = sec["type"]
    if t == "maxpool":
        return R.max_pool(ins[0], *pool_geometry(sec))
    if t == "upsample":
        return R.upsample_nearest(ins[0], int(sec.get("stride", 2))) if semantics == "darknet" else R.upsample_tf(ins[0])
    if t == "reorg":
        return (R.reorg_darknet if semantics == "darknet" else R.space_to_depth)(ins[0], int(sec.get("stride", 1)))
    if t == "route":
        return np.concatenate(ins, axis=-1)
    if t == "shortcut":
        return ins[0] + ins[1]
    raise ValueError(t)


def _ok(cfg, dtype=hip.BF16):
    rc, msg = hip.plan_check(cfg, dtype=dtype)
    assert rc == 0, msg


def _refused(cfg, *needles, dtype=hip.BF16):
    rc, msg = hip.plan_check(cfg, dtype=dtype)
    assert rc != 0, "planned: " + cfg
    for n in needles:
        assert n in msg, (n, msg)
    return msg


# ---- the fixture is what its docstring says ----
def test_fixture_covers_the_edges():
    g = golden(FIXTURE); secs = IO.parse_cfg(str(g["cfg"]))
    assert (int(secs[0]["height"]), int(secs[0]["width"])) == (15, 22) and g["images_u8"].shape == (3, 15, 22, 3)
    shapes = IO.layer_shapes(secs); secs = secs[1:]
    convs = [(conv_geometry(s), int(s.get("batch_normalize", 0))) for s in secs if s["type"] == "convolutional"]
    geos = {c[0] for c in convs}
    assert {(3, 1, 0), (3, 2, 2), (3, 1, 2), (3, 3, 2), (3, 1, 1), (1, 1, 0)} <= geos
    assert 2 * sum(1 for c in convs if not c[1]) >= len(convs)          # at least half are bias-only
    assert {pool_geometry(s) for s in secs if s["type"] == "maxpool"} == {(2, 2, 0), (2, 1, 0), (3, 2, 1), (3, 1, 0), (3, 2, 0)}
    for s, sh in zip(secs, shapes):
        if s["type"] == "maxpool":          # no window wholly outside: padding < min(size, stride)
            k, st, pad = pool_geometry(s)
            assert pad < min(k, st)
    assert all(sh[3] % 8 for sh in shapes if sh[0] in ("maxpool", "upsample", "shortcut"))          # every one of them moves a ragged channel count
    assert {sh[3] for sh in shapes} >= {20, 12, 27}
    cat = [i for i, s in enumerate(secs) if s["type"] == "route" and "," in s["layers"]]
    assert len(cat) == 1 and [shapes[j][3] for j in route_inputs(secs[cat[0]], cat[0])] == [20, 12]
    assert sum(1 for s in secs if s["type"] == "route" and "," not in s["layers"]) >= 1
    sc = [i for i, s in enumerate(secs) if s["type"] == "shortcut"][0]
    assert secs[sc - 1]["activation"] == "leaky" and any(sc - 1 in layer_inputs(secs, j) for j in range(sc + 1, len(secs)))      # its conv has a second reader: never folded
    for i in range(len(secs)):
        assert g["layer_%02d" % i].shape == (3,) + shapes[i][1:4]
        assert float(g["max_abs"][i]) == float(np.abs(g["layer_%02d" % i]).max()) < 1e3
    # filters are bf16-exact and fp16-exact
    for p in stream_params(str(g["cfg"]), g["weights"]).values():
        assert np.array_equal(R.to_bf16(p["w"]), p["w"]) and np.array_equal(R.to_f16(p["w"]), p["w"])


# ---- the restatements against the reference's recorded layers ----
def test_restatements_match_the_reference_layers():
    """every layer of mini_edges on the fixture's own input tensors of that layer: the movers bit for bit, the convs within 1e-5 of the
    tensor's scale (fp32 summation order between two CPU programs; measured: at most 8e-7)"""
    g = golden(FIXTURE); cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    params = stream_params(cfg, g["weights"])
    x0 = g["images_u8"].astype(np.float32) / np.float32(255)
    tensor = lambda j: x0 if j < 0 else g["layer_%02d" % j]
    seen = set()
    for i, s in enumerate(secs):
        want = g["layer_%02d" % i]
        ins = [tensor(j) for j in layer_inputs(secs, i)]
        if s["type"] == "convolutional":
            got = conv_ref(s, params[i], ins[0])
            assert got.shape == want.shape
            r = float(np.abs(got - want).max() / np.abs(want).max())
            print("layer %d conv %s: relmax %.3e" % (i, conv_geometry(s), r))
            assert r <= 1e-5, "layer %d" % i
        else:
            assert s["type"] in MOVERS
            got = mover_ref(s, i, ins)
            assert got.dtype == np.float32 and np.array_equal(got, want), "layer %d (%s)" % (i, s["type"])
        seen.add(s["type"])
    assert seen == set(MOVERS) | {"convolutional"}


# ---- the planner ----
@pytest.mark.parametrize("dtype", [hip.FP32, hip.BF16, hip.FP16, hip.FP16X2])
def test_fixture_cfg_plans_or_is_refused_by_layer(dtype):
    rc, msg = hip.plan_check(str(golden(FIXTURE)["cfg"]), dtype=dtype)
    if dtype == hip.FP16X2:          # pairs are interleaved per 32-channel group: the [reorg] of 20 channels is the first layer that cannot be served
        assert rc != 0 and msg.startswith("layer 13:") and "[reorg]" in msg and "32" in msg
    else:
        assert rc == 0, msg


NET = "[net]\nwidth=%d\nheight=%d\nchannels=3\nyolo_output=map\n\n"
CONV = "[convolutional]\nfilters=%d\nsize=%d\nstride=%d\npad=0\npadding=%d\nactivation=leaky\n\n"


def test_conv_larger_than_its_padded_input_is_refused():
    """a 3x3 pad=0 conv on a 2 x 2 tensor would plan an output of height 0"""
    _refused(NET % (2, 2) + CONV % (8, 3, 1, 0), "layer 0", "larger than its padded input")
    _refused(NET % (8, 2) + CONV % (8, 3, 1, 0), "layer 0", "larger than its padded input")          # one side is enough
    _refused(NET % (8, 8) + CONV % (8, 3, 2, 0) + CONV % (8, 3, 2, 0) + CONV % (8, 3, 1, 0), "layer 2", "larger than its padded input")      # 8 -> 3 -> 1
    _ok(NET % (2, 2) + CONV % (8, 3, 1, 1))
    _ok(NET % (3, 3) + CONV % (8, 3, 3, 0))
    _refused(NET % (8, 8) + CONV % (8, 3, 0, 1), "layer 0", "stride 0")
    _refused(NET % (8, 8) + CONV % (8, 3, 1, -1), "layer 0", "padding -1")
    _refused(NET % (8, 8) + CONV % (0, 3, 1, 1), "layer 0", "filters 0")


def test_pool_geometry_is_checked():
    pool = "[maxpool]\nsize=%d\nstride=%d\n\n"
    _ok(NET % (8, 8) + CONV % (12, 3, 1, 1) + pool % (3, 2))
    _refused(NET % (8, 8) + CONV % (12, 3, 1, 1) + pool % (2, 0), "layer 1", "[maxpool]")
    _refused(NET % (4, 4) + CONV % (12, 3, 1, 1) + pool % (2, 8), "layer 1", "no output pixel")


def _cat(c0, c1, c2=None):
    """a chain of two or three 3x3 convs of c0, c1 (, c2) filters, their outputs concatenated in that order by layer 2 (3), then a 1x1 conv"""
    cs = [c for c in (c0, c1, c2) if c is not None]
    return (NET % (8, 8) + "".join(CONV % (c, 3, 1, 1) for c in cs) + "[route]\nlayers=%s\n\n" % ",".join(str(j) for j in range(len(cs))) + CONV % (6, 1, 1, 0))


def test_what_the_run_refused_is_refused_or_served_at_plan_time():
    """`route copy of %d channels` and `reorg of a pair tensor` were refusals of the first forward, behind a yolo_plan_check that said OK"""
    for dtype in (hip.FP32, hip.BF16, hip.FP16):
        _ok(_cat(20, 12), dtype); _ok(_cat(16, 12), dtype); _ok(_cat(20, 16), dtype); _ok(_cat(3, 5, 9), dtype); _ok(_cat(27, 8, 20), dtype)
    _refused(_cat(20, 12), "layer 2", "[route]", "20 channels", "32-channel groups", dtype=hip.FP16X2)
    _refused(_cat(32, 12), "layer 2", "[route]", "12 channels", "offset 32", dtype=hip.FP16X2)
    _ok(_cat(32, 64), hip.FP16X2)
    _refused(_cat(20, 12), "layer 2", "[route]", "20 channels", "fp8", dtype=hip.FP8)
    _ok(_cat(16, 32), hip.FP8)
    # reorg
    reorg = lambda c: NET % (8, 8) + CONV % (c, 3, 1, 1) + "[reorg]\nstride=2\n\n" + CONV % (6, 1, 1, 0)
    for dtype in (hip.FP32, hip.BF16, hip.FP16):
        _ok(reorg(20), dtype); _ok(reorg(12), dtype); _ok(reorg(3), dtype)
    _refused(reorg(20), "layer 1", "[reorg]", "multiple of 32", dtype=hip.FP16X2)
    _refused(reorg(8), "layer 1", "[reorg]", "multiple of 32", dtype=hip.FP16X2)
    _ok(reorg(32), hip.FP16X2)
    _refused(NET % (8, 6) + CONV % (8, 3, 1, 1) + "[reorg]\nstride=4\n", "layer 1", "reorg stride")
