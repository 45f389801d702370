"""The YOLOv1 family on the device, layer by layer: k_local (ew_ops.hip), the dense conv run as a [connected] GEMM with the CHW -> HWC filter permutation
of yolo_pack.cpp, k_decode_v1 (post_ops.hip) and the space-to-depth form of the 7x7 / 2 first conv.  Against the compiled reference's recorded layers
(tests/golden/mini_v1_edges.npz, mini_v1_stem.npz; fp32), against the float64 restatements of tests/test_v1_host.py applied to the device's OWN stored
input of each layer (fp32, bf16, fp16), by exact integer counts through [net] yolo_input=planes networks whose first layer is the layer under test, and
bit for bit for the decoded rows.  tests/test_v1_host.py ties the restatements to the reference and asserts, from the cfg's arithmetic and the planner's
dump, that each network has the property its test relies on.  Batch 3 throughout."""
import numpy as np
import pytest
from conftest import golden
from oracle import postprocess_ref as P
from yolo_tensorflow_amd import darknet_io as IO
import test_v1_host as H
from test_gpu_edges import DTYPES, _dt, _round
from test_gpu_resnet import U, _storage_half_ulp, act64

pytestmark = pytest.mark.gpu
SLOPES = {"linear": 1.0, "leaky": 0.1, "relu": 0.0}
LIPSCHITZ = {"tanh": 1.0, "logistic": 0.25}          # |act'| at most: what an error of the stored pre-activation becomes behind the activation


def _run(hiplib, cfg, flat, x, name, keep=True, scale=1.0 / 255.0, detections=True):
    """one forward of the whole batch -> (engine, decoded tensor or None, every layer's stored output as fp32 or None); the caller closes the engine"""
    eng = hiplib.Engine(cfg, max_batch=x.shape[0], dtype=_dt(hiplib, name), semantics=hiplib.SEM_DARKNET, keep_layers=keep)
    eng.set_weights(flat)
    det = eng.forward(x, scale=scale, want_detections=detections)
    types = [s["type"] for s in IO.parse_cfg(cfg)[1:]]
    outs = [None if t in ("detection", "softmax") else eng.layer_output(i, x.shape[0]) for i, t in enumerate(types)] if keep else None
    return eng, det, outs


def _head_raw(eng, n):
    """the vectors the [detection] layer decodes, [n, side^2 (classes + 5 num)] (yolo_head_raw writes them one after the other)"""
    per = eng.last_layer_output(1).shape[1]
    return eng.head_raw(0, n).reshape(-1)[:n * per].reshape(n, per).copy()


@pytest.fixture(scope="module")
def nets(hiplib):
    """the two fixture networks, keep_layers=True, once per storage type: {(fixture, type): dict(det, outs, raw, boxes)}"""
    out = {}
    for fx in H.NEW:
        g = golden(fx); cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg)
        hh, ww = int(secs[0]["height"]), int(secs[0]["width"])
        for name in DTYPES:
            eng, det, outs = _run(hiplib, cfg, g["weights"], g["images_u8"], name)
            out[fx, name] = dict(det=det, outs=outs, raw=_head_raw(eng, 3), staged=eng.staged_input(3),
                                 boxes=[eng.darknet_boxes(b, ww, hh, thresh=float(g["thresh"])) for b in range(3)])
            eng.close()
    return out


# ---- (a) whole networks against the reference's own C code, fp32 ----
@pytest.mark.parametrize("fx", H.NEW)
def test_fixture_networks_match_the_compiled_reference_fp32(hiplib, nets, fx):
    """every layer of the reference's forward pass, fp32 device path, batch 3: 5e-4 of each tensor's scale (the bound of
    test_mini_edges_matches_compiled_reference_fp32); the plan that keeps no layer gives the same decoded tensor bit for bit"""
    g = golden(fx); cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    run = nets[fx, "fp32"]
    worst = []
    for i, s in enumerate(secs):
        if s["type"] == "detection":
            got, ref = run["raw"], g["layer_%02d" % i]
        else:
            got, ref = run["outs"][i], g["layer_%02d" % i]
        assert got.shape == ref.shape, "layer %d (%s)" % (i, s["type"])
        worst.append(float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12)))
        print("%s layer %d (%s): relmax %.3e" % (fx, i, s["type"], worst[-1]))
    for i, r in enumerate(worst):
        assert r < 5e-4, "layer %d (%s): %.3e" % (i, secs[i]["type"], r)
    eng, lean, _ = _run(hiplib, cfg, g["weights"], g["images_u8"], "fp32", keep=False)
    eng.close()
    assert np.array_equal(lean, run["det"])


# ---- (b) layer-local values on the device's own stored inputs ----
def _rule(out_name, want):
    """what the project allows a dense conv's stored output to differ from its reference rounded once to the storage type by: _assert_bf16_close,
    _assert_f16_close, and the fp32 rule of test_conv_fp32_exact_path"""
    a = np.abs(want).astype(np.float64)
    if out_name == "bf16":
        return 2.0 ** -7 * a + 2e-3
    if out_name == "fp16":
        return 2.0 ** -9 * a + 3e-4
    return 1e-4 * a + 1e-4 * float(a.max())


def _check_values(hiplib, out_name, y, mag, K, act, got, what):
    """`got` against the float64 pre-activation y of a layer of K products per output: the output rounding of _rule plus the accumulation term K 2^-24 sum |x w|.
    A slope-family activation is part of the kernel's epilogue (one rounding); tanh / logistic run as a pass of their own over the stored pre-activation, and are
    compared behind the activation: its Lipschitz constant times the pre-activation's bound, plus test_op_activate's bound for that function.  -> the worst share"""
    acc = K * U * mag
    assert got.shape == y.shape and np.isfinite(got).all(), what
    if act in SLOPES:
        ref = np.where(y > 0, y, SLOPES[act] * y)
        want = _round(out_name, ref.astype(np.float32)).astype(np.float64)
        bound = _rule(out_name, want) + acc
    else:
        pre = _round(out_name, y.astype(np.float32))
        want = act64(act, pre)
        bound = LIPSCHITZ[act] * (_rule(out_name, pre) + acc) + 8 * U * np.maximum(1, np.abs(want)) + _storage_half_ulp(hiplib, want, _dt(hiplib, out_name))
    err = np.abs(got.astype(np.float64) - want)
    share = float((err / bound).max())
    strict = float((err / (acc + _storage_half_ulp(hiplib, want, _dt(hiplib, out_name)) + 8 * U * np.maximum(1, np.abs(want)))).max())
    print("%s stored as %s: worst share of the bound %.4f (of accumulation term + half a unit in the last place alone: %.3f); max err %.3e of scale %.3f" % (
        what, out_name, share, strict, float(err.max()), float(np.abs(want).max())))
    assert (err <= bound).all(), "%s %s: %g over the bound at %s" % (what, out_name, float((err - bound).max()), np.unravel_index((err - bound).argmax(), err.shape))
    return share


def _check_local(hiplib, name, sec, p, x, got, what):
    y, mag = H.local64(sec, dict(bias=p["bias"], w=_round(name, p["w"])), x)
    return _check_values(hiplib, name, y, mag, int(sec["size"]) ** 2 * x.shape[3] + 1, sec.get("activation", "logistic"), got, what)


def _check_connected(hiplib, name, sec, p, x, got, what, head):
    """a head's output is stored as fp32 in every configuration"""
    w, b = H.connected_fold(p)
    y, mag = H.connected64(p, x, w=_round(name, w.astype(np.float32)).astype(np.float64), b=b)
    return _check_values(hiplib, "fp32" if head else name, y, mag, w.shape[1] + 1, sec.get("activation", "logistic"), got, what)


def _check_v1_layers(hiplib, name, cfg, flat, outs, first_input=None):
    """every [local] and [connected] layer of `cfg` on the device's own stored input -> {(type, activation)} seen"""
    secs = IO.parse_cfg(cfg)[1:]; params = H.layer_params(cfg, flat); seen = set()
    for i, s in enumerate(secs):
        if s["type"] not in ("local", "connected"):
            continue
        x = outs[i - 1] if i else first_input
        what = "layer %d (%s %s)" % (i, s["type"], s.get("activation", "logistic"))
        if s["type"] == "local":
            _check_local(hiplib, name, s, params[i], x, outs[i], what)
        else:
            _check_connected(hiplib, name, s, params[i], x, outs[i], what, head=i + 1 < len(secs) and secs[i + 1]["type"] == "detection")
        seen.add((s["type"], s.get("activation", "logistic")))
    return seen


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("fx", H.NEW)
def test_local_and_connected_layers_on_their_stored_inputs(hiplib, nets, fx, name):
    g = golden(fx)
    seen = _check_v1_layers(hiplib, name, str(g["cfg"]), g["weights"], nets[fx, name]["outs"])
    if fx == "mini_v1_edges.npz":
        assert seen == {("local", "leaky"), ("local", "relu"), ("local", "tanh"), ("connected", "logistic"), ("connected", "linear")}
        secs = IO.parse_cfg(str(g["cfg"])); L = secs[1:]; shapes = IO.layer_shapes(secs)
        assert H.local_k8(secs, 3) == 72 and int(L[3]["filters"]) % 4 == 1 and shapes[3][1:3] == (3, 5)          # a second pass of k_local's lanes; zero-fill waves; Wo != Ho
        assert (int(L[5]["stride"]), int(L[5]["pad"])) == (2, 1) and (int(L[6]["size"]), int(L[6]["pad"])) == (2, 0)
        assert shapes[7][4] == 48 and int(L[7]["output"]) == 37 and "activation" not in L[7]                       # K < 64, 37 outputs, the default logistic
        assert H.detection_of(L[9]) == (2, 3, 2, 0)
    else:
        secs = IO.parse_cfg(str(g["cfg"])); shapes = IO.layer_shapes(secs)
        assert seen == {("connected", "linear")} and shapes[2][4] == 280 and 280 % 64 and shapes[1][1:4] == (5, 7, 8)      # a half-empty last K-step, a rectangular CHW flatten
        assert H.detection_of(secs[-1]) == (1, 1, 2, 1)


# ---- (c) exact counts: the layer under test is the network's first ----
def _taps_inside(h, w, k, st, pad):
    _, _, _, ho, wo = H.local_geometry(dict(size=k, stride=st, pad=pad), h, w)
    cnt = np.zeros((ho, wo), np.int64)
    for oy in range(ho):
        for ox in range(wo):
            cnt[oy, ox] = sum(1 for kh in range(k) for kw in range(k) if 0 <= oy * st - pad + kh < h and 0 <= ox * st - pad + kw < w)
    return cnt


def _with_params(cfg, seed, edit):
    """the seeded stream of `cfg` with `edit(params)` applied"""
    secs = IO.parse_cfg(cfg)
    p = H.layer_params(cfg, IO.synth_weights(secs, seed=seed))
    edit(p)
    return H.flatten_params(cfg, p)


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("key", sorted(H.LOCAL_FIRST))
def test_local_counts_and_one_hot_filters(hiplib, key, name):
    """64 planes of 3 x 5 into a [local]: all ones against filters of ones give 64 x (taps inside the image) exactly; and filters that are one at a single (tap,
    channel) per (location, filter) return the value of that channel at that tap's pixel -- image 0 names the channel (plane c holds 1 + c), image 1 the pixel
    (1 + y W + x), image 2 holds 1 + c % 8 -- or zero where the tap lies outside.  Every value is an integer below 256: exact in the three storage types."""
    F, k, st, pad = H.LOCAL_FIRST[key]; cfg = H.local_first_cfg(key)
    h, w, C = 3, 5, 64
    cnt = _taps_inside(h, w, k, st, pad); ho, wo = cnt.shape

    def ones(p):
        for i in range(3):
            p[i]["w"][:] = 1; p[i]["bias"][:] = 0
    x1 = np.ones((3, h, w, C), np.float32)
    eng, _, outs = _run(hiplib, cfg, _with_params(cfg, 1, ones), x1, name, scale=1.0)
    want = np.broadcast_to((C * cnt)[None, :, :, None], (3, ho, wo, F)).astype(np.float32)
    assert float(want.max()) < 2048 and np.array_equal(outs[0], want), key
    # the 1x1 conv of ones sums every stored channel of the pixel (the zero fill behind 13 filters adds nothing), the head every pixel of its 8 channels
    conv = np.broadcast_to((F * C * cnt)[None, :, :, None], (3, ho, wo, 8)).astype(np.float32)
    assert np.array_equal(_round(name, conv), conv) and np.array_equal(outs[1], conv), key
    assert np.array_equal(_head_raw(eng, 3), np.full((3, 7), 8 * F * C * cnt.sum(), np.float32)) and 8 * F * C * cnt.sum() < 2 ** 24
    # one-hot filters
    loc, f = np.meshgrid(np.arange(ho * wo), np.arange(F), indexing="ij")
    tap = (loc * 7 + f * 3 + 8) % (k * k); ch = (loc * 5 + f * 11 + 3) % C
    gran = tap * (C // 8) + ch // 8          # the granule of the filter row k_local's lanes stride over

    def one_hot(p):
        p[0]["w"][:] = 0; p[0]["bias"][:] = 0
        p[0]["w"][loc, f, ch, tap // k, tap % k] = 1
    c = np.arange(C, dtype=np.float32)[None, None, :]; q = np.arange(h * w, dtype=np.float32).reshape(h, w, 1)
    x = np.stack([np.broadcast_to(1 + c, (h, w, C)), np.broadcast_to(1 + q, (h, w, C)), np.broadcast_to(1 + c % 8, (h, w, C))]).astype(np.float32)
    eng.set_weights(_with_params(cfg, 1, one_hot))
    eng.forward(x, scale=1.0)
    got = eng.layer_output(0, 3)
    eng.close()
    oy, ox = loc // wo, loc % wo
    iy, ix = oy * st - pad + tap // k, ox * st - pad + tap % k
    inside = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    want = np.where(inside[None], x[:, np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1), ch], 0).reshape(3, ho, wo, F)
    assert inside.any() and (~inside).any() == bool(pad)
    if k == 3:
        assert (gran[inside] >= 64).any() and (gran[inside] < 64).any()          # a lane's second pass reads a tap inside the image
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s %s: %d outputs name another tap or channel, first at %s: got %g, want %g" % (key, name, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", DTYPES)
def test_local_pad_channels_are_zero_in_a_recycled_buffer(hiplib, name):
    """F = 13 filters are stored in 16 channels, and k_local's waves f = 13 .. 15 write zeros there.  A new engine's buffers start as zeros, so stale data can
    only come from an earlier layer of the same forward: in the plan that pools its buffers (keep_layers=False) a [local] layer of 16 filters that nothing reads
    fills a buffer with infinities, and the 13-filter [local] layer two layers on takes that buffer over -- the shared physical buffer is asserted from the dump.
    The 1x1 conv behind it multiplies channels 13 .. 15 by zero filters, and 0 x inf is NaN: the head holds the exact sum only if k_local wrote zeros.  (With that
    store removed on a scratch copy this test fails in fp32 and bf16: docs/NOTEBOOK.md.  fp16 stores saturate at 65504 -- elt.h -- so an fp16 buffer never holds an
    infinity and the fp16 case pins the sum alone.)  The recycled-buffer case of test_local_layer_pad_channels_are_zero..., for F % 4 == 1"""
    cfg = H.RECYCLED
    rc, dump = hiplib.plan_dump(cfg, _dt(hiplib, name), 3, False)
    assert rc == 0, dump
    first, second, stride = H.recycled_buffers(dump)
    assert first == second and stride == 16 and H.layer_fields(dump, 3)["C"] == "13" and H.layer_fields(dump, 4)["cin_pad"] == "16"

    def edit(p):
        p[0]["w"][:] = np.eye(64, dtype=np.float32)[None, None]; p[1]["w"][:] = np.inf          # the conv hands the planes on; the unread [local]: infinities
        for i in (3, 4, 5):
            p[i]["w"][:] = 1
        for i in p:
            p[i]["bias"][:] = 0
    x1 = np.ones((3, 3, 5, 64), np.float32)
    cnt = _taps_inside(3, 5, 3, 1, 1)
    eng, _, _ = _run(hiplib, cfg, _with_params(cfg, 1, edit), x1, name, keep=False, scale=1.0)
    raw = [_head_raw(eng, 3)]
    eng.forward(x1, scale=1.0)          # a second forward: the buffer now also holds what the first one's later layers left
    raw.append(_head_raw(eng, 3))
    eng.close()
    for r in raw:
        assert np.array_equal(r, np.full((3, 7), 8 * 13 * 64 * cnt.sum(), np.float32)), r
    # the same network with every layer kept: the unread layer did leave infinities (65504 in fp16), and the 13-filter layer's values are the counts
    eng, _, outs = _run(hiplib, cfg, _with_params(cfg, 1, edit), x1, name, scale=1.0)
    eng.close()
    assert (np.isinf(outs[1]) if name != "fp16" else outs[1] == 65504).all()
    assert np.array_equal(outs[3], np.broadcast_to((64 * cnt)[None, :, :, None], (3, 3, 5, 13)).astype(np.float32))
    assert np.array_equal(outs[4], np.broadcast_to((13 * 64 * cnt)[None, :, :, None], (3, 3, 5, 8)).astype(np.float32))


@pytest.mark.parametrize("name", DTYPES)
def test_connected_counts_and_chw_permutation(hiplib, name):
    """72 planes of 6 x 10 into a batch-normalised [connected] of 264 outputs (K = 4320 in 68 K-steps, the last half empty; a second channel tile), unit
    statistics: gamma = 1 + 1e-6 in float32 over a variance of one makes the folded scale gamma / (sqrt(var) + 1e-6f) exactly one.  Ones against ones give 4320,
    rounded once to the storage type.  Then each output row's filter is a single one at darknet's CHW index c hw + q, (c, q) chosen per row: image 0 (plane c
    holds 1 + c) must return 1 + c, image 1 (pixel q holds 1 + q, q = y W + x) must return 1 + q: a permutation that sends a row's one to another (channel, pixel)
    cannot pass.  (The packer's permutation depends on fc_h * fc_w and the channel count only, so there is no fc_h / fc_w exchange to catch.)  Last, a seeded
    stream whose batch-norm vectors are not trivial over a seeded input: layers 0 and 1 against float64 on their stored inputs, the fold restated in
    test_v1_host.connected_fold -- a wrong order of the stream's gamma / mean / variance, or a fold that misses the mean, cannot pass."""
    cfg = H.FC_FIRST; h, w, C, O = 6, 10, 72, 264; hw = h * w
    rc, dump = hiplib.plan_dump(cfg, _dt(hiplib, name), 3, True)
    f0 = H.layer_fields(dump, 0)
    assert rc == 0 and (f0["in"], f0["fc_h"], f0["fc_w"], f0["fc_c"], f0["cin"], f0["kpad"], f0["filters"], f0["bn"]) == ("[-1]", "6", "10", "72", "4320", "4352", "264", "1")

    def unit_bn(p):
        p[0]["gamma"][:] = np.float32(1) + np.float32(.000001); p[0]["mean"][:] = 0; p[0]["var"][:] = 1; p[0]["bias"][:] = 0

    def ones(p):
        unit_bn(p); p[0]["w"][:] = 1
    o = np.arange(O); co = (o * 7 + 3) % C; qo = (o * 13 + 5) % hw
    assert len(set(zip(co.tolist(), qo.tolist()))) == O

    def one_hot(p):
        unit_bn(p); p[0]["w"][:] = 0; p[0]["w"][o, co * hw + qo] = 1
    x1 = np.ones((3, h, w, C), np.float32)
    eng, _, outs = _run(hiplib, cfg, _with_params(cfg, 2, ones), x1, name, scale=1.0, detections=False)
    assert outs[0].shape == (3, 1, 1, O) and np.array_equal(outs[0], np.full((3, 1, 1, O), _round(name, np.float32(4320))))
    c = np.arange(C, dtype=np.float32)[None, None, :]; q = np.arange(hw, dtype=np.float32).reshape(h, w, 1)
    x = np.stack([np.broadcast_to(1 + c, (h, w, C)), np.broadcast_to(1 + q, (h, w, C)), np.ones((h, w, C))]).astype(np.float32)
    eng.set_weights(_with_params(cfg, 2, one_hot))
    eng.forward(x, scale=1.0, want_detections=False)
    got = eng.layer_output(0, 3).reshape(3, O)
    want = np.stack([1 + co, 1 + qo, np.ones(O)]).astype(np.float32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d rows read another input, first (image, row) %s: got %g, want %g" % (name, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    # batch-norm vectors that are not trivial
    secs = IO.parse_cfg(cfg); flat = IO.synth_weights(secs, seed=2); params = H.layer_params(cfg, flat)
    p0 = params[0]
    assert np.abs(p0["gamma"] - 1).max() > .1 and np.abs(p0["mean"]).max() > .05 and np.abs(p0["var"] - 1).max() > .1 and np.abs(p0["bias"]).max() > .05
    eng.set_weights(flat)
    xr = np.random.default_rng(3).random((3, h, w, C), dtype=np.float32)
    eng.forward(xr, scale=1.0, want_detections=False)
    xs = eng.staged_input(3)
    y0, y1 = eng.layer_output(0, 3), eng.layer_output(1, 3)
    eng.close()
    assert xs.shape == (3, h, w, C) and np.abs(xs - xr).max() <= 2.0 ** -9
    _check_connected(hiplib, name, secs[1], p0, xs, y0, "[connected] 264, batch-normalised, over 6 x 10 x 72", head=False)
    _check_connected(hiplib, name, secs[2], params[1], y0, y1, "[connected] 37 over the 264", head=False)


# ---- (d) k_local reading and writing channel windows of a concatenation ----
@pytest.mark.parametrize("name", DTYPES)
def test_local_in_and_out_of_a_concatenation_window(hiplib, name):
    """conv -> 16, [local] 8 over it, [route] of both, a 1x1 [local] over the 24 channels.  The planner places both producers in the route's buffer: the first
    [local] reads its producer at pixel stride 24 (channel offset 8) and writes at stride 24 (offset 0) -- asserted from the dump.  Values as in (b); the
    conv's window is bit-identical to the conv's output in the network without that [local]."""
    cfg = H.window_cfg(True)
    rc, dump = hiplib.plan_dump(cfg, _dt(hiplib, name), 3, True)
    assert rc == 0, dump
    f = [H.layer_fields(dump, i) for i in range(4)]
    assert f[0]["storage"] == f[1]["storage"] == f[2]["storage"] and H.storage_fields(dump, int(f[2]["storage"]))["stride"] == "24"
    assert (f[0]["ch_off"], f[1]["ch_off"], f[2]["ch_off"]) == ("8", "0", "0") and f[2]["copy_inputs"] == "[]" and f[3]["cin"] == "24"
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=31)
    imgs = np.random.default_rng(32).integers(0, 256, (3, 4, 6, 3), dtype=np.uint8)
    eng, det, outs = _run(hiplib, cfg, flat, imgs, name)
    eng.close()
    assert np.array_equal(outs[2], np.concatenate([outs[1], outs[0]], -1))
    params = H.layer_params(cfg, flat); L = secs[1:]
    _check_local(hiplib, name, L[1], params[1], outs[0], outs[1], "window: layer 1 ([local] 3x3 out of and into the concatenation)")
    _check_local(hiplib, name, L[3], params[3], outs[2], outs[3], "window: layer 3 ([local] 1x1 over the 24 channels)")
    _check_connected(hiplib, name, L[4], params[4], outs[3], outs[4], "window: layer 4 ([connected])", head=True)
    plain = H.window_cfg(False); psecs = IO.parse_cfg(plain)
    pp = H.layer_params(plain, IO.synth_weights(psecs, seed=33)); pp[0] = params[0]
    eng, _, pouts = _run(hiplib, plain, H.flatten_params(plain, pp), imgs, name)
    eng.close()
    assert np.array_equal(pouts[0], outs[0]) and np.array_equal(outs[2][..., 8:], pouts[0])
    eng, lean, _ = _run(hiplib, cfg, flat, imgs, name, keep=False)
    eng.close()
    assert np.array_equal(lean, det)


# ---- (e) [detection] ----
def _head_stream(side, num, classes, seed):
    """a linear [connected] over 8 planes whose class rows are their biases alone (five levels: ties), whose confidences are negative for a third of the boxes"""
    rng = np.random.default_rng(seed); cells = side * side
    cls = rng.choice(np.float32([.1, .3, .5, .7, .9]), (cells, classes))
    if classes > 1:
        cls[0, :2] = np.float32(.9)          # cell 0: classes 0 and 1 tie for the best score
    conf = rng.uniform(-.9, .95, (cells, num)).astype(np.float32); conf[0, 0] = np.float32(.8); conf[-1, -1] = np.float32(-.6)
    box = np.stack([rng.uniform(.1, .9, (cells, num)), rng.uniform(.1, .9, (cells, num)), rng.uniform(-.3, .8, (cells, num)), rng.uniform(-.3, .8, (cells, num))], -1)
    box[0, 0, 2] = -.25          # a negative width: sqrt=0 hands it on, sqrt=1 squares it
    bias = np.concatenate([cls.reshape(-1), conf.reshape(-1), box.reshape(-1)]).astype(np.float32)
    w = rng.normal(0, .05, (bias.size, 8)).astype(np.float32); w[:cells * classes] = 0
    if cells * num == 1:         # one box: its confidence follows input 0, which the test sets to -1, .5, 1 for the three images
        bias[classes] = np.float32(.1); w[classes] = 0; w[classes, 0] = np.float32(.7)
    return np.concatenate([bias, w.reshape(-1)])


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("head", H.HEADS, ids=lambda h: "side%d_num%d_classes%d_sqrt%d" % h)
def test_detection_rows_bit_for_bit(hiplib, head, name):
    side, num, classes, sqrt = head
    cfg = H.head_cfg(*head); rows = side * side * num
    x = np.random.default_rng(41).uniform(-1, 1, (3, 1, 1, 8)).astype(np.float32); x[:, 0, 0, 0] = (-1, .5, 1)
    eng, det, outs = _run(hiplib, cfg, _head_stream(side, num, classes, 40 + side), x, name, scale=1.0)
    raw = _head_raw(eng, 3)
    assert det.shape == (3, rows, 5 + classes) and np.array_equal(raw, outs[0].reshape(3, -1))
    want = np.stack([H.v1_rows32(raw[b], side, num, classes, sqrt) for b in range(3)])
    assert np.array_equal(det, want), np.argwhere(det != want)[:4]
    assert (det[..., 4] < 0).any() and (det[..., 4] > 0).any()
    if not sqrt:
        assert (det[..., 2:4] < 0).any() and np.array_equal(det[..., 2:4], raw[:, side * side * (classes + num):].reshape(3, rows, 4)[..., 2:])
    sc = det[..., 4:5] * det[..., 5:]
    best = sc.max(-1); tie = (sc == best[..., None]).sum(-1) > 1
    assert tie.any() == (classes > 1)
    # the label: every row through the NMS that keeps everything (no two boxes of one class overlap by more than 1.5)
    recs, rws = eng.postprocess(3, score_thr=-10.0, iou_thr=1.5, max_out=rows, nms_mode=hiplib.NMS_DARKNET, select_mode=hiplib.SELECT_GT, return_rows=True)
    for b in range(3):
        assert sorted(rws[b].tolist()) == list(range(rows))
        assert np.array_equal(recs[b]["cls"], sc[b].argmax(-1)[rws[b]]) and np.array_equal(recs[b]["score"], best[b][rws[b]])
        if classes > 1:
            assert recs[b]["cls"][rws[b] == 0][0] == 0          # cell 0, box 0: classes 0 and 1 tie, the first wins
    for mode, select in ((hiplib.NMS_TF_V1, hiplib.SELECT_GE), (hiplib.NMS_DARKNET, hiplib.SELECT_GT)):
        kw = dict(score_thr=0.2, iou_thr=0.4, max_out=rows, nms_mode=mode, select_mode=select)
        post = eng.postprocess(3, **kw)
        both = eng.detect(x, scale=1.0, **kw)
        for b in range(3):
            ref, _ = P.postprocess_records(det[b], 0.2, 0.4, rows, mode, select)
            assert np.array_equal(post[b], both[b]) and len(post[b]) == len(ref)
            for fld in P.REC_DTYPE.names:
                assert np.array_equal(post[b][fld], ref[fld]), (mode, b, fld)
        assert sum(len(r) for r in post) > 0 or max(float(best.max()), 0.0) < 0.2
    eng.close()


@pytest.mark.parametrize("fx", H.NEW)
def test_darknet_boxes_of_the_fixture_networks(hiplib, nets, fx):
    """darknet_boxes against the reference's get_network_boxes per image, the comparison of test_mini_v1_matches_compiled_reference_fp32 (boxes there in
    units of the image: the absolute term is scaled by the side here); scores within 1e-3 of the threshold are left out of the gate, at most 5 % of them;
    and the decoded rows bit for bit from the device's own head vector, in every storage type"""
    g = golden(fx); secs = IO.parse_cfg(str(g["cfg"])); side, num, classes, sqrt = H.detection_of(secs[-1])
    hh, ww = float(secs[0]["height"]), float(secs[0]["width"]); thresh = float(g["thresh"]); tol = 2e-4
    for name in DTYPES:
        run = nets[fx, name]
        assert np.array_equal(run["det"], np.stack([H.v1_rows32(run["raw"][b], side, num, classes, sqrt) for b in range(3)])), name
    run = nets[fx, "fp32"]; left_out = 0
    for b in range(3):
        rec = run["boxes"][b]
        assert rec.shape == (g["obj_raw"].shape[1], 5 + classes)
        err = np.abs(rec[:, :4] - g["boxes_raw"][b])
        assert (err <= tol * 10 * np.abs(g["boxes_raw"][b]) + tol * np.array([ww, hh, ww, hh])).all(), (b, float(err.max()))
        np.testing.assert_allclose(rec[:, 4], g["obj_raw"][b], rtol=tol * 10, atol=tol)
        pr = run["det"][b][:, 4:5] * run["det"][b][:, 5:]
        clear = ~H.near_threshold(pr, thresh); left_out += int((~clear).sum())
        assert np.array_equal((rec[:, 5:] > 0)[clear], (g["prob_raw"][b] > 0)[clear])
        np.testing.assert_allclose(rec[:, 5:][clear], g["prob_raw"][b][clear], rtol=2e-3, atol=2e-4)
    assert left_out * 20 <= g["prob_raw"].size, left_out
    assert 0 < int((g["prob_raw"] > 0).sum()) < g["prob_raw"].size


# ---- (f) the two forms of the 7x7 / 2 / pad 3 first conv ----
def _conv64(x, w, bias, stride, pad):
    x = np.pad(np.asarray(x, np.float64), ((0, 0), (pad, pad), (pad, pad), (0, 0))); k = w.shape[0]
    win = np.lib.stride_tricks.sliding_window_view(x, (k, k), axis=(1, 2))[:, ::stride, ::stride]          # [n, ho, wo, c, kh, kw]
    return np.einsum("nhwcij,ijco->nhwo", win, np.asarray(w, np.float64)) + np.asarray(bias, np.float64)


def _check_stem(hiplib, name, y, slope, got, what):
    """_check_conv's rules (test_gpu_edges.py) against the float64 convolution"""
    ref = np.where(y > 0, y, slope * y).astype(np.float32)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    want = _round(name, ref)
    err = np.abs(got.astype(np.float64) - want)
    print("%s %s: worst share of the bound %.4f, max err %.3e of scale %.3f" % (what, name, float((err / _rule(name, want)).max()), float(err.max()), float(np.abs(ref).max())))
    assert (err <= _rule(name, want)).all(), "%s %s: max err %.3e at %s" % (what, name, float(err.max()), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("name", DTYPES)
def test_stem_of_the_fixture_in_both_forms(hiplib, nets, name):
    """mini_v1_stem's first layer (s2d7=1: H / 2 = 5 and W / 2 = 7, odd, below the 4 x 4 window's reach; 20 filters) against float64 on the staged input, filters
    rounded to the storage type; and the same filters through op_conv2d(stride=2, padding=3), the plain wide kernel: the same bound against the same values"""
    g = golden("mini_v1_stem.npz"); cfg = str(g["cfg"])
    rc, dump = hiplib.plan_dump(cfg, _dt(hiplib, name), 3, True)
    assert rc == 0 and H.layer_fields(dump, 0)["s2d7"] == "1"
    run = nets["mini_v1_stem.npz", name]
    p = H.layer_params(cfg, g["weights"])[0]; wq = _round(name, p["w"])
    x = run["staged"][..., :3]
    assert x.shape == (3, 10, 14, 3) and np.abs(x - g["images_u8"] / 255.0).max() <= (2.0 ** -9 if name == "bf16" else 2.0 ** -12 if name == "fp16" else 2.0 ** -23)
    y = _conv64(x, wq, p["bias"], 2, 3)
    _check_stem(hiplib, name, y, 0.1, run["outs"][0], "s2d form")
    plain = hiplib.op_conv2d(x, wq, p["bias"], stride=2, act=1, dtype=_dt(hiplib, name), padding=3)
    _check_stem(hiplib, name, y, 0.1, plain, "plain 7x7 / 2")


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("hw", H.STEM_SIZES, ids=lambda s: "%dx%d" % s)
def test_stem_sizes_values_and_counts(hiplib, hw, name):
    """the space-to-depth form at 2 x 2 (smaller than a window), 4 x 6, 10 x 14 and 6 x 30: seeded images against float64 and against the plain kernel's bound,
    then all ones against filters of ones: 3 x (taps inside the image), exactly -- the zero weights at the 4 x 4 form's taps kh = -1 and 7 add nothing"""
    h, w = hw; cfg = H.stem_cfg(h, w); secs = IO.parse_cfg(cfg)
    rc, dump = hiplib.plan_dump(cfg, _dt(hiplib, name), 3, True)
    assert rc == 0 and H.layer_fields(dump, 0)["s2d7"] == "1"
    # (the map is a head: kept as fp32 in every configuration, so the s2d form's output is not rounded to the storage type here; test_stem_of_the_fixture_in_both_forms
    # has it stored in 16 bits)
    stored = "fp32" if H.storage_fields(dump, int(H.layer_fields(dump, 0)["storage"]))["dt"] == str(hiplib.FP32) else name
    flat = IO.bf16_exact_filters(secs, IO.synth_weights(secs, seed=51))
    p = H.layer_params(cfg, flat)[0]
    assert np.array_equal(_round(name, p["w"]), p["w"])
    imgs = np.random.default_rng(52).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    eng, _, outs = _run(hiplib, cfg, flat, imgs, name, detections=False)
    x = eng.staged_input(3)[..., :3]
    y = _conv64(x, p["w"], p["bias"], 2, 3)
    _check_stem(hiplib, stored, y, 1.0, outs[0], "s2d form %dx%d" % hw)
    _check_stem(hiplib, name, y, 1.0, hiplib.op_conv2d(x, p["w"], p["bias"], stride=2, act=0, dtype=_dt(hiplib, name), padding=3), "plain 7x7 / 2 %dx%d" % hw)

    def ones(q):
        q[0]["w"][:] = 1; q[0]["bias"][:] = 0
    eng.set_weights(_with_params(cfg, 51, ones))
    eng.forward(np.ones((3, h, w, 3), np.float32), scale=1.0, want_detections=False)
    got = eng.layer_output(0, 3)
    eng.close()
    iy = (np.arange(h // 2) * 2 - 3)[:, None] + np.arange(7)[None]; ix = (np.arange(w // 2) * 2 - 3)[:, None] + np.arange(7)[None]
    cnt = ((iy >= 0) & (iy < h)).sum(1)[:, None] * ((ix >= 0) & (ix < w)).sum(1)[None]
    want = np.broadcast_to((3 * cnt)[None, :, :, None], got.shape).astype(np.float32)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
