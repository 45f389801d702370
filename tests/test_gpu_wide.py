"""Dense convs of any size 1..11 on the device: op_conv2d(..., padding=) against the float64 restatement of test_grouped_host.py (tied to
the compiled reference's recorded layers in test_wide_host.py), exact integer counts, every tap in its place, every tile id, a whole
network against the reference's own C code (tests/golden/mini_wide.npz), and the public surface (autotune, export, Classifier over
cfg/zoo/alexnet.cfg, a 9-1-5 map network).  Batch 3 throughout."""
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
import test_grouped_host as GH

pytestmark = pytest.mark.gpu

MARGIN_TOL = 5e-4                            # the fp32 bound of the network tests, as a share of the tensor's largest value
TOL16 = {"bf16": 3e-2, "fp16": 4e-3}         # the factors of test_gpu_grouped.py, as a share of the largest logit

CASES = [          # (size, stride, pad, h, w, cin, cout)
    (5, 1, 2, 6, 7, 16, 16),          # 25 taps, the last size one validity bit per tap holds
    (6, 2, 3, 9, 8, 24, 20),          # 36 taps, even size, ragged cout
    (7, 1, 3, 5, 6, 64, 32),          # image smaller than the filter: every pixel has outside taps on both sides; uniform cursor
    (7, 2, 3, 9, 13, 3, 16),          # what the space-to-depth form refuses: odd extents, Cin_pad 8, per-lane taps
    (11, 4, 0, 27, 23, 3, 24),        # AlexNet's stem, 121 taps
    (11, 1, 5, 6, 5, 128, 16),        # two channel chunks x 121 taps
    (9, 1, 4, 9, 13, 32, 40),         # per-lane taps; more than one pixel tile, the last one ragged
    (5, 1, 1, 9, 13, 72, 8),          # padding != size / 2
    (2, 1, 0, 7, 9, 16, 16),          # size 2 without padding
    (4, 2, 2, 8, 8, 8, 16),           # even size with stride 2
]
_IDS = ["k%ds%dp%d_%dx%d_%dto%d" % c for c in CASES]
N = 3


def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _stored(hiplib, x, dtype):
    return _bf16(x) if dtype == hiplib.BF16 else np.asarray(x, np.float32).astype(np.float16).astype(np.float32) if dtype == hiplib.FP16 else np.asarray(x, dtype=np.float32)


def _relmax(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / (np.abs(b).max() + 1e-12))


def _hwio(w_oihw):
    return np.ascontiguousarray(np.transpose(w_oihw, (2, 3, 1, 0)))


def _leaky(y):
    return np.where(y > 0, y, np.float64(np.float32(0.1)) * y)


def _within(hiplib, got, want, dtype, what, scale=None):
    """fp32: 1e-4 of the tensor's largest value; bf16: 2^-7 |want| + 2e-3; fp16: 2^-10 |want| + 2e-3 (test_gpu_grouped.py).  `scale`: the
    magnitude the 16-bit ulp refers to where the result is a sum of separately rounded terms (a folded shortcut adds the stored
    residual to the conv's own value rounded to the storage type, exactly as the unfused [shortcut] of two stored tensors would:
    |conv| + |residual|, the rule of test_gpu_ops.py -- where the two cancel, |want| alone says nothing about either rounding)"""
    assert got.shape == want.shape and got.dtype == np.float32, (got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    if dtype == hiplib.FP32:
        r = float(err.max() / np.abs(want).max())
        print("%s fp32: relmax %.3e" % (what, r))
        assert r < 1e-4, what
    else:
        bound = 2.0 ** (-7 if dtype == hiplib.BF16 else -10) * (np.abs(want) if scale is None else scale) + 2e-3
        print("%s %s: max err / bound %.3f" % (what, "bf16" if dtype == hiplib.BF16 else "fp16", float((err / bound).max())))
        assert (err <= bound).all(), "%s: %g over at %r" % (what, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))


@pytest.fixture(scope="module")
def conv_data():
    """operands per case, drawn once: filters with variance 1 / fan-in"""
    rng = np.random.default_rng(171)
    data = {}
    for case in CASES:
        k, s, p, h, w, cin, cout = case
        x = rng.standard_normal((N, h, w, cin)).astype(np.float32)
        wt = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        r = rng.standard_normal((N, ho, wo, cout)).astype(np.float32)
        data[case] = (x, wt, b, r)
    return data


# ---- 1: values ----
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_op_conv2d_values(hiplib, conv_data, case):
    """bias and leaky, with and without a residual, fp32 / bf16 / fp16, against float64 on operands pre-rounded to the storage type"""
    k, s, p, h, w, cin, cout = case
    x, wt, b, r = conv_data[case]
    for dtype in (hiplib.FP32, hiplib.BF16, hiplib.FP16):
        y = _leaky(GH.gconv_ref(_stored(hiplib, x, dtype), _stored(hiplib, wt, dtype), b, 1, s, p))
        for res in (None, r):
            want = y if res is None else y + _stored(hiplib, res, dtype).astype(np.float64)
            got = hiplib.op_conv2d(x, _hwio(wt), b, stride=s, act=1, residual=res, dtype=dtype, padding=p)
            _within(hiplib, got, want, dtype, "conv %s res %d" % (_IDS[CASES.index(case)], res is not None), None if res is None else np.abs(y) + np.abs(res))


# ---- 2: exact counts ----
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_op_conv2d_counts_exactly(hiplib, case):
    """all-ones operands, linear, no bias: every product is 1 and the fp32 accumulator holds integers (at most 128 x 121 < 2^24), so the
    fp32 result is EXACTLY cin x (taps inside the image) -- a tap dropped or invented at a border shows as a whole unit.  The 16-bit
    result is that integer rounded once to the storage type."""
    k, s, p, h, w, cin, cout = case
    x = np.ones((N, h, w, cin), np.float32); wt = np.ones((k, k, cin, cout), np.float32)
    taps = GH.taps_inside(h, w, k, s, p)
    want = np.broadcast_to((taps * cin).astype(np.float32)[None, :, :, None], (N,) + taps.shape + (cout,))
    assert want.max() < 2 ** 24
    got = hiplib.op_conv2d(x, wt, None, stride=s, act=0, dtype=hiplib.FP32, padding=p)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    for dtype in (hiplib.BF16, hiplib.FP16):
        got = hiplib.op_conv2d(x, wt, None, stride=s, act=0, dtype=dtype, padding=p)
        assert np.array_equal(got, _stored(hiplib, want, dtype)), np.argwhere(got != _stored(hiplib, want, dtype))[:5]


# ---- 3: every tap in its place ----
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_op_conv2d_every_tap_in_its_place(hiplib, case):
    """cout = size^2, filter t is one-hot at tap t on channel 0; the input's channel 0 holds 1 + (y W + x) mod 240 (at most 240, exact in
    bf16 and fp16; the 27 x 23 image has more than 240 pixels, so the ramp wraps there -- neighbours still differ), the other channels
    a constant the filters never read: output channel t is exactly the image shifted by tap t, zero outside, in all three types.  A
    transposed or off-by-one tap order cannot pass this, though it passes the counts."""
    k, s, p, h, w, cin, _ = case
    cout = k * k
    x = np.full((N, h, w, cin), 7, np.float32)
    x[..., 0] = (1 + (np.arange(h * w) % 240)).reshape(h, w).astype(np.float32)[None] + np.arange(N, dtype=np.float32)[:, None, None]
    assert x.max() <= 240 + N - 1 <= 256
    wt = np.zeros((cout, cin, k, k), np.float32)
    for t in range(cout):
        wt[t, 0, t // k, t % k] = 1
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    want = np.zeros((N, ho, wo, cout), np.float32)
    for t in range(cout):
        for oy in range(ho):
            for ox in range(wo):
                iy, ix = oy * s - p + t // k, ox * s - p + t % k
                if 0 <= iy < h and 0 <= ix < w:
                    want[:, oy, ox, t] = x[:, iy, ix, 0]
    assert np.array_equal(want, GH.gconv_ref(x, wt, None, 1, s, p).astype(np.float32))
    for dtype in (hiplib.FP32, hiplib.BF16, hiplib.FP16):
        got = hiplib.op_conv2d(x, _hwio(wt), None, stride=s, act=0, dtype=dtype, padding=p)
        assert np.array_equal(got, want), (dtype, np.argwhere(got != want)[:5])


# ---- 4: every tile id ----
@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=[_IDS[2], _IDS[4]])
def test_every_tile_id_refuses_or_agrees(hiplib, conv_data, case):
    """bf16: each tile id either raises (it has no row / column mask form: running it on a conv of more than 25 taps would read the wrong
    taps silently) or returns what the default id returns, within the 16-bit bound"""
    k, s, p, h, w, cin, cout = case
    x, wt, b, _ = conv_data[case]
    want = _leaky(GH.gconv_ref(_bf16(x), _bf16(wt), b, 1, s, p))
    base = hiplib.op_conv2d(x, _hwio(wt), b, stride=s, act=1, dtype=hiplib.BF16, padding=p)
    _within(hiplib, base, want, hiplib.BF16, "default id")
    ran = []
    for cfg in range(hiplib.op_conv_num_cfgs()):
        try:
            got = hiplib.op_conv2d(x, _hwio(wt), b, stride=s, act=1, dtype=hiplib.BF16, tile_cfg=cfg, padding=p)
        except hiplib.YoloError:
            continue
        _within(hiplib, got, want, hiplib.BF16, "tile id %d" % cfg)
        ran.append(cfg)
    print("tile ids that ran:", ran)
    assert len(ran) >= 2


# ---- 5: mini_wide against the compiled reference ----
def _engine(hiplib, g, dtype, keep=False, batch=N):
    eng = hiplib.Engine(str(g["cfg"]), max_batch=batch, dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
    assert eng.weights_count() == g["weights"].size
    eng.set_weights(g["weights"])
    return eng


def test_mini_wide_matches_compiled_reference_fp32(hiplib):
    """every layer of the reference's own C forward pass, fp32 device path: within MARGIN_TOL of that layer's largest value; the plan that
    keeps every layer and the production plan give the same probabilities; batch 3 in one call equals three calls"""
    g = golden("mini_wide.npz")
    secs = IO.parse_cfg(str(g["cfg"]))[1:]
    probs = []
    for keep in (True, False):
        eng = _engine(hiplib, g, hiplib.FP32, keep)
        p = eng.classify(g["images_u8"], top_k=0)
        if keep:
            for i, s in enumerate(secs):
                got = eng.layer_output(i, N); ref = g["layer_%02d" % i]
                assert got.reshape(N, -1).shape == ref.reshape(N, -1).shape
                r = _relmax(got.reshape(N, -1), ref.reshape(N, -1))
                print("mini_wide layer %d (%s size=%s): relmax %.3e" % (i, s["type"], s.get("size", "-"), r))
                assert r < MARGIN_TOL, "layer %d (%s)" % (i, s["type"])
        else:
            singles = np.concatenate([eng.classify(g["images_u8"][b:b + 1], top_k=0) for b in range(N)])
            assert np.array_equal(singles, p)
        probs.append(p)
        eng.close()
    assert np.array_equal(probs[0], probs[1])
    assert _relmax(probs[0], g["layer_%02d" % (len(secs) - 1)]) < MARGIN_TOL


def _check16(hiplib, g, eng, dtype_name):
    n = len(IO.parse_cfg(str(g["cfg"]))) - 1
    cls, _ = eng.classify(g["images_u8"], top_k=1)
    logit_map, pooled = eng.layer_output(n - 3, N), eng.layer_output(n - 2, N).reshape(N, -1)
    want_map, want = g["layer_%02d" % (n - 3)], g["layer_%02d" % (n - 2)]
    bound = TOL16[dtype_name] * float(np.abs(want_map).max())
    print("mini_wide %s: logit map max err / bound %.3f, pooled %.3f" % (dtype_name, float(np.abs(logit_map - want_map).max() / bound), float(np.abs(pooled - want).max() / bound)))
    assert np.abs(logit_map.astype(np.float64) - want_map).max() <= bound
    assert np.abs(pooled.astype(np.float64) - want).max() <= TOL16[dtype_name] * float(np.abs(want).max())
    assert np.array_equal(np.asarray(cls).reshape(N), np.argmax(want, axis=-1))


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_mini_wide_16bit(hiplib, dtype_name):
    """bf16 / fp16 storage against the FIXTURE: the logit map (the class conv's fp32 store) and the pooled logits within TOL16 of the largest
    logit; top-1 equal to the reference's on all three images (their margins: test_wide_host.py); the production plan gives the
    keep-layers plan's probabilities"""
    dtype = getattr(hiplib, dtype_name.upper())
    g = golden("mini_wide.npz")
    eng = _engine(hiplib, g, dtype, keep=True)
    _check16(hiplib, g, eng, dtype_name)
    p = eng.classify(g["images_u8"], top_k=0)
    eng.close()
    e2 = _engine(hiplib, g, dtype, keep=False)
    assert np.array_equal(e2.classify(g["images_u8"], top_k=0), p)
    e2.close()


def test_mini_wide_autotuned_bf16(hiplib):
    """after the in-situ autotune at batch 3 every conv of more than 25 taps still runs an id with the row / column mask form: the logits stay
    inside the bound"""
    g = golden("mini_wide.npz")
    eng = _engine(hiplib, g, hiplib.BF16, keep=True)
    eng.autotune(N, iters=1)
    print("tuned ids:", list(eng.resolved_tile_configs(N)))
    _check16(hiplib, g, eng, "bf16")
    eng.close()


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_mini_wide_export_round_trip(hiplib, tmp_path, dtype_name):
    g = golden("mini_wide.npz")
    eng = _engine(hiplib, g, getattr(hiplib, dtype_name.upper()))
    p = eng.classify(g["images_u8"], top_k=0)
    path = str(tmp_path / "mini_wide.yolohip")
    eng.export(path)
    e2 = hiplib.Engine.from_file(path, max_batch=N)
    assert e2.rows == 0 and e2.num_classes == 10
    assert np.array_equal(e2.classify(g["images_u8"], top_k=0), p)
    e2.close(); eng.close()


# ---- the window store ----
_C = lambda f, k: "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=%d\nstride=1\npad=1\nactivation=leaky\n\n" % (f, k)
_MAP_NET = "[net]\nwidth=12\nheight=10\nchannels=3\nyolo_output=map\n\n"
WINDOW = _MAP_NET + _C(16, 3) + _C(8, 3) + "[route]\nlayers=0\n\n" + _C(16, 9) + "[route]\nlayers=0\n\n" + _C(8, 1) + "[route]\nlayers=1,3,5\n"


def _map_of(hiplib, cfg, flat, img, dtype):
    eng = hiplib.Engine(cfg, max_batch=img.shape[0], dtype=dtype, semantics=hiplib.SEM_DARKNET)
    assert eng.weights_count() == flat.size
    eng.set_weights(flat)
    eng.forward(img, want_detections=False)
    m = eng.output_map(img.shape[0])
    eng.close()
    return m


@pytest.mark.parametrize("dtype_name", ["bf16", "fp32"])
def test_wide_conv_writes_into_the_middle_of_a_concat_buffer(hiplib, dtype_name):
    """a dense 3x3 conv, a 9x9 conv and a dense 1x1 conv of one tensor write the three windows of a [route]'s buffer, the 9x9 one in the
    middle (channels 8 .. 24 of 32).  The channels on both sides are bit for bit what networks WITHOUT the 9x9 conv give, and the middle
    is the 9x9 conv of layer 0's tensor."""
    dtype = getattr(hiplib, dtype_name.upper())
    rc, table = hiplib.plan_table(WINDOW, dtype=dtype, max_batch=N)
    rows = table.splitlines(); st = lambda i: next(v for v in rows[i].split() if v.startswith("storage="))
    assert rc == 0 and st(1) == st(3) == st(5) == st(6)
    secs = IO.parse_cfg(WINDOW)
    flat = IO.synth_weights(secs, seed=181)
    img = np.random.default_rng(182).integers(0, 256, (N, 10, 12, 3), dtype=np.uint8)
    whole = _map_of(hiplib, WINDOW, flat, img, dtype)
    assert whole.shape == (N, 10, 12, 32)
    n = [c["filters"] * 4 + c["filters"] * c["cin"] * c["size"] ** 2 for c in IO.conv_specs(secs)]
    off = np.concatenate([[0], np.cumsum(n)])
    left = _map_of(hiplib, _MAP_NET + _C(16, 3) + _C(8, 3), flat[:off[2]], img, dtype)
    right = _map_of(hiplib, _MAP_NET + _C(16, 3) + _C(8, 1), np.concatenate([flat[:off[1]], flat[off[3]:off[4]]]), img, dtype)
    stem = _map_of(hiplib, _MAP_NET + _C(16, 3), flat[:off[1]], img, dtype)
    # (the cut networks' last conv is their map's producer and stores fp32: rounded once to the storage type it is the window's content)
    assert np.array_equal(whole[..., :8], _stored(hiplib, left, dtype)) and np.array_equal(whole[..., 24:], _stored(hiplib, right, dtype))
    stem = _stored(hiplib, stem, dtype)
    prm, w = GH.layer_params(secs, flat)[3]
    beta, gamma, mean, var = prm.astype(np.float64)
    y = (GH.gconv_ref(stem, _stored(hiplib, w * (gamma / (np.sqrt(var) + 1e-6))[:, None, None, None].astype(np.float32), dtype), None, 1, 1, 4) + (beta - mean * gamma / (np.sqrt(var) + 1e-6)))
    want = np.where(y > 0, y, 0.1 * y)
    err = np.abs(whole[..., 8:24].astype(np.float64) - want)
    assert np.abs(want).max() > 0.5
    assert (err <= (2.0 ** -7 * np.abs(want) + 2e-3 if dtype == hiplib.BF16 else 1e-4 * np.abs(want).max())).all()


# ---- 6: AlexNet through the Classifier ----
def test_alexnet_classifier(hiplib):
    """cfg/zoo/alexnet.cfg through Classifier with synthetic weights at batch 2, bf16"""
    from yolo_tensorflow_amd.classifier import Classifier
    clf = Classifier("alexnet", dtype=hiplib.BF16, max_batch=2)
    assert clf.num_classes == 1000 and clf.engine.size == 227
    img = np.random.default_rng(19).integers(0, 256, (2, 227, 227, 3), dtype=np.uint8)
    p = clf.engine.classify(img, top_k=0)
    recs = clf.classify_from_images(list(img), top=3)
    clf.close()
    assert p.shape == (2, 1000) and np.isfinite(p).all()
    assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 1e-3
    for b in range(2):
        assert [k for k, _ in recs[b]] == [int(k) for k in np.argsort(-p[b], kind="stable")[:3]]


# ---- 7: a 9-1-5 map network ----
def test_srcnn_style_map_network_fp32(hiplib):
    """three convs 9-1-5 (relu, relu, linear; bias, no batch norm) at 12 x 10 with yolo_output=map, fp32, against the float64 restatement
    within 1e-4 of the map's largest value"""
    conv = lambda f, k, act: "[convolutional]\nfilters=%d\nsize=%d\nstride=1\npad=1\nactivation=%s\n\n" % (f, k, act)
    cfg = _MAP_NET + conv(16, 9, "relu") + conv(8, 1, "relu") + conv(3, 5, "linear")
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=191)
    img = np.random.default_rng(192).integers(0, 256, (N, 10, 12, 3), dtype=np.uint8)
    got = _map_of(hiplib, cfg, flat, img, hiplib.FP32)
    params = GH.layer_params(secs, flat)
    y = img.astype(np.float32) / np.float32(255.0)
    for i, act in ((0, "relu"), (1, "relu"), (2, "linear")):
        prm, w = params[i]
        y = GH.ACTS[act](GH.gconv_ref(y, w, prm[0], 1, 1, w.shape[2] // 2))
    assert got.shape == y.shape == (N, 10, 12, 3)
    r = _relmax(got, y)
    print("9-1-5 map network fp32: relmax %.3e" % r)
    assert r < 1e-4
