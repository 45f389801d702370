"""[convolutional] with groups= on the device: the grouped kernel (gconv.hip) against the float64 restatement of test_grouped_host.py (where
it is checked against the reference's recorded layers), exact integer counts that a dropped tap, a non-zero off-diagonal filter entry or
a read of a neighbouring group's channels would break, the window store, two whole networks against the reference's own C code
(tests/golden/mini_grouped.npz, mini_dw_v3.npz), and the public surface (export, Classifier, resnext50.cfg)."""
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
import test_grouped_host as GH

pytestmark = pytest.mark.gpu

MARGIN_TOL = 5e-4                            # the fp32 bound of the network tests, as a share of the tensor's largest value
TOL16 = {"bf16": 3e-2, "fp16": 4e-3}         # the factors of test_gpu_resnet.py / test_gpu_unet.py, as a share of the largest logit


def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _stored(hiplib, x, dtype):
    return _bf16(x) if dtype == hiplib.BF16 else np.asarray(x, np.float32).astype(np.float16).astype(np.float32) if dtype == hiplib.FP16 else np.asarray(x, dtype=np.float32)


def _relmax(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / (np.abs(b).max() + 1e-12))


# ---- 1: op_conv2d_grouped ----
GCONV_CASES = [          # (size, stride, pad, h, w, cin, cout, groups)
    (3, 1, 1, 7, 9, 16, 16, 4),          # 4 groups per bundle
    (3, 1, 1, 7, 9, 16, 16, 16),         # depthwise
    (3, 2, 1, 7, 9, 24, 24, 24),         # depthwise, stride 2, odd extents, a trailing bundle of 8 groups
    (3, 1, 1, 5, 6, 16, 32, 16),         # channel multiplier 2
    (3, 1, 1, 5, 6, 24, 40, 8),          # cg 3, m 5: one short bundle
    (3, 2, 0, 8, 8, 12, 20, 4),          # C no multiple of 8, a ragged store, no padding
    (1, 1, 0, 13, 9, 64, 64, 2),         # 1x1
    (3, 1, 1, 6, 5, 64, 64, 2),          # several K-steps
    (5, 1, 2, 6, 7, 16, 16, 2),          # five taps across
    (3, 1, 1, 9, 13, 72, 72, 9),         # several pixel tiles, an odd bundle count
    (3, 1, 1, 7, 9, 24, 40, 1),          # groups=1: the same kernel with one group
]
_IDS = ["k%ds%dp%d_%dx%d_%dto%d_g%d" % c for c in GCONV_CASES]


@pytest.fixture(scope="module")
def gconv_data():
    """operands per case, drawn once"""
    rng = np.random.default_rng(71)
    data = {}
    for case in GCONV_CASES:
        k, s, p, h, w, cin, cout, groups = case
        x = rng.standard_normal((3, h, w, cin)).astype(np.float32)
        wt = (rng.standard_normal((cout, cin // groups, k, k)) / np.sqrt(cin // groups * k * k)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        data[case] = (x, wt, b)
    return data


@pytest.mark.parametrize("case", GCONV_CASES, ids=_IDS)
def test_op_conv2d_grouped(hiplib, gconv_data, case):
    """batch 3, with bias, leaky, against float64 on operands pre-rounded to the storage type, with the bounds of
    test_gpu_unet.py::test_op_deconv2d: fp32 1e-4 of the tensor's largest value; bf16 2^-7 |want| + 2e-3; fp16 2^-10 |want| + 2e-3; the
    fp32 ("head") store of the 16-bit kernels under the 16-bit bound too."""
    k, s, p, h, w, cin, cout, groups = case
    x, wt, b = gconv_data[case]
    for dtype, name in ((hiplib.FP32, "fp32"), (hiplib.BF16, "bf16"), (hiplib.FP16, "fp16")):
        y = GH.gconv_ref(_stored(hiplib, x, dtype), _stored(hiplib, wt, dtype), b, groups, s, p)
        want = np.where(y > 0, y, np.float64(np.float32(0.1)) * y)
        for out_f32 in ((False,) if dtype == hiplib.FP32 else (False, True)):
            got = hiplib.op_conv2d_grouped(x, wt, b, groups=groups, stride=s, padding=p, activation="leaky", dtype=dtype, out_f32=out_f32)
            assert got.shape == want.shape and got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - want)
            if dtype == hiplib.FP32:
                r = float(err.max() / np.abs(want).max())
                print("gconv %s fp32: relmax %.3e" % (_IDS[GCONV_CASES.index(case)], r))
                assert r < 1e-4
            else:
                bound = 2.0 ** (-7 if dtype == hiplib.BF16 else -10) * np.abs(want) + 2e-3
                print("gconv %s %s out_f32 %d: max err / bound %.3f" % (_IDS[GCONV_CASES.index(case)], name, out_f32, float((err / bound).max())))
                assert (err <= bound).all(), "%s: %g over at %r" % (name, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))


@pytest.mark.parametrize("case", GCONV_CASES, ids=_IDS)
def test_op_conv2d_grouped_counts_exactly(hiplib, case):
    """all-ones operands, linear, no bias, the fp32 store: every product is 1 and the fp32 accumulator holds integers, so the result is
    EXACTLY cg x (taps inside the image) -- a tap dropped at a border, or a non-zero filter entry off a bundle's diagonal, shows as a whole
    unit.  The 16-bit store is that integer rounded once to the storage type."""
    k, s, p, h, w, cin, cout, groups = case
    x = np.ones((3, h, w, cin), np.float32); wt = np.ones((cout, cin // groups, k, k), np.float32)
    taps = GH.taps_inside(h, w, k, s, p)
    want = np.broadcast_to((taps * (cin // groups)).astype(np.float32)[None, :, :, None], (3,) + taps.shape + (cout,))
    for dtype in (hiplib.BF16, hiplib.FP16, hiplib.FP32):
        got = hiplib.op_conv2d_grouped(x, wt, None, groups=groups, stride=s, padding=p, activation="linear", dtype=dtype, out_f32=True)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    for dtype in (hiplib.BF16, hiplib.FP16):
        got = hiplib.op_conv2d_grouped(x, wt, None, groups=groups, stride=s, padding=p, activation="linear", dtype=dtype)
        assert np.array_equal(got, _stored(hiplib, want, dtype))


@pytest.mark.parametrize("case", GCONV_CASES, ids=_IDS)
def test_op_conv2d_grouped_isolates_the_groups(hiplib, case):
    """input channel c holds the constant 1 + c // cg, the filters are ones: the outputs of group g are exactly (g + 1) cg taps (at most
    25 x 32 x 25 < 2^24, and 1 + g <= 25 is a bf16 and an fp16 number) -- a kernel that reads a neighbouring group's channels cannot pass"""
    k, s, p, h, w, cin, cout, groups = case
    cg, m = cin // groups, cout // groups
    x = np.broadcast_to((1 + np.arange(cin) // cg).astype(np.float32), (3, h, w, cin)).copy()
    wt = np.ones((cout, cg, k, k), np.float32)
    taps = GH.taps_inside(h, w, k, s, p)
    want = (taps[None, :, :, None] * (cg * (1 + np.arange(cout) // m))[None, None, None, :]).astype(np.float32)
    want = np.broadcast_to(want, (3,) + want.shape[1:])
    assert want.max() < 2 ** 24
    for dtype in (hiplib.BF16, hiplib.FP16, hiplib.FP32):
        got = hiplib.op_conv2d_grouped(x, wt, None, groups=groups, stride=s, padding=p, activation="linear", dtype=dtype, out_f32=True)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_op_conv2d_grouped_post_activation(hiplib):
    """an activation outside the slope family: a linear epilogue, then k_activate (what plan_activation plans)"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 4, 5, 8)).astype(np.float32); wt = (rng.standard_normal((16, 2, 3, 3)) * 0.3).astype(np.float32)
    want = np.tanh(GH.gconv_ref(x, wt, None, 4, 1, 1))
    got = hiplib.op_conv2d_grouped(x, wt, None, groups=4, stride=1, padding=1, activation="tanh", dtype=hiplib.FP32)
    assert np.abs(got - want).max() < 1e-5


# ---- 2: the window store ----
_C = lambda f, k, g=1, extra="": "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=%d\nstride=1\npad=1\n%sactivation=leaky\n\n" % (f, k, ("groups=%d\n" % g if g != 1 else "") + extra)
_MAP_NET = "[net]\nwidth=12\nheight=10\nchannels=3\nyolo_output=map\n\n"
WINDOW = _MAP_NET + _C(16, 3) + _C(8, 3) + "[route]\nlayers=0\n\n" + _C(16, 3, 4) + "[route]\nlayers=0\n\n" + _C(8, 1) + "[route]\nlayers=1,3,5\n"


def _map_of(hiplib, cfg, flat, img, dtype):
    eng = hiplib.Engine(cfg, max_batch=img.shape[0], dtype=dtype, semantics=hiplib.SEM_DARKNET)
    assert eng.weights_count() == flat.size
    eng.set_weights(flat)
    eng.forward(img, want_detections=False)
    m = eng.output_map(img.shape[0])
    eng.close()
    return m


@pytest.mark.parametrize("dtype_name", ["bf16", "fp32"])
def test_gconv_writes_into_the_middle_of_a_concat_buffer(hiplib, dtype_name):
    """a dense 3x3 conv, a grouped conv and a dense 1x1 conv of one tensor write the three windows of a [route]'s buffer, the grouped one
    in the middle (channels 8 .. 24 of 32).  The channels on both sides are bit for bit what networks WITHOUT the grouped conv give, and
    the middle is the grouped conv of layer 0's tensor."""
    dtype = getattr(hiplib, dtype_name.upper())
    rc, table = hiplib.plan_table(WINDOW, dtype=dtype, max_batch=3)
    rows = table.splitlines(); st = lambda i: next(v for v in rows[i].split() if v.startswith("storage="))
    assert rc == 0 and st(1) == st(3) == st(5) == st(6)
    secs = IO.parse_cfg(WINDOW)
    flat = IO.synth_weights(secs, seed=81)
    img = np.random.default_rng(82).integers(0, 256, (3, 10, 12, 3), dtype=np.uint8)
    whole = _map_of(hiplib, WINDOW, flat, img, dtype)
    assert whole.shape == (3, 10, 12, 32)
    n = [c["filters"] * 4 + c["filters"] * (c["cin"] // c["groups"]) * c["size"] ** 2 for c in IO.conv_specs(secs)]
    off = np.concatenate([[0], np.cumsum(n)])
    left = _map_of(hiplib, _MAP_NET + _C(16, 3) + _C(8, 3), flat[:off[2]], img, dtype)
    right = _map_of(hiplib, _MAP_NET + _C(16, 3) + _C(8, 1), np.concatenate([flat[:off[1]], flat[off[3]:off[4]]]), img, dtype)
    stem = _map_of(hiplib, _MAP_NET + _C(16, 3), flat[:off[1]], img, dtype)
    # (the cut networks' last conv is their map's producer and stores fp32: rounded once to the storage type it is the window's content)
    assert np.array_equal(whole[..., :8], _stored(hiplib, left, dtype)) and np.array_equal(whole[..., 24:], _stored(hiplib, right, dtype))
    stem = _stored(hiplib, stem, dtype)
    prm, w = GH.layer_params(secs, flat)[3]
    beta, gamma, mean, var = prm.astype(np.float64)
    y = (GH.gconv_ref(stem, _stored(hiplib, w * (gamma / (np.sqrt(var) + 1e-6))[:, None, None, None].astype(np.float32), dtype), None, 4, 1, 1) + (beta - mean * gamma / (np.sqrt(var) + 1e-6)))
    want = np.where(y > 0, y, 0.1 * y)
    err = np.abs(whole[..., 8:24].astype(np.float64) - want)
    assert np.abs(want).max() > 0.5
    assert (err <= (2.0 ** -7 * np.abs(want) + 2e-3 if dtype == hiplib.BF16 else 1e-4 * np.abs(want).max())).all()


# ---- 3: whole networks against the compiled reference ----
def _engine(hiplib, g, dtype, keep=False, batch=3):
    eng = hiplib.Engine(str(g["cfg"]), max_batch=batch, dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
    assert eng.weights_count() == g["weights"].size
    eng.set_weights(g["weights"])
    return eng


def test_mini_grouped_matches_compiled_reference_fp32(hiplib):
    """every layer of the reference's own C forward pass, fp32 device path: within MARGIN_TOL of that layer's largest value; the plan that
    keeps every layer and the production plan give the same probabilities; batch 3 in one call equals three calls"""
    g = golden("mini_grouped.npz")
    secs = IO.parse_cfg(str(g["cfg"]))[1:]
    probs = []
    for keep in (True, False):
        eng = _engine(hiplib, g, hiplib.FP32, keep)
        p = eng.classify(g["images_u8"], top_k=0)
        if keep:
            for i, s in enumerate(secs):
                got = eng.layer_output(i, 3); ref = g["layer_%02d" % i]
                assert got.reshape(3, -1).shape == ref.reshape(3, -1).shape
                r = _relmax(got.reshape(3, -1), ref.reshape(3, -1))
                print("mini_grouped layer %d (%s groups=%s %s): relmax %.3e" % (i, s["type"], s.get("groups", "-"), s.get("activation", ""), r))
                assert r < MARGIN_TOL, "layer %d (%s)" % (i, s["type"])
        else:
            singles = np.concatenate([eng.classify(g["images_u8"][b:b + 1], top_k=0) for b in range(3)])
            assert np.array_equal(singles, p)
        probs.append(p)
        eng.close()
    assert np.array_equal(probs[0], probs[1])
    assert _relmax(probs[0], g["layer_%02d" % (len(secs) - 1)]) < MARGIN_TOL


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_mini_grouped_16bit(hiplib, dtype_name):
    """bf16 / fp16 storage against the FIXTURE: the logit map (the grouped 1x1's fp32 store) and the pooled logits within TOL16 of the
    largest logit; top-1 equal to the reference's on every image whose two largest pooled logits differ by more than twice that bound
    -- all three, which the generator asserted and test_grouped_host.py checks again"""
    dtype = getattr(hiplib, dtype_name.upper())
    g = golden("mini_grouped.npz")
    n = len(IO.parse_cfg(str(g["cfg"]))) - 1
    eng = _engine(hiplib, g, dtype, keep=True)
    cls, top = eng.classify(g["images_u8"], top_k=1)
    logit_map, pooled = eng.layer_output(n - 3, 3), eng.layer_output(n - 2, 3).reshape(3, -1)
    eng.close()
    want_map, want = g["layer_%02d" % (n - 3)], g["layer_%02d" % (n - 2)]
    bound = TOL16[dtype_name] * float(np.abs(want_map).max())
    print("mini_grouped %s: logit map max err / bound %.3f, pooled %.3f" % (dtype_name, float(np.abs(logit_map - want_map).max() / bound), float(np.abs(pooled - want).max() / bound)))
    assert np.abs(logit_map.astype(np.float64) - want_map).max() <= bound
    assert np.abs(pooled.astype(np.float64) - want).max() <= TOL16[dtype_name] * float(np.abs(want).max())
    top2 = np.sort(want, axis=-1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > 2 * TOL16[dtype_name] * float(np.abs(want).max())
    assert sure.all()
    assert np.array_equal(np.asarray(cls).reshape(3)[sure], np.argmax(want, axis=-1)[sure])
    # the production plan gives the same probabilities
    e2 = _engine(hiplib, g, dtype, keep=False)
    e3 = _engine(hiplib, g, dtype, keep=True)
    assert np.array_equal(e2.classify(g["images_u8"], top_k=0), e3.classify(g["images_u8"], top_k=0))
    e2.close(); e3.close()


def test_mini_dw_v3_matches_compiled_reference(hiplib):
    """the depthwise-separable two-head detector: every layer in fp32 within MARGIN_TOL, and the decoded candidates against
    get_network_boxes of the compiled reference as test_gpu_network.py compares mini_v3.npz, with its thresholds"""
    g = golden("mini_dw_v3.npz")
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET, keep_layers=True)
    eng.set_weights(g["weights"])
    eng.forward(g["image_u8"][None], scale=1.0 / 255.0)
    for i, s in enumerate(IO.parse_cfg(str(g["cfg"]))[1:]):
        if s["type"] == "yolo":
            continue
        got = eng.layer_output(i, 1); ref = g["layer_%02d" % i]
        assert got.shape == ref.shape
        assert _relmax(got, ref) < MARGIN_TOL, "layer %d (%s)" % (i, s["type"])
    eng.close()
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(g["weights"])
    det = eng.forward(g["image_u8"][None])[0]
    keep = det[:, 4] > float(g["thresh"])
    assert keep.sum() == len(g["boxes_raw"])
    np.testing.assert_allclose(det[keep, :4], g["boxes_raw"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(det[keep, 4], g["obj_raw"], rtol=2e-3, atol=2e-4)
    eng.close()


def test_mini_dw_v3_bf16_tracks_reference(hiplib):
    g = golden("mini_dw_v3.npz")
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.BF16, semantics=hiplib.SEM_DARKNET, keep_layers=True)
    eng.set_weights(g["weights"])
    eng.forward(g["image_u8"][None])
    for i, s in enumerate(IO.parse_cfg(str(g["cfg"]))[1:]):
        if s["type"] != "yolo":          # bf16 storage compounding over the layers: the bound of test_mini_network_bf16_tracks_reference
            assert _relmax(eng.layer_output(i, 1), g["layer_%02d" % i]) < 3e-2, "layer %d" % i
    eng.close()


# ---- 4: surface ----
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_export_round_trip(hiplib, tmp_path, dtype_name):
    g = golden("mini_grouped.npz")
    eng = _engine(hiplib, g, getattr(hiplib, dtype_name.upper()))
    p = eng.classify(g["images_u8"], top_k=0)
    path = str(tmp_path / "mini_grouped.yolohip")
    eng.export(path)
    e2 = hiplib.Engine.from_file(path, max_batch=3)
    assert e2.rows == 0 and e2.num_classes == 24
    assert np.array_equal(e2.classify(g["images_u8"], top_k=0), p)
    e2.close(); eng.close()


def test_classifier_over_mini_grouped(hiplib, tmp_path):
    """the Classifier class over a grouped cfg and a .weights file: the same top-k as Engine.classify"""
    from yolo_tensorflow_amd.classifier import Classifier
    g = golden("mini_grouped.npz")
    path = str(tmp_path / "mini_grouped.weights")
    IO.write_weights_file(path, g["weights"])
    clf = Classifier(str(g["cfg"]), weights_file=path, dtype=hiplib.BF16, max_batch=3)
    recs = clf.classify_from_images(list(g["images_u8"]), top=5)
    clf.close()
    eng = _engine(hiplib, g, hiplib.BF16)
    cls, probs = eng.classify(g["images_u8"], top_k=5)
    eng.close()
    assert [[k for k, _ in r] for r in recs] == [[int(k) for k in row] for row in cls]
    assert [[q for _, q in r] for r in recs] == [[float(q) for q in row] for row in probs]


def test_resnext50_classifier(hiplib):
    """the whole library once: resnext50.cfg through Classifier with synthetic weights at batch 2"""
    from yolo_tensorflow_amd.classifier import Classifier
    clf = Classifier("resnext50", dtype=hiplib.BF16, max_batch=2)
    assert clf.num_classes == 1000 and clf.engine.size == 256
    img = np.random.default_rng(9).integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)
    p = clf.engine.classify(img, top_k=0)
    recs = clf.classify_from_images(list(img), top=3)
    clf.close()
    assert p.shape == (2, 1000) and np.isfinite(p).all()
    assert np.abs(p.astype(np.float64).sum(axis=1) - 1).max() <= 1e-3
    assert [k for k, _ in recs[0]] == [int(k) for k in np.argsort(-p[0], kind="stable")[:3]]
