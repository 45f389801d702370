"""Dense-prediction networks on the device: the transposed-convolution kernel (deconv.hip) against a float64 restatement, [l2norm],
darknet's [upsample], the label kernels, two whole map networks against the reference's own C code (tests/golden/mini_unet.npz,
mini_deconv_odd.npz), the ragged native-size segmentation path and the public surface (Segmenter, export, the darknet veneer).
The restatements live in test_unet_host.py, where they are checked against the reference's recorded layers."""
import ctypes as C
import os
import numpy as np
import pytest
from conftest import golden
from oracle import darknet_ref as DR
from yolo_tensorflow_amd import darknet_io as IO
import test_unet_host as UH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_DIR = os.path.join(ROOT, "tests", "golden", "images")
U = 2.0 ** -24
FIXTURES = ("mini_unet.npz", "mini_deconv_odd.npz")
# what a 16-bit network's pre-activation map may stand off from the fixture by, as a share of that tensor's largest value: the factors
# of test_gpu_resnet.py::test_mini_resnet_fused_plan_equals_layer_by_layer_plan (3e-2 of the largest logit in bf16, 4e-3 in fp16)
TOL16 = {"bf16": 3e-2, "fp16": 4e-3}
SURE_FLOOR = {"bf16": 0.65, "fp16": 0.95}          # the least share of the output pixels the 16-bit label comparison must cover


def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _stored(hiplib, x, dtype):
    return _bf16(x) if dtype == hiplib.BF16 else np.asarray(x, np.float32).astype(np.float16).astype(np.float32) if dtype == hiplib.FP16 else np.asarray(x, dtype=np.float32)


# ---- 1: op_deconv2d ----
DECONV_CASES = [          # (size, stride, pad, h, w, cin, cout)
    (4, 2, 1, 5, 7, 24, 16),
    (2, 2, 0, 5, 7, 24, 16),
    (3, 1, 1, 13, 9, 16, 40),
    (3, 2, 1, 5, 7, 20, 5),          # ragged channels, an odd output extent
    (3, 2, 0, 4, 4, 8, 8),
    (5, 3, 2, 6, 5, 8, 24),
    (1, 2, 0, 5, 7, 16, 16),         # empty phases
    (1, 1, 0, 13, 9, 136, 8),        # more than two K-steps
    (6, 2, 2, 9, 13, 72, 72),        # nine taps per phase, several K-steps, more than one pixel tile
]
_IDS = ["k%ds%dp%d_%dx%d_%dto%d" % c for c in DECONV_CASES]


@pytest.fixture(scope="module")
def deconv_data():
    """operands and the float64 restatement per case and storage type, computed once"""
    rng = np.random.default_rng(61)
    data = {}
    for case in DECONV_CASES:
        k, s, p, h, w, cin, cout = case
        x = rng.standard_normal((3, h, w, cin)).astype(np.float32)
        wt = (rng.standard_normal((cin, cout, k, k)) / np.sqrt(cin * max(k * k / (s * s), 1.0))).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        data[case] = (x, wt, b)
    return data


@pytest.mark.parametrize("case", DECONV_CASES, ids=_IDS)
def test_op_deconv2d(hiplib, deconv_data, case):
    """batch 3, with bias, against float64 on operands pre-rounded to the storage type.  fp32: rtol 1e-4 of the tensor's scale
    (test_conv_fp32_exact_path); bf16: 2^-7 |want| + 2e-3 (_assert_bf16_close); fp16: the same with 2^-10.  Leaky, so that the epilogue's
    activation is in the comparison; the fp32 ("head") store of the 16-bit kernels under the 16-bit bound too."""
    k, s, p, h, w, cin, cout = case
    x, wt, b = deconv_data[case]
    for dtype, name in ((hiplib.FP32, "fp32"), (hiplib.BF16, "bf16"), (hiplib.FP16, "fp16")):
        y = UH.deconv_ref(_stored(hiplib, x, dtype), _stored(hiplib, wt, dtype), b, s, p)
        want = np.where(y > 0, y, np.float64(np.float32(0.1)) * y)
        for out_f32 in ((False,) if dtype == hiplib.FP32 else (False, True)):
            got = hiplib.op_deconv2d(x, wt, b, stride=s, padding=p, activation="leaky", dtype=dtype, out_f32=out_f32)
            assert got.shape == want.shape and got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - want)
            if dtype == hiplib.FP32:
                r = float(err.max() / np.abs(want).max())
                print("deconv %s fp32: relmax %.3e" % (_IDS[DECONV_CASES.index(case)], r))
                assert r < 1e-4
            else:
                bound = 2.0 ** (-7 if dtype == hiplib.BF16 else -10) * np.abs(want) + 2e-3
                print("deconv %s %s out_f32 %d: max err / bound %.3f" % (_IDS[DECONV_CASES.index(case)], name, out_f32, float((err / bound).max())))
                assert (err <= bound).all(), "%s: %g over at %r" % (name, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))


@pytest.mark.parametrize("case", DECONV_CASES, ids=_IDS)
def test_op_deconv2d_counts_taps_exactly(hiplib, case):
    """act linear, all-ones operands, no bias, 16-bit: every product is 1 and the fp32 accumulator holds integers, so the result is the
    integer cin x (taps that land on the pixel) EXACTLY -- a tap counted twice or dropped at a phase border shows as a whole unit.  The
    fp32 store returns the integer itself; the 16-bit store that integer rounded once to the storage type."""
    k, s, p, h, w, cin, cout = case
    x = np.ones((3, h, w, cin), np.float32); wt = np.ones((cin, cout, k, k), np.float32)
    want = np.broadcast_to((UH.tap_counts(h, w, k, s, p) * cin).astype(np.float32)[None, :, :, None], (3, (h - 1) * s + k - 2 * p, (w - 1) * s + k - 2 * p, cout))
    for dtype in (hiplib.BF16, hiplib.FP16):
        got = hiplib.op_deconv2d(x, wt, None, stride=s, padding=p, activation="linear", dtype=dtype, out_f32=True)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        got = hiplib.op_deconv2d(x, wt, None, stride=s, padding=p, activation="linear", dtype=dtype)
        assert np.array_equal(got, _stored(hiplib, want, dtype))


def test_op_deconv2d_post_activation(hiplib):
    """an activation outside the slope family: a linear epilogue, then k_activate (what plan_activation plans)"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 4, 5, 8)).astype(np.float32); wt = (rng.standard_normal((8, 12, 2, 2)) * 0.3).astype(np.float32)
    want = np.tanh(UH.deconv_ref(x, wt, None, 2, 0))
    got = hiplib.op_deconv2d(x, wt, None, stride=2, padding=0, activation="tanh", dtype=hiplib.FP32)
    assert np.abs(got - want).max() < 1e-5


# ---- 2: the small operators ----
@pytest.mark.parametrize("c", [6, 40, 200])
def test_op_l2norm(hiplib, c):
    """fp32 against float64 within (C / 2 + 4) u |y|: C rounded adds under a square root, one division, one rounding.  A planted
    all-zero pixel is NaN on both sides (0 / 0, no epsilon)."""
    rng = np.random.default_rng(c)
    x = rng.standard_normal((3, 5, 7, c)).astype(np.float32)
    x[1, 2, 3, :] = 0
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = x64 / np.sqrt((x64 * x64).sum(axis=-1, keepdims=True))
    got = hiplib.op_l2norm(x)
    assert np.isnan(want[1, 2, 3]).all() and np.isnan(got[1, 2, 3]).all()
    ok = ~np.isnan(want)
    assert not np.isnan(got[ok]).any()
    err = np.abs(got.astype(np.float64) - want)[ok]; bound = ((c / 2 + 4) * U * np.abs(want))[ok]
    print("l2norm C %d: max err / bound %.3f" % (c, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    for dtype in (hiplib.BF16, hiplib.FP16):          # 16-bit storage: the same on the stored input, plus half a unit of the stored result
        xs = _stored(hiplib, x, dtype).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            w16 = xs / np.sqrt((xs * xs).sum(axis=-1, keepdims=True))
        g16 = hiplib.op_l2norm(x, dtype=dtype)
        assert np.isnan(g16[1, 2, 3]).all()
        assert (np.abs(g16.astype(np.float64) - w16)[ok] <= (2.0 ** (-8 if dtype == hiplib.BF16 else -11) * np.abs(w16) + (c / 2 + 4) * U * np.abs(w16) + 2.0 ** -25)[ok]).all()


@pytest.mark.parametrize("stride", [1, 2, 3, 8])
def test_op_upsample(hiplib, stride):
    rng = np.random.default_rng(stride)
    x = rng.standard_normal((3, 3, 5, 12)).astype(np.float32)          # twelve channels: the second granule is half used
    for scale in (1.0, 0.5):
        want = np.repeat(np.repeat(x, stride, axis=1), stride, axis=2) * np.float32(scale)
        got = hiplib.op_upsample(x, stride=stride, scale=scale)
        assert got.shape == want.shape and np.array_equal(got, want)


def test_op_label_map(hiplib):
    """exact equality with numpy on random maps, with planted exact ties (the lowest index wins), a maximum equal to thresh (labelled)
    and maxima just below it (255)"""
    rng = np.random.default_rng(9)
    for c in (1, 6, 37, 255):
        m = rng.random((2, 9, 11, c)).astype(np.float32)
        thresh = np.float32(0.7)
        if c > 1:
            m[0, 0, 0, :] = 0.25; m[0, 0, 0, [c - 1, c // 2]] = 0.9          # an exact tie between two channels
            m[0, 0, 1, :] = 0.8                                               # ... between all of them
        m[0, 1, 0, :] = 0.1; m[0, 1, 0, c - 1] = thresh                       # the maximum equals thresh: labelled
        m[0, 1, 1, :] = 0.1; m[0, 1, 1, 0] = np.nextafter(thresh, np.float32(0))          # just below: 255
        m[1, 3, 3, :] = np.nextafter(thresh, np.float32(0))
        want = np.where(m.max(axis=-1) < thresh, 255, np.argmax(m, axis=-1)).astype(np.uint8)
        got = hiplib.op_label_map(m, thresh=float(thresh))
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert got[0, 1, 0] == c - 1 and got[0, 1, 1] == 255 and got[1, 3, 3] == 255
        if c > 1:
            assert got[0, 0, 0] == c // 2 and got[0, 0, 1] == 0
        assert (want == 255).any() and (want != 255).any()


# ---- 3: whole networks against the compiled reference ----
def _relmax(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / (np.abs(b).max() + 1e-12))


def _engine(hiplib, g, dtype, keep=False, batch=3):
    eng = hiplib.Engine(str(g["cfg"]), max_batch=batch, dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
    assert eng.rows == 0 and eng.weights_count() == g["weights"].size
    eng.set_weights(g["weights"])
    return eng


@pytest.mark.parametrize("name", FIXTURES)
def test_mini_networks_match_compiled_reference_fp32(hiplib, name):
    """Every layer of the reference's own C forward pass, fp32 device path, batch 3: 5e-4 of each tensor's scale, the bound of
    test_mini_resnet_matches_compiled_reference_fp32 for the same two reasons (darknet's sqrt(var) + 1e-6 against the folded
    sqrt(var + 1e-5); the summation order).  The plan that keeps every layer and the production plan (in-place [logistic] /
    [activation], pooled buffers) give the same map bit for bit; the labels equal the reference's arg-max wherever its margin exceeds
    twice the bound, and the excluded share is the fixture's recorded one."""
    g = golden(name)
    secs = IO.parse_cfg(str(g["cfg"]))[1:]
    maps = []
    for keep in (True, False):
        eng = _engine(hiplib, g, hiplib.FP32, keep)
        eng.forward(g["images_u8"], want_detections=False)
        m = eng.output_map(3)
        want = g["layer_%02d" % (len(secs) - 1)]
        assert m.shape == want.shape and eng.map_geometry() == want.shape[1:]
        print("%s keep %d: map relmax %.3e" % (name, keep, _relmax(m, want)))
        assert _relmax(m, want) < 5e-4
        if keep:
            for i, s in enumerate(secs):
                got = eng.layer_output(i, 3); ref = g["layer_%02d" % i]
                assert got.shape == ref.shape
                r = _relmax(got, ref)
                print("%s layer %d (%s %s): relmax %.3e" % (name, i, s["type"], s.get("activation", ""), r))
                assert r < 5e-4, "layer %d (%s)" % (i, s["type"])
        labels = eng.label_map(3, thresh=-1e30)
        sure = g["margin"] > 2 * 5e-4 * float(g["scale"])
        assert np.array_equal(labels[sure], g["argmax"][sure])
        assert np.allclose(1.0 - sure.reshape(3, -1).mean(axis=1), g["tight_share"])
        assert np.array_equal(labels, np.argmax(m, axis=-1))          # ... and the device's own map's arg-max everywhere
        maps.append(m)
        eng.close()
    assert np.array_equal(maps[0], maps[1])


def _final_bound(g, n_layers, tol, last_type):
    """the bound on the final map for a pre-activation map that stands off by tol x its largest value: a linear output layer passes it
    on, [logistic] scales it by its slope s (1 - s) <= 1/4 at the reference's value, widened by e^d for the curvature across d"""
    if last_type == "logistic":
        d = tol * float(np.abs(g["layer_%02d" % (n_layers - 2)]).max())
        s = g["layer_%02d" % (n_layers - 1)].astype(np.float64)
        return s * (1 - s) * d * np.exp(d) + 1e-6
    return np.full(g["layer_%02d" % (n_layers - 1)].shape, tol * float(np.abs(g["layer_%02d" % (n_layers - 1)]).max()))


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_mini_networks_16bit(hiplib, name, dtype_name):
    """bf16 / fp16 storage, both plans, against the FIXTURE (never another device run).  The pre-activation map may stand off by 3e-2
    (bf16) / 4e-3 (fp16) of its largest value, the factors test_mini_resnet_fused_plan_equals_layer_by_layer_plan allows a logit; a
    [logistic] output layer passes that on scaled by its slope (_final_bound).  Labels: equal to the reference's wherever its margin
    exceeds twice that bound; the excluded share is computed from the fixture alone."""
    dtype = getattr(hiplib, dtype_name.upper())
    g = golden(name)
    secs = IO.parse_cfg(str(g["cfg"]))[1:]
    want = g["layer_%02d" % (len(secs) - 1)]
    bound = _final_bound(g, len(secs), TOL16[dtype_name], secs[-1]["type"])
    maps = []
    for keep in (False, True):
        eng = _engine(hiplib, g, dtype, keep)
        eng.forward(g["images_u8"], want_detections=False)
        m = eng.output_map(3)
        err = np.abs(m.astype(np.float64) - want)
        print("%s %s keep %d: max err / bound %.3f" % (name, dtype_name, keep, float((err / bound).max())))
        assert (err <= bound).all()
        labels = eng.label_map(3, thresh=-1e30)
        sure = g["margin"] > 2 * bound.max(axis=-1)
        cap = 1.0 - sure.mean()
        print("%s %s: %.1f %% of the pixels are within twice the bound of a tie and left out" % (name, dtype_name, 100 * cap))
        # `sure` is the fixture's alone (its margins, its values): the comparison below covers at least this share of the pixels --
        # mini_unet 69 % in bf16 and 96 % in fp16, mini_deconv_odd 93 % and 99 %
        assert sure.mean() >= SURE_FLOOR[dtype_name]
        assert np.array_equal(labels[sure], g["argmax"][sure])
        maps.append(m)
        eng.close()
    assert np.array_equal(maps[0], maps[1])


def test_deconv_writes_into_a_concat_window(hiplib):
    """mini_unet layers 3-4, the skip connection: the 4/2/1 deconv and the first stride-2 conv both write into windows of the route's
    buffer.  The route is their concatenation bit for bit, and the conv's half is what that conv gives in a network without the
    deconv (the cfg cut behind layer 2) -- the deconv's stores did not touch its neighbour's channels."""
    g = golden("mini_unet.npz")
    eng = _engine(hiplib, g, hiplib.BF16, keep=True)
    eng.forward(g["images_u8"], want_detections=False)
    conv, dec, route = eng.layer_output(1, 3), eng.layer_output(3, 3), eng.layer_output(4, 3)
    eng.close()
    assert route.shape[-1] == 48 and np.array_equal(route, np.concatenate([dec, conv], axis=-1))
    cfg = str(g["cfg"]); cut = cfg[:cfg.index("[deconvolutional]")]
    n = IO.weights_count(IO.parse_cfg(cut))
    e2 = hiplib.Engine(cut, max_batch=3, dtype=hiplib.BF16, semantics=hiplib.SEM_DARKNET, keep_layers=True)
    e2.set_weights(g["weights"][:n])
    e2.forward(g["images_u8"], want_detections=False)
    alone = e2.layer_output(1, 3)
    e2.close()
    assert np.array_equal(conv, alone) and np.abs(dec).max() > 0


TWO_READERS = ("[net]\nwidth=20\nheight=12\nchannels=3\nyolo_output=map\n\n[convolutional]\nbatch_normalize=1\nfilters=12\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"
               "[activation]\nactivation=tanh\n\n[shortcut]\nfrom=-2\nactivation=relu\n\n[deconvolutional]\nfilters=6\nsize=2\nstride=2\npadding=0\nactivation=linear\n\n[logistic]\n")


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_activation_layer_with_a_second_reader_of_its_producer(hiplib, dtype_name):
    """the conv (12 channels: half a granule of padding) is read by the [activation] AND by the (relu, so unfolded) [shortcut] behind it, so the production
    plan gives the [activation] a tensor of its own in a pooled buffer and copies first, whole granules; the [logistic] at the end has
    its producer to itself and runs in place.  Both plans give the same map bit for bit, and it is tanh and logistic of the kept layers."""
    dtype = getattr(hiplib, dtype_name.upper())
    rc, table = hiplib.plan_table(TWO_READERS, dtype, 3, False)
    assert rc == 0, table
    st = [dict(kv.split("=") for kv in line.split()[2:])["storage"] for line in table.splitlines()[:5]]
    assert st[1] != st[0] and st[4] == st[3]
    flat = IO.synth_weights(IO.parse_cfg(TWO_READERS), seed=6)
    img = np.random.default_rng(4).integers(0, 256, (3, 12, 20, 3), dtype=np.uint8)
    maps = []
    for keep in (True, False):
        eng = hiplib.Engine(TWO_READERS, max_batch=3, dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
        eng.set_weights(flat)
        eng.forward(img, want_detections=False)
        maps.append(eng.output_map(3))
        if keep and dtype == hiplib.FP32:
            a, t, s, d = (eng.layer_output(i, 3) for i in range(4))
            assert np.abs(t - np.tanh(a.astype(np.float64))).max() <= 4 * U and np.array_equal(s, np.maximum(t + a, 0))
            assert np.abs(maps[0] - 1 / (1 + np.exp(-d.astype(np.float64)))).max() <= 4 * U
        eng.close()
    assert np.isfinite(maps[0]).all() and np.array_equal(maps[0], maps[1])


# ---- 4: the ragged native-size path ----
def _native_images():
    rng = np.random.default_rng(77)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((37, 91), (12, 20), (200, 50))]          # the second one: exactly the input's size


@pytest.mark.parametrize("fit_name", ["stretch", "letterbox"])
def test_segment_images(hiplib, fit_name):
    """three images of different native sizes, one of them exactly the input's: segment_images equals label_map of the per-image single
    forward pushed through the numpy integer mapping, exactly"""
    fit = hiplib.FIT_LETTERBOX if fit_name == "letterbox" else hiplib.FIT_STRETCH
    g = golden("mini_unet.npz")
    eng = _engine(hiplib, g, hiplib.FP32)
    imgs = _native_images()
    thresh = float(np.median(g["layer_11"].max(axis=-1)))          # about half of the fixture's pixels are below it: both outcomes occur
    got = eng.segment_images(imgs, fit=fit, thresh=thresh)
    mh, mw, _ = eng.map_geometry()
    assert [a.shape for a in got] == [im.shape[:2] for im in imgs] and all(a.dtype == np.uint8 for a in got)
    for im, lab in zip(imgs, got):
        eng.forward_images([im], fit=fit, want_detections=False)
        single = eng.label_map(1, thresh=thresh)[0]
        my, mx = UH.native_to_map(im.shape[0], im.shape[1], fit_name == "letterbox", eng.input_hw, (mh, mw))
        assert np.array_equal(lab, single[my][:, mx])
        assert set(np.unique(lab)) <= set(range(6)) | {255}
    assert any((a == 255).any() for a in got) and any((a != 255).any() for a in got)
    eng.close()


def test_segmenter_end_to_end(hiplib):
    from PIL import Image
    from yolo_tensorflow_amd.segmenter import Segmenter
    g = golden("mini_unet.npz")
    imgs = [np.ascontiguousarray(np.asarray(Image.open(os.path.join(IMG_DIR, n)).convert("RGB"))) for n in ("dog.jpg", "eagle.jpg", "person.jpg")]
    seg = Segmenter(str(g["cfg"]), g["weights"], max_batch=3, dtype=hiplib.BF16, fit="letterbox")
    maps = seg.predict_from_images(imgs)
    assert len(maps) == 3 and all(m.shape == (24, 40, 6) and m.dtype == np.float32 for m in maps)
    labels = seg.segment_from_images(imgs, thresh=0.5)
    assert [a.shape for a in labels] == [im.shape[:2] for im in imgs]
    assert all(a.dtype == np.uint8 and set(np.unique(a)) <= set(range(6)) | {255} for a in labels)
    for im, m, lab in zip(imgs, maps, labels):          # one at a time: identical
        assert np.array_equal(seg.predict_from_images([im])[0], m)
        assert np.array_equal(seg.segment_from_images([im], thresh=0.5)[0], lab)
    assert not np.array_equal(maps[0], maps[1])
    seg.close()


# ---- 5: round trips and wrong-kind calls ----
@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_export_round_trip(hiplib, tmp_path, dtype_name):
    g = golden("mini_unet.npz")
    eng = _engine(hiplib, g, getattr(hiplib, dtype_name.upper()))
    eng.forward(g["images_u8"], want_detections=False)
    m = eng.output_map(3)
    path = str(tmp_path / "mini_unet.yolohip")
    eng.export(path)
    e2 = hiplib.Engine.from_file(path, max_batch=3)
    assert e2.rows == 0 and e2.map_geometry() == (24, 40, 6)
    e2.forward(g["images_u8"], want_detections=False)
    assert np.array_equal(e2.output_map(3), m)
    e2.close(); eng.close()


def test_last_layer_output_is_the_planar_map(hiplib):
    g = golden("mini_unet.npz")
    eng = _engine(hiplib, g, hiplib.FP32)
    eng.forward(g["images_u8"], want_detections=False)
    m = eng.output_map(3)
    assert np.array_equal(eng.last_layer_output(3), m.transpose(0, 3, 1, 2).reshape(3, -1))
    eng.close()


def test_veneer_network_predict_returns_the_planar_map(hiplib, tmp_path, monkeypatch):
    """network_predict of the darknet veneer on mini_unet: the CHW transpose of output_map, and within the fp32 bound of the fixture"""
    from yolo_tensorflow_amd import darknet_hip as DH
    monkeypatch.setenv("DARKNET_HIP_DTYPE", "fp32")
    g = golden("mini_unet.npz")
    cfg = str(tmp_path / "net.cfg"); wf = str(tmp_path / "net.weights")
    open(cfg, "w").write(str(g["cfg"])); IO.write_weights_file(wf, g["weights"], 0, 2)
    x = np.ascontiguousarray((g["images_u8"][0].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    net = DH.load_net(cfg, wf)
    try:
        out = np.ctypeslib.as_array(DH._load().network_predict(net, x.ctypes.data_as(C.POINTER(C.c_float))), shape=(6, 24, 40)).copy()
    finally:
        DH.free_net(net)
    eng = _engine(hiplib, g, hiplib.FP32)
    eng.forward(x.transpose(1, 2, 0)[None].copy(), scale=1.0, want_detections=False)
    m = eng.output_map(1)[0]
    eng.close()
    assert np.array_equal(out, m.transpose(2, 0, 1))
    assert _relmax(out.transpose(1, 2, 0), g["layer_11"][0]) < 5e-4


def test_wrong_kind_calls(hiplib):
    g = golden("mini_unet.npz")
    eng = _engine(hiplib, g, hiplib.BF16)
    x = g["images_u8"]
    with pytest.raises(hiplib.YoloError, match="map network"):
        eng.detect(x)
    with pytest.raises(hiplib.YoloError, match="map network"):
        eng.classify(x)
    eng.forward(x, want_detections=False)
    with pytest.raises(hiplib.YoloError, match="map network"):
        eng.postprocess(3)
    with pytest.raises(hiplib.YoloError, match="map network"):
        eng.detect_images([x[0]])
    assert eng.output_map(3).shape == (3, 24, 40, 6)
    eng.close()
    v3 = golden("mini_v3.npz")
    det = hiplib.Engine(str(v3["cfg"]), max_batch=1, dtype=hiplib.BF16)
    with pytest.raises(hiplib.YoloError, match="map network"):
        det.output_map(1)
    with pytest.raises(hiplib.YoloError, match="map network"):
        det.label_map(1)
    with pytest.raises(hiplib.YoloError, match="map network"):
        det.segment_images([x[0]])
    det.close()
    cls = golden("mini_cls19.npz")
    clf = hiplib.Engine(str(cls["cfg"]), max_batch=1, dtype=hiplib.BF16)
    with pytest.raises(hiplib.YoloError, match="map network"):
        clf.map_geometry()
    clf.close()
