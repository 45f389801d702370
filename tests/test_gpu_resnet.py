"""ResNet / VGG classifiers on the device: darknet's thirteen activations (k_activate), the general [shortcut] (k_shortcut: a `from`
tensor with other channels or another size, any activation), whole networks against the reference's own C code
(tests/golden/mini_resnet.npz / mini_resnet_30.npz), the fused plan against the layer-by-layer one, split-fp16 pairs and the public
surface (Classifier("resnet50"), export, the darknet veneer)."""
import ctypes as C
import os
import re
import numpy as np
import pytest
from conftest import golden
from oracle import darknet_ref as DR
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_DIR = os.path.join(ROOT, "tests", "golden", "images")
JPGS = ["dog.jpg", "eagle.jpg", "giraffe.jpg", "horses.jpg", "kite.jpg", "person.jpg"]
U = 2.0 ** -24          # unit roundoff of fp32
ACTS = ("linear", "leaky", "relu", "relie", "logistic", "loggy", "elu", "ramp", "tanh", "plse", "stair", "hardtan", "lhtan")
EXP_ACTS = ("logistic", "loggy", "elu", "tanh")          # the activations of DN/activations.h that call exp
# what the reference's C code stands off from the float64 formulas below by, in u max(1, |y|), over act_inputs(): measured 0.500 for each
# of logistic, loggy, elu and tanh (it evaluates in double and rounds once); test_resnet_host.py measures it again where oracle/_ref is built
K_REF = 0.5


def act64(name, x):
    """DN/activations.h restated in float64 on float32 inputs"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    if name == "linear": return x
    if name == "leaky": return np.where(x > 0, x, .1 * x)
    if name == "relu": return x * (x > 0)
    if name == "relie": return np.where(x > 0, x, .01 * x)
    if name == "logistic": return 1. / (1. + np.exp(-x))
    if name == "loggy": return 2. / (1. + np.exp(-x)) - 1
    if name == "elu": return (x >= 0) * x + (x < 0) * (np.exp(x) - 1)
    if name == "ramp": return x * (x > 0) + .1 * x
    if name == "tanh": return (np.exp(2 * x) - 1) / (np.exp(2 * x) + 1)
    if name == "plse": return np.where(x < -4, .01 * (x + 4), np.where(x > 4, .01 * (x - 4) + 1, .125 * x + .5))
    if name == "stair":
        n = np.floor(x)
        return np.where(n % 2 == 0, np.floor(x / 2.), (x - n) + np.floor(x / 2.))
    if name == "hardtan": return np.clip(x, -1, 1)
    if name == "lhtan": return np.where(x < 0, .001 * x, np.where(x > 1, .001 * (x - 1) + 1, x))
    raise ValueError(name)


def act_inputs():
    """4096 values in [-12, 12], the breakpoints +-4, +-1, 0, and the integers and half-integers (stair)"""
    rng = np.random.default_rng(5)
    return np.concatenate([rng.uniform(-12, 12, 4096), [-4, 4, -1, 1, 0], np.arange(-12, 12.5, 0.5)]).astype(np.float32)


def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _stored(hiplib, x, dtype):
    return _bf16(x) if dtype == hiplib.BF16 else x.astype(np.float16).astype(np.float32) if dtype == hiplib.FP16 else np.asarray(x, dtype=np.float32)


def _half_ulp(v, mant_bits, min_exp):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** min_exp)))
    return 0.5 * 2.0 ** (e - mant_bits)


def _storage_half_ulp(hiplib, y, dtype):
    return _half_ulp(y, 7, -126) if dtype == hiplib.BF16 else _half_ulp(y, 10, -14) if dtype == hiplib.FP16 else 0.0


def _relmax(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _prob_bound(p_ref, tol, max_logit):
    d = tol * float(max_logit)
    return p_ref.astype(np.float64) * np.expm1(2 * d) + 1e-7


# ---- 2: op_activate ----
@pytest.mark.parametrize("name", ACTS)
def test_op_activate(hiplib, name):
    """fp32 against the float64 restatement of DN/activations.h.  Piecewise-linear activations: 4 u max(1, |y|).  The exp-based ones:
    k u max(1, |y|) with k = max(8 K_REF, 8) = 8, K_REF = 0.5 being what the reference's own C code stands off from float64 by on these
    inputs (measured: 0.500 for logistic, loggy, elu and tanh alike -- it evaluates in double and rounds once, and so does k_activate).
    bf16 / fp16: the same reference on the stored inputs, plus half a unit in the last place of the storage type.  The tensor is
    [1, 5, 83, 10]: ten channels, so the second 8-channel (third 4-channel) granule of every pixel is masked."""
    x = act_inputs().reshape(1, 5, 83, 10)
    k = max(8 * K_REF, 8.0) if name in EXP_ACTS else 4.0
    for dtype in (hiplib.FP32, hiplib.BF16, hiplib.FP16):
        xs = _stored(hiplib, x, dtype)
        y = act64(name, xs)
        bound = k * U * np.maximum(1, np.abs(y)) + _storage_half_ulp(hiplib, y, dtype)
        got = hiplib.op_activate(x, name, dtype=dtype)
        assert got.shape == x.shape and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - y)
        print("activate %s dtype %d: max err / bound %.3f (max err %.3g u max(1, |y|))" % (name, dtype, float((err / bound).max()), float((err / (U * np.maximum(1, np.abs(y)))).max())))
        assert (err <= bound).all(), "%s dtype %d: %g over the bound at x = %r" % (name, dtype, float((err - bound).max()), float(xs.reshape(-1)[np.argmax(err - bound)]))


def test_op_activate_signed_zero_and_infinities(hiplib):
    """relu as max(v, 0 * v): -0 for negative inputs like the reference's x * (x > 0), +-0 and +inf pass; -inf stays -inf (the reference: NaN)"""
    x = np.array([-3.0, -0.0, 0.0, 2.0, np.inf, -np.inf, 1.0, 1.0], np.float32).reshape(1, 1, 1, 8)
    got = hiplib.op_activate(x, "relu").reshape(-1)
    assert np.array_equal(got[:5].view(np.uint32), np.array([-0.0, -0.0, 0.0, 2.0, np.inf], np.float32).view(np.uint32))
    assert got[5] == -np.inf


# ---- 3: op_shortcut ----
def shortcut_ref(x, f, dtype=np.float64):
    """DN/blas.c:68-92 shortcut_cpu, literally: (w1, h1, c1) the `from` tensor, (w2, h2, c2) the output"""
    out = np.array(x, dtype=dtype)
    f = np.asarray(f, dtype=dtype)
    h2, w2, c2 = x.shape[1:]; h1, w1, c1 = f.shape[1:]
    stride, sample = w1 // w2, w2 // w1
    assert stride == h1 // h2 and sample == h2 // h1
    stride, sample = max(stride, 1), max(sample, 1)
    minw, minh, minc = min(w1, w2), min(h1, h2), min(c1, c2)
    for j in range(minh):
        for i in range(minw):
            out[:, j * sample, i * sample, :minc] = out[:, j * sample, i * sample, :minc] + f[:, j * stride, i * stride, :minc]
    return out


SHORTCUT_CASES = {          # name: ((h2, w2, c2), (h1, w1, c1))
    "matched": ((8, 8, 16), (8, 8, 16)),
    "from_narrower": ((8, 8, 40), (8, 8, 12)),
    "from_wider": ((8, 8, 12), (8, 8, 40)),
    "strided": ((8, 8, 32), (16, 16, 16)),
    "int_division_15_into_8": ((8, 8, 16), (15, 15, 16)),
    "sample_2": ((8, 8, 16), (4, 4, 16)),
    "blocks_and_odd": ((19, 19, 72), (38, 38, 21)),          # more than one block, minc 21
}


@pytest.fixture(scope="module")
def shortcut_data():
    rng = np.random.default_rng(17)
    data = {}
    for name, (a, b) in SHORTCUT_CASES.items():
        x = (rng.standard_normal((3,) + a) * 3).astype(np.float32); f = (rng.standard_normal((3,) + b) * 3).astype(np.float32)
        x[0, 1, 1, -1] = -0.0          # where nothing is added (a channel beyond minc, a position between samples) a -0 must survive: no add of +0
        data[name] = (x, f)
    return data


@pytest.mark.parametrize("case", list(SHORTCUT_CASES))
def test_op_shortcut_fp32(hiplib, shortcut_data, case):
    """linear: one add of two floats, so the float32 restatement is met bit for bit (batch 3).  leaky, relu: 4 u |y| against the
    float64 restatement -- the add is rounded once (u |s|), and the device's slope product is a float one where the reference's .1 * x
    is a double one (0.1f is 1.5e-8 off .1, the product rounds once more)."""
    x, f = shortcut_data[case]
    want = shortcut_ref(x, f, np.float32)
    got = hiplib.op_shortcut(x, f, "linear")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for act in ("leaky", "relu"):
        y = act64(act, want)          # (the float32 sum is what the reference activates too)
        got = hiplib.op_shortcut(x, f, act)
        err = np.abs(got.astype(np.float64) - y)
        print("shortcut %s %s: max err %.3g u |y|" % (case, act, float((err / (U * np.abs(y) + 1e-300)).max())))
        assert (err <= 4 * U * np.abs(y)).all()


@pytest.mark.parametrize("case", list(SHORTCUT_CASES))
def test_op_shortcut_16bit(hiplib, shortcut_data, case):
    """bf16 / fp16: the float64 result of the stored operands, to half a unit in the last place of the storage type -- plus the fp32
    arithmetic in front of that one rounding: u |y| for the add, 4 u |y| with leaky or relu (as in fp32 above)."""
    x, f = shortcut_data[case]
    for dtype in (hiplib.BF16, hiplib.FP16):
        s = shortcut_ref(_stored(hiplib, x, dtype), _stored(hiplib, f, dtype))
        for act, slope, k in (("linear", 1., 1), ("leaky", .1, 4), ("relu", 0., 4)):
            y = np.where(s > 0, s, slope * s)
            got = hiplib.op_shortcut(x, f, act, dtype=dtype)
            err = np.abs(got.astype(np.float64) - y)
            bound = _storage_half_ulp(hiplib, y, dtype) + k * U * np.abs(y)
            assert (err <= bound).all(), "%s %s dtype %d: %g over" % (case, act, dtype, float((err - bound).max()))


def test_op_shortcut_pairs(hiplib):
    """split-fp16 pairs (channel counts multiples of 32) keep 22 significant bits: 2^-22 of each operand on the way in (the activations
    used here do not amplify it), the fp32 arithmetic (4 u max(1, |y|)), 2^-22 |y| on the way out, and the fp16 subnormal floor of a lo half"""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((3, 8, 8, 64)) * 3).astype(np.float32); f = (rng.standard_normal((3, 16, 16, 32)) * 3).astype(np.float32)
    mag = shortcut_ref(np.abs(x), np.abs(f))
    for act in ("linear", "leaky", "tanh"):
        y = act64(act, shortcut_ref(x, f).astype(np.float32))
        got = hiplib.op_shortcut(x, f, act, dtype=hiplib.FP16X2)
        err = np.abs(got.astype(np.float64) - y)
        bound = 2.0 ** -22 * mag + 4 * U * np.maximum(1, np.abs(y)) + 2.0 ** -22 * np.abs(y) + 2.0 ** -24
        print("shortcut pairs %s: max err / bound %.3f" % (act, float((err / bound).max())))
        assert (err <= bound).all(), "%s: %g over" % (act, float((err - bound).max()))
    with pytest.raises(hiplib.YoloError, match="multiples of 32"):
        hiplib.op_shortcut(x[..., :40], f, dtype=hiplib.FP16X2)


def test_shortcut_operands_as_channel_windows(hiplib):
    """yolo_op_shortcut takes dense tensors, so windows are covered through a network: the [shortcut] (relu, `from` narrower) writes
    into a channel window of the concat buffer behind it, and its `from` operand is another window of that buffer"""
    c = lambda f, k, act: "[convolutional]\nfilters=%d\nsize=%d\nstride=1\npad=1\nactivation=%s\n\n" % (f, k, act)
    cfg = ("[net]\nwidth=20\nheight=20\nchannels=3\n\n" + c(16, 3, "leaky") + c(24, 3, "linear") + "[shortcut]\nfrom=-2\nactivation=relu\n\n[route]\nlayers=-1,-3\n\n" +
           c(24, 1, "linear") + "[avgpool]\n\n[softmax]\n")
    flat = IO.synth_weights(IO.parse_cfg(cfg), seed=4)
    img = np.random.default_rng(2).integers(0, 256, (3, 20, 20, 3), dtype=np.uint8)
    probs = []
    for keep in (True, False):
        eng = hiplib.Engine(cfg, max_batch=3, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
        eng.set_weights(flat)
        probs.append(eng.classify(img, top_k=0))
        if keep:
            a, b, s, r = (eng.layer_output(i, 3) for i in range(4))
            want = shortcut_ref(b, a, np.float32); want = want * (want > 0)
            assert np.array_equal(s, want) and np.array_equal(r, np.concatenate([s, a], axis=-1))
        eng.close()
    assert np.array_equal(probs[0], probs[1])


# ---- 4: mini networks against the compiled reference ----
@pytest.mark.parametrize("name", ["mini_resnet.npz", "mini_resnet_30.npz"])
def test_mini_resnet_matches_compiled_reference_fp32(hiplib, name):
    """Every layer of the reference's own C forward pass, fp32 device path, batch 3: 5e-4 of each tensor's scale (the bound of
    test_mini_network_matches_compiled_reference_fp32: darknet's batch-norm uses sqrt(var) + 1e-6 where the folded filters use
    sqrt(var + 1e-5), and the summation order differs); the probabilities within _prob_bound(want, 2e-4, max |logit|)."""
    g = golden(name)
    cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    for keep in (True, False):
        eng = hiplib.Engine(cfg, max_batch=3, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
        eng.set_weights(g["weights"])
        p = eng.classify(g["images_u8"], top_k=0)
        want = g["layer_%02d" % (len(secs) - 1)]
        err = np.abs(p.astype(np.float64) - want)
        print("%s keep %d: probabilities max err / bound %.3f" % (name, keep, float((err / _prob_bound(want, 2e-4, g["max_abs_logit"])).max())))
        assert (err <= _prob_bound(want, 2e-4, g["max_abs_logit"])).all()
        if keep:
            for i, s in enumerate(secs[:-1]):
                got = eng.layer_output(i, 3); ref = g["layer_%02d" % i]
                assert got.reshape(3, -1).shape == ref.reshape(3, -1).shape
                r = _relmax(got.reshape(3, -1), ref.reshape(3, -1))
                print("%s layer %d (%s %s): relmax %.3e" % (name, i, s["type"], s.get("activation", ""), r))
                assert r < 5e-4, "layer %d (%s)" % (i, s["type"])
        eng.close()


# ---- 5: fused plan == layer-by-layer plan ----
def _probs_both_plans(hiplib, cfg, flat, img, dtype):
    out = []
    for keep in (False, True):
        eng = hiplib.Engine(cfg, max_batch=img.shape[0], dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
        eng.set_weights(flat)
        out.append(eng.classify(img, top_k=0))
        eng.close()
    return out


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_mini_resnet_fused_plan_equals_layer_by_layer_plan(hiplib, dtype_name):
    dtype = getattr(hiplib, dtype_name.upper())
    for name in ("mini_resnet.npz", "mini_resnet_30.npz"):
        g = golden(name)
        a, b = _probs_both_plans(hiplib, str(g["cfg"]), g["weights"], g["images_u8"], dtype)
        assert np.array_equal(a, b) and np.abs(a.astype(np.float64).sum(axis=1) - 1).max() <= 1e-5
        want = g["layer_20"]
        assert (np.abs(a.astype(np.float64) - want) <= _prob_bound(want, 3e-2 if dtype == hiplib.BF16 else 4e-3, g["max_abs_logit"])).all()


def block_cfg(size, inner_act="leaky", shortcut_act="linear"):
    """darknet-53's first stages in small: the fused stem (3 -> 32 -> 64 / 2, 1 x 1 to 32), conv3 + shortcut + the 64 -> 128 stride-2
    conv, and the 128 -> 64 -> 128 residual block -- every fused launch the planner knows; then a class conv, [avgpool], [softmax]"""
    c = lambda f, k, st=1, act="leaky", bn=True: "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", f, k, st, act)
    return ("[net]\nwidth=%d\nheight=%d\nchannels=3\n\n" % (size, size) + c(32, 3) + c(64, 3, 2) + c(32, 1) + c(64, 3) + "[shortcut]\nfrom=-3\nactivation=linear\n\n" +
            c(128, 3, 2) + c(64, 1, act=inner_act) + c(128, 3) + "[shortcut]\nfrom=-3\nactivation=%s\n\n" % shortcut_act + c(24, 1, act="linear", bn=False) + "[avgpool]\n\n[softmax]\n")


def _plan(hiplib, cfg, dtype, keep=False):
    rc, text = hiplib.plan_table(cfg, dtype, 3, keep)
    assert rc == 0, text
    return [dict(kv.split("=") for kv in line.split()[2:]) for line in text.splitlines()[:-1]]


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("size", [64, 52])
def test_block_network_fused_plan_equals_layer_by_layer_plan(hiplib, dtype_name, size):
    """64 x 64 (the stem and the conv3 + stride-2 launch are eligible) and 52 x 52 (13 x 13 at the 128-channel stage: the residual block
    too).  A `logistic` conv inside the block: the planner must decline that fusion -- and every other use of the layer --; a leaky
    [shortcut] on the block is not folded, so the block launch does not apply either.  Probabilities equal bit for bit throughout."""
    dtype = getattr(hiplib, dtype_name.upper())
    img = np.random.default_rng(size).integers(0, 256, (3, size, size, 3), dtype=np.uint8)
    base = _plan(hiplib, block_cfg(size), dtype)
    assert [base[i]["fused"] for i in (0, 1, 2)] == ["stem"] * 3 and base[3]["fused"] == base[5]["fused"] == "c3s2" and base[3]["residual_from"] == "1"
    assert [base[i]["fused"] for i in (6, 7)] == (["resblock"] * 2 if size == 52 else ["none"] * 2) and base[7]["residual_from"] == "5"
    assert all(l["fused"] == "none" and l["residual_from"] == "-2" and l["tail_layer"] == "-1" for l in _plan(hiplib, block_cfg(size), dtype, keep=True))
    logi = _plan(hiplib, block_cfg(size, inner_act="logistic"), dtype)
    assert logi[6]["fused"] == logi[7]["fused"] == "none" and logi[5]["tail_layer"] == "-1" and logi[6]["tail_layer"] == "-1" and logi[7]["residual_from"] == "5"
    assert logi[3]["fused"] == "c3s2" and logi[0]["fused"] == "stem"
    leaky = _plan(hiplib, block_cfg(size, shortcut_act="leaky"), dtype)
    assert leaky[6]["fused"] == leaky[7]["fused"] == "none" and leaky[7]["residual_from"] == "-2"
    for kw in ({}, {"inner_act": "logistic"}, {"shortcut_act": "leaky"}, {"inner_act": "tanh", "shortcut_act": "elu"}):
        cfg = block_cfg(size, **kw)
        flat = IO.synth_weights(IO.parse_cfg(cfg), seed=9)
        a, b = _probs_both_plans(hiplib, cfg, flat, img, dtype)
        assert np.array_equal(a, b), kw
        assert np.isfinite(a).all() and np.abs(a.astype(np.float64).sum(axis=1) - 1).max() <= 1e-5 and not np.array_equal(a[0], a[1])


# ---- 6: split-fp16 pairs ----
def raised(cfg, mul=2):
    return re.sub(r"filters=(\d+)", lambda m: "filters=%d" % (int(m.group(1)) * (1 if m.group(1) == "24" else mul)), cfg)


def _scaled_weights(hiplib, cfg, img, logit_layer, seed):
    """synthetic weights with the class conv scaled until the fp32 logits reach +-5 (as tools/make_golden.py does) -> (flat, fp32 probs, max |logit|)"""
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=seed)
    last = IO.conv_specs(secs)[-1]
    tail = last["filters"] * (1 + last["cin"] * last["size"] ** 2)
    for _ in range(2):
        eng = hiplib.Engine(cfg, max_batch=img.shape[0], dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET, keep_layers=True)
        eng.set_weights(flat)
        p = eng.classify(img, top_k=0)
        m = float(np.abs(eng.layer_output(logit_layer, img.shape[0])).max())
        eng.close()
        if 4.0 <= m <= 6.0:
            break
        flat[-tail:] *= np.float32(5.0 / m)
    return flat, p, m


@pytest.mark.parametrize("name", ["mini_resnet.npz", "mini_resnet_30.npz"])
def test_mini_resnet_split_fp16(hiplib, name):
    """channel counts raised to multiples of 32: the probabilities of the pairs network within the pairs tests' bound (2e-4 of the
    largest logit, as test_gpu_classifier.py's _dtypes) of the fp32 network's, in both plans; the unraised network is refused"""
    g = golden(name)
    cfg = raised(str(g["cfg"]))
    flat, p32, m = _scaled_weights(hiplib, cfg, g["images_u8"], int(g["logit_layer"]), seed=41)
    for keep in (False, True):
        eng = hiplib.Engine(cfg, max_batch=3, dtype=hiplib.FP16X2, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
        eng.set_weights(flat)
        p = eng.classify(g["images_u8"], top_k=0)
        eng.close()
        err = np.abs(p.astype(np.float64) - p32)
        print("%s fp16x2 keep %d: max err / bound %.3f (max |logit| %.2f)" % (name, keep, float((err / _prob_bound(p32, 2e-4, m)).max()), m))
        assert (err <= _prob_bound(p32, 2e-4, m)).all()
    with pytest.raises(hiplib.YoloError, match="multiples of 32"):
        hiplib.Engine(str(g["cfg"]), dtype=hiplib.FP16X2)


# ---- 7: surface ----
def test_resnet50_classifier(hiplib):
    from PIL import Image
    from yolo_tensorflow_amd.classifier import Classifier
    imgs = [np.ascontiguousarray(np.asarray(Image.open(os.path.join(IMG_DIR, n)).convert("RGB"))) for n in JPGS]
    clf = Classifier("resnet50", dtype=hiplib.BF16, max_batch=8)
    assert clf.num_classes == 1000 and clf.engine.size == 256
    recs = clf.classify_from_images(imgs, top=5)
    assert len(recs) == 6 and all(len(r) == 5 for r in recs)
    full = clf.engine.classify_images(imgs, fit=hiplib.FIT_STRETCH, top_k=0)
    assert full.shape == (6, 1000) and np.abs(full.astype(np.float64).sum(axis=1) - 1).max() <= 1e-5
    for b, r in enumerate(recs):
        probs = [q for _, q in r]
        assert all(0.0 < q <= 1.0 for q in probs) and probs == sorted(probs, reverse=True)
        want = np.argsort(-full[b], kind="stable")[:5]
        assert [k for k, _ in r] == [int(k) for k in want]
        assert probs == [float(q) for q in full[b][want]]
    assert not np.array_equal(full[0], full[1])
    clf.close()


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_export_round_trip(hiplib, tmp_path, dtype_name):
    g = golden("mini_resnet.npz")
    eng = hiplib.Engine(str(g["cfg"]), max_batch=3, dtype=getattr(hiplib, dtype_name.upper()), semantics=hiplib.SEM_DARKNET)
    eng.set_weights(g["weights"])
    p = eng.classify(g["images_u8"], top_k=0)
    path = str(tmp_path / "mini_resnet.yolohip")
    eng.export(path)
    e2 = hiplib.Engine.from_file(path, max_batch=3)
    assert e2.rows == 0 and e2.num_classes == 24
    assert np.array_equal(e2.classify(g["images_u8"], top_k=0), p)
    e2.close(); eng.close()


class IMAGE(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]


def test_veneer_predict_matches_libdarknet(hiplib, tmp_path):
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")
    from yolo_tensorflow_amd import darknet_hip as DH
    os.environ["DARKNET_HIP_DTYPE"] = "fp32"
    g = golden("mini_resnet.npz")
    cfg = str(tmp_path / "net.cfg"); wf = str(tmp_path / "net.weights")
    open(cfg, "w").write(str(g["cfg"])); IO.write_weights_file(wf, g["weights"], 0, 2)
    ref = DR.lib()
    ref.network_predict_image.argtypes = [C.c_void_p, IMAGE]; ref.network_predict_image.restype = C.POINTER(C.c_float)
    with DR._Quiet():
        rnet = ref.load_network(cfg.encode(), wf.encode(), 0)
        ref.set_batch_network(rnet, 1)
    net = DH.load_net(cfg, wf)
    logit_layer = int(g["logit_layer"])
    try:
        for w, h in ((90, 60), (40, 75)):
            img = np.ascontiguousarray(np.random.default_rng(w * 7 + h).random((3, h, w), dtype=np.float32))
            want = np.ctypeslib.as_array(ref.network_predict_image(rnet, IMAGE(w, h, 3, img.ctypes.data_as(C.POINTER(C.c_float)))), shape=(24,)).copy()
            n_logits = ref.ref_layer_outputs(rnet, logit_layer)
            max_logit = float(np.abs(np.ctypeslib.as_array(ref.ref_layer_output(rnet, logit_layer), shape=(n_logits,))).max())
            im = DH.IMAGE(w, h, 3, img.ctypes.data_as(C.POINTER(C.c_float)))
            got = np.ctypeslib.as_array(DH.predict_image(net, im), shape=(24,)).copy()
            err = np.abs(got.astype(np.float64) - want)
            print("veneer %dx%d: max err / bound %.3f" % (w, h, float((err / _prob_bound(want, 2e-4, max_logit)).max())))
            assert (err <= _prob_bound(want, 2e-4, max_logit)).all()
    finally:
        DH.free_net(net)
        ref.free_network(rnet)


def test_resnet18_split_fp16_small(hiplib):
    """ResNet-18 at 64 x 64 as split-fp16 pairs (the 7 x 7 / 2 stem reads the image as plain fp16) against the fp32 network"""
    cfg = IO.with_input_size(IO.cfg_text("resnet18"), 64).replace("filters=1000", "filters=24")
    img = np.random.default_rng(8).integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    logit_layer = len(IO.parse_cfg(cfg)) - 4
    flat, p32, m = _scaled_weights(hiplib, cfg, img, logit_layer, seed=43)
    eng = hiplib.Engine(cfg, max_batch=2, dtype=hiplib.FP16X2, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(flat)
    p = eng.classify(img, top_k=0)
    eng.close()
    err = np.abs(p.astype(np.float64) - p32)
    print("resnet18 64 fp16x2: max err / bound %.3f (max |logit| %.2f)" % (float((err / _prob_bound(p32, 2e-4, m)).max()), m))
    assert (err <= _prob_bound(p32, 2e-4, m)).all()
