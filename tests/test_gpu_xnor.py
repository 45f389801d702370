"""[convolutional] with xnor=1 on the device: the int8-MFMA kernel (xconv.hip) against the float64 restatement of test_xnor_host.py (where it
is tied to the compiled reference's recorded layers) -- exact sign sums that a transposed or permuted MFMA fragment, a border tap counted
as -1 or a zero counted as +1 would break --, two whole networks against the reference's own C code (tests/golden/mini_xnor.npz,
xnor_layer_cases.npz), and the public surface (export, the cfg without the key, libdarknet_hip.so).

The kernel's tiles (kernels.h): a workgroup computes a block of XCONV_TILE x XCONV_TILE = 8 x 8 output pixels of one image against tiles of
XCONV_CO_TILE = 64 filters; the channels are cut into chunks where a block's int8 window would not fit 128 KiB of LDS; a 4 x 4 block serves
the geometries whose 8 x 8 window has more than 64 x 64 positions."""
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
import test_xnor_host as XH

pytestmark = pytest.mark.gpu

MARGIN_TOL = XH.MARGIN_TOL                   # the fp32 bound of the network tests, as a share of the tensor's largest value


def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _stored(hiplib, x, dtype):
    return _bf16(x) if dtype == hiplib.BF16 else np.asarray(x, np.float32).astype(np.float16).astype(np.float32) if dtype == hiplib.FP16 else np.asarray(x, dtype=np.float32)


def _relmax(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / (np.abs(b).max() + 1e-12))


def _dtypes(hiplib):
    return ((hiplib.FP32, "fp32"), (hiplib.BF16, "bf16"), (hiplib.FP16, "fp16"))


# ---- 1-4: op_conv2d_xnor ----
XCONV_CASES = [          # (size, stride, pad, h, w, cin, cout), each at batch 3
    (3, 1, 1, 7, 9, 16, 16),
    (3, 1, 1, 7, 9, 12, 20),           # neither count a multiple of 8 or 16
    (3, 2, 1, 7, 9, 24, 24),
    (3, 2, 0, 8, 8, 20, 12),
    (1, 1, 0, 13, 9, 64, 64),
    (3, 1, 1, 6, 5, 80, 32),           # more than one K step plus a ragged one
    (5, 1, 2, 6, 7, 16, 16),
    (7, 2, 3, 9, 11, 8, 16),
    (3, 1, 1, 9, 13, 72, 72),          # several pixel tiles
    (3, 1, 1, 5, 6, 16, 80),           # more filters than one workgroup's filter tile (64)
    (3, 1, 1, 17, 10, 16, 16),         # more pixels than one pixel tile (8 x 8): three block rows, two block columns
]
# the sizes at which the kernel takes another path (exact tests only)
PATH_CASES = [
    (7, 2, 3, 9, 11, 288, 16),         # two channel chunks: a 21 x 21 window holds at most 272 channels
    (11, 8, 5, 20, 20, 16, 16),        # the 4 x 4 block: an 8 x 8 block's window would have 67 x 67 positions
    (3, 1, 1, 128, 64, 16, 256),       # 384 blocks of pixels: two workgroups per block, each staging its window once for two filter tiles
]
_ID = lambda c: "k%ds%dp%d_%dx%d_%dto%d" % c


def _signed_operands(case, seed):
    """x in {+-0.5, +-1, +-3} (exact in every storage type), w random signs times a per-filter 2^-j: both asymmetric"""
    k, s, p, h, w, cin, cout = case
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([0.5, 1, 3, -0.5, -1, -3], np.float32), size=(3, h, w, cin), p=[0.25, 0.2, 0.15, 0.1, 0.2, 0.1])
    wt = np.where(rng.random((cout, cin, k, k)) < 0.4, 1, -1).astype(np.float32) * (2.0 ** -(np.arange(cout) % 5)).astype(np.float32)[:, None, None, None]
    return x, wt


@pytest.mark.parametrize("case", XCONV_CASES + PATH_CASES, ids=_ID)
def test_op_conv2d_xnor_exact(hiplib, case):
    """The operand-map check: no bias, linear, the fp32 store.  The sign sum is an integer and alpha_f (a power of two, or that times the
    rounded reciprocal product of xnor_alpha) multiplies it in one rounding: the result is BIT-equal to the restatement rounded to fp32, and in
    16-bit storage to that value rounded once more.  Random asymmetric signs in both operands: a transposed or permuted fragment cannot pass."""
    k, s, p, h, w, cin, cout = case
    x, wt = _signed_operands(case, 7)
    want = XH.xnor_ref(x, wt, None, s, p).astype(np.float32)
    assert np.abs(want).max() > 4          # (not a sum that cancels everywhere)
    for dtype, name in _dtypes(hiplib):
        got = hiplib.op_conv2d_xnor(x, wt, None, stride=s, padding=p, activation="linear", dtype=dtype, out_f32=True)
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        if dtype != hiplib.FP32:
            got = hiplib.op_conv2d_xnor(x, wt, None, stride=s, padding=p, activation="linear", dtype=dtype)
            assert np.array_equal(got, _stored(hiplib, want, dtype)), name


@pytest.mark.parametrize("case", XCONV_CASES + PATH_CASES[:2], ids=_ID)
def test_border_taps_count_as_zero(hiplib, case):
    """x = -1 everywhere, w = +1 everywhere: exactly -cin * (taps inside the image) -- alpha_f is 1 at every K of XCONV_CASES, asserted --; a
    kernel that pads with -1 gives -cin * k^2 at the border"""
    k, s, p, h, w, cin, cout = case
    x = -np.ones((3, h, w, cin), np.float32); wt = np.ones((cout, cin, k, k), np.float32)
    alpha = XH.xnor_alpha(wt)
    if case in XCONV_CASES:
        assert (alpha == 1).all()
    taps = XH.taps_inside(h, w, k, s, p)
    want = np.broadcast_to((-(taps * cin)[None, :, :, None] * alpha.astype(np.float64)).astype(np.float32), (3,) + taps.shape + (cout,))
    if p > 0:
        assert taps.min() < k * k
    for dtype, name in _dtypes(hiplib):
        got = hiplib.op_conv2d_xnor(x, wt, None, stride=s, padding=p, activation="linear", dtype=dtype, out_f32=True)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("k", [1, 3])
def test_zero_is_not_positive(hiplib, k):
    """+0.0, -0.0, the storage type's smallest positive subnormal and its negative, +- its smallest normal, against all-ones filters: exact,
    with both zeros counted as -1 and the subnormals by their sign"""
    cin, cout, h, w = 12, 16, 4, 6
    for dtype, name, sub, nrm in ((hiplib.FP32, "fp32", 2.0 ** -149, 2.0 ** -126), (hiplib.BF16, "bf16", 2.0 ** -133, 2.0 ** -126), (hiplib.FP16, "fp16", 2.0 ** -24, 2.0 ** -14)):
        vals = np.array([0.0, -0.0, sub, -sub, nrm, -nrm], np.float32)
        assert (vals[2:] != 0).all() and np.signbit(vals[1]) and not np.signbit(vals[0])
        idx = (np.arange(h)[:, None, None] * 5 + np.arange(w)[None, :, None] + np.arange(cin)[None, None, :] * 7) % 6
        x = np.broadcast_to(vals[idx], (3, h, w, cin)).copy()
        assert np.array_equal(_stored(hiplib, x, dtype).view(np.uint32), x.view(np.uint32))          # every value is one of the storage type's own
        wt = np.ones((cout, cin, k, k), np.float32)
        assert (XH.xnor_alpha(wt) == 1).all()
        signs = np.where(np.isin(idx, (2, 4)), 1.0, -1.0)
        want = XH.sign_sums(np.broadcast_to(signs, (3, h, w, cin)), wt, 1, k // 2).astype(np.float32)
        assert np.array_equal(want, XH.xnor_ref(x, wt, None, 1, k // 2).astype(np.float32))
        got = hiplib.op_conv2d_xnor(x, wt, None, stride=1, padding=k // 2, activation="linear", dtype=dtype, out_f32=True)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])


@pytest.fixture(scope="module")
def xconv_data():
    """operands per case, drawn once"""
    rng = np.random.default_rng(73)
    data = {}
    for case in XCONV_CASES:
        k, s, p, h, w, cin, cout = case
        data[case] = (rng.standard_normal((3, h, w, cin)).astype(np.float32), (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32),
                      rng.standard_normal(cout).astype(np.float32))
    return data


@pytest.mark.parametrize("case", XCONV_CASES, ids=_ID)
def test_op_conv2d_xnor(hiplib, xconv_data, case):
    """Gaussian operands, a bias, leaky and tanh (a post-activation), batch 3, against the restatement on the input pre-rounded to the storage
    type (the filters enter as fp32: only their signs and alpha_f are used), with the bounds of test_gpu_grouped.py::test_op_conv2d_grouped:
    fp32 1e-4 of the tensor's largest value; bf16 2^-7 |want| + 2e-3; fp16 2^-10 |want| + 2e-3; the fp32 store of the 16-bit configurations
    under the 16-bit bound too."""
    k, s, p, h, w, cin, cout = case
    x, wt, b = xconv_data[case]
    for dtype, name in _dtypes(hiplib):
        for act in ("leaky", "tanh"):
            want = XH.xnor_ref(_stored(hiplib, x, dtype), wt, b, s, p, act)
            for out_f32 in ((False,) if dtype == hiplib.FP32 else (False, True)):
                got = hiplib.op_conv2d_xnor(x, wt, b, stride=s, padding=p, activation=act, dtype=dtype, out_f32=out_f32)
                assert got.shape == want.shape and got.dtype == np.float32
                err = np.abs(got.astype(np.float64) - want)
                if dtype == hiplib.FP32:
                    r = float(err.max() / np.abs(want).max())
                    print("xconv %s fp32 %s: relmax %.3e" % (_ID(case), act, r))
                    assert r < 1e-4
                else:
                    bound = 2.0 ** (-7 if dtype == hiplib.BF16 else -10) * np.abs(want) + 2e-3
                    print("xconv %s %s %s out_f32 %d: max err / bound %.3f" % (_ID(case), name, act, out_f32, float((err / bound).max())))
                    assert (err <= bound).all(), "%s: %g over at %r" % (name, float((err - bound).max()), np.unravel_index(np.argmax(err - bound), err.shape))


# ---- 5, 6: whole networks against the compiled reference ----
def _engine(hiplib, g, dtype, keep=False, batch=1, cfg=None):
    eng = hiplib.Engine(cfg if cfg is not None else str(g["cfg"]), max_batch=batch, dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
    assert eng.weights_count() == g["weights"].size
    eng.set_weights(g["weights"])
    return eng


def test_mini_xnor_matches_compiled_reference_fp32(hiplib):
    """the detector: every layer of the reference's own C forward pass within MARGIN_TOL of that layer's largest value on the fp32 device
    path, and the decoded candidates against get_network_boxes of the compiled reference as test_gpu_grouped.py compares mini_dw_v3.npz"""
    g = golden("mini_xnor.npz")
    secs = IO.parse_cfg(str(g["cfg"]))[1:]
    eng = _engine(hiplib, g, hiplib.FP32, keep=True)
    eng.forward(g["image_u8"][None], scale=1.0 / 255.0)
    for i, s in enumerate(secs):
        if s["type"] == "yolo":
            continue
        got = eng.layer_output(i, 1); ref = g["layer_%02d" % i]
        assert got.shape == ref.shape
        r = _relmax(got, ref)
        print("mini_xnor layer %d (%s xnor=%s): relmax %.3e" % (i, s["type"], s.get("xnor", "-"), r))
        assert r < MARGIN_TOL, "layer %d (%s)" % (i, s["type"])
    eng.close()
    eng = _engine(hiplib, g, hiplib.FP32)
    det = eng.forward(g["image_u8"][None])[0]
    keep = det[:, 4] > float(g["thresh"])
    assert keep.sum() == len(g["boxes_raw"])
    np.testing.assert_allclose(det[keep, :4], g["boxes_raw"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(det[keep, 4], g["obj_raw"], rtol=2e-3, atol=2e-4)
    eng.close()


def test_xnor_layer_cases_match_compiled_reference_fp32(hiplib):
    """the classifier of differently shaped xnor layers, likewise; the plan that keeps every layer and the production plan give the same probabilities"""
    g = golden("xnor_layer_cases.npz")
    secs = IO.parse_cfg(str(g["cfg"]))[1:]
    probs = []
    for keep in (True, False):
        eng = _engine(hiplib, g, hiplib.FP32, keep)
        probs.append(eng.classify(g["image_u8"][None], top_k=0))
        if keep:
            for i, s in enumerate(secs):
                got = eng.layer_output(i, 1); ref = g["layer_%02d" % i]
                assert got.size == ref.size
                r = _relmax(got.reshape(ref.shape), ref)
                print("xnor_layer_cases layer %d (%s xnor=%s %s): relmax %.3e" % (i, s["type"], s.get("xnor", "-"), s.get("activation", ""), r))
                assert r < MARGIN_TOL, "layer %d (%s)" % (i, s["type"])
        eng.close()
    assert np.array_equal(probs[0], probs[1])
    assert _relmax(probs[0].reshape(-1), g["layer_%02d" % (len(secs) - 1)]) < MARGIN_TOL


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", XH.FIXTURES)
def test_xnor_layers_16bit(hiplib, name, dtype_name):
    """bf16 / fp16 storage, layer by layer on identical inputs: for each xnor layer i the device's layer_output(i - 1) as stored, layer i
    restated from it in float64, the device's layer_output(i) within the 16-bit bounds of test_op_conv2d_xnor.  End to end is NOT compared
    in 16 bits: a rounding upstream may flip the sign of a value near zero, and with it whole sums downstream."""
    dtype = getattr(hiplib, dtype_name.upper())
    g = golden(name)
    secs = IO.parse_cfg(str(g["cfg"]))
    params = XH.layer_params(secs, g["weights"])
    eng = _engine(hiplib, g, dtype, keep=True)
    eng.forward(g["image_u8"][None], want_detections=False)
    layers = XH.xnor_layers(secs)
    assert len(layers) >= 3
    for i in layers:
        x = eng.layer_output(i - 1, 1); got = eng.layer_output(i, 1)
        assert np.array_equal(_stored(hiplib, x, dtype), x)
        want = XH.restate_layer(secs, params, i, x)
        assert got.shape == want.shape
        err = np.abs(got.astype(np.float64) - want)
        bound = 2.0 ** (-7 if dtype == hiplib.BF16 else -10) * np.abs(want) + 2e-3
        print("%s %s layer %d: max err / bound %.3f" % (name, dtype_name, i, float((err / bound).max())))
        assert (err <= bound).all(), "layer %d: %g over" % (i, float((err - bound).max()))
    eng.close()


# ---- 7: surface ----
def _outputs(eng, g, name):
    if name == "mini_xnor.npz":
        return eng.forward(g["image_u8"][None])
    return eng.classify(g["image_u8"][None], top_k=0)


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
@pytest.mark.parametrize("name", XH.FIXTURES)
def test_export_round_trip(hiplib, tmp_path, name, dtype_name):
    g = golden(name)
    eng = _engine(hiplib, g, getattr(hiplib, dtype_name.upper()))
    out = _outputs(eng, g, name)
    path = str(tmp_path / "xnor.yolohip")
    eng.export(path)
    e2 = hiplib.Engine.from_file(path, max_batch=1)
    assert np.array_equal(_outputs(e2, g, name), out)
    e2.close(); eng.close()


@pytest.mark.parametrize("name", XH.FIXTURES)
def test_the_key_is_not_ignored(hiplib, name):
    """the same cfg and weights without xnor=1 give different outputs"""
    g = golden(name)
    eng = _engine(hiplib, g, hiplib.FP32)
    with_key = _outputs(eng, g, name)
    eng.close()
    eng = _engine(hiplib, g, hiplib.FP32, cfg=str(g["cfg"]).replace("xnor=1\n", ""))
    without = _outputs(eng, g, name)
    eng.close()
    assert with_key.shape == without.shape
    assert np.abs(with_key - without).max() > 1e-2 * np.abs(with_key).max()


def test_loads_through_the_darknet_veneer(hiplib, tmp_path):
    """the detector cfg and a .weights file through libdarknet_hip.so's load_network (yolo_tensorflow_amd.darknet_hip): it detects"""
    from yolo_tensorflow_amd import darknet_hip as DK
    g = golden("mini_xnor.npz")
    cfg = str(tmp_path / "x.cfg"); wf = str(tmp_path / "x.weights")
    open(cfg, "w").write(str(g["cfg"])); IO.write_weights_file(wf, g["weights"], 0, 2)
    net = DK.load_net(cfg, wf, 0)
    assert net
    got = DK.detect(net, ["a", "b", "c"], g["image_u8"], thresh=0.5, nms=0.45)
    DK.free_net(net)
    assert len(got) >= 1 and all(name in ("a", "b", "c") and 0.5 < prob <= 1 for name, prob, _ in got)
