"""The layers that move data (max-pool, 2x upsample, reorg, the plain shortcut add, the route copy) and the dense conv's geometry keys
(pad=0, padding=, any stride) at the edges the planner accepts: channel counts that are no multiples of 8, odd extents, a concatenation
at channel offset 20.  Against the compiled reference's recorded layers (tests/golden/mini_edges.npz, fp32), and layer by layer
against the numpy restatements applied to the device's OWN stored input of that layer (fp32, bf16, fp16) -- no tolerance for a layer
that only moves values.  tests/test_edges_host.py ties those restatements to the reference at these shapes."""
import numpy as np
import pytest
from conftest import golden
from oracle import yolo_ref as R
from yolo_tensorflow_amd import darknet_io as IO
from test_edges_host import FIXTURE, MOVERS, SLOPES, conv_geometry, layer_inputs, mover_ref, stream_params
from test_gpu_ops import _assert_bf16_close
from test_gpu_fp16 import _assert_f16_close
from test_gpu_resnet import U, _relmax, _storage_half_ulp

pytestmark = pytest.mark.gpu
DTYPES = ("fp32", "bf16", "fp16")


def _dt(hiplib, name):
    return {"fp32": hiplib.FP32, "bf16": hiplib.BF16, "fp16": hiplib.FP16}[name]


def _round(name, x):
    """a fp32 result rounded once to the storage type"""
    return R.to_bf16(x) if name == "bf16" else R.to_f16(x) if name == "fp16" else np.asarray(x, dtype=np.float32)


def _layers(hiplib, cfg, flat, imgs, dtype, semantics, keep=True):
    """(every layer's stored output as fp32, the map) of one forward of the whole batch"""
    eng = hiplib.Engine(cfg, max_batch=imgs.shape[0], dtype=dtype, semantics=semantics, keep_layers=keep)
    eng.set_weights(flat)
    eng.forward(imgs, want_detections=False)
    n = imgs.shape[0]
    outs = [eng.layer_output(i, n) for i in range(eng.num_layers)] if keep else None
    m = eng.output_map(n)
    eng.close()
    return outs, m


@pytest.fixture(scope="module")
def edges(hiplib):
    """mini_edges, keep_layers=True, once per storage type: {name: (layer outputs, map)}"""
    g = golden(FIXTURE)
    return {name: _layers(hiplib, str(g["cfg"]), g["weights"], g["images_u8"], _dt(hiplib, name), hiplib.SEM_DARKNET) for name in DTYPES}


# ---- (a) the whole network against the reference's own C code, fp32 ----
def test_mini_edges_matches_compiled_reference_fp32(hiplib, edges):
    """Every layer of the reference's forward pass, fp32 device path, batch 3: shapes equal and 5e-4 of each tensor's scale (the bound of
    test_mini_resnet_matches_compiled_reference_fp32).  The plan that keeps no layer and reuses pooled buffers gives the same map bit
    for bit.  Observed worst layer: see docs/NOTEBOOK.md."""
    g = golden(FIXTURE); cfg = str(g["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    outs, m = edges["fp32"]
    assert len(outs) == len(secs)
    worst = []
    for i, s in enumerate(secs):
        got, ref = outs[i], g["layer_%02d" % i]
        assert got.shape == ref.shape, "layer %d (%s)" % (i, s["type"])
        worst.append(_relmax(got, ref))
        print("mini_edges layer %d (%s): relmax %.3e" % (i, s["type"], worst[-1]))
    assert m.shape == g["layer_%02d" % (len(secs) - 1)].shape and np.array_equal(m, outs[-1])
    for i, r in enumerate(worst):
        assert r < 5e-4, "layer %d (%s): %.3e" % (i, secs[i]["type"], r)
    _, lean = _layers(hiplib, cfg, g["weights"], g["images_u8"], hiplib.FP32, hiplib.SEM_DARKNET, keep=False)
    assert np.array_equal(lean, m)


# ---- (b) layer-local exactness ----
def _check_conv(hiplib, name, sec, p, x, got, what):
    """a bias-only conv on bf16-exact filters and its stored input: one rounding, the output's.  bf16: the rule of _assert_bf16_close;
    fp16: the one tests/test_gpu_fp16.py applies to conv outputs; fp32: that of test_conv_fp32_exact_path"""
    k, st, pad = conv_geometry(sec)
    y = R.conv2d_nhwc(x, p["w"], st, pad) + p["bias"]
    ref = np.where(y > 0, y, np.float32(SLOPES[sec["activation"]]) * y).astype(np.float32)
    assert got.shape == ref.shape, what
    err = float(np.abs(got - _round(name, ref)).max())
    print("%s %s (%d/%d/%d): max err %.3e of scale %.3f" % (what, name, k, st, pad, err, float(np.abs(ref).max())))
    assert np.isfinite(got).all(), what
    if name == "bf16":
        _assert_bf16_close(got, ref)
    elif name == "fp16":
        _assert_f16_close(got, ref)
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def _check_layers(hiplib, name, cfg, flat, outs, semantics):
    """every mover of `cfg` against its restatement on the device's own stored inputs, every bias-only conv by _check_conv; a conv
    behind a mover must be finite (the pad lanes of a ragged granule are zeros, never -inf or what a pooled buffer held)"""
    secs = IO.parse_cfg(cfg)[1:]
    params = stream_params(cfg, flat)
    seen = set()
    for i, s in enumerate(secs):
        src = layer_inputs(secs, i)
        if min(src) < 0:
            continue          # (layer 0 reads the image)
        ins = [outs[j] for j in src]
        what = "layer %d (%s)" % (i, s["type"])
        if s["type"] == "convolutional":
            if secs[src[0]]["type"] in MOVERS:
                assert np.isfinite(outs[i]).all(), what + " behind a " + secs[src[0]]["type"]
            if "bias" in params[i]:
                _check_conv(hiplib, name, s, params[i], ins[0], outs[i], what)
                seen.add(("conv",) + conv_geometry(s))
        elif s["type"] == "shortcut":
            # a + b in fp32, rounded once to the storage type: the rule of test_op_shortcut_16bit
            y = ins[0].astype(np.float64) + ins[1].astype(np.float64)
            err = np.abs(outs[i].astype(np.float64) - y)
            bound = _storage_half_ulp(hiplib, y, _dt(hiplib, name)) + U * np.abs(y)
            assert outs[i].shape == y.shape and (err <= bound).all(), "%s %s: %g over at %s" % (what, name, float((err - bound).max()), np.unravel_index((err - bound).argmax(), err.shape))
            if name == "fp32":
                assert np.array_equal(outs[i], ins[0] + ins[1]), what
            seen.add("shortcut")
        else:
            want = mover_ref(s, i, ins, "darknet" if semantics == hiplib.SEM_DARKNET else "tf")
            if s["type"] == "upsample" and semantics == hiplib.SEM_TF:
                want = _round(name, want)          # the one mover that computes: TF's lerp in fp32, rounded once (test_upsample)
            assert outs[i].shape == want.shape, what
            bad = np.argwhere(outs[i] != want)
            assert bad.size == 0, "%s %s: %d elements differ, first at %s (channels %s)" % (what, name, len(bad), bad[0].tolist(), np.unique(bad[:, 3]).tolist())
            seen.add(s["type"])
    return seen


@pytest.mark.parametrize("name", DTYPES)
def test_mini_edges_layers_are_exact_on_their_stored_inputs(hiplib, edges, name):
    g = golden(FIXTURE)
    seen = _check_layers(hiplib, name, str(g["cfg"]), g["weights"], edges[name][0], hiplib.SEM_DARKNET)
    assert set(MOVERS) <= seen and {("conv", 3, 1, 0), ("conv", 3, 1, 2), ("conv", 3, 2, 2), ("conv", 3, 3, 2), ("conv", 3, 1, 1)} <= seen


def _c(filters, size, stride=1, padding=0, act="leaky"):
    return "[convolutional]\nfilters=%d\nsize=%d\nstride=%d\npad=0\npadding=%d\nactivation=%s\n\n" % (filters, size, stride, padding, act)


# TF semantics (space_to_depth, the bilinear 2x upsample), and the two conv geometries the reference's C code cannot pin (its 1x1 conv
# skips im2col: tools/make_golden.py, mini_edges_cfg): a 1x1 conv with padding=1, whose border is the bias alone, and a 1x1 conv with
# stride=2.  10 high x 12 wide:  0 conv 3x3 -> 20 | 1 reorg (C = 20) -> 5 x 6 x 80 | 2 conv 1x1 -> 12 | 3 upsample -> 10 x 12 x 12 |
# 4 reorg (C = 12) -> 5 x 6 x 48 | 5 conv 1x1 padding=1 -> 7 x 8 x 20 | 6 conv 1x1 stride=2 -> 4 x 4 x 12 | 7 upsample -> 8 x 8 x 12 |
# 8 maxpool 2/2 -> 4 x 4 x 12 | 9 route 6, 8: 12 + 12 channels, the second at offset 12 | 10 conv 3x3 -> the 4 x 4 x 6 map
TF_EDGES = ("[net]\nbatch=1\nwidth=12\nheight=10\nchannels=3\nyolo_output=map\n\n" + _c(20, 3, padding=1) + "[reorg]\nstride=2\n\n" + _c(12, 1) +
            "[upsample]\nstride=2\n\n[reorg]\nstride=2\n\n" + _c(20, 1, padding=1) + _c(12, 1, stride=2, act="linear") + "[upsample]\nstride=2\n\n" +
            "[maxpool]\nsize=2\nstride=2\n\n[route]\nlayers=6,8\n\n" + _c(6, 3, padding=1, act="linear"))


@pytest.mark.parametrize("name", DTYPES)
def test_tf_semantics_edges_are_exact_on_their_stored_inputs(hiplib, name):
    secs = IO.parse_cfg(TF_EDGES)
    assert [s[1:4] for s in IO.layer_shapes(secs)][:7] == [(10, 12, 20), (5, 6, 80), (5, 6, 12), (10, 12, 12), (5, 6, 48), (7, 8, 20), (4, 4, 12)]
    flat = IO.bf16_exact_filters(secs, IO.synth_weights(secs, seed=81))
    imgs = np.random.default_rng(82).integers(0, 256, (3, 10, 12, 3), dtype=np.uint8)
    outs, m = _layers(hiplib, TF_EDGES, flat, imgs, _dt(hiplib, name), hiplib.SEM_TF)
    seen = _check_layers(hiplib, name, TF_EDGES, flat, outs, hiplib.SEM_TF)
    assert {"reorg", "upsample", "maxpool", "route", ("conv", 1, 1, 1), ("conv", 1, 2, 0), ("conv", 1, 1, 0)} <= seen
    # the border of the padded 1x1 conv is the bias alone (leaky), rounded to the storage type
    p = stream_params(TF_EDGES, flat)[5]
    border = _round(name, np.where(p["bias"] > 0, p["bias"], np.float32(0.1) * p["bias"]).astype(np.float32))
    for edge in (outs[5][:, 0], outs[5][:, -1], outs[5][:, :, 0], outs[5][:, :, -1]):
        assert np.array_equal(edge, np.broadcast_to(border, edge.shape))
    assert np.array_equal(m, outs[-1])
    _, lean = _layers(hiplib, TF_EDGES, flat, imgs, _dt(hiplib, name), hiplib.SEM_TF, keep=False)
    assert np.array_equal(lean, m)


# padding > 1 under a conv whose input has whole 64-channel K-steps: the 16-bit tiled kernel then addresses a tap as (window origin) +
# (scalar tap offset), and the origin of a border window lies `padding` rows and columns outside the image -- it must not wrap below zero.
# 9 high x 11 wide:  0 conv 3x3 -> 64 | 1 conv 3x3 padding=2 -> 11 x 13 x 20 | 2 conv 3x3 padding=2 stride=2 -> 7 x 8 x 12 (16 channels
# per K-step: the per-lane tap cursor) | 3 conv 1x1 -> the map
WIDE_PAD = ("[net]\nbatch=1\nwidth=11\nheight=9\nchannels=3\nyolo_output=map\n\n" + _c(64, 3, padding=1) + _c(20, 3, padding=2) + _c(12, 3, stride=2, padding=2) +
            _c(6, 1, act="linear"))


@pytest.mark.parametrize("name", DTYPES)
def test_padding_2_under_whole_k_steps(hiplib, name):
    secs = IO.parse_cfg(WIDE_PAD)
    assert [s[1:4] for s in IO.layer_shapes(secs)] == [(9, 11, 64), (11, 13, 20), (7, 8, 12), (7, 8, 6)]
    flat = IO.bf16_exact_filters(secs, IO.synth_weights(secs, seed=85))
    imgs = np.random.default_rng(86).integers(0, 256, (3, 9, 11, 3), dtype=np.uint8)
    outs, m = _layers(hiplib, WIDE_PAD, flat, imgs, _dt(hiplib, name), hiplib.SEM_DARKNET)
    assert {("conv", 3, 1, 2), ("conv", 3, 2, 2), ("conv", 1, 1, 0)} <= _check_layers(hiplib, name, WIDE_PAD, flat, outs, hiplib.SEM_DARKNET)
    _, lean = _layers(hiplib, WIDE_PAD, flat, imgs, _dt(hiplib, name), hiplib.SEM_DARKNET, keep=False)
    assert np.array_equal(lean, m)


# ---- (d) the plan that reuses pooled buffers == the plan that keeps every layer, 16-bit storage ----
# A 27-channel tensor first (pixel stride 32), 20-channel movers behind it at no more pixels: in the pooled plan the max-pool of layer 2
# writes into the buffer the 27-channel tensor left, so a channel that is never written holds a stale value there and a zero in the
# plan that keeps every layer.  Layer 7's conv is leaky with one reader: the pooled plan folds the [shortcut] into it.
REUSE = ("[net]\nbatch=1\nwidth=22\nheight=15\nchannels=3\nyolo_output=map\n\n" + _c(27, 3, padding=1) + _c(20, 3, padding=1) + "[maxpool]\nsize=2\nstride=2\n\n" +
         _c(20, 3, padding=1) + "[maxpool]\nsize=3\nstride=1\npadding=0\n\n[upsample]\nstride=2\n\n" + _c(12, 3, padding=1) + _c(20, 1) +
         "[shortcut]\nfrom=5\nactivation=linear\n\n[maxpool]\nsize=2\nstride=1\n\n[reorg]\nstride=2\n\n" + _c(12, 1) + "[upsample]\nstride=2\n\n[route]\nlayers=-1,9\n\n" +
         _c(6, 3, padding=1, act="linear"))


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("which", ["mini_edges", "reuse"])
def test_pooled_plan_equals_layer_by_layer_plan_16bit(hiplib, edges, name, which):
    if which == "mini_edges":
        g = golden(FIXTURE); cfg, flat, imgs = str(g["cfg"]), g["weights"], g["images_u8"]
        kept = edges[name][1]
    else:
        cfg = REUSE; secs = IO.parse_cfg(cfg)
        assert [s[3] for s in IO.layer_shapes(secs)][:3] == [27, 20, 20] and IO.layer_shapes(secs)[-1][1:4] == (14, 22, 6)
        rc, table = hiplib.plan_table(cfg, dtype=_dt(hiplib, name), max_batch=3)
        assert rc == 0, table
        flat = IO.synth_weights(secs, seed=91); imgs = np.random.default_rng(92).integers(0, 256, (3, 15, 22, 3), dtype=np.uint8)
        _, kept = _layers(hiplib, cfg, flat, imgs, _dt(hiplib, name), hiplib.SEM_DARKNET)
    _, lean = _layers(hiplib, cfg, flat, imgs, _dt(hiplib, name), hiplib.SEM_DARKNET, keep=False)
    assert np.isfinite(kept).all() and float(np.abs(kept).max()) > 0.1
    bad = np.argwhere(lean != kept)
    assert bad.size == 0, "%s %s: %d map elements differ between the two plans, first at %s" % (which, name, len(bad), bad[0].tolist())
