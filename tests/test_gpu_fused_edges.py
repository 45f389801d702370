"""The fused first-stage kernels off YOLO's input sizes: the fused stem (conv_stem_c32_c64: staged and uint8 forms, with its 1x1 tail), the
32 -> 64 halo conv, the 64 -> 128 stride-2 conv, conv3 + shortcut + stride-2 in one launch, the fused residual block, the image layer's
direct kernels and the split-fp16 stem.  Their planner rules and `*_ok` predicates accept any input size, any slope-family activation per
layer and channel windows on either side; every earlier test ran them at multiples of 32 (and 52) with leaky activations.

The network is darknet-53's first stage as a map network (tests/test_fused_edges_host.py: stage_cfg; that file pins the plan rows of
every fixture without a device).  Sizes, height x width:
  27 x 37   raw rows of 111 bytes start at all four byte alignments of the uint8 gather, N * H * W * 3 is no multiple of 4 unless N is; the
            stem's 14 x 19 output is two ragged tile rows and two tile columns, the second 3 wide with its window past the right edge; the
            7 x 10 output of conv3 + stride-2 is two ragged rows and columns of 4 x 8 tiles; 7 x 10 fails the block's 115 % rule
  50 x 50   stem output 25 x 25, an odd grid into conv3 + stride-2; 13 x 13: the residual block on exactly one block
  99 x 47   50 x 24 -> 25 x 12: the block on ragged blocks, 13 + 12 rows of 12 columns
  5 x 3     3 x 2 -> 2 x 1: the smallest the predicates of conv3 + stride-2 and of the stride-2 conv accept; every window is mostly
            padding, fewer tiles than prefetch stages
  2 x 2     1 x 1 throughout: both predicates refuse (H >= 2) at launch time; the plan still names the fused launch, so a forward that
            succeeds took yolo_run.cpp's fall-back to the members' own kernels (launch_conv_c3s2 refuses what its predicate refuses)
Every kernel named above masks by position and addresses images through descriptors or guarded pointers: no size is refused.

Checks: (1) the plan that keeps every layer, each layer against the restatements on the device's own stored inputs (the helpers and bounds
of test_gpu_edges.py / test_gpu_tile_matrix.py, unchanged), and bit for bit against the same plan without the halo and stride-2 kernels;
(2) the fused plan against the plan that keeps every layer and the plan under each knob, bit for bit, the map and every tensor still
stored; (3) the same images as host uint8, device uint8 and float32 = byte / 255: identical bits, the last image's bottom-right pixel
named; (4) one image alone == its slice of the batch; (5) mixed activations; (6) channel windows; and every case asserts its plan rows
first.  The uint8 form of the stem serves batches of whole dwords only (stage_in): at the odd sizes batch 4 is what reaches it."""
import contextlib
import os
import numpy as np
import pytest
from yolo_tensorflow_amd import darknet_io as IO
from test_edges_host import layer_inputs, stream_params
from test_fused_edges_host import (KNOBS, SIZES, PAIR_SIZES, VARIANT_SIZES, LARGE_BATCHES, MIXED_BIAS_ONLY, stage_cfg, mixed_cfg, plan_rows, fused_of,
                                   expected_fused, block_planned)
from test_gpu_edges import _check_conv, _check_layers, _round
from test_gpu_tile_matrix import _check_fp16x2

pytestmark = pytest.mark.gpu
DIRECT = 1000          # CONV_CFG_DIRECT: the image layer's direct kernel (conv_c8_direct, conv_c8_direct_pair)
SCALE = np.float32(1.0 / 255.0)
ids = lambda hw: "%dx%d" % hw


def _dt(hiplib, fam):
    return {"bf16": hiplib.BF16, "fp16": hiplib.FP16, "fp16x2": hiplib.FP16X2}[fam]


@contextlib.contextmanager
def _env(knobs):
    """the planner reads its knobs when a context is created"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({k: "1" for k in knobs})
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def _engine(hiplib, cfg, flat, fam, max_batch, keep=False, knobs=()):
    with _env(knobs):
        eng = hiplib.Engine(cfg, max_batch=max_batch, dtype=_dt(hiplib, fam), semantics=hiplib.SEM_DARKNET, keep_layers=keep)
    eng.set_weights(flat)
    return eng


def _read(hiplib, eng, n):
    """(the map, {layer: tensor} of every layer the plan still stores) of the last forward"""
    stored = {}
    for i in range(eng.num_layers):
        try:
            stored[i] = eng.layer_output(i, n)
        except hiplib.YoloError:
            pass
    return eng.output_map(n), stored


def _run(hiplib, cfg, flat, imgs, fam, keep=False, knobs=(), scale=1.0 / 255.0):
    eng = _engine(hiplib, cfg, flat, fam, len(imgs), keep, knobs)
    try:
        eng.forward(imgs, want_detections=False, scale=scale)
        return _read(hiplib, eng, len(imgs))
    finally:
        eng.close()


def _weights(cfg, seed):
    secs = IO.parse_cfg(cfg)
    return IO.bf16_exact_filters(secs, IO.synth_weights(secs, seed=seed))


def _images(hw, n, seed=7):
    return np.random.default_rng(seed + 100 * hw[0] + hw[1]).integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)


def _same(a, b, what):
    assert a.shape == b.shape, what
    bad = np.argwhere(a != b)
    assert bad.size == 0, "%s: %d elements differ, first at %s (%r against %r)" % (what, len(bad), bad[0].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def _same_plan(got, want, what):
    """(map, stored) of a plan against the (map, every layer) of the plan that keeps every layer"""
    _same(got[0], want[0], what + ": the map")
    for i, t in got[1].items():
        _same(t, want[1][i], "%s: layer %d" % (what, i))


class _Kept:
    """what _check_fp16x2 reads of a network: the plan that keeps every layer"""
    def __init__(self, net, cfg, flat, x0, outs):
        self.net, self.cfg, self.flat, self.x0, self.outs = net, cfg, flat, x0, outs
        self.secs = IO.parse_cfg(cfg)[1:]


def _check_kept(hiplib, fam, cfg, flat, imgs, kept, what, affine=False):
    """check 1 on the (map, layers) of the plan that keeps every layer"""
    m, outs = kept
    outs = [outs[i] for i in range(len(outs))]
    x0 = imgs.astype(np.float32) * SCALE
    if affine:
        x0 = x0 * np.float32(2) + np.float32(-1)
    assert np.array_equal(m, outs[-1]) and np.isfinite(m).all() and float(np.abs(m).max()) > 1e-3, what
    if fam == "fp16x2":
        worst = _check_fp16x2(_Kept(what, cfg, flat, x0, outs))
        print("%s fp16x2: worst layer %.3e of the tensor's scale (bound 4e-6)" % (what, worst))
        return
    seen = _check_layers(hiplib, fam, cfg, flat, outs, hiplib.SEM_DARKNET)
    secs = IO.parse_cfg(cfg)[1:]
    if "batch_normalize" not in secs[0]:
        _check_conv(hiplib, fam, secs[0], stream_params(cfg, flat)[0], _round(fam, x0), outs[0], what + " layer 0 (the image layer)")
        assert {("conv", 3, 1, 1), ("conv", 3, 2, 1), ("conv", 1, 1, 0), "shortcut"} <= seen, seen
    else:
        assert {("conv", 3, 1, 1), ("conv", 1, 1, 0), "shortcut"} <= seen, seen          # (the mixed variant: its bias-only layer and the map conv)


# ---- checks 1, 2, 7: every size, batches 1 and 3 ----
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("fam", ["bf16", "fp16"])
@pytest.mark.parametrize("hw", SIZES, ids=ids)
def test_stage_layer_by_layer_and_fused_against_unfused(hiplib, hw, fam, batch):
    cfg = stage_cfg(hw); flat = _weights(cfg, 11 + hw[0]); imgs = _images(hw, batch); dt = _dt(hiplib, fam)
    what = "%dx%d %s batch %d" % (hw + (fam, batch))
    # the plans this case means to run
    assert fused_of(plan_rows(cfg, dt, batch, keep=True)) == expected_fused(hw, fam, keep=True) == {3: ("halo", "none", -1), 5: ("s2", "none", -1)}
    fused = expected_fused(hw, fam)
    assert fused_of(plan_rows(cfg, dt, batch)) == fused and fused[1] == ("tiled", "stem", 1) and fused[5] == ("s2", "c3s2", 5)
    assert (fused.get(7) == ("tiled", "resblock", 7)) == block_planned(hw) == (hw in ((50, 50), (99, 47)))          # not at 7 x 10, 2 x 1, 1 x 1
    # 1: the plan that keeps every layer -- conv_c8_direct, the halo conv and the stride-2 conv on their own
    eng = _engine(hiplib, cfg, flat, fam, batch, keep=True)
    try:
        assert eng.resolved_tile_configs(batch)[0] == DIRECT
        eng.forward(imgs, want_detections=False)
        kept = _read(hiplib, eng, batch)
    finally:
        eng.close()
    assert sorted(kept[1]) == list(range(10))
    _check_kept(hiplib, fam, cfg, flat, imgs, kept, what)
    tiled = _run(hiplib, cfg, flat, imgs, fam, keep=True, knobs=("YOLO_NO_HALO", "YOLO_NO_S2"))
    _same_plan(tiled, kept, what + ": the tiled kernel in place of the halo and stride-2 kernels")
    # 2: the fused plan, and the plan under each knob
    got = _run(hiplib, cfg, flat, imgs, fam)
    assert 2 in got[1] and 5 in got[1], sorted(got[1])          # the stem's 1x1 tail and the stride-2 output are stored in every plan
    _same_plan(got, kept, what + ": the fused plan")
    for knob in KNOBS:
        with _env((knob,)):
            assert fused_of(plan_rows(cfg, dt, batch)) == expected_fused(hw, fam, knobs=(knob,))
        _same_plan(_run(hiplib, cfg, flat, imgs, fam, knobs=(knob,)), kept, "%s: the plan under %s" % (what, knob))


# ---- checks 1, 2, 7 in split fp16: the pair stem and conv_c8_direct_pair ----
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hw", PAIR_SIZES, ids=ids)
def test_stage_in_split_fp16(hiplib, hw, batch):
    cfg = stage_cfg(hw); flat = IO.synth_weights(IO.parse_cfg(cfg), seed=13 + hw[0]); imgs = _images(hw, batch)
    what = "%dx%d fp16x2 batch %d" % (hw + (batch,))
    want = {0: ("tiled", "pair-stem", 1), 1: ("tiled", "pair-stem", 1)} if hw != (27, 37) else {}          # odd size: no pair stem
    assert fused_of(plan_rows(cfg, hiplib.FP16X2, batch)) == want == expected_fused(hw, "fp16x2")
    assert fused_of(plan_rows(cfg, hiplib.FP16X2, batch, keep=True)) == {}
    eng = _engine(hiplib, cfg, flat, "fp16x2", batch, keep=True)
    try:
        assert eng.resolved_tile_configs(batch)[0] == DIRECT          # conv_c8_direct_pair: 32 filters on the image's three blocks
        eng.forward(imgs, want_detections=False)
        kept = _read(hiplib, eng, batch)
    finally:
        eng.close()
    _check_kept(hiplib, "fp16x2", cfg, flat, imgs, kept, what)
    _same_plan(_run(hiplib, cfg, flat, imgs, "fp16x2"), kept, what + ": the fused plan")
    for knob in KNOBS:
        _same_plan(_run(hiplib, cfg, flat, imgs, "fp16x2", knobs=(knob,)), kept, "%s: the plan under %s" % (what, knob))


# ---- check 3: uint8 from the host, uint8 on the device, float32 = byte / 255 ----
def _three_forms(hiplib, eng, imgs, what):
    """-> (map, stored) of the host uint8 form, after comparing the three forms bit for bit"""
    import torch
    n = len(imgs)
    f32 = imgs.astype(np.float32) * SCALE
    forms = []
    for name, x, scale in (("host uint8", imgs, 1.0 / 255.0), ("device uint8", torch.from_numpy(imgs).cuda(), 1.0 / 255.0), ("float32", f32, 1.0)):
        eng.forward(x, want_detections=False, scale=scale)
        forms.append((name, _read(hiplib, eng, n)))
    base = forms[0][1]
    assert 2 in base[1]
    for name, got in forms[1:]:
        # the last image's bottom-right pixel first, by name: where a batch whose byte count is no multiple of 4 loses its last bytes
        for t, u, tensor in [(got[0], base[0], "the map")] + [(got[1][i], base[1][i], "layer %d" % i) for i in sorted(base[1])]:
            assert np.array_equal(t[-1, -1, -1], u[-1, -1, -1]), "%s: %s against host uint8, %s, bottom-right pixel of the last image: %r against %r" % (what, name, tensor, t[-1, -1, -1], u[-1, -1, -1])
        assert sorted(got[1]) == sorted(base[1])
        _same_plan(got, base, "%s: %s against host uint8" % (what, name))
    return base


@pytest.mark.parametrize("fam", ["bf16", "fp16"])
@pytest.mark.parametrize("hw,affine", [(hw, False) for hw in SIZES] + [(hw, True) for hw in VARIANT_SIZES], ids=lambda v: ids(v) if isinstance(v, tuple) else ("affine" if v else "plain"))
def test_uint8_form_against_the_conversion_launch(hiplib, hw, affine, fam):
    """batches 1, 3 and 4 of one context (4: whole dwords at the odd sizes too, where the stem gathers the raw rows itself).  Then an all-zero
    batch whose very last source pixel is 255: a dropped byte moves the bottom-right outputs by far more than any rounding -- and the pixel
    must move them, or the case has no power.  Before stage_in kept batches of ragged byte counts away from the uint8 form this failed at
    27 x 37, 99 x 47 and 5 x 3, batch 1 already: the map's bottom-right pixel off by up to 2.6e-3 / 4.4e-3 / 3.2e-3 (docs/NOTEBOOK.md)."""
    cfg = stage_cfg(hw, affine=affine); flat = _weights(cfg, 17 + hw[0]); imgs = _images(hw, 4, seed=9)
    assert fused_of(plan_rows(cfg, _dt(hiplib, fam), 4)) == expected_fused(hw, fam)
    eng = _engine(hiplib, cfg, flat, fam, 4)
    try:
        for n in (1, 3, 4):
            what = "%dx%d %s%s batch %d" % (hw + (fam, " mul=2 add=-1" if affine else "", n))
            got = _three_forms(hiplib, eng, imgs[:n], what)
            if n == 3:          # against the plan that keeps every layer (its layer 0 is stored: the conversion launch, every layer's own kernel)
                kept = _run(hiplib, cfg, flat, imgs[:n], fam, keep=True)
                _same_plan(got, kept, what + ": against the plan that keeps every layer")
                if affine:
                    _check_kept(hiplib, fam, cfg, flat, imgs[:n], kept, what, affine=True)
        for n in (1, 3, 4):
            what = "%dx%d %s%s batch %d, a zero batch with its last pixel at 255" % (hw + (fam, " mul=2 add=-1" if affine else "", n))
            dark = np.zeros_like(imgs[:n])
            eng.forward(dark, want_detections=False)
            zero = _read(hiplib, eng, n)
            dark[-1, -1, -1, :] = 255
            lit = _three_forms(hiplib, eng, dark, what)
            moved = float(np.abs(lit[1][2][-1, -1, -1] - zero[1][2][-1, -1, -1]).max())
            print("%s: moves layer 2's bottom-right pixel by up to %.3f" % (what, moved))
            assert moved > 0, what          # layer 2's bottom-right pixel sees the source's
    finally:
        eng.close()


# ---- check 4: one image alone == its slice of the batch ----
@pytest.mark.parametrize("fam", ["bf16", "fp16", "fp16x2"])
@pytest.mark.parametrize("hw", SIZES + PAIR_SIZES[:2], ids=ids)
def test_one_image_alone_equals_its_slice_of_the_batch(hiplib, hw, fam):
    cfg = stage_cfg(hw); flat = _weights(cfg, 19 + hw[0]); imgs = _images(hw, 3, seed=10)
    eng = _engine(hiplib, cfg, flat, fam, 3)
    try:
        eng.forward(imgs, want_detections=False)
        whole = _read(hiplib, eng, 3)
        for k in (1, 2):
            eng.forward(imgs[k:k + 1], want_detections=False)
            one = _read(hiplib, eng, 1)
            _same(one[0], whole[0][k:k + 1], "%dx%d %s: image %d alone, the map" % (hw + (fam, k)))
            assert sorted(one[1]) == sorted(whole[1])
            for i, t in one[1].items():
                _same(t, whole[1][i][k:k + 1], "%dx%d %s: image %d alone, layer %d" % (hw + (fam, k, i)))
    finally:
        eng.close()


# ---- check 5: a different slope-family activation on every member of a fused launch, batch norm folded, one bias-only layer ----
@pytest.mark.parametrize("fam", ["bf16", "fp16"])
@pytest.mark.parametrize("hw", VARIANT_SIZES, ids=ids)
def test_mixed_activations(hiplib, hw, fam):
    """a fused launch that swapped two of act0 / act1 / act2, act3 / act5 or the block's act1 / act2 differs from the plan in which every
    layer runs its own kernel with its own activation; that plan's bias-only layer (leaky), shortcuts and map conv are checked on their
    stored inputs, and every activation changes the tensor it is applied to (else a swap could hide)"""
    cfg = mixed_cfg(hw); secs = IO.parse_cfg(cfg); flat = _weights(cfg, 23 + hw[0]); imgs = _images(hw, 3, seed=11)
    what = "%dx%d %s mixed activations" % (hw + (fam,))
    assert fused_of(plan_rows(cfg, _dt(hiplib, fam), 3)) == expected_fused(hw, fam) and secs[1 + MIXED_BIAS_ONLY]["activation"] == "leaky"
    kept = _run(hiplib, cfg, flat, imgs, fam, keep=True)
    _check_kept(hiplib, fam, cfg, flat, imgs, kept, what)
    for i, s in enumerate(secs[1:9]):
        if s["type"] == "convolutional":
            neg = float((kept[1][i] < 0).mean())
            print("%s layer %d (%s): %.3f of the outputs negative" % (what, i, s["activation"], neg))
            assert (neg == 0.0) if s["activation"] == "relu" else (neg > 0.05), (what, i)          # negative inputs reach every activation
    _same_plan(_run(hiplib, cfg, flat, imgs, fam), kept, what + ": the fused plan")
    for knob in KNOBS[:4]:
        _same_plan(_run(hiplib, cfg, flat, imgs, fam, knobs=(knob,)), kept, "%s: the plan under %s" % (what, knob))
    _same_plan(_run(hiplib, cfg, flat, imgs[:1], fam), (kept[0][:1], {i: t[:1] for i, t in kept[1].items()}), what + ": the fused plan, batch 1")


# ---- check 6: the fused kernels read and write windows of concatenations ----
@pytest.mark.parametrize("fam", ["bf16", "fp16"])
@pytest.mark.parametrize("hw", VARIANT_SIZES, ids=ids)
def test_channel_windows(hiplib, hw, fam):
    """layers 1 and 2 are windows of a 96-channel concatenation (the stem writes both; the halo conv and conv3 + stride-2 read layer 2 at pixel
    stride 96, channel offset 64, their shortcut source at stride 96); layer 5 and the block's output are windows of a 272-channel one (the
    stride-2 conv and conv3 + stride-2 write at offset 128, the block reads there and writes at offset 0).  Every fusion survives
    (test_fused_edges_host.py pins the storage of each tensor); the routes must come out as the concatenation of their sources"""
    cfg = stage_cfg(hw, cat=True); flat = _weights(cfg, 29 + hw[0]); imgs = _images(hw, 3, seed=12)
    what = "%dx%d %s channel windows" % (hw + (fam,))
    rows = plan_rows(cfg, _dt(hiplib, fam), 3)
    assert fused_of(rows) == expected_fused(hw, fam) and rows[2]["storage"] == rows[9]["storage"] and rows[5]["storage"] == rows[8]["storage"] == rows[12]["storage"]
    kept = _run(hiplib, cfg, flat, imgs, fam, keep=True)
    assert sorted(kept[1]) == list(range(14))
    m, outs = kept
    x0 = imgs.astype(np.float32) * SCALE
    seen = _check_layers(hiplib, fam, cfg, flat, [outs[i] for i in range(14)], hiplib.SEM_DARKNET)
    _check_conv(hiplib, fam, IO.parse_cfg(cfg)[1], stream_params(cfg, flat)[0], _round(fam, x0), outs[0], what + " layer 0 (the image layer)")
    assert {("conv", 3, 1, 1), ("conv", 3, 2, 1), ("conv", 1, 1, 0), "shortcut", "route"} <= seen, seen
    _same_plan(_run(hiplib, cfg, flat, imgs, fam, keep=True, knobs=("YOLO_NO_HALO", "YOLO_NO_S2")), kept, what + ": the tiled kernel in place of the halo and stride-2 kernels")
    _same_plan(_run(hiplib, cfg, flat, imgs, fam), kept, what + ": the fused plan")
    for knob in KNOBS[:4]:
        _same_plan(_run(hiplib, cfg, flat, imgs, fam, knobs=(knob,)), kept, "%s: the plan under %s" % (what, knob))
    _same_plan(_run(hiplib, cfg, flat, imgs[:1], fam), (m[:1], {i: t[:1] for i, t in outs.items()}), what + ": the fused plan, batch 1")


# ---- every persistent workgroup of the stem and of conv3 + stride-2 walks at least four tiles ----
@pytest.mark.parametrize("fam", ["bf16", "fp16"])
@pytest.mark.parametrize("n", LARGE_BATCHES)
def test_large_batch_at_27x37(hiplib, n, fam):
    """257 images (odd: the conversion launch feeds the staged form of the stem) and 260 (whole dwords: the uint8 form), 4 tiles per image
    in either launch, 256 workgroups (test_fused_edges_host.py: test_large_batch_count).  The fused plan against the plan that keeps every
    layer and the plan without conv3 + stride-2; uint8 against float32; the first three images against a batch of three."""
    hw = (27, 37)
    cfg = stage_cfg(hw); flat = _weights(cfg, 31); imgs = _images(hw, n, seed=13)
    what = "27x37 %s batch %d" % (fam, n)
    assert fused_of(plan_rows(cfg, _dt(hiplib, fam), n)) == expected_fused(hw, fam)
    kept = _run(hiplib, cfg, flat, imgs, fam, keep=True)
    small = _run(hiplib, cfg, flat, imgs[:3], fam, keep=True)
    _check_kept(hiplib, fam, cfg, flat, imgs[:3], small, what + ", its first three images alone")
    _same_plan((small[0], {i: small[1][i] for i in (2, 5, 9)}), (kept[0][:3], {i: t[:3] for i, t in kept[1].items()}), what + ": three images alone against their slice")
    eng = _engine(hiplib, cfg, flat, fam, n)
    try:
        eng.forward(imgs, want_detections=False)
        got = _read(hiplib, eng, n)
        _same_plan(got, kept, what + ": the fused plan")
        eng.forward(imgs.astype(np.float32) * SCALE, want_detections=False, scale=1.0)
        _same_plan(_read(hiplib, eng, n), got, what + ": float32 against uint8")
    finally:
        eng.close()
    _same_plan(_run(hiplib, cfg, flat, imgs, fam, knobs=("YOLO_NO_C3S2",)), kept, what + ": the plan under YOLO_NO_C3S2")
