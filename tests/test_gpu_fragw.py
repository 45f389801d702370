"""The free-running halo forms with their filters as MFMA fragments straight from the fragment-order image (conv_igemm_kernel.h FRAGW,
yolo_pack.cpp filter_fragments) instead of through filter stages in LDS.  K order and every rounding point are the LDS path's, so every
comparison here is np.array_equal: the new path against the same tile id with YOLO_NO_FRAGW=1 (the LDS path, the same build) and against
the tiled id 16."""
import numpy as np
import pytest
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu

# (n, h, w, cin, cout): one block and four blocks of 13 x 13 (13, 26); ragged blocks -- 25 = 13 + 12 both ways, and 52 x 46 = three blocks and
# one of 7 columns per block row (the halo forms refuse a layer whose blocks cover more than 115 % of it, conv_halo13.hip halo_ok: 20 x 20 =
# 13 + 7 both ways is refused, 52 x 46 is the smallest layer with a 7-wide block they accept); one, two and three 64-channel chunks (no next
# chunk at all, the look-ahead of the last K-step, both parities of the nine-step chunk); whole channel tiles, a tile whose last row is a zero
# row of the image (255), one that is mostly zero rows (18), and two / four channel tiles (512 with 256- and 128-channel ids)
GEOMS = [(2, 13, 13, 64, 256), (2, 26, 26, 128, 256), (2, 25, 25, 192, 256), (2, 13, 13, 128, 255), (2, 26, 26, 64, 18), (1, 52, 46, 64, 255),
         (2, 13, 13, 192, 512), (2, 26, 26, 64, 512)]
_cache = {}


def _case(hiplib, dtype_name, geom):
    """inputs of a geometry and the tiled form's result with and without the shortcut: computed once, read-only afterwards"""
    key = (dtype_name,) + geom
    if key not in _cache:
        n, h, wd, cin, cout = geom
        dt = hiplib.BF16 if dtype_name == "bf16" else hiplib.FP16
        rng = np.random.default_rng(h * 100000 + cin * 1000 + cout)
        x = rng.standard_normal((n, h, wd, cin)).astype(np.float32)
        w = (rng.standard_normal((3, 3, cin, cout)) * 0.05).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        res = rng.standard_normal((n, h, wd, cout)).astype(np.float32)
        want = [hiplib.op_conv2d(x, w, b, act=1, residual=r, dtype=dt, tile_cfg=16) for r in (None, res)]
        for a in (x, w, b, res, *want): a.setflags(write=False)
        assert np.abs(want[0]).max() > 0.5
        _cache[key] = (dt, x, w, b, res, want)
    return _cache[key]


def _on_off(hiplib, monkeypatch, x, w, b, r, dt, cfg):
    monkeypatch.delenv("YOLO_NO_FRAGW", raising=False)
    on = hiplib.op_conv2d(x, w, b, act=1, residual=r, dtype=dt, tile_cfg=cfg)
    monkeypatch.setenv("YOLO_NO_FRAGW", "1")
    off = hiplib.op_conv2d(x, w, b, act=1, residual=r, dtype=dt, tile_cfg=cfg)
    monkeypatch.delenv("YOLO_NO_FRAGW", raising=False)
    return on, off


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("cfg", [40, 41, 42, 43])
def test_fragment_path_equals_lds_path_and_tiled_form(hiplib, monkeypatch, cfg, dtype_name):
    for geom in GEOMS:
        dt, x, w, b, res, want = _case(hiplib, dtype_name, geom)
        for r, ref in ((None, want[0]), (res, want[1])):
            on, off = _on_off(hiplib, monkeypatch, x, w, b, r, dt, cfg)
            assert np.array_equal(on, off), (cfg, dtype_name, geom, r is not None, "vs the LDS path")
            assert np.array_equal(on, ref), (cfg, dtype_name, geom, r is not None, "vs tiled id 16")


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
def test_fragment_path_on_rectangular_blocks(hiplib, monkeypatch, dtype_name):
    """10 x 19 blocks (54: x 256 channels, 55: x 128) and 5 x 19 strips (56), at 38 x 38 (4 x 2 / 8 x 2 blocks, the last row ragged) and 19 x 19"""
    dt = hiplib.BF16 if dtype_name == "bf16" else hiplib.FP16
    rng = np.random.default_rng(54)
    for h in (38, 19):
        x = rng.standard_normal((2, h, h, 128)).astype(np.float32)
        w = (rng.standard_normal((3, 3, 128, 256)) * 0.05).astype(np.float32)
        b = rng.standard_normal(256).astype(np.float32)
        res = rng.standard_normal((2, h, h, 256)).astype(np.float32)
        want = hiplib.op_conv2d(x, w, b, act=1, residual=res, dtype=dt, tile_cfg=16)
        for cfg in (54, 55, 56):
            on, off = _on_off(hiplib, monkeypatch, x, w, b, res, dt, cfg)
            assert np.array_equal(on, off) and np.array_equal(on, want), (cfg, dtype_name, h)


def _conv(f, size, act="leaky", bn=1):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=1\npad=1\nactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", f, size, act)


def _tail_net(size, head):
    """3x3 (256) with the 1x1 (128) behind it as its tail; 3x3 (256) + shortcut with a 1x1 tail on the summed tile; 3x3 (256) whose tail is
    the detection head (`head` filters)"""
    t = "[net]\nwidth=%d\nheight=%d\nchannels=3\n\n" % (size, size)
    t += _conv(64, 3) + _conv(256, 3) + _conv(128, 1) + _conv(256, 3) + "[shortcut]\nfrom=-3\nactivation=linear\n\n" + _conv(128, 1) + _conv(256, 3) + _conv(head, 1, "linear", 0)
    return t + "[yolo]\nmask=0,1,2\nanchors=10,13, 16,30, 33,23\nclasses=%d\nnum=3\n" % (head // 3 - 5)


def _engine(hiplib, monkeypatch, txt, flat, batch, dtype, off, plan=None, keep=False):
    if off: monkeypatch.setenv("YOLO_NO_FRAGW", "1")
    else: monkeypatch.delenv("YOLO_NO_FRAGW", raising=False)
    eng = hiplib.Engine(txt, max_batch=batch, dtype=dtype, keep_layers=keep)
    eng.set_weights(flat)
    monkeypatch.delenv("YOLO_NO_FRAGW", raising=False)
    if plan is not None: eng.set_tile_configs(plan)
    return eng


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("size,head", [(26, 75), (25, 18)])
def test_fragment_path_with_the_1x1_tail_and_the_head_tail(hiplib, monkeypatch, size, head, dtype_name):
    """id 40 hosting the fused 1x1 tail (plain, and behind a folded shortcut) and a head as the tail (75 filters of a VOC head, 18 of a
    one-class head), 26 x 26 and ragged 25 x 25, batch 2: detections with the switch on and off, and against the layer-by-layer plan"""
    dtype = hiplib.BF16 if dtype_name == "bf16" else hiplib.FP16
    txt = _tail_net(size, head)
    flat = IO.synth_weights(IO.parse_cfg(txt), seed=size + head)
    img = np.random.default_rng(size).integers(0, 256, (2, size, size, 3), dtype=np.uint8)
    plan = [-1, 10040, -1, 10040, -1, -1, 10040, -1, -1]
    dets = []
    for off, p, keep in ((False, plan, False), (True, plan, False), (False, None, True)):
        eng = _engine(hiplib, monkeypatch, txt, flat, 2, dtype, off, plan=p, keep=keep)
        if p is not None:
            ids = [int(v) for v in eng.resolved_tile_configs(2)]
            assert [ids[i] for i in (1, 3, 6)] == [40, 40, 40] and [ids[i] for i in (2, 5, 7)] == [-1, -1, -1]      # the three 1x1 convs ride as tails
        dets.append(eng.forward(img))
        eng.close()
    assert np.abs(dets[0]).max() > 0
    assert np.array_equal(dets[0], dets[1]) and np.array_equal(dets[0], dets[2])


def test_fragment_path_whole_network(hiplib, monkeypatch):
    """YOLOv3, batch 3, at 416 x 416: the smallest input the cfg plans at (a multiple of 32: 104 x 104 fails its route at layer 86) whose
    3x3 / stride 1 layers (104, 52, 26, 13) all tile into 13 x 13 blocks.  Detections with the switch on and off, and with the switch on
    under plans that put id 42 / id 40 on every layer that runs them."""
    txt = IO.with_input_size(IO.cfg_text("yolov3"), 416)
    flat = IO.synth_weights(IO.parse_cfg(txt), seed=3)
    img = np.random.default_rng(416).integers(0, 256, (3, 416, 416, 3), dtype=np.uint8)
    eng = _engine(hiplib, monkeypatch, txt, flat, 3, hiplib.BF16, True)
    want = eng.forward(img)
    eng.close()
    assert np.abs(want).max() > 0
    eng = _engine(hiplib, monkeypatch, txt, flat, 3, hiplib.BF16, False)
    assert np.array_equal(eng.forward(img), want)
    ids = [int(v) for v in eng.resolved_tile_configs(3)]
    for cfg in (42, 40):
        eng.set_tile_configs([cfg if v >= 0 else -1 for v in ids])
        assert [int(v) for v in eng.resolved_tile_configs(3)].count(cfg) >= 20
        assert np.array_equal(eng.forward(img), want), cfg
    eng.close()
