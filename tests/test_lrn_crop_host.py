"""[normalization] / [lrn], [crop] and the classifier's centre-crop fit, host side (no device): what the planner accepts and refuses, the shapes
darknet_io derives, the exported symbols, the shipped AlexNet with LRN -- and the numpy restatements the GPU tests (test_gpu_lrn_crop.py) compare the
device against, checked here against the compiled reference's recorded outputs (tests/golden/mini_lrn.npz, lrn_crop_cases.npz; tools/make_golden.py
lrn_crop).

The stand-alone [normalization] cases, (channels, size), and why each is there:
    (7, 5) (13, 6) (9, 3) (5, 1)   general shapes: odd and even windows (an even one reaches further up than down), the one-channel window
    (3, 5)                         the window covers every channel
    (2, 5) (2, 4)                  size / 2 == C: the channel the reference never adds does not exist (odd and even size)
    (96, 5)                        AlexNet's first LRN
    (520, 5)                       65 granules: more than a wave has lanes
    (24, 16)                       a window of 16: 8 channels up, 7 down -- into both neighbouring granules
    (11, 5) with beta = 0.6        a power other than the default 0.75"""
import os
import subprocess
import sys
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import hip, darknet_io as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LRN_CASES = [(7, 5), (13, 6), (9, 3), (5, 1), (3, 5), (2, 5), (2, 4), (96, 5), (520, 5), (24, 16)]
LRN_BETA_CASE = (11, 5, 0.6)
CROP_CASES = ("odd", "noadjust", "whole", "conv20")
FIT_CASES = ("landscape", "portrait", "same", "upscale", "one_wide", "rect_short")
U = 2.0 ** -24


# ---- restatements shared with test_gpu_lrn_crop.py ----
def lrn_ref(x, size, alpha, beta, kappa, ghost=True):
    """The closed form of DN/normalization_layer.c:66-95 in float64 over the last axis: norms[k] = kappa + alpha (W(k) - g), W(k) the sum of x[j]^2 over
    max(0, k - lo) <= j <= min(C - 1, k + h) with h = size / 2 and lo = (size - 1) / 2, g = x[h]^2 where h < C and 0 where h == C (the reference's running
    sum never adds channel h, and subtracts it once the window has passed it); out = x * norms^(-beta).  ghost=False: the textbook formula, g = 0.
    alpha, beta and kappa are the floats the layer holds.  -> out, float64 (NaN where norms is negative, as the reference's pow)"""
    x64 = np.asarray(x, dtype=np.float64)
    C = x64.shape[-1]; h, lo = size // 2, (size - 1) // 2
    sq = x64 * x64
    W = np.stack([sq[..., max(0, k - lo):min(C - 1, k + h) + 1].sum(axis=-1) for k in range(C)], axis=-1)
    g = sq[..., h:h + 1] if (ghost and h < C) else 0.0
    norms = np.float64(np.float32(kappa)) + np.float64(np.float32(alpha)) * (W - g)
    with np.errstate(invalid="ignore", divide="ignore"):
        return x64 * norms ** -np.float64(np.float32(beta))


def lrn_norms(x, size, alpha, kappa):
    """norms of lrn_ref and, per pixel, the largest sum of squares the reference's running sum ever holds or subtracts: the largest window's, or the
    never-added channel's (what its rounding is measured by)"""
    x64 = np.asarray(x, dtype=np.float64)
    C = x64.shape[-1]; h, lo = size // 2, (size - 1) // 2
    sq = x64 * x64
    W = np.stack([sq[..., max(0, k - lo):min(C - 1, k + h) + 1].sum(axis=-1) for k in range(C)], axis=-1)
    g = sq[..., h:h + 1] if h < C else np.zeros_like(sq[..., :1])
    return np.float64(np.float32(kappa)) + np.float64(np.float32(alpha)) * (W - g), np.maximum(W.max(axis=-1, keepdims=True), g)


def lrn_reference_bound(want, norms, peak, ch, alpha, beta, kappa):
    """How far the reference's own fp32 output may stand off from the float64 closed form `want`: its running sum rounds twice per channel (one term leaves,
    one enters), each time a value of magnitude at most kappa + alpha x `peak` (lrn_norms) -- 2 C half-ulps of that on norms, carried to the output
    through d(norms^-beta) / norms^-beta = beta d(norms) / norms --, then the square's, the pow's and the product's roundings: 8 half-ulps of the result."""
    return np.abs(want) * ((2 * ch + 4) * U * (kappa + alpha * peak) * beta / np.abs(norms) + 8 * U) + 1e-30


def lrn_case(g, ch, size, beta=0.75):
    """(x, y, alpha, beta, kappa) of one stand-alone case of lrn_crop_cases.npz"""
    tag = "lrn_%d_%d" % (ch, size) + ("" if beta == 0.75 else "_beta")
    return g[tag + "_x"], g[tag + "_y"], float(g["lrn_alpha"]), float(g[tag]) if beta != 0.75 else 0.75, float(g["lrn_kappa"])


def crop_ref(x, crop_h, crop_w, adjust=True):
    """DN/crop_layer.c:67-102 at inference on [..., H, W, C] float32: the centred window, times 2 plus -1 in float32 (two rounded operations)"""
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape[-3], x.shape[-2]
    dh, dw = (H - crop_h) // 2, (W - crop_w) // 2
    win = x[..., dh:dh + crop_h, dw:dw + crop_w, :]
    return win * np.float32(2) + np.float32(-1) if adjust else win.copy()


def resize_image_f32(im, w, h):
    """DN/image.c:1347-1389 resize_image on an [ih, iw, c] float32 image, operation for operation in float32: the horizontal pass, then the vertical one"""
    f = np.float32
    im = np.asarray(im, dtype=f); ih, iw = im.shape[:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        w_scale = f(iw - 1) / f(w - 1); h_scale = f(ih - 1) / f(h - 1)
    part = np.zeros((ih, w, im.shape[2]), f)
    for c in range(w):
        if c == w - 1 or iw == 1:
            part[:, c] = im[:, iw - 1]
        else:
            sx = f(c) * w_scale; ix = int(sx); dx = f(sx - f(ix))
            part[:, c] = (f(1) - dx) * im[:, ix] + dx * im[:, ix + 1]
    out = np.zeros((h, w, im.shape[2]), f)
    for r in range(h):
        if ih == 1:
            out[r] = part[0]          # (h_scale is 0: iy = 0, dy = 0)
            continue
        sy = f(r) * h_scale; iy = int(sy); dy = f(sy - f(iy))
        out[r] = (f(1) - dy) * part[iy]
        if r != h - 1:
            out[r] = out[r] + dy * part[iy + 1]
    return out


def center_crop_ref(img_u8, net_h, net_w):
    """darknet's classifier validation preprocessing (DN/examples/classifier.c:635-636) of a uint8 [h, w, 3] image: (float)p / 255. (a double division),
    resize_min(im, net_w) (DN/image.c:997-1011: integer divisions; no resize where the size does not change), crop_image from the centre with clamped
    coordinates (DN/image.c:857-875; C's division truncates toward zero) -> ([net_h, net_w, 3] float32, (resized h, resized w))"""
    im = (np.asarray(img_u8).astype(np.float64) / 255.).astype(np.float32)
    h, w = im.shape[:2]
    rh, rw = ((h * net_w) // w, net_w) if w < h else (net_w, (w * net_w) // h)
    resized = im if (rw == w and rh == h) else resize_image_f32(im, rw, rh)
    dx, dy = int((rw - net_w) / 2), int((rh - net_h) / 2)
    rows = np.clip(np.arange(net_h) + dy, 0, rh - 1); cols = np.clip(np.arange(net_w) + dx, 0, rw - 1)
    return resized[rows][:, cols], (rh, rw)


def _ok(cfg, dtype):
    rc, msg = hip.plan_check(cfg, dtype=dtype)
    assert rc == 0, msg


def _refused(cfg, *needles, dtype=hip.BF16):
    rc, msg = hip.plan_check(cfg, dtype=dtype)
    assert rc != 0, "planned: " + cfg
    for n in needles:
        assert n in msg, (n, msg)
    return msg


@pytest.fixture(scope="module")
def cases():
    return golden("lrn_crop_cases.npz")


NET = "[net]\nwidth=%d\nheight=%d\nchannels=3\n\n"
CONV = "[convolutional]\nfilters=%d\nsize=1\nstride=1\npad=1\nactivation=linear\n\n"
TAIL = "[convolutional]\nfilters=4\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n"


# ---- the planner ----
@pytest.mark.parametrize("dtype", [hip.FP32, hip.BF16, hip.FP16])
def test_fixture_cfgs_plan(cases, dtype):
    _ok(str(golden("mini_lrn.npz")["cfg"]), dtype)
    _ok(IO.cfg_text("alexnet-lrn"), dtype)
    for name in CROP_CASES:          # (a headless cfg plans as a map network)
        _ok(str(cases["crop_%s_cfg" % name]).replace("channels=3\n", "channels=3\nyolo_output=map\n"), dtype)
    for ch, size in LRN_CASES:
        _ok(NET % (7, 5) + CONV % ch + "[normalization]\nsize=%d\n\n" % size + TAIL, dtype)
    _ok(NET % (7, 5) + CONV % 12 + "[lrn]\n\n" + TAIL, dtype)          # the alias, every key at its default


def test_refusals_name_the_layer():
    lrn = NET % (7, 5) + CONV % 12 + "[normalization]\nsize=%d\n\n" + TAIL
    crop = NET % (14, 11) + CONV % 12 + "[crop]\ncrop_height=%d\ncrop_width=%d\n\n" + TAIL
    msgs = [_refused(lrn % 5, "layer 1: [normalization] is not served in the fp8 / split-fp16 configurations", dtype=hip.FP8),
            _refused(lrn % 5, "layer 1: [normalization] is not served in the fp8 / split-fp16 configurations", dtype=hip.FP16X2),
            _refused(crop % (8, 9), "layer 1: [crop] is not served in the fp8 / split-fp16 configurations", dtype=hip.FP8),
            _refused(crop % (8, 9), "layer 1: [crop] is not served in the fp8 / split-fp16 configurations", dtype=hip.FP16X2),
            _refused(NET % (7, 5) + "[crop]\ncrop_height=4\ncrop_width=4\n\n" + TAIL, "layer 0: [crop] is not served", dtype=hip.FP16X2),
            _refused(lrn % 0, "layer 1", "[normalization]", "size=0"),
            _refused(lrn % 18, "layer 1", "[normalization]", "size=18", "1..17"),
            _refused(NET % (7, 5) + CONV % 2 + "[normalization]\nsize=6\n\n" + TAIL, "layer 1", "[normalization]", "size=6 over 2 channels"),
            _refused(crop % (12, 9), "layer 1", "[crop]", "larger than its 14 x 11 input"),
            _refused(crop % (8, 15), "layer 1", "[crop]", "larger than its 14 x 11 input"),
            _refused(crop % (0, 9), "layer 1", "[crop]", "crop_height=0"),
            _refused(crop % (8, -1), "layer 1", "[crop]", "crop_width=-1")]
    assert len({m for m in msgs}) >= 9, msgs
    _ok(NET % (7, 5) + CONV % 2 + "[normalization]\nsize=5\n\n" + TAIL, hip.BF16)          # size / 2 == C is served
    _ok(lrn % 17, hip.BF16)
    with pytest.raises(hip.YoloError, match="1..17"):          # refused before a device is touched
        hip.op_lrn(np.zeros((1, 2, 2, 24), np.float32), size=18)
    with pytest.raises(hip.YoloError, match="channel count"):
        hip.op_lrn(np.zeros((1, 2, 2, 2), np.float32), size=6)
    with pytest.raises(hip.YoloError, match="dtype"):
        hip.op_lrn(np.zeros((1, 2, 2, 8), np.float32), dtype=hip.FP8)


def test_plan_of_a_leading_crop():
    """[crop] at layer 0: a layer of its own kind with a tensor of its own, no fused stem, the first conv on the tiled kernel over a 3-channel layer
    tensor (8 padded channels); the dump says where the window lies.  Folding a leading crop into the input staging is left undone."""
    rc, text = hip.plan_dump(IO.cfg_text("alexnet-lrn"), hip.BF16, 32, False)
    assert rc == 0, text
    lines = text.splitlines()
    assert lines[0].startswith("layer 0 crop type=19 H=227 W=227 C=3 in=[-1]") and " noop=0 " in lines[0]
    assert lines[1] == "crop 0 from=256x256 to=227x227 dh=14 dw=14 adjust=1"
    conv = lines[2]
    assert conv.startswith("layer 1 convolutional type=0 H=55 W=55 C=96 in=[0]") and " cin=3 cin_pad=8 " in conv and " kernel=0 fused=0 " in conv and " s2d7=0 " in conv
    lrn = [ln.split() for ln in lines if ln.startswith("lrn ")]
    assert [ln[:5] for ln in lrn] == [["lrn", "3", "size=5", "lo=2", "h=2"], ["lrn", "6", "size=5", "lo=2", "h=2"]] and all(ln[8] == "ghost=2" for ln in lrn)
    for ln in lrn:          # (%a of the floats the layer holds)
        assert [float.fromhex(f.split("=")[1]) for f in ln[5:8]] == [float(np.float32(1e-4)), 0.75, 2.0]
    assert sum(" normalization type=18 " in ln for ln in lines) == 2
    rc, table = hip.plan_table(IO.cfg_text("alexnet-lrn"), hip.BF16, 32, False)
    assert rc == 0 and table.splitlines()[0].startswith("0 crop kernel=- fused=none ") and table.splitlines()[3].startswith("3 normalization kernel=- ")


def test_lrn_and_crop_as_route_members():
    """their output as a member of a concatenation: at a whole-granule offset a window of the [route] buffer, else a copied source -- served either way"""
    for first, placed in ((16, True), (12, False)):
        for sec in ("[normalization]\nsize=3\n\n", "[crop]\ncrop_height=5\ncrop_width=7\nnoadjust=1\n\n"):
            cfg = NET % (7, 5) + CONV % first + CONV % 8 + sec + "[route]\nlayers=0,-1\n\n" + TAIL
            rc, text = hip.plan_dump(cfg, hip.BF16, 1, False)
            assert rc == 0, text
            lines = text.splitlines()
            member = [ln for ln in lines if ln.startswith("layer 2 ")][0]; route = [ln for ln in lines if ln.startswith("layer 3 ")][0]
            if placed:
                assert member.endswith(" ch_off=16") and " copy_inputs=[] " in route
            else:
                assert member.endswith(" ch_off=0") and " copy_inputs=[0,2] copy_offsets=[0,12] " in route


def test_layer_shapes_agree_with_the_fixtures(cases):
    g = golden("mini_lrn.npz")
    shapes = IO.layer_shapes(IO.parse_cfg(str(g["cfg"])))
    assert [s[0] for s in shapes] == ["crop", "convolutional", "normalization", "maxpool", "convolutional", "normalization", "convolutional", "avgpool", "softmax"]
    for i, s in enumerate(shapes):
        assert g["layer_%02d" % i].shape == (3,) + s[1:4], i
    assert shapes[0][1:] == (16, 21, 3, 3) and shapes[2][1:] == (16, 21, 13, 13) and shapes[5][1:] == (8, 10, 24, 24)
    for name in CROP_CASES:
        secs = IO.parse_cfg(str(cases["crop_%s_cfg" % name]))
        for i, s in enumerate(IO.layer_shapes(secs)):
            assert cases["crop_%s_layer_%02d" % (name, i)].shape == s[1:4]
        assert IO.weights_count(secs) == cases["crop_%s_weights" % name].size          # neither layer has weights: the stream walkers pass them by
    assert IO.weights_count(IO.parse_cfg(str(g["cfg"]))) == g["weights"].size
    assert IO.synth_weights(IO.parse_cfg(IO.cfg_text("alexnet-lrn")), seed=0).size == IO.weights_count(IO.parse_cfg(IO.cfg_text("alexnet")))


# ---- the restatements against the compiled reference ----
def test_lrn_closed_form_reproduces_the_reference(cases):
    """float64 closed form against the reference's fp32 running sum: within its rounding -- C adds of terms up to alpha x (the sum of all squares), carried
    through beta / norms, plus the pow and the product -- while the textbook formula (no never-added channel) misses by orders of magnitude more wherever
    that channel exists, and is the same thing where it does not (size / 2 == C)."""
    for ch, size, beta in [(c, s, 0.75) for c, s in LRN_CASES] + [LRN_BETA_CASE]:
        x, y, alpha, beta, kappa = lrn_case(cases, ch, size, beta)
        assert x.shape == (5, 7, ch) and y.shape == x.shape
        want = lrn_ref(x, size, alpha, beta, kappa); text = lrn_ref(x, size, alpha, beta, kappa, ghost=False)
        norms, peak = lrn_norms(x, size, alpha, kappa)
        bound = lrn_reference_bound(want, norms, peak, ch, alpha, beta, kappa)
        err = np.abs(y - want)
        print("lrn C %d size %d beta %g: closed form max err / bound %.3f, max rel err %.2e; textbook %.2e" % (ch, size, beta, float((err / bound).max()),
              float((err / np.abs(want).max()).max()), float(np.abs(y - text).max() / np.abs(want).max())))
        assert (err <= bound).all()
        if size // 2 < ch:
            assert np.abs(y - text).max() > 10 * bound.max() and np.abs(y - text).max() > 1e-3 * np.abs(want).max()
        else:
            assert np.array_equal(text, want)


def test_mini_lrn_layers_follow_the_restatements():
    g = golden("mini_lrn.npz")
    assert np.array_equal(g["layer_00"], crop_ref(g["images_u8"].astype(np.float32) / np.float32(255.0), 16, 21))
    for i, (size, alpha, kappa) in ((2, (5, 1e-4, 1.0)), (5, (4, 0.05, 1.5))):
        want = lrn_ref(g["layer_%02d" % (i - 1)], size, alpha, 0.75, kappa)
        assert np.abs(g["layer_%02d" % i] - want).max() < 1e-5 * np.abs(want).max()
    # the second one's never-added channel is far outside the 5e-4 of the fp32 network test
    text = lrn_ref(g["layer_04"], 4, 0.05, 0.75, 1.5, ghost=False)
    assert np.abs(g["layer_05"] - text).max() > 20 * 5e-4 * np.abs(g["layer_05"]).max()


def test_crop_restatement_is_exact(cases):
    for name in CROP_CASES:
        secs = IO.parse_cfg(str(cases["crop_%s_cfg" % name]))[1:]
        i = [s["type"] for s in secs].index("crop")
        src = cases["crop_%s_layer_%02d" % (name, i - 1)] if i else cases["crop_%s_image_u8" % name].astype(np.float32) / np.float32(255.0)
        want = crop_ref(src, int(secs[i]["crop_height"]), int(secs[i]["crop_width"]), not int(secs[i].get("noadjust", 0)))
        assert np.array_equal(cases["crop_%s_layer_%02d" % (name, i)], want), name
        assert (name == "conv20") == (i == 1) and (src.shape[-1] == 20) == (name == "conv20")
    assert np.array_equal(cases["crop_whole_layer_00"].shape, (11, 14, 3)) and cases["crop_odd_layer_00"].shape == (8, 9, 3)


def test_center_crop_restatement_is_exact(cases):
    seen = {}
    for name in FIT_CASES:
        img = cases["fit_%s_image_u8" % name]; nh, nw = (int(v) for v in cases["fit_%s_net_hw" % name])
        want, (rh, rw) = center_crop_ref(img, nh, nw)
        assert (rh, rw) == tuple(int(v) for v in cases["fit_%s_resized_hw" % name])
        assert want.shape == (nh, nw, 3) and np.array_equal(want, cases["fit_%s_input" % name]), name
        seen[name] = (img.shape[:2], (rh, rw), (nh, nw))
    assert seen["same"][0] == seen["same"][1]                                       # the no-resize branch
    assert min(seen["upscale"][0]) < 16 and seen["one_wide"][0][1] == 1
    assert seen["rect_short"][1][0] < seen["rect_short"][2][0]                      # resized lower than the network: a negative offset, replicated rows
    r = cases["fit_rect_short_input"]
    assert np.array_equal(r[0], r[4]) and np.array_equal(r[23], r[19]) and not np.array_equal(r[4], r[5])
    assert seen["landscape"][1][1] > 16 and seen["portrait"][1][0] > 16


# ---- the public surface ----
def test_symbols_and_constants():
    lib = hip.load_library()
    assert hip.FIT_CENTER_CROP == 4 and "yolo_op_lrn" in hip.EXPORTS and hasattr(lib, "yolo_op_lrn") and callable(hip.op_lrn)
    lib.yolo_fit_unit_value.restype = __import__("ctypes").c_float
    for p in (0, 1, 127, 200, 255):
        assert lib.yolo_fit_unit_value(4, p) == lib.yolo_fit_unit_value(hip.FIT_LETTERBOX, p) == np.float32(p / 255.)
    assert np.isnan(lib.yolo_fit_unit_value(5, 10)) and np.isnan(lib.yolo_fit_unit_value(9, 10))
    header = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    assert "YOLO_FIT_CENTER_CROP = 4" in header and "int yolo_op_lrn(" in header


def test_existing_plan_dumps_are_unchanged():
    """tests/test_plan_dump.py, unchanged, in a process of its own: every recorded plan dump is byte-identical"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", os.path.join(ROOT, "tests", "test_plan_dump.py"), "-k", "equal_the_recorded or covers_every"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-500:]


def test_shipped_alexnet_lrn_is_what_make_cfgs_writes(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_cfgs.py"), "--alexnet-lrn", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(str(tmp_path), "alexnet-lrn.cfg")).read()
    assert text == IO.cfg_text("alexnet-lrn")
    secs = IO.parse_cfg(text)
    assert (secs[0]["width"], secs[0]["height"]) == ("256", "256")
    assert [s["type"] for s in secs[1:8]] == ["crop", "convolutional", "maxpool", "normalization", "convolutional", "maxpool", "normalization"]
    assert (secs[1]["crop_height"], secs[1]["crop_width"]) == ("227", "227")
    assert all((s["size"], s["alpha"], s["beta"], s["kappa"]) == ("5", "0.0001", "0.75", "2") for s in secs[1:] if s["type"] == "normalization")
    plain = [s for s in IO.parse_cfg(IO.cfg_text("alexnet"))[1:]]
    assert [s for s in secs[1:] if s["type"] not in ("crop", "normalization")] == plain
