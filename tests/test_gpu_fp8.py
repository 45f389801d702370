"""BASELINE config 5 (fp8 filters and activations on the fp8 MFMA) against the oracle's emulation of the same
quantisation scheme (oracle/yolo_ref.py fp8_scheme_forward; DESIGN.md "fp8 scheme").

Tolerance: an e4m3 code is 4 significant bits, so the device and the emulation agree EXACTLY except where the fp32
accumulation order moves a value across a rounding boundary; on identical layer inputs (teacher forcing) at least
99.7 % of every layer's codes must be bit-identical and the rest at most one e4m3 step apart (|diff| <= 1/8 of the
value, 2^-9 * scale in the subnormal range; for a shortcut sum, one step of its larger operand, since the sum itself may
cancel to something much smaller, plus the re-rounding of the sum).

One documented exception (tools/probe/mfma_fp8.hip, DESIGN.md "fp8 scheme"): v_mfma_f32_16x16x128_f8f6f4 adds each group
of 8 consecutive-K products in a narrow datapath -- a product 2^14 or more below the largest of its group is dropped -- so
where a sum cancels against the bias to far less than its terms the device can land two or three steps away from the
fp32-accumulating emulation.  Allowed for at most 5e-4 of a layer's elements and never beyond 2^-10 of the layer's
largest magnitude."""
import numpy as np
import pytest
from oracle import yolo_ref as R
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu


def _codes_close(got, want, scale, what, min_same=0.997, operands=()):
    assert got.shape == want.shape, what
    same = float(np.mean(got == want))
    mag = np.maximum(np.abs(got), np.abs(want))
    omag = np.zeros_like(mag)
    for o in operands:
        omag = np.maximum(omag, np.abs(o))
    step = np.maximum((mag + omag) * 0.125, scale * 2.0 ** -9) * 1.0001     # operand flip + re-rounding of the sum
    far = np.abs(got - want) > step
    assert far.mean() <= 5e-4, "%s: %.5f of the elements more than one e4m3 step apart" % (what, far.mean())
    assert np.all(np.abs(got - want)[far] <= float(np.abs(want).max()) * 2.0 ** -10), "%s: cancellation outlier too large" % what
    allowed = max((1.0 - min_same) * got.size, 12.0)      # small tensors: a handful of boundary flips is not a rate
    assert float(np.sum(got != want)) <= allowed, "%s: only %.5f identical" % (what, same)
    return same


def _conv_ref(x, w, b, stride, residual, pad=None, leaky=True):
    """pad: zero padding each side (None: size / 2); leaky=False: a linear conv (test_gpu_tile_matrix.py: the cfg's padding= and activation)"""
    xq = R.to_fp8_e4m3(x)
    amax = np.abs(w).max(axis=(0, 1, 2)); osc = np.where(amax > 0, amax / np.float32(448), np.float32(1)).astype(np.float32)
    wq = R.to_fp8_e4m3(w / osc[None, None, None, :])
    v = (R.conv2d_nhwc(xq, wq, stride, pad).astype(np.float64) * osc + b.astype(np.float64)).astype(np.float32)
    q = R.to_fp8_e4m3(R.to_bf16(R.leaky_relu(v) if leaky else v))
    return (q, ()) if residual is None else (R.to_fp8_e4m3(q + R.to_fp8_e4m3(residual)), (q, residual))


@pytest.mark.parametrize("n,h,cin,cout,k,stride,res", [(2, 13, 64, 128, 3, 1, False), (2, 16, 128, 64, 1, 1, True), (1, 26, 32, 64, 3, 2, False),
                                                       (2, 13, 256, 512, 3, 1, True), (1, 13, 48, 255, 1, 1, False), (1, 7, 16, 40, 3, 1, True)])
def test_fp8_conv_operator(hiplib, n, h, cin, cout, k, stride, res):
    rng = np.random.default_rng(cin * 7 + cout)
    x = rng.normal(0, 1, (n, h, h, cin)).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    b = rng.normal(0, 0.1, cout).astype(np.float32)
    ho = (h + 2 * (k // 2) - k) // stride + 1
    r = rng.normal(0, 1, (n, ho, ho, cout)).astype(np.float32) if res else None
    want, operands = _conv_ref(x, w, b, stride, r)
    ran = []
    for cfg in [-1] + list(range(hiplib.op_conv_num_cfgs())):          # every id the operator accepts for e4m3 operands; it errors on the rest
        try:
            got = hiplib.op_conv2d(x, w, b, stride=stride, act=1, residual=r, dtype=hiplib.FP8, tile_cfg=cfg)
        except hiplib.YoloError:
            continue
        _codes_close(got, want, 1.0, "cfg %d" % cfg, operands=operands)
        ran.append(cfg)
    # csrc/conv_cfgs.h: CfgsFp8, every one of them; CfgsHaloFp8 (36..43) where the shape is 3x3 / stride 1 on whole 128-channel chunks over 13 x 13 blocks
    assert [c for c in ran if not 36 <= c <= 43] == [-1, 0, 2, 4, 6, 8, 12, 14, 16, 17, 19, 20, 23, 31, 32, 33, 34, 45, 48, 49, 51], ran
    assert [c for c in ran if 36 <= c <= 43] == (list(range(36, 44)) if (k, stride, h % 13, cin % 128) == (3, 1, 0, 0) else []), ran


def test_fp8_saturates_and_keeps_zero(hiplib):
    """|value| > 448 saturates to +-448 (no NaN / wrap), exact zeros stay zero, identity filter passes codes through."""
    x = np.zeros((1, 4, 4, 16), np.float32)
    x[0, 0, 0, :4] = [1000.0, -1000.0, 448.0, 0.0]
    x[0, 1, 1, :4] = [2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, -0.3]
    w = np.zeros((1, 1, 16, 16), np.float32); w[0, 0, np.arange(16), np.arange(16)] = 1.0
    got = hiplib.op_conv2d(x, w, None, act=0, dtype=hiplib.FP8)
    assert np.array_equal(got, R.to_fp8_e4m3(x))
    assert got[0, 0, 0, 0] == 448.0 and got[0, 0, 0, 1] == -448.0 and got[0, 1, 1, 1] == 0.0 and got[0, 1, 1, 2] == 2.0 ** -8


@pytest.mark.parametrize("cfg,size,sem", [("yolov3", 96, "tf"), ("yolov3", 96, "darknet"), ("yolov3-tiny", 96, "tf"), ("yolov2", 96, "tf"), ("yolov2", 96, "darknet")])
def test_fp8_network_layers_vs_emulation(hiplib, cfg, size, sem):
    txt = IO.with_input_size(IO.cfg_text(cfg), size)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=0)
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (2, size, size, 3), dtype=np.uint8)
    x01 = img.astype(np.float32) / np.float32(255)
    osecs = R.parse_cfg(txt); params = R.unflatten_weights(flat, osecs)
    _, outs32 = R.forward(osecs, params, x01, semantics=sem, collect=True)
    scales = R.fp8_calibrate_scales(osecs, outs32)
    assert len(set(scales.tolist())) > 1                   # the calibrated run exercises non-trivial scales
    semantics = hiplib.SEM_TF if sem == "tf" else hiplib.SEM_DARKNET
    for sc in (None, scales):
        eng = hiplib.Engine(txt, max_batch=2, dtype=hiplib.FP8, semantics=semantics, keep_layers=True)
        if sc is not None:
            eng.set_act_scales(sc)
        eng.set_weights(flat)
        det = eng.forward(img)
        dev = []
        for i, s in enumerate(osecs[1:]):
            multi_route = s["type"] == "route" and "," in s["layers"]
            dev.append(None if s["type"] in ("yolo", "region") or multi_route else eng.layer_output(i, 2))
        heads, outs = R.fp8_scheme_forward(osecs, params, x01, scales=sc, semantics=sem, teacher=dev)
        worst = 1.0
        for i, s in enumerate(osecs[1:]):
            if dev[i] is None:
                continue
            is_head = i + 1 < len(osecs) - 1 and osecs[i + 2]["type"] in ("yolo", "region")
            if is_head:
                np.testing.assert_allclose(dev[i], outs[i], rtol=2e-3, atol=2e-3 * float(np.abs(outs[i]).max()), err_msg="head conv %d" % i)
            else:
                a = 1.0 if sc is None else float(sc[i]) if s["type"] in ("convolutional", "shortcut") else 1.0
                ops = ()
                if s["type"] == "shortcut":
                    f = int(s["from"]); f = f if f >= 0 else i + f
                    ops = (dev[i - 1], dev[f])
                worst = min(worst, _codes_close(dev[i], outs[i], a, "%s layer %d (%s)" % (cfg, i, s["type"]), operands=ops))
        # the fused plan (shortcuts folded into conv epilogues, no per-layer storage) must give the same detections
        eng2 = hiplib.Engine(txt, max_batch=2, dtype=hiplib.FP8, semantics=semantics)
        if sc is not None:
            eng2.set_act_scales(sc)
        eng2.set_weights(flat)
        det2 = eng2.forward(img)
        assert np.array_equal(det, det2), "fused and unfused fp8 plans differ"
        eng.close(); eng2.close()


def test_fp8_tracks_full_precision(hiplib):
    """Free-running fp8 network vs the fp32 oracle: calibrated scales keep the decoded boxes close (e4m3 has 3
    mantissa bits, so this is a sanity bound, not a parity bound)."""
    size = 96
    txt = IO.with_input_size(IO.cfg_text("yolov3"), size)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=0)
    img = np.random.default_rng(3).integers(0, 256, (2, size, size, 3), dtype=np.uint8)
    x01 = img.astype(np.float32) / np.float32(255)
    osecs = R.parse_cfg(txt); params = R.unflatten_weights(flat, osecs)
    heads, outs32 = R.forward(osecs, params, x01, collect=True)
    ref = R.yolo_v3_detections(heads, size, ratio=True)
    eng = hiplib.Engine(txt, max_batch=2, dtype=hiplib.FP8)
    eng.set_act_scales(R.fp8_calibrate_scales(osecs, outs32))
    eng.set_weights(flat)
    det = eng.forward(img)
    err_xy = float(np.abs(det[..., :2] - ref[..., :2]).mean())
    assert err_xy < 0.02, err_xy                           # centres in image-ratio units
    rel = float(np.linalg.norm(det[..., 4:] - ref[..., 4:]) / np.linalg.norm(ref[..., 4:]))
    assert rel < 0.25, rel
    with pytest.raises(hiplib.YoloError):
        eng.set_act_scales(np.zeros(eng.num_layers, np.float32))
    with pytest.raises(hiplib.YoloError):
        eng.forward(img) if False else hiplib.Engine(txt, dtype=hiplib.BF16).set_act_scales(np.ones(eng.num_layers, np.float32))
    eng.close()


def test_mixed_e4m3_bf16_plan_vs_emulation(hiplib):
    """Mixed-precision plans (cfg key yolo_store=bf16 on [convolutional] sections of an fp8 network, darknet_io.with_layer_store): the
    13x13 stage and the FPN blocks keep bf16 tensors and run on the bf16 MFMA, the backbone up to 26x26 stays e4m3.  Every layer under
    teacher forcing against the oracle's emulation of the same plan: e4m3 layers to the code (as above), bf16 layers to a bf16 ulp;
    the closure rule (one storage type per residual stream / concatenation) is enforced by the library; fused == unfused."""
    size = 96
    txt0 = IO.with_input_size(IO.cfg_text("yolov3"), size)
    secs0 = IO.parse_cfg(txt0); flat = IO.synth_weights(secs0, seed=0)
    convs = [i for i, s in enumerate(secs0[1:]) if s["type"] == "convolutional"]
    heads_in = [i for i in convs if secs0[1:][i + 1]["type"] == "yolo"]
    want = [i for i in convs if i >= 62 and i not in heads_in]
    with pytest.raises(hiplib.YoloError, match="different types"):
        hiplib.Engine(IO.with_layer_store(txt0, want), max_batch=2, dtype=hiplib.FP8)          # route 86 would concatenate bf16 and e4m3
    with pytest.raises(hiplib.YoloError, match="fp8 networks"):
        hiplib.Engine(IO.with_layer_store(txt0, [5]), max_batch=2, dtype=hiplib.BF16)
    S = IO.store_closure(secs0, want)
    assert set(want) < set(S)
    txt = IO.with_layer_store(txt0, S)
    img = np.random.default_rng(2).integers(0, 256, (2, size, size, 3), dtype=np.uint8)
    x01 = img.astype(np.float32) / np.float32(255)
    osecs = R.parse_cfg(txt); params = R.unflatten_weights(flat, osecs)
    eng = hiplib.Engine(txt, max_batch=2, dtype=hiplib.FP8, keep_layers=True)
    eng.set_weights(flat)
    det = eng.forward(img)
    dev = []
    for i, s in enumerate(osecs[1:]):
        multi_route = s["type"] == "route" and "," in s["layers"]
        dev.append(None if s["type"] in ("yolo", "region") or multi_route else eng.layer_output(i, 2))
    heads, outs = R.fp8_scheme_forward(osecs, params, x01, teacher=dev)
    n16 = 0
    for i, s in enumerate(osecs[1:]):
        if dev[i] is None:
            continue
        is_head = i + 1 < len(osecs) - 1 and osecs[i + 2]["type"] in ("yolo", "region")
        if is_head:
            np.testing.assert_allclose(dev[i], outs[i], rtol=2e-3, atol=2e-3 * float(np.abs(outs[i]).max()), err_msg="head conv %d" % i)
        elif not _stored16(osecs, i):
            ops = ()
            if s["type"] == "shortcut":
                f = int(s["from"]); f = f if f >= 0 else i + f
                ops = (dev[i - 1], dev[f])
            _codes_close(dev[i], outs[i], 1.0, "mixed layer %d (%s)" % (i, s["type"]), operands=ops)
        else:
            n16 += 1
            err = np.abs(dev[i] - outs[i]); tol = 2.0 ** -7 * np.maximum(np.abs(outs[i]), np.abs(dev[i])) + 2e-3
            if s["type"] == "shortcut":
                f = int(s["from"]); f = f if f >= 0 else i + f
                tol = 2.0 ** -7 * (np.abs(dev[i - 1]) + np.abs(dev[f])) + 2e-3
            assert (err <= tol).all(), "bf16-stored layer %d (%s): max err %.3e" % (i, s["type"], err.max())
    assert n16 > 40
    eng.close()
    eng2 = hiplib.Engine(txt, max_batch=2, dtype=hiplib.FP8)
    eng2.set_weights(flat)
    assert np.array_equal(eng2.forward(img), det), "fused and unfused mixed plans differ"
    eng2.close()


def _stored16(osecs, i):
    """is layer i's tensor stored in bf16 under the plan in the cfg text (yolo_store keys + inheritance)?"""
    L = osecs[1:]
    t = L[i]["type"]
    if t == "convolutional":
        return L[i].get("yolo_store") == "bf16"
    if t in ("yolo", "region"):
        return False
    if t == "shortcut":
        return _stored16(osecs, i - 1)
    if t == "route":
        ls = [int(v) if int(v) >= 0 else i + int(v) for v in L[i]["layers"].split(",")]
        return _stored16(osecs, ls[0])
    return _stored16(osecs, i - 1)
