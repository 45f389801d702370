"""Recurrent networks on the device: the stacked gate GEMM (rnn_ops.hip) against float64 on pre-rounded operands, a whole network against
the reference's own C code over sequences of frames (tests/golden/mini_seq.npz, mini_crnn.npz: one live network, 5 frames), streams, what may and may
not move a state, the captured detect step, and the public surface.  The restatement lives in test_recurrent_host.py, where it is
checked against the reference's recorded layers."""
import os
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
import test_recurrent_host as RH

pytestmark = pytest.mark.gpu

T = 5
# test_gpu_unet.py's TOL16: what a 16-bit network's tensor may stand off from the fixture by, as a share of that tensor's largest value
TOL16 = {"bf16": 3e-2, "fp16": 4e-3}
# (a [connected] layer needs a producer of whole 8-channel granules: a small conv in front of it)
_NET = "[net]\nbatch=1\nwidth=4\nheight=4\nchannels=3\n\n[convolutional]\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"


def _dtypes(hiplib):
    return ((hiplib.FP32, "fp32", None), (hiplib.BF16, "bf16", RH.bf16), (hiplib.FP16, "fp16", RH.fp16))


def _engine(hiplib, cfg, flat, dtype, batch=1, keep=False):
    eng = hiplib.Engine(cfg, max_batch=batch, dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
    assert eng.weights_count() == flat.size
    eng.set_weights(flat)
    return eng


def _states(eng, streams):
    return [[eng.state(k, b).copy() for b in range(streams)] for k in range(eng.num_state_tensors)]


def _same_states(a, b):
    return all(np.array_equal(x, y) for ka, kb in zip(a, b) for x, y in zip(ka, kb))


# ---- 1: the gate GEMM, one recurrent layer per cfg ----
GATE_SHAPES = [(24, 16), (136, 40), (1024, 264)]          # (inputs, outputs): one K step; several, a ragged last one; many K steps over the four waves and a ragged last M tile
GATE_KINDS = [("lstm", ""), ("lstm", "batch_normalize=1\n"), ("gru", "tanh=1\n"), ("gru", "batch_normalize=1\n"), ("rnn", "activation=leaky\nshortcut=1\n"),
              ("rnn", "batch_normalize=1\n")]


def _gate_cfg(kind, keys, inputs, outputs):
    # the producer: a linear [connected] layer, whose stored output is the layer's x operand exactly; the layer's own output goes to a [softmax]
    # unrounded (fp32), as logits do
    return _NET + "[connected]\noutput=%d\nactivation=linear\n\n[%s]\noutput=%d\n%s\n[softmax]\n" % (inputs, kind, outputs, keys)


@pytest.mark.parametrize("shape", GATE_SHAPES, ids=["%dto%d" % s for s in GATE_SHAPES])
@pytest.mark.parametrize("kind,keys", GATE_KINDS, ids=["lstm", "lstm_bn", "gru_tanh", "gru_bn", "rnn_leaky_shortcut", "rnn_bn"])
def test_gate_gemm_against_float64(hiplib, kind, keys, shape):
    """streams 1, 3 and 32 of a 32-stream context, non-zero state through set_state, against float64 on operands pre-rounded to the storage
    type.  The bounds of test_gpu_unet.py::test_op_deconv2d: fp32 1e-4 of the tensor's scale; bf16 2^-7 |want| + 2e-3; fp16 2^-10 |want| +
    2e-3 -- on the layer's fp32 output and on every state it leaves (read back through get_state: an operand state is rounded once more)."""
    inputs, outputs = shape
    cfg = _gate_cfg(kind, keys, inputs, outputs)
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=inputs + outputs)
    rng = np.random.default_rng(outputs)
    imgs = rng.integers(0, 256, (32, 4, 4, 3), dtype=np.uint8)
    start = [rng.uniform(-0.9, 0.9, (32, outputs)).astype(np.float32) for _ in range(2 if kind == "lstm" else 1)]
    for dtype, name, store in _dtypes(hiplib):
        eng = _engine(hiplib, cfg, flat, dtype, batch=32, keep=True)
        assert eng.num_state_tensors == len(start) and eng.state_geometry(0) == (2, outputs)
        ref = RH.Net(cfg, flat, store)
        st = store or (lambda v: v)
        for n in (1, 3, 32):
            eng.reset_state()
            for k, s in enumerate(start):
                for b in range(32):
                    eng.set_state(k, b, s[b])
            eng.forward(imgs[:n], want_detections=False)
            x = eng.layer_output(1, n).astype(np.float64)
            got = eng.layer_output(2, n).reshape(n, outputs).astype(np.float64)
            want = np.zeros((n, outputs)); left = [np.zeros((n, outputs)) for _ in start]
            for b in range(n):
                h0 = start[0][b].astype(np.float64)
                ref.state[2] = (st(h0).astype(np.float64), start[1][b].astype(np.float64)) if kind == "lstm" else h0 if kind == "gru" else st(h0).astype(np.float64)
                want[b] = ref.layer(2, x[b]).reshape(-1)
                after = ref.state[2] if kind == "lstm" else (ref.state[2],)
                for k in range(len(start)):
                    left[k][b] = after[k]
            pairs = [("out", got, want)] + [("state %d" % k, np.stack([eng.state(k, b) for b in range(n)]).astype(np.float64), left[k]) for k in range(len(start))]
            for what, g, w in pairs:
                err = np.abs(g - w)
                if dtype == hiplib.FP32:
                    r = float(err.max() / np.abs(w).max())
                    print("%s %s %s n=%d %s: relmax %.3e" % (kind, keys.strip().replace("\n", ","), name, n, what, r))
                    assert r < 1e-4, (what, n)
                else:
                    bound = 2.0 ** (-7 if dtype == hiplib.BF16 else -10) * np.abs(w) + 2e-3
                    print("%s %s %s n=%d %s: max err / bound %.3f" % (kind, keys.strip().replace("\n", ","), name, n, what, float((err / bound).max())))
                    assert (err <= bound).all(), (what, n, float((err - bound).max()))
            # streams n .. 31 were not touched: every one of them
            for k, s in enumerate(start):
                for b in range(n, 32):
                    keep = s[b] if (dtype == hiplib.FP32 or kind == "gru" or k == 1) else st(s[b])
                    assert np.array_equal(eng.state(k, b), keep)
        eng.close()


# ---- 2, 3: the fixture, every layer at every step ----
@pytest.fixture(scope="module")
def seq():
    return golden("mini_seq.npz")


def test_mini_seq_matches_compiled_reference_fp32(hiplib, seq):
    """every layer at every one of the 5 steps, fp32 device path: 5e-4 of each tensor's scale (test_gpu_unet.py's bound); the production plan
    (pooled buffers) gives the same probabilities bit for bit"""
    cfg = str(seq["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    eng = _engine(hiplib, cfg, seq["weights"], hiplib.FP32, keep=True)
    prod = _engine(hiplib, cfg, seq["weights"], hiplib.FP32)
    assert eng.num_state_tensors == 8 and [eng.state_geometry(k)[0] for k in range(8)] == [4, 5, 6, 7, 8, 8, 9, 9]
    worst = 0.0
    for t in range(T):
        eng.forward(seq["images_u8"][t:t + 1], want_detections=False)
        for i, s in enumerate(secs):
            r = RH.standoff(eng.layer_output(i, 1), seq["layer_%02d" % i][t])
            worst = max(worst, r)
            assert r < 5e-4, "step %d layer %d (%s): %g" % (t, i, s["type"], r)
        assert np.array_equal(prod.classify(seq["images_u8"][t:t + 1], top_k=0)[0], eng.layer_output(len(secs) - 1, 1).reshape(-1))
    print("mini_seq fp32: worst stand-off %.3e" % worst)
    eng.close(); prod.close()


@pytest.fixture(scope="module")
def crnn():
    return golden("mini_crnn.npz")


def test_mini_crnn_matches_compiled_reference_fp32(hiplib, crnn):
    """every layer at every step under the same bound; per frame the decoded candidates above the fixture's threshold equal the reference's
    get_network_boxes of that frame, as test_gpu_network.py::test_mini_v3_boxes_match_darknet compares them (production plan)"""
    cfg = str(crnn["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    eng = _engine(hiplib, cfg, crnn["weights"], hiplib.FP32, keep=True)
    prod = _engine(hiplib, cfg, crnn["weights"], hiplib.FP32)
    assert eng.num_state_tensors == 2 and eng.state_geometry(0) == (3, 8 * 8 * 20) and eng.state_geometry(1) == (4, 8 * 8 * 16)
    worst = 0.0
    for t in range(T):
        eng.forward(crnn["images_u8"][t:t + 1], want_detections=False)
        for i in RH.compared_layers(cfg):
            got = eng.layer_output(i, 1); want = crnn["layer_%02d" % i][t]
            assert got.shape[1:] == want.shape
            r = RH.standoff(got, want)
            worst = max(worst, r)
            assert r < 5e-4, "step %d layer %d (%s): %g" % (t, i, secs[i]["type"], r)
        det = prod.forward(crnn["images_u8"][t:t + 1])[0]
        keep = det[:, 4] > float(crnn["thresh"])
        assert keep.sum() == len(crnn["boxes_%d" % t]) > 0
        np.testing.assert_allclose(det[keep, :4], crnn["boxes_%d" % t], rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(det[keep, 4], crnn["obj_%d" % t], rtol=2e-3, atol=2e-4)
    # the state is the map the reference's second step read: its own tensor order, 20 of 24 stored channels
    assert eng.state(0, 0).shape == (8 * 8 * 20,) and np.array_equal(eng.state(0, 0), prod.state(0, 0))
    print("mini_crnn fp32: worst stand-off %.3e" % worst)
    eng.close(); prod.close()


@pytest.mark.parametrize("act", ["logistic", "tanh"])
def test_crnn_with_an_activation_outside_the_conv_epilogue(hiplib, crnn, act):
    """the section's default activation (logistic) and tanh: every conv followed by k_activate and, where the layer sums, an add launch.
    Three streams over the 5 frames against the float64 restatement (which test_recurrent_host.py holds against the reference for the
    slope-family fixture): the fp32 network bound at every layer and step; bf16 under TOL16 at step 1"""
    cfg = str(crnn["cfg"]).replace("activation=leaky\nbatch_normalize=1\n\n[crnn]", "activation=%s\nbatch_normalize=1\n\n[crnn]" % act).replace("activation=relu\nshortcut=1", "shortcut=1")
    secs = IO.parse_cfg(cfg)[1:]
    assert [s.get("activation", "logistic") for s in secs if s["type"] == "crnn"] == [act, "logistic"]
    flat = crnn["weights"]; imgs = crnn["images_u8"]
    orders = ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 2, 0, 4, 1])
    want = [RH.run_frames(cfg, flat, imgs[o]) for o in orders]
    eng = _engine(hiplib, cfg, flat, hiplib.FP32, batch=3, keep=True)
    for t in range(T):
        eng.forward(np.stack([imgs[o[t]] for o in orders]), want_detections=False)
        for i in RH.compared_layers(cfg):
            got = eng.layer_output(i, 3)
            for b in range(3):
                assert RH.standoff(got[b], want[b][t][i]) < 5e-4, (t, i, b)
    eng.close()
    eng = _engine(hiplib, cfg, flat, hiplib.BF16, keep=True)
    eng.forward(imgs[:1], want_detections=False)
    for i in RH.compared_layers(cfg):
        assert RH.standoff(eng.layer_output(i, 1), want[0][0][i]) <= TOL16["bf16"], i
    eng.close()


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("fixture", ["mini_seq", "mini_crnn"])
def test_fixture_16bit_drift(hiplib, fixture, name):
    """step 1 under TOL16; steps 2..5: at most twice what the rounded host restatement stands off from the fixture at that step and layer
    (drift16_*: it rounds where the device rounds, but sums in another order), or TOL16 if that is larger"""
    seq = golden(fixture + ".npz")
    dtype = hiplib.BF16 if name == "bf16" else hiplib.FP16
    cfg = str(seq["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    eng = _engine(hiplib, cfg, seq["weights"], dtype, keep=True)
    drift = seq["drift16_" + name]
    for t in range(T):
        eng.forward(seq["images_u8"][t:t + 1], want_detections=False)
        for j, i in enumerate(RH.compared_layers(cfg)):
            r = RH.standoff(eng.layer_output(i, 1), seq["layer_%02d" % i][t])
            bound = TOL16[name] if t == 0 else max(2 * float(drift[t, j]), TOL16[name])
            print("%s %s step %d layer %d (%s): %.3e (restatement %.3e, bound %.3e)" % (fixture, name, t + 1, i, secs[i]["type"], r, float(drift[t, j]), bound))
            assert r <= bound, "step %d layer %d (%s)" % (t, i, secs[i]["type"])
    eng.close()


# ---- 4: streams ----
ORDERS = ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 2, 0, 4, 1])


def test_batch_index_is_the_stream(hiplib, seq):
    """batch 3 fed three different frame orders equals three batch-1 engines, each fed one of them (the fp32 bound)"""
    cfg = str(seq["cfg"]); imgs = seq["images_u8"]
    many = _engine(hiplib, cfg, seq["weights"], hiplib.FP32, batch=3)
    ones = [_engine(hiplib, cfg, seq["weights"], hiplib.FP32) for _ in ORDERS]
    for t in range(T):
        p3 = many.classify(np.stack([imgs[o[t]] for o in ORDERS]), top_k=0)
        for b, o in enumerate(ORDERS):
            p1 = ones[b].classify(imgs[o[t]:o[t] + 1], top_k=0)[0]
            assert RH.standoff(p3[b], p1) < 5e-4, (t, b)
    for k in range(many.num_state_tensors):
        for b in range(3):
            assert RH.standoff(many.state(k, b), ones[b].state(k, 0)) < 5e-4
    assert not np.array_equal(many.state(0, 0), many.state(0, 1))
    for e in [many] + ones:
        e.close()


def _step(eng, images):
    """one time step of streams 0 .. len(images) - 1 -> the network's output (a classifier's probabilities, a detector's decoded tensor)"""
    return eng.forward(images) if eng.rows else eng.classify(images, top_k=0)


@pytest.mark.parametrize("name", ["fp32", "bf16"])
@pytest.mark.parametrize("fixture", ["mini_seq", "mini_crnn"])
def test_streams_keep_reset_and_restore(hiplib, fixture, name):
    seq = golden(fixture + ".npz")
    dtype = hiplib.FP32 if name == "fp32" else hiplib.BF16
    cfg = str(seq["cfg"]); imgs = seq["images_u8"]
    eng = _engine(hiplib, cfg, seq["weights"], dtype, batch=3)
    assert all(not s.any() for k in _states(eng, 3) for s in k)          # zero at creation
    _step(eng, imgs[:3])
    before = _states(eng, 3)
    assert all(s.any() for k in before for s in k)
    # n = 2 on a 3-stream engine leaves stream 2 bit-identical
    _step(eng, imgs[3:5])
    after = _states(eng, 3)
    for k in range(len(before)):
        assert np.array_equal(after[k][2], before[k][2]) and not np.array_equal(after[k][0], before[k][0]) and not np.array_equal(after[k][1], before[k][1])
    # reset_state(1) zeroes stream 1 only
    eng.reset_state(1)
    z = _states(eng, 3)
    for k in range(len(z)):
        assert not z[k][1].any() and np.array_equal(z[k][0], after[k][0]) and np.array_equal(z[k][2], after[k][2])
    # get_state -> set_state on a fresh engine reproduces the next step bit for bit
    fresh = _engine(hiplib, cfg, seq["weights"], dtype, batch=3)
    for k in range(len(z)):
        for b in range(3):
            fresh.set_state(k, b, z[k][b])
    assert _same_states(_states(fresh, 3), z)
    nxt = np.stack([imgs[1], imgs[0], imgs[4]])
    assert np.array_equal(_step(eng, nxt), _step(fresh, nxt))
    assert _same_states(_states(eng, 3), _states(fresh, 3))
    eng.reset_state()
    assert all(not s.any() for k in _states(eng, 3) for s in k)
    with pytest.raises(hiplib.YoloError):
        eng.state(0, 3)
    with pytest.raises(hiplib.YoloError):
        eng.set_state(0, 0, np.zeros(7, np.float32))
    eng.close(); fresh.close()


# ---- 5: step accounting ----
def test_refused_calls_and_timing_passes_leave_the_states(hiplib, seq):
    cfg = str(seq["cfg"]); imgs = seq["images_u8"]
    eng = _engine(hiplib, cfg, seq["weights"], hiplib.BF16, batch=2)
    twin = _engine(hiplib, cfg, seq["weights"], hiplib.BF16, batch=2)
    eng.classify(imgs[:2], top_k=0); twin.classify(imgs[:2], top_k=0)
    s0 = _states(eng, 2)
    for bad in (lambda: eng.classify(imgs[:3], top_k=0),                      # a batch beyond max_batch
                lambda: eng.classify(imgs[:2], top_k=11),                     # top_k beyond the classes
                lambda: eng.detect_fused(imgs[:2]),                           # a classifier has no detections
                lambda: eng.forward(imgs[:2].astype(np.float64), want_detections=False, fmt=7)):
        with pytest.raises(hiplib.YoloError):
            bad()
        assert _same_states(_states(eng, 2), s0)
    eng.time_forward(2, 2); assert _same_states(_states(eng, 2), s0)
    eng.time_forward(1, 1, conv=False); assert _same_states(_states(eng, 2), s0)
    eng.time_layers(2, 2); assert _same_states(_states(eng, 2), s0)
    eng.autotune(2, iters=1); assert _same_states(_states(eng, 2), s0)
    # ... and the next step is the one a context that never ran them takes
    assert np.array_equal(eng.classify(imgs[2:4], top_k=0), twin.classify(imgs[2:4], top_k=0))
    assert _same_states(_states(eng, 2), _states(twin, 2))
    eng.close(); twin.close()


# a recurrent detector: YOLOv1's form ([connected] -> [detection]) with an [lstm] and a [gru] over the conv features
SEQ_DET = ("[net]\nbatch=1\nwidth=32\nheight=32\nchannels=3\n\n[convolutional]\nbatch_normalize=1\nfilters=8\nsize=3\nstride=2\npad=1\nactivation=leaky\n\n"
           "[maxpool]\nsize=2\nstride=2\n\n[lstm]\noutput=48\n\n[gru]\noutput=40\nbatch_normalize=1\n\n[connected]\noutput=36\nactivation=linear\n\n"
           "[detection]\nclasses=4\ncoords=4\nside=2\nnum=1\nsqrt=1\n")


def _detector(hiplib, which):
    if which == "mini_crnn":
        g = golden("mini_crnn.npz")
        return str(g["cfg"]), g["weights"], dict(score_thr=0.7, iou_thr=0.5, max_out=8, nms_mode=hiplib.NMS_TF)
    return SEQ_DET, IO.synth_weights(IO.parse_cfg(SEQ_DET), seed=17), dict(score_thr=0.05, iou_thr=0.5, max_out=8, nms_mode=hiplib.NMS_TF)


@pytest.mark.parametrize("which", ["mini_crnn", "lstm_gru_v1"])
def test_detect_graph_carries_the_state(hiplib, seq, which):
    """yolo_detect_graph over the 5 frames (eager, capture, three replays; the frames copied into one device buffer) equals five eager
    yolo_detect calls bit for bit: the records of every frame and the states at the end"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the GPU in this process")
    cfg, flat, kw = _detector(hiplib, which)
    imgs = seq["images_u8"]
    eager = _engine(hiplib, cfg, flat, hiplib.BF16, batch=2); graph = _engine(hiplib, cfg, flat, hiplib.BF16, batch=2)
    d_img = torch.zeros((2, 32, 32, 3), dtype=torch.uint8, device="cuda")
    boxes = torch.zeros((2, 8 * 6), dtype=torch.int32, device="cuda"); counts = torch.zeros((2,), dtype=torch.int32, device="cuda")
    seen = []
    for t in range(T):
        pair = np.stack([imgs[t], imgs[(t + 2) % T]])
        want = eager.detect_fused(pair, **kw)
        d_img.copy_(torch.from_numpy(pair)); torch.cuda.synchronize()
        graph.detect_graph(d_img, boxes, counts, **kw)
        graph.synchronize()
        got_counts = counts.cpu().numpy(); got = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(2, 8)
        for b in range(2):
            assert got_counts[b] == len(want[b]) and np.array_equal(got[b, :got_counts[b]], want[b]), "step %d stream %d" % (t, b)
        seen.append(np.concatenate([w["score"] for w in want]))
    assert sum(len(s) for s in seen) > 0 and _same_states(_states(eager, 2), _states(graph, 2))
    assert all(s.any() for k in _states(graph, 2) for s in k)
    eager.close(); graph.close()


def test_detect_images_graph_carries_the_state(hiplib, crnn):
    """the same for yolo_detect_images_graph on mini_crnn with frames of their own sizes (stretched to the network input on the device)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the GPU in this process")
    cfg, flat, kw = _detector(hiplib, "mini_crnn")
    rng = np.random.default_rng(23)
    frames = [[rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in pair] for pair in
              [((40, 52), (32, 32)), ((17, 90), (64, 48)), ((40, 52), (33, 31)), ((96, 96), (5, 7)), ((48, 20), (32, 32))]]
    eager = _engine(hiplib, cfg, flat, hiplib.BF16, batch=2); graph = _engine(hiplib, cfg, flat, hiplib.BF16, batch=2)
    packed = [hiplib.pack_images(f) for f in frames]
    dev = torch.zeros(max(p.size for p, _ in packed), dtype=torch.uint8, device="cuda")
    boxes = torch.zeros(2 * 8 * 6, dtype=torch.int32, device="cuda"); counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    total = 0
    for t in range(T):
        want = eager.detect_images(frames[t], fit=hiplib.FIT_STRETCH, **kw)
        pix, descs = packed[t]
        dev.zero_(); dev[:pix.size].copy_(torch.from_numpy(pix)); torch.cuda.synchronize()
        graph.detect_images_graph(dev, descs, boxes, counts, fit=hiplib.FIT_STRETCH, **kw)
        graph.synchronize()
        ct = counts.cpu().numpy(); got = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(2, 8)
        for b in range(2):
            assert ct[b] == len(want[b]) and np.array_equal(got[b, :ct[b]], want[b]), "step %d stream %d" % (t, b)
            total += len(want[b])
    assert total > 0 and _same_states(_states(eager, 2), _states(graph, 2))
    eager.close(); graph.close()


# ---- 6: surface ----
@pytest.mark.parametrize("fixture", ["mini_seq", "mini_crnn"])
def test_export_and_reload_from_zero_state(hiplib, fixture, tmp_path):
    seq = golden(fixture + ".npz")
    cfg = str(seq["cfg"]); imgs = seq["images_u8"]
    eng = _engine(hiplib, cfg, seq["weights"], hiplib.BF16)
    first = [_step(eng, imgs[t:t + 1]) for t in range(3)]
    path = os.path.join(str(tmp_path), "seq.yolohip")
    eng.export(path)                                   # (after three steps: the state is no part of the artifact)
    back = hiplib.Engine.from_file(path)
    assert back.num_state_tensors == eng.num_state_tensors and all(not s.any() for k in _states(back, 1) for s in k)
    for t in range(3):
        assert np.array_equal(_step(back, imgs[t:t + 1]), first[t])
    eng.close(); back.close()


def test_veneer_network_predict_carries_and_resets_the_state(hiplib, seq, tmp_path, monkeypatch):
    """the darknet veneer: network_predict over 3 frames equals the reference's recorded probabilities (the fp32 bound); reset_network_state
    (and reset_rnn) start the sequence again"""
    import ctypes as C
    from yolo_tensorflow_amd import darknet_hip as DH
    monkeypatch.setenv("DARKNET_HIP_DTYPE", "fp32")
    cfg = str(tmp_path / "net.cfg"); wf = str(tmp_path / "net.weights")
    open(cfg, "w").write(str(seq["cfg"])); IO.write_weights_file(wf, seq["weights"], 0, 2)
    x = [np.ascontiguousarray((seq["images_u8"][t].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)) for t in range(3)]
    lib = DH._load(); net = DH.load_net(cfg, wf)
    predict = lambda t: np.ctypeslib.as_array(lib.network_predict(net, x[t].ctypes.data_as(C.POINTER(C.c_float))), shape=(10,)).copy()
    try:
        first = [predict(t) for t in range(3)]
        lib.reset_network_state(net, 0)
        again = [predict(t) for t in range(2)]
        lib.reset_rnn(net)
        third = predict(0)
        unreset = predict(0)
    finally:
        DH.free_net(net)
    for t in range(3):
        assert RH.standoff(first[t], seq["layer_11"][t]) < 5e-4
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]) and np.array_equal(third, first[0])
    assert not np.array_equal(unreset, first[0])


def test_classifier_follows_the_sequence(hiplib, seq):
    from yolo_tensorflow_amd.classifier import Classifier
    clf = Classifier(str(seq["cfg"]), dtype=hiplib.FP32)
    clf.engine.set_weights(seq["weights"])
    tops = [clf.classify_from_image(seq["images_u8"][t], top=1)[0][0] for t in range(T)]
    assert tops == seq["top"].tolist() and len(set(tops)) > 1
    clf.close()


def test_batch_normalised_connected_against_float64(hiplib):
    """[connected] batch_normalize=1, alone: the fold of its rolling statistics into rows and bias"""
    cfg = _NET + "[connected]\noutput=24\nbatch_normalize=1\nactivation=leaky\n\n[connected]\noutput=6\nbatch_normalize=1\nactivation=linear\n\n[softmax]\n"
    flat = IO.synth_weights(IO.parse_cfg(cfg), seed=3)
    imgs = np.random.default_rng(4).integers(0, 256, (3, 4, 4, 3), dtype=np.uint8)
    eng = _engine(hiplib, cfg, flat, hiplib.FP32, batch=3, keep=True)
    eng.forward(imgs, want_detections=False)
    for b in range(3):
        outs = RH.Net(cfg, flat).step(imgs[b].astype(np.float32) / np.float32(255.0))
        for i in range(4):
            assert RH.standoff(eng.layer_output(i, 3)[b], outs[i]) < 1e-4
    eng.close()
