"""Vector-input networks on the device: the sampler against its numpy restatement, exactly; tests/golden/mini_char_rnn.npz -- the
compiled reference driven as examples/rnn.c test_char_rnn drives it -- step by step and in one yolo_sequence call; 16-bit drift; streams; split
and refused calls; forward_vectors; temperature and entry-point routing.  The restatements live in test_char_rnn_host.py, where they are
checked against the reference's recorded layers and tokens."""
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
import test_recurrent_host as RH
import test_char_rnn_host as CH

pytestmark = pytest.mark.gpu

STEPS, SEED_LEN, SAMPLED, N = CH.STEPS, CH.SEED_LEN, CH.SAMPLED, 37
TOL16 = {"bf16": 3e-2, "fp16": 4e-3}          # test_gpu_recurrent.py's
PROBS = 4                                      # the [softmax] layer


@pytest.fixture(scope="module")
def fx():
    return golden(CH.FIXTURE)


def _engine(hiplib, cfg, flat, dtype, batch=1, keep=False):
    eng = hiplib.Engine(cfg, max_batch=batch, dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
    assert eng.weights_count() == flat.size
    eng.set_weights(flat)
    return eng


def _states(eng, streams):
    return [[eng.state(k, b).copy() for b in range(streams)] for k in range(eng.num_state_tensors)]


def _same_states(a, b):
    return all(np.array_equal(x, y) for ka, kb in zip(a, b) for x, y in zip(ka, kb))


def _forced(eng, fed):
    """teacher forcing: one call, every step's probabilities [steps, N] of stream 0"""
    fed = np.asarray(fed, dtype=np.int32)
    toks, probs = eng.sequence(fed, fed.size, want_probs=True)
    assert toks is None
    return probs[:, 0, :]


# ---- 1: the sampler ----
def _rows(rng, n, ln):
    x = rng.normal(0, 4.0, (n, ln))
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("ln", [1, 37, 256, 8192])
def test_op_sample_equals_the_numpy_sampler(hiplib, ln):
    """n = 3 rows of softmax outputs (many below the clip at the longer lengths) under u = 0, u = 0.99999994 (the largest float below 1: the
    walk runs to the end, or to the n - 1 exit) and a u inside; a row the clip leaves one class of; a row it leaves nothing of (NaN, n - 1)"""
    rng = np.random.default_rng(ln)
    probs = _rows(rng, 3, ln)
    for u in (np.array([0.0, 0.99999994, 0.5], dtype=np.float32), rng.uniform(0, 1, 3).astype(np.float32), np.full(3, 0.99999994, dtype=np.float32)):
        got = hiplib.op_sample(probs, u, clip=CH.CLIP)
        want = [CH.sample_np(probs[b], u[b]) for b in range(3)]
        assert got.tolist() == want, (ln, u, got, want)
    single = np.full((3, ln), 2e-5, dtype=np.float32); single[:, ln // 2] = 1 - 2e-5 * (ln - 1)
    none = np.full((3, ln), 1e-5, dtype=np.float32)
    for rows in (single, none):
        u = np.array([0.0, 0.3, 0.99999994], dtype=np.float32)
        got = hiplib.op_sample(rows, u, clip=CH.CLIP)
        want = [CH.sample_np(rows[b], u[b]) for b in range(3)]
        assert got.tolist() == want, (ln, got, want)
    assert hiplib.op_sample(none, np.full(3, 0.3, dtype=np.float32), clip=CH.CLIP).tolist() == [ln - 1] * 3
    if ln > 1:
        assert hiplib.op_sample(single, np.full(3, 0.3, dtype=np.float32), clip=CH.CLIP).tolist() == [ln // 2] * 3


def test_op_sample_refuses_a_row_the_kernel_cannot_stage(hiplib):
    with pytest.raises(hiplib.YoloError, match="8192"):
        hiplib.op_sample(np.full((1, 8193), 1.0 / 8193, dtype=np.float32), np.zeros(1, dtype=np.float32))


# ---- 2, 3: fp32 against the fixture ----
@pytest.fixture(scope="module")
def stepwise32(hiplib, fx):
    """fp32, one step per call: every layer of every step, and the probabilities each call returned"""
    cfg = str(fx["cfg"])
    eng = _engine(hiplib, cfg, fx["weights"], hiplib.FP32, keep=True)
    assert eng.vector_inputs == N and eng.input_hw == (1, 1) and eng.num_state_tensors == 4
    layers, probs = [], []
    for t in range(STEPS):
        _, p = eng.sequence(fx["fed"][t:t + 1], 1, want_probs=True)
        probs.append(p[0, 0])
        layers.append([eng.layer_output(i, 1).reshape(-1) for i in CH.compared_layers(cfg)])
    eng.close()
    return layers, np.stack(probs)


def test_fp32_step_by_step_matches_the_reference_at_every_layer(fx, stepwise32):
    layers, probs = stepwise32
    worst = 0.0
    for t in range(STEPS):
        for i in CH.compared_layers(str(fx["cfg"])):
            r = RH.standoff(layers[t][i], fx["layer_%02d" % i][t])
            worst = max(worst, r)
            assert r < 5e-4, "step %d layer %d: %g" % (t, i, r)
        assert np.array_equal(probs[t], layers[t][PROBS])
    print("mini_char_rnn fp32: worst stand-off %.3e" % worst)


def _running_sums(p):
    a = np.array(p, dtype=np.float64); a[np.asarray(p, dtype=np.float32) < CH.CLIP] = 0
    return np.cumsum(a / a.sum())


def test_fp32_one_call_for_all_steps(hiplib, fx, stepwise32):
    """teacher-forced along the recorded tokens: bit-identical to the step-by-step run; the running sums the sampler walks stand within half the
    fixture's margin of the reference's, so the free-running call must draw the reference's tokens -- and does"""
    eng = _engine(hiplib, str(fx["cfg"]), fx["weights"], hiplib.FP32)
    probs = _forced(eng, fx["fed"])
    assert np.array_equal(probs, stepwise32[1])
    for k in range(SAMPLED):
        t = SEED_LEN - 1 + k
        d = float(np.abs(_running_sums(probs[t]) - _running_sums(fx["layer_04"][t].reshape(-1))).max())
        print("step %d: running sums differ by %.2e, margin %.2e" % (t, d, fx["margin"][k]))
        assert d < fx["margin"][k] / 2
    eng.reset_state()
    toks, free = eng.sequence(fx["seed_tokens"], STEPS, uniforms=fx["uniforms"], clip=CH.CLIP, want_probs=True)
    assert toks.shape == (SAMPLED, 1) and toks[:, 0].tolist() == fx["tokens"].tolist()
    assert np.array_equal(free[:, 0, :], probs)
    eng.close()


# ---- 4, 5: 16 bit ----
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_16_bit_teacher_forced_drift(hiplib, fx, name):
    """the probabilities along the recorded tokens: TOL16 at the first step, max(2 x the fixture's recorded drift, TOL16) after
    (test_gpu_recurrent.py::test_fixture_16bit_drift's rule)"""
    eng = _engine(hiplib, str(fx["cfg"]), fx["weights"], getattr(hiplib, name.upper()))
    probs = _forced(eng, fx["fed"])
    for t in range(STEPS):
        r = RH.standoff(probs[t], fx["layer_04"][t])
        bound = TOL16[name] if t == 0 else max(2 * float(fx["drift16_" + name][t][PROBS]), TOL16[name])
        print("%s step %d: %.3e (bound %.3e)" % (name, t, r, bound))
        assert r < bound, (t, r, bound)
    eng.close()


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_16_bit_free_running_is_self_consistent(hiplib, fx, name):
    """every token is the numpy sampler's over the device's own row and uniform; forcing the device's own tokens reproduces its probabilities"""
    eng = _engine(hiplib, str(fx["cfg"]), fx["weights"], getattr(hiplib, name.upper()))
    toks, probs = eng.sequence(fx["seed_tokens"], STEPS, uniforms=fx["uniforms"], clip=CH.CLIP, want_probs=True)
    for k in range(SAMPLED):
        assert int(toks[k, 0]) == CH.sample_np(probs[SEED_LEN - 1 + k, 0], fx["uniforms"][k]), k
    eng.reset_state()
    again = _forced(eng, np.concatenate([fx["seed_tokens"], toks[:-1, 0]]))
    assert np.array_equal(again, probs[:, 0, :])
    eng.close()


# ---- 6: streams ----
def test_streams_are_independent(hiplib, fx):
    cfg = str(fx["cfg"])
    orders = np.stack([fx["fed"], fx["fed"][::-1], np.roll(fx["fed"], 3)], axis=1).astype(np.int32)          # [steps, 3]
    eng3 = _engine(hiplib, cfg, fx["weights"], hiplib.FP32, batch=3)
    _, p3 = eng3.sequence(orders, STEPS, want_probs=True)
    eng1 = _engine(hiplib, cfg, fx["weights"], hiplib.FP32)
    for b in range(3):
        eng1.reset_state()
        p1 = _forced(eng1, orders[:, b])
        for t in range(STEPS):
            assert RH.standoff(p3[t, b], p1[t]) < 5e-4, (b, t)
    before = _states(eng3, 3)
    eng3.sequence(orders[:4, :2], 4)
    after = _states(eng3, 3)
    for k in range(eng3.num_state_tensors):
        assert np.array_equal(before[k][2], after[k][2]) and not np.array_equal(before[k][0], after[k][0])
    eng1.close(); eng3.close()


# ---- 7: split and refused calls ----
@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_split_calls_and_refused_calls(hiplib, fx, name):
    eng = _engine(hiplib, str(fx["cfg"]), fx["weights"], getattr(hiplib, name.upper()), batch=2)
    seed = np.stack([fx["seed_tokens"], fx["seed_tokens"][::-1]], axis=1).astype(np.int32)          # [4, 2]
    u = np.random.default_rng(5).uniform(0, 1, (9, 2)).astype(np.float32)
    whole_t, whole_p = eng.sequence(seed, 12, uniforms=u, clip=CH.CLIP, want_probs=True)
    eng.reset_state()
    t5, p5 = eng.sequence(seed, 5, uniforms=u[:2], clip=CH.CLIP, want_probs=True)
    t7, p7 = eng.sequence(t5[-1:], 7, uniforms=u[2:], clip=CH.CLIP, want_probs=True)
    assert t5.shape == (2, 2) and t7.shape == (7, 2)
    assert np.array_equal(np.concatenate([t5, t7]), whole_t) and np.array_equal(np.concatenate([p5, p7]), whole_p)
    eng.reset_state()
    again_t, again_p = eng.sequence(seed, 12, uniforms=u, clip=CH.CLIP, want_probs=True)
    assert np.array_equal(again_t, whole_t) and np.array_equal(again_p, whole_p)
    before = _states(eng, 2)
    bad = seed.copy(); bad[2, 1] = N
    for kw, word in ((dict(tokens=bad, steps=12, uniforms=u), "token %d" % N), (dict(tokens=seed, steps=3), "forced = 4"),
                     (dict(tokens=seed, steps=12), "uniforms == NULL"), (dict(tokens=np.zeros((4, 3), dtype=np.int32), steps=4), "streams")):
        with pytest.raises(hiplib.YoloError, match=word):
            eng.sequence(**kw)
        assert _same_states(before, _states(eng, 2)), word
    eng.close()


def test_device_buffers_stay_on_the_device(hiplib, fx):
    """loc = device: tokens, uniforms, sampled tokens and probabilities are read and written in place; the same values as through the host"""
    import torch
    eng = _engine(hiplib, str(fx["cfg"]), fx["weights"], hiplib.BF16)
    want_t, want_p = eng.sequence(fx["seed_tokens"], STEPS, uniforms=fx["uniforms"], clip=CH.CLIP, want_probs=True)
    eng.reset_state()
    tok = torch.from_numpy(fx["seed_tokens"].astype(np.int32)).cuda(); uni = torch.from_numpy(fx["uniforms"]).cuda()
    out = torch.full((SAMPLED,), -1, dtype=torch.int32, device="cuda"); probs = torch.zeros((STEPS, 1, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = eng.lib.yolo_sequence(eng.ctx, 1, STEPS, tok.data_ptr(), SEED_LEN, uni.data_ptr(), float(CH.CLIP), out.data_ptr(), probs.data_ptr(), hiplib.DEVICE)
    assert rc == 0, eng.lib.yolo_last_error(eng.ctx).decode()
    eng.synchronize()
    assert np.array_equal(out.cpu().numpy(), want_t[:, 0]) and np.array_equal(probs.cpu().numpy(), want_p)
    eng.close()


# ---- 8: forward_vectors ----
_DENSE = "[net]\ninputs=37\nyolo_input=vector\n\n[connected]\noutput=20\nactivation=leaky\n\n[connected]\noutput=5\nactivation=linear\n\n[softmax]\n"


def test_forward_vectors_against_float64(hiplib):
    """an input that is no one-hot row, batch 2, through two [connected] layers whose widths (37, 20) are no multiples of 8, against float64 on
    operands pre-rounded to the storage type: 5e-4 of the tensor's scale in fp32, TOL16 in 16 bit"""
    secs = IO.parse_cfg(_DENSE)
    flat = IO.synth_weights(secs, seed=3)
    x = np.random.default_rng(4).normal(0, 1, (2, N)).astype(np.float32)
    for dtype, name, store in ((hiplib.FP32, "fp32", None), (hiplib.BF16, "bf16", RH.bf16), (hiplib.FP16, "fp16", RH.fp16)):
        eng = _engine(hiplib, _DENSE, flat, dtype, batch=2, keep=True)
        got = eng.forward_vectors(x)
        assert got.shape == (2, 5)
        for b in range(2):
            want = CH.CharNet(_DENSE, flat, store).step(x[b])
            for i in range(3):
                r = RH.standoff(eng.layer_output(i, 2)[b], want[i])
                print("forward_vectors %s stream %d layer %d: %.3e" % (name, b, i, r))
                assert r < (5e-4 if store is None else TOL16[name]), (name, b, i, r)
            assert np.array_equal(got[b], eng.layer_output(2, 2)[b].reshape(-1))
        eng.close()


# ---- 9: temperature and routing ----
def test_set_temperature_equals_the_cfg_key(hiplib, fx):
    cfg = str(fx["cfg"])
    a = _engine(hiplib, cfg, fx["weights"], hiplib.BF16)
    b = _engine(hiplib, cfg.replace("temperature=0.7", "temperature=0.5"), fx["weights"], hiplib.BF16)
    base = _forced(a, fx["fed"])
    a.reset_state(); a.set_temperature(0.5)
    pa, pb = _forced(a, fx["fed"]), _forced(b, fx["fed"])
    assert np.array_equal(pa, pb) and not np.array_equal(pa, base)
    with pytest.raises(hiplib.YoloError, match="> 0"):
        a.set_temperature(0.0)
    a.close(); b.close()


def test_entry_points_refuse_the_other_kind_of_network_by_name(hiplib, fx):
    vec = _engine(hiplib, str(fx["cfg"]), fx["weights"], hiplib.BF16)
    img = np.zeros((1, 1, 1, 3), dtype=np.uint8)
    for call in (lambda: vec.forward(img), lambda: vec.detect(img), lambda: vec.classify(img, top_k=1), lambda: vec.forward_images([img[0]]),
                 lambda: vec.detect_images([img[0]]), lambda: vec.classify_images([img[0]], top_k=1), lambda: vec.detect_tiled([img[0]]),
                 lambda: vec.segment_images([img[0]]), lambda: vec.forward_image(img[0])):
        with pytest.raises(hiplib.YoloError, match="vector-input network.*yolo_forward_vectors / yolo_sequence"):
            call()
    with pytest.raises(hiplib.YoloError, match="not built"):
        vec.export("/dev/null")
    vec.close()
    g = golden("mini_v3.npz")
    det = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.BF16)
    det.set_weights(g["weights"])
    assert det.vector_inputs == 0
    for call in (lambda: det.lib.yolo_forward_vectors(det.ctx, np.zeros(8, dtype=np.float32).ctypes.data, 1, hiplib.HOST, None, 0),
                 lambda: det.lib.yolo_sequence(det.ctx, 1, 1, np.zeros(1, dtype=np.int32).ctypes.data, 1, None, 1e-4, None, None, hiplib.HOST)):
        assert call() != 0
        msg = det.lib.yolo_last_error(det.ctx).decode()
        assert "reads images" in msg and "yolo_forward*" in msg and "yolo_input=vector" in msg, msg
    det.close()


def test_veneer_network_predict_is_one_step(hiplib, fx, tmp_path, monkeypatch):
    """libdarknet_hip.so: load_network of darknet's own cfg (inputs= and no image size: the veneer adds the key), network_predict over one-hot
    rows equals Engine.sequence step by step, bit for bit; reset_rnn starts again"""
    import ctypes as C
    from yolo_tensorflow_amd import darknet_hip as DH
    monkeypatch.setenv("DARKNET_HIP_DTYPE", "fp32")
    cfg = str(tmp_path / "net.cfg"); wf = str(tmp_path / "net.weights")
    open(cfg, "w").write(str(fx["cfg"]).replace("yolo_input=vector\n", "")); IO.write_weights_file(wf, fx["weights"], 0, 2)
    eng = hiplib.Engine(str(fx["cfg"]), max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(fx["weights"])
    want = _forced(eng, fx["fed"][:5])
    eng.close()
    lib = DH._load(); net = DH.load_net(cfg, wf)
    assert net
    x = [CH.one_hot(t, N) for t in fx["fed"][:5]]
    predict = lambda t: np.ctypeslib.as_array(lib.network_predict(net, x[t].ctypes.data_as(C.POINTER(C.c_float))), shape=(N,)).copy()
    try:
        first = [predict(t) for t in range(5)]
        lib.reset_rnn(net)
        again = predict(0)
    finally:
        DH.free_net(net)
    assert np.array_equal(np.stack(first), want) and np.array_equal(again, first[0])
    for t in range(5):
        assert RH.standoff(first[t], fx["layer_04"][t]) < 5e-4


def test_char_rnn_generates_and_scores(hiplib, fx):
    """CharRNN over the fixture: generate() is test_char_rnn -- the reference's tokens in fp32 -- and score() is valid_char_rnn's sum over the
    teacher-forced probabilities"""
    from yolo_tensorflow_amd.char_rnn import CharRNN
    plain = str(fx["cfg"]).replace("yolo_input=vector\n", "")
    net = CharRNN(plain, fx["weights"], dtype=hiplib.FP32)
    assert net.inputs == N
    out = net.generate(fx["seed_tokens"], SAMPLED, temp=0.7, rseed=int(fx["rseed"]))
    assert out.tolist() == fx["seed_tokens"].tolist() + fx["tokens"].tolist()
    text = np.concatenate([fx["seed_tokens"], fx["tokens"]])
    s = net.score(text)
    want = -np.mean([np.log2(float(fx["layer_04"][t].reshape(-1)[text[t + 1]])) for t in range(STEPS)])
    assert s["count"] == STEPS and abs(s["bpc"] - want) < 1e-3 * want, (s, want)
    net.close()


def _small_variance_weights(fx, k=0.03):
    """the fixture's stream with the batch-normalised [rnn] layer's rows and rolling means times k and its rolling variances times k^2 (4e-4 ..
    9e-4, the range of a trained file's): the same network up to the epsilon of the fold, which now matters -- gamma / (sqrt(var) + 1e-6), CPU
    darknet's, and gamma / sqrt(var + 1e-5) differ by about 1 %"""
    flat = fx["weights"].copy(); pos = 0
    for inputs in (N, 24, 24):          # input, self, output: biases, rows, scales, rolling mean, rolling variance
        rows = slice(pos + 24, pos + 24 + 24 * inputs); mean = slice(rows.stop + 24, rows.stop + 48); var = slice(rows.stop + 48, rows.stop + 72)
        flat[rows] *= np.float32(k); flat[mean] *= np.float32(k); flat[var] *= np.float32(k * k)
        pos = var.stop
    assert pos == IO.recurrent_specs(IO.parse_cfg(str(fx["cfg"])))[0]["outputs"] * (3 * 4 + N + 24 + 24) and flat[var].max() < 1e-3
    return flat


def test_char_rnn_is_darknets_arithmetic_and_keeps_the_cfg_temperature_for_scoring(hiplib, fx):
    """on weights whose rolling variances are small, where the two batch-norm folds part: CharRNN's engine equals an engine with darknet
    semantics bit for bit and differs from one with TF semantics; score() after a generate() at another temperature runs at the cfg's own"""
    from yolo_tensorflow_amd.char_rnn import CharRNN
    flat = _small_variance_weights(fx)
    cfg = str(fx["cfg"]).replace("temperature=0.7", "temperature=0.9")
    net = CharRNN(cfg.replace("yolo_input=vector\n", ""), flat, dtype=hiplib.FP32)
    dn = _engine(hiplib, cfg, flat, hiplib.FP32)
    tf = hiplib.Engine(cfg, max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_TF); tf.set_weights(flat)
    text = np.concatenate([fx["seed_tokens"], fx["tokens"]])
    own, want, other = _forced(net.engine, text[:-1]), _forced(dn, text[:-1]), _forced(tf, text[:-1])
    gap = max(RH.standoff(other[t], want[t]) for t in range(STEPS))
    print("darknet against TF fold on these weights: %.3e" % gap)
    assert np.array_equal(own, want) and gap > 1e-4
    # generate at 0.7, then score: the cfg's 0.9
    dn.reset_state(); dn.set_temperature(0.7)
    toks = dn.sequence(fx["seed_tokens"], STEPS, uniforms=fx["uniforms"], clip=CH.CLIP)
    out = net.generate(fx["seed_tokens"], SAMPLED, temp=0.7, rseed=int(fx["rseed"]))
    assert out.tolist() == fx["seed_tokens"].tolist() + toks[:, 0].tolist()
    bpc = lambda p: -np.mean([np.log2(float(p[t][text[t + 1]])) for t in range(STEPS)])
    dn.reset_state()
    at07 = bpc(_forced(dn, text[:-1]))
    s = net.score(text)
    assert abs(s["bpc"] - bpc(want)) < 1e-5 * bpc(want) and abs(s["bpc"] - at07) > 1e-3 * at07, (s, bpc(want), at07)
    dn.reset_state(); dn.reset_temperature()
    assert np.array_equal(_forced(dn, text[:-1]), want)
    net.close(); dn.close(); tf.close()
