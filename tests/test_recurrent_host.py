"""Recurrent networks, host side (no device): a numpy restatement of [crnn], [rnn], [gru], [lstm] and of the batch-norm-folded [connected]
layer -- the whole of a small network, stepped over a sequence of frames with its state carried along -- checked against the compiled
reference's recorded layer outputs (tests/golden/mini_seq.npz, mini_crnn.npz: 5 frames through one live network each); what the planner accepts and refuses; the weight
stream's length; the launches a plan holds per recurrent layer.  test_gpu_recurrent.py compares the device against the same restatement,
tools/make_golden.py runs it with 16-bit rounding for the fixture's drift16_* figures."""
import re
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import hip, darknet_io as IO

FIXTURE = "mini_seq.npz"
FIXTURES = ("mini_seq.npz", "mini_crnn.npz")
STATEFUL = tuple(IO.RECURRENT) + ("crnn",)
T = 5
SLOPES = {"linear": 1.0, "leaky": 0.1, "relu": 0.0, "relie": 0.01}


# ---- restatement shared with test_gpu_recurrent.py and tools/make_golden.py ----
def bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def fp16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def activate(y, name):
    if name in SLOPES:
        return np.where(y > 0, y, SLOPES[name] * y)
    if name == "logistic":
        return 1.0 / (1.0 + np.exp(-y))
    if name == "tanh":
        return np.tanh(y)
    raise ValueError(name)


def _fold(bias, w, bn):
    """rows and bias of a layer with its batch norm folded (DN/blas.c normalize_cpu: (x - mean) / (sqrt(var) + .000001f), scale, bias)"""
    w = w.astype(np.float64); bias = bias.astype(np.float64)
    if bn is None:
        return w, bias
    gamma, mean, var = (v.astype(np.float64) for v in bn)
    s = gamma / (np.sqrt(var) + np.float64(np.float32(1e-6)))
    return w * s.reshape((-1,) + (1,) * (w.ndim - 1)), bias - mean * s


def _take_connected(flat, pos, inputs, outputs, bn):
    """one [connected] (sub)layer of the stream: biases, weights [outputs][inputs], then scales, rolling mean, rolling variance"""
    b = flat[pos:pos + outputs]; pos += outputs
    w = flat[pos:pos + outputs * inputs].reshape(outputs, inputs); pos += outputs * inputs
    stats = None
    if bn:
        stats = (flat[pos:pos + outputs], flat[pos + outputs:pos + 2 * outputs], flat[pos + 2 * outputs:pos + 3 * outputs]); pos += 3 * outputs
    return _fold(b, w, stats), pos


def stream_params(cfg, flat):
    """per layer: None, or (w, b) of a conv ([cout][cin][k][k]) / [connected], or the list of (w, b) of a recurrent layer's sublayers in file order"""
    secs = IO.parse_cfg(cfg); shapes = IO.layer_shapes(secs); flat = np.asarray(flat, dtype=np.float32)
    out, pos = [], 0
    for i, s in enumerate(secs[1:]):
        t, cin = s["type"], shapes[i][4]
        bn = int(s.get("batch_normalize", 0))
        if t == "convolutional":
            n, k = int(s["filters"]), int(s["size"])
            b = flat[pos:pos + n]; pos += n
            stats = None
            if bn:
                stats = (flat[pos:pos + n], flat[pos + n:pos + 2 * n], flat[pos + 2 * n:pos + 3 * n]); pos += 3 * n
            w = flat[pos:pos + n * cin * k * k].reshape(n, cin, k, k); pos += n * cin * k * k
            out.append(_fold(b, w, stats))
        elif t == "connected":
            p, pos = _take_connected(flat, pos, cin, int(s["output"]), bn)
            out.append(p)
        elif t == "crnn":
            convs = []
            for ci, n in ((cin, int(s["hidden_filters"])), (int(s["hidden_filters"]), int(s["hidden_filters"])), (int(s["hidden_filters"]), int(s["output_filters"]))):
                b = flat[pos:pos + n]; pos += n
                stats = None
                if bn:
                    stats = (flat[pos:pos + n], flat[pos + n:pos + 2 * n], flat[pos + 2 * n:pos + 3 * n]); pos += 3 * n
                w = flat[pos:pos + n * ci * 9].reshape(n, ci, 3, 3); pos += n * ci * 9
                convs.append(_fold(b, w, stats))
            out.append(convs)
        elif t in IO.RECURRENT:
            subs = []
            for kind in IO.RECURRENT[t]:
                p, pos = _take_connected(flat, pos, cin if kind == "x" else int(s["output"]), int(s["output"]), bn)
                subs.append(p)
            out.append(subs)
        else:
            out.append(None)
    assert pos == flat.size, (pos, flat.size)
    return out


def conv_ref(x, w, b, stride, pad):
    """x [h, w, cin], w [cout][cin][k][k] -> [ho, wo, cout] (float64)"""
    k = w.shape[2]; h, wd, _ = x.shape
    xp = np.zeros((h + 2 * pad, wd + 2 * pad, x.shape[2])); xp[pad:pad + h, pad:pad + wd] = x
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    y = np.zeros((ho, wo, w.shape[0]))
    for kh in range(k):
        for kw in range(k):
            y += xp[kh:kh + (ho - 1) * stride + 1:stride, kw:kw + (wo - 1) * stride + 1:stride] @ w[:, :, kh, kw].T
    return y + b


class Net:
    """The layers of a cfg over frames, one per step() call, state carried between calls (zero at construction).  store: None -- float64
    throughout, the restatement proper -- or a rounding function (bf16 / fp16): then every operand and every stored tensor is rounded where
    the device rounds it -- the folded weights, the staged image, each layer's output (the fp32 logits in front of a [softmax] excepted), the
    state an [rnn] / [lstm] keeps as a matrix operand, a [gru]'s r * h -- while biases, an [lstm]'s cell, a [gru]'s own state and z stay
    unrounded, as the device keeps them in fp32."""

    def __init__(self, cfg, flat, store=None):
        self.secs = IO.parse_cfg(cfg)[1:]
        self.store = store or (lambda v: v)
        self.params = stream_params(cfg, flat)
        rw = lambda p: (self.store(p[0]).astype(np.float64), p[1])
        self.params = [None if p is None else [rw(q) for q in p] if isinstance(p, list) else rw(p) for p in self.params]
        self.state = {}

    def _flat(self, x):          # darknet flattens CHW
        return np.transpose(x, (2, 0, 1)).reshape(-1)

    def step(self, image01):
        """image [h, w, 3] in 0..1 -> the list of every layer's output [h, w, c] of this time step"""
        x = self.store(np.asarray(image01, dtype=np.float32)).astype(np.float64)
        outs = []
        for i in range(len(self.secs)):
            x = self.layer(i, x)
            outs.append(x)
        return outs

    def layer(self, i, x):
        """layer i over its input tensor x [h, w, c] (float64, already as stored); a recurrent layer advances its state"""
        st = self.store; s = self.secs[i]; t = s["type"]
        if True:
            fp32_out = i + 1 < len(self.secs) and self.secs[i + 1]["type"] in ("softmax", "yolo", "detection")
            keep = (lambda v: v) if fp32_out else (lambda v: st(v).astype(np.float64))
            if t == "convolutional":
                w, b = self.params[i]
                k = int(s["size"]); pad = k // 2 if int(s.get("pad", 0)) else int(s.get("padding", 0))
                x = keep(activate(conv_ref(x, w, b, int(s.get("stride", 1)), pad), s.get("activation", "logistic")))
            elif t == "maxpool":
                k, sd = int(s["size"]), int(s["stride"]); h, wd, c = x.shape
                assert k == sd and h % k == 0 and wd % k == 0
                x = x.reshape(h // k, k, wd // k, k, c).max(axis=(1, 3))
            elif t == "avgpool":
                x = keep(x.mean(axis=(0, 1), keepdims=True))
            elif t == "connected":
                w, b = self.params[i]
                x = keep(activate(w @ self._flat(x) + b, s.get("activation", "logistic"))).reshape(1, 1, -1)
            elif t == "crnn":
                (wi, bi), (ws, bs), (wo, bo) = self.params[i]
                act = s.get("activation", "logistic"); hid = int(s["hidden_filters"])
                h = self.state.get(i, np.zeros(x.shape[:2] + (hid,)))
                # the device sums in the convs' epilogues and stores each sum: [state +] act(conv_in(x)), then that + act(conv_self(state))
                mid = st((h if int(s.get("shortcut", 0)) else 0.0) + activate(conv_ref(x, wi, bi, 1, 1), act)).astype(np.float64)
                new = st(mid + activate(conv_ref(h, ws, bs, 1, 1), act)).astype(np.float64)
                self.state[i] = new
                x = keep(activate(conv_ref(new, wo, bo, 1, 1), act))
            elif t == "yolo":
                pass
            elif t == "rnn":
                (wi, bi), (ws, bs), (wo, bo) = self.params[i]
                n, act = int(s["output"]), s.get("activation", "logistic")
                h = self.state.get(i, np.zeros(n))
                new = (h if int(s.get("shortcut", 0)) else 0.0) + activate(wi @ self._flat(x) + bi, act) + activate(ws @ h + bs, act)
                new = st(new).astype(np.float64)
                self.state[i] = new
                x = keep(activate(wo @ new + bo, act)).reshape(1, 1, -1)
            elif t == "gru":
                (wz, bwz), (wr, bwr), (wh, bwh), (uz, buz), (ur, bur), (uh, buh) = self.params[i]
                n = int(s["output"])
                h = self.state.get(i, np.zeros(n)); hop = st(h).astype(np.float64); xin = self._flat(x)
                z = activate((uz @ xin + buz) + (wz @ hop + bwz), "logistic")
                r = activate((ur @ xin + bur) + (wr @ hop + bwr), "logistic")
                rh = st(r * h).astype(np.float64)
                cand = activate((uh @ xin + buh) + (wh @ rh + bwh), "tanh" if int(s.get("tanh", 0)) else "logistic")
                self.state[i] = z * h + (1 - z) * cand
                x = keep(self.state[i]).reshape(1, 1, -1)
            elif t == "lstm":
                (wi, bwi), (wf, bwf), (wo, bwo), (wg, bwg), (ui, bui), (uf, buf), (uo, buo), (ug, bug) = self.params[i]
                n = int(s["output"])
                h, c = self.state.get(i, (np.zeros(n), np.zeros(n))); xin = self._flat(x)
                gi = activate((wi @ h + bwi) + (ui @ xin + bui), "logistic"); gf = activate((wf @ h + bwf) + (uf @ xin + buf), "logistic")
                go = activate((wo @ h + bwo) + (uo @ xin + buo), "logistic"); gg = activate((wg @ h + bwg) + (ug @ xin + bug), "tanh")
                c = gf * c + gi * gg
                h = st(go * np.tanh(c)).astype(np.float64)
                self.state[i] = (h, c)
                x = keep(h).reshape(1, 1, -1)
            elif t == "softmax":
                e = np.exp(x - x.max()); x = e / e.sum()
            else:
                raise ValueError(t)
        return x


def run_frames(cfg, flat, images_u8, store=None):
    """[T][layer] outputs of one stream fed the frames in order"""
    net = Net(cfg, flat, store)
    return [net.step(img.astype(np.float32) / np.float32(255.0)) for img in images_u8]


def standoff(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - np.asarray(want, dtype=np.float64).reshape(-1)).max() / np.abs(want).max())


# ---- the tests ----
@pytest.fixture(scope="module")
def seq():
    return golden(FIXTURE)


def compared_layers(cfg):
    """every layer but a [yolo] head (the reference's copy of it holds activated values; the raw tensor is the conv's in front of it)"""
    return [i for i, s in enumerate(IO.parse_cfg(cfg)[1:]) if s["type"] != "yolo"]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_the_reference_at_every_layer_and_step(name):
    """float64, the whole network on its own tensors and its own carried state: 5e-4 of each tensor's scale, the bound of
    test_unet_host.py's restatements (measured: below 2e-6, the reference's fp32 sums)"""
    seq = golden(name)
    cfg = str(seq["cfg"])
    outs = run_frames(cfg, seq["weights"], seq["images_u8"])
    assert len(outs) == T == seq["images_u8"].shape[0]
    worst = 0.0
    for t in range(T):
        for i in compared_layers(cfg):
            got, want = outs[t][i], seq["layer_%02d" % i][t]
            assert got.size == want.size
            r = standoff(got, want)
            worst = max(worst, r)
            assert r < 5e-4, (t, i, r)
    print("worst stand-off %.3e" % worst)
    # the state matters: step 2 of a fresh network is not what the fixture holds for it
    fresh = Net(cfg, seq["weights"]).step(seq["images_u8"][1].astype(np.float32) / np.float32(255.0))
    rnn = [i for i, s in enumerate(IO.parse_cfg(cfg)[1:]) if s["type"] in STATEFUL]
    assert rnn and all(standoff(fresh[i], seq["layer_%02d" % i][1]) > 5e-3 for i in rnn)


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fixture_drift_figures_are_the_restatements(fixture):
    """drift16_*: what tools/make_golden.py recorded is what the rounded restatement gives here"""
    seq = golden(fixture)
    cfg = str(seq["cfg"])
    for name, store in (("bf16", bf16), ("fp16", fp16)):
        outs = run_frames(cfg, seq["weights"], seq["images_u8"], store)
        drift = np.array([[standoff(outs[t][i], seq["layer_%02d" % i][t]) for i in compared_layers(cfg)] for t in range(T)])
        assert np.allclose(drift, seq["drift16_" + name], rtol=1e-3, atol=1e-9)
        assert drift.max() < (0.1 if name == "bf16" else 0.02)


def _first_recurrent(cfg):
    secs = IO.parse_cfg(cfg)[1:]
    return next(i for i, s in enumerate(secs) if s["type"] in STATEFUL), secs


@pytest.mark.parametrize("fixture", FIXTURES)
def test_planner_serves_the_fixture_in_16_bit_and_fp32_and_refuses_it_elsewhere(fixture):
    cfg = str(golden(fixture)["cfg"])
    for dt in (hip.BF16, hip.FP16, hip.FP32):
        rc, msg = hip.plan_check(cfg, dtype=dt)
        assert rc == 0, msg
    first, secs = _first_recurrent(cfg)
    for dt, word in ((hip.FP8, "fp8"), (hip.FP16X2, "split-fp16")):
        rc, msg = hip.plan_check(cfg, dtype=dt)
        assert rc != 0 and msg.startswith("layer %d: [%s]" % (first, secs[first]["type"])) and word in msg, msg


_HEAD = "[net]\nbatch=1\nwidth=16\nheight=16\nchannels=3\n\n[convolutional]\nfilters=8\nsize=3\nstride=2\npad=1\nactivation=leaky\n\n"


@pytest.mark.parametrize("kind", ["rnn", "gru", "lstm", "connected"])
def test_zero_and_negative_sizes_are_refused(kind):
    for n in (0, -3):
        rc, msg = hip.plan_check(_HEAD + "[%s]\noutput=%d\n\n[connected]\noutput=4\nactivation=linear\n\n[softmax]\n" % (kind, n), dtype=hip.BF16)
        assert rc != 0 and "layer 1: [%s] output=%d" % (kind, n) in msg, msg


@pytest.mark.parametrize("keys", ["hidden_filters=0\noutput_filters=8", "hidden_filters=8\noutput_filters=0", "hidden_filters=-2\noutput_filters=8"])
def test_crnn_sizes_must_be_positive(keys):
    rc, msg = hip.plan_check(_HEAD + "[crnn]\n%s\nactivation=leaky\n\n[convolutional]\nfilters=18\nsize=1\nactivation=linear\n\n[yolo]\nmask=0,1,2\nanchors=4,5,8,6,10,14\nclasses=1\nnum=3\n" % keys, dtype=hip.BF16)
    assert rc != 0 and msg.startswith("layer 1: [crnn] hidden_filters="), msg


def test_rectangular_crnn_is_refused_and_a_square_one_served():
    """DN/parser.c:215 hands make_crnn_layer (w, h) for (h, w): the reference's layer means something on a square map only"""
    tail = "[crnn]\nhidden_filters=12\noutput_filters=8\nactivation=leaky\n\n[convolutional]\nfilters=18\nsize=1\nactivation=linear\n\n[yolo]\nmask=0,1,2\nanchors=4,5,8,6,10,14\nclasses=1\nnum=3\n"
    rc, msg = hip.plan_check(_HEAD + tail, dtype=hip.BF16)
    assert rc == 0, msg
    rc, msg = hip.plan_check(_HEAD.replace("width=16", "width=24") + tail, dtype=hip.BF16)
    assert rc != 0 and msg.startswith("layer 1: [crnn]") and "square" in msg, msg
    rc, msg = hip.plan_check(_HEAD + tail.replace("activation=leaky\n", "", 1), dtype=hip.BF16)          # the section's default activation, logistic
    assert rc == 0, msg


@pytest.mark.parametrize("kind", ["rnn", "gru", "lstm"])
def test_sizes_that_are_no_multiple_of_8_and_a_direct_softmax_are_served(kind):
    """output=20: the state's and the output's last granule is padded with zeros; a [softmax] straight behind the layer reads fp32"""
    for dt in (hip.BF16, hip.FP16, hip.FP32):
        rc, msg = hip.plan_check(_HEAD + "[%s]\noutput=20\n\n[softmax]\n" % kind, dtype=dt)
        assert rc == 0, msg


def test_batch_normalised_connected_is_served():
    cfg = _HEAD + "[connected]\noutput=12\nbatch_normalize=1\nactivation=leaky\n\n[connected]\noutput=4\nactivation=linear\n\n[softmax]\n"
    rc, msg = hip.plan_check(cfg, dtype=hip.BF16)
    assert rc == 0, msg
    assert IO.weights_count(IO.parse_cfg(cfg)) == 8 * (1 + 27) + 12 * (1 + 512 + 3) + 4 * (1 + 12)


def test_vector_input_networks_stay_refused():
    """[net] inputs=256 without height / width / channels (char-rnn): outside the scope, refused as before"""
    rc, msg = hip.plan_check("[net]\nbatch=1\ninputs=256\ntime_steps=8\n\n[rnn]\noutput=64\n\n[connected]\noutput=256\nactivation=linear\n\n[softmax]\n", dtype=hip.BF16)
    assert rc != 0 and "3 channels" in msg, msg


@pytest.mark.parametrize("fixture", FIXTURES)
def test_weight_stream_length(fixture):
    seq = golden(fixture)
    cfg = str(seq["cfg"])
    rc, dump = hip.plan_dump(cfg, dtype=hip.BF16)
    assert rc == 0, dump
    planned = int(re.search(r"weights_count=(\d+)", dump).group(1))
    assert planned == seq["weights"].size == IO.weights_count(IO.parse_cfg(cfg)) == IO.synth_weights(IO.parse_cfg(cfg)).size


def test_plan_dump_names_the_launches_of_every_recurrent_layer(seq):
    """one launch per [lstm] step, two per [gru] step, at most two per [rnn] step; the states are allocations of the layers' own, no
    members of the pool"""
    cfg = str(seq["cfg"]); secs = IO.parse_cfg(cfg)[1:]
    for dt in (hip.BF16, hip.FP32):
        rc, dump = hip.plan_dump(cfg, dtype=dt, max_batch=3)
        assert rc == 0, dump
        lines = {int(m.group(1)): m.group(0) for m in re.finditer(r"^recurrent (\d+) .*$", dump, flags=re.M)}
        want = [i for i, s in enumerate(secs) if s["type"] in IO.RECURRENT]
        assert sorted(lines) == want and len(want) == 6
        for i in want:
            kind, launches = secs[i]["type"], int(re.search(r"launches=(\d+)", lines[i]).group(1))
            assert "kind=%s " % kind in lines[i] and "state=own" in lines[i]
            assert launches == 1 if kind == "lstm" else launches == 2 if kind == "gru" else launches <= 2
            assert lines[i].count("launch") - 1 == launches


def test_plan_dump_of_the_crnn_fixture():
    """three conv launches per [crnn] layer, none of them visible to the 1x1-tail and fused-block passes (they are no layers of the plan)"""
    g = golden("mini_crnn.npz"); cfg = str(g["cfg"])
    rc, dump = hip.plan_dump(cfg, dtype=hip.BF16, max_batch=2)
    assert rc == 0, dump
    lines = re.findall(r"^recurrent (\d+) kind=crnn .*$", dump, flags=re.M)
    assert lines == ["3", "4"]
    for m in re.finditer(r"^recurrent \d+ kind=crnn (.*)$", dump, flags=re.M):
        assert "launches=3" in m.group(1) and m.group(1).count("conv") == 3 and "state=own(8x8x" in m.group(1)
    assert "hidden=20 output=24 shortcut=0" in dump and "hidden=16 output=16 shortcut=1" in dump
    assert not re.search(r"^layer [34] .* tail_layer=[0-9]", dump, flags=re.M) and not re.search(r"^layer [34] .* fused=[1-9]", dump, flags=re.M)


def test_the_video_cfgs_plan(tmp_path):
    """tools/make_cfgs.py --video DIR: yolov3-tiny with a [crnn] ahead of each head, darknet19 features -> [gru] -> [connected] -> [softmax],
    and their twins without the recurrent layers"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, os.path.join(root, "tools", "make_cfgs.py"), "--video", str(tmp_path)], check=True, capture_output=True)
    want = {"yolov3-tiny-crnn.cfg": ["crnn", "crnn"], "darknet19-gru.cfg": ["gru"], "yolov3-tiny-conv.cfg": [], "darknet19-fc.cfg": []}
    assert sorted(os.listdir(str(tmp_path))) == sorted(want)
    for name, kinds in want.items():
        cfg = open(os.path.join(str(tmp_path), name)).read()
        assert [s["type"] for s in IO.parse_cfg(cfg)[1:] if s["type"] in STATEFUL] == kinds
        for dt in (hip.BF16, hip.FP16, hip.FP32):
            rc, msg = hip.plan_dump(cfg, dtype=dt, max_batch=32)
            assert rc == 0, (name, msg)
        assert IO.synth_weights(IO.parse_cfg(cfg)).size == IO.weights_count(IO.parse_cfg(cfg)) == int(re.search(r"weights_count=(\d+)", msg).group(1))


def test_dump_of_a_network_without_recurrent_layers_has_no_new_line():
    rc, dump = hip.plan_dump(IO.cfg_text("yolov3-tiny"), dtype=hip.BF16)
    assert rc == 0 and "recurrent" not in dump
