"""Vector-input networks (char-rnn), host side (no device): what the planner accepts and refuses under `[net] yolo_input=vector`, the weight
stream and the plan dump of such a network, and tests/golden/mini_char_rnn.npz -- one live network of the compiled reference fed a 4-token
seed and then 8 tokens its own sample_array drew, every layer of all 11 steps -- against the float64 restatement of test_recurrent_host.py
and a float32 numpy restatement of the sampler (rnn.c:290-293 + utils.c:592-603).  test_gpu_char_rnn.py compares the device against the
same pieces; tools/make_golden.py records the fixture with them."""
import re
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import hip, darknet_io as IO
from yolo_tensorflow_amd.char_rnn import CharRNN
import test_recurrent_host as RH

FIXTURE = "mini_char_rnn.npz"
STEPS, SEED_LEN, SAMPLED = 11, 4, 8
CLIP = np.float32(CharRNN.CLIP)          # rnn.c:291's `out[j] < .0001` (a double) as a float bound


# ---- restatement shared with test_gpu_char_rnn.py and tools/make_golden.py ----
class CharNet(RH.Net):
    """RH.Net over rows of values: step(x) takes the input vector; a [softmax] applies its temperature (DN/blas.c:305-321); [cost] is left out"""

    def step(self, x):
        x = self.store(np.asarray(x, dtype=np.float32)).astype(np.float64).reshape(1, 1, -1)
        outs = []
        for i, s in enumerate(self.secs):
            if s["type"] == "cost":
                break
            if s["type"] == "softmax":
                t = float(s.get("temperature", 1))
                e = np.exp(x / t - x.max() / t); x = e / e.sum()
            else:
                x = self.layer(i, x)
            outs.append(x)
        return outs


def one_hot(token, n):
    v = np.zeros(n, dtype=np.float32); v[int(token)] = 1
    return v


def run_tokens(cfg, flat, tokens, store=None):
    """[step][layer] outputs of one stream fed the one-hot rows of `tokens` in order"""
    net = CharNet(cfg, flat, store)
    n = IO.vector_inputs(IO.parse_cfg(cfg))
    return [net.step(one_hot(t, n)) for t in tokens]


def sample_np(probs, u, clip=CLIP):
    """rnn.c:290-293 and sample_array in float32, in their order: clip, the sum in index order, every element times (float)(1. / sum), then
    r = u; r -= a[i]; r <= 0 -> i; else n - 1"""
    a = np.array(probs, dtype=np.float32).reshape(-1)
    a[a < np.float32(clip)] = 0
    s = np.float32(0)
    for v in a:
        s = np.float32(s + v)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = (a * np.float32(1.0 / np.float64(s))).astype(np.float32)
        r = np.float32(u)
        for i, v in enumerate(a):
            r = np.float32(r - v)
            if r <= 0:
                return i
    return a.size - 1


def cdf_margin(probs, u, clip=CLIP):
    """how far u stands from the nearest boundary of the clipped, normalised row's running sums (float64)"""
    a = np.array(probs, dtype=np.float64).reshape(-1)
    a[np.asarray(probs, dtype=np.float32).reshape(-1) < np.float32(clip)] = 0
    return float(np.abs(np.cumsum(a / a.sum()) - float(u)).min())


def compared_layers(cfg):
    return [i for i, s in enumerate(IO.parse_cfg(cfg)[1:]) if s["type"] != "cost"]


# ---- rows wider than one block of granules (shared with test_gpu_stream_tiles.py): the input kernels take one 8-element granule per thread and
#      256 threads per block, the sampler writes the next row 256 granules per pass: element BLOCK is the first of a second block / pass ----
BLOCK = 2048
WIDE_N = (2085, 8192)          # 261 granules, the last one ragged; the sampler's limit
LAST_U = np.float32(0.99999994)          # the largest float below 1
# uniforms [10 sampled steps][3 streams]: tails (with near-uniform rows u > 2048 / 2085 = 0.9823 lands past BLOCK at the narrower width too) next to
# heads, and LAST_U for the walk to the end of the row
WIDE_U = np.array([[.30, .995, .10, LAST_U, .15, .99, .20, .999, .05, .70],
                   [LAST_U, .12, .997, .40, LAST_U, .08, .993, .18, .60, .02],
                   [.07, LAST_U, .19, .996, .03, LAST_U, .14, .55, .998, .11]], dtype=np.float32).T.copy()


def wide_cfg(n):
    return "[net]\ninputs=%d\nyolo_input=vector\n\n[lstm]\noutput=16\n\n[connected]\noutput=%d\nactivation=linear\n\n[softmax]\n" % (n, n)


def wide_seed(n):
    """the one forced token of each of the 3 streams: in the first block, just past it, the row's last element"""
    return np.array([[5, BLOCK + 2, n - 1]], dtype=np.int32)


def free_run(cfg, flat, seed, uniforms, store=None):
    """the restatement free-running, as yolo_sequence runs: seed [forced][streams] fed, then the tokens sample_np draws with uniforms [sampled][streams]
    -> tokens [sampled][streams]"""
    n = IO.vector_inputs(IO.parse_cfg(cfg))
    toks = np.zeros(uniforms.shape, dtype=np.int32)
    for b in range(seed.shape[1]):
        net = CharNet(cfg, flat, store)
        for t in seed[:, b]:
            probs = net.step(one_hot(t, n))[-1]
        for k in range(uniforms.shape[0]):
            toks[k, b] = sample_np(probs, uniforms[k, b])
            if k + 1 < uniforms.shape[0]:
                probs = net.step(one_hot(toks[k, b], n))[-1]
    return toks


def wide_coverage(toks, uniforms, n):
    """what a free run over wide rows must have drawn for its self-consistency to say anything about the granules past BLOCK -> the list of what is
    missing.  Only a token that is fed again (every one but the last of a stream) counts."""
    fed = toks[:-1]
    missing = []
    if not (fed >= BLOCK).any() or not (fed < BLOCK).any():
        missing.append("fed tokens on both sides of element %d" % BLOCK)
    if not ((fed == n - 1) & (uniforms[:-1] == LAST_U)).any():
        missing.append("a walk to the row's end (token %d under u = %.8f) that is fed again" % (n - 1, LAST_U))
    if not ((fed[:-1] >= BLOCK) & (fed[1:] < BLOCK)).any():
        missing.append("a fed token past element %d followed by a fed one below it (a stale granule would show)" % BLOCK)
    return missing


# ---- the tests ----
@pytest.fixture(scope="module")
def fx():
    return golden(FIXTURE)


_VEC = ("[net]\ninputs=37\nyolo_input=vector\ntime_steps=8\n\n[rnn]\nbatch_normalize=1\noutput=24\nactivation=leaky\n\n[gru]\noutput=20\n\n[lstm]\noutput=12\n\n"
        "[connected]\noutput=37\nactivation=leaky\n\n[softmax]\ntemperature=0.7\n\n[cost]\n")


def test_a_vector_network_plans_in_16_bit_and_fp32(fx):
    for cfg in (_VEC, str(fx["cfg"])):
        for dt in (hip.BF16, hip.FP16, hip.FP32):
            rc, msg = hip.plan_check(cfg, dtype=dt)
            assert rc == 0, msg


def test_fp8_and_split_fp16_are_refused_by_name():
    dense = "[net]\ninputs=37\nyolo_input=vector\n\n[connected]\noutput=20\nactivation=leaky\n\n[connected]\noutput=5\nactivation=linear\n\n[softmax]\n"
    for dt, word in ((hip.FP8, "fp8"), (hip.FP16X2, "split-fp16")):
        rc, msg = hip.plan_check(_VEC, dtype=dt)
        assert rc != 0 and msg.startswith("layer 0: [rnn]") and word in msg, msg
        rc, msg = hip.plan_check(dense, dtype=dt)
        assert rc != 0 and "vector-input network" in msg and word in msg, msg
    assert hip.plan_check(dense, dtype=hip.BF16)[0] == 0


def test_contradictions_and_bad_sizes_are_refused():
    rc, msg = hip.plan_check(_VEC.replace("inputs=37", "inputs=37\nheight=8\nwidth=8"), dtype=hip.BF16)
    assert rc != 0 and "yolo_input=vector" in msg and "height=8" in msg and "width=8" in msg, msg
    for bad in ("inputs=0", "inputs=-4", "batch=1"):
        rc, msg = hip.plan_check(_VEC.replace("inputs=37", bad), dtype=hip.BF16)
        assert rc != 0 and "inputs=" in msg and "yolo_input=vector" in msg, msg
    rc, msg = hip.plan_check(_VEC.replace("yolo_input=vector", "yolo_input=image"), dtype=hip.BF16)
    assert rc != 0 and "yolo_input=image" in msg, msg
    # without the key nothing changes: the old refusal, now with a pointer at the key
    rc, msg = hip.plan_check(_VEC.replace("yolo_input=vector\n", ""), dtype=hip.BF16)
    assert rc != 0 and "3 channels" in msg and "yolo_input=vector" in msg, msg


@pytest.mark.parametrize("section", ["[convolutional]\nfilters=8\nsize=1\nactivation=leaky\n", "[maxpool]\nsize=2\nstride=2\n", "[avgpool]\n"])
def test_image_sections_are_refused_in_a_vector_network(section):
    kind = section[1:section.index("]")]
    rc, msg = hip.plan_check(_VEC.replace("[gru]\noutput=20\n", section), dtype=hip.BF16)
    assert rc != 0 and msg.startswith("layer 1: [%s]" % kind) and "image-shaped input" in msg, msg


def test_the_output_layer_must_be_a_softmax():
    rc, msg = hip.plan_check(_VEC.replace("[softmax]\ntemperature=0.7\n\n", ""), dtype=hip.BF16)
    assert rc != 0 and "[softmax]" in msg and "vector-input" in msg, msg


def test_weight_stream_and_plan_dump(fx):
    for cfg, n, streams in ((_VEC, 37, 3), (str(fx["cfg"]), 37, 1), (_VEC.replace("inputs=37", "inputs=256"), 256, 32)):
        secs = IO.parse_cfg(cfg)
        assert IO.vector_inputs(secs) == n and IO.layer_shapes(secs)[0][1:] == (1, 1, 24, n)
        rc, dump = hip.plan_dump(cfg, dtype=hip.BF16, max_batch=streams)
        assert rc == 0, dump
        planned = int(re.search(r"weights_count=(\d+)", dump).group(1))
        assert planned == IO.weights_count(secs) == IO.synth_weights(secs).size
        assert len(IO.recurrent_specs(secs)) == 3 and IO.recurrent_specs(secs)[0]["inputs"] == n
        assert re.search(r"^vector_input inputs=%d stride=%d dt=0 streams=%d$" % (n, (n + 7) // 8 * 8, streams), dump, flags=re.M), dump
        assert "in_h=1 in_w=1 in_c=%d " % n in dump
    assert fx["weights"].size == IO.weights_count(IO.parse_cfg(str(fx["cfg"])))
    rc, dump = hip.plan_dump(IO.cfg_text("yolov3-tiny"), dtype=hip.BF16)
    assert rc == 0 and "vector_input" not in dump


def test_the_key_is_added_to_a_darknet_cfg_that_lacks_it():
    plain = _VEC.replace("yolo_input=vector\n", "")
    added = IO.with_vector_input(plain)
    assert IO.parse_cfg(added)[0]["yolo_input"] == "vector" and IO.parse_cfg(added)[1:] == IO.parse_cfg(plain)[1:]
    assert hip.plan_check(added, dtype=hip.BF16)[0] == 0
    assert IO.with_vector_input(_VEC) == _VEC and IO.with_vector_input(IO.cfg_text("yolov3-tiny")) == IO.cfg_text("yolov3-tiny")


def test_fixture_shape(fx):
    cfg = str(fx["cfg"]); secs = IO.parse_cfg(cfg)
    assert [s["type"] for s in secs[1:]] == ["rnn", "gru", "lstm", "connected", "softmax", "cost"] and secs[0]["yolo_input"] == "vector"
    assert fx["seed_tokens"].shape == (SEED_LEN,) and fx["tokens"].shape == (SAMPLED,) and fx["uniforms"].shape == (SAMPLED,) and fx["fed"].shape == (STEPS,)
    assert np.array_equal(fx["fed"], np.concatenate([fx["seed_tokens"], fx["tokens"][:-1]]))
    for i, width in enumerate((24, 20, 12, 37, 37)):
        assert fx["layer_%02d" % i].shape == (STEPS, 1, 1, width)


def test_restatement_matches_the_reference_at_every_layer_and_step(fx):
    """float64 on its own carried state, fed the tokens the reference fed itself: test_recurrent_host.py's fixture bound, 5e-4 of each
    tensor's scale"""
    cfg = str(fx["cfg"])
    outs = run_tokens(cfg, fx["weights"], fx["fed"])
    worst = 0.0
    for t in range(STEPS):
        for i in compared_layers(cfg):
            r = RH.standoff(outs[t][i], fx["layer_%02d" % i][t])
            worst = max(worst, r)
            assert r < 5e-4, (t, i, r)
    print("worst stand-off %.3e" % worst)
    fresh = CharNet(cfg, fx["weights"]).step(one_hot(fx["fed"][1], 37))          # the state matters
    assert all(RH.standoff(fresh[i], fx["layer_%02d" % i][1]) > 5e-3 for i in (0, 1, 2))


def test_fixture_drift_figures_are_the_restatements(fx):
    cfg = str(fx["cfg"])
    for name, store in (("bf16", RH.bf16), ("fp16", RH.fp16)):
        outs = run_tokens(cfg, fx["weights"], fx["fed"], store)
        drift = np.array([[RH.standoff(outs[t][i], fx["layer_%02d" % i][t]) for i in compared_layers(cfg)] for t in range(STEPS)])
        assert np.allclose(drift, fx["drift16_" + name], rtol=1e-3, atol=1e-9)
        assert drift.max() < (0.1 if name == "bf16" else 0.02)


def test_numpy_sampler_reproduces_the_reference_and_the_fixture_conditions_hold(fx):
    probs = fx["layer_04"].reshape(STEPS, -1)[SEED_LEN - 1:]
    assert probs.shape == (SAMPLED, 37)
    got = [sample_np(probs[k], fx["uniforms"][k]) for k in range(SAMPLED)]
    assert got == fx["tokens"].tolist()
    margins = np.array([cdf_margin(probs[k], fx["uniforms"][k]) for k in range(SAMPLED)])
    assert np.allclose(margins, fx["margin"], rtol=1e-6, atol=1e-12)
    assert fx["margin"].min() >= 1e-3, fx["margin"]
    assert ((probs > 0) & (probs < 1e-4)).any(), "the clip changes nothing in this fixture"
    assert len(set(fx["tokens"].tolist())) > 1


def test_sampler_edges():
    """u = 0 takes class 0 whatever its probability (r = 0 - a[0] <= 0), also where the clip removed it; a u on a boundary takes the class below
    it; u just below 1 walks to the class whose running sum reaches it; a row clipped whole gives the last class, through NaN"""
    p = np.array([0.25, 0.25, 0.5], dtype=np.float32)
    assert sample_np(p, 0.0) == 0 and sample_np(p, 0.25) == 0 and sample_np(p, 0.2500001) == 1 and sample_np(p, 0.99999994) == 2
    assert sample_np(np.array([5e-5, 0.9999, 5e-5], dtype=np.float32), 0.0) == 0
    assert sample_np(np.array([5e-5, 0.9999, 5e-5], dtype=np.float32), 0.5) == 1
    assert sample_np(np.full(7, 1e-5, dtype=np.float32), 0.3) == 6


@pytest.mark.parametrize("n", WIDE_N)
def test_wide_row_inputs_reach_both_sides_of_the_second_block(n):
    """the inputs test_gpu_stream_tiles.py free-runs over rows wider than one block of granules, under the restatement alone (float64, and rounded
    where a 16-bit device rounds): the tokens it draws and feeds again lie on both sides of element BLOCK, one walk ends at the row's last element,
    one token past BLOCK is followed by one below it.  The device test asserts the same of the tokens the device returned."""
    cfg = wide_cfg(n); secs = IO.parse_cfg(cfg)
    for dt in (hip.BF16, hip.FP16, hip.FP32):
        rc, msg = hip.plan_check(cfg, dtype=dt)
        assert rc == 0, msg
    flat = IO.synth_weights(secs, seed=n)
    assert WIDE_U.shape == (10, 3) and (WIDE_U == LAST_U).sum() == 5 and LAST_U < 1 and np.nextafter(LAST_U, np.float32(2)) == 1
    for store in (None, RH.bf16, RH.fp16):
        toks = free_run(cfg, flat, wide_seed(n), WIDE_U, store)
        print("N = %d %s: %s" % (n, store.__name__ if store else "float64", toks.T.tolist()))
        assert wide_coverage(toks, WIDE_U, n) == []
    none = np.full((10, 3), 7, dtype=np.int32)
    assert len(wide_coverage(none, WIDE_U, n)) == 3


def test_darknet_uniforms_are_the_fixtures(fx):
    u = CharRNN.darknet_uniforms(int(fx["rseed"]), SAMPLED)
    assert u.dtype == np.float32 and np.array_equal(u, fx["uniforms"])
    assert np.array_equal(CharRNN.darknet_uniforms(int(fx["rseed"]), 3), fx["uniforms"][:3])
