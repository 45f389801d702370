"""The stream dimension of the recurrent and sequence kernels, and rows wider than one block of granules.

k_recur (rnn_ops.hip) tiles the streams: NT = 1 covers 16 streams where n <= 16, else NT = 2 covers 32 per workgroup and grid.y = ceil(n / 32).
Here it runs at the exact NT = 1 edge (16), at ragged NT = 2 tiles (17, 31), with a second and a third block row (33 .. 65), and with a block whose
second 16-stream tile is wholly empty (33, 65), every stream against float64 and every stream behind n against what was set.  The kernels of
seq_ops.hip take one 8-element granule per thread and 256 threads per block: rows of 2085 and 8192 elements need a second block of k_vector_in /
k_token_in and further passes of the sampler's row loop.  yolo_sequence, the [connected] GEMM whose M is the stream count, op_sample and a
device-resident token outside the row run at the same stream counts and widths.

Every restatement and every bound is an existing one: test_recurrent_host.Net, test_char_rnn_host.CharNet / sample_np / one_hot, the bounds of
test_gpu_recurrent.py::test_gate_gemm_against_float64 and of test_gpu_char_rnn.py::test_forward_vectors_against_float64."""
import numpy as np
import pytest
from yolo_tensorflow_amd import darknet_io as IO
import test_recurrent_host as RH
import test_char_rnn_host as CH
import test_gpu_recurrent as GR
import test_gpu_char_rnn as GC

pytestmark = pytest.mark.gpu

STREAMS = 72                                             # three block rows of NT = 2, the last one with 8 streams
TILE_EDGES = (15, 16, 17, 31, 32, 33, 48, 64, 65)
TOL16 = GC.TOL16
KIND_IDS = ["lstm", "lstm_bn", "gru_tanh", "gru_bn", "rnn_leaky_shortcut", "rnn_bn"]
DTYPES = ["fp32", "bf16", "fp16"]
INPUTS, UNITS = 136, 40                                  # Kx 136 -> 160: five K steps, a ragged last one, all four waves; a ragged last M tile


def _dtype(hiplib, name):
    return {"fp32": (hiplib.FP32, None), "bf16": (hiplib.BF16, RH.bf16), "fp16": (hiplib.FP16, RH.fp16)}[name]


def _all_states(eng):
    return GC._states(eng, STREAMS)


# ---- A: the gate GEMM at every stream-tile boundary ----
def _gate_cfg(kind, keys):
    # the recurrent layer first: its x operand is the input row exactly; its own output goes to the [softmax] unrounded (fp32)
    return "[net]\ninputs=%d\nyolo_input=vector\n\n[%s]\noutput=%d\n%s\n[softmax]\n" % (INPUTS, kind, UNITS, keys)


class _Gate:
    """one recurrent layer on a 72-stream engine, and the float64 restatement of one step of it from a given state"""

    def __init__(self, hiplib, kind, keys, name):
        self.kind, self.name = kind, name
        self.dtype, store = _dtype(hiplib, name)
        self.st = store or (lambda v: v)
        cfg = _gate_cfg(kind, keys)
        flat = IO.synth_weights(IO.parse_cfg(cfg), seed=INPUTS + UNITS)
        self.eng = GR._engine(hiplib, cfg, flat, self.dtype, batch=STREAMS, keep=True)
        self.tensors = 2 if kind == "lstm" else 1
        assert self.eng.vector_inputs == INPUTS and self.eng.num_state_tensors == self.tensors and self.eng.state_geometry(0) == (0, UNITS)
        self.ref = RH.Net(cfg, flat, store)
        self.fp32 = self.dtype == hiplib.FP32

    def want(self, x, start):
        """x [INPUTS], start [tensors][UNITS] (float32, as handed to set_state) -> the layer's output and every state it leaves (float64)"""
        st = self.st
        h0 = start[0].astype(np.float64)
        self.ref.state[0] = (st(h0).astype(np.float64), start[1].astype(np.float64)) if self.kind == "lstm" else h0 if self.kind == "gru" else st(h0).astype(np.float64)
        out = self.ref.layer(0, st(x).astype(np.float64).reshape(1, 1, -1)).reshape(-1)
        after = self.ref.state[0] if self.kind == "lstm" else (self.ref.state[0],)
        return out, [np.asarray(a, dtype=np.float64) for a in after]

    def kept(self, k, values):
        """what get_state returns of a state that set_state wrote and no step touched: the operand states are stored rounded"""
        return values if (self.fp32 or self.kind == "gru" or k == 1) else self.st(values)

    def set_all(self, start):
        self.eng.reset_state()
        for k in range(self.tensors):
            for b in range(STREAMS):
                self.eng.set_state(k, b, start[k][b])

    def step(self, x):
        """forward_vectors over x [n][INPUTS] -> the layer's fp32 output [n][UNITS]"""
        n = x.shape[0]
        self.eng.forward_vectors(x)
        out = self.eng.layer_output(0, n).reshape(n, -1)
        assert out.shape == (n, UNITS)
        return out

    def ratio(self, got, want):
        """the error as a share of test_gate_gemm_against_float64's bound: fp32 1e-4 of the tensor's scale; bf16 2^-7 |want| + 2e-3; fp16 2^-10 |want| + 2e-3"""
        err = np.abs(got.astype(np.float64) - want)
        if self.fp32:
            return float(err.max() / np.abs(want).max()) / 1e-4
        return float((err / (2.0 ** (-7 if self.name == "bf16" else -10) * np.abs(want) + 2e-3)).max())


def _gate_inputs():
    rng = np.random.default_rng(UNITS)
    x = rng.normal(0, 1, (STREAMS, INPUTS)).astype(np.float32)
    start = [rng.uniform(-0.9, 0.9, (STREAMS, UNITS)).astype(np.float32) for _ in range(2)]
    return x, start


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("kind,keys", GR.GATE_KINDS, ids=KIND_IDS)
def test_gate_gemm_at_every_stream_tile_boundary(hiplib, kind, keys, name):
    """n = 15 .. 65 of a 72-stream context, every state of every stream non-zero: the layer's fp32 output and every state it leaves, of EVERY
    stream below n, against float64 on operands pre-rounded to the storage type (test_gate_gemm_against_float64's bounds); every state of every
    stream from n on -- stream n is the first masked lane -- bit-identical to what was set"""
    g = _Gate(hiplib, kind, keys, name)
    x, start = _gate_inputs()
    start = start[:g.tensors]
    top = max(TILE_EDGES)
    want = [g.want(x[b], [s[b] for s in start]) for b in range(top)]          # a stream's step does not depend on n: once
    for n in TILE_EDGES:
        g.set_all(start)
        got = g.step(x[:n])
        pairs = [("out", got, np.stack([want[b][0] for b in range(n)]))]
        pairs += [("state %d" % k, np.stack([g.eng.state(k, b) for b in range(n)]), np.stack([want[b][1][k] for b in range(n)])) for k in range(g.tensors)]
        worst = {what: g.ratio(a, w) for what, a, w in pairs}
        print("stream tiles %s %s n=%d: worst error / bound %.2e (%s)" % (KIND_IDS[GR.GATE_KINDS.index((kind, keys))], name, n, max(worst.values()),
                                                                          ", ".join("%s %.2e" % kv for kv in worst.items())))
        for what, a, w in pairs:
            per_stream = [g.ratio(a[b:b + 1], w[b:b + 1]) for b in range(n)] if not g.fp32 else None
            assert (worst[what] < 1.0) if g.fp32 else (worst[what] <= 1.0), (what, n, worst[what], per_stream and int(np.argmax(per_stream)))
        for k in range(g.tensors):
            for b in range(n, STREAMS):
                assert np.array_equal(g.eng.state(k, b), g.kept(k, start[k][b])), "n = %d moved state %d of stream %d" % (n, k, b)
    g.eng.close()


PLACES = ((1, 0), (17, 16), (33, 32), (65, 64))          # (n, stream): NT = 1; the second tile of NT = 2; the second and third block rows, the tile behind empty


@pytest.mark.parametrize("name", DTYPES)
@pytest.mark.parametrize("kind,keys", GR.GATE_KINDS, ids=KIND_IDS)
def test_a_streams_step_does_not_depend_on_its_place(hiplib, kind, keys, name):
    """the K order of one stream's sums depends on neither NT, blockIdx.y nor the lane: the same (x row, state) in stream 0 of an n = 1 call, stream
    16 of n = 17, stream 32 of n = 33 and stream 64 of n = 65, among other streams' values, gives the same output and states bit for bit"""
    g = _Gate(hiplib, kind, keys, name)
    x, start = _gate_inputs()
    start = start[:g.tensors]
    rng = np.random.default_rng(7)
    xp = rng.normal(0, 1, INPUTS).astype(np.float32)
    sp = [rng.uniform(-0.9, 0.9, UNITS).astype(np.float32) for _ in range(g.tensors)]
    seen = []
    for n, at in PLACES:
        g.set_all(start)
        for k in range(g.tensors):
            g.eng.set_state(k, at, sp[k])
        rows = x[:n].copy(); rows[at] = xp
        out = g.step(rows)
        seen.append([out[at].copy()] + [g.eng.state(k, at).copy() for k in range(g.tensors)])
    want_out, want_states = g.want(xp, sp)
    assert g.ratio(seen[0][0], want_out) <= 1.0 and seen[0][0].any()
    for (n, at), tensors in zip(PLACES[1:], seen[1:]):
        for j, (a, b) in enumerate(zip(seen[0], tensors)):
            assert np.array_equal(a, b), "%s of stream %d of n = %d differs from stream 0 of n = 1 in %d values" % ("output" if j == 0 else "state %d" % (j - 1), at, n, int((a != b).sum()))
    g.eng.close()


# ---- B: a whole vector network at ragged stream counts ----
def _vec_weights():
    return IO.synth_weights(IO.parse_cfg(CH._VEC), seed=37)


def _zero_from(eng, n):
    return all(not eng.state(k, b).any() for k in range(eng.num_state_tensors) for b in range(n, STREAMS))


@pytest.mark.parametrize("n", [17, 33, 65])
@pytest.mark.parametrize("name", DTYPES)
def test_vector_network_at_ragged_stream_counts(hiplib, name, n):
    """rnn_bn 24 -> gru 20 -> lstm 12 -> connected 37 (a one-pixel conv whose GEMM M is the stream count) -> softmax, three steps of rows of their
    own per stream and step: every layer of every stream at every step against the restatement stepped per stream -- 5e-4 of the tensor's scale in
    fp32, TOL16 in 16 bit (test_forward_vectors_against_float64's) -- and the states of the streams from n on stay zero"""
    dtype, store = _dtype(hiplib, name)
    cfg = CH._VEC; flat = _vec_weights()
    x = np.random.default_rng(n).normal(0, 1, (3, n, GC.N)).astype(np.float32)
    eng = GC._engine(hiplib, cfg, flat, dtype, batch=STREAMS, keep=True)
    ref = CH.CharNet(cfg, flat, store)
    carried = [dict() for _ in range(n)]          # one restatement, each stream's own state
    layers = CH.compared_layers(cfg)
    worst = [0.0] * len(layers)
    for t in range(3):
        probs = eng.forward_vectors(x[t])
        got = [eng.layer_output(i, n).reshape(n, -1) for i in layers]
        assert np.array_equal(probs, got[-1])
        for b in range(n):
            ref.state = carried[b]
            want = ref.step(x[t, b])
            for j, i in enumerate(layers):
                r = RH.standoff(got[j][b], want[i])
                worst[j] = max(worst[j], r)
                assert r < (5e-4 if store is None else TOL16[name]), "step %d stream %d layer %d: %g" % (t, b, i, r)
        assert _zero_from(eng, n), "step %d" % t
    print("vector network %s n=%d: worst stand-off per layer %s" % (name, n, " ".join("%.3e" % w for w in worst)))
    assert all(eng.state(k, b).any() for k in range(eng.num_state_tensors) for b in range(n))
    eng.close()


# ---- C: yolo_sequence over many streams ----
@pytest.mark.parametrize("n", [33, 65])
@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_sequence_over_many_streams(hiplib, name, n):
    """a 4-token seed of its own per stream, 12 steps, 9 x n uniforms: every token is the numpy sampler's over the device's own row and uniform;
    forcing the device's tokens reproduces its probabilities bit for bit; the last stream, fed what stream 0 is fed, does what stream 0 does; at
    n = 33 twelve steps equal five then seven; a call over the first 17 streams leaves every state of every other stream as it was"""
    dtype, _ = _dtype(hiplib, name)
    rng = np.random.default_rng(100 + n)
    seed = rng.integers(0, GC.N, (4, n)).astype(np.int32)
    u = rng.uniform(0, 1, (9, n)).astype(np.float32)
    seed[:, n - 1] = seed[:, 0]; u[:, n - 1] = u[:, 0]          # the last stream, alone in its block row, is fed what stream 0 is fed
    eng = GC._engine(hiplib, CH._VEC, _vec_weights(), dtype, batch=STREAMS)
    toks, probs = eng.sequence(seed, 12, uniforms=u, clip=CH.CLIP, want_probs=True)
    assert toks.shape == (9, n) and probs.shape == (12, n, GC.N)
    # ... and so does what stream 0 does, at every step (self-consistency alone would pass a stream whose state never moved)
    assert np.array_equal(toks[:, n - 1], toks[:, 0]) and np.array_equal(probs[:, n - 1], probs[:, 0]) and not np.array_equal(probs[:, 1], probs[:, 0])
    for k in range(9):
        for b in range(n):
            assert int(toks[k, b]) == CH.sample_np(probs[3 + k, b], u[k, b]), (k, b)
    assert len(set(toks.reshape(-1).tolist())) > 8 and _zero_from(eng, n)
    eng.reset_state()
    _, again = eng.sequence(np.concatenate([seed, toks[:-1]]), 12, want_probs=True)
    assert np.array_equal(again, probs)
    if n == 33:
        eng.reset_state()
        t5, p5 = eng.sequence(seed, 5, uniforms=u[:2], clip=CH.CLIP, want_probs=True)
        t7, p7 = eng.sequence(t5[-1:], 7, uniforms=u[2:], clip=CH.CLIP, want_probs=True)
        assert np.array_equal(np.concatenate([t5, t7]), toks) and np.array_equal(np.concatenate([p5, p7]), probs)
    before = _all_states(eng)
    eng.sequence(seed[:, :17], 4)
    after = _all_states(eng)
    for k in range(eng.num_state_tensors):
        for b in range(STREAMS):
            assert np.array_equal(before[k][b], after[k][b]) == (b >= 17), (k, b)
    eng.close()


# ---- D: rows wider than one block of granules ----
@pytest.mark.parametrize("n", CH.WIDE_N)
@pytest.mark.parametrize("name", DTYPES)
def test_forward_vectors_over_wide_rows(hiplib, name, n):
    """[lstm] 16 -> [connected] N -> [softmax] over rows of N = 2085 (261 granules, the last one ragged) and 8192 values, non-zero up to element N - 1:
    against float64 under the bounds of the whole-network test; a row that differs from another only from element 2048 on gives another [lstm] output
    (the second block of k_vector_in is read)"""
    dtype, store = _dtype(hiplib, name)
    cfg = CH.wide_cfg(n); flat = IO.synth_weights(IO.parse_cfg(cfg), seed=n)
    x = np.random.default_rng(n).normal(0, 1, (3, n)).astype(np.float32)
    x[1, :CH.BLOCK] = x[0, :CH.BLOCK]
    assert x[:, -1].all() and x[:, CH.BLOCK:].all() and not np.array_equal(x[0], x[1])
    eng = GC._engine(hiplib, cfg, flat, dtype, batch=3, keep=True)
    assert eng.vector_inputs == n
    probs = eng.forward_vectors(x)
    got = [eng.layer_output(i, 3).reshape(3, -1) for i in range(3)]
    assert probs.shape == (3, n) and np.array_equal(probs, got[2])
    for b in range(3):
        want = CH.CharNet(cfg, flat, store).step(x[b])
        for i in range(3):
            r = RH.standoff(got[i][b], want[i])
            print("wide rows N=%d %s stream %d layer %d: %.3e" % (n, name, b, i, r))
            assert r < (5e-4 if store is None else TOL16[name]), (b, i, r)
    assert not np.array_equal(got[0][0], got[0][1])
    eng.close()


@pytest.mark.parametrize("n", CH.WIDE_N)
@pytest.mark.parametrize("name", DTYPES)
def test_free_running_over_wide_rows_is_self_consistent(hiplib, name, n):
    """one forced token, ten sampled steps, three streams: every token is the numpy sampler's over the device's own row; forcing the device's tokens
    (rows written by k_token_in) reproduces the probabilities of the free run (rows written by the sampler) bit for bit.  That says something about
    the granules past element 2048 only if tokens were drawn there: the conditions test_char_rnn_host.py shows for the restatement are asserted
    here of the device's tokens"""
    dtype, _ = _dtype(hiplib, name)
    cfg = CH.wide_cfg(n); flat = IO.synth_weights(IO.parse_cfg(cfg), seed=n)
    seed, u = CH.wide_seed(n), CH.WIDE_U
    eng = GC._engine(hiplib, cfg, flat, dtype, batch=3)
    toks, probs = eng.sequence(seed, 10, uniforms=u, clip=CH.CLIP, want_probs=True)
    assert toks.shape == (10, 3) and probs.shape == (10, 3, n)
    print("wide rows N=%d %s tokens: %s" % (n, name, toks.T.tolist()))
    assert CH.wide_coverage(toks, u, n) == []
    for k in range(10):
        for b in range(3):
            assert int(toks[k, b]) == CH.sample_np(probs[k, b], u[k, b]), (k, b)
    eng.reset_state()
    _, again = eng.sequence(np.concatenate([seed, toks[:-1]]), 10, want_probs=True)
    assert np.array_equal(again, probs)
    eng.close()


# ---- E: the sampler over many rows ----
@pytest.mark.parametrize("rows,ln", [(257, 37), (64, 8192)])
def test_op_sample_over_many_rows(hiplib, rows, ln):
    """one workgroup per row: 257 rows of 37 and 64 rows of 8192, uniforms of their own per row, 0 and the largest float below 1 among them, against
    the numpy sampler exactly"""
    rng = np.random.default_rng(rows)
    probs = GC._rows(rng, rows, ln)
    u = rng.uniform(0, 1, rows).astype(np.float32)
    u[0] = u[rows // 2] = 0.0
    u[1] = u[rows - 1] = CH.LAST_U
    got = hiplib.op_sample(probs, u, clip=CH.CLIP)
    want = [CH.sample_np(probs[b], u[b]) for b in range(rows)]
    assert got.tolist() == want
    assert len(set(want)) > 8 and want[0] == 0


# ---- F: a device-resident token outside the row ----
@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_device_token_outside_the_row_is_a_row_of_zeros(hiplib, name):
    """loc = device, one forced step, tokens [5, N, -1] (the host path refuses such a token; a device buffer is not read before the launch): streams 1
    and 2 give the probabilities and states forward_vectors gives over an all-zero row from the same states, stream 0 those of one_hot(5)"""
    import torch
    dtype, _ = _dtype(hiplib, name)
    N = GC.N
    eng = GC._engine(hiplib, CH._VEC, _vec_weights(), dtype, batch=3)
    eng.forward_vectors(np.random.default_rng(6).normal(0, 1, (3, N)).astype(np.float32))          # a start state that is not zero
    start = GC._states(eng, 3)
    assert all(s.any() for k in start for s in k)
    tok = torch.tensor([5, N, -1], dtype=torch.int32).cuda(); probs = torch.zeros((1, 3, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = eng.lib.yolo_sequence(eng.ctx, 3, 1, tok.data_ptr(), 1, None, float(CH.CLIP), None, probs.data_ptr(), hiplib.DEVICE)
    assert rc == 0, eng.lib.yolo_last_error(eng.ctx).decode()
    eng.synchronize()
    got_p, got_s = probs.cpu().numpy()[0], GC._states(eng, 3)
    for k in range(eng.num_state_tensors):
        for b in range(3):
            eng.set_state(k, b, start[k][b])
    assert GC._same_states(GC._states(eng, 3), start)
    rows = np.stack([CH.one_hot(5, N), np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)])
    want_p = eng.forward_vectors(rows)
    assert np.array_equal(got_p, want_p) and GC._same_states(got_s, GC._states(eng, 3))
    assert not np.array_equal(got_p[0], got_p[1]) and not np.array_equal(got_p[1], got_p[2])          # (the streams' states differ)
    eng.close()
