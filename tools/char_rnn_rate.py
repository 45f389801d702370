#!/usr/bin/env python
"""Token rate of darknet's rnn.cfg shape (tools/make_cfgs.py --char-rnn: 256 symbols, 3 x [rnn] of 1024 units) with seeded weights, bf16, over 1 and
32 streams and 1000 steps (NOTEBOOK, "char-rnn"; profiles/r17_char_rnn_rate.json):

  python tools/char_rnn_rate.py OUT.json

  sequence      one yolo_sequence call: the sampled token is fed back on the device, the host synchronises once at the end
  stepwise      1000 yolo_sequence calls of one step each: the token is still sampled on the device, but comes back to the host after every step
                and is handed to the next call as its forced token
  reference     the compiled reference's network_predict + sample_array loop on the CPU, one stream, where oracle/_ref is present

Each measurement is a process of its own under `timeout`; the first that fails ends the run.  A host clock around calls that end in a device
synchronise, after a warm-up of the same call shape, repeated REPS times: tokens/s = streams * steps / the median of the windows' seconds, the
fastest and the slowest window beside it.  No threshold is asserted."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
STEPS, WARM, REF_STEPS, REPS = 1000, 50, 200, 7
LIMIT = {"sequence": 180, "stepwise": 240, "reference": 300}


def _cfg():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_cfgs", os.path.join(ROOT, "tools", "make_cfgs.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m.char_rnn()


def _weights(cfg):
    """synth_weights(seed 0) with every [rnn] layer's self sublayer (the second of its three: biases, then its rows) damped to a quarter: a leaky
    state fed back through rows of unit gain grows without bound over 1000 steps, and the rate of a network full of Inf is nobody's workload"""
    from yolo_tensorflow_amd import darknet_io as IO
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=0)
    pos = 0
    for r in IO.recurrent_specs(secs):          # (the stream begins with the recurrent layers: nothing with parameters stands in front of them)
        sizes = [IO.connected_floats(i, o, r["bn"]) for i, o in r["subs"]]
        at = pos + sizes[0] + r["outputs"]
        flat[at:at + r["outputs"] * r["outputs"]] *= np.float32(0.25)
        pos += sum(sizes)
    return flat


def _net(streams):
    from yolo_tensorflow_amd import hip, darknet_io as IO
    from yolo_tensorflow_amd.char_rnn import CharRNN
    return CharRNN(_cfg(), _weights(IO.with_vector_input(_cfg())), dtype=hip.BF16, streams=streams)


def _timed(window, tokens):
    """REPS windows -> the result record"""
    secs = []
    for _ in range(REPS):
        t0 = time.perf_counter(); window(); secs.append(time.perf_counter() - t0)
    med = float(np.median(secs))
    return {"tokens_per_s": tokens / med, "tokens_per_s_slowest": tokens / max(secs), "tokens_per_s_fastest": tokens / min(secs), "seconds_median": med, "windows": REPS}


def one(mode, streams):
    rng = np.random.default_rng(0)
    first = rng.integers(0, 256, (1, streams)).astype(np.int32)
    u = rng.uniform(0, 1, (STEPS, streams)).astype(np.float32)
    if mode == "reference":
        import ctypes as C
        from oracle import darknet_ref as D
        from yolo_tensorflow_amd import darknet_io as IO
        cfg = IO.with_vector_input(_cfg())
        net = D.RefNet(cfg, _weights(cfg), 0, 2)
        l = D.lib(); l.sample_array.argtypes = [C.POINTER(C.c_float), C.c_int]; l.sample_array.restype = C.c_int
        x = np.zeros(256, dtype=np.float32); c = int(first[0, 0])
        def run(n):
            nonlocal c
            for _ in range(n):
                x[:] = 0; x[c] = 1
                out = l.network_predict(net.net, x.ctypes.data_as(C.POINTER(C.c_float)))
                c = int(l.sample_array(out, 256))
        run(5)
        res = _timed(lambda: run(REF_STEPS), REF_STEPS)
        net.close()
        return dict(res, steps=REF_STEPS)
    net = _net(streams); eng = net.engine
    if mode == "sequence":
        eng.sequence(first, WARM, uniforms=u[:WARM], clip=net.CLIP)
        eng.synchronize()
        res = _timed(lambda: eng.sequence(first, STEPS, uniforms=u, clip=net.CLIP), streams * STEPS)
    else:
        tok = first
        def run(n):
            nonlocal tok
            for t in range(n):
                tok = eng.sequence(tok, 1, uniforms=u[t:t + 1], clip=net.CLIP)
        run(WARM)
        res = _timed(lambda: run(STEPS), streams * STEPS)
    net.close()
    return dict(res, steps=STEPS, steps_per_s=STEPS / res["seconds_median"])


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        print("RESULT " + json.dumps(one(sys.argv[2], int(sys.argv[3]))))
        return
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    res = {"cfg": "char-rnn (256 symbols, 3 x [rnn] 1024 leaky batch-normalised, [connected] 256, [softmax])", "dtype": "bf16", "weights": "synth seed 0, self sublayers x 0.25"}
    jobs = [(m, s) for s in (1, 32) for m in ("sequence", "stepwise")]
    if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libdarknet_ref.so")):
        jobs.append(("reference", 1))
    for mode, streams in jobs:
        p = subprocess.run(["timeout", "-k", "10", str(LIMIT[mode]), sys.executable, os.path.abspath(__file__), "--one", mode, str(streams)], capture_output=True, text=True)
        line = [q for q in p.stdout.splitlines() if q.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            raise SystemExit("%s over %d streams ended with status %d: nothing further is started" % (mode, streams, p.returncode))
        res["%s_b%d" % (mode, streams) if mode != "reference" else "reference_cpu_b1"] = json.loads(line[0][7:])
        print(mode, streams, line[0][7:], flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
