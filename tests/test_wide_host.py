"""Dense [convolutional] sections of any size 1..11, host side (no device): the planner's acceptance in bf16, fp16 and fp32 with the layer
geometry it derives (tests/golden/mini_wide.npz's cfg and cfg/zoo/alexnet.cfg), its refusals -- the fp8 configuration's old message
verbatim, split fp16 and the sizes outside 1..11 with a message that names the layer --, and the float64 restatement the GPU tests
(test_gpu_wide.py) compare the device against, checked here against the compiled reference's recorded layer outputs."""
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import hip, darknet_io as IO
import test_grouped_host as GH

UNSUPPORTED = -6          # YOLO_ERR_UNSUPPORTED (include/yolo_hip.h)
DTYPES = [hip.BF16, hip.FP16, hip.FP32]


def _mini():
    return str(golden("mini_wide.npz")["cfg"])


def _dump_rows(cfg, dtype):
    rc, text = hip.plan_dump(cfg, dtype=dtype, max_batch=3)
    assert rc == 0, text
    rows = {}
    for line in text.splitlines():
        if line.startswith("layer "):
            f = line.split()
            rows[int(f[1])] = dict([("kind", f[2])] + [kv.split("=", 1) for kv in f[3:] if "=" in kv])
    return rows, text


def _weights_count(text):
    return int(next(l for l in text.splitlines() if "weights_count" in l).split("weights_count")[1].replace("=", " ").split()[0])


# ---- the planner ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_mini_wide_plans_with_its_geometry(dtype):
    cfg = _mini()
    rc, table = hip.plan_table(cfg, dtype=dtype, max_batch=3)
    assert rc == 0, table
    rows, text = _dump_rows(cfg, dtype)
    hwc = [(int(rows[i]["H"]), int(rows[i]["W"]), int(rows[i]["C"])) for i in range(len(rows))]
    #            11x11/4 p0   5x5         7x7         shortcut    6x6/2 p3    2x2 p0     9x9 p4      route       1x1         avgpool     softmax
    assert hwc == [(7, 9, 16), (7, 9, 16), (7, 9, 16), (7, 9, 16), (4, 5, 24), (3, 4, 8), (3, 4, 16), (3, 4, 24), (3, 4, 10), (1, 1, 10), (1, 1, 10)]
    assert [(rows[i]["size"], rows[i]["stride"], rows[i]["pad"]) for i in (0, 1, 2, 4, 5, 6)] == [("11", "4", "0"), ("5", "1", "2"), ("7", "1", "3"), ("6", "2", "3"), ("2", "1", "0"), ("9", "1", "4")]
    assert all(rows[i]["kind"] == "convolutional" and rows[i]["s2d7"] == "0" for i in (0, 1, 2, 4, 5, 6, 8))
    secs = IO.parse_cfg(cfg)
    assert _weights_count(text) == IO.weights_count(secs) == golden("mini_wide.npz")["weights"].size
    # the 9x9 and the 2x2 conv write windows of the [route]'s buffer
    trow = table.splitlines(); st = lambda i: next(v for v in trow[i].split() if v.startswith("storage="))
    assert st(5) == st(6) == st(7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_alexnet_plans_with_its_geometry(dtype):
    cfg = IO.cfg_text("alexnet")
    rc, table = hip.plan_table(cfg, dtype=dtype, max_batch=2)
    assert rc == 0, table
    rows, text = _dump_rows(cfg, dtype)
    hw = [(rows[i]["kind"], int(rows[i]["H"]), int(rows[i]["W"]), int(rows[i]["C"])) for i in range(8)]
    assert hw == [("convolutional", 55, 55, 96), ("maxpool", 27, 27, 96), ("convolutional", 27, 27, 256), ("maxpool", 13, 13, 256),
                  ("convolutional", 13, 13, 384), ("convolutional", 13, 13, 384), ("convolutional", 13, 13, 256), ("maxpool", 6, 6, 256)]
    assert (rows[0]["size"], rows[0]["stride"], rows[0]["pad"]) == ("11", "4", "0") and (rows[2]["size"], rows[2]["pad"]) == ("5", "2")
    assert [int(rows[i]["C"]) for i in (8, 10, 12, 13)] == [4096, 4096, 1000, 1000] and rows[13]["kind"] == "softmax"
    # the stream: five convs with bias, three [connected] layers
    want = (96 + 96 * 3 * 121) + (256 + 256 * 96 * 25) + (384 + 384 * 256 * 9) + (384 + 384 * 384 * 9) + (256 + 256 * 384 * 9) + \
           (4096 + 4096 * 9216) + (4096 + 4096 * 4096) + (1000 + 1000 * 4096)
    assert _weights_count(text) == want == IO.weights_count(IO.parse_cfg(cfg))


def test_fp8_keeps_its_refusal_verbatim():
    for cfg, size in ((_mini(), 11), (IO.cfg_text("alexnet"), 11)):
        rc, msg = hip.plan_check(cfg, dtype=hip.FP8)
        assert rc == UNSUPPORTED and msg == "layer 0: conv size %d unsupported on the device path" % size, msg
    # every size other than 1 and 3, the ones outside the served range included
    net = "[net]\nwidth=16\nheight=16\nchannels=3\n\n[convolutional]\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"
    for size in (0, 2, 5, 12):
        rc, msg = hip.plan_check(net + "[convolutional]\nfilters=8\nsize=%d\nstride=1\npad=1\nactivation=leaky\n" % size, dtype=hip.FP8)
        assert rc == UNSUPPORTED and msg == "layer 1: conv size %d unsupported on the device path" % size, msg


def test_refusals_name_the_layer_and_the_range():
    cfg = _mini()
    rc, msg = hip.plan_check(cfg, dtype=hip.FP16X2)
    assert rc == UNSUPPORTED and "layer 0" in msg and "size 11" in msg and "split-fp16" in msg, msg
    msgs = [msg]
    for size in (12, 0):
        for dtype in DTYPES:
            rc, msg = hip.plan_check(cfg.replace("size=9\n", "size=%d\n" % size), dtype=dtype)
            assert rc == UNSUPPORTED and "layer 6" in msg and "size %d" % size in msg and "1..11" in msg, msg
        msgs.append(msg)
    assert len(set(msgs)) == 3
    # every size in between plans, at any position, on an odd extent, with pad=1 and with padding=0
    net = "[net]\nwidth=29\nheight=23\nchannels=3\n\n"
    for size in range(1, 12):
        for pad in ("pad=1", "padding=0"):
            body = "".join("[convolutional]\nbatch_normalize=1\nfilters=8\nsize=%d\nstride=%d\n%s\nactivation=leaky\n\n" % (size, s, pad) for s in (2, 1)) + "[avgpool]\n\n[softmax]\n"
            for dtype in DTYPES:
                rc, msg = hip.plan_check(net + body, dtype=dtype)
                fits = pad == "pad=1" or (23 - size) // 2 + 1 >= size          # (padding=0: the second conv must still fit its 23-row input's output)
                assert rc == (0 if fits else -1), (size, pad, msg)


def test_s2d7_keeps_its_plan():
    """the 7x7 / 2 / pad 3 first layer on an even 3-channel image is still the space-to-depth form; on an odd extent it is now a plain conv"""
    net = "[net]\nwidth=%d\nheight=32\nchannels=3\n\n[convolutional]\nbatch_normalize=1\nfilters=16\nsize=7\nstride=2\npad=1\nactivation=leaky\n\n[avgpool]\n\n[softmax]\n"
    rows, _ = _dump_rows(net % 32, hip.BF16)
    assert rows[0]["s2d7"] == "1" and rows[0]["cin_pad"] == "32" and rows[0]["kpad"] == "512"
    rows, _ = _dump_rows(net % 31, hip.BF16)
    assert rows[0]["s2d7"] == "0" and rows[0]["cin_pad"] == "8" and rows[0]["kpad"] == str((49 * 8 + 63) // 64 * 64)


# ---- the fixture against a second derivation ----
def test_restatement_reproduces_every_conv_layer_of_the_fixture():
    """each conv layer of mini_wide.npz from its producer's STORED output: float64 conv (test_grouped_host.gconv_ref with one group),
    darknet's batch norm, the activation -- within 1e-5 of the layer's largest value"""
    g = golden("mini_wide.npz")
    secs = IO.parse_cfg(str(g["cfg"]))
    params = GH.layer_params(secs, g["weights"])
    x0 = g["images_u8"].astype(np.float32) / np.float32(255.0)
    seen = []
    for i, s in enumerate(secs[1:]):
        if s["type"] != "convolutional":
            continue
        prm, w = params[i]
        k, st = int(s["size"]), int(s["stride"])
        pad = k // 2 if int(s.get("pad", 0)) else int(s.get("padding", 0))
        y = GH.gconv_ref(x0 if i == 0 else g["layer_%02d" % (i - 1)], w, None, 1, st, pad)
        if int(s.get("batch_normalize", 0)):
            beta, gamma, mean, var = prm.astype(np.float64)
            y = (y - mean) / (np.sqrt(var) + 1e-6) * gamma + beta
        else:
            y = y + prm[0].astype(np.float64)
        y = GH.ACTS[s["activation"]](y)
        ref = g["layer_%02d" % i]
        assert y.shape == ref.shape
        err = float(np.abs(y - ref).max() / np.abs(ref).max())
        assert err < 1e-5, "layer %d (size %d): %.3e" % (i, k, err)
        seen.append((k, st, pad))
    assert seen == [(11, 4, 0), (5, 1, 2), (7, 1, 3), (6, 2, 3), (2, 1, 0), (9, 1, 4), (1, 1, 0)]
    # the shortcut and the route, exactly
    a = g["layer_02"] + g["layer_01"]
    assert np.array_equal(g["layer_03"], np.where(a > 0, a, (0.1 * a.astype(np.float64)).astype(np.float32)))          # DN/activations.h: .1 * x in double
    assert np.array_equal(g["layer_07"], np.concatenate([g["layer_06"], g["layer_05"]], axis=-1))
    # taps_inside: the count an all-ones conv must give (test_gpu_wide.py), against the closed form on one case
    t = GH.taps_inside(5, 6, 7, 1, 3)
    assert t.shape == (5, 6) and t[0, 0] == 4 * 4 and t[2, 2] == 5 * 6 and t.max() == 30


def test_fixture_margin():
    """the fixture's own claims: logits that reach +-5, and on all three images a top-1 margin above twice the bf16 bound"""
    g = golden("mini_wide.npz")
    n = len(IO.parse_cfg(str(g["cfg"]))) - 1
    pooled = g["layer_%02d" % (n - 2)]
    assert int(g["logit_layer"]) == n - 3 and float(np.abs(g["layer_%02d" % int(g["logit_layer"])]).max()) > 4.5
    top2 = np.sort(pooled, axis=-1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) > 2 * 3e-2 * np.abs(pooled).max()).all()
    assert np.abs(g["layer_%02d" % (n - 1)].sum(axis=-1) - 1).max() < 1e-5
