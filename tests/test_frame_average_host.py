"""Frame averaging (darknet's `detector demo`: remember_network + avg_predictions of DN/examples/demo.c) restated in numpy, and
pinned to the compiled reference: tests/golden/frame_average_cases.npz (tools/make_golden.py --frame-average) holds, per case, the [yolo] /
[region] layers' l.output after every frame and what get_network_boxes returned once l.output was the mean of the last K frames.  The restatement
below -- mean of the activated tensors in SLOT order, get_yolo_box / get_region_box, correct_yolo_boxes -- reproduces those boxes from those tensors
bit for bit, operation for operation in the float / double mix of the reference's build (correct_boxes says where that build departs from the source order).  That pins what the fixture means; tests/test_gpu_frame_average.py
holds the device to the same functions.  No GPU."""
import os
import re
import numpy as np
import pytest
from conftest import golden, ROOT
from yolo_tensorflow_amd import darknet_io as IO

F = np.float32
FIXTURE = "frame_average_cases.npz"


def cases():
    g = golden(FIXTURE)
    return [str(n) for n in g["names"]]


def heads_of(cfg_text):
    """The detection heads of a cfg in file order: kind, grid, anchors as the reference's box functions read them ([yolo]: the masked pairs in
    pixels; [region]: the first `num` pairs, in cells), and the network size."""
    secs = IO.parse_cfg(cfg_text)
    shapes = IO.layer_shapes(secs)
    netw, neth = int(secs[0]["width"]), int(secs[0]["height"])
    out = []
    for s, (t, h, w, _, _) in zip(secs[1:], shapes):
        if t not in ("yolo", "region"):
            continue
        a = np.array([float(v) for v in s["anchors"].split(",")], F).reshape(-1, 2)
        a = a[[int(m) for m in s["mask"].split(",")]] if t == "yolo" else a[:int(s["num"])]
        out.append(dict(kind=t, gh=h, gw=w, na=len(a), classes=int(s["classes"]), anchors=a, netw=netw, neth=neth))
    return out


def planar_to_rows(out, hd):
    """l.output of one image (anchor, attribute, cell: DN/yolo_layer.c entry_index) -> [cell, anchor, attribute]"""
    return np.ascontiguousarray(out.reshape(hd["na"], 5 + hd["classes"], hd["gh"] * hd["gw"]).transpose(2, 0, 1))


def slot_mean(slots):
    """avg_predictions: fill_cpu(0), then axpy_cpu((float)(1. / K), slot j) for j = 0 .. K-1 -- slot order, not age order; fp32, no contraction"""
    alpha = F(1. / len(slots))
    avg = np.zeros_like(slots[0])
    for s in slots:
        avg = avg + alpha * s
    return avg


def ring_means(outputs, K):
    """outputs[t]: one head's activated tensor after frame t.  -> the mean after every step of a ring that starts as zeros (demo()'s calloc)"""
    ring = [np.zeros_like(outputs[0]) for _ in range(K)]
    means = []
    for t, o in enumerate(outputs):
        ring[t % K] = o
        means.append(slot_mean(ring))
    return means


def head_boxes(act, hd):
    """get_yolo_box / get_region_box of every box of one head: act [cell, anchor, attribute] activated values -> (cx, cy, w, h) [cell, anchor, 4],
    normalised.  x, y: float sums and quotients; w, h: exp() in double times the float anchor over the int extent, rounded to float once"""
    gh, gw = hd["gh"], hd["gw"]
    cell = np.arange(gh * gw)
    col, row = (cell % gw).astype(F)[:, None], (cell // gw).astype(F)[:, None]
    b = np.empty(act.shape[:2] + (4,), F)
    b[..., 0] = (col + act[..., 0]) / F(gw)
    b[..., 1] = (row + act[..., 1]) / F(gh)
    dw, dh = (hd["netw"], hd["neth"]) if hd["kind"] == "yolo" else (gw, gh)
    b[..., 2] = (np.exp(act[..., 2].astype(np.float64)) * hd["anchors"][None, :, 0].astype(np.float64) / dw).astype(F)
    b[..., 3] = (np.exp(act[..., 3].astype(np.float64)) * hd["anchors"][None, :, 1].astype(np.float64) / dh).astype(F)
    return b


def correct_boxes(b, w, h, netw, neth, relative, wh_scale=None):
    """correct_yolo_boxes = correct_region_boxes (DN/yolo_layer.c:247-273) over the n boxes of ONE layer, float and double mixed as there.
    wh_scale [relative][2]: how the golden's build of the reference scales w and h, read off its own code and a unit box.  Its -Ofast build (a) forms
    (float)netw / new_w and (float)neth / new_h through a reciprocal estimate and one Newton step (128 / 128 = 0x3f7fffff there): the two factors are
    recorded in wh_scale[1]; (b) with relative = 0 its vector loop, which takes the boxes in pairs up to 2 * ((n - 1) >> 1), multiplies by the ONE
    factor (netw / new_w) * w, while the one or two boxes its scalar tail takes are multiplied twice, in source order.  None: IEEE in source order"""
    if F(netw) / F(w) < F(neth) / F(h):
        new_w, new_h = netw, (h * netw) // w
    else:
        new_h, new_w = neth, (w * neth) // h
    o = np.empty_like(b)
    o[:, 0] = ((b[:, 0].astype(np.float64) - (netw - new_w) / 2. / netw) / np.float64(F(new_w) / F(netw))).astype(F)
    o[:, 1] = ((b[:, 1].astype(np.float64) - (neth - new_h) / 2. / neth) / np.float64(F(new_h) / F(neth))).astype(F)
    sw, sh = (F(netw) / F(new_w), F(neth) / F(new_h)) if wh_scale is None else (F(wh_scale[1][0]), F(wh_scale[1][1]))
    o[:, 2] = b[:, 2] * sw; o[:, 3] = b[:, 3] * sh
    if not relative:
        o[:, 0] *= F(w); o[:, 1] *= F(h)
        paired = 0 if wh_scale is None else 2 * ((len(b) - 1) >> 1)
        o[:paired, 2] = b[:paired, 2] * (sw * F(w)); o[:paired, 3] = b[:paired, 3] * (sh * F(h))
        o[paired:, 2] *= F(w); o[paired:, 3] *= F(h)
    return o


def network_boxes(acts, heads, w, h, relative, thresh=0.0, wh_scale=None):
    """get_network_boxes over the heads' activated tensors (acts[k]: [cell, anchor, attribute]) -> bbox [n, 4], objectness [n], prob [n, classes] in the
    reference's order: a [yolo] head's boxes above thresh, cell by cell, the anchor inner; a [region] head's every box, anchor by anchor"""
    bb, ob, pr = [], [], []
    for act, hd in zip(acts, heads):
        box = head_boxes(act, hd)
        obj, cls = act[..., 4], act[..., 5:]
        if hd["kind"] == "region":
            box, obj, cls = box.transpose(1, 0, 2), obj.T, cls.transpose(1, 0, 2)
            obj = np.where(obj > thresh, obj, F(0))
        box, obj, cls = box.reshape(-1, 4), obj.reshape(-1), cls.reshape(-1, cls.shape[-1])
        prob = obj[:, None] * cls
        prob = np.where(prob > thresh, prob, F(0))
        if hd["kind"] == "yolo":
            keep = obj > thresh
            box, obj, prob = box[keep], obj[keep], prob[keep]
        bb.append(correct_boxes(box, w, h, hd["netw"], hd["neth"], relative, wh_scale)); ob.append(obj); pr.append(prob)
    return np.concatenate(bb), np.concatenate(ob), np.concatenate(pr)


def decoded_rows(acts, heads):
    """The library's decoded tensor [rows, 5 + classes] of one image over activated tensors: per head cell by cell, the anchor inner,
    (cx, cy, w, h) normalised as head_boxes gives them, objectness, classes"""
    return np.concatenate([np.concatenate([head_boxes(a, hd), a[..., 4:]], -1).reshape(-1, a.shape[-1]) for a, hd in zip(acts, heads)])


def case_means(g, name):
    """-> heads, K, steps, means[t][k]: head k's averaged activated tensor [cell, anchor, attribute] after step t"""
    heads = heads_of(str(g[name + "_cfg"]))
    K = int(g[name + "_K"]); steps = len(g[name + "_frames"])
    per_head = [ring_means([planar_to_rows(g["%s_out_t%d_h%d" % (name, t, k)], hd) for t in range(steps)], K) for k, hd in enumerate(heads)]
    return heads, K, steps, [[per_head[k][t] for k in range(len(heads))] for t in range(steps)]


@pytest.mark.parametrize("name", cases())
def test_restatement_reproduces_the_reference_boxes(name):
    g = golden(FIXTURE)
    heads, K, steps, means = case_means(g, name)
    assert steps >= K + 2                                          # the ring wraps
    w, h = (int(v) for v in g[name + "_src_wh"])
    # the recorded factors are the IEEE quotients to within one unit in the last place, and a lone box is scaled twice (relative = 0)
    scale = g[name + "_wh_scale"]
    assert np.abs(scale[1] / correct_boxes(np.ones((1, 4), F), w, h, heads[0]["netw"], heads[0]["neth"], 1)[0, 2:] - 1).max() < 2e-7
    assert np.array_equal(scale[0], scale[1] * np.array([w, h], F))
    assert w != h
    for t in range(steps):
        for relative in (1, 0):
            bb, obj, prob = network_boxes(means[t], heads, w, h, relative, wh_scale=g[name + "_wh_scale"])
            ref = g["%s_bbox_t%d_rel%d" % (name, t, relative)]
            assert np.array_equal(bb, ref), (t, relative)
        assert np.array_equal(obj, g["%s_obj_t%d" % (name, t)]) and np.array_equal(prob, g["%s_prob_t%d" % (name, t)]), t
        assert len(obj) == sum(hd["gh"] * hd["gw"] * hd["na"] for hd in heads)      # thresh 0: every box


@pytest.mark.parametrize("name", cases())
def test_fixture_shows_the_averaging(name):
    """The first K - 1 steps are attenuated by the empty slots, and later the mean differs from the single frame by far more than any tolerance"""
    g = golden(FIXTURE)
    heads, K, steps, means = case_means(g, name)
    single = [planar_to_rows(g["%s_out_t%d_h0" % (name, t)], heads[0]) for t in range(steps)]
    assert np.array_equal(means[0][0], slot_mean([single[0]] + [np.zeros_like(single[0])] * (K - 1)))
    assert means[0][0][..., 4].max() <= 1.0 / K + 1e-6
    assert np.abs(means[steps - 1][0][..., 4] - single[steps - 1][..., 4]).max() > 0.02          # ten times the GPU test's objectness tolerance
    # slot order is not age order: after the wrap the newest frame sits in slot (steps - 1) % K
    last = [single[t] for t in range(steps - K, steps)]
    by_slot = sorted(range(steps - K, steps), key=lambda t: t % K)
    assert np.array_equal(means[steps - 1][0], slot_mean([single[t] for t in by_slot]))
    assert len(last) == K


def test_symbols_are_exported_and_declared():
    from yolo_tensorflow_amd import hip
    header = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    assert re.search(r"int\s+yolo_set_frame_average\s*\(\s*yolo_ctx\s*\*\s*ctx\s*,\s*int\s+frames\s*\)\s*;", header)
    assert re.search(r"int\s+yolo_frame_average\s*\(\s*const\s+yolo_ctx\s*\*\s*ctx\s*\)\s*;", header)
    assert "yolo_set_frame_average" in hip.EXPORTS and "yolo_frame_average" in hip.EXPORTS
    lib = hip.load_library()
    assert hasattr(lib, "yolo_set_frame_average") and hasattr(lib, "yolo_frame_average")
    assert hasattr(hip.Engine, "set_frame_average") and hasattr(hip.Engine, "frame_average")
