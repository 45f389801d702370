#!/usr/bin/env python3
"""Generate the committed golden vectors under tests/golden/ FROM THE REFERENCE ITSELF.

Runs only in the build container (it reads /root/reference and oracle/_ref); the outputs are small
`.npz` data files (inputs + expected outputs), never reference source text.

  nms_v3_numpy.npz   inputs/outputs of the reference's numpy `non_max_suppression` + `_iou`
                     (V3/yolo_v3.py:350-420), imported with stub `tensorflow` modules
  v2_postprocess.npz inputs/outputs of V2 `postprocess` / `bboxes_iou` (V2/utils.py:30-187), imported
                     with stub `cv2` (and np.bool shim)
  mini_v3.npz / mini_v2.npz
                     a small darknet topology covering every hot-path layer type, its synthetic weights,
                     an input image, EVERY layer output, and the boxes after get_network_boxes /
                     do_nms_sort -- produced by the reference's own C code compiled CPU-only
                     (oracle/Makefile -> oracle/_ref/libdarknet_ref.so)
  mini_resnet.npz / mini_resnet_30.npz
                    a ResNet in miniature (general [shortcut] forms, activations outside the slope family) at 32 x 32 and 30 x 30:
                    three images each, every layer's output from the compiled reference
  mini_grouped.npz / mini_dw_v3.npz
                    [convolutional] sections with groups= (ResNeXt-style bottlenecks, depthwise and pointwise pairs, a grouped 5x5, a
                    grouped class conv): a classifier with three images and every layer's output, and a two-head depthwise-separable
                    [yolo] detector with its boxes, from the compiled reference
  mini_cls53.npz / mini_cls19.npz
                     two small classifier topologies ([avgpool], [softmax], [cost]; darknet-53's and darknet-19's tail order), every
                     layer output and the probability vector, from the same compiled reference
  mini_v3_rect.npz / mini_v2_rect.npz / mini_cls_rect.npz / mini_v3_rect_letterbox.npz
                     the minis at width != height (64 high x 96 wide, 96 x 64, 64 x 96): layers and boxes as above; the letterbox file holds
                     the reference's own letterbox_image of three source images and its corrected boxes at each image's size
  mini_edges.npz
                    the layers that move data and the dense conv's geometry keys at ragged channel counts (a map network, 15 high x 22
                    wide: pad=0, padding=2, stride 3, five max-pool geometries, reorg, a concatenation at channel offset 20): three
                    images, every layer's output from the compiled reference; written with fixed member dates, so it regenerates byte for byte
  mini_seq.npz / mini_crnn.npz
                    recurrent networks ([rnn], [gru], [lstm] behind a conv stack, a classifier; two [crnn] layers in front of a [yolo] head):
                    ONE live network of the compiled reference over 5 frames, every layer's output after each frame (mini_crnn: the boxes too), and
                    drift16_*: the stand-off of the 16-bit-rounded host restatement (tests/test_recurrent_host.py) per frame and layer
  mini_planes_grey.npz / mini_planes_rgbd.npz / mini_planes_nine.npz / mini_planes_17.npz / planes_fit_cases.npz
                    image networks of 1, 4, 9 and 17 planes (darknet's own cfg text, no yolo_input key), each opening with the shape of one fused first-stage
                    kernel of the RGB path: one image, every layer's output (the grey one: get_network_boxes too); letterbox_image and resize_min +
                    crop_image of images of 1, 4 and 9 planes; fixed member dates
  mini_lrn.npz / lrn_crop_cases.npz
                    [crop] and [normalization]: a classifier that opens with a [crop] and has two LRN layers (three images, every layer), eleven
                    stand-alone [normalization] shapes behind a 1x1 conv, four [crop] networks, and six uint8 images through the reference's
                    resize_min + crop_image (the classifier's validation preprocessing); fixed member dates
  frame_average_cases.npz   (--frame-average)
                    darknet's `detector demo` averaging (DN/examples/demo.c remember_network + avg_predictions) on three small detectors: per case
                    cfg, weight seed, K, K + 2 uint8 frames, every [yolo] / [region] layer's l.output after each frame, and get_network_boxes of
                    the compiled reference over the mean of the last K outputs (written back into l.output) after every step; fixed member dates
  mini_v1_edges.npz / mini_v1_stem.npz   (v1_edges)
                    the YOLOv1 family at its kernels' edges: three [local] layers (72 granules per filter row, 13 filters, stride 2 under padding, tanh), two
                    [connected] layers (the default logistic, K = 48) and [detection] with num=3, sqrt=0 on a 6 x 10 input; a 7x7 / 2 conv on 10 x 14,
                    a [connected] over 5 x 7 x 8 and [detection] with side=1: three images, every layer, get_network_boxes per image; fixed member dates
  mini_xnor.npz / xnor_layer_cases.npz   (--xnor)
                    XNOR-Net layers ([convolutional] with xnor=1, DN/convolutional_layer.c:28-49, 451-485): a [yolo] detector with xnor=1 on every conv but
                    the first and the last two (one image, every layer's output, get_network_boxes), and a classifier whose xnor layers differ in shape (a
                    5x5 with padding=1, a stride-2 3x3 with a bias, a 1x1 with tanh); the weight seed is the first at which no value entering an xnor
                    layer is non-zero and within 5e-4 of its tensor's largest value of zero; fixed member dates
  yolov3_bn_real.npz / yolov2_bn_real.npz
                     the COMPLETE batch-norm vectors (beta, gamma, rolling mean, rolling variance) of every
                     batch-normalised conv of yolov3.weights / yolov2.weights, and the first l.n filter
                     values of every conv, as the reference's own load_convolutional_weights printed them
                     (DN/parser.c:1176-1228) into D2T/log.txt:224-949 / :1-222 -- numbers, not source
"""
import os
import sys
import types
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")

MINI_V3 = """[net]
batch=1
width=64
height=64
channels=3

[convolutional]
batch_normalize=1
filters=8
size=3
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=16
size=3
stride=2
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=8
size=1
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=16
size=3
stride=1
pad=1
activation=leaky

[shortcut]
from=-3
activation=linear

[convolutional]
batch_normalize=1
filters=32
size=3
stride=2
pad=1
activation=leaky

[maxpool]
size=2
stride=2

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=1

[convolutional]
batch_normalize=1
filters=16
size=1
stride=1
pad=1
activation=leaky

[convolutional]
size=1
stride=1
pad=1
filters=27
activation=linear

[yolo]
mask=3,4,5
anchors=4,5,  8,6,  10,14,  20,18,  30,40,  50,44
classes=4
num=6

[route]
layers=-3

[convolutional]
batch_normalize=1
filters=8
size=1
stride=1
pad=1
activation=leaky

[upsample]
stride=2

[route]
layers=-1,5

[convolutional]
batch_normalize=1
filters=24
size=3
stride=1
pad=1
activation=leaky

[convolutional]
size=1
stride=1
pad=1
filters=27
activation=linear

[yolo]
mask=0,1,2
anchors=4,5,  8,6,  10,14,  20,18,  30,40,  50,44
classes=4
num=6
"""

MINI_V2 = """[net]
batch=1
width=64
height=64
channels=3

[convolutional]
batch_normalize=1
filters=8
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=2

[convolutional]
batch_normalize=1
filters=16
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=2

[convolutional]
batch_normalize=1
filters=16
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=2

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky

[route]
layers=-4

[convolutional]
batch_normalize=1
filters=8
size=1
stride=1
pad=1
activation=leaky

[reorg]
stride=2

[route]
layers=-1,-4

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky

[convolutional]
size=1
stride=1
pad=1
filters=30
activation=linear

[region]
anchors=0.6,0.7,  1.9,2.1,  3.3,5.5
bias_match=1
classes=5
coords=4
num=3
softmax=1
"""


def stub_modules():
    tf = types.ModuleType("tensorflow")
    contrib = types.ModuleType("tensorflow.contrib")
    slim = types.ModuleType("tensorflow.contrib.slim")
    fw = types.ModuleType("tensorflow.contrib.framework")
    fw.add_arg_scope = lambda f: f
    contrib.slim = slim; contrib.framework = fw; tf.contrib = contrib
    sys.modules.update({"tensorflow": tf, "tensorflow.contrib": contrib, "tensorflow.contrib.slim": slim,
                        "tensorflow.contrib.framework": fw, "cv2": types.ModuleType("cv2")})
    if not hasattr(np, "bool"):
        np.bool = bool


def planted_detections(rng, n_img, rows, classes, clusters=6, per=7, size=416.0):
    """[n,rows,5+C] with clusters of jittered boxes (corners, pixels) so NMS has real work."""
    det = np.zeros((n_img, rows, 5 + classes), dtype=np.float32)
    det[..., :4] = rng.uniform(0, size, (n_img, rows, 4)).astype(np.float32)
    det[..., 4] = rng.uniform(0.0, 0.3, (n_img, rows)).astype(np.float32)
    det[..., 5:] = rng.uniform(0.01, 1, (n_img, rows, classes)).astype(np.float32)
    for b in range(n_img):
        r = 0
        for c in range(clusters):
            cx, cy = rng.uniform(60, size - 60, 2); w, h = rng.uniform(30, 120, 2)
            cls = int(rng.integers(0, classes))
            for _ in range(per):
                j = rng.normal(0, 6, 4)
                det[b, r, :4] = [cx - w / 2 + j[0], cy - h / 2 + j[1], cx + w / 2 + j[2], cy + h / 2 + j[3]]
                det[b, r, 4] = rng.uniform(0.55, 0.999)
                det[b, r, 5:] = rng.uniform(0.01, 0.3, classes); det[b, r, 5 + cls] = rng.uniform(0.7, 1.0)
                r += 1
    perm = rng.permutation(rows)
    return det[:, perm]


def gen_nms_v3():
    sys.path.insert(0, os.path.join(REF, "YOLO_V3", "YOLOv3-Tensorflow-detect-export"))
    import yolo_v3 as ref
    rng = np.random.default_rng(2)
    det = planted_detections(rng, 2, 300, 6)
    res = ref.non_max_suppression(det, confidence_threshold=0.5, iou_threshold=0.4)
    keys = sorted(res.keys())
    boxes = [np.array([b for b, _ in res[k]], dtype=np.float32) for k in keys]
    scores = [np.array([s for _, s in res[k]], dtype=np.float32) for k in keys]
    pairs = rng.uniform(0, 100, (64, 2, 4)).astype(np.float32)
    ious = np.array([ref._iou(p[0], p[1]) for p in pairs], dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "nms_v3_numpy.npz"), det=det, conf=0.5, iou=0.4, classes=np.array(keys),
                        counts=np.array([len(b) for b in boxes]), boxes=np.concatenate(boxes), scores=np.concatenate(scores),
                        pairs=pairs, pair_ious=ious)
    print("nms_v3_numpy:", {int(k): len(res[k]) for k in keys})


def gen_v2_post():
    sys.path.insert(0, os.path.join(REF, "YOLO_V2", "YOLOv2-Tensorflow-detect-export"))
    cwd = os.getcwd()
    os.chdir(os.path.join(REF, "YOLO_V2", "YOLOv2-Tensorflow-detect-export"))   # config.py reads ./yolo2_data at import
    import utils as ref
    os.chdir(cwd)
    rng = np.random.default_rng(3)
    n = 13 * 13 * 5
    # normalised corner boxes with planted overlapping clusters
    cx = rng.uniform(0.1, 0.9, n); cy = rng.uniform(0.1, 0.9, n); w = rng.uniform(0.02, 0.5, n); h = rng.uniform(0.02, 0.5, n)
    for c in range(8):
        base = c * 9
        cx[base:base + 9] = cx[base] + rng.normal(0, .01, 9); cy[base:base + 9] = cy[base] + rng.normal(0, .01, 9)
        w[base:base + 9] = w[base] + rng.normal(0, .01, 9); h[base:base + 9] = h[base] + rng.normal(0, .01, 9)
    bboxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32).reshape(1, 169, 5, 4)
    obj = rng.uniform(0, 0.4, n).astype(np.float32); obj[:72] = rng.uniform(0.7, 1, 72)
    cls = rng.dirichlet(np.ones(80) * 0.05, n).astype(np.float32)
    for c in range(8):
        v = rng.uniform(0.0, 0.01, 80); v[int(rng.integers(0, 80))] = 0.9
        cls[c * 9:(c + 1) * 9] = (v / v.sum()).astype(np.float32)
    # two overlapping clusters of DIFFERENT classes must both survive (V2/utils.py:183)
    cx[72:81] = cx[0] + rng.normal(0, .01, 9); cy[72:81] = cy[0] + rng.normal(0, .01, 9)
    w[72:81] = w[0]; h[72:81] = h[0]; obj[72:81] = rng.uniform(0.7, 1, 9)
    v = rng.uniform(0.0, 0.01, 80); v[(int(np.argmax(cls[0])) + 1) % 80] = 0.9
    cls[72:81] = (v / v.sum()).astype(np.float32)
    bboxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32).reshape(1, 169, 5, 4)
    out_b, out_s, out_c = ref.postprocess(bboxes.copy(), obj.reshape(1, 169, 5).copy(), cls.reshape(1, 169, 5, 80).copy(),
                                          image_shape=(576, 768), threshold=0.5)
    ib = rng.integers(0, 400, (40, 4)).astype(np.int32); ib[:, 2:] += ib[:, :2]
    with np.errstate(all="ignore"):
        pair_iou = ref.bboxes_iou(ib[0], ib[1:])
    np.savez_compressed(os.path.join(OUT, "v2_postprocess.npz"), bboxes=bboxes, obj=obj.reshape(1, 169, 5),
                        cls=cls.reshape(1, 169, 5, 80), image_shape=np.array([576, 768]), threshold=0.5,
                        out_boxes=out_b, out_scores=out_s, out_classes=out_c, int_boxes=ib, int_ious=pair_iou)
    print("v2_postprocess: kept", len(out_s))


MINI_V1 = """[net]
batch=1
width=64
height=64
channels=3

[convolutional]
filters=16
size=7
stride=2
pad=1
activation=leaky

[maxpool]
size=2
stride=2

[convolutional]
filters=32
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=2

[convolutional]
filters=64
size=3
stride=2
pad=1
activation=leaky

[connected]
output=96
activation=leaky

[dropout]
probability=.5

[connected]
output=270
activation=linear

[detection]
classes=20
coords=4
rescore=1
side=3
num=2
softmax=0
sqrt=1
"""


def gen_mini_v1():
    """YOLOv1-style topology (7x7/2 bias conv, SAME pools, [connected] x2 with a [dropout] between, [detection]) through the
    compiled reference: every layer output, and get_network_boxes -> get_detection_detections (DN/detection_layer.c:225-254).
    The input is already in the reference's (x/255)*2-1 range (V1/YOLO_V1_Inference.py:67-71)."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    secs = IO.parse_cfg(MINI_V1)
    flat = IO.synth_weights(secs, seed=9)
    net = D.RefNet(MINI_V1, flat, 0, 1)
    rng = np.random.default_rng(13)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    x = (img.astype(np.float32) / np.float32(255.0)) * np.float32(2) - np.float32(1)
    net.predict(x)
    data = {"cfg": np.array(MINI_V1), "weights": flat, "image_u8": img, "header": np.array([0, 1])}
    for i in range(net.n):
        data["layer_%02d" % i] = net.layer_output_nhwc(i).astype(np.float32)
    thresh = 0.2
    bb, obj, pr = net.boxes(thresh, None, 20)
    data["boxes_raw"], data["obj_raw"], data["prob_raw"] = bb, obj, pr
    data["thresh"] = np.float32(thresh)
    np.savez_compressed(os.path.join(OUT, "mini_v1.npz"), **data)
    print("mini_v1 layers", net.n, "boxes", len(bb), "nonzero probs", int((pr > 0).sum()))
    net.close()


MINI_LOCAL = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mini_local.cfg")).read()


def gen_mini_local():
    """[local] layers (locally connected: unshared filters per output location, DN/local_layer.c:91-120; darknet's own yolov1.cfg has one
    between its last conv and the fully connected head): a same-size 3x3 / pad 1 one and a 2x2 / stride 2 / unpadded one, then
    [connected] + [detection], through the compiled reference.  (The first conv is there for its workspace: the reference sizes a
    [local] layer's im2col workspace in elements, not bytes -- DN/local_layer.c:64 -- and relies on an earlier conv's being larger.)"""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    secs = IO.parse_cfg(MINI_LOCAL)
    flat = IO.synth_weights(secs, seed=2)
    net = D.RefNet(MINI_LOCAL, flat, 0, 1)
    img = np.random.default_rng(17).integers(0, 256, (48, 48, 3), dtype=np.uint8)
    net.predict(img.astype(np.float32) / np.float32(255.0))
    data = {"cfg": np.array(MINI_LOCAL), "weights": flat, "image_u8": img, "header": np.array([0, 1])}
    for i in range(net.n):
        data["layer_%02d" % i] = net.layer_output_nhwc(i).astype(np.float32)
    bb, obj, pr = net.boxes(0.2, None, 2)
    data["boxes_raw"], data["obj_raw"], data["prob_raw"] = bb, obj, pr
    data["thresh"] = np.float32(0.2)
    np.savez_compressed(os.path.join(OUT, "mini_local.npz"), **data)
    print("mini_local layers", net.n, "boxes", len(bb))
    net.close()


def gen_mini(name, cfg, classes, nms_thresh=0.3, thresh=0.15):
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=7, obj_bias=0.5)
    mj, mn = IO.default_header(secs)
    net = D.RefNet(cfg, flat, mj, mn)
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    x = img.astype(np.float32) / np.float32(255.0)
    net.predict(x)
    data = {"cfg": np.array(cfg), "weights": flat, "image_u8": img, "header": np.array([mj, mn])}
    for i in range(net.n):
        data["layer_%02d" % i] = net.layer_output_nhwc(i).astype(np.float32)
    bb, obj, pr = net.boxes(thresh, None, classes)
    data["boxes_raw"], data["obj_raw"], data["prob_raw"] = bb, obj, pr
    net.predict(x)
    bb2, obj2, pr2 = net.boxes(thresh, nms_thresh, classes)
    data["boxes_nms"], data["obj_nms"], data["prob_nms"] = bb2, obj2, pr2
    data["thresh"] = np.float32(thresh); data["nms"] = np.float32(nms_thresh)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **data)
    print(name, "layers", net.n, "boxes", len(bb), "nonzero probs before/after nms", int((pr > 0).sum()), int((pr2 > 0).sum()))
    net.close()


def _conv(filters, size, stride=1, bn=True, act="leaky"):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", filters, size, stride, act)


_CLS_NET = "[net]\nbatch=1\nwidth=64\nheight=64\nchannels=3\n\n"
# darknet-53's tail order: ... -> [avgpool] -> 1x1 conv to the classes -> [softmax] (here with groups and a temperature) -> [cost]
MINI_CLS53 = (_CLS_NET + _conv(8, 3) + _conv(16, 3, 2) + _conv(8, 1) + _conv(16, 3) + "[shortcut]\nfrom=-3\nactivation=linear\n\n" + _conv(32, 3, 2) +
              "[avgpool]\n\n" + _conv(24, 1, bn=False, act="linear") + "[softmax]\ngroups=2\ntemperature=2\n\n[cost]\n")
# darknet-19's: ... -> 1x1 conv to the classes -> [avgpool] -> [softmax]
MINI_CLS19 = (_CLS_NET + _conv(8, 3) + "[maxpool]\nsize=2\nstride=2\n\n" + _conv(16, 3) + _conv(8, 1) + _conv(16, 3) + "[shortcut]\nfrom=-3\nactivation=linear\n\n" +
              "[maxpool]\nsize=2\nstride=2\n\n" + _conv(32, 3) + _conv(24, 1, bn=False, act="linear") + "[avgpool]\n\n[softmax]\ngroups=1\n")


def gen_mini_cls():
    """Two small classifier topologies, one of each tail order, through the compiled reference (avgpool_layer.c, softmax_layer.c,
    cost_layer.c): every layer output and the vector network_predict returns (the last layer that is not [cost]).  The last conv's
    parameters are scaled so that the reference's logits reach +-5: the probabilities must not be a near-uniform distribution."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    for name, cfg, seed, logit_layer in (("mini_cls53", MINI_CLS53, 21, 7), ("mini_cls19", MINI_CLS19, 23, 8)):
        secs = IO.parse_cfg(cfg)
        flat = IO.synth_weights(secs, seed=seed)
        last = IO.conv_specs(secs)[-1]
        tail = last["filters"] * (1 + last["cin"] * last["size"] ** 2)          # bias + filters of the (linear, bias-only) last conv
        img = np.random.default_rng(seed + 1).integers(0, 256, (64, 64, 3), dtype=np.uint8)
        x = img.astype(np.float32) / np.float32(255.0)
        net = D.RefNet(cfg, flat, 0, 2)
        net.predict(x)
        factor = np.float32(round(5.0 / float(np.abs(net.layer_output_nhwc(logit_layer)).max()), 2))
        net.close()
        flat[-tail:] *= factor
        net = D.RefNet(cfg, flat, 0, 2)
        net.predict(x)
        data = {"cfg": np.array(cfg), "weights": flat, "image_u8": img, "header": np.array([0, 2])}
        for i in range(net.n):
            data["layer_%02d" % i] = np.asarray(net.layer_output_nhwc(i), dtype=np.float32)
        out_layer = max(i for i in range(net.n) if secs[i + 1]["type"] != "cost")
        data["output"] = np.asarray(data["layer_%02d" % out_layer], dtype=np.float32).reshape(-1)
        data["max_abs_logit"] = np.float32(np.abs(data["layer_%02d" % logit_layer]).max())
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **data)
        print(name, "layers", net.n, "max|logit|", float(data["max_abs_logit"]), "p max/min", float(data["output"].max()), float(data["output"].min()))
        net.close()


def mini_resnet_cfg(size=32, mul=1):
    """A ResNet in miniature, one block per form of the general [shortcut] (DN/blas.c:68-92) and a sample of the activations outside
    the conv epilogues' slope family: a relu stem and a 2/2 max-pool; a bottleneck whose `from` tensor has fewer channels (16 -> 32); a
    matched one closed by relu; one whose 3x3 conv has stride 2, so that `from` is both larger and narrower (32 -> 64); one with
    logistic and tanh convs under an elu shortcut; a linear 1x1 conv to 24 classes, [avgpool], [softmax].  size=30 makes the pooled map
    15 x 15 and the strided block's output 8 x 8: stride = 15 / 8 = 1, the top-left 8 x 8 of `from` is added unstrided.  `mul` scales
    the channel counts (2: multiples of 32, what split-fp16 pairs need)."""
    m = mul
    sc = lambda act: "[shortcut]\nfrom=-4\nactivation=%s\n\n" % act
    return ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\n\n" % (size, size) + _conv(16 * m, 3, act="relu") + "[maxpool]\nsize=2\nstride=2\n\n" +
            _conv(8 * m, 1) + _conv(8 * m, 3) + _conv(32 * m, 1, act="linear") + sc("leaky") +
            _conv(8 * m, 1) + _conv(8 * m, 3) + _conv(32 * m, 1, act="linear") + sc("relu") +
            _conv(16 * m, 1) + _conv(16 * m, 3, 2) + _conv(64 * m, 1, act="linear") + sc("leaky") +
            _conv(16 * m, 1, act="logistic") + _conv(16 * m, 3, act="tanh") + _conv(64 * m, 1, act="linear") + sc("elu") +
            _conv(24, 1, bn=False, act="linear") + "[avgpool]\n\n[softmax]\ngroups=1\n")


def gen_mini_resnet():
    """mini_resnet_cfg at 32 x 32 and at 30 x 30 through the compiled reference (shortcut_layer.c, blas.c shortcut_cpu, activations.h):
    cfg text, weights, three images and every layer's output for each of them.  The last conv is scaled as gen_mini_cls does."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    for name, size, seed in (("mini_resnet", 32, 31), ("mini_resnet_30", 30, 33)):      # (one archive each: three images x every layer is 0.9 MB of floats that do not compress)
        cfg = mini_resnet_cfg(size)
        secs = IO.parse_cfg(cfg)
        flat = IO.synth_weights(secs, seed=seed)
        last = IO.conv_specs(secs)[-1]
        tail = last["filters"] * (1 + last["cin"] * last["size"] ** 2)
        imgs = np.random.default_rng(seed + 1).integers(0, 256, (3, size, size, 3), dtype=np.uint8)
        x = imgs.astype(np.float32) / np.float32(255.0)
        logit_layer = len(secs) - 4
        net = D.RefNet(cfg, flat, 0, 2)
        net.predict(x[0])
        factor = np.float32(round(5.0 / float(np.abs(net.layer_output_nhwc(logit_layer)).max()), 2))
        net.close()
        flat[-tail:] *= factor
        net = D.RefNet(cfg, flat, 0, 2)
        outs = [[] for _ in range(net.n)]
        for b in range(3):
            net.predict(x[b])
            for i in range(net.n):
                outs[i].append(np.asarray(net.layer_output_nhwc(i), dtype=np.float32).reshape(-1) if secs[i + 1]["type"] in ("avgpool", "softmax") else np.asarray(net.layer_output_nhwc(i), dtype=np.float32)[0])
        data = {"cfg": np.array(cfg), "weights": flat, "images_u8": imgs, "logit_layer": np.int32(logit_layer)}
        for i in range(net.n):
            data["layer_%02d" % i] = np.stack(outs[i])
        data["max_abs_logit"] = np.float32(np.abs(data["layer_%02d" % logit_layer]).max())
        print(name, "layers", net.n, "max|logit|", float(data["max_abs_logit"]), "p max", float(data["layer_%02d" % (net.n - 1)].max()))
        net.close()
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **data)


def _deconv(filters, size, stride, padding, bn=True, act="leaky"):
    return "[deconvolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npadding=%d\nactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", filters, size, stride, padding, act)


def mini_unet_cfg(height=12, width=20):
    """A U-Net in miniature, a map network ([net] yolo_output=map): two stride-2 convs down, a batch-normalised 4/2/1 deconv up whose output is
    concatenated with the encoder's tensor of that size (the skip connection: both write into windows of the concat buffer), a conv, a
    2/2/0 deconv with a tanh (a post-activation), a [shortcut] back to the first conv (not folded), [l2norm], darknet's [upsample] with
    a scale, a linear 3/1/1 deconv to six classes and [logistic].  The INPUT is 12 high x 20 wide -- half of the 24 x 40 first planned:
    at that size three images x every layer are 2.4 MB of floats that do not compress, and a committed fixture stays under 1 MB (the
    input was shrunk, not the layer list).  The [upsample] doubles the size again, so the MAP is 24 x 40 x 6: that is what the (24, 40)
    of the tests are."""
    return ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\nyolo_output=map\n\n" % (width, height) + _conv(16, 3) + _conv(24, 3, 2) + _conv(40, 3, 2) +
            _deconv(24, 4, 2, 1) + "[route]\nlayers=-1,1\n\n" + _conv(24, 3) + _deconv(16, 2, 2, 0, bn=False, act="tanh") +
            "[shortcut]\nfrom=0\nactivation=linear\n\n[l2norm]\n\n[upsample]\nstride=2\nscale=0.5\n\n" + _deconv(6, 3, 1, 1, bn=False, act="linear") + "[logistic]\n")


def mini_deconv_odd_cfg(height=10, width=14):
    """The deconv shapes the U-Net leaves out, on a 10 x 14 input taken down to 3 x 4 first: 3/2/1 (phases of unequal tap counts, an odd output
    extent: 5 x 7), an [activation] elu, 5/3/2 (13 x 19) and 1/2/0 (stride > size: three of four phases have no tap; 25 x 37)."""
    return ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\nyolo_output=map\n\n" % (width, height) + _conv(8, 3, 2) + _conv(16, 3, 2) +
            _deconv(12, 3, 2, 1) + "[activation]\nactivation=elu\n\n" + _deconv(8, 5, 3, 2, act="relu") + _deconv(6, 1, 2, 0, bn=False, act="linear"))


MARGIN_TOL = 5e-4          # the fp32 bound of the network tests, as a share of the output tensor's scale


def gen_mini_unet():
    """mini_unet_cfg and mini_deconv_odd_cfg through the compiled reference (deconvolutional_layer.c, l2norm_layer.c, upsample_layer.c,
    logistic_layer.c, activation_layer.c), the recipe of gen_mini_resnet: cfg text, weights, three images, every layer's output for each
    of them (separate predicts).  Per image also `margin`, the difference of the two largest channels of every output pixel, `argmax`,
    and `tight_share`, the share of pixels whose margin is below 2 x MARGIN_TOL x the output's scale -- the pixels a label comparison
    must leave out; it is asserted to be at most 2 %."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    for name, cfg, hw, seed in (("mini_unet", mini_unet_cfg(), (12, 20), 51), ("mini_deconv_odd", mini_deconv_odd_cfg(), (10, 14), 53)):
        secs = IO.parse_cfg(cfg)
        flat = IO.synth_weights(secs, seed=seed)
        imgs = np.random.default_rng(seed + 1).integers(0, 256, (3, hw[0], hw[1], 3), dtype=np.uint8)
        x = imgs.astype(np.float32) / np.float32(255.0)
        if name == "mini_unet":
            # the class deconv reads unit-norm pixels halved by the [upsample]: its filters are scaled until the reference's logits reach +-4
            # and its biases shrunk, as gen_mini_cls scales its class conv -- the labels must not be one class everywhere
            last = IO.conv_specs(secs)[-1]
            nw = last["filters"] * last["cin"] * last["size"] ** 2
            flat[-nw - last["filters"]:-nw] *= np.float32(0.2)
            net = D.RefNet(cfg, flat, 0, 2)
            net.predict(x[0])
            factor = np.float32(round(4.0 / float(np.abs(net.layer_output_nhwc(net.n - 2)).max()), 2))
            net.close()
            flat[-nw:] *= factor
        net = D.RefNet(cfg, flat, 0, 2)
        outs = [[] for _ in range(net.n)]
        for b in range(3):
            net.predict(x[b])
            for i in range(net.n):
                outs[i].append(np.asarray(net.layer_output_nhwc(i), dtype=np.float32)[0])
        data = {"cfg": np.array(cfg), "weights": flat, "images_u8": imgs}
        for i in range(net.n):
            data["layer_%02d" % i] = np.stack(outs[i])
        out = data["layer_%02d" % (net.n - 1)]
        top2 = np.sort(out, axis=-1)[..., -2:]
        scale = float(np.abs(out).max())
        data["margin"] = (top2[..., 1] - top2[..., 0]).astype(np.float32)
        data["argmax"] = np.argmax(out, axis=-1).astype(np.uint8)
        data["scale"] = np.float32(scale)
        data["tight_share"] = (data["margin"] < 2 * MARGIN_TOL * scale).reshape(3, -1).mean(axis=1).astype(np.float32)
        print(name, "layers", net.n, "map", out.shape[1:], "scale %.3f" % scale, "tight share per image", data["tight_share"],
              "labels used", np.unique(data["argmax"]).tolist())
        assert float(data["tight_share"].max()) <= 0.02, "too many near-ties: change the seed, not the cap"
        net.close()
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **data)
        print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


def _gconv(filters, size, groups, stride=1, bn=True, act="leaky"):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=1\ngroups=%d\nactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", filters, size, stride, groups, act)


def mini_grouped_cfg(size=32):
    """A classifier whose [convolutional] sections carry groups= (DN/parser.c:184, DN/convolutional_layer.c:458-471), one layer per shape the
    grouped kernel's bundle rule distinguishes: a relu stem (16) and a 2/2 max-pool; a bottleneck 1x1 16 -> 3x3 groups=4 16 -> 1x1 32 linear
    + leaky shortcut; one whose 3x3 is groups=8 with stride 2, its shortcut from the larger, narrower tensor; a depthwise 3x3 (groups =
    channels) and its pointwise 1x1; a depthwise stride-2 3x3 with bias and tanh (a post-activation); a grouped 5x5, groups=2; a [route] that
    concatenates that layer's output with the tensor it read (two grouped convs store into windows of one buffer); a grouped 1x1, groups=2,
    to 24 classes (the fp32 store), [avgpool], [softmax]."""
    sc = lambda act: "[shortcut]\nfrom=-4\nactivation=%s\n\n" % act
    return ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\n\n" % (size, size) + _conv(16, 3, act="relu") + "[maxpool]\nsize=2\nstride=2\n\n" +
            _conv(16, 1) + _gconv(16, 3, 4) + _conv(32, 1, act="linear") + sc("leaky") +
            _conv(16, 1) + _gconv(16, 3, 8, stride=2) + _conv(64, 1, act="linear") + sc("leaky") +
            _gconv(64, 3, 64) + _conv(32, 1) +
            _gconv(32, 3, 32, stride=2, bn=False, act="tanh") +
            _gconv(32, 5, 2) + "[route]\nlayers=-1,-2\n\n" +
            _gconv(24, 1, 2, bn=False, act="linear") + "[avgpool]\n\n[softmax]\ngroups=1\n")


MINI_DW_V3 = ("[net]\nbatch=1\nwidth=64\nheight=64\nchannels=3\n\n" + _conv(8, 3) + _gconv(8, 3, 8, stride=2) + _conv(16, 1) + _gconv(16, 3, 16) + _conv(16, 1, act="linear") +
              "[shortcut]\nfrom=-3\nactivation=linear\n\n" + _gconv(16, 3, 16, stride=2) + _conv(32, 1) + "[maxpool]\nsize=2\nstride=2\n\n" + _gconv(32, 3, 32) + _conv(16, 1) +
              _conv(27, 1, bn=False, act="linear") + "[yolo]\nmask=3,4,5\nanchors=4,5,  8,6,  10,14,  20,18,  30,40,  50,44\nclasses=4\nnum=6\n\n" +
              "[route]\nlayers=-3\n\n" + _conv(8, 1) + "[upsample]\nstride=2\n\n[route]\nlayers=-1,7\n\n" + _gconv(40, 3, 40) + _conv(24, 1) +
              _conv(27, 1, bn=False, act="linear") + "[yolo]\nmask=0,1,2\nanchors=4,5,  8,6,  10,14,  20,18,  30,40,  50,44\nclasses=4\nnum=6\n")

TOL16_BF16 = 3e-2          # the bf16 bound of the classifier tests, as a share of the largest logit


def gen_mini_grouped():
    """mini_grouped_cfg through the compiled reference (convolutional_layer.c with l.groups), the recipe of gen_mini_resnet: cfg text,
    weights, three images, every layer's output for each (separate predicts); the class conv scaled until the reference's logits reach
    +-5.  Asserted: on every image the two largest pooled logits differ by more than twice the bf16 bound, so that a top-1 comparison
    holds for all three.  And mini_dw_v3: a two-head [yolo] detector on a depthwise-separable backbone, through gen_mini."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    name, size, seed = "mini_grouped", 32, 61
    cfg = mini_grouped_cfg(size)
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=seed)
    last = IO.conv_specs(secs)[-1]
    tail = last["filters"] * (1 + (last["cin"] // last["groups"]) * last["size"] ** 2)
    imgs = np.random.default_rng(seed + 1).integers(0, 256, (3, size, size, 3), dtype=np.uint8)
    x = imgs.astype(np.float32) / np.float32(255.0)
    logit_layer = len(secs) - 4
    net = D.RefNet(cfg, flat, 0, 2)
    net.predict(x[0])
    factor = np.float32(round(5.0 / float(np.abs(net.layer_output_nhwc(logit_layer)).max()), 2))
    net.close()
    flat[-tail:] *= factor
    net = D.RefNet(cfg, flat, 0, 2)
    outs = [[] for _ in range(net.n)]
    for b in range(3):
        net.predict(x[b])
        for i in range(net.n):
            outs[i].append(np.asarray(net.layer_output_nhwc(i), dtype=np.float32).reshape(-1) if secs[i + 1]["type"] in ("avgpool", "softmax") else np.asarray(net.layer_output_nhwc(i), dtype=np.float32)[0])
    data = {"cfg": np.array(cfg), "weights": flat, "images_u8": imgs, "logit_layer": np.int32(logit_layer)}
    for i in range(net.n):
        data["layer_%02d" % i] = np.stack(outs[i])
    data["max_abs_logit"] = np.float32(np.abs(data["layer_%02d" % logit_layer]).max())
    pooled = data["layer_%02d" % (net.n - 2)]
    top2 = np.sort(pooled, axis=-1)[:, -2:]
    data["top1_margin"] = (top2[:, 1] - top2[:, 0]).astype(np.float32)
    print(name, "layers", net.n, "max|logit|", float(data["max_abs_logit"]), "pooled max", float(np.abs(pooled).max()), "top-1 margins", data["top1_margin"], "p max", float(data["layer_%02d" % (net.n - 1)].max()))
    assert float(data["top1_margin"].min()) > 2 * TOL16_BF16 * float(np.abs(pooled).max()), "a top-1 margin below twice the bf16 bound: change the seed, not the rule"
    net.close()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **data)
    print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")
    gen_mini("mini_dw_v3", MINI_DW_V3, 4)


def _wconv(filters, size, stride=1, pad="pad=1", bn=True, act="leaky"):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\n%s\nactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", filters, size, stride, pad, act)


def mini_wide_cfg(width=43, height=35):
    """A small rectangular, odd-sized classifier of dense convs whose size is neither 1 nor 3: an 11x11 / 4 relu stem without padding and
    without batch norm on the image (AlexNet's first layer); a 5x5 (the last size one validity bit per tap holds); a 7x7 with a linear
    epilogue and a leaky [shortcut] from the 5x5 layer behind it; a 6x6 / 2 (even, strided); a 2x2 with padding=0; a 9x9 over a tensor
    smaller than the filter; a [route] that concatenates the last two (the 9x9 and the 2x2 store into windows of one buffer); a 1x1 to
    10 classes (the fp32 store), [avgpool], [softmax]."""
    return ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\n\n" % (width, height) + _wconv(16, 11, 4, "pad=0", bn=False, act="relu") +
            _wconv(16, 5) + _wconv(16, 7, act="linear") + "[shortcut]\nfrom=-2\nactivation=leaky\n\n" +
            _wconv(24, 6, 2) + _wconv(8, 2, 1, "pad=0\npadding=0") + _wconv(16, 9) + "[route]\nlayers=-1,-2\n\n" +
            _wconv(10, 1, bn=False, act="linear") + "[avgpool]\n\n[softmax]\ngroups=1\n")


def gen_mini_wide():
    """mini_wide_cfg through the compiled reference, the recipe of gen_mini_grouped: cfg text, weights, three images, every layer's output
    for each (separate predicts); the class conv scaled until the reference's logits reach +-5.  Asserted: on every image the two largest
    pooled logits differ by more than twice the bf16 bound."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    name, width, height, seed = "mini_wide", 43, 35, 73
    cfg = mini_wide_cfg(width, height)
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=seed)
    last = IO.conv_specs(secs)[-1]
    tail = last["filters"] * (1 + last["cin"] * last["size"] ** 2)
    imgs = np.random.default_rng(seed + 1).integers(0, 256, (3, height, width, 3), dtype=np.uint8)
    x = imgs.astype(np.float32) / np.float32(255.0)
    logit_layer = len(secs) - 4
    net = D.RefNet(cfg, flat, 0, 2)
    net.predict(x[0])
    factor = np.float32(round(5.0 / float(np.abs(net.layer_output_nhwc(logit_layer)).max()), 2))
    net.close()
    flat[-tail:] *= factor
    net = D.RefNet(cfg, flat, 0, 2)
    outs = [[] for _ in range(net.n)]
    for b in range(3):
        net.predict(x[b])
        for i in range(net.n):
            outs[i].append(np.asarray(net.layer_output_nhwc(i), dtype=np.float32).reshape(-1) if secs[i + 1]["type"] in ("avgpool", "softmax") else np.asarray(net.layer_output_nhwc(i), dtype=np.float32)[0])
    data = {"cfg": np.array(cfg), "weights": flat, "images_u8": imgs, "logit_layer": np.int32(logit_layer)}
    for i in range(net.n):
        data["layer_%02d" % i] = np.stack(outs[i])
    data["max_abs_logit"] = np.float32(np.abs(data["layer_%02d" % logit_layer]).max())
    pooled = data["layer_%02d" % (net.n - 2)]
    top2 = np.sort(pooled, axis=-1)[:, -2:]
    data["top1_margin"] = (top2[:, 1] - top2[:, 0]).astype(np.float32)
    print(name, "layers", net.n, "max|logit|", float(data["max_abs_logit"]), "pooled max", float(np.abs(pooled).max()), "top-1 margins", data["top1_margin"], "p max", float(data["layer_%02d" % (net.n - 1)].max()))
    assert float(data["top1_margin"].min()) > 2 * TOL16_BF16 * float(np.abs(pooled).max()), "a top-1 margin below twice the bf16 bound: change the seed, not the rule"
    net.close()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **data)
    print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


def gen_bn_real():
    """D2T/log.txt is the reference's stdout of two detect runs (yolov2 then yolov3) with the printf block of DN/parser.c:1176-1228
    enabled: per batch-normalised conv five lines of numbers (beta, gamma, rolling mean, rolling variance -- l.n values each -- and the
    first l.n of the l.nweights filter values), per plain conv (the heads) the filter line only; line 223 / 950 are the detections."""
    import re
    lines = open(os.path.join(REF, "Darknet2Tensorflow", "darknet-master", "log.txt")).read().split("\n")
    for name, lo, hi, n_bn, n_conv in (("yolov2", 1, 222, 22, 23), ("yolov3", 224, 949, 72, 75)):
        convs = []; cur = None; k = lo - 1
        while k < hi:
            h = lines[k]
            m = re.match(r"\*+robin#convolutional_(\w+?)(?:/\w+)?\((?:l\.n|num)=(\d+)\)", h)
            assert m, (k + 1, h[:80])
            vals = np.array([float(v) for v in lines[k + 1].replace(" ", "").split(",") if v], dtype=np.float32)
            what, cnt = m.group(1), int(m.group(2))
            if what == "biases":
                cur = {"n": cnt, "beta": vals}
            elif what in ("scales", "rolling_mean", "rolling_variance"):
                cur[{"scales": "gamma", "rolling_mean": "mean", "rolling_variance": "var"}[what]] = vals
            else:
                assert what == "weights"
                c = cur if cur is not None else {"n": len(vals)}
                c["nweights"] = cnt; c["w_first"] = vals
                assert all(len(c[q]) == c["n"] for q in ("beta", "gamma", "mean", "var") if q in c) and len(vals) == c["n"]
                convs.append(c); cur = None
            k += 2
        assert len(convs) == n_conv and sum("beta" in c for c in convs) == n_bn, (len(convs), name)
        data = {"n_conv": np.int32(len(convs)), "filters": np.array([c["n"] for c in convs], np.int32),
                "nweights": np.array([c["nweights"] for c in convs], np.int64), "bn": np.array(["beta" in c for c in convs])}
        for i, c in enumerate(convs):
            for q in ("beta", "gamma", "mean", "var", "w_first"):
                if q in c:
                    data["%s_%d" % (q, i)] = c[q]
        np.savez_compressed(os.path.join(OUT, name + "_bn_real.npz"), **data)
        bn = [c for c in convs if "beta" in c]
        print(name + "_bn_real: %d convs (%d batch-normalised), gamma %.4g..%.4g (%.1f%% negative), beta %.3g..%.3g, mean %.3g..%.3g, var %.3g..%.3g"
              % (len(convs), len(bn), min(c["gamma"].min() for c in bn), max(c["gamma"].max() for c in bn),
                 100.0 * sum((c["gamma"] < 0).sum() for c in bn) / sum(c["n"] for c in bn),
                 min(c["beta"].min() for c in bn), max(c["beta"].max() for c in bn), min(c["mean"].min() for c in bn), max(c["mean"].max() for c in bn),
                 min(c["var"].min() for c in bn), max(c["var"].max() for c in bn)))


def gen_known_answers():
    """The reference's only recorded END-TO-END results: the detections its darknet binding printed for dog.jpg with the genuine
    yolov2.weights (D2T/log.txt:223) and yolov3.weights (:950) -- `detect()` of D2T/darknet.py:125-142, thresh .5, nms .45: a list of
    (class name, probability, (cx, cy, w, h) in pixels of the 768 x 576 image).  Numbers only -> tests/golden/dog_known_answers.json; they
    become checkable the day somebody supplies the files (tests/test_gpu_real_weights.py, YOLO_REAL_WEIGHTS / YOLO_REAL_WEIGHTS_V2)."""
    import ast, json
    lines = open(os.path.join(REF, "Darknet2Tensorflow", "darknet-master", "log.txt")).read().split("\n")
    out = {"image": "dog.jpg", "image_size_wh": [768, 576], "call": "darknet.py detect(net, meta, image, thresh=.5, hier_thresh=.5, nms=.45)",
           "coco_index": {"bicycle": 1, "truck": 7, "dog": 16}}
    for name, ln in (("yolov2", 223), ("yolov3", 950)):
        dets = ast.literal_eval(lines[ln - 1])
        out[name] = {"log_line": ln, "detections": [{"name": n, "prob": p, "box_cxcywh": list(b)} for n, p, b in dets]}
        print(name, [(n, round(p, 4)) for n, p, _ in dets])
    json.dump(out, open(os.path.join(OUT, "dog_known_answers.json"), "w"), indent=1)


def gen_darknet_py_symbols():
    """Every symbol the reference's Python binding resolves from libdarknet.so (`lib.X` in D2T/darknet.py:49-115): the names only ->
    tests/golden/darknet_py_bound_symbols.json, what tests/test_host.py holds libdarknet_hip.so's exports against."""
    import json, re
    text = open(os.path.join(REF, "Darknet2Tensorflow", "darknet-master", "darknet.py")).read()
    names = sorted(set(re.findall(r"\blib\.(\w+)", text)))
    json.dump({"source": "D2T/darknet.py", "lib_symbols": names}, open(os.path.join(OUT, "darknet_py_bound_symbols.json"), "w"), indent=1)
    print("darknet.py binds", len(names), "symbols")


# ---- rectangular networks (width != height): the same minis at another [net] size, through the same compiled reference ----
def _rect_cfg(cfg, height, width):
    from yolo_tensorflow_amd import darknet_io as IO
    return IO.with_input_size(cfg, (height, width))


def _head_counts(net, secs, thresh, classes):
    """Boxes whose objectness exceeds `thresh`, per [yolo] / [region] layer, from the layer's own output (planar, logistic applied)."""
    counts = []
    for i in range(net.n):
        if secs[i + 1]["type"] not in ("yolo", "region"):
            continue
        o = net.layer_output_nhwc(i)[0]
        counts.append(int((o[..., 4::5 + classes] > thresh).sum()))
    return counts


def gen_mini_rect(name, cfg, classes, height, width, nms_thresh=0.3, thresh=0.15, letterbox=False):
    """gen_mini at height x width.  The image seed is the first from 11 on for which every head has a box above thresh, there are at
    least 8 boxes in all, and do_nms_sort suppresses at least one box and leaves at least one (thresholds are never lowered).
    letterbox: also the reference's own letterbox_image of three float CHW source images (wider than, taller than and of the network's
    aspect) and get_network_boxes at each image's (w, h), relative=1 -- written to <name>_letterbox.npz (the committed-file size limit)."""
    import ctypes as C
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    cfg = _rect_cfg(cfg, height, width)
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=7, obj_bias=0.5)
    mj, mn = IO.default_header(secs)
    net = D.RefNet(cfg, flat, mj, mn)
    assert (net.h, net.w) == (height, width)
    for seed in range(11, 200):
        img = np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)
        x = img.astype(np.float32) / np.float32(255.0)
        net.predict(x)
        layers = [net.layer_output_nhwc(i).astype(np.float32) for i in range(net.n)]
        heads = _head_counts(net, secs, thresh, classes)
        bb, obj, pr = net.boxes(thresh, None, classes)
        net.predict(x)
        bb2, obj2, pr2 = net.boxes(thresh, nms_thresh, classes)
        before, after = int((pr > 0).sum()), int((pr2 > 0).sum())
        if min(heads) >= 1 and len(bb) >= 8 and 0 < after < before:
            break
    else:
        raise SystemExit(name + ": no image seed meets the fixture conditions")
    data = {"cfg": np.array(cfg), "weights": flat, "image_u8": img, "header": np.array([mj, mn])}
    for i, o in enumerate(layers):
        data["layer_%02d" % i] = o
    data["boxes_raw"], data["obj_raw"], data["prob_raw"] = bb, obj, pr
    data["boxes_nms"], data["obj_nms"], data["prob_nms"] = bb2, obj2, pr2
    data["thresh"] = np.float32(thresh); data["nms"] = np.float32(nms_thresh)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **data)
    print(name, "image seed", seed, "layers", net.n, "boxes", len(bb), "per head", heads, "nonzero probs before/after nms", before, after)
    if letterbox:
        class IMAGE(C.Structure):
            _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]
        l = D.lib()
        l.letterbox_image.argtypes = [IMAGE, C.c_int, C.c_int]; l.letterbox_image.restype = IMAGE
        l.free_image.argtypes = [IMAGE]
        lb = {"thresh": np.float32(thresh), "nms": np.float32(nms_thresh)}
        for k, (ih, iw) in enumerate(((37, 80), (50, 37), (32, 48))):
            for sseed in range(31 + 100 * k, 31 + 100 * k + 100):
                src = np.ascontiguousarray(np.random.default_rng(sseed).random((3, ih, iw), dtype=np.float32))
                im = IMAGE(iw, ih, 3, src.ctypes.data_as(C.POINTER(C.c_float)))
                boxed = l.letterbox_image(im, net.w, net.h)
                inp = np.ctypeslib.as_array(boxed.data, shape=(3, net.h, net.w)).copy()
                l.free_image(boxed)
                net.predict(np.transpose(inp, (1, 2, 0)))
                num = C.c_int(0)
                dets = l.get_network_boxes(net.net, iw, ih, thresh, .5, None, 1, C.byref(num))
                n = num.value
                bbk = np.zeros((n, 4), np.float32); objk = np.zeros(n, np.float32); prk = np.zeros((n, classes), np.float32)
                for i in range(n):
                    d = dets[i]
                    bbk[i] = (d.bbox.x, d.bbox.y, d.bbox.w, d.bbox.h); objk[i] = d.objectness
                    prk[i] = np.ctypeslib.as_array(d.prob, shape=(classes,))
                l.do_nms_sort(dets, n, classes, nms_thresh)
                prn = np.zeros((n, classes), np.float32); bbn = np.zeros((n, 4), np.float32)
                for i in range(n):
                    prn[i] = np.ctypeslib.as_array(dets[i].prob, shape=(classes,))
                    bbn[i] = (dets[i].bbox.x, dets[i].bbox.y, dets[i].bbox.w, dets[i].bbox.h)
                l.free_detections(dets, n)
                b4, a4 = int((prk > 0).sum()), int((prn > 0).sum())
                if min(_head_counts(net, secs, thresh, classes)) >= 1 and n >= 8 and 0 < a4 < b4:
                    break
            else:
                raise SystemExit(name + ": no source seed meets the fixture conditions for %d x %d" % (ih, iw))
            lb["src_%d" % k], lb["input_%d" % k] = src, inp
            lb["boxes_%d" % k], lb["obj_%d" % k], lb["prob_%d" % k], lb["prob_nms_%d" % k], lb["boxes_nms_%d" % k] = bbk, objk, prk, prn, bbn
            print(name, "letterbox source %d x %d seed %d: boxes %d, nonzero probs before/after nms %d %d" % (ih, iw, sseed, n, b4, a4))
        np.savez_compressed(os.path.join(OUT, name + "_letterbox.npz"), **lb)
    net.close()


def gen_mini_cls_rect():
    """gen_mini_cls's darknet-19 mini at 64 high x 96 wide: every layer output and the softmax vector."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    cfg, seed, logit_layer = _rect_cfg(MINI_CLS19, 64, 96), 23, 8
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=seed)
    last = IO.conv_specs(secs)[-1]
    tail = last["filters"] * (1 + last["cin"] * last["size"] ** 2)
    img = np.random.default_rng(seed + 1).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    x = img.astype(np.float32) / np.float32(255.0)
    net = D.RefNet(cfg, flat, 0, 2)
    net.predict(x)
    factor = np.float32(round(5.0 / float(np.abs(net.layer_output_nhwc(logit_layer)).max()), 2))
    net.close()
    flat[-tail:] *= factor
    net = D.RefNet(cfg, flat, 0, 2)
    net.predict(x)
    data = {"cfg": np.array(cfg), "weights": flat, "image_u8": img, "header": np.array([0, 2])}
    for i in range(net.n):
        data["layer_%02d" % i] = np.asarray(net.layer_output_nhwc(i), dtype=np.float32)
    out_layer = max(i for i in range(net.n) if secs[i + 1]["type"] != "cost")
    data["output"] = np.asarray(data["layer_%02d" % out_layer], dtype=np.float32).reshape(-1)
    data["max_abs_logit"] = np.float32(np.abs(data["layer_%02d" % logit_layer]).max())
    np.savez_compressed(os.path.join(OUT, "mini_cls_rect.npz"), **data)
    print("mini_cls_rect layers", net.n, "max|logit|", float(data["max_abs_logit"]), "p max/min", float(data["output"].max()), float(data["output"].min()))
    net.close()


def _econv(filters, size, stride=1, pad=None, padding=None, bn=False, act="leaky"):
    """a [convolutional] section with its geometry keys spelled out: pad=1 (size / 2), or pad=0 and a literal padding="""
    geo = "pad=1\n" if pad else "pad=0\n" + ("padding=%d\n" % padding if padding is not None else "")
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\n%sactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", filters, size, stride, geo, act)


def _pool(size, stride, padding=None):
    return "[maxpool]\nsize=%d\nstride=%d\n%s\n" % (size, stride, "padding=%d\n" % padding if padding is not None else "")


def mini_edges_cfg(height=15, width=22):
    """The layers that move data and the dense conv's geometry keys at the edges the planner accepts: a map network on a 15 high x 22 wide
    input whose channel counts are no multiples of 8 or 4 where a layer allows it (3 -> 20 -> 12 -> 27 -> 20).  Layer by layer (H x W x C):
      0 conv 3x3 pad=0 ("valid"), bn                      13 x 20 x 20
      1 maxpool 2/2 on odd extents                          6 x 10 x 20
      2 maxpool 3/2 padding=0                               3 x  5 x 20
      3 conv 1x1, bn                                        3 x  5 x 12
      4 route 0 (one input)                                13 x 20 x 20
      5 conv 3x3 pad=0 padding=2, bias: windows of padding 15 x 22 x 12
      6 maxpool 3/2 (padding 1)                             8 x 12 x 12
      7 conv 3x3 pad=0 padding=2 stride=2, bias, linear     5 x  7 x 27
      8 maxpool 2/1                                         5 x  7 x 27
      9 conv 3x3 stride=2 pad=1, bn                         3 x  4 x 20
     10 upsample 2                                          6 x  8 x 20
     11 conv 3x3 pad=1, bias, leaky                         6 x  8 x 20
     12 shortcut from 10 (identity; layer 11 is read again by 15, so no plan folds the add into the conv)
     13 reorg 2                                             3 x  4 x 80
     14 conv 3x3 pad=0 ("valid"), bias                       1 x  2 x 12
     15 route 11 (one input)                                6 x  8 x 20
     16 maxpool 3/1 padding=0                               6 x  8 x 20
     17 route 5 (one input)                                15 x 22 x 12
     18 conv 3x3 stride=3 pad=0 padding=2, bias             6 x  8 x 12
     19 route 16, 18: 20 + 12 channels, the second at channel offset 20
     20 conv 3x3 pad=1 to 6 channels, bias, linear: the map 6 x 8 x 6
    Every pool has padding < min(size, stride): no window lies wholly outside its tensor (there darknet writes -FLT_MAX, the device -inf).
    No 1x1 conv here has a padding or a stride: the reference's forward_convolutional_layer hands a 1x1 conv's input to gemm without im2col
    (DN/convolutional_layer.c:468), as if stride were 1 and padding 0 -- with padding=1 it reads past its input (two runs of this generator
    gave two answers), with stride=2 it reads the wrong pixels.  Those two layers are tested on the device against the convolution's
    definition instead (tests/test_gpu_edges.py)."""
    return ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\nyolo_output=map\n\n" % (width, height) +
            _econv(20, 3, pad=0, bn=True) + _pool(2, 2) + _pool(3, 2, 0) + _econv(12, 1, pad=0, bn=True) + "[route]\nlayers=0\n\n" +
            _econv(12, 3, padding=2) + _pool(3, 2) + _econv(27, 3, stride=2, padding=2, act="linear") + _pool(2, 1) + _econv(20, 3, stride=2, pad=1, bn=True) +
            "[upsample]\nstride=2\n\n" + _econv(20, 3, pad=1) + "[shortcut]\nfrom=-2\nactivation=linear\n\n[reorg]\nstride=2\n\n" + _econv(12, 3, pad=0) +
            "[route]\nlayers=11\n\n" + _pool(3, 1, 0) + "[route]\nlayers=5\n\n" + _econv(12, 3, stride=3, padding=2) + "[route]\nlayers=16,18\n\n" +
            _econv(6, 3, pad=1, act="linear"))


def save_npz_reproducibly(path, data):
    """np.savez_compressed with a fixed member date: the same arrays give the same bytes"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, val in data.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)); info.compress_type = zipfile.ZIP_DEFLATED; info.external_attr = 0o644 << 16
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(val), allow_pickle=False)


def gen_edges():
    """mini_edges_cfg through the compiled reference (maxpool_layer.c, upsample_layer.c, reorg_layer.c, route_layer.c, shortcut_layer.c and
    convolutional_layer.c with pad=0 / padding= / stride), the recipe of gen_mini_unet: cfg text, weights (filters bf16-exact), three images,
    every layer's output for each of them (separate predicts), `max_abs` per layer."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    name, cfg, hw, seed = "mini_edges", mini_edges_cfg(), (15, 22), 71
    secs = IO.parse_cfg(cfg)
    flat = IO.bf16_exact_filters(secs, IO.synth_weights(secs, seed=seed))
    imgs = np.random.default_rng(seed + 1).integers(0, 256, (3, hw[0], hw[1], 3), dtype=np.uint8)
    x = imgs.astype(np.float32) / np.float32(255.0)
    net = D.RefNet(cfg, flat, 0, 2)
    outs = [[] for _ in range(net.n)]
    for b in range(3):
        net.predict(x[b])
        for i in range(net.n):
            outs[i].append(np.asarray(net.layer_output_nhwc(i), dtype=np.float32)[0])
    data = {"cfg": np.array(cfg), "weights": flat, "images_u8": imgs}
    for i in range(net.n):
        data["layer_%02d" % i] = np.stack(outs[i])
    data["max_abs"] = np.array([np.abs(data["layer_%02d" % i]).max() for i in range(net.n)], dtype=np.float32)
    shapes = IO.layer_shapes(secs)
    for i in range(net.n):
        assert data["layer_%02d" % i].shape[1:] == shapes[i][1:4], (i, data["layer_%02d" % i].shape, shapes[i])
        assert np.isfinite(data["layer_%02d" % i]).all() and np.abs(data["layer_%02d" % i]).max() < 1e30, "layer %d holds -FLT_MAX: a pool window wholly outside its tensor" % i
    net.close()
    path = os.path.join(OUT, name + ".npz")
    save_npz_reproducibly(path, data)
    print(name, "layers", len(shapes), "map", data["layer_%02d" % (len(shapes) - 1)].shape[1:], "max_abs", np.round(data["max_abs"], 3).tolist(), os.path.getsize(path), "bytes")


def mini_seq_cfg():
    """Recurrent layers behind a small conv stack: 32 x 32 x 3 -> 4 x 4 x 16 -> [connected] 64, then two [rnn] (batch-normalised leaky; logistic with
    shortcut=1), two [gru] (batch-normalised with tanh=1; plain), two [lstm] (batch-normalised; plain), a batch-normalised [connected] to 10
    classes and [softmax]."""
    return ("[net]\nbatch=1\nwidth=32\nheight=32\nchannels=3\ntime_steps=1\n\n" + _conv(8, 3, 2) + "[maxpool]\nsize=2\nstride=2\n\n" + _conv(16, 3, 2) +
            "[connected]\noutput=64\nactivation=leaky\n\n"
            "[rnn]\noutput=40\nactivation=leaky\nbatch_normalize=1\n\n[rnn]\noutput=40\nshortcut=1\n\n"
            "[gru]\noutput=48\ntanh=1\nbatch_normalize=1\n\n[gru]\noutput=24\n\n"
            "[lstm]\noutput=40\nbatch_normalize=1\n\n[lstm]\noutput=24\n\n"
            "[connected]\noutput=10\nbatch_normalize=1\nactivation=linear\n\n[softmax]\n")


def mini_crnn_cfg():
    """A detector with temporal context: 32 x 32 x 3 -> 3x3/2 conv -> 2x2 max-pool (8 x 8) -> a batch-normalised leaky [crnn] whose 20 hidden channels are
    no multiple of 8 -> a relu [crnn] with shortcut=1 -> a linear 1x1 conv to 18 channels -> [yolo] with one class and three anchors.
    In front of all that stands one 3x3/1 conv at full size, for the reference's sake: darknet sizes the im2col workspace all layers share from
    the layers' own workspace_size, make_crnn_layer sets none, and the [crnn] convs' 46 KB columns would overrun the 27 KB the 3x3/2 conv over
    3 channels asks for (the reference then corrupts its heap); a 32 x 32 conv asks for 110 KB."""
    return ("[net]\nbatch=1\nwidth=32\nheight=32\nchannels=3\ntime_steps=1\n\n" + _conv(8, 3) + _conv(8, 3, 2) + "[maxpool]\nsize=2\nstride=2\n\n"
            "[crnn]\nhidden_filters=20\noutput_filters=24\nactivation=leaky\nbatch_normalize=1\n\n"
            "[crnn]\nhidden_filters=16\noutput_filters=16\nactivation=relu\nshortcut=1\n\n" + _conv(18, 1, bn=False, act="linear") +
            "[yolo]\nmask=0,1,2\nanchors=4,5,  8,6,  10,14\nclasses=1\nnum=3\n")


def gen_recurrent(seed=93):
    gen_mini_seq(seed)
    gen_mini_crnn()


def gen_mini_crnn(seed=57, thresh=0.7):
    """mini_crnn_cfg through the compiled reference (crnn_layer.c): one live network over T = 5 frames, every layer's output and the boxes
    get_network_boxes returns after each of them; drift16_* as in mini_seq.npz."""
    import importlib.util
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    spec = importlib.util.spec_from_file_location("test_recurrent_host", os.path.join(ROOT, "tests", "test_recurrent_host.py"))
    sys.path.insert(0, os.path.join(ROOT, "tests")); RH = importlib.util.module_from_spec(spec); spec.loader.exec_module(RH)
    name, cfg, steps = "mini_crnn", mini_crnn_cfg(), 5
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=seed, obj_bias=0.5)
    imgs = np.random.default_rng(seed + 1).integers(0, 256, (steps, 32, 32, 3), dtype=np.uint8)
    x = imgs.astype(np.float32) / np.float32(255.0)
    shapes = IO.layer_shapes(secs)
    net = D.RefNet(cfg, flat, 0, 2)
    outs = [[] for _ in range(net.n)]
    data = {"cfg": np.array(cfg), "weights": flat, "images_u8": imgs, "thresh": np.float32(thresh)}
    for t in range(steps):
        net.predict(x[t])
        for i in range(net.n):
            outs[i].append(np.asarray(net.layer_output_nhwc(i), dtype=np.float32).reshape(-1))
        bb, obj, pr = net.boxes(thresh, None, 1)
        data["boxes_%d" % t], data["obj_%d" % t], data["prob_%d" % t] = bb, obj, pr
    net.close()
    for i, o in enumerate(outs):
        o = np.stack(o); assert np.isfinite(o).all()
        data["layer_%02d" % i] = o.reshape((steps,) + tuple(shapes[i][1:4])) if secs[i + 1]["type"] != "yolo" else o
    nl = len(outs) - 1          # (the [yolo] layer's own output is the reference's activated copy: not compared)
    for tag, store in (("bf16", RH.bf16), ("fp16", RH.fp16)):
        sim = RH.run_frames(cfg, flat, imgs, store)
        data["drift16_" + tag] = np.array([[RH.standoff(sim[t][i], data["layer_%02d" % i][t]) for i in range(nl)] for t in range(steps)], dtype=np.float64)
    exact = RH.run_frames(cfg, flat, imgs)
    worst = max(RH.standoff(exact[t][i], data["layer_%02d" % i][t]) for t in range(steps) for i in range(nl))
    path = os.path.join(OUT, name + ".npz")
    save_npz_reproducibly(path, data)
    print(name, "layers", len(outs), "boxes per frame", [len(data["boxes_%d" % t]) for t in range(steps)], "restatement stand-off %.2e" % worst,
          "drift bf16 %.3g fp16 %.3g" % (data["drift16_bf16"].max(), data["drift16_fp16"].max()), os.path.getsize(path), "bytes")


def gen_mini_seq(seed=93):
    """mini_seq_cfg through the compiled reference (rnn_layer.c, gru_layer.c, lstm_layer.c, connected_layer.c with batch norm): ONE network kept
    alive over T = 5 distinct frames, every layer's output after each of them, the top class per frame.  drift16_bf16 / drift16_fp16 [T][layers]:
    how far the host restatement (tests/test_recurrent_host.py) stands off from those outputs, as a share of each tensor's largest value, when
    it rounds operands and stored tensors to that type where the device does -- the yardstick of the 16-bit device tests at steps 2..5."""
    import importlib.util
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    spec = importlib.util.spec_from_file_location("test_recurrent_host", os.path.join(ROOT, "tests", "test_recurrent_host.py"))
    sys.path.insert(0, os.path.join(ROOT, "tests")); RH = importlib.util.module_from_spec(spec); spec.loader.exec_module(RH)
    name, cfg, steps = "mini_seq", mini_seq_cfg(), 5
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=seed)
    imgs = np.random.default_rng(seed + 1).integers(0, 256, (steps, 32, 32, 3), dtype=np.uint8)
    x = imgs.astype(np.float32) / np.float32(255.0)
    # the class layer's rows are scaled until the reference's logits reach +-4 over the sequence: the probabilities must not be near-uniform
    last = IO.conv_specs(secs)[-1]
    tail = IO.connected_floats(last["cin"], last["filters"], 1)
    def run(weights):
        net = D.RefNet(cfg, weights, 0, 2)
        outs = [[] for _ in range(net.n)]
        for t in range(steps):
            net.predict(x[t])
            for i in range(net.n):
                outs[i].append(np.asarray(net.layer_output_nhwc(i), dtype=np.float32).reshape(-1))
        net.close()
        return [np.stack(o) for o in outs]
    logits = run(flat)[-2]
    nw = last["filters"] * last["cin"]
    flat[-tail + last["filters"]:-tail + last["filters"] + nw] *= np.float32(round(4.0 / float(np.abs(logits).max()), 2))      # (the rows; batch norm renormalises them unless the variance is kept)
    flat[-last["filters"]:] *= np.float32(0.05)          # ... so the rolling variance is shrunk with them
    outs = run(flat)
    shapes = IO.layer_shapes(secs)
    data = {"cfg": np.array(cfg), "weights": flat, "images_u8": imgs}
    for i, o in enumerate(outs):
        data["layer_%02d" % i] = o.reshape((steps,) + tuple(shapes[i][1:4]))          # (layer_output_nhwc: image-shaped layers come as HWC; the rest are 1 x 1 x C)
        assert np.isfinite(o).all()
    data["top"] = np.argmax(outs[-1], axis=1).astype(np.int32)
    for tag, store in (("bf16", RH.bf16), ("fp16", RH.fp16)):
        sim = RH.run_frames(cfg, flat, imgs, store)
        data["drift16_" + tag] = np.array([[RH.standoff(sim[t][i], data["layer_%02d" % i][t]) for i in range(len(outs))] for t in range(steps)], dtype=np.float64)
    exact = RH.run_frames(cfg, flat, imgs)
    worst = max(RH.standoff(exact[t][i], data["layer_%02d" % i][t]) for t in range(steps) for i in range(len(outs)))
    path = os.path.join(OUT, name + ".npz")
    save_npz_reproducibly(path, data)
    print(name, "layers", len(outs), "top", data["top"].tolist(), "p max", np.round(outs[-1].max(axis=1), 3).tolist(), "restatement stand-off %.2e" % worst,
          "drift bf16 %.3g fp16 %.3g" % (data["drift16_bf16"].max(), data["drift16_fp16"].max()), os.path.getsize(path), "bytes")


def mini_char_rnn_cfg():
    """darknet's rnn.cfg in miniature, one layer of each recurrent kind: a one-hot symbol of 37 in, a batch-normalised leaky [rnn] of 24, a [gru] of
    20, an [lstm] of 12, a leaky [connected] back to 37, [softmax] at temperature 0.7, [cost].  37, 20 and 12 are ragged against the 8-element
    granule and the 16-row MFMA tile.  yolo_input=vector: the key this project declares the input with; darknet ignores it."""
    return ("[net]\ninputs=37\nyolo_input=vector\n\n[rnn]\nbatch_normalize=1\noutput=24\nactivation=leaky\n\n[gru]\noutput=20\n\n[lstm]\noutput=12\n\n"
            "[connected]\noutput=37\nactivation=leaky\n\n[softmax]\ntemperature=0.7\n\n[cost]\n")


def gen_mini_char_rnn(seed=131, logit_peak=6.0):
    """mini_char_rnn_cfg through the compiled reference as examples/rnn.c test_char_rnn drives it: ONE live network, srand(rseed), a 4-token seed,
    then 8 tokens the reference's own sample_array draws from its clipped output (rnn.c:290-293), each fed back.  Recorded: every layer's output at
    each of the 11 steps (before the clip touches the output), the tokens, the uniforms sample_array consumed -- srand(rseed) again and
    (float)rand() / RAND_MAX --, per sampled step the distance of the uniform from the nearest boundary of the row's running sums (`margin`), and
    drift16_* as in mini_seq.npz.  The [connected] layer's rows are scaled until the logits peak near `logit_peak`, so that some probabilities fall
    below the clip; rseed is the first of 0 .. 15 at which every margin is at least 1e-3 and the clip changes a sampled row."""
    import ctypes as C
    import importlib.util
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    spec = importlib.util.spec_from_file_location("test_char_rnn_host", os.path.join(ROOT, "tests", "test_char_rnn_host.py"))
    CH = importlib.util.module_from_spec(spec); spec.loader.exec_module(CH)
    RH = CH.RH
    name, cfg, n_in, seed_len, sampled = "mini_char_rnn", mini_char_rnn_cfg(), 37, 4, 8
    secs = IO.parse_cfg(cfg)
    flat = IO.synth_weights(secs, seed=seed)
    seed_tokens = np.random.default_rng(seed + 1).integers(0, n_in, seed_len).astype(np.int32)
    libc = C.CDLL(None); libc.rand.restype = C.c_int
    l = D.lib(); l.sample_array.argtypes = [C.POINTER(C.c_float), C.c_int]; l.sample_array.restype = C.c_int
    nl = len(secs) - 2          # ([cost] holds nothing at inference)

    def run(weights, rseed):
        net = D.RefNet(cfg, weights, 0, 2)
        libc.srand(C.c_uint(rseed))
        outs, fed, toks = [[] for _ in range(nl)], [], []
        x = np.zeros(n_in, dtype=np.float32)
        def predict(c):
            x[:] = 0; x[c] = 1
            out = l.network_predict(net.net, x.ctypes.data_as(C.POINTER(C.c_float)))
            fed.append(c)
            for i in range(nl):
                outs[i].append(np.asarray(net.layer_output_nhwc(i), dtype=np.float32).reshape(-1))
            return out
        for c in seed_tokens[:-1]:
            predict(int(c))
        c = int(seed_tokens[-1])
        for _ in range(sampled):
            out = predict(c)
            for j in range(n_in):
                if out[j] < .0001:
                    out[j] = 0
            c = int(l.sample_array(out, n_in))
            toks.append(c)
        net.close()
        return [np.stack(o) for o in outs], np.array(fed, dtype=np.int32), np.array(toks, dtype=np.int32)

    # the [rnn] layer's self sublayer (the second of the stream: biases, then its rows) is damped: a leaky state that feeds itself through rows of
    # unit gain doubles per step, and the gates behind it would saturate within the 11 steps
    rnn = IO.recurrent_specs(secs)[0]
    at = IO.connected_floats(rnn["subs"][0][0], rnn["subs"][0][1], rnn["bn"]) + rnn["outputs"]
    flat[at:at + rnn["outputs"] * rnn["outputs"]] *= np.float32(0.25)
    # the [connected] layer's rows, scaled until the logits of the seed steps peak near logit_peak
    last = IO.conv_specs(secs)[-1]
    nw = last["filters"] * last["cin"]
    logits = run(flat, 0)[0][nl - 2]
    flat[-nw:] *= np.float32(round(logit_peak / float(np.abs(logits).max()), 2))
    for rseed in range(16):
        outs, fed, toks = run(flat, rseed)
        libc.srand(C.c_uint(rseed))
        uniforms = (np.array([libc.rand() for _ in range(sampled)], dtype=np.int64).astype(np.float32) / np.float32(2147483647)).astype(np.float32)
        probs = outs[nl - 1][seed_len - 1:]
        margin = np.array([CH.cdf_margin(probs[k], uniforms[k]) for k in range(sampled)], dtype=np.float64)
        own = [CH.sample_np(probs[k], uniforms[k]) for k in range(sampled)]
        assert own == toks.tolist(), (rseed, own, toks.tolist())          # the numpy restatement of the sampler is the reference's
        print("rseed", rseed, "tokens", toks.tolist(), "margin min %.2e" % margin.min(), "clipped", int(((probs > 0) & (probs < 1e-4)).sum()))
        if margin.min() >= 1e-3 and ((probs > 0) & (probs < 1e-4)).any() and len(set(toks.tolist())) > 1:
            break
    else:
        raise SystemExit("no rseed of 0 .. 15 meets the fixture's conditions")
    shapes = IO.layer_shapes(secs)
    data = {"cfg": np.array(cfg), "weights": flat, "seed_tokens": seed_tokens, "rseed": np.int32(rseed), "uniforms": uniforms, "tokens": toks, "fed": fed, "margin": margin}
    for i, o in enumerate(outs):
        assert np.isfinite(o).all()
        data["layer_%02d" % i] = o.reshape((len(fed),) + tuple(shapes[i][1:4]))
    for tag, store in (("bf16", RH.bf16), ("fp16", RH.fp16)):
        sim = CH.run_tokens(cfg, flat, fed, store)
        data["drift16_" + tag] = np.array([[RH.standoff(sim[t][i], data["layer_%02d" % i][t]) for i in range(nl)] for t in range(len(fed))], dtype=np.float64)
    exact = CH.run_tokens(cfg, flat, fed)
    worst = max(RH.standoff(exact[t][i], data["layer_%02d" % i][t]) for t in range(len(fed)) for i in range(nl))
    path = os.path.join(OUT, name + ".npz")
    save_npz_reproducibly(path, data)
    print(name, "rseed", rseed, "seed", seed_tokens.tolist(), "tokens", toks.tolist(), "p max", np.round(probs.max(axis=1), 3).tolist(), "margin min %.2e" % margin.min(),
          "restatement stand-off %.2e" % worst, "drift bf16 %.3g fp16 %.3g" % (data["drift16_bf16"].max(), data["drift16_fp16"].max()), os.path.getsize(path), "bytes")


def _lrn(size=None, alpha=None, beta=None, kappa=None):
    keys = [("size", size), ("alpha", alpha), ("beta", beta), ("kappa", kappa)]
    return "[normalization]\n" + "".join("%s=%s\n" % (k, v) for k, v in keys if v is not None) + "\n"


def _crop(height, width, noadjust=False):
    return "[crop]\ncrop_height=%d\ncrop_width=%d\nflip=1\nangle=0\nsaturation=1\nexposure=1\n%s\n" % (height, width, "noadjust=1\n" if noadjust else "")


def mini_lrn_cfg(height=20, width=26):
    """AlexNet's opening in miniature: a leading [crop] of the 20 high x 26 wide input to 16 x 21 (odd differences), a 3x3 conv to 13 filters, [normalization]
    size=5 with darknet's defaults, a 2/2 max-pool, a 3x3 conv to 24 filters, [normalization] size=4 alpha=0.05 kappa=1.5 -- an even window, whose two reaches
    differ, and an alpha at which the channel the reference's running sum never adds is a tenth of the sum --, a 1x1 conv to 10 classes, [avgpool], [softmax]."""
    return ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\n\n" % (width, height) + _crop(16, 21) + _conv(13, 3, bn=False) + _lrn(size=5) +
            "[maxpool]\nsize=2\nstride=2\n\n" + _conv(24, 3, bn=False) + _lrn(size=4, alpha=0.05, kappa=1.5) + _conv(10, 1, bn=False, act="linear") + "[avgpool]\n\n[softmax]\ngroups=1\n")


LRN_CASES = [(7, 5), (13, 6), (9, 3), (5, 1), (3, 5), (2, 5), (2, 4), (96, 5), (520, 5), (24, 16)]          # (channels, size): tests/test_lrn_crop_host.py says why each
LRN_BETA_CASE = (11, 5, 0.6)          # ... and one whose beta is not the default: the kernel's other power
LRN_ALPHA, LRN_KAPPA = 0.05, 1.5
CROP_CASES = [("odd", 11, 14, 8, 9, False, 0), ("noadjust", 11, 14, 8, 9, True, 0), ("whole", 11, 14, 11, 14, False, 0), ("conv20", 11, 14, 8, 9, False, 20)]      # (name, H, W, crop_h, crop_w, noadjust, channels of a 3x3 conv in front)
# (name, network h, w, image h, w): darknet's validation fit, resize_min(im, net_w) then the centred crop_image
FIT_CASES = [("landscape", 16, 16, 20, 33), ("portrait", 16, 16, 37, 19), ("same", 16, 16, 16, 23), ("upscale", 16, 16, 9, 13), ("one_wide", 16, 16, 21, 1), ("rect_short", 24, 16, 30, 40)]


def gen_lrn_crop(seed=109):          # (a seed at which channel 2 of mini_lrn's second conv -- the one its [normalization] never adds -- is of the tensor's own size; biases of N(0, 1) decide that)
    """[normalization], [crop] and the classifier's validation fit through the compiled reference (normalization_layer.c, crop_layer.c; image.c
    resize_min + crop_image).  mini_lrn.npz: mini_lrn_cfg, weights, three images, every layer's output for each of them (separate predicts).
    lrn_crop_cases.npz: per LRN case a 1x1 linear conv + [normalization] on a 5 x 7 input -- the conv's output is lrn_C_size_x, the layer's lrn_C_size_y --;
    per [crop] case cfg, weights, one image and every layer's output; per fit case a seeded uint8 image and the reference's float network input.
    Asserted here: leaving the never-added channel out of the closed form (tests/test_lrn_crop_host.py lrn_ref) moves mini_lrn's second [normalization] by
    more than twenty times the 5e-4 bound of the fp32 network test, and every stand-alone case that has such a channel by far more than fp32 rounding --
    else the fixtures would not pin it."""
    import ctypes as C
    import importlib.util
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    spec = importlib.util.spec_from_file_location("test_lrn_crop_host", os.path.join(ROOT, "tests", "test_lrn_crop_host.py"))
    sys.path.insert(0, os.path.join(ROOT, "tests")); LH = importlib.util.module_from_spec(spec); spec.loader.exec_module(LH)

    def run(cfg, flat, x):
        net = D.RefNet(cfg, flat, 0, 2)
        net.predict(x)
        outs = [np.asarray(net.layer_output_nhwc(i), dtype=np.float32) for i in range(net.n)]
        net.close()
        return outs

    def pins_ghost(x, y, size, alpha, beta, kappa):
        with_g = LH.lrn_ref(x, size, alpha, beta, kappa); without = LH.lrn_ref(x, size, alpha, beta, kappa, ghost=False)
        assert np.abs(with_g - y).max() < 1e-5 * np.abs(y).max(), "the closed form does not give the reference's output"
        return float(np.abs(without - y).max() / np.abs(y).max())

    # ---- mini_lrn ----
    cfg = mini_lrn_cfg(); secs = IO.parse_cfg(cfg); shapes = IO.layer_shapes(secs)
    flat = IO.synth_weights(secs, seed=seed)
    last = IO.conv_specs(secs)[-1]
    tail = last["filters"] * (1 + last["cin"] * last["size"] ** 2)
    imgs = np.random.default_rng(seed + 1).integers(0, 256, (3, 20, 26, 3), dtype=np.uint8)
    x = imgs.astype(np.float32) / np.float32(255.0)
    logit_layer = len(secs) - 4
    # the second conv (bias and filters; leaky is homogeneous), until its output's root mean square is 1.5: at alpha = 0.05 the never-added channel is then
    # about a tenth of norms.  Then the class conv, until the logits reach +-5 (gen_mini_cls)
    first, second = IO.conv_specs(secs)[:2]
    lo = first["filters"] * (1 + first["cin"] * first["size"] ** 2); hi = lo + second["filters"] * (1 + second["cin"] * second["size"] ** 2)
    flat[lo:hi] *= np.float32(round(1.5 / float(np.sqrt(np.mean(run(cfg, flat, x[0])[4].astype(np.float64) ** 2))), 2))
    flat[-tail:] *= np.float32(round(5.0 / float(np.abs(run(cfg, flat, x[0])[logit_layer]).max()), 2))
    per_image = [run(cfg, flat, x[b]) for b in range(3)]
    data = {"cfg": np.array(cfg), "weights": flat, "images_u8": imgs, "logit_layer": np.int32(logit_layer)}
    for i in range(len(shapes)):
        data["layer_%02d" % i] = np.stack([o[i].reshape(shapes[i][1:4]) for o in per_image])
        assert np.isfinite(data["layer_%02d" % i]).all()
    data["max_abs_logit"] = np.float32(np.abs(data["layer_%02d" % logit_layer]).max())
    pooled = data["layer_%02d" % (len(shapes) - 2)].reshape(3, -1)
    top2 = np.sort(pooled, axis=-1)[:, -2:]
    data["top1_margin"] = (top2[:, 1] - top2[:, 0]).astype(np.float32)
    assert float(data["top1_margin"].min()) > 2 * TOL16_BF16 * float(np.abs(pooled).max()), "a top-1 margin below twice the bf16 bound: change the seed, not the rule"
    gap = pins_ghost(data["layer_04"], data["layer_05"], 4, 0.05, 0.75, 1.5)
    assert gap > 20 * MARGIN_TOL, "mini_lrn: the never-added channel moves the second [normalization] by %.2e of its scale only" % gap
    pins_ghost(data["layer_01"], data["layer_02"], 5, 1e-4, 0.75, 1.0)
    path = os.path.join(OUT, "mini_lrn.npz")
    save_npz_reproducibly(path, data)
    print("mini_lrn layers", len(shapes), "max|logit| %.2f" % float(data["max_abs_logit"]), "top-1 margins", data["top1_margin"], "ghost gap %.3f of the scale" % gap, os.path.getsize(path), "bytes")

    # ---- stand-alone cases ----
    data = {"lrn_alpha": np.float32(LRN_ALPHA), "lrn_kappa": np.float32(LRN_KAPPA)}
    rng = np.random.default_rng(seed + 2)
    for k, (ch, size, beta) in enumerate([(c, s, 0.75) for c, s in LRN_CASES] + [LRN_BETA_CASE]):
        cfg = "[net]\nbatch=1\nwidth=7\nheight=5\nchannels=3\n\n" + _conv(ch, 1, bn=False, act="linear") + _lrn(size, LRN_ALPHA, beta, LRN_KAPPA)
        secs = IO.parse_cfg(cfg)
        outs = run(cfg, IO.synth_weights(secs, seed=seed + 10 + k), rng.random((5, 7, 3), dtype=np.float32))
        tag = "lrn_%d_%d" % (ch, size) + ("" if beta == 0.75 else "_beta")
        data[tag + "_x"], data[tag + "_y"] = outs[0][0], outs[1][0]
        if beta != 0.75:
            data[tag] = np.float32(beta)
        gap = pins_ghost(outs[0][0], outs[1][0], size, LRN_ALPHA, beta, LRN_KAPPA)
        assert (gap > 100 * 2.0 ** -20) == (size // 2 < ch), (tag, gap)
        print(tag, "max|x| %.2f" % float(np.abs(outs[0]).max()), "ghost gap %.3g of the scale" % gap)
    for name, h, w, ch_, cw_, noadjust, front in CROP_CASES:
        cfg = ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\n\n" % (w, h) + (_conv(front, 3, bn=False) if front else "") + _crop(ch_, cw_, noadjust) +
               _conv(6, 1, bn=False, act="linear"))
        secs = IO.parse_cfg(cfg); shapes = IO.layer_shapes(secs)
        flat = IO.synth_weights(secs, seed=seed + 40)
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        outs = run(cfg, flat, img.astype(np.float32) / np.float32(255.0))
        data["crop_%s_cfg" % name], data["crop_%s_weights" % name], data["crop_%s_image_u8" % name] = np.array(cfg), flat, img
        for i, o in enumerate(outs):
            data["crop_%s_layer_%02d" % (name, i)] = o[0]
            assert o[0].shape == shapes[i][1:4]
    # the fit: darknet's `image` by value (DN/include/darknet.h: w, h, c, data), planar float
    class IMAGE(C.Structure):
        _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]
    lib = D.lib()
    lib.resize_min.argtypes = [IMAGE, C.c_int]; lib.resize_min.restype = IMAGE
    lib.crop_image.argtypes = [IMAGE, C.c_int, C.c_int, C.c_int, C.c_int]; lib.crop_image.restype = IMAGE
    lib.free_image.argtypes = [IMAGE]
    for name, nh, nw, h, w in FIT_CASES:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        chw = np.ascontiguousarray((img.astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1))          # darknet's loader: (float)p / 255.
        im = IMAGE(w, h, 3, chw.ctypes.data_as(C.POINTER(C.c_float)))
        resized = lib.resize_min(im, nw)
        crop = lib.crop_image(resized, int((resized.w - nw) / 2), int((resized.h - nh) / 2), nw, nh)      # (C's division truncates toward zero: int() of the quotient, not //)
        out = np.ctypeslib.as_array(crop.data, shape=(3, nh, nw)).copy().transpose(1, 2, 0)
        data["fit_%s_image_u8" % name], data["fit_%s_net_hw" % name], data["fit_%s_input" % name] = img, np.array([nh, nw], np.int32), np.ascontiguousarray(out)
        data["fit_%s_resized_hw" % name] = np.array([resized.h, resized.w], np.int32)
        same = C.addressof(resized.data.contents) == chw.ctypes.data
        print("fit", name, "image %dx%d -> resized %dx%d%s -> network %dx%d" % (h, w, resized.h, resized.w, " (no resize)" if same else "", nh, nw))
        assert same == (name == "same")
        if not same:
            lib.free_image(resized)
        lib.free_image(crop)
    path = os.path.join(OUT, "lrn_crop_cases.npz")
    save_npz_reproducibly(path, data)
    print("lrn_crop_cases", len(data), "arrays", os.path.getsize(path), "bytes")


def _planes_net(width, height, channels, extra=""):
    return "[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=%d\n%s\n" % (width, height, channels, extra)


# Image networks whose channel count is not three, as darknet reads them: the cfgs carry NO yolo_input key (the library's loaders add it:
# darknet_io.with_planes_input, the veneer's load_network).  Each opens with the shape of one fused first-stage kernel of the 3-channel path, which
# must not be chosen for them: (name, cfg, (h, w, c), seed)
PLANES_NETS = [
    # the fused stem's shape: 3x3/1 -> 32, 3x3/2 -> 64, batch-normalised, leaky; a 1x1 head of 3 anchors x (5 + 2 classes) and [yolo]
    ("mini_planes_grey", _planes_net(32, 32, 1) + _conv(32, 3) + _conv(64, 3, 2) + _conv(21, 1, bn=False, act="linear") +
     "[yolo]\nmask=0,1,2\nanchors=4,5, 9,8, 14,17\nclasses=2\nnum=3\n", (32, 32, 1), 141),
    # the space-to-depth 7x7 / stride 2 / pad 3 first conv (even extents), a max-pool, a conv to ten classes, [avgpool], [softmax]
    ("mini_planes_rgbd", _planes_net(30, 22, 4) + "[convolutional]\nbatch_normalize=1\nfilters=16\nsize=7\nstride=2\npad=1\nactivation=leaky\n\n" +
     "[maxpool]\nsize=2\nstride=2\n\n" + _conv(10, 3, bn=False, act="linear") + "[avgpool]\n\n[softmax]\ngroups=1\n", (22, 30, 4), 143),
    # a first-layer [crop] of nine planes (two granules, the second with one real channel), a 5x5 conv, a stride-2 deconv, a linear 1x1: a map
    ("mini_planes_nine", _planes_net(22, 15, 9, "yolo_output=map\n") + _crop(13, 20) + _conv(12, 5) + _deconv(8, 2, 2, 0) + _conv(5, 1, bn=False, act="linear"), (15, 22, 9), 145),
    # seventeen planes (three granules) into a 1x1 first conv, then a linear 3x3: a map
    ("mini_planes_17", _planes_net(11, 9, 17, "yolo_output=map\n") + _conv(12, 1) + _conv(8, 3, bn=False, act="linear"), (9, 11, 17), 147),
]
# (planes, image h, w) of the fit cases, network 16 x 16: one image wider and one taller than the network per plane count, odd sizes
PLANES_FIT_NET = (16, 16)
PLANES_FIT_CASES = [(1, 21, 37), (1, 35, 19), (4, 13, 29), (4, 27, 15), (9, 17, 23), (9, 31, 11)]


def gen_planes(thresh=0.15):
    """The networks of PLANES_NETS through the compiled reference: cfg text (darknet's own, without yolo_input), the seeded weight stream (filters
    bf16-exact), one uint8 image [h, w, c] and every layer's output of network_predict on image / 255, `layer_%02d` [1, h, w, c]; mini_planes_grey also the
    reference's get_network_boxes (boxes_raw / obj_raw / prob_raw at `thresh`, network-sized image: no letterbox correction).  planes_fit_cases.npz: the
    reference's letterbox_image and resize_min + crop_image (the classifier's validation fit) of seeded images of 1, 4 and 9 planes."""
    import ctypes as C
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    for name, cfg, (h, w, ch), seed in PLANES_NETS:
        secs = IO.parse_cfg(cfg); shapes = IO.layer_shapes(secs)
        flat = IO.bf16_exact_filters(secs, IO.synth_weights(secs, seed=seed, obj_bias=0.5))
        img = np.random.default_rng(seed + 1).integers(0, 256, (h, w, ch), dtype=np.uint8)
        net = D.RefNet(cfg, flat, 0, 2)
        assert (net.h, net.w) == (h, w)
        net.predict(img.astype(np.float32) / np.float32(255.0))
        data = {"cfg": np.array(cfg), "weights": flat, "image_u8": img}
        for i in range(net.n):
            o = np.asarray(net.layer_output_nhwc(i), dtype=np.float32)
            data["layer_%02d" % i] = o.reshape((1,) + tuple(shapes[i][1:4])) if shapes[i][0] not in ("yolo",) else o
            assert np.isfinite(o).all()
        if name == "mini_planes_grey":
            bb, obj, pr = net.boxes(thresh, None, 2)
            assert len(bb) >= 8, "too few boxes above the threshold to pin anything: %d" % len(bb)
            data["boxes_raw"], data["obj_raw"], data["prob_raw"], data["thresh"] = bb, obj, pr, np.float32(thresh)
        net.close()
        path = os.path.join(OUT, name + ".npz")
        save_npz_reproducibly(path, data)
        print(name, "layers", len(shapes), [tuple(data["layer_%02d" % i].shape[1:]) for i in range(len(shapes))], "boxes", len(data.get("boxes_raw", [])), os.path.getsize(path), "bytes")

    class IMAGE(C.Structure):
        _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]
    lib = D.lib()
    lib.resize_min.argtypes = [IMAGE, C.c_int]; lib.resize_min.restype = IMAGE
    lib.crop_image.argtypes = [IMAGE, C.c_int, C.c_int, C.c_int, C.c_int]; lib.crop_image.restype = IMAGE
    lib.letterbox_image.argtypes = [IMAGE, C.c_int, C.c_int]; lib.letterbox_image.restype = IMAGE
    lib.free_image.argtypes = [IMAGE]
    nh, nw = PLANES_FIT_NET
    rng = np.random.default_rng(149)
    data = {"net_hw": np.array([nh, nw], np.int32), "cases": np.array(PLANES_FIT_CASES, np.int32)}
    for ch, h, w in PLANES_FIT_CASES:
        img = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        chw = np.ascontiguousarray((img.astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1))          # darknet's loader: (float)p / 255.
        im = IMAGE(w, h, ch, chw.ctypes.data_as(C.POINTER(C.c_float)))
        boxed = lib.letterbox_image(im, nw, nh)
        resized = lib.resize_min(im, nw)
        crop = lib.crop_image(resized, int((resized.w - nw) / 2), int((resized.h - nh) / 2), nw, nh)
        tag = "fit_%d_%dx%d" % (ch, h, w)
        data[tag + "_image_u8"] = img
        data[tag + "_letterbox"] = np.ctypeslib.as_array(boxed.data, shape=(ch, nh, nw)).copy().transpose(1, 2, 0)
        data[tag + "_center_crop"] = np.ctypeslib.as_array(crop.data, shape=(ch, nh, nw)).copy().transpose(1, 2, 0)
        if C.addressof(resized.data.contents) != chw.ctypes.data:
            lib.free_image(resized)
        lib.free_image(crop); lib.free_image(boxed)
    path = os.path.join(OUT, "planes_fit_cases.npz")
    save_npz_reproducibly(path, data)
    print("planes_fit_cases", len(data), "arrays", os.path.getsize(path), "bytes")


def frame_average_cfgs():
    """(name, cfg text, classes, K): a yolov3-tiny-shaped net 96 high x 128 wide with 7 classes (36 head channels: 3 x 4 and 6 x 8 cells), stock yolov3-tiny and
    yolov2-tiny-voc at 96 x 96"""
    from yolo_tensorflow_amd import darknet_io as IO
    tiny = IO.cfg_text("yolov3-tiny")
    rect = IO.with_input_size(tiny.replace("classes=80", "classes=7").replace("filters=255", "filters=36"), (96, 128))
    return [("rect7", rect, 7, 3), ("tiny80", IO.with_input_size(tiny, 96), 80, 2), ("voc", IO.with_input_size(IO.cfg_text("yolov2-tiny-voc"), 96), 20, 5)]


def frame_average_frames(seed, count, h, w):
    """a fixed base image plus seeded noise of sigma 0.25 (of the 0 .. 1 range) per frame, uint8.  The noise is drawn per 8 x 8 block: white noise is
    averaged away by the first convs and pools and would move the heads' outputs by a few hundredths only"""
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3))
    noise = lambda: np.repeat(np.repeat(rng.normal(0, 0.25, (h // 8, w // 8, 3)), 8, 0), 8, 1)
    return np.stack([np.clip(np.rint((base + noise()) * 255), 0, 255).astype(np.uint8) for _ in range(count)])


def gen_frame_average(weight_seed=21, src_wh=(200, 120)):
    """demo.c's loop restated around the compiled reference: predict, remember every detection layer's l.output in ring slot (step % K), fill l.output with
    avg = 0; avg += (float)(1. / K) * slot[j] in slot order (axpy_cpu, fp32), get_network_boxes at thresh 0 for relative 1 and 0 of a 200 x 120 source image."""
    import ctypes as C
    from oracle import darknet_ref as DR
    from yolo_tensorflow_amd import darknet_io as IO
    data = {"names": np.array([c[0] for c in frame_average_cfgs()])}
    l = DR.lib()
    for name, cfg, classes, K in frame_average_cfgs():
        secs = IO.parse_cfg(cfg)
        flat = IO.synth_weights(secs, weight_seed, obj_bias=0.0)
        net = DR.RefNet(cfg, flat)
        heads = [i for i, s in enumerate(secs[1:]) if s["type"] in ("yolo", "region")]
        steps = K + 2
        frames = frame_average_frames(1000 + K, steps, net.h, net.w)
        ring = {i: np.zeros((K, l.ref_layer_outputs(net.net, i)), np.float32) for i in heads}
        alpha = np.float32(1. / K)
        data[name + "_cfg"] = np.array(cfg); data[name + "_weight_seed"] = np.array(weight_seed); data[name + "_K"] = np.array(K)
        data[name + "_frames"] = frames; data[name + "_classes"] = np.array(classes); data[name + "_src_wh"] = np.array(src_wh)
        # (float)netw / new_w and (float)neth / new_h as THIS build of the reference evaluates them in correct_*_boxes: -Ofast turns the float division
        # into a reciprocal approximation (128 / 128 comes out as 0x3f7fffff) and folds `*= w` into the same factor, so the factors are recorded, read off a unit box
        probe = (DR.DETECTION * 1)(); probe[0].bbox = DR.BOX(0.5, 0.5, 1.0, 1.0)
        fn = l.correct_yolo_boxes if secs[1 + heads[0]]["type"] == "yolo" else l.correct_region_boxes
        fn.argtypes = [C.POINTER(DR.DETECTION)] + [C.c_int] * 6; fn.restype = None
        scale = np.zeros((2, 2), np.float32)          # [relative]: what a box's (w, h) are multiplied by in all (relative = 0: the source size included, as one factor)
        for relative in (0, 1):
            probe[0].bbox = DR.BOX(0.5, 0.5, 1.0, 1.0)
            fn(probe, 1, src_wh[0], src_wh[1], net.w, net.h, relative)
            scale[relative] = (probe[0].bbox.w, probe[0].bbox.h)
        data[name + "_wh_scale"] = scale
        for t in range(steps):
            net.predict(frames[t].astype(np.float32) / np.float32(255))
            for k, i in enumerate(heads):
                out = np.ctypeslib.as_array(l.ref_layer_output(net.net, i), shape=(ring[i].shape[1],))      # a view of l.output: writable
                ring[i][t % K] = out
                data["%s_out_t%d_h%d" % (name, t, k)] = out.copy()
                avg = np.zeros_like(out)
                for j in range(K):
                    avg = avg + alpha * ring[i][j]
                out[:] = avg
            for relative in (1, 0):
                num = C.c_int(0)
                dets = l.get_network_boxes(net.net, src_wh[0], src_wh[1], 0.0, .5, None, relative, C.byref(num))
                n = num.value
                bb = np.zeros((n, 4), np.float32); obj = np.zeros(n, np.float32); pr = np.zeros((n, classes), np.float32)
                for d in range(n):
                    bb[d] = (dets[d].bbox.x, dets[d].bbox.y, dets[d].bbox.w, dets[d].bbox.h); obj[d] = dets[d].objectness
                    pr[d] = np.ctypeslib.as_array(dets[d].prob, shape=(classes,))
                l.free_detections(dets, n)
                data["%s_bbox_t%d_rel%d" % (name, t, relative)] = bb
                if relative:
                    data["%s_obj_t%d" % (name, t)] = obj; data["%s_prob_t%d" % (name, t)] = pr
            # the gap the GPU test needs at every step: more than 20 boxes above a hole of 8e-3 in the reference's objectness
            cand = np.sort(obj)[::-1]
            gaps = [k for k in range(20, len(cand) - 1) if cand[k] - cand[k + 1] > 8e-3]
            print("  %s step %d: %d boxes, objectness %.3f .. %.3f, first gap after %s" % (name, t, n, cand[-1], cand[0], gaps[:1]))
            assert gaps, "no objectness gap wider than 8e-3 below the 21st box"
        net.close()
    path = os.path.join(OUT, "frame_average_cases.npz")
    save_npz_reproducibly(path, data)
    print("frame_average_cases", len(data), "arrays", os.path.getsize(path), "bytes")


def _local(filters, size, stride, pad, act):
    return "[local]\nsize=%d\nstride=%d\npad=%d\nfilters=%d\nactivation=%s\n\n" % (size, stride, pad, filters, act)


def _detection(side, num, classes, sqrt):
    return "[detection]\nclasses=%d\ncoords=4\nrescore=1\nside=%d\nnum=%d\nsoftmax=0\nsqrt=%d\n" % (classes, side, num, sqrt)


def mini_v1_edges_cfg(height=6, width=10):
    """The YOLOv1 family at the edges of its kernels, 6 high x 10 wide.  Layer by layer (H x W x C):
      0 conv 3x3 -> 64, bn, leaky                               6 x 10 x 64
      1 conv 3x3 -> 64, bn, leaky                               6 x 10 x 64   (its im2col workspace, 60 * 9 * 64 floats, is the one the [local] layers lean on)
      2 maxpool 2/2                                             3 x  5 x 64
      3 [local] 3x3 / 1 / pad 1 -> 13, leaky                    3 x  5 x 13   72 granules per filter row: a ragged second pass of 64 lanes; 13 filters
      4 conv 1x1 -> 16, bias, leaky                             3 x  5 x 16
      5 [local] 3x3 / 2 / pad 1 -> 8, relu                      2 x  3 x  8   stride 2 under padding
      6 [local] 2x2 / 1 / pad 0 -> 24, tanh                     1 x  2 x 24   even size, no padding, an activation outside the slope family
      7 [connected] 37, no activation key (logistic)            K = 48
      8 [connected] 68, linear                                  the head: 2 * 2 * (2 + 3 * 5)
      9 [detection] side 2, num 3, classes 2, sqrt=0"""
    return ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\n\n" % (width, height) + _econv(64, 3, pad=1, bn=True) + _econv(64, 3, pad=1, bn=True) + _pool(2, 2) +
            _local(13, 3, 1, 1, "leaky") + _econv(16, 1, pad=0) + _local(8, 3, 2, 1, "relu") + _local(24, 2, 1, 0, "tanh") +
            "[connected]\noutput=37\n\n[connected]\noutput=68\nactivation=linear\n\n" + _detection(2, 3, 2, 0))


def mini_v1_stem_cfg(height=10, width=14):
    """The 7x7 / 2 / pad 3 first conv where its space-to-depth form has odd extents below the 4 x 4 window's reach, 10 high x 14 wide:
      0 conv 7x7 / 2 -> 20, bias, leaky                         5 x  7 x 20
      1 conv 1x1 -> 8, bias, leaky                              5 x  7 x  8
      2 [connected] 7, linear                                   K = 5 * 7 * 8 = 280: no multiple of 64, a rectangular CHW flatten
      3 [detection] side 1, num 1, classes 2, sqrt=1"""
    return ("[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\n\n" % (width, height) + _econv(20, 7, stride=2, pad=1) + _econv(8, 1, pad=0) +
            "[connected]\noutput=7\nactivation=linear\n\n" + _detection(1, 1, 2, 1))


V1_EDGES_NETS = [("mini_v1_edges", mini_v1_edges_cfg, (6, 10), 171, 2), ("mini_v1_stem", mini_v1_stem_cfg, (10, 14), 173, 2)]


def gen_mini_v1_edges(out_dir=None, thresh=0.2):
    """mini_v1_edges_cfg and mini_v1_stem_cfg through the compiled reference (local_layer.c, connected_layer.c, detection_layer.c), gen_mini_local's
    recipe for three images: cfg text, the seeded weight stream, three uint8 images, every layer's output of network_predict on image / 255 (one predict per
    image), and get_network_boxes -> get_detection_detections per image (boxes_raw [3, rows, 4] in network pixels, obj_raw, prob_raw at `thresh`).
    Checked here: every [local] layer's im2col workspace (which the reference sizes in elements, DN/local_layer.c:64) fits in layer 1's, and the seed leaves
    at most 5 % of the (box, class) scores within 1e-3 of the threshold.  Fixed member dates.  -> the paths written."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    paths = []
    for name, make, (h, w), seed, classes in V1_EDGES_NETS:
        cfg = make(); secs = IO.parse_cfg(cfg); shapes = IO.layer_shapes(secs)
        conv_ws = [sh[1] * sh[2] * int(s["size"]) ** 2 * sh[4] * 4 for s, sh in zip(secs[1:], shapes) if s["type"] == "convolutional"]
        for s, sh in zip(secs[1:], shapes):
            if s["type"] == "local":
                need = sh[1] * sh[2] * int(s["size"]) ** 2 * sh[4] * 4
                assert need < max(conv_ws), "[local] workspace of %d bytes, the largest conv's is %d" % (need, max(conv_ws))
        flat = IO.synth_weights(secs, seed=seed)
        imgs = np.random.default_rng(seed + 1).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
        net = D.RefNet(cfg, flat, 0, 2)
        assert (net.h, net.w) == (h, w) and net.n == len(shapes)
        outs = [[] for _ in range(net.n)]; bb, obj, pr = [], [], []
        for b in range(3):
            net.predict(imgs[b].astype(np.float32) / np.float32(255.0))
            for i in range(net.n):
                outs[i].append(np.asarray(net.layer_output_nhwc(i), dtype=np.float32).reshape(-1))
            r = net.boxes(thresh, None, classes)
            bb.append(r[0]); obj.append(r[1]); pr.append(r[2])
        net.close()
        data = {"cfg": np.array(cfg), "weights": flat, "images_u8": imgs, "thresh": np.float32(thresh)}
        for i in range(net.n):
            o = np.stack(outs[i])
            data["layer_%02d" % i] = o.reshape((3,) + tuple(shapes[i][1:4])) if shapes[i][0] != "detection" else o
            assert np.isfinite(o).all()
        data["boxes_raw"], data["obj_raw"], data["prob_raw"] = np.stack(bb), np.stack(obj), np.stack(pr)
        cells, num = int(secs[-1]["side"]) ** 2, int(secs[-1]["num"])
        cls = np.repeat(data["layer_%02d" % (net.n - 1)][:, :cells * classes].reshape(3, cells, classes), num, axis=1)          # a cell's class scores, once per box
        near = int((np.abs(data["obj_raw"][..., None] * cls - np.float32(thresh)) <= 1e-3).sum())
        pairs = data["prob_raw"].size
        assert near * 20 <= pairs, "%s: %d of %d (box, class) scores lie within 1e-3 of the threshold: choose another seed" % (name, near, pairs)
        assert 0 < int((data["prob_raw"] > 0).sum()) < pairs, "%s: the threshold separates nothing" % name
        path = os.path.join(out_dir or OUT, name + ".npz")
        save_npz_reproducibly(path, data)
        paths.append(path)
        print(name, "layers", net.n, "boxes", data["boxes_raw"].shape, "scores above the threshold", int((data["prob_raw"] > 0).sum()), "of", pairs, "near it", near,
              os.path.getsize(path), "bytes")
    return paths


def _xconv(filters, size, stride=1, pad="pad=1", bn=True, act="leaky", xnor=True):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\n%s\n%sactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", filters, size, stride, pad, "xnor=1\n" if xnor else "", act)


_XNOR_NET = "[net]\nbatch=1\nwidth=24\nheight=24\nchannels=3\n\n"
_XNOR_STEM = _xconv(8, 3, 2, xnor=False) + "[maxpool]\nsize=2\nstride=2\n\n"          # 24 x 24 x 3 -> 12 x 12 x 8 -> 6 x 6 x 8: few values enter the first xnor layer
# a tiny-YOLO in miniature: xnor=1 on every conv but the first and the last two
MINI_XNOR = (_XNOR_NET + _XNOR_STEM + _xconv(16, 3) + _xconv(24, 3) + _xconv(16, 1) + _xconv(32, 3, xnor=False) + _xconv(16, 1, bn=False, act="linear", xnor=False) +
             "[yolo]\nmask=0,1\nanchors=3,4,  8,6,  10,14\nclasses=3\nnum=3\n")
# a classifier whose xnor layers differ in shape: 12 filters over 8 channels; a 5x5 with padding=1 over 12 channels; a stride-2 3x3 with a bias; a 1x1 with tanh (a post-activation)
XNOR_LAYER_CASES = (_XNOR_NET + _XNOR_STEM + _xconv(12, 3) + _xconv(20, 5, pad="padding=1") + _xconv(16, 3, 2, bn=False) + _xconv(24, 1, act="tanh") +
                    _xconv(32, 3, xnor=False) + _xconv(10, 1, bn=False, act="linear", xnor=False) + "[avgpool]\n\n[softmax]\ngroups=1\n")
XNOR_MARGIN = 5e-4          # MARGIN_TOL of the fp32 network tests: a value this close to zero (as a share of its tensor's largest) may change sign on the device


def xnor_inputs_clear(secs, layers):
    """no value entering an xnor layer is non-zero and within XNOR_MARGIN * max|tensor| of zero (an exact zero is -1 on both sides)"""
    for i, s in enumerate(secs[1:]):
        if s["type"] == "convolutional" and int(s.get("xnor", 0)):
            x = np.abs(layers[i - 1])
            if ((x > 0) & (x <= XNOR_MARGIN * x.max())).any():
                return False
    return True


def gen_xnor(first_seed=301, tries=4000, thresh=0.6):
    """MINI_XNOR and XNOR_LAYER_CASES through the compiled reference (convolutional_layer.c with l.xnor: binarize_weights, binarize_cpu, im2col, gemm):
    cfg text, weights, one image, every layer's output, the detector's get_network_boxes, and per xnor layer `alpha_NN`: the magnitude the reference's own
    binarize_weights gives each filter.  The weight seed is the first from `first_seed` at which
    xnor_inputs_clear holds in the reference's run: otherwise an fp32 device run may flip a sign and an end-to-end comparison means nothing."""
    from oracle import darknet_ref as D
    from yolo_tensorflow_amd import darknet_io as IO
    for name, cfg, classes in (("mini_xnor", MINI_XNOR, 3), ("xnor_layer_cases", XNOR_LAYER_CASES, 0)):
        secs = IO.parse_cfg(cfg)
        img = np.random.default_rng(first_seed - 1).integers(0, 256, (24, 24, 3), dtype=np.uint8)
        x = img.astype(np.float32) / np.float32(255.0)
        for seed in range(first_seed, first_seed + tries):
            flat = IO.synth_weights(secs, seed=seed, obj_bias=0.5)
            net = D.RefNet(cfg, flat, 0, 2)
            net.predict(x)
            layers = [np.asarray(net.layer_output_nhwc(i), dtype=np.float32) for i in range(net.n)]
            if xnor_inputs_clear(secs, layers):
                break
            net.close()
        else:
            raise SystemExit("%s: no seed in %d tries" % (name, tries))
        data = {"cfg": np.array(cfg), "weights": flat, "image_u8": img, "seed": np.int32(seed)}
        for i in range(net.n):
            data["layer_%02d" % i] = layers[i].reshape(-1) if secs[i + 1]["type"] in ("avgpool", "softmax") else layers[i]
        import ctypes as C
        p = 0
        for c in IO.conv_specs(secs):
            nb, per = c["filters"] * (4 if c["bn"] else 1), c["cin"] * c["size"] ** 2
            if int(secs[1 + c["index"]].get("xnor", 0)):
                w = np.ascontiguousarray(flat[p + nb:p + nb + c["filters"] * per]); out = np.empty_like(w)
                fp = C.POINTER(C.c_float)
                D.lib().binarize_weights(w.ctypes.data_as(fp), C.c_int(c["filters"]), C.c_int(per), out.ctypes.data_as(fp))
                out = out.reshape(c["filters"], per)
                assert (np.abs(out) == np.abs(out[:, :1])).all() and ((out > 0) == (w.reshape(c["filters"], per) > 0)).all()
                data["alpha_%02d" % c["index"]] = np.abs(out[:, 0]).copy()
            p += nb + c["filters"] * per
        assert p == flat.size
        if classes:
            bb, obj, pr = net.boxes(thresh, None, classes)
            data["boxes_raw"], data["obj_raw"], data["prob_raw"] = bb, obj, pr
            data["thresh"] = np.float32(thresh)
            assert 3 <= len(bb) <= 60, "the threshold should cut the 72 candidates: %d pass" % len(bb)
        net.close()
        path = os.path.join(OUT, name + ".npz")
        save_npz_reproducibly(path, data)
        print(name, "seed", seed, "layers", len(layers), "boxes", len(data.get("boxes_raw", [])), os.path.getsize(path), "bytes")


def gen_rect():
    gen_mini_rect("mini_v3_rect", MINI_V3, 4, 64, 96, letterbox=True)
    gen_mini_rect("mini_v2_rect", MINI_V2, 5, 96, 64)
    gen_mini_cls_rect()


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    if sys.argv[1:] == ["bn_real"]:
        gen_bn_real(); sys.exit(0)
    if sys.argv[1:] == ["known_answers"]:
        gen_known_answers(); sys.exit(0)
    if sys.argv[1:] == ["mini_resnet"]:
        gen_mini_resnet(); sys.exit(0)
    if sys.argv[1:] == ["mini_unet"]:
        gen_mini_unet(); sys.exit(0)
    if sys.argv[1:] == ["mini_grouped"]:
        gen_mini_grouped(); sys.exit(0)
    if sys.argv[1:] == ["mini_wide"]:
        gen_mini_wide(); sys.exit(0)
    if sys.argv[1:] == ["darknet_py_symbols"]:
        gen_darknet_py_symbols(); sys.exit(0)
    if sys.argv[1:] == ["rect"]:
        gen_rect(); sys.exit(0)
    if sys.argv[1:] == ["edges"]:
        gen_edges(); sys.exit(0)
    if sys.argv[1:] == ["recurrent"]:
        gen_recurrent(); sys.exit(0)
    if sys.argv[1:] == ["lrn_crop"]:
        gen_lrn_crop(); sys.exit(0)
    if sys.argv[1:] == ["char_rnn"]:
        gen_mini_char_rnn(); sys.exit(0)
    if sys.argv[1:] == ["planes"]:
        gen_planes(); sys.exit(0)
    if sys.argv[1:] == ["v1_edges"]:
        gen_mini_v1_edges(); sys.exit(0)
    if sys.argv[1:] == ["--frame-average"]:
        gen_frame_average(); sys.exit(0)
    if sys.argv[1:] == ["--xnor"]:
        gen_xnor(); sys.exit(0)
    stub_modules()
    gen_nms_v3()
    gen_v2_post()
    gen_mini("mini_v3", MINI_V3, 4)
    gen_mini("mini_v2", MINI_V2, 5)
    gen_mini_v1()
    gen_mini_local()
    gen_mini_cls()
    gen_mini_resnet()
    gen_mini_unet()
    gen_mini_grouped()
    gen_mini_wide()
    gen_rect()
    gen_edges()
    gen_recurrent()
    gen_lrn_crop()
    gen_mini_char_rnn()
    gen_planes()
    gen_frame_average()
    gen_mini_v1_edges()
    gen_xnor()
    gen_bn_real()
    gen_known_answers()
    gen_darknet_py_symbols()
