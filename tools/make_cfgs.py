#!/usr/bin/env python3
"""Author the Darknet topology descriptions (`*.cfg`) shipped in yolo_tensorflow_amd/cfg/.

The reference ships no cfg/ directory (SURVEY.md 8c gotcha 1); these are written from the
reference's layer tables and TF graph builders:
  yolov3          V3/yolov3.txt:2-107  == V3/yolo_v3.py:15-44,93-102,195-267
  yolov3-tiny     D2T/YOLO_V3_Tiny_convert_darkenet_to_Tensorflow.py:376-465 (anchors :29)
  yolov2          V2/yolov2.txt:2-32   == V2/model_darknet19_slim.py:119-200 (anchors V2/config.py:7-11)
  yolov2-tiny-voc D2T/YOLO_V2_Tiny_Voc_convert_darkenet_to_Tensorflow.py:162-225
  darknet19 / darknet53
                  the classifiers those two backbones are (cfg layers 0-22 of yolov2 / 0-74 of yolov3, same tables) with the tail the
                  reference's parser reads: [avgpool] (DN/parser.c:493-507), [softmax] (:268-280), 1000 classes, 256 x 256
  resnet18 / 34 / 50 / 101 / 152, resnext50 / 101 / 152, vgg-16
                  written from the architectures (He et al. 2015, Simonyan & Zisserman 2014) in the layer vocabulary of darknet's own model
                  zoo: see resnet() and vgg16() below.  What they need of the reference is its general [shortcut] (DN/blas.c:68-92) and
                  the activations of DN/activations.h
  yolov1          V1/YOLO_V1_Inference.py:124-210 (`_build_network`: 24 bias convs, 7x7/2 first, four SAME pools, CHW flatten,
                  FC 50176 -> 512 -> 4096 -> 1470) + :213-270 ([detection]: side 7, 2 boxes, 20 classes, sqrt sizes); the two
                  `yolo_input_*` keys of [net] state its input normalisation (x/255)*2-1 (:67-71) for the HIP planner (darknet ignores them)
The key names are the ones the reference's cfg parser reads (DN/parser.c:177-205 convolutional,
:303-339 yolo, :341-391 region, :471-486 maxpool, :527-545 shortcut, :580-587 upsample,
:589-628 route, reorg :447-459), so the same text drives three consumers: the HIP library's
planner, oracle/yolo_ref.py and the compiled reference in oracle/_ref.

Run:  python tools/make_cfgs.py   (idempotent; output is committed)
"""
import os

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "yolo_tensorflow_amd", "cfg")


class Cfg:
    def __init__(self, size, channels=3, extra=()):
        self.lines = ["[net]", "batch=1", "subdivisions=1", f"width={size}", f"height={size}",
                      f"channels={channels}"] + list(extra) + [""]
        self.n = 0  # next layer index

    def _sec(self, name, **kv):
        self.lines.append(f"[{name}]")
        for k, v in kv.items():
            self.lines.append(f"{k}={v}")
        self.lines.append("")
        self.n += 1
        return self.n - 1

    def conv(self, filters, size, stride=1, bn=True, act="leaky", groups=1, xnor=False):
        kv = {}
        if bn:
            kv["batch_normalize"] = 1
        kv.update(filters=filters, size=size, stride=stride, pad=1, activation=act)
        if groups != 1:
            kv["groups"] = groups            # DN/parser.c:184
        if xnor:
            kv["xnor"] = 1                   # DN/parser.c:198
        return self._sec("convolutional", **kv)

    def shortcut(self, frm, act="linear"):
        return self._sec("shortcut", **{"from": frm, "activation": act})

    def route(self, *layers):
        return self._sec("route", layers=",".join(str(l) for l in layers))

    def upsample(self, stride=2):
        return self._sec("upsample", stride=stride)

    def maxpool(self, size=2, stride=2):
        return self._sec("maxpool", size=size, stride=stride)

    def reorg(self, stride=2):
        return self._sec("reorg", stride=stride)

    def yolo(self, mask, anchors, classes):
        return self._sec("yolo", mask=",".join(map(str, mask)),
                         anchors=",  ".join(f"{a},{b}" for a, b in anchors),
                         classes=classes, num=len(anchors), jitter=.3, ignore_thresh=.7,
                         truth_thresh=1, random=0)

    def region(self, anchors, classes):
        return self._sec("region", anchors=",  ".join(f"{a},{b}" for a, b in anchors),
                         bias_match=1, classes=classes, coords=4, num=len(anchors), softmax=1,
                         jitter=.3, rescore=1, object_scale=5, noobject_scale=1, class_scale=1,
                         coord_scale=1, absolute=1, thresh=.6, random=0)

    def connected(self, output, act="leaky"):
        return self._sec("connected", output=output, activation=act)

    def dropout(self, p=.5):
        return self._sec("dropout", probability=p)

    def detection(self, classes=20, side=7, num=2):
        return self._sec("detection", classes=classes, coords=4, rescore=1, side=side, num=num, softmax=0, sqrt=1,
                         jitter=.2, object_scale=1, noobject_scale=.5, class_scale=1, coord_scale=5)

    def avgpool(self):
        return self._sec("avgpool")

    def deconv(self, filters, size, stride, padding, bn=True, act="leaky"):
        kv = {"batch_normalize": 1} if bn else {}
        kv.update(filters=filters, size=size, stride=stride, padding=padding, activation=act)
        return self._sec("deconvolutional", **kv)

    def logistic(self):
        return self._sec("logistic")

    def softmax(self, groups=1, temperature=None):
        kv = {"groups": groups}
        if temperature is not None:
            kv["temperature"] = temperature
        return self._sec("softmax", **kv)

    def crnn(self, hidden, output, act="leaky", bn=True, shortcut=False):          # DN/parser.c:207-220
        kv = {"batch_normalize": 1} if bn else {}
        kv.update(hidden_filters=hidden, output_filters=output, activation=act)
        if shortcut:
            kv["shortcut"] = 1
        return self._sec("crnn", **kv)

    def gru(self, output, tanh=True, bn=False):                                      # DN/parser.c:236-245
        kv = {"batch_normalize": 1} if bn else {}
        kv.update(output=output, tanh=int(tanh))
        return self._sec("gru", **kv)

    def lstm(self, output, bn=False):                                                # DN/parser.c:247-255
        kv = {"batch_normalize": 1} if bn else {}
        kv.update(output=output)
        return self._sec("lstm", **kv)

    def cost(self):
        return self._sec("cost")        # (type defaults to sse, DN/parser.c:419)

    def text(self):
        return "\n".join(self.lines)


V3_ANCHORS = [(10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326)]
V3_TINY_ANCHORS = [(10, 14), (23, 27), (37, 58), (81, 82), (135, 169), (344, 319)]
V2_ANCHORS = [(0.57273, 0.677385), (1.87446, 2.06253), (3.33843, 5.47434), (7.88282, 3.52778), (9.77052, 9.16828)]
V2_TINY_VOC_ANCHORS = [(1.08, 1.19), (3.42, 4.41), (6.63, 11.38), (9.42, 5.11), (16.62, 10.52)]


def darknet53_backbone(c):
    """cfg layers 0-74 of yolov3: the stem conv and the five residual stages; -> the two layers the detector routes back to."""
    c.conv(32, 3)

    def stage(filters, blocks):
        c.conv(filters, 3, stride=2)
        for _ in range(blocks):
            c.conv(filters // 2, 1)
            c.conv(filters, 3)
            c.shortcut(-3)
    stage(64, 1); stage(128, 2); stage(256, 8)
    route_1 = c.n - 1           # 36
    stage(512, 8)
    route_2 = c.n - 1           # 61
    stage(1024, 4)
    return route_1, route_2


def yolov3(size=416, classes=80):
    c = Cfg(size)
    route_1, route_2 = darknet53_backbone(c)

    def yolo_block(f):
        for _ in range(2):
            c.conv(f, 1); c.conv(2 * f, 3)
        r = c.conv(f, 1)
        c.conv(2 * f, 3)
        return r
    nout = 3 * (5 + classes)
    r = yolo_block(512)
    c.conv(nout, 1, bn=False, act="linear"); c.yolo([6, 7, 8], V3_ANCHORS, classes)
    c.route(r); c.conv(256, 1); up = c.upsample(); c.route(up, route_2)
    r = yolo_block(256)
    c.conv(nout, 1, bn=False, act="linear"); c.yolo([3, 4, 5], V3_ANCHORS, classes)
    c.route(r); c.conv(128, 1); up = c.upsample(); c.route(up, route_1)
    yolo_block(128)
    c.conv(nout, 1, bn=False, act="linear"); c.yolo([0, 1, 2], V3_ANCHORS, classes)
    return c.text()


def yolov3_tiny(size=416, classes=80):
    c = Cfg(size)
    for f in (16, 32, 64, 128):
        c.conv(f, 3); c.maxpool()
    route_1 = c.conv(256, 3)    # 8
    c.maxpool()
    c.conv(512, 3)
    c.maxpool(2, 1)             # 'SAME' stride-1 pool (D2T V3_Tiny :445)
    c.conv(1024, 3)
    route_2 = c.conv(256, 1)    # 13
    c.conv(512, 3)
    nout = 3 * (5 + classes)
    c.conv(nout, 1, bn=False, act="linear"); c.yolo([3, 4, 5], V3_TINY_ANCHORS, classes)
    c.route(route_2); c.conv(128, 1); up = c.upsample(); c.route(up, route_1)
    c.conv(256, 3)
    c.conv(nout, 1, bn=False, act="linear"); c.yolo([0, 1, 2], V3_TINY_ANCHORS, classes)
    return c.text()


def yolov3_tiny_video(size=416, classes=80, recurrent=True):
    """yolov3-tiny with a [crnn] ahead of each head: the detector keeps a state map per head from frame to frame (recurrent=False: the
    same network with a 3x3 conv in the [crnn]'s place, for rate comparisons)"""
    c = Cfg(size)
    for f in (16, 32, 64, 128):
        c.conv(f, 3); c.maxpool()
    route_1 = c.conv(256, 3)
    c.maxpool()
    c.conv(512, 3)
    c.maxpool(2, 1)
    c.conv(1024, 3)
    route_2 = c.conv(256, 1)
    c.conv(512, 3)
    c.crnn(256, 512) if recurrent else c.conv(512, 3)
    nout = 3 * (5 + classes)
    c.conv(nout, 1, bn=False, act="linear"); c.yolo([3, 4, 5], V3_TINY_ANCHORS, classes)
    c.route(route_2); c.conv(128, 1); up = c.upsample(); c.route(up, route_1)
    c.conv(256, 3)
    c.crnn(128, 256) if recurrent else c.conv(256, 3)
    c.conv(nout, 1, bn=False, act="linear"); c.yolo([0, 1, 2], V3_TINY_ANCHORS, classes)
    return c.text()


def darknet19_video(size=256, classes=1000, recurrent=True):
    """darknet19's features, pooled, then a [gru] of 1024 units over the frames of a stream, a [connected] layer to the classes and
    [softmax] (the per-frame features + recurrent layer of the reference's examples/rnn_vid.c); recurrent=False: without the [gru]"""
    c = Cfg(size)
    darknet19_backbone(c)
    c.avgpool()
    if recurrent:
        c.gru(1024)
    c.connected(classes, act="linear")
    c.softmax()
    return c.text()


def darknet19_backbone(c):
    """cfg layers 0-22 of yolov2: the eighteen backbone convs and their five pools; -> the layer the detector's passthrough reads."""
    c.conv(32, 3); c.maxpool()
    c.conv(64, 3); c.maxpool()
    c.conv(128, 3); c.conv(64, 1); c.conv(128, 3); c.maxpool()
    c.conv(256, 3); c.conv(128, 1); c.conv(256, 3); c.maxpool()
    c.conv(512, 3); c.conv(256, 1); c.conv(512, 3); c.conv(256, 1)
    sc = c.conv(512, 3)         # 16
    c.maxpool()
    c.conv(1024, 3); c.conv(512, 1); c.conv(1024, 3); c.conv(512, 1); c.conv(1024, 3)
    return sc


def yolov2(size=416, classes=80):
    c = Cfg(size)
    sc = darknet19_backbone(c)
    c.conv(1024, 3)
    main = c.conv(1024, 3)      # 24
    c.route(sc)
    c.conv(64, 1)
    ro = c.reorg()
    c.route(ro, main)
    c.conv(1024, 3)
    c.conv(len(V2_ANCHORS) * (5 + classes), 1, bn=False, act="linear")
    c.region(V2_ANCHORS, classes)
    return c.text()


def yolov2_tiny_voc(size=416, classes=20):
    c = Cfg(size)
    for f in (16, 32, 64, 128, 256):
        c.conv(f, 3); c.maxpool()
    c.conv(512, 3); c.maxpool(2, 1)
    c.conv(1024, 3)
    c.conv(1024, 3)
    c.conv(len(V2_TINY_VOC_ANCHORS) * (5 + classes), 1, bn=False, act="linear")
    c.region(V2_TINY_VOC_ANCHORS, classes)
    return c.text()


def xnor_yolov2_tiny_voc(size=416, classes=20, xnor=True):
    """yolov2-tiny-voc as an XNOR-Net detector (darknet's tiny-yolo-xnor): xnor=1 on every conv but the first and the last two"""
    c = Cfg(size)
    for f in (16, 32, 64, 128, 256):
        c.conv(f, 3, xnor=xnor and f != 16); c.maxpool()
    c.conv(512, 3, xnor=xnor); c.maxpool(2, 1)
    c.conv(1024, 3, xnor=xnor)
    c.conv(1024, 3)
    c.conv(len(V2_TINY_VOC_ANCHORS) * (5 + classes), 1, bn=False, act="linear")
    c.region(V2_TINY_VOC_ANCHORS, classes)
    return c.text()


def xnor_darknet_reference(size=256, classes=1000, xnor=True):
    """darknet's reference classifier (darknet.cfg: 16 .. 1024 filters of 3x3 with a max-pool between them, a 1x1 conv to the classes, [avgpool],
    [softmax]) written likewise: xnor=1 on every conv but the first and the last two"""
    c = Cfg(size)
    for f in (16, 32, 64, 128, 256, 512):
        c.conv(f, 3, xnor=xnor and f != 16); c.maxpool()
    c.conv(1024, 3)
    c.conv(classes, 1, bn=False, act="linear")
    c.avgpool()
    c.softmax()
    return c.text()


def yolov1(size=448, classes=20):
    c = Cfg(size, extra=("yolo_input_mul=2", "yolo_input_add=-1"))
    b = dict(bn=False)
    c.conv(64, 7, stride=2, **b); c.maxpool()
    c.conv(192, 3, **b); c.maxpool()
    c.conv(128, 1, **b); c.conv(256, 3, **b); c.conv(256, 1, **b); c.conv(512, 3, **b); c.maxpool()
    for _ in range(4):
        c.conv(256, 1, **b); c.conv(512, 3, **b)
    c.conv(512, 1, **b); c.conv(1024, 3, **b); c.maxpool()
    for _ in range(2):
        c.conv(512, 1, **b); c.conv(1024, 3, **b)
    c.conv(1024, 3, **b); c.conv(1024, 3, stride=2, **b); c.conv(1024, 3, **b); c.conv(1024, 3, **b)
    c.connected(512); c.connected(4096); c.dropout(); c.connected(7 * 7 * (classes + 2 * 5), act="linear")
    c.detection(classes, 7, 2)
    return c.text()


def yolov1_tiny(size=448, classes=20):
    """D2T/YOLO_V1_Tiny_convert_darkenet_to_Tensorflow.py:256-322 `_build_network`: eight BN + leaky 3x3 convs (16 .. 1024, 256), a
    2x2 max-pool after each of the first six, the CHW flatten and one fully connected layer of S*S*(C + 5 B) = 1470 linear outputs;
    input x / 255 (`_input_process`, :212-216)."""
    c = Cfg(size)
    for f in (16, 32, 64, 128, 256, 512):
        c.conv(f, 3); c.maxpool()
    c.conv(1024, 3); c.conv(256, 3)
    c.connected(7 * 7 * (classes + 2 * 5), act="linear")
    c.detection(classes, 7, 2)
    return c.text()


def darknet53(size=256, classes=1000):
    """The ImageNet classifier the yolov3 backbone was trained as: layers 0-74, global average pool, a 1x1 conv to the classes
    (linear, no batch norm) and the softmax."""
    c = Cfg(size)
    darknet53_backbone(c)
    c.avgpool()
    c.conv(classes, 1, bn=False, act="linear")
    c.softmax()
    return c.text()


def darknet19(size=256, classes=1000):
    """... and the yolov2 backbone's: layers 0-22, the 1x1 conv to the classes on the last feature map, global average pool, softmax."""
    c = Cfg(size)
    darknet19_backbone(c)
    c.conv(classes, 1, bn=False, act="linear")
    c.avgpool()
    c.softmax()
    return c.text()


RESNET_BLOCKS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}


def resnet(depth, size=256, classes=1000):
    """ResNet-18/34 (basic blocks: 3x3, 3x3, `from=-3`) and ResNet-50/101/152 (bottlenecks: 1x1, 3x3, 1x1 to four times the width,
    `from=-4`) as darknet spells them: a 7x7/2 stem of 64 filters and a 2/2 max-pool, four stages of 64, 128, 256, 512 filters whose
    first block (from the second stage on) has stride 2 on its 3x3 conv, every conv batch-normalised and leaky but the last of a block,
    which is linear, and `[shortcut] activation=leaky` closing the block.  There are no projection convs: the first block of a stage
    adds a tensor with fewer channels -- and, from the second stage on, twice the size --, which darknet's shortcut defines as the
    first min(c1, c2) channels sampled with stride w1 / w2.  Tail: a 1x1 conv to the classes, [avgpool], [softmax]."""
    c = Cfg(size)
    c.conv(64, 7, stride=2); c.maxpool()
    bottleneck = depth >= 50
    for stage, blocks in enumerate(RESNET_BLOCKS[depth]):
        f = 64 << stage
        for b in range(blocks):
            st = 2 if stage > 0 and b == 0 else 1
            if bottleneck:
                c.conv(f, 1); c.conv(f, 3, stride=st); c.conv(4 * f, 1, act="linear"); c.shortcut(-4, act="leaky")
            else:
                c.conv(f, 3, stride=st); c.conv(f, 3, act="linear"); c.shortcut(-3, act="leaky")
    c.conv(classes, 1, bn=False, act="linear")
    c.avgpool()
    c.softmax()
    return c.text()


def resnext(depth, size=256, classes=1000, groups=32):
    """ResNeXt-50/101/152 (32x4d; Xie et al. 2016) as darknet's model zoo spells them: resnet()'s stem, stages and tail, with bottlenecks
    of 1x1 / 3x3 groups=32 / 1x1 linear + [shortcut] whose inner width is twice ResNet's: 128/256, 256/512, 512/1024, 1024/2048."""
    c = Cfg(size)
    c.conv(64, 7, stride=2); c.maxpool()
    for stage, blocks in enumerate(RESNET_BLOCKS[depth]):
        f = 128 << stage
        for b in range(blocks):
            st = 2 if stage > 0 and b == 0 else 1
            c.conv(f, 1); c.conv(f, 3, stride=st, groups=groups); c.conv(2 * f, 1, act="linear"); c.shortcut(-4, act="leaky")
    c.conv(classes, 1, bn=False, act="linear")
    c.avgpool()
    c.softmax()
    return c.text()


def dw_yolo(size=416, classes=80):
    """A depthwise-separable detector in the shape of yolov3_tiny(), for rate runs (no trained weights exist for it): the dense 3x3 first
    conv stays, every later 3x3 conv becomes a depthwise 3x3 (groups = its input channels) followed by a pointwise 1x1 to the filters;
    the two head convs are ordinary 1x1 convs."""
    c = Cfg(size)
    ch = [16]

    def sep(f):
        c.conv(ch[0], 3, groups=ch[0]); ch[0] = f
        return c.conv(f, 1)
    c.conv(16, 3); c.maxpool()
    for f in (32, 64, 128):
        sep(f); c.maxpool()
    route_1 = sep(256)
    c.maxpool()
    sep(512)
    c.maxpool(2, 1)
    sep(1024)
    route_2 = c.conv(256, 1); ch[0] = 256
    sep(512)
    nout = 3 * (5 + classes)
    c.conv(nout, 1, bn=False, act="linear"); c.yolo([3, 4, 5], V3_TINY_ANCHORS, classes)
    c.route(route_2); c.conv(128, 1); up = c.upsample(); c.route(up, route_1); ch[0] = 128 + 256
    sep(256)
    c.conv(nout, 1, bn=False, act="linear"); c.yolo([0, 1, 2], V3_TINY_ANCHORS, classes)
    return c.text()


def vgg16(size=224, classes=1000):
    """VGG-16 (configuration D): thirteen 3x3 convs with bias and relu in five groups of 64 .. 512 filters, a 2/2 max-pool behind each
    group, then [connected] 4096, 4096 (relu, with dropout) and the classes (linear), [softmax]."""
    c = Cfg(size)
    for f, n in ((64, 2), (128, 2), (256, 3), (512, 3), (512, 3)):
        for _ in range(n):
            c.conv(f, 3, bn=False, act="relu")
        c.maxpool()
    c.connected(4096, act="relu"); c.dropout()
    c.connected(4096, act="relu"); c.dropout()
    c.connected(classes, act="linear")
    c.softmax()
    return c.text()


def alexnet(size=227, classes=1000):
    """AlexNet (Krizhevsky et al. 2012) as one tower, the way darknet's model zoo spells it: 96 x 11x11 / 4 without padding, 256 x 5x5,
    384, 384, 256 x 3x3, all with bias and relu, a 3/2 max-pool without padding behind the first, the second and the last conv (227 ->
    55 -> 27 -> 13 -> 6), then [connected] 4096, 4096 (relu, with dropout) and the classes (linear), [softmax]."""
    c = Cfg(size)
    pool = lambda: c._sec("maxpool", size=3, stride=2, padding=0)
    c._sec("convolutional", filters=96, size=11, stride=4, pad=0, activation="relu"); pool()
    c.conv(256, 5, bn=False, act="relu"); pool()
    c.conv(384, 3, bn=False, act="relu")
    c.conv(384, 3, bn=False, act="relu")
    c.conv(256, 3, bn=False, act="relu"); pool()
    c.connected(4096, act="relu"); c.dropout()
    c.connected(4096, act="relu"); c.dropout()
    c.connected(classes, act="linear")
    c.softmax()
    return c.text()


def alexnet_lrn(size=256, crop=227, classes=1000):
    """The 2012 network as Caffe-era zoos carry it: `alexnet` above behind a leading [crop] of the 256 x 256 input to 227 x 227 (darknet's own
    classifier cfgs begin that way; flip / angle / saturation / exposure act while training only), with local response normalisation
    ([normalization] size=5 alpha=0.0001 beta=0.75 kappa=2) behind the max-pool of the first and of the second conv."""
    c = Cfg(size)
    pool = lambda: c._sec("maxpool", size=3, stride=2, padding=0)
    lrn = lambda: c._sec("normalization", size=5, alpha=0.0001, beta=0.75, kappa=2)
    c._sec("crop", crop_height=crop, crop_width=crop, flip=1, angle=0, saturation=1, exposure=1)
    c._sec("convolutional", filters=96, size=11, stride=4, pad=0, activation="relu"); pool(); lrn()
    c.conv(256, 5, bn=False, act="relu"); pool(); lrn()
    c.conv(384, 3, bn=False, act="relu")
    c.conv(384, 3, bn=False, act="relu")
    c.conv(256, 3, bn=False, act="relu"); pool()
    c.connected(4096, act="relu"); c.dropout()
    c.connected(4096, act="relu"); c.dropout()
    c.connected(classes, act="linear")
    c.softmax()
    return c.text()


def synthetic_tree(nodes=9418, roots=10, seed=0, max_group=120):
    """A seeded tree in darknet's file format (DN/tree.c:83-139: `name parent` lines, the children of a node one contiguous run, a
    parent below its own index): the reference ships no 9k.tree.  Breadth-first: every run of siblings is appended whole, its size
    drawn from a skewed distribution as WordNet's are (most nodes have few children, a few have many)."""
    import random
    rng = random.Random(seed)
    parent = [-1] * roots
    queue = list(range(roots))
    while len(parent) < nodes and queue:
        p = queue.pop(0)
        if rng.random() < 0.35 and len(queue) > 2:
            continue                                    # a leaf
        k = min(nodes - len(parent), 1 + int(rng.paretovariate(1.1)) if rng.random() < 0.9 else rng.randint(20, max_group))
        k = min(k, max_group)
        queue.extend(range(len(parent), len(parent) + k))
        parent.extend([p] * k)
    while len(parent) < nodes:                          # the queue ran dry: hang the rest under the last node as one run
        parent.append(len(parent) - 1) if parent[-1] != len(parent) - 2 else parent.append(parent[-1])
    return "".join("n%05d %d\n" % (i, q) for i, q in enumerate(parent))


YOLO9000_ANCHORS = [(0.77871, 1.14074), (3.00525, 4.31277), (9.22725, 9.61974)]


def yolo9000(size=544, classes=9418, tree="9k.tree"):
    """A YOLO9000-shaped detector (the other half of the YOLOv2 paper): the darknet-19 backbone, a 1x1 head of 3 x (5 + classes)
    channels and a [region] layer whose class scores are a softmax tree (DN/region_layer.c:171-181).  At 544 x 544 the grid is
    17 x 17.  `tree` names the tree file, opened relative to the working directory like darknet does."""
    c = Cfg(size)
    darknet19_backbone(c)
    c.conv(len(YOLO9000_ANCHORS) * (5 + classes), 1, bn=False, act="linear")
    c._sec("region", anchors=",  ".join(f"{a},{b}" for a, b in YOLO9000_ANCHORS), bias_match=1, classes=classes, coords=4,
           num=len(YOLO9000_ANCHORS), softmax=1, tree=tree, jitter=.2, rescore=1, object_scale=5, noobject_scale=1, class_scale=1,
           coord_scale=1, absolute=1, thresh=.6, random=0)
    return c.text()


def unet(size=416, classes=21, base=32):
    """A U-Net-shaped map network ([net] yolo_output=map; darknet ignores the key): four 3x3 conv pairs going down by stride-2 convs
    (base .. 8 x base channels), three 4/2/1 [deconvolutional] layers going up, each concatenated with the encoder tensor of its size
    (the skip connections) and followed by a 3x3 conv, a linear 1x1 conv to `classes` maps at the input's size and [logistic].  For rate
    measurements (tools/segmenter_rate.py); no trained weights exist for it."""
    c = Cfg(size, extra=["yolo_output=map"])
    skips = []
    ch = base
    c.conv(ch, 3); skips.append(c.conv(ch, 3))
    for _ in range(3):
        ch *= 2
        c.conv(ch, 3, stride=2); last = c.conv(ch, 3)
        skips.append(last)
    skips.pop()                     # the bottleneck itself is no skip
    for skip in reversed(skips):
        ch //= 2
        d = c.deconv(ch, 4, 2, 1)
        c.route(d, skip)
        c.conv(ch, 3)
    c.conv(classes, 1, bn=False, act="linear")
    c.logistic()
    return c.text()


HEADER = "# generated by tools/make_cfgs.py -- do not edit\n"


def char_rnn(inputs=256, units=1024, layers=3):
    """darknet's rnn.cfg (cfg/rnn.cfg of the reference): a one-hot byte in, three batch-normalised leaky [rnn] layers of 1024 units, a leaky
    [connected] back to the 256 symbols, [softmax], [cost].  As darknet writes it: `inputs=` and no image size; CharRNN and the darknet veneer
    add the [net] key yolo_input=vector that declares such an input here (darknet_io.with_vector_input)."""
    rnn = "[rnn]\nbatch_normalize=1\noutput=%d\nactivation=leaky\n\n" % units
    return "[net]\ninputs=%d\nbatch=1\ntime_steps=1\n\n" % inputs + rnn * layers + "[connected]\noutput=%d\nactivation=leaky\n\n[softmax]\n\n[cost]\n" % inputs


def main():
    import sys
    if len(sys.argv) > 2 and sys.argv[1] == "--char-rnn":      # python tools/make_cfgs.py --char-rnn DIR: char-rnn.cfg, darknet's rnn.cfg shape
        os.makedirs(sys.argv[2], exist_ok=True)
        with open(os.path.join(sys.argv[2], "char-rnn.cfg"), "w") as f:
            f.write(char_rnn())
        print("wrote char-rnn.cfg to", sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--unet":          # python tools/make_cfgs.py --unet DIR: unet.cfg at 416 x 416
        os.makedirs(sys.argv[2], exist_ok=True)
        with open(os.path.join(sys.argv[2], "unet.cfg"), "w") as f:
            f.write(unet() + "\n")
        print("wrote unet.cfg to", sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--video":         # python tools/make_cfgs.py --video DIR: the two recurrent cfgs of the rate measurements and their twins without the recurrent layers
        os.makedirs(sys.argv[2], exist_ok=True)
        files = {"yolov3-tiny-crnn.cfg": yolov3_tiny_video(), "yolov3-tiny-conv.cfg": yolov3_tiny_video(recurrent=False),
                 "darknet19-gru.cfg": darknet19_video(), "darknet19-fc.cfg": darknet19_video(recurrent=False)}
        for name, text in files.items():
            with open(os.path.join(sys.argv[2], name), "w") as f:
                f.write(text + "\n")
        print("wrote", ", ".join(files), "to", sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--xnor":          # python tools/make_cfgs.py --xnor DIR: the two XNOR-Net cfgs (tools/xnor_rate.py measures the first)
        os.makedirs(sys.argv[2], exist_ok=True)
        for name, text in (("yolov2-tiny-voc-xnor.cfg", xnor_yolov2_tiny_voc()), ("darknet-reference-xnor.cfg", xnor_darknet_reference())):
            with open(os.path.join(sys.argv[2], name), "w") as f:
                f.write(HEADER + text)
        print("wrote yolov2-tiny-voc-xnor.cfg and darknet-reference-xnor.cfg to", sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--dw-yolo":       # python tools/make_cfgs.py --dw-yolo DIR: dw-yolo.cfg, a depthwise-separable yolov3-tiny
        os.makedirs(sys.argv[2], exist_ok=True)
        with open(os.path.join(sys.argv[2], "dw-yolo.cfg"), "w") as f:
            f.write(dw_yolo() + "\n")
        print("wrote dw-yolo.cfg to", sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--alexnet-lrn":   # python tools/make_cfgs.py --alexnet-lrn DIR: alexnet-lrn.cfg, the file shipped as cfg/zoo/alexnet-lrn.cfg
        os.makedirs(sys.argv[2], exist_ok=True)
        with open(os.path.join(sys.argv[2], "alexnet-lrn.cfg"), "w") as f:
            f.write(HEADER + alexnet_lrn())
        print("wrote alexnet-lrn.cfg to", sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--resnext":     # python tools/make_cfgs.py --resnext DIR: the 101 and 152 depths (50 is shipped in cfg/zoo)
        os.makedirs(sys.argv[2], exist_ok=True)
        for depth in (101, 152):
            with open(os.path.join(sys.argv[2], "resnext%d.cfg" % depth), "w") as f:
                f.write(resnext(depth) + "\n")
        print("wrote resnext101.cfg and resnext152.cfg to", sys.argv[2])
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--yolo9000":      # python tools/make_cfgs.py --yolo9000 DIR: yolo9000.cfg + its seeded tree
        os.makedirs(sys.argv[2], exist_ok=True)
        with open(os.path.join(sys.argv[2], "9k.tree"), "w") as f:
            f.write(synthetic_tree())
        with open(os.path.join(sys.argv[2], "yolo9000.cfg"), "w") as f:
            f.write(yolo9000())
        print("wrote yolo9000.cfg and 9k.tree (synthetic) to", sys.argv[2])
        return
    os.makedirs(OUT, exist_ok=True)
    files = {
        "yolov1.cfg": yolov1(448), "yolov1-tiny.cfg": yolov1_tiny(448),
        "yolov3.cfg": yolov3(416), "yolov3-608.cfg": yolov3(608),
        "yolov3-tiny.cfg": yolov3_tiny(416),
        "yolov2.cfg": yolov2(416), "yolov2-tiny-voc.cfg": yolov2_tiny_voc(416),
        "darknet19.cfg": darknet19(256), "darknet53.cfg": darknet53(256),
        # cfg/zoo/: classifiers of darknet's model zoo that are no YOLO backbone (cfg/ itself is the set tests/golden/plan_tables.json pins)
        "zoo/resnet18.cfg": resnet(18), "zoo/resnet50.cfg": resnet(50), "zoo/vgg-16.cfg": vgg16(),
        "zoo/resnext50.cfg": resnext(50), "zoo/alexnet.cfg": alexnet(), "zoo/alexnet-lrn.cfg": alexnet_lrn(),
    }
    os.makedirs(os.path.join(OUT, "zoo"), exist_ok=True)
    for name, text in files.items():
        with open(os.path.join(OUT, name), "w") as f:
            f.write(HEADER + text)
        print("wrote", name)


if __name__ == "__main__":
    main()
