"""Classifier networks, host side (no GPU): the generated darknet19 / darknet53 topologies, the classifier goldens against the
compiled reference (oracle/_ref, when built) and against a float64 restatement of [avgpool] + [softmax], and the public surface."""
import ctypes as C
import os
import numpy as np
import pytest
from conftest import golden
from oracle import darknet_ref as DR
from yolo_tensorflow_amd import darknet_io as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,detector,backbone", [("darknet19", "yolov2", 23), ("darknet53", "yolov3", 75)])
def test_classifier_cfgs_share_the_detector_backbone(name, detector, backbone):
    secs = IO.parse_cfg(IO.cfg_text(name))
    det = IO.parse_cfg(IO.cfg_text(detector))
    assert secs[0]["width"] == secs[0]["height"] == "256" and secs[0]["channels"] == "3"
    assert secs[1:1 + backbone] == det[1:1 + backbone]
    tail = [s["type"] for s in secs[1 + backbone:]]
    assert tail == (["convolutional", "avgpool", "softmax"] if name == "darknet19" else ["avgpool", "convolutional", "softmax"])
    head = [s for s in secs[1 + backbone:] if s["type"] == "convolutional"][0]
    assert head["filters"] == "1000" and head["size"] == "1" and head["activation"] == "linear" and "batch_normalize" not in head
    shapes = IO.layer_shapes(secs)
    assert shapes[-1][1:4] == (1, 1, 1000)
    assert [sh[1:4] for sh in shapes if sh[0] == "avgpool"] == [(1, 1, 1000 if name == "darknet19" else 1024)]
    # no parameters in the three new section types; the stream is the backbone's plus the 1x1 conv to the classes
    assert IO.weights_count(secs) == IO.synth_weights(secs, seed=0).size
    assert IO.weights_count(secs) == sum(c["filters"] * (4 if c["bn"] else 1) + c["filters"] * c["cin"] * c["size"] ** 2 for c in IO.conv_specs(secs))
    assert not any(c["head"] for c in IO.conv_specs(secs))


def _restate_tail(g):
    """float64 numpy restatement of the tail of a classifier golden: [avgpool] = mean over the pixels, [softmax] per group
    exp(x / t - max / t) / sum -> (pooled vector or None, probabilities), from the reference's own conv outputs."""
    secs = IO.parse_cfg(str(g["cfg"]))[1:]
    types = [s["type"] for s in secs]
    sm = types.index("softmax")
    groups, temp = int(secs[sm].get("groups", 1)), float(secs[sm].get("temperature", 1))
    pooled = None
    if types[sm - 1] == "avgpool":
        pooled = g["layer_%02d" % (sm - 2)].astype(np.float64).mean(axis=(1, 2)).reshape(-1)
        x = pooled
    else:
        x = g["layer_%02d" % (sm - 1)].astype(np.float64).reshape(-1)
    x = x.reshape(groups, -1) / temp
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return pooled, (e / e.sum(axis=1, keepdims=True)).reshape(-1)


@pytest.mark.parametrize("name", ["mini_cls19", "mini_cls53"])
def test_classifier_goldens_are_the_reference(name):
    g = golden(name + ".npz")
    cfg = str(g["cfg"])
    secs = IO.parse_cfg(cfg)
    types = [s["type"] for s in secs[1:]]
    assert "avgpool" in types and "softmax" in types and float(g["max_abs_logit"]) > 3.0
    out = g["output"]
    assert out.shape == (24,) and out.max() > 4 * out.min() and out.max() > 0.1          # not a near-uniform distribution
    # the float64 restatement of the two layers agrees with what the reference computed in fp32
    pooled, p = _restate_tail(g)
    assert np.abs(p - out.astype(np.float64)).max() <= 1e-6
    if pooled is not None and types[types.index("softmax") - 1] == "avgpool":
        ap = types.index("avgpool")
        assert np.abs(pooled - g["layer_%02d" % ap].astype(np.float64).reshape(-1)).max() <= 1e-6 * max(1.0, float(np.abs(pooled).max()))
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built: the fixture cannot be re-derived here")
    net = DR.RefNet(cfg, g["weights"], int(g["header"][0]), int(g["header"][1]))
    try:
        assert net.n == len(secs) - 1
        net.predict(g["image_u8"].astype(np.float32) / np.float32(255.0))
        for i in range(net.n):
            assert np.array_equal(np.asarray(net.layer_output_nhwc(i), dtype=np.float32), g["layer_%02d" % i]), "layer %d" % i
        ret = net.l.network_predict(net.net, net._keep.ctypes.data_as(C.POINTER(C.c_float)))
        assert np.array_equal(np.ctypeslib.as_array(ret, shape=(24,)), out)          # the last layer that is not [cost]
    finally:
        net.close()


def test_classifier_surface_exists():
    from yolo_tensorflow_amd import hip, darknet_hip, classifier
    import yolo_tensorflow_amd
    lib = hip.load_library()
    for name in ("yolo_classify", "yolo_classify_images_u8", "yolo_num_classes", "yolo_op_avgpool", "yolo_op_softmax"):
        assert name in hip.EXPORTS and hasattr(lib, name), name
    assert callable(darknet_hip.classify) and callable(classifier.Classifier)
    assert "classifier" in yolo_tensorflow_amd.__all__
    for attr in ("classify", "classify_images", "num_classes"):
        assert hasattr(hip.Engine, attr), attr
    assert callable(hip.op_avgpool) and callable(hip.op_softmax)
