"""The entry points of the launch sequence (yolo_run.cpp) against each other, on one small network: the two captured detect steps
(yolo_detect_graph, yolo_detect_images_graph) sharing a context, a refused call between two replays, the state a replay of the images
graph leaves behind, and the single-image entry points against their row of a ragged batch in the split-fp16 configuration -- the only
one that takes the `in_pair` branch of every input staging site.

Network: YOLOv3 at 96 x 96 (three cells per side at stride 32), max_batch 3.  Every comparison is bit for bit: the entry points issue
the same launches on the same buffers, only the host code around them differs."""
import numpy as np
import pytest
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu

S = 96
N = 3
SIZES = [(1, 1), (50, 131), (96, 96)]          # (height, width) of the ragged batch
POST = dict(score_thr=0.3, iou_thr=0.45, max_out=30)
DTYPES = ["BF16", "FP16X2"]

_NET = {}
_WANT = {}


def _net():
    if not _NET:
        txt = IO.with_input_size(IO.cfg_text("yolov3"), S)
        _NET["v"] = (txt, IO.synth_weights(IO.parse_cfg(txt), seed=2, obj_bias=-0.75))
    return _NET["v"]


def _engine(hip, dtype):
    txt, flat = _net()
    e = hip.Engine(txt, max_batch=N, dtype=getattr(hip, dtype))
    e.set_weights(flat)
    return e


def _inputs():
    rng = np.random.default_rng(7)
    G = rng.integers(0, 256, (N, S, S, 3), dtype=np.uint8)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    A = rng.integers(0, 256, (N, S, S, 3), dtype=np.uint8)
    return G, imgs, A


def _want(hip, dtype):
    """the eager records of the fixed inputs, computed once per dtype on an engine of their own"""
    if dtype not in _WANT:
        G, imgs, A = _inputs()
        ref = _engine(hip, dtype)
        w = {"G": G, "imgs": imgs, "A": A}
        w["g"] = ref.detect(G, **POST)
        w["i"] = ref.detect_images(imgs, fit=hip.FIT_STRETCH, units=hip.UNITS_SOURCE_PIXELS, **POST)
        w["i_net"] = ref.detect_images(imgs, fit=hip.FIT_STRETCH, units=hip.UNITS_NETWORK, **POST)
        ref.close()
        print("kept (%s): batch %s, ragged batch %s" % (dtype, [len(r) for r in w["g"]], [len(r) for r in w["i"]]))
        assert sum(len(r) for r in w["g"]) > 0 and sum(len(r) for r in w["i"]) > 0 and sum(len(r) for r in w["i_net"]) > 0
        _WANT[dtype] = w
    return _WANT[dtype]


def _recs_equal(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class _Steps:
    """device buffers of the two graph entry points on one engine; g() / i() make one call and return its records"""

    def __init__(self, hip, eng, w, units):
        import torch
        self.hip, self.eng, self.units = hip, eng, units
        self.mo = POST["max_out"]
        self.dG = torch.from_numpy(w["G"]).cuda()
        pix, self.descs = hip.pack_images(w["imgs"])
        self.dpix = torch.from_numpy(pix).cuda()
        self.out = {k: (torch.zeros(N * self.mo * 6, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")) for k in "gi"}

    def _read(self, k):
        self.eng.synchronize()
        boxes, counts = self.out[k]
        bx = boxes.cpu().numpy().view(self.hip.BOX_DTYPE).reshape(N, self.mo); ct = counts.cpu().numpy()
        return [bx[b, :ct[b]].copy() for b in range(N)]

    def g(self, **kw):
        a = dict(POST); a.update(kw)
        self.eng.detect_graph(self.dG, self.out["g"][0], self.out["g"][1], **a)
        return self._read("g")

    def i(self, **kw):
        a = dict(POST); a.update(kw)
        self.eng.detect_images_graph(self.dpix, self.descs, self.out["i"][0], self.out["i"][1], fit=self.hip.FIT_STRETCH, units=self.units, **a)
        return self._read("i")


def _same(got, want, what):
    for b in range(N):
        assert _recs_equal(got[b], want[b]), "%s, image %d" % (what, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_graphs_on_one_context(hiplib, dtype):
    """G G G I I I G I G I on one engine: each entry point keeps its own captured step, and every call's boxes and counts are the
    eager detect's / detect_images' of the same inputs."""
    w = _want(hiplib, dtype)
    eng = _engine(hiplib, dtype)
    st = _Steps(hiplib, eng, w, hiplib.UNITS_SOURCE_PIXELS)
    for k, which in enumerate("GGGIIIGIGI"):
        if which == "G":
            _same(st.g(), w["g"], "call %d (detect_graph)" % (k + 1))
        else:
            _same(st.i(), w["i"], "call %d (detect_images_graph)" % (k + 1))
    eng.close()


@pytest.mark.parametrize("entry", ["g", "i"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_call_between_replays(hiplib, dtype, entry):
    """three good calls (eager, capture, replay), two refused ones, two good ones"""
    w = _want(hiplib, dtype)
    eng = _engine(hiplib, dtype)
    st = _Steps(hiplib, eng, w, hiplib.UNITS_SOURCE_PIXELS)
    call, want = (st.g, w["g"]) if entry == "g" else (st.i, w["i"])
    for k in range(3):
        _same(call(), want, "call %d" % (k + 1))
    with pytest.raises(hiplib.YoloError):
        call(max_out=0)
    with pytest.raises(hiplib.YoloError):
        call(nms_mode=9)
    for k in range(2):
        _same(call(), want, "call %d after the refused ones" % (k + 1))
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_images_graph_replay_leaves_the_eager_state(hiplib, dtype):
    """forward(A) leaves A's decoded tensor resident; a replay of the images graph on the ragged batch B must leave what the eager call
    it was captured from leaves: B's lean rows (no decoded tensor), B's threshold, the fitted input of B as what the stem reads.
    The timing entry points then run a full forward over the resident input: every layer's time, the forward's and the convs' share
    are finite and positive, and the decoded tensor they leave is B's."""
    w = _want(hiplib, dtype)
    eng = _engine(hiplib, dtype)
    st = _Steps(hiplib, eng, w, hiplib.UNITS_NETWORK)
    for k in range(3):
        _same(st.i(), w["i_net"], "call %d" % (k + 1))
    eng.forward(w["A"])
    _same(st.i(), w["i_net"], "replay after forward(A)")
    _same(eng.postprocess(N, **POST), w["i_net"], "postprocess after the replay")
    with pytest.raises(hiplib.YoloError, match="without materialising"):
        eng.postprocess(N, nms_mode=hiplib.NMS_NUMPY_V3, **POST)
    with pytest.raises(hiplib.YoloError, match="lower threshold"):
        eng.postprocess(N, score_thr=0.1, iou_thr=POST["iou_thr"], max_out=POST["max_out"])
    with pytest.raises(hiplib.YoloError, match="needs a yolo_forward"):
        eng.darknet_boxes(0, S, S, thresh=0.3)
    ms = eng.time_layers(N, 1)
    total, conv = eng.time_forward(N, 1)
    print("time_layers (%s): min %.6f ms, %d of %d layers at zero, sum %.4f ms; time_forward %.4f ms, convs %.4f ms" % (
        dtype, float(ms.min()), int((ms == 0).sum()), len(ms), float(ms.sum()), total, conv))
    assert np.isfinite(ms).all() and (ms > 0).all()
    assert np.isfinite(total) and np.isfinite(conv) and total > 0 and conv > 0
    _same(eng.postprocess(N, **POST), w["i_net"], "postprocess after time_forward")
    eng.close()


def _chw_darknet(im):
    """the image as darknet's loader stores it: planar, (float)p/255."""
    return np.ascontiguousarray((im.astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1))


def test_letterbox_single_image_equals_its_row_of_the_batch(hiplib):
    """split fp16 (test_gpu_native_batch.py holds the bf16 cases): row i of a ragged batch's decoded tensor is the decoded tensor of
    image i alone, through yolo_forward_letterbox_chw on FIT_LETTERBOX and through yolo_forward_image_u8 on FIT_STRETCH."""
    imgs = _want(hiplib, "FP16X2")["imgs"]
    eng = _engine(hiplib, "FP16X2")
    det = eng.forward_images(imgs, fit=hiplib.FIT_LETTERBOX)
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        chw = _chw_darknet(im)
        one = np.empty((1, eng.rows, eng.attrs), dtype=np.float32)
        rc = eng.lib.yolo_forward_letterbox_chw(eng.ctx, chw.ctypes.data, w, h, hiplib.HOST, one.ctypes.data, hiplib.HOST)
        assert rc == 0
        assert np.array_equal(one[0].view(np.uint32), det[i].view(np.uint32)), "letterbox, image %d" % i
    det = eng.forward_images(imgs, fit=hiplib.FIT_STRETCH)
    for i, im in enumerate(imgs):
        assert np.array_equal(eng.forward_image(im)[0].view(np.uint32), det[i].view(np.uint32)), "stretch, image %d" % i
    eng.close()
