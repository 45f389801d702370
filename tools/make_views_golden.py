#!/usr/bin/env python
"""tests/golden/views_cases.npz: darknet's multi-view classification (DN/examples/classifier.c:234-301 validate_classifier_10, DN/examples/cifar.c:101-128
test_cifar_multi) through the compiled reference (oracle/_ref/libdarknet_ref.so), composed through ctypes in validate_classifier_10's own order:

    resize_image(im, W', H') (load_image's rule: only where the size differs) -> five crop_image -> flip_image -> the same five crop_image
    -> per view network_predict (+ hierarchy_predictions(.., only_leaves = 1) where the network has a tree) -> axpy_cpu into a zeroed row -> top_k

Per case <name>: <name>_image_u8 [h, w, c], <name>_views [K, net_h, net_w, c] float32 (what network_predict was fed, as NHWC), <name>_rows [K, classes],
<name>_sum [classes], <name>_topk [TOP] int32, <name>_max_logit [K] (max |.| of the last conv's output, what tests/test_gpu_classifier.py::_prob_bound
scales its tolerance by); per network <net>_cfg, <net>_weights (and tree_text).  `cases` lists (name, net, mode, shift), <name>_seed the image seed the search settled on.  Data only.

The module is also what the tests import: the cfgs, the case list, the numpy restatement of the view pixel rule (ten_crop_numpy) and the ctypes composition
(RefViews), so that the fixture, the host test and a fresh composition state one thing.

    python tools/make_views_golden.py          (needs oracle/_ref built: __graft_entry__.build())
"""
import ctypes as C
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "views_cases.npz")
NET_W, NET_H, CLASSES, TOP = 24, 20, 24, 5
FLIP, TEN_CROP = 1, 2          # include/yolo_hip.h enum yolo_views
U = 2.0 ** -24


def _conv(filters, size, stride=1, bn=True, act="leaky"):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", filters, size, stride, act)


def _net(channels):
    return "[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=%d\n\n" % (NET_W, NET_H, channels)


def cls19_cfg(tail="groups=1\n"):
    """tools/make_golden.py's MINI_CLS19 (darknet-19's tail order) at a non-square input of 24 wide x 20 high"""
    return (_net(3) + _conv(8, 3) + "[maxpool]\nsize=2\nstride=2\n\n" + _conv(16, 3) + _conv(8, 1) + _conv(16, 3) + "[shortcut]\nfrom=-3\nactivation=linear\n\n" +
            "[maxpool]\nsize=2\nstride=2\n\n" + _conv(32, 3) + _conv(CLASSES, 1, bn=False, act="linear") + "[avgpool]\n\n[softmax]\n" + tail)


def planes_cfg(channels):
    """a classifier of `channels` planes as darknet reads it (no yolo_input key: darknet_io.with_planes_input adds it for the library)"""
    return (_net(channels) + _conv(8, 3) + "[maxpool]\nsize=2\nstride=2\n\n" + _conv(16, 3) + _conv(CLASSES, 1, bn=False, act="linear") + "[avgpool]\n\n[softmax]\ngroups=1\n")


TREE_FILE = "views.tree"          # the tree cfg names its tree by this relative path: darknet opens it relative to the working directory


def tree_text():
    """a 24-node tree as tools/make_cfgs.py writes them (synthetic_tree): the tree classifier's [softmax] has one output per node"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_cfgs", os.path.join(ROOT, "tools", "make_cfgs.py"))
    M = importlib.util.module_from_spec(spec); spec.loader.exec_module(M)
    return M.synthetic_tree(nodes=CLASSES, roots=4, seed=5, max_group=20)


# (net name, cfg, channels, weight seed, has a tree)
NETS = [("rgb", cls19_cfg(), 3, 301, False), ("grey", planes_cfg(1), 1, 303, False), ("rgbd", planes_cfg(4), 4, 305, False),
        ("tree", cls19_cfg("tree=%s\n" % TREE_FILE), 3, 307, True)]
# (case, net, mode, shift, source h, source w).  W' x H' = (24 + shift) x (20 + shift).  shift 32 is larger than the network: the -s views are all edge;
# shift 0: the five crops coincide.  Sources: smaller than W' x H', larger in both axes, exactly W' x H' (no resize), one axis equal, odd extents, 1 x 1
CASES = [
    ("s32_smaller", "rgb", TEN_CROP, 32, 17, 30), ("s32_1x1", "rgb", TEN_CROP, 32, 1, 1),
    ("s5_larger", "rgb", TEN_CROP, 5, 37, 41), ("s5_exact", "rgb", TEN_CROP, 5, 25, 29), ("s5_axis", "rgb", TEN_CROP, 5, 40, 29), ("s5_odd", "rgb", TEN_CROP, 5, 23, 37),
    ("s0_other", "rgb", TEN_CROP, 0, 18, 31), ("s0_exact", "rgb", TEN_CROP, 0, 20, 24),
    ("grey_s5", "grey", TEN_CROP, 5, 23, 37), ("rgbd_s32", "rgbd", TEN_CROP, 32, 23, 37), ("tree_s5", "tree", TEN_CROP, 5, 37, 41),
    ("flip_rgb", "rgb", FLIP, 0, 23, 37), ("flip_grey", "grey", FLIP, 0, 31, 18),
]
TEN_OFFSETS = [(-1, -1), (1, -1), (0, 0), (-1, 1), (1, 1)]          # (dx, dy) in units of shift, classifier.c:273-277


def unit(img_u8):
    """darknet's loader: (float)p / 255., a double division rounded to float"""
    return (np.asarray(img_u8).astype(np.float64) / 255.).astype(np.float32)


def resize_image_f32(im, w, h):
    """DN/image.c:1347-1389 resize_image on an [ih, iw, c] float32 image, operation for operation in float32 (tests/test_lrn_crop_host.py's restatement)"""
    f = np.float32
    im = np.asarray(im, dtype=f); ih, iw = im.shape[:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        w_scale = f(iw - 1) / f(w - 1); h_scale = f(ih - 1) / f(h - 1)
    part = np.zeros((ih, w, im.shape[2]), f)
    for c in range(w):
        if c == w - 1 or iw == 1:
            part[:, c] = im[:, iw - 1]
        else:
            sx = f(c) * w_scale; ix = int(sx); dx = f(sx - f(ix))
            part[:, c] = (f(1) - dx) * im[:, ix] + dx * im[:, ix + 1]
    out = np.zeros((h, w, im.shape[2]), f)
    for r in range(h):
        if ih == 1:
            out[r] = part[0]
            continue
        sy = f(r) * h_scale; iy = int(sy); dy = f(sy - f(iy))
        out[r] = (f(1) - dy) * part[iy]
        if r != h - 1:
            out[r] = out[r] + dy * part[iy + 1]
    return out


def ten_crop_numpy(img_u8, shift, net_h=NET_H, net_w=NET_W):
    """The view pixel rule of YOLO_VIEWS_TEN_CROP in float32 numpy: view v, pixel (x, y) = R[clamp(y + dy)][cx] (v < 5) or R[..][W' - 1 - cx] (v >= 5),
    cx = clamp(x + dx), R the unit image resized to W' x H' (the image itself where it has that size) -> [10, net_h, net_w, c]"""
    im = unit(img_u8)
    rw, rh = net_w + shift, net_h + shift
    R = im if im.shape[:2] == (rh, rw) else resize_image_f32(im, rw, rh)
    out = []
    for v in range(10):
        dx, dy = TEN_OFFSETS[v % 5][0] * shift, TEN_OFFSETS[v % 5][1] * shift
        rows = np.clip(np.arange(net_h) + dy, 0, rh - 1); cols = np.clip(np.arange(net_w) + dx, 0, rw - 1)
        if v >= 5:
            cols = rw - 1 - cols
        out.append(R[rows][:, cols])
    return np.stack(out)


class IMAGE(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]


class RefViews:
    """the compiled reference's functions validate_classifier_10 calls, bound through ctypes"""

    def __init__(self):
        from oracle import darknet_ref as D
        self.D = D
        l = self.l = D.lib()
        FP = C.POINTER(C.c_float)
        l.resize_image.argtypes = [IMAGE, C.c_int, C.c_int]; l.resize_image.restype = IMAGE
        l.crop_image.argtypes = [IMAGE, C.c_int, C.c_int, C.c_int, C.c_int]; l.crop_image.restype = IMAGE
        l.flip_image.argtypes = [IMAGE]; l.flip_image.restype = None
        l.free_image.argtypes = [IMAGE]; l.free_image.restype = None
        l.read_tree.argtypes = [C.c_char_p]; l.read_tree.restype = C.c_void_p
        l.hierarchy_predictions.argtypes = [FP, C.c_int, C.c_void_p, C.c_int, C.c_int]; l.hierarchy_predictions.restype = None
        l.axpy_cpu.argtypes = [C.c_int, C.c_float, FP, C.c_int, FP, C.c_int]; l.axpy_cpu.restype = None
        l.top_k.argtypes = [FP, C.c_int, C.c_int, C.POINTER(C.c_int)]; l.top_k.restype = None

    def ten_views(self, img_u8, shift, net_h=NET_H, net_w=NET_W):
        """classifier.c:268-283 on the unit image -> [10, net_h, net_w, c] float32"""
        l = self.l
        h, w, ch = img_u8.shape
        chw = np.array(unit(img_u8).transpose(2, 0, 1), order="C", copy=True)
        im = IMAGE(w, h, ch, chw.ctypes.data_as(C.POINTER(C.c_float)))
        W, H = net_w + shift, net_h + shift
        resized = (H != h or W != w)          # load_image: `if((h && w) && (h != out.h || w != out.w))`
        if resized:
            im = l.resize_image(im, W, H)
        views = []

        def crops():
            for dx, dy in TEN_OFFSETS:
                cr = l.crop_image(im, dx * shift, dy * shift, net_w, net_h)
                views.append(np.ctypeslib.as_array(cr.data, shape=(ch, net_h, net_w)).copy().transpose(1, 2, 0))
                l.free_image(cr)
        crops()
        l.flip_image(im)          # (in place: on `chw` where nothing was resized)
        crops()
        if resized:
            l.free_image(im)
        return np.ascontiguousarray(np.stack(views))

    def flip_views(self, view0):
        """test_cifar_multi: the network-sized image, then flip_image on it -> [2, net_h, net_w, c]"""
        chw = np.array(np.asarray(view0, np.float32).transpose(2, 0, 1), order="C", copy=True)          # (a copy also for one plane, whose transpose is contiguous already: flip_image works in place)
        ch, h, w = chw.shape
        self.l.flip_image(IMAGE(w, h, ch, chw.ctypes.data_as(C.POINTER(C.c_float))))
        return np.ascontiguousarray(np.stack([np.asarray(view0, np.float32), chw.transpose(1, 2, 0)]))

    def reduce(self, net, views, logit_layer, tree=None):
        """per view network_predict (+ hierarchy_predictions with only_leaves), axpy_cpu into a zeroed row, top_k -> rows [K, classes], sum, topk, max |logit| [K]"""
        l = self.l
        FP = C.POINTER(C.c_float)
        classes = l.ref_layer_outputs(net.net, net.n - 1)
        pred = np.zeros(classes, np.float32)
        rows, logits = [], []
        for v in views:
            chw = np.array(v.transpose(2, 0, 1), order="C", copy=True)
            p = l.network_predict(net.net, chw.ctypes.data_as(FP))
            if tree is not None:
                l.hierarchy_predictions(p, classes, tree, 1, 1)
            rows.append(np.ctypeslib.as_array(p, shape=(classes,)).copy())
            logits.append(np.float32(np.abs(net.layer_output_nhwc(logit_layer)).max()))
            l.axpy_cpu(classes, 1.0, p, 1, pred.ctypes.data_as(FP), 1)
        idx = (C.c_int * TOP)()
        l.top_k(pred.ctypes.data_as(FP), classes, TOP, idx)
        return np.stack(rows), pred, np.array(list(idx), np.int32), np.array(logits, np.float32)


def stretch_numpy(img_u8, net_h=NET_H, net_w=NET_W):
    """YOLO_FIT_STRETCH in float32 numpy (value / 255.0f, then TF's legacy bilinear: src = dst * in / out, no half-pixel offset): view 0 of the FLIP cases"""
    f = np.float32
    im = np.asarray(img_u8).astype(f) / f(255.0)
    h, w = im.shape[:2]
    hs, ws = f(h) / f(net_h), f(w) / f(net_w)
    out = np.zeros((net_h, net_w, im.shape[2]), f)
    for oy in range(net_h):
        fy = f(oy) * hs; y0 = int(np.floor(fy)); y1 = min(y0 + 1, h - 1); yl = f(fy - f(y0))
        for ox in range(net_w):
            fx = f(ox) * ws; x0 = int(np.floor(fx)); x1 = min(x0 + 1, w - 1); xl = f(fx - f(x0))
            top = im[y0, x0] + (im[y0, x1] - im[y0, x0]) * xl
            bot = im[y1, x0] + (im[y1, x1] - im[y1, x0]) * xl
            out[oy, ox] = top + (bot - top) * yl
    return out


def prob_bound(p_ref, tol, max_logit):
    """tests/test_gpu_classifier.py::_prob_bound"""
    return p_ref.astype(np.float64) * np.expm1(2 * tol * float(max_logit)) + 1e-7


def sum_bound(rows, total, max_logit, tol):
    """a sum of K rows, each within its own bound, plus K roundings of the additions"""
    K = rows.shape[0]
    return sum(prob_bound(rows[v], tol, max_logit[v]) for v in range(K)) + K * U * np.abs(total.astype(np.float64))


def generate():
    from yolo_tensorflow_amd import darknet_io as IO
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden import save_npz_reproducibly
    import tempfile
    R = RefViews()
    data = {"cases": np.array([[c[0], c[1], str(c[2]), str(c[3])] for c in CASES]), "net_hw": np.array([NET_H, NET_W], np.int32), "top": np.int32(TOP),
            "tree_text": np.array(tree_text())}
    work = tempfile.mkdtemp(prefix="views_")
    with open(os.path.join(work, TREE_FILE), "w") as f:
        f.write(tree_text())
    here = os.getcwd()
    os.chdir(work)          # darknet opens the tree relative to the working directory
    try:
        nets = {}
        for name, cfg, ch, seed, has_tree in NETS:
            secs = IO.parse_cfg(cfg)
            flat = IO.synth_weights(secs, seed=seed)
            last = IO.conv_specs(secs)[-1]
            tail = last["filters"] * (1 + last["cin"] * last["size"] ** 2)
            logit_layer = max(i for i, s in enumerate(secs[1:]) if s["type"] == "convolutional")
            probe = np.random.default_rng(seed + 1).integers(0, 256, (NET_H, NET_W, ch), dtype=np.uint8)
            net = R.D.RefNet(cfg, flat, 0, 2)
            net.predict(unit(probe))
            flat[-tail:] *= np.float32(round(5.0 / float(np.abs(net.layer_output_nhwc(logit_layer)).max()), 2))      # logits reach +-5, as gen_mini_cls does
            net.close()
            net = R.D.RefNet(cfg, flat, 0, 2)
            assert (net.h, net.w) == (NET_H, NET_W)
            nets[name] = (net, logit_layer, R.l.read_tree(TREE_FILE.encode()) if has_tree else None, ch)
            data[name + "_cfg"], data[name + "_weights"] = np.array(cfg), flat
        for k, (case, netname, mode, shift, h, w) in enumerate(CASES):
            net, logit_layer, tree, ch = nets[netname]
            # the image is chosen so that the fp32 top-k is decided: the reference's k-th and (k+1)-th sums further apart than twice the fp32 bound of a sum
            for seed in range(400 + k, 400 + k + 100 * 64, 100):
                img = np.random.default_rng(seed).integers(0, 256, (h, w, ch), dtype=np.uint8)
                views = R.ten_views(img, shift) if mode == TEN_CROP else R.flip_views(stretch_numpy(img))
                rows, total, topk, max_logit = R.reduce(net, views, logit_layer, tree)
                order = np.argsort(-total, kind="stable")
                bound = sum_bound(rows, total, max_logit, 2e-4)
                if all(float(total[order[j]]) - float(total[order[j + 1]]) > 2 * max(bound[order[j]], bound[order[j + 1]]) for j in range(TOP)):
                    break
            if mode == TEN_CROP:
                assert np.array_equal(views.view(np.uint32), ten_crop_numpy(img, shift).view(np.uint32)), case
            assert np.array_equal(order[:TOP].astype(np.int32), topk), (case, order[:TOP], topk)
            for j in range(TOP):
                a, b = order[j], order[j + 1]
                gap = float(total[a]) - float(total[b])
                assert gap > 2 * max(bound[a], bound[b]), "%s: ranks %d / %d are %g apart, the bound is %g" % (case, j, j + 1, gap, max(bound[a], bound[b]))
            data[case + "_seed"] = np.int32(seed)
            data[case + "_image_u8"], data[case + "_views"], data[case + "_rows"] = img, views, rows
            data[case + "_sum"], data[case + "_topk"], data[case + "_max_logit"] = total, topk, max_logit
            print(case, "views", views.shape, "sum top", total[topk[0]], "max|logit|", float(max_logit.max()))
        for net, _, _, _ in nets.values():
            net.close()
    finally:
        os.chdir(here)
    save_npz_reproducibly(OUT, data)
    print("views_cases", len(data), "arrays", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    generate()
