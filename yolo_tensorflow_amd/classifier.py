"""Classifier networks (darknet-19, darknet-53, ResNet-18 .. 152, VGG-16, any cfg that ends in [softmax]): "Darknet weights in, top classes out".

Counterpart of what the reference's ctypes binding does with such a network (`classify`, D2T/darknet.py:117-123: predict, pair every
probability with its name, sort by -prob), with the pooling, the softmax and the selection of the top classes on the device: uint8
images of any sizes are fitted to the network input in one launch, and only `top` records per image come back."""
import numpy as np
from . import hip, darknet_io as IO


class Classifier:
    def __init__(self, cfg_or_name, weights_file=None, dtype=hip.BF16, max_batch=1, names=None, device=0, fit=hip.FIT_STRETCH, seed=0, hierarchy=None, jpeg_entropy="host"):
        """cfg_or_name: a shipped topology ('darknet19', 'darknet53', 'resnet18', 'resnet50', 'resnext50', 'vgg-16'), a cfg file path, or cfg text
        (a ResNet's [shortcut] layers with fewer or larger `from` tensors and any of darknet's thirteen activations are served).  weights_file: a darknet
        `.weights` file; None loads darknet_io's seeded synthetic parameters (`seed`).  names: a list of class names or the path of a
        file with one name per line; without it the class index stands in for the name.  fit: how an image of any size becomes the network
        input, a hip.FIT_* code -- hip.FIT_CENTER_CROP is darknet's validation preprocessing (resize_min to the network width, then the centred
        crop), e.g. for 'alexnet-lrn'.  hierarchy (a [softmax] with tree=): None
        returns the conditional probabilities network_predict gives, "absolute" the products along the path to the root
        (hierarchy_predictions), "leaves" those with every inner node zeroed -- what darknet's classifier apps rank.  jpeg_entropy: "host" or "auto" --
        who Huffman-decodes the files of classify_from_files (Engine.set_jpeg_entropy); the results are the same."""
        text = cfg_or_name if "[net]" in cfg_or_name or "[network]" in cfg_or_name else IO.cfg_text(cfg_or_name)
        text = IO.with_planes_input(text)          # darknet's own grey / multi-plane cfgs ([net] channels != 3) load unchanged
        self.engine = hip.Engine(text, max_batch=max_batch, dtype=dtype, semantics=hip.SEM_DARKNET, device=device)
        if self.engine.rows != 0:
            self.engine.close()
            raise hip.YoloError("Classifier: the cfg describes a detector (it has a detection head)")
        if weights_file is not None:
            self.engine.load_weights(weights_file)
        else:
            self.engine.set_weights(IO.synth_weights(IO.parse_cfg(text), seed=seed))
        if jpeg_entropy != "host":
            self.engine.set_jpeg_entropy(jpeg_entropy)
        if hierarchy is not None:
            self.engine.set_hierarchy_mode(hierarchy)
        self.max_batch, self.fit = max_batch, fit
        self.num_classes = self.engine.num_classes
        if isinstance(names, str):
            with open(names) as fh:
                names = [line.rstrip("\r\n") for line in fh]
        self.names = list(names) if names is not None else None

    def _name(self, k):
        return self.names[k] if self.names is not None and 0 <= k < len(self.names) else int(k)

    VIEWS = {"flip": hip.VIEWS_FLIP, "ten_crop": hip.VIEWS_TEN_CROP}

    def classify_from_images(self, images, top=5, views=None, shift=32):
        """images: a list of uint8 [h, w, C] arrays of any sizes (RGB; a network of C planes: [h, w, C], one plane also [h, w]) -> per image [(name_or_index, prob), ...], `top` entries,
        probability descending.  views: None predicts each image once; "flip" averages the image (fitted by the classifier's fit) and its mirror, as
        darknet's test_cifar_multi adds them; "ten_crop" averages darknet's `classifier valid10` views, five crops of the image resized to the network
        input + `shift` and the same five of its mirror (the fit is not used).  Both return the MEAN over the views, formed and ranked on the device."""
        return self._classify(images, top, views, shift, self.engine.classify_images, self.engine.classify_views)

    def _classify(self, items, top, views, shift, once, multi):
        """classify_from_*: `once` the engine's single-view call over a chunk of max_batch items, `multi` its multi-view call over all of them"""
        if views is not None:
            if views not in self.VIEWS:
                raise hip.YoloError("Classifier: views must be None, 'flip' or 'ten_crop', got %r" % (views,))
            mode = self.VIEWS[views]
            cls, probs = multi(items, mode, fit=self.fit, shift=shift, scale=1.0 / len(hip.view_table(mode, shift)), top_k=top)
            return [[(self._name(int(k)), float(q)) for k, q in zip(c, p)] for c, p in zip(cls, probs)]
        out = []
        for lo in range(0, len(items), self.max_batch):
            cls, probs = once(items[lo:lo + self.max_batch], fit=self.fit, top_k=top)
            for c, p in zip(cls, probs):
                out.append([(self._name(int(k)), float(q)) for k, q in zip(c, p)])
        return out

    def classify_from_image(self, image, top=5):
        return self.classify_from_images([np.ascontiguousarray(image, dtype=np.uint8)], top=top)[0]

    def classify_from_files(self, paths, top=5, views=None, shift=32):
        """paths: a list of JPEG files (paths or bytes objects) -> what classify_from_images returns, over the pixels darknet's load_image reads from them:
        entropy decode on the host, IDCT, chroma upsampling, colour and the fit on the device.  With fit=hip.FIT_CENTER_CROP this is `darknet classifier
        predict cfg weights file.jpg`; views="ten_crop" is `classifier valid10` over files."""
        return self._classify(list(paths), top, views, shift, self.engine.classify_jpegs, self.engine.classify_views_jpegs)

    def classify_from_frames(self, frames, top=5, views=None, shift=32):
        """frames: a list of hip.Frame (NV12, I420, pitched RGB / BGR surfaces) -> what classify_from_images returns; every frame is converted while it is
        fitted, no RGB copy of it is made."""
        return self._classify(list(frames), top, views, shift, self.engine.classify_frames, self.engine.classify_views_frames)

    def close(self):
        self.engine.close()
