"""Dense-prediction networks (segmentation masks, heat maps, any U-Net-shaped cfg with `yolo_output=map` in [net]): "Darknet weights in,
maps and label images out".

Counterpart of the reference's examples/segmenter.c `predict_segmenter`, which letterboxes an image, calls network_predict and reads the
prediction back with get_network_image.  Here uint8 images of any sizes are fitted to the network input in one launch, the map stays
on the device in fp32, and `segment_from_images` returns every image's labels AT ITS OWN SIZE (the reference only ever shows the
letterboxed prediction; the native-pixel -> map-pixel rule is this project's own, include/yolo_hip.h yolo_segment_images_u8)."""
import numpy as np
from . import hip, darknet_io as IO

_FITS = {"letterbox": hip.FIT_LETTERBOX, "stretch": hip.FIT_STRETCH}


class Segmenter:
    def __init__(self, cfg, weights=None, max_batch=1, dtype=hip.BF16, fit="letterbox", device=0, seed=0, jpeg_entropy="host"):
        """cfg: a cfg file path or cfg text with `yolo_output=map` in its [net] section.  weights: a darknet `.weights` file or a flat
        float32 parameter stream; None loads darknet_io's seeded synthetic parameters (`seed`).  fit: "letterbox" (darknet's
        letterbox_image) or "stretch", or a hip.FIT_* code.  jpeg_entropy: "host" or "auto" -- who Huffman-decodes the files of the *_from_files methods
        (Engine.set_jpeg_entropy); the results are the same."""
        text = IO.with_planes_input(cfg if "[net]" in cfg or "[network]" in cfg else IO.cfg_text(cfg))          # ([net] channels != 3: the key is added here)
        self.engine = hip.Engine(text, max_batch=max_batch, dtype=dtype, semantics=hip.SEM_DARKNET, device=device)
        try:
            self.map_hwc = self.engine.map_geometry()
        except hip.YoloError:
            self.engine.close()
            raise
        if weights is None:
            self.engine.set_weights(IO.synth_weights(IO.parse_cfg(text), seed=seed))
        elif isinstance(weights, str):
            self.engine.load_weights(weights)
        else:
            self.engine.set_weights(weights)
        if jpeg_entropy != "host":
            self.engine.set_jpeg_entropy(jpeg_entropy)
        self.max_batch = max_batch
        self.fit = _FITS[fit] if isinstance(fit, str) else int(fit)
        self.num_classes = self.map_hwc[2]

    def predict_from_images(self, images):
        """images: a list of uint8 [h, w, C] arrays of any sizes (RGB; a network of C planes: [h, w, C], one plane also [h, w]) -> a list of [map_h, map_w, c] float32 maps (of the fitted input)."""
        out = []
        for lo in range(0, len(images), self.max_batch):
            chunk = images[lo:lo + self.max_batch]
            self.engine.forward_images(chunk, fit=self.fit, want_detections=False)
            out.extend(m.copy() for m in self.engine.output_map(len(chunk)))
        return out

    def segment_from_images(self, images, thresh=0.5):
        """-> a list of [h_i, w_i] uint8 label arrays, each at its image's own size: the arg-max channel of the map pixel the native pixel
        falls on, 255 where that maximum is below `thresh`."""
        out = []
        for lo in range(0, len(images), self.max_batch):
            out.extend(self.engine.segment_images(images[lo:lo + self.max_batch], fit=self.fit, thresh=thresh))
        return out

    def segment_from_files(self, paths, thresh=0.5):
        """paths: a list of JPEG files (paths or bytes objects) -> segment_from_images over the pixels darknet's load_image reads from them (the
        reference's `segmenter test` takes a file), decoded and fitted on the device; labels at each picture's own size."""
        paths, out = list(paths), []
        for lo in range(0, len(paths), self.max_batch):
            out.extend(self.engine.segment_jpegs(paths[lo:lo + self.max_batch], fit=self.fit, thresh=thresh))
        return out

    def segment_from_frames(self, frames, thresh=0.5):
        """frames: a list of hip.Frame -> segment_from_images over them, each converted while it is fitted; labels at each frame's own size."""
        frames, out = list(frames), []
        for lo in range(0, len(frames), self.max_batch):
            out.extend(self.engine.segment_frames(frames[lo:lo + self.max_batch], fit=self.fit, thresh=thresh))
        return out

    def close(self):
        self.engine.close()
