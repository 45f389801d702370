"""MI355X-native YOLO inference hot path.  `hip` is the ctypes shim over libyolo_hip.so (`hip.Frame` / `hip.pack_frames`:
decoded NV12 / I420 / pitched RGB / BGR video frames for the `*_frames` entry points);
`yolo_v3`, `yolo_v2`, `detector`, `classifier` mirror the reference's Python entry points; `darknet_io` handles cfg/.weights;
`dist` shards batches across GPUs; `char_rnn` generates and scores text with darknet's character networks."""
__all__ = ["hip", "darknet_io", "yolo_v3", "yolo_v2", "detector", "classifier", "dist", "char_rnn"]
