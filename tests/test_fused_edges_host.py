"""The fixtures of tests/test_gpu_fused_edges.py, host side (no device): darknet-53's first stage as a map network at input sizes that are
no multiples of 32, and the plan rows (yolo_plan_table) every one of them must have -- which layers the fused stem, conv3 + shortcut +
stride-2, the residual block and the split-fp16 stem take, which keep the halo / stride-2 kernels, and the negative cases (no residual
block where 13 x 13 blocks waste more than 15 %, no pair stem at an odd size).  The expectations are computed from the sizes by the
planner's published rules (csrc/yolo_plan.cpp), not recorded from it: a fixture that silently stops fusing cannot pass the GPU
file as a test of the tiled kernel."""
import numpy as np
import pytest
from yolo_tensorflow_amd import hip, darknet_io as IO

KNOBS = ("YOLO_NO_RESBLOCK", "YOLO_NO_C3S2", "YOLO_NO_HALO", "YOLO_NO_S2", "YOLO_NO_PAIR_STEM")
# height x width (the table of the GPU file's docstring says what each reaches)
SIZES = ((27, 37), (50, 50), (99, 47), (5, 3), (2, 2))
PAIR_SIZES = ((26, 38), (6, 4), (27, 37))          # split fp16: the pair stem applies at the first two, not at the odd one
VARIANT_SIZES = ((27, 37), (50, 50))               # the activation and channel-window variants
FUSED_LAYERS = (0, 1, 2, 3, 5, 6, 7)
# a different slope-family activation on every member of each fused launch: stem act0 / act1 / act2 = relu / relie / linear, conv3 + stride-2
# act3 / act5 = leaky / relie, the block's act1 / act2 = relu / leaky
MIXED_ACTS = {0: "relu", 1: "relie", 2: "linear", 3: "leaky", 5: "relie", 6: "relu", 7: "leaky"}
MIXED_BIAS_ONLY = 3                                 # the one layer of that variant with batch_normalize=0
DTYPES = {"bf16": hip.BF16, "fp16": hip.FP16, "fp16x2": hip.FP16X2}


def _conv(filters, size, stride=1, act="leaky", bn=False):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % ("batch_normalize=1\n" if bn else "", filters, size, stride, act)


def stage_cfg(hw, acts=None, bn=(), cat=False, affine=False):
    """0 conv 3x3 3 -> 32 | 1 conv 3x3 / 2 -> 64 | 2 conv 1x1 -> 32 | 3 conv 3x3 -> 64 | 4 shortcut from=-3 | 5 conv 3x3 / 2 -> 128 | 6 conv 1x1 -> 64 |
    7 conv 3x3 -> 128 | 8 shortcut from=-3 | 9 conv 1x1 linear -> the 6-channel fp32 map.  Bias-only convs unless the layer is in `bn`.
    cat=True, the channel windows:  9 route 1,2 -> 96 channels (layer 2 at channel offset 64, pixel stride 96; layer 1, the shortcut source of
    layer 4, at offset 0) | 10 conv 3x3 / 2 -> 8, the concatenation's second reader | 11 conv 3x3 -> 16 | 12 route 8,5,11 -> 272 channels
    (the block's output at offset 0, layer 5 -- the block's input and shortcut source -- at 128, pixel stride 272) | 13 the map conv.
    affine=True: [net] yolo_input_mul=2, yolo_input_add=-1."""
    a = dict.fromkeys(FUSED_LAYERS, "leaky"); a.update(acts or {})
    c = lambda i, f, k, st=1: _conv(f, k, st, a[i], i in bn)
    sc = "[shortcut]\nfrom=-3\nactivation=linear\n\n"
    net = "[net]\nbatch=1\nwidth=%d\nheight=%d\nchannels=3\nyolo_output=map\n%s\n" % (hw[1], hw[0], "yolo_input_mul=2\nyolo_input_add=-1\n" if affine else "")
    body = c(0, 32, 3) + c(1, 64, 3, 2) + c(2, 32, 1) + c(3, 64, 3) + sc + c(5, 128, 3, 2) + c(6, 64, 1) + c(7, 128, 3) + sc
    if cat:
        body += "[route]\nlayers=1,2\n\n" + _conv(8, 3, 2) + _conv(16, 3) + "[route]\nlayers=8,5,11\n\n"
    return net + body + _conv(6, 1, act="linear")


def mixed_cfg(hw):
    return stage_cfg(hw, acts=MIXED_ACTS, bn=tuple(i for i in FUSED_LAYERS if i != MIXED_BIAS_ONLY))


def half(n):
    """output extent of a 3x3 / stride 2 / pad 1 conv"""
    return (n - 1) // 2 + 1


def block_planned(hw):
    """the residual block's 115 % rule on the 128-channel grid: whole 13 x 13 blocks may waste at most 15 % of their pixels"""
    h, w = half(half(hw[0])), half(half(hw[1]))
    return -(-h // 13) * -(-w // 13) * 169 * 100 <= h * w * 115


def plan_rows(cfg, dtype, max_batch=3, keep=False, knobs=(), monkeypatch=None):
    """the plan table's layer rows as dicts (kernel, fused, launcher, residual_from, tail_layer, storage, ...), planned under `knobs`"""
    assert set(knobs) <= set(KNOBS) and (monkeypatch is not None or not knobs)
    if monkeypatch is not None:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k in knobs:
            monkeypatch.setenv(k, "1")
    try:
        rc, text = hip.plan_table(cfg, dtype=dtype, max_batch=max_batch, keep_layers=keep)
    finally:
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
    assert rc == 0, text
    return [dict(kv.split("=") for kv in line.split()[2:]) for line in text.splitlines() if line[:1].isdigit()]


def fused_of(rows):
    """{layer: (kernel, fused, launcher)} of the conv layers that are not `tiled, own launch`"""
    return {i: (r["kernel"], r["fused"], int(r["launcher"])) for i, r in enumerate(rows) if r["kernel"] != "-" and (r["kernel"], r["fused"]) != ("tiled", "none")}


def expected_fused(hw, fam, knobs=(), keep=False):
    """What fused_of() must say of stage_cfg(hw) -- any variant: the windows and the activations take no fusion away -- by the planner's rules.
    The halo and stride-2 kernels are properties of a layer (kept by the plan that keeps every layer); the fused launches need the plan that
    keeps none.  16-bit storage: stem = layers 0-2 at any size; conv3 + shortcut + stride-2 = layers 3, 5 at any size (what the launch cannot
    serve falls back when it is issued); the block = layers 6, 7 under the 115 % rule.  Split fp16: the pair stem = layers 0, 1 at even sizes."""
    want = {}
    if fam == "fp16x2":
        if not keep and "YOLO_NO_PAIR_STEM" not in knobs and hw[0] % 2 == 0 and hw[1] % 2 == 0:
            want[0] = want[1] = ("tiled", "pair-stem", 1)
        return want
    halo = "YOLO_NO_HALO" not in knobs
    s2 = halo and "YOLO_NO_S2" not in knobs
    c3s2 = halo and s2 and not keep and "YOLO_NO_C3S2" not in knobs
    if not keep:
        want[0] = want[1] = want[2] = ("tiled", "stem", 1)
    if halo:
        want[3] = ("halo", "c3s2" if c3s2 else "none", 5 if c3s2 else -1)
    if s2:
        want[5] = ("s2", "c3s2" if c3s2 else "none", 5 if c3s2 else -1)
    if not keep and "YOLO_NO_RESBLOCK" not in knobs and block_planned(hw):
        want[6] = want[7] = ("tiled", "resblock", 7)
    return want


def test_the_sizes_reach_what_the_table_says():
    shapes = lambda hw: [s[1:4] for s in IO.layer_shapes(IO.parse_cfg(stage_cfg(hw)))]
    assert shapes((27, 37)) == [(27, 37, 32), (14, 19, 64), (14, 19, 32), (14, 19, 64), (14, 19, 64), (7, 10, 128), (7, 10, 64), (7, 10, 128), (7, 10, 128), (7, 10, 6)]
    assert [shapes(hw)[1][:2] + shapes(hw)[5][:2] for hw in SIZES] == [(14, 19, 7, 10), (25, 25, 13, 13), (50, 24, 25, 12), (3, 2, 2, 1), (1, 1, 1, 1)]
    assert [block_planned(hw) for hw in SIZES] == [False, True, True, False, False]
    assert 2 * 169 * 100 <= 25 * 12 * 115 and not 169 * 100 <= 7 * 10 * 115          # 99 x 47: two ragged blocks pass; 27 x 37: one block does not
    assert 27 * 37 * 3 % 4 == 1 and 3 * 27 * 37 * 3 % 4 == 3 and (37 * 3) % 4 == 3   # raw rows of 111 bytes: all four alignments; an odd byte count for odd n
    cat = [s[1:4] for s in IO.layer_shapes(IO.parse_cfg(stage_cfg((27, 37), cat=True)))]
    assert cat[9:] == [(14, 19, 96), (7, 10, 8), (7, 10, 16), (7, 10, 272), (7, 10, 6)]


def test_large_batch_count():
    """27 x 37: the stem's 14 x 19 output is 2 x 2 tiles of 8 x 16, the 7 x 10 output of conv3 + stride-2 2 x 2 tiles of 4 x 8; both launch
    min(256, tiles) persistent workgroups and prefetch three tiles ahead, so every workgroup walks at least 4 tiles from 256 images on"""
    from math import ceil
    per_stem = ceil(14 / 8) * ceil(19 / 16); per_c3s2 = ceil(7 / 4) * ceil(10 / 8)
    assert per_stem == per_c3s2 == 4
    for n in LARGE_BATCHES:
        assert min(n * per_stem // 256, n * per_c3s2 // 256) >= 4
    assert LARGE_BATCHES[0] % 2 == 1 and (LARGE_BATCHES[0] * 27 * 37 * 3) % 4          # odd: the conversion launch feeds the stem
    assert (LARGE_BATCHES[1] * 27 * 37 * 3) % 4 == 0                                     # whole dwords: the stem reads the uint8 image itself


LARGE_BATCHES = (257, 260)


@pytest.mark.parametrize("fam", ["bf16", "fp16"])
@pytest.mark.parametrize("hw", SIZES)
def test_plan_rows_of_the_stage(monkeypatch, hw, fam):
    cfg = stage_cfg(hw)
    for keep in (False, True):
        rows = plan_rows(cfg, DTYPES[fam], keep=keep)
        assert fused_of(rows) == expected_fused(hw, fam, keep=keep), (hw, fam, keep)
        assert all(r["tail_layer"] == "-1" for r in rows)
        assert [rows[i]["residual_from"] for i in (3, 7)] == (["-2", "-2"] if keep else ["1", "5"])          # both shortcuts are folded in the plan that keeps no layer
    for knob in KNOBS:
        assert fused_of(plan_rows(cfg, DTYPES[fam], knobs=(knob,), monkeypatch=monkeypatch)) == expected_fused(hw, fam, knobs=(knob,)), (hw, fam, knob)
    both = plan_rows(cfg, DTYPES[fam], keep=True, knobs=("YOLO_NO_HALO", "YOLO_NO_S2"), monkeypatch=monkeypatch)
    assert fused_of(both) == {}          # every conv through the tiled kernel (the image layer: its direct kernel)
    if hw == (27, 37):          # the negative case, named: one 13 x 13 block over 7 x 10 pixels wastes 141 %
        assert all(r["fused"] != "resblock" for r in plan_rows(cfg, DTYPES[fam]))


@pytest.mark.parametrize("hw", PAIR_SIZES)
def test_plan_rows_of_the_stage_in_split_fp16(monkeypatch, hw):
    cfg = stage_cfg(hw)
    rows = plan_rows(cfg, hip.FP16X2)
    assert fused_of(rows) == expected_fused(hw, "fp16x2")
    assert ("pair-stem" in {r["fused"] for r in rows}) == (hw != (27, 37))          # odd size: the pair stem must not be planned
    assert fused_of(plan_rows(cfg, hip.FP16X2, keep=True)) == {}
    assert fused_of(plan_rows(cfg, hip.FP16X2, knobs=("YOLO_NO_PAIR_STEM",), monkeypatch=monkeypatch)) == {}


@pytest.mark.parametrize("fam", ["bf16", "fp16"])
@pytest.mark.parametrize("hw", VARIANT_SIZES)
def test_plan_rows_of_the_variants(monkeypatch, hw, fam):
    """mixed activations, one bias-only layer, yolo_input_mul / add: the same fusions.  Channel windows: every fusion survives the extra
    readers -- the stem asks only that layer 0 has one reader, conv3 + stride-2 that layers 3 and 4 have one, the block that its 1x1 has one
    -- and the tensors sit where the docstring of stage_cfg says"""
    for cfg in (mixed_cfg(hw), stage_cfg(hw, affine=True), stage_cfg(hw, cat=True)):
        for keep in (False, True):
            assert fused_of(plan_rows(cfg, DTYPES[fam], keep=keep)) == expected_fused(hw, fam, keep=keep), (hw, fam, keep)
        for knob in KNOBS:
            assert fused_of(plan_rows(cfg, DTYPES[fam], knobs=(knob,), monkeypatch=monkeypatch)) == expected_fused(hw, fam, knobs=(knob,))
    for keep in (False, True):
        rows = plan_rows(stage_cfg(hw, cat=True), DTYPES[fam], keep=keep)
        assert rows[1]["storage"] == rows[2]["storage"] == rows[9]["storage"] != rows[3]["storage"]               # layers 1 and 2 are windows of the first concatenation
        assert rows[5]["storage"] == rows[8]["storage"] == rows[11]["storage"] == rows[12]["storage"]             # layer 5, the block's output and layer 11 of the second
        assert rows[7]["storage"] == rows[12]["storage"] or keep                                                   # (the conv whose shortcut is folded writes the shortcut's window)
    secs = IO.parse_cfg(mixed_cfg(hw))[1:]
    assert {secs[i]["activation"] for i in FUSED_LAYERS} == {"relu", "relie", "linear", "leaky"}
    assert [i for i in FUSED_LAYERS if "batch_normalize" not in secs[i]] == [MIXED_BIAS_ONLY]
    assert all(MIXED_ACTS[a] != MIXED_ACTS[b] for a, b in ((0, 1), (1, 2), (0, 2), (3, 5), (6, 7)))          # a swapped pair within one launch shows
