"""Every tile configuration of the implicit-GEMM conv (csrc/conv_cfgs.h) at the conv geometries the planner serves off YOLO's: rectangular
inputs, pad=0 / padding=2, stride 3, ragged channel counts, reads and writes of concat windows at channel offsets that are no multiples of
64, the fp32 map store of a 16-bit kernel, a 27-pixel layer hosting the fused 1x1 tail.  The autotuner may put any id conv_cfg_runs()
admits on any tunable layer, and a tuned plan is trusted to equal the built-in plan bit for bit: here the default plan is checked layer by
layer against the restatements of each storage family ON THE DEVICE'S OWN stored inputs (the bounds of test_gpu_edges.py, test_gpu_fp8.py,
test_gpu_fp16x2.py, unchanged), and then every id is forced on every conv layer and compared with the default plan bit for bit.  A pair
(layer, id) counts only where Engine.resolved_tile_configs says the layer launches that id -- a layer an id does not apply to falls back
to its default without a word -- and the coverage is asserted, never assumed."""
import numpy as np
import pytest
from oracle import yolo_ref as R
from yolo_tensorflow_amd import darknet_io as IO
from test_edges_host import conv_geometry, layer_inputs, stream_params
from test_gpu_edges import _c, _check_conv, _check_layers, _dt as _dt16, _round
from test_gpu_fp8 import _codes_close, _conv_ref
from test_gpu_fp16x2 import SPLIT_CFGS, SPLIT_HALO, _emu_conv

pytestmark = pytest.mark.gpu
FAMILIES = ("bf16", "fp16", "fp8", "fp16x2")
B = 3
DIRECT = 1000                                                            # CONV_CFG_DIRECT: the image layer's direct kernel, outside the tile table
# the id lists of csrc/conv_cfgs.h (SPLIT_CFGS / SPLIT_HALO of test_gpu_fp16x2.py: CfgsPairK / CfgsHaloPairK)
CFGS16 = tuple(range(0, 36)) + tuple(range(44, 54))
CFGS_FP8 = (0, 2, 4, 6, 8, 12, 14, 16, 17, 19, 20, 23, 31, 32, 33, 34, 45, 48, 49, 51)
HALO13 = tuple(range(36, 44))                                            # the halo-staged forms on 13 x 13 blocks
HALO_RECT = (54, 55, 56)                                                 # ... on 10 x 19 / 5 x 19 blocks: neither network tiles into them
TILED = {"bf16": CFGS16, "fp16": CFGS16, "fp8": CFGS_FP8, "fp16x2": SPLIT_CFGS}
HALO = {"bf16": {1: HALO13, 4: HALO13}, "fp16": {1: HALO13, 4: HALO13}, "fp8": {4: HALO13}, "fp16x2": {1: SPLIT_HALO, 4: SPLIT_HALO}}      # HALO_EDGES: layer -> ids
TAILS = {"bf16": [32, 44, 45, 50], "fp16": [32, 44, 45, 50], "fp8": [31, 32, 45], "fp16x2": []}          # 8-wave shapes of 256 channels the family instantiates


# 11 high x 13 wide (output H x W x C; M = 3 * H * W pixels):
#  0 conv 3x3 padding=1 -> 11x13x96, M 429: the image layer through the tiled kernel (96 filters: not the direct kernel's), Cin_pad 8 --
#    up to 8 taps per K-step, the per-lane tap cursor | 1 conv 3x3 padding=0 -> 9x11x136, M 297: Cin 96 is a whole K-step of the BK = 32 ids
#    (scalar tap cursor) and none of the BK = 64 ids; K = 864 -> Kpad 896, a half-empty last K-step; written into the concat at channel offset 72
#  | 2 conv 1x1 -> 72: reads that window (pixel stride 208, offset 72), writes the window at offset 0 | 3 route -1,-2 -> 208 | 4 conv 3x3
#  stride 2 padding=2 -> 6x7x264, M 126: 264 = 256 + 8, a second channel tile of one granule | 5 conv 1x1 linear -> 264 (Cin 264, 264 % 32 = 8)
#  | 6 shortcut from=-2 (folded into 5's epilogue in the plan that keeps no layer) | 7 conv 3x3 padding=2 -> 8x9x255: the output grows
#  | 8 conv 3x3 stride 3 padding=1 -> 3x3x40, M 27: Cin 255 -> 256, scalar tap cursor, the padding lane zeroed; less than one pixel tile
#  | 9 conv 3x3 padding=1 -> 256 (Cin 40): hosts the fused tail | 10 conv 1x1 -> 128: the tail | 11 conv 1x1 stride 2 padding=1 linear -> 3x3x6:
#  a padded, strided 1x1; the fp32 map store.   Split fp16 refuses ragged routes: there 136 -> 160 and 72 -> 64.
def tile_edges(a=136, b=72):
    return ("[net]\nbatch=1\nwidth=13\nheight=11\nchannels=3\nyolo_output=map\n\n" + _c(96, 3, padding=1) + _c(a, 3) + _c(b, 1) + "[route]\nlayers=-1,-2\n\n" +
            _c(264, 3, stride=2, padding=2) + _c(264, 1, act="linear") + "[shortcut]\nfrom=-2\nactivation=linear\n\n" + _c(255, 3, padding=2) +
            _c(40, 3, stride=3, padding=1) + _c(256, 3, padding=1) + _c(128, 1) + _c(6, 1, stride=2, padding=1, act="linear"))


# 13 high x 26 wide, two 13 x 13 blocks per image:  0 conv 3x3 -> 64, at offset 136 of the concat | 1 conv 3x3 -> 136: halo-eligible, reads
# layer 0 from that window (pixel stride 200), writes the window at offset 0, ragged Cout | 2 route -1,-2 | 3 conv 1x1 -> 128 | 4 conv 3x3
# linear -> 128: halo-eligible with e4m3 operands too (Cin 128) | 5 shortcut from=-2 (folded into 4) | 6 conv 1x1 linear -> the 6-channel map
def halo_edges(a=136):
    return ("[net]\nbatch=1\nwidth=26\nheight=13\nchannels=3\nyolo_output=map\n\n" + _c(64, 3, padding=1) + _c(a, 3, padding=1) + "[route]\nlayers=-1,-2\n\n" +
            _c(128, 1) + _c(128, 3, padding=1, act="linear") + "[shortcut]\nfrom=-2\nactivation=linear\n\n" + _c(6, 1, act="linear"))


# 9 high x 11 wide.  The scalar tap cursor under padding >= 2, the product in which the conv last read zeros for taps inside the image (the
# window origin of a border pixel lies `padding` rows and columns outside it; test_gpu_edges.py pins it under the built-in id only), and no
# layer of the two networks above has both:  0 conv 3x3 -> c | 1 conv 3x3 padding=2 -> 11x13xc, c input channels: whole K-steps of every id
# (c = 64; e4m3 operands: 128) | 2 conv 3x3 stride 2 padding=3 -> 8x9x24: the windows of the border pixels lie wholly outside the image,
# their output is the bias | 3 conv 1x1 linear -> the 6-channel map
def wide_pad(c=64):
    return ("[net]\nbatch=1\nwidth=11\nheight=9\nchannels=3\nyolo_output=map\n\n" + _c(c, 3, padding=1) + _c(c, 3, padding=2) + _c(24, 3, stride=2, padding=3) +
            _c(6, 1, act="linear"))


# name -> (builder, its arguments, ... with split-fp16 pairs, ... with e4m3 operands, input height, width)
NETS = {"tile_edges": (tile_edges, (136, 72), (160, 64), (136, 72), 11, 13), "halo_edges": (halo_edges, (136,), (160,), (136,), 13, 26),
        "wide_pad": (wide_pad, (64,), (64,), (128,), 9, 11)}


def net_cfg(net, fam):
    make, plain, pairs, e4m3, h, w = NETS[net]
    return make(*(pairs if fam == "fp16x2" else e4m3 if fam == "fp8" else plain)), h, w


def _dt(hiplib, fam):
    return hiplib.FP8 if fam == "fp8" else hiplib.FP16X2 if fam == "fp16x2" else _dt16(hiplib, fam)


class Net:
    """one network in one storage family: the engine that keeps every layer, its default plan and that plan's stored layers and map"""
    def __init__(self, hiplib, net, fam):
        self.net, self.fam, self.hip = net, fam, hiplib
        self.cfg, h, w = net_cfg(net, fam)
        secs = IO.parse_cfg(self.cfg); self.secs = secs[1:]
        self.flat = IO.synth_weights(secs, seed=101 + h)
        if fam in ("bf16", "fp16"):
            self.flat = IO.bf16_exact_filters(secs, self.flat)
        self.imgs = np.random.default_rng(102 + h).integers(0, 256, (B, h, w, 3), dtype=np.uint8)
        self.x0 = self.imgs.astype(np.float32) * np.float32(1.0 / 255.0)          # k_preprocess: byte * scale, then the storage type's rounding
        self.convs = [i for i, s in enumerate(self.secs) if s["type"] == "convolutional"]
        self.readers = {i: [j for j in range(len(self.secs)) if i in layer_inputs(self.secs, j)] for i in self.convs}
        self.eng = self.engine(True)
        self.base = self.eng.get_tile_configs().copy()
        assert (self.base[self.convs] == -1).all()                                # the built-in plan: no tuned id, no tail
        self.default = self.eng.resolved_tile_configs(B)
        self.eng.forward(self.imgs, want_detections=False)
        self.outs = [self.fetch(self.eng, i, B) for i in range(self.eng.num_layers)]
        self.map = self.eng.output_map(B)
        self.sweep = None

    def engine(self, keep):
        e = self.hip.Engine(self.cfg, max_batch=B, dtype=_dt(self.hip, self.fam), semantics=self.hip.SEM_DARKNET, keep_layers=keep)
        e.set_weights(self.flat)
        return e

    def fetch(self, eng, i, n):
        """layer i's stored tensor; an e4m3 concatenation is read through its sources (the library hands out no tensor of several scales)"""
        if self.fam == "fp8" and self.secs[i]["type"] == "route" and "," in self.secs[i]["layers"]:
            return np.concatenate([eng.layer_output(j, n) for j in layer_inputs(self.secs, i)], axis=-1)
        return eng.layer_output(i, n)

    def tunable(self):
        """conv layers whose built-in id is a tile id (not the image layer's direct kernel)"""
        return [i for i in self.convs if 0 <= self.default[i] < self.hip.op_conv_num_cfgs()]

    def force(self, eng, base, cfg, layers=None):
        """`cfg` on every conv layer (or `layers`) of a copy of `base`; -> the ids the layers then launch"""
        plan = base.copy(); plan[self.convs if layers is None else layers] = cfg
        eng.set_tile_configs(plan)
        return eng.resolved_tile_configs(B)


@pytest.fixture(scope="module")
def nets(hiplib):
    cache = {}

    def get(net, fam):
        if (net, fam) not in cache:
            cache[net, fam] = Net(hiplib, net, fam)
        return cache[net, fam]
    yield get
    for n in cache.values():
        n.eng.close()


CASES = [(net, fam) for net in NETS for fam in FAMILIES]


def test_the_fixture_networks_are_what_their_comments_say(hiplib):
    for net, (make, ragged, whole32, _, h, w) in NETS.items():
        for fam in FAMILIES:
            cfg = net_cfg(net, fam)[0]
            for keep in (True, False):
                rc, table = hiplib.plan_table(cfg, dtype=_dt(hiplib, fam), max_batch=B, keep_layers=keep)
                assert rc == 0, (net, fam, keep, table)
                rows = table.splitlines()
                assert all("kernel=tiled" in r and "fused=none" in r for r in rows if " convolutional " in r), table      # no fixed kernel: every conv is tunable
                if not keep and net != "wide_pad":          # the plan that keeps no layer folds the shortcut, and (not on pairs) offers the 1x1 behind the 3 x 3 x 256 conv as a tail
                    fold, tail = (5, 9) if net == "tile_edges" else (4, None)
                    assert "residual_from=%d" % (fold - 1) in rows[fold], rows[fold]
                    if tail is not None:
                        assert ("tail_layer=%d" % (tail + 1) in rows[tail]) == (fam != "fp16x2"), rows[tail]
        if ragged != whole32:
            rc, msg = hiplib.plan_table(make(*ragged), dtype=hiplib.FP16X2, max_batch=B)
            assert rc != 0 and "32-channel groups" in msg
    shapes = [s[1:4] for s in IO.layer_shapes(IO.parse_cfg(tile_edges()))]
    assert shapes == [(11, 13, 96), (9, 11, 136), (9, 11, 72), (9, 11, 208), (6, 7, 264), (6, 7, 264), (6, 7, 264), (8, 9, 255), (3, 3, 40), (3, 3, 256), (3, 3, 128), (3, 3, 6)]
    assert [s[1:4] for s in IO.layer_shapes(IO.parse_cfg(halo_edges()))] == [(13, 26, 64), (13, 26, 136), (13, 26, 200), (13, 26, 128), (13, 26, 128), (13, 26, 128), (13, 26, 6)]
    assert [s[1:4] for s in IO.layer_shapes(IO.parse_cfg(wide_pad()))] == [(9, 11, 64), (11, 13, 64), (8, 9, 24), (8, 9, 6)]


# ---- (a) the default plan, every layer on the device's own stored input of that layer ----
def _slope_act(sec):
    assert sec["activation"] in ("leaky", "linear")
    return sec["activation"] == "leaky"


def _check_fp8(N):
    """e4m3 storage at unit scales: test_gpu_fp8.py's _conv_ref per layer under _codes_close; the image layer runs bf16 operands and the
    fp32 map is not quantised (oracle.fp8_scheme_forward: the first conv, a head), the latter under that file's head rule.  -> the
    smallest fraction of bit-identical codes over the layers"""
    params = stream_params(N.cfg, N.flat); worst = 1.0
    for i, s in enumerate(N.secs):
        got = N.outs[i]; what = "%s fp8 layer %d (%s)" % (N.net, i, s["type"])
        ins = [N.outs[j] if j >= 0 else None for j in layer_inputs(N.secs, i)]
        if s["type"] == "route":
            assert np.array_equal(got, np.concatenate(ins, axis=-1)), what
            continue
        if s["type"] == "shortcut":
            worst = min(worst, _codes_close(got, R.to_fp8_e4m3(ins[0] + ins[1]), 1.0, what, operands=(ins[0], ins[1])))
            continue
        k, st, pad = conv_geometry(s); p = params[i]; leaky = _slope_act(s)
        if i == 0:
            y = R.conv2d_nhwc(R.to_bf16(N.x0), R.to_bf16(p["w"]), st, pad) + p["bias"]
            want = R.to_fp8_e4m3(R.to_bf16(R.leaky_relu(y) if leaky else y))
        elif i == len(N.secs) - 1:
            amax = np.abs(p["w"]).max(axis=(0, 1, 2)); osc = np.where(amax > 0, amax / np.float32(448), np.float32(1)).astype(np.float32)
            y = (R.conv2d_nhwc(ins[0], R.to_fp8_e4m3(p["w"] / osc[None, None, None, :]), st, pad).astype(np.float64) * osc + p["bias"].astype(np.float64)).astype(np.float32)
            want = R.leaky_relu(y) if leaky else y
            print("%s: max err %.3e of scale %.3f" % (what, float(np.abs(got - want).max()), float(np.abs(want).max())))
            np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-3 * float(np.abs(want).max()), err_msg=what)
            continue
        else:
            want, _ = _conv_ref(ins[0], p["w"], p["bias"], st, None, pad, leaky)
        assert float(np.abs(want).max()) < 448.0, what          # (unit scales hold these tensors: nothing saturates)
        same = _codes_close(got, want, 1.0, what)
        print("%s (%d/%d/%d): %.5f of the codes identical" % (what, k, st, pad, same))
        worst = min(worst, same)
    return worst


def _check_fp16x2(N):
    """split fp16: test_gpu_fp16x2.py's _emu_conv per layer at that file's 4e-6 of the tensor's scale; -> the worst error / scale"""
    params = stream_params(N.cfg, N.flat); worst = 0.0
    for i, s in enumerate(N.secs):
        got = N.outs[i]; what = "%s fp16x2 layer %d (%s)" % (N.net, i, s["type"])
        ins = [N.outs[j] if j >= 0 else N.x0 for j in layer_inputs(N.secs, i)]
        if s["type"] == "route":
            assert np.array_equal(got, np.concatenate(ins, axis=-1)), what
            continue
        if s["type"] == "shortcut":
            h, l = R.split_f16(ins[0] + ins[1]); want = h + l
        else:
            k, st, pad = conv_geometry(s); p = params[i]
            want = _emu_conv(ins[0], p["w"], p["bias"], st, 1 if _slope_act(s) else 0, None, pad, f32_out=i == len(N.secs) - 1)
        assert got.shape == want.shape and np.isfinite(got).all(), what
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        print("%s: max err %.3e of the tensor's scale" % (what, rel))
        assert rel <= 4e-6, what
        worst = max(worst, rel)
    return worst


@pytest.mark.parametrize("net,fam", CASES)
def test_default_plan_layers_on_their_stored_inputs(hiplib, nets, net, fam):
    N = nets(net, fam)
    assert np.array_equal(N.map, N.outs[-1]) and np.isfinite(N.map).all() and float(np.abs(N.map).max()) > 0.1
    if fam == "fp8":
        print("%s fp8: default plan, worst layer %.5f of the codes identical (bound 0.997)" % (net, _check_fp8(N)))
    elif fam == "fp16x2":
        print("%s fp16x2: default plan, worst layer %.3e of the tensor's scale (bound 4e-6)" % (net, _check_fp16x2(N)))
    else:
        seen = _check_layers(hiplib, fam, N.cfg, N.flat, N.outs, hiplib.SEM_DARKNET)
        _check_conv(hiplib, fam, N.secs[0], stream_params(N.cfg, N.flat)[0], _round(fam, N.x0), N.outs[0], "%s layer 0 (the image layer)" % net)
        want = {"tile_edges": {("conv", 3, 1, 1), ("conv", 1, 1, 0), "route", "shortcut", ("conv", 3, 1, 0), ("conv", 3, 2, 2), ("conv", 3, 1, 2), ("conv", 3, 3, 1), ("conv", 1, 2, 1)},
                "halo_edges": {("conv", 3, 1, 1), ("conv", 1, 1, 0), "route", "shortcut"}, "wide_pad": {("conv", 3, 1, 2), ("conv", 3, 2, 3), ("conv", 1, 1, 0)}}[net]
        assert want <= seen, seen
    if net == "wide_pad":          # padding=3 under a 3x3 conv: the window of a corner pixel lies wholly outside the image, its output is the activated bias
        p = stream_params(N.cfg, N.flat)[2]; b = np.where(p["bias"] > 0, p["bias"], np.float32(0.1) * p["bias"]).astype(np.float32)
        corner = {"bf16": R.to_bf16, "fp16": R.to_f16, "fp8": lambda v: R.to_fp8_e4m3(R.to_bf16(v)), "fp16x2": lambda v: sum(R.split_f16(v))}[fam](b)
        assert np.array_equal(N.outs[2][:, 0, 0], np.broadcast_to(corner, (B, 24)))


# ---- (b), (c) every id on every conv layer == the default plan, and what that covered ----
def _sweep(N):
    """{id: [layers that launched it]} of the keep-layers engine, every such layer and its readers compared with the default plan"""
    if N.sweep is not None:
        return N.sweep
    hit = {}
    try:
        for cfg in range(N.hip.op_conv_num_cfgs()):
            res = N.force(N.eng, N.base, cfg)
            on = [i for i in N.convs if res[i] == cfg]
            assert all(res[i] == N.default[i] for i in N.convs if i not in on), (cfg, res)          # the others: their default
            if not on:
                continue
            N.eng.forward(N.imgs, want_detections=False)          # (a launch the library refuses raises: a failure, not a skip)
            for j in sorted(set(on) | {r for i in on for r in N.readers[i]}):
                got = N.fetch(N.eng, j, B)
                bad = np.argwhere(got != N.outs[j])
                assert bad.size == 0, "%s %s: tile config %d on layers %s: layer %d differs from the default plan in %d elements, first at %s (got %r, default %r)" % (
                    N.net, N.fam, cfg, on, j, len(bad), bad[0].tolist(), got[tuple(bad[0])], N.outs[j][tuple(bad[0])])
            assert np.array_equal(N.eng.output_map(B), N.map), (N.net, N.fam, cfg)
            hit[cfg] = on
    finally:
        N.eng.set_tile_configs(N.base)
    N.sweep = hit
    return hit


@pytest.mark.parametrize("net,fam", CASES)
def test_every_tile_config_equals_the_default_plan(hiplib, nets, net, fam):
    N = nets(net, fam)
    hit = _sweep(N)
    tunable = N.tunable()
    print("%s %s: %d (layer, id) pairs over %d ids on the tunable layers %s; built-in ids %s" % (net, fam, sum(len(v) for v in hit.values()), len(hit), tunable, N.default[N.convs].tolist()))
    assert not set(hit) & set(HALO_RECT)                                 # 10 x 19 / 5 x 19 blocks: refused, through the accessor
    if net == "tile_edges":
        assert tunable == N.convs                                         # the image layer too: 96 filters are none of the direct kernels'
        assert len(hit) >= {"bf16": 46, "fp16": 46, "fp8": 20, "fp16x2": 16}[fam]
        assert not set(hit) & set(HALO13 + SPLIT_HALO), hit               # no layer of it is 3x3 / padding 1 on whole 64-channel chunks over 13 x 13 blocks
        for cfg in TILED[fam]:
            assert set(tunable) <= set(hit.get(cfg, ())), "tile config %d ran on %s only" % (cfg, hit.get(cfg))
    elif net == "wide_pad":
        assert {1, 2, 3} <= set(tunable) and not set(hit) & set(HALO13 + SPLIT_HALO)          # (padding 2: no halo-staged form)
        for cfg in TILED[fam]:
            assert set(tunable) <= set(hit.get(cfg, ())), "tile config %d ran on %s only" % (cfg, hit.get(cfg))
    else:
        assert N.default[0] == DIRECT or fam == "fp16x2"               # 3 -> 64 filters: the direct kernel, nothing to tune; pairs: its direct kernel has 16 or 32
        for layer, ids in HALO[fam].items():
            for cfg in ids:
                assert layer in hit.get(cfg, ()), "halo-staged tile config %d did not run on layer %d (ran on %s)" % (cfg, layer, hit.get(cfg))
        eligible = set(HALO[fam])
        for cfg in HALO13 + SPLIT_HALO:
            assert set(hit.get(cfg, ())) <= eligible, (cfg, hit.get(cfg))  # ... and on no other layer (1x1, the 8-channel image, the fp32 map)
        for cfg in TILED[fam]:
            assert set(tunable) <= set(hit.get(cfg, ())), "tile config %d ran on %s only" % (cfg, hit.get(cfg))


# ---- (d) the plan that keeps no layer: folded shortcut, pooled buffers, the fused 1x1 tail at M = 27 ----
@pytest.mark.parametrize("net,fam", CASES)
def test_lean_plan_every_tile_config_and_the_fused_tail(hiplib, nets, net, fam):
    N = nets(net, fam)
    eng = N.engine(False)
    try:
        base = eng.get_tile_configs().copy()
        base = np.where(base >= 10000, base - 10000, base).astype(np.int32)          # (the built-in plan turns no tail on; were it to, off)
        eng.set_tile_configs(base)
        eng.forward(N.imgs, want_detections=False)
        lean = eng.output_map(B)
        bad = np.argwhere(lean != N.map)
        assert bad.size == 0, "%s %s: the plan that keeps no layer differs from the layer-by-layer plan in %d map elements, first at %s" % (net, fam, len(bad), bad[0].tolist())
        pairs = 0
        for cfg in range(hiplib.op_conv_num_cfgs()):
            res = N.force(eng, base, cfg)
            on = [i for i in N.convs if res[i] == cfg]
            if not on:
                continue
            eng.forward(N.imgs, want_detections=False)
            assert np.array_equal(eng.output_map(B), N.map), "%s %s: tile config %d on layers %s, plan that keeps no layer" % (net, fam, cfg, on)
            pairs += len(on)
        print("%s %s, plan that keeps no layer: %d (layer, id) pairs" % (net, fam, pairs))
        assert pairs >= len(TILED[fam]) * (len(N.convs) - 1)
        if net != "tile_edges":
            return
        accepted = []
        for cfg in range(hiplib.op_conv_num_cfgs()):
            trial = base.copy(); trial[9] = 10000 + cfg
            try:
                eng.set_tile_configs(trial)
            except hiplib.YoloError:
                continue          # no 8-wave shape of 256 channels, not instantiated for this storage family, or a halo form (3 x 3 pixels)
            res = eng.resolved_tile_configs(B)
            assert res[9] == cfg and res[10] == -1, (cfg, res)          # what is accepted with the tail runs, and layer 10 launches nothing
            eng.forward(N.imgs, want_detections=False)
            assert np.array_equal(eng.output_map(B), N.map), "%s: the 1x1 conv fused into layer 9 under tile config %d differs from its own launch" % (fam, cfg)
            accepted.append(cfg)
        print("%s %s: fused 1x1 tail at M = 27 under tile configs %s" % (net, fam, accepted))
        assert accepted == TAILS[fam]
    finally:
        eng.close()


# ---- (e) one image of the batch ----
@pytest.mark.parametrize("fam", FAMILIES)
def test_one_image_alone_equals_its_slice_of_the_batch(hiplib, nets, fam):
    """image 1 alone (n = 1 of max_batch 3) under two ids of different pixel-tile heights, 176 and 96 pixels, neither a built-in choice"""
    N = nets("tile_edges", fam)
    try:
        for cfg in (16, 23):
            res = N.force(N.eng, N.base, cfg)
            assert cfg not in N.default.tolist() and all(res[i] == cfg for i in N.tunable())
            N.eng.forward(N.imgs[1:2], want_detections=False)
            for j in range(N.eng.num_layers):
                assert np.array_equal(N.fetch(N.eng, j, 1), N.outs[j][1:2]), (fam, cfg, j)
            assert np.array_equal(N.eng.output_map(1), N.map[1:2])
            assert np.array_equal(N.eng.resolved_tile_configs(1), res)
    finally:
        N.eng.set_tile_configs(N.base)
    with pytest.raises(hiplib.YoloError):
        N.eng.resolved_tile_configs(B + 1)
