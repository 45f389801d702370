// Tile selection of libyolo_hip.so: the one rule that says which tile configuration a conv runs (conv_default_cfg / conv_cfg_runs /
// conv_resolve_cfg, declared in kernels.h), the in-situ autotuner and the plan's getter / setter.
#include "yolo_ctx.h"
#include "conv_cfgs.h"

template <int... I> static constexpr bool in_every_family(CfgList<I...>) { return ((Cfgs16::has(I) && CfgsFp8::has(I) && CfgsSplit::has(I) && CfgsPairK::has(I) && CfgsPairKPlain::has(I) && CfgsWide16::has(I)) && ...); }
static_assert(in_every_family(CfgList<0, 2, 4, 6, 8, 14>{}), "every id conv_default_cfg returns is instantiated for every storage family, and with row / column tap masks (a conv of more than 25 taps runs no other form)");

int conv_default_cfg(const ConvArgs &a)
{
    // the image layer: the direct kernel of the storage family wherever it applies.  (Split fp16: ONLY it -- its K grouping differs from the
    // tiled kernel's: were both selectable, a tuned plan would no longer be the built-in plan bit for bit)
    if (a.split || a.pairk ? conv_c8_direct_pair_ok(a) : conv_c8_direct_ok(a)) return CONV_CFG_DIRECT;
    const long M = (long)a.N * a.Ho * a.Wo;
    if (a.Cout <= 32) return 4;
    if (a.Cout <= 64) return M >= 65536 ? 8 : 6;
    const long tiles128 = ((M + 127) / 128) * ((a.Cout + 127) / 128);
    if (tiles128 < 512) return M < 8192 && tiles128 < 128 ? 14 : 2;
    return 0;
}

bool conv_cfg_runs(const ConvArgs &a, int cfg)
{
    if (a.split || a.pairk) {
        if (conv_c8_direct_pair_ok(a) || cfg == CONV_CFG_DIRECT) return cfg == CONV_CFG_DIRECT && conv_c8_direct_pair_ok(a);
        if (conv_cfg_is_halo(cfg) && a.out_dt == DT_F32) return false;      // (the halo forms write no fp32 head)
    } else if (cfg == CONV_CFG_DIRECT) return conv_c8_direct_ok(a);
    return conv_cfg_is_halo(cfg) ? conv_halo_cfg_ok(a, cfg) : conv_cfg_instantiated(a, cfg);
}

int conv_resolve_cfg(const ConvArgs &a, int planned)
{
    // a plan tuned at another batch or input size may hold a halo form (or DIRECT) that no longer applies, and the plan of one storage
    // family ids another does not instantiate: the layer then runs its default
    return planned >= 0 && conv_cfg_runs(a, planned) ? planned : conv_default_cfg(a);
}

extern "C" {

// Tile selection is measured IN SITU: every candidate configuration is timed inside the real layer sequence (per-layer
// events around a full forward), not as the same kernel launched back to back.  Back-to-back timing flatters
// configurations that live off a warm L2: in the real sequence each layer's filters come cold from HBM (124 MB of
// filters and up to 350 MB of activations pass through the 32 MB of L2 / 256 MB of Infinity Cache between two uses), and
// the deep, filter-heavy layers ran 0.069 ms in the network against 0.050 ms in isolation.
int yolo_autotune(yolo_ctx *c, int n, int iters)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "weights not loaded");
    if (c->dtype == YOLO_FP32) return YOLO_OK;
    if (n < 1 || n > c->max_batch || iters < 1) return fail(c, YOLO_ERR_INVALID, "bad n/iters");
    HIPCK(c, hipSetDevice(c->device));
    const int NL = (int)c->layers.size();
    auto shape_key = [&](const Layer &L) {
        ConvArgs a = conv_args(c, L, n);
        char key[128]; snprintf(key, sizeof key, "%d_%d_%d_%d_%d_%d_%d%d_%d%d%d", a.H, a.W, a.Cin_pad, a.Cout, a.ksize, a.stride, a.in_dt, a.out_dt, a.res != nullptr, a.split, a.pairk);
        return std::string(key);
    };
    auto valid = [&](const Layer &L, int cfg) { return !fixed_kernel(L) && conv_cfg_runs(conv_args(c, L, n), cfg); };      // (a fused stem / block: nothing to choose)
    for (auto &L : c->layers) L.tail_on = false;
    std::vector<int> fallback(NL, -1);
    for (int i = 0; i < NL; ++i) if (c->layers[i].type == L_CONV && !fixed_kernel(c->layers[i])) fallback[i] = conv_default_cfg(conv_args(c, c->layers[i], n));
    std::map<std::string, std::map<int, double>> score;          // shape -> cfg -> summed ms over the layers of that shape
    std::vector<float> ms(NL);
    for (int ci = 0; ci <= conv_num_cfgs(); ++ci) {
        const int cfg = ci == conv_num_cfgs() ? CONV_CFG_DIRECT : ci;
        bool any = false;
        for (int i = 0; i < NL; ++i) {
            Layer &L = c->layers[i];
            if (L.type != L_CONV) continue;
            const bool ok = valid(L, cfg);
            L.tile_cfg = ok ? cfg : fallback[i]; any |= ok;
        }
        if (!any) continue;
        // a configuration a layer cannot launch (LDS / 2 GiB window) must not abort the pass: probe once
        for (int i = 0; i < NL; ++i) {
            Layer &L = c->layers[i];
            if (L.type != L_CONV || L.tile_cfg != cfg || fixed_kernel(L)) continue;
            ConvArgs a = conv_args(c, L, n);
            hipError_t e = a.in_dt == DT_FP8 ? launch_conv_fp8(a, cfg, c->stream) : launch_conv_bf16(a, cfg, c->stream);
            if (e != hipSuccess) { (void)hipGetLastError(); L.tile_cfg = fallback[i]; }
        }
        int r = yolo_time_layers(c, n, iters, ms.data()); if (r) return r;
        for (int i = 0; i < NL; ++i) {
            const Layer &L = c->layers[i];
            if (L.type == L_CONV && L.tile_cfg == cfg && !fixed_kernel(L)) score[shape_key(L)][cfg] += ms[i];
        }
        if (getenv("YOLO_TUNE_VERBOSE")) {
            std::map<std::string, double> seen;
            for (int i = 0; i < NL; ++i) if (c->layers[i].type == L_CONV && c->layers[i].tile_cfg == cfg && !fixed_kernel(c->layers[i])) seen[shape_key(c->layers[i])] = score[shape_key(c->layers[i])][cfg];
            for (auto &kv : seen) fprintf(stderr, "tune %s cfg %d %-16s %.4f ms (sum over the layers of this shape, in situ)\n", kv.first.c_str(), cfg, conv_cfg_name(cfg), kv.second);
        }
    }
    for (int i = 0; i < NL; ++i) {
        Layer &L = c->layers[i];
        if (L.type != L_CONV || fixed_kernel(L)) continue;
        auto it = score.find(shape_key(L));
        int best = fallback[i]; double bt = 1e30;
        if (it != score.end()) for (auto &kv : it->second) if (kv.second < bt) { bt = kv.second; best = kv.first; }
        L.tile_cfg = best;
    }
    // second pass: fold 1x1 convs into their producers where that beats the best unfused pair.  Base = the plan just
    // chosen; candidate = every tail-capable tile shape on all producers at once; decided per producer shape.
    {
        int r = yolo_time_layers(c, n, iters, ms.data()); if (r) return r;
        std::vector<float> base(ms);
        std::vector<int> base_cfg(NL, -1);
        for (int i = 0; i < NL; ++i) base_cfg[i] = c->layers[i].tile_cfg;
        std::map<std::string, std::pair<double, int>> best;         // producer shape (+ kind of tail) -> (pair time, cfg), cfg -1 = unfused
        auto tail_key = [&](const Layer &L) { return shape_key(L) + (c->layers[L.tail_layer].head ? "_head" : ""); };      // (a head as the tail: another set of configurations can host it)
        for (int i = 0; i < NL; ++i) {
            const Layer &L = c->layers[i];
            if (L.type != L_CONV || L.tail_layer < 0) continue;
            auto &b = best[tail_key(L)];
            if (b.second == 0 && b.first == 0) b = {0.0, -1};
            b.first += base[i] + base[L.tail_layer];
        }
        for (int cfg = 0; cfg < conv_num_cfgs(); ++cfg) {
            bool any = false;
            for (int i = 0; i < NL; ++i) {
                Layer &L = c->layers[i];
                if (L.type != L_CONV || L.tail_layer < 0) continue;
                const bool ok = conv_cfg_tail_ok(cfg, L.filters, L.in_dt == DT_FP8, c->layers[L.tail_layer].head) && c->layers[L.tail_layer].in_dt == L.in_dt && valid(L, cfg);      // (valid: e.g. a shape the e4m3 table does not instantiate, a halo form that does not fit)
                L.tile_cfg = ok ? cfg : base_cfg[i]; L.tail_on = ok; any |= ok;
            }
            if (!any) continue;
            r = yolo_time_layers(c, n, iters, ms.data()); if (r) return r;
            std::map<std::string, double> t;
            for (int i = 0; i < NL; ++i) {
                const Layer &L = c->layers[i];
                if (L.type == L_CONV && L.tail_layer >= 0 && L.tail_on) t[tail_key(L)] += ms[i] + ms[L.tail_layer];
            }
            for (auto &kv : t) {
                auto &b = best[kv.first];
                if (getenv("YOLO_TUNE_VERBOSE")) fprintf(stderr, "tune-tail %s cfg %d %-16s fused pair %.4f ms (unfused best so far %.4f)\n", kv.first.c_str(), cfg, conv_cfg_name(cfg), kv.second, b.first);
                if (kv.second < b.first) b = {kv.second, cfg};
            }
        }
        for (int i = 0; i < NL; ++i) {
            Layer &L = c->layers[i];
            if (L.type != L_CONV || L.tail_layer < 0) continue;
            const auto &b = best[tail_key(L)];
            L.tail_on = b.second >= 0; L.tile_cfg = b.second >= 0 ? b.second : base_cfg[i];
        }
    }
    drop_graph(c);
    return YOLO_OK;
}

int yolo_get_tile_configs(const yolo_ctx *c, int32_t *cfgs)
{
    if (!c || !cfgs) return YOLO_ERR_INVALID;
    // a conv whose plan folds the following 1x1 conv into its epilogue is reported as cfg + 10000
    for (size_t i = 0; i < c->layers.size(); ++i) {
        const Layer &L = c->layers[i];
        cfgs[i] = L.type == L_CONV ? (L.tail_on && L.tile_cfg >= 0 ? L.tile_cfg + 10000 : L.tile_cfg) : -1;
    }
    return YOLO_OK;
}

// What run_conv would launch at batch n under the plan as it stands: yolo_set_tile_configs stores any in-range id, and a layer whose id
// does not run (another storage family's, a halo form that does not fit) falls back to its default without a word.  No device call, no state.
int yolo_resolved_tile_configs(const yolo_ctx *c, int n, int32_t *out)
{
    if (!c || !out || n < 1 || n > c->max_batch) return YOLO_ERR_INVALID;
    for (size_t i = 0; i < c->layers.size(); ++i) {
        const Layer &L = c->layers[i];
        // -1: no [convolutional] layer, a fixed kernel (stem / block / conv3 / stride-2), a 1x1 computed in its producer's epilogue, fp32 (no tile ids)
        const bool tiled = L.type == L_CONV && !fixed_kernel(L) && !rides_as_tail(c, L) && c->dtype != YOLO_FP32;
        out[i] = tiled ? conv_resolve_cfg(conv_args(c, L, n), L.tile_cfg) : -1;
    }
    return YOLO_OK;
}

int yolo_set_tile_configs(yolo_ctx *c, const int32_t *cfgs)
{
    if (!c || !cfgs) return YOLO_ERR_INVALID;
    for (size_t i = 0; i < c->layers.size(); ++i) {
        if (c->layers[i].type != L_CONV) continue;
        int v = cfgs[i]; bool tail = false;
        if (v >= 10000) { v -= 10000; tail = true; }
        if (v != -1 && v != CONV_CFG_DIRECT && (v < 0 || v >= conv_num_cfgs())) return fail(c, YOLO_ERR_INVALID, "layer %zu: tile config %d out of range", i, v);
        if (tail && (c->layers[i].tail_layer < 0 || !conv_cfg_tail_ok(v, c->layers[i].filters, c->layers[i].in_dt == DT_FP8, c->layers[c->layers[i].tail_layer].head) || c->layers[c->layers[i].tail_layer].in_dt != c->layers[i].in_dt))
            return fail(c, YOLO_ERR_INVALID, "layer %zu: plan asks for a fused 1x1 tail this layer / tile config cannot run", i);
        if (tail && fixed_kernel(c->layers[i])) return fail(c, YOLO_ERR_INVALID, "layer %zu runs a fixed kernel (stem / conv3 / block / stride-2): it hosts no fused 1x1 tail", i);
        // (any id, not the halo forms alone: with a tiled id its storage family does not instantiate -- 44 and 50 on e4m3 operands -- the layer
        // would fall back to its default id, which hosts no tail, and the forward would refuse the plan)
        if (tail && !conv_cfg_runs(conv_args(c, c->layers[i], c->max_batch), v))
            return fail(c, YOLO_ERR_INVALID, "layer %zu: tile config %d does not run on this layer (its storage type does not instantiate it, or a halo-staged form does not fit), so it cannot carry the fused 1x1 tail", i, v);
        c->layers[i].tile_cfg = v; c->layers[i].tail_on = tail;
    }
    drop_graph(c);
    return YOLO_OK;
}

}  // extern "C"
