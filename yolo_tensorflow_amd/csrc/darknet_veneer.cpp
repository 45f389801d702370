// libdarknet_hip.so: darknet's detection ABI (include/darknet_hip.h) marshalled onto the C ABI of libyolo_hip.so.
// Host code only.  What computes -- the network, the letterbox / resize, the head activations, thresholding + box correction of
// get_network_boxes, both NMS flavours -- is a call into include/yolo_hip.h and runs on the GPU; this file allocates and fills
// darknet's structs, parses the two small text formats darknet.py hands over (.data files, class-name lists) and decodes PPM
// images (the reference decodes JPEG/PNG with the vendored stb_image, which is outside the inference path and not re-implemented).
#include "../../include/darknet_hip.h"
#include "../../include/yolo_hip.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct network {
    yolo_ctx *ctx = nullptr;
    int w = 0, h = 0, c = 3, rows = 0, attrs = 0, batch = 1;
    std::string cfg_text, weights_path;
    std::vector<float> out;              // last layer's output in darknet layout (what network_predict returns)
    std::vector<float> rec;              // get_network_boxes staging: [count][5 + classes]
    bool have = false;
    int fwd_n = 1;                       // images of the last forward (network_predict: batch; network_predict_image: 1)
};

namespace {
int g_device = 0;                        // cuda_set_device

bool read_text(const char *path, std::string &out)
{
    FILE *f = path ? fopen(path, "rb") : nullptr;
    if (!f) return false;
    char buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}

std::string trim(const std::string &s)
{
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) ++a;
    while (b > a && isspace((unsigned char)s[b - 1])) --b;
    return s.substr(a, b - a);
}

// darknet's char-rnn cfgs name `inputs=` and no image size in [net] (examples/rnn.c over rnn.cfg): the library wants such a network declared
// ([net] yolo_input=vector); the key is added behind the [net] line of a cfg that lacks it.  Likewise an image network whose channels= is not 3 (grey,
// RGB-D, the go board): [net] yolo_input=planes
void declare_input_kind(std::string &cfg)
{
    bool in_net = false, inputs = false, declared = false; int height = 0, width = 0, channels = 3; size_t net_end = std::string::npos;
    for (size_t pos = 0; pos < cfg.size();) {
        size_t e = cfg.find('\n', pos); if (e == std::string::npos) e = cfg.size();
        const std::string line = trim(cfg.substr(pos, e - pos));
        if (!line.empty() && line[0] == '[') { if (in_net) break; in_net = true; net_end = e; }
        else if (in_net && !line.empty() && line[0] != '#' && line[0] != ';') {
            const size_t eq = line.find('=');
            const std::string k = trim(line.substr(0, eq)), v = eq == std::string::npos ? "" : trim(line.substr(eq + 1));
            inputs |= k == "inputs"; declared |= k == "yolo_input";
            if (k == "height") height = atoi(v.c_str());
            if (k == "width") width = atoi(v.c_str());
            if (k == "channels") channels = atoi(v.c_str());
        }
        pos = e + 1;
    }
    if (declared || net_end == std::string::npos) return;
    if (inputs && height <= 0 && width <= 0) cfg.insert(net_end, "\nyolo_input=vector");
    else if (height > 0 && width > 0 && channels != 3) cfg.insert(net_end, "\nyolo_input=planes");
}

bool open_ctx(network *net)
{
    yolo_config yc; memset(&yc, 0, sizeof yc);
    const char *dt = getenv("DARKNET_HIP_DTYPE");
    yc.struct_size = sizeof yc; yc.cfg_text = net->cfg_text.c_str(); yc.max_batch = net->batch;
    yc.dtype = dt && !strcmp(dt, "fp32") ? YOLO_FP32 : dt && !strcmp(dt, "fp16") ? YOLO_FP16 : dt && !strcmp(dt, "fp16x2") ? YOLO_FP16X2 : YOLO_BF16;
    yc.semantics = YOLO_SEM_DARKNET; yc.decode = YOLO_DECODE_RATIO; yc.device = g_device;
    char err[512] = {0};
    net->ctx = yolo_create(&yc, err, sizeof err);
    if (!net->ctx) { fprintf(stderr, "darknet_hip: %s\n", err); return false; }
    if (!net->weights_path.empty() && yolo_load_darknet_weights(net->ctx, net->weights_path.c_str(), 0) != YOLO_OK) {
        fprintf(stderr, "darknet_hip: %s\n", yolo_last_error(net->ctx)); yolo_destroy(net->ctx); net->ctx = nullptr; return false;
    }
    yolo_input_size(net->ctx, &net->h, &net->w, &net->c);
    net->rows = yolo_num_rows(net->ctx); net->attrs = yolo_num_attrs(net->ctx);
    net->out.assign(yolo_last_layer_size(net->ctx) * (size_t)net->batch, 0.f);      // net->output: batch * outputs floats
    net->have = false;
    return true;
}

float *fetch_output(network *net)
{
    net->have = yolo_last_layer_output_batch(net->ctx, net->fwd_n, net->out.data(), net->out.size()) == YOLO_OK;
    if (!net->have) { fprintf(stderr, "darknet_hip: %s\n", yolo_last_error(net->ctx)); return nullptr; }
    return net->out.data();
}
}  // namespace

extern "C" {

void cuda_set_device(int n) { g_device = n; }                                        /* DN/cuda.c:12 */

network *load_network(char *cfg, char *weights, int clear)
{
    (void)clear;                                   // `*net->seen = 0`: training state, nothing to clear here
    network *net = new network();
    if (!read_text(cfg, net->cfg_text)) { fprintf(stderr, "darknet_hip: cannot open cfg '%s'\n", cfg ? cfg : "(null)"); delete net; return nullptr; }
    declare_input_kind(net->cfg_text);
    if (weights && weights[0]) net->weights_path = weights;
    if (!open_ctx(net)) { delete net; return nullptr; }
    return net;
}

void free_network(network *net) { if (!net) return; if (net->ctx) yolo_destroy(net->ctx); delete net; }
int network_width(network *net) { return net ? net->w : 0; }
int network_height(network *net) { return net ? net->h : 0; }
// network_predict carries the state of [crnn] / [rnn] / [gru] / [lstm] layers from call to call by itself (one call, one time step); these zero it.
// (Both go through a file-local function: a process that also holds libdarknet itself resolves an exported name to whichever library came first)
static void reset_stream(network *net, int b) { if (net && net->ctx && yolo_reset_state(net->ctx, b) != YOLO_OK) fprintf(stderr, "darknet_hip: %s\n", yolo_last_error(net->ctx)); }
void reset_network_state(network *net, int b) { reset_stream(net, b); }              /* DN/network.c:69 */
void reset_rnn(network *net) { reset_stream(net, 0); }                               /* DN/network.c:85 */

// DN/network.c:339-356 resizes every layer for `b` images; here the plan is rebuilt for that batch (weights are re-read)
void set_batch_network(network *net, int b)
{
    if (!net || b < 1 || b == net->batch) return;
    const int old = net->batch;
    yolo_ctx *prev = net->ctx;
    net->batch = b; net->ctx = nullptr;
    if (!open_ctx(net)) { fprintf(stderr, "darknet_hip: set_batch_network(%d) failed, keeping batch %d\n", b, old); net->batch = old; net->ctx = prev; return; }
    yolo_destroy(prev);
}

// `input`: batch x planar [c][h][w] at network size (c: the cfg's channels=).  Returns net->output: the last layer's output of every image of the batch
// (a classifier cfg: the probabilities of its [softmax] layer, what darknet.py's classify() reads),
// image after image (batch * outputs floats, DN/network.c:497-508), see include/darknet_hip.h.
float *network_predict(network *net, float *input)
{
    if (!net || !input) return nullptr;
    // a vector-input network (char-rnn): `input` is batch x inputs values, one step of the streams 0 .. batch-1
    const int rc = yolo_vector_inputs(net->ctx) > 0 ? yolo_forward_vectors(net->ctx, input, net->batch, YOLO_HOST, nullptr, 0)
                                                    : yolo_forward(net->ctx, input, net->batch, YOLO_IMG_F32_CHW, YOLO_HOST, 1.0f, nullptr, YOLO_HOST);
    if (rc != YOLO_OK) {
        net->have = false; fprintf(stderr, "darknet_hip: %s\n", yolo_last_error(net->ctx)); return nullptr;
    }
    net->fwd_n = net->batch;
    return fetch_output(net);
}

float *network_predict_image(network *net, image im)
{
    if (!net || !im.data) return nullptr;
    if (im.c != net->c) { net->have = false; fprintf(stderr, "darknet_hip: network_predict_image: an image of %d channels for a network of %d\n", im.c, net->c); return nullptr; }
    if (yolo_forward_letterbox_chw(net->ctx, im.data, im.w, im.h, YOLO_HOST, nullptr, YOLO_HOST) != YOLO_OK) {
        net->have = false; fprintf(stderr, "darknet_hip: %s\n", yolo_last_error(net->ctx)); return nullptr;
    }
    net->fwd_n = 1;
    return fetch_output(net);
}

// DN/network.c:526-540: `num` boxes above thresh, each with a zeroed prob array
detection *make_network_boxes(network *net, float thresh, int *num)
{
    if (num) *num = 0;
    if (!net || !net->have) return nullptr;
    if (net->rows == 0) return (detection *)calloc(1, sizeof(detection));      // a classifier: no boxes (DN/network.c:510-524 counts the detection layers)
    int count = 0;
    if (yolo_darknet_boxes(net->ctx, net->w, net->h, thresh, 1, nullptr, 0, &count) != YOLO_OK) { fprintf(stderr, "darknet_hip: %s\n", yolo_last_error(net->ctx)); return nullptr; }
    const int C = net->attrs - 5;
    detection *dets = (detection *)calloc(count > 0 ? count : 1, sizeof(detection));
    for (int i = 0; i < count; ++i) { dets[i].classes = C; dets[i].prob = (float *)calloc(C, sizeof(float)); }
    if (num) *num = count;
    return dets;
}

// DN/network.c:562-567.  Thresholding, ordering and the un-letterboxing run on the device (yolo_darknet_boxes); only the
// surviving boxes cross PCIe and are copied into darknet's structs here.
detection *get_network_boxes(network *net, int w, int h, float thresh, float hier, int *map, int relative, int *num)
{
    if (num) *num = 0;
    if (!net || !net->have) return nullptr;
    if (net->rows == 0) return (detection *)calloc(1, sizeof(detection));      // a classifier: no boxes
    const int A = net->attrs, C = A - 5;
    net->rec.resize((size_t)net->rows * A);
    int count = 0;
    // `hier` and `map` are what a [region] head with a softmax tree reads (DN/region_layer.c:412-424); other heads ignore both
    int32_t tree_nodes = 0;
    yolo_tree_geometry(net->ctx, &tree_nodes, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (tree_nodes > 0 && yolo_set_hier_thresh(net->ctx, hier) != YOLO_OK) { fprintf(stderr, "darknet_hip: %s\n", yolo_last_error(net->ctx)); return nullptr; }
    if (yolo_darknet_boxes_map(net->ctx, 0, w, h, thresh, relative, tree_nodes > 0 ? map : nullptr, net->rec.data(), net->rows, &count) != YOLO_OK) {
        fprintf(stderr, "darknet_hip: %s\n", yolo_last_error(net->ctx)); return nullptr;
    }
    detection *dets = (detection *)calloc(count > 0 ? count : 1, sizeof(detection));
    for (int i = 0; i < count; ++i) {
        const float *p = &net->rec[(size_t)i * A];
        detection &d = dets[i];
        d.bbox = box{p[0], p[1], p[2], p[3]}; d.classes = C; d.objectness = p[4];
        d.prob = (float *)malloc((size_t)C * sizeof(float));
        memcpy(d.prob, p + 5, (size_t)C * sizeof(float));
    }
    if (num) *num = count;
    return dets;
}

void free_detections(detection *dets, int n)
{
    if (!dets) return;
    for (int i = 0; i < n; ++i) { free(dets[i].prob); if (dets[i].mask) free(dets[i].mask); }
    free(dets);
}

void free_ptrs(void **ptrs, int n)                                                   /* DN/utils.c:328 */
{
    if (!ptrs) return;
    for (int i = 0; i < n; ++i) free(ptrs[i]);
    free(ptrs);
}

static void nms_arrays(detection *dets, int total, int classes, float thresh, int by_obj)
{
    if (!dets || total < 1 || classes < 1) return;
    std::vector<float> b((size_t)total * 4), p((size_t)total * classes), o(total);
    for (int i = 0; i < total; ++i) {
        b[4 * i] = dets[i].bbox.x; b[4 * i + 1] = dets[i].bbox.y; b[4 * i + 2] = dets[i].bbox.w; b[4 * i + 3] = dets[i].bbox.h;
        o[i] = dets[i].objectness; memcpy(&p[(size_t)i * classes], dets[i].prob, (size_t)classes * 4);
    }
    if (yolo_op_nms_detections(b.data(), p.data(), o.data(), total, classes, thresh, by_obj, g_device) != YOLO_OK) {
        fprintf(stderr, "darknet_hip: nms: %s\n", yolo_last_error(NULL)); return;
    }
    for (int i = 0; i < total; ++i) { dets[i].objectness = o[i]; memcpy(dets[i].prob, &p[(size_t)i * classes], (size_t)classes * 4); }
}
void do_nms_sort(detection *dets, int total, int classes, float thresh) { nms_arrays(dets, total, classes, thresh, 0); }
void do_nms_obj(detection *dets, int total, int classes, float thresh) { nms_arrays(dets, total, classes, thresh, 1); }

image make_image(int w, int h, int c) { image m; m.w = w; m.h = h; m.c = c; m.data = (float *)calloc((size_t)w * h * c, sizeof(float)); return m; }
void free_image(image m) { free(m.data); }

image letterbox_image(image im, int w, int h)                                        /* DN/image.c:960-981, on the device */
{
    image out = make_image(w, h, im.c);
    if (!im.data || im.c < 1) { fprintf(stderr, "darknet_hip: letterbox_image: no image\n"); return out; }
    if (im.c == 3) { if (yolo_op_letterbox(im.data, im.w, im.h, w, h, 1, out.data, g_device) != YOLO_OK) fprintf(stderr, "darknet_hip: letterbox_image: %s\n", yolo_last_error(NULL)); return out; }
    // any other plane count: the planes are independent, so they go through the three-plane operator three at a time (the last group padded with its own last plane)
    const size_t ip = (size_t)im.w * im.h, op = (size_t)w * h;
    std::vector<float> src(3 * ip), dst(3 * op);
    for (int k0 = 0; k0 < im.c; k0 += 3) {
        for (int k = 0; k < 3; ++k) memcpy(&src[k * ip], im.data + (size_t)std::min(k0 + k, im.c - 1) * ip, ip * sizeof(float));
        if (yolo_op_letterbox(src.data(), im.w, im.h, w, h, 1, dst.data(), g_device) != YOLO_OK) { fprintf(stderr, "darknet_hip: letterbox_image: %s\n", yolo_last_error(NULL)); return out; }
        for (int k = 0; k < 3 && k0 + k < im.c; ++k) memcpy(out.data + (size_t)(k0 + k) * op, &dst[k * op], op * sizeof(float));
    }
    return out;
}

void rgbgr_image(image im)                                                           /* DN/image.c:527 */
{
    if (!im.data || im.c < 3) return;
    const size_t n = (size_t)im.w * im.h;
    for (size_t i = 0; i < n; ++i) { const float t = im.data[i]; im.data[i] = im.data[i + 2 * n]; im.data[i + 2 * n] = t; }
}

// the bytes / 255. as darknet's planar image (DN/image.c:1458), resized by darknet's resize_image on the device when a size is given (DN/image.c:1475-1479)
static image planar_image(const unsigned char *raw, int iw, int ih, int ch, int w, int h)
{
    image im = make_image(iw, ih, 3);
    const size_t n = (size_t)iw * ih;
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < n; ++i) im.data[k * n + i] = (float)raw[i * ch + (ch == 3 ? k : 0)] / 255.;       /* DN/image.c:1458 */
    if (h && w && (h != im.h || w != im.w)) {
        image r = make_image(w, h, 3);
        if (yolo_op_letterbox(im.data, im.w, im.h, w, h, 0, r.data, g_device) != YOLO_OK) fprintf(stderr, "darknet_hip: resize: %s\n", yolo_last_error(NULL));
        free_image(im); im = r;
    }
    return im;
}

// DN/image.c:1442-1485 (load_image_stb + optional resize_image).  JPEG files of the kinds yolo_jpeg_to_rgb_host serves (bit-equal to the reference's stb decode),
// binary PPM (P6) and PGM (P5) of 8 bits per sample.  Anything else -- PNG, the refused JPEG kinds -- prints why and returns the empty image.
image load_image_color(char *filename, int w, int h)
{
    image bad = {0, 0, 0, nullptr};
    FILE *f = filename ? fopen(filename, "rb") : nullptr;
    if (!f) { fprintf(stderr, "darknet_hip: cannot load image \"%s\"\n", filename ? filename : "(null)"); return bad; }
    unsigned char soi[2] = {0, 0};
    const bool jpeg = fread(soi, 1, 2, f) == 2 && soi[0] == 0xff && soi[1] == 0xd8;
    rewind(f);
    if (jpeg) {
        std::vector<unsigned char> file;
        unsigned char chunk[65536];
        for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + got);
        fclose(f);
        struct yolo_jpeg_info info;
        if (yolo_jpeg_info(file.data(), file.size(), &info) != YOLO_OK) { fprintf(stderr, "darknet_hip: \"%s\": %s\n", filename, yolo_last_error(NULL)); return bad; }
        std::vector<unsigned char> rgb((size_t)info.h * info.w * 3);
        if (yolo_jpeg_to_rgb_host(file.data(), file.size(), rgb.data(), rgb.size()) != YOLO_OK) { fprintf(stderr, "darknet_hip: \"%s\": %s\n", filename, yolo_last_error(NULL)); return bad; }
        return planar_image(rgb.data(), info.w, info.h, 3, w, h);
    }
    auto token = [&](std::string &t) {
        t.clear(); int ch;
        for (;;) {
            ch = fgetc(f);
            if (ch == '#') { while ((ch = fgetc(f)) != EOF && ch != '\n') {} continue; }
            if (ch == EOF || !isspace(ch)) break;
        }
        while (ch != EOF && !isspace(ch)) { t.push_back((char)ch); ch = fgetc(f); }
        return !t.empty();
    };
    std::string magic, sw, sh, smax;
    if (!token(magic) || (magic != "P6" && magic != "P5") || !token(sw) || !token(sh) || !token(smax) || atoi(smax.c_str()) != 255) {
        fclose(f); fprintf(stderr, "darknet_hip: \"%s\" is neither a JPEG file nor an 8-bit binary PPM/PGM (PNG decoding is outside the inference path: convert the image first)\n", filename); return bad;
    }
    const int iw = atoi(sw.c_str()), ih = atoi(sh.c_str()), ch = magic == "P6" ? 3 : 1;
    if (iw < 1 || ih < 1 || (long)iw * ih > (1L << 28)) { fclose(f); return bad; }
    std::vector<unsigned char> raw((size_t)iw * ih * ch);
    const bool ok = fread(raw.data(), 1, raw.size(), f) == raw.size();
    fclose(f);
    if (!ok) { fprintf(stderr, "darknet_hip: short read on \"%s\"\n", filename); return bad; }
    return planar_image(raw.data(), iw, ih, ch, w, h);
}

// DN/option_list.c:35-50 + get_labels DN/data.c:618: `classes = N`, `names = path` (or `labels = path`); one class name per line
metadata get_metadata(char *file)
{
    metadata m = {0, nullptr};
    std::string text;
    if (!read_text(file, text)) { fprintf(stderr, "darknet_hip: couldn't open file: %s\n", file ? file : "(null)"); return m; }
    std::string names_path; int classes = 2;
    size_t pos = 0;
    while (pos < text.size()) {
        size_t e = text.find('\n', pos); if (e == std::string::npos) e = text.size();
        std::string line = trim(text.substr(pos, e - pos)); pos = e + 1;
        if (line.empty() || line[0] == '#' || line[0] == ';') continue;
        const size_t eq = line.find('='); if (eq == std::string::npos) continue;
        const std::string k = trim(line.substr(0, eq)), v = trim(line.substr(eq + 1));
        if (k == "classes") classes = atoi(v.c_str());
        else if (k == "names" || (k == "labels" && names_path.empty())) names_path = v;
    }
    m.classes = classes;
    if (names_path.empty()) { fprintf(stderr, "No names or labels found\n"); return m; }
    std::string list;
    if (!read_text(names_path.c_str(), list)) { fprintf(stderr, "darknet_hip: couldn't open file: %s\n", names_path.c_str()); return m; }
    std::vector<std::string> names;
    pos = 0;
    while (pos < list.size()) {
        size_t e = list.find('\n', pos); if (e == std::string::npos) e = list.size();
        std::string line = list.substr(pos, e - pos); pos = e + 1;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty() || pos < list.size()) names.push_back(line);
    }
    m.names = (char **)calloc(names.size() ? names.size() : 1, sizeof(char *));
    for (size_t i = 0; i < names.size(); ++i) m.names[i] = strdup(names[i].c_str());
    return m;
}

}  // extern "C"
