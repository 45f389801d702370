// Softmax trees on the host side of libyolo_hip.so: the reader of darknet's tree files, the device copy of a tree, and the entry
// points that exist because of trees (thresholds and modes, the geometry query, the `map` form of get_network_boxes, the two single
// operators).  The kernels are in tree_ops.hip.
//
// A tree file (DN/tree.c:83-139) has one `name parent` line per node.  A group is a maximal run of consecutive lines with the same
// parent; child[parent] is the index of that run, leaf[i] says nobody names i as parent.  The reference accepts any file; three of
// its silent assumptions are checked here because the arithmetic depends on them: a parent lies below its own index (the ascending
// product of hierarchy_predictions), the children of a node are ONE run (read_tree overwrites child[] otherwise and the first run
// becomes unreachable), and the file begins with a root (a first parent other than -1 makes group 0 empty).
#include "yolo_ctx.h"

namespace yolo_impl {

thread_local const std::vector<std::pair<std::string, std::string>> *g_tree_texts = nullptr;

static int tree_fail(std::string &err, const char *fmt, ...)
{
    char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    err = buf; return YOLO_ERR_INVALID;
}

int parse_tree(const std::string &text, Tree &t, std::string &err)
{
    t.text = text; t.n = 0; t.groups = 0;
    t.parent.clear(); t.child.clear(); t.goff.clear(); t.gsize.clear(); t.leaf.clear(); t.order.clear(); t.lvl.clear();
    std::vector<int> group;              // group of every node
    int last_parent = -1, line_no = 0;
    size_t pos = 0;
    while (pos < text.size()) {
        size_t e = text.find('\n', pos); if (e == std::string::npos) e = text.size();
        const std::string line = text.substr(pos, e - pos); pos = e + 1; ++line_no;
        char id[256]; int parent = -1;
        const int got = sscanf(line.c_str(), "%255s %d", id, &parent);          // the reference's own `%s %d`
        if (got < 1) return tree_fail(err, "tree line %d: no node name", line_no);
        const int i = t.n;
        if (i == 0 && parent != -1) return tree_fail(err, "tree line %d: the first node must be a root (parent -1), it names parent %d", line_no, parent);
        if (parent < -1 || parent >= i) return tree_fail(err, "tree line %d: parent %d is not below the node's own index %d", line_no, parent, i);
        if (i == 0 || parent != last_parent) {
            if (i > 0 && (parent < 0 || t.child[parent] >= 0))
                return tree_fail(err, "tree line %d: the children of %s are not one contiguous run", line_no, parent < 0 ? "the root" : ("node " + std::to_string(parent)).c_str());
            t.goff.push_back(i); t.gsize.push_back(0);
            if (parent >= 0) t.child[parent] = (int)t.goff.size() - 1;
            last_parent = parent;
        }
        t.parent.push_back(parent); t.child.push_back(-1); group.push_back((int)t.goff.size() - 1);
        ++t.gsize.back(); ++t.n;
    }
    if (t.n == 0) return tree_fail(err, "tree line 1: the file has no nodes");
    t.groups = (int)t.goff.size();
    t.leaf.assign(t.n, 1);
    for (int i = 0; i < t.n; ++i) if (t.parent[i] >= 0) t.leaf[t.parent[i]] = 0;
    // groups by depth: a group's parent node lies in an earlier group, so one ascending pass gives every depth
    std::vector<int> depth(t.groups, 0);
    int levels = 1;
    for (int g = 1; g < t.groups; ++g) { depth[g] = depth[group[t.parent[t.goff[g]]]] + 1; levels = std::max(levels, depth[g] + 1); }
    t.levels = levels; t.lvl.assign(levels + 1, 0);
    for (int g = 0; g < t.groups; ++g) ++t.lvl[depth[g] + 1];
    for (int l = 0; l < levels; ++l) t.lvl[l + 1] += t.lvl[l];
    t.order.resize(t.groups);
    { std::vector<int> at(t.lvl.begin(), t.lvl.end() - 1); for (int g = 0; g < t.groups; ++g) t.order[at[depth[g]]++] = g; }
    return YOLO_OK;
}

int load_tree(const std::string &path, Tree &t, std::string &err)
{
    t.path = path;
    if (g_tree_texts) for (auto &pt : *g_tree_texts) if (pt.first == path) return parse_tree(pt.second, t, err);
    FILE *f = fopen(path.c_str(), "rb");          // relative to the working directory, as darknet opens it
    if (!f) return tree_fail(err, "tree file '%s' cannot be opened", path.c_str());
    std::string text; char buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    fclose(f);
    const int r = parse_tree(text, t, err);
    if (r) err = "tree file '" + path + "': " + err;
    return r;
}

std::vector<int> pack_tree(const Tree &t, size_t at[7])
{
    std::vector<int> all;
    const std::vector<int> *src[7] = {&t.parent, &t.child, &t.goff, &t.gsize, &t.leaf, &t.order, &t.lvl};
    for (int k = 0; k < 7; ++k) { at[k] = all.size(); all.insert(all.end(), src[k]->begin(), src[k]->end()); }
    return all;
}

TreeDev tree_dev(const Tree &t, const int *d, const size_t at[7])
{
    return TreeDev{t.n, t.groups, t.levels, d + at[0], d + at[1], d + at[2], d + at[3], d + at[4], d + at[5], d + at[6]};
}

int upload_tree(yolo_ctx *c, Tree &t)
{
    size_t at[7];
    const std::vector<int> all = pack_tree(t, at);
    HIPCK(c, hipMalloc((void **)&t.d_all, all.size() * 4));
    HIPCK(c, hipMemcpyAsync(t.d_all, all.data(), all.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    t.dev = tree_dev(t, t.d_all, at);
    return YOLO_OK;
}

void free_tree(Tree &t) { if (t.d_all) hipFree(t.d_all); t.d_all = nullptr; }

int score_tree_rows(yolo_ctx *c, int n)
{
    const Tree &t = c->trees[c->layers[c->tree_head].tree];
    HIPCK(c, launch_tree_score_rows(c->d_det, (size_t)n * c->rows, c->attrs, t.dev, c->hier_thresh, c->d_scores, c->d_labels, c->stream));
    return YOLO_OK;
}

}  // namespace yolo_impl

extern "C" {

int yolo_set_hier_thresh(yolo_ctx *c, float hier_thresh)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!(hier_thresh == hier_thresh)) return fail(c, YOLO_ERR_INVALID, "yolo_set_hier_thresh: not a number");
    if (c->tree_head >= 0 && hier_thresh != c->hier_thresh) drop_graph(c);      // a captured detect step holds the old value
    c->hier_thresh = hier_thresh;
    return YOLO_OK;
}

int yolo_set_hierarchy_mode(yolo_ctx *c, int mode)
{
    if (!c) return YOLO_ERR_INVALID;
    if (mode < YOLO_HIER_CONDITIONAL || mode > YOLO_HIER_LEAVES) return fail(c, YOLO_ERR_INVALID, "yolo_set_hierarchy_mode: mode %d outside 0..2", mode);
    c->hierarchy_mode = mode;
    return YOLO_OK;
}

int yolo_tree_read(const char *path, int32_t *nodes, int32_t *groups, int32_t *parent, int32_t *child, int32_t *group_offset, int32_t *group_size,
                   int32_t *leaf, char *err, size_t err_len)
{
    Tree t; std::string e;
    const int r = load_tree(path ? path : "", t, e);
    if (r) { if (err && err_len) snprintf(err, err_len, "%s", e.c_str()); return r; }
    if (nodes) *nodes = t.n;
    if (groups) *groups = t.groups;
    if (parent) memcpy(parent, t.parent.data(), (size_t)t.n * 4);
    if (child) memcpy(child, t.child.data(), (size_t)t.n * 4);
    if (leaf) memcpy(leaf, t.leaf.data(), (size_t)t.n * 4);
    if (group_offset) memcpy(group_offset, t.goff.data(), (size_t)t.groups * 4);
    if (group_size) memcpy(group_size, t.gsize.data(), (size_t)t.groups * 4);
    return YOLO_OK;
}

int yolo_tree_geometry(const yolo_ctx *c, int32_t *nodes, int32_t *groups, int32_t *parent, int32_t *child, int32_t *group_offset, int32_t *group_size, int32_t *leaf)
{
    if (!c) return YOLO_ERR_INVALID;
    // the network's hierarchy: the [region] head's tree, or the tree of the last [softmax] layer that has one (DN/parser.c:798)
    int ti = c->tree_head >= 0 ? c->layers[c->tree_head].tree : -1;
    if (ti < 0) for (auto &L : c->layers) if (L.type == L_SOFTMAX && L.tree >= 0) ti = L.tree;
    if (nodes) *nodes = 0;
    if (groups) *groups = 0;
    if (ti < 0) return YOLO_OK;
    const Tree &t = c->trees[ti];
    if (nodes) *nodes = t.n;
    if (groups) *groups = t.groups;
    if (parent) memcpy(parent, t.parent.data(), (size_t)t.n * 4);
    if (child) memcpy(child, t.child.data(), (size_t)t.n * 4);
    if (leaf) memcpy(leaf, t.leaf.data(), (size_t)t.n * 4);
    if (group_offset) memcpy(group_offset, t.goff.data(), (size_t)t.groups * 4);
    if (group_size) memcpy(group_size, t.gsize.data(), (size_t)t.groups * 4);
    return YOLO_OK;
}

}  // extern "C"
