// cascade_xml.cpp -- reader of OpenCV's cascade XML: old-format Haar files and new-format LBP / HAAR files (further down).  The old
// format (type_id="opencv-haar-classifier") is the format of every cascade file the reference loads: FACE/kmsfacedetect.cpp:40,162-177, EYE/kmseyedetect.cpp:27-29,
// NOSE/kmsnosedetect.cpp:31-32, MOUTH/kmsmouthdetect.cpp:37-38, EAR/kmseardetect.cpp:29-31.
// Mirrors what OpenCV 2.4's icvReadHaarClassifier stores: numbers are parsed as
// double and kept as float; a *_val leaf becomes alpha[last++] with child index -last.
#include "cascade_model.h"
#include <memory>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <cfloat>
#include <cerrno>
#include <climits>

namespace nvca {
namespace {

struct XNode {
    std::string name, type_id, text;
    std::vector<std::unique_ptr<XNode>> kids;
    const XNode *child(const char *n) const {
        for (auto &k : kids) if (k->name == n) return k.get();
        return nullptr;
    }
};

struct XParser {
    const char *p, *end; std::string err;
    bool fail(const std::string &m) { if (err.empty()) err = m; return false; }
    void skip_ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) ++p; }
    bool starts(const char *s) { size_t n = strlen(s); return (size_t)(end - p) >= n && !memcmp(p, s, n); }
    bool skip_misc() {           // comments, PIs, doctype
        for (;;) {
            skip_ws();
            if (starts("<!--")) { const char *e = (const char *)memmem(p, end - p, "-->", 3); if (!e) return fail("unterminated comment"); p = e + 3; }
            else if (starts("<?")) { const char *e = (const char *)memmem(p, end - p, "?>", 2); if (!e) return fail("unterminated PI"); p = e + 2; }
            else if (starts("<!")) { const char *e = (const char *)memchr(p, '>', end - p); if (!e) return fail("unterminated decl"); p = e + 1; }
            else return true;
        }
    }
    bool parse_elem(XNode &n, int depth) {
        if (depth > 64) return fail("XML too deep");
        if (p >= end || *p != '<') return fail("expected '<'");
        ++p;
        const char *s = p;
        while (p < end && *p != ' ' && *p != '>' && *p != '/' && *p != '\n' && *p != '\t' && *p != '\r') ++p;
        n.name.assign(s, p);
        if (n.name.empty()) return fail("empty tag name");
        // attributes
        for (;;) {
            skip_ws();
            if (p >= end) return fail("unterminated tag");
            if (*p == '/') { if (p + 1 < end && p[1] == '>') { p += 2; return true; } return fail("bad '/'"); }
            if (*p == '>') { ++p; break; }
            const char *as = p;
            while (p < end && *p != '=' && *p != '>' && *p != ' ') ++p;
            std::string an(as, p);
            skip_ws();
            if (p >= end || *p != '=') return fail("attribute without value");
            ++p; skip_ws();
            if (p >= end || (*p != '"' && *p != '\'')) return fail("attribute value not quoted");
            char q = *p++;
            const char *vs = p;
            while (p < end && *p != q) ++p;
            if (p >= end) return fail("unterminated attribute");
            if (an == "type_id") n.type_id.assign(vs, p);
            ++p;
        }
        // content
        for (;;) {
            const char *ts = p;
            while (p < end && *p != '<') ++p;
            n.text.append(ts, p);
            if (p >= end) return fail("unterminated element <" + n.name + ">");
            if (starts("<!--")) { const char *e = (const char *)memmem(p, end - p, "-->", 3); if (!e) return fail("unterminated comment"); p = e + 3; continue; }
            if (starts("</")) {
                p += 2;
                const char *cs = p;
                while (p < end && *p != '>') ++p;
                if (p >= end) return fail("unterminated close tag");
                std::string cn(cs, p);
                while (!cn.empty() && (cn.back() == ' ' || cn.back() == '\n')) cn.pop_back();
                ++p;
                if (cn != n.name) return fail("mismatched </" + cn + "> for <" + n.name + ">");
                return true;
            }
            std::unique_ptr<XNode> k(new XNode());
            if (!parse_elem(*k, depth + 1)) return false;
            n.kids.push_back(std::move(k));
        }
    }
};

bool to_double(const std::string &s, double &v) {
    const char *b = s.c_str(); char *e = nullptr;
    v = strtod(b, &e);
    if (e == b) return false;
    while (*e == ' ' || *e == '\n' || *e == '\r' || *e == '\t') ++e;
    return *e == 0;
}
bool to_int(const std::string &s, int &v) {
    const char *b = s.c_str(); char *e = nullptr;
    long l = strtol(b, &e, 10);
    if (e == b) return false;
    while (*e == ' ' || *e == '\n' || *e == '\r' || *e == '\t') ++e;
    if (*e) return false;
    v = (int)l; return true;
}

int parse_root(const char *text, size_t len, XNode &root, std::string &err)
{
    XParser xp{text, text + len, {}};
    if (!xp.skip_misc()) { err = xp.err; return NVCA_ERR_PARSE; }
    if (!xp.parse_elem(root, 0)) { err = xp.err; return NVCA_ERR_PARSE; }
    if (root.name != "opencv_storage") { err = "root element is not <opencv_storage>"; return NVCA_ERR_PARSE; }
    return NVCA_OK;
}

// the old-format branch (icvReadHaarClassifier)
int parse_haar(const XNode &root, Cascade &out, std::string &err)
{
    const XNode *cn = nullptr;
    for (auto &k : root.kids) if (k->type_id == "opencv-haar-classifier") { cn = k.get(); break; }
    if (!cn) { err = "no opencv-haar-classifier node (new-format cascades are not Haar old-format)"; return NVCA_ERR_PARSE; }

    const XNode *size = cn->child("size"), *stages = cn->child("stages");
    if (!size || !stages) { err = "missing <size> or <stages>"; return NVCA_ERR_PARSE; }
    if (sscanf(size->text.c_str(), "%d %d", &out.ow, &out.oh) != 2 || out.ow <= 2 || out.oh <= 2 || out.ow > 1024 || out.oh > 1024) {
        err = "bad <size>"; return NVCA_ERR_PARSE;             // stock cascades are 18..45 pixels a side; the bound keeps every later sum in range
    }
    out.stages.clear(); out.cls.clear(); out.nodes.clear(); out.alpha.clear();
    out.stump_based = true; out.has_tilted = false;
    int si = 0;
    for (auto &st : stages->kids) {
        const XNode *trees = st->child("trees"), *sthr = st->child("stage_threshold");
        const XNode *par = st->child("parent"), *nxt = st->child("next");
        if (!trees || !sthr || !par || !nxt) { err = "stage without trees/stage_threshold/parent/next"; return NVCA_ERR_PARSE; }
        double d; int parent, next;
        if (!to_double(sthr->text, d) || !to_int(par->text, parent) || !to_int(nxt->text, next)) { err = "bad stage scalar"; return NVCA_ERR_PARSE; }
        if (parent != si - 1 || next != -1) { err = "tree-structured stage graph is not supported"; return NVCA_ERR_UNSUPPORTED; }
        HaarStage hs; hs.first_cls = (int)out.cls.size(); hs.ncls = (int)trees->kids.size(); hs.threshold = (float)d;
        if (hs.ncls <= 0) { err = "empty stage"; return NVCA_ERR_PARSE; }
        for (auto &tree : trees->kids) {
            HaarClassifier hc; hc.first_node = (int)out.nodes.size(); hc.nnodes = (int)tree->kids.size();
            hc.first_alpha = (int)out.alpha.size();
            if (hc.nnodes <= 0) { err = "empty tree"; return NVCA_ERR_PARSE; }
            if (hc.nnodes != 1) out.stump_based = false;
            int last = 0;
            for (auto &nd : tree->kids) {
                HaarNode hn; memset(&hn, 0, sizeof(hn));
                const XNode *feat = nd->child("feature"), *thr = nd->child("threshold");
                if (!feat || !thr) { err = "node without feature/threshold"; return NVCA_ERR_PARSE; }
                const XNode *rects = feat->child("rects"), *tilted = feat->child("tilted");
                if (!rects || !tilted) { err = "feature without rects/tilted"; return NVCA_ERR_PARSE; }
                if (rects->kids.size() < 2 || rects->kids.size() > 3) { err = "feature must have 2 or 3 rects"; return NVCA_ERR_PARSE; }
                for (size_t k = 0; k < rects->kids.size(); k++) {
                    double wt; int r[4];
                    if (sscanf(rects->kids[k]->text.c_str(), "%d %d %d %d %lf", &r[0], &r[1], &r[2], &r[3], &wt) != 5) {
                        err = "bad rect"; return NVCA_ERR_PARSE;
                    }
                    for (int q = 0; q < 4; q++) hn.rect[k][q] = r[q];
                    hn.weight[k] = (float)wt;
                    if (r[0] < 0 || r[1] < 0 || r[2] <= 0 || r[3] <= 0 || r[0] > out.ow || r[2] > out.ow || r[1] > out.oh || r[3] > out.oh) { err = "rect outside the window"; return NVCA_ERR_PARSE; }
                }
                if (!to_int(tilted->text, hn.tilted)) { err = "bad <tilted>"; return NVCA_ERR_PARSE; }
                hn.tilted = hn.tilted != 0;
                for (size_t k = 0; k < rects->kids.size(); k++) {
                    const int *r = hn.rect[k];
                    // upright: x .. x+w, y .. y+h.  tilted: the rectangle rotated about (x, y) reads the tilted integral at
                    // columns x-h .. x+w and rows y .. y+w+h (cvSetImagesForHaarClassifierCascade)
                    const bool inside = !hn.tilted ? (r[0] + r[2] <= out.ow && r[1] + r[3] <= out.oh)
                                                   : (r[0] - r[3] >= 0 && r[0] + r[2] <= out.ow && r[1] + r[2] + r[3] <= out.oh);
                    if (!inside) { err = hn.tilted ? "tilted rect outside the window" : "rect outside the window"; return NVCA_ERR_PARSE; }
                }
                if (hn.tilted) out.has_tilted = true;
                // icvCreateHidHaarClassifierCascade: rect[2] is dropped when its weight or size is zero
                hn.nrect = (fabs(hn.weight[2]) < DBL_EPSILON || hn.rect[2][2] == 0 || hn.rect[2][3] == 0) ? 2 : 3;
                if (!to_double(thr->text, d)) { err = "bad <threshold>"; return NVCA_ERR_PARSE; }
                hn.threshold = (float)d;
                for (int side = 0; side < 2; side++) {
                    const XNode *cn2 = nd->child(side == 0 ? "left_node" : "right_node");
                    int &dst = side == 0 ? hn.left : hn.right;
                    if (cn2) {
                        // a child comes after its parent (haartraining writes trees in that order): every walk from the root ends,
                        // on the device too -- an index at or before the node itself would make the evaluator loop for ever
                        const int self = (int)out.nodes.size() - hc.first_node;
                        if (!to_int(cn2->text, dst) || dst <= self || dst >= hc.nnodes) { err = "bad child node index"; return NVCA_ERR_PARSE; }
                    } else {
                        const XNode *cv = nd->child(side == 0 ? "left_val" : "right_val");
                        if (!cv || !to_double(cv->text, d)) { err = "node without left/right value"; return NVCA_ERR_PARSE; }
                        dst = -last; out.alpha.push_back((float)d); last++;
                    }
                }
                out.nodes.push_back(hn);
            }
            if (last != hc.nnodes + 1) { err = "tree leaf count mismatch"; return NVCA_ERR_PARSE; }
            out.cls.push_back(hc);
        }
        out.stages.push_back(hs);
        si++;
    }
    if (out.stages.empty()) { err = "cascade has no stages"; return NVCA_ERR_PARSE; }
    return NVCA_OK;
}

// whitespace-separated decimal integers of a sequence node, each inside int32
bool to_ints(const std::string &s, std::vector<int> &v)
{
    v.clear();
    const char *p = s.c_str();
    for (;;) {
        while (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t') ++p;
        if (!*p) return true;
        char *e = nullptr;
        errno = 0;
        const long long l = strtoll(p, &e, 10);
        if (e == p || errno == ERANGE || l < INT32_MIN || l > INT32_MAX) return false;
        if (*e && *e != ' ' && *e != '\n' && *e != '\r' && *e != '\t') return false;
        v.push_back((int)l);
        p = e;
    }
}
bool to_doubles(const std::string &s, std::vector<double> &v)
{
    v.clear();
    const char *p = s.c_str();
    for (;;) {
        while (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t') ++p;
        if (!*p) return true;
        char *e = nullptr;
        const double d = strtod(p, &e);
        if (e == p || (*e && *e != ' ' && *e != '\n' && *e != '\r' && *e != '\t')) return false;
        v.push_back(d);
        p = e;
    }
}
bool one_int(const XNode *n, int &v) { std::vector<int> t; if (!n || !to_ints(n->text, t) || t.size() != 1) return false; v = t[0]; return true; }
std::string word(const XNode *n)
{
    std::string s = n ? n->text : std::string();
    while (!s.empty() && (s.back() == ' ' || s.back() == '\n' || s.back() == '\r' || s.back() == '\t')) s.pop_back();
    size_t b = 0;
    while (b < s.size() && (s[b] == ' ' || s[b] == '\n' || s[b] == '\r' || s[b] == '\t')) b++;
    return s.substr(b);
}

// the envelope of a new-format file (type_id="opencv-cascade-classifier"), as OpenCV 2.4 cascadedetect.cpp's CascadeClassifier::Data::read
// takes it, for either feature type: everything in front of the stages and the features.  maxCatCount is checked against the feature
// type here, before any feature or node is read: Data::read takes a stump's nodes for categorical ones whenever it is not 0.
struct NewEnvelope { const XNode *stages = nullptr, *features = nullptr; int ow = 0, oh = 0, nstages = 0; bool haar = false; };
int read_envelope(const XNode &cn, bool general, NewEnvelope &e, std::string &err)
{
    const XNode *stype = cn.child("stageType"), *ftype = cn.child("featureType"), *hn = cn.child("height"), *wn = cn.child("width");
    const XNode *sparams = cn.child("stageParams"), *fparams = cn.child("featureParams"), *snum = cn.child("stageNum");
    e.stages = cn.child("stages"); e.features = cn.child("features");
    if (!stype || !ftype || !hn || !wn || !sparams || !fparams || !snum || !e.stages || !e.features) {
        err = "new-format cascade without stageType/featureType/height/width/stageParams/featureParams/stageNum/stages/features"; return NVCA_ERR_PARSE;
    }
    if (word(stype) != "BOOST") { err = "stageType '" + word(stype) + "' is not supported (BOOST only)"; return NVCA_ERR_UNSUPPORTED; }
    const std::string ft = word(ftype);
    if (ft == "HOG") { err = "new-format HOG cascades are not supported (LBP and HAAR only)"; return NVCA_ERR_UNSUPPORTED; }
    if (ft != "LBP" && ft != "HAAR") { err = "unknown featureType"; return NVCA_ERR_PARSE; }
    e.haar = ft == "HAAR";
    if (!one_int(wn, e.ow) || !one_int(hn, e.oh) || e.ow <= 2 || e.oh <= 2 || e.ow > 1024 || e.oh > 1024) { err = "bad <width> / <height>"; return NVCA_ERR_PARSE; }
    int v = 0;
    if (!one_int(sparams->child("maxWeakCount"), v)) { err = "stageParams without maxWeakCount"; return NVCA_ERR_PARSE; }
    if (const XNode *md = sparams->child("maxDepth")) {
        if (!one_int(md, v)) { err = "bad <maxDepth>"; return NVCA_ERR_PARSE; }
        // (a general HAAR load reads the trees themselves: the header's maxDepth chooses nothing)
        if (v > 1 && !(general && e.haar)) { err ="weak classifiers with maxDepth > 1 (trees) are not supported"; return NVCA_ERR_UNSUPPORTED; }
    }
    if (!one_int(fparams->child("maxCatCount"), v)) { err = "featureParams without maxCatCount"; return NVCA_ERR_PARSE; }
    if (!e.haar && v != 256) { err = "maxCatCount is not 256 (LBP codes are 8 bits)"; return NVCA_ERR_UNSUPPORTED; }
    if (e.haar && v != 0) { err = "featureType HAAR with maxCatCount other than 0 (categorical nodes on Haar features) is not supported"; return NVCA_ERR_UNSUPPORTED; }
    if (!one_int(snum, e.nstages)) { err = "bad <stageNum>"; return NVCA_ERR_PARSE; }
    return NVCA_OK;
}

// featureType LBP: what Data::read and LBPEvaluator::read keep of an LBP cascade of stumps -- numbers parsed as double and kept as
// float, the stage threshold less 1e-5f (subtracted in float), a stump's subset as eight int32 words
int parse_lbp(const NewEnvelope &e, LbpCascade &out, std::string &err)
{
    const XNode *stages = e.stages, *features = e.features;
    const int nstages = e.nstages;
    out.ow = e.ow; out.oh = e.oh;

    out.features.clear(); out.weak.clear(); out.stages.clear();
    std::vector<int> iv; std::vector<double> dv;
    for (auto &f : features->kids) {
        const XNode *r = f->child("rect");
        if (!r || !to_ints(r->text, iv) || iv.size() != 4) { err = "feature without a <rect> of four integers"; return NVCA_ERR_PARSE; }
        // the 3 x 3 cells of w x h pixels lie inside the window: every corner the evaluator reads exists at every window position
        if (iv[0] < 0 || iv[1] < 0 || iv[2] <= 0 || iv[3] <= 0 || iv[2] > out.ow || iv[3] > out.oh ||
            (long long)iv[0] + 3ll * iv[2] > out.ow || (long long)iv[1] + 3ll * iv[3] > out.oh) { err = "feature rect outside the window"; return NVCA_ERR_PARSE; }
        out.features.push_back(LbpFeature{iv[0], iv[1], iv[2], iv[3]});
    }
    for (auto &st : stages->kids) {
        const XNode *sthr = st->child("stageThreshold"), *wk = st->child("weakClassifiers");
        int mwc = 0; double d;
        if (!sthr || !wk || !one_int(st->child("maxWeakCount"), mwc) || !to_double(sthr->text, d)) { err = "stage without maxWeakCount/stageThreshold/weakClassifiers"; return NVCA_ERR_PARSE; }
        LbpStage ls; ls.first = (int)out.weak.size(); ls.count = (int)wk->kids.size();
        ls.threshold = (float)d - 1e-5f;                  // THRESHOLD_EPS, subtracted in float
        if (ls.count <= 0) { err = "empty stage"; return NVCA_ERR_PARSE; }
        if (ls.count != mwc) { err = "stage's maxWeakCount disagrees with its weak classifiers"; return NVCA_ERR_PARSE; }
        for (auto &w : wk->kids) {
            const XNode *in = w->child("internalNodes"), *lv = w->child("leafValues");
            if (!in || !lv || !to_ints(in->text, iv) || !to_doubles(lv->text, dv)) { err = "weak classifier without internalNodes/leafValues"; return NVCA_ERR_PARSE; }
            if (iv.size() > 11 && iv.size() % 11 == 0 && dv.size() == iv.size() / 11 + 1) { err = "weak classifiers with more than one internal node (trees) are not supported"; return NVCA_ERR_UNSUPPORTED; }
            if (iv.size() != 11 || iv[0] != 0 || iv[1] != -1 || dv.size() != 2) { err = "internalNodes is not '0 -1 featureIdx' and 8 subset words with two leaf values"; return NVCA_ERR_PARSE; }
            if (iv[2] < 0 || (size_t)iv[2] >= out.features.size()) { err = "featureIdx outside the feature list"; return NVCA_ERR_PARSE; }
            LbpWeak lw; lw.feature = iv[2];
            for (int k = 0; k < 8; k++) lw.subset[k] = iv[3 + k];
            lw.leaf[0] = (float)dv[0]; lw.leaf[1] = (float)dv[1];
            out.weak.push_back(lw);
        }
        out.stages.push_back(ls);
    }
    if (out.stages.empty()) { err = "cascade has no stages"; return NVCA_ERR_PARSE; }
    if ((int)out.stages.size() != nstages) { err = "stageNum disagrees with the stages"; return NVCA_ERR_PARSE; }
    return NVCA_OK;
}

// featureType HAAR: what Data::read and HaarEvaluator::Feature::read keep of a cascade of stumps on upright features.
// A stump's internalNodes is "0 -1 featureIdx threshold" (the threshold a real), a feature one to three rects "x y w h weight".
// `general` (NVCA_LOAD_HAAR_GENERAL): a feature may be tilted -- all of its rects read the tilted integral, CV_TILTED_PTRS --
// and a weak classifier a tree: internalNodes holds "left right featureIdx threshold" per node, leafValues one value more than nodes.
// The checks are stricter than Data::read's, so that no walk loops or leaves its tables: a child node lies behind its parent and inside
// the tree, a leaf index inside [0, nodeCount].  A file that turns out to hold stumps "0 -1" on upright features alone leaves the very
// model the plain load leaves.
int parse_hnew(const NewEnvelope &e, bool general, HnewCascade &out, std::string &err)
{
    out = HnewCascade();
    out.ow = e.ow; out.oh = e.oh;
    std::vector<double> dv, lv;
    for (auto &f : e.features->kids) {
        const XNode *rects = f->child("rects"), *tilted = f->child("tilted");
        if (!rects) { err = "feature without <rects>"; return NVCA_ERR_PARSE; }
        int tl = 0;
        if (tilted && !one_int(tilted, tl)) { err = "bad <tilted>"; return NVCA_ERR_PARSE; }
        if (tl != 0 && !general) { err = "tilted features are not supported in a new-format HAAR cascade"; return NVCA_ERR_UNSUPPORTED; }
        if (rects->kids.empty() || rects->kids.size() > 3) { err = "feature must have 1 to 3 rects"; return NVCA_ERR_PARSE; }
        HnewFeature hf; memset(&hf, 0, sizeof(hf));
        hf.nrect = (int)rects->kids.size();
        for (int k = 0; k < hf.nrect; k++) {
            if (!to_doubles(rects->kids[(size_t)k]->text, dv) || dv.size() != 5) { err = "rect is not 'x y w h weight'"; return NVCA_ERR_PARSE; }
            for (int q = 0; q < 4; q++) {
                if (!(dv[(size_t)q] >= -4096. && dv[(size_t)q] <= 4096.) || dv[(size_t)q] != floor(dv[(size_t)q])) { err = "rect coordinate is not a small integer"; return NVCA_ERR_PARSE; }
                hf.rect[k][q] = (int)dv[(size_t)q];
            }
            const int *r = hf.rect[k];
            // every corner the evaluator reads exists at every window position
            if (r[0] < 0 || r[1] < 0 || r[2] <= 0 || r[3] <= 0 || r[0] + r[2] > e.ow || (tl == 0 && r[1] + r[3] > e.oh)) { err = "rect outside the window"; return NVCA_ERR_PARSE; }
            // tilted: the corners (x, y), (x - h, y + h), (x + w, y + w), (x + w - h, y + w + h) lie on the window's own lattice as well
            if (tl != 0 && (r[0] - r[3] < 0 || r[1] + r[2] + r[3] > e.oh)) { err = "tilted rect outside the window"; return NVCA_ERR_PARSE; }
            if (!std::isfinite(dv[4])) { err = "rect weight is not a finite number"; return NVCA_ERR_PARSE; }
            hf.weight[k] = (float)dv[4];
        }
        out.features.push_back(hf);
        if (general) { out.tilted.push_back(tl != 0 ? 1 : 0); if (tl != 0) out.has_tilted = true; }
    }
    bool stumps = true;          // (general) every weak classifier read so far is the stump "0 -1"
    for (auto &st : e.stages->kids) {
        const XNode *sthr = st->child("stageThreshold"), *wk = st->child("weakClassifiers");
        int mwc = 0; double d;
        if (!sthr || !wk || !one_int(st->child("maxWeakCount"), mwc) || !to_double(sthr->text, d)) { err = "stage without maxWeakCount/stageThreshold/weakClassifiers"; return NVCA_ERR_PARSE; }
        LbpStage ls; ls.first = (int)(general ? out.trees.size() : out.weak.size()); ls.count = (int)wk->kids.size();
        ls.threshold = (float)d - 1e-5f;                  // THRESHOLD_EPS, subtracted in float
        if (ls.count <= 0) { err = "empty stage"; return NVCA_ERR_PARSE; }
        if (ls.count != mwc) { err = "stage's maxWeakCount disagrees with its weak classifiers"; return NVCA_ERR_PARSE; }
        for (auto &w : wk->kids) {
            const XNode *in = w->child("internalNodes"), *lf = w->child("leafValues");
            if (!in || !lf || !to_doubles(in->text, dv) || !to_doubles(lf->text, lv)) { err = "weak classifier without internalNodes/leafValues"; return NVCA_ERR_PARSE; }
            if (general) {
                if (dv.empty() || dv.size() % 4 != 0) { err = "internalNodes is not 'left right featureIdx threshold' per node"; return NVCA_ERR_PARSE; }
                const size_t nn = dv.size() / 4;
                if (nn > (size_t)kHgenMaxNodes) { err = "weak classifiers with more than 15 internal nodes are not supported"; return NVCA_ERR_UNSUPPORTED; }
                if (lv.size() != nn + 1) { err = "leafValues does not hold one value more than internalNodes has nodes"; return NVCA_ERR_PARSE; }
                HgenTree t; t.first_node = (int)out.nodes.size(); t.nnodes = (int)nn; t.first_leaf = (int)out.leaves.size();
                for (size_t j = 0; j < nn; j++) {
                    const double *q = &dv[4 * j];
                    for (int side = 0; side < 2; side++) {
                        const double c = q[side];
                        if (!(c >= -(double)nn && c < (double)nn) || c != floor(c)) { err = c > 0. ? "child node index outside the tree" : "leaf index outside the leaf values"; return NVCA_ERR_PARSE; }
                        // every walk from the root ends, on the device too: an index at or before the node itself would make the evaluator loop
                        if (c > 0. && c <= (double)j) { err = "child node index does not lie behind its parent"; return NVCA_ERR_PARSE; }
                    }
                    if (!(q[2] >= 0. && q[2] < (double)out.features.size()) || q[2] != floor(q[2])) { err = "featureIdx outside the feature list"; return NVCA_ERR_PARSE; }
                    if (!std::isfinite(q[3])) { err = "threshold or leaf value is not a finite number"; return NVCA_ERR_PARSE; }
                    out.nodes.push_back(HgenNode{(int)q[0], (int)q[1], (int)q[2], (float)q[3]});
                }
                for (double v : lv) {
                    if (!std::isfinite(v)) { err = "threshold or leaf value is not a finite number"; return NVCA_ERR_PARSE; }
                    out.leaves.push_back((float)v);
                }
                if (nn != 1 || dv[0] != 0. || dv[1] != -1.) stumps = false;
                out.trees.push_back(t);
                continue;
            }
            if (dv.size() > 4 && dv.size() % 4 == 0 && lv.size() == dv.size() / 4 + 1) { err = "weak classifiers with more than one internal node (trees) are not supported"; return NVCA_ERR_UNSUPPORTED; }
            if (dv.size() != 4 || dv[0] != 0. || dv[1] != -1. || lv.size() != 2) { err = "internalNodes is not '0 -1 featureIdx threshold' with two leaf values"; return NVCA_ERR_PARSE; }
            if (!(dv[2] >= 0. && dv[2] < (double)out.features.size()) || dv[2] != floor(dv[2])) { err = "featureIdx outside the feature list"; return NVCA_ERR_PARSE; }
            if (!std::isfinite(dv[3]) || !std::isfinite(lv[0]) || !std::isfinite(lv[1])) { err = "threshold or leaf value is not a finite number"; return NVCA_ERR_PARSE; }
            HnewWeak hw; hw.feature = (int)dv[2]; hw.threshold = (float)dv[3]; hw.leaf[0] = (float)lv[0]; hw.leaf[1] = (float)lv[1];
            out.weak.push_back(hw);
        }
        out.stages.push_back(ls);
    }
    if (out.stages.empty()) { err = "cascade has no stages"; return NVCA_ERR_PARSE; }
    if ((int)out.stages.size() != e.nstages) { err = "stageNum disagrees with the stages"; return NVCA_ERR_PARSE; }
    if (general && stumps && !out.has_tilted) {          // nothing the stump evaluator cannot take: the plain load's model
        for (const HgenTree &t : out.trees) {
            const HgenNode &n = out.nodes[(size_t)t.first_node];
            out.weak.push_back(HnewWeak{n.feature, n.threshold, {out.leaves[(size_t)t.first_leaf], out.leaves[(size_t)t.first_leaf + 1]}});
        }
        out.trees.clear(); out.nodes.clear(); out.leaves.clear(); out.tilted.clear();
    } else if (general) out.general = true;
    return NVCA_OK;
}

} // namespace

int parse_cascade_xml(const char *text, size_t len, Cascade &out, std::string &err)
{
    XNode root;
    if (int rc = parse_root(text, len, root, err)) return rc;
    return parse_haar(root, out, err);
}

// cv::CascadeClassifier::load's dispatch (cascadedetect.cpp: Data::read, else the old-format cvLoad): the type_id of the first
// child of <opencv_storage> decides the branch
int parse_cascade_file(const char *text, size_t len, CascadeFile &out, std::string &err) { return parse_cascade_file(text, len, 0u, out, err); }

int parse_cascade_file(const char *text, size_t len, unsigned flags, CascadeFile &out, std::string &err)
{
    const bool general = (flags & NVCA_LOAD_HAAR_GENERAL) != 0;
    XNode root;
    if (int rc = parse_root(text, len, root, err)) return rc;
    if (!root.kids.empty() && root.kids[0]->type_id == "opencv-cascade-classifier") {
        NewEnvelope e;
        out.format = NVCA_CASCADE_LBP;
        if (int rc = read_envelope(*root.kids[0], general, e, err)) return rc;
        out.format = e.haar ? NVCA_CASCADE_HAAR_NEW : NVCA_CASCADE_LBP;
        const int rc = e.haar ? parse_hnew(e, general, out.hnew, err) : parse_lbp(e, out.lbp, err);
        if (rc == NVCA_OK) { out.haar.ow = e.ow; out.haar.oh = e.oh; }
        return rc;
    }
    out.format = NVCA_CASCADE_HAAR;
    return parse_haar(root, out.haar, err);
}

} // namespace nvca
