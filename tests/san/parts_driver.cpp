// parts_driver.cpp -- the part detectors' per-frame logic (csrc/part_logic.cpp) on the CPU, under ASan + UBSan: built by
// tests/test_part_logic_cpu.py from part_logic.cpp, host_logic.cpp and cascade_xml.cpp, no HIP header anywhere, linked against the
// oracle library.  A stream's frame goes gate -> images -> face pass -> ROIs -> searches -> finish exactly as part_call.cpp drives it,
// with the oracle's primitives where the product uses the GPU -- the image chain and every search parameter are taken from what the
// logic returned.  Only the product sources are instrumented: the oracle is the checker (the test compares the lists printed here with
// those of its PartStream).
//
//   parts_driver <script>
// script lines:
//   S <id> <kind> <width_to_process> <process_x_every_4> <scale_factor_pct> <detect_event> <face.xml> <a.xml> <b.xml | -> <W> <H> <frames> <raw BGR file> <twin>
//   F <frame> <n> x y w h ...         faces pushed before that frame of the stream above (detect-event)
// twin = 1: a second stream of the same settings, which on frames 1, 2 and 4 first takes a snapshot, runs the gate and the ROI step
// and is restored, then runs the frame for real (a batched call that failed late); its lists are printed under <id>_twin.
#include "../../nubomedia-vca_amd/csrc/part_logic.h"
#include "../../nubomedia-vca_amd/csrc/cascade_model.h"
#include "../../oracle/nvca_oracle.h"
#include <cstdio>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>

using namespace nvca;

static int fail(const std::string &m) { fprintf(stderr, "parts_driver: %s\n", m.c_str()); return 1; }

// a cascade read by the product's loader, handed to the oracle as its flat description
struct Casc {
    Cascade c; orc_cascade o;
    std::vector<int> stage_ncls, cls_nnodes, rects, tilted, left, right;
    std::vector<float> stage_thr, rweights, node_thr, alpha;
    bool load(const std::string &path, std::string &err)
    {
        std::ifstream f(path, std::ios::binary);
        if (!f) { err = "cannot read " + path; return false; }
        std::stringstream ss; ss << f.rdbuf();
        const std::string xml = ss.str();
        if (parse_cascade_xml(xml.data(), xml.size(), c, err)) return false;
        for (const HaarStage &s : c.stages) { stage_ncls.push_back(s.ncls); stage_thr.push_back(s.threshold); }
        for (const HaarClassifier &hc : c.cls) {
            cls_nnodes.push_back(hc.nnodes);
            for (int k = 0; k < hc.nnodes; k++) {
                const HaarNode &n = c.nodes[hc.first_node + k];
                for (int r = 0; r < 3; r++) { for (int q = 0; q < 4; q++) rects.push_back(n.rect[r][q]); rweights.push_back(n.weight[r]); }
                tilted.push_back(n.tilted); node_thr.push_back(n.threshold); left.push_back(n.left); right.push_back(n.right);
            }
            for (int k = 0; k < hc.nnodes + 1; k++) alpha.push_back(c.alpha[hc.first_alpha + k]);
        }
        o.ow = c.ow; o.oh = c.oh;
        o.n_stages = (int)stage_ncls.size(); o.stage_ncls = stage_ncls.data(); o.stage_thr = stage_thr.data();
        o.n_cls = (int)cls_nnodes.size(); o.cls_nnodes = cls_nnodes.data();
        o.n_nodes = (int)tilted.size(); o.rects = rects.data(); o.rweights = rweights.data(); o.tilted = tilted.data();
        o.node_thr = node_thr.data(); o.left = left.data(); o.right = right.data(); o.alpha = alpha.data();
        return true;
    }
};

struct Stream { nvca_part_params p{0, 320, 4, 25, 0}; const Casc *face = nullptr, *a = nullptr, *b = nullptr; PartState st; };

static RectV detect(const Casc *c, const uint8_t *img, int w, int h, int stride, double sf, int mn, int flags, int minw, int minh, int maxw, int maxh)
{
    std::vector<orc_rect> buf(4096);
    const int n = orc_detect_multiscale(&c->o, img, w, h, stride, sf, mn, flags, minw, minh, maxw, maxh, ORC_SUM_F32PAIR, buf.data(), (int)buf.size(), nullptr);
    RectV out;
    for (int i = 0; i < n; i++) out.push_back(nvca_rect{buf[i].x, buf[i].y, buf[i].w, buf[i].h});
    return out;
}

// [equalizeHist](resize(gray)) as the device chain makes a working image
static std::vector<uint8_t> working_image(const std::vector<uint8_t> &gray, int W, int H, int dw, int dh, bool post_eq)
{
    std::vector<uint8_t> img((size_t)dw * dh);
    orc_resize_linear(gray.data(), W, H, W, 1, img.data(), dw, dh, dw);
    if (post_eq) orc_equalize_hist(img.data(), dw, dh, dw, img.data(), dw);
    return img;
}

// One frame of one stream.  dry: a call that fails after the gate and the ROI step -- nothing is searched, nothing finished.
static int run_frame(Stream &s, const uint8_t *bgr, int W, int H, bool dry, PartSnap *snap)
{
    PartScales sc;
    if (!part_scales(s.p, W, H, sc)) return fail("frame too small");
    const PartFrame fr = part_gate(s.st, s.p);
    if (fr.popped && snap) snap->note_popped(s.st);
    std::vector<PartSearch> searches;
    std::vector<RectV> found;
    if (fr.run) {
        std::vector<uint8_t> gray((size_t)W * H);
        orc_bgr2gray(bgr, W, H, W * 3, 3, gray.data(), W);
        if (fr.eye_chain) orc_equalize_hist(gray.data(), W, H, W, gray.data(), W);
        RectV faces, faces_mirror;
        if (fr.face_image) {
            const std::vector<uint8_t> small = working_image(gray, W, H, sc.fw, sc.fh, fr.face_post_eq);
            const FacePassRule &rule = face_pass_rule(fr.pass);
            const int maxw = rule.max_is_image ? sc.fw : 0, maxh = rule.max_is_image ? sc.fh : 0;
            faces = detect(s.face, small.data(), sc.fw, sc.fh, sc.fw, fr.pass_sf, rule.min_neighbors, rule.flags, rule.minw, rule.minh, maxw, maxh);
            if (fr.mirror != rule.mirrored) return fail("mirror image without a mirrored pass");
            if (fr.mirror) {
                std::vector<uint8_t> flip(small.size());
                orc_flip_h(small.data(), sc.fw, sc.fh, sc.fw, flip.data(), sc.fw);
                faces_mirror = detect(s.face, flip.data(), sc.fw, sc.fh, sc.fw, fr.pass_sf, rule.min_neighbors, rule.flags, rule.minw, rule.minh, maxw, maxh);
            }
        }
        const bool has_pass = fr.pass != kPassNone;
        part_rois(s.st, s.p, sc, fr, has_pass ? &faces : nullptr, fr.mirror ? &faces_mirror : nullptr, searches);
        if (dry) return 0;
        const std::vector<uint8_t> part = working_image(gray, W, H, sc.pw, sc.ph, true);
        for (const PartSearch &q : searches) {
            found.emplace_back();
            if (!q.valid) continue;
            const Casc *c = q.cascade ? s.b : s.a;
            if (!c) return fail("search on a cascade the stream does not have");
            if (q.roi.x < 0 || q.roi.y < 0 || q.roi.x + q.roi.w > sc.pw || q.roi.y + q.roi.h > sc.ph) return fail("valid search outside the part image");
            found.back() = detect(c, part.data() + (size_t)q.roi.y * sc.pw + q.roi.x, q.roi.w, q.roi.h, sc.pw, q.sf, q.min_neighbors, q.flags, q.minw, q.minh, 0, 0);
        }
    }
    if (dry) return 0;
    std::vector<const RectV *> results;
    for (size_t k = 0; k < searches.size(); k++) results.push_back(searches[k].valid ? &found[k] : nullptr);
    part_finish(s.st, s.p, sc, fr, searches, results);
    return 0;
}

static void print_lists(const std::string &id, int frame, const PartState &st)
{
    printf("{\"case\": \"%s\", \"frame\": %d", id.c_str(), frame);
    const RectV *lists[2] = {&st.la, &st.lb};
    for (int l = 0; l < 2; l++) {
        printf(", \"%s\": [", l ? "b" : "a");
        for (size_t k = 0; k < lists[l]->size(); k++) {
            const nvca_rect &r = (*lists[l])[k];
            printf("%s[%d, %d, %d, %d]", k ? ", " : "", r.x, r.y, r.w, r.h);
        }
        printf("]");
    }
    printf("}\n");
}

struct Case {
    std::string id, raw; Stream s; int W = 0, H = 0, frames = 0, twin = 0;
    std::map<int, RectV> pushes;
};

static int run_case(Case &c)
{
    std::ifstream f(c.raw, std::ios::binary);
    if (!f) return fail("cannot read " + c.raw);
    const size_t frame_bytes = (size_t)c.W * c.H * 3;
    std::vector<uint8_t> bgr(frame_bytes);
    Stream twin = c.s;
    for (int i = 0; i < c.frames; i++) {
        if (!f.read((char *)bgr.data(), (std::streamsize)frame_bytes)) return fail("short frame file " + c.raw);
        const auto push = c.pushes.find(i);
        if (push != c.pushes.end()) {
            c.s.st.push_faces(push->second.data(), (int)push->second.size());
            twin.st.push_faces(push->second.data(), (int)push->second.size());
        }
        if (run_frame(c.s, bgr.data(), c.W, c.H, false, nullptr)) return 1;
        print_lists(c.id, i, c.s.st);
        if (!c.twin) continue;
        if (i == 1 || i == 2 || i == 4) {
            PartSnap snap = part_snapshot(twin.st);
            if (run_frame(twin, bgr.data(), c.W, c.H, true, &snap)) return 1;
            part_restore(twin.st, snap);
        }
        if (run_frame(twin, bgr.data(), c.W, c.H, false, nullptr)) return 1;
        print_lists(c.id + "_twin", i, twin.st);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return fail("usage: parts_driver <script>");
    std::ifstream in(argv[1]);
    if (!in) return fail("cannot read the script");
    std::map<std::string, std::unique_ptr<Casc>> cascades;
    auto cascade = [&](const std::string &path) -> const Casc * {
        if (path == "-") return nullptr;
        std::unique_ptr<Casc> &slot = cascades[path];
        if (!slot) {
            slot.reset(new Casc());
            std::string err;
            if (!slot->load(path, err)) { fail(err); exit(1); }
        }
        return slot.get();
    };
    std::vector<Case> cases;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string tag;
        if (!(ls >> tag)) continue;
        if (tag == "S") {
            Case c; std::string face, a, b;
            if (!(ls >> c.id >> c.s.p.kind >> c.s.p.width_to_process >> c.s.p.process_x_every_4 >> c.s.p.scale_factor_pct >> c.s.p.detect_event >> face >> a >> b >>
                  c.W >> c.H >> c.frames >> c.raw >> c.twin)) return fail("bad S line: " + line);
            c.s.face = cascade(face); c.s.a = cascade(a); c.s.b = cascade(b);
            cases.push_back(std::move(c));
        } else if (tag == "F") {
            int frame = 0, n = 0;
            if (cases.empty() || !(ls >> frame >> n) || n < 0) return fail("bad F line: " + line);
            RectV v((size_t)n);
            for (nvca_rect &r : v) if (!(ls >> r.x >> r.y >> r.w >> r.h)) return fail("bad F line: " + line);
            cases.back().pushes[frame] = v;
        } else return fail("bad line: " + line);
    }
    for (Case &c : cases) if (run_case(c)) return 1;
    printf("{\"cases\": %zu}\n", cases.size());
    return 0;
}
