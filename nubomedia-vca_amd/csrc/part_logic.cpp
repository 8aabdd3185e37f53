// part_logic.cpp -- the per-frame state machine of NuboEyeDetector / NuboNoseDetector / NuboMouthDetector / NuboEarDetector:
// host glue of kms_{eye,nose,mouth,ear}_detect_process_frame (EYE/kmseyedetect.cpp:915-1064, NOSE/kmsnosedetect.cpp:792-868,
// MOUTH/kmsmouthdetect.cpp:798-873, EAR/kmseardetect.cpp:644-729,767-812) without its cv:: calls.  The conf_images scales,
// __receive_event and the frame gate, the face-to-ROI geometry, find_ears around its searches, the merge calls, the eye hysteresis
// and the roll-back of all of it are O(#faces) integer and float arithmetic on box lists: pure host code, no HIP header, built and
// driven on the CPU under the sanitizers as well (tests/san/parts_driver.cpp).  Every cv:: call in between (cvtColor, equalizeHist,
// resize, flip, detectMultiScale) belongs to the caller: the gate says which images and which face pass a frame needs, part_rois
// which searches, part_finish takes what they found.  The reference's quirks are kept on purpose ((float)W / (float)W, the
// `int scale` truncation of the merge helpers, one no-detection counter for both ears).
// std::vector idioms of the reference that rely on libstdc++ behaviour (erase through a reverse iterator, erase(end()-i) inside a
// counting loop) are written out as the index operations they perform (host_logic.cpp).
#include "part_logic.h"
#include <algorithm>

namespace nvca {

bool part_scales(const nvca_part_params &p, int W, int H, PartScales &out)
{
    const int kind = p.kind;
    // conf_images: float arithmetic (EYE/kmseyedetect.cpp:331-339 and siblings)
    const float o2f = (kind != NVCA_PART_EAR && p.detect_event) ? ((float)W) / ((float)W) : ((float)W) / ((float)160);
    const float x2o = ((float)W) / ((float)p.width_to_process);
    const float f2x = ((float)o2f) / ((float)x2o);
    out.o2f = o2f; out.x2o = x2o; out.f2x = f2x;
    out.fw = cv_round(W / out.o2f); out.fh = cv_round(H / out.o2f);
    out.pw = cv_round(W / out.x2o); out.ph = cv_round(H / out.x2o);
    return !(out.fw <= 0 || out.fh <= 0 || out.pw <= 0 || out.ph <= 0);
}

const FacePassRule &face_pass_rule(int pass)
{
    static const FacePassRule rules[3] = {
        {3, 0, 30, 30, false, false},                                // kPassEye: plain scan, EYE :958-960
        {2, NVCA_HAAR_SCALE_IMAGE, 3, 3, false, false},              // kPassNoseMouth: NOSE :843-846, MOUTH :845-848
        {2, NVCA_HAAR_SCALE_IMAGE, 3, 3, true, true},                // kPassEar: EAR :656-659, over the image and its mirror image (:796-803)
    };
    return rules[pass];
}

PartFrame part_gate(PartState &st, const nvca_part_params &p)
{
    PartFrame fr;
    const int kind = p.kind;
    bool received = true;
    if (kind != NVCA_PART_EAR) {                                            // __receive_event
        if (p.detect_event) {
            received = false;
            if (!st.queue.empty()) {
                st.faces = st.queue.front(); st.queue.pop_front();
                fr.popped = true;
                received = true;
                st.num_frames_to_process = 10 / (5 - p.process_x_every_4);
            }
        }
        if (!received && st.num_frames_to_process <= 0) fr.early_return = true;
    }
    if (fr.early_return) return fr;
    if (4 == st.num_frame) st.num_frame = 0;                                // GOP (the reference resets at the end of the frame before: nothing reads the counter in between)
    st.num_frame++;
    const int px = p.process_x_every_4;
    fr.run = (2 == px && (1 == st.num_frame % 2)) || ((2 != px) && (st.num_frame <= px));
    if (!fr.run) return fr;
    st.num_frames_to_process--;
    // the images this frame is worked on.  EYE :948-950: cvtColor + equalizeHist of the whole frame, then the resizes
    fr.eye_chain = kind == NVCA_PART_EYE;
    fr.face_image = kind == NVCA_PART_EAR || 0 == p.detect_event;
    fr.face_post_eq = kind != NVCA_PART_EYE;
    fr.mirror = kind == NVCA_PART_EAR;                                      // EAR :800
    if (fr.face_image) {
        fr.pass = kind == NVCA_PART_EYE ? kPassEye : (kind == NVCA_PART_EAR ? kPassEar : kPassNoseMouth);
        fr.pass_sf = 1 + p.scale_factor_pct * 1.0 / 100;
    }
    if (fr.pass == kPassNone) fr.faces = st.faces;
    return fr;
}

namespace {
PartSearch make_search(const PartScales &sc, const nvca_rect &roi, int cascade, int side, double sf, int mn, int flags, int minw, int minh)
{
    PartSearch s;
    s.roi = roi; s.cascade = cascade; s.side = side; s.sf = sf; s.min_neighbors = mn; s.flags = flags; s.minw = minw; s.minh = minh;
    const int cols = sc.pw, rows = sc.ph;
    s.valid = !(roi.x < 0 || roi.y < 0 || roi.w <= 0 || roi.h <= 0 || roi.x + roi.w > cols || roi.y + roi.h > rows);
    return s;
}
RectV capped(const RectV *v)
{
    if (!v) return RectV();
    return RectV(v->begin(), v->begin() + std::min<size_t>(v->size(), 256));
}

// kms_ear_detect_find_ears EAR/kmseardetect.cpp:644-729, in two halves around the ear searches.
// `profile_faces`: the profile-face pass on this side's image (the image itself / its mirror), :656-659.
// First half: the bookkeeping the reference does before it searches, and one FIND_BIGGEST search per profile face.
void find_ears_begin(PartState &st, const PartScales &sc, const RectV &profile_faces, int side, std::vector<PartSearch> &out)
{
    const int fcols = sc.fw, ecols = sc.pw;
    const double scale_f2e = sc.f2x;
    st.faces.assign(profile_faces.begin(), profile_faces.begin() + std::min<size_t>(profile_faces.size(), 256));
    if (st.faces.empty()) return;
    RectV &ears = side == 0 ? st.la : st.lb;
    if (!ears.empty()) ears.clear();
    else if (st.no_det_a < 4) st.no_det_a += 1;            // MAX_NUM_FPS_WITH_NO_DETECTION 4, one counter for both sides
    else { st.no_det_a = 0; ears.clear(); }
    for (nvca_rect &r : st.faces) {
        const int top_height = cv_round((float)r.h * 20 / 100), down_height = cv_round((float)r.h * 20 / 100);
        if (side == 0) {
            r.y = (int)((r.y + top_height) * scale_f2e);
            r.x = (int)((r.x + (r.w / 2)) * scale_f2e);
            r.h = (int)((r.h - down_height) * scale_f2e);
            r.w = (int)((r.w / 2) * scale_f2e + 50);        // EXTRA_ROI
            if (r.x + r.w > ecols) r.w = ecols - r.x - 1;
        } else {
            r.y = (int)((r.y + top_height) * scale_f2e);
            r.x = (int)((fcols - r.x - r.w) * scale_f2e - 50);
            r.h = (int)((r.h - down_height) * scale_f2e);
            r.w = (int)((r.w / 2) * scale_f2e);
            if (r.x < 0) r.x = 0;
        }
        out.push_back(make_search(sc, r, side, side, 1.1, 3, NVCA_HAAR_FIND_BIGGEST_OBJECT, 1, 1));
    }
}
// second half: the ears found in one profile face's region
void find_ears_end(PartState &st, const PartScales &sc, const PartSearch &search, const RectV *found)
{
    RectV &ears = search.side == 0 ? st.la : st.lb;
    const nvca_rect &r = search.roi;
    for (const nvca_rect &e : capped(found)) {
        nvca_rect o;
        o.x = cv_round((r.x + e.x) * sc.x2o); o.y = cv_round((r.y + e.y) * sc.x2o);
        o.w = (int)((e.w - 1) * sc.x2o); o.h = (int)((e.h - 1) * sc.x2o);
        ears.push_back(o);
    }
}
} // namespace

void part_rois(PartState &st, const nvca_part_params &p, const PartScales &sc, const PartFrame &pf, const RectV *faces, const RectV *faces_mirror,
               std::vector<PartSearch> &out)
{
    const int kind = p.kind;
    if (kind == NVCA_PART_EAR) {              // both sides' first halves before either side's results are appended (part_finish)
        static const RectV none;
        find_ears_begin(st, sc, faces ? *faces : none, 0, out);
        find_ears_begin(st, sc, faces_mirror ? *faces_mirror : none, 1, out);
        return;
    }
    if (faces) st.faces.assign(faces->begin(), faces->begin() + std::min<size_t>(faces->size(), 256));
    const double scale_f2x = sc.f2x;
    const RectV &faces_now = faces ? st.faces : pf.faces;
    for (const nvca_rect &r : faces_now) {
        if (kind == NVCA_PART_EYE) {
            nvca_rect ra, fr, fl;
            ra.x = (int)(r.x * scale_f2x); ra.y = (int)(r.y * scale_f2x); ra.w = (int)(r.w * scale_f2x); ra.h = (int)(r.h * scale_f2x);
            const int down_height = cv_round((float)ra.h * 40 / 100), top_height = cv_round((float)ra.h * 25 / 100);
            fr.x = ra.x; fr.y = ra.y + top_height; fr.h = ra.h - top_height - down_height; fr.w = ra.w / 2;
            fl.x = ra.x + ra.w / 2; fl.y = ra.y + top_height; fl.h = ra.h - top_height - down_height; fl.w = ra.w / 2;
            out.push_back(make_search(sc, fr, 0, 0, 1.1, 2, NVCA_HAAR_SCALE_IMAGE, 20, 20));
            out.push_back(make_search(sc, fl, 1, 1, 1.1, 2, NVCA_HAAR_SCALE_IMAGE, 20, 20));
        } else {
            nvca_rect ra;
            if (kind == NVCA_PART_NOSE) {                   // NOSE :858-868
                const int top = cv_round((float)r.h * 25 / 100), down = cv_round((float)r.h * 10 / 100);
                const int side = cv_round((float)r.w * 25 / 100);
                ra.y = (int)((r.y + top) * scale_f2x); ra.x = (int)((r.x + side) * scale_f2x);
                ra.h = (int)((r.h - down - top) * scale_f2x); ra.w = (int)((r.w - side) * scale_f2x);
            } else {                                        // MOUTH :859-865
                const int half = cv_round((float)r.h / 1.8);
                ra.y = (int)((r.y + half) * scale_f2x); ra.x = (int)(r.x * scale_f2x);
                ra.h = (int)(half * scale_f2x); ra.w = (int)(r.w * scale_f2x);
            }
            out.push_back(make_search(sc, ra, 0, 0, 1.1, 3, NVCA_HAAR_FIND_BIGGEST_OBJECT, 1, 1));
        }
    }
}

void part_finish(PartState &st, const nvca_part_params &p, const PartScales &sc, const PartFrame &pf, const std::vector<PartSearch> &searches,
                 const std::vector<const RectV *> &results)
{
    const int kind = p.kind;
    if (pf.early_return) return;
    RectV res_a, res_b;
    if (pf.run) {
        const int iscale = (int)sc.x2o;                      // the merge helpers take `int scale`
        if (kind == NVCA_PART_EAR) {
            for (size_t k = 0; k < searches.size(); k++) find_ears_end(st, sc, searches[k], results[k]);      // side 0's faces, then side 1's
        } else if (kind == NVCA_PART_EYE) {
            for (size_t k = 0; k + 1 < searches.size(); k += 2) {
                const nvca_rect &fr = searches[k].roi, &fl = searches[k + 1].roi;
                RectV eye_r = capped(results[k]), eye_l = capped(results[k + 1]), aux;
                to_global(eye_r, fr, iscale); to_global(eye_l, fl, iscale);
                if (!eye_r.empty()) {
                    merge_eyes_current(fr, eye_r, eye_r, iscale, false);
                    merge_eyes_consecutive(eye_r, st.la, aux);
                    res_a.insert(res_a.end(), aux.begin(), aux.end());
                }
                if (!eye_l.empty()) {
                    merge_eyes_current(fl, res_a, eye_l, iscale, true);
                    merge_eyes_consecutive(eye_l, st.lb, aux);
                    res_b.insert(res_b.end(), aux.begin(), aux.end());
                }
            }
        } else {
            const int dis = kind == NVCA_PART_NOSE ? 6 : 4;
            for (size_t k = 0; k < searches.size(); k++) {
                RectV cn = capped(results[k]), aux;
                if (!cn.empty()) {
                    merge_consecutive_nm(cn, st.la, searches[k].roi, iscale, dis, aux);
                    res_a.insert(res_a.end(), aux.begin(), aux.end());
                }
            }
        }
        if (kind == NVCA_PART_EYE) {                                // per-side hysteresis EYE :1034-1064
            if (res_a.empty()) { if (st.no_det_a < 1) st.no_det_a += 1; else { st.no_det_a = 0; st.la.clear(); } }
            else { st.no_det_a = 0; st.la = res_a; }
            if (res_b.empty()) { if (st.no_det_b < 1) st.no_det_b += 1; else { st.no_det_b = 0; st.lb.clear(); } }
            else { st.no_det_b = 0; st.lb = res_b; }
        }
    }
    if (kind == NVCA_PART_NOSE || kind == NVCA_PART_MOUTH) st.la = res_a;   // rebuilt on every call that gets here
}

PartSnap part_snapshot(const PartState &st)
{
    PartSnap g;
    g.faces = st.faces; g.la = st.la; g.lb = st.lb;
    g.num_frame = st.num_frame; g.to_process = st.num_frames_to_process; g.no_a = st.no_det_a; g.no_b = st.no_det_b;
    return g;
}
void part_restore(PartState &st, PartSnap &g)
{
    st.faces.swap(g.faces); st.la.swap(g.la); st.lb.swap(g.lb);
    st.num_frame = g.num_frame; st.num_frames_to_process = g.to_process; st.no_det_a = g.no_a; st.no_det_b = g.no_b;
    if (g.popped) st.queue.push_front(std::move(g.front));
}

} // namespace nvca
