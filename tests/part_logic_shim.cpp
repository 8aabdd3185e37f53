// part_logic_shim.cpp -- test infrastructure: the part detectors' per-frame logic (csrc/part_logic.cpp, host_logic.cpp) behind a
// plain C interface, so that a Python harness can drive a stream's frame gate -> ROIs -> finish around a detector of its own choice
// (tests/lbp_part_cases.py: the numpy statement of the LBP scan, or the oracle's detectMultiScale).  Built by the tests as a plain
// shared library and loaded with ctypes; no HIP, no sanitizer.  One handle is one stream's state and the frame it is in.
#include "../nubomedia-vca_amd/csrc/part_logic.h"
#include <new>

using namespace nvca;

namespace {
struct Shim {
    nvca_part_params p{0, 320, 4, 25, 0};
    PartState st; PartScales sc; PartFrame fr;
    std::vector<PartSearch> searches;
};
RectV rects(const int *r, int n) { RectV v; for (int i = 0; i < n; i++) v.push_back(nvca_rect{r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]}); return v; }
} // namespace

// (the library is built with hidden visibility and unused sections dropped: host_logic.cpp's overlay blend calls into plan.cpp, which is
// not part of it; only the functions below are exported)
#pragma GCC visibility push(default)
extern "C" {

void *pls_new(int kind, int width_to_process, int process_x_every_4, int scale_factor_pct, int detect_event)
{
    Shim *s = new (std::nothrow) Shim();
    if (s) s->p = nvca_part_params{kind, width_to_process, process_x_every_4, scale_factor_pct, detect_event};
    return s;
}
void pls_free(void *h) { delete (Shim *)h; }
void pls_push_faces(void *h, const int *r, int n) { const RectV v = rects(r, n); ((Shim *)h)->st.push_faces(v.data(), n); }

// conf_images: sizes[4] = face-pass image fw, fh, part image pw, ph; 0: the frame is too small
int pls_scales(void *h, int W, int H, int *sizes)
{
    Shim *s = (Shim *)h;
    if (!part_scales(s->p, W, H, s->sc)) return 0;
    sizes[0] = s->sc.fw; sizes[1] = s->sc.fh; sizes[2] = s->sc.pw; sizes[3] = s->sc.ph;
    return 1;
}
// the frame gate: f[8] = early_return, run, popped, eye_chain, face_image, face_post_eq, mirror, pass; *pass_sf
void pls_gate(void *h, int *f, double *pass_sf)
{
    Shim *s = (Shim *)h;
    s->fr = part_gate(s->st, s->p);
    s->searches.clear();
    f[0] = s->fr.early_return; f[1] = s->fr.run; f[2] = s->fr.popped; f[3] = s->fr.eye_chain; f[4] = s->fr.face_image; f[5] = s->fr.face_post_eq;
    f[6] = s->fr.mirror; f[7] = s->fr.pass; *pass_sf = s->fr.pass_sf;
}
// r[6] = min_neighbors, flags, minw, minh, max_is_image, mirrored
void pls_pass_rule(int pass, int *r)
{
    const FacePassRule &q = face_pass_rule(pass);
    r[0] = q.min_neighbors; r[1] = q.flags; r[2] = q.minw; r[3] = q.minh; r[4] = q.max_is_image; r[5] = q.mirrored;
}
// the searches of the frame; nf / nm < 0: no face pass / no mirrored pass.  out[k * 11 ..] = roi x, y, w, h, cascade, side, min_neighbors,
// flags, minw, minh, valid; sf[k].  Returns their number (all of them are kept in the handle for pls_finish), -1: more than cap.
int pls_rois(void *h, const int *faces, int nf, const int *mirror, int nm, int cap, int *out, double *sf)
{
    Shim *s = (Shim *)h;
    const RectV f = rects(faces, nf < 0 ? 0 : nf), m = rects(mirror, nm < 0 ? 0 : nm);
    part_rois(s->st, s->p, s->sc, s->fr, nf < 0 ? nullptr : &f, nm < 0 ? nullptr : &m, s->searches);
    if ((int)s->searches.size() > cap) return -1;
    for (size_t k = 0; k < s->searches.size(); k++) {
        const PartSearch &q = s->searches[k];
        int *o = out + 11 * k;
        o[0] = q.roi.x; o[1] = q.roi.y; o[2] = q.roi.w; o[3] = q.roi.h; o[4] = q.cascade; o[5] = q.side; o[6] = q.min_neighbors; o[7] = q.flags;
        o[8] = q.minw; o[9] = q.minh; o[10] = q.valid; sf[k] = q.sf;
    }
    return (int)s->searches.size();
}
// merging, hysteresis, clearing; search k found counts[k] rectangles (< 0: not searched), laid end to end in found
void pls_finish(void *h, const int *found, const int *counts)
{
    Shim *s = (Shim *)h;
    std::vector<RectV> res(s->searches.size());
    std::vector<const RectV *> ptr;
    size_t at = 0;
    for (size_t k = 0; k < s->searches.size(); k++) {
        if (counts[k] >= 0) { res[k] = rects(found + 4 * at, counts[k]); at += (size_t)counts[k]; }
        ptr.push_back(counts[k] >= 0 ? &res[k] : nullptr);
    }
    part_finish(s->st, s->p, s->sc, s->fr, s->searches, ptr);
}
// output list a (0) / b (1): its length; up to cap rectangles into out
int pls_list(void *h, int which, int *out, int cap)
{
    const RectV &l = which ? ((Shim *)h)->st.lb : ((Shim *)h)->st.la;
    for (size_t k = 0; k < l.size() && (int)k < cap; k++) { out[4 * k] = l[k].x; out[4 * k + 1] = l[k].y; out[4 * k + 2] = l[k].w; out[4 * k + 3] = l[k].h; }
    return (int)l.size();
}

} // extern "C"
#pragma GCC visibility pop
