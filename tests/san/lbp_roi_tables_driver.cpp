// lbp_roi_tables_driver.cpp -- what the small-image LBP evaluator is launched with (csrc/lbp_roi_tables.cpp: the LDS bound, a job's
// step records with their resize tables, the bands of whole rows, the cascade's device table) on the loader's cascades
// (csrc/cascade_xml.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (linked with plan.cpp for
// build_resize_tab, without any HIP library): tests/test_lbp_roi_cpu.py hands it a manifest and checks every line it prints.  Manifest lines:
//   consts ID                                           the route's constants
//   fits   ID cols rows                                 lbp_roi_fits_lds / lbp_roi_image_bytes
//   steps  ID XML cols rows sf minw minh maxw maxh      build_lbp_roi_steps -> roi_split_bands, build_lbp_roi_table
// One JSON line per case.  Every table a step record names is read through, entry by entry, at the offsets the kernel would use.
#include "lbp_roi_tables.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

using namespace nvca;

static void load(const std::string &path, CascadeFile &c)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    std::stringstream ss; ss << f.rdbuf();
    const std::string text = ss.str();
    std::string err;
    const int rc = parse_cascade_file(text.data(), text.size(), c, err);
    if (rc || c.format != NVCA_CASCADE_LBP) { fprintf(stderr, "%s: not a new-format LBP cascade (%d: %s)\n", path.c_str(), rc, err.c_str()); exit(2); }
}

static void steps(const std::string &id, const LbpCascade &c, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh)
{
    const size_t tab0 = 40;          // (a blob that holds something already, not a multiple of 16)
    LbpRoiSteps ls;
    build_lbp_roi_steps(c, cols, rows, sf, minw, minh, maxw, maxh, tab0, ls);
    printf("{\"case\": \"%s\", \"fits\": %s, \"plane_words\": %d, \"lev_bytes\": %d, \"levels\": [", id.c_str(), ls.fits ? "true" : "false", ls.plane_words, ls.lev_bytes);
    for (size_t i = 0; i < ls.info.size(); i++) printf("%s[%.17g, %d, %d]", i ? ", " : "", ls.info[i].factor, ls.info[i].winw, ls.info[i].winh);
    // the blob as the launch holds it: tab0 bytes of something else, then this job's tables -- copied to a buffer of exactly that size
    std::vector<unsigned char> blob(tab0 + ls.tabs.size());
    if (!ls.tabs.empty()) memcpy(blob.data() + tab0, ls.tabs.data(), ls.tabs.size());
    long long tabsum = 0; bool aligned = true;
    for (const RoiStep &st : ls.steps) {
        if (st.mode != 1) continue;
        aligned = aligned && !(st.xofs_off & 15) && !(st.yofs_off & 15) && !(st.ialpha_off & 15) && !(st.ibeta_off & 15);
        const int *xofs = (const int *)(blob.data() + st.xofs_off), *yofs = (const int *)(blob.data() + st.yofs_off);
        const short *ia = (const short *)(blob.data() + st.ialpha_off), *ib = (const short *)(blob.data() + st.ibeta_off);
        for (int x = 0; x < st.szw; x++) tabsum += xofs[x] + ia[2 * x] + ia[2 * x + 1];
        for (int y = 0; y < st.szh; y++) tabsum += yofs[y] + ib[2 * y] + ib[2 * y + 1];
    }
    std::vector<RoiStep> bands = ls.steps;
    const bool rows_fit = roi_split_bands(bands);
    printf("], \"tabs_aligned\": %s, \"tabsum\": %lld, \"rows_fit\": %s, \"bands\": [", aligned ? "true" : "false", tabsum, rows_fit ? "true" : "false");
    for (size_t i = 0; i < bands.size(); i++) {
        const RoiStep &b = bands[i];
        printf("%s[%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d]", i ? ", " : "", b.key_step, b.szw, b.szh, b.step, b.mode, b.startX, b.endX, b.startY, b.endY,
               b.key_x0, b.key_dx, b.key_y0, b.key_dy, b.xmax);
    }
    std::vector<unsigned char> tab; build_lbp_roi_table(c, tab);
    const LbpStageDev *sd = (const LbpStageDev *)tab.data();
    const RoiLbpWeak *wk = (const RoiLbpWeak *)(tab.data() + roi_lbp_weak_off((int)c.stages.size()));
    printf("], \"lds\": %d, \"weak_off\": %zu, \"table_bytes\": %zu, \"stages\": [", roi_lbp_lds_bytes(ls.plane_words, ls.lev_bytes), roi_lbp_weak_off((int)c.stages.size()), tab.size());
    for (size_t i = 0; i < c.stages.size(); i++) printf("%s[%d, %d, %.9g, %d]", i ? ", " : "", sd[i].first, sd[i].count, sd[i].thr, sd[i].pad);
    printf("], \"weak\": [");
    for (size_t i = 0; i < c.weak.size(); i++) {
        printf("%s{\"rect\": [%d, %d, %d, %d], \"subset\": [", i ? ", " : "", wk[i].x, wk[i].y, wk[i].w, wk[i].h);
        for (int k = 0; k < 8; k++) printf("%s%d", k ? ", " : "", wk[i].subset[k]);
        printf("], \"leaf\": [%.9g, %.9g], \"pad\": %d}", wk[i].leaf[0], wk[i].leaf[1], wk[i].pad[0] | wk[i].pad[1]);
    }
    printf("]}\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: lbp_roi_tables_driver MANIFEST\n"); return 2; }
    std::ifstream mf(argv[1]);
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    int n = 0;
    while (std::getline(mf, line)) {
        std::istringstream in(line);
        std::string verb, id, path;
        if (!(in >> verb >> id)) continue;
        if (verb == "consts") {
            printf("{\"case\": \"%s\", \"max_bytes\": %d, \"short_win\": %d, \"vote_words\": %d, \"max_win\": %d, \"fixed_bytes\": %d, \"weak_bytes\": %zu}\n", id.c_str(),
                   kRoiLbpMaxBytes, kRoiLbpShortWin, kRoiLbpVoteWords, kRoiMaxWin, roi_lbp_fixed_bytes(), sizeof(RoiLbpWeak));
        } else if (verb == "fits") {
            int cols, rows;
            if (!(in >> cols >> rows)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            printf("{\"case\": \"%s\", \"fits\": %s, \"bytes\": %lld}\n", id.c_str(), lbp_roi_fits_lds(cols, rows) ? "true" : "false", lbp_roi_image_bytes(cols, rows));
        } else if (verb == "steps") {
            int cols, rows, minw, minh, maxw, maxh; double sf;
            if (!(in >> path >> cols >> rows >> sf >> minw >> minh >> maxw >> maxh)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            CascadeFile c; load(path, c);
            steps(id, c.lbp, cols, rows, sf, minw, minh, maxw, maxh);
        } else { fprintf(stderr, "unknown verb: %s\n", line.c_str()); return 2; }
        n++;
    }
    fprintf(stderr, "%d cases\n", n);
    return 0;
}
