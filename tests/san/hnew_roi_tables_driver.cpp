// hnew_roi_tables_driver.cpp -- what the small-image evaluator of new-format HAAR cascades is launched with (csrc/hnew_roi_tables.cpp:
// the LDS bound and the cascade's device table; csrc/lbp_roi_tables.cpp on the window size: a job's step records with their resize
// tables and the bands of whole rows) on the loader's cascades (csrc/cascade_xml.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a stand-alone program (linked with plan.cpp for build_resize_tab, without any HIP library):
// tests/test_hnew_roi_cpu.py hands it a manifest and checks every line it prints.  Manifest lines:
//   consts ID                                           the route's constants
//   fits   ID cols rows                                 hnew_roi_fits_lds / hnew_roi_image_bytes
//   steps  ID XML cols rows sf minw minh maxw maxh      build_lbp_roi_steps(ow, oh, ...) -> roi_split_bands, build_hnew_roi_table
// One JSON line per case.  Every table a step record names is read through, entry by entry, at the offsets the kernel would use.
#include "hnew_roi_tables.h"
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
    if (rc || c.format != NVCA_CASCADE_HAAR_NEW) { fprintf(stderr, "%s: not a new-format HAAR cascade (%d: %s)\n", path.c_str(), rc, err.c_str()); exit(2); }
}

static void steps(const std::string &id, const HnewCascade &c, int cols, int rows, double sf, int minw, int minh, int maxw, int maxh)
{
    const size_t tab0 = 40;          // (a blob that holds something already, not a multiple of 16)
    LbpRoiSteps ls;
    build_lbp_roi_steps(c.ow, c.oh, cols, rows, sf, minw, minh, maxw, maxh, tab0, ls);
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
    std::vector<unsigned char> tab; build_hnew_roi_table(c, tab);
    const size_t o_weak = roi_hnew_weak_off((int)c.stages.size());
    const LbpStageDev *sd = (const LbpStageDev *)tab.data();
    const RoiHnewWeak *wk = (const RoiHnewWeak *)(tab.data() + o_weak);
    // what lies between the stage records and the weak records, and behind the last weak record: zeros
    int slack = 0;
    for (size_t i = c.stages.size() * sizeof(LbpStageDev); i < o_weak; i++) slack |= tab[i];
    for (size_t i = o_weak + c.weak.size() * sizeof(RoiHnewWeak); i < tab.size(); i++) slack |= tab[i];
    printf("], \"lds\": %d, \"weak_off\": %zu, \"table_bytes\": %zu, \"tail_bytes\": %zu, \"slack\": %d, \"stages\": [", roi_hnew_lds_bytes(ls.plane_words), o_weak, tab.size(),
           tab.size() - o_weak - c.weak.size() * sizeof(RoiHnewWeak), slack);
    for (size_t i = 0; i < c.stages.size(); i++) printf("%s[%d, %d, %.9g, %d]", i ? ", " : "", sd[i].first, sd[i].count, sd[i].thr, sd[i].pad);
    printf("], \"weak\": [");
    for (size_t i = 0; i < c.weak.size(); i++) {
        printf("%s{\"rects\": [", i ? ", " : "");
        for (int r = 0; r < 3; r++) printf("%s[%d, %d, %d, %d]", r ? ", " : "", wk[i].rect[r][0], wk[i].rect[r][1], wk[i].rect[r][2], wk[i].rect[r][3]);
        printf("], \"w\": [%.9g, %.9g, %.9g], \"thr\": %.9g, \"leaf\": [%.9g, %.9g], \"pad\": %d}", wk[i].w[0], wk[i].w[1], wk[i].w[2], wk[i].thr, wk[i].leaf[0], wk[i].leaf[1],
               wk[i].pad[0] | wk[i].pad[1]);
    }
    printf("]}\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: hnew_roi_tables_driver MANIFEST\n"); return 2; }
    std::ifstream mf(argv[1]);
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    int n = 0;
    while (std::getline(mf, line)) {
        std::istringstream in(line);
        std::string verb, id, path;
        if (!(in >> verb >> id)) continue;
        if (verb == "consts") {
            printf("{\"case\": \"%s\", \"max_bytes\": %d, \"short_win\": %d, \"vote_words\": %d, \"max_win\": %d, \"fixed_bytes\": %d, \"lev_bytes\": %d, \"weak_bytes\": %zu}\n", id.c_str(),
                   kRoiHnewMaxBytes, kRoiHnewShortWin, kRoiHnewVoteWords, kRoiMaxWin, roi_hnew_fixed_bytes(), kRoiHnewLevBytes, sizeof(RoiHnewWeak));
        } else if (verb == "fits") {
            int cols, rows;
            if (!(in >> cols >> rows)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            printf("{\"case\": \"%s\", \"fits\": %s, \"bytes\": %lld}\n", id.c_str(), hnew_roi_fits_lds(cols, rows) ? "true" : "false", hnew_roi_image_bytes(cols, rows));
        } else if (verb == "steps") {
            int cols, rows, minw, minh, maxw, maxh; double sf;
            if (!(in >> path >> cols >> rows >> sf >> minw >> minh >> maxw >> maxh)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            CascadeFile c; load(path, c);
            steps(id, c.hnew, cols, rows, sf, minw, minh, maxw, maxh);
        } else { fprintf(stderr, "unknown verb: %s\n", line.c_str()); return 2; }
        n++;
    }
    fprintf(stderr, "%d cases\n", n);
    return 0;
}
