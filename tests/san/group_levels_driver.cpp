// group_levels_driver.cpp -- the weighted groupRectangles of detectMultiScale with outputRejectLevels (csrc/group_levels.cpp on
// host_logic.cpp's partition and averaging) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
// tests/test_levels_cpu.py hands it a manifest and checks every line it prints against the numpy statement.  Manifest:
//   case ID groupThreshold eps n          followed by n lines:   x y w h level weight-bits
// (weight-bits: the double's 64 bits as an unsigned decimal, so that no digit is lost either way).  One JSON line per case:
//   {"case": ID, "ok": true, "rects": [[x, y, w, h] ...], "levels": [...], "weights": [bits ...]}
// A last built-in case hands the function lists of unequal lengths: it must refuse and leave them alone.
#include "group_levels.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace nvca;

// host_logic.cpp's overlay code calls plan.cpp's table builder; nothing here reaches it: a link double, so that the program is built from
// group_levels.cpp and host_logic.cpp alone
namespace nvca { struct ResizeTab; void build_resize_tab(int, int, int, int, ResizeTab &) { abort(); } }

static void print_case(const std::string &id, bool ok, const std::vector<nvca_rect> &r, const std::vector<int> &lv, const std::vector<double> &wt)
{
    printf("{\"case\": \"%s\", \"ok\": %s, \"rects\": [", id.c_str(), ok ? "true" : "false");
    for (size_t i = 0; i < r.size(); i++) printf("%s[%d, %d, %d, %d]", i ? ", " : "", r[i].x, r[i].y, r[i].w, r[i].h);
    printf("], \"levels\": [");
    for (size_t i = 0; i < lv.size(); i++) printf("%s%d", i ? ", " : "", lv[i]);
    printf("], \"weights\": [");
    for (size_t i = 0; i < wt.size(); i++) { uint64_t b; memcpy(&b, &wt[i], 8); printf("%s%" PRIu64, i ? ", " : "", b); }
    printf("]}\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: group_levels_driver MANIFEST\n"); return 2; }
    std::ifstream mf(argv[1]);
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    int ncases = 0;
    while (std::getline(mf, line)) {
        std::istringstream in(line);
        std::string verb, id; int thr, n; double eps;
        if (!(in >> verb)) continue;
        if (verb != "case" || !(in >> id >> thr >> eps >> n) || n < 0) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        std::vector<nvca_rect> r((size_t)n); std::vector<int> lv((size_t)n); std::vector<double> wt((size_t)n);
        for (int i = 0; i < n; i++) {
            uint64_t bits;
            if (!std::getline(mf, line)) { fprintf(stderr, "%s: short case\n", id.c_str()); return 2; }
            std::istringstream row(line);
            if (!(row >> r[i].x >> r[i].y >> r[i].w >> r[i].h >> lv[i] >> bits)) { fprintf(stderr, "bad row: %s\n", line.c_str()); return 2; }
            memcpy(&wt[i], &bits, 8);
        }
        const bool ok = group_rectangles_levels(r, lv, wt, thr, eps);
        print_case(id, ok, r, lv, wt);
        ncases++;
    }
    {   // lists of unequal lengths
        std::vector<nvca_rect> r(3, nvca_rect{1, 2, 3, 4}); std::vector<int> lv(2, 5); std::vector<double> wt(3, 1.0);
        const bool ok = group_rectangles_levels(r, lv, wt, 1, 0.2);
        print_case("unequal-lengths", ok, r, lv, wt);
    }
    fprintf(stderr, "%d cases\n", ncases);
    return 0;
}
