// lbp_tables_driver.cpp -- the pyramid rules (csrc/pyr_levels.cpp) and the LBP table builder (csrc/lbp_tables.cpp) on the loader's
// cascades (csrc/cascade_xml.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program built without any HIP
// include path: tests/test_lbp_tables_cpu.py hands it a manifest and checks every line it prints.  Manifest lines:
//   scan   ID XML cols rows sf minw minh maxw maxh      lbp_levels(..., every level) -> pyr_layout -> build_lbp_tables
//   levels ID XML n szw szh [szw szh ...]               the same from a level list given directly (factor 1, the cascade's window)
//   rules  ID ow oh cols rows sf minw minh maxw maxh    si_levels beside lbp_levels
// One JSON line per case.
#include "lbp_tables.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

using namespace nvca;

static void put_levels(const char *name, const std::vector<SiLevel> &lv)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < lv.size(); i++) printf("%s[%.17g, %d, %d, %d, %d]", i ? ", " : "", lv[i].factor, lv[i].szw, lv[i].szh, lv[i].winw, lv[i].winh);
    printf("]");
}

static void put_weak(const char *name, const std::vector<LbpWeakDev> &t)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < t.size(); i++) {
        printf("%s{\"off\": [", i ? ", " : "");
        for (int k = 0; k < 16; k++) printf("%s%d", k ? ", " : "", t[i].off[k]);
        printf("], \"subset\": [");
        for (int k = 0; k < 8; k++) printf("%s%d", k ? ", " : "", t[i].subset[k]);
        int pad = 0;
        for (int k = 0; k < 6; k++) pad |= t[i].pad[k];
        printf("], \"leaf\": [%.9g, %.9g], \"pad\": %d}", t[i].leaf[0], t[i].leaf[1], pad);
    }
    printf("]");
}

static int load(const std::string &path, CascadeFile &c)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    std::stringstream ss; ss << f.rdbuf();
    const std::string text = ss.str();
    std::string err;
    const int rc = parse_cascade_file(text.data(), text.size(), c, err);
    if (rc || c.format != NVCA_CASCADE_LBP) { fprintf(stderr, "%s: not a new-format LBP cascade (%d: %s)\n", path.c_str(), rc, err.c_str()); exit(2); }
    return rc;
}

static void tables(const std::string &id, const LbpCascade &c, const std::vector<SiLevel> &sl, int cols)
{
    const PyrLayout lay = pyr_layout(sl, cols);
    printf("{\"case\": \"%s\", ", id.c_str());
    put_levels("levels", sl);
    printf(", \"P\": %d, \"gray_total\": %zu, \"plane_total\": %zu, \"layout\": [", lay.P, lay.gray_total, lay.plane_total);
    for (size_t i = 0; i < lay.lv.size(); i++) {
        const PyrLevel &L = lay.lv[i];
        printf("%s[%.17g, %d, %d, %d, %d, %zu, %d, %d]", i ? ", " : "", L.f, L.szw, L.szh, L.winw, L.winh, L.gray_off, L.gpitch, L.plane_off);
    }
    printf("]");
    if (lay.lv.empty()) { printf(", \"built\": false}\n"); return; }             // (a plan without levels builds no tables)
    LbpTables t; std::string err;
    const int rc = build_lbp_tables(c, lay.lv, lay.P, t, err);
    printf(", \"built\": true, \"rc\": %d, \"err\": \"%s\", \"lev\": [", rc, err.c_str());
    for (size_t i = 0; i < t.levels.size(); i++) {
        const LbpLevelDev &d = t.levels[i];
        printf("%s[%d, %d, %d, %d, %d, %d, %d, %d, %d, %d]", i ? ", " : "", d.plane_off, d.szw, d.szh, d.nx, d.ny, d.step, d.wpr, d.bit_off, d.row_first, d.pad0 | d.pad1 | d.pad2);
    }
    printf("], \"tiles\": [");
    for (size_t i = 0; i < t.tiles.size(); i++) printf("%s[%d, %d, %d, %d]", i ? ", " : "", t.tiles[i].level, t.tiles[i].tx, t.tiles[i].ty, t.tiles[i].pad);
    printf("], \"stages\": [");
    for (size_t i = 0; i < t.stages.size(); i++) printf("%s[%d, %d, %.9g, %d]", i ? ", " : "", t.stages[i].first, t.stages[i].count, t.stages[i].thr, t.stages[i].pad);
    printf("], ");
    put_weak("gweak", t.gweak); printf(", "); put_weak("tweak", t.tweak);
    printf(", \"TP\": %d, \"nrows\": %d, \"key_sy\": %d, \"key_ss\": %d, \"tile_stages\": %d, \"lds\": %d, \"bit_words\": %zu, \"positions\": %zu}\n",
           t.TP, t.nrows, t.key_sy, t.key_ss, t.tile_stages, t.lds, t.bit_words, t.positions);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: lbp_tables_driver MANIFEST\n"); return 2; }
    std::ifstream mf(argv[1]);
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    int n = 0;
    while (std::getline(mf, line)) {
        std::istringstream in(line);
        std::string verb, id, path;
        if (!(in >> verb >> id)) continue;
        if (verb == "scan") {
            int cols, rows, minw, minh, maxw, maxh; double sf;
            if (!(in >> path >> cols >> rows >> sf >> minw >> minh >> maxw >> maxh)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            CascadeFile c; load(path, c);
            tables(id, c.lbp, lbp_levels(c.lbp.ow, c.lbp.oh, cols, rows, sf, minw, minh, maxw, maxh, kMaxPyrLevels + 1), cols);
        } else if (verb == "levels") {
            int nl;
            if (!(in >> path >> nl)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            CascadeFile c; load(path, c);
            std::vector<SiLevel> sl; int cols = 0;
            for (int k = 0; k < nl; k++) {
                int szw, szh;
                if (!(in >> szw >> szh)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
                sl.push_back(SiLevel{1., szw, szh, c.lbp.ow, c.lbp.oh});
                if (szw > cols) cols = szw;
            }
            tables(id, c.lbp, sl, cols);
        } else if (verb == "rules") {
            int ow, oh, cols, rows, minw, minh, maxw, maxh; double sf;
            if (!(in >> ow >> oh >> cols >> rows >> sf >> minw >> minh >> maxw >> maxh)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            printf("{\"case\": \"%s\", ", id.c_str());
            put_levels("si", si_levels(ow, oh, cols, rows, sf, minw, minh, maxw, maxh, kMaxPyrLevels + 1)); printf(", ");
            put_levels("lbp", lbp_levels(ow, oh, cols, rows, sf, minw, minh, maxw, maxh, kMaxPyrLevels + 1));
            printf(", \"steps\": [%d, %d, %d]}\n", level_step(1.), level_step(2.), level_step(2.0000001));
        } else { fprintf(stderr, "unknown verb: %s\n", line.c_str()); return 2; }
        n++;
    }
    fprintf(stderr, "%d cases\n", n);
    return 0;
}
