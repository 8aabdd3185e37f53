// lbp_group_tables_driver.cpp -- the tables k_group reads on a new-format LBP scan (csrc/lbp_tables.cpp: a ScaleRec per pyramid level and
// the levels' output coordinates) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program built without any HIP
// include path: tests/test_lbp_streams_cpu.py hands it a manifest and checks every line it prints.  Manifest lines:
//   scan ID XML cols rows sf minw minh maxw maxh      lbp_levels(..., every level) -> pyr_layout -> build_lbp_tables
// One JSON line per case: the key layout, per level [factor, step, nx, ny] and the ScaleRec fields k_group and its launch use, the
// position table, and whether every field k_group does not read is zero.
#include "lbp_tables.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

using namespace nvca;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: lbp_group_tables_driver MANIFEST\n"); return 2; }
    std::ifstream mf(argv[1]);
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    int n = 0;
    while (std::getline(mf, line)) {
        std::istringstream in(line);
        std::string verb, id, path;
        int cols, rows, minw, minh, maxw, maxh; double sf;
        if (!(in >> verb >> id)) continue;
        if (verb != "scan" || !(in >> path >> cols >> rows >> sf >> minw >> minh >> maxw >> maxh)) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        std::ifstream f(path, std::ios::binary);
        if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); return 2; }
        std::stringstream ss; ss << f.rdbuf();
        const std::string text = ss.str();
        CascadeFile c; std::string err;
        if (parse_cascade_file(text.data(), text.size(), c, err) || c.format != NVCA_CASCADE_LBP) { fprintf(stderr, "%s: not a new-format LBP cascade (%s)\n", path.c_str(), err.c_str()); return 2; }
        const PyrLayout lay = pyr_layout(lbp_levels(c.lbp.ow, c.lbp.oh, cols, rows, sf, minw, minh, maxw, maxh, kMaxPyrLevels + 1), cols);
        LbpTables t;
        const int rc = lay.lv.empty() ? 0 : build_lbp_tables(c.lbp, lay.lv, lay.P, t, err);
        printf("{\"case\": \"%s\", \"rc\": %d, \"key_sy\": %d, \"key_ss\": %d, \"levels\": [", id.c_str(), rc, t.key_sy, t.key_ss);
        for (size_t i = 0; i < t.levels.size(); i++)
            printf("%s[%.17g, %d, %d, %d]", i ? ", " : "", lay.lv[i].f, t.levels[i].step, t.levels[i].nx, t.levels[i].ny);
        printf("], \"scales\": [");
        bool rest_zero = true;
        for (size_t i = 0; i < t.gscales.size(); i++) {
            ScaleRec g = t.gscales[i];
            printf("%s[%d, %d, %d, %d, %d, %d, %d, %d, %.17g]", i ? ", " : "", g.winw, g.winh, g.endX, g.endY, g.xpos_off, g.ypos_off, g.plane_off, g.pitch, g.factor);
            g.winw = g.winh = g.endX = g.endY = g.xpos_off = g.ypos_off = g.plane_off = g.pitch = 0; g.factor = 0;
            const ScaleRec zero = ScaleRec();
            rest_zero = rest_zero && memcmp(&g, &zero, sizeof(g)) == 0;
        }
        printf("], \"rest_zero\": %s, \"pos\": [", rest_zero ? "true" : "false");
        for (size_t i = 0; i < t.gpos.size(); i++) printf("%s%d", i ? ", " : "", t.gpos[i]);
        printf("]}\n");
        n++;
    }
    fprintf(stderr, "%d cases\n", n);
    return 0;
}
