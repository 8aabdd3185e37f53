// hgen_tables_driver.cpp -- the cascade loader (csrc/cascade_xml.cpp) with NVCA_LOAD_HAAR_GENERAL and, for every file that loads as a
// general new-format HAAR cascade, the table builder of its scan (csrc/hgen_tables.cpp on hnew_tables.cpp, lbp_tables.cpp and
// pyr_levels.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program built without any HIP include path:
// tests/test_haar_tree_loader_san_cpu.py hands it a manifest of "case-id flags path" lines.  Every file is read into a heap block of
// exactly its size (a read past the text is a finding), parsed with parse_cascade_file, and answered with one JSON line: status, format,
// shape, whether the model is general, whether an error text came back, the model as the tree dump states it, and the tables of its
// scan of a 97 x 83 image at scale factor 1.2 (an image three windows wide where the window is larger): every field of every node
// record, the weak classifiers' places, the normalisation rectangle.
#include "hgen_tables.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>

using namespace nvca;

static void put_ints(const char *name, const int *v, int n)
{
    printf("\"%s\": [", name);
    for (int k = 0; k < n; k++) printf("%s%d", k ? ", " : "", v[k]);
    printf("]");
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: hgen_tables_driver MANIFEST\n"); return 2; }
    std::ifstream mf(argv[1]);
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string id, path;
    unsigned flags = 0;
    int n = 0;
    while (mf >> id >> flags >> path) {
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); return 2; }
        fseek(f, 0, SEEK_END);
        const long len = ftell(f);
        fseek(f, 0, SEEK_SET);
        char *buf = (char *)malloc(len > 0 ? (size_t)len : 1);
        if (len > 0 && fread(buf, 1, (size_t)len, f) != (size_t)len) { fprintf(stderr, "short read %s\n", path.c_str()); return 2; }
        fclose(f);
        CascadeFile c;
        std::string err;
        const int rc = len > 0 ? parse_cascade_file(buf, (size_t)len, flags, c, err) : NVCA_ERR_ARG;
        free(buf);
        const bool hnew = !rc && c.format == NVCA_CASCADE_HAAR_NEW, lbp = !rc && c.format == NVCA_CASCADE_LBP;
        const HnewCascade &h = c.hnew;
        printf("{\"case\": \"%s\", \"rc\": %d, \"format\": %d, \"shape\": [%d, %d, %d, %d], \"general\": %s, \"err\": %s", id.c_str(), rc, rc ? -1 : c.format,
               rc ? 0 : c.haar.ow, rc ? 0 : c.haar.oh, rc ? 0 : (int)(hnew ? h.stages.size() : lbp ? c.lbp.stages.size() : c.haar.stages.size()),
               rc ? 0 : (int)(hnew ? h.nweak() : lbp ? c.lbp.weak.size() : c.haar.cls.size()), hnew && h.general ? "true" : "false", err.empty() ? "false" : "true");
        if (hnew && h.general) {
            printf(", \"model\": {\"tilted\": [");
            for (size_t i = 0; i < h.tilted.size(); i++) printf("%s%d", i ? ", " : "", (int)h.tilted[i]);
            printf("], \"node_counts\": [");
            for (size_t i = 0; i < h.trees.size(); i++) printf("%s%d", i ? ", " : "", h.trees[i].nnodes);
            printf("], \"nodes\": [");
            for (size_t i = 0; i < h.nodes.size(); i++) printf("%s[%d, %d, %d, %.9g]", i ? ", " : "", h.nodes[i].left, h.nodes[i].right, h.nodes[i].feature, h.nodes[i].threshold);
            printf("], \"leaves\": [");
            for (size_t i = 0; i < h.leaves.size(); i++) printf("%s%.9g", i ? ", " : "", h.leaves[i]);
            printf("]}");
            const int cols = h.ow > 30 ? 3 * h.ow : 97, rows = h.oh > 30 ? 3 * h.oh : 83;
            const PyrLayout lay = pyr_layout(lbp_levels(h.ow, h.oh, cols, rows, 1.2, 0, 0, cols, rows, kMaxPyrLevels + 1), cols);
            HgenTables t; std::string terr;
            const int trc = lay.lv.empty() ? -1 : build_hgen_tables(h, lay.lv, lay.P, t, terr);
            const LbpTables &s = t.base.scan;
            printf(", \"tables\": {\"rc\": %d, \"P\": %d, \"TP\": %d, \"levels\": %zu, \"stages\": %zu, \"tile_stages\": %d, \"lds\": %d, \"stump_weak\": %zu, \"area\": %.17g, ",
                   trc, lay.P, s.TP, s.levels.size(), s.stages.size(), s.tile_stages, s.lds, t.base.gweak.size() + t.base.tweak.size() + s.gweak.size() + s.tweak.size(), t.base.area);
            put_ints("nr", t.base.nr, 4); printf(", "); put_ints("nrt", t.base.nrt, 4);
            printf(", \"stage_first\": [");
            for (size_t i = 0; i < s.stages.size(); i++) printf("%s[%d, %d]", i ? ", " : "", s.stages[i].first, s.stages[i].count);
            printf("], \"weak\": [");
            for (size_t i = 0; i < t.weak.size(); i++) printf("%s[%d, %d]", i ? ", " : "", t.weak[i].first, t.weak[i].count);
            printf("], \"nodes\": [");
            for (size_t i = 0; i < t.nodes.size(); i++) {
                const HgenNodeDev &d = t.nodes[i];
                printf("%s{", i ? ", " : "");
                put_ints("off", d.off, 12); printf(", "); put_ints("offt", d.offt, 12);
                printf(", \"w\": [%.9g, %.9g, %.9g], \"thr\": %.9g, \"left\": %d, \"right\": %d, \"tilted\": %d, \"lv\": [%.9g, %.9g], \"pad\": %d}",
                       d.w[0], d.w[1], d.w[2], d.thr, d.left, d.right, d.tilted, d.lv[0], d.lv[1], d.pad | d.pad2[0] | d.pad2[1]);
            }
            printf("]}");
        }
        printf("}\n");
        n++;
    }
    fprintf(stderr, "%d files\n", n);
    return 0;
}
