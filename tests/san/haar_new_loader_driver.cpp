// haar_new_loader_driver.cpp -- the cascade loader (csrc/cascade_xml.cpp) on new-format HAAR files and, for every file that loads as
// one, the table builder of its scan (csrc/hnew_tables.cpp on csrc/lbp_tables.cpp and csrc/pyr_levels.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a stand-alone program built without any HIP include path: tests/test_haar_new_loader_san_cpu.py hands
// it a manifest of "case-id path" lines.  Every file is read into a heap block of exactly its size (a read past the text is a finding),
// parsed with parse_cascade_file, and answered with one JSON line: status, format, shape, whether an error text came back, and -- for a
// new-format HAAR cascade -- the tables of its scan of a 97 x 83 image at scale factor 1.2 (or of an image three windows wide where the
// window is larger): the weak records at both pitches, the normalisation rectangle, the shared scan tables' sizes.
#include "hnew_tables.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

using namespace nvca;

static void put_weak(const char *name, const std::vector<HnewWeakDev> &t)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < t.size(); i++) {
        printf("%s{\"off\": [", i ? ", " : "");
        for (int k = 0; k < 12; k++) printf("%s%d", k ? ", " : "", t[i].off[k]);
        printf("], \"w\": [%.9g, %.9g, %.9g], \"thr\": %.9g, \"leaf\": [%.9g, %.9g], \"pad\": %d}", t[i].w[0], t[i].w[1], t[i].w[2], t[i].thr, t[i].leaf[0], t[i].leaf[1],
               t[i].pad[0] | t[i].pad[1]);
    }
    printf("]");
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: haar_new_loader_driver MANIFEST\n"); return 2; }
    std::ifstream mf(argv[1]);
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string id, path;
    int n = 0;
    while (mf >> id >> path) {
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
        const int rc = len > 0 ? parse_cascade_file(buf, (size_t)len, c, err) : NVCA_ERR_ARG;
        free(buf);
        const bool hnew = !rc && c.format == NVCA_CASCADE_HAAR_NEW, lbp = !rc && c.format == NVCA_CASCADE_LBP;
        long long sum = 0;                              // touch everything the loader filled
        for (const HnewWeak &w : c.hnew.weak) { const HnewFeature &ft = c.hnew.features[(size_t)w.feature]; sum += ft.nrect + ft.rect[2][3] + (w.leaf[0] < w.leaf[1]); }
        for (const LbpStage &s : c.hnew.stages) sum += s.first + s.count;
        printf("{\"case\": \"%s\", \"rc\": %d, \"format\": %d, \"shape\": [%d, %d, %d, %d], \"err\": %s, \"touch\": %lld", id.c_str(), rc, rc ? -1 : c.format,
               rc ? 0 : c.haar.ow, rc ? 0 : c.haar.oh, rc ? 0 : (int)(hnew ? c.hnew.stages.size() : lbp ? c.lbp.stages.size() : c.haar.stages.size()),
               rc ? 0 : (int)(hnew ? c.hnew.weak.size() : lbp ? c.lbp.weak.size() : c.haar.cls.size()), err.empty() ? "false" : "true", rc ? 0 : sum);
        if (hnew) {
            const int cols = c.hnew.ow > 30 ? 3 * c.hnew.ow : 97, rows = c.hnew.oh > 30 ? 3 * c.hnew.oh : 83;
            const PyrLayout lay = pyr_layout(lbp_levels(c.hnew.ow, c.hnew.oh, cols, rows, 1.2, 0, 0, cols, rows, kMaxPyrLevels + 1), cols);
            HnewTables t; std::string terr;
            const int trc = lay.lv.empty() ? -1 : build_hnew_tables(c.hnew, lay.lv, lay.P, t, terr);
            printf(", \"tables\": {\"rc\": %d, \"P\": %d, \"TP\": %d, \"levels\": %zu, \"tiles\": %zu, \"stages\": %zu, \"tile_stages\": %d, \"lds\": %d, \"scan_weak\": %zu, "
                   "\"nr\": [%d, %d, %d, %d], \"nrt\": [%d, %d, %d, %d], \"area\": %.17g, ", trc, lay.P, t.scan.TP, t.scan.levels.size(), t.scan.tiles.size(), t.scan.stages.size(),
                   t.scan.tile_stages, t.scan.lds, t.scan.gweak.size() + t.scan.tweak.size(), t.nr[0], t.nr[1], t.nr[2], t.nr[3], t.nrt[0], t.nrt[1], t.nrt[2], t.nrt[3], t.area);
            put_weak("gweak", t.gweak); printf(", "); put_weak("tweak", t.tweak);
            printf("}");
        }
        printf("}\n");
        n++;
    }
    fprintf(stderr, "%d files\n", n);
    return 0;
}
