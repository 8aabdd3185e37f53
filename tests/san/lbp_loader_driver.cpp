// lbp_loader_driver.cpp -- the cascade loader alone (csrc/cascade_xml.cpp: both formats) under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a stand-alone program: tests/test_lbp_loader_san_cpu.py builds it and hands it a manifest of
// "case-id path" lines.  Every file is read into a heap block of exactly its size (a read past the text is a finding), parsed
// with parse_cascade_file, and answered with one JSON line: status, format, shape, whether an error text came back.
#include "cascade_model.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

using namespace nvca;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: lbp_loader_driver MANIFEST\n"); return 2; }
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
        const bool lbp = c.format == NVCA_CASCADE_LBP;
        long long sum = 0;                              // touch everything the loader filled
        for (const LbpWeak &w : c.lbp.weak) { sum += c.lbp.features[(size_t)w.feature].w; for (int k = 0; k < 8; k++) sum += w.subset[k] & 1; }
        for (const LbpStage &s : c.lbp.stages) sum += s.first + s.count;
        printf("{\"case\": \"%s\", \"rc\": %d, \"format\": %d, \"shape\": [%d, %d, %d, %d], \"err\": %s, \"touch\": %lld}\n", id.c_str(), rc, rc ? -1 : c.format,
               rc ? 0 : c.haar.ow, rc ? 0 : c.haar.oh, rc ? 0 : (int)(lbp ? c.lbp.stages.size() : c.haar.stages.size()),
               rc ? 0 : (int)(lbp ? c.lbp.weak.size() : c.haar.cls.size()), err.empty() ? "false" : "true", rc ? 0 : sum);
        n++;
    }
    fprintf(stderr, "%d files\n", n);
    return 0;
}
