// stage_recs_driver.cpp -- test infrastructure (never shipped): loads cascades with the product's cascade_xml.cpp and prints the
// StageRec of every stage that plan.cpp's build_stage_recs makes of them, as one JSON line per cascade, for
// tests/test_stage_sums_cpu.py (the proof that a stage's votes may be summed in any order, and the integer form of the stage).
// Next to every record it prints what the record was made from -- the stage threshold and the two votes of every stump as
// the loader stored them -- in C99 hex-float notation ("%a"), so that the test checks the record against exact arithmetic
// on exactly those numbers.  Like tile_geom_driver.cpp it links no HIP library: the few runtime calls of plan.cpp get host
// doubles, nothing runs a kernel.
//
//   stage_recs_driver <cascade.xml> ...      one line per file: {"file", "error"} or {"file", "stages": [...]}
#include "../../nubomedia-vca_amd/csrc/plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

extern "C" hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) { memcpy(dst, src, n); return hipSuccess; }
extern "C" hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
extern "C" hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
namespace nvca {
struct Workspace { int unused; };
struct GeomPlan { int unused; };
int DevBuf::ensure(size_t n) { if (n <= bytes) return 0; free(p); p = malloc(n); bytes = p ? n : 0; return p ? 0 : 1; }
void DevBuf::release() { if (p && bytes) free(p); p = nullptr; bytes = 0; }
DetectPlan::~DetectPlan() { release_tables(); d_blob.release(); }
}
nvca_ctx::nvca_ctx() {}
nvca_ctx::~nvca_ctx() { plans.clear(); nvca::free_scale_tables(this); }

using namespace nvca;

static void hexf(double v) { printf("\"%a\"", v); }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: stage_recs_driver <xml> ...\n"); return 2; }
    for (int a = 1; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        std::stringstream ss; ss << f.rdbuf();
        const std::string xml = ss.str();
        Cascade c;
        std::string err;
        printf("{\"file\": \"%s\", ", argv[a]);
        if (int rc = parse_cascade_xml(xml.data(), xml.size(), c, err)) {
            std::string e;
            for (char ch : err) if (ch != '"' && ch != '\\') e += ch;
            printf("\"error\": %d, \"message\": \"%s\"}\n", rc, e.c_str());
            continue;
        }
        std::vector<StageRec> st;
        build_stage_recs(c, st);
        printf("\"stump_based\": %d, \"stages\": [", c.stump_based ? 1 : 0);
        for (size_t i = 0; i < st.size(); i++) {
            const StageRec &r = st[i];
            printf("%s{\"first\": %d, \"count\": %d, \"flags\": %d, \"thr_i\": %d, \"vote_exp\": %d, \"spec_run\": %d, \"thr\": ",
                   i ? ", " : "", r.first, r.count, r.flags, r.thr_i, r.vote_exp, r.spec_run);
            hexf(r.thr);
            printf(", \"stage_threshold\": "); hexf(c.stages[i].threshold);
            printf(", \"nrect\": [");
            for (int j = 0; j < r.count; j++) printf("%s%d", j ? ", " : "", c.nodes[c.cls[r.first + j].first_node].nrect);
            printf("], \"votes\": [");
            for (int j = 0; j < r.count; j++) {
                const HaarClassifier &hc = c.cls[r.first + j];
                printf("%s[", j ? ", " : ""); hexf(c.alpha[hc.first_alpha]); printf(", "); hexf(c.alpha[hc.first_alpha + 1]); printf("]");
            }
            printf("]}");
        }
        printf("]}\n");
    }
    return 0;
}
