// options_driver.cpp -- test infrastructure: the table of the context's switches (csrc/options.cpp) under ASan + UBSan.  Every
// row is checked against expectations written out here by hand: what the environment variable makes of the process default,
// what option_set stores and option_get returns, which options drop the cached plans, and that an unknown name is refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../nubomedia-vca_amd/csrc/switches.h"
using nvca::Switches;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "options_driver: check failed at line %d: %s [%s]\n", __LINE__, #c, what.c_str()); return 1; } } while (0)

enum Env { PRESENT, ABSENT, BOOL01, RAW, ATLEAST1, COUNT8 };
enum Set { ASGIVEN, FLAG, POS_OR_1, POS_OR_0 };
struct Row { const char *name, *env; int dflt; int (*member)(const Switches &); Env from_env; Set on_set; bool replan; };
#define M(m) [](const Switches &w) -> int { return w.m; }
static const Row rows[] = {
    {"group_zerocopy", "NVCA_GROUP_ZEROCOPY", 1, M(group_zero_copy), BOOL01, FLAG, false},
    {"skip_cascade", "NVCA_SKIP_CASCADE", 0, M(skip_cascade), PRESENT, FLAG, false},
    {"host_group", "NVCA_HOST_GROUP", 0, M(host_group), PRESENT, FLAG, false},
    {"band_map", "NVCA_BAND_MAP", 0, M(band_map), RAW, ASGIVEN, false},
    {"band", "NVCA_BAND", -1, M(band), RAW, ASGIVEN, false},
    {"host_profile", "NVCA_HOST_PROFILE", 0, M(host_profile), PRESENT, FLAG, false},
    {"sparse_ingest", "NVCA_SPARSE_INGEST", 1, M(sparse_ingest), BOOL01, FLAG, false},
    {"pyr_off", "NVCA_PYR_OFF", 0, M(pyr_off), PRESENT, FLAG, true},
    {"part_stats", "NVCA_PART_STATS", 0, M(part_stats), COUNT8, ASGIVEN, false},
    {"ingest_chunk", "NVCA_INGEST_CHUNK", 8, M(ingest_chunk), RAW, ASGIVEN, false},
    {"deep_stage", "NVCA_DEEP_STAGE", 0, M(deep_stage), ATLEAST1, POS_OR_0, true},
    {"tiles", "NVCA_TILES", 1, M(tiles), BOOL01, FLAG, true},
    {"plan_debug", "NVCA_PLAN_DEBUG", 0, M(plan_debug), PRESENT, FLAG, false},
    {"deep_lds", "NVCA_DEEP_LDS_OFF", 1, M(deep_lds), ABSENT, FLAG, true},
    {"trk_fold", "NVCA_TRK_FOLD", 1, M(trk_fold), BOOL01, FLAG, false},
    {"trk_order", "NVCA_TRK_ORDER", -1, M(trk_order), RAW, ASGIVEN, false},
    {"host_threads", "NVCA_HOST_THREADS", -1, M(host_threads), RAW, ASGIVEN, false},
    {"fb_dense", "NVCA_FB_DENSE", 1, M(fb_dense), BOOL01, FLAG, false},
    {"roi", "NVCA_ROI", 1, M(roi), BOOL01, FLAG, false},
    {"stage_order", "NVCA_STAGE_ORDER", 0, M(stage_order), BOOL01, FLAG, false},
    {"pair_max", "NVCA_PAIR_MAX", 32, M(pair_max), RAW, ASGIVEN, false},
    {"spec_pairs", "NVCA_SPEC_PAIRS", 1536, M(spec_pairs), ATLEAST1, POS_OR_1, false},
    {"quiet", "NVCA_QUIET", 0, M(quiet), PRESENT, FLAG, false},
};
struct EnvCase { const char *text; int expect; };
// the value the member must hold after read_switches() with the variable set to `text`
static std::vector<EnvCase> env_cases(Env k)
{
    switch (k) {
    case PRESENT: return {{"1", 1}, {"0", 1}, {"", 1}, {"no", 1}};
    case ABSENT: return {{"1", 0}, {"0", 0}, {"", 0}};
    case BOOL01: return {{"0", 0}, {"1", 1}, {"2", 1}, {"-1", 1}, {"", 0}, {"x", 0}};
    case RAW: return {{"0", 0}, {"1", 1}, {"-1", -1}, {"-7", -7}, {"40", 40}, {"5000", 5000}, {"", 0}};
    case ATLEAST1: return {{"0", 1}, {"-2", 1}, {"", 1}, {"1", 1}, {"7", 7}, {"768", 768}};
    case COUNT8: return {{"", 8}, {"0", 8}, {"-1", 8}, {"1", 1}, {"3", 3}, {"12", 12}};
    }
    return {};
}

int main()
{
    std::string what = "start";
    const size_t n = sizeof(rows) / sizeof(rows[0]);
    CHECK(n == 23);
    for (const Row &r : rows) unsetenv(r.env);
    unsetenv("NVCA_STAMPS_OUT");
    {   // nothing set: the defaults, which are those of a default-constructed Switches
        const Switches w = nvca::read_switches(), d;
        for (const Row &r : rows) { what = r.name; CHECK(r.member(w) == r.dflt && r.member(d) == r.dflt); }
        CHECK(w.stamps_out == nullptr);
    }
    for (const Row &r : rows)
        for (const EnvCase &c : env_cases(r.from_env)) {
            what = std::string(r.env) + "=" + c.text;
            setenv(r.env, c.text, 1);
            const Switches w = nvca::read_switches();
            CHECK(r.member(w) == c.expect);
            for (const Row &o : rows) if (&o != &r) CHECK(o.member(w) == o.dflt);       // and nothing else moved
            unsetenv(r.env);
        }
    {   // not an option: a string, the diagnostic build's
        what = "NVCA_STAMPS_OUT";
        setenv("NVCA_STAMPS_OUT", "/tmp/stamps.bin", 1);
        const Switches w = nvca::read_switches();
        CHECK(w.stamps_out && !strcmp(w.stamps_out, "/tmp/stamps.bin"));
        for (const Row &o : rows) CHECK(o.member(w) == o.dflt);
        unsetenv("NVCA_STAMPS_OUT");
        int v = 0; bool replan = false; Switches s;
        CHECK(!nvca::option_set(s, "stamps_out", 1, &replan) && !nvca::option_get(s, "stamps_out", &v));
    }
    const int values[] = {-2, -1, 0, 1, 2, 40, 5000};
    int nreplan = 0;
    for (const Row &r : rows) {
        nreplan += r.replan;
        for (int v : values) {
            what = std::string(r.name) + " <- " + std::to_string(v);
            Switches w;
            bool replan = !r.replan;
            CHECK(nvca::option_set(w, r.name, v, &replan));
            CHECK(replan == r.replan);
            const int expect = r.on_set == FLAG ? (v != 0 ? 1 : 0) : r.on_set == POS_OR_1 ? (v > 0 ? v : 1) : r.on_set == POS_OR_0 ? (v > 0 ? v : 0) : v;
            int got = 12345;
            CHECK(r.member(w) == expect);
            CHECK(nvca::option_get(w, r.name, &got) && got == expect);
            for (const Row &o : rows) if (&o != &r) CHECK(o.member(w) == o.dflt);
        }
    }
    what = "replan set";
    CHECK(nreplan == 4);
    for (const char *bad : {"", "nope", "group_zero_copy", "NVCA_BAND", "Band", "band ", "tile"}) {
        what = std::string("unknown: '") + bad + "'";
        Switches w;
        bool replan = false; int got = 12345;
        CHECK(!nvca::option_set(w, bad, 1, &replan) && !replan);
        CHECK(!nvca::option_get(w, bad, &got) && got == 12345);
        for (const Row &o : rows) CHECK(o.member(w) == o.dflt);
    }
    printf("options ok\n");
    return 0;
}
