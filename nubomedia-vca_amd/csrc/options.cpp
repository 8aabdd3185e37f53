// options.cpp -- the context's switches (struct Switches, switches.h): ONE table, a row per switch in the order of the
// struct, that says how the environment sets its process default and how nvca_ctx_set_option / _get_option reach it.  Pure
// host logic, no HIP calls.  nubovca.h's option list and DESIGN.md's appendix follow this table (tests/test_abi_cpu.py).
#include "switches.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>

namespace nvca {
namespace {

// how the environment variable becomes the process default (unset: the member keeps its initialiser in struct Switches)
enum EnvRule {
    kPresent,        // set to ANY value, "0" included: true
    kAbsent,         // set to any value: false (the variable names the inverse of the option)
    kBool,           // atoi(value) != 0
    kInt,            // atoi(value)
    kAtLeast1,       // max(1, atoi(value))
    kCountOr8,       // atoi(value); anything <= 0 (also ""): 8
};
// how nvca_ctx_set_option stores a value in an int member (a bool member takes value != 0)
enum SetRule { kAsGiven, kPositiveOr1, kPositiveOr0 };

struct Option {
    const char *name, *env;
    bool Switches::*flag;          // exactly one of flag / num names the member
    int Switches::*num;
    EnvRule from_env;
    SetRule on_set;
    bool replan;                   // changing it drops the context's cached plans
};
constexpr Option flag_opt(const char *name, const char *env, bool Switches::*m, EnvRule r, bool replan = false) { return {name, env, m, nullptr, r, kAsGiven, replan}; }
constexpr Option num_opt(const char *name, const char *env, int Switches::*m, EnvRule r, SetRule s = kAsGiven, bool replan = false) { return {name, env, nullptr, m, r, s, replan}; }

const Option kOptions[] = {
    flag_opt("group_zerocopy", "NVCA_GROUP_ZEROCOPY", &Switches::group_zero_copy, kBool),
    flag_opt("skip_cascade", "NVCA_SKIP_CASCADE", &Switches::skip_cascade, kPresent),
    flag_opt("host_group", "NVCA_HOST_GROUP", &Switches::host_group, kPresent),
    num_opt("band_map", "NVCA_BAND_MAP", &Switches::band_map, kInt),
    num_opt("band", "NVCA_BAND", &Switches::band, kInt),
    flag_opt("host_profile", "NVCA_HOST_PROFILE", &Switches::host_profile, kPresent),
    flag_opt("sparse_ingest", "NVCA_SPARSE_INGEST", &Switches::sparse_ingest, kBool),
    flag_opt("pyr_off", "NVCA_PYR_OFF", &Switches::pyr_off, kPresent, true),
    num_opt("part_stats", "NVCA_PART_STATS", &Switches::part_stats, kCountOr8),
    num_opt("ingest_chunk", "NVCA_INGEST_CHUNK", &Switches::ingest_chunk, kInt),
    num_opt("deep_stage", "NVCA_DEEP_STAGE", &Switches::deep_stage, kAtLeast1, kPositiveOr0, true),
    flag_opt("tiles", "NVCA_TILES", &Switches::tiles, kBool, true),
    flag_opt("plan_debug", "NVCA_PLAN_DEBUG", &Switches::plan_debug, kPresent),
    flag_opt("deep_lds", "NVCA_DEEP_LDS_OFF", &Switches::deep_lds, kAbsent, true),
    flag_opt("trk_fold", "NVCA_TRK_FOLD", &Switches::trk_fold, kBool),
    num_opt("trk_order", "NVCA_TRK_ORDER", &Switches::trk_order, kInt),
    num_opt("host_threads", "NVCA_HOST_THREADS", &Switches::host_threads, kInt),
    flag_opt("fb_dense", "NVCA_FB_DENSE", &Switches::fb_dense, kBool),
    flag_opt("roi", "NVCA_ROI", &Switches::roi, kBool),
    flag_opt("stage_order", "NVCA_STAGE_ORDER", &Switches::stage_order, kBool),
    num_opt("pair_max", "NVCA_PAIR_MAX", &Switches::pair_max, kInt),
    num_opt("spec_pairs", "NVCA_SPEC_PAIRS", &Switches::spec_pairs, kAtLeast1, kPositiveOr1),
    flag_opt("quiet", "NVCA_QUIET", &Switches::quiet, kPresent),
};

const Option *find_option(const char *name)
{
    for (const Option &o : kOptions)
        if (!strcmp(o.name, name)) return &o;
    return nullptr;
}

} // namespace

Switches read_switches()
{
    Switches w;
    for (const Option &o : kOptions) {
        const char *e = getenv(o.env);
        if (!e) continue;
        const int v = atoi(e);
        switch (o.from_env) {
        case kPresent: w.*o.flag = true; break;
        case kAbsent: w.*o.flag = false; break;
        case kBool: w.*o.flag = v != 0; break;
        case kInt: w.*o.num = v; break;
        case kAtLeast1: w.*o.num = std::max(1, v); break;
        case kCountOr8: w.*o.num = v > 0 ? v : 8; break;
        }
    }
    w.stamps_out = getenv("NVCA_STAMPS_OUT");       // not an option: a string, diagnostic build only
    return w;
}

bool option_set(Switches &w, const char *name, int value, bool *replan)
{
    const Option *o = find_option(name);
    if (!o) return false;
    if (o->flag) w.*o->flag = value != 0;
    else w.*o->num = o->on_set == kPositiveOr1 ? (value > 0 ? value : 1) : o->on_set == kPositiveOr0 ? (value > 0 ? value : 0) : value;
    *replan = o->replan;
    return true;
}

bool option_get(const Switches &w, const char *name, int *value)
{
    const Option *o = find_option(name);
    if (!o) return false;
    *value = o->flag ? (int)(w.*o->flag) : w.*o->num;
    return true;
}

} // namespace nvca
