// tile_geom_driver.cpp -- test infrastructure (never shipped): builds a detection plan with the product's plan.cpp on the CPU and
// prints the tile geometry of every scale as JSON lines, for tests/test_tile_geometry_cpu.py (the LDS budget of the tile kernels
// and the tile sides the plan gives each scale; "xs" / "ys": the first window column / row of every tile column / row of the scale's
// grid, for tests/prefix_cascades.py, which sorts raw candidates into tile cells).  Like tests/san/san_driver.cpp it links no HIP library: the few runtime calls
// of plan.cpp get host doubles, a "device" buffer is a malloc'd block, nothing runs a kernel.
//
//   tile_geom_driver <cascade.xml> <cols> <rows> <scaleFactor> <minw> <minh>
#include "../../nubomedia-vca_amd/csrc/plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
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

int main(int argc, char **argv)
{
    if (argc < 7) { fprintf(stderr, "usage: tile_geom_driver <xml> <cols> <rows> <scaleFactor> <minw> <minh>\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::stringstream ss; ss << f.rdbuf();
    const std::string xml = ss.str();
    const int cols = atoi(argv[2]), rows = atoi(argv[3]), minw = atoi(argv[5]), minh = atoi(argv[6]);
    const double sf = atof(argv[4]);
    nvca_ctx ctx;
    nvca_cascade casc; casc.ctx = &ctx;
    std::string err;
    if (parse_cascade_xml(xml.data(), xml.size(), casc.c, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    casc.c.uid = ctx.next_uid++;
    const int pitch = (cols + 1 + 7) / 8 * 8;
    DetectPlan dp;
    if (int rc = dp.build_scale_cascade(&ctx, casc.c, cols, rows, pitch, sf, minw, minh, cols, rows, err)) { fprintf(stderr, "plan: %d %s\n", rc, err.c_str()); return 1; }
    printf("{\"tile_win\": %d, \"tile_rows\": %d, \"tile_threads\": %d, \"lds_budget\": %d, \"lds_fixed\": %d, \"tile_lds\": %d, "
           "\"deep_stage\": %d, \"stages\": %zu, \"tiles\": %zu, \"bands\": %zu, \"strips\": %zu}\n",
           kTileWin, kTileRows, kTileThreads, kTileLdsBudget, tile_lds_fixed(), dp.tile_lds, dp.deep_stage, dp.stages.size(),
           dp.tiles.size(), dp.bands.size(), dp.strips.size());
    for (size_t s = 0; s < dp.scales.size(); s++) {
        int side = 0, th = 0, ncol = 0, nrow = 0, bytes = 0;
        std::set<int> xs, ys;
        size_t cells = 0;
        for (const TileRec &t : dp.tiles) {
            if (t.scale != (int)s) continue;
            xs.insert(t.ix0); ys.insert(t.iy0); cells++;
            side = std::max(side, t.nx); th = std::max(th, t.ny);
            ncol = std::max(ncol, t.ncol); nrow = std::max(nrow, t.nrow);
            bytes = std::max(bytes, tile_lds_bytes(t.ncol, t.nrow, t.span_x, t.span_y));
        }
        if (cells != xs.size() * ys.size()) { fprintf(stderr, "scale %zu: %zu tiles are no %zu x %zu grid\n", s, cells, xs.size(), ys.size()); return 1; }
        printf("{\"scale\": %zu, \"factor\": %.17g, \"window\": [%d, %d], \"windows\": [%d, %d], \"tile\": [%d, %d], \"samples\": [%d, %d], \"bytes\": %d, \"xs\": [", s,
               dp.scales[s].factor, dp.scales[s].winw, dp.scales[s].winh, dp.scales[s].endX, dp.scales[s].endY, side, th, ncol, nrow, bytes);
        const char *sep = "";
        for (int v : xs) { printf("%s%d", sep, v); sep = ", "; }
        printf("], \"ys\": [");
        sep = "";
        for (int v : ys) { printf("%s%d", sep, v); sep = ", "; }
        printf("]}\n");
    }
    return 0;
}
