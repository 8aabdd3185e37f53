// lbp_tables.cpp -- the device tables of a new-format LBP scan (lbp_tables.h): pure host code.
#include "lbp_tables.h"
#include "host_math.h"
#include <algorithm>
#include <cstring>

namespace nvca {

// what depends on the window, the stages' shape and the levels alone
int build_scan_tables(int ow, int oh, const std::vector<LbpStage> &stages, const std::vector<PyrLevel> &lv, int P, LbpTables &out, std::string &err)
{
    out = LbpTables();
    // the evaluator's level records: each level's grid, and where its pass bits and scan rows lie among all levels'
    size_t mx = 1, my = 1;
    for (const PyrLevel &L : lv) {
        LbpLevelDev d; memset(&d, 0, sizeof(d));
        d.plane_off = L.plane_off; d.szw = L.szw; d.szh = L.szh; d.step = level_step(L.f);
        d.nx = level_positions(L.szw, ow, d.step); d.ny = level_positions(L.szh, oh, d.step);
        d.wpr = (d.nx + kLbpTileW - 1) / kLbpTileW; d.bit_off = (int)out.bit_words; d.row_first = out.nrows;
        out.bit_words += (size_t)d.wpr * d.ny; out.nrows += d.ny; out.positions += (size_t)d.nx * d.ny;
        mx = std::max(mx, (size_t)d.nx); my = std::max(my, (size_t)d.ny);
        out.levels.push_back(d);
        // the level as k_group reads it: a candidate (level, gy, gx) is Rect(cvRound(gx * step * f), cvRound(gy * step * f), winw, winh)
        // (DetectPlan::hit_rect's arithmetic on the level's scan grid), the rounded coordinates in the position table
        ScaleRec g; memset(&g, 0, sizeof(g));
        g.winw = L.winw; g.winh = L.winh; g.plane_off = L.plane_off; g.pitch = P; g.endX = d.nx; g.endY = d.ny; g.factor = L.f;
        g.xpos_off = (int)out.gpos.size();
        for (int gx = 0; gx < d.nx; gx++) out.gpos.push_back(cv_round(gx * d.step * L.f));
        g.ypos_off = (int)out.gpos.size();
        for (int gy = 0; gy < d.ny; gy++) out.gpos.push_back(cv_round(gy * d.step * L.f));
        out.gscales.push_back(g);
    }
    int bx, by, bs;
    candidate_key_bits(mx, my, lv.size(), &bx, &by, &bs);
    if (bx + by + bs > 32 || out.bit_words > (1u << 30) || out.positions > (1u << 30)) { err = "scan too large for the candidate key (levels x rows x columns of windows beyond 2^32)"; return NVCA_ERR_ARG; }
    out.key_sy = bx; out.key_ss = bx + by;
    for (size_t li = 0; li < out.levels.size(); li++)
        for (int ty = 0; ty * kLbpTileH < out.levels[li].ny; ty++)
            for (int tx = 0; tx < out.levels[li].wpr; tx++) out.tiles.push_back(LbpTile{(int)li, tx, ty, 0});
    out.TP = lbp_tile_pitch(ow);
    for (const LbpStage &st : stages) out.stages.push_back(LbpStageDev{st.first, st.count, st.threshold, 0});
    out.tile_stages = std::min((int)out.stages.size(), 3);          // at LDS speed while most windows are alive; later stages see scattered survivors
    // the stage-0 tile at step 2 (the larger one); a window too large for 64 KiB of LDS gathers from the plane instead
    const size_t lds = (size_t)out.TP * lbp_tile_rows(oh, 2) * sizeof(int);
    out.lds = lds <= 64 * 1024 ? (int)lds : 0;
    return NVCA_OK;
}

int build_lbp_tables(const LbpCascade &c, const std::vector<PyrLevel> &lv, int P, LbpTables &out, std::string &err)
{
    if (int rc = build_scan_tables(c.ow, c.oh, c.stages, lv, P, out, err)) return rc;
    out.gweak.resize(c.weak.size()); out.tweak.resize(c.weak.size());
    for (size_t i = 0; i < c.weak.size(); i++) {
        const LbpWeak &w = c.weak[i]; const LbpFeature &f = c.features[(size_t)w.feature];
        for (std::vector<LbpWeakDev> *tab : {&out.gweak, &out.tweak}) {
            LbpWeakDev &d = (*tab)[i]; memset(&d, 0, sizeof(d));
            const int pitch = tab == &out.gweak ? P : out.TP;
            for (int r = 0; r < 4; r++)
                for (int q = 0; q < 4; q++) d.off[r * 4 + q] = (f.y + r * f.h) * pitch + f.x + q * f.w;
            memcpy(d.subset, w.subset, sizeof(d.subset)); d.leaf[0] = w.leaf[0]; d.leaf[1] = w.leaf[1];
        }
    }
    return NVCA_OK;
}

} // namespace nvca
