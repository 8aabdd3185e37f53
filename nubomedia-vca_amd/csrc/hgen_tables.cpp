// hgen_tables.cpp -- the device tables of a general new-format HAAR scan (hgen_tables.h): pure host code.
#include "hgen_tables.h"
#include <cstring>

namespace nvca {

// the corners of rect (x, y, w, h) in the order p0 - p1 - p2 + p3: HaarEvaluator's CV_SUM_PTRS, or CV_TILTED_PTRS on the tilted plane
static void hgen_corners(int *off, const int *r, bool tilted, int pitch)
{
    const int x = r[0], y = r[1], w = r[2], h = r[3];
    if (!tilted) { off[0] = y * pitch + x; off[1] = y * pitch + x + w; off[2] = (y + h) * pitch + x; off[3] = (y + h) * pitch + x + w; }
    else { off[0] = y * pitch + x; off[1] = (y + h) * pitch + x - h; off[2] = (y + w) * pitch + x + w; off[3] = (y + w + h) * pitch + x + w - h; }
}

int build_hgen_tables(const HnewCascade &c, const std::vector<PyrLevel> &lv, int P, HgenTables &out, std::string &err)
{
    out = HgenTables();
    if (!c.general) { err = "internal: not a general cascade"; return NVCA_ERR_INTERNAL; }
    HnewCascade shell; shell.ow = c.ow; shell.oh = c.oh; shell.stages = c.stages;          // (the scan's tables and normrect: no weak record)
    if (int rc = build_hnew_tables(shell, lv, P, out.base, err)) return rc;
    const int TP = out.base.scan.TP;
    out.nodes.resize(c.nodes.size()); out.weak.resize(c.trees.size());
    for (size_t t = 0; t < c.trees.size(); t++) {
        const HgenTree &tr = c.trees[t];
        out.weak[t] = HgenWeakDev{tr.first_node, tr.nnodes};
        for (int j = 0; j < tr.nnodes; j++) {
            const HgenNode &n = c.nodes[(size_t)(tr.first_node + j)]; const HnewFeature &f = c.features[(size_t)n.feature];
            HgenNodeDev &d = out.nodes[(size_t)(tr.first_node + j)]; memset(&d, 0, sizeof(d));
            const bool tilted = c.tilted[(size_t)n.feature] != 0;
            for (int r = 0; r < 3; r++) {
                if (r < f.nrect) { hgen_corners(d.off + 4 * r, f.rect[r], tilted, P); hgen_corners(d.offt + 4 * r, f.rect[r], tilted, TP); }
                d.w[r] = r < f.nrect ? f.weight[r] : 0.f;
            }
            d.thr = n.threshold; d.tilted = tilted ? 1 : 0;
            const int child[2] = {n.left, n.right};
            int *enc[2] = {&d.left, &d.right};
            for (int s = 0; s < 2; s++) {
                if (child[s] > 0) { *enc[s] = tr.first_node + child[s]; d.lv[s] = 0.f; }
                else { *enc[s] = -1; d.lv[s] = c.leaves[(size_t)(tr.first_leaf - child[s])]; }
            }
        }
    }
    return NVCA_OK;
}

} // namespace nvca
