// trk_host.cpp -- the pure host parts of nvca_tracker_batch_process (trk_host.h).  No HIP header.
#include "trk_host.h"
#include "host_math.h"
#include "yuv_layout.h"
#include <algorithm>
#include <utility>

namespace nvca {

void trk_launch_sets(const TrkFrameKey *keys, int n, TrkLaunchSets &sets)
{
    sets.member.clear(); sets.begin.assign(1, 0);
    sets.member.reserve(n);
    std::vector<char> done(n, 0);
    for (int i0 = 0; i0 < n; i0++) {
        if (done[i0]) continue;
        const TrkFrameKey k = keys[i0];
        for (int j = i0; j < n; j++)
            if (!done[j] && keys[j].w == k.w && keys[j].h == k.h && keys[j].fmt == k.fmt) { sets.member.push_back(j); done[j] = 1; }
        sets.begin.push_back((int)sets.member.size());
    }
}

bool trk_wide_ok(int fmt, const nvca_pixel_layout *layout, int mem, uintptr_t base, int stride, int width)
{
    if (width % 4) return false;
    if (mem != NVCA_MEM_DEVICE) base = 0;
    if (fmt == NVCA_PIX_BGR) return !(stride & 15) && !(base & 15);
    if (yuv_is_422(fmt)) return !((base + layout->offset[0]) & 7) && !(layout->stride[0] & 7);       // k_trk_pixel_yuv422x4: 8-byte loads of the one plane
    const size_t cmask = fmt == NVCA_PIX_NV12 ? 7 : 3;
    if (((base + layout->offset[0]) & 7) || (layout->stride[0] & 7) || ((base + layout->offset[1]) & cmask) || ((size_t)layout->stride[1] & cmask)) return false;
    return !(fmt == NVCA_PIX_I420 && (((base + layout->offset[2]) & 3) || (layout->stride[2] & 3)));
}

size_t trk_staged_bytes(const nvca_pixel_layout *yuv, int stride, int w, int h)
{
    return round_up(yuv ? yuv_extent(*yuv, w, h) : (size_t)stride * h, 256);
}

int trk_component_count(int total, std::string &err)
{
    if (total < 0) { err = "internal: negative component count"; return NVCA_ERR_INTERNAL; }
    if (total > kCompCap) { err = "tracker: more motion components than the list holds"; return NVCA_ERR_OVERFLOW; }
    return NVCA_OK;
}

int trk_component_lists(const int *words, int total, int batch, std::vector<std::vector<nvca_rect>> &lists, std::string &err)
{
    lists.assign(batch, std::vector<nvca_rect>());
    // the components slot by slot (a counting pass, then each at its slot's cursor), every slot's then by seed: a component's first seed is a
    // pixel of its own, so seeds differ inside a slot
    std::vector<int> at(batch + 1, 0);
    for (int k = 0; k < total; k++) {
        const int slot = words[trk_comp_words(k)];
        if (slot < 0 || slot >= batch) { err = "internal: motion component of an unknown slot (device result rejected)"; return NVCA_ERR_INTERNAL; }
        at[slot + 1]++;
    }
    for (int b = 0; b < batch; b++) at[b + 1] += at[b];
    std::vector<std::pair<int, int>> keyed(total);          // (seed, component)
    for (int k = 0; k < total; k++) { const int *o = words + trk_comp_words(k); keyed[at[o[0]]++] = {o[1], k}; }
    for (int b = 0; b < batch; b++) {                       // at[b] is now where slot b ends
        const int s = b ? at[b - 1] : 0, e = at[b];
        std::sort(keyed.begin() + s, keyed.begin() + e);
        lists[b].reserve(e - s);
        for (int i = s; i < e; i++) { const int *o = words + trk_comp_words(keyed[i].second); lists[b].push_back(nvca_rect{o[2], o[3], o[4], o[5]}); }
    }
    return NVCA_OK;
}

} // namespace nvca
