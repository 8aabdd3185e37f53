// trk_host_driver.cpp -- the tracker's buffer layout (csrc/trk_layout.h) and the pure host parts of nvca_tracker_batch_process
// (csrc/trk_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program built without any HIP include
// path: tests/test_trk_host_cpu.py hands it a manifest and checks every line it prints.  Manifest lines (ID first, then integers):
//   layout ID w h batch div                                     every offset and size of trk_layout.h
//   wide   ID fmt mem base width stride o0 o1 o2 s0 s1 s2       trk_wide_ok (fmt 0: the layout is not given to it)
//   sets   ID n (w h fmt) x n                                   trk_launch_sets
//   staged ID fmt stride w h o0 o1 o2 s0 s1 s2                  trk_staged_bytes beside yuv_extent
//   count  ID total                                             trk_component_count
//   comps  ID batch total (slot seed x y w h) x total           trk_component_lists on header + words
// One JSON line per case.
#include "trk_host.h"
#include "yuv_layout.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

using namespace nvca;

static nvca_pixel_layout read_layout(std::istream &in, int fmt)
{
    nvca_pixel_layout l{};
    l.format = fmt;
    for (int p = 0; p < 3; p++) in >> l.offset[p];
    for (int p = 0; p < 3; p++) in >> l.stride[p];
    return l;
}

static void put_json_string(const std::string &s)
{
    putchar('"');
    for (char c : s) { if (c == '"' || c == '\\') putchar('\\'); putchar(c); }
    putchar('"');
}

static void layout(const std::string &id, int w, int h, int batch, int div)
{
    printf("{\"case\": \"%s\", \"seg_per_row\": %d, \"tile_rows\": %d, \"tiles_per_slot\": %d", id.c_str(), seg_per_row(w), tile_rows(h), tiles_per_slot(w, h));
    printf(", \"tile_w\": %d, \"tile_h\": %d, \"tile_waves\": %d, \"rows\": [%d, %d, %d]", kTrkSegW, kCclTileRows, kCclTileWaves, kCclRowsDefault, kCclRowsUf, kCclRowsMax);
    // flag bytes: the first and the last index the kernels form, the counts behind them
    printf(", \"flag_first\": %zu, \"flag_last\": %zu, \"flag_second_row\": %zu, \"count_offset\": %zu, \"flag_bytes\": %zu", trk_flag_index(w, h, 0, 0, 0),
           trk_flag_index(w, h, batch - 1, h - 1, seg_per_row(w) - 1), trk_flag_index(w, h, 0, 1, 0), trk_count_offset(w, h, batch), trk_flag_bytes(w, h, batch));
    {
        std::vector<uint8_t> flags(trk_flag_bytes(w, h, batch));
        printf(", \"counts_at\": %td, \"counted\": [%d, %d, %d], \"counted_rows\": %d", (uint8_t *)segment_counts(flags.data(), w, h, batch) - flags.data(),
               (int)trk_counted_row(0), (int)trk_counted_row(kTrkCountEvery - 1), (int)trk_counted_row(kTrkCountEvery), trk_counted_rows(h));
    }
    // tile list: the parts as tile_list() carves them, for both tick parities
    printf(", \"tiles_list_offset\": %zu, \"tiles_count_offset\": [%zu, %zu], \"tiles_words\": %zu, \"tile_last\": %d, \"tile_second_row\": %d", trk_tiles_list_offset(w, h, batch),
           trk_tiles_count_offset(w, h, batch, 0), trk_tiles_count_offset(w, h, batch, 1), trk_tiles_words(w, h, batch), tile_of(w, h - 1, seg_per_row(w) - 1),
           tile_of(w, kCclTileRows, 0));
    {
        std::vector<int> tiles(trk_tiles_words(w, h, batch));
        printf(", \"tile_list\": [");
        for (int tick = 1; tick <= 2; tick++) {
            const TileList t = tile_list(tiles.data(), w, h, batch, tick);
            printf("%s[%td, %td, %td, %td, %d]", tick > 1 ? ", " : "", t.mark - tiles.data(), t.list - tiles.data(), t.cnt_now - tiles.data(), t.cnt_next - tiles.data(), t.per_slot);
        }
        printf("]");
    }
    const int cap = trk_roots_cap(w, h, batch, div);
    printf(", \"roots\": {\"entries\": %d, \"overflowed\": %d, \"error\": %d, \"error_words\": %d, \"hdr\": %d, \"cap\": %d, \"words\": %zu}", kRootsEntries, kRootsOverflowed, kRootsError,
           kRootsErrorWords, kRootsHdr, cap, trk_roots_words(cap));
    printf(", \"comp\": {\"count\": %d, \"flags\": %d, \"hdr\": %d, \"bit_overflowed\": %d, \"bit_error\": %d, \"words\": %d, \"cap\": %d, \"first\": %d, \"at\": [%zu, %zu, %zu, %zu]}}\n",
           kCompCount, kCompFlags, kCompHdr, kCompRootsOverflowed, kCompLabelError, kCompWords, kCompCap, kCompFirstRead, trk_comp_words(0), trk_comp_words(1),
           trk_comp_words(kCompFirstRead), trk_comp_words(kCompCap));
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s MANIFEST\n", argv[0]); return 2; }
    std::ifstream mf(argv[1]);
    if (!mf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(mf, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string verb, id;
        in >> verb >> id;
        if (verb == "layout") {
            int w, h, batch, div;
            in >> w >> h >> batch >> div;
            layout(id, w, h, batch, div);
        } else if (verb == "wide") {
            int fmt, mem, width, stride; unsigned long long base;
            in >> fmt >> mem >> base >> width >> stride;
            const nvca_pixel_layout l = read_layout(in, fmt);
            printf("{\"case\": \"%s\", \"wide\": %d}\n", id.c_str(), (int)trk_wide_ok(fmt, fmt == NVCA_PIX_BGR ? nullptr : &l, mem, (uintptr_t)base, stride, width));
        } else if (verb == "sets") {
            int n;
            in >> n;
            std::vector<TrkFrameKey> keys(n);
            for (TrkFrameKey &k : keys) in >> k.w >> k.h >> k.fmt;
            TrkLaunchSets sets;
            sets.member.assign(3, 77); sets.begin.assign(5, 77);       // (what an earlier call left is gone)
            trk_launch_sets(keys.data(), n, sets);
            printf("{\"case\": \"%s\", \"sets\": [", id.c_str());
            for (int s = 0; s < sets.count(); s++) {
                printf("%s[", s ? ", " : "");
                for (int k = sets.begin[s]; k < sets.begin[s + 1]; k++) printf("%s%d", k > sets.begin[s] ? ", " : "", sets.member[k]);
                printf("]");
            }
            printf("], \"members\": %zu}\n", sets.member.size());
        } else if (verb == "staged") {
            int fmt, stride, w, h;
            in >> fmt >> stride >> w >> h;
            const nvca_pixel_layout l = read_layout(in, fmt);
            printf("{\"case\": \"%s\", \"staged\": %zu, \"extent\": %zu}\n", id.c_str(), trk_staged_bytes(fmt == NVCA_PIX_BGR ? nullptr : &l, stride, w, h),
                   fmt == NVCA_PIX_BGR ? (size_t)0 : yuv_extent(l, w, h));
        } else if (verb == "count") {
            int total;
            in >> total;
            std::string err;
            const int rc = trk_component_count(total, err);
            printf("{\"case\": \"%s\", \"rc\": %d, \"err\": ", id.c_str(), rc);
            put_json_string(err);
            printf("}\n");
        } else if (verb == "comps") {
            int batch, total;
            in >> batch >> total;
            std::vector<int> words(trk_comp_words(total));             // exactly the words of `total` components: a read past them is the sanitizer's
            words[kCompCount] = total; words[kCompFlags] = 0;
            for (size_t k = kCompHdr; k < words.size(); k++) in >> words[k];
            std::vector<std::vector<nvca_rect>> lists(2, std::vector<nvca_rect>(3));      // (what an earlier launch set left is gone)
            std::string err;
            const int rc = trk_component_lists(words.data(), total, batch, lists, err);
            printf("{\"case\": \"%s\", \"rc\": %d, \"err\": ", id.c_str(), rc);
            put_json_string(err);
            printf(", \"lists\": [");
            for (size_t b = 0; rc == 0 && b < lists.size(); b++) {
                printf("%s[", b ? ", " : "");
                for (size_t k = 0; k < lists[b].size(); k++) printf("%s[%d, %d, %d, %d]", k ? ", " : "", lists[b][k].x, lists[b][k].y, lists[b][k].w, lists[b][k].h);
                printf("]");
            }
            printf("]}\n");
        } else { fprintf(stderr, "unknown manifest line: %s\n", line.c_str()); return 2; }
        if (!in) { fprintf(stderr, "short manifest line: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
