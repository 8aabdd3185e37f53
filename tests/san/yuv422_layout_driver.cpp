// yuv422_layout_driver.cpp -- the pure host side of the packed 4:2:2 ingest (csrc/yuv_layout.h, csrc/pixel_rules.h's byte positions,
// csrc/trk_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program built without any HIP include path:
// tests/test_yuv422_layout_san_cpu.py hands it a manifest and checks every line it prints.  Manifest lines (ID first, then integers):
//   pos    ID fmt                                               yuv422_pos: where Y0, U and V lie in a pair's four bytes
//   rules  ID fmt w h o0 o1 o2 s0 s1 s2                         yuv_layout_fault, planes, rows, row bytes, extent, yuv_layout_aligned16
//   wide   ID fmt mem base width stride o0 o1 o2 s0 s1 s2       trk_wide_ok
//   staged ID fmt stride w h o0 o1 o2 s0 s1 s2                  trk_staged_bytes beside yuv_extent
//   copy   ID fmt w h o0 s0 first period run count              the staged copy of a host frame: count 0 = the whole plane (yuv_plane_bytes
//                                                               from offset[0]), else the row runs of row_run_pieces -- from a source buffer
//                                                               of EXACTLY yuv_extent bytes into a zeroed one of the same size (a read or
//                                                               write past the last pixel is the sanitizer's); prints the copy's checksum
// One JSON line per case.
#include "trk_host.h"
#include "yuv_layout.h"
#include "pixel_rules.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace nvca;

static nvca_pixel_layout read_layout(std::istream &in, int fmt)
{
    nvca_pixel_layout l{};
    l.format = fmt;
    for (int p = 0; p < 3; p++) in >> l.offset[p];
    for (int p = 0; p < 3; p++) in >> l.stride[p];
    return l;
}

static unsigned long long fnv1a(const uint8_t *p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
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
        if (verb == "pos") {
            int fmt;
            in >> fmt;
            const Yuv422Pos q = yuv422_pos(fmt);
            printf("{\"case\": \"%s\", \"pos\": [%d, %d, %d]}\n", id.c_str(), q.y0, q.u, q.v);
        } else if (verb == "rules") {
            int fmt, w, h;
            in >> fmt >> w >> h;
            const nvca_pixel_layout l = read_layout(in, fmt);
            const char *fault = yuv_layout_fault(l, w, h);
            printf("{\"case\": \"%s\", \"fault\": \"%s\"", id.c_str(), fault ? fault : "");
            if (!fault) printf(", \"planes\": %d, \"rows\": %zu, \"row_bytes\": %zu, \"extent\": %zu, \"aligned16\": %d", yuv_planes_of(l), yuv_plane_rows(0, h),
                               yuv_plane_row_bytes(l, 0, w), yuv_extent(l, w, h), (int)yuv_layout_aligned16(l));
            printf("}\n");
        } else if (verb == "wide") {
            int fmt, mem, width, stride; unsigned long long base;
            in >> fmt >> mem >> base >> width >> stride;
            const nvca_pixel_layout l = read_layout(in, fmt);
            printf("{\"case\": \"%s\", \"wide\": %d}\n", id.c_str(), (int)trk_wide_ok(fmt, &l, mem, (uintptr_t)base, stride, width));
        } else if (verb == "staged") {
            int fmt, stride, w, h;
            in >> fmt >> stride >> w >> h;
            const nvca_pixel_layout l = read_layout(in, fmt);
            printf("{\"case\": \"%s\", \"staged\": %zu, \"extent\": %zu}\n", id.c_str(), trk_staged_bytes(&l, stride, w, h), yuv_extent(l, w, h));
        } else if (verb == "copy") {
            int fmt, w, h; size_t first, period, run, count;
            nvca_pixel_layout l{};
            in >> fmt >> w >> h >> l.offset[0] >> l.stride[0] >> first >> period >> run >> count;
            l.format = fmt;
            if (yuv_layout_fault(l, w, h)) { fprintf(stderr, "bad layout: %s\n", line.c_str()); return 2; }
            const size_t n = yuv_extent(l, w, h);
            uint8_t *src = (uint8_t *)malloc(n), *dst = (uint8_t *)malloc(n);          // exactly the extent: nothing behind the last pixel
            for (size_t i = 0; i < n; i++) { src[i] = (uint8_t)(i * 131 + 7); dst[i] = 0; }
            size_t copied = 0;
            const uint8_t *sp = src + l.offset[0];
            uint8_t *dp = dst + l.offset[0];
            if (count == 0) { copied = yuv_plane_bytes(l, 0, w, h); memcpy(dp, sp, copied); }
            else {
                RowPiece pc[2];
                const int np = row_run_pieces((size_t)l.stride[0], yuv_plane_row_bytes(l, 0, w), yuv_plane_rows(0, h), first, period, run, count, pc);
                for (int k = 0; k < np; k++)
                    for (size_t r = 0; r < pc[k].n; r++) { memcpy(dp + pc[k].off + r * pc[k].pitch, sp + pc[k].off + r * pc[k].pitch, pc[k].width); copied += pc[k].width; }
            }
            printf("{\"case\": \"%s\", \"bytes\": %zu, \"copied\": %zu, \"fnv\": \"%016llx\"}\n", id.c_str(), n, copied, fnv1a(dst, n));
            free(src); free(dst);
        } else { fprintf(stderr, "unknown manifest line: %s\n", line.c_str()); return 2; }
        if (!in) { fprintf(stderr, "short manifest line: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
