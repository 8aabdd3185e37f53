// yuv_out_driver.cpp -- the host loops of the way out in 4:2:0 (csrc/yuv_out_host.cpp: nvca_draw_shapes_yuv420 / nvca_overlay_blend_yuv420
// on host frames, and the host statement of nvca_bgr_to_yuv420) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone
// program, never loaded into Python.  It reads a manifest written by tests/test_yuv_out_san_cpu.py -- one case a line, the case table
// of tests/yuv_out_cases.py -- runs every case on a heap copy of its frame that ends with the last plane's last byte (a read or write
// past a plane's last row is a heap-buffer-overflow), and prints a checksum of the frame a case leaves.
//
//   draw    <name> <w> <h> <fmt> <off0> <off1> <off2> <st0> <st1> <st2> <frame file> <n> { kind x y w h b g r a }
//   overlay <name> <w> <h> <fmt> <off0> <off1> <off2> <st0> <st1> <st2> <frame file> <image file> <iw> <ih> <cn> <ox> <oy> <wp> <hp> <n> { x y w h }
//   convert <name> <w> <h> <fmt> <off0> <off1> <off2> <st0> <st1> <st2> <frame file> <image file> <cn> <stride>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "../../nubomedia-vca_amd/csrc/pixel_rules.h"

using namespace nvca;

// a file's bytes in a heap block of exactly that size
static std::unique_ptr<uint8_t[]> slurp(const std::string &path, size_t &n)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    n = (size_t)f.tellg();
    f.seekg(0);
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    f.read((char *)p.get(), (std::streamsize)n);
    return p;
}
static unsigned long long fnv1a(const uint8_t *p, size_t n)
{
    unsigned long long h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: yuv_out_driver <manifest>\n"); return 2; }
    std::ifstream mf(argv[1]);
    std::string line;
    while (std::getline(mf, line)) {
        std::istringstream in(line);
        std::string what, name, frame_file;
        int w, h, ystride; YuvPlanes p{};
        in >> what >> name >> w >> h >> p.fmt >> p.off_y >> p.off_u >> p.off_v >> ystride >> p.cstride >> p.vstride >> frame_file;
        if (!in) { fprintf(stderr, "bad manifest line: %s\n", line.c_str()); return 2; }
        size_t nb = 0;
        std::unique_ptr<uint8_t[]> buf = slurp(frame_file, nb);
        if (what == "draw") {
            int n; in >> n;
            std::unique_ptr<nvca_shape[]> shapes(new nvca_shape[n]);          // exactly n records (n may be 0)
            for (int i = 0; i < n; i++) {
                int c[4];
                in >> shapes[i].kind >> shapes[i].x >> shapes[i].y >> shapes[i].w >> shapes[i].h >> c[0] >> c[1] >> c[2] >> c[3];
                for (int k = 0; k < 4; k++) shapes[i].bgra[k] = (uint8_t)c[k];
            }
            draw_shapes_yuv420_host(buf.get(), w, h, ystride, p, shapes.get(), n);
        } else if (what == "overlay") {
            std::string image_file; nvca_overlay ov{}; int n;
            in >> image_file >> ov.width >> ov.height >> ov.channels >> ov.offset_x_percent >> ov.offset_y_percent >> ov.width_percent >> ov.height_percent >> n;
            size_t ni = 0;
            std::unique_ptr<uint8_t[]> img = slurp(image_file, ni);
            ov.data = img.get(); ov.stride = ov.width * ov.channels;
            if (ni != (size_t)ov.stride * ov.height) { fprintf(stderr, "image size\n"); return 2; }
            std::unique_ptr<nvca_rect[]> boxes(new nvca_rect[n]);
            for (int i = 0; i < n; i++) in >> boxes[i].x >> boxes[i].y >> boxes[i].w >> boxes[i].h;
            overlay_blend_yuv420_host(buf.get(), w, h, ystride, p, boxes.get(), n, ov);
        } else if (what == "convert") {
            std::string image_file; int cn, stride;
            in >> image_file >> cn >> stride;
            size_t ni = 0;
            std::unique_ptr<uint8_t[]> img = slurp(image_file, ni);
            if (ni != (size_t)stride * (h - 1) + (size_t)w * cn) { fprintf(stderr, "image size\n"); return 2; }
            bgr_to_yuv420_host(img.get(), w, h, stride, cn, buf.get(), ystride, p);
        } else { fprintf(stderr, "unknown case kind %s\n", what.c_str()); return 2; }
        if (!in) { fprintf(stderr, "bad manifest line: %s\n", line.c_str()); return 2; }
        printf("{\"case\": \"%s\", \"bytes\": %zu, \"fnv\": \"%016llx\"}\n", name.c_str(), nb, fnv1a(buf.get(), nb));
    }
    return 0;
}
