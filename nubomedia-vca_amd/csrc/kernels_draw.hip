// kernels_draw.hip -- gfx950 kernels that draw on a device frame: the image-to-overlay blend
// (kms_face_detect_display_detections_overlay_img, FACE/kmsfacedetect.cpp:427-502) and the view-* outlines.  Their pixel rules
// are pixel_rules.h's, shared with the host loops.
#include "launch.h"

namespace nvca {

// ---- image-to-overlay on a device frame: one thread per pixel of the scaled overlay image of one box
__global__ __launch_bounds__(256) void k_overlay(uint8_t *__restrict__ frame, int W, int H, int stride, OverlayPlace p, OverlayImage o)
{
    const int w = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
    if (w >= p.w || h >= p.h || w + p.x < 0 || w + p.x >= W || h + p.y < 0 || h + p.y >= H) return;
    int v[4] = {0, 0, 0, 0};
    for (int k = 0; k < o.cn; k++) v[k] = resize_sample_cn(o.img, o.ih, o.istride, o.cn, o.tab, w, h, k);
    overlay_pixel(frame + (size_t)(h + p.y) * stride + (size_t)(w + p.x) * 3, v, o.cn);
}
void launch_overlay(hipStream_t st, uint8_t *frame, int W, int H, int stride, const OverlayPlace &p, const OverlayImage &o)
{
    NVCA_LAUNCH(k_overlay, dim3((p.w + 255) / 256, p.h), dim3(256), 0, st, frame, W, H, stride, p, o);
}

// ---- view-* outlines on a device frame: a thread per pixel of the shapes' common bounding box; the last shape of the list
// that covers the pixel colours it (= the shapes drawn one after the other)
__global__ __launch_bounds__(256) void k_draw_shapes(uint8_t *__restrict__ data, int w, int h, int stride, int channels,
                                                     const nvca_shape *__restrict__ shapes, int n, int bx0, int by0, int bx1, int by1)
{
    extern __shared__ nvca_shape sh_s[];
    for (int i = threadIdx.x; i < n; i += 256) sh_s[i] = shapes[i];
    __syncthreads();
    const int x = bx0 + blockIdx.x * 64 + (threadIdx.x & 63), y = by0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x > bx1 || y > by1 || x >= w || y >= h) return;
    for (int i = n - 1; i >= 0; i--)
        if (shape_covers(sh_s[i], x, y)) {
            uint8_t *p = data + (size_t)y * stride + (size_t)x * channels;
            for (int k = 0; k < channels; k++) p[k] = sh_s[i].bgra[k];
            return;
        }
}
void launch_draw_shapes(hipStream_t st, uint8_t *data, int w, int h, int stride, int channels, const nvca_shape *d_shapes, int n,
                        int bx0, int by0, int bx1, int by1)
{
    dim3 grid((bx1 - bx0 + 64) / 64, (by1 - by0 + 4) / 4, 1);
    NVCA_LAUNCH(k_draw_shapes, grid, dim3(256), (size_t)n * sizeof(nvca_shape), st, data, w, h, stride, channels, d_shapes, n, bx0, by0, bx1, by1);
}

} // namespace nvca
