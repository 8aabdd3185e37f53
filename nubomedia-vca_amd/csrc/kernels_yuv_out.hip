// kernels_yuv_out.hip -- gfx950 kernels of the way out in 4:2:0: cv::cvtColor(CV_BGR2YUV_I420) into NV12 / I420 planes
// (nvca_bgr_to_yuv420, SURVEY A.14: the videoconvert behind the element, FACE/run_plugin.sh:3), and the view-* outlines and the
// image-to-overlay blend on a 4:2:0 device frame.  Their pixel rules are pixel_rules.h's, shared with the host loops
// (yuv_out_host.cpp).  All integer but the overlay's blend; HBM-bound streaming work.
#include "launch.h"

namespace nvca {

// ---- BGR -> 4:2:0, wide: a thread owns 16 pixels of two rows -- the block one row of 8 chroma samples serves.  Per row three
// 16-byte loads (48 bytes: 16 packed BGR pixels; a wave's three loads cover 3072 contiguous bytes between them) and one 16-byte
// luma store; the chroma of the strip is one 16-byte store (NV12: 8 U,V pairs) or two 8-byte stores (I420).  Units are numbered
// along the rows and on from one row pair to the next, as k_gray_yuv16's.  Wants w % 16 == 0, 3 channels, and the source, every
// plane and every stride aligned to these accesses (launch_bgr_to_yuv420 sends anything else to k_bgr_yuv_generic).
__device__ __forceinline__ int byte_of(const unsigned *d, int j) { return (d[j >> 2] >> ((j & 3) * 8)) & 255; }
template <int FMT>
__global__ __launch_bounds__(256) void k_bgr_yuv16(const uint8_t *__restrict__ src, int w, int h, int sstride,
                                                   uint8_t *__restrict__ base, int ystride, YuvPlanes p)
{
    const int upr = w >> 4;                                 // units per row pair
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (unit >= upr * (h >> 1)) return;
    const int ry = unit / upr, x = (unit - ry * upr) << 4;
    unsigned cu[2] = {0, 0}, cv[2] = {0, 0};                // the strip's 8 U and 8 V samples, from row 0's even pixels
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const uint4 *s = (const uint4 *)(src + (size_t)(2 * ry + j) * sstride + (size_t)x * 3);
        const uint4 a = s[0], b = s[1], c = s[2];
        const unsigned d[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            int Y, U, V;
            bgr_yuv(byte_of(d, 3 * k), byte_of(d, 3 * k + 1), byte_of(d, 3 * k + 2), Y, U, V);
            o[k >> 2] |= (unsigned)Y << ((k & 3) * 8);
            if (j == 0 && !(k & 1)) { cu[k >> 3] |= (unsigned)U << (((k >> 1) & 3) * 8); cv[k >> 3] |= (unsigned)V << (((k >> 1) & 3) * 8); }
        }
        *(uint4 *)(base + p.off_y + (size_t)(2 * ry + j) * ystride + x) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    if (FMT == 1) {
        unsigned uv[4];                                     // U0 V0 U1 V1 ...: bytes of cu / cv interleaved
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned u2 = (cu[i >> 1] >> ((i & 1) * 16)) & 0xffff, v2 = (cv[i >> 1] >> ((i & 1) * 16)) & 0xffff;
            uv[i] = (u2 & 255) | ((v2 & 255) << 8) | ((u2 >> 8) << 16) | ((v2 >> 8) << 24);
        }
        *(uint4 *)(base + p.off_u + (size_t)ry * p.cstride + x) = make_uint4(uv[0], uv[1], uv[2], uv[3]);
    } else {
        *(uint2 *)(base + p.off_u + (size_t)ry * p.cstride + (x >> 1)) = make_uint2(cu[0], cu[1]);
        *(uint2 *)(base + p.off_v + (size_t)ry * p.vstride + (x >> 1)) = make_uint2(cv[0], cv[1]);
    }
}

// ---- BGR / BGRA -> 4:2:0, generic: a thread per 2 x 2 block, byte accesses, any alignment, any even size
__global__ __launch_bounds__(256) void k_bgr_yuv_generic(const uint8_t *__restrict__ src, int w, int h, int sstride, int cn,
                                                         uint8_t *__restrict__ base, int ystride, YuvPlanes p)
{
    const int cx = blockIdx.x * 64 + (threadIdx.x & 63), cy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (2 * cx >= w || 2 * cy >= h) return;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int x = 2 * cx + (j & 1), y = 2 * cy + (j >> 1);
        const uint8_t *s = src + (size_t)y * sstride + (size_t)x * cn;
        int Y, U, V;
        bgr_yuv(s[0], s[1], s[2], Y, U, V);
        *yuv_luma_at(base, p, ystride, x, y) = (uint8_t)Y;
        if (j == 0) { *yuv_u_at(base, p, cx, cy) = (uint8_t)U; *yuv_v_at(base, p, cx, cy) = (uint8_t)V; }
    }
}

bool launch_bgr_to_yuv420(hipStream_t st, const uint8_t *src, int w, int h, int sstride, int cn, uint8_t *base, int ystride, const YuvPlanes &p, bool aligned16)
{
    if (aligned16 && cn == 3 && !(w & 15)) {
        const int units = (w >> 4) * (h >> 1);
        if (p.fmt == 1) NVCA_LAUNCH(k_bgr_yuv16<1>, dim3((units + 255) / 256), dim3(256), 0, st, src, w, h, sstride, base, ystride, p);
        else            NVCA_LAUNCH(k_bgr_yuv16<2>, dim3((units + 255) / 256), dim3(256), 0, st, src, w, h, sstride, base, ystride, p);
        return true;
    }
    NVCA_LAUNCH(k_bgr_yuv_generic, dim3((w / 2 + 63) / 64, (h / 2 + 3) / 4), dim3(256), 0, st, src, w, h, sstride, cn, base, ystride, p);
    return false;
}

// ---- view-* outlines on a 4:2:0 device frame: a thread per chroma block of the shapes' common bounding box (even-aligned, clipped:
// blocks [cx0, cx1] x [cy0, cy1]); for each of its four pixels the last shape of the list that covers it leaves Y(colour), and
// the block's top-left pixel its (U, V) too.  uv2: the NV12 pair takes one 2-byte store (the U,V plane and its stride are even).
__global__ __launch_bounds__(256) void k_draw_shapes_yuv(uint8_t *__restrict__ base, int ystride, YuvPlanes p, const nvca_shape *__restrict__ shapes, int n,
                                                         int cx0, int cy0, int cx1, int cy1, int uv2)
{
    extern __shared__ nvca_shape sh_s[];
    for (int i = threadIdx.x; i < n; i += 256) sh_s[i] = shapes[i];
    __syncthreads();
    const int cx = cx0 + blockIdx.x * 64 + (threadIdx.x & 63), cy = cy0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (cx > cx1 || cy > cy1) return;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int x = 2 * cx + (j & 1), y = 2 * cy + (j >> 1);
        for (int i = n - 1; i >= 0; i--)
            if (shape_covers(sh_s[i], x, y)) {
                int Y, U, V;
                bgr_yuv(sh_s[i].bgra[0], sh_s[i].bgra[1], sh_s[i].bgra[2], Y, U, V);
                *yuv_luma_at(base, p, ystride, x, y) = (uint8_t)Y;
                if (j == 0) {
                    if (uv2) *(unsigned short *)yuv_u_at(base, p, cx, cy) = (unsigned short)(U | (V << 8));
                    else { *yuv_u_at(base, p, cx, cy) = (uint8_t)U; *yuv_v_at(base, p, cx, cy) = (uint8_t)V; }
                }
                break;
            }
    }
}
void launch_draw_shapes_yuv(hipStream_t st, uint8_t *base, int ystride, const YuvPlanes &p, const nvca_shape *d_shapes, int n,
                            int cx0, int cy0, int cx1, int cy1, bool uv2)
{
    dim3 grid((cx1 - cx0 + 64) / 64, (cy1 - cy0 + 4) / 4, 1);
    NVCA_LAUNCH(k_draw_shapes_yuv, grid, dim3(256), (size_t)n * sizeof(nvca_shape), st, base, ystride, p, d_shapes, n, cx0, cy0, cx1, cy1, uv2 ? 1 : 0);
}

// ---- image-to-overlay on a 4:2:0 device frame, one box: a thread per chroma block of the placed image inside the frame (blocks
// [cx0, cx1] x [cy0, cy1]).  overlay_block_yuv reads the block's chroma and Y bytes, then writes them; no thread reads a sample
// another thread of the launch writes.
__global__ __launch_bounds__(256) void k_overlay_yuv(uint8_t *__restrict__ base, int W, int H, int ystride, YuvPlanes yp, OverlayPlace p, OverlayImage o,
                                                     int cx0, int cy0, int cx1, int cy1)
{
    const int cx = cx0 + blockIdx.x * 64 + (threadIdx.x & 63), cy = cy0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (cx > cx1 || cy > cy1) return;
    overlay_block_yuv(base, W, H, ystride, yp, p, o, cx, cy);
}
void launch_overlay_yuv(hipStream_t st, uint8_t *base, int W, int H, int ystride, const YuvPlanes &yp, const OverlayPlace &p, const OverlayImage &o,
                        int cx0, int cy0, int cx1, int cy1)
{
    dim3 grid((cx1 - cx0 + 64) / 64, (cy1 - cy0 + 4) / 4, 1);
    NVCA_LAUNCH(k_overlay_yuv, grid, dim3(256), 0, st, base, W, H, ystride, yp, p, o, cx0, cy0, cx1, cy1);
}

} // namespace nvca
