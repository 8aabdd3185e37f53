// kernels_gray.hip -- gfx950 kernels for the colour conversion and the resizes in front of the cascade: cv::resize +
// cv::cvtColor as the reference calls them (FACE/kmsfacedetect.cpp:805-811), with the histogram of the cv::equalizeHist that
// follows; the working images of the part detectors and the levels of a CV_HAAR_SCALE_IMAGE pyramid.  All integer;
// HBM-bound streaming work.  Every kernel that resizes takes its geometry as a ResizeView and calls the one statement of
// cv::resize's 8-bit rule, resize_sample (pixel_rules.h), with a tap of its own: a packed pixel, a gray byte (plain or through the
// LDS LUT), gray_of of a BGR pixel, yuv_gray / yuv_bgr of a 4:2:0 pixel.  k_gray_fast4 and k_gray_yuv16, the full-resolution
// paths, do not resize.
#include "launch.h"
#include "pre_device.h"
#include "yuv_device.h"

namespace nvca {

// ---- K1 generic: one output pixel per thread, any resize mode, any alignment: cv::resize on the packed frame, then BGR2GRAY
__global__ __launch_bounds__(256) void k_gray_generic(
    const uint8_t *const *__restrict__ srcs, PreGeom g, ResizeView t,
    uint8_t *__restrict__ gray, unsigned *__restrict__ hist)
{
    __shared__ unsigned lh[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, slot = blockIdx.z;
    for (int i = tid; i < 1024; i += 256) (&lh[0][0])[i] = 0;
    __syncthreads();
    const uint8_t *src = srcs[slot];
    const int cn = g.cn;
    const int x = blockIdx.x * 256 + tid;
    uint8_t *grow = gray + (size_t)slot * g.gray_slot;
    auto tap = [&](int r, int c, int *p) {
        const uint8_t *s = src + (size_t)r * g.sstride + (size_t)c * cn;
        p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
    };
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y >= g.h) break;
        if (x < g.w) {
            int c[3];
            resize_sample<3>(tap, g.sh, t, x, y, c);
            const int v = gray_of(c[0] & 255, c[1] & 255, c[2] & 255);
            grow[(size_t)y * g.gpitch + x] = (uint8_t)v;
            if (hist) atomicAdd(&lh[wave][v], 1u);
        }
    }
    if (hist) hist_flush(lh, hist + slot * 256, tid);
}

// ---- K1 fast path: identity geometry, rows and base 4-byte aligned: 4 pixels per thread.
template <int CN>
__global__ __launch_bounds__(256) void k_gray_fast4(
    const uint8_t *const *__restrict__ srcs, PreGeom g, uint8_t *__restrict__ gray,
    unsigned *__restrict__ hist)
{
    __shared__ unsigned lh[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, slot = blockIdx.z;
    for (int i = tid; i < 1024; i += 256) (&lh[0][0])[i] = 0;
    __syncthreads();
    const uint8_t *src = srcs[slot];
    const int x4 = (blockIdx.x * 256 + tid) * 4;
    uint8_t *grow = gray + (size_t)slot * g.gray_slot;
    if (x4 < g.w) {
        for (int ry = 0; ry < kGrayRows; ry++) {
            const int y = blockIdx.y * kGrayRows + ry;
            if (y >= g.h) break;
            const unsigned *s = (const unsigned *)(src + (size_t)y * g.sstride + (size_t)x4 * CN);
            int v[4];
            if (x4 + 4 <= g.w) {
                if (CN == 3) {
                    const unsigned d0 = s[0], d1 = s[1], d2 = s[2];
                    v[0] = gray_of(d0 & 255, (d0 >> 8) & 255, (d0 >> 16) & 255);
                    v[1] = gray_of(d0 >> 24, d1 & 255, (d1 >> 8) & 255);
                    v[2] = gray_of((d1 >> 16) & 255, d1 >> 24, d2 & 255);
                    v[3] = gray_of((d2 >> 8) & 255, (d2 >> 16) & 255, d2 >> 24);
                } else {
                    const uint4 d = *(const uint4 *)s;
                    v[0] = gray_of(d.x & 255, (d.x >> 8) & 255, (d.x >> 16) & 255);
                    v[1] = gray_of(d.y & 255, (d.y >> 8) & 255, (d.y >> 16) & 255);
                    v[2] = gray_of(d.z & 255, (d.z >> 8) & 255, (d.z >> 16) & 255);
                    v[3] = gray_of(d.w & 255, (d.w >> 8) & 255, (d.w >> 16) & 255);
                }
                *(unsigned *)(grow + (size_t)y * g.gpitch + x4) =
                    (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
                if (hist) {
                    atomicAdd(&lh[wave][v[0]], 1u); atomicAdd(&lh[wave][v[1]], 1u);
                    atomicAdd(&lh[wave][v[2]], 1u); atomicAdd(&lh[wave][v[3]], 1u);
                }
            } else {
                const uint8_t *sb = (const uint8_t *)s;
                for (int k = 0; x4 + k < g.w; k++) {
                    const int vv = gray_of(sb[k * CN], sb[k * CN + 1], sb[k * CN + 2]);
                    grow[(size_t)y * g.gpitch + x4 + k] = (uint8_t)vv;
                    if (hist) atomicAdd(&lh[wave][vv], 1u);
                }
            }
        }
    }
    if (hist) hist_flush(lh, hist + slot * 256, tid);
}

void launch_gray(hipStream_t st, const uint8_t *const *d_src, const PreGeom &g, const ResizeView &t,
                 uint8_t *gray, unsigned *hist, int batch, bool aligned4)
{
    const int gy = (g.h + kGrayRows - 1) / kGrayRows;
    if (t.mode == 0 && aligned4 && (g.cn == 3 || g.cn == 4)) {
        dim3 grid((g.w + 1023) / 1024, gy, batch);
        if (g.cn == 3) NVCA_LAUNCH(k_gray_fast4<3>, grid, dim3(256), 0, st, d_src, g, gray, hist);
        else           NVCA_LAUNCH(k_gray_fast4<4>, grid, dim3(256), 0, st, d_src, g, gray, hist);
    } else {
        dim3 grid((g.w + 255) / 256, gy, batch);
        NVCA_LAUNCH(k_gray_generic, grid, dim3(256), 0, st, d_src, g, t, gray, hist);
    }
}

// ---- 4:2:0 sources (NV12 / I420 face streams, nvca_yuv420_to_bgr): cv::cvtColor(CV_YUV2BGR_NV12 / _I420) in front of
// FACE/kmsfacedetect.cpp:805, computed where the frame is read.  OpenCV 2.4 color.cpp, BT.601 limited range, shift 20:
// pixel (x, y) takes the chroma sample (x >> 1, y >> 1); all int32, the shift arithmetic.
// (the arithmetic: yuv_device.h)

// ---- K1 for 4:2:0 frames at full resolution, beside k_gray_fast4: a thread owns 16 pixels of two rows -- the block one row of
// chroma samples serves -- and reads them with one 16-byte load per luma row and 16 bytes of chroma (NV12: 8 U,V pairs; I420: 8
// bytes of each plane).  Units are numbered along the rows and on from one row pair to the next, so every lane of a launch but
// the last few has work whatever the width.  The unit at the end of a row that holds fewer than 16 pixels goes byte by byte.
// Wants every plane and its stride aligned to the loads (launch_gray_yuv sends anything else to k_gray_yuv_generic).
template <int FMT>
__global__ __launch_bounds__(256) void k_gray_yuv16(
    const uint8_t *const *__restrict__ srcs, PreGeom g, YuvPlanes p, uint8_t *__restrict__ gray, unsigned *__restrict__ hist)
{
    __shared__ unsigned lh[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, slot = blockIdx.z;
    for (int i = tid; i < 1024; i += 256) (&lh[0][0])[i] = 0;
    __syncthreads();
    const uint8_t *__restrict__ src = srcs[slot];
    const int upr = (g.w + 15) >> 4;                        // units per row pair
    const int unit = blockIdx.x * 256 + tid;
    if (unit < upr * (g.h >> 1)) {
        const int ry = unit / upr, x = (unit - ry * upr) << 4;
        const uint8_t *y0 = src + p.off_y + (size_t)(2 * ry) * g.sstride + x, *y1 = y0 + g.sstride;
        uint8_t *g0 = gray + (size_t)slot * g.gray_slot + (size_t)(2 * ry) * g.gpitch + x, *g1 = g0 + g.gpitch;
        if (x + 16 <= g.w) {
            const uint4 a = *(const uint4 *)y0, b = *(const uint4 *)y1;
            const unsigned yw0[4] = {a.x, a.y, a.z, a.w}, yw1[4] = {b.x, b.y, b.z, b.w};
            unsigned cw[4];                                 // NV12: U,V pairs; I420: cw[0..1] U, cw[2..3] V
            if (FMT == 1) {
                const uint4 c = *(const uint4 *)(src + p.off_u + (size_t)ry * p.cstride + x);
                cw[0] = c.x; cw[1] = c.y; cw[2] = c.z; cw[3] = c.w;
            } else {
                const uint2 u = *(const uint2 *)(src + p.off_u + (size_t)ry * p.cstride + (x >> 1));
                const uint2 v = *(const uint2 *)(src + p.off_v + (size_t)ry * p.vstride + (x >> 1));
                cw[0] = u.x; cw[1] = u.y; cw[2] = v.x; cw[3] = v.y;
            }
            unsigned o0[4] = {0, 0, 0, 0}, o1[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                int U, V;
                if (FMT == 1) { const unsigned w = cw[k >> 1] >> ((k & 1) * 16); U = w & 255; V = (w >> 8) & 255; }
                else { U = (cw[k >> 2] >> ((k & 3) * 8)) & 255; V = (cw[2 + (k >> 2)] >> ((k & 3) * 8)) & 255; }
                const ChromaTerm c = chroma_term(U, V);
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int wi = (2 * k + j) >> 2, sh = ((2 * k + j) & 3) * 8;
                    const int v0 = yuv_gray((yw0[wi] >> sh) & 255, c), v1 = yuv_gray((yw1[wi] >> sh) & 255, c);
                    o0[wi] |= (unsigned)v0 << sh; o1[wi] |= (unsigned)v1 << sh;
                    if (hist) { atomicAdd(&lh[wave][v0], 1u); atomicAdd(&lh[wave][v1], 1u); }
                }
            }
            *(uint4 *)g0 = make_uint4(o0[0], o0[1], o0[2], o0[3]);
            *(uint4 *)g1 = make_uint4(o1[0], o1[1], o1[2], o1[3]);
        } else {
            for (int k = 0; x + k < g.w; k += 2) {          // the width is even: whole chroma pairs
                const ChromaTerm c = chroma_at<FMT>(src, p, (x + k) >> 1, ry);
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int v0 = yuv_gray(y0[k + j], c), v1 = yuv_gray(y1[k + j], c);
                    g0[k + j] = (uint8_t)v0; g1[k + j] = (uint8_t)v1;
                    if (hist) { atomicAdd(&lh[wave][v0], 1u); atomicAdd(&lh[wave][v1], 1u); }
                }
            }
        }
    }
    if (hist) hist_flush(lh, hist + slot * 256, tid);
}

// ---- K1 generic for 4:2:0 frames: one output pixel per thread, any resize mode, any alignment.  The reference's order
// (convert, cv::resize on BGR, BGR2GRAY): every tap of the resize is a converted pixel.
template <int FMT>
__global__ __launch_bounds__(256) void k_gray_yuv_generic(
    const uint8_t *const *__restrict__ srcs, PreGeom g, YuvPlanes p, ResizeView t,
    uint8_t *__restrict__ gray, unsigned *__restrict__ hist)
{
    __shared__ unsigned lh[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, slot = blockIdx.z;
    for (int i = tid; i < 1024; i += 256) (&lh[0][0])[i] = 0;
    __syncthreads();
    const uint8_t *__restrict__ src = srcs[slot];
    const int x = blockIdx.x * 256 + tid;
    uint8_t *grow = gray + (size_t)slot * g.gray_slot;
    auto tap = [&](int r, int c, int *v) {
        yuv_bgr(src[p.off_y + (size_t)r * g.sstride + c], chroma_at<FMT>(src, p, c >> 1, r >> 1), v[0], v[1], v[2]);
    };
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y >= g.h) break;
        if (x < g.w) {
            int c[3];
            resize_sample<3>(tap, g.sh, t, x, y, c);
            const int v = gray_of(c[0] & 255, c[1] & 255, c[2] & 255);
            grow[(size_t)y * g.gpitch + x] = (uint8_t)v;
            if (hist) atomicAdd(&lh[wave][v], 1u);
        }
    }
    if (hist) hist_flush(lh, hist + slot * 256, tid);
}

// ---- packed 4:2:2 sources (YUY2 / UYVY / YVYU face streams, the eye chain's gray image): cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU)
// in front of FACE/kmsfacedetect.cpp:805, computed where the frame is read (the fetches: yuv_device.h).
// K1 at full resolution, beside k_gray_yuv16: a thread owns 16 pixels of ONE row -- every row carries its own chroma -- and reads them
// with two 16-byte loads of the packed row (8 pixel pairs, a word each), one 16-byte gray store.  Units are numbered along the rows and
// on from row to row; the unit at the end of a row that holds fewer than 16 pixels goes byte by byte.  Wants the base, the offset and
// the stride 16-byte aligned (launch_gray_yuv sends anything else to k_gray_yuv422_generic).
template <int FMT>
__global__ __launch_bounds__(256) void k_gray_yuv422_16(
    const uint8_t *const *__restrict__ srcs, PreGeom g, YuvPlanes p, uint8_t *__restrict__ gray, unsigned *__restrict__ hist)
{
    __shared__ unsigned lh[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, slot = blockIdx.z;
    for (int i = tid; i < 1024; i += 256) (&lh[0][0])[i] = 0;
    __syncthreads();
    const uint8_t *__restrict__ src = srcs[slot];
    const int upr = (g.w + 15) >> 4;                        // units per row
    const int unit = blockIdx.x * 256 + tid;
    if (unit < upr * g.h) {
        const int y = unit / upr, x = (unit - y * upr) << 4;
        const uint8_t *row = src + p.off_y + (size_t)y * g.sstride + 2 * (size_t)x;
        uint8_t *go = gray + (size_t)slot * g.gray_slot + (size_t)y * g.gpitch + x;
        if (x + 16 <= g.w) {
            const uint4 a = *(const uint4 *)row, b = *(const uint4 *)(row + 16);
            const unsigned pw[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const ChromaTerm c = chroma_of_pair<FMT>(pw[k]);
                const int v0 = yuv_gray(luma_of_pair<FMT>(pw[k], 0), c), v1 = yuv_gray(luma_of_pair<FMT>(pw[k], 1), c);
                o[k >> 1] |= ((unsigned)v0 | ((unsigned)v1 << 8)) << ((k & 1) * 16);
                if (hist) { atomicAdd(&lh[wave][v0], 1u); atomicAdd(&lh[wave][v1], 1u); }
            }
            *(uint4 *)go = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            for (int k = 0; x + k < g.w; k++) {             // (the width is even: whole pairs; the term of a pair is formed for each of its pixels here)
                ChromaTerm c;
                const int Y = yuv422_at<FMT>(src, p, g.sstride, y, x + k, c), v = yuv_gray(Y, c);
                go[k] = (uint8_t)v;
                if (hist) atomicAdd(&lh[wave][v], 1u);
            }
        }
    }
    if (hist) hist_flush(lh, hist + slot * 256, tid);
}

// K1 generic for packed 4:2:2 frames, beside k_gray_yuv_generic: one output pixel per thread, any resize mode, any alignment; every
// tap of the resize is a converted pixel
template <int FMT>
__global__ __launch_bounds__(256) void k_gray_yuv422_generic(
    const uint8_t *const *__restrict__ srcs, PreGeom g, YuvPlanes p, ResizeView t,
    uint8_t *__restrict__ gray, unsigned *__restrict__ hist)
{
    __shared__ unsigned lh[4][256];
    const int tid = threadIdx.x, wave = tid >> 6, slot = blockIdx.z;
    for (int i = tid; i < 1024; i += 256) (&lh[0][0])[i] = 0;
    __syncthreads();
    const uint8_t *__restrict__ src = srcs[slot];
    const int x = blockIdx.x * 256 + tid;
    uint8_t *grow = gray + (size_t)slot * g.gray_slot;
    auto tap = [&](int r, int c, int *v) {
        ChromaTerm ct;
        const int Y = yuv422_at<FMT>(src, p, g.sstride, r, c, ct);
        yuv_bgr(Y, ct, v[0], v[1], v[2]);
    };
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y >= g.h) break;
        if (x < g.w) {
            int c[3];
            resize_sample<3>(tap, g.sh, t, x, y, c);
            const int v = gray_of(c[0] & 255, c[1] & 255, c[2] & 255);
            grow[(size_t)y * g.gpitch + x] = (uint8_t)v;
            if (hist) atomicAdd(&lh[wave][v], 1u);
        }
    }
    if (hist) hist_flush(lh, hist + slot * 256, tid);
}

template <int FMT>
static bool launch_gray_yuv422(hipStream_t st, const uint8_t *const *d_src, const PreGeom &g, const YuvPlanes &p, const ResizeView &t,
                               uint8_t *gray, unsigned *hist, int batch, bool aligned16)
{
    if (t.mode == 0 && aligned16) {
        const int units = ((g.w + 15) >> 4) * g.h;
        NVCA_LAUNCH(k_gray_yuv422_16<FMT>, dim3((units + 255) / 256, 1, batch), dim3(256), 0, st, d_src, g, p, gray, hist);
        return true;
    }
    dim3 grid((g.w + 255) / 256, (g.h + kGrayRows - 1) / kGrayRows, batch);
    NVCA_LAUNCH(k_gray_yuv422_generic<FMT>, grid, dim3(256), 0, st, d_src, g, p, t, gray, hist);
    return false;
}

const char *gray_yuv_kernel_name(int fmt, bool wide)
{
    if (fmt >= NVCA_PIX_YUY2) return wide ? "k_gray_yuv422_16" : "k_gray_yuv422_generic";
    return wide ? "k_gray_yuv16" : "k_gray_yuv_generic";
}

bool launch_gray_yuv(hipStream_t st, const uint8_t *const *d_src, const PreGeom &g, const YuvPlanes &p, const ResizeView &t,
                     uint8_t *gray, unsigned *hist, int batch, bool aligned16)
{
    if (p.fmt == NVCA_PIX_YUY2) return launch_gray_yuv422<NVCA_PIX_YUY2>(st, d_src, g, p, t, gray, hist, batch, aligned16);
    if (p.fmt == NVCA_PIX_UYVY) return launch_gray_yuv422<NVCA_PIX_UYVY>(st, d_src, g, p, t, gray, hist, batch, aligned16);
    if (p.fmt == NVCA_PIX_YVYU) return launch_gray_yuv422<NVCA_PIX_YVYU>(st, d_src, g, p, t, gray, hist, batch, aligned16);
    if (t.mode == 0 && aligned16) {
        const int units = ((g.w + 15) >> 4) * (g.h >> 1);
        dim3 grid((units + 255) / 256, 1, batch);
        if (p.fmt == 1) NVCA_LAUNCH(k_gray_yuv16<1>, grid, dim3(256), 0, st, d_src, g, p, gray, hist);
        else            NVCA_LAUNCH(k_gray_yuv16<2>, grid, dim3(256), 0, st, d_src, g, p, gray, hist);
        return true;
    } else {
        dim3 grid((g.w + 255) / 256, (g.h + kGrayRows - 1) / kGrayRows, batch);
        if (p.fmt == 1) NVCA_LAUNCH(k_gray_yuv_generic<1>, grid, dim3(256), 0, st, d_src, g, p, t, gray, hist);
        else            NVCA_LAUNCH(k_gray_yuv_generic<2>, grid, dim3(256), 0, st, d_src, g, p, t, gray, hist);
        return false;
    }
}

// ---- cv::cvtColor(CV_YUV2BGR_NV12 / _I420) as a primitive (nvca_yuv420_to_bgr): a thread converts the 2 x 2 blocks of one
// chroma column, kGrayRows chroma rows of it
template <int FMT>
__global__ __launch_bounds__(256) void k_yuv420_to_bgr(const uint8_t *__restrict__ src, int w, int h, int ystride, YuvPlanes p,
                                                       uint8_t *__restrict__ dst, int dstride)
{
    const int cx = blockIdx.x * 256 + threadIdx.x;
    if (2 * cx >= w) return;
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int cy = blockIdx.y * kGrayRows + ry;
        if (2 * cy >= h) break;
        const ChromaTerm c = chroma_at<FMT>(src, p, cx, cy);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint8_t *y = src + p.off_y + (size_t)(2 * cy + j) * ystride + 2 * cx;
            uint8_t *d = dst + (size_t)(2 * cy + j) * dstride + (size_t)cx * 6;
#pragma unroll
            for (int i = 0; i < 2; i++) {
                int B, G, R;
                yuv_bgr(y[i], c, B, G, R);
                d[3 * i] = (uint8_t)B; d[3 * i + 1] = (uint8_t)G; d[3 * i + 2] = (uint8_t)R;
            }
        }
    }
}
void launch_yuv420_to_bgr(hipStream_t st, const uint8_t *src, int w, int h, int ystride, const YuvPlanes &p, uint8_t *dst, int dstride)
{
    dim3 grid((w / 2 + 255) / 256, (h / 2 + kGrayRows - 1) / kGrayRows, 1);
    if (p.fmt == 1) NVCA_LAUNCH(k_yuv420_to_bgr<1>, grid, dim3(256), 0, st, src, w, h, ystride, p, dst, dstride);
    else            NVCA_LAUNCH(k_yuv420_to_bgr<2>, grid, dim3(256), 0, st, src, w, h, ystride, p, dst, dstride);
}

// ---- cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU) as a primitive (nvca_yuv422_to_bgr): a thread converts one pixel pair, kGrayRows
// rows of it; byte reads and byte stores, any alignment
template <int FMT>
__global__ __launch_bounds__(256) void k_yuv422_to_bgr(const uint8_t *__restrict__ src, int w, int h, int sstride, YuvPlanes p,
                                                       uint8_t *__restrict__ dst, int dstride)
{
    const int cx = blockIdx.x * 256 + threadIdx.x;
    if (2 * cx >= w) return;
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y >= h) break;
        uint8_t *d = dst + (size_t)y * dstride + (size_t)cx * 6;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            ChromaTerm c;
            int B, G, R;
            const int Y = yuv422_at<FMT>(src, p, sstride, y, 2 * cx + i, c);
            yuv_bgr(Y, c, B, G, R);
            d[3 * i] = (uint8_t)B; d[3 * i + 1] = (uint8_t)G; d[3 * i + 2] = (uint8_t)R;
        }
    }
}
void launch_yuv422_to_bgr(hipStream_t st, const uint8_t *src, int w, int h, int sstride, const YuvPlanes &p, uint8_t *dst, int dstride)
{
    dim3 grid((w / 2 + 255) / 256, (h + kGrayRows - 1) / kGrayRows, 1);
    if (p.fmt == NVCA_PIX_UYVY)      NVCA_LAUNCH(k_yuv422_to_bgr<NVCA_PIX_UYVY>, grid, dim3(256), 0, st, src, w, h, sstride, p, dst, dstride);
    else if (p.fmt == NVCA_PIX_YVYU) NVCA_LAUNCH(k_yuv422_to_bgr<NVCA_PIX_YVYU>, grid, dim3(256), 0, st, src, w, h, sstride, p, dst, dstride);
    else                             NVCA_LAUNCH(k_yuv422_to_bgr<NVCA_PIX_YUY2>, grid, dim3(256), 0, st, src, w, h, sstride, p, dst, dstride);
}

// ---- 8UC1 resize (gray-then-resize order of the part detectors, pyramid levels): resize_sample on one channel, the value as a
// byte.  `px(row, col)`: the source sample (a gray byte, a gray byte through a LUT, or the gray value of a converted pixel)
template <class Px>
__device__ __forceinline__ int resize1_sample(Px px, int sh, const ResizeView &t, int x, int y)
{
    int v;
    resize_sample<1>([&](int r, int c, int *p) { p[0] = px(r, c); }, sh, t, x, y, &v);
    return v & 255;
}
__device__ __forceinline__ int resize1_value(const uint8_t *__restrict__ src, int sh, int sstride, const ResizeView &t, int x, int y)
{
    return resize1_sample([&](int r, int c) { return (int)src[(size_t)r * sstride + c]; }, sh, t, x, y);
}

// the LDS copy of a frame's LUT in the kernels that read an image through one (none in the instantiations that do not)
template <bool LUT>
__device__ __forceinline__ uint8_t *lut_lds()
{
    if constexpr (LUT) { __shared__ uint8_t sl[256]; return sl; }
    else return nullptr;
}

// LUT: image z's sample is lut[z][byte] (cv::equalizeHist in front of the resize, applied where the image is read: the frame's 256-byte
// LUT is staged in LDS once a workgroup, as k_work_resize<kWorkGray> does it); otherwise the byte itself, and `luts` is not read
template <bool LUT>
__device__ __forceinline__ void resize1_rows(
    const uint8_t *__restrict__ src, int sh, int sstride, ResizeView t,
    uint8_t *__restrict__ dst, int dw, int dh, int dstride, unsigned *__restrict__ hist, size_t src_slot, size_t dst_slot,
    const uint8_t *__restrict__ luts)
{
    __shared__ unsigned lh[4][256];
    uint8_t *const sl = lut_lds<LUT>();
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < 1024; i += 256) (&lh[0][0])[i] = 0;
    if (LUT) sl[tid] = luts[(size_t)blockIdx.z * 256 + tid];
    __syncthreads();
    src += (size_t)blockIdx.z * src_slot; dst += (size_t)blockIdx.z * dst_slot;      // several images of one geometry
    if (hist) hist += (size_t)blockIdx.z * 256;
    const int x = blockIdx.x * 256 + tid;
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y >= dh) break;
        if (x < dw) {
            const int v = LUT ? resize1_sample([&](int r, int c) { return (int)sl[src[(size_t)r * sstride + c]]; }, sh, t, x, y)
                              : resize1_value(src, sh, sstride, t, x, y);
            dst[(size_t)y * dstride + x] = (uint8_t)v;
            if (hist) atomicAdd(&lh[wave][v], 1u);
        }
    }
    if (hist) hist_flush(lh, hist, tid);
}
__global__ __launch_bounds__(256) void k_resize1(
    const uint8_t *__restrict__ src, int sw, int sh, int sstride, ResizeView t,
    uint8_t *__restrict__ dst, int dw, int dh, int dstride, unsigned *__restrict__ hist, size_t src_slot, size_t dst_slot)
{
    resize1_rows<false>(src, sh, sstride, t, dst, dw, dh, dstride, hist, src_slot, dst_slot, nullptr);
}
__global__ __launch_bounds__(256) void k_resize1_lut(
    const uint8_t *__restrict__ src, int sw, int sh, int sstride, ResizeView t,
    uint8_t *__restrict__ dst, int dw, int dh, int dstride, unsigned *__restrict__ hist, size_t src_slot, size_t dst_slot,
    const uint8_t *__restrict__ luts)
{
    resize1_rows<true>(src, sh, sstride, t, dst, dw, dh, dstride, hist, src_slot, dst_slot, luts);
}

// ---- 8UC3 resize (cv::resize on the BGR frame, FACE/kmsfacedetect.cpp:805, as a stand-alone primitive;
// the face stream fuses it with BGR2GRAY in k_gray_generic)
__global__ __launch_bounds__(256) void k_resize3(
    const uint8_t *__restrict__ src, int sw, int sh, int sstride, ResizeView t,
    uint8_t *__restrict__ dst, int dw, int dh, int dstride)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    auto tap = [&](int r, int c, int *p) {
        const uint8_t *s = src + (size_t)r * sstride + (size_t)c * 3;
        p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
    };
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y >= dh || x >= dw) continue;
        int c[3];
        resize_sample<3>(tap, sh, t, x, y, c);
        uint8_t *d = dst + (size_t)y * dstride + (size_t)x * 3;
        d[0] = (uint8_t)c[0]; d[1] = (uint8_t)c[1]; d[2] = (uint8_t)c[2];
    }
}
void launch_resize3(hipStream_t st, const uint8_t *src, int sw, int sh, int sstride, const ResizeView &t,
                    uint8_t *dst, int dw, int dh, int dstride)
{
    dim3 grid((dw + 255) / 256, (dh + kGrayRows - 1) / kGrayRows, 1);
    NVCA_LAUNCH(k_resize3, grid, dim3(256), 0, st, src, sw, sh, sstride, t, dst, dw, dh, dstride);
}

void launch_resize1(hipStream_t st, const uint8_t *src, int sw, int sh, int sstride, const ResizeView &t,
                    uint8_t *dst, int dw, int dh, int dstride, unsigned *hist, int batch, size_t src_slot, size_t dst_slot, const uint8_t *luts)
{
    dim3 grid((dw + 255) / 256, (dh + kGrayRows - 1) / kGrayRows, batch);
    if (luts) NVCA_LAUNCH(k_resize1_lut, grid, dim3(256), 0, st, src, sw, sh, sstride, t, dst, dw, dh, dstride, hist, src_slot, dst_slot, luts);
    else      NVCA_LAUNCH(k_resize1, grid, dim3(256), 0, st, src, sw, sh, sstride, t, dst, dw, dh, dstride, hist, src_slot, dst_slot);
}

// ---- working images of the part detectors, all frames of a batched call in one launch: image z of the launch is
// resize(gray(frame z)) (SRC = kWorkBgr: the gray value of a source pixel is computed where the resize reads it -- cvtColor then
// resize, EYE/kmseyedetect.cpp:948-956, NOSE/kmsnosedetect.cpp:836-841 -- without writing the full-size gray image; kWorkNv12 /
// kWorkI420: the same with cv::cvtColor(CV_YUV2BGR_NV12 / _I420) in front, tap (r, c) = yuv_gray(Y[r][c], chroma(c >> 1, r >> 1))) or
// resize(lut[gray z]) (kWorkGray: the eye detector equalizes the full-size gray image first, EYE :950), plus its histogram.
// kWorkYuy2 / kWorkUyvy / kWorkYvyu: the same with cv::cvtColor(CV_YUV2BGR_YUY2 / _UYVY / _YVYU) in front, tap (r, c) = yuv_gray of the
// pixel's luma and its pair's chroma in row r (yuv422_at).
enum { kWorkGray = 0, kWorkBgr = 1, kWorkNv12 = 2, kWorkI420 = 3, kWorkYuy2 = 4, kWorkUyvy = 5, kWorkYvyu = 6 };
static_assert(kWorkYuy2 == NVCA_PIX_YUY2 && kWorkUyvy == NVCA_PIX_UYVY && kWorkYvyu == NVCA_PIX_YVYU, "a 4:2:2 source's number is its format");
template <int SRC>
__global__ __launch_bounds__(256) void k_work_resize(
    const uint8_t *const *__restrict__ srcs, const int *__restrict__ lut_idx, const uint8_t *__restrict__ luts, YuvPlanes yp,
    int sh, int sstride, ResizeView t, uint8_t *__restrict__ dst, int dw, int dh, int dstride, size_t dst_slot, unsigned *__restrict__ hist)
{
    __shared__ unsigned lh[4][256];
    __shared__ uint8_t sl[256];
    const int tid = threadIdx.x, wave = tid >> 6, z = blockIdx.z;
    for (int i = tid; i < 1024; i += 256) (&lh[0][0])[i] = 0;
    const uint8_t *__restrict__ src = srcs[z];
    const bool use_lut = SRC == kWorkGray && lut_idx != nullptr;
    if (use_lut) sl[tid] = luts[(size_t)lut_idx[z] * 256 + tid];
    __syncthreads();
    dst += (size_t)z * dst_slot;
    const int x = blockIdx.x * 256 + tid;
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y >= dh) break;
        if (x < dw) {
            int v;
            if (SRC == kWorkBgr) v = resize1_sample([&](int r, int c) { const uint8_t *p = src + (size_t)r * sstride + (size_t)c * 3; return gray_of(p[0], p[1], p[2]); }, sh, t, x, y);
            else if (SRC == kWorkNv12 || SRC == kWorkI420)
                v = resize1_sample([&](int r, int c) { return yuv_gray(src[yp.off_y + (size_t)r * sstride + c], chroma_at<SRC == kWorkNv12 ? 1 : 2>(src, yp, c >> 1, r >> 1)); }, sh, t, x, y);
            else if (SRC >= kWorkYuy2)
                v = resize1_sample([&](int r, int c) { ChromaTerm ct; const int Y = yuv422_at<SRC>(src, yp, sstride, r, c, ct); return yuv_gray(Y, ct); }, sh, t, x, y);
            else if (use_lut) v = resize1_sample([&](int r, int c) { return (int)sl[src[(size_t)r * sstride + c]]; }, sh, t, x, y);
            else v = resize1_value(src, sh, sstride, t, x, y);
            dst[(size_t)y * dstride + x] = (uint8_t)v;
            if (hist) atomicAdd(&lh[wave][v], 1u);
        }
    }
    if (hist) hist_flush(lh, hist + (size_t)z * 256, tid);
}
// yuv: planes of the frames' 4:2:0 layout (fmt 0 / null: `bgr` says whether the sources are packed BGR frames or gray images)
void launch_work_resize(hipStream_t st, bool bgr, const uint8_t *const *d_srcs, const int *d_lut_idx, const uint8_t *d_luts, int sh, int sstride,
                        const ResizeView &t, uint8_t *dst, int dw, int dh, int dstride, size_t dst_slot, unsigned *hist, int batch, const YuvPlanes *yuv)
{
    dim3 grid((dw + 255) / 256, (dh + kGrayRows - 1) / kGrayRows, batch);
    const YuvPlanes yp = yuv ? *yuv : YuvPlanes{};
#define NVCA_WORK_RESIZE(SRC) NVCA_LAUNCH(k_work_resize<SRC>, grid, dim3(256), 0, st, d_srcs, d_lut_idx, d_luts, yp, sh, sstride, t, dst, dw, dh, dstride, dst_slot, hist)
    if (yp.fmt == 1) NVCA_WORK_RESIZE(kWorkNv12);
    else if (yp.fmt == 2) NVCA_WORK_RESIZE(kWorkI420);
    else if (yp.fmt == NVCA_PIX_YUY2) NVCA_WORK_RESIZE(kWorkYuy2);
    else if (yp.fmt == NVCA_PIX_UYVY) NVCA_WORK_RESIZE(kWorkUyvy);
    else if (yp.fmt == NVCA_PIX_YVYU) NVCA_WORK_RESIZE(kWorkYvyu);
    else if (bgr) NVCA_WORK_RESIZE(kWorkBgr);
    else NVCA_WORK_RESIZE(kWorkGray);
#undef NVCA_WORK_RESIZE
}

// ---- CV_HAAR_SCALE_IMAGE / LBP pyramids: every level of every image in one launch (k_pyr_integral, kernels_integral.hip, takes them from here).
// LUT: the pyramid of lut[img][image] -- a face stream's equalised working image, which is never written out: equalizeHist first, cv::resize
// second, as OpenCV orders them; level 0 (identity) is the equalised image itself
template <bool LUT>
__device__ __forceinline__ void pyr_resize_rows(const uint8_t *__restrict__ src, int sh, int sstride, size_t src_slot,
                                                const PyrLevelDev *__restrict__ levels, int nimg,
                                                uint8_t *__restrict__ aux, size_t aux_slot, const uint8_t *__restrict__ luts)
{
    uint8_t *const sl = lut_lds<LUT>();
    const int lev = blockIdx.z / nimg, img = blockIdx.z - lev * nimg;
    const PyrLevelDev L = levels[lev];
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= L.szw || blockIdx.y * kGrayRows >= L.szh) return;
    if (LUT) { sl[threadIdx.x] = luts[(size_t)img * 256 + threadIdx.x]; __syncthreads(); }      // (the return above is the whole workgroup's)
    const uint8_t *s = src + (size_t)img * src_slot;
    uint8_t *d = aux + (size_t)img * aux_slot + L.gray_off;
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y >= L.szh) break;
        if (x < L.szw) {
            if (LUT) d[(size_t)y * L.gpitch + x] = (uint8_t)resize1_sample([&](int r, int c) { return (int)sl[s[(size_t)r * sstride + c]]; }, sh, L.tab, x, y);
            else d[(size_t)y * L.gpitch + x] = (uint8_t)resize1_value(s, sh, sstride, L.tab, x, y);
        }
    }
}
__global__ __launch_bounds__(256) void k_pyr_resize(const uint8_t *__restrict__ src, int sw, int sh, int sstride, size_t src_slot,
                                                    const PyrLevelDev *__restrict__ levels, int nimg,
                                                    uint8_t *__restrict__ aux, size_t aux_slot)
{
    pyr_resize_rows<false>(src, sh, sstride, src_slot, levels, nimg, aux, aux_slot, nullptr);
}
__global__ __launch_bounds__(256) void k_pyr_resize_lut(const uint8_t *__restrict__ src, int sw, int sh, int sstride, size_t src_slot,
                                                        const PyrLevelDev *__restrict__ levels, int nimg,
                                                        uint8_t *__restrict__ aux, size_t aux_slot, const uint8_t *__restrict__ luts)
{
    pyr_resize_rows<true>(src, sh, sstride, src_slot, levels, nimg, aux, aux_slot, luts);
}
void launch_pyr_resize(hipStream_t st, const uint8_t *src, int sw, int sh, int sstride, size_t src_slot, const PyrLevelDev *levels,
                       int nlev, int nimg, int maxw, int maxh, uint8_t *aux, size_t aux_slot, const uint8_t *luts)
{
    dim3 grid((maxw + 255) / 256, (maxh + kGrayRows - 1) / kGrayRows, nlev * nimg);
    if (luts) NVCA_LAUNCH(k_pyr_resize_lut, grid, dim3(256), 0, st, src, sw, sh, sstride, src_slot, levels, nimg, aux, aux_slot, luts);
    else      NVCA_LAUNCH(k_pyr_resize, grid, dim3(256), 0, st, src, sw, sh, sstride, src_slot, levels, nimg, aux, aux_slot);
}

} // namespace nvca
