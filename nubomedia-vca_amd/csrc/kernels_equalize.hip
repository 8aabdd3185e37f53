// kernels_equalize.hip -- gfx950 kernels for cv::equalizeHist (FACE/kmsfacedetect.cpp:811: the LUT from the histogram the gray
// kernels leave, the histogram and the LUT pass as stand-alone primitives) and cv::flip(src, dst, 1) (EAR/kmseardetect.cpp:800).
#include "launch.h"
#include "pre_device.h"

namespace nvca {

// ---- K2: equalizeHist LUT from the histogram (one block per slot)
// `rezero`: the histogram is cleared again once read (the next frame's gray kernel accumulates into it) and the two
// list counters of the cascade that follows are reset -- three fill launches less per batch.
__global__ __launch_bounds__(256) void k_lut(unsigned *__restrict__ hist, int total, uint8_t *__restrict__ lut, int rezero,
                                             unsigned long long *__restrict__ zero_a, unsigned long long *__restrict__ zero_b)
{
    __shared__ unsigned wsum[4];
    __shared__ unsigned long long wmask[4];
    __shared__ unsigned hs[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, slot = blockIdx.x;
    const unsigned h = hist[slot * 256 + tid];
    hs[tid] = h;
    if (rezero) hist[slot * 256 + tid] = 0;
    if (slot == 0 && tid == 0) { if (zero_a) *zero_a = 0; if (zero_b) *zero_b = 0; }
    unsigned incl = h;
    for (int d = 1; d < 64; d <<= 1) { unsigned t = __shfl_up(incl, d); if (lane >= d) incl += t; }
    const unsigned long long m = __ballot(h != 0);
    if (lane == 63) wsum[wave] = incl;
    if (lane == 0) wmask[wave] = m;
    __syncthreads();
    for (int j = 0; j < wave; j++) incl += wsum[j];
    int first = 256;
    for (int j = 3; j >= 0; j--) if (wmask[j]) first = j * 64 + __ffsll((long long)wmask[j]) - 1;
    uint8_t out;
    if (first == 256) out = 0;
    else {
        const unsigned hf = hs[first];
        if (hf == (unsigned)total) out = (uint8_t)first;         // dst.setTo(i)
        else if (tid <= first) out = 0;
        else {
            const float scale = 255.f / (float)(int)(total - (int)hf);   // (hist_sz-1.f)/(total-hist[i])
            const float v = (float)(int)(incl - hf) * scale;             // sum*scale, int -> float
            int iv = (int)rintf(v);                                      // saturate_cast<uchar>: cvRound + clamp
            out = (uint8_t)(iv < 0 ? 0 : (iv > 255 ? 255 : iv));
        }
    }
    lut[slot * 256 + tid] = out;
}

void launch_lut(hipStream_t st, unsigned *hist, int total, uint8_t *lut, int batch, int rezero, unsigned long long *zero_a,
                unsigned long long *zero_b)
{
    NVCA_LAUNCH(k_lut, dim3(batch), dim3(256), 0, st, hist, total, lut, rezero, zero_a, zero_b);
}

__global__ __launch_bounds__(256) void k_hist(const uint8_t *__restrict__ gray, int w, int h, int pitch,
                                              unsigned *__restrict__ hist)
{
    __shared__ unsigned lh[4][256];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < 1024; i += 256) (&lh[0][0])[i] = 0;
    __syncthreads();
    const int x = blockIdx.x * 256 + tid;
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y < h && x < w) atomicAdd(&lh[wave][gray[(size_t)y * pitch + x]], 1u);
    }
    hist_flush(lh, hist, tid);
}
void launch_hist(hipStream_t st, const uint8_t *gray, int w, int h, int pitch, unsigned *hist)
{
    dim3 grid((w + 255) / 256, (h + kGrayRows - 1) / kGrayRows, 1);
    NVCA_LAUNCH(k_hist, grid, dim3(256), 0, st, gray, w, h, pitch, hist);
}

__global__ __launch_bounds__(256) void k_apply_lut(const uint8_t *__restrict__ src, int w, int h, int spitch,
                                                   const uint8_t *__restrict__ lut, uint8_t *__restrict__ dst, int dpitch,
                                                   size_t src_slot, size_t dst_slot)
{
    __shared__ uint8_t sl[256];
    sl[threadIdx.x] = lut[(size_t)blockIdx.z * 256 + threadIdx.x];          // image z of the launch: its own LUT and slot
    src += (size_t)blockIdx.z * src_slot; dst += (size_t)blockIdx.z * dst_slot;
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x;
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y < h && x < w) dst[(size_t)y * dpitch + x] = sl[src[(size_t)y * spitch + x]];
    }
}
void launch_apply_lut(hipStream_t st, const uint8_t *src, int w, int h, int spitch, const uint8_t *lut,
                      uint8_t *dst, int dpitch, int batch, size_t src_slot, size_t dst_slot)
{
    dim3 grid((w + 255) / 256, (h + kGrayRows - 1) / kGrayRows, batch);
    NVCA_LAUNCH(k_apply_lut, grid, dim3(256), 0, st, src, w, h, spitch, lut, dst, dpitch, src_slot, dst_slot);
}

// ---- cv::flip(src, dst, 1) (EAR/kmseardetect.cpp:800)
__global__ __launch_bounds__(256) void k_flip_h(const uint8_t *__restrict__ src, int w, int h, int spitch,
                                                uint8_t *__restrict__ dst, int dpitch, size_t src_slot, size_t dst_slot)
{
    src += (size_t)blockIdx.z * src_slot; dst += (size_t)blockIdx.z * dst_slot;
    const int x = blockIdx.x * 256 + threadIdx.x;
    for (int ry = 0; ry < kGrayRows; ry++) {
        const int y = blockIdx.y * kGrayRows + ry;
        if (y < h && x < w) dst[(size_t)y * dpitch + x] = src[(size_t)y * spitch + (w - 1 - x)];
    }
}
void launch_flip_h(hipStream_t st, const uint8_t *src, int w, int h, int spitch, uint8_t *dst, int dpitch, int batch, size_t src_slot,
                   size_t dst_slot)
{
    dim3 grid((w + 255) / 256, (h + kGrayRows - 1) / kGrayRows, batch);
    NVCA_LAUNCH(k_flip_h, grid, dim3(256), 0, st, src, w, h, spitch, dst, dpitch, src_slot, dst_slot);
}

} // namespace nvca
