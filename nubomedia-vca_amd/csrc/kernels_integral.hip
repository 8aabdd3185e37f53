// kernels_integral.hip -- gfx950 kernels for cv::integral as detectMultiScale calls it: sum and squared sum (three launches
// for a frame, one for a small image or a whole pyramid) and the tilted plane.  All integer; HBM-bound streaming work.
//
// Data layout (per batch slot): gray u8 [h][gpitch]; sum i32 [(h+1)][spitch];
// sqsum [(h+1)][spitch] as a u32 low-word plane + a u8 high-byte plane (exact integers below 2^40 -> bit-identical to OpenCV's f64);
// band partials u32 [nbands][bpitch] for column sums of pixel and pixel^2.
#include "launch.h"

namespace nvca {

// ---- K3a: per-band column sums of lut[gray] and its square
__global__ __launch_bounds__(256) void k_colsum(const uint8_t *__restrict__ gray, const uint8_t *__restrict__ lut,
                                                int lut_stride, PreGeom g, unsigned *__restrict__ bandsum,
                                                unsigned *__restrict__ bandsq)
{
    __shared__ uint8_t sl[256];
    const int tid = threadIdx.x, band = blockIdx.y, slot = blockIdx.z;
    sl[tid] = lut ? lut[(size_t)slot * lut_stride + tid] : (uint8_t)tid;
    __syncthreads();
    const int x4 = (blockIdx.x * 256 + tid) * 4;
    const int bpitch = (int)(g.band_slot / g.nbands);
    if (x4 >= bpitch) return;
    const int y0 = band * kIntegralBand, y1 = min(g.h, y0 + kIntegralBand);
    unsigned s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    if (x4 < g.w) {
        const uint8_t *base = gray + (size_t)slot * g.gray_slot + x4;
        for (int y = y0; y < y1; y++) {
            const unsigned px = *(const unsigned *)(base + (size_t)y * g.gpitch);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned v = (x4 + k < g.w) ? sl[(px >> (8 * k)) & 255] : 0u;
                s[k] += v; q[k] += v * v;
            }
        }
    }
    const size_t o = (size_t)slot * g.band_slot + (size_t)band * bpitch + x4;
    *(uint4 *)(bandsum + o) = make_uint4(s[0], s[1], s[2], s[3]);
    *(uint4 *)(bandsq + o) = make_uint4(q[0], q[1], q[2], q[3]);
}
void launch_colsum(hipStream_t st, const uint8_t *gray, const uint8_t *lut, int lut_stride, const PreGeom &g,
                   unsigned *bandsum, unsigned *bandsq, int batch)
{
    const int bpitch = (int)(g.band_slot / g.nbands);
    dim3 grid((bpitch / 4 + 255) / 256, g.nbands, batch);
    NVCA_LAUNCH(k_colsum, grid, dim3(256), 0, st, gray, lut, lut_stride, g, bandsum, bandsq);
}

// ---- K3b: exclusive scan over bands, per column (in place)
__global__ __launch_bounds__(256) void k_bandscan(PreGeom g, unsigned *__restrict__ bandsum, unsigned *__restrict__ bandsq)
{
    const int bpitch = (int)(g.band_slot / g.nbands);
    const int x = blockIdx.x * 256 + threadIdx.x, slot = blockIdx.y;
    if (x >= bpitch) return;
    unsigned rs = 0, rq = 0;
    size_t o = (size_t)slot * g.band_slot + x;
    // 16 bands at a time: the loads of a chunk are all in flight before the first store (a load-add-store loop
    // serialises on the round trip: the stores may alias the next loads as far as the compiler knows)
    for (int b0 = 0; b0 < g.nbands; b0 += 16) {
        unsigned ts[16], tq[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const bool in = b0 + k < g.nbands;
            ts[k] = in ? bandsum[o + (size_t)k * bpitch] : 0u; tq[k] = in ? bandsq[o + (size_t)k * bpitch] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (b0 + k < g.nbands) {
                bandsum[o + (size_t)k * bpitch] = rs; bandsq[o + (size_t)k * bpitch] = rq;
                rs += ts[k]; rq += tq[k];
            }
        o += (size_t)16 * bpitch;
    }
}
void launch_bandscan(hipStream_t st, const PreGeom &g, unsigned *bandsum, unsigned *bandsq, int batch)
{
    const int bpitch = (int)(g.band_slot / g.nbands);
    NVCA_LAUNCH(k_bandscan, dim3((bpitch + 255) / 256, batch), dim3(256), 0, st, g, bandsum, bandsq);
}

// wave64 inclusive add-scan on the VALU (DPP row shifts inside each row of 16 lanes, then the three row totals
// through readlane): no LDS traffic, unlike ds_bpermute-based __shfl_up
__device__ __forceinline__ unsigned wave_incl_scan_u32(unsigned v, int lane)
{
    unsigned x = v;
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x113, 0xf, 0xf, true);   // row_shr:3
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xe, true);   // row_shr:4, lanes 4..15 of a row
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xc, true);   // row_shr:8, lanes 8..15
    const unsigned t0 = (unsigned)__builtin_amdgcn_readlane((int)x, 15), t1 = (unsigned)__builtin_amdgcn_readlane((int)x, 31),
                   t2 = (unsigned)__builtin_amdgcn_readlane((int)x, 47);
    const int row = lane >> 4;
    return x + (row >= 1 ? t0 : 0u) + (row >= 2 ? t1 : 0u) + (row >= 3 ? t2 : 0u);
}

// ---- K3c: integral + squared integral.  One block (512 threads) per band of rows; a block scans whole
// rows (4 integral columns per thread, 2048 per pass), keeps the vertical running sums in registers and
// writes one fully contiguous 16-byte vector per thread and plane: sum (i32) and the squared integral as
// two u32 planes (low / high word) -- 64-bit values written 8 B per column would leave every store
// instruction touching a quarter of each 64-byte sector (measured: 2.7 TB/s vs 3.7 TB/s for the sum plane).
// Thread t owns integral columns X in [4t, 4t+4): value(X) = prefix up to pixel X-1
// = exclusive base of the thread (X = 4t) or base + local inclusive (X > 4t).
static constexpr int kIntThreads = 512;
static constexpr int kIntWaves = kIntThreads / 64;

__global__ __launch_bounds__(kIntThreads) void k_integral(const uint8_t *__restrict__ gray, const uint8_t *__restrict__ lut,
                                                          int lut_stride, PreGeom g, const unsigned *__restrict__ bandsum,
                                                          const unsigned *__restrict__ bandsq, int *__restrict__ sum,
                                                          unsigned *__restrict__ sq32)
{
    __shared__ uint8_t sl[256];
    __shared__ unsigned wrow_s[kIntegralBand][kIntWaves], wrow_q[kIntegralBand][kIntWaves];
    __shared__ unsigned wb_s[kIntWaves];
    __shared__ unsigned long long wb_q[kIntWaves];
    __shared__ unsigned carry_s[kIntegralBand], carry_q[kIntegralBand];
    __shared__ unsigned cbase_s;
    __shared__ unsigned long long cbase_q;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int band = blockIdx.x, slot = blockIdx.y;
    if (tid < 256) sl[tid] = lut ? lut[(size_t)slot * lut_stride + tid] : (uint8_t)tid;
    if (tid < kIntegralBand) { carry_s[tid] = 0; carry_q[tid] = 0; }
    if (tid == 0) { cbase_s = 0; cbase_q = 0; }
    __syncthreads();
    const int y0 = band * kIntegralBand, y1 = min(g.h, y0 + kIntegralBand);
    const int bpitch = (int)(g.band_slot / g.nbands);
    const uint8_t *gbase = gray + (size_t)slot * g.gray_slot;
    int *sbase = sum + (size_t)slot * g.sum_slot;
    unsigned *lbase = sq32 + (size_t)slot * 2 * g.sum_slot;
    uint8_t *hbase = (uint8_t *)(lbase + g.sum_slot);        // high bytes (bits 32..39), one per element
    const unsigned *bs = bandsum + (size_t)slot * g.band_slot + (size_t)band * bpitch;
    const unsigned *bq = bandsq + (size_t)slot * g.band_slot + (size_t)band * bpitch;
    const int nchunks = (g.w + 1 + 2047) / 2048;

    for (int c = 0; c < nchunks; c++) {
        const int X0 = c * 2048 + tid * 4;
        const bool in_pitch = X0 < g.spitch;
        // ---- base row: prefix over x of the column sums above this band
        unsigned ps[4]; unsigned long long pq[4];
        {
            uint4 a = make_uint4(0, 0, 0, 0), e = make_uint4(0, 0, 0, 0);
            if (X0 + 4 <= bpitch) { a = *(const uint4 *)(bs + X0); e = *(const uint4 *)(bq + X0); }
            const unsigned vs[4] = {a.x, a.y, a.z, a.w}, vq[4] = {e.x, e.y, e.z, e.w};
            unsigned rs = 0; unsigned long long rq = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool ok = X0 + k < g.w;
                rs += ok ? vs[k] : 0u; rq += ok ? vq[k] : 0u;
                ps[k] = rs; pq[k] = rq;
            }
        }
        const unsigned ts = ps[3]; const unsigned long long tq = pq[3];
        unsigned is = wave_incl_scan_u32(ts + (tid == 0 ? cbase_s : 0u), lane);
        unsigned long long iq = tq + (tid == 0 ? cbase_q : 0ull);
        for (int d = 1; d < 64; d <<= 1) { const unsigned long long b = __shfl_up(iq, d); if (lane >= d) iq += b; }
        if (lane == 63) { wb_s[wave] = is; wb_q[wave] = iq; }
        __syncthreads();
        for (int j = 0; j < wave; j++) { is += wb_s[j]; iq += wb_q[j]; }
        unsigned acc_s[4]; unsigned long long acc_q[4];
        {
            const unsigned es = is - ts; const unsigned long long eq = iq - tq;
            acc_s[0] = es; acc_q[0] = eq;
#pragma unroll
            for (int k = 1; k < 4; k++) { acc_s[k] = es + ps[k - 1]; acc_q[k] = eq + pq[k - 1]; }
        }
        __syncthreads();                                   // wb_* consumed
        if (tid == kIntThreads - 1) { cbase_s = is; cbase_q = iq; }
        if (band == 0 && in_pitch) {                        // integral row 0 (all zero)
            *(int4 *)(sbase + X0) = make_int4(0, 0, 0, 0);
            *(uint4 *)(lbase + X0) = make_uint4(0, 0, 0, 0);
            *(unsigned *)(hbase + X0) = 0u;
        }
        // ---- rows of the band.  All rows' pixels are requested at once; every row's prefix over x is scanned inside the waves
        // (DPP), the wave totals of all rows are exchanged through LDS behind ONE barrier (it was one per row), and the
        // vertical running sums are then carried and stored row by row without further synchronisation.
        const int nr = y1 - y0;
        unsigned px[kIntegralBand];
#pragma unroll
        for (int r = 0; r < kIntegralBand; r++)
            px[r] = (X0 < g.w && r < nr) ? *(const unsigned *)(gbase + (size_t)(y0 + r) * g.gpitch + X0) : 0u;
        unsigned inc_s[kIntegralBand], inc_q[kIntegralBand];          // inclusive prefix (inside the wave) of the thread totals, per row
#pragma unroll
        for (int r = 0; r < kIntegralBand; r++) {
            unsigned rs = 0, rq = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned v = (X0 + k < g.w) ? (unsigned)sl[(px[r] >> (8 * k)) & 255] : 0u;
                rs += v; rq += v * v;
            }
            inc_s[r] = wave_incl_scan_u32(rs, lane); inc_q[r] = wave_incl_scan_u32(rq, lane);
            if (lane == 63) { wrow_s[r][wave] = inc_s[r]; wrow_q[r][wave] = inc_q[r]; }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kIntegralBand; r++) {
            if (r < nr) {
            // exclusive prefix of this thread in row r: the chunks to the left (carry), the waves to the left, the lanes to the left
            unsigned e_s = carry_s[r], e_q = carry_q[r];
            for (int j = 0; j < wave; j++) { e_s += wrow_s[r][j]; e_q += wrow_q[r][j]; }
            unsigned ls[4], lq[4];
            unsigned rs = 0, rq = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned v = (X0 + k < g.w) ? (unsigned)sl[(px[r] >> (8 * k)) & 255] : 0u;
                rs += v; rq += v * v;
                ls[k] = rs; lq[k] = rq;
            }
            e_s += inc_s[r] - rs; e_q += inc_q[r] - rq;
            acc_s[0] += e_s; acc_q[0] += e_q;
#pragma unroll
            for (int k = 1; k < 4; k++) { acc_s[k] += e_s + ls[k - 1]; acc_q[k] += e_q + lq[k - 1]; }
            if (in_pitch) {
                const size_t o = (size_t)(y0 + r + 1) * g.spitch + X0;
                *(int4 *)(sbase + o) = make_int4((int)acc_s[0], (int)acc_s[1], (int)acc_s[2], (int)acc_s[3]);
                *(uint4 *)(lbase + o) = make_uint4((unsigned)acc_q[0], (unsigned)acc_q[1], (unsigned)acc_q[2], (unsigned)acc_q[3]);
                *(unsigned *)(hbase + o) = (unsigned)(acc_q[0] >> 32) | ((unsigned)(acc_q[1] >> 32) << 8) | ((unsigned)(acc_q[2] >> 32) << 16) |
                                           ((unsigned)(acc_q[3] >> 32) << 24);
            }
            }
        }
        __syncthreads();                                   // wrow_* and carry_* consumed
        if (tid < kIntegralBand) {                          // this chunk's row totals join the carries (images wider than one chunk)
            unsigned ts_ = 0, tq_ = 0;
            for (int j = 0; j < kIntWaves; j++) { ts_ += wrow_s[tid][j]; tq_ += wrow_q[tid][j]; }
            carry_s[tid] += ts_; carry_q[tid] += tq_;
        }
        __syncthreads();
    }
}
void launch_integral(hipStream_t st, const uint8_t *gray, const uint8_t *lut, int lut_stride, const PreGeom &g,
                     const unsigned *bandsum, const unsigned *bandsq, int *sum, unsigned long long *sqsum,
                     int batch)
{
    NVCA_LAUNCH(k_integral, dim3(g.nbands, batch), dim3(kIntThreads), 0, st, gray, lut, lut_stride, g, bandsum,
                       bandsq, sum, (unsigned *)sqsum);
}

// ---- CV_HAAR_SCALE_IMAGE pyramids: every level of every image in one launch per step -----------------------------
// The levels of a pyramid are small (the part detectors work at 320 pixels width) and there are ~15 of them: resizing
// and integrating them one level at a time is a chain of ~60 tiny dependent launches.  k_pyr_resize writes all levels
// (grid.z = level x image); k_pyr_integral gives each (level, image) one workgroup that walks the rows with one column
// per thread: running column sums in registers, one workgroup-wide scan per row (sum i32, squared sum u64 -> two u32
// planes, same layout as k_integral).  Levels wider than 1024 pixels take the general three-kernel path.
// Integral pair of a SMALL image (rows x (cols | 1) <= kSmallIntWords words of LDS) by one workgroup, without a barrier per
// row: (1) every wave scans whole rows -- 64 pixels per step, DPP wave scan, carry from chunk to chunk -- and leaves the row
// prefix sums in LDS; (2) after one barrier every thread owns a column and adds the rows up out of LDS, writing the
// integral rows to global memory fully coalesced.  Once for the pixel sums, once for their squares (row prefixes of squares
// stay below 2^32; the column sums are 64-bit and leave as the u32 low-word plane + u8 high-byte plane of k_integral).
// 160 x 90 (the part detectors' face-pass image): ~3 us instead of ~36 us for the row-by-row walk below.
static constexpr int kSmallIntWords = 16 * 1024 - 256;     // dynamic LDS: with the static scan words still inside the 64 KiB a kernel gets without asking
__device__ __forceinline__ void small_integral(const uint8_t *__restrict__ g, int gpitch, const uint8_t *__restrict__ lut, int w, int h,
                                               int *__restrict__ s, unsigned *__restrict__ lo, uint8_t *__restrict__ hi, int P, unsigned *sm)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, nwaves = nthreads >> 6;
    const int pitch = w | 1;
    for (int X = tid; X <= w; X += nthreads) { s[X] = 0; lo[X] = 0; hi[X] = 0; }            // integral row 0
    for (int pass = 0; pass < 2; pass++) {
        for (int y = wave; y < h; y += nwaves) {
            const uint8_t *row = g + (size_t)y * gpitch;
            unsigned carry = 0;
            for (int x0 = 0; x0 < w; x0 += 64) {
                const int x = x0 + lane;
                unsigned v = 0;
                if (x < w) { v = row[x]; if (lut) v = lut[v]; if (pass) v *= v; }
                const unsigned inc = wave_incl_scan_u32(v, lane) + carry;
                if (x < w) sm[y * pitch + x] = inc;
                carry = (unsigned)__builtin_amdgcn_readlane((int)inc, 63);
            }
        }
        __syncthreads();
        for (int x = tid; x < w; x += nthreads) {
            if (pass == 0) {
                unsigned acc = 0;
                for (int y = 0; y < h; y++) { acc += sm[y * pitch + x]; s[(size_t)(y + 1) * P + x + 1] = (int)acc; }
            } else {
                unsigned long long acc = 0;
                for (int y = 0; y < h; y++) {
                    acc += sm[y * pitch + x];
                    const size_t o = (size_t)(y + 1) * P + x + 1;
                    lo[o] = (unsigned)acc; hi[o] = (uint8_t)(acc >> 32);
                }
            }
        }
        if (pass == 0) for (int y = tid; y < h; y += nthreads) { const size_t o = (size_t)(y + 1) * P; s[o] = 0; lo[o] = 0; hi[o] = 0; }   // column 0
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void k_pyr_integral(const uint8_t *__restrict__ aux, size_t aux_slot,
                                                       const PyrLevelDev *__restrict__ levels, int nimg,
                                                       int *__restrict__ sum, unsigned *__restrict__ sq32, size_t sum_slot, int P)
{
    extern __shared__ unsigned pyr_sm[];
    __shared__ unsigned wt_s[2][16], wt_l[2][16], wt_h[2][16];
    const int lev = blockIdx.x / nimg, img = blockIdx.x - lev * nimg;
    const PyrLevelDev L = levels[lev];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, w = L.szw, h = L.szh;
    const uint8_t *g = aux + (size_t)img * aux_slot + L.gray_off;
    int *s = sum + (size_t)img * sum_slot + L.plane_off;
    unsigned *lo = sq32 + (size_t)img * 2 * sum_slot + L.plane_off;
    uint8_t *hi = (uint8_t *)(sq32 + (size_t)img * 2 * sum_slot + sum_slot) + L.plane_off;   // high-byte plane
    if (h * (w | 1) <= kSmallIntWords) { small_integral(g, L.gpitch, nullptr, w, h, s, lo, hi, P, pyr_sm); return; }
    if (tid <= w) { s[tid] = 0; lo[tid] = 0; hi[tid] = 0; }            // integral row 0
    // running sums of this thread's column; the squared one stays below 2^32 (rows x 255^2), so its row prefix can be
    // scanned as two 32-bit halves (low 16 bits / the rest) on the VALU and recombined in 64 bits
    unsigned cs = 0, cq = 0;
    unsigned pix = (tid < w && h > 0) ? g[tid] : 0;
    int par = 0;
    for (int y = 0; y < h; y++) {
        const unsigned cur = pix;
        if (tid < w && y + 1 < h) pix = g[(size_t)(y + 1) * L.gpitch + tid];      // next row in flight during the scan
        cs += cur; cq += cur * cur;
        unsigned is = wave_incl_scan_u32(cs, lane);
        unsigned il = wave_incl_scan_u32(cq & 0xffffu, lane), ih = wave_incl_scan_u32(cq >> 16, lane);
        if (lane == 63) { wt_s[par][wave] = is; wt_l[par][wave] = il; wt_h[par][wave] = ih; }
        __syncthreads();
        for (int j = 0; j < wave; j++) { is += wt_s[par][j]; il += wt_l[par][j]; ih += wt_h[par][j]; }
        par ^= 1;
        const unsigned long long iq = ((unsigned long long)ih << 16) + il;
        const size_t row = (size_t)(y + 1) * P;
        if (tid < w) { s[row + tid + 1] = (int)is; lo[row + tid + 1] = (unsigned)iq; hi[row + tid + 1] = (uint8_t)(iq >> 32); }
        if (tid == 0) { s[row] = 0; lo[row] = 0; hi[row] = 0; }
    }
}

// one small image per workgroup (batch slots), the planes laid out like k_integral's: the ROI-sized images of the part
// detectors' FIND_BIGGEST searches take one launch instead of column sums + band scan + row pass
__global__ __launch_bounds__(1024) void k_small_integral(const uint8_t *__restrict__ gray, const uint8_t *__restrict__ lut, int lut_stride, PreGeom g,
                                                         int *__restrict__ sum, unsigned *__restrict__ sq32)
{
    extern __shared__ unsigned pyr_sm[];
    const int slot = blockIdx.x;
    unsigned *lo = sq32 + (size_t)slot * 2 * g.sum_slot;
    small_integral(gray + (size_t)slot * g.gray_slot, g.gpitch, lut ? lut + (size_t)slot * lut_stride : nullptr, g.w, g.h,
                   sum + (size_t)slot * g.sum_slot, lo, (uint8_t *)(lo + g.sum_slot), g.spitch, pyr_sm);
}
bool small_integral_fits(const PreGeom &g) { return g.h * (g.w | 1) <= kSmallIntWords; }
void launch_small_integral(hipStream_t st, const uint8_t *gray, const uint8_t *lut, int lut_stride, const PreGeom &g, int *sum,
                           unsigned long long *sqsum, int batch)
{
    NVCA_LAUNCH(k_small_integral, dim3(batch), dim3(1024), (size_t)g.h * (g.w | 1) * sizeof(unsigned), st, gray, lut, lut_stride, g, sum, (unsigned *)sqsum);
}

// ---- tilted integral: cv::integral's third plane, read by tilted Haar features ------------------------------------------
// tilted(X,Y) = sum of image(x,y) over y < Y, abs(x - X + 1) <= Y - y - 1  (int32, (h+1) x (w+1), row 0 zero).
// Row Y of the triangle under (X,Y) differs from row Y-1's by the apex pixel (X-1,Y-1) and by its two end pixels per
// earlier row, which lie on the diagonals through (X-2,Y-2) and (X,Y-2): dl[c - y] / dr[c + y] are running sums along the two
// diagonal families.  One workgroup per image walks the rows; thread X reads its two diagonal sums (as of row Y-2), emits
// tilted(X,Y), then adds pixel (X-1,Y-1) to exactly those two sums -- the element a thread reads in a row is the one it
// updates, so one barrier per row orders everything.  Serial in the rows (cheap: the path is only taken for cascades that
// hold tilted features, on the small working images of the part detectors); exact 32-bit integer arithmetic.
static constexpr int kTiltedCols = 8;                 // columns per thread: w + 1 <= 8 * 1024
__device__ __forceinline__ void tilted_image(const uint8_t *__restrict__ g, int gpitch, const uint8_t *__restrict__ lut, int w, int h,
                                             int *__restrict__ out, int opitch, int *dl, int *dr)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < w + h + 2; i += 1024) { dl[i] = 0; dr[i] = 0; }
    for (int X = tid; X <= w; X += 1024) out[X] = 0;
    int prev[kTiltedCols];
#pragma unroll
    for (int k = 0; k < kTiltedCols; k++) prev[k] = 0;
    __syncthreads();
    for (int Y = 1; Y <= h; Y++) {
        const uint8_t *row = g + (size_t)(Y - 1) * gpitch;
#pragma unroll
        for (int k = 0; k < kTiltedCols; k++) {
            const int X = tid + 1024 * k;
            if (X > w) break;
            int p = 0;
            if (X >= 1) { p = row[X - 1]; if (lut) p = lut[p]; }
            int v = prev[k] + p;
            const int il = X - Y + h, ir = X + Y - 2;         // dl index of diagonal c - y = X - Y (shifted by h), dr index of c + y
            if (Y >= 2) {
                if (X >= 2) v += dl[il];
                if (X < w) v += dr[ir];
            }
            if (X >= 1) { dl[il] += p; dr[ir] += p; }
            out[(size_t)Y * opitch + X] = v;
            prev[k] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void k_tilted(const uint8_t *__restrict__ gray, const uint8_t *__restrict__ lut, int lut_stride, PreGeom g,
                                                 int *__restrict__ tilted)
{
    extern __shared__ int tl_lds[];
    const int slot = blockIdx.x;
    tilted_image(gray + (size_t)slot * g.gray_slot, g.gpitch, lut ? lut + (size_t)slot * lut_stride : nullptr, g.w, g.h,
                 tilted + (size_t)slot * g.sum_slot, g.spitch, tl_lds, tl_lds + g.w + g.h + 2);
}

__global__ __launch_bounds__(1024) void k_pyr_tilted(const uint8_t *__restrict__ aux, size_t aux_slot, const PyrLevelDev *__restrict__ levels,
                                                     int nimg, int *__restrict__ tilted, size_t sum_slot, int P, int lds_half)
{
    extern __shared__ int tl_lds[];
    const int lev = blockIdx.x / nimg, img = blockIdx.x - lev * nimg;
    const PyrLevelDev L = levels[lev];
    tilted_image(aux + (size_t)img * aux_slot + L.gray_off, L.gpitch, nullptr, L.szw, L.szh,
                 tilted + (size_t)img * sum_slot + L.plane_off, P, tl_lds, tl_lds + lds_half);
}

void launch_tilted(hipStream_t st, const uint8_t *gray, const uint8_t *lut, int lut_stride, const PreGeom &g, int *tilted, int batch)
{
    NVCA_LAUNCH(k_tilted, dim3(batch), dim3(1024), (size_t)2 * (g.w + g.h + 2) * sizeof(int), st, gray, lut, lut_stride, g, tilted);
}
void launch_pyr_tilted(hipStream_t st, const uint8_t *aux, size_t aux_slot, const PyrLevelDev *levels, int nlev, int nimg,
                       int *tilted, size_t sum_slot, int P, int maxw, int maxh)
{
    const int half = maxw + maxh + 2;
    NVCA_LAUNCH(k_pyr_tilted, dim3(nlev * nimg), dim3(1024), (size_t)2 * half * sizeof(int), st, aux, aux_slot, levels, nimg, tilted, sum_slot, P, half);
}

void launch_pyr_integral(hipStream_t st, const uint8_t *aux, size_t aux_slot, const PyrLevelDev *levels, int nlev, int nimg,
                         int *sum, unsigned *sq32, size_t sum_slot, int P)
{
    // dynamic LDS: the row prefix sums of the largest level that takes the LDS-resident path (64 KiB at most)
    NVCA_LAUNCH(k_pyr_integral, dim3(nlev * nimg), dim3(1024), (size_t)kSmallIntWords * sizeof(unsigned), st, aux, aux_slot, levels, nimg, sum, sq32, sum_slot, P);
}

} // namespace nvca
