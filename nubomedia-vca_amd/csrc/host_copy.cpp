// host_copy.cpp -- caller host memory <-> device: the page-locked staging ring and its copies, 2-D staging of images, and the
// staging of a batch's source frames.
#include "host_state.h"
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <thread>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

using namespace nvca;

namespace nvca {

// ---- caller host memory -------------------------------------------------------------------------------------------------------
// A caller's host pointer reaches the HIP runtime as it stands ONLY while the memory lies inside a range the caller page-locked
// through nvca_host_register (ctx->host_ranges): a copy of pageable memory makes the runtime pin the caller's pages behind the
// library's back, and under PyTorch's bundled ROCm 7.0 runtime exactly such a copy -- a 97 x 83 numpy image, two tests after frames
// of the same heap had been page-locked and released again -- ended now and then in "Memory access fault by GPU ... on address <a
// page of the host heap>" (DESIGN 6a).  Whatever the runtime remembers about host ranges it has seen, the library does not depend
// on it: everything else is copied by the CPU into / out of page-locked slots of the context's own (ctx->bounce) and crosses
// from there.  A slot carries the event of the last copy that used it and is waited for before it is used again, so the CPU
// copy of piece k + 1 runs beside the DMA of piece k.
static int stream_id(const nvca_ctx *ctx, hipStream_t st)
{
    for (int l = 0; l < kLanes; l++) if (st == ctx->lane_streams[l]) return l;
    if (st == ctx->copy_stream) return kLanes;
    return 63;
}
hipStream_t stream_of_id(const nvca_ctx *ctx, int id)
{
    if (id < kLanes) return ctx->lane_streams[id];
    if (id == kLanes) return ctx->copy_stream;
    return nullptr;
}
static int bounce_take(nvca_ctx *ctx, uint8_t **p, int *slot)
{
    BounceRing &b = ctx->bounce;
    if (!b.buf.p) {
        if (b.buf.ensure(BounceRing::kSlot * BounceRing::kSlots)) { (void)hipGetLastError(); ctx->set_error("allocation failed (page-locked staging)"); return NVCA_ERR_NOMEM; }
        for (hipEvent_t &e : b.ev) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { ctx->set_error("hipEventCreate failed (page-locked staging)"); return NVCA_ERR_HIP; }
    }
    const int k = b.next;
    b.next = (k + 1) % BounceRing::kSlots;
    if (b.pending[k]) { NVCA_HIP_CHECK(ctx, hipEventSynchronize(b.ev[k])); b.pending[k] = false; }
    *p = b.buf.as<uint8_t>() + (size_t)k * BounceRing::kSlot; *slot = k;
    return NVCA_OK;
}
static int bounce_used(nvca_ctx *ctx, int slot, hipStream_t st)
{
    NVCA_HIP_CHECK(ctx, hipEventRecord(ctx->bounce.ev[slot], st));
    ctx->bounce.pending[slot] = true;
    return NVCA_OK;
}
// large pieces are copied by the context's helper threads too (the PCIe link moves ~50 GB/s; one core's memcpy a fifth of that): as
// many equal parts as there are threads, none below 256 KB
// A large piece on its way INTO a page-locked slot is written once and next read by the DMA engine, never by this core: streaming
// stores (no read-for-ownership of the destination lines, no pollution of the caches with 6 MB a frame).  memcpy picks them only
// above a threshold that a thread's share of a frame does not reach.  NVCA_NT_COPY=0: plain memcpy.
static void copy_streaming(uint8_t *d, const uint8_t *s, size_t n)
{
#if defined(__SSE2__)
    static const bool on = [] { const char *e = getenv("NVCA_NT_COPY"); return !(e && e[0] == '0'); }();
    if (on && n >= (64u << 10)) {
        size_t head = (size_t)(-(intptr_t)d) & 15;
        memcpy(d, s, head); d += head; s += head; n -= head;
        const size_t blocks = n / 64;
        for (size_t i = 0; i < blocks; i++, s += 64, d += 64) {
            const __m128i a = _mm_loadu_si128((const __m128i *)s), b = _mm_loadu_si128((const __m128i *)(s + 16)),
                          c = _mm_loadu_si128((const __m128i *)(s + 32)), e = _mm_loadu_si128((const __m128i *)(s + 48));
            _mm_stream_si128((__m128i *)d, a); _mm_stream_si128((__m128i *)(d + 16), b);
            _mm_stream_si128((__m128i *)(d + 32), c); _mm_stream_si128((__m128i *)(d + 48), e);
        }
        _mm_sfence();
        n -= blocks * 64;
    }
#endif
    memcpy(d, s, n);
}
static void host_copy(nvca_ctx *ctx, void *dst, const void *src, size_t bytes, bool into_slot = false)
{
    static constexpr size_t kMinPart = 256u << 10;
    const int threads = work_pool_threads(ctx->pool) + 1;
    const int parts = (int)std::min<size_t>((size_t)threads, bytes / kMinPart);
    if (parts < 4 || !ctx->pool) { if (into_slot) copy_streaming((uint8_t *)dst, (const uint8_t *)src, bytes); else memcpy(dst, src, bytes); return; }
    struct Arg { uint8_t *d; const uint8_t *s; size_t n, part; bool nt; } arg{(uint8_t *)dst, (const uint8_t *)src, bytes, ((bytes + parts - 1) / parts + 63) & ~(size_t)63, into_slot};
    work_pool_run(ctx->pool, parts, [](void *a, int i) {
        const Arg *g = (const Arg *)a;
        const size_t o = (size_t)i * g->part;
        if (o >= g->n) return;
        if (g->nt) copy_streaming(g->d + o, g->s + o, std::min(g->part, g->n - o)); else memcpy(g->d + o, g->s + o, std::min(g->part, g->n - o));
    }, &arg);
}
void ensure_pool(nvca_ctx *ctx)
{
    if (ctx->pool || ctx->pool_tried) return;
    ctx->pool_tried = true;
    int t = ctx->sw.host_threads;
    if (t < 0) { const int hc = (int)std::thread::hardware_concurrency(); t = std::min(8, hc / 2) - 1; }
    ctx->pool = work_pool_create(t);
}
int caller_h2d(nvca_ctx *ctx, void *dst, const void *src, size_t bytes, hipStream_t st)
{
    if (!bytes) return NVCA_OK;
    if (ctx->host_ranges.note_copy(src, bytes, stream_id(ctx, st))) {
        NVCA_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
        return NVCA_OK;
    }
    if (bytes >= (1u << 20)) ensure_pool(ctx);
    for (size_t o = 0; o < bytes; o += BounceRing::kSlot) {
        const size_t len = std::min(BounceRing::kSlot, bytes - o);
        uint8_t *h; int slot, rc;
        if ((rc = bounce_take(ctx, &h, &slot))) return rc;
        host_copy(ctx, h, (const uint8_t *)src + o, len, true);
        NVCA_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)dst + o, h, len, hipMemcpyHostToDevice, st));
        if ((rc = bounce_used(ctx, slot, st))) return rc;
    }
    return NVCA_OK;
}
// rows of `width` bytes, spitch apart in the caller's memory, to rows dpitch apart on the device
int caller_h2d_rows(nvca_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipStream_t st)
{
    if (!rows || !width) return NVCA_OK;
    if (width > BounceRing::kSlot) { ctx->set_error("row too long for the page-locked staging"); return NVCA_ERR_ARG; }
    if (ctx->host_ranges.note_copy(src, spitch * (rows - 1) + width, stream_id(ctx, st))) {
        NVCA_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyHostToDevice, st));
        return NVCA_OK;
    }
    const size_t per = std::max<size_t>(1, BounceRing::kSlot / width);
    for (size_t r0 = 0; r0 < rows; r0 += per) {
        const size_t nr = std::min(per, rows - r0);
        uint8_t *h; int slot, rc;
        if ((rc = bounce_take(ctx, &h, &slot))) return rc;
        if (spitch == width) host_copy(ctx, h, (const uint8_t *)src + r0 * spitch, nr * width, true);
        else for (size_t y = 0; y < nr; y++) memcpy(h + y * width, (const uint8_t *)src + (r0 + y) * spitch, width);
        if (dpitch == width) NVCA_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t *)dst + r0 * dpitch, h, nr * width, hipMemcpyHostToDevice, st));
        else NVCA_HIP_CHECK(ctx, hipMemcpy2DAsync((uint8_t *)dst + r0 * dpitch, dpitch, h, width, width, nr, hipMemcpyHostToDevice, st));
        if ((rc = bounce_used(ctx, slot, st))) return rc;
    }
    return NVCA_OK;
}
int caller_d2h_rows(nvca_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows, hipStream_t st)
{
    if (!rows || !width) { NVCA_HIP_CHECK(ctx, hipStreamSynchronize(st)); return NVCA_OK; }
    if (width > BounceRing::kSlot) { ctx->set_error("row too long for the page-locked staging"); return NVCA_ERR_ARG; }
    if (ctx->host_ranges.note_copy(dst, dpitch * (rows - 1) + width, stream_id(ctx, st))) {
        NVCA_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToHost, st));
        NVCA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        return NVCA_OK;
    }
    const size_t per = std::max<size_t>(1, BounceRing::kSlot / width);
    for (size_t r0 = 0; r0 < rows; r0 += per) {
        const size_t nr = std::min(per, rows - r0);
        uint8_t *h; int slot, rc;
        if ((rc = bounce_take(ctx, &h, &slot))) return rc;
        if (spitch == width) NVCA_HIP_CHECK(ctx, hipMemcpyAsync(h, (const uint8_t *)src + r0 * spitch, nr * width, hipMemcpyDeviceToHost, st));
        else NVCA_HIP_CHECK(ctx, hipMemcpy2DAsync(h, width, (const uint8_t *)src + r0 * spitch, spitch, width, nr, hipMemcpyDeviceToHost, st));
        NVCA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        for (size_t y = 0; y < nr; y++) memcpy((uint8_t *)dst + (r0 + y) * dpitch, h + y * width, width);
    }
    return NVCA_OK;
}
// copy a host/device 2-D byte image into device memory with a pitch
int stage_2d(nvca_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes,
             size_t height, int mem)
{
    if (mem == NVCA_MEM_HOST) return caller_h2d_rows(ctx, dst, dpitch, src, spitch, width_bytes, height, ctx->cs());
    NVCA_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, height, hipMemcpyDeviceToDevice, ctx->cs()));
    return NVCA_OK;
}
int unstage_2d(nvca_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes,
               size_t height, int mem)
{
    NVCA_LAUNCH_CHECK(ctx);
    if (mem == NVCA_MEM_HOST) {
        const int rc = caller_d2h_rows(ctx, dst, dpitch, src, spitch, width_bytes, height, ctx->cs());
        if (!rc) drain_timer(ctx);
        return rc;
    }
    NVCA_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, height, hipMemcpyDeviceToDevice, ctx->cs()));
    if (ctx->defer_device_sync > 0) return NVCA_OK;   // consumer is queued on the same stream
    NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    drain_timer(ctx);
    return NVCA_OK;
}

// end of a primitive that wrote device memory directly
int finish_device_op(nvca_ctx *ctx)
{
    NVCA_LAUNCH_CHECK(ctx);
    if (ctx->defer_device_sync > 0) return NVCA_OK;
    NVCA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->cs()));
    drain_timer(ctx);
    return NVCA_OK;
}

int check_img(nvca_ctx *ctx, const void *p, int w, int h, int stride, int bpp, int mem)
{
    if (!ctx || !p || w <= 0 || h <= 0 || stride < w * bpp || (mem != NVCA_MEM_HOST && mem != NVCA_MEM_DEVICE)) return NVCA_ERR_ARG;
    return NVCA_OK;
}

// ---- 4:2:0 and packed 4:2:2 layouts (nvca_pixel_layout); the planes' rows, bytes, the frame's extent and the layout rules
// (yuv_layout_fault): yuv_layout.h
int check_yuv_layout(nvca_ctx *ctx, const nvca_pixel_layout &l, int w, int h)
{
    const char *fault = yuv_layout_fault(l, w, h);
    if (!fault) return NVCA_OK;
    if (ctx) ctx->set_error(fault);
    return NVCA_ERR_ARG;
}
// nvca_*_set_input: the caller's layout, validated, as the stream keeps it (null / NVCA_PIX_BGR: packed frames).  What the format
// does not use stays zero: layouts compare by value.
int parse_pixel_layout(nvca_ctx *ctx, const nvca_pixel_layout *layout, nvca_pixel_layout &out)
{
    nvca_pixel_layout in{};
    if (layout && layout->format != NVCA_PIX_BGR) {
        if (!yuv_is_420(layout->format) && !yuv_is_422(layout->format)) { ctx->set_error("pixel layout: format must be NVCA_PIX_BGR, NVCA_PIX_NV12, NVCA_PIX_I420, NVCA_PIX_YUY2, NVCA_PIX_UYVY or NVCA_PIX_YVYU"); return NVCA_ERR_ARG; }
        in.format = layout->format;
        for (int p = 0; p < yuv_planes_of(*layout); p++) {
            if (layout->stride[p] <= 0) { ctx->set_error("pixel layout: plane strides must be positive"); return NVCA_ERR_ARG; }
            in.offset[p] = layout->offset[p]; in.stride[p] = layout->stride[p];
        }
    }
    out = in;
    return NVCA_OK;
}
// a frame of a 4:2:0 / 4:2:2 stream against the stream's layout
int check_yuv_frame(nvca_ctx *ctx, const nvca_pixel_layout &l, const nvca_frame &f)
{
    if (!f.data || (f.mem != NVCA_MEM_HOST && f.mem != NVCA_MEM_DEVICE)) return NVCA_ERR_ARG;
    if (check_yuv_layout(ctx, l, f.width, f.height)) return NVCA_ERR_ARG;
    if (f.stride != l.stride[0]) { if (ctx) ctx->set_error(yuv_is_422(l.format) ? "4:2:2 frame: its stride is not the stride[0] of the stream's layout" : "4:2:0 frame: its stride is not the stride[0] of the stream's layout"); return NVCA_ERR_ARG; }
    return NVCA_OK;
}
// a host 4:2:0 frame to device memory, plane by plane, each at the caller's offset (gaps between planes are not copied); `dst` holds
// yuv_extent() bytes
int caller_h2d_planes(nvca_ctx *ctx, void *dst, const void *src, const nvca_pixel_layout &l, int w, int h, hipStream_t st)
{
    for (int p = 0; p < yuv_planes_of(l); p++)
        if (int rc = caller_h2d(ctx, (uint8_t *)dst + l.offset[p], (const uint8_t *)src + l.offset[p], yuv_plane_bytes(l, p, w, h), st)) return rc;
    return NVCA_OK;
}
YuvPlanes yuv_planes(const nvca_pixel_layout *l)
{
    YuvPlanes p{};
    if (!l || l->format == NVCA_PIX_BGR) return p;
    p.fmt = l->format; p.cstride = l->stride[1]; p.vstride = l->stride[2];
    p.off_y = (long long)l->offset[0]; p.off_u = (long long)l->offset[1]; p.off_v = (long long)l->offset[2];
    return p;
}

// stage `n` source frames (host or device) and return device pointers in ws.srcptrs
// yuv: the frames are 4:2:0 / 4:2:2 buffers of this layout (staged with their planes at the caller's offsets)
size_t staging_need(const nvca_frame *frames, const int *idx, int n, const nvca_pixel_layout *yuv)
{
    size_t need = 0;
    for (int i = 0; i < n; i++) {
        const nvca_frame &f = frames[idx ? idx[i] : i];
        if (f.mem == NVCA_MEM_HOST) need += round_up(yuv ? yuv_extent(*yuv, f.width, f.height) : (size_t)f.stride * f.height, 256);
    }
    return need;
}

// Rows [first + k * period, + run), k < count, of a host image plane (`rows` rows of `row_bytes` bytes, `stride` apart) to the same
// places of its staged copy: one strided 2-D copy; a run that ends on the plane's last row is copied without the row padding (the
// caller's buffer need not extend past the last pixel)
static int copy_row_runs(nvca_ctx *ctx, uint8_t *d, const uint8_t *s, size_t stride, size_t row_bytes, size_t rows,
                         size_t first, size_t period, size_t run, size_t count, hipStream_t st)
{
    RowPiece pc[2];
    const int np = row_run_pieces(stride, row_bytes, rows, first, period, run, count, pc);
    for (int k = 0; k < np; k++) {
        int rc;
        if (pc[k].n == 1) rc = caller_h2d(ctx, d + pc[k].off, s + pc[k].off, pc[k].width, st);          // one run: no pitch to speak of
        else rc = caller_h2d_rows(ctx, d + pc[k].off, pc[k].pitch, s + pc[k].off, pc[k].pitch, pc[k].width, pc[k].n, st);
        if (rc) return rc;
    }
    return NVCA_OK;
}
// the chroma rows that the luma rows of `rows` use, of one chroma plane: row r uses chroma row r >> 1
static int copy_chroma_runs(nvca_ctx *ctx, uint8_t *d, const uint8_t *s, size_t stride, size_t row_bytes, size_t plane_rows,
                            const RowCopy &rows, hipStream_t st)
{
    const int c0 = rows.first >> 1, c1 = (rows.first + rows.run - 1) >> 1;
    if (!(rows.period & 1) || rows.count == 1)              // an even period: the chroma runs are as regular as the luma runs
        return copy_row_runs(ctx, d, s, stride, row_bytes, plane_rows, (size_t)c0, (size_t)std::max(rows.period / 2, 1), (size_t)(c1 - c0 + 1), (size_t)rows.count, st);
    int done = -1, rc;                                       // an odd period: run by run, no chroma row twice
    for (int k = 0; k < rows.count; k++) {
        const int a = std::max((rows.first + k * rows.period) >> 1, done + 1), b = (rows.first + k * rows.period + rows.run - 1) >> 1;
        if (b < a) continue;
        if ((rc = copy_row_runs(ctx, d, s, stride, row_bytes, plane_rows, (size_t)a, 1, (size_t)(b - a + 1), 1, st))) return rc;
        done = b;
    }
    return NVCA_OK;
}

// frame pointers of n frames -> device pointer array entries [r0, r0 + n); host frames are copied into the staging
// buffer first (from byte offset *off on, advanced).  `st`: the stream the copies are queued on.
int stage_frames(nvca_ctx *ctx, const nvca_frame *frames, const int *idx, int n, int bpp, int r0, hipStream_t st, size_t *off_io,
                 const RowCopy *rows, const nvca_pixel_layout *yuv)
{
    const bool sparse_off = !ctx->sw.sparse_ingest;
    if (sparse_off || (rows && !rows->on)) rows = nullptr;
    Workspace &ws = *ctx->ws;
    if (!st) st = ctx->cs();
    if (!off_io) {           // stand-alone call: size the buffers here
        if (ws.res[ws.cur_res].srcptrs.ensure((size_t)(r0 + n) * sizeof(void *)) || ws.res[ws.cur_res].h_srcptrs.ensure((size_t)(r0 + n) * sizeof(void *))) {
            ctx->set_error("allocation failed"); return NVCA_ERR_NOMEM;
        }
        const size_t need = staging_need(frames, idx, n, yuv);
        if (need && ws.res[ws.cur_res].staging.ensure(need)) { ctx->set_error("allocation failed (frame staging)"); return NVCA_ERR_NOMEM; }
    }
    const void **hp = ws.res[ws.cur_res].h_srcptrs.as<const void *>() + r0;
    size_t off = off_io ? *off_io : 0;
    for (int i = 0; i < n; i++) {
        const nvca_frame &f = frames[idx ? idx[i] : i];
        if (f.mem == NVCA_MEM_HOST) {
            uint8_t *d = ws.res[ws.cur_res].staging.as<uint8_t>() + off;
            int rc;
            if (yuv) {
                // plane by plane, each at the caller's offset: whole planes (the staging every 4:2:0 element shares), or the luma rows
                // the resize reads and exactly the chroma rows those use (packed 4:2:2: its one plane, 2 * w bytes a row; every row
                // carries its own chroma, so the rows the resize reads are all there is to copy)
                if (!rows) { if ((rc = caller_h2d_planes(ctx, d, f.data, *yuv, f.width, f.height, st))) return rc; }
                else for (int p = 0; p < yuv_planes_of(*yuv); p++) {
                    uint8_t *dp = d + yuv->offset[p];
                    const uint8_t *sp = (const uint8_t *)f.data + yuv->offset[p];
                    const size_t stride = (size_t)yuv->stride[p], rb = yuv_plane_row_bytes(*yuv, p, f.width), pr = yuv_plane_rows(p, f.height);
                    if (p == 0) rc = copy_row_runs(ctx, dp, sp, stride, rb, pr, (size_t)rows->first, (size_t)rows->period, (size_t)rows->run, (size_t)rows->count, st);
                    else rc = copy_chroma_runs(ctx, dp, sp, stride, rb, pr, *rows, st);
                    if (rc) return rc;
                }
                hp[i] = d;
                off += round_up(yuv_extent(*yuv, f.width, f.height), 256);
                continue;
            }
            if (rows) {
                // only the rows the resize reads
                if ((rc = copy_row_runs(ctx, d, (const uint8_t *)f.data, (size_t)f.stride, (size_t)f.width * bpp, (size_t)f.height,
                                        (size_t)rows->first, (size_t)rows->period, (size_t)rows->run, (size_t)rows->count, st))) return rc;
            } else if ((rc = caller_h2d(ctx, d, f.data, (size_t)f.stride * (f.height - 1) + (size_t)f.width * bpp, st))) return rc;
            hp[i] = d;
            off += round_up((size_t)f.stride * f.height, 256);
        } else
            hp[i] = f.data;
    }
    NVCA_HIP_CHECK(ctx, hipMemcpyAsync(ws.res[ws.cur_res].srcptrs.as<const void *>() + r0, hp, (size_t)n * sizeof(void *), hipMemcpyHostToDevice, st));
    if (off_io) *off_io = off;
    return NVCA_OK;
}

bool frames_aligned4(const nvca_frame *frames, const int *idx, int n)
{
    for (int i = 0; i < n; i++) {
        const nvca_frame &f = frames[idx ? idx[i] : i];
        if ((f.stride & 3) || (f.mem == NVCA_MEM_DEVICE && ((uintptr_t)f.data & 15))) return false;
    }
    return true;
}

// frames of one 4:2:0 / 4:2:2 layout: the layout (yuv_layout_aligned16, yuv_layout.h) and every device frame's base take the wide gray
// kernel's loads -- k_gray_yuv16 / k_gray_yuv422_16 (staged host frames start on 256 bytes)
bool frames_yuv_aligned16(const nvca_frame *frames, const int *idx, int n, const nvca_pixel_layout &l)
{
    if (!yuv_layout_aligned16(l)) return false;
    for (int i = 0; i < n; i++) {
        const nvca_frame &f = frames[idx ? idx[i] : i];
        if (f.mem == NVCA_MEM_DEVICE && ((uintptr_t)f.data & 15)) return false;
    }
    return true;
}

} // namespace nvca
