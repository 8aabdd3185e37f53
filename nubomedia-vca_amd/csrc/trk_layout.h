// trk_layout.h -- the one statement of NuboTracker's work buffers: what tracker.cpp allocates and what the kernels of
// kernels_trk_pixel.hip / kernels_trk_ccl.hip index.  Host + device (NVCA_HD); no HIP header: a plain C++ compiler reads this file
// (tests/san/trk_host_driver.cpp prints every offset and size below, tests/test_trk_host_cpu.py checks them).
#pragma once
#include "device_records.h"     // NVCA_HD

namespace nvca {

// ---- geometry.  A SEGMENT is 256 pixels of a row: a wave's share of the pixel pass, a block's row in the component kernels.  A TILE
// is one segment wide and kCclTileRows rows high: what a block of k_ccl_tile labels out of LDS, with kCclTileWaves waves.
static constexpr int kTrkSegW = 256;
static constexpr int kCclTileRows = 8;
static constexpr int kCclTileWaves = 4;
static_assert(kCclTileWaves * 64 == kTrkSegW, "a tile block has a thread per pixel of a segment");
// A block of the per-pixel component kernels walks kCclRows rows of its 256-pixel column: most segments of a frame hold no motion and
// are skipped on their flag byte, and a grid of one block per segment (69 k blocks for 8 x 1080p) cost 30 us per kernel in
// block dispatch alone -- five kernels a tick.
static constexpr int kCclRowsDefault = 8;
// the two union-find kernels walk fewer: a thread's unions / finds are chains of dependent global round trips, one row after the
// other (measured on 8 x 1080p: 1 / 2 / 4 / 8 rows -> trackers alone 0.261 / 0.250 / 0.259 / 0.274 ms per tick)
static constexpr int kCclRowsUf = 2;
static constexpr int kCclRowsMax = 16;        // rows whose flag bytes live_rows asks for at once (a bit per row): the limit of NVCA_CCL_ROWS / _UF
static_assert(kCclRowsDefault <= kCclRowsMax && kCclRowsUf <= kCclRowsMax && kCclTileRows <= kCclRowsMax, "live_rows holds kCclRowsMax rows");

NVCA_HD inline int seg_per_row(int w) { return (w + kTrkSegW - 1) / kTrkSegW; }
NVCA_HD inline int tile_rows(int h) { return (h + kCclTileRows - 1) / kCclTileRows; }
NVCA_HD inline int tiles_per_slot(int w, int h) { return seg_per_row(w) * tile_rows(h); }
NVCA_HD inline int tile_of(int w, int y, int seg) { return (y / kCclTileRows) * seg_per_row(w) + seg; }     // a slot's tiles, row-major

// ---- flag bytes (TrkWorkspace::flags): [batch][h][seg_per_row] one byte per segment -- does it hold any motion history? -- then, on
// the next multiple of 64 bytes, one int per slot: the live segments of every kTrkCountEvery-th row (an estimate of how much of the
// frame moves: it steers k_ccl_reduce's visiting order and nothing else)
static constexpr int kTrkCountEvery = 16;
NVCA_HD inline size_t trk_flag_index(int w, int h, int slot, int y, int seg) { return ((size_t)slot * h + y) * seg_per_row(w) + seg; }
NVCA_HD inline size_t trk_count_offset(int w, int h, int batch) { return ((size_t)seg_per_row(w) * h * batch + 63) & ~(size_t)63; }
NVCA_HD inline size_t trk_flag_bytes(int w, int h, int batch) { return trk_count_offset(w, h, batch) + sizeof(int) * (size_t)batch; }
NVCA_HD inline int *segment_counts(const uint8_t *flags, int w, int h, int batch) { return (int *)(flags + trk_count_offset(w, h, batch)); }
NVCA_HD inline bool trk_counted_row(int y) { return (y & (kTrkCountEvery - 1)) == 0; }
NVCA_HD inline int trk_counted_rows(int h) { return (h + kTrkCountEvery - 1) / kTrkCountEvery; }

// ---- tile list (TrkWorkspace::tiles, ints).  The tiles that hold motion history are LISTED, per slot, by the first of their segments
// that finds some: [mark per tile: batch x per_slot][list, a slot's tiles: batch x per_slot][count per slot, set 0][count per slot, set 1].
// A mark equal to this launch's tick means "listed already" (marks are never cleared: the tick moves on); the counts of tick t live in
// set t & 1, and the pixel pass of tick t clears set (t + 1) & 1, which nobody reads or writes during tick t.  The component kernels
// then walk the live tiles only, evenly spread over their blocks (k_ccl_tile was bound by the blocks that drew three live tiles out
// of eight).
NVCA_HD inline size_t trk_tiles_list_offset(int w, int h, int batch) { return (size_t)tiles_per_slot(w, h) * batch; }
NVCA_HD inline size_t trk_tiles_count_offset(int w, int h, int batch, int set) { return 2 * (size_t)tiles_per_slot(w, h) * batch + (size_t)(set * batch); }      // set: 0 / 1
NVCA_HD inline size_t trk_tiles_words(int w, int h, int batch) { return (2 * (size_t)tiles_per_slot(w, h) + 2) * (size_t)batch; }
struct TileList { int *mark, *list, *cnt_now, *cnt_next; int per_slot; };      // mark / list of slot z's entry e: [z * per_slot + e]
NVCA_HD inline TileList tile_list(int *tiles, int w, int h, int batch, int tick)
{
    TileList t;
    t.per_slot = tiles_per_slot(w, h);
    t.mark = tiles; t.list = tiles + trk_tiles_list_offset(w, h, batch);
    int *cnt = tiles + trk_tiles_count_offset(w, h, batch, 0);
    t.cnt_now = cnt + (tick & 1) * batch; t.cnt_next = cnt + ((tick + 1) & 1) * batch;
    return t;
}

// ---- root list (TrkWorkspace::roots, ints): a header, then one entry (slot * w * h + pixel) per tile root of the folded path
static constexpr int kRootsEntries = 0;       // tile roots listed (counts on past the capacity: the entries beyond it are not stored)
static constexpr int kRootsOverflowed = 1;    // set by the tile that found the list full
static constexpr int kRootsError = 2;         // the label walks' "must never happen" record, kRootsErrorWords words: times, where, which kernel
static constexpr int kRootsErrorWords = 3;
static constexpr int kRootsHdr = 8;           // words in front of the first entry (cleared by the pixel pass, a thread a word)
static_assert(kRootsError + kRootsErrorWords <= kRootsHdr, "the error record lies inside the header");
// the list holds one entry per `div` pixels of the launch set (NVCA_TRK_ROOTS_DIV; 8): a frame of single-pixel components has more, and
// goes through the per-pixel kernels instead
inline int trk_roots_cap(int w, int h, int batch, int div)
{
    const size_t want = (size_t)w * h * batch / div, most = (size_t)1 << 30;
    return (int)(want < most ? want : most);
}
inline size_t trk_roots_words(int roots_cap) { return kRootsHdr + (size_t)roots_cap + 64; }

// ---- component list (TrkWorkspace::out / h_out, ints): [count][flags], then kCompWords words per component: slot, first seed
// (pixel index), x, y, w, h.  The count runs on past kCompCap (the components beyond it are not stored: the host refuses the frame).
static constexpr int kCompCount = 0, kCompFlags = 1, kCompHdr = 2;
static constexpr int kCompRootsOverflowed = 1;      // flag bit: the root list overflowed -- the host re-runs the launch set on the per-pixel kernels
static constexpr int kCompLabelError = 2;           // flag bit: a label walk met a word it must never meet -- the host reports an internal error
static constexpr int kCompWords = 6;
static constexpr int kCompCap = 1 << 18;
static constexpr int kCompFirstRead = 1024;         // components the host reads back with the header; the rest only when there are more
NVCA_HD inline size_t trk_comp_words(size_t comps) { return kCompHdr + kCompWords * comps; }      // = the offset of component `comps`
static_assert(kCompFirstRead <= kCompCap, "the first read-back lies inside the list");

} // namespace nvca
