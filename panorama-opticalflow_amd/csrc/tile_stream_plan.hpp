// Piece sizes of the streamed tile smoothing (k_tile_blur<true>, kernels_misc.hip): how a tile's (step+k-1)^2 window and its
// (step+k-1) x step fp64 row sums go through a FIXED amount of LDS.  The window is staged in chunks of whole window rows (one
// lane walks one row, so its sliding sum never leaves its register); every row sum goes to a per-block scratch area in HBM,
// column-major, and comes back in strips of whole output columns (one lane walks one column).  Plain C++ so that the CPU test
// tier can check it (tests/cpp/tile_stream_plan_test.cpp).
#ifndef PF_TILE_STREAM_PLAN_HPP_
#define PF_TILE_STREAM_PLAN_HPP_
#include <stddef.h>

namespace pf {

constexpr size_t kTileStreamLdsBudget = 160 * 1024 - 256;   // the 160 KiB of a CU (one block per CU) less the kernels' static LDS
constexpr int kTileStreamMaxBlocks = 32;               // the grid-size cap of the tile smoothing launchers

struct TileStreamPlan {
  int nr = 0;           // window rows = window columns = step + k - 1
  int win_stride = 0;   // floats per staged window row: odd (the lanes of the row walk hit different banks) unless that costs a chunk
  int chunk_rows = 0;   // window rows per LDS piece; 0 = one window row alone exceeds the budget (no plan)
  int n_chunks = 0;
  int sum_stride = 0;   // doubles per output column, in scratch and in LDS (odd, >= nr)
  int strip_cols = 0;   // output columns per LDS piece; 0 = one column of row sums alone exceeds the budget (no plan)
  int n_strips = 0;
  size_t lds_bytes = 0;       // dynamic LDS of the launch: the larger of the two kinds of piece (they share the space)
  size_t scratch_bytes = 0;   // per block: step columns of sum_stride doubles, rounded up to 256 bytes
  bool ok() const { return chunk_rows > 0 && strip_cols > 0; }
};

inline TileStreamPlan tile_stream_plan(int step, int k, size_t lds_budget = kTileStreamLdsBudget) {
  TileStreamPlan p;
  if (step < 1 || k < 1) return p;
  const size_t nr = size_t(step) + k - 1;
  if (nr > (size_t(1) << 28)) return p;
  p.nr = int(nr);
  p.sum_stride = int(nr | 1);
  auto chunks = [&](size_t stride) { const size_t fit = lds_budget / (stride * sizeof(float)); return fit ? (nr + fit - 1) / fit : size_t(0); };
  if (chunks(nr) == 0) return p;
  // the window of a 400x26200 strip (202 x 202 floats) fits a CU's LDS in one piece only without the padding column: a row walk
  // with two-way bank conflicts is cheaper than a second piece
  p.win_stride = int(chunks(nr | 1) == chunks(nr) ? (nr | 1) : nr);
  const size_t row_bytes = size_t(p.win_stride) * sizeof(float), col_bytes = size_t(p.sum_stride) * sizeof(double);
  const size_t max_rows = lds_budget / row_bytes, max_cols = lds_budget / col_bytes;
  if (max_rows < 1 || max_cols < 1) return p;
  // equal pieces: 299 rows at 136 per piece are 3 x 100, not 136 + 136 + 27 (the row walk is one lane per row)
  p.n_chunks = int((nr + max_rows - 1) / max_rows);
  p.chunk_rows = int((nr + p.n_chunks - 1) / p.n_chunks);
  p.n_strips = int((size_t(step) + max_cols - 1) / max_cols);
  p.strip_cols = (step + p.n_strips - 1) / p.n_strips;
  const size_t a = size_t(p.chunk_rows) * row_bytes, b = size_t(p.strip_cols) * col_bytes;
  p.lds_bytes = a > b ? a : b;
  p.scratch_bytes = (size_t(step) * col_bytes + 255) & ~size_t(255);
  return p;
}

}  // namespace pf
#endif
