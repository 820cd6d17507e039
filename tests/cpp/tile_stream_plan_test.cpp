// CPU check of csrc/tile_stream_plan.hpp: for every tile size 1..400 and window 1..600 the pieces of the streamed tile smoothing
// fit 160 KiB of LDS, the row chunks cover every window row exactly once and the column strips every output column exactly once,
// walked the way the kernel walks them; the scratch area holds every row sum; small budgets end in "no plan", never in a wrong one.
#include <cstdio>
#include <vector>

#include "tile_stream_plan.hpp"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_plan(int step, int k, size_t budget) {
  const pf::TileStreamPlan p = pf::tile_stream_plan(step, k, budget);
  const int nr = step + k - 1;
  if (!p.ok()) {   // only when a single window row, or a single column of row sums, is larger than the budget
    CHECK(size_t(nr | 1) * 8 > budget, "step %d k %d budget %zu: no plan", step, k, budget);
    return;
  }
  CHECK(p.nr == nr && p.win_stride >= nr && p.sum_stride >= nr && (p.sum_stride & 1), "step %d k %d", step, k);
  CHECK(p.lds_bytes <= budget, "step %d k %d: %zu bytes of LDS", step, k, p.lds_bytes);
  CHECK(size_t(p.chunk_rows) * p.win_stride * sizeof(float) <= p.lds_bytes && size_t(p.strip_cols) * p.sum_stride * sizeof(double) <= p.lds_bytes,
        "step %d k %d: a piece exceeds lds_bytes", step, k);
  CHECK(p.scratch_bytes >= size_t(step) * p.sum_stride * sizeof(double) && p.scratch_bytes % 256 == 0, "step %d k %d: scratch", step, k);
  std::vector<int> row(nr, 0), col(step, 0);
  int chunks = 0, strips = 0;
  for (int j0 = 0; j0 < nr; j0 += p.chunk_rows, ++chunks) {
    const int n = nr - j0 < p.chunk_rows ? nr - j0 : p.chunk_rows;
    for (int j = 0; j < n; ++j) ++row[j0 + j];
  }
  for (int xs = 0; xs < step; xs += p.strip_cols, ++strips) {
    const int n = step - xs < p.strip_cols ? step - xs : p.strip_cols;
    for (int x = 0; x < n; ++x) ++col[xs + x];
  }
  CHECK(chunks == p.n_chunks && strips == p.n_strips, "step %d k %d: %d chunks (plan %d), %d strips (plan %d)", step, k, chunks, p.n_chunks, strips, p.n_strips);
  for (int j = 0; j < nr; ++j) CHECK(row[j] == 1, "step %d k %d: window row %d covered %d times", step, k, j, row[j]);
  for (int x = 0; x < step; ++x) CHECK(col[x] == 1, "step %d k %d: output column %d covered %d times", step, k, x, col[x]);
}

int main() {
  for (int step = 1; step <= 400; ++step)
    for (int k = 1; k <= 600; ++k) {
      check_plan(step, k, pf::kTileStreamLdsBudget);
      CHECK(pf::tile_stream_plan(step, k).ok() && pf::tile_stream_plan(step, k).lds_bytes <= 160 * 1024, "step %d k %d", step, k);
    }
  for (size_t budget : {size_t(64), size_t(1000), size_t(4096), size_t(40000)})
    for (int step = 1; step <= 120; step += 7)
      for (int k = 1; k <= 300; k += 11) check_plan(step, k, budget);
  CHECK(!pf::tile_stream_plan(0, 5).ok() && !pf::tile_stream_plan(5, 0).ok(), "degenerate");
  // the geometries the design names: a 400x26200 strip, a 30000x15000 panorama, row sums alone beyond LDS
  CHECK(pf::tile_stream_plan(2, 201).n_chunks == 1 && pf::tile_stream_plan(2, 201).win_stride == 202 && pf::tile_stream_plan(2, 201).n_strips == 1, "2/201");
  CHECK(pf::tile_stream_plan(75, 115).n_chunks == 1 && pf::tile_stream_plan(75, 115).win_stride == 189 && pf::tile_stream_plan(75, 115).n_strips == 1, "75/115");
  CHECK(pf::tile_stream_plan(5, 200).n_chunks == 2 && pf::tile_stream_plan(5, 200).win_stride == 205, "5/200");
  CHECK(pf::tile_stream_plan(120, 180).n_chunks == 3 && pf::tile_stream_plan(120, 180).chunk_rows == 100 && pf::tile_stream_plan(120, 180).n_strips == 2 &&
            pf::tile_stream_plan(120, 180).strip_cols == 60, "120/180");
  if (fails) { printf("%d failures\n", fails); return 1; }
  printf("ok\n");
  return 0;
}
