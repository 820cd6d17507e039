// Part of pf_api.hip (one translation unit): the resize entry points.  The host makes the two axes' tables (resize_table.hpp), keeps
// the last few in the context and uploads them; the passes run in kernels_resize.hip, horizontal first, through an intermediate plane
// of out_cols x rows.  An axis whose size stays runs no pass; a size that stays altogether is a copy.  The scratch ("rz_*") is the
// resize's own: no entry point here touches the chain, the prefetch records, the batch slots, the plans or what pf_stitch_visualize reads.
}  // extern "C"
namespace {

constexpr size_t kRzTablesKept = 8;   // host tables a context keeps (a run resizes to one or two sizes)

const resize_table::Table* resize_table_of(pf_ctx* c, int in, int out, int filter) {
  for (const auto& t : c->rz_tables) if (t.in == in && t.out == out && t.filter == filter) return &t;
  if (c->rz_tables.size() >= kRzTablesKept) c->rz_tables.erase(c->rz_tables.begin());
  c->rz_tables.emplace_back();
  resize_table::make(in, out, filter, &c->rz_tables.back());
  return &c->rz_tables.back();
}

// the table of one axis resident in the arena: bounds, then the coefficients at the next 256-byte boundary
int resize_table_dev(pf_ctx* c, int axis, int in, int out, int filter, const int** d_bounds, const int** d_k) {
  const resize_table::Table* t = resize_table_of(c, in, out, filter);
  const size_t nb = t->bounds.size() * 4, nk = t->k.size() * 4, at_k = (nb + 255) & ~size_t(255);
  const uint8_t* d;
  auto fill = [&](uint8_t* h) { memcpy(h, t->bounds.data(), nb); memcpy(h + at_k, t->k.data(), nk); };
  if (int e = resident_table(c, axis ? "rz_tab_v" : "rz_tab_h", c->rz_dev[axis], in, out, filter, at_k + nk, fill, &d)) return e;
  *d_bounds = (const int*)d; *d_k = (const int*)(d + at_k);
  return 0;
}

// sizes, the filter and the tables' bound: everything known without a pointer
int resize_check(pf_ctx* c, int cols, int rows, int out_cols, int out_rows, int filter) {
  if (int e = check_image(c, cols, rows)) return e;
  if (out_cols <= 0 || out_rows <= 0) return fail(c, PF_ERR_ARG, "resize: bad output size %dx%d", out_cols, out_rows);
  if ((double)out_cols * out_rows > 2.0e9 || (double)out_cols * rows > 2.0e9) return fail(c, PF_ERR_ARG, "resize: output %dx%d too large", out_cols, out_rows);
  if (!resize_table::known(filter)) return fail(c, PF_ERR_ARG, "resize: unknown filter %d (1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING)", filter);
  if (out_cols != cols && !resize_table::fits(cols, out_cols, filter)) return fail(c, PF_ERR_ARG, "resize: the table of %d -> %d columns exceeds %.0f coefficients", cols, out_cols, resize_table::kMaxCoefs);
  if (out_rows != rows && !resize_table::fits(rows, out_rows, filter)) return fail(c, PF_ERR_ARG, "resize: the table of %d -> %d rows exceeds %.0f coefficients", rows, out_rows, resize_table::kMaxCoefs);
  return 0;
}

// n device images of cols x rows -> n of out_cols x out_rows, enqueued on s_main in groups of kMaxBatch; the caller drains
int resize_many(pf_ctx* c, int n, const uint8_t* const* d_src, int cols, int rows, uint8_t* const* d_dst, int out_cols, int out_rows, int filter) {
  const size_t in_bytes = size_t(cols) * rows * 4, out_bytes = size_t(out_cols) * out_rows * 4;
  if (int e = check_dev_images(c, "resize", n, d_src, in_bytes, d_dst, out_bytes)) return e;
  hipStream_t sm = c->s_main;
  const bool do_h = out_cols != cols, do_v = out_rows != rows;
  if (!do_h && !do_v) {
    for (int k = 0; k < n; ++k) HIPCHK(c, hipMemcpyAsync(d_dst[k], d_src[k], in_bytes, hipMemcpyDeviceToDevice, sm));
    return 0;
  }
  const int *bh = nullptr, *kh = nullptr, *bv = nullptr, *kv = nullptr;
  if (do_h) if (int e = resize_table_dev(c, 0, cols, out_cols, filter, &bh, &kh)) return e;
  if (do_v) if (int e = resize_table_dev(c, 1, rows, out_rows, filter, &bv, &kv)) return e;
  const size_t mid_bytes = (size_t(out_cols) * rows * 4 + 255) & ~size_t(255);
  uint8_t* d_mid = nullptr;
  if (do_h && do_v) { d_mid = (uint8_t*)ensure(c, "rz_mid", mid_bytes * std::min(n, kMaxBatch)); if (!d_mid) return PF_ERR_NOMEM; }
  for (int first = 0; first < n; first += kMaxBatch) {
    const int count = std::min(kMaxBatch, n - first);
    ResizePtrs h, v;
    memset(&h, 0, sizeof h); memset(&v, 0, sizeof v);
    for (int k = 0; k < count; ++k) {
      uint32_t* mid = (uint32_t*)(d_mid + k * mid_bytes);
      h.src[k] = (const uint32_t*)d_src[first + k]; h.dst[k] = do_v ? mid : (uint32_t*)d_dst[first + k];
      v.src[k] = do_h ? mid : (const uint32_t*)d_src[first + k]; v.dst[k] = (uint32_t*)d_dst[first + k];
    }
    if (do_h) { PROF(c, sm, "resize_h"); launch_resize_h(sm, count, h, cols, rows, out_cols, bh, kh, true, !do_v); }
    if (do_v) { PROF(c, sm, "resize_v"); launch_resize_v(sm, count, v, out_cols, rows, out_rows, bv, kv, !do_h, true); }
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

}  // namespace
extern "C" {

int pf_resize_dev(pf_ctx* c, const uint8_t* d_src_bgra, int cols, int rows, uint8_t* d_dst_bgra, int out_cols, int out_rows, int filter) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_src_bgra || !d_dst_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = resize_check(c, cols, rows, out_cols, out_rows, filter)) return e;
  if (int e = resize_many(c, 1, &d_src_bgra, cols, rows, &d_dst_bgra, out_cols, out_rows, filter)) return e;
  return finish(c);
}

int pf_resize(pf_ctx* c, const uint8_t* src_bgra, size_t src_step, int cols, int rows, uint8_t* dst_bgra, size_t dst_step, int out_cols, int out_rows, int filter) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!src_bgra || !dst_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = resize_check(c, cols, rows, out_cols, out_rows, filter)) return e;
  if (src_step < size_t(cols) * 4 || dst_step < size_t(out_cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  if (ranges_overlap(dst_bgra, bgra_span(out_cols, out_rows, dst_step), src_bgra, bgra_span(cols, rows, src_step))) return fail(c, PF_ERR_ARG, "resize: the destination overlaps the source");
  const uint8_t* d_src;
  if (int e = upload_bgra(c, "rz_src", src_bgra, src_step, cols, rows, &d_src)) return e;
  uint8_t* d_dst = (uint8_t*)ensure(c, "rz_dst", size_t(out_cols) * out_rows * 4);
  if (!d_dst) return PF_ERR_NOMEM;
  if (int e = resize_many(c, 1, &d_src, cols, rows, &d_dst, out_cols, out_rows, filter)) return e;
  if (int e = down_plane(c, dst_bgra, dst_step, d_dst, out_cols, out_rows, 4)) return e;
  return finish(c);
}

// stage entry: ONE pass of the resize on host images, its two fusions as the caller says.  axis 0: k_resize_h, cols -> n_out columns;
// axis 1: k_resize_v, rows -> n_out rows.  The table is the library's own for that axis; an n_out that equals the axis still runs the pass.
int pf_stage_resize_pass(pf_ctx* c, const uint8_t* src_bgra, int cols, int rows, int axis, int n_out, int filter, int premul, int unpremul, uint8_t* dst_bgra) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!src_bgra || !dst_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  if (axis != 0 && axis != 1) return fail(c, PF_ERR_ARG, "resize pass: bad axis %d (0 horizontal, 1 vertical)", axis);
  const int out_cols = axis ? cols : n_out, out_rows = axis ? n_out : rows;
  if (int e = resize_check(c, cols, rows, out_cols, out_rows, filter)) return e;
  const int in = axis ? rows : cols;
  if (!resize_table::fits(in, n_out, filter)) return fail(c, PF_ERR_ARG, "resize: the table of %d -> %d %s exceeds %.0f coefficients", in, n_out, axis ? "rows" : "columns", resize_table::kMaxCoefs);
  const size_t in_step = size_t(cols) * 4, out_step = size_t(out_cols) * 4;   // both host images are packed
  if (ranges_overlap(dst_bgra, bgra_span(out_cols, out_rows, out_step), src_bgra, bgra_span(cols, rows, in_step))) return fail(c, PF_ERR_ARG, "resize: the destination overlaps the source");
  const uint8_t* d_src;
  if (int e = upload_bgra(c, "rz_src", src_bgra, in_step, cols, rows, &d_src)) return e;
  uint8_t* d_dst = (uint8_t*)ensure(c, "rz_dst", out_step * out_rows);
  if (!d_dst) return PF_ERR_NOMEM;
  const int *bounds = nullptr, *k = nullptr;
  if (int e = resize_table_dev(c, axis, in, n_out, filter, &bounds, &k)) return e;
  ResizePtrs io;
  memset(&io, 0, sizeof io);
  io.src[0] = (const uint32_t*)d_src; io.dst[0] = (uint32_t*)d_dst;
  if (axis) { PROF(c, c->s_main, "resize_v"); launch_resize_v(c->s_main, 1, io, cols, rows, n_out, bounds, k, premul != 0, unpremul != 0); }
  else { PROF(c, c->s_main, "resize_h"); launch_resize_h(c->s_main, 1, io, cols, rows, n_out, bounds, k, premul != 0, unpremul != 0); }
  HIPCHK(c, hipGetLastError());
  if (int e = down_plane(c, dst_bgra, out_step, d_dst, out_cols, out_rows, 4)) return e;
  return finish(c);
}

int pf_resize_batch_dev(pf_ctx* c, int n,const uint8_t* const* d_src_bgra, int cols, int rows, uint8_t* const* d_dst_bgra, int out_cols, int out_rows, int filter) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (n < 0 || !d_src_bgra || !d_dst_bgra) return fail(c, PF_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  if (int e = resize_check(c, cols, rows, out_cols, out_rows, filter)) return e;
  if (int e = resize_many(c, n, d_src_bgra, cols, rows, d_dst_bgra, out_cols, out_rows, filter)) return e;
  return finish(c);
}

// The composite the last pf_stitch_step / pf_stitch_step_planned left in HBM, read in place
int pf_stitch_result_resized_dev(pf_ctx* c, int out_cols, int out_rows, int filter, uint8_t* d_dst_bgra) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_dst_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  DevImage r;
  if (int e = resident_result(c, "pf_stitch_result_resized_dev", nullptr, &r)) return e;
  if (int e = resize_check(c, r.cols, r.rows, out_cols, out_rows, filter)) return e;
  if (int e = resize_many(c, 1, &r.p, r.cols, r.rows, &d_dst_bgra, out_cols, out_rows, filter)) return e;
  return finish(c);
}

// ... and frame slot `frame` of the last host-form pf_stitch_step_batch* call
int pf_stitch_batch_result_resized_dev(pf_ctx* c, int frame, int out_cols, int out_rows, int filter, uint8_t* d_dst_bgra) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_dst_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  DevImage r;
  if (int e = resident_result(c, "pf_stitch_batch_result_resized_dev", &frame, &r)) return e;
  if (int e = resize_check(c, r.cols, r.rows, out_cols, out_rows, filter)) return e;
  if (int e = resize_many(c, 1, &r.p, r.cols, r.rows, &d_dst_bgra, out_cols, out_rows, filter)) return e;
  return finish(c);
}
