// Part of pf_api.hip (one translation unit): the PNG encoder's entry points.  Filtering, deflate and compaction run in kernels_png.hip;
// only the finished deflate stream crosses the link, straight into its place in the caller's buffer, and the host frames it
// (png_frame.hpp: signature, IHDR, zlib header, IDAT lengths and CRCs, the Adler-32 combined from the segments' sums, IEND).
// The scratch ("png_*") is the encoder's own: no entry point here touches the chain, the prefetch records, the batch slots or what
// pf_stitch_visualize reads.

// n <= kMaxBatch same-size device images -> n files.  Every image's kernels are enqueued before the one drain; then per image the
// stream's length and the segments' Adler sums come down, then the stream itself.
static int png_encode_group(pf_ctx* c, int n, const uint8_t* const* d_bgra, int cols, int rows, uint8_t* const* png_out, size_t cap, size_t* sizes_out) {
  const size_t stream = png_frame::stream_bytes(cols, rows), nseg = png_frame::segments(stream);
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t st_stream = al(png_stream_alloc_bytes(cols, rows)), st_slots = al(nseg * png_frame::kSegSlot), st_packed = al(png_frame::deflate_bound(stream));
  const size_t st_words = al(nseg * 4), st_offs = al((nseg + 1) * 8);
  uint8_t* d_stream = (uint8_t*)ensure(c, "png_stream", st_stream * n); uint8_t* d_slots = (uint8_t*)ensure(c, "png_slots", st_slots * n);
  uint8_t* d_packed = (uint8_t*)ensure(c, "png_packed", st_packed * n);
  uint8_t* d_sizes = (uint8_t*)ensure(c, "png_sizes", st_words * n); uint8_t* d_adler = (uint8_t*)ensure(c, "png_adler", st_words * n);
  uint8_t* d_offs = (uint8_t*)ensure(c, "png_offs", st_offs * n);
  if (!d_stream || !d_slots || !d_packed || !d_sizes || !d_adler || !d_offs) return PF_ERR_NOMEM;
  hipStream_t sm = c->s_main;
  for (int k = 0; k < n; ++k) {
    PngWork w;
    w.stream = d_stream + k * st_stream; w.slots = d_slots + k * st_slots; w.packed = d_packed + k * st_packed;
    w.sizes = (unsigned*)(d_sizes + k * st_words); w.adler = (unsigned*)(d_adler + k * st_words); w.offs = (unsigned long long*)(d_offs + k * st_offs);
    { PROF(c, sm, "png_filter"); launch_png_filter(sm, d_bgra[k], cols, rows, w); }
    { PROF(c, sm, "png_deflate"); launch_png_deflate(sm, cols, rows, w); }
    { PROF(c, sm, "png_pack"); launch_png_pack(sm, cols, rows, w); }
  }
  std::vector<unsigned long long> dlen(n);
  std::vector<unsigned> adl(nseg * n);
  for (int k = 0; k < n; ++k) {
    HIPCHK(c, hipMemcpyAsync(&dlen[k], d_offs + k * st_offs + nseg * 8, 8, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipMemcpyAsync(&adl[k * nseg], d_adler + k * st_words, nseg * 4, hipMemcpyDeviceToHost, sm));
  }
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  int short_k = -1;
  for (int k = 0; k < n; ++k) {
    if (dlen[k] > png_frame::deflate_bound(stream)) return fail(c, PF_ERR_DEVICE, "png: deflate stream of image %d exceeds its bound", k);
    sizes_out[k] = png_frame::Frame(cols, rows, (size_t)dlen[k]).file_size();
    if (sizes_out[k] > cap && short_k < 0) short_k = k;
  }
  if (short_k >= 0) return fail(c, PF_ERR_ARG, "png: the file of image %d needs %zu bytes, the buffer holds %zu", short_k, sizes_out[short_k], cap);
  c->drained = false;
  for (int k = 0; k < n; ++k) {
    const png_frame::Frame fr(cols, rows, (size_t)dlen[k]);
    fr.write_head(png_out[k]);
    for (size_t d = 0; d < fr.deflate_len;) {
      size_t run;
      const size_t at = fr.deflate_run(d, fr.deflate_len - d, &run);
      HIPCHK(c, hipMemcpyAsync(png_out[k] + at, d_packed + k * st_packed + d, run, hipMemcpyDeviceToHost, sm));
      d += run;
    }
  }
  if (int e = finish(c)) return e;
  for (int k = 0; k < n; ++k) {
    // the segments' Adler sums in stream order; every segment but the last is kSegBytes long
    uint32_t ad = 1;
    for (size_t s = 0; s < nseg; ++s) ad = png_frame::adler32_combine(ad, adl[k * nseg + s], s + 1 < nseg ? png_frame::kSegBytes : stream - s * png_frame::kSegBytes);
    png_frame::Frame(cols, rows, (size_t)dlen[k]).write_tail(png_out[k], ad);
  }
  return 0;
}

static int png_encode_many(pf_ctx* c, int n, const uint8_t* const* d_bgra, int cols, int rows, uint8_t* const* png_out, size_t cap, size_t* sizes_out) {
  for (int k = 0; k < n; ++k) if (!png_out[k]) return fail(c, PF_ERR_ARG, "null pointer (image %d)", k);
  if (int e = check_dev_images(c, "png", n, d_bgra, size_t(cols) * rows * 4)) return e;
  for (int first = 0; first < n; first += kMaxBatch) {
    const int count = std::min(kMaxBatch, n - first);
    if (int e = png_encode_group(c, count, d_bgra + first, cols, rows, png_out + first, cap, sizes_out + first)) return e;
  }
  return 0;
}

size_t pf_png_bound(int cols, int rows) { return (cols > 0 && rows > 0) ? png_frame::bound(cols, rows) : 0; }
size_t pf_png_segment_bytes(void) { return png_frame::kSegBytes; }

int pf_png_encode_dev(pf_ctx* c, const uint8_t* d_bgra, int cols, int rows, uint8_t* png_out, size_t cap, size_t* size_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_bgra || !png_out || !size_out) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  return png_encode_many(c, 1, &d_bgra, cols, rows, &png_out, cap, size_out);
}

int pf_png_encode(pf_ctx* c, const uint8_t* bgra, size_t step_bytes, int cols, int rows, uint8_t* png_out, size_t cap, size_t* size_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!bgra || !png_out || !size_out) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (step_bytes < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const uint8_t* d;
  if (int e = upload_bgra(c, "png_src", bgra, step_bytes, cols, rows, &d)) return e;
  return png_encode_many(c, 1, &d, cols, rows, &png_out, cap, size_out);
}

int pf_png_encode_batch_dev(pf_ctx* c, int n, const uint8_t* const* d_bgra, int cols, int rows, uint8_t* const* png_out, size_t cap_each, size_t* sizes_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (n < 0 || !d_bgra || !png_out || !sizes_out) return fail(c, PF_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  if (int e = check_image(c, cols, rows)) return e;
  return png_encode_many(c, n, d_bgra, cols, rows, png_out, cap_each, sizes_out);
}

// The composite the last pf_stitch_step / pf_stitch_step_planned left in HBM (what r == NULL chains on), read in place
int pf_stitch_result_png(pf_ctx* c, uint8_t* png_out, size_t cap, size_t* size_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!png_out || !size_out) return fail(c, PF_ERR_ARG, "null pointer");
  DevImage r;
  if (int e = resident_result(c, "pf_stitch_result_png", nullptr, &r)) return e;
  return png_encode_many(c, 1, &r.p, r.cols, r.rows, &png_out, cap, size_out);
}

// ... and frame slot `frame` of the last host-form pf_stitch_step_batch* call
int pf_stitch_batch_result_png(pf_ctx* c, int frame, uint8_t* png_out, size_t cap, size_t* size_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!png_out || !size_out) return fail(c, PF_ERR_ARG, "null pointer");
  DevImage r;
  if (int e = resident_result(c, "pf_stitch_batch_result_png", &frame, &r)) return e;
  return png_encode_many(c, 1, &r.p, r.cols, r.rows, &png_out, cap, size_out);
}
