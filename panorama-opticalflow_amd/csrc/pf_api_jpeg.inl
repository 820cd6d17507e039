// Part of pf_api.hip (one translation unit): the JPEG encoder's entry points.  The colour transform, DCT, quantisation and the entropy
// coder run in kernels_jpeg.hip; only the finished entropy-coded segment crosses the link, straight into its place in the caller's
// buffer behind the header the host writes (jpeg_frame.hpp: SOI .. SOS, the GPano XMP segment on request, EOI).
// The scratch ("jpg_*") is the encoder's own: no entry point here touches the chain, the prefetch records, the batch slots or what
// pf_stitch_visualize reads.

static int jpeg_restart_of(int subsampling) {
  int r = jpeg_frame::restart_interval(subsampling);
#ifdef PF_EXPERIMENTS
  // lab build only: tests/micro/jpeg_device_ab.py measures the product's interval against half and double
  if (const char* e = getenv("PANOFLOW_JPEG_RESTART")) { const int v = atoi(e); if (jpeg_restart_fits(subsampling, v)) r = v; }
#endif
  return r;
}

static int jpeg_check(pf_ctx* c, int cols, int rows, const pf_jpeg_params* p, pf_jpeg_params* out) {
  pf_jpeg_params_init(out);
  if (p) {
    if (p->struct_size != (int)sizeof(pf_jpeg_params)) return fail(c, PF_ERR_ARG, "jpeg: struct_size does not match this library's pf_jpeg_params");
    *out = *p;
  }
  if (out->quality < 1 || out->quality > 100) return fail(c, PF_ERR_ARG, "jpeg: quality %d is outside 1..100", out->quality);
  if (out->subsampling != 0 && out->subsampling != 1) return fail(c, PF_ERR_ARG, "jpeg: subsampling %d (0 is 4:4:4, 1 is 4:2:0)", out->subsampling);
  if (out->gpano != 0 && out->gpano != 1) return fail(c, PF_ERR_ARG, "jpeg: gpano %d (0 or 1)", out->gpano);
  if (cols > jpeg_frame::kMaxSide || rows > jpeg_frame::kMaxSide) return fail(c, PF_ERR_ARG, "jpeg: %dx%d, the format holds at most %d a side", cols, rows, jpeg_frame::kMaxSide);
  if (out->gpano && cols != 2 * rows) return fail(c, PF_ERR_ARG, "jpeg: gpano declares a full equirectangular sphere, which %dx%d (not 2:1) is not", cols, rows);
  return 0;
}

// n <= kMaxBatch same-size device images -> n files.  Every image's block, size and scan kernels are enqueued before the first drain,
// which brings the segments' lengths down; then the write passes go to buffers of exactly those lengths, and the segments come down.
static int jpeg_encode_group(pf_ctx* c, int n, const uint8_t* const* d_bgra, int cols, int rows, const pf_jpeg_params& p, uint8_t* const* jpg_out, size_t cap, size_t* sizes_out) {
  const int sub = p.subsampling, restart = jpeg_restart_of(sub);
  const size_t nint = jpeg_frame::intervals(cols, rows, sub, restart);
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t st_coef = al(jpeg_frame::coef_bytes(cols, rows, sub)), st_sizes = al(nint * 4), st_offs = al((nint + 1) * 8);
  uint8_t* d_coef = (uint8_t*)ensure(c, "jpg_coef", st_coef * n); uint8_t* d_sizes = (uint8_t*)ensure(c, "jpg_sizes", st_sizes * n);
  uint8_t* d_offs = (uint8_t*)ensure(c, "jpg_offs", st_offs * n); void* d_tab = ensure(c, "jpg_tables", sizeof(jpeg_frame::Tables));
  if (!d_coef || !d_sizes || !d_offs || !d_tab) return PF_ERR_NOMEM;
  hipStream_t sm = c->s_main;
  jpeg_frame::Tables tab;
  jpeg_frame::make_tables(p.quality, &tab);
  HIPCHK(c, hipMemcpyAsync(d_tab, &tab, sizeof tab, hipMemcpyHostToDevice, sm));
  HIPCHK(c, hipStreamSynchronize(sm));   // `tab` is this frame's
  std::vector<JpegWork> w(n);
  for (int k = 0; k < n; ++k) {
    w[k].coef = (int16_t*)(d_coef + k * st_coef); w[k].tables = d_tab;
    w[k].sizes = (unsigned*)(d_sizes + k * st_sizes); w[k].offs = (unsigned long long*)(d_offs + k * st_offs);
    { PROF(c, sm, "jpeg_blocks"); launch_jpeg_blocks(sm, d_bgra[k], cols, rows, sub, w[k]); }
    { PROF(c, sm, "jpeg_sizes"); launch_jpeg_sizes(sm, cols, rows, sub, restart, w[k]); }
  }
  std::vector<unsigned long long> slen(n);
  for (int k = 0; k < n; ++k) HIPCHK(c, hipMemcpyAsync(&slen[k], d_offs + k * st_offs + nint * 8, 8, hipMemcpyDeviceToHost, sm));
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  uint8_t head[jpeg_frame::kHeadMax];
  const size_t nhead = jpeg_frame::write_head(cols, rows, p.quality, sub, restart, p.gpano, head);
  int short_k = -1;
  size_t total = 0;
  std::vector<size_t> at(n);
  for (int k = 0; k < n; ++k) {
    if (restart == jpeg_frame::restart_interval(sub) && slen[k] > jpeg_frame::scan_bound(cols, rows, sub)) return fail(c, PF_ERR_DEVICE, "jpeg: the segment of image %d exceeds its bound", k);
    sizes_out[k] = nhead + (size_t)slen[k] + 2;
    if (sizes_out[k] > cap && short_k < 0) short_k = k;
    at[k] = total; total += al((size_t)slen[k]);
  }
  if (short_k >= 0) return fail(c, PF_ERR_ARG, "jpeg: the file of image %d needs %zu bytes, the buffer holds %zu", short_k, sizes_out[short_k], cap);
  uint8_t* d_packed = (uint8_t*)ensure(c, "jpg_packed", total);
  if (!d_packed) return PF_ERR_NOMEM;
  c->drained = false;
  for (int k = 0; k < n; ++k) {
    { PROF(c, sm, "jpeg_write"); launch_jpeg_write(sm, cols, rows, sub, restart, w[k], d_packed + at[k]); }
    memcpy(jpg_out[k], head, nhead);
    HIPCHK(c, hipMemcpyAsync(jpg_out[k] + nhead, d_packed + at[k], (size_t)slen[k], hipMemcpyDeviceToHost, sm));
    jpeg_frame::write_eoi(jpg_out[k] + nhead + (size_t)slen[k]);
  }
  HIPCHK(c, hipGetLastError());
  return finish(c);
}

static int jpeg_encode_many(pf_ctx* c, int n, const uint8_t* const* d_bgra, int cols, int rows, const pf_jpeg_params& p, uint8_t* const* jpg_out, size_t cap, size_t* sizes_out) {
  for (int k = 0; k < n; ++k) if (!jpg_out[k]) return fail(c, PF_ERR_ARG, "null pointer (image %d)", k);
  if (int e = check_dev_images(c, "jpeg", n, d_bgra, size_t(cols) * rows * 4)) return e;
  for (int first = 0; first < n; first += kMaxBatch) {
    const int count = std::min(kMaxBatch, n - first);
    if (int e = jpeg_encode_group(c, count, d_bgra + first, cols, rows, p, jpg_out + first, cap, sizes_out + first)) return e;
  }
  return 0;
}

void pf_jpeg_params_init(pf_jpeg_params* p) {
  if (!p) return;
  p->struct_size = (int)sizeof *p; p->quality = 90; p->subsampling = 1; p->gpano = 0;
}

size_t pf_jpeg_bound(int cols, int rows, const pf_jpeg_params* p) {
  const int sub = p ? p->subsampling : 1;
  if (cols <= 0 || rows <= 0 || cols > jpeg_frame::kMaxSide || rows > jpeg_frame::kMaxSide || (sub != 0 && sub != 1)) return 0;
  return jpeg_frame::bound(cols, rows, sub);
}

int pf_jpeg_restart_interval(int subsampling) { return jpeg_frame::restart_interval(subsampling); }

int pf_jpeg_encode_dev(pf_ctx* c, const uint8_t* d_bgra, int cols, int rows, const pf_jpeg_params* params, uint8_t* jpg_out, size_t cap, size_t* size_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_bgra || !jpg_out || !size_out) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  pf_jpeg_params p;
  if (int e = jpeg_check(c, cols, rows, params, &p)) return e;
  return jpeg_encode_many(c, 1, &d_bgra, cols, rows, p, &jpg_out, cap, size_out);
}

int pf_jpeg_encode(pf_ctx* c, const uint8_t* bgra, size_t step_bytes, int cols, int rows, const pf_jpeg_params* params, uint8_t* jpg_out, size_t cap, size_t* size_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!bgra || !jpg_out || !size_out) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  pf_jpeg_params p;
  if (int e = jpeg_check(c, cols, rows, params, &p)) return e;
  if (step_bytes < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const uint8_t* d;
  if (int e = upload_bgra(c, "jpg_src", bgra, step_bytes, cols, rows, &d)) return e;
  return jpeg_encode_many(c, 1, &d, cols, rows, p, &jpg_out, cap, size_out);
}

int pf_jpeg_encode_batch_dev(pf_ctx* c, int n, const uint8_t* const* d_bgra, int cols, int rows, const pf_jpeg_params* params, uint8_t* const* jpg_out, size_t cap_each,
                             size_t* sizes_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (n < 0 || !d_bgra || !jpg_out || !sizes_out) return fail(c, PF_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  if (int e = check_image(c, cols, rows)) return e;
  pf_jpeg_params p;
  if (int e = jpeg_check(c, cols, rows, params, &p)) return e;
  return jpeg_encode_many(c, n, d_bgra, cols, rows, p, jpg_out, cap_each, sizes_out);
}

// The composite the last pf_stitch_step / pf_stitch_step_planned left in HBM (what r == NULL chains on), read in place
int pf_stitch_result_jpeg(pf_ctx* c, const pf_jpeg_params* params, uint8_t* jpg_out, size_t cap, size_t* size_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!jpg_out || !size_out) return fail(c, PF_ERR_ARG, "null pointer");
  DevImage r;
  if (int e = resident_result(c, "pf_stitch_result_jpeg", nullptr, &r)) return e;
  pf_jpeg_params p;
  if (int e = jpeg_check(c, r.cols, r.rows, params, &p)) return e;
  return jpeg_encode_many(c, 1, &r.p, r.cols, r.rows, p, &jpg_out, cap, size_out);
}

// ... and frame slot `frame` of the last host-form pf_stitch_step_batch* call
int pf_stitch_batch_result_jpeg(pf_ctx* c, int frame, const pf_jpeg_params* params, uint8_t* jpg_out, size_t cap, size_t* size_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!jpg_out || !size_out) return fail(c, PF_ERR_ARG, "null pointer");
  DevImage r;
  if (int e = resident_result(c, "pf_stitch_batch_result_jpeg", &frame, &r)) return e;
  pf_jpeg_params p;
  if (int e = jpeg_check(c, r.cols, r.rows, params, &p)) return e;
  return jpeg_encode_many(c, 1, &r.p, r.cols, r.rows, p, &jpg_out, cap, size_out);
}
