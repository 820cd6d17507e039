// Part of pf_api.hip (one translation unit): the JPEG decoder's entry points.  The host parses the markers up to the scan
// (jpeg_parse.hpp) and uploads the file's bytes as they are and the decode tables; the entropy segment is decoded in kernels_jpegd.hip by
// self-synchronising lanes, launch after launch until no lane's exit state changes, then written, summed, transformed and packed to BGRA.
// Only the compressed file crosses the link.  The scratch ("jd_*") is the decoder's own: no entry point here touches the chain, the
// prefetch records, the batch slots, the plans or another family's scratch.

static unsigned jpegd_subseq() {
  unsigned s = kJpegdSubseq;
#ifdef PF_EXPERIMENTS
  // lab build only: tests/micro/jpeg_decode_ab.py measures the product's subsequence size against the others; the tests run the seams at the smallest
  if (const char* e = getenv("PANOFLOW_JPEGD_SUBSEQ")) { const unsigned v = (unsigned)atoi(e); if (v >= kJpegdSubseqMin && v <= kJpegdSubseqMax && !(v & (v - 1))) s = v; }
#endif
  return s;
}
}  // extern "C"
namespace {

struct JpegdSizes { size_t states, first, coef, planes, dcsum; unsigned nsub; };
JpegdSizes jpegd_sizes(const jpeg_parse::Info& f, unsigned S) {
  JpegdSizes z;
  const uint64_t seg = f.end - f.begin;
  z.nsub = (unsigned)std::max<uint64_t>(1, (seg + S - 1) / S);
  z.states = size_t(z.nsub) * 16; z.first = size_t(z.nsub) * 8;
  z.coef = size_t(f.blocks()) * 64 * 2;
  z.planes = size_t(f.mcus()) * 64 * (f.ncomp == 3 ? f.hs * f.vs + 2 : 1);
  z.dcsum = size_t(f.intervals()) * f.ncomp * jpegd_dc_chunks(f.ncomp, f.hs, f.vs, f.restart, (unsigned)f.mcus()) * 4;
  return z;
}

// what is known before any work: pointers, the header, the size the caller expects
int jpegd_check_file(pf_ctx* c, int k, const uint8_t* file, size_t bytes, int cols, int rows, const uint8_t* d_out, jpeg_parse::Info* info) {
  std::string why;
  if (!file || !d_out) return fail(c, PF_ERR_ARG, "null pointer (file %d)", k);
  if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(c, PF_ERR_ARG, "jpeg: device image %d is not 4-byte aligned", k);
  if (!jpeg_parse::parse(file, bytes, info, &why)) return fail(c, PF_ERR_ARG, "jpeg: file %d: %s", k, why.c_str());
  if ((long long)info->cols != cols || (long long)info->rows != rows)
    return fail(c, PF_ERR_ARG, "jpeg: file %d is %u x %u, the caller expects %d x %d", k, info->cols, info->rows, cols, rows);
  return 0;
}

struct JpegdStage { uint32_t* states; int16_t* coef; uint8_t* planes; int* counts; };   // pf_stage_jpeg_decode's host outputs

// n <= kMaxBatch files of cols x rows -> n packed device images.  Every file's kernels of a step are enqueued before the step's one
// drain: the synchronisation launches (all files still changing, then their "changed" words in one copy), then write, sums, IDCT and
// pixels of all files and their status words in one copy.  An event on a file's true path fails the call and zero-fills every output:
// this group's, the `done` outputs in front of them that earlier groups of the same call delivered, and the `after` behind them.
int jpegd_decode_group(pf_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, int cols, int rows, uint8_t* const* d_out, int done, int after, const JpegdStage* stage = nullptr) {
  std::vector<jpeg_parse::Info> info(n);
  const unsigned S = jpegd_subseq();
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t file_total = 0, st_total = 0, first_total = 0, coef_total = 0, plane_total = 0, dc_total = 0;
  std::vector<size_t> file_at(n), st_at(n), first_at(n), coef_at(n), plane_at(n), dc_at(n);
  std::vector<JpegdSizes> sz(n);
  for (int k = 0; k < n; ++k) {
    if (int e = jpegd_check_file(c, done + k, files[k], bytes[k], cols, rows, d_out[k], &info[k])) return e;
    sz[k] = jpegd_sizes(info[k], S);
    file_at[k] = file_total; file_total += al(bytes[k]);
    st_at[k] = st_total; st_total += 2 * al(sz[k].states);
    first_at[k] = first_total; first_total += al(sz[k].first);
    coef_at[k] = coef_total; coef_total += al(sz[k].coef);
    plane_at[k] = plane_total; plane_total += al(sz[k].planes);
    dc_at[k] = dc_total; dc_total += al(sz[k].dcsum);
  }
  uint8_t* d_file = (uint8_t*)ensure(c, "jd_file", file_total); uint8_t* d_tab = (uint8_t*)ensure(c, "jd_tables", al(sizeof(jpeg_parse::Tables)) * n);
  uint8_t* d_st = (uint8_t*)ensure(c, "jd_states", st_total); uint8_t* d_first = (uint8_t*)ensure(c, "jd_first", first_total);
  uint8_t* d_coef = (uint8_t*)ensure(c, "jd_coef", coef_total); uint8_t* d_planes = (uint8_t*)ensure(c, "jd_planes", plane_total);
  unsigned* d_words = (unsigned*)ensure(c, "jd_words", size_t(n) * 16); uint8_t* d_dc = (uint8_t*)ensure(c, "jd_dcsum", dc_total);
  if (!d_file || !d_tab || !d_st || !d_first || !d_coef || !d_planes || !d_words || !d_dc) return PF_ERR_NOMEM;
  hipStream_t sm = c->s_main;
  std::vector<JpegdWork> w(n);
  std::vector<unsigned> words(size_t(n) * 4);
  for (int k = 0; k < n; ++k) { words[4 * k] = 0; words[4 * k + 1] = 0; words[4 * k + 2] = 0xFFFFFFFFu; words[4 * k + 3] = 0; }
  HIPCHK(c, hipMemcpyAsync(d_words, words.data(), size_t(n) * 16, hipMemcpyHostToDevice, sm));
  HIPCHK(c, hipMemsetAsync(d_coef, 0, coef_total, sm));
  for (int k = 0; k < n; ++k) {
    const jpeg_parse::Info& f = info[k];
    HIPCHK(c, hipMemcpyAsync(d_file + file_at[k], files[k], bytes[k], hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemcpyAsync(d_tab + k * al(sizeof(jpeg_parse::Tables)), &f.tab, sizeof(jpeg_parse::Tables), hipMemcpyHostToDevice, sm));   // (info[] outlives the drains)
    JpegdWork& x = w[k];
    x.seg = d_file + file_at[k] + f.begin; x.seg_bytes = (unsigned)(f.end - f.begin); x.S = S; x.nsub = sz[k].nsub;
    x.ncomp = f.ncomp; x.hs = f.hs; x.vs = f.vs; x.restart = f.restart; x.cols = f.cols; x.rows = f.rows;
    x.tables = d_tab + k * al(sizeof(jpeg_parse::Tables));
    x.states[0] = d_st + st_at[k]; x.states[1] = d_st + st_at[k] + al(sz[k].states);
    x.words = d_words + 4 * k; x.first = d_first + first_at[k]; x.coef = (int16_t*)(d_coef + coef_at[k]); x.planes = d_planes + plane_at[k];
    x.dcsum = (unsigned*)(d_dc + dc_at[k]);
  }
  // synchronise: a launch per file still changing, until none is.  A file needs at most one launch per workgroup, and one to see it.
  std::vector<int> from(n, 0), live(n, 1), launches(n, 0), rounds(n, 0);
  for (int any = 1; any;) {
    for (int k = 0; k < n; ++k) {
      if (!live[k]) continue;
      PROF(c, sm, "jpegd_sync");
      launch_jpegd_sync(sm, w[k], launches[k] == 0, from[k]);
    }
    HIPCHK(c, hipMemcpyAsync(words.data(), d_words, size_t(n) * 16, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(sm));
    any = 0;
    for (int k = 0; k < n; ++k) {
      if (!live[k]) continue;
      from[k] ^= 1; launches[k] += 1; rounds[k] += (int)words[4 * k + 1];
      const int bound = (int)((w[k].nsub + kJpegdLanes - 1) / kJpegdLanes) + 1;
      if (words[4 * k] && launches[k] > bound) {   // (never expected; nothing was delivered yet, so the outputs are zeroed as for a damaged scan)
        for (int q = -done; q < n + after; ++q) HIPCHK(c, hipMemsetAsync(d_out[q], 0, size_t(cols) * rows * 4, sm));
        HIPCHK(c, hipStreamSynchronize(sm));
      }
      if (words[4 * k] && launches[k] > bound) return fail(c, PF_ERR_DEVICE, "jpeg: file %d: the synchronisation did not settle in %d launches", done + k, bound);
      live[k] = words[4 * k] != 0;
      any |= live[k];
    }
    for (int k = 0; k < n; ++k) if (live[k]) HIPCHK(c, hipMemsetAsync(d_words + 4 * k, 0, 8, sm));   // changed and rounds start again
  }
  for (int k = 0; k < n; ++k) {
    { PROF(c, sm, "jpegd_write"); launch_jpegd_write(sm, w[k], from[k]); }
    { PROF(c, sm, "jpegd_pixels"); launch_jpegd_pixels(sm, w[k], d_out[k]); }
  }
  HIPCHK(c, hipMemcpyAsync(words.data(), d_words, size_t(n) * 16, hipMemcpyDeviceToHost, sm));
  if (stage) {   // one file: what the kernels left, for the tests
    HIPCHK(c, hipMemcpyAsync(stage->states, w[0].states[from[0]], sz[0].states, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipMemcpyAsync(stage->coef, w[0].coef, sz[0].coef, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipMemcpyAsync(stage->planes, w[0].planes, sz[0].planes, hipMemcpyDeviceToHost, sm));
    stage->counts[0] = (int)sz[0].nsub; stage->counts[1] = rounds[0]; stage->counts[2] = launches[0]; stage->counts[3] = (int)S;
  }
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  if (stage) stage->counts[4] = (int)words[3];
  for (int k = 0; k < n; ++k) {
    const unsigned mcu = words[4 * k + 2];
    if (mcu == 0xFFFFFFFFu) continue;
    c->drained = false;
    for (int q = -done; q < n + after; ++q) HIPCHK(c, hipMemsetAsync(d_out[q], 0, size_t(cols) * rows * 4, sm));
    if (int e = finish(c)) return e;
    return fail(c, PF_ERR_ARG, "jpeg: file %d: the scan is damaged: decoding stopped at MCU %u of %llu; the device path refuses the file", done + k, mcu,
                (unsigned long long)info[k].mcus());
  }
  return 0;
}

int jpegd_decode_many(pf_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, int cols, int rows, uint8_t* const* d_out) {
  if (cols > 65535 || rows > 65535) return fail(c, PF_ERR_ARG, "jpeg: %dx%d, the format holds at most 65535 a side", cols, rows);
  {   // every file's refusal comes before any work; no output may lie inside another
    jpeg_parse::Info info;
    for (int k = 0; k < n; ++k) if (int e = jpegd_check_file(c, k, files[k], bytes[k], cols, rows, d_out[k], &info)) return e;
    const size_t ob = size_t(cols) * rows * 4;
    for (int k = 0; k < n; ++k)
      for (int q = k + 1; q < n; ++q)
        if (ranges_overlap(d_out[k], ob, d_out[q], ob)) return fail(c, PF_ERR_ARG, "jpeg: device image %d overlaps device image %d", k, q);
  }
  for (int first = 0; first < n; first += kMaxBatch) {
    const int count = std::min(kMaxBatch, n - first);
    if (int e = jpegd_decode_group(c, count, files + first, bytes + first, cols, rows, d_out + first, first, n - first - count)) return e;
  }
  return 0;
}

}  // namespace
extern "C" {

int pf_jpeg_probe(pf_ctx* c, const uint8_t* file, size_t bytes, pf_jpeg_info* out) {
  if (!file || !out) return fail(c, PF_ERR_ARG, "null pointer");
  if (out->struct_size != (int)sizeof(pf_jpeg_info)) return fail(c, PF_ERR_ARG, "pf_jpeg_probe: struct_size does not match this library's pf_jpeg_info");
  if (bytes < 2 || file[0] != 0xFF || file[1] != 0xD8) return fail(c, PF_ERR_ARG, "jpeg: not a JPEG");
  jpeg_parse::Info f;
  std::string why;
  const bool ok = jpeg_parse::parse(file, bytes, &f, &why);
  out->cols = (int)f.cols; out->rows = (int)f.rows; out->components = f.ncomp; out->subsampling = ok ? f.subsampling() : 0; out->restart_interval = ok ? (int)f.restart : 0;
  out->device_decodable = ok ? 1 : 0;
  memset(out->reason, 0, sizeof out->reason);
  if (!ok) snprintf(out->reason, sizeof out->reason, "%s", why.c_str());
  return 0;
}

int pf_jpeg_decode_dev(pf_ctx* c, const uint8_t* file, size_t bytes, int cols, int rows, uint8_t* d_out_bgra) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!file || !d_out_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  return jpegd_decode_many(c, 1, &file, &bytes, cols, rows, &d_out_bgra);
}

int pf_jpeg_decode(pf_ctx* c, const uint8_t* file, size_t bytes, int cols, int rows, uint8_t* out_bgra, size_t out_step) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!file || !out_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (out_step < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  uint8_t* d = (uint8_t*)ensure(c, "jd_dst", size_t(cols) * rows * 4);
  if (!d) return PF_ERR_NOMEM;
  if (int e = jpegd_decode_many(c, 1, &file, &bytes, cols, rows, &d)) return e;   // on failure the host image is not written
  c->drained = false;
  if (int e = down_plane(c, out_bgra, out_step, d, cols, rows, 4)) return e;
  return finish(c);
}

int pf_jpeg_decode_batch_dev(pf_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, int cols, int rows, uint8_t* const* d_out_bgra) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (n < 0 || !files || !bytes || !d_out_bgra) return fail(c, PF_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  if (int e = check_image(c, cols, rows)) return e;
  return jpegd_decode_many(c, n, files, bytes, cols, rows, d_out_bgra);
}

int pf_stage_jpeg_decode(pf_ctx* c, const uint8_t* file, size_t bytes, uint32_t* states_out, size_t states_cap, int16_t* coef_out, size_t coef_cap, uint8_t* planes_out,
                         size_t planes_cap, int* counts_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!file || !states_out || !coef_out || !planes_out || !counts_out) return fail(c, PF_ERR_ARG, "null pointer");
  jpeg_parse::Info f;
  std::string why;
  if (!jpeg_parse::parse(file, bytes, &f, &why)) return fail(c, PF_ERR_ARG, "jpeg: file 0: %s", why.c_str());
  if (int e = check_image(c, (int)f.cols, (int)f.rows)) return e;
  const JpegdSizes z = jpegd_sizes(f, jpegd_subseq());
  if (states_cap < z.states || coef_cap < z.coef || planes_cap < z.planes)
    return fail(c, PF_ERR_ARG, "pf_stage_jpeg_decode: the outputs need %zu, %zu and %zu bytes", z.states, z.coef, z.planes);
  uint8_t* d = (uint8_t*)ensure(c, "jd_dst", size_t(f.cols) * f.rows * 4);
  if (!d) return PF_ERR_NOMEM;
  const JpegdStage stage = {states_out, coef_out, planes_out, counts_out};
  return jpegd_decode_group(c, 1, &file, &bytes, (int)f.cols, (int)f.rows, &d, 0, 0, &stage);
}
