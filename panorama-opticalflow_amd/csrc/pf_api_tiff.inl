// Part of pf_api.hip (one translation unit): the TIFF decoder's entry points.  The host parses the first IFD (tiff_parse.hpp) and
// uploads the file's bytes and its strip tables; the strips decode in kernels_tiff.hip, one workgroup each, and one workgroup per row
// undoes the predictor and stores BGRA.  Only the compressed file crosses the link.  The scratch ("tiff_*") is the decoder's own: no
// entry point here touches the chain, the prefetch records, the batch slots, the plans or what pf_stitch_visualize reads.
// Deflate files are refused unless the context's switch is on (pf_tiff_set_inflate); then their strips go to k_tiff_inflate, and a
// deflate strip is bad when it is short OR carries a reason (a wrong Adler-32 is full and wrong).
}  // extern "C"
namespace {

const char* tiff_reason(unsigned r) {
  switch (r) {
    case kTiffBadCode: return "an LZW code the encoder cannot have produced";
    case kTiffBadTableFull: return "an LZW code beyond the full table";
    case kTiffCutPacket: return "a PackBits packet runs past the strip";
    case kTiffZlibHeader: return "a bad zlib header";
    case kTiffBlockHeader: return "a bad deflate block header";
    case kTiffCodeLengths: return "a bad deflate code lengths set";
    case kTiffInvalidSymbol: return "an invalid deflate symbol";
    case kTiffFarBack: return "a deflate distance too far back";
    case kTiffDataCheck: return "the Adler-32 does not match";
    default: return "the stream ends early";
  }
}

// what is known before any work: pointers, the IFD, the size the caller expects, a compression the device decodes, whole uncompressed strips
int tiff_check_file(pf_ctx* c, int k, const uint8_t* file, size_t bytes, int cols, int rows, const uint8_t* d_out, tiff_parse::Info* info) {
  std::string why;
  if (!file || !d_out) return fail(c, PF_ERR_ARG, "null pointer (file %d)", k);
  if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(c, PF_ERR_ARG, "tiff: device image %d is not 4-byte aligned", k);
  if (!tiff_parse::parse(file, bytes, info, &why)) return fail(c, PF_ERR_ARG, "tiff: file %d: %s", k, why.c_str());
  const tiff_parse::Info& f = *info;
  if ((long long)f.cols != cols || (long long)f.rows != rows) return fail(c, PF_ERR_ARG, "tiff: file %d is %u x %u, the caller expects %d x %d", k, f.cols, f.rows, cols, rows);
  const bool deflate = f.compression == 8 || f.compression == 32946;
  if (deflate && !c->tiff_inflate) return fail(c, PF_ERR_ARG, "tiff: file %d is deflate-compressed (compression %u), which the device does not decode; use the host reader", k, f.compression);
  if (!(deflate ? tiff_parse::device_decodable_with_inflate(f) : tiff_parse::device_decodable(f))) return fail(c, PF_ERR_ARG, "tiff: file %d is not device-decodable (compression %u, %u rows per strip)", k, f.compression, f.rows_per_strip);
  if (f.compression == 1)   // known from the tables alone: no kernel needs to find it
    for (size_t s = 0; s < f.n_strips(); ++s)
      if (f.counts[s] < f.strip_bytes(s)) return fail(c, PF_ERR_ARG, "tiff: file %d: strip %zu is short: %u of %llu bytes", k, s, f.counts[s], (unsigned long long)f.strip_bytes(s));
  return 0;
}

// n <= kMaxBatch files of cols x rows -> n packed device images.  Every file's kernels are enqueued before the one drain; then all
// strips' status words come down in one copy.  A bad or short strip fails the call and zero-fills every output: this group's and the
// `done` outputs in front of them that earlier groups of the same call delivered.
int tiff_decode_group(pf_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, int cols, int rows, uint8_t* const* d_out, int done) {
  std::vector<tiff_parse::Info> info(n);
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t file_total = 0, plane_total = 0, tab_total = 0, strips_total = 0;
  std::vector<size_t> file_at(n), plane_at(n), tab_at(n), status_at(n);
  for (int k = 0; k < n; ++k) {
    if (int e = tiff_check_file(c, done + k, files[k], bytes[k], cols, rows, d_out[k], &info[k])) return e;
    const tiff_parse::Info& f = info[k];
    file_at[k] = file_total; file_total += al(bytes[k]);
    plane_at[k] = plane_total; plane_total += f.compression == 1 ? 0 : al(size_t(f.row_bytes()) * f.rows);
    tab_at[k] = tab_total; tab_total += al(f.n_strips() * 8);
    status_at[k] = strips_total; strips_total += f.n_strips();
  }
  uint8_t* d_file = (uint8_t*)ensure(c, "tiff_file", file_total); uint8_t* d_plane = (uint8_t*)ensure(c, "tiff_samples", std::max<size_t>(plane_total, 256));
  uint8_t* d_tab = (uint8_t*)ensure(c, "tiff_tab", tab_total); unsigned long long* d_status = (unsigned long long*)ensure(c, "tiff_status", strips_total * 8);
  if (!d_file || !d_plane || !d_tab || !d_status) return PF_ERR_NOMEM;
  hipStream_t sm = c->s_main;
  HIPCHK(c, hipMemsetAsync(d_status, 0, strips_total * 8, sm));   // (uncompressed files launch no strip kernel: their words stay 0 and are not read)
  for (int k = 0; k < n; ++k) {
    const tiff_parse::Info& f = info[k];
    const size_t ns = f.n_strips();
    HIPCHK(c, hipMemcpyAsync(d_file + file_at[k], files[k], bytes[k], hipMemcpyHostToDevice, sm));
    HIPCHK(c, hipMemcpyAsync(d_tab + tab_at[k], f.offsets.data(), ns * 4, hipMemcpyHostToDevice, sm));   // (info[] outlives the drain below)
    HIPCHK(c, hipMemcpyAsync(d_tab + tab_at[k] + ns * 4, f.counts.data(), ns * 4, hipMemcpyHostToDevice, sm));
    TiffWork w;
    w.file = d_file + file_at[k]; w.bytes = bytes[k];
    w.offsets = (const uint32_t*)(d_tab + tab_at[k]); w.counts = w.offsets + ns;
    w.n_strips = (int)ns; w.cols = cols; w.rows = rows; w.samples = (int)f.samples; w.rows_per_strip = (int)f.rows_per_strip; w.predictor = (int)f.predictor;
    w.plane = d_plane + plane_at[k]; w.status = d_status + status_at[k];
    if (f.compression == 5) { PROF(c, sm, "tiff_lzw"); launch_tiff_lzw(sm, w); }
    else if (f.compression == 32773) { PROF(c, sm, "tiff_packbits"); launch_tiff_packbits(sm, w); }
    else if (f.compression == 8 || f.compression == 32946) { PROF(c, sm, "tiff_inflate"); launch_tiff_inflate(sm, w); }
    { PROF(c, sm, "tiff_finish"); launch_tiff_finish(sm, w, f.compression == 1, d_out[k]); }
  }
  std::vector<unsigned long long> status(strips_total);
  HIPCHK(c, hipMemcpyAsync(status.data(), d_status, strips_total * 8, hipMemcpyDeviceToHost, sm));
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  for (int k = 0; k < n; ++k) {
    const tiff_parse::Info& f = info[k];
    if (f.compression == 1) continue;
    for (size_t s = 0; s < f.n_strips(); ++s) {
      const unsigned long long st = status[status_at[k] + s];
      // a deflate strip is also bad when it is full and zlib refuses it (a wrong Adler-32, an error behind the last byte)
      if ((st & 0xffffffffull) == f.strip_bytes(s) && !((f.compression == 8 || f.compression == 32946) && (st >> 32))) continue;
      c->drained = false;
      for (int q = -done; q < n; ++q) HIPCHK(c, hipMemsetAsync(d_out[q], 0, size_t(cols) * rows * 4, sm));
      if (int e = finish(c)) return e;
      return fail(c, PF_ERR_ARG, "tiff: file %d: strip %zu decoded %llu of %llu bytes (%s); the device path refuses the file", done + k, s, st & 0xffffffffull,
                  (unsigned long long)f.strip_bytes(s), tiff_reason((unsigned)(st >> 32)));
    }
  }
  return 0;
}

int tiff_decode_many(pf_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, int cols, int rows, uint8_t* const* d_out) {
  if (n > kMaxBatch) {   // a call of several groups: every file's refusal comes before any group's work
    tiff_parse::Info info;
    for (int k = 0; k < n; ++k) if (int e = tiff_check_file(c, k, files[k], bytes[k], cols, rows, d_out[k], &info)) return e;
  }
  for (int first = 0; first < n; first += kMaxBatch) {
    const int count = std::min(kMaxBatch, n - first);
    if (int e = tiff_decode_group(c, count, files + first, bytes + first, cols, rows, d_out + first, first)) return e;
  }
  return 0;
}

}  // namespace
extern "C" {

int pf_tiff_probe(pf_ctx* c, const uint8_t* file, size_t bytes, pf_tiff_info* out) {
  if (!file || !out) return fail(c, PF_ERR_ARG, "null pointer");
  if (out->struct_size != (int)sizeof(pf_tiff_info)) return fail(c, PF_ERR_ARG, "pf_tiff_probe: struct_size does not match this library's pf_tiff_info");
  tiff_parse::Info f;
  std::string why;
  if (!tiff_parse::parse(file, bytes, &f, &why)) return fail(c, PF_ERR_ARG, "tiff: %s", why.c_str());
  if (f.cols > 0x7fffffffu || f.rows > 0x7fffffffu) return fail(c, PF_ERR_ARG, "tiff: TIFF too large");
  out->cols = (int)f.cols; out->rows = (int)f.rows; out->samples = (int)f.samples; out->compression = (int)f.compression; out->predictor = (int)f.predictor;
  out->rows_per_strip = (int)f.rows_per_strip; out->n_strips = (int)f.n_strips(); out->big_endian = f.big_endian ? 1 : 0;
  out->device_decodable = (tiff_parse::device_decodable(f) && (double)f.cols * f.rows <= 2.0e9) ? 1 : 0;
  return 0;
}

int pf_tiff_set_inflate(pf_ctx* c, int on) {
  if (!c) return fail(nullptr, PF_ERR_ARG, "null context");
  c->tiff_inflate = on != 0;
  return 0;
}

int pf_tiff_device_decodable(const pf_ctx* c, const pf_tiff_info* info) {
  if (!info || info->struct_size != (int)sizeof(pf_tiff_info) || info->cols <= 0 || info->rows <= 0 || info->rows_per_strip <= 0) return 0;
  tiff_parse::Info f;
  f.cols = (uint32_t)info->cols; f.rows = (uint32_t)info->rows; f.samples = (uint32_t)info->samples; f.compression = (uint32_t)info->compression;
  f.rows_per_strip = (uint32_t)info->rows_per_strip;
  const bool ok = (c && c->tiff_inflate) ? tiff_parse::device_decodable_with_inflate(f) : tiff_parse::device_decodable(f);
  return (ok && (double)f.cols * f.rows <= 2.0e9) ? 1 : 0;
}

int pf_tiff_decode_dev(pf_ctx* c, const uint8_t* file, size_t bytes, int cols, int rows, uint8_t* d_out_bgra) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!file || !d_out_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  return tiff_decode_many(c, 1, &file, &bytes, cols, rows, &d_out_bgra);
}

int pf_tiff_decode(pf_ctx* c, const uint8_t* file, size_t bytes, int cols, int rows, uint8_t* out_bgra, size_t out_step) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!file || !out_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (out_step < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  uint8_t* d = (uint8_t*)ensure(c, "tiff_dst", size_t(cols) * rows * 4);
  if (!d) return PF_ERR_NOMEM;
  if (int e = tiff_decode_many(c, 1, &file, &bytes, cols, rows, &d)) return e;   // on failure the host image is not written
  c->drained = false;
  if (int e = down_plane(c, out_bgra, out_step, d, cols, rows, 4)) return e;
  return finish(c);
}

int pf_tiff_decode_batch_dev(pf_ctx* c, int n, const uint8_t* const* files, const size_t* bytes, int cols, int rows, uint8_t* const* d_out_bgra) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (n < 0 || !files || !bytes || !d_out_bgra) return fail(c, PF_ERR_ARG, "bad argument");
  if (n == 0) return 0;
  if (int e = check_image(c, cols, rows)) return e;
  return tiff_decode_many(c, n, files, bytes, cols, rows, d_out_bgra);
}
