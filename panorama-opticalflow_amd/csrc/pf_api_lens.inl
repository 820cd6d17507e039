// Part of pf_api.hip (one translation unit): the lens remap's entry points.  The host checks the arguments, makes the tables a launch
// reads (reproject_math.hpp: the Catmull-Rom phases once per context, the canvas's sines and cosines per canvas size) and launches
// k_lens_remap (kernels_lens.hip); all geometry and sampling runs there.  The scratch ("ln_*") is the remap's own: no entry point here
// touches the chain, the frame slots, the plans or the reprojection's scratch ("rp_*").
}  // extern "C"
namespace {

// everything known without an image pointer of one lens; on success *out holds the kernel's form of it
int lens_check_one(pf_ctx* c, const pf_lens* p, int k, lens::Lens* out) {
  if (p->model < PF_LENS_RECTILINEAR || p->model > PF_LENS_FISHEYE_EQUISOLID)
    return fail(c, PF_ERR_ARG, "lens %d: unknown model %d (0 RECTILINEAR, 1 FISHEYE_EQUIDISTANT, 2 FISHEYE_STEREOGRAPHIC, 3 FISHEYE_EQUISOLID)", k, p->model);
  if (p->filter != PF_REPROJECT_BILINEAR && p->filter != PF_REPROJECT_BICUBIC) return fail(c, PF_ERR_ARG, "lens %d: unknown filter %d (2 BILINEAR, 3 BICUBIC)", k, p->filter);
  const double vals[8] = {p->focal_px, p->a, p->b, p->c, p->dd, p->shift_x, p->shift_y, p->min_cos};
  static const char* const names[8] = {"focal_px", "a", "b", "c", "dd", "shift_x", "shift_y", "min_cos"};
  for (int q = 0; q < 8; ++q)
    if (!std::isfinite(vals[q])) return fail(c, PF_ERR_ARG, "lens %d: %s is not finite", k, names[q]);
  for (int q = 0; q < 9; ++q)
    if (!std::isfinite(p->rot[q])) return fail(c, PF_ERR_ARG, "lens %d: rot[%d] is not finite", k, q);
  if (!(p->focal_px > 0.0)) return fail(c, PF_ERR_ARG, "lens %d: focal_px %g is not positive", k, p->focal_px);
  if (!(p->min_cos >= -1.0 && p->min_cos < 1.0)) return fail(c, PF_ERR_ARG, "lens %d: min_cos %g outside [-1, 1)", k, p->min_cos);
  if (p->model == PF_LENS_RECTILINEAR && p->min_cos < 0.0) return fail(c, PF_ERR_ARG, "lens %d: min_cos %g below 0 for a rectilinear lens", k, p->min_cos);
  if (p->crop_r256 < 0) return fail(c, PF_ERR_ARG, "lens %d: negative crop_r256 %d", k, p->crop_r256);
  out->model = p->model;
  out->crop_cx256 = p->crop_cx256; out->crop_cy256 = p->crop_cy256; out->crop_r256 = p->crop_r256;
  out->focal_px = p->focal_px; out->a = p->a; out->b = p->b; out->c = p->c; out->dd = p->dd;
  out->shift_x = p->shift_x; out->shift_y = p->shift_y; out->min_cos = p->min_cos;
  for (int q = 0; q < 9; ++q) out->rot[q] = p->rot[q];
  return 0;
}

// the sizes and the n lenses; on success *g holds the sizes and out[0 .. n) the lenses
int lens_check(pf_ctx* c, int photo_cols, int photo_rows, int cols, int rows, int n, const pf_lens* p, lens::Geometry* g, std::vector<lens::Lens>* out) {
  if (!p) return fail(c, PF_ERR_ARG, "null pointer (lens)");
  if (int e = check_image(c, photo_cols, photo_rows)) return e;
  if (cols <= 0 || rows <= 0) return fail(c, PF_ERR_ARG, "lens: bad canvas size %dx%d", cols, rows);
  if (photo_cols > kRpMaxSide || photo_rows > kRpMaxSide || cols > kRpMaxSide || rows > kRpMaxSide)
    return fail(c, PF_ERR_ARG, "lens: a side of %dx%d -> %dx%d is above %d", photo_cols, photo_rows, cols, rows, kRpMaxSide);
  if ((double)cols * rows > 2.0e9) return fail(c, PF_ERR_ARG, "lens: canvas %dx%d too large", cols, rows);
  out->resize(n);
  for (int k = 0; k < n; ++k)
    if (int e = lens_check_one(c, p + k, k, out->data() + k)) return e;
  g->filter = 0;
  g->photo_cols = photo_cols; g->photo_rows = photo_rows; g->cols = cols; g->rows = rows;
  return 0;
}

// n device photos -> n device canvases, image k under lenses[k] and filters[k], enqueued on s_main in launches of up to kMaxBatch images
// of one filter; the caller drains
int lens_many(pf_ctx* c, int n, const uint8_t* const* d_src, uint8_t* const* d_dst, const lens::Geometry& g, const lens::Lens* lenses, const pf_lens* params) {
  const size_t in_bytes = size_t(g.photo_cols) * g.photo_rows * 4, out_bytes = size_t(g.cols) * g.rows * 4;
  if (int e = check_dev_images(c, "lens", n, d_src, in_bytes, d_dst, out_bytes, "canvas", "photo")) return e;
  bool cubic = false;
  for (int k = 0; k < n; ++k) cubic = cubic || params[k].filter == PF_REPROJECT_BICUBIC;
  LensArgs a;
  memset(&a, 0, sizeof a);
  a.g = g;
  if (int e = sphere_tables(c, c->ln_tab, cubic, true, g.cols, g.rows, &a.eq, &a.cubic)) return e;
  for (int filter : {PF_REPROJECT_BILINEAR, PF_REPROJECT_BICUBIC}) {
    a.g.filter = filter;
    int count = 0;
    for (int k = 0; k <= n; ++k) {
      if (k < n && params[k].filter == filter) { a.src[count] = (const uint32_t*)d_src[k]; a.dst[count] = (uint32_t*)d_dst[k]; a.lens[count] = lenses[k]; ++count; }
      if (count == kMaxBatch || (k == n && count > 0)) {
        PROF(c, c->s_main, "lens");
        launch_lens_remap(c->s_main, count, a);
        count = 0;
      }
    }
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

}  // namespace
extern "C" {

void pf_lens_init(pf_lens* p, int model) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->model = model; p->filter = PF_REPROJECT_BICUBIC;
  p->dd = 1.0;
  p->min_cos = model == PF_LENS_RECTILINEAR ? 0.0 : -0.5;
  p->rot[0] = p->rot[4] = p->rot[8] = 1.0;
}

double pf_lens_focal(int model, int photo_cols, double hfov_deg) { return lens::focal(model, photo_cols, hfov_deg); }

void pf_lens_rotation(double yaw_deg, double pitch_deg, double roll_deg, double* rot_out) {
  if (rot_out) lens::rotation(yaw_deg, pitch_deg, roll_deg, rot_out);
}

int pf_lens_remap_dev(pf_ctx* c, const uint8_t* d_photo_bgra, int photo_cols, int photo_rows, uint8_t* d_canvas_bgra, int cols, int rows, const pf_lens* params) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_photo_bgra || !d_canvas_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  lens::Geometry g;
  std::vector<lens::Lens> l;
  if (int e = lens_check(c, photo_cols, photo_rows, cols, rows, 1, params, &g, &l)) return e;
  if (int e = lens_many(c, 1, &d_photo_bgra, &d_canvas_bgra, g, l.data(), params)) return e;
  return finish(c);
}

int pf_lens_remap(pf_ctx* c, const uint8_t* photo_bgra, size_t photo_step, int photo_cols, int photo_rows, uint8_t* canvas_bgra, size_t canvas_step, int cols, int rows,
                  const pf_lens* params) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!photo_bgra || !canvas_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  lens::Geometry g;
  std::vector<lens::Lens> l;
  if (int e = lens_check(c, photo_cols, photo_rows, cols, rows, 1, params, &g, &l)) return e;
  if (photo_step < size_t(photo_cols) * 4 || canvas_step < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  if (ranges_overlap(canvas_bgra, bgra_span(cols, rows, canvas_step), photo_bgra, bgra_span(photo_cols, photo_rows, photo_step))) return fail(c, PF_ERR_ARG, "lens: the canvas overlaps the photo");
  const uint8_t* d_src;
  if (int e = upload_bgra(c, "ln_src", photo_bgra, photo_step, photo_cols, photo_rows, &d_src)) return e;
  uint8_t* d_dst = (uint8_t*)ensure(c, "ln_dst", size_t(cols) * rows * 4);
  if (!d_dst) return PF_ERR_NOMEM;
  if (int e = lens_many(c, 1, &d_src, &d_dst, g, l.data(), params)) return e;
  if (int e = down_plane(c, canvas_bgra, canvas_step, d_dst, cols, rows, 4)) return e;
  return finish(c);
}

int pf_lens_remap_batch_dev(pf_ctx* c, int n, const uint8_t* const* d_photos_bgra, int photo_cols, int photo_rows, uint8_t* const* d_canvases_bgra, int cols, int rows,
                            const pf_lens* lenses) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (n < 0 || !d_photos_bgra || !d_canvases_bgra) return fail(c, PF_ERR_ARG, "bad argument");
  lens::Geometry g;
  std::vector<lens::Lens> l;
  if (int e = lens_check(c, photo_cols, photo_rows, cols, rows, n, lenses, &g, &l)) return e;
  if (n == 0) return 0;
  if (int e = lens_many(c, n, d_photos_bgra, d_canvases_bgra, g, l.data(), lenses)) return e;
  return finish(c);
}

// stage entry: the quantised photo coordinates of every canvas pixel as the DEVICE computes them, int32 planes of cols x rows
int pf_stage_lens_coords(pf_ctx* c, int photo_cols, int photo_rows, int cols, int rows, const pf_lens* params, int32_t* fx_out, int32_t* fy_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!fx_out || !fy_out) return fail(c, PF_ERR_ARG, "null pointer");
  LensArgs a;
  memset(&a, 0, sizeof a);
  std::vector<lens::Lens> l;
  if (int e = lens_check(c, photo_cols, photo_rows, cols, rows, 1, params, &a.g, &l)) return e;
  a.g.filter = params->filter; a.lens[0] = l[0];
  const size_t bytes = size_t(cols) * rows * 4;
  a.fx_out = (int*)ensure(c, "ln_fx", bytes); a.fy_out = (int*)ensure(c, "ln_fy", bytes);
  if (!a.fx_out || !a.fy_out) return PF_ERR_NOMEM;
  if (int e = sphere_tables(c, c->ln_tab, false, true, cols, rows, &a.eq, &a.cubic)) return e;   // (no destination: no tap, no phase table)
  { PROF(c, c->s_main, "lens"); launch_lens_remap(c->s_main, 1, a); }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(fx_out, a.fx_out, bytes, hipMemcpyDeviceToHost, c->s_main));
  HIPCHK(c, hipMemcpyAsync(fy_out, a.fy_out, bytes, hipMemcpyDeviceToHost, c->s_main));
  return finish(c);
}
