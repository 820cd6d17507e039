// Part of pf_api.hip (one translation unit): the reprojection entry points.  The host checks the arguments, makes the tables a launch
// reads (reproject_math.hpp: the Catmull-Rom phases once per context, the equirect output's sines and cosines per output size) and
// launches k_reproject (kernels_reproject.hip); all geometry and sampling runs there.  The scratch ("rp_*") is the reprojection's own:
// no entry point here touches the chain, the prefetch records, the batch slots, the plans or what pf_stitch_visualize reads.
}  // extern "C"
namespace {

constexpr int kRpMaxSide = 65535;

// everything known without an image pointer; on success *g holds the launch's geometry
int reproject_check(pf_ctx* c, int cols, int rows, int out_cols, int out_rows, const pf_reproject_params* p, reproject::Geometry* g) {
  if (!p) return fail(c, PF_ERR_ARG, "null pointer (params)");
  if (int e = check_image(c, cols, rows)) return e;
  if (out_cols <= 0 || out_rows <= 0) return fail(c, PF_ERR_ARG, "reproject: bad output size %dx%d", out_cols, out_rows);
  if (cols > kRpMaxSide || rows > kRpMaxSide || out_cols > kRpMaxSide || out_rows > kRpMaxSide)
    return fail(c, PF_ERR_ARG, "reproject: a side of %dx%d -> %dx%d is above %d", cols, rows, out_cols, out_rows, kRpMaxSide);
  if ((double)out_cols * out_rows > 2.0e9) return fail(c, PF_ERR_ARG, "reproject: output %dx%d too large", out_cols, out_rows);
  if (p->projection != PF_PROJ_CUBE && p->projection != PF_PROJ_RECTILINEAR && p->projection != PF_PROJ_EQUIRECT)
    return fail(c, PF_ERR_ARG, "reproject: unknown projection %d (0 CUBE, 1 RECTILINEAR, 2 EQUIRECT)", p->projection);
  if (p->filter != PF_REPROJECT_BILINEAR && p->filter != PF_REPROJECT_BICUBIC) return fail(c, PF_ERR_ARG, "reproject: unknown filter %d (2 BILINEAR, 3 BICUBIC)", p->filter);
  g->t = 0.0;
  if (p->projection == PF_PROJ_CUBE) {
    if (p->face < PF_FACE_FRONT || p->face > PF_FACE_DOWN) return fail(c, PF_ERR_ARG, "reproject: unknown face %d (0 front, right, back, left, up, 5 down)", p->face);
    if (out_cols != out_rows) return fail(c, PF_ERR_ARG, "reproject: a cube face is square, not %dx%d", out_cols, out_rows);
  }
  if (p->projection == PF_PROJ_RECTILINEAR) {
    if (!(p->hfov_deg > 0.0 && p->hfov_deg < 180.0)) return fail(c, PF_ERR_ARG, "reproject: hfov %g outside (0, 180) degrees", p->hfov_deg);
    g->t = reproject::tan_half_fov(p->hfov_deg);
  }
  for (int k = 0; k < 9; ++k) {
    if (!std::isfinite(p->rot[k])) return fail(c, PF_ERR_ARG, "reproject: rot[%d] is not finite", k);
    g->rot[k] = p->rot[k];
  }
  g->projection = p->projection; g->filter = p->filter;
  g->cols = cols; g->rows = rows; g->out_cols = out_cols; g->out_rows = out_rows;
  return 0;
}

// The two tables a launch of either sphere sampler reads (reproject_math.hpp), resident in the family's own slots: the Catmull-Rom
// phases (want_cubic) and the sines and cosines of an equirect grid of cols x rows (want_eq).  A table not wanted comes back null.
int sphere_tables(pf_ctx* c, pf_ctx::SphereTables& t, bool want_cubic, bool want_eq, int cols, int rows, const double** d_eq, const int** d_cubic) {
  const uint8_t *eq = nullptr, *cubic = nullptr;
  if (want_cubic)
    if (int e = resident_table(c, t.cubic_slot, t.cubic, 0, 0, 0, 1024 * sizeof(int), [](uint8_t* h) { reproject::make_cubic_table((int*)h); }, &cubic)) return e;
  if (want_eq)
    if (int e = resident_table(c, t.eq_slot, t.eq, cols, rows, 0, 2 * (size_t(cols) + rows) * sizeof(double),
                               [&](uint8_t* h) { reproject::make_equirect_tables(cols, rows, (double*)h); }, &eq)) return e;
  *d_eq = (const double*)eq; *d_cubic = (const int*)cubic;
  return 0;
}

// n device images of g.cols x g.rows -> n of g.out_cols x g.out_rows, enqueued on s_main in groups of kMaxBatch; the caller drains.
// faces: null (every image takes `face`), or the face of each image.
int reproject_many(pf_ctx* c, int n, const uint8_t* const* d_src, uint8_t* const* d_dst, const reproject::Geometry& g, int face, const int* faces) {
  const size_t in_bytes = size_t(g.cols) * g.rows * 4, out_bytes = size_t(g.out_cols) * g.out_rows * 4;
  if (int e = check_dev_images(c, "reproject", n, d_src, in_bytes, d_dst, out_bytes)) return e;
  ReprojectArgs a;
  memset(&a, 0, sizeof a);
  a.g = g;
  if (int e = sphere_tables(c, c->rp_tab, g.filter == PF_REPROJECT_BICUBIC, g.projection == PF_PROJ_EQUIRECT, g.out_cols, g.out_rows, &a.eq, &a.cubic)) return e;
  for (int first = 0; first < n; first += kMaxBatch) {
    const int count = std::min(kMaxBatch, n - first);
    for (int k = 0; k < count; ++k) {
      a.src[k] = (const uint32_t*)d_src[first + k]; a.dst[k] = (uint32_t*)d_dst[first + k];
      a.face[k] = faces ? faces[first + k] : face;
    }
    PROF(c, c->s_main, "reproject");
    launch_reproject(c->s_main, count, a);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

}  // namespace
extern "C" {

void pf_reproject_params_init(pf_reproject_params* p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->projection = PF_PROJ_CUBE; p->face = PF_FACE_FRONT; p->filter = PF_REPROJECT_BICUBIC; p->hfov_deg = 90.0;
  p->rot[0] = p->rot[4] = p->rot[8] = 1.0;
}

void pf_reproject_rotation(double yaw_deg, double pitch_deg, double roll_deg, double* rot_out) {
  if (rot_out) reproject::rotation(yaw_deg, pitch_deg, roll_deg, rot_out);
}

int pf_reproject_dev(pf_ctx* c, const uint8_t* d_src_bgra, int cols, int rows, uint8_t* d_dst_bgra, int out_cols, int out_rows, const pf_reproject_params* params) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_src_bgra || !d_dst_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  reproject::Geometry g;
  if (int e = reproject_check(c, cols, rows, out_cols, out_rows, params, &g)) return e;
  if (int e = reproject_many(c, 1, &d_src_bgra, &d_dst_bgra, g, params->face, nullptr)) return e;
  return finish(c);
}

int pf_reproject(pf_ctx* c, const uint8_t* src_bgra, size_t src_step, int cols, int rows, uint8_t* dst_bgra, size_t dst_step, int out_cols, int out_rows,
                 const pf_reproject_params* params) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!src_bgra || !dst_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  reproject::Geometry g;
  if (int e = reproject_check(c, cols, rows, out_cols, out_rows, params, &g)) return e;
  if (src_step < size_t(cols) * 4 || dst_step < size_t(out_cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  if (ranges_overlap(dst_bgra, bgra_span(out_cols, out_rows, dst_step), src_bgra, bgra_span(cols, rows, src_step))) return fail(c, PF_ERR_ARG, "reproject: the destination overlaps the source");
  const uint8_t* d_src;
  if (int e = upload_bgra(c, "rp_src", src_bgra, src_step, cols, rows, &d_src)) return e;
  uint8_t* d_dst = (uint8_t*)ensure(c, "rp_dst", size_t(out_cols) * out_rows * 4);
  if (!d_dst) return PF_ERR_NOMEM;
  if (int e = reproject_many(c, 1, &d_src, &d_dst, g, params->face, nullptr)) return e;
  if (int e = down_plane(c, dst_bgra, dst_step, d_dst, out_cols, out_rows, 4)) return e;
  return finish(c);
}

int pf_reproject_batch_dev(pf_ctx* c, int n, const uint8_t* const* d_src_bgra, int cols, int rows, uint8_t* const* d_dst_bgra, int out_cols, int out_rows,
                           const pf_reproject_params* params) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (n < 0 || !d_src_bgra || !d_dst_bgra) return fail(c, PF_ERR_ARG, "bad argument");
  reproject::Geometry g;
  if (int e = reproject_check(c, cols, rows, out_cols, out_rows, params, &g)) return e;
  if (n == 0) return 0;
  if (int e = reproject_many(c, n, d_src_bgra, d_dst_bgra, g, params->face, nullptr)) return e;
  return finish(c);
}

// the six faces of one source in one launch (blockIdx.z = face); params->projection and params->face are not read
int pf_reproject_cube_dev(pf_ctx* c, const uint8_t* d_src_bgra, int cols, int rows, uint8_t* const* d_faces_bgra, int face_size, const pf_reproject_params* params) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_src_bgra || !d_faces_bgra || !params) return fail(c, PF_ERR_ARG, "null pointer");
  pf_reproject_params p = *params;
  p.projection = PF_PROJ_CUBE; p.face = PF_FACE_FRONT;
  reproject::Geometry g;
  if (int e = reproject_check(c, cols, rows, face_size, face_size, &p, &g)) return e;
  const uint8_t* srcs[6];
  int faces[6];
  for (int k = 0; k < 6; ++k) { srcs[k] = d_src_bgra; faces[k] = k; }
  if (int e = reproject_many(c, 6, srcs, d_faces_bgra, g, 0, faces)) return e;
  return finish(c);
}

// The composite the last pf_stitch_step / pf_stitch_step_planned left in HBM, read in place
int pf_stitch_result_reprojected_dev(pf_ctx* c, int out_cols, int out_rows, const pf_reproject_params* params, uint8_t* d_dst_bgra) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_dst_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  DevImage r;
  if (int e = resident_result(c, "pf_stitch_result_reprojected_dev", nullptr, &r)) return e;
  reproject::Geometry g;
  if (int e = reproject_check(c, r.cols, r.rows, out_cols, out_rows, params, &g)) return e;
  if (int e = reproject_many(c, 1, &r.p, &d_dst_bgra, g, params->face, nullptr)) return e;
  return finish(c);
}

// ... and frame slot `frame` of the last host-form pf_stitch_step_batch* call
int pf_stitch_batch_result_reprojected_dev(pf_ctx* c, int frame, int out_cols, int out_rows, const pf_reproject_params* params, uint8_t* d_dst_bgra) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_dst_bgra) return fail(c, PF_ERR_ARG, "null pointer");
  DevImage r;
  if (int e = resident_result(c, "pf_stitch_batch_result_reprojected_dev", &frame, &r)) return e;
  reproject::Geometry g;
  if (int e = reproject_check(c, r.cols, r.rows, out_cols, out_rows, params, &g)) return e;
  if (int e = reproject_many(c, 1, &r.p, &d_dst_bgra, g, params->face, nullptr)) return e;
  return finish(c);
}

// stage entry: the quantised source coordinates of every output pixel as the DEVICE computes them, int32 planes of out_cols x out_rows
int pf_stage_reproject_coords(pf_ctx* c, int cols, int rows, int out_cols, int out_rows, const pf_reproject_params* params, int32_t* fx_out, int32_t* fy_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!fx_out || !fy_out) return fail(c, PF_ERR_ARG, "null pointer");
  ReprojectArgs a;
  memset(&a, 0, sizeof a);
  if (int e = reproject_check(c, cols, rows, out_cols, out_rows, params, &a.g)) return e;
  const size_t bytes = size_t(out_cols) * out_rows * 4;
  a.fx_out = (int*)ensure(c, "rp_fx", bytes); a.fy_out = (int*)ensure(c, "rp_fy", bytes);
  if (!a.fx_out || !a.fy_out) return PF_ERR_NOMEM;
  if (int e = sphere_tables(c, c->rp_tab, a.g.filter == PF_REPROJECT_BICUBIC, a.g.projection == PF_PROJ_EQUIRECT, out_cols, out_rows, &a.eq, &a.cubic)) return e;
  a.face[0] = params->face;
  { PROF(c, c->s_main, "reproject"); launch_reproject(c->s_main, 1, a); }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(fx_out, a.fx_out, bytes, hipMemcpyDeviceToHost, c->s_main));
  HIPCHK(c, hipMemcpyAsync(fy_out, a.fy_out, bytes, hipMemcpyDeviceToHost, c->s_main));
  return finish(c);
}
