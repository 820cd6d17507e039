// Part of pf_api.hip (one translation unit): the flow visualisers (CPU/OpticalFlow.cpp:147-204) and the panel of buildvisualizations
// (CPU/main.cpp:20-45), kernels in kernels_vis.hip.  Debug output: none of this runs inside pf_stitch_step; pf_stitch_visualize reads
// what the last step left in HBM.

// Enqueue on s_main: zero the parameter block, the grey reduction (want_grey) and the arrows' LineAA set-up (want_arrows).
static int vis_prepare(pf_ctx* c, const float* d_flow, int cols, int rows, bool want_grey, bool want_arrows, VisParams** par, void** arrows) {
  *par = (VisParams*)ensure(c, "vis_params", sizeof(VisParams));
  float* part = (float*)ensure(c, "vis_part", vis_part_bytes());
  *arrows = ensure(c, "vis_arrows", vis_arrow_bytes(cols, rows));
  if (!*par || !part || !*arrows) return PF_ERR_NOMEM;
  hipStream_t sm = c->s_main;
  HIPCHK(c, hipMemsetAsync(*par, 0, sizeof(VisParams), sm));
  if (want_grey) { PROF(c, sm, "vis_reduce"); launch_vis_reduce(sm, d_flow, cols, rows, part, *par); }
  if (want_arrows) { PROF(c, sm, "vis_arrows"); launch_vis_arrows(sm, d_flow, cols, rows, *arrows); }
  return 0;
}

// Drain the streams and refuse a flow with non-finite components (the reference's result there rests on OpenCV's SIMD min/max and
// on undefined float -> uchar conversions)
static int vis_finish(pf_ctx* c, const VisParams* d_par) {
  VisParams h;
  HIPCHK(c, hipMemcpyAsync(&h, d_par, sizeof h, hipMemcpyDeviceToHost, c->s_main));
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  if (h.nonfinite) return fail(c, PF_ERR_ARG, "flow has %d non-finite components (the visualisers are defined for finite flows only)", h.nonfinite);
  return 0;
}

static int vis_check_args(pf_ctx* c, const void* flow, size_t fstep, int cols, int rows, const void* out, size_t ostep, size_t out_row_bytes) {
  if (!flow || !out) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (fstep < size_t(cols) * 8 || ostep < out_row_bytes) return fail(c, PF_ERR_ARG, "row step too small");
  return 0;
}

// Panel of one direction from device-resident packed flow + image into the packed "vis_out" buffer or d_out
static int vis_panel_dev(pf_ctx* c, const float* d_flow, const uint8_t* d_img, int cols, int rows, uint8_t* d_out) {
  VisParams* par; void* arrows;
  if (int e = vis_prepare(c, d_flow, cols, rows, true, true, &par, &arrows)) return e;
  { PROF(c, c->s_main, "vis_panel"); launch_vis_panel(c->s_main, d_flow, d_img, cols, rows, par, arrows, d_out); }
  return vis_finish(c, par);
}

int pf_vis_grey_disparity(pf_ctx* c, const float* flow, size_t fstep, int cols, int rows, uint8_t* out, size_t ostep) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (int e = vis_check_args(c, flow, fstep, cols, rows, out, ostep, size_t(cols))) return e;
  const size_t n = size_t(cols) * rows;
  float* df = (float*)ensure(c, "vis_flow", n * 8); uint8_t* dout = (uint8_t*)ensure(c, "vis_out", n);
  if (!df || !dout) return PF_ERR_NOMEM;
  if (int e = up_plane(c, df, flow, fstep, cols, rows, 8)) return e;
  VisParams* par; void* arrows;
  if (int e = vis_prepare(c, df, cols, rows, true, false, &par, &arrows)) return e;
  { PROF(c, c->s_main, "vis_grey"); launch_vis_grey(c->s_main, df, cols, rows, par, dout); }
  if (int e = vis_finish(c, par)) return e;
  if (int e = down_plane(c, out, ostep, dout, cols, rows, 1)) return e;
  return finish(c);
}

int pf_vis_color_wheel(pf_ctx* c, const float* flow, size_t fstep, int cols, int rows, uint8_t* out, size_t ostep) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (int e = vis_check_args(c, flow, fstep, cols, rows, out, ostep, size_t(cols) * 3)) return e;
  const size_t n = size_t(cols) * rows;
  float* df = (float*)ensure(c, "vis_flow", n * 8); uint8_t* dout = (uint8_t*)ensure(c, "vis_out", n * 3);
  VisParams* par = (VisParams*)ensure(c, "vis_params", sizeof(VisParams));
  if (!df || !dout || !par) return PF_ERR_NOMEM;
  if (int e = up_plane(c, df, flow, fstep, cols, rows, 8)) return e;
  HIPCHK(c, hipMemsetAsync(par, 0, sizeof(VisParams), c->s_main));
  { PROF(c, c->s_main, "vis_wheel"); launch_vis_wheel(c->s_main, df, cols, rows, par, dout); }   // counts non-finite components itself
  if (int e = vis_finish(c, par)) return e;
  if (int e = down_plane(c, out, ostep, dout, cols, rows, 3)) return e;
  return finish(c);
}

int pf_vis_vector_field(pf_ctx* c, const float* flow, size_t fstep, const uint8_t* img, size_t istep, int cols, int rows, uint8_t* out, size_t ostep) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!img) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = vis_check_args(c, flow, fstep, cols, rows, out, ostep, size_t(cols) * 4)) return e;
  if (istep < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  float* df = (float*)ensure(c, "vis_flow", n * 8); uint8_t* di = (uint8_t*)ensure(c, "vis_img", n * 4); uint8_t* dout = (uint8_t*)ensure(c, "vis_out", n * 4);
  if (!df || !di || !dout) return PF_ERR_NOMEM;
  if (int e = up_plane(c, df, flow, fstep, cols, rows, 8)) return e;
  if (int e = up_plane(c, di, img, istep, cols, rows, 4)) return e;
  VisParams* par; void* arrows;
  // the reduction only for its count of non-finite components: every entry point refuses such a flow, not just where an arrow reads it
  if (int e = vis_prepare(c, df, cols, rows, true, true, &par, &arrows)) return e;
  { PROF(c, c->s_main, "vis_field"); launch_vis_field(c->s_main, di, cols, rows, arrows, dout); }
  if (int e = vis_finish(c, par)) return e;
  if (int e = down_plane(c, out, ostep, dout, cols, rows, 4)) return e;
  return finish(c);
}

int pf_vis_panel(pf_ctx* c, const float* flow, size_t fstep, const uint8_t* img, size_t istep, int cols, int rows, uint8_t* out, size_t ostep) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!img) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = vis_check_args(c, flow, fstep, cols, rows, out, ostep, size_t(cols) * 12)) return e;
  if (istep < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  float* df = (float*)ensure(c, "vis_flow", n * 8); uint8_t* di = (uint8_t*)ensure(c, "vis_img", n * 4); uint8_t* dout = (uint8_t*)ensure(c, "vis_out", n * 12);
  if (!df || !di || !dout) return PF_ERR_NOMEM;
  if (int e = up_plane(c, df, flow, fstep, cols, rows, 8)) return e;
  if (int e = up_plane(c, di, img, istep, cols, rows, 4)) return e;
  if (int e = vis_panel_dev(c, df, di, cols, rows, dout)) return e;
  if (int e = down_plane(c, out, ostep, dout, cols, rows, 12)) return e;
  return finish(c);
}

int pf_vis_panel_dev(pf_ctx* c, const float* d_flow, const uint8_t* d_img, int cols, int rows, uint8_t* d_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_flow || !d_img || !d_out) return fail(c, PF_ERR_ARG, "null device pointer");
  if (int e = check_image(c, cols, rows)) return e;
  {
    const size_t n = size_t(cols) * rows;
    const DevPlane pl[] = {{d_flow, n * 8, 8, false, "d_flow", -1}, {d_img, n * 4, 4, false, "d_image", -1}, {d_out, n * 12, 4, true, "d_out", -1}};
    if (int e = check_dev_planes(c, "pf_vis_panel_dev", pl, 3)) return e;
  }
  return vis_panel_dev(c, d_flow, d_img, cols, rows, d_out);
}

// The two panels of the last pf_stitch_step from what it left in HBM: L->R over the step's left input, R->L over its right input
// (the images buildvisualizations is handed at the reference's commented-out call site, CPU/main.cpp:85)
int pf_stitch_visualize(pf_ctx* c, uint8_t* l2r_panel, uint8_t* r2l_panel, size_t step) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!c->vis_step_valid) return fail(c, PF_ERR_ARG, "pf_stitch_visualize: no pf_stitch_step result in HBM (none ran, or a later call reused its buffers)");
  const int cols = c->chain_cols, rows = c->chain_rows;
  if (step < size_t(cols) * 12) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  uint8_t* dout = (uint8_t*)ensure(c, "vis_out", n * 12);
  if (!dout) return PF_ERR_NOMEM;
  const char* imgs[2] = {"ch_l", "ch_r"}; const char* flows[2] = {"nv_flow_l2r", "nv_flow_r2l"};
  uint8_t* outs[2] = {l2r_panel, r2l_panel};
  for (int d = 0; d < 2; ++d) {
    if (!outs[d]) continue;
    if (int e = vis_panel_dev(c, (const float*)c->bufs[flows[d]].p, (const uint8_t*)c->bufs[imgs[d]].p, cols, rows, dout)) return e;
    if (int e = down_plane(c, outs[d], step, dout, cols, rows, 12)) return e;
    if (int e = finish(c)) return e;
  }
  return 0;
}
