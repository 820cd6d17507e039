// Part of pf_api.hip (one translation unit, split along its seams in round 5): the stage-level entry points the parity tests call, profiling queries, geometry queries.
// ---- stage-level entry points (tests) ----
#define STAGE_BEGIN(c) if (int e_ = use(c)) return e_; CallGuard guard_(c); hipStream_t sm = c->s_main; (void)sm
static void* stage_up(pf_ctx* c, const char* name, const void* host, size_t bytes) {
  void* d = ensure(c, name, bytes);
  if (d && host) hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, c->s_main);
  return d;
}
static int stage_down(pf_ctx* c, void* host, const void* dev, size_t bytes) {
  HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->s_main));
  HIPCHK(c, hipGetLastError());
  return finish(c);
}

// k_downscale_gray wraps a tap of the virtually padded image [last pad columns | image | first pad columns] back into the image ONCE
// (+- cols): that covers pad <= cols.  The product passes cols / 20; anything else is refused before a launch.
static int check_pad(pf_ctx* c, int cols, int pad) {
  if (pad < 0 || pad > cols) return fail(c, PF_ERR_ARG, "pad %d outside 0..cols (%d): the wrap padding repeats the image at most once per side", pad, cols);
  return 0;
}
int pf_stage_preprocess(pf_ctx* c, const uint8_t* bgra, int cols, int rows, int pad, float* gray_half, float* alpha_half) {
  STAGE_BEGIN(c);
  if (int e = check_pad(c, cols, pad)) return e;
  if (int e = check_dims(c, cols, rows, pad)) return e;
  const int dw = int((cols + 2 * pad) * kDownscaleFactor), dh = int(rows * kDownscaleFactor);
  uint8_t* d = (uint8_t*)stage_up(c, "sg_a", bgra, size_t(cols) * rows * 4);
  float* t = (float*)ensure(c, "sg_b", size_t(dw) * dh * 4); float* g = (float*)ensure(c, "sg_c", size_t(dw) * dh * 4); float* a = (float*)ensure(c, "sg_d", size_t(dw) * dh * 4);
  if (!d || !t || !g || !a) return PF_ERR_NOMEM;
  launch_downscale_gray(sm, d, cols, rows, pad, t, a, dw, dh);
  launch_gauss_small(sm, t, g, dw, dh, 1, c->g5);
  HIPCHK(c, hipMemcpyAsync(gray_half, g, size_t(dw) * dh * 4, hipMemcpyDeviceToHost, sm));
  return stage_down(c, alpha_half, a, size_t(dw) * dh * 4);
}
int pf_stage_pyr_down(pf_ctx* c, const float* src, int sw, int sh, float* dst, int dw, int dh) {
  STAGE_BEGIN(c);
  float* s = (float*)stage_up(c, "sg_a", src, size_t(sw) * sh * 4); float* d = (float*)ensure(c, "sg_b", size_t(dw) * dh * 4);
  if (!s || !d) return PF_ERR_NOMEM;
  launch_pyr_down4(sm, s, nullptr, nullptr, nullptr, sw, sh, d, nullptr, nullptr, nullptr, dw, dh, Batch(), 1);
  return stage_down(c, dst, d, size_t(dw) * dh * 4);
}
int pf_stage_gradients(pf_ctx* c, const float* img, int w, int h, float* gxy) {
  STAGE_BEGIN(c);
  float* s = (float*)stage_up(c, "sg_a", img, size_t(w) * h * 4); float* d = (float*)ensure(c, "sg_b", size_t(w) * h * 8);
  if (!s || !d) return PF_ERR_NOMEM;
  LevelTable t{}; t.n = 1; t.w[0] = w; t.h[0] = h;
  launch_gradients_all(sm, s, nullptr, d, nullptr, t, 0, size_t(w) * h, c->g3_05);
  return stage_down(c, gxy, d, size_t(w) * h * 8);
}
int pf_stage_gauss(pf_ctx* c, const float* src, int w, int h, int cn, int ksize, double sigma, float* dst) {
  STAGE_BEGIN(c);
  if (!((ksize == 3 || ksize == 5) && (cn == 1 || cn == 2)) && !(ksize == 15 && cn == 2)) return fail(c, PF_ERR_ARG, "unsupported gaussian %d/%d", ksize, cn);
  const size_t nb = size_t(w) * h * cn * 4;
  float* s = (float*)stage_up(c, "sg_a", src, nb); float* d = (float*)ensure(c, "sg_b", nb);
  if (!s || !d) return PF_ERR_NOMEM;
  const Gauss g = make_gauss(ksize, sigma);
  if (ksize == 15) launch_gauss15(sm, s, d, w, h, g); else launch_gauss_small(sm, s, d, w, h, cn, g);
  return stage_down(c, dst, d, nb);
}
int pf_stage_median5(pf_ctx* c, const float* flow, int w, int h, float* out) {
  STAGE_BEGIN(c);
  float* s = (float*)stage_up(c, "sg_a", flow, size_t(w) * h * 8); float* d = (float*)ensure(c, "sg_b", size_t(w) * h * 8);
  if (!s || !d) return PF_ERR_NOMEM;
  // the stage entry runs BOTH forms of the kernel (direct and LDS-tiled; the solver picks by level size) and requires identical bits
  float* d2 = (float*)ensure(c, "sg_c", size_t(w) * h * 8); int* neq = (int*)ensure(c, "sg_d", 256);
  if (!d2 || !neq) return PF_ERR_NOMEM;
  launch_median5_form(sm, s, d, w, h, false);
  launch_median5_form(sm, s, d2, w, h, true);
  HIPCHK(c, hipMemsetAsync(neq, 0, 4, sm));
  launch_count_diff_u32(sm, reinterpret_cast<const uint32_t*>(d), reinterpret_cast<const uint32_t*>(d2), size_t(w) * h * 2, neq);
  int hneq = 0;
  HIPCHK(c, hipMemcpyAsync(&hneq, neq, 4, hipMemcpyDeviceToHost, sm));
  if (int e = stage_down(c, out, d, size_t(w) * h * 8)) return e;
  if (hneq) return fail(c, PF_ERR_DEVICE, "median5: the direct and the LDS-tiled kernel disagree in %d words", hneq);
  return 0;
}
int pf_stage_sweep(pf_ctx* c, const float* g0, const float* g1, const float* blurred, const float* a0, const float* a1, float* flow, int w, int h, int forward) {
  STAGE_BEGIN(c);
  const size_t n = size_t(w) * h;
  float* dg0 = (float*)stage_up(c, "sg_a", g0, n * 8); float* dg1 = (float*)stage_up(c, "sg_b", g1, n * 8); float* dbl = (float*)stage_up(c, "sg_c", blurred, n * 8);
  float* da0 = (float*)stage_up(c, "sg_d", a0, n * 4); float* da1 = (float*)stage_up(c, "sg_e", a1, n * 4); float* df = (float*)stage_up(c, "sg_f", flow, n * 8);
  uint8_t* gate = (uint8_t*)ensure(c, "sg_g", n);
  const size_t nb = sweep_boundary_elems(w, h);
  unsigned long long* bnd = (unsigned long long*)ensure(c, "sg_h", nb * 8); int* ctrl = (int*)ensure(c, "sg_i", 16);
  if (!dg0 || !dg1 || !dbl || !da0 || !da1 || !df || !gate || !bnd || !ctrl) return PF_ERR_NOMEM;
  launch_fill_u64(sm, bnd, nb, kNotReady);
  HIPCHK(c, hipMemsetAsync(ctrl, 0, 16, sm));
  SweepArgs sa; sa.cf = c->cf; sa.g0 = (const float2*)dg0; sa.g1 = (const float2*)dg1; sa.blurred = (const float2*)dbl; sa.gate = gate; sa.flow = (float2*)df;
  sa.boundary = bnd; sa.ctrl = ctrl; sa.W = w; sa.H = h; sa.forward = forward; sa.sparse = (w * h) % 2;   // stage test: exercise both variants
  sa.wide = c->cfg.sweep_wide > 0 ? c->cfg.sweep_wide : 0;   // the sweep form the context was created for (auto = latency form: one pair)
  if (sa.wide == 2) sa.sparse = 0;            // (the throughput form has no sparse variant)
  {
    int box[4];
    if (int e = gate_level(c, sm, da0, da1, gate, w, h, box, nullptr)) return e;
    sa.ax0 = box[0]; sa.ay0 = box[1]; sa.ax1 = box[2] + 1; sa.ay1 = box[3] + 1;
  }
  float* rec = (float*)ensure(c, "sg_rec", sweep2_rec_bytes(w, h));
  if (!rec) return PF_ERR_NOMEM;
#ifdef PF_EXPERIMENTS
  if (c->cfg.sweep_impl == 1) { PROF(c, sm, "sweep"); launch_sweep(sm, sa); } else
#endif
  { PROF(c, sm, "sweep"); (void)launch_sweep2(sm, sa, rec); }
  int hc[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(hc, ctrl, 16, hipMemcpyDeviceToHost, sm));
  if (int e = stage_down(c, flow, df, n * 8)) return e;
  if (hc[1]) return fail(c, PF_ERR_TIMEOUT, "sweep band timed out");
#ifdef PF_SWEEP_STATS_PRINT
  fprintf(stderr, "[panoflow] sweep %dx%d: edge waits %d, spin iterations %d\n", w, h, hc[2], hc[3]);
#endif
  return 0;
}
int pf_stage_diffusion(pf_ctx* c, const float* a0, const float* a1, float* flow, int w, int h) {
  STAGE_BEGIN(c);
  const size_t n = size_t(w) * h;
  float* da0 = (float*)stage_up(c, "sg_a", a0, n * 4); float* da1 = (float*)stage_up(c, "sg_b", a1, n * 4); float* df = (float*)stage_up(c, "sg_c", flow, n * 8);
  float* o = (float*)ensure(c, "sg_d", n * 8);
  if (!da0 || !da1 || !df || !o) return PF_ERR_NOMEM;
  launch_gauss15_mix(sm, df, da0, da1, w, h, c->g15, o);
  return stage_down(c, flow, o, n * 8);
}
int pf_stage_upsample_cubic(pf_ctx* c, const float* flow, int sw, int sh, float* out, int dw, int dh, float scale) {
  STAGE_BEGIN(c);
  if (sw < 1 || sh < 1 || dw < 1 || dh < 1) return fail(c, PF_ERR_ARG, "bad upsample size %dx%d -> %dx%d", sw, sh, dw, dh);
  if (!upsample_cubic_fits(sh, dh)) return fail(c, PF_ERR_ARG, "upsample %d -> %d rows: the kernel covers source / destination rows <= 1.1875 (a pyramid never shrinks on the way up)", sh, dh);
  float* s = (float*)stage_up(c, "sg_a", flow, size_t(sw) * sh * 8); float* d = (float*)ensure(c, "sg_b", size_t(dw) * dh * 8);
  if (!s || !d) return PF_ERR_NOMEM;
  launch_upsample_cubic(sm, s, sw, sh, d, dw, dh, scale);
  return stage_down(c, out, d, size_t(dw) * dh * 8);
}
int pf_stage_final(pf_ctx* c, const float* flow, int sw, int sh, int pad_cols, int rows, int pad, float scale, float* out) {
  STAGE_BEGIN(c);
  const int cols = pad_cols - 2 * pad;
  float* s = (float*)stage_up(c, "sg_a", flow, size_t(sw) * sh * 8); float* d = (float*)ensure(c, "sg_b", size_t(cols) * rows * 8);
  if (!s || !d) return PF_ERR_NOMEM;
  launch_final_flow(sm, s, sw, sh, pad_cols, rows, pad, scale, c->g3_1, d);
  return stage_down(c, out, d, size_t(cols) * rows * 8);
}
int pf_stage_adjust_initial_flow(pf_ctx* c, const float* i0, const float* i1, const float* a0, const float* a1, int w, int h, int hint, int max_pct, float* flow_out) {
  STAGE_BEGIN(c);
  const size_t n = size_t(w) * h;
  float* d0 = (float*)stage_up(c, "sg_a", i0, n * 4); float* d1 = (float*)stage_up(c, "sg_b", i1, n * 4); float* da0 = (float*)stage_up(c, "sg_c", a0, n * 4);
  float* da1 = (float*)stage_up(c, "sg_d", a1, n * 4); float* df = (float*)ensure(c, "sg_e", n * 8); float* rt = (float*)ensure(c, "sg_f", 256);
  if (!d0 || !d1 || !da0 || !da1 || !df || !rt) return PF_ERR_NOMEM;
  HIPCHK(c, hipMemsetAsync(df, 0, n * 8, sm));
  if (max_pct > 0) launch_adjust_initial_flow(sm, d0, d1, da0, da1, w, h, hint, max_pct, rt, df);
  return stage_down(c, flow_out, df, n * 8);
}
int pf_stage_level(pf_ctx* c, const float* i0, const float* i1, const float* a0, const float* a1, int w, int h, const float* flow_in, int hint, int max_pct,
                   float* flow_out) {
  STAGE_BEGIN(c);
  const size_t n = size_t(w) * h;
  float* d0 = (float*)stage_up(c, "sg_a", i0, n * 4); float* d1 = (float*)stage_up(c, "sg_b", i1, n * 4); float* da0 = (float*)stage_up(c, "sg_c", a0, n * 4);
  float* da1 = (float*)stage_up(c, "sg_d", a1, n * 4);
  float* g0 = (float*)ensure(c, "sg_e", n * 8); float* g1 = (float*)ensure(c, "sg_f", n * 8); uint8_t* gate = (uint8_t*)ensure(c, "sg_g", n);
  LevelBufs b; b.rec = (float*)ensure(c, "sg_rec", sweep2_rec_bytes(w, h)); if (!b.rec) return PF_ERR_NOMEM;
  b.flow_a = (float*)ensure(c, "sg_h", n * 8); b.flow_b = (float*)ensure(c, "sg_i", n * 8); b.blurred = (float*)ensure(c, "sg_j", n * 8); b.tmp = (float*)ensure(c, "sg_k", n * 8);
  const size_t nb = sweep_boundary_elems(w, h);
  unsigned long long* bnd = (unsigned long long*)ensure(c, "sg_l", nb * 16); int* ctrl = (int*)ensure(c, "sg_m", 16); float* rt = (float*)ensure(c, "sg_n", 256);
  if (!d0 || !d1 || !da0 || !da1 || !g0 || !g1 || !gate || !b.flow_a || !b.flow_b || !b.blurred || !b.tmp || !bnd || !ctrl || !rt) return PF_ERR_NOMEM;
  { LevelTable t{}; t.n = 1; t.w[0] = w; t.h[0] = h; launch_gradients_all(sm, d0, d1, g0, g1, t, 0, n, c->g3_05); }
  launch_fill_u64(sm, bnd, nb * 2, kNotReady);
  HIPCHK(c, hipMemsetAsync(ctrl, 0, 16, sm));
  if (flow_in) HIPCHK(c, hipMemcpyAsync(b.flow_a, flow_in, n * 8, hipMemcpyHostToDevice, sm));
  else {
    HIPCHK(c, hipMemsetAsync(b.flow_a, 0, n * 8, sm));
    if (max_pct > 0 && hint != PF_HINT_UNKNOWN) launch_adjust_initial_flow(sm, d0, d1, da0, da1, w, h, hint, max_pct, rt, b.flow_a);
  }
  float* res = nullptr;
  int box[4];
  if (int e = gate_level(c, sm, da0, da1, gate, w, h, box, nullptr)) return e;
  run_level(c, sm, g0, g1, da0, da1, gate, w, h, (w + h) % 2, box, b, bnd, bnd + nb, ctrl, ctrl + 2, &res);
  int hc[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(hc, ctrl, 16, hipMemcpyDeviceToHost, sm));
  if (int e = stage_down(c, flow_out, res, n * 8)) return e;
  if (hc[1] || hc[3]) return fail(c, PF_ERR_TIMEOUT, "sweep band timed out");
  return 0;
}
int pf_stage_blend_smooth(pf_ctx* c, float* blend, const float* md, int cols, int rows) {
  STAGE_BEGIN(c);
  const size_t n = size_t(cols) * rows;
  float* db = (float*)stage_up(c, "st_blend", blend, n * 4); float* dmd = (float*)stage_up(c, "st_md", md, n * 4);
  if (!db || !dmd) return PF_ERR_NOMEM;
  const RampGeom g = ramp_geom(cols, rows);
  StitchPtrs p{}; p.blend[0] = db; p.md[0] = dmd;
  RampWork w;
  if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w)) return e;
  const float* ramp = nullptr;
  if (int e = blend_ramp_dev(c, sm, p, 1, cols, rows, g, w, false, &ramp)) return e;
  if (int e = stage_down(c, blend, ramp, n * 4)) return e;
  return check_sweeps(c);
}
// The tile pass of the ramp smoothing alone (StitchTool.cpp:134-141, without the final rows/400 blur) with the geometry given
// explicitly: the kernel the stitch entry points use, on images small enough to check against the reference.
// form: -1 = the library's choice, 0 = resident, 1 = streamed.
int pf_stage_tile_blur(pf_ctx* c, float* blend, const float* md, int cols, int rows, int step, int k, int form) {
  STAGE_BEGIN(c);
  if (!blend || !md) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (step < 1 || k < 1 || form < -1 || form > 1) return fail(c, PF_ERR_ARG, "bad step / k / form");
  if (step >= (cols < rows ? cols : rows)) return fail(c, PF_ERR_ARG, "step %d leaves no tile on a %dx%d canvas", step, cols, rows);
  if (!tile_reach_ok(cols, rows, k)) return fail(c, PF_ERR_ARG, "window %d reaches across the whole %dx%d canvas", k, cols, rows);
  const bool fits = tile_blur_resident_fits(step, k);
  if (form == 0 && !fits) return fail(c, PF_ERR_ARG, "step %d, k %d: the resident form needs %zu bytes of LDS", step, k, tile_blur_lds_bytes(step, k));
  const bool streamed = form < 0 ? !fits : form == 1;
  if (streamed && !tile_blur_stream_ok(step, k)) return fail(c, PF_ERR_ARG, "step %d, k %d: one window row exceeds the streamed form's LDS piece", step, k);
  const size_t n = size_t(cols) * rows;
  float* db = (float*)stage_up(c, "st_blend", blend, n * 4); float* dmd = (float*)stage_up(c, "st_md", md, n * 4);
  if (!db || !dmd) return PF_ERR_NOMEM;
  if (int e = tile_blur_dev(c, sm, db, dmd, cols, rows, step, k, streamed)) return e;
  if (int e = stage_down(c, blend, db, n * 4)) return e;
  return check_sweeps(c);
}
// The rows/400 box blur of the ramp smoothing alone (StitchTool.cpp:142-143) with the kernel width given explicitly, through the
// launcher blend_ramp_dev uses (tests/test_gpu_stitch_forms.py).  n_batch frames as a batched stitch step lays them out: the ramps as
// stitch_group's, the fp64 row sums and the result planes as ramp_planes', all 256-byte-aligned frame strides.  The three areas are
// filled with 0xFF bytes before the ramps go in: whatever a kernel reads outside a plane is a NaN.
int pf_stage_box_blur(pf_ctx* c, int n_batch, const float* src, int cols, int rows, int k, float* dst) {
  STAGE_BEGIN(c);
  if (!src || !dst) return fail(c, PF_ERR_ARG, "null pointer");
  if (n_batch < 1 || n_batch > 3 || k < 1) return fail(c, PF_ERR_ARG, "n_batch %d (1..3) / k %d (>= 1)", n_batch, k);
  if (int e = check_image(c, cols, rows)) return e;
  const size_t n = size_t(cols) * rows;
  RampGeom g; g.k2 = k;   // no tile pass: ramp_planes sets up the box blur's planes only
  StitchPtrs p{};
  RampWork w;
  if (int e = ramp_planes(c, kRampBatch, n_batch, cols, rows, g, p, w)) return e;
  size_t s4;
  float* blend = frame_planes<float>(c, "sb_blend", n_batch, n * 4, s4);
  if (!blend) return PF_ERR_NOMEM;
  const size_t s8 = (n * 8 + 255) & ~size_t(255);   // frame_planes' strides of p.rs (p.tmp: s4)
  HIPCHK(c, hipMemsetAsync(blend, 0xFF, s4 * n_batch, sm));
  HIPCHK(c, hipMemsetAsync(p.rs[0], 0xFF, s8 * n_batch, sm));
  HIPCHK(c, hipMemsetAsync(p.tmp[0], 0xFF, s4 * n_batch, sm));
  for (int f = 0; f < n_batch; ++f) {
    p.blend[f] = (float*)((char*)blend + f * s4);
    HIPCHK(c, hipMemcpyAsync(p.blend[f], src + size_t(f) * n, n * 4, hipMemcpyHostToDevice, sm));
  }
  { PROF(c, sm, "box_blur"); launch_box_blur(sm, p, n_batch, cols, rows, k); }
  HIPCHK(c, hipGetLastError());
  for (int f = 0; f < n_batch; ++f) HIPCHK(c, hipMemcpyAsync(dst + size_t(f) * n, p.tmp[f], n * 4, hipMemcpyDeviceToHost, sm));
  return finish(c);
}

// ---- every form of the fused Gaussian 15 and a whole level table (tests/test_gpu_stage_forms.py) ----
// Slabs as a batched solve lays them out: one per pair, `stride` bytes apart, every plane at the same 256-byte-aligned offset inside.
struct StageSlab {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~size_t(255); return o; }
  size_t stride() const { return (off + 4095) & ~size_t(4095); }
};
int pf_stage_gauss15_form(pf_ctx* c, int form, int n_batch, int max_blocks, const float* src, int sw, int sh, float mul, const float* a0, const float* a1, int w, int h,
                          float* dst, float* up_out) {
  STAGE_BEGIN(c);
  if (form < PF_G15_PLAIN || form > PF_G15_MEDIAN_MIX) return fail(c, PF_ERR_ARG, "gauss15 form %d (0..3)", form);
  if (n_batch < 1 || n_batch > 3 || max_blocks < 0) return fail(c, PF_ERR_ARG, "n_batch %d (1..3) / max_blocks %d (>= 0)", n_batch, max_blocks);
  if (int e = check_image(c, w, h)) return e;
  const bool ups = form == PF_G15_UPSAMPLE, mix = form == PF_G15_MIX || form == PF_G15_MEDIAN_MIX;
  if (!src || !dst || (mix && (!a0 || !a1)) || (ups && !up_out)) return fail(c, PF_ERR_ARG, "null pointer");
  if (ups) { if (int e = check_image(c, sw, sh)) return e; } else { sw = w; sh = h; }
  const size_t n = size_t(w) * h, ns = size_t(sw) * sh;
  StageSlab L;
  const size_t oS = L.take(ns * 8), oA0 = L.take(n * 4), oA1 = L.take(n * 4), oD = L.take(n * 8), oU = L.take(n * 8);
  const size_t stride = L.stride();
  char* base = (char*)ensure(c, "sg_g15", stride * size_t(n_batch));
  if (!base) return PF_ERR_NOMEM;
  HIPCHK(c, hipMemsetAsync(base, 0xFF, stride * size_t(n_batch), sm));   // whatever a kernel reads outside its planes is a NaN
  for (int p = 0; p < n_batch; ++p) {
    char* sl = base + size_t(p) * stride;
    HIPCHK(c, hipMemcpyAsync(sl + oS, src + size_t(p) * ns * 2, ns * 8, hipMemcpyHostToDevice, sm));
    if (mix) {
      HIPCHK(c, hipMemcpyAsync(sl + oA0, a0 + size_t(p) * n, n * 4, hipMemcpyHostToDevice, sm));
      HIPCHK(c, hipMemcpyAsync(sl + oA1, a1 + size_t(p) * n, n * 4, hipMemcpyHostToDevice, sm));
    }
  }
  Batch bt; bt.n = n_batch; bt.stride = n_batch > 1 ? stride : 0;
  float* dS = (float*)(base + oS); float* dA0 = (float*)(base + oA0); float* dA1 = (float*)(base + oA1); float* dD = (float*)(base + oD); float* dU = (float*)(base + oU);
  switch (form) {
    case PF_G15_PLAIN: launch_gauss15(sm, dS, dD, w, h, c->g15, bt, max_blocks); break;
    case PF_G15_MIX: launch_gauss15_mix(sm, dS, dA0, dA1, w, h, c->g15, dD, bt, max_blocks); break;
    case PF_G15_UPSAMPLE: launch_gauss15_upsample(sm, dS, sw, sh, mul, dU, dD, w, h, c->g15, bt, max_blocks); break;
    default: launch_median_gauss15_mix(sm, dS, dA0, dA1, w, h, c->g15, dD, bt, max_blocks); break;
  }
  HIPCHK(c, hipGetLastError());
  for (int p = 0; p < n_batch; ++p) {
    const char* sl = base + size_t(p) * stride;
    HIPCHK(c, hipMemcpyAsync(dst + size_t(p) * n * 2, sl + oD, n * 8, hipMemcpyDeviceToHost, sm));
    if (ups) HIPCHK(c, hipMemcpyAsync(up_out + size_t(p) * n * 2, sl + oU, n * 8, hipMemcpyDeviceToHost, sm));
  }
  return finish(c);
}
// Host planes are packed (levels back to back, no padding); the device planes are a solve's pyramid planes: level l at off[l], offsets
// rounded up to 64 elements (make_geometry).  Device planes are filled with 0xFF bytes before the inputs go in, and gradients / gate come
// back as whole padded planes: what the kernels did not write still reads 0xFF.
int pf_stage_level_table(pf_ctx* c, int n_levels, const int* ws, const int* hs, int n_batch, const float* img0, const float* img1, const float* a0, const float* a1,
                         long long first, long long total, int max_blocks, long long* off_out, float* g0, float* g1, uint8_t* gate, int* boxes, int* count0) {
  STAGE_BEGIN(c);
  if (n_levels < 1 || n_levels > kLevelTableMax || !ws || !hs) return fail(c, PF_ERR_ARG, "%d levels (1..%d)", n_levels, kLevelTableMax);
  if (n_batch < 1 || n_batch > 3 || max_blocks < 0) return fail(c, PF_ERR_ARG, "n_batch %d (1..3) / max_blocks %d (>= 0)", n_batch, max_blocks);
  if (!img0 || !img1 || !a0 || !a1 || !off_out || !g0 || !g1 || !gate || !boxes || !count0) return fail(c, PF_ERR_ARG, "null pointer");
  LevelTable t{}; t.n = n_levels;
  size_t P = 0, Pexact = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (ws[l] < 2 || hs[l] < 2) return fail(c, PF_ERR_ARG, "level %d is %dx%d (at least 2x2)", l, ws[l], hs[l]);
    const size_t px = size_t(ws[l]) * hs[l];
    if (P + px >= (size_t(1) << 31)) return fail(c, PF_ERR_ARG, "level table too large");
    t.w[l] = ws[l]; t.h[l] = hs[l]; t.off[l] = (unsigned)P; off_out[l] = (long long)P;
    Pexact += px; P += (px + 63) & ~size_t(63);
  }
  off_out[n_levels] = (long long)P;
  if (total == 0) total = (long long)P;
  if (first < 0 || first % 4 || total % 4 || first > total || total > (long long)P) return fail(c, PF_ERR_ARG, "gradient range [%lld, %lld) of %zu elements (multiples of 4)", first, total, P);
  StageSlab L;
  const size_t oW = L.take(kGateWords * sizeof(int));   // first: the one area the fill below leaves alone (self-resetting, initialised once per layout)
  const size_t oI0 = L.take(P * 4), oI1 = L.take(P * 4), oA0 = L.take(P * 4), oA1 = L.take(P * 4), oG0 = L.take(P * 8), oG1 = L.take(P * 8), oGate = L.take(P);
  const size_t stride = L.stride();
  char* base = (char*)ensure(c, "sg_tbl", stride * size_t(n_batch));
  if (!base) return PF_ERR_NOMEM;
  int* work = nullptr;
  if (n_batch == 1) work = gate_work(c);   // a lone solve's area
  else {
    work = (int*)(base + oW);
    if (c->tbl_slab != base || c->tbl_stride != stride || c->tbl_pairs < n_batch) {
      const std::vector<int> init = gate_work_init();
      for (int p = 0; p < n_batch; ++p) HIPCHK(c, hipMemcpy(base + size_t(p) * stride + oW, init.data(), init.size() * sizeof(int), hipMemcpyHostToDevice));
      c->tbl_slab = base; c->tbl_stride = stride; c->tbl_pairs = n_batch;
    }
  }
  if (!work) return PF_ERR_NOMEM;
  for (int p = 0; p < n_batch; ++p) {
    char* sl = base + size_t(p) * stride;
    HIPCHK(c, hipMemsetAsync(sl + oI0, 0xFF, stride - oI0, sm));
    const float* hsrc[4] = {img0, img1, a0, a1}; const size_t ooff[4] = {oI0, oI1, oA0, oA1};
    for (int k = 0; k < 4; ++k) {
      size_t e = 0;
      for (int l = 0; l < n_levels; ++l) {
        const size_t px = size_t(ws[l]) * hs[l];
        HIPCHK(c, hipMemcpyAsync(sl + ooff[k] + size_t(t.off[l]) * 4, hsrc[k] + size_t(p) * Pexact + e, px * 4, hipMemcpyHostToDevice, sm));
        e += px;
      }
    }
  }
  Batch bt; bt.n = n_batch; bt.stride = n_batch > 1 ? stride : 0;
  launch_gradients_all(sm, (const float*)(base + oI0), (const float*)(base + oI1), (float*)(base + oG0), (float*)(base + oG1), t, size_t(first), size_t(total), c->g3_05, max_blocks, bt);
  const int epoch = ++c->gate_epoch;
  launch_gate_bbox_all(sm, (const float*)(base + oA0), (const float*)(base + oA1), (uint8_t*)(base + oGate), t, P, work, c->d_gate, epoch, bt, kGateWords * sizeof(int));
  HIPCHK(c, hipGetLastError());
  for (int p = 0; p < n_batch; ++p) {
    unsigned cnt = 0;
    if (int e = wait_gate_boxes(c, sm, epoch, n_levels, boxes + size_t(p) * n_levels * 4, cnt, p)) return e;
    count0[p] = (int)cnt;
    const char* sl = base + size_t(p) * stride;
    HIPCHK(c, hipMemcpyAsync(g0 + size_t(p) * P * 2, sl + oG0, P * 8, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipMemcpyAsync(g1 + size_t(p) * P * 2, sl + oG1, P * 8, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipMemcpyAsync(gate + size_t(p) * P, sl + oGate, P, hipMemcpyDeviceToHost, sm));
  }
  return finish(c);
}


// ---- the head of the pipeline in the forms a solve runs (tests/test_gpu_front_forms.py) ----
// As above: slabs laid out as a batched solve lays them, filled with 0xFF bytes before the inputs go in, outputs returned as whole planes
// up to their 256-byte padding, so that a write outside its place shows.  n_batch = 1 runs the lone form (stride 0), as solve_n does.
static int check_batch3(pf_ctx* c, int n_batch) {
  if (n_batch < 1 || n_batch > 3) return fail(c, PF_ERR_ARG, "n_batch %d (1..3)", n_batch);
  return 0;
}
int pf_stage_preprocess_batch(pf_ctx* c, int n_batch, const uint8_t* bgra, int cols, int rows, int pad, float* gray_half, float* alpha_half) {
  STAGE_BEGIN(c);
  if (int e = check_batch3(c, n_batch)) return e;
  if (!bgra || !gray_half || !alpha_half) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_pad(c, cols, pad)) return e;
  if (int e = check_dims(c, cols, rows, pad)) return e;
  const Geometry g = make_geometry(cols, rows, pad);
  const size_t npad = (size_t(g.w0) * g.h0 + 63) & ~size_t(63), nimg = size_t(cols) * rows * 4;
  StageSlab L;
  const size_t oT = L.take(npad * 4), oG = L.take(npad * 4), oA = L.take(npad * 4);
  const size_t stride = L.stride();
  char* base = (char*)ensure(c, "sg_pre", stride * size_t(n_batch));
  if (!base) return PF_ERR_NOMEM;
  static const char* const names[3] = {"sg_img0", "sg_img1", "sg_img2"};   // one caller-style buffer per pair
  ExtPtrs imgs{};
  for (int p = 0; p < n_batch; ++p) {
    void* d = stage_up(c, names[p], bgra + size_t(p) * nimg, nimg);
    if (!d) return PF_ERR_NOMEM;
    imgs.p[p] = d;
  }
  HIPCHK(c, hipMemsetAsync(base, 0xFF, stride * size_t(n_batch), sm));
  Batch bt; bt.n = n_batch; bt.stride = n_batch > 1 ? stride : 0;
  float* half_tmp = (float*)(base + oT); float* gray = (float*)(base + oG); float* alpha = (float*)(base + oA);
  launch_downscale_gray(sm, nullptr, cols, rows, pad, half_tmp, alpha, g.w0, g.h0, bt, &imgs);   // as solve_n
  launch_gauss_small(sm, half_tmp, gray, g.w0, g.h0, 1, c->g5, bt);
  HIPCHK(c, hipGetLastError());
  for (int p = 0; p < n_batch; ++p) {
    const char* sl = base + size_t(p) * stride;
    HIPCHK(c, hipMemcpyAsync(gray_half + size_t(p) * npad, sl + oG, npad * 4, hipMemcpyDeviceToHost, sm));
    HIPCHK(c, hipMemcpyAsync(alpha_half + size_t(p) * npad, sl + oA, npad * 4, hipMemcpyDeviceToHost, sm));
  }
  return finish(c);
}
int pf_stage_pyramid(pf_ctx* c, int n_batch, int mode, const float* level0, int w0, int h0, int cap_levels, long long cap_plane, int* n_levels, int* ws, int* hs,
                     long long* off, int* ks, int* n_launches, float* planes) {
  STAGE_BEGIN(c);
  if (int e = check_batch3(c, n_batch)) return e;
  if (mode < 0 || mode > 3) return fail(c, PF_ERR_ARG, "chaining mode %d (0..3)", mode);
  if (!level0 || !n_levels || !ws || !hs || !off || !ks || !n_launches || !planes) return fail(c, PF_ERR_ARG, "null pointer");
  if (w0 < 2 || h0 < 2) return fail(c, PF_ERR_ARG, "level 0 is %dx%d (at least 2x2)", w0, h0);
  if ((double)w0 * h0 > 5.0e8) return fail(c, PF_ERR_ARG, "level 0 too large");
  const Geometry g = make_geometry_level0(w0, h0);
  if (g.n > cap_levels || (long long)g.P > cap_plane) return fail(c, PF_ERR_ARG, "%d levels, planes of %zu elements: the caller's arrays hold %d and %lld", g.n, g.P, cap_levels, cap_plane);
  StageSlab L;
  size_t o[4];
  for (int k = 0; k < 4; ++k) o[k] = L.take(g.P * 4);   // I0, I1, A0, A1
  const size_t stride = L.stride(), n0 = size_t(w0) * h0;
  char* base = (char*)ensure(c, "sg_pyr", stride * size_t(n_batch));
  if (!base) return PF_ERR_NOMEM;
  HIPCHK(c, hipMemsetAsync(base, 0xFF, stride * size_t(n_batch), sm));
  for (int p = 0; p < n_batch; ++p)
    for (int k = 0; k < 4; ++k) HIPCHK(c, hipMemcpyAsync(base + size_t(p) * stride + o[k], level0 + (size_t(p) * 4 + k) * n0, n0 * 4, hipMemcpyHostToDevice, sm));
  Batch bt; bt.n = n_batch; bt.stride = n_batch > 1 ? stride : 0;
  float* pyrI[2] = {(float*)(base + o[0]), (float*)(base + o[1])}; float* pyrA[2] = {(float*)(base + o[2]), (float*)(base + o[3])};
  std::vector<int> launched;
  launch_pyramids(c, sm, pyrI, pyrA, g, mode, bt, &launched);
  HIPCHK(c, hipGetLastError());
  *n_levels = g.n; *n_launches = (int)launched.size();
  for (int l = 0; l < g.n; ++l) { ws[l] = g.ws[l]; hs[l] = g.hs[l]; off[l] = (long long)g.off[l]; }
  off[g.n] = (long long)g.P;
  std::copy(launched.begin(), launched.end(), ks);   // at most g.n - 1
  for (int p = 0; p < n_batch; ++p)
    for (int k = 0; k < 4; ++k) HIPCHK(c, hipMemcpyAsync(planes + (size_t(p) * 4 + k) * g.P, base + size_t(p) * stride + o[k], g.P * 4, hipMemcpyDeviceToHost, sm));
  return finish(c);
}
// The slabs of the search entries: per pair the four planes of one level (I0, I1, A0, A1), the flow plane (flow_bytes, may be 0) and the ratio
// scratch (SolveBufs::ratio).  up() lays them out, fills everything with 0xFF bytes -- the ratio scratch too: a NaN where it is read before it
// is written -- and copies the inputs in.
struct SearchSlabs {
  char* base = nullptr; size_t stride = 0, o[4] = {0, 0, 0, 0}, oFlow = 0, oRatio = 0;
  Batch bt;
  const float* plane(int k) const { return (const float*)(base + o[k]); }
  float* flow() const { return (float*)(base + oFlow); }
  float* ratio() const { return (float*)(base + oRatio); }
  int up(pf_ctx* c, hipStream_t sm, int n_batch, const float* const src[4], size_t n, size_t flow_bytes) {
    StageSlab L;
    const size_t npad = (n + 63) & ~size_t(63);
    for (int k = 0; k < 4; ++k) o[k] = L.take(npad * 4);
    oFlow = flow_bytes ? L.take(flow_bytes) : 0;
    oRatio = L.take(256);
    stride = L.stride();
    base = (char*)ensure(c, "sg_search", stride * size_t(n_batch));
    if (!base) return PF_ERR_NOMEM;
    HIPCHK(c, hipMemsetAsync(base, 0xFF, stride * size_t(n_batch), sm));
    for (int p = 0; p < n_batch; ++p)
      for (int k = 0; k < 4; ++k) HIPCHK(c, hipMemcpyAsync(base + size_t(p) * stride + o[k], src[k] + size_t(p) * n, n * 4, hipMemcpyHostToDevice, sm));
    bt.n = n_batch; bt.stride = n_batch > 1 ? stride : 0;
    return 0;
  }
};
int pf_stage_adjust_initial_flow_batch(pf_ctx* c, int n_batch, const float* i0, const float* i1, const float* a0, const float* a1, int w, int h, int hint, int max_pct,
                                       float* flow_out) {
  STAGE_BEGIN(c);
  if (int e = check_batch3(c, n_batch)) return e;
  if (!i0 || !i1 || !a0 || !a1 || !flow_out) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, w, h)) return e;
  if (hint < PF_HINT_RIGHT || hint > PF_HINT_UP || max_pct < 1 || max_pct > 100) return fail(c, PF_ERR_ARG, "hint %d (1..4) / max_percentage %d (1..100)", hint, max_pct);
  const size_t n = size_t(w) * h, fpad = (n * 2 + 63) & ~size_t(63);
  const float* const src[4] = {i0, i1, a0, a1};
  SearchSlabs s;
  if (int e = s.up(c, sm, n_batch, src, n, fpad * 4)) return e;
  launch_fill_u32(sm, reinterpret_cast<unsigned*>(s.flow()), n * 2, 0u, s.bt);   // PixFlow.hpp:298, as solve_n
  launch_adjust_initial_flow(sm, s.plane(0), s.plane(1), s.plane(2), s.plane(3), w, h, hint, max_pct, s.ratio(), s.flow(), s.bt);
  HIPCHK(c, hipGetLastError());
  for (int p = 0; p < n_batch; ++p) HIPCHK(c, hipMemcpyAsync(flow_out + size_t(p) * fpad, (char*)s.flow() + size_t(p) * s.stride, fpad * 4, hipMemcpyDeviceToHost, sm));
  return finish(c);
}
int pf_stage_intensity_ratio(pf_ctx* c, int n_batch, const float* i0, const float* i1, const float* a0, const float* a1, int n, float* ratio_out) {
  STAGE_BEGIN(c);
  if (int e = check_batch3(c, n_batch)) return e;
  if (!i0 || !i1 || !a0 || !a1 || !ratio_out) return fail(c, PF_ERR_ARG, "null pointer");
  if (n < 1) return fail(c, PF_ERR_ARG, "%d elements", n);
  const float* const src[4] = {i0, i1, a0, a1};
  SearchSlabs s;
  if (int e = s.up(c, sm, n_batch, src, size_t(n), 0)) return e;
  launch_intensity_ratio(sm, s.plane(0), s.plane(1), s.plane(2), s.plane(3), n, s.ratio(), s.bt);
  HIPCHK(c, hipGetLastError());
  for (int p = 0; p < n_batch; ++p) HIPCHK(c, hipMemcpyAsync(ratio_out + p, (char*)s.ratio() + size_t(p) * s.stride, 4, hipMemcpyDeviceToHost, sm));
  return finish(c);
}

// ---- profiling ----
int pf_profile_enable(pf_ctx* c, int on) { if (!c) return PF_ERR_ARG; c->prof = on < 0 ? 0 : (on > 2 ? 1 : on); return 0; }
int pf_profile_reset(pf_ctx* c) { if (!c) return PF_ERR_ARG; for (auto& t : c->prof_tot) t = ProfEntry(); return 0; }
// (kernel families only: warnings are reported by pf_last_warning / pf_warning_count, not as a pseudo-entry of this list -- round 5 had one)
int pf_profile_count(pf_ctx* c) { return c ? (int)c->prof_names.size() : 0; }
int pf_profile_get(pf_ctx* c, int idx, char* name, int cap, double* ms, int* launches) {
  if (!c || idx < 0 || idx >= (int)c->prof_names.size()) return PF_ERR_ARG;
  if (name && cap > 0) { strncpy(name, c->prof_names[idx].c_str(), cap - 1); name[cap - 1] = 0; }
  if (ms) *ms = c->prof_tot[idx].ms;
  if (launches) *launches = c->prof_tot[idx].n;
  return 0;
}

long long pf_last_swept_steps(pf_ctx* c) { return c ? c->last_swept_steps : 0; }

long long pf_level_pixels(int cols, int rows, int* n_levels, long long* sweep_steps) {
  const Geometry g = make_geometry(cols, rows, cols / 20);
  long long steps = 0;
  for (int l = 0; l < g.n; ++l) steps += g.ws[l] + g.hs[l] - 1;
  if (n_levels) *n_levels = g.n;
  if (sweep_steps) *sweep_steps = 2 * steps;
  return (long long)g.Pexact;
}
double pf_algorithmic_bytes(int cols, int rows) {  // B_alg = 472.75*P + 102.4*C*R
  return 472.75 * (double)pf_level_pixels(cols, rows, nullptr, nullptr) + 102.4 * (double)cols * rows;
}

