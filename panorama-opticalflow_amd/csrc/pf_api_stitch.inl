// Part of pf_api.hip (one translation unit, split along its seams in round 5): Stitchtools: prepare / match / blend ramp / gather, the device-resident chain step and its prefetch.

// The ramp's geometry is ramp_geom()'s (kernels_misc.hip), computed once per call.
static bool tile_reach_ok(int cols, int rows, int k) { return tile_blur_reach(k) < (cols < rows ? cols : rows); }
// refuses a canvas whose ramp neither form of the tile smoothing covers (never one that was accepted before the streamed form existed)
static int check_blend_ramp(pf_ctx* c, int cols, int rows, const RampGeom& g) {
  if (g.ok) return 0;
  return fail(c, PF_ERR_ARG, "canvas %dx%d: the blend-ramp smoothing window (%d) reaches across the whole canvas", cols, rows, g.k1);
}
namespace {
// per-frame planes of a group, `count` frames back to back in one arena buffer (256-byte aligned frames)
extern "C++" template <class T> T* frame_planes(pf_ctx* c, const char* name, int count, size_t per_frame, size_t& stride) {
  stride = (per_frame + 255) & ~size_t(255);
  return (T*)ensure(c, name, stride * count);
}
}  // namespace
// What the ramp of `count` frames needs beside blend / md: the tile pass's work area and (streamed form) row sums, the box blur's
// fp64 row sums and result planes (p.rs / p.tmp).  From the arena buffers named here: the lone entry points' (pre-sized by
// pf_create) or the batched step's.  own_tmp = false: the caller supplies p.tmp (a plan's ramp planes), none is allocated here.
struct RampArena { const char* work; const char* scratch; const char* rowsum; const char* blur_tmp; };
static const RampArena kRampLone = {"st_tile_work", "st_tile_scratch", "st_rowsum", "st_blur_tmp"}, kRampBatch = {"sb_tile_work", "sb_tile_scratch", "sb_rowsum", "sb_blur_tmp"};
struct RampWork { void* work = nullptr; void* scratch = nullptr; };
static int ramp_planes(pf_ctx* c, const RampArena& a, int count, int cols, int rows, const RampGeom& g, StitchPtrs& p, RampWork& w, bool own_tmp = true) {
  if (!g.ok) return 0;   // blend_ramp_dev refuses the canvas
  const size_t n = size_t(cols) * rows;
  if (g.tiles) {
    w.work = ensure(c, a.work, tile_blur_work_bytes(cols, rows, g.step, g.k1) + 256);
    if (g.streamed) w.scratch = ensure(c, a.scratch, tile_blur_stream_scratch_bytes(g.step, g.k1));
    if (!w.work || (g.streamed && !w.scratch)) return PF_ERR_NOMEM;
  }
  if (g.k2 > 0) {
    size_t s8, s4 = 0;
    double* rs = frame_planes<double>(c, a.rowsum, count, n * 8, s8); float* tmp = own_tmp ? frame_planes<float>(c, a.blur_tmp, count, n * 4, s4) : nullptr;
    if (!rs || (own_tmp && !tmp)) return PF_ERR_NOMEM;
    for (int f = 0; f < count; ++f) { p.rs[f] = (double*)((char*)rs + f * s8); p.tmp[f] = own_tmp ? (float*)((char*)tmp + f * s4) : nullptr; }
  }
  return 0;
}
// the tile pass alone: p.blend of `count` frames in place, explicit geometry
static void tile_pass_dev(pf_ctx* c, hipStream_t sm, const StitchPtrs& p, int count, int cols, int rows, int step, int k, bool streamed, const RampWork& w) {
  { PROF(c, sm, "tile_blur"); launch_tile_blur(sm, p, count, cols, rows, step, k, w.work, streamed, w.scratch); }
  launch_collect_status(sm, static_cast<const int*>(w.work), 2, c->d_status, 4);   // word 1 = a grid barrier of the tile smoothing gave up
}
// ... of one canvas on the lone entry points' arena buffers (pf_stage_tile_blur)
static int tile_blur_dev(pf_ctx* c, hipStream_t sm, float* d_blend, float* d_md, int cols, int rows, int step, int k, bool streamed) {
  RampGeom g; g.step = step; g.k1 = k; g.tiles = true; g.streamed = streamed;
  StitchPtrs p{}; p.blend[0] = d_blend; p.md[0] = d_md;
  RampWork w;
  if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w)) return e;
  tile_pass_dev(c, sm, p, 1, cols, rows, step, k, streamed, w);
  return 0;
}
// The blend ramp of `count` frames on stream sm (GenerateBlend + countblend + smoothing, StitchTool.cpp:98-191): countblend from
// p.map (from_map; otherwise p.blend / p.md are given), the tile pass in place, its status word, the rows/400 box blur into p.tmp.
// ramp[f] = where frame f's finished ramp lies: p.tmp[f] if the box blur ran, else p.blend[f].
static int blend_ramp_dev(pf_ctx* c, hipStream_t sm, const StitchPtrs& p, int count, int cols, int rows, const RampGeom& g, const RampWork& w, bool from_map,
                          const float** ramp) {
  if (int e = check_blend_ramp(c, cols, rows, g)) return e;
  if (from_map) { PROF(c, sm, "countblend"); launch_countblend(sm, p, count, cols, rows); }
  if (g.tiles) tile_pass_dev(c, sm, p, count, cols, rows, g.step, g.k1, g.streamed, w);
  if (g.k2 > 0) { PROF(c, sm, "box_blur"); launch_box_blur(sm, p, count, cols, rows, g.k2); }
  for (int f = 0; f < count; ++f) ramp[f] = g.k2 > 0 ? p.tmp[f] : p.blend[f];
  return 0;
}
// One iteration of the reference's stitch loop (CPU/main.cpp:70-95) for `count` frames on device planes the caller supplies (p: all
// but L / R / out are working planes; w and p.rs / p.tmp from ramp_planes; flows[2f], flows[2f + 1]: frame f's two flow planes):
// Stitchtools::prepare -> NovelViewGeneratorAsymmetricFlow::prepare/generateNovelView -> Gather, enqueued, not drained.
// With a plan (stitch plans, further down): p.map[f] = the plan's map for every frame, the match verifies against it
// (c->h_plan_diff[f], read by the caller after its final sync), the ramp is the plan's, and there is no ramp launch, stream or event.
static int stitch_step_dev(pf_ctx* c, const StitchPtrs& p, int count, float* const* flows, int cols, int rows, int max_pct, const RampGeom& g, const RampWork& w,
                           const pf_stitch_plan* plan = nullptr) {
  hipStream_t sm = c->s_main;
  const int hints[2] = {PF_HINT_LEFT, PF_HINT_RIGHT};
  BlendPtrs bp{};
  if (plan) {
    for (int f = 0; f < count; ++f) c->h_plan_diff[f] = 0;
    { PROF(c, sm, "match_verify"); launch_match_verify(sm, p, count, cols, rows, c->d_plan_diff); }
    if (int e = solve_n(c, count, p.ovL, p.ovR, cols, rows, cols / 20, max_pct, 2, hints, flows)) return e;
    for (int f = 0; f < count; ++f) bp.blend[f] = plan->ramp;
  } else {
    { PROF(c, sm, "match_images"); launch_match_images(sm, p, count, cols, rows); }
    // The blend ramp only depends on the map and is only needed by the final blend: it runs on its own stream beside the two flow
    // solves.  Its launches (a dozen since the tile smoothing became ONE persistent launch in round 3; ~850 before) are enqueued AFTER
    // the solver's, so that the solver's first kernel is not kept waiting by them.
    if (!c->s_aux) HIPCHK(c, hipStreamCreateWithFlags(&c->s_aux, hipStreamNonBlocking));
    hipStream_t sa = c->s_aux;
    HIPCHK(c, hipEventRecord(c->ev_aux_go, sm));
    if (int e = solve_n(c, count, p.ovL, p.ovR, cols, rows, cols / 20, max_pct, 2, hints, flows)) return e;
    HIPCHK(c, hipStreamWaitEvent(sa, c->ev_aux_go, 0));
    if (int e = blend_ramp_dev(c, sa, p, count, cols, rows, g, w, true, bp.blend)) return e;
    HIPCHK(c, hipEventRecord(c->ev_aux_done, sa));
    HIPCHK(c, hipStreamWaitEvent(sm, c->ev_aux_done, 0));
  }
  for (int f = 0; f < count; ++f) { bp.L[f] = p.ovL[f]; bp.R[f] = p.ovR[f]; bp.fLR[f] = flows[2 * f]; bp.fRL[f] = flows[2 * f + 1]; bp.out[f] = p.merged[f]; }
  { PROF(c, sm, "blend"); launch_blend(sm, bp, count, cols, rows); }
  { PROF(c, sm, "gather"); launch_gather(sm, p, count, cols, rows); }
  return 0;
}

int pf_stitch_prepare(pf_ctx* c, const uint8_t* l, const uint8_t* r, int cols, int rows, size_t step, uint8_t* map_out, size_t mstep, uint8_t* ovl,
                      uint8_t* ovr, float* blend_out, size_t bstep, float* merged_dis) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!l || !r) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (step < size_t(cols) * 4 || (map_out && mstep < size_t(cols)) || (blend_out && bstep < size_t(cols) * 4)) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  uint8_t* dl = (uint8_t*)ensure(c, "h_img0", n * 4); uint8_t* dr = (uint8_t*)ensure(c, "h_img1", n * 4);
  uint8_t* dm = (uint8_t*)ensure(c, "st_map", n); uint8_t* dol = (uint8_t*)ensure(c, "st_ovl", n * 4); uint8_t* dor = (uint8_t*)ensure(c, "st_ovr", n * 4);
  float* db = (float*)ensure(c, "st_blend", n * 4); float* dmd = (float*)ensure(c, "st_md", n * 4);
  if (!dl || !dr || !dm || !dol || !dor || !db || !dmd) return PF_ERR_NOMEM;
  const RampGeom g = ramp_geom(cols, rows);
  StitchPtrs p{}; p.L[0] = dl; p.R[0] = dr; p.map[0] = dm; p.ovL[0] = dol; p.ovR[0] = dor; p.blend[0] = db; p.md[0] = dmd;
  RampWork w;
  if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w)) return e;
  hipStream_t sm = c->s_main;
  if (int e = up2d(c, dl, size_t(cols) * 4, l, step, size_t(cols) * 4, rows)) return e;
  if (int e = up2d(c, dr, size_t(cols) * 4, r, step, size_t(cols) * 4, rows)) return e;
  { PROF(c, sm, "match_images"); launch_match_images(sm, p, 1, cols, rows); }
  const float* ramp = nullptr;
  if (int e = blend_ramp_dev(c, sm, p, 1, cols, rows, g, w, true, &ramp)) return e;
  if (map_out) if (int e = down2d(c, map_out, mstep, dm, cols, cols, rows)) return e;
  if (ovl) if (int e = down2d(c, ovl, step, dol, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  if (ovr) if (int e = down2d(c, ovr, step, dor, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  if (blend_out) if (int e = down2d(c, blend_out, bstep, ramp, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  if (merged_dis) if (int e = down2d(c, merged_dis, size_t(cols) * 4, dmd, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  return check_sweeps(c);
}

// Stitchtools::MatchImages (StitchTool.cpp:38-50) + the overlap masking of prepare() (:17-33) alone: map and the two masked images.
int pf_stitch_match(pf_ctx* c, const uint8_t* l, const uint8_t* r, int cols, int rows, size_t step, uint8_t* map_out, size_t mstep, uint8_t* ovl, uint8_t* ovr) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!l || !r) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (step < size_t(cols) * 4 || (map_out && mstep < size_t(cols))) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  uint8_t* dl = (uint8_t*)ensure(c, "h_img0", n * 4); uint8_t* dr = (uint8_t*)ensure(c, "h_img1", n * 4);
  uint8_t* dm = (uint8_t*)ensure(c, "st_map", n); uint8_t* dol = (uint8_t*)ensure(c, "st_ovl", n * 4); uint8_t* dor = (uint8_t*)ensure(c, "st_ovr", n * 4);
  if (!dl || !dr || !dm || !dol || !dor) return PF_ERR_NOMEM;
  if (int e = up2d(c, dl, size_t(cols) * 4, l, step, size_t(cols) * 4, rows)) return e;
  if (int e = up2d(c, dr, size_t(cols) * 4, r, step, size_t(cols) * 4, rows)) return e;
  StitchPtrs p{}; p.L[0] = dl; p.R[0] = dr; p.map[0] = dm; p.ovL[0] = dol; p.ovR[0] = dor;
  { PROF(c, c->s_main, "match_images"); launch_match_images(c->s_main, p, 1, cols, rows); }
  if (map_out) if (int e = down2d(c, map_out, mstep, dm, cols, cols, rows)) return e;
  if (ovl) if (int e = down2d(c, ovl, step, dol, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  if (ovr) if (int e = down2d(c, ovr, step, dor, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  HIPCHK(c, hipGetLastError());
  return finish(c);
}

// Stitchtools::GenerateBlend (StitchTool.cpp:98-146) from a GIVEN map -- the reference reads its public `Map` member there, so a
// caller that edits the map between MatchImages() and GenerateBlend() gets the ramp of the edited map.
int pf_stitch_generate_blend(pf_ctx* c, const uint8_t* map, size_t mstep, int cols, int rows, float* blend_out, size_t bstep, float* merged_dis) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!map || !blend_out) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (mstep < size_t(cols) || bstep < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  uint8_t* dm = (uint8_t*)ensure(c, "st_map", n); float* db = (float*)ensure(c, "st_blend", n * 4); float* dmd = (float*)ensure(c, "st_md", n * 4);
  if (!dm || !db || !dmd) return PF_ERR_NOMEM;
  const RampGeom g = ramp_geom(cols, rows);
  StitchPtrs p{}; p.map[0] = dm; p.blend[0] = db; p.md[0] = dmd;
  RampWork w;
  if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w)) return e;
  if (int e = up2d(c, dm, cols, map, mstep, cols, rows)) return e;
  const float* ramp = nullptr;
  if (int e = blend_ramp_dev(c, c->s_main, p, 1, cols, rows, g, w, true, &ramp)) return e;
  if (int e = down2d(c, blend_out, bstep, ramp, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  if (merged_dis) if (int e = down2d(c, merged_dis, size_t(cols) * 4, dmd, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  return check_sweeps(c);
}

// GenerateBlend's per-pixel part alone (StitchTool.cpp:113-125 with countblend :148-191): the ramp BEFORE the tile / global
// box smoothing, i.e. what Stitchtools::countblend(x, y) returns for overlap pixels, and MergedDis.
int pf_stitch_raw_blend(pf_ctx* c, const uint8_t* l, const uint8_t* r, int cols, int rows, size_t step, float* raw_blend, size_t bstep, float* merged_dis) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!l || !r || !raw_blend) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (step < size_t(cols) * 4 || bstep < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  uint8_t* dl = (uint8_t*)ensure(c, "h_img0", n * 4); uint8_t* dr = (uint8_t*)ensure(c, "h_img1", n * 4);
  uint8_t* dm = (uint8_t*)ensure(c, "st_map", n); uint8_t* dol = (uint8_t*)ensure(c, "st_ovl", n * 4); uint8_t* dor = (uint8_t*)ensure(c, "st_ovr", n * 4);
  float* db = (float*)ensure(c, "st_blend", n * 4); float* dmd = (float*)ensure(c, "st_md", n * 4);
  if (!dl || !dr || !dm || !dol || !dor || !db || !dmd) return PF_ERR_NOMEM;
  hipStream_t sm = c->s_main;
  if (int e = up2d(c, dl, size_t(cols) * 4, l, step, size_t(cols) * 4, rows)) return e;
  if (int e = up2d(c, dr, size_t(cols) * 4, r, step, size_t(cols) * 4, rows)) return e;
  StitchPtrs p{}; p.L[0] = dl; p.R[0] = dr; p.map[0] = dm; p.ovL[0] = dol; p.ovR[0] = dor; p.blend[0] = db; p.md[0] = dmd;
  { PROF(c, sm, "match_images"); launch_match_images(sm, p, 1, cols, rows); }
  { PROF(c, sm, "countblend"); launch_countblend(sm, p, 1, cols, rows); }
  if (int e = down2d(c, raw_blend, bstep, db, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  if (merged_dis) if (int e = down2d(c, merged_dis, size_t(cols) * 4, dmd, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  HIPCHK(c, hipGetLastError());
  return finish(c);
}

int pf_stitch_gather(pf_ctx* c, const uint8_t* l, const uint8_t* r, const uint8_t* merged, size_t step, const uint8_t* map, size_t mstep, int cols,
                     int rows, uint8_t* out, size_t ostep) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!l || !r || !merged || !map || !out) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (step < size_t(cols) * 4 || ostep < size_t(cols) * 4 || mstep < size_t(cols)) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  uint8_t* dl = (uint8_t*)ensure(c, "h_img0", n * 4); uint8_t* dr = (uint8_t*)ensure(c, "h_img1", n * 4); uint8_t* dg = (uint8_t*)ensure(c, "st_merged", n * 4);
  uint8_t* dm = (uint8_t*)ensure(c, "st_map", n); uint8_t* dout = (uint8_t*)ensure(c, "h_out", n * 4);
  if (!dl || !dr || !dg || !dm || !dout) return PF_ERR_NOMEM;
  if (int e = up2d(c, dl, size_t(cols) * 4, l, step, size_t(cols) * 4, rows)) return e;
  if (int e = up2d(c, dr, size_t(cols) * 4, r, step, size_t(cols) * 4, rows)) return e;
  if (int e = up2d(c, dg, size_t(cols) * 4, merged, step, size_t(cols) * 4, rows)) return e;
  if (int e = up2d(c, dm, cols, map, mstep, cols, rows)) return e;
  StitchPtrs p{}; p.L[0] = dl; p.R[0] = dr; p.merged[0] = dg; p.map[0] = dm; p.out[0] = dout;
  { PROF(c, c->s_main, "gather"); launch_gather(c->s_main, p, 1, cols, rows); }
  if (int e = down2d(c, out, ostep, dout, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  HIPCHK(c, hipGetLastError());
  return finish(c);
}


// One whole iteration of the reference's stitch loop without leaving the device (stitch_step_dev with one frame on the arena's
// own planes).  r_bgra == NULL chains on the previous call's result, which stays resident in HBM (main.cpp:64-65).
// Content signature of a host image: 16 evenly spaced rows, 8 bytes at a time (~0.1 ms at 9000x4000).  The prefetched device copy of
// an image is only used if the caller's buffer still carries the signature it had when it was uploaded: pointer, size and step alone
// cannot tell a buffer from another image that an allocator later placed at the same address (the intended use is one cv::Mat freed and
// re-read per image).
static uint64_t host_image_sig(const uint8_t* p, int cols, int rows, size_t step) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  const size_t rb = size_t(cols) * 4;
  for (int i = 0; i < 16; ++i) {
    const uint8_t* row = p + size_t((long long)(rows - 1) * i / 15) * step;
    for (size_t o = 0; o + 8 <= rb; o += 8) { uint64_t v; memcpy(&v, row + o, 8); h = (h ^ v) * 0xBF58476D1CE4E5B9ull; h ^= h >> 29; }
  }
  return h;
}

// a handle is valid if the context lists it (no dereference before that: a destroyed plan, or another context's, is refused by address)
static int check_plan(pf_ctx* c, const pf_stitch_plan* plan, int cols, int rows, const char* what) {
  if (std::find(c->plans.begin(), c->plans.end(), plan) == c->plans.end()) return fail(c, PF_ERR_ARG, "%s: not a live stitch plan of this context", what);
  if (plan->cols != cols || plan->rows != rows) return fail(c, PF_ERR_ARG, "%s: the plan is %dx%d, the canvas %dx%d", what, plan->cols, plan->rows, cols, rows);
  return 0;
}
// after the final sync of a planned group of `count` frames (first = index of its frame 0 in the call): pixels per frame that differ
// from the plan, into diff[first ..] (the caller reports); the words are left zeroed
static void collect_plan_diff(pf_ctx* lane, int first, int count, unsigned* diff) {
  for (int f = 0; f < count; ++f) { diff[first + f] = __atomic_load_n(lane->h_plan_diff + f, __ATOMIC_ACQUIRE); lane->h_plan_diff[f] = 0; }
}
// (tools/pano_stitch.cpp reads the frame index out of this message to name the directory: keep "frame %d differs from the stitch plan")
static int report_plan_diff(pf_ctx* c, const char* what, const unsigned* diff, int n_frames) {
  for (int k = 0; k < n_frames; ++k)
    if (diff[k]) return fail(c, PF_ERR_ARG, "%s: frame %d differs from the stitch plan in %u pixels' region codes (alpha masks are not the plan's)", what, k, diff[k]);
  return 0;
}

static int stitch_step_lone(pf_ctx* c, const pf_stitch_plan* plan, const uint8_t* l, const uint8_t* r, int cols, int rows, size_t step, int max_pct, uint8_t* out, size_t ostep) {
  const char* const what = plan ? "pf_stitch_step_planned" : "pf_stitch_step";
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!l) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_dims(c, cols, rows, cols / 20)) return e;
  if (plan) if (int e = check_plan(c, plan, cols, rows, what)) return e;
  if (step < size_t(cols) * 4 || (out && ostep < size_t(cols) * 4)) return fail(c, PF_ERR_ARG, "row step too small");
  check_hw_queues(c, plan ? 4 : 5, what);   // front end, two flow directions, blend ramp (unplanned), prefetch copy
  c->vis_step_valid = false;
  const size_t n = size_t(cols) * rows;
  uint8_t* dl = (uint8_t*)ensure(c, "ch_l", n * 4); uint8_t* dr = (uint8_t*)ensure(c, "ch_r", n * 4); uint8_t* dfin = (uint8_t*)ensure(c, "ch_final", n * 4);
  // a planned step needs neither a map nor ramp planes of its own
  uint8_t* dm = plan ? plan->map : (uint8_t*)ensure(c, "st_map", n); uint8_t* dol = (uint8_t*)ensure(c, "st_ovl", n * 4); uint8_t* dor = (uint8_t*)ensure(c, "st_ovr", n * 4);
  float* db = plan ? nullptr : (float*)ensure(c, "st_blend", n * 4); float* dmd = plan ? nullptr : (float*)ensure(c, "st_md", n * 4);
  uint8_t* dmerged = (uint8_t*)ensure(c, "st_merged", n * 4);
  float* f0 = (float*)ensure(c, "nv_flow_l2r", n * 8); float* f1 = (float*)ensure(c, "nv_flow_r2l", n * 8);
  if (!dl || !dr || !dfin || !dm || !dol || !dor || (!plan && (!db || !dmd)) || !dmerged || !f0 || !f1) return PF_ERR_NOMEM;
  hipStream_t sm = c->s_main;
  uint8_t* dnext = (uint8_t*)ensure(c, "ch_l_next", n * 4);
  if (!dnext) return PF_ERR_NOMEM;
  const RampGeom g = ramp_geom(cols, rows);
  StitchPtrs p{};
  RampWork w;
  if (!plan) if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w)) return e;
  // both prefetch records are one-shot: latched and cleared here, whatever this step does with them
  const pf_ctx::HostImage ready = c->ready, hint = c->hint;
  c->ready = pf_ctx::HostImage(); c->hint = pf_ctx::HostImage();
  if (ready.src == l && ready.cols == cols && ready.rows == rows && ready.step == step && ready.sig == host_image_sig(l, cols, rows, step)) {
    // this step's left image was uploaded while the previous step computed: the two buffers trade places (no copy; the old
    // "ch_l" is free -- the previous call drained every stream -- and receives the next prefetch)
    std::swap(c->bufs["ch_l"], c->bufs["ch_l_next"]);
    std::swap(dl, dnext);
  } else {
    if (int e = up2d(c, dl, size_t(cols) * 4, l, step, size_t(cols) * 4, rows)) return e;
  }
  if (r) { if (int e = up2d(c, dr, size_t(cols) * 4, r, step, size_t(cols) * 4, rows)) return e; }
  else {
    if (c->chain_cols != cols || c->chain_rows != rows) return fail(c, PF_ERR_ARG, "%s: no previous result of this size to chain on", what);
    HIPCHK(c, hipMemcpyAsync(dr, dfin, n * 4, hipMemcpyDeviceToDevice, sm));
  }
  if (!c->s_copy) HIPCHK(c, hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking));
  p.L[0] = dl; p.R[0] = dr; p.map[0] = dm; p.ovL[0] = dol; p.ovR[0] = dor; p.blend[0] = db; p.md[0] = dmd; p.merged[0] = dmerged; p.out[0] = dfin;
  float* const flows[2] = {f0, f1};
  // "ch_final" is rewritten from here on; a frame that fails the plan leaves nothing to chain on.  (So does a planned step that fails for
  // any other reason, e.g. an allocation inside the solve, where the unplanned step keeps the old chain size: the composite it
  // would chain on is being overwritten either way, and the planned step says so.)
  if (plan) { c->chain_cols = c->chain_rows = 0; }
  if (int e = stitch_step_dev(c, p, 1, flows, cols, rows, max_pct, g, w, plan)) return e;
  // everything of this step is enqueued: upload the NEXT step's left image now (announced with pf_stitch_prefetch); the
  // host-side staging of a pageable source runs while the GPU computes
  auto prefetch_next = [&]() -> int {
    if (hint.src && hint.src != l && hint.cols == cols && hint.rows == rows) {
      if (hint.step == size_t(cols) * 4) HIPCHK(c, hipMemcpyAsync(dnext, hint.src, n * 4, hipMemcpyHostToDevice, c->s_copy));
      else HIPCHK(c, hipMemcpy2DAsync(dnext, size_t(cols) * 4, hint.src, hint.step, size_t(cols) * 4, rows, hipMemcpyHostToDevice, c->s_copy));
      HIPCHK(c, hipStreamSynchronize(c->s_copy));
      c->ready = hint;
      c->ready.sig = host_image_sig(hint.src, cols, rows, hint.step);
    }
    return 0;
  };
  if (!plan) {
    if (out) if (int e = down2d(c, out, ostep, dfin, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
    if (int e = prefetch_next()) return e;
  } else {
    // the composite goes to the caller only once the frame is known to match the plan: the step is drained (the prefetch upload ran
    // beside it), the word read, and only then the download enqueued
    if (int e = prefetch_next()) return e;
    HIPCHK(c, hipGetLastError());
    if (int e = finish(c)) return e;
    unsigned diff = 0;
    collect_plan_diff(c, 0, 1, &diff);
    if (int e = check_sweeps(c)) return e;
    if (int e = report_plan_diff(c, what, &diff, 1)) return e;
    c->drained = false;   // the download below is this call's work again
    if (out) if (int e = down2d(c, out, ostep, dfin, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  }
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  c->chain_cols = cols; c->chain_rows = rows;
  if (int e = check_sweeps(c)) return e;
  c->vis_step_valid = true;
  return 0;
}

int pf_stitch_step(pf_ctx* c, const uint8_t* l, const uint8_t* r, int cols, int rows, size_t step, int max_pct, uint8_t* out, size_t ostep) {
  return stitch_step_lone(c, nullptr, l, r, cols, rows, step, max_pct, out, ostep);
}
int pf_stitch_step_planned(pf_ctx* c, const pf_stitch_plan* plan, const uint8_t* l, const uint8_t* r, int cols, int rows, size_t step, int max_pct, uint8_t* out,
                           size_t ostep) {
  if (!c) return fail(nullptr, PF_ERR_ARG, "null context");
  if (!plan) return fail(c, PF_ERR_ARG, "pf_stitch_step_planned: null plan");
  return stitch_step_lone(c, plan, l, r, cols, rows, step, max_pct, out, ostep);
}

// Announce the left image of the pf_stitch_step call AFTER the coming one: the coming step uploads it while its own kernels run
// (the copy is issued after they are enqueued).  One-shot: the hint is consumed by the coming step; the buffer must stay valid
// and unchanged until the step after it has returned, and that step must pass the same pointer / size / step -- anything else
// simply uploads as usual and the prefetched copy is dropped.  NULL cancels.
int pf_stitch_prefetch(pf_ctx* c, const uint8_t* next_l, int cols, int rows, size_t step) {
  if (!c) return fail(nullptr, PF_ERR_ARG, "null context");
  if (next_l && (cols <= 0 || rows <= 0)) return fail(c, PF_ERR_ARG, "bad argument");
  if (next_l && step < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  c->hint.src = next_l; c->hint.cols = cols; c->hint.rows = rows; c->hint.step = step;
  return 0;
}


// ---- batched stitch step: many canvases in flight ----
// Frame k of a call is exactly one pf_stitch_step of its own chain; frames share nothing but the launches.  Groups of up to
// kMaxBatch frames go through one set of launches (blockIdx.z = frame) on a lane of the throughput mode (run_lanes): the batched
// match on the lane's main stream, the blend ramp (countblend, ONE persistent tile-smoothing launch for all frames, box blur) on
// its aux stream beside solve_n() of the overlaps on the direction streams, then the batched novel-view blend and gather.
namespace {
// everything pf_stitch_step refuses about the canvas, before any work
int check_stitch_canvas(pf_ctx* c, int cols, int rows, int max_pct) {
  if (int e = check_dims(c, cols, rows, cols / 20)) return e;
  if (int e = check_blend_ramp(c, cols, rows, ramp_geom(cols, rows))) return e;
  if (max_pct < 0 || max_pct > 100) return fail(c, PF_ERR_ARG, "max_percentage %d out of range", max_pct);
  return 0;
}
// plan != nullptr: a planned group -- every frame on the plan's map and ramp, 12 B/px of StitchTool planes per frame (overlaps 8,
// novel view 4) instead of 33; diff[first ..] receives the frames' counts of pixels that differ from the plan (the call reports them)
int stitch_group(pf_ctx* lane, int first, int count, const uint8_t* const* d_l, const uint8_t* const* d_r, int cols, int rows, int max_pct,
                 uint8_t* const* d_out, const pf_stitch_plan* plan = nullptr, unsigned* diff = nullptr) {
  if (int e = use(lane)) return e;
  CallGuard guard_(lane);
  const size_t n = size_t(cols) * rows;
  const RampGeom g = ramp_geom(cols, rows);
  // 33 B/px of StitchTool planes per frame (map 1, overlaps 8, ramp + MergedDis 8, box blur 12, novel view 4) + 16 B/px of flows
  size_t s1 = 0, s4, s16;
  uint8_t* map = plan ? plan->map : frame_planes<uint8_t>(lane, "sb_map", count, n, s1);
  uint8_t* ovl = frame_planes<uint8_t>(lane, "sb_ovl", count, n * 4, s4); uint8_t* ovr = frame_planes<uint8_t>(lane, "sb_ovr", count, n * 4, s4);
  float* blend = plan ? nullptr : frame_planes<float>(lane, "sb_blend", count, n * 4, s4); float* md = plan ? nullptr : frame_planes<float>(lane, "sb_md", count, n * 4, s4);
  uint8_t* merged = frame_planes<uint8_t>(lane, "sb_merged", count, n * 4, s4);
  float* flow = frame_planes<float>(lane, "sb_flow", count, n * 16, s16);
  if (!map || !ovl || !ovr || (!plan && (!blend || !md)) || !merged || !flow) return PF_ERR_NOMEM;
  StitchPtrs sp{};
  RampWork w;
  if (!plan) if (int e = ramp_planes(lane, kRampBatch, count, cols, rows, g, sp, w)) return e;
  float* flows[2 * kMaxBatch];
  for (int p = 0; p < count; ++p) {
    sp.L[p] = d_l[first + p]; sp.R[p] = d_r[first + p]; sp.out[p] = d_out[first + p];
    sp.map[p] = map + p * s1; sp.ovL[p] = ovl + p * s4; sp.ovR[p] = ovr + p * s4;
    if (!plan) { sp.blend[p] = (float*)((char*)blend + p * s4); sp.md[p] = (float*)((char*)md + p * s4); }
    sp.merged[p] = merged + p * s4;
    flows[2 * p] = (float*)((char*)flow + p * s16); flows[2 * p + 1] = flows[2 * p] + n * 2;
  }
  if (int e = stitch_step_dev(lane, sp, count, flows, cols, rows, max_pct, g, w, plan)) return e;
  HIPCHK(lane, hipGetLastError());
  if (int e = finish(lane)) return e;
  if (plan) collect_plan_diff(lane, first, count, diff);
  return check_sweeps(lane);
}
bool overlaps(const void* a, const void* b, size_t bytes) { return ranges_overlap(a, bytes, b, bytes); }
}  // namespace

static int stitch_batch_dev(pf_ctx* c, const pf_stitch_plan* plan, int n_frames, const uint8_t* const* d_l, const uint8_t* const* d_r, int cols, int rows, int max_pct,
                            uint8_t* const* d_out, int in_flight) {
  if (int e = use(c)) return e;
  c->vis_step_valid = false;   // lane 0 solves in this context's arena
  if (n_frames < 0 || !d_l || !d_r || !d_out) return fail(c, PF_ERR_ARG, "bad argument");
  if (plan) if (int e = check_plan(c, plan, cols, rows, "pf_stitch_step_batch_planned_dev")) return e;
  if (n_frames == 0) return 0;
  if (int e = check_stitch_canvas(c, cols, rows, max_pct)) return e;
  const size_t bytes = size_t(cols) * rows * 4;
  for (int k = 0; k < n_frames; ++k)
    if (!d_l[k] || !d_r[k] || !d_out[k]) return fail(c, PF_ERR_ARG, "null device pointer (frame %d)", k);
  {
    const char* const fn = plan ? "pf_stitch_step_batch_planned_dev" : "pf_stitch_step_batch_dev";
    if (int e = check_dev_align(c, fn, "d_l", d_l, n_frames)) return e;
    if (int e = check_dev_align(c, fn, "d_r", d_r, n_frames)) return e;
    if (int e = check_dev_align(c, fn, "d_out", d_out, n_frames)) return e;
  }
  // a composite is written while the frame's inputs (and those of the frames in its launches) are still read: no aliasing
  for (int k = 0; k < n_frames; ++k)
    for (int j = 0; j < n_frames; ++j)
      if (overlaps(d_out[k], d_l[j], bytes) || overlaps(d_out[k], d_r[j], bytes) || (j != k && overlaps(d_out[k], d_out[j], bytes)))
        return fail(c, PF_ERR_ARG, "d_out[%d] overlaps an input or another output of the call (frame %d)", k, j);
  if (!plan)
    return run_lanes(c, n_frames, in_flight, cols, rows, 3, "pf_stitch_step_batch", [&](pf_ctx* lane, int first, int count) {
      return stitch_group(lane, first, count, d_l, d_r, cols, rows, max_pct, d_out);
    });
  std::vector<unsigned> diff(n_frames, 0u);
  if (int e = run_lanes(c, n_frames, in_flight, cols, rows, 3, "pf_stitch_step_batch_planned", [&](pf_ctx* lane, int first, int count) {
        return stitch_group(lane, first, count, d_l, d_r, cols, rows, max_pct, d_out, plan, diff.data());
      })) return e;
  if (std::all_of(diff.begin(), diff.end(), [](unsigned d) { return d == 0; })) return 0;
  // the call fails as a whole: no composite is delivered (the gathers have run, so the caller's buffers are cleared)
  {
    CallGuard guard_(c);
    for (int k = 0; k < n_frames; ++k) HIPCHK(c, hipMemsetAsync(d_out[k], 0, bytes, c->s_main));
    if (int e = finish(c)) return e;
  }
  return report_plan_diff(c, "pf_stitch_step_batch_planned_dev", diff.data(), n_frames);
}
int pf_stitch_step_batch_dev(pf_ctx* c, int n_frames, const uint8_t* const* d_l, const uint8_t* const* d_r, int cols, int rows, int max_pct,
                             uint8_t* const* d_out, int in_flight) {
  return stitch_batch_dev(c, nullptr, n_frames, d_l, d_r, cols, rows, max_pct, d_out, in_flight);
}
int pf_stitch_step_batch_planned_dev(pf_ctx* c, const pf_stitch_plan* plan, int n_frames, const uint8_t* const* d_l, const uint8_t* const* d_r, int cols, int rows,
                                     int max_pct, uint8_t* const* d_out, int in_flight) {
  if (!c) return fail(nullptr, PF_ERR_ARG, "null context");
  if (!plan) return fail(c, PF_ERR_ARG, "pf_stitch_step_batch_planned_dev: null plan");
  return stitch_batch_dev(c, plan, n_frames, d_l, d_r, cols, rows, max_pct, d_out, in_flight);
}

// Host form: one slot of three planes per frame index (12 B/px: left, right, composite), kept between calls so that frame k may
// chain on its own previous composite.  The slots are separate from pf_stitch_step's chain ("ch_*") and prefetch records.
static int stitch_batch_host(pf_ctx* c, const pf_stitch_plan* plan, int n_frames, const uint8_t* const* l, const uint8_t* const* r, int cols, int rows, size_t step,
                             int max_pct, uint8_t* const* out, size_t ostep, int in_flight) {
  if (int e = use(c)) return e;
  c->vis_step_valid = false;
  if (n_frames < 0 || !l) return fail(c, PF_ERR_ARG, "bad argument");
  if (plan) if (int e = check_plan(c, plan, cols, rows, "pf_stitch_step_batch_planned")) return e;
  if (n_frames == 0) return 0;
  for (int k = 0; k < n_frames; ++k) if (!l[k]) return fail(c, PF_ERR_ARG, "null pointer (frame %d)", k);
  if (int e = check_stitch_canvas(c, cols, rows, max_pct)) return e;
  if (step < size_t(cols) * 4 || (out && ostep < size_t(cols) * 4)) return fail(c, PF_ERR_ARG, "row step too small");
  for (int k = 0; k < n_frames; ++k)
    if ((!r || !r[k]) && (c->sb_cols != cols || c->sb_rows != rows || k >= c->sb_frames))
      return fail(c, PF_ERR_ARG, "pf_stitch_step_batch: frame %d has no previous batch result of this size to chain on", k);
  const size_t n = size_t(cols) * rows;
  std::vector<uint8_t*> dl(n_frames), dr(n_frames), dfin(n_frames);
  for (int k = 0; k < n_frames; ++k) {
    char name[32];
    snprintf(name, sizeof name, "sb_l%d", k); dl[k] = (uint8_t*)ensure(c, name, n * 4);
    snprintf(name, sizeof name, "sb_r%d", k); dr[k] = (uint8_t*)ensure(c, name, n * 4);
    snprintf(name, sizeof name, "sb_fin%d", k); dfin[k] = (uint8_t*)ensure(c, name, n * 4);
    if (!dl[k] || !dr[k] || !dfin[k]) return PF_ERR_NOMEM;
  }
  c->sb_frames = 0;   // the slots are rewritten from here on: chaining needs this call to succeed
  {
    CallGuard guard_(c);
    for (int k = 0; k < n_frames; ++k) {
      if (int e = up2d(c, dl[k], size_t(cols) * 4, l[k], step, size_t(cols) * 4, rows)) return e;
      if (r && r[k]) { if (int e = up2d(c, dr[k], size_t(cols) * 4, r[k], step, size_t(cols) * 4, rows)) return e; }
      else HIPCHK(c, hipMemcpyAsync(dr[k], dfin[k], n * 4, hipMemcpyDeviceToDevice, c->s_main));
    }
    if (int e = finish(c)) return e;   // the lanes' streams start from complete inputs
  }
  std::vector<unsigned> diff(plan ? n_frames : 0, 0u);
  const int e = run_lanes(c, n_frames, in_flight, cols, rows, 3, plan ? "pf_stitch_step_batch_planned" : "pf_stitch_step_batch", [&](pf_ctx* lane, int first, int count) {
    return stitch_group(lane, first, count, dl.data(), dr.data(), cols, rows, max_pct, dfin.data(), plan, diff.data());
  });
  if (e) return e;
  // a frame off the plan fails the call as a whole: nothing is downloaded, and the slots stay invalid (sb_frames = 0 above)
  if (plan) if (int e2 = report_plan_diff(c, "pf_stitch_step_batch_planned", diff.data(), n_frames)) return e2;
  if (out) {
    CallGuard guard_(c);
    for (int k = 0; k < n_frames; ++k)
      if (out[k]) if (int e2 = down2d(c, out[k], ostep, dfin[k], size_t(cols) * 4, size_t(cols) * 4, rows)) return e2;
    HIPCHK(c, hipGetLastError());
    if (int e2 = finish(c)) return e2;
  }
  c->sb_cols = cols; c->sb_rows = rows; c->sb_frames = n_frames;
  return 0;
}
int pf_stitch_step_batch(pf_ctx* c, int n_frames, const uint8_t* const* l, const uint8_t* const* r, int cols, int rows, size_t step, int max_pct,
                         uint8_t* const* out, size_t ostep, int in_flight) {
  return stitch_batch_host(c, nullptr, n_frames, l, r, cols, rows, step, max_pct, out, ostep, in_flight);
}
int pf_stitch_step_batch_planned(pf_ctx* c, const pf_stitch_plan* plan, int n_frames, const uint8_t* const* l, const uint8_t* const* r, int cols, int rows, size_t step,
                                 int max_pct, uint8_t* const* out, size_t ostep, int in_flight) {
  if (!c) return fail(nullptr, PF_ERR_ARG, "null context");
  if (!plan) return fail(c, PF_ERR_ARG, "pf_stitch_step_batch_planned: null plan");
  return stitch_batch_host(c, plan, n_frames, l, r, cols, rows, step, max_pct, out, ostep, in_flight);
}

// ---- stitch plans ----
// Creation: MatchImages into the plan's map, then the blend ramp by blend_ramp_dev with ramp_geom()'s geometry and form, finishing in
// the plan's ramp plane (the box blur's result plane, or the in-place ramp where the canvas has no box blur); the working planes are the
// lone entry points' ("st_*"), the inputs go through "h_img0/1": the chain ("ch_*"), the prefetch records and the visualiser's inputs stay.
static int stitch_plan_make(pf_ctx* c, const uint8_t* dl, const uint8_t* dr, int cols, int rows, const RampGeom& g, pf_stitch_plan** plan_out) {
  const size_t n = size_t(cols) * rows;
  uint8_t* dol = (uint8_t*)ensure(c, "st_ovl", n * 4); uint8_t* dor = (uint8_t*)ensure(c, "st_ovr", n * 4);
  float* db = (float*)ensure(c, "st_blend", n * 4); float* dmd = (float*)ensure(c, "st_md", n * 4);
  unsigned* dcount = (unsigned*)ensure(c, "plan_count", 256);
  if (!dol || !dor || !db || !dmd || !dcount) return PF_ERR_NOMEM;
  StitchPtrs p{};
  RampWork w;
  if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w, false)) return e;
  pf_stitch_plan* pl = new pf_stitch_plan();
  pl->cols = cols; pl->rows = rows;
  struct Drop { pf_stitch_plan* pl; ~Drop() { if (pl) { hipFree(pl->map); hipFree(pl->ramp); delete pl; } } } drop{pl};
  if (hipMalloc((void**)&pl->map, (n + 255) & ~size_t(255)) != hipSuccess || hipMalloc((void**)&pl->ramp, (n * 4 + 255) & ~size_t(255)) != hipSuccess)
    return fail(c, PF_ERR_NOMEM, "hipMalloc of a %dx%d stitch plan (5 B/px) failed", cols, rows);
  hipStream_t sm = c->s_main;
  p.L[0] = dl; p.R[0] = dr; p.map[0] = pl->map; p.ovL[0] = dol; p.ovR[0] = dor; p.md[0] = dmd;
  if (g.k2 > 0) { p.blend[0] = db; p.tmp[0] = pl->ramp; } else p.blend[0] = pl->ramp;
  { PROF(c, sm, "match_images"); launch_match_images(sm, p, 1, cols, rows); }
  const float* ramp = nullptr;
  if (int e = blend_ramp_dev(c, sm, p, 1, cols, rows, g, w, true, &ramp)) return e;
  HIPCHK(c, hipMemsetAsync(dcount, 0, 4, sm));
  launch_count_code(sm, pl->map, cols, rows, 150, dcount);
  unsigned overlap = 0;
  HIPCHK(c, hipMemcpyAsync(&overlap, dcount, 4, hipMemcpyDeviceToHost, sm));
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  if (int e = check_sweeps(c)) return e;
  pl->overlap_px = overlap;
  c->plans.push_back(pl);
  drop.pl = nullptr;
  *plan_out = pl;
  return 0;
}
int pf_stitch_plan_create(pf_ctx* c, const uint8_t* l, const uint8_t* r, int cols, int rows, size_t step, pf_stitch_plan** plan_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!l || !plan_out) return fail(c, PF_ERR_ARG, "null pointer");
  *plan_out = nullptr;
  if (int e = check_dims(c, cols, rows, cols / 20)) return e;
  if (step < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const RampGeom g = ramp_geom(cols, rows);
  if (int e = check_blend_ramp(c, cols, rows, g)) return e;
  const size_t n = size_t(cols) * rows;
  uint8_t* dl = (uint8_t*)ensure(c, "h_img0", n * 4);
  if (!dl) return PF_ERR_NOMEM;
  const uint8_t* dr = nullptr;
  if (r) {
    uint8_t* up = (uint8_t*)ensure(c, "h_img1", n * 4);
    if (!up) return PF_ERR_NOMEM;
    if (int e = up2d(c, up, size_t(cols) * 4, r, step, size_t(cols) * 4, rows)) return e;
    dr = up;
  } else {
    if (c->chain_cols != cols || c->chain_rows != rows) return fail(c, PF_ERR_ARG, "pf_stitch_plan_create: no previous result of this size to take the R mask from");
    dr = (const uint8_t*)ensure(c, "ch_final", n * 4);   // read in place
    if (!dr) return PF_ERR_NOMEM;
  }
  if (int e = up2d(c, dl, size_t(cols) * 4, l, step, size_t(cols) * 4, rows)) return e;
  return stitch_plan_make(c, dl, dr, cols, rows, g, plan_out);
}
int pf_stitch_plan_create_dev(pf_ctx* c, const uint8_t* d_l, const uint8_t* d_r, int cols, int rows, pf_stitch_plan** plan_out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!d_l || !d_r || !plan_out) return fail(c, PF_ERR_ARG, "null pointer");
  *plan_out = nullptr;
  if (int e = check_dims(c, cols, rows, cols / 20)) return e;
  const RampGeom g = ramp_geom(cols, rows);
  if (int e = check_blend_ramp(c, cols, rows, g)) return e;
  const uint8_t* const imgs[2] = {d_l, d_r};
  if (int e = check_dev_align(c, "pf_stitch_plan_create_dev", "image", imgs, 2)) return e;
  return stitch_plan_make(c, d_l, d_r, cols, rows, g, plan_out);
}
int pf_stitch_plan_destroy(pf_ctx* c, pf_stitch_plan* plan) {
  if (int e = use(c)) return e;
  auto it = std::find(c->plans.begin(), c->plans.end(), plan);
  if (it == c->plans.end()) return fail(c, PF_ERR_ARG, "pf_stitch_plan_destroy: not a live stitch plan of this context");
  if (plan->rig_owned) return fail(c, PF_ERR_ARG, "pf_stitch_plan_destroy: the plan is a step of a rig plan (pf_rig_plan_destroy frees it)");
  c->plans.erase(it);
  hipFree(plan->map); hipFree(plan->ramp);   // every call is synchronous on return: nothing in flight reads them
  delete plan;
  return 0;
}
int pf_stitch_plan_info(const pf_stitch_plan* plan, int* cols, int* rows, long long* overlap_px) {
  if (!plan) return fail(nullptr, PF_ERR_ARG, "null plan");
  if (cols) *cols = plan->cols;
  if (rows) *rows = plan->rows;
  if (overlap_px) *overlap_px = plan->overlap_px;
  return 0;
}
int pf_stitch_plan_download(pf_ctx* c, const pf_stitch_plan* plan, uint8_t* map_out, size_t mstep, float* blend_out, size_t bstep) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (std::find(c->plans.begin(), c->plans.end(), plan) == c->plans.end()) return fail(c, PF_ERR_ARG, "pf_stitch_plan_download: not a live stitch plan of this context");
  const int cols = plan->cols, rows = plan->rows;
  if ((map_out && mstep < size_t(cols)) || (blend_out && bstep < size_t(cols) * 4)) return fail(c, PF_ERR_ARG, "row step too small");
  if (map_out) if (int e = down2d(c, map_out, mstep, plan->map, cols, cols, rows)) return e;
  if (blend_out) if (int e = down2d(c, blend_out, bstep, plan->ramp, size_t(cols) * 4, size_t(cols) * 4, rows)) return e;
  return finish(c);
}

// ---- rig plans: the plans of a whole chain from its n + 1 input masks, and the chain in one call ----
// A composite's alpha is > 0 exactly where L's or R's is, so the R mask of step i is top | L_1 | .. | L_{i-1}: k_rig_maps (kernels_misc.hip)
// derives every step's map in one pass over the inputs, and the n ramps go through blend_ramp_dev as ONE group of n frames.
namespace {
// a handle is valid if the context lists it (never dereferenced before that, as with stitch plans)
int check_rig(pf_ctx* c, const pf_rig_plan* rig, int cols, int rows, const char* what) {
  if (std::find(c->rigs.begin(), c->rigs.end(), rig) == c->rigs.end()) return fail(c, PF_ERR_ARG, "%s: not a live rig plan of this context", what);
  if (cols > 0 && (rig->cols != cols || rig->rows != rows)) return fail(c, PF_ERR_ARG, "%s: the rig plan is %dx%d, the canvas %dx%d", what, rig->cols, rig->rows, cols, rows);
  return 0;
}
// the mapped words k_rig_maps (verify) counts into, zeroed: frames x steps of one call
int rig_diff_words(pf_ctx* c, size_t words) {
  if (c->rig_diff_cap < words) {
    if (c->h_rig_diff) hipHostFree(c->h_rig_diff);
    c->h_rig_diff = c->d_rig_diff = nullptr; c->rig_diff_cap = 0;
    const size_t cap = std::max(words, size_t(kMaxBatch) * kMaxBatch);
    if (hipHostMalloc((void**)&c->h_rig_diff, cap * sizeof(unsigned), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->d_rig_diff, c->h_rig_diff, 0) != hipSuccess) {
      if (c->h_rig_diff) hipHostFree(c->h_rig_diff);
      c->h_rig_diff = c->d_rig_diff = nullptr;
      return fail(c, PF_ERR_NOMEM, "hipHostMalloc of %zu mapped words failed", cap);
    }
    c->rig_diff_cap = cap;
  }
  memset(c->h_rig_diff, 0, words * sizeof(unsigned));
  return 0;
}
// after the sync that followed the verifying launches: the first frame off the rig, its first differing step and the pixel count
// (tools/pano_stitch.cpp reads the frame index out of this message: keep "frame %d differs from the rig plan")
int report_rig_diff(pf_ctx* c, const char* what, int n_frames, int n_steps) {
  for (int k = 0; k < n_frames; ++k)
    for (int i = 0; i < n_steps; ++i) {
      const unsigned d = __atomic_load_n(c->h_rig_diff + size_t(k) * n_steps + i, __ATOMIC_ACQUIRE);
      if (d) return fail(c, PF_ERR_ARG, "%s: frame %d differs from the rig plan at step %d in %u pixels' region codes (alpha masks are not the rig's)", what, k, i + 1, d);
    }
  return 0;
}
uint8_t* rig_slot(pf_ctx* c, const char* kind, int w, int j, size_t bytes) {
  char name[40];
  snprintf(name, sizeof name, "rg_%s%d_%d", kind, w, j);
  return (uint8_t*)ensure(c, name, bytes);
}
bool all_aligned16(const uint8_t* const* p, size_t count) {
  uintptr_t bits = 0;
  for (size_t i = 0; i < count; ++i) bits |= (uintptr_t)p[i];
  return (bits & 15) == 0;
}
RigMaps rig_maps(const pf_rig_plan* rig) {
  RigMaps m{};
  for (int i = 0; i < rig->n_steps; ++i) m.m[i] = rig->steps[i]->map;
  return m;
}
int clamp_in_flight(int in_flight, int n_frames) {   // run_lanes' clamp
  if (in_flight < 1) in_flight = 1;
  if (in_flight > 2 * kMaxBatch) in_flight = 2 * kMaxBatch;
  if (in_flight > n_frames) in_flight = n_frames;
  return in_flight;
}
// d_img: n_steps + 1 device images (top, L_1 .. L_n) of this context's device, complete on s_main's timeline
int rig_plan_make(pf_ctx* c, int n_steps, const uint8_t* const* d_img, int cols, int rows, const RampGeom& g, pf_rig_plan** out) {
  const size_t n = size_t(cols) * rows;
  const uint8_t** tbl = (const uint8_t**)ensure(c, "rg_tbl", size_t(n_steps + 1) * sizeof(void*));
  unsigned* dcount = (unsigned*)ensure(c, "plan_count", 256);
  size_t s4 = 0;
  float* blend = frame_planes<float>(c, "sb_blend", n_steps, n * 4, s4); float* md = frame_planes<float>(c, "sb_md", n_steps, n * 4, s4);
  if (!tbl || !dcount || !blend || !md) return PF_ERR_NOMEM;
  StitchPtrs p{};
  RampWork w;
  if (int e = ramp_planes(c, kRampBatch, n_steps, cols, rows, g, p, w, false)) return e;
  pf_rig_plan* rig = new pf_rig_plan();
  rig->n_steps = n_steps; rig->cols = cols; rig->rows = rows;
  struct Drop { pf_rig_plan* rig; ~Drop() { if (rig) { for (pf_stitch_plan* pl : rig->steps) { hipFree(pl->map); hipFree(pl->ramp); delete pl; } delete rig; } } } drop{rig};
  for (int i = 0; i < n_steps; ++i) {
    pf_stitch_plan* pl = new pf_stitch_plan();
    pl->cols = cols; pl->rows = rows; pl->rig_owned = true;
    rig->steps.push_back(pl);
    if (hipMalloc((void**)&pl->map, (n + 255) & ~size_t(255)) != hipSuccess || hipMalloc((void**)&pl->ramp, (n * 4 + 255) & ~size_t(255)) != hipSuccess)
      return fail(c, PF_ERR_NOMEM, "hipMalloc of a %dx%d rig plan (5 B/px per step, %d steps) failed", cols, rows, n_steps);
  }
  hipStream_t sm = c->s_main;
  HIPCHK(c, hipMemcpyAsync(tbl, d_img, size_t(n_steps + 1) * sizeof(void*), hipMemcpyHostToDevice, sm));
  HIPCHK(c, hipMemsetAsync(dcount, 0, kMaxBatch * sizeof(unsigned), sm));
  { PROF(c, sm, "rig_maps"); launch_rig_maps_make(sm, tbl, all_aligned16(d_img, n_steps + 1), rig_maps(rig), n_steps, cols, rows, dcount); }
  for (int i = 0; i < n_steps; ++i) {
    p.map[i] = rig->steps[i]->map; p.md[i] = (float*)((char*)md + i * s4);
    float* work = (float*)((char*)blend + i * s4);
    if (g.k2 > 0) { p.blend[i] = work; p.tmp[i] = rig->steps[i]->ramp; } else p.blend[i] = rig->steps[i]->ramp;
  }
  const float* ramp[kMaxBatch];
  if (int e = blend_ramp_dev(c, sm, p, n_steps, cols, rows, g, w, true, ramp)) return e;
  unsigned overlap[kMaxBatch] = {0};
  HIPCHK(c, hipMemcpyAsync(overlap, dcount, kMaxBatch * sizeof(unsigned), hipMemcpyDeviceToHost, sm));
  HIPCHK(c, hipGetLastError());
  if (int e = finish(c)) return e;
  if (int e = check_sweeps(c)) return e;
  for (int i = 0; i < n_steps; ++i) { rig->steps[i]->overlap_px = overlap[i]; c->plans.push_back(rig->steps[i]); }
  c->rigs.push_back(rig);
  drop.rig = nullptr;
  *out = rig;
  return 0;
}
int check_rig_create(pf_ctx* c, int n_steps, const void* top, const void* l, int cols, int rows, pf_rig_plan** out, RampGeom& g) {
  if (!top || !l || !out) return fail(c, PF_ERR_ARG, "null pointer");
  *out = nullptr;
  if (n_steps < 1 || n_steps > kMaxBatch) return fail(c, PF_ERR_ARG, "a rig plan has 1..%d steps (n_steps = %d)", kMaxBatch, n_steps);
  if (int e = check_dims(c, cols, rows, cols / 20)) return e;
  g = ramp_geom(cols, rows);
  return check_blend_ramp(c, cols, rows, g);
}
}  // namespace

int pf_rig_plan_create(pf_ctx* c, int n_steps, const uint8_t* top, const uint8_t* const* l, int cols, int rows, size_t step, pf_rig_plan** out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  RampGeom g;
  if (int e = check_rig_create(c, n_steps, top, l, cols, rows, out, g)) return e;
  for (int i = 0; i < n_steps; ++i) if (!l[i]) return fail(c, PF_ERR_ARG, "null pointer (step %d)", i + 1);
  if (step < size_t(cols) * 4) return fail(c, PF_ERR_ARG, "row step too small");
  const size_t n = size_t(cols) * rows;
  const uint8_t* d_img[kMaxBatch + 1];
  for (int j = 0; j <= n_steps; ++j) {
    uint8_t* d = rig_slot(c, "in", 0, j, n * 4);
    if (!d) return PF_ERR_NOMEM;
    if (int e = up2d(c, d, size_t(cols) * 4, j == 0 ? top : l[j - 1], step, size_t(cols) * 4, rows)) return e;
    d_img[j] = d;
  }
  return rig_plan_make(c, n_steps, d_img, cols, rows, g, out);
}
int pf_rig_plan_create_dev(pf_ctx* c, int n_steps, const uint8_t* d_top, const uint8_t* const* d_l, int cols, int rows, pf_rig_plan** out) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  RampGeom g;
  if (int e = check_rig_create(c, n_steps, d_top, d_l, cols, rows, out, g)) return e;
  const uint8_t* d_img[kMaxBatch + 1];
  d_img[0] = d_top;
  for (int i = 0; i < n_steps; ++i) { if (!d_l[i]) return fail(c, PF_ERR_ARG, "null device pointer (step %d)", i + 1); d_img[i + 1] = d_l[i]; }
  if (int e = check_dev_align(c, "pf_rig_plan_create_dev", "image", d_img, size_t(n_steps) + 1)) return e;
  return rig_plan_make(c, n_steps, d_img, cols, rows, g, out);
}
int pf_rig_plan_destroy(pf_ctx* c, pf_rig_plan* rig) {
  if (int e = use(c)) return e;
  auto it = std::find(c->rigs.begin(), c->rigs.end(), rig);
  if (it == c->rigs.end()) return fail(c, PF_ERR_ARG, "pf_rig_plan_destroy: not a live rig plan of this context");
  c->rigs.erase(it);
  for (pf_stitch_plan* pl : rig->steps) {   // every call is synchronous on return: nothing in flight reads them
    c->plans.erase(std::remove(c->plans.begin(), c->plans.end(), pl), c->plans.end());
    hipFree(pl->map); hipFree(pl->ramp);
    delete pl;
  }
  delete rig;
  return 0;
}
int pf_rig_plan_info(const pf_rig_plan* rig, int* n_steps, int* cols, int* rows) {
  if (!rig) return fail(nullptr, PF_ERR_ARG, "null rig plan");
  if (n_steps) *n_steps = rig->n_steps;
  if (cols) *cols = rig->cols;
  if (rows) *rows = rig->rows;
  return 0;
}
const pf_stitch_plan* pf_rig_plan_step(pf_ctx* c, const pf_rig_plan* rig, int step) {
  if (!c) { fail(nullptr, PF_ERR_ARG, "null context"); return nullptr; }
  if (check_rig(c, rig, 0, 0, "pf_rig_plan_step")) return nullptr;
  if (step < 0 || step >= rig->n_steps) { fail(c, PF_ERR_ARG, "pf_rig_plan_step: step %d of a rig plan of %d steps (0-based)", step, rig->n_steps); return nullptr; }
  return rig->steps[step];
}

// The chain in one call.  Frames go through in waves of `in_flight`; a wave runs its steps one after the other through stitch_group with
// step i's plan (run_lanes' lanes and groups), R of step i + 1 = the composite of step i, which ping-pongs between two internal planes
// per frame in flight (or lies in the caller's buffer, device form).  Every frame is verified against the rig's maps before any solve.
namespace {
// one step of one wave: `count` frames, arrays indexed by the frame's place in the wave
int rig_wave_step(pf_ctx* c, const pf_rig_plan* rig, int i, int count, const uint8_t* const* dl, const uint8_t* const* dr, uint8_t* const* dout, int cols, int rows,
                  int max_pct, int in_flight, const char* what) {
  std::vector<unsigned> diff(count, 0u);
  if (int e = run_lanes(c, count, in_flight, cols, rows, 3, what, [&](pf_ctx* lane, int first, int cnt) {
        return stitch_group(lane, first, cnt, dl, dr, cols, rows, max_pct, dout, rig->steps[i], diff.data());
      })) return e;
  for (int k = 0; k < count; ++k)
    if (diff[k]) return fail(c, PF_ERR_DEVICE, "%s: internal error: step %d's match found %u pixels off the plan in a frame that passed the rig's verification", what, i + 1, diff[k]);
  return 0;
}
}  // namespace

int pf_rig_stitch_batch(pf_ctx* c, const pf_rig_plan* rig, int n_frames, const uint8_t* const* top, const uint8_t* const* l, int cols, int rows, size_t step,
                        int max_pct, uint8_t* const* out, size_t ostep, int in_flight) {
  const char* const what = "pf_rig_stitch_batch";
  if (int e = use(c)) return e;
  c->vis_step_valid = false;   // lane 0 solves in this context's arena
  if (n_frames < 0 || !top || !l) return fail(c, PF_ERR_ARG, "bad argument");
  if (int e = check_rig(c, rig, cols, rows, what)) return e;
  if (n_frames == 0) return 0;
  const int ns = rig->n_steps;
  for (int k = 0; k < n_frames; ++k) {
    if (!top[k]) return fail(c, PF_ERR_ARG, "null pointer (frame %d)", k);
    for (int i = 0; i < ns; ++i) if (!l[size_t(k) * ns + i]) return fail(c, PF_ERR_ARG, "null pointer (frame %d, step %d)", k, i + 1);
  }
  if (int e = check_stitch_canvas(c, cols, rows, max_pct)) return e;
  if (step < size_t(cols) * 4 || (out && ostep < size_t(cols) * 4)) return fail(c, PF_ERR_ARG, "row step too small");
  const int W = clamp_in_flight(in_flight, n_frames), nwaves = (n_frames + W - 1) / W;
  const size_t n = size_t(cols) * rows, rb = size_t(cols) * 4;
  // per frame in flight: the n + 1 inputs -- two sets of them where the call has several waves, wave wv in set wv & 1 -- and two composites
  const int nsets = nwaves > 1 ? 2 : 1;
  const size_t set_len = size_t(W) * (ns + 1);
  std::vector<const uint8_t*> in(nsets * set_len);
  std::vector<uint8_t*> comp(size_t(W) * 2);
  for (int w = 0; w < nsets * W; ++w)
    for (int j = 0; j <= ns; ++j) if (!(in[size_t(w) * (ns + 1) + j] = rig_slot(c, "in", w, j, n * 4))) return PF_ERR_NOMEM;
  for (int w = 0; w < W; ++w)
    for (int j = 0; j < 2; ++j) if (!(comp[w * 2 + j] = rig_slot(c, "c", w, j, n * 4))) return PF_ERR_NOMEM;
  const uint8_t** tbl = (const uint8_t**)ensure(c, "rg_tbl", in.size() * sizeof(void*));
  if (!tbl) return PF_ERR_NOMEM;
  if (int e = rig_diff_words(c, size_t(n_frames) * ns)) return e;
  auto upload_wave = [&](int wv) -> int {
    const int first = wv * W, count = std::min(W, n_frames - first);
    const uint8_t* const* slot = in.data() + (wv & 1) * set_len;
    for (int w = 0; w < count; ++w)
      for (int j = 0; j <= ns; ++j) {
        const uint8_t* src = j == 0 ? top[first + w] : l[size_t(first + w) * ns + j - 1];
        if (int e = up2d(c, (void*)slot[size_t(w) * (ns + 1) + j], rb, src, step, rb, rows)) return e;
      }
    return 0;
  };
  // The overlapped form of a later wave's second upload: while wave wv - 1 computes, a host thread of its own copies wave wv (>= 2) into
  // the set wave wv - 2 has left, on the copy stream.  (A thread, because the copy of a pageable source blocks its caller while it is
  // staged: issued from the calling thread it would hold back the launches it is meant to run beside.)
  struct Prefetch {
    std::thread th; hipError_t err = hipSuccess;
    int join() { if (th.joinable()) th.join(); return err == hipSuccess ? 0 : 1; }
    ~Prefetch() { if (th.joinable()) th.join(); }
  } pre;
  auto prefetch_wave = [&](int wv) {
    pre.err = hipSuccess;
    pre.th = std::thread([&, wv]() {
      const int first = wv * W, count = std::min(W, n_frames - first);
      const uint8_t* const* slot = in.data() + (wv & 1) * set_len;
      hipError_t e = hipSetDevice(c->device);
      for (int w = 0; w < count && e == hipSuccess; ++w)
        for (int j = 0; j <= ns && e == hipSuccess; ++j) {
          const uint8_t* src = j == 0 ? top[first + w] : l[size_t(first + w) * ns + j - 1];
          void* dst = (void*)slot[size_t(w) * (ns + 1) + j];
          e = step == rb ? hipMemcpyAsync(dst, src, rb * size_t(rows), hipMemcpyHostToDevice, c->s_copy)
                         : hipMemcpy2DAsync(dst, rb, src, step, rb, rows, hipMemcpyHostToDevice, c->s_copy);
        }
      if (e == hipSuccess) e = hipStreamSynchronize(c->s_copy);
      pre.err = e;
    });
  };
  const bool overlap = c->rig_overlap_uploads && nwaves > 2;
  if (overlap && !c->s_copy) HIPCHK(c, hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking));
  {
    // verification: every wave's images go through its set of slots and one verifying launch, the last wave first, so that waves 0 and 1
    // are resident when the solves begin (a call of up to two waves uploads nothing twice)
    CallGuard guard_(c);
    HIPCHK(c, hipMemcpyAsync(tbl, in.data(), in.size() * sizeof(void*), hipMemcpyHostToDevice, c->s_main));
    for (int wv = nwaves - 1; wv >= 0; --wv) {
      const int first = wv * W, count = std::min(W, n_frames - first);
      if (int e = upload_wave(wv)) return e;
      PROF(c, c->s_main, "rig_verify");
      launch_rig_maps_verify(c->s_main, tbl + (wv & 1) * set_len, true, rig_maps(rig), ns, count, cols, rows, c->d_rig_diff + size_t(first) * ns);
    }
    HIPCHK(c, hipGetLastError());
    if (int e = finish(c)) return e;
  }
  if (int e = report_rig_diff(c, what, n_frames, ns)) return e;   // nothing is solved, nothing downloaded
  std::vector<const uint8_t*> dl(W), dr(W);
  std::vector<uint8_t*> dout(W);
  for (int wv = 0; wv < nwaves; ++wv) {
    const int first = wv * W, count = std::min(W, n_frames - first);
    if (wv > 1) {   // into the set wave wv - 2 has left
      if (overlap) {
        if (pre.join()) return fail(c, PF_ERR_DEVICE, "%s: the upload of wave %d beside wave %d's compute failed: %s", what, wv, wv - 1, hipGetErrorString(pre.err));
      } else {
        CallGuard guard_(c);
        if (int e = upload_wave(wv)) return e;
        if (int e = finish(c)) return e;   // the lanes' streams start from complete inputs
      }
    }
    if (overlap && wv >= 1 && wv + 1 < nwaves) prefetch_wave(wv + 1);
    const uint8_t* const* slot = in.data() + (wv & 1) * set_len;
    for (int i = 0; i < ns; ++i) {
      for (int w = 0; w < count; ++w) {
        dl[w] = slot[size_t(w) * (ns + 1) + i + 1];
        dr[w] = i == 0 ? slot[size_t(w) * (ns + 1)] : comp[w * 2 + ((i - 1) & 1)];
        dout[w] = comp[w * 2 + (i & 1)];
      }
      if (int e = rig_wave_step(c, rig, i, count, dl.data(), dr.data(), dout.data(), cols, rows, max_pct, in_flight, what)) return e;
      bool any = false;
      for (int w = 0; out && w < count; ++w) any = any || out[size_t(first + w) * ns + i];
      if (!any) continue;
      CallGuard guard_(c);
      for (int w = 0; w < count; ++w)
        if (uint8_t* o = out[size_t(first + w) * ns + i]) if (int e = down2d(c, o, ostep, dout[w], rb, rb, rows)) return e;
      HIPCHK(c, hipGetLastError());
      if (int e = finish(c)) return e;
    }
  }
  return 0;
}

int pf_rig_stitch_batch_dev(pf_ctx* c, const pf_rig_plan* rig, int n_frames, const uint8_t* const* d_top, const uint8_t* const* d_l, int cols, int rows,
                            int max_pct, uint8_t* const* d_out, int in_flight) {
  const char* const what = "pf_rig_stitch_batch_dev";
  if (int e = use(c)) return e;
  c->vis_step_valid = false;
  if (n_frames < 0 || !d_top || !d_l || !d_out) return fail(c, PF_ERR_ARG, "bad argument");
  if (int e = check_rig(c, rig, cols, rows, what)) return e;
  if (n_frames == 0) return 0;
  const int ns = rig->n_steps;
  if (int e = check_stitch_canvas(c, cols, rows, max_pct)) return e;
  const size_t n = size_t(cols) * rows, bytes = n * 4;
  std::vector<const uint8_t*> img(size_t(n_frames) * (ns + 1));   // the verifying launch's table: frame-major (top, L_1 .. L_n)
  std::vector<uint8_t*> outs;                                     // the caller's composites
  for (int k = 0; k < n_frames; ++k) {
    if (!d_top[k]) return fail(c, PF_ERR_ARG, "null device pointer (frame %d)", k);
    img[size_t(k) * (ns + 1)] = d_top[k];
    for (int i = 0; i < ns; ++i) {
      if (!d_l[size_t(k) * ns + i]) return fail(c, PF_ERR_ARG, "null device pointer (frame %d, step %d)", k, i + 1);
      img[size_t(k) * (ns + 1) + i + 1] = d_l[size_t(k) * ns + i];
      if (uint8_t* o = d_out[size_t(k) * ns + i]) outs.push_back(o);
    }
    if (!d_out[size_t(k) * ns + ns - 1]) return fail(c, PF_ERR_ARG, "frame %d: the last step's d_out must not be NULL", k);
  }
  if (int e = check_dev_align(c, what, "image", img.data(), img.size())) return e;
  if (int e = check_dev_align(c, what, "d_out", outs.data(), outs.size())) return e;
  // a composite is written while inputs of the call are still read: no aliasing (the rules of pf_stitch_step_batch_dev)
  for (size_t a = 0; a < outs.size(); ++a) {
    for (size_t j = 0; j < img.size(); ++j)
      if (overlaps(outs[a], img[j], bytes)) return fail(c, PF_ERR_ARG, "a d_out of the call overlaps an input of the call (frame %d)", (int)(j / (ns + 1)));
    for (size_t b = a + 1; b < outs.size(); ++b)
      if (overlaps(outs[a], outs[b], bytes)) return fail(c, PF_ERR_ARG, "two d_out entries of the call overlap");
  }
  const int W = clamp_in_flight(in_flight, n_frames), nwaves = (n_frames + W - 1) / W;
  std::vector<uint8_t*> comp(size_t(W) * 2);
  for (int w = 0; w < W; ++w)
    for (int j = 0; j < 2; ++j) if (!(comp[w * 2 + j] = rig_slot(c, "c", w, j, bytes))) return PF_ERR_NOMEM;
  const uint8_t** tbl = (const uint8_t**)ensure(c, "rg_tbl", img.size() * sizeof(void*));
  if (!tbl) return PF_ERR_NOMEM;
  if (int e = rig_diff_words(c, size_t(n_frames) * ns)) return e;
  {
    CallGuard guard_(c);
    HIPCHK(c, hipMemcpyAsync(tbl, img.data(), img.size() * sizeof(void*), hipMemcpyHostToDevice, c->s_main));
    const bool vec = all_aligned16(img.data(), img.size());
    for (int first = 0; first < n_frames; first += 32768) {   // (one launch for any call below the grid's z limit)
      PROF(c, c->s_main, "rig_verify");
      launch_rig_maps_verify(c->s_main, tbl + size_t(first) * (ns + 1), vec, rig_maps(rig), ns, std::min(32768, n_frames - first), cols, rows,
                             c->d_rig_diff + size_t(first) * ns);
    }
    HIPCHK(c, hipGetLastError());
    if (int e = finish(c)) return e;
  }
  if (report_rig_diff(c, what, n_frames, ns)) {
    // the call fails as a whole before any solve; the caller's buffers are cleared, as the planned device form clears them
    const std::string msg = c->err;
    CallGuard guard_(c);
    for (uint8_t* o : outs) HIPCHK(c, hipMemsetAsync(o, 0, bytes, c->s_main));
    if (int e = finish(c)) return e;
    return fail(c, PF_ERR_ARG, "%s", msg.c_str());
  }
  std::vector<const uint8_t*> dl(W), dr(W);
  std::vector<uint8_t*> dout(W);
  for (int wv = 0; wv < nwaves; ++wv) {
    const int first = wv * W, count = std::min(W, n_frames - first);
    std::vector<int> tog(count, 0);
    for (int i = 0; i < ns; ++i) {
      for (int w = 0; w < count; ++w) {
        const size_t k = size_t(first + w);
        dl[w] = d_l[k * ns + i];
        dr[w] = i == 0 ? d_top[k] : dout[w];   // the previous step's composite, wherever it went
        uint8_t* o = d_out[k * ns + i];
        if (!o) { o = comp[w * 2 + tog[w]]; tog[w] ^= 1; }   // never the plane the previous step wrote
        dout[w] = o;
      }
      if (int e = rig_wave_step(c, rig, i, count, dl.data(), dr.data(), dout.data(), cols, rows, max_pct, in_flight, what)) return e;
    }
  }
  return 0;
}
int pf_rig_set_upload_overlap(pf_ctx* c, int on) {
  if (!c) return fail(nullptr, PF_ERR_ARG, "null context");
  c->rig_overlap_uploads = on != 0;
  return 0;
}
int pf_rig_stitch(pf_ctx* c, const pf_rig_plan* rig, const uint8_t* top, const uint8_t* const* l, int cols, int rows, size_t step, int max_pct, uint8_t* const* out,
                  size_t ostep) {
  return pf_rig_stitch_batch(c, rig, 1, top ? &top : nullptr, l, cols, rows, step, max_pct, out, ostep, 1);
}
int pf_rig_stitch_dev(pf_ctx* c, const pf_rig_plan* rig, const uint8_t* d_top, const uint8_t* const* d_l, int cols, int rows, int max_pct, uint8_t* const* d_out) {
  return pf_rig_stitch_batch_dev(c, rig, 1, d_top ? &d_top : nullptr, d_l, cols, rows, max_pct, d_out, 1);
}
