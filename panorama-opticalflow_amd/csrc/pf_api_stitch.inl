// Part of pf_api.hip (one translation unit, split along its seams in round 5): Stitchtools: prepare / match / blend ramp / gather, the device-resident chain step and its prefetch, the batched step.  (Plans and the rig chain: pf_api_plan.inl.)

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

// The lone calls' planes: the subset `want` of the arena slots below, under the names pf_create pre-sizes, into frame 0 of p (what is not
// asked for stays null).  SP_CHAIN: the inputs and the composite are the chain's, which stay resident between steps, not the staging slots.
enum { SP_IN = 1, SP_MAP = 2, SP_OV = 4, SP_RAMP = 8, SP_MERGED = 16, SP_OUT = 32, SP_CHAIN = 64 };
static int stitch_planes(pf_ctx* c, int want, int cols, int rows, StitchPtrs& p) {
  const size_t n = size_t(cols) * rows;
  const bool chain = want & SP_CHAIN;
  bool ok = true;
  auto slot = [&](int bit, const char* name, size_t bytes) -> void* {
    if (!(want & bit)) return nullptr;
    void* d = ensure(c, name, bytes);
    ok = ok && d;
    return d;
  };
  p.L[0] = (uint8_t*)slot(SP_IN, chain ? "ch_l" : "h_img0", n * 4); p.R[0] = (uint8_t*)slot(SP_IN, chain ? "ch_r" : "h_img1", n * 4);
  p.map[0] = (uint8_t*)slot(SP_MAP, "st_map", n); p.ovL[0] = (uint8_t*)slot(SP_OV, "st_ovl", n * 4); p.ovR[0] = (uint8_t*)slot(SP_OV, "st_ovr", n * 4);
  p.blend[0] = (float*)slot(SP_RAMP, "st_blend", n * 4); p.md[0] = (float*)slot(SP_RAMP, "st_md", n * 4);
  p.merged[0] = (uint8_t*)slot(SP_MERGED, "st_merged", n * 4); p.out[0] = (uint8_t*)slot(SP_OUT, chain ? "ch_final" : "h_out", n * 4);
  return ok ? 0 : PF_ERR_NOMEM;
}
// a lone call's two input images into p.L / p.R (enqueued on s_main)
static int up_inputs(pf_ctx* c, const StitchPtrs& p, const uint8_t* l, const uint8_t* r, size_t step, int cols, int rows) {
  if (int e = up_plane(c, (void*)p.L[0], l, step, cols, rows, 4)) return e;
  return up_plane(c, (void*)p.R[0], r, step, cols, rows, 4);
}

int pf_stitch_prepare(pf_ctx* c, const uint8_t* l, const uint8_t* r, int cols, int rows, size_t step, uint8_t* map_out, size_t mstep, uint8_t* ovl,
                      uint8_t* ovr, float* blend_out, size_t bstep, float* merged_dis) {
  if (int e = use(c)) return e;
  CallGuard guard_(c);
  if (!l || !r) return fail(c, PF_ERR_ARG, "null pointer");
  if (int e = check_image(c, cols, rows)) return e;
  if (step < size_t(cols) * 4 || (map_out && mstep < size_t(cols)) || (blend_out && bstep < size_t(cols) * 4)) return fail(c, PF_ERR_ARG, "row step too small");
  StitchPtrs p{};
  if (int e = stitch_planes(c, SP_IN | SP_MAP | SP_OV | SP_RAMP, cols, rows, p)) return e;
  const RampGeom g = ramp_geom(cols, rows);
  RampWork w;
  if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w)) return e;
  hipStream_t sm = c->s_main;
  if (int e = up_inputs(c, p, l, r, step, cols, rows)) return e;
  { PROF(c, sm, "match_images"); launch_match_images(sm, p, 1, cols, rows); }
  const float* ramp = nullptr;
  if (int e = blend_ramp_dev(c, sm, p, 1, cols, rows, g, w, true, &ramp)) return e;
  if (map_out) if (int e = down_plane(c, map_out, mstep, p.map[0], cols, rows, 1)) return e;
  if (ovl) if (int e = down_plane(c, ovl, step, p.ovL[0], cols, rows, 4)) return e;
  if (ovr) if (int e = down_plane(c, ovr, step, p.ovR[0], cols, rows, 4)) return e;
  if (blend_out) if (int e = down_plane(c, blend_out, bstep, ramp, cols, rows, 4)) return e;
  if (merged_dis) if (int e = down_plane(c, merged_dis, size_t(cols) * 4, p.md[0], cols, rows, 4)) return e;
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
  StitchPtrs p{};
  if (int e = stitch_planes(c, SP_IN | SP_MAP | SP_OV, cols, rows, p)) return e;
  if (int e = up_inputs(c, p, l, r, step, cols, rows)) return e;
  { PROF(c, c->s_main, "match_images"); launch_match_images(c->s_main, p, 1, cols, rows); }
  if (map_out) if (int e = down_plane(c, map_out, mstep, p.map[0], cols, rows, 1)) return e;
  if (ovl) if (int e = down_plane(c, ovl, step, p.ovL[0], cols, rows, 4)) return e;
  if (ovr) if (int e = down_plane(c, ovr, step, p.ovR[0], cols, rows, 4)) return e;
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
  StitchPtrs p{};
  if (int e = stitch_planes(c, SP_MAP | SP_RAMP, cols, rows, p)) return e;
  const RampGeom g = ramp_geom(cols, rows);
  RampWork w;
  if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w)) return e;
  if (int e = up_plane(c, p.map[0], map, mstep, cols, rows, 1)) return e;
  const float* ramp = nullptr;
  if (int e = blend_ramp_dev(c, c->s_main, p, 1, cols, rows, g, w, true, &ramp)) return e;
  if (int e = down_plane(c, blend_out, bstep, ramp, cols, rows, 4)) return e;
  if (merged_dis) if (int e = down_plane(c, merged_dis, size_t(cols) * 4, p.md[0], cols, rows, 4)) return e;
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
  StitchPtrs p{};
  if (int e = stitch_planes(c, SP_IN | SP_MAP | SP_OV | SP_RAMP, cols, rows, p)) return e;
  hipStream_t sm = c->s_main;
  if (int e = up_inputs(c, p, l, r, step, cols, rows)) return e;
  { PROF(c, sm, "match_images"); launch_match_images(sm, p, 1, cols, rows); }
  { PROF(c, sm, "countblend"); launch_countblend(sm, p, 1, cols, rows); }
  if (int e = down_plane(c, raw_blend, bstep, p.blend[0], cols, rows, 4)) return e;
  if (merged_dis) if (int e = down_plane(c, merged_dis, size_t(cols) * 4, p.md[0], cols, rows, 4)) return e;
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
  StitchPtrs p{};
  if (int e = stitch_planes(c, SP_IN | SP_MERGED | SP_MAP | SP_OUT, cols, rows, p)) return e;
  if (int e = up_inputs(c, p, l, r, step, cols, rows)) return e;
  if (int e = up_plane(c, p.merged[0], merged, step, cols, rows, 4)) return e;
  if (int e = up_plane(c, p.map[0], map, mstep, cols, rows, 1)) return e;
  { PROF(c, c->s_main, "gather"); launch_gather(c->s_main, p, 1, cols, rows); }
  if (int e = down_plane(c, out, ostep, p.out[0], cols, rows, 4)) return e;
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

// (plan_is_live, pf_api_life.inl: no dereference before the context is found to list the handle)
static int check_plan(pf_ctx* c, const pf_stitch_plan* plan, int cols, int rows, const char* what) {
  if (!plan_is_live(c, plan)) return fail(c, PF_ERR_ARG, "%s: not a live stitch plan of this context", what);
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
  StitchPtrs p{};
  // a planned step needs neither a map nor ramp planes of its own
  if (int e = stitch_planes(c, SP_CHAIN | SP_IN | SP_OUT | SP_OV | SP_MERGED | (plan ? 0 : SP_MAP | SP_RAMP), cols, rows, p)) return e;
  if (plan) p.map[0] = plan->map;
  float* f0 = (float*)ensure(c, "nv_flow_l2r", n * 8); float* f1 = (float*)ensure(c, "nv_flow_r2l", n * 8);
  uint8_t* dnext = (uint8_t*)ensure(c, "ch_l_next", n * 4);
  if (!f0 || !f1 || !dnext) return PF_ERR_NOMEM;
  hipStream_t sm = c->s_main;
  const RampGeom g = ramp_geom(cols, rows);
  RampWork w;
  if (!plan) if (int e = ramp_planes(c, kRampLone, 1, cols, rows, g, p, w)) return e;
  // both prefetch records are one-shot: latched and cleared here, whatever this step does with them
  const pf_ctx::HostImage ready = c->ready, hint = c->hint;
  c->ready = pf_ctx::HostImage(); c->hint = pf_ctx::HostImage();
  if (ready.src == l && ready.cols == cols && ready.rows == rows && ready.step == step && ready.sig == host_image_sig(l, cols, rows, step)) {
    // this step's left image was uploaded while the previous step computed: the two buffers trade places (no copy; the old
    // "ch_l" is free -- the previous call drained every stream -- and receives the next prefetch)
    std::swap(c->bufs["ch_l"], c->bufs["ch_l_next"]);
    uint8_t* const freed = (uint8_t*)p.L[0];
    p.L[0] = dnext; dnext = freed;
  } else {
    if (int e = up_plane(c, (void*)p.L[0], l, step, cols, rows, 4)) return e;
  }
  if (r) { if (int e = up_plane(c, (void*)p.R[0], r, step, cols, rows, 4)) return e; }
  else {
    if (c->chain_cols != cols || c->chain_rows != rows) return fail(c, PF_ERR_ARG, "%s: no previous result of this size to chain on", what);
    HIPCHK(c, hipMemcpyAsync((void*)p.R[0], p.out[0], n * 4, hipMemcpyDeviceToDevice, sm));
  }
  if (!c->s_copy) HIPCHK(c, hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking));
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
      HIPCHK(c, up_plane_on(c->s_copy, dnext, hint.src, hint.step, cols, rows, 4));
      HIPCHK(c, hipStreamSynchronize(c->s_copy));
      c->ready = hint;
      c->ready.sig = host_image_sig(hint.src, cols, rows, hint.step);
    }
    return 0;
  };
  if (!plan) {
    if (out) if (int e = down_plane(c, out, ostep, p.out[0], cols, rows, 4)) return e;
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
    if (out) if (int e = down_plane(c, out, ostep, p.out[0], cols, rows, 4)) return e;
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

// A device form fails as a whole: no composite is delivered.  The caller's `count` buffers of `bytes` each are cleared and the call fails
// with `code` and the message it had on entry (the first error's).
static int clear_outputs(pf_ctx* c, int code, uint8_t* const* d_out, size_t count, size_t bytes) {
  const std::string msg = c->err;
  CallGuard guard_(c);
  for (size_t k = 0; k < count; ++k) HIPCHK(c, hipMemsetAsync(d_out[k], 0, bytes, c->s_main));
  if (int e = finish(c)) return e;
  return fail(c, code, "%s", msg.c_str());
}

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
  std::vector<unsigned> diff(plan ? n_frames : 0, 0u);
  if (int e = run_lanes(c, n_frames, in_flight, cols, rows, 3, plan ? "pf_stitch_step_batch_planned" : "pf_stitch_step_batch", [&](pf_ctx* lane, int first, int count) {
        return stitch_group(lane, first, count, d_l, d_r, cols, rows, max_pct, d_out, plan, diff.data());
      })) return e;
  // a frame off the plan: the gathers have run, so the caller's buffers are cleared
  if (plan) if (int e = report_plan_diff(c, "pf_stitch_step_batch_planned_dev", diff.data(), n_frames)) return clear_outputs(c, e, d_out, n_frames, bytes);
  return 0;
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
      if (int e = up_plane(c, dl[k], l[k], step, cols, rows, 4)) return e;
      if (r && r[k]) { if (int e = up_plane(c, dr[k], r[k], step, cols, rows, 4)) return e; }
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
      if (out[k]) if (int e2 = down_plane(c, out[k], ostep, dfin[k], cols, rows, 4)) return e2;
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
