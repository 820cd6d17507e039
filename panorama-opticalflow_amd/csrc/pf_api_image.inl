// Part of pf_api.hip (one translation unit): what the file-and-image entry points (PNG, TIFF, JPEG, resize, reproject, lens) share.
// Where a stitch result sits in HBM, the checks of a list of device images, a host BGRA image's way into and out of an arena slot, and
// a host-made table kept resident in one.  Helpers only: no entry point lives here, and a new format uses these, not a neighbour's copy.
}  // extern "C"
namespace {

struct DevImage { const uint8_t* p = nullptr; int cols = 0, rows = 0; };

// The composite a stitch call left in HBM, read in place.  frame == null: the last pf_stitch_step / pf_stitch_step_planned's
// ("ch_final", what r == NULL chains on); else frame slot *frame of the last host-form pf_stitch_step_batch* call ("sb_fin<frame>").
int resident_result(pf_ctx* c, const char* fn, const int* frame, DevImage* out) {
  if (!frame) {
    if (c->chain_cols <= 0 || c->chain_rows <= 0 || !c->bufs["ch_final"].p) return fail(c, PF_ERR_ARG, "%s: no stitch step result in HBM", fn);
    out->p = (const uint8_t*)c->bufs["ch_final"].p; out->cols = c->chain_cols; out->rows = c->chain_rows;
    return 0;
  }
  if (*frame < 0 || *frame >= c->sb_frames) return fail(c, PF_ERR_ARG, "%s: no batch result in frame slot %d (%d slots hold one)", fn, *frame, c->sb_frames);
  char name[32];
  snprintf(name, sizeof name, "sb_fin%d", *frame);
  out->p = (const uint8_t*)c->bufs[name].p; out->cols = c->sb_cols; out->rows = c->sb_rows;
  if (!out->p) return fail(c, PF_ERR_ARG, "%s: no batch result in frame slot %d", fn, *frame);
  return 0;
}

// (ranges_overlap: pf_api_ctx.inl, beside the checks of the core device forms)
// n device images of src_bytes each and, where d_dst is given, their n destinations of dst_bytes each: none null, all 4-byte aligned,
// no destination inside any source.  The refusals speak the family's words ("resize: destination 1 overlaps source 0").
int check_dev_images(pf_ctx* c, const char* family, int n, const uint8_t* const* d_src, size_t src_bytes, uint8_t* const* d_dst = nullptr, size_t dst_bytes = 0,
                     const char* dst_noun = "destination", const char* src_noun = "source") {
  for (int k = 0; k < n; ++k) {
    if (!d_src[k] || (d_dst && !d_dst[k])) return fail(c, PF_ERR_ARG, "null pointer (image %d)", k);
    if ((reinterpret_cast<uintptr_t>(d_src[k]) | (d_dst ? reinterpret_cast<uintptr_t>(d_dst[k]) : 0)) & 3) return fail(c, PF_ERR_ARG, "%s: device image %d is not 4-byte aligned", family, k);
  }
  for (int k = 0; d_dst && k < n; ++k)
    for (int q = 0; q < n; ++q)
      if (ranges_overlap(d_dst[k], dst_bytes, d_src[q], src_bytes)) return fail(c, PF_ERR_ARG, "%s: %s %d overlaps %s %d", family, dst_noun, k, src_noun, q);
  return 0;
}

// bytes from the first to the last pixel of a host BGRA image whose rows are `step` apart
size_t bgra_span(int cols, int rows, size_t step) { return size_t(rows - 1) * step + size_t(cols) * 4; }

// a host BGRA image, rows `step` apart, packed into the arena slot `slot` (enqueued on s_main)
int upload_bgra(pf_ctx* c, const char* slot, const uint8_t* host, size_t step, int cols, int rows, const uint8_t** d_out) {
  void* d = ensure(c, slot, size_t(cols) * rows * 4);
  if (!d) return PF_ERR_NOMEM;
  *d_out = (const uint8_t*)d;
  return up_plane(c, d, host, step, cols, rows, 4);
}
// (... and a packed device image back into one: down_plane, pf_api_life.inl; the caller drains)

// A table the host makes, resident in the arena slot `slot`: fill(host) writes its `bytes` bytes, and only when the slot does not hold
// them already.  It does not when the slot moved, when it grew (a slot that grew is a fresh allocation, wherever it landed) or when it
// holds another key's table.  The record is void while the copy is in flight, and the copy is drained because the host bytes are this
// frame's.  A hit enqueues nothing.
template <class Fill>
int resident_table(pf_ctx* c, const char* slot, pf_ctx::Resident& r, int k0, int k1, int k2, size_t bytes, Fill fill, const uint8_t** d_out) {
  uint8_t* d = (uint8_t*)ensure(c, slot, bytes);
  if (!d) return PF_ERR_NOMEM;
  const size_t cap = c->bufs[slot].cap;
  if (r.p != d || r.cap != cap || r.key[0] != k0 || r.key[1] != k1 || r.key[2] != k2) {
    r.p = nullptr;
    std::vector<uint8_t> host(bytes);
    fill(host.data());
    HIPCHK(c, hipMemcpyAsync(d, host.data(), bytes, hipMemcpyHostToDevice, c->s_main));
    HIPCHK(c, hipStreamSynchronize(c->s_main));
    r.p = d; r.cap = cap; r.key[0] = k0; r.key[1] = k1; r.key[2] = k2;
  }
  *d_out = d;
  return 0;
}

}  // namespace
extern "C" {
