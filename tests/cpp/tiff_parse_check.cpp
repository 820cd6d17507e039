// csrc/tiff_parse.hpp under the address and undefined-behaviour sanitizers, against tools/image_io.hpp read_tiff as the behaviour model.
//   * every file truncated at every length up to the end of its IFD and strip tables: a clean refusal;
//   * IFDs with hostile counts and offsets (an offset past the end, a count of 2^32 - 1, an IFD that points at itself or at the last
//     byte, 65535 entries, a field without values, strips past the file): a clean refusal, each buffer allocated at its exact size;
//   * every file read_tiff accepts gets the same geometry from the parser, every file read_tiff refuses is refused, and the parser's
//     two extra refusals (FillOrder 2, a strip outside the file -- which read_tiff meets only when it decodes) are the only differences.
// Built and run by tests/test_tiff_parse.py:  g++ -std=c++17 -fsanitize=address,undefined tests/cpp/tiff_parse_check.cpp -lz
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include <functional>
#include <memory>

#include "../../panorama-opticalflow_amd/csrc/tiff_parse.hpp"
#include "../../panorama-opticalflow_amd/tools/image_io.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                                    \
  do {                                                                                 \
    if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

struct Tag { unsigned tag, type; std::vector<unsigned> v; long count = -1 /* -1: v.size() */; long field = -1 /* >= 0: the raw value / offset field */; };
struct Spec {
  bool le = true;
  unsigned w = 5, h = 7, spp = 3, rps = 2, bps = 8, comp = 1, photo = 2, planar = 1;
  long ifd_at = -1;        // >= 0: the header's IFD offset, whatever lies there
  long n_entries = -1;     // >= 0: the IFD's entry count as written
  std::function<void(std::vector<Tag>&)> edit;   // before the layout: may add fields or resize their arrays
  std::function<void(std::vector<Tag>&)> late;   // after the strip tables are filled in: values, counts and offset fields only
};

static void put(std::vector<uint8_t>& b, bool le, unsigned v, int n) {
  for (int i = 0; i < n; ++i) b.push_back((uint8_t)(v >> 8 * (le ? i : n - 1 - i)));
}
// header, IFD, the fields' arrays, then the pixels; *tables_end = where the pixels begin
static std::vector<uint8_t> build(const Spec& s, size_t* tables_end = nullptr) {
  const unsigned rps = s.rps ? s.rps : 1, nstrips = (unsigned)((uint64_t(s.h) + rps - 1) / rps);
  std::vector<Tag> tags = {{256, 4, {s.w}}, {257, 4, {s.h}}, {258, 3, std::vector<unsigned>(s.spp, s.bps)}, {259, 3, {s.comp}}, {262, 3, {s.photo}},
                           {273, 4, std::vector<unsigned>(nstrips, 0)}, {277, 3, {s.spp}}, {278, 4, {s.rps}}, {279, 4, std::vector<unsigned>(nstrips, 0)}, {284, 3, {s.planar}}};
  const size_t row = size_t(s.w) * s.spp * (s.bps / 8 ? s.bps / 8 : 1);
  auto sz = [](const Tag& t) { return size_t(t.type == 3 ? 2 : t.type == 4 ? 4 : 1) * t.v.size(); };
  if (s.edit) s.edit(tags);
  {
    size_t at = 8 + 2 + 12 * tags.size() + 4;
    for (const Tag& t : tags) if (sz(t) > 4) at += sz(t) + (sz(t) & 1);
    for (Tag& t : tags)   // (a table an edit resized keeps the edit's values)
      for (unsigned k = 0; k < nstrips && (t.tag == 273 || t.tag == 279) && t.v.size() == nstrips; ++k)
        t.v[k] = t.tag == 273 ? (unsigned)(at + size_t(k) * rps * row) : (unsigned)(std::min(rps, s.h - k * rps) * row);
  }
  if (s.late) s.late(tags);
  std::vector<uint8_t> b = {uint8_t(s.le ? 'I' : 'M'), uint8_t(s.le ? 'I' : 'M')};
  put(b, s.le, 42, 2); put(b, s.le, s.ifd_at >= 0 ? (unsigned)s.ifd_at : 8, 4);
  put(b, s.le, s.n_entries >= 0 ? (unsigned)s.n_entries : (unsigned)tags.size(), 2);
  size_t ext = 8 + 2 + 12 * tags.size() + 4;
  std::vector<uint8_t> arrays;
  for (const Tag& t : tags) {
    put(b, s.le, t.tag, 2); put(b, s.le, t.type, 2); put(b, s.le, t.count >= 0 ? (unsigned)t.count : (unsigned)t.v.size(), 4);
    const int es = t.type == 3 ? 2 : t.type == 4 ? 4 : 1;
    if (t.field >= 0) put(b, s.le, (unsigned)t.field, 4);
    else if (sz(t) > 4) {
      put(b, s.le, (unsigned)(ext + arrays.size()), 4);
      for (unsigned v : t.v) put(arrays, s.le, v, es);
      if (arrays.size() & 1) arrays.push_back(0);
    } else {
      std::vector<uint8_t> f;
      for (unsigned v : t.v) put(f, s.le, v, es);
      f.resize(4, 0);
      b.insert(b.end(), f.begin(), f.end());
    }
  }
  put(b, s.le, 0, 4);
  b.insert(b.end(), arrays.begin(), arrays.end());
  if (tables_end) *tables_end = b.size();
  for (size_t i = 0; i < size_t(s.h) * row; ++i) b.push_back((uint8_t)(i * 37 + 11));
  return b;
}

// the parser on a heap block of exactly n bytes
static bool parse_exact(const uint8_t* p, size_t n, tiff_parse::Info* f, std::string* why) {
  std::unique_ptr<uint8_t[]> blk(new uint8_t[n ? n : 1]);
  if (n) memcpy(blk.get(), p, n);
  return tiff_parse::parse(n ? blk.get() : blk.get(), n, f, why);
}

static bool model_reads(const std::vector<uint8_t>& b, int* cols, int* rows, std::string* why) {
  char path[] = "/tmp/tiff_parse_check_XXXXXX.tif";
  const int fd = mkstemps(path, 4);
  if (fd < 0 || write(fd, b.data(), b.size()) != (ssize_t)b.size()) { printf("cannot write %s\n", path); exit(2); }
  close(fd);
  bool ok = true;
  try { const panocv::Mat m = pano_io::read_tiff(path); *cols = m.cols; *rows = m.rows; }
  catch (const util::VrCamException& e) { ok = false; *why = e.what(); }
  unlink(path);
  return ok;
}

static void refused(const char* what, const Spec& s) {
  const std::vector<uint8_t> b = build(s);
  tiff_parse::Info f; std::string why;
  const bool ok = parse_exact(b.data(), b.size(), &f, &why);
  CHECK(!ok && !why.empty());
  printf("  %-34s %s\n", what, ok ? "ACCEPTED" : why.c_str());
}

// `extra`: refused by the parser although read_tiff takes it (the parser's added checks)
static void agree(const char* what, const Spec& s, bool extra = false) {
  const std::vector<uint8_t> b = build(s);
  tiff_parse::Info f; std::string why, mwhy;
  int cols = 0, rows = 0;
  const bool ok = parse_exact(b.data(), b.size(), &f, &why), mok = model_reads(b, &cols, &rows, &mwhy);
  if (extra) CHECK(!ok && mok);
  else CHECK(ok == mok);
  if (ok && mok) {
    CHECK((int)f.cols == cols && (int)f.rows == rows && f.samples == s.spp && f.big_endian == !s.le && f.compression == s.comp);
    CHECK(f.rows_per_strip == std::min(s.rps, s.h) && f.n_strips() == (s.h + f.rows_per_strip - 1) / f.rows_per_strip);
    for (size_t k = 0; k < f.n_strips(); ++k) CHECK(uint64_t(f.offsets[k]) + f.counts[k] <= b.size() && f.counts[k] == f.strip_bytes(k));
  }
  printf("  %-34s parser: %s | read_tiff: %s\n", what, ok ? "ok" : why.c_str(), mok ? "ok" : mwhy.c_str());
}

static Tag* find(std::vector<Tag>& tags, unsigned tag) { for (Tag& t : tags) if (t.tag == tag) return &t; return nullptr; }

int main() {
  // ---- truncation at every length up to the end of the tables (and a little into the pixels)
  for (int variant = 0; variant < 4; ++variant) {
    Spec s; s.le = variant & 1; s.spp = variant & 2 ? 4 : 3; s.rps = variant & 2 ? 1 : 2;
    size_t tables_end = 0;
    const std::vector<uint8_t> b = build(s, &tables_end);
    tiff_parse::Info f; std::string why;
    CHECK(parse_exact(b.data(), b.size(), &f, &why));
    for (size_t n = 0; n <= tables_end + 3; ++n) { why.clear(); CHECK(!parse_exact(b.data(), n, &f, &why) && !why.empty()); }
    CHECK(!parse_exact(b.data(), b.size() - 1, &f, &why));   // the last strip's last byte
    printf("  truncation, variant %d: %zu lengths refused\n", variant, tables_end + 5);
  }
  // ---- hostile IFDs
  printf("hostile IFDs\n");
  { Spec s; s.late = [](std::vector<Tag>& t) { find(t, 273)->count = 0xffffffffl; }; refused("StripOffsets count 2^32 - 1", s); }
  { Spec s; s.late = [](std::vector<Tag>& t) { find(t, 279)->count = 0x40000000l; }; refused("StripByteCounts count 2^30", s); }
  { Spec s; s.late = [](std::vector<Tag>& t) { find(t, 273)->field = 0xfffffff0l; }; refused("StripOffsets array past the end", s); }
  { Spec s; s.late = [](std::vector<Tag>& t) { find(t, 273)->v[1] = 0xfffffffeu; }; refused("a strip offset past the end", s); }
  { Spec s; s.late = [](std::vector<Tag>& t) { find(t, 279)->v[3] = 0xffffffffu; }; refused("a strip count of 2^32 - 1", s); }
  { Spec s; s.late = [](std::vector<Tag>& t) { find(t, 279)->v[3] += 1; }; refused("last strip one byte past the file", s); }
  { Spec s; s.ifd_at = 4; refused("IFD that points at itself", s); }
  { Spec s; s.ifd_at = 2; refused("IFD inside the header", s); }
  { Spec s; s.ifd_at = 0xffffffffl; refused("IFD offset 2^32 - 1", s); }
  { Spec s; s.n_entries = 65535; refused("65535 entries", s); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { find(t, 256)->count = 0; }; refused("ImageWidth without a value", s); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { find(t, 256)->type = 5; }; refused("ImageWidth as a RATIONAL", s); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { find(t, 258)->count = 0xffffffffl; }; refused("BitsPerSample count 2^32 - 1", s); }
  { Spec s;   // (the builder appends w * h * spp pixel bytes: a small file that states a large size)
    s.edit = [](std::vector<Tag>& t) { find(t, 273)->v.assign(1, 8); find(t, 279)->v.assign(1, 16); };
    s.late = [](std::vector<Tag>& t) { find(t, 256)->v[0] = 0x7fffffffu; find(t, 257)->v[0] = 0x7fffffffu; find(t, 278)->v[0] = 0x7fffffffu; };
    refused("2^31 x 2^31 pixels", s); }
  { tiff_parse::Info f; std::string why; CHECK(!tiff_parse::parse(nullptr, 0, &f, &why)); const uint8_t two[2] = {'I', 'I'}; CHECK(!parse_exact(two, 2, &f, &why)); }
  // ---- agreement with read_tiff
  printf("agreement with read_tiff\n");
  for (int le = 0; le < 2; ++le)
    for (unsigned spp : {3u, 4u})
      for (unsigned rps : {1u, 2u, 7u, 1000u, 0xffffffffu}) { Spec s; s.le = le; s.spp = spp; s.rps = rps; agree("strips", s); }
  { Spec s; s.w = 1; s.h = 1; agree("1 x 1", s); }
  { Spec s; s.bps = 16; agree("16-bit", s); }
  { Spec s; s.photo = 3; agree("palette", s); }
  { Spec s; s.planar = 2; agree("planar", s); }
  { Spec s; s.spp = 1; agree("one sample per pixel", s); }
  { Spec s; s.rps = 0; agree("RowsPerStrip 0", s); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { t.push_back({322, 4, {16}}); t.push_back({324, 4, {8}}); }; agree("tiled", s); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { find(t, 273)->v.pop_back(); }; agree("a strip offset missing", s); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { find(t, 279)->v.push_back(1); }; agree("a strip count too many", s); }
  { Spec s; s.late = [](std::vector<Tag>& t) { find(t, 278)->v[0] = 3; }; agree("RowsPerStrip against the table", s); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { t.push_back({317, 3, {2}}); }; agree("predictor 2", s); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { find(t, 256)->type = 5; }; agree("a RATIONAL field", s); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { t.push_back({266, 3, {2}}); }; agree("FillOrder 2", s, true); }
  { Spec s; s.edit = [](std::vector<Tag>& t) { t.push_back({266, 3, {1}}); }; agree("FillOrder 1", s); }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
