// TIFF header parsing for the device decoder (kernels_tiff.hip, pf_api_tiff.inl): the first IFD of a byte buffer -> a plain struct.
// Host code only, no HIP.  It accepts and refuses what tools/image_io.hpp read_tiff accepts and refuses -- 8-bit chunky RGB / RGBA strips;
// tiles, 16-bit, palette and planar files, an inconsistent strip table and images over 4e9 pixels are refused -- and adds two checks:
// every strip's [offset, offset + count) lies inside the file, and FillOrder 2 is refused.  Every number the file supplies is widened
// to 64 bits before it takes part in arithmetic and compared with the buffer's size before it is used as an index, so a hostile IFD (an
// offset past the end, a count of 2^32 - 1, an IFD that points at itself) gets a message and never a read outside the buffer.  Only the
// first IFD is read and nothing follows a "next IFD" link, so there is no loop a file could keep alive.
#ifndef PF_TIFF_PARSE_HPP_
#define PF_TIFF_PARSE_HPP_

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace tiff_parse {

struct Info {
  uint32_t cols = 0, rows = 0;
  uint32_t samples = 0;          // 3 (RGB) or 4 (RGBA)
  uint32_t compression = 1;      // 1 none, 5 LZW, 8 / 32946 deflate, 32773 PackBits
  uint32_t predictor = 1;        // 2 = horizontal differencing; any other value means none, as in read_tiff
  uint32_t rows_per_strip = 0;   // clamped to rows
  bool big_endian = false;
  std::vector<uint32_t> offsets, counts;   // one entry per strip, each [offset, offset + count) inside the buffer
  size_t n_strips() const { return offsets.size(); }
  uint32_t rows_in_strip(size_t s) const { const uint64_t left = uint64_t(rows) - uint64_t(s) * rows_per_strip; return (uint32_t)(left < rows_per_strip ? left : rows_per_strip); }
  uint64_t row_bytes() const { return uint64_t(cols) * samples; }
  uint64_t strip_bytes(size_t s) const { return uint64_t(rows_in_strip(s)) * row_bytes(); }
};

namespace detail {
struct Reader {
  const uint8_t* b; uint64_t n; bool le; std::string* err;
  bool have(uint64_t o, uint64_t len) const { return o <= n && len <= n - o; }
  bool u16(uint64_t o, uint32_t* v) const {
    if (!have(o, 2)) return trunc();
    *v = le ? uint32_t(b[o]) | (uint32_t(b[o + 1]) << 8) : (uint32_t(b[o]) << 8) | uint32_t(b[o + 1]);
    return true;
  }
  bool u32(uint64_t o, uint32_t* v) const {
    if (!have(o, 4)) return trunc();
    *v = le ? uint32_t(b[o]) | (uint32_t(b[o + 1]) << 8) | (uint32_t(b[o + 2]) << 16) | (uint32_t(b[o + 3]) << 24)
            : (uint32_t(b[o]) << 24) | (uint32_t(b[o + 1]) << 16) | (uint32_t(b[o + 2]) << 8) | uint32_t(b[o + 3]);
    return true;
  }
  bool trunc() const { *err = "truncated TIFF"; return false; }
  // the values of one IFD entry (BYTE, SHORT or LONG); `all` false: only the first one is wanted
  bool values(uint64_t entry, bool all, std::vector<uint32_t>* out) const {
    uint32_t type = 0, count = 0;
    if (!u16(entry + 2, &type) || !u32(entry + 4, &count)) return false;
    const uint64_t sz = type == 3 ? 2 : (type == 4 ? 4 : (type == 1 ? 1 : 0));
    if (!sz) { *err = "unsupported TIFF field type"; return false; }
    if (!count) { *err = "TIFF field without a value"; return false; }
    uint64_t off = entry + 8;
    if (sz * uint64_t(count) > 4) { uint32_t o = 0; if (!u32(entry + 8, &o)) return false; off = o; }
    if (!have(off, sz * uint64_t(count))) return trunc();   // the whole array, before anything is sized by `count`
    const uint64_t take = all ? count : 1;
    out->resize((size_t)take);
    for (uint64_t i = 0; i < take; ++i) {
      uint32_t v = 0;
      if (sz == 2) { if (!u16(off + 2 * i, &v)) return false; }
      else if (sz == 4) { if (!u32(off + 4 * i, &v)) return false; }
      else v = b[off + i];
      (*out)[(size_t)i] = v;
    }
    return true;
  }
};
}  // namespace detail

// false: *err says why.  `out` is only meaningful after true.
inline bool parse(const uint8_t* file, size_t bytes, Info* out, std::string* err) {
  std::string dummy;
  if (!err) err = &dummy;
  if (!file || bytes < 8 || !((file[0] == 'I' && file[1] == 'I') || (file[0] == 'M' && file[1] == 'M'))) { *err = "not a TIFF"; return false; }
  detail::Reader t{file, (uint64_t)bytes, file[0] == 'I', err};
  uint32_t magic = 0, ifd32 = 0, n = 0;
  if (!t.u16(2, &magic)) return false;
  if (magic != 42) { *err = "not a TIFF"; return false; }
  if (!t.u32(4, &ifd32)) return false;
  const uint64_t ifd = ifd32;
  if (!t.u16(ifd, &n)) return false;
  uint32_t w = 0, h = 0, spp = 1, comp = 1, photo = 2, rps = 0xffffffffu, planar = 1, pred = 1, bps = 8, fill = 1;
  std::vector<uint32_t> so, sc, one;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t e = ifd + 2 + 12 * uint64_t(i);
    uint32_t tag = 0;
    if (!t.u16(e, &tag)) return false;
    uint32_t* scalar = nullptr;
    switch (tag) {
      case 256: scalar = &w; break;      case 257: scalar = &h; break;
      case 258: scalar = &bps; break;    case 259: scalar = &comp; break;
      case 262: scalar = &photo; break;  case 266: scalar = &fill; break;
      case 277: scalar = &spp; break;    case 278: scalar = &rps; break;
      case 284: scalar = &planar; break; case 317: scalar = &pred; break;
      case 273: if (!t.values(e, true, &so)) return false; break;
      case 279: if (!t.values(e, true, &sc)) return false; break;
      case 322: case 324: *err = "tiled TIFF not supported"; return false;
      default: break;
    }
    if (scalar) { if (!t.values(e, false, &one)) return false; *scalar = one[0]; }
  }
  if (!w || !h || bps != 8 || planar != 1 || (spp != 3 && spp != 4) || photo != 2 || so.empty() || so.size() != sc.size()) {
    *err = "unsupported TIFF layout (need 8-bit chunky RGB/RGBA strips)"; return false;
  }
  if (fill != 1) { *err = "TIFF FillOrder 2 (bit-reversed bytes) is not supported"; return false; }
  if (rps > h) rps = h;
  if (rps == 0 || uint64_t(so.size()) != (uint64_t(h) + rps - 1) / rps) { *err = "inconsistent TIFF strip table (RowsPerStrip / StripOffsets)"; return false; }
  if ((double)w * (double)h > 4.0e9) { *err = "TIFF too large"; return false; }
  if (comp != 1 && comp != 5 && comp != 8 && comp != 32946 && comp != 32773) { *err = "unsupported TIFF compression"; return false; }
  for (size_t s = 0; s < so.size(); ++s)
    if (!t.have(so[s], sc[s])) { *err = "truncated TIFF: strip " + std::to_string(s) + " does not lie inside the file"; return false; }
  out->cols = w; out->rows = h; out->samples = spp; out->compression = comp; out->predictor = pred; out->rows_per_strip = rps;
  out->big_endian = !t.le; out->offsets.swap(so); out->counts.swap(sc);
  return true;
}

// what kernels_tiff.hip decodes: no compression, LZW and PackBits (deflate strips stay with the host reader), and strips whose decoded
// bytes fit the kernels' 32-bit positions
inline bool device_decodable(const Info& f) {
  if (f.compression != 1 && f.compression != 5 && f.compression != 32773) return false;
  return uint64_t(f.rows_per_strip) * f.row_bytes() < (uint64_t(1) << 31);
}

// the same with the decoder's inflate switch on (pf_tiff_set_inflate): deflate strips (8, and 32946 of older writers) join, under the
// same strip-size limit
inline bool device_decodable_with_inflate(const Info& f) {
  if (f.compression != 8 && f.compression != 32946) return device_decodable(f);
  return uint64_t(f.rows_per_strip) * f.row_bytes() < (uint64_t(1) << 31);
}

// LZW code geometry (TIFF flavour, early change).  Code j (j = 0 is the first code after a Clear, or the first code of the strip) is
// read while the table holds min(4096, 258 + max(0, j - 1)) entries; the width steps up after the codes that bring the table to 511,
// 1023 and 2047 entries, which are j = 253, 765 and 1789.  So the width and the bit offset are closed functions of j alone.
inline uint32_t lzw_code_width(uint64_t j) { return 9 + (j >= 254) + (j >= 766) + (j >= 1790); }
inline uint64_t lzw_code_bit_offset(uint64_t j) { return 9 * j + (j > 254 ? j - 254 : 0) + (j > 766 ? j - 766 : 0) + (j > 1790 ? j - 1790 : 0); }

}  // namespace tiff_parse
#endif
