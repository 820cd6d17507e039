// JPEG header parsing for the device decoder (kernels_jpegd.hip, pf_api_jpegd.inl): the markers up to the scan's first byte -> a plain
// struct.  Host code only, no HIP.  It accepts what DESIGN.md 8.10 lists -- baseline SOF0, 8-bit, grey or Y Cb Cr at 4:4:4 / 4:2:2 /
// 4:2:0, one interleaved scan, any restart interval -- and refuses everything else with a reason.  Every length the file supplies is
// widened to 64 bits and compared with the buffer before it indexes anything, and every loop consumes input or leaves.  The decode
// tables the kernels read (Tables: libjpeg's jpeg_make_d_derived_tbl, flattened) are derived here, in one copy: the kernels, the
// host-run test and the library all take them from this file.
#ifndef PF_JPEG_PARSE_HPP_
#define PF_JPEG_PARSE_HPP_

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

namespace jpeg_parse {

constexpr uint64_t kMaxSegment = uint64_t(1) << 28;   // bytes of entropy-coded data: the kernels' bit positions are 32-bit

// one Huffman table as the kernels walk it
struct DTab {
  int32_t maxcode[18];   // [l]: the largest code of length l, -1 where there is none; [17] ends every search
  int32_t valoff[17];    // [l]: index into vals of the first symbol of length l, less its code
  uint16_t look[256];    // the next 8 bits -> (length << 8) | symbol; 0: the code is longer than 8 bits
  uint8_t vals[256];
};

// everything the kernels need beyond the bytes: resolved per component, so no kernel follows a table id
struct Tables {
  DTab dc[3], ac[3];
  uint8_t quant[3][64];   // zigzag order, as in the file
};

struct Info {
  uint32_t cols = 0, rows = 0;
  int ncomp = 0;           // 1 (grey) or 3 (Y Cb Cr)
  int hs = 1, vs = 1;      // luma sampling; chroma is 1 x 1
  uint32_t restart = 0;    // MCUs per interval, 0: none
  uint64_t begin = 0, end = 0;   // the entropy segment [begin, end): end is EOI's 0xFF
  uint32_t mcu_cols() const { return (cols + 8 * hs - 1) / (8 * hs); }
  uint32_t mcu_rows() const { return (rows + 8 * vs - 1) / (8 * vs); }
  int blocks_per_mcu() const { return ncomp == 3 ? hs * vs + 2 : 1; }
  uint64_t mcus() const { return uint64_t(mcu_cols()) * mcu_rows(); }
  uint64_t blocks() const { return mcus() * blocks_per_mcu(); }
  uint64_t intervals() const { return restart ? (mcus() + restart - 1) / restart : 1; }
  int subsampling() const { return ncomp == 1 ? 0 : (hs == 1 ? 444 : (vs == 1 ? 422 : 420)); }
  Tables tab;
};

namespace detail {
struct Huff { bool have = false; uint8_t bits[16]; uint8_t vals[256]; int count = 0; };

// jpeg_make_d_derived_tbl; false where libjpeg refuses the table
inline bool derive(const Huff& h, bool is_dc, DTab* t) {
  uint8_t size[257]; uint32_t code[257];
  int p = 0;
  for (int l = 1; l <= 16; ++l)
    for (int i = 0; i < h.bits[l - 1]; ++i) { if (p >= 256) return false; size[p++] = (uint8_t)l; }
  const int n = p;
  size[n] = 0;
  uint32_t c = 0; int si = size[0]; p = 0;
  while (p < n) {
    while (p < n && size[p] == si) code[p++] = c++;
    if (c >= (uint32_t(1) << si)) return false;
    c <<= 1; ++si;
  }
  memset(t, 0, sizeof *t);
  p = 0;
  for (int l = 1; l <= 16; ++l) {
    if (h.bits[l - 1]) { t->valoff[l] = p - (int32_t)code[p]; p += h.bits[l - 1]; t->maxcode[l] = (int32_t)code[p - 1]; }
    else t->maxcode[l] = -1;
  }
  t->maxcode[0] = -1; t->maxcode[17] = 0xFFFFF;
  p = 0;
  for (int l = 1; l <= 8; ++l)
    for (int i = 0; i < h.bits[l - 1]; ++i, ++p) {
      const uint32_t first = code[p] << (8 - l);
      for (uint32_t k = 0; k < (uint32_t(1) << (8 - l)); ++k) t->look[first + k] = (uint16_t)((l << 8) | h.vals[p]);
    }
  memcpy(t->vals, h.vals, 256);
  if (is_dc) for (int i = 0; i < n; ++i) if (h.vals[i] > 15) return false;
  return true;
}
}  // namespace detail

// false: *err says why.  `out` is only meaningful after true.
inline bool parse(const uint8_t* d, size_t bytes, Info* out, std::string* err) {
  std::string dummy;
  if (!err) err = &dummy;
  Info f;
  int nf = 0;
  // (a refusal still says what the frame header gave, for the probe)
  auto no = [&](const std::string& why) { *err = why; out->cols = f.cols; out->rows = f.rows; out->ncomp = nf; return false; };
  const uint64_t n = bytes;
  if (!d || n < 2 || d[0] != 0xFF || d[1] != 0xD8) return no("not a JPEG");
  uint64_t pos = 2;
  bool have_q[4] = {false, false, false, false}; uint8_t q[4][64];
  detail::Huff huff[2][4]; DTab derived[2][4];
  bool have_frame = false, jfif = false; int adobe = -1;
  uint8_t cid[4] = {0, 0, 0, 0}, chs[4] = {0, 0, 0, 0}, cvs[4] = {0, 0, 0, 0}, ctq[4] = {0, 0, 0, 0};
  int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  for (;;) {
    if (pos >= n) return no("truncated JPEG");
    if (d[pos] != 0xFF) return no("no marker where one is expected");
    while (pos < n && d[pos] == 0xFF) ++pos;
    if (pos >= n) return no("truncated JPEG");
    const int m = d[pos++];
    if (m == 0xD9) return no("no scan before EOI");
    if (m == 0xD8 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return no("unexpected marker");
    if (n - pos < 2) return no("truncated JPEG");
    const uint64_t L = (uint64_t(d[pos]) << 8) | d[pos + 1];
    if (L < 2 || L > n - pos) return no("truncated JPEG");
    const uint8_t* body = d + pos + 2; const uint64_t len = L - 2;
    pos += L;
    if (m == 0xDB) {
      for (uint64_t k = 0; k < len; k += 65) {
        const int pq = body[k] >> 4, tq = body[k] & 15;
        if (pq != 0) return no("16-bit quantisation table");
        if (tq > 3 || len - k < 65) return no("bad quantisation table");
        memcpy(q[tq], body + k + 1, 64); have_q[tq] = true;
      }
    } else if (m == 0xC4) {
      for (uint64_t k = 0; k < len;) {
        if (len - k < 17) return no("bad Huffman table");
        const int tc = body[k] >> 4, th = body[k] & 15;
        uint64_t cnt = 0;
        for (int i = 0; i < 16; ++i) cnt += body[k + 1 + i];
        if (tc > 1 || th > 3 || cnt > 256 || len - k - 17 < cnt) return no("bad Huffman table");
        detail::Huff& h = huff[tc][th];
        memset(&h, 0, sizeof h);
        memcpy(h.bits, body + k + 1, 16); memcpy(h.vals, body + k + 17, (size_t)cnt); h.count = (int)cnt;
        if (!detail::derive(h, tc == 0, &derived[tc][th])) return no("bad Huffman table");
        h.have = true;
        k += 17 + cnt;
      }
    } else if (m == 0xC0) {
      if (have_frame) return no("two frame headers");
      if (len < 6) return no("bad frame header");
      const int prec = body[0];
      f.rows = (uint32_t(body[1]) << 8) | body[2]; f.cols = (uint32_t(body[3]) << 8) | body[4]; nf = body[5];
      if (prec != 8) return no(std::to_string(prec) + "-bit samples");
      if (f.rows == 0) return no("height 0 (DNL)");
      if (f.cols == 0) return no("width 0");
      if (len != 6 + 3 * uint64_t(nf)) return no("bad frame header");
      if (nf == 4) return no("four components");
      if (nf != 1 && nf != 3) return no(std::to_string(nf) + " components");
      for (int i = 0; i < nf; ++i) { cid[i] = body[6 + 3 * i]; chs[i] = body[7 + 3 * i] >> 4; cvs[i] = body[7 + 3 * i] & 15; ctq[i] = body[8 + 3 * i]; }
      have_frame = true;
    } else if (m == 0xCC) {
      return no("arithmetic coding");
    } else if (m >= 0xC1 && m <= 0xCF) {
      return no("frame type SOF" + std::to_string(m - 0xC0) + " (only baseline SOF0 is decoded)");
    } else if (m == 0xDD) {
      if (len != 2) return no("bad DRI");
      f.restart = (uint32_t(body[0]) << 8) | body[1];
    } else if (m == 0xDC) {
      return no("DNL");
    } else if (m == 0xE0) {
      if (len >= 14 && !memcmp(body, "JFIF\0", 5)) jfif = true;
    } else if (m == 0xEE) {
      if (len >= 12 && !memcmp(body, "Adobe", 5)) adobe = body[11];
    } else if (m == 0xDA) {
      if (!have_frame) return no("scan before the frame header");
      if (len < 1 || len != 4 + 2 * uint64_t(body[0])) return no("bad scan header");
      const int ns = body[0];
      if (ns != nf) return no("several scans (the scan holds " + std::to_string(ns) + " of " + std::to_string(nf) + " components)");
      for (int i = 0; i < ns; ++i) {
        if (body[1 + 2 * i] != cid[i]) return no("scan components out of frame order");
        td[i] = body[2 + 2 * i] >> 4; ta[i] = body[2 + 2 * i] & 15;
        if (td[i] > 3 || ta[i] > 3 || !huff[0][td[i]].have || !huff[1][ta[i]].have) return no("the scan refers to a missing Huffman table");
      }
      if (body[1 + 2 * ns] != 0 || body[2 + 2 * ns] != 63 || body[3 + 2 * ns] != 0) return no("several scans (spectral selection or successive approximation)");
      break;
    }
    // every other segment (APPn, COM, ...) is skipped
  }
  f.ncomp = nf;
  auto sampling = [&]() { std::string s; for (int i = 0; i < nf; ++i) s += (i ? "," : "") + std::to_string(chs[i]) + "x" + std::to_string(cvs[i]); return s; };
  if (nf == 1) {
    if (chs[0] != 1 || cvs[0] != 1) return no("sampling " + sampling() + " of a grey file");
    f.hs = f.vs = 1;
  } else {
    f.hs = chs[0]; f.vs = cvs[0];
    const bool ok = (f.hs == 1 && f.vs == 1) || (f.hs == 2 && f.vs == 1) || (f.hs == 2 && f.vs == 2);
    if (!ok || chs[1] != 1 || cvs[1] != 1 || chs[2] != 1 || cvs[2] != 1) return no("sampling " + sampling() + " (4:4:4, 4:2:2 and 4:2:0 are decoded)");
    if (!jfif && (adobe == 0 || (adobe < 0 && cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B'))) return no("an RGB file (no YCbCr transform)");
  }
  for (int i = 0; i < nf; ++i) {
    if (ctq[i] > 3 || !have_q[ctq[i]]) return no("the frame refers to a missing quantisation table");
    memcpy(f.tab.quant[i], q[ctq[i]], 64);
    f.tab.dc[i] = derived[0][td[i]]; f.tab.ac[i] = derived[1][ta[i]];
  }
  for (int i = nf; i < 3; ++i) { memset(f.tab.quant[i], 0, 64); memset(&f.tab.dc[i], 0, sizeof(DTab)); memset(&f.tab.ac[i], 0, sizeof(DTab)); }
  f.begin = pos;
  // the entropy segment runs up to EOI; only stuffing and RSTn may stand in it
  bool found = false;
  for (uint64_t k = pos; k + 1 < n;) {
    const void* hit = memchr(d + k, 0xFF, (size_t)(n - k));
    if (!hit) break;
    k = (uint64_t)((const uint8_t*)hit - d);
    if (k + 1 >= n) break;
    const int nb = d[k + 1];
    if (nb == 0 || (nb >= 0xD0 && nb <= 0xD7)) { k += 2; continue; }
    if (nb == 0xD9) { f.end = k; found = true; break; }
    if (nb == 0xFF) return no("fill bytes in the scan");
    if (nb == 0xDC) return no("DNL");
    char hex[8]; snprintf(hex, sizeof hex, "%02X", nb);
    return no(std::string("several scans (marker 0x") + hex + " after the scan)");
  }
  if (!found) return no("truncated JPEG: no EOI");
  if (f.end - f.begin >= kMaxSegment) return no("scan too large");
  *out = f;
  return true;
}

}  // namespace jpeg_parse
#endif
