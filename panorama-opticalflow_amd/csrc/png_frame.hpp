// PNG framing on the host, header-only and free of HIP and zlib: CRC-32, the Adler-32 combine, the chunk writer and the size bound of the
// device PNG encoder (kernels_png.hip makes the deflate stream; pf_api_png.inl frames it with what is here).  Checked without a GPU by
// tests/cpp/png_frame_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace png_frame {

// ---- the deflate stream's segment format (shared with kernels_png.hip) ----
// The filtered scanlines are cut into segments of kSegBytes; each becomes complete deflate blocks that end on a byte boundary with an
// empty stored block (the sync marker: 3 header bits, padding, 00 00 FF FF).  A segment that does not shrink is one stored block and the
// marker.  4 * 4095: a multiple of 4 (dword loads of a segment) with odd factors 3^2 5 7 13, so that whole rows of 4 * cols + 1 bytes can
// fill a segment exactly (cols = 16: 252 rows), which a power of two never allows.
constexpr size_t kSegBytes = 16380;
constexpr size_t kSegOverhead = 10;   // worst case beyond the segment's own bytes: stored-block header 5 + sync marker 5
constexpr size_t kSegSlot = kSegBytes + 16;   // bytes reserved per segment before compaction (a multiple of 4)
constexpr uint32_t kAdlerBase = 65521;
constexpr size_t kIdatMax = 0x7fffffffu;   // a chunk's length field is 31 bits

inline size_t stream_bytes(int cols, int rows) { return size_t(rows) * (size_t(cols) * 4 + 1); }
inline size_t segments(size_t stream) { return (stream + kSegBytes - 1) / kSegBytes; }
inline size_t deflate_bound(size_t stream) { return stream + kSegOverhead * segments(stream); }

// ---- CRC-32 (IEEE 802.3, reflected, as PNG and zlib use it), slicing by 8 ----
struct CrcTable {
  uint32_t t[8][256];
  CrcTable() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 8; ++s) t[s][i] = t[0][t[s - 1][i] & 0xff] ^ (t[s - 1][i] >> 8);
  }
};
inline const CrcTable& crc_table() { static const CrcTable tab; return tab; }
// running form: crc32(crc32(0, a), b) == crc32(0, a ++ b)
inline uint32_t crc32(uint32_t crc, const uint8_t* p, size_t n) {
  const CrcTable& T = crc_table();
  uint32_t c = ~crc;
  while (n && (reinterpret_cast<uintptr_t>(p) & 3)) { c = T.t[0][(c ^ *p++) & 0xff] ^ (c >> 8); --n; }
  while (n >= 8) {
    uint32_t a, b;
    memcpy(&a, p, 4); memcpy(&b, p + 4, 4);   // little-endian host (x86-64)
    a ^= c;
    c = T.t[7][a & 0xff] ^ T.t[6][(a >> 8) & 0xff] ^ T.t[5][(a >> 16) & 0xff] ^ T.t[4][a >> 24] ^
        T.t[3][b & 0xff] ^ T.t[2][(b >> 8) & 0xff] ^ T.t[1][(b >> 16) & 0xff] ^ T.t[0][b >> 24];
    p += 8; n -= 8;
  }
  while (n--) c = T.t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
  return ~c;
}

// ---- Adler-32 ----
// serial form (the reference the combine is checked against); adler starts at 1
inline uint32_t adler32(uint32_t adler, const uint8_t* p, size_t n) {
  uint64_t a = adler & 0xffff, b = adler >> 16;
  while (n) {
    const size_t k = n < 5552 ? n : 5552;   // the largest run that keeps b inside 32 bits; 64 bits here anyway
    for (size_t i = 0; i < k; ++i) { a += p[i]; b += a; }
    a %= kAdlerBase; b %= kAdlerBase;
    p += k; n -= k;
  }
  return uint32_t(b << 16 | a);
}
// Adler-32 of x ++ y from adler32(1, x), adler32(1, y) and y's length: a = a1 + a2 - 1, b = b1 + b2 + len2 * (a1 - 1)   (mod 65521)
inline uint32_t adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2) {
  const uint64_t M = kAdlerBase;
  const uint64_t a1 = ad1 & 0xffff, b1 = ad1 >> 16, a2 = ad2 & 0xffff, b2 = ad2 >> 16;
  const uint64_t a = (a1 + a2 + M - 1) % M;
  const uint64_t b = (b1 + b2 + (len2 % M) * ((a1 + M - 1) % M)) % M;
  return uint32_t(b << 16 | a);
}

// ---- the file's layout ----
// signature 8, IHDR chunk 25, the zlib stream (2 header bytes, the deflate bytes, 4 Adler bytes) in IDAT chunks of at most idat_max
// data bytes (12 bytes of length / type / CRC around each), IEND 12.
inline void put_be32(uint8_t* p, uint32_t v) { p[0] = uint8_t(v >> 24); p[1] = uint8_t(v >> 16); p[2] = uint8_t(v >> 8); p[3] = uint8_t(v); }

struct Frame {
  int cols, rows;
  size_t deflate_len;   // bytes of the deflate stream
  size_t idat_max;
  Frame(int cols_, int rows_, size_t deflate_len_, size_t idat_max_ = kIdatMax) : cols(cols_), rows(rows_), deflate_len(deflate_len_), idat_max(idat_max_) {}
  size_t zlib_len() const { return deflate_len + 6; }
  size_t idat_chunks() const { return (zlib_len() + idat_max - 1) / idat_max; }
  size_t file_size() const { return 8 + 25 + zlib_len() + 12 * idat_chunks() + 12; }
  // where byte `z` of the zlib stream lies in the file
  size_t file_offset(size_t z) const { return 33 + (z / idat_max) * (idat_max + 12) + 8 + z % idat_max; }
  // the deflate bytes [d, d + *run) lie contiguously in the file from the returned offset; *run = how many do (at most `want`)
  size_t deflate_run(size_t d, size_t want, size_t* run) const {
    const size_t z = d + 2, room = idat_max - z % idat_max;
    *run = want < room ? want : room;
    return file_offset(z);
  }
  // signature and IHDR: 8 bits, colour type 6 (RGBA), deflate, adaptive filtering, no interlace
  void write_head(uint8_t* out) const {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    memcpy(out, sig, 8);
    uint8_t* h = out + 8;
    put_be32(h, 13); memcpy(h + 4, "IHDR", 4);
    put_be32(h + 8, uint32_t(cols)); put_be32(h + 12, uint32_t(rows));
    h[16] = 8; h[17] = 6; h[18] = 0; h[19] = 0; h[20] = 0;
    put_be32(h + 21, crc32(0, h + 4, 17));
  }
  // after the deflate bytes are in place (deflate_run): the zlib header, the Adler-32, every IDAT's length / type / CRC, and IEND
  void write_tail(uint8_t* out, uint32_t adler) const {
    out[file_offset(0)] = 0x78; out[file_offset(1)] = 0x01;   // deflate, 32 KB window, fastest level; (0x7801 % 31 == 0)
    for (int i = 0; i < 4; ++i) out[file_offset(deflate_len + 2 + i)] = uint8_t(adler >> (24 - 8 * i));
    const size_t zl = zlib_len(), nch = idat_chunks();
    for (size_t k = 0; k < nch; ++k) {
      const size_t len = (k + 1 < nch) ? idat_max : zl - k * idat_max;
      uint8_t* ch = out + 33 + k * (idat_max + 12);
      put_be32(ch, uint32_t(len)); memcpy(ch + 4, "IDAT", 4);
      put_be32(ch + 8 + len, crc32(0, ch + 4, len + 4));
    }
    uint8_t* e = out + file_size() - 12;
    put_be32(e, 0); memcpy(e + 4, "IEND", 4); put_be32(e + 8, crc32(0, e + 4, 4));
  }
};

// capacity that suffices for any cols x rows image, whatever its content
inline size_t bound(int cols, int rows) { return Frame(cols, rows, deflate_bound(stream_bytes(cols, rows))).file_size(); }

}  // namespace png_frame
