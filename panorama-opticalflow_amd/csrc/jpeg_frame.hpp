// JPEG framing on the host, header-only and free of HIP: the Annex K tables, libjpeg's quality scaling, the Huffman code tables the
// entropy kernel reads, the file header (SOI .. SOS) in libjpeg's order, the GPano XMP segment, EOI and the size bound of the device
// JPEG encoder (kernels_jpeg.hip makes the entropy-coded segment; pf_api_jpeg.inl frames it with what is here).  DESIGN.md 8.4.
// The file is a baseline sequential JPEG (SOF0), 8 bits, Y Cb Cr, JFIF 1.01.  The input is packed BGRA: alpha is dropped and the
// colour bytes are encoded as stored (no un-premultiplying, no matte).  Checked without a GPU by tests/cpp/jpeg_frame_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace jpeg_frame {

// ---- Annex K (read out of files libjpeg wrote: quality 50 gives the base tables as they are) ----
constexpr uint8_t kQuantLuma[64] = {   // natural (row-major) order
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kQuantChroma[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr uint8_t kZigzag[64] = {   // zigzag position -> natural index
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// ---- geometry ----
// subsampling 0: 4:4:4, an MCU is one 8x8 block per component; 1: 4:2:0, an MCU is 16x16 pixels, four luma blocks and one of each chroma
constexpr int kMaxSide = 65535;          // SOF0 holds a side in 16 bits
constexpr int kBlockBits = 1660;         // the most one block can send: DC 11 + 11 (chroma), 63 x (16 + 10) AC
constexpr size_t kBlockBytes = 208;      // ... in bytes, rounded up; every byte may be 0xFF and take a stuffed 0x00 behind it
// MCUs per restart interval: 192 blocks either way, one per thread of the entropy kernel's workgroup (chosen against half and double:
// DESIGN.md 8.4)
inline int restart_interval(int subsampling) { return subsampling == 0 ? 64 : subsampling == 1 ? 32 : 0; }
inline int mcu_side(int subsampling) { return subsampling ? 16 : 8; }
inline int blocks_per_mcu(int subsampling) { return subsampling ? 6 : 3; }
inline size_t mcu_cols(int cols, int subsampling) { return (size_t(cols) + mcu_side(subsampling) - 1) / mcu_side(subsampling); }
inline size_t mcus(int cols, int rows, int subsampling) { return mcu_cols(cols, subsampling) * mcu_cols(rows, subsampling); }
inline size_t blocks(int cols, int rows, int subsampling) { return mcus(cols, rows, subsampling) * blocks_per_mcu(subsampling); }
inline size_t intervals(int cols, int rows, int subsampling, int restart) { return (mcus(cols, rows, subsampling) + restart - 1) / restart; }
inline size_t coef_bytes(int cols, int rows, int subsampling) { return blocks(cols, rows, subsampling) * 128; }   // int16 x 64

// ---- quality ----
// jpeg_set_quality: table entry = (base * scale + 50) / 100 clamped to 1..255 (baseline); out[] in natural order
inline void quant_table(const uint8_t* base, int quality, uint8_t* out) {
  const long scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    long v = (base[i] * scale + 50) / 100;
    out[i] = uint8_t(v < 1 ? 1 : v > 255 ? 255 : v);
  }
}

// ---- what the kernels read (shared with kernels_jpeg.hip) ----
// qv: 8 * table entry, per component class (0 luma, 1 chroma), in zigzag order; unzig: natural index -> zigzag position;
// Huffman: code << 5 | length per symbol, 0 where the table has no such symbol
struct Tables {
  uint16_t qv[2][64];
  uint8_t unzig[64];
  uint32_t dc[2][16];
  uint32_t ac[2][256];
};
inline void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out, int nout) {
  for (int i = 0; i < nout; ++i) out[i] = 0;
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = code++ << 5 | uint32_t(len);
    code <<= 1;
  }
}
inline void make_tables(int quality, Tables* t) {
  uint8_t q[2][64];
  quant_table(kQuantLuma, quality, q[0]); quant_table(kQuantChroma, quality, q[1]);
  for (int c = 0; c < 2; ++c)
    for (int z = 0; z < 64; ++z) t->qv[c][z] = uint16_t(8 * q[c][kZigzag[z]]);
  for (int z = 0; z < 64; ++z) t->unzig[kZigzag[z]] = uint8_t(z);
  huff_codes(kDcLumaBits, kDcVals, t->dc[0], 16); huff_codes(kDcChromaBits, kDcVals, t->dc[1], 16);
  huff_codes(kAcLumaBits, kAcLumaVals, t->ac[0], 256); huff_codes(kAcChromaBits, kAcChromaVals, t->ac[1], 256);
}

// ---- the file ----
constexpr char kXmpId[] = "http://ns.adobe.com/xap/1.0/";   // with its terminating NUL: 29 bytes
constexpr size_t kXmpMax = 1024;   // room for the packet below with four 5-digit sizes

// the XMP packet of an equirectangular panorama that fills the sphere; returns its length (< kXmpMax)
inline size_t xmp_packet(int cols, int rows, char* out) {
  const int n = snprintf(out, kXmpMax,
                         "<x:xmpmeta xmlns:x=\"adobe:ns:meta/\"><rdf:RDF xmlns:rdf=\"http://www.w3.org/1999/02/22-rdf-syntax-ns#\">"
                         "<rdf:Description rdf:about=\"\" xmlns:GPano=\"http://ns.google.com/photos/1.0/panorama/\" "
                         "GPano:ProjectionType=\"equirectangular\" GPano:UsePanoramaViewer=\"True\" "
                         "GPano:FullPanoWidthPixels=\"%d\" GPano:FullPanoHeightPixels=\"%d\" "
                         "GPano:CroppedAreaImageWidthPixels=\"%d\" GPano:CroppedAreaImageHeightPixels=\"%d\" "
                         "GPano:CroppedAreaLeftPixels=\"0\" GPano:CroppedAreaTopPixels=\"0\"/></rdf:RDF></x:xmpmeta>",
                         cols, rows, cols, rows);
  return size_t(n);
}

inline uint8_t* put_segment(uint8_t* p, uint8_t marker, const uint8_t* body, size_t n) {
  p[0] = 0xFF; p[1] = marker; p[2] = uint8_t((n + 2) >> 8); p[3] = uint8_t(n + 2);
  memcpy(p + 4, body, n);
  return p + 4 + n;
}

// APP1: the identifier, its NUL, the packet.  Returns the segment's length, marker included.
inline size_t write_xmp(int cols, int rows, uint8_t* out) {
  uint8_t body[sizeof kXmpId + kXmpMax];
  memcpy(body, kXmpId, sizeof kXmpId);
  const size_t n = sizeof kXmpId + xmp_packet(cols, rows, reinterpret_cast<char*>(body) + sizeof kXmpId);
  return size_t(put_segment(out, 0xE1, body, n) - out);
}

constexpr size_t kHeadPlain = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 6 + 14;   // SOI, APP0, 2 DQT, SOF0, 4 DHT, DRI, SOS = 629
constexpr size_t kHeadMax = kHeadPlain + 4 + sizeof kXmpId + kXmpMax;

// SOI .. SOS in libjpeg's order; returns the header's length (at most kHeadMax)
inline size_t write_head(int cols, int rows, int quality, int subsampling, int restart, int gpano, uint8_t* out) {
  uint8_t* p = out;
  *p++ = 0xFF; *p++ = 0xD8;
  static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};   // 1.01, no units, density 1 x 1, no thumbnail
  p = put_segment(p, 0xE0, jfif, sizeof jfif);
  if (gpano) p += write_xmp(cols, rows, p);
  for (int c = 0; c < 2; ++c) {
    uint8_t q[64], body[65];
    quant_table(c ? kQuantChroma : kQuantLuma, quality, q);
    body[0] = uint8_t(c);
    for (int z = 0; z < 64; ++z) body[1 + z] = q[kZigzag[z]];
    p = put_segment(p, 0xDB, body, sizeof body);
  }
  const uint8_t sof[15] = {8, uint8_t(rows >> 8), uint8_t(rows), uint8_t(cols >> 8), uint8_t(cols), 3, 1, uint8_t(subsampling ? 0x22 : 0x11), 0, 2, 0x11, 1, 3, 0x11, 1};
  p = put_segment(p, 0xC0, sof, sizeof sof);
  const struct { uint8_t id; const uint8_t* bits; const uint8_t* vals; size_t n; } dht[4] = {
      {0x00, kDcLumaBits, kDcVals, 12}, {0x10, kAcLumaBits, kAcLumaVals, 162}, {0x01, kDcChromaBits, kDcVals, 12}, {0x11, kAcChromaBits, kAcChromaVals, 162}};
  for (const auto& h : dht) {
    uint8_t body[1 + 16 + 162];
    body[0] = h.id; memcpy(body + 1, h.bits, 16); memcpy(body + 17, h.vals, h.n);
    p = put_segment(p, 0xC4, body, 17 + h.n);
  }
  const uint8_t dri[2] = {uint8_t(restart >> 8), uint8_t(restart)};
  p = put_segment(p, 0xDD, dri, 2);
  static const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  p = put_segment(p, 0xDA, sos, sizeof sos);
  return size_t(p - out);
}

inline void write_eoi(uint8_t* p) { p[0] = 0xFF; p[1] = 0xD9; }

// the most the entropy-coded segment of any image of this shape can take: every block at its longest, every byte stuffed, and per
// interval the padding's byte and the marker
inline size_t scan_bound(int cols, int rows, int subsampling) {
  return blocks(cols, rows, subsampling) * (2 * kBlockBytes) + intervals(cols, rows, subsampling, restart_interval(subsampling)) * 4;
}
// capacity that suffices for any cols x rows image, whatever its content and parameters
inline size_t bound(int cols, int rows, int subsampling) { return kHeadMax + scan_bound(cols, rows, subsampling) + 2; }

}  // namespace jpeg_frame
