// The JPEG header parser (csrc/jpeg_parse.hpp) under the address and undefined-behaviour sanitizers, stand-alone.
//   jpeg_parse_check IN.pack OUT.txt   IN.pack: uint32 count, then per file uint32 length and its bytes.  Every file is parsed from a
//   heap buffer of exactly its length, so that a read past the end is caught.  One line per file: "P <reason>" where the parser refuses
//   it, else "A cols rows components hs vs restart begin end" and a checksum of the derived tables.
// Built and run by tests/test_jpegd_parse.py:  g++ -std=c++17 -fsanitize=address,undefined ...
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../panorama-opticalflow_amd/csrc/jpeg_parse.hpp"

int main(int argc, char** argv) {
  if (argc != 3) { printf("usage: %s IN.pack OUT.txt\n", argv[0]); return 2; }
  std::vector<uint8_t> pack;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) pack.insert(pack.end(), buf, buf + k);
  fclose(f);
  FILE* o = fopen(argv[2], "w");
  if (!o || pack.size() < 4) { printf("cannot write %s\n", argv[2]); return 2; }
  uint32_t n; memcpy(&n, pack.data(), 4);
  size_t at = 4;
  for (uint32_t k = 0; k < n; ++k) {
    uint32_t len; memcpy(&len, pack.data() + at, 4); at += 4;
    uint8_t* exact = new uint8_t[len ? len : 1];
    memcpy(exact, pack.data() + at, len); at += len;
    jpeg_parse::Info info;
    std::string why;
    if (!jpeg_parse::parse(exact, len, &info, &why)) fprintf(o, "P %s\n", why.c_str());
    else {
      // maxcode and valoff of the six tables and the quantisation tables, as the model derives them
      unsigned long long h = 1469598103934665603ull;
      auto mix = [&](long long v) { h ^= (unsigned long long)v & 0xffffffffull; h *= 1099511628211ull; };
      for (int c = 0; c < info.ncomp; ++c) {
        for (const jpeg_parse::DTab* t : {&info.tab.dc[c], &info.tab.ac[c]}) { for (int l = 1; l <= 17; ++l) mix(t->maxcode[l]); for (int l = 1; l <= 16; ++l) mix(t->maxcode[l] < 0 ? 0 : t->valoff[l]); }
        for (int i = 0; i < 64; ++i) mix(info.tab.quant[c][i]);
      }
      fprintf(o, "A %u %u %d %d %d %u %llu %llu %llu\n", info.cols, info.rows, info.ncomp, info.hs, info.vs, info.restart, (unsigned long long)info.begin,
              (unsigned long long)info.end, h);
    }
    delete[] exact;
  }
  fclose(o);
  printf("ok\n");
  return 0;
}
