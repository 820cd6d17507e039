// pano_stitch's reader of lens descriptions (tools/lens_rig.hpp) as a stand-alone program under the address and undefined-behaviour
// sanitizers: parses the file given as its argument and prints one line per image,
//   name w h f v y p r a b c d e crop(left right top bottom, or -)
// with the doubles as hex floats; a malformed file prints "error: <message>" and exits with 1.  Only the parser runs here: the mapping
// onto pf_lens calls the library and is covered where the library runs (tests/test_cli_lens.py).
// Built and run by tests/test_lens_rig_parser.py:  g++ -std=c++17 -fsanitize=address,undefined ...
#include <stdio.h>

#include <fstream>
#include <iterator>

#include "../../panorama-opticalflow_amd/tools/lens_rig.hpp"

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: %s FILE.pto\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  if (!in) { printf("cannot open %s\n", argv[1]); return 2; }
  const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  try {
    for (const lens_rig::Image& im : lens_rig::parse(text)) {
      printf("%s %d %d %d", im.name.c_str(), im.w(), im.h(), im.f());
      for (int k = 3; k < 12; ++k) printf(" %a", im.value[k]);
      if (im.has_crop) printf(" %d %d %d %d\n", im.crop[0], im.crop[1], im.crop[2], im.crop[3]);
      else printf(" -\n");
    }
  } catch (const lens_rig::ParseError& e) {
    printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
