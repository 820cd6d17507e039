// pano_stitch -lens_rig FILE: the description of a rig's cameras, read from a subset of Hugin's .pto project format, and its mapping
// onto the library's pf_lens (include/panoflow.h, "Lens remap on the device").
//
// What is read: the `i` lines, one per image, each carrying all of
//   w h      the photo's size in pixels
//   f        0 rectilinear; 2 circular fisheye and 3 full-frame fisheye, both equidistant; and, this project's own extension, 100
//            stereographic and 101 equisolid fisheye
//   v        the horizontal field of view in degrees
//   y p r    yaw, pitch, roll of the camera in degrees
//   a b c    the radial polynomial's coefficients
//   d e      the shift of the optical centre in pixels
//   n"name"  the file name
// A value `=N` takes the value the same letter has on image N (counted from 0 in the file's order; N must come earlier).  Optional:
// S (or C) left,right,top,bottom, the crop; with f 2 its inscribed circle becomes the lens's image circle, otherwise it is ignored.
// Every other token of an `i` line (the photometric letters Ra.. Eev Er Eb Va.. Vx Vy, TrX.., g t j ..) and every other line is ignored.
// A malformed `i` line -- an unknown f, a missing letter, a bad number, a dangling =N -- is an error that gives the line's number.
//
// The mapping, as panotools documents the letters: d, e -> shift_x, shift_y;  a, b, c -> a, b, c with dd = 1 - (a + b + c);
// v -> focal_px through pf_lens_focal (of the line's w);  y, p, r -> rot through pf_lens_rotation.  Images are matched to the run's
// input files by file name (the part after the last '/').
// AGREEMENT WITH nona'S PIXELS IS NEITHER CLAIMED NOR TESTED: the bytes are the library's own definition, and Hugin's
// conventions beyond the documented meaning of these letters (its interpolators, its sign of roll, its crop of f 3) are not reproduced.
#ifndef PANO_LENS_RIG_HPP_
#define PANO_LENS_RIG_HPP_

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/panoflow.h"

namespace lens_rig {

struct ParseError : std::runtime_error {
  explicit ParseError(const std::string& what) : std::runtime_error(what) {}
};

// the letters of one `i` line
struct Image {
  double value[12];   // in the order of kLetters: w h f v y p r a b c d e
  std::string name;
  bool has_crop = false;
  int crop[4] = {0, 0, 0, 0};   // left, right, top, bottom
  int w() const { return (int)value[0]; }
  int h() const { return (int)value[1]; }
  int f() const { return (int)value[2]; }
};
static const char kLetters[] = "whfvyprabcde";

static inline int letter_index(char c) {
  const char* at = c ? strchr(kLetters, c) : nullptr;
  return at ? int(at - kLetters) : -1;
}

static inline std::string at_line(int line, const std::string& what) { return "line " + std::to_string(line) + ": " + what; }

// a whole token as a finite number, or an error
static inline double number(const std::string& s, int line, const std::string& token) {
  errno = 0;
  char* end = nullptr;
  const double v = strtod(s.c_str(), &end);
  if (s.empty() || end != s.c_str() + s.size() || errno == ERANGE || !std::isfinite(v)) throw ParseError(at_line(line, "bad number in '" + token + "'"));
  return v;
}

static inline std::vector<Image> parse(const std::string& text) {
  std::vector<Image> images;
  std::istringstream in(text);
  std::string row;
  for (int line = 1; std::getline(in, row); ++line) {
    if (!row.empty() && row.back() == '\r') row.pop_back();
    if (row.size() < 2 || row[0] != 'i' || (row[1] != ' ' && row[1] != '\t')) continue;
    Image im;
    bool have[12] = {false}, have_name = false;
    size_t at = 1;
    while (at < row.size()) {
      while (at < row.size() && (row[at] == ' ' || row[at] == '\t')) ++at;
      if (at >= row.size()) break;
      size_t end = at;
      if (row[at] == 'n' && at + 1 < row.size() && row[at + 1] == '"') {   // the name may hold blanks
        end = row.find('"', at + 2);
        if (end == std::string::npos) throw ParseError(at_line(line, "unterminated file name"));
        im.name = row.substr(at + 2, end - at - 2);
        if (im.name.empty()) throw ParseError(at_line(line, "empty file name"));
        have_name = true;
        at = end + 1;
        continue;
      }
      while (end < row.size() && row[end] != ' ' && row[end] != '\t') ++end;
      const std::string token = row.substr(at, end - at);
      at = end;
      const std::string rest = token.substr(1);
      if (token[0] == 'S' || token[0] == 'C') {
        std::istringstream parts(rest);
        std::string part;
        int k = 0;
        while (std::getline(parts, part, ',')) {
          if (k >= 4) throw ParseError(at_line(line, "a crop has four numbers: '" + token + "'"));
          const double v = number(part, line, token);
          if (v != std::floor(v) || std::fabs(v) > 1.0e6) throw ParseError(at_line(line, "bad number in '" + token + "'"));
          im.crop[k++] = (int)v;
        }
        if (k != 4 || im.crop[1] <= im.crop[0] || im.crop[3] <= im.crop[2]) throw ParseError(at_line(line, "a crop is left,right,top,bottom with left < right and top < bottom: '" + token + "'"));
        im.has_crop = true;
        continue;
      }
      const int k = token.size() >= 2 ? letter_index(token[0]) : -1;
      if (k < 0) continue;   // not ours: photometric and translation letters, and whatever else Hugin writes
      if (rest[0] == '=') {
        const double ref = number(rest.substr(1), line, token);
        if (ref != std::floor(ref) || ref < 0 || ref >= (double)images.size()) throw ParseError(at_line(line, "'" + token + "' refers to an image that does not come earlier"));
        im.value[k] = images[(size_t)ref].value[k];
      } else {
        if (!(rest[0] == '-' || rest[0] == '+' || rest[0] == '.' || (rest[0] >= '0' && rest[0] <= '9'))) continue;   // another key that starts with our letter
        im.value[k] = number(rest, line, token);
      }
      have[k] = true;
    }
    for (int k = 0; k < 12; ++k)
      if (!have[k]) throw ParseError(at_line(line, std::string("the image has no '") + kLetters[k] + "'"));
    if (!have_name) throw ParseError(at_line(line, "the image has no n\"name\""));
    for (int k = 0; k < 3; ++k)
      if (im.value[k] != std::floor(im.value[k])) throw ParseError(at_line(line, std::string("'") + kLetters[k] + "' must be a whole number"));
    if (im.value[0] < 1 || im.value[0] > 65535 || im.value[1] < 1 || im.value[1] > 65535) throw ParseError(at_line(line, "w and h must be 1..65535"));
    const double fv = im.value[2];
    if (fv != 0 && fv != 2 && fv != 3 && fv != 100 && fv != 101) throw ParseError(at_line(line, "unknown f (0 rectilinear, 2 or 3 equidistant fisheye, 100 stereographic, 101 equisolid)"));
    const int f = im.f();
    if (!(im.value[3] > 0.0 && im.value[3] < (f == 0 ? 180.0 : 360.0))) throw ParseError(at_line(line, "v is outside the lens's field of view"));
    images.push_back(im);
  }
  return images;
}

static inline std::string base_name(const std::string& path) {
  const size_t slash = path.rfind('/');
  return slash == std::string::npos ? path : path.substr(slash + 1);
}

// the image whose name's last part is the path's, or null
static inline const Image* find(const std::vector<Image>& images, const std::string& path) {
  for (const Image& im : images)
    if (base_name(im.name) == base_name(path)) return &im;
  return nullptr;
}

static inline pf_lens to_lens(const Image& im, int filter) {
  const int f = im.f();
  pf_lens l;
  pf_lens_init(&l, f == 0 ? PF_LENS_RECTILINEAR : f == 100 ? PF_LENS_FISHEYE_STEREOGRAPHIC : f == 101 ? PF_LENS_FISHEYE_EQUISOLID : PF_LENS_FISHEYE_EQUIDISTANT);
  l.filter = filter;
  l.focal_px = pf_lens_focal(l.model, im.w(), im.value[3]);
  pf_lens_rotation(im.value[4], im.value[5], im.value[6], l.rot);
  l.a = im.value[7]; l.b = im.value[8]; l.c = im.value[9];
  l.dd = 1.0 - (l.a + l.b + l.c);
  l.shift_x = im.value[10]; l.shift_y = im.value[11];
  if (f == 2 && im.has_crop) {   // the inscribed circle; the crop's numbers are pixel edges, a position is a pixel centre
    const int wide = im.crop[1] - im.crop[0], tall = im.crop[3] - im.crop[2];
    l.crop_cx256 = 128 * (im.crop[0] + im.crop[1]) - 128;
    l.crop_cy256 = 128 * (im.crop[2] + im.crop[3]) - 128;
    l.crop_r256 = 128 * (wide < tall ? wide : tall);
  }
  return l;
}

}  // namespace lens_rig

#endif  // PANO_LENS_RIG_HPP_
