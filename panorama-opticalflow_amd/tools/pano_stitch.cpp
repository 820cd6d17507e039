// Drop-in for the reference's CLI driver (CPU/main.cpp:47-110): same flags, same file names, same
// 5-step chain (R_i = FinalResult_{i-1}, main.cpp:64-65), same timing lines; all pixel work on the MI355X.
//   pano_stitch -test_dir <dir> -top_img top.tif -flow_alg pixflow_low|pixflow_search_20 [-steps 5] [-fused 0|1]
//   pano_stitch -inputs 4 -test_dir <dir> -flow_alg ...      the one-pass 4-photo variant (CPU_4Input/main.cpp:45-120)
//   -visualize 1: also writes <dir>/disparity/LtoR_<alg>_step<i>.png and RtoL_<alg>_step<i>.png for every step i, the panels of the
//   reference's buildvisualizations (main.cpp:20-45, its call site :85 is commented out there).  Deviation: the reference names them
//   LtoR_<alg>.png / RtoL_<alg>.png, so each step would overwrite the previous one; the step number keeps them all.
// reads <dir>/<top_img> and <dir>/1.tif .. 5.tif (8-bit RGB/RGBA TIFF or PNG), writes ProcessResult{i}.png and
// FinalResult.png (main.cpp:97-100).
//   pano_stitch -test_dirs <dir1>,<dir2>,... -top_img top.tif -flow_alg ... [-steps 5] [-in_flight 8]: the -test_dir flow for every
//   directory at once through the batched step (pf_stitch_step_batch, one frame per directory); each directory gets the same files as
//   its own -test_dir run, and one "Part<i> Finished!" line is printed per batched step.
//   -static_rig 1 (with -test_dirs): the directories are frames of ONE camera rig, i.e. they share their alpha masks.  Before step i a
//   stitch plan (overlap map + blend ramp) is made from the first directory's <i>.tif and its R of that step (the top image, then its
//   previous composite), and step i of all directories runs on it (pf_stitch_step_batch_planned): the same files, without recomputing
//   the map and the ramp per directory.  A directory whose masks differ from the first one's ends the run with an error that names it.
//   -rig_chain 1 (with -test_dirs ... -static_rig 1): ONE rig plan is made from the first directory's top image and <1..steps>.tif before
//   anything is solved, and all directories run their whole chains through one pf_rig_stitch_batch call: the same files; a directory off
//   the rig ends the run before any solve, with an error that names it and the step.  Host memory: the call takes all inputs and gives all
//   composites at once, so the run holds steps + 1 images per directory until the call returns and steps composites until they are
//   written: 4 (2 steps + 1) B/px per directory (25 GB for 16 directories of 9000x4000 x 5 steps), where -static_rig 1 alone holds one
//   step's images at a time.
//   -png_device 1 (any mode; off by default): every PNG is filtered, deflated and framed on the GPU (pf_png_*) and decodes to the same
//   pixels as the default writer's file.  The lone fused chain and -test_dirs without -rig_chain encode the composites where they lie in
//   HBM (pf_stitch_result_png / pf_stitch_batch_result_png) and bring no raw composite down (-static_rig 1: only the first directory's,
//   which the next plan is made from); -rig_chain 1, -inputs 4, -fused 0 and the -visualize panels hold their images on the host and
//   send them up to be encoded (pf_png_encode).
//   -jpeg_device 1 [-jpeg_quality Q] [-jpeg_subsampling 444|420] [-jpeg_gpano 1] (any mode; off by default): the results are written as
//   ProcessResult{i}.jpg and FinalResult.jpg IN PLACE OF the .png, baseline JPEGs made on the GPU (pf_jpeg_*: quality 1..100, default 90;
//   4:2:0 by default; -jpeg_gpano 1 adds the GPano XMP packet that makes a 2:1 result open as a sphere, and ends the run on any other
//   shape), encoded where -png_device 1 would encode them: in HBM where the composite lies there, sent up from the host otherwise.  The
//   -visualize panels stay PNG (by the default writer, or with -png_device 1 as well by the device PNG encoder).
//   -tiff_device 1 (any mode; off by default): a .tif input is decoded on the GPU (pf_tiff_*) when the library can decode it there -- no
//   compression, LZW or PackBits -- and it is uncompressed or has at least 64 strips (strips decode in parallel; a single LZW strip is one
//   serial stream and stays with the host).  Every other file, deflate TIFFs included, goes through the host reader as before.  The
//   pixels are the host reader's, with one difference: a malformed or short strip, which the host reader zero-fills silently, ends the run
//   with an error.  With -rig_chain 1 every input is decoded into its own device buffer, the rig plan is made from device images
//   (pf_rig_plan_create_dev) and the chains run through pf_rig_stitch_batch_dev; with -png_device 1 as well each composite is encoded
//   where it lies, so no raw image crosses the link in either direction; without it the composites are downloaded and written by the
//   default writer.
//   -tiff_inflate 1 (with -tiff_device 1; off by default): deflate TIFFs (compression 8 / 32946) fall under the same rule as LZW ones --
//   at least 64 strips -- through the library's inflate switch (pf_tiff_set_inflate).  A strip is accepted exactly when zlib's uncompress
//   into the strip's size succeeds or ends with Z_BUF_ERROR and the strip full; a short or malformed strip ends the run.
//   -result_size WxH [-result_filter lanczos|bicubic|bilinear|hamming|box] (any mode; needs -png_device 1 or -jpeg_device 1): every result
//   file of the run -- ProcessResult{i}, FinalResult, in every directory of -test_dirs -- is written at W x H, resized on the GPU between
//   the composite and the encoder (pf_resize_*: Pillow's Image.resize of the RGBA image, byte for byte; lanczos by default).  The chain
//   itself stays at full size.  Where the composite lies in HBM it is resized from there; where the mode holds it on the host it is sent
//   up once and resized there.  The -visualize panels are not scaled.  With -jpeg_gpano 1 it is W x H that must be 2:1.
//   -level yaw,pitch,roll (degrees; any mode; needs -png_device 1 or -jpeg_device 1): every result file of the run is the composite turned
//   on the GPU at the canvas's size (pf_reproject_*: equirect to equirect, bicubic; yaw turns the view to the right, pitch up, roll lifts
//   its right side), before -result_size and before the encoder.  The chain itself runs on the unturned composites.  The shape does not
//   change, so the -jpeg_gpano rules are the same.
//   -cube N [-cube_filter bicubic|bilinear] (any mode; needs -png_device 1 or -jpeg_device 1): beside every result file <stem>.(png|jpg) six
//   cube faces <stem>_front|right|back|left|up|down.(png|jpg) of N x N are written, cut on the GPU from the result at the canvas's size
//   (the levelled one with -level) and encoded where they lie; -result_size does not apply to them, nor does -jpeg_gpano.  There is no
//   antialiasing: choose N near a quarter of the canvas's width.
//   -lens_rig FILE -canvas WxH (any mode; both or neither): every input the run reads -- 1.tif .. 5.tif, the top image, in every directory of
//   -test_dirs -- is a RAW PHOTO of a camera that FILE describes (tools/lens_rig.hpp: a subset of Hugin's .pto; rectilinear and fisheye
//   lenses, pose, radial polynomial, shift, image circle), matched by file name, and is remapped on the GPU onto a W x H equirectangular
//   canvas (pf_lens_*; bicubic) before anything else sees it: the warp that otherwise has to be done by another program
//   beforehand.  The host-image modes remap inside the image read (pf_lens_remap); -rig_chain 1 -tiff_device 1 decodes a directory's
//   photos into device buffers and remaps them there (pf_lens_remap_batch_dev, one launch per directory when the photos have one size), so
//   that no raw image crosses the link.  The canvas is 360 degrees across with square angular pixels, centred on the horizon.  Agreement
//   with Hugin's nona is not claimed.
//   -input_ext jpg (any mode; default tif; needs -lens_rig and -canvas): the photos are 1.jpg .. 5.jpg -- what a camera writes -- and are
//   decoded on the GPU (pf_jpeg_decode*, DESIGN.md 8.10: baseline files, grey or Y Cb Cr at 4:4:4 / 4:2:2 / 4:2:0).  The top image is as
//   -top_img names it; a .jpg or .jpeg top image is decoded the same way.  A JPEG has no alpha, so the flag is refused without -lens_rig,
//   whose remap makes the masks.  There is no host JPEG reader: the host-image modes call pf_jpeg_decode, and -rig_chain 1 -tiff_device 1
//   decodes a directory's photos in one pf_jpeg_decode_batch_dev per photo size into the buffers pf_lens_remap_batch_dev reads.  A file
//   outside the decoder's contract or with a damaged scan ends the run with the library's reason.
#include <sys/stat.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../include/OpticalFlow.hpp"
#include "../include/StitchTool.hpp"
#include "image_io.hpp"
#include "lens_rig.hpp"

using namespace panocv;
using namespace util;
using namespace optical_flow;
using namespace stitch_tools;

static bool g_png_device = false;   // -png_device 1
// a host image to a PNG file, by the default writer or through the device encoder
static void writeImage(const std::string& path, const Mat& image) {
  if (g_png_device) pano_io::write_png_device(path, pano::context(), image);
  else pano_io::imwriteExceptionOnFail(path, image);
}
static bool g_jpeg_device = false;   // -jpeg_device 1: the results (not the panels) as JPEGs made on the device
static pf_jpeg_params g_jpeg;
static int g_result_cols = 0, g_result_rows = 0, g_result_filter = PF_RESIZE_LANCZOS;   // -result_size WxH (0: the canvas's size) -result_filter
// <stem>.jpg or <stem>.png of the result-size image that resize(d_dst) -- a pf_*resize* call bound to its source -- makes in device memory
template <class Resize>
static void writeResized(const std::string& stem, Resize resize) {
  pf_ctx* ctx = pano::context();
  pano_io::DeviceImage d(ctx, g_result_cols, g_result_rows);
  pano::check(resize(d.p));
  if (g_jpeg_device) pano_io::write_jpeg_device(stem + ".jpg", ctx, g_jpeg, d.p, d.cols, d.rows);
  else pano_io::write_png_bytes(stem + ".png", ctx, d.cols, d.rows, [&](unsigned char* b, size_t cap, size_t* n) { return pf_png_encode_dev(ctx, d.p, d.cols, d.rows, b, cap, n); });
}
static bool g_level = false;         // -level yaw,pitch,roll
static double g_level_rot[9];
static int g_cube = 0, g_cube_filter = PF_REPROJECT_BICUBIC;   // -cube N -cube_filter
// <stem>.jpg or <stem>.png of a packed device image
static void writeDeviceImage(const std::string& stem, const unsigned char* d, int cols, int rows, const pf_jpeg_params& jpeg) {
  pf_ctx* ctx = pano::context();
  if (g_jpeg_device) pano_io::write_jpeg_device(stem + ".jpg", ctx, jpeg, d, cols, rows);
  else pano_io::write_png_bytes(stem + ".png", ctx, cols, rows, [&](unsigned char* b, size_t cap, size_t* n) { return pf_png_encode_dev(ctx, d, cols, rows, b, cap, n); });
}
// -level and -cube: with -level the result file itself, from the composite turned at its own size (then -result_size, then the encoder); with
// -cube the six faces beside it, from the turned composite if there is one.  Nothing but the encoded files comes down.
static void writeReprojected(const std::string& stem, pano_io::ResultSource src) {
  pf_ctx* ctx = pano::context();
  std::unique_ptr<pano_io::DeviceImage> level;
  pf_reproject_params p;
  pf_reproject_params_init(&p);
  if (g_level) {
    level.reset(new pano_io::DeviceImage(ctx, src.cols, src.rows));
    p.projection = PF_PROJ_EQUIRECT;
    for (int k = 0; k < 9; ++k) p.rot[k] = g_level_rot[k];
    pano::check(pano_io::reproject_result(ctx, src, src.cols, src.rows, p, level->p));
    src = pano_io::ResultSource::device(level->p, src.cols, src.rows);
    if (g_result_cols) writeResized(stem, [&](unsigned char* d) { return pf_resize_dev(ctx, src.d, src.cols, src.rows, d, g_result_cols, g_result_rows, g_result_filter); });
    else writeDeviceImage(stem, src.d, src.cols, src.rows, g_jpeg);
  }
  if (!g_cube) return;
  static const char* const names[6] = {"front", "right", "back", "left", "up", "down"};
  std::unique_ptr<pano_io::DeviceImage> faces[6];
  unsigned char* d_faces[6];
  for (int f = 0; f < 6; ++f) { faces[f].reset(new pano_io::DeviceImage(ctx, g_cube, g_cube)); d_faces[f] = faces[f]->p; }
  pf_reproject_params_init(&p);   // the identity: a turn is in the source already
  p.filter = g_cube_filter;
  if (src.kind == pano_io::ResultSource::kDevice) pano::check(pf_reproject_cube_dev(ctx, src.d, src.cols, src.rows, d_faces, g_cube, &p));
  else for (int f = 0; f < 6; ++f) { p.face = f; pano::check(pano_io::reproject_result(ctx, src, g_cube, g_cube, p, d_faces[f])); }
  pf_jpeg_params plain = g_jpeg;
  plain.gpano = 0;
  for (int f = 0; f < 6; ++f) writeDeviceImage(stem + "_" + names[f], d_faces[f], g_cube, g_cube, plain);
}
// a host result image to <stem>.png, or with -jpeg_device 1 to <stem>.jpg; with -result_size sent up once and resized there
static void writeResult(const std::string& stem, const Mat& image) {
  if (g_level || g_cube) {
    pano_io::DeviceImage up(pano::context(), image.cols, image.rows);
    pano::check(pano_io::upload_host_image(pano::context(), image, up.p));
    writeReprojected(stem, pano_io::ResultSource::device(up.p, image.cols, image.rows));
    if (g_level) return;
  }
  if (g_result_cols) return writeResized(stem, [&](unsigned char* d) { return pano_io::resize_host_image(pano::context(), image, g_result_cols, g_result_rows, g_result_filter, d); });
  if (g_jpeg_device) pano_io::write_jpeg_device(stem + ".jpg", pano::context(), g_jpeg, image);
  else writeImage(stem + ".png", image);
}
static bool g_tiff_device = false;   // -tiff_device 1
static bool g_tiff_inflate = false;  // -tiff_inflate 1
// the context the device readers decode with: the process's one context (this program is single-threaded), its inflate switch set once,
// when the first reader asks for it -- after every refusal of the command line
static pf_ctx* tiffContext() {
  pf_ctx* ctx = pano::context();
  static bool set = false;
  if (!set) { pano::check(pf_tiff_set_inflate(ctx, g_tiff_inflate ? 1 : 0)); set = true; }
  return ctx;
}
static std::vector<lens_rig::Image> g_lens_rig;   // -lens_rig FILE: the cameras; empty: the inputs are canvases already
static std::string g_lens_rig_file;
static int g_canvas_cols = 0, g_canvas_rows = 0;   // -canvas WxH
// the lens of the photo read from `path`, which must have the size its description gives
static pf_lens lensOf(const std::string& path, int cols, int rows) {
  const lens_rig::Image* im = lens_rig::find(g_lens_rig, path);
  if (!im) throw VrCamException("-lens_rig: " + g_lens_rig_file + " describes no image named " + lens_rig::base_name(path));
  if (im->w() != cols || im->h() != rows)
    throw VrCamException("-lens_rig: " + path + " is " + std::to_string(cols) + "x" + std::to_string(rows) + ", not the " + std::to_string(im->w()) + "x" + std::to_string(im->h()) + " of its description");
  return lens_rig::to_lens(*im, PF_REPROJECT_BICUBIC);
}
static std::string g_input_ext = "tif";   // -input_ext tif|jpg: the extension of <1..steps>.<ext>
static bool isJpegName(const std::string& path) {
  const size_t dot = path.rfind('.'); std::string ext = dot == std::string::npos ? "" : path.substr(dot + 1);
  for (auto& c : ext) c = (char)tolower(c);
  return ext == "jpg" || ext == "jpeg";
}
// a JPEG file's bytes and what the decoder's probe says of them; a file the device does not decode ends the run with the reason
static std::vector<unsigned char> readJpegFile(const std::string& path, pf_jpeg_info* info) {
  if (g_lens_rig.empty()) throw VrCamException("a JPEG input needs -lens_rig FILE and -canvas WxH (a JPEG has no alpha; the remap makes the masks): " + path);
  std::vector<unsigned char> b = pano_io::read_file(path);
  info->struct_size = sizeof *info;
  if (pf_jpeg_probe(nullptr, b.data(), b.size(), info) != 0) throw VrCamException(std::string("panoflow: ") + pf_last_error(nullptr) + ": " + path);
  if (!info->device_decodable) throw VrCamException(std::string("panoflow: jpeg: ") + info->reason + ": " + path);
  return b;
}
// an image file to a host image, by the host readers or (a .tif under the device rule, see the usage note) through the device decoder;
// with -lens_rig the file is a raw photo and the image its canvas
static Mat readImage(const std::string& path) {
  if (isJpegName(path)) {   // (always a raw photo: readJpegFile refuses it without -lens_rig)
    pf_jpeg_info info;
    const std::vector<unsigned char> b = readJpegFile(path, &info);
    Mat photo(info.rows, info.cols, CV_8UC4);
    if (pf_jpeg_decode(pano::context(), b.data(), b.size(), info.cols, info.rows, photo.data, photo.step) != 0)
      throw VrCamException(std::string("panoflow: ") + pf_last_error(pano::context()) + ": " + path);
    const pf_lens lens = lensOf(path, photo.cols, photo.rows);
    Mat canvas(g_canvas_rows, g_canvas_cols, CV_8UC4);
    pano::check(pf_lens_remap(pano::context(), photo.data, photo.step, photo.cols, photo.rows, canvas.data, canvas.step, canvas.cols, canvas.rows, &lens));
    return canvas;
  }
  Mat raw = g_tiff_device ? pano_io::imread_device(path, tiffContext()) : pano_io::imreadExceptionOnFail(path);
  if (g_lens_rig.empty()) return raw;
  if (raw.type() != CV_8UC4) throw VrCamException("-lens_rig: " + path + " is not a CV_8UC4 image");
  const pf_lens lens = lensOf(path, raw.cols, raw.rows);
  Mat canvas(g_canvas_rows, g_canvas_cols, CV_8UC4);
  pano::check(pf_lens_remap(pano::context(), raw.data, raw.step, raw.cols, raw.rows, canvas.data, canvas.step, canvas.cols, canvas.rows, &lens));
  return canvas;
}

static std::map<std::string, std::string> parseFlags(int argc, char** argv) {   // gflags syntax: -name value | --name=value
  std::map<std::string, std::string> f;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a.empty() || a[0] != '-') throw VrCamException("unexpected argument: " + a);
    a = a.substr(a.find_first_not_of('-'));
    const size_t eq = a.find('=');
    if (eq != std::string::npos) f[a.substr(0, eq)] = a.substr(eq + 1);
    else if (i + 1 < argc) f[a] = argv[++i];
    else throw VrCamException("missing value for flag: " + a);
  }
  return f;
}


// cvtColor(GRAY2BGRA / BGR2BGRA) of the 8-bit images buildvisualizations converts (alpha 255)
static Mat toBGRA(const Mat& m) {
  Mat out(m.rows, m.cols, CV_8UC4);
  for (int y = 0; y < m.rows; ++y)
    for (int x = 0; x < m.cols; ++x) {
      const unsigned char* p = m.ptr<unsigned char>(y) + size_t(x) * m.elemSize();
      out.at<Vec4b>(y, x) = m.type() == CV_8UC1 ? Vec4b(p[0], p[0], p[0], 255) : Vec4b(p[0], p[1], p[2], 255);
    }
  return out;
}

// CPU/main.cpp:20-45, one file per direction and step (see the usage note at the top)
static void buildvisualizations(const Mat flowLtoR, const Mat flowRtoL, const Mat ImageL, const Mat ImageR, const std::string& dir,
                                const std::string& alg, int step) {
  Mat flowVisLtoR = visualizeFlowAsGreyDisparity(flowLtoR);
  Mat flowVisRtoL = visualizeFlowAsGreyDisparity(flowRtoL);
  Mat flowVisLtoRColorWheel = visualizeFlowColorWheel(flowLtoR);
  Mat flowVisRtoLColorWheel = visualizeFlowColorWheel(flowRtoL);
  Mat flowVisLtoRColorWithLines = visualizeFlowAsVectorField(flowLtoR, ImageL);
  Mat flowVisRtoLColorWithLines = visualizeFlowAsVectorField(flowRtoL, ImageR);
  Mat horizontalVisLtoR = stackHorizontal(std::vector<Mat>({toBGRA(flowVisLtoR), toBGRA(flowVisLtoRColorWheel), flowVisLtoRColorWithLines}));
  Mat horizontalVisRtoL = stackHorizontal(std::vector<Mat>({toBGRA(flowVisRtoL), toBGRA(flowVisRtoLColorWheel), flowVisRtoLColorWithLines}));
  writeImage(dir + "/disparity/LtoR_" + alg + "_step" + std::to_string(step) + ".png", horizontalVisLtoR);
  writeImage(dir + "/disparity/RtoL_" + alg + "_step" + std::to_string(step) + ".png", horizontalVisRtoL);
}

// the same panels of a fused step, from the flows and inputs pf_stitch_step left in HBM
static void stitchVisualizations(int cols, int rows, const std::string& dir, const std::string& alg, int step) {
  Mat l2r(rows, 3 * cols, CV_8UC4), r2l(rows, 3 * cols, CV_8UC4);
  pano::check(pf_stitch_visualize(pano::context(), l2r.data, r2l.data, l2r.step));
  writeImage(dir + "/disparity/LtoR_" + alg + "_step" + std::to_string(step) + ".png", l2r);
  writeImage(dir + "/disparity/RtoL_" + alg + "_step" + std::to_string(step) + ".png", r2l);
}

// CPU_4Input/main.cpp:54-113: crop every photo to the columns where its centre row is opaque, L = 1 + 3, R = 2 + 4
// (saturating), then ONE stitch step.  The crop/sum is the driver's own image preparation (byte copies on the host,
// as in the reference); the stitch step runs on the device.
static int run4Input(const std::string& dir, const std::string& flow_alg) {
  double StartTime = getCurrTimeSec();
  Mat im[4];
  for (int i = 0; i < 4; ++i) im[i] = readImage(dir + "/" + char(i + 49) + "." + g_input_ext);
  for (int i = 1; i < 4; ++i)
    if (im[i].rows != im[0].rows || im[i].cols != im[0].cols) throw VrCamException("4-input mode: the four photos must have the same size");
  const int rows = im[0].rows, cols = im[0].cols;
  for (int i = 0; i < 4; ++i)
    for (int x = 0; x < cols; ++x)
      if (!im[i].at<Vec4b>(rows / 2, x)[3])
        for (int y = 0; y < rows; ++y) im[i].at<Vec4b>(y, x) = Vec4b(0, 0, 0, 0);
  Mat colorImageL(rows, cols, CV_8UC4), colorImageR(rows, cols, CV_8UC4);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols * 4; ++x) {
      const int l = im[0].ptr<unsigned char>(y)[x] + im[2].ptr<unsigned char>(y)[x], r = im[1].ptr<unsigned char>(y)[x] + im[3].ptr<unsigned char>(y)[x];
      colorImageL.ptr<unsigned char>(y)[x] = (unsigned char)(l > 255 ? 255 : l);   // cv::Mat + cv::Mat on CV_8U saturates
      colorImageR.ptr<unsigned char>(y)[x] = (unsigned char)(r > 255 ? 255 : r);
    }
  Mat FinalResult = stitchStep(colorImageL, &colorImageR, flow_alg);
  writeResult(dir + "/FinalResult", FinalResult);
  std::cout << "TotalRunTime (sec) = " << (getCurrTimeSec() - StartTime) << std::endl;
  return EXIT_SUCCESS;
}

// the -test_dir flow for several directories, step i of all of them in one pf_stitch_step_batch call (frame k = directory k; the
// chain R_i = FinalResult_{i-1} of every directory stays in HBM)
static std::vector<std::string> splitDirs(const std::string& list) {
  std::vector<std::string> dirs;
  size_t b = 0;
  while (true) {
    const size_t e = list.find(',', b);
    const std::string d = list.substr(b, e == std::string::npos ? std::string::npos : e - b);
    if (d.empty()) throw VrCamException("-test_dirs: empty directory name in '" + list + "'");
    struct stat st;
    if (stat(d.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) throw VrCamException("-test_dirs: no such directory: " + d);
    dirs.push_back(d);
    if (e == std::string::npos) return dirs;
    b = e + 1;
  }
}
static int runBatchDirs(const std::vector<std::string>& dirs, const std::string& top_img, const std::string& flow_alg, int nsteps, int in_flight,
                        bool static_rig) {
  const int maxPct = pf_max_percentage_by_name(flow_alg.c_str());
  if (maxPct < 0) throw VrCamException("unrecognized flow algorithm name: " + flow_alg);
  double StartTime = getCurrTimeSec();
  const int n = (int)dirs.size();
  std::vector<Mat> tops(n), Ls(n), outs(n);
  Mat prev0;   // -static_rig: the first directory's previous composite, the R of its next plan
  for (int k = 0; k < n; ++k) tops[k] = readImage(dirs[k] + "/" + top_img);
  for (int i = 1; i <= nsteps; i++) {
    double StepStart = getCurrTimeSec();
    for (int k = 0; k < n; ++k) Ls[k] = readImage(dirs[k] + "/" + char(i + 48) + "." + g_input_ext);
    std::vector<const uint8_t*> l(n), r(n);
    std::vector<uint8_t*> o(n);
    for (int k = 0; k < n; ++k) {
      auto same = [&](const Mat& m) { return m.type() == CV_8UC4 && m.rows == Ls[0].rows && m.cols == Ls[0].cols && m.step == Ls[0].step; };
      if (!same(Ls[k]) || (i == 1 && !same(tops[k])))
        throw VrCamException("-test_dirs: every directory's images must be CV_8UC4 images of one size");
      // -png_device: the composites stay in their frame slots and are encoded there; only the one the next plan needs comes down
      const bool want = !(g_png_device || g_jpeg_device) || (static_rig && k == 0);
      outs[k] = want ? Mat(Ls[0].rows, Ls[0].cols, CV_8UC4) : Mat();
      l[k] = Ls[k].data; r[k] = tops[k].data; o[k] = want ? outs[k].data : nullptr;
    }
    const size_t ostep = size_t(Ls[0].cols) * 4;   // a fresh Mat's step
    if (static_rig) {
      // outs[0] was replaced above, prev0 still holds the first directory's composite of step i - 1
      StitchPlan plan(Ls[0], i == 1 ? &tops[0] : &prev0);
      const int rc = pf_stitch_step_batch_planned(pano::context(), plan.get(), n, l.data(), i == 1 ? r.data() : nullptr, Ls[0].cols, Ls[0].rows, Ls[0].step,
                                                  maxPct, o.data(), ostep, in_flight);
      if (rc != 0) {
        // the frame index is read out of the library's message: the wording "frame <k> differs from the stitch plan" is
        // report_plan_diff()'s in csrc/pf_api_stitch.inl (keep the two in step; tests/test_cli_stitch_static_rig.py pins both)
        const std::string msg = pf_last_error(pano::context());
        const size_t at = msg.find("frame ");
        int k = -1;
        if (at != std::string::npos && msg.find("differs from the stitch plan") != std::string::npos) k = atoi(msg.c_str() + at + 6);
        if (k >= 0 && k < n)
          throw VrCamException("-static_rig: step " + std::to_string(i) + ": the alpha masks of directory " + dirs[k] + " are not those of " + dirs[0] +
                               " (panoflow: " + msg + ")");
        throw VrCamException("panoflow: " + msg);
      }
    } else
    pano::check(pf_stitch_step_batch(pano::context(), n, l.data(), i == 1 ? r.data() : nullptr, Ls[0].cols, Ls[0].rows, Ls[0].step, maxPct,
                                     o.data(), ostep, in_flight));
    prev0 = outs[0];
    for (int k = 0; k < n; ++k) {
      const std::string stem = dirs[k] + "/" + (i == nsteps ? std::string("FinalResult") : std::string("ProcessResult") + char(i + 48));
      if (g_level || g_cube) writeReprojected(stem, pano_io::ResultSource::slot(k, Ls[0].cols, Ls[0].rows));
      if (g_level) continue;
      if (g_result_cols) writeResized(stem, [&](unsigned char* d) { return pf_stitch_batch_result_resized_dev(pano::context(), k, g_result_cols, g_result_rows, g_result_filter, d); });
      else if (g_jpeg_device) pano_io::write_jpeg_device(stem + ".jpg", pano::context(), g_jpeg, k, Ls[0].cols, Ls[0].rows);
      else if (g_png_device) pano_io::write_png_device(stem + ".png", pano::context(), k, Ls[0].cols, Ls[0].rows);
      else pano_io::imwriteExceptionOnFail(stem + ".png", outs[k]);
    }
    std::cout << "Part" << i << " Finished!" << "RUNTIME (sec) = " << (getCurrTimeSec() - StepStart) << std::endl;
  }
  std::cout << "TotalRunTime (sec) = " << (getCurrTimeSec() - StartTime) << std::endl;
  return EXIT_SUCCESS;
}

// -rig_chain 1: the whole chain of every directory in one call on one rig plan
static int runRigChain(const std::vector<std::string>& dirs, const std::string& top_img, const std::string& flow_alg, int nsteps, int in_flight) {
  const int maxPct = pf_max_percentage_by_name(flow_alg.c_str());
  if (maxPct < 0) throw VrCamException("unrecognized flow algorithm name: " + flow_alg);
  if (nsteps < 1 || nsteps > 9) throw VrCamException("-rig_chain: -steps must be 1..9");
  double StartTime = getCurrTimeSec();
  const int n = (int)dirs.size();
  std::vector<Mat> tops(n), Ls(size_t(n) * nsteps), outs(size_t(n) * nsteps);
  std::vector<const uint8_t*> t(n), l(size_t(n) * nsteps);
  std::vector<uint8_t*> o(size_t(n) * nsteps);
  for (int k = 0; k < n; ++k) {
    tops[k] = readImage(dirs[k] + "/" + top_img);
    for (int i = 0; i < nsteps; ++i) Ls[size_t(k) * nsteps + i] = readImage(dirs[k] + "/" + char(i + 49) + "." + g_input_ext);
  }
  auto same = [&](const Mat& m) { return m.type() == CV_8UC4 && m.rows == tops[0].rows && m.cols == tops[0].cols && m.step == tops[0].step; };
  for (int k = 0; k < n; ++k) {
    if (!same(tops[k])) throw VrCamException("-test_dirs: every directory's images must be CV_8UC4 images of one size");
    t[k] = tops[k].data;
    for (int i = 0; i < nsteps; ++i) {
      const size_t at = size_t(k) * nsteps + i;
      if (!same(Ls[at])) throw VrCamException("-test_dirs: every directory's images must be CV_8UC4 images of one size");
      outs[at] = Mat(tops[0].rows, tops[0].cols, CV_8UC4);
      l[at] = Ls[at].data; o[at] = outs[at].data;
    }
  }
  RigPlan rig(tops[0], std::vector<Mat>(Ls.begin(), Ls.begin() + nsteps));
  std::cout << "Rig plan of " << nsteps << " steps made!" << "RUNTIME (sec) = " << (getCurrTimeSec() - StartTime) << std::endl;
  const int rc = pf_rig_stitch_batch(pano::context(), rig.get(), n, t.data(), l.data(), tops[0].cols, tops[0].rows, tops[0].step, maxPct, o.data(),
                                     outs[0].step, in_flight);
  if (rc != 0) {
    // the frame and the step are read out of the library's message: the wording "frame <k> differs from the rig plan at step <i>" is
    // report_rig_diff()'s in csrc/pf_api_stitch.inl (keep the two in step; tests/test_cli_rig_chain.py pins both)
    const std::string msg = pf_last_error(pano::context());
    const size_t at = msg.find("frame "), st = msg.find("differs from the rig plan at step ");
    if (at != std::string::npos && st != std::string::npos) {
      const int k = atoi(msg.c_str() + at + 6), i = atoi(msg.c_str() + st + 34);
      if (k >= 0 && k < n)
        throw VrCamException("-rig_chain: step " + std::to_string(i) + ": the alpha masks of directory " + dirs[k] + " are not those of " + dirs[0] +
                             " (panoflow: " + msg + ")");
    }
    throw VrCamException("panoflow: " + msg);
  }
  tops.clear(); Ls.clear();   // the inputs are done with; every composite is released as soon as it is written
  for (int k = 0; k < n; ++k)
    for (int i = 1; i <= nsteps; ++i) {
      Mat& o_ki = outs[size_t(k) * nsteps + i - 1];
      if (i == nsteps) writeResult(dirs[k] + "/" + "FinalResult", o_ki);
      else writeResult(dirs[k] + "/" + "ProcessResult" + char(i + 48), o_ki);
      o_ki = Mat();
    }
  std::cout << "TotalRunTime (sec) = " << (getCurrTimeSec() - StartTime) << std::endl;
  return EXIT_SUCCESS;
}

// -rig_chain 1 -tiff_device 1: the same chains with every image in device memory.  Each input is decoded into its own pf_dev_alloc buffer,
// the rig plan is made from the first directory's device images, the chains run through pf_rig_stitch_batch_dev with a d_out per step, and
// each composite is encoded where it lies (-png_device 1) or downloaded for the default writer.
static int runRigChainDevice(const std::vector<std::string>& dirs, const std::string& top_img, const std::string& flow_alg, int nsteps, int in_flight) {
  const int maxPct = pf_max_percentage_by_name(flow_alg.c_str());
  if (maxPct < 0) throw VrCamException("unrecognized flow algorithm name: " + flow_alg);
  if (nsteps < 1 || nsteps > 9) throw VrCamException("-rig_chain: -steps must be 1..9");
  double StartTime = getCurrTimeSec();
  pf_ctx* ctx = tiffContext();
  const int n = (int)dirs.size();
  struct DevImages {   // frees what was allocated, however the run ends
    pf_ctx* ctx; std::vector<uint8_t*> p;
    ~DevImages() { for (uint8_t* q : p) if (q) pf_dev_free(ctx, q); }
  } dev{ctx, {}};
  std::vector<const uint8_t*> t(n), l(size_t(n) * nsteps);
  std::vector<uint8_t*> o(size_t(n) * nsteps);
  int cols = 0, rows = 0;
  // -lens_rig: a directory's raw photos wait in device buffers of their own until remapRaws() has made their canvases
  struct Raw { uint8_t* d; int cols, rows; pf_lens lens; uint8_t* canvas; };
  std::vector<Raw> raws;
  DevImages raw_dev{ctx, {}};
  // JPEG photos: their bytes wait on the host until remapRaws() decodes those of one size in one call, into their raw buffers
  struct Jpeg { std::vector<unsigned char> bytes; uint8_t* d; int cols, rows; std::string path; };
  std::vector<Jpeg> jpegs;
  auto load = [&](const std::string& path) {
    int c = 0, r = 0;
    if (!g_lens_rig.empty()) {
      if (isJpegName(path)) {
        pf_jpeg_info info;
        std::vector<unsigned char> b = readJpegFile(path, &info);
        c = info.cols; r = info.rows;
        uint8_t* d = (uint8_t*)pf_dev_alloc(ctx, size_t(c) * r * 4);
        if (!d) throw VrCamException(std::string("panoflow: ") + pf_last_error(ctx));
        raw_dev.p.push_back(d);
        jpegs.push_back(Jpeg{std::move(b), d, c, r, path});
      } else {
        raw_dev.p.push_back(pano_io::imread_to_device(path, ctx, &c, &r));
      }
      cols = g_canvas_cols; rows = g_canvas_rows;
      uint8_t* canvas = (uint8_t*)pf_dev_alloc(ctx, size_t(cols) * rows * 4);
      if (!canvas) throw VrCamException(std::string("panoflow: ") + pf_last_error(ctx));
      dev.p.push_back(canvas);
      raws.push_back(Raw{raw_dev.p.back(), c, r, lensOf(path, c, r), canvas});
      return canvas;
    }
    dev.p.push_back(pano_io::imread_to_device(path, ctx, &c, &r));
    if (cols == 0) { cols = c; rows = r; }
    if (c != cols || r != rows) throw VrCamException("-test_dirs: every directory's images must be CV_8UC4 images of one size");
    return dev.p.back();
  };
  // the waiting photos onto their canvases, the photos of one size in one call (a rig's cameras: one launch), then the photos freed
  auto remapRaws = [&]() {
    {
      std::vector<bool> decoded(jpegs.size(), false);
      for (size_t a = 0; a < jpegs.size(); ++a) {
        if (decoded[a]) continue;
        std::vector<const uint8_t*> files; std::vector<size_t> sizes; std::vector<uint8_t*> dst; std::string names;
        for (size_t b = a; b < jpegs.size(); ++b)
          if (!decoded[b] && jpegs[b].cols == jpegs[a].cols && jpegs[b].rows == jpegs[a].rows) {
            files.push_back(jpegs[b].bytes.data()); sizes.push_back(jpegs[b].bytes.size()); dst.push_back(jpegs[b].d); decoded[b] = true;
            names += " " + std::to_string(files.size() - 1) + "=" + jpegs[b].path;
          }
        if (pf_jpeg_decode_batch_dev(ctx, (int)files.size(), files.data(), sizes.data(), jpegs[a].cols, jpegs[a].rows, dst.data()) != 0)
          throw VrCamException(std::string("panoflow: ") + pf_last_error(ctx) + " (files:" + names + ")");
      }
      jpegs.clear();
    }
    std::vector<bool> done(raws.size(), false);
    for (size_t a = 0; a < raws.size(); ++a) {
      if (done[a]) continue;
      std::vector<const uint8_t*> src; std::vector<uint8_t*> dst; std::vector<pf_lens> lenses;
      for (size_t b = a; b < raws.size(); ++b)
        if (!done[b] && raws[b].cols == raws[a].cols && raws[b].rows == raws[a].rows) { src.push_back(raws[b].d); dst.push_back(raws[b].canvas); lenses.push_back(raws[b].lens); done[b] = true; }
      pano::check(pf_lens_remap_batch_dev(ctx, (int)src.size(), src.data(), raws[a].cols, raws[a].rows, dst.data(), cols, rows, lenses.data()));
    }
    for (uint8_t*& q : raw_dev.p) { pf_dev_free(ctx, q); q = nullptr; }
    raw_dev.p.clear(); raws.clear();
  };
  for (int k = 0; k < n; ++k) {
    t[k] = load(dirs[k] + "/" + top_img);
    for (int i = 0; i < nsteps; ++i) l[size_t(k) * nsteps + i] = load(dirs[k] + "/" + char(i + 49) + "." + g_input_ext);
    remapRaws();
  }
  for (size_t at = 0; at < o.size(); ++at) {
    o[at] = (uint8_t*)pf_dev_alloc(ctx, size_t(cols) * rows * 4);
    if (!o[at]) throw VrCamException(std::string("panoflow: ") + pf_last_error(ctx));
    dev.p.push_back(o[at]);
  }
  pf_rig_plan* rig = nullptr;
  pano::check(pf_rig_plan_create_dev(ctx, nsteps, t[0], l.data(), cols, rows, &rig));
  std::cout << "Rig plan of " << nsteps << " steps made!" << "RUNTIME (sec) = " << (getCurrTimeSec() - StartTime) << std::endl;
  const int rc = pf_rig_stitch_batch_dev(ctx, rig, n, t.data(), l.data(), cols, rows, maxPct, o.data(), in_flight);
  const std::string msg = rc != 0 ? pf_last_error(ctx) : "";
  pf_rig_plan_destroy(ctx, rig);
  if (rc != 0) {
    // the same wording as runRigChain's: "frame <k> differs from the rig plan at step <i>" is report_rig_diff()'s (tests/test_cli_rig_chain.py pins both)
    const size_t at = msg.find("frame "), st = msg.find("differs from the rig plan at step ");
    if (at != std::string::npos && st != std::string::npos) {
      const int k = atoi(msg.c_str() + at + 6), i = atoi(msg.c_str() + st + 34);
      if (k >= 0 && k < n)
        throw VrCamException("-rig_chain: step " + std::to_string(i) + ": the alpha masks of directory " + dirs[k] + " are not those of " + dirs[0] +
                             " (panoflow: " + msg + ")");
    }
    throw VrCamException("panoflow: " + msg);
  }
  for (int k = 0; k < n; ++k)
    for (int i = 1; i <= nsteps; ++i) {
      const uint8_t* d = o[size_t(k) * nsteps + i - 1];
      const std::string path = dirs[k] + "/" + (i == nsteps ? std::string("FinalResult.png") : std::string("ProcessResult") + char(i + 48) + ".png");
      if (g_level || g_cube) writeReprojected(path.substr(0, path.size() - 4), pano_io::ResultSource::device(d, cols, rows));
      if (g_level) continue;
      if (g_result_cols) {
        writeResized(path.substr(0, path.size() - 4), [&](unsigned char* dst) { return pf_resize_dev(ctx, d, cols, rows, dst, g_result_cols, g_result_rows, g_result_filter); });
      } else if (g_jpeg_device) {
        pano_io::write_jpeg_device(path.substr(0, path.size() - 4) + ".jpg", ctx, g_jpeg, d, cols, rows);
      } else if (g_png_device) {
        pano_io::write_png_bytes(path, ctx, cols, rows, [&](unsigned char* b, size_t cap, size_t* size) { return pf_png_encode_dev(ctx, d, cols, rows, b, cap, size); });
      } else {
        Mat m(rows, cols, CV_8UC4);
        for (int y = 0; y < rows; ++y) pano::check(pf_download(ctx, m.ptr<unsigned char>(y), d + size_t(y) * cols * 4, size_t(cols) * 4));
        pano_io::imwriteExceptionOnFail(path, m);
      }
    }
  std::cout << "TotalRunTime (sec) = " << (getCurrTimeSec() - StartTime) << std::endl;
  return EXIT_SUCCESS;
}

int main(int argc, char** argv) {
  try {
    auto flags = parseFlags(argc, argv);
    g_png_device = flags.count("png_device") && atoi(flags["png_device"].c_str()) != 0;
    g_jpeg_device = flags.count("jpeg_device") && atoi(flags["jpeg_device"].c_str()) != 0;
    pf_jpeg_params_init(&g_jpeg);
    if (g_jpeg_device) {   // every refusal before any device call
      if (flags.count("jpeg_quality")) g_jpeg.quality = atoi(flags["jpeg_quality"].c_str());
      if (g_jpeg.quality < 1 || g_jpeg.quality > 100) throw VrCamException("-jpeg_quality must be 1..100");
      const std::string sub = flags.count("jpeg_subsampling") ? flags["jpeg_subsampling"] : "420";
      if (sub != "444" && sub != "420") throw VrCamException("-jpeg_subsampling must be 444 or 420");
      g_jpeg.subsampling = sub == "420";
      g_jpeg.gpano = flags.count("jpeg_gpano") && atoi(flags["jpeg_gpano"].c_str()) != 0;
    }
    if (flags.count("result_size")) {   // every refusal before any device call
      char tail = 0;
      if (sscanf(flags["result_size"].c_str(), "%dx%d%c", &g_result_cols, &g_result_rows, &tail) != 2 || g_result_cols <= 0 || g_result_rows <= 0)
        throw VrCamException("-result_size must be WxH with both positive, e.g. 4096x2048");
      if (!g_png_device && !g_jpeg_device) throw VrCamException("-result_size needs -png_device 1 or -jpeg_device 1 (the results are resized and encoded on the GPU)");
      const std::string name = flags.count("result_filter") ? flags["result_filter"] : "lanczos";
      const std::map<std::string, int> filters = {{"lanczos", PF_RESIZE_LANCZOS}, {"bicubic", PF_RESIZE_BICUBIC}, {"bilinear", PF_RESIZE_BILINEAR},
                                                  {"hamming", PF_RESIZE_HAMMING}, {"box", PF_RESIZE_BOX}};
      if (!filters.count(name)) throw VrCamException("-result_filter must be lanczos, bicubic, bilinear, hamming or box");
      g_result_filter = filters.at(name);
      if (g_jpeg_device && g_jpeg.gpano && g_result_cols != 2 * g_result_rows) throw VrCamException("-jpeg_gpano 1 declares a full sphere, which -result_size " + flags["result_size"] + " (not 2:1) is not");
    } else if (flags.count("result_filter")) throw VrCamException("-result_filter needs -result_size WxH");
    if (flags.count("level")) {   // every refusal before any device call
      double ypr[3];
      char tail = 0;
      if (sscanf(flags["level"].c_str(), "%lf,%lf,%lf%c", &ypr[0], &ypr[1], &ypr[2], &tail) != 3 || !std::isfinite(ypr[0]) || !std::isfinite(ypr[1]) || !std::isfinite(ypr[2]))
        throw VrCamException("-level must be yaw,pitch,roll in degrees, e.g. 0,-2.5,1");
      if (!g_png_device && !g_jpeg_device) throw VrCamException("-level needs -png_device 1 or -jpeg_device 1 (the results are turned and encoded on the GPU)");
      pf_reproject_rotation(ypr[0], ypr[1], ypr[2], g_level_rot);
      g_level = true;
    }
    if (flags.count("cube")) {
      char tail = 0;
      if (sscanf(flags["cube"].c_str(), "%d%c", &g_cube, &tail) != 1 || g_cube <= 0 || g_cube > 65535) throw VrCamException("-cube must be the faces' size N, 1..65535");
      if (!g_png_device && !g_jpeg_device) throw VrCamException("-cube needs -png_device 1 or -jpeg_device 1 (the faces are cut and encoded on the GPU)");
      const std::string name = flags.count("cube_filter") ? flags["cube_filter"] : "bicubic";
      if (name != "bicubic" && name != "bilinear") throw VrCamException("-cube_filter must be bicubic or bilinear");
      g_cube_filter = name == "bicubic" ? PF_REPROJECT_BICUBIC : PF_REPROJECT_BILINEAR;
    } else if (flags.count("cube_filter")) throw VrCamException("-cube_filter needs -cube N");
    if (flags.count("lens_rig") || flags.count("canvas")) {   // every refusal before any device call
      if (!flags.count("lens_rig") || !flags.count("canvas")) throw VrCamException("-lens_rig FILE and -canvas WxH go together");
      char tail = 0;
      if (sscanf(flags["canvas"].c_str(), "%dx%d%c", &g_canvas_cols, &g_canvas_rows, &tail) != 2 || g_canvas_cols <= 0 || g_canvas_rows <= 0 || g_canvas_cols > 65535 || g_canvas_rows > 65535)
        throw VrCamException("-canvas must be WxH with both 1..65535, e.g. 9000x4000");
      g_lens_rig_file = flags["lens_rig"];
      FILE* f = fopen(g_lens_rig_file.c_str(), "rb");
      if (!f) throw VrCamException("-lens_rig: cannot read " + g_lens_rig_file);
      std::string text;
      char buf[4096];
      for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
      fclose(f);
      try { g_lens_rig = lens_rig::parse(text); }
      catch (const lens_rig::ParseError& e) { throw VrCamException("-lens_rig: " + g_lens_rig_file + ": " + e.what()); }
      if (g_lens_rig.empty()) throw VrCamException("-lens_rig: " + g_lens_rig_file + " describes no image (no `i` line)");
    }
    if (flags.count("input_ext")) {   // (refused before any device call)
      g_input_ext = flags["input_ext"];
      if (g_input_ext != "tif" && g_input_ext != "jpg") throw VrCamException("-input_ext must be tif or jpg");
      if (g_input_ext == "jpg" && g_lens_rig.empty())
        throw VrCamException("-input_ext jpg needs -lens_rig FILE and -canvas WxH (a JPEG has no alpha; the remap makes the masks)");
    }
    g_tiff_device = flags.count("tiff_device") && atoi(flags["tiff_device"].c_str()) != 0;
    g_tiff_inflate = flags.count("tiff_inflate") && atoi(flags["tiff_inflate"].c_str()) != 0;   // (read only on the -tiff_device 1 paths)
    if (flags.count("test_dirs")) {   // every refusal before any device call
      if (flags.count("test_dir")) throw VrCamException("-test_dirs and -test_dir are exclusive");
      const bool static_rig = flags.count("static_rig") && atoi(flags["static_rig"].c_str()) != 0;
      const bool rig_chain = flags.count("rig_chain") && atoi(flags["rig_chain"].c_str()) != 0;
      if (rig_chain && !static_rig) throw VrCamException("-rig_chain 1 needs -static_rig 1 (it plans the whole chain of one rig)");
      if (flags.count("fused") && atoi(flags["fused"].c_str()) == 0) throw VrCamException("-test_dirs runs the fused step only (-fused 0 is not supported)");
      if (flags.count("visualize") && atoi(flags["visualize"].c_str()) != 0) throw VrCamException("-test_dirs does not support -visualize 1");
      if (flags.count("inputs")) throw VrCamException("-test_dirs does not support -inputs");
      if (flags["test_dirs"].empty()) throw VrCamException("-test_dirs: empty directory list");
      const std::vector<std::string> dirs = splitDirs(flags["test_dirs"]);
      requireArg(flags["top_img"], "top_img");
      requireArg(flags["flow_alg"], "flow_alg");
      const int nsteps = flags.count("steps") ? atoi(flags["steps"].c_str()) : 5;
      const int in_flight = flags.count("in_flight") ? atoi(flags["in_flight"].c_str()) : 8;
      if (in_flight < 1 || in_flight > 32) throw VrCamException("-in_flight must be 1..32");
      if (rig_chain && g_tiff_device) return runRigChainDevice(dirs, flags["top_img"], flags["flow_alg"], nsteps, in_flight);
      if (rig_chain) return runRigChain(dirs, flags["top_img"], flags["flow_alg"], nsteps, in_flight);
      return runBatchDirs(dirs, flags["top_img"], flags["flow_alg"], nsteps, in_flight, static_rig);
    }
    if (flags.count("static_rig") && atoi(flags["static_rig"].c_str()) != 0) throw VrCamException("-static_rig 1 needs -test_dirs (it plans the batched step)");
    if (flags.count("rig_chain") && atoi(flags["rig_chain"].c_str()) != 0) throw VrCamException("-rig_chain 1 needs -test_dirs ... -static_rig 1");
    const std::string FLAGS_test_dir = flags["test_dir"], FLAGS_top_img = flags["top_img"], FLAGS_flow_alg = flags["flow_alg"];
    const int nsteps = flags.count("steps") ? atoi(flags["steps"].c_str()) : 5;
    const bool fused = !flags.count("fused") || atoi(flags["fused"].c_str()) != 0;   // -fused 0: the reference's object-by-object sequence
    const bool visualize = flags.count("visualize") && atoi(flags["visualize"].c_str()) != 0;
    if (flags.count("inputs") && atoi(flags["inputs"].c_str()) == 4) {
      requireArg(FLAGS_test_dir, "test_dir");
      requireArg(FLAGS_flow_alg, "flow_alg");
      return run4Input(FLAGS_test_dir, FLAGS_flow_alg);
    }
    double StartTime = getCurrTimeSec();
    requireArg(FLAGS_test_dir, "test_dir");
    requireArg(FLAGS_top_img, "top_img");
    requireArg(FLAGS_flow_alg, "flow_alg");

    Mat colorImageL, colorImageR, FinalResult;
    Mat colorImageT = readImage(FLAGS_test_dir + "/" + FLAGS_top_img);
    if (visualize && mkdir((FLAGS_test_dir + "/disparity").c_str(), 0777) != 0 && errno != EEXIST)
      throw VrCamException("cannot create " + FLAGS_test_dir + "/disparity");
    for (int i = 1; i <= nsteps; i++) {
      double StepStart = getCurrTimeSec();
      if (i == 1) colorImageR = colorImageT; else colorImageR = FinalResult;
      colorImageL = readImage(FLAGS_test_dir + "/" + char(i + 48) + "." + g_input_ext);

      if (fused && (g_png_device || g_jpeg_device)) {
        // the composite stays in HBM (out_bgra = NULL) for the next step to chain on and for the encoder: only its PNG or JPEG comes down
        const int maxPct = pf_max_percentage_by_name(FLAGS_flow_alg.c_str());
        if (maxPct < 0) throw VrCamException("unrecognized flow algorithm name: " + FLAGS_flow_alg);
        if (colorImageL.type() != CV_8UC4 || (i == 1 && (colorImageR.type() != CV_8UC4 || colorImageR.rows != colorImageL.rows ||
                                                         colorImageR.cols != colorImageL.cols || colorImageR.step != colorImageL.step)))
          throw VrCamException("stitchStep: inputs must be CV_8UC4 images of equal size");
        pano::check(pf_stitch_step(pano::context(), colorImageL.data, i == 1 ? colorImageR.data : nullptr, colorImageL.cols, colorImageL.rows,
                                   colorImageL.step, maxPct, nullptr, 0));
        if (visualize) stitchVisualizations(colorImageL.cols, colorImageL.rows, FLAGS_test_dir, FLAGS_flow_alg, i);
      } else if (fused) {
        // same kernels, same results; the step's intermediates and the chained R stay in HBM
        FinalResult = stitchStep(colorImageL, i == 1 ? &colorImageR : nullptr, FLAGS_flow_alg);
        if (visualize) stitchVisualizations(colorImageL.cols, colorImageL.rows, FLAGS_test_dir, FLAGS_flow_alg, i);
      } else {
      Stitchtools Stools;
      Stools.prepare(colorImageL, colorImageR);
      Mat overlappedL = Stools.getOverlappedL();
      Mat overlappedR = Stools.getOverlappedR();
      Mat blend = Stools.getBlend();

      NovelViewGenerator* novelViewGen = new NovelViewGeneratorAsymmetricFlow(FLAGS_flow_alg);
      novelViewGen->prepare(overlappedL, overlappedR);

      if (visualize) buildvisualizations(novelViewGen->getFlowLtoR(), novelViewGen->getFlowRtoL(), colorImageL, colorImageR, FLAGS_test_dir, FLAGS_flow_alg, i);
      novelViewGen->setBlend(blend);
      Mat novelViewMerged = Mat();
      novelViewGen->generateNovelView(novelViewMerged);

      Stools.setMergedmiddle(novelViewMerged);
      Stools.Gather();
      FinalResult = Stools.getFinalResult();
      delete novelViewGen;
      }

      const std::string resultStem = FLAGS_test_dir + "/" + (i == nsteps ? std::string("FinalResult") : std::string("ProcessResult") + char(i + 48));
      const bool resident = fused && (g_png_device || g_jpeg_device);   // the composite lies in HBM, not in FinalResult
      if (resident && (g_level || g_cube)) writeReprojected(resultStem, pano_io::ResultSource::resident(colorImageL.cols, colorImageL.rows));
      if (resident && g_level) {}   // written above: the turned composite is the result
      else if (fused && g_result_cols) writeResized(resultStem, [&](unsigned char* d) { return pf_stitch_result_resized_dev(pano::context(), g_result_cols, g_result_rows, g_result_filter, d); });
      else if (fused && g_jpeg_device) pano_io::write_jpeg_device(resultStem + ".jpg", pano::context(), g_jpeg, colorImageL.cols, colorImageL.rows);
      else if (fused && g_png_device) pano_io::write_png_device(resultStem + ".png", pano::context(), colorImageL.cols, colorImageL.rows);
      else writeResult(resultStem, FinalResult);
      std::cout << "Part" << i << " Finished!" << "RUNTIME (sec) = " << (getCurrTimeSec() - StepStart) << std::endl;
    }
    std::cout << "TotalRunTime (sec) = " << (getCurrTimeSec() - StartTime) << std::endl;
    return EXIT_SUCCESS;
  } catch (const VrCamException& e) {
    std::cerr << "VrCamException: " << e.what() << std::endl;   // the reference's terminate handler prints and aborts (util.cpp:59-78)
    return EXIT_FAILURE;
  }
}
