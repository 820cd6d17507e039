// C-ABI implementation (include/panoflow.h): context, HBM arena, orchestration of the kernel families
// on HIP streams.  Host code only launches kernels and moves data; all pixel arithmetic is in the
// kernels_*.hip files.  There is no CPU fallback anywhere in this library.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/panoflow.h"
#include "pf_common.hpp"
#include "png_frame.hpp"
#include "jpeg_frame.hpp"
#include "tiff_parse.hpp"
#include "jpeg_parse.hpp"
#include "resize_table.hpp"

using namespace pf;


// One translation unit in sixteen parts (the anonymous namespace and the extern "C" block span several of them):
#include "pf_api_ctx.inl"      // pf_ctx, errors / warnings, arena, profiling events, geometry, checks
#include "pf_api_solve.inl"    // run_level, solve buffers, solve / solve_n (stream orchestration)
#include "pf_api_life.inl"     // finish / CallGuard, pf_create* / pf_destroy, memory helpers            (opens extern "C")
#include "pf_api_entry.inl"    // pf_flow* / pf_blend* / pf_novel_view* incl. the throughput mode
#include "pf_api_stitch.inl"   // pf_stitch_* but the plans: lone calls, the chain step and its prefetch, the batched step
#include "pf_api_plan.inl"     // pf_stitch_plan_*, pf_rig_plan_*, pf_rig_stitch* (stitch plans, rig plans, the rig chain)
#include "pf_api_image.inl"    // shared by the file-and-image parts below: resident results, device-image checks, host-image staging, resident tables
#include "pf_api_stage.inl"    // pf_stage_*, pf_profile_*, pf_level_pixels / pf_algorithmic_bytes
#include "pf_api_vis.inl"      // pf_vis_*, pf_stitch_visualize (flow visualisers)
#include "pf_api_png.inl"      // pf_png_*, pf_stitch_result_png (PNG files made on the device)
#include "pf_api_tiff.inl"     // pf_tiff_* (TIFF files decoded on the device)
#include "pf_api_jpeg.inl"     // pf_jpeg_*, pf_stitch_result_jpeg (JPEG files made on the device)
#include "pf_api_jpegd.inl"    // pf_jpeg_probe, pf_jpeg_decode* (JPEG files decoded on the device)
#include "pf_api_resize.inl"   // pf_resize*, pf_stitch_result_resized_dev (Pillow's resample on the device)
#include "pf_api_reproject.inl"   // pf_reproject*, pf_stitch_result_reprojected_dev (cube faces, views, a turned sphere)
#include "pf_api_lens.inl"        // pf_lens_* (raw photos of a rig remapped onto the canvas: fisheye and rectilinear lenses)
}  // extern "C"

