// trik_hsv_preview_tasks.h -- the task split of the previews that read a range
// per frame (trik_hsv_frame_ranges_preview.hip, DESIGN.md 4.13;
// trik_hsv_line_frame_ranges_preview.hip, 4.14): a wave takes one task at a
// time, 64 consecutive units of ONE frame, tasks round robin over the grid's
// waves, so the frame index -- and with it the frame's range -- is
// wave-uniform.  The geometry a kernel reads, the grid, and the launch.
#pragma once

#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"

namespace trik_hsv {

namespace {

constexpr int kFpBlock = 256;                // 4 waves; 1 KiB of LUTs per workgroup
constexpr int kFpWaves = kFpBlock / 64;
constexpr int kFpBlocksPerCu = 8;            // the grid: 8 waves per SIMD
constexpr int kFpQ = 2;                      // gather: output groups per lane and task
constexpr int64_t kFpMapLdsBytes = 32 * 1024;  // gather: maps up to this size are staged in LDS

struct FrPreviewGeom {
  const uint16_t* ranges;  // frame f's six-tuple at ranges + f * range_stride (entry t already added)
  uint32_t range_stride;   // 6 * n_ranges
  FastDiv segs;            // tasks per frame
  FastDiv per_row;         // units (2:1) or 4-byte groups (gather) per output row
  uint32_t per_frame;      // out_h * per_row.d
  uint32_t tasks;          // n_frames * segs.d, < 2^31
  uint32_t maps_lds;       // gather: the inverse maps are staged in LDS
};

using FpKernel = void (*)(PreviewArgs, FrPreviewGeom);

// `per_frame` units of `per_row` a row, 64 * per_task of them a task
int launch_tasks(FpKernel kern, const PreviewArgs& a, FrPreviewGeom g, int64_t per_row, int per_task, size_t lds,
                 hipStream_t s) {
  const int64_t per_frame = a.out_h * per_row, segs = (per_frame + 64 * per_task - 1) / (64 * per_task);
  g.per_row = make_div((uint32_t)per_row);
  g.per_frame = (uint32_t)per_frame;
  g.segs = make_div((uint32_t)segs);
  g.tasks = (uint32_t)(a.n_frames * segs);  // <= n_frames * per_frame < 2^31
  const int64_t blocks = ((int64_t)g.tasks + kFpWaves - 1) / kFpWaves, slots = (int64_t)kFpBlocksPerCu * device_cus();
  hipLaunchKernelGGL(kern, dim3((unsigned)(blocks < slots ? blocks : slots)), dim3(kFpBlock), lds, s, a, g);
  return hipGetLastError();
}

}  // namespace

}  // namespace trik_hsv
