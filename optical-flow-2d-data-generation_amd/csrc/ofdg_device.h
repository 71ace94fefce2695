// Device-side records of the render pipeline (host realize -> geom -> raster ->
// compose).  Plain PODs shared by host code and HIP kernels.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/ofdg_detmath.h"
#include "../../include/ofdg.h"  // the ABI: each Dev* record below that restates one of its structs is held to it next to its definition

// Marks a function shared by host code and kernels (this header, realize.h): the pattern of OFDG_DM_FN
// (include/ofdg_detmath.h); plain inline in a C++ translation unit.  always_inline: the device code then is what it was when
// the device had copies of its own, written inline (profiles/shared_realize_device_code.txt).
#if defined(__HIPCC__) || defined(__HIP__)
#define OFDG_HD_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define OFDG_HD_FN inline
#endif

namespace ofdg {

constexpr int kMaxSegments = 20;    // OFDG_MAX_SEGMENTS
constexpr int kMaxComponents = 8;   // OFDG_MAX_COMPONENTS
constexpr int kMaxVerts = 1024;     // flattened outline capacity per (shape, frame)
constexpr int kCurveMaxPts = 96;    // points one curve3 may flatten to
constexpr int kCurveMaxDepth = 16;  // DFS stack depth for curve3 subdivision
constexpr int kBandRows = 8;        // scanlines one raster workgroup accumulates in LDS
constexpr int kMaxFgObjects = 64;   // foreground objects per sample (bits of a tile mask)
constexpr int kRasterGrid = 512;    // x4 persistent single-wave raster workgroups: enough to finish in time, few enough not to crowd compose
// ... and of a launch that rasterises two batches of a chain (the paired front end; profiles/paired_front_raster_grid.txt)
#ifndef OFDG_RASTER_GRID_PAIRED
#define OFDG_RASTER_GRID_PAIRED 768
#endif
constexpr int kRasterGridPaired = OFDG_RASTER_GRID_PAIRED;
// ... and three or four (ofdg_set_front_batches; profiles/front_n_raster_grid.txt).  15 waves of 10.2 KB LDS fit a
// CU, 960 x 4 on the device: the waves beyond them start as the first ones finish their share of the list.
#ifndef OFDG_RASTER_GRID_3
#define OFDG_RASTER_GRID_3 1536
#endif
#ifndef OFDG_RASTER_GRID_4
#define OFDG_RASTER_GRID_4 1536
#endif
constexpr int kMaxFrontBatches = 4;  // batches of a chain one sampler -> geom -> raster launch may serve
constexpr int kRasterGridFront[kMaxFrontBatches + 1] = {kRasterGrid, kRasterGrid, kRasterGridPaired, OFDG_RASTER_GRID_3, OFDG_RASTER_GRID_4};
// ... of which the FIRST group a chain launches after a start or a discard holds at most this many.  4: every group is N.  2
// ("first a pair": a shorter fill, fewer parts nobody asks for at the end of a short run) measured worse at N = 4 in a 20-step
// run and better at N = 3 (profiles/front_n_ab.txt).
#ifndef OFDG_FRONT_FIRST_GROUP
#define OFDG_FRONT_FIRST_GROUP 4
#endif
constexpr int kFrontFirstGroup = OFDG_FRONT_FIRST_GROUP;
// ... and a new context's setting (profiles/front_n_ab.txt)
#ifndef OFDG_FRONT_DEFAULT
#define OFDG_FRONT_DEFAULT 4
#endif
constexpr int kFrontDefault = OFDG_FRONT_DEFAULT;

// error bits raised by kernels (device word, read by ofdg_synchronize)
constexpr uint32_t kErrVertCapacity = 1u;   // outline has more than kMaxVerts vertices
constexpr uint32_t kErrCurveCapacity = 2u;  // a curve exceeded kCurveMaxPts / kCurveMaxDepth
constexpr uint32_t kErrDxLimit = 4u;        // an edge spans >= 16384 px (AGG dx_limit)
constexpr uint32_t kErrBgPrepCapacity = 8u; // background_prep: a crop of the rotated image exceeds the workspace (zoom < 0.75)

// A slot filled for up to kMaxFrontBatches batches of a chain in equal parts: what belongs to the part element i is in (its
// error word, its offset).  Compares and selects, no division: i and part are wave-uniform where this is used, so it stays scalar.
template <typename T>
OFDG_HD_FN T front_pick(int i, int part, T p0, T p1, T p2, T p3) {
  return i < part ? p0 : (i < 2 * part ? p1 : (i < 3 * part ? p2 : p3));
}

// 2x3 affine in AGG's member order (sx, shy, shx, sy, tx, ty), fp64.
struct Mat {
  double sx, shy, shx, sy, tx, ty;
};

// One rasterised outline: an ellipse or polygon blueprint (top-level object or a
// component of a composite) with its two outline transforms.
// Reference: MovingObjectEllipse/Polygon::renderMasks, DataGenerator.cpp:465-479, 520-534.
struct DevShape {
  Mat m[2];        // frame 0: intrinsic; frame 1: intrinsic * motion
  float seg_x[kMaxSegments];
  float seg_y[kMaxSegments];
  int32_t seg_type[kMaxSegments];
  float rx, ry;    // ellipse radii
  int32_t type;    // 1 ellipse, 2 polygon
  int32_t n_seg;
  int32_t sample;  // batch slot
  int32_t deform;  // mode 9: frame-1 mask is re-sampled through warp slot `deform-1`
  int32_t object;  // index of the owning DevObject in the batch
  int32_t obj_local;  // index of the owner among its sample's foreground objects (bit of the block masks)
};

// Produced by the geom kernel for each (shape, frame).
struct DevShapeFrame {
  int32_t n_verts;
  int32_t x0, y0, x1, y1;  // pixel bbox clipped to the screen, inclusive; empty: x0 > x1
  int32_t pad[3];
};

// One blitted object (background or top-level foreground object), in z-order.
// Reference: RenderCore::blitObject / getPointFlow, DataGenerator.cpp:762-799, 388-407, 692-718.
struct DevObject {
  Mat motion;         // m_motion (fg: incl. background motion)
  Mat tex_inv;        // inverse of the texture warp transform (getTransformedTexture, :203-205)
  uint64_t tex_base;  // texel offset of the pool image's crop origin
  int32_t first_shape;
  int32_t n_shapes;   // 0 background, 1 simple shape, >=1 composite
  uint32_t additive;  // bit k: component k is additive (composite only)
  int32_t kind;       // 0 background, 1 simple, 2 composite
  int32_t id;
  int32_t deform;     // mode 9: warp slot + 1, 0 = rigid
  int32_t pad[2];
};
static_assert(sizeof(DevObject) == 136, "record layout is read dword-wise by compose");

// The sample record is self-contained for the background: compose reads it with ONE scalar load batch (the
// background's DevObject at objects[first_object] holds the same matrices; the mode-9 kernels use that one).
struct DevSample {
  int32_t first_object;  // background first, then foreground objects by ascending ID
  int32_t n_objects;
  int32_t first_shape;
  int32_t n_shapes;
  Mat bg_motion;         // = objects[first_object].motion
  Mat bg_tex_inv;        // = objects[first_object].tex_inv
  uint64_t bg_tex_base;  // = objects[first_object].tex_base
  int32_t bg_deform;
  int32_t pad;
  // foreground object k (bit k of the block masks): first outline slot relative to first_shape; bit 15 = composite.
  // In the same record as the matrices above: by the time a wave knows its block's objects these lines are in the
  // scalar cache, and the coverage of a simple object can be fetched without first reading the object's own record.
  uint16_t shape_of[kMaxFgObjects];
};
static_assert(sizeof(DevSample) == 256, "compose reads the sample record as 128 + 128 bytes");
constexpr uint16_t kShapeComposite = 0x8000u;

// The tail of a DevObject as compose reads it ahead of a visit (one 32-byte scalar load at offset 96).
struct DevObjectHdr {
  uint64_t tex_base;
  int32_t first_shape, n_shapes;
  uint32_t additive;
  int32_t kind, id, deform;
};

// One row of the per-object annotation table (ofdg_object_row of include/ofdg.h, field for field): the kernels update the
// int32 fields of a frame with atomics, so area and box are arrays over the frame here.
struct DevObjectRow {
  int32_t obj_id, obj_type;
  int32_t area[2];    // [frame]
  int32_t box[2][4];  // [frame]{x0, y0, x1, y1}
  double motion[6];
};
constexpr int kObjectRows = kMaxFgObjects + 1;  // OFDG_MAX_OBJECT_ROWS: background + foreground objects
static_assert(sizeof(ofdg_object_row) == sizeof(DevObjectRow) && sizeof(DevObjectRow) == 96 && offsetof(ofdg_object_row, area0) == offsetof(DevObjectRow, area) &&
              offsetof(ofdg_object_row, box0) == offsetof(DevObjectRow, box) && offsetof(ofdg_object_row, box1) == offsetof(DevObjectRow, box) + 16 &&
              offsetof(ofdg_object_row, motion) == offsetof(DevObjectRow, motion) && OFDG_MAX_OBJECT_ROWS == kObjectRows,
              "ofdg_object_row: 96 bytes without padding, the layout the kernels write; background + kMaxFgObjects rows");

// ---- Caller-given planes (ofdg_flow_stats, ofdg_flow_pyramid, ofdg_crop and their host twins) ------------------------------
// The element types are the codes of include/ofdg.h: OFDG_FMT_F32, OFDG_FMT_U8, OFDG_FMT_F16.
OFDG_HD_FN int fmt_elem_bytes(int fmt) { return fmt == OFDG_FMT_F32 ? 4 : fmt == OFDG_FMT_U8 ? 1 : 2; }
inline const char* fmt_name(int fmt) { return fmt == OFDG_FMT_F32 ? "float32" : fmt == OFDG_FMT_U8 ? "uint8" : "binary16"; }
// What the device entries ask of an input plane's base: a lane reads four elements at once (16, 4 or 8 bytes).
inline int plane_alignment(int fmt) { return 4 * fmt_elem_bytes(fmt); }
inline bool plane_misaligned(const void* p, int fmt) { return (uintptr_t)p & (uintptr_t)(plane_alignment(fmt) - 1); }
// The rules of a flow with its optional occlusion map that the reductions share, in two parts (the entries have rules of
// their own between them): the format codes, then the batch and the plane.  The first rule broken, or nullptr.
inline const char* flow_occ_fmt_error(int flow_fmt, bool with_occ, int occ_fmt) {
  if (flow_fmt != OFDG_FMT_F32 && flow_fmt != OFDG_FMT_F16) return "flow_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if (with_occ && occ_fmt != OFDG_FMT_F32 && occ_fmt != OFDG_FMT_U8) return "occ_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  return nullptr;
}
inline const char* batch_plane_error(int n, int width, int height) {
  if (n < 1) return "n_samples must be at least 1";
  if (width < 1 || height < 1) return "width and height must be at least 1";
  return nullptr;
}

// One row of the flow statistics (ofdg_flow_stats_row of include/ofdg.h, field for field): the kernel adds to the counts and
// the Q8 sums with unsigned atomics (two's complement: the sums are int64 to the caller), so they are arrays here.
constexpr int kFlowHistBins = 64;  // OFDG_FLOW_HIST_BINS
struct DevFlowStatsRow {
  uint32_t hist[kFlowHistBins];
  uint32_t count[4];              // n_counted, n_bad, n_occluded, reserved
  unsigned long long sum_q8[3];   // sum_u_q8, sum_v_q8, sum_mag_q8
  unsigned long long max_key;
};
static_assert(sizeof(ofdg_flow_stats_row) == sizeof(DevFlowStatsRow) && sizeof(DevFlowStatsRow) == 304 && OFDG_FLOW_HIST_BINS == kFlowHistBins &&
              offsetof(ofdg_flow_stats_row, n_counted) == offsetof(DevFlowStatsRow, count) && offsetof(ofdg_flow_stats_row, sum_u_q8) == offsetof(DevFlowStatsRow, sum_q8) &&
              offsetof(ofdg_flow_stats_row, max_key) == offsetof(DevFlowStatsRow, max_key) && offsetof(DevFlowStatsRow, max_key) == 296,
              "ofdg_flow_stats_row: 304 bytes without padding, the layout the kernel adds to");
// The argument rules ofdg_flow_stats and ofdg_host_flow_stats share: the first rule broken, or nullptr.
inline const char* flow_stats_arg_error(const void* flow, int flow_fmt, const void* occ, int occ_fmt, int n, int width, int height,
                                        float bin_px, int flags, const void* rows) {
  if (!flow) return "d_flow is NULL";
  if (!rows) return "d_rows is NULL";
  if (const char* why = flow_occ_fmt_error(flow_fmt, occ != nullptr, occ_fmt)) return why;
  if (const char* why = batch_plane_error(n, width, height)) return why;
  if (!(bin_px >= 0.0009765625f && bin_px <= 16384.0f)) return "bin_px must lie in [2^-10, 2^14]";
  if (flags & ~(OFDG_STATS_ACCUMULATE | OFDG_STATS_VISIBLE_ONLY | OFDG_STATS_ONE_ROW)) return "flags holds unknown bits";
  if ((flags & OFDG_STATS_VISIBLE_ONLY) && !occ) return "flags: OFDG_STATS_VISIBLE_ONLY needs d_occ";
  if ((flags & OFDG_STATS_ONE_ROW) && (unsigned long long)n * (unsigned long long)width * (unsigned long long)height >= (1ull << 32))
    return "flags: OFDG_STATS_ONE_ROW needs n*H*W below 2^32";
  if ((uintptr_t)rows & 7) return "d_rows must be 8-byte aligned";
  return nullptr;
}

// Where the levels of a flow pyramid go (struct ofdg_flow_pyramid of include/ofdg.h, field for field): passed to the kernel
// by value.
constexpr int kPyrMaxLevels = 6;  // OFDG_PYR_MAX_LEVELS
struct DevFlowPyramid {
  void* flow[kPyrMaxLevels];
  void* weight[kPyrMaxLevels];
  int32_t levels, out_fmt;
};
static_assert(sizeof(struct ofdg_flow_pyramid) == sizeof(DevFlowPyramid) && sizeof(DevFlowPyramid) == 104 && OFDG_PYR_MAX_LEVELS == kPyrMaxLevels &&
              offsetof(struct ofdg_flow_pyramid, weight) == offsetof(DevFlowPyramid, weight) && offsetof(struct ofdg_flow_pyramid, levels) == offsetof(DevFlowPyramid, levels) &&
              offsetof(struct ofdg_flow_pyramid, out_fmt) == offsetof(DevFlowPyramid, out_fmt) && offsetof(DevFlowPyramid, out_fmt) == 100,
              "struct ofdg_flow_pyramid: 104 bytes, the layout the kernel takes");
// The argument rules ofdg_flow_pyramid and ofdg_host_flow_pyramid share: the first rule broken, or nullptr.  The planes of
// the input are aligned by the device entry only.
inline const char* flow_pyramid_arg_error(const void* flow, int flow_fmt, const void* occ, int occ_fmt, int n, int width, int height,
                                          int flags, const DevFlowPyramid* pyr) {
  if (!flow) return "d_flow is NULL";
  if (!pyr) return "pyr is NULL";
  if (const char* why = flow_occ_fmt_error(flow_fmt, occ != nullptr, occ_fmt)) return why;
  if (pyr->out_fmt != OFDG_FMT_F32 && pyr->out_fmt != OFDG_FMT_F16) return "pyr->out_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if (const char* why = batch_plane_error(n, width, height)) return why;
  if (flags & ~OFDG_PYR_SCALE) return "flags holds unknown bits";
  if (pyr->levels < 1 || pyr->levels > kPyrMaxLevels) return "pyr->levels must lie in 1..6";
  const int cell = 1 << pyr->levels;
  if (width % cell || height % cell) return "pyr->levels: width and height must be multiples of 2^levels";
  int with_weight = 0;
  for (int k = 0; k < pyr->levels; ++k) {
    if (!pyr->flow[k]) return "pyr->flow holds NULL for a level <= levels";
    with_weight += pyr->weight[k] ? 1 : 0;
  }
  if (with_weight != 0 && with_weight != pyr->levels) return "pyr->weight must be set for every level <= levels or for none";
  for (int k = 0; k < pyr->levels; ++k) {
    if ((uintptr_t)pyr->flow[k] & 15) return "pyr->flow: every level must be 16-byte aligned";
    if ((uintptr_t)pyr->weight[k] & 3) return "pyr->weight: every level must be 4-byte aligned";
  }
  return nullptr;
}

// The plane-size rule of the sized reductions (ofdg_flow_stats_sized, ofdg_flow_pyramid_sized): the context's own.
inline const char* plane_size_error(int width, int height) {
  if (width < 8 || height < 2 || (width % 8) != 0 || (height % 2) != 0) return "width must be a multiple of 8 and height even";
  return nullptr;
}

// ---- Argument rules every post-processing operation shares (host code only) ------------------------------------------------
// The plane size of a job: its own when set, else the one offered (the context's frame, the host twin's arguments).
constexpr const char* kPlanePairRule = "width and height must both be 0 or both be set";  // (host_api.cpp's host_open says it too)
template <typename Job>
inline const char* job_plane_size(const Job& j, int* width, int* height) {
  if ((j.width == 0) != (j.height == 0)) return kPlanePairRule;
  if (j.width != 0) { *width = j.width; *height = j.height; }
  return plane_size_error(*width, *height);
}
// The byte ranges a job names, at most N of them, and the rule on them: a written range may meet no other range of the job,
// except the one it is in place with (dst[f] == src[f] in one format).  Ranges that touch (hi == lo) do not meet.
struct Range { uintptr_t lo, hi; bool written; int in_place_with; };
template <int N>
struct RangeSet {
  Range r[N];
  int n = 0;
  // -> the range's index, for a partner's in_place_with.  N is an operation's own count of pointers: one add too many is a
  // mistake in that operation's rules, never a caller's input, and ends the process rather than write past r.
  int add(const void* p, unsigned long long bytes, bool written, int in_place_with = -1) {
    if (n >= N) abort();
    r[n] = Range{(uintptr_t)p, (uintptr_t)p + (uintptr_t)bytes, written, in_place_with};
    return n++;
  }
  void add_if(const void* p, unsigned long long bytes, bool written) {
    if (p) add(p, bytes, written);
  }
  // `why` when a written range meets another one, in the order the ranges were added; else nullptr
  const char* overlap(const char* why) const {
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b)
        if (a != b && r[a].written && r[a].in_place_with != b && r[a].lo < r[b].hi && r[b].lo < r[a].hi) return why;
    return nullptr;
  }
};
// The frame-pair jobs (photo, jitter, camera, jpeg; motion blur as far as frame_pair_fmt_error): src[2], dst[2], src_fmt,
// dst_fmt, recs, recs_out under the same names.  Three pieces, since each operation has rules of its own between them.
template <typename Job>
inline const char* frame_pair_fmt_error(const Job* j, int n, int width, int height) {
  if (!j) return "job is NULL";
  if (n < 1) return "n_samples must be at least 1";
  if (3ull * (unsigned long long)width * (unsigned long long)height >= (1ull << 32)) return "3 * width * height must be below 2^32";
  if (j->src_fmt != OFDG_FMT_F32 && j->src_fmt != OFDG_FMT_U8) return "src_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->dst_fmt != OFDG_FMT_F32 && j->dst_fmt != OFDG_FMT_U8) return "dst_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  return nullptr;
}
template <typename Job>
inline const char* frame_pair_frames_error(const Job* j) {
  int frames = 0;
  for (int f = 0; f < 2; ++f) {
    if (j->src[f] && !j->dst[f]) return "dst: a frame has a source and no destination";
    if (!j->src[f] && j->dst[f]) return "src: a frame has a destination and no source";
    frames += j->src[f] ? 1 : 0;
  }
  if (!frames) return "src: no frame is set";
  return nullptr;
}
// src and dst of each frame set, then recs and recs_out: six ranges at most.  in_place_form: does the operation take dst[f] == src[f]?
template <int N, typename Job>
inline void frame_pair_ranges(RangeSet<N>& set, const Job* j, int n, int width, int height, bool in_place_form) {
  const unsigned long long elems = 3ull * (unsigned long long)n * width * height;
  for (int f = 0; f < 2; ++f) {
    if (!j->src[f]) continue;
    const bool in_place = in_place_form && j->dst[f] == j->src[f] && j->src_fmt == j->dst_fmt;
    const int s = set.add(j->src[f], elems * fmt_elem_bytes(j->src_fmt), false);
    set.add(j->dst[f], elems * fmt_elem_bytes(j->dst_fmt), true, in_place ? s : -1);
  }
  set.add_if(j->recs, (unsigned long long)n * sizeof(*j->recs), false);
  set.add_if(j->recs_out, (unsigned long long)n * sizeof(*j->recs), true);
}

// ---- Training crop (ofdg_crop, include/ofdg.h) -----------------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job as the kernel takes it, the record's draw and its
// sanitising, the window test of the occlusion rule and the argument rules.
constexpr int kCropPlanes = 8;  // OFDG_CROP_PLANES: image0, image1, flow, flow1, occ0, occ1, label0, label1
struct DevCropRec {
  int32_t x0, y0, flags, reserved;
};
struct DevCropJob {  // struct ofdg_crop_job, field for field
  const void* src[kCropPlanes];
  void* dst[kCropPlanes];
  const DevCropRec* recs;
  DevCropRec* recs_out;
  long long first_index;
  uint32_t seed;
  int32_t crop_w, crop_h, flags, image_fmt, flow_fmt, occ_fmt, reserved;
};
static_assert(sizeof(ofdg_crop_rec) == sizeof(DevCropRec) && sizeof(DevCropRec) == 16 && sizeof(struct ofdg_crop_job) == sizeof(DevCropJob) &&
              sizeof(DevCropJob) == 184 && OFDG_CROP_PLANES == kCropPlanes && offsetof(struct ofdg_crop_job, dst) == offsetof(DevCropJob, dst) &&
              offsetof(struct ofdg_crop_job, recs) == offsetof(DevCropJob, recs) && offsetof(struct ofdg_crop_job, recs_out) == offsetof(DevCropJob, recs_out) &&
              offsetof(struct ofdg_crop_job, first_index) == offsetof(DevCropJob, first_index) && offsetof(struct ofdg_crop_job, seed) == offsetof(DevCropJob, seed) &&
              offsetof(struct ofdg_crop_job, crop_w) == offsetof(DevCropJob, crop_w) && offsetof(struct ofdg_crop_job, occ_fmt) == offsetof(DevCropJob, occ_fmt) &&
              offsetof(struct ofdg_crop_job, reserved) == offsetof(DevCropJob, reserved) && offsetof(DevCropJob, reserved) == 180,
              "ofdg_crop_rec: 16 bytes; struct ofdg_crop_job: 184 bytes, the layout the kernel takes");
static_assert(OFDG_CROP_HFLIP == 1 && OFDG_CROP_VFLIP == 2 && OFDG_CROP_RANDOM_HFLIP == 4 && OFDG_CROP_RANDOM_VFLIP == 8 && OFDG_CROP_FLOW == 2 &&
              OFDG_CROP_OCC0 == 4 && OFDG_CROP_LABEL0 == 6, "crop_draw_rec, crop_sanitise, crop_channels and crop_kernel spell these codes out");
OFDG_HD_FN int crop_channels(int plane) { return plane < 2 ? 3 : plane < 4 ? 2 : 1; }
// the element type of plane k (the labels are uint8) and its bytes
OFDG_HD_FN int crop_plane_fmt(const DevCropJob& j, int plane) { return plane < 2 ? j.image_fmt : plane < 4 ? j.flow_fmt : plane < 6 ? j.occ_fmt : OFDG_FMT_U8; }
OFDG_HD_FN int crop_elem_bytes(const DevCropJob& j, int plane) { return fmt_elem_bytes(crop_plane_fmt(j, plane)); }

// Philox4x32-10 (Salmon et al., SC'11), the function of csrc/sampler_counter.hip restated for host and device.  The sampler's
// own device copy stays as it is; this one is held to the three published known answers through ofdg_crop_philox
// (tests/test_crop.py), and host and kernel to each other through the drawn records (tests/test_gpu_crop.py).
struct CropWords {
  uint32_t x, y, z, w;
};
OFDG_HD_FN CropWords crop_philox(CropWords ctr, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * ctr.x, p1 = 0xCD9E8D57ull * ctr.z;
    ctr = CropWords{(uint32_t)(p1 >> 32) ^ ctr.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ ctr.w ^ k1, (uint32_t)p0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return ctr;
}
// The record of global sample g: one Philox block under the sampler's key of g (cs_key) and the counter {0, 0, 0x0c70, 0} -
// the sampler's third counter word is always 0x0fd9, so no stream of the sampler is touched.  x0 = floor(w.x * range / 2^32):
// no rejection loop, so a value's probability is off by at most range / 2^32 (below 2^-16 for any frame).  Needs
// crop_w <= width and crop_h <= height.  flags: the job's (RANDOM_HFLIP 4, RANDOM_VFLIP 8).
OFDG_HD_FN DevCropRec crop_draw_rec(uint32_t seed, unsigned long long g, int width, int height, int crop_w, int crop_h, int flags) {
  const CropWords w = crop_philox(CropWords{0u, 0u, 0x0c70u, 0u}, seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, (uint32_t)g);
  DevCropRec r;
  r.x0 = (int32_t)(uint32_t)(((unsigned long long)w.x * (uint32_t)(width - crop_w + 1)) >> 32);
  r.y0 = (int32_t)(uint32_t)(((unsigned long long)w.y * (uint32_t)(height - crop_h + 1)) >> 32);
  r.flags = ((flags & 4) ? (int32_t)(w.z & 1u) : 0) | ((flags & 8) ? (int32_t)((w.z >> 1) & 1u) << 1 : 0);
  r.reserved = 0;
  return r;
}
// What is used of a record, given or drawn: the window inside the frame, the two flip bits, nothing else.
OFDG_HD_FN DevCropRec crop_sanitise(DevCropRec r, int width, int height, int crop_w, int crop_h) {
  r.x0 = r.x0 < 0 ? 0 : r.x0 > width - crop_w ? width - crop_w : r.x0;
  r.y0 = r.y0 < 0 ? 0 : r.y0 > height - crop_h ? height - crop_h : r.y0;
  r.flags &= 3;
  r.reserved = 0;
  return r;
}
// OFDG_CROP_OCC_WINDOW, one axis: does the flow target of source coordinate `at` (displacement d) lie in [lo, lo + len - 1]?
// Three float32 roundings, no contraction; a NaN fails both comparisons.
OFDG_HD_FN bool crop_target_inside(int at, float d, int lo, int len) {
  const float s = (float)at + d;
  const float h = s + 0.5f;
  const float t = floorf(h);
  return t >= (float)lo && t <= (float)(lo + len - 1);
}
// The argument rules ofdg_crop and ofdg_host_crop share: the first rule broken, or nullptr.  Alignment is asked by the device
// entry only.
inline const char* crop_arg_error(const DevCropJob* j, int n, int width, int height) {
  if (!j) return "job is NULL";
  if (n < 1) return "n_samples must be at least 1";
  if (j->crop_w < 8 || j->crop_w > width || (j->crop_w % 8) != 0) return "crop_w must be a multiple of 8 in [8, width]";
  if (j->crop_h < 2 || j->crop_h > height || (j->crop_h % 2) != 0) return "crop_h must be even and in [2, height]";
  if ((unsigned long long)width * (unsigned long long)height >= (1ull << 31)) return "width * height must be below 2^31";
  if (j->flags & ~(OFDG_CROP_RANDOM_HFLIP | OFDG_CROP_RANDOM_VFLIP | OFDG_CROP_OCC_WINDOW)) return "flags holds unknown bits";
  if (j->reserved != 0) return "reserved must be 0";
  if (j->image_fmt != OFDG_FMT_F32 && j->image_fmt != OFDG_FMT_U8) return "image_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (const char* why = flow_occ_fmt_error(j->flow_fmt, true, j->occ_fmt)) return why;  // (the job's occ_fmt is checked with or without a map)
  int planes = 0;
  for (int k = 0; k < kCropPlanes; ++k) {
    if (j->src[k] && !j->dst[k]) return "dst: a plane has a source and no destination";
    if (!j->src[k] && j->dst[k]) return "src: a plane has a destination and no source";
    planes += j->src[k] ? 1 : 0;
  }
  if (!planes) return "src: no plane is set";
  if ((j->flags & OFDG_CROP_OCC_WINDOW) && j->src[OFDG_CROP_OCC0] && !j->src[OFDG_CROP_FLOW]) return "flags: OFDG_CROP_OCC_WINDOW with occ0 needs flow";
  if ((j->flags & OFDG_CROP_OCC_WINDOW) && j->src[OFDG_CROP_OCC1] && !j->src[OFDG_CROP_FLOW1]) return "flags: OFDG_CROP_OCC_WINDOW with occ1 needs flow1";
  // no in-place form: a destination range may meet no other range of the job
  RangeSet<2 * kCropPlanes + 2> r;
  for (int k = 0; k < kCropPlanes; ++k) {
    if (!j->src[k]) continue;
    const unsigned long long per = (unsigned long long)n * crop_channels(k) * crop_elem_bytes(*j, k);
    r.add(j->src[k], per * width * height, false);
    r.add(j->dst[k], per * j->crop_w * j->crop_h, true);
  }
  r.add_if(j->recs, (unsigned long long)n * 16, false);
  r.add_if(j->recs_out, (unsigned long long)n * 16, true);
  return r.overlap("dst: a destination range overlaps another range of the job");
}

// ---- Photometric augmentation (ofdg_photo, include/ofdg.h) -----------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job as the kernel takes it, the record's draw and its
// sanitising, one table entry, the element's index, the noise and the argument rules.  Everything here is compiled without
// contraction, so every operation below is its own rounding.
struct DevPhotoRec {  // ofdg_photo_rec, field for field
  float gamma[2], contrast[2], brightness[2], gain[2][3], sigma[2];
  int32_t reserved[2];
};
struct DevPhotoJob {  // struct ofdg_photo_job, field for field
  const void* src[2];
  void* dst[2];
  const DevPhotoRec* recs;
  DevPhotoRec* recs_out;
  long long first_index;
  uint32_t seed;
  int32_t width, height, src_fmt, dst_fmt, flags, reserved;
  float gamma_log, contrast_log, brightness, colour_log, sigma_max;
  float pair_gamma_log, pair_contrast_log, pair_brightness, pair_colour_log;
};
static_assert(sizeof(ofdg_photo_rec) == sizeof(DevPhotoRec) && sizeof(DevPhotoRec) == 64 && offsetof(ofdg_photo_rec, gain) == offsetof(DevPhotoRec, gain) &&
              offsetof(DevPhotoRec, gain) == 24 && offsetof(ofdg_photo_rec, sigma) == offsetof(DevPhotoRec, sigma) && offsetof(DevPhotoRec, sigma) == 48 &&
              offsetof(ofdg_photo_rec, reserved) == offsetof(DevPhotoRec, reserved), "ofdg_photo_rec: 64 bytes without padding, the layout the kernel reads and writes");
static_assert(sizeof(struct ofdg_photo_job) == sizeof(DevPhotoJob) && sizeof(DevPhotoJob) == 120 && offsetof(struct ofdg_photo_job, dst) == offsetof(DevPhotoJob, dst) &&
              offsetof(struct ofdg_photo_job, recs) == offsetof(DevPhotoJob, recs) && offsetof(struct ofdg_photo_job, recs_out) == offsetof(DevPhotoJob, recs_out) &&
              offsetof(struct ofdg_photo_job, first_index) == offsetof(DevPhotoJob, first_index) && offsetof(struct ofdg_photo_job, seed) == offsetof(DevPhotoJob, seed) &&
              offsetof(struct ofdg_photo_job, width) == offsetof(DevPhotoJob, width) && offsetof(struct ofdg_photo_job, src_fmt) == offsetof(DevPhotoJob, src_fmt) &&
              offsetof(struct ofdg_photo_job, reserved) == offsetof(DevPhotoJob, reserved) && offsetof(struct ofdg_photo_job, gamma_log) == offsetof(DevPhotoJob, gamma_log) &&
              offsetof(DevPhotoJob, gamma_log) == 84 && offsetof(struct ofdg_photo_job, pair_colour_log) == offsetof(DevPhotoJob, pair_colour_log) &&
              offsetof(DevPhotoJob, pair_colour_log) == 116, "struct ofdg_photo_job: 120 bytes, the layout the kernel takes");
// u(w) = (w >> 8) * 2^-24 in [0, 1), exact; sym(w, a) = a * (2 u - 1) in [-a, a), one rounding (2 u and 2 u - 1 are exact); a
// zero of either sign is +0, so the ranges 0 give the identity record bit for bit.
OFDG_HD_FN float photo_unit(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }
OFDG_HD_FN float photo_sym(uint32_t w, float a) {
  const float t = 2.0f * photo_unit(w) - 1.0f;
  const float r = a * t;
  return r == 0.0f ? 0.0f : r;
}
OFDG_HD_FN float photo_exp(float l) { return (float)ofdg_det_exp((double)l); }
// The record of global sample g: Philox blocks 0, 1, 2 under the sampler's key of g and the counters {j, 0, 0x0c71, 0} (the
// sampler's third counter word is 0x0fd9, the crop's 0x0c70).  `j` supplies the nine ranges.
OFDG_HD_FN DevPhotoRec photo_draw_rec(uint32_t seed, unsigned long long g, const DevPhotoJob& j) {
  const uint32_t k0 = seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
  const CropWords a = crop_philox(CropWords{0u, 0u, 0x0c71u, 0u}, k0, k1);
  const CropWords b = crop_philox(CropWords{1u, 0u, 0x0c71u, 0u}, k0, k1);
  const CropWords d = crop_philox(CropWords{2u, 0u, 0x0c71u, 0u}, k0, k1);
  const float lg0 = photo_sym(a.x, j.gamma_log), lc0 = photo_sym(a.y, j.contrast_log), b0 = photo_sym(a.z, j.brightness);
  const float sigma = j.sigma_max * photo_unit(a.w);
  const float col0 = photo_sym(b.x, j.colour_log), col1 = photo_sym(b.y, j.colour_log), col2 = photo_sym(b.z, j.colour_log);
  const float dg = photo_sym(d.x, j.pair_gamma_log), dc = photo_sym(d.y, j.pair_contrast_log), db = photo_sym(d.z, j.pair_brightness);
  const float dcol = photo_sym(d.w, j.pair_colour_log);
  const float lg1 = lg0 + dg, lc1 = lc0 + dc, b1 = b0 + db, col0b = col0 + dcol, col1b = col1 + dcol, col2b = col2 + dcol;
  DevPhotoRec r;
  r.gamma[0] = photo_exp(lg0); r.gamma[1] = photo_exp(lg1);
  r.contrast[0] = photo_exp(lc0); r.contrast[1] = photo_exp(lc1);
  r.brightness[0] = b0; r.brightness[1] = b1;
  r.gain[0][0] = photo_exp(col0); r.gain[0][1] = photo_exp(col1); r.gain[0][2] = photo_exp(col2);
  r.gain[1][0] = photo_exp(col0b); r.gain[1][1] = photo_exp(col1b); r.gain[1][2] = photo_exp(col2b);
  r.sigma[0] = sigma; r.sigma[1] = sigma;
  r.reserved[0] = 0; r.reserved[1] = 0;
  return r;
}
// What is used of a record, given or drawn: a NaN becomes the identity value, then the lower bound, then the upper one (an
// infinity lands on a bound; -0.0 passes as it is).
OFDG_HD_FN float photo_clamp(float x, float lo, float hi, float identity) { return x != x ? identity : x < lo ? lo : x > hi ? hi : x; }
OFDG_HD_FN DevPhotoRec photo_sanitise(DevPhotoRec r) {
  for (int f = 0; f < 2; ++f) {
    r.gamma[f] = photo_clamp(r.gamma[f], 0.125f, 8.0f, 1.0f);
    r.contrast[f] = photo_clamp(r.contrast[f], 0.0f, 4.0f, 1.0f);
    r.brightness[f] = photo_clamp(r.brightness[f], -1.0f, 1.0f, 0.0f);
    for (int c = 0; c < 3; ++c) r.gain[f][c] = photo_clamp(r.gain[f][c], 0.0f, 8.0f, 1.0f);
    r.sigma[f] = photo_clamp(r.sigma[f], 0.0f, 64.0f, 0.0f);
    r.reserved[f] = 0;
  }
  return r;
}
// Entry k of the table of one (frame, channel) of a sanitised record: fp64, every operation rounded on its own, the sums
// from left to right; below 0 (or NaN, which a sanitised record cannot give) becomes 0, then above 255 becomes 255.
OFDG_HD_FN float photo_table_entry(float gamma, float gain, float contrast, float brightness, int k) {
  const double x = (double)k / 255.0;
  double p = x;
  if (k == 0) p = 0.0;
  else if (gamma != 1.0f) p = ofdg_det_exp((double)gamma * ofdg_det_log(x));
  const double a = p * (double)gain;
  const double b = a - 0.5;
  const double c = b * (double)contrast;
  const double d = c + 0.5;
  const double e = d + (double)brightness;
  double t = 255.0 * e;
  t = t > 0.0 ? t : 0.0;
  t = t < 255.0 ? t : 255.0;
  return (float)t;
}
// The table index of a float32 element: clamped to [0, 255] (a NaN becomes 0), then rounded to nearest even.
OFDG_HD_FN int photo_index(float x) {
  x = x > 0.0f ? x : 0.0f;
  x = x < 255.0f ? x : 255.0f;
  return (int)rintf(x);
}
// sigma / sqrt(4 * (256^2 - 1) / 12): what one unit of the centred byte sum is worth
OFDG_HD_FN float photo_noise_scale(float sigma) { return sigma / 147.80054f; }
// v with the noise of one Philox word: the word's four bytes summed (0..1020, mean 510), two float32 products / sums, clamped.
OFDG_HD_FN float photo_add_noise(float v, float scale, uint32_t word) {
  const int s = (int)((word & 255u) + ((word >> 8) & 255u) + ((word >> 16) & 255u) + (word >> 24));
  const float d = scale * (float)(s - 510);
  float o = v + d;
  o = o > 0.0f ? o : 0.0f;
  o = o < 255.0f ? o : 255.0f;
  return o;
}
// The nine ranges of the draw: the first that is negative, NaN or infinite, or nullptr.
inline const char* photo_ranges_error(const DevPhotoJob& job) {
  const DevPhotoJob* const j = &job;
  const struct { float v; const char* why; } ranges[9] = {
      {j->gamma_log, "gamma_log must be finite and not negative"}, {j->contrast_log, "contrast_log must be finite and not negative"},
      {j->brightness, "brightness must be finite and not negative"}, {j->colour_log, "colour_log must be finite and not negative"},
      {j->sigma_max, "sigma_max must be finite and not negative"}, {j->pair_gamma_log, "pair_gamma_log must be finite and not negative"},
      {j->pair_contrast_log, "pair_contrast_log must be finite and not negative"}, {j->pair_brightness, "pair_brightness must be finite and not negative"},
      {j->pair_colour_log, "pair_colour_log must be finite and not negative"}};
  for (int k = 0; k < 9; ++k)
    if (!(ranges[k].v >= 0.0f && ranges[k].v <= 3.4028234663852886e38f)) return ranges[k].why;
  return nullptr;
}
// The argument rules ofdg_photo and ofdg_host_photo share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment is asked by the device entry only.
inline const char* photo_arg_error(const DevPhotoJob* j, int n, int width, int height) {
  if (const char* why = frame_pair_fmt_error(j, n, width, height)) return why;
  if (j->flags != 0) return "flags must be 0";
  if (j->reserved != 0) return "reserved must be 0";
  if (const char* why = photo_ranges_error(*j)) return why;
  if (const char* why = frame_pair_frames_error(j)) return why;
  RangeSet<6> r;
  frame_pair_ranges(r, j, n, width, height, true);
  return r.overlap("dst: a destination range overlaps another range of the job");
}

// ---- Spatial augmentation (ofdg_spatial, include/ofdg.h) -------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job as the kernel takes it, the record's draw and its
// sanitising, the inverse, the tap, the blend, the flow's transform, the occlusion rule and the argument rules.  Compiled
// without contraction, so every operation below is its own rounding.
struct DevSpatialRec {  // ofdg_spatial_rec, field for field
  double m[2][6];       // [frame]{a, b, c, d, e, g}
  int32_t reserved[4];
};
struct DevSpatialJob {  // struct ofdg_spatial_job, field for field
  const void* src[kCropPlanes];
  void* dst[kCropPlanes];
  const DevSpatialRec* recs;
  DevSpatialRec* recs_out;
  long long first_index;
  uint32_t seed;
  int32_t width, height, out_w, out_h, flags, image_fmt, flow_fmt, occ_fmt;
  int32_t reserved[2];
  float zoom_log, rot, squeeze_log, translate, pair_zoom_log, pair_rot, pair_translate;
};
static_assert(sizeof(ofdg_spatial_rec) == sizeof(DevSpatialRec) && sizeof(DevSpatialRec) == 112 && offsetof(ofdg_spatial_rec, reserved) == offsetof(DevSpatialRec, reserved) &&
              offsetof(DevSpatialRec, reserved) == 96, "ofdg_spatial_rec: 112 bytes without padding, the layout the kernel reads and writes");
static_assert(sizeof(struct ofdg_spatial_job) == sizeof(DevSpatialJob) && sizeof(DevSpatialJob) == 224 && offsetof(struct ofdg_spatial_job, dst) == offsetof(DevSpatialJob, dst) &&
              offsetof(struct ofdg_spatial_job, recs) == offsetof(DevSpatialJob, recs) && offsetof(struct ofdg_spatial_job, recs_out) == offsetof(DevSpatialJob, recs_out) &&
              offsetof(struct ofdg_spatial_job, first_index) == offsetof(DevSpatialJob, first_index) && offsetof(struct ofdg_spatial_job, seed) == offsetof(DevSpatialJob, seed) &&
              offsetof(struct ofdg_spatial_job, width) == offsetof(DevSpatialJob, width) && offsetof(struct ofdg_spatial_job, out_w) == offsetof(DevSpatialJob, out_w) &&
              offsetof(struct ofdg_spatial_job, occ_fmt) == offsetof(DevSpatialJob, occ_fmt) && offsetof(struct ofdg_spatial_job, reserved) == offsetof(DevSpatialJob, reserved) &&
              offsetof(DevSpatialJob, reserved) == 188 && offsetof(struct ofdg_spatial_job, zoom_log) == offsetof(DevSpatialJob, zoom_log) &&
              offsetof(struct ofdg_spatial_job, pair_translate) == offsetof(DevSpatialJob, pair_translate) && offsetof(DevSpatialJob, pair_translate) == 220,
              "struct ofdg_spatial_job: 224 bytes, the layout the kernel takes");
static_assert(OFDG_SPATIAL_RANDOM_HFLIP == 4 && OFDG_SPATIAL_RANDOM_VFLIP == 8 && OFDG_SPATIAL_OCC_WINDOW == 16, "spatial_draw_rec and spatial_kernel spell these codes out");
constexpr int kSpatialMaxSide = 1 << 20;  // of a source or output plane: (side - 1) * 256 stays far inside an int
OFDG_HD_FN double spatial_abs(double x) { return x < 0.0 ? -x : x; }
OFDG_HD_FN double spatial_plus_zero(double x) { return x == 0.0 ? 0.0 : x; }
// a, b, d, e of one frame into m[0], m[1], m[3], m[4]: zoom exp(lz), squeeze exp(lq), rotation th, flips h, v = +-1
OFDG_HD_FN void spatial_linear(float lz, float th, float lq, double h, double v, double* m) {
  const float lx = lz + lq, ly = lz - lq;
  const double gx = ofdg_det_exp(-(double)lx), gy = ofdg_det_exp(-(double)ly);
  double s, c;
  ofdg_det_sincos((double)th, &s, &c);
  m[0] = spatial_plus_zero(c * gx * h);
  m[1] = spatial_plus_zero(-(s * gy) * v);
  m[3] = spatial_plus_zero(s * gx * h);
  m[4] = spatial_plus_zero(c * gy * v);
}
// c (or g) of a frame: the centre `at` of the window minus where the linear part puts the window's centre
OFDG_HD_FN double spatial_offset(double at, double p, double q, double hw, double hh) {
  const double t0 = p * hw, t1 = q * hh;
  return at - (t0 + t1);
}
// the centre of frame 0 on one axis of a source of `side` pixels: (side - 1) / 2 + (tf * translate) * slack
OFDG_HD_FN double spatial_centre(int side, double p, double q, double hw, double hh, float tf, float translate) {
  const double mid = (double)(side - 1) / 2.0;
  const double t0 = spatial_abs(p) * hw, t1 = spatial_abs(q) * hh;
  const double ex = t0 + t1;
  double slack = mid - ex;
  slack = slack > 0.0 ? slack : 0.0;
  const double f = (double)tf * (double)translate;
  return mid + f * slack;
}
// The record of global sample g for a W x H source: Philox blocks 0, 1, 2 under the sampler's key of g at the counters {j, 0,
// 0x0c73, 0}.  `j` supplies the seven ranges, the flags and the output size.
OFDG_HD_FN DevSpatialRec spatial_draw_rec(uint32_t seed, unsigned long long g, const DevSpatialJob& j, int W, int H) {
  const uint32_t k0 = seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
  const CropWords w0 = crop_philox(CropWords{0u, 0u, 0x0c73u, 0u}, k0, k1);
  const CropWords w1 = crop_philox(CropWords{1u, 0u, 0x0c73u, 0u}, k0, k1);
  const CropWords w2 = crop_philox(CropWords{2u, 0u, 0x0c73u, 0u}, k0, k1);
  const float lz = photo_sym(w0.x, j.zoom_log), th = photo_sym(w0.y, j.rot), lq = photo_sym(w0.z, j.squeeze_log);
  const double h = ((j.flags & 4) && (w0.w & 1u)) ? -1.0 : 1.0, v = ((j.flags & 8) && ((w0.w >> 1) & 1u)) ? -1.0 : 1.0;
  const float tfx = 2.0f * photo_unit(w1.x) - 1.0f, tfy = 2.0f * photo_unit(w1.y) - 1.0f;
  const float dlz = photo_sym(w2.x, j.pair_zoom_log), dth = photo_sym(w2.y, j.pair_rot);
  const float dtx = photo_sym(w2.z, j.pair_translate), dty = photo_sym(w2.w, j.pair_translate);
  const double hw = (double)(j.out_w - 1) / 2.0, hh = (double)(j.out_h - 1) / 2.0;
  DevSpatialRec r;
  spatial_linear(lz, th, lq, h, v, r.m[0]);
  const double cx = spatial_centre(W, r.m[0][0], r.m[0][1], hw, hh, tfx, j.translate);
  const double cy = spatial_centre(H, r.m[0][3], r.m[0][4], hw, hh, tfy, j.translate);
  r.m[0][2] = spatial_offset(cx, r.m[0][0], r.m[0][1], hw, hh);
  r.m[0][5] = spatial_offset(cy, r.m[0][3], r.m[0][4], hw, hh);
  const float lz1 = lz + dlz, th1 = th + dth;
  spatial_linear(lz1, th1, lq, h, v, r.m[1]);
  r.m[1][2] = spatial_offset(cx + (double)dtx, r.m[1][0], r.m[1][1], hw, hh);
  r.m[1][5] = spatial_offset(cy + (double)dty, r.m[1][3], r.m[1][4], hw, hh);
  for (int k = 0; k < 4; ++k) r.reserved[k] = 0;
  return r;
}
OFDG_HD_FN double spatial_det(const double* m) {
  const double p = m[0] * m[4], q = m[1] * m[3];
  return p - q;
}
// What is used of a record, given or drawn: a frame whose map is not finite, out of bounds or (nearly) singular becomes the
// centred integer window.  (A comparison with a NaN fails, so a NaN fails its bound.)
OFDG_HD_FN DevSpatialRec spatial_sanitise(DevSpatialRec r, int W, int H, int out_w, int out_h) {
  for (int f = 0; f < 2; ++f) {
    double* const m = r.m[f];
    bool ok = spatial_abs(m[0]) <= 64.0 && spatial_abs(m[1]) <= 64.0 && spatial_abs(m[3]) <= 64.0 && spatial_abs(m[4]) <= 64.0;
    ok = ok && spatial_abs(m[2]) <= 1048576.0 && spatial_abs(m[5]) <= 1048576.0;
    const double det = spatial_abs(spatial_det(m));
    ok = ok && det >= 0.000244140625 && det <= 4096.0;
    if (!ok) {
      m[0] = 1.0; m[1] = 0.0; m[2] = (double)((W - out_w) >> 1);
      m[3] = 0.0; m[4] = 1.0; m[5] = (double)((H - out_h) >> 1);
    }
  }
  for (int k = 0; k < 4; ++k) r.reserved[k] = 0;
  return r;
}
// The inverse of a sanitised frame's map (its linear part, and the offsets the target is taken against), made once per sample.
struct SpatialInv {
  double ia, ib, id, ie, c, g;
};
OFDG_HD_FN SpatialInv spatial_inverse(const double* m) {
  const double det = spatial_det(m);
  SpatialInv v;
  v.ia = m[4] / det; v.ib = -m[1] / det; v.id = -m[3] / det; v.ie = m[0] / det;
  v.c = m[2]; v.g = m[5];
  return v;
}
// One coordinate of a destination pixel: q = (p * X + r * Y) + o, three roundings.  `row` = fl64(r * Y) is the same for a row.
OFDG_HD_FN double spatial_row_term(double r, int Y) { return r * (double)Y; }
OFDG_HD_FN double spatial_coord(double p, int X, double row, double o) {
  const double t = p * (double)X;
  const double s = t + row;
  return s + o;
}
// 24.8 fixed point of a coordinate, saturating at +-2^30
OFDG_HD_FN int spatial_fixed(double q) {
  const double s = q * 256.0;
  double t = floor(s + 0.5);
  t = t < -1073741824.0 ? -1073741824.0 : t;
  t = t > 1073741824.0 ? 1073741824.0 : t;
  return (int)t;
}
OFDG_HD_FN int spatial_clamp(int i, int side) { return i < 0 ? 0 : i > side - 1 ? side - 1 : i; }
OFDG_HD_FN bool spatial_inside(int Qx, int Qy, int W, int H) { return Qx >= 0 && Qx <= (W - 1) * 256 && Qy >= 0 && Qy <= (H - 1) * 256; }
OFDG_HD_FN float spatial_quiet(float v) {  // a NaN as 0x7FC00000
  const uint32_t bits = 0x7FC00000u;
  float nan;
  memcpy(&nan, &bits, 4);
  return v != v ? nan : v;
}
// The bilinear blend of four elements widened to float32, with the fractions fx, fy in 0..255
OFDG_HD_FN float spatial_blend(float e00, float e10, float e01, float e11, int fx, int fy) {
  const float w00 = (float)((256 - fx) * (256 - fy)), w10 = (float)(fx * (256 - fy)), w01 = (float)((256 - fx) * fy), w11 = (float)(fx * fy);
  const float p00 = w00 * e00, p10 = w10 * e10, p01 = w01 * e01, p11 = w11 * e11;
  const float top = p00 + p10, bottom = p01 + p11;
  const float sum = top + bottom;
  return spatial_quiet(sum * 1.52587890625e-05f);
}
OFDG_HD_FN uint32_t spatial_to_byte(float v) { return (uint32_t)photo_index(v); }  // clamped to [0, 255] (a NaN becomes 0), then to nearest even
// Where the pixel at (qx, qy) of its own frame's source, moving by (u, v), lands in the OTHER frame's destination
OFDG_HD_FN void spatial_partner(double qx, double qy, float u, float v, const SpatialInv& o, double* px, double* py) {
  const double tx = qx + (double)u, ty = qy + (double)v;
  const double dx = tx - o.c, dy = ty - o.g;
  const double xa = o.ia * dx, xb = o.ib * dy, ya = o.id * dx, yb = o.ie * dy;
  *px = xa + xb;
  *py = ya + yb;
}
OFDG_HD_FN float spatial_flow_of(double p, int at) { return spatial_quiet((float)(p - (double)at)); }
// OFDG_SPATIAL_OCC_WINDOW, one axis: floor(p + 0.5) in [0, len - 1]; a NaN fails both comparisons
OFDG_HD_FN bool spatial_partner_inside(double p, int len) {
  const double t = floor(p + 0.5);
  return t >= 0.0 && t <= (double)(len - 1);
}
// float32 -> binary16 to nearest even; an overflow becomes +-inf, a NaN 0x7E00
OFDG_HD_FN uint32_t spatial_half_bits(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7FFFFFFFu;
  if (x > 0x7F800000u) return 0x7E00u;
  if (x >= 0x477FF000u) return sign | 0x7C00u;
  if (x >= 0x38800000u) {
    x -= 0x38000000u;
    x += 0xFFFu + ((x >> 13) & 1u);
    return sign | (x >> 13);
  }
  const int shift = 126 - (int)(x >> 23);
  if (shift > 24) return sign;
  const uint32_t m = (x & 0x7FFFFFu) | 0x800000u, h = m >> shift, rem = m & ((1u << shift) - 1u), mid = 1u << (shift - 1);
  return sign | (h + ((rem > mid || (rem == mid && (h & 1u))) ? 1u : 0u));
}
// The source size of a job: its own when set, else the one offered (the context's frame, the host twin's arguments).
inline const char* spatial_plane_size(const DevSpatialJob& j, int* width, int* height) {
  if (const char* why = job_plane_size(j, width, height)) return why;
  if (*width > kSpatialMaxSide || *height > kSpatialMaxSide) return "width and height must not exceed 2^20";
  return nullptr;
}
// What the draw reads of a job besides the source size: the output size, the flags and the seven ranges.
inline const char* spatial_draw_error(const DevSpatialJob& job) {
  const DevSpatialJob* const j = &job;
  if (j->out_w < 8 || (j->out_w % 8) != 0 || j->out_w > kSpatialMaxSide) return "out_w must be a multiple of 8 in [8, 2^20]";
  if (j->out_h < 2 || (j->out_h % 2) != 0 || j->out_h > kSpatialMaxSide) return "out_h must be even and in [2, 2^20]";
  if (j->flags & ~(OFDG_SPATIAL_RANDOM_HFLIP | OFDG_SPATIAL_RANDOM_VFLIP | OFDG_SPATIAL_OCC_WINDOW)) return "flags holds unknown bits";
  const struct { float v; const char* why; } ranges[7] = {
      {j->zoom_log, "zoom_log must be finite and not negative"}, {j->rot, "rot must be finite and not negative"},
      {j->squeeze_log, "squeeze_log must be finite and not negative"}, {j->translate, "translate must lie in [0, 1]"},
      {j->pair_zoom_log, "pair_zoom_log must be finite and not negative"}, {j->pair_rot, "pair_rot must be finite and not negative"},
      {j->pair_translate, "pair_translate must be finite and not negative"}};
  for (int k = 0; k < 7; ++k)
    if (!(ranges[k].v >= 0.0f && ranges[k].v <= 3.4028234663852886e38f)) return ranges[k].why;
  if (j->translate > 1.0f) return "translate must lie in [0, 1]";
  return nullptr;
}
// The argument rules ofdg_spatial and ofdg_host_spatial share: the first rule broken, or nullptr.  width, height: what
// spatial_plane_size gave.  Alignment is asked by the device entry only.
inline const char* spatial_arg_error(const DevSpatialJob* j, int n, int width, int height) {
  if (!j) return "job is NULL";
  if (n < 1) return "n_samples must be at least 1";
  if (const char* why = spatial_draw_error(*j)) return why;
  if ((unsigned long long)width * (unsigned long long)height >= (1ull << 31)) return "width * height must be below 2^31";
  if ((unsigned long long)j->out_w * (unsigned long long)j->out_h >= (1ull << 31)) return "out_w * out_h must be below 2^31";
  if (j->reserved[0] != 0 || j->reserved[1] != 0) return "reserved must be 0";
  if (j->image_fmt != OFDG_FMT_F32 && j->image_fmt != OFDG_FMT_U8) return "image_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (const char* why = flow_occ_fmt_error(j->flow_fmt, true, j->occ_fmt)) return why;
  int planes = 0;
  for (int k = 0; k < kCropPlanes; ++k) {
    if (j->src[k] && !j->dst[k]) return "dst: a plane has a source and no destination";
    if (!j->src[k] && j->dst[k]) return "src: a plane has a destination and no source";
    planes += j->src[k] ? 1 : 0;
  }
  if (!planes) return "src: no plane is set";
  if ((j->flags & OFDG_SPATIAL_OCC_WINDOW) && j->src[OFDG_CROP_OCC0] && !j->src[OFDG_CROP_FLOW]) return "flags: OFDG_SPATIAL_OCC_WINDOW with occ0 needs flow";
  if ((j->flags & OFDG_SPATIAL_OCC_WINDOW) && j->src[OFDG_CROP_OCC1] && !j->src[OFDG_CROP_FLOW1]) return "flags: OFDG_SPATIAL_OCC_WINDOW with occ1 needs flow1";
  // no in-place form: a destination range may meet no other range of the job
  RangeSet<2 * kCropPlanes + 2> r;
  for (int k = 0; k < kCropPlanes; ++k) {
    if (!j->src[k]) continue;
    const int es = fmt_elem_bytes(k < 2 ? j->image_fmt : k < 4 ? j->flow_fmt : k < 6 ? j->occ_fmt : OFDG_FMT_U8);
    const unsigned long long per = (unsigned long long)n * crop_channels(k) * es;
    r.add(j->src[k], per * width * height, false);
    r.add(j->dst[k], per * j->out_w * j->out_h, true);
  }
  r.add_if(j->recs, (unsigned long long)n * sizeof(DevSpatialRec), false);
  r.add_if(j->recs_out, (unsigned long long)n * sizeof(DevSpatialRec), true);
  return r.overlap("dst: a destination range overlaps another range of the job");
}

// ---- Network-ready packing (ofdg_pack, include/ofdg.h) ---------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job as the kernel takes it, the value, the bfloat16
// rounding, the placement and the argument rules.  Compiled without contraction, so a product and a sum are two roundings.
constexpr int kPackPlanes = 3;  // OFDG_PACK_PLANES: image0, image1, flow
struct DevPackJob {             // struct ofdg_pack_job, field for field
  const void* src[kPackPlanes];
  void* dst[kPackPlanes];
  int32_t width, height, image_src_fmt, flow_src_fmt, image_dst_fmt, flow_dst_fmt, layout, flags;
  float scale[3], bias[3];
  float flow_scale;
  int32_t reserved;
};
static_assert(sizeof(struct ofdg_pack_job) == sizeof(DevPackJob) && sizeof(DevPackJob) == 112 && OFDG_PACK_PLANES == kPackPlanes &&
              offsetof(struct ofdg_pack_job, dst) == offsetof(DevPackJob, dst) && offsetof(struct ofdg_pack_job, width) == offsetof(DevPackJob, width) &&
              offsetof(struct ofdg_pack_job, image_src_fmt) == offsetof(DevPackJob, image_src_fmt) && offsetof(struct ofdg_pack_job, flow_dst_fmt) == offsetof(DevPackJob, flow_dst_fmt) &&
              offsetof(struct ofdg_pack_job, layout) == offsetof(DevPackJob, layout) && offsetof(struct ofdg_pack_job, flags) == offsetof(DevPackJob, flags) &&
              offsetof(DevPackJob, flags) == 76 && offsetof(struct ofdg_pack_job, scale) == offsetof(DevPackJob, scale) && offsetof(struct ofdg_pack_job, bias) == offsetof(DevPackJob, bias) &&
              offsetof(struct ofdg_pack_job, flow_scale) == offsetof(DevPackJob, flow_scale) && offsetof(struct ofdg_pack_job, reserved) == offsetof(DevPackJob, reserved) &&
              offsetof(DevPackJob, reserved) == 108 && OFDG_FMT_BF16 == 3 && OFDG_PACK_NHWC == 1 && OFDG_PACK_CONCAT == 1 && OFDG_PACK_RGB == 2,
              "struct ofdg_pack_job: 112 bytes, the layout the kernel takes; pack_kernel spells the codes out");
// y of a frame element x under its source channel's constants, and of a flow element u: each operation its own rounding
OFDG_HD_FN float pack_value(float x, float scale, float bias) {
  const float p = x * scale;
  return p + bias;
}
OFDG_HD_FN float pack_flow_value(float u, float flow_scale) { return u * flow_scale; }
// float32 -> bfloat16 to nearest even on the upper 16 bits; a NaN becomes 0x7FC0.  (b <= 0xFF800000 here: the sum stays
// inside 32 bits.)
OFDG_HD_FN uint32_t pack_bf16_bits(float y) {
  uint32_t b;
  memcpy(&b, &y, 4);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
  return (b + 0x7FFFu + ((b >> 16) & 1u)) >> 16;
}
// What is stored of y in a destination of `fmt`: 32 bits of float32, else 16
OFDG_HD_FN uint32_t pack_stored_bits(float y, int fmt) {
  if (fmt == OFDG_FMT_BF16) return pack_bf16_bits(y);
  if (fmt == OFDG_FMT_F16) return spatial_half_bits(y);
  const float q = spatial_quiet(y);
  uint32_t b;
  memcpy(&b, &q, 4);
  return b;
}
// channels of a destination plane; the destination channel of source channel c of frame f
OFDG_HD_FN int pack_channels(int plane, int flags) { return plane == OFDG_PACK_FLOW ? 2 : (flags & OFDG_PACK_CONCAT) ? 6 : 3; }
OFDG_HD_FN int pack_dst_channel(int f, int c, int flags) { return ((flags & OFDG_PACK_CONCAT) ? 3 * f : 0) + ((flags & OFDG_PACK_RGB) ? 2 - c : c); }
// element index of (sample i, destination channel cd, row y, column x) in a destination of C channels
OFDG_HD_FN size_t pack_dst_index(int layout, int C, int i, int cd, int y, int x, int width, int height) {
  if (layout == OFDG_PACK_NHWC) return (((size_t)i * height + y) * width + x) * C + cd;
  return (((size_t)i * C + cd) * height + y) * width + x;
}
inline bool pack_finite(float v) { return v >= -3.4028234663852886e38f && v <= 3.4028234663852886e38f; }
// The argument rules ofdg_pack and ofdg_host_pack share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment is asked by the device entry only.
inline const char* pack_arg_error(const DevPackJob* j, int n, int width, int height) {
  if (!j) return "job is NULL";
  if (n < 1) return "n_samples must be at least 1";
  if (6ull * (unsigned long long)width * (unsigned long long)height >= (1ull << 31)) return "6 * width * height must be below 2^31";
  if (j->image_src_fmt != OFDG_FMT_F32 && j->image_src_fmt != OFDG_FMT_U8) return "image_src_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->flow_src_fmt != OFDG_FMT_F32 && j->flow_src_fmt != OFDG_FMT_F16) return "flow_src_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if (j->image_dst_fmt != OFDG_FMT_F32 && j->image_dst_fmt != OFDG_FMT_F16 && j->image_dst_fmt != OFDG_FMT_BF16)
    return "image_dst_fmt must be OFDG_FMT_F32, OFDG_FMT_F16 or OFDG_FMT_BF16";
  if (j->flow_dst_fmt != OFDG_FMT_F32 && j->flow_dst_fmt != OFDG_FMT_F16 && j->flow_dst_fmt != OFDG_FMT_BF16)
    return "flow_dst_fmt must be OFDG_FMT_F32, OFDG_FMT_F16 or OFDG_FMT_BF16";
  if (j->layout != OFDG_PACK_NCHW && j->layout != OFDG_PACK_NHWC) return "layout must be OFDG_PACK_NCHW or OFDG_PACK_NHWC";
  if (j->flags & ~(OFDG_PACK_CONCAT | OFDG_PACK_RGB)) return "flags holds unknown bits";
  if (j->reserved != 0) return "reserved must be 0";
  for (int c = 0; c < 3; ++c) {
    if (!pack_finite(j->scale[c])) return "scale must be finite";
    if (!pack_finite(j->bias[c])) return "bias must be finite";
  }
  if (!pack_finite(j->flow_scale)) return "flow_scale must be finite";
  const bool concat = j->flags & OFDG_PACK_CONCAT;
  int planes = 0;
  for (int k = 0; k < kPackPlanes; ++k) {
    if (concat && k == OFDG_PACK_IMAGE1) continue;
    if (j->src[k] && !j->dst[k]) return "dst: a plane has a source and no destination";
    if (!j->src[k] && j->dst[k]) return "src: a plane has a destination and no source";
    planes += j->src[k] ? 1 : 0;
  }
  if (concat && (!j->src[OFDG_PACK_IMAGE0] || !j->src[OFDG_PACK_IMAGE1])) return "flags: OFDG_PACK_CONCAT needs both frames";
  if (concat && j->dst[OFDG_PACK_IMAGE1]) return "flags: OFDG_PACK_CONCAT takes dst[image1] NULL";
  if (!planes) return "src: no plane is set";
  // no in-place form: a destination range may meet no other range of the job
  RangeSet<2 * kPackPlanes> r;
  const unsigned long long per = (unsigned long long)n * width * height;
  for (int k = 0; k < kPackPlanes; ++k) {
    const bool flow = k == OFDG_PACK_FLOW;
    r.add_if(j->src[k], per * (flow ? 2 : 3) * fmt_elem_bytes(flow ? j->flow_src_fmt : j->image_src_fmt), false);
    r.add_if(j->dst[k], per * pack_channels(k, j->flags) * fmt_elem_bytes(flow ? j->flow_dst_fmt : j->image_dst_fmt), true);
  }
  return r.overlap("dst: a destination range overlaps another range of the job");
}

// ---- Motion boundaries (ofdg_boundaries, include/ofdg.h) -------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job as the kernel takes it, the pair rule and the argument
// rules.  Compiled without contraction, so the two squares and their sum are three roundings.
constexpr int kBndMaxRadius = 15;  // OFDG_BND_MAX_RADIUS
struct DevBoundaryJob {            // struct ofdg_boundary_job, field for field
  const void* flow[2];
  const uint8_t* label[2];
  uint8_t* edge[2];
  uint8_t* dist2[2];
  int32_t width, height, flow_fmt, flags, radius;
  float min_step;
  int32_t reserved[2];
};
static_assert(sizeof(struct ofdg_boundary_job) == sizeof(DevBoundaryJob) && sizeof(DevBoundaryJob) == 96 && OFDG_BND_MAX_RADIUS == kBndMaxRadius &&
              offsetof(struct ofdg_boundary_job, label) == offsetof(DevBoundaryJob, label) && offsetof(struct ofdg_boundary_job, edge) == offsetof(DevBoundaryJob, edge) &&
              offsetof(struct ofdg_boundary_job, dist2) == offsetof(DevBoundaryJob, dist2) && offsetof(struct ofdg_boundary_job, width) == offsetof(DevBoundaryJob, width) &&
              offsetof(DevBoundaryJob, width) == 64 && offsetof(struct ofdg_boundary_job, flow_fmt) == offsetof(DevBoundaryJob, flow_fmt) &&
              offsetof(struct ofdg_boundary_job, flags) == offsetof(DevBoundaryJob, flags) && offsetof(struct ofdg_boundary_job, radius) == offsetof(DevBoundaryJob, radius) &&
              offsetof(struct ofdg_boundary_job, min_step) == offsetof(DevBoundaryJob, min_step) && offsetof(DevBoundaryJob, min_step) == 84 &&
              offsetof(struct ofdg_boundary_job, reserved) == offsetof(DevBoundaryJob, reserved) && OFDG_BND_LABELS == 1 && OFDG_BND_FAR == 255,
              "struct ofdg_boundary_job: 96 bytes, the layout the kernel takes; boundary_kernel spells the codes out");
// Are the 4-neighbours p and q a step?  (u, v) of each widened to float32, t2 = fl32(min_step * min_step); with kLabels the
// caller has compared the labels.  A NaN d2 compares false.
OFDG_HD_FN bool boundary_step(float up, float vp, float uq, float vq, float t2) {
  const float du = up - uq, dv = vp - vq;
  const float a = du * du, b = dv * dv;
  const float d2 = a + b;
  return d2 > t2;
}
OFDG_HD_FN float boundary_threshold(float min_step) { return min_step * min_step; }
// The argument rules ofdg_boundaries and ofdg_host_boundaries share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment is asked by the device entry only.
inline const char* boundary_arg_error(const DevBoundaryJob* j, int n, int width, int height) {
  if (!j) return "job is NULL";
  if (const char* why = batch_plane_error(n, width, height)) return why;
  if ((unsigned long long)width * (unsigned long long)height >= (1ull << 31)) return "width * height must be below 2^31";
  if (j->flags & ~OFDG_BND_LABELS) return "flags holds unknown bits";
  if (j->reserved[0] != 0 || j->reserved[1] != 0) return "reserved must be 0";
  if (j->flow_fmt != OFDG_FMT_F32 && j->flow_fmt != OFDG_FMT_F16) return "flow_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if (!j->flow[0] && !j->flow[1]) return "flow: no frame is present";
  for (int f = 0; f < 2; ++f) {
    if (!j->flow[f] && j->edge[f]) return "edge: an output of a frame without its flow";
    if (!j->flow[f] && j->dist2[f]) return "dist2: an output of a frame without its flow";
    if (j->flow[f] && !j->edge[f] && !j->dist2[f]) return "edge, dist2: a frame has a flow and no output";
    if (j->flow[f] && (j->flags & OFDG_BND_LABELS) && !j->label[f]) return "label: OFDG_BND_LABELS needs the label plane of every frame present";
  }
  if (!(j->min_step >= 0.0f && j->min_step <= 3.4028234663852886e38f)) return "min_step must be finite and not negative";
  if ((j->dist2[0] || j->dist2[1]) && (j->radius < 1 || j->radius > kBndMaxRadius)) return "radius must lie in 1..15";
  // an output may meet no other range of the job
  RangeSet<8> r;
  const unsigned long long plane = (unsigned long long)n * width * height;
  for (int f = 0; f < 2; ++f) {
    if (!j->flow[f]) continue;
    r.add(j->flow[f], plane * 2 * fmt_elem_bytes(j->flow_fmt), false);
    r.add_if(j->label[f], plane, false);
    r.add_if(j->edge[f], plane, true);
    r.add_if(j->dist2[f], plane, true);
  }
  return r.overlap("edge, dist2: an output range overlaps another range of the job");
}

// ---- Occluder rectangles (ofdg_erase, include/ofdg.h) ----------------------------------------------------------------------
// What the device entry, the kernels and the host twin share: the job as the kernels take it, the record's draw and its
// sanitising, the integer mean, the noise byte, the target test of the occlusion rule and the argument rules.
constexpr int kEraseMaxRects = 4;  // OFDG_ERASE_MAX_RECTS
struct DevEraseRect {
  int32_t x0, y0, w, h, frame;
};
struct DevEraseRec {  // ofdg_erase_rec, field for field
  int32_t count;
  DevEraseRect rect[kEraseMaxRects];
  uint8_t fill[2][3];
  uint8_t reserved[6];
};
struct DevEraseWork {  // one sample's part of job->work: the Q8 sums of the frames that have a rectangle
  unsigned long long sum[2][3];
  unsigned long long pad[2];
};
struct DevEraseJob {  // struct ofdg_erase_job, field for field
  void* image[2];
  void* occ[2];
  const void* flow[2];
  const DevEraseRec* recs;
  DevEraseRec* recs_out;
  DevEraseWork* work;
  long long first_index;
  uint32_t seed;
  int32_t width, height, image_fmt, occ_fmt, flow_fmt, flags, fill;
  int32_t min_rects, max_rects, min_size, max_size;
  float prob;
  int32_t color[3];
  int32_t reserved[2];
};
static_assert(sizeof(ofdg_erase_rec) == sizeof(DevEraseRec) && sizeof(DevEraseRec) == 96 && sizeof(ofdg_erase_rect) == sizeof(DevEraseRect) &&
              offsetof(ofdg_erase_rec, rect) == offsetof(DevEraseRec, rect) && offsetof(DevEraseRec, rect) == 4 && offsetof(ofdg_erase_rec, fill) == offsetof(DevEraseRec, fill) &&
              offsetof(DevEraseRec, fill) == 84 && offsetof(ofdg_erase_rec, reserved) == offsetof(DevEraseRec, reserved) && offsetof(DevEraseRec, reserved) == 90 &&
              OFDG_ERASE_MAX_RECTS == kEraseMaxRects && sizeof(DevEraseWork) == OFDG_ERASE_WORK_BYTES,
              "ofdg_erase_rec: 96 bytes, the layout the kernels read and write as six 16-byte pieces; a sample's workspace");
static_assert(sizeof(struct ofdg_erase_job) == sizeof(DevEraseJob) && sizeof(DevEraseJob) == 152 && offsetof(struct ofdg_erase_job, occ) == offsetof(DevEraseJob, occ) &&
              offsetof(struct ofdg_erase_job, flow) == offsetof(DevEraseJob, flow) && offsetof(struct ofdg_erase_job, recs) == offsetof(DevEraseJob, recs) &&
              offsetof(struct ofdg_erase_job, recs_out) == offsetof(DevEraseJob, recs_out) && offsetof(struct ofdg_erase_job, work) == offsetof(DevEraseJob, work) &&
              offsetof(struct ofdg_erase_job, first_index) == offsetof(DevEraseJob, first_index) && offsetof(struct ofdg_erase_job, seed) == offsetof(DevEraseJob, seed) &&
              offsetof(DevEraseJob, seed) == 80 && offsetof(struct ofdg_erase_job, width) == offsetof(DevEraseJob, width) &&
              offsetof(struct ofdg_erase_job, image_fmt) == offsetof(DevEraseJob, image_fmt) && offsetof(struct ofdg_erase_job, fill) == offsetof(DevEraseJob, fill) &&
              offsetof(struct ofdg_erase_job, min_rects) == offsetof(DevEraseJob, min_rects) && offsetof(DevEraseJob, min_rects) == 112 &&
              offsetof(struct ofdg_erase_job, prob) == offsetof(DevEraseJob, prob) && offsetof(struct ofdg_erase_job, color) == offsetof(DevEraseJob, color) &&
              offsetof(struct ofdg_erase_job, reserved) == offsetof(DevEraseJob, reserved) && offsetof(DevEraseJob, reserved) == 144 && OFDG_ERASE_FRAME0 == 1 &&
              OFDG_ERASE_FRAME1 == 2 && OFDG_ERASE_OCC == 4 && OFDG_ERASE_MEAN == 0 && OFDG_ERASE_CONST == 1 && OFDG_ERASE_NOISE == 2,
              "struct ofdg_erase_job: 152 bytes, the layout the kernels take; the helpers below spell the codes out");
// lo + floor(w * (hi - lo + 1) / 2^32): the multiply-shift of the crop's draw
OFDG_HD_FN int32_t erase_pick(uint32_t w, int32_t lo, int32_t hi) { return lo + (int32_t)(uint32_t)(((unsigned long long)w * (uint32_t)(hi - lo + 1)) >> 32); }
// The record of global sample g for a width x height plane: Philox blocks 0..4 under the sampler's key of g at the counters
// {j, 0, 0x0c74, 0}.  `j` supplies flags, prob and the four ranges (erase_ranges_error has passed).  Not sanitised.  Here and
// below the four rectangles are spelled out one by one, never indexed by a variable: a kernel then keeps the record in
// registers.
OFDG_HD_FN DevEraseRect erase_draw_rect(int k, int count, uint32_t frame_bits, uint32_t k0, uint32_t k1, int width, int height, const DevEraseJob& j) {
  const CropWords b = crop_philox(CropWords{(uint32_t)k + 1u, 0u, 0x0c74u, 0u}, k0, k1);
  const int frames = j.flags & 3;
  const bool on = k < count;
  DevEraseRect q;
  q.x0 = on ? erase_pick(b.z, 0, width - 1) : 0;
  q.y0 = on ? erase_pick(b.w, 0, height - 1) : 0;
  q.w = on ? erase_pick(b.x, j.min_size, j.max_size) : 0;
  q.h = on ? erase_pick(b.y, j.min_size, j.max_size) : 0;
  q.frame = on ? (frames == 3 ? (int32_t)((frame_bits >> k) & 1u) : frames == 2 ? 1 : 0) : 0;
  return q;
}
OFDG_HD_FN DevEraseRec erase_draw_rec(uint32_t seed, unsigned long long g, int width, int height, const DevEraseJob& j) {
  const uint32_t k0 = seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
  const CropWords a = crop_philox(CropWords{0u, 0u, 0x0c74u, 0u}, k0, k1);
  DevEraseRec r;
  const bool erased = photo_unit(a.x) < j.prob;
  r.count = erased ? erase_pick(a.y, j.min_rects, j.max_rects) : 0;
  r.rect[0] = erase_draw_rect(0, r.count, a.z, k0, k1, width, height, j);
  r.rect[1] = erase_draw_rect(1, r.count, a.z, k0, k1, width, height, j);
  r.rect[2] = erase_draw_rect(2, r.count, a.z, k0, k1, width, height, j);
  r.rect[3] = erase_draw_rect(3, r.count, a.z, k0, k1, width, height, j);
  r.fill[0][0] = r.fill[0][1] = r.fill[0][2] = r.fill[1][0] = r.fill[1][1] = r.fill[1][2] = 0;
  r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = r.reserved[4] = r.reserved[5] = 0;
  return r;
}
// What is used of a record, given or drawn: the rectangles of flagged frames, clipped to the plane, the empty ones dropped
// and the kept ones moved to the front in their order; everything else 0.
OFDG_HD_FN DevEraseRect erase_clip(const DevEraseRect& q, bool counted, int width, int height, int flags, bool* keep) {
  const int f = q.frame & 1;
  const long long x0 = q.x0 < 0 ? 0 : q.x0, y0 = q.y0 < 0 ? 0 : q.y0;
  const long long xe = (long long)q.x0 + q.w, ye = (long long)q.y0 + q.h;
  const long long x1 = xe < width ? xe : width, y1 = ye < height ? ye : height;
  *keep = counted && ((flags >> f) & 1) && q.w >= 1 && q.h >= 1 && x1 > x0 && y1 > y0;
  return DevEraseRect{(int32_t)x0, (int32_t)y0, (int32_t)(x1 - x0), (int32_t)(y1 - y0), f};
}
// a if on, else b - field by field and on values: a conditional between members would select their addresses
OFDG_HD_FN int32_t erase_select_int(bool on, int32_t a, int32_t b) { return on ? a : b; }
OFDG_HD_FN DevEraseRect erase_select(bool on, const DevEraseRect& a, const DevEraseRect& b) {
  return DevEraseRect{erase_select_int(on, a.x0, b.x0), erase_select_int(on, a.y0, b.y0), erase_select_int(on, a.w, b.w), erase_select_int(on, a.h, b.h),
                      erase_select_int(on, a.frame, b.frame)};
}
OFDG_HD_FN DevEraseRec erase_sanitise(const DevEraseRec& in, int width, int height, int flags) {
  const int count = in.count < 0 ? 0 : in.count > kEraseMaxRects ? kEraseMaxRects : in.count;
  bool k0, k1, k2, k3;
  const DevEraseRect o0 = erase_clip(in.rect[0], count > 0, width, height, flags, &k0), o1 = erase_clip(in.rect[1], count > 1, width, height, flags, &k1);
  const DevEraseRect o2 = erase_clip(in.rect[2], count > 2, width, height, flags, &k2), o3 = erase_clip(in.rect[3], count > 3, width, height, flags, &k3);
  const int p1 = k0 ? 1 : 0, p2 = p1 + (k1 ? 1 : 0), p3 = p2 + (k2 ? 1 : 0);  // the kept ones in front of rectangle 1, 2, 3
  const DevEraseRect none = DevEraseRect{0, 0, 0, 0, 0};
  DevEraseRec r;
  r.count = p3 + (k3 ? 1 : 0);
  r.rect[0] = erase_select(k0, o0, erase_select(k1 && p1 == 0, o1, erase_select(k2 && p2 == 0, o2, erase_select(k3 && p3 == 0, o3, none))));
  r.rect[1] = erase_select(k1 && p1 == 1, o1, erase_select(k2 && p2 == 1, o2, erase_select(k3 && p3 == 1, o3, none)));
  r.rect[2] = erase_select(k2 && p2 == 2, o2, erase_select(k3 && p3 == 2, o3, none));
  r.rect[3] = erase_select(k3 && p3 == 3, o3, none);
  r.fill[0][0] = r.fill[0][1] = r.fill[0][2] = r.fill[1][0] = r.fill[1][1] = r.fill[1][2] = 0;
  r.reserved[0] = r.reserved[1] = r.reserved[2] = r.reserved[3] = r.reserved[4] = r.reserved[5] = 0;
  return r;
}
// bit f: frame f has a rectangle (of a sanitised record)
OFDG_HD_FN int erase_frames_of(const DevEraseRec& r) {
  return (r.count > 0 ? 1 << r.rect[0].frame : 0) | (r.count > 1 ? 1 << r.rect[1].frame : 0) | (r.count > 2 ? 1 << r.rect[2].frame : 0) |
         (r.count > 3 ? 1 << r.rect[3].frame : 0);
}
// The Q8 value of a float32 element: clamped to [0, 255] (a NaN becomes 0), times 256, to nearest even.
OFDG_HD_FN uint32_t erase_q8(float v) {
  v = v > 0.0f ? v : 0.0f;
  v = v < 255.0f ? v : 255.0f;
  return (uint32_t)rintf(v * 256.0f);
}
// The fill byte of a channel whose P elements sum to S in Q8: the mean rounded half up to Q8, then half up to a byte.
OFDG_HD_FN uint32_t erase_mean_byte(unsigned long long S, unsigned long long P) {
  const unsigned long long mean_q8 = (2ull * S + P) / (2ull * P);
  return (uint32_t)((mean_q8 + 128ull) >> 8);
}
// The noise byte of element e of frame f: the top byte of word e & 3 of the block {e >> 2, f, 0x0c75, 0}.
OFDG_HD_FN uint32_t erase_noise_word(const CropWords& w, uint32_t e) { return ((e & 3u) == 0u ? w.x : (e & 3u) == 1u ? w.y : (e & 3u) == 2u ? w.z : w.w) >> 24; }
OFDG_HD_FN uint32_t erase_noise_byte(uint32_t k0, uint32_t k1, int f, uint32_t e) {
  return erase_noise_word(crop_philox(CropWords{e >> 2, (uint32_t)f, 0x0c75u, 0u}, k0, k1), e);
}
// Does the flow target of (x, y) with displacement (u, v) lie inside rectangle q?  The crop's formula per axis.
OFDG_HD_FN bool erase_target_inside(int x, int y, float u, float v, const DevEraseRect& q) {
  return crop_target_inside(x, u, q.x0, q.w) && crop_target_inside(y, v, q.y0, q.h);
}
OFDG_HD_FN bool erase_inside(int x, int y, const DevEraseRect& q) { return x >= q.x0 && x < q.x0 + q.w && y >= q.y0 && y < q.y0 + q.h; }
OFDG_HD_FN bool erase_marks_one(const DevEraseRect& q, int f, bool cross, int x, int y, float u, float v) {
  return q.frame == f ? erase_inside(x, y, q) : cross && erase_target_inside(x, y, u, v, q);
}
// Is element (x, y) of the map of frame f marked by a sanitised record?  cross: frame 1 - f is flagged and (u, v) is the
// element's flow[f].
OFDG_HD_FN bool erase_marks(const DevEraseRec& r, int f, bool cross, int x, int y, float u, float v) {
  // (spelled out rectangle by rectangle: no indexed access, so a kernel keeps the record in registers)
  return (r.count > 0 && erase_marks_one(r.rect[0], f, cross, x, y, u, v)) || (r.count > 1 && erase_marks_one(r.rect[1], f, cross, x, y, u, v)) ||
         (r.count > 2 && erase_marks_one(r.rect[2], f, cross, x, y, u, v)) || (r.count > 3 && erase_marks_one(r.rect[3], f, cross, x, y, u, v));
}
// does the map of frame f need its flow?  (OFDG_ERASE_OCC, the map given, frame 1 - f flagged)
OFDG_HD_FN bool erase_cross(const DevEraseJob& j, int f) { return (j.flags & OFDG_ERASE_OCC) && j.occ[f] && ((j.flags >> (1 - f)) & 1); }
// What the draw reads of a job: the first rule broken, or nullptr.
inline const char* erase_ranges_error(const DevEraseJob& j) {
  if (j.flags & ~(OFDG_ERASE_FRAME0 | OFDG_ERASE_FRAME1 | OFDG_ERASE_OCC)) return "flags holds unknown bits";
  if (!(j.flags & (OFDG_ERASE_FRAME0 | OFDG_ERASE_FRAME1))) return "flags: OFDG_ERASE_FRAME0 or OFDG_ERASE_FRAME1 must be set";
  if (!(j.prob >= 0.0f && j.prob <= 1.0f)) return "prob must lie in [0, 1]";
  if (j.min_rects < 0 || j.max_rects > kEraseMaxRects || j.min_rects > j.max_rects) return "min_rects <= max_rects must lie in 0..4";
  if (j.min_size < 1 || j.max_size > 32767 || j.min_size > j.max_size) return "min_size <= max_size must lie in 1..32767";
  return nullptr;
}
// The argument rules ofdg_erase and ofdg_host_erase share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment and `work` are asked by the device entry only (with_work).
inline const char* erase_arg_error(const DevEraseJob* j, int n, int width, int height, bool with_work) {
  if (!j) return "job is NULL";
  if (n < 1) return "n_samples must be at least 1";
  if (3ull * (unsigned long long)width * (unsigned long long)height >= (1ull << 31)) return "3 * width * height must be below 2^31";
  if (j->image_fmt != OFDG_FMT_F32 && j->image_fmt != OFDG_FMT_U8) return "image_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->flags & ~(OFDG_ERASE_FRAME0 | OFDG_ERASE_FRAME1 | OFDG_ERASE_OCC)) return "flags holds unknown bits";
  if (j->reserved[0] != 0 || j->reserved[1] != 0) return "reserved must be 0";
  if (!(j->flags & (OFDG_ERASE_FRAME0 | OFDG_ERASE_FRAME1))) return "flags: OFDG_ERASE_FRAME0 or OFDG_ERASE_FRAME1 must be set";
  if (!j->image[0] && !j->image[1]) return "image: no frame is set";
  for (int f = 0; f < 2; ++f)
    if (((j->flags >> f) & 1) && !j->image[f]) return "image: a flagged frame has no image";
  if (j->fill != OFDG_ERASE_MEAN && j->fill != OFDG_ERASE_CONST && j->fill != OFDG_ERASE_NOISE) return "fill must be OFDG_ERASE_MEAN, OFDG_ERASE_CONST or OFDG_ERASE_NOISE";
  if (j->fill == OFDG_ERASE_CONST)
    for (int c = 0; c < 3; ++c)
      if (j->color[c] < 0 || j->color[c] > 255) return "color must lie in 0..255";
  if (!j->recs)
    if (const char* why = erase_ranges_error(*j)) return why;
  const bool occ = j->flags & OFDG_ERASE_OCC;
  if (occ) {
    if (!j->occ[0] && !j->occ[1]) return "occ: OFDG_ERASE_OCC needs a map";
    if (j->occ_fmt != OFDG_FMT_F32 && j->occ_fmt != OFDG_FMT_U8) return "occ_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
    for (int f = 0; f < 2; ++f)
      if (erase_cross(*j, f)) {
        if (!j->flow[f]) return "flow: a map needs its flow when the other frame is flagged";
        if (j->flow_fmt != OFDG_FMT_F32 && j->flow_fmt != OFDG_FMT_F16) return "flow_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
      }
  }
  const bool work = with_work && j->fill == OFDG_ERASE_MEAN;
  if (work && !j->work) return "work is NULL under OFDG_ERASE_MEAN";
  // a written range may meet no other range of the job
  RangeSet<9> r;
  const unsigned long long plane = (unsigned long long)n * width * height;
  for (int f = 0; f < 2; ++f) {
    if (((j->flags >> f) & 1)) r.add(j->image[f], plane * 3 * fmt_elem_bytes(j->image_fmt), true);
    if (occ && j->occ[f]) r.add(j->occ[f], plane * fmt_elem_bytes(j->occ_fmt), true);
    if (erase_cross(*j, f)) r.add(j->flow[f], plane * 2 * fmt_elem_bytes(j->flow_fmt), false);
  }
  r.add_if(j->recs, (unsigned long long)n * sizeof(DevEraseRec), false);
  r.add_if(j->recs_out, (unsigned long long)n * sizeof(DevEraseRec), true);
  if (work) r.add(j->work, (unsigned long long)n * sizeof(DevEraseWork), true);
  return r.overlap("a written range overlaps another range of the job");
}

// ---- Colour jitter (ofdg_jitter, include/ofdg.h) ---------------------------------------------------------------------------
// What the device entry, the kernels and the host twin share: the job as the kernels take it, the record's draw and its
// sanitising, the order's decoding, the four operations on the bytes of a pixel, the mean and the argument rules.  Integers
// throughout; >> of a negative int is the arithmetic shift on every compiler this builds with.
struct DevJitterRec {  // ofdg_jitter_rec, field for field
  int32_t brightness[2], contrast[2], saturation[2], hue[2], order[2], shared, mean[2], reserved[3];
};
struct DevJitterWork {  // one sample's part of job->work: the luminance sums of the frames whose contrast needs a mean
  unsigned long long sum[2];
};
struct DevJitterJob {  // struct ofdg_jitter_job, field for field
  const void* src[2];
  void* dst[2];
  const DevJitterRec* recs;
  DevJitterRec* recs_out;
  DevJitterWork* work;
  long long first_index;
  uint32_t seed;
  int32_t width, height, src_fmt, dst_fmt, flags, reserved;
  float brightness, contrast, saturation, hue, asym_prob;
};
static_assert(sizeof(ofdg_jitter_rec) == sizeof(DevJitterRec) && sizeof(DevJitterRec) == 64 && offsetof(ofdg_jitter_rec, hue) == offsetof(DevJitterRec, hue) &&
              offsetof(DevJitterRec, hue) == 24 && offsetof(ofdg_jitter_rec, order) == offsetof(DevJitterRec, order) && offsetof(ofdg_jitter_rec, shared) == offsetof(DevJitterRec, shared) &&
              offsetof(DevJitterRec, shared) == 40 && offsetof(ofdg_jitter_rec, mean) == offsetof(DevJitterRec, mean) && offsetof(ofdg_jitter_rec, reserved) == offsetof(DevJitterRec, reserved) &&
              offsetof(DevJitterRec, reserved) == 52 && sizeof(DevJitterWork) == OFDG_JITTER_WORK_BYTES,
              "ofdg_jitter_rec: 64 bytes, the layout the kernels read and write as four 16-byte pieces; a sample's workspace");
static_assert(sizeof(struct ofdg_jitter_job) == sizeof(DevJitterJob) && sizeof(DevJitterJob) == 112 && offsetof(struct ofdg_jitter_job, dst) == offsetof(DevJitterJob, dst) &&
              offsetof(struct ofdg_jitter_job, recs) == offsetof(DevJitterJob, recs) && offsetof(struct ofdg_jitter_job, recs_out) == offsetof(DevJitterJob, recs_out) &&
              offsetof(struct ofdg_jitter_job, work) == offsetof(DevJitterJob, work) && offsetof(struct ofdg_jitter_job, first_index) == offsetof(DevJitterJob, first_index) &&
              offsetof(struct ofdg_jitter_job, seed) == offsetof(DevJitterJob, seed) && offsetof(DevJitterJob, seed) == 64 && offsetof(struct ofdg_jitter_job, width) == offsetof(DevJitterJob, width) &&
              offsetof(struct ofdg_jitter_job, src_fmt) == offsetof(DevJitterJob, src_fmt) && offsetof(struct ofdg_jitter_job, reserved) == offsetof(DevJitterJob, reserved) &&
              offsetof(struct ofdg_jitter_job, brightness) == offsetof(DevJitterJob, brightness) && offsetof(DevJitterJob, brightness) == 92 &&
              offsetof(struct ofdg_jitter_job, asym_prob) == offsetof(DevJitterJob, asym_prob) && offsetof(DevJitterJob, asym_prob) == 108,
              "struct ofdg_jitter_job: 112 bytes, the layout the kernels take");
constexpr int kJitterOne = 65536;      // a Q16 factor that changes nothing; the hue units of one sector
constexpr int kJitterTurn = 393216;    // the hue units of a whole turn
enum { kJitterBrightness = 0, kJitterContrast = 1, kJitterSaturation = 2, kJitterHue = 3 };  // the operations as order[f] permutes them
// The five fields of one frame of a record (by value: a conditional between members would select their addresses).
struct JitterFrame {
  int32_t brightness, contrast, saturation, hue, order;
};
OFDG_HD_FN JitterFrame jitter_frame(const DevJitterRec& r, int f) {
  return JitterFrame{f ? r.brightness[1] : r.brightness[0], f ? r.contrast[1] : r.contrast[0], f ? r.saturation[1] : r.saturation[0], f ? r.hue[1] : r.hue[0],
                     f ? r.order[1] : r.order[0]};
}
OFDG_HD_FN bool jitter_same(const JitterFrame& a, const JitterFrame& b) {
  return a.brightness == b.brightness && a.contrast == b.contrast && a.saturation == b.saturation && a.hue == b.hue && a.order == b.order;
}
// does nothing to any pixel: the frame is copied
OFDG_HD_FN bool jitter_identity(const JitterFrame& p) { return p.brightness == kJitterOne && p.contrast == kJitterOne && p.saturation == kJitterOne && p.hue == 0; }
// A = lrintf(range * unit), to nearest even; isym(w, A) uniform on [-A, A] by the multiply-shift of the crop's draw
OFDG_HD_FN int32_t jitter_amp(float range, float unit) { return (int32_t)lrintf(range * unit); }
OFDG_HD_FN int32_t jitter_isym(uint32_t w, int32_t A) { return (int32_t)(uint32_t)(((unsigned long long)w * (uint32_t)(2 * A + 1)) >> 32) - A; }
// The record of global sample g: Philox blocks 0, 1, 2 under the sampler's key of g and the counters {j, 0, 0x0c78, 0}.  `j`
// supplies the five ranges (jitter_ranges_error has passed).  Not sanitised.
OFDG_HD_FN DevJitterRec jitter_draw_rec(uint32_t seed, unsigned long long g, const DevJitterJob& j) {
  const uint32_t k0 = seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
  const CropWords a = crop_philox(CropWords{0u, 0u, 0x0c78u, 0u}, k0, k1);
  const CropWords b = crop_philox(CropWords{1u, 0u, 0x0c78u, 0u}, k0, k1);
  const CropWords d = crop_philox(CropWords{2u, 0u, 0x0c78u, 0u}, k0, k1);
  const int32_t Ab = jitter_amp(j.brightness, 65536.0f), Ac = jitter_amp(j.contrast, 65536.0f), As = jitter_amp(j.saturation, 65536.0f);
  const int32_t Ah = jitter_amp(j.hue, 393216.0f);
  const bool asym = photo_unit(d.x) < j.asym_prob;
  DevJitterRec r;
  r.brightness[0] = kJitterOne + jitter_isym(a.x, Ab); r.contrast[0] = kJitterOne + jitter_isym(a.y, Ac);
  r.saturation[0] = kJitterOne + jitter_isym(a.z, As); r.hue[0] = jitter_isym(a.w, Ah);
  r.order[0] = (int32_t)(((d.y >> 8) * 24u) >> 24);
  r.brightness[1] = asym ? kJitterOne + jitter_isym(b.x, Ab) : r.brightness[0]; r.contrast[1] = asym ? kJitterOne + jitter_isym(b.y, Ac) : r.contrast[0];
  r.saturation[1] = asym ? kJitterOne + jitter_isym(b.z, As) : r.saturation[0]; r.hue[1] = asym ? jitter_isym(b.w, Ah) : r.hue[0];
  r.order[1] = asym ? (int32_t)(((d.z >> 8) * 24u) >> 24) : r.order[0];
  r.shared = asym ? 0 : 1;
  r.mean[0] = -1; r.mean[1] = -1;
  r.reserved[0] = 0; r.reserved[1] = 0; r.reserved[2] = 0;
  return r;
}
OFDG_HD_FN int32_t jitter_clamp(int32_t x, int32_t lo, int32_t hi) { return x < lo ? lo : x > hi ? hi : x; }
// What is used of a record, given or drawn.  No record makes a kernel touch a byte outside a plane.
OFDG_HD_FN DevJitterRec jitter_sanitise(DevJitterRec r) {
  for (int f = 0; f < 2; ++f) {
    r.brightness[f] = jitter_clamp(r.brightness[f], 0, 4 * kJitterOne);
    r.contrast[f] = jitter_clamp(r.contrast[f], 0, 4 * kJitterOne);
    r.saturation[f] = jitter_clamp(r.saturation[f], 0, 4 * kJitterOne);
    r.hue[f] = jitter_clamp(r.hue[f], -kJitterTurn / 2, kJitterTurn / 2);
    r.order[f] = jitter_clamp(r.order[f], 0, 23);
    r.mean[f] = -1;
  }
  r.shared = (r.shared != 0 && jitter_same(jitter_frame(r, 0), jitter_frame(r, 1))) ? 1 : 0;
  r.reserved[0] = 0; r.reserved[1] = 0; r.reserved[2] = 0;
  return r;
}
// The permutation number `order` names, as four nibbles: the operation at place p is (ops >> 4 p) & 15.  The factorial
// digits of order pick, place by place, among the operations still left (kept as nibbles too, in rising order).
OFDG_HD_FN uint32_t jitter_pop(uint32_t* left, int i) {
  const uint32_t sh = 4u * (uint32_t)i, v = (*left >> sh) & 15u;
  *left = (*left & ((1u << sh) - 1u)) | ((*left >> (sh + 4u)) << sh);
  return v;
}
OFDG_HD_FN uint32_t jitter_ops(int order) {
  const int i0 = order / 6, rest = order - 6 * i0, i1 = rest / 2, i2 = rest - 2 * i1;
  uint32_t left = 0x3210u;
  const uint32_t o0 = jitter_pop(&left, i0), o1 = jitter_pop(&left, i1), o2 = jitter_pop(&left, i2);
  return o0 | (o1 << 4) | (o2 << 8) | ((left & 15u) << 12);
}
OFDG_HD_FN int jitter_op_at(uint32_t ops, int place) { return (int)((ops >> (4 * place)) & 15u); }
// the place of the contrast: the operations in front of it shape the image its mean is taken of
OFDG_HD_FN int jitter_contrast_place(uint32_t ops) {
  return jitter_op_at(ops, 0) == kJitterContrast ? 0 : jitter_op_at(ops, 1) == kJitterContrast ? 1 : jitter_op_at(ops, 2) == kJitterContrast ? 2 : 3;
}
OFDG_HD_FN int jitter_lum(int B, int G, int R) { return (7471 * B + 38470 * G + 19595 * R + 32768) >> 16; }
OFDG_HD_FN int jitter_mix(int a, int m, int q) {
  const int v = (q * a + (kJitterOne - q) * m + 32768) >> 16;
  return v < 0 ? 0 : v > 255 ? 255 : v;
}
// floor(num / d) for 0 <= num < 2^24 and 1 <= d <= 255, exact.  On the device: the product with the hardware's reciprocal
// (off by less than 2^-6 here, so its integer part is the quotient or a neighbour) and one correction step either way,
// measured against the compiler's integer division (CHANGELOG; tools/patches/jitter_integer_division.patch).
OFDG_HD_FN int jitter_div(int num, int d) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int q = (int)((float)num * __builtin_amdgcn_rcpf((float)d));
  const int r = num - q * d;
  return q + (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
#else
  return num / d;
#endif
}
// The hue shift of one pixel.  A grey pixel (d = 0) falls out unchanged: t = 0 and every channel becomes mn + 0.
OFDG_HD_FN void jitter_hue(int& B, int& G, int& R, int hue) {
  const int mx = R > G ? (R > B ? R : B) : (G > B ? G : B), mn = R < G ? (R < B ? R : B) : (G < B ? G : B), d = mx - mn;
  const int s = (R == mx && B == mn) ? 0 : (G == mx && B == mn) ? 1 : (G == mx && R == mn) ? 2 : (B == mx && R == mn) ? 3 : (B == mx && G == mn) ? 4 : 5;
  const int mid = (s == 0 || s == 3) ? G : (s == 1 || s == 4) ? R : B;
  const int t = (s & 1) ? d - (mid - mn) : mid - mn;
  int hq = kJitterOne * s + jitter_div(kJitterOne * t, d > 0 ? d : 1) + hue;  // within a turn of [0, kJitterTurn) for any hue in [-kJitterTurn, kJitterTurn]
  hq += hq < 0 ? kJitterTurn : 0;
  hq -= hq >= kJitterTurn ? kJitterTurn : 0;
  const int s2 = hq >> 16, f2 = hq & 65535;
  const int nm = mn + ((d * ((s2 & 1) ? kJitterOne - f2 : f2) + 32768) >> 16);
  R = (s2 == 0 || s2 == 5) ? mx : (s2 == 2 || s2 == 3) ? mn : nm;
  G = (s2 == 1 || s2 == 2) ? mx : (s2 == 4 || s2 == 5) ? mn : nm;
  B = (s2 == 3 || s2 == 4) ? mx : (s2 == 0 || s2 == 1) ? mn : nm;
}
// One operation on one pixel; `mean` is looked at by the contrast only.
OFDG_HD_FN void jitter_op(int op, const JitterFrame& p, int mean, int& B, int& G, int& R) {
  if (op == kJitterBrightness) {
    B = jitter_mix(B, 0, p.brightness); G = jitter_mix(G, 0, p.brightness); R = jitter_mix(R, 0, p.brightness);
  } else if (op == kJitterContrast) {
    B = jitter_mix(B, mean, p.contrast); G = jitter_mix(G, mean, p.contrast); R = jitter_mix(R, mean, p.contrast);
  } else if (op == kJitterSaturation) {
    const int l = jitter_lum(B, G, R);
    B = jitter_mix(B, l, p.saturation); G = jitter_mix(G, l, p.saturation); R = jitter_mix(R, l, p.saturation);
  } else {
    jitter_hue(B, G, R, p.hue);
  }
}
// (2 S + N) / (2 N): the mean of N luminances, to nearest, a tie upwards
OFDG_HD_FN int32_t jitter_mean_byte(unsigned long long S, unsigned long long N) { return (int32_t)((2ull * S + N) / (2ull * N)); }
// The five ranges of the draw: the first that is negative, NaN, infinite or above its bound, or nullptr.
inline const char* jitter_ranges_error(const DevJitterJob& j) {
  if (!(j.brightness >= 0.0f && j.brightness <= 3.0f)) return "brightness must lie in [0, 3]";
  if (!(j.contrast >= 0.0f && j.contrast <= 3.0f)) return "contrast must lie in [0, 3]";
  if (!(j.saturation >= 0.0f && j.saturation <= 3.0f)) return "saturation must lie in [0, 3]";
  if (!(j.hue >= 0.0f && j.hue <= 0.5f)) return "hue must lie in [0, 0.5]";
  if (!(j.asym_prob >= 0.0f && j.asym_prob <= 1.0f)) return "asym_prob must lie in [0, 1]";
  return nullptr;
}
// Can a record of this job have a contrast, so that the device entry needs `work`?  Given records are not looked at on the
// host: they always can.
inline bool jitter_needs_work(const DevJitterJob& j) { return j.recs || jitter_amp(j.contrast, 65536.0f) != 0; }
// The argument rules ofdg_jitter and ofdg_host_jitter share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment and `work` are asked by the device entry only (with_work).
inline const char* jitter_arg_error(const DevJitterJob* j, int n, int width, int height, bool with_work) {
  if (const char* why = frame_pair_fmt_error(j, n, width, height)) return why;
  if (j->flags != 0) return "flags must be 0";
  if (j->reserved != 0) return "reserved must be 0";
  if (const char* why = jitter_ranges_error(*j)) return why;
  if (const char* why = frame_pair_frames_error(j)) return why;
  const bool work = with_work && jitter_needs_work(*j);
  if (work && !j->work) return "work is NULL where a record may hold a contrast";
  RangeSet<7> r;
  frame_pair_ranges(r, j, n, width, height, true);
  if (work) r.add(j->work, (unsigned long long)n * sizeof(DevJitterWork), true);
  return r.overlap("a written range overlaps another range of the job");
}

// ---- Camera (ofdg_camera, include/ofdg.h) ----------------------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job as the kernel takes it, the record's draw and its
// sanitising, the tap table, the roundings of the two blur passes, the mosaic's sites, the demosaic's means and the argument
// rules.  The taps are fp64 +, -, * through ofdg_det_exp (no contraction in any unit that includes this) and one rint;
// everything else is integers.
constexpr int kCameraMaxSigma = OFDG_CAMERA_MAX_SIGMA_Q8, kCameraMaxRadius = OFDG_CAMERA_MAX_RADIUS;
struct DevCameraRec {  // ofdg_camera_rec, field for field
  int32_t sigma_q8[2], bayer, radius[2], reserved[3];
};
struct DevCameraJob {  // struct ofdg_camera_job, field for field
  const void* src[2];
  void* dst[2];
  const DevCameraRec* recs;
  DevCameraRec* recs_out;
  long long first_index;
  uint32_t seed;
  int32_t width, height, src_fmt, dst_fmt, flags, pattern;
  float sigma_min, sigma_max, sigma_delta, blur_prob, bayer_prob;
  int32_t reserved;
};
static_assert(sizeof(ofdg_camera_rec) == sizeof(DevCameraRec) && sizeof(DevCameraRec) == 32 && offsetof(ofdg_camera_rec, bayer) == offsetof(DevCameraRec, bayer) &&
              offsetof(DevCameraRec, bayer) == 8 && offsetof(ofdg_camera_rec, radius) == offsetof(DevCameraRec, radius) && offsetof(DevCameraRec, radius) == 12 &&
              offsetof(ofdg_camera_rec, reserved) == offsetof(DevCameraRec, reserved) && offsetof(DevCameraRec, reserved) == 20,
              "ofdg_camera_rec: 32 bytes, the layout the kernel reads and writes as two 16-byte pieces");
static_assert(sizeof(struct ofdg_camera_job) == sizeof(DevCameraJob) && sizeof(DevCameraJob) == 112 && offsetof(struct ofdg_camera_job, dst) == offsetof(DevCameraJob, dst) &&
              offsetof(struct ofdg_camera_job, recs) == offsetof(DevCameraJob, recs) && offsetof(struct ofdg_camera_job, recs_out) == offsetof(DevCameraJob, recs_out) &&
              offsetof(struct ofdg_camera_job, first_index) == offsetof(DevCameraJob, first_index) && offsetof(struct ofdg_camera_job, seed) == offsetof(DevCameraJob, seed) &&
              offsetof(DevCameraJob, seed) == 56 && offsetof(struct ofdg_camera_job, width) == offsetof(DevCameraJob, width) &&
              offsetof(struct ofdg_camera_job, src_fmt) == offsetof(DevCameraJob, src_fmt) && offsetof(struct ofdg_camera_job, pattern) == offsetof(DevCameraJob, pattern) &&
              offsetof(DevCameraJob, pattern) == 80 && offsetof(struct ofdg_camera_job, sigma_min) == offsetof(DevCameraJob, sigma_min) && offsetof(DevCameraJob, sigma_min) == 84 &&
              offsetof(struct ofdg_camera_job, bayer_prob) == offsetof(DevCameraJob, bayer_prob) && offsetof(struct ofdg_camera_job, reserved) == offsetof(DevCameraJob, reserved) &&
              offsetof(DevCameraJob, reserved) == 104,
              "struct ofdg_camera_job: 112 bytes, the layout the kernel takes");
OFDG_HD_FN int32_t camera_q8(float px) { return (int32_t)lrintf(px * 256.0f); }
// The record of global sample g: Philox blocks 0 and 1 under the sampler's key of g at the counters {j, 0, 0x0c79, 0}.  `j`
// supplies the five ranges and the pattern (camera_ranges_error has passed).  Not sanitised.
OFDG_HD_FN DevCameraRec camera_draw_rec(uint32_t seed, unsigned long long g, const DevCameraJob& j) {
  const uint32_t k0 = seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
  const CropWords a = crop_philox(CropWords{0u, 0u, 0x0c79u, 0u}, k0, k1);
  const CropWords b = crop_philox(CropWords{1u, 0u, 0x0c79u, 0u}, k0, k1);
  const int32_t lo = camera_q8(j.sigma_min), hi = camera_q8(j.sigma_max), D = camera_q8(j.sigma_delta);
  const bool blurred = photo_unit(a.x) < j.blur_prob, mosaic = photo_unit(a.w) < j.bayer_prob;
  const int32_t s0 = lo + (int32_t)(uint32_t)(((unsigned long long)a.y * (uint32_t)(hi - lo + 1)) >> 32);
  const int32_t s1 = s0 + jitter_isym(a.z, D);
  const int32_t p = j.pattern >= 0 ? j.pattern : (int32_t)(b.x >> 30);
  DevCameraRec r;
  r.sigma_q8[0] = blurred ? s0 : 0; r.sigma_q8[1] = blurred ? s1 : 0;
  r.bayer = mosaic ? p : -1;
  r.radius[0] = 0; r.radius[1] = 0;
  r.reserved[0] = 0; r.reserved[1] = 0; r.reserved[2] = 0;
  return r;
}
OFDG_HD_FN int32_t camera_radius(int32_t s) {
  const int32_t R = (3 * s + 255) >> 8;
  return R < kCameraMaxRadius ? R : kCameraMaxRadius;
}
// What is used of a record, given or drawn.  No record makes the kernel touch a byte outside a plane or its tile's window.
OFDG_HD_FN DevCameraRec camera_sanitise(DevCameraRec r) {
  for (int f = 0; f < 2; ++f) {
    r.sigma_q8[f] = jitter_clamp(r.sigma_q8[f], 0, kCameraMaxSigma);
    r.radius[f] = camera_radius(r.sigma_q8[f]);
  }
  r.bayer = (r.bayer < -1 || r.bayer > 3) ? -1 : r.bayer;
  r.reserved[0] = 0; r.reserved[1] = 0; r.reserved[2] = 0;
  return r;
}
// e[k] of the tap table: the Gaussian at distance k in 8.24, for s in 1..1024 and k in 0..12
OFDG_HD_FN uint32_t camera_tap_e(int s, int k) {
  const double x = -(double)(k * k) * 32768.0 / (double)(s * s);
  return (uint32_t)(long long)rint(ofdg_det_exp(x) * 16777216.0);
}
// w[k], k >= 1: e[k] of the 65536 the taps sum to, to nearest (E < 2^29, e 65536 < 2^41)
OFDG_HD_FN uint32_t camera_tap_w(uint32_t e, uint32_t E) { return (uint32_t)(((unsigned long long)e * 65536ull + (unsigned long long)(E / 2u)) / (unsigned long long)E); }
// The table w[0..R] of sigma s (1..1024) and its radius R; entries above R are zeroed.
OFDG_HD_FN void camera_taps(int s, int R, uint32_t (&w)[kCameraMaxRadius + 1]) {
  uint32_t e[kCameraMaxRadius + 1], E = 0u, side = 0u;
  for (int k = 0; k <= kCameraMaxRadius; ++k) {
    e[k] = k <= R ? camera_tap_e(s, k) : 0u;
    E += k ? 2u * e[k] : e[k];
  }
  for (int k = 1; k <= kCameraMaxRadius; ++k) {
    w[k] = k <= R ? camera_tap_w(e[k], E) : 0u;
    side += w[k];
  }
  w[0] = 65536u - 2u * side;
}
// the roundings of the two passes: a row sum to h8 (at most 65280), a column sum of h8 to the byte
OFDG_HD_FN uint32_t camera_h8(uint32_t S) { return (S + 128u) >> 8; }
OFDG_HD_FN uint32_t camera_byte(uint32_t S) { return (S + (1u << 23)) >> 24; }
// edge replication, and reflection without repeating the edge (side >= 2; at is in [-1, side])
OFDG_HD_FN int camera_clamp(int at, int side) { return at < 0 ? 0 : at >= side ? side - 1 : at; }
OFDG_HD_FN int camera_reflect(int at, int side) { return at < 0 ? -at : at >= side ? 2 * side - 2 - at : at; }
// The channel (0 B, 1 G, 2 R: the plane order) the mosaic of pattern p samples at the site (a, b) of a pixel.
OFDG_HD_FN int camera_site_a(int x, int p) { return (x + (p & 1)) & 1; }
OFDG_HD_FN int camera_site_b(int y, int p) { return (y + (p >> 1)) & 1; }
OFDG_HD_FN int camera_site_channel(int a, int b) { return (a | b) == 0 ? 2 : (a & b) ? 0 : 1; }
// The demosaiced pixel from its own sample c, the sums of its two horizontal (sh), two vertical (sv) and four diagonal (sd)
// neighbours in the mosaic and its site: o[0..2] = B, G, R.
OFDG_HD_FN void camera_demosaic(int a, int b, uint32_t c, uint32_t sh, uint32_t sv, uint32_t sd, uint32_t (&o)[3]) {
  const uint32_t hz = (sh + 1u) >> 1, vt = (sv + 1u) >> 1, cr = (sh + sv + 2u) >> 2, dg = (sd + 2u) >> 2;
  if (a == b) {  // an R site (0, 0) or a B site (1, 1)
    o[a ? 0 : 2] = c; o[1] = cr; o[a ? 2 : 0] = dg;
  } else {       // a G site: on an R row (b = 0) R lies beside it and B above and below, on a B row the reverse
    o[1] = c; o[b ? 0 : 2] = hz; o[b ? 2 : 0] = vt;
  }
}
// The ranges of the draw and the pattern: the first rule broken, or nullptr.
inline const char* camera_ranges_error(const DevCameraJob& j) {
  if (!(j.sigma_min >= 0.0f && j.sigma_min <= 4.0f)) return "sigma_min must lie in [0, 4]";
  if (!(j.sigma_max >= 0.0f && j.sigma_max <= 4.0f)) return "sigma_max must lie in [0, 4]";
  if (j.sigma_min > j.sigma_max) return "sigma_min must not be above sigma_max";
  if (!(j.sigma_delta >= 0.0f && j.sigma_delta <= 4.0f)) return "sigma_delta must lie in [0, 4]";
  if (!(j.blur_prob >= 0.0f && j.blur_prob <= 1.0f)) return "blur_prob must lie in [0, 1]";
  if (!(j.bayer_prob >= 0.0f && j.bayer_prob <= 1.0f)) return "bayer_prob must lie in [0, 1]";
  if (j.pattern < -1 || j.pattern > 3) return "pattern must lie in -1..3";
  return nullptr;
}
// The argument rules ofdg_camera and ofdg_host_camera share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment is asked by the device entry only.
inline const char* camera_arg_error(const DevCameraJob* j, int n, int width, int height) {
  if (const char* why = frame_pair_fmt_error(j, n, width, height)) return why;
  if (j->flags != 0) return "flags must be 0";
  if (j->reserved != 0) return "reserved must be 0";
  if (const char* why = camera_ranges_error(*j)) return why;
  if (const char* why = frame_pair_frames_error(j)) return why;
  RangeSet<6> r;
  frame_pair_ranges(r, j, n, width, height, false);  // no in-place form: a pixel reads its neighbours
  return r.overlap("a written range overlaps another range of the job");
}

// ---- Lens (ofdg_lens, include/ofdg.h) --------------------------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job as the kernel takes it, the record's draw and its
// sanitising, the per-sample set-up, the forward map, the 8-step inverse with its verdict, the vignette and the argument
// rules.  The taps, the blend and the stores are the spatial augmentation's above.  Compiled without contraction, so every
// operation below is its own rounding.
struct DevLensRec {  // ofdg_lens_rec, field for field
  double k1, z, ca_b, ca_r, vig, cx, cy;
  int32_t reserved[2];
};
struct DevLensJob {  // struct ofdg_lens_job, field for field
  const void* src[kCropPlanes];
  void* dst[kCropPlanes];
  const DevLensRec* recs;
  DevLensRec* recs_out;
  long long first_index;
  uint32_t seed;
  int32_t width, height, flags, image_fmt, flow_fmt, occ_fmt, reserved;
  float prob, k1_range, ca_range, vig_max, centre;
};
static_assert(sizeof(ofdg_lens_rec) == sizeof(DevLensRec) && sizeof(DevLensRec) == 64 && offsetof(ofdg_lens_rec, cy) == offsetof(DevLensRec, cy) &&
              offsetof(DevLensRec, cy) == 48 && offsetof(ofdg_lens_rec, reserved) == offsetof(DevLensRec, reserved) && offsetof(DevLensRec, reserved) == 56,
              "ofdg_lens_rec: 64 bytes without padding, the layout the kernel reads and writes");
static_assert(sizeof(struct ofdg_lens_job) == sizeof(DevLensJob) && sizeof(DevLensJob) == 208 && offsetof(struct ofdg_lens_job, dst) == offsetof(DevLensJob, dst) &&
              offsetof(struct ofdg_lens_job, recs) == offsetof(DevLensJob, recs) && offsetof(struct ofdg_lens_job, recs_out) == offsetof(DevLensJob, recs_out) &&
              offsetof(struct ofdg_lens_job, first_index) == offsetof(DevLensJob, first_index) && offsetof(struct ofdg_lens_job, seed) == offsetof(DevLensJob, seed) &&
              offsetof(struct ofdg_lens_job, width) == offsetof(DevLensJob, width) && offsetof(struct ofdg_lens_job, flags) == offsetof(DevLensJob, flags) &&
              offsetof(struct ofdg_lens_job, occ_fmt) == offsetof(DevLensJob, occ_fmt) && offsetof(struct ofdg_lens_job, reserved) == offsetof(DevLensJob, reserved) &&
              offsetof(DevLensJob, reserved) == 180 && offsetof(struct ofdg_lens_job, prob) == offsetof(DevLensJob, prob) &&
              offsetof(struct ofdg_lens_job, centre) == offsetof(DevLensJob, centre) && offsetof(DevLensJob, centre) == 200,
              "struct ofdg_lens_job: 208 bytes, the layout the kernel takes");
static_assert(OFDG_LENS_FILL == 1 && OFDG_LENS_OCC_WINDOW == 16, "lens_draw_rec and lens_kernel spell these codes out");
OFDG_HD_FN DevLensRec lens_identity(int W, int H) {
  DevLensRec r;
  r.k1 = 0.0; r.z = 1.0; r.ca_b = 0.0; r.ca_r = 0.0; r.vig = 0.0;
  r.cx = (double)(W - 1) / 2.0; r.cy = (double)(H - 1) / 2.0;
  r.reserved[0] = 0; r.reserved[1] = 0;
  return r;
}
// one over the squared half-diagonal of a W x H plane
OFDG_HD_FN double lens_inv_diag2(int W, int H) {
  const double hw = (double)(W - 1) / 2.0, hh = (double)(H - 1) / 2.0;
  const double a = hw * hw, b = hh * hh;
  const double s = a + b;
  return 1.0 / s;
}
// rho of an offset (dx, dy) from the centre: the squared radius over the squared half-diagonal
OFDG_HD_FN double lens_rho(double dx, double dy, double inv) {
  const double a = dx * dx, b = dy * dy;
  const double s = a + b;
  return s * inv;
}
OFDG_HD_FN double lens_L(double k1, double rho) {
  const double t = k1 * rho;
  return 1.0 + t;
}
// one coordinate of the source position under magnification m: c + (m * L) * d
OFDG_HD_FN double lens_coord(double c, double m, double L, double d) {
  const double ml = m * L;
  const double t = ml * d;
  return c + t;
}
// The record of global sample g for a W x H plane: Philox blocks 0, 1 under the sampler's key of g at the counters {j, 0, 0x0c7a,
// 0}.  `j` supplies the five ranges and the flags.  Not sanitised.
OFDG_HD_FN DevLensRec lens_draw_rec(uint32_t seed, unsigned long long g, const DevLensJob& j, int W, int H) {
  const uint32_t k0 = seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
  const CropWords w0 = crop_philox(CropWords{0u, 0u, 0x0c7au, 0u}, k0, k1);
  const CropWords w1 = crop_philox(CropWords{1u, 0u, 0x0c7au, 0u}, k0, k1);
  DevLensRec r = lens_identity(W, H);
  if (!(photo_unit(w0.x) < j.prob)) return r;
  const float fk = photo_sym(w0.y, j.k1_range), fb = photo_sym(w0.z, j.ca_range), fr = photo_sym(w0.w, j.ca_range);
  const float fv = photo_unit(w1.x) * j.vig_max;
  const float ox = photo_sym(w1.y, j.centre), oy = photo_sym(w1.z, j.centre);
  const double hw = r.cx, hh = r.cy;
  r.k1 = (double)fk; r.ca_b = (double)fb; r.ca_r = (double)fr; r.vig = (double)fv;
  const double sx = (double)ox * hw, sy = (double)oy * hh;
  r.cx = hw + sx; r.cy = hh + sy;
  if (j.flags & 1) {  // OFDG_LENS_FILL: the farthest corner's L, when above 1, is undone
    const double inv = lens_inv_diag2(W, H);
    const double x0 = 0.0 - r.cx, x1 = (double)(W - 1) - r.cx, y0 = 0.0 - r.cy, y1 = (double)(H - 1) - r.cy;
    double rc = lens_rho(x0, y0, inv);
    const double r1 = lens_rho(x1, y0, inv), r2 = lens_rho(x0, y1, inv), r3 = lens_rho(x1, y1, inv);
    rc = r1 > rc ? r1 : rc; rc = r2 > rc ? r2 : rc; rc = r3 > rc ? r3 : rc;
    const double Lc = lens_L(r.k1, rc);
    r.z = Lc > 1.0 ? 1.0 / Lc : 1.0;
  }
  return r;
}
// What is used of a record, given or drawn: one that is not finite or out of its bounds becomes the identity.  (A comparison
// with a NaN fails, so a NaN fails its bound; every entry has one.)
OFDG_HD_FN DevLensRec lens_sanitise(DevLensRec r, int W, int H) {
  const double hw = (double)(W - 1) / 2.0, hh = (double)(H - 1) / 2.0;
  bool ok = spatial_abs(r.k1) <= 0.125 && r.z >= 0.5 && r.z <= 2.0 && spatial_abs(r.ca_b) <= 0.015625 && spatial_abs(r.ca_r) <= 0.015625;
  ok = ok && r.vig >= 0.0 && r.vig <= 0.5 && spatial_abs(r.cx - hw) <= hw / 4.0 && spatial_abs(r.cy - hh) <= hh / 4.0;
  if (!ok) return lens_identity(W, H);
  r.reserved[0] = 0; r.reserved[1] = 0;
  return r;
}
// What a sample's pixels share, made once from its sanitised record
struct LensSetup {
  double k1, k3, z, iz, zb, zr, vig, cx, cy, inv;  // k3 = 3 k1, iz = 1 / z, zb / zr: the magnification of B / R (G's is z)
};
OFDG_HD_FN LensSetup lens_setup(const DevLensRec& r, int W, int H) {
  LensSetup s;
  s.k1 = r.k1; s.k3 = 3.0 * r.k1; s.z = r.z; s.iz = 1.0 / r.z;
  const double b = 1.0 + r.ca_b, c = 1.0 + r.ca_r;
  s.zb = r.z * b; s.zr = r.z * c;
  s.vig = r.vig; s.cx = r.cx; s.cy = r.cy;
  s.inv = lens_inv_diag2(W, H);
  return s;
}
OFDG_HD_FN double lens_channel_z(const LensSetup& s, int c) { return c == 0 ? s.zb : c == 2 ? s.zr : s.z; }
// the vignette of a destination pixel
OFDG_HD_FN float lens_gain(double vig, double rho) {
  const double t = vig * rho;
  return (float)(1.0 - t);
}
// a, g and the bracket of the derivative at s: g = z s (1 + k1 a) - 1 with a = ru s^2, D = 1 + 3 k1 a
OFDG_HD_FN void lens_residual(const LensSetup& o, double ru, double s, double* g, double* D) {
  const double rs = ru * s;
  const double a = rs * s;
  const double zs = o.z * s;
  const double ka = o.k1 * a;
  const double b = 1.0 + ka;
  const double p = zs * b;
  *g = p - 1.0;
  const double k3a = o.k3 * a;
  *D = 1.0 + k3a;
}
// P with S(P) = (tx, ty): eight Newton steps for s in P = c + s (t - c), then the verdict.  false: unsolvable.
OFDG_HD_FN bool lens_inverse(const LensSetup& o, double tx, double ty, double* px, double* py) {
  const double dtx = tx - o.cx, dty = ty - o.cy;
  double s = o.iz;
  bool solved = true;
  if (o.k1 != 0.0) {
    const double ru = lens_rho(dtx, dty, o.inv);
    if (!(ru <= 16.0)) return false;
    double g, D;
    for (int k = 0; k < 8; ++k) {
      lens_residual(o, ru, s, &g, &D);
      const double d = o.z * D;
      const double q = g / d;
      s = s - q;
    }
    lens_residual(o, ru, s, &g, &D);
    solved = spatial_abs(g) <= 9.31322574615478515625e-10 && D >= 0.25 && s > 0.0;
  }
  const double ax = s * dtx, ay = s * dty;
  *px = o.cx + ax;
  *py = o.cy + ay;
  return solved;
}
OFDG_HD_FN float lens_nan() {  // 0x7FC00000: what an unsolvable pixel's flow holds
  const uint32_t bits = 0x7FC00000u;
  float nan;
  memcpy(&nan, &bits, 4);
  return nan;
}
// The plane size of a job: its own when set, else the one offered (the context's frame, the host twin's arguments).
inline const char* lens_plane_size(const DevLensJob& j, int* width, int* height) {
  if (const char* why = job_plane_size(j, width, height)) return why;
  if (*width > kSpatialMaxSide || *height > kSpatialMaxSide) return "width and height must not exceed 2^20";
  if ((unsigned long long)*width * (unsigned long long)*height >= (1ull << 31)) return "width * height must be below 2^31";
  return nullptr;
}
// What the draw reads of a job besides the size: the flags and the five ranges.
inline const char* lens_draw_error(const DevLensJob& j) {
  if (j.flags & ~(OFDG_LENS_FILL | OFDG_LENS_OCC_WINDOW)) return "flags holds unknown bits";
  if (!(j.prob >= 0.0f && j.prob <= 1.0f)) return "prob must lie in [0, 1]";
  if (!(j.k1_range >= 0.0f && j.k1_range <= 0.125f)) return "k1_range must lie in [0, 0.125]";
  if (!(j.ca_range >= 0.0f && j.ca_range <= 0.015625f)) return "ca_range must lie in [0, 1/64]";
  if (!(j.vig_max >= 0.0f && j.vig_max <= 0.5f)) return "vig_max must lie in [0, 0.5]";
  if (!(j.centre >= 0.0f && j.centre <= 0.25f)) return "centre must lie in [0, 0.25]";
  return nullptr;
}
// The argument rules ofdg_lens and ofdg_host_lens share: the first rule broken, or nullptr.  width, height: what
// lens_plane_size gave.  Alignment is asked by the device entry only.
inline const char* lens_arg_error(const DevLensJob* j, int n, int width, int height) {
  if (!j) return "job is NULL";
  if (n < 1) return "n_samples must be at least 1";
  if (const char* why = lens_draw_error(*j)) return why;
  if (j->reserved != 0) return "reserved must be 0";
  if (j->image_fmt != OFDG_FMT_F32 && j->image_fmt != OFDG_FMT_U8) return "image_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (const char* why = flow_occ_fmt_error(j->flow_fmt, true, j->occ_fmt)) return why;
  int planes = 0;
  for (int k = 0; k < kCropPlanes; ++k) {
    if (j->src[k] && !j->dst[k]) return "dst: a plane has a source and no destination";
    if (!j->src[k] && j->dst[k]) return "src: a plane has a destination and no source";
    planes += j->src[k] ? 1 : 0;
  }
  if (!planes) return "src: no plane is set";
  if ((j->flags & OFDG_LENS_OCC_WINDOW) && j->src[OFDG_CROP_OCC0] && !j->src[OFDG_CROP_FLOW]) return "flags: OFDG_LENS_OCC_WINDOW with occ0 needs flow";
  if ((j->flags & OFDG_LENS_OCC_WINDOW) && j->src[OFDG_CROP_OCC1] && !j->src[OFDG_CROP_FLOW1]) return "flags: OFDG_LENS_OCC_WINDOW with occ1 needs flow1";
  // no in-place form: a destination range may meet no other range of the job
  RangeSet<2 * kCropPlanes + 2> r;
  for (int k = 0; k < kCropPlanes; ++k) {
    if (!j->src[k]) continue;
    const int es = fmt_elem_bytes(k < 2 ? j->image_fmt : k < 4 ? j->flow_fmt : k < 6 ? j->occ_fmt : OFDG_FMT_U8);
    const unsigned long long bytes = (unsigned long long)n * crop_channels(k) * es * width * height;
    r.add(j->src[k], bytes, false);
    r.add(j->dst[k], bytes, true);
  }
  r.add_if(j->recs, (unsigned long long)n * sizeof(DevLensRec), false);
  r.add_if(j->recs_out, (unsigned long long)n * sizeof(DevLensRec), true);
  return r.overlap("dst: a destination range overlaps another range of the job");
}

// ---- Block compression (ofdg_jpeg, include/ofdg.h) -------------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job as the kernel takes it, the record's draw and its
// sanitising, the quantisation tables, the colour transforms, the transform table, the roundings of the four passes, the
// quantiser and the argument rules.  Everything is 32-bit integers; >> on a negative value is arithmetic.
struct DevJpegRec {  // ofdg_jpeg_rec, field for field
  int32_t quality[2], subsample, phase_x, phase_y, reserved[3];
};
struct DevJpegJob {  // struct ofdg_jpeg_job, field for field
  const void* src[2];
  void* dst[2];
  const DevJpegRec* recs;
  DevJpegRec* recs_out;
  long long first_index;
  uint32_t seed;
  int32_t width, height, src_fmt, dst_fmt, flags, subsample, quality_min, quality_max, quality_delta;
  float prob, sub_prob;
  int32_t reserved[2];
};
static_assert(sizeof(ofdg_jpeg_rec) == sizeof(DevJpegRec) && sizeof(DevJpegRec) == 32 && offsetof(ofdg_jpeg_rec, subsample) == offsetof(DevJpegRec, subsample) &&
              offsetof(DevJpegRec, subsample) == 8 && offsetof(ofdg_jpeg_rec, phase_x) == offsetof(DevJpegRec, phase_x) && offsetof(DevJpegRec, phase_x) == 12 &&
              offsetof(ofdg_jpeg_rec, phase_y) == offsetof(DevJpegRec, phase_y) && offsetof(ofdg_jpeg_rec, reserved) == offsetof(DevJpegRec, reserved) &&
              offsetof(DevJpegRec, reserved) == 20 && OFDG_JPEG_PHASE == 1,
              "ofdg_jpeg_rec: 32 bytes, the layout the kernel reads and writes as two 16-byte pieces");
static_assert(sizeof(struct ofdg_jpeg_job) == sizeof(DevJpegJob) && sizeof(DevJpegJob) == 112 && offsetof(struct ofdg_jpeg_job, dst) == offsetof(DevJpegJob, dst) &&
              offsetof(struct ofdg_jpeg_job, recs) == offsetof(DevJpegJob, recs) && offsetof(struct ofdg_jpeg_job, recs_out) == offsetof(DevJpegJob, recs_out) &&
              offsetof(struct ofdg_jpeg_job, first_index) == offsetof(DevJpegJob, first_index) && offsetof(struct ofdg_jpeg_job, seed) == offsetof(DevJpegJob, seed) &&
              offsetof(DevJpegJob, seed) == 56 && offsetof(struct ofdg_jpeg_job, width) == offsetof(DevJpegJob, width) &&
              offsetof(struct ofdg_jpeg_job, src_fmt) == offsetof(DevJpegJob, src_fmt) && offsetof(struct ofdg_jpeg_job, flags) == offsetof(DevJpegJob, flags) &&
              offsetof(struct ofdg_jpeg_job, subsample) == offsetof(DevJpegJob, subsample) && offsetof(DevJpegJob, subsample) == 80 &&
              offsetof(struct ofdg_jpeg_job, quality_min) == offsetof(DevJpegJob, quality_min) && offsetof(struct ofdg_jpeg_job, quality_delta) == offsetof(DevJpegJob, quality_delta) &&
              offsetof(DevJpegJob, quality_delta) == 92 && offsetof(struct ofdg_jpeg_job, prob) == offsetof(DevJpegJob, prob) &&
              offsetof(struct ofdg_jpeg_job, sub_prob) == offsetof(DevJpegJob, sub_prob) && offsetof(struct ofdg_jpeg_job, reserved) == offsetof(DevJpegJob, reserved) &&
              offsetof(DevJpegJob, reserved) == 104,
              "struct ofdg_jpeg_job: 112 bytes, the layout the kernel takes");
// T.81 Annex K, Table K.1 (luminance) and Table K.2 (chrominance), row-major [v][u]
constexpr uint8_t kJpegBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                       14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kJpegBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// T[u][x] = lrint(4096 s(u) cos((2 x + 1) u pi / 16)), s(0) = 1 / sqrt 2, else 1: 8192 times the orthonormal DCT-II matrix
constexpr int32_t kJpegT[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,  4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,
                                3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,  3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,
                                2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,  2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,
                                1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,  799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};
// The record of global sample g: Philox blocks 0 and 1 under the sampler's key of g at the counters {j, 0, 0x0c7b, 0}.  `j`
// supplies the ranges, subsample and flags (jpeg_ranges_error has passed).  Not sanitised.
OFDG_HD_FN DevJpegRec jpeg_draw_rec(uint32_t seed, unsigned long long g, const DevJpegJob& j) {
  const uint32_t k0 = seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
  const CropWords a = crop_philox(CropWords{0u, 0u, 0x0c7bu, 0u}, k0, k1);
  const CropWords b = crop_philox(CropWords{1u, 0u, 0x0c7bu, 0u}, k0, k1);
  const bool on = photo_unit(a.x) < j.prob;
  const int32_t q0 = j.quality_min + (int32_t)(uint32_t)(((unsigned long long)a.y * (uint32_t)(j.quality_max - j.quality_min + 1)) >> 32);
  const int32_t q1 = jitter_clamp(q0 + jitter_isym(a.z, j.quality_delta), 1, 100);
  const bool phase = (j.flags & OFDG_JPEG_PHASE) != 0;
  DevJpegRec r;
  r.quality[0] = on ? q0 : 0; r.quality[1] = on ? q1 : 0;
  r.subsample = j.subsample >= 0 ? j.subsample : (photo_unit(a.w) < j.sub_prob ? 1 : 0);
  r.phase_x = phase ? (int32_t)(b.x >> 28) : 0; r.phase_y = phase ? (int32_t)(b.y >> 28) : 0;
  r.reserved[0] = 0; r.reserved[1] = 0; r.reserved[2] = 0;
  return r;
}
// What is used of a record, given or drawn.  No record makes the kernel touch a byte outside a plane.
OFDG_HD_FN DevJpegRec jpeg_sanitise(DevJpegRec r) {
  r.quality[0] = jitter_clamp(r.quality[0], 0, 100); r.quality[1] = jitter_clamp(r.quality[1], 0, 100);
  r.subsample = r.subsample == 1 ? 1 : 0;
  r.phase_x = (r.phase_x < 0 || r.phase_x > 15) ? 0 : r.phase_x;
  r.phase_y = (r.phase_y < 0 || r.phase_y > 15) ? 0 : r.phase_y;
  r.reserved[0] = 0; r.reserved[1] = 0; r.reserved[2] = 0;
  return r;
}
// the side of an MCU and the phase that counts: 4:4:4 uses phase & 7
OFDG_HD_FN int jpeg_mcu(int subsample) { return subsample ? 16 : 8; }
OFDG_HD_FN int jpeg_phase(int phase, int subsample) { return subsample ? phase : phase & 7; }
// libjpeg's table entry of a quality in 1..100
OFDG_HD_FN uint32_t jpeg_quant(uint32_t base, int quality) {
  const uint32_t scale = quality < 50 ? 5000u / (uint32_t)quality : 200u - 2u * (uint32_t)quality;
  const uint32_t q = (base * scale + 50u) / 100u;
  return q < 1u ? 1u : q > 255u ? 255u : q;
}
// libjpeg's 16-bit colour constants, there and back; the results of the first three are bytes by construction
OFDG_HD_FN int32_t jpeg_luma(int32_t r, int32_t g, int32_t b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
OFDG_HD_FN int32_t jpeg_cb(int32_t r, int32_t g, int32_t b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
OFDG_HD_FN int32_t jpeg_cr(int32_t r, int32_t g, int32_t b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }
OFDG_HD_FN int32_t jpeg_byte(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
OFDG_HD_FN int32_t jpeg_red(int32_t y, int32_t cr) { return jpeg_byte(y + ((91881 * (cr - 128) + 32768) >> 16)); }
OFDG_HD_FN int32_t jpeg_green(int32_t y, int32_t cb, int32_t cr) { return jpeg_byte(y + ((-22554 * (cb - 128) - 46802 * (cr - 128) + 32768) >> 16)); }
OFDG_HD_FN int32_t jpeg_blue(int32_t y, int32_t cb) { return jpeg_byte(y + ((116130 * (cb - 128) + 32768) >> 16)); }
// the mean of the four samples of a chroma cell
OFDG_HD_FN int32_t jpeg_cell(int32_t s4) { return (s4 + 2) >> 2; }
// the roundings: behind a first pass (forward and inverse), the quantiser and what it hands on, the byte behind the last pass
OFDG_HD_FN int32_t jpeg_round9(int32_t a) { return (a + 256) >> 9; }
OFDG_HD_FN int32_t jpeg_level(int32_t F, uint32_t Q) {
  const uint32_t m = ((uint32_t)(F < 0 ? -F : F) + Q * 65536u) / (Q * 131072u);
  return F < 0 ? -(int32_t)m : (int32_t)m;
}
OFDG_HD_FN int32_t jpeg_sample(int32_t P) { return jpeg_byte(((P + 65536) >> 17) + 128); }
// Steps 4-6 of one block the plain way (the host twin's; the kernel runs the same passes a lane an element): in, q, levels and
// out are row-major [8][8].
inline void jpeg_block(const uint8_t* in, const uint16_t* q, int32_t* levels, uint8_t* out) {
  int32_t a[64], d[64];
  for (int y = 0; y < 8; ++y)
    for (int u = 0; u < 8; ++u) {
      int32_t s = 0;
      for (int x = 0; x < 8; ++x) s += kJpegT[u * 8 + x] * ((int32_t)in[y * 8 + x] - 128);
      a[y * 8 + u] = jpeg_round9(s);
    }
  for (int v = 0; v < 8; ++v)
    for (int u = 0; u < 8; ++u) {
      int32_t s = 0;
      for (int y = 0; y < 8; ++y) s += kJpegT[v * 8 + y] * a[y * 8 + u];
      const int32_t level = jpeg_level(s, q[v * 8 + u]);
      if (levels) levels[v * 8 + u] = level;
      d[v * 8 + u] = level * (int32_t)q[v * 8 + u];
    }
  for (int y = 0; y < 8; ++y)
    for (int u = 0; u < 8; ++u) {
      int32_t s = 0;
      for (int v = 0; v < 8; ++v) s += kJpegT[v * 8 + y] * d[v * 8 + u];
      a[y * 8 + u] = jpeg_round9(s);
    }
  for (int y = 0; y < 8; ++y)
    for (int x = 0; x < 8; ++x) {
      int32_t s = 0;
      for (int u = 0; u < 8; ++u) s += kJpegT[u * 8 + x] * a[y * 8 + u];
      out[y * 8 + x] = (uint8_t)jpeg_sample(s);
    }
}
// The ranges of the draw, subsample and flags: the first rule broken, or nullptr.
inline const char* jpeg_ranges_error(const DevJpegJob& j) {
  if (j.flags != 0 && j.flags != OFDG_JPEG_PHASE) return "flags must be 0 or OFDG_JPEG_PHASE";
  if (j.quality_min < 1 || j.quality_min > 100) return "quality_min must lie in 1..100";
  if (j.quality_max < 1 || j.quality_max > 100) return "quality_max must lie in 1..100";
  if (j.quality_min > j.quality_max) return "quality_min must not be above quality_max";
  if (j.quality_delta < 0 || j.quality_delta > 99) return "quality_delta must lie in 0..99";
  if (!(j.prob >= 0.0f && j.prob <= 1.0f)) return "prob must lie in [0, 1]";
  if (!(j.sub_prob >= 0.0f && j.sub_prob <= 1.0f)) return "sub_prob must lie in [0, 1]";
  if (j.subsample < -1 || j.subsample > 1) return "subsample must lie in -1..1";
  return nullptr;
}
// The argument rules ofdg_jpeg and ofdg_host_jpeg share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment is asked by the device entry only.
inline const char* jpeg_arg_error(const DevJpegJob* j, int n, int width, int height) {
  if (const char* why = frame_pair_fmt_error(j, n, width, height)) return why;
  if (j->reserved[0] != 0 || j->reserved[1] != 0) return "reserved must be 0";
  if (const char* why = jpeg_ranges_error(*j)) return why;
  if (const char* why = frame_pair_frames_error(j)) return why;
  RangeSet<6> r;
  frame_pair_ranges(r, j, n, width, height, true);
  return r.overlap("a written range overlaps another range of the job");
}

// ---- Motion blur (ofdg_motion_blur, include/ofdg.h) ------------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job as the kernel takes it, the record's draw and its
// sanitising, the half-displacement, the tap count and step, the tap value, the mean and the argument rules.  Compiled
// without contraction, so every float operation below is its own rounding; behind the half-displacement and the step
// everything is integers.
constexpr int kMblurMaxTapsSide = OFDG_MBLUR_MAX_TAPS_SIDE;
static_assert(256 * OFDG_MBLUR_MAX_HALF_PX == 8192, "mblur_half spells the clamp out");
struct DevMblurRec {  // ofdg_mblur_rec, field for field
  float shutter[2];
  int32_t reserved[2];
};
struct DevMblurJob {  // struct ofdg_mblur_job, field for field
  const void* src[2];
  void* dst[2];
  const void* flow[2];
  const DevMblurRec* recs;
  DevMblurRec* recs_out;
  long long first_index;
  uint32_t seed;
  int32_t width, height, src_fmt, dst_fmt, flow_fmt, flags, taps_side;
  float prob, shutter_min, shutter_max, pair_shutter;
  int32_t reserved[2];
};
static_assert(sizeof(ofdg_mblur_rec) == sizeof(DevMblurRec) && sizeof(DevMblurRec) == 16 && offsetof(ofdg_mblur_rec, reserved) == offsetof(DevMblurRec, reserved) &&
              offsetof(DevMblurRec, reserved) == 8, "ofdg_mblur_rec: 16 bytes without padding, the layout the kernel reads and writes");
static_assert(sizeof(struct ofdg_mblur_job) == sizeof(DevMblurJob) && sizeof(DevMblurJob) == 128 && offsetof(struct ofdg_mblur_job, dst) == offsetof(DevMblurJob, dst) &&
              offsetof(struct ofdg_mblur_job, flow) == offsetof(DevMblurJob, flow) && offsetof(struct ofdg_mblur_job, recs) == offsetof(DevMblurJob, recs) &&
              offsetof(struct ofdg_mblur_job, recs_out) == offsetof(DevMblurJob, recs_out) && offsetof(struct ofdg_mblur_job, first_index) == offsetof(DevMblurJob, first_index) &&
              offsetof(struct ofdg_mblur_job, seed) == offsetof(DevMblurJob, seed) && offsetof(struct ofdg_mblur_job, width) == offsetof(DevMblurJob, width) &&
              offsetof(struct ofdg_mblur_job, src_fmt) == offsetof(DevMblurJob, src_fmt) && offsetof(struct ofdg_mblur_job, taps_side) == offsetof(DevMblurJob, taps_side) &&
              offsetof(DevMblurJob, taps_side) == 100 && offsetof(struct ofdg_mblur_job, prob) == offsetof(DevMblurJob, prob) &&
              offsetof(struct ofdg_mblur_job, pair_shutter) == offsetof(DevMblurJob, pair_shutter) && offsetof(DevMblurJob, pair_shutter) == 116 &&
              offsetof(struct ofdg_mblur_job, reserved) == offsetof(DevMblurJob, reserved), "struct ofdg_mblur_job: 128 bytes, the layout the kernel takes");
// The record of global sample g: Philox block 0 under the sampler's key of g at the counter {0, 0, 0x0c76, 0}.  `j` supplies
// prob and the three ranges.
OFDG_HD_FN DevMblurRec mblur_draw_rec(uint32_t seed, unsigned long long g, const DevMblurJob& j) {
  const CropWords w = crop_philox(CropWords{0u, 0u, 0x0c76u, 0u}, seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, (uint32_t)g);
  const bool on = photo_unit(w.x) < j.prob;
  const float span = j.shutter_max - j.shutter_min;
  const float part = span * photo_unit(w.y);
  const float s0 = j.shutter_min + part;
  const float s1 = s0 + photo_sym(w.z, j.pair_shutter);
  DevMblurRec r;
  r.shutter[0] = on ? s0 : 0.0f;
  r.shutter[1] = on ? s1 : 0.0f;
  r.reserved[0] = 0; r.reserved[1] = 0;
  return r;
}
// What is used of a record, given or drawn: a NaN, a negative value and -0.0 become +0, a value above 2 becomes 2.
OFDG_HD_FN float mblur_shutter(float s) { return s > 0.0f ? (s > OFDG_MBLUR_MAX_SHUTTER ? OFDG_MBLUR_MAX_SHUTTER : s) : 0.0f; }
OFDG_HD_FN DevMblurRec mblur_sanitise(DevMblurRec r) {
  for (int f = 0; f < 2; ++f) {
    r.shutter[f] = mblur_shutter(r.shutter[f]);
    r.reserved[f] = 0;
  }
  return r;
}
// finite: neither NaN nor an infinity (on the bits: no comparison the compiler may fold)
OFDG_HD_FN bool mblur_finite(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  return (b & 0x7f800000u) != 0x7f800000u;
}
// One component of the half-displacement in 24.8 for a finite flow component d and a sanitised shutter s: two float32
// products (an overflow to an infinity lands on the clamp), the clamp, ties to even.
OFDG_HD_FN int mblur_half(float d, float s) {
  const float a = d * s;
  float h = a * 128.0f;
  h = h < -8192.0f ? -8192.0f : h > 8192.0f ? 8192.0f : h;
  return (int)rintf(h);
}
OFDG_HD_FN int mblur_abs(int v) { return v < 0 ? -v : v; }
// taps on each side of the centre: one per pixel of half-extent on the major axis, up to the cap
OFDG_HD_FN int mblur_taps_side(int Dx, int Dy, int cap) {
  const int ax = mblur_abs(Dx), ay = mblur_abs(Dy), L = ax > ay ? ax : ay, m = (L + 255) >> 8;
  return m < cap ? m : cap;
}
// the step between taps on one axis, for m > 0: an IEEE float32 division, ties to even
OFDG_HD_FN int mblur_step(int D, int m) { return (int)rintf((float)D / (float)m); }
// a tap's coordinate on one axis, clamped into the plane: side is the width or the height
OFDG_HD_FN int mblur_coord(int at, int k, int step, int side) {
  const int q = 256 * at + k * step, hi = 256 * (side - 1);
  return q < 0 ? 0 : q > hi ? hi : q;
}
// the 24.8 bilinear tap of four bytes, the integer form of ofdg_spatial's: at most 65280
OFDG_HD_FN uint32_t mblur_tap(uint32_t e00, uint32_t e10, uint32_t e01, uint32_t e11, int fx, int fy) {
  const uint32_t ux = (uint32_t)fx, uy = (uint32_t)fy;
  const uint32_t T = (256u - ux) * (256u - uy) * e00 + ux * (256u - uy) * e10 + (256u - ux) * uy * e01 + ux * uy * e11;
  return (T + 128u) >> 8;
}
// the weight of tap k of N = 2 m + 1: 65536 / N, the centre takes what the division leaves
OFDG_HD_FN uint32_t mblur_weight(int k, int m) {
  const uint32_t w = 65536u / (uint32_t)(2 * m + 1);
  return k == 0 ? 65536u - 2u * (uint32_t)m * w : w;
}
// the byte of a weighted sum of taps (the weights sum to 65536, a tap is at most 65280: no overflow)
OFDG_HD_FN uint32_t mblur_byte(uint32_t S) { return (S + (1u << 23)) >> 24; }
// What the draw reads of a job: the first rule broken, or nullptr.
inline const char* mblur_ranges_error(const DevMblurJob& j) {
  if (!(j.prob >= 0.0f && j.prob <= 1.0f)) return "prob must lie in [0, 1]";
  if (!(j.shutter_min >= 0.0f && j.shutter_min <= OFDG_MBLUR_MAX_SHUTTER)) return "shutter_min must lie in [0, 2]";
  if (!(j.shutter_max >= 0.0f && j.shutter_max <= OFDG_MBLUR_MAX_SHUTTER)) return "shutter_max must lie in [0, 2]";
  if (j.shutter_min > j.shutter_max) return "shutter_min must not be above shutter_max";
  if (!(j.pair_shutter >= 0.0f && j.pair_shutter <= 3.4028234663852886e38f)) return "pair_shutter must be finite and not negative";
  return nullptr;
}
// The argument rules ofdg_motion_blur and ofdg_host_motion_blur share: the first rule broken, or nullptr.  width, height:
// what job_plane_size gave.  Alignment is asked by the device entry only.
inline const char* mblur_arg_error(const DevMblurJob* j, int n, int width, int height) {
  if (const char* why = frame_pair_fmt_error(j, n, width, height)) return why;  // (as far as the rules coincide: a frame here has a flow)
  if (j->flow_fmt != OFDG_FMT_F32 && j->flow_fmt != OFDG_FMT_F16) return "flow_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if (j->flags != 0) return "flags must be 0";
  if (j->reserved[0] != 0 || j->reserved[1] != 0) return "reserved must be 0";
  if (j->taps_side < 1 || j->taps_side > kMblurMaxTapsSide) return "taps_side must lie in 1..16";
  int frames = 0;
  for (int f = 0; f < 2; ++f) {
    const int set = (j->src[f] ? 1 : 0) + (j->dst[f] ? 1 : 0) + (j->flow[f] ? 1 : 0);
    if (set != 0 && set != 3) return !j->src[f] ? "src: a frame is incomplete (src, dst and flow go together)" : !j->dst[f] ? "dst: a frame is incomplete (src, dst and flow go together)"
                                                                                                                               : "flow: a frame is incomplete (src, dst and flow go together)";
    frames += set ? 1 : 0;
  }
  if (!frames) return "src: no frame is set";
  if (!j->recs)
    if (const char* why = mblur_ranges_error(*j)) return why;
  // no in-place form: a destination range may meet no other range of the job
  RangeSet<8> r;
  const unsigned long long plane = (unsigned long long)n * width * height;
  for (int f = 0; f < 2; ++f) {
    if (!j->src[f]) continue;
    r.add(j->src[f], plane * 3 * fmt_elem_bytes(j->src_fmt), false);
    r.add(j->dst[f], plane * 3 * fmt_elem_bytes(j->dst_fmt), true);
    r.add(j->flow[f], plane * 2 * fmt_elem_bytes(j->flow_fmt), false);
  }
  r.add_if(j->recs, (unsigned long long)n * sizeof(DevMblurRec), false);
  r.add_if(j->recs_out, (unsigned long long)n * sizeof(DevMblurRec), true);
  return r.overlap("dst: a destination range overlaps another range of the job");
}

// ---- Reprojection (ofdg_reproject, include/ofdg.h) -------------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job and the row as the kernel takes them, the 24.8
// displacement, the inside test, the warped byte, the backward displacement at the target, the residual and the argument
// rules.  The tap is mblur_tap, the finite test mblur_finite, the clamps spatial_clamp, the byte of a float32 photo_index.
// Behind the two float32 products everything is integers.
constexpr int kReprojErrBins = OFDG_REPROJ_ERR_BINS;
constexpr long long kReprojE2Sat = 1ll << 47;  // e2 of a non-finite backward tap: ex = ey = 2^23
struct DevReprojFrameRow {  // ofdg_reproject_frame_row, field for field: the kernel adds to the words with unsigned atomics
  uint32_t cnt[4];          // n_bad, n_outside, n_visible, n_hidden
  uint32_t err_hist[kReprojErrBins];
  uint32_t max_err_visible;
  uint32_t n_fb_over[2];    // visible, hidden
  uint32_t reserved;
  unsigned long long sum_err[2];  // visible, hidden
  unsigned long long sum_fb2_visible, max_fb2_visible;
};
struct DevReprojRow { DevReprojFrameRow frame[2]; };
struct DevReprojJob {  // struct ofdg_reproject_job, field for field
  const void* img[2];
  const void* flow[2];
  const void* occ[2];
  void* warped[2];
  void* err[2];
  void* mask[2];
  void* fb2[2];
  DevReprojRow* rows;
  int32_t width, height, img_fmt, dst_fmt, flow_fmt, occ_fmt, flags, fb_thresh_q8;
  int32_t reserved[2];
};
static_assert(sizeof(ofdg_reproject_frame_row) == sizeof(DevReprojFrameRow) && sizeof(DevReprojFrameRow) == 128 &&
              offsetof(ofdg_reproject_frame_row, n_bad) == offsetof(DevReprojFrameRow, cnt) && offsetof(ofdg_reproject_frame_row, err_hist) == offsetof(DevReprojFrameRow, err_hist) &&
              offsetof(ofdg_reproject_frame_row, max_err_visible) == offsetof(DevReprojFrameRow, max_err_visible) && offsetof(DevReprojFrameRow, max_err_visible) == 80 &&
              offsetof(ofdg_reproject_frame_row, n_fb_over_visible) == offsetof(DevReprojFrameRow, n_fb_over) &&
              offsetof(ofdg_reproject_frame_row, sum_err_visible) == offsetof(DevReprojFrameRow, sum_err) && offsetof(DevReprojFrameRow, sum_err) == 96 &&
              offsetof(ofdg_reproject_frame_row, sum_fb2_visible) == offsetof(DevReprojFrameRow, sum_fb2_visible) &&
              offsetof(ofdg_reproject_frame_row, max_fb2_visible) == offsetof(DevReprojFrameRow, max_fb2_visible) && offsetof(DevReprojFrameRow, max_fb2_visible) == 120,
              "ofdg_reproject_frame_row: 128 bytes without padding, the layout the kernel adds to");
static_assert(sizeof(ofdg_reproject_row) == sizeof(DevReprojRow) && sizeof(DevReprojRow) == 256 && offsetof(ofdg_reproject_row, frame) == 0,
              "ofdg_reproject_row: 256 bytes without padding, a block per frame");
static_assert(sizeof(struct ofdg_reproject_job) == sizeof(DevReprojJob) && sizeof(DevReprojJob) == 160 && offsetof(struct ofdg_reproject_job, flow) == offsetof(DevReprojJob, flow) &&
              offsetof(struct ofdg_reproject_job, occ) == offsetof(DevReprojJob, occ) && offsetof(struct ofdg_reproject_job, warped) == offsetof(DevReprojJob, warped) &&
              offsetof(struct ofdg_reproject_job, err) == offsetof(DevReprojJob, err) && offsetof(struct ofdg_reproject_job, mask) == offsetof(DevReprojJob, mask) &&
              offsetof(struct ofdg_reproject_job, fb2) == offsetof(DevReprojJob, fb2) && offsetof(struct ofdg_reproject_job, rows) == offsetof(DevReprojJob, rows) &&
              offsetof(DevReprojJob, rows) == 112 && offsetof(struct ofdg_reproject_job, width) == offsetof(DevReprojJob, width) &&
              offsetof(struct ofdg_reproject_job, img_fmt) == offsetof(DevReprojJob, img_fmt) && offsetof(struct ofdg_reproject_job, occ_fmt) == offsetof(DevReprojJob, occ_fmt) &&
              offsetof(struct ofdg_reproject_job, flags) == offsetof(DevReprojJob, flags) && offsetof(struct ofdg_reproject_job, fb_thresh_q8) == offsetof(DevReprojJob, fb_thresh_q8) &&
              offsetof(DevReprojJob, fb_thresh_q8) == 148 && offsetof(struct ofdg_reproject_job, reserved) == offsetof(DevReprojJob, reserved),
              "struct ofdg_reproject_job: 160 bytes, the layout the kernel takes");
// A finite displacement component in 24.8: one float32 product (an overflow to an infinity lands on the clamp), the clamp,
// ties to even.
OFDG_HD_FN int reproj_q8(float d) {
  float h = d * 256.0f;
  h = h < -1073741824.0f ? -1073741824.0f : h > 1073741824.0f ? 1073741824.0f : h;
  return (int)rintf(h);
}
// Is the rounded target of the 24.8 coordinate (Qx, Qy) a pixel of the plane?
OFDG_HD_FN bool reproj_inside(int Qx, int Qy, int W, int H) {
  const int rx = (Qx + 128) >> 8, ry = (Qy + 128) >> 8;
  return rx >= 0 && rx <= W - 1 && ry >= 0 && ry <= H - 1;
}
// a 24.8 coordinate clamped into the plane: side is the width or the height
OFDG_HD_FN int reproj_coord(int Q, int side) {
  const int hi = 256 * (side - 1);
  return Q < 0 ? 0 : Q > hi ? hi : Q;
}
// the warped byte of a tap (mblur_tap: at most 65280)
OFDG_HD_FN uint32_t reproj_byte(uint32_t t) { return (t + 128u) >> 8; }
// One component of the backward displacement at the target, in 24.8: the four finite elements in Q8 under the tap's
// weights, in int64.
OFDG_HD_FN int reproj_back(float b00, float b10, float b01, float b11, int fx, int fy) {
  const long long T = (long long)((256 - fx) * (256 - fy)) * reproj_q8(b00) + (long long)(fx * (256 - fy)) * reproj_q8(b10) +
                      (long long)((256 - fx) * fy) * reproj_q8(b01) + (long long)(fx * fy) * reproj_q8(b11);
  return (int)((T + 32768) >> 16);
}
// the squared forward-backward residual in units of 2^-16 px^2: each component clamped to 2^23 on its own
OFDG_HD_FN long long reproj_e2(int Dx, int Dy, int bx, int by) {
  long long ex = (long long)Dx + bx, ey = (long long)Dy + by;
  ex = ex < -8388608 ? -8388608 : ex > 8388608 ? 8388608 : ex;
  ey = ey < -8388608 ? -8388608 : ey > 8388608 ? 8388608 : ey;
  return ex * ex + ey * ey;
}
OFDG_HD_FN float reproj_fb2(long long e2) { return (float)e2 * 1.52587890625e-05f; }
// what a frame's block of the row can hold, from the inputs that are given
OFDG_HD_FN bool reproj_with_err(const DevReprojJob& j) { return j.img[0] && j.img[1]; }
OFDG_HD_FN bool reproj_with_fb(const DevReprojJob& j, int f) { return j.flow[1 - f] != nullptr; }
inline const char* reproj_plane_size(const DevReprojJob& j, int* width, int* height) { return job_plane_size(j, width, height); }  // (the name tests/test_reproject.py asks for)
// The argument rules ofdg_reproject and ofdg_host_reproject share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment is asked by the device entry only.
inline const char* reproj_arg_error(const DevReprojJob* j, int n, int width, int height) {
  if (!j) return "job is NULL";
  if (n < 1) return "n_samples must be at least 1";
  if (3ull * (unsigned long long)width * (unsigned long long)height >= (1ull << 32)) return "3 * width * height must be below 2^32";
  if (j->img_fmt != OFDG_FMT_F32 && j->img_fmt != OFDG_FMT_U8) return "img_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->dst_fmt != OFDG_FMT_F32 && j->dst_fmt != OFDG_FMT_U8) return "dst_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->flow_fmt != OFDG_FMT_F32 && j->flow_fmt != OFDG_FMT_F16) return "flow_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if ((j->occ[0] || j->occ[1]) && j->occ_fmt != OFDG_FMT_F32 && j->occ_fmt != OFDG_FMT_U8) return "occ_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->flags & ~(OFDG_REPROJ_FRAME0 | OFDG_REPROJ_FRAME1 | OFDG_REPROJ_ACCUMULATE)) return "flags holds unknown bits";
  if (j->reserved[0] != 0 || j->reserved[1] != 0) return "reserved must be 0";
  if (j->fb_thresh_q8 < 0 || j->fb_thresh_q8 > OFDG_REPROJ_MAX_FB_THRESH_Q8) return "fb_thresh_q8 must lie in 0..2^23";
  if (!(j->flags & (OFDG_REPROJ_FRAME0 | OFDG_REPROJ_FRAME1))) return "flags: no frame is flagged";
  bool any = j->rows != nullptr;
  for (int f = 0; f < 2; ++f) {
    const bool planes = j->warped[f] || j->err[f] || j->mask[f];
    if (!((j->flags >> f) & 1)) {
      if (planes || j->fb2[f]) return f ? "flags: frame 1 has an output but is not flagged" : "flags: frame 0 has an output but is not flagged";
      continue;
    }
    any = any || planes || j->fb2[f];
    if (!j->flow[f]) return f ? "flow[1]: a flagged frame needs its flow" : "flow[0]: a flagged frame needs its flow";
    if (planes && !j->img[1 - f]) return f ? "img[0]: warped, err and mask of frame 1 need the other frame" : "img[1]: warped, err and mask of frame 0 need the other frame";
    if (j->err[f] && !j->img[f]) return f ? "img[1]: err of frame 1 needs its own frame" : "img[0]: err of frame 0 needs its own frame";
    if (j->fb2[f] && !j->flow[1 - f]) return f ? "flow[0]: fb2 of frame 1 needs both flows" : "flow[1]: fb2 of frame 0 needs both flows";
  }
  if (!any) return "rows: no output is given";
  // no in-place form: a destination range may meet no other range of the job
  RangeSet<15> r;
  const unsigned long long plane = (unsigned long long)n * width * height;
  for (int f = 0; f < 2; ++f) {
    r.add_if(j->img[f], plane * 3 * fmt_elem_bytes(j->img_fmt), false);
    r.add_if(j->flow[f], plane * 2 * fmt_elem_bytes(j->flow_fmt), false);
    r.add_if(j->occ[f], plane * fmt_elem_bytes(j->occ_fmt), false);
    r.add_if(j->warped[f], plane * 3 * fmt_elem_bytes(j->dst_fmt), true);
    r.add_if(j->err[f], plane, true);
    r.add_if(j->mask[f], plane, true);
    r.add_if(j->fb2[f], plane * 4, true);
  }
  r.add_if(j->rows, (unsigned long long)n * sizeof(DevReprojRow), true);
  return r.overlap("a destination range overlaps another range of the job");
}

// ---- Splat (ofdg_splat, include/ofdg.h) ------------------------------------------------------------------------------------
// What the device entry, the kernels and the host twin share: the job, the record and the row as the kernels take them, the
// record's draw and its sanitising, the scaled displacement, the rounded target, the key and its decoding, the flow to the
// other frame and the argument rules.  The displacement is reproj_q8, the finite test mblur_finite, the byte of a float32
// photo_index.  Behind the one float32 product per component everything is integers.
constexpr uint32_t kSplatIndexMask = (1u << 24) - 1u;
static_assert(OFDG_SPLAT_MAX_PIXELS == (int)kSplatIndexMask, "a key holds a source index in 24 bits and is never 0");
struct DevSplatRec {  // ofdg_splat_rec, field for field
  int32_t t_q8[2];
  int32_t reserved[2];
};
struct DevSplatFrameRow {  // ofdg_splat_frame_row, field for field: the kernels add to the words with unsigned atomics
  uint32_t src[3];         // n_bad, n_outside, n_inside
  uint32_t dst[2];         // n_filled, n_holes
  uint32_t n_covered;
  uint32_t covered[2];     // visible, hidden
  uint32_t hole_other[2];  // visible, hidden
  uint32_t t_q8;
  uint32_t reserved[5];
};
struct DevSplatRow { DevSplatFrameRow frame[2]; };
struct DevSplatJob {  // struct ofdg_splat_job, field for field
  const void* img[2];
  const void* flow[2];
  const uint8_t* label[2];
  const void* occ[2];
  uint32_t* keys[2];
  void* image[2];
  void* to_own[2];
  void* to_other[2];
  void* mask[2];
  void* fate[2];
  DevSplatRow* rows;
  const DevSplatRec* recs;
  DevSplatRec* recs_out;
  long long first_index;
  uint32_t seed;
  int32_t width, height, img_fmt, dst_fmt, flow_fmt, oflow_fmt, occ_fmt, flags, t_min_q8, t_max_q8;
  int32_t reserved[2];
};
static_assert(sizeof(ofdg_splat_rec) == sizeof(DevSplatRec) && sizeof(DevSplatRec) == 16 && offsetof(ofdg_splat_rec, reserved) == offsetof(DevSplatRec, reserved) &&
              offsetof(DevSplatRec, reserved) == 8, "ofdg_splat_rec: 16 bytes without padding, the layout the kernels read and write");
static_assert(sizeof(ofdg_splat_frame_row) == sizeof(DevSplatFrameRow) && sizeof(DevSplatFrameRow) == 64 && offsetof(ofdg_splat_frame_row, n_bad) == offsetof(DevSplatFrameRow, src) &&
              offsetof(ofdg_splat_frame_row, n_filled) == offsetof(DevSplatFrameRow, dst) && offsetof(ofdg_splat_frame_row, n_covered) == offsetof(DevSplatFrameRow, n_covered) &&
              offsetof(DevSplatFrameRow, n_covered) == 20 && offsetof(ofdg_splat_frame_row, n_covered_visible) == offsetof(DevSplatFrameRow, covered) &&
              offsetof(ofdg_splat_frame_row, n_hole_other_visible) == offsetof(DevSplatFrameRow, hole_other) && offsetof(ofdg_splat_frame_row, t_q8) == offsetof(DevSplatFrameRow, t_q8) &&
              offsetof(DevSplatFrameRow, t_q8) == 40 && offsetof(ofdg_splat_frame_row, reserved) == offsetof(DevSplatFrameRow, reserved),
              "ofdg_splat_frame_row: 64 bytes without padding, the layout the kernels add to");
static_assert(sizeof(ofdg_splat_row) == sizeof(DevSplatRow) && sizeof(DevSplatRow) == 128 && offsetof(ofdg_splat_row, frame) == 0, "ofdg_splat_row: 128 bytes without padding, a block per frame");
static_assert(sizeof(struct ofdg_splat_job) == sizeof(DevSplatJob) && sizeof(DevSplatJob) == 248 && offsetof(struct ofdg_splat_job, flow) == offsetof(DevSplatJob, flow) &&
              offsetof(struct ofdg_splat_job, label) == offsetof(DevSplatJob, label) && offsetof(struct ofdg_splat_job, occ) == offsetof(DevSplatJob, occ) &&
              offsetof(struct ofdg_splat_job, keys) == offsetof(DevSplatJob, keys) && offsetof(struct ofdg_splat_job, image) == offsetof(DevSplatJob, image) &&
              offsetof(struct ofdg_splat_job, to_own) == offsetof(DevSplatJob, to_own) && offsetof(struct ofdg_splat_job, to_other) == offsetof(DevSplatJob, to_other) &&
              offsetof(struct ofdg_splat_job, mask) == offsetof(DevSplatJob, mask) && offsetof(struct ofdg_splat_job, fate) == offsetof(DevSplatJob, fate) &&
              offsetof(struct ofdg_splat_job, rows) == offsetof(DevSplatJob, rows) && offsetof(DevSplatJob, rows) == 160 && offsetof(struct ofdg_splat_job, recs) == offsetof(DevSplatJob, recs) &&
              offsetof(struct ofdg_splat_job, recs_out) == offsetof(DevSplatJob, recs_out) && offsetof(struct ofdg_splat_job, first_index) == offsetof(DevSplatJob, first_index) &&
              offsetof(struct ofdg_splat_job, seed) == offsetof(DevSplatJob, seed) && offsetof(DevSplatJob, seed) == 192 && offsetof(struct ofdg_splat_job, width) == offsetof(DevSplatJob, width) &&
              offsetof(struct ofdg_splat_job, img_fmt) == offsetof(DevSplatJob, img_fmt) && offsetof(struct ofdg_splat_job, occ_fmt) == offsetof(DevSplatJob, occ_fmt) &&
              offsetof(struct ofdg_splat_job, flags) == offsetof(DevSplatJob, flags) && offsetof(struct ofdg_splat_job, t_min_q8) == offsetof(DevSplatJob, t_min_q8) &&
              offsetof(struct ofdg_splat_job, t_max_q8) == offsetof(DevSplatJob, t_max_q8) && offsetof(DevSplatJob, t_max_q8) == 232 &&
              offsetof(struct ofdg_splat_job, reserved) == offsetof(DevSplatJob, reserved), "struct ofdg_splat_job: 248 bytes, the layout the kernels take");
// The record of global sample g: Philox block 0 under the sampler's key of g at the counter {0, 0, 0x0c77, 0}.  `j` supplies
// the range (splat_ranges_error has passed).
OFDG_HD_FN DevSplatRec splat_draw_rec(uint32_t seed, unsigned long long g, const DevSplatJob& j) {
  const CropWords w = crop_philox(CropWords{0u, 0u, 0x0c77u, 0u}, seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, (uint32_t)g);
  const int t = j.t_min_q8 + (int)(((unsigned long long)w.x * (unsigned long long)(j.t_max_q8 - j.t_min_q8 + 1)) >> 32);
  DevSplatRec r;
  r.t_q8[0] = t; r.t_q8[1] = 256 - t;
  r.reserved[0] = 0; r.reserved[1] = 0;
  return r;
}
// what is used of a record, given or drawn: each fraction clamped into 0..256
OFDG_HD_FN DevSplatRec splat_sanitise(DevSplatRec r) {
  for (int f = 0; f < 2; ++f) {
    r.t_q8[f] = r.t_q8[f] < 0 ? 0 : r.t_q8[f] > 256 ? 256 : r.t_q8[f];
    r.reserved[f] = 0;
  }
  return r;
}
// the 24.8 displacement D (reproj_q8) scaled by T / 256, T in 0..256
OFDG_HD_FN int splat_scale(int D, int T) { return (int)(((long long)D * T + 128) >> 8); }
// the rounded target on one axis of pixel `at` displaced by the scaled S (int64: 256 at + S may pass 2^31 on a very wide plane)
OFDG_HD_FN int splat_round(int at, int S) { return (int)((256ll * at + S + 128) >> 8); }
OFDG_HD_FN bool splat_inside(int rx, int ry, int W, int H) { return rx >= 0 && rx < W && ry >= 0 && ry < H; }
// the key of source index s (below 2^24 - 1) under label L: never 0
OFDG_HD_FN uint32_t splat_key(uint32_t L, uint32_t s) { return (L << 24) | (kSplatIndexMask - s); }
// the source index of a non-zero key
OFDG_HD_FN uint32_t splat_source(uint32_t K) { return kSplatIndexMask - (K & kSplatIndexMask); }
// one component of the flow from the target to the other frame: d = source - target in pixels, D the winner's displacement
OFDG_HD_FN float splat_to_other(int d, int D) { return (float)(256ll * d + D) * 0.00390625f; }
// does the launch of splat_resolve_kernel have anything to do?
OFDG_HD_FN bool splat_resolves(const DevSplatJob& j) {
  return j.rows || j.image[0] || j.image[1] || j.to_own[0] || j.to_own[1] || j.to_other[0] || j.to_other[1] || j.mask[0] || j.mask[1] || j.fate[0] || j.fate[1];
}
inline const char* splat_plane_size(const DevSplatJob& j, int* width, int* height) { return job_plane_size(j, width, height); }  // (the name tests/test_splat.py asks for)
// What the draw reads of a job: the first rule broken, or nullptr.
inline const char* splat_ranges_error(const DevSplatJob& j) {
  if (j.t_min_q8 < 0 || j.t_min_q8 > 256) return "t_min_q8 must lie in 0..256";
  if (j.t_max_q8 < 0 || j.t_max_q8 > 256) return "t_max_q8 must lie in 0..256";
  if (j.t_min_q8 > j.t_max_q8) return "t_min_q8 must not be above t_max_q8";
  return nullptr;
}
// The argument rules ofdg_splat and ofdg_host_splat share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment is asked by the device entry only.
inline const char* splat_arg_error(const DevSplatJob* j, int n, int width, int height) {
  if (!j) return "job is NULL";
  if (n < 1) return "n_samples must be at least 1";
  if ((unsigned long long)width * (unsigned long long)height > (unsigned long long)OFDG_SPLAT_MAX_PIXELS) return "width * height must be at most 2^24 - 1";
  if (j->img_fmt != OFDG_FMT_F32 && j->img_fmt != OFDG_FMT_U8) return "img_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->dst_fmt != OFDG_FMT_F32 && j->dst_fmt != OFDG_FMT_U8) return "dst_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->flow_fmt != OFDG_FMT_F32 && j->flow_fmt != OFDG_FMT_F16) return "flow_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if (j->oflow_fmt != OFDG_FMT_F32 && j->oflow_fmt != OFDG_FMT_F16) return "oflow_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if ((j->occ[0] || j->occ[1]) && j->occ_fmt != OFDG_FMT_F32 && j->occ_fmt != OFDG_FMT_U8) return "occ_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->flags & ~(OFDG_SPLAT_FRAME0 | OFDG_SPLAT_FRAME1 | OFDG_SPLAT_ACCUMULATE)) return "flags holds unknown bits";
  if (j->reserved[0] != 0 || j->reserved[1] != 0) return "reserved must be 0";
  if (!(j->flags & (OFDG_SPLAT_FRAME0 | OFDG_SPLAT_FRAME1))) return "flags: no frame is flagged";
  for (int f = 0; f < 2; ++f) {
    if (!((j->flags >> f) & 1)) {
      if (j->img[f] || j->flow[f] || j->label[f] || j->keys[f] || j->image[f] || j->to_own[f] || j->to_other[f] || j->mask[f] || j->fate[f])
        return f ? "flags: frame 1 has a pointer but is not flagged" : "flags: frame 0 has a pointer but is not flagged";
      continue;
    }
    if (!j->flow[f]) return f ? "flow[1]: a flagged frame needs its flow" : "flow[0]: a flagged frame needs its flow";
    if (!j->keys[f]) return f ? "keys[1]: a flagged frame needs its key plane" : "keys[0]: a flagged frame needs its key plane";
    if (j->image[f] && !j->img[f]) return f ? "img[1]: image of frame 1 needs its frame" : "img[0]: image of frame 0 needs its frame";
  }
  if (!j->recs)
    if (const char* why = splat_ranges_error(*j)) return why;
  // no in-place form: a written range may meet no other range of the job
  RangeSet<23> r;
  const unsigned long long plane = (unsigned long long)n * width * height;
  for (int f = 0; f < 2; ++f) {
    r.add_if(j->img[f], plane * 3 * fmt_elem_bytes(j->img_fmt), false);
    r.add_if(j->flow[f], plane * 2 * fmt_elem_bytes(j->flow_fmt), false);
    r.add_if(j->label[f], plane, false);
    r.add_if(j->occ[f], plane * fmt_elem_bytes(j->occ_fmt), false);
    r.add_if(j->keys[f], plane * 4, true);
    r.add_if(j->image[f], plane * 3 * fmt_elem_bytes(j->dst_fmt), true);
    r.add_if(j->to_own[f], plane * 2 * fmt_elem_bytes(j->oflow_fmt), true);
    r.add_if(j->to_other[f], plane * 2 * fmt_elem_bytes(j->oflow_fmt), true);
    r.add_if(j->mask[f], plane, true);
    r.add_if(j->fate[f], plane, true);
  }
  r.add_if(j->rows, (unsigned long long)n * sizeof(DevSplatRow), true);
  r.add_if(j->recs, (unsigned long long)n * sizeof(DevSplatRec), false);
  r.add_if(j->recs_out, (unsigned long long)n * sizeof(DevSplatRec), true);
  return r.overlap("a written range overlaps another range of the job");
}

// ---- Flow visualisation (ofdg_flow_vis, include/ofdg.h) --------------------------------------------------------------------
// What the device entry, the kernels and the host twin share: the job as the kernels take it, the two constant tables, the
// steps of the definition on one pixel and the argument rules.  Behind the rounding of u and v to Q8 everything is integers.
struct DevVisRow {  // ofdg_flow_vis_row, field for field
  unsigned long long max_r2;
  uint32_t scale_q8, reserved;
};
struct DevVisJob {  // struct ofdg_flow_vis_job, field for field
  const void* flow;
  const void* occ;
  void* dst;
  DevVisRow* rows_out;
  unsigned long long* work;  // one 64-bit maximum per sample
  int32_t width, height, flow_fmt, occ_fmt, layout, norm, flags, reserved;
  float max_flow;
  int32_t reserved2[5];
};
static_assert(sizeof(ofdg_flow_vis_row) == sizeof(DevVisRow) && sizeof(DevVisRow) == 16 && offsetof(ofdg_flow_vis_row, scale_q8) == offsetof(DevVisRow, scale_q8) &&
              offsetof(DevVisRow, scale_q8) == 8 && sizeof(unsigned long long) == OFDG_FLOW_VIS_WORK_BYTES,
              "ofdg_flow_vis_row: 16 bytes, written as one piece; a sample's workspace");
static_assert(sizeof(struct ofdg_flow_vis_job) == sizeof(DevVisJob) && sizeof(DevVisJob) == 96 && offsetof(struct ofdg_flow_vis_job, occ) == offsetof(DevVisJob, occ) &&
              offsetof(struct ofdg_flow_vis_job, dst) == offsetof(DevVisJob, dst) && offsetof(struct ofdg_flow_vis_job, rows_out) == offsetof(DevVisJob, rows_out) &&
              offsetof(struct ofdg_flow_vis_job, work) == offsetof(DevVisJob, work) && offsetof(struct ofdg_flow_vis_job, width) == offsetof(DevVisJob, width) &&
              offsetof(DevVisJob, width) == 40 && offsetof(struct ofdg_flow_vis_job, norm) == offsetof(DevVisJob, norm) && offsetof(DevVisJob, norm) == 60 &&
              offsetof(struct ofdg_flow_vis_job, max_flow) == offsetof(DevVisJob, max_flow) && offsetof(DevVisJob, max_flow) == 72 &&
              offsetof(struct ofdg_flow_vis_job, reserved2) == offsetof(DevVisJob, reserved2),
              "struct ofdg_flow_vis_job: 96 bytes, the layout the kernels take");
constexpr int kVisAtanEntries = 257, kVisWheelEntries = 55;
// A[k] = lrint(atan(k / 256) / (2 pi) * 2^24): the angle of slope k / 256 as a turn fraction in Q24
constexpr int32_t kVisAtan[kVisAtanEntries] = {
    0, 10430, 20860, 31290, 41718, 52145, 62571, 72994, 83416, 93835, 104251, 114664, 125073, 135479, 145880, 156277,
    166669, 177056, 187438, 197815, 208185, 218549, 228906, 239256, 249600, 259935, 270263, 280583, 290894, 301197, 311491, 321775,
    332050, 342315, 352570, 362814, 373047, 383270, 393481, 403681, 413869, 424044, 434208, 444358, 454496, 464620, 474731, 484829,
    494912, 504981, 515035, 525075, 535100, 545109, 555103, 565081, 575043, 584989, 594918, 604831, 614727, 624606, 634467, 644311,
    654136, 663944, 673734, 683505, 693257, 702990, 712705, 722400, 732076, 741732, 751368, 760984, 770579, 780155, 789709, 799243,
    808756, 818248, 827718, 837168, 846595, 856001, 865384, 874746, 884085, 893402, 902696, 911968, 921217, 930443, 939645, 948825,
    957981, 967114, 976223, 985308, 994370, 1003407, 1012421, 1021410, 1030375, 1039316, 1048232, 1057123, 1065990, 1074832, 1083649, 1092442,
    1101209, 1109951, 1118668, 1127359, 1136026, 1144667, 1153282, 1161872, 1170436, 1178975, 1187488, 1195975, 1204436, 1212871, 1221280, 1229664,
    1238021, 1246352, 1254658, 1262937, 1271189, 1279416, 1287616, 1295790, 1303938, 1312059, 1320154, 1328223, 1336265, 1344281, 1352271, 1360234,
    1368170, 1376081, 1383964, 1391822, 1399652, 1407457, 1415234, 1422986, 1430711, 1438409, 1446081, 1453727, 1461346, 1468939, 1476505, 1484045,
    1491559, 1499046, 1506507, 1513942, 1521350, 1528733, 1536089, 1543419, 1550722, 1558000, 1565251, 1572477, 1579676, 1586849, 1593997, 1601118,
    1608214, 1615284, 1622328, 1629346, 1636338, 1643305, 1650246, 1657162, 1664052, 1670917, 1677757, 1684570, 1691359, 1698123, 1704861, 1711574,
    1718262, 1724925, 1731563, 1738176, 1744764, 1751327, 1757866, 1764380, 1770869, 1777334, 1783774, 1790190, 1796582, 1802949, 1809292, 1815611,
    1821906, 1828177, 1834423, 1840646, 1846846, 1853021, 1859173, 1865301, 1871405, 1877486, 1883544, 1889578, 1895590, 1901578, 1907542, 1913484,
    1919403, 1925299, 1931173, 1937023, 1942851, 1948656, 1954439, 1960199, 1965938, 1971653, 1977347, 1983018, 1988668, 1994295, 1999901, 2005485,
    2011047, 2016588, 2022107, 2027604, 2033080, 2038535, 2043968, 2049381, 2054772, 2060142, 2065491, 2070820, 2076127, 2081414, 2086681, 2091927,
    2097152};
// The colour wheel of Baker et al., entry k as R | G << 8 | B << 16: RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 entries
#define VIS_RGB(r, g, b) ((uint32_t)(r) | ((uint32_t)(g) << 8) | ((uint32_t)(b) << 16))
constexpr uint32_t kVisWheel[kVisWheelEntries] = {
    VIS_RGB(255, 0, 0), VIS_RGB(255, 17, 0), VIS_RGB(255, 34, 0), VIS_RGB(255, 51, 0), VIS_RGB(255, 68, 0), VIS_RGB(255, 85, 0),
    VIS_RGB(255, 102, 0), VIS_RGB(255, 119, 0), VIS_RGB(255, 136, 0), VIS_RGB(255, 153, 0), VIS_RGB(255, 170, 0), VIS_RGB(255, 187, 0),
    VIS_RGB(255, 204, 0), VIS_RGB(255, 221, 0), VIS_RGB(255, 238, 0), VIS_RGB(255, 255, 0), VIS_RGB(213, 255, 0), VIS_RGB(170, 255, 0),
    VIS_RGB(128, 255, 0), VIS_RGB(85, 255, 0), VIS_RGB(43, 255, 0), VIS_RGB(0, 255, 0), VIS_RGB(0, 255, 63), VIS_RGB(0, 255, 127),
    VIS_RGB(0, 255, 191), VIS_RGB(0, 255, 255), VIS_RGB(0, 232, 255), VIS_RGB(0, 209, 255), VIS_RGB(0, 186, 255), VIS_RGB(0, 163, 255),
    VIS_RGB(0, 140, 255), VIS_RGB(0, 116, 255), VIS_RGB(0, 93, 255), VIS_RGB(0, 70, 255), VIS_RGB(0, 47, 255), VIS_RGB(0, 24, 255),
    VIS_RGB(0, 0, 255), VIS_RGB(19, 0, 255), VIS_RGB(39, 0, 255), VIS_RGB(58, 0, 255), VIS_RGB(78, 0, 255), VIS_RGB(98, 0, 255),
    VIS_RGB(117, 0, 255), VIS_RGB(137, 0, 255), VIS_RGB(156, 0, 255), VIS_RGB(176, 0, 255), VIS_RGB(196, 0, 255), VIS_RGB(215, 0, 255),
    VIS_RGB(235, 0, 255), VIS_RGB(255, 0, 255), VIS_RGB(255, 0, 213), VIS_RGB(255, 0, 170), VIS_RGB(255, 0, 128), VIS_RGB(255, 0, 85),
    VIS_RGB(255, 0, 43)};
#undef VIS_RGB
constexpr uint32_t kVisRhoOut = 65537u;  // the radius of every vector out of range
// steps 1 and 2: the usable pixel and its Q8 components
OFDG_HD_FN bool vis_usable(float u, float v) { return fabsf(u) < 1048576.0f && fabsf(v) < 1048576.0f; }
OFDG_HD_FN int vis_fixed(float u) { return (int)rintf(u * 256.0f); }
OFDG_HD_FN unsigned long long vis_r2(int U, int V) { return (unsigned long long)((long long)U * U) + (unsigned long long)((long long)V * V); }
// floor(sqrt(x)) for x < 2^58, exact.  On the device: the hardware's float root, one Newton step in double (the error falls
// from 2^-22 of the root to far below 1) and one correction step either way; on the host the double root and the same step.
OFDG_HD_FN uint32_t vis_isqrt(unsigned long long x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double xd = (double)x;
  const float s = __builtin_amdgcn_sqrtf((float)xd);
  const double g = (double)s;
  const double g1 = g + __builtin_fma(-g, g, xd) * (double)(0.5f * __builtin_amdgcn_rcpf(s > 0.0f ? s : 1.0f));
  uint32_t r = (uint32_t)g1;
#else
  uint32_t r = (uint32_t)sqrt((double)x);
#endif
  const unsigned long long rr = (unsigned long long)r * r;
  return rr > x ? r - 1u : rr + 2ull * r + 1ull <= x ? r + 1u : r;
}
// floor((a << 16) / d) for a < 2^29 and 1 <= d < 2^30: exact where the quotient is at most `cap` (<= 65536), some value above
// `cap` where it is larger.  On the device: the float quotient (off by less than 2^-21 of itself, so by less than 1 up to the
// cap) and one correction step either way, as jitter_div; inv: the float reciprocal of d, which the caller may keep.
OFDG_HD_FN uint32_t vis_div16(uint32_t a, uint32_t d, float inv, uint32_t cap) {
  const unsigned long long num = (unsigned long long)a << 16;
#if defined(__HIP_DEVICE_COMPILE__)
  const float qf = (float)a * inv * 65536.0f;
  const uint32_t q = (uint32_t)(qf < (float)(cap + 1u) ? qf : (float)(cap + 1u));
  const long long r = (long long)num - (long long)((unsigned long long)q * d);
  return q + (r >= (long long)d ? 1u : 0u) - (r < 0 ? 1u : 0u);
#else
  (void)inv;
  const unsigned long long q = num / d;
  return q > cap + 1u ? cap + 1u : (uint32_t)q;
#endif
}
OFDG_HD_FN float vis_inv(uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf((float)d);
#else
  (void)d;
  return 0.0f;
#endif
}
// step 3: M of a largest R2, and of max_flow
OFDG_HD_FN uint32_t vis_scale_of(unsigned long long max_r2) {
  const uint32_t m = vis_isqrt(max_r2);
  return m > 1u ? m : 1u;
}
OFDG_HD_FN uint32_t vis_scale_fixed(float max_flow) { return (uint32_t)lrintf(max_flow * 256.0f); }
// step 5: the angle of (U, V) as a turn fraction in Q16, y pointing down; A: the 257 entries of kVisAtan where they lie
OFDG_HD_FN uint32_t vis_angle(int U, int V, const int32_t* A) {
  const uint32_t ax = (uint32_t)(U < 0 ? -U : U), ay = (uint32_t)(V < 0 ? -V : V);
  const uint32_t mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax, div = mx ? mx : 1u;
  const uint32_t t = vis_div16(mn, div, vis_inv(div), 65536u);  // (mn <= mx: at most 65536)
  const uint32_t i = t >> 8, fr = t & 255u, i1 = i < 256u ? i + 1u : 256u;
  const int32_t a24 = A[i] + (((A[i1] - A[i]) * (int32_t)fr + 128) >> 8);
  const int32_t o = (a24 + 128) >> 8;
  int32_t b = ax >= ay ? o : 16384 - o;
  b = U < 0 ? 32768 - b : b;
  b = V < 0 ? (65536 - b) & 65535 : b;
  return (uint32_t)b;
}
// steps 6 and 7 for one channel: w0, w1 the two wheel entries' bytes, f the fraction between them in Q16
OFDG_HD_FN uint32_t vis_channel(uint32_t w0, uint32_t w1, uint32_t f, uint32_t rho) {
  const uint32_t c16 = w0 * (65536u - f) + w1 * f;
  if (rho > 65536u) return (3u * c16) >> 18;
  return (uint32_t)(((16711680ll << 16) - (long long)rho * (long long)(16711680u - c16)) >> 32);
}
// Steps 2 and 4 to 8 of a usable pixel: R | G << 8 | B << 16.  M: the scale, inv_m: vis_inv(M); wheel: the 55 entries of
// kVisWheel where they lie.
OFDG_HD_FN uint32_t vis_pixel(float u, float v, uint32_t M, float inv_m, bool dim, const int32_t* A, const uint32_t* wheel) {
  const int U = vis_fixed(u), V = vis_fixed(v);
  const uint32_t Rq = vis_isqrt(vis_r2(U, V));
  const uint32_t q = vis_div16(Rq, M, inv_m, 65536u);
  const uint32_t rho = q > kVisRhoOut ? kVisRhoOut : q;
  const uint32_t fk = vis_angle(U, V, A) * 54u, k0 = fk >> 16, f = fk & 65535u;
  const uint32_t e0 = wheel[k0], e1 = wheel[k0 + 1u];
  uint32_t R = vis_channel(e0 & 255u, e1 & 255u, f, rho), G = vis_channel((e0 >> 8) & 255u, (e1 >> 8) & 255u, f, rho), B = vis_channel(e0 >> 16, e1 >> 16, f, rho);
  if (dim) { R >>= 1; G >>= 1; B >>= 1; }
  return R | (G << 8) | (B << 16);
}
inline bool vis_needs_work(const DevVisJob& j) { return j.norm != OFDG_VIS_NORM_FIXED; }
// The argument rules ofdg_flow_vis and ofdg_host_flow_vis share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment and `work` are asked by the device entry only (with_work).
inline const char* vis_arg_error(const DevVisJob* j, int n, int width, int height, bool with_work) {
  if (!j) return "job is NULL";
  if (!j->flow) return "flow is NULL";
  if (!j->dst) return "dst is NULL";
  if (n < 1) return "n_samples must be at least 1";
  if (3ull * (unsigned long long)width * (unsigned long long)height >= (1ull << 32)) return "3 * width * height must be below 2^32";
  if (const char* why = flow_occ_fmt_error(j->flow_fmt, j->occ != nullptr, j->occ_fmt)) return why;
  if (j->layout != OFDG_VIS_PLANAR_BGR && j->layout != OFDG_VIS_HWC_RGB) return "layout must be OFDG_VIS_PLANAR_BGR or OFDG_VIS_HWC_RGB";
  if (j->norm != OFDG_VIS_NORM_FIXED && j->norm != OFDG_VIS_NORM_SAMPLE && j->norm != OFDG_VIS_NORM_BATCH)
    return "norm must be OFDG_VIS_NORM_FIXED, OFDG_VIS_NORM_SAMPLE or OFDG_VIS_NORM_BATCH";
  if (j->flags & ~OFDG_VIS_DIM_OCC) return "flags holds unknown bits";
  if (j->reserved != 0) return "reserved must be 0";
  for (int k = 0; k < 5; ++k)
    if (j->reserved2[k] != 0) return "reserved2 must be 0";
  if ((j->flags & OFDG_VIS_DIM_OCC) && !j->occ) return "flags: OFDG_VIS_DIM_OCC needs occ";
  if (j->norm == OFDG_VIS_NORM_FIXED && !(j->max_flow >= 0.00390625f && j->max_flow <= 1048576.0f)) return "max_flow must lie in [2^-8, 2^20]";
  const bool work = with_work && vis_needs_work(*j);
  if (work && !j->work) return "work is NULL where norm is not OFDG_VIS_NORM_FIXED";
  RangeSet<5> r;
  const unsigned long long plane = (unsigned long long)n * width * height;
  r.add(j->flow, 2ull * plane * fmt_elem_bytes(j->flow_fmt), false);
  r.add_if(j->occ, plane * fmt_elem_bytes(j->occ_fmt), false);
  r.add(j->dst, 3ull * plane, true);
  r.add_if(j->rows_out, (unsigned long long)n * sizeof(DevVisRow), true);
  if (work) r.add(j->work, (unsigned long long)n * sizeof(unsigned long long), true);
  return r.overlap("a written range overlaps another range of the job");
}

// ---- Flow error (ofdg_flow_error, include/ofdg.h) --------------------------------------------------------------------------
// What the device entry, the kernel and the host twin share: the job and the row as the kernel takes them, the colour table,
// the steps of the definition on one pixel and the argument rules.  Behind the rounding of the four components to Q8
// (vis_fixed) everything is integers; the roots are vis_isqrt, whose correction step is exact for every x below 2^60 (r < 2^30:
// r r + 2 r + 1 stays in 64 bits) - E2 is below 2^59.
struct DevErrCell {  // ofdg_flow_error_cell, field for field
  unsigned long long sum_epe_q8;
  uint32_t n, n_1px, n_3px, n_5px, n_fl, reserved;
};
constexpr int kErrCells = 18, kErrHistBins = OFDG_FLOW_ERROR_HIST_BINS, kErrColours = 10;
struct DevErrRow {  // ofdg_flow_error_row, field for field
  DevErrCell cell[kErrCells];  // [hidden][speed band][distance band]
  uint32_t hist[kErrHistBins];
  unsigned long long max_key;
  uint32_t n_bad[2];  // n_bad_gt, n_bad_est
  uint32_t reserved[4];
};
struct DevErrJob {  // struct ofdg_flow_error_job, field for field
  const void* gt;
  const void* est;
  const void* occ;
  const uint8_t* dist2;
  DevErrRow* rows;
  void* epe;
  void* picture;
  int32_t width, height, gt_fmt, est_fmt, occ_fmt, epe_fmt, layout, flags;
  float est_scale;
  float speed_px[2];
  int32_t dist2_edge[2];
  int32_t reserved[5];
};
static_assert(sizeof(ofdg_flow_error_cell) == sizeof(DevErrCell) && sizeof(DevErrCell) == 32 && offsetof(ofdg_flow_error_cell, n) == offsetof(DevErrCell, n) &&
              offsetof(DevErrCell, n) == 8 && offsetof(ofdg_flow_error_cell, n_fl) == offsetof(DevErrCell, n_fl) && offsetof(DevErrCell, n_fl) == 24,
              "ofdg_flow_error_cell: 32 bytes");
static_assert(sizeof(ofdg_flow_error_row) == sizeof(DevErrRow) && sizeof(DevErrRow) == 672 && offsetof(ofdg_flow_error_row, hist) == offsetof(DevErrRow, hist) &&
              offsetof(DevErrRow, hist) == 576 && offsetof(ofdg_flow_error_row, max_key) == offsetof(DevErrRow, max_key) && offsetof(DevErrRow, max_key) == 640 &&
              offsetof(ofdg_flow_error_row, n_bad_gt) == offsetof(DevErrRow, n_bad) && offsetof(ofdg_flow_error_row, n_bad_est) == offsetof(DevErrRow, n_bad) + 4 &&
              offsetof(ofdg_flow_error_row, reserved) == offsetof(DevErrRow, reserved),
              "ofdg_flow_error_row: 672 bytes, no padding");
static_assert(sizeof(struct ofdg_flow_error_job) == sizeof(DevErrJob) && sizeof(DevErrJob) == 128 && offsetof(struct ofdg_flow_error_job, dist2) == offsetof(DevErrJob, dist2) &&
              offsetof(struct ofdg_flow_error_job, rows) == offsetof(DevErrJob, rows) && offsetof(struct ofdg_flow_error_job, picture) == offsetof(DevErrJob, picture) &&
              offsetof(struct ofdg_flow_error_job, width) == offsetof(DevErrJob, width) && offsetof(DevErrJob, width) == 56 &&
              offsetof(struct ofdg_flow_error_job, flags) == offsetof(DevErrJob, flags) && offsetof(DevErrJob, flags) == 84 &&
              offsetof(struct ofdg_flow_error_job, est_scale) == offsetof(DevErrJob, est_scale) && offsetof(DevErrJob, est_scale) == 88 &&
              offsetof(struct ofdg_flow_error_job, speed_px) == offsetof(DevErrJob, speed_px) &&
              offsetof(struct ofdg_flow_error_job, dist2_edge) == offsetof(DevErrJob, dist2_edge) && offsetof(DevErrJob, dist2_edge) == 100 &&
              offsetof(struct ofdg_flow_error_job, reserved) == offsetof(DevErrJob, reserved) && OFDG_ERR_ACCUMULATE == 1 && OFDG_ERR_ONE_ROW == 2 && OFDG_ERR_DIM_OCC == 4,
              "struct ofdg_flow_error_job: 128 bytes, the layout the kernel takes");
// The KITTI devkit's error colours, bin k as R | G << 8 | B << 16
#define ERR_RGB(r, g, b) ((uint32_t)(r) | ((uint32_t)(g) << 8) | ((uint32_t)(b) << 16))
constexpr uint32_t kErrColour[kErrColours] = {ERR_RGB(49, 54, 149),   ERR_RGB(69, 117, 180), ERR_RGB(116, 173, 209), ERR_RGB(171, 217, 233),
                                              ERR_RGB(224, 243, 248), ERR_RGB(254, 224, 144), ERR_RGB(253, 174, 97),  ERR_RGB(244, 109, 67),
                                              ERR_RGB(215, 48, 39),   ERR_RGB(165, 0, 38)};
#undef ERR_RGB
// step 1: bfloat16 bits widened (exact), and the estimate's scaling - one float32 product
OFDG_HD_FN float err_bf16(uint32_t bits) {
  const uint32_t w = bits << 16;
  float f;
  __builtin_memcpy(&f, &w, 4);
  return f;
}
OFDG_HD_FN float err_scaled(float e, float est_scale) { return e * est_scale; }
// what a call keeps of the job's bands: S_0, S_1 in Q8 pixels and the two edges of dist2
struct ErrBands {
  uint32_t speed[2];
  uint32_t dist[2];
};
OFDG_HD_FN ErrBands err_bands(const DevErrJob& j) {
  return ErrBands{{(uint32_t)lrintf(j.speed_px[0] * 256.0f), (uint32_t)lrintf(j.speed_px[1] * 256.0f)}, {(uint32_t)j.dist2_edge[0], (uint32_t)j.dist2_edge[1]}};
}
// step 5 of a pixel whose four components are usable
struct ErrPixel {
  uint32_t Eq, Gq;
};
OFDG_HD_FN ErrPixel err_pixel(float ug, float vg, float ue, float ve) {
  const int Ug = vis_fixed(ug), Vg = vis_fixed(vg), Ue = vis_fixed(ue), Ve = vis_fixed(ve);
  return ErrPixel{vis_isqrt(vis_r2(Ue - Ug, Ve - Vg)), vis_isqrt(vis_r2(Ug, Vg))};
}
// step 6: the cell's index, (hidden * 3 + speed band) * 3 + distance band; d2: the pixel's dist2, 0 without a plane
OFDG_HD_FN uint32_t err_cell(bool hidden, uint32_t Gq, uint32_t d2, bool with_dist, const ErrBands& b) {
  const uint32_t sb = (Gq >= b.speed[0] ? 1u : 0u) + (Gq >= b.speed[1] ? 1u : 0u);
  const uint32_t db = with_dist ? (d2 >= b.dist[0] ? 1u : 0u) + (d2 >= b.dist[1] ? 1u : 0u) : 0u;
  return ((hidden ? 3u : 0u) + sb) * 3u + db;
}
// step 7: the four flags of a pixel, bit 0 n_1px, 1 n_3px, 2 n_5px, 3 n_fl
OFDG_HD_FN uint32_t err_flags(uint32_t Eq, uint32_t Gq) {
  return (Eq > 256u ? 1u : 0u) | (Eq > 768u ? 2u : 0u) | (Eq > 1280u ? 4u : 0u) | ((Eq > 768u && 20ull * Eq > (unsigned long long)Gq) ? 8u : 0u);
}
// step 8: the number of k in 0..14 with Eq >= (16 << k): 0 below 16, else floor(log2(Eq)) - 3, at most 15
OFDG_HD_FN uint32_t err_hist_bin(uint32_t Eq) {
  if (Eq < 16u) return 0u;
  const uint32_t b = (uint32_t)(31 - __builtin_clz(Eq)) - 3u;
  return b < 15u ? b : 15u;
}
OFDG_HD_FN unsigned long long err_key(uint32_t Eq, uint32_t idx) { return ((unsigned long long)Eq << 32) | (unsigned long long)(0xFFFFFFFFu - idx); }
// step 9: the float32 of Eq / 256 (the conversion rounds to nearest even, the product is exact)
OFDG_HD_FN float err_epe(uint32_t Eq) { return (float)Eq * 0.00390625f; }
// step 10: the bin - both conditions only get harder with j, so the count stops at the first that fails - and the colour
OFDG_HD_FN uint32_t err_colour_bin(uint32_t Eq, uint32_t Gq) {
  uint32_t bin = 0;
  for (int j = 0; j < 9; ++j) bin += (Eq >= (48u << j) && 320ull * Eq >= ((unsigned long long)Gq << j)) ? 1u : 0u;
  return bin;
}
OFDG_HD_FN uint32_t err_colour(uint32_t Eq, uint32_t Gq, bool dim, const uint32_t* table) {
  const uint32_t c = table[err_colour_bin(Eq, Gq)];
  return dim ? (c >> 1) & 0x7F7F7Fu : c;
}
// The argument rules ofdg_flow_error and ofdg_host_flow_error share: the first rule broken, or nullptr.  width, height: what
// job_plane_size gave.  Alignment is asked by the device entry only.
inline const char* err_arg_error(const DevErrJob* j, int n, int width, int height) {
  if (!j) return "job is NULL";
  if (!j->gt) return "gt is NULL";
  if (!j->est) return "est is NULL";
  if (!j->rows && !j->epe && !j->picture) return "rows, epe and picture are all NULL: no output";
  if (n < 1) return "n_samples must be at least 1";
  const unsigned long long plane = (unsigned long long)width * (unsigned long long)height;
  if (3ull * plane >= (1ull << 32)) return "3 * width * height must be below 2^32";
  if (j->flags & ~(OFDG_ERR_ACCUMULATE | OFDG_ERR_ONE_ROW | OFDG_ERR_DIM_OCC)) return "flags holds unknown bits";
  if ((j->flags & OFDG_ERR_ONE_ROW) && (unsigned long long)n * plane >= (1ull << 32)) return "flags: OFDG_ERR_ONE_ROW needs n_samples * height * width below 2^32";
  if (j->gt_fmt != OFDG_FMT_F32 && j->gt_fmt != OFDG_FMT_F16) return "gt_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if (j->est_fmt != OFDG_FMT_F32 && j->est_fmt != OFDG_FMT_F16 && j->est_fmt != OFDG_FMT_BF16) return "est_fmt must be OFDG_FMT_F32, OFDG_FMT_F16 or OFDG_FMT_BF16";
  if (j->occ && j->occ_fmt != OFDG_FMT_F32 && j->occ_fmt != OFDG_FMT_U8) return "occ_fmt must be OFDG_FMT_F32 or OFDG_FMT_U8";
  if (j->epe && j->epe_fmt != OFDG_FMT_F32 && j->epe_fmt != OFDG_FMT_F16) return "epe_fmt must be OFDG_FMT_F32 or OFDG_FMT_F16";
  if (j->layout != OFDG_VIS_PLANAR_BGR && j->layout != OFDG_VIS_HWC_RGB) return "layout must be OFDG_VIS_PLANAR_BGR or OFDG_VIS_HWC_RGB";
  for (int k = 0; k < 5; ++k)
    if (j->reserved[k] != 0) return "reserved must be 0";
  if ((j->flags & OFDG_ERR_DIM_OCC) && !j->occ) return "flags: OFDG_ERR_DIM_OCC needs occ";
  if ((j->flags & OFDG_ERR_DIM_OCC) && !j->picture) return "flags: OFDG_ERR_DIM_OCC needs picture";
  if (!(fabsf(j->est_scale) >= 0.0009765625f && fabsf(j->est_scale) <= 1024.0f)) return "est_scale: its magnitude must lie in [2^-10, 2^10]";
  if (!(j->speed_px[0] > 0.0f && j->speed_px[0] <= j->speed_px[1] && j->speed_px[1] <= 1048576.0f)) return "speed_px must be 0 < speed_px[0] <= speed_px[1] <= 2^20";
  if (j->dist2 && !(1 <= j->dist2_edge[0] && j->dist2_edge[0] <= j->dist2_edge[1] && j->dist2_edge[1] <= 255))
    return "dist2_edge must be 1 <= dist2_edge[0] <= dist2_edge[1] <= 255";
  RangeSet<7> r;
  const unsigned long long all = (unsigned long long)n * plane;
  r.add(j->gt, 2ull * all * fmt_elem_bytes(j->gt_fmt), false);
  r.add(j->est, 2ull * all * fmt_elem_bytes(j->est_fmt), false);
  r.add_if(j->occ, all * fmt_elem_bytes(j->occ_fmt), false);
  r.add_if(j->dist2, all, false);
  r.add_if(j->rows, sizeof(DevErrRow) * (unsigned long long)((j->flags & OFDG_ERR_ONE_ROW) ? 1 : n), true);
  r.add_if(j->epe, all * fmt_elem_bytes(j->epe_fmt), true);
  r.add_if(j->picture, 3ull * all, true);
  return r.overlap("a written range overlaps another range of the job");
}

// Background texture preparation of one sample (ofdg_params.background_prep = 1):
// Texture::getRandomizedCrop(2W, 2H, rot, zoom, shift), DG:87-109 - the CImg chain
// get_shift -> rotate -> crop -> resize as ONE resampling along its composed coordinate map.
struct DevBgPrep {
  float ca, sa;            // cos / sin of the rotation (CImg: the angle counts as degrees)
  float w2, h2, rw2, rh2;  // centres of the pool image and of the (grown) rotated image
  float fx, fy;            // resize step: crop columns / rows per prepared texel
  int32_t x0, y0;          // crop origin in the rotated image
  int32_t cw, ch;          // crop size
  int32_t shx, shy;        // get_shift offsets
  uint64_t image_addr;     // device address of the pool image (BGRX texels, pw x ph)
  int32_t rx0, ry0, rx1, ry1;  // texels of the 2W x 2H texture compose can read (inclusive); the rest is not rendered
  int32_t rw, rh;              // size of the rotated image (crop coordinates are mirrored into it)
  int32_t pw, ph;              // size of the pool image (texture lists may hold images of different sizes)
};
// Where a whole pool image lives (background preparation reads the original image): the table of a pool with images of
// different sizes; a uniform pool needs none (image i = base + i * w * h).
struct DevTexEntry {
  uint64_t addr;
  int32_t w, h;
};

// Where an object's texture lives relative to a pool pointer: image i starts at i * stride, its
// W x H (foreground) or 2W x 2H (background) window at + origin, rows are `pitch` texels apart.
// Pool images at least as large as the window: the centre crop of the image itself
// (getRandomizedCrop, DG:96-101); smaller images: a pool of resized copies (DG:102-106).
struct TexSource {
  uint64_t stride, origin;
  int32_t pitch, pad;
};

// Pointers the kernels read out of records are typed as GLOBAL memory in device code (a pointer loaded from memory is
// generic otherwise: flat_load, which also counts on lgkmcnt and so serialises with every scalar wait).
// OFDG_CONSTANT: memory no kernel writes while it runs; a uniform load from it is a scalar load even behind the kernel's own
// stores (which the compiler must otherwise assume could alias it).
#if defined(__HIP_DEVICE_COMPILE__)
#define OFDG_GLOBAL __attribute__((address_space(1)))
#define OFDG_CONSTANT __attribute__((address_space(4)))
#else
#define OFDG_GLOBAL
#define OFDG_CONSTANT
#endif
// One served warp crop as the kernels see it (mode 9).
struct DevCropRef {
  OFDG_GLOBAL const float* data;         // two planes of w*h float PAIRS: (flow x, flow y), then (iflow x, iflow y)
  OFDG_GLOBAL const unsigned* max_bits;  // float bits of max |iflow| over the crop (NaNs ignored)
  int32_t w, h;
};
inline DevCropRef make_crop_ref(const float* data, const unsigned* max_bits, int w, int h) {
  DevCropRef r;
  r.data = (OFDG_GLOBAL const float*)data; r.max_bits = (OFDG_GLOBAL const unsigned*)max_bits; r.w = w; r.h = h;
  return r;
}

struct RenderDims {
  int32_t W, H;            // output size
  int32_t pool_w, pool_h;  // pool image size (texels are BGRX u32)
  int32_t use_aa;
  int32_t n_samples;
  int32_t n_shapes;        // total rasterised shapes in the batch
  int32_t tiles_x, tiles_y;
  int32_t bg_pitch;        // row pitch (texels) of the background textures: pool_w, or 2W when they are prepared per sample / resized
  int32_t fg_pitch;        // row pitch of the foreground textures: pool_w, or W when the pool images are smaller than W x H
};

}  // namespace ofdg
