// HIP kernels of the render pipeline, written for gfx950 (MI355X, wave64).
//
//   geom_kernel     blueprint shape + 2x3 affine  -> 24.8 fixed-point outline + bbox
//   raster_kernel   outline -> AGG-exact coverage bytes (cells accumulated in LDS with
//                   integer atomics, per-row wavefront prefix sum of `cover`)
//   compose_kernel  background + painter's-order objects -> image0, image1, flow
//
// Everything the reference computes in integers is bit-exact here; fp64 affine
// algebra is evaluated with the reference's operation order and no contraction
// (the file is compiled with -ffp-contract=off).
//
// Reference (lmb-freiburg/optical-flow-2d-data-generation):
//   DG = src/caffe/DataGenerator.cpp.  AGG = Anti-Grain Geometry 2.4 (un-vendored
//   dependency, cmake/Dependencies.cmake:4-19); its algorithms are restated here in
//   closed form so that (edge, scanline) pairs can be processed independently.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/ofdg_detmath.h"
#include "ofdg_device.h"
#include "realize.h"  // mat_invert
#include "warpfields.h"

namespace ofdg {

// The file's vector types: what one 4-, 8- or 16-byte load or store instruction moves.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// --------------------------------------------------------------------------
// small helpers
// --------------------------------------------------------------------------
__device__ __forceinline__ int iround_d(double v) {  // agg::iround
  return (int)((v < 0.0) ? v - 0.5 : v + 0.5);
}
__device__ __forceinline__ void xform(const Mat& m, double& x, double& y) {  // trans_affine::transform
  double t = x;
  x = t * m.sx + y * m.shx + m.tx;
  y = t * m.shy + y * m.sy + m.ty;
}
// floor(a / b) for b > 0, |a| < 2^52: fp64 quotient + exact integer correction.
__device__ __forceinline__ long long floordiv64(long long a, long long b) {
  long long q = (long long)floor((double)a / (double)b);
  long long r = a - q * b;
  if (r < 0) --q;
  else if (r >= b) ++q;
  return q;
}

// --------------------------------------------------------------------------
// wave-level helpers (wave64)
// --------------------------------------------------------------------------
// Issue priority.  Every kernel of a step but the background preparation raises its waves' priority: sampler, geom and raster
// are latency-bound (a few hundred waves that gate their chain), compose is memory-bound (few instructions, long waits) - what
// they can issue should go out at once - while the ALU-bound preparation of the OTHER chains fills the issue slots they leave.
// +2.3 % on the headline step, +2.1 % with the composite objects of config 5 (priority for compose alone: +2.9 % / -0.7 .. -3 %;
// profiles/r04_experiments_log.md section 10).  Without the preparation every wave has the same priority and nothing changes.
__device__ __forceinline__ void step_kernel_priority() { __builtin_amdgcn_s_setprio(3); }
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}
// inclusive prefix sum over the 64 lanes: DPP row shifts + row broadcasts (gfx9 DPP)
__device__ __forceinline__ int wave_scan_incl(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
  return v;
}

// --------------------------------------------------------------------------
// geom_kernel: one WAVE per (shape, frame), four per workgroup.
// Reference: RealizeObjectBlueprint geometry (DG:1073-1117), conv_transform +
// conv_curve feeding rasterizer_scanline_aa::add_path (DG:465-479, 520-534),
// agg::ellipse (100 steps), agg::curve3_div, ras_conv_int::upscale = iround(v*256).
// --------------------------------------------------------------------------
constexpr int kTileW = 64, kTileH = 16, kPx = 4;
constexpr int kChunkW = 128;  // columns one raster item covers
constexpr int kGeomWaves = 1;   // single-wave workgroups: any retiring compose wave makes room for one
constexpr int kCurveSlots = 10;  // a polygon of <= 20 segments holds <= 9 curve3 segments

// curve3_div::recursive_bezier as an explicit depth-first walk (left subtree first).
// Writes the subdivision points followed by the end point to `out` (24.8 fixed point)
// and returns how many.  `stack` holds the pending right halves: the start of a popped
// half is the end of the half just finished, so 4 doubles + the level suffice.
__device__ __forceinline__ int flatten_curve3(double x1, double y1, double x2, double y2, double x3, double y3,
                                              double (*stack)[5], int2* out, int cap, bool* overflow) {
  const double ex = x3, ey = y3;
  const double tol_sq = 0.25;  // (0.5 / approximation_scale)^2
  int cnt = 0, sp = 0, level = 0;
  for (;;) {
    bool subdivide = false;
    if (level <= 32) {  // curve_recursion_limit
      const double x12 = (x1 + x2) / 2, y12 = (y1 + y2) / 2;
      const double x23 = (x2 + x3) / 2, y23 = (y2 + y3) / 2;
      const double x123 = (x12 + x23) / 2, y123 = (y12 + y23) / 2;
      const double dx = x3 - x1, dy = y3 - y1;
      double d = fabs(((x2 - x3) * dy - (y2 - y3) * dx));
      bool emit = false;
      double px = 0, py = 0;
      if (d > 1e-30) {  // curve_collinearity_epsilon
        if (d * d <= tol_sq * (dx * dx + dy * dy)) { emit = true; px = x123; py = y123; }
        else subdivide = true;
      } else {
        const double da = dx * dx + dy * dy;
        bool stop = false;
        if (da == 0) {
          d = (x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1);
        } else {
          d = ((x2 - x1) * dx + (y2 - y1) * dy) / da;
          if (d > 0 && d < 1) stop = true;
          else if (d <= 0) d = (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2);
          else d = (x3 - x2) * (x3 - x2) + (y3 - y2) * (y3 - y2);
        }
        if (!stop) {
          if (d < tol_sq) { emit = true; px = x2; py = y2; }
          else subdivide = true;
        }
      }
      if (emit) {
        if (cnt < cap - 1) out[cnt++] = make_int2(iround_d(px * 256.0), iround_d(py * 256.0));
        else *overflow = true;
      }
      if (subdivide) {
        if (sp < kCurveMaxDepth) {
          double* st = stack[sp++];
          st[0] = x23; st[1] = y23; st[2] = x3; st[3] = y3; st[4] = (double)(level + 1);
          x3 = x123; y3 = y123; x2 = x12; y2 = y12;  // descend into the left half
          ++level;
          continue;
        }
        *overflow = true;
      }
    }
    if (sp == 0) break;
    const double* st = stack[--sp];
    x1 = x3; y1 = y3;  // the right half starts where the left half ended
    x2 = st[0]; y2 = st[1]; x3 = st[2]; y3 = st[3]; level = (int)st[4];
  }
  out[cnt++] = make_int2(iround_d(ex * 256.0), iround_d(ey * 256.0));
  return cnt;
}

// Block masks: for every 64 x 8 block of every sample two 64-bit words (frame 0, frame 1);
// bit k = the (dilated) box of an outline of foreground object k touches the block.  compose
// reads its block's pair with one scalar load and visits exactly these objects.

// A path of up to 64 segments (lane = segment; type 1 = line_to, 3 = curve3 control point followed by its end point,
// segment 0 = the move_to vertex) flattened the way conv_curve + curve3_div do it.  type_of(i) / point(i, x, y) give a
// segment's type and its point in OUTPUT coordinates.  Returns the vertex count; the box is per lane (reduce it).
template <class OutPtr, class TypeFn, class PointFn>
__device__ __forceinline__ int path_verts(int n_seg, TypeFn type_of, PointFn point, OutPtr out, double (*stack)[kCurveMaxDepth][5],
                                          int2 (*stage)[kCurveMaxPts], uint32_t* __restrict__ err, int lane, int& minx, int& miny,
                                          int& maxx, int& maxy) {
  int n_verts = 0;
  // segment i: 0 = the move_to vertex, Line -> 1 vertex, Curve3 -> its flattening
  // (all but the first point), the Dummy after a Curve3 (its end point) -> nothing
  const int t = (lane >= n_seg) ? 0 : (lane == 0 ? 1 : type_of(lane));
  const bool is_curve = (t == 3);
  const unsigned long long cmask = __ballot(is_curve);
  const int slot = __popcll(cmask & ((1ull << lane) - 1ull));
  bool overflow = false;
  int cnt = 0;
  int2 v0 = make_int2(0, 0);
  if (t == 1) {
    double x, y;
    point(lane, x, y);
    v0 = make_int2(iround_d(x * 256.0), iround_d(y * 256.0));
    cnt = 1;
  } else if (is_curve) {
    if (slot < kCurveSlots) {
      // conv_curve: curve3(ctrl = seg[i], to = seg[i+1]) from the current point seg[i-1]
      double x1, y1, x2, y2, x3, y3;
      const int ie = (lane + 1 < n_seg) ? lane + 1 : lane;
      point(lane - 1, x1, y1); point(lane, x2, y2); point(ie, x3, y3);
      cnt = flatten_curve3(x1, y1, x2, y2, x3, y3, stack[slot], stage[slot], kCurveMaxPts, &overflow);
    } else {
      overflow = true;
    }
  }
  const int incl = wave_scan_incl(cnt);
  n_verts = __shfl(incl, 63, 64);
  const int off = incl - cnt;
  if (n_verts > kMaxVerts) {
    if (lane == 0) atomicOr(err, kErrVertCapacity);
    n_verts = 0;
  } else if (t == 1) {
    out[off] = v0;
    minx = v0.x; maxx = v0.x; miny = v0.y; maxy = v0.y;
  } else if (cnt > 0) {
    for (int k = 0; k < cnt; ++k) {
      const int2 v = stage[slot][k];
      out[off + k] = v;
      minx = min(minx, v.x); maxx = max(maxx, v.x);
      miny = min(miny, v.y); maxy = max(maxy, v.y);
    }
  }
  if (overflow) atomicOr(err, kErrCurveCapacity);
  return n_verts;
}

// The flattened outline of one (shape, frame): vertices in 24.8 fixed point written to `out` (global memory or LDS),
// their number and bounding box (wave-reduced).  One wave; lanes = ellipse steps or path segments.
// Reference: agg::ellipse (100 steps), conv_curve / curve3_div, ras_conv_int::upscale = iround(v * 256).
template <class OutPtr>
__device__ __forceinline__ int outline_verts(const DevShape& S, const Mat& M, const double* __restrict__ cs_tab, OutPtr out,
                                             double (*stack)[kCurveMaxDepth][5], int2 (*stage)[kCurveMaxPts],
                                             uint32_t* __restrict__ err, int lane, int& minx, int& miny, int& maxx, int& maxy) {
  int n_verts = 0;
  minx = 0x7FFFFFFF; miny = 0x7FFFFFFF; maxx = (int)0x80000000; maxy = (int)0x80000000;
  if (S.type == 1) {
    // agg::ellipse::vertex: x = cx + cos(angle)*rx with angle = step/100 * 2*pi; the
    // cos/sin table comes from the host's libm so the doubles match the CPU's.
    n_verts = 100;
    for (int k = lane; k < 100; k += 64) {
      double x = 0.0 + cs_tab[2 * k] * (double)S.rx;
      double y = 0.0 + cs_tab[2 * k + 1] * (double)S.ry;
      xform(M, x, y);
      const int2 v = make_int2(iround_d(x * 256.0), iround_d(y * 256.0));
      out[k] = v;
      minx = min(minx, v.x); maxx = max(maxx, v.x);
      miny = min(miny, v.y); maxy = max(maxy, v.y);
    }
  } else {
    n_verts = path_verts(S.n_seg, [&](int i) { return S.seg_type[i]; },
                         [&](int i, double& x, double& y) { x = (double)S.seg_x[i]; y = (double)S.seg_y[i]; xform(M, x, y); },
                         out, stack, stage, err, lane, minx, miny, maxx, maxy);
  }
  minx = wave_min(minx); miny = wave_min(miny); maxx = wave_max(maxx); maxy = wave_max(maxy);
  return n_verts;
}

// LDS of one geom wave: the curve3 stacks and the staging of their points
struct GeomWs {
  double stack[kCurveSlots][kCurveMaxDepth][5];
  int2 stage[kCurveSlots][kCurveMaxPts];
};
// one wave = one (outline, frame) sf
__device__ __forceinline__ void geom_wave(GeomWs& ws, int sf, int lane, const DevShape* __restrict__ shapes, int n_shapes,
                                          const double* __restrict__ cs_tab, int W, int H, DevShapeFrame* __restrict__ frames,
                                          int2* __restrict__ verts, unsigned long long* __restrict__ blockmask, uint32_t* __restrict__ err,
                                          int* __restrict__ item_count, int4* __restrict__ items, const DevCropRef* __restrict__ crops) {
  if (sf >= n_shapes * 2) return;  // wave-uniform
  const DevShape& S = shapes[sf >> 1];
  if (S.type == 0) return;  // unused slot of a device-sampled batch (wave-uniform)
  const Mat M = S.m[sf & 1];
  int2* out = verts + (size_t)sf * kMaxVerts;

  int minx, miny, maxx, maxy;
  int n_verts = outline_verts(S, M, cs_tab, out, ws.stack, ws.stage, err, lane, minx, miny, maxx, maxy);
  // AGG dx_limit: an edge spanning >= 16384 px takes a different code path in
  // rasterizer_cells_aa::line; blueprints never get close, flag it if one does.
  if (n_verts > 0 && ((long long)maxx - (long long)minx >= (16384LL << 8))) {
    if (lane == 0) atomicOr(err, kErrDxLimit);
    n_verts = 0;
  }
  int x0 = minx >> 8, y0 = miny >> 8, x1 = maxx >> 8, y1 = maxy >> 8;
  const bool visible = !(n_verts < 2 || x1 < 0 || y1 < 0 || x0 > W - 1 || y0 > H - 1);
  int bx0 = 1, by0 = 1, bx1 = 0, by1 = 0;  // box compose / raster work with (dilated for deforming shapes)
  if (visible) {
    x0 = max(x0, 0); y0 = max(y0, 0); x1 = min(x1, W - 1); y1 = min(y1, H - 1);
    bx0 = x0; by0 = y0; bx1 = x1; by1 = y1;
    if ((sf & 1) && S.deform > 0) {
      // mode 9: the frame-1 mask is re-sampled through the inverse warp field, so it can
      // reach max |iflow| (+ the bilinear footprint) beyond the outline's box
      const int d = (int)ceilf(__uint_as_float(*crops[S.deform - 1].max_bits)) + 2;
      bx0 = max(x0 - d, 0); by0 = max(y0 - d, 0); bx1 = min(x1 + d, W - 1); by1 = min(y1 + d, H - 1);
    }
  } else {
    x0 = 1; x1 = 0; y0 = 1; y1 = 0;  // nothing on screen
  }
  if (lane == 0) {
    DevShapeFrame f;
    f.n_verts = n_verts;
    f.x0 = x0; f.y0 = y0; f.x1 = x1; f.y1 = y1;
    f.pad[0] = S.sample; f.pad[1] = S.obj_local; f.pad[2] = 0;  // (raster_kernel marks the block masks with these)
    frames[sf] = f;
  }
  // Raster work list: one item per 8-row band x 128-column chunk of the 64 x 8 blocks the
  // (dilated) box touches.  Coverage outside these blocks is never read: compose tests the
  // block against the same box.
  if (visible) {
    const int band0 = by0 / kBandRows, band1 = by1 / kBandRows;
    // Block masks: raster_kernel marks the blocks in which the outline really has coverage.  Only
    // a deforming frame-1 outline (mode 9) is marked here, by its dilated box: its mask is
    // re-sampled from displaced positions.
    if ((sf & 1) && S.deform > 0) {
      const int nbx = (W + kTileW - 1) / kTileW, nby = (H + kBandRows - 1) / kBandRows;
      const int c0 = bx0 / kTileW, nc = bx1 / kTileW - c0 + 1;
      unsigned long long* m = blockmask + ((size_t)S.sample * nbx * nby) * 2 + (sf & 1);
      const unsigned long long bit = 1ull << S.obj_local;
      for (int i = lane; i < (band1 - band0 + 1) * nc; i += 64)
        atomicOr(m + (size_t)((band0 + i / nc) * nbx + c0 + i % nc) * 2, bit);
    }
    const int xa = (bx0 / kTileW) * kTileW, xb = min((bx1 / kTileW) * kTileW + kTileW - 1, W - 1);
    const int nchunks = (xb - xa + kChunkW) / kChunkW;
    const int n_items = (band1 - band0 + 1) * nchunks;
    int base = 0;
    if (lane == 0) base = atomicAdd(item_count, n_items);
    base = __shfl(base, 0, 64);
    for (int i = lane; i < n_items; i += 64) {
      const int b = band0 + i / nchunks, cx = xa + (i % nchunks) * kChunkW;
      items[base + i] = make_int4(sf, b, cx, min(cx + kChunkW - 1, xb));
    }
  }
}

__global__ __launch_bounds__(64 * kGeomWaves) void geom_kernel(const DevShape* __restrict__ shapes, int n_shapes,
                                                   const double* __restrict__ cs_tab, int W, int H,
                                                   DevShapeFrame* __restrict__ frames, int2* __restrict__ verts,
                                                   unsigned long long* __restrict__ blockmask, uint32_t* __restrict__ err,
                                                   int* __restrict__ item_count, int4* __restrict__ items,
                                                   const DevCropRef* __restrict__ crops, int part_sf, uint32_t* __restrict__ err1,
                                                   uint32_t* __restrict__ err2, uint32_t* __restrict__ err3) {
  __shared__ GeomWs s_ws[kGeomWaves];
  step_kernel_priority();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int sf = __builtin_amdgcn_readfirstlane(blockIdx.x * kGeomWaves + wave);
  // (a slot that holds up to four batches of a chain in parts of part_sf outlines: an outline flags in ITS batch's word)
  geom_wave(s_ws[wave], sf, lane, shapes, n_shapes, cs_tab, W, H, frames, verts, blockmask,
            front_pick(sf, part_sf, err, err1, err2, err3), item_count, items, crops);
}

// --------------------------------------------------------------------------
// raster_kernel: persistent workgroups walk the item list; one item = one outline x one
// band of kBandRows scanlines x the padded column range [X0, X1].
//
// AGG's rasterizer_cells_aa walks each edge scanline by scanline and cell by cell
// with incremental lift/rem/mod stepping.  Its per-cell sums of (cover, area) are
// order independent, and the stepping has a closed form (floor of the cumulative
// rational), so every (edge, scanline) pair is processed by its own thread and
// accumulated into LDS with integer atomics.  Column 0 of a row collects the cover
// of all cells left of the column range.
// Then rasterizer_scanline_aa::sweep_scanline: running cover prefix sum per row
// (wavefront DPP scan), alpha = min(|((C << 9) - area) >> 9|, 255) (non-zero rule,
// gamma_none).  The thresholded (gamma_threshold 0.5) mask is alpha >= 128.
// Reference: MovingObjectBase::draw, DG:351-368.
// --------------------------------------------------------------------------
struct CellAcc {
  int* cover;  // [kBandRows][pitch]
  int* area;
  int pitch, X0, X1;
  __device__ __forceinline__ void add(int r, int cell, int dcover, int darea) const {
    if (cell > X1 || dcover == 0) return;  // (darea is a multiple of dcover)
    if (cell < X0) {
      atomicAdd(&cover[r * pitch], dcover);
    } else {
      const int i = r * pitch + (cell - X0 + 1);
      atomicAdd(&cover[i], dcover);
      atomicAdd(&area[i], darea);
    }
  }
};

// ---- 32-bit fast path ---------------------------------------------------------------
// For edges shorter than 8192 px horizontally and 1024 px vertically every product in
// the closed forms fits 32 bits, and all floor divisions can use a float reciprocal
// followed by an exact integer correction.
// floor(num / den), den >= 1, |true quotient| <= 4096: one estimate, one +-1 fix.
__device__ __forceinline__ int fdiv_small(int num, int den, float rcp) {
  int q = (int)floorf((float)num * rcp);
  const int r = num - q * den;
  if (r < 0) --q;
  else if (r >= den) ++q;
  return q;
}
// floor(num / den), den >= 1, |num| < 2^29: two-step estimate (the first remainder is
// small enough for the second estimate to be within one of the truth).
__device__ __forceinline__ int fdiv_big(int num, int den, float rcp) {
  const int q0 = (int)floorf((float)num * rcp);
  const int r0 = num - q0 * den;
  return q0 + fdiv_small(r0, den, rcp);
}

// render_hline in closed form, both directions in one code path.
template <class Acc>
__device__ __forceinline__ void hline32(const Acc& acc, int r, int xa, int ya, int xb, int yb) {
  if (ya == yb) return;
  const int exa = xa >> 8, exb = xb >> 8;
  const int fxa = xa & 255, fxb = xb & 255;
  const int Dy = yb - ya;
  if (exa == exb) {
    acc.add(r, exa, Dy, (fxa + fxb) * Dy);
    return;
  }
  const int lo = min(exa, exb), hi = max(exa, exb);
  if (hi < acc.X0) { acc.add(r, acc.X0 - 1, Dy, 0); return; }  // entirely left: only its cover counts
  if (lo > acc.X1) return;                                      // entirely right: no effect
  const bool right = xb > xa;
  const int adx = right ? xb - xa : xa - xb;
  const float rcp = __frcp_rn((float)adx);
  const int m = hi - lo;
  const int f0 = right ? 256 - fxa : fxa;
  const int j_lo = right ? max(0, acc.X0 - exa) : max(0, exa - acc.X1);
  const int j_hi = right ? min(m, acc.X1 - exa) : min(m, exa - acc.X0);
  // y where the hline enters cell j (j = 1..m): ya + floor((f0 + 256 (j-1)) Dy / adx)
  int yprev = (j_lo == 0) ? ya : ya + fdiv_small((f0 + 256 * (j_lo - 1)) * Dy, adx, rcp);
  if (right && j_lo > 0) acc.add(r, acc.X0 - 1, yprev - ya, 0);  // cells left of the range
  for (int j = j_lo; j <= j_hi; ++j) {
    const int ynext = (j == m) ? yb : ya + fdiv_small((f0 + 256 * j) * Dy, adx, rcp);
    const int d = ynext - yprev;
    const int fin = (j == 0) ? fxa : (right ? 0 : 256);
    const int fout = (j == m) ? fxb : (right ? 256 : 0);
    acc.add(r, right ? exa + j : exa - j, d, (fin + fout) * d);
    yprev = ynext;
  }
  if (!right && j_hi < m) acc.add(r, acc.X0 - 1, yb - yprev, 0);  // what remains lies left of the range
}

// rasterizer_cells_aa::render_hline(ey, xa, ya, xb, yb) in closed form.
template <class Acc>
__device__ __forceinline__ void hline(const Acc& acc, int r, int xa, int ya, int xb, int yb) {
  if (ya == yb) return;
  const int exa = xa >> 8, exb = xb >> 8;
  const int fxa = xa & 255, fxb = xb & 255;
  const int Dy = yb - ya;
  if (exa == exb) {
    acc.add(r, exa, Dy, (fxa + fxb) * Dy);
    return;
  }
  if (xb > xa) {
    const int m = exb - exa;
    const long long dxh = xb - xa;
    const long long f0 = 256 - fxa;
    int j = 0;
    int yprev = ya;
    // cells left of the bbox only contribute their total cover
    if (exa < acc.X0) {
      const int jb = min(acc.X0 - exa, m + 1);  // first cell index that is inside (or past the end)
      // y at the left boundary of cell exa+jb (or yb if the hline ends before it)
      int yb0 = (jb > m) ? yb : ya + (int)floordiv64((f0 + 256LL * (jb - 1)) * Dy, dxh);
      acc.add(r, acc.X0 - 1, yb0 - ya, 0);
      yprev = yb0;
      j = jb;
    }
    for (; j <= m; ++j) {
      const int cell = exa + j;
      if (cell > acc.X1) break;
      const int ynext = (j == m) ? yb : ya + (int)floordiv64((f0 + 256LL * j) * Dy, dxh);
      const int d = ynext - yprev;
      const int fin = (j == 0) ? fxa : 0;
      const int fout = (j == m) ? fxb : 256;
      acc.add(r, cell, d, (fin + fout) * d);
      yprev = ynext;
    }
  } else {
    const int m = exa - exb;
    const long long dxh = xa - xb;
    const long long f0 = fxa;
    // walking leftwards: cells right of X1 are skipped, cells left of X0 are lumped
    int j = 0;
    int yprev = ya;
    if (exa > acc.X1) {
      const int jb = min(exa - acc.X1, m + 1);
      yprev = (jb > m) ? yb : ya + (int)floordiv64((f0 + 256LL * (jb - 1)) * Dy, dxh);
      j = jb;
    }
    for (; j <= m; ++j) {
      const int cell = exa - j;
      if (cell < acc.X0) {
        acc.add(r, acc.X0 - 1, yb - yprev, 0);  // everything that remains, in one go
        break;
      }
      const int ynext = (j == m) ? yb : ya + (int)floordiv64((f0 + 256LL * j) * Dy, dxh);
      const int d = ynext - yprev;
      const int fin = (j == 0) ? fxa : 256;
      const int fout = (j == m) ? fxb : 0;
      acc.add(r, cell, d, (fin + fout) * d);
      yprev = ynext;
    }
  }
}

// rasterizer_cells_aa::line restricted to scanline y (closed form of the stepping).
template <class Acc>
__device__ __forceinline__ void edge_scanline(const Acc& acc, int r, int y, int x1, int y1, int x2, int y2) {
  const int ey1 = y1 >> 8, ey2 = y2 >> 8;
  const int fy1 = y1 & 255, fy2 = y2 & 255;
  {
    const int dxi = x2 - x1, dyi = y2 - y1;
    const int adx = dxi < 0 ? -dxi : dxi, ady = dyi < 0 ? -dyi : dyi;
    if (adx < (1 << 21) && ady < (1 << 18)) {  // 32-bit fast path (virtually every edge)
      if (ey1 == ey2) {
        if (y == ey1) hline32(acc, r, x1, fy1, x2, fy2);
        return;
      }
      const bool up = dyi < 0;
      if (y < min(ey1, ey2) || y > max(ey1, ey2)) return;
      const int k = up ? ey1 - y : y - ey1;
      const bool last = (y == ey2);
      const float rcp = __frcp_rn((float)ady);
      // X(k) = x1 + floor((base + 256 (k-1)) dx / |dy|)
      //      = x1 + d1 + (k-1) lift + floor((m1 + (k-1) rem) / |dy|)   (exact identity)
      const int p1 = (up ? fy1 : 256 - fy1) * dxi;
      const int d1 = fdiv_big(p1, ady, rcp), m1 = p1 - d1 * ady;
      const int lift = fdiv_big(256 * dxi, ady, rcp), rem = 256 * dxi - lift * ady;
      const int xa = (k == 0) ? x1 : x1 + d1 + (k - 1) * lift + fdiv_small(m1 + (k - 1) * rem, ady, rcp);
      const int xb = last ? x2 : x1 + d1 + k * lift + fdiv_small(m1 + k * rem, ady, rcp);
      const int ya = (k == 0) ? fy1 : (up ? 256 : 0);
      const int yb = last ? fy2 : (up ? 0 : 256);
      hline32(acc, r, xa, ya, xb, yb);
      return;
    }
  }
  if (ey1 == ey2) {
    if (y == ey1) hline(acc, r, x1, fy1, x2, fy2);
    return;
  }
  const long long dx = x2 - x1;
  if (y2 > y1) {
    if (y < ey1 || y > ey2) return;
    const long long dy = y2 - y1;
    const int k = y - ey1;
    const int xa = (k == 0) ? x1 : x1 + (int)floordiv64(((256 - fy1) + 256LL * (k - 1)) * dx, dy);
    const int ya = (k == 0) ? fy1 : 0;
    const int xb = (y == ey2) ? x2 : x1 + (int)floordiv64(((256 - fy1) + 256LL * k) * dx, dy);
    const int yb = (y == ey2) ? fy2 : 256;
    hline(acc, r, xa, ya, xb, yb);
  } else {
    if (y > ey1 || y < ey2) return;
    const long long dy = y1 - y2;
    const int k = ey1 - y;
    const int xa = (k == 0) ? x1 : x1 + (int)floordiv64((fy1 + 256LL * (k - 1)) * dx, dy);
    const int ya = (k == 0) ? fy1 : 256;
    const int xb = (y == ey2) ? x2 : x1 + (int)floordiv64((fy1 + 256LL * k) * dx, dy);
    const int yb = (y == ey2) ? fy2 : 0;
    hline(acc, r, xa, ya, xb, yb);
  }
}

struct ChunkAcc {
  int* cover;  // [kBandRows][kChunkW]
  int* area;
  int* carry;  // [kBandRows]: cover of all cells left of the chunk
  int X0, X1;
  __device__ __forceinline__ void add(int r, int cell, int dcover, int darea) const {
    if (cell > X1 || dcover == 0) return;  // (darea is a multiple of dcover)
    if (cell < X0) {
      atomicAdd(&carry[r], dcover);
    } else {
      const int i = r * kChunkW + (cell - X0);
      atomicAdd(&cover[i], dcover);
      atomicAdd(&area[i], darea);
    }
  }
};

constexpr int kRasterWaves = 1;
struct ChunkCells {
  int cover[kBandRows][kChunkW];
  int area[kBandRows][kChunkW];
  int carry[kBandRows];
};

// LDS of one rasterising wave
struct RasterWs {
  ChunkCells cells;
  int queue[64 * kBandRows];
};

// One item = one outline x one band of kBandRows scanlines x the padded column range [X0, X1], by ONE wave (no
// workgroup barriers): clear its cells, accumulate every (edge, scanline) pair of the outline that can reach the
// chunk, sweep, store the coverage bytes, mark the block masks.  v: the outline's nv vertices; F*: its pixel box.
// pa, pb: v[lane] and v[lane + 1], requested by the caller while the previous item was being rasterised.
__device__ __forceinline__ void raster_item(RasterWs& ws, const int2* __restrict__ v, int nv, int Fx0, int Fy0, int Fx1, int Fy1, int sf,
                                            int band, int X0, int X1, int W, int H, uint8_t* __restrict__ cov,
                                            unsigned long long* __restrict__ blockmask, int sample, int obj_local, int lane, int2 pa, int2 pb) {
  ChunkCells& tc = ws.cells;
  const int by0 = band * kBandRows;
  const int rows = min(kBandRows, H - by0);
  const bool has_edges = (Fx0 <= Fx1) && (by0 <= Fy1) && (by0 + kBandRows - 1 >= Fy0) && (Fx0 <= X1) && (Fx1 >= X0);
  uint8_t* dst = cov + ((size_t)sf * H + by0) * W + X0;
  const int c2 = 2 * lane;  // this lane's two columns of the chunk
  const bool in_range = (X0 + c2) <= X1;  // X0 is even and X1 odd (tile-aligned, W % 4 == 0)
  if (!has_edges) {
    if (in_range)
      for (int r = 0; r < rows; ++r) *reinterpret_cast<uint16_t*>(dst + (size_t)r * W + c2) = 0;
    return;
  }
  {  // clear
    int4* z = reinterpret_cast<int4*>(&tc);
    const int n16 = (2 * kBandRows * kChunkW) / 4;
    for (int i = lane; i < n16; i += 64) z[i] = make_int4(0, 0, 0, 0);
    if (lane < kBandRows) tc.carry[lane] = 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  ChunkAcc acc;
  acc.cover = &tc.cover[0][0]; acc.area = &tc.area[0][0]; acc.carry = &tc.carry[0];
  acc.X0 = X0; acc.X1 = X1;
  // Lane = edge: find the scanlines of the band each edge crosses, compact the
  // (edge, scanline) pairs that can reach the chunk into a dense queue, then let
  // all 64 lanes work on real pairs.  The closing edge (last -> first) is edge nv-1.
  int* queue = ws.queue;
  for (int e0 = 0; e0 < nv; e0 += 64) {
    const int e = e0 + lane;
    int n_rows = 0, rlo = 0;
    // this lane's edge (a -> b); the first 64 edges' vertices are in hand already
    int2 a = pa, b = pb;
    if (e0 > 0 && e < nv) { a = v[e]; b = v[(e + 1 == nv) ? 0 : e + 1]; }  // (never past the outline's slot: nv may be kMaxVerts)
    {
      const int v0x = __shfl(pa.x, 0, 64), v0y = __shfl(pa.y, 0, 64);  // the closing edge ends at vertex 0
      if (e + 1 == nv) b = make_int2(v0x, v0y);
    }
    if (e < nv) {
      const int eya = a.y >> 8, eyb = b.y >> 8;
      rlo = max(min(eya, eyb), by0);
      const int rhi = min(max(eya, eyb), by0 + rows - 1);
      if (rhi >= rlo && (min(a.x, b.x) >> 8) <= X1 && a.y != b.y) n_rows = rhi - rlo + 1;
    }
    const int incl = wave_scan_incl(n_rows);
    const int total = __shfl(incl, 63, 64);
    int at = incl - n_rows;
    for (int k = 0; k < n_rows; ++k) queue[at++] = (e << 4) | (rlo + k - by0);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    for (int q0 = 0; q0 < total; q0 += 64) {
      const int q = q0 + lane;
      const int code = (q < total) ? queue[q] : (e0 << 4);
      const int src = (code >> 4) - e0, r = code & 15;   // the pair's edge sits in lane `src` of this block: no second trip to memory
      const int ax = __shfl(a.x, src, 64), ay = __shfl(a.y, src, 64), bx = __shfl(b.x, src, 64), by = __shfl(b.y, src, 64);
      if (q < total) edge_scanline(acc, r, by0 + r, ax, ay, bx, by);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  // sweep: lane l owns columns 2l, 2l+1 of every row
  int nonzero = 0;
  for (int r = 0; r < rows; ++r) {
    const int2 cv = *reinterpret_cast<const int2*>(&tc.cover[r][c2]);
    const int2 ar = *reinterpret_cast<const int2*>(&tc.area[r][c2]);
    const int s2 = cv.x + cv.y;
    const int base = tc.carry[r] + wave_scan_incl(s2) - s2;
    int a0 = ((base + cv.x) << 9) - ar.x, a1 = ((base + s2) << 9) - ar.y;  // calculate_alpha (shift 9)
    a0 >>= 9; a1 >>= 9;
    a0 = a0 < 0 ? -a0 : a0; a1 = a1 < 0 ? -a1 : a1;
    a0 = a0 > 255 ? 255 : a0; a1 = a1 > 255 ? 255 : a1;
    if (in_range) { *reinterpret_cast<uint16_t*>(dst + (size_t)r * W + c2) = (uint16_t)(a0 | (a1 << 8)); nonzero |= a0 | a1; }
  }
  // lanes 0-31 hold the left 64 x 8 block of the chunk, lanes 32-63 the right one
  const unsigned long long nz = __ballot(nonzero != 0);
  if (blockmask) {
    // compose visits an object in a 64 x 8 block only if its outline has coverage there
    const int half = lane >> 5;
    if ((lane & 31) == 0 && ((nz >> (32 * half)) & 0xFFFFFFFFull)) {
      const int nbx = (W + kTileW - 1) / kTileW, nby = (H + kBandRows - 1) / kBandRows;
      atomicOr(blockmask + ((size_t)(sample * nby + band) * nbx + (X0 / kTileW + half)) * 2 + (sf & 1), 1ull << obj_local);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // reads done before the next item's clear
}

// raster_kernel: persistent single-wave workgroups walk geom_kernel's item list.
__global__ __launch_bounds__(64 * kRasterWaves) void raster_kernel(const DevShapeFrame* __restrict__ frames,
                                                     const int4* __restrict__ items,
                                                     const int* __restrict__ item_count,
                                                     const int2* __restrict__ verts, int W, int H,
                                                     uint8_t* __restrict__ cov,
                                                     unsigned long long* __restrict__ blockmask_next, int n_mask_words,
                                                     unsigned long long* __restrict__ blockmask) {
  __shared__ __attribute__((aligned(16))) RasterWs s_ws[kRasterWaves];
  step_kernel_priority();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // clear the block masks the NEXT launch of this slot accumulates into (the other parity)
  for (int gid = blockIdx.x * blockDim.x + threadIdx.x; gid < n_mask_words; gid += gridDim.x * blockDim.x) blockmask_next[gid] = 0ull;
  const int n_items = *item_count;
  const int n_waves = gridDim.x * kRasterWaves;
  // An item is three dependent trips to memory before its first instruction of work (the item, its outline's record, the
  // vertices): the loop is a software pipeline - item k + 2, the record of item k + 1 and its first 64 vertices are requested
  // before item k is rasterised.  The work list and the records are constant while this kernel runs (scalar loads).
  typedef OFDG_CONSTANT const int4 ConstItem;
  typedef OFDG_CONSTANT const DevShapeFrame ConstFrame;
  int it = __builtin_amdgcn_readfirstlane(blockIdx.x * kRasterWaves + wave);
  if (it >= n_items) return;
  // (what is carried around the loop is a per-lane value to the compiler: readfirstlane says "uniform" again)
  struct Item { int sf, band, X0, X1; };
  struct Frame { int nv, x0, y0, x1, y1, sample, obj_local; };
  auto item_at = [&](int i) {
    const int4 q = ((ConstItem*)items)[i];
    return Item{q.x, q.y, q.z, q.w};
  };
  auto frame_of = [&](int sf) {
    const ConstFrame& f = ((ConstFrame*)frames)[sf];
    return Frame{f.n_verts, f.x0, f.y0, f.x1, f.y1, f.pad[0], f.pad[1]};
  };
  auto uni = [](int x) { return __builtin_amdgcn_readfirstlane(x); };
  int it1 = it + n_waves;
  Item I0 = item_at(it), I1 = item_at(it1 < n_items ? it1 : it);
  Frame F0 = frame_of(I0.sf);
  int2 pa = verts[(size_t)I0.sf * kMaxVerts + lane], pb = verts[(size_t)I0.sf * kMaxVerts + lane + 1];
  for (;;) {
    I0 = Item{uni(I0.sf), uni(I0.band), uni(I0.X0), uni(I0.X1)};
    I1 = Item{uni(I1.sf), uni(I1.band), uni(I1.X0), uni(I1.X1)};
    F0 = Frame{uni(F0.nv), uni(F0.x0), uni(F0.y0), uni(F0.x1), uni(F0.y1), uni(F0.sample), uni(F0.obj_local)};
    it1 = uni(it1);
    const int it2 = it1 + n_waves;
    const Item I2 = item_at(it2 < n_items ? it2 : it1 < n_items ? it1 : it);
    const Frame F1 = frame_of(I1.sf);
    const int2 na = verts[(size_t)I1.sf * kMaxVerts + lane], nb = verts[(size_t)I1.sf * kMaxVerts + lane + 1];
    raster_item(s_ws[wave], verts + (size_t)I0.sf * kMaxVerts, F0.nv, F0.x0, F0.y0, F0.x1, F0.y1, I0.sf, I0.band, I0.X0, I0.X1, W, H, cov, blockmask,
                F0.sample, F0.obj_local, lane, pa, pb);
    if (it1 >= n_items) break;
    I0 = I1; F0 = F1; I1 = I2; pa = na; pb = nb;
    it = it1; it1 = it2;
  }
}

// --------------------------------------------------------------------------
// compose_kernel
// --------------------------------------------------------------------------
// pixfmt_gray8 solid blend of colour 255 onto a cleared buffer (AGG 2.4): the AA mask byte.
__device__ __forceinline__ int aa_byte(int c) { return c == 255 ? 255 : (255 * c) >> 8; }
// floor(a / 255) for 0 <= a <= 65025
__device__ __forceinline__ int div255(int a) { return (a + 1 + (a >> 8)) >> 8; }
// CImg::draw_image(sprite, mask, 1, 255): d = floor((m*s + (255-m)*d) / 255)
__device__ __forceinline__ int blend(int d, int s, int m) { return div255(m * s + (255 - m) * d); }

// The same blend on a packed B | G<<8 | R<<16 pixel: B and R share one multiply-add
// (16-bit lanes: m*s + (255-m)*d <= 65025 never carries), G goes alone.
__device__ __forceinline__ uint32_t blend_px(uint32_t d, uint32_t s, uint32_t m) {
  const uint32_t im = 255u - m;
  uint32_t rb = m * (s & 0x00FF00FFu) + im * (d & 0x00FF00FFu);
  uint32_t g = m * ((s >> 8) & 255u) + im * ((d >> 8) & 255u);
  rb = ((rb + 0x00010001u + ((rb >> 8) & 0x00FF00FFu)) >> 8) & 0x00FF00FFu;  // floor(x / 255) per lane
  g = (g + 1u + (g >> 8)) >> 8;
  return rb | (g << 8);
}

// MovingObjectComposite::renderMasks, strict fp32 (DG:606, 626)
// (float)u / 255.f, correctly rounded, for a byte u: the product with rn(1/255) is wrong for 126 of the 256 bytes, one
// Newton step on it (exact residual through an fma) is right for all of them (tests: the exhaustive byte-formula test
// against the oracle's division; tools/check_q255.py derives it).  3 VALU instructions instead of the ~10 of a division -
// a composite evaluates 32 of these per component and pixel quad.
__device__ __forceinline__ float byte_over_255(int u) {
  const float fu = (float)u, c = 0x1.010102p-8f;  // rn(1 / 255)
  const float q0 = __fmul_rn(fu, c);
  return __fmaf_rn(__fmaf_rn(-q0, 255.f, fu), c, q0);
}
__device__ __forceinline__ int comp_add(int u, int v) {
  const float fu = byte_over_255(u), fv = byte_over_255(v);
  const float t = __fmul_rn(__fsub_rn(1.f, fu), __fsub_rn(1.f, fv));
  return (int)(unsigned char)__fmul_rn(255.f, __fsub_rn(1.f, t));
}
__device__ __forceinline__ int comp_sub(int u, int v) {
  const float fu = byte_over_255(u), fv = byte_over_255(v);
  return (int)(unsigned char)__fmul_rn(255.f, __fmul_rn(fu, __fsub_rn(1.f, fv)));
}

// --------------------------------------------------------------------------
// Load helpers of the texture warps
// --------------------------------------------------------------------------
// a wave-uniform pointer the compiler can see is uniform (SGPR pair): loads take it as scalar base + 32-bit lane offset
template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}
// ... and the loads through it name the GLOBAL address space (a pointer rebuilt from integers is generic: flat_load with a
// 64-bit address per lane; as global memory it is global_load v, voffset32, s[base])
typedef __attribute__((address_space(1))) const u32x2 g_uint2;
typedef __attribute__((address_space(1))) const uint32_t g_uint32;
typedef __attribute__((address_space(1))) const char g_char;
__device__ __forceinline__ uint2 gload2(const char* base, uint32_t off) {
  asm("" : "+v"(off));  // (the offset stays a 32-bit VGPR: a select folded into a 64-bit phi would defeat the saddr form)
  const u32x2 v = *(g_uint2*)((g_char*)base + off);
  return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint32_t gload1(const char* base, uint32_t off) { return *(g_uint32*)((g_char*)base + off); }
// span_interpolator_linear::begin + dda2_line_interpolator for one output row.
struct RowDDA {
  int x1, lx, rx;  // start, lft, rem (rem in [1, n])
  int y1, ly, ry;
};
template <bool kPow2 = false>
__device__ __forceinline__ void dda_setup(int a, int b, int n, int nshift, int& lft, int& rem) {
  const int D = b - a;
  if (kPow2 || nshift >= 0) {  // n is a power of two (wave-uniform): floor quotient / remainder by shifts
    const int q = D >> nshift, r = D & (n - 1);
    lft = r > 0 ? q : q - 1;  // dda2_line_interpolator: rem in [1, n]
    rem = r > 0 ? r : n;
  } else {
    lft = D / n;
    rem = D % n;
    if (rem <= 0) { rem += n; lft--; }
  }
}
template <bool kPow2 = false>
__device__ __forceinline__ RowDDA make_row(const Mat& inv, int row, int len, int nshift) {
  RowDDA R;
  double tx = 0 + 0.5, ty = row + 0.5;
  xform(inv, tx, ty);
  R.x1 = iround_d(tx * 256.0);
  R.y1 = iround_d(ty * 256.0);
  tx = 0 + 0.5 + len; ty = row + 0.5;
  xform(inv, tx, ty);
  const int x2 = iround_d(tx * 256.0), y2 = iround_d(ty * 256.0);
  dda_setup<kPow2>(R.x1, x2, len, nshift, R.lx, R.rx);
  dda_setup<kPow2>(R.y1, y2, len, nshift, R.ly, R.ry);
  return R;
}
// value of the interpolator after i increments
template <bool kPow2 = false>
__device__ __forceinline__ int dda_at(int y1, int lft, int rem, int n, int nshift, int i) {
  const int a = (i + 1) * rem + n - 1;
  const int q = (kPow2 || nshift >= 0) ? (a >> nshift) : (a / n);
  return y1 + i * lft + q - 1;
}
template <bool kPow2 = false>
__device__ __forceinline__ int wrap_reflect(int v, int size, int size2, int mask2, int& raw) {
  int m;
  if (kPow2 || mask2 >= 0) {  // power-of-two period (wave-uniform)
    m = v & mask2;
  } else if ((unsigned)(v + size2) < 3u * (unsigned)size2) {  // within one period of the image: no division
    m = v;
    if (m < 0) m += size2;
    if (m >= size2) m -= size2;
  } else {
    m = v % size2;
    if (m < 0) m += size2;
  }
  raw = m;
  return m >= size ? size2 - 1 - m : m;
}
__device__ __forceinline__ int wrap_next(int raw, int size, int size2) {
  int m = raw + 1;
  if (m >= size2) m = 0;
  return m >= size ? size2 - 1 - m : m;
}

struct WarpGeom {
  int tw, th;        // texture size the warp runs on (fg: W x H, bg: 2W x 2H)
  int tw2, th2;      // 2 * size
  int mx2, my2;      // size2 - 1 if power of two else -1
  int nshift;        // log2(tw) if power of two else -1
  int pitch;         // pool image pitch in texels
};

// span_image_filter_rgb_bilinear with wrap_mode_reflect: returns packed B | G<<8 | R<<16.
template <bool kPow2 = false>
__device__ __forceinline__ uint32_t sample_bilinear(const uint32_t* __restrict__ tex, const WarpGeom& g,
                                                    const RowDDA& R, int i) {
  int x_hr = dda_at<kPow2>(R.x1, R.lx, R.rx, g.tw, g.nshift, i) - 128;
  int y_hr = dda_at<kPow2>(R.y1, R.ly, R.ry, g.tw, g.nshift, i) - 128;
  const int x_lr = x_hr >> 8, y_lr = y_hr >> 8;
  x_hr &= 255; y_hr &= 255;
  int rx, ry;
  const int xa = wrap_reflect<kPow2>(x_lr, g.tw, g.tw2, g.mx2, rx);  // (the width's period is a power of two with it)
  const int ya = wrap_reflect(y_lr, g.th, g.th2, g.my2, ry);
  const int xb = wrap_next(rx, g.tw, g.tw2);
  const int yb = wrap_next(ry, g.th, g.th2);
  const uint32_t ra = (uint32_t)(ya * g.pitch), rb = (uint32_t)(yb * g.pitch);
  const uint32_t p00 = tex[ra + (uint32_t)xa];
  const uint32_t p10 = tex[ra + (uint32_t)xb];
  const uint32_t p01 = tex[rb + (uint32_t)xa];
  const uint32_t p11 = tex[rb + (uint32_t)xb];
  const uint32_t w00 = (256 - x_hr) * (256 - y_hr), w10 = x_hr * (256 - y_hr);
  const uint32_t w01 = (256 - x_hr) * y_hr, w11 = x_hr * y_hr;
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sh = 8 * c;
    uint32_t fg = 32768u + w00 * ((p00 >> sh) & 255u) + w10 * ((p10 >> sh) & 255u) +
                  w01 * ((p01 >> sh) & 255u) + w11 * ((p11 >> sh) & 255u);
    out |= (fg >> 16) << sh;
  }
  return out;
}

// The same filter for kPx consecutive pixels of one row.  kPow2 (the row length is a power of
// two, e.g. 512 or 1024): the interpolators advance by additions, and when every needed lane
// of the wave stays inside the texture (no reflection: checked at the two end pixels, the
// interpolators are monotone) the four taps of a pixel are two 8-byte loads.  Otherwise, and
// for other row lengths, sample_bilinear.
__device__ __forceinline__ uint32_t bilerp_rgb(uint2 t0, uint2 t1, uint32_t xf, uint32_t yf) {
  // sum w_ij * p_ij with w = (256 - xf | xf) * (256 - yf | yf): vertical pass on 16-bit lanes
  // (B and R share a multiply: (256 - yf) * a + yf * b <= 65280), horizontal pass per channel
  const uint32_t ify = 256u - yf, ifx = 256u - xf;
  const uint32_t rb0 = (t0.x & 0x00FF00FFu) * ify + (t1.x & 0x00FF00FFu) * yf;
  const uint32_t rb1 = (t0.y & 0x00FF00FFu) * ify + (t1.y & 0x00FF00FFu) * yf;
  const uint32_t g0 = ((t0.x >> 8) & 255u) * ify + ((t1.x >> 8) & 255u) * yf;
  const uint32_t g1 = ((t0.y >> 8) & 255u) * ify + ((t1.y >> 8) & 255u) * yf;
  const uint32_t b = (rb0 & 0xFFFFu) * ifx + (rb1 & 0xFFFFu) * xf + 32768u;
  const uint32_t r = (rb0 >> 16) * ifx + (rb1 >> 16) * xf + 32768u;
  const uint32_t g = g0 * ifx + g1 * xf + 32768u;
  return (b >> 16) | ((g >> 8) & 0xFF00u) | (r & 0xFF0000u);
}
// CImg<float>::_linear_atXY (Neumann): clamp, nx = dx > 0 ? x+1 : x, fp32 polynomial.
template <class Ptr>
__device__ __forceinline__ float linear_neumann(Ptr img, int w, int h, float fx, float fy) {
  const float nfx = fx <= 0 ? 0 : (fx >= (float)(w - 1) ? (float)(w - 1) : fx);
  const float nfy = fy <= 0 ? 0 : (fy >= (float)(h - 1) ? (float)(h - 1) : fy);
  const unsigned x = (unsigned)nfx, y = (unsigned)nfy;
  const float dx = nfx - (float)x, dy = nfy - (float)y;
  const unsigned nx = dx > 0 ? x + 1 : x, ny = dy > 0 ? y + 1 : y;
  const float Icc = img[(size_t)y * w + x], Inc = img[(size_t)y * w + nx];
  const float Icn = img[(size_t)ny * w + x], Inn = img[(size_t)ny * w + nx];
  return Icc + dx * (Inc - Icc + dy * (Icc + Inn - Icn - Inc)) + dy * (Icn - Icc);
}

// ---- mode 9 helpers: CImg<unsigned char>::linear_atXY(fx, fy, 0, c, 0) (Dirichlet), fp32 ----
struct Taps {
  int x, y;      // integer tap (x, y); the others are x+1 / y+1
  float dx, dy;  // fractions
  bool ok;       // false: NaN displacement -> the result is 0 (SURVEY F-9)
};
__device__ __forceinline__ Taps make_taps(float fx, float fy) {
  Taps t;
  t.ok = (fx == fx) && (fy == fy) && fabsf(fx) < 1e8f && fabsf(fy) < 1e8f;
  if (!t.ok) { fx = 0.f; fy = 0.f; }
  t.x = (int)fx - (fx >= 0 ? 0 : 1);
  t.y = (int)fy - (fy >= 0 ? 0 : 1);
  t.dx = fx - (float)t.x;
  t.dy = fy - (float)t.y;
  return t;
}
__device__ __forceinline__ int lerp_u8(const Taps& t, float Icc, float Inc, float Icn, float Inn) {
  const float v = Icc + t.dx * (Inc - Icc + t.dy * (Icc + Inn - Icn - Inc)) + t.dy * (Icn - Icc);
  return t.ok ? (int)(unsigned char)v : 0;
}

// Warp crops as the kernels read them: two interleaved planes of w*h float pairs - (flow x, flow y), then
// (iflow x, iflow y) - so that a pixel's displacement is ONE 8-byte load.
__device__ __forceinline__ float2 crop_pair(const DevCropRef& C, int plane_pair, int x, int y) {
  const f32x2 v = *(OFDG_GLOBAL const f32x2*)(C.data + ((size_t)plane_pair * C.w * C.h + (size_t)y * C.w + x) * 2);
  return make_float2(v.x, v.y);
}
// CImg<float>::_linear_atXY (Neumann) of both components of the forward field at once (four 8-byte taps)
__device__ __forceinline__ float2 linear_neumann2(const DevCropRef& C, float fx, float fy) {
  const int w = C.w, h = C.h;
  const float nfx = fx <= 0 ? 0 : (fx >= (float)(w - 1) ? (float)(w - 1) : fx);
  const float nfy = fy <= 0 ? 0 : (fy >= (float)(h - 1) ? (float)(h - 1) : fy);
  const unsigned x = (unsigned)nfx, y = (unsigned)nfy;
  const float dx = nfx - (float)x, dy = nfy - (float)y;
  const unsigned nx = dx > 0 ? x + 1 : x, ny = dy > 0 ? y + 1 : y;
  const float2 Icc = crop_pair(C, 0, (int)x, (int)y), Inc = crop_pair(C, 0, (int)nx, (int)y);
  const float2 Icn = crop_pair(C, 0, (int)x, (int)ny), Inn = crop_pair(C, 0, (int)nx, (int)ny);
  return make_float2(Icc.x + dx * (Inc.x - Icc.x + dy * (Icc.x + Inn.x - Icn.x - Inc.x)) + dy * (Icn.x - Icc.x),
                     Icc.y + dx * (Inc.y - Icc.y + dy * (Icc.y + Inn.y - Icn.y - Inc.y)) + dy * (Icn.y - Icc.y));
}
// applyWarpFieldToTexture(getTransformedTexture(tex, motion), iwarp) for one pixel (DG:237-252, 341-345, 670-678): the
// four texels of the TRANSFORMED texture around the displaced position t (each a bilinear filter of the source through
// the inverse motion `inv`; Dirichlet 0 outside the tw x th texture), then CImg's fp32 lerp per channel.  While every
// source tap of every lane that needs one lies inside the texture the eight tap pairs of a pixel are eight 8-byte loads
// issued together; otherwise the general interpolator (reflection), sample by sample.
template <bool kPow2>
__device__ __forceinline__ uint32_t deform_texel(const uint32_t* __restrict__ tex_, const WarpGeom& g, const Mat& inv, const Taps& t, bool need) {
  const uint32_t* __restrict__ tex = uniform_ptr(tex_);
  uint32_t tap[4] = {0, 0, 0, 0};
  int xh[4], yh[4];
  bool valid[4];
  RowDDA R[2];
  bool fast = true;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ty = t.y + j;
    const bool row_ok = need && t.ok && ty >= 0 && ty < g.th;
    R[j] = make_row<kPow2>(inv, row_ok ? ty : 0, g.tw, g.nshift);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int tx = t.x + i, k = 2 * j + i;
      valid[k] = row_ok && tx >= 0 && tx < g.tw;
      xh[k] = dda_at<kPow2>(R[j].x1, R[j].lx, R[j].rx, g.tw, g.nshift, valid[k] ? tx : 0) - 128;
      yh[k] = dda_at<kPow2>(R[j].y1, R[j].ly, R[j].ry, g.tw, g.nshift, valid[k] ? tx : 0) - 128;
      const bool in_range = (unsigned)(xh[k] >> 8) <= (unsigned)(g.tw - 2) && (unsigned)(yh[k] >> 8) <= (unsigned)(g.th - 2);
      fast = fast && (!valid[k] || in_range);
    }
  }
  if (__ballot(!fast) == 0ull) {
    const char* base = reinterpret_cast<const char*>(tex);
    const char* base1 = uniform_ptr(base + (size_t)g.pitch * 4u);
    uint2 t0[4], t1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t off = valid[k] ? ((uint32_t)(yh[k] >> 8) * (uint32_t)g.pitch + (uint32_t)(xh[k] >> 8)) * 4u : 0u;
      t0[k] = gload2(base, off);
      t1[k] = gload2(base1, off);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tap[k] = valid[k] ? bilerp_rgb(t0[k], t1[k], (uint32_t)xh[k] & 255u, (uint32_t)yh[k] & 255u) : 0u;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) tap[k] = valid[k] ? sample_bilinear<kPow2>(tex, g, R[k >> 1], t.x + (k & 1)) : 0u;
  }
  uint32_t o = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sh = 8 * c;
    o |= (uint32_t)lerp_u8(t, (float)((tap[0] >> sh) & 255u), (float)((tap[1] >> sh) & 255u),
                           (float)((tap[2] >> sh) & 255u), (float)((tap[3] >> sh) & 255u)) << sh;
  }
  return o;
}

struct Taps4 {
  uint2 t0[kPx], t1[kPx];  // texel pairs of the two rows (mode 2: t0[p].x = the finished pixel)
  uint32_t xf, yf;         // fractions, byte p = pixel p
  int mode;                // 0 paired loads, 1 reflected single loads, 2 general interpolator (nothing issued)
};
// the four frame-1 texels of a lane (span_image_filter_rgb_bilinear along the row's interpolator), first half: addresses + loads
__device__ __forceinline__ Taps4 taps_issue(const uint32_t* __restrict__ tex_, const WarpGeom& g, const RowDDA& R, int i0, bool need) {
  const uint32_t* __restrict__ tex = uniform_ptr(tex_);
  Taps4 T;
  int xh[kPx], yh[kPx];
  {
    int ax = (i0 + 1) * R.rx + g.tw - 1, bx = R.x1 - 129 + i0 * R.lx;  // dda_at(...) - 128
    int ay = (i0 + 1) * R.ry + g.tw - 1, by = R.y1 - 129 + i0 * R.ly;
#pragma unroll
    for (int p = 0; p < kPx; ++p) {
      xh[p] = bx + (ax >> g.nshift); yh[p] = by + (ay >> g.nshift);
      ax += R.rx; bx += R.lx; ay += R.ry; by += R.ly;
    }
  }
  T.xf = ((uint32_t)xh[0] & 255u) | (((uint32_t)xh[1] & 255u) << 8) | (((uint32_t)xh[2] & 255u) << 16) | ((uint32_t)xh[3] << 24);
  T.yf = ((uint32_t)yh[0] & 255u) | (((uint32_t)yh[1] & 255u) << 8) | (((uint32_t)yh[2] & 255u) << 16) | ((uint32_t)yh[3] << 24);
  const bool in_range = (unsigned)(xh[0] >> 8) <= (unsigned)(g.tw - 2) && (unsigned)(xh[kPx - 1] >> 8) <= (unsigned)(g.tw - 2) &&
                        (unsigned)(yh[0] >> 8) <= (unsigned)(g.th - 2) && (unsigned)(yh[kPx - 1] >> 8) <= (unsigned)(g.th - 2);
  if (__ballot(need && !in_range) == 0ull) {
    T.mode = 0;
    const char* base = reinterpret_cast<const char*>(tex);
    const char* base1 = uniform_ptr(base + (size_t)g.pitch * 4u);
#pragma unroll
    for (int p = 0; p < kPx; ++p) {
      const uint32_t off = need ? ((uint32_t)(yh[p] >> 8) * (uint32_t)g.pitch + (uint32_t)(xh[p] >> 8)) * 4u : 0u;
      T.t0[p] = gload2(base, off);
      T.t1[p] = gload2(base1, off);
    }
  } else {
    const int tw2 = g.tw2, th2 = g.th2;
    bool one_period = true;
#pragma unroll
    for (int p = 0; p < kPx; p += kPx - 1)
      one_period = one_period && (unsigned)((xh[p] >> 8) + tw2) < 3u * (unsigned)tw2 - 1u && (unsigned)((yh[p] >> 8) + th2) < 3u * (unsigned)th2 - 1u;
    if (__ballot(need && !one_period) == 0ull) {
      T.mode = 1;
      auto reflect = [](int v, int size, int size2) {  // wrap_mode_reflect for -size2 <= v < 2 * size2
        int m = v < 0 ? v + size2 : v;
        m = m >= size2 ? m - size2 : m;
        return m >= size ? size2 - 1 - m : m;
      };
#pragma unroll
      for (int p = 0; p < kPx; ++p) {
        const int xl = need ? xh[p] >> 8 : 0, yl = need ? yh[p] >> 8 : 0;
        const uint32_t xa = (uint32_t)reflect(xl, g.tw, tw2), xb = (uint32_t)reflect(xl + 1, g.tw, tw2);
        const uint32_t ra = (uint32_t)reflect(yl, g.th, th2) * (uint32_t)g.pitch, rb = (uint32_t)reflect(yl + 1, g.th, th2) * (uint32_t)g.pitch;
        const char* base = reinterpret_cast<const char*>(tex);
        T.t0[p] = make_uint2(gload1(base, (ra + xa) * 4u), gload1(base, (ra + xb) * 4u));
        T.t1[p] = make_uint2(gload1(base, (rb + xa) * 4u), gload1(base, (rb + xb) * 4u));
        __builtin_amdgcn_sched_barrier(0);  // one pixel's addresses at a time: this (rare) path must not set the kernel's register count
      }
    } else {
      T.mode = 2;  // absurd motions only: the general interpolator, pixel by pixel, right here
      uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;  // (a rolled loop and selects: this path must not set the kernel's register count)
#pragma unroll 1
      for (int p = 0; p < kPx; ++p) {
        const uint32_t v = sample_bilinear<true>(tex, g, R, i0 + p);
        r0 = p == 0 ? v : r0; r1 = p == 1 ? v : r1; r2 = p == 2 ? v : r2; r3 = p == 3 ? v : r3;
      }
      T.t0[0] = make_uint2(r0, 0); T.t0[1] = make_uint2(r1, 0); T.t0[2] = make_uint2(r2, 0); T.t0[3] = make_uint2(r3, 0);
#pragma unroll
      for (int p = 0; p < kPx; ++p) T.t1[p] = make_uint2(0, 0);
    }
  }
  return T;
}
__device__ __forceinline__ void taps_finish(const Taps4& T, uint32_t out[kPx]) {
  if (T.mode == 2) {  // (wave-uniform)
#pragma unroll
    for (int p = 0; p < kPx; ++p) out[p] = T.t0[p].x;
  } else {
#pragma unroll
    for (int p = 0; p < kPx; ++p) out[p] = bilerp_rgb(T.t0[p], T.t1[p], (T.xf >> (8 * p)) & 255u, (T.yf >> (8 * p)) & 255u);
  }
}

// --------------------------------------------------------------------------
// compose_rigid: the compose kernel of every mode (kDeform compiles the mode-9 paths in), written around the latency of a
// strip: what a wave waits for is fetched in as few dependent round trips as the data allows.  One single-wave workgroup
// renders a 64 x 4 strip, a lane kPx = 4 horizontally adjacent pixels; objects are visited in painter's order (ascending
// ID) through the block's object masks; their coverage comes from the slots raster_kernel filled (valid over every
// touched block, zero outside the outlines).
// Reference: Process_TaskBucket DG:1216-1245, blitObject DG:762-799, computeFlowImage/getPointFlow DG:801-818, 388-407, 692-718.
//   scalar stage 1   sample record (background matrices inline) + the block's object masks   [kernel arguments are
//                    preloaded into SGPRs: leading scalar parameters, -amdgpu-kernarg-preload-count]
//   scalar stage 2   headers (coverage slot, texture origin, kind) of the first kPre objects of the mask
//   vector stage 1   background texels of both frames, coverage of those objects, their full records (lane i reads
//                    dword i; the matrices are moved to SGPRs with v_readlane when the visit needs them)
//   per visit        texture taps of both frames (one round trip), blend, flow
//   stores           8 fp32 planes, 16-byte non-temporal stores
// Mode 9 (kDeform): a deformed object's frame-1 mask, its frame-1 texture and its flow - and the same for a deformed
// background - are re-sampled through the object's warp crop, pixel by pixel, inside the same visit (DG:370-386, 341-345,
// 403-406, 670-678, 714-717); everything rigid in a mode-9 batch takes the rigid path above.  120 VGPRs = four waves per
// SIMD (the former separate mode-9 body: 158 = three); sharing the displacement loads between the mask and the texture
// of a visit costs the fourth wave (149 VGPRs) and more than it saves.
// --------------------------------------------------------------------------
constexpr int kPre = 2;  // objects of a block whose header / coverage / record are fetched ahead of their visit
#ifndef OFDG_DEFORM_FENCE
#define OFDG_DEFORM_FENCE 1
#endif

// Optional outputs of the extras variant (kExtra; rigid modes only): computeFlowImage(objects_map, true) (DG:801-818) and
// the two index images (DG:762-775) as painter's positions.  A NULL pointer is not written.
struct ExtOut {
  float* flow1;     // [n,2,H,W]
  uint8_t* label0;  // [n,H,W]
  uint8_t* label1;  // [n,H,W]
};
// Stores of the extras variant: non-temporal like the plain kernels (OFDG_EXT_NT 1), or ordinary stores that leave the flows
// and labels in L2 / MALL for the occlusion pass that reads them next (0).
#ifndef OFDG_EXT_NT
#define OFDG_EXT_NT 1
#endif

// Compact output formats (kCompact; the bits of the wrapper kernels' out_fmt argument, wave-uniform): the frames as the bytes
// the kernel holds anyway instead of their floats, the flow rounded once to binary16.
constexpr int kOutImageU8 = 1, kOutFlowF16 = 2;
// ... and of the occlusion pass that goes with them: its maps as bytes (1 / 0) instead of floats; a rounded flow target
// outside the frame in the packed targets compose leaves for it.
constexpr int kOutOccU8 = 4;
constexpr uint32_t kOccOutside = 0xFFFFFFFFu;

template <bool kPow2, bool kDeform = false, bool kExtra = false, bool kCompact = false>
__device__ __forceinline__ void compose_rigid(const DevSample* __restrict__ samples, const unsigned long long* __restrict__ blockmask,
                                              const DevObject* __restrict__ objects, const uint8_t* __restrict__ cov,
                                              int n_strips, int tiles_x, int tiles_y, int W, int H, int use_aa, int bg_pitch, int fg_pitch,
                                              const uint32_t* __restrict__ pool, const uint32_t* __restrict__ bgpool,
                                              float* __restrict__ img0, float* __restrict__ img1, float* __restrict__ flow,
                                              const DevShapeFrame* __restrict__ frames, int* __restrict__ item_count,
                                              const DevCropRef* __restrict__ crops = nullptr, ExtOut ext = ExtOut{nullptr, nullptr, nullptr},
                                              int out_fmt = 0, uint32_t* __restrict__ tgt0 = nullptr,
                                              uint32_t* __restrict__ tgt1 = nullptr) {
  static_assert(kPx == 4, "mask bytes are packed four to a word");
  static_assert(!(kDeform && kExtra), "the extras are defined for the rigid modes only");
  step_kernel_priority();
  if (blockIdx.x == 0 && threadIdx.x == 0) *item_count = 0;  // raster_kernel has consumed the work list
  // XCD-aware strip mapping: blocks b and b + 8 share an XCD (round-robin dispatch).  Every XCD takes every 8th run of 32
  // consecutive strips (= one 64 x 16 tile row of 8 tiles): neighbouring strips share their background rows, coverage and
  // object records in that XCD's L2, and the foreground-heavy samples are spread over all XCDs.  One wave per workgroup: a
  // finished wave's slot is refilled at once, not when the slowest of four sibling waves retires.
  int wg = blockIdx.x;
  if (wg < (n_strips & ~255)) {
    const int xcd = wg & 7, slot = wg >> 3;
    wg = (((slot >> 5) * 8 + xcd) << 5) + (slot & 31);
  }
  const int tile = wg >> 2, sub = wg & 3;
  const int tiles = tiles_x * tiles_y;
  const int s = tile / tiles;
  const int t = tile - s * tiles;
  const int trow = t / tiles_x;
  const int ty0 = trow * kTileH, tx0 = (t - trow * tiles_x) * kTileW;
  const int lane = (int)threadIdx.x;
  const int x0 = tx0 + (lane & 15) * kPx;
  const int y = ty0 + sub * 4 + (lane >> 4);
  const bool inside = (x0 < W) && (y < H);

  // ---- scalar stage 1: sample (+ background) record and block masks, requested in ONE batch ----
  // (the compiler loads a struct field where its first use is; an empty asm statement that names every value right here
  //  makes that one place: one s_waitcnt for the whole record instead of one per use site)
  struct SmpRec { int first_object, first_shape; Mat bg_motion, bg_tex_inv; unsigned long long bg_tex_base; int bg_deform; } smp;
  unsigned long long mask0, mask1;
  {
    const DevSample& R = samples[s];
    smp.first_object = R.first_object; smp.first_shape = R.first_shape;
    smp.bg_motion = R.bg_motion; smp.bg_tex_inv = R.bg_tex_inv; smp.bg_tex_base = R.bg_tex_base;
    smp.bg_deform = kDeform ? R.bg_deform : 0;
    const int nby = (H + kBandRows - 1) / kBandRows;
    const int brow = (ty0 + (sub >> 1) * kBandRows) / kBandRows;
    const ulonglong2 mm = *reinterpret_cast<const ulonglong2*>(blockmask + ((size_t)(s * nby + min(brow, nby - 1)) * tiles_x + tx0 / kTileW) * 2);
    mask0 = mm.x; mask1 = mm.y;
    asm volatile("" : "+s"(smp.first_object), "+s"(smp.first_shape), "+s"(smp.bg_tex_base), "+s"(mask0), "+s"(mask1),
                      "+s"(smp.bg_tex_inv.sx), "+s"(smp.bg_tex_inv.shy), "+s"(smp.bg_tex_inv.shx), "+s"(smp.bg_tex_inv.sy),
                      "+s"(smp.bg_tex_inv.tx), "+s"(smp.bg_tex_inv.ty));
    asm volatile("" : "+s"(smp.bg_motion.sx), "+s"(smp.bg_motion.shy), "+s"(smp.bg_motion.shx), "+s"(smp.bg_motion.sy),
                      "+s"(smp.bg_motion.tx), "+s"(smp.bg_motion.ty));
  }
  unsigned long long omask = mask0 | mask1;
  const DevObject* objs = objects + smp.first_object;
  const uint32_t pix = (uint32_t)(y * W + x0);
  const size_t slot_bytes = (size_t)W * H;
  constexpr int kRecLast = kDeform ? 31 : 25;  // last dword of an object's record a visit needs (31: DevObject.deform)
  static_assert(offsetof(DevObject, deform) == 31 * 4 && offsetof(DevObject, tex_base) == 24 * 4, "record dwords");

  // ---- scalar stage 2: outline slots of the first kPre objects of the mask (sample record: scalar-cache hits) ----
  const uint32_t* shape_tab = reinterpret_cast<const uint32_t*>(samples[s].shape_of);
  auto shape_entry = [&](int oi) -> uint32_t {  // oi >= 1; two 16-bit entries per dword
    const uint32_t w = shape_tab[(oi - 1) >> 1];
    return ((oi - 1) & 1) ? (w >> 16) : (w & 0xFFFFu);
  };
  int pre_oi[kPre];
  uint32_t pre_sh[kPre];
  {
    unsigned long long m = omask;
#pragma unroll
    for (int k = 0; k < kPre; ++k) {
      pre_oi[k] = m ? __ffsll((long long)m) : 0;
      m &= m - 1;  // (0 stays 0)
      pre_sh[k] = pre_oi[k] ? shape_entry(pre_oi[k]) : (uint32_t)kShapeComposite;
    }
  }

  // ---- vector stage 1: EVERY load the wave knows how to address goes out before anything is waited for: background
  // taps of frame 1, background texels of frame 0, coverage + records of the first kPre objects.  Lanes outside the frame
  // (W, H not multiples of the strip) read the texel at the origin instead of branching around the loads. ----
  WarpGeom gb;
  gb.tw = 2 * W; gb.th = 2 * H; gb.tw2 = 4 * W; gb.th2 = 4 * H;
  gb.mx2 = ((gb.tw2 & (gb.tw2 - 1)) == 0) ? gb.tw2 - 1 : -1;
  gb.my2 = ((gb.th2 & (gb.th2 - 1)) == 0) ? gb.th2 - 1 : -1;
  gb.nshift = ((gb.tw & (gb.tw - 1)) == 0) ? (31 - __clz(gb.tw)) : -1;
  gb.pitch = bg_pitch;
  const uint32_t* btex = bgpool + smp.bg_tex_base;
  const int yy = y + H / 2, xx = x0 + W / 2;
  uint4 bq = make_uint4(0, 0, 0, 0);
  RowDDA Rb;
  Taps4 Tb;
  Rb = make_row<kPow2>(smp.bg_tex_inv, inside ? yy : H / 2, gb.tw, gb.nshift);
  if constexpr (kPow2) Tb = taps_issue(btex, gb, Rb, xx, inside);
  {
    uint32_t boff = inside ? (uint32_t)(yy * gb.pitch + xx) * 4u : 0u;
    asm("" : "+v"(boff));
    const u32x4 v = *(__attribute__((address_space(1))) const u32x4*)((g_char*)reinterpret_cast<const char*>(btex) + boff);  // frame 0: identity warp == copy (DG:667-668, 680)
    bq = make_uint4(v.x, v.y, v.z, v.w);
  }
  uint32_t pre_c0[kPre], pre_c1[kPre], pre_rec[kPre];
#pragma unroll
  for (int k = 0; k < kPre; ++k) {
    pre_c0[k] = 0; pre_c1[k] = 0; pre_rec[k] = 0;
    if (!(pre_sh[k] & kShapeComposite)) {  // a simple object (wave-uniform)
      const uint8_t* c = cov + (size_t)(smp.first_shape + (int)pre_sh[k]) * 2 * slot_bytes;
      if (inside) {
        if ((mask0 >> (pre_oi[k] - 1)) & 1ull) pre_c0[k] = *reinterpret_cast<const uint32_t*>(c + pix);
        if ((mask1 >> (pre_oi[k] - 1)) & 1ull) pre_c1[k] = *reinterpret_cast<const uint32_t*>(c + slot_bytes + pix);
      }
      pre_rec[k] = reinterpret_cast<const uint32_t*>(&objs[pre_oi[k]])[min(lane, kRecLast)];  // motion, tex_inv, tex_base (mode 9: .. deform)
    }
  }

  // ---- background: frames start as its textures (masks are all 255), flow of every pixel ----
  uint32_t px0[kPx], px1[kPx];
  float fu[kPx], fv[kPx];
  if (inside) {
    if constexpr (kPow2) taps_finish(Tb, px1);
    else {
#pragma unroll
      for (int p = 0; p < kPx; ++p) px1[p] = sample_bilinear(btex, gb, Rb, xx + p);
    }
    const uint32_t tt[4] = {bq.x, bq.y, bq.z, bq.w};
    // MovingObjectBackground::getPointFlow (DG:692-718): T(-W,-H), motion, T(W,H)
    const double by = (double)(y + H / 2) + (double)(-H);
#pragma unroll
    for (int p = 0; p < kPx; ++p) {
      px0[p] = tt[p] & 0x00FFFFFFu;
      double ix = (double)(x0 + p + W / 2), iy = by;
      const float save_x = (float)(x0 + p + W / 2), save_y = (float)(y + H / 2);
      ix = ix + (double)(-W);
      xform(smp.bg_motion, ix, iy);
      ix = ix + (double)W; iy = iy + (double)H;
      fu[p] = (float)(ix - (double)save_x);
      fv[p] = (float)(iy - (double)save_y);
    }
    if constexpr (kDeform) {
      if (smp.bg_deform > 0) {  // background re-sampled through its (2W x 2H, upscaled) warp crop (DG:670-678, 714-717)
        const DevCropRef C = crops[smp.bg_deform - 1];
        const int X0 = x0 + W / 2, Y = y + H / 2;
#pragma unroll 1
        for (int p = 0; p < kPx; ++p) {
          const int X = X0 + p;
          const float2 iw = crop_pair(C, 1, X, Y);
          const Taps t = make_taps((float)X + iw.x, (float)Y + iw.y);
          px1[p] = deform_texel<kPow2>(btex, gb, smp.bg_tex_inv, t, true);
          // flow: + forward field at the destination (detour coordinates), Neumann
          double ix = (double)(x0 + p + W / 2) + (double)(-W), iy = by;
          xform(smp.bg_motion, ix, iy);
          ix = ix + (double)W; iy = iy + (double)H;
          if (ix >= 0 && ix < (double)(2 * W) && iy >= 0 && iy < (double)(2 * H)) {
            const float2 f = linear_neumann2(C, (float)ix, (float)iy);
            fu[p] += f.x;
            fv[p] += f.y;
          }
        }
      }
    }
  } else {
#pragma unroll
    for (int p = 0; p < kPx; ++p) { fu[p] = fv[p] = 0.f; px0[p] = px1[p] = 0; }
  }
  // extras: the background's backward flow, getPointFlow(.., inverse = true) (DG:692-718) with m_motion_inv = invert(bg_motion)
  // (wave-uniform fp64, once); the labels start as the background's (painter's position 0)
  float fu1[kPx], fv1[kPx];
  uint32_t lab0 = 0, lab1 = 0;
  if constexpr (kExtra) {
    const Mat bi = mat_invert(smp.bg_motion);
    const double by = (double)(y + H / 2) + (double)(-H);
#pragma unroll
    for (int p = 0; p < kPx; ++p) {
      double ix = (double)(x0 + p + W / 2), iy = by;
      const float save_x = (float)(x0 + p + W / 2), save_y = (float)(y + H / 2);
      ix = ix + (double)(-W);
      xform(bi, ix, iy);
      ix = ix + (double)W; iy = iy + (double)H;
      fu1[p] = (float)(ix - (double)save_x);
      fv1[p] = (float)(iy - (double)save_y);
    }
  }

  // ---- foreground objects in z-order ----
  WarpGeom g_frame;
  g_frame.tw = W; g_frame.th = H; g_frame.tw2 = 2 * W; g_frame.th2 = 2 * H;
  g_frame.mx2 = ((g_frame.tw2 & (g_frame.tw2 - 1)) == 0) ? g_frame.tw2 - 1 : -1;
  g_frame.my2 = ((g_frame.th2 & (g_frame.th2 - 1)) == 0) ? g_frame.th2 - 1 : -1;
  g_frame.nshift = ((W & (W - 1)) == 0) ? (31 - __clz(W)) : -1;
  g_frame.pitch = fg_pitch;
  int vi = 0;  // visit number
  while (omask) {
    const int oi = __ffsll((long long)omask);  // 1-based == index into objs[]
    omask &= omask - 1;
    const bool has0 = (mask0 >> (oi - 1)) & 1ull, has1 = (mask1 >> (oi - 1)) & 1ull;  // wave-uniform
    // (opaque copies: the int -> double conversions of the pixel coordinates are redone per visit instead of being
    //  hoisted out of the loop, where they would hold two dozen registers across every visit)
    int xv = x0, yv = y;
    asm volatile("" : "+v"(xv), "+v"(yv));
    // (mode 9, likewise: what depends only on the frame size or the lane - the doubles of W / H and + 0.5 of the row set-up, record
    //  and coverage addresses - is redone per visit instead of being held across all of them: 111 instead of 120 VGPRs)
    int Wv = W, Hv = H, lanev = lane;
    if constexpr (kDeform && OFDG_DEFORM_FENCE) asm volatile("" : "+s"(Wv), "+s"(Hv), "+v"(lanev));
    WarpGeom g_visit;
    if constexpr (kDeform && OFDG_DEFORM_FENCE) {
      g_visit.tw = Wv; g_visit.th = Hv; g_visit.tw2 = 2 * Wv; g_visit.th2 = 2 * Hv;
      g_visit.mx2 = ((g_visit.tw2 & (g_visit.tw2 - 1)) == 0) ? g_visit.tw2 - 1 : -1;
      g_visit.my2 = ((g_visit.th2 & (g_visit.th2 - 1)) == 0) ? g_visit.th2 - 1 : -1;
      g_visit.nshift = ((Wv & (Wv - 1)) == 0) ? (31 - __clz(Wv)) : -1;
      g_visit.pitch = fg_pitch;
    }
    const WarpGeom& g = (kDeform && OFDG_DEFORM_FENCE) ? g_visit : g_frame;
    const int lane = lanev;
    const int W = Wv, H = Hv;
    uint32_t sh, c0w = 0, c1w = 0, recw = 0;
    if (vi < kPre) {
      sh = vi == 0 ? pre_sh[0] : pre_sh[kPre - 1];
      c0w = vi == 0 ? pre_c0[0] : pre_c0[kPre - 1];
      c1w = vi == 0 ? pre_c1[0] : pre_c1[kPre - 1];
      recw = vi == 0 ? pre_rec[0] : pre_rec[kPre - 1];
    } else {
      sh = shape_entry(oi);
      if (!(sh & kShapeComposite)) {
        const uint8_t* c = cov + (size_t)(smp.first_shape + (int)sh) * 2 * slot_bytes;
        if (inside) {
          if (has0) c0w = *reinterpret_cast<const uint32_t*>(c + pix);
          if (has1) c1w = *reinterpret_cast<const uint32_t*>(c + slot_bytes + pix);
        }
        recw = reinterpret_cast<const uint32_t*>(&objs[oi])[min(lane, kRecLast)];
      }
    }
    ++vi;
    static_assert(kPre == 2 || kPre == 1, "the selects above pick between two prefetched sets");

    // mode 9: frame-1 mask bytes (AA and thresholded) of one outline re-sampled through the inverse field
    // (MovingObjectBase::renderMasks, DG:370-386).  Taps outside the outline's rasterised box read as 0 (the mask is 0
    // there; outside the frame: Dirichlet).
    auto warped_mask1 = [&](int shape, const DevShapeFrame& F, const DevCropRef& C, int p, int& aa, int& na) {
      aa = 0; na = 0;
      if (!inside || !has1) return;
      if (F.x0 > F.x1) return;
      const int x = xv + p;
      const float2 iw = crop_pair(C, 1, x, yv);
      const Taps t = make_taps((float)x + iw.x, (float)yv + iw.y);
      if (!t.ok || t.x + 1 < F.x0 || t.x > F.x1 || t.y + 1 < F.y0 || t.y > F.y1) return;
      const uint8_t* c = cov + ((size_t)shape * 2 + 1) * slot_bytes;
      float va[4], vn[4];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int tx = t.x + i, ty = t.y + j;
          int cv = 0;
          if (tx >= F.x0 && tx <= F.x1 && ty >= F.y0 && ty <= F.y1) cv = c[(size_t)ty * W + tx];
          va[2 * j + i] = (float)aa_byte(cv);
          vn[2 * j + i] = cv >= 128 ? 255.f : 0.f;
        }
      aa = lerp_u8(t, va[0], va[1], va[2], va[3]);
      na = lerp_u8(t, vn[0], vn[1], vn[2], vn[3]);
    };
    int odef = 0;  // mode 9: the object's warp slot + 1 (0: rigid)

    uint32_t m0w, m1w, n0w;  // blending masks of the two frames and the thresholded frame-0 mask, byte p = pixel p
    uint32_t n1w = 0;        // extras: the thresholded frame-1 mask
    if (!(sh & kShapeComposite)) {
      if constexpr (kDeform) odef = __builtin_amdgcn_readlane((int)recw, 31);
      // the box touches the block but the outline covers none of this strip's pixels: nothing to mask, sample or blend
      // (mode 9 re-samples a deformed object's frame-1 mask from elsewhere: no such shortcut)
      if (odef <= 0 && __ballot((c0w | c1w) != 0u) == 0ull) continue;
      m0w = 0; m1w = 0; n0w = 0;
#pragma unroll
      for (int p = 0; p < kPx; ++p) {
        const int c0 = (int)((c0w >> (8 * p)) & 255), c1 = (int)((c1w >> (8 * p)) & 255);
        const int na0 = c0 >= 128 ? 255 : 0;
        n0w |= (uint32_t)na0 << (8 * p);
        m0w |= (uint32_t)(use_aa ? aa_byte(c0) : na0) << (8 * p);
        m1w |= (uint32_t)(use_aa ? aa_byte(c1) : (c1 >= 128 ? 255 : 0)) << (8 * p);
        if constexpr (kExtra) n1w |= (uint32_t)(c1 >= 128 ? 255 : 0) << (8 * p);
      }
      if constexpr (kDeform) {
        if (odef > 0) {
          const int shape = smp.first_shape + (int)sh;
          const DevShapeFrame F1 = frames[shape * 2 + 1];  // (once per visit, not once per pixel)
          const DevCropRef C = crops[odef - 1];
          m1w = 0;
#pragma unroll 1
          for (int p = 0; p < kPx; ++p) {
            int aa, na;
            warped_mask1(shape, F1, C, p, aa, na);
            m1w |= (uint32_t)(use_aa ? aa : na) << (8 * p);
          }
        }
      }
    } else {
      // composite: sequential fp32 add / subtract over the components (DG:591-646)
      const DevObjectHdr h = *reinterpret_cast<const DevObjectHdr*>(&objs[oi].tex_base);
      if constexpr (kDeform) odef = h.deform;
      int ua0[kPx], ua1[kPx], un1[kPx], na0[kPx];
#pragma unroll
      for (int p = 0; p < kPx; ++p) { ua0[p] = ua1[p] = un1[p] = 0; na0[p] = 0; }
      for (int k = 0; k < h.n_shapes; ++k) {
        const uint8_t* c = cov + (size_t)(h.first_shape + k) * 2 * slot_bytes;
        uint32_t k0w = 0, k1w = 0;
        const DevShapeFrame F0 = frames[(h.first_shape + k) * 2], F1 = frames[(h.first_shape + k) * 2 + 1];
        if (inside) {
          // a component's coverage exists only in the 64 x 8 blocks its own box touches
          const int by0c = ty0 + (sub >> 1) * kBandRows;
          int d1 = 0;
          if constexpr (kDeform) { if (odef > 0) d1 = (int)ceilf(__uint_as_float(*crops[odef - 1].max_bits)) + 2; }
          const bool v0 = F0.x0 <= F0.x1 && F0.x0 <= tx0 + kTileW - 1 && F0.x1 >= tx0 && F0.y0 <= by0c + kBandRows - 1 && F0.y1 >= by0c;
          const bool v1 = F1.x0 <= F1.x1 && F1.x0 - d1 <= tx0 + kTileW - 1 && F1.x1 + d1 >= tx0 && F1.y0 - d1 <= by0c + kBandRows - 1 && F1.y1 + d1 >= by0c;
          if (has0 && v0) k0w = *reinterpret_cast<const uint32_t*>(c + pix);
          if (has1 && v1) k1w = *reinterpret_cast<const uint32_t*>(c + slot_bytes + pix);
        }
        const bool additive = (h.additive >> k) & 1u;
#pragma unroll
        for (int p = 0; p < kPx; ++p) {
          const int c0 = (int)((k0w >> (8 * p)) & 255), c1 = (int)((k1w >> (8 * p)) & 255);
          const int va0 = aa_byte(c0);
          int va1 = aa_byte(c1);
          const int vn0 = c0 >= 128 ? 255 : 0;
          int vn1 = c1 >= 128 ? 255 : 0;
          if constexpr (kDeform) {
            if (odef > 0) warped_mask1(h.first_shape + k, F1, crops[odef - 1], p, va1, vn1);  // components warp individually
          }
          if (additive) {
            ua0[p] = comp_add(ua0[p], va0); ua1[p] = comp_add(ua1[p], va1);
            na0[p] = comp_add(na0[p], vn0); un1[p] = comp_add(un1[p], vn1);
          } else {
            ua0[p] = comp_sub(ua0[p], va0); ua1[p] = comp_sub(ua1[p], va1);
            na0[p] = comp_sub(na0[p], vn0); un1[p] = comp_sub(un1[p], vn1);
          }
        }
      }
      m0w = 0; m1w = 0; n0w = 0;
#pragma unroll
      for (int p = 0; p < kPx; ++p) {
        m0w |= (uint32_t)(use_aa ? ua0[p] : na0[p]) << (8 * p);
        m1w |= (uint32_t)(use_aa ? ua1[p] : un1[p]) << (8 * p);
        n0w |= (uint32_t)na0[p] << (8 * p);
        if constexpr (kExtra) n1w |= (uint32_t)un1[p] << (8 * p);
      }
      if (__ballot((m0w | m1w | n0w | n1w) != 0u) == 0ull) continue;
      recw = reinterpret_cast<const uint32_t*>(&objs[oi])[min(lane, kRecLast)];
    }

    // the object's matrices: dword i of the record sits in lane i
    auto rec_double = [&](int i) { return __hiloint2double(__builtin_amdgcn_readlane((int)recw, 2 * i + 1), __builtin_amdgcn_readlane((int)recw, 2 * i)); };
    // origin of the W x H centre crop: dwords 24, 25 of the record
    const uint32_t* tex = pool + (((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)recw, 25) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)recw, 24));
    // frame 0 texture: identity warp == the crop itself (DG:339-340); issued with the frame-1 taps: one round trip
    uint4 q0 = make_uint4(0, 0, 0, 0);
    if (m0w) q0 = *reinterpret_cast<const uint4*>(tex + (uint32_t)(yv * g.pitch + xv));
    if (__ballot(m1w != 0u)) {
      Mat ti;
      ti.sx = rec_double(6); ti.shy = rec_double(7); ti.shx = rec_double(8); ti.sy = rec_double(9); ti.tx = rec_double(10); ti.ty = rec_double(11);
      uint32_t t1[kPx];
      if (kDeform && odef > 0) {  // applyWarpFieldToTexture(getTransformedTexture(tex, motion), iwarp) (DG:341-345)
        const DevCropRef C = crops[odef - 1];
#pragma unroll
        for (int p = 0; p < kPx; ++p) t1[p] = 0;
#pragma unroll 1
        for (int p = 0; p < kPx; ++p) {
          const bool need = ((m1w >> (8 * p)) & 255u) != 0u;
          if (__ballot(need) == 0ull) continue;
          const int x = xv + p;
          const float2 iw = need ? crop_pair(C, 1, x, yv) : make_float2(0.f, 0.f);
          const Taps t = make_taps((float)x + iw.x, (float)yv + iw.y);
          const uint32_t o = deform_texel<kPow2>(tex, g, ti, t, need);
          const uint32_t keep = need ? o : 0u;
          t1[0] = p == 0 ? keep : t1[0]; t1[1] = p == 1 ? keep : t1[1]; t1[2] = p == 2 ? keep : t1[2]; t1[3] = p == 3 ? keep : t1[3];
        }
      } else {
        const RowDDA R = make_row<kPow2>(ti, yv, W, g.nshift);
        if constexpr (kPow2) {
          const Taps4 T = taps_issue(tex, g, R, xv, m1w != 0u);
          taps_finish(T, t1);
        } else {
#pragma unroll
          for (int p = 0; p < kPx; ++p) t1[p] = m1w ? sample_bilinear(tex, g, R, xv + p) : 0u;
        }
      }
#pragma unroll
      for (int p = 0; p < kPx; ++p) px1[p] = blend_px(px1[p], t1[p], (m1w >> (8 * p)) & 255u);  // m == 0 leaves the pixel as is
    }
    if (m0w) {
      const uint32_t tt[4] = {q0.x, q0.y, q0.z, q0.w};
#pragma unroll
      for (int p = 0; p < kPx; ++p) px0[p] = blend_px(px0[p], tt[p], (m0w >> (8 * p)) & 255u);
    }
    if (__ballot(n0w != 0u)) {
      // MovingObjectBase::getPointFlow (DG:388-407) for pixels this object now owns
      Mat mo;
      mo.sx = rec_double(0); mo.shy = rec_double(1); mo.shx = rec_double(2); mo.sy = rec_double(3); mo.tx = rec_double(4); mo.ty = rec_double(5);
#pragma unroll
      for (int p = 0; p < kPx; ++p) {
        if (((n0w >> (8 * p)) & 255u) == 255u) {
          double ix = (double)(xv + p), iy = (double)yv;
          const float save_x = (float)(xv + p), save_y = (float)yv;
          xform(mo, ix, iy);
          fu[p] = (float)(ix - (double)save_x);
          fv[p] = (float)(iy - (double)save_y);
          if constexpr (kDeform) {
            if (odef > 0 && ix >= 0 && ix < (double)W && iy >= 0 && iy < (double)H) {  // DG:403-406
              const float2 f = linear_neumann2(crops[odef - 1], (float)ix, (float)iy);
              fu[p] += f.x;
              fv[p] += f.y;
            }
          }
        }
      }
    }
    if constexpr (kExtra) {
      // blitObject's index images (DG:762-775): where the non-AA mask is 255 the object (painter's position oi) owns the pixel
      uint32_t s0 = 0, s1 = 0;
#pragma unroll
      for (int p = 0; p < kPx; ++p) {
        if (((n0w >> (8 * p)) & 255u) == 255u) s0 |= 0xFFu << (8 * p);
        if (((n1w >> (8 * p)) & 255u) == 255u) s1 |= 0xFFu << (8 * p);
      }
      const uint32_t rep = (uint32_t)oi * 0x01010101u;
      lab0 = (lab0 & ~s0) | (rep & s0);
      lab1 = (lab1 & ~s1) | (rep & s1);
      if (__ballot(s1 != 0u)) {
        // getPointFlow(.., inverse = true) (DG:388-407): m_motion_inv is the record's tex_inv (dwords 12-23, = invert(motion))
        Mat mi;
        mi.sx = rec_double(6); mi.shy = rec_double(7); mi.shx = rec_double(8); mi.sy = rec_double(9); mi.tx = rec_double(10); mi.ty = rec_double(11);
#pragma unroll
        for (int p = 0; p < kPx; ++p) {
          if ((s1 >> (8 * p)) & 1u) {
            double ix = (double)(xv + p), iy = (double)yv;
            const float save_x = (float)(xv + p), save_y = (float)yv;
            xform(mi, ix, iy);
            fu1[p] = (float)(ix - (double)save_x);
            fv1[p] = (float)(iy - (double)save_y);
          }
        }
      }
    }
  }

  if (!inside) return;
  if constexpr (kCompact) {
    // Compact epilogue.  uint8 frames: DG:1229-1244 skipped - the B, G, R bytes of the lane's four BGRX words gathered into one
    // dword per plane (v_perm_b32, no conversion), 4-byte streaming stores (a row of a plane is 8-byte aligned: W % 8 == 0).
    // fp16 flow: the float32 flow converted once, round to nearest even (v_cvt_f16_f32 under the default rounding mode - not
    // v_cvt_pkrtz, which rounds towards zero), 8-byte stores.  Offsets in pixels, scaled by the element size of each output.
    const size_t plane = (size_t)W * H;
    uint32_t op = (uint32_t)y * (uint32_t)W + (uint32_t)x0;
    asm volatile("" : "+v"(op));
    if (out_fmt & kOutImageU8) {
      char* b0 = reinterpret_cast<char*>(img0) + (size_t)s * 3 * plane;
      char* b1 = reinterpret_cast<char*>(img1) + (size_t)s * 3 * plane;
      // v_perm_b32 selectors (bytes 0-3: second operand, 4-7: first): two words -> {B0, B1, G0, G1} and {R0, R1, 0, 0}, then
      // the halves of two such pairs side by side: seven instructions per frame
      auto planes = [](const uint32_t (&px)[kPx], uint32_t& b, uint32_t& g, uint32_t& r) {
        const uint32_t lo_bg = __builtin_amdgcn_perm(px[1], px[0], 0x05010400u), lo_r = __builtin_amdgcn_perm(px[1], px[0], 0x0C0C0602u);
        const uint32_t hi_bg = __builtin_amdgcn_perm(px[3], px[2], 0x05010400u), hi_r = __builtin_amdgcn_perm(px[3], px[2], 0x0C0C0602u);
        b = __builtin_amdgcn_perm(hi_bg, lo_bg, 0x05040100u);
        g = __builtin_amdgcn_perm(hi_bg, lo_bg, 0x07060302u);
        r = __builtin_amdgcn_perm(hi_r, lo_r, 0x05040100u);
      };
      uint32_t c[3];
      planes(px0, c[0], c[1], c[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) __builtin_nontemporal_store(c[k], reinterpret_cast<uint32_t*>(b0 + (size_t)k * plane + op));
      planes(px1, c[0], c[1], c[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) __builtin_nontemporal_store(c[k], reinterpret_cast<uint32_t*>(b1 + (size_t)k * plane + op));
    } else {
      char* b0 = reinterpret_cast<char*>(img0 + (size_t)s * 3 * plane);
      char* b1 = reinterpret_cast<char*>(img1 + (size_t)s * 3 * plane);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        f32x4 a = {(float)((px0[0] >> (8 * c)) & 255u), (float)((px0[1] >> (8 * c)) & 255u),
                   (float)((px0[2] >> (8 * c)) & 255u), (float)((px0[3] >> (8 * c)) & 255u)};
        f32x4 b = {(float)((px1[0] >> (8 * c)) & 255u), (float)((px1[1] >> (8 * c)) & 255u),
                   (float)((px1[2] >> (8 * c)) & 255u), (float)((px1[3] >> (8 * c)) & 255u)};
        __builtin_nontemporal_store(a, reinterpret_cast<f32x4*>(b0 + ((size_t)c * plane + op) * 4));
        __builtin_nontemporal_store(b, reinterpret_cast<f32x4*>(b1 + ((size_t)c * plane + op) * 4));
      }
    }
    if (out_fmt & kOutFlowF16) {
      char* bf = reinterpret_cast<char*>(flow) + (size_t)s * 2 * plane * 2;
      const f16x4 u = {(_Float16)fu[0], (_Float16)fu[1], (_Float16)fu[2], (_Float16)fu[3]};
      const f16x4 v = {(_Float16)fv[0], (_Float16)fv[1], (_Float16)fv[2], (_Float16)fv[3]};
      __builtin_nontemporal_store(u, reinterpret_cast<f16x4*>(bf + (size_t)op * 2));
      __builtin_nontemporal_store(v, reinterpret_cast<f16x4*>(bf + (plane + op) * 2));
    } else {
      char* bf = reinterpret_cast<char*>(flow + (size_t)s * 2 * plane);
      const f32x4 u = {fu[0], fu[1], fu[2], fu[3]};
      const f32x4 v = {fv[0], fv[1], fv[2], fv[3]};
      __builtin_nontemporal_store(u, reinterpret_cast<f32x4*>(bf + (size_t)op * 4));
      __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(bf + (plane + op) * 4));
    }
    if constexpr (kExtra) {
      // The optional outputs behind a compact epilogue (every test is wave-uniform: kernel arguments).  flow1 goes through the
      // same out_fmt bit as the flow, the labels are stored as in the float32 variant.
      if (ext.flow1) {
        if (out_fmt & kOutFlowF16) {
          char* bf1 = reinterpret_cast<char*>(ext.flow1) + (size_t)s * 2 * plane * 2;
          const f16x4 u1 = {(_Float16)fu1[0], (_Float16)fu1[1], (_Float16)fu1[2], (_Float16)fu1[3]};
          const f16x4 v1 = {(_Float16)fv1[0], (_Float16)fv1[1], (_Float16)fv1[2], (_Float16)fv1[3]};
          __builtin_nontemporal_store(u1, reinterpret_cast<f16x4*>(bf1 + (size_t)op * 2));
          __builtin_nontemporal_store(v1, reinterpret_cast<f16x4*>(bf1 + (plane + op) * 2));
        } else {
          char* bf1 = reinterpret_cast<char*>(ext.flow1 + (size_t)s * 2 * plane);
          const f32x4 u1 = {fu1[0], fu1[1], fu1[2], fu1[3]};
          const f32x4 v1 = {fv1[0], fv1[1], fv1[2], fv1[3]};
          __builtin_nontemporal_store(u1, reinterpret_cast<f32x4*>(bf1 + (size_t)op * 4));
          __builtin_nontemporal_store(v1, reinterpret_cast<f32x4*>(bf1 + (plane + op) * 4));
        }
      }
      if (ext.label0) __builtin_nontemporal_store(lab0, reinterpret_cast<uint32_t*>(ext.label0 + (size_t)s * plane + op));
      if (ext.label1) __builtin_nontemporal_store(lab1, reinterpret_cast<uint32_t*>(ext.label1 + (size_t)s * plane + op));
      // Occlusion targets for occlusion_fmt_kernel: where the float32 flow, rounded as occlusion_quad rounds it (the same
      // __fadd_rn / floorf / float compares), sends each of the lane's four pixels - the linear index yr * W + xr of the other
      // frame's pixel, kOccOutside when it leaves the frame.  Taken here, from the registers: the stored flow may be binary16,
      // and an occlusion bit must not depend on that.  One 16-byte vector store per frame into the chain's workspace.
      auto targets = [&](const float (&uu)[kPx], const float (&vv)[kPx]) {
        uint32_t t[kPx];
#pragma unroll
        for (int p = 0; p < kPx; ++p) {
          const float fx = floorf(__fadd_rn(__fadd_rn((float)(x0 + p), uu[p]), 0.5f));
          const float fy = floorf(__fadd_rn(__fadd_rn((float)y, vv[p]), 0.5f));
          const bool in = fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H;
          t[p] = in ? (uint32_t)((int)fy * W + (int)fx) : kOccOutside;
        }
        const u32x4 r = {t[0], t[1], t[2], t[3]};
        return r;
      };
      if (tgt0) __builtin_nontemporal_store(targets(fu, fv), reinterpret_cast<u32x4*>(tgt0 + (size_t)s * plane + op));
      if (tgt1) __builtin_nontemporal_store(targets(fu1, fv1), reinterpret_cast<u32x4*>(tgt1 + (size_t)s * plane + op));
    }
    return;
  }
  // u8 -> float planes (DG:1229-1245); streaming 16-byte stores, never re-read.  Every plane is a wave-uniform base
  // (SGPR pair) + one 32-bit byte offset per lane; the offset is made opaque so that no address arithmetic is
  // hoisted above the object loop (it would hold registers there).
  const size_t plane = (size_t)W * H;
  uint32_t ob = ((uint32_t)y * (uint32_t)W + (uint32_t)x0) * 4u;
  asm volatile("" : "+v"(ob));
  char* b0 = reinterpret_cast<char*>(img0 + (size_t)s * 3 * plane);
  char* b1 = reinterpret_cast<char*>(img1 + (size_t)s * 3 * plane);
  char* bf = reinterpret_cast<char*>(flow + (size_t)s * 2 * plane);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f32x4 a = {(float)((px0[0] >> (8 * c)) & 255u), (float)((px0[1] >> (8 * c)) & 255u),
               (float)((px0[2] >> (8 * c)) & 255u), (float)((px0[3] >> (8 * c)) & 255u)};
    f32x4 b = {(float)((px1[0] >> (8 * c)) & 255u), (float)((px1[1] >> (8 * c)) & 255u),
               (float)((px1[2] >> (8 * c)) & 255u), (float)((px1[3] >> (8 * c)) & 255u)};
    __builtin_nontemporal_store(a, reinterpret_cast<f32x4*>(b0 + (size_t)c * plane * 4 + ob));
    __builtin_nontemporal_store(b, reinterpret_cast<f32x4*>(b1 + (size_t)c * plane * 4 + ob));
  }
  f32x4 u = {fu[0], fu[1], fu[2], fu[3]};
  f32x4 v = {fv[0], fv[1], fv[2], fv[3]};
  if constexpr (kExtra && !OFDG_EXT_NT) {
    *reinterpret_cast<f32x4*>(bf + ob) = u;
    *reinterpret_cast<f32x4*>(bf + plane * 4 + ob) = v;
  } else {
    __builtin_nontemporal_store(u, reinterpret_cast<f32x4*>(bf + ob));
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(bf + plane * 4 + ob));
  }
  if constexpr (kExtra) {
    // (the pointers are kernel arguments: every test below is wave-uniform)
    if (ext.flow1) {
      char* bf1 = reinterpret_cast<char*>(ext.flow1 + (size_t)s * 2 * plane);
      const f32x4 u1 = {fu1[0], fu1[1], fu1[2], fu1[3]};
      const f32x4 v1 = {fv1[0], fv1[1], fv1[2], fv1[3]};
      if constexpr (!OFDG_EXT_NT) {
        *reinterpret_cast<f32x4*>(bf1 + ob) = u1;
        *reinterpret_cast<f32x4*>(bf1 + plane * 4 + ob) = v1;
      } else {
        __builtin_nontemporal_store(u1, reinterpret_cast<f32x4*>(bf1 + ob));
        __builtin_nontemporal_store(v1, reinterpret_cast<f32x4*>(bf1 + plane * 4 + ob));
      }
    }
    const uint32_t lb = ob >> 2;  // byte offset of the lane's 4 label bytes in the sample's plane (W is a multiple of 8)
    if (ext.label0) {
      uint32_t* d = reinterpret_cast<uint32_t*>(ext.label0 + (size_t)s * plane + lb);
      if constexpr (!OFDG_EXT_NT) *d = lab0; else __builtin_nontemporal_store(lab0, d);
    }
    if (ext.label1) {
      uint32_t* d = reinterpret_cast<uint32_t*>(ext.label1 + (size_t)s * plane + lb);
      if constexpr (!OFDG_EXT_NT) *d = lab1; else __builtin_nontemporal_store(lab1, d);
    }
  }
}

// Leading scalar parameters are preloaded into SGPRs (no load, no wait before the first record fetch).
__global__ __launch_bounds__(64) void compose_rigid_kernel(
    const DevSample* __restrict__ samples, const unsigned long long* __restrict__ blockmask, const DevObject* __restrict__ objects,
    const uint8_t* __restrict__ cov, int n_strips, int tiles_x, int tiles_y, int W, int H, int use_aa, int bg_pitch, int fg_pitch,
    const uint32_t* __restrict__ pool, const uint32_t* __restrict__ bgpool, float* __restrict__ img0, float* __restrict__ img1,
    float* __restrict__ flow, const DevShapeFrame* __restrict__ frames, int* __restrict__ item_count) {
  compose_rigid<false>(samples, blockmask, objects, cov, n_strips, tiles_x, tiles_y, W, H, use_aa, bg_pitch, fg_pitch, pool, bgpool, img0, img1,
                       flow, frames, item_count);
}
// W a power of two (512, 1024, ...): shift-only interpolators and paired tap loads.
__global__ __launch_bounds__(64) void compose_rigid_pow2_kernel(
    const DevSample* __restrict__ samples, const unsigned long long* __restrict__ blockmask, const DevObject* __restrict__ objects,
    const uint8_t* __restrict__ cov, int n_strips, int tiles_x, int tiles_y, int W, int H, int use_aa, int bg_pitch, int fg_pitch,
    const uint32_t* __restrict__ pool, const uint32_t* __restrict__ bgpool, float* __restrict__ img0, float* __restrict__ img1,
    float* __restrict__ flow, const DevShapeFrame* __restrict__ frames, int* __restrict__ item_count) {
  compose_rigid<true>(samples, blockmask, objects, cov, n_strips, tiles_x, tiles_y, W, H, use_aa, bg_pitch, fg_pitch, pool, bgpool, img0, img1,
                      flow, frames, item_count);
}
// The same two with the optional outputs (backward flow, index images of both frames) written as well.
__global__ __launch_bounds__(64) void compose_rigid_ext_kernel(
    const DevSample* __restrict__ samples, const unsigned long long* __restrict__ blockmask, const DevObject* __restrict__ objects,
    const uint8_t* __restrict__ cov, int n_strips, int tiles_x, int tiles_y, int W, int H, int use_aa, int bg_pitch, int fg_pitch,
    const uint32_t* __restrict__ pool, const uint32_t* __restrict__ bgpool, float* __restrict__ img0, float* __restrict__ img1,
    float* __restrict__ flow, const DevShapeFrame* __restrict__ frames, int* __restrict__ item_count, ExtOut ext) {
  compose_rigid<false, false, true>(samples, blockmask, objects, cov, n_strips, tiles_x, tiles_y, W, H, use_aa, bg_pitch, fg_pitch, pool, bgpool,
                                    img0, img1, flow, frames, item_count, nullptr, ext);
}
__global__ __launch_bounds__(64) void compose_rigid_ext_pow2_kernel(
    const DevSample* __restrict__ samples, const unsigned long long* __restrict__ blockmask, const DevObject* __restrict__ objects,
    const uint8_t* __restrict__ cov, int n_strips, int tiles_x, int tiles_y, int W, int H, int use_aa, int bg_pitch, int fg_pitch,
    const uint32_t* __restrict__ pool, const uint32_t* __restrict__ bgpool, float* __restrict__ img0, float* __restrict__ img1,
    float* __restrict__ flow, const DevShapeFrame* __restrict__ frames, int* __restrict__ item_count, ExtOut ext) {
  compose_rigid<true, false, true>(samples, blockmask, objects, cov, n_strips, tiles_x, tiles_y, W, H, use_aa, bg_pitch, fg_pitch, pool, bgpool,
                                   img0, img1, flow, frames, item_count, nullptr, ext);
}
// ... and with the compact output formats (out_fmt: kOutImageU8 | kOutFlowF16; img0 / img1 / flow point at buffers of
// those element types).
__global__ __launch_bounds__(64) void compose_rigid_fmt_kernel(
    const DevSample* __restrict__ samples, const unsigned long long* __restrict__ blockmask, const DevObject* __restrict__ objects,
    const uint8_t* __restrict__ cov, int n_strips, int tiles_x, int tiles_y, int W, int H, int use_aa, int bg_pitch, int fg_pitch,
    const uint32_t* __restrict__ pool, const uint32_t* __restrict__ bgpool, void* __restrict__ img0, void* __restrict__ img1,
    void* __restrict__ flow, const DevShapeFrame* __restrict__ frames, int* __restrict__ item_count, int out_fmt) {
  compose_rigid<false, false, false, true>(samples, blockmask, objects, cov, n_strips, tiles_x, tiles_y, W, H, use_aa, bg_pitch, fg_pitch, pool,
                                           bgpool, static_cast<float*>(img0), static_cast<float*>(img1), static_cast<float*>(flow), frames,
                                           item_count, nullptr, ExtOut{nullptr, nullptr, nullptr}, out_fmt);
}
__global__ __launch_bounds__(64) void compose_rigid_fmt_pow2_kernel(
    const DevSample* __restrict__ samples, const unsigned long long* __restrict__ blockmask, const DevObject* __restrict__ objects,
    const uint8_t* __restrict__ cov, int n_strips, int tiles_x, int tiles_y, int W, int H, int use_aa, int bg_pitch, int fg_pitch,
    const uint32_t* __restrict__ pool, const uint32_t* __restrict__ bgpool, void* __restrict__ img0, void* __restrict__ img1,
    void* __restrict__ flow, const DevShapeFrame* __restrict__ frames, int* __restrict__ item_count, int out_fmt) {
  compose_rigid<true, false, false, true>(samples, blockmask, objects, cov, n_strips, tiles_x, tiles_y, W, H, use_aa, bg_pitch, fg_pitch, pool,
                                          bgpool, static_cast<float*>(img0), static_cast<float*>(img1), static_cast<float*>(flow), frames,
                                          item_count, nullptr, ExtOut{nullptr, nullptr, nullptr}, out_fmt);
}

// Occlusion maps from the labels and flows compose wrote (one pass per batch, behind compose on the same stream).  A pixel
// of frame f is occluded (1.0f) when its flow, rounded as (int)floorf((float)x + u + 0.5f), leaves the frame or lands on a
// pixel of the other frame with another label.  A lane takes 4 adjacent pixels: 16-byte flow loads, one 4-byte label load,
// 4 byte gathers of the other frame's label (local: mostly L2 hits), 16-byte stores.  occ0 / occ1 NULL: not computed.
__device__ __forceinline__ f32x4 occlusion_quad(const float* __restrict__ u_plane, const float* __restrict__ v_plane,
                                                 const uint8_t* __restrict__ own, const uint8_t* __restrict__ other, int x0, int y,
                                                 int W, int H) {
  const float4 u = *reinterpret_cast<const float4*>(u_plane);
  const float4 v = *reinterpret_cast<const float4*>(v_plane);
  const uint32_t l = *reinterpret_cast<const uint32_t*>(own);
  const float uu[4] = {u.x, u.y, u.z, u.w}, vv[4] = {v.x, v.y, v.z, v.w};
  float o[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float fx = floorf(__fadd_rn(__fadd_rn((float)(x0 + p), uu[p]), 0.5f));
    const float fy = floorf(__fadd_rn(__fadd_rn((float)y, vv[p]), 0.5f));
    // (compared as floats: the same as testing the int of floorf against [0, W) x [0, H), and defined for any value)
    const bool in = fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H;
    const int off = in ? ((int)fy - y) * W + ((int)fx - x0) : 0;  // relative to pixel x0 of row y of the other frame
    const uint32_t t = in ? (uint32_t)other[off] : 0u;
    o[p] = (in && t == ((l >> (8 * p)) & 255u)) ? 0.f : 1.f;
  }
  const f32x4 r = {o[0], o[1], o[2], o[3]};
  return r;
}
__global__ __launch_bounds__(256) void occlusion_kernel(const float* __restrict__ flow, const float* __restrict__ flow1,
                                                        const uint8_t* __restrict__ label0, const uint8_t* __restrict__ label1,
                                                        float* __restrict__ occ0, float* __restrict__ occ1, int W, int H, int n) {
  const int qpr = W >> 2;  // quads per row
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (long long)n * H * qpr) return;
  const int row = (int)(q / qpr);  // s * H + y
  const int x0 = (int)(q - (long long)row * qpr) * 4;
  const int s = row / H, y = row - s * H;
  const size_t plane = (size_t)W * H;
  const size_t pix = (size_t)y * W + x0;
  if (occ0) {
    const float* f = flow + (size_t)s * 2 * plane + pix;
    const f32x4 o = occlusion_quad(f, f + plane, label0 + s * plane + pix, label1 + s * plane + pix, x0, y, W, H);
    __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(occ0 + s * plane + pix));
  }
  if (occ1) {
    const float* f = flow1 + (size_t)s * 2 * plane + pix;
    const f32x4 o = occlusion_quad(f, f + plane, label1 + s * plane + pix, label0 + s * plane + pix, x0, y, W, H);
    __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(occ1 + s * plane + pix));
  }
}

// The optional outputs together with the compact formats: the kExtra body with the compact epilogue (out_fmt as for
// compose_rigid_fmt_kernel; ext.flow1 has the flow's element type), plus the packed occlusion targets of the frames whose
// occlusion map is asked for (tgt0 / tgt1 [n,H,W], NULL: not stored).
__global__ __launch_bounds__(64) void compose_rigid_ext_fmt_kernel(
    const DevSample* __restrict__ samples, const unsigned long long* __restrict__ blockmask, const DevObject* __restrict__ objects,
    const uint8_t* __restrict__ cov, int n_strips, int tiles_x, int tiles_y, int W, int H, int use_aa, int bg_pitch, int fg_pitch,
    const uint32_t* __restrict__ pool, const uint32_t* __restrict__ bgpool, void* __restrict__ img0, void* __restrict__ img1,
    void* __restrict__ flow, const DevShapeFrame* __restrict__ frames, int* __restrict__ item_count, ExtOut ext, int out_fmt,
    uint32_t* __restrict__ tgt0, uint32_t* __restrict__ tgt1) {
  compose_rigid<false, false, true, true>(samples, blockmask, objects, cov, n_strips, tiles_x, tiles_y, W, H, use_aa, bg_pitch, fg_pitch, pool,
                                          bgpool, static_cast<float*>(img0), static_cast<float*>(img1), static_cast<float*>(flow), frames,
                                          item_count, nullptr, ext, out_fmt, tgt0, tgt1);
}
__global__ __launch_bounds__(64) void compose_rigid_ext_fmt_pow2_kernel(
    const DevSample* __restrict__ samples, const unsigned long long* __restrict__ blockmask, const DevObject* __restrict__ objects,
    const uint8_t* __restrict__ cov, int n_strips, int tiles_x, int tiles_y, int W, int H, int use_aa, int bg_pitch, int fg_pitch,
    const uint32_t* __restrict__ pool, const uint32_t* __restrict__ bgpool, void* __restrict__ img0, void* __restrict__ img1,
    void* __restrict__ flow, const DevShapeFrame* __restrict__ frames, int* __restrict__ item_count, ExtOut ext, int out_fmt,
    uint32_t* __restrict__ tgt0, uint32_t* __restrict__ tgt1) {
  compose_rigid<true, false, true, true>(samples, blockmask, objects, cov, n_strips, tiles_x, tiles_y, W, H, use_aa, bg_pitch, fg_pitch, pool,
                                         bgpool, static_cast<float*>(img0), static_cast<float*>(img1), static_cast<float*>(flow), frames,
                                         item_count, nullptr, ext, out_fmt, tgt0, tgt1);
}

// Occlusion maps from the labels and the packed targets compose_rigid_ext_fmt_kernel wrote (behind it on the same stream):
// the definition of occlusion_kernel with the rounding already done from the float32 flow.  A lane takes 4 adjacent pixels
// of a frame: one 16-byte load of targets, one 4-byte load of its own labels, 4 byte gathers of the other frame's labels,
// one 4-byte (uint8 maps: 1 / 0) or 16-byte (float32: 1.0f / 0.0f) store.  occ0 / occ1 NULL: not computed.
__device__ __forceinline__ uint32_t occlusion_fmt_quad(const uint32_t* __restrict__ tgt, const uint8_t* __restrict__ own,
                                                       const uint8_t* __restrict__ other, uint32_t plane) {
  const uint4 t = *reinterpret_cast<const uint4*>(tgt);
  const uint32_t l = *reinterpret_cast<const uint32_t*>(own);
  const uint32_t tt[4] = {t.x, t.y, t.z, t.w};
  uint32_t o = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const bool in = tt[p] < plane;  // (kOccOutside is not; nothing else is ever stored, and no index leaves the sample's plane)
    const uint32_t b = (uint32_t)other[in ? tt[p] : 0u];  // (`other`: the sample's plane)
    o |= ((in && b == ((l >> (8 * p)) & 255u)) ? 0u : 1u) << (8 * p);
  }
  return o;
}
__global__ __launch_bounds__(256) void occlusion_fmt_kernel(const uint32_t* __restrict__ tgt0, const uint32_t* __restrict__ tgt1,
                                                            const uint8_t* __restrict__ label0, const uint8_t* __restrict__ label1,
                                                            void* __restrict__ occ0, void* __restrict__ occ1, int W, int H, int n,
                                                            int out_fmt) {
  const int qpr = W >> 2;  // quads per row
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (long long)n * H * qpr) return;
  const size_t plane = (size_t)W * H;
  const size_t pix = (size_t)q * 4;  // s * plane + y * W + x0
  const size_t sp = (size_t)(q / ((long long)H * qpr)) * plane;  // the sample's plane
  auto store = [&](void* dst, uint32_t o) {
    if (out_fmt & kOutOccU8) {
      __builtin_nontemporal_store(o, reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(dst) + pix));
    } else {
      const f32x4 f = {(float)(o & 1u), (float)((o >> 8) & 1u), (float)((o >> 16) & 1u), (float)(o >> 24)};
      __builtin_nontemporal_store(f, reinterpret_cast<f32x4*>(static_cast<float*>(dst) + pix));
    }
  };
  if (occ0) store(occ0, occlusion_fmt_quad(tgt0 + pix, label0 + pix, label1 + sp, (uint32_t)plane));
  if (occ1) store(occ1, occlusion_fmt_quad(tgt1 + pix, label1 + pix, label0 + sp, (uint32_t)plane));
}

// --------------------------------------------------------------------------
// Per-object annotation table (ofdg_object_table): what the label planes and the batch's records say about each object.
// Two launches behind the call that wrote the labels.
// --------------------------------------------------------------------------
// The header: one thread per (sample, row).  Row k < count takes id, type and motion from objects[first_object + k] (row 0: the
// background), area 0 and the empty box {W, H, -1, -1} of both frames; rows past the count are zero bytes; row 0's thread writes
// the count.  Every byte of the table is written here, so the reduction behind it only ever adds to it.
__global__ __launch_bounds__(256) void object_table_header_kernel(const DevSample* __restrict__ samples, const DevObject* __restrict__ objects,
                                                                  const DevShape* __restrict__ shapes, int n, int rows_per_sample, int W,
                                                                  int H, DevObjectRow* __restrict__ rows, int32_t* __restrict__ counts) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * rows_per_sample) return;
  const int s = (int)(t / rows_per_sample), k = (int)(t - (long long)s * rows_per_sample);
  const int count = samples[s].n_objects;  // (the background counts)
  if (k == 0) counts[s] = count;
  DevObjectRow r = DevObjectRow();
  if (k < count) {
    const DevObject& o = objects[samples[s].first_object + k];
    r.obj_id = o.id;
    // ObjType_t of the blueprint: a composite's record says so itself, a simple object's outline carries the type
    r.obj_type = o.kind == 2 ? 3 : (o.kind == 1 && o.n_shapes > 0) ? shapes[o.first_shape].type : 0;
#pragma unroll
    for (int f = 0; f < 2; ++f) { r.box[f][0] = W; r.box[f][1] = H; r.box[f][2] = -1; r.box[f][3] = -1; }
    r.motion[0] = o.motion.sx; r.motion[1] = o.motion.shy; r.motion[2] = o.motion.shx;
    r.motion[3] = o.motion.sy; r.motion[4] = o.motion.tx; r.motion[5] = o.motion.ty;
  }
  rows[t] = r;
}

// The reduction: one workgroup per (band of kTabBand rows, frame, sample), a wave per row, a lane per 4 adjacent label bytes
// (one 4-byte load; the planes are dense uint8 and W is a multiple of 8).  Labels are spatially coherent, so a wave first
// reduces per DISTINCT label of its row segment: it takes the first unretired byte's label, one ballot per byte position says
// which lanes hold it there, and count / min x / max x fall out of the four masks in scalar code (a lane's x grows with the
// lane: the first and last set bit of a mask are its extremes) - no cross-lane data movement; y is the wave's row.  Lane 0
// adds the result to the workgroup's table in LDS (65 rows x {count, min x, min y, max x, max y}); at the end the non-empty
// rows below min(count, rows_per_sample) go to the global table with one int32 atomic per field.  A byte that is no valid
// label of the sample (the planes are the caller's word) is counted nowhere.
constexpr int kTabBand = 16;   // rows of a frame per workgroup
constexpr int kTabWaves = 4;
__global__ __launch_bounds__(64 * kTabWaves) void object_table_reduce_kernel(const DevSample* __restrict__ samples,
                                                                             const uint8_t* __restrict__ label0,
                                                                             const uint8_t* __restrict__ label1, int W, int H,
                                                                             int rows_per_sample, DevObjectRow* __restrict__ rows) {
  __shared__ int tab[kObjectRows * 5];
  const int band = (int)blockIdx.x, f = (int)blockIdx.y, s = (int)blockIdx.z;
  const uint8_t* const labels = f ? label1 : label0;
  if (!labels) return;  // (that frame was not asked for: its areas stay 0, its boxes empty)
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < kObjectRows * 5; i += 64 * kTabWaves) {
    const int j = i % 5;
    tab[i] = j == 0 ? 0 : (j < 3 ? 0x7FFFFFFF : -1);
  }
  __syncthreads();
  const uint8_t* const plane = labels + (size_t)s * W * H;
  const int y_end = min(H, (band + 1) * kTabBand);
  for (int y = band * kTabBand + wave; y < y_end; y += kTabWaves) {
    for (int xc = 0; xc < W; xc += 256) {
      const int x0 = xc + 4 * lane;
      const bool act = x0 < W;  // (W % 4 == 0: the whole quad is inside)
      const uint32_t w = act ? *reinterpret_cast<const uint32_t*>(plane + (size_t)y * W + x0) : 0u;
      uint32_t rem = act ? 0xFu : 0u;  // bytes of this lane no label has taken yet
      for (;;) {
        const unsigned long long live = __ballot(rem != 0u);
        if (!live) break;
        const int leader = __ffsll(live) - 1;
        const uint32_t mine = rem ? (w >> (8 * (__ffs((int)rem) - 1))) & 255u : 0u;
        const uint32_t lab = (uint32_t)__shfl((int)mine, leader, 64);
        int cnt = 0, lo = 0x7FFFFFFF, hi = -1;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const bool hit = act && ((w >> (8 * p)) & 255u) == lab;
          const unsigned long long m = __ballot(hit);
          if (hit) rem &= ~(1u << p);
          if (m) {
            cnt += __popcll(m);
            lo = min(lo, xc + 4 * (__ffsll(m) - 1) + p);
            hi = max(hi, xc + 4 * (63 - __clzll((long long)m)) + p);
          }
        }
        if (lane == 0 && lab < (uint32_t)kObjectRows) {
          int* const e = tab + lab * 5;
          atomicAdd(e, cnt);
          atomicMin(e + 1, lo); atomicMin(e + 2, y);
          atomicMax(e + 3, hi); atomicMax(e + 4, y);
        }
      }
    }
  }
  __syncthreads();
  const int limit = min(min(samples[s].n_objects, rows_per_sample), kObjectRows);
  DevObjectRow* const out = rows + (size_t)s * rows_per_sample;
  for (int i = tid; i < limit * 5; i += 64 * kTabWaves) {
    const int k = i / 5, j = i - 5 * k;
    if (tab[k * 5] == 0) continue;
    if (j == 0) atomicAdd(&out[k].area[f], tab[i]);
    else if (j < 3) atomicMin(&out[k].box[f][j - 1], tab[i]);
    else atomicMax(&out[k].box[f][j - 1], tab[i]);
  }
}

// Mode 9: the same body with the deformation paths compiled in (masks, textures and flow of deformed objects and backgrounds
// re-sampled through their warp crops).
__global__ __launch_bounds__(64) void compose_deform_kernel(
    RenderDims dm, const DevSample* __restrict__ samples, const DevObject* __restrict__ objects,
    const unsigned long long* __restrict__ blockmask, const uint8_t* __restrict__ cov, const uint32_t* __restrict__ pool,
    const uint32_t* __restrict__ bgpool, float* __restrict__ img0, float* __restrict__ img1, float* __restrict__ flow,
    const DevShapeFrame* __restrict__ frames, const DevCropRef* __restrict__ crops, int* __restrict__ item_count) {
  compose_rigid<false, true>(samples, blockmask, objects, cov, (int)gridDim.x, dm.tiles_x, dm.tiles_y, dm.W, dm.H, dm.use_aa, dm.bg_pitch, dm.fg_pitch,
                             pool, bgpool, img0, img1, flow, frames, item_count, crops);
}
// Mode 9, W a power of two.
#ifdef OFDG_DEFORM_WAVES
#define OFDG_DEFORM_OCC __attribute__((amdgpu_waves_per_eu(OFDG_DEFORM_WAVES)))
#else
#define OFDG_DEFORM_OCC
#endif
__global__ __launch_bounds__(64) OFDG_DEFORM_OCC void compose_deform_pow2_kernel(
    RenderDims dm, const DevSample* __restrict__ samples, const DevObject* __restrict__ objects,
    const unsigned long long* __restrict__ blockmask, const uint8_t* __restrict__ cov, const uint32_t* __restrict__ pool,
    const uint32_t* __restrict__ bgpool, float* __restrict__ img0, float* __restrict__ img1, float* __restrict__ flow,
    const DevShapeFrame* __restrict__ frames, const DevCropRef* __restrict__ crops, int* __restrict__ item_count) {
  compose_rigid<true, true>(samples, blockmask, objects, cov, (int)gridDim.x, dm.tiles_x, dm.tiles_y, dm.W, dm.H, dm.use_aa, dm.bg_pitch, dm.fg_pitch,
                            pool, bgpool, img0, img1, flow, frames, item_count, crops);
}
// Mode 9 with the compact output formats (out_fmt as for compose_rigid_fmt_kernel).
__global__ __launch_bounds__(64) void compose_deform_fmt_kernel(
    RenderDims dm, const DevSample* __restrict__ samples, const DevObject* __restrict__ objects,
    const unsigned long long* __restrict__ blockmask, const uint8_t* __restrict__ cov, const uint32_t* __restrict__ pool,
    const uint32_t* __restrict__ bgpool, void* __restrict__ img0, void* __restrict__ img1, void* __restrict__ flow,
    const DevShapeFrame* __restrict__ frames, const DevCropRef* __restrict__ crops, int* __restrict__ item_count, int out_fmt) {
  compose_rigid<false, true, false, true>(samples, blockmask, objects, cov, (int)gridDim.x, dm.tiles_x, dm.tiles_y, dm.W, dm.H, dm.use_aa, dm.bg_pitch,
                                          dm.fg_pitch, pool, bgpool, static_cast<float*>(img0), static_cast<float*>(img1),
                                          static_cast<float*>(flow), frames, item_count, crops, ExtOut{nullptr, nullptr, nullptr}, out_fmt);
}
__global__ __launch_bounds__(64) OFDG_DEFORM_OCC void compose_deform_fmt_pow2_kernel(
    RenderDims dm, const DevSample* __restrict__ samples, const DevObject* __restrict__ objects,
    const unsigned long long* __restrict__ blockmask, const uint8_t* __restrict__ cov, const uint32_t* __restrict__ pool,
    const uint32_t* __restrict__ bgpool, void* __restrict__ img0, void* __restrict__ img1, void* __restrict__ flow,
    const DevShapeFrame* __restrict__ frames, const DevCropRef* __restrict__ crops, int* __restrict__ item_count, int out_fmt) {
  compose_rigid<true, true, false, true>(samples, blockmask, objects, cov, (int)gridDim.x, dm.tiles_x, dm.tiles_y, dm.W, dm.H, dm.use_aa, dm.bg_pitch,
                                         dm.fg_pitch, pool, bgpool, static_cast<float*>(img0), static_cast<float*>(img1),
                                         static_cast<float*>(flow), frames, item_count, crops, ExtOut{nullptr, nullptr, nullptr}, out_fmt);
}

// --------------------------------------------------------------------------
// Mode-9 warp fields (reference: src/caffe/WarpFields.cpp = WF).
// A field is 4 planes of S*S floats: flow x, flow y, iflow x, iflow y.
// --------------------------------------------------------------------------
// DisplacementComposer::flow_at / iflow_at sampled on the S x S grid (WF:296-316, 347-354)
__global__ __launch_bounds__(256) void wf_sample_kernel(const DevDisplacer* __restrict__ disp, int n_disp, int S,
                                                        float* __restrict__ field) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * S) return;
  const float x = (float)(i % S), y = (float)(i / S);
  float fu = 0, fv = 0, iu = 0, iv = 0;
  for (int k = 0; k < n_disp; ++k) {
    const DevDisplacer& D = disp[k];
    float u, v, ju, jv;
    if (D.type == 0) {
      u = D.dx; v = D.dy; ju = -D.dx; jv = -D.dy;
    } else {
      const float dx = x - D.cx, dy = y - D.cy;
      if (D.type == 1) {
        u = (D.cos_nomega * dx - D.sin_nomega * dy) - dx;
        v = (D.sin_nomega * dx + D.cos_nomega * dy) - dy;
        ju = (D.cos_omega * dx - D.sin_omega * dy) - dx;
        jv = (D.sin_omega * dx + D.cos_omega * dy) - dy;
      } else {
        u = D.factor * dx - dx; v = D.factor * dy - dy;
        ju = D.ifactor * dx - dx; jv = D.ifactor * dy - dy;
      }
    }
    // Gaussian2D::at (WF:101-112)
    const float rx = D.a * (x - D.scx) + D.b * (y - D.scy);
    const float ry = (D.c * (x - D.scx) + D.d * (y - D.scy)) * D.ratio_x_y;
    const float dist_sq = rx * rx + ry * ry;
    // (expf = ofdg_det_expf: the fp64 value rounded once, the same on the device and in the oracle)
    const float w = D.normalizer * (D.gauss_prefactor * ofdg_det_expf(-dist_sq / D.two_sigma_sq));
    fu += u * w; fv += v * w;
    iu += ju * w; iv += jv * w;
  }
  const size_t n = (size_t)S * S;
  field[i] = fu; field[n + i] = fv; field[2 * n + i] = iu; field[3 * n + i] = iv;
}

// One self-composition pass f <- f + f o (id + f) for both the forward pair (planes 0,1)
// and the inverse pair (planes 2,3) (WF:366-384, 406-424); flags pixels leaving the field.
__global__ __launch_bounds__(256) void wf_compose_kernel(const float* __restrict__ from, float* __restrict__ to, int S,
                                                         uint8_t* __restrict__ flagged) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int pair = blockIdx.y;  // 0 forward, 1 inverse
  if (i >= S * S) return;
  const size_t n = (size_t)S * S;
  const float* fx_p = from + (size_t)(2 * pair) * n;
  const float* fy_p = fx_p + n;
  const int x = i % S, y = i / S;
  const float fx = fx_p[i], fy = fy_p[i];
  float ox = fx, oy = fy;
  if ((float)x + fx < 0 || (float)x + fx >= (float)S || (float)y + fy < 0 || (float)y + fy >= (float)S) {
    flagged[(size_t)pair * n + i] = 255;
  } else {
    ox = fx + linear_neumann(fx_p, S, S, (float)x + fx, (float)y + fy);
    oy = fy + linear_neumann(fy_p, S, S, (float)x + fx, (float)y + fy);
  }
  to[(size_t)(2 * pair) * n + i] = ox;
  to[(size_t)(2 * pair + 1) * n + i] = oy;
}

// NaN-out flagged pixels, then clamp_near_zeros (WF:389-398, 425-434, 444-455)
__global__ __launch_bounds__(256) void wf_finish_kernel(float* __restrict__ field, int S, const uint8_t* __restrict__ flagged) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int pair = blockIdx.y;
  if (i >= S * S) return;
  const size_t n = (size_t)S * S;
  float* fx_p = field + (size_t)(2 * pair) * n;
  float* fy_p = fx_p + n;
  const int x = i % S, y = i / S;
  float fx = fx_p[i], fy = fy_p[i];
  bool flag = flagged[(size_t)pair * n + i] != 0;
  if ((float)x + fx < 0 || (float)x + fx >= (float)S || (float)y + fy < 0 || (float)y + fy >= (float)S) flag = true;
  if (flag) {
    fx = __int_as_float(0x7fc00000); fy = fx;
  } else {
    if (fabsf(fx) < 1e-3f) fx = 0.f;
    if (fabsf(fy) < 1e-3f) fy = 0.f;
  }
  fx_p[i] = fx; fy_p[i] = fy;
}

// get_crop(x, y, x+W, y+H) (WF:623-624): copy the four planes of one crop out of a field,
// and reduce max |iflow| (NaNs ignored) for the box dilation of deforming objects.
__global__ __launch_bounds__(256) void wf_crop_kernel(const float* __restrict__ field, int S, int x0, int y0, int cw, int ch,
                                                      float* __restrict__ crop, unsigned* __restrict__ max_bits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  float m = 0.f;
  if (i < cw * ch) {
    const int x = i % cw, y = i / cw;
    const size_t n = (size_t)S * S, cn = (size_t)cw * ch;
    for (int f = 0; f < 4; ++f) {
      const float v = field[f * n + (size_t)(y0 + y) * S + (x0 + x)];
      crop[(size_t)(f >> 1) * 2 * cn + 2 * (size_t)i + (f & 1)] = v;  // interleaved pairs: (flow x, flow y), (iflow x, iflow y)
      if (f >= 2 && v == v) m = fmaxf(m, fabsf(v));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(max_bits, __float_as_uint(m));  // non-negative floats order as uints
}

// Background warp field: CImg resize(2W, 2H, -100, -100, 3) then *= 2 (DG:1197-1200), linear
// interpolation, X pass then Y pass, each pass rounded to float (CImg 2.x linear resize,
// boundary 0, upscaling branch).  off/foff tables come from the host.
__global__ __launch_bounds__(256) void wf_resize2_kernel(const float* __restrict__ crop, int cw, int ch, int sx, int sy,
                                                         const int* __restrict__ xi, const double* __restrict__ xa,
                                                         const int* __restrict__ yi, const double* __restrict__ ya,
                                                         float* __restrict__ out, unsigned* __restrict__ max_bits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  float m = 0.f;
  if (i < sx * sy) {
    const int x = i % sx, y = i / sx;
    const size_t cn = (size_t)cw * ch, on = (size_t)sx * sy;
    const int x1 = xi[x], x2 = min(x1 + 1, cw - 1);
    const int y1 = yi[y], y2 = min(y1 + 1, ch - 1);
    const double ax = xa[x], ay = ya[y];
    for (int f = 0; f < 4; ++f) {
      const float* p = crop + (size_t)(f >> 1) * 2 * cn + (f & 1);  // (interleaved pairs, as wf_crop_kernel writes them)
      const float r1 = (float)((1 - ax) * (double)p[2 * ((size_t)y1 * cw + x1)] + ax * (double)p[2 * ((size_t)y1 * cw + x2)]);
      const float r2 = (float)((1 - ax) * (double)p[2 * ((size_t)y2 * cw + x1)] + ax * (double)p[2 * ((size_t)y2 * cw + x2)]);
      const float v = (float)((1 - ay) * (double)r1 + ay * (double)r2);
      const float v2 = (float)((double)v * 2.);
      out[(size_t)(f >> 1) * 2 * on + 2 * (size_t)i + (f & 1)] = v2;
      if (f >= 2 && v2 == v2) m = fmaxf(m, fabsf(v2));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(max_bits, __float_as_uint(m));
}

// --------------------------------------------------------------------------
// texture pool kernels (BGRX u32 texels)
// --------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ uint32_t lattice(uint32_t seed, uint32_t tex, uint32_t c, uint32_t oct, uint32_t ix, uint32_t iy) {
  uint32_t h = mix32(seed ^ 0x9e3779b9u);
  h = mix32(h ^ (tex * 0x632be5abu + 1u));
  h = mix32(h ^ (c * 0x1b873593u + oct * 0xcc9e2d51u + 7u));
  h = mix32(h ^ (ix * 0x27d4eb2fu));
  h = mix32(h ^ (iy * 0x165667b1u));
  return h & 255u;
}
// Synthetic texture = 3 octaves of integer value noise (cell sizes 64, 16, 4; weights
// 4:2:1), i.e. a smooth field with fine detail so that bilinear filtering and LSB
// errors are visible.  Pure integer arithmetic: reproducible anywhere.
// Background texture preparation (ofdg_params.background_prep = 1): one thread per texel of the
// sample's 2W x 2H texture; see DevBgPrep.  Texture::getRandomizedCrop, DG:87-109 (CImg chain
// restated as one resampling; parity unpinned).  Strict fp32, same operation order as the oracle.
__device__ __forceinline__ float cimg_modf(float x, float m) { return (float)((double)x - (double)m * floor((double)x / (double)m)); }
__device__ __forceinline__ int mirror_index(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;  // (in range: no division)
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - m - 1;
}
// R(x, y) of CImg's rotate(angle, 1, 3) for xc = x - rw2, yc = y - rh2, on the SHIFTED pool image (strict fp32, the
// oracle's operation order): mirrored float coordinates, _linear_atXY (Neumann), truncation to u8 per channel
__device__ __forceinline__ uint32_t bgprep_rot_sample(const DevBgPrep& p, float xc, float yc) {
  OFDG_GLOBAL const uint32_t* img = (OFDG_GLOBAL const uint32_t*)p.image_addr;
  const int pw = p.pw, ph = p.ph;
  const float ww = 2.0f * pw, hh = 2.0f * ph;
  float mx = __fadd_rn(__fadd_rn(p.w2, __fmul_rn(xc, p.ca)), __fmul_rn(yc, p.sa));
  float my = __fadd_rn(__fsub_rn(p.h2, __fmul_rn(xc, p.sa)), __fmul_rn(yc, p.ca));
  if (!(mx >= 0.f && mx < ww)) mx = cimg_modf(mx, ww);  // (cimg::mod is the identity on [0, m))
  if (!(my >= 0.f && my < hh)) my = cimg_modf(my, hh);
  mx = mx < (float)pw ? mx : __fsub_rn(__fsub_rn(ww, mx), 1.0f);
  my = my < (float)ph ? my : __fsub_rn(__fsub_rn(hh, my), 1.0f);
  // _linear_atXY (Neumann) on the shifted image
  const float nfx = mx <= 0 ? 0.f : (mx >= (float)(pw - 1) ? (float)(pw - 1) : mx);
  const float nfy = my <= 0 ? 0.f : (my >= (float)(ph - 1) ? (float)(ph - 1) : my);
  const int x = (int)nfx, y = (int)nfy;
  const float dx = __fsub_rn(nfx, (float)x), dy = __fsub_rn(nfy, (float)y);
  const int nx = dx > 0 ? x + 1 : x, ny = dy > 0 ? y + 1 : y;
  // texel (i, j) of the shifted image = pool texel (mirror(i - shx), mirror(j - shy)); for
  // 0 <= shift <= size the mirror of a negative index -k is k - 1
  auto shifted = [](int i, int sh, int n) { const int j = i - sh; return (sh >= 0 && sh <= n) ? (j < 0 ? -j - 1 : j) : mirror_index(j, n); };
  const int xa = shifted(x, p.shx, pw), xb = shifted(nx, p.shx, pw);
  const int ya = shifted(y, p.shy, ph), yb = shifted(ny, p.shy, ph);
  const uint32_t ra = (uint32_t)ya * (uint32_t)pw, rb = (uint32_t)yb * (uint32_t)pw;
  const uint32_t tcc = img[ra + xa], tnc = img[ra + xb], tcn = img[rb + xa], tnn = img[rb + xb];
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sh = 8 * c;
    const float Icc = (float)((tcc >> sh) & 255u), Inc = (float)((tnc >> sh) & 255u);
    const float Icn = (float)((tcn >> sh) & 255u), Inn = (float)((tnn >> sh) & 255u);
    // Icc + dx*(Inc - Icc + dy*(Icc + Inn - Icn - Inc)) + dy*(Icn - Icc)
    const float t = __fsub_rn(__fsub_rn(__fadd_rn(Icc, Inn), Icn), Inc);
    const float val = __fadd_rn(__fadd_rn(Icc, __fmul_rn(dx, __fadd_rn(__fsub_rn(Inc, Icc), __fmul_rn(dy, t)))), __fmul_rn(dy, __fsub_rn(Icn, Icc)));
    out |= (uint32_t)(unsigned char)val << sh;
  }
  return out;
}
// background_prep = 2 (fast form): one prepared texel by ONE resampling along the composed coordinate map
__device__ __forceinline__ uint32_t bgprep_texel(const DevBgPrep& p, int u, int v) {
  const float cxf = fminf((float)(p.cw - 1), __fmul_rn((float)u, p.fx)), cyf = fminf((float)(p.ch - 1), __fmul_rn((float)v, p.fy));
  const float xc = __fsub_rn(__fadd_rn((float)p.x0, cxf), p.rw2), yc = __fsub_rn(__fadd_rn((float)p.y0, cyf), p.rh2);
  return bgprep_rot_sample(p, xc, yc);
}

// ---- background_prep = 1: the CImg chain stage by stage (DG:96-103), four u8 images -------------------------------
//   C = crop(rotate(shift(T)))  cw x ch   bgprep_rotcrop_kernel (shift, rotate and crop are per-texel maps: fused, exact)
//   M = resize of C along x     2W x ch   } bgprep_resize_kernel: every texel of B evaluates the one or two (enlarging) or
//   B = resize of M along y     2W x 2H   } few (moving average) texels of M it needs from C, rounded to u8 as CImg stores them
// Only what compose can read of B (DevBgPrep.r*) is produced, and of C what that needs.
// CImg's enlarging tables (source index and weight of every destination pixel: running double sums, curr = min(n - 1,
// curr + f), sequential by definition) depend on the source and destination lengths only: the host tabulates them once
// for every source length below the destination's (ofdg_api.hip ensure_bgprep_tables): entry [n * S + x].
struct DevResizeTabs {
  const uint16_t* at_x;    // [2W][2W]
  const double* alpha_x;
  const uint16_t* at_y;    // [2H][2H]
  const double* alpha_y;
};
// source range [lo, hi] a resize pass reads for destination pixels d0..d1 (n source, s destination pixels)
__device__ __forceinline__ void cimg_resize_range(int n, int s, int d0, int d1, const uint16_t* __restrict__ at, int* lo, int* hi) {
  if (s > n) { *lo = at[(size_t)n * s + d0]; *hi = min((int)at[(size_t)n * s + d1] + 1, n - 1); }
  else if (s == n) { *lo = d0; *hi = d1; }
  else { *lo = (d0 * n) / s; *hi = ((d1 + 1) * n - 1) / s; }
}
// the region of C (columns cx0..cx1, rows cy0..cy1) the sample's visible part of B needs; false: the crop does not fit the workspace
__device__ __forceinline__ bool bgprep_region(const DevBgPrep& p, const DevResizeTabs& T, int TW, int TH, int cap_cw, int cap_ch,
                                              int* cx0, int* cx1, int* cy0, int* cy1) {
  if (!(p.cw >= 1 && p.ch >= 1 && p.cw <= cap_cw && p.ch <= cap_ch)) return false;
  cimg_resize_range(p.ch, TH, p.ry0, p.ry1, T.at_y, cy0, cy1);
  cimg_resize_range(p.cw, TW, p.rx0, p.rx1, T.at_x, cx0, cx1);
  return true;
}
// Two horizontally adjacent texels of C at once: R(x, y) of bgprep_rot_sample for (xc0, yc) and (xc1, yc), the same
// strict-fp32 operations per texel, evaluated on float pairs (v_pk_mul_f32 / v_pk_add_f32: one instruction for both), and
// - when no lane of the wave leaves the image (no mirroring, no clamping: the usual case, the rotation is a few degrees) -
// without the wrap logic.
struct RotPair { f32x2 mx, my; };
// mx = (w2 + xc * ca) + yc * sa;  my = (h2 - xc * sa) + yc * ca   (element-wise: exactly the scalar sequence)
__device__ __forceinline__ RotPair bgprep_rot_coords(const DevBgPrep& p, float xc0, float xc1, float yc) {
  const f32x2 xc = {xc0, xc1};
  RotPair r;
  // (w2, h2 as opaque scalars: read straight into the vector initialisers the two loads become vector loads of the record,
  //  which keep a copy of the record's floats in private memory - scratch traffic in the middle of the callers' loops)
  float w2 = p.w2, h2 = p.h2;
  asm("" : "+v"(w2), "+v"(h2));
  r.mx = (f32x2{w2, w2} + xc * f32x2{p.ca, p.ca}) + f32x2{__fmul_rn(yc, p.sa), __fmul_rn(yc, p.sa)};
  r.my = (f32x2{h2, h2} - xc * f32x2{p.sa, p.sa}) + f32x2{__fmul_rn(yc, p.ca), __fmul_rn(yc, p.ca)};
  return r;
}
__device__ __forceinline__ bool bgprep_shift_plain(const DevBgPrep& p) { return p.shx >= 0 && p.shx <= p.pw && p.shy >= 0 && p.shy <= p.ph; }
// Both texels lie inside [0, pw - 1) x [0, ph - 1) of the rotated image's source coordinates (mod, mirror and the Neumann
// clamp are identities, x + 1 and y + 1 exist) and the shift is plain (0 <= shift <= size).
// the strict-fp32 bilinear form of bgprep_rot_sample for two texels at once (taps cc / nc / cn / nn of texel 0 and 1, their
// fractions as float pairs): Icc + dx*(Inc - Icc + dy*(Icc + Inn - Icn - Inc)) + dy*(Icn - Icc), truncated to u8 per channel
__device__ __forceinline__ uint2 rot_blend2(uint32_t cc0, uint32_t nc0, uint32_t cn0, uint32_t nn0, uint32_t cc1, uint32_t nc1, uint32_t cn1, uint32_t nn1,
                                            f32x2 dx, f32x2 dy) {
  uint2 out = make_uint2(0, 0);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int b = 8 * c;
    f32x2 Icc = {(float)((cc0 >> b) & 255u), (float)((cc1 >> b) & 255u)}, Inc = {(float)((nc0 >> b) & 255u), (float)((nc1 >> b) & 255u)};
    f32x2 Icn = {(float)((cn0 >> b) & 255u), (float)((cn1 >> b) & 255u)}, Inn = {(float)((nn0 >> b) & 255u), (float)((nn1 >> b) & 255u)};
    // (opaque: differences of converted bytes are exact, and where two taps are visibly halves of ONE load the compiler subtracts
    //  the bytes as integers and converts the differences - 30 more instructions per texel pair, none of them packed)
    asm("" : "+v"(Icc), "+v"(Inc), "+v"(Icn), "+v"(Inn));
    const f32x2 t = ((Icc + Inn) - Icn) - Inc;
    const f32x2 val = (Icc + dx * ((Inc - Icc) + dy * t)) + dy * (Icn - Icc);
    out.x |= (uint32_t)(unsigned char)val.x << b;
    out.y |= (uint32_t)(unsigned char)val.y << b;
  }
  return out;
}
template <class PairFn>
__device__ __forceinline__ uint2 bgprep_rot_inside2_t(const DevBgPrep& p, const RotPair& r, bool second, PairFn pair) {
  const f32x2 mx = r.mx, my = r.my;
  const int x0i = (int)mx.x, y0i = (int)my.x, x1i = (int)mx.y, y1i = (int)my.y;
  const f32x2 dx = mx - f32x2{(float)x0i, (float)x1i}, dy = my - f32x2{(float)y0i, (float)y1i};
  // The neighbours are ALWAYS x + 1 and y + 1 here: where dx (dy) is 0 the scalar form reads the texel itself instead, but
  // the neighbour's weight is then an exact zero and the value the same.  Texel (i, j) of the shifted image = pool texel
  // (mirror(i - shx), mirror(j - shy)), for 0 <= shift <= size -k -> k - 1: x and x + 1 are neighbours in the pool too
  // (ascending, descending left of the mirror line, or twice texel 0 across it), so ONE 8-byte load per row fetches both.
  // pair(row, col): pool texels (col, row) and (col + 1, row).
  auto sh = [](int i, int s_) { const int j = i - s_; return j < 0 ? -j - 1 : j; };
  auto row_pair = [&](int xi, int ya, int yb, uint32_t* cc, uint32_t* nc, uint32_t* cn, uint32_t* nn) {
    const int j = xi - p.shx;
    const int base = j >= 0 ? j : max(-j - 2, 0);
    const uint2 r0 = pair(ya, base), r1 = pair(yb, base);
    const bool rev = j < 0, swap = j < -1;
    *cc = swap ? r0.y : r0.x; *nc = rev ? r0.x : r0.y;
    *cn = swap ? r1.y : r1.x; *nn = rev ? r1.x : r1.y;
  };
  uint32_t cc0, nc0, cn0, nn0, cc1 = 0, nc1 = 0, cn1 = 0, nn1 = 0;
  row_pair(x0i, sh(y0i, p.shy), sh(y0i + 1, p.shy), &cc0, &nc0, &cn0, &nn0);
  if (second) row_pair(x1i, sh(y1i, p.shy), sh(y1i + 1, p.shy), &cc1, &nc1, &cn1, &nn1);
  return rot_blend2(cc0, nc0, cn0, nn0, cc1, nc1, cn1, nn1, dx, dy);
}
// ... with the taps fetched from the pool image in memory
__device__ __forceinline__ uint2 bgprep_rot_inside2(const DevBgPrep& p, const RotPair& r, bool second) {
  const char* imgc = (const char*)p.image_addr;
  const uint32_t upw = (uint32_t)p.pw;
  return bgprep_rot_inside2_t(p, r, second, [&](int row, int col) { return gload2(imgc, (__umul24((uint32_t)row, upw) + (uint32_t)col) * 4u); });
}
__device__ __forceinline__ uint2 bgprep_rot_sample2(const DevBgPrep& p, float xc0, float xc1, float yc, bool second) {
  const int pw = p.pw, ph = p.ph;
  const RotPair r = bgprep_rot_coords(p, xc0, xc1, yc);
  const bool in0 = r.mx.x >= 0.f && r.mx.x < (float)(pw - 1) && r.my.x >= 0.f && r.my.x < (float)(ph - 1);
  const bool in1 = !second || (r.mx.y >= 0.f && r.mx.y < (float)(pw - 1) && r.my.y >= 0.f && r.my.y < (float)(ph - 1));
  if (__ballot(!(in0 && in1)) != 0ull || !bgprep_shift_plain(p))
    return make_uint2(bgprep_rot_sample(p, xc0, yc), second ? bgprep_rot_sample(p, xc1, yc) : 0u);
  return bgprep_rot_inside2(p, r, second);
}
// C(i, j) = R(mirror(x0 + i), mirror(y0 + j)), R = rotate(shift(T)); sample blockIdx.y; a thread takes texel PAIRS
__global__ __launch_bounds__(256) void bgprep_rotcrop_kernel(const DevBgPrep* __restrict__ prep, DevResizeTabs T, int W, int H,
                                                             int cap_cw, int cap_ch, uint32_t* __restrict__ C, uint32_t* __restrict__ err) {
  const int s = blockIdx.y;
  const DevBgPrep p = prep[s];
  int cx0, cx1, cy0, cy1;
  if (!bgprep_region(p, T, 2 * W, 2 * H, cap_cw, cap_ch, &cx0, &cx1, &cy0, &cy1)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, kErrBgPrepCapacity);
    return;
  }
  const int rw_ = cx1 - cx0 + 1, rh_ = cy1 - cy0 + 1;
  const int pairs = (rw_ + 1) / 2;  // texel pairs per row of the region
  uint32_t* Cs = C + (size_t)s * cap_cw * cap_ch;
  const float inv_pairs = 1.0f / (float)pairs;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < pairs * rh_; k += gridDim.x * blockDim.x) {  // (the region's size is only known on the device)
    int jj = (int)((float)k * inv_pairs);  // k / pairs (k < 2^22: the float quotient is off by one at most)
    int pi = k - jj * pairs;
    if (pi < 0) { --jj; pi += pairs; } else if (pi >= pairs) { ++jj; pi -= pairs; }
    const int j = cy0 + jj, i = cx0 + 2 * pi;
    const bool second = i + 1 <= cx1;
    const int rx0 = mirror_index(p.x0 + i, p.rw), rx1 = mirror_index(p.x0 + i + 1, p.rw), ry = mirror_index(p.y0 + j, p.rh);
    const float xc0 = __fsub_rn((float)rx0, p.rw2), xc1 = __fsub_rn((float)rx1, p.rw2), yc = __fsub_rn((float)ry, p.rh2);
    const uint2 v = bgprep_rot_sample2(p, xc0, xc1, yc, second);
    const uint32_t o = (uint32_t)(j * p.cw + i);
    Cs[o] = v.x;
    if (second) Cs[o + 1] = v.y;
  }
}
// a / d correctly rounded for operands that need none of the IEEE division's range handling (here 0 <= a < 2^31,
// 1 <= d < 2^16): the compiler's own expansion of a / d - v_rcp_f32, two fma on the reciprocal, a product and four fma on
// the quotient - without v_div_scale / v_div_fixup, and with the reciprocal's part computed once per divisor.
struct UniformDivisor { float d, r; };
__device__ __forceinline__ UniformDivisor make_divisor(float d) {
  const float r0 = __builtin_amdgcn_rcpf(d);
  return {d, __fmaf_rn(__fmaf_rn(-d, r0, 1.f), r0, r0)};
}
__device__ __forceinline__ float div_rn(float a, const UniformDivisor& u) {
  float q = __fmul_rn(a, u.r);
  q = __fmaf_rn(__fmaf_rn(-u.d, q, a), u.r, q);
  return __fmaf_rn(__fmaf_rn(-u.d, q, a), u.r, q);
}
// one axis of CImg's linear get_resize on BGRX texels: destination pixel k of a line whose source texels are texel(j),
// j < n; sdim = destination length.  Enlarging: (T)((1 - a) * v1 + a * v2) in double; shrinking: moving average over the
// n * sdim grid in float, / n, truncated; same length: copy.
// (double)u for u < 2^32 without v_cvt_f64_u32 (9 issue cycles against 5 for an addition, tools/microbench/f64_rates.hip):
// the bits of 2^52 + u, minus 2^52 - exact
__device__ __forceinline__ double u32_to_double(uint32_t u) { return __hiloint2double(0x43300000, (int)u) - 4503599627370496.0; }
// `at` / `alpha`: the enlarging tables' rows of THIS source length (the caller adds n * sdim once: uniform per sample)
template <class Texel>
__device__ __forceinline__ uint32_t cimg_resize_texel(int n, int sdim, int k, const uint16_t* __restrict__ at, const double* __restrict__ alpha,
                                                      Texel texel) {
  uint32_t out = 0;
  if (sdim == n) {
    out = texel(k);
  } else if (sdim > n) {
    const int a0 = at[(uint32_t)k];
    const double al = alpha[(uint32_t)k], al1 = 1 - al;
    const uint32_t t1 = texel(a0), t2 = a0 < n - 1 ? texel(a0 + 1) : t1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v1 = u32_to_double((t1 >> (8 * c)) & 255u), v2 = u32_to_double((t2 >> (8 * c)) & 255u);
      out |= (uint32_t)(unsigned char)(al1 * v1 + al * v2) << (8 * c);
    }
  } else {
    float acc[3] = {0.f, 0.f, 0.f};
    const int lo = k * n, hi = lo + n;  // (< 2^31: both lengths are a few thousand at most)
    for (int j = lo / sdim; j * sdim < hi; ++j) {
      const int a = j * sdim, b = a + sdim;
      const float d = (float)((b < hi ? b : hi) - (a > lo ? a : lo));
      const uint32_t t = texel(j);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn((float)((t >> (8 * c)) & 255u), d));
    }
    const UniformDivisor dn = make_divisor((float)n);
#pragma unroll
    for (int c = 0; c < 3; ++c) out |= (uint32_t)(unsigned char)div_rn(acc[c], dn) << (8 * c);
  }
  return out;
}
// B(x, y) = Y-resize of M(x, .), M(x, j) = X-resize of C(., j); M never touches memory.  The kernel is bound by its
// arithmetic (≈ 100 VALU instructions per texel, 12 M texels per batch), so a thread renders kResizeRun consecutive rows
// of one column and evaluates every row of M they share ONCE (one more than the run when enlarging, at most 4/3 of it
// + 1 when shrinking), parked in the thread's own LDS column - an indexable scratch: registers cannot be indexed by a
// run-time row.  (Issuing a run's loads together, or four texels per thread in bgprep_rotcrop_kernel, made both
// kernels slower: profiles/r02_ab_background_prep_kernels.txt.)
constexpr int kResizeRun = 4, kResizeMaxM = 8;
__global__ __launch_bounds__(256) void bgprep_resize_kernel(const DevBgPrep* __restrict__ prep, DevResizeTabs T, int W, int H, int cap_cw,
                                                            int cap_ch, const uint32_t* __restrict__ C, uint32_t* __restrict__ B) {
  __shared__ uint32_t s_m[kResizeMaxM][256];
  const int s = blockIdx.y, TW = 2 * W, TH = 2 * H, tid = threadIdx.x;
  const DevBgPrep p = prep[s];
  if (!(p.cw >= 1 && p.ch >= 1 && p.cw <= cap_cw && p.ch <= cap_ch)) return;
  const int rw_ = p.rx1 - p.rx0 + 1, rh_ = p.ry1 - p.ry0 + 1;
  const int runs = (rh_ + kResizeRun - 1) / kResizeRun;
  const uint32_t* Cs = C + (size_t)s * cap_cw * cap_ch;
  uint32_t* Bs = B + (size_t)s * TW * TH;
  // the enlarging tables' rows of this sample's source lengths (entry [n * S + x]: uniform bases, 32-bit indices below)
  const uint16_t* at_x = T.at_x + (size_t)p.cw * TW;
  const double* alpha_x = T.alpha_x + (size_t)p.cw * TW;
  const uint16_t* at_y = T.at_y + (size_t)p.ch * TH;
  const double* alpha_y = T.alpha_y + (size_t)p.ch * TH;
  const float inv_rw = 1.0f / (float)rw_;
  for (int k = blockIdx.x * blockDim.x + tid; k < runs * rw_; k += gridDim.x * blockDim.x) {
    int rr = (int)((float)k * inv_rw);  // k / rw_ (k < 2^22: the float quotient is off by one at most)
    int xo = k - rr * rw_;
    if (xo < 0) { --rr; xo += rw_; } else if (xo >= rw_) { ++rr; xo -= rw_; }
    const int x = p.rx0 + xo, y0 = p.ry0 + rr * kResizeRun, y1 = min(y0 + kResizeRun - 1, p.ry1);
    auto c_row = [&](int j) {  // M(x, j)
      return cimg_resize_texel(p.cw, TW, x, at_x, alpha_x, [&](int i) { return Cs[(uint32_t)(j * p.cw + i)]; });
    };
    int jlo, jhi;
    cimg_resize_range(p.ch, TH, y0, y1, T.at_y, &jlo, &jhi);
    if (jhi - jlo < kResizeMaxM) {
#pragma unroll
      for (int m = 0; m < kResizeMaxM; ++m)
        if (jlo + m <= jhi) s_m[m][tid] = c_row(jlo + m);
#pragma unroll
      for (int r = 0; r < kResizeRun; ++r)
        if (y0 + r <= y1) Bs[(uint32_t)((y0 + r) * TW + x)] = cimg_resize_texel(p.ch, TH, y0 + r, at_y, alpha_y, [&](int j) { return s_m[j - jlo][tid]; });
    } else {  // (a crop beyond 4/3 of the texture is refused before it gets here; kept for safety)
      for (int y = y0; y <= y1; ++y) Bs[(uint32_t)(y * TW + x)] = cimg_resize_texel(p.ch, TH, y, at_y, alpha_y, c_row);
    }
  }
}

// ---- the same chain in ONE launch (pool images at least 2W x 2H: a crop is at most 4/3 of the texture) ------------------
// bgprep_stream_kernel: ONE WAVE renders a 64 x kPrepH tile of B = the sample's 2W x 2H texture by walking the tile's rows of
// C = crop(rotate(shift(T))) once, top to bottom, kPrepG rows at a time:
//   rotation   the group's texels of C are sampled into kPrepG LDS rows (texel pairs, two rounds of gathers in flight);
//   X resize   lane = column x of the tile computes M(x, j) from LDS row j into a REGISTER; the last three rows of M stay
//              (m0, m1, m2);
//   Y resize   source rows are monotone in y, so every row y of B whose last source row is j is complete as soon as M(., j)
//              exists: it is computed from the register window and stored.
// C lives in 8.4 KB of LDS per wave, M never exists outside registers, B goes to memory once; no barrier between waves, one
// pass over the tile, and a tile may be as tall as one likes (its rows of C are streamed; a taller tile recomputes fewer seam
// rows: 2 of kPrepH / zoom + 2).  The tiles of all samples are numbered consecutively (their count per sample is only known
// on the device) and handed out grid-stride to kPrepGrid single-wave workgroups (ofdg_api.hip; a bench batch has fewer tiles
// than that: one tile per wave).
// Round 5 replaced the round-4 form with it (two-wave workgroups, a 64 x 16 tile's whole piece of C in 9 KB of LDS through
// three barrier-separated passes; tools/patches/r05_bgprep_experiment_switches.patch): +3 - 4 % on the headline step in same-box
// A/Bs (profiles/r05_experiments_log.md section 2), no __syncthreads between waves, no cap on a tile's rows.  What decides its
// speed is the LENGTH OF A WAVE'S DEPENDENT CHAIN per tile - rounds of gathers, then LDS, then stores, and a gather behind a
// store waits for that store too (vmcnt counts loads and stores in issue order) - so rows are sampled in groups of 24: most
// tiles are two groups (groups of 4 / 8: -6 % / -3 %; 16 / 20: the same step with compose's launch 10 us longer; 28: -4 %;
// 44 rows = 16 KB of LDS: -14 %), the next round's gathers are requested before this round is blended (three rounds in
// flight: 98 registers, -4 %), and a tile is 32 rows (24: faster alone, slower in the step; 16 / 64: -10 %).
constexpr int kPrepW = 64;                      // columns of B per tile: lane = column
constexpr int kPrepH = 32;                      // rows of B per tile (<= 64: lane r holds row r's resize entry)
constexpr int kPrepG = 24;                      // rows of C sampled per group
constexpr int kPrepRun = 16;                    // consecutive tiles that share an XCD (the kernel's blockIdx -> tile mapping)
constexpr int kPrepCW = 90;                     // columns of C a tile needs at most: 64 * 4/3 + 2, even (texel pairs), + the margin of the crop size
#ifndef OFDG_PREP_DIRS
#define OFDG_PREP_DIRS 1
#endif
#ifndef OFDG_PREP_FAST_RESIZE
#define OFDG_PREP_FAST_RESIZE 1
#endif
constexpr bool kPrepFastResize = OFDG_PREP_FAST_RESIZE != 0;  // the resize passes specialised by a tile's case (both axes enlarge / shrink)
#ifndef OFDG_PREP_ROUND2
#define OFDG_PREP_ROUND2 1
#endif
constexpr bool kPrepDirs = OFDG_PREP_DIRS != 0;  // the rotation specialised by a tile's side of the shift's mirror lines
constexpr int kPrepMaxSamples = 512;            // (the counter sampler's batch limit; ofdg_api.hip falls back to the two-kernel form beyond)
// A tile's placement costs small dependent loads - which sample holds tile t (prefix of the samples' tile counts: LDS),
// that sample's record, the four resize-table entries that bound the tile's piece of C - so a workgroup that has another
// tile to do requests those for the NEXT tile (scalar loads) at the top of this tile's turn.
struct PrepTile {
  int s;                    // sample; n_samples: no tile left
  int bx0, bx1, by0, by1;   // texels of B the tile renders
  int cx0, cx1, cy0, cy1;   // texels of C it needs
  int fits;                 // ... which fit the LDS tile of C
  int inside;               // no mirroring / clamping anywhere in the tile: the per-texel range tests are skipped
  int xdir, ydir;           // ... and where the tile lies relative to the shift's mirror lines: 1 = every tap right of / below the line
                            // (pool index = i - shift), 2 = every tap left of / above it (pool index = shift - 1 - i), 0 = per lane
};
__host__ __device__ __forceinline__ bool prep_sample_fits(const DevBgPrep& q, int cap_cw, int cap_ch) { return q.cw >= 1 && q.ch >= 1 && q.cw <= cap_cw && q.ch <= cap_ch; }  // (caps <= 4/3 of the texture + 2)
__host__ __device__ __forceinline__ int prep_tile_cols(const DevBgPrep& q) { return (q.rx1 - q.rx0 + kPrepW) / kPrepW; }
__host__ __device__ __forceinline__ int prep_tile_rows(const DevBgPrep& q) { return (q.ry1 - q.ry0 + kPrepH) / kPrepH; }
// cimg_resize_range with the two table entries it reads already in hand (e0 = at[n * s + d0], e1 = at[n * s + d1])
__device__ __forceinline__ void prep_range(int n, int s, int d0, int d1, int e0, int e1, int* lo, int* hi) {
  if (s > n) { *lo = e0; *hi = min(e1 + 1, n - 1); }
  else if (s == n) { *lo = d0; *hi = d1; }
  else { *lo = (d0 * n) / s; *hi = ((d1 + 1) * n - 1) / s; }
}
// the tile's piece of C and whether the whole of it maps inside the source image (S3)
__device__ __forceinline__ void prep_finish_tile(const DevBgPrep& p, PrepTile& F, int TW, int TH, int ex0, int ex1, int ey0, int ey1) {
  prep_range(p.cw, TW, F.bx0, F.bx1, ex0, ex1, &F.cx0, &F.cx1);
  prep_range(p.ch, TH, F.by0, F.by1, ey0, ey1, &F.cy0, &F.cy1);
  const int cx0 = F.cx0, cx1 = F.cx1, cy0 = F.cy0, cy1 = F.cy1;
  F.fits = cx1 - cx0 + 1 <= kPrepCW ? 1 : 0;  // (rows are streamed: any number of them)
  // The usual tile: its crop coordinates need no mirroring and its four corners - so, the map being affine, all its texels
  // (a margin of one texel covers the rounding of the per-texel evaluation) - lie inside the source image: no per-texel tests.
  bool inside = F.fits && bgprep_shift_plain(p) && p.x0 + cx0 >= 0 && p.x0 + cx1 + 1 < p.rw && p.y0 + cy0 >= 0 && p.y0 + cy1 < p.rh;
  int xdir = 0, ydir = 0;
  if (inside) {
    const float xa = __fsub_rn((float)(p.x0 + cx0), p.rw2), xb = __fsub_rn((float)(p.x0 + cx1 + 1), p.rw2);
    const float ya = __fsub_rn((float)(p.y0 + cy0), p.rh2), yb = __fsub_rn((float)(p.y0 + cy1), p.rh2);
    const RotPair ra = bgprep_rot_coords(p, xa, xb, ya), rb = bgprep_rot_coords(p, xa, xb, yb);
    const float lo_x = fminf(fminf(ra.mx.x, ra.mx.y), fminf(rb.mx.x, rb.mx.y)), hi_x = fmaxf(fmaxf(ra.mx.x, ra.mx.y), fmaxf(rb.mx.x, rb.mx.y));
    const float lo_y = fminf(fminf(ra.my.x, ra.my.y), fminf(rb.my.x, rb.my.y)), hi_y = fmaxf(fmaxf(ra.my.x, ra.my.y), fmaxf(rb.my.x, rb.my.y));
    inside = lo_x >= 1.f && hi_x < (float)(p.pw - 2) && lo_y >= 1.f && hi_y < (float)(p.ph - 2);
    // a tap's column is floor(mx) (and + 1), mx within [lo_x, hi_x] up to the rounding the margin of one texel covers
    xdir = lo_x - 1.f >= (float)p.shx ? 1 : (hi_x + 3.f <= (float)p.shx ? 2 : 0);
    ydir = lo_y - 1.f >= (float)p.shy ? 1 : (hi_y + 3.f <= (float)p.shy ? 2 : 0);
  }
  F.inside = __builtin_amdgcn_readfirstlane(inside ? 1 : 0);  // (wave-uniform by construction)
  F.xdir = __builtin_amdgcn_readfirstlane(inside ? xdir : 0);
  F.ydir = __builtin_amdgcn_readfirstlane(inside ? ydir : 0);
}
// ---- the resize passes in exact INTEGER arithmetic --------------------------------------------------------------------------
// Enlarging: CImg evaluates (T)((1 - a) v1 + a v2) in double.  Where the weight a has at most 45 fractional bits - every
// table entry whose source position is >= 128: the weight is `curr - floor(curr)` of a double `curr`, which then has at most
// 52 - 7 fractional bits - 1 - a is exact, both products (8-bit integer x 45 fractional bits: 53 bits) are exact and so is
// their sum (below 256): the double result IS the real number v1 + a (v2 - v1), and its truncation is
//     v1 + floor(d A / 2^45),  d = v2 - v1,  A = a 2^45 = A1 2^23 + A0:
//     d A = (d A1 + floor(d A0 / 2^23)) 2^23 + r,  0 <= r < 2^23   =>   floor(d A / 2^45) = (d A1 + (d A0 >> 23)) >> 22
// (arithmetic shifts; |d A0| < 2^31, |d A1| < 2^30): two 24-bit multiplies, two shifts, two additions per channel instead of
// two conversions, two fp64 products, an fp64 sum and a conversion.  Entries that are not exact keep the double form.
// Shrinking: CImg's float moving average sum(v_j w_j) / n, truncated.  The sum is an integer below 2^24 (weights are overlap
// lengths, sum n <= 4/3 of 1024..2048): exact in float; the correctly rounded quotient of an integer by n < 2^13 cannot round
// up to the next integer (it is at least 1 / n below it, half an ulp at 255 is 2^-17): the byte is floor(sum / n), in integers
// sum via v_mad_u32_u24 and the division by a multiply-high with M = ceil(2^32 / n) (exact for sum < 2^19 n / ... : the
// error sum e / 2^32 < 2^-13 < 1 / n).
struct FixWeight { int a1, a0; bool exact; };
__device__ __forceinline__ FixWeight fix_weight(double al) {
  const double t = ldexp(al, 45);           // (exact: a power of two)
  const double u = floor(ldexp(t, -23));    // floor(a 2^22)
  FixWeight w;
  w.exact = al >= 0.0 && al < 1.0 && t == floor(t);
  w.a1 = (int)u;
  w.a0 = (int)(t - ldexp(u, 23));           // (exact when w.exact; unused otherwise)
  return w;
}
__device__ __forceinline__ uint32_t enlarge_texel_fix(uint32_t t1, uint32_t t2, int a1, int a0) {
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v1 = (int)((t1 >> (8 * c)) & 255u), d = (int)((t2 >> (8 * c)) & 255u) - v1;
    const int m = (__mul24(d, a1) + (__mul24(d, a0) >> 23)) >> 22;
    out |= (uint32_t)(v1 + m) << (8 * c);
  }
  return out;
}
// Shrinking by less than half (n <= 2 sdim: what a tile of the one-launch form holds, prep_sample_fits): destination texel k averages the source
// interval [k n, (k + 1) n) in units of 1 / sdim, which touches at most THREE source texels j0, j0 + 1, j0 + 2 with overlap
// lengths d0 > 0, d1, d2 >= 0 (sum n).  The taps depend on (n, sdim, k) only: once per column of a tile in the X pass, once
// per row in the Y pass (scalar) - not per texel.
struct ShrinkTaps { int j0; uint32_t d0, d1, d2; };
__device__ __forceinline__ ShrinkTaps shrink_taps(int n, int sdim, int k) {
  const int lo = k * n, hi = lo + n;  // (< 2^31: both lengths are a few thousand at most)
  ShrinkTaps t;
  t.j0 = lo / sdim;
  const int a = t.j0 * sdim;
  t.d0 = (uint32_t)(min(a + sdim, hi) - lo);
  t.d1 = (uint32_t)min(max(hi - (a + sdim), 0), sdim);
  t.d2 = (uint32_t)min(max(hi - (a + 2 * sdim), 0), sdim);
  return t;
}
// floor(acc / n) for acc <= 255 n as a multiply-high by mdiv = ceil(2^32 / n) = 2^32 / n + e, 0 <= e < 1: the product is
// 2^32 (acc / n + acc e / 2^32), and the excess acc e / 2^32 < 255 n / 2^32 stays below the 1 / n that separates acc / n from the
// next integer as long as 255 n^2 < 2^32: n <= 4103 (crops of frames up to 1536 wide).  With n > 256 both factors are also
// below 2^24: the full-rate 24-bit multiply-high instead of the quarter-rate 32-bit one.  Any other n: 32-bit multiply-high
// (one too large at most) and a correction.
__device__ __forceinline__ bool shrink_div24(int n) { return n > 256 && n <= 4103; }
__device__ __forceinline__ uint32_t mulhi_u24(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// bgprep_rot_inside2 in two halves - the four 8-byte gathers of a texel pair requested, and the pair blended - so that the
// next pair's gathers can be in flight while this one is blended
// kXD / kYD: the tile's side of the shift's mirror lines when it is the same for every tap (PrepTile.xdir / ydir; 0: per lane).
// Right of the line a tap's pool column is i - shx and its neighbour's the next one: the 8-byte load IS (cc, nc); left of it the
// columns descend (shx - 1 - i): the load at the neighbour's column is (nc, cc).  Rows likewise (y + 1 is the row below or above).
struct RotTaps { uint2 a0, a1, b0, b1; f32x2 dx, dy; int ja, jb; };
template <int kXD = 0, int kYD = 0>
__device__ __forceinline__ RotTaps rot_issue(const DevBgPrep& p, const RotPair& r) {
  const char* imgc = (const char*)p.image_addr;
  const uint32_t upw = (uint32_t)p.pw;
  const f32x2 mx = r.mx, my = r.my;
  const int x0i = (int)mx.x, y0i = (int)my.x, x1i = (int)mx.y, y1i = (int)my.y;
  RotTaps t;
  t.dx = mx - f32x2{(float)x0i, (float)x1i};
  t.dy = my - f32x2{(float)y0i, (float)y1i};
  auto pair = [&](int row, int col) { return gload2(imgc, (__umul24((uint32_t)row, upw) + (uint32_t)col) * 4u); };
  t.ja = x0i - p.shx; t.jb = x1i - p.shx;
  int basea, baseb;
  if (kXD == 1) { basea = t.ja; baseb = t.jb; }
  else if (kXD == 2) { basea = -t.ja - 2; baseb = -t.jb - 2; }
  else { basea = t.ja >= 0 ? t.ja : max(-t.ja - 2, 0); baseb = t.jb >= 0 ? t.jb : max(-t.jb - 2, 0); }
  int ra0, ra1, rb0, rb1;  // pool rows of texel a's and b's upper and lower taps
  if (kYD == 1) { ra0 = y0i - p.shy; ra1 = ra0 + 1; rb0 = y1i - p.shy; rb1 = rb0 + 1; }
  else if (kYD == 2) { ra0 = p.shy - 1 - y0i; ra1 = ra0 - 1; rb0 = p.shy - 1 - y1i; rb1 = rb0 - 1; }
  else {
    auto sh = [](int i, int s_) { const int j = i - s_; return j < 0 ? -j - 1 : j; };
    ra0 = sh(y0i, p.shy); ra1 = sh(y0i + 1, p.shy); rb0 = sh(y1i, p.shy); rb1 = sh(y1i + 1, p.shy);
  }
  t.a0 = pair(ra0, basea); t.a1 = pair(ra1, basea);
  t.b0 = pair(rb0, baseb); t.b1 = pair(rb1, baseb);
  return t;
}
template <int kXD = 0>
__device__ __forceinline__ uint2 rot_finish(const RotTaps& t) {
  if (kXD == 1) return rot_blend2(t.a0.x, t.a0.y, t.a1.x, t.a1.y, t.b0.x, t.b0.y, t.b1.x, t.b1.y, t.dx, t.dy);
  if (kXD == 2) return rot_blend2(t.a0.y, t.a0.x, t.a1.y, t.a1.x, t.b0.y, t.b0.x, t.b1.y, t.b1.x, t.dx, t.dy);
  const bool reva = t.ja < 0, swapa = t.ja < -1, revb = t.jb < 0, swapb = t.jb < -1;
  const uint32_t cc0 = swapa ? t.a0.y : t.a0.x, nc0 = reva ? t.a0.x : t.a0.y, cn0 = swapa ? t.a1.y : t.a1.x, nn0 = reva ? t.a1.x : t.a1.y;
  const uint32_t cc1 = swapb ? t.b0.y : t.b0.x, nc1 = revb ? t.b0.x : t.b0.y, cn1 = swapb ? t.b1.y : t.b1.x, nn1 = revb ? t.b1.x : t.b1.y;
  return rot_blend2(cc0, nc0, cn0, nn0, cc1, nc1, cn1, nn1, t.dx, t.dy);
}
// entry [idx] of a resize table of 16-bit entries, for a uniform idx, as ONE scalar load (the tables are constant while the
// kernel runs; there is no scalar load of 16 bits: the dword that holds the entry, hipMalloc'ed base)
__device__ __forceinline__ int tab_entry_uniform(const uint16_t* at, uint32_t idx) {
  const uint32_t w = ((OFDG_CONSTANT const uint32_t*)at)[idx >> 1];
  return (int)((w >> ((idx & 1u) * 16u)) & 0xffffu);
}
// One destination pixel's share of a resize axis (n source, sdim destination pixels) in three registers - the kernel keeps one
// per lane for its column and one per lane for "its" row all through a tile, so they are packed:
//   enlarging   u0 = source index a0, u1 = A1, u2 = A0 | exact << 31   (fix_weight of the table's alpha; not exact: u1 = u2 = 0)
//   same size   u0 = k
//   shrinking   u0 = first source index j0, u1 = d0, u2 = d1           (shrink_taps; d2 = n - d0 - d1)
struct AxisEntry { int u0; uint32_t u1, u2; };
__device__ __forceinline__ AxisEntry axis_entry(int n, int sdim, int k, const uint16_t* __restrict__ at, const double* __restrict__ alpha) {
  AxisEntry e{k, 0u, 0u};
  if (sdim > n) {
    const uint32_t i = (uint32_t)(n * sdim + k);
    e.u0 = at[i];
    const FixWeight w = fix_weight(alpha[i]);
    if (w.exact) { e.u1 = (uint32_t)w.a1; e.u2 = (uint32_t)w.a0 | 0x80000000u; }
  } else if (sdim < n) {
    const ShrinkTaps t = shrink_taps(n, sdim, k);
    e.u0 = t.j0; e.u1 = t.d0; e.u2 = t.d1;
  }
  return e;
}
// the last source index the pixel needs
__device__ __forceinline__ int axis_last(int n, int sdim, int u0, uint32_t u1, uint32_t u2) {
  if (sdim > n) return min(u0 + 1, n - 1);
  if (sdim == n) return u0;
  return u0 + ((uint32_t)n - u1 - u2 > 0u ? 2 : (u2 > 0u ? 1 : 0));
}
// ... and its value from the source texels t0, t1, t2 at u0, u0 + 1, u0 + 2 (clamped by the caller to what exists; enlarging
// reads t0, t1 - t1 = t0 in the last source pixel -, same size t0).  `exact`: u1 / u2 hold the weight (uniform); otherwise
// CImg's double form with the table's alpha[k] loaded here (entries at source positions below 128: rare).
__device__ __forceinline__ uint32_t axis_texel(int n, int sdim, int k, uint32_t u1, uint32_t u2, bool exact, uint32_t t0, uint32_t t1, uint32_t t2,
                                               uint32_t mdiv, bool div24, const double* __restrict__ alpha) {
  if (sdim > n) {
    if (exact) return enlarge_texel_fix(t0, t1, (int)u1, (int)(u2 & 0x7fffffffu));
    const double al = alpha[(uint32_t)(n * sdim + k)], al1 = 1 - al;
    uint32_t out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v1 = u32_to_double((t0 >> (8 * c)) & 255u), v2 = u32_to_double((t1 >> (8 * c)) & 255u);
      out |= (uint32_t)(unsigned char)(al1 * v1 + al * v2) << (8 * c);
    }
    return out;
  }
  if (sdim == n) return t0;
  const uint32_t d0 = u1, d1 = u2, d2 = (uint32_t)n - u1 - u2;
  uint32_t acc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    acc[c] = __umul24((t2 >> (8 * c)) & 255u, d2) + (__umul24((t1 >> (8 * c)) & 255u, d1) + __umul24((t0 >> (8 * c)) & 255u, d0));
  if (div24) return mulhi_u24(acc[0], mdiv) | (mulhi_u24(acc[1], mdiv) << 8) | (mulhi_u24(acc[2], mdiv) << 16);
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint32_t q = __umulhi(acc[c], mdiv);
    q -= (q * (uint32_t)n > acc[c]) ? 1u : 0u;
    out |= q << (8 * c);
  }
  return out;
}
// paths (diagnostics, nullptr in production): 9 counters of tiles by the form that rendered them, [rotation + 3 * resize]: rotation
// 0 = general (off the `inside` fast path), 1 = inside, side of the mirror lines decided per lane, 2 = inside and specialised by
// side; resize 0 = decided per row, 1 = both axes enlarge, 2 = both shrink
__global__ __launch_bounds__(64) void bgprep_stream_kernel(const DevBgPrep* __restrict__ prep, DevResizeTabs T, int W, int H, int n_samples,
                                                           int cap_cw, int cap_ch, uint32_t* __restrict__ B, uint32_t* __restrict__ err,
                                                           uint32_t* __restrict__ paths) {
  __shared__ uint32_t s_c[kPrepG][kPrepCW];
  extern __shared__ int s_first[];  // [n_samples + 1]: tiles of the samples before sample i
  const int TW = 2 * W, TH = 2 * H, lane = threadIdx.x;
  {  // the tiles of all samples are numbered consecutively: prefix of their counts, 64 samples at a time
    int running = 0;
    if (lane == 0) s_first[0] = 0;
    for (int c = 0; c < n_samples; c += 64) {
      const int i = c + lane;
      int nt = 0;
      if (i < n_samples) {
        const DevBgPrep& q = prep[i];
        const bool fits = prep_sample_fits(q, cap_cw, cap_ch);
        if (!fits && blockIdx.x == 0) atomicOr(err, kErrBgPrepCapacity);
        nt = fits ? prep_tile_cols(q) * prep_tile_rows(q) : 0;
      }
      const int incl = wave_scan_incl(nt);
      if (i < n_samples) s_first[i + 1] = running + incl;
      running += __shfl(incl, 63, 64);
    }
  }
  __syncthreads();
  const int total = __builtin_amdgcn_readfirstlane(s_first[n_samples]);
  // the sample that holds tile t: the number of samples whose tiles end at or before t (64 samples per ballot)
  auto sample_of = [&](int t) {
    int n = 0;
    for (int c = 0; c < n_samples; c += 64) {
      const int i = c + lane;
      n += __popcll(__ballot(i < n_samples && t >= s_first[i + 1]));
    }
    return __builtin_amdgcn_readfirstlane(n);
  };
  auto tab_index = [](int n, int dim, int k) { return (uint32_t)(n < dim ? n * dim + k : 0); };
  struct PrepBox { int cw, ch, rx0, ry0, rx1, ry1; };
  typedef OFDG_CONSTANT const DevBgPrep ConstPrep;  // (records are constant while this kernel runs: scalar loads)
  auto box_fields = [&](int s) { const ConstPrep& q = ((ConstPrep*)prep)[s]; return PrepBox{q.cw, q.ch, q.rx0, q.ry0, q.rx1, q.ry1}; };
  auto box_of = [&](const PrepBox& q, int t, int s, PrepTile& F) {  // the tile's texels of B
    const int tcols = (q.rx1 - q.rx0 + kPrepW) / kPrepW;
    const int ti = t - __builtin_amdgcn_readfirstlane(s_first[s]), ty = ti / tcols, tx = ti - ty * tcols;
    F.s = s;
    F.bx0 = q.rx0 + tx * kPrepW; F.bx1 = min(F.bx0 + kPrepW - 1, q.rx1);
    F.by0 = q.ry0 + ty * kPrepH; F.by1 = min(F.by0 + kPrepH - 1, q.ry1);
  };
  // Workgroups are dealt to the 8 XCDs round-robin.  Runs of kPrepRun consecutive tiles - neighbours in a sample's tile row and
  // the row below: they share the source lines under their seams - go to ONE XCD, so that what one tile fetched the next finds
  // in that XCD's L2: the kernel's memory-side reads fall from 45.7 to 28.7 MB per batch (FETCH_SIZE; 64-tile runs: 24.8 MB but a
  // worse balance), the step gains 0.6 % (profiles/r05_ab_prep_xcd_runs*.txt).  (The tail of a grid that is no multiple of
  // 8 runs keeps its order.)
  int t = blockIdx.x;
  if (t < (int)(gridDim.x / (8 * kPrepRun)) * (8 * kPrepRun)) {
    const int xcd = t & 7, slot = t >> 3;
    t = ((slot / kPrepRun) * 8 + xcd) * kPrepRun + (slot % kPrepRun);
  }
  if (t >= total) return;
  PrepTile cur;
  int ex0, ex1, ey0, ey1;  // the four table entries that bound the tile's piece of C (requested one tile ahead)
  {
    const int s0 = sample_of(t);
    const PrepBox q = box_fields(s0);
    box_of(q, t, s0, cur);
    ex0 = tab_entry_uniform(T.at_x, tab_index(q.cw, TW, cur.bx0)); ex1 = tab_entry_uniform(T.at_x, tab_index(q.cw, TW, cur.bx1));
    ey0 = tab_entry_uniform(T.at_y, tab_index(q.ch, TH, cur.by0)); ey1 = tab_entry_uniform(T.at_y, tab_index(q.ch, TH, cur.by1));
  }
  for (;;) {
    // ---- this tile's sample record, the placement of the next tile and the entries that bound ITS piece of C: scalar loads,
    // requested here, used at the top of the next turn ----
    const int tn = t + (int)gridDim.x;
    const bool more = tn < total;
    const int sc = __builtin_amdgcn_readfirstlane(cur.s);
    const int sn = more ? sample_of(tn) : sc;
    const DevBgPrep p = ((ConstPrep*)prep)[sc];
    const PrepBox qn = box_fields(sn);
    prep_finish_tile(p, cur, TW, TH, ex0, ex1, ey0, ey1);
    const int bx0 = cur.bx0, bx1 = cur.bx1, by0 = cur.by0, by1 = cur.by1;
    const int cx0 = cur.cx0, cx1 = cur.cx1, cy0 = cur.cy0, cy1 = cur.cy1;
    const int ncw = cx1 - cx0 + 1, nch = cy1 - cy0 + 1;
    // this tile's resize entries: column bx0 + lane (the X pass), row by0 + lane (the Y pass: lane r holds row r's)
    const int x = bx0 + lane;
    const bool have_x = x <= bx1;
    const AxisEntry ex = axis_entry(p.cw, TW, min(x, bx1), T.at_x, T.alpha_x);
    const AxisEntry ey = axis_entry(p.ch, TH, min(by0 + lane, by1), T.at_y, T.alpha_y);
    PrepTile nxt = cur;
    int nx0 = 0, nx1 = 0, ny0 = 0, ny1 = 0;
    if (more) {
      box_of(qn, tn, sn, nxt);
      nx0 = tab_entry_uniform(T.at_x, tab_index(qn.cw, TW, nxt.bx0)); nx1 = tab_entry_uniform(T.at_x, tab_index(qn.cw, TW, nxt.bx1));
      ny0 = tab_entry_uniform(T.at_y, tab_index(qn.ch, TH, nxt.by0)); ny1 = tab_entry_uniform(T.at_y, tab_index(qn.ch, TH, nxt.by1));
    }
    if (!cur.fits) {  // (a crop beyond 4/3 of the texture: the host launches the two-kernel form for such pools)
      if (lane == 0) atomicOr(err, kErrBgPrepCapacity);
    } else {
      const bool x_exact = __ballot(have_x && TW > p.cw && !(ex.u2 >> 31)) == 0ull;  // (the wave's columns all have exact weights: uniform)
      const uint32_t xdiv = 0xFFFFFFFFu / (uint32_t)p.cw + 1u, ydiv = 0xFFFFFFFFu / (uint32_t)p.ch + 1u;
      const bool xdiv24 = shrink_div24(p.cw), ydiv24 = shrink_div24(p.ch);
      // LDS columns of the X pass's three taps (clamped to what the tile holds; a clamped tap has weight 0 or is not read)
      const int xi0 = ex.u0 - cx0;
      const int xi1 = (TW > p.cw ? min(ex.u0 + 1, p.cw - 1) : min(ex.u0 + 1, cx1)) - cx0, xi2 = min(ex.u0 + 2, cx1) - cx0;
      const int ylastv = axis_last(p.ch, TH, ey.u0, ey.u1, ey.u2);
      uint32_t* Bs = B + (size_t)cur.s * TW * TH;
      // the tile's resize case (uniform): both axes enlarge with exact weights in every column and row of the tile / both shrink
      // with 24-bit quotients
      const bool y_exact = __ballot(lane <= by1 - by0 && TH > p.ch && !(ey.u2 >> 31)) == 0ull;
      const bool fast_enlarge = TW > p.cw && TH > p.ch && x_exact && y_exact;
      const bool fast_shrink = TW < p.cw && TH < p.ch && xdiv24 && ydiv24;
      if (paths && lane == 0)
        atomicAdd(&paths[(cur.inside ? ((kPrepDirs && cur.xdir && cur.ydir) ? 2 : 1) : 0) + 3 * (kPrepFastResize ? (fast_enlarge ? 1 : fast_shrink ? 2 : 0) : 0)], 1u);
      uint32_t m0 = 0, m1 = 0, m2 = 0;  // M(x, j - 2), M(x, j - 1), M(x, j)
      int y = by0;                      // the next row of B to emit ...
      int ylast = __builtin_amdgcn_readlane(ylastv, 0);  // ... and the last row of M it needs
      const int pairs = (ncw + 1) / 2;
      const uint32_t inv_pairs = (1u << 20) / (uint32_t)pairs + 1u;  // k / pairs = (k * inv) >> 20, exact for k <= 45 * 48
      for (int g0 = 0; g0 < nch; g0 += kPrepG) {
        const int rows = min(kPrepG, nch - g0);
        const int items = pairs * rows;
        // ---- rotation: C(cx0 + 2 pi .., cy0 + g0 + jj), texel pairs ----
        if (cur.inside) {
          // two rounds in flight: the next round's four gathers are requested before this round's texels are blended
          auto rotate = [&](auto xd, auto yd) {
            constexpr int kXD = decltype(xd)::value, kYD = decltype(yd)::value;
            auto issue = [&](int k) {
              const int jj = (int)(__umul24((uint32_t)k, inv_pairs) >> 20);
              const int pi = k - jj * pairs;
              const int xi = p.x0 + cx0 + 2 * pi;
              return rot_issue<kXD, kYD>(p, bgprep_rot_coords(p, __fsub_rn((float)xi, p.rw2), __fsub_rn((float)(xi + 1), p.rw2), __fsub_rn((float)(p.y0 + cy0 + g0 + jj), p.rh2)));
            };
#if OFDG_PREP_ROUND2
            // a round = TWO pairs per lane (k and k + 64), all eight gathers requested before the first wait: one exposed round trip
            // per four texels, uniform control flow (the last round's lanes beyond the end repeat the last pair), no set of taps copied
            for (int k0 = 0; k0 < items; k0 += 128) {
              const int ka = min(k0 + lane, items - 1), kb = min(k0 + 64 + lane, items - 1);
              const RotTaps ta = issue(ka);
              const RotTaps tb = issue(kb);
              const int ja = (int)(__umul24((uint32_t)ka, inv_pairs) >> 20), jb = (int)(__umul24((uint32_t)kb, inv_pairs) >> 20);
              *reinterpret_cast<uint2*>(&s_c[ja][2 * (ka - ja * pairs)]) = rot_finish<kXD>(ta);
              *reinterpret_cast<uint2*>(&s_c[jb][2 * (kb - jb * pairs)]) = rot_finish<kXD>(tb);
            }
          };
#else
            RotTaps tcur = issue(min(lane, items - 1));
            for (int k = lane; k < items; k += 64) {
              const int kn = k + 64;
              RotTaps tnext = tcur;
              if (kn < items) tnext = issue(kn);
              const int jj = (int)(__umul24((uint32_t)k, inv_pairs) >> 20);
              const int pi = k - jj * pairs;
              *reinterpret_cast<uint2*>(&s_c[jj][2 * pi]) = rot_finish<kXD>(tcur);  // (the odd texel beyond an odd-width region is inside too; nobody reads it)
              tcur = tnext;
            }
          };
#endif
          // (a tile lies on ONE side of the shift's mirror lines unless a line crosses it: the per-lane selects and mirrored
          //  indices of the general form drop out - 140 instead of 168 vector instructions per texel pair)
          using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
          if (kPrepDirs && cur.xdir == 1 && cur.ydir == 1) rotate(I1{}, I1{});
          else if (kPrepDirs && cur.xdir == 2 && cur.ydir == 1) rotate(I2{}, I1{});
          else if (kPrepDirs && cur.xdir == 1 && cur.ydir == 2) rotate(I1{}, I2{});
          else if (kPrepDirs && cur.xdir == 2 && cur.ydir == 2) rotate(I2{}, I2{});
          else rotate(I0{}, I0{});
        } else {
          // (the rare general form - mirrored crop coordinates, modulo, clamps: an opaque copy of the record's sizes, so that nothing it
          //  derives from them - floats, doubles of the image size - is computed in front of the tile and held through the fast forms)
          DevBgPrep q = p;
          asm volatile("" : "+s"(q.pw), "+s"(q.ph), "+s"(q.rw), "+s"(q.rh), "+s"(q.shx), "+s"(q.shy));
          for (int k = lane; k < items; k += 64) {
            const int jj = (int)(__umul24((uint32_t)k, inv_pairs) >> 20);
            const int pi = k - jj * pairs;
            const int i = cx0 + 2 * pi, j = cy0 + g0 + jj;
            const bool second = i + 1 <= cx1;
            const int rx0 = mirror_index(q.x0 + i, q.rw), rx1 = mirror_index(q.x0 + i + 1, q.rw), ry = mirror_index(q.y0 + j, q.rh);
            const float xc0 = __fsub_rn((float)rx0, q.rw2), xc1 = __fsub_rn((float)rx1, q.rw2), yc = __fsub_rn((float)ry, q.rh2);
            *reinterpret_cast<uint2*>(&s_c[jj][2 * pi]) = bgprep_rot_sample2(q, xc0, xc1, yc, second);
          }
        }
        __syncthreads();  // (one wave: the rows are complete before its lanes read their neighbours' texels)
        // ---- X resize into the register window, and every row of B that is complete with it ----
        // The general loop decides per row what its axis does (enlarge with an exact weight / in double, copy, shrink with a 24-bit
        // or a 32-bit quotient): a chain of uniform branches per row of C and per row of B.  A sample's zoom makes BOTH axes
        // enlarge (zoom > 1) or BOTH shrink (zoom < 1), and all weights of a tile compose can see are exact: the two loops
        // below are those two cases with nothing to decide inside (round 6; the resize passes are 40 % of the kernel's time).
        auto emit_rows = [&](int j, auto value) {  // every row y of B whose last source row is j
          while (y <= by1 && ylast <= j) {
            const int rr = y - by0;
            const int v0 = __builtin_amdgcn_readlane(ey.u0, rr);
            const uint32_t v1 = (uint32_t)__builtin_amdgcn_readlane((int)ey.u1, rr), v2 = (uint32_t)__builtin_amdgcn_readlane((int)ey.u2, rr);
            const uint32_t v = value(j - v0, v1, v2);
            // (non-temporal like compose's planes: written once here, read once by the next kernel - +3.5 % on the step over plain
            //  stores, profiles/r05_ab_nt_intermediate_stores.txt; raster's coverage bytes: no difference)
            if (have_x) __builtin_nontemporal_store(v, &Bs[(uint32_t)(y * TW + x)]);
            ++y;
            ylast = y <= by1 ? __builtin_amdgcn_readlane(ylastv, y - by0) : 0x7fffffff;
          }
        };
        if (kPrepFastResize && fast_enlarge) {
          const int xa1 = (int)ex.u1, xa0 = (int)(ex.u2 & 0x7fffffffu);
          for (int r = 0; r < rows; ++r) {
            const uint32_t t0 = s_c[r][xi0], t1 = s_c[r][xi1];
            m1 = m2;
            m2 = enlarge_texel_fix(t0, t1, xa1, xa0);
            // rows v0, v0 + 1 of M: the row's last source row j is v0 + 1, or v0 in the last row of M
            emit_rows(cy0 + g0 + r, [&](int dj, uint32_t v1, uint32_t v2) { return enlarge_texel_fix(dj >= 1 ? m1 : m2, m2, (int)v1, (int)(v2 & 0x7fffffffu)); });
          }
        } else if (kPrepFastResize && fast_shrink) {
          const uint32_t xd0 = ex.u1, xd1 = ex.u2, xd2 = (uint32_t)p.cw - ex.u1 - ex.u2;
          auto shrink24 = [](uint32_t t0, uint32_t t1, uint32_t t2, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t mdiv) {
            uint32_t acc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
              acc[c] = __umul24((t2 >> (8 * c)) & 255u, d2) + (__umul24((t1 >> (8 * c)) & 255u, d1) + __umul24((t0 >> (8 * c)) & 255u, d0));
            return mulhi_u24(acc[0], mdiv) | (mulhi_u24(acc[1], mdiv) << 8) | (mulhi_u24(acc[2], mdiv) << 16);
          };
          for (int r = 0; r < rows; ++r) {
            const uint32_t t0 = s_c[r][xi0], t1 = s_c[r][xi1], t2 = s_c[r][xi2];
            m0 = m1; m1 = m2;
            m2 = shrink24(t0, t1, t2, xd0, xd1, xd2, xdiv);
            // rows v0 .. v0 + 2 of M, clamped to j: j is v0 + 2, or v0 + 1 where the third tap has no weight
            emit_rows(cy0 + g0 + r, [&](int dj, uint32_t v1, uint32_t v2) {
              const uint32_t t0y = dj >= 2 ? m0 : (dj == 1 ? m1 : m2), t1y = dj >= 2 ? m1 : m2;
              return shrink24(t0y, t1y, m2, v1, v2, (uint32_t)p.ch - v1 - v2, ydiv);
            });
          }
        } else {
        int xg = x, cwg = p.cw, chg = p.ch;  // (opaque: see the general rotation above)
        asm volatile("" : "+v"(xg), "+s"(cwg), "+s"(chg));
        for (int r = 0; r < rows; ++r) {
          const int j = cy0 + g0 + r;
          m0 = m1; m1 = m2;
          m2 = have_x ? axis_texel(cwg, TW, xg, ex.u1, ex.u2, x_exact, s_c[r][xi0], s_c[r][xi1], s_c[r][xi2], xdiv, xdiv24, T.alpha_x) : 0u;
          emit_rows(j, [&](int dj, uint32_t v1, uint32_t v2) {
            // rows v0, v0 + 1, v0 + 2 of M (uniform), clamped to j = the row's last source row: the window holds j - 2 .. j
            // (enlarging: j is v0 + 1, or v0 in the last row of M; shrinking: v0 + 2, or v0 + 1 where the third tap has no weight)
            uint32_t t0 = m2, t1 = m2;
            if (dj >= 2) { t0 = m0; t1 = m1; } else if (dj == 1) { t0 = m1; }
            return axis_texel(chg, TH, y, v1, v2, (v2 >> 31) != 0u, t0, t1, m2, ydiv, ydiv24, T.alpha_y);
          });
        }
        }
        __syncthreads();  // (the next group overwrites the rows)
      }
    }
    if (!more) break;
    ex0 = nx0; ex1 = nx1; ey0 = ny0; ey1 = ny1;
    cur = nxt;
    t = tn;
  }
}

// one thread = 4 consecutive texels of a row of sample blockIdx.y's texture; texels outside the
// sample's read region (DevBgPrep.r*) are skipped - compose never looks at them
__global__ __launch_bounds__(256) void bgprep_kernel(const DevBgPrep* __restrict__ prep, int W, int H, uint32_t* __restrict__ bgtex) {
  const int TW = 2 * W, TH = 2 * H, quads = TW / 4;
  const int s = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= quads * TH) return;
  const int v = i / quads, u0 = (i - v * quads) * 4;
  const DevBgPrep p = prep[s];
  if (v < p.ry0 || v > p.ry1 || u0 + 3 < p.rx0 || u0 > p.rx1) return;
  uint4 o;
  o.x = bgprep_texel(p, u0, v);
  o.y = bgprep_texel(p, u0 + 1, v);
  o.z = bgprep_texel(p, u0 + 2, v);
  o.w = bgprep_texel(p, u0 + 3, v);
  *reinterpret_cast<uint4*>(bgtex + (size_t)s * TW * TH + (size_t)v * TW + u0) = o;
}

__global__ __launch_bounds__(256) void pool_synth_kernel(uint32_t* __restrict__ pool, int n, int w, int h, uint32_t seed) {
  const size_t total = (size_t)n * w * h;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t tex = (uint32_t)(i / ((size_t)w * h));
    const uint32_t rem = (uint32_t)(i - (size_t)tex * w * h);
    const uint32_t y = rem / w, x = rem - y * w;
    uint32_t px = 0;
    for (uint32_t c = 0; c < 3; ++c) {
      uint32_t acc = 0;
      for (uint32_t oct = 0; oct < 3; ++oct) {
        const uint32_t sh = 6 - 2 * oct, cs = 1u << sh;
        const uint32_t ix = x >> sh, iy = y >> sh, fx = x & (cs - 1), fy = y & (cs - 1);
        const uint32_t l00 = lattice(seed, tex, c, oct, ix, iy), l10 = lattice(seed, tex, c, oct, ix + 1, iy);
        const uint32_t l01 = lattice(seed, tex, c, oct, ix, iy + 1), l11 = lattice(seed, tex, c, oct, ix + 1, iy + 1);
        const uint32_t v = (l00 * (cs - fx) * (cs - fy) + l10 * fx * (cs - fy) + l01 * (cs - fx) * fy + l11 * fx * fy) >> (2 * sh);
        acc += v << (2 - oct);
      }
      px |= ((acc + 3) / 7) << (8 * c);
    }
    pool[i] = px;
  }
}
__global__ __launch_bounds__(256) void pool_pack_kernel(const uint8_t* __restrict__ planar, uint32_t* __restrict__ dst, int w, int h) {
  const size_t n = (size_t)w * h;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = (uint32_t)planar[i] | ((uint32_t)planar[n + i] << 8) | ((uint32_t)planar[2 * n + i] << 16);
}
__global__ __launch_bounds__(256) void pool_unpack_kernel(const uint32_t* __restrict__ src, uint8_t* __restrict__ planar, int w, int h) {
  const size_t n = (size_t)w * h;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t p = src[i];
    planar[i] = p & 255; planar[n + i] = (p >> 8) & 255; planar[2 * n + i] = (p >> 16) & 255;
  }
}

// CImg<unsigned char>::get_resize(.., 3) along ONE axis of every image of a BGRX pool (the
// reference resizes pool images that are smaller than the texture it needs, DG:102-106).
// Enlarging: linear, table `at` = source index, `alpha` = weight (CImg's running double sums, built
// on the host); value (T)((1 - a) * v1 + a * v2).  Shrinking (at == nullptr): moving average over
// the w*s grid in float, / w, truncated.  dst images are ow x oh, src w x h.
__global__ __launch_bounds__(256) void pool_resize_axis_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int n_images,
                                                               int w, int h, int s, int along_x, const int* __restrict__ at,
                                                               const double* __restrict__ alpha) {
  const int ow = along_x ? s : w, oh = along_x ? h : s;
  const size_t per = (size_t)ow * oh, total = per * n_images;
  const int n = along_x ? w : h;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / per, r = i - img * per;
    const int x = (int)(r % ow), y = (int)(r / ow);
    const int k = along_x ? x : y, line = along_x ? y : x;
    const uint32_t* sp = src + img * (size_t)w * h;
    auto texel = [&](int j) { return along_x ? sp[(size_t)line * w + j] : sp[(size_t)j * w + line]; };
    uint32_t out = 0;
    if (at) {
      const int a0 = at[k];
      const double al = alpha[k];
      const uint32_t t1 = texel(a0), t2 = a0 < n - 1 ? texel(a0 + 1) : t1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v1 = (double)((t1 >> (8 * c)) & 255u), v2 = (double)((t2 >> (8 * c)) & 255u);
        out |= (uint32_t)(unsigned char)((1 - al) * v1 + al * v2) << (8 * c);
      }
    } else {
      // destination k integrates [k*n, (k+1)*n) of the n*s grid; source j covers [j*s, (j+1)*s)
      float acc[3] = {0.f, 0.f, 0.f};
      const long long lo = (long long)k * n, hi = lo + n;
      for (int j = (int)(lo / s); (long long)j * s < hi; ++j) {
        const long long a = (long long)j * s, b = a + s;
        const float d = (float)((b < hi ? b : hi) - (a > lo ? a : lo));
        const uint32_t t = texel(j);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn((float)((t >> (8 * c)) & 255u), d));
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) out |= (uint32_t)(unsigned char)__fdiv_rn(acc[c], (float)n) << (8 * c);
    }
    dst[i] = out;
  }
}

// include/ofdg_detmath.h evaluated on the device (tests: device == host bit for bit)
// Debug entries of the tests: the device's curve flattening and span interpolator on caller-given doubles.
// (path: one wave, the same path_verts the outlines go through; writes the vertices + their number)
__global__ __launch_bounds__(64) void debug_path_kernel(const double* __restrict__ xy, const int* __restrict__ types, int n_seg,
                                                        int2* __restrict__ verts, int* __restrict__ n_out, uint32_t* __restrict__ err) {
  __shared__ double s_stack[kCurveSlots][kCurveMaxDepth][5];
  __shared__ int2 s_stage[kCurveSlots][kCurveMaxPts];
  const int lane = (int)threadIdx.x;
  int minx = 0x7FFFFFFF, miny = 0x7FFFFFFF, maxx = (int)0x80000000, maxy = (int)0x80000000;
  const int n = path_verts(n_seg, [&](int i) { return types[i]; }, [&](int i, double& x, double& y) { x = xy[2 * i]; y = xy[2 * i + 1]; },
                           verts, s_stack, s_stage, err, lane, minx, miny, maxx, maxy);
  if (lane == 0) *n_out = n;
}
// (span interpolator: make_row + dda_at of `rows` output rows of length `len` under the inverse affine `inv`)
__global__ void debug_dda_kernel(Mat inv, int rows, int len, int2* __restrict__ out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= rows * len) return;
  const int y = i / len, x = i - y * len;
  const int nshift = ((len & (len - 1)) == 0) ? (31 - __clz(len)) : -1;
  const RowDDA R = make_row(inv, y, len, nshift);
  out[i] = make_int2(dda_at(R.x1, R.lx, R.rx, len, nshift, x), dda_at(R.y1, R.ly, R.ry, len, nshift, x));
}

// ofdg_poll_errors / ofdg_poll_errors_of: read and clear n device error words in one step (one wave), *out = their OR
__global__ void err_exchange_kernel(uint32_t* __restrict__ d_err, int n, uint32_t* __restrict__ out) {
  uint32_t e = 0;
  for (int i = (int)threadIdx.x; i < n; i += 64) e |= atomicExch(d_err + i, 0u);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) e |= (uint32_t)__shfl_xor((int)e, d, 64);
  if (threadIdx.x == 0) *out = e;
}

__global__ void detmath_kernel(const double* __restrict__ a, int n, double* __restrict__ s, double* __restrict__ c,
                               const float* __restrict__ x, int m, float* __restrict__ e) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ofdg_det_sincos(a[i], s + i, c + i);
  if (i < m) e[i] = ofdg_det_expf(x[i]);
}

// exhaustive probe of the per-byte device formulas (tests): tables of 65536 entries
__global__ void tables_kernel(uint8_t* add_tbl, uint8_t* sub_tbl, uint8_t* aa_tbl, uint8_t* blend_tbl /*256*256 for s=200? no: d,m with s fixed*/, int s_fixed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 65536) return;
  const int u = i >> 8, v = i & 255;
  add_tbl[i] = (uint8_t)comp_add(u, v);
  sub_tbl[i] = (uint8_t)comp_sub(u, v);
  blend_tbl[i] = (uint8_t)((blend_px((uint32_t)u * 0x00010101u, (uint32_t)s_fixed * 0x00010101u, (uint32_t)v) >> 16) & 255u);  // d = u, m = v (R lane)
  if (((blend_px((uint32_t)u * 0x00010101u, (uint32_t)s_fixed * 0x00010101u, (uint32_t)v)) & 255u) != (uint32_t)blend(u, s_fixed, v) || ((blend_px((uint32_t)u * 0x00010101u, (uint32_t)s_fixed * 0x00010101u, (uint32_t)v) >> 8) & 255u) != (uint32_t)blend(u, s_fixed, v)) blend_tbl[i] = 0xEE;  // all three lanes must agree with the scalar form
  if (i < 256) aa_tbl[i] = (uint8_t)aa_byte(i);
}

// --------------------------------------------------------------------------
// Plane accessors of the post-processing kernels below: how a lane reads and writes its QUAD - four adjacent pixels of one
// row of one plane - in each storage format.  The format rules, stated once (the host twins in csrc/ofdg_device.h and
// csrc/host_api.cpp hold the same):
//   flow       float32 (16 bytes a quad), binary16 (8 bytes) or - flow_error's estimate only - bfloat16 (8 bytes, err_bf16),
//              widened to float32; usable where both components are below 2^20 in magnitude (flow_usable: a NaN is not),
//              finite where the exponent is not all ones (flow_finite).
//   image      uint8 (one 4-byte word, pixel p in byte p) or float32 (16 bytes) taken to a byte by photo_index: clamped to
//              [0, 255], a NaN to 0, ties to even.  A byte goes back as itself or as (float)byte.
//   occlusion  uint8 (4 bytes) or float32 (16 bytes): a pixel is hidden where its element is NON-ZERO (a NaN is hidden, -0.0
//              is not).
// A quad_* function takes a ready pointer to the lane's first element - the address arithmetic, 32-bit or size_t, stays with
// the kernel, which knows its guard - and issues one load or store instruction of the quad's size; the elem_* forms read one
// element at the caller's index, in the caller's index type.  Stores of whole pieces are non-temporal: the planes are read
// next by another kernel.  A new op reads and writes its planes through these.
// --------------------------------------------------------------------------
constexpr int quad_fmt(bool half) { return half ? OFDG_FMT_F16 : OFDG_FMT_F32; }
template <int kFmt> struct FlowFmt;  // the element and the quad of a flow format, for the kernel's pointer arithmetic
template <> struct FlowFmt<OFDG_FMT_F32> { typedef float elem; typedef f32x4 quad; };
template <> struct FlowFmt<OFDG_FMT_F16> { typedef _Float16 elem; typedef f16x4 quad; };
template <> struct FlowFmt<OFDG_FMT_BF16> { typedef uint16_t elem; typedef u32x2 quad; };
__device__ __forceinline__ bool flow_finite(float x) { return mblur_finite(x); }            // (the twins' names, as the
__device__ __forceinline__ bool flow_usable(float u, float v) { return vis_usable(u, v); }  // ops that came first left them)
template <int kFmt>  // OFDG_FMT_F32, OFDG_FMT_F16 or OFDG_FMT_BF16
__device__ __forceinline__ void quad_load(const void* p4, float (&o)[4]) {
  if constexpr (kFmt == OFDG_FMT_F16) {
    const f16x4 a = *static_cast<const f16x4*>(p4);
#pragma unroll
    for (int p = 0; p < 4; ++p) o[p] = (float)a[p];
  } else if constexpr (kFmt == OFDG_FMT_BF16) {
    const u32x2 a = *static_cast<const u32x2*>(p4);
    o[0] = err_bf16(a[0] & 0xFFFFu);
    o[1] = err_bf16(a[0] >> 16);
    o[2] = err_bf16(a[1] & 0xFFFFu);
    o[3] = err_bf16(a[1] >> 16);
  } else {
    static_assert(kFmt == OFDG_FMT_F32, "a flow format");
    const f32x4 a = *static_cast<const f32x4*>(p4);
#pragma unroll
    for (int p = 0; p < 4; ++p) o[p] = a[p];
  }
}
template <int kFmt, typename Index>  // OFDG_FMT_F32 or OFDG_FMT_F16: element e of the plane(s) at base
__device__ __forceinline__ float elem_load(const uint8_t* __restrict__ base, Index e) {
  static_assert(kFmt == OFDG_FMT_F32 || kFmt == OFDG_FMT_F16, "a flow format of a source plane");
  return (float)reinterpret_cast<const typename FlowFmt<kFmt>::elem*>(base)[e];
}
template <bool kU8, typename T>  // T: uint32_t or int; o[0..3] are the quad's bytes
__device__ __forceinline__ void quad_load_bytes(const void* p4, T* o) {
  if constexpr (kU8) {
    const uint32_t w = *static_cast<const uint32_t*>(p4);
    o[0] = (T)(w & 255u); o[1] = (T)((w >> 8) & 255u); o[2] = (T)((w >> 16) & 255u); o[3] = (T)(w >> 24);
  } else {
    const f32x4 e = *static_cast<const f32x4*>(p4);
#pragma unroll
    for (int p = 0; p < 4; ++p) o[p] = (T)photo_index(e[p]);
  }
}
template <bool kU8>
__device__ __forceinline__ uint32_t elem_load_byte(const uint8_t* __restrict__ base, uint32_t e) {
  if constexpr (kU8) return base[e];
  else return (uint32_t)photo_index(reinterpret_cast<const float*>(base)[e]);
}
template <bool kU8>  // bit p: pixel p of the quad is hidden
__device__ __forceinline__ uint32_t quad_load_hidden(const void* p4) {
  uint32_t hidden = 0u;
  if constexpr (kU8) {
    const uint32_t o = *static_cast<const uint32_t*>(p4);
#pragma unroll
    for (int p = 0; p < 4; ++p) hidden |= (((o >> (8 * p)) & 255u) != 0u ? 1u : 0u) << p;
  } else {
    const f32x4 o = *static_cast<const f32x4*>(p4);
#pragma unroll
    for (int p = 0; p < 4; ++p) hidden |= (o[p] != 0.0f ? 1u : 0u) << p;
  }
  return hidden;
}
__device__ __forceinline__ uint32_t quad_word(const uint32_t (&b)[4]) { return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); }
// The quads of a pair of lanes - 8 bytes of a uint8 plane, whose rows start at multiples of 8 bytes only - stored by the even
// lane, the odd lane's word fetched with a wave shuffle: every lane of the wave calls this, `on` says whether the lane's
// quad exists (the lanes of a pair agree).  dst8: the lane's own quad.
__device__ __forceinline__ void quad_store_bytes_pair(void* dst8, uint32_t word, bool on) {
  const u32x2 o = {word, (uint32_t)__shfl_down((int)word, 1)};
  if (on && (threadIdx.x & 1u) == 0u) __builtin_nontemporal_store(o, static_cast<u32x2*>(dst8));
}
__device__ __forceinline__ void quad_store_bytes_f32(void* dst, const uint32_t (&b)[4], bool on) {
  const f32x4 o = {(float)b[0], (float)b[1], (float)b[2], (float)b[3]};
  if (on) __builtin_nontemporal_store(o, static_cast<f32x4*>(dst));
}
__device__ __forceinline__ void quad_store_u32x4(u32x4* p, u32x4 v) {
  __builtin_nontemporal_store(v, p);  // (whole lines, read next by another kernel: measured against plain stores, CHANGELOG)
}

// --------------------------------------------------------------------------
// Per-sample flow statistics (ofdg_flow_stats): displacement histogram, counts, Q8 sums and the largest |flow|^2 of a
// [n,2,H,W] flow tensor, float32 or binary16, with an optional [n,1,H,W] occlusion map (float32 or uint8).  One launch
// behind the call that wrote the planes; a pure function of the buffers.
// --------------------------------------------------------------------------
// Squared upper edge of bin k - 1 / lower edge of bin k: fl32(fl32(k * bin_px)^2).  Non-decreasing in k (rounding is monotone),
// so "the number of k in 1..63 with edge2(k) <= m2" is the one b with edge2(b) <= m2 < edge2(b + 1).
__device__ __forceinline__ float stats_edge2(int k, float bin_px) {
  const float e = __fmul_rn((float)k, bin_px);
  return __fmul_rn(e, e);
}

// One workgroup per (piece of kStatsQuads quads of a sample's plane, sample); a lane takes a quad - 4 adjacent pixels of each
// plane in one 16-byte (float32), 8-byte (binary16) or 4-byte (uint8 map) load; H * W is a multiple of 16, so a plane is whole
// quads and every plane of an aligned tensor is aligned.  The bin of a counted pixel starts from sqrt(m2) / bin_px and is
// walked to the exact one with the edges recomputed in two multiplications - no table, no LDS read.  Histogram: one copy of
// the 64 bins per wave in LDS.  Flow is spatially coherent, so per pixel position the wave first votes: the lanes whose bin is
// the first live lane's are counted with one ballot and added once (kStatsPeel rounds), and only lanes still left add their
// own 1 with an LDS atomic.  Counts, Q8 sums (int64 per lane: 16 values of up to 2^29) and the key go across the wave with
// __shfl_xor, then through LDS; at the end the workgroup issues one global atomicAdd per non-empty bin and count, one
// 64-bit atomicAdd per sum and one 64-bit atomicMax for the key.  Integer atomics only: no result depends on arrival order.
// sqrtf is the correctly rounded root here (hipcc expands it so unless told otherwise); __fsqrt_rn of this toolchain is the
// native 1-ulp approximation, which would make sum_mag_q8 differ from the host's.
constexpr int kStatsThreads = 256;
constexpr int kStatsQuads = 1024;  // 4 quads per lane
constexpr int kStatsPeel = 2;
template <bool kHalf, int kOcc>  // kOcc: 0 no map, 1 float32, 2 uint8
__global__ __launch_bounds__(kStatsThreads) void flow_stats_kernel(const void* __restrict__ flow, const void* __restrict__ occ, int n,
                                                                   uint32_t plane_quads, float bin_px, float inv_bin, int visible_only,
                                                                   int one_row, DevFlowStatsRow* __restrict__ rows) {
  typedef typename FlowFmt<quad_fmt(kHalf)>::quad FlowQuad;
  __shared__ uint32_t s_hist[kStatsThreads / 64][kFlowHistBins];
  __shared__ uint32_t s_cnt[3];
  __shared__ unsigned long long s_sum[3];
  __shared__ unsigned long long s_key;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q_begin = blockIdx.x * (uint32_t)kStatsQuads;
  const uint32_t q_end = min(q_begin + (uint32_t)kStatsQuads, plane_quads);
  for (int s = (int)blockIdx.y; s < n; s += (int)gridDim.y) {
    for (int i = tid; i < (kStatsThreads / 64) * kFlowHistBins; i += kStatsThreads) (&s_hist[0][0])[i] = 0u;
    if (tid < 3) { s_cnt[tid] = 0u; s_sum[tid] = 0ull; }
    if (tid == 3) s_key = 0ull;
    __syncthreads();
    const size_t pu = (size_t)s * 2 * plane_quads, pv = pu + plane_quads, po = (size_t)s * plane_quads;  // in quads
    const uint32_t idx_base = one_row ? (uint32_t)s * plane_quads * 4u : 0u;
    uint32_t n_counted = 0, n_bad = 0, n_occ = 0;
    long long sum_u = 0, sum_v = 0, sum_m = 0;
    unsigned long long key = 0;
    for (uint32_t q0 = q_begin; q0 < q_end; q0 += kStatsThreads) {  // (wave-uniform trip count: the ballots below see whole waves)
      const uint32_t q = q0 + (uint32_t)tid;
      const bool act = q < q_end;
      float u[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
      uint32_t hidden = 0;  // bit j: the map says pixel j is occluded
      if (act) {
        quad_load<quad_fmt(kHalf)>(static_cast<const FlowQuad*>(flow) + (pu + q), u);
        quad_load<quad_fmt(kHalf)>(static_cast<const FlowQuad*>(flow) + (pv + q), v);
        if constexpr (kOcc == 1) hidden = quad_load_hidden<false>(static_cast<const f32x4*>(occ) + (po + q));
        else if constexpr (kOcc == 2) hidden = quad_load_hidden<true>(static_cast<const uint32_t*>(occ) + (po + q));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool occluded = (hidden >> j) & 1u;
        n_occ += occluded ? 1u : 0u;
        const bool look = act && !(occluded && visible_only);
        const bool good = flow_usable(u[j], v[j]);
        n_bad += (look && !good) ? 1u : 0u;
        const bool counted = look && good;
        int b = -1;
        if (counted) {
          ++n_counted;
          const float m2 = __fadd_rn(__fmul_rn(u[j], u[j]), __fmul_rn(v[j], v[j]));
          const float r = sqrtf(m2);
          b = (int)fminf(__fmul_rn(r, inv_bin), (float)(kFlowHistBins - 1));
          while (b < kFlowHistBins - 1 && stats_edge2(b + 1, bin_px) <= m2) ++b;
          while (b > 0 && stats_edge2(b, bin_px) > m2) --b;
          sum_u += (long long)rintf(__fmul_rn(u[j], 256.0f));
          sum_v += (long long)rintf(__fmul_rn(v[j], 256.0f));
          sum_m += (long long)rintf(__fmul_rn(r, 256.0f));
          const uint32_t idx = idx_base + q * 4u + (uint32_t)j;
          const unsigned long long k = ((unsigned long long)__float_as_uint(m2) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
          key = k > key ? k : key;
        }
        bool live = counted;
#pragma unroll
        for (int p = 0; p < kStatsPeel; ++p) {
          const unsigned long long todo = __ballot(live);
          if (!todo) break;
          const int leader = __ffsll(todo) - 1;
          const int lb = __shfl(b, leader, 64);
          const bool same = live && b == lb;
          const unsigned long long m = __ballot(same);
          if (lane == leader) atomicAdd(&s_hist[wave][lb], (uint32_t)__popcll(m));
          live = live && !same;
        }
        if (live) atomicAdd(&s_hist[wave][b], 1u);
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      n_counted += (uint32_t)__shfl_xor((int)n_counted, d, 64);
      n_bad += (uint32_t)__shfl_xor((int)n_bad, d, 64);
      n_occ += (uint32_t)__shfl_xor((int)n_occ, d, 64);
      sum_u += __shfl_xor(sum_u, d, 64);
      sum_v += __shfl_xor(sum_v, d, 64);
      sum_m += __shfl_xor(sum_m, d, 64);
      const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, d, 64);
      key = other > key ? other : key;
    }
    if (lane == 0) {
      if (n_counted) atomicAdd(&s_cnt[0], n_counted);
      if (n_bad) atomicAdd(&s_cnt[1], n_bad);
      if (n_occ) atomicAdd(&s_cnt[2], n_occ);
      if (n_counted) {
        atomicAdd(&s_sum[0], (unsigned long long)sum_u);
        atomicAdd(&s_sum[1], (unsigned long long)sum_v);
        atomicAdd(&s_sum[2], (unsigned long long)sum_m);
        atomicMax(&s_key, key);
      }
    }
    __syncthreads();
    DevFlowStatsRow* const out = rows + (one_row ? 0 : s);
    if (wave == 0) {
      uint32_t h = 0;
#pragma unroll
      for (int w = 0; w < kStatsThreads / 64; ++w) h += s_hist[w][lane];
      if (h) atomicAdd(&out->hist[lane], h);
    } else if (wave == 1) {
      if (lane < 3 && s_cnt[lane]) atomicAdd(&out->count[lane], s_cnt[lane]);
    } else if (wave == 2) {
      if (lane < 3 && s_sum[lane]) atomicAdd(&out->sum_q8[lane], s_sum[lane]);
    } else if (lane == 0 && s_key) {
      atomicMax(&out->max_key, s_key);
    }
    __syncthreads();  // (the next sample of this workgroup clears the tables)
  }
}

// --------------------------------------------------------------------------
// Multi-scale flow pyramid (ofdg_flow_pyramid): levels 1..L of the mean flow of the usable pixels of a [n,2,H,W] flow tensor,
// float32 or binary16, with an optional [n,1,H,W] occlusion map, and optionally the usable-pixel counts.  One launch, the
// input read once; the summation tree is the definition's (include/ofdg.h), so the result is the host twin's bit for bit.
// --------------------------------------------------------------------------
// One workgroup of four waves per (64x64 tile, sample).  A lane owns a 4x4 block of pixels: four 16-byte loads per plane (8
// bytes for binary16, 4 or 16 bytes of map), all requested before the first is used; of a wave's load instruction every 16
// lanes read 256 (128) contiguous bytes of one row.  Lane l of wave w holds block (bx, by) = (l & 15, 4w + (l >> 4)), so
//   levels 1 and 2 (2x2 cells and the one cell of the block) are sums of the lane's own registers,
//   level 3 adds the lanes 1 and 16 away, level 4 the lanes 2 and 32 away (__shfl_xor: both partners compute the same sum,
//     float32 addition commutes bit for bit - the sums hold no NaN - so "left + right, then top + bottom" holds in every lane),
//   the four level-4 sums and counts of each wave meet in LDS behind one barrier, and wave 0 finishes levels 5 and 6 from
//     there in the order the definition fixes (only when levels >= 5: the test is uniform).
// Pixels outside the frame (partial tiles; H may be 2 mod 4 when levels = 1) count as unusable and their lanes stay in the
// shuffles; a cell is stored when it lies inside its level, and W, H are multiples of 2^levels, so such a cell never holds a
// pixel outside.  Stores: level 1 is two adjacent cells per lane and row - one 8-byte (float32), 4-byte (binary16, weights)
// store, aligned because W / 2 is a multiple of 4 -, 16 lanes fill 128 (64) contiguous bytes; the flow of level 1 is stored
// non-temporally like the other output planes.  Everything narrower than a line - the weights, and the deeper levels, one
// element per storing lane because their row pitch may be odd - is stored plainly, so that L2 merges the pieces of a line
// (measured: non-temporal stores there cost 4 - 9 us per launch at 512x384x32).  No atomics, no scratch.
constexpr int kPyrThreads = 256;
constexpr int kPyrTile = 64;
__device__ __forceinline__ void pyr_cell(float& su, float& sv, uint32_t c, float scale) {  // the sums of a cell -> its output
  // c == 0: every pixel of the cell went in as +0, so the sums are +0 and +0 / 1 is the +0 the definition asks for - no test.
  // A count that is a power of two (a cell without unusable pixels: the common case) divides exactly by a multiplication with
  // 2^-log2(c) - the product is the correctly rounded quotient, denormals included - so the division's expansion runs only
  // in a wave where some lane holds another count (the test is uniform: every lane takes the same, equally exact, path).
  const uint32_t d = max(c, 1u);
  if (__ballot((d & (d - 1u)) != 0u)) {
    su = su / (float)d;
    sv = sv / (float)d;
  } else {
    const float r = __uint_as_float((uint32_t)(96 + __clz((int)d)) << 23);  // 2^-log2(d): exponent 127 - (31 - clz)
    su = __fmul_rn(su, r);
    sv = __fmul_rn(sv, r);
  }
  su = __fmul_rn(su, scale);  // (1 or 2^-k: exact but for denormals)
  sv = __fmul_rn(sv, scale);
}
template <typename OutT>
__device__ __forceinline__ void pyr_store(const DevFlowPyramid& out, int k, int n_weights, int s, int W, int H, int X, int Y, float su, float sv,
                                          uint32_t c, float scale) {  // one cell of level k (1-based)
  const int w = W >> k, h = H >> k;
  if (X >= w || Y >= h) return;
  const size_t plane = (size_t)w * h, at = (size_t)Y * w + X;
  OutT* const f = static_cast<OutT*>(out.flow[k - 1]) + (size_t)s * 2 * plane + at;
  pyr_cell(su, sv, c, scale);
  f[0] = (OutT)su;
  f[plane] = (OutT)sv;
  if (n_weights) (static_cast<uint16_t*>(out.weight[k - 1]) + (size_t)s * plane + at)[0] = (uint16_t)c;
}
template <bool kHalf, bool kHalfOut, int kOcc>  // kOcc: 0 no map, 1 float32, 2 uint8
__global__ __launch_bounds__(kPyrThreads) void flow_pyramid_kernel(const void* __restrict__ flow, const void* __restrict__ occ, int n, int W,
                                                                   int H, int scaled, int n_weights, const DevFlowPyramid out) {
  typedef typename FlowFmt<quad_fmt(kHalf)>::quad FlowQuad;
  typedef typename std::conditional<kHalfOut, _Float16, float>::type OutT;
  typedef typename std::conditional<kHalfOut, f16x2, f32x2>::type OutT2;
  __shared__ float s_u[4][4], s_v[4][4];
  __shared__ uint32_t s_c[4][4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bx = lane & 15, by = wave * 4 + (lane >> 4);
  const int x0 = (int)blockIdx.x * kPyrTile + bx * 4, y0 = (int)blockIdx.y * kPyrTile + by * 4;  // the block's first pixel
  const int levels = out.levels;
  const size_t plane = (size_t)W * H;
  float scale[kPyrMaxLevels + 1];
#pragma unroll
  for (int k = 1; k <= kPyrMaxLevels; ++k) scale[k] = scaled ? 1.0f / (float)(1 << k) : 1.0f;
  for (int s = (int)blockIdx.z; s < n; s += (int)gridDim.z) {
    // level 0: the block's pixels, unusable ones as (+0, +0) with count 0
    float u[4][4], v[4][4];
    uint32_t hidden[4] = {0u, 0u, 0u, 0u};  // bit i of row j: the map says the pixel is occluded
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      in[j] = x0 < W && y0 + j < H;
      const size_t q = in[j] ? ((size_t)(y0 + j) * W + x0) / 4 : 0;  // in quads of a plane (W % 4 == 0)
      const size_t pu = (size_t)s * 2 * (plane / 4) + q, pv = pu + plane / 4, po = (size_t)s * (plane / 4) + q;
      // (a row outside the frame reads the plane's first quad instead and is masked below: no branch around the loads)
      quad_load<quad_fmt(kHalf)>(static_cast<const FlowQuad*>(flow) + pu, u[j]);
      quad_load<quad_fmt(kHalf)>(static_cast<const FlowQuad*>(flow) + pv, v[j]);
      if constexpr (kOcc == 1) hidden[j] = quad_load_hidden<false>(static_cast<const f32x4*>(occ) + po);
      else if constexpr (kOcc == 2) hidden[j] = quad_load_hidden<true>(static_cast<const uint32_t*>(occ) + po);
    }
    uint32_t c0[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // (flow_usable, spelled out: as a call in this chain of && the kernel compiled to half as many basic blocks again)
        const bool usable = in[j] && fabsf(u[j][i]) < 1048576.0f && fabsf(v[j][i]) < 1048576.0f && !((hidden[j] >> i) & 1u);
        u[j][i] = usable ? u[j][i] : 0.0f;
        v[j][i] = usable ? v[j][i] : 0.0f;
        c0[j][i] = usable ? 1u : 0u;
      }
    // level 1: 2x2 cells of the block, cell (a, b) = columns 2a, 2a+1 of rows 2b, 2b+1
    float u1[2][2], v1[2][2];
    uint32_t c1[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        u1[b][a] = __fadd_rn(__fadd_rn(u[2 * b][2 * a], u[2 * b][2 * a + 1]), __fadd_rn(u[2 * b + 1][2 * a], u[2 * b + 1][2 * a + 1]));
        v1[b][a] = __fadd_rn(__fadd_rn(v[2 * b][2 * a], v[2 * b][2 * a + 1]), __fadd_rn(v[2 * b + 1][2 * a], v[2 * b + 1][2 * a + 1]));
        c1[b][a] = c0[2 * b][2 * a] + c0[2 * b][2 * a + 1] + c0[2 * b + 1][2 * a] + c0[2 * b + 1][2 * a + 1];
      }
    {
      const int w = W >> 1, h = H >> 1, X = x0 >> 1;
      const size_t lp = (size_t)w * h;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int Y = (y0 >> 1) + b;
        if (X < w && Y < h) {
          const size_t at = (size_t)Y * w + X;
          OutT* const f = static_cast<OutT*>(out.flow[0]) + (size_t)s * 2 * lp + at;
          float mu[2] = {u1[b][0], u1[b][1]}, mv[2] = {v1[b][0], v1[b][1]};
          pyr_cell(mu[0], mv[0], c1[b][0], scale[1]);
          pyr_cell(mu[1], mv[1], c1[b][1], scale[1]);
          const OutT2 pu = {(OutT)mu[0], (OutT)mu[1]};
          const OutT2 pv = {(OutT)mv[0], (OutT)mv[1]};
          __builtin_nontemporal_store(pu, reinterpret_cast<OutT2*>(f));
          __builtin_nontemporal_store(pv, reinterpret_cast<OutT2*>(f + lp));
          if (n_weights) {
            const u16x2 pc = {(uint16_t)c1[b][0], (uint16_t)c1[b][1]};
            *reinterpret_cast<u16x2*>(static_cast<uint16_t*>(out.weight[0]) + (size_t)s * lp + at) = pc;
          }
        }
      }
    }
    // level 2: the block
    float su = __fadd_rn(__fadd_rn(u1[0][0], u1[0][1]), __fadd_rn(u1[1][0], u1[1][1]));
    float sv = __fadd_rn(__fadd_rn(v1[0][0], v1[0][1]), __fadd_rn(v1[1][0], v1[1][1]));
    uint32_t c = c1[0][0] + c1[0][1] + c1[1][0] + c1[1][1];
    if (levels >= 2) pyr_store<OutT>(out, 2, n_weights, s, W, H, x0 >> 2, y0 >> 2, su, sv, c, scale[2]);
    // levels 3 and 4: across the wave (every lane takes part; a lane whose block leads the cell stores it)
#pragma unroll
    for (int k = 3; k <= 4; ++k) {
      const int dx = k == 3 ? 1 : 2, dy = k == 3 ? 16 : 32;
      su = __fadd_rn(su, __shfl_xor(su, dx, 64));
      sv = __fadd_rn(sv, __shfl_xor(sv, dx, 64));
      c += (uint32_t)__shfl_xor((int)c, dx, 64);
      su = __fadd_rn(su, __shfl_xor(su, dy, 64));
      sv = __fadd_rn(sv, __shfl_xor(sv, dy, 64));
      c += (uint32_t)__shfl_xor((int)c, dy, 64);
      const int m = (1 << (k - 2)) - 1;  // blocks per cell side, less one
      if (levels >= k && !(bx & m) && !(by & m)) pyr_store<OutT>(out, k, n_weights, s, W, H, x0 >> k, y0 >> k, su, sv, c, scale[k]);
    }
    // levels 5 and 6: the tile's 4x4 level-4 cells through LDS, [row = wave][column]
    if (levels >= 5) {
      if ((lane & 0x33) == 0) { s_u[wave][bx >> 2] = su; s_v[wave][bx >> 2] = sv; s_c[wave][bx >> 2] = c; }
      __syncthreads();
      if (wave == 0) {
        const int X = lane & 1, Y = (lane >> 1) & 1;  // (lanes 0..3 hold the tile's 2x2 level-5 cells; the others repeat them)
        float tu = __fadd_rn(__fadd_rn(s_u[2 * Y][2 * X], s_u[2 * Y][2 * X + 1]), __fadd_rn(s_u[2 * Y + 1][2 * X], s_u[2 * Y + 1][2 * X + 1]));
        float tv = __fadd_rn(__fadd_rn(s_v[2 * Y][2 * X], s_v[2 * Y][2 * X + 1]), __fadd_rn(s_v[2 * Y + 1][2 * X], s_v[2 * Y + 1][2 * X + 1]));
        uint32_t tc = s_c[2 * Y][2 * X] + s_c[2 * Y][2 * X + 1] + s_c[2 * Y + 1][2 * X] + s_c[2 * Y + 1][2 * X + 1];
        if (lane < 4) pyr_store<OutT>(out, 5, n_weights, s, W, H, (int)blockIdx.x * 2 + X, (int)blockIdx.y * 2 + Y, tu, tv, tc, scale[5]);
        if (levels >= 6) {
          tu = __fadd_rn(tu, __shfl_xor(tu, 1, 64));
          tv = __fadd_rn(tv, __shfl_xor(tv, 1, 64));
          tc += (uint32_t)__shfl_xor((int)tc, 1, 64);
          tu = __fadd_rn(tu, __shfl_xor(tu, 2, 64));
          tv = __fadd_rn(tv, __shfl_xor(tv, 2, 64));
          tc += (uint32_t)__shfl_xor((int)tc, 2, 64);
          if (lane == 0) pyr_store<OutT>(out, 6, n_weights, s, W, H, (int)blockIdx.x, (int)blockIdx.y, tu, tv, tc, scale[6]);
        }
      }
      __syncthreads();  // (the next sample of this workgroup writes the table again)
    }
  }
}

// --------------------------------------------------------------------------
// Training crop (ofdg_crop): a window of every output plane of a batch, per sample its own, optionally mirrored, in one
// launch.  Bits are moved; the only other operations are the sign-bit XOR of a mirrored flow component and the window test
// of OFDG_CROP_OCC_WINDOW (include/ofdg.h), so the result is the host twin's bit for bit.
// --------------------------------------------------------------------------
// The destination of a (plane, channel, sample) is crop_w * crop_h elements without gaps, a whole number of 16-byte pieces
// (crop_w % 8 == 0, crop_h even).  A piece is 4 float32, 8 binary16 - both inside one row - or 16 uint8: two halves of 8, each
// inside one row (a row of uint8 is whole halves, two rows are whole pieces: the rows are paired).  A workgroup owns 1024
// consecutive pieces of one channel, lane t the pieces t, t + 256, t + 512, t + 768 of them, so every store instruction of a
// wave writes 1 KiB of consecutive, 16-byte aligned destination bytes: whole 128-byte lines.  blockIdx.x counts the
// workgroups of all 14 channel slots of a sample (the table of their first blocks comes with the launch: absent planes own
// none), blockIdx.y the samples.  Sources: x0 is arbitrary, so float32 is read by 4-byte loads, binary16 and uint8 by the
// aligned 4-byte words that cover the run - one word more than the run is long when it starts inside a word, that index
// clamped to the tensor's last word - and a byte funnel shift (v_alignbit); a mirrored run is read at its mirrored address and reversed in registers.  All loads
// of a lane's four pieces are requested before the first is used.  Pieces past the channel's end (the last workgroup) read
// pixel (0, 0) and are not stored.  The record is drawn or read, and sanitised, on uniform values once per (workgroup,
// sample); workgroup 0 of a sample writes it back from lane 0 with a vector store.  The occlusion planes under
// OFDG_CROP_OCC_WINDOW take a path of their own that also fetches both flow components of the piece's pixels, one piece at a
// time.  No LDS, no atomics, no scratch.
constexpr int kCropThreads = 256;
constexpr int kCropPerLane = 4;  // 16-byte pieces a lane moves
constexpr int kCropSlots = 14;   // channels of the eight planes: 3 3 2 2 1 1 1 1
struct DevCropGrid {
  uint32_t first_block[kCropSlots + 1];  // slot s owns blocks [first_block[s], first_block[s + 1]) of blockIdx.x
};
// kWords 32-bit words of destination: the kWords * 4 / kES elements that start at element `first` of the tensor at p (`last`:
// index of its last whole word), in destination order - reversed element by element when the row is mirrored.
template <int kES, int kWords>
__device__ __forceinline__ void crop_fetch(const uint32_t* __restrict__ p, size_t last, size_t first, bool mirrored, uint32_t (&out)[kWords]) {
  uint32_t t[kWords];
  if constexpr (kES == 4) {
#pragma unroll
    for (int i = 0; i < kWords; ++i) t[i] = p[first + i];
  } else {
    const size_t byte = first * kES, word = byte >> 2;
    const uint32_t shift = ((uint32_t)byte & 3u) * 8u;
    uint32_t w[kWords + 1];
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = p[word + i];  // (the run lies inside the tensor, so these words do)
    // the word behind them only when the run starts inside a word: an aligned run (the same for every lane of a sample: W, the
    // window's width and a run's length are multiples of 8 elements) requests no byte it does not move
    w[kWords] = shift ? p[word + kWords < last ? word + kWords : last] : 0u;
#pragma unroll
    for (int i = 0; i < kWords; ++i) t[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], shift);
  }
#pragma unroll
  for (int i = 0; i < kWords; ++i) {
    const uint32_t m = t[kWords - 1 - i];
    const uint32_t r = kES == 4 ? m : kES == 2 ? (m >> 16) | (m << 16) : __builtin_bswap32(m);
    out[i] = mirrored ? r : t[i];
  }
}
// Position of a lane's pieces: piece q of a channel starts at pixel q * kPixels of the crop_w x crop_h window.
struct CropAt {
  uint32_t X, Y;
};
__device__ __forceinline__ CropAt crop_advance(CropAt a, uint32_t dX, uint32_t dY, uint32_t crop_w) {
  a.X += dX;
  a.Y += dY;
  if (a.X >= crop_w) { a.X -= crop_w; ++a.Y; }
  return a;
}
// First source element (relative to the channel's plane) of the run of `run` destination pixels that starts at (X, Y).
__device__ __forceinline__ size_t crop_source(const DevCropRec& r, CropAt a, int run, int W, int crop_w, int crop_h) {
  const uint32_t ys = (uint32_t)r.y0 + ((r.flags & 2) ? (uint32_t)crop_h - 1u - a.Y : a.Y);
  const uint32_t xs = (uint32_t)r.x0 + ((r.flags & 1) ? (uint32_t)crop_w - a.X - (uint32_t)run : a.X);
  return (size_t)ys * (uint32_t)W + xs;
}
// The plain move of one channel: src / dst are the tensors of the plane, `chan` = sample * C + channel, sign: the XOR of
// every destination word (the sign bits of a mirrored flow component, else 0).
template <int kES>
__device__ __forceinline__ void crop_move(const void* __restrict__ src, void* __restrict__ dst, size_t chan, size_t tensor_words,
                                          const DevCropRec& r, int W, int H, int crop_w, int crop_h, uint32_t block, uint32_t sign) {
  constexpr int kPixels = 16 / kES;                       // of a piece
  constexpr int kRun = kES == 1 ? 8 : kPixels;            // of one fetch: uint8 pieces are two runs
  const uint32_t pieces = (uint32_t)crop_w * (uint32_t)crop_h / kPixels;
  const uint32_t* const sp = static_cast<const uint32_t*>(src);
  const size_t plane = chan * ((size_t)W * H), last = tensor_words - 1;
  u32x4* const dp = static_cast<u32x4*>(dst) + chan * pieces;
  const uint32_t q0 = block * (kCropThreads * kCropPerLane) + threadIdx.x;
  const uint32_t dX = (kCropThreads * kPixels) % (uint32_t)crop_w, dY = (kCropThreads * kPixels) / (uint32_t)crop_w;
  const bool mirrored = r.flags & 1;
  CropAt a;
  a.Y = (q0 * kPixels) / (uint32_t)crop_w;  // (q0 * kPixels < 2^31 + 2^14: crop_arg_error bounds the frame)
  a.X = q0 * kPixels - a.Y * (uint32_t)crop_w;
  uint32_t v[kCropPerLane][4];
#pragma unroll
  for (int j = 0; j < kCropPerLane; ++j) {
    const bool ok = q0 + j * kCropThreads < pieces;
    const CropAt at = ok ? a : CropAt{0u, 0u};
    if constexpr (kES == 1) {
      const CropAt b = crop_advance(at, 8u, 0u, (uint32_t)crop_w);
      uint32_t lo[2], hi[2];
      crop_fetch<1, 2>(sp, last, plane + crop_source(r, at, kRun, W, crop_w, crop_h), mirrored, lo);
      crop_fetch<1, 2>(sp, last, plane + crop_source(r, ok ? b : at, kRun, W, crop_w, crop_h), mirrored, hi);
      v[j][0] = lo[0]; v[j][1] = lo[1]; v[j][2] = hi[0]; v[j][3] = hi[1];
    } else {
      crop_fetch<kES, 4>(sp, last, plane + crop_source(r, at, kRun, W, crop_w, crop_h), mirrored, v[j]);
    }
    a = crop_advance(a, dX, dY, (uint32_t)crop_w);
  }
#pragma unroll
  for (int j = 0; j < kCropPerLane; ++j) {
    const uint32_t q = q0 + j * kCropThreads;
    if (q < pieces) {
      const u32x4 o = {v[j][0] ^ sign, v[j][1] ^ sign, v[j][2] ^ sign, v[j][3] ^ sign};
      quad_store_u32x4(dp + q, o);
    }
  }
}
// An occlusion plane under OFDG_CROP_OCC_WINDOW: the map's elements (kES 4: float32, 1: uint8) with both components of the
// flow that goes with it (kFES 4: float32, 2: binary16) at the same source pixels; an element becomes 1.0f / 1 where it is
// non-zero (float32: compares unequal to 0, so a NaN does and -0.0 does not) or the flow target leaves the window.
template <int kES, int kFES>
__device__ __forceinline__ void crop_occ_window(const void* __restrict__ src, void* __restrict__ dst, const void* __restrict__ flow, size_t sample,
                                                size_t n, const DevCropRec& r, int W, int H, int crop_w, int crop_h, uint32_t block) {
  constexpr int kPixels = 16 / kES, kRun = kES == 1 ? 8 : 4, kRuns = kPixels / kRun;
  constexpr int kOccWords = kRun * kES / 4, kFlowWords = kRun * kFES / 4;
  const uint32_t pieces = (uint32_t)crop_w * (uint32_t)crop_h / kPixels;
  const size_t frame = (size_t)W * H;
  const uint32_t* const sp = static_cast<const uint32_t*>(src);
  const uint32_t* const fp = static_cast<const uint32_t*>(flow);
  const size_t last = n * frame * kES / 4 - 1, flow_last = n * 2 * frame * kFES / 4 - 1;
  u32x4* const dp = static_cast<u32x4*>(dst) + sample * pieces;
  const uint32_t q0 = block * (kCropThreads * kCropPerLane) + threadIdx.x;
  const uint32_t dX = (kCropThreads * kPixels) % (uint32_t)crop_w, dY = (kCropThreads * kPixels) / (uint32_t)crop_w;
  const bool mirrored = r.flags & 1;
  CropAt a;
  a.Y = (q0 * kPixels) / (uint32_t)crop_w;
  a.X = q0 * kPixels - a.Y * (uint32_t)crop_w;
#pragma unroll 1  // (one piece at a time: up to 34 loads each, and the registers of four would halve the occupancy of the whole kernel)
  for (int j = 0; j < kCropPerLane; ++j) {
    const uint32_t q = q0 + j * kCropThreads;
    const bool ok = q < pieces;
    uint32_t o[4];
#pragma unroll
    for (int g = 0; g < kRuns; ++g) {
      CropAt at = ok ? a : CropAt{0u, 0u};
      if (g == 1 && ok) at = crop_advance(at, 8u, 0u, (uint32_t)crop_w);
      const size_t first = crop_source(r, at, kRun, W, crop_w, crop_h);
      uint32_t m[kOccWords], u[kFlowWords], v[kFlowWords];
      crop_fetch<kES, kOccWords>(sp, last, sample * frame + first, mirrored, m);
      crop_fetch<kFES, kFlowWords>(fp, flow_last, sample * 2 * frame + first, mirrored, u);
      crop_fetch<kFES, kFlowWords>(fp, flow_last, (sample * 2 + 1) * frame + first, mirrored, v);
      const int ys = r.y0 + (int)((r.flags & 2) ? (uint32_t)crop_h - 1u - at.Y : at.Y);
#pragma unroll
      for (int p = 0; p < kRun; ++p) {
        const int xs = r.x0 + (int)(mirrored ? (uint32_t)crop_w - 1u - (at.X + p) : at.X + p);
        float fu, fv;
        if constexpr (kFES == 4) {
          fu = __uint_as_float(u[p]);
          fv = __uint_as_float(v[p]);
        } else {
          fu = (float)__builtin_bit_cast(_Float16, (uint16_t)(u[p / 2] >> (16 * (p & 1))));
          fv = (float)__builtin_bit_cast(_Float16, (uint16_t)(v[p / 2] >> (16 * (p & 1))));
        }
        const bool inside = crop_target_inside(xs, fu, r.x0, crop_w) && crop_target_inside(ys, fv, r.y0, crop_h);
        if constexpr (kES == 4) {
          m[p] = (__uint_as_float(m[p]) != 0.0f || !inside) ? 0x3f800000u : m[p];
        } else {
          const uint32_t sh = 8u * (p & 3), b = (m[p / 4] >> sh) & 255u;
          m[p / 4] = (m[p / 4] & ~(255u << sh)) | (((b != 0u || !inside) ? 1u : b) << sh);
        }
      }
#pragma unroll
      for (int i = 0; i < kOccWords; ++i) o[g * kOccWords + i] = m[i];
    }
    if (ok) {
      const u32x4 ov = {o[0], o[1], o[2], o[3]};
      quad_store_u32x4(dp + q, ov);
    }
    a = crop_advance(a, dX, dY, (uint32_t)crop_w);
  }
}
template <bool kImageU8, bool kFlowHalf, bool kOccU8>
__global__ __launch_bounds__(kCropThreads) void crop_kernel(const DevCropJob job, const DevCropGrid grid, int n, int W, int H) {
  constexpr int kImageES = kImageU8 ? 1 : 4, kFlowES = kFlowHalf ? 2 : 4, kOccES = kOccU8 ? 1 : 4;
  const uint32_t bx = blockIdx.x;
  int slot = 0;
#pragma unroll
  for (int s = 1; s < kCropSlots; ++s) slot += bx >= grid.first_block[s] ? 1 : 0;
  uint32_t first = 0;
#pragma unroll
  for (int s = 1; s < kCropSlots; ++s) first = slot == s ? grid.first_block[s] : first;
  const uint32_t block = bx - first;
  const int plane = slot < 6 ? slot / 3 : slot < 10 ? 2 + (slot - 6) / 2 : slot - 6;
  const int channel = slot < 6 ? slot % 3 : slot < 10 ? (slot - 6) % 2 : 0;
  const void* src = nullptr;
  void* dst = nullptr;
#pragma unroll
  for (int k = 0; k < kCropPlanes; ++k) {  // (selects, not an indexed read of the argument)
    src = plane == k ? job.src[k] : src;
    dst = plane == k ? job.dst[k] : dst;
  }
  const int crop_w = job.crop_w, crop_h = job.crop_h, C = crop_channels(plane);
  const size_t frame = (size_t)W * H;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    DevCropRec r;
    if (job.recs) r = job.recs[i];
    else r = crop_draw_rec(job.seed, (unsigned long long)(job.first_index + i), W, H, crop_w, crop_h, job.flags);
    r = crop_sanitise(r, W, H, crop_w, crop_h);
    if (job.recs_out && bx == 0u && threadIdx.x == 0u) *reinterpret_cast<int4*>(job.recs_out + i) = make_int4(r.x0, r.y0, r.flags, 0);
    const size_t chan = (size_t)i * C + channel, elems = (size_t)n * C * frame;
    if (plane < 2) {
      crop_move<kImageES>(src, dst, chan, elems * kImageES / 4, r, W, H, crop_w, crop_h, block, 0u);
    } else if (plane < 4) {
      const bool negate = channel == 0 ? (r.flags & 1) : (r.flags & 2);
      crop_move<kFlowES>(src, dst, chan, elems * kFlowES / 4, r, W, H, crop_w, crop_h, block, negate ? (kFlowHalf ? 0x80008000u : 0x80000000u) : 0u);
    } else if (plane < 6) {
      if (job.flags & 16) crop_occ_window<kOccES, kFlowES>(src, dst, plane == 4 ? job.src[2] : job.src[3], (size_t)i, (size_t)n, r, W, H, crop_w, crop_h, block);
      else crop_move<kOccES>(src, dst, chan, elems * kOccES / 4, r, W, H, crop_w, crop_h, block, 0u);
    } else {
      crop_move<1>(src, dst, chan, elems / 4, r, W, H, crop_w, crop_h, block, 0u);
    }
  }
}

// --------------------------------------------------------------------------
// Photometric augmentation (ofdg_photo): a 256-entry table per (sample, frame, channel), a lookup per element and, where the
// sample's sigma is above 0, the noise of one Philox word per element, in one launch.  The functions of the definition are
// the host twin's (csrc/ofdg_device.h), so the result is the twin's bit for bit.
// --------------------------------------------------------------------------
// A channel of a sample is width * height elements without gaps, a whole number of 16-element runs (width % 8 == 0, height
// even).  A workgroup serves kPhotoBlockPixels consecutive elements of one (sample, frame, channel): each thread first makes
// one entry of that table in LDS (one fp64 log and exp), then the workgroup moves pieces - what one 16-byte store holds of the
// destination: 4 float32 or 16 uint8 - lane t the pieces t, t + 256, ... of the block, so a wave's store instruction writes
// 1 KiB of consecutive bytes.  A piece of a uint8 source is read as 4-byte words (the alignment asked of it), of a float32
// source as 16-byte ones.  A piece starts at an element number that is a multiple of 4, so the noise of its elements is whole
// Philox blocks: one per 4 elements.  A piece is read whole before it is written and by the same lane, which is all the
// in-place form needs.  The lookup is a ds_read_b32 at a data-dependent index (neighbouring pixels: mostly the same or
// nearby entries, so few lanes of a half-wave meet on a bank with different addresses).  blockIdx.x counts the blocks of the
// channels of the frames that are set, blockIdx.y the samples.  The record is drawn or read, and sanitised, on uniform
// values once per (workgroup, sample); workgroup 0 writes it back from lane 0 with vector stores.  The noise branch is
// uniform per (sample, frame).  No atomics, no scratch, 1 KiB of LDS.
constexpr int kPhotoThreads = 256;
#ifndef OFDG_PHOTO_BLOCK_PIXELS
#define OFDG_PHOTO_BLOCK_PIXELS 32768
#endif
constexpr int kPhotoBlockPixels = OFDG_PHOTO_BLOCK_PIXELS;  // 6 workgroups per channel of a 512 x 384 frame, a table entry per 128 elements (measured against 4096 .. 65536: CHANGELOG)
static_assert(kPhotoBlockPixels % (kPhotoThreads * 16) == 0, "whole rounds of pieces of either kind");
template <bool kSrcU8, bool kDstU8>
__global__ __launch_bounds__(kPhotoThreads) void photo_kernel(const DevPhotoJob job, int n, int W, int H, uint32_t per_channel) {
  constexpr int kP = kDstU8 ? 16 : 4;  // elements of a piece
  typedef typename std::conditional<kSrcU8, uint8_t, float>::type SrcT;
  __shared__ float table[256];
  const uint32_t slot = blockIdx.x / per_channel, block = blockIdx.x - slot * per_channel;
  const int f = (int)(slot / 3u) + (job.src[0] ? 0 : 1), c = (int)(slot % 3u);
  const void* const src = f ? job.src[1] : job.src[0];
  void* const dst = f ? job.dst[1] : job.dst[0];
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (3 * plane < 2^32: photo_arg_error)
  const uint32_t first = block * (uint32_t)kPhotoBlockPixels;
  const uint32_t end = first + (uint32_t)kPhotoBlockPixels < plane ? first + (uint32_t)kPhotoBlockPixels : plane;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    const unsigned long long g = (unsigned long long)(job.first_index + i);
    DevPhotoRec r;
    if (job.recs) r = job.recs[i];
    else r = photo_draw_rec(job.seed, g, job);
    r = photo_sanitise(r);
    if (job.recs_out && blockIdx.x == 0u && threadIdx.x == 0u) {
      float4* const o = reinterpret_cast<float4*>(job.recs_out + i);
      o[0] = make_float4(r.gamma[0], r.gamma[1], r.contrast[0], r.contrast[1]);
      o[1] = make_float4(r.brightness[0], r.brightness[1], r.gain[0][0], r.gain[0][1]);
      o[2] = make_float4(r.gain[0][2], r.gain[1][0], r.gain[1][1], r.gain[1][2]);
      o[3] = make_float4(r.sigma[0], r.sigma[1], 0.0f, 0.0f);
    }
    const float gamma = f ? r.gamma[1] : r.gamma[0], contrast = f ? r.contrast[1] : r.contrast[0];
    const float brightness = f ? r.brightness[1] : r.brightness[0], sigma = f ? r.sigma[1] : r.sigma[0];
    const float gain = f ? (c == 0 ? r.gain[1][0] : c == 1 ? r.gain[1][1] : r.gain[1][2]) : (c == 0 ? r.gain[0][0] : c == 1 ? r.gain[0][1] : r.gain[0][2]);
    table[threadIdx.x] = photo_table_entry(gamma, gain, contrast, brightness, (int)threadIdx.x);
    __syncthreads();
    const bool noisy = sigma > 0.0f;
    const float scale = photo_noise_scale(sigma);
    const uint32_t k0 = job.seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
    const size_t chan = ((size_t)i * 3 + (size_t)c) * plane;  // first element of the channel in the tensor
    for (uint32_t at = first + threadIdx.x * (uint32_t)kP; at < end; at += (uint32_t)(kPhotoThreads * kP)) {
      int k[kP];
      const SrcT* const sp = static_cast<const SrcT*>(src) + chan + at;
#pragma unroll
      for (int q = 0; q < kP / 4; ++q) quad_load_bytes<kSrcU8>(sp + 4 * q, k + 4 * q);
      float v[kP];
#pragma unroll
      for (int q = 0; q < kP; ++q) v[q] = table[k[q]];
      if (noisy) {
        const uint32_t m = (uint32_t)c * plane + at;  // element number of the piece's first element: a multiple of 4
#pragma unroll
        for (int q = 0; q < kP / 4; ++q) {
          const CropWords w = crop_philox(CropWords{(m >> 2) + (uint32_t)q, (uint32_t)f, 0x0c72u, 0u}, k0, k1);
          v[4 * q] = photo_add_noise(v[4 * q], scale, w.x);
          v[4 * q + 1] = photo_add_noise(v[4 * q + 1], scale, w.y);
          v[4 * q + 2] = photo_add_noise(v[4 * q + 2], scale, w.z);
          v[4 * q + 3] = photo_add_noise(v[4 * q + 3], scale, w.w);
        }
      }
      u32x4 o;
      if constexpr (kDstU8) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          o[q] = (uint32_t)rintf(v[4 * q]) | ((uint32_t)rintf(v[4 * q + 1]) << 8) | ((uint32_t)rintf(v[4 * q + 2]) << 16) | ((uint32_t)rintf(v[4 * q + 3]) << 24);
        quad_store_u32x4(reinterpret_cast<u32x4*>(static_cast<uint8_t*>(dst) + chan + at), o);
      } else {
        o = u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
        quad_store_u32x4(reinterpret_cast<u32x4*>(static_cast<float*>(dst) + chan + at), o);
      }
    }
    __syncthreads();  // (the next sample of this workgroup writes the table again)
  }
}
// ofdg_debug_photo_table: the table [2][3][256] of one record as the device computes its entries - workgroup b = f * 3 + c.
__global__ __launch_bounds__(256) void photo_table_kernel(const DevPhotoRec* __restrict__ rec, float* __restrict__ out) {
  const DevPhotoRec r = photo_sanitise(*rec);
  const int f = (int)blockIdx.x / 3, c = (int)blockIdx.x % 3;
  const float gain = f ? (c == 0 ? r.gain[1][0] : c == 1 ? r.gain[1][1] : r.gain[1][2]) : (c == 0 ? r.gain[0][0] : c == 1 ? r.gain[0][1] : r.gain[0][2]);
  out[blockIdx.x * 256u + threadIdx.x] =
      photo_table_entry(f ? r.gamma[1] : r.gamma[0], gain, f ? r.contrast[1] : r.contrast[0], f ? r.brightness[1] : r.brightness[0], (int)threadIdx.x);
}

// --------------------------------------------------------------------------
// Spatial augmentation (ofdg_spatial): every plane of a batch resampled through an affine map per (sample, frame) - a gather
// with bilinear interpolation for the frames, the nearest tap for flow, maps and labels -, the flow transformed to match, in
// one launch.  The functions of the definition are the host twin's (csrc/ofdg_device.h), so the result is the twin's bit for
// bit.
// --------------------------------------------------------------------------
// The destination of a (plane, channel, sample) is out_w * out_h elements without gaps; 16 consecutive elements - a unit - are
// one 16-byte piece of a uint8 plane, two of a binary16 and four of a float32 one.  A unit is two runs of 8 pixels, each
// inside one row (out_w % 8 == 0; where out_w / 8 is odd every other unit has its runs in two rows, which is why units are
// counted in row PAIRS: rows 2P and 2P + 1 together are out_w / 8 whole units).  Four neighbouring lanes own a unit, a lane
// four consecutive pixels of it, so the lanes of a wave read neighbouring source pixels in the same instruction: a line
// fetched serves its lanes at once and the next three pixels right behind (a lane that walked 16 pixels on its own asked for
// every line 16 times, from L2: CHANGELOG).  The coordinates, the taps and the weights of a pixel are computed once and serve
// every plane of the frame: three image channels, two flow components, the map and the label.  Every store is one 16-byte
// piece: a float32 piece is a lane's own; a binary16 piece is gathered by the even lane of a pair, a uint8 piece by the
// first lane of the four (wave shuffles, no LDS allocated), so a wave's store instruction writes whole consecutive rows of
// the tile.  A workgroup owns a 2-D tile of kSpatialTileQ units x (64 / kSpatialTileQ) * kSpatialPasses row pairs - a compact
// footprint in the source also when the map rotates - and walks it in kSpatialPasses passes; blockIdx.x counts the tiles,
// blockIdx.y the samples, blockIdx.z the frames that have a plane.  Sources are read element by element at computed, clamped
// indices (dword / ushort / ubyte loads: nothing is asked of x), so no record reaches outside a plane.  The record is drawn
// or read, sanitised and inverted on uniform values once per (workgroup, sample); workgroup 0 writes it back from lane 0
// with vector stores.  No LDS, no atomics, no scratch.
constexpr int kSpatialThreads = 256;
#ifndef OFDG_SPATIAL_TILE_Q
#define OFDG_SPATIAL_TILE_Q 8
#endif
#ifndef OFDG_SPATIAL_PASSES
#define OFDG_SPATIAL_PASSES 2
#endif
constexpr int kSpatialTileQ = OFDG_SPATIAL_TILE_Q;                   // units of 16 pixels across a tile (measured against 4 and 16: CHANGELOG)
constexpr int kSpatialRowPairs = kSpatialThreads / 4 / kSpatialTileQ;  // row pairs of one pass
constexpr int kSpatialPasses = OFDG_SPATIAL_PASSES;                  // 8 pixels a lane: the record's draw is paid once for them (measured against 4 and 8: CHANGELOG)
constexpr int kSpatialTileP = kSpatialRowPairs * kSpatialPasses;     // row pairs of a tile
static_assert(kSpatialTileQ * kSpatialRowPairs * 4 == kSpatialThreads, "four lanes per unit of a pass");
__device__ __forceinline__ void spatial_store(void* p, u32x4 v) {
  quad_store_u32x4(static_cast<u32x4*>(p), v);  // (whole pieces, read next by another kernel: measured against plain stores, CHANGELOG)
}
template <bool kImageU8, bool kFlowHalf, bool kOccU8>
__global__ __launch_bounds__(kSpatialThreads) void spatial_kernel(const DevSpatialJob job, int n, int W, int H, uint32_t tiles_x) {
  constexpr int kImageES = kImageU8 ? 1 : 4, kFlowES = kFlowHalf ? 2 : 4, kOccES = kOccU8 ? 1 : 4;
  const int ow = job.out_w, oh = job.out_h;
  const uint32_t R = (uint32_t)ow / 8u, pairs = (uint32_t)oh / 2u;  // units per row pair, row pairs
  const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const uint32_t j = threadIdx.x & 3u, u = threadIdx.x >> 2;  // the lane's four pixels of its unit; the unit of the pass
  const uint32_t q = tx * kSpatialTileQ + u % kSpatialTileQ, P0 = ty * kSpatialTileP + u / kSpatialTileQ;
  const uint32_t t = 2u * q + (j >> 1);  // the run of 8 among the 2 R runs of a row pair
  const bool second = t >= R;
  const int X0 = (int)((t - (second ? R : 0u)) * 8u + (j & 1u) * 4u);
  const bool frame0 = job.src[0] || job.src[2] || job.src[4] || job.src[6];
  const int f = (blockIdx.z != 0u || !frame0) ? 1 : 0;
  const uint8_t* const s_img = static_cast<const uint8_t*>(f ? job.src[1] : job.src[0]);
  const uint8_t* const s_flow = static_cast<const uint8_t*>(f ? job.src[3] : job.src[2]);
  const uint8_t* const s_occ = static_cast<const uint8_t*>(f ? job.src[5] : job.src[4]);
  const uint8_t* const s_lab = static_cast<const uint8_t*>(f ? job.src[7] : job.src[6]);
  uint8_t* const d_img = static_cast<uint8_t*>(f ? job.dst[1] : job.dst[0]);
  uint8_t* const d_flow = static_cast<uint8_t*>(f ? job.dst[3] : job.dst[2]);
  uint8_t* const d_occ = static_cast<uint8_t*>(f ? job.dst[5] : job.dst[4]);
  uint8_t* const d_lab = static_cast<uint8_t*>(f ? job.dst[7] : job.dst[6]);
  const bool occ_window = job.flags & 16;
  const size_t frame = (size_t)W * H, window = (size_t)ow * oh;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    DevSpatialRec r;
    if (job.recs) r = job.recs[i];
    else r = spatial_draw_rec(job.seed, (unsigned long long)(job.first_index + i), job, W, H);
    r = spatial_sanitise(r, W, H, ow, oh);
    if (job.recs_out && blockIdx.x == 0u && blockIdx.z == 0u && threadIdx.x == 0u) {
      double2* const o = reinterpret_cast<double2*>(job.recs_out + i);
      o[0] = make_double2(r.m[0][0], r.m[0][1]); o[1] = make_double2(r.m[0][2], r.m[0][3]); o[2] = make_double2(r.m[0][4], r.m[0][5]);
      o[3] = make_double2(r.m[1][0], r.m[1][1]); o[4] = make_double2(r.m[1][2], r.m[1][3]); o[5] = make_double2(r.m[1][4], r.m[1][5]);
      *reinterpret_cast<int4*>(o + 6) = make_int4(0, 0, 0, 0);
    }
    if (q >= R) continue;  // (a whole unit, its four lanes together)
    const double ma = f ? r.m[1][0] : r.m[0][0], mb = f ? r.m[1][1] : r.m[0][1], mc = f ? r.m[1][2] : r.m[0][2];
    const double md = f ? r.m[1][3] : r.m[0][3], me = f ? r.m[1][4] : r.m[0][4], mg = f ? r.m[1][5] : r.m[0][5];
    const double om[6] = {f ? r.m[0][0] : r.m[1][0], f ? r.m[0][1] : r.m[1][1], f ? r.m[0][2] : r.m[1][2],
                          f ? r.m[0][3] : r.m[1][3], f ? r.m[0][4] : r.m[1][4], f ? r.m[0][5] : r.m[1][5]};
    const SpatialInv other = spatial_inverse(om);
    const uint8_t* const si = s_img + (size_t)i * 3 * frame * kImageES;
    const uint8_t* const sf = s_flow + (size_t)i * 2 * frame * kFlowES;
    const uint8_t* const so = s_occ + (size_t)i * frame * kOccES;
    const uint8_t* const sl = s_lab + (size_t)i * frame;
#pragma unroll 1
    for (int pass = 0; pass < kSpatialPasses; ++pass) {
      const uint32_t P = P0 + (uint32_t)pass * kSpatialRowPairs;
      if (P >= pairs) break;  // (whole units again)
      const int Y = (int)(2u * P + (second ? 1u : 0u));
      const size_t at = ((size_t)P * R + q) * 16u + 4u * j;  // the lane's first element in a channel of the destination
      const double rowx = spatial_row_term(mb, Y), rowy = spatial_row_term(me, Y);
      float img[3][4], fu[4], fv[4];
      uint32_t hid[4], lab[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int X = X0 + p;
        const double qx = spatial_coord(ma, X, rowx, mc), qy = spatial_coord(md, X, rowy, mg);
        const int Qx = spatial_fixed(qx), Qy = spatial_fixed(qy);
        const uint32_t near = (uint32_t)spatial_clamp((Qy + 128) >> 8, H) * (uint32_t)W + (uint32_t)spatial_clamp((Qx + 128) >> 8, W);
        if (s_img) {
          const int fx = Qx & 255, fy = Qy & 255;
          const uint32_t x0 = (uint32_t)spatial_clamp(Qx >> 8, W), x1 = (uint32_t)spatial_clamp((Qx >> 8) + 1, W);
          const uint32_t y0 = (uint32_t)spatial_clamp(Qy >> 8, H) * (uint32_t)W, y1 = (uint32_t)spatial_clamp((Qy >> 8) + 1, H) * (uint32_t)W;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float e00, e10, e01, e11;
            if constexpr (kImageU8) {
              const uint8_t* const pc = si + (size_t)c * frame;
              e00 = (float)pc[y0 + x0]; e10 = (float)pc[y0 + x1]; e01 = (float)pc[y1 + x0]; e11 = (float)pc[y1 + x1];
            } else {
              const float* const pc = reinterpret_cast<const float*>(si) + (size_t)c * frame;
              e00 = pc[y0 + x0]; e10 = pc[y0 + x1]; e01 = pc[y1 + x0]; e11 = pc[y1 + x1];
            }
            img[c][p] = spatial_blend(e00, e10, e01, e11, fx, fy);
          }
        }
        double px = 0.0, py = 0.0;
        if (s_flow) {
          float su, sv;
          if constexpr (kFlowHalf) {
            const _Float16* const pf = reinterpret_cast<const _Float16*>(sf);
            su = (float)pf[near]; sv = (float)pf[frame + near];
          } else {
            const float* const pf = reinterpret_cast<const float*>(sf);
            su = pf[near]; sv = pf[frame + near];
          }
          spatial_partner(qx, qy, su, sv, other, &px, &py);
          fu[p] = spatial_flow_of(px, X);
          fv[p] = spatial_flow_of(py, Y);
        }
        if (s_occ) {
          bool hidden;
          if constexpr (kOccU8) hidden = so[near] != 0;
          else hidden = reinterpret_cast<const float*>(so)[near] != 0.0f;
          hidden = hidden || !spatial_inside(Qx, Qy, W, H);
          if (occ_window) hidden = hidden || !(spatial_partner_inside(px, ow) && spatial_partner_inside(py, oh));
          hid[p] = hidden ? 1u : 0u;
        }
        if (s_lab) lab[p] = sl[near];
      }
      // (the lanes of a unit are all here: q and P are the unit's)
      if (s_img) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if constexpr (kImageU8) {
            const uint32_t w = spatial_to_byte(img[c][0]) | (spatial_to_byte(img[c][1]) << 8) | (spatial_to_byte(img[c][2]) << 16) | (spatial_to_byte(img[c][3]) << 24);
            const u32x4 o = {w, (uint32_t)__shfl_down((int)w, 1), (uint32_t)__shfl_down((int)w, 2), (uint32_t)__shfl_down((int)w, 3)};
            if (j == 0u) spatial_store(d_img + ((size_t)i * 3 + c) * window + at, o);
          } else {
            const u32x4 o = {__float_as_uint(img[c][0]), __float_as_uint(img[c][1]), __float_as_uint(img[c][2]), __float_as_uint(img[c][3])};
            spatial_store(d_img + (((size_t)i * 3 + c) * window + at) * 4u, o);
          }
        }
      }
      if (s_flow) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float* const v = c ? fv : fu;
          if constexpr (kFlowHalf) {
            const uint32_t w0 = spatial_half_bits(v[0]) | (spatial_half_bits(v[1]) << 16), w1 = spatial_half_bits(v[2]) | (spatial_half_bits(v[3]) << 16);
            const u32x4 o = {w0, w1, (uint32_t)__shfl_down((int)w0, 1), (uint32_t)__shfl_down((int)w1, 1)};
            if ((j & 1u) == 0u) spatial_store(d_flow + (((size_t)i * 2 + c) * window + at) * 2u, o);
          } else {
            const u32x4 o = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
            spatial_store(d_flow + (((size_t)i * 2 + c) * window + at) * 4u, o);
          }
        }
      }
      if (s_occ) {
        if constexpr (kOccU8) {
          const uint32_t w = hid[0] | (hid[1] << 8) | (hid[2] << 16) | (hid[3] << 24);
          const u32x4 o = {w, (uint32_t)__shfl_down((int)w, 1), (uint32_t)__shfl_down((int)w, 2), (uint32_t)__shfl_down((int)w, 3)};
          if (j == 0u) spatial_store(d_occ + (size_t)i * window + at, o);
        } else {
          const u32x4 o = {hid[0] ? 0x3f800000u : 0u, hid[1] ? 0x3f800000u : 0u, hid[2] ? 0x3f800000u : 0u, hid[3] ? 0x3f800000u : 0u};
          spatial_store(d_occ + ((size_t)i * window + at) * 4u, o);
        }
      }
      if (s_lab) {
        const uint32_t w = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
        const u32x4 o = {w, (uint32_t)__shfl_down((int)w, 1), (uint32_t)__shfl_down((int)w, 2), (uint32_t)__shfl_down((int)w, 3)};
        if (j == 0u) spatial_store(d_lab + (size_t)i * window + at, o);
      }
    }
  }
}

// --------------------------------------------------------------------------
// Network-ready packing (ofdg_pack): scale and shift, channel order, element type, layout and the concatenation of both
// frames, and the flow times a constant, in one launch.  The functions of the definition are the host twin's
// (csrc/ofdg_device.h), so the result is the twin's bit for bit.
// --------------------------------------------------------------------------
// A streaming kernel: its bound is bytes.  A channel of a sample is width * height elements without gaps, whole units of 8
// consecutive pixels of one row (width % 8 == 0).  A lane owns one unit of one plane group - a frame (3 channels), both frames
// (6, OFDG_PACK_CONCAT) or the flow (2) - and all of its channels: per channel it reads 8 bytes of a uint8 source as two
// 4-byte words, 16 bytes of a binary16 one as two 8-byte pieces, 32 bytes of a float32 one as two 16-byte pieces (the
// alignments the entry asks of a source), every load requested before the first value is used, and converts in registers.
// What a lane then holds is kP consecutive 16-byte pieces of a run of 64 * kP pieces that the wave's 64 units fill without
// gaps: one piece per channel of a planar 16-bit destination, two per channel of a planar float32 one, the unit's 8 * C
// interleaved elements - 8 * C * es / 16 = 2, 3, 4, 6 or 12 pieces - of a channels-last one.  Where kP > 1 a store
// instruction that wrote each lane's m-th piece would touch 16 bytes out of every kP * 16 (measured: CHANGELOG), so the
// lanes of a wave exchange their pieces through the wave's own LDS slots and store instruction m writes pieces 64 m .. 64 m +
// 63 of the run, 1 KiB of consecutive bytes.  The exchange stays inside a wave (its LDS instructions execute in order), so
// it needs no workgroup barrier and lanes past the last unit take part without storing.  Every store is a whole 16-byte
// piece, non-temporal, as in crop_kernel.  blockIdx.x counts the workgroups of the plane groups that are set (frames, then
// the flow), blockIdx.y the samples.  Lanes past the last unit read unit 0.  The frames' formats, the layout and the
// concatenation are template arguments; the flow's two formats, the channel order and every constant are uniform at run
// time (the flow's six forms are in every instantiation, behind uniform branches).  The bfloat16 rounding is the integer
// form of the definition.  LDS: 16 bytes * 256 * the largest kP of the instantiation (8 - 48 KiB); no atomics, no scratch.
constexpr int kPackThreads = 256;
constexpr int kPackSrcF32 = 0, kPackSrcU8 = 1, kPackSrcF16 = 2;  // how pack_unit reads a source
struct PackRun {          // the wave's units
  u32x4* lds;        // the wave's 64 * kP slots
  uint32_t first_unit;    // the unit of its lane 0
  uint32_t units;         // units of a channel: those from here on do not exist
};
__device__ __forceinline__ void pack_wave_sync() {  // the wave's LDS accesses so far before those that follow
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The wave's run of 64 * kP pieces from `dp` on, lane l holding pieces l * kP .. l * kP + kP - 1 of it.
template <int kP>
__device__ __forceinline__ void pack_store_run(const u32x4 (&piece)[kP], uint8_t* dp, const PackRun& run) {
  const uint32_t lane = threadIdx.x & 63u;
  u32x4* const d = reinterpret_cast<u32x4*>(dp);
  if constexpr (kP == 1) {
    if (run.first_unit + lane < run.units) quad_store_u32x4(d + lane, piece[0]);
  } else {
#pragma unroll
    for (int m = 0; m < kP; ++m) run.lds[lane * kP + m] = piece[m];
    pack_wave_sync();
#pragma unroll
    for (int m = 0; m < kP; ++m) {
      const uint32_t idx = (uint32_t)m * 64u + lane;
      if (run.first_unit + idx / kP < run.units) quad_store_u32x4(d + idx, run.lds[idx]);
    }
    pack_wave_sync();  // (the slots are written again by the next channel, plane group or sample)
  }
}
template <int kDst>
__device__ __forceinline__ uint32_t pack_device_bits(float y) {
  if constexpr (kDst == OFDG_FMT_F32) return __float_as_uint(spatial_quiet(y));
  else if constexpr (kDst == OFDG_FMT_BF16) return pack_bf16_bits(y);
  else return y != y ? 0x7E00u : (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)y);  // (v_cvt_f16_f32: to nearest even, denormals kept)
}
// One unit per lane: sp[cd] the 8 source elements of destination channel cd; dp the first destination byte of the wave's
// first unit (planar: in channel 0, the channels chan_bytes apart; channels-last: of its 8 * kC elements).
template <int kC, int kSrc, int kDst, bool kNhwc, bool kBias>
__device__ __forceinline__ void pack_unit(const uint8_t* const (&sp)[kC], const float (&scale)[kC], const float (&bias)[kC], uint8_t* dp, size_t chan_bytes,
                                          const PackRun& run) {
  constexpr int kSW = kSrc == kPackSrcU8 ? 2 : kSrc == kPackSrcF16 ? 4 : 8;  // 32-bit words of 8 source elements
  constexpr bool kWide = kDst == OFDG_FMT_F32;
  uint32_t raw[kC][kSW];
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    if constexpr (kSrc == kPackSrcU8) {
      const uint32_t* const p = reinterpret_cast<const uint32_t*>(sp[c]);
      raw[c][0] = p[0]; raw[c][1] = p[1];
    } else if constexpr (kSrc == kPackSrcF16) {
      const uint2* const p = reinterpret_cast<const uint2*>(sp[c]);
      const uint2 a = p[0], b = p[1];
      raw[c][0] = a.x; raw[c][1] = a.y; raw[c][2] = b.x; raw[c][3] = b.y;
    } else {
      const uint4* const p = reinterpret_cast<const uint4*>(sp[c]);
      const uint4 a = p[0], b = p[1];
      raw[c][0] = a.x; raw[c][1] = a.y; raw[c][2] = a.z; raw[c][3] = a.w;
      raw[c][4] = b.x; raw[c][5] = b.y; raw[c][6] = b.z; raw[c][7] = b.w;
    }
  }
  uint32_t o[kC][8];  // what is stored of each element (the low 16 bits of a 16-bit format)
#pragma unroll
  for (int c = 0; c < kC; ++c) {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      float x;
      if constexpr (kSrc == kPackSrcU8) x = (float)((raw[c][p / 4] >> (8 * (p & 3))) & 255u);
      else if constexpr (kSrc == kPackSrcF16) x = (float)__builtin_bit_cast(_Float16, (uint16_t)(raw[c][p / 2] >> (16 * (p & 1))));
      else x = __uint_as_float(raw[c][p]);
      float y;
      if constexpr (kBias) y = pack_value(x, scale[c], bias[c]);
      else y = pack_flow_value(x, scale[c]);
      o[c][p] = pack_device_bits<kDst>(y);
    }
  }
  if constexpr (!kNhwc) {
#pragma unroll
    for (int c = 0; c < kC; ++c) {
      if constexpr (kWide) {
        const u32x4 piece[2] = {u32x4{o[c][0], o[c][1], o[c][2], o[c][3]}, u32x4{o[c][4], o[c][5], o[c][6], o[c][7]}};
        pack_store_run<2>(piece, dp + (size_t)c * chan_bytes, run);
      } else {
        const u32x4 piece[1] = {u32x4{o[c][0] | (o[c][1] << 16), o[c][2] | (o[c][3] << 16), o[c][4] | (o[c][5] << 16), o[c][6] | (o[c][7] << 16)}};
        pack_store_run<1>(piece, dp + (size_t)c * chan_bytes, run);
      }
    }
  } else {
    // element e = pixel * kC + channel of the unit is o[e % kC][e / kC]
    constexpr int kP = kWide ? 2 * kC : kC;
    u32x4 piece[kP];
    if constexpr (kWide) {
#pragma unroll
      for (int m = 0; m < kP; ++m) {
        const int e = 4 * m;
        piece[m] = u32x4{o[e % kC][e / kC], o[(e + 1) % kC][(e + 1) / kC], o[(e + 2) % kC][(e + 2) / kC], o[(e + 3) % kC][(e + 3) / kC]};
      }
    } else {
#pragma unroll
      for (int m = 0; m < kP; ++m) {
        const int e = 8 * m;
        piece[m] = u32x4{o[e % kC][e / kC] | (o[(e + 1) % kC][(e + 1) / kC] << 16), o[(e + 2) % kC][(e + 2) / kC] | (o[(e + 3) % kC][(e + 3) / kC] << 16),
                              o[(e + 4) % kC][(e + 4) / kC] | (o[(e + 5) % kC][(e + 5) / kC] << 16),
                              o[(e + 6) % kC][(e + 6) / kC] | (o[(e + 7) % kC][(e + 7) / kC] << 16)};
      }
    }
    pack_store_run<kP>(piece, dp, run);
  }
}
template <bool kImgU8, int kImgDst, bool kNhwc, bool kConcat>
__global__ __launch_bounds__(kPackThreads) void pack_kernel(const DevPackJob job, int n, int W, int H, uint32_t per_group) {
  constexpr int kImgSrc = kImgU8 ? kPackSrcU8 : kPackSrcF32, kImgC = kConcat ? 6 : 3;
  constexpr uint32_t kImgSES = kImgU8 ? 1 : 4, kImgDES = kImgDst == OFDG_FMT_F32 ? 4 : 2;
  // the largest kP: planar 2 (a float32 channel); channels-last the frames' 8 * C * es / 16, or a float32 flow's 4
  constexpr int kImgP = kImgC * (int)kImgDES / 2, kMaxP = !kNhwc ? 2 : kImgP > 4 ? kImgP : 4;
  __shared__ u32x4 slots[kPackThreads * kMaxP];
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (6 * plane < 2^31: pack_arg_error)
  const uint32_t units = plane / 8u;
  const uint32_t group = blockIdx.x / per_group;
  const uint32_t mine = (blockIdx.x - group * per_group) * (uint32_t)kPackThreads + threadIdx.x;
  const uint32_t at = mine < units ? mine * 8u : 0u;  // the unit's first pixel in a channel; past the end: unit 0, read and not stored
  const PackRun run{slots + (threadIdx.x >> 6) * (uint32_t)(64 * kMaxP), mine - (threadIdx.x & 63u), units};
  const size_t run_at = (size_t)run.first_unit * 8u;  // first pixel of the wave's run (its lane 0 exists, or nothing is stored)
  const uint32_t frame_groups = kConcat ? 1u : (job.src[0] ? 1u : 0u) + (job.src[1] ? 1u : 0u);
  const bool rgb = job.flags & 2;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    if (group < frame_groups) {
      const int f = (!kConcat && (group != 0u || !job.src[0])) ? 1 : 0;
      const float s3[3] = {rgb ? job.scale[2] : job.scale[0], job.scale[1], rgb ? job.scale[0] : job.scale[2]};  // by destination channel
      const float b3[3] = {rgb ? job.bias[2] : job.bias[0], job.bias[1], rgb ? job.bias[0] : job.bias[2]};
      const uint8_t* sp[kImgC];
      float scale[kImgC], bias[kImgC];
#pragma unroll
      for (int cd = 0; cd < kImgC; ++cd) {
        const uint8_t* const s = static_cast<const uint8_t*>((kConcat ? cd >= 3 : f != 0) ? job.src[1] : job.src[0]);
        const uint32_t c = rgb ? 2u - (uint32_t)(cd % 3) : (uint32_t)(cd % 3);  // the source channel
        sp[cd] = s + ((size_t)i * 3u * plane + c * plane + at) * kImgSES;
        scale[cd] = s3[cd % 3]; bias[cd] = b3[cd % 3];
      }
      uint8_t* const d = static_cast<uint8_t*>(f ? job.dst[1] : job.dst[0]);
      uint8_t* const dp = d + (kNhwc ? ((size_t)i * plane + run_at) * kImgC : (size_t)i * kImgC * plane + run_at) * kImgDES;
      pack_unit<kImgC, kImgSrc, kImgDst, kNhwc, true>(sp, scale, bias, dp, (size_t)plane * kImgDES, run);
    } else {
      const bool half = job.flow_src_fmt == OFDG_FMT_F16;
      const uint32_t ses = half ? 2u : 4u, des = job.flow_dst_fmt == OFDG_FMT_F32 ? 4u : 2u;
      const uint8_t* const s = static_cast<const uint8_t*>(job.src[2]);
      const uint8_t* const sp[2] = {s + ((size_t)i * 2u * plane + at) * ses, s + ((size_t)i * 2u * plane + plane + at) * ses};
      const float scale[2] = {job.flow_scale, job.flow_scale}, bias[2] = {0.0f, 0.0f};
      uint8_t* const dp = static_cast<uint8_t*>(job.dst[2]) + (kNhwc ? ((size_t)i * plane + run_at) * 2u : (size_t)i * 2u * plane + run_at) * des;
      const size_t chan_bytes = (size_t)plane * des;
      if (half) {
        if (job.flow_dst_fmt == OFDG_FMT_F32) pack_unit<2, kPackSrcF16, OFDG_FMT_F32, kNhwc, false>(sp, scale, bias, dp, chan_bytes, run);
        else if (job.flow_dst_fmt == OFDG_FMT_F16) pack_unit<2, kPackSrcF16, OFDG_FMT_F16, kNhwc, false>(sp, scale, bias, dp, chan_bytes, run);
        else pack_unit<2, kPackSrcF16, OFDG_FMT_BF16, kNhwc, false>(sp, scale, bias, dp, chan_bytes, run);
      } else {
        if (job.flow_dst_fmt == OFDG_FMT_F32) pack_unit<2, kPackSrcF32, OFDG_FMT_F32, kNhwc, false>(sp, scale, bias, dp, chan_bytes, run);
        else if (job.flow_dst_fmt == OFDG_FMT_F16) pack_unit<2, kPackSrcF32, OFDG_FMT_F16, kNhwc, false>(sp, scale, bias, dp, chan_bytes, run);
        else pack_unit<2, kPackSrcF32, OFDG_FMT_BF16, kNhwc, false>(sp, scale, bias, dp, chan_bytes, run);
      }
    }
  }
}

// ---- Motion boundaries (ofdg_boundaries, include/ofdg.h) -------------------------------------------------------------------
// A workgroup owns a kBndTileW x kBndTileH tile of one frame of one sample; blockIdx.x counts the tiles, blockIdx.y the
// samples, blockIdx.z the frames that are present.  Its REGION is the tile and a halo of R = radius pixels (0 when the frame
// has no dist2 plane), one more row above and one more column to the left for the steps that reach into it; what lies outside
// the plane holds no step, so nothing wraps.  Four passes, a workgroup barrier between them:
//   1. steps.   A wave takes 64 consecutive columns of a region row at a time: a lane decides whether its pixel and the one to
//               its right, and its pixel and the one below, are a step (boundary_step, the labels compared first: where they
//               agree the flow is not read), and __ballot makes the two 64-bit words of the run.  A region row is kBndWords words.
//   2. edge.    edge word = right | right << 1 (the carry from the word before) | down | down of the row above.
//   3. across.  For four tile columns of a region row at a time: the row's words shifted into a 31-bit window centred on the
//               column, the nearest set bit on either side by count-leading / count-trailing zeros, g^2 (or 255: none within
//               R) as a byte in LDS.
//   4. down.    A lane owns 8 consecutive columns of kBndOwn vertically adjacent rows: dist2 = min over |dy| <= R of dy^2 +
//               g^2(x, y + dy), kept where <= R^2; edge is the window's centre bit.  8 bytes per lane and plane, non-temporal.
// Element loads at checked indices only; no atomics, no scratch.  LDS: 12 KiB at 128 x 32.
constexpr int kBndThreads = 256;
#ifndef OFDG_BND_TILE_W
#define OFDG_BND_TILE_W 128
#endif
#ifndef OFDG_BND_TILE_H
#define OFDG_BND_TILE_H 32
#endif
constexpr int kBndTileW = OFDG_BND_TILE_W, kBndTileH = OFDG_BND_TILE_H;  // (measured against 64 x 32 and 128 x 64: CHANGELOG)
constexpr int kBndPad = kBndMaxRadius + 1;                             // region columns left of the tile
constexpr int kBndWords = (kBndTileW + 2 * kBndPad + 63) / 64;         // 64-column words of a region row
constexpr int kBndRows = kBndTileH + 2 * kBndMaxRadius;                // region rows at the largest radius
constexpr int kBndOwn = kBndTileW * kBndTileH / (8 * kBndThreads);     // rows of 8 columns a lane owns in pass 4
static_assert(kBndTileW % 64 == 0 && kBndOwn >= 1 && kBndOwn * 8 * kBndThreads == kBndTileW * kBndTileH && kBndThreads % (kBndTileW / 8) == 0 &&
              kBndTileW + kBndPad + kBndMaxRadius <= 64 * kBndWords, "a lane owns whole runs of 8 columns; the region fits its words");
// 8 bits -> 8 bytes of 1 / 0, the lowest bit in the lowest byte
__device__ __forceinline__ u32x2 bnd_spread(uint32_t bits) {
  return u32x2{((bits & 15u) * 0x00204081u) & 0x01010101u, (((bits >> 4) & 15u) * 0x00204081u) & 0x01010101u};
}
template <bool kHalf, bool kLabels>
__global__ __launch_bounds__(kBndThreads) void boundary_kernel(const DevBoundaryJob job, int n, int W, int H, uint32_t tiles_x) {
  __shared__ unsigned long long s_right[kBndRows + 1][kBndWords], s_down[kBndRows + 1][kBndWords];  // row 0: the row above the region
  __shared__ unsigned long long s_edge[kBndRows][kBndWords];
  __shared__ uint32_t s_g2[kBndRows][kBndTileW / 4];
  const int f = (blockIdx.z != 0u || !job.flow[0]) ? 1 : 0;
  const uint8_t* const s_flow = static_cast<const uint8_t*>(f ? job.flow[1] : job.flow[0]);
  const uint8_t* const s_lab = f ? job.label[1] : job.label[0];
  uint8_t* const d_edge = f ? job.edge[1] : job.edge[0];
  uint8_t* const d_dist = f ? job.dist2[1] : job.dist2[0];
  const int R = d_dist ? job.radius : 0;
  const float t2 = boundary_threshold(job.min_step);
  const int x0 = (int)(blockIdx.x % tiles_x) * kBndTileW, y0 = (int)(blockIdx.x / tiles_x) * kBndTileH;
  const int lane = (int)(threadIdx.x & 63u), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int rows = kBndTileH + 2 * R;  // region rows: row e is row y0 - R + e of the plane
  const int x_lo = max(x0 - R - 1, 0), x_hi = min(x0 + kBndTileW + R, W);  // columns whose steps the tile can see
  const size_t plane = (size_t)W * H;
  constexpr int kPerRow = kBndTileW / 8;
  const int col8 = (int)threadIdx.x % kPerRow, cy0 = (int)threadIdx.x / kPerRow * kBndOwn;  // pass 4: the lane's columns and first row
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    const uint8_t* const fl = s_flow + (size_t)i * 2 * plane * (kHalf ? 2 : 4);
    const uint8_t* const lab = s_lab + (size_t)i * plane;  // (read with kLabels only)
    for (int unit = wave; unit < (rows + 1) * kBndWords; unit += kBndThreads / 64) {
      const int ry = unit / kBndWords, w = unit - ry * kBndWords;
      const int y = y0 - R - 1 + ry, x = x0 - kBndPad + 64 * w + lane;
      unsigned long long right = 0ull, down = 0ull;
      if (y >= 0 && y < H) {
        const bool in = x >= x_lo && x < x_hi;
        bool want_r = in && x + 1 < W, want_d = in && y + 1 < H, step_r = false, step_d = false;
        const size_t p = (size_t)y * W + (size_t)(in ? x : 0);
        if constexpr (kLabels) {
          if (in) {
            const uint8_t l = lab[p];
            want_r = want_r && lab[p + 1] != l;
            want_d = want_d && lab[p + W] != l;
          }
        }
        if (want_r || want_d) {
          const float u = elem_load<quad_fmt(kHalf)>(fl, p), v = elem_load<quad_fmt(kHalf)>(fl, plane + p);
          if (want_r) step_r = boundary_step(u, v, elem_load<quad_fmt(kHalf)>(fl, p + 1), elem_load<quad_fmt(kHalf)>(fl, plane + p + 1), t2);
          if (want_d) step_d = boundary_step(u, v, elem_load<quad_fmt(kHalf)>(fl, p + W), elem_load<quad_fmt(kHalf)>(fl, plane + p + W), t2);
        }
        right = __ballot(step_r);
        down = __ballot(step_d);
      }
      if (lane == 0) { s_right[ry][w] = right; s_down[ry][w] = down; }
    }
    __syncthreads();
    for (int t = (int)threadIdx.x; t < rows * kBndWords; t += kBndThreads) {
      const int e = t / kBndWords, w = t - e * kBndWords;
      const unsigned long long r = s_right[e + 1][w];
      s_edge[e][w] = r | (r << 1) | (w ? s_right[e + 1][w - 1] >> 63 : 0ull) | s_down[e + 1][w] | s_down[e][w];
    }
    __syncthreads();
    if (d_dist) {
      for (int t = (int)threadIdx.x; t < rows * (kBndTileW / 4); t += kBndThreads) {
        const int e = t / (kBndTileW / 4), c4 = t - e * (kBndTileW / 4);
        const int first = 4 * c4 + kBndPad - kBndMaxRadius;  // the window of the first of the four columns starts at this bit
        const int w0 = first >> 6, sh = first & 63;
        unsigned long long chunk = s_edge[e][w0] >> sh;
        if (sh != 0 && w0 + 1 < kBndWords) chunk |= s_edge[e][w0 + 1] << (64 - sh);
        uint32_t g2 = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint32_t win = (uint32_t)(chunk >> b) & 0x7FFFFFFFu;  // bit 15: the column itself
          const uint32_t hi = win >> kBndMaxRadius, lo = win & 0x7FFFu;
          const int dr = hi ? __builtin_ctz(hi) : 64, dl = lo ? __builtin_clz(lo) - 16 : 64;
          const int g = min(dr, dl);
          g2 |= (g <= R ? (uint32_t)(g * g) : 255u) << (8 * b);
        }
        s_g2[e][c4] = g2;
      }
      __syncthreads();
    }
    const int X = x0 + 8 * col8;
    if (X < W) {  // (W is a multiple of 8: the lane's 8 columns exist or none does)
      if (d_dist) {
        uint32_t best[kBndOwn][8];
#pragma unroll
        for (int k = 0; k < kBndOwn; ++k)
#pragma unroll
          for (int b = 0; b < 8; ++b) best[k][b] = 255u;
        for (int r = 0; r < kBndOwn + 2 * R; ++r) {
          const uint2 g = *reinterpret_cast<const uint2*>(&s_g2[cy0 + r][2 * col8]);
#pragma unroll
          for (int k = 0; k < kBndOwn; ++k) {
            const int dy = r - R - k;  // region row cy0 + r against the lane's row cy0 + k
            const uint32_t dy2 = (dy < -R || dy > R) ? 255u : (uint32_t)(dy * dy);
#pragma unroll
            for (int b = 0; b < 8; ++b) best[k][b] = min(best[k][b], (((b < 4 ? g.x : g.y) >> (8 * (b & 3))) & 255u) + dy2);
          }
        }
        const uint32_t r2 = (uint32_t)(R * R);
#pragma unroll
        for (int k = 0; k < kBndOwn; ++k) {
          const int Y = y0 + cy0 + k;
          if (Y >= H) break;
          uint32_t o[8];
#pragma unroll
          for (int b = 0; b < 8; ++b) o[b] = best[k][b] <= r2 ? best[k][b] : 255u;
          __builtin_nontemporal_store(u32x2{o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24), o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24)},
                                      reinterpret_cast<u32x2*>(d_dist + (size_t)i * plane + (size_t)Y * W + X));
        }
      }
      if (d_edge) {
        const int bit = 8 * col8 + kBndPad;
#pragma unroll
        for (int k = 0; k < kBndOwn; ++k) {
          const int Y = y0 + cy0 + k;
          if (Y >= H) break;
          const uint32_t bits = (uint32_t)(s_edge[cy0 + k + R][bit >> 6] >> (bit & 63)) & 255u;
          __builtin_nontemporal_store(bnd_spread(bits), reinterpret_cast<u32x2*>(d_edge + (size_t)i * plane + (size_t)Y * W + X));
        }
      }
    }
    __syncthreads();  // (the words are written again for the next sample)
  }
}

// ---- Occluder rectangles (ofdg_erase, include/ofdg.h) ----------------------------------------------------------------------
// Two launches on the caller's stream, behind the clearing of `work` under OFDG_ERASE_MEAN: erase_mean_kernel adds the Q8 sums
// of the frames that have a rectangle, erase_apply_kernel paints the rectangles and extends the maps.  In place: the second
// launch starts after the first has ended - the order of the stream, nothing a workgroup waits for -, so no rectangle of a
// frame is painted before that frame's sum is complete, and no workgroup waits or spins for another.  Both kernels get the
// record of a sample the same way: read or drawn, and sanitised, on wave-uniform values (erase_record), so every workgroup of
// a sample holds the same rectangles in scalar registers.  The functions of the definition are the host twin's
// (csrc/ofdg_device.h), so the result is the twin's byte for byte.
constexpr int kEraseThreads = 256;
constexpr int kEraseMeanPixels = 32768;  // elements of a channel per reduction workgroup, as photo_kernel's: 6 per channel of a 512 x 384 frame
constexpr int kEraseFillSplit = 4;       // workgroups that share the rows of one (rectangle, plane): 16 rows in flight
constexpr int kEraseFillBlocks = kEraseMaxRects * 4 * kEraseFillSplit;  // planes of a rectangle: B, G, R and the map of its frame
constexpr int kEraseOccQuads = 1024;     // quads of a map per workgroup of the pass over flow and map, as flow_stats_kernel's
static_assert(kEraseMeanPixels % (kEraseThreads * 16) == 0 && (unsigned long long)kEraseMeanPixels * 65280ull < (1ull << 32),
              "whole rounds of pieces of either kind; a workgroup's Q8 sum fits 32 bits");
__device__ __forceinline__ DevEraseRec erase_record(const DevEraseJob& job, int i, int W, int H) {
  DevEraseRec r;
  if (job.recs) r = job.recs[i];
  else r = erase_draw_rec(job.seed, (unsigned long long)(job.first_index + i), W, H, job);
  return erase_sanitise(r, W, H, job.flags);
}
// rectangle k of a record for a wave-uniform k, through selects (no indexed access: the record stays in registers), pinned
// to scalar registers
// (arguments by value: a conditional between members would select their addresses and pin the record to memory)
__device__ __forceinline__ int erase_pick4(int k, int v0, int v1, int v2, int v3) { return k == 0 ? v0 : k == 1 ? v1 : k == 2 ? v2 : v3; }
__device__ __forceinline__ DevEraseRect erase_rect_at(const DevEraseRec& r, int k) {
#define OFDG_ERASE_PICK(field) __builtin_amdgcn_readfirstlane(erase_pick4(k, r.rect[0].field, r.rect[1].field, r.rect[2].field, r.rect[3].field))
  return DevEraseRect{OFDG_ERASE_PICK(x0), OFDG_ERASE_PICK(y0), OFDG_ERASE_PICK(w), OFDG_ERASE_PICK(h), OFDG_ERASE_PICK(frame)};
#undef OFDG_ERASE_PICK
}

// The mean's reduction.  blockIdx.x counts the kEraseMeanPixels-element blocks of the channels of the flagged frames,
// blockIdx.y the samples.  A sample whose record has no rectangle in the workgroup's frame is left before any load.  A lane
// reads pieces - 16 bytes of float32, four 4-byte words of uint8 - as photo_kernel does, sums Q8 values in 32 bits (at most
// 128 elements of 65280), the wave adds across with __shfl_xor, the workgroup through LDS, and one 64-bit integer atomicAdd
// per workgroup goes to the sample's sum of (frame, channel) in `work`.  Integers only: no bit depends on arrival order.
template <bool kU8>
__global__ __launch_bounds__(kEraseThreads) void erase_mean_kernel(const DevEraseJob job, int n, int W, int H, uint32_t per_channel) {
  constexpr int kP = kU8 ? 16 : 4;  // elements of a piece
  __shared__ uint32_t s_part[kEraseThreads / 64];
  const uint32_t slot = blockIdx.x / per_channel, block = blockIdx.x - slot * per_channel;
  const int f = (job.flags & 3) == 3 ? (int)(slot / 3u) : (job.flags & 3) == 2 ? 1 : 0, c = (int)(slot % 3u);
  const void* const src = f ? job.image[1] : job.image[0];
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (3 * plane < 2^31: erase_arg_error)
  const uint32_t first = block * (uint32_t)kEraseMeanPixels;
  const uint32_t end = first + (uint32_t)kEraseMeanPixels < plane ? first + (uint32_t)kEraseMeanPixels : plane;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    const DevEraseRec r = erase_record(job, i, W, H);
    if (!((erase_frames_of(r) >> f) & 1)) continue;  // (uniform over the workgroup)
    const size_t chan = ((size_t)i * 3 + (size_t)c) * plane;
    uint32_t sum = 0;
    for (uint32_t at = first + threadIdx.x * (uint32_t)kP; at < end; at += (uint32_t)(kEraseThreads * kP)) {
      if constexpr (kU8) {
        const uint32_t* const sp = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(src) + chan + at);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t w = sp[q];
          sum += (w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24);
        }
      } else {
        const float4 e = *reinterpret_cast<const float4*>(static_cast<const float*>(src) + chan + at);
        sum += erase_q8(e.x) + erase_q8(e.y) + erase_q8(e.z) + erase_q8(e.w);
      }
    }
    if constexpr (kU8) sum *= 256u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, 64);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long total = 0;
#pragma unroll
      for (int w = 0; w < kEraseThreads / 64; ++w) total += s_part[w];
      atomicAdd(f ? &job.work[i].sum[1][c] : &job.work[i].sum[0][c], total);
    }
    __syncthreads();  // (the next sample of this workgroup writes the parts again)
  }
}

// One row piece of a rectangle: w elements of kB bytes from element number e0 of the sample's plane `base`, by one wave.  The
// row starts anywhere, so the elements up to the first 16-byte boundary and those behind the last whole piece are stored
// singly and the pieces between with 16-byte non-temporal stores.  A piece starts at an element number that is a multiple of
// 4 (the plane's base is 4-byte aligned at least and a sample's planes are multiples of 16 elements), so the noise of a piece
// is whole Philox blocks.
template <int kB>
__device__ __forceinline__ void erase_fill_row(uint8_t* base, uint32_t e0, int w, int lane, bool noise, uint32_t k0, uint32_t k1, int f, uint32_t byte) {
  constexpr int kP = 16 / kB;  // elements of a piece
  const uint32_t addr = (uint32_t)(uintptr_t)(base + (size_t)e0 * kB);
  const int to_boundary = (int)(((16u - (addr & 15u)) & 15u) / (uint32_t)kB);
  const int head = to_boundary < w ? to_boundary : w;
  const int pieces = (w - head) / kP;
  const int tail0 = head + pieces * kP;
  const int singles = head + (w - tail0);
  for (int t = lane; t < singles; t += 64) {
    const uint32_t e = e0 + (uint32_t)(t < head ? t : tail0 + (t - head));
    const uint32_t b = noise ? erase_noise_byte(k0, k1, f, e) : byte;
    if constexpr (kB == 1) base[e] = (uint8_t)b;
    else reinterpret_cast<float*>(base)[e] = (float)b;
  }
  for (int p = lane; p < pieces; p += 64) {
    const uint32_t e = e0 + (uint32_t)(head + p * kP);
    u32x4 o;
    if (noise) {
#pragma unroll
      for (int q = 0; q < kP / 4; ++q) {
        const CropWords nw = crop_philox(CropWords{(e >> 2) + (uint32_t)q, (uint32_t)f, 0x0c75u, 0u}, k0, k1);
        if constexpr (kB == 1) o[q] = (nw.x >> 24) | ((nw.y >> 24) << 8) | ((nw.z >> 24) << 16) | ((nw.w >> 24) << 24);
        else o = u32x4{__float_as_uint((float)(nw.x >> 24)), __float_as_uint((float)(nw.y >> 24)), __float_as_uint((float)(nw.z >> 24)), __float_as_uint((float)(nw.w >> 24))};
      }
    } else {
      const uint32_t v = kB == 1 ? byte * 0x01010101u : __float_as_uint((float)byte);
      o = u32x4{v, v, v, v};
    }
    quad_store_u32x4(reinterpret_cast<u32x4*>(base + (size_t)e * kB), o);
  }
}

// Painting and marking.  blockIdx.y counts the samples; blockIdx.x first the kEraseFillBlocks fill workgroups - (rectangle k,
// plane B / G / R / the map of the rectangle's frame, one of kEraseFillSplit shares of its rows), a wave per row, so only the
// rectangles' rows are touched and a sample without rectangles does no memory traffic - and then, per map given under
// OFDG_ERASE_OCC, the workgroups of a pass over flow[f] and occ[f] in quads as flow_stats_kernel reads them.  That pass runs
// only for a sample with a rectangle in frame 1 - f (and that frame flagged); it then also makes the direct marks of the
// rectangles of frame f, and the fill workgroups leave that map alone - so every element of a map has one writer.  A quad of
// the map is read and written back only where a mark falls into it.  The fill byte of the mean comes from the sums the first
// launch left in `work`; workgroup 0 writes the sanitised record with the fill bytes from lane 0 with six vector stores.
template <bool kU8, bool kOccU8, bool kHalf>
__global__ __launch_bounds__(kEraseThreads) void erase_apply_kernel(const DevEraseJob job, int n, int W, int H, uint32_t occ_blocks) {
  constexpr int kB = kU8 ? 1 : 4, kOB = kOccU8 ? 1 : 4;
  typedef typename FlowFmt<quad_fmt(kHalf)>::quad FlowQuad;
  const uint32_t plane = (uint32_t)W * (uint32_t)H;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const bool mark = job.flags & OFDG_ERASE_OCC;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    const DevEraseRec r = erase_record(job, i, W, H);
    const int frames = erase_frames_of(r);
    const unsigned long long g = (unsigned long long)(job.first_index + i);
    const uint32_t k0 = job.seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
    if (job.recs_out && blockIdx.x == 0u && threadIdx.x == 0u) {
      uint32_t fb[6];
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const int f = s / 3, c = s % 3;
        fb[s] = !((frames >> f) & 1) || job.fill == OFDG_ERASE_NOISE ? 0u
                : job.fill == OFDG_ERASE_CONST ? (uint32_t)job.color[c] : erase_mean_byte(job.work[i].sum[f][c], plane);
      }
      u32x4* const o = reinterpret_cast<u32x4*>(job.recs_out + i);
      const DevEraseRect q0 = r.rect[0], q1 = r.rect[1], q2 = r.rect[2], q3 = r.rect[3];
      o[0] = u32x4{(uint32_t)r.count, (uint32_t)q0.x0, (uint32_t)q0.y0, (uint32_t)q0.w};
      o[1] = u32x4{(uint32_t)q0.h, (uint32_t)q0.frame, (uint32_t)q1.x0, (uint32_t)q1.y0};
      o[2] = u32x4{(uint32_t)q1.w, (uint32_t)q1.h, (uint32_t)q1.frame, (uint32_t)q2.x0};
      o[3] = u32x4{(uint32_t)q2.y0, (uint32_t)q2.w, (uint32_t)q2.h, (uint32_t)q2.frame};
      o[4] = u32x4{(uint32_t)q3.x0, (uint32_t)q3.y0, (uint32_t)q3.w, (uint32_t)q3.h};
      o[5] = u32x4{(uint32_t)q3.frame, fb[0] | (fb[1] << 8) | (fb[2] << 16) | (fb[3] << 24), fb[4] | (fb[5] << 8), 0u};
    }
    if (blockIdx.x < (uint32_t)kEraseFillBlocks) {
      const int k = (int)blockIdx.x / (4 * kEraseFillSplit), pl = ((int)blockIdx.x / kEraseFillSplit) % 4, part = (int)blockIdx.x % kEraseFillSplit;
      if (k >= r.count) continue;
      const DevEraseRect q = erase_rect_at(r, k);
      const int f = q.frame;
      if (pl == 3) {  // the direct marks of the rectangle, unless the pass below serves this map
        uint8_t* const map = static_cast<uint8_t*>(f ? job.occ[1] : job.occ[0]);
        if (!mark || !map || (erase_cross(job, f) && ((frames >> (1 - f)) & 1))) continue;
        uint8_t* const base = map + (size_t)i * plane * kOB;
        for (int y = q.y0 + part * 4 + wave; y < q.y0 + q.h; y += 4 * kEraseFillSplit)
          erase_fill_row<kOB>(base, (uint32_t)y * (uint32_t)W + (uint32_t)q.x0, q.w, lane, false, 0u, 0u, 0, 1u);
      } else {
        const bool noise = job.fill == OFDG_ERASE_NOISE;
        const uint32_t byte = noise ? 0u : job.fill == OFDG_ERASE_CONST ? (uint32_t)(pl == 0 ? job.color[0] : pl == 1 ? job.color[1] : job.color[2])
                                         : erase_mean_byte(f ? job.work[i].sum[1][pl] : job.work[i].sum[0][pl], plane);
        uint8_t* const base = static_cast<uint8_t*>(f ? job.image[1] : job.image[0]) + (size_t)i * 3 * plane * kB;
        for (int y = q.y0 + part * 4 + wave; y < q.y0 + q.h; y += 4 * kEraseFillSplit)
          erase_fill_row<kB>(base, (uint32_t)pl * plane + (uint32_t)y * (uint32_t)W + (uint32_t)q.x0, q.w, lane, noise, k0, k1, f, byte);
      }
    } else {
      const uint32_t b = blockIdx.x - (uint32_t)kEraseFillBlocks;
      const int f = job.occ[0] && job.occ[1] ? (int)(b / occ_blocks) : job.occ[0] ? 0 : 1;
      if (!erase_cross(job, f) || !((frames >> (1 - f)) & 1)) continue;
      DevEraseRec rs;  // the four rectangles in scalar registers (fill and reserved are not read)
      rs.rect[0] = erase_rect_at(r, 0);
      rs.rect[1] = erase_rect_at(r, 1);
      rs.rect[2] = erase_rect_at(r, 2);
      rs.rect[3] = erase_rect_at(r, 3);
      rs.count = __builtin_amdgcn_readfirstlane(r.count);
      const uint32_t plane_quads = plane / 4u;
      const uint32_t q_begin = (b % occ_blocks) * (uint32_t)kEraseOccQuads;
      const uint32_t q_end = min(q_begin + (uint32_t)kEraseOccQuads, plane_quads);
      const void* const flow = f ? job.flow[1] : job.flow[0];
      void* const map = f ? job.occ[1] : job.occ[0];
      const size_t pu = (size_t)i * 2 * plane_quads, pv = pu + plane_quads, po = (size_t)i * plane_quads;  // in quads
      for (uint32_t qd = q_begin + threadIdx.x; qd < q_end; qd += (uint32_t)kEraseThreads) {
        float u[4], v[4];
        quad_load<quad_fmt(kHalf)>(static_cast<const FlowQuad*>(flow) + (pu + qd), u);
        quad_load<quad_fmt(kHalf)>(static_cast<const FlowQuad*>(flow) + (pv + qd), v);
        const uint32_t at = qd * 4u;
        const int y = (int)(at / (uint32_t)W), x = (int)(at - (uint32_t)y * (uint32_t)W);  // (W % 8 == 0: a quad lies in one row)
        uint32_t hits = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) hits |= (erase_marks(rs, f, true, x + s, y, u[s], v[s]) ? 1u : 0u) << s;
        if (!hits) continue;
        if constexpr (kOccU8) {
          uint32_t* const p = reinterpret_cast<uint32_t*>(map) + po + qd;
          uint32_t o = *p;
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if ((hits >> s) & 1u) o = (o & ~(255u << (8 * s))) | (1u << (8 * s));
          *p = o;
        } else {
          f32x4* const p = reinterpret_cast<f32x4*>(map) + po + qd;
          f32x4 o = *p;
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if ((hits >> s) & 1u) o[s] = 1.0f;
          *p = o;
        }
      }
    }
  }
}

// ---- Colour jitter (ofdg_jitter, include/ofdg.h) ---------------------------------------------------------------------------
// Two launches on the caller's stream, behind the clearing of `work` where a record may hold a contrast: jitter_mean_kernel
// adds the luminance sums of the frames whose contrast needs a mean, jitter_apply_kernel runs the four operations.  The second
// launch starts after the first has ended - the order of the stream -, so no pixel is written before its frame's sum is
// complete (the in-place form reads the un-jittered frame in both launches), and no workgroup waits for another.  A
// workgroup serves kJitterBlockPixels consecutive pixels of one (sample, frame), all three channels: a lane takes the same
// piece of the B, G and R plane, reads the three whole, works on the bytes in registers and - in the second launch - writes the
// three back, which is all the in-place form needs.  The record is read or drawn, and sanitised, on wave-uniform values once
// per (workgroup, sample); the frame's five fields are pinned to scalar registers, so the switch over the operation at a place
// of the order does not diverge, and an operation at its identity is stepped over.  The functions of the definition are the
// host twin's (csrc/ofdg_device.h), so the result is the twin's byte for byte.  No scratch; 16 bytes of LDS in the reduction.
constexpr int kJitterThreads = 256;
#ifndef OFDG_JITTER_BLOCK_PIXELS
#define OFDG_JITTER_BLOCK_PIXELS 8192
#endif
constexpr int kJitterBlockPixels = OFDG_JITTER_BLOCK_PIXELS;  // 24 workgroups per 512 x 384 frame: two rounds of 16-pixel pieces, eight of 4-pixel ones
static_assert(kJitterBlockPixels % (kJitterThreads * 16) == 0 && (unsigned long long)kJitterBlockPixels * 255ull < (1ull << 32),
              "whole rounds of pieces of either kind; a workgroup's luminance sum fits 32 bits");
__device__ __forceinline__ DevJitterRec jitter_record(const DevJitterJob& job, int i) {
  DevJitterRec r;
  if (job.recs) r = job.recs[i];
  else r = jitter_draw_rec(job.seed, (unsigned long long)(job.first_index + i), job);
  return jitter_sanitise(r);
}
__device__ __forceinline__ JitterFrame jitter_frame_uniform(const DevJitterRec& r, int f) {
  const JitterFrame p = jitter_frame(r, f);
  return JitterFrame{__builtin_amdgcn_readfirstlane(p.brightness), __builtin_amdgcn_readfirstlane(p.contrast), __builtin_amdgcn_readfirstlane(p.saturation),
                     __builtin_amdgcn_readfirstlane(p.hue), __builtin_amdgcn_readfirstlane(p.order)};
}
// the bytes of kP consecutive elements from element `at` of one channel: uint8 as 4-byte words (the alignment asked of a
// source), float32 as 16-byte ones through the index rule
template <bool kU8, int kP>
__device__ __forceinline__ void jitter_load_channel(const void* src, size_t at, int (&v)[kP]) {
  typedef typename std::conditional<kU8, uint8_t, float>::type SrcT;
  const SrcT* const sp = static_cast<const SrcT*>(src) + at;
#pragma unroll
  for (int q = 0; q < kP / 4; ++q) quad_load_bytes<kU8>(sp + 4 * q, v + 4 * q);
}
// one 16-byte piece of a destination channel: 16 bytes, or 4 times (float)byte
template <bool kU8, int kP>
__device__ __forceinline__ void jitter_store_channel(void* dst, size_t at, const int (&v)[kP]) {
  u32x4 o;
  if constexpr (kU8) {
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (uint32_t)v[4 * q] | ((uint32_t)v[4 * q + 1] << 8) | ((uint32_t)v[4 * q + 2] << 16) | ((uint32_t)v[4 * q + 3] << 24);
    quad_store_u32x4(reinterpret_cast<u32x4*>(static_cast<uint8_t*>(dst) + at), o);
  } else {
    o = u32x4{__float_as_uint((float)v[0]), __float_as_uint((float)v[1]), __float_as_uint((float)v[2]), __float_as_uint((float)v[3])};
    quad_store_u32x4(reinterpret_cast<u32x4*>(static_cast<float*>(dst) + at), o);
  }
}
// The operations at the places [0, places) of `ops` on kP pixels.  The place loop stays a loop, its switch is uniform; the
// pixels of a case are unrolled, so the arrays are registers.
template <int kP>
__device__ __forceinline__ void jitter_run(uint32_t ops, int places, const JitterFrame& p, int mean, int (&B)[kP], int (&G)[kP], int (&R)[kP]) {
#pragma unroll 1
  for (int place = 0; place < places; ++place) {
    switch (jitter_op_at(ops, place)) {
      case kJitterBrightness:
        if (p.brightness == kJitterOne) break;
#pragma unroll
        for (int q = 0; q < kP; ++q) { B[q] = jitter_mix(B[q], 0, p.brightness); G[q] = jitter_mix(G[q], 0, p.brightness); R[q] = jitter_mix(R[q], 0, p.brightness); }
        break;
      case kJitterContrast:
        if (p.contrast == kJitterOne) break;
#pragma unroll
        for (int q = 0; q < kP; ++q) { B[q] = jitter_mix(B[q], mean, p.contrast); G[q] = jitter_mix(G[q], mean, p.contrast); R[q] = jitter_mix(R[q], mean, p.contrast); }
        break;
      case kJitterSaturation:
        if (p.saturation == kJitterOne) break;
#pragma unroll
        for (int q = 0; q < kP; ++q) {
          const int l = jitter_lum(B[q], G[q], R[q]);
          B[q] = jitter_mix(B[q], l, p.saturation); G[q] = jitter_mix(G[q], l, p.saturation); R[q] = jitter_mix(R[q], l, p.saturation);
        }
        break;
      default:
        if (p.hue == 0) break;
#pragma unroll
        for (int q = 0; q < kP; ++q) jitter_hue(B[q], G[q], R[q], p.hue);
        break;
    }
  }
}

// The mean's reduction.  blockIdx.x counts the kJitterBlockPixels-pixel blocks of the frames that are set, blockIdx.y the
// samples.  A workgroup whose (sample, frame) has no contrast leaves before any load.  A lane reads pieces of the source - 16
// bytes of float32, four 4-byte words of uint8 - of all three channels, runs the operations that stand before the contrast,
// sums the luminances in 32 bits (at most 32 pixels of 255), the wave adds across with __shfl_xor, the workgroup through LDS,
// and one 64-bit integer atomicAdd per workgroup goes to the frame's sum in `work`.  Integers only: no bit depends on arrival
// order.
template <bool kU8>
__global__ __launch_bounds__(kJitterThreads) void jitter_mean_kernel(const DevJitterJob job, int n, int W, int H, uint32_t per_frame) {
  constexpr int kP = kU8 ? 16 : 4;  // pixels of a piece
  __shared__ uint32_t s_part[kJitterThreads / 64];
  const uint32_t slot = blockIdx.x / per_frame, block = blockIdx.x - slot * per_frame;
  const int f = (int)slot + (job.src[0] ? 0 : 1);
  const void* const src = f ? job.src[1] : job.src[0];
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (3 * plane < 2^32: jitter_arg_error)
  const uint32_t first = block * (uint32_t)kJitterBlockPixels;
  const uint32_t end = first + (uint32_t)kJitterBlockPixels < plane ? first + (uint32_t)kJitterBlockPixels : plane;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    const DevJitterRec r = jitter_record(job, i);
    const JitterFrame p = jitter_frame_uniform(r, f);
    if (p.contrast == kJitterOne) continue;  // (uniform over the workgroup)
    const uint32_t ops = jitter_ops(p.order);
    const int places = jitter_contrast_place(ops);
    const size_t base = (size_t)i * 3 * plane;
    uint32_t sum = 0;
    for (uint32_t at = first + threadIdx.x * (uint32_t)kP; at < end; at += (uint32_t)(kJitterThreads * kP)) {
      int B[kP], G[kP], R[kP];
      jitter_load_channel<kU8, kP>(src, base + at, B);
      jitter_load_channel<kU8, kP>(src, base + plane + at, G);
      jitter_load_channel<kU8, kP>(src, base + 2 * (size_t)plane + at, R);
      jitter_run<kP>(ops, places, p, 0, B, G, R);
#pragma unroll
      for (int q = 0; q < kP; ++q) sum += (uint32_t)jitter_lum(B[q], G[q], R[q]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, 64);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long total = 0;
#pragma unroll
      for (int w = 0; w < kJitterThreads / 64; ++w) total += s_part[w];
      atomicAdd(f ? &job.work[i].sum[1] : &job.work[i].sum[0], total);
    }
    __syncthreads();  // (the next sample of this workgroup writes the parts again)
  }
}

// The byte the contrast of frame f of sample i pivots on, from the sums the first launch left in `work`; -1 for an absent
// frame and for one without a contrast (`work` is not read then: it may be NULL where no record can hold a contrast).
__device__ __forceinline__ int jitter_mean_of(const DevJitterJob& job, const DevJitterRec& r, int i, int f, uint32_t plane) {
  if (!(f ? job.src[1] : job.src[0]) || (f ? r.contrast[1] : r.contrast[0]) == kJitterOne) return -1;
  const bool joint = r.shared && job.src[0] && job.src[1];
  const unsigned long long s0 = job.work[i].sum[0], s1 = job.work[i].sum[1];
  return jitter_mean_byte(joint ? s0 + s1 : f ? s1 : s0, joint ? 2ull * plane : (unsigned long long)plane);
}

// The operations.  The grid is jitter_mean_kernel's; a piece is what one 16-byte store holds of the destination - 4 float32 or
// 16 uint8 -, lane t takes the pieces t, t + 256, ... of the block, so a wave's store instruction writes 1 KiB of consecutive
// bytes per channel.  A frame at the identity is copied bit for bit where the formats agree - and left alone in place -, and
// goes through its bytes where they differ.  Workgroup 0 of a sample writes the sanitised record with both means from lane 0
// with four vector stores.
template <bool kSrcU8, bool kDstU8>
__global__ __launch_bounds__(kJitterThreads) void jitter_apply_kernel(const DevJitterJob job, int n, int W, int H, uint32_t per_frame) {
  constexpr int kP = kDstU8 ? 16 : 4;  // pixels of a piece
  const uint32_t slot = blockIdx.x / per_frame, block = blockIdx.x - slot * per_frame;
  const int f = (int)slot + (job.src[0] ? 0 : 1);
  const void* const src = f ? job.src[1] : job.src[0];
  void* const dst = f ? job.dst[1] : job.dst[0];
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (3 * plane < 2^32: jitter_arg_error)
  const uint32_t first = block * (uint32_t)kJitterBlockPixels;
  const uint32_t end = first + (uint32_t)kJitterBlockPixels < plane ? first + (uint32_t)kJitterBlockPixels : plane;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    const DevJitterRec r = jitter_record(job, i);
    if (job.recs_out && blockIdx.x == 0u && threadIdx.x == 0u) {
      const int m0 = jitter_mean_of(job, r, i, 0, plane), m1 = jitter_mean_of(job, r, i, 1, plane);
      u32x4* const o = reinterpret_cast<u32x4*>(job.recs_out + i);
      o[0] = u32x4{(uint32_t)r.brightness[0], (uint32_t)r.brightness[1], (uint32_t)r.contrast[0], (uint32_t)r.contrast[1]};
      o[1] = u32x4{(uint32_t)r.saturation[0], (uint32_t)r.saturation[1], (uint32_t)r.hue[0], (uint32_t)r.hue[1]};
      o[2] = u32x4{(uint32_t)r.order[0], (uint32_t)r.order[1], (uint32_t)r.shared, (uint32_t)m0};
      o[3] = u32x4{(uint32_t)m1, 0u, 0u, 0u};
    }
    const JitterFrame p = jitter_frame_uniform(r, f);
    const size_t base = (size_t)i * 3 * plane;
    if (jitter_identity(p)) {  // (uniform over the workgroup)
      if constexpr (kSrcU8 == kDstU8) {
        if (src == dst) continue;
        constexpr int kB = kSrcU8 ? 1 : 4;
        for (int c = 0; c < 3; ++c)
          for (uint32_t at = first + threadIdx.x * (uint32_t)kP; at < end; at += (uint32_t)(kJitterThreads * kP)) {
            const size_t e = (base + (size_t)c * plane + at) * kB;
            const uint32_t* const sp = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(src) + e);
            quad_store_u32x4(reinterpret_cast<u32x4*>(static_cast<uint8_t*>(dst) + e), u32x4{sp[0], sp[1], sp[2], sp[3]});
          }
        continue;
      }
    }
    const int mean = __builtin_amdgcn_readfirstlane(jitter_mean_of(job, r, i, f, plane));
    const uint32_t ops = jitter_ops(p.order);
    for (uint32_t at = first + threadIdx.x * (uint32_t)kP; at < end; at += (uint32_t)(kJitterThreads * kP)) {
      int B[kP], G[kP], R[kP];
      jitter_load_channel<kSrcU8, kP>(src, base + at, B);
      jitter_load_channel<kSrcU8, kP>(src, base + plane + at, G);
      jitter_load_channel<kSrcU8, kP>(src, base + 2 * (size_t)plane + at, R);
      jitter_run<kP>(ops, 4, p, mean, B, G, R);
      jitter_store_channel<kDstU8, kP>(dst, base + at, B);
      jitter_store_channel<kDstU8, kP>(dst, base + plane + at, G);
      jitter_store_channel<kDstU8, kP>(dst, base + 2 * (size_t)plane + at, R);
    }
  }
}

// ---- Motion blur (ofdg_motion_blur, include/ofdg.h) ------------------------------------------------------------------------
// One launch for both frames and every sample: blockIdx.x counts the kMblurTileW x kMblurTileH tiles of a frame, blockIdx.y
// the samples, blockIdx.z the frames that are set.  A 4-wave workgroup owns a tile, a lane four consecutive pixels of one row
// (width % 8 == 0: a lane's four pixels, and the eight of a pair of lanes, are whole or outside together), so a wave's loads
// of the centre pieces and of the flow are whole consecutive rows of the tile.  The record is drawn or read, and sanitised,
// on uniform values once per (workgroup, sample) and stays in scalar registers; workgroup 0 writes it back from lane 0 with
// one vector store.  A frame whose shutter is 0 reads no flow.  The workgroup then takes one of three paths, agreed on
// through one word of LDS per wave (two ballots packed into it, no atomics; eight words in all: a row of four per parity
// of the sample's turn):
//   copy    no pixel of the tile has a tap beside its centre (m = 0 everywhere): every lane stores the bytes of the centre
//           piece it read whole; nothing is staged.
//   window  every tap of the tile lies within kMblurHalo pixels of its pixel: the tile and that halo - (64 + 33) x (16 + 33)
//           pixels, one dword each: B, G, R packed, the float32-to-byte rule applied once on the way in, the border
//           replicated, so the clamp of ix + 1 and iy + 1 is the window's own - go to LDS (18.6 KiB), and a tap is four
//           ds_read_b32 (two pairs of neighbours) for all three channels.
//   gather  some streak is longer than the halo: every pixel of the tile gathers its taps from global memory at clamped
//           indices (ubyte / dword loads), the coordinates of a tap computed once for the three channels.
// With OFDG_MBLUR_WINDOW=0 the window path is compiled out (the all-global-gather variant: CHANGELOG).  No record or flow
// reaches outside a plane or the window: every index is clamped, and the window path is taken only when m |step| <= 256
// kMblurHalo on both axes for every pixel of the tile.  Stores are whole pieces, non-temporal: 16 bytes of float32 a lane,
// 8 bytes of uint8 a pair of lanes (a row of uint8 starts at a multiple of 8 bytes only), gathered by the even lane with a
// wave shuffle.  The functions of the definition are the host twin's (csrc/ofdg_device.h), so the result is the twin's byte
// for byte.  No atomics, no scratch.
constexpr int kMblurThreads = 256;
constexpr int kMblurTileW = 64, kMblurTileH = 16;
#ifndef OFDG_MBLUR_WINDOW
#define OFDG_MBLUR_WINDOW 1
#endif
constexpr bool kMblurWindow = OFDG_MBLUR_WINDOW != 0;
constexpr int kMblurHalo = 16;  // pixels of halo on every side of the tile (and one more column and row for ix + 1, iy + 1)
constexpr int kMblurWinW = kMblurTileW + 2 * kMblurHalo + 1, kMblurWinH = kMblurTileH + 2 * kMblurHalo + 1;
static_assert(kMblurTileW / 4 * kMblurTileH == kMblurThreads, "a lane per four pixels of the tile");
template <bool kSrcU8, bool kDstU8, bool kFlowHalf>
__global__ __launch_bounds__(kMblurThreads) void mblur_kernel(const DevMblurJob job, int n, int W, int H, uint32_t tiles_x) {
  constexpr int kSES = kSrcU8 ? 1 : 4, kDES = kDstU8 ? 1 : 4, kFES = kFlowHalf ? 2 : 4;
  __shared__ uint32_t win[kMblurWindow ? kMblurWinW * kMblurWinH : 1];
  __shared__ uint32_t paths[2][kMblurThreads / 64];  // [parity of the sample's turn][wave]: bit 0 a tap beside the centre, bit 1 one beyond the halo
  const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int X0 = (int)(tx * kMblurTileW + (threadIdx.x & 15u) * 4u), Y = (int)(ty * kMblurTileH + (threadIdx.x >> 4));
  const int wx0 = (int)(tx * kMblurTileW) - kMblurHalo, wy0 = (int)(ty * kMblurTileH) - kMblurHalo;  // the window's first column and row in the frame
  const int f = (blockIdx.z != 0u || !job.src[0]) ? 1 : 0;
  const uint8_t* const s_img = static_cast<const uint8_t*>(f ? job.src[1] : job.src[0]);
  const uint8_t* const s_flow = static_cast<const uint8_t*>(f ? job.flow[1] : job.flow[0]);
  uint8_t* const d_img = static_cast<uint8_t*>(f ? job.dst[1] : job.dst[0]);
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (3 * plane < 2^32: mblur_arg_error)
  const bool inside = X0 < W && Y < H;
  const uint32_t at = inside ? (uint32_t)Y * (uint32_t)W + (uint32_t)X0 : 0u;  // the lane's first pixel in a channel
  const int cap = job.taps_side;
  uint32_t turn = 0u;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y, turn ^= 1u) {
    DevMblurRec r;
    if (job.recs) r = job.recs[i];
    else r = mblur_draw_rec(job.seed, (unsigned long long)(job.first_index + i), job);
    r = mblur_sanitise(r);
    if (job.recs_out && blockIdx.x == 0u && blockIdx.z == 0u && threadIdx.x == 0u)
      *reinterpret_cast<u32x4*>(job.recs_out + i) = u32x4{__float_as_uint(r.shutter[0]), __float_as_uint(r.shutter[1]), 0u, 0u};
    const float s = f ? r.shutter[1] : r.shutter[0];
    const uint8_t* const sp = s_img + (size_t)i * 3 * plane * kSES;
    uint32_t out[3][4] = {};  // the bytes to store: the centre piece, unless taps say otherwise
    float u[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (inside) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {  // (quad_load_bytes, spelled out: through the call the float32-source kernels were scheduled
                                     // otherwise, 27 instructions longer, and the copy path measured 1 - 2 % slower)
        if constexpr (kSrcU8) {
          const uint32_t w = *reinterpret_cast<const uint32_t*>(sp + (uint32_t)c * plane + at);
          out[c][0] = w & 255u; out[c][1] = (w >> 8) & 255u; out[c][2] = (w >> 16) & 255u; out[c][3] = w >> 24;
        } else {
          const f32x4 e = *reinterpret_cast<const f32x4*>(sp + ((size_t)c * plane + at) * 4u);
#pragma unroll
          for (int p = 0; p < 4; ++p) out[c][p] = (uint32_t)photo_index(e[p]);
        }
      }
      if (s > 0.0f) {  // (uniform: a frame with shutter 0 reads no flow)
        const uint8_t* const fp = s_flow + ((size_t)i * 2 * plane + at) * kFES;
        quad_load<quad_fmt(kFlowHalf)>(fp, u);
        quad_load<quad_fmt(kFlowHalf)>(fp + (size_t)plane * kFES, v);
      }
    }
    int m[4], sx[4], sy[4];
    bool blurred = false, far = false;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool finite = flow_finite(u[p]) && flow_finite(v[p]);
      const int Dx = finite ? mblur_half(u[p], s) : 0, Dy = finite ? mblur_half(v[p], s) : 0;
      m[p] = mblur_taps_side(Dx, Dy, cap);
      sx[p] = m[p] ? mblur_step(Dx, m[p]) : 0;
      sy[p] = m[p] ? mblur_step(Dy, m[p]) : 0;
      blurred = blurred || m[p] != 0;
      far = far || m[p] * mblur_abs(sx[p]) > 256 * kMblurHalo || m[p] * mblur_abs(sy[p]) > 256 * kMblurHalo;
    }
    // the path of the workgroup (every lane is here: a lane outside the frame has m = 0)
    const uint32_t mine = (__any(blurred) ? 1u : 0u) | (__any(far) ? 2u : 0u);
    if ((threadIdx.x & 63u) == 0u) paths[turn][threadIdx.x >> 6] = mine;
    __syncthreads();  // (a wave is at most one barrier ahead of another, and the next sample's words go to the other row)
    const uint32_t path = paths[turn][0] | paths[turn][1] | paths[turn][2] | paths[turn][3];
    if (kMblurWindow && path == 1u) {
      for (int j = (int)threadIdx.x; j < kMblurWinW * kMblurWinH; j += kMblurThreads) {
        const int wy = j / kMblurWinW, wx = j - wy * kMblurWinW;
        const uint32_t e = (uint32_t)spatial_clamp(wy0 + wy, H) * (uint32_t)W + (uint32_t)spatial_clamp(wx0 + wx, W);
        win[j] = elem_load_byte<kSrcU8>(sp, e) | (elem_load_byte<kSrcU8>(sp, plane + e) << 8) | (elem_load_byte<kSrcU8>(sp, 2u * plane + e) << 16);
      }
      __syncthreads();
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int mp = m[p];
        if (mp == 0) continue;
        uint32_t S0 = 0u, S1 = 0u, S2 = 0u;
#pragma unroll 1
        for (int k = -mp; k <= mp; ++k) {
          const int Qx = mblur_coord(X0 + p, k, sx[p], W), Qy = mblur_coord(Y, k, sy[p], H);
          const int fx = Qx & 255, fy = Qy & 255;
          // (0 <= column <= 95, 0 <= row <= 47: the tap is within the halo of its pixel, and a clamp only moves it towards the tile)
          const uint32_t* const q = win + ((Qy >> 8) - wy0) * kMblurWinW + ((Qx >> 8) - wx0);
          const uint32_t w00 = q[0], w10 = q[1], w01 = q[kMblurWinW], w11 = q[kMblurWinW + 1];
          const uint32_t wk = mblur_weight(k, mp);
          S0 += wk * mblur_tap(w00 & 255u, w10 & 255u, w01 & 255u, w11 & 255u, fx, fy);
          S1 += wk * mblur_tap((w00 >> 8) & 255u, (w10 >> 8) & 255u, (w01 >> 8) & 255u, (w11 >> 8) & 255u, fx, fy);
          S2 += wk * mblur_tap(w00 >> 16, w10 >> 16, w01 >> 16, w11 >> 16, fx, fy);
        }
        out[0][p] = mblur_byte(S0); out[1][p] = mblur_byte(S1); out[2][p] = mblur_byte(S2);
      }
      __syncthreads();  // (the next sample of this workgroup stages the window again)
    } else if (path != 0u) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int mp = m[p];
        if (mp == 0) continue;
        uint32_t S0 = 0u, S1 = 0u, S2 = 0u;
#pragma unroll 1
        for (int k = -mp; k <= mp; ++k) {
          const int Qx = mblur_coord(X0 + p, k, sx[p], W), Qy = mblur_coord(Y, k, sy[p], H);
          const int fx = Qx & 255, fy = Qy & 255;
          const uint32_t xa = (uint32_t)spatial_clamp(Qx >> 8, W), xb = (uint32_t)spatial_clamp((Qx >> 8) + 1, W);
          const uint32_t ya = (uint32_t)spatial_clamp(Qy >> 8, H) * (uint32_t)W, yb = (uint32_t)spatial_clamp((Qy >> 8) + 1, H) * (uint32_t)W;
          const uint32_t wk = mblur_weight(k, mp);
          S0 += wk * mblur_tap(elem_load_byte<kSrcU8>(sp, ya + xa), elem_load_byte<kSrcU8>(sp, ya + xb), elem_load_byte<kSrcU8>(sp, yb + xa),
                               elem_load_byte<kSrcU8>(sp, yb + xb), fx, fy);
          S1 += wk * mblur_tap(elem_load_byte<kSrcU8>(sp, plane + ya + xa), elem_load_byte<kSrcU8>(sp, plane + ya + xb),
                               elem_load_byte<kSrcU8>(sp, plane + yb + xa), elem_load_byte<kSrcU8>(sp, plane + yb + xb), fx, fy);
          S2 += wk * mblur_tap(elem_load_byte<kSrcU8>(sp, 2u * plane + ya + xa), elem_load_byte<kSrcU8>(sp, 2u * plane + ya + xb),
                               elem_load_byte<kSrcU8>(sp, 2u * plane + yb + xa), elem_load_byte<kSrcU8>(sp, 2u * plane + yb + xb), fx, fy);
        }
        out[0][p] = mblur_byte(S0); out[1][p] = mblur_byte(S1); out[2][p] = mblur_byte(S2);
      }
    }
    // (the lanes of a pair are inside together: X0 of the even one is a multiple of 8)
    uint8_t* const dp = d_img + (size_t)i * 3 * plane * kDES;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (kDstU8) quad_store_bytes_pair(dp + (uint32_t)c * plane + at, quad_word(out[c]), inside);
      else quad_store_bytes_f32(dp + ((size_t)c * plane + at) * 4u, out[c], inside);
    }
  }
}

// ---- Reprojection (ofdg_reproject, include/ofdg.h) -------------------------------------------------------------------------
// One launch for both frames and every sample: blockIdx.x counts the kReprojTileW x kReprojTileH tiles of a frame, blockIdx.y
// the samples, blockIdx.z the frames that are flagged.  A 4-wave workgroup owns a tile, a lane four consecutive pixels of one
// row (width % 8 == 0: a lane's four pixels, and the eight of a pair of lanes, are whole or outside together), so the own
// frame, the flow and the map are read as whole 16 / 8 / 4-byte pieces.  The other frame and the backward flow are gathered
// from global memory at clamped indices (ubyte / ushort / dword loads), the coordinates of a target computed once for the
// three channels and the two components: no index leaves a plane.  (A floating LDS window over the box of a tile's targets
// lost to this gather by 1.2 to 1.6 times - one tap per pixel amortises no staging:
// tools/patches/reproject_kernel_floating_window.patch, CHANGELOG.)  Stores are whole pieces, non-temporal: 16 bytes of
// float32 a lane, 8 bytes of uint8 a pair of lanes, gathered by the even lane with a wave shuffle.  The presence of each
// output, the destination format and the map's format are uniform run-time branches; the source format and the flow format
// are template arguments (4 instantiations).
// Rows: a lane sums its four pixels in registers (the six counts packed three to a word of 10-bit fields, the two error
// sums two to a word: a wave holds 256 pixels), the wave reduces them with __shfl_xor and counts the histogram with ballots,
// lane 0 (lanes 0..15 for the bins) writes the wave's slots in LDS - a row of slots per parity of the sample's turn, so one
// barrier a sample suffices - and the workgroup issues one integer atomic per non-zero word of the (sample, frame) block:
// atomicAdd on u32 / u64, atomicMax on u32 / u64.  No float atomics, so no bit depends on the order of arrival.  A launch
// without rows runs none of this and no barrier.  The functions of the definition are the host twin's (csrc/ofdg_device.h).
// No scratch.
constexpr int kReprojThreads = 256;
constexpr int kReprojTileW = 64, kReprojTileH = 16;
constexpr int kReprojWords = 23;  // the 32-bit words of a frame's block ahead of `reserved`
static_assert(kReprojTileW / 4 * kReprojTileH == kReprojThreads, "a lane per four pixels of the tile");
static_assert(offsetof(DevReprojFrameRow, reserved) == 4 * kReprojWords && offsetof(DevReprojFrameRow, sum_err) == 96, "the words and the 64-bit sums the kernel adds to");
template <bool kSrcU8, bool kFlowHalf>
__global__ __launch_bounds__(kReprojThreads) void reproject_kernel(const DevReprojJob job, int n, int W, int H, uint32_t tiles_x) {
  constexpr int kSES = kSrcU8 ? 1 : 4, kFES = kFlowHalf ? 2 : 4;
  __shared__ uint32_t s_words[2][kReprojThreads / 64][kReprojWords];  // [parity of the sample's turn][wave]
  __shared__ unsigned long long s_sums[2][kReprojThreads / 64][4];    // sum_err visible, hidden, sum_fb2_visible, max_fb2_visible
  const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int X0 = (int)(tx * kReprojTileW + (threadIdx.x & 15u) * 4u), Y = (int)(ty * kReprojTileH + (threadIdx.x >> 4));
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int f = (blockIdx.z != 0u || !(job.flags & OFDG_REPROJ_FRAME0)) ? 1 : 0;
  const uint8_t* const s_own = static_cast<const uint8_t*>(f ? job.img[1] : job.img[0]);
  const uint8_t* const s_other = static_cast<const uint8_t*>(f ? job.img[0] : job.img[1]);
  const uint8_t* const s_flow = static_cast<const uint8_t*>(f ? job.flow[1] : job.flow[0]);
  const uint8_t* const s_back = static_cast<const uint8_t*>(f ? job.flow[0] : job.flow[1]);
  const uint8_t* const s_occ = static_cast<const uint8_t*>(f ? job.occ[1] : job.occ[0]);
  uint8_t* const d_warped = static_cast<uint8_t*>(f ? job.warped[1] : job.warped[0]);
  uint8_t* const d_err = static_cast<uint8_t*>(f ? job.err[1] : job.err[0]);
  uint8_t* const d_mask = static_cast<uint8_t*>(f ? job.mask[1] : job.mask[0]);
  float* const d_fb2 = static_cast<float*>(f ? job.fb2[1] : job.fb2[0]);
  // what the launch has to compute: the taps of the other frame for warped, err and the rows' residuals, the backward taps
  // for fb2 and the rows' counts (uniform)
  const bool with_err = s_own && s_other && (d_err || job.rows), with_other = s_other && (d_warped || with_err);
  const bool with_fb = s_back && (d_fb2 || job.rows);
  const bool dst_u8 = job.dst_fmt == OFDG_FMT_U8, occ_u8 = job.occ_fmt == OFDG_FMT_U8;
  const long long thr2 = (long long)job.fb_thresh_q8 * job.fb_thresh_q8;
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (3 * plane < 2^32: reproj_arg_error)
  const bool act = X0 < W && Y < H;
  const uint32_t at = act ? (uint32_t)Y * (uint32_t)W + (uint32_t)X0 : 0u;  // the lane's first pixel in a channel
  uint32_t turn = 0u;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y, turn ^= 1u) {
    const uint8_t* const op = s_other + (size_t)i * 3 * plane * kSES;
    const uint8_t* const bp = s_back + (size_t)i * 2 * plane * kFES;
    float u[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t own[3][4] = {};
    uint32_t hidden = 0u;  // bit p: the map says pixel p is hidden
    if (act) {
      const uint8_t* const fp = s_flow + ((size_t)i * 2 * plane + at) * kFES;
      quad_load<quad_fmt(kFlowHalf)>(fp, u);
      quad_load<quad_fmt(kFlowHalf)>(fp + (size_t)plane * kFES, v);
      if (with_err) {
        const uint8_t* const sp = s_own + (size_t)i * 3 * plane * kSES;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if constexpr (kSrcU8) quad_load_bytes<true>(sp + (uint32_t)c * plane + at, own[c]);
          else quad_load_bytes<false>(sp + ((size_t)c * plane + at) * 4u, own[c]);
        }
      }
      if (s_occ) {
        if (occ_u8) hidden = quad_load_hidden<true>(s_occ + (size_t)i * plane + at);
        else hidden = quad_load_hidden<false>(s_occ + ((size_t)i * plane + at) * 4u);
      }
    }
    uint32_t out[3][4] = {};
    uint32_t errs = 0u, masks = 0u;  // a byte per pixel
    float fb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    // the lane's part of the row
    uint32_t cnt_a = 0u, cnt_b = 0u;  // 10-bit fields: bad, outside, visible | hidden, over visible, over hidden
    uint32_t sum_err = 0u, max_err = 0u;  // 16-bit fields: visible, hidden
    int bin[4] = {kReprojErrBins, kReprojErrBins, kReprojErrBins, kReprojErrBins};
    unsigned long long sum_fb2 = 0ull, max_fb2 = 0ull;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool bad = !(flow_finite(u[p]) && flow_finite(v[p]));
      const int Dx = bad ? 0 : reproj_q8(u[p]), Dy = bad ? 0 : reproj_q8(v[p]);
      const int Qx0 = 256 * (X0 + p) + Dx, Qy0 = 256 * Y + Dy;
      const bool in = act && !bad && reproj_inside(Qx0, Qy0, W, H);
      uint32_t err = 0u;
      long long e2 = 0;
      if (in) {
        const int Qx = reproj_coord(Qx0, W), Qy = reproj_coord(Qy0, H);
        const int fx = Qx & 255, fy = Qy & 255;
        const uint32_t xa = (uint32_t)spatial_clamp(Qx >> 8, W), xb = (uint32_t)spatial_clamp((Qx >> 8) + 1, W);
        const uint32_t ya = (uint32_t)spatial_clamp(Qy >> 8, H) * (uint32_t)W, yb = (uint32_t)spatial_clamp((Qy >> 8) + 1, H) * (uint32_t)W;
        masks |= 1u << (8 * p);
        if (with_other) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const uint32_t o = (uint32_t)c * plane;
            const uint32_t w = reproj_byte(mblur_tap(elem_load_byte<kSrcU8>(op, o + ya + xa), elem_load_byte<kSrcU8>(op, o + ya + xb),
                                                     elem_load_byte<kSrcU8>(op, o + yb + xa), elem_load_byte<kSrcU8>(op, o + yb + xb), fx, fy));
            out[c][p] = w;
            const uint32_t d = w > own[c][p] ? w - own[c][p] : own[c][p] - w;
            err = d > err ? d : err;
          }
          err = with_err ? err : 0u;
          errs |= err << (8 * p);
        }
        if (with_fb) {
          const float b0 = elem_load<quad_fmt(kFlowHalf)>(bp, ya + xa), b1 = elem_load<quad_fmt(kFlowHalf)>(bp, ya + xb);
          const float b2 = elem_load<quad_fmt(kFlowHalf)>(bp, yb + xa), b3 = elem_load<quad_fmt(kFlowHalf)>(bp, yb + xb);
          const float c0 = elem_load<quad_fmt(kFlowHalf)>(bp, plane + ya + xa), c1 = elem_load<quad_fmt(kFlowHalf)>(bp, plane + ya + xb);
          const float c2 = elem_load<quad_fmt(kFlowHalf)>(bp, plane + yb + xa), c3 = elem_load<quad_fmt(kFlowHalf)>(bp, plane + yb + xb);
          const bool finite = flow_finite(b0) && flow_finite(b1) && flow_finite(b2) && flow_finite(b3) && flow_finite(c0) && flow_finite(c1) &&
                              flow_finite(c2) && flow_finite(c3);
          if (finite) {
            e2 = reproj_e2(Dx, Dy, reproj_back(b0, b1, b2, b3, fx, fy), reproj_back(c0, c1, c2, c3, fx, fy));
            fb[p] = reproj_fb2(e2);
          } else {
            e2 = kReprojE2Sat;
            fb[p] = __uint_as_float(0x7f800000u);
          }
        }
      }
      if (job.rows) {  // (uniform)
        const bool hid = (hidden >> p) & 1u;
        const bool vis = in && !hid;
        const bool over = in && with_fb && e2 > thr2;
        cnt_a += (act && bad ? 1u : 0u) | ((act && !bad && !in ? 1u : 0u) << 10) | ((vis ? 1u : 0u) << 20);
        cnt_b += (in && hid ? 1u : 0u) | ((over && !hid ? 1u : 0u) << 10) | ((over && hid ? 1u : 0u) << 20);
        if (with_err) {
          sum_err += in ? (hid ? err << 16 : err) : 0u;
          max_err = vis && err > max_err ? err : max_err;
          bin[p] = vis ? (int)(err >> 4) : kReprojErrBins;
        }
        if (with_fb && vis) {
          sum_fb2 += (unsigned long long)(e2 < 4294967295ll ? e2 : 4294967295ll);
          max_fb2 = (unsigned long long)e2 > max_fb2 ? (unsigned long long)e2 : max_fb2;
        }
      }
    }
    // (the lanes of a pair are inside together: X0 of the even one is a multiple of 8)
    if (d_warped) {
      if (dst_u8) {
        uint8_t* const dp = d_warped + (size_t)i * 3 * plane;
#pragma unroll
        for (int c = 0; c < 3; ++c) quad_store_bytes_pair(dp + (uint32_t)c * plane + at, quad_word(out[c]), act);
      } else {
        uint8_t* const dp = d_warped + (size_t)i * 3 * plane * 4u;
#pragma unroll
        for (int c = 0; c < 3; ++c) quad_store_bytes_f32(dp + ((size_t)c * plane + at) * 4u, out[c], act);
      }
    }
    if (d_err) quad_store_bytes_pair(d_err + (size_t)i * plane + at, errs, act);
    if (d_mask) quad_store_bytes_pair(d_mask + (size_t)i * plane + at, masks, act);
    if (d_fb2) {
      const f32x4 o = {fb[0], fb[1], fb[2], fb[3]};
      if (act) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(d_fb2 + (size_t)i * plane + at));
    }
    if (job.rows) {  // (uniform: every lane of the workgroup is here)
      uint32_t hist = 0u;  // lane b: the wave's count of bin b
      if (with_err) {
#pragma unroll
        for (int b = 0; b < kReprojErrBins; ++b) {
          const uint32_t k = (uint32_t)(__popcll(__ballot(bin[0] == b)) + __popcll(__ballot(bin[1] == b)) + __popcll(__ballot(bin[2] == b)) + __popcll(__ballot(bin[3] == b)));
          hist = lane == b ? k : hist;
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        cnt_a += (uint32_t)__shfl_xor((int)cnt_a, d, 64);
        cnt_b += (uint32_t)__shfl_xor((int)cnt_b, d, 64);
        sum_err += (uint32_t)__shfl_xor((int)sum_err, d, 64);
        const uint32_t me = (uint32_t)__shfl_xor((int)max_err, d, 64);
        max_err = me > max_err ? me : max_err;
        sum_fb2 += (unsigned long long)__shfl_xor((long long)sum_fb2, d, 64);
        const unsigned long long mf = (unsigned long long)__shfl_xor((long long)max_fb2, d, 64);
        max_fb2 = mf > max_fb2 ? mf : max_fb2;
      }
      uint32_t* const sw = s_words[turn][wave];
      if (lane < kReprojErrBins) sw[4 + lane] = hist;
      if (lane == 0) {
        sw[0] = cnt_a & 1023u; sw[1] = (cnt_a >> 10) & 1023u; sw[2] = cnt_a >> 20; sw[3] = cnt_b & 1023u;
        sw[20] = max_err; sw[21] = (cnt_b >> 10) & 1023u; sw[22] = cnt_b >> 20;
        s_sums[turn][wave][0] = sum_err & 65535u; s_sums[turn][wave][1] = sum_err >> 16;
        s_sums[turn][wave][2] = sum_fb2; s_sums[turn][wave][3] = max_fb2;
      }
      __syncthreads();  // (a wave is at most one barrier ahead of another, and the next sample's slots are the other row's)
      DevReprojFrameRow* const fr = &job.rows[i].frame[f];
      if (threadIdx.x < (uint32_t)kReprojWords) {
        const uint32_t t = threadIdx.x, a = s_words[turn][0][t], b = s_words[turn][1][t], c = s_words[turn][2][t], d = s_words[turn][3][t];
        uint32_t* const word = reinterpret_cast<uint32_t*>(fr) + t;
        if (t == 20u) {
          const uint32_t m = max(max(a, b), max(c, d));
          if (m) atomicMax(word, m);
        } else {
          const uint32_t s = a + b + c + d;
          if (s) atomicAdd(word, s);
        }
      } else if (threadIdx.x >= 64u && threadIdx.x < 68u) {
        const uint32_t t = threadIdx.x - 64u;
        const unsigned long long a = s_sums[turn][0][t], b = s_sums[turn][1][t], c = s_sums[turn][2][t], d = s_sums[turn][3][t];
        unsigned long long* const word = reinterpret_cast<unsigned long long*>(fr) + 12 + t;
        if (t == 3u) {
          const unsigned long long m = max(max(a, b), max(c, d));
          if (m) atomicMax(word, m);
        } else {
          const unsigned long long s = a + b + c + d;
          if (s) atomicAdd(word, s);
        }
      }
    }
  }
}

// ---- Splat (ofdg_splat, include/ofdg.h) ------------------------------------------------------------------------------------
// Two launches behind the clears, each for both frames and every sample, on reproject_kernel's layout: blockIdx.x counts
// the kSplatTileW x kSplatTileH tiles of a frame, blockIdx.y the samples, blockIdx.z the frames that are flagged; a 4-wave
// workgroup owns a tile, a lane four consecutive pixels of one row (width % 8 == 0: a lane's four pixels, and the eight of a
// pair of lanes, are whole or outside together), so the flow, the label, the maps and the keys are read as whole 16 / 8 / 4-byte
// pieces and every plane is written as whole pieces.
// splat_scatter_kernel: a lane's pixels as SOURCES.  Targets of a tile mostly land near it: an LDS key window - the tile and
// a halo of 16 pixels, 96 x 48 cells, 18 432 bytes - takes the maxima of the targets inside it on chip (ds_max_u32), and behind
// a barrier the workgroup flushes it, a thread 18 cells, with one relaxed agent-scope atomic max without a return value per
// touched cell: a wave's flush is 256 contiguous bytes of a row, where the per-pixel form issued four atomics a lane 16 bytes
// apart.  A target outside the window goes straight to global memory with the same atomic.  Every target is tested against
// the plane first, and a flushed cell again, so no index leaves it.  (The form without the window - one global atomic per
// inside pixel - passed the same tests and took 1.3 to 2.4 times as long: tools/patches/splat_scatter_atomics_only.patch,
// CHANGELOG.)  Thread 0 of the first tile writes the sanitised record and the row's t_q8.
// splat_resolve_kernel: a lane's pixels in both roles.  As TARGETS it decodes the four keys, gathers the winner's bytes and
// flow (ubyte / ushort / dword loads at an index below the plane's size: the keys were cleared and raised by this call only,
// and an index is tested all the same) and stores image, to_own, to_other and mask; as SOURCES it aims again, reads the key
// at the target and stores the fate.  Stores are non-temporal: 16 bytes of float32 a lane, 8 bytes of binary16 a lane, 8
// bytes of uint8 a pair of lanes, gathered by the even lane with a wave shuffle.
// Rows: a lane counts its four pixels in 10-bit fields three to a word (a wave holds 256 pixels), the wave reduces them
// with __shfl_xor, lane 0 writes the wave's slots in LDS - a row of slots per parity of the sample's turn, so one barrier a
// sample suffices - and the workgroup issues one atomicAdd per non-zero count.  Integer atomics only: no bit depends on the
// order of arrival.  A launch without rows runs none of this and no barrier.  The presence of each output, the destination
// formats and the maps' format are uniform run-time branches; the flow format (both kernels) and the source format
// (resolve) are template arguments: 2 + 4 instantiations.  The functions of the definition are the host twin's
// (csrc/ofdg_device.h).  No scratch.
constexpr int kSplatThreads = 256;
constexpr int kSplatTileW = 64, kSplatTileH = 16;
constexpr int kSplatResolveWords = 7;  // n_filled .. n_hole_other_hidden: the words the resolve adds to
static_assert(kSplatTileW / 4 * kSplatTileH == kSplatThreads, "a lane per four pixels of the tile");
static_assert(offsetof(DevSplatFrameRow, dst) == 12 && offsetof(DevSplatFrameRow, t_q8) == 12 + 4 * kSplatResolveWords, "the words the two kernels add to");
__device__ __forceinline__ DevSplatRec splat_rec_of(const DevSplatJob& job, int i) {
  DevSplatRec r;
  if (job.recs) r = job.recs[i];
  else r = splat_draw_rec(job.seed, (unsigned long long)(job.first_index + i), job);
  return splat_sanitise(r);
}
template <bool kFlowHalf>
__global__ __launch_bounds__(kSplatThreads) void splat_scatter_kernel(const DevSplatJob job, int n, int W, int H, uint32_t tiles_x) {
  constexpr int kFES = kFlowHalf ? 2 : 4;
  __shared__ uint32_t s_cnt[2][kSplatThreads / 64];  // [parity of the sample's turn][wave]: bad, outside, inside in 10-bit fields
  // the LDS key window: the tile and a halo of kSplatHalo pixels; the maxima of the targets that land in it are taken on chip
  // and flushed with one global atomic per touched cell, the others go straight to global memory
  constexpr int kSplatHalo = 16, kWinW = kSplatTileW + 2 * kSplatHalo, kWinH = kSplatTileH + 2 * kSplatHalo, kWinCells = kWinW * kWinH;
  static_assert(kWinCells % kSplatThreads == 0, "a thread clears and flushes a whole number of cells");
  __shared__ uint32_t s_win[kWinCells];
  const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int X0 = (int)(tx * kSplatTileW + (threadIdx.x & 15u) * 4u), Y = (int)(ty * kSplatTileH + (threadIdx.x >> 4));
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int f = (blockIdx.z != 0u || !(job.flags & OFDG_SPLAT_FRAME0)) ? 1 : 0;
  const uint8_t* const s_flow = static_cast<const uint8_t*>(f ? job.flow[1] : job.flow[0]);
  const uint8_t* const s_label = f ? job.label[1] : job.label[0];
  uint32_t* const d_keys = f ? job.keys[1] : job.keys[0];
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (below 2^24: splat_arg_error)
  const bool act = X0 < W && Y < H;
  const uint32_t at = act ? (uint32_t)Y * (uint32_t)W + (uint32_t)X0 : 0u;  // the lane's first pixel in a plane
  const int wx0 = (int)(tx * kSplatTileW) - kSplatHalo, wy0 = (int)(ty * kSplatTileH) - kSplatHalo;  // the window's first column and row in the frame
  uint32_t turn = 0u;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y, turn ^= 1u) {
    const DevSplatRec r = splat_rec_of(job, i);
    const int T = f ? r.t_q8[1] : r.t_q8[0];
#pragma unroll
    for (int k = 0; k < kWinCells / kSplatThreads; ++k) s_win[(uint32_t)k * kSplatThreads + threadIdx.x] = 0u;
    __syncthreads();
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
      if (job.recs_out && blockIdx.z == 0u) *reinterpret_cast<u32x4*>(job.recs_out + i) = u32x4{(uint32_t)r.t_q8[0], (uint32_t)r.t_q8[1], 0u, 0u};
      if (job.rows) job.rows[i].frame[f].t_q8 = (uint32_t)T;
    }
    float u[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t labels = 0u;  // a byte per pixel
    if (act) {
      const uint8_t* const fp = s_flow + ((size_t)i * 2 * plane + at) * kFES;
      quad_load<quad_fmt(kFlowHalf)>(fp, u);
      quad_load<quad_fmt(kFlowHalf)>(fp + (size_t)plane * kFES, v);
      if (s_label) labels = *reinterpret_cast<const uint32_t*>(s_label + (size_t)i * plane + at);
    }
    uint32_t* const kp = d_keys + (size_t)i * plane;
    uint32_t cnt = 0u;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool bad = !(flow_finite(u[p]) && flow_finite(v[p]));
      const int rx = splat_round(X0 + p, splat_scale(bad ? 0 : reproj_q8(u[p]), T)), ry = splat_round(Y, splat_scale(bad ? 0 : reproj_q8(v[p]), T));
      const bool in = act && !bad && splat_inside(rx, ry, W, H);
      if (in) {
        const uint32_t key = splat_key((labels >> (8 * p)) & 255u, at + (uint32_t)p);
        const int cx = rx - wx0, cy = ry - wy0;
        if (cx >= 0 && cx < kWinW && cy >= 0 && cy < kWinH) atomicMax(&s_win[cy * kWinW + cx], key);
        else __hip_atomic_fetch_max(kp + ((uint32_t)ry * (uint32_t)W + (uint32_t)rx), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      cnt += (act && bad ? 1u : 0u) | ((act && !bad && !in ? 1u : 0u) << 10) | ((in ? 1u : 0u) << 20);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kWinCells / kSplatThreads; ++k) {
      const uint32_t c = (uint32_t)k * kSplatThreads + threadIdx.x, key = s_win[c];
      const int gx = wx0 + (int)(c % (uint32_t)kWinW), gy = wy0 + (int)(c / (uint32_t)kWinW);
      if (key != 0u && splat_inside(gx, gy, W, H)) __hip_atomic_fetch_max(kp + ((uint32_t)gy * (uint32_t)W + (uint32_t)gx), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();  // (the window is cleared again for the next sample only behind its flush)
    if (job.rows) {  // (uniform: every lane of the workgroup is here)
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, d, 64);
      if (lane == 0) s_cnt[turn][wave] = cnt;
      __syncthreads();  // (a wave is at most one barrier ahead of another, and the next sample's slots are the other row's)
      if (threadIdx.x < 3u) {
        const uint32_t sh = 10u * threadIdx.x;
        const uint32_t s = ((s_cnt[turn][0] >> sh) & 1023u) + ((s_cnt[turn][1] >> sh) & 1023u) + ((s_cnt[turn][2] >> sh) & 1023u) + ((s_cnt[turn][3] >> sh) & 1023u);
        if (s) atomicAdd(&job.rows[i].frame[f].src[threadIdx.x], s);
      }
    }
  }
}
template <bool kSrcU8, bool kFlowHalf>
__global__ __launch_bounds__(kSplatThreads) void splat_resolve_kernel(const DevSplatJob job, int n, int W, int H, uint32_t tiles_x) {
  constexpr int kSES = kSrcU8 ? 1 : 4, kFES = kFlowHalf ? 2 : 4;
  __shared__ uint32_t s_cnt[2][kSplatThreads / 64][3];  // [parity of the sample's turn][wave]: the seven counts in 10-bit fields
  const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int X0 = (int)(tx * kSplatTileW + (threadIdx.x & 15u) * 4u), Y = (int)(ty * kSplatTileH + (threadIdx.x >> 4));
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int f = (blockIdx.z != 0u || !(job.flags & OFDG_SPLAT_FRAME0)) ? 1 : 0;
  const uint8_t* const s_img = static_cast<const uint8_t*>(f ? job.img[1] : job.img[0]);
  const uint8_t* const s_flow = static_cast<const uint8_t*>(f ? job.flow[1] : job.flow[0]);
  const uint8_t* const s_label = f ? job.label[1] : job.label[0];
  const uint8_t* const s_occ = static_cast<const uint8_t*>(f ? job.occ[1] : job.occ[0]);
  const uint8_t* const s_occ_other = static_cast<const uint8_t*>(f ? job.occ[0] : job.occ[1]);
  const uint32_t* const s_keys = f ? job.keys[1] : job.keys[0];
  uint8_t* const d_image = static_cast<uint8_t*>(f ? job.image[1] : job.image[0]);
  uint8_t* const d_own = static_cast<uint8_t*>(f ? job.to_own[1] : job.to_own[0]);
  uint8_t* const d_other = static_cast<uint8_t*>(f ? job.to_other[1] : job.to_other[0]);
  uint8_t* const d_mask = static_cast<uint8_t*>(f ? job.mask[1] : job.mask[0]);
  uint8_t* const d_fate = static_cast<uint8_t*>(f ? job.fate[1] : job.fate[0]);
  // what the launch has to do (uniform)
  const bool as_target = d_image || d_own || d_other || d_mask || job.rows, as_source = d_fate || job.rows;
  const bool dst_u8 = job.dst_fmt == OFDG_FMT_U8, occ_u8 = job.occ_fmt == OFDG_FMT_U8, oflow_half = job.oflow_fmt == OFDG_FMT_F16;
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (below 2^24: splat_arg_error)
  const bool act = X0 < W && Y < H;
  const uint32_t at = act ? (uint32_t)Y * (uint32_t)W + (uint32_t)X0 : 0u;  // the lane's first pixel in a plane
  uint32_t turn = 0u;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y, turn ^= 1u) {
    const uint32_t* const kp = s_keys + (size_t)i * plane;
    const uint8_t* const fp = s_flow + (size_t)i * 2 * plane * kFES;
    uint32_t cnt_a = 0u, cnt_b = 0u, cnt_c = 0u;  // filled, holes, covered | covered visible, covered hidden, hole other visible | hole other hidden
    if (as_target) {
      u32x4 K = {0u, 0u, 0u, 0u};
      uint32_t hidden = 0u;  // bit p: the other frame's map says pixel p is hidden
      if (act) {
        K = *reinterpret_cast<const u32x4*>(kp + at);
        if (s_occ_other && job.rows) {
          if (occ_u8) hidden = quad_load_hidden<true>(s_occ_other + (size_t)i * plane + at);
          else hidden = quad_load_hidden<false>(s_occ_other + ((size_t)i * plane + at) * 4u);
        }
      }
      uint32_t out[3][4] = {};
      uint32_t masks = 0u;  // a byte per pixel
      float own[2][4] = {}, other[2][4] = {};
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const uint32_t s = splat_source(K[p]);
        const bool filled = K[p] != 0u && s < plane;
        if (filled) {
          const uint32_t y = s / (uint32_t)W, x = s - y * (uint32_t)W;
          const int dx = (int)x - (X0 + p), dy = (int)y - Y;
          masks |= 1u << (8 * p);
          own[0][p] = (float)dx; own[1][p] = (float)dy;
          if (d_other) {
            other[0][p] = splat_to_other(dx, reproj_q8(elem_load<quad_fmt(kFlowHalf)>(fp, s)));
            other[1][p] = splat_to_other(dy, reproj_q8(elem_load<quad_fmt(kFlowHalf)>(fp, plane + s)));
          }
          if (d_image) {
            const uint8_t* const sp = s_img + (size_t)i * 3 * plane * kSES;
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c][p] = elem_load_byte<kSrcU8>(sp, (uint32_t)c * plane + s);
          }
        }
        const bool hole = act && !filled, hid = (hidden >> p) & 1u;
        cnt_a += (filled ? 1u : 0u) | ((hole ? 1u : 0u) << 10);
        cnt_b += (hole && s_occ_other && !hid ? 1u : 0u) << 20;
        cnt_c += hole && s_occ_other && hid ? 1u : 0u;
      }
      // (the lanes of a pair are inside together: X0 of the even one is a multiple of 8)
      if (d_image) {
        if (dst_u8) {
          uint8_t* const dp = d_image + (size_t)i * 3 * plane;
#pragma unroll
          for (int c = 0; c < 3; ++c) quad_store_bytes_pair(dp + (uint32_t)c * plane + at, quad_word(out[c]), act);
        } else {
          uint8_t* const dp = d_image + (size_t)i * 3 * plane * 4u;
#pragma unroll
          for (int c = 0; c < 3; ++c) quad_store_bytes_f32(dp + ((size_t)c * plane + at) * 4u, out[c], act);
        }
      }
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        uint8_t* const dq = which ? d_other : d_own;
        if (!dq || !act) continue;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float* const e = which ? other[c] : own[c];
          const size_t o = (size_t)i * 2 * plane + (size_t)c * plane + at;
          if (oflow_half) __builtin_nontemporal_store(f16x4{(_Float16)e[0], (_Float16)e[1], (_Float16)e[2], (_Float16)e[3]}, reinterpret_cast<f16x4*>(dq + o * 2u));
          else __builtin_nontemporal_store(f32x4{e[0], e[1], e[2], e[3]}, reinterpret_cast<f32x4*>(dq + o * 4u));
        }
      }
      if (d_mask) quad_store_bytes_pair(d_mask + (size_t)i * plane + at, masks, act);
    }
    if (as_source) {
      const DevSplatRec r = splat_rec_of(job, i);
      const int T = f ? r.t_q8[1] : r.t_q8[0];
      float u[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      uint32_t labels = 0u, hidden = 0u;
      if (act) {
        quad_load<quad_fmt(kFlowHalf)>(fp + (size_t)at * kFES, u);
        quad_load<quad_fmt(kFlowHalf)>(fp + ((size_t)plane + at) * kFES, v);
        if (s_label) labels = *reinterpret_cast<const uint32_t*>(s_label + (size_t)i * plane + at);
        if (s_occ && job.rows) {
          if (occ_u8) hidden = quad_load_hidden<true>(s_occ + (size_t)i * plane + at);
          else hidden = quad_load_hidden<false>(s_occ + ((size_t)i * plane + at) * 4u);
        }
      }
      uint32_t fates = 0u;  // a byte per pixel
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const bool bad = !(flow_finite(u[p]) && flow_finite(v[p]));
        const int rx = splat_round(X0 + p, splat_scale(bad ? 0 : reproj_q8(u[p]), T)), ry = splat_round(Y, splat_scale(bad ? 0 : reproj_q8(v[p]), T));
        const bool in = act && !bad && splat_inside(rx, ry, W, H);
        bool covered = false;
        if (in) covered = kp[(uint32_t)ry * (uint32_t)W + (uint32_t)rx] != splat_key((labels >> (8 * p)) & 255u, at + (uint32_t)p);
        fates |= (bad ? 3u : !in ? 2u : covered ? 1u : 0u) << (8 * p);
        const bool hid = (hidden >> p) & 1u;
        cnt_a += (covered ? 1u : 0u) << 20;
        cnt_b += (covered && s_occ && !hid ? 1u : 0u) | ((covered && s_occ && hid ? 1u : 0u) << 10);
      }
      if (d_fate) quad_store_bytes_pair(d_fate + (size_t)i * plane + at, fates, act);
    }
    if (job.rows) {  // (uniform: every lane of the workgroup is here)
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        cnt_a += (uint32_t)__shfl_xor((int)cnt_a, d, 64);
        cnt_b += (uint32_t)__shfl_xor((int)cnt_b, d, 64);
        cnt_c += (uint32_t)__shfl_xor((int)cnt_c, d, 64);
      }
      if (lane == 0) { s_cnt[turn][wave][0] = cnt_a; s_cnt[turn][wave][1] = cnt_b; s_cnt[turn][wave][2] = cnt_c; }
      __syncthreads();  // (a wave is at most one barrier ahead of another, and the next sample's slots are the other row's)
      if (threadIdx.x < (uint32_t)kSplatResolveWords) {
        const uint32_t w = threadIdx.x / 3u, sh = 10u * (threadIdx.x % 3u);
        const uint32_t s = ((s_cnt[turn][0][w] >> sh) & 1023u) + ((s_cnt[turn][1][w] >> sh) & 1023u) + ((s_cnt[turn][2][w] >> sh) & 1023u) + ((s_cnt[turn][3][w] >> sh) & 1023u);
        if (s) atomicAdd(reinterpret_cast<uint32_t*>(&job.rows[i].frame[f]) + 3u + threadIdx.x, s);
      }
    }
  }
}

// ---- Flow visualisation (ofdg_flow_vis, include/ofdg.h) --------------------------------------------------------------------
// Under OFDG_VIS_NORM_FIXED one launch, else two behind the clearing of `work`: flow_vis_max_kernel leaves the largest R2 of
// each sample (BATCH: of the call, in slot 0) in `work`, flow_vis_colour_kernel - which starts after the first has ended, the
// order of the stream - takes the scale from it and writes the picture.  blockIdx.x counts the kVisBlockPixels-pixel blocks
// of a plane, blockIdx.y the samples (strided beyond 65535 of them, as in the jitter: no test runs that many).  A lane takes 4
// consecutive pixels - 16 bytes of each float32 flow plane, 8 of a
// binary16 one, 16 or 4 of the map - in rounds of 1024 pixels per workgroup; H * W is a multiple of 16, so a plane is whole
// pieces and rows never split one.  The steps of the definition are the host twin's functions (csrc/ofdg_device.h), so the
// bytes are the twin's.  No scratch; the colour kernel holds the two tables in 1260 bytes of LDS.
constexpr int kVisThreads = 256;
constexpr int kVisBlockPixels = 4096;  // 48 workgroups per 512 x 384 plane, four rounds each
static_assert(kVisBlockPixels % (kVisThreads * 4) == 0, "whole rounds of 4-pixel pieces");
#ifndef OFDG_VIS_READ_FIRST
#define OFDG_VIS_READ_FIRST 1
#endif
constexpr int kVisReadFirst = OFDG_VIS_READ_FIRST;  // which slots of `work` the reduction reads before its atomic: 0 none, 1 BATCH's one slot, 2 every slot

// The maximum's reduction: a running 64-bit maximum of R2 per lane over the usable pixels, across the wave with __shfl_xor,
// across the workgroup through LDS, and at most one 64-bit integer atomicMax per workgroup (none where nothing is usable: the
// slot is cleared to 0 before the launch).  No bit depends on arrival order.
template <bool kHalf>
__global__ __launch_bounds__(kVisThreads) void flow_vis_max_kernel(const DevVisJob job, int n, uint32_t plane) {
  typedef typename FlowFmt<quad_fmt(kHalf)>::elem FlowElem;
  __shared__ unsigned long long s_part[kVisThreads / 64];
  const uint32_t first = blockIdx.x * (uint32_t)kVisBlockPixels;
  const uint32_t end = first + (uint32_t)kVisBlockPixels < plane ? first + (uint32_t)kVisBlockPixels : plane;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    const size_t base = (size_t)i * 2 * plane;
    unsigned long long best = 0;
    for (uint32_t at = first + threadIdx.x * 4u; at < end; at += (uint32_t)(kVisThreads * 4)) {
      float u[4], v[4];
      quad_load<quad_fmt(kHalf)>(static_cast<const FlowElem*>(job.flow) + (base + at), u);
      quad_load<quad_fmt(kHalf)>(static_cast<const FlowElem*>(job.flow) + (base + plane + at), v);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned long long r2 = flow_usable(u[q], v[q]) ? vis_r2(vis_fixed(u[q]), vis_fixed(v[q])) : 0ull;
        best = r2 > best ? r2 : best;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long other = (unsigned long long)__shfl_xor((long long)best, d, 64);
      best = other > best ? other : best;
    }
    if (lane == 0) s_part[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long total = 0;
#pragma unroll
      for (int w = 0; w < kVisThreads / 64; ++w) total = s_part[w] > total ? s_part[w] : total;
      // BATCH: every workgroup of the call meets on slot 0, which only grows - one that reads a value no smaller than its own
      // has nothing to add (a stale, smaller reading costs an atomic that changes nothing), which spares the slot most of
      // the atomics.  A sample's own slot has 1 / n of them, and there the reading's round trip costs more than it saves
      // (the three forms measured: CHANGELOG; kVisReadFirst 0: no slot is read first, 2: every slot is).
      unsigned long long* const slot = job.work + (job.norm == OFDG_VIS_NORM_BATCH ? 0 : i);
      const bool read_first = kVisReadFirst == 2 || (kVisReadFirst == 1 && job.norm == OFDG_VIS_NORM_BATCH);
      if (read_first ? total > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : total != 0ull) atomicMax(slot, total);
    }
    __syncthreads();  // (the next sample of this workgroup writes the parts again)
  }
}

// The picture.  The grid is flow_vis_max_kernel's.  The tables are copied to LDS once per workgroup; the scale is read or
// rounded on wave-uniform values once per (workgroup, sample).  Planar: a lane stores one dword of each of the B, G and R
// planes, a wave 256 consecutive bytes per plane; HWC: a lane stores the 12 bytes of its 4 pixels as three dwords, a wave 768
// consecutive bytes.  Workgroup 0 of a sample writes its row from lane 0 with one 16-byte store.
template <bool kHalf, int kOcc, bool kHwc>  // kOcc: 0 no dimming, 1 by a float32 map, 2 by a uint8 one
__global__ __launch_bounds__(kVisThreads) void flow_vis_colour_kernel(const DevVisJob job, int n, uint32_t plane) {
  typedef typename FlowFmt<quad_fmt(kHalf)>::elem FlowElem;
  __shared__ int32_t s_atan[kVisAtanEntries];
  __shared__ uint32_t s_wheel[kVisWheelEntries];
  for (int k = (int)threadIdx.x; k < kVisAtanEntries; k += kVisThreads) s_atan[k] = kVisAtan[k];
  if (threadIdx.x < (uint32_t)kVisWheelEntries) s_wheel[threadIdx.x] = kVisWheel[threadIdx.x];
  __syncthreads();
  const uint32_t first = blockIdx.x * (uint32_t)kVisBlockPixels;
  const uint32_t end = first + (uint32_t)kVisBlockPixels < plane ? first + (uint32_t)kVisBlockPixels : plane;
  uint8_t* const dst = static_cast<uint8_t*>(job.dst);
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    unsigned long long max_r2 = 0;
    uint32_t M;
    if (job.norm == OFDG_VIS_NORM_FIXED) M = vis_scale_fixed(job.max_flow);
    else {
      max_r2 = job.work[job.norm == OFDG_VIS_NORM_BATCH ? 0 : i];
      M = vis_scale_of(max_r2);
    }
    M = (uint32_t)__builtin_amdgcn_readfirstlane((int)M);
    const float inv_m = vis_inv(M);
    if (job.rows_out && blockIdx.x == 0u && threadIdx.x == 0u)
      *reinterpret_cast<u32x4*>(job.rows_out + i) = u32x4{(uint32_t)max_r2, (uint32_t)(max_r2 >> 32), M, 0u};
    const size_t base = (size_t)i * 2 * plane;
    for (uint32_t at = first + threadIdx.x * 4u; at < end; at += (uint32_t)(kVisThreads * 4)) {
      float u[4], v[4];
      quad_load<quad_fmt(kHalf)>(static_cast<const FlowElem*>(job.flow) + (base + at), u);
      quad_load<quad_fmt(kHalf)>(static_cast<const FlowElem*>(job.flow) + (base + plane + at), v);
      uint32_t hidden = 0;  // bit q: pixel q is dimmed
      if constexpr (kOcc == 1) hidden = quad_load_hidden<false>(static_cast<const float*>(job.occ) + (size_t)i * plane + at);
      else if constexpr (kOcc == 2) hidden = quad_load_hidden<true>(static_cast<const uint8_t*>(job.occ) + (size_t)i * plane + at);
      uint32_t px[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) px[q] = flow_usable(u[q], v[q]) ? vis_pixel(u[q], v[q], M, inv_m, (hidden >> q) & 1u, s_atan, s_wheel) : 0u;
      if constexpr (kHwc) {
        uint32_t* const dp = reinterpret_cast<uint32_t*>(dst + ((size_t)i * plane + at) * 3);
        dp[0] = px[0] | (px[1] << 24);
        dp[1] = (px[1] >> 8) | (px[2] << 16);
        dp[2] = (px[2] >> 16) | (px[3] << 8);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {  // c: R, G, B of a pixel's word; plane 2 - c
          const uint32_t sh = 8u * (uint32_t)c;
          const uint32_t w = ((px[0] >> sh) & 255u) | (((px[1] >> sh) & 255u) << 8) | (((px[2] >> sh) & 255u) << 16) | (((px[3] >> sh) & 255u) << 24);
          *reinterpret_cast<uint32_t*>(dst + ((size_t)i * 3 + (size_t)(2 - c)) * plane + at) = w;
        }
      }
    }
  }
}

// ---- Flow error (ofdg_flow_error, include/ofdg.h) --------------------------------------------------------------------------
// One launch behind the optional clearing of the rows.  The grid is the colour-wheel's: blockIdx.x counts the
// kErrBlockPixels-pixel blocks of a plane, blockIdx.y the samples (strided beyond 65535 of them).  A lane takes 4 consecutive
// pixels - 16 bytes of each float32 plane, 8 of a binary16 / bfloat16 one, 16 or 4 of the map, 4 of dist2 - in rounds of 1024
// pixels per workgroup; the steps of the definition are the host twin's functions (csrc/ofdg_device.h).
// The row is 168 words, too many to keep per lane, so each wave keeps a copy in LDS, packed: a workgroup sees at most
// kErrBlockPixels = 4096 pixels of a sample, so a cell is two 64-bit words - sum_epe_q8 (below 2^42) with n above bit 48, and
// the four outlier counts in 16 bits each - and a pixel costs at most two 64-bit LDS atomics.  Neighbouring pixels mostly fall
// into one cell and one histogram bin, so a lane first adds in registers and goes to LDS only when the cell (the bin) changes
// and at the end of the sample.  The key and the two unusable counts stay in registers and cross the wave with __shfl_xor.
// Then the workgroup unpacks and issues one global integer atomic per non-zero word of the row and one 64-bit atomicMax for
// the key.  Integer atomics only: no bit depends on arrival order.  kPlanes: epe or the picture is written - the rows-only
// form holds none of that code.  No scratch.
constexpr int kErrThreads = 256;
constexpr int kErrBlockPixels = 4096;
constexpr int kErrWaves = kErrThreads / 64;
static_assert(kErrBlockPixels % (kErrThreads * 4) == 0 && kErrBlockPixels <= 4096, "whole rounds of 4-pixel pieces; the packed counters hold 4096 pixels");
template <bool kGtHalf, int kEst, bool kPlanes>
__global__ __launch_bounds__(kErrThreads) void flow_error_kernel(const DevErrJob job, int n, uint32_t plane) {
  typedef typename FlowFmt<quad_fmt(kGtHalf)>::elem GtElem;
  typedef typename FlowFmt<kEst>::elem EstElem;
  __shared__ unsigned long long s_sum_n[kErrWaves][kErrCells];  // sum_epe_q8 | n << 48
  __shared__ unsigned long long s_out[kErrWaves][kErrCells];    // n_1px | n_3px << 16 | n_5px << 32 | n_fl << 48
  __shared__ uint32_t s_hist[kErrWaves][kErrHistBins];
  __shared__ unsigned long long s_key;
  __shared__ uint32_t s_bad[2];
  __shared__ uint32_t s_colour[kErrColours];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (kPlanes) {
    if (tid < kErrColours) s_colour[tid] = kErrColour[tid];  // (the first barrier of the sample loop orders it)
  }
  const uint32_t first = blockIdx.x * (uint32_t)kErrBlockPixels;
  const uint32_t end = first + (uint32_t)kErrBlockPixels < plane ? first + (uint32_t)kErrBlockPixels : plane;
  const ErrBands bands = err_bands(job);
  const bool with_rows = job.rows != nullptr, with_dist = job.dist2 != nullptr, one_row = job.flags & OFDG_ERR_ONE_ROW;
  const bool dim_occ = job.flags & OFDG_ERR_DIM_OCC, occ_u8 = job.occ_fmt == OFDG_FMT_U8;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    for (int k = tid; k < kErrWaves * kErrCells; k += kErrThreads) { (&s_sum_n[0][0])[k] = 0ull; (&s_out[0][0])[k] = 0ull; }
    if (tid < kErrWaves * kErrHistBins) (&s_hist[0][0])[tid] = 0u;
    if (tid == 64) s_key = 0ull;
    if (tid == 65 || tid == 66) s_bad[tid - 65] = 0u;
    __syncthreads();
    const size_t base = (size_t)i * 2 * plane, base1 = (size_t)i * plane;
    const uint32_t idx_base = one_row ? (uint32_t)i * plane : 0u;
    uint32_t cur_cell = 0, cur_bin = 0, bin_count = 0, n_bad_gt = 0, n_bad_est = 0;
    unsigned long long acc_sum_n = 0, acc_out = 0, key = 0;
    for (uint32_t at = first + (uint32_t)tid * 4u; at < end; at += (uint32_t)(kErrThreads * 4)) {
      float ug[4], vg[4], ue[4], ve[4];
      quad_load<quad_fmt(kGtHalf)>(static_cast<const GtElem*>(job.gt) + (base + at), ug);
      quad_load<quad_fmt(kGtHalf)>(static_cast<const GtElem*>(job.gt) + (base + plane + at), vg);
      quad_load<kEst>(static_cast<const EstElem*>(job.est) + (base + at), ue);
      quad_load<kEst>(static_cast<const EstElem*>(job.est) + (base + plane + at), ve);
      uint32_t hidden = 0, d2 = 0;  // bit q: pixel q is hidden; byte q: its dist2
      if (job.occ) {
        if (occ_u8) hidden = quad_load_hidden<true>(static_cast<const uint8_t*>(job.occ) + base1 + at);
        else hidden = quad_load_hidden<false>(static_cast<const float*>(job.occ) + base1 + at);
      }
      if (with_dist) d2 = *reinterpret_cast<const uint32_t*>(job.dist2 + base1 + at);
      float out_epe[4];
      uint32_t px[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float se = err_scaled(ue[q], job.est_scale), te = err_scaled(ve[q], job.est_scale);
        const bool gt_ok = flow_usable(ug[q], vg[q]), ok = gt_ok && flow_usable(se, te);
        n_bad_gt += gt_ok ? 0u : 1u;
        n_bad_est += (gt_ok && !ok) ? 1u : 0u;
        if constexpr (kPlanes) { out_epe[q] = -1.0f; px[q] = 0u; }
        if (ok) {
          const ErrPixel e = err_pixel(ug[q], vg[q], se, te);
          const bool hid = (hidden >> q) & 1u;
          if (with_rows) {
            const uint32_t cell = err_cell(hid, e.Gq, (d2 >> (8 * q)) & 255u, with_dist, bands), flags = err_flags(e.Eq, e.Gq), bin = err_hist_bin(e.Eq);
            if (cell != cur_cell) {
              if (acc_sum_n) atomicAdd(&s_sum_n[wave][cur_cell], acc_sum_n);
              if (acc_out) atomicAdd(&s_out[wave][cur_cell], acc_out);
              acc_sum_n = acc_out = 0ull;
              cur_cell = cell;
            }
            acc_sum_n += (unsigned long long)e.Eq | (1ull << 48);
            acc_out += (unsigned long long)(flags & 1u) | ((unsigned long long)((flags >> 1) & 1u) << 16) | ((unsigned long long)((flags >> 2) & 1u) << 32) |
                       ((unsigned long long)((flags >> 3) & 1u) << 48);
            if (bin != cur_bin) {
              if (bin_count) atomicAdd(&s_hist[wave][cur_bin], bin_count);
              bin_count = 0u;
              cur_bin = bin;
            }
            ++bin_count;
            const unsigned long long k = err_key(e.Eq, idx_base + at + (uint32_t)q);
            key = k > key ? k : key;
          }
          if constexpr (kPlanes) {
            out_epe[q] = err_epe(e.Eq);
            if (job.picture) px[q] = err_colour(e.Eq, e.Gq, dim_occ && hid, s_colour);
          }
        }
      }
      if constexpr (kPlanes) {
        if (job.epe) {
          if (job.epe_fmt == OFDG_FMT_F16)
            *reinterpret_cast<f16x4*>(static_cast<_Float16*>(job.epe) + base1 + at) = f16x4{(_Float16)out_epe[0], (_Float16)out_epe[1], (_Float16)out_epe[2], (_Float16)out_epe[3]};
          else
            *reinterpret_cast<f32x4*>(static_cast<float*>(job.epe) + base1 + at) = f32x4{out_epe[0], out_epe[1], out_epe[2], out_epe[3]};
        }
        if (job.picture) {
          uint8_t* const dst = static_cast<uint8_t*>(job.picture);
          if (job.layout == OFDG_VIS_HWC_RGB) {
            uint32_t* const dp = reinterpret_cast<uint32_t*>(dst + (base1 + at) * 3);
            dp[0] = px[0] | (px[1] << 24);
            dp[1] = (px[1] >> 8) | (px[2] << 16);
            dp[2] = (px[2] >> 16) | (px[3] << 8);
          } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {  // c: R, G, B of a pixel's word; plane 2 - c
              const uint32_t sh = 8u * (uint32_t)c;
              const uint32_t w = ((px[0] >> sh) & 255u) | (((px[1] >> sh) & 255u) << 8) | (((px[2] >> sh) & 255u) << 16) | (((px[3] >> sh) & 255u) << 24);
              *reinterpret_cast<uint32_t*>(dst + ((size_t)i * 3 + (size_t)(2 - c)) * plane + at) = w;
            }
          }
        }
      }
    }
    if (with_rows) {
      if (acc_sum_n) atomicAdd(&s_sum_n[wave][cur_cell], acc_sum_n);
      if (acc_out) atomicAdd(&s_out[wave][cur_cell], acc_out);
      if (bin_count) atomicAdd(&s_hist[wave][cur_bin], bin_count);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        n_bad_gt += (uint32_t)__shfl_xor((int)n_bad_gt, d, 64);
        n_bad_est += (uint32_t)__shfl_xor((int)n_bad_est, d, 64);
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, d, 64);
        key = other > key ? other : key;
      }
      if (lane == 0) {
        if (n_bad_gt) atomicAdd(&s_bad[0], n_bad_gt);
        if (n_bad_est) atomicAdd(&s_bad[1], n_bad_est);
        if (key) atomicMax(&s_key, key);
      }
      __syncthreads();
      DevErrRow* const out = job.rows + (one_row ? 0 : i);
      if (tid < kErrCells * 6) {  // word f of cell c: the sum, then n, n_1px, n_3px, n_5px, n_fl
        const int c = tid / 6, f = tid - c * 6;
        unsigned long long a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < kErrWaves; ++w) { a += s_sum_n[w][c]; b += s_out[w][c]; }
        if (f == 0) {
          const unsigned long long sum = a & ((1ull << 48) - 1ull);
          if (sum) atomicAdd(&out->cell[c].sum_epe_q8, sum);
        } else {
          const uint32_t v = f == 1 ? (uint32_t)(a >> 48) : (uint32_t)(b >> (16 * (f - 2))) & 0xFFFFu;
          if (v) atomicAdd(&out->cell[c].n + (f - 1), v);
        }
      } else if (tid < kErrCells * 6 + kErrHistBins) {
        const int b = tid - kErrCells * 6;
        uint32_t h = 0;
#pragma unroll
        for (int w = 0; w < kErrWaves; ++w) h += s_hist[w][b];
        if (h) atomicAdd(&out->hist[b], h);
      } else if (tid < kErrCells * 6 + kErrHistBins + 2) {
        const int k = tid - (kErrCells * 6 + kErrHistBins);
        if (s_bad[k]) atomicAdd(&out->n_bad[k], s_bad[k]);
      } else if (tid == kErrCells * 6 + kErrHistBins + 2 && s_key) {
        atomicMax(&out->max_key, s_key);
      }
    }
    __syncthreads();  // (the next sample of this workgroup clears the tables)
  }
}

// ---- Camera (ofdg_camera, include/ofdg.h) ----------------------------------------------------------------------------------
// One launch for both frames and every sample: blockIdx.x counts the kCameraTileW x kCameraTileH tiles of a frame, blockIdx.y
// the samples, blockIdx.z the frames that are set.  A 4-wave workgroup owns a tile, a lane four consecutive pixels of one row
// (width % 8 == 0: a lane's four pixels, and the eight of a pair of lanes, are whole or outside together).  The record is read
// or drawn, and sanitised, on uniform values once per (workgroup, sample); sigma, radius and pattern of the frame are pinned
// to scalar registers, so the four cases are uniform branches:
//   neither  the lane's own quad goes from source to destination: bit for bit (float32 to float32), else through its bytes.
//            Nothing is staged.
//   blur     channel by channel: the source bytes of the tile and a halo of R + 1 - rows clamped to the plane, columns as whole
//            aligned quads, a quad outside the plane replicating the edge byte (width % 4 == 0: a quad is inside or outside
//            whole) - go to LDS as bytes (`src`), the horizontal pass writes 16-bit rows (`h16`), the vertical pass the blurred
//            bytes of the tile and one pixel around it (`blur`).  A lane computes four neighbouring sums at a time: the
//            horizontal pass reads `src` a word at a time, unrolled over the words the radius needs, the weights in scalar
//            registers; the vertical pass reads four 16-bit sums a time.  Products are 24-bit multiply-adds.  Every source
//            element is read once per tile that needs it.
//   Bayer    the demosaic reads the mosaic from `blur` - a neighbour's sample is the blurred byte of the channel its site
//            has -, the coordinates reflected within the plane before they are made relative to the tile, so the entries of
//            `blur` outside the plane are never looked at.  Without a blur the bytes go to `blur` straight from the source.
// The taps are built once per (workgroup, sample): lane k makes e[k], lane k >= 1 then w[k], lane 0 w[0], through the
// functions of the host twin (csrc/ofdg_device.h), as is all the arithmetic, so the result is the twin's byte for byte.
// Every global index is clamped into the plane; every LDS index is bounded by the constants below (R <= 12).  13.7 KiB of
// LDS, no atomics, no scratch.
constexpr int kCameraThreads = 256;
constexpr int kCameraTileW = 64, kCameraTileH = 16;
constexpr int kCameraSrcHalo = 16;                                                   // columns of `src` left of the tile: R + 1 <= 13, rounded up to whole quads
constexpr int kCameraSrcW = kCameraTileW + 2 * kCameraSrcHalo;                       // 96 bytes a row of `src`
constexpr int kCameraRowsMax = kCameraTileH + 2 + 2 * kCameraMaxRadius;              // 42 rows of `src` and `h16`
constexpr int kCameraOutHalo = 4;                                                    // columns of `h16` and `blur` left of the tile: 1, rounded up to a quad
constexpr int kCameraOutW = kCameraTileW + 2 * kCameraOutHalo, kCameraOutH = kCameraTileH + 2;  // 72 x 18
static_assert(kCameraTileW / 4 * kCameraTileH == kCameraThreads, "a lane per four pixels of the tile");
static_assert(kCameraSrcHalo >= kCameraOutHalo + kCameraMaxRadius && kCameraThreads > kCameraMaxRadius, "the horizontal pass stays within `src`; a lane per tap");
// a weight times a byte, an h8 or a sum of two h8: both below 2^24, so one 24-bit multiply-add gives the low 32 bits of the product
__device__ __forceinline__ uint32_t camera_mad(uint32_t w, uint32_t v, uint32_t acc) { return __umul24(w, v) + acc; }
// Four neighbouring sums of the horizontal pass: `at` is the word of `src` that holds the four centre bytes, w[d] the weight at
// distance d (0 above the radius), kNW = ceil(R / 4) the words to look at on either side.  Unrolled: every distance is a constant.
template <int kNW>
__device__ __forceinline__ void camera_row_quad(const uint32_t* at, const uint32_t (&w)[kCameraMaxRadius + 1], uint32_t (&S)[4]) {
#pragma unroll
  for (int m = -kNW; m <= kNW; ++m) {
    const uint32_t word = at[m];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t v = (word >> (8 * b)) & 255u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int d = 4 * m + b - q, ad = d < 0 ? -d : d;
        if (ad <= 4 * kNW && ad <= kCameraMaxRadius) S[q] = camera_mad(w[ad], v, S[q]);
      }
    }
  }
}
template <bool kSrcU8, bool kDstU8>
__global__ __launch_bounds__(kCameraThreads) void camera_kernel(const DevCameraJob job, int n, int W, int H, uint32_t tiles_x) {
  constexpr int kSES = kSrcU8 ? 1 : 4, kDES = kDstU8 ? 1 : 4;
  __shared__ uint32_t s_src[kCameraRowsMax * kCameraSrcW / 4];
  __shared__ uint16_t s_h16[kCameraRowsMax * kCameraOutW] __attribute__((aligned(8)));
  __shared__ uint32_t s_blur[3 * kCameraOutH * kCameraOutW / 4];
  __shared__ uint32_t s_e[kCameraMaxRadius + 1], s_w[kCameraMaxRadius + 1];
  const uint8_t* const blur8 = reinterpret_cast<const uint8_t*>(s_blur);
  const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int TX = (int)(tx * kCameraTileW), TY = (int)(ty * kCameraTileH);  // the tile's first column and row in the frame
  const int lx = (int)(threadIdx.x & 15u) * 4, ly = (int)(threadIdx.x >> 4);
  const int X0 = TX + lx, Y = TY + ly;
  const int f = (blockIdx.z != 0u || !job.src[0]) ? 1 : 0;
  const uint8_t* const s_img = static_cast<const uint8_t*>(f ? job.src[1] : job.src[0]);
  uint8_t* const d_img = static_cast<uint8_t*>(f ? job.dst[1] : job.dst[0]);
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (3 * plane < 2^32: camera_arg_error)
  const bool inside = X0 < W && Y < H;
  const uint32_t at = inside ? (uint32_t)Y * (uint32_t)W + (uint32_t)X0 : 0u;  // the lane's first pixel in a channel
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    DevCameraRec r;
    if (job.recs) r = job.recs[i];
    else r = camera_draw_rec(job.seed, (unsigned long long)(job.first_index + i), job);
    r = camera_sanitise(r);
    if (job.recs_out && blockIdx.x == 0u && blockIdx.z == 0u && threadIdx.x == 0u) {
      u32x4* const o = reinterpret_cast<u32x4*>(job.recs_out + i);
      o[0] = u32x4{(uint32_t)r.sigma_q8[0], (uint32_t)r.sigma_q8[1], (uint32_t)r.bayer, (uint32_t)r.radius[0]};
      o[1] = u32x4{(uint32_t)r.radius[1], 0u, 0u, 0u};
    }
    const int s = __builtin_amdgcn_readfirstlane(f ? r.sigma_q8[1] : r.sigma_q8[0]);
    const int R = __builtin_amdgcn_readfirstlane(f ? r.radius[1] : r.radius[0]);
    const int p = __builtin_amdgcn_readfirstlane(r.bayer);
    const uint8_t* const sp = s_img + (size_t)i * 3 * plane * kSES;
    uint8_t* const dp = d_img + (size_t)i * 3 * plane * kDES;
    if (s == 0 && p < 0) {  // neither (uniform): the copy
      if constexpr (!kSrcU8 && !kDstU8) {
        if (inside) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const size_t e = ((size_t)c * plane + at) * 4u;
            quad_store_u32x4(reinterpret_cast<u32x4*>(dp + e), *reinterpret_cast<const u32x4*>(sp + e));
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          uint32_t own[4] = {0u, 0u, 0u, 0u};
          if (inside) quad_load_bytes<kSrcU8>(sp + ((size_t)c * plane + at) * kSES, own);
          if constexpr (kDstU8) quad_store_bytes_pair(dp + (uint32_t)c * plane + at, quad_word(own), inside);
          else quad_store_bytes_f32(dp + ((size_t)c * plane + at) * 4u, own, inside);
        }
      }
      continue;
    }
    if (s > 0) {  // the taps of this frame
      if ((int)threadIdx.x <= R) s_e[threadIdx.x] = camera_tap_e(s, (int)threadIdx.x);
      __syncthreads();
      if ((int)threadIdx.x >= 1 && (int)threadIdx.x <= R) {
        uint32_t E = s_e[0];
        for (int k = 1; k <= R; ++k) E += 2u * s_e[k];
        s_w[threadIdx.x] = camera_tap_w(s_e[threadIdx.x], E);
      } else if ((int)threadIdx.x > R && (int)threadIdx.x <= kCameraMaxRadius) {
        s_w[threadIdx.x] = 0u;
      }
      __syncthreads();
      if (threadIdx.x == 0u) {
        uint32_t side = 0u;
        for (int k = 1; k <= R; ++k) side += s_w[k];
        s_w[0] = 65536u - 2u * side;
      }
      // (the barrier behind the first staging stands between this and the first use of s_w[0])
    }
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
      const uint8_t* const cp = sp + (size_t)c * plane * kSES;
      uint32_t* const bl = s_blur + c * (kCameraOutH * kCameraOutW / 4);
      if (s > 0) {
        // `src`: row j is the frame's row TY - 1 - R + j, clamped; quad q its columns TX - 16 + 4 q ..
        const int rows = kCameraOutH + 2 * R;
        const int q0 = (kCameraSrcHalo - kCameraOutHalo - R) >> 2, nq = kCameraSrcW / 4 - 2 * q0;
        for (int t = (int)threadIdx.x; t < rows * nq; t += kCameraThreads) {
          const int j = t / nq, q = q0 + (t - j * nq);
          const int gy = camera_clamp(TY - 1 - R + j, H), gx = TX - kCameraSrcHalo + 4 * q;
          const int cx = gx < 0 ? 0 : gx >= W ? W - 4 : gx;
          uint32_t b[4];
          quad_load_bytes<kSrcU8>(cp + ((size_t)gy * (uint32_t)W + (uint32_t)cx) * kSES, b);
          const uint32_t word = gx < 0 ? b[0] * 0x01010101u : gx >= W ? b[3] * 0x01010101u : quad_word(b);
          s_src[j * (kCameraSrcW / 4) + q] = word;
        }
        __syncthreads();  // (also: the last channel's vertical pass has read `h16`, and s_w[0] is written)
        // the horizontal pass: `h16` row j, columns TX - 4 + 4 g .. + 3.  The weights go to scalar registers (they are the
        // workgroup's), the bytes are read a word at a time.
        uint32_t w[kCameraMaxRadius + 1];
#pragma unroll
        for (int k = 0; k <= kCameraMaxRadius; ++k) w[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_w[k]) & 0x1FFFFu;
        const int words = (R + 3) >> 2;  // (uniform)
        for (int t = (int)threadIdx.x; t < rows * (kCameraOutW / 4); t += kCameraThreads) {
          const int j = t / (kCameraOutW / 4), g = t - j * (kCameraOutW / 4);
          const uint32_t* const at = s_src + j * (kCameraSrcW / 4) + (kCameraSrcHalo - kCameraOutHalo) / 4 + g;
          uint32_t S[4] = {0u, 0u, 0u, 0u};
          if (words == 1) camera_row_quad<1>(at, w, S);
          else if (words == 2) camera_row_quad<2>(at, w, S);
          else camera_row_quad<3>(at, w, S);
          const u32x2 o = {camera_h8(S[0]) | (camera_h8(S[1]) << 16), camera_h8(S[2]) | (camera_h8(S[3]) << 16)};
          *reinterpret_cast<u32x2*>(s_h16 + j * kCameraOutW + 4 * g) = o;
        }
        __syncthreads();
        // the vertical pass: `blur` row v is the frame's row TY - 1 + v, from the rows v .. v + 2 R of `h16`, four columns
        // (8 bytes) a read
        for (int t = (int)threadIdx.x; t < kCameraOutH * (kCameraOutW / 4); t += kCameraThreads) {
          const int v = t / (kCameraOutW / 4), g = t - v * (kCameraOutW / 4);
          const u32x2* const col = reinterpret_cast<const u32x2*>(s_h16 + (v + R) * kCameraOutW + 4 * g);
          const u32x2 c = col[0];
          uint32_t S0 = camera_mad(w[0], c[0] & 0xFFFFu, 0u), S1 = camera_mad(w[0], c[0] >> 16, 0u);
          uint32_t S2 = camera_mad(w[0], c[1] & 0xFFFFu, 0u), S3 = camera_mad(w[0], c[1] >> 16, 0u);
#pragma unroll 1
          for (int k = 1; k <= R; ++k) {
            const uint32_t wk = s_w[k] & 0x1FFFFu;
            const u32x2 up = col[-k * (kCameraOutW / 4)], dn = col[k * (kCameraOutW / 4)];
            S0 = camera_mad(wk, (up[0] & 0xFFFFu) + (dn[0] & 0xFFFFu), S0);
            S1 = camera_mad(wk, (up[0] >> 16) + (dn[0] >> 16), S1);
            S2 = camera_mad(wk, (up[1] & 0xFFFFu) + (dn[1] & 0xFFFFu), S2);
            S3 = camera_mad(wk, (up[1] >> 16) + (dn[1] >> 16), S3);
          }
          bl[v * (kCameraOutW / 4) + g] = camera_byte(S0) | (camera_byte(S1) << 8) | (camera_byte(S2) << 16) | (camera_byte(S3) << 24);
        }
        // (the next channel's first barrier stands between this pass and the next writing of `h16`; `src` was last read
        // in front of the barrier above)
      } else {
        // Bayer alone: the bytes of the tile and one pixel around it, as whole quads at clamped places (an entry outside the
        // plane is not looked at)
        for (int t = (int)threadIdx.x; t < kCameraOutH * (kCameraOutW / 4); t += kCameraThreads) {
          const int v = t / (kCameraOutW / 4), g = t - v * (kCameraOutW / 4);
          const int gy = camera_clamp(TY - 1 + v, H), gx = TX - kCameraOutHalo + 4 * g;
          const int cx = gx < 0 ? 0 : gx >= W ? W - 4 : gx;
          uint32_t b[4];
          quad_load_bytes<kSrcU8>(cp + ((size_t)gy * (uint32_t)W + (uint32_t)cx) * kSES, b);
          bl[v * (kCameraOutW / 4) + g] = quad_word(b);
        }
      }
    }
    __syncthreads();
    uint32_t out[3][4] = {};
    if (inside) {
      const int at0 = (ly + 1) * kCameraOutW + kCameraOutHalo + lx;  // the lane's first pixel in a channel of `blur`
      if (p < 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint32_t w = s_blur[(c * kCameraOutH * kCameraOutW + at0) >> 2];
          out[c][0] = w & 255u; out[c][1] = (w >> 8) & 255u; out[c][2] = (w >> 16) & 255u; out[c][3] = w >> 24;
        }
      } else {
        const int b = camera_site_b(Y, p);
        const int rm = (camera_reflect(Y - 1, H) - TY + 1) * kCameraOutW, rp = (camera_reflect(Y + 1, H) - TY + 1) * kCameraOutW, r0 = (ly + 1) * kCameraOutW;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int x = X0 + q, a = camera_site_a(x, p);
          const int x0 = kCameraOutHalo + lx + q, xm = camera_reflect(x - 1, W) - TX + kCameraOutHalo, xp = camera_reflect(x + 1, W) - TX + kCameraOutHalo;
          const uint8_t* const pc = blur8 + camera_site_channel(a, b) * (kCameraOutH * kCameraOutW);
          const uint8_t* const ph = blur8 + camera_site_channel(a ^ 1, b) * (kCameraOutH * kCameraOutW);
          const uint8_t* const pv = blur8 + camera_site_channel(a, b ^ 1) * (kCameraOutH * kCameraOutW);
          const uint8_t* const pd = blur8 + camera_site_channel(a ^ 1, b ^ 1) * (kCameraOutH * kCameraOutW);
          uint32_t o[3];
          camera_demosaic(a, b, pc[r0 + x0], (uint32_t)ph[r0 + xm] + ph[r0 + xp], (uint32_t)pv[rm + x0] + pv[rp + x0],
                          (uint32_t)pd[rm + xm] + pd[rm + xp] + pd[rp + xm] + pd[rp + xp], o);
          out[0][q] = o[0]; out[1][q] = o[1]; out[2][q] = o[2];
        }
      }
    }
    // (the lanes of a pair are inside together: X0 of the even one is a multiple of 8)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (kDstU8) quad_store_bytes_pair(dp + (uint32_t)c * plane + at, quad_word(out[c]), inside);
      else quad_store_bytes_f32(dp + ((size_t)c * plane + at) * 4u, out[c], inside);
    }
    __syncthreads();  // (the next sample of this workgroup stages the tile again)
  }
}

// --------------------------------------------------------------------------
// Lens (ofdg_lens): every plane of a batch bent by one radial distortion per sample - the spatial augmentation's gather with
// another map, a Newton inverse for the flow, a magnification per colour channel and a vignette.  The functions of the
// definition are the host twin's (csrc/ofdg_device.h), so the result is the twin's bit for bit.
// --------------------------------------------------------------------------
// The walk is spatial_kernel's, with the output of the source's size: four neighbouring lanes own a unit of 16 elements, a
// lane four consecutive pixels, a workgroup a tile of kSpatialTileQ units x kSpatialTileP row pairs; blockIdx.x counts the
// tiles, blockIdx.y the samples, blockIdx.z the frames that have a plane.  The record is drawn or read, sanitised and turned
// into the sample's constants (inv, both other magnifications, 1 / z, 3 k1) on uniform values once per (workgroup, sample);
// rho, L, the geometric taps and the vignette of a pixel are computed once and serve the three channels, the flow, the map
// and the label.  G is always sampled at the geometric position, B and R too where their aberration is 0 (a uniform branch).
// The inverse - eight Newton steps, each with an fp64 division - is the only long fp64 chain, one per pixel of a frame that
// has a flow.  Sources are read element by element at computed, clamped indices, so no record reaches outside a plane; every
// store is one 16-byte piece.  No LDS, no atomics, no scratch.
template <bool kImageU8, bool kFlowHalf, bool kOccU8>
__global__ __launch_bounds__(kSpatialThreads) void lens_kernel(const DevLensJob job, int n, int W, int H, uint32_t tiles_x) {
  constexpr int kImageES = kImageU8 ? 1 : 4, kFlowES = kFlowHalf ? 2 : 4, kOccES = kOccU8 ? 1 : 4;
  const uint32_t R = (uint32_t)W / 8u, pairs = (uint32_t)H / 2u;  // units per row pair, row pairs
  const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const uint32_t j = threadIdx.x & 3u, u = threadIdx.x >> 2;  // the lane's four pixels of its unit; the unit of the pass
  const uint32_t q = tx * kSpatialTileQ + u % kSpatialTileQ, P0 = ty * kSpatialTileP + u / kSpatialTileQ;
  const uint32_t t = 2u * q + (j >> 1);  // the run of 8 among the 2 R runs of a row pair
  const bool second = t >= R;
  const int X0 = (int)((t - (second ? R : 0u)) * 8u + (j & 1u) * 4u);
  const bool frame0 = job.src[0] || job.src[2] || job.src[4] || job.src[6];
  const int f = (blockIdx.z != 0u || !frame0) ? 1 : 0;
  const uint8_t* const s_img = static_cast<const uint8_t*>(f ? job.src[1] : job.src[0]);
  const uint8_t* const s_flow = static_cast<const uint8_t*>(f ? job.src[3] : job.src[2]);
  const uint8_t* const s_occ = static_cast<const uint8_t*>(f ? job.src[5] : job.src[4]);
  const uint8_t* const s_lab = static_cast<const uint8_t*>(f ? job.src[7] : job.src[6]);
  uint8_t* const d_img = static_cast<uint8_t*>(f ? job.dst[1] : job.dst[0]);
  uint8_t* const d_flow = static_cast<uint8_t*>(f ? job.dst[3] : job.dst[2]);
  uint8_t* const d_occ = static_cast<uint8_t*>(f ? job.dst[5] : job.dst[4]);
  uint8_t* const d_lab = static_cast<uint8_t*>(f ? job.dst[7] : job.dst[6]);
  const bool occ_window = job.flags & 16;
  const size_t frame = (size_t)W * H;
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    DevLensRec r;
    if (job.recs) r = job.recs[i];
    else r = lens_draw_rec(job.seed, (unsigned long long)(job.first_index + i), job, W, H);
    r = lens_sanitise(r, W, H);
    if (job.recs_out && blockIdx.x == 0u && blockIdx.z == 0u && threadIdx.x == 0u) {
      double2* const o = reinterpret_cast<double2*>(job.recs_out + i);
      o[0] = make_double2(r.k1, r.z); o[1] = make_double2(r.ca_b, r.ca_r); o[2] = make_double2(r.vig, r.cx);
      o[3] = make_double2(r.cy, 0.0);  // (the reserved words are the bits of +0.0)
    }
    if (q >= R) continue;  // (a whole unit, its four lanes together)
    const LensSetup o = lens_setup(r, W, H);
    const bool vignette = o.vig != 0.0;
    const uint8_t* const si = s_img + (size_t)i * 3 * frame * kImageES;
    const uint8_t* const sf = s_flow + (size_t)i * 2 * frame * kFlowES;
    const uint8_t* const so = s_occ + (size_t)i * frame * kOccES;
    const uint8_t* const sl = s_lab + (size_t)i * frame;
#pragma unroll 1
    for (int pass = 0; pass < kSpatialPasses; ++pass) {
      const uint32_t P = P0 + (uint32_t)pass * kSpatialRowPairs;
      if (P >= pairs) break;  // (whole units again)
      const int Y = (int)(2u * P + (second ? 1u : 0u));
      const size_t at = ((size_t)P * R + q) * 16u + 4u * j;  // the lane's first element in a channel of the destination
      const double dy = (double)Y - o.cy;
      float img[3][4], fu[4], fv[4];
      uint32_t hid[4], lab[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int X = X0 + p;
        const double dx = (double)X - o.cx;
        const double rho = lens_rho(dx, dy, o.inv);
        const double L = lens_L(o.k1, rho);
        const double qx = lens_coord(o.cx, o.z, L, dx), qy = lens_coord(o.cy, o.z, L, dy);
        const int Qx = spatial_fixed(qx), Qy = spatial_fixed(qy);
        const uint32_t near = (uint32_t)spatial_clamp((Qy + 128) >> 8, H) * (uint32_t)W + (uint32_t)spatial_clamp((Qx + 128) >> 8, W);
        if (s_img) {
          const float gain = lens_gain(o.vig, rho);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const double zc = lens_channel_z(o, c);
            int Cx = Qx, Cy = Qy;
            if (zc != o.z) {  // (uniform: the sample's)
              Cx = spatial_fixed(lens_coord(o.cx, zc, L, dx));
              Cy = spatial_fixed(lens_coord(o.cy, zc, L, dy));
            }
            const int fx = Cx & 255, fy = Cy & 255;
            const uint32_t x0 = (uint32_t)spatial_clamp(Cx >> 8, W), x1 = (uint32_t)spatial_clamp((Cx >> 8) + 1, W);
            const uint32_t y0 = (uint32_t)spatial_clamp(Cy >> 8, H) * (uint32_t)W, y1 = (uint32_t)spatial_clamp((Cy >> 8) + 1, H) * (uint32_t)W;
            float e00, e10, e01, e11;
            if constexpr (kImageU8) {
              const uint8_t* const pc = si + (size_t)c * frame;
              e00 = (float)pc[y0 + x0]; e10 = (float)pc[y0 + x1]; e01 = (float)pc[y1 + x0]; e11 = (float)pc[y1 + x1];
            } else {
              const uint8_t* const pc = si + (size_t)c * frame * 4u;
              e00 = elem_load<OFDG_FMT_F32>(pc, y0 + x0); e10 = elem_load<OFDG_FMT_F32>(pc, y0 + x1);
              e01 = elem_load<OFDG_FMT_F32>(pc, y1 + x0); e11 = elem_load<OFDG_FMT_F32>(pc, y1 + x1);
            }
            float v = spatial_blend(e00, e10, e01, e11, fx, fy);
            if (vignette) v = spatial_quiet(v * gain);
            img[c][p] = v;
          }
        }
        double px = 0.0, py = 0.0;
        bool solved = true;
        if (s_flow) {
          const float su = elem_load<quad_fmt(kFlowHalf)>(sf, near), sv = elem_load<quad_fmt(kFlowHalf)>(sf, frame + near);
          const double tx_ = qx + (double)su, ty_ = qy + (double)sv;
          solved = lens_inverse(o, tx_, ty_, &px, &py);
          fu[p] = solved ? spatial_flow_of(px, X) : lens_nan();
          fv[p] = solved ? spatial_flow_of(py, Y) : lens_nan();
        }
        if (s_occ) {
          bool hidden;
          if constexpr (kOccU8) hidden = so[near] != 0;
          else hidden = elem_load<OFDG_FMT_F32>(so, near) != 0.0f;
          hidden = hidden || !spatial_inside(Qx, Qy, W, H) || !solved;
          if (occ_window) hidden = hidden || !(spatial_partner_inside(px, W) && spatial_partner_inside(py, H));
          hid[p] = hidden ? 1u : 0u;
        }
        if (s_lab) lab[p] = sl[near];
      }
      // (the lanes of a unit are all here: q and P are the unit's)
      if (s_img) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if constexpr (kImageU8) {
            const uint32_t b[4] = {spatial_to_byte(img[c][0]), spatial_to_byte(img[c][1]), spatial_to_byte(img[c][2]), spatial_to_byte(img[c][3])};
            const uint32_t w = quad_word(b);
            const u32x4 v = {w, (uint32_t)__shfl_down((int)w, 1), (uint32_t)__shfl_down((int)w, 2), (uint32_t)__shfl_down((int)w, 3)};
            if (j == 0u) spatial_store(d_img + ((size_t)i * 3 + c) * frame + at, v);
          } else {
            const u32x4 v = {__float_as_uint(img[c][0]), __float_as_uint(img[c][1]), __float_as_uint(img[c][2]), __float_as_uint(img[c][3])};
            spatial_store(d_img + (((size_t)i * 3 + c) * frame + at) * 4u, v);
          }
        }
      }
      if (s_flow) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float* const v = c ? fv : fu;
          if constexpr (kFlowHalf) {
            const uint32_t w0 = spatial_half_bits(v[0]) | (spatial_half_bits(v[1]) << 16), w1 = spatial_half_bits(v[2]) | (spatial_half_bits(v[3]) << 16);
            const u32x4 w = {w0, w1, (uint32_t)__shfl_down((int)w0, 1), (uint32_t)__shfl_down((int)w1, 1)};
            if ((j & 1u) == 0u) spatial_store(d_flow + (((size_t)i * 2 + c) * frame + at) * 2u, w);
          } else {
            const u32x4 w = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
            spatial_store(d_flow + (((size_t)i * 2 + c) * frame + at) * 4u, w);
          }
        }
      }
      if (s_occ) {
        if constexpr (kOccU8) {
          const uint32_t w = quad_word(hid);
          const u32x4 v = {w, (uint32_t)__shfl_down((int)w, 1), (uint32_t)__shfl_down((int)w, 2), (uint32_t)__shfl_down((int)w, 3)};
          if (j == 0u) spatial_store(d_occ + (size_t)i * frame + at, v);
        } else {
          const u32x4 v = {hid[0] ? 0x3f800000u : 0u, hid[1] ? 0x3f800000u : 0u, hid[2] ? 0x3f800000u : 0u, hid[3] ? 0x3f800000u : 0u};
          spatial_store(d_occ + ((size_t)i * frame + at) * 4u, v);
        }
      }
      if (s_lab) {
        const uint32_t w = quad_word(lab);
        const u32x4 v = {w, (uint32_t)__shfl_down((int)w, 1), (uint32_t)__shfl_down((int)w, 2), (uint32_t)__shfl_down((int)w, 3)};
        if (j == 0u) spatial_store(d_lab + (size_t)i * frame + at, v);
      }
    }
  }
}

// ---- Block compression (ofdg_jpeg, include/ofdg.h) -------------------------------------------------------------------------
// One launch for both frames and every sample: blockIdx.x counts the 16x16 regions of the block grid, blockIdx.y the samples,
// blockIdx.z the frames that are set.  A 4-wave workgroup owns one region at the sample's phase - one 4:2:0 MCU, or 2 x 2 MCUs
// of 4:4:4 -, wave w its 8x8 quadrant, a lane one pixel: lane = 8 row + column.  The grid covers the largest phase (15); a
// region that does not meet the plane at the sample's phase is skipped by its whole workgroup.  The record is read or drawn,
// and sanitised, on uniform values once per (workgroup, sample); quality, subsampling and phase are pinned to scalar
// registers, so every branch on them is uniform.
//   A lane reads its pixel at clamped coordinates (the edge replicated), makes Y, Cb, Cr in registers, and a wave transforms one
//   8x8 block at a time with a lane an element: the two passes of each transform exchange through the wave's own 64 words of
//   LDS, a row read for the passes along x, a column read for those along y.  The pitch is 8 words: a 32-lane half (four rows of eight
//   lanes) meets 4 addresses 8 banks apart in a row read and 8 consecutive words in a column read (the other lanes share one
//   of them), and writes 32 consecutive words, so no access conflicts under the 32-bank rule of a one-word LDS read or write
//   (profiles/jpeg_device_code.txt).  The lane's four slices of T stay
//   in registers.  4:4:4: three blocks a wave (Y, Cb, Cr of its quadrant).  4:2:0: the four Y blocks, then Cb and Cr go
//   through LDS as bytes, a lane averages one 2x2 cell, waves 0 and 1 transform the two chroma blocks (2 and 3 run along on
//   the same values and drop them), and every lane picks up its cell's decoded pair.
//   The two tables of the (sample, frame) are built once per workgroup by 128 lanes.  All the arithmetic is the host twin's
//   (csrc/ofdg_device.h), so the result is the twin's byte for byte.
// Every global read of a sample stands in front of the first barrier of the first transform and every write behind the last,
// and a clamped coordinate of a region that meets the plane lies in that region: the in-place form (dst[f] == src[f]) reads
// nothing another workgroup writes.  quality 0: three waves copy the region at phase 0, a channel each and a quad a lane (bit for
// bit from float32 to float32, else through the bytes), or, in place, nothing.
// Every global index is clamped into the plane or guarded by `inside`; every LDS index is below its array's bound by
// construction (lane < 64; X, Y < 16).  2176 bytes of LDS, no atomics, no scratch.
constexpr int kJpegThreads = 256, kJpegRegion = 16;
// One block, a lane an element (lx, ly): step 6 of the definition.  xb: the wave's 64 words; q: the table; the lane's slices of
// T: rx[k] = T[lx][k], ry[k] = T[ly][k], cx[k] = T[k][lx], cy[k] = T[k][ly].  Every lane of the workgroup calls it together.
__device__ __forceinline__ int32_t jpeg_lane_block(int32_t sample, const uint16_t* q, int32_t* xb, int lx, int ly, const int32_t (&rx)[8],
                                                   const int32_t (&ry)[8], const int32_t (&cx)[8], const int32_t (&cy)[8]) {
  const int own = ly * 8 + lx;
  int32_t s;
  xb[own] = sample - 128;
  __syncthreads();
  s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += rx[k] * xb[ly * 8 + k];  // A[y][u]: y = ly, u = lx
  s = jpeg_round9(s);
  __syncthreads();
  xb[own] = s;
  __syncthreads();
  s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += ry[k] * xb[k * 8 + lx];  // F[v][u]: v = ly, u = lx
  const uint32_t Q = q[own];
  s = jpeg_level(s, Q) * (int32_t)Q;
  __syncthreads();
  xb[own] = s;
  __syncthreads();
  s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += cy[k] * xb[k * 8 + lx];  // B[y][u]: y = ly, u = lx
  s = jpeg_round9(s);
  __syncthreads();
  xb[own] = s;
  __syncthreads();
  s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += cx[k] * xb[ly * 8 + k];  // P[y][x]: y = ly, x = lx
  __syncthreads();  // (the next block of this wave writes xb)
  return jpeg_sample(s);
}
template <bool kSrcU8, bool kDstU8>
__global__ __launch_bounds__(kJpegThreads) void jpeg_kernel(const DevJpegJob job, int n, int W, int H, uint32_t tiles_x) {
  constexpr int kSES = kSrcU8 ? 1 : 4, kDES = kDstU8 ? 1 : 4;
  __shared__ int32_t s_x[4][64];
  __shared__ int32_t s_t[64];
  __shared__ uint16_t s_q[2][64];
  __shared__ uint8_t s_c[2][kJpegRegion * kJpegRegion];
  __shared__ uint8_t s_d[2][64];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int lx = lane & 7, ly = lane >> 3;
  const int X = 8 * (wave & 1) + lx, Y = 8 * (wave >> 1) + ly;  // the lane's pixel in the region
  const int TX = (int)(blockIdx.x % tiles_x) * kJpegRegion, TY = (int)(blockIdx.x / tiles_x) * kJpegRegion;
  const int f = (blockIdx.z != 0u || !job.src[0]) ? 1 : 0;
  const uint8_t* const s_img = static_cast<const uint8_t*>(f ? job.src[1] : job.src[0]);
  uint8_t* const d_img = static_cast<uint8_t*>(f ? job.dst[1] : job.dst[0]);
  const uint32_t plane = (uint32_t)W * (uint32_t)H;  // (3 * plane < 2^32: jpeg_arg_error)
  if (threadIdx.x < 64u) s_t[threadIdx.x] = kJpegT[threadIdx.x];
  __syncthreads();
  int32_t t_rx[8], t_ry[8], t_cx[8], t_cy[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    t_rx[k] = s_t[lx * 8 + k]; t_ry[k] = s_t[ly * 8 + k];
    t_cx[k] = s_t[k * 8 + lx]; t_cy[k] = s_t[k * 8 + ly];
  }
  int32_t* const xb = s_x[wave];
  for (int i = (int)blockIdx.y; i < n; i += (int)gridDim.y) {
    DevJpegRec r;
    if (job.recs) r = job.recs[i];
    else r = jpeg_draw_rec(job.seed, (unsigned long long)(job.first_index + i), job);
    r = jpeg_sanitise(r);
    if (job.recs_out && blockIdx.x == 0u && blockIdx.z == 0u && threadIdx.x == 0u) {
      u32x4* const o = reinterpret_cast<u32x4*>(job.recs_out + i);
      o[0] = u32x4{(uint32_t)r.quality[0], (uint32_t)r.quality[1], (uint32_t)r.subsample, (uint32_t)r.phase_x};
      o[1] = u32x4{(uint32_t)r.phase_y, 0u, 0u, 0u};
    }
    const int quality = __builtin_amdgcn_readfirstlane(f ? r.quality[1] : r.quality[0]);
    const int sub = __builtin_amdgcn_readfirstlane(r.subsample);
    const uint8_t* const sp = s_img + (size_t)i * 3 * plane * kSES;
    uint8_t* const dp = d_img + (size_t)i * 3 * plane * kDES;
    if (quality == 0) {  // (uniform) the copy of the region at phase 0; in place: nothing
      if (d_img != s_img) {
        // as quads: wave c < 3 takes channel c, a lane four pixels of one row (W % 4 == 0: a quad is whole or outside)
        const int gx = TX + 4 * (lane & 3), gy = TY + (lane >> 2);
        const bool on = wave < 3 && gx < W && gy < H;
        const uint32_t e = on ? (uint32_t)wave * plane + (uint32_t)gy * (uint32_t)W + (uint32_t)gx : 0u;
        if constexpr (!kSrcU8 && !kDstU8) {
          if (on) quad_store_u32x4(reinterpret_cast<u32x4*>(dp + (size_t)e * 4u), *reinterpret_cast<const u32x4*>(sp + (size_t)e * 4u));
        } else {
          uint32_t own[4] = {0u, 0u, 0u, 0u};
          if (on) quad_load_bytes<kSrcU8>(sp + (size_t)e * kSES, own);
          if constexpr (!kDstU8) quad_store_bytes_f32(dp + (size_t)e * 4u, own, on);
          else if (on) *reinterpret_cast<uint32_t*>(dp + e) = quad_word(own);  // (the lane's own word: the pair store's shuffle costs this kernel a wave a SIMD)
        }
      }
      continue;
    }
    const int ox = TX - __builtin_amdgcn_readfirstlane(jpeg_phase(r.phase_x, sub)), oy = TY - __builtin_amdgcn_readfirstlane(jpeg_phase(r.phase_y, sub));
    if (ox >= W || oy >= H) continue;  // (uniform; ox + 16 > 0 and oy + 16 > 0 always) the region lies outside the plane
    const int px = ox + X, py = oy + Y;
    const bool inside = px >= 0 && px < W && py >= 0 && py < H;
    const uint32_t at = (uint32_t)camera_clamp(py, H) * (uint32_t)W + (uint32_t)camera_clamp(px, W);
    int32_t yv, cb, cr;
    {
      const int32_t b = (int32_t)elem_load_byte<kSrcU8>(sp, at), g = (int32_t)elem_load_byte<kSrcU8>(sp, plane + at), rr = (int32_t)elem_load_byte<kSrcU8>(sp, 2u * plane + at);
      yv = jpeg_luma(rr, g, b); cb = jpeg_cb(rr, g, b); cr = jpeg_cr(rr, g, b);
    }
    if (threadIdx.x < 128u) s_q[wave][lane] = (uint16_t)jpeg_quant(wave ? kJpegBaseChroma[lane] : kJpegBaseLuma[lane], quality);
    // (the barriers of the first pass stand between this and the first quantiser)
    yv = jpeg_lane_block(yv, s_q[0], xb, lx, ly, t_rx, t_ry, t_cx, t_cy);
    if (!sub) {
      cb = jpeg_lane_block(cb, s_q[1], xb, lx, ly, t_rx, t_ry, t_cx, t_cy);
      cr = jpeg_lane_block(cr, s_q[1], xb, lx, ly, t_rx, t_ry, t_cx, t_cy);
    } else {
      s_c[0][Y * kJpegRegion + X] = (uint8_t)cb;
      s_c[1][Y * kJpegRegion + X] = (uint8_t)cr;
      __syncthreads();
      const uint8_t* const cell = s_c[wave & 1] + 2 * ly * kJpegRegion + 2 * lx;  // the cell (lx, ly) of Cb (even waves) or Cr
      const int32_t mean = jpeg_cell((int32_t)cell[0] + cell[1] + cell[kJpegRegion] + cell[kJpegRegion + 1]);
      const int32_t dec = jpeg_lane_block(mean, s_q[1], xb, lx, ly, t_rx, t_ry, t_cx, t_cy);
      if (wave < 2) s_d[wave][lane] = (uint8_t)dec;
      __syncthreads();
      cb = s_d[0][(Y >> 1) * 8 + (X >> 1)];
      cr = s_d[1][(Y >> 1) * 8 + (X >> 1)];
    }
    if (inside) {
      const int32_t o[3] = {jpeg_blue(yv, cb), jpeg_green(yv, cb, cr), jpeg_red(yv, cr)};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const size_t e = (size_t)c * plane + at;
        if constexpr (kDstU8) dp[e] = (uint8_t)o[c];
        else reinterpret_cast<float*>(dp)[e] = (float)o[c];
      }
    }
    __syncthreads();  // (the next sample of this workgroup writes the tables and the chroma bytes again)
  }
}

}  // namespace ofdg
