// Host "realize" step: blueprints -> device records (fp64 affines in the
// reference's operation order, texture placement, z-order), and the pieces it
// shares with the device realize (OFDG_HD_FN of ofdg_device.h).
//
// Mirrors DataGenerator::RealizeObjectBlueprint and the object set-up half of
// Process_TaskBucket (reference src/caffe/DataGenerator.cpp:1065-1173, 1183-1211)
// and MovingObjectBase::setIntrinsicTransform / setMotion / addBackgroundMotion
// (:302-335).  The 2x3 algebra restates agg::trans_affine (AGG 2.4
// agg_trans_affine.h): multiply = "apply this, then m"; members sx,shy,shx,sy,tx,ty.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "../../include/ofdg.h"
#include "ofdg_device.h"  // (OFDG_HD_FN too)

namespace ofdg {

// The algebra is one definition for the host and the device (both built with -ffp-contract=off: the same bits).  Only the
// sine and cosine differ: libm on the host, as in the reference; ofdg_det_sincos on the device (sampler_counter.hip).
OFDG_HD_FN Mat mat_identity() { return Mat{1.0, 0.0, 0.0, 1.0, 0.0, 0.0}; }
OFDG_HD_FN Mat mat_rotation_sc(double s, double c) { return Mat{c, s, -s, c, 0.0, 0.0}; }  // agg::trans_affine_rotation
inline Mat mat_rotation(double a) { return mat_rotation_sc(std::sin(a), std::cos(a)); }
OFDG_HD_FN Mat mat_scaling(double s) { return Mat{s, 0.0, 0.0, s, 0.0, 0.0}; }
OFDG_HD_FN Mat mat_translation(double x, double y) { return Mat{1.0, 0.0, 0.0, 1.0, x, y}; }
OFDG_HD_FN Mat mat_mul(const Mat& a, const Mat& m) {  // a *= m
  Mat r;
  r.sx = a.sx * m.sx + a.shy * m.shx;
  r.shx = a.shx * m.sx + a.sy * m.shx;
  r.tx = a.tx * m.sx + a.ty * m.shx + m.tx;
  r.shy = a.sx * m.shy + a.shy * m.sy;
  r.sy = a.shx * m.shy + a.sy * m.sy;
  r.ty = a.tx * m.shy + a.ty * m.sy + m.ty;
  return r;
}
OFDG_HD_FN Mat mat_invert(const Mat& a) {  // trans_affine::invert
  Mat r;
  const double d = 1.0 / (a.sx * a.sy - a.shy * a.shx);
  const double t0 = a.sy * d;
  r.sy = a.sx * d;
  r.shy = -a.shy * d;
  r.shx = -a.shx * d;
  const double t4 = -a.tx * t0 - a.ty * r.shx;
  r.ty = -a.tx * r.shy - a.ty * r.sy;
  r.sx = t0;
  r.tx = t4;
  return r;
}

// A warp-crop use of the batch (mode 9): entry k of the batch's crop table.
struct CropUse {
  int32_t crop;        // index of the served crop
  int32_t background;  // 1: the 2W x 2H upscaled copy is needed (DataGenerator.cpp:1194-1202)
};

struct RealizedBatch {
  std::vector<DevShape> shapes;
  std::vector<DevObject> objects;
  std::vector<DevSample> samples;
  std::vector<CropUse> crops;  // DevObject/DevShape.deform - 1 indexes this table
  std::vector<DevBgPrep> bgprep;  // per sample, if RealizeConfig.background_prep
};

// CropGenerator::get_crop (WarpFields.cpp:516-538): crops are served in order, each
// reuse_same + 1 = 3 times (DataGenerator.cpp:1018); the set is cycled when exhausted.
struct CropServer {
  int n_crops = 0, head = 0, counter = 0, reuse_same = 2;
  int get() {
    const int c = head % n_crops;
    if (++counter > reuse_same) { ++head; counter = 0; }
    return c;
  }
};

struct RealizeConfig {
  int W, H, mode;
  int pool_n, pool_w, pool_h;
  int background_prep = 0;
  // texture sources (TexSource of the ctx); 0 stride = "centre crops of the pool images" computed from pool_w/h
  uint64_t fg_stride = 0, fg_origin = 0, bg_stride = 0, bg_origin = 0;
  // background_prep: where the whole images are - a uniform pool at pool_addr, or one entry per image (mixed pool)
  uint64_t pool_addr = 0;
  const DevTexEntry* tex_table = nullptr;
};

// getRandomizedCrop(2W, 2H, angle, zoom, shift) of a pool image as one coordinate map (DG:87-109), from the cosine and
// sine of bg_prep_rad(angle).  CImg 2.x: rotate() takes degrees and grows the image to round(1 + |(w-1)cos| + |(h-1)sin|);
// crop(x0, y0, x1, y1) with float -> int truncation of x1 = x0 + 2W/zoom - 1; linear get_resize with boundary 0 steps
// (w - 1)/(sx - 1) when enlarging, w/sx otherwise.
OFDG_HD_FN float bg_prep_rad(float angle) {
  const float nangle = (float)((double)angle - 360.0 * floor((double)angle / 360.0));
  return (float)((double)nangle * 3.14159265358979323846 / 180.0);
}
OFDG_HD_FN DevBgPrep make_bg_prep(int pw, int ph, int W, int H, float ca, float sa, float zoom, int shift_x, int shift_y, uint64_t image_addr) {
  DevBgPrep p;
  const int TW = 2 * W, TH = 2 * H;
  p.ca = ca; p.sa = sa;
  const float ux = fabsf((pw - 1) * p.ca), uy = fabsf((pw - 1) * p.sa);
  const float vx = fabsf((ph - 1) * p.sa), vy = fabsf((ph - 1) * p.ca);
  const int rw = (int)floorf(1 + ux + vx + 0.5f), rh = (int)floorf(1 + uy + vy + 0.5f);
  p.w2 = 0.5f * (pw - 1); p.h2 = 0.5f * (ph - 1);
  p.rw2 = 0.5f * (rw - 1); p.rh2 = 0.5f * (rh - 1);
  p.rw = rw; p.rh = rh;
  if (pw >= TW && ph >= TH) {
    p.x0 = pw / 2 - TW / 2; p.y0 = ph / 2 - TH / 2;
    const int x1 = (int)((float)p.x0 + (float)TW / zoom - 1.0f), y1 = (int)((float)p.y0 + (float)TH / zoom - 1.0f);
    p.cw = x1 - p.x0 + 1; p.ch = y1 - p.y0 + 1;
  } else {  // smaller image: no crop, the whole rotated image is resized (DG:102-106)
    p.x0 = 0; p.y0 = 0; p.cw = rw; p.ch = rh;
  }
  p.fx = TW > p.cw ? (float)((p.cw - 1.0) / (TW - 1.0)) : (float)((double)p.cw / TW);
  p.fy = TH > p.ch ? (float)((p.ch - 1.0) / (TH - 1.0)) : (float)((double)p.ch / TH);
  p.shx = shift_x; p.shy = shift_y;
  p.image_addr = image_addr;
  p.pw = pw; p.ph = ph;
  p.rx0 = 0; p.ry0 = 0; p.rx1 = TW - 1; p.ry1 = TH - 1;
  return p;
}
// the host's record: libm's cosine and sine of a float, as the reference's CImg computes them
inline DevBgPrep make_bg_prep_host(int pw, int ph, int W, int H, float angle, float zoom, int shift_x, int shift_y, uint64_t image_addr) {
  const float rad = bg_prep_rad(angle);
  return make_bg_prep(pw, ph, W, H, std::cos(rad), std::sin(rad), zoom, shift_x, shift_y, image_addr);
}
// Narrows p's region to the texels of the 2W x 2H background texture compose reads: the centre W x H window (frame 0)
// and the window mapped through the texture warp `ti` (frame 1, bilinear), with a margin; the whole texture (as
// make_bg_prep leaves it) if that leaves it (reflection).  A background that mode 9 re-samples through a warp field reads
// frame 1 at displaced positions: `grow` widens the mapped window by the largest displacement, clipped to the texture (a tap
// outside it reads nothing); 0 for a rigid background.
OFDG_HD_FN void bg_prep_region(const Mat ti /* by value, see OFDG_HD_FN */, int W, int H, double grow, DevBgPrep* p) {
  const double wx0 = fmax(W / 2. - grow, 0.), wx1 = fmin(3 * W / 2. + grow, 2. * W - 1.), wy0 = fmax(H / 2. - grow, 0.), wy1 = fmin(3 * H / 2. + grow, 2. * H - 1.);
  double lox = W / 2., hix = 3 * W / 2., loy = H / 2., hiy = 3 * H / 2.;
  for (int k = 0; k < 4; ++k) {
    const double px = (k & 1) ? wx1 : wx0, py = (k & 2) ? wy1 : wy0;
    const double x = px * ti.sx + py * ti.shx + ti.tx, y = px * ti.shy + py * ti.sy + ti.ty;
    lox = fmin(lox, x); hix = fmax(hix, x); loy = fmin(loy, y); hiy = fmax(hiy, y);
  }
  const int m = 3;
  if (lox - m >= 0 && loy - m >= 0 && hix + m <= 2 * W - 1 && hiy + m <= 2 * H - 1) {
    p->rx0 = (int)lox - m; p->ry0 = (int)loy - m;
    p->rx1 = (int)hix + m + 1 < 2 * W - 1 ? (int)hix + m + 1 : 2 * W - 1;
    p->ry1 = (int)hiy + m + 1 < 2 * H - 1 ? (int)hiy + m + 1 : 2 * H - 1;
  }
}

// Returns OFDG_OK or an error code; *msg explains failures.
int realize_batch(const RealizeConfig& cfg, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps,
                  int n_bps, RealizedBatch* out, std::string* msg, CropServer* crops = nullptr);

}  // namespace ofdg
