// TEST INFRASTRUCTURE -- container shell of Anti-Grain Geometry, written for this
// repository so that the reference's DataGenerator.cpp compiles WITHOUT the real
// library (make -C oracle ref).  Only agg::trans_affine is real: its arithmetic is
// AGG 2.4's published definition (agg_trans_affine.h / .cpp), operation for
// operation, because setIntrinsicTransform / setMotion / addBackgroundMotion /
// getPointFlow of the reference are pinned through it.  Every other class has the
// right name and constructor shapes and renders NOTHING: masks, textures and
// frames of a harness built on this header are meaningless, only blueprints and
// affines are the reference's.
#ifndef OFDG_REF_SHELL_AGG_H_
#define OFDG_REF_SHELL_AGG_H_

#include <cmath>

namespace agg {

const double pi = 3.14159265358979323846;

struct trans_affine {
  double sx, shy, shx, sy, tx, ty;
  trans_affine() : sx(1.0), shy(0.0), shx(0.0), sy(1.0), tx(0.0), ty(0.0) {}
  trans_affine(double v0, double v1, double v2, double v3, double v4, double v5)
      : sx(v0), shy(v1), shx(v2), sy(v3), tx(v4), ty(v5) {}
  const trans_affine& multiply(const trans_affine& m) {
    double t0 = sx * m.sx + shy * m.shx;
    double t2 = shx * m.sx + sy * m.shx;
    double t4 = tx * m.sx + ty * m.shx + m.tx;
    shy = sx * m.shy + shy * m.sy;
    sy = shx * m.shy + sy * m.sy;
    ty = tx * m.shy + ty * m.sy + m.ty;
    sx = t0;
    shx = t2;
    tx = t4;
    return *this;
  }
  const trans_affine& invert() {
    double d = 1.0 / (sx * sy - shy * shx);
    double t0 = sy * d;
    sy = sx * d;
    shy = -shy * d;
    shx = -shx * d;
    double t4 = -tx * t0 - ty * shx;
    ty = -tx * shy - ty * sy;
    sx = t0;
    tx = t4;
    return *this;
  }
  const trans_affine& operator*=(const trans_affine& m) { return multiply(m); }
  trans_affine operator*(const trans_affine& m) const { return trans_affine(*this).multiply(m); }
  void transform(double* x, double* y) const {
    double tmp = *x;
    *x = tmp * sx + *y * shx + tx;
    *y = tmp * shy + *y * sy + ty;
  }
};

struct trans_affine_rotation : trans_affine {
  trans_affine_rotation(double a) : trans_affine(std::cos(a), std::sin(a), -std::sin(a), std::cos(a), 0.0, 0.0) {}
};
struct trans_affine_scaling : trans_affine {
  trans_affine_scaling(double x, double y) : trans_affine(x, 0.0, 0.0, y, 0.0, 0.0) {}
  trans_affine_scaling(double s) : trans_affine(s, 0.0, 0.0, s, 0.0, 0.0) {}
};
struct trans_affine_translation : trans_affine {
  trans_affine_translation(double x, double y) : trans_affine(1.0, 0.0, 0.0, 1.0, x, y) {}
};

// ---- everything below: names only ----
struct gray8 { gray8(unsigned = 0, unsigned = 255) {} };
struct rgba8 {};
struct rendering_buffer { void attach(unsigned char*, unsigned, unsigned, int) {} };
struct pixfmt_gray8 { pixfmt_gray8() {} explicit pixfmt_gray8(rendering_buffer&) {} };
struct pixfmt_rgb24 { pixfmt_rgb24() {} explicit pixfmt_rgb24(rendering_buffer&) {} };
struct pixfmt_rgba32 { pixfmt_rgba32() {} explicit pixfmt_rgba32(rendering_buffer&) {} };
template <class PixFmt> struct renderer_base {
  renderer_base() {}
  explicit renderer_base(PixFmt&) {}
  template <class C> void clear(const C&) {}
};
template <class Base> struct renderer_scanline_aa_solid {
  renderer_scanline_aa_solid() {}
  explicit renderer_scanline_aa_solid(Base&) {}
  template <class C> void color(const C&) {}
};
struct scanline_u8 {};
struct gamma_none {};
struct gamma_threshold { gamma_threshold(double = 0.5) {} };
struct rasterizer_sl_clip_int {};
template <class Clip = rasterizer_sl_clip_int> struct rasterizer_scanline_aa {
  void reset() {}
  template <class VS> void add_path(VS&, unsigned = 0) {}
  template <class G> void gamma(const G&) {}
};
template <class Ras, class Sl, class Ren> void render_scanlines(Ras&, Sl&, Ren&) {}
template <class Ras, class Sl, class Base, class Alloc, class Gen>
void render_scanlines_aa(Ras&, Sl&, Base&, Alloc&, Gen&) {}
struct ellipse { void init(double, double, double, double, unsigned = 0, bool = false) {} };
struct path_storage {
  void remove_all() {}
  void move_to(double, double) {}
  void line_to(double, double) {}
  void curve3(double, double, double, double) {}
  void close_polygon(unsigned = 0) {}
};
template <class VS, class Tr = trans_affine> struct conv_transform { conv_transform(VS&, const Tr&) {} };
template <class VS> struct conv_curve { explicit conv_curve(VS&) {} };
struct wrap_mode_reflect {};
template <class PixFmt, class WrapX, class WrapY> struct image_accessor_wrap { explicit image_accessor_wrap(PixFmt&) {} };
template <class Tr = trans_affine> struct span_interpolator_linear { explicit span_interpolator_linear(Tr&) {} };
template <class C> struct span_allocator {};
template <class Src, class Interp> struct span_image_filter_rgb_bilinear { span_image_filter_rgb_bilinear(Src&, Interp&) {} };

}  // namespace agg

#endif
