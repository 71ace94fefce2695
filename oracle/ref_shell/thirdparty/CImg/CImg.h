// TEST INFRASTRUCTURE -- container shell of CImg, written for this repository so
// that the reference's WarpFields.cpp and DataGenerator.cpp compile WITHOUT the
// real library (make -C oracle ref).  CImg<T> here is a plain w x h x d x s array
// with CImg's memory layout, offset = x + w*(y + h*(z + d*c)).  Real: storage,
// operator(), fill, get_crop, resize(w,h,d,s) of an empty image, and the two
// bilinear accessors the reference calls (linear_atXY / _linear_atXY, from CImg
// 2.x's published definition).  Every image-PROCESSING member (shift, rotate,
// crop in place, interpolating resize, permute_axes, draw_image, load, save) does
// nothing: textures and frames of a harness built on this header are meaningless.
#ifndef OFDG_REF_SHELL_CIMG_H_
#define OFDG_REF_SHELL_CIMG_H_

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#define cimg_forX(img, x) for (int x = 0; x < (img).width(); ++x)
#define cimg_forY(img, y) for (int y = 0; y < (img).height(); ++y)
#define cimg_forC(img, c) for (int c = 0; c < (img).spectrum(); ++c)
#define cimg_forXY(img, x, y) cimg_forY(img, y) cimg_forX(img, x)
#define cimg_forXYC(img, x, y, c) cimg_forC(img, c) cimg_forXY(img, x, y)

namespace cimg_library {

template <typename T>
class CImg {
 public:
  CImg() : w_(0), h_(0), d_(0), s_(0), ext_(NULL) {}
  CImg(int w, int h, int d = 1, int s = 1) : ext_(NULL) { assign(w, h, d, s); }
  // view of (or copy of) caller-owned memory; shared == true keeps the pointer
  CImg(T* values, int w, int h, int d, int s, bool shared) : w_(w), h_(h), d_(d), s_(s), ext_(NULL) {
    if (shared) ext_ = values;
    else own_.assign(values, values + size());
  }
  CImg(const CImg& o) : w_(o.w_), h_(o.h_), d_(o.d_), s_(o.s_), own_(o.data(), o.data() + o.size()), ext_(NULL) {}
  CImg(CImg&& o) : w_(o.w_), h_(o.h_), d_(o.d_), s_(o.s_), own_(std::move(o.own_)), ext_(o.ext_) { o.w_ = o.h_ = o.d_ = o.s_ = 0; o.ext_ = NULL; }
  CImg& operator=(CImg o) {
    std::swap(w_, o.w_); std::swap(h_, o.h_); std::swap(d_, o.d_); std::swap(s_, o.s_);
    own_.swap(o.own_); std::swap(ext_, o.ext_);
    return *this;
  }

  CImg& assign(int w, int h, int d, int s) {
    w_ = w; h_ = h; d_ = d; s_ = s; ext_ = NULL;
    own_.assign(size(), T());
    return *this;
  }
  int width() const { return w_; }
  int height() const { return h_; }
  int depth() const { return d_; }
  int spectrum() const { return s_; }
  size_t size() const { return (size_t)w_ * h_ * d_ * s_; }
  bool is_empty() const { return size() == 0; }
  T* data() { return ext_ ? ext_ : own_.data(); }
  const T* data() const { return ext_ ? ext_ : own_.data(); }
  size_t offset(int x, int y, int z, int c) const { return x + (size_t)w_ * (y + (size_t)h_ * (z + (size_t)d_ * c)); }
  T& operator()(unsigned x, unsigned y = 0, unsigned z = 0, unsigned c = 0) { return data()[offset(x, y, z, c)]; }
  const T& operator()(unsigned x, unsigned y = 0, unsigned z = 0, unsigned c = 0) const { return data()[offset(x, y, z, c)]; }

  CImg& fill(const T& v) { for (size_t i = 0, n = size(); i < n; ++i) data()[i] = v; return *this; }
  // resize without interpolation argument: the reference calls it on empty images only (a zeroed allocation)
  CImg& resize(int w, int h, int d, int s) {
    if (w == w_ && h == h_ && d == d_ && s == s_) return *this;
    return assign(w, h, d, s);
  }
  // sub-image [x0,x1] x [y0,y1], all z and c; texels outside the image are 0 (Dirichlet, CImg's default)
  CImg get_crop(int x0, int y0, int x1, int y1) const {
    CImg r(x1 - x0 + 1, y1 - y0 + 1, d_, s_);
    for (int c = 0; c < s_; ++c) for (int z = 0; z < d_; ++z)
      for (int y = y0; y <= y1; ++y) for (int x = x0; x <= x1; ++x)
        if (x >= 0 && y >= 0 && x < w_ && y < h_) r(x - x0, y - y0, z, c) = (*this)(x, y, z, c);
    return r;
  }

  // bilinear, Neumann boundary (coordinates clamped to the image).  NOTE the third parameter is z.
  float _linear_atXY(float fx, float fy, int z = 0, int c = 0) const {
    const float nfx = fx <= 0 ? 0 : (fx >= w_ - 1 ? (float)(w_ - 1) : fx);
    const float nfy = fy <= 0 ? 0 : (fy >= h_ - 1 ? (float)(h_ - 1) : fy);
    const unsigned int x = (unsigned int)nfx, y = (unsigned int)nfy;
    const float dx = nfx - x, dy = nfy - y;
    const unsigned int nx = dx > 0 ? x + 1 : x, ny = dy > 0 ? y + 1 : y;
    const float Icc = (float)(*this)(x, y, z, c), Inc = (float)(*this)(nx, y, z, c);
    const float Icn = (float)(*this)(x, ny, z, c), Inn = (float)(*this)(nx, ny, z, c);
    return Icc + dx * (Inc - Icc + dy * (Icc + Inn - Icn - Inc)) + dy * (Icn - Icc);
  }
  float linear_atXY(float fx, float fy, int z = 0, int c = 0) const { return _linear_atXY(fx, fy, z, c); }
  // bilinear, Dirichlet boundary (out_value outside)
  float linear_atXY(float fx, float fy, int z, int c, const T& out_value) const {
    const int x = (int)fx - (fx >= 0 ? 0 : 1), nx = x + 1, y = (int)fy - (fy >= 0 ? 0 : 1), ny = y + 1;
    const float dx = fx - x, dy = fy - y;
    const float Icc = at(x, y, z, c, out_value), Inc = at(nx, y, z, c, out_value);
    const float Icn = at(x, ny, z, c, out_value), Inn = at(nx, ny, z, c, out_value);
    return Icc + dx * (Inc - Icc + dy * (Icc + Inn - Icn - Inc)) + dy * (Icn - Icc);
  }

  // ---- names only: no image processing happens here ----
  CImg get_shift(int, int = 0, int = 0, int = 0, int = 0) const { return *this; }
  CImg& rotate(float, int = 1, int = 0) { return *this; }
  CImg& crop(int, int, int, int, int = 0) { return *this; }
  CImg& resize(int, int, int, int, int) { return *this; }
  CImg& permute_axes(const char*) { return *this; }
  CImg get_permute_axes(const char*) const { return *this; }
  CImg& load(const char*) { return *this; }
  const CImg& save(const char*) const { return *this; }
  template <typename S, typename M> CImg& draw_image(int, int, const CImg<S>&, const CImg<M>&, float = 1, float = 1) { return *this; }
  CImg& operator*=(double) { return *this; }

 private:
  float at(int x, int y, int z, int c, const T& out_value) const {
    return (x < 0 || y < 0 || x >= w_ || y >= h_) ? (float)out_value : (float)(*this)(x, y, z, c);
  }
  int w_, h_, d_, s_;
  std::vector<T> own_;
  T* ext_;
};

}  // namespace cimg_library

#endif
