// C-ABI wrappers of the host-side pieces that never touch the GPU (declared in include/ofdg.h): no HIP header here.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <exception>
#include <memory>
#include <type_traits>
#include <vector>

#include "host_input.h"
#include "realize.h"
#include "sampler_ref.h"

using namespace ofdg;

struct ofdg_host_sampler {
  RefSampler s;
  ofdg_host_sampler(int m, int w, int h, int n) : s(m, w, h, n) {}
};
thread_local std::string ofdg::g_host_error;

// How a host twin opens: the job's own width and height against the plane size given, the plane-size rule, then the rules the
// twin shares with its device entry (arg_error(j, n, width, height): a function, or a lambda where the twin has rules of its
// own in front).  pair_rule: does the twin refuse a job with one of width and height 0 before it compares them?  (Eight twins
// do not; such a job is refused by the comparison.)  -> false with ofdg_host_last_error set.
template <typename Job, typename Rules>
static bool host_open(const char* who, const Job* j, int n, int width, int height, bool pair_rule, Rules arg_error) {
  const char* why = !j ? "job is NULL" : pair_rule && (j->width == 0) != (j->height == 0) ? kPlanePairRule
                        : (j->width != 0 || j->height != 0) && (j->width != width || j->height != height)
                        ? "width and height of the job must be 0, 0 or the plane size given" : nullptr;
  if (!why) why = plane_size_error(width, height);
  if (!why) why = arg_error(j, n, width, height);
  if (why) g_host_error = std::string(who) + ": " + why;
  return !why;
}
// Record i of a job as it is used: the caller's when recs is given, else draw(global index), then sanitised.  Bytes are moved
// with memcpy, so no alignment is asked.  record_out: ... and handed back when recs_out is given.
template <typename Job, typename Draw, typename Sanitise>
static auto record_of(const Job* j, int i, Draw draw, Sanitise sanitise) {
  std::remove_const_t<std::remove_pointer_t<decltype(j->recs)>> r;
  if (j->recs) std::memcpy(&r, reinterpret_cast<const uint8_t*>(j->recs) + sizeof(r) * (size_t)i, sizeof(r));
  else r = draw((unsigned long long)(j->first_index + i));
  return sanitise(r);
}
template <typename Job, typename Rec>
static void record_out(const Job* j, int i, const Rec& r) {
  if (j->recs_out) std::memcpy(reinterpret_cast<uint8_t*>(j->recs_out) + sizeof(r) * (size_t)i, &r, sizeof(r));
}

// An ofdg_X_draw entry whose draw reads nothing but the job: its ranges checked, then the record of global sample `index`.
// (crop and erase take a frame size, spatial and lens the job's own: those four are written out.)
template <typename Dev, typename Rec, typename Job, typename Out>
static int draw_entry(const char* who, const char* (*ranges_error)(const Dev&), Rec (*draw)(uint32_t, unsigned long long, const Dev&), uint32_t seed,
                      long long index, const Job* ranges, Out* out) {
  static_assert(sizeof(Dev) == sizeof(Job) && sizeof(Rec) == sizeof(Out), "the public structs, restated");
  if (!ranges || !out) { g_host_error = std::string(who) + ": ranges or out is NULL"; return OFDG_EINVAL; }
  Dev j;
  std::memcpy(&j, ranges, sizeof(j));
  if (const char* why = ranges_error(j)) { g_host_error = std::string(who) + ": " + why; return OFDG_EINVAL; }
  const Rec r = draw(seed, (unsigned long long)index, j);
  std::memcpy(out, &r, sizeof(r));
  return OFDG_OK;
}

extern "C" {

void ofdg_default_params(ofdg_params* p) {
  std::memset(p, 0, sizeof(*p));
  p->width = 512;               // DGEN_WIDTH
  p->height = 384;              // DGEN_HEIGHT
  p->mode = 1;                  // caffe.proto:7
  p->use_antialiasing = 1;      // caffe.proto:11
  p->batch_size = 1;
  p->prefetch = 1;
  p->first_level_threads = 16;  // caffe.proto:9
  p->second_level_threads = 1;  // caffe.proto:10
  p->sampler = OFDG_SAMPLER_REF;
  p->world_size = 1;
}

const char* ofdg_host_last_error(void) { return g_host_error.c_str(); }

int ofdg_host_decode_image(const char* path, uint8_t* planar_bgr, size_t capacity, int* width, int* height) {
  if (!path || !width || !height) return OFDG_EINVAL;
  try {
    std::vector<uint8_t> img;
    std::string why;
    if (!read_image(path, planar_bgr ? &img : nullptr, width, height, &why)) { g_host_error = std::string("cannot read ") + path + ": " + why; return OFDG_ETEXTURES; }
    if (planar_bgr) {
      if (img.size() > capacity) { g_host_error = "image buffer too small"; return OFDG_ECAPACITY; }
      std::memcpy(planar_bgr, img.data(), img.size());
    }
    return OFDG_OK;
  } catch (const std::exception& e) {
    g_host_error = e.what();
    return OFDG_ETEXTURES;
  }
}

int ofdg_host_sampler_create(int mode, int width, int height, int num_objects, ofdg_host_sampler** out) {
  if (!out) return OFDG_EINVAL;
  *out = nullptr;
  std::unique_ptr<ofdg_host_sampler> s(new ofdg_host_sampler(mode, width, height, num_objects));
  if (!s->s.ok()) { g_host_error = "BAD MODE"; return OFDG_EBADMODE; }
  *out = s.release();
  return OFDG_OK;
}
void ofdg_host_sampler_destroy(ofdg_host_sampler* s) { delete s; }
int ofdg_host_sampler_next(ofdg_host_sampler* s, int n_tasks, ofdg_task* tasks, ofdg_blueprint* bps, int cap, int* n_bps) {
  if (!s || !tasks || !bps || !n_bps) return OFDG_EINVAL;
  std::vector<ofdg_blueprint> pool;
  for (int i = 0; i < n_tasks; ++i) {
    int rc = s->s.next_task(&pool, &tasks[i], &g_host_error);
    if (rc != OFDG_OK) return rc;
  }
  *n_bps = (int)pool.size();
  if ((int)pool.size() > cap) { g_host_error = "blueprint capacity exceeded"; return OFDG_ECAPACITY; }
  std::memcpy(bps, pool.data(), pool.size() * sizeof(ofdg_blueprint));
  return OFDG_OK;
}

int ofdg_host_realize(const ofdg_params* prm, int pool_n, int pool_w, int pool_h, const ofdg_task* tasks, int n_tasks,
                      const ofdg_blueprint* bps, int n_bps, double* shape_mats, int shape_cap, int* n_shapes,
                      double* object_mats, int object_cap, int* n_objects) {
  if (!prm || !tasks || !bps || !n_shapes || !n_objects) return OFDG_EINVAL;
  RealizeConfig cfg{prm->width, prm->height, prm->mode, pool_n, pool_w, pool_h};
  RealizedBatch b;
  int rc = realize_batch(cfg, tasks, n_tasks, bps, n_bps, &b, &g_host_error);
  if (rc != OFDG_OK) return rc;
  *n_shapes = (int)b.shapes.size();
  *n_objects = (int)b.objects.size();
  if ((int)b.shapes.size() > shape_cap || (int)b.objects.size() > object_cap) { g_host_error = "capacity"; return OFDG_ECAPACITY; }
  for (size_t i = 0; i < b.shapes.size() && shape_mats; ++i) std::memcpy(shape_mats + 12 * i, b.shapes[i].m, sizeof(double) * 12);
  for (size_t i = 0; i < b.objects.size() && object_mats; ++i) {
    std::memcpy(object_mats + 12 * i, &b.objects[i].motion, sizeof(double) * 6);
    std::memcpy(object_mats + 12 * i + 6, &b.objects[i].tex_inv, sizeof(double) * 6);
  }
  return OFDG_OK;
}

int ofdg_parse_prototxt(const char* text, ofdg_params* out, char* texture_dbases, int cap, int* n_top) {
  if (!text || !out) return OFDG_EINVAL;
  try {
    LayerConfig cfg = parse_layer_prototxt(text);
    *out = cfg.params;
    if (texture_dbases && cap > 0) {
      std::strncpy(texture_dbases, cfg.texture_dbases.c_str(), (size_t)cap - 1);
      texture_dbases[cap - 1] = 0;
    }
    if (n_top) *n_top = (int)cfg.top.size();
    return OFDG_OK;
  } catch (const std::exception& e) {
    g_host_error = e.what();
    return OFDG_EINVAL;
  }
}

// The background preparation record of getRandomizedCrop(2W, 2H, angle, zoom, shift) on a pool_w x pool_h image
// (host logic, no GPU): f[8] = ca, sa, w2, h2, rw2, rh2, fx, fy; i[6] = x0, y0, cw, ch, shift_x, shift_y.
int ofdg_host_bg_prep(int pool_w, int pool_h, int width, int height, float angle, float zoom, int shift_x, int shift_y, float* f,
                      int* i) {
  if (!f || !i || pool_w < 2 * width || pool_h < 2 * height || !(zoom > 0)) return OFDG_EINVAL;
  const ofdg::DevBgPrep p = ofdg::make_bg_prep_host(pool_w, pool_h, width, height, angle, zoom, shift_x, shift_y, 0);
  f[0] = p.ca; f[1] = p.sa; f[2] = p.w2; f[3] = p.h2; f[4] = p.rw2; f[5] = p.rh2; f[6] = p.fx; f[7] = p.fy;
  i[0] = p.x0; i[1] = p.y0; i[2] = p.cw; i[3] = p.ch; i[4] = p.shx; i[5] = p.shy;
  return OFDG_OK;
}

// ofdg_object_table's reduction on host label planes (no GPU): areas and boxes of the visible pixels of each label.
int ofdg_host_object_table(const uint8_t* label0, const uint8_t* label1, int n, int width, int height, const int32_t* counts,
                           ofdg_object_row* rows, int rows_per_sample) {
  if (!counts || !rows || n < 1 || width < 1 || height < 1 || rows_per_sample < 1) {
    g_host_error = "ofdg_host_object_table: counts / rows NULL, or n, width, height or rows_per_sample below 1";
    return OFDG_EINVAL;
  }
  const size_t plane = (size_t)width * height;
  for (int s = 0; s < n; ++s) {
    ofdg_object_row* const r = rows + (size_t)s * rows_per_sample;
    const int limit = std::min(std::max(counts[s], 0), rows_per_sample);
    for (int f = 0; f < 2; ++f) {
      const uint8_t* const lab = f ? label1 : label0;
      for (int k = 0; k < limit; ++k) {
        int32_t* const box = f ? r[k].box1 : r[k].box0;
        (f ? r[k].area1 : r[k].area0) = 0;
        box[0] = width; box[1] = height; box[2] = -1; box[3] = -1;
      }
      if (!lab) continue;
      const uint8_t* px = lab + (size_t)s * plane;
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x, ++px) {
          const int k = *px;
          if (k >= limit) continue;  // (no label of this sample, or a row the table does not hold)
          int32_t* const box = f ? r[k].box1 : r[k].box0;
          ++(f ? r[k].area1 : r[k].area0);
          box[0] = std::min(box[0], x); box[1] = std::min(box[1], y);
          box[2] = std::max(box[2], x); box[3] = std::max(box[3], y);
        }
    }
  }
  return OFDG_OK;
}

// ofdg_flow_stats on host buffers (no GPU): the definition of include/ofdg.h pixel by pixel.  This file is compiled with
// -ffp-contract=off, so m2 is two products and one sum, each rounded to float32.
static float half_bits_to_float(uint16_t h) {  // binary16 -> float32, exact
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
  uint32_t bits;
  if (e == 31u) bits = sign | 0x7F800000u | (m << 13);
  else if (e != 0u) bits = sign | ((e + 112u) << 23) | (m << 13);
  else if (m == 0u) bits = sign;
  else {  // subnormal: m * 2^-24
    float f = (float)m * 5.9604644775390625e-8f;
    std::memcpy(&bits, &f, 4);
    bits |= sign;
  }
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}
// How the host twins read a caller's plane: element by element through memcpy, so no alignment is asked of it.
struct FlowPlane {  // binary16 or float32, widened to float32
  const void* p;
  int fmt;
  float at(size_t i) const {
    if (fmt == OFDG_FMT_F16) {
      uint16_t h;
      std::memcpy(&h, static_cast<const uint8_t*>(p) + 2 * i, 2);
      return half_bits_to_float(h);
    }
    float f;
    std::memcpy(&f, static_cast<const uint8_t*>(p) + 4 * i, 4);
    return f;
  }
};
struct OccPlane {  // uint8 or float32: is the element non-zero?
  const void* p;
  int fmt;
  bool at(size_t i) const {
    if (fmt == OFDG_FMT_U8) return static_cast<const uint8_t*>(p)[i] != 0;
    float f;
    std::memcpy(&f, static_cast<const uint8_t*>(p) + 4 * i, 4);
    return f != 0.0f;
  }
};
int ofdg_host_flow_stats(const void* flow, int flow_fmt, const void* occ, int occ_fmt, int n, int width, int height, float bin_px,
                         int flags, ofdg_flow_stats_row* rows) {
  if (const char* why = flow_stats_arg_error(flow, flow_fmt, occ, occ_fmt, n, width, height, bin_px, flags, rows)) {
    g_host_error = std::string("ofdg_host_flow_stats: ") + why;
    return OFDG_EINVAL;
  }
  const bool one_row = flags & OFDG_STATS_ONE_ROW, visible_only = flags & OFDG_STATS_VISIBLE_ONLY;
  if (!(flags & OFDG_STATS_ACCUMULATE)) std::memset(rows, 0, sizeof(ofdg_flow_stats_row) * (one_row ? 1 : (size_t)n));
  float edge2[OFDG_FLOW_HIST_BINS];
  for (int k = 0; k < OFDG_FLOW_HIST_BINS; ++k) {
    const float e = (float)k * bin_px;
    edge2[k] = e * e;
  }
  const size_t plane = (size_t)width * height;
  const FlowPlane fl{flow, flow_fmt};
  const OccPlane hidden{occ, occ_fmt};
  for (int s = 0; s < n; ++s) {
    ofdg_flow_stats_row& r = rows[one_row ? 0 : s];
    for (size_t p = 0; p < plane; ++p) {
      if (occ && hidden.at((size_t)s * plane + p)) {
        ++r.n_occluded;
        if (visible_only) continue;
      }
      const float u = fl.at((size_t)s * 2 * plane + p), v = fl.at(((size_t)s * 2 + 1) * plane + p);
      if (!(std::fabs(u) < 1048576.0f && std::fabs(v) < 1048576.0f)) { ++r.n_bad; continue; }
      ++r.n_counted;
      const float uu = u * u, vv = v * v, m2 = uu + vv;
      int b = 0;
      for (int k = 1; k < OFDG_FLOW_HIST_BINS; ++k) b += edge2[k] <= m2;
      ++r.hist[b];
      r.sum_u_q8 += (int64_t)std::rint(u * 256.0f);
      r.sum_v_q8 += (int64_t)std::rint(v * 256.0f);
      r.sum_mag_q8 += (int64_t)std::rint(std::sqrt(m2) * 256.0f);
      uint32_t bits;
      std::memcpy(&bits, &m2, 4);
      const uint32_t idx = (uint32_t)((one_row ? (size_t)s * plane : 0) + p);
      r.max_key = std::max(r.max_key, ((uint64_t)bits << 32) | (uint64_t)(0xFFFFFFFFu - idx));
    }
  }
  return OFDG_OK;
}

// ofdg_flow_pyramid on host buffers (no GPU): the definition of include/ofdg.h cell by cell, level by level - the sums and
// counts of level k are kept and level k + 1 is made of them.  -ffp-contract=off: every sum is its own float32 rounding.
static uint16_t float_to_half_bits(float f) {  // float32 -> binary16, to nearest even, an overflow becomes +-inf
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  x &= 0x7FFFFFFFu;
  if (x > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);
  if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // 65520 and above (inf too)
  if (x >= 0x38800000u) {                                  // a normal half: 2^-14 and above
    x -= 0x38000000u;
    x += 0xFFFu + ((x >> 13) & 1u);
    return (uint16_t)(sign | (x >> 13));
  }
  const int shift = 126 - (int)(x >> 23);  // a subnormal half: units of 2^-24
  if (shift > 24) return sign;
  const uint32_t m = (x & 0x7FFFFFu) | 0x800000u, h = m >> shift, rem = m & ((1u << shift) - 1u), mid = 1u << (shift - 1);
  return (uint16_t)(sign | (h + ((rem > mid || (rem == mid && (h & 1u))) ? 1u : 0u)));
}
int ofdg_host_flow_pyramid(const void* flow, int flow_fmt, const void* occ, int occ_fmt, int n, int width, int height, int flags,
                           const struct ofdg_flow_pyramid* pyr) {
  if (const char* why = flow_pyramid_arg_error(flow, flow_fmt, occ, occ_fmt, n, width, height, flags,
                                               reinterpret_cast<const DevFlowPyramid*>(pyr))) {
    g_host_error = std::string("ofdg_host_flow_pyramid: ") + why;
    return OFDG_EINVAL;
  }
  const size_t plane = (size_t)width * height;
  const FlowPlane fl{flow, flow_fmt};
  const OccPlane hidden{occ, occ_fmt};
  std::vector<float> su(plane), sv(plane), tu, tv;
  std::vector<uint32_t> sc(plane), tc;
  for (int s = 0; s < n; ++s) {
    su.resize(plane); sv.resize(plane); sc.resize(plane);
    for (size_t p = 0; p < plane; ++p) {
      const float u = fl.at((size_t)s * 2 * plane + p), v = fl.at(((size_t)s * 2 + 1) * plane + p);
      const bool usable = std::fabs(u) < 1048576.0f && std::fabs(v) < 1048576.0f && !(occ && hidden.at((size_t)s * plane + p));
      su[p] = usable ? u : 0.0f;
      sv[p] = usable ? v : 0.0f;
      sc[p] = usable ? 1u : 0u;
    }
    for (int k = 1; k <= pyr->levels; ++k) {
      const size_t w = (size_t)(width >> k), h = (size_t)(height >> k), pw = 2 * w;  // pw: the pitch of level k - 1
      const float scale = (flags & OFDG_PYR_SCALE) ? 1.0f / (float)(1 << k) : 1.0f;
      tu.assign(w * h, 0.0f); tv.assign(w * h, 0.0f); tc.assign(w * h, 0u);
      for (size_t Y = 0; Y < h; ++Y)
        for (size_t X = 0; X < w; ++X) {
          const size_t a = 2 * Y * pw + 2 * X, b = a + pw, at = Y * w + X;
          const float ut = su[a] + su[a + 1], ub = su[b] + su[b + 1], vt = sv[a] + sv[a + 1], vb = sv[b] + sv[b + 1];
          const float cu = ut + ub, cv = vt + vb;
          const uint32_t c = sc[a] + sc[a + 1] + sc[b] + sc[b + 1];
          tu[at] = cu; tv[at] = cv; tc[at] = c;
          float mu = 0.0f, mv = 0.0f;
          if (c) {
            const float qu = cu / (float)c, qv = cv / (float)c;
            mu = qu * scale;
            mv = qv * scale;
          }
          const size_t ou = (size_t)s * 2 * w * h + at, ov = ou + w * h;
          if (pyr->out_fmt == OFDG_FMT_F16) {
            uint16_t* const o = static_cast<uint16_t*>(pyr->flow[k - 1]);
            o[ou] = float_to_half_bits(mu);
            o[ov] = float_to_half_bits(mv);
          } else {
            float* const o = static_cast<float*>(pyr->flow[k - 1]);
            o[ou] = mu;
            o[ov] = mv;
          }
          if (pyr->weight[k - 1]) static_cast<uint16_t*>(pyr->weight[k - 1])[(size_t)s * w * h + at] = (uint16_t)c;
        }
      su.swap(tu); sv.swap(tv); sc.swap(tc);
    }
  }
  return OFDG_OK;
}

// ofdg_crop on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The draw, the sanitising and the window
// test are the functions the kernel runs (csrc/ofdg_device.h); elements are moved with memcpy, so no alignment is asked.
int ofdg_crop_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  if (!counter || !key || !out) { g_host_error = "ofdg_crop_philox: counter, key or out is NULL"; return OFDG_EINVAL; }
  const CropWords w = crop_philox(CropWords{counter[0], counter[1], counter[2], counter[3]}, key[0], key[1]);
  out[0] = w.x; out[1] = w.y; out[2] = w.z; out[3] = w.w;
  return OFDG_OK;
}
int ofdg_crop_draw(uint32_t seed, long long index, int width, int height, int crop_w, int crop_h, int flags, ofdg_crop_rec* out) {
  const char* why = !out ? "out is NULL"
                    : crop_w < 1 || crop_w > width ? "crop_w must lie in [1, width]"
                    : crop_h < 1 || crop_h > height ? "crop_h must lie in [1, height]"
                    : (flags & ~(OFDG_CROP_RANDOM_HFLIP | OFDG_CROP_RANDOM_VFLIP | OFDG_CROP_OCC_WINDOW)) ? "flags holds unknown bits" : nullptr;
  if (why) { g_host_error = std::string("ofdg_crop_draw: ") + why; return OFDG_EINVAL; }
  const DevCropRec r = crop_draw_rec(seed, (unsigned long long)index, width, height, crop_w, crop_h, flags);
  *out = ofdg_crop_rec{r.x0, r.y0, r.flags, r.reserved};
  return OFDG_OK;
}
int ofdg_host_crop(const struct ofdg_crop_job* job, int n_samples, int width, int height) {
  const DevCropJob* const j = reinterpret_cast<const DevCropJob*>(job);
  const char* why = (width < 1 || height < 1) ? "width and height must be at least 1" : crop_arg_error(j, n_samples, width, height);
  if (why) { g_host_error = std::string("ofdg_host_crop: ") + why; return OFDG_EINVAL; }
  const int cw = j->crop_w, ch = j->crop_h;
  const size_t frame = (size_t)width * height, window = (size_t)cw * ch;
  for (int i = 0; i < n_samples; ++i) {
    DevCropRec r = record_of(j, i, [&](unsigned long long g) { return crop_draw_rec(j->seed, g, width, height, cw, ch, j->flags); },
                             [&](const DevCropRec& r) { return crop_sanitise(r, width, height, cw, ch); });
    record_out(j, i, r);
    const bool hflip = r.flags & OFDG_CROP_HFLIP, vflip = r.flags & OFDG_CROP_VFLIP;
    for (int k = 0; k < kCropPlanes; ++k) {
      if (!j->src[k]) continue;
      const int C = crop_channels(k), es = crop_elem_bytes(*j, k);
      const bool is_flow = k == OFDG_CROP_FLOW || k == OFDG_CROP_FLOW1, is_occ = k == OFDG_CROP_OCC0 || k == OFDG_CROP_OCC1;
      const FlowPlane fl{(is_occ && (j->flags & OFDG_CROP_OCC_WINDOW)) ? j->src[k - 2] : nullptr, j->flow_fmt};  // (of an occlusion map under the window rule)
      for (int c = 0; c < C; ++c) {
        const uint8_t* const sp = static_cast<const uint8_t*>(j->src[k]) + ((size_t)i * C + c) * frame * es;
        uint8_t* const dp = static_cast<uint8_t*>(j->dst[k]) + ((size_t)i * C + c) * window * es;
        const bool negate = is_flow && (c == 0 ? hflip : vflip);
        for (int Y = 0; Y < ch; ++Y)
          for (int X = 0; X < cw; ++X) {
            const int xs = r.x0 + (hflip ? cw - 1 - X : X), ys = r.y0 + (vflip ? ch - 1 - Y : Y);
            const size_t at = (size_t)ys * width + xs;
            uint8_t e[4];
            std::memcpy(e, sp + at * es, es);
            if (negate) e[es - 1] ^= 0x80u;  // (little-endian: the sign bit is in the element's last byte)
            if (fl.p) {
              const float u = fl.at((size_t)i * 2 * frame + at), v = fl.at(((size_t)i * 2 + 1) * frame + at);
              const bool inside = crop_target_inside(xs, u, r.x0, cw) && crop_target_inside(ys, v, r.y0, ch);
              if (OccPlane{e, j->occ_fmt}.at(0) || !inside) {
                const float one = 1.0f;
                if (es == 4) std::memcpy(e, &one, 4);
                else e[0] = 1;
              }
            }
            std::memcpy(dp + ((size_t)Y * cw + X) * es, e, es);
          }
      }
    }
  }
  return OFDG_OK;
}

// ofdg_photo on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The draw, the sanitising, the table
// entry, the index and the noise are the functions the kernel runs (csrc/ofdg_device.h); elements are moved with memcpy.
static void photo_table_of(const DevPhotoRec& r, float* table) {
  for (int f = 0; f < 2; ++f)
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < 256; ++k) table[(f * 3 + c) * 256 + k] = photo_table_entry(r.gamma[f], r.gain[f][c], r.contrast[f], r.brightness[f], k);
}
int ofdg_host_det_log(const double* x, int n, double* log_out) {
  if (n < 0 || (n > 0 && (!x || !log_out))) { g_host_error = "ofdg_host_det_log: x or log_out is NULL, or n below 0"; return OFDG_EINVAL; }
  for (int i = 0; i < n; ++i) log_out[i] = ofdg_det_log(x[i]);
  return OFDG_OK;
}
int ofdg_host_photo_table(const ofdg_photo_rec* rec, float* table) {
  if (!rec || !table) { g_host_error = "ofdg_host_photo_table: rec or table is NULL"; return OFDG_EINVAL; }
  DevPhotoRec r;
  std::memcpy(&r, rec, sizeof(r));
  photo_table_of(photo_sanitise(r), table);
  return OFDG_OK;
}
int ofdg_photo_draw(uint32_t seed, long long index, const struct ofdg_photo_job* ranges, ofdg_photo_rec* out) {
  return draw_entry("ofdg_photo_draw", photo_ranges_error, photo_draw_rec, seed, index, ranges, out);
}
int ofdg_host_photo(const struct ofdg_photo_job* job, int n_samples, int width, int height) {
  const DevPhotoJob* const j = reinterpret_cast<const DevPhotoJob*>(job);
  if (!host_open("ofdg_host_photo", j, n_samples, width, height, /*pair_rule=*/false, photo_arg_error)) return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  const int ses = fmt_elem_bytes(j->src_fmt), des = fmt_elem_bytes(j->dst_fmt);
  std::vector<float> table(2 * 3 * 256);
  for (int i = 0; i < n_samples; ++i) {
    const unsigned long long g = (unsigned long long)(j->first_index + i);
    DevPhotoRec r = record_of(j, i, [&](unsigned long long g) { return photo_draw_rec(j->seed, g, *j); }, photo_sanitise);
    record_out(j, i, r);
    photo_table_of(r, table.data());
    const uint32_t k0 = j->seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
    for (int f = 0; f < 2; ++f) {
      if (!j->src[f]) continue;
      const bool noisy = r.sigma[f] > 0.0f;
      const float scale = photo_noise_scale(r.sigma[f]);
      for (int c = 0; c < 3; ++c) {
        const uint8_t* const sp = static_cast<const uint8_t*>(j->src[f]) + ((size_t)i * 3 + c) * plane * ses;
        uint8_t* const dp = static_cast<uint8_t*>(j->dst[f]) + ((size_t)i * 3 + c) * plane * des;
        const float* const T = table.data() + (f * 3 + c) * 256;
        CropWords block{0u, 0u, 0u, 0u};
        for (size_t p = 0; p < plane; ++p) {
          int k = sp[p];
          if (ses == 4) {
            float e;
            std::memcpy(&e, sp + 4 * p, 4);
            k = photo_index(e);
          }
          float v = T[k];
          if (noisy) {
            const uint32_t m = (uint32_t)((size_t)c * plane + p);
            if ((m & 3u) == 0u || p == 0) block = crop_philox(CropWords{m >> 2, (uint32_t)f, 0x0c72u, 0u}, k0, k1);
            const uint32_t word = (m & 3u) == 0u ? block.x : (m & 3u) == 1u ? block.y : (m & 3u) == 2u ? block.z : block.w;
            v = photo_add_noise(v, scale, word);
          }
          if (des == 4) std::memcpy(dp + 4 * p, &v, 4);
          else dp[p] = (uint8_t)rintf(v);
        }
      }
    }
  }
  return OFDG_OK;
}

// ofdg_spatial on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The draw, the sanitising, the
// inverse, the tap, the blend, the flow's transform and the occlusion rule are the functions the kernel runs
// (csrc/ofdg_device.h); elements are moved with memcpy, so no alignment is asked.
int ofdg_spatial_draw(uint32_t seed, long long index, const struct ofdg_spatial_job* ranges, ofdg_spatial_rec* out) {
  if (!ranges || !out) { g_host_error = "ofdg_spatial_draw: ranges or out is NULL"; return OFDG_EINVAL; }
  DevSpatialJob j;
  std::memcpy(&j, ranges, sizeof(j));
  int W = 0, H = 0;
  const char* why = j.width == 0 && j.height == 0 ? "width and height must be set" : spatial_plane_size(j, &W, &H);
  if (!why) why = spatial_draw_error(j);
  if (why) { g_host_error = std::string("ofdg_spatial_draw: ") + why; return OFDG_EINVAL; }
  const DevSpatialRec r = spatial_draw_rec(seed, (unsigned long long)index, j, W, H);
  std::memcpy(out, &r, sizeof(r));
  return OFDG_OK;
}
struct SpatialElems {  // a plane's elements widened to float32: float32, binary16 or uint8
  const uint8_t* p;
  int es;
  bool half;
  float at(size_t i) const {
    if (es == 1) return (float)p[i];
    if (half) return FlowPlane{p, OFDG_FMT_F16}.at(i);
    float f;
    std::memcpy(&f, p + 4 * i, 4);
    return f;
  }
};
int ofdg_host_spatial(const struct ofdg_spatial_job* job, int n_samples, int width, int height) {
  const DevSpatialJob* const j = reinterpret_cast<const DevSpatialJob*>(job);
  if (!host_open("ofdg_host_spatial", j, n_samples, width, height, /*pair_rule=*/false, [](const auto* j, int n, int width, int height) -> const char* {
    if (width > kSpatialMaxSide || height > kSpatialMaxSide) return "width and height must not exceed 2^20";
    return spatial_arg_error(j, n, width, height);
  })) return OFDG_EINVAL;
  const int W = width, H = height, ow = j->out_w, oh = j->out_h;
  const size_t frame = (size_t)W * H, window = (size_t)ow * oh;
  const bool occ_window = j->flags & OFDG_SPATIAL_OCC_WINDOW;
  const int ies = fmt_elem_bytes(j->image_fmt), fes = fmt_elem_bytes(j->flow_fmt), oes = fmt_elem_bytes(j->occ_fmt);
  for (int i = 0; i < n_samples; ++i) {
    DevSpatialRec r = record_of(j, i, [&](unsigned long long g) { return spatial_draw_rec(j->seed, g, *j, W, H); },
                             [&](const DevSpatialRec& r) { return spatial_sanitise(r, W, H, ow, oh); });
    record_out(j, i, r);
    for (int f = 0; f < 2; ++f) {
      const double* const m = r.m[f];
      const SpatialInv other = spatial_inverse(r.m[1 - f]);
      const void* const s_img = j->src[OFDG_CROP_IMAGE0 + f];
      const void* const s_flow = j->src[OFDG_CROP_FLOW + f];
      const void* const s_occ = j->src[OFDG_CROP_OCC0 + f];
      const void* const s_lab = j->src[OFDG_CROP_LABEL0 + f];
      uint8_t* const d_img = static_cast<uint8_t*>(j->dst[OFDG_CROP_IMAGE0 + f]);
      uint8_t* const d_flow = static_cast<uint8_t*>(j->dst[OFDG_CROP_FLOW + f]);
      uint8_t* const d_occ = static_cast<uint8_t*>(j->dst[OFDG_CROP_OCC0 + f]);
      uint8_t* const d_lab = static_cast<uint8_t*>(j->dst[OFDG_CROP_LABEL0 + f]);
      if (!s_img && !s_flow && !s_occ && !s_lab) continue;
      const SpatialElems img{static_cast<const uint8_t*>(s_img), ies, false};
      const SpatialElems flow{static_cast<const uint8_t*>(s_flow), fes, fes == 2};
      for (int Y = 0; Y < oh; ++Y) {
        const double rowx = spatial_row_term(m[1], Y), rowy = spatial_row_term(m[4], Y);
        for (int X = 0; X < ow; ++X) {
          const double qx = spatial_coord(m[0], X, rowx, m[2]), qy = spatial_coord(m[3], X, rowy, m[5]);
          const int Qx = spatial_fixed(qx), Qy = spatial_fixed(qy);
          const size_t to = (size_t)Y * ow + X;
          const size_t near = (size_t)spatial_clamp((Qy + 128) >> 8, H) * W + spatial_clamp((Qx + 128) >> 8, W);
          if (s_img) {
            const int fx = Qx & 255, fy = Qy & 255;
            const size_t x0 = spatial_clamp(Qx >> 8, W), x1 = spatial_clamp((Qx >> 8) + 1, W);
            const size_t y0 = (size_t)spatial_clamp(Qy >> 8, H) * W, y1 = (size_t)spatial_clamp((Qy >> 8) + 1, H) * W;
            for (int c = 0; c < 3; ++c) {
              const size_t base = ((size_t)i * 3 + c) * frame;
              const float v = spatial_blend(img.at(base + y0 + x0), img.at(base + y0 + x1), img.at(base + y1 + x0), img.at(base + y1 + x1), fx, fy);
              uint8_t* const o = d_img + (((size_t)i * 3 + c) * window + to) * ies;
              if (ies == 4) std::memcpy(o, &v, 4);
              else *o = (uint8_t)spatial_to_byte(v);
            }
          }
          double px = 0.0, py = 0.0;
          if (s_flow) {
            const float u = flow.at((size_t)i * 2 * frame + near), v = flow.at(((size_t)i * 2 + 1) * frame + near);
            spatial_partner(qx, qy, u, v, other, &px, &py);
            const float ou = spatial_flow_of(px, X), ov = spatial_flow_of(py, Y);
            uint8_t* const o0 = d_flow + ((size_t)i * 2 * window + to) * fes;
            uint8_t* const o1 = d_flow + (((size_t)i * 2 + 1) * window + to) * fes;
            if (fes == 4) {
              std::memcpy(o0, &ou, 4);
              std::memcpy(o1, &ov, 4);
            } else {
              const uint16_t hu = (uint16_t)spatial_half_bits(ou), hv = (uint16_t)spatial_half_bits(ov);
              std::memcpy(o0, &hu, 2);
              std::memcpy(o1, &hv, 2);
            }
          }
          if (s_occ) {
            bool hidden = OccPlane{static_cast<const uint8_t*>(s_occ) + ((size_t)i * frame + near) * oes, j->occ_fmt}.at(0);
            hidden = hidden || !spatial_inside(Qx, Qy, W, H);
            if (occ_window) hidden = hidden || !(spatial_partner_inside(px, ow) && spatial_partner_inside(py, oh));
            uint8_t* const o = d_occ + ((size_t)i * window + to) * oes;
            const float one = hidden ? 1.0f : 0.0f;
            if (oes == 4) std::memcpy(o, &one, 4);
            else *o = hidden ? 1 : 0;
          }
          if (s_lab) d_lab[(size_t)i * window + to] = static_cast<const uint8_t*>(s_lab)[(size_t)i * frame + near];
        }
      }
    }
  }
  return OFDG_OK;
}

// ofdg_lens on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The draw, the sanitising, the set-up,
// the forward map, the inverse and the vignette are the functions the kernel runs (csrc/ofdg_device.h), the taps and the
// blend the spatial augmentation's; elements are moved with memcpy, so no alignment is asked.
int ofdg_lens_draw(uint32_t seed, long long index, const struct ofdg_lens_job* ranges, ofdg_lens_rec* out) {
  if (!ranges || !out) { g_host_error = "ofdg_lens_draw: ranges or out is NULL"; return OFDG_EINVAL; }
  DevLensJob j;
  std::memcpy(&j, ranges, sizeof(j));
  int W = 0, H = 0;
  const char* why = j.width == 0 && j.height == 0 ? "width and height must be set" : lens_plane_size(j, &W, &H);
  if (!why) why = lens_draw_error(j);
  if (why) { g_host_error = std::string("ofdg_lens_draw: ") + why; return OFDG_EINVAL; }
  const DevLensRec r = lens_draw_rec(seed, (unsigned long long)index, j, W, H);
  std::memcpy(out, &r, sizeof(r));
  return OFDG_OK;
}
int ofdg_host_lens(const struct ofdg_lens_job* job, int n_samples, int width, int height) {
  const DevLensJob* const j = reinterpret_cast<const DevLensJob*>(job);
  if (!host_open("ofdg_host_lens", j, n_samples, width, height, /*pair_rule=*/false, [](const auto* j, int n, int width, int height) -> const char* {
    if (width > kSpatialMaxSide || height > kSpatialMaxSide) return "width and height must not exceed 2^20";
    if ((unsigned long long)width * (unsigned long long)height >= (1ull << 31)) return "width * height must be below 2^31";
    return lens_arg_error(j, n, width, height);
  })) return OFDG_EINVAL;
  const int W = width, H = height;
  const size_t frame = (size_t)W * H;
  const bool occ_window = j->flags & OFDG_LENS_OCC_WINDOW;
  const int ies = fmt_elem_bytes(j->image_fmt), fes = fmt_elem_bytes(j->flow_fmt), oes = fmt_elem_bytes(j->occ_fmt);
  for (int i = 0; i < n_samples; ++i) {
    DevLensRec r = record_of(j, i, [&](unsigned long long g) { return lens_draw_rec(j->seed, g, *j, W, H); },
                             [&](const DevLensRec& r) { return lens_sanitise(r, W, H); });
    record_out(j, i, r);
    const LensSetup o = lens_setup(r, W, H);
    for (int f = 0; f < 2; ++f) {
      const void* const s_img = j->src[OFDG_CROP_IMAGE0 + f];
      const void* const s_flow = j->src[OFDG_CROP_FLOW + f];
      const void* const s_occ = j->src[OFDG_CROP_OCC0 + f];
      const void* const s_lab = j->src[OFDG_CROP_LABEL0 + f];
      uint8_t* const d_img = static_cast<uint8_t*>(j->dst[OFDG_CROP_IMAGE0 + f]);
      uint8_t* const d_flow = static_cast<uint8_t*>(j->dst[OFDG_CROP_FLOW + f]);
      uint8_t* const d_occ = static_cast<uint8_t*>(j->dst[OFDG_CROP_OCC0 + f]);
      uint8_t* const d_lab = static_cast<uint8_t*>(j->dst[OFDG_CROP_LABEL0 + f]);
      if (!s_img && !s_flow && !s_occ && !s_lab) continue;
      const SpatialElems img{static_cast<const uint8_t*>(s_img), ies, false};
      const SpatialElems flow{static_cast<const uint8_t*>(s_flow), fes, fes == 2};
      for (int Y = 0; Y < H; ++Y) {
        const double dy = (double)Y - o.cy;
        for (int X = 0; X < W; ++X) {
          const double dx = (double)X - o.cx;
          const double rho = lens_rho(dx, dy, o.inv);
          const double L = lens_L(o.k1, rho);
          const double qx = lens_coord(o.cx, o.z, L, dx), qy = lens_coord(o.cy, o.z, L, dy);
          const int Qx = spatial_fixed(qx), Qy = spatial_fixed(qy);
          const size_t to = (size_t)Y * W + X;
          const size_t near = (size_t)spatial_clamp((Qy + 128) >> 8, H) * W + spatial_clamp((Qx + 128) >> 8, W);
          if (s_img) {
            const float gain = lens_gain(o.vig, rho);
            for (int c = 0; c < 3; ++c) {
              const double zc = lens_channel_z(o, c);
              const int Cx = spatial_fixed(lens_coord(o.cx, zc, L, dx)), Cy = spatial_fixed(lens_coord(o.cy, zc, L, dy));
              const int fx = Cx & 255, fy = Cy & 255;
              const size_t x0 = spatial_clamp(Cx >> 8, W), x1 = spatial_clamp((Cx >> 8) + 1, W);
              const size_t y0 = (size_t)spatial_clamp(Cy >> 8, H) * W, y1 = (size_t)spatial_clamp((Cy >> 8) + 1, H) * W;
              const size_t base = ((size_t)i * 3 + c) * frame;
              float v = spatial_blend(img.at(base + y0 + x0), img.at(base + y0 + x1), img.at(base + y1 + x0), img.at(base + y1 + x1), fx, fy);
              if (o.vig != 0.0) v = spatial_quiet(v * gain);
              uint8_t* const d = d_img + (base + to) * ies;
              if (ies == 4) std::memcpy(d, &v, 4);
              else *d = (uint8_t)spatial_to_byte(v);
            }
          }
          double px = 0.0, py = 0.0;
          bool solved = true;
          if (s_flow) {
            const float u = flow.at((size_t)i * 2 * frame + near), v = flow.at(((size_t)i * 2 + 1) * frame + near);
            const double tx = qx + (double)u, ty = qy + (double)v;
            solved = lens_inverse(o, tx, ty, &px, &py);
            const float ou = solved ? spatial_flow_of(px, X) : lens_nan(), ov = solved ? spatial_flow_of(py, Y) : lens_nan();
            uint8_t* const o0 = d_flow + ((size_t)i * 2 * frame + to) * fes;
            uint8_t* const o1 = d_flow + (((size_t)i * 2 + 1) * frame + to) * fes;
            if (fes == 4) {
              std::memcpy(o0, &ou, 4);
              std::memcpy(o1, &ov, 4);
            } else {
              const uint16_t hu = (uint16_t)spatial_half_bits(ou), hv = (uint16_t)spatial_half_bits(ov);
              std::memcpy(o0, &hu, 2);
              std::memcpy(o1, &hv, 2);
            }
          }
          if (s_occ) {
            bool hidden = OccPlane{static_cast<const uint8_t*>(s_occ) + ((size_t)i * frame + near) * oes, j->occ_fmt}.at(0);
            hidden = hidden || !spatial_inside(Qx, Qy, W, H) || !solved;
            if (occ_window) hidden = hidden || !(spatial_partner_inside(px, W) && spatial_partner_inside(py, H));
            uint8_t* const d = d_occ + ((size_t)i * frame + to) * oes;
            const float one = hidden ? 1.0f : 0.0f;
            if (oes == 4) std::memcpy(d, &one, 4);
            else *d = hidden ? 1 : 0;
          }
          if (s_lab) d_lab[(size_t)i * frame + to] = static_cast<const uint8_t*>(s_lab)[(size_t)i * frame + near];
        }
      }
    }
  }
  return OFDG_OK;
}

// ofdg_pack on host arrays (no GPU): the definition of include/ofdg.h element by element.  The value, the roundings, the
// placement and the argument rules are the functions the kernel runs (csrc/ofdg_device.h); elements are moved with memcpy,
// so no alignment is asked.
int ofdg_host_pack(const struct ofdg_pack_job* job, int n_samples, int width, int height) {
  const DevPackJob* const j = reinterpret_cast<const DevPackJob*>(job);
  if (!host_open("ofdg_host_pack", j, n_samples, width, height, /*pair_rule=*/true, pack_arg_error)) return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  for (int k = 0; k < kPackPlanes; ++k) {
    if (!j->src[k]) continue;
    const bool flow = k == OFDG_PACK_FLOW;
    const int sfmt = flow ? j->flow_src_fmt : j->image_src_fmt, dfmt = flow ? j->flow_dst_fmt : j->image_dst_fmt;
    const int Cs = flow ? 2 : 3, Cd = pack_channels(k, j->flags), des = fmt_elem_bytes(dfmt);
    const SpatialElems src{static_cast<const uint8_t*>(j->src[k]), fmt_elem_bytes(sfmt), sfmt == OFDG_FMT_F16};
    uint8_t* const dst = static_cast<uint8_t*>(j->dst[(j->flags & OFDG_PACK_CONCAT) && !flow ? OFDG_PACK_IMAGE0 : k]);
    for (int i = 0; i < n_samples; ++i)
      for (int c = 0; c < Cs; ++c) {
        const int cd = flow ? c : pack_dst_channel(k, c, j->flags);
        for (int y = 0; y < height; ++y)
          for (int x = 0; x < width; ++x) {
            const float e = src.at(((size_t)i * Cs + c) * plane + (size_t)y * width + x);
            const float v = flow ? pack_flow_value(e, j->flow_scale) : pack_value(e, j->scale[c], j->bias[c]);
            const uint32_t bits = pack_stored_bits(v, dfmt);
            std::memcpy(dst + pack_dst_index(j->layout, Cd, i, cd, y, x, width, height) * des, &bits, des);
          }
      }
  }
  return OFDG_OK;
}

// ofdg_boundaries on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The pair rule and the argument
// rules are the functions the kernel runs (csrc/ofdg_device.h); the distance is the minimum over the offsets of the disc.
int ofdg_host_boundaries(const struct ofdg_boundary_job* job, int n_samples, int width, int height) {
  const DevBoundaryJob* const j = reinterpret_cast<const DevBoundaryJob*>(job);
  if (!host_open("ofdg_host_boundaries", j, n_samples, width, height, /*pair_rule=*/true, boundary_arg_error)) return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  const bool labels = j->flags & OFDG_BND_LABELS;
  const float t2 = boundary_threshold(j->min_step);
  std::vector<uint8_t> edge(plane);
  for (int f = 0; f < 2; ++f) {
    if (!j->flow[f]) continue;
    const FlowPlane flow{j->flow[f], j->flow_fmt};
    const int R = j->dist2[f] ? j->radius : 0;
    for (int i = 0; i < n_samples; ++i) {
      const size_t fu = (size_t)i * 2 * plane, fv = fu + plane;
      const uint8_t* const lab = labels ? j->label[f] + (size_t)i * plane : nullptr;
      auto step = [&](size_t p, size_t q) {
        if (lab && lab[p] == lab[q]) return false;
        return boundary_step(flow.at(fu + p), flow.at(fv + p), flow.at(fu + q), flow.at(fv + q), t2);
      };
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
          const size_t p = (size_t)y * width + x;
          edge[p] = (x > 0 && step(p, p - 1)) || (x + 1 < width && step(p, p + 1)) || (y > 0 && step(p, p - width)) ||
                    (y + 1 < height && step(p, p + width)) ? 1 : 0;
        }
      if (j->edge[f]) std::memcpy(j->edge[f] + (size_t)i * plane, edge.data(), plane);
      if (!j->dist2[f]) continue;
      uint8_t* const out = j->dist2[f] + (size_t)i * plane;
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
          // every offset of the disc, the near ones first: ay = |dy|, ax = |dx|, both signs of each
          int best = OFDG_BND_FAR;
          for (int ay = 0; ay <= R && ay * ay < best; ++ay)
            for (int ax = 0; ax * ax + ay * ay <= R * R && ax * ax + ay * ay < best; ++ax)
              for (int s = 0; s < 4; ++s) {
                const int px = x + ((s & 1) ? -ax : ax), py = y + ((s & 2) ? -ay : ay);
                if (px < 0 || px >= width || py < 0 || py >= height) continue;
                if (edge[(size_t)py * width + px]) best = ax * ax + ay * ay;
              }
          out[(size_t)y * width + x] = (uint8_t)best;
        }
    }
  }
  return OFDG_OK;
}

// ofdg_erase on host arrays (no GPU): the definition of include/ofdg.h element by element.  The draw, the sanitising, the Q8
// value, the mean byte, the noise byte, the marking rule and the argument rules are the functions the kernels run
// (csrc/ofdg_device.h); elements are moved with memcpy.
int ofdg_erase_draw(uint32_t seed, long long index, int width, int height, const struct ofdg_erase_job* ranges, ofdg_erase_rec* out) {
  const char* why = !ranges || !out ? "ranges or out is NULL" : width < 1 || width > 32768 || height < 1 || height > 32768 ? "width and height must lie in 1..32768" : nullptr;
  DevEraseJob j;
  if (!why) {
    std::memcpy(&j, ranges, sizeof(j));
    why = erase_ranges_error(j);
  }
  if (why) { g_host_error = std::string("ofdg_erase_draw: ") + why; return OFDG_EINVAL; }
  const DevEraseRec r = erase_draw_rec(seed, (unsigned long long)index, width, height, j);
  std::memcpy(out, &r, sizeof(r));
  return OFDG_OK;
}
int ofdg_host_erase(const struct ofdg_erase_job* job, int n_samples, int width, int height) {
  const DevEraseJob* const j = reinterpret_cast<const DevEraseJob*>(job);
  if (!host_open("ofdg_host_erase", j, n_samples, width, height, /*pair_rule=*/true,
                 [](const auto* j, int n, int w, int h) { return erase_arg_error(j, n, w, h, /*with_work=*/false); }))
    return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  const int es = fmt_elem_bytes(j->image_fmt);
  const bool occ = j->flags & OFDG_ERASE_OCC;
  for (int i = 0; i < n_samples; ++i) {
    const unsigned long long g = (unsigned long long)(j->first_index + i);
    DevEraseRec r = record_of(j, i, [&](unsigned long long g) { return erase_draw_rec(j->seed, g, width, height, *j); },
                             [&](const DevEraseRec& r) { return erase_sanitise(r, width, height, j->flags); });
    const int frames = erase_frames_of(r);
    const uint32_t k0 = j->seed ^ (uint32_t)(g >> 32) * 0x9E3779B9u, k1 = (uint32_t)g;
    for (int f = 0; f < 2; ++f) {
      if (!((frames >> f) & 1)) continue;
      uint8_t* const img = static_cast<uint8_t*>(j->image[f]) + (size_t)i * 3 * plane * es;
      for (int c = 0; c < 3; ++c) {  // the fill bytes first: of the frame before any rectangle is painted
        uint32_t m = 0;
        if (j->fill == OFDG_ERASE_CONST) m = (uint32_t)j->color[c];
        else if (j->fill == OFDG_ERASE_MEAN) {
          unsigned long long S = 0;
          for (size_t p = 0; p < plane; ++p) {
            if (es == 1) S += 256u * img[(size_t)c * plane + p];
            else {
              float v;
              std::memcpy(&v, img + 4 * ((size_t)c * plane + p), 4);
              S += erase_q8(v);
            }
          }
          m = erase_mean_byte(S, plane);
        }
        r.fill[f][c] = (uint8_t)m;
      }
      for (int k = 0; k < r.count; ++k) {
        const DevEraseRect& q = r.rect[k];
        if (q.frame != f) continue;
        for (int c = 0; c < 3; ++c)
          for (int y = q.y0; y < q.y0 + q.h; ++y)
            for (int x = q.x0; x < q.x0 + q.w; ++x) {
              const uint32_t e = (uint32_t)((size_t)c * plane + (size_t)y * width + x);
              const uint32_t b = j->fill == OFDG_ERASE_NOISE ? erase_noise_byte(k0, k1, f, e) : r.fill[f][c];
              const float v = (float)b;
              if (es == 1) img[e] = (uint8_t)b;
              else std::memcpy(img + 4 * (size_t)e, &v, 4);
            }
      }
    }
    record_out(j, i, r);
    for (int f = 0; f < 2 && occ; ++f) {
      if (!j->occ[f] || !r.count) continue;
      const bool cross = erase_cross(*j, f);
      const FlowPlane flow{j->flow[f], j->flow_fmt};
      const size_t fu = (size_t)i * 2 * plane, fv = fu + plane;
      uint8_t* const map = static_cast<uint8_t*>(j->occ[f]) + (size_t)i * plane * fmt_elem_bytes(j->occ_fmt);
      const float one = 1.0f;
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
          const size_t p = (size_t)y * width + x;
          const float u = cross ? flow.at(fu + p) : 0.0f, v = cross ? flow.at(fv + p) : 0.0f;
          if (!erase_marks(r, f, cross, x, y, u, v)) continue;
          if (j->occ_fmt == OFDG_FMT_U8) map[p] = 1;
          else std::memcpy(map + 4 * p, &one, 4);
        }
    }
  }
  return OFDG_OK;
}

// ofdg_jitter on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The draw, the sanitising, the order's
// decoding, the operations and the mean are the functions the kernels run (csrc/ofdg_device.h); elements are moved with memcpy.
int ofdg_jitter_draw(uint32_t seed, long long index, const struct ofdg_jitter_job* ranges, ofdg_jitter_rec* out) {
  return draw_entry("ofdg_jitter_draw", jitter_ranges_error, jitter_draw_rec, seed, index, ranges, out);
}
int ofdg_host_jitter_hue(const uint8_t* bgr, uint8_t* out, size_t pixels, int hue) {
  if (!bgr || !out || hue < -kJitterTurn || hue > kJitterTurn) { g_host_error = "ofdg_host_jitter_hue: bgr or out is NULL, or hue outside [-393216, 393216]"; return OFDG_EINVAL; }
  for (size_t k = 0; k < pixels; ++k) {
    int B = bgr[k], G = bgr[pixels + k], R = bgr[2 * pixels + k];
    jitter_hue(B, G, R, hue);
    out[k] = (uint8_t)B; out[pixels + k] = (uint8_t)G; out[2 * pixels + k] = (uint8_t)R;
  }
  return OFDG_OK;
}
int ofdg_host_jitter(const struct ofdg_jitter_job* job, int n_samples, int width, int height) {
  const DevJitterJob* const j = reinterpret_cast<const DevJitterJob*>(job);
  if (!host_open("ofdg_host_jitter", j, n_samples, width, height, /*pair_rule=*/false,
                 [](const auto* j, int n, int w, int h) { return jitter_arg_error(j, n, w, h, /*with_work=*/false); }))
    return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  const int ses = fmt_elem_bytes(j->src_fmt), des = fmt_elem_bytes(j->dst_fmt);
  std::vector<uint8_t> px[2];  // the bytes of a sample's frame, pixel by pixel: B G R
  for (int i = 0; i < n_samples; ++i) {
    DevJitterRec r = record_of(j, i, [&](unsigned long long g) { return jitter_draw_rec(j->seed, g, *j); }, jitter_sanitise);
    unsigned long long S[2] = {0, 0};
    for (int f = 0; f < 2; ++f) {
      if (!j->src[f]) continue;
      const JitterFrame p = jitter_frame(r, f);
      px[f].resize(3 * plane);
      for (int c = 0; c < 3; ++c) {
        const uint8_t* const sp = static_cast<const uint8_t*>(j->src[f]) + ((size_t)i * 3 + c) * plane * ses;
        for (size_t k = 0; k < plane; ++k) {
          int b = sp[k];
          if (ses == 4) {
            float e;
            std::memcpy(&e, sp + 4 * k, 4);
            b = photo_index(e);
          }
          px[f][3 * k + c] = (uint8_t)b;
        }
      }
      if (p.contrast == kJitterOne) continue;
      const uint32_t ops = jitter_ops(p.order);
      const int places = jitter_contrast_place(ops);
      for (size_t k = 0; k < plane; ++k) {
        int B = px[f][3 * k], G = px[f][3 * k + 1], R = px[f][3 * k + 2];
        for (int place = 0; place < places; ++place) jitter_op(jitter_op_at(ops, place), p, 0, B, G, R);
        S[f] += (unsigned long long)jitter_lum(B, G, R);
      }
    }
    const bool joint = r.shared && j->src[0] && j->src[1];
    for (int f = 0; f < 2; ++f) {
      if (!j->src[f]) continue;
      const JitterFrame p = jitter_frame(r, f);
      const int mean = p.contrast == kJitterOne ? -1 : jitter_mean_byte(joint ? S[0] + S[1] : S[f], joint ? 2ull * plane : (unsigned long long)plane);
      r.mean[f] = mean;
      const bool same_fmt = j->src_fmt == j->dst_fmt;
      if (jitter_identity(p) && same_fmt) {  // copied bit for bit; in place: not touched
        if (j->dst[f] != j->src[f])
          std::memmove(static_cast<uint8_t*>(j->dst[f]) + (size_t)i * 3 * plane * des, static_cast<const uint8_t*>(j->src[f]) + (size_t)i * 3 * plane * ses, 3 * plane * ses);
        continue;
      }
      const uint32_t ops = jitter_ops(p.order);
      for (size_t k = 0; k < plane; ++k) {
        int v[3] = {px[f][3 * k], px[f][3 * k + 1], px[f][3 * k + 2]};
        for (int place = 0; place < 4; ++place) jitter_op(jitter_op_at(ops, place), p, mean, v[0], v[1], v[2]);
        for (int c = 0; c < 3; ++c) {
          uint8_t* const dp = static_cast<uint8_t*>(j->dst[f]) + (((size_t)i * 3 + c) * plane + k) * des;
          const float e = (float)v[c];
          if (des == 4) std::memcpy(dp, &e, 4);
          else *dp = (uint8_t)v[c];
        }
      }
    }
    record_out(j, i, r);
  }
  return OFDG_OK;
}

// ofdg_flow_vis on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The usable rule, the Q8 components,
// the roots, the scale, the angle, the wheel and the colour are the functions the kernels run (csrc/ofdg_device.h) on the two
// tables of that header; elements are moved with memcpy.
int ofdg_host_flow_vis_tables(int32_t atan_q24[257], uint8_t wheel_rgb[55][3]) {
  if (!atan_q24 || !wheel_rgb) { g_host_error = "ofdg_host_flow_vis_tables: atan_q24 or wheel_rgb is NULL"; return OFDG_EINVAL; }
  for (int k = 0; k < kVisAtanEntries; ++k) atan_q24[k] = kVisAtan[k];
  for (int k = 0; k < kVisWheelEntries; ++k)
    for (int c = 0; c < 3; ++c) wheel_rgb[k][c] = (uint8_t)(kVisWheel[k] >> (8 * c));
  return OFDG_OK;
}
int ofdg_host_flow_vis(const struct ofdg_flow_vis_job* job, int n_samples, int width, int height) {
  const DevVisJob* const j = reinterpret_cast<const DevVisJob*>(job);
  if (!host_open("ofdg_host_flow_vis", j, n_samples, width, height, /*pair_rule=*/false,
                 [](const auto* j, int n, int w, int h) { return vis_arg_error(j, n, w, h, /*with_work=*/false); }))
    return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  const FlowPlane fl{j->flow, j->flow_fmt};
  const OccPlane hidden{j->occ, j->occ_fmt};
  const bool dim = j->flags & OFDG_VIS_DIM_OCC, hwc = j->layout == OFDG_VIS_HWC_RGB;
  // the largest R2 of each sample's usable pixels, occluded ones included; BATCH: the largest of them all
  std::vector<unsigned long long> max_r2((size_t)n_samples, 0ull);
  if (j->norm != OFDG_VIS_NORM_FIXED) {
    unsigned long long all = 0;
    for (int i = 0; i < n_samples; ++i) {
      for (size_t k = 0; k < plane; ++k) {
        const float u = fl.at((size_t)i * 2 * plane + k), v = fl.at(((size_t)i * 2 + 1) * plane + k);
        if (vis_usable(u, v)) max_r2[i] = std::max(max_r2[i], vis_r2(vis_fixed(u), vis_fixed(v)));
      }
      all = std::max(all, max_r2[i]);
    }
    if (j->norm == OFDG_VIS_NORM_BATCH) std::fill(max_r2.begin(), max_r2.end(), all);
  }
  uint8_t* const dst = static_cast<uint8_t*>(j->dst);
  for (int i = 0; i < n_samples; ++i) {
    const uint32_t M = j->norm == OFDG_VIS_NORM_FIXED ? vis_scale_fixed(j->max_flow) : vis_scale_of(max_r2[i]);
    if (j->rows_out) {
      const DevVisRow row{max_r2[i], M, 0u};
      std::memcpy(reinterpret_cast<uint8_t*>(j->rows_out) + sizeof(row) * (size_t)i, &row, sizeof(row));
    }
    for (size_t k = 0; k < plane; ++k) {
      const float u = fl.at((size_t)i * 2 * plane + k), v = fl.at(((size_t)i * 2 + 1) * plane + k);
      const uint32_t rgb = vis_usable(u, v) ? vis_pixel(u, v, M, vis_inv(M), dim && hidden.at((size_t)i * plane + k), kVisAtan, kVisWheel) : 0u;
      for (int c = 0; c < 3; ++c) {  // c: R, G, B
        const uint8_t byte = (uint8_t)(rgb >> (8 * c));
        if (hwc) dst[((size_t)i * plane + k) * 3 + c] = byte;
        else dst[((size_t)i * 3 + (2 - c)) * plane + k] = byte;
      }
    }
  }
  return OFDG_OK;
}

// ofdg_flow_error on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The usable rule, the Q8
// components, the roots, the cell, the flags, the bins, the key, epe and the colour are the functions the kernel runs
// (csrc/ofdg_device.h); elements are moved with memcpy, the rows are added to field by field.
int ofdg_host_flow_error_colours(uint8_t rgb[10][3]) {
  if (!rgb) { g_host_error = "ofdg_host_flow_error_colours: rgb is NULL"; return OFDG_EINVAL; }
  for (int k = 0; k < kErrColours; ++k)
    for (int c = 0; c < 3; ++c) rgb[k][c] = (uint8_t)(kErrColour[k] >> (8 * c));
  return OFDG_OK;
}
int ofdg_host_flow_error(const struct ofdg_flow_error_job* job, int n_samples, int width, int height) {
  const DevErrJob* const j = reinterpret_cast<const DevErrJob*>(job);
  if (!host_open("ofdg_host_flow_error", j, n_samples, width, height, /*pair_rule=*/false, err_arg_error)) return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  const FlowPlane gt{j->gt, j->gt_fmt}, est_f{j->est, j->est_fmt};
  const auto est = [&](size_t i) {
    if (j->est_fmt != OFDG_FMT_BF16) return est_f.at(i);
    uint16_t h;
    std::memcpy(&h, static_cast<const uint8_t*>(j->est) + 2 * i, 2);
    return err_bf16(h);
  };
  const OccPlane hidden{j->occ, j->occ_fmt};
  const bool one_row = j->flags & OFDG_ERR_ONE_ROW, dim = j->flags & OFDG_ERR_DIM_OCC, hwc = j->layout == OFDG_VIS_HWC_RGB;
  const ErrBands bands = err_bands(*j);
  uint8_t* const rows = reinterpret_cast<uint8_t*>(j->rows);
  if (rows && !(j->flags & OFDG_ERR_ACCUMULATE)) std::memset(rows, 0, sizeof(DevErrRow) * (one_row ? 1 : (size_t)n_samples));
  uint8_t* const picture = static_cast<uint8_t*>(j->picture);
  for (int i = 0; i < n_samples; ++i) {
    DevErrRow row{};
    if (rows) std::memcpy(&row, rows + sizeof(row) * (one_row ? 0 : (size_t)i), sizeof(row));
    for (size_t k = 0; k < plane; ++k) {
      const float ug = gt.at((size_t)i * 2 * plane + k), vg = gt.at(((size_t)i * 2 + 1) * plane + k);
      const float ue = err_scaled(est((size_t)i * 2 * plane + k), j->est_scale), ve = err_scaled(est(((size_t)i * 2 + 1) * plane + k), j->est_scale);
      const bool gt_ok = vis_usable(ug, vg), ok = gt_ok && vis_usable(ue, ve);
      float epe = -1.0f;
      uint32_t rgb = 0u;
      if (!gt_ok) ++row.n_bad[0];
      else if (!ok) ++row.n_bad[1];
      else {
        const ErrPixel e = err_pixel(ug, vg, ue, ve);
        const bool hid = j->occ && hidden.at((size_t)i * plane + k);
        DevErrCell& cell = row.cell[err_cell(hid, e.Gq, j->dist2 ? j->dist2[(size_t)i * plane + k] : 0u, j->dist2 != nullptr, bands)];
        const uint32_t flags = err_flags(e.Eq, e.Gq);
        ++cell.n;
        cell.sum_epe_q8 += e.Eq;
        cell.n_1px += flags & 1u;
        cell.n_3px += (flags >> 1) & 1u;
        cell.n_5px += (flags >> 2) & 1u;
        cell.n_fl += (flags >> 3) & 1u;
        ++row.hist[err_hist_bin(e.Eq)];
        row.max_key = std::max(row.max_key, err_key(e.Eq, (uint32_t)((one_row ? (size_t)i * plane : 0) + k)));
        epe = err_epe(e.Eq);
        rgb = err_colour(e.Eq, e.Gq, dim && hid, kErrColour);
      }
      if (j->epe) {
        if (j->epe_fmt == OFDG_FMT_F16) {
          const uint16_t h = float_to_half_bits(epe);
          std::memcpy(static_cast<uint8_t*>(j->epe) + 2 * ((size_t)i * plane + k), &h, 2);
        } else {
          std::memcpy(static_cast<uint8_t*>(j->epe) + 4 * ((size_t)i * plane + k), &epe, 4);
        }
      }
      if (picture)
        for (int c = 0; c < 3; ++c) {  // c: R, G, B
          const uint8_t byte = (uint8_t)(rgb >> (8 * c));
          if (hwc) picture[((size_t)i * plane + k) * 3 + c] = byte;
          else picture[((size_t)i * 3 + (2 - c)) * plane + k] = byte;
        }
    }
    if (rows) std::memcpy(rows + sizeof(row) * (one_row ? 0 : (size_t)i), &row, sizeof(row));
  }
  return OFDG_OK;
}

// ofdg_camera on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The draw, the sanitising, the tap
// table, the roundings, the sites and the demosaic are the functions the kernel runs (csrc/ofdg_device.h); elements are moved
// with memcpy.
int ofdg_camera_draw(uint32_t seed, long long index, const struct ofdg_camera_job* ranges, ofdg_camera_rec* out) {
  return draw_entry("ofdg_camera_draw", camera_ranges_error, camera_draw_rec, seed, index, ranges, out);
}
int ofdg_camera_taps(int sigma_q8, uint32_t out[13]) {
  if (!out || sigma_q8 < 1 || sigma_q8 > kCameraMaxSigma) { g_host_error = "ofdg_camera_taps: out is NULL, or sigma_q8 outside 1..1024"; return OFDG_EINVAL; }
  uint32_t w[kCameraMaxRadius + 1];
  camera_taps(sigma_q8, camera_radius(sigma_q8), w);
  std::memcpy(out, w, sizeof(w));
  return OFDG_OK;
}
int ofdg_host_camera(const struct ofdg_camera_job* job, int n_samples, int width, int height) {
  const DevCameraJob* const j = reinterpret_cast<const DevCameraJob*>(job);
  if (!host_open("ofdg_host_camera", j, n_samples, width, height, /*pair_rule=*/false, camera_arg_error)) return OFDG_EINVAL;
  const int W = width, H = height;
  const size_t plane = (size_t)W * H;
  const int ses = fmt_elem_bytes(j->src_fmt), des = fmt_elem_bytes(j->dst_fmt);
  std::vector<uint8_t> px[3], out[3];   // the bytes of a sample's frame by channel: blurred, then demosaiced
  std::vector<uint16_t> h8(plane);
  for (int c = 0; c < 3; ++c) { px[c].resize(plane); out[c].resize(plane); }
  for (int i = 0; i < n_samples; ++i) {
    DevCameraRec r = record_of(j, i, [&](unsigned long long g) { return camera_draw_rec(j->seed, g, *j); }, camera_sanitise);
    record_out(j, i, r);
    for (int f = 0; f < 2; ++f) {
      if (!j->src[f]) continue;
      const int s = r.sigma_q8[f], R = r.radius[f], p = r.bayer;
      const uint8_t* const sp = static_cast<const uint8_t*>(j->src[f]) + (size_t)i * 3 * plane * ses;
      uint8_t* const dp = static_cast<uint8_t*>(j->dst[f]) + (size_t)i * 3 * plane * des;
      if (s == 0 && p < 0 && j->src_fmt == j->dst_fmt) {  // copied bit for bit
        std::memcpy(dp, sp, 3 * plane * ses);
        continue;
      }
      uint32_t w[kCameraMaxRadius + 1] = {};
      if (s > 0) camera_taps(s, R, w);
      for (int c = 0; c < 3; ++c) {
        for (size_t k = 0; k < plane; ++k) {
          int b = sp[c * plane + k];
          if (ses == 4) {
            float e;
            std::memcpy(&e, sp + (c * plane + k) * 4, 4);
            b = photo_index(e);
          }
          px[c][k] = (uint8_t)b;
        }
        if (s == 0) continue;
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            uint32_t S = 0;
            for (int k = -R; k <= R; ++k) S += w[k < 0 ? -k : k] * px[c][(size_t)y * W + camera_clamp(x + k, W)];
            h8[(size_t)y * W + x] = (uint16_t)camera_h8(S);
          }
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            uint32_t S = 0;
            for (int k = -R; k <= R; ++k) S += w[k < 0 ? -k : k] * h8[(size_t)camera_clamp(y + k, H) * W + x];
            px[c][(size_t)y * W + x] = (uint8_t)camera_byte(S);
          }
      }
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          uint32_t o[3] = {px[0][(size_t)y * W + x], px[1][(size_t)y * W + x], px[2][(size_t)y * W + x]};
          if (p >= 0) {
            const int a = camera_site_a(x, p), b = camera_site_b(y, p);
            const size_t xm = camera_reflect(x - 1, W), xp = camera_reflect(x + 1, W);
            const size_t ym = (size_t)camera_reflect(y - 1, H) * W, yp = (size_t)camera_reflect(y + 1, H) * W, y0 = (size_t)y * W;
            const uint8_t* const ph = px[camera_site_channel(a ^ 1, b)].data();
            const uint8_t* const pv = px[camera_site_channel(a, b ^ 1)].data();
            const uint8_t* const pd = px[camera_site_channel(a ^ 1, b ^ 1)].data();
            camera_demosaic(a, b, px[camera_site_channel(a, b)][y0 + x], (uint32_t)ph[y0 + xm] + ph[y0 + xp], (uint32_t)pv[ym + x] + pv[yp + x],
                            (uint32_t)pd[ym + xm] + pd[ym + xp] + pd[yp + xm] + pd[yp + xp], o);
          }
          for (int c = 0; c < 3; ++c) out[c][(size_t)y * W + x] = (uint8_t)o[c];
        }
      for (int c = 0; c < 3; ++c)
        for (size_t k = 0; k < plane; ++k) {
          uint8_t* const q = dp + (c * plane + k) * des;
          const float e = (float)out[c][k];
          if (des == 4) std::memcpy(q, &e, 4);
          else *q = out[c][k];
        }
    }
  }
  return OFDG_OK;
}

// ofdg_jpeg on host arrays (no GPU): the definition of include/ofdg.h MCU by MCU.  The draw, the sanitising, the tables, the
// colour transforms, the block's passes and the argument rules are the functions the kernel runs (csrc/ofdg_device.h);
// elements are moved with memcpy.  A frame is read whole before any of it is written, so the in-place form needs no care.
int ofdg_jpeg_draw(uint32_t seed, long long index, const struct ofdg_jpeg_job* ranges, ofdg_jpeg_rec* out) {
  return draw_entry("ofdg_jpeg_draw", jpeg_ranges_error, jpeg_draw_rec, seed, index, ranges, out);
}
int ofdg_jpeg_tables(int quality, uint16_t luma[64], uint16_t chroma[64]) {
  if (!luma || !chroma || quality < 1 || quality > 100) { g_host_error = "ofdg_jpeg_tables: luma or chroma is NULL, or quality outside 1..100"; return OFDG_EINVAL; }
  for (int k = 0; k < 64; ++k) {
    luma[k] = (uint16_t)jpeg_quant(kJpegBaseLuma[k], quality);
    chroma[k] = (uint16_t)jpeg_quant(kJpegBaseChroma[k], quality);
  }
  return OFDG_OK;
}
int ofdg_host_jpeg_block(const uint8_t in[64], const uint16_t q[64], int32_t levels[64], uint8_t out[64]) {
  if (!in || !q || !out) { g_host_error = "ofdg_host_jpeg_block: in, q or out is NULL"; return OFDG_EINVAL; }
  for (int k = 0; k < 64; ++k)
    if (q[k] < 1 || q[k] > 255) { g_host_error = "ofdg_host_jpeg_block: q: every entry must lie in 1..255"; return OFDG_EINVAL; }
  uint8_t o[64];
  jpeg_block(in, q, levels, o);
  std::memcpy(out, o, sizeof(o));
  return OFDG_OK;
}
int ofdg_host_jpeg(const struct ofdg_jpeg_job* job, int n_samples, int width, int height) {
  const DevJpegJob* const j = reinterpret_cast<const DevJpegJob*>(job);
  if (!host_open("ofdg_host_jpeg", j, n_samples, width, height, /*pair_rule=*/false, jpeg_arg_error)) return OFDG_EINVAL;
  const int W = width, H = height;
  const size_t plane = (size_t)W * H;
  const int ses = fmt_elem_bytes(j->src_fmt), des = fmt_elem_bytes(j->dst_fmt);
  std::vector<uint8_t> ycc[3], out[3];   // a sample's frame as Y, Cb, Cr; the decoded B, G, R
  for (int c = 0; c < 3; ++c) { ycc[c].resize(plane); out[c].resize(plane); }
  for (int i = 0; i < n_samples; ++i) {
    DevJpegRec r = record_of(j, i, [&](unsigned long long g) { return jpeg_draw_rec(j->seed, g, *j); }, jpeg_sanitise);
    record_out(j, i, r);
    for (int f = 0; f < 2; ++f) {
      if (!j->src[f]) continue;
      const int quality = r.quality[f];
      const uint8_t* const sp = static_cast<const uint8_t*>(j->src[f]) + (size_t)i * 3 * plane * ses;
      uint8_t* const dp = static_cast<uint8_t*>(j->dst[f]) + (size_t)i * 3 * plane * des;
      if (quality == 0 && j->src_fmt == j->dst_fmt) {  // copied bit for bit; in place: left as it is
        if (dp != sp) std::memcpy(dp, sp, 3 * plane * ses);
        continue;
      }
      for (size_t k = 0; k < plane; ++k) {
        int bgr[3];
        for (int c = 0; c < 3; ++c) {
          bgr[c] = sp[c * plane + k];
          if (ses == 4) {
            float e;
            std::memcpy(&e, sp + (c * plane + k) * 4, 4);
            bgr[c] = photo_index(e);
          }
        }
        if (quality == 0) {
          for (int c = 0; c < 3; ++c) out[c][k] = (uint8_t)bgr[c];
        } else {
          ycc[0][k] = (uint8_t)jpeg_luma(bgr[2], bgr[1], bgr[0]);
          ycc[1][k] = (uint8_t)jpeg_cb(bgr[2], bgr[1], bgr[0]);
          ycc[2][k] = (uint8_t)jpeg_cr(bgr[2], bgr[1], bgr[0]);
        }
      }
      if (quality > 0) {
        uint16_t q[2][64];
        for (int k = 0; k < 64; ++k) {
          q[0][k] = (uint16_t)jpeg_quant(kJpegBaseLuma[k], quality);
          q[1][k] = (uint16_t)jpeg_quant(kJpegBaseChroma[k], quality);
        }
        const int sub = r.subsample, M = jpeg_mcu(sub);
        const int px = jpeg_phase(r.phase_x, sub), py = jpeg_phase(r.phase_y, sub);
        for (int oy = -py; oy < H; oy += M)
          for (int ox = -px; ox < W; ox += M) {
            uint8_t dec[3][256];  // the decoded Y, Cb, Cr of the MCU, [M][M]
            for (int c = 0; c < 3; ++c) {
              const bool coarse = sub && c > 0;
              for (int b = 0; b < (sub && c == 0 ? 4 : 1); ++b) {
                const int bx = 8 * (b & 1), by = 8 * (b >> 1);
                uint8_t in[64], o[64];
                for (int y = 0; y < 8; ++y)
                  for (int x = 0; x < 8; ++x) {
                    if (!coarse) {
                      in[y * 8 + x] = ycc[c][(size_t)camera_clamp(oy + by + y, H) * W + camera_clamp(ox + bx + x, W)];
                    } else {
                      const size_t y0 = (size_t)camera_clamp(oy + 2 * y, H) * W, y1 = (size_t)camera_clamp(oy + 2 * y + 1, H) * W;
                      const int x0 = camera_clamp(ox + 2 * x, W), x1 = camera_clamp(ox + 2 * x + 1, W);
                      in[y * 8 + x] = (uint8_t)jpeg_cell((int32_t)ycc[c][y0 + x0] + ycc[c][y0 + x1] + ycc[c][y1 + x0] + ycc[c][y1 + x1]);
                    }
                  }
                jpeg_block(in, q[c ? 1 : 0], nullptr, o);
                for (int y = 0; y < (coarse ? 16 : 8); ++y)
                  for (int x = 0; x < (coarse ? 16 : 8); ++x) dec[c][(by + y) * M + bx + x] = coarse ? o[(y >> 1) * 8 + (x >> 1)] : o[y * 8 + x];
              }
            }
            for (int y = oy < 0 ? -oy : 0; y < M && oy + y < H; ++y)
              for (int x = ox < 0 ? -ox : 0; x < M && ox + x < W; ++x) {
                const int Y = dec[0][y * M + x], cb = dec[1][y * M + x], cr = dec[2][y * M + x];
                const size_t k = (size_t)(oy + y) * W + (size_t)(ox + x);
                out[0][k] = (uint8_t)jpeg_blue(Y, cb); out[1][k] = (uint8_t)jpeg_green(Y, cb, cr); out[2][k] = (uint8_t)jpeg_red(Y, cr);
              }
          }
      }
      for (int c = 0; c < 3; ++c)
        for (size_t k = 0; k < plane; ++k) {
          uint8_t* const q = dp + (c * plane + k) * des;
          const float e = (float)out[c][k];
          if (des == 4) std::memcpy(q, &e, 4);
          else *q = out[c][k];
        }
    }
  }
  return OFDG_OK;
}

// ofdg_motion_blur on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The draw, the sanitising, the
// half-displacement, the tap count, step and coordinate, the tap value, the weights and the argument rules are the functions
// the kernel runs (csrc/ofdg_device.h); elements are moved with memcpy.
int ofdg_motion_blur_draw(uint32_t seed, long long index, const struct ofdg_mblur_job* ranges, ofdg_mblur_rec* out) {
  return draw_entry("ofdg_motion_blur_draw", mblur_ranges_error, mblur_draw_rec, seed, index, ranges, out);
}
int ofdg_host_motion_blur(const struct ofdg_mblur_job* job, int n_samples, int width, int height) {
  const DevMblurJob* const j = reinterpret_cast<const DevMblurJob*>(job);
  if (!host_open("ofdg_host_motion_blur", j, n_samples, width, height, /*pair_rule=*/true, mblur_arg_error)) return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  const int ses = fmt_elem_bytes(j->src_fmt), des = fmt_elem_bytes(j->dst_fmt);
  for (int i = 0; i < n_samples; ++i) {
    DevMblurRec r = record_of(j, i, [&](unsigned long long g) { return mblur_draw_rec(j->seed, g, *j); }, mblur_sanitise);
    record_out(j, i, r);
    for (int f = 0; f < 2; ++f) {
      if (!j->src[f]) continue;
      const float s = r.shutter[f];
      const FlowPlane flow{j->flow[f], j->flow_fmt};
      const size_t fu = (size_t)i * 2 * plane, fv = fu + plane;
      const uint8_t* const sp = static_cast<const uint8_t*>(j->src[f]) + (size_t)i * 3 * plane * ses;
      uint8_t* const dp = static_cast<uint8_t*>(j->dst[f]) + (size_t)i * 3 * plane * des;
      const auto byte_at = [&](int c, int x, int y) -> uint32_t {
        const size_t e = (size_t)c * plane + (size_t)spatial_clamp(y, height) * width + spatial_clamp(x, width);
        if (ses == 1) return sp[e];
        float v;
        std::memcpy(&v, sp + 4 * e, 4);
        return (uint32_t)photo_index(v);
      };
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
          const size_t p = (size_t)y * width + x;
          const float u = flow.at(fu + p), v = flow.at(fv + p);
          const bool finite = mblur_finite(u) && mblur_finite(v);
          const int Dx = finite ? mblur_half(u, s) : 0, Dy = finite ? mblur_half(v, s) : 0;
          const int m = mblur_taps_side(Dx, Dy, j->taps_side);
          const int sx = m ? mblur_step(Dx, m) : 0, sy = m ? mblur_step(Dy, m) : 0;
          for (int c = 0; c < 3; ++c) {
            uint32_t S = 0;
            for (int k = -m; k <= m; ++k) {
              const int Qx = mblur_coord(x, k, sx, width), Qy = mblur_coord(y, k, sy, height);
              const int ix = Qx >> 8, iy = Qy >> 8;
              S += mblur_weight(k, m) * mblur_tap(byte_at(c, ix, iy), byte_at(c, ix + 1, iy), byte_at(c, ix, iy + 1), byte_at(c, ix + 1, iy + 1), Qx & 255, Qy & 255);
            }
            const uint32_t b = mblur_byte(S);
            const float o = (float)b;
            if (des == 1) dp[(size_t)c * plane + p] = (uint8_t)b;
            else std::memcpy(dp + 4 * ((size_t)c * plane + p), &o, 4);
          }
        }
    }
  }
  return OFDG_OK;
}

// ofdg_reproject on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel.  The displacement, the inside
// test, the tap, the warped byte, the backward displacement, the residual and the argument rules are the functions the kernel
// runs (csrc/ofdg_device.h); elements are moved with memcpy.
int ofdg_host_reproject(const struct ofdg_reproject_job* job, int n_samples, int width, int height) {
  const DevReprojJob* const j = reinterpret_cast<const DevReprojJob*>(job);
  if (!host_open("ofdg_host_reproject", j, n_samples, width, height, /*pair_rule=*/true, reproj_arg_error)) return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  const int ses = fmt_elem_bytes(j->img_fmt), des = fmt_elem_bytes(j->dst_fmt);
  const bool with_err = reproj_with_err(*j);
  const long long thr2 = (long long)j->fb_thresh_q8 * j->fb_thresh_q8;
  uint8_t* const rows = reinterpret_cast<uint8_t*>(j->rows);
  if (rows && !(j->flags & OFDG_REPROJ_ACCUMULATE)) std::memset(rows, 0, sizeof(DevReprojRow) * (size_t)n_samples);
  for (int i = 0; i < n_samples; ++i)
    for (int f = 0; f < 2; ++f) {
      if (!((j->flags >> f) & 1)) continue;
      const bool with_fb = reproj_with_fb(*j, f), with_own = j->img[f] != nullptr, with_other = j->img[1 - f] != nullptr;
      const FlowPlane flow{j->flow[f], j->flow_fmt}, back{j->flow[1 - f], j->flow_fmt};
      const OccPlane occ{j->occ[f], j->occ_fmt};
      const size_t fu = (size_t)i * 2 * plane, fv = fu + plane;
      const auto byte_at = [&](int g, int c, int x, int y) -> uint32_t {
        const uint8_t* const sp = static_cast<const uint8_t*>(j->img[g]) + (size_t)i * 3 * plane * ses;
        const size_t e = (size_t)c * plane + (size_t)spatial_clamp(y, height) * width + spatial_clamp(x, width);
        if (ses == 1) return sp[e];
        float v;
        std::memcpy(&v, sp + 4 * e, 4);
        return (uint32_t)photo_index(v);
      };
      DevReprojFrameRow r;
      if (rows) std::memcpy(&r, rows + sizeof(DevReprojRow) * (size_t)i + sizeof(r) * (size_t)f, sizeof(r));
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
          const size_t p = (size_t)y * width + x;
          const float u = flow.at(fu + p), v = flow.at(fv + p);
          const bool bad = !(mblur_finite(u) && mblur_finite(v));
          const int Dx = bad ? 0 : reproj_q8(u), Dy = bad ? 0 : reproj_q8(v);
          const bool in = !bad && reproj_inside(256 * x + Dx, 256 * y + Dy, width, height);
          uint32_t w[3] = {0u, 0u, 0u}, err = 0u;
          long long e2 = 0;
          float fb2 = 0.0f;
          if (in) {
            const int Qx = reproj_coord(256 * x + Dx, width), Qy = reproj_coord(256 * y + Dy, height);
            const int ix = Qx >> 8, iy = Qy >> 8, fx = Qx & 255, fy = Qy & 255;
            if (with_other)
              for (int c = 0; c < 3; ++c) {
                w[c] = reproj_byte(mblur_tap(byte_at(1 - f, c, ix, iy), byte_at(1 - f, c, ix + 1, iy), byte_at(1 - f, c, ix, iy + 1), byte_at(1 - f, c, ix + 1, iy + 1), fx, fy));
                if (with_own) {
                  const uint32_t own = byte_at(f, c, x, y), d = w[c] > own ? w[c] - own : own - w[c];
                  err = d > err ? d : err;
                }
              }
            if (with_fb) {
              const size_t xa = (size_t)spatial_clamp(ix, width), xb = (size_t)spatial_clamp(ix + 1, width);
              const size_t ya = (size_t)spatial_clamp(iy, height) * width, yb = (size_t)spatial_clamp(iy + 1, height) * width;
              float b[2][4];
              bool finite = true;
              for (int k = 0; k < 2; ++k) {
                const size_t o = fu + (size_t)k * plane;
                b[k][0] = back.at(o + ya + xa); b[k][1] = back.at(o + ya + xb); b[k][2] = back.at(o + yb + xa); b[k][3] = back.at(o + yb + xb);
                for (int t = 0; t < 4; ++t) finite = finite && mblur_finite(b[k][t]);
              }
              if (finite) {
                e2 = reproj_e2(Dx, Dy, reproj_back(b[0][0], b[0][1], b[0][2], b[0][3], fx, fy), reproj_back(b[1][0], b[1][1], b[1][2], b[1][3], fx, fy));
                fb2 = reproj_fb2(e2);
              } else {
                e2 = kReprojE2Sat;
                fb2 = INFINITY;
              }
            }
          }
          for (int c = 0; c < 3 && j->warped[f]; ++c) {
            uint8_t* const dp = static_cast<uint8_t*>(j->warped[f]) + (size_t)i * 3 * plane * des;
            const float o = (float)w[c];
            if (des == 1) dp[(size_t)c * plane + p] = (uint8_t)w[c];
            else std::memcpy(dp + 4 * ((size_t)c * plane + p), &o, 4);
          }
          if (j->err[f]) static_cast<uint8_t*>(j->err[f])[(size_t)i * plane + p] = (uint8_t)err;
          if (j->mask[f]) static_cast<uint8_t*>(j->mask[f])[(size_t)i * plane + p] = in ? 1 : 0;
          if (j->fb2[f]) std::memcpy(static_cast<uint8_t*>(j->fb2[f]) + 4 * ((size_t)i * plane + p), &fb2, 4);
          if (!rows) continue;
          if (!in) { ++r.cnt[bad ? 0 : 1]; continue; }
          const int hid = j->occ[f] && occ.at((size_t)i * plane + p) ? 1 : 0;
          ++r.cnt[2 + hid];
          if (with_err) {
            r.sum_err[hid] += err;
            if (!hid) { ++r.err_hist[err >> 4]; r.max_err_visible = err > r.max_err_visible ? err : r.max_err_visible; }
          }
          if (with_fb) {
            if (e2 > thr2) ++r.n_fb_over[hid];
            if (!hid) {
              r.sum_fb2_visible += (unsigned long long)(e2 < 4294967295ll ? e2 : 4294967295ll);
              r.max_fb2_visible = (unsigned long long)e2 > r.max_fb2_visible ? (unsigned long long)e2 : r.max_fb2_visible;
            }
          }
        }
      if (rows) std::memcpy(rows + sizeof(DevReprojRow) * (size_t)i + sizeof(r) * (size_t)f, &r, sizeof(r));
    }
  return OFDG_OK;
}

// ofdg_splat on host arrays (no GPU): the definition of include/ofdg.h pixel by pixel - the scatter over the sources, then
// the targets, then the fates.  The draw, the sanitising, the displacement, its scaling, the rounded target, the key and the
// argument rules are the functions the kernels run (csrc/ofdg_device.h); elements are moved with memcpy.
int ofdg_splat_draw(uint32_t seed, long long index, const struct ofdg_splat_job* ranges, ofdg_splat_rec* out) {
  return draw_entry("ofdg_splat_draw", splat_ranges_error, splat_draw_rec, seed, index, ranges, out);
}
int ofdg_host_splat(const struct ofdg_splat_job* job, int n_samples, int width, int height) {
  const DevSplatJob* const j = reinterpret_cast<const DevSplatJob*>(job);
  if (!host_open("ofdg_host_splat", j, n_samples, width, height, /*pair_rule=*/true, splat_arg_error)) return OFDG_EINVAL;
  const size_t plane = (size_t)width * height;
  const int ses = fmt_elem_bytes(j->img_fmt), des = fmt_elem_bytes(j->dst_fmt);
  uint8_t* const rows = reinterpret_cast<uint8_t*>(j->rows);
  if (rows && !(j->flags & OFDG_SPLAT_ACCUMULATE)) std::memset(rows, 0, sizeof(DevSplatRow) * (size_t)n_samples);
  const auto put_flow = [&](void* base, size_t e, float v) {
    if (j->oflow_fmt == OFDG_FMT_F16) {
      const uint16_t h = float_to_half_bits(v);
      std::memcpy(static_cast<uint8_t*>(base) + 2 * e, &h, 2);
    } else std::memcpy(static_cast<uint8_t*>(base) + 4 * e, &v, 4);
  };
  for (int i = 0; i < n_samples; ++i) {
    DevSplatRec rec = record_of(j, i, [&](unsigned long long g) { return splat_draw_rec(j->seed, g, *j); }, splat_sanitise);
    record_out(j, i, rec);
    for (int f = 0; f < 2; ++f) {
      if (!((j->flags >> f) & 1)) continue;
      const int T = rec.t_q8[f];
      const FlowPlane flow{j->flow[f], j->flow_fmt};
      const OccPlane own_occ{j->occ[f], j->occ_fmt}, other_occ{j->occ[1 - f], j->occ_fmt};
      const size_t fu = (size_t)i * 2 * plane, fv = fu + plane;
      uint8_t* const keys = reinterpret_cast<uint8_t*>(j->keys[f]) + 4 * (size_t)i * plane;
      const auto key_at = [&](size_t p) { uint32_t k; std::memcpy(&k, keys + 4 * p, 4); return k; };
      // where source s goes: 3 bad, 2 outside, else 0 with its target in *tp and its key in *key
      const auto aim = [&](int x, int y, size_t* tp, uint32_t* key, int* Dx, int* Dy) -> int {
        const size_t s = (size_t)y * width + x;
        const float u = flow.at(fu + s), v = flow.at(fv + s);
        if (!(mblur_finite(u) && mblur_finite(v))) return 3;
        *Dx = reproj_q8(u); *Dy = reproj_q8(v);
        const int rx = splat_round(x, splat_scale(*Dx, T)), ry = splat_round(y, splat_scale(*Dy, T));
        if (!splat_inside(rx, ry, width, height)) return 2;
        *tp = (size_t)ry * width + rx;
        *key = splat_key(j->label[f] ? j->label[f][(size_t)i * plane + s] : 0u, (uint32_t)s);
        return 0;
      };
      DevSplatFrameRow r{};
      if (rows) std::memcpy(&r, rows + sizeof(DevSplatRow) * (size_t)i + sizeof(r) * (size_t)f, sizeof(r));
      std::memset(keys, 0, 4 * plane);
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
          size_t tp = 0;
          uint32_t key = 0;
          int Dx = 0, Dy = 0;
          const int fate = aim(x, y, &tp, &key, &Dx, &Dy);
          ++r.src[fate == 3 ? 0 : fate == 2 ? 1 : 2];
          if (fate == 0 && key > key_at(tp)) std::memcpy(keys + 4 * tp, &key, 4);
        }
      for (int py = 0; py < height; ++py)
        for (int px = 0; px < width; ++px) {
          const size_t p = (size_t)py * width + px;
          const uint32_t K = key_at(p);
          uint32_t byte[3] = {0u, 0u, 0u};
          float own[2] = {0.0f, 0.0f}, other[2] = {0.0f, 0.0f};
          if (K) {
            const size_t s = splat_source(K);
            const int x = (int)(s % (size_t)width), y = (int)(s / (size_t)width);
            own[0] = (float)(x - px); own[1] = (float)(y - py);
            other[0] = splat_to_other(x - px, reproj_q8(flow.at(fu + s)));
            other[1] = splat_to_other(y - py, reproj_q8(flow.at(fv + s)));
            for (int c = 0; c < 3 && j->img[f]; ++c) {
              const uint8_t* const sp = static_cast<const uint8_t*>(j->img[f]) + (size_t)i * 3 * plane * ses;
              const size_t e = (size_t)c * plane + s;
              if (ses == 1) byte[c] = sp[e];
              else {
                float v;
                std::memcpy(&v, sp + 4 * e, 4);
                byte[c] = (uint32_t)photo_index(v);
              }
            }
            ++r.dst[0];
          } else {
            ++r.dst[1];
            if (j->occ[1 - f]) ++r.hole_other[other_occ.at((size_t)i * plane + p) ? 1 : 0];
          }
          for (int c = 0; c < 3 && j->image[f]; ++c) {
            uint8_t* const dp = static_cast<uint8_t*>(j->image[f]) + (size_t)i * 3 * plane * des;
            const float o = (float)byte[c];
            if (des == 1) dp[(size_t)c * plane + p] = (uint8_t)byte[c];
            else std::memcpy(dp + 4 * ((size_t)c * plane + p), &o, 4);
          }
          for (int c = 0; c < 2; ++c) {
            if (j->to_own[f]) put_flow(j->to_own[f], fu + (size_t)c * plane + p, own[c]);
            if (j->to_other[f]) put_flow(j->to_other[f], fu + (size_t)c * plane + p, other[c]);
          }
          if (j->mask[f]) static_cast<uint8_t*>(j->mask[f])[(size_t)i * plane + p] = K ? 1 : 0;
        }
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
          const size_t s = (size_t)y * width + x;
          size_t tp = 0;
          uint32_t key = 0;
          int Dx = 0, Dy = 0;
          int fate = aim(x, y, &tp, &key, &Dx, &Dy);
          if (fate == 0 && key_at(tp) != key) {
            fate = 1;
            ++r.n_covered;
            if (j->occ[f]) ++r.covered[own_occ.at((size_t)i * plane + s) ? 1 : 0];
          }
          if (j->fate[f]) static_cast<uint8_t*>(j->fate[f])[(size_t)i * plane + s] = (uint8_t)fate;
        }
      r.t_q8 = (uint32_t)T;
      if (rows) std::memcpy(rows + sizeof(DevSplatRow) * (size_t)i + sizeof(r) * (size_t)f, &r, sizeof(r));
    }
  }
  return OFDG_OK;
}

}  // extern "C"
