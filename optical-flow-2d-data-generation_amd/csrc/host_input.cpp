#include "host_input.h"

#include <dlfcn.h>

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <new>
#include <stdexcept>

namespace ofdg {

// ---- prototxt subset parser ----
namespace {
struct Tok {
  enum Kind { kIdent, kString, kNumber, kLBrace, kRBrace, kColon, kEnd } kind;
  std::string text;
};
class Lexer {
 public:
  explicit Lexer(const std::string& s) : s_(s) {}
  Tok next() {
    for (;;) {
      while (i_ < s_.size() && std::isspace((unsigned char)s_[i_])) ++i_;
      if (i_ < s_.size() && s_[i_] == '#') { while (i_ < s_.size() && s_[i_] != '\n') ++i_; continue; }
      break;
    }
    if (i_ >= s_.size()) return {Tok::kEnd, ""};
    const char ch = s_[i_];
    if (ch == '{') { ++i_; return {Tok::kLBrace, "{"}; }
    if (ch == '}') { ++i_; return {Tok::kRBrace, "}"}; }
    if (ch == ':') { ++i_; return {Tok::kColon, ":"}; }
    if (ch == '"' || ch == '\'') {
      const char q = ch;
      std::string v;
      ++i_;
      while (i_ < s_.size() && s_[i_] != q) {
        if (s_[i_] == '\\' && i_ + 1 < s_.size()) ++i_;
        v += s_[i_++];
      }
      if (i_ >= s_.size()) throw std::runtime_error("prototxt: unterminated string");
      ++i_;
      return {Tok::kString, v};
    }
    if (std::isalpha((unsigned char)ch) || ch == '_') {
      std::string v;
      while (i_ < s_.size() && (std::isalnum((unsigned char)s_[i_]) || s_[i_] == '_')) v += s_[i_++];
      return {Tok::kIdent, v};
    }
    if (std::isdigit((unsigned char)ch) || ch == '-' || ch == '+' || ch == '.') {
      std::string v;
      while (i_ < s_.size() && (std::isalnum((unsigned char)s_[i_]) || s_[i_] == '-' || s_[i_] == '+' || s_[i_] == '.')) v += s_[i_++];
      return {Tok::kNumber, v};
    }
    throw std::runtime_error(std::string("prototxt: unexpected character '") + ch + "'");
  }

 private:
  const std::string& s_;
  size_t i_ = 0;
};

int to_int(const Tok& t, const std::string& scope, const std::string& field) {
  if (t.kind == Tok::kIdent && (t.text == "true" || t.text == "false")) return t.text == "true";
  if (t.kind != Tok::kNumber) throw std::runtime_error("prototxt: expected a number for " + (scope.empty() ? field : scope + "." + field));
  return (int)std::strtol(t.text.c_str(), nullptr, 10);
}

// A loop, not a recursion: the text sets the nesting depth.  `scope` is the dotted path of the open messages; it grows at
// '{' and is cut back at '}' to the length `open` kept, so memory stays linear in the text.  A field is looked at without its
// full key being built: time stays linear too.
void parse_message(Lexer& lx, LayerConfig* cfg) {
  struct Open { size_t cut; bool in_dgp; };
  std::string scope;
  std::vector<Open> open;
  bool in_dgp = false;  // "data_generation_param." occurs in the dotted path: an open message's name ends with it
  const std::string dgp = "data_generation_param";
  for (;;) {
    Tok k = lx.next();
    if (k.kind == Tok::kEnd) {
      if (!open.empty()) throw std::runtime_error("prototxt: missing '}'");
      return;
    }
    if (k.kind == Tok::kRBrace) {
      if (open.empty()) throw std::runtime_error("prototxt: unbalanced '}'");
      scope.resize(open.back().cut);
      in_dgp = open.back().in_dgp;
      open.pop_back();
      continue;
    }
    if (k.kind != Tok::kIdent) throw std::runtime_error("prototxt: expected a field name");
    Tok v = lx.next();
    if (v.kind == Tok::kColon) v = lx.next();
    if (v.kind == Tok::kLBrace) {
      open.push_back({scope.size(), in_dgp});
      if (!scope.empty()) scope += '.';
      scope += k.text;
      in_dgp = in_dgp || (k.text.size() >= dgp.size() && k.text.compare(k.text.size() - dgp.size(), dgp.size(), dgp) == 0);
      continue;
    }
    const std::string& f = k.text;
    const bool top = scope.empty() || scope == "layer", data = scope == "data_param" || scope == "layer.data_param";
    ofdg_params& p = cfg->params;
    auto num = [&] { return to_int(v, scope, f); };
    if (top && f == "name") cfg->name = v.text;
    else if (top && f == "type") cfg->type = v.text;
    else if (top && f == "top") cfg->top.push_back(v.text);
    else if (data && f == "batch_size") p.batch_size = num();
    else if (data && f == "prefetch") p.prefetch = num();
    else if (in_dgp) {
      if (f == "mode") p.mode = num();
      else if (f == "texture_dbases") { if (cfg->texture_dbases.empty()) cfg->texture_dbases = v.text; }
      else if (f == "first_level_threads") p.first_level_threads = num();
      else if (f == "second_level_threads") p.second_level_threads = num();
      else if (f == "use_antialiasing") p.use_antialiasing = num();
      // extension keys (not in the reference's proto)
      else if (f == "width") p.width = num();
      else if (f == "height") p.height = num();
      else if (f == "num_objects") p.num_objects = num();
      else if (f == "seed") p.seed = num();
      else if (f == "chains") p.chains = num();        // scheduling (extension keys): internal streams,
      else if (f == "lookahead") p.lookahead = num();  // batches prepared ahead of the Forward that composes them
      else if (f == "background_prep")  // true / 1: the CImg chain stage by stage; fast / 2: one resampling; false / 0: centre crop
        p.background_prep = (v.text == "true" || v.text == "1") ? 1 : (v.text == "fast" || v.text == "2") ? 2 : 0;
      else if (f == "sampler") p.sampler = (v.text == "counter") ? OFDG_SAMPLER_COUNTER : OFDG_SAMPLER_REF;
      else throw std::runtime_error("prototxt: unknown data_generation_param field '" + f + "'");
    }
    // other fields (bottom, include, data_param.verbose ...) are accepted and ignored
  }
}
}  // namespace

LayerConfig parse_layer_prototxt(const std::string& text) {
  LayerConfig cfg;
  ofdg_default_params(&cfg.params);
  // the reference always runs getRandomizedCrop(2W, 2H, rot, zoom, shift) on the background (DataGenerator.cpp:1186-1192):
  // the layer does too unless the prototxt says `background_prep: false` (extension key)
  cfg.params.background_prep = 1;
  Lexer lx(text);
  parse_message(lx, &cfg);
  return cfg;
}

// ---- image files ----
namespace {
// interleaved R, G, B (stride 3) or R, G, B, A (stride 4) -> CImg's planes with c0 and c2 swapped (DataGenerator.cpp:129-131)
void to_planar_bgr(const uint8_t* px, int stride, size_t n, std::vector<uint8_t>* planar_bgr) {
  planar_bgr->resize(3 * n);
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) (*planar_bgr)[c * n + i] = px[stride * i + 2 - c];
}
// The one PPM header reader: magic, '#' comments, w, h, maxval == 255, both sizes > 0, the single whitespace byte after
// maxval.  The numbers are operator>>(int&)'s: its signs, its overflow, its trailing characters.
bool ppm_header(std::istream& f, int* w, int* h) {
  std::string magic;
  f >> magic;
  if (magic != "P6") return false;
  auto next_int = [&](int* out) {
    for (;;) {
      int c = f.peek();
      if (c == '#') { std::string line; std::getline(f, line); continue; }
      if (std::isspace(c)) { f.get(); continue; }
      break;
    }
    f >> *out;
    return !f.fail();
  };
  int maxv = 0;
  if (!next_int(w) || !next_int(h) || !next_int(&maxv) || maxv != 255 || *w <= 0 || *h <= 0) return false;
  f.get();  // single whitespace after maxval
  return !f.fail();
}
// planar_bgr == nullptr: the size only (the header and the file's length, no payload)
bool read_ppm(std::istream& f, std::vector<uint8_t>* planar_bgr, int* w, int* h) {
  if (!ppm_header(f, w, h)) return false;
  const std::streamoff payload = f.tellg();
  f.seekg(0, std::ios::end);
  const uint64_t n = (uint64_t)*w * (uint64_t)*h;
  // before anything is sized by the header: the file holds the 3 * w * h bytes it claims (w, h < 2^31: no overflow)
  if (payload < 0 || (uint64_t)(f.tellg() - payload) < 3 * n) return false;
  if (!planar_bgr) return true;
  f.seekg(payload);
  std::vector<uint8_t> rgb(3 * n);
  f.read((char*)rgb.data(), (std::streamsize)rgb.size());
  if ((size_t)f.gcount() != rgb.size()) return false;
  to_planar_bgr(rgb.data(), 3, n, planar_bgr);
  return true;
}

// PNG through the system's libpng 1.6, bound at run time (dlopen: the library is part of the image, a build dependency on
// it is not wanted).  Its "simplified API" (png.h 1.6: png_image_begin_read_from_memory / png_image_finish_read /
// png_image_free over a caller-owned png_image) is a stable C ABI; the struct below restates png_image field by field.
// 8-bit R, G, B, A come back as stored (alpha is read and dropped: CImg's load keeps it as a fourth channel the
// reference never looks at, DataGenerator.cpp:128-131); palette, grey and 16-bit files are expanded by libpng.
struct PngImage {
  void* opaque;
  uint32_t version, width, height, format, flags, colormap_entries, warning_or_error;
  char message[64];
};
struct PngApi {
  int (*begin_read_from_memory)(PngImage*, const void*, size_t) = nullptr;
  int (*finish_read)(PngImage*, const void* background, void* buffer, int32_t row_stride, void* colormap) = nullptr;
  void (*image_free)(PngImage*) = nullptr;
  bool ok = false;
  PngApi() {
    void* h = nullptr;
    for (const char* name : {"libpng16.so.16", "libpng16.so"}) if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) return;
    begin_read_from_memory = (decltype(begin_read_from_memory))dlsym(h, "png_image_begin_read_from_memory");
    finish_read = (decltype(finish_read))dlsym(h, "png_image_finish_read");
    image_free = (decltype(image_free))dlsym(h, "png_image_free");
    ok = begin_read_from_memory && finish_read && image_free;
  }
};
const PngApi& png_api() { static const PngApi api; return api; }
constexpr uint32_t kPngImageVersion = 1, kPngFormatRgba = 0x03;  // PNG_IMAGE_VERSION; PNG_FORMAT_FLAG_ALPHA | PNG_FORMAT_FLAG_COLOR
constexpr unsigned char kPngSignature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};

// libpng's simplified API hands out 8-bit sRGB samples: it honours the file's colour-management chunks (a gAMA that is not
// sRGB's re-encodes every sample), while the reference's CImg::load (DataGenerator.cpp:128) keeps the raw sample values with
// no gamma handling.  So the file is decoded from MEMORY with those chunks - gAMA, cHRM, sRGB, iCCP: ancillary, each chunk
// carries its own CRC - left out: libpng then takes 8-bit samples as what they are, and the pool holds the bytes the
// reference's holds, whatever the file says about its gamma.  16 bits per sample stay refused, with the way out in the
// message: CImg would hand the reference's `unsigned char` image the truncated 16-bit values, libpng a conversion from linear
// light - neither is a texture anybody meant.
bool png_without_colour_chunks(const std::vector<unsigned char>& in, std::vector<unsigned char>* out, std::string* why) {
  auto be32 = [](const unsigned char* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; };
  out->assign(in.begin(), in.begin() + 8);  // (the signature: read_image has seen it)
  size_t i = 8;
  while (i + 12 <= in.size()) {
    const uint32_t len = be32(&in[i]);
    const std::string type((const char*)&in[i + 4], 4);
    if ((size_t)len + 12 > in.size() - i) break;
    if (type == "IHDR" && len >= 9 && in[i + 8 + 8] == 16) {
      *why = "16-bit PNG: the reference's 8-bit texture would hold its truncated samples; convert the texture to 8 bit (tools/convert_textures.py)";
      return false;
    }
    if (type != "gAMA" && type != "cHRM" && type != "sRGB" && type != "iCCP") out->insert(out->end(), in.begin() + i, in.begin() + i + 12 + len);
    i += 12 + (size_t)len;
    if (type == "IEND") return true;
  }
  *why = "truncated PNG";
  return false;
}
// `in`: the whole file.  planar_bgr == nullptr: the size only
bool read_png(const std::vector<unsigned char>& in, std::vector<uint8_t>* planar_bgr, int* w, int* h, std::string* why) {
  const PngApi& api = png_api();
  if (!api.ok) { *why = "libpng16 is not available on this system"; return false; }
  std::vector<unsigned char> file;
  if (!png_without_colour_chunks(in, &file, why)) return false;
  PngImage img;
  std::memset(&img, 0, sizeof(img));
  img.version = kPngImageVersion;
  struct Free {  // (png_image_free of an image already freed, by a failed call or a finished read, does nothing)
    PngImage* img;
    ~Free() { png_api().image_free(img); }
  } free_at_exit{&img};
  if (!api.begin_read_from_memory(&img, file.data(), file.size())) { *why = img.message; return false; }
  *w = (int)img.width; *h = (int)img.height;
  if (!planar_bgr) return true;
  img.format = kPngFormatRgba;
  const size_t n = (size_t)img.width * img.height;
  std::unique_ptr<uint8_t[]> rgba(new uint8_t[n * 4]);  // (not zeroed: a page costs nothing until libpng has a row for it)
  if (!api.finish_read(&img, nullptr, rgba.get(), 0, nullptr)) { *why = img.message; return false; }
  to_planar_bgr(rgba.get(), 4, n, planar_bgr);
  return true;
}
}  // namespace

bool read_image(std::istream& f, std::vector<uint8_t>* planar_bgr, int* w, int* h, std::string* why) {
  *w = *h = 0;
  try {
    std::vector<unsigned char> in(8);
    f.read((char*)in.data(), 8);
    if (f.gcount() == 8 && std::memcmp(in.data(), kPngSignature, 8) == 0) {  // a PNG is read whole, once: filter and libpng work on `in`
      in.insert(in.end(), std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
      return read_png(in, planar_bgr, w, h, why);
    }
    f.clear();
    f.seekg(0);
    if (read_ppm(f, planar_bgr, w, h)) return true;
    *why = "neither a binary PPM (P6, maxval 255) nor a PNG";
    return false;
  } catch (const std::bad_alloc&) {  // (after the PPM payload check only a PNG's header can ask for this much)
  } catch (const std::length_error&) {
  }
  *why = std::to_string(*w) + " x " + std::to_string(*h) + " image does not fit in memory";
  return false;
}
bool read_image(const std::string& path, std::vector<uint8_t>* planar_bgr, int* w, int* h, std::string* why) {
  std::ifstream f(path, std::ios::binary);
  return read_image(f, planar_bgr, w, h, why);
}

// ---- texture collection, as far as files tell ----
TexturePlan plan_texture_collection(const std::string& spec) {
  TexturePlan plan;
  if (spec.compare(0, 10, "synthetic:") == 0) {
    plan.synthetic = true;
    if (std::sscanf(spec.c_str(), "synthetic:%d:%d:%d:%u", &plan.n, &plan.w, &plan.h, &plan.seed) < 3)
      plan.error = "Could not open texture collection (bad synthetic spec)";
    return plan;
  }
  std::ifstream infile(spec);
  if (infile.bad() || !infile.is_open()) { plan.error = "Could not open texture collection"; return plan; }  // DataGenerator.cpp:121
  std::string imagepath;
  while (!infile.eof()) {  // reference loop: a last line without '\n' is dropped (DataGenerator.cpp:124-126)
    std::getline(infile, imagepath);
    if (infile.eof()) break;
    plan.paths.push_back(imagepath);
  }
  if (plan.paths.empty()) { plan.error = "Could not open texture collection (no images listed)"; return plan; }
  // headers decide; every file that cannot be used is named in ONE error (a collection with a few 16-bit PNGs is fixed in one go)
  std::string unreadable;
  int n_unreadable = 0;
  for (const std::string& path : plan.paths) {
    int w = 0, h = 0;
    std::string why;
    if (!read_image(path, nullptr, &w, &h, &why) && ++n_unreadable <= 16) unreadable += (unreadable.empty() ? "" : "; ") + path + ": " + why;
    plan.widths.push_back(w);
    plan.heights.push_back(h);
    // images of one size: the pool keeps them whole; of different sizes: every image is reduced to the two
    // textures the path reads (ofdg_pool_alloc_mixed)
    if (w != plan.widths[0] || h != plan.heights[0]) plan.mixed = true;
  }
  if (n_unreadable)
    plan.error = "Could not open texture collection (cannot read " + std::string(n_unreadable == 1 ? "" : std::to_string(n_unreadable) + " files: ") + unreadable +
                 (n_unreadable > 16 ? "; ..." : "") + ")";
  return plan;
}

}  // namespace ofdg
