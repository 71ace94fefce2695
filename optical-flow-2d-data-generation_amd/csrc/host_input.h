// Everything that reads untrusted input - the layer's prototxt, image files, texture lists - and nothing of the GPU:
// no HIP header, no call that takes an ofdg_ctx.  The seam to the GPU is layer.cpp, which turns a TexturePlan into
// ofdg_pool_* uploads.  tools/host_input_check.cpp links this code on its own (make san).
#pragma once
#include <stdint.h>

#include <istream>
#include <string>
#include <vector>

#include "../../include/ofdg.h"

namespace ofdg {

// ofdg_host_last_error's text: one string per thread, set by the ofdg_host_* and ofdg_layer_* wrappers (host_api.cpp)
extern thread_local std::string g_host_error;

// What the prototxt subset parser extracts (src/caffe/proto/caffe.proto:6-12 and
// the LMB data_param fields used at data_generation_layer.cpp:44, 109-113).
struct LayerConfig {
  std::string name, type;
  std::vector<std::string> top;
  ofdg_params params;
  std::string texture_dbases;  // list file, or "synthetic:N:W:H[:seed]"
};

// Parses one `layer { ... }` block (protobuf text format subset: nested messages,
// key: value, strings, numbers, true/false, '#' comments).  Throws std::runtime_error.
LayerConfig parse_layer_prototxt(const std::string& text);

// An image file of a texture list: binary PPM or PNG, by its first bytes.  planar_bgr == nullptr is the probe (the size
// only: a PPM's header and the file's length, no payload), otherwise the decode (planes B, G, R).  A refusal returns false
// with the reason in *why; no allocation is made from a header the file's length does not bear out.
bool read_image(std::istream& file, std::vector<uint8_t>* planar_bgr, int* w, int* h, std::string* why);
bool read_image(const std::string& path, std::vector<uint8_t>* planar_bgr, int* w, int* h, std::string* why);

// What a texture_dbases spec asks for, as far as files tell: TextureCollection (DataGenerator.cpp:117-149) up to the uploads.
struct TexturePlan {
  std::string error;  // not empty: the collection cannot be opened, and this is the whole message
  bool synthetic = false;
  int n = 0, w = 0, h = 0;  // synthetic:N:W:H[:seed]
  unsigned seed = 0;
  std::vector<std::string> paths;  // a list: its files, the size of each ...
  std::vector<int> widths, heights;
  bool mixed = false;  // ... and whether the sizes differ
};
TexturePlan plan_texture_collection(const std::string& spec);

}  // namespace ofdg
