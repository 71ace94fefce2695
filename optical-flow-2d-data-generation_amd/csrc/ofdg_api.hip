// C-ABI of the MI355X-native optical-flow data generator (include/ofdg.h).
// Owns the HIP context state (texture pool, workspaces) and launches the kernels
// in kernels.hip.  There is no CPU fallback: without a HIP device every entry
// point that would render fails with OFDG_EHIP.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ofdg.h"
#include "kernels.hip"
#include "sampler_counter.hip"
#include "cimg_resize.h"
#include "ofdg_device.h"
#include "owners.h"
#include "realize.h"
#include "sampler_ref.h"
#include "warpfields.h"

using namespace ofdg;

static thread_local std::string g_create_error;
// GPU_MAX_HW_QUEUES as the process environment had it when this library was loaded: HIP reads the variable once, when the
// runtime starts, so what counts is the environment the process was started with
static const int g_hw_queues_env = [] { const char* q = std::getenv("GPU_MAX_HW_QUEUES"); return q ? std::atoi(q) : 0; }();

// (every device, pinned, event and stream resource below is held by an owner of owners.h: the context's destructor is its teardown)
struct ofdg_ctx {
  ofdg_params prm;
  std::string err;
  std::string info;
  DevBuf<uint32_t> d_prep_paths;  // diagnostics: tiles of bgprep_stream_kernel by form (ofdg_debug_bgprep_paths switches it on)
  // texture pool
  DevBuf<uint32_t> pool;
  int pool_n = 0, pool_w = 0, pool_h = 0;
  // where foreground (W x H) and background (2W x 2H) textures are read from: the pool images
  // themselves (centre crops) or pools of resized copies when the images are smaller (DG:96-106)
  DevBuf<uint32_t> pool_fg;   // [n][H][W] if the images are smaller than W x H
  DevBuf<uint32_t> pool_bg;   // [n][2H][2W] if the images are smaller than 2W x 2H
  TexSource fg_src{}, bg_src{};
  bool pool_final = false;       // derived pools match the current pool contents
  bool pool_mixed = false;       // ofdg_pool_alloc_mixed: only the derived pools exist (images of different sizes)
  std::vector<std::pair<int, int>> mixed_sizes;  // source image sizes of a mixed pool (index table)
  // background_prep on a mixed pool: the whole images stay resident (getRandomizedCrop works on the original image)
  std::vector<DevBuf<uint32_t>> mixed_images;
  std::vector<DevTexEntry> tex_table;   // host copy of ...
  DevBuf<DevTexEntry> d_tex_table;      // ... the per-image table the device sampler reads
  int pool_kind = OFDG_POOL_UNIFORM;
  uint32_t pool_seed = 0;
  // sampler
  std::unique_ptr<RefSampler> sampler;
  long long step = 0;
  // host staging (pinned) + device records.  A "slot" is one realised batch resident
  // in HBM (shapes, objects, samples, outlines); slot 0 is what ofdg_render uses, the
  // others let a caller keep several batches in flight (data_param.prefetch).
  struct Slot {
    RealizedBatch batch;
    DevBuf<DevShape> d_shapes;
    DevBuf<DevShapeFrame> d_frames;
    DevBuf<int2> d_verts;
    DevBuf<DevObject> d_objects;
    DevBuf<DevSample> d_samples;
    DevBuf<char> d_rec;  // uploaded batches: shapes | objects | samples in ONE allocation (one copy per batch; the three above look into it)
    DevBuf<int4> d_items;
    DevBuf<DevBgPrep> d_bgprep;   // background_prep: one record ...
    DevBuf<uint32_t> d_bgtex;     // ... and one prepared 2W x 2H BGRX texture per sample
    // background_prep = 1 (the CImg chain stage by stage): crop of the rotated image, X-resized image, resize tables, plan
    DevBuf<uint32_t> d_bgC;
    DevBuf<unsigned long long> d_blockmask;  // [2 parities][samples][64 x 8 blocks][2 frames]
    int res_objects = 0;
    bool bgprep_pending = false;  // background_prep: the records are in d_bgprep, the textures are rendered by the next launch_prepare
    int box_parity = 0;
    size_t box_stride = 0;   // mask words per parity
    int mask_used[2] = {0, 0};  // words the last launch on each parity marked (what the next clear must cover)
    Event ev_uploaded;
    bool upload_pending = false;
    hipStream_t upload_stream = nullptr;   // where the records were (last) written
    DevBuf<DevCropRef> d_croptab;      // mode 9: crops of this batch's deforming objects
    DevBuf<float> d_bgwarp;            // mode 9: upscaled (2W x 2H) background crops
    DevBuf<unsigned> d_bgwarp_max;
    hipEvent_t compose_event = nullptr;  // last tracked compose that read this slot's records: NOT owned, an alias of a chain's ev_done ...
    bool compose_pending = false;
    hipStream_t compose_stream = nullptr;  // ... and the stream it ran on
    DevBuf<int> d_item_count;  // raster work items of the batch (ensure_item_count)
    int res_samples = 0, res_shapes = 0;
  };
  static constexpr int kUserSlots = 16;              // ofdg_upload_slot / ofdg_render_slot
  Slot slots[kUserSlots];
  // pinned staging of one batch's records on their way to the device
  struct Stage {
    PinnedBuf h;
    Event free_ev;
    bool pending = false;
  };
  Stage user_stage;  // ofdg_upload_slot
  // The pipeline: independent IN-ORDER chains.  One call = one chain (round robin); the chain's
  // stream runs [record upload | counter sampler] -> geom -> raster -> compose back to back, with no
  // cross-stream hand-over between them (an event wait in front of a kernel exposes ~15 us of
  // dispatch latency per step; kernels of one stream follow each other without a gap).  The
  // latency-bound preparation kernels of one chain overlap the compose kernels of the others.
  // Each chain owns its coverage workspace, a private record slot (ofdg_render / ofdg_forward*)
  // and its staging buffer, so chains share nothing that is written per call.
  struct Chain {
    Stream stream;
    DevBuf<uint8_t> cov;
    // extras: the labels [2][n][H][W] / backward flow [n][2][H][W] an occlusion pass needs when the caller does not want them
    // (written by compose, read by the occlusion pass behind it; guarded by ev_done like `cov`)
    DevBuf<uint8_t> x_labels;
    DevBuf<float> x_flow1;
    // ... and the packed occlusion targets [2][n][H][W] of the calls that combine the extras with a compact format (written by
    // compose, read by occlusion_fmt_kernel behind it; guarded likewise)
    DevBuf<uint32_t> x_targets;
    Slot slot;
    Stage stage;
    Event ev_prep;  // coverage ready (hand-over to a caller's stream)
    Event ev_done;  // the chain's last tracked compose ...
    bool done_pending = false;
    hipStream_t done_stream = nullptr;  // ... and the stream it ran on (the chain's own, or a caller's)
    // A batch whose preparation kernels have been enqueued on this chain and whose compose has not: what launch_prepare
    // hands to launch_compose (and, for the counter sampler, which samples it holds: the look-ahead of ofdg_forward_counter)
    struct Prepared {
      bool valid = false;
      Slot* slot = nullptr;
      long long first_index = -1;  // counter sampler: global index of the batch's first sample (-1: host blueprints)
      int n = 0;
      unsigned long long* box_cur = nullptr;
      const DevCropRef* croptab = nullptr;
      Event* ev = nullptr;         // profiled launch: its event set
      hipStream_t stream = nullptr;  // where the preparation was enqueued
      long long ticket = -1;       // the batch's number (its error word)
      bool ahead = false;          // prepared by an EARLIER call (look-ahead): the end of its preparation says nothing about when compose could start
      int base = 0;                // its first sample in the slot (a slot filled for N batches: part k starts at k x n)
    } prep;
    // The shared front end (ofdg_set_front_batches): the sampler -> geom -> raster launches of a counter-sampler call fill the
    // private slot for a GROUP of N batches, the call's own (part 0) and the ones this chain is asked for next.  `rest` are the
    // parts 1 .. N - 1 that still wait for their calls, in the order they will be asked for (rest_next is the next one): sampled,
    // outlined and rasterised in samples [k n, (k + 1) n) of the slot, their background preparation and their compose still to
    // be enqueued (launch_next_part).  Everything that forgets `prep` forgets them all (discard_prepared).
    Prepared rest[kMaxFrontBatches - 1];
    int rest_next = 0;
    bool fresh = true;  // no group since the start or since parts were discarded: the next group is a first one (kFrontFirstGroup)
    Prepared* next_part() { return rest_next < kMaxFrontBatches - 1 && rest[rest_next].valid ? &rest[rest_next] : nullptr; }
  };
  static constexpr int kMaxChains = 8;
  Chain chains[kMaxChains];
  int lookahead = 0;      // counter sampler: batches prepared ahead of the call that composes them (0: none)
  int front_batches = kFrontDefault;  // counter sampler: batches of a chain one sampler -> geom -> raster launch serves (ofdg_set_front_batches)
  std::string info_head;  // ofdg_ctx_info without its " front=N"
  long long last_first = -1;  // first index of the previous ofdg_forward_counter call (the stride of the caller's sequence)
  int n_chains = 3;       // one hardware queue each: HIP maps streams onto GPU_MAX_HW_QUEUES (4 by default) queues
  unsigned next_chain = 0;
  int last_chain = 0;     // the chain and the slot the last launch used (ofdg_render_resident, debug read-back)
  Slot* last_slot = nullptr;
  int last_base = 0, last_n = 0;       // ... and the samples of that slot the last launch composed (a slot may hold several batches)
  Chain* last_ch = nullptr;            // the chain that composed the batch in last_slot ...
  hipStream_t last_stream = nullptr;   // ... and the internal stream that call worked on (ofdg_object_table: OFDG_STREAM_OWN)
  hipStream_t last_user_st = nullptr;  // serial mode: the caller's stream of the last launch
  bool have_last_user_st = false;
  // device counter sampler (OFDG_SAMPLER_COUNTER)
  CsMode cs_mode;
  DevBuf<ofdg_blueprint> d_cs_bps;
  DevBuf<int> d_cs_nobj;
  long long next_index = 0;  // next global sample index of this rank's stream
  long long last_ticket = -1;  // ticket of the batch the last render / forward call composed
  // mode 9: served warp crops, each 4 planes of (W+1)*(H+1) floats, contiguous
  DevBuf<float> d_warp;            // [n_crops][2 pairs][(H+1)][(W+1)][2]: (flow x, flow y), (iflow x, iflow y) interleaved
  DevBuf<unsigned> d_warp_max;     // [n_crops] float bits of max |iflow|
  // counter sampler, mode 9: every crop as the kernels see it, [k] the crop itself (foreground), [n_crops + k] its
  // 2W x 2H upscaled copy (backgrounds); built once per set of crops
  DevBuf<DevCropRef> d_cs_croptab;
  DevBuf<float> d_cs_bgwarp;
  DevBuf<unsigned> d_cs_bgwarp_max;
  CropServer crop_server;
  int rs_w = 0, rs_h = 0;          // CImg resize tables for the background crops
  DevBuf<int> d_rs_xi, d_rs_yi;
  DevBuf<double> d_rs_xa, d_rs_ya;
  bool overlap = true;
  DevBuf<double> d_cs_tab;
  // Device error flags, ONE WORD PER CALL: call number q ("ticket") raises its flags in word q mod kErrWords, so that a prefetch
  // ring can ask at a batch's hand-over whether THAT batch was truncated (ofdg_poll_errors_of) - the reference drops a bad
  // sample silently (DG:1285-1292).  A word is cleared when it is read; one that was never asked for is read by
  // ofdg_synchronize / ofdg_poll_errors.  For a caller that asks by ticket (a prefetch ring) a word must not carry what an
  // EARLIER owner left in it - a look-ahead preparation that was discarded, a batch the caller never asked about: once
  // anybody has asked by ticket, a word that was not read since its last use is cleared on the chain's stream in front of
  // the first kernel of the call that takes it over (`word_clean`, launch_prepare).  A caller that only ever uses the
  // device-wide forms (bench.py) pays nothing.  Word kErrWords belongs to the debug entry points.
  static constexpr int kErrWords = 256;
  DevBuf<uint32_t> d_err;        // [kErrWords + 1]
  bool asked_by_ticket = false;  // ofdg_poll_errors_of has been called on this context
  bool word_clean[kErrWords];    // the word holds nothing of a call before the one that owns it now (all true at creation)
  long long word_reserved = -1;  // the ticket whose word an upload's background preparation already writes into (ofdg_upload_slot)
  long long ticket = 0;          // calls made so far = the ticket of the next call
  // background_prep = 1: CImg's enlarging tables for every source length below 2W (x) / 2H (y), tabulated once
  DevBuf<uint16_t> d_bg_at_x, d_bg_at_y;
  DevBuf<double> d_bg_alpha_x, d_bg_alpha_y;
  int bg_tab_w = 0, bg_tab_h = 0;
  int bg_cap_cw = 0, bg_cap_ch = 0, bg_cap_n = -1;  // bgprep_caps of the current pool (reset when the pool changes)
  bool bg_fusable = false;
  PinnedBuf h_err;                  // pinned copy for ofdg_poll_errors, on its own stream
  Stream err_stream;
  // profiling: ring of event sets, 6 events per launch: start/stop of geom, raster and compose,
  // attached to the kernels' own dispatch packets
  int profiling = 0;  // 0 off, 1 compose kernel only, 2 all three kernels
  std::vector<Event> ev;
  int ev_sets = 0, ev_stride = 1;
  long long ev_count = 0, ev_alloc = 0, launch_count = 0;  // event sets: composed / handed out (a prepared batch holds one)
  std::vector<char> ev_composed;  // per set: its compose was enqueued (a prepared batch that is discarded leaves its set incomplete)
  std::vector<char> ev_bgprep;    // per set: the batch's background preparation ran behind raster and is timed (ev[3] .. ev[2] or ev[4])
  std::vector<char> ev_front;     // per set: geom and raster were launched for it (a batch served from a later part of a group has neither)
  std::vector<ofdg_task> fw_tasks;
  std::vector<ofdg_blueprint> fw_bps;
};

#define HIP_OK(ctx, call)                                                                     \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
      return OFDG_EHIP;                                                                       \
    }                                                                                         \
  } while (0)
// ... and for the functions of this file that return an OFDG_* code themselves
#define OFDG_TRY(expr)                                                                        \
  do {                                                                                        \
    const int rc_ = (expr);                                                                   \
    if (rc_ != OFDG_OK) return rc_;                                                           \
  } while (0)

// One kernel launch with events on its own dispatch packet (`start` / `stop`, either may be null).  An argument has its
// parameter's type or, for a pointer parameter, converts to it implicitly - or is a void*: an output buffer travels as void* and
// arrives as the float* of the float32 kernels.  Nothing else compiles (no int for a float, no pointer of another type).
template <typename P, typename A>
constexpr bool kArgFits = std::is_same<A, P>::value ||
                          (std::is_pointer<P>::value && (std::is_convertible<A, P>::value || std::is_same<A, void*>::value));
struct Launch { unsigned grid, block; hipStream_t stream; hipEvent_t start, stop; };
template <typename... P, typename... A>
static void launch_kernel(const Launch& l, void (*kernel)(P...), A... args) {
  static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
  static_assert((kArgFits<P, A> && ...), "an argument that is neither of its parameter's type nor a void* for a pointer");
  hipExtLaunchKernelGGL(kernel, dim3(l.grid), dim3(l.block), 0, l.stream, l.start, l.stop, 0, static_cast<P>(args)...);
}

// the error word of the call being made (its ticket is taken - c->ticket advanced - when the call's first kernel is enqueued)
static uint32_t* err_word(ofdg_ctx* c, long long ticket) { return c->d_err.p + (size_t)(ticket % ofdg_ctx::kErrWords); }
// The call with this ticket is about to enqueue its first kernel on `s`: what an earlier owner left in its word goes first
// (only for callers that ask by ticket; see ofdg_ctx::word_clean).
static hipError_t take_err_word(ofdg_ctx* c, long long ticket, hipStream_t s) {
  const size_t i = (size_t)(ticket % ofdg_ctx::kErrWords);
  hipError_t e = hipSuccess;
  if (c->word_reserved == ticket) c->word_reserved = -1;  // (an upload for this very call already raised its flags here: they are this call's)
  else if (c->asked_by_ticket && !c->word_clean[i]) e = hipMemsetAsync(c->d_err.p + i, 0, sizeof(uint32_t), s);
  c->word_clean[i] = false;
  return e;
}
static std::string err_text(uint32_t e) {
  std::string t = "device capacity exceeded:";
  if (e & kErrVertCapacity) t += " outline vertices > 1024;";
  if (e & kErrCurveCapacity) t += " curve3 subdivision points/depth;";
  if (e & kErrDxLimit) t += " edge spans >= 16384 px;";
  if (e & kErrBgPrepCapacity) t += " background_prep: crop of the rotated image exceeds the workspace (zoom < 0.75);";
  return t;
}

// ---- Post-processing of planes the caller holds: ofdg_object_table, ofdg_flow_stats, ofdg_flow_pyramid, ofdg_crop, ofdg_photo,
// ofdg_spatial, ofdg_pack, ofdg_boundaries, ofdg_erase, ofdg_jitter, ofdg_camera, ofdg_motion_blur, ofdg_reproject, ofdg_splat, ofdg_flow_vis,
// ofdg_flow_error, ofdg_lens, ofdg_jpeg
// How each of them opens: the entry's name in front of every refusal, the job and its plane size, the alignment of its
// planes, its stream - in that order, which is the order of the refusals.
struct PostOp {
  ofdg_ctx* c;
  const char* who;  // the entry's name in the error text
  int fail(const std::string& why) const { c->err = std::string(who) + ": " + why; return OFDG_EINVAL; }
  // A job-struct entry's first lines: the context, the job as the kernels take it (Dev: what arg_error takes), its plane size
  // (the job's own, else the context's frame) and the rules the entry shares with its host twin.  more: arg_error's with_work.
  template <typename Dev, typename Job, typename... More>
  int open(const Job* job, int n_samples, const char* (*plane_size)(const Dev&, int*, int*),
           const char* (*arg_error)(const Dev*, int, int, int, More...), const Dev** j, int* W, int* H, More... more) const {
    if (!c) return OFDG_EINVAL;
    *j = reinterpret_cast<const Dev*>(job);
    if (!*j) return fail("job is NULL");
    *W = c->prm.width, *H = c->prm.height;
    if (const char* why = plane_size(**j, W, H)) return fail(why);
    if (const char* why = arg_error(*j, n_samples, *W, *H, more...)) return fail(why);
    return OFDG_OK;
  }
  // a plane the kernels write, or a record array, in 16-byte pieces (NULL: not given); its name in up to three parts
  int aligned16(const void* p, const char* name, const char* name2 = "", const char* name3 = "") const {
    return ((uintptr_t)p & 15) ? fail(std::string(name) + name2 + name3 + " must be 16-byte aligned") : OFDG_OK;
  }
  // an input plane of element type fmt (NULL: not given) at the alignment the kernels read it with (plane_alignment)
  int aligned(const std::string& name, const void* p, int fmt, bool say_fmt = true) const {
    if (!plane_misaligned(p, fmt)) return OFDG_OK;
    return fail(name + " must be " + std::to_string(plane_alignment(fmt)) + "-byte aligned" + (say_fmt ? std::string(" (") + fmt_name(fmt) + ")" : ""));
  }
  // the frames and records of a frame-pair job (photo, jitter, camera, jpeg) as those take them
  template <typename Job>
  int frame_pair_aligned(const Job& j) const {
    for (int f = 0; f < 2; ++f) {
      if (!j.src[f]) continue;
      OFDG_TRY(aligned(f ? "src[image1]" : "src[image0]", j.src[f], j.src_fmt, /*say_fmt=*/false));
      OFDG_TRY(aligned16(j.dst[f], f ? "dst[image1]" : "dst[image0]"));
    }
    OFDG_TRY(aligned16(j.recs, "recs"));
    return aligned16(j.recs_out, "recs_out");
  }
  // `stream` of the call; OFDG_STREAM_OWN: the internal stream the last render / forward call worked on
  int stream_of(void* stream, hipStream_t* st) const {
    if (stream == OFDG_STREAM_OWN && !c->last_ch) return fail("stream: OFDG_STREAM_OWN before any render / forward call on this context");
    *st = stream == OFDG_STREAM_OWN ? c->last_stream : (hipStream_t)stream;
    return OFDG_OK;
  }
};
// A run-time value as a template argument: f(std::integral_constant<T, V>) for the V among Vs that v equals.  The lists at
// the call sites are the instantiations that exist: 6 flow_stats_kernel, 12 flow_pyramid_kernel, 8 crop_kernel, 4 photo_kernel,
// 8 spatial_kernel, 24 pack_kernel, 4 boundary_kernel, 2 erase_mean_kernel, 8 erase_apply_kernel, 8 mblur_kernel,
// 4 reproject_kernel, 2 splat_scatter_kernel, 4 splat_resolve_kernel, 2 jitter_mean_kernel, 4 jitter_apply_kernel,
// 2 flow_vis_max_kernel, 12 flow_vis_colour_kernel, 12 flow_error_kernel, 4 camera_kernel, 8 lens_kernel, 4 jpeg_kernel.
template <class T, T... Vs, class F>
static void with_constant(T v, F&& f) {
  (void)(... || (v == Vs && (f(std::integral_constant<T, Vs>{}), true)));
}
template <class F>
static void with_bool(bool v, F&& f) { with_constant<bool, false, true>(v, f); }
// the kernels' kOcc of an optional occlusion map: 0 no map, 1 float32, 2 uint8
template <class F>
static void with_occ_kind(const void* d_occ, int occ_fmt, F&& f) { with_constant<int, 0, 1, 2>(!d_occ ? 0 : occ_fmt == OFDG_FMT_U8 ? 2 : 1, f); }

static int discard_all_prepared(ofdg_ctx* c);
static int texture_of_image(ofdg_ctx* c, const uint32_t* image, int w, int h, int tw, int th, uint32_t* out);

extern "C" {

const char* ofdg_last_error(const ofdg_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int ofdg_create(const ofdg_params* params, ofdg_ctx** out) {
  if (!params || !out) { g_create_error = "null argument"; return OFDG_EINVAL; }
  *out = nullptr;
  if (params->mode < 1 || params->mode > 13) { g_create_error = "BAD MODE"; return OFDG_EBADMODE; }
  if (params->width < 8 || params->height < 2 || (params->width % 8) != 0 || (params->height % 2) != 0) {
    g_create_error = "width must be a multiple of 8 and height even";
    return OFDG_EINVAL;
  }
  {  // a sample holds at most 64 foreground objects (bits of a block mask); the device sampler generates at most 32
    const int cap = params->sampler == OFDG_SAMPLER_COUNTER ? kCsMaxObjects : kMaxFgObjects;
    if (params->num_objects < 0 || params->num_objects > cap) {
      g_create_error = "num_objects must be 0 (reference: 16..23) or 1.." + std::to_string(cap) + " for this sampler";
      return OFDG_EINVAL;
    }
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_error = "no HIP device available (the HIP kernels are the only render path)";
    return OFDG_EHIP;
  }
  e = hipSetDevice(params->device);
  if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return OFDG_EHIP; }
  std::unique_ptr<ofdg_ctx> c(new ofdg_ctx());  // (an early return below frees what the context holds by then)
  std::fill(c->word_clean, c->word_clean + ofdg_ctx::kErrWords, true);
  c->prm = *params;
  if (c->prm.world_size < 1) c->prm.world_size = 1;
  c->sampler.reset(new RefSampler(params->mode, params->width, params->height, params->num_objects));
  if (!c->sampler->ok()) { g_create_error = "BAD MODE"; return OFDG_EBADMODE; }
  c->cs_mode = make_cs_mode(params->mode, params->width, params->height, params->num_objects, (uint32_t)params->seed);  // the device sampler's constants
  // cos/sin of agg::ellipse's 100 step angles, from the host libm
  double tab[200];
  const double pi = 3.14159265358979323846;
  for (int step = 0; step < 100; ++step) {
    const double angle = double(step) / double(100) * 2.0 * pi;
    tab[2 * step] = std::cos(angle);
    tab[2 * step + 1] = std::sin(angle);
  }
  if ((e = c->d_cs_tab.alloc(sizeof(tab) / sizeof(tab[0]))) != hipSuccess ||
      (e = hipMemcpy(c->d_cs_tab.p, tab, sizeof(tab), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = c->d_err.alloc(ofdg_ctx::kErrWords + 1)) != hipSuccess ||
      (e = hipMemset(c->d_err.p, 0, (ofdg_ctx::kErrWords + 1) * sizeof(uint32_t))) != hipSuccess ||
      (e = c->user_stage.free_ev.create(hipEventDisableTiming)) != hipSuccess) {
    g_create_error = std::string("HIP initialisation: ") + hipGetErrorString(e);
    return OFDG_EHIP;
  }
  c->overlap = params->serial == 0;  // serial: everything on the caller's stream
  c->lookahead = std::max(params->lookahead, 0);
  // One hardware queue per chain: HIP maps its streams onto GPU_MAX_HW_QUEUES (default 4) queues.  A process started
  // with GPU_MAX_HW_QUEUES >= 8 gets four chains (+5-8 % throughput, profiles/r02_chains_vs_hw_queues.txt); four chains
  // on four queues share a queue with the caller's streams and are slower than three.
  c->n_chains = params->chains > 0 ? std::min(params->chains, (int)ofdg_ctx::kMaxChains) : (g_hw_queues_env >= 8 ? 4 : 3);
  c->info_head = "chains=" + std::to_string(c->n_chains) +
            (params->chains > 0 ? " (ofdg_params.chains)"
             : g_hw_queues_env >= 8 ? " (GPU_MAX_HW_QUEUES=" + std::to_string(g_hw_queues_env) + ": one hardware queue per chain)"
             : g_hw_queues_env > 0 ? " (GPU_MAX_HW_QUEUES=" + std::to_string(g_hw_queues_env) + " < 8: start the process with GPU_MAX_HW_QUEUES=8 for four chains, +5-8 %)"
                                   : " (GPU_MAX_HW_QUEUES was not set when the library was loaded: HIP's default of 4 hardware queues; start the process with GPU_MAX_HW_QUEUES=8 for four chains, +5-8 %)") +
            " lookahead=" + std::to_string(c->lookahead) + (c->overlap ? "" : " serial");
  c->info = c->info_head + " front=" + std::to_string(c->front_batches);
  for (int i = 0; i < c->n_chains; ++i) {
    ofdg_ctx::Chain& ch = c->chains[i];
    if ((e = ch.stream.create(hipStreamNonBlocking)) != hipSuccess ||
        (e = ch.stage.free_ev.create(hipEventDisableTiming)) != hipSuccess ||
        (e = ch.ev_prep.create(hipEventDisableTiming)) != hipSuccess ||
        (e = ch.ev_done.create(hipEventDisableTiming)) != hipSuccess) {
      g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e);
      return OFDG_EHIP;
    }
  }
  // fail early (and loudly) if the gfx950 code object is not usable on this device
  {
    hipFuncAttributes fa;
    e = hipFuncGetAttributes(&fa, (const void*)compose_rigid_kernel);
    if (e != hipSuccess) {
      g_create_error = std::string("compose_rigid_kernel is not loadable (is the gfx950 code object present?): ") + hipGetErrorString(e);
      return OFDG_EHIP;
    }
  }
  *out = c.release();
  return OFDG_OK;
}

const ofdg_params* ofdg_ctx_params(const ofdg_ctx* c) { return c ? &c->prm : nullptr; }
const char* ofdg_ctx_info(const ofdg_ctx* c) { return c ? c->info.c_str() : ""; }

void ofdg_destroy(ofdg_ctx* c) {
  if (!c) return;
  (void)hipDeviceSynchronize();  // (nothing is freed under a kernel that still runs)
  delete c;
}

// ---- texture pool -------------------------------------------------------------------
static int pool_check_dims(ofdg_ctx* c, int n, int w, int h) {
  const int W = c->prm.width, H = c->prm.height;
  if (n < 1) { c->err = "texture pool needs at least one image"; return OFDG_ETEXTURES; }
  (void)W; (void)H;
  if (w < 2 || h < 2) { c->err = "pool images must be at least 2 x 2"; return OFDG_ETEXTURES; }
  return OFDG_OK;
}

int ofdg_pool_alloc(ofdg_ctx* c, int n, int w, int h) {
  if (!c) return OFDG_EINVAL;
  OFDG_TRY(discard_all_prepared(c));  // (batches prepared ahead read the old pool / crops)
  OFDG_TRY(pool_check_dims(c, n, w, h));
  HIP_OK(c, hipDeviceSynchronize());
  HIP_OK(c, c->pool.alloc((size_t)n * w * h));
  HIP_OK(c, hipMemset(c->pool.p, 0, (size_t)n * w * h * sizeof(uint32_t)));
  c->pool_n = n; c->pool_w = w; c->pool_h = h;
  c->pool_final = false;
  c->pool_mixed = false;
  c->pool_kind = OFDG_POOL_UNIFORM;
  return OFDG_OK;
}

// A pool of n images of DIFFERENT sizes (real texture lists): only what the path reads is kept - every
// image's W x H foreground texture and 2W x 2H background texture (centre crop, or the resized image if
// it is smaller; DG:96-106), in two uniform arrays.  background_prep needs the originals: not available here.
int ofdg_pool_alloc_mixed(ofdg_ctx* c, int n) {
  if (!c) return OFDG_EINVAL;
  OFDG_TRY(discard_all_prepared(c));  // (batches prepared ahead read the old pool / crops)
  if (n < 1) { c->err = "texture pool needs at least one image"; return OFDG_ETEXTURES; }
  const int W = c->prm.width, H = c->prm.height;
  HIP_OK(c, hipDeviceSynchronize());
  c->mixed_images.clear();
  c->mixed_images.resize((size_t)n);
  c->d_tex_table.release();
  c->tex_table.clear();
  c->pool.release(); c->pool_fg.release(); c->pool_bg.release();  // (all three go before the new ones come)
  HIP_OK(c, c->pool_fg.alloc((size_t)n * W * H));
  HIP_OK(c, c->pool_bg.alloc((size_t)n * 4 * W * H));
  HIP_OK(c, hipMemset(c->pool_fg.p, 0, (size_t)n * W * H * sizeof(uint32_t)));
  HIP_OK(c, hipMemset(c->pool_bg.p, 0, (size_t)n * 4 * W * H * sizeof(uint32_t)));
  HIP_OK(c, hipDeviceSynchronize());
  c->pool_n = n; c->pool_w = 0; c->pool_h = 0;
  c->fg_src = TexSource{(uint64_t)W * H, 0, W, 0};
  c->bg_src = TexSource{(uint64_t)4 * W * H, 0, 2 * W, 0};
  c->pool_mixed = true;
  c->pool_final = true;
  c->pool_kind = OFDG_POOL_MIXED;
  c->mixed_sizes.assign((size_t)n, std::make_pair(0, 0));
  return OFDG_OK;
}

// image `index` of a mixed pool: planar B,G,R u8 of any size >= 2 x 2
int ofdg_pool_upload_mixed(ofdg_ctx* c, int index, const uint8_t* bgr_planar, int w, int h) {
  if (!c || !bgr_planar) return OFDG_EINVAL;
  OFDG_TRY(discard_all_prepared(c));  // (batches prepared ahead read the old pool / crops)
  if (!c->pool_mixed || index < 0 || index >= c->pool_n || w < 2 || h < 2) {
    c->err = "pool_upload_mixed: no mixed pool (ofdg_pool_alloc_mixed), bad index or image smaller than 2 x 2";
    return OFDG_ETEXTURES;
  }
  const int W = c->prm.width, H = c->prm.height;
  DevBuf<uint8_t> tmp;
  DevBuf<uint32_t> img;
  const size_t n = (size_t)w * h;
  HIP_OK(c, hipDeviceSynchronize());
  HIP_OK(c, tmp.alloc(3 * n));
  HIP_OK(c, img.alloc(n));
  HIP_OK(c, hipMemcpy(tmp.p, bgr_planar, 3 * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(pool_pack_kernel, dim3(1024), dim3(256), 0, 0, tmp.p, img.p, w, h);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipDeviceSynchronize());
  int rc = texture_of_image(c, img.p, w, h, W, H, c->pool_fg.p + (size_t)index * W * H);
  if (rc == OFDG_OK) rc = texture_of_image(c, img.p, w, h, 2 * W, 2 * H, c->pool_bg.p + (size_t)index * 4 * W * H);
  HIP_OK(c, hipDeviceSynchronize());
  if (rc == OFDG_OK && c->prm.background_prep) {  // the background preparation reads the original image
    c->mixed_images[(size_t)index] = std::move(img);  // (the image it replaces goes with `img`)
    c->d_tex_table.release();
  }
  if (rc == OFDG_OK) c->mixed_sizes[(size_t)index] = std::make_pair(w, h);
  return rc;
}

int ofdg_pool_synthetic(ofdg_ctx* c, int n, int w, int h, uint32_t seed) {
  OFDG_TRY(ofdg_pool_alloc(c, n, w, h));
  hipLaunchKernelGGL(pool_synth_kernel, dim3(256 * 8), dim3(256), 0, 0, c->pool.p, n, w, h, seed);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipDeviceSynchronize());
  c->pool_final = false;
  c->pool_kind = OFDG_POOL_SYNTHETIC;
  c->pool_seed = seed;
  return OFDG_OK;
}

int ofdg_pool_upload(ofdg_ctx* c, int index, const uint8_t* bgr_planar, int w, int h) {
  if (!c || !bgr_planar) return OFDG_EINVAL;
  OFDG_TRY(discard_all_prepared(c));  // (batches prepared ahead read the old pool / crops)
  if (!c->pool.p || index < 0 || index >= c->pool_n || w != c->pool_w || h != c->pool_h) {
    c->err = "pool_upload: index / size does not match the allocated pool";
    return OFDG_ETEXTURES;
  }
  DevBuf<uint8_t> tmp;
  const size_t n = (size_t)w * h;
  HIP_OK(c, tmp.alloc(3 * n));
  HIP_OK(c, hipMemcpy(tmp.p, bgr_planar, 3 * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(pool_pack_kernel, dim3(1024), dim3(256), 0, 0, tmp.p, c->pool.p + (size_t)index * n, w, h);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipDeviceSynchronize());
  c->pool_final = false;
  return OFDG_OK;
}

int ofdg_pool_download(ofdg_ctx* c, int index, uint8_t* bgr_planar) {
  if (!c || !bgr_planar) return OFDG_EINVAL;
  if (!c->pool.p || index < 0 || index >= c->pool_n) { c->err = "pool_download: bad index"; return OFDG_ETEXTURES; }
  DevBuf<uint8_t> tmp;
  const size_t n = (size_t)c->pool_w * c->pool_h;
  HIP_OK(c, tmp.alloc(3 * n));
  hipLaunchKernelGGL(pool_unpack_kernel, dim3(1024), dim3(256), 0, 0, c->pool.p + (size_t)index * n, tmp.p, c->pool_w, c->pool_h);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipMemcpy(bgr_planar, tmp.p, 3 * n, hipMemcpyDeviceToHost));  // (waits for the kernel: tmp is idle when it goes)
  return OFDG_OK;
}

int ofdg_pool_info(const ofdg_ctx* c, int* n, int* w, int* h) {
  if (!c) return OFDG_EINVAL;
  if (n) *n = c->pool_n;
  if (w) *w = c->pool_w;
  if (h) *h = c->pool_h;
  return OFDG_OK;
}

// The resident pool as raw device memory (n * h * w BGRX texels): for filling it from another GPU - rank 0 loads
// the texture collection, the other ranks receive it with one RCCL broadcast over xGMI into their own replica.
// `mark_written` != 0 tells the context that the contents changed (derived textures are rebuilt at the next use).
int ofdg_pool_device(ofdg_ctx* c, void** ptr, unsigned long long* bytes, int mark_written) {
  if (!c || !ptr || !bytes) return OFDG_EINVAL;
  if (!c->pool.p || c->pool_mixed) { c->err = "pool_device: needs a pool of one image size (ofdg_pool_alloc / ofdg_pool_synthetic)"; return OFDG_ETEXTURES; }
  HIP_OK(c, hipDeviceSynchronize());
  *ptr = (void*)c->pool.p;
  *bytes = (unsigned long long)c->pool_n * c->pool_w * c->pool_h * sizeof(uint32_t);
  if (mark_written) {
    c->pool_final = false;
    OFDG_TRY(discard_all_prepared(c));  // (batches prepared ahead would render the old contents)
  }
  return OFDG_OK;
}

int ofdg_pool_device_mixed(ofdg_ctx* c, void** fg, unsigned long long* fg_bytes, void** bg, unsigned long long* bg_bytes) {
  if (!c || !fg || !fg_bytes || !bg || !bg_bytes) return OFDG_EINVAL;
  if (!c->pool_mixed) { c->err = "pool_device_mixed: needs a mixed pool (ofdg_pool_alloc_mixed)"; return OFDG_ETEXTURES; }
  OFDG_TRY(discard_all_prepared(c));  // (the caller is about to write the textures)
  HIP_OK(c, hipDeviceSynchronize());
  const unsigned long long px = (unsigned long long)c->prm.width * c->prm.height;
  *fg = (void*)c->pool_fg.p; *fg_bytes = (unsigned long long)c->pool_n * px * sizeof(uint32_t);
  *bg = (void*)c->pool_bg.p; *bg_bytes = (unsigned long long)c->pool_n * 4 * px * sizeof(uint32_t);
  return OFDG_OK;
}

// ---- multi-GPU start-up: what the root broadcasts (csrc/comm.cpp) ------------------------------------
int ofdg_setup_of(const ofdg_ctx* c, ofdg_setup* su, ofdg_tex_entry* table, int table_cap) {
  if (!c || !su || table_cap < 0 || (table_cap > 0 && !table)) return OFDG_EINVAL;
  std::memset(su, 0, sizeof(*su));
  const ofdg_params& p = c->prm;
  su->seed = p.seed; su->mode = p.mode; su->width = p.width; su->height = p.height; su->num_objects = p.num_objects;
  su->use_antialiasing = p.use_antialiasing; su->batch_size = p.batch_size; su->sampler = p.sampler;
  su->background_prep = p.background_prep; su->max_shapes_per_sample = p.max_shapes_per_sample;
  // (a pool of images of different sizes needs every entry of the table: a table that does not fit is the root's failure,
  //  which the broadcast carries to every rank)
  if (c->pool_mixed && c->pool_n > table_cap) su->status = OFDG_ECAPACITY;
  su->n_tex = c->pool_n; su->pool_kind = c->pool_kind; su->pool_w = c->pool_w; su->pool_h = c->pool_h; su->pool_seed = c->pool_seed;
  su->n_table = std::min(c->pool_n, table_cap);
  const uint64_t W = (uint64_t)p.width, H = (uint64_t)p.height;
  for (int i = 0; i < su->n_table; ++i) {
    ofdg_tex_entry& e = table[i];
    std::memset(&e, 0, sizeof(e));
    if (c->pool_mixed) {  // the path reads the derived [n][H][W] foreground textures
      e.offset = (uint64_t)i * W * H; e.pitch = (uint32_t)W;
      e.w = (uint32_t)c->mixed_sizes[(size_t)i].first; e.h = (uint32_t)c->mixed_sizes[(size_t)i].second;
    } else {
      e.offset = (uint64_t)i * (uint64_t)c->pool_w * (uint64_t)c->pool_h; e.pitch = (uint32_t)c->pool_w;
      e.w = (uint32_t)c->pool_w; e.h = (uint32_t)c->pool_h;
    }
  }
  return OFDG_OK;
}

int ofdg_setup_alloc_pool(ofdg_ctx* c, const ofdg_setup* su, const ofdg_tex_entry* table) {
  if (!c || !su) return OFDG_EINVAL;
  OFDG_TRY(discard_all_prepared(c));  // (batches prepared ahead read the old pool / crops)
  if (su->width != c->prm.width || su->height != c->prm.height) { c->err = "setup_alloc_pool: the context was not created from this setup"; return OFDG_EINVAL; }
  if (su->pool_kind == OFDG_POOL_SYNTHETIC) return ofdg_pool_synthetic(c, su->n_tex, su->pool_w, su->pool_h, su->pool_seed);
  if (su->pool_kind != OFDG_POOL_MIXED) return ofdg_pool_alloc(c, su->n_tex, su->pool_w, su->pool_h);
  OFDG_TRY(ofdg_pool_alloc_mixed(c, su->n_tex));
  if (!table || su->n_table < su->n_tex) { c->err = "setup_alloc_pool: a mixed pool needs the index table (image sizes)"; return OFDG_EINVAL; }
  for (int i = 0; i < su->n_tex; ++i) {
    c->mixed_sizes[(size_t)i] = std::make_pair((int)table[i].w, (int)table[i].h);
    if (c->prm.background_prep)  // the whole images arrive with ofdg_comm_bcast_pool
      HIP_OK(c, c->mixed_images[(size_t)i].alloc((size_t)table[i].w * table[i].h));
  }
  return OFDG_OK;
}

// image `index` of a mixed pool kept whole for the background preparation, as raw device memory (w * h BGRX texels)
int ofdg_pool_device_image(ofdg_ctx* c, int index, void** ptr, unsigned long long* bytes) {
  if (!c || !ptr || !bytes) return OFDG_EINVAL;
  if (!c->pool_mixed || !c->prm.background_prep || index < 0 || index >= c->pool_n || !c->mixed_images[(size_t)index].p) {
    c->err = "pool_device_image: no whole image " + std::to_string(index) + " (mixed pool with background_prep only)";
    return OFDG_ETEXTURES;
  }
  HIP_OK(c, hipDeviceSynchronize());
  *ptr = (void*)c->mixed_images[(size_t)index].p;
  *bytes = (unsigned long long)c->mixed_sizes[(size_t)index].first * c->mixed_sizes[(size_t)index].second * sizeof(uint32_t);
  return OFDG_OK;
}

// ---- sampler ---------------------------------------------------------------------------
int ofdg_sample(ofdg_ctx* c, int n_tasks, ofdg_task* tasks, ofdg_blueprint* bps, int bps_capacity, int* n_bps) {
  if (!c || !tasks || !bps || !n_bps || n_tasks < 0) return OFDG_EINVAL;
  if (c->prm.sampler != OFDG_SAMPLER_REF) { c->err = "only OFDG_SAMPLER_REF is implemented on the host"; return OFDG_EINVAL; }
  std::vector<ofdg_blueprint> pool;
  for (int i = 0; i < n_tasks; ++i) {
    OFDG_TRY(c->sampler->next_task(&pool, &tasks[i], &c->err));
  }
  *n_bps = (int)pool.size();
  if ((int)pool.size() > bps_capacity) { c->err = "blueprint capacity exceeded"; return OFDG_ECAPACITY; }
  std::memcpy(bps, pool.data(), pool.size() * sizeof(ofdg_blueprint));
  return OFDG_OK;
}

// block masks of a slot: two parities, cleared once here; afterwards raster_kernel clears
// the other parity every launch
static int reserve_blockmask(ofdg_ctx* c, ofdg_ctx::Slot& sl, int n_samples) {
  const int W = c->prm.width, H = c->prm.height;
  const size_t words = (size_t)n_samples * ((W + kTileW - 1) / kTileW) * ((H + kBandRows - 1) / kBandRows) * 2;
  if (words > sl.box_stride) {
    HIP_OK(c, hipDeviceSynchronize());
    HIP_OK(c, sl.d_blockmask.reserve((words + 16) * 2));
    sl.box_stride = sl.d_blockmask.cap / 2;
    HIP_OK(c, hipMemset(sl.d_blockmask.p, 0, sl.d_blockmask.cap * sizeof(unsigned long long)));
    HIP_OK(c, hipDeviceSynchronize());  // (the fill runs on the null stream; the kernels use non-blocking streams)
    sl.mask_used[0] = sl.mask_used[1] = 0;
  }
  return OFDG_OK;
}

// CImg linear resize tables (X then Y), boundary 0, upscaling branch: (W+1) x (H+1) -> 2W x 2H (DG:1197-1200)
static int ensure_resize_tables(ofdg_ctx* c) {
  const int W = c->prm.width, H = c->prm.height;
  if (c->rs_w == W && c->rs_h == H) return OFDG_OK;
  auto table = [&](int w, int sx, DevBuf<int>& d_at, DevBuf<double>& d_alpha) -> int {
    std::vector<int> at(sx);
    std::vector<double> alpha(sx);
    cimg_enlarge_table(w, sx, at.data(), alpha.data());
    HIP_OK(c, d_at.alloc(at.size()));
    HIP_OK(c, d_alpha.alloc(alpha.size()));
    HIP_OK(c, hipMemcpy(d_at.p, at.data(), at.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(c, hipMemcpy(d_alpha.p, alpha.data(), alpha.size() * sizeof(double), hipMemcpyHostToDevice));
    return OFDG_OK;
  };
  OFDG_TRY(table(W + 1, 2 * W, c->d_rs_xi, c->d_rs_xa));
  OFDG_TRY(table(H + 1, 2 * H, c->d_rs_yi, c->d_rs_ya));
  c->rs_w = W; c->rs_h = H;
  return OFDG_OK;
}

// mode 9: a (W+1) x (H+1) warp crop upscaled on stream `s` into the 2W x 2H crop `dst` a background reads; returns dst's table entry
static int upscale_crop(ofdg_ctx* c, const float* src, float* dst, unsigned* dst_max, hipStream_t s, DevCropRef* ref) {
  const int W = c->prm.width, H = c->prm.height;
  hipLaunchKernelGGL(wf_resize2_kernel, dim3((2 * W * 2 * H + 255) / 256), dim3(256), 0, s, src, W + 1, H + 1, 2 * W, 2 * H,
                     c->d_rs_xi.p, c->d_rs_xa.p, c->d_rs_yi.p, c->d_rs_ya.p, dst, dst_max);
  HIP_OK(c, hipGetLastError());
  *ref = make_crop_ref(dst, dst_max, 2 * W, 2 * H);
  return OFDG_OK;
}

// counter sampler, mode 9: the static crop table (see ofdg_ctx::d_cs_croptab)
static int ensure_counter_croptab(ofdg_ctx* c) {
  if (c->d_cs_croptab.p) return OFDG_OK;
  const int n = c->crop_server.n_crops;
  if (!c->d_warp.p || n < 1) { c->err = "mode 9 needs warp fields: call ofdg_warp_generate or ofdg_warp_upload first"; return OFDG_EINVAL; }
  OFDG_TRY(ensure_resize_tables(c));
  const int W = c->prm.width, H = c->prm.height;
  const size_t crop_floats = (size_t)4 * (W + 1) * (H + 1), bg_floats = (size_t)4 * 2 * W * 2 * H;
  HIP_OK(c, hipDeviceSynchronize());
  HIP_OK(c, c->d_cs_bgwarp.alloc((size_t)n * bg_floats));
  HIP_OK(c, c->d_cs_bgwarp_max.alloc((size_t)n));
  HIP_OK(c, hipMemset(c->d_cs_bgwarp_max.p, 0, (size_t)n * sizeof(unsigned)));
  HIP_OK(c, c->d_cs_croptab.alloc((size_t)2 * n));
  std::vector<DevCropRef> tab((size_t)2 * n);
  for (int k = 0; k < n; ++k) {
    const float* src = c->d_warp.p + (size_t)k * crop_floats;
    OFDG_TRY(upscale_crop(c, src, c->d_cs_bgwarp.p + (size_t)k * bg_floats, c->d_cs_bgwarp_max.p + k, 0, &tab[(size_t)n + k]));
    tab[k] = make_crop_ref(src, c->d_warp_max.p + k, W + 1, H + 1);
  }
  HIP_OK(c, hipMemcpy(c->d_cs_croptab.p, tab.data(), tab.size() * sizeof(DevCropRef), hipMemcpyHostToDevice));
  HIP_OK(c, hipDeviceSynchronize());
  return OFDG_OK;
}
static void drop_counter_croptab(ofdg_ctx* c) { c->d_cs_croptab.release(); c->d_cs_bgwarp.release(); c->d_cs_bgwarp_max.release(); }

// CImg<unsigned char>::get_resize(tw, th, -100, -100, 3) of every pool image (X pass, then Y pass, u8 in
// between) into dst[n][th][tw]
static int resize_images(ofdg_ctx* c, const uint32_t* images, int n, int w, int h, int tw, int th, uint32_t* out_images) {
  DevBuf<uint32_t> mid;  // [n][h][tw]
  HIP_OK(c, mid.alloc((size_t)n * tw * h));
  auto pass = [&](const uint32_t* src, uint32_t* out, int sw, int sh, int s, int along_x) -> int {
    const int len = along_x ? sw : sh;
    DevBuf<int> d_at;
    DevBuf<double> d_alpha;
    if (s > len) {  // enlarging
      std::vector<int> at(s);
      std::vector<double> alpha(s);
      cimg_enlarge_table(len, s, at.data(), alpha.data());
      HIP_OK(c, d_at.alloc(s));
      HIP_OK(c, d_alpha.alloc(s));
      HIP_OK(c, hipMemcpy(d_at.p, at.data(), s * sizeof(int), hipMemcpyHostToDevice));
      HIP_OK(c, hipMemcpy(d_alpha.p, alpha.data(), s * sizeof(double), hipMemcpyHostToDevice));
    }
    if (s == len) {
      HIP_OK(c, hipMemcpy(out, src, (size_t)n * sw * sh * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    } else {
      hipLaunchKernelGGL(pool_resize_axis_kernel, dim3(2048), dim3(256), 0, 0, src, out, n, sw, sh, s, along_x, d_at.p, d_alpha.p);
      HIP_OK(c, hipGetLastError());
    }
    HIP_OK(c, hipDeviceSynchronize());  // (the tables go with this scope)
    return OFDG_OK;
  };
  OFDG_TRY(pass(images, mid.p, w, h, tw, 1));
  return pass(mid.p, out_images, tw, h, th, 0);
}
static int pool_resized_copy(ofdg_ctx* c, int tw, int th, DevBuf<uint32_t>& dst) {
  HIP_OK(c, dst.alloc((size_t)c->pool_n * tw * th));
  return resize_images(c, c->pool.p, c->pool_n, c->pool_w, c->pool_h, tw, th, dst.p);
}
// the tw x th texture of ONE image of any size (getRandomizedCrop with default arguments, DG:96-106):
// its centre crop if it is large enough, else the resized whole image
static int texture_of_image(ofdg_ctx* c, const uint32_t* image, int w, int h, int tw, int th, uint32_t* out) {
  if (w >= tw && h >= th) {
    HIP_OK(c, hipMemcpy2D(out, (size_t)tw * 4, image + (size_t)(h / 2 - th / 2) * w + (w / 2 - tw / 2), (size_t)w * 4, (size_t)tw * 4, th,
                          hipMemcpyDeviceToDevice));
    return OFDG_OK;
  }
  return resize_images(c, image, 1, w, h, tw, th, out);
}

// after the pool contents are final: where foreground / background textures are read from
static int finalise_pool(ofdg_ctx* c) {
  if (c->pool_final) return OFDG_OK;
  if (c->pool_mixed) { c->pool_final = true; return OFDG_OK; }
  HIP_OK(c, hipDeviceSynchronize());
  const int W = c->prm.width, H = c->prm.height, w = c->pool_w, h = c->pool_h;
  const uint64_t img = (uint64_t)w * h;
  c->pool_fg.release();
  c->pool_bg.release();
  if (w >= W && h >= H) {
    c->fg_src = TexSource{img, (uint64_t)(h / 2 - H / 2) * w + (uint64_t)(w / 2 - W / 2), w, 0};
  } else {
    OFDG_TRY(pool_resized_copy(c, W, H, c->pool_fg));
    c->fg_src = TexSource{(uint64_t)W * H, 0, W, 0};
  }
  if (w >= 2 * W && h >= 2 * H) {
    c->bg_src = TexSource{img, (uint64_t)(h / 2 - H) * w + (uint64_t)(w / 2 - W), w, 0};
  } else {
    OFDG_TRY(pool_resized_copy(c, 2 * W, 2 * H, c->pool_bg));
    c->bg_src = TexSource{(uint64_t)4 * W * H, 0, 2 * W, 0};
  }
  c->pool_final = true;
  return OFDG_OK;
}

// background_prep on a mixed pool: the per-image table (address, size) on the device, and the workspace the staged chain
// needs for the largest crop of a rotated image
static int ensure_tex_table(ofdg_ctx* c) {
  if (!c->pool_mixed || !c->prm.background_prep || c->d_tex_table.p) return OFDG_OK;
  c->tex_table.resize((size_t)c->pool_n);
  for (int i = 0; i < c->pool_n; ++i) {
    if (!c->mixed_images[(size_t)i].p) { c->err = "background_prep: image " + std::to_string(i) + " of the mixed pool has not been uploaded"; return OFDG_ETEXTURES; }
    c->tex_table[(size_t)i] = DevTexEntry{(uint64_t)(uintptr_t)c->mixed_images[(size_t)i].p, c->mixed_sizes[(size_t)i].first, c->mixed_sizes[(size_t)i].second};
  }
  HIP_OK(c, c->d_tex_table.alloc(c->tex_table.size()));
  HIP_OK(c, hipMemcpy(c->d_tex_table.p, c->tex_table.data(), c->tex_table.size() * sizeof(DevTexEntry), hipMemcpyHostToDevice));
  return OFDG_OK;
}
// `fusable`: every pool image is at least 2W x 2H, so a crop is at most 4/3 of the texture (beyond that it is refused), which
// is what the tiles of bgprep_stream_kernel hold; smaller images are resized by any factor (DG:102-106): the two-kernel form
static void bgprep_caps(ofdg_ctx* c, int* cap_cw, int* cap_ch, bool* fusable) {
  if (c->bg_cap_n == c->pool_n && c->bg_cap_cw > 0) { *cap_cw = c->bg_cap_cw; *cap_ch = c->bg_cap_ch; *fusable = c->bg_fusable; return; }  // (per pool, not per step)
  const int TW = 2 * c->prm.width, TH = 2 * c->prm.height;
  // crops of the rotated image up to zoom 0.75 (the sampler draws 0.8 .. 1.2) ...
  int cw = (int)((float)TW / 0.75f) + 2, ch = (int)((float)TH / 0.75f) + 2;
  // ... or the whole rotated image when a pool image is smaller than 2W x 2H (DG:102-106; rotation by up to +-3.2 "degrees")
  bool all_large = true;
  auto small = [&](int w, int h) { if (w < TW || h < TH) { all_large = false; cw = std::max(cw, w + h / 8 + 4); ch = std::max(ch, h + w / 8 + 4); } };
  if (c->pool_mixed) for (const auto& wh : c->mixed_sizes) small(wh.first, wh.second);
  else small(c->pool_w, c->pool_h);
  c->bg_cap_cw = cw; c->bg_cap_ch = ch; c->bg_cap_n = c->pool_n; c->bg_fusable = all_large;
  *cap_cw = cw; *cap_ch = ch; *fusable = all_large;
}

// per-chain coverage workspaces of a batch of n_shapes outlines.  Growing them waits for the device: every chain may be
// reading its own.
static int reserve_workspaces(ofdg_ctx* c, size_t n_shapes) {
  const size_t need_cov = n_shapes * 2 * (size_t)c->prm.width * c->prm.height + 16;
  if (need_cov <= c->chains[0].cov.cap) return OFDG_OK;
  HIP_OK(c, hipDeviceSynchronize());
  for (int k = 0; k < c->n_chains; ++k) HIP_OK(c, c->chains[k].cov.reserve(need_cov));
  return OFDG_OK;
}

// the slot's count of raster work items: allocated, cleared and waited for once
static int ensure_item_count(ofdg_ctx* c, ofdg_ctx::Slot& sl) {
  if (sl.d_item_count.p) return OFDG_OK;
  HIP_OK(c, sl.d_item_count.alloc(1));
  HIP_OK(c, hipMemset(sl.d_item_count.p, 0, sizeof(int)));
  HIP_OK(c, hipDeviceSynchronize());
  return OFDG_OK;
}
// What slot `sl` (and the chains) need for a batch of n_samples samples with n_shapes outlines.  n_objects > 0: the records are
// written on the device (counter sampler), so the slot owns them too; 0: they are views of the uploaded arena (upload_slot).
// The reservations come in the order they always had.
static int size_slot(ofdg_ctx* c, ofdg_ctx::Slot& sl, int n_samples, size_t n_shapes, size_t n_objects = 0) {
  const int W = c->prm.width, H = c->prm.height;
  if (n_objects) HIP_OK(c, sl.d_shapes.reserve(n_shapes));
  HIP_OK(c, sl.d_frames.reserve(n_shapes * 2));
  HIP_OK(c, sl.d_verts.reserve(n_shapes * 2 * kMaxVerts));
  if (n_objects) {
    HIP_OK(c, sl.d_objects.reserve(n_objects));
    HIP_OK(c, sl.d_samples.reserve(n_samples));
  }
  OFDG_TRY(reserve_workspaces(c, n_shapes));
  HIP_OK(c, sl.d_items.reserve(n_shapes * 2 * (size_t)((H + kBandRows - 1) / kBandRows) * ((W + kChunkW - 1) / kChunkW) + 1));
  OFDG_TRY(reserve_blockmask(c, sl, n_samples));
  if (n_objects && c->prm.background_prep) {
    HIP_OK(c, sl.d_bgprep.reserve(n_samples));
    HIP_OK(c, sl.d_bgtex.reserve((size_t)n_samples * 4 * W * H));
  }
  return ensure_item_count(c, sl);
}

// ---- render -------------------------------------------------------------------------------
// device counter sampler + device realize fill the slot's records (no host data)
static int prepare_backgrounds(ofdg_ctx* c, ofdg_ctx::Slot& sl, int n, bool records_resident, hipStream_t s, uint32_t* err, hipEvent_t stop = nullptr,
                               int base = 0, hipEvent_t start = nullptr);
//   the slot is sized for res_samples / part batches: samples [k part, (k + 1) part) are first_index + k x part_stride .. and flag in err[k]
static int launch_counter_sampler(ofdg_ctx* c, ofdg_ctx::Slot& sl, long long first_index, hipStream_t s, uint32_t* const err[kMaxFrontBatches],
                                  int part, long long part_stride) {
  const int stride = sl.res_shapes / sl.res_samples;
  const int prep = c->prm.background_prep ? 1 : 0;
  CsRealizeDims D{c->prm.width, c->prm.height, c->pool_n, c->pool_w, c->pool_h, sl.res_samples, stride, prep,
                  c->prm.mode == 9 ? c->crop_server.n_crops : 0, c->fg_src.stride, c->fg_src.origin, c->bg_src.stride, c->bg_src.origin,
                  (unsigned long long)(uintptr_t)c->pool.p, c->d_tex_table.p, c->prm.mode == 9 ? c->d_cs_croptab.p : nullptr};
  hipLaunchKernelGGL(cs_sample_realize_kernel, dim3(sl.res_samples * kCsGroups), dim3(64), 0, s, c->cs_mode, D, first_index,
                     sl.d_shapes.p, sl.d_objects.p, sl.d_samples.p, err[0], sl.d_bgprep.p, part, part_stride, err[1], err[2], err[3]);
  HIP_OK(c, hipGetLastError());
  sl.bgprep_pending = prep != 0;  // (rendered behind raster: launch_prepare)
  return OFDG_OK;
}

// OFDG_STREAM_OWN as a call's `stream`: the internal stream that call works on (what ofdg_stream() returns right before it)
static void* own_stream(ofdg_ctx* c, void* stream) { return stream == OFDG_STREAM_OWN ? ofdg_stream(c) : stream; }

static ofdg_ctx::Chain& take_chain(ofdg_ctx* c) {
  const int k = (int)(c->next_chain % (unsigned)c->n_chains);
  c->next_chain++;
  c->last_chain = k;
  return c->chains[k];
}
// the stream chain `ch` works on for a call made with the caller's stream `st`
static hipStream_t chain_stream(const ofdg_ctx* c, const ofdg_ctx::Chain& ch, hipStream_t st) { return c->overlap ? ch.stream.s : st; }

// A prepared batch that will never be composed (the caller's sequence jumped, the pool changed, the chain's private slot is
// needed for something else): forget it.  compose is what resets the slot's raster work list, so do that here.
// what the kernels of a batch that is never handed over flagged is nobody's (its word must not speak for ticket + kErrWords,
// nor make ofdg_synchronize report a batch that was never composed)
static int clean_discarded_word(ofdg_ctx* c, const ofdg_ctx::Chain::Prepared& p) {
  if (p.ticket >= 0 && p.ticket + ofdg_ctx::kErrWords > c->ticket) {
    HIP_OK(c, hipMemsetAsync(err_word(c, p.ticket), 0, sizeof(uint32_t), p.stream));
    c->word_clean[(size_t)(p.ticket % ofdg_ctx::kErrWords)] = true;
  }
  return OFDG_OK;
}
// The remaining parts of a group that their calls will not come for.  Their raster items are consumed and the work list was
// reset by part 0's compose (or is, by discard_prepared, if that compose never ran either): only their words are left.
static int discard_rest(ofdg_ctx* c, ofdg_ctx::Chain& ch) {
  for (ofdg_ctx::Chain::Prepared& p : ch.rest) {
    if (!p.valid) continue;
    p.valid = false;
    ch.fresh = true;
    OFDG_TRY(clean_discarded_word(c, p));
  }
  return OFDG_OK;
}
static int discard_prepared(ofdg_ctx* c, ofdg_ctx::Chain& ch) {
  OFDG_TRY(discard_rest(c, ch));
  if (!ch.prep.valid) return OFDG_OK;
  ch.prep.valid = false;
  ch.fresh = true;
  if (ch.prep.slot && ch.prep.slot->d_item_count.p) HIP_OK(c, hipMemsetAsync(ch.prep.slot->d_item_count.p, 0, sizeof(int), ch.prep.stream));
  return clean_discarded_word(c, ch.prep);
}
static int discard_all_prepared(ofdg_ctx* c) {
  c->bg_cap_n = -1;  // (called by everything that changes the pool)
  for (int k = 0; k < c->n_chains; ++k) OFDG_TRY(discard_prepared(c, c->chains[k]));
  return OFDG_OK;
}

static RenderDims render_dims(const ofdg_ctx* c, const ofdg_ctx::Slot& sl) {
  const int W = c->prm.width, H = c->prm.height;
  RenderDims dm;
  dm.W = W; dm.H = H; dm.pool_w = c->pool_w; dm.pool_h = c->pool_h;
  dm.use_aa = c->prm.use_antialiasing ? 1 : 0;
  dm.n_samples = sl.res_samples;
  dm.n_shapes = sl.res_shapes;
  dm.tiles_x = (W + kTileW - 1) / kTileW;
  dm.tiles_y = (H + kTileH - 1) / kTileH;
  dm.bg_pitch = c->prm.background_prep ? 2 * W : c->bg_src.pitch;
  dm.fg_pitch = c->fg_src.pitch;
  return dm;
}

// Work about to be enqueued on `s` must follow what `ev` marks on another stream.  An event that has already fired costs a
// query and clears `*pending`; otherwise `s` waits for it, and `*pending` stays set for the other streams that may still
// have to wait - unless `settles`: the waiting stream is the only one that ever asks.
static int wait_unless_fired(ofdg_ctx* c, hipStream_t s, hipEvent_t ev, bool* pending, bool settles = false) {
  if (hipEventQuery(ev) == hipSuccess) { *pending = false; return OFDG_OK; }
  HIP_OK(c, hipStreamWaitEvent(s, ev, 0));
  if (settles) *pending = false;
  return OFDG_OK;
}
// Kernels that read slot `sl` and the workspaces of chain `ch` were enqueued on `s`, the last one with `done` (the chain's
// ev_done) on its packet: whoever rewrites either from another stream waits for it (launch_prepare, upload_slot).
static void track_completion(ofdg_ctx::Slot& sl, ofdg_ctx::Chain& ch, hipStream_t s, hipEvent_t done) {
  sl.compose_pending = true; sl.compose_stream = s; sl.compose_event = done;
  ch.done_pending = true; ch.done_stream = s;
}

// The preparation kernels of the batch resident in `sl`, in order on chain `ch`: [counter sampler ->] geom -> raster
//   `st` is the stream of the call the batch is prepared for (only the serial mode prepares on it).
//   view_n > 0: the batch is samples [view_base, view_base + view_n) of the slot (ofdg_render_resident of a slot that was filled
//   for several batches).  group > 1 (the shared front end, counter sampler): the slot is sized for group x n_first samples, part k
//   holding the batch of first index cs_first_index + k x part_stride; the three launches serve them all, the preparation behind
//   them part 0 only, and parts 1 .. group - 1 are left in ch.rest.
static int launch_prepare(ofdg_ctx* c, ofdg_ctx::Chain& ch, ofdg_ctx::Slot& sl, hipStream_t st, long long cs_first_index = -1,
                          bool hand_over = true, int view_base = 0, int view_n = 0, int group = 1, long long part_stride = 0, int n_first = 0) {
  const int W = c->prm.width, H = c->prm.height;
  const int n_sf = sl.res_shapes * 2;
  const RenderDims dm = render_dims(c, sl);
  const bool grouped = cs_first_index >= 0 && group > 1;
  if (!grouped) group = 1;
  OFDG_TRY(discard_prepared(c, ch));
  // (this launch rewrites the slot's outlines and flips its block masks: the parts another chain keeps in it are gone)
  if (&sl != &ch.slot)
    for (int k = 0; k < c->n_chains; ++k)
      if (c->chains[k].next_part() && c->chains[k].next_part()->slot == &sl) OFDG_TRY(discard_rest(c, c->chains[k]));
  // this batch's number: its kernels raise their flags in its own word ... and the later parts': every kernel of the front end
  // knows its sample (words past the group are part 0's: no sample selects them)
  const long long ticket = c->ticket;
  c->ticket += group;
  uint32_t* errs[kMaxFrontBatches];
  for (int k = 0; k < kMaxFrontBatches; ++k) errs[k] = err_word(c, ticket + (k < group ? k : 0));
  uint32_t* const err = errs[0];
  Event* ev = nullptr;
  if (c->profiling && c->ev_sets > 0 && (c->launch_count % c->ev_stride) == 0) {
    const size_t set = (size_t)(c->ev_alloc++ % c->ev_sets);
    ev = &c->ev[set * 6];
    c->ev_composed[set] = 0;
    c->ev_bgprep[set] = 0;
    c->ev_front[set] = 1;
  }
  c->launch_count++;
  if (!c->overlap) {
    // everything runs on the caller's stream; a caller that switches streams loses the ordering
    if (c->have_last_user_st && c->last_user_st != st) HIP_OK(c, hipDeviceSynchronize());
    c->last_user_st = st; c->have_last_user_st = true;
  }
  hipStream_t S = chain_stream(c, ch, st);
  uint8_t* cov = ch.cov.p;
  // the slot's records: written on another stream, or still read by a compose of another chain
  // (a user slot rendered again; the chain's private slot only ever sees its own stream)
  if (sl.upload_pending && sl.upload_stream != S) OFDG_TRY(wait_unless_fired(c, S, sl.ev_uploaded, &sl.upload_pending));
  // the chain's workspace (and private slot) may still be read by its previous compose if that ran on a caller's stream
  // (the chain's stream is ordered behind it from here on: settled either way)
  if (ch.done_pending && ch.done_stream != S) OFDG_TRY(wait_unless_fired(c, S, ch.ev_done, &ch.done_pending, /*settles=*/true));
  if (sl.compose_pending && sl.compose_stream != S) OFDG_TRY(wait_unless_fired(c, S, sl.compose_event, &sl.compose_pending));
  // mode 9: the batch's own crop table (host path) or the static table of all crops (counter sampler)
  const DevCropRef* croptab = cs_first_index >= 0 ? c->d_cs_croptab.p : sl.d_croptab.p;
  HIP_OK(c, take_err_word(c, ticket, S));  // (nothing is enqueued unless this caller asks by ticket AND the word's last owner was never asked about)
  for (int k = 1; k < group; ++k) HIP_OK(c, take_err_word(c, ticket + k, S));
  if (cs_first_index >= 0) {  // device counter sampler + device realize
    OFDG_TRY(launch_counter_sampler(c, sl, cs_first_index, S, errs, grouped ? n_first : sl.res_samples, grouped ? part_stride : 0));
  }
  // (the background preparation of the batch goes LAST, right in front of compose: below)
  // geom: outlines, bounding boxes, per-object boxes (parity `bp`), raster work list
  const int bp = sl.box_parity;
  sl.box_parity ^= 1;
  unsigned long long* box_cur = sl.d_blockmask.p + (size_t)bp * sl.box_stride;
  unsigned long long* box_next = sl.d_blockmask.p + (size_t)(bp ^ 1) * sl.box_stride;
  sl.mask_used[bp] = sl.res_samples * dm.tiles_x * ((H + kBandRows - 1) / kBandRows) * 2;
  const int n_mask_words = sl.mask_used[bp ^ 1];
  const bool prof_prep = ev && c->profiling == 2;
  // Profiled launches: a kernel's time is the span between the completion of its predecessor on the
  // chain's stream and its own completion - both taken from the kernels' own dispatch packets (stop
  // events).  A start event is a marker packet in front of the kernel, which delays its dispatch by
  // ~6-10 us: geom (first of the three) and compose (ev[4], launch_compose) have one, raster has none.
  // geom: outlines, boxes, raster work list -> raster: coverage slots + block masks (persistent waves over the list)
  hipExtLaunchKernelGGL(geom_kernel, dim3(std::max(1, (n_sf + kGeomWaves - 1) / kGeomWaves)), dim3(64 * kGeomWaves), 0, S,
                        prof_prep ? ev[0].e : nullptr, prof_prep ? ev[1].e : nullptr, 0, sl.d_shapes.p, sl.res_shapes, c->d_cs_tab.p, W, H,
                        sl.d_frames.p, sl.d_verts.p, box_cur, err, sl.d_item_count.p, sl.d_items.p, croptab,
                        grouped ? n_first * (sl.res_shapes / sl.res_samples) * 2 : std::max(n_sf, 1), errs[1], errs[2], errs[3]);
  HIP_OK(c, hipGetLastError());
  // The batch's last preparation kernel - raster, or the background preparation behind it - carries two things on its own
  // packet: the hand-over event of a compose on a caller's stream, or (profiling 1) the start of the compose launch's time.
  // The ALU-bound background preparation runs LAST, right in front of compose: sampler -> geom -> raster -> preparation ->
  // compose is 4 % faster in the steady state than with the preparation behind the sampler (the latency-bound kernels of a
  // chain follow each other, the two heavy ones too; profiles/r04_experiments_log.md section 11).
  const bool prep_last = sl.bgprep_pending;
  hipEvent_t last_stop = ev ? (c->profiling == 2 ? nullptr : ev[4].e) : (hand_over ? ch.ev_prep.e : nullptr);
  // (a profiled batch with a preparation behind raster also takes raster's completion: the preparation is timed from there)
  hipExtLaunchKernelGGL(raster_kernel, dim3(kRasterGridFront[group] * 4 / kRasterWaves), dim3(64 * kRasterWaves), 0, S, nullptr,
                        (ev && (c->profiling == 2 || prep_last)) ? ev[3].e : (prep_last ? nullptr : last_stop), 0,
                        sl.d_frames.p, sl.d_items.p, sl.d_item_count.p, sl.d_verts.p, W, H, cov, box_next, n_mask_words, box_cur);
  HIP_OK(c, hipGetLastError());
  if (prep_last) {
    // (of a group: part 0's only - a later part's goes in front of ITS compose, launch_next_part)
    OFDG_TRY(prepare_backgrounds(c, sl, grouped ? n_first : sl.res_samples, /*records_resident=*/true, S, err, (ev && c->profiling == 2) ? ev[2].e : last_stop));
    sl.bgprep_pending = false;
    if (ev) c->ev_bgprep[(size_t)(ev - c->ev.data()) / 6] = 1;
  }
  if (ev && hand_over) HIP_OK(c, hipEventRecord(ch.ev_prep, S));
  ch.prep.valid = true; ch.prep.slot = &sl; ch.prep.first_index = cs_first_index;
  ch.prep.n = grouped ? n_first : (view_n > 0 ? view_n : sl.res_samples);
  ch.prep.base = view_n > 0 ? view_base : 0;
  ch.prep.box_cur = box_cur; ch.prep.croptab = croptab; ch.prep.ev = ev; ch.prep.stream = S; ch.prep.ticket = ticket;
  ch.prep.ahead = false;
  ch.rest_next = 0;
  for (int k = 1; k < group; ++k) {
    ofdg_ctx::Chain::Prepared& p = ch.rest[k - 1];
    p = ch.prep;
    p.first_index = cs_first_index + k * part_stride; p.base = k * n_first; p.ev = nullptr; p.ticket = ticket + k;
  }
  ch.fresh = false;
  return OFDG_OK;
}

// The call the next part of a group was made for has come: samples [k n, (k + 1) n) of the chain's private slot are
// sampled, outlined and rasterised.  What is left is the batch's own background preparation, on the chain's stream, and the
// hand-over of a compose on a caller's stream - recorded behind THAT preparation.  No geom / raster launch: a profiled call's
// event set says so (ev_front), and profiling 1 has a predecessor of compose on the chain only where there is a preparation.
static int launch_next_part(ofdg_ctx* c, ofdg_ctx::Chain& ch, bool hand_over) {
  ofdg_ctx::Chain::Prepared h = *ch.next_part();
  ofdg_ctx::Slot& sl = *h.slot;
  const hipStream_t S = h.stream;
  const bool prep = c->prm.background_prep != 0;
  Event* ev = nullptr;
  if (c->profiling && c->ev_sets > 0 && (c->launch_count % c->ev_stride) == 0 && (c->profiling == 2 || prep)) {
    const size_t set = (size_t)(c->ev_alloc++ % c->ev_sets);
    ev = &c->ev[set * 6];
    c->ev_composed[set] = 0;
    c->ev_bgprep[set] = 0;
    c->ev_front[set] = 0;
  }
  c->launch_count++;
  // the previous part's compose may have run on a caller's stream: the chain's stream is ordered behind it from here on, as in
  // launch_prepare (the event is about to be taken by this batch's compose)
  if (ch.done_pending && ch.done_stream != S) OFDG_TRY(wait_unless_fired(c, S, ch.ev_done, &ch.done_pending, /*settles=*/true));
  if (sl.compose_pending && sl.compose_stream != S) OFDG_TRY(wait_unless_fired(c, S, sl.compose_event, &sl.compose_pending));
  ch.rest[ch.rest_next++].valid = false;  // (taken: a failure below leaves it to discard_prepared as `prep`)
  h.ev = ev;
  ch.prep = h;
  if (prep) {
    const bool prof2 = ev && c->profiling == 2;
    const hipEvent_t stop = ev ? (prof2 ? ev[2].e : ev[4].e) : (hand_over ? ch.ev_prep.e : nullptr);
    OFDG_TRY(prepare_backgrounds(c, sl, h.n, /*records_resident=*/true, S, err_word(c, h.ticket), stop, h.base, prof2 ? ev[3].e : nullptr));
    if (prof2) c->ev_bgprep[(size_t)(ev - c->ev.data()) / 6] = 1;  // (its own start marker .. its end)
  }
  if (hand_over && (ev || !prep)) HIP_OK(c, hipEventRecord(ch.ev_prep, S));
  return OFDG_OK;
}

// ---- what one render / forward call writes -----------------------------------------------------------
// The twelve entry points (ofdg_render, ofdg_forward, ofdg_forward_counter; plain, _ex, _fmt, _ex_fmt) differ in how the
// caller says it; from check_call on a call is this.
struct CallOut {
  const char* fn;           // the entry point, for messages
  void *img0, *img1, *flow; // element types as out_fmt says
  ofdg_extras_fmt ex;       // the optional outputs (an ofdg_extras is this with float32 occlusion maps); no pointer set: none
  int out_fmt;              // the compose kernels' bits, kOutImageU8 | kOutFlowF16 (0: float32 throughout)
};
static int invalid_argument(ofdg_ctx* c, const char* fn) {
  if (c) c->err = std::string(fn) + ": invalid argument";
  return OFDG_EINVAL;
}
static bool extras_requested(const ofdg_extras_fmt* ex) { return ex && (ex->flow1 || ex->occ0 || ex->occ1 || ex->label0 || ex->label1); }
static ofdg_extras_fmt widen_extras(const ofdg_extras* ex) {
  ofdg_extras_fmt x{};
  if (ex) { x.flow1 = ex->flow1; x.occ0 = ex->occ0; x.occ1 = ex->occ1; x.label0 = ex->label0; x.label1 = ex->label1; }
  x.occ = OFDG_FMT_F32;
  return x;
}
// The optional outputs are defined for the rigid modes.
static int check_extras(ofdg_ctx* c, const ofdg_extras_fmt* ex, const char* fn) {
  if (extras_requested(ex) && c->prm.mode == 9) {
    c->err = std::string(fn) + ": backward flow, labels and occlusion are defined for the rigid modes only (mode 9: the reference's "
             "inverse branch adds the forward warp field, DG:403-406, 715-716)";
    return OFDG_EINVAL;
  }
  return OFDG_OK;
}
// ofdg_extras_fmt: its own fields first (whether or not a pointer is set), then what ofdg_extras is checked for.
static int check_extras_fmt(ofdg_ctx* c, const ofdg_extras_fmt* ex, const char* fn) {
  if (!ex) return OFDG_OK;
  auto fail = [&](const std::string& field, int value, const char* valid) {
    c->err = std::string(fn) + ": ofdg_extras_fmt." + field + " = " + std::to_string(value) + " (valid: " + valid + ")";
    return OFDG_EINVAL;
  };
  if (ex->occ != OFDG_FMT_F32 && ex->occ != OFDG_FMT_U8) return fail("occ", ex->occ, "OFDG_FMT_F32, OFDG_FMT_U8");
  for (int k = 0; k < 3; ++k)
    if (ex->reserved[k] != 0) return fail("reserved[" + std::to_string(k) + "]", ex->reserved[k], "0");
  return check_extras(c, ex, fn);
}
// ofdg_out_format -> the compose kernels' out_fmt bits (0: the plain call)
static int check_out_format(ofdg_ctx* c, const ofdg_out_format* fmt, const char* fn, int* out_fmt) {
  *out_fmt = 0;
  if (!fmt) return OFDG_OK;
  auto fail = [&](const char* field, int value, const char* valid) {
    c->err = std::string(fn) + ": ofdg_out_format." + field + " = " + std::to_string(value) + " (valid: " + valid + ")";
    return OFDG_EINVAL;
  };
  if (fmt->image != OFDG_FMT_F32 && fmt->image != OFDG_FMT_U8) return fail("image", fmt->image, "OFDG_FMT_F32, OFDG_FMT_U8");
  if (fmt->flow != OFDG_FMT_F32 && fmt->flow != OFDG_FMT_F16) return fail("flow", fmt->flow, "OFDG_FMT_F32, OFDG_FMT_F16");
  for (int k = 0; k < 2; ++k)
    if (fmt->reserved[k] != 0) return fail(k ? "reserved[1]" : "reserved[0]", fmt->reserved[k], "0");
  *out_fmt = (fmt->image == OFDG_FMT_U8 ? kOutImageU8 : 0) | (fmt->flow == OFDG_FMT_F16 ? kOutFlowF16 : 0);
  return OFDG_OK;
}
// What entry point `fn` received, as a CallOut, before anything is enqueued: its own argument test (`args_ok`; it speaks as
// `args_fn` where that is given), then the format, then the extras (at most one of ex / exf is given; any of the three may be NULL).
static int check_call(ofdg_ctx* c, const char* fn, bool args_ok, void* img0, void* img1, void* flow, const ofdg_extras* ex,
                      const ofdg_extras_fmt* exf, const ofdg_out_format* fmt, CallOut* o, const char* args_fn = nullptr) {
  if (!args_ok) return invalid_argument(c, args_fn ? args_fn : fn);
  *o = CallOut{fn, img0, img1, flow, exf ? *exf : widen_extras(ex), 0};
  OFDG_TRY(check_out_format(c, fmt, fn, &o->out_fmt));
  return exf ? check_extras_fmt(c, exf, fn) : check_extras(c, &o->ex, fn);
}

// ---- compose ------------------------------------------------------------------------------------------
// The optional outputs of one compose launch (rigid modes) as the kernels take them.
struct ComposeExtras {
  bool any = false;   // the _ext kernels
  bool occ = false;   // ... with an occlusion pass behind compose
  bool fmt = false;   // in a compact format of the outputs or of their own (uint8 maps): compose_rigid_ext_fmt + occlusion_fmt
  ExtOut xo{nullptr, nullptr, nullptr};       // where compose writes the backward flow and the labels
  uint32_t *tgt0 = nullptr, *tgt1 = nullptr;  // ... and, `fmt`, its rounded targets for the occlusion pass
};
// Where compose writes the backward flow and the labels: the caller's buffers, or the chain's workspace when only the
// occlusion pass needs them (grown only; growing waits for the device, like reserve_workspaces).
static int plan_extras(ofdg_ctx* c, ofdg_ctx::Chain& ch, int n_samples, const CallOut& o, ComposeExtras* x) {
  const ofdg_extras_fmt& ex = o.ex;
  if (!extras_requested(&ex)) return OFDG_OK;
  x->any = true;
  x->occ = ex.occ0 || ex.occ1;
  x->fmt = o.out_fmt || ex.occ == OFDG_FMT_U8;
  const size_t plane = (size_t)c->prm.width * c->prm.height, n = (size_t)n_samples;
  // (with a compact format the occlusion pass reads compose's rounded targets, not flow / flow1: no flow1 workspace)
  const bool ws_labels = x->occ && (!ex.label0 || !ex.label1), ws_flow1 = !x->fmt && ex.occ1 && !ex.flow1, ws_tgt = x->fmt && x->occ;
  if ((ws_labels && 2 * n * plane > ch.x_labels.cap) || (ws_flow1 && 2 * n * plane > ch.x_flow1.cap) ||
      (ws_tgt && 2 * n * plane > ch.x_targets.cap)) {
    HIP_OK(c, hipDeviceSynchronize());
    if (ws_labels) HIP_OK(c, ch.x_labels.reserve(2 * n * plane));
    if (ws_flow1) HIP_OK(c, ch.x_flow1.reserve(2 * n * plane));
    if (ws_tgt) HIP_OK(c, ch.x_targets.reserve(2 * n * plane));
  }
  if (ws_tgt) {  // stored only for the frames whose map is asked for
    x->tgt0 = ex.occ0 ? ch.x_targets.p : nullptr;
    x->tgt1 = ex.occ1 ? ch.x_targets.p + n * plane : nullptr;
  }
  x->xo.flow1 = ex.flow1 ? static_cast<float*>(ex.flow1) : (ws_flow1 ? ch.x_flow1.p : nullptr);
  x->xo.label0 = ex.label0 ? ex.label0 : (x->occ ? ch.x_labels.p : nullptr);
  x->xo.label1 = ex.label1 ? ex.label1 : (x->occ ? ch.x_labels.p + n * plane : nullptr);
  return OFDG_OK;
}

// Where compose runs: on the chain's stream, right behind the preparation - or, if the caller passed another stream,
// on THAT stream (in order with the caller's own work, which may still read the outputs) once the batch is prepared.
static int compose_stream(ofdg_ctx* c, ofdg_ctx::Chain& ch, hipStream_t st, hipStream_t* cs) {
  *cs = ch.prep.stream;
  if (*cs == st) return OFDG_OK;
  HIP_OK(c, hipStreamWaitEvent(st, ch.ev_prep, 0));
  *cs = st;
  return OFDG_OK;
}

// The compose kernel of the prepared batch on `cs`, and the occlusion pass behind it.  `done` (or null) goes on the packet of
// the last kernel.
//   Profiled launches (ev): start and stop are the timestamps of the compose kernel's own dispatch packet.  profiling 1
//   (compose only, what bench.py runs the timed region with): NO start marker - the compose launch is timed from the
//   completion of its predecessor on the chain (the last preparation kernel's own packet, ev[4], launch_prepare) to its own
//   completion: its dispatch gap (1 - 2 us) is counted with it, and nothing is added to the stream.  profiling 2: the
//   kernel's own start (a marker, ev[4]) and end.
//   The batch is samples [ch.prep.base, + ch.prep.n) of the slot: the sample records and the block-mask rows are passed from
//   there on (a kernel's sample 0 is the batch's first); shapes, objects, coverage slots and the prepared textures are
//   addressed by what the records hold, which is slot-global.
static int launch_compose_kernels(ofdg_ctx* c, const ofdg_ctx::Chain& ch, const ofdg_ctx::Slot& sl, const CallOut& o, const ComposeExtras& x,
                                  const uint32_t* fgpool, const uint32_t* bgpool, hipStream_t cs, hipEvent_t done) {
  const int W = c->prm.width, H = c->prm.height;
  RenderDims dm = render_dims(c, sl);
  dm.n_samples = ch.prep.n;
  const DevSample* const samples = sl.d_samples.p + ch.prep.base;
  const unsigned long long* const box = ch.prep.box_cur + (size_t)ch.prep.base * dm.tiles_x * ((H + kBandRows - 1) / kBandRows) * 2;
  const int grid = dm.tiles_x * dm.tiles_y * dm.n_samples * 4;  // one 64 x 4 strip per single-wave workgroup
  Event* const ev = ch.prep.ev;
  // the variant, decided here once (the optional outputs exist in the rigid modes only: check_extras)
  enum class Kind { kRigid, kRigidExt, kRigidFmt, kRigidExtFmt, kDeform, kDeformFmt };
  const Kind kind = c->prm.mode == 9 ? (o.out_fmt ? Kind::kDeformFmt : Kind::kDeform)
                                     : x.fmt ? Kind::kRigidExtFmt : x.any ? Kind::kRigidExt : o.out_fmt ? Kind::kRigidFmt : Kind::kRigid;
  const bool pow2 = (W & (W - 1)) == 0;
  const Launch lc{(unsigned)grid, 64, cs, (ev && c->profiling == 2) ? ev[4].e : nullptr, ev ? ev[5].e : (x.occ ? nullptr : done)};
  // every family has a _pow2 and a general kernel of one function type: this is the one place a compose kernel is launched
  auto compose = [&](auto* k_pow2, auto* k, auto... args) { launch_kernel(lc, pow2 ? k_pow2 : k, args...); };
  auto rigid = [&](auto* k_pow2, auto* k, auto... tail) {
    compose(k_pow2, k, samples, box, sl.d_objects.p, ch.cov.p, grid, dm.tiles_x, dm.tiles_y, W, H, dm.use_aa, dm.bg_pitch,
            dm.fg_pitch, fgpool, bgpool, o.img0, o.img1, o.flow, sl.d_frames.p, sl.d_item_count.p, tail...);
  };
  auto deform = [&](auto* k_pow2, auto* k, auto... tail) {
    compose(k_pow2, k, dm, samples, sl.d_objects.p, box, ch.cov.p, fgpool, bgpool, o.img0, o.img1, o.flow, sl.d_frames.p,
            ch.prep.croptab, sl.d_item_count.p, tail...);
  };
  switch (kind) {
    case Kind::kRigid: rigid(compose_rigid_pow2_kernel, compose_rigid_kernel); break;
    case Kind::kRigidExt: rigid(compose_rigid_ext_pow2_kernel, compose_rigid_ext_kernel, x.xo); break;
    case Kind::kRigidFmt: rigid(compose_rigid_fmt_pow2_kernel, compose_rigid_fmt_kernel, o.out_fmt); break;
    case Kind::kRigidExtFmt: rigid(compose_rigid_ext_fmt_pow2_kernel, compose_rigid_ext_fmt_kernel, x.xo, o.out_fmt, x.tgt0, x.tgt1); break;
    case Kind::kDeform: deform(compose_deform_pow2_kernel, compose_deform_kernel); break;
    case Kind::kDeformFmt: deform(compose_deform_fmt_pow2_kernel, compose_deform_fmt_kernel, o.out_fmt); break;
  }
  HIP_OK(c, hipGetLastError());
  if (x.occ) {  // behind compose on the same stream; the chain's completion event (workspace, slot) goes on THIS packet
    const long long quads = (long long)dm.n_samples * H * (W / 4);
    const Launch lo{(unsigned)((quads + 255) / 256), 256, cs, nullptr, ev ? nullptr : done};
    if (x.fmt)
      launch_kernel(lo, occlusion_fmt_kernel, x.tgt0, x.tgt1, x.xo.label0, x.xo.label1, o.ex.occ0, o.ex.occ1, W, H, dm.n_samples,
                    o.ex.occ == OFDG_FMT_U8 ? kOutOccU8 : 0);
    else
      launch_kernel(lo, occlusion_kernel, o.flow, x.xo.flow1, x.xo.label0, x.xo.label1, o.ex.occ0, o.ex.occ1, W, H, dm.n_samples);
    HIP_OK(c, hipGetLastError());
  }
  return OFDG_OK;
}

// What a compose launch leaves behind on the host: the profiled launch's event set, and who has to wait for it.
static int note_compose(ofdg_ctx* c, ofdg_ctx::Chain& ch, ofdg_ctx::Slot& sl, hipStream_t cs, bool foreign, hipEvent_t done) {
  if (Event* const ev = ch.prep.ev) {
    if (done) HIP_OK(c, hipEventRecord(done, cs));
    // profiling 1 times compose from the completion of the chain's last preparation kernel: that is the launch's time only
    // when compose is enqueued right behind it on the same stream.  A batch prepared ahead by an earlier call, or composed
    // on a caller's stream behind the hand-over event, would count host and queue idle time: such a set is not a sample.
    const bool span_is_the_launch = c->profiling == 2 || (!foreign && !ch.prep.ahead);
    if (span_is_the_launch) {
      c->ev_count++;
      c->ev_composed[(size_t)(ev - c->ev.data()) / 6] = 1;
    }
  }
  if (done) track_completion(sl, ch, cs, done);
  else sl.compose_pending = false;  // private slot on its own chain: stream order is all it needs
  return OFDG_OK;
}

// compose of the batch chain `ch` has prepared, into what `o` (checked) describes.  `st` is the caller's stream: if it is
// not the chain's own stream (ofdg_stream), compose runs on `st` instead, behind what the caller enqueued there (the outputs
// may still be read) and behind the chain's preparation kernels.
static int launch_compose(ofdg_ctx* c, ofdg_ctx::Chain& ch, const CallOut& o, hipStream_t st) {
  if (!ch.prep.valid) { c->err = "internal: compose without a prepared batch"; return OFDG_EINVAL; }
  ofdg_ctx::Slot& sl = *ch.prep.slot;
  ComposeExtras x;
  OFDG_TRY(plan_extras(c, ch, ch.prep.n, o, &x));
  const uint32_t* bgpool = c->prm.background_prep ? sl.d_bgtex.p : (c->pool_bg.p ? c->pool_bg.p : c->pool.p);  // (after the slot's buffers are final)
  const uint32_t* fgpool = c->pool_fg.p ? c->pool_fg.p : c->pool.p;
  if (c->prm.background_prep && !bgpool) { c->err = "background_prep: the slot has no prepared backgrounds"; return OFDG_EINVAL; }
  c->last_slot = &sl; c->last_ch = &ch;
  c->last_base = ch.prep.base; c->last_n = ch.prep.n;
  c->last_stream = ch.prep.stream; c->last_ticket = ch.prep.ticket;
  ch.prep.valid = false;  // (consumed from here on; an argument error above leaves it to discard_prepared, which resets the work list)
  const bool foreign = ch.prep.stream != st;  // the caller's stream is not the chain's
  hipStream_t cs;
  OFDG_TRY(compose_stream(c, ch, st, &cs));
  // It is tracked by the chain's event whenever somebody else may have to wait for it: the chain itself (workspace, private
  // slot) after a compose on a caller's stream, other chains for a shared slot.
  const bool shared_slot = &sl != &ch.slot;
  const hipEvent_t done = (foreign || shared_slot) ? ch.ev_done.e : nullptr;
  OFDG_TRY(launch_compose_kernels(c, ch, sl, o, x, fgpool, bgpool, cs, done));
  return note_compose(c, ch, sl, cs, foreign, done);
}

// preparation + compose of the batch resident in `sl`, in order on chain `ch`
//   view_n > 0: of its samples [view_base, view_base + view_n) only
static int launch_resident(ofdg_ctx* c, ofdg_ctx::Chain& ch, ofdg_ctx::Slot& sl, const CallOut& o, hipStream_t st, long long cs_first_index = -1,
                           int view_base = 0, int view_n = 0) {
  // (the preparation's completion event is only needed when compose runs on another stream than the chain's)
  OFDG_TRY(launch_prepare(c, ch, sl, st, cs_first_index, chain_stream(c, ch, st) != st, view_base, view_n));
  return launch_compose(c, ch, o, st);
}

// CImg get_resize(.., 3), enlarging branch: source index and weight of every destination pixel (cimg_enlarge_table) for
// EVERY source length n < s, entry [n * s + x]; once per context and frame size
constexpr int kPrepGrid = 4096;  // single-wave workgroups of bgprep_stream_kernel: four per SIMD (2048 / 3072 / 8192: -6 % / -2 % / -1 %, profiles/r05_experiments_log.md section 2)
static int ensure_bgprep_tables(ofdg_ctx* c) {
  const int TW = 2 * c->prm.width, TH = 2 * c->prm.height;
  if (c->bg_tab_w == TW && c->bg_tab_h == TH) return OFDG_OK;
  auto build = [&](int s, DevBuf<uint16_t>& d_at, DevBuf<double>& d_alpha) -> int {
    std::vector<uint16_t> at((size_t)s * s, 0);
    std::vector<double> alpha((size_t)s * s, 0.0);
    for (int n = 1; n < s; ++n) cimg_enlarge_table(n, s, &at[(size_t)n * s], &alpha[(size_t)n * s]);
    HIP_OK(c, d_at.reserve(at.size()));
    HIP_OK(c, d_alpha.reserve(alpha.size()));
    HIP_OK(c, hipMemcpy(d_at.p, at.data(), at.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_OK(c, hipMemcpy(d_alpha.p, alpha.data(), alpha.size() * sizeof(double), hipMemcpyHostToDevice));
    return OFDG_OK;
  };
  if (TW > 65535 || TH > 65535) { c->err = "background_prep: frame too large for the resize tables"; return OFDG_EINVAL; }
  HIP_OK(c, hipDeviceSynchronize());
  int rc = build(TW, c->d_bg_at_x, c->d_bg_alpha_x);
  if (rc == OFDG_OK) rc = build(TH, c->d_bg_at_y, c->d_bg_alpha_y);
  if (rc != OFDG_OK) return rc;
  c->bg_tab_w = TW; c->bg_tab_h = TH;
  return OFDG_OK;
}

// background_prep: render the 2W x 2H background textures of n samples into the slot's buffer on stream `s`; their
// records are in sl.d_bgprep already (written by the device sampler, or uploaded with the batch's other records)
//   stop: an event for the completion of the LAST kernel launched here (on that kernel's own packet); start: a marker in front
//   of the first one (profiling 2 of a batch that has no raster launch to be timed from)
//   base: the slot's first sample of the n (the second batch of a slot filled for two: its records and textures start there)
static int prepare_backgrounds(ofdg_ctx* c, ofdg_ctx::Slot& sl, int n, bool records_resident, hipStream_t s, uint32_t* err, hipEvent_t stop, int base,
                               hipEvent_t start) {
  const int W = c->prm.width, H = c->prm.height;
  if (!records_resident || !sl.d_bgprep.p || sl.d_bgprep.cap < (size_t)(base + n)) { c->err = "internal: background preparation without its records"; return OFDG_EINVAL; }
  if (base == 0) HIP_OK(c, sl.d_bgtex.reserve((size_t)n * 4 * W * H));
  else if (sl.d_bgtex.cap < (size_t)(base + n) * 4 * W * H) { c->err = "internal: background preparation of a second batch the slot was not sized for"; return OFDG_EINVAL; }
  const DevBgPrep* const rec = sl.d_bgprep.p + base;
  uint32_t* const tex = sl.d_bgtex.p + (size_t)base * 4 * W * H;
  int cap_cw, cap_ch;
  bool fusable;
  bgprep_caps(c, &cap_cw, &cap_ch, &fusable);
  const bool staged = c->prm.background_prep == 1;
  constexpr int kBgPrepBlocks = 192;  // x 256 threads per sample, grid-stride over the (device-known) region
  if (staged) {
    OFDG_TRY(ensure_bgprep_tables(c));
  }
  if (!staged) {
    hipExtLaunchKernelGGL(bgprep_kernel, dim3((W * H + 255) / 256, n), dim3(256), 0, s, start, stop, 0, rec, W, H, tex);
    HIP_OK(c, hipGetLastError());
    return OFDG_OK;
  }
  const DevResizeTabs T{c->d_bg_at_x.p, c->d_bg_alpha_x.p, c->d_bg_at_y.p, c->d_bg_alpha_y.p};
  if (fusable && n <= kPrepMaxSamples) {
    hipExtLaunchKernelGGL(bgprep_stream_kernel, dim3(kPrepGrid), dim3(64), (size_t)(n + 1) * sizeof(int), s, start, stop, 0, rec, T, W, H, n, cap_cw, cap_ch, tex, err,
                          c->d_prep_paths.p);
    HIP_OK(c, hipGetLastError());
    return OFDG_OK;
  }
  HIP_OK(c, sl.d_bgC.reserve((size_t)n * cap_cw * cap_ch));
  hipExtLaunchKernelGGL(bgprep_rotcrop_kernel, dim3(kBgPrepBlocks, n), dim3(256), 0, s, start, nullptr, 0, rec, T, W, H, cap_cw, cap_ch, sl.d_bgC.p,
                        err);
  hipExtLaunchKernelGGL(bgprep_resize_kernel, dim3(kBgPrepBlocks, n), dim3(256), 0, s, nullptr, stop, 0, rec, T, W, H, cap_cw, cap_ch, sl.d_bgC.p,
                        tex);
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// realise on the host, stage, and copy the records of one batch into slot `sl`
//   `shared`: the slot may be rendered on other streams than `st` (a caller's slot): the upload is tracked by an event
static int upload_slot(ofdg_ctx* c, ofdg_ctx::Slot& sl, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps,
                       int n_bps, hipStream_t st, ofdg_ctx::Stage& stage, bool shared) {
  if (!c->pool.p && !c->pool_mixed) { c->err = "Could not open texture collection (no texture pool)"; return OFDG_ETEXTURES; }
  OFDG_TRY(finalise_pool(c));
  OFDG_TRY(ensure_tex_table(c));
  RealizeConfig cfg{c->prm.width, c->prm.height, c->prm.mode, c->pool_n, c->pool_w, c->pool_h, c->prm.background_prep};
  cfg.pool_addr = (uint64_t)(uintptr_t)c->pool.p;
  cfg.tex_table = c->pool_mixed && c->prm.background_prep ? c->tex_table.data() : nullptr;
  cfg.fg_stride = c->fg_src.stride; cfg.fg_origin = c->fg_src.origin; cfg.bg_stride = c->bg_src.stride; cfg.bg_origin = c->bg_src.origin;
  // the previous copies out of this staging buffer must have left it
  if (stage.pending) {  // (normally long done - the chain has rendered three other batches since: a query costs 0.1 us, a wait 1 us)
    if (hipEventQuery(stage.free_ev) != hipSuccess) HIP_OK(c, hipEventSynchronize(stage.free_ev));
    stage.pending = false;
  }
  // a compose on another stream may still read the records this upload replaces
  if (sl.compose_pending && sl.compose_stream != st) {
    HIP_OK(c, hipStreamWaitEvent(st, sl.compose_event, 0));
    sl.compose_pending = false;
  }
  sl.res_samples = 0;
  OFDG_TRY(realize_batch(cfg, tasks, n_tasks, bps, n_bps, &sl.batch, &c->err, &c->crop_server));
  const RealizedBatch& B = sl.batch;
  const size_t n_shapes = B.shapes.size(), n_obj = B.objects.size();
  // the batch's records - shapes | objects | samples - travel as ONE copy into one allocation (three copies cost the host
  // 7 us a batch, one 2.5: tools/microbench/launch_cost.hip - most of what a batch of one sample costs)
  const size_t b_shapes = (n_shapes * sizeof(DevShape) + 255) & ~(size_t)255, b_obj = (n_obj * sizeof(DevObject) + 255) & ~(size_t)255,
               b_smp = ((size_t)n_tasks * sizeof(DevSample) + 255) & ~(size_t)255,
               b_prep = c->prm.background_prep ? B.bgprep.size() * sizeof(DevBgPrep) : 0;  // (the background preparation's records ride along)
  const size_t need = b_shapes + b_obj + b_smp + b_prep + 64;
  if (need > sl.d_rec.cap) {  // (growing waits for the device: a compose of this slot may still read the old arena)
    HIP_OK(c, hipDeviceSynchronize());
    HIP_OK(c, sl.d_rec.reserve(need));
  }
  HIP_OK(c, sl.d_shapes.alias((DevShape*)sl.d_rec.p, n_shapes));
  HIP_OK(c, sl.d_objects.alias((DevObject*)(sl.d_rec.p + b_shapes), n_obj));
  HIP_OK(c, sl.d_samples.alias((DevSample*)(sl.d_rec.p + b_shapes + b_obj), (size_t)n_tasks));
  if (b_prep) HIP_OK(c, sl.d_bgprep.alias((DevBgPrep*)(sl.d_rec.p + b_shapes + b_obj + b_smp), B.bgprep.size()));
  OFDG_TRY(size_slot(c, sl, n_tasks, n_shapes));
  if (need > stage.h.bytes) HIP_OK(c, stage.h.alloc(need * 2, hipHostMallocDefault));
  char* hs = (char*)stage.h.p;
  if (n_shapes) std::memcpy(hs, B.shapes.data(), n_shapes * sizeof(DevShape));
  std::memcpy(hs + b_shapes, B.objects.data(), n_obj * sizeof(DevObject));
  std::memcpy(hs + b_shapes + b_obj, B.samples.data(), (size_t)n_tasks * sizeof(DevSample));
  if (b_prep) std::memcpy(hs + b_shapes + b_obj + b_smp, B.bgprep.data(), b_prep);
  HIP_OK(c, hipMemcpyAsync(sl.d_rec.p, hs, b_shapes + b_obj + b_smp + b_prep, hipMemcpyHostToDevice, st));
  if (!B.crops.empty()) {  // mode 9: this batch's crop table (+ upscaled background copies)
    const int W = c->prm.width, H = c->prm.height;
    const size_t crop_floats = (size_t)4 * (W + 1) * (H + 1), bg_floats = (size_t)4 * 2 * W * 2 * H;
    size_t n_bg = 0;
    for (const CropUse& u : B.crops) n_bg += u.background ? 1 : 0;
    HIP_OK(c, sl.d_croptab.reserve(B.crops.size()));
    if (n_bg) {
      HIP_OK(c, sl.d_bgwarp.reserve(n_bg * bg_floats));
      HIP_OK(c, sl.d_bgwarp_max.reserve(n_bg));
      HIP_OK(c, hipMemsetAsync(sl.d_bgwarp_max.p, 0, n_bg * sizeof(unsigned), st));
      OFDG_TRY(ensure_resize_tables(c));
    }
    std::vector<DevCropRef> tab(B.crops.size());
    size_t bg_at = 0;
    for (size_t k = 0; k < B.crops.size(); ++k) {
      const float* src = c->d_warp.p + (size_t)B.crops[k].crop * crop_floats;
      if (B.crops[k].background) {
        OFDG_TRY(upscale_crop(c, src, sl.d_bgwarp.p + bg_at * bg_floats, sl.d_bgwarp_max.p + bg_at, st, &tab[k]));
        ++bg_at;
      } else {
        tab[k] = make_crop_ref(src, c->d_warp_max.p + B.crops[k].crop, W + 1, H + 1);
      }
    }
    // small table: a synchronous copy from pageable memory is fine here (upload path)
    HIP_OK(c, hipMemcpyAsync(sl.d_croptab.p, tab.data(), tab.size() * sizeof(DevCropRef), hipMemcpyHostToDevice, st));
    HIP_OK(c, hipStreamSynchronize(st));  // `tab` is a stack vector
  }
  if (c->prm.background_prep) {
    if (shared) {  // a caller's slot is prepared once, here, and rendered any number of times
      // (flags go into the word of the call that renders this batch next; that call must not clear them: word_reserved)
      if (c->word_reserved != c->ticket) { HIP_OK(c, take_err_word(c, c->ticket, st)); c->word_reserved = c->ticket; }
      OFDG_TRY(prepare_backgrounds(c, sl, n_tasks, /*records_resident=*/true, st, err_word(c, c->ticket)));
      sl.bgprep_pending = false;
    } else {
      sl.bgprep_pending = true;  // (a chain's private slot: behind raster, launch_prepare)
    }
  }
  HIP_OK(c, hipEventRecord(stage.free_ev, st));
  stage.pending = true;
  if (shared) {
    if (!sl.ev_uploaded.e) HIP_OK(c, sl.ev_uploaded.create(hipEventDisableTiming));
    HIP_OK(c, hipEventRecord(sl.ev_uploaded, st));
    sl.upload_pending = true;
    sl.upload_stream = st;
  } else {
    sl.upload_pending = false;  // (a chain's private slot: uploaded and rendered in order on the chain's own stream)
  }
  sl.res_samples = n_tasks;
  sl.res_shapes = (int)n_shapes;
  sl.res_objects = (int)n_obj;
  return OFDG_OK;
}

// ofdg_render / _ex / _fmt / _ex_fmt: the batch's records travel on the chain's own stream into its private slot
static int render_impl(ofdg_ctx* c, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, int n_bps, const CallOut& o, void* stream) {
  stream = own_stream(c, stream);
  ofdg_ctx::Chain& ch = take_chain(c);
  OFDG_TRY(upload_slot(c, ch.slot, tasks, n_tasks, bps, n_bps, chain_stream(c, ch, (hipStream_t)stream), ch.stage, false));
  return launch_resident(c, ch, ch.slot, o, (hipStream_t)stream);
}
static bool render_args_ok(const ofdg_ctx* c, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, const void* d_img0,
                           const void* d_img1, const void* d_flow) {
  return c && tasks && bps && n_tasks >= 1 && d_img0 && d_img1 && d_flow;
}
int ofdg_render(ofdg_ctx* c, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, int n_bps,
                float* d_img0, float* d_img1, float* d_flow, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_render", render_args_ok(c, tasks, n_tasks, bps, d_img0, d_img1, d_flow),
                      d_img0, d_img1, d_flow, nullptr, nullptr, nullptr, &o));
  return render_impl(c, tasks, n_tasks, bps, n_bps, o, stream);
}
int ofdg_render_ex(ofdg_ctx* c, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, int n_bps,
                   float* d_img0, float* d_img1, float* d_flow, const ofdg_extras* ex, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_render_ex", render_args_ok(c, tasks, n_tasks, bps, d_img0, d_img1, d_flow),
                      d_img0, d_img1, d_flow, ex, nullptr, nullptr, &o, /*args_fn=*/"ofdg_render"));  // (as it always has)
  return render_impl(c, tasks, n_tasks, bps, n_bps, o, stream);
}
int ofdg_render_fmt(ofdg_ctx* c, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, int n_bps,
                    void* d_img0, void* d_img1, void* d_flow, const ofdg_out_format* fmt, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_render_fmt", render_args_ok(c, tasks, n_tasks, bps, d_img0, d_img1, d_flow),
                      d_img0, d_img1, d_flow, nullptr, nullptr, fmt, &o));
  return render_impl(c, tasks, n_tasks, bps, n_bps, o, stream);
}
int ofdg_render_ex_fmt(ofdg_ctx* c, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, int n_bps,
                       void* d_img0, void* d_img1, void* d_flow, const ofdg_extras_fmt* ex, const ofdg_out_format* fmt, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_render_ex_fmt", render_args_ok(c, tasks, n_tasks, bps, d_img0, d_img1, d_flow),
                      d_img0, d_img1, d_flow, nullptr, ex, fmt, &o));
  return render_impl(c, tasks, n_tasks, bps, n_bps, o, stream);
}

int ofdg_upload_slot(ofdg_ctx* c, int slot, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, int n_bps,
                     void* stream) {
  if (!c || !tasks || !bps || n_tasks < 1 || slot < 0 || slot >= ofdg_ctx::kUserSlots) return invalid_argument(c, "ofdg_upload_slot");
  return upload_slot(c, c->slots[slot], tasks, n_tasks, bps, n_bps, (hipStream_t)stream, c->user_stage, true);
}

int ofdg_render_slot(ofdg_ctx* c, int slot, float* d_img0, float* d_img1, float* d_flow, void* stream) {
  if (!c || !d_img0 || !d_img1 || !d_flow || slot < 0 || slot >= ofdg_ctx::kUserSlots) return invalid_argument(c, "ofdg_render_slot");
  if (c->slots[slot].res_samples <= 0) { c->err = "ofdg_render_slot: no batch is resident in this slot"; return OFDG_EINVAL; }
  stream = own_stream(c, stream);
  return launch_resident(c, take_chain(c), c->slots[slot], CallOut{"ofdg_render_slot", d_img0, d_img1, d_flow, {}, 0}, (hipStream_t)stream);
}

int ofdg_render_resident(ofdg_ctx* c, float* d_img0, float* d_img1, float* d_flow, void* stream) {
  if (!c || !d_img0 || !d_img1 || !d_flow) return invalid_argument(c, "ofdg_render_resident");
  if (!c->last_slot || c->last_slot->res_samples <= 0) { c->err = "ofdg_render_resident: nothing has been rendered yet"; return OFDG_EINVAL; }
  stream = own_stream(c, stream);
  // a chain's private slot is not tracked by events while only that chain uses it: let its owner drain first
  for (int k = 0; k < c->n_chains; ++k)
    if (&c->chains[k].slot == c->last_slot && !c->last_slot->compose_pending) HIP_OK(c, hipStreamSynchronize(c->chains[k].stream));
  // (the batch the last call composed: of a slot that was filled for a group of batches, that call's samples)
  const int view_base = c->last_base, view_n = c->last_n;
  return launch_resident(c, take_chain(c), *c->last_slot, CallOut{"ofdg_render_resident", d_img0, d_img1, d_flow, {}, 0}, (hipStream_t)stream, -1,
                         view_base, view_n);
}

// The per-object annotation table of the batch the last render / forward call composed (c->last_slot): two small kernels on
// `stream` - the stream the labels were written on - that read the slot's records and the caller's label planes.  Nothing but
// argument checks happens on the host.
int ofdg_object_table(ofdg_ctx* c, const uint8_t* d_label0, const uint8_t* d_label1, ofdg_object_row* d_rows, int rows_per_sample,
                      int32_t* d_counts, void* stream) {
  if (!c) return OFDG_EINVAL;
  const PostOp op{c, "ofdg_object_table"};
  if (c->prm.mode == 9) return op.fail("the table restates the label planes, which are defined for the rigid modes only (mode 9)");
  if (!d_rows) return op.fail("d_rows is NULL");
  if (!d_counts) return op.fail("d_counts is NULL");
  if (rows_per_sample < 1) return op.fail("rows_per_sample = " + std::to_string(rows_per_sample) + " (valid: >= 1)");
  if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_counts & 3) || plane_misaligned(d_label0, OFDG_FMT_U8) || plane_misaligned(d_label1, OFDG_FMT_U8))
    return op.fail("d_rows must be 8-byte aligned, d_counts and the label planes 4-byte aligned");
  if (!c->last_slot || !c->last_ch || c->last_slot->res_samples <= 0)
    return op.fail("no render / forward call has been made yet on this context");
  ofdg_ctx::Slot& sl = *c->last_slot;
  ofdg_ctx::Chain& ch = *c->last_ch;
  const hipStream_t S = c->last_stream;  // the internal stream that call worked on
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const int W = c->prm.width, H = c->prm.height, n = c->last_n;
  const DevSample* const samples = sl.d_samples.p + c->last_base;  // (the batch that call composed: a slot may hold several)
  // The slot's records must outlive the kernels.  On the chain's own stream the order of the stream sees to that (a private
  // slot is rewritten there only); on a caller's stream - or for a caller's slot, which any stream may rewrite - the last
  // kernel carries the chain's completion event, as a compose on a caller's stream does (launch_compose): a later call
  // that reuses the slot or the chain's workspaces waits for it.
  const bool tracked = st != S || &sl != &ch.slot;
  const hipEvent_t done = tracked ? ch.ev_done.e : nullptr;
  const bool reduce = d_label0 || d_label1;
  DevObjectRow* const rows = reinterpret_cast<DevObjectRow*>(d_rows);
  const long long cells = (long long)n * rows_per_sample;
  hipExtLaunchKernelGGL(object_table_header_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, nullptr, reduce ? nullptr : done, 0,
                        samples, sl.d_objects.p, sl.d_shapes.p, n, rows_per_sample, W, H, rows, d_counts);
  HIP_OK(c, hipGetLastError());
  if (reduce) {
    hipExtLaunchKernelGGL(object_table_reduce_kernel, dim3((unsigned)((H + kTabBand - 1) / kTabBand), 2, (unsigned)n), dim3(64 * kTabWaves), 0,
                          st, nullptr, done, 0, samples, d_label0, d_label1, W, H, rows_per_sample, rows);
    HIP_OK(c, hipGetLastError());
  }
  if (tracked) track_completion(sl, ch, st, done);
  return OFDG_OK;
}

// The two reductions and the crop read nothing of the context's own (no slot record, no workspace), so no completion
// bookkeeping is needed on any stream.  A flow with its optional occlusion map as they take it:
static int flow_planes_aligned(const PostOp& op, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt) {
  OFDG_TRY(op.aligned("d_flow", d_flow, flow_fmt));
  return op.aligned("d_occ", d_occ, occ_fmt);
}

// Flow statistics of caller-given planes: the clearing of the rows and one kernel on `stream`.
// (op.who: the entry's name; W, H: the context's frame, or the plane size a sized call gave and checked)
static int flow_stats_on(const PostOp& op, int W, int H, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt, int n_samples,
                         float bin_px, int flags, ofdg_flow_stats_row* d_rows, void* stream) {
  ofdg_ctx* const c = op.c;
  if (const char* why = flow_stats_arg_error(d_flow, flow_fmt, d_occ, occ_fmt, n_samples, W, H, bin_px, flags, d_rows)) return op.fail(why);
  OFDG_TRY(flow_planes_aligned(op, d_flow, flow_fmt, d_occ, occ_fmt));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const bool one_row = flags & OFDG_STATS_ONE_ROW;
  if (!(flags & OFDG_STATS_ACCUMULATE))
    HIP_OK(c, hipMemsetAsync(d_rows, 0, sizeof(ofdg_flow_stats_row) * (one_row ? 1 : (size_t)n_samples), st));
  const uint32_t plane_quads = (uint32_t)((size_t)W * H / 4);  // (W % 8 == 0: whole quads)
  const dim3 grid((plane_quads + kStatsQuads - 1) / kStatsQuads, (unsigned)std::min(n_samples, 65535));
  DevFlowStatsRow* const rows = reinterpret_cast<DevFlowStatsRow*>(d_rows);
  const float inv_bin = 1.0f / bin_px;
  const int vis = (flags & OFDG_STATS_VISIBLE_ONLY) ? 1 : 0, one = one_row ? 1 : 0;
  with_bool(flow_fmt == OFDG_FMT_F16, [&](auto half) {
    with_occ_kind(d_occ, occ_fmt, [&](auto occ) {
      hipLaunchKernelGGL((flow_stats_kernel<decltype(half)::value, decltype(occ)::value>), grid, dim3(kStatsThreads), 0, st, d_flow, d_occ,
                         n_samples, plane_quads, bin_px, inv_bin, vis, one, rows);
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}
int ofdg_flow_stats(ofdg_ctx* c, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt, int n_samples, float bin_px,
                    int flags, ofdg_flow_stats_row* d_rows, void* stream) {
  if (!c) return OFDG_EINVAL;
  return flow_stats_on(PostOp{c, "ofdg_flow_stats"}, c->prm.width, c->prm.height, d_flow, flow_fmt, d_occ, occ_fmt, n_samples, bin_px, flags, d_rows, stream);
}
int ofdg_flow_stats_sized(ofdg_ctx* c, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt, int n_samples, int width, int height,
                          float bin_px, int flags, ofdg_flow_stats_row* d_rows, void* stream) {
  if (!c) return OFDG_EINVAL;
  const PostOp op{c, "ofdg_flow_stats_sized"};
  if (const char* why = plane_size_error(width, height)) return op.fail(why);
  return flow_stats_on(op, width, height, d_flow, flow_fmt, d_occ, occ_fmt, n_samples, bin_px, flags, d_rows, stream);
}

// Flow pyramid of caller-given planes: one kernel on `stream`.
static int flow_pyramid_on(const PostOp& op, int W, int H, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt, int n_samples,
                           int flags, const struct ofdg_flow_pyramid* pyr, void* stream) {
  ofdg_ctx* const c = op.c;
  const DevFlowPyramid* const out = reinterpret_cast<const DevFlowPyramid*>(pyr);
  if (const char* why = flow_pyramid_arg_error(d_flow, flow_fmt, d_occ, occ_fmt, n_samples, W, H, flags, out)) return op.fail(why);
  OFDG_TRY(flow_planes_aligned(op, d_flow, flow_fmt, d_occ, occ_fmt));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  DevFlowPyramid arg = *out;
  for (int k = arg.levels; k < kPyrMaxLevels; ++k) arg.flow[k] = arg.weight[k] = nullptr;  // (never read: nothing of them travels)
  const dim3 grid((unsigned)((W + kPyrTile - 1) / kPyrTile), (unsigned)((H + kPyrTile - 1) / kPyrTile), (unsigned)std::min(n_samples, 65535));
  const int scaled = (flags & OFDG_PYR_SCALE) ? 1 : 0, n_weights = arg.weight[0] ? 1 : 0;
  with_bool(flow_fmt == OFDG_FMT_F16, [&](auto half) {
    with_bool(pyr->out_fmt == OFDG_FMT_F16, [&](auto half_out) {
      with_occ_kind(d_occ, occ_fmt, [&](auto occ) {
        hipLaunchKernelGGL((flow_pyramid_kernel<decltype(half)::value, decltype(half_out)::value, decltype(occ)::value>), grid, dim3(kPyrThreads), 0,
                           st, d_flow, d_occ, n_samples, W, H, scaled, n_weights, arg);
      });
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}
int ofdg_flow_pyramid(ofdg_ctx* c, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt, int n_samples, int flags,
                      const struct ofdg_flow_pyramid* pyr, void* stream) {
  if (!c) return OFDG_EINVAL;
  return flow_pyramid_on(PostOp{c, "ofdg_flow_pyramid"}, c->prm.width, c->prm.height, d_flow, flow_fmt, d_occ, occ_fmt, n_samples, flags, pyr, stream);
}
int ofdg_flow_pyramid_sized(ofdg_ctx* c, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt, int n_samples, int width, int height,
                            int flags, const struct ofdg_flow_pyramid* pyr, void* stream) {
  if (!c) return OFDG_EINVAL;
  const PostOp op{c, "ofdg_flow_pyramid_sized"};
  if (const char* why = plane_size_error(width, height)) return op.fail(why);
  return flow_pyramid_on(op, width, height, d_flow, flow_fmt, d_occ, occ_fmt, n_samples, flags, pyr, stream);
}

// Training crop of caller-given planes: one kernel on `stream` for every plane and sample.
int ofdg_crop(ofdg_ctx* c, const struct ofdg_crop_job* job, int n_samples, void* stream) {
  if (!c) return OFDG_EINVAL;
  const PostOp op{c, "ofdg_crop"};
  const int W = c->prm.width, H = c->prm.height;
  const DevCropJob* const j = reinterpret_cast<const DevCropJob*>(job);
  if (const char* why = crop_arg_error(j, n_samples, W, H)) return op.fail(why);
  static const char* const kPlane[kCropPlanes] = {"image0", "image1", "flow", "flow1", "occ0", "occ1", "label0", "label1"};
  for (int k = 0; k < kCropPlanes; ++k) {
    if (!j->src[k]) continue;
    OFDG_TRY(op.aligned(std::string("src[") + kPlane[k] + "]", j->src[k], crop_plane_fmt(*j, k), /*say_fmt=*/false));
    OFDG_TRY(op.aligned16(j->dst[k], "dst[", kPlane[k], "]"));
  }
  OFDG_TRY(op.aligned16(j->recs, "recs"));
  OFDG_TRY(op.aligned16(j->recs_out, "recs_out"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  DevCropGrid grid;
  uint32_t blocks = 0;
  for (int k = 0, slot = 0; k < kCropPlanes; ++k) {
    const uint32_t pieces = (uint32_t)((size_t)j->crop_w * j->crop_h * crop_elem_bytes(*j, k) / 16);
    const uint32_t per_channel = j->src[k] ? (pieces + kCropThreads * kCropPerLane - 1) / (kCropThreads * kCropPerLane) : 0u;
    for (int ch = 0; ch < crop_channels(k); ++ch, ++slot) {
      grid.first_block[slot] = blocks;
      blocks += per_channel;
    }
  }
  grid.first_block[kCropSlots] = blocks;
  const dim3 g(blocks, (unsigned)std::min(n_samples, 65535));
  with_bool(j->image_fmt == OFDG_FMT_U8, [&](auto image_u8) {
    with_bool(j->flow_fmt == OFDG_FMT_F16, [&](auto flow_half) {
      with_bool(j->occ_fmt == OFDG_FMT_U8, [&](auto occ_u8) {
        hipLaunchKernelGGL((crop_kernel<decltype(image_u8)::value, decltype(flow_half)::value, decltype(occ_u8)::value>), g, dim3(kCropThreads), 0,
                           st, *j, grid, n_samples, W, H);
      });
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Photometric augmentation of caller-given frames: one kernel on `stream` for both frames, every channel and sample.
int ofdg_photo(ofdg_ctx* c, const struct ofdg_photo_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_photo"};
  const DevPhotoJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevPhotoJob>, photo_arg_error, &j, &W, &H));
  OFDG_TRY(op.frame_pair_aligned(*j));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const uint32_t plane = (uint32_t)W * (uint32_t)H;
  const uint32_t per_channel = (plane + kPhotoBlockPixels - 1) / kPhotoBlockPixels;
  const dim3 g(per_channel * 3u * ((j->src[0] ? 1u : 0u) + (j->src[1] ? 1u : 0u)), (unsigned)std::min(n_samples, 65535));
  with_bool(j->src_fmt == OFDG_FMT_U8, [&](auto src_u8) {
    with_bool(j->dst_fmt == OFDG_FMT_U8, [&](auto dst_u8) {
      hipLaunchKernelGGL((photo_kernel<decltype(src_u8)::value, decltype(dst_u8)::value>), g, dim3(kPhotoThreads), 0, st, *j, n_samples, W, H, per_channel);
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Spatial augmentation of caller-given planes: one kernel on `stream` for every plane, both frames and every sample.
int ofdg_spatial(ofdg_ctx* c, const struct ofdg_spatial_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_spatial"};
  const DevSpatialJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, spatial_plane_size, spatial_arg_error, &j, &W, &H));
  static const char* const kPlane[kCropPlanes] = {"image0", "image1", "flow", "flow1", "occ0", "occ1", "label0", "label1"};
  for (int k = 0; k < kCropPlanes; ++k) {
    if (!j->src[k]) continue;
    const int fmt = k < 2 ? j->image_fmt : k < 4 ? j->flow_fmt : k < 6 ? j->occ_fmt : OFDG_FMT_U8;
    OFDG_TRY(op.aligned(std::string("src[") + kPlane[k] + "]", j->src[k], fmt, /*say_fmt=*/false));
    OFDG_TRY(op.aligned16(j->dst[k], "dst[", kPlane[k], "]"));
  }
  OFDG_TRY(op.aligned16(j->recs, "recs"));
  OFDG_TRY(op.aligned16(j->recs_out, "recs_out"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const bool frame0 = j->src[0] || j->src[2] || j->src[4] || j->src[6], frame1 = j->src[1] || j->src[3] || j->src[5] || j->src[7];
  const uint32_t tiles_x = ((uint32_t)j->out_w / 8u + kSpatialTileQ - 1) / kSpatialTileQ;
  const uint32_t tiles_y = ((uint32_t)j->out_h / 2u + kSpatialTileP - 1) / kSpatialTileP;
  const dim3 g(tiles_x * tiles_y, (unsigned)std::min(n_samples, 65535), (frame0 ? 1u : 0u) + (frame1 ? 1u : 0u));
  with_bool(j->image_fmt == OFDG_FMT_U8, [&](auto image_u8) {
    with_bool(j->flow_fmt == OFDG_FMT_F16, [&](auto flow_half) {
      with_bool(j->occ_fmt == OFDG_FMT_U8, [&](auto occ_u8) {
        hipLaunchKernelGGL((spatial_kernel<decltype(image_u8)::value, decltype(flow_half)::value, decltype(occ_u8)::value>), g, dim3(kSpatialThreads), 0,
                           st, *j, n_samples, W, H, tiles_x);
      });
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Network-ready packing of caller-given planes: one kernel on `stream` for both frames, the flow and every sample.
int ofdg_pack(ofdg_ctx* c, const struct ofdg_pack_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_pack"};
  const DevPackJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevPackJob>, pack_arg_error, &j, &W, &H));
  static const char* const kPlane[kPackPlanes] = {"image0", "image1", "flow"};
  for (int k = 0; k < kPackPlanes; ++k) {
    if (!j->src[k]) continue;
    OFDG_TRY(op.aligned(std::string("src[") + kPlane[k] + "]", j->src[k], k == OFDG_PACK_FLOW ? j->flow_src_fmt : j->image_src_fmt, /*say_fmt=*/false));
    OFDG_TRY(op.aligned16(j->dst[k], "dst[", kPlane[k], "]"));
  }
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const bool concat = j->flags & OFDG_PACK_CONCAT;
  const uint32_t units = (uint32_t)W * (uint32_t)H / 8u, per_group = (units + kPackThreads - 1) / kPackThreads;
  const uint32_t groups = (concat ? 1u : (j->src[OFDG_PACK_IMAGE0] ? 1u : 0u) + (j->src[OFDG_PACK_IMAGE1] ? 1u : 0u)) + (j->src[OFDG_PACK_FLOW] ? 1u : 0u);
  const dim3 g(per_group * groups, (unsigned)std::min(n_samples, 65535));
  with_bool(j->image_src_fmt == OFDG_FMT_U8, [&](auto image_u8) {
    with_constant<int, OFDG_FMT_F32, OFDG_FMT_F16, OFDG_FMT_BF16>(j->image_dst_fmt, [&](auto image_dst) {
      with_bool(j->layout == OFDG_PACK_NHWC, [&](auto nhwc) {
        with_bool(concat, [&](auto both) {
          hipLaunchKernelGGL((pack_kernel<decltype(image_u8)::value, decltype(image_dst)::value, decltype(nhwc)::value, decltype(both)::value>), g,
                             dim3(kPackThreads), 0, st, *j, n_samples, W, H, per_group);
        });
      });
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Motion boundaries of caller-given flows: one kernel on `stream` for both frames, both outputs and every sample.
int ofdg_boundaries(ofdg_ctx* c, const struct ofdg_boundary_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_boundaries"};
  const DevBoundaryJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevBoundaryJob>, boundary_arg_error, &j, &W, &H));
  const bool labels = j->flags & OFDG_BND_LABELS;
  for (int f = 0; f < 2; ++f) {
    if (!j->flow[f]) continue;
    OFDG_TRY(op.aligned(f ? "flow[1]" : "flow[0]", j->flow[f], j->flow_fmt));
    OFDG_TRY(op.aligned(f ? "label[1]" : "label[0]", j->label[f], OFDG_FMT_U8, /*say_fmt=*/false));
    OFDG_TRY(op.aligned16(j->edge[f], f ? "edge[1]" : "edge[0]"));
    OFDG_TRY(op.aligned16(j->dist2[f], f ? "dist2[1]" : "dist2[0]"));
  }
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const uint32_t tiles_x = ((uint32_t)W + kBndTileW - 1) / kBndTileW, tiles_y = ((uint32_t)H + kBndTileH - 1) / kBndTileH;
  const dim3 g(tiles_x * tiles_y, (unsigned)std::min(n_samples, 65535), (j->flow[0] ? 1u : 0u) + (j->flow[1] ? 1u : 0u));
  with_bool(j->flow_fmt == OFDG_FMT_F16, [&](auto half) {
    with_bool(labels, [&](auto with_labels) {
      hipLaunchKernelGGL((boundary_kernel<decltype(half)::value, decltype(with_labels)::value>), g, dim3(kBndThreads), 0, st, *j, n_samples, W, H, tiles_x);
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Occluder rectangles on caller-given planes, in place: under OFDG_ERASE_MEAN the clearing of `work` and the reduction, then
// one kernel that paints and marks, all on `stream`.
int ofdg_erase(ofdg_ctx* c, const struct ofdg_erase_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_erase"};
  const DevEraseJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevEraseJob>, erase_arg_error, &j, &W, &H, /*with_work=*/true));
  const bool mark = j->flags & OFDG_ERASE_OCC, mean = j->fill == OFDG_ERASE_MEAN;
  for (int f = 0; f < 2; ++f) {
    if ((j->flags >> f) & 1) OFDG_TRY(op.aligned(f ? "image[1]" : "image[0]", j->image[f], j->image_fmt));
    if (mark) OFDG_TRY(op.aligned(f ? "occ[1]" : "occ[0]", j->occ[f], j->occ_fmt));
    if (erase_cross(*j, f)) OFDG_TRY(op.aligned(f ? "flow[1]" : "flow[0]", j->flow[f], j->flow_fmt));
  }
  OFDG_TRY(op.aligned16(j->recs, "recs"));
  OFDG_TRY(op.aligned16(j->recs_out, "recs_out"));
  if (mean) OFDG_TRY(op.aligned16(j->work, "work"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const uint32_t plane = (uint32_t)W * (uint32_t)H;
  const unsigned ny = (unsigned)std::min(n_samples, 65535);
  if (mean) {
    HIP_OK(c, hipMemsetAsync(j->work, 0, sizeof(DevEraseWork) * (size_t)n_samples, st));
    const uint32_t per_channel = (plane + kEraseMeanPixels - 1) / kEraseMeanPixels;
    const dim3 g(per_channel * 3u * ((j->flags & 3) == 3 ? 2u : 1u), ny);
    with_bool(j->image_fmt == OFDG_FMT_U8, [&](auto image_u8) {
      hipLaunchKernelGGL((erase_mean_kernel<decltype(image_u8)::value>), g, dim3(kEraseThreads), 0, st, *j, n_samples, W, H, per_channel);
    });
    HIP_OK(c, hipGetLastError());
  }
  const uint32_t occ_blocks = (plane / 4u + kEraseOccQuads - 1) / kEraseOccQuads;
  const uint32_t maps = mark ? (j->occ[0] ? 1u : 0u) + (j->occ[1] ? 1u : 0u) : 0u;
  const dim3 g((uint32_t)kEraseFillBlocks + occ_blocks * maps, ny);
  with_bool(j->image_fmt == OFDG_FMT_U8, [&](auto image_u8) {
    with_bool(mark && j->occ_fmt == OFDG_FMT_U8, [&](auto occ_u8) {
      with_bool(mark && j->flow_fmt == OFDG_FMT_F16, [&](auto half) {
        hipLaunchKernelGGL((erase_apply_kernel<decltype(image_u8)::value, decltype(occ_u8)::value, decltype(half)::value>), g, dim3(kEraseThreads), 0, st,
                           *j, n_samples, W, H, occ_blocks);
      });
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Colour jitter of caller-given frames: where a record may hold a contrast the clearing of `work` and the reduction, then one
// kernel for both frames and every sample, all on `stream`.
int ofdg_jitter(ofdg_ctx* c, const struct ofdg_jitter_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_jitter"};
  const DevJitterJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevJitterJob>, jitter_arg_error, &j, &W, &H, /*with_work=*/true));
  const bool mean = jitter_needs_work(*j);
  OFDG_TRY(op.frame_pair_aligned(*j));
  if (mean) OFDG_TRY(op.aligned16(j->work, "work"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const uint32_t plane = (uint32_t)W * (uint32_t)H;
  const uint32_t per_frame = (plane + kJitterBlockPixels - 1) / kJitterBlockPixels;
  const dim3 g(per_frame * ((j->src[0] ? 1u : 0u) + (j->src[1] ? 1u : 0u)), (unsigned)std::min(n_samples, 65535));
  if (mean) {
    HIP_OK(c, hipMemsetAsync(j->work, 0, sizeof(DevJitterWork) * (size_t)n_samples, st));
    with_bool(j->src_fmt == OFDG_FMT_U8, [&](auto src_u8) {
      hipLaunchKernelGGL((jitter_mean_kernel<decltype(src_u8)::value>), g, dim3(kJitterThreads), 0, st, *j, n_samples, W, H, per_frame);
    });
    HIP_OK(c, hipGetLastError());
  }
  with_bool(j->src_fmt == OFDG_FMT_U8, [&](auto src_u8) {
    with_bool(j->dst_fmt == OFDG_FMT_U8, [&](auto dst_u8) {
      hipLaunchKernelGGL((jitter_apply_kernel<decltype(src_u8)::value, decltype(dst_u8)::value>), g, dim3(kJitterThreads), 0, st, *j, n_samples, W, H, per_frame);
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// The camera of caller-given frames - lens blur, Bayer mosaic and demosaic -: one kernel on `stream` for both frames and every
// sample.
int ofdg_camera(ofdg_ctx* c, const struct ofdg_camera_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_camera"};
  const DevCameraJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevCameraJob>, camera_arg_error, &j, &W, &H));
  OFDG_TRY(op.frame_pair_aligned(*j));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const uint32_t tiles_x = ((uint32_t)W + kCameraTileW - 1) / kCameraTileW, tiles_y = ((uint32_t)H + kCameraTileH - 1) / kCameraTileH;
  const dim3 g(tiles_x * tiles_y, (unsigned)std::min(n_samples, 65535), (j->src[0] ? 1u : 0u) + (j->src[1] ? 1u : 0u));
  with_bool(j->src_fmt == OFDG_FMT_U8, [&](auto src_u8) {
    with_bool(j->dst_fmt == OFDG_FMT_U8, [&](auto dst_u8) {
      hipLaunchKernelGGL((camera_kernel<decltype(src_u8)::value, decltype(dst_u8)::value>), g, dim3(kCameraThreads), 0, st, *j, n_samples, W, H, tiles_x);
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Motion blur of caller-given frames along their flows: one kernel on `stream` for both frames and every sample.
int ofdg_motion_blur(ofdg_ctx* c, const struct ofdg_mblur_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_motion_blur"};
  const DevMblurJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevMblurJob>, mblur_arg_error, &j, &W, &H));
  for (int f = 0; f < 2; ++f) {
    if (!j->src[f]) continue;
    OFDG_TRY(op.aligned(f ? "src[1]" : "src[0]", j->src[f], j->src_fmt));
    OFDG_TRY(op.aligned(f ? "flow[1]" : "flow[0]", j->flow[f], j->flow_fmt));
    OFDG_TRY(op.aligned16(j->dst[f], f ? "dst[1]" : "dst[0]"));
  }
  OFDG_TRY(op.aligned16(j->recs, "recs"));
  OFDG_TRY(op.aligned16(j->recs_out, "recs_out"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const uint32_t tiles_x = ((uint32_t)W + kMblurTileW - 1) / kMblurTileW, tiles_y = ((uint32_t)H + kMblurTileH - 1) / kMblurTileH;
  const dim3 g(tiles_x * tiles_y, (unsigned)std::min(n_samples, 65535), (j->src[0] ? 1u : 0u) + (j->src[1] ? 1u : 0u));
  with_bool(j->src_fmt == OFDG_FMT_U8, [&](auto src_u8) {
    with_bool(j->dst_fmt == OFDG_FMT_U8, [&](auto dst_u8) {
      with_bool(j->flow_fmt == OFDG_FMT_F16, [&](auto half) {
        hipLaunchKernelGGL((mblur_kernel<decltype(src_u8)::value, decltype(dst_u8)::value, decltype(half)::value>), g, dim3(kMblurThreads), 0, st, *j,
                           n_samples, W, H, tiles_x);
      });
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Reprojection of caller-given frames through their flows: the rows cleared on `stream` unless they accumulate, then one kernel
// for both frames and every sample.
int ofdg_reproject(ofdg_ctx* c, const struct ofdg_reproject_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_reproject"};
  const DevReprojJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, reproj_plane_size, reproj_arg_error, &j, &W, &H));
  for (int f = 0; f < 2; ++f) {
    OFDG_TRY(op.aligned(f ? "img[1]" : "img[0]", j->img[f], j->img_fmt));
    OFDG_TRY(op.aligned(f ? "flow[1]" : "flow[0]", j->flow[f], j->flow_fmt));
    if (j->occ[f]) OFDG_TRY(op.aligned(f ? "occ[1]" : "occ[0]", j->occ[f], j->occ_fmt));
    OFDG_TRY(op.aligned16(j->warped[f], f ? "warped[1]" : "warped[0]"));
    OFDG_TRY(op.aligned16(j->err[f], f ? "err[1]" : "err[0]"));
    OFDG_TRY(op.aligned16(j->mask[f], f ? "mask[1]" : "mask[0]"));
    OFDG_TRY(op.aligned16(j->fb2[f], f ? "fb2[1]" : "fb2[0]"));
  }
  OFDG_TRY(op.aligned16(j->rows, "rows"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  if (j->rows && !(j->flags & OFDG_REPROJ_ACCUMULATE)) HIP_OK(c, hipMemsetAsync(j->rows, 0, sizeof(DevReprojRow) * (size_t)n_samples, st));
  const uint32_t tiles_x = ((uint32_t)W + kReprojTileW - 1) / kReprojTileW, tiles_y = ((uint32_t)H + kReprojTileH - 1) / kReprojTileH;
  const dim3 g(tiles_x * tiles_y, (unsigned)std::min(n_samples, 65535), ((j->flags & OFDG_REPROJ_FRAME0) ? 1u : 0u) + ((j->flags & OFDG_REPROJ_FRAME1) ? 1u : 0u));
  with_bool(j->img_fmt == OFDG_FMT_U8, [&](auto src_u8) {
    with_bool(j->flow_fmt == OFDG_FMT_F16, [&](auto half) {
      hipLaunchKernelGGL((reproject_kernel<decltype(src_u8)::value, decltype(half)::value>), g, dim3(kReprojThreads), 0, st, *j, n_samples, W, H, tiles_x);
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Splat of caller-given frames along their flows: the key planes (and, unless they accumulate, the rows) cleared on `stream`,
// then the scatter and the resolve, each one kernel for both frames and every sample.
int ofdg_splat(ofdg_ctx* c, const struct ofdg_splat_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_splat"};
  const DevSplatJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, splat_plane_size, splat_arg_error, &j, &W, &H));
  for (int f = 0; f < 2; ++f) {
    const std::string at = f ? "[1]" : "[0]";
    OFDG_TRY(op.aligned("img" + at, j->img[f], j->img_fmt));
    OFDG_TRY(op.aligned("flow" + at, j->flow[f], j->flow_fmt));
    OFDG_TRY(op.aligned("label" + at, j->label[f], OFDG_FMT_U8, false));
    if (j->occ[f]) OFDG_TRY(op.aligned("occ" + at, j->occ[f], j->occ_fmt));
    const std::pair<const char*, const void*> outs[] = {{"keys", j->keys[f]}, {"image", j->image[f]}, {"to_own", j->to_own[f]}, {"to_other", j->to_other[f]},
                                                         {"mask", j->mask[f]}, {"fate", j->fate[f]}};
    for (const auto& o : outs) OFDG_TRY(op.aligned16(o.second, o.first, at.c_str()));
  }
  OFDG_TRY(op.aligned16(j->rows, "rows"));
  OFDG_TRY(op.aligned16(j->recs, "recs"));
  OFDG_TRY(op.aligned16(j->recs_out, "recs_out"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const size_t plane = (size_t)W * (size_t)H;
  for (int f = 0; f < 2; ++f)
    if (j->keys[f]) HIP_OK(c, hipMemsetAsync(j->keys[f], 0, 4 * plane * (size_t)n_samples, st));
  if (j->rows && !(j->flags & OFDG_SPLAT_ACCUMULATE)) HIP_OK(c, hipMemsetAsync(j->rows, 0, sizeof(DevSplatRow) * (size_t)n_samples, st));
  const uint32_t tiles_x = ((uint32_t)W + kSplatTileW - 1) / kSplatTileW, tiles_y = ((uint32_t)H + kSplatTileH - 1) / kSplatTileH;
  const dim3 g(tiles_x * tiles_y, (unsigned)std::min(n_samples, 65535), ((j->flags & OFDG_SPLAT_FRAME0) ? 1u : 0u) + ((j->flags & OFDG_SPLAT_FRAME1) ? 1u : 0u));
  with_bool(j->flow_fmt == OFDG_FMT_F16, [&](auto half) {
    hipLaunchKernelGGL((splat_scatter_kernel<decltype(half)::value>), g, dim3(kSplatThreads), 0, st, *j, n_samples, W, H, tiles_x);
    if (!splat_resolves(*j)) return;
    with_bool(j->img_fmt == OFDG_FMT_U8, [&](auto src_u8) {
      hipLaunchKernelGGL((splat_resolve_kernel<decltype(src_u8)::value, decltype(half)::value>), g, dim3(kSplatThreads), 0, st, *j, n_samples, W, H, tiles_x);
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// The colour-wheel picture of a caller-given flow: unless the scale is fixed the clearing of `work` and the maximum's
// reduction, then one kernel for every sample, all on `stream`.
int ofdg_flow_vis(ofdg_ctx* c, const struct ofdg_flow_vis_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_flow_vis"};
  const DevVisJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevVisJob>, vis_arg_error, &j, &W, &H, /*with_work=*/true));
  const bool maxima = vis_needs_work(*j);
  OFDG_TRY(op.aligned("flow", j->flow, j->flow_fmt));
  if (j->occ) OFDG_TRY(op.aligned("occ", j->occ, j->occ_fmt));
  OFDG_TRY(op.aligned16(j->dst, "dst"));
  OFDG_TRY(op.aligned16(j->rows_out, "rows_out"));
  if (maxima) OFDG_TRY(op.aligned16(j->work, "work"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const uint32_t plane = (uint32_t)W * (uint32_t)H;
  const dim3 g((plane + kVisBlockPixels - 1) / kVisBlockPixels, (unsigned)std::min(n_samples, 65535));
  const bool half = j->flow_fmt == OFDG_FMT_F16;
  if (maxima) {
    HIP_OK(c, hipMemsetAsync(j->work, 0, sizeof(unsigned long long) * (size_t)n_samples, st));
    with_bool(half, [&](auto h) { hipLaunchKernelGGL((flow_vis_max_kernel<decltype(h)::value>), g, dim3(kVisThreads), 0, st, *j, n_samples, plane); });
    HIP_OK(c, hipGetLastError());
  }
  with_bool(half, [&](auto h) {
    with_occ_kind((j->flags & OFDG_VIS_DIM_OCC) ? j->occ : nullptr, j->occ_fmt, [&](auto occ_kind) {
      with_bool(j->layout == OFDG_VIS_HWC_RGB, [&](auto hwc) {
        hipLaunchKernelGGL((flow_vis_colour_kernel<decltype(h)::value, decltype(occ_kind)::value, decltype(hwc)::value>), g, dim3(kVisThreads), 0, st, *j,
                           n_samples, plane);
      });
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// The error of a caller-given estimate against a caller-given ground truth: unless the rows are added to their clearing,
// then one kernel for every sample, all on `stream`.
int ofdg_flow_error(ofdg_ctx* c, const struct ofdg_flow_error_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_flow_error"};
  const DevErrJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevErrJob>, err_arg_error, &j, &W, &H));
  OFDG_TRY(op.aligned("gt", j->gt, j->gt_fmt));
  OFDG_TRY(op.aligned("est", j->est, j->est_fmt, /*say_fmt=*/false));
  if (j->occ) OFDG_TRY(op.aligned("occ", j->occ, j->occ_fmt));
  if ((uintptr_t)j->dist2 & 3) return op.fail("dist2 must be 4-byte aligned");
  if ((uintptr_t)j->rows & 7) return op.fail("rows must be 8-byte aligned");
  OFDG_TRY(op.aligned16(j->epe, "epe"));
  OFDG_TRY(op.aligned16(j->picture, "picture"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  if (j->rows && !(j->flags & OFDG_ERR_ACCUMULATE))
    HIP_OK(c, hipMemsetAsync(j->rows, 0, sizeof(DevErrRow) * ((j->flags & OFDG_ERR_ONE_ROW) ? 1 : (size_t)n_samples), st));
  const uint32_t plane = (uint32_t)W * (uint32_t)H;
  const dim3 g((plane + kErrBlockPixels - 1) / kErrBlockPixels, (unsigned)std::min(n_samples, 65535));
  with_bool(j->gt_fmt == OFDG_FMT_F16, [&](auto half) {
    with_constant<int, OFDG_FMT_F32, OFDG_FMT_F16, OFDG_FMT_BF16>(j->est_fmt, [&](auto est) {
      with_bool(j->epe || j->picture, [&](auto planes) {
        hipLaunchKernelGGL((flow_error_kernel<decltype(half)::value, decltype(est)::value, decltype(planes)::value>), g, dim3(kErrThreads), 0, st, *j,
                           n_samples, plane);
      });
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// The lens on caller-given planes: one kernel on `stream` for every plane, both frames and every sample.
int ofdg_lens(ofdg_ctx* c, const struct ofdg_lens_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_lens"};
  const DevLensJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, lens_plane_size, lens_arg_error, &j, &W, &H));
  static const char* const kPlane[kCropPlanes] = {"image0", "image1", "flow", "flow1", "occ0", "occ1", "label0", "label1"};
  for (int k = 0; k < kCropPlanes; ++k) {
    if (!j->src[k]) continue;
    const int fmt = k < 2 ? j->image_fmt : k < 4 ? j->flow_fmt : k < 6 ? j->occ_fmt : OFDG_FMT_U8;
    OFDG_TRY(op.aligned(std::string("src[") + kPlane[k] + "]", j->src[k], fmt, /*say_fmt=*/false));
    OFDG_TRY(op.aligned16(j->dst[k], "dst[", kPlane[k], "]"));
  }
  OFDG_TRY(op.aligned16(j->recs, "recs"));
  OFDG_TRY(op.aligned16(j->recs_out, "recs_out"));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const bool frame0 = j->src[0] || j->src[2] || j->src[4] || j->src[6], frame1 = j->src[1] || j->src[3] || j->src[5] || j->src[7];
  const uint32_t tiles_x = ((uint32_t)W / 8u + kSpatialTileQ - 1) / kSpatialTileQ;
  const uint32_t tiles_y = ((uint32_t)H / 2u + kSpatialTileP - 1) / kSpatialTileP;
  const dim3 g(tiles_x * tiles_y, (unsigned)std::min(n_samples, 65535), (frame0 ? 1u : 0u) + (frame1 ? 1u : 0u));
  with_bool(j->image_fmt == OFDG_FMT_U8, [&](auto image_u8) {
    with_bool(j->flow_fmt == OFDG_FMT_F16, [&](auto flow_half) {
      with_bool(j->occ_fmt == OFDG_FMT_U8, [&](auto occ_u8) {
        hipLaunchKernelGGL((lens_kernel<decltype(image_u8)::value, decltype(flow_half)::value, decltype(occ_u8)::value>), g, dim3(kSpatialThreads), 0,
                           st, *j, n_samples, W, H, tiles_x);
      });
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// Block compression of caller-given frames, in place or into other frames: one kernel on `stream` for both frames and every
// sample.  The grid covers the block grid at its largest phase (15 on either axis).
int ofdg_jpeg(ofdg_ctx* c, const struct ofdg_jpeg_job* job, int n_samples, void* stream) {
  const PostOp op{c, "ofdg_jpeg"};
  const DevJpegJob* j;
  int W, H;
  OFDG_TRY(op.open(job, n_samples, job_plane_size<DevJpegJob>, jpeg_arg_error, &j, &W, &H));
  OFDG_TRY(op.frame_pair_aligned(*j));
  hipStream_t st;
  OFDG_TRY(op.stream_of(stream, &st));
  const uint32_t tiles_x = ((uint32_t)W + 15u + kJpegRegion - 1) / kJpegRegion, tiles_y = ((uint32_t)H + 15u + kJpegRegion - 1) / kJpegRegion;
  const dim3 g(tiles_x * tiles_y, (unsigned)std::min(n_samples, 65535), (j->src[0] ? 1u : 0u) + (j->src[1] ? 1u : 0u));
  with_bool(j->src_fmt == OFDG_FMT_U8, [&](auto src_u8) {
    with_bool(j->dst_fmt == OFDG_FMT_U8, [&](auto dst_u8) {
      hipLaunchKernelGGL((jpeg_kernel<decltype(src_u8)::value, decltype(dst_u8)::value>), g, dim3(kJpegThreads), 0, st, *j, n_samples, W, H, tiles_x);
    });
  });
  HIP_OK(c, hipGetLastError());
  return OFDG_OK;
}

// size slot `sl` for n device-sampled samples: a fixed number of shape slots per sample
// (unused ones are typed 0 and produce no outline)
//   front = N: the slot holds N such batches (a group of the shared front end)
static int prepare_counter_slot(ofdg_ctx* c, ofdg_ctx::Slot& sl, int n, int front = 1) {
  if (c->prm.mode == 9) OFDG_TRY(ensure_counter_croptab(c));
  OFDG_TRY(finalise_pool(c));
  OFDG_TRY(ensure_tex_table(c));
  if (!c->pool.p && !c->pool_mixed) { c->err = "Could not open texture collection (no texture pool)"; return OFDG_ETEXTURES; }
  if (n < 1 || n > 512) { c->err = "counter sampler: batch must be 1..512 samples"; return OFDG_EINVAL; }
  n *= front;
  // outline slots per sample: the worst case, so that no sample can run out (composites have up to 7 parts)
  const int max_objects = c->prm.num_objects > 0 ? std::min(c->prm.num_objects, kCsMaxObjects) : 24;
  const size_t shapes_cap = (size_t)n * (size_t)(c->prm.mode >= 6 ? max_objects * 7 : max_objects);
  const size_t n_obj = (size_t)n * (1 + kCsMaxObjects);
  OFDG_TRY(size_slot(c, sl, n, shapes_cap, n_obj));
  sl.res_samples = n;
  sl.res_shapes = (int)shapes_cap;
  sl.res_objects = (int)n_obj;
  sl.batch.samples.clear();
  return OFDG_OK;
}

// Sample n_samples blueprints with global indices first_index.. on the DEVICE (counter
// sampler: a sample is a pure function of (seed, global index)) and render them.
static int forward_counter_impl(ofdg_ctx* c, long long first_index, int n_samples, const CallOut& o, void* stream) {
  stream = own_stream(c, stream);
  // A sample is a pure function of (seed, global index): the chain samples, realises and prepares the batch on the device
  // and composes it, all in order on its stream.  Like the reference's prefetch thread (data_generation_layer.cpp:141-172)
  // the context runs AHEAD of its caller: after composing batch k it enqueues the preparation of the batches the caller's
  // sequence reaches next (first index + d x the stride of the last two calls, d = 1 .. lookahead) on the chains that
  // will compose them, so a call normally finds its batch prepared and only launches compose.  A call for other samples
  // than the prepared ones prepares its own (nothing is ever rendered from a stale preparation).
  const int k = (int)(c->next_chain % (unsigned)c->n_chains);
  ofdg_ctx::Chain& ch = take_chain(c);
  hipStream_t st = (hipStream_t)stream;
  auto prepare_on = [&](ofdg_ctx::Chain& cj, long long first, hipStream_t s_, bool hand_over) -> int {
    if (cj.prep.valid && cj.prep.slot == &cj.slot && cj.prep.first_index == first && cj.prep.n == n_samples) return OFDG_OK;
    OFDG_TRY(prepare_counter_slot(c, cj.slot, n_samples));
    return launch_prepare(c, cj, cj.slot, s_, first, hand_over);
  };
  const long long prev_first = c->last_first;
  // the stride of the caller's sequence: that of its last two calls, else the sharding rule's
  const long long stride = (prev_first >= 0 && first_index > prev_first) ? first_index - prev_first
                                                                           : (long long)n_samples * std::max(1, c->prm.world_size);
  const bool hand_over = chain_stream(c, ch, st) != st;
  // The shared front end: sampler, geom and raster are latency-bound single-wave kernels whose launches last little longer
  // for several batches than for one, so this chain runs them for a GROUP: its batch and the N - 1 it will be asked for NEXT
  // (n_chains calls on each), and those calls launch only their background preparation and compose.  Stream order and what
  // runs beside what stay as they are.  A call for anything else than the group's next part forgets the rest of it and
  // prepares a group of its own.  (N x n stays within the kPrepMaxSamples a slot was ever sized for: the largest N that does.)
  const int front = (c->overlap && c->lookahead == 0) ? ofdg_front_batches_for(c->front_batches, n_samples) : 1;
  if (front > 1) {
    const ofdg_ctx::Chain::Prepared* const nx = ch.next_part();
    if (nx && nx->slot == &ch.slot && nx->first_index == first_index && nx->n == n_samples && !ch.prep.valid) {
      OFDG_TRY(launch_next_part(c, ch, hand_over));
    } else {
      OFDG_TRY(discard_prepared(c, ch));
      const int group = ch.fresh ? std::min(front, kFrontFirstGroup) : front;
      // (a shorter first group reserves what the whole ones behind it need: growing a workspace waits for the device)
      if (group < front) OFDG_TRY(prepare_counter_slot(c, ch.slot, n_samples, front));
      OFDG_TRY(prepare_counter_slot(c, ch.slot, n_samples, group));
      OFDG_TRY(launch_prepare(c, ch, ch.slot, st, first_index, hand_over, 0, 0, group, (long long)c->n_chains * stride, n_samples));
    }
  } else {
    OFDG_TRY(prepare_on(ch, first_index, st, hand_over));
  }
  OFDG_TRY(launch_compose(c, ch, o, st));
  // (the caller's batch is composed: from here on the call has succeeded, whatever happens to the batches prepared ahead)
  c->last_first = first_index;
  if (c->overlap && c->lookahead > 0) {
    for (int d = 1; d <= std::min(c->lookahead, c->n_chains - 1); ++d) {
      ofdg_ctx::Chain& cj = c->chains[(k + d) % c->n_chains];
      // a preparation ahead that cannot be enqueued is dropped: the call that needs the batch prepares it itself and
      // reports the failure if it persists
      if (prepare_on(cj, first_index + (long long)d * stride, cj.stream, true) != OFDG_OK) { (void)discard_prepared(c, cj); break; }
      cj.prep.ahead = true;
    }
  }
  return OFDG_OK;
}

static bool forward_counter_args_ok(const ofdg_ctx* c, long long first_index, const void* d_img0, const void* d_img1, const void* d_flow) {
  return c && d_img0 && d_img1 && d_flow && first_index >= 0;
}
int ofdg_forward_counter(ofdg_ctx* c, long long first_index, int n_samples, float* d_img0, float* d_img1, float* d_flow,
                         void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_forward_counter", forward_counter_args_ok(c, first_index, d_img0, d_img1, d_flow),
                      d_img0, d_img1, d_flow, nullptr, nullptr, nullptr, &o));
  return forward_counter_impl(c, first_index, n_samples, o, stream);
}
int ofdg_forward_counter_ex(ofdg_ctx* c, long long first_index, int n_samples, float* d_img0, float* d_img1, float* d_flow,
                            const ofdg_extras* ex, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_forward_counter_ex", forward_counter_args_ok(c, first_index, d_img0, d_img1, d_flow),
                      d_img0, d_img1, d_flow, ex, nullptr, nullptr, &o));
  return forward_counter_impl(c, first_index, n_samples, o, stream);
}
int ofdg_forward_counter_fmt(ofdg_ctx* c, long long first_index, int n_samples, void* d_img0, void* d_img1, void* d_flow,
                             const ofdg_out_format* fmt, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_forward_counter_fmt", forward_counter_args_ok(c, first_index, d_img0, d_img1, d_flow),
                      d_img0, d_img1, d_flow, nullptr, nullptr, fmt, &o));
  return forward_counter_impl(c, first_index, n_samples, o, stream);
}
int ofdg_forward_counter_ex_fmt(ofdg_ctx* c, long long first_index, int n_samples, void* d_img0, void* d_img1, void* d_flow,
                                const ofdg_extras_fmt* ex, const ofdg_out_format* fmt, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_forward_counter_ex_fmt", forward_counter_args_ok(c, first_index, d_img0, d_img1, d_flow),
                      d_img0, d_img1, d_flow, nullptr, ex, fmt, &o));
  return forward_counter_impl(c, first_index, n_samples, o, stream);
}

// The internal stream the NEXT render / forward call of this context works on (the chains take turns).
// A caller that passes it as that call's `stream` gets the outputs ordered on it and no cross-stream wait
// at all; with any other stream the compose kernel runs on that stream after one event (standard stream
// semantics: the compose kernels of consecutive calls then run one after the other).
int ofdg_num_chains(const ofdg_ctx* c) { return c ? c->n_chains : OFDG_EINVAL; }
void* ofdg_stream(ofdg_ctx* c) {
  if (!c) return nullptr;
  return (void*)c->chains[c->next_chain % (unsigned)c->n_chains].stream.s;
}

// Download the blueprints the counter sampler produces for samples first_index.. (tests):
// tasks[n], bps[n * 257] in the fixed per-sample layout (background, 32 object slots, 32 x 7
// component slots); unused slots have obj_type 0.
int ofdg_sample_counter(ofdg_ctx* c, long long first_index, int n_samples, ofdg_task* tasks, ofdg_blueprint* bps) {
  if (!c || !tasks || !bps || n_samples < 1 || first_index < 0) return OFDG_EINVAL;
  HIP_OK(c, hipDeviceSynchronize());
  HIP_OK(c, c->d_cs_bps.reserve((size_t)n_samples * kCsBlueprintsPerSample));
  HIP_OK(c, c->d_cs_nobj.reserve(n_samples));
  hipLaunchKernelGGL(cs_sample_kernel, dim3(n_samples * kCsGroups), dim3(64), 0, 0, c->cs_mode, first_index, n_samples,
                     c->prm.mode == 9 ? c->crop_server.n_crops : 0, c->d_cs_bps.p,
                     c->d_cs_nobj.p);
  HIP_OK(c, hipGetLastError());
  std::vector<int> nobj(n_samples);
  HIP_OK(c, hipMemcpy(bps, c->d_cs_bps.p, (size_t)n_samples * kCsBlueprintsPerSample * sizeof(ofdg_blueprint), hipMemcpyDeviceToHost));
  HIP_OK(c, hipMemcpy(nobj.data(), c->d_cs_nobj.p, n_samples * sizeof(int), hipMemcpyDeviceToHost));
  for (int s = 0; s < n_samples; ++s) {
    tasks[s].background = s * kCsBlueprintsPerSample;
    tasks[s].first_object = s * kCsBlueprintsPerSample + 1;
    tasks[s].n_objects = nobj[s];
    tasks[s].reserved = 0;
  }
  return OFDG_OK;
}

// The sharding rule: of the global sample stream, step `step` of rank `rank` renders the `batch` samples
// starting at this index.  The ranks' ranges tile the stream: every index belongs to exactly one (step, rank).
long long ofdg_shard_first_index(long long step, int batch, int world_size, int rank) {
  if (step < 0 || batch < 1 || world_size < 1 || rank < 0 || rank >= world_size) return -1;
  return step * (long long)batch * world_size + (long long)rank * batch;
}

// ofdg_forward / _ex / _fmt / _ex_fmt: the next batch_size samples of this rank's share of the stream.  The output pointers
// are tested here, behind the format and the extras: a failed call leaves the step counter (and the streams) where they were.
static int forward_impl(ofdg_ctx* c, const CallOut& o, void* stream) {
  const int B = c->prm.batch_size, world = c->prm.world_size, rank = c->prm.rank;
  if (B < 1 || rank < 0 || rank >= world) { c->err = "ofdg_forward: bad batch_size / rank"; return OFDG_EINVAL; }
  const bool outputs = o.img0 && o.img1 && o.flow;
  int rc = OFDG_EINVAL;
  if (c->prm.sampler == OFDG_SAMPLER_COUNTER) {
    // rank r owns global indices step*B*world + r*B + [0, B)
    const long long first = ofdg_shard_first_index(c->step, B, world, rank);
    if (!outputs || first < 0) return invalid_argument(c, o.fn);
    rc = forward_counter_impl(c, first, B, o, stream);
    if (rc == OFDG_OK) c->step++;  // (a failed call does not advance the checkpoint counter)
    return rc;
  }
  // every rank walks the identical sequential stream and keeps its own block of
  // B consecutive tasks out of each B*world (disjoint shards, no communication)
  c->fw_bps.clear();
  c->fw_tasks.assign((size_t)B * world, ofdg_task());
  for (int i = 0; i < B * world; ++i) OFDG_TRY(c->sampler->next_task(&c->fw_bps, &c->fw_tasks[i], &c->err));
  if (!outputs) c->err = "ofdg_render: invalid argument";
  else rc = render_impl(c, c->fw_tasks.data() + (size_t)rank * B, B, c->fw_bps.data(), (int)c->fw_bps.size(), o, stream);
  // the streams have moved on either way; the batch counts once it is in flight
  if (rc == OFDG_OK) c->step++;
  else ofdg_set_step(c, c->step);  // rewind the streams (and the crop server) to the start of this batch
  return rc;
}
int ofdg_forward(ofdg_ctx* c, float* d_img0, float* d_img1, float* d_flow, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_forward", c != nullptr, d_img0, d_img1, d_flow, nullptr, nullptr, nullptr, &o));
  return forward_impl(c, o, stream);
}
int ofdg_forward_ex(ofdg_ctx* c, float* d_img0, float* d_img1, float* d_flow, const ofdg_extras* ex, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_forward_ex", c != nullptr, d_img0, d_img1, d_flow, ex, nullptr, nullptr, &o));
  return forward_impl(c, o, stream);
}
int ofdg_forward_fmt(ofdg_ctx* c, void* d_img0, void* d_img1, void* d_flow, const ofdg_out_format* fmt, void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_forward_fmt", c != nullptr, d_img0, d_img1, d_flow, nullptr, nullptr, fmt, &o));
  return forward_impl(c, o, stream);
}
int ofdg_forward_ex_fmt(ofdg_ctx* c, void* d_img0, void* d_img1, void* d_flow, const ofdg_extras_fmt* ex, const ofdg_out_format* fmt,
                        void* stream) {
  CallOut o;
  OFDG_TRY(check_call(c, "ofdg_forward_ex_fmt", c != nullptr, d_img0, d_img1, d_flow, nullptr, ex, fmt, &o));
  return forward_impl(c, o, stream);
}

// Checkpoint / resume of ofdg_forward (the reference has none: a restarted job replays its streams from the
// seeds): the step counter is the whole state.  Counter sampler: the next call renders the indices of `step`.
// Reference-stream sampler: the 45 streams are rebuilt and step * batch_size * world_size tasks are drawn and
// dropped (host, ~30 us per task); in mode 9 the crop server (CropGenerator::get_crop's serving order, WF:516-538)
// is replayed as well: one crop per deforming background / top-level object of THIS rank's tasks.
long long ofdg_get_step(const ofdg_ctx* c) { return c ? c->step : -1; }
int ofdg_set_step(ofdg_ctx* c, long long step) {
  if (!c || step < 0) return OFDG_EINVAL;
  if (c->prm.sampler != OFDG_SAMPLER_COUNTER) {
    const long long n = step * (long long)std::max(c->prm.batch_size, 1) * c->prm.world_size;
    c->sampler.reset(new RefSampler(c->prm.mode, c->prm.width, c->prm.height, c->prm.num_objects));
    std::vector<ofdg_blueprint> bps;
    ofdg_task t;
    const int B = std::max(c->prm.batch_size, 1), world = c->prm.world_size, rank = c->prm.rank;
    const bool crops = c->prm.mode == 9 && c->crop_server.n_crops > 0;
    if (crops) { c->crop_server.head = 0; c->crop_server.counter = 0; }
    for (long long i = 0; i < n; ++i) {
      bps.clear();
      OFDG_TRY(c->sampler->next_task(&bps, &t, &c->err));
      if (crops && (i / B) % world == rank) {  // realize_batch serves one crop per deforming background / object
        if (bps[t.background].do_warpfield_deformation) (void)c->crop_server.get();
        for (int k = 0; k < t.n_objects; ++k)
          if (bps[t.first_object + k].do_warpfield_deformation) (void)c->crop_server.get();
      }
    }
  }
  // (the remaining parts of a group were sampled for the sequence the old counter was walking)
  if (step != c->step) for (int k = 0; k < c->n_chains; ++k) OFDG_TRY(discard_rest(c, c->chains[k]));
  c->step = step;
  return OFDG_OK;
}

// Batches of a chain that one sampler -> geom -> raster launch serves on the counter-sampler path: 1 (every call launches its
// own front end) .. kMaxFrontBatches (see forward_counter_impl).  A scheduling choice: the bytes are the same.
// ... and how many of them a call for n_samples samples gets: the largest N <= front with N x n_samples <= kPrepMaxSamples
// (OFDG_EINVAL: front is out of range).  No context, no device.
int ofdg_front_batches_for(int front, int n_samples) {
  if (front < 1 || front > kMaxFrontBatches) return OFDG_EINVAL;
  while (front > 1 && (long long)front * n_samples > kPrepMaxSamples) --front;
  return front;
}
// How many batches are sampled, outlined and rasterised and still wait for their calls, over all chains.
int ofdg_front_pending(const ofdg_ctx* c) {
  if (!c) return OFDG_EINVAL;
  int n = 0;
  for (int k = 0; k < c->n_chains; ++k)
    for (const ofdg_ctx::Chain::Prepared& p : c->chains[k].rest) n += p.valid ? 1 : 0;
  return n;
}
int ofdg_set_front_batches(ofdg_ctx* c, int n) {
  if (!c || ofdg_front_batches_for(n, 1) < 1) {
    if (c) c->err = "ofdg_set_front_batches: n = " + std::to_string(n) + " (valid: 1 .. " + std::to_string(kMaxFrontBatches) + ")";
    return OFDG_EINVAL;
  }
  for (int k = 0; k < c->n_chains; ++k) OFDG_TRY(discard_rest(c, c->chains[k]));
  c->front_batches = n;
  c->info = c->info_head + " front=" + std::to_string(n);
  return OFDG_OK;
}

int ofdg_synchronize(ofdg_ctx* c, void* stream) {
  if (!c) return OFDG_EINVAL;
  if (stream == OFDG_STREAM_OWN) stream = nullptr;  // (every internal stream is waited for below)
  HIP_OK(c, hipStreamSynchronize((hipStream_t)stream));
  for (int k = 0; k < c->n_chains; ++k) {
    HIP_OK(c, hipStreamSynchronize(c->chains[k].stream));
    if (c->chains[k].done_pending) HIP_OK(c, hipEventSynchronize(c->chains[k].ev_done));  // (a compose on another caller stream)
  }
  uint32_t words[ofdg_ctx::kErrWords];
  HIP_OK(c, hipMemcpy(words, c->d_err.p, sizeof(words), hipMemcpyDeviceToHost));
  uint32_t e = 0;
  long long first_bad = -1;
  for (int i = 0; i < ofdg_ctx::kErrWords; ++i)
    if (words[i]) {
      e |= words[i];
      // the most recent call that used this word
      const long long q = c->ticket - 1 - ((c->ticket - 1 - i) % ofdg_ctx::kErrWords + ofdg_ctx::kErrWords) % ofdg_ctx::kErrWords;
      if (first_bad < 0 || q < first_bad) first_bad = q;
    }
  if (e) HIP_OK(c, hipMemset(c->d_err.p, 0, sizeof(words)));
  if (c->word_reserved < 0) std::fill(c->word_clean, c->word_clean + ofdg_ctx::kErrWords, true);  // (nothing in flight, every word read)
  if (e) {
    c->err = err_text(e) + " (first in batch " + std::to_string(first_bad) + " of this context, or one " + std::to_string(ofdg_ctx::kErrWords) + " calls earlier)";
    return OFDG_ECAPACITY;
  }
  return OFDG_OK;
}

// The device-side error flags without waiting for anything in flight (a prefetch ring checks them when it hands
// a finished batch over; flags of younger batches are reported at their own hand-over at the latest).
static int poll_words(ofdg_ctx* c, int first, int n, uint32_t* flags) {
  if (!c->h_err.p) HIP_OK(c, c->h_err.alloc(sizeof(uint32_t), hipHostMallocMapped));
  if (!c->err_stream.s) HIP_OK(c, c->err_stream.create(hipStreamNonBlocking));
  // read AND clear in one atomic exchange per word (younger batches are still running and may raise a flag at any time: a
  // copy followed by a memset would lose what is raised in between)
  uint32_t* h_dev = nullptr;
  HIP_OK(c, hipHostGetDevicePointer((void**)&h_dev, c->h_err.p, 0));
  hipLaunchKernelGGL(err_exchange_kernel, dim3(1), dim3(64), 0, c->err_stream, c->d_err.p + first, n, h_dev);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipStreamSynchronize(c->err_stream));
  *flags = *(const uint32_t*)c->h_err.p;
  return OFDG_OK;
}
int ofdg_poll_errors(ofdg_ctx* c) {
  if (!c) return OFDG_EINVAL;
  uint32_t e = 0;
  OFDG_TRY(poll_words(c, 0, ofdg_ctx::kErrWords, &e));
  if (e) { c->err = err_text(e); return OFDG_ECAPACITY; }
  return OFDG_OK;
}

// The flags of ONE batch (ticket = ofdg_last_ticket() right after the call that rendered it), without waiting for anything:
// what a prefetch ring asks when it hands that batch over, having waited for the batch's own completion event.  The word
// is cleared.  Tickets older than kErrWords calls are gone (OFDG_EINVAL).
long long ofdg_last_ticket(const ofdg_ctx* c) { return c ? c->last_ticket : -1; }
int ofdg_poll_errors_of(ofdg_ctx* c, long long ticket) {
  if (!c) return OFDG_EINVAL;
  if (ticket < 0 || ticket >= c->ticket || ticket + ofdg_ctx::kErrWords <= c->ticket) { c->err = "ofdg_poll_errors_of: no such batch (tickets of the last " + std::to_string(ofdg_ctx::kErrWords) + " calls are kept)"; return OFDG_EINVAL; }
  uint32_t e = 0;
  c->asked_by_ticket = true;
  OFDG_TRY(poll_words(c, (int)(ticket % ofdg_ctx::kErrWords), 1, &e));
  c->word_clean[(size_t)(ticket % ofdg_ctx::kErrWords)] = true;  // (read and cleared; the caller waited for this batch before asking)
  if (e) { c->err = "batch " + std::to_string(ticket) + ": " + err_text(e); return OFDG_ECAPACITY; }
  return OFDG_OK;
}

// ---- mode 9 warp fields -----------------------------------------------------------------------------
static int warp_alloc(ofdg_ctx* c, int n_crops) {
  const size_t crop_floats = (size_t)4 * (c->prm.width + 1) * (c->prm.height + 1);
  HIP_OK(c, hipDeviceSynchronize());
  drop_counter_croptab(c);
  HIP_OK(c, c->d_warp.alloc((size_t)n_crops * crop_floats));
  HIP_OK(c, c->d_warp_max.alloc((size_t)n_crops));
  HIP_OK(c, hipMemset(c->d_warp_max.p, 0, (size_t)n_crops * sizeof(unsigned)));
  c->crop_server = CropServer();
  c->crop_server.n_crops = n_crops;
  return OFDG_OK;
}

// Replaces WarpFields::CropGenerator (WF:469-641): n_fields big fields of side 3*max(W,H)
// are generated on the device from seeded displacer lists (seed, seed+1, ...), composed
// 17 times with themselves (x 2^17), cleaned, and cut into (W+1) x (H+1) crops.
int ofdg_warp_generate(ofdg_ctx* c, int n_fields, uint32_t seed) {
  if (!c || n_fields < 1) return OFDG_EINVAL;
  OFDG_TRY(discard_all_prepared(c));  // (batches prepared ahead read the old pool / crops)
  const int W = c->prm.width, H = c->prm.height;
  const int S = std::max(W, H) * 3;
  std::vector<std::pair<int, int>> org;  // crop grid (WF:617-633)
  for (int y = H / 4; y < S - 5 * H / 4; y += H / 3)
    for (int x = W / 4; x < S - 5 * W / 4; x += W / 3) org.push_back({x, y});
  if (org.empty()) { c->err = "frame too small for warp crops"; return OFDG_EINVAL; }
  OFDG_TRY(warp_alloc(c, n_fields * (int)org.size()));
  const size_t n = (size_t)S * S;
  DevBuf<float> fa, fb;
  DevBuf<uint8_t> flagged;
  DevBuf<DevDisplacer> dd;
  HIP_OK(c, fa.alloc(4 * n));
  HIP_OK(c, fb.alloc(4 * n));
  HIP_OK(c, flagged.alloc(2 * n));
  const int cw = W + 1, ch = H + 1;
  const size_t crop_floats = (size_t)4 * cw * ch;
  const int blocks = (int)((n + 255) / 256);
  for (int f = 0; f < n_fields; ++f) {
    std::vector<DevDisplacer> disp = make_device_displacers(make_displacer_params(W, H, seed + (uint32_t)f));
    HIP_OK(c, dd.alloc(std::max<size_t>(1, disp.size())));
    HIP_OK(c, hipMemcpy(dd.p, disp.data(), disp.size() * sizeof(DevDisplacer), hipMemcpyHostToDevice));
    HIP_OK(c, hipMemset(flagged.p, 0, 2 * n));
    hipLaunchKernelGGL(wf_sample_kernel, dim3(blocks), dim3(256), 0, 0, dd.p, (int)disp.size(), S, fa.p);
    float *from = fa.p, *to = fb.p;
    for (int iter = 17; iter > 0; --iter) {  // WF:366, 406
      hipLaunchKernelGGL(wf_compose_kernel, dim3(blocks, 2), dim3(256), 0, 0, from, to, S, flagged.p);
      std::swap(from, to);
    }
    hipLaunchKernelGGL(wf_finish_kernel, dim3(blocks, 2), dim3(256), 0, 0, from, S, flagged.p);
    for (size_t k = 0; k < org.size(); ++k) {
      const size_t ci = (size_t)f * org.size() + k;
      hipLaunchKernelGGL(wf_crop_kernel, dim3((cw * ch + 255) / 256), dim3(256), 0, 0, from, S, org[k].first, org[k].second, cw, ch,
                         c->d_warp.p + ci * crop_floats, c->d_warp_max.p + ci);
    }
    HIP_OK(c, hipGetLastError());
    HIP_OK(c, hipDeviceSynchronize());  // (the field's temporaries are idle from here: `dd` is replaced, the others go with the scope)
  }
  return OFDG_OK;
}

// Install caller-provided crops: n x 4 planes (flow x, flow y, iflow x, iflow y) of (H+1)*(W+1) floats.
int ofdg_warp_upload(ofdg_ctx* c, const float* crops, int n) {
  if (!c || !crops || n < 1) return OFDG_EINVAL;
  OFDG_TRY(discard_all_prepared(c));  // (batches prepared ahead read the old pool / crops)
  OFDG_TRY(warp_alloc(c, n));
  const size_t plane = (size_t)(c->prm.width + 1) * (c->prm.height + 1), crop_floats = 4 * plane;
  {  // the kernels read a crop as two planes of interleaved pairs: (flow x, flow y), (iflow x, iflow y)
    std::vector<float> il((size_t)n * crop_floats);
    for (int k = 0; k < n; ++k)
      for (int f = 0; f < 4; ++f) {
        const float* src = crops + (size_t)k * crop_floats + (size_t)f * plane;
        float* dst = il.data() + (size_t)k * crop_floats + (size_t)(f >> 1) * 2 * plane + (f & 1);
        for (size_t i = 0; i < plane; ++i) dst[2 * i] = src[i];
      }
    HIP_OK(c, hipMemcpy(c->d_warp.p, il.data(), il.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  std::vector<unsigned> mx(n, 0u);
  for (int k = 0; k < n; ++k) {
    float m = 0.f;
    const float* p = crops + (size_t)k * crop_floats + 2 * plane;
    for (size_t i = 0; i < 2 * plane; ++i) if (p[i] == p[i]) m = std::max(m, std::fabs(p[i]));
    std::memcpy(&mx[k], &m, sizeof(float));
  }
  HIP_OK(c, hipMemcpy(c->d_warp_max.p, mx.data(), (size_t)n * sizeof(unsigned), hipMemcpyHostToDevice));
  return OFDG_OK;
}

int ofdg_warp_info(const ofdg_ctx* c, int* n_crops, int* w, int* h) {
  if (!c) return OFDG_EINVAL;
  if (n_crops) *n_crops = c->crop_server.n_crops;
  if (w) *w = c->prm.width + 1;
  if (h) *h = c->prm.height + 1;
  return OFDG_OK;
}

int ofdg_warp_download(ofdg_ctx* c, int index, float* crop) {
  if (!c || !crop || index < 0 || index >= c->crop_server.n_crops) return OFDG_EINVAL;
  const size_t crop_floats = (size_t)4 * (c->prm.width + 1) * (c->prm.height + 1);
  HIP_OK(c, hipDeviceSynchronize());
  std::vector<float> il(crop_floats);
  HIP_OK(c, hipMemcpy(il.data(), c->d_warp.p + (size_t)index * crop_floats, crop_floats * sizeof(float), hipMemcpyDeviceToHost));
  const size_t plane = crop_floats / 4;  // (device layout: interleaved pairs; the API's: four planes)
  for (int f = 0; f < 4; ++f) {
    const float* src = il.data() + (size_t)(f >> 1) * 2 * plane + (f & 1);
    for (size_t i = 0; i < plane; ++i) crop[(size_t)f * plane + i] = src[2 * i];
  }
  return OFDG_OK;
}

// Displacer draws of one big field (host only): n x 9 doubles {type, p0, p1, p2, support cx, cy, sx, sy, angle}.
int ofdg_host_displacers(int width, int height, uint32_t seed, double* out, int cap) {
  std::vector<DisplacerParams> d = make_displacer_params(width, height, seed);
  if ((int)d.size() > cap || !out) return -(int)d.size();
  std::memcpy(out, d.data(), d.size() * sizeof(DisplacerParams));
  return (int)d.size();
}

// ---- inspection ---------------------------------------------------------------------------------
static inline int iround_h(double v) { return int((v < 0.0) ? v - 0.5 : v + 0.5); }

// rasterise ONE outline given as 24.8 vertices over the whole frame (slot 0 serves as scratch)
static int debug_rasterize_verts(ofdg_ctx* c, const std::vector<int2>& v, int n, uint8_t* coverage_host) {
  const int W = c->prm.width, H = c->prm.height;
  int minx = 0x7fffffff, miny = 0x7fffffff, maxx = -0x7fffffff - 1, maxy = -0x7fffffff - 1;
  for (int i = 0; i < n; ++i) {
    minx = std::min(minx, v[i].x); maxx = std::max(maxx, v[i].x);
    miny = std::min(miny, v[i].y); maxy = std::max(maxy, v[i].y);
  }
  DevShapeFrame f = DevShapeFrame();
  f.n_verts = n;
  int x0 = minx >> 8, y0 = miny >> 8, x1 = maxx >> 8, y1 = maxy >> 8;
  if (n < 2 || x1 < 0 || y1 < 0 || x0 > W - 1 || y0 > H - 1) { x0 = 1; x1 = 0; y0 = 1; y1 = 0; }
  else { x0 = std::max(x0, 0); y0 = std::max(y0, 0); x1 = std::min(x1, W - 1); y1 = std::min(y1, H - 1); }
  f.x0 = x0; f.y0 = y0; f.x1 = x1; f.y1 = y1;
  HIP_OK(c, hipDeviceSynchronize());
  ofdg_ctx::Slot& sl = c->slots[0];
  HIP_OK(c, sl.d_frames.reserve(2));
  HIP_OK(c, sl.d_verts.reserve(2 * kMaxVerts));
  HIP_OK(c, c->chains[0].cov.reserve((size_t)2 * W * H + 16));
  HIP_OK(c, hipMemcpy(sl.d_frames.p, &f, sizeof(f), hipMemcpyHostToDevice));
  HIP_OK(c, hipMemcpy(sl.d_verts.p, v.data(), sizeof(int2) * kMaxVerts, hipMemcpyHostToDevice));
  HIP_OK(c, hipMemset(c->chains[0].cov.p, 0xAB, (size_t)W * H));  // poison: every byte must be written
  const int bands = (H + kBandRows - 1) / kBandRows;
  std::vector<int4> items;
  for (int b = 0; b < bands; ++b)
    for (int cx = 0; cx < W; cx += kChunkW) items.push_back(make_int4(0, b, cx, std::min(cx + kChunkW - 1, W - 1)));
  const int n_items = (int)items.size();
  HIP_OK(c, sl.d_items.reserve(items.size()));
  OFDG_TRY(ensure_item_count(c, sl));
  HIP_OK(c, hipMemcpy(sl.d_items.p, items.data(), sizeof(int4) * items.size(), hipMemcpyHostToDevice));
  HIP_OK(c, hipMemcpy(sl.d_item_count.p, &n_items, sizeof(int), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(raster_kernel, dim3(64 * 4 / kRasterWaves), dim3(64 * kRasterWaves), 0, 0, sl.d_frames.p, sl.d_items.p, sl.d_item_count.p, sl.d_verts.p,
                     W, H, c->chains[0].cov.p, nullptr, 0, (unsigned long long*)nullptr);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipMemcpy(coverage_host, c->chains[0].cov.p, (size_t)W * H, hipMemcpyDeviceToHost));
  HIP_OK(c, hipMemset(sl.d_item_count.p, 0, sizeof(int)));
  sl.res_samples = 0;  // (slot 0 served as scratch)
  c->last_slot = nullptr;
  return OFDG_OK;
}

int ofdg_debug_rasterize(ofdg_ctx* c, const double* xy, int n, uint8_t* coverage_host) {
  if (!c || !xy || !coverage_host || n < 1 || n > kMaxVerts) return OFDG_EINVAL;
  OFDG_TRY(discard_all_prepared(c));
  std::vector<int2> v(kMaxVerts);
  for (int i = 0; i < n; ++i) v[i] = make_int2(iround_h(xy[2 * i] * 256.0), iround_h(xy[2 * i + 1] * 256.0));
  return debug_rasterize_verts(c, v, n, coverage_host);
}

// A path with curve3 segments (types: 1 line_to, 3 curve3 control point followed by its end point; entry 0 is the
// move_to vertex) through the DEVICE's flattening (path_verts / flatten_curve3, what geom_kernel runs) and rasteriser.
int ofdg_debug_rasterize_path(ofdg_ctx* c, const double* xy, const int* types, int n, uint8_t* coverage_host) {
  if (!c || !xy || !types || !coverage_host || n < 1 || n > 64) return OFDG_EINVAL;
  OFDG_TRY(discard_all_prepared(c));
  HIP_OK(c, hipDeviceSynchronize());
  DevBuf<double> d_xy;
  DevBuf<int> d_ty, d_n;
  DevBuf<int2> d_v;
  HIP_OK(c, d_xy.alloc(2 * (size_t)n));
  HIP_OK(c, d_ty.alloc(n));
  HIP_OK(c, d_v.alloc(kMaxVerts));
  HIP_OK(c, d_n.alloc(1));
  HIP_OK(c, hipMemcpy(d_xy.p, xy, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
  HIP_OK(c, hipMemcpy(d_ty.p, types, sizeof(int) * n, hipMemcpyHostToDevice));
  HIP_OK(c, hipMemset(d_v.p, 0, sizeof(int2) * kMaxVerts));
  uint32_t* const dbg_err = c->d_err.p + ofdg_ctx::kErrWords;  // (the debug entry points' own word: no batch inherits it)
  hipLaunchKernelGGL(debug_path_kernel, dim3(1), dim3(64), 0, 0, d_xy.p, d_ty.p, n, d_v.p, d_n.p, dbg_err);
  HIP_OK(c, hipGetLastError());
  uint32_t dbg_flags = 0;
  HIP_OK(c, hipMemcpy(&dbg_flags, dbg_err, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (dbg_flags) HIP_OK(c, hipMemset(dbg_err, 0, sizeof(uint32_t)));
  std::vector<int2> v(kMaxVerts);
  int nv = 0;
  HIP_OK(c, hipMemcpy(v.data(), d_v.p, sizeof(int2) * kMaxVerts, hipMemcpyDeviceToHost));
  HIP_OK(c, hipMemcpy(&nv, d_n.p, sizeof(int), hipMemcpyDeviceToHost));
  if (dbg_flags) { c->err = "debug_rasterize_path: " + err_text(dbg_flags); return OFDG_ECAPACITY; }
  if (nv < 1 || nv > kMaxVerts) { c->err = "debug_rasterize_path: the flattened outline has " + std::to_string(nv) + " vertices"; return OFDG_ECAPACITY; }
  return debug_rasterize_verts(c, v, nv, coverage_host);
}

// The DEVICE's span interpolator (make_row + dda_at, what the texture warps run): (x, y) in 24.8 fixed point of every
// pixel of `rows` output rows of length `len` under the inverse affine inv[6] (AGG member order), before the -128.
int ofdg_debug_dda_rows(ofdg_ctx* c, const double* inv, int rows, int len, int* out_xy) {
  if (!c || !inv || !out_xy || rows < 1 || len < 1 || (size_t)rows * len > (1u << 24)) return OFDG_EINVAL;
  DevBuf<int2> d;
  HIP_OK(c, d.alloc((size_t)rows * len));
  const Mat m{inv[0], inv[1], inv[2], inv[3], inv[4], inv[5]};
  hipLaunchKernelGGL(debug_dda_kernel, dim3((rows * len + 255) / 256), dim3(256), 0, 0, m, rows, len, d.p);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipMemcpy(out_xy, d.p, sizeof(int2) * (size_t)rows * len, hipMemcpyDeviceToHost));
  return OFDG_OK;
}

int ofdg_debug_num_shapes(ofdg_ctx* c, int sample) {
  if (!c || !c->last_slot) return OFDG_EINVAL;
  const ofdg_ctx::Slot& sl = *c->last_slot;
  if (sl.res_samples <= 0 || sample < 0 || sample >= (int)sl.batch.samples.size()) return OFDG_EINVAL;
  return sl.batch.samples[sample].n_shapes;
}

int ofdg_debug_coverage(ofdg_ctx* c, int sample, int shape, int frame, uint8_t* coverage_host) {
  if (!c || !coverage_host || frame < 0 || frame > 1 || !c->last_slot || c->last_slot->res_samples <= 0) return OFDG_EINVAL;
  const ofdg_ctx::Slot& sl = *c->last_slot;
  if (sample < 0 || sample >= (int)sl.batch.samples.size()) return OFDG_EINVAL;
  const DevSample& s = sl.batch.samples[sample];
  if (shape < 0 || shape >= s.n_shapes) return OFDG_EINVAL;
  const int W = c->prm.width, H = c->prm.height;
  const size_t sf = (size_t)(s.first_shape + shape) * 2 + frame;
  HIP_OK(c, hipDeviceSynchronize());
  DevShapeFrame f;
  HIP_OK(c, hipMemcpy(&f, sl.d_frames.p + sf, sizeof(f), hipMemcpyDeviceToHost));
  std::vector<uint8_t> tmp((size_t)W * H);
  HIP_OK(c, hipMemcpy(tmp.data(), c->chains[c->last_chain].cov.p + sf * W * H, tmp.size(), hipMemcpyDeviceToHost));
  std::memset(coverage_host, 0, tmp.size());
  for (int y = f.y0; y <= f.y1; ++y)
    for (int x = f.x0; x <= f.x1; ++x) coverage_host[(size_t)y * W + x] = tmp[(size_t)y * W + x];
  return OFDG_OK;
}

// number of raster work items left by the last launch (diagnostics)
int ofdg_debug_item_count(ofdg_ctx* c) {
  if (!c || !c->last_slot || !c->last_slot->d_item_count.p) return OFDG_EINVAL;
  int n = 0;
  if (hipDeviceSynchronize() != hipSuccess) return OFDG_EHIP;
  if (hipMemcpy(&n, c->last_slot->d_item_count.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return OFDG_EHIP;
  return n;
}

// How bgprep_stream_kernel walked the last batch: the number of its tiles (only known on the device: a sample's read region
// depends on its background motion) and of the workgroups that shared them grid-stride - a test that means to compare the
// SECOND, third ... tile of a workgroup with the oracle asserts tiles > k * workgroups.  0 tiles: the batch took another form
// of the preparation (background_prep != 1, pool images smaller than 2W x 2H, more samples than the one-launch form numbers).
int ofdg_debug_bgprep_tiles(ofdg_ctx* c, int* tiles, int* workgroups) {
  if (!c || !tiles || !workgroups || !c->last_slot) return OFDG_EINVAL;
  const ofdg_ctx::Slot& sl = *c->last_slot;
  *tiles = 0; *workgroups = kPrepGrid;
  int cap_cw, cap_ch;
  bool fusable;
  bgprep_caps(c, &cap_cw, &cap_ch, &fusable);
  const int n = c->last_n;  // (the batch the last call composed: a slot may hold several)
  if (c->prm.background_prep != 1 || !fusable || n > kPrepMaxSamples || n < 1 || !sl.d_bgprep.p) return OFDG_OK;
  HIP_OK(c, hipDeviceSynchronize());
  std::vector<DevBgPrep> rec((size_t)n);
  HIP_OK(c, hipMemcpy(rec.data(), sl.d_bgprep.p + c->last_base, rec.size() * sizeof(DevBgPrep), hipMemcpyDeviceToHost));
  for (const DevBgPrep& q : rec)
    if (prep_sample_fits(q, cap_cw, cap_ch)) *tiles += prep_tile_cols(q) * prep_tile_rows(q);
  return OFDG_OK;
}

// Which forms of bgprep_stream_kernel rendered the tiles since the last call (the first call switches the counting on and returns
// zeros): counts[rotation + 3 * resize], see the kernel.  A guard for the tests: parity cannot tell a batch whose tiles all fell
// back to the general forms from one that took the fast ones.
int ofdg_debug_bgprep_paths(ofdg_ctx* c, unsigned* counts9) {
  if (!c || !counts9) return OFDG_EINVAL;
  HIP_OK(c, hipDeviceSynchronize());
  if (!c->d_prep_paths.p) {
    HIP_OK(c, c->d_prep_paths.alloc(9));
    HIP_OK(c, hipMemset(c->d_prep_paths.p, 0, 9 * sizeof(uint32_t)));
  }
  HIP_OK(c, hipMemcpy(counts9, c->d_prep_paths.p, 9 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_OK(c, hipMemset(c->d_prep_paths.p, 0, 9 * sizeof(uint32_t)));
  return OFDG_OK;
}

int ofdg_set_profiling(ofdg_ctx* c, int mode) {
  if (!c || mode < 0 || mode > 2) return OFDG_EINVAL;
  HIP_OK(c, hipDeviceSynchronize());
  OFDG_TRY(discard_all_prepared(c));
  HIP_OK(c, hipDeviceSynchronize());
  c->profiling = mode;
  c->ev_count = 0; c->ev_alloc = 0;
  c->launch_count = 0;
  c->ev_stride = (mode == 1) ? 4 : 1;  // mode 1 samples every 4th launch (no marker packets: two completion signals per sampled launch)
  if (mode && c->ev.empty()) {
    c->ev_sets = 256;
    c->ev.resize((size_t)c->ev_sets * 6);
    for (auto& e : c->ev) HIP_OK(c, e.create(hipEventDefault));
  }
  c->ev_composed.assign((size_t)c->ev_sets, 0);
  c->ev_bgprep.assign((size_t)c->ev_sets, 0);
  c->ev_front.assign((size_t)c->ev_sets, 0);
  return OFDG_OK;
}

// Average device time (ms) per launch of one kernel over the launches recorded since
// ofdg_set_profiling (at most the last 256), from HIP events attached to the kernels' dispatch
// packets on their launch streams: completion of the predecessor .. completion of the kernel.
int ofdg_kernel_ms(ofdg_ctx* c, const char* kernel, float* ms) {
  if (!c || !kernel || !ms) return OFDG_EINVAL;
  int i = -1;
  if (!std::strcmp(kernel, "geom")) i = 0;
  else if (!std::strcmp(kernel, "raster")) i = 1;
  else if (!std::strcmp(kernel, "compose")) i = 2;
  else if (!std::strcmp(kernel, "background_prep")) i = 3;  // (timed where it runs behind raster: not for a caller's slot prepared at its upload)
  if (i < 0) { c->err = "unknown kernel name"; return OFDG_EINVAL; }
  if (!c->profiling || c->ev_count == 0 || (i < 2 && c->profiling != 2)) {
    c->err = "no profiled launch of that kernel yet (ofdg_set_profiling)";
    return OFDG_EINVAL;
  }
  int n = 0;
  double acc = 0;
  for (int k = 0; k < c->ev_sets; ++k) {
    if (!c->ev_composed[(size_t)k]) continue;  // (never handed out, or its prepared batch was discarded before compose)
    if (i == 3 && !c->ev_bgprep[(size_t)k]) continue;
    if (i < 2 && !c->ev_front[(size_t)k]) continue;  // (served from a later part of a group: no geom / raster launch, its ev[0 .. 3] are stale)
    ++n;
    const Event* ev = &c->ev[(size_t)k * 6];
    HIP_OK(c, hipEventSynchronize(ev[5]));
    float t = 0;
    if (i == 3) {  // completion of raster .. completion of the (last) preparation kernel
      HIP_OK(c, hipEventElapsedTime(&t, ev[3], ev[c->profiling == 2 ? 2 : 4]));
      acc += t;
      continue;
    }
    // geom: its own start .. its end; raster: end of geom .. its end; compose: its own start (profiling 2) or the end of the
    // last preparation kernel (profiling 1) .. its end
    HIP_OK(c, hipEventElapsedTime(&t, ev[i == 0 ? 0 : (i == 2 ? 4 : 1)], ev[2 * i + 1]));
    acc += t;
  }
  if (n == 0) { c->err = "no profiled launch of that kernel yet (ofdg_set_profiling)"; return OFDG_EINVAL; }
  *ms = (float)(acc / n);
  return OFDG_OK;
}

// Exhaustive device tables of the per-byte formulas (tests): add/sub [256*256],
// aa [256], blend(d, s_fixed, m) [256*256] indexed d*256+m.
int ofdg_debug_tables(ofdg_ctx* c, uint8_t* add_tbl, uint8_t* sub_tbl, uint8_t* aa_tbl, uint8_t* blend_tbl, int s_fixed) {
  if (!c) return OFDG_EINVAL;
  DevBuf<uint8_t> buf;
  HIP_OK(c, buf.alloc(3 * 65536 + 256));
  uint8_t* const d = buf.p;
  hipLaunchKernelGGL(tables_kernel, dim3(256), dim3(256), 0, 0, d, d + 65536, d + 3 * 65536, d + 2 * 65536, s_fixed);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipMemcpy(add_tbl, d, 65536, hipMemcpyDeviceToHost));
  HIP_OK(c, hipMemcpy(sub_tbl, d + 65536, 65536, hipMemcpyDeviceToHost));
  HIP_OK(c, hipMemcpy(blend_tbl, d + 2 * 65536, 65536, hipMemcpyDeviceToHost));
  HIP_OK(c, hipMemcpy(aa_tbl, d + 3 * 65536, 256, hipMemcpyDeviceToHost));
  return OFDG_OK;
}

// include/ofdg_detmath.h on the device: n angles -> sin, cos; m floats -> expf (host arrays)
int ofdg_debug_detmath(ofdg_ctx* c, const double* angles, int n, double* sin_out, double* cos_out, const float* x, int m, float* expf_out) {
  if (!c || n < 0 || m < 0 || (n > 0 && (!angles || !sin_out || !cos_out)) || (m > 0 && (!x || !expf_out))) return OFDG_EINVAL;
  DevBuf<double> dbuf;
  DevBuf<float> fbuf;
  const int k = std::max(std::max(n, m), 1);
  HIP_OK(c, dbuf.alloc((size_t)3 * k));
  HIP_OK(c, fbuf.alloc((size_t)2 * k));
  double* const d = dbuf.p;
  float* const f = fbuf.p;
  if (n) HIP_OK(c, hipMemcpy(d, angles, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  if (m) HIP_OK(c, hipMemcpy(f, x, (size_t)m * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(detmath_kernel, dim3((k + 255) / 256), dim3(256), 0, 0, d, n, d + k, d + 2 * k, f, m, f + k);
  HIP_OK(c, hipGetLastError());
  if (n) {
    HIP_OK(c, hipMemcpy(sin_out, d + k, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(c, hipMemcpy(cos_out, d + 2 * k, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (m) HIP_OK(c, hipMemcpy(expf_out, f + k, (size_t)m * sizeof(float), hipMemcpyDeviceToHost));
  return OFDG_OK;
}

int ofdg_debug_photo_table(ofdg_ctx* c, const ofdg_photo_rec* rec_host, float* table_host) {
  if (!c) return OFDG_EINVAL;
  if (!rec_host || !table_host) { c->err = "ofdg_debug_photo_table: rec_host or table_host is NULL"; return OFDG_EINVAL; }
  DevBuf<DevPhotoRec> rec;
  DevBuf<float> table;
  HIP_OK(c, rec.alloc(1));
  HIP_OK(c, table.alloc((size_t)2 * 3 * 256));
  HIP_OK(c, hipMemcpy(rec.p, rec_host, sizeof(DevPhotoRec), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(photo_table_kernel, dim3(6), dim3(256), 0, 0, rec.p, table.p);
  HIP_OK(c, hipGetLastError());
  HIP_OK(c, hipMemcpy(table_host, table.p, (size_t)2 * 3 * 256 * sizeof(float), hipMemcpyDeviceToHost));
  return OFDG_OK;
}

}  // extern "C"
