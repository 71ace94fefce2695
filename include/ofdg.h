/*
 * ofdg.h -- C-ABI of the MI355X-native optical-flow data generator.
 *
 * This is the drop-in boundary for the reference's per-sample hot path
 * (blueprint -> masks -> warped textures -> composited image0/image1 + flow).
 * Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Every entry point names the reference interface it replaces.  Citations are
 * relative to the reference repository root
 * (lmb-freiburg/optical-flow-2d-data-generation):
 *   DG  = src/caffe/DataGenerator.cpp
 *   DGH = include/caffe/data_generation/DataGenerator.h
 *   LAY = src/caffe/layers/data_generation_layer.cpp
 *   WF  = src/caffe/WarpFields.cpp
 */
#ifndef OFDG_H_
#define OFDG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* Error codes (reference: std::runtime_error / glog CHECK, DG:121,    */
/* DG:1143, DG:2004; silently dropped "bad" samples DG:1285-1292).     */
/* ------------------------------------------------------------------ */
#define OFDG_OK          0
#define OFDG_EBADMODE   (-1) /* "BAD MODE"                      DG:2004  */
#define OFDG_ETEXTURES  (-2) /* "Could not open texture ..."    DG:121   */
#define OFDG_EOBJTYPE   (-3) /* "Bad object type ..."           DG:1143  */
#define OFDG_EHIP       (-4) /* HIP runtime failure / extension missing  */
#define OFDG_ECAPACITY  (-5) /* fixed-capacity array exceeded            */
#define OFDG_EINVAL     (-6) /* invalid argument                         */
#define OFDG_ESTARTUP   (-7) /* multi-GPU start-up: another rank failed  */

/* ObjType_t (DGH:369-374) and PolySegmentType_t (DGH:377-381) values. */
#define OFDG_OBJ_DUMMY     0
#define OFDG_OBJ_ELLIPSE   1
#define OFDG_OBJ_POLYGON   2
#define OFDG_OBJ_COMPOSITE 3
#define OFDG_SEG_DUMMY     0
#define OFDG_SEG_LINE      1
#define OFDG_SEG_CURVE3    3

#define OFDG_MAX_SEGMENTS    20 /* RNG_PolyObj_spokes in [3,20]   DG:1687 */
#define OFDG_MAX_COMPONENTS   8 /* RNG_CompObiNumberOfComponents <= 7     */
#define OFDG_BACKGROUND_ID    1 /* BACKGROUND_OBJ_ID              DGH:60  */

/* sampler kinds */
#define OFDG_SAMPLER_REF      0 /* bit-identical 45-stream mt19937 sampler */
#define OFDG_SAMPLER_COUNTER  1 /* device counter-based sampler            */

/*
 * POD mirror of DataGenerator::ObjectBlueprint (DGH:388-421).  Children of a
 * composite live in the same flat array (first_component, n_components)
 * instead of owning heap pointers (DG:934-940).
 */
typedef struct ofdg_blueprint {
  int32_t obj_id;       /* top-level foreground blueprints of one task: distinct and > OFDG_BACKGROUND_ID, in any order (they are
                           rendered in ascending obj_id); a repeated id is refused with OFDG_EINVAL */
  int32_t obj_type;
  float   init_rot, init_scale, init_trans_x, init_trans_y;
  float   rot, scale, trans_x, trans_y;
  int32_t tex_id;
  float   tex_rot, tex_scale;
  int32_t tex_shift_x, tex_shift_y;
  float   ellipse_scale_x, ellipse_scale_y;
  int32_t n_segments;
  int32_t segment_type[OFDG_MAX_SEGMENTS];
  float   segment_x[OFDG_MAX_SEGMENTS];
  float   segment_y[OFDG_MAX_SEGMENTS];
  int32_t first_component;
  int32_t n_components;
  int32_t is_additive_component;
  int32_t do_warpfield_deformation;
} ofdg_blueprint;

/*
 * POD mirror of DataGenerator::TaskBucket (DGH:423-437): one sample = one
 * background blueprint + n_objects top-level foreground blueprints, which are
 * contiguous in the flat blueprint array.
 */
typedef struct ofdg_task {
  int32_t background;   /* index of the background blueprint */
  int32_t first_object; /* index of the first top-level foreground blueprint */
  int32_t n_objects;
  int32_t reserved;
} ofdg_task;

/*
 * Options: data_param{batch_size,prefetch} + data_generation_param{mode,
 * first_level_threads, second_level_threads, use_antialiasing}
 * (src/caffe/proto/caffe.proto:6-12, example-prototxt/train.prototxt:9-30)
 * plus extension keys (width/height are #defines in the reference, DGH:55-56).
 */
typedef struct ofdg_params {
  int32_t width;                /* DGEN_WIDTH  (512) */
  int32_t height;               /* DGEN_HEIGHT (384) */
  int32_t mode;                 /* 1..13 */
  int32_t use_antialiasing;     /* default 1 */
  int32_t batch_size;
  int32_t prefetch;
  int32_t first_level_threads;  /* accepted; only used by CPU paths */
  int32_t second_level_threads; /* accepted; only used by CPU paths */
  int32_t num_objects;          /* 0 = reference behaviour (16..23, DG:1666) */
  int32_t sampler;              /* OFDG_SAMPLER_* */
  int32_t seed;                 /* counter sampler seed; ref sampler uses 0..44 */
  int32_t rank, world_size;     /* sample sharding (g = step*B*world + rank*B + i) */
  int32_t device;               /* HIP device ordinal */
  int32_t max_shapes_per_sample;/* 0 = default capacity */
  int32_t background_prep;      /* background texture m_textures[0] (DG:1186-1192):
                                   0 = centre 2W x 2H crop of the pool image (the C-ABI default; parity boundary of round 1);
                                   1 = Texture::getRandomizedCrop(2W, 2H, tex_rot, tex_scale, tex_shift) (DG:87-109) the way
                                       CImg runs it: get_shift -> rotate (linear, mirror, grown canvas) -> u8 -> crop (float ->
                                       int truncation, mirror) -> resize (per axis linear / moving average, u8 in between);
                                   2 = the same geometry as ONE resampling along the composed coordinate map (fast form:
                                       one interpolation less of blur, values differ from 1).  CImg itself: parity unpinned */
  /* how the context schedules its work (no effect on the bytes it renders; tests/test_gpu_sampler.py):
   *   chains     internal in-order streams, each [sampler ->] geom -> raster -> compose of one batch (1..8).  0 = automatic:
   *              4 when the process was started with GPU_MAX_HW_QUEUES >= 8 (one hardware queue per chain), else 3;
   *              ofdg_ctx_info() says which and why
   *   lookahead  counter sampler: batches whose preparation kernels are enqueued ahead of the call that composes them
   *              (the reference's prefetch thread, LAY:141-172); 0 = none
   *   serial     1 = everything on the caller's stream, one kernel after the other (debugging, per-kernel timing) */
  int32_t chains, lookahead, serial;
  int32_t reserved[5];
} ofdg_params;

typedef struct ofdg_ctx ofdg_ctx;

/* Fill *p with the reference's defaults (caffe.proto:6-12, DGH:55-56). */
void ofdg_default_params(ofdg_params* p);

/*
 * Replaces DataGenerationLayer ctor + LayerSetUp (LAY:36-56, 106-132):
 * DataGenerator(param) + ObjectParametersGenerator(param) (DG:990-998,
 * DG:1358-2054).  Fails with OFDG_EHIP if no HIP device / kernel image.
 */
int ofdg_create(const ofdg_params* params, ofdg_ctx** out);
void ofdg_destroy(ofdg_ctx* ctx);
/* The parameters the ctx was created with. */
const ofdg_params* ofdg_ctx_params(const ofdg_ctx* ctx);
/* Message of the last failure on this ctx (or of a failed ofdg_create if ctx==NULL). */
const char* ofdg_last_error(const ofdg_ctx* ctx);
/* One line on how the context is set up: number of chains and what decided it (GPU_MAX_HW_QUEUES as the library found it
 * when it was loaded; HIP reads the variable when the runtime starts, so it must be in the environment of the process),
 * look-ahead, serial mode.  Valid until the ctx is destroyed. */
const char* ofdg_ctx_info(const ofdg_ctx* ctx);

/* ---- texture pool: replaces TextureCollection (DG:117-161) ---------------- */
/* n seeded synthetic w x h textures generated directly in HBM. */
int ofdg_pool_synthetic(ofdg_ctx* ctx, int n, int w, int h, uint32_t seed);
/* Reserve an empty pool of n textures of w x h, to be filled by ofdg_pool_upload. */
int ofdg_pool_alloc(ofdg_ctx* ctx, int n, int w, int h);
/* Upload one texture: planar B,G,R u8 (CImg layout after the swap at DG:129-131). */
int ofdg_pool_upload(ofdg_ctx* ctx, int index, const uint8_t* bgr_planar, int w, int h);
/* A pool of n images of DIFFERENT sizes (real texture lists, TextureCollection DG:117-149): every image is
 * reduced at upload to what the path reads - its W x H foreground texture and its 2W x 2H background texture
 * (centre crop, or the CImg-resized whole image if it is smaller, DG:96-106); with background_prep the whole
 * image stays resident as well (the preparation works on the original image). */
int ofdg_pool_alloc_mixed(ofdg_ctx* ctx, int n);
int ofdg_pool_upload_mixed(ofdg_ctx* ctx, int index, const uint8_t* bgr_planar, int w, int h);
/* Download texture `index` as planar B,G,R u8 (w*h*3 bytes). */
int ofdg_pool_download(ofdg_ctx* ctx, int index, uint8_t* bgr_planar);
int ofdg_pool_info(const ofdg_ctx* ctx, int* n, int* w, int* h);
/* The resident pool (one image size) as raw device memory, n*h*w BGRX texels: lets rank 0 load the texture
 * collection (TextureCollection, DG:117-149) and the other ranks receive their replica with one RCCL broadcast
 * over xGMI instead of reading the files again.  mark_written != 0: the caller is about to overwrite it. */
int ofdg_pool_device(ofdg_ctx* ctx, void** ptr, unsigned long long* bytes, int mark_written);

/*
 * Replaces the sampling half of load_batch (LAY:197-213):
 * generateBackground / generateNumberOfFgObjects / generateForegroundObject
 * (DG:2105-2835).  Appends n_tasks tasks; blueprints go to bps[0..*n_bps).
 * OFDG_SAMPLER_REF continues the 45 seeded streams of this ctx.
 */
int ofdg_sample(ofdg_ctx* ctx, int n_tasks, ofdg_task* tasks,
                ofdg_blueprint* bps, int bps_capacity, int* n_bps);

/*
 * THE HOT PATH.  Replaces commissionNewTask + Process_TaskBucket +
 * retrieveFinishedTask (DG:1175-1254, 1308-1349) and the batch assembly of
 * load_batch (LAY:227-250).  Renders task i into slot i of the caller-owned
 * DEVICE buffers image0 [n,3,H,W], image1 [n,3,H,W], flow [n,2,H,W] (float32,
 * planar, B,G,R order, 0..255).  Asynchronous on `stream` (a hipStream_t): the
 * outputs are written by a kernel on `stream`, after the work enqueued there before
 * the call, and work enqueued there after it sees them.  Internally the context owns
 * a few in-order streams ("chains", taking turns call by call) on which the record
 * upload / device sampler and the outline and coverage kernels of one call run back
 * to back, overlapping the neighbouring calls; the compose kernel follows on
 * `stream` after one event.  Pass ofdg_stream(ctx) as `stream` to run compose on the
 * chain's own stream too (no cross-stream wait at all; the compose kernels of
 * consecutive calls then overlap as well - the fast way to drive a prefetch ring:
 * one output buffer set per call in flight).
 */
/* As a call's `stream`: "the internal stream this call works on" - the same as passing ofdg_stream(ctx) read right before
 * the call, without the extra call. */
#define OFDG_STREAM_OWN ((void*)(~(uintptr_t)0))
int ofdg_render(ofdg_ctx* ctx, const ofdg_task* tasks, int n_tasks,
                const ofdg_blueprint* bps, int n_bps,
                float* d_image0, float* d_image1, float* d_flow, void* stream);

/* Re-run the device half of the last render / forward call (records already
 * resident in HBM): used to time the path with inputs resident. */
int ofdg_render_resident(ofdg_ctx* ctx, float* d_image0, float* d_image1,
                         float* d_flow, void* stream);

/* Prefetch ring (maps data_param.prefetch, LAY:36-56, 141-172): up to 16 batches can be
 * resident in HBM at once.  ofdg_upload_slot realises + uploads one batch into `slot`;
 * ofdg_render_slot renders a resident slot (any number of times).  ofdg_render and
 * ofdg_forward* keep their records in private slots of their own. */
int ofdg_upload_slot(ofdg_ctx* ctx, int slot, const ofdg_task* tasks, int n_tasks,
                     const ofdg_blueprint* bps, int n_bps, void* stream);
int ofdg_render_slot(ofdg_ctx* ctx, int slot, float* d_image0, float* d_image1,
                     float* d_flow, void* stream);

/* The sharding rule of ofdg_forward: step `step` of rank `rank` renders the global sample indices
 * ofdg_shard_first_index(step, batch, world_size, rank) + [0, batch) = step * batch * world_size + rank * batch + [0, batch);
 * over all ranks and steps these ranges tile the stream without gaps or overlap.  -1 for invalid arguments.
 * (The reference has no counterpart: every solver's layer renders the same samples, data_generation_layer.hpp:54.) */
long long ofdg_shard_first_index(long long step, int batch, int world_size, int rank);

/* Replaces Forward_cpu/Forward_gpu (LAY:266-291): sample batch_size tasks and
 * render them. */
int ofdg_forward(ofdg_ctx* ctx, float* d_image0, float* d_image1, float* d_flow,
                 void* stream);

/* Device counter-based sampler (OFDG_SAMPLER_COUNTER): the sampling half of load_batch
 * (LAY:197-213) on the GPU.  Sample g is a pure function of (seed, g); same modes and
 * distributions as the reference stream, statistically (not bitwise) equal to it.
 * ofdg_forward_counter samples + renders global indices first_index .. first_index+n-1
 * with no host data in the loop (ofdg_forward uses it when params.sampler is COUNTER:
 * rank r takes indices step*B*world + r*B + [0,B)).  ofdg_sample_counter downloads the
 * blueprints instead (fixed layout: 257 per sample = background, 32 object slots,
 * 32 x 7 component slots; unused slots have obj_type 0). */
int ofdg_forward_counter(ofdg_ctx* ctx, long long first_index, int n_samples,
                         float* d_image0, float* d_image1, float* d_flow, void* stream);
int ofdg_sample_counter(ofdg_ctx* ctx, long long first_index, int n_samples,
                        ofdg_task* tasks, ofdg_blueprint* bps);

/*
 * Optional outputs besides image0 / image1 / flow (rigid modes 1-8 and 10-13; caller-owned DEVICE buffers, slot i = task i):
 *   flow1   float32 [n,2,H,W]  backward flow (frame 1 -> frame 0): RenderCore::computeFlowImage(objects_map, true) (DG:801-818),
 *                              i.e. getPointFlow(x, y, inverse = true) of the object that owns index_image1(x, y) (DG:388-407,
 *                              background DG:692-718) with m_motion_inv (DG:320-321, 333-334) - the reference computes it but
 *                              never calls it (Process_TaskBucket, DG:1226)
 *   label0  uint8   [n,H,W]    index_image0 / index_image1 of blitObject (DG:762-775) as the painter's position of the owner:
 *   label1                     0 = background, k = the k-th top-level foreground object in ascending obj_id; an object owns a
 *                              pixel where its non-AA mask of that frame is 255 (a composite: its composed mask, DG:591-646),
 *                              the last owner in painter's order wins.  The ids of a task's foreground blueprints must be
 *                              distinct and > OFDG_BACKGROUND_ID (else OFDG_EINVAL); their order in the array is free
 *   occ0    float32 [n,1,H,W]  1.0f where the forward flow, rounded as xr = (int)floorf((float)x + u + 0.5f) (likewise y), leaves
 *                              the frame or lands on a frame-1 pixel of another label (label1[yr][xr] != label0[y][x]), else 0.0f
 *   occ1    float32 [n,1,H,W]  the same for frame-1 pixels with flow1, label1 at (x, y) and label0 at the target
 * Every member may be NULL independently.  ex == NULL (or all members NULL) is exactly the plain call.  Occlusion without
 * the labels / flow1 it needs keeps them in a workspace of the context.  Everything is written on the call's stream, in
 * the same order as the outputs.  Mode 9 with any member set fails with OFDG_EINVAL and enqueues nothing.
 */
typedef struct ofdg_extras {
  float*   flow1;   /* [n,2,H,W] or NULL */
  float*   occ0;    /* [n,1,H,W] or NULL */
  float*   occ1;    /* [n,1,H,W] or NULL */
  uint8_t* label0;  /* [n,H,W]   or NULL */
  uint8_t* label1;  /* [n,H,W]   or NULL */
} ofdg_extras;
int ofdg_render_ex(ofdg_ctx* ctx, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, int n_bps,
                   float* d_image0, float* d_image1, float* d_flow, const ofdg_extras* ex, void* stream);
int ofdg_forward_ex(ofdg_ctx* ctx, float* d_image0, float* d_image1, float* d_flow, const ofdg_extras* ex, void* stream);
int ofdg_forward_counter_ex(ofdg_ctx* ctx, long long first_index, int n_samples, float* d_image0, float* d_image1,
                            float* d_flow, const ofdg_extras* ex, void* stream);

/*
 * Compact output formats: the same calls with the frames as uint8 and / or the flow as IEEE binary16, chosen per call (like
 * ofdg_extras the format belongs to the call, not to the context).
 *   image  OFDG_FMT_F32  float32 [n,3,H,W] as in the plain calls
 *          OFDG_FMT_U8   uint8   [n,3,H,W], planar B,G,R: the byte itself - the value whose float is what the plain call stores
 *                        (the u8 -> float widening of DG:1229-1244 skipped; exact)
 *   flow   OFDG_FMT_F32  float32 [n,2,H,W] as in the plain calls
 *          OFDG_FMT_F16  binary16 [n,2,H,W]: the plain call's float32 value converted ONCE, round to nearest even.  This is
 *                        lossy: a half has 11 significant bits, so the spacing is 0.125 px from |flow| = 128 and 0.25 px from
 *                        256 (0.0625 px below 128), and values beyond 65504 become infinite.
 * Valid: image F32 | U8, flow F32 | F16.  fmt == NULL or {F32, F32} IS the plain call (same kernels, same bytes).  Any other
 * code in `image` / `flow`, or a non-zero `reserved`, fails with OFDG_EINVAL, enqueues nothing and names the field in
 * ofdg_last_error.  All 13 modes (mode 9 included), both samplers, every background_prep.  Layout, sample slots, stream
 * semantics, chains, tickets and error words are those of the plain calls.
 * The optional outputs of ofdg_extras in these formats: ofdg_*_ex_fmt below (these three calls take none).
 * Not offered: ofdg_render_slot / ofdg_render_resident, and the Caffe-shaped layer (ofdg_layer_forward returns float blobs,
 * as the layer it stands for does).
 */
#define OFDG_FMT_F32 0   /* float32 (the plain calls) */
#define OFDG_FMT_U8  1   /* frames only: the byte itself, uint8 [n,3,H,W] planar B,G,R */
#define OFDG_FMT_F16 2   /* flow only: IEEE binary16 [n,2,H,W], the float32 flow rounded to nearest even, once */
typedef struct ofdg_out_format { int32_t image; int32_t flow; int32_t reserved[2]; } ofdg_out_format;
int ofdg_render_fmt(ofdg_ctx* ctx, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, int n_bps,
                    void* d_image0, void* d_image1, void* d_flow, const ofdg_out_format* fmt, void* stream);
int ofdg_forward_fmt(ofdg_ctx* ctx, void* d_image0, void* d_image1, void* d_flow, const ofdg_out_format* fmt, void* stream);
int ofdg_forward_counter_fmt(ofdg_ctx* ctx, long long first_index, int n_samples, void* d_image0, void* d_image1,
                             void* d_flow, const ofdg_out_format* fmt, void* stream);

/*
 * The optional outputs together with the compact formats: ofdg_*_ex with an ofdg_out_format, and the extras in formats of
 * their own.  Everything is exact; nothing here has a tolerance.
 *   frames, flow    exactly what ofdg_*_fmt stores for `fmt`
 *   flow1           the float32 value ofdg_*_ex stores, in the element type of the flow (fmt->flow): with OFDG_FMT_F16 converted
 *                   once, round to nearest even - the same conversion as the flow
 *   label0, label1  as in ofdg_extras
 *   occ0, occ1      the definition of ofdg_extras, word for word: the target is rounded from the FLOAT32 flow,
 *                   xr = (int)floorf((float)x + u + 0.5f), whatever format the flow is stored in - asking for an fp16 flow never
 *                   changes an occlusion bit.  `occ` = OFDG_FMT_F32: float32 maps (1.0f / 0.0f, as ofdg_extras);
 *                   OFDG_FMT_U8: uint8 [n,1,H,W], 1 where the float32 map is 1.0f, else 0
 * ex == NULL or all pointers NULL behaves as the ofdg_*_fmt call; fmt == NULL or {F32, F32} with occ == OFDG_FMT_F32 behaves as
 * the ofdg_*_ex call: in both cases the kernels and the bytes are those calls'.  An invalid `occ` code, a non-zero `reserved`,
 * an invalid `fmt`, or mode 9 with any pointer set fail with OFDG_EINVAL, enqueue nothing and name the field in
 * ofdg_last_error.  As in the calls above every pointer is optional independently, occlusion without the labels it needs
 * keeps them (and the rounded targets) in a workspace of the context, and stream order, chains, tickets and error words are
 * the same.  Rigid modes 1-8 and 10-13, both samplers, every background_prep.
 */
typedef struct ofdg_extras_fmt {
  void*    flow1;   /* [n,2,H,W], element type = fmt->flow (float32 or binary16), or NULL */
  void*    occ0;    /* [n,1,H,W], element type by `occ`, or NULL */
  void*    occ1;    /* [n,1,H,W], element type by `occ`, or NULL */
  uint8_t* label0;  /* [n,H,W] or NULL, as in ofdg_extras */
  uint8_t* label1;  /* [n,H,W] or NULL, as in ofdg_extras */
  int32_t  occ;     /* OFDG_FMT_F32 (1.0f / 0.0f) | OFDG_FMT_U8 (1 / 0) */
  int32_t  reserved[3];
} ofdg_extras_fmt;
int ofdg_render_ex_fmt(ofdg_ctx* ctx, const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps, int n_bps,
                       void* d_image0, void* d_image1, void* d_flow, const ofdg_extras_fmt* ex, const ofdg_out_format* fmt,
                       void* stream);
int ofdg_forward_ex_fmt(ofdg_ctx* ctx, void* d_image0, void* d_image1, void* d_flow, const ofdg_extras_fmt* ex,
                        const ofdg_out_format* fmt, void* stream);
int ofdg_forward_counter_ex_fmt(ofdg_ctx* ctx, long long first_index, int n_samples, void* d_image0, void* d_image1,
                                void* d_flow, const ofdg_extras_fmt* ex, const ofdg_out_format* fmt, void* stream);

/*
 * Per-object annotation table: which objects a sample holds, where each one is visible in frame 0 and in frame 1, how much
 * of it, and the affine motion that produced its flow.  It restates what the reference keeps per object while it renders:
 * the index images of RenderCore::blitObject (DG:762-775) - here the label planes of ofdg_extras - reduced per object, and
 * m_motion as setMotion / addBackgroundMotion leave it (DG:312-335), the matrix the flow of the object's pixels is computed
 * with.  Rigid modes 1-8 and 10-13, both samplers.
 *
 * ofdg_object_table annotates the batch of the LAST render / forward call of this context (the batch ofdg_render_resident
 * and ofdg_debug_coverage speak of).  Row k of sample i is d_rows[i * rows_per_sample + k] and describes the object whose
 * label is k in the numbering of ofdg_extras: row 0 the background, row k the k-th top-level foreground object in ascending
 * obj_id (ids within a task are distinct and > OFDG_BACKGROUND_ID, whatever their order in the blueprint array: a task that
 * repeats one is refused when it is rendered).  d_counts[i] = 1 + n_objects of sample i whatever rows_per_sample is; rows k >= d_counts[i] inside the table are
 * all-zero bytes; objects k >= rows_per_sample are not reported (the count shows the truncation; no error flag is raised).
 * Areas and boxes are of VISIBLE pixels - those whose label is the row's index, i.e. after the painter's order has hidden
 * what lies below: an object wholly covered or moved out of the frame has area 0 and the empty box.
 *
 * d_label0 / d_label1: the [n,H,W] uint8 planes that call wrote (the caller's buffers; the workspace labels of an
 * occlusion-only call are not used).  Either may be NULL: that frame's areas are 0 and its boxes empty; both NULL leaves ids,
 * types, motions and counts.  The library cannot verify that the planes belong to that batch: it reduces what it is given
 * (a byte that is no label of the sample is counted nowhere).  d_rows is 8-byte, the planes and d_counts 4-byte aligned.
 *
 * Asynchronous: two small kernels on `stream`, nothing on the host beyond the argument checks.  `stream` is the stream the
 * labels were written on, i.e. the `stream` of that call; OFDG_STREAM_OWN: the internal stream that call worked on (which the
 * context remembers - ofdg_stream() already names the next call's).  The batch's records stay valid until the kernels have
 * read them: a later call that reuses them waits, as it does for a compose on a caller's stream.
 *
 * OFDG_EINVAL, nothing enqueued, the cause in ofdg_last_error: d_rows or d_counts NULL, rows_per_sample < 1, a misaligned
 * pointer, no render / forward call made yet on this context, a mode-9 context.
 */
#define OFDG_MAX_OBJECT_ROWS 65          /* background + 64 foreground objects */
typedef struct ofdg_object_row {         /* 96 bytes, no padding */
  int32_t obj_id;      /* blueprint obj_id (background: OFDG_BACKGROUND_ID) */
  int32_t obj_type;    /* OFDG_OBJ_ELLIPSE / POLYGON / COMPOSITE; 0 for the background row */
  int32_t area0, area1;/* pixels of frame 0 / frame 1 whose label is this row's index */
  int32_t box0[4];     /* x0, y0, x1, y1 inclusive, of those pixels in frame 0; area0 == 0: {W, H, -1, -1} */
  int32_t box1[4];     /* the same in frame 1 */
  double  motion[6];   /* m_motion as compose uses it (sx, shy, shx, sy, tx, ty; foreground: incl. background motion) */
} ofdg_object_row;
int ofdg_object_table(ofdg_ctx* ctx, const uint8_t* d_label0, const uint8_t* d_label1,
                      ofdg_object_row* d_rows, int rows_per_sample, int32_t* d_counts, void* stream);
/* The same reduction on the host (no GPU): fills area0 / area1 / box0 / box1 of the first min(counts[i], rows_per_sample)
 * rows of each of the n samples from HOST label planes [n,height,width] (either may be NULL: area 0, the empty box) and
 * leaves every other field and every other row alone.  OFDG_EINVAL (ofdg_host_last_error) for NULL counts / rows or sizes
 * below 1. */
int ofdg_host_object_table(const uint8_t* label0, const uint8_t* label1, int n, int width, int height,
                           const int32_t* counts, ofdg_object_row* rows, int rows_per_sample);

/*
 * Per-sample flow statistics: what the flow of a batch looks like, without copying the planes to the host - the histogram
 * of the displacement |flow| in bins of bin_px pixels (the sampler's tables were tuned against such a histogram), how many
 * pixels are unusable or occluded, the Q8 sums behind the mean u, v and |flow|, and the largest |flow|^2 with the pixel it
 * occurs at (what decides whether OFDG_FMT_F16 is safe: 0.125 px spacing from 128 px, infinite beyond 65504).  The reference
 * drops a "bad" task silently (DG:1285-1292); n_bad is the per-sample count a training loop can screen with.
 *
 * d_flow: any [n,2,H,W] flow tensor of the context's frame size - the forward flow or flow1 of ofdg_extras - float32
 * (flow_fmt = OFDG_FMT_F32, 16-byte aligned) or binary16 (OFDG_FMT_F16, 8-byte aligned).  d_occ: NULL, or the [n,1,H,W] map
 * that goes with it, float32 (occ_fmt = OFDG_FMT_F32, 16-byte aligned) or uint8 (OFDG_FMT_U8, 4-byte aligned); occ_fmt is not
 * looked at when d_occ is NULL.  All 13 modes, both samplers.  The result is a pure function of the buffers: the context
 * supplies W, H, the device and the stream only.
 *
 * Definition - integers and an order-independent maximum only, so every field is exact and the same on every run.  For pixel
 * (x, y) of sample i, u and v widened to float32 (exact for a binary16):
 *   1. d_occ given and occ != 0: n_occluded += 1; with OFDG_STATS_VISIBLE_ONLY the pixel contributes nothing else.
 *   2. not (fabsf(u) < 1048576.0f && fabsf(v) < 1048576.0f): n_bad += 1 and nothing else (NaN, +-inf, an overflowed half).
 *   3. otherwise n_counted += 1, and with m2 = fl32(fl32(u*u) + fl32(v*v)) (float32, no contraction):
 *        hist[b] += 1, b = the number of k in 1..63 with edge2[k] <= m2, edge2[k] = fl32(fl32((float)k * bin_px)^2)
 *                      (bins bin_px wide in pixels, a value on an edge belongs to the bin above, the last bin is open);
 *        sum_u_q8 += (int64)rintf(u * 256.0f), sum_v_q8 likewise, sum_mag_q8 += (int64)rintf(sqrtf(m2) * 256.0f)
 *                      (sqrtf correctly rounded, rintf to nearest even);
 *        max_key = max(max_key, ((uint64)bits(m2) << 32) | (0xFFFFFFFFu - idx)), idx = y*W + x, or (i*H + y)*W + x with
 *                      OFDG_STATS_ONE_ROW.
 * max_key >> 32 is the bit pattern of the largest |flow|^2, 0xFFFFFFFF - (uint32)max_key its first pixel in row-major order;
 * max_key == 0: no pixel was counted.  hist sums to n_counted; n_counted + n_bad (+ n_occluded with VISIBLE_ONLY) = H*W.
 *
 * Row i of d_rows is sample i's; with OFDG_STATS_ONE_ROW all n samples reduce into d_rows[0].  Without
 * OFDG_STATS_ACCUMULATE the call first writes every byte of its rows as zero on `stream`, then reduces; with it the rows are
 * added to (max for the key) - an all-zero row is the identity, so a caller zeroes rows once and keeps a running histogram
 * over an epoch with no host work.  d_rows is 8-byte aligned.
 *
 * Asynchronous on `stream`, the stream the flow was written on; OFDG_STREAM_OWN: the internal stream the last render /
 * forward call worked on, as in ofdg_object_table.  One kernel (behind the clearing of the rows), integer atomics only.
 *
 * OFDG_EINVAL, nothing enqueued, the rows untouched, the field named in ofdg_last_error: d_flow or d_rows NULL, flow_fmt /
 * occ_fmt not one of the codes above, n_samples < 1, bin_px NaN or outside [2^-10, 2^14], unknown bits in flags,
 * OFDG_STATS_VISIBLE_ONLY without d_occ, OFDG_STATS_ONE_ROW with n*H*W >= 2^32, a misaligned pointer, OFDG_STREAM_OWN before
 * any render / forward call on the context.
 */
#define OFDG_FLOW_HIST_BINS 64
#define OFDG_STATS_ACCUMULATE   1  /* add to the rows instead of overwriting them */
#define OFDG_STATS_VISIBLE_ONLY 2  /* pixels with occ != 0 count in n_occluded only */
#define OFDG_STATS_ONE_ROW      4  /* all n samples reduce into d_rows[0] */
typedef struct ofdg_flow_stats_row {   /* 304 bytes, no padding, 8-byte aligned */
  uint32_t hist[OFDG_FLOW_HIST_BINS];
  uint32_t n_counted, n_bad, n_occluded, reserved;
  int64_t  sum_u_q8, sum_v_q8, sum_mag_q8;
  uint64_t max_key;
} ofdg_flow_stats_row;
int ofdg_flow_stats(ofdg_ctx* ctx, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt,
                    int n_samples, float bin_px, int flags, ofdg_flow_stats_row* d_rows, void* stream);
/* The same on HOST buffers (no GPU): flow [n,2,height,width], occ NULL or [n,1,height,width], any width / height >= 1, no
 * alignment asked of the planes.  Errors as above (and for width / height < 1) through ofdg_host_last_error. */
int ofdg_host_flow_stats(const void* flow, int flow_fmt, const void* occ, int occ_fmt, int n, int width, int height,
                         float bin_px, int flags, ofdg_flow_stats_row* rows);

/*
 * Multi-scale ground-truth flow pyramid: the flow at 1/2 ... 1/64 resolution, as the losses of a coarse-to-fine network
 * (FlowNet, PWC-Net and their successors) read it, with a defined treatment of occluded and non-finite pixels and a fixed
 * order of summation - one launch behind the call that wrote the planes, the input read once, every level written in it.
 *
 * d_flow / d_occ: exactly as in the flow statistics above - any [n,2,H,W] flow tensor of the context's frame size (the
 * forward flow or flow1 of ofdg_extras), float32 (flow_fmt = OFDG_FMT_F32, 16-byte aligned) or binary16 (OFDG_FMT_F16, 8-byte
 * aligned); d_occ NULL, or the [n,1,H,W] map that goes with it, float32 (OFDG_FMT_F32, 16-byte aligned) or uint8 (OFDG_FMT_U8,
 * 4-byte aligned); occ_fmt is not looked at when d_occ is NULL.  All 13 modes, both samplers.  The result is a pure function
 * of the buffers: the context supplies W, H, the device and the stream only.
 *
 * pyr: where the levels go.  Level k = 1..levels is flow[k-1], [n,2,H>>k,W>>k] of out_fmt (OFDG_FMT_F32 or OFDG_FMT_F16), and -
 * when asked for - weight[k-1], [n,1,H>>k,W>>k] uint16.  A row of a level is (W>>k) elements and nothing more is assumed of it
 * (72 >> 3 = 9).  W and H must be multiples of 2^levels, so no cell straddles the frame's edge.  Entries at index >= levels are
 * never read.
 *
 * Definition - a fixed summation tree in float32 without contraction, so every bit is the same on every run.  For sample i,
 * u and v widened to float32 (exact for a binary16):
 *   usable pixel: fabsf(u) < 1048576.0f && fabsf(v) < 1048576.0f (the rule of n_bad above: it leaves out NaN, +-inf and an
 *                 overflowed half), and, when d_occ is given, occ == 0.
 *   level 0:      S0(x,y) = usable ? (u,v) : (+0.0f,+0.0f);  c0(x,y) = usable ? 1 : 0.
 *   level k >= 1, per component, over level k-1:
 *                 Sk(X,Y) = fl32( fl32(S(2X,2Y) + S(2X+1,2Y)) + fl32(S(2X,2Y+1) + S(2X+1,2Y+1)) )
 *                 (the left-right pairs first, then top and bottom);  ck = the integer sum of the four children.
 *   output of level k: ck == 0: +0.0f;  otherwise fl32(Sk / (float)ck), a correctly rounded division, and with
 *                 OFDG_PYR_SCALE then fl32(that * 2^-k) - the flow in pixels of level k.  Float32 denormals are kept.  For
 *                 OFDG_FMT_F16 the result is then rounded once to nearest even (an overflow becomes +-inf).
 *   weight[k-1](X,Y) = (uint16)ck: the usable pixels among the cell's 4^k, 0..4096.
 *
 * Asynchronous on `stream`, the stream the flow was written on; OFDG_STREAM_OWN: the internal stream the last render /
 * forward call worked on, as in the flow statistics.  One kernel, no atomics; it reads no record of the context, so no
 * completion bookkeeping is involved.
 *
 * OFDG_EINVAL, nothing enqueued, no output byte written, the field named in ofdg_last_error: d_flow or pyr NULL, levels
 * outside 1..OFDG_PYR_MAX_LEVELS, W or H not a multiple of 2^levels, flow[k-1] NULL for a k <= levels, weight[] set for some
 * levels <= levels and NULL for others, flow_fmt / occ_fmt / out_fmt not one of the codes above, n_samples < 1, unknown bits
 * in flags, a misaligned pointer (flow[k-1] 16-byte, weight[k-1] 4-byte), OFDG_STREAM_OWN before any render / forward call on
 * the context.
 *
 * The structure and the call share their name, as `struct stat` and stat do: say `struct ofdg_flow_pyramid` for the type.
 */
#define OFDG_PYR_MAX_LEVELS 6
#define OFDG_PYR_SCALE 1              /* level k in level-k pixels: the mean times 2^-k */
struct ofdg_flow_pyramid {
  void* flow[OFDG_PYR_MAX_LEVELS];    /* flow[k-1] = level k: [n,2,H>>k,W>>k], element type out_fmt; 16-byte aligned base */
  void* weight[OFDG_PYR_MAX_LEVELS];  /* all NULL, or weight[k-1] = [n,1,H>>k,W>>k] uint16: usable pixels of the cell, 0..4^k */
  int32_t levels;                     /* 1..6 */
  int32_t out_fmt;                    /* OFDG_FMT_F32 or OFDG_FMT_F16 */
};
int ofdg_flow_pyramid(ofdg_ctx* ctx, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt,
                      int n_samples, int flags, const struct ofdg_flow_pyramid* pyr, void* stream);
/* The same on HOST buffers (no GPU), the definition cell by cell: flow [n,2,height,width], occ NULL or [n,1,height,width],
 * any width / height >= 1 that are multiples of 2^levels, no alignment asked of any plane.  Errors as above through
 * ofdg_host_last_error. */
int ofdg_host_flow_pyramid(const void* flow, int flow_fmt, const void* occ, int occ_fmt, int n, int width, int height,
                           int flags, const struct ofdg_flow_pyramid* pyr);

/* The two reductions above on planes of another size than the context's frame - the planes ofdg_crop below wrote, for one.
 * ofdg_flow_stats_sized / ofdg_flow_pyramid_sized are ofdg_flow_stats / ofdg_flow_pyramid in every respect (definition,
 * stream, refusals, the same kernels) with [n,2,height,width] and [n,1,height,width] planes; the plane size follows the
 * context's own rule - width a multiple of 8 and at least 8, height even and at least 2 -, and the pyramid's rule that both
 * are multiples of 2^levels.  OFDG_EINVAL with the field named otherwise. */
int ofdg_flow_stats_sized(ofdg_ctx* ctx, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt, int n_samples,
                          int width, int height, float bin_px, int flags, ofdg_flow_stats_row* d_rows, void* stream);
int ofdg_flow_pyramid_sized(ofdg_ctx* ctx, const void* d_flow, int flow_fmt, const void* d_occ, int occ_fmt, int n_samples,
                            int width, int height, int flags, const struct ofdg_flow_pyramid* pyr, void* stream);

/*
 * Batch and tensor sizes of the operations on finished planes (ofdg_flow_stats above to ofdg_jpeg below).  n_samples is any
 * positive int: a launch has min(n_samples, 65535) rows of workgroups and a workgroup walks the samples i, i + rows, ..., so
 * from n_samples = 65536 on a workgroup serves several samples.  Pixel indices inside a sample are 32-bit (hence the refusal
 * of 3 * width * height of 2^32 and more); a sample's base is formed in 64 bits, so a tensor may exceed 4 GiB.  Both are
 * supported and tested for every one of these operations with n_samples = 65551 and tensors of 4.8 GiB and more
 * (tests/test_gpu_many_samples.py); none refuses them.  The one limit that involves n_samples is OFDG_STATS_ONE_ROW /
 * OFDG_ERR_ONE_ROW, whose pixel index runs over the whole batch: n_samples * height * width below 2^32.
 */

/*
 * Training crop: a crop_w x crop_h window of every output of a batch - frames, both flows, both occlusion maps, both label
 * planes -, each sample at its own position, optionally mirrored left-right and / or top-bottom, in ONE launch behind the
 * call that wrote the planes.  The window is a pure function of (seed, global sample index), so a resumed or sharded run
 * cuts the same windows.  Bits are moved and nothing is converted; a window that is also zoomed, rotated or squeezed is
 * ofdg_spatial below.
 *
 * Planes: src[k] is the [n,C,H,W] tensor of the context's frame size, dst[k] the [n,C,crop_h,crop_w] tensor of the same
 * element type; C = 3, 3, 2, 2, 1, 1, 1, 1 in the order of the enumerators.  image_fmt (image0, image1): OFDG_FMT_F32 or
 * OFDG_FMT_U8; flow_fmt (flow, flow1): OFDG_FMT_F32 or OFDG_FMT_F16; occ_fmt (occ0, occ1): OFDG_FMT_F32 or OFDG_FMT_U8; the
 * labels are uint8.  Every plane is optional on its own: src[k] and dst[k] both NULL.
 *
 * Record of sample i: recs[i] when recs is given, else ofdg_crop_draw(seed, first_index + i, W, H, crop_w, crop_h, flags).
 * Either way it is sanitised before use - x0 clamped to [0, W - crop_w], y0 to [0, H - crop_h], flags &= 3, reserved = 0 -,
 * so no record makes the kernel read outside a plane; the sanitised record is what recs_out[i] receives.
 *
 * Draw (ofdg_crop_draw): one block w of Philox4x32-10 with the counter sampler's key of global index g,
 * {seed ^ (uint32)(g >> 32) * 0x9E3779B9, (uint32)g}, and the counter {0, 0, 0x0c70, 0} (the sampler's third counter word is
 * always 0x0fd9: none of its streams is touched):  x0 = (uint32)(((uint64)w.x * (uint32)(W - crop_w + 1)) >> 32), y0 likewise
 * from w.y and H - crop_h + 1, HFLIP = w.z & 1 with OFDG_CROP_RANDOM_HFLIP (else 0), VFLIP = (w.z >> 1) & 1 with
 * OFDG_CROP_RANDOM_VFLIP (else 0).  No rejection loop: a position's probability is off by at most range / 2^32.
 *
 * Move, for destination pixel (X, Y) of channel c:  xs = x0 + (HFLIP ? crop_w - 1 - X : X), ys = y0 + (VFLIP ? crop_h - 1 - Y
 * : Y);  dst[i,c,Y,X] = the bits of src[i,c,ys,xs], with the sign bit inverted (XOR 0x80000000, 0x8000 for binary16) in
 * channel 0 of flow / flow1 under HFLIP and in channel 1 under VFLIP.  NaN payloads, -0.0 and infinities travel as bits.
 *
 * Occlusion with OFDG_CROP_OCC_WINDOW: a pixel whose flow target lies outside the window has no partner in the cropped
 * pair.  In source coordinates, with u, v of the GIVEN flow plane (flow for occ0, flow1 for occ1) at (xs, ys) widened to
 * float32:  tx = floorf(fl32(fl32((float)xs + u) + 0.5f)), ty likewise from ys and v;  inside iff tx >= (float)x0 && tx <=
 * (float)(x0 + crop_w - 1) and the same for ty with y0 and crop_h (a NaN is outside).  The map's element becomes 1.0f / 1
 * where the source element is non-zero (float32: compares unequal to zero - a NaN does, -0.0 does not) or the target is
 * outside, and keeps the source's bits otherwise.  No contraction anywhere.
 *
 * Asynchronous on `stream`, the stream the planes were written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  One kernel for
 * any n_samples, no atomics; it reads no record of the context, so no completion bookkeeping is involved.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, crop_w not a
 * multiple of 8 in [8, W], crop_h not even in [2, H], unknown flag bits, non-zero reserved, another format code, no plane
 * set, src[k] without dst[k] or the reverse, OFDG_CROP_OCC_WINDOW with occ0 but no flow (occ1 / flow1 likewise), a
 * misaligned pointer (sources as the render calls ask: 16-byte float32, 8-byte binary16, 4-byte uint8; destinations and both
 * record arrays 16-byte), a destination range (recs_out included) that overlaps any other range of the job (there is no
 * in-place form), W * H of 2^31 and more, OFDG_STREAM_OWN before any render / forward call on the context.
 */
#define OFDG_CROP_HFLIP         1   /* record flag: columns mirrored, u negated   */
#define OFDG_CROP_VFLIP         2   /* record flag: rows mirrored, v negated      */
#define OFDG_CROP_RANDOM_HFLIP  4   /* job flag: drawn records may carry HFLIP    */
#define OFDG_CROP_RANDOM_VFLIP  8   /* job flag: drawn records may carry VFLIP    */
#define OFDG_CROP_OCC_WINDOW   16   /* job flag: see "occlusion" above            */
typedef struct ofdg_crop_rec { int32_t x0, y0, flags, reserved; } ofdg_crop_rec;      /* 16 bytes */
enum { OFDG_CROP_IMAGE0, OFDG_CROP_IMAGE1, OFDG_CROP_FLOW, OFDG_CROP_FLOW1,
       OFDG_CROP_OCC0, OFDG_CROP_OCC1, OFDG_CROP_LABEL0, OFDG_CROP_LABEL1, OFDG_CROP_PLANES };
struct ofdg_crop_job {
  const void* src[OFDG_CROP_PLANES];   /* [n,C,H,W] of the context's frame, or NULL  */
  void*       dst[OFDG_CROP_PLANES];   /* [n,C,crop_h,crop_w], same element type     */
  const ofdg_crop_rec* recs;           /* DEVICE, n records, or NULL: drawn          */
  ofdg_crop_rec*       recs_out;       /* DEVICE, n records, or NULL                 */
  long long first_index;  uint32_t seed;
  int32_t crop_w, crop_h, flags, image_fmt, flow_fmt, occ_fmt, reserved;
};
int ofdg_crop(ofdg_ctx* ctx, const struct ofdg_crop_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes [n,C,height,width], records in host memory, no
 * alignment asked of any pointer.  Errors as above through ofdg_host_last_error. */
int ofdg_host_crop(const struct ofdg_crop_job* job, int n_samples, int width, int height);
/* The drawn record of global sample `index` (pure, no GPU).  OFDG_EINVAL (ofdg_host_last_error) for out NULL, crop_w outside
 * [1, width], crop_h outside [1, height] or flags other than OFDG_CROP_RANDOM_HFLIP | OFDG_CROP_RANDOM_VFLIP |
 * OFDG_CROP_OCC_WINDOW. */
int ofdg_crop_draw(uint32_t seed, long long index, int width, int height, int crop_w, int crop_h, int flags, ofdg_crop_rec* out);
/* The Philox4x32-10 block the draw is made of (pure, no GPU): out = Philox(counter, key) - the one definition the host draw and
 * the kernel share, exposed so that it can be held to the published known answers.  OFDG_EINVAL for a NULL pointer. */
int ofdg_crop_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);

/*
 * Photometric augmentation: gamma, contrast, brightness, per-channel colour gain and additive noise on image0 and image1 of
 * a batch, each sample by a record of its own and frame 1 slightly apart from frame 0, in ONE launch behind the call that
 * wrote the frames.  The record is a pure function of (seed, global sample index), the noise of (seed, global sample index,
 * frame, element), so a resumed or sharded run makes the same pixels.  Everything below is exact: the kernel, ofdg_host_photo
 * and the numpy restatement of the tests give the same bits.  float32 and fp64 operations are IEEE, each rounded on its own
 * (no contraction); fl32(.) marks a float32 rounding where the text would otherwise leave it open.
 *
 * Planes: src[f] is image f as [n,3,height,width] of src_fmt, dst[f] the same shape of dst_fmt; OFDG_FMT_F32 or OFDG_FMT_U8,
 * chosen independently.  A frame is optional on its own (src[f] and dst[f] both NULL).  width = height = 0: the context's
 * frame; otherwise any size the context's rule allows (width a multiple of 8 and at least 8, height even and at least 2) - the
 * frames ofdg_crop wrote, for one.  dst[f] == src[f] with src_fmt == dst_fmt is the in-place form.  The float32 frames of the
 * render / forward calls hold the blended BYTE values (compose blends in integers and stores (float)byte; the uint8 format
 * stores "the byte itself - the value whose float is what the plain call stores"), so both element types name a table index.
 *
 * Record of sample i: recs[i] when recs is given, else ofdg_photo_draw(seed, first_index + i, the job's ranges).  Either way
 * it is sanitised before use, and the sanitised record is what recs_out[i] receives.
 *
 * 1. Draw.  Philox4x32-10 (ofdg_crop_philox) under the counter sampler's key of global index g,
 *    {seed ^ (uint32)(g >> 32) * 0x9E3779B9, (uint32)g}, blocks j = 0, 1, 2 at the counters {j, 0, 0x0c71, 0} (the sampler's
 *    third counter word is 0x0fd9, the crop's 0x0c70).  u(w) = (float)(w >> 8) * 2^-24 (exact);  sym(w, a) = fl32(a *
 *    fl32(fl32(2 u(w)) - 1)), and a zero of either sign counts as +0.
 *      block 0:  lg0 = sym(.x, gamma_log)   lc0 = sym(.y, contrast_log)   b0 = sym(.z, brightness)   sigma = fl32(sigma_max * u(.w))
 *      block 1:  lB = sym(.x, colour_log)   lG = sym(.y, colour_log)      lR = sym(.z, colour_log)
 *      block 2:  dg = sym(.x, pair_gamma_log)  dc = sym(.y, pair_contrast_log)  db = sym(.z, pair_brightness)  dcol = sym(.w, pair_colour_log)
 *    Frame 1: lg1 = fl32(lg0 + dg), lc1 = fl32(lc0 + dc), b1 = fl32(b0 + db), and dcol is added to each of lB, lG, lR.  Every
 *    logarithm l becomes (float)EXP((double)l) - EXP and LOG: ofdg_det_exp, ofdg_det_log of include/ofdg_detmath.h -: gamma[f], contrast[f], gain[f][c];
 *    brightness[f] = b_f; sigma[1] = sigma[0] = sigma.  All ranges 0 give the identity record: gamma, contrast, gain 1.0f,
 *    brightness, sigma +0.
 * 2. Sanitise, field by field:  x is NaN ? identity : x < lo ? lo : x > hi ? hi : x  with  gamma [1/8, 8] identity 1,
 *    contrast [0, 4] identity 1, gain [0, 8] identity 1, brightness [-1, 1] identity 0, sigma [0, 64] identity 0; an infinity
 *    lands on a bound, -0.0 stays.  reserved = 0.  No record makes the kernel read or write outside a plane.
 * 3. Table, in fp64, for frame f, channel c (B, G, R) and k = 0..255:  x = k / 255.0;  p = 0 for k = 0, p = x for gamma[f] ==
 *    1.0f, else p = EXP((double)gamma[f] * LOG(x));  t = 255.0 * ((((p * gain[f][c]) - 0.5) * contrast[f] + 0.5)
 *    + brightness[f]), the float32 fields widened, evaluated in that order, six roundings;  t = t > 0 ? t : 0, then t = t < 255
 *    ? t : 255;  T[f][c][k] = (float)t.  The identity record gives T[f][c][k] = k.
 * 4. Pixel (y, x) of channel c of frame f of sample i.  k: the uint8 element; for float32 the element e with e = e > 0 ? e : 0
 *    (a NaN becomes 0), e = e < 255 ? e : 255, k = (int)rintf(e) (ties to even).  v = T[f][c][k].  Where sigma[f] > 0: with the
 *    element number m = (c * height + y) * width + x, w = word (m & 3) of the Philox block under the sample's key at the counter
 *    {m >> 2, f, 0x0c72, 0}, s = the sum of w's four bytes (0..1020, mean 510, variance 4 * (256^2 - 1) / 12 = 147.80054^2):
 *    v = fl32(v + fl32(fl32(sigma[f] / 147.80054f) * (float)(s - 510))), then v = v > 0 ? v : 0, v = v < 255 ? v : 255 - an
 *    Irwin-Hall normal of unit variance in 1021 levels, made of integers only.  sigma[f] == 0 draws nothing and leaves v as it
 *    is.  Output: float32 stores v, uint8 stores rintf(v) (ties to even).
 *
 * Asynchronous on `stream`, the stream the frames were written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  One kernel for any
 * n_samples, both frames and all channels, no atomics, no table in global memory; it reads no record of the context.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, one of width /
 * height 0 or a size that breaks the rule above, 3 * width * height of 2^32 and more, another format code, non-zero flags or
 * reserved, a range that is negative, NaN or infinite, no frame set, src[f] without dst[f] or the reverse, a misaligned pointer
 * (sources as the render calls ask: 16-byte float32, 4-byte uint8; destinations and both record arrays 16-byte), a destination
 * range (recs_out included) that overlaps any other range of the job - but for dst[f] == src[f] with src_fmt == dst_fmt -,
 * OFDG_STREAM_OWN before any render / forward call on the context.
 */
typedef struct ofdg_photo_rec {          /* 64 bytes; index [f] = frame 0 / 1, gain[f][c] c = B,G,R */
  float gamma[2], contrast[2], brightness[2], gain[2][3], sigma[2];
  int32_t reserved[2];
} ofdg_photo_rec;
struct ofdg_photo_job {
  const void* src[2]; void* dst[2];      /* image0, image1: [n,3,height,width]; each frame optional (src and dst both NULL) */
  const ofdg_photo_rec* recs;            /* DEVICE, n records, or NULL: drawn */
  ofdg_photo_rec*       recs_out;        /* DEVICE, n records, or NULL */
  long long first_index; uint32_t seed;
  int32_t width, height;                 /* 0, 0: the context's frame */
  int32_t src_fmt, dst_fmt;              /* OFDG_FMT_F32 or OFDG_FMT_U8, independently */
  int32_t flags, reserved;               /* no flag yet: both must be 0 */
  float gamma_log, contrast_log, brightness, colour_log, sigma_max;                 /* ranges of the draw, all >= 0 */
  float pair_gamma_log, pair_contrast_log, pair_brightness, pair_colour_log;        /* frame 1 against frame 0 */
};
int ofdg_photo(ofdg_ctx* ctx, const struct ofdg_photo_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes [n,3,height,width], records in host memory, no
 * alignment asked of any pointer.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above
 * through ofdg_host_last_error. */
int ofdg_host_photo(const struct ofdg_photo_job* job, int n_samples, int width, int height);
/* The drawn record of global sample `index` (step 1 alone: not sanitised; pure, no GPU).  Of `ranges` only the nine ranges are
 * read.  OFDG_EINVAL (ofdg_host_last_error) for a NULL pointer or a range that is negative, NaN or infinite. */
int ofdg_photo_draw(uint32_t seed, long long index, const struct ofdg_photo_job* ranges, ofdg_photo_rec* out);
/* The table [2][3][256] (frame, channel, k) of a HOST record after sanitising: as the DEVICE computes it (one small launch, waited
 * for), and as the host does.  Bit for bit the same.  OFDG_EINVAL for a NULL pointer. */
int ofdg_debug_photo_table(ofdg_ctx* ctx, const ofdg_photo_rec* rec_host, float* table_host);
int ofdg_host_photo_table(const ofdg_photo_rec* rec, float* table);
/* The function ofdg_det_log of include/ofdg_detmath.h on n numbers as this library was compiled (pure, no GPU): what the table's gamma is
 * made of, exposed so that its stated error bound can be held to libm.  OFDG_EINVAL for a NULL pointer or n < 0. */
int ofdg_host_det_log(const double* x, int n, double* log_out);

/*
 * Spatial augmentation: every output of a batch - frames, both flows, both occlusion maps, both label planes - resampled
 * through an affine map per sample and per frame (zoom, rotation, squeeze, translation, flips; frame 1 slightly apart from
 * frame 0) into an out_w x out_h window, the ground-truth flow transformed to match, in ONE launch behind the call that wrote
 * the planes.  The record is a pure function of (seed, global sample index), so a resumed or sharded run makes the same warps.
 * Everything below is exact: the kernel, ofdg_host_spatial and the numpy restatement of the tests give the same bits.  All
 * arithmetic is IEEE, each operation rounded on its own (no contraction); fl64(.) / fl32(.) mark a rounding where the text
 * would otherwise leave it open.
 *
 * Planes: the eight planes, their order and their formats are ofdg_crop's (OFDG_CROP_IMAGE0 .. OFDG_CROP_LABEL1, image_fmt,
 * flow_fmt, occ_fmt).  src[k] is [n,C,H,W] of the source size, dst[k] [n,C,out_h,out_w] of the same element type.  width =
 * height = 0: the source is the context's frame.  Source and output size each obey the context's rule (width a multiple of 8
 * and at least 8, height even and at least 2) and no side exceeds 2^20; the output may be smaller or larger than the source.
 * Every plane is optional on its own: src[k] and dst[k] both NULL.
 *
 * Record: m[f] = {a, b, c, d, e, g} maps destination pixel index (X, Y) of frame f to source pixel coordinates,
 *   qx = fl64(fl64(fl64(a * X) + fl64(b * Y)) + c),   qy = fl64(fl64(fl64(d * X) + fl64(e * Y)) + g).
 * The record of sample i is recs[i] when recs is given, else ofdg_spatial_draw(seed, first_index + i, ...).  Either way it is
 * sanitised before use, and the sanitised record is what recs_out[i] receives.  Sanitising, per frame f: when one of the six
 * entries is not finite, or one of |a|, |b|, |d|, |e| exceeds 64, or |c| or |g| exceeds 2^20, or det = fl64(fl64(a * e) -
 * fl64(b * d)) has |det| outside [2^-12, 2^12], m[f] becomes the centred integer window {1, 0, (W - out_w) / 2, 0, 1,
 * (H - out_h) / 2} (the quotients rounded toward -inf).  reserved = 0.  No record makes the kernel touch memory outside a plane.
 *
 * Tap of a pixel: Qx = (int)t, t = floor(fl64(fl64(qx * 256) + 0.5)) - 24.8 fixed point, as in the span interpolator of the
 * render path -; t below -2^30 counts as -2^30, above 2^30 as 2^30.  Qy likewise.  The pixel is inside when 0 <= Qx <= (W - 1)
 * * 256 && 0 <= Qy <= (H - 1) * 256.  ix = Qx >> 8, fx = Qx & 255 (arithmetic shift), likewise y; the four taps (ix, ix + 1) x
 * (iy, iy + 1) are each clamped to the frame, which replicates the border.  The nearest tap is nx = (Qx + 128) >> 8, ny
 * likewise, clamped.
 *
 * Frames: each element is widened to float32, both element types by the same expressions.  With the float32 weights w00 =
 * (256 - fx)(256 - fy), w10 = fx (256 - fy), w01 = (256 - fx) fy, w11 = fx fy and the elements e00 (ix, iy), e10 (ix + 1, iy),
 * e01 (ix, iy + 1), e11:
 *   v = fl32(fl32(fl32(fl32(w00 * e00) + fl32(w10 * e10)) + fl32(fl32(w01 * e01) + fl32(w11 * e11))) * 2^-16).
 * Every partial result is an integer below 2^24 when the elements are bytes, so the rendered frames (byte values in either
 * format) are interpolated exactly.  float32 stores v (a NaN as 0x7FC00000); uint8 stores rintf of v clamped to [0, 255] (ties
 * to even, a NaN becomes 0).
 *
 * Flow, at destination pixel (X, Y) of frame 0: (u, v) is the source flow at the NEAREST tap of m[0], widened to float32 -
 * interpolating it would mix the motions of two objects at every boundary.  The target in source frame 1 is tx = fl64(qx +
 * (double)u), ty likewise; it is mapped back through the inverse of m[1], made once per sample in fp64 with det as above:
 * ia = e / det, ib = -b / det, id = -d / det, ie = a / det;
 *   px = fl64(fl64(ia * fl64(tx - c)) + fl64(ib * fl64(ty - g))),   py = fl64(fl64(id * fl64(tx - c)) + fl64(ie * fl64(ty - g)))
 * with c, g of m[1];  u' = (float)fl64(px - X), v' = (float)fl64(py - Y); binary16 is then rounded once to nearest even.  A
 * non-finite source flow gives what that arithmetic gives, a NaN stored as 0x7FC00000 / 0x7E00 (the statistics and the pyramid
 * leave such pixels out).  flow1 is the same with the frames exchanged: taps of m[1], inverse of m[0].
 *
 * Labels: the element at the nearest tap of its frame.
 *
 * Occlusion maps: the element becomes 1.0f / 1 when the source element at the nearest tap is non-zero (the crop's rule: a NaN
 * is, -0.0 is not), or the pixel is not inside, or - with OFDG_SPATIAL_OCC_WINDOW - floor(fl64(px + 0.5)) lies outside [0,
 * out_w - 1] or floor(fl64(py + 0.5)) outside [0, out_h - 1], px, py from that frame's flow (occ0: flow, occ1: flow1; a NaN is
 * outside).  Otherwise it becomes +0.0f / 0.
 *
 * Draw (ofdg_spatial_draw): Philox4x32-10 (ofdg_crop_philox) under the counter sampler's key of global index g, blocks j = 0,
 * 1, 2 at the counters {j, 0, 0x0c73, 0} (0x0c70 .. 0x0c72 and 0x0fd9 are taken); u(w) and sym(w, a) are ofdg_photo's.
 *   block 0:  lz = sym(.x, zoom_log)  th = sym(.y, rot)  lq = sym(.z, squeeze_log);  h = -1 with OFDG_SPATIAL_RANDOM_HFLIP and
 *             .w & 1, else 1;  v = -1 with OFDG_SPATIAL_RANDOM_VFLIP and (.w >> 1) & 1, else 1
 *   block 1:  tfx = fl32(fl32(2 u(.x)) - 1)   tfy likewise from .y
 *   block 2:  dlz = sym(.x, pair_zoom_log)  dth = sym(.y, pair_rot)  dtx = sym(.z, pair_translate)  dty = sym(.w, pair_translate)
 * The map, in fp64 with EXP = ofdg_det_exp and sincos = ofdg_det_sincos of include/ofdg_detmath.h, for frame 0: gx = EXP(-(double)fl32(lz
 * + lq)), gy = EXP(-(double)fl32(lz - lq)), (s, c) = sincos((double)th);  a = c * gx * h, b = -(s * gy) * v, d = s * gx * h, e =
 * c * gy * v, each from left to right, a zero of either sign counting as +0.  The centre keeps the window inside the frame
 * where it fits: hw = (out_w - 1) / 2.0, hh = (out_h - 1) / 2.0, ex = |a| * hw + |b| * hh, slack = max((W - 1) / 2.0 - ex, 0), cx
 * = (W - 1) / 2.0 + ((double)tfx * translate) * slack, c = cx - (a * hw + b * hh); y the same with d, e, H, tfy: cy and g.
 * Frame 1: the same formulas with fl32(lz + dlz) for lz, fl32(th + dth) for th and the centre (cx + dtx, cy + dty).  No
 * rejection loop.  All ranges 0 give the centred identity window, frame 1 as frame 0.  translate is a fraction of the slack
 * in [0, 1], rot and pair_rot are radians, pair_translate is in source pixels.
 *
 * Asynchronous on `stream`, the stream the planes were written on; OFDG_STREAM_OWN as in ofdg_crop.  One kernel for any
 * n_samples, all planes and both frames, no atomics; it reads no record of the context.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, only one of
 * width / height 0, a source or output size that breaks the rule above, W * H or out_w * out_h of 2^31 and more, unknown flag
 * bits, non-zero reserved, another format code, a range that is negative, NaN or infinite, translate above 1, no plane set,
 * src[k] without dst[k] or the reverse, OFDG_SPATIAL_OCC_WINDOW with occ0 but no flow (occ1 / flow1 likewise), a misaligned
 * pointer (sources as the render calls ask: 16-byte float32, 8-byte binary16, 4-byte uint8; destinations and both record arrays
 * 16-byte), a destination range (recs_out included) that overlaps any other range of the job (there is no in-place form),
 * OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: bilinear sampling of the flow, mapping the boxes of the object table, non-affine (mode-9-style) augmentation
 * warps, an in-place form.
 */
#define OFDG_SPATIAL_RANDOM_HFLIP  4   /* job flag: drawn maps may mirror the columns */
#define OFDG_SPATIAL_RANDOM_VFLIP  8   /* job flag: drawn maps may mirror the rows    */
#define OFDG_SPATIAL_OCC_WINDOW   16   /* job flag: see "occlusion maps" above        */
typedef struct ofdg_spatial_rec {        /* 112 bytes; m[f] = {a, b, c, d, e, g} of frame f */
  double m[2][6];
  int32_t reserved[4];
} ofdg_spatial_rec;
struct ofdg_spatial_job {
  const void* src[OFDG_CROP_PLANES];     /* [n,C,height,width], or NULL                */
  void*       dst[OFDG_CROP_PLANES];     /* [n,C,out_h,out_w], same element type       */
  const ofdg_spatial_rec* recs;          /* DEVICE, n records, or NULL: drawn          */
  ofdg_spatial_rec*       recs_out;      /* DEVICE, n records, or NULL                 */
  long long first_index;  uint32_t seed;
  int32_t width, height;                 /* the source size; 0, 0: the context's frame */
  int32_t out_w, out_h, flags, image_fmt, flow_fmt, occ_fmt;
  int32_t reserved[2];
  float zoom_log, rot, squeeze_log, translate;            /* ranges of the draw, all >= 0 */
  float pair_zoom_log, pair_rot, pair_translate;          /* frame 1 against frame 0      */
};
int ofdg_spatial(ofdg_ctx* ctx, const struct ofdg_spatial_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes [n,C,height,width], records in host memory, no
 * alignment asked of any pointer.  width, height: the source size; the job's own must be 0, 0 or the same.  Errors as above
 * through ofdg_host_last_error. */
int ofdg_host_spatial(const struct ofdg_spatial_job* job, int n_samples, int width, int height);
/* The drawn record of global sample `index` (the draw alone: not sanitised; pure, no GPU).  Of `ranges` the seven ranges, flags,
 * width, height, out_w and out_h are read; the sizes must be set.  OFDG_EINVAL (ofdg_host_last_error) for a NULL pointer, a
 * size that breaks the rule, unknown flag bits or a range ofdg_spatial refuses. */
int ofdg_spatial_draw(uint32_t seed, long long index, const struct ofdg_spatial_job* ranges, ofdg_spatial_rec* out);

/* ---- network-ready frames and flow: ofdg_pack ----------------------------------------------------------------------------
 * The last stage of a data recipe in one launch: planar B,G,R frames holding 0..255 and a flow in pixels become what a network
 * reads - every channel scaled and shifted, optionally reordered to R,G,B, cast to the training element type, in planar or
 * channels-last memory, both frames optionally concatenated into one 6-channel tensor, the flow multiplied by a constant.
 *
 * Planes: src[OFDG_PACK_IMAGE0], src[OFDG_PACK_IMAGE1] are [n,3,height,width] of image_src_fmt (OFDG_FMT_F32 or OFDG_FMT_U8),
 * src[OFDG_PACK_FLOW] is [n,2,height,width] of flow_src_fmt (OFDG_FMT_F32 or OFDG_FMT_F16); any subset, a plane that is NULL
 * in src is NULL in dst.  width, height: 0, 0 for the context's frame, or a width that is a multiple of 8 (at least 8) with an
 * even height (at least 2) - the planes ofdg_crop and ofdg_spatial wrote.  Destinations are of image_dst_fmt / flow_dst_fmt:
 * OFDG_FMT_F32, OFDG_FMT_F16 or OFDG_FMT_BF16, chosen independently of each other and of the sources.
 *
 * Value.  Every float32 operation is IEEE, rounded on its own (no fused multiply-add), denormals kept.  A frame element x of
 * SOURCE channel c - (float)byte of a uint8 source, the element itself of a float32 one - gives y = fl32(fl32(x * scale[c]) +
 * bias[c]); scale and bias are per source channel B, G, R and serve both frames.  A flow element u - the float32 element, or
 * the binary16 one widened exactly - gives y = fl32(u * flow_scale).  What is stored of y:
 *   OFDG_FMT_F32   its bits
 *   OFDG_FMT_F16   y rounded once to nearest even: an overflow becomes +-inf, subnormals are kept (the conversion of the
 *                  compact formats above)
 *   OFDG_FMT_BF16  with b = the bits of y: (uint16_t)((b + 0x7FFF + ((b >> 16) & 1)) >> 16), i.e. round to nearest even on the
 *                  upper 16 bits; what is above 0x7F7F7FFF in magnitude becomes +-inf; a float32 denormal keeps its upper bits
 *   a NaN y        0x7FC00000 / 0x7E00 / 0x7FC0, whatever its sign and payload were (ofdg_spatial's rule)
 * -0.0 stays -0.0 in every format.  Which products overflow is the caller's business: with scale = 1/255 nothing does.
 *
 * Placement.  C = 3 for a frame, 6 with OFDG_PACK_CONCAT, 2 for the flow.  Source channel c of frame f goes to destination
 * channel cd = (OFDG_PACK_CONCAT ? 3 * f : 0) + (OFDG_PACK_RGB ? 2 - c : c) of dst[f] (of dst[0] with OFDG_PACK_CONCAT); the
 * flow's channels keep their order.  Element (i, cd, y, x) of a destination sits at element index
 *   OFDG_PACK_NCHW  ((i * C + cd) * height + y) * width + x
 *   OFDG_PACK_NHWC  ((i * height + y) * width + x) * C + cd      (what torch calls channels_last memory of a [n,C,H,W] tensor)
 * `layout` holds for the frames and the flow alike.
 *
 * Asynchronous on `stream`, the stream the planes were written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  ONE kernel for any
 * n_samples and every plane given, no atomics; it reads no record of the context.  Sources are left as they are.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, only one of
 * width / height 0, a size that breaks the rule above, 6 * width * height of 2^31 and more, a format code not listed for its
 * field, a layout other than 0 / 1, unknown flag bits, non-zero reserved, a scale, bias or flow_scale that is NaN or infinite,
 * no plane set, src[k] without dst[k] or the reverse, OFDG_PACK_CONCAT without both frames or with dst[1] set, a misaligned
 * pointer (sources as the render calls ask: 16-byte float32, 8-byte binary16, 4-byte uint8; destinations 16-byte), a
 * destination range that meets any other range of the job (there is no in-place form; a range is the n * C * height * width
 * elements of its plane), OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: a validity mask output, packing the levels of the flow pyramid, an in-place form; labels and occlusion maps
 * are left as they are.
 */
#define OFDG_FMT_BF16 3            /* ofdg_pack destinations only: bfloat16, the float32 value rounded to nearest even, once */
#define OFDG_PACK_NCHW 0           /* layout: [n,C,height,width] */
#define OFDG_PACK_NHWC 1           /* layout: [n,height,width,C] (torch channels_last memory) */
#define OFDG_PACK_CONCAT 1         /* flag: dst[0] holds both frames, C = 6 (image0's three channels, then image1's); dst[1] NULL */
#define OFDG_PACK_RGB    2         /* flag: destination channel c of a frame is source channel 2 - c (R,G,B instead of B,G,R) */
enum { OFDG_PACK_IMAGE0, OFDG_PACK_IMAGE1, OFDG_PACK_FLOW, OFDG_PACK_PLANES };
struct ofdg_pack_job {                       /* 112 bytes */
  const void* src[OFDG_PACK_PLANES];         /* image0, image1 [n,3,height,width]; flow [n,2,height,width]; each optional */
  void*       dst[OFDG_PACK_PLANES];
  int32_t width, height;                     /* 0, 0: the context's frame */
  int32_t image_src_fmt, flow_src_fmt;       /* F32 | U8;  F32 | F16 */
  int32_t image_dst_fmt, flow_dst_fmt;       /* F32 | F16 | BF16, independently */
  int32_t layout, flags;
  float scale[3], bias[3];                   /* per SOURCE channel B, G, R; both frames */
  float flow_scale;
  int32_t reserved;
};
int ofdg_pack(ofdg_ctx* ctx, const struct ofdg_pack_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition element by element: no alignment asked of any pointer.  width, height: the
 * plane size; the job's own must be 0, 0 or the same.  Errors as above through ofdg_host_last_error. */
int ofdg_host_pack(const struct ofdg_pack_job* job, int n_samples, int width, int height);

/* ---- motion boundaries: ofdg_boundaries --------------------------------------------------------------------------------------
 * The ground truth FlyingThings3D ships next to its occlusion masks and Sintel evaluates in bands of (d0-10, d10-60, d60-140):
 * a mask of the pixels on either side of a step in the flow, and the squared distance of every pixel to the nearest of them,
 * of both frames and every sample in ONE launch behind the call that wrote the flow.  Everything below is exact: the kernel,
 * ofdg_host_boundaries and the numpy restatement of the tests give the same bytes.
 *
 * Frames.  Frame f is processed when flow[f] is set and must then have at least one of edge[f] and dist2[f].  Frame 0 takes
 * flow (and label0), frame 1 flow1 (and label1); of a frame that is absent the label is not looked at.  flow[f] is
 * [n,2,height,width] of flow_fmt (OFDG_FMT_F32 or OFDG_FMT_F16), label[f] [n,height,width] uint8, edge[f] and dist2[f]
 * [n,1,height,width] uint8.  width, height: 0, 0 for the context's frame, or a width that is a multiple of 8 (at least 8) with
 * an even height (at least 2) - the planes ofdg_crop and ofdg_spatial wrote.
 *
 * Edge.  u and v are widened to float32 (exact for binary16).  Two 4-neighbours p, q (one apart in x or in y), both inside the
 * plane, are a STEP when - with OFDG_BND_LABELS - label[p] != label[q], and d2 > t2, where du = fl32(u_p - u_q), dv = fl32(v_p
 * - v_q), d2 = fl32(fl32(du * du) + fl32(dv * dv)) and t2 = fl32(min_step * min_step): IEEE float32, every operation rounded
 * on its own (no contraction), denormals kept.  A NaN d2 compares false, so inf - inf and anything beside a NaN is no step; an
 * infinite d2 is one (inf beside a finite value; +-65504 beside its negation in float32 is finite and compares as such).  With
 * min_step 0 a difference whose square underflows to 0 is no step.  The rule is symmetric in p and q.  edge(p) = 1 when p
 * belongs to at least one step, else 0: a boundary is two pixels thick, one on each side.  Without OFDG_BND_LABELS label[f]
 * is not read and may be NULL or set (left open by the issue: fixed here).
 *
 * Distance.  dist2(x, y) is the smallest (x - x')^2 + (y - y')^2 over the edge pixels (x', y') of the same sample and frame
 * for which that value is <= radius^2, or OFDG_BND_FAR when there is none: at most 225, 0 on the edge itself, and the Sintel
 * bands are thresholds on it (d < 10 is dist2 < 100).  Nothing wraps across samples, frames or the plane's border.  radius is
 * read only when a dist2 plane is set and must then lie in 1 .. OFDG_BND_MAX_RADIUS.
 *
 * All 13 modes: mode 9 renders no labels and works without OFDG_BND_LABELS (min_step then decides alone).
 *
 * Asynchronous on `stream`, the stream the planes were written on; OFDG_STREAM_OWN as in ofdg_crop.  One kernel for any
 * n_samples, both frames and both outputs, no atomics; it reads no record of the context.  Sources are left as they are.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, only one of
 * width / height 0, a size that breaks the rule above, width * height of 2^31 and more, unknown flag bits, non-zero reserved,
 * another flow_fmt, no frame present, an output of a frame without its flow, a frame with a flow and no output,
 * OFDG_BND_LABELS with a present frame that lacks its label, a min_step that is NaN, negative or infinite, a radius outside 1
 * .. 15 with a dist2 set, a misaligned pointer (flow 16-byte float32 / 8-byte binary16, labels 4-byte, outputs 16-byte), an
 * output range that overlaps any other range of the job (a range is the n * C * height * width elements of its plane; the label
 * of a present frame counts when set, used or not), OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: an 8-neighbour rule, radii above 15 or a float distance, per-sample boundary counts, packing these planes in
 * ofdg_pack, mapping them through ofdg_spatial other than by calling this entry on the warped planes, an in-place form.
 */
#define OFDG_BND_LABELS 1       /* a neighbour pair counts only where its labels differ; label[f] required */
#define OFDG_BND_MAX_RADIUS 15
#define OFDG_BND_FAR 255
struct ofdg_boundary_job {      /* 96 bytes */
  const void*    flow[2];       /* [n,2,H,W] flow / flow1, element type flow_fmt, or NULL: frame absent */
  const uint8_t* label[2];      /* [n,H,W] label0 / label1, or NULL */
  uint8_t*       edge[2];       /* [n,1,H,W] uint8 1 / 0, or NULL */
  uint8_t*       dist2[2];      /* [n,1,H,W] uint8, or NULL */
  int32_t width, height;        /* 0, 0: the context's frame */
  int32_t flow_fmt, flags, radius;
  float   min_step;
  int32_t reserved[2];
};
int ofdg_boundaries(ofdg_ctx* ctx, const struct ofdg_boundary_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: no alignment asked of any pointer.  width, height: the plane
 * size; the job's own must be 0, 0 or the same.  Errors as above through ofdg_host_last_error. */
int ofdg_host_boundaries(const struct ofdg_boundary_job* job, int n_samples, int width, int height);

/*
 * Occluder rectangles ("eraser" of the RAFT-style recipes): up to OFDG_ERASE_MAX_RECTS rectangles of image0 and / or image1 of
 * every sample are painted over IN PLACE - with the frame's mean colour, a constant or noise - and, with OFDG_ERASE_OCC, the
 * occlusion maps are extended by what the rectangles hide.  The record is a pure function of (seed, global sample index), the
 * noise of (seed, global sample index, frame, element), so a resumed or sharded run makes the same pixels.  Everything below
 * is exact: the kernels, ofdg_host_erase and the numpy restatement of the tests give the same bytes.  fl32(.) marks a float32
 * rounding (no contraction).
 *
 * Planes, all written in place: image[f] is image f as [n,3,height,width] of image_fmt (OFDG_FMT_F32 or OFDG_FMT_U8; the
 * float32 frames hold byte values, see ofdg_photo); occ[f] the occlusion map of frame f, [n,1,height,width] of occ_fmt (F32 or
 * U8), or NULL; flow[0] the forward flow, flow[1] flow1, [n,2,height,width] of flow_fmt (F32 or F16), read only, or NULL.
 * width = height = 0: the context's frame; otherwise any size the context's rule allows (the planes ofdg_crop / ofdg_spatial
 * wrote, for one).  flags: OFDG_ERASE_FRAME0 | OFDG_ERASE_FRAME1, the frames that may hold rectangles - at least one, and
 * image[f] of each must be given; an image[f] of a frame that is not flagged is not looked at -, and OFDG_ERASE_OCC.
 *
 * Record of sample i: recs[i] when recs is given, else ofdg_erase_draw(seed, first_index + i, width, height, the job).  Either
 * way it is sanitised before use, and the sanitised record, with the fill bytes, is what recs_out[i] receives.
 *
 * 1. Draw.  Philox4x32-10 (ofdg_crop_philox) under the counter sampler's key of global index g, {seed ^ (uint32)(g >> 32) *
 *    0x9E3779B9, (uint32)g}, blocks j = 0..4 at the counters {j, 0, 0x0c74, 0} (taken: 0x0fd9 the sampler, 0x0c70 crop, 0x0c71 and
 *    0x0c72 photo, 0x0c73 spatial; 0x0c75 is the noise fill below).  u(w) = (float)(w >> 8) * 2^-24 as in ofdg_photo;
 *    pick(w, lo, hi) = lo + (int)(((uint64)w * (uint32)(hi - lo + 1)) >> 32), the multiply-shift of the crop's draw.
 *      block 0:  erased = u(.x) < prob;  count = pick(.y, min_rects, max_rects);  frame of rectangle k = bit k of .z when both
 *                frames are flagged, else the flagged frame.
 *      block k + 1 (k = 0..3):  w = pick(.x, min_size, max_size)  h = pick(.y, min_size, max_size)
 *                x0 = pick(.z, 0, width - 1)  y0 = pick(.w, 0, height - 1)  - the top-left corner anywhere in the frame, the
 *                rectangle then clipped by step 2, as the RAFT recipe places it.  No rejection loop.
 *    Not erased: count 0.  Rectangles k >= count, fill and reserved are 0.
 * 2. Sanitise.  count = count < 0 ? 0 : count > 4 ? 4 : count.  For k < count in order: frame &= 1; the rectangle is dropped
 *    when its frame is not flagged, when w < 1 or h < 1, or when the clipped rectangle [max(x0, 0), min(x0 + w, width)) x
 *    [max(y0, 0), min(y0 + h, height)) (the sums in 64 bits) is empty; else it is kept, clipped.  The kept rectangles move to
 *    the front in their order, count becomes their number, every other rectangle, fill and reserved become 0.  No record makes
 *    a kernel touch a byte outside a plane.
 * 3. Fill byte of frame f, channel c (B, G, R), for every frame f that has a rectangle after step 2 (else fill[f][c] = 0):
 *      OFDG_ERASE_MEAN   the mean of that channel of the sample's frame BEFORE any rectangle is painted, in integers:
 *                        q = 256 * b for a uint8 element b; for a float32 element v:  v = v > 0 ? v : 0 (a NaN becomes 0),
 *                        v = v < 255 ? v : 255,  q = (uint32)rintf(fl32(v * 256.0f)) (ties to even).  S = the sum of q over
 *                        the P = width * height elements (64 bits),  mean_q8 = (2 S + P) / (2 P) by integer division,
 *                        m = (mean_q8 + 128) >> 8.  The same frame in either format gets the same m.
 *      OFDG_ERASE_CONST  m = color[c], each in 0..255.
 *      OFDG_ERASE_NOISE  fill[f][c] = 0; the element e = c * P + y * width + x of the frame gets the top byte (>> 24) of
 *                        word (e & 3) of the Philox block under the sample's key at the counter {e >> 2, f, 0x0c75, 0}.
 *    Every element inside a rectangle of frame f becomes m (the noise byte): a uint8 frame stores the byte, a float32 frame
 *    (float)byte.  A painted value does not depend on the rectangle, so overlapping rectangles need no order.  Elements
 *    outside keep their bits.
 * 4. Occlusion, with OFDG_ERASE_OCC, for each occ[f] given: element (y, x) becomes 1.0f / 1 when it lies inside a rectangle of
 *    frame f, or - when frame 1 - f is flagged - when its target lies inside a rectangle of frame 1 - f: with (u, v) the
 *    element's flow[f] widened to float32, tx = floorf(fl32(fl32((float)x + u) + 0.5f)), ty likewise from y and v (the
 *    formula of OFDG_CROP_OCC_WINDOW), inside when x0 <= tx <= x0 + w - 1 and y0 <= ty <= y0 + h - 1, compared as float32 (a
 *    NaN is in no rectangle).  All other elements keep their bits.  When frame 1 - f is flagged, occ[f] needs flow[f].
 *    Without the flag occ and flow are not looked at; nor is a flow[f] that no given map needs.
 *
 * work: DEVICE memory of n_samples * OFDG_ERASE_WORK_BYTES, 16-byte aligned, required for OFDG_ERASE_MEAN only (else not looked
 * at); contents unspecified before and after.  Asynchronous on `stream`, the stream the planes were written on; OFDG_STREAM_OWN
 * as in ofdg_flow_stats.  At most one clearing of `work` and two kernels per call, integer atomics only.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, a size that
 * breaks the rule above, 3 * width * height of 2^31 and more, another format code (occ_fmt and flow_fmt count with
 * OFDG_ERASE_OCC only), unknown flag bits, non-zero reserved, no frame flag, a flagged frame without its image, another fill
 * code, a colour outside 0..255 (OFDG_ERASE_CONST), prob outside [0, 1] or NaN, min_rects <= max_rects outside 0..4, 1 <=
 * min_size <= max_size <= 32767 broken (the ranges count when recs is NULL), OFDG_ERASE_OCC with no map or with a map
 * that lacks its flow, work NULL under OFDG_ERASE_MEAN, a misaligned pointer (images, maps and flows as the render calls ask:
 * 16-byte float32, 8-byte binary16, 4-byte uint8; work and both record arrays 16-byte), a written range (images, maps, work,
 * recs_out) that overlaps any other range of the job, OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: textured occluders from the pool, shapes other than rectangles, a copying form, label planes, the object table
 * and boundary planes (they stay those of the un-erased sample), mode 9 beyond painting (it has no maps to mark).
 */
#define OFDG_ERASE_MAX_RECTS 4
#define OFDG_ERASE_FRAME0 1          /* job flag: frame 0 may hold rectangles */
#define OFDG_ERASE_FRAME1 2          /* job flag: frame 1 may hold rectangles */
#define OFDG_ERASE_OCC    4          /* job flag: step 4 */
#define OFDG_ERASE_MEAN  0           /* job->fill */
#define OFDG_ERASE_CONST 1
#define OFDG_ERASE_NOISE 2
#define OFDG_ERASE_WORK_BYTES 64     /* of job->work per sample */
typedef struct ofdg_erase_rect { int32_t x0, y0, w, h, frame; } ofdg_erase_rect;
typedef struct ofdg_erase_rec {      /* 96 bytes */
  int32_t count;                     /* 0..OFDG_ERASE_MAX_RECTS */
  ofdg_erase_rect rect[OFDG_ERASE_MAX_RECTS];
  uint8_t fill[2][3];                /* [frame][B,G,R]: written into recs_out, never read */
  uint8_t reserved[6];
} ofdg_erase_rec;
struct ofdg_erase_job {              /* 152 bytes */
  void* image[2];                    /* [n,3,height,width] of image_fmt, in place */
  void* occ[2];                      /* [n,1,height,width] of occ_fmt, in place, or NULL */
  const void* flow[2];               /* [n,2,height,width] of flow_fmt: flow, flow1, or NULL */
  const ofdg_erase_rec* recs;        /* DEVICE, n records, or NULL: drawn */
  ofdg_erase_rec*       recs_out;    /* DEVICE, n records, or NULL */
  void* work;                        /* DEVICE, n * OFDG_ERASE_WORK_BYTES (OFDG_ERASE_MEAN) */
  long long first_index; uint32_t seed;
  int32_t width, height;             /* 0, 0: the context's frame */
  int32_t image_fmt, occ_fmt, flow_fmt, flags, fill;
  int32_t min_rects, max_rects, min_size, max_size;   /* ranges of the draw */
  float   prob;
  int32_t color[3];                  /* B, G, R of OFDG_ERASE_CONST */
  int32_t reserved[2];
};
int ofdg_erase(ofdg_ctx* ctx, const struct ofdg_erase_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes and records in host memory, no alignment asked of any
 * pointer, work not looked at.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above
 * through ofdg_host_last_error. */
int ofdg_host_erase(const struct ofdg_erase_job* job, int n_samples, int width, int height);
/* The drawn record of global sample `index` for a width x height plane (step 1 alone: not sanitised; pure, no GPU).  Of `ranges`
 * only flags, prob and the four ranges are read.  OFDG_EINVAL (ofdg_host_last_error), `out` untouched, for a NULL pointer, width or
 * height outside 1..32768, no frame flag, unknown flag bits or a range that breaks the rules above. */
int ofdg_erase_draw(uint32_t seed, long long index, int width, int height, const struct ofdg_erase_job* ranges, ofdg_erase_rec* out);

/*
 * Colour jitter ("ColorJitter" of the RAFT-family recipes): brightness, contrast about the frame's own mean luminance,
 * saturation and hue on image0 and / or image1 of a batch, each sample by a record of its own, the four operations in the
 * sample's own order, both frames alike or - with a drawn probability - each on its own.  What ofdg_photo's one table per
 * channel cannot hold: saturation and hue mix the three channels of a pixel, the contrast needs a reduction over the frame at
 * its place in the chain.  The record is a pure function of (seed, global sample index).  Everything below is integers: the
 * kernels, ofdg_host_jitter and the numpy restatement of the tests give the same bytes.  >> is the arithmetic (floor) shift.
 *
 * Planes, formats, sizes and aliasing as in ofdg_photo: src[f] is image f as [n,3,height,width] planar B, G, R of src_fmt, dst[f]
 * the same shape of dst_fmt; OFDG_FMT_F32 or OFDG_FMT_U8, chosen independently.  A frame is present when both its pointers are
 * given (src[f] and dst[f] both NULL: absent).  width = height = 0: the context's frame; otherwise any size the context's rule
 * allows.  dst[f] == src[f] with src_fmt == dst_fmt is the in-place form.  The byte of a uint8 element is itself, of a float32
 * element the index rule of ofdg_photo (clamped to [0, 255], a NaN 0, to nearest even); a uint8 destination stores the byte, a
 * float32 one (float)byte.
 *
 * Record of sample i: recs[i] when recs is given, else ofdg_jitter_draw(seed, first_index + i, the job's ranges).  Either way
 * it is sanitised before use, and the sanitised record, with the means, is what recs_out[i] receives.  Per frame f:
 * brightness[f], contrast[f], saturation[f] in Q16 (65536: no change), hue[f] in units of 1 / 393216 of a turn (65536 per
 * 60-degree sector), order[f] in 0..23: the index of the permutation of (brightness, contrast, saturation, hue) in
 * lexicographic order - 0: b c s h, 1: b c h s, ... 23: h s c b.  shared: the contrast's mean is taken over both frames together.
 *
 * 1. Draw.  Philox4x32-10 (ofdg_crop_philox) under the counter sampler's key of global index g, {seed ^ (uint32)(g >> 32) *
 *    0x9E3779B9, (uint32)g}, blocks j = 0, 1, 2 at the counters {j, 0, 0x0c78, 0} (taken: 0x0fd9 the sampler, 0x0c70 crop, 0x0c71
 *    and 0x0c72 photo, 0x0c73 spatial, 0x0c74 and 0x0c75 erase, 0x0c76 motion blur, 0x0c77 splat).  A = (int)lrintf(range *
 *    65536.0f) for brightness, contrast and saturation, (int)lrintf(range * 393216.0f) for hue (to nearest even);  isym(w, A) =
 *    (int)(((uint64)w * (uint32)(2 A + 1)) >> 32) - A, uniform on [-A, A];  u(w) = (float)(w >> 8) * 2^-24 as in ofdg_photo.
 *      block f (f = 0, 1):  brightness[f] = 65536 + isym(.x, A_b)   contrast[f] = 65536 + isym(.y, A_c)
 *                           saturation[f] = 65536 + isym(.z, A_s)   hue[f] = isym(.w, A_h)
 *      block 2:  asymmetric = u(.x) < asym_prob;  order[0] = (int)(((w.y >> 8) * 24) >> 24);  order[1] likewise from .z
 *    Not asymmetric: frame 1 takes frame 0's five fields and shared = 1; asymmetric: shared = 0.  mean = {-1, -1}, reserved 0.
 *    All ranges 0 give an identity record: every factor 65536, both hues 0 (the order is drawn all the same; it then changes
 *    nothing).
 * 2. Sanitise.  Factors clamp to [0, 4 * 65536], hue to [-196608, 196608] (half a turn either way), order to 0..23; shared
 *    becomes 1 where it is non-zero and the two frames' five fields are equal, else 0; mean = {-1, -1}; reserved = 0.
 * 3. The operations, on the three bytes (B, G, R) of a pixel; each ends in bytes, as the recipe's uint8 pipeline does.
 *      lum = (7471 B + 38470 G + 19595 R + 32768) >> 16                        (Rec.601; the weights sum to 65536)
 *      mix(a, m, q) = clamp((q a + (65536 - q) m + 32768) >> 16, 0, 255)        (fits 32 bits; mix(a, m, 65536) == a)
 *      brightness:  c = mix(c, 0, brightness[f])        saturation:  c = mix(c, lum of the pixel, saturation[f])
 *      contrast:    c = mix(c, mean, contrast[f]), mean of step 4
 *      hue: the HSV hue shift without leaving integers.  mx, mn: the largest and smallest of the three, d = mx - mn.  d == 0:
 *        unchanged.  Else the sector s of the hexagon is the first of  0: max R min B,  1: max G min B,  2: max G min R,
 *        3: max B min R,  4: max B min G,  5: max R min G  that holds (mid: the third channel), and the distance into it
 *        t = mid - mn in even sectors, d - (mid - mn) in odd ones.  Hq = (65536 s + (65536 t) / d + hue[f]) mod 393216, the
 *        division floored, the modulus non-negative;  s' = Hq >> 16, f' = Hq & 65535;  the new third channel is
 *        mn + ((d f' + 32768) >> 16) in even s', mn + ((d (65536 - f') + 32768) >> 16) in odd s'; mx and mn go where sector
 *        s' has its largest and smallest.  A hue of 0 changes nothing, one of 131072 is (R, G, B) -> (B, R, G); against a float
 *        HSV round trip a channel is off by less than 0.5 + 255 / 65536.
 *    The four run in the order order[f] names.  A frame whose three factors are 65536 and whose hue is 0 is copied - bit for
 *    bit where src_fmt == dst_fmt (in place: not touched at all), else through its bytes.
 * 4. Mean, for a frame with contrast[f] != 65536 (else none is computed and mean[f] = -1):  S = the sum of lum over the N =
 *    width * height pixels of the frame AFTER the operations that stand before the contrast in order[f], in 64 bits;
 *    mean[f] = (2 S + N) / (2 N) by integer division: a byte.  With shared set and both frames present S and N are those of
 *    both frames together (the frames' fields are equal then), and mean[1] = mean[0]; with one frame present, that frame's.
 *    An absent frame has mean[f] = -1.
 *
 * work: DEVICE memory of n_samples * OFDG_JITTER_WORK_BYTES, 16-byte aligned; contents unspecified before and after (the call
 * clears it).  Required whenever recs is given, and with drawn records unless A_c = 0 (a contrast range of at most 2^-17: no
 * drawn record has a contrast then, so no mean is taken and `work` is not looked at).  Asynchronous on `stream`, the stream
 * the frames were written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  At most one clearing of `work` and two kernels per
 * call, integer atomics only; it reads no record of the context and works in every mode.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, one of width /
 * height 0 or a size that breaks the rule, 3 * width * height of 2^32 and more, another format code, non-zero flags or
 * reserved, a range that is negative, NaN, infinite or above its bound (brightness, contrast, saturation 3, hue 0.5,
 * asym_prob 1), no frame set, src[f] without dst[f] or the reverse, work NULL where it is required, a misaligned pointer
 * (sources as the render calls ask: 16-byte float32, 4-byte uint8; destinations, work and both record arrays 16-byte), a
 * written range (destinations, work, recs_out) that overlaps any other range of the job - but for dst[f] == src[f] with
 * src_fmt == dst_fmt -, OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: bit parity with any framework's ColorJitter (those truncate where this rounds, and keep a float mean), a
 * probability per operation, gamma and noise (ofdg_photo).
 */
#define OFDG_JITTER_WORK_BYTES 16    /* of job->work per sample */
typedef struct ofdg_jitter_rec {     /* 64 bytes; index [f] = frame 0 / 1 */
  int32_t brightness[2], contrast[2], saturation[2];   /* Q16 */
  int32_t hue[2];                    /* 1 / 393216 of a turn */
  int32_t order[2];                  /* 0..23 */
  int32_t shared;                    /* 0 / 1 */
  int32_t mean[2];                   /* written into recs_out, never read: the byte the contrast pivots on, or -1 */
  int32_t reserved[3];
} ofdg_jitter_rec;
struct ofdg_jitter_job {             /* 112 bytes */
  const void* src[2]; void* dst[2];  /* image0, image1: [n,3,height,width]; each frame optional (src and dst both NULL) */
  const ofdg_jitter_rec* recs;       /* DEVICE, n records, or NULL: drawn */
  ofdg_jitter_rec*       recs_out;   /* DEVICE, n records, or NULL */
  void* work;                        /* DEVICE, n * OFDG_JITTER_WORK_BYTES */
  long long first_index; uint32_t seed;
  int32_t width, height;             /* 0, 0: the context's frame */
  int32_t src_fmt, dst_fmt;          /* OFDG_FMT_F32 or OFDG_FMT_U8, independently */
  int32_t flags, reserved;           /* no flag yet: both must be 0 */
  float brightness, contrast, saturation, hue, asym_prob;   /* ranges of the draw: <= 3, 3, 3, 0.5 (turns), 1 */
};
int ofdg_jitter(ofdg_ctx* ctx, const struct ofdg_jitter_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes and records in host memory, no alignment asked of any
 * pointer, work not looked at.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above
 * through ofdg_host_last_error. */
int ofdg_host_jitter(const struct ofdg_jitter_job* job, int n_samples, int width, int height);
/* The drawn record of global sample `index` (step 1 alone: not sanitised; pure, no GPU).  Of `ranges` only the five ranges are
 * read.  OFDG_EINVAL (ofdg_host_last_error), `out` untouched, for a NULL pointer or a range that is negative, NaN, infinite
 * or above its bound. */
int ofdg_jitter_draw(uint32_t seed, long long index, const struct ofdg_jitter_job* ranges, ofdg_jitter_rec* out);
/* The hue operation of step 3 alone on `pixels` pixels of planar bytes (pure, no GPU): bgr and out are [3][pixels], B, G, R; out
 * may be bgr.  hue is taken as it is, not sanitised, anywhere in [-393216, 393216] - exposed so that the operation's identities
 * (a whole turn either way, the channel rotation) can be held over the whole colour cube.  OFDG_EINVAL for a NULL pointer or a
 * hue outside that range. */
int ofdg_host_jitter_hue(const uint8_t* bgr, uint8_t* out, size_t pixels, int hue);

/*
 * Camera: the optics and the sensor on image0 and / or image1 of a batch - a Gaussian lens blur and the artefacts of a Bayer
 * mosaic that is interpolated back (the two camera effects Mayer et al., IJCV 2018, found to help on real data), each sample
 * by a record of its own.  ofdg_motion_blur is the exposure; this is what stands behind it and in front of the sensor noise
 * of ofdg_photo.  The record is a pure function of (seed, global sample index).  Everything below is integers on bytes but
 * for the tap table, which is fp64 through ofdg_det_exp of include/ofdg_detmath.h, and therefore the same bits on host and
 * device: the kernel, ofdg_host_camera and the numpy restatement of the tests give the same bytes.
 *
 * Planes, formats and sizes as in ofdg_jitter: src[f] is image f as [n,3,height,width] planar B, G, R of src_fmt, dst[f] the
 * same shape of dst_fmt; OFDG_FMT_F32 or OFDG_FMT_U8, chosen independently.  A frame is present when both its pointers are
 * given (src[f] and dst[f] both NULL: absent).  width = height = 0: the context's frame; otherwise any size the context's
 * rule allows (width a multiple of 8 and at least 8, height even and at least 2).  There is NO in-place form - a pixel reads
 * its neighbours -: dst[f] == src[f] is an overlap and is refused.  The byte of a uint8 element is itself, of a float32
 * element the index rule of ofdg_photo (clamped to [0, 255], a NaN 0, to nearest even); a uint8 destination stores the byte,
 * a float32 one (float)byte.  It reads no record of the context and works in every mode.
 *
 * Record of sample i: recs[i] (DEVICE memory) when recs is given, else ofdg_camera_draw(seed, first_index + i, the job's
 * ranges).  Either way it is sanitised before use, and the sanitised record, with the radii, is what recs_out[i] receives.
 * sigma_q8[f]: the lens blur's sigma of frame f in 1 / 256 px, 0..1024 (0: none).  bayer: -1 none, 0..3 the pattern.
 *
 * 1. Draw.  Philox4x32-10 (ofdg_crop_philox) under the counter sampler's key of global index g, {seed ^ (uint32)(g >> 32) *
 *    0x9E3779B9, (uint32)g}, blocks j = 0, 1 at the counters {j, 0, 0x0c79, 0} (taken: 0x0c70 .. 0x0c78 and 0x0fd9, see
 *    ofdg_jitter).  u() and isym() as in ofdg_jitter.  lo = lrintf(sigma_min * 256), hi = lrintf(sigma_max * 256),
 *    D = lrintf(sigma_delta * 256) (to nearest even).
 *      block 0:  blurred = u(.x) < blur_prob
 *                s0 = lo + (int)(((uint64).y * (uint32)(hi - lo + 1)) >> 32)         uniform on [lo, hi]
 *                s1 = s0 + isym(.z, D)
 *                mosaic = u(.w) < bayer_prob
 *      block 1:  p = pattern >= 0 ? pattern : (int)(.x >> 30)
 *    sigma_q8 = blurred ? {s0, s1} : {0, 0};  bayer = mosaic ? p : -1;  radius = {0, 0};  reserved = 0.  Both frames share
 *    the pattern - it is one camera -, frame 1's focus is up to sigma_delta apart, as the other stages keep frame 1 slightly
 *    apart.
 * 2. Sanitise.  sigma_q8 clamps to [0, 1024]; a bayer outside -1..3 becomes -1; radius[f] = min(12, (3 sigma_q8[f] + 255)
 *    >> 8): three sigma, rounded up; reserved = 0.
 * 3. Taps, for s = sigma_q8[f] > 0 and R = radius[f], exp being ofdg_det_exp of include/ofdg_detmath.h in fp64:
 *      e[k] = (uint32)llrint(exp(-(double)(k k) * 32768.0 / (double)(s s)) * 16777216.0)       k = 0..R
 *      E    = e[0] + 2 (e[1] + .. + e[R])
 *      w[k] = (e[k] * 65536 + E / 2) / E        k >= 1, in 64-bit integers, the division floored
 *      w[0] = 65536 - 2 (w[1] + .. + w[R])
 *    The weights sum to exactly 65536, do not increase outward, and w[0] > 0, for every s.  ofdg_camera_taps exports the
 *    table.  Known answers: s = 85: 64160, 688;  s = 256: 26152, 15862, 3539, 291.
 * 4. Blur, per channel, on the bytes a(x, y); coordinates are clamped to the plane (the edge is replicated):
 *      h8(x, y)  = (sum_k w[|k|] a(x + k, y) + 128) >> 8                     at most 65280
 *      out(x, y) = (sum_k w[|k|] h8(x, y + k) + 8388608) >> 24
 *    Both sums fit unsigned 32 bits (the largest is 65280 * 65536 + 2^23).  A constant plane is unchanged.  s = 0: no blur.
 *    Against the float64 separable convolution with the same truncated, normalised Gaussian a byte is off by at most 0.75
 *    (0.5 the last rounding, 1 / 512 that of h8, under 0.19 the quantised taps over two passes).
 * 5. Mosaic and demosaic, on the blurred bytes P_B, P_G, P_R, for bayer = p >= 0.  The site of (x, y) is a = (x + (p & 1)) & 1,
 *    b = (y + (p >> 1)) & 1:  (0, 0) is R, (1, 1) is B, the other two are G - p = 0 is RGGB.  m(x, y) = P_site(x, y)(x, y), the one
 *    sample the sensor has there.  Coordinates are reflected without repeating the edge (-1 -> 1, W -> W - 2), which keeps the
 *    parity, so a reflected neighbour has the colour the pattern expects there (W >= 8, H >= 2 by the size rule).  With
 *      hz = (m(x-1,y) + m(x+1,y) + 1) >> 1     vt = (m(x,y-1) + m(x,y+1) + 1) >> 1
 *      cr = (the four edge neighbours + 2) >> 2     dg = (the four diagonal neighbours + 2) >> 2     c = m(x, y)
 *                                        R     G     B
 *      R site                            c     cr    dg
 *      B site                            dg    cr    c
 *      G site on an R row (b = 0)        hz    c     vt
 *      G site on a B row  (b = 1)        vt    c     hz
 *    - the classic bilinear demosaic.  Planes that are each constant come back unchanged.
 * 6. Identity.  A frame with sigma_q8[f] = 0 and bayer = -1 is copied - bit for bit where src_fmt == dst_fmt, else through its
 *    bytes.
 *
 * Asynchronous on `stream`, the stream the frames were written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  One kernel per
 * call, no atomics, no workspace.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, one of width /
 * height 0 or a size that breaks the rule, 3 * width * height of 2^32 and more, another format code, non-zero flags or
 * reserved, a range that is negative, NaN, infinite or above its bound (sigma_min, sigma_max, sigma_delta 4, blur_prob,
 * bayer_prob 1), sigma_min > sigma_max, pattern outside -1..3, no frame set, src[f] without dst[f] or the reverse, a
 * misaligned pointer (sources as the render calls ask: 16-byte float32, 4-byte uint8; destinations and both record arrays
 * 16-byte), a written range (destinations, recs_out) that overlaps any other range of the job - dst[f] == src[f] included -,
 * OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: noise between mosaic and demosaic (ofdg_photo's noise stays per element), any demosaicer but bilinear, white
 * balance, gamma, sharpening, depth of field by label, a sigma above 4 px, a pattern per frame, an in-place form.  Lens
 * distortion, lateral chromatic aberration and vignetting are ofdg_lens below: they move pixels, so they change the flow.
 * The flow, maps, labels, splat and reprojection planes are not touched.
 */
#define OFDG_CAMERA_MAX_SIGMA_Q8 1024  /* 4 px */
#define OFDG_CAMERA_MAX_RADIUS 12      /* taps on each side of the centre */
typedef struct ofdg_camera_rec {     /* 32 bytes; index [f] = frame 0 / 1 */
  int32_t sigma_q8[2];               /* 1 / 256 px, 0..1024 */
  int32_t bayer;                     /* -1: none; 0..3: the pattern */
  int32_t radius[2];                 /* written into recs_out, never read */
  int32_t reserved[3];
} ofdg_camera_rec;
struct ofdg_camera_job {             /* 112 bytes */
  const void* src[2]; void* dst[2];  /* image0, image1: [n,3,height,width]; each frame optional (src and dst both NULL) */
  const ofdg_camera_rec* recs;       /* DEVICE, n records, or NULL: drawn */
  ofdg_camera_rec*       recs_out;   /* DEVICE, n records, or NULL */
  long long first_index; uint32_t seed;
  int32_t width, height;             /* 0, 0: the context's frame */
  int32_t src_fmt, dst_fmt;          /* OFDG_FMT_F32 or OFDG_FMT_U8, independently */
  int32_t flags;                     /* no flag yet: must be 0 */
  int32_t pattern;                   /* of the draw: -1 drawn per sample, 0..3 fixed */
  float sigma_min, sigma_max, sigma_delta, blur_prob, bayer_prob;   /* ranges of the draw: <= 4, 4, 4 (px), 1, 1 */
  int32_t reserved;                  /* must be 0 */
};
int ofdg_camera(ofdg_ctx* ctx, const struct ofdg_camera_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes and records in host memory, no alignment asked of any
 * pointer.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above through
 * ofdg_host_last_error. */
int ofdg_host_camera(const struct ofdg_camera_job* job, int n_samples, int width, int height);
/* The drawn record of global sample `index` (step 1 alone: not sanitised; pure, no GPU).  Of `ranges` only the five ranges and
 * pattern are read.  OFDG_EINVAL (ofdg_host_last_error), `out` untouched, for a NULL pointer, a range that is negative, NaN,
 * infinite or above its bound, sigma_min > sigma_max or a pattern outside -1..3. */
int ofdg_camera_draw(uint32_t seed, long long index, const struct ofdg_camera_job* ranges, ofdg_camera_rec* out);
/* The tap table of step 3 for sigma_q8 in 1..1024 (pure, no GPU): out[0..R] the weights, out[R+1..12] zero.  OFDG_EINVAL
 * (ofdg_host_last_error) for out NULL or a sigma_q8 outside 1..1024. */
int ofdg_camera_taps(int sigma_q8, uint32_t out[13]);

/*
 * Lens: every output of a batch - frames, both flows, both occlusion maps, both label planes - bent by a one-parameter radial
 * distortion about a centre drawn per sample (ONE lens for both frames: it is one camera), the ground-truth flow carried
 * through it exactly, the frames with lateral chromatic aberration (B and R sampled at a slightly different magnification
 * than G) and vignetting, in ONE launch behind the call that wrote the planes.  The record is a pure function of (seed,
 * global sample index).  Everything below is exact: the kernel, ofdg_host_lens and the numpy restatement of the tests give
 * the same bits.  All arithmetic is IEEE, each operation rounded on its own (no contraction); fl64(.) / fl32(.) mark a
 * rounding where the text would otherwise leave it open.
 *
 * Planes: the eight planes, their order and their formats are ofdg_crop's (OFDG_CROP_IMAGE0 .. OFDG_CROP_LABEL1, image_fmt,
 * flow_fmt, occ_fmt).  src[k] and dst[k] are both [n,C,height,width]: the output has the source's size; a window is
 * ofdg_crop's or ofdg_spatial's business.  width = height = 0: the context's frame; otherwise any size the context's rule
 * allows (width a multiple of 8 and at least 8, height even and at least 2, no side above 2^20, W * H below 2^31).  Every
 * plane is optional on its own: src[k] and dst[k] both NULL.  There is no in-place form.
 *
 * Record (ofdg_lens_rec, 64 bytes): doubles k1, z, ca_b, ca_r, vig, cx, cy, then int32 reserved[2].  Per sample, in fp64:
 * hw = (W - 1) / 2.0, hh = (H - 1) / 2.0, inv = fl64(1 / fl64(fl64(hw * hw) + fl64(hh * hh))) - one over the squared
 * half-diagonal -, and the magnification of channel ch, zc = fl64(z * fl64(1 + ca)) with ca = ca_b for B, 0 for G, ca_r for R.
 * For destination pixel (X, Y):  dx = fl64(X - cx), dy = fl64(Y - cy), rho = fl64(fl64(fl64(dx * dx) + fl64(dy * dy)) * inv),
 * L = fl64(1 + fl64(k1 * rho)).  The source position under magnification m is
 *   qx = fl64(cx + fl64(fl64(m * L) * dx)),   qy = fl64(cy + fl64(fl64(m * L) * dy)).
 * The GEOMETRIC map S uses m = z; frames use m = zc of their channel.  k1 > 0 is barrel, k1 < 0 pincushion distortion.
 *
 * The record of sample i is recs[i] when recs is given, else ofdg_lens_draw(seed, first_index + i, ...).  Either way it is
 * sanitised before use, and the sanitised record is what recs_out[i] receives.  Sanitising: the record becomes the identity
 * {0, 1, 0, 0, 0, hw, hh} when an entry is not finite, or |k1| > 0.125, or z is outside [0.5, 2], or |ca_b| or |ca_r| exceeds
 * 1 / 64, or vig is outside [0, 0.5], or |fl64(cx - hw)| > hw / 4, or |fl64(cy - hh)| > hh / 4.  reserved = 0.  No record
 * makes the kernel touch memory outside a plane.
 *
 * Taps: ofdg_spatial's, word for word, from (qx, qy) - 24.8 fixed point Qx, Qy with the same clamps, "inside" (decided on the
 * geometric map), the four clamped bilinear taps, the nearest tap.
 *
 * Frames: each channel is interpolated at its own zc position by ofdg_spatial's bilinear expression (exact on byte values);
 * the result v is multiplied by the vignette of the DESTINATION pixel, gain = (float)fl64(1 - fl64(vig * rho)) - positive for
 * every sanitised record, rho <= 1.5625 given the centre limit -: v' = fl32(v * gain).  float32 stores v' (a NaN as
 * 0x7FC00000); uint8 stores rintf(v') clamped to [0, 255] (ties to even, a NaN becomes 0).  With vig == 0 the multiplication
 * is left out, so the identity record moves bytes only.
 *
 * Flow, at destination pixel (X, Y) of frame 0: (u, v) is the source flow at the NEAREST tap of S, widened to float32.  The
 * target is tx = fl64(qx + (double)u), ty likewise, (qx, qy) of S.  The new flow needs P with S(P) = t.  Write P = c + s (t -
 * c): dtx = fl64(tx - cx), dty likewise, ru = fl64(fl64(fl64(dtx * dtx) + fl64(dty * dty)) * inv), and s solves
 * z s (1 + k1 ru s^2) = 1.
 *   k1 == 0:  s = fl64(1 / z), and the pixel counts as solved.
 *   k1 != 0 and ru <= 16 does not hold (a NaN does not):  the pixel is UNSOLVABLE.
 *   otherwise s = fl64(1 / z), then exactly 8 Newton steps
 *       a = fl64(fl64(ru * s) * s)
 *       g = fl64(fl64(fl64(z * s) * fl64(1 + fl64(k1 * a))) - 1)
 *       d = fl64(z * fl64(1 + fl64(fl64(3 * k1) * a)))
 *       s = fl64(s - fl64(g / d))
 *   then a, g and D = fl64(1 + fl64(fl64(3 * k1) * a)) once more from the final s; solved when |g| <= 2^-30 && D >= 0.25 && s >
 *   0, else unsolvable.
 * Solved: px = fl64(cx + fl64(s * dtx)), py likewise; u' = (float)fl64(px - X), v' = (float)fl64(py - Y) (a NaN as
 * 0x7FC00000); binary16 is rounded once after that.  Unsolvable: both components are the canonical NaN (0x7FC00000 / 0x7E00),
 * which the statistics and the pyramid leave out.  flow1 is the same from its own plane, through the same S.
 * Why this is well defined (checked in numpy over 2 10^6 random (k1, z, ru) of the ranges above): for k1 > 0 the function is
 * convex and the start lies right of the root, for k1 < 0 it is concave and the start - the first Newton step from 0 - lies
 * left of it, so the iteration is monotone; 6 steps decide every case as 60 do, 8 is the margin.  D >= 0.25 keeps away from
 * the fold of the pincushion branch (a = 1 / (3 |k1|)); a solution with a <= 1 / (4 |k1|) exists for every target inside the
 * destination frame: 2 at |k1| = 0.125, against at most 1.5625 for an in-frame pixel given the centre limit.
 *
 * Labels: the element at the nearest tap of S.
 *
 * Occlusion maps: the element becomes 1.0f / 1 when the source element at the nearest tap of S is non-zero (the crop's rule),
 * or the pixel is not inside, or that frame's flow plane is given and the pixel is unsolvable, or - with
 * OFDG_LENS_OCC_WINDOW - floor(fl64(px + 0.5)) lies outside [0, W - 1] or floor(fl64(py + 0.5)) outside [0, H - 1] (a NaN is
 * outside).  Otherwise it becomes +0.0f / 0.  OFDG_LENS_OCC_WINDOW needs the flow plane, as the spatial flag does.
 *
 * Draw (ofdg_lens_draw; pure, no GPU): Philox4x32-10 (ofdg_crop_philox) under the counter sampler's key of global index g,
 * blocks j = 0, 1 at the counters {j, 0, 0x0c7a, 0} (0x0c70 .. 0x0c79 and 0x0fd9 are taken); u(w) and sym(w, a) are
 * ofdg_photo's.
 *   block 0:  on = u(.x) < prob   k1 = sym(.y, k1_range)   ca_b = sym(.z, ca_range)   ca_r = sym(.w, ca_range)
 *   block 1:  vig = fl32(u(.x) * vig_max)   ox = sym(.y, centre)   oy = sym(.z, centre)
 * The record widens each float to double; cx = fl64(hw + fl64((double)ox * hw)), cy likewise with oy and hh.  z with
 * OFDG_LENS_FILL: rc = the largest rho (as above, about (cx, cy)) of the four frame corners, Lc = fl64(1 + fl64(k1 * rc)), z =
 * Lc > 1 ? fl64(1 / Lc) : 1 - with it every destination pixel is inside: for k1 > 0 L grows with rho, so the farthest corner
 * is the worst pixel; for k1 <= 0 sources move inward.  Without the flag z = 1.  When !on the record is the identity.  Ranges
 * and their limits: prob in [0, 1], k1_range <= 0.125, ca_range <= 1 / 64, vig_max <= 0.5, centre <= 0.25, none negative or
 * NaN; they are checked even when records are given.  All ranges 0, or prob = 0, give the identity.
 *
 * Identity: under the identity record every destination plane has the source's bytes and a flow keeps its bits - for every
 * finite flow below 2^20 px, qx = X exactly, s = 1, and cx + (t - cx) is exact -; a NaN flow is stored as the canonical NaN.
 *
 * Asynchronous on `stream`, the stream the planes were written on; OFDG_STREAM_OWN as in ofdg_crop.  One kernel for any
 * n_samples, all planes and both frames, no atomics; it reads no record of the context.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, only one of
 * width / height 0, a size that breaks the rule above, unknown flag bits, non-zero reserved, another format code, a range
 * outside its limits, no plane set, src[k] without dst[k] or the reverse, OFDG_LENS_OCC_WINDOW with occ0 but no flow (occ1 /
 * flow1 likewise), a misaligned pointer (sources as the render calls ask: 16-byte float32, 8-byte binary16, 4-byte uint8;
 * destinations and both record arrays 16-byte), a destination range (recs_out included) that overlaps any other range of the
 * job, OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: higher radial terms or tangential distortion, a lens per frame, longitudinal aberration, interpolated flow,
 * mapping the object table's boxes, a changed output size, an in-place form, vignetting other than linear in rho.
 */
#define OFDG_LENS_FILL         1   /* job flag: the drawn z keeps every destination pixel inside */
#define OFDG_LENS_OCC_WINDOW  16   /* job flag: see "occlusion maps" above                        */
typedef struct ofdg_lens_rec {           /* 64 bytes */
  double k1, z, ca_b, ca_r, vig, cx, cy;
  int32_t reserved[2];
} ofdg_lens_rec;
struct ofdg_lens_job {                   /* 208 bytes */
  const void* src[OFDG_CROP_PLANES];     /* [n,C,height,width], or NULL                */
  void*       dst[OFDG_CROP_PLANES];     /* the same shape and element type            */
  const ofdg_lens_rec* recs;             /* DEVICE, n records, or NULL: drawn          */
  ofdg_lens_rec*       recs_out;         /* DEVICE, n records, or NULL                 */
  long long first_index;  uint32_t seed;
  int32_t width, height;                 /* 0, 0: the context's frame                  */
  int32_t flags, image_fmt, flow_fmt, occ_fmt;
  int32_t reserved;                      /* must be 0 */
  float prob, k1_range, ca_range, vig_max, centre;        /* ranges of the draw: <= 1, 0.125, 1 / 64, 0.5, 0.25 */
};
int ofdg_lens(ofdg_ctx* ctx, const struct ofdg_lens_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes [n,C,height,width], records in host memory, no
 * alignment asked of any pointer.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above
 * through ofdg_host_last_error. */
int ofdg_host_lens(const struct ofdg_lens_job* job, int n_samples, int width, int height);
/* The drawn record of global sample `index` (the draw alone: not sanitised; pure, no GPU).  Of `ranges` the five ranges, flags,
 * width and height are read; the size must be set.  OFDG_EINVAL (ofdg_host_last_error), `out` untouched, for a NULL pointer,
 * a size that breaks the rule, unknown flag bits or a range ofdg_lens refuses. */
int ofdg_lens_draw(uint32_t seed, long long index, const struct ofdg_lens_job* ranges, ofdg_lens_rec* out);

/*
 * Block compression: what a baseline JFIF encoder followed by a decoder leaves in the pixels of image0 and / or image1 of a
 * batch - 8x8 blocking, ringing at edges, chroma coarser than luma -, each sample by a record of its own.  It is the last
 * physical step of the chain, behind the sensor noise and the colour response (ofdg_photo, ofdg_jitter): almost every real frame
 * a flow network sees has been compressed.  This is NOT a codec: there is no entropy coding, no bit stream and no file.  The
 * record is a pure function of (seed, global sample index).  Everything below is 32-bit integers on bytes (the largest
 * intermediate over the extreme blocks is below 2^28; >> on a negative value is arithmetic): the kernel, ofdg_host_jpeg and the
 * numpy restatement of the tests give the same bytes.
 *
 * Planes, formats, sizes, the byte of a float32 element and alignment as in ofdg_camera: src[f] is image f as
 * [n,3,height,width] planar B, G, R of src_fmt, dst[f] the same shape of dst_fmt; OFDG_FMT_F32 or OFDG_FMT_U8, chosen
 * independently.  A frame is present when both its pointers are given.  width = height = 0: the context's frame; otherwise any
 * size the context's rule allows.  There IS an in-place form: dst[f] == src[f] is allowed when src_fmt == dst_fmt (a
 * workgroup owns whole MCUs, reads all it needs and writes behind a barrier; see step 5).  It reads no record of the context
 * and works in every mode.
 *
 * Record of sample i: recs[i] (DEVICE memory) when recs is given, else ofdg_jpeg_draw(seed, first_index + i, the job's ranges).
 * Either way it is sanitised before use, and the sanitised record is what recs_out[i] receives.
 *
 * 1. Draw.  Philox4x32-10 (ofdg_crop_philox) under the counter sampler's key of global index g, blocks j = 0, 1 at the counters
 *    {j, 0, 0x0c7b, 0} (taken: 0x0c70 .. 0x0c7a and 0x0fd9, see ofdg_jitter).  u() and isym() as in ofdg_jitter.
 *      block 0:  on  = u(.x) < prob
 *                q0  = quality_min + (int)(((uint64).y * (uint32)(quality_max - quality_min + 1)) >> 32)
 *                q1  = clamp(q0 + isym(.z, quality_delta), 1, 100)
 *                sub = subsample >= 0 ? subsample : (u(.w) < sub_prob)
 *      block 1:  phase_x = .x >> 28, phase_y = .y >> 28 when OFDG_JPEG_PHASE is set, else 0
 *    quality = on ? {q0, q1} : {0, 0};  subsample = sub;  reserved = 0.
 * 2. Sanitise.  quality clamps to [0, 100]; a subsample other than 0 / 1 becomes 0; a phase outside 0..15 becomes 0;
 *    reserved = 0.
 * 3. Tables.  T.81 Annex K, Table K.1 (luminance) and K.2 (chrominance), as literals, under libjpeg's rule:
 *      scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;   Q = clamp((base * scale + 50) / 100, 1, 255)
 *    ofdg_jpeg_tables exports them; Pillow reports exactly these at quality 10, 50 and 90.
 * 4. Colour, on the bytes, with libjpeg's 16-bit constants (each row sums to 65536 or 0):
 *      Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *      Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *      Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 * 5. Geometry.  The plane is extended by replicating its edge on all four sides: coordinates are clamped.  The grid's origin
 *    is (-phase_x, -phase_y) (4:4:4 uses phase & 7).  An MCU is 8x8 (4:4:4) or 16x16 (4:2:0: four Y blocks, one Cb, one Cr);
 *    every MCU that meets the plane is processed, only pixels inside the plane are written.  4:2:0: a chroma sample is (the
 *    four of its 2x2 cell + 2) >> 2, and on the way back each chroma sample is repeated over its cell.  A clamped coordinate of
 *    an MCU always lands in that MCU's own part of the plane - that is what makes the in-place form sound.
 * 6. Block, for p = sample - 128 and Q of step 3, with T[u][x] = lrint(4096 s(u) cos((2 x + 1) u pi / 16)), s(0) = 1 / sqrt 2,
 *    else 1, as a literal (magnitudes 2896 and 4017, 3784, 3406, 2896, 2276, 1567, 799):
 *      A[y][u] = sum_x T[u][x] p[y][x]      A1 = (A + 256) >> 9
 *      F[v][u] = sum_y T[v][y] A1[y][u]     2^17 times the orthonormal coefficient
 *      level   = sign(F) * ((|F| + Q * 65536) / (Q * 131072))      D = level * Q
 *      B[y][u] = sum_v T[v][y] D[v][u]      B1 = (B + 256) >> 9
 *      P[y][x] = sum_u T[u][x] B1[y][u]     out = clamp(((P + 65536) >> 17) + 128, 0, 255)
 *    Against the orthonormal float64 DCT with round-half-away quantisation a level is off by at most 1 and under 3 % of them
 *    are; where all levels of a block agree every byte is within 1 (tests/test_jpeg.py).
 * 7. Back, with cb = Cb - 128 and cr = Cr - 128, each clamped to a byte:
 *      R = Y + ((91881 cr + 32768) >> 16)
 *      G = Y + ((-22554 cb - 46802 cr + 32768) >> 16)
 *      B = Y + ((116130 cb + 32768) >> 16)
 *    A uint8 destination stores the byte, a float32 one (float)byte.
 * 8. Identity.  A frame with quality[f] = 0 is copied - bit for bit where src_fmt == dst_fmt, else through its bytes; in place
 *    it is left untouched.  Quality 100 is NOT the identity: every Q is 1, yet the colour transform and the roundings of the
 *    passes remain (a grey plane, B = G = R, does come back exactly at quality 100).
 *
 * Asynchronous on `stream`, the stream the frames were written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  One kernel per
 * call, no atomics, no workspace.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, one of width /
 * height 0 or a size that breaks the rule, 3 * width * height of 2^32 and more, another format code, flags other than 0 /
 * OFDG_JPEG_PHASE, non-zero reserved, quality_min / quality_max outside 1..100 or min > max, quality_delta outside 0..99, prob
 * / sub_prob negative, NaN, infinite or above 1, subsample outside -1..1 (the ranges are checked even when records are given),
 * no frame set, src[f] without dst[f] or the reverse, a misaligned pointer (sources as the render calls ask: 16-byte float32,
 * 4-byte uint8; destinations and both record arrays 16-byte), a written range (destinations, recs_out) that overlaps any other
 * range of the job - dst[f] == src[f] with src_fmt != dst_fmt and every partial overlap included, dst[f] == src[f] in one
 * format excepted -, OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: an entropy coder, a bit stream or a file size; triangle ("fancy") chroma upsampling across blocks - which is why
 * 4:2:0 differs from libjpeg-turbo's decoder by several bytes on saturated edges, and which would end the in-place form -;
 * 4:2:2 and other samplings; custom tables; progressive, arithmetic or 12-bit modes; deblocking filters and video codecs'
 * inter-frame prediction; a quality per channel; compression of flow, maps, labels, splat or reprojection planes; packing of
 * the records.
 */
#define OFDG_JPEG_PHASE 1            /* flags: the block grid's phase is drawn; without it the grid starts at (0, 0) */
typedef struct ofdg_jpeg_rec {       /* 32 bytes; index [f] = frame 0 / 1 */
  int32_t quality[2];                /* 0: frame f is not compressed; 1..100: libjpeg's quality */
  int32_t subsample;                 /* 0: 4:4:4;  1: 4:2:0 */
  int32_t phase_x, phase_y;          /* 0..15: the grid's origin is (-phase_x, -phase_y); 4:4:4 uses phase & 7 */
  int32_t reserved[3];
} ofdg_jpeg_rec;
struct ofdg_jpeg_job {               /* 112 bytes */
  const void* src[2]; void* dst[2];  /* as ofdg_camera; dst[f] == src[f] IS allowed when src_fmt == dst_fmt (in place) */
  const ofdg_jpeg_rec* recs;         /* DEVICE, n records, or NULL: drawn */
  ofdg_jpeg_rec*       recs_out;     /* DEVICE, n records, or NULL */
  long long first_index; uint32_t seed;
  int32_t width, height;             /* 0, 0: the context's frame */
  int32_t src_fmt, dst_fmt;          /* OFDG_FMT_F32 or OFDG_FMT_U8, independently */
  int32_t flags;                     /* 0 or OFDG_JPEG_PHASE */
  int32_t subsample;                 /* of the draw: -1 drawn per sample, 0 / 1 fixed */
  int32_t quality_min, quality_max, quality_delta;   /* 1..100, min <= max; delta 0..99 */
  float prob, sub_prob;              /* 0..1 */
  int32_t reserved[2];               /* must be 0 */
};
int ofdg_jpeg(ofdg_ctx* ctx, const struct ofdg_jpeg_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition block by block: planes and records in host memory, no alignment asked of any
 * pointer.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above through
 * ofdg_host_last_error. */
int ofdg_host_jpeg(const struct ofdg_jpeg_job* job, int n_samples, int width, int height);
/* The drawn record of global sample `index` (step 1 alone: not sanitised; pure, no GPU).  Of `ranges` only the five ranges,
 * subsample and flags are read.  OFDG_EINVAL (ofdg_host_last_error), `out` untouched, for a NULL pointer or a range, subsample
 * or flags ofdg_jpeg refuses. */
int ofdg_jpeg_draw(uint32_t seed, long long index, const struct ofdg_jpeg_job* ranges, ofdg_jpeg_rec* out);
/* The tables of step 3 for a quality in 1..100 (pure, no GPU), row-major [v][u].  OFDG_EINVAL (ofdg_host_last_error) for a NULL
 * pointer or a quality outside 1..100. */
int ofdg_jpeg_tables(int quality, uint16_t luma[64], uint16_t chroma[64]);
/* Steps 4-6 on one block (pure, no GPU): `in` the 64 samples row-major [y][x], q the table (each entry 1..255), levels the
 * quantised coefficients [v][u] (may be NULL), out the decoded samples.  OFDG_EINVAL for a NULL in, q or out, or an entry of q
 * outside 1..255. */
int ofdg_host_jpeg_block(const uint8_t in[64], const uint16_t q[64], int32_t levels[64], uint8_t out[64]);

/*
 * Flow visualisation: the Middlebury colour wheel (Baker et al., "A Database and Evaluation Methodology for Optical Flow") of
 * any [n,2,height,width] flow tensor - the forward flow, flow1, a cropped, warped or splat flow, a residual - as a uint8
 * picture: the direction is the hue, the length the saturation, zero flow white.  Behind the producing call on the same
 * stream, so that a ready picture and no float plane goes to an image writer.  Everything below is integers behind one
 * rounding of each flow component: the kernels, ofdg_host_flow_vis and the numpy restatement of the tests give the same bytes.
 * >> is the arithmetic shift; divisions are floored, on non-negative operands.
 *
 * flow: [n,2,height,width] of flow_fmt, OFDG_FMT_F32 (16-byte aligned) or OFDG_FMT_F16 (8-byte).  occ: NULL, or the
 * [n,1,height,width] map of occ_fmt that goes with it, OFDG_FMT_U8 (4-byte) or OFDG_FMT_F32 (16-byte), as in ofdg_flow_stats;
 * read only under OFDG_VIS_DIM_OCC.  dst: 16-byte aligned, [n,3,height,width] (OFDG_VIS_PLANAR_BGR) or [n,height,width,3]
 * (OFDG_VIS_HWC_RGB).  width = height = 0: the context's frame; otherwise width a multiple of 8 and at least 8, height even
 * and at least 2.
 *
 * 1. Usable.  u, v are widened to float32.  The pixel is usable when fabsf(u) < 1048576.0f && fabsf(v) < 1048576.0f (rule 2
 *    of ofdg_flow_stats).  An unusable pixel is written as (0, 0, 0) and takes no part in any maximum.
 * 2. Fixed point.  U = (int)rintf(u * 256.0f), V likewise (to nearest even; |U| <= 2^28).  R2 = U U + V V in 64 bits.
 *    Rq = isqrt(R2) (floor).
 * 3. Scale M (Q8 pixels).  OFDG_VIS_NORM_FIXED: M = (int)lrintf(max_flow * 256.0f).  OFDG_VIS_NORM_SAMPLE: M = max(1,
 *    isqrt(the largest R2 of the sample's usable pixels)), occluded ones included.  OFDG_VIS_NORM_BATCH: the same over all
 *    n_samples.  rows_out[i] = { that largest R2 (0 under FIXED: none is taken), M, 0 }.
 * 4. Radius.  rho = min((Rq << 16) / M, 65537), in 64 bits.
 * 5. Angle, as a turn fraction in Q16: the angle of (u, v) with y pointing down, which is what Middlebury's
 *    atan2(-v, -u) / pi mapped to [0, 1] is.  ax = |U|, ay = |V|, mx = max(ax, ay), mn = min(ax, ay);
 *    t = mx ? (mn << 16) / mx : 0 (0..65536);  i = t >> 8, fr = t & 255;
 *    a24 = A[i] + (((A[min(i + 1, 256)] - A[i]) fr + 128) >> 8);  o = (a24 + 128) >> 8 (0..8192);
 *    b = ax >= ay ? o : 16384 - o;  U < 0: b = 32768 - b;  V < 0: b = (65536 - b) & 65535.
 *    A[k] = lrint(atan(k / 256) / (2 pi) 2^24), k = 0..256, a literal table (A[1] = 10430, A[128] = 1238021,
 *    A[255] = 2091927, A[256] = 2097152; the 257 entries sum to 301013384).
 * 6. Wheel: the 55 entries (R, G, B) of Baker et al., a literal table too (its 165 bytes sum to 21038, entry 54 is
 *    (255, 0, 43)); i counts from 0 within a segment:
 *      RY, 15 entries: (255, 255 i / 15, 0)        YG, 6: (255 - 255 i / 6, 255, 0)      GC, 4: (0, 255, 255 i / 4)
 *      CB, 11: (0, 255 - 255 i / 11, 255)          BM, 13: (255 i / 13, 0, 255)          MR, 6: (255, 0, 255 - 255 i / 6)
 *    fk = 54 b, k0 = fk >> 16 (0..53), f = fk & 65535;  per channel c16 = wheel[k0][c] (65536 - f) + wheel[k0 + 1][c] f.
 *    The seam between entry 54 and entry 0 is Middlebury's own and is kept.
 * 7. Colour.  rho <= 65536: out = (int)(((16711680 << 16) - rho (16711680 - c16)) >> 32), in 64 bits - zero flow is white,
 *    radius 1 the pure wheel colour, floored as Middlebury floors.  rho > 65536: out = (3 c16) >> 18, Middlebury's 0.75 for
 *    vectors out of range.
 * 8. Dimming.  With OFDG_VIS_DIM_OCC and occ != 0: out >>= 1.  A float32 map is compared with != 0.0f; a NaN counts as
 *    occluded.
 * With max_flow = 8, as (R, G, B): (8, 0) is (255, 0, 0), (0, 8) (255, 229, 0), (-8, 0) (0, 209, 255), (0, -8) (88, 0, 255),
 * (0, 0) (255, 255, 255), (8, 8) - out of range - (191, 86, 0), (-8, 8) (24, 191, 0).  Against the float code of the paper a
 * channel differs by at most 1 away from radius 1 and from the wheel's seam, the two places where the code itself jumps
 * (DESIGN.md).
 *
 * work: DEVICE memory of n_samples * OFDG_FLOW_VIS_WORK_BYTES, 16-byte aligned, contents unspecified before and after (the
 * call clears it); required unless norm is FIXED, which does not look at it.  Asynchronous on `stream`, the stream the flow
 * was written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  At most one clearing of `work` and two kernels per call (FIXED: one
 * kernel); the only atomic is a 64-bit integer maximum; it reads no record of the context and works in every mode.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, flow or dst, n_samples < 1, a
 * size that breaks the rule, 3 * width * height of 2^32 and more, another format, layout or norm code, unknown flag bits, a
 * non-zero reserved field, OFDG_VIS_DIM_OCC without occ, max_flow NaN or outside [2^-8, 2^20] under FIXED, work NULL where
 * it is required, a misaligned pointer (rows_out: 16-byte), a written range (dst, work, rows_out) that overlaps any other
 * range of the job, OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: arrows and quiver plots, an HSV (OpenCV-style) code, error maps against a second flow, percentile
 * normalisation, a float output, montages with the frames, an in-place form.
 */
#define OFDG_VIS_PLANAR_BGR 0   /* dst [n,3,height,width] uint8, planes B, G, R: the frames' own layout */
#define OFDG_VIS_HWC_RGB    1   /* dst [n,height,width,3] uint8, R, G, B: what image writers and TensorBoard take */
#define OFDG_VIS_NORM_FIXED  0  /* radius 1 is max_flow pixels */
#define OFDG_VIS_NORM_SAMPLE 1  /* radius 1 is the sample's own largest usable displacement */
#define OFDG_VIS_NORM_BATCH  2  /* ... the largest of the whole call */
#define OFDG_VIS_DIM_OCC 1      /* flag: pixels with occ != 0 at half brightness; occ required */
#define OFDG_FLOW_VIS_WORK_BYTES 8   /* of job->work per sample */
typedef struct ofdg_flow_vis_row { uint64_t max_r2_q16; uint32_t scale_q8; uint32_t reserved; } ofdg_flow_vis_row;  /* 16 bytes */
struct ofdg_flow_vis_job {       /* 96 bytes */
  const void* flow;              /* [n,2,height,width], OFDG_FMT_F32 (16-byte aligned) or OFDG_FMT_F16 (8-byte) */
  const void* occ;               /* NULL, or [n,1,height,width] OFDG_FMT_U8 (4-byte) / OFDG_FMT_F32 (16-byte), as in ofdg_flow_stats */
  void* dst;                     /* 16-byte aligned */
  ofdg_flow_vis_row* rows_out;   /* DEVICE, n rows, or NULL */
  void* work;                    /* DEVICE, n * OFDG_FLOW_VIS_WORK_BYTES, 16-byte aligned; required unless norm is FIXED */
  int32_t width, height, flow_fmt, occ_fmt, layout, norm, flags, reserved;
  float max_flow;                /* NORM_FIXED only: in [2^-8, 2^20]; otherwise not looked at */
  int32_t reserved2[5];
};
int ofdg_flow_vis(ofdg_ctx* ctx, const struct ofdg_flow_vis_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes and rows in host memory, no alignment asked of any
 * pointer, work not looked at.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above
 * through ofdg_host_last_error. */
int ofdg_host_flow_vis(const struct ofdg_flow_vis_job* job, int n_samples, int width, int height);
/* The two constant tables of steps 5 and 6, copied out (pure, no GPU).  OFDG_EINVAL for a NULL pointer. */
int ofdg_host_flow_vis_tables(int32_t atan_q24[257], uint8_t wheel_rgb[55][3]);

/*
 * Flow error: the end-point error (EPE) of an estimated flow against the ground truth, split the way Sintel and KITTI report
 * it - matched / unmatched pixels by the occlusion map, three bands of ground-truth speed, three bands of distance to the next
 * motion boundary (the dist2 plane of ofdg_boundaries) -, with the 1 / 3 / 5 px and KITTI Fl outlier counts, a histogram of
 * the error, the worst pixel, and optionally the error as a plane and as the KITTI devkit's colour picture.  Behind the call
 * that made the ground truth, on the same stream.  Everything below is integers behind one rounding of each flow component:
 * the kernel, ofdg_host_flow_error and the numpy restatement of the tests give the same bytes, and the rows are the same bits
 * on every run, so that curves compare across runs and ranks and an epoch accumulates on the device.
 *
 * gt: [n,2,height,width] of gt_fmt, OFDG_FMT_F32 (16-byte aligned) or OFDG_FMT_F16 (8-byte).  est: the same shape of est_fmt,
 * OFDG_FMT_F32 (16-byte), OFDG_FMT_F16 or OFDG_FMT_BF16 (8-byte).  occ: NULL, or the [n,1,height,width] map of occ_fmt,
 * OFDG_FMT_U8 (4-byte) or OFDG_FMT_F32 (16-byte), as in ofdg_flow_stats.  dist2: NULL, or the uint8 [n,1,height,width] dist2
 * plane of ofdg_boundaries of this flow (4-byte).  At least one of rows, epe and picture is set.  width = height = 0: the
 * context's frame; otherwise width a multiple of 8 and at least 8, height even and at least 2.
 *
 * A pixel is (x, y) of sample i; idx = y * width + x, under OFDG_ERR_ONE_ROW idx = (i * height + y) * width + x.
 * 1. Widen and scale.  ug, vg are widened to float32.  The components of est are widened to float32 (exact for binary16 and
 *    bfloat16), then each is fl32(e * est_scale).
 * 2. Unusable ground truth.  Not (fabsf(ug) < 1048576.0f && fabsf(vg) < 1048576.0f): n_bad_gt += 1 and nothing else (rule 2
 *    of ofdg_flow_stats: NaN, +-inf, an overflowed half).
 * 3. Unusable estimate.  Otherwise, the scaled estimate fails the same test: n_bad_est += 1 and nothing else - a diverged
 *    network is a count, not NaN metrics.
 * 4. An unusable pixel of either kind writes epe = -1 and the picture (0, 0, 0).
 * 5. Fixed point.  Ug = (int)rintf(ug * 256.0f), likewise Vg, Ue, Ve (|.| <= 2^28).  E2 = (Ue - Ug)^2 + (Ve - Vg)^2 in 64
 *    bits, Eq = isqrt(E2) (floor; Q8 pixels, below 2^30).  G2 = Ug^2 + Vg^2, Gq = isqrt(G2).
 * 6. Cell.  hidden = 1 when occ is given and occ != 0, else 0 (a float32 map is compared with != 0.0f; a NaN counts as
 *    hidden).  Speed band: the number of k in {0, 1} with Gq >= S_k, S_k = lrintf(speed_px[k] * 256.0f).  Distance band: the
 *    number of k in {0, 1} with dist2 >= dist2_edge[k]; without a dist2 plane band 0.  OFDG_BND_FAR is in the last band.
 * 7. cell[hidden][speed][distance]: n += 1, sum_epe_q8 += Eq, n_1px += (Eq > 256), n_3px += (Eq > 768), n_5px += (Eq > 1280),
 *    n_fl += (Eq > 768 && 20 Eq > Gq) - KITTI's Fl outlier: more than 3 px and more than 5 % of the true length.
 * 8. Row.  hist[b] += 1, b the number of k in 0..14 with Eq >= (16 << k) (edges 1/16, 1/8, ... 1024 px);
 *    max_key = max(max_key, ((uint64)Eq << 32) | (0xFFFFFFFFu - idx)): the worst pixel, the first of equals.  max_key == 0:
 *    nothing was counted.
 * 9. epe.  OFDG_FMT_F32: fl32((float)Eq * 0.00390625f), the conversion to nearest even; OFDG_FMT_F16: that float32 rounded once
 *    to nearest even (inf above 65504).
 * 10. picture, the KITTI devkit's error colours.  bin = the number of j in 0..8 with Eq >= (48 << j) && 320 Eq >= (Gq << j), in
 *    64 bits - the devkit's min(E / 3, 20 E / |gt|) against its edges 1/16 ... 16; Gq = 0 leaves E / 3 alone.  (R, G, B) of
 *    bins 0..9, a literal table whose 30 bytes sum to 4523: (49,54,149) (69,117,180) (116,173,209) (171,217,233) (224,243,248)
 *    (254,224,144) (253,174,97) (244,109,67) (215,48,39) (165,0,38).  With OFDG_ERR_DIM_OCC and a hidden pixel every channel
 *    is shifted right by 1.  A pixel is an Fl outlier exactly when its bin is 5 or more, except at equality on an edge: Fl
 *    is strict, the bins are not.
 * With est_scale 1: gt (10, 0), est (10, 0) is Eq 0, bin 0; gt (0, 0), est (3, 0) Eq 768, bin 5, no outlier, not in n_3px;
 * gt (100, 0), est (104, 0) Eq 1024, bin 4, in n_3px, not in n_fl; gt (100, 0), est (106, 0) in n_fl, bin 5.  Eq / 256 is
 * within 2.5 / 256 px of the float64 EPE of the same inputs.
 *
 * Without OFDG_ERR_ACCUMULATE the call first writes every byte of its rows as zero on `stream`, then reduces; with it the rows
 * are added to (the key: the maximum), and an all-zero row is the identity.  Asynchronous on `stream`; OFDG_STREAM_OWN as in
 * ofdg_flow_stats.  At most one clearing and one kernel; integer atomics only, so no bit depends on arrival order.  It reads
 * no record of the context and works in every mode.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, gt or est; no output set;
 * n_samples < 1; a size that breaks the rule; 3 * width * height of 2^32 and more; OFDG_ERR_ONE_ROW with n * height * width of
 * 2^32 and more; another gt_fmt, est_fmt, occ_fmt (where occ is set), epe_fmt (where epe is set), layout or flag bit; a
 * non-zero reserved field; OFDG_ERR_DIM_OCC without occ or without picture; est_scale NaN or |est_scale| outside [2^-10,
 * 2^10]; speed_px not 0 < speed_px[0] <= speed_px[1] <= 2^20 (a NaN fails); where dist2 is set, dist2_edge not 1 <=
 * dist2_edge[0] <= dist2_edge[1] <= 255; a misaligned pointer (rows: 8-byte; epe, picture: 16-byte); a written range (rows,
 * epe, picture) that overlaps any other range of the job; OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: an estimate at another resolution, angular error, an outlier mask plane, radii above 15 for the distance
 * bands (the limit of ofdg_boundaries), percentiles, flow1's estimate in the same call, packing these planes, an in-place
 * form.
 */
#define OFDG_ERR_ACCUMULATE 1   /* add to the rows instead of overwriting them (max for the key) */
#define OFDG_ERR_ONE_ROW    2   /* all n samples reduce into rows[0] */
#define OFDG_ERR_DIM_OCC    4   /* picture: pixels with occ != 0 at half brightness, as the KITTI devkit draws them; occ required */
#define OFDG_FLOW_ERROR_HIST_BINS 16
typedef struct ofdg_flow_error_cell { uint64_t sum_epe_q8; uint32_t n, n_1px, n_3px, n_5px, n_fl, reserved; } ofdg_flow_error_cell;  /* 32 bytes */
typedef struct ofdg_flow_error_row {      /* 672 bytes, no padding, 8-byte aligned */
  ofdg_flow_error_cell cell[2][3][3];     /* [hidden][speed band][distance band] */
  uint32_t hist[OFDG_FLOW_ERROR_HIST_BINS];
  uint64_t max_key;
  uint32_t n_bad_gt, n_bad_est;
  uint32_t reserved[4];
} ofdg_flow_error_row;
struct ofdg_flow_error_job {              /* 128 bytes */
  const void* gt;                         /* [n,2,H,W], gt_fmt: OFDG_FMT_F32 (16-byte aligned) or OFDG_FMT_F16 (8-byte) */
  const void* est;                        /* [n,2,H,W], est_fmt: OFDG_FMT_F32, OFDG_FMT_F16 or OFDG_FMT_BF16 (what autocast nets emit) */
  const void* occ;                        /* NULL, or [n,1,H,W], occ_fmt OFDG_FMT_U8 (4-byte) / OFDG_FMT_F32 (16-byte), as in ofdg_flow_stats */
  const uint8_t* dist2;                   /* NULL, or [n,1,H,W] uint8: the dist2 plane of ofdg_boundaries for this flow (4-byte) */
  ofdg_flow_error_row* rows;              /* DEVICE, n rows (one with ONE_ROW), 8-byte aligned, or NULL */
  void* epe;                              /* NULL, or [n,1,H,W] of epe_fmt OFDG_FMT_F32 / OFDG_FMT_F16, 16-byte aligned */
  void* picture;                          /* NULL, or uint8 [n,3,H,W] (OFDG_VIS_PLANAR_BGR) / [n,H,W,3] (OFDG_VIS_HWC_RGB), 16-byte aligned */
  int32_t width, height, gt_fmt, est_fmt, occ_fmt, epe_fmt, layout, flags;
  float   est_scale;                      /* the estimate is multiplied by it first (networks that predict flow / 20); 1.0f: as is */
  float   speed_px[2];                    /* edges of the speed bands, pixels */
  int32_t dist2_edge[2];                  /* edges of the distance bands, in units of dist2 */
  int32_t reserved[5];
};
int ofdg_flow_error(ofdg_ctx* ctx, const struct ofdg_flow_error_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes and rows in host memory, no alignment asked of any
 * pointer.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above through
 * ofdg_host_last_error. */
int ofdg_host_flow_error(const struct ofdg_flow_error_job* job, int n_samples, int width, int height);
/* The colour table of step 10 as (R, G, B), copied out (pure, no GPU).  OFDG_EINVAL for a NULL pointer. */
int ofdg_host_flow_error_colours(uint8_t rgb[10][3]);

/*
 * Motion blur: every pixel of image0 and / or image1 becomes a weighted mean of its frame along a short segment through the
 * pixel, whose direction and length are the pixel's own flow times the sample's shutter - the fraction of the inter-frame
 * interval the exposure lasts.  The exposure is centred on the frame's instant, so the segment is symmetric about the pixel
 * and the sign of the flow does not matter: flow1 serves frame 1 as it is.  Flow, occlusion maps and labels are not touched:
 * the ground truth is the motion of the sharp frames.  NOT in place (a pixel reads its neighbours).  The record is a pure
 * function of (seed, global sample index), so a resumed or sharded run makes the same pixels.  Everything is integers once
 * the half-displacement is rounded: the kernel, ofdg_host_motion_blur and the numpy restatement of the tests give the same
 * bytes.  fl32(.) marks a float32 rounding (no contraction).
 *
 * Planes: src[f] and dst[f] are image f as [n,3,height,width] of src_fmt / dst_fmt (OFDG_FMT_F32 or OFDG_FMT_U8, chosen
 * independently; float32 frames hold byte values, see ofdg_photo); flow[f] is [n,2,height,width] of flow_fmt (OFDG_FMT_F32 or
 * OFDG_FMT_F16), read only: flow[0] the forward flow, flow[1] flow1.  A frame is absent (src[f], dst[f], flow[f] all NULL) or
 * complete (all three set).  width = height = 0: the context's frame; otherwise any size the context's rule allows, as in
 * ofdg_photo.  Mode 9 has no flow1: there only frame 0 can be blurred.
 *
 * Record of sample i: recs[i] when recs is given, else ofdg_motion_blur_draw(seed, first_index + i, the job).  Either way it
 * is sanitised before use, and the sanitised record is what recs_out[i] receives.
 *
 * 1. Draw.  Philox4x32-10 (ofdg_crop_philox) under the counter sampler's key of global index g, {seed ^ (uint32)(g >> 32) *
 *    0x9E3779B9, (uint32)g}, block 0 at the counter {0, 0, 0x0c76, 0} (taken: 0x0fd9 the sampler, 0x0c70 crop, 0x0c71 and 0x0c72
 *    photo, 0x0c73 spatial, 0x0c74 and 0x0c75 erase).  u(w) and sym(w, a) are ofdg_photo's.  on = u(.x) < prob;
 *    s0 = fl32(shutter_min + fl32(fl32(shutter_max - shutter_min) * u(.y)));  s1 = fl32(s0 + sym(.z, pair_shutter)).
 *    shutter = {s0, s1}; without `on` both are +0.  reserved = 0.  (.w is not used.)
 * 2. Sanitise, per frame: a NaN becomes 0, a value below 0 becomes 0 (-0.0 becomes +0), a value above OFDG_MBLUR_MAX_SHUTTER
 *    (2) becomes 2.  reserved = 0.
 * 3. Pixel (x, y) of frame f, s = shutter[f]:
 *    a. Half-displacement in 24.8.  (u, v) = the element of flow[f] widened to float32.  When u or v is not finite, Dx = Dy =
 *       0.  Otherwise Dx = (int)rintf(clamp(fl32(fl32(u * s) * 128.0f), -8192.0f, 8192.0f)), Dy likewise from v (ties to
 *       even; each component clamped on its own: a streak is at most 64 px long, OFDG_MBLUR_MAX_HALF_PX 32 each way).
 *    b. Taps.  L = max(|Dx|, |Dy|);  m = min(taps_side, (L + 255) >> 8) - one tap per pixel of half-extent on the major axis,
 *       no gaps until the cap taps_side (1..OFDG_MBLUR_MAX_TAPS_SIDE);  N = 2 m + 1.  For m > 0:  sx = (int)rintf(fl32((float)Dx
 *       / (float)m)), sy likewise (IEEE division).  Taps k = -m..m at Qx = clamp(256 x + k sx, 0, 256 (width - 1)), Qy =
 *       clamp(256 y + k sy, 0, 256 (height - 1)): a streak that leaves the frame repeats the border.
 *    c. Tap value, per channel.  The byte of an element: itself for uint8; for float32 the index rule of ofdg_photo (clamped
 *       to [0, 255], a NaN becomes 0, then rintf).  ix = Qx >> 8, fx = Qx & 255, iy and fy likewise; e00, e10, e01, e11 the
 *       bytes at (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1), each index clamped into the plane as ofdg_spatial
 *       does.  T = (256 - fx)(256 - fy) e00 + fx (256 - fy) e10 + (256 - fx) fy e01 + fx fy e11, an integer;  t = (T + 128)
 *       >> 8.
 *    d. Mean.  w = 65536 / N by integer division; the centre tap weighs 65536 - 2 m w, every other tap w.  S = the sum of
 *       weight_k * t_k (below 2^32 - 2^23: uint32 suffices).  b = (S + 2^23) >> 24.  A uint8 destination stores b, a float32
 *       one (float)b.  m = 0 gives the source byte: zero shutter, zero or non-finite flow, a sample the draw left out.
 *
 * Asynchronous on `stream`, the stream the planes were written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  One kernel for any
 * n and both frames; no atomics.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, a size that
 * breaks the rule above, 3 * width * height of 2^32 and more, another format code, non-zero flags or reserved, taps_side
 * outside 1..16, an incomplete frame or no frame at all, - when recs is NULL, as in ofdg_erase - prob outside [0, 1] or NaN,
 * shutter_min or shutter_max negative, NaN, infinite or above 2, shutter_min > shutter_max, pair_shutter negative, NaN or
 * infinite; a misaligned pointer (sources and flows as the render calls ask: 16-byte float32, 8-byte binary16, 4-byte uint8;
 * destinations and both record arrays 16-byte), a destination range (dst[f], recs_out) that overlaps any other range of the
 * job, OFDG_STREAM_OWN before any render / forward call on the context.
 *
 * Out of scope: layered blur at occlusion boundaries (a pixel is smeared along its own motion only, so a moving object does
 * not bleed over a still background), blur of the ground-truth planes, an in-place form, frame 1 in mode 9, streaks above
 * 64 px.
 */
#define OFDG_MBLUR_MAX_SHUTTER 2.0f
#define OFDG_MBLUR_MAX_HALF_PX 32      /* |Dx|, |Dy| <= 256 * 32 */
#define OFDG_MBLUR_MAX_TAPS_SIDE 16
typedef struct ofdg_mblur_rec {        /* 16 bytes */
  float   shutter[2];                  /* [frame], 0..OFDG_MBLUR_MAX_SHUTTER */
  int32_t reserved[2];
} ofdg_mblur_rec;
struct ofdg_mblur_job {                /* 128 bytes */
  const void* src[2];                  /* [n,3,height,width] of src_fmt: image0, image1, or NULL */
  void*       dst[2];                  /* [n,3,height,width] of dst_fmt */
  const void* flow[2];                 /* [n,2,height,width] of flow_fmt: flow, flow1 */
  const ofdg_mblur_rec* recs;          /* DEVICE, n records, or NULL: drawn */
  ofdg_mblur_rec*       recs_out;      /* DEVICE, n records, or NULL */
  long long first_index; uint32_t seed;
  int32_t width, height;               /* 0, 0: the context's frame */
  int32_t src_fmt, dst_fmt, flow_fmt, flags, taps_side;
  float   prob, shutter_min, shutter_max, pair_shutter;   /* ranges of the draw */
  int32_t reserved[2];
};
int ofdg_motion_blur(ofdg_ctx* ctx, const struct ofdg_mblur_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes and records in host memory, no alignment asked of any
 * pointer.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above through
 * ofdg_host_last_error. */
int ofdg_host_motion_blur(const struct ofdg_mblur_job* job, int n_samples, int width, int height);
/* The drawn record of global sample `index` (step 1 alone: not sanitised; pure, no GPU).  Of `ranges` only prob, shutter_min,
 * shutter_max and pair_shutter are read.  OFDG_EINVAL (ofdg_host_last_error), `out` untouched, for a NULL pointer or a range
 * that breaks the rules above. */
int ofdg_motion_blur_draw(uint32_t seed, long long index, const struct ofdg_mblur_job* ranges, ofdg_mblur_rec* out);

/*
 * Reprojection: each frame pulled through its own ground-truth flow, with residuals.  For frame f in {0, 1} ("own"; frame
 * 1 - f is "other") every pixel looks up the other frame where flow[f] says it went - flow[0] the forward flow, flow[1] flow1 -
 * and reports the other frame's bilinear value there (warped), how far that is from its own byte (err), whether the target is
 * in the frame (mask), and how far flow[1 - f], read at the target as the backward field, is from undoing the displacement
 * (fb2, the squared forward-backward residual in px^2).  Per sample and frame a row of integer counts and sums splits the
 * residuals by what occ[f] calls visible and hidden.  Every input is read only; NOT in place.  A pure function of the
 * buffers.  Everything is integers once a displacement is rounded to 1/256 px: the kernel, ofdg_host_reproject and the numpy
 * restatement of the tests give the same bytes and the same rows on every run.  fl32(.) marks a float32 rounding (no
 * contraction).
 *
 * Inputs: img[f] is image f as [n,3,height,width] of img_fmt (OFDG_FMT_F32 or OFDG_FMT_U8; float32 frames hold byte values, see
 * ofdg_photo); flow[f] is [n,2,height,width] of flow_fmt (OFDG_FMT_F32 or OFDG_FMT_F16); occ[f] is [n,1,height,width] of occ_fmt
 * (OFDG_FMT_F32 or OFDG_FMT_U8) or NULL.  Outputs, each optional on its own, per frame: warped[f] [n,3,height,width] of dst_fmt
 * (OFDG_FMT_F32 or OFDG_FMT_U8), err[f] and mask[f] uint8 [n,1,height,width], fb2[f] float32 [n,1,height,width]; rows:
 * n ofdg_reproject_row.  flags holds OFDG_REPROJ_FRAME0 and / or OFDG_REPROJ_FRAME1, the frames that are worked on (an output of
 * a frame that is not flagged must be NULL), and OFDG_REPROJ_ACCUMULATE.  width = height = 0: the context's frame; otherwise
 * any size the context's rule allows, as in ofdg_photo.
 *
 * Pixel (x, y) of a flagged frame f, (u, v) the element of flow[f] widened to float32:
 * 1. Bad.  u or v is not finite (exponent bits all set): the pixel is bad.
 * 2. Displacement in 24.8.  Dx = (int)rintf(clamp(fl32(u * 256.0f), -2^30, 2^30)) (ties to even), Dy likewise from v.
 *    Qx = 256 x + Dx, Qy = 256 y + Dy.
 * 3. Rounded target.  rx = (Qx + 128) >> 8 (arithmetic shift), ry likewise.  The pixel is inside iff 0 <= rx <= width - 1 and
 *    0 <= ry <= height - 1, else outside.
 * 4. Bad or outside: every warped element is 0, err 0, mask 0, fb2 +0.0f; of the row only n_bad or n_outside counts the pixel.
 * 5. Inside: mask 1.  Qx is clamped into [0, 256 (width - 1)], Qy into [0, 256 (height - 1)]; ix = Qx >> 8, fx = Qx & 255, iy
 *    and fy likewise, ix + 1 and iy + 1 clamped into the plane - step 3c of ofdg_motion_blur, as is the byte of an element
 *    (itself for uint8, the index rule of ofdg_photo for float32).  Per channel, e00, e10, e01, e11 the bytes of the OTHER frame
 *    at (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1): T = (256 - fx)(256 - fy) e00 + fx (256 - fy) e10 + (256 - fx)
 *    fy e01 + fx fy e11;  t = (T + 128) >> 8;  the warped byte w = (t + 128) >> 8.  A uint8 destination stores w, a float32 one
 *    (float)w.  err = the largest |w - own byte| of the three channels.
 * 6. Forward-backward residual, when flow[1 - f] is given.  Per component, b00, b10, b01, b11 the elements of flow[1 - f] at
 *    the same four places, B = (int)rintf(clamp(fl32(b * 256.0f), -2^30, 2^30)) each;  T = (256 - fx)(256 - fy) B00 + fx (256 -
 *    fy) B10 + (256 - fx) fy B01 + fx fy B11 in int64 (the weights sum to 65536);  bx = (T + 32768) >> 16 (arithmetic shift), by
 *    likewise.  ex = clamp(Dx + bx, -2^23, 2^23), ey likewise;  e2 = ex ex + ey ey (int64, at most 2^47);  fb2 = fl32((float)e2)
 *    * 2^-16 (exact).  When one of the eight elements is not finite, e2 = 2^47 and fb2 = +infinity.
 * 7. Visibility.  An inside pixel is visible when occ[f] is NULL or its element there is zero (float32: compares equal to 0,
 *    so -0.0 is and a NaN is not - ofdg_crop's rule), else hidden.
 * 8. Row of sample i, block f (nothing is added to an unflagged frame's block).  n_bad, n_outside, n_visible, n_hidden count the
 *    pixels; they sum to width * height.  With img[0] and img[1] both given: err_hist[err >> 4], sum_err_visible and
 *    max_err_visible over visible pixels, sum_err_hidden over hidden ones.  With flow[1 - f] given: n_fb_over_visible and
 *    n_fb_over_hidden count the pixels with e2 > (int64)fb_thresh_q8^2, sum_fb2_visible adds min(e2, 2^32 - 1) and
 *    max_fb2_visible is the largest e2, over visible pixels (units of 2^-16 px^2).  Fields whose inputs are absent stay 0.
 *    Without OFDG_REPROJ_ACCUMULATE the call first writes every byte of the n rows as zero on `stream`; with it the counts and
 *    sums are added to and the maxima raised (as OFDG_STATS_ACCUMULATE).
 *
 * Asynchronous on `stream`, the stream the planes were written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  One kernel for any
 * n and both frames; integer atomics only, so no bit depends on the order of arrival.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, a size that
 * breaks the rule above, 3 * width * height of 2^32 and more, another format code (occ_fmt counts only when a map is given),
 * unknown bits in flags, non-zero reserved, fb_thresh_q8 outside 0..2^23, no frame flagged, an output of an unflagged frame,
 * no output at all, a flagged frame without flow[f], warped / err / mask of frame f without img[1 - f], err without img[f], fb2
 * without flow[1 - f]; a misaligned pointer (inputs as the render calls ask: 16-byte float32, 8-byte binary16, 4-byte uint8;
 * destinations and rows 16-byte), a destination range (warped, err, mask, fb2, rows) that overlaps any other range of the job,
 * OFDG_STREAM_OWN before any render / forward call on the context.  Mode 9 has no flow1 and no maps: there frame 0 can be
 * reprojected, without fb2.
 *
 * Out of scope: sub-pixel affine-aware taps (affine-free: plain bilinear), the nearest label is not used to pick taps,
 * splatting / a forward warp (ofdg_splat below), an in-place form, one row for the whole batch, rows mapped through ofdg_pack, frame 1 and fb2 in
 * mode 9.
 */
#define OFDG_REPROJ_FRAME0     1
#define OFDG_REPROJ_FRAME1     2
#define OFDG_REPROJ_ACCUMULATE 4   /* add to the rows instead of overwriting them */
#define OFDG_REPROJ_ERR_BINS   16
#define OFDG_REPROJ_MAX_FB_THRESH_Q8 (1 << 23)
typedef struct ofdg_reproject_frame_row {   /* 128 bytes without padding */
  uint32_t n_bad, n_outside, n_visible, n_hidden;
  uint32_t err_hist[OFDG_REPROJ_ERR_BINS];  /* visible pixels, bin err >> 4 */
  uint32_t max_err_visible;
  uint32_t n_fb_over_visible, n_fb_over_hidden;
  uint32_t reserved;
  uint64_t sum_err_visible, sum_err_hidden;
  uint64_t sum_fb2_visible;                 /* of min(e2, 2^32 - 1), units of 2^-16 px^2 */
  uint64_t max_fb2_visible;                 /* the largest e2 */
} ofdg_reproject_frame_row;
typedef struct ofdg_reproject_row {         /* 256 bytes without padding: a block per frame */
  ofdg_reproject_frame_row frame[2];
} ofdg_reproject_row;
struct ofdg_reproject_job {                 /* 160 bytes */
  const void* img[2];                       /* [n,3,height,width] of img_fmt: image0, image1, or NULL */
  const void* flow[2];                      /* [n,2,height,width] of flow_fmt: flow, flow1, or NULL */
  const void* occ[2];                       /* [n,1,height,width] of occ_fmt: occ0, occ1, or NULL */
  void* warped[2];                          /* [n,3,height,width] of dst_fmt, or NULL */
  void* err[2];                             /* uint8 [n,1,height,width], or NULL */
  void* mask[2];                            /* uint8 [n,1,height,width], or NULL */
  void* fb2[2];                             /* float32 [n,1,height,width], or NULL */
  ofdg_reproject_row* rows;                 /* DEVICE, n rows, or NULL */
  int32_t width, height;                    /* 0, 0: the context's frame */
  int32_t img_fmt, dst_fmt, flow_fmt, occ_fmt;
  int32_t flags;                            /* OFDG_REPROJ_* */
  int32_t fb_thresh_q8;                     /* 0..2^23, in 1/256 px */
  int32_t reserved[2];
};
int ofdg_reproject(ofdg_ctx* ctx, const struct ofdg_reproject_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes and rows in host memory, no alignment asked of any
 * pointer.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above through
 * ofdg_host_last_error. */
int ofdg_host_reproject(const struct ofdg_reproject_job* job, int n_samples, int width, int height);

/*
 * Splat: each frame pushed along its own ground-truth flow to the instant t in [0, 1] - the forward warp, the counterpart
 * of ofdg_reproject's gather.  For frame f in {0, 1} ("own"; frame 1 - f is "other") every source pixel goes where the
 * fraction t_q8[f] / 256 of flow[f] takes it - flow[0] the forward flow, flow[1] flow1 -, and where several land on one
 * target pixel the generator's own order decides: the higher label (later in painter's order) wins, among equal labels the
 * lowest source index.  Frame 0 pushed by t and frame 1 by 1 - t show the same instant, with the exact flows from it to both
 * end frames; the targets nobody reached are the disocclusion holes, the sources that lost are the pixels covered at that
 * instant.  The winner is an integer maximum per target, so the scatter gives the same bits on every run: the kernels,
 * ofdg_host_splat and the numpy restatement of the tests agree byte for byte.  Every input is read only; NOT in place.
 * fl32(.) marks a float32 rounding (no contraction).
 *
 * Inputs: img[f] is image f as [n,3,height,width] of img_fmt (OFDG_FMT_F32 or OFDG_FMT_U8; float32 frames hold byte values, see
 * ofdg_photo) or NULL; flow[f] is [n,2,height,width] of flow_fmt (OFDG_FMT_F32 or OFDG_FMT_F16); label[f] is uint8
 * [n,height,width] (label0 / label1) or NULL: every priority 0; occ[f] is [n,1,height,width] of occ_fmt (OFDG_FMT_F32 or
 * OFDG_FMT_U8) or NULL, read by the rows only.  keys[f], uint32 [n,height,width] on the TARGET grid, is REQUIRED for a flagged
 * frame: workspace and output, what it held before the call does not matter (the call clears it on `stream`), after the call
 * it holds the winning keys.  Outputs, each optional on its own, per frame: image[f] [n,3,height,width] of dst_fmt (OFDG_FMT_F32
 * or OFDG_FMT_U8), to_own[f] and to_other[f] [n,2,height,width] of oflow_fmt (OFDG_FMT_F32 or OFDG_FMT_F16), mask[f] uint8
 * [n,1,height,width] on the TARGET grid, fate[f] uint8 [n,1,height,width] on the SOURCE grid; rows: n ofdg_splat_row.  flags
 * holds OFDG_SPLAT_FRAME0 and / or OFDG_SPLAT_FRAME1, the frames that are worked on, and OFDG_SPLAT_ACCUMULATE.  width = height
 * = 0: the context's frame; otherwise any size the context's rule allows, as in ofdg_photo, of at most OFDG_SPLAT_MAX_PIXELS
 * pixels.
 *
 * Record of sample i: recs[i] when recs is given, else ofdg_splat_draw(seed, first_index + i, the job).  Either way it is
 * sanitised before use, and the sanitised record is what recs_out[i] and the row's t_q8 receive.
 *
 * 1. Draw.  Philox4x32-10 (ofdg_crop_philox) under the counter sampler's key of global index g, {seed ^ (uint32)(g >> 32) *
 *    0x9E3779B9, (uint32)g}, block 0 at the counter {0, 0, 0x0c77, 0} (taken: 0x0fd9 the sampler, 0x0c70 crop, 0x0c71 and 0x0c72
 *    photo, 0x0c73 spatial, 0x0c74 and 0x0c75 erase, 0x0c76 motion blur).  t = t_min_q8 + (int)(((uint64).x * (uint64)(t_max_q8
 *    - t_min_q8 + 1)) >> 32);  t_q8 = {t, 256 - t}: frame 0 goes forward by t, frame 1 comes back by the rest, so both land
 *    on the same instant.  reserved = 0.  (.y, .z, .w are not used.)
 * 2. Sanitise.  Each t_q8[f] is clamped into 0..256; reserved = 0.
 * 3. Source pixel s = (x, y) of a flagged frame f, T = t_q8[f], (u, v) the element of flow[f] widened to float32:
 *    a. Bad.  u or v is not finite (exponent bits all set): the fate is 3.
 *    b. Displacement in 24.8.  Dx = (int)rintf(clamp(fl32(u * 256.0f), -2^30, 2^30)) (ties to even), Dy likewise from v:
 *       ofdg_reproject's step 2, bit for bit.
 *    c. Scaled displacement.  Sx = (int)(((int64)Dx * T + 128) >> 8) (arithmetic shift);  Qx = 256 x + Sx;  rx = (Qx + 128)
 *       >> 8 (arithmetic shift).  Sy, Qy, ry likewise.
 *    d. Inside iff 0 <= rx < width and 0 <= ry < height; otherwise the fate is 2.
 *    e. Key.  key = (L << 24) | (2^24 - 1 - (y * width + x)), L the label byte at s, 0 without a label plane.  Never 0, because
 *       width * height <= 2^24 - 1.
 *    f. Scatter.  keys[f][i][ry][rx] = max(itself, key) over all inside sources of sample i; the plane starts at 0.
 * 4. Target pixel p = (px, py), K its final key.  K = 0, a hole: mask 0, every element of image, to_own and to_other there is
 *    0 / +0.0.  Otherwise mask 1; the winner is the source s = 2^24 - 1 - (K & 0xFFFFFF) at (x, y) = (s % width, s / width).
 *    image holds the three bytes of img[f] at s (the byte of an element: itself for uint8, the index rule of ofdg_photo for
 *    float32); a uint8 destination stores the byte, a float32 one (float)byte.  to_own = ((float)(x - px), (float)(y - py)).
 *    to_other = (fl32((float)(256 (x - px) + Dx)) * 2^-8, likewise y), Dx and Dy the winner's.  An OFDG_FMT_F16 oflow_fmt rounds
 *    the float32 value once, to nearest even (an overflow becomes an infinity).  What p shows sat at p + to_own in frame f and
 *    sits at p + to_other in frame 1 - f.
 * 5. Fate of an inside source: 0 (shown) when the key at its target equals its own, else 1 (covered).
 * 6. Row of sample i, block f (nothing is written to an unflagged frame's block).  n_bad, n_outside, n_inside count the source
 *    pixels; n_filled and n_holes the target pixels; each triple / pair sums to width * height.  n_covered counts the sources
 *    of fate 1 and equals n_inside - n_filled.  With occ[f]: n_covered_visible / n_covered_hidden split the covered sources
 *    by occ[f] at the source.  With occ[1 - f]: n_hole_other_visible / n_hole_other_hidden split the holes by occ[1 - f] at the
 *    hole.  An element is visible when it is zero (float32: compares equal to 0 - ofdg_reproject's rule 7), else hidden;
 *    without the map both counts stay 0.  t_q8 = T.  Without OFDG_SPLAT_ACCUMULATE the call first writes every byte of the n
 *    rows as zero on `stream`; with it the counts are added to and t_q8 is overwritten.
 *
 * Asynchronous on `stream`, the stream the planes were written on; OFDG_STREAM_OWN as in ofdg_flow_stats.  A fixed number of
 * launches for any n and both frames: the clears, splat_scatter_kernel, splat_resolve_kernel (left out when nothing but keys
 * is asked for).  Integer atomics only, so no bit depends on the order of arrival.
 *
 * OFDG_EINVAL, nothing enqueued, no byte written, the field named in ofdg_last_error: NULL job, n_samples < 1, a size that
 * breaks the rule above, width * height above OFDG_SPLAT_MAX_PIXELS, another format code (occ_fmt counts only when a map is
 * given), unknown bits in flags, non-zero reserved, no frame flagged, a flagged frame without flow[f] or without keys[f], any
 * pointer of an unflagged frame (but occ[f], which the other frame's holes are set against), image[f] without img[f]; with
 * recs NULL, t_min_q8 or t_max_q8 outside 0..256 or t_min_q8 > t_max_q8; a misaligned pointer (inputs as the render calls ask:
 * 16-byte float32, 8-byte binary16, 4-byte uint8; keys, outputs, rows and records 16-byte), a written range (keys, image,
 * to_own, to_other, mask, fate, rows, recs_out) that overlaps any other range of the job, OFDG_STREAM_OWN before any render /
 * forward call on the context.  Mode 9 has no flow1, no labels and no maps: there frame 0 can be splatted, every priority 0.
 *
 * Out of scope: bilinear / summation / softmax splatting, sub-pixel-closest tie-breaks, hole filling, per-pixel hit counts,
 * an in-place form, planes of more than 2^24 - 1 pixels, frame 1 in mode 9.
 */
#define OFDG_SPLAT_FRAME0     1
#define OFDG_SPLAT_FRAME1     2
#define OFDG_SPLAT_ACCUMULATE 4   /* add to the rows instead of overwriting them */
#define OFDG_SPLAT_MAX_PIXELS ((1 << 24) - 1)   /* width * height at most */
typedef struct ofdg_splat_rec {             /* 16 bytes */
  int32_t t_q8[2];                          /* the fraction of flow[f] frame f is pushed by, in 1/256 */
  int32_t reserved[2];
} ofdg_splat_rec;
typedef struct ofdg_splat_frame_row {       /* 64 bytes without padding */
  uint32_t n_bad, n_outside, n_inside;      /* source pixels; sum = width * height */
  uint32_t n_filled, n_holes;               /* target pixels; sum = width * height */
  uint32_t n_covered;                       /* = n_inside - n_filled */
  uint32_t n_covered_visible, n_covered_hidden;       /* by occ[f] at the source; 0 without occ[f] */
  uint32_t n_hole_other_visible, n_hole_other_hidden; /* by occ[1 - f] at the hole; 0 without occ[1 - f] */
  uint32_t t_q8;                            /* the sanitised fraction used (overwritten, never added) */
  uint32_t reserved[5];
} ofdg_splat_frame_row;
typedef struct ofdg_splat_row {             /* 128 bytes without padding: a block per frame */
  ofdg_splat_frame_row frame[2];
} ofdg_splat_row;
struct ofdg_splat_job {                     /* 248 bytes (4 of padding at the end) */
  const void* img[2];                       /* [n,3,height,width] of img_fmt: image0, image1, or NULL */
  const void* flow[2];                      /* [n,2,height,width] of flow_fmt: flow, flow1 */
  const uint8_t* label[2];                  /* [n,height,width]: label0, label1, or NULL: every priority 0 */
  const void* occ[2];                       /* [n,1,height,width] of occ_fmt: occ0, occ1, or NULL: rows only */
  uint32_t* keys[2];                        /* [n,height,width] DEVICE: REQUIRED for a flagged frame; workspace AND output */
  void* image[2];                           /* [n,3,height,width] of dst_fmt, or NULL */
  void* to_own[2];                          /* [n,2,height,width] of oflow_fmt, or NULL */
  void* to_other[2];                        /* [n,2,height,width] of oflow_fmt, or NULL */
  void* mask[2];                            /* uint8 [n,1,height,width] on the TARGET grid: 1 filled, 0 hole */
  void* fate[2];                            /* uint8 [n,1,height,width] on the SOURCE grid: 0 shown, 1 covered, 2 outside, 3 bad */
  ofdg_splat_row* rows;                     /* DEVICE, n rows, or NULL */
  const ofdg_splat_rec* recs;               /* DEVICE, n records, or NULL: drawn */
  ofdg_splat_rec* recs_out;                 /* DEVICE, n records, or NULL */
  long long first_index;                    /* global index of sample 0 (the draw) */
  uint32_t seed;                            /* (the draw) */
  int32_t width, height;                    /* 0, 0: the context's frame */
  int32_t img_fmt, dst_fmt, flow_fmt, oflow_fmt, occ_fmt;
  int32_t flags;                            /* OFDG_SPLAT_* */
  int32_t t_min_q8, t_max_q8;               /* range of the draw, 0..256 */
  int32_t reserved[2];
};
int ofdg_splat(ofdg_ctx* ctx, const struct ofdg_splat_job* job, int n_samples, void* stream);
/* The same on HOST arrays (no GPU), the definition pixel by pixel: planes, keys, rows and records in host memory, no
 * alignment asked of any pointer.  width, height: the plane size; the job's own must be 0, 0 or the same.  Errors as above
 * through ofdg_host_last_error. */
int ofdg_host_splat(const struct ofdg_splat_job* job, int n_samples, int width, int height);
/* The record of global sample `index` under `seed` (step 1; pure, no GPU): of `ranges` only t_min_q8 and t_max_q8 are read.
 * Not sanitised.  OFDG_EINVAL for a NULL argument or a range that breaks the rule above. */
int ofdg_splat_draw(uint32_t seed, long long index, const struct ofdg_splat_job* ranges, ofdg_splat_rec* out);

/* Checkpoint / resume of ofdg_forward: the number of batches this context has produced is its whole sampler
 * state (the reference cannot resume: a restarted job replays its 45 streams from their seeds).
 * ofdg_set_step(k) makes the next ofdg_forward produce batch k (counter sampler: at no cost; reference-stream
 * sampler: the streams are rebuilt and k * batch_size * world_size tasks drawn and dropped on the host; mode 9:
 * the crop serving order of this rank is replayed too - install the warp fields BEFORE calling it). */
long long ofdg_get_step(const ofdg_ctx* ctx);
int ofdg_set_step(ofdg_ctx* ctx, long long step);

/* The internal stream the NEXT render / forward call of this context will work on
 * (a hipStream_t; they take turns).  See ofdg_render. */
void* ofdg_stream(ofdg_ctx* ctx);
/* How many internal streams take turns: a caller that cycles k * ofdg_num_chains output buffer sets and passes
 * ofdg_stream() finds every set always written by the same stream (no event needed between its writers). */
int ofdg_num_chains(const ofdg_ctx* ctx);
/* Counter sampler: how many batches of a chain ONE sampler -> geom -> raster launch serves, n = 1 .. 4 (the default is 4).
 * A call that finds no front end ready on its chain runs those three latency-bound kernels for a GROUP: its own batch and
 * the n - 1 batches that chain is asked for next (first_index + k x ofdg_num_chains x the stride of the caller's last two
 * calls, else batch x world_size; k = 1 .. n - 1); each of those calls then launches only its background preparation and
 * compose.  A call for anything else than the group's next batch - another first_index or n_samples, after ofdg_set_step,
 * ofdg_set_front_batches or a change of the pool - forgets the rest of the group and prepares its own: nothing is rendered
 * from a stale front end, and the bytes are those of n = 1, where every call launches its own front end.  It applies to the
 * overlapped pipeline without look-ahead (serial = 0, lookahead = 0); a chain's workspaces hold n batches, and a call whose
 * n x n_samples exceeds 512 samples gets the largest group that fits (ofdg_front_batches_for).  ofdg_ctx_info() ends in
 * " front=N".  OFDG_EINVAL unless n is 1 .. 4. */
int ofdg_set_front_batches(ofdg_ctx* ctx, int n);
/* The group a call for n_samples samples gets under the setting `front`: the largest N <= front with N x n_samples <= 512,
 * at least 1; OFDG_EINVAL unless front is 1 .. 4.  Needs no context and no device. */
int ofdg_front_batches_for(int front, int n_samples);
/* How many batches the chains hold ready for calls that have not come yet (the remaining parts of their groups): what the next
 * call for something else forgets.  OFDG_EINVAL for a NULL context. */
int ofdg_front_pending(const ofdg_ctx* ctx);

/* Wait for `stream` and for everything the context has in flight, and report
 * device-side error flags raised by kernels. */
int ofdg_synchronize(ofdg_ctx* ctx, void* stream);

/* The same device-side error flags WITHOUT waiting for anything in flight (all batches rendered so far). */
int ofdg_poll_errors(ofdg_ctx* ctx);
/* ... and per batch.  Every render / forward call has a number in its context ("ticket", ofdg_last_ticket right after the
 * call) and raises its device flags in a word of its own: ofdg_poll_errors_of(ticket) says whether THAT batch was truncated
 * (OFDG_ECAPACITY, the message names the batch) - what a prefetch ring calls when it hands over a batch whose own completion
 * event it has waited for (prefetch_full_.pop, LAY:269), so that an error of batch k is reported at batch k's Forward, not
 * at an older batch's, and batches k - 1 and k + 1 stay valid.  (The reference drops a bad sample silently, DG:1285-1292.)
 * The flags of the last 256 calls are kept; reading a word clears it - the error is reported ONCE, so a caller that wants to
 * go on must drop that batch when it gets the error (ofdg::DataGenerationLayer retires the buffer set before it throws).
 * A word never speaks for another batch: once a caller has asked by ticket, a word whose last owner was not asked about
 * is cleared in front of the first kernel of the call that takes it over (256 calls later), and a batch that was prepared
 * ahead and discarded takes its flags with it. */
long long ofdg_last_ticket(const ofdg_ctx* ctx);
int ofdg_poll_errors_of(ofdg_ctx* ctx, long long ticket);

/* ---- mode 9 (non-rigid deformation) warp fields: replaces WarpFields::CropGenerator
 * (WF:469-641), which DataGenerator::Start launches for MODE == 9 (DG:1016-1020). ---- */
/* Generate n_fields big fields (side 3*max(W,H)) on the device from seeded displacer
 * lists (the reference seeds from std::random_device) and cut them into (W+1)x(H+1)
 * crops; crops are then served like CropGenerator::get_crop (each 3 times, in order).
 * The Gaussian supports' exponential (WF:101-112) is the det_expf of include/ofdg_detmath.h (the fp64 exponential rounded
 * once) for BOTH samplers, not libm's expf: the fields are reproducible bit for bit on any device and in the oracle's detmath
 * mode, and agree with a libm evaluation to a small fraction of a pixel (tests/test_gpu_parity.py). */
int ofdg_warp_generate(ofdg_ctx* ctx, int n_fields, uint32_t seed);
/* Install caller-provided crops instead: n x {flow x, flow y, iflow x, iflow y} planes of
 * (H+1)*(W+1) floats (host memory). */
int ofdg_warp_upload(ofdg_ctx* ctx, const float* crops, int n);
int ofdg_warp_info(const ofdg_ctx* ctx, int* n_crops, int* w, int* h);
int ofdg_warp_download(ofdg_ctx* ctx, int index, float* crop);
/* Host only: displacer draws of one big field, n x 9 doubles {type, p0, p1, p2, support
 * cx, cy, sigma_x, sigma_y, angle} (WF:572-610). Returns n, or -n if cap is too small. */
int ofdg_host_displacers(int width, int height, uint32_t seed, double* out, int cap);

/* ---- inspection (tests / profiling) ---------------------------------------- */
/* Rasterise one polygon (n double vertices, already in screen space) with the
 * device rasteriser and return the raw AGG coverage (0..255) as w*h bytes. */
int ofdg_debug_rasterize(ofdg_ctx* ctx, const double* xy, int n_vertices,
                         uint8_t* coverage_host);
/* The same for a path with curve3 segments, flattened by the DEVICE (types[i]: 1 line_to, 3 curve3 control point
 * followed by its end point; entry 0 is the move_to vertex; n <= 64): conv_curve / curve3_div as geom_kernel runs them
 * (DG:493-517), pinned against compiled AGG in tests/test_gpu_parity.py. */
int ofdg_debug_rasterize_path(ofdg_ctx* ctx, const double* xy, const int* types, int n, uint8_t* coverage_host);
/* The DEVICE's span_interpolator_linear + dda2_line_interpolator (DG:203-216): out_xy[rows][len][2] = (x, y) in 24.8
 * fixed point under the inverse affine inv[6] (AGG member order), before the filter's -128 offset. */
int ofdg_debug_dda_rows(ofdg_ctx* ctx, const double* inv, int rows, int len, int* out_xy);
/* After ofdg_render: raw coverage of rasterised shape `shape` of sample
 * `sample`, frame 0/1, as w*h host bytes (zero outside its bounding box). */
int ofdg_debug_coverage(ofdg_ctx* ctx, int sample, int shape, int frame,
                        uint8_t* coverage_host);
int ofdg_debug_num_shapes(ofdg_ctx* ctx, int sample);
/* Number of raster work items the last launch left unprocessed (diagnostics: 0). */
int ofdg_debug_item_count(ofdg_ctx* ctx);
/* After a render / forward call with background_prep = 1: the number of tiles the one-launch form of the preparation
 * (bgprep_stream_kernel) walked for that batch and the number of workgroups that shared them grid-stride (0 tiles: the batch took
 * another form of the preparation).  Tests use it to make sure they reach a workgroup's 2nd, 3rd ... tile. */
int ofdg_debug_bgprep_tiles(ofdg_ctx* ctx, int* tiles, int* workgroups);
/* Tiles of bgprep_stream_kernel since the last call, by the form that rendered them: counts9[rotation + 3 * resize], rotation
 * 0 = general (mirrored / clamped crop coordinates), 1 = inside the image, 2 = inside and specialised by the side of the shift's
 * mirror lines; resize 0 = decided per row, 1 = both axes enlarge, 2 = both shrink.  The first call switches the counting on and
 * returns zeros.  (Texture::getRandomizedCrop, DG:87-109: which of its branches the batch took.) */
int ofdg_debug_bgprep_paths(ofdg_ctx* ctx, unsigned* counts9);
/* Exhaustive device evaluation of the per-byte formulas: composite add / subtract
 * [u*256+v] (DG:606, 626), AA mask byte [c], draw_image blend [d*256+m] for s=s_fixed. */
int ofdg_debug_tables(ofdg_ctx* ctx, uint8_t* add_tbl, uint8_t* sub_tbl, uint8_t* aa_tbl,
                      uint8_t* blend_tbl, int s_fixed);
/* include/ofdg_detmath.h (the sin / cos / expf the device counter-sampler path is defined with) evaluated
 * on the device: n angles -> sin, cos; m floats -> expf.  Host arrays. */
int ofdg_debug_detmath(ofdg_ctx* ctx, const double* angles, int n, double* sin_out, double* cos_out,
                       const float* x, int m, float* expf_out);
/* Per-kernel device time (ms), averaged over the launches recorded since ofdg_set_profiling (mode 1: the compose launch
 * and the background preparation of every 4th batch, completion signals on the kernels' own packets, nothing added to the
 * streams; mode 2: every kernel of every batch, with start markers; 0: off).  Names: "geom", "raster" (mode 2), "compose",
 * "background_prep" (where the preparation runs behind raster: batches the library prepares itself).
 * Mode 1 takes the compose launch's time from the completion of the chain's last preparation kernel to its own completion
 * (no marker packet in the stream): only launches enqueued right behind their preparation on the chain's own stream are
 * samples - a batch prepared ahead (ofdg_params.lookahead) or composed on a caller's stream is left out, since that span
 * would hold host and queue idle time; with nothing but such launches ofdg_kernel_ms reports "no profiled launch".  Mode 2
 * (start markers) times every launch. */
int ofdg_set_profiling(ofdg_ctx* ctx, int mode);
int ofdg_kernel_ms(ofdg_ctx* ctx, const char* kernel, float* ms);

/* ---- host-side pieces (no HIP device needed) --------------------------------- */
/* The reference-stream sampler on its own: ObjectParametersGenerator (DG:1358-2835)
 * driven like load_batch (LAY:197-213). */
typedef struct ofdg_host_sampler ofdg_host_sampler;
int ofdg_host_sampler_create(int mode, int width, int height, int num_objects,
                             ofdg_host_sampler** out);
int ofdg_host_sampler_next(ofdg_host_sampler* s, int n_tasks, ofdg_task* tasks,
                           ofdg_blueprint* bps, int bps_capacity, int* n_bps);
void ofdg_host_sampler_destroy(ofdg_host_sampler* s);
/* Blueprint -> fp64 affines exactly as RealizeObjectBlueprint / setMotion /
 * addBackgroundMotion compute them (DG:302-335, 1065-1173).  shape_mats: 12 doubles
 * per rasterised shape {intrinsic[6], intrinsic*motion[6]}; object_mats: 12 doubles
 * per blitted object {motion[6], inverse texture warp[6]} (sx,shy,shx,sy,tx,ty). */
int ofdg_host_realize(const ofdg_params* prm, int pool_n, int pool_w, int pool_h,
                      const ofdg_task* tasks, int n_tasks, const ofdg_blueprint* bps,
                      int n_bps, double* shape_mats, int shape_cap, int* n_shapes,
                      double* object_mats, int object_cap, int* n_objects);
/* Host logic of ofdg_params.background_prep = 1 (no GPU): the coordinate-map record of
 * Texture::getRandomizedCrop(2W, 2H, angle, zoom, shift) (DG:87-109) on a pool_w x pool_h image.
 * f[8] = ca, sa, w2, h2, rw2, rh2, fx, fy; i[6] = x0, y0, cw, ch, shift_x, shift_y. */
int ofdg_host_bg_prep(int pool_w, int pool_h, int width, int height, float angle, float zoom,
                      int shift_x, int shift_y, float* f, int* i);

/* One image file of a texture list as the layer's loader decodes it (TextureCollection, DG:117-149: CImg::load, then
 * R <-> B): binary PPM natively, PNG through the system's libpng 1.6 (bound at run time).  planar_bgr: 3 planes of
 * width x height bytes (B, G, R), or NULL to ask for the size only. */
int ofdg_host_decode_image(const char* path, uint8_t* planar_bgr, size_t capacity, int* width, int* height);

/* Parse a `layer { ... }` prototxt block (example-prototxt/train.prototxt). */
int ofdg_parse_prototxt(const char* text, ofdg_params* out, char* texture_dbases,
                        int texture_dbases_cap, int* n_top);
const char* ofdg_host_last_error(void);

/* ---- Caffe-layer-shaped surface: DataGenerationLayer (LAY:36-132, 266-291) ------ */
typedef struct ofdg_layer ofdg_layer;
/* ctor + LayerSetUp: parses the prototxt, opens the texture collection
 * ("synthetic:N:W:H[:seed]" or a list file of binary PPMs), reshapes 3 tops. */
int ofdg_layer_create(const char* layer_prototxt, ofdg_layer** out);
/* Forward_gpu: returns the device pointers of image0/image1/flow and the
 * shape {N,3,H,W} of image0. */
int ofdg_layer_forward(ofdg_layer* layer, float** image0, float** image1, float** flow,
                       int* shape4);
void ofdg_layer_destroy(ofdg_layer* layer);
/* data_param.prefetch > 1: how many of the batches rendered ahead were still unfinished when the last
 * ofdg_layer_forward returned (it waits for the oldest batch only, like prefetch_full_.pop, LAY:269). */
int ofdg_layer_in_flight(const ofdg_layer* layer);

/* ---- multi-GPU start-up (one process per GPU) -----------------------------------------------
 * Samples shard by global index with no data-path collective; what the ranks must agree on is the stream and
 * the pool.  ONE RCCL broadcast (ncclBroadcast over xGMI) carries rank 0's setup header + texture index table.
 * The reference has nothing to replace here: Caffe's multi-GPU solvers each build their own layer from the same
 * prototxt and the same 45 seeds (data_generation_layer.hpp:54, DG:1360) and so render identical samples. */
#define OFDG_UNIQUE_ID_BYTES 128 /* sizeof(ncclUniqueId) */
#define OFDG_POOL_SYNTHETIC 0    /* every rank generates the pool itself from pool_seed */
#define OFDG_POOL_UNIFORM   1    /* images of one size (pool_w x pool_h), contents replicated with ofdg_comm_bcast_pool */
#define OFDG_POOL_MIXED     2    /* images of different sizes (ofdg_pool_alloc_mixed), contents replicated likewise */
typedef struct ofdg_setup {
  int32_t seed, mode, width, height, num_objects, use_antialiasing, batch_size, sampler, background_prep;
  int32_t n_tex;          /* images in the texture pool */
  int32_t pool_kind;      /* OFDG_POOL_* */
  int32_t pool_w, pool_h; /* image size (0 x 0 for a mixed pool) */
  uint32_t pool_seed;     /* synthetic pools */
  int32_t n_table;        /* valid entries of the index table that travels with the header */
  int32_t status;         /* 0, or the root's error code (< 0): the root could not set itself up; every receiver fails with it */
  int32_t max_shapes_per_sample;
  int32_t reserved;
} ofdg_setup;
/* One texture of the pool as the kernels address it: `offset` texels into the pool the foreground path reads,
 * rows `pitch` texels apart; w x h = size of the source image. */
typedef struct ofdg_tex_entry {
  uint64_t offset;
  uint32_t w, h, pitch, reserved;
} ofdg_tex_entry;
typedef struct ofdg_comm ofdg_comm;
/* rank 0: ncclGetUniqueId into id[OFDG_UNIQUE_ID_BYTES]; hand it to the other processes through the launcher's
 * rendezvous (file, environment, key-value store). */
int ofdg_comm_unique_id(void* id);
/* hipSetDevice(device), then ncclCommInitRank.  Call it before any other HIP work of the process. */
int ofdg_comm_init(const void* id, int rank, int world_size, int device, ofdg_comm** out);
/* Use a communicator the caller already owns (an ncclComm_t); it is not destroyed by ofdg_comm_destroy. */
int ofdg_comm_adopt(void* nccl_comm, int rank, int world_size, int device, ofdg_comm** out);
void ofdg_comm_destroy(ofdg_comm* comm);
int ofdg_comm_rank(const ofdg_comm* comm);
int ofdg_comm_world_size(const ofdg_comm* comm);
const char* ofdg_comm_last_error(const ofdg_comm* comm);
/* THE start-up collective: root's *setup and table[0 .. setup->n_table) reach every rank in one ncclBroadcast.
 * Success or failure is decided together: a root that cannot provide a setup (its context or texture collection failed,
 * its table exceeds table_cap) still broadcasts - a header whose `status` carries its error code - so that every
 * receiver returns that code instead of waiting for a broadcast that never comes (ofdg_comm_bcast_abort is that call
 * for a root that failed before it had a setup at all). */
int ofdg_comm_bcast_setup(ofdg_comm* comm, int root, ofdg_setup* setup, ofdg_tex_entry* table, int table_cap);
int ofdg_comm_bcast_abort(ofdg_comm* comm, int root, int error_code, int table_cap);
/* Ranks of the communicator as RCCL reports them (ncclCommCount): what a multi-GPU run prints as its proof that the
 * native start-up really spanned world_size processes. */
int ofdg_comm_nccl_count(ofdg_comm* comm);
/* Replicate the root's resident pool into the (identically allocated) pools of the other ranks: ncclBroadcast
 * between the HBM pools, so that only the root reads the texture collection from disk (DG:117-149).  Every rank first
 * checks that all of its buffers exist and the ranks agree on that (one ncclAllReduce of a flag) before the first
 * payload broadcast: a rank that cannot take part makes the call fail on every rank. */
int ofdg_comm_bcast_pool(ofdg_comm* comm, int root, ofdg_ctx* ctx);
/* "Did every rank get this far?"  One ncclAllReduce(min) of a flag; every rank of the communicator must call it, with
 * local_ok = 0 if its own step failed (context creation, pool allocation ...).  Returns OFDG_OK on every rank if all
 * passed 1, otherwise OFDG_ESTARTUP on every rank - so a rank that failed between two collectives takes the others
 * out with it instead of leaving them waiting in the next one.  (A failure of the collective itself returns OFDG_EHIP
 * on the rank that saw it; RCCL then aborts the others.) */
int ofdg_comm_agree(ofdg_comm* comm, int local_ok);
/* The header / index table of a context's stream and pool (what the root broadcasts), and the parameters a
 * receiving rank creates its context with (rank, world_size and device come from the communicator). */
int ofdg_setup_of(const ofdg_ctx* ctx, ofdg_setup* setup, ofdg_tex_entry* table, int table_cap);
int ofdg_setup_params(const ofdg_setup* setup, const ofdg_comm* comm, ofdg_params* params);
/* Allocate (synthetic: also fill) this rank's pool as the setup describes it; a mixed pool takes its image sizes
 * from the index table that came with the setup. */
int ofdg_setup_alloc_pool(ofdg_ctx* ctx, const ofdg_setup* setup, const ofdg_tex_entry* table);
/* The derived textures of a mixed pool as raw device memory: [n][H][W] foreground and [n][2H][2W] background. */
int ofdg_pool_device_mixed(ofdg_ctx* ctx, void** fg, unsigned long long* fg_bytes, void** bg,
                           unsigned long long* bg_bytes);
/* ... and, with background_prep, whole image `index` (w * h BGRX texels): getRandomizedCrop reads the original. */
int ofdg_pool_device_image(ofdg_ctx* ctx, int index, void** ptr, unsigned long long* bytes);
/* DataGenerationLayer on a communicator: every rank passes the same prototxt; rank 0's options and texture
 * collection win (one broadcast), rank / world_size / device come from the communicator, and Forward yields
 * this rank's shard of every global batch. */
int ofdg_layer_create_dist(const char* layer_prototxt, ofdg_comm* comm, ofdg_layer** out);

#ifdef __cplusplus
}
#endif
#endif /* OFDG_H_ */
