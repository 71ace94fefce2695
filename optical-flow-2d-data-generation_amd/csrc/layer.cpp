#include "layer.h"

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>

namespace ofdg {

// ---------------------------------------------------------------------------
// Blob
// ---------------------------------------------------------------------------
Blob::~Blob() {
  if (data_ && !external_) (void)hipFree(data_);
}
void Blob::set_gpu_data(float* data) {
  if (data_ && !external_) (void)hipFree(data_);
  data_ = data;
  external_ = true;
  capacity_ = 0;
}
void Blob::Reshape(const std::vector<int>& shape) {
  size_t n = 1;
  for (int d : shape) {
    if (d < 0) throw std::runtime_error("Blob::Reshape: negative dimension");
    n *= (size_t)d;
  }
  shape_ = shape;
  count_ = n;
  if (external_) return;  // (the owner of the memory sized it)
  if (n > capacity_) {
    if (data_) (void)hipFree(data_);
    data_ = nullptr;
    if (hipMalloc((void**)&data_, n * sizeof(float)) != hipSuccess) throw std::runtime_error("Blob::Reshape: hipMalloc failed");
    capacity_ = n;
  }
}
size_t Blob::offset(int n, int c, int h, int w) const {
  size_t o = (size_t)n;
  o = o * (shape_.size() > 1 ? shape_[1] : 1) + c;
  o = o * (shape_.size() > 2 ? shape_[2] : 1) + h;
  o = o * (shape_.size() > 3 ? shape_[3] : 1) + w;
  return o;
}

// ---------------------------------------------------------------------------
// texture collection: the plan the files give (host_input.cpp), then the uploads
// ---------------------------------------------------------------------------
void load_texture_collection(ofdg_ctx* ctx, const std::string& spec) {
  const TexturePlan plan = plan_texture_collection(spec);
  if (!plan.error.empty()) throw std::runtime_error(plan.error);
  auto check = [&](int rc) {
    if (rc != OFDG_OK) throw std::runtime_error(std::string("Could not open texture collection: ") + ofdg_last_error(ctx));
  };
  if (plan.synthetic) return check(ofdg_pool_synthetic(ctx, plan.n, plan.w, plan.h, plan.seed));
  const int n = (int)plan.paths.size();
  check(plan.mixed ? ofdg_pool_alloc_mixed(ctx, n) : ofdg_pool_alloc(ctx, n, plan.widths[0], plan.heights[0]));
  for (int i = 0; i < n; ++i) {
    std::vector<uint8_t> img;
    int w = 0, h = 0;
    std::string why;
    if (!read_image(plan.paths[i], &img, &w, &h, &why)) throw std::runtime_error("Could not open texture collection (cannot read " + plan.paths[i] + ": " + why + ")");
    check(plan.mixed ? ofdg_pool_upload_mixed(ctx, i, img.data(), w, h) : ofdg_pool_upload(ctx, i, img.data(), w, h));
  }
}

// ---------------------------------------------------------------------------
// DataGenerationLayer
// ---------------------------------------------------------------------------
DataGenerationLayer::DataGenerationLayer(const std::string& layer_prototxt, ofdg_comm* comm) : cfg_(parse_layer_prototxt(layer_prototxt)) {
  if (!cfg_.type.empty() && cfg_.type != "DataGeneration") throw std::runtime_error("layer type is not \"DataGeneration\"");
  constexpr int kTableCap = 65536;
  std::vector<ofdg_tex_entry> table;
  ofdg_setup su;
  std::memset(&su, 0, sizeof(su));
  const int rank = comm ? ofdg_comm_rank(comm) : 0;
  std::exception_ptr local_failure;
  auto create = [&]() {
    int rc = ofdg_create(&cfg_.params, &ctx_);
    if (rc == OFDG_EBADMODE) throw std::runtime_error("BAD MODE");  // DataGenerator.cpp:2004
    if (rc != OFDG_OK) throw std::runtime_error(std::string("DataGenerationLayer: ") + ofdg_last_error(nullptr));
  };
  auto bcast = [&]() {  // the one start-up collective: rank 0's stream + pool description
    table.resize(kTableCap);
    if (ofdg_comm_bcast_setup(comm, 0, &su, table.data(), kTableCap) != OFDG_OK)
      throw std::runtime_error(std::string("DataGenerationLayer: ") + ofdg_comm_last_error(comm));
  };
  try {
    if (comm) {
      ofdg_params mine;
      ofdg_setup_params(&su, comm, &mine);  // (rank, world_size, device of the communicator)
      cfg_.params.rank = mine.rank; cfg_.params.world_size = mine.world_size; cfg_.params.device = mine.device;
    }
    if (!comm || rank == 0) {
      try {
        create();
        load_texture_collection(ctx_, cfg_.texture_dbases);  // DataGenerator ctor -> TextureCollection (DataGenerator.cpp:992)
      } catch (...) {
        // the other ranks are waiting in the start-up broadcast: tell them that it failed, then fail here
        if (comm) (void)ofdg_comm_bcast_abort(comm, 0, OFDG_ETEXTURES, kTableCap);
        throw;
      }
      if (comm) {
        table.resize(kTableCap);
        int rcs = ofdg_setup_of(ctx_, &su, table.data(), kTableCap);
        if (rcs != OFDG_OK) su.status = rcs;  // (travels with the broadcast: every rank fails together)
        bcast();
      }
    } else {
      bcast();
      // From here to the next collective this rank works alone (context, pool allocation): if that fails the others
      // must not be left waiting in the collective - the failure is kept and every rank learns of it in the agreement.
      try {
        ofdg_params p;
        ofdg_setup_params(&su, comm, &p);
        p.prefetch = cfg_.params.prefetch;
        p.first_level_threads = cfg_.params.first_level_threads; p.second_level_threads = cfg_.params.second_level_threads;
        cfg_.params = p;
        create();
        if (ofdg_setup_alloc_pool(ctx_, &su, table.data()) != OFDG_OK)
          throw std::runtime_error(std::string("Could not open texture collection: ") + ofdg_last_error(ctx_));
      } catch (...) {
        local_failure = std::current_exception();
      }
    }
    if (comm) {  // every rank that came through the broadcast: did everybody set itself up?
      const int rca = ofdg_comm_agree(comm, local_failure ? 0 : 1);
      if (local_failure) std::rethrow_exception(local_failure);
      if (rca != OFDG_OK) throw std::runtime_error(std::string("DataGenerationLayer: ") + ofdg_comm_last_error(comm));
    }
    // a texture collection read from disk lives on rank 0 only until here: replicate it over xGMI
    if (comm && su.pool_kind != OFDG_POOL_SYNTHETIC && ofdg_comm_bcast_pool(comm, 0, ctx_) != OFDG_OK)
      throw std::runtime_error(std::string("DataGenerationLayer: ") + ofdg_comm_last_error(comm));
    // DataGenerator::Start launches the CropGenerator for MODE == 9 (DataGenerator.cpp:1016-1020)
    if (cfg_.params.mode == 9 && ofdg_warp_generate(ctx_, 2, (uint32_t)cfg_.params.seed) != OFDG_OK)
      throw std::runtime_error(std::string("warp field generation: ") + ofdg_last_error(ctx_));
  } catch (...) {
    if (ctx_) ofdg_destroy(ctx_);
    ctx_ = nullptr;
    throw;
  }
}

DataGenerationLayer::~DataGenerationLayer() {
  if (ctx_) (void)ofdg_synchronize(ctx_, nullptr);
  for (float* p : ring_) if (p) (void)hipFree(p);
  for (void* e : ring_done_) if (e) (void)hipEventDestroy((hipEvent_t)e);
  ofdg_destroy(ctx_);
}

// render the next batch of the stream into its buffer set, on the context's next internal stream
void DataGenerationLayer::enqueue_next() {
  const int P = (int)ring_.size() / 3;
  float** set = &ring_[(size_t)(produced_ % P) * 3];
  void* chain = ofdg_stream(ctx_);  // the whole batch runs in order on this internal stream
  if (ofdg_forward(ctx_, set[0], set[1], set[2], chain) != OFDG_OK)
    throw std::runtime_error(std::string("DataGenerationLayer::Forward: ") + ofdg_last_error(ctx_));
  if (hipEventRecord((hipEvent_t)ring_done_[(size_t)(produced_ % P)], (hipStream_t)chain) != hipSuccess)
    throw std::runtime_error("DataGenerationLayer::Forward: hipEventRecord failed");
  ring_ticket_[(size_t)(produced_ % P)] = ofdg_last_ticket(ctx_);
  ++produced_;
}

void DataGenerationLayer::LayerSetUp(const std::vector<Blob*>& bottom, const std::vector<Blob*>& top) {
  if (!bottom.empty()) throw std::runtime_error("DataGeneration takes no bottom blobs");  // ExactNumBottomBlobs() == 0
  if (top.size() != 3) throw std::runtime_error("DataGeneration produces exactly 3 top blobs");  // load_batch indexes output[0..2]
  const int N = cfg_.params.batch_size, H = cfg_.params.height, W = cfg_.params.width;
  // StartInternalThread (data_generation_layer.cpp:132): the first prefetch - 1 batches start rendering now
  const int P = cfg_.params.prefetch;
  if (P > 1 && ring_.empty()) {
    ring_.assign((size_t)P * 3, nullptr);
    for (int k = 0; k < P * 3; ++k)
      if (hipMalloc((void**)&ring_[k], (size_t)N * (k % 3 == 2 ? 2 : 3) * H * W * sizeof(float)) != hipSuccess)
        throw std::runtime_error("DataGenerationLayer: hipMalloc of the prefetch buffers failed");
    ring_done_.assign((size_t)P, nullptr);
    ring_ticket_.assign((size_t)P, -1);
    for (int k = 0; k < P; ++k)
      if (hipEventCreateWithFlags((hipEvent_t*)&ring_done_[k], hipEventDisableTiming) != hipSuccess)
        throw std::runtime_error("DataGenerationLayer: hipEventCreate failed");
    while (produced_ < P - 1) enqueue_next();
  }
  if (!ring_.empty())
    for (int k = 0; k < 3; ++k) top[k]->set_gpu_data(ring_[k]);  // (the tops never own memory in this mode)
  top[0]->Reshape({N, 3, H, W});  // data_generation_layer.cpp:128-130
  top[1]->Reshape({N, 3, H, W});
  top[2]->Reshape({N, 2, H, W});
}

void DataGenerationLayer::Forward_gpu(const std::vector<Blob*>& bottom, const std::vector<Blob*>& top) {
  (void)bottom;
  if (top.size() != 3) throw std::runtime_error("DataGeneration produces exactly 3 top blobs");
  const int N = cfg_.params.batch_size, H = cfg_.params.height, W = cfg_.params.width;
  top[0]->Reshape({N, 3, H, W});
  top[1]->Reshape({N, 3, H, W});
  top[2]->Reshape({N, 2, H, W});
  if (!ring_.empty()) {
    // prefetch_full_.pop (data_generation_layer.cpp:269): the oldest batch in flight - finished long ago when the
    // caller's own work takes longer than a render - becomes the tops; its successor starts rendering at once
    const int P = (int)ring_.size() / 3;
    if (produced_ == consumed_) enqueue_next();
    // wait for THIS set's event only: the batches behind it keep rendering
    if (hipEventSynchronize((hipEvent_t)ring_done_[(size_t)(consumed_ % P)]) != hipSuccess)
      throw std::runtime_error("DataGenerationLayer::Forward: hipEventSynchronize failed");
    // THIS batch's device error flags (a flag raised by a younger batch still rendering is reported at that batch's own turn).
    // The word is cleared by the read, so the error is reported once.  A truncated batch is RETIRED like a good one before
    // the exception leaves: the tops point at ITS buffer set - the one set no batch in flight renders into until the next
    // Forward, so what a caller that catches the exception still reads there is stable (and marked bad by the exception:
    // the reference drops a bad sample and leaves stale data in its batch slot, DG:1285-1292) - and its successor starts
    // rendering; the next Forward hands out the NEXT batch.
    std::string bad;
    if (ofdg_poll_errors_of(ctx_, ring_ticket_[(size_t)(consumed_ % P)]) != OFDG_OK) bad = ofdg_last_error(ctx_);
    float** set = &ring_[(size_t)(consumed_ % P) * 3];
    for (int k = 0; k < 3; ++k) top[k]->set_gpu_data(set[k]);
    ++consumed_;
    in_flight_ = 0;
    for (long long b = consumed_; b < produced_; ++b)
      if (hipEventQuery((hipEvent_t)ring_done_[(size_t)(b % P)]) == hipErrorNotReady) ++in_flight_;
    try {
      while (produced_ < consumed_ + P - 1) enqueue_next();
    } catch (const std::exception& e) {  // (the batch's own error comes first: a failed enqueue shows again at the next Forward)
      if (bad.empty()) throw;
      bad += std::string(" (and the next batch could not be enqueued: ") + e.what() + ")";
    }
    if (!bad.empty()) throw std::runtime_error("DataGenerationLayer::Forward: " + bad);
    return;
  }
  int rc = ofdg_forward(ctx_, top[0]->mutable_gpu_data(), top[1]->mutable_gpu_data(), top[2]->mutable_gpu_data(), nullptr);
  if (rc == OFDG_OK) rc = ofdg_synchronize(ctx_, nullptr);
  if (rc != OFDG_OK) throw std::runtime_error(std::string("DataGenerationLayer::Forward: ") + ofdg_last_error(ctx_));
}

void DataGenerationLayer::Forward_cpu(const std::vector<Blob*>& bottom, const std::vector<Blob*>& top) {
  Forward_gpu(bottom, top);
}

}  // namespace ofdg

// ---------------------------------------------------------------------------
// C-ABI of the layer (declared in include/ofdg.h; the wrappers that need no GPU are in host_api.cpp)
// ---------------------------------------------------------------------------
using namespace ofdg;

struct ofdg_layer {
  std::unique_ptr<DataGenerationLayer> layer;
  Blob top[3];
  std::string err;
};
extern "C" {

int ofdg_layer_create(const char* prototxt, ofdg_layer** out) { return ofdg_layer_create_dist(prototxt, nullptr, out); }
int ofdg_layer_create_dist(const char* prototxt, ofdg_comm* comm, ofdg_layer** out) {
  if (!prototxt || !out) return OFDG_EINVAL;
  *out = nullptr;
  std::unique_ptr<ofdg_layer> L(new ofdg_layer());
  try {
    L->layer.reset(new DataGenerationLayer(prototxt, comm));
    std::vector<Blob*> top = {&L->top[0], &L->top[1], &L->top[2]};
    L->layer->LayerSetUp({}, top);
  } catch (const std::exception& e) {
    g_host_error = e.what();
    if (g_host_error == "BAD MODE") return OFDG_EBADMODE;
    if (g_host_error.find("texture collection") != std::string::npos) return OFDG_ETEXTURES;
    return OFDG_EINVAL;
  }
  *out = L.release();
  return OFDG_OK;
}
void ofdg_layer_destroy(ofdg_layer* L) { delete L; }
int ofdg_layer_in_flight(const ofdg_layer* L) { return L ? L->layer->in_flight_after_last_forward() : OFDG_EINVAL; }
// Forward(): fills the three top blobs and returns their device pointers.
int ofdg_layer_forward(ofdg_layer* L, float** image0, float** image1, float** flow, int* shape4) {
  if (!L) return OFDG_EINVAL;
  try {
    std::vector<Blob*> top = {&L->top[0], &L->top[1], &L->top[2]};
    L->layer->Forward_gpu({}, top);
  } catch (const std::exception& e) {
    g_host_error = e.what();
    return OFDG_EHIP;
  }
  if (image0) *image0 = L->top[0].mutable_gpu_data();
  if (image1) *image1 = L->top[1].mutable_gpu_data();
  if (flow) *flow = L->top[2].mutable_gpu_data();
  if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = L->top[0].shape()[i];
  return OFDG_OK;
}
}  // extern "C"
