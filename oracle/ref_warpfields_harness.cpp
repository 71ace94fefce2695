// TEST INFRASTRUCTURE.  Runs the REFERENCE's own WarpFields.cpp -- supports, displacers,
// DisplacementComposer, the 17 self-composition passes, NaN flagging, clamp_near_zeros --
// on a given displacer list.  The reference source is included from where it lies in the
// reference checkout (nothing is copied); CImg is oracle/ref_shell's container shell.
//
//   ref_warpfields SIZE displacers.f64 out.f32
//     displacers.f64: n x 9 float64, the layout of oracle.displacers (type, p0, p1, p2,
//                     support cx, cy, sigma_x, sigma_y, angle)
//     out.f32:        flow x, flow y, iflow x, iflow y -- four SIZE x SIZE float32 planes
//
// Built twice (make -C oracle ref): as is (libm), and with -DOFDG_DET_EXPF -fno-builtin-expf,
// where this file DEFINES expf as include/ofdg_detmath.h's ofdg_det_expf: the reference's
// code then computes with the exponential the device is defined with.  The number of calls
// that arrived here is printed; a fixture generator must refuse 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#ifdef OFDG_DET_EXPF
#include "ofdg_detmath.h"
static unsigned long long g_expf_calls = 0;
extern "C" float expf(float x) noexcept {
  ++g_expf_calls;
  return ofdg_det_expf(x);
}
#endif

#include "src/caffe/WarpFields.cpp"

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s SIZE displacers.f64 out.f32\n", argv[0]); return 2; }
  const int size = atoi(argv[1]);
  FILE* f = fopen(argv[2], "rb");
  if (!f || size < 1) { fprintf(stderr, "bad arguments\n"); return 2; }
  std::vector<double> d;
  double row[9];
  while (fread(row, sizeof(double), 9, f) == 9) d.insert(d.end(), row, row + 9);
  fclose(f);
  const size_t n = d.size() / 9;

  WarpFields::DisplacementComposer dc(size, size);
  for (size_t i = 0; i < n; ++i) {
    const double* p = &d[i * 9];
    WarpFields::Displacers::DisplacerBase* ptr = nullptr;
    // double -> float at the call, as in CropGenerator::worker_thread_loop
    switch ((int)p[0]) {
      case 0: ptr = new WarpFields::Displacers::Translation(p[1], p[2]); break;
      case 1: ptr = new WarpFields::Displacers::Rotation(p[1], p[2], p[3]); break;
      case 2: ptr = new WarpFields::Displacers::Zoom(p[1], p[2], p[3]); break;
      default: fprintf(stderr, "bad displacer type\n"); return 2;
    }
    dc.add_displacer(ptr).with_support(new WarpFields::Supports::Gaussian2D(p[4], p[5], p[6], p[7], p[8]));
  }
  WarpFields::FlowField ff;
  ff.init_from_DisplacementComposer(dc).clamp_near_zeros();
  const CImg<float> flow = ff.get_flow();
  const CImg<float> iflow = ff.get_iflow();

  FILE* o = fopen(argv[3], "wb");
  if (!o) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
  const size_t plane2 = (size_t)2 * size * size;
  if (flow.size() != plane2 || iflow.size() != plane2) { fprintf(stderr, "unexpected field shape\n"); return 3; }
  fwrite(flow.data(), sizeof(float), plane2, o);
  fwrite(iflow.data(), sizeof(float), plane2, o);
  fclose(o);
#ifdef OFDG_DET_EXPF
  printf("{\"displacers\": %zu, \"expf\": \"ofdg_det_expf\", \"expf_calls\": %llu}\n", n, g_expf_calls);
#else
  printf("{\"displacers\": %zu, \"expf\": \"libm\"}\n", n);
#endif
  return 0;
}
