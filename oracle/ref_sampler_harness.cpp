// TEST INFRASTRUCTURE.  Drives the REFERENCE's own ObjectParametersGenerator (all 13 mode
// tables, DataGenerator.cpp) exactly like DataGenerationLayer::load_batch
// (data_generation_layer.cpp: background with obj_id 1, generateNumberOfFgObjects, objects with
// obj_id 10 + index) and writes the task stream as bytes.  The reference sources are included
// from where they lie in the reference checkout (nothing is copied); AGG / CImg / protobuf are
// oracle/ref_shell's container shells -- the sampler uses none of their arithmetic.
//
//   ref_sampler MODE N_TASKS > stream.bin          (ref_tasks.h: the byte layout)
#include "ref_tasks.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s MODE N_TASKS\n", argv[0]); return 2; }
  caffe::LayerParameter param;
  param.dgp.mode_ = atoi(argv[1]);
  DataGenerator::ObjectParametersGenerator gen(param);
  const int n = atoi(argv[2]);
  for (int t = 0; t < n; ++t) {
    DataGenerator::TaskBucket* task = ref_next_task(gen);
    std::string s;
    ref_put_task(s, task);
    fwrite(s.data(), 1, s.size(), stdout);
    ref_free_task(task);
  }
  return 0;
}
