// TEST INFRASTRUCTURE -- stands in for the protobuf-generated header: the five fields of
// data_generation_param the reference's DataGenerator.cpp reads, as plain data.
#ifndef OFDG_REF_SHELL_CAFFE_PB_H_
#define OFDG_REF_SHELL_CAFFE_PB_H_
#include <string>
namespace caffe {
struct DataGenerationParameter {
  int mode_ = 7, first_level_threads_ = 1, second_level_threads_ = 1;
  bool use_antialiasing_ = true;
  std::string texture_dbases_;
  int mode() const { return mode_; }
  int first_level_threads() const { return first_level_threads_; }
  int second_level_threads() const { return second_level_threads_; }
  bool use_antialiasing() const { return use_antialiasing_; }
  const std::string& texture_dbases(int) const { return texture_dbases_; }
};
struct LayerParameter {
  DataGenerationParameter dgp;
  const DataGenerationParameter& data_generation_param() const { return dgp; }
};
}  // namespace caffe
#endif
