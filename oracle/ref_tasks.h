// TEST INFRASTRUCTURE, shared by ref_sampler_harness.cpp and ref_motion_harness.cpp: includes the
// reference's DataGenerator.cpp / WarpFields.cpp from the reference checkout, produces tasks the way
// DataGenerationLayer::load_batch does, and serialises them.
//
// Byte layout of one task (little endian; float = IEEE binary32 bits, everything else int32):
//   blueprint(background), int32 n_objects, blueprint(object) x n_objects
//   blueprint := every ObjectBlueprint member in declaration order:
//     obj_id, obj_type, init_rot, init_scale, init_trans_x, init_trans_y, rot, scale, trans_x, trans_y,
//     tex_id, tex_rot, tex_scale, tex_shift_x, tex_shift_y, ellipse_scale_x, ellipse_scale_y,
//     n_segments, (segment type, x, y) x n_segments, n_components, blueprint(component) x n_components,
//     is_additive_component, do_warpfield_deformation
//
// The reference's ObjectBlueprint constructor leaves every member but obj_type uninitialised, and each mode
// sets only the members it uses.  So that the stream is a function of the reference's code alone, the global
// operator new below hands out ZEROED memory: a member the reference never writes reads as 0 / 0.f / false.
#ifndef OFDG_REF_TASKS_H_
#define OFDG_REF_TASKS_H_
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

void* operator new(std::size_t n) {
  void* p = calloc(1, n ? n : 1);
  if (!p) throw std::bad_alloc();
  return p;
}
void* operator new[](std::size_t n) { return operator new(n); }
void operator delete(void* p) noexcept { free(p); }
void operator delete[](void* p) noexcept { free(p); }
void operator delete(void* p, std::size_t) noexcept { free(p); }
void operator delete[](void* p, std::size_t) noexcept { free(p); }

#include "src/caffe/WarpFields.cpp"
#include "src/caffe/DataGenerator.cpp"

static void ref_put_i(std::string& s, int32_t v) { s.append((const char*)&v, 4); }
static void ref_put_f(std::string& s, float v) { s.append((const char*)&v, 4); }

static void ref_put_blueprint(std::string& s, const DataGenerator::ObjectBlueprint* b) {
  ref_put_i(s, b->obj_id); ref_put_i(s, (int32_t)b->obj_type);
  ref_put_f(s, b->init_rot); ref_put_f(s, b->init_scale); ref_put_f(s, b->init_trans_x); ref_put_f(s, b->init_trans_y);
  ref_put_f(s, b->rot); ref_put_f(s, b->scale); ref_put_f(s, b->trans_x); ref_put_f(s, b->trans_y);
  ref_put_i(s, b->tex_id); ref_put_f(s, b->tex_rot); ref_put_f(s, b->tex_scale);
  ref_put_i(s, b->tex_shift_x); ref_put_i(s, b->tex_shift_y);
  ref_put_f(s, b->ellipse_scale_x); ref_put_f(s, b->ellipse_scale_y);
  const size_t n = b->polygon_segment_types.size();
  if (b->polygon_segment_x.size() != n || b->polygon_segment_y.size() != n) {
    fprintf(stderr, "segment vectors of different lengths\n");
    exit(3);
  }
  ref_put_i(s, (int32_t)n);
  for (size_t i = 0; i < n; ++i) {
    ref_put_i(s, (int32_t)b->polygon_segment_types[i]);
    ref_put_f(s, b->polygon_segment_x[i]);
    ref_put_f(s, b->polygon_segment_y[i]);
  }
  ref_put_i(s, (int32_t)b->composite_component_blueprint_ptrs.size());
  for (const DataGenerator::ObjectBlueprint* c : b->composite_component_blueprint_ptrs) ref_put_blueprint(s, c);
  ref_put_i(s, b->is_additive_component ? 1 : 0);
  ref_put_i(s, b->do_warpfield_deformation ? 1 : 0);
}

static void ref_put_task(std::string& s, const DataGenerator::TaskBucket* t) {
  ref_put_blueprint(s, t->background_blueprint);
  ref_put_i(s, (int32_t)t->object_blueprints.size());
  for (const DataGenerator::ObjectBlueprint* b : t->object_blueprints) ref_put_blueprint(s, b);
}

// one task, in the order of calls of DataGenerationLayer::load_batch
static DataGenerator::TaskBucket* ref_next_task(DataGenerator::ObjectParametersGenerator& gen) {
  DataGenerator::TaskBucket* task = new DataGenerator::TaskBucket();
  {
    DataGenerator::ObjectBlueprint* b = new DataGenerator::ObjectBlueprint();
    b->obj_id = 1;
    gen.generateBackground(b);
    task->background_blueprint = b;
  }
  const int count = gen.generateNumberOfFgObjects();
  task->object_blueprints.resize(count);
  for (int k = 0; k < count; ++k) {
    DataGenerator::ObjectBlueprint* b = new DataGenerator::ObjectBlueprint();
    b->obj_id = k + 10;
    gen.generateForegroundObject(b);
    task->object_blueprints[k] = b;
  }
  return task;
}

static void ref_free_task(DataGenerator::TaskBucket* task) {
  delete task->background_blueprint;
  for (DataGenerator::ObjectBlueprint* b : task->object_blueprints) delete b;
  delete task;
}
#endif
