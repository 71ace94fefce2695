// TEST INFRASTRUCTURE.  Runs the REFERENCE's own affine code -- setIntrinsicTransform, setMotion,
// addBackgroundMotion, getPointFlow (DataGenerator.cpp) -- on the first tasks of a mode, with the calls
// Process_TaskBucket makes for the background and RealizeObjectBlueprint makes for every top-level
// object.  The reference sources are included from the reference checkout (nothing is copied);
// agg::trans_affine is oracle/ref_shell's statement of AGG's six published formulas, everything else
// of AGG / CImg is a no-op shell (no mask or texture is rendered here).
//
//   ref_motion MODE N_TASKS > motions.json
//     per object: obj_id, obj_type, m_motion and m_motion_inv as fp64 bit patterns (sx, shy, shx, sy, tx, ty),
//     getPointFlow forward and inverse as fp32 bit patterns at the grid "xs" x "ys" (row-major, y outer).
#include "ref_tasks.h"

static const int GX[] = {0, 1, 37, 101, 255, 256, 300, 511};
static const int GY[] = {0, 1, 95, 191, 192, 383};

static void put_affine(const char* key, const agg::trans_affine& m) {
  const double v[6] = {m.sx, m.shy, m.shx, m.sy, m.tx, m.ty};
  printf("\"%s\": [", key);
  for (int i = 0; i < 6; ++i) {
    uint64_t b;
    memcpy(&b, &v[i], 8);
    printf("\"%016llx\"%s", (unsigned long long)b, i < 5 ? ", " : "]");
  }
}

static void put_flow(const char* key, const DataGenerator::MovingObjectBase* obj, bool inverse) {
  printf("\"%s\": \"", key);
  for (int y : GY)
    for (int x : GX) {
      float u = x, v = y;
      obj->getPointFlow(&u, &v, inverse);   // virtual: the background goes through its own override
      uint32_t bu, bv;
      memcpy(&bu, &u, 4);
      memcpy(&bv, &v, 4);
      printf("%08x%08x", bu, bv);
    }
  printf("\"");
}

static void put_object(const DataGenerator::MovingObjectBase* obj, int obj_id, int obj_type, bool last) {
  printf("    {\"obj_id\": %d, \"obj_type\": %d, ", obj_id, obj_type);
  put_affine("m_motion", obj->m_motion);
  printf(", ");
  put_affine("m_motion_inv", obj->m_motion_inv);
  printf(",\n     ");
  put_flow("flow", obj, false);
  printf(",\n     ");
  put_flow("iflow", obj, true);
  printf("}%s\n", last ? "" : ",");
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s MODE N_TASKS\n", argv[0]); return 2; }
  caffe::LayerParameter param;
  param.dgp.mode_ = atoi(argv[1]);
  DataGenerator::ObjectParametersGenerator gen(param);
  const int n = atoi(argv[2]);
  printf("{\"mode\": %d, \"width\": %d, \"height\": %d, \"xs\": [", param.dgp.mode_, W, H);
  for (size_t i = 0; i < sizeof(GX) / sizeof(GX[0]); ++i) printf("%s%d", i ? ", " : "", GX[i]);
  printf("], \"ys\": [");
  for (size_t i = 0; i < sizeof(GY) / sizeof(GY[0]); ++i) printf("%s%d", i ? ", " : "", GY[i]);
  printf("],\n \"tasks\": [\n");
  for (int t = 0; t < n; ++t) {
    DataGenerator::TaskBucket* task = ref_next_task(gen);
    printf("  [\n");
    const DataGenerator::ObjectBlueprint* p = task->background_blueprint;
    DataGenerator::MovingObjectBackground bg(p->obj_id);
    bg.setMotion(p->rot, p->scale, p->trans_x, p->trans_y);
    put_object(&bg, p->obj_id, 0, task->object_blueprints.empty());
    for (size_t i = 0; i < task->object_blueprints.size(); ++i) {
      p = task->object_blueprints[i];
      DataGenerator::MovingObjectBase* obj = nullptr;
      switch (p->obj_type) {
        case DataGenerator::ObjType_t::Ellipse: obj = new DataGenerator::MovingObjectEllipse(p->obj_id); break;
        case DataGenerator::ObjType_t::Polygon: obj = new DataGenerator::MovingObjectPolygon(p->obj_id); break;
        case DataGenerator::ObjType_t::Composite: obj = new DataGenerator::MovingObjectComposite(p->obj_id); break;
        default: fprintf(stderr, "bad object type\n"); return 3;
      }
      obj->setIntrinsicTransform(p->init_rot, p->init_trans_x, p->init_trans_y);
      obj->setMotion(p->rot, p->scale, p->trans_x, p->trans_y);
      obj->addBackgroundMotion(bg.m_motion);
      put_object(obj, p->obj_id, (int)p->obj_type, i + 1 == task->object_blueprints.size());
      delete obj;
    }
    printf("  ]%s\n", t + 1 < n ? "," : "");
    ref_free_task(task);
  }
  printf(" ]}\n");
  return 0;
}
