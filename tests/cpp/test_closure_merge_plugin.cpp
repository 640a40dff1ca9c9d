// The closure merger's C++ adapters (plugin/proslam_hip_plugin.hpp, MergerCorrespondenceProjectiveDepth3DHIP and
// MergerCorrespondencePointIntensityDescriptor3fHIP) on one (scene, measurement) pair passed in as raw arrays:
//   test_closure_merge_plugin <uvd|xyz> <n> <nm> <nc> <rows> <cols> <fx> <fy> <cx> <cy> <target> <distance2> <scene.bin> <scene_desc.bin>
//                             <meas.bin> <meas_desc.bin> <corr.bin> <T.bin> <out.bin> <out_desc.bin>
// scene.bin float [n][3], meas.bin float [nm][3] ((u, v, d) or (x, y, z)), the descriptors uint8 [.][32], corr.bin {int32, int32,
// float} [nc], T.bin float [16] (measurement in scene).  rows = 0 leaves the canvas unset, as the first of the reference's two
// gtests does (tests/test_mergers.cpp:174-205).  Prints "points <k> merged <m> added <a>" and writes the scene after compute()
// (float [k][3], uint8 [k][32]) for the Python test to compare with the batch entry.  Also checks that compute() without a
// scene throws and that the measurement cloud is not modified.  Exit status 0 = every check passed, 1 = a check failed, 2 = no device.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "proslam_hip_plugin.hpp"

using namespace proslam_hip;

static int failures = 0;
#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);           \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

template <class T>
static bool read_array(const char* path, size_t count, std::vector<T>& out) {
  std::ifstream in(path, std::ios::binary);
  const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (raw.size() != count * sizeof(T)) {
    return false;
  }
  out.resize(count);
  if (count) {
    std::memcpy(out.data(), raw.data(), raw.size());
  }
  return true;
}

static PointIntensityDescriptorVectorCloud<3> cloud_of(const std::vector<float>& xyz, const std::vector<uint8_t>& desc) {
  PointIntensityDescriptorVectorCloud<3> c(xyz.size() / 3);
  for (size_t i = 0; i < c.size(); ++i) {
    std::memcpy(c[i].coords, &xyz[3 * i], 3 * sizeof(float));
    std::memcpy(c[i].descriptor_row, &desc[PRS_DESC_BYTES * i], PRS_DESC_BYTES);
  }
  return c;
}

template <class Merger>
static int run(ContextPtr ctx, char** argv, PointIntensityDescriptorVectorCloud<3>& scene, const PointIntensityDescriptorVectorCloud<3>& meas,
               const CorrespondenceVector& corr, const std::vector<float>& T) {
  Merger merger(ctx);
  bool threw = false;
  try {
    merger.compute();
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  const float K[9] = {(float) std::atof(argv[7]), 0.f, (float) std::atof(argv[9]), 0.f, (float) std::atof(argv[8]), (float) std::atof(argv[10]), 0.f, 0.f, 1.f};
  merger.param_maximum_response.setValue(50.f);
  merger.param_maximum_distance_geometry_squared.setValue((float) std::atof(argv[12]));
  if (std::atoi(argv[5]) > 0) {
    merger.param_unprojector->param_canvas_rows.setValue((uint64_t) std::atoi(argv[5]));
    merger.param_unprojector->param_canvas_cols.setValue((uint64_t) std::atoi(argv[6]));
  }
  merger.param_unprojector->setCameraMatrix(K);
  merger.param_target_number_of_merges.setValue((uint64_t) std::atol(argv[11]));
  merger.setMeasurementInScene(T.data());
  merger.setScene(&scene);
  merger.setMeasurement(&meas);
  merger.setCorrespondences(&corr);
  const size_t before = scene.size();
  const PointIntensityDescriptorVectorCloud<3> backup(meas);
  merger.compute();
  CHECK(scene.size() == before + merger.numberOfAddedPoints());
  CHECK(scene.size() <= before + meas.size());  // tests/test_mergers.cpp:235-236
  CHECK(meas.size() == backup.size());
  for (size_t i = 0; i < meas.size(); ++i) {
    CHECK(std::memcmp(meas[i].coords, backup[i].coords, sizeof(backup[i].coords)) == 0);
  }
  std::printf("points %zu merged %zu added %zu\n", scene.size(), merger.numberOfMergedPoints(), merger.numberOfAddedPoints());
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 21) {
    std::fprintf(stderr, "usage: %s <uvd|xyz> <n> <nm> <nc> <rows> <cols> <fx> <fy> <cx> <cy> <target> <distance2> <8 files>\n", argv[0]);
    return 1;
  }
  const std::string kind = argv[1];
  const long n = std::atol(argv[2]), nm = std::atol(argv[3]), nc = std::atol(argv[4]);
  std::vector<float> xyz, z, T;
  std::vector<uint8_t> desc, zdesc;
  CorrespondenceVector corr;
  if (n < 0 || nm < 0 || nc < 0 || (kind != "uvd" && kind != "xyz") || !read_array(argv[13], (size_t) n * 3, xyz) ||
      !read_array(argv[14], (size_t) n * PRS_DESC_BYTES, desc) || !read_array(argv[15], (size_t) nm * 3, z) ||
      !read_array(argv[16], (size_t) nm * PRS_DESC_BYTES, zdesc) || !read_array(argv[17], (size_t) nc, corr) || !read_array(argv[18], 16, T)) {
    std::printf("input size does not match\n");
    return 1;
  }
  ContextPtr ctx;
  try {
    ctx.reset(new Context(0));
  } catch (const std::exception& e) {
    std::printf("no device: %s\n", e.what());
    return 2;
  }
  PointIntensityDescriptorVectorCloud<3> scene = cloud_of(xyz, desc);
  const PointIntensityDescriptorVectorCloud<3> meas = cloud_of(z, zdesc);
  if (kind == "uvd") {
    run<MergerCorrespondenceProjectiveDepth3DHIP>(ctx, argv, scene, meas, corr, T);
  } else {
    run<MergerCorrespondencePointIntensityDescriptor3fHIP>(ctx, argv, scene, meas, corr, T);
  }
  std::ofstream out(argv[19], std::ios::binary), out_desc(argv[20], std::ios::binary);
  for (const auto& p : scene) {
    out.write(reinterpret_cast<const char*>(p.coords), 3 * sizeof(float));
    out_desc.write(reinterpret_cast<const char*>(p.descriptor_row), PRS_DESC_BYTES);
  }
  std::printf("%s\n", failures == 0 ? "all checks passed" : "checks failed");
  return failures == 0 ? 0 : 1;
}
