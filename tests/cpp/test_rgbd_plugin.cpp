// The RGB-D preprocessor's C++ adapter (plugin/proslam_hip_plugin.hpp) on one ICL frame, passed in as raw bytes:
//   test_rgbd_plugin <gray.raw> <depth_mm.raw> <rows> <cols> <out.bin>
// Runs RawDataPreprocessorMonocularDepthHIP configured as icl.conf:642-650,745-770 (FAST 5, 3x3 detectors, 500 keypoints,
// depth_scaling_factor_to_meters 0.001) on the uint16 depth image and writes the cloud to out.bin (int32 n, then n x (float u, v, d,
// intensity, 32 descriptor bytes)) for the Python test to compare with tests/rgbd_ref.py.  Then checks that an all-zero depth image
// leaves the status at Error with an empty cloud and that an unknown depth type throws.
// Exit status 0 = every check passed, 1 = a check failed, 2 = no device.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "proslam_hip_plugin.hpp"

using namespace proslam_hip;

static int failures = 0;
#define CHECK_EQ(a, b)                                                                               \
  do {                                                                                               \
    const long long va = (long long) (a), vb = (long long) (b);                                      \
    if (va != vb) {                                                                                  \
      std::printf("  FAILED %s:%d: %s == %lld, expected %lld\n", __FILE__, __LINE__, #a, va, vb); \
      ++failures;                                                                                    \
    }                                                                                                \
  } while (0)

static std::vector<uint8_t> read_file(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s <gray.raw> <depth_mm.raw> <rows> <cols> <out.bin>\n", argv[0]);
    return 1;
  }
  const int rows = std::atoi(argv[3]), cols = std::atoi(argv[4]);
  const std::vector<uint8_t> gray = read_file(argv[1]), depth = read_file(argv[2]);
  if ((int) gray.size() != rows * cols || (int) depth.size() != 2 * rows * cols) {
    std::printf("image files hold %zu / %zu bytes, expected %d / %d\n", gray.size(), depth.size(), rows * cols, 2 * rows * cols);
    return 1;
  }
  ContextPtr ctx;
  try {
    ctx.reset(new Context(0));
  } catch (const std::exception& e) {
    std::printf("no device: %s\n", e.what());
    return 2;
  }
  RawDataPreprocessorMonocularDepthHIP pre(ctx);
  pre.param_depth_scaling_factor_to_meters.setValue(0.001f);
  IntensityFeatureExtractorBinnedHIP& ex = pre.featureExtractor();
  ex.param_detector_threshold.setValue(5.f);
  ex.param_enable_non_maximum_suppression.setValue(true);
  ex.param_target_number_of_keypoints.setValue(500);
  ex.param_number_of_detectors_vertical.setValue(3);
  ex.param_number_of_detectors_horizontal.setValue(3);
  RawDataPreprocessorMonocularDepthHIP::MeasurementType meas;
  pre.setMeas(&meas);
  pre.compute(gray.data(), rows, cols, cols, depth.data(), rows, cols, 2 * cols, PRS_DEPTH_U16);
  CHECK_EQ(pre.status(), RawDataPreprocessorMonocularDepthHIP::Ready);
  CHECK_EQ(meas.size() > 0, 1);
  {
    std::ofstream out(argv[5], std::ios::binary);
    const int32_t n = (int32_t) meas.size();
    out.write(reinterpret_cast<const char*>(&n), sizeof(n));
    for (const auto& q : meas) {
      out.write(reinterpret_cast<const char*>(q.coords), 3 * sizeof(float));
      out.write(reinterpret_cast<const char*>(&q.intensity_value), sizeof(float));
      out.write(reinterpret_cast<const char*>(q.descriptor_row), PRS_DESC_BYTES);
    }
  }
  std::printf("[  OK  ] ICL frame: %zu measurements with depth, status Ready\n", meas.size());
  // no depth anywhere: every feature is dropped, the status is Error (raw_data_preprocessor_monocular_depth.cpp:131-136)
  {
    const std::vector<uint16_t> zero((size_t) rows * cols, 0);
    pre.compute(gray.data(), rows, cols, cols, zero.data(), rows, cols, 2 * cols, PRS_DEPTH_U16);
    CHECK_EQ(pre.status(), RawDataPreprocessorMonocularDepthHIP::Error);
    CHECK_EQ(meas.size(), 0);
    std::printf("[  OK  ] all-zero depth: empty cloud, status Error\n");
  }
  // an unknown depth type throws (:126-128)
  {
    bool threw = false;
    try {
      pre.compute(gray.data(), rows, cols, cols, depth.data(), rows, cols, 2 * cols, 7);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK_EQ(threw, 1);
    CHECK_EQ(pre.status(), RawDataPreprocessorMonocularDepthHIP::Error);
    std::printf("[  OK  ] unknown depth type throws\n");
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
