// The selective extractor's C++ adapter (plugin/proslam_hip_plugin.hpp) driven like the reference's own gtests
// (srrg2_proslam/tests/test_feature_extractors.cpp:168-262) on KITTI city_left[0], passed in as raw bytes:
//   test_selective_plugin <image.raw> <rows> <cols>
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

template <typename Extractor>
static void reference_sequence(const ContextPtr& ctx, const std::vector<uint8_t>& img, int rows, int cols, const char* descriptor) {
  Extractor extractor(ctx);
  extractor.param_detector_type.setValue("GFTT");
  extractor.param_descriptor_type.setValue(descriptor);
  extractor.param_target_number_of_keypoints.setValue(100);
  extractor.param_target_bin_width_pixels.setValue(10);
  extractor.param_enable_seeding_when_tracking.setValue(false);
  typename Extractor::PointCloudType initial;
  extractor.setFeatures(&initial);
  extractor.compute(img.data(), rows, cols, cols);
  CHECK_EQ(initial.size(), 94);
  extractor.param_target_number_of_keypoints.setValue(1000);
  const int radius[4] = {100, 50, 10, 5}, expected[4] = {719, 581, 294, 237};
  for (int k = 0; k < 4; ++k) {
    typename Extractor::PointCloudType candidates;
    extractor.setFeatures(&candidates);
    extractor.setProjections(&initial, radius[k]);
    extractor.compute(img.data(), rows, cols, cols);
    CHECK_EQ(candidates.size(), expected[k]);
  }
  // the projections were consumed: the next call seeds in the whole image (1000 keypoints budget)
  typename Extractor::PointCloudType again, fresh;
  extractor.setFeatures(&again);
  extractor.compute(img.data(), rows, cols, cols);
  Extractor seeder(ctx);
  seeder.param_detector_type.setValue("GFTT");
  seeder.param_target_number_of_keypoints.setValue(1000);
  seeder.param_target_bin_width_pixels.setValue(10);
  seeder.setFeatures(&fresh);
  seeder.compute(img.data(), rows, cols, cols);
  CHECK_EQ(again.size(), fresh.size());
  CHECK_EQ(again.size() > 94, 1);
  std::printf("[  OK  ] %s %s: 94 / 719 / 581 / 294 / 237, projections cleared after tracking\n", Extractor::PointCloudType::value_type::Dim == 2 ? "2D" : "3D", descriptor);
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <image.raw> <rows> <cols>\n", argv[0]);
    return 1;
  }
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<uint8_t> img((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if ((int) img.size() != rows * cols) {
    std::printf("image file holds %zu bytes, expected %d\n", img.size(), rows * cols);
    return 1;
  }
  ContextPtr ctx;
  try {
    ctx.reset(new Context(0));
  } catch (const std::exception& e) {
    std::printf("no device: %s\n", e.what());
    return 2;
  }
  reference_sequence<IntensityFeatureExtractorSelective2DHIP>(ctx, img, rows, cols, "ORB-256");
  reference_sequence<IntensityFeatureExtractorSelective2DHIP>(ctx, img, rows, cols, "BRIEF-256");
  reference_sequence<IntensityFeatureExtractorSelective3DHIP>(ctx, img, rows, cols, "ORB-256");
  // the external mask (seeding mode): only the left half of the image detects
  {
    IntensityFeatureExtractorSelective2DHIP extractor(ctx);
    extractor.param_detector_type.setValue("GFTT");
    extractor.param_target_number_of_keypoints.setValue(1000);
    std::vector<uint8_t> mask((size_t) rows * cols, 0);
    for (int r = 0; r < rows; ++r) {
      for (int c = 0; c < cols / 2; ++c) mask[(size_t) r * cols + c] = 1;
    }
    IntensityFeatureExtractorSelective2DHIP::PointCloudType masked, unmasked;
    extractor.setFeatures(&masked);
    extractor.setKeypointDetectionMask(mask.data(), cols);
    extractor.compute(img.data(), rows, cols, cols);
    extractor.setFeatures(&unmasked);
    extractor.compute(img.data(), rows, cols, cols);  // the mask was consumed
    int outside = 0;
    for (const auto& q : masked) outside += q.coords[0] >= cols / 2;
    CHECK_EQ(outside, 0);
    CHECK_EQ(masked.size() > 0 && unmasked.size() > masked.size(), 1);
    std::printf("[  OK  ] external seeding mask: %zu keypoints inside, %zu without it\n", masked.size(), unmasked.size());
  }
  // FAST (the reference's default detector type) is not built: a loud error, never another detector
  {
    IntensityFeatureExtractorSelective2DHIP extractor(ctx);
    IntensityFeatureExtractorSelective2DHIP::PointCloudType out;
    extractor.setFeatures(&out);
    bool threw = false;
    try {
      extractor.compute(img.data(), rows, cols, cols);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK_EQ(threw, 1);
    std::printf("[  OK  ] detector_type FAST throws\n");
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
