// The loop detector's C++ adapter (plugin/proslam_hip_plugin.hpp, CorrespondenceFinderPlaceHIP) on two descriptor clouds passed in
// as raw bytes, in the sequence of test_place_recognition.cpp:
//   test_place_plugin <a.bin> <n_a> <b.bin> <n_b> <out.bin>
// a.bin / b.bin: uint8 descriptors [n][32] of local map 0 (graph id 0) and local map 1 (graph id 1).  Threshold 50, age 0, 50 inliers:
// compute() on map 0 finds nothing, addPreviousQuery(), compute() on map 1; prints "indices <count> <first>" and writes candidate 0's
// correspondences (prs_corr rows) to out.bin for the Python test to compare with tests/place_ref.py.  Also checks that compute()
// without a local map throws.  Exit status 0 = every check passed, 1 = a check failed, 2 = no device.
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

static bool read_cloud(const char* path, long n, PointIntensityDescriptorVectorCloud<3>& out) {
  std::ifstream in(path, std::ios::binary);
  const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (n < 0 || raw.size() != (size_t) n * PRS_DESC_BYTES) {
    return false;
  }
  out.resize((size_t) n);
  for (long i = 0; i < n; ++i) {
    std::memcpy(out[(size_t) i].descriptor(), raw.data() + (size_t) i * PRS_DESC_BYTES, PRS_DESC_BYTES);
    out[(size_t) i].coords[0] = out[(size_t) i].coords[1] = out[(size_t) i].coords[2] = 0.0f;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s <a.bin> <n_a> <b.bin> <n_b> <out.bin>\n", argv[0]);
    return 1;
  }
  PointIntensityDescriptorVectorCloud<3> map_a, map_b;
  if (!read_cloud(argv[1], std::atol(argv[2]), map_a) || !read_cloud(argv[3], std::atol(argv[4]), map_b)) {
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
  CorrespondenceFinderPlaceHIP<3> finder(ctx);
  finder.param_maximum_descriptor_distance.setValue(50.0f);
  finder.param_minimum_age_difference_to_candidates.setValue(0);
  finder.param_relocalize_min_inliers.setValue(50);
  bool threw = false;
  try {
    finder.compute();
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  finder.setCurrentLocalMapAndPoints(0, &map_a);
  finder.compute();
  CHECK(finder.indices().empty());
  finder.addPreviousQuery();
  finder.setCurrentLocalMapAndPoints(1, &map_b);
  finder.compute();
  finder.addPreviousQuery();
  CHECK(finder.indices().size() == 1);
  std::printf("indices %zu %zu\n", finder.indices().size(), finder.indices().empty() ? (size_t) 999 : finder.indices()[0]);
  if (!finder.indices().empty()) {
    const CorrespondenceVector corr = finder.correspondences(0);
    for (const Correspondence& c : corr) {
      CHECK(c.response < 50.0f);
    }
    std::ofstream out(argv[5], std::ios::binary);
    out.write(reinterpret_cast<const char*>(corr.data()), (std::streamsize) (corr.size() * sizeof(Correspondence)));
  }
  std::printf("%s\n", failures == 0 ? "all checks passed" : "checks failed");
  return failures == 0 ? 0 : 1;
}
