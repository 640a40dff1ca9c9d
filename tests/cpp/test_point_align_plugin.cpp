// The loop aligner's C++ adapter (plugin/proslam_hip_plugin.hpp, AlignerSliceProcessor3DHIP) on one cloud pair passed in as raw bytes:
//   test_point_align_plugin <in.bin> <out.bin>
// in.bin: int32 n_fixed, n_moving, n_corr; float fixed [n_fixed][3], moving [n_moving][3]; int32 corr [n_corr][2] (fixed, moving).
// Runs the adapter with its defaults (the kitti.conf loop aligner: Clamp 3, 100 iterations, 10 inliers, 30 correspondences, verdict
// 25 / 0.5 / 2) from identity and writes float X[16], the prs_point_align_result bytes and the inlier flags [n_corr] to out.bin for the
// Python test to compare with tests/point_align_ref.py.  Then checks that compute() without correspondences throws and that an index
// outside the fixed cloud throws.  Exit status 0 = every check passed, 1 = a check failed, 2 = no device.
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

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <in.bin> <out.bin>\n", argv[0]);
    return 1;
  }
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (raw.size() < 12) {
    std::printf("input too short\n");
    return 1;
  }
  int32_t n[3];
  std::memcpy(n, raw.data(), sizeof(n));
  if (raw.size() != 12 + 12 * (size_t) n[0] + 12 * (size_t) n[1] + 8 * (size_t) n[2]) {
    std::printf("input holds %zu bytes, expected %zu\n", raw.size(), 12 + 12 * (size_t) n[0] + 12 * (size_t) n[1] + 8 * (size_t) n[2]);
    return 1;
  }
  const char* at = raw.data() + 12;
  AlignerSliceProcessor3DHIP::CloudType fixed(n[0]), moving(n[1]);
  for (auto& pt : fixed) {
    std::memcpy(pt.coordinates(), at, 12);
    at += 12;
  }
  for (auto& pt : moving) {
    std::memcpy(pt.coordinates(), at, 12);
    at += 12;
  }
  CorrespondenceVector corr(n[2]);
  for (auto& c : corr) {
    std::memcpy(&c.fixed_idx, at, 4);
    std::memcpy(&c.moving_idx, at + 4, 4);
    c.response = 0.f;
    at += 8;
  }
  ContextPtr ctx;
  try {
    ctx.reset(new Context(0));
  } catch (const std::exception& e) {
    std::printf("no device: %s\n", e.what());
    return 2;
  }
  AlignerSliceProcessor3DHIP aligner(ctx);
  aligner.setFixed(&fixed);
  aligner.setMoving(&moving);
  bool threw = false;
  try {
    aligner.compute();
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  std::printf("[  OK  ] compute() without correspondences throws\n");
  aligner.setCorrespondences(&corr);
  const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  aligner.setMovingInFixed(identity);
  aligner.compute();
  CHECK(aligner.status() == AlignerSliceProcessor3DHIP::Success);
  CHECK(aligner.accepted());
  CHECK(aligner.result().iterations == 100);
  std::ofstream out(argv[2], std::ios::binary);
  out.write(reinterpret_cast<const char*>(aligner.movingInFixed()), 16 * sizeof(float));
  out.write(reinterpret_cast<const char*>(&aligner.result()), sizeof(prs_point_align_result));
  out.write(reinterpret_cast<const char*>(aligner.inliers().data()), (std::streamsize) aligner.inliers().size());
  out.close();
  std::printf("[  OK  ] compute() registers the pair\n");
  CorrespondenceVector bad = corr;
  if (!bad.empty()) {
    bad[bad.size() / 2].fixed_idx = n[0];
  }
  aligner.setCorrespondences(&bad);
  aligner.setMovingInFixed(identity);
  threw = false;
  try {
    aligner.compute();
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw && !bad.empty());
  std::printf("[  OK  ] an index outside the fixed cloud throws\n");
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
