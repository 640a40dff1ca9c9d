// The local-map manager's C++ adapter (plugin/proslam_hip_plugin.hpp, LocalMapManagerHIP) on one planted sequence:
//   test_session_plugin <frames> <X.bin> <status.bin> <warnings.bin> <out.bin>
// X.bin float [frames][16], status.bin / warnings.bin int32 [frames].  Shipped KITTI settings (10 m, 0.25 rad), a graph of 3 nodes
// and 3 edges (so that the sequence runs into the last node).  Writes, for the Python test to compare with the Python path's bytes:
// reason int32 [frames], status int32 [frames], pose float [frames][16], prediction float [frames][16], then n_nodes, n_edges int32,
// estimates double [n_nodes][16], from / to int32 [n_edges], measurements float [n_edges][16], information float [n_edges][36],
// the log (local map int32 [frames], pose float [frames][16]) and the unrolled trajectory float [frames][16].
// Exit status 0 = every check passed, 1 = a check failed, 2 = no device.
#include <cstdio>
#include <fstream>
#include <iterator>

#define PROSLAM_HIP_WITH_HIP_RUNTIME
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
  std::memcpy(out.data(), raw.data(), raw.size());
  return true;
}

template <class T>
static void put(std::ofstream& out, const std::vector<T>& v) {
  out.write(reinterpret_cast<const char*>(v.data()), (std::streamsize) (v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s <frames> <X.bin> <status.bin> <warnings.bin> <out.bin>\n", argv[0]);
    return 1;
  }
  const long n = std::atol(argv[1]);
  std::vector<float> X;
  std::vector<int32_t> status, warnings;
  if (n < 1 || !read_array(argv[2], (size_t) n * 16, X) || !read_array(argv[3], (size_t) n, status) || !read_array(argv[4], (size_t) n, warnings)) {
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
  LocalMapManagerHIP manager(ctx, 64, 3, 3, (int) n);
  CHECK(manager.numLocalMaps() == 1 && manager.currentLocalMap() == 0 && manager.numFrames() == 0);
  std::vector<int32_t> reasons, statuses;
  std::vector<float> poses, predictions;
  for (long k = 0; k < n; ++k) {
    const int nodes_before = manager.numLocalMaps();
    const int reason       = manager.step(X.data() + 16 * k, status[(size_t) k], warnings[(size_t) k]);
    CHECK(manager.hasToSplit() == (reason != PRS_SESSION_NO_SPLIT));
    CHECK(manager.numLocalMaps() == nodes_before + (reason != PRS_SESSION_NO_SPLIT ? 1 : 0));
    CHECK(manager.currentLocalMap() == manager.numLocalMaps() - 1);
    if (k > 0 && (status[(size_t) k] != 1 || warnings[(size_t) k] < 0) && manager.status() == PRS_OK) {
      CHECK(reason == PRS_SESSION_SPLIT_LOST);
    }
    reasons.push_back(reason);
    statuses.push_back(manager.status());
    const std::vector<float> pose = manager.robotInLocalMap(), pred = manager.prediction();
    poses.insert(poses.end(), pose.begin(), pose.end());
    predictions.insert(predictions.end(), pred.begin(), pred.end());
  }
  CHECK(manager.numFrames() == (int) n);
  std::vector<int32_t> from, to, local_map;
  std::vector<float> Z, omega, logged;
  manager.factors(from, to, Z, omega);
  manager.fullTrajectory(local_map, logged);
  const std::vector<double> estimates = manager.estimates();
  const std::vector<float> unrolled   = manager.unrollFullTrajectory();
  CHECK(from.size() + 1 == estimates.size() / 16 && unrolled.size() == (size_t) n * 16 && local_map.size() == (size_t) n);
  std::ofstream out(argv[5], std::ios::binary);
  put(out, reasons), put(out, statuses), put(out, poses), put(out, predictions);
  put(out, std::vector<int32_t>{(int32_t) (estimates.size() / 16), (int32_t) from.size()});
  put(out, estimates), put(out, from), put(out, to), put(out, Z), put(out, omega), put(out, local_map), put(out, logged), put(out, unrolled);
  std::printf("%d local maps, %d frames\n", manager.numLocalMaps(), manager.numFrames());
  std::printf("%s\n", failures == 0 ? "all checks passed" : "checks failed");
  return failures == 0 ? 0 : 1;
}
