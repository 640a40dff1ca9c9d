// The global solver's C++ adapter (plugin/proslam_hip_plugin.hpp, SolverPoseGraphHIP) with the Levenberg-Marquardt algorithm:
//   test_pose_graph_lm_plugin <n> <m> <poses.bin> <fixed.bin> <from.bin> <to.bin> <Z.bin> <out.bin>
// poses.bin double [n][16], fixed.bin uint8 [n], from.bin / to.bin int32 [m], Z.bin float [m][16].  The last factor is held back from
// setGraph() and added with addFactor().  The adapter's defaults are Gauss-Newton (checked); then param_algorithm selects
// LevenbergMarquardt with the parameters of icl.conf / tum.conf (the adapter's defaults: 10 rounds, epsilon 1e-3, 100 trials, tau
// 1e-5, clamps 1/3 and 2/3, variable damping).  Prints "iterations <k> trials <t0,t1,...> chi2 <v>" and writes the estimates (double
// [n][16]) to out.bin for the Python test to compare with tests/pose_graph_lm_ref.py.  Exit status 0 = every check passed,
// 1 = a check failed, 2 = no device.
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
  std::memcpy(out.data(), raw.data(), raw.size());
  return true;
}

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr, "usage: %s <n> <m> <poses.bin> <fixed.bin> <from.bin> <to.bin> <Z.bin> <out.bin>\n", argv[0]);
    return 1;
  }
  const long n = std::atol(argv[1]), m = std::atol(argv[2]);
  std::vector<double> poses;
  std::vector<uint8_t> fixed;
  std::vector<int32_t> from, to;
  std::vector<float> Z;
  if (n < 1 || m < 1 || !read_array(argv[3], (size_t) n * 16, poses) || !read_array(argv[4], (size_t) n, fixed) ||
      !read_array(argv[5], (size_t) m, from) || !read_array(argv[6], (size_t) m, to) || !read_array(argv[7], (size_t) m * 16, Z)) {
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
  SolverPoseGraphHIP solver(ctx);
  CHECK(solver.param_algorithm.value() == SolverPoseGraphHIP::GaussNewton);
  solver.param_algorithm.setValue(SolverPoseGraphHIP::LevenbergMarquardt);
  solver.setGraph((size_t) n, poses.data(), fixed.data(), (size_t) (m - 1), from.data(), to.data(), Z.data());
  solver.addFactor(from[(size_t) m - 1], to[(size_t) m - 1], Z.data() + 16 * (size_t) (m - 1));
  solver.compute();
  const prs_pose_graph_lm_result& r = solver.resultLM();
  CHECK(solver.size() == (size_t) n);
  CHECK(r.status == PRS_OK);
  CHECK(r.linearizations >= 1 && solver.chi2() <= r.chi[0] && solver.chi2() == r.chi_final);
  CHECK(solver.iterations() == r.iterations && r.trials_total >= r.iterations);
  for (long i = 0; i < n; ++i) {
    if (fixed[(size_t) i]) {
      CHECK(std::memcmp(solver.pose((size_t) i), poses.data() + 16 * i, 16 * sizeof(double)) == 0);
    }
  }
  std::printf("iterations %d trials ", solver.iterations());
  for (int i = 0; i < PRS_POSE_GRAPH_MAX_ITERATIONS && r.trials[i] > 0; ++i) {
    std::printf("%s%d", i ? "," : "", r.trials[i]);
  }
  std::printf(" chi2 %.17g\n", solver.chi2());
  // an unknown algorithm is refused
  solver.param_algorithm.setValue(7);
  bool threw = false;
  try {
    solver.compute();
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  std::ofstream out(argv[8], std::ios::binary);
  out.write(reinterpret_cast<const char*>(solver.poses().data()), (std::streamsize) (solver.poses().size() * sizeof(double)));
  std::printf("%s\n", failures == 0 ? "all checks passed" : "checks failed");
  return failures == 0 ? 0 : 1;
}
