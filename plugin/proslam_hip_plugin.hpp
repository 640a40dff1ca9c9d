// proslam_hip_plugin.hpp -- C++ host side above the C-ABI (include/proslam_hip.h), mirroring the
// reference's operator surface for the tracking hot path: same member names, argument meaning and
// error behaviour as the srrg2 classes it stands in for, so call sites (and tests) read like the
// reference's own.  Header-only, C++11, depends only on libproslam_hip.so.
//
//   reference class (srrg2_proslam)                               -> class here
//   CorrespondenceFinderDescriptorBasedEpipolar<..>                -> CorrespondenceFinderDescriptorBasedEpipolarHIP
//     (CF/correspondence_finder_descriptor_based_epipolar.h:8-47)
//   CorrespondenceFinderDescriptorBasedBruteforce<..>              -> CorrespondenceFinderDescriptorBasedBruteforceHIP
//     (CF/correspondence_finder_descriptor_based_bruteforce.h:8-95)
//   CorrespondenceFinderProjective{KDTree,Square,Circle,Rhombus}   -> CorrespondenceFinderProjectiveHIP<SEARCH>
//     (CF/correspondence_finder_projective_base.h:14-155)
//   TriangulatorRigidStereo (mapping/triangulator_rigid_stereo.h)  -> TriangulatorRigidStereoHIP
//   SceneClipperProjective3D (mapping/scene_clipper_projective_3d.h) -> SceneClipperProjective3DHIP
//   MultiAligner3DQR + AlignerSliceProcessorProjective*            -> AlignerProjectiveHIP
//     (registration/aligner_slice_processor_projective.h:14-192, tests/test_aligners.cpp:1237-1253)
//   IntensityFeatureExtractorSelective{2D,3D}                      -> IntensityFeatureExtractorSelective{2D,3D}HIP
//     (sensor_processing/feature_extractors/intensity_feature_extractor_selective.h)
//   RawDataPreprocessorMonocularDepth                              -> RawDataPreprocessorMonocularDepthHIP
//     (sensor_processing/raw_data_preprocessor_monocular_depth.{h,cpp})
//   MultiAligner3DQR "loop_aligner" + AlignerSliceProcessor3D      -> AlignerSliceProcessor3DHIP
//     (registration/aligner_slice_processor_3d.hpp:7-22, the relocalize_aligner of the loop detector)
//   CorrespondenceFinderHBST_ (the loop detector's candidate search) -> CorrespondenceFinderPlaceHIP
//     (registration/correspondence_finders/correspondence_finder_hbst.{h,cpp}; exhaustive search in place of the HBST tree)
//   SLAMBenchmark::benchmarkCompute's status switch + LocalMapSplittingCriterionViewpoint3D -> LocalMapManagerHIP
//     (apps/app_benchmark.cpp:100-183; only with PROSLAM_HIP_WITH_HIP_RUNTIME: it owns device arrays, so it needs the HIP runtime)
//
// When the srrg2 headers are available the same bodies become real plugin subclasses: see
// INTEGRATION.md for the BOSS_REGISTER_CLASS adapters.  Points are AoS like the reference's
// PointIntensityDescriptor_<Dim> (coordinates, intensity, 32-byte descriptor row); the adapters
// gather them into the SoA layout the C-ABI takes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "proslam_hip.h"
#ifdef PROSLAM_HIP_WITH_HIP_RUNTIME
#include <hip/hip_runtime_api.h>
#endif

namespace proslam_hip {

// ---- the data model the reference's clouds reduce to on this path -------------------------------
template <int Dim_>
struct PointIntensityDescriptor_ {
  static constexpr int Dim = Dim_;
  float coords[Dim_];
  float intensity_value = 0.f;
  uint8_t descriptor_row[PRS_DESC_BYTES];  // cv::Mat 1x32 CV_8U in the reference
  uint32_t number_of_optimizations = 0;    // statistics().numberOfOptimizations()
  bool valid                        = true; // status == Valid
  float* coordinates() { return coords; }
  const float* coordinates() const { return coords; }
  uint8_t* descriptor() { return descriptor_row; }
  const uint8_t* descriptor() const { return descriptor_row; }
};
using PointIntensityDescriptor2f = PointIntensityDescriptor_<2>;
using PointIntensityDescriptor3f = PointIntensityDescriptor_<3>;
using PointIntensityDescriptor4f = PointIntensityDescriptor_<4>;
template <int Dim_>
using PointIntensityDescriptorVectorCloud = std::vector<PointIntensityDescriptor_<Dim_>>;

struct Correspondence {
  int fixed_idx;
  int moving_idx;
  float response;
};
using CorrespondenceVector = std::vector<Correspondence>;
static_assert(sizeof(Correspondence) == sizeof(prs_corr), "Correspondence must match prs_corr");

// PARAM(PropertyT, name, ...) stand-in: value() / setValue() like srrg2_core properties
template <typename T>
class Property_ {
public:
  explicit Property_(const T& v, bool* changed_flag = nullptr) : _v(v), _flag(changed_flag) {}
  const T& value() const { return _v; }
  void setValue(const T& v) {
    _v = v;
    if (_flag) *_flag = true;
  }

private:
  T _v;
  bool* _flag;
};
using PropertyFloat       = Property_<float>;
using PropertyUnsignedInt = Property_<uint64_t>;
using PropertyBool        = Property_<bool>;
using PropertyInt         = Property_<int>;

// one prs_context shared by the plugin objects of a process (one device, one stream)
class Context {
public:
  explicit Context(int device = 0) {
    // the header this adapter was compiled against and the library it loaded must describe the same structs
    if (PRS_ABI_CHECK() != PRS_OK) {
      throw std::runtime_error("proslam_hip::Context|ERROR: libproslam_hip.so (version " + std::to_string(prs_version()) +
                               ") does not match proslam_hip.h (version " + std::to_string(PRS_ABI_VERSION) + "): rebuild the plugin");
    }
    const int rc = prs_context_create(device, &_ctx);
    if (rc != PRS_OK) throw std::runtime_error(std::string("proslam_hip::Context|ERROR: ") + prs_status_string(rc));
  }
  ~Context() { prs_context_destroy(_ctx); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  prs_context* get() const { return _ctx; }

private:
  prs_context* _ctx = nullptr;
};
using ContextPtr = std::shared_ptr<Context>;

inline void warn(const char* who, int flags) {
  // the reference prints yellow warnings to std::cerr and returns (bruteforce_impl.cpp:217-226,237-242)
  if (flags & PRS_WARN_EMPTY_INPUT) std::cerr << who << "|WARNING: no points in fixed or moving" << std::endl;
  if (flags & PRS_WARN_NO_MATCHES) std::cerr << who << "|WARNING: no correspondences found" << std::endl;
  if (flags & PRS_WARN_LOW_RATIO) std::cerr << who << "|low matching ratio" << std::endl;
  if (flags & PRS_WARN_RETRIED) std::cerr << who << "|WARNING: bad initial guess - triggering internal repeat with increased search radius" << std::endl;
  if (flags & PRS_WARN_TRACK_LOST) std::cerr << who << "|WARNING: complete track loss - fallback to identity motion guess" << std::endl;
}

// ---- stereo epipolar matcher ---------------------------------------------------------------------
template <typename FixedType_, typename MovingType_>
class CorrespondenceFinderDescriptorBasedEpipolarHIP {
public:
  using FixedType  = FixedType_;
  using MovingType = MovingType_;
  explicit CorrespondenceFinderDescriptorBasedEpipolarHIP(ContextPtr ctx) : _ctx(std::move(ctx)) {}
  // CF/correspondence_finder_descriptor_based_bruteforce.h:22-36
  PropertyFloat param_maximum_descriptor_distance{50.0f};
  PropertyFloat param_maximum_distance_ratio_to_second_best{0.9f};
  PropertyFloat param_minimum_matching_ratio{0.25f};
  // CF/correspondence_finder_descriptor_based_epipolar.h:22-32
  PropertyUnsignedInt param_maximum_disparity_pixels{100};
  PropertyUnsignedInt param_epipolar_line_thickness_pixels{0};
  // extent of the row table (image rows); the reference needs none because it compare-sorts
  PropertyUnsignedInt param_image_rows{4096};
  PropertyUnsignedInt param_image_cols{0};  // reserved

  void setFixed(const FixedType* fixed_) {
    _fixed              = fixed_;
    _fixed_changed_flag = true;
  }
  void setMoving(const MovingType* moving_) {
    _moving              = moving_;
    _moving_changed_flag = true;
  }
  void setCorrespondences(CorrespondenceVector* correspondences_) { _correspondences = correspondences_; }

  void compute() {
    // _preCompute (CF/..bruteforce_impl.cpp:203-216)
    if (!_fixed) throw std::runtime_error("CorrespondenceFinderDescriptorBased::compute|ERROR: fixed not set");
    if (!_moving) throw std::runtime_error("CorrespondenceFinderDescriptorBased::compute|ERROR: moving not set");
    if (!_correspondences) throw std::runtime_error("CorrespondenceFinderDescriptorBased::compute|ERROR: correspondences not set");
    // unchanged inputs keep the last computation state (CF/..epipolar_impl.cpp:50-52)
    if (!_fixed_changed_flag && !_moving_changed_flag) return;
    std::vector<prs_kp2> kl(_fixed->size()), kr(_moving->size());
    std::vector<uint8_t> dl(_fixed->size() * PRS_DESC_BYTES), dr(_moving->size() * PRS_DESC_BYTES);
    for (size_t i = 0; i < _fixed->size(); ++i) {
      kl[i] = prs_kp2{(*_fixed)[i].coordinates()[0], (*_fixed)[i].coordinates()[1]};
      std::memcpy(&dl[i * PRS_DESC_BYTES], (*_fixed)[i].descriptor(), PRS_DESC_BYTES);
    }
    for (size_t i = 0; i < _moving->size(); ++i) {
      kr[i] = prs_kp2{(*_moving)[i].coordinates()[0], (*_moving)[i].coordinates()[1]};
      std::memcpy(&dr[i * PRS_DESC_BYTES], (*_moving)[i].descriptor(), PRS_DESC_BYTES);
    }
    prs_stereo_params p;
    p.maximum_descriptor_distance           = param_maximum_descriptor_distance.value();
    p.maximum_distance_ratio_to_second_best = param_maximum_distance_ratio_to_second_best.value();
    p.minimum_matching_ratio                = param_minimum_matching_ratio.value();
    p.maximum_disparity_pixels              = (int32_t) param_maximum_disparity_pixels.value();
    p.epipolar_line_thickness_pixels        = (int32_t) param_epipolar_line_thickness_pixels.value();
    p.image_rows                            = (int32_t) param_image_rows.value();
    p.image_cols                            = (int32_t) param_image_cols.value();
    _correspondences->clear();
    _correspondences->resize(_fixed->size() + 1);
    int32_t n    = 0;
    const int rc = prs_stereo_match(_ctx->get(), &p, kl.data(), dl.data(), (int32_t) kl.size(), kr.data(), dr.data(), (int32_t) kr.size(),
                                    reinterpret_cast<prs_corr*>(_correspondences->data()), (int32_t) _correspondences->size(), &n);
    if (rc < 0) {
      _correspondences->clear();
      throw std::runtime_error(std::string("CorrespondenceFinderDescriptorBasedEpipolarHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    }
    _correspondences->resize((size_t) n);
    warn("CorrespondenceFinderDescriptorBasedEpipolarHIP::compute", rc);
    // _postCompute (CF/..bruteforce_impl.cpp:231-236)
    _fixed_changed_flag = _moving_changed_flag = false;
  }

protected:
  ContextPtr _ctx;
  const FixedType* _fixed                 = nullptr;
  const MovingType* _moving               = nullptr;
  CorrespondenceVector* _correspondences = nullptr;
  bool _fixed_changed_flag = false, _moving_changed_flag = false;
};
using CorrespondenceFinderDescriptorBasedEpipolarHIP3D3D =
  CorrespondenceFinderDescriptorBasedEpipolarHIP<PointIntensityDescriptorVectorCloud<3>, PointIntensityDescriptorVectorCloud<3>>;
using CorrespondenceFinderDescriptorBasedEpipolarHIP2D2D =
  CorrespondenceFinderDescriptorBasedEpipolarHIP<PointIntensityDescriptorVectorCloud<2>, PointIntensityDescriptorVectorCloud<2>>;

// ---- bijective brute-force matcher -----------------------------------------------------------------
// CorrespondenceFinderDescriptorBasedBruteforce (CF/correspondence_finder_descriptor_based_bruteforce.h:8-95)
template <typename FixedType_, typename MovingType_>
class CorrespondenceFinderDescriptorBasedBruteforceHIP {
public:
  using FixedType  = FixedType_;
  using MovingType = MovingType_;
  explicit CorrespondenceFinderDescriptorBasedBruteforceHIP(ContextPtr ctx) : _ctx(std::move(ctx)) {}
  // CF/correspondence_finder_descriptor_based_bruteforce.h:22-36
  PropertyFloat param_maximum_descriptor_distance{50.0f};
  PropertyFloat param_maximum_distance_ratio_to_second_best{0.9f};
  PropertyFloat param_minimum_matching_ratio{0.25f};
  void setFixed(const FixedType* fixed_) {
    _fixed              = fixed_;
    _fixed_changed_flag = true;
  }
  void setMoving(const MovingType* moving_) {
    _moving              = moving_;
    _moving_changed_flag = true;
  }
  void setCorrespondences(CorrespondenceVector* correspondences_) { _correspondences = correspondences_; }
  void compute() {
    // _preCompute (CF/..bruteforce_impl.cpp:203-226)
    if (!_fixed) throw std::runtime_error("CorrespondenceFinderDescriptorBased::compute|ERROR: fixed not set");
    if (!_moving) throw std::runtime_error("CorrespondenceFinderDescriptorBased::compute|ERROR: moving not set");
    if (!_correspondences) throw std::runtime_error("CorrespondenceFinderDescriptorBased::compute|ERROR: correspondences not set");
    if (!_fixed_changed_flag && !_moving_changed_flag) return;  // :12-14
    std::vector<uint8_t> df(_fixed->size() * PRS_DESC_BYTES), dm(_moving->size() * PRS_DESC_BYTES);
    for (size_t i = 0; i < _fixed->size(); ++i) std::memcpy(&df[i * PRS_DESC_BYTES], (*_fixed)[i].descriptor(), PRS_DESC_BYTES);
    for (size_t i = 0; i < _moving->size(); ++i) std::memcpy(&dm[i * PRS_DESC_BYTES], (*_moving)[i].descriptor(), PRS_DESC_BYTES);
    prs_bruteforce_params p;
    p.maximum_descriptor_distance           = param_maximum_descriptor_distance.value();
    p.maximum_distance_ratio_to_second_best = param_maximum_distance_ratio_to_second_best.value();
    p.minimum_matching_ratio                = param_minimum_matching_ratio.value();
    _correspondences->clear();
    _correspondences->resize(std::min(_fixed->size(), _moving->size()) + 1);
    int32_t n    = 0;
    const int rc = prs_bruteforce_match(_ctx->get(), &p, df.data(), (int32_t) _fixed->size(), dm.data(), (int32_t) _moving->size(),
                                        reinterpret_cast<prs_corr*>(_correspondences->data()), (int32_t) _correspondences->size(), &n);
    if (rc < 0) {
      _correspondences->clear();
      throw std::runtime_error(std::string("CorrespondenceFinderDescriptorBasedBruteforceHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    }
    _correspondences->resize((size_t) n);
    warn("CorrespondenceFinderDescriptorBasedBruteforceHIP::compute", rc);
    _fixed_changed_flag = _moving_changed_flag = false;  // _postCompute (:231-236)
  }

protected:
  ContextPtr _ctx;
  const FixedType* _fixed                 = nullptr;
  const MovingType* _moving               = nullptr;
  CorrespondenceVector* _correspondences = nullptr;
  bool _fixed_changed_flag = false, _moving_changed_flag = false;
};
using CorrespondenceFinderDescriptorBasedBruteforceHIP3D3D =
  CorrespondenceFinderDescriptorBasedBruteforceHIP<PointIntensityDescriptorVectorCloud<3>, PointIntensityDescriptorVectorCloud<3>>;

// ---- pinhole projector parameters (PointProjectorPinhole_ as seen through param_projector) -------
struct ProjectorPinholeHIP {
  float camera_matrix[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // row-major K
  PropertyUnsignedInt param_canvas_cols{0};
  PropertyUnsignedInt param_canvas_rows{0};
  PropertyFloat param_range_min{0.3f};
  PropertyFloat param_range_max{20.0f};
  void setCameraMatrix(const float* K9) { std::memcpy(camera_matrix, K9, sizeof(camera_matrix)); }
  prs_projector raw() const {
    prs_projector p;
    p.fx = camera_matrix[0];
    p.fy = camera_matrix[4];
    p.cx = camera_matrix[2];
    p.cy = camera_matrix[5];
    p.canvas_cols = (int32_t) param_canvas_cols.value();
    p.canvas_rows = (int32_t) param_canvas_rows.value();
    p.range_min   = param_range_min.value();
    p.range_max   = param_range_max.value();
    return p;
  }
};
using ProjectorPinholeHIPPtr = std::shared_ptr<ProjectorPinholeHIP>;

// ---- projective finder ------------------------------------------------------------------------------
template <int SEARCH_, typename FixedType_, typename MovingType_>
class CorrespondenceFinderProjectiveHIP {
public:
  using FixedType  = FixedType_;
  using MovingType = MovingType_;
  explicit CorrespondenceFinderProjectiveHIP(ContextPtr ctx) : _ctx(std::move(ctx)), param_projector(new ProjectorPinholeHIP()) {}
  ~CorrespondenceFinderProjectiveHIP() {
    if (_h) prs_pcf_destroy(_h);
  }
  // CF/correspondence_finder_descriptor_based_bruteforce.h:22-36
  PropertyFloat param_maximum_descriptor_distance{50.0f};
  PropertyFloat param_maximum_distance_ratio_to_second_best{0.9f};
  PropertyFloat param_minimum_matching_ratio{0.25f};
  // CF/correspondence_finder_projective_base.h:30-74
  PropertyFloat param_minimum_descriptor_distance{25.0f, &_config_changed};
  PropertyFloat param_descriptor_distance_step_size_pixels{5.0f};
  PropertyUnsignedInt param_maximum_search_radius_pixels{100, &_config_changed};
  PropertyUnsignedInt param_minimum_search_radius_pixels{10};
  PropertyUnsignedInt param_search_radius_step_size_pixels{5};
  PropertyUnsignedInt param_minimum_number_of_iterations{10};
  PropertyFloat param_maximum_estimate_change_norm_for_convergence{1e-5f};
  PropertyUnsignedInt param_number_of_solver_iterations_per_projection{25};
  PropertyUnsignedInt param_minimum_number_of_points_per_cluster{10};  // KD-tree finder only (CF/..projective_kdtree.h:24-28)
  ProjectorPinholeHIPPtr param_projector;

  void setFixed(const FixedType* fixed_) {
    _fixed         = fixed_;
    _fixed_changed = true;
  }
  void setMoving(const MovingType* moving_) {
    _moving         = moving_;
    _moving_changed = true;
  }
  void setCorrespondences(CorrespondenceVector* correspondences_) { _correspondences = correspondences_; }
  void setLocalMapInSensor(const float* T16_row_major) { std::memcpy(_local_map_in_sensor, T16_row_major, sizeof(_local_map_in_sensor)); }
  void setSearchradiusPixels(const size_t& r) {  // CF/..projective_base.h:82-85
    ensureHandle();
    prs_pcf_set_search_radius(_h, r);
    _config_changed = false;
  }
  void setDescriptorDistance(const float& d) {  // CF/..projective_base.h:94-97
    ensureHandle();
    prs_pcf_set_descriptor_distance(_h, d);
    _config_changed = false;
  }
  size_t searchRadiusPixels() {
    prs_pcf_state s = state();
    return (size_t) s.search_radius_pixels;
  }
  prs_pcf_state state() {
    ensureHandle();
    prs_pcf_state s;
    prs_pcf_get_state(_h, &s);
    return s;
  }
  prs_pcf* handle() {
    ensureHandle();
    uploadIfChanged();
    return _h;
  }
  prs_pcf_params rawParams() const {
    prs_pcf_params p;
    p.maximum_descriptor_distance                  = param_maximum_descriptor_distance.value();
    p.maximum_distance_ratio_to_second_best        = param_maximum_distance_ratio_to_second_best.value();
    p.minimum_matching_ratio                       = param_minimum_matching_ratio.value();
    p.minimum_descriptor_distance                  = param_minimum_descriptor_distance.value();
    p.descriptor_distance_step_size_pixels         = param_descriptor_distance_step_size_pixels.value();
    p.maximum_search_radius_pixels                 = param_maximum_search_radius_pixels.value();
    p.minimum_search_radius_pixels                 = param_minimum_search_radius_pixels.value();
    p.search_radius_step_size_pixels               = param_search_radius_step_size_pixels.value();
    p.minimum_number_of_iterations                 = param_minimum_number_of_iterations.value();
    p.maximum_estimate_change_norm_for_convergence = param_maximum_estimate_change_norm_for_convergence.value();
    p.number_of_solver_iterations_per_projection   = param_number_of_solver_iterations_per_projection.value();
    p.search_type                                  = SEARCH_;
    p.projector                                    = param_projector->raw();
    p.minimum_number_of_points_per_cluster         = (int32_t) param_minimum_number_of_points_per_cluster.value();
    return p;
  }

  void compute() {
    if (!_fixed) throw std::runtime_error("CorrespondenceFinderDescriptorBased::compute|ERROR: fixed not set");
    if (!_moving) throw std::runtime_error("CorrespondenceFinderDescriptorBased::compute|ERROR: moving not set");
    if (!_correspondences) throw std::runtime_error("CorrespondenceFinderDescriptorBased::compute|ERROR: correspondences not set");
    if (!param_projector) throw std::runtime_error("CorrespondenceFinderProjective::compute|ERROR: projector not set");
    ensureHandle();
    uploadIfChanged();
    prs_pcf_set_local_map_in_sensor(_h, _local_map_in_sensor);
    std::vector<prs_corr> out(_fixed->size() + 1);
    int32_t n    = 0;
    const int rc = prs_pcf_compute(_h, out.data(), (int32_t) out.size(), &n);
    if (rc < 0) throw std::runtime_error(std::string("CorrespondenceFinderProjectiveHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    _correspondences->assign(reinterpret_cast<Correspondence*>(out.data()), reinterpret_cast<Correspondence*>(out.data()) + n);
    warn("CorrespondenceFinderProjectiveHIP::compute", rc & ~PRS_WARN_LOW_RATIO);
  }

protected:
  void ensureHandle() {
    if (!_h) {
      prs_pcf_params p = rawParams();
      const int rc     = prs_pcf_create(_ctx->get(), &p, &_h);
      if (rc != PRS_OK) throw std::runtime_error("CorrespondenceFinderProjectiveHIP|ERROR: cannot create finder handle");
      _config_changed = false;
    } else if (_config_changed) {
      prs_pcf_params p = rawParams();
      prs_pcf_set_params(_h, &p);
      _config_changed = false;
    }
  }
  void uploadIfChanged() {
    if (_fixed && _fixed_changed) {
      std::vector<float> c(_fixed->size() * FixedType::value_type::Dim);
      std::vector<uint8_t> d(_fixed->size() * PRS_DESC_BYTES);
      for (size_t i = 0; i < _fixed->size(); ++i) {
        std::memcpy(&c[i * FixedType::value_type::Dim], (*_fixed)[i].coordinates(), sizeof(float) * FixedType::value_type::Dim);
        std::memcpy(&d[i * PRS_DESC_BYTES], (*_fixed)[i].descriptor(), PRS_DESC_BYTES);
      }
      if (prs_pcf_set_fixed(_h, c.data(), FixedType::value_type::Dim, d.data(), (int32_t) _fixed->size()) < 0)
        throw std::runtime_error("CorrespondenceFinderProjectiveHIP|ERROR: set_fixed failed");
      _fixed_changed = false;
    }
    if (_moving && _moving_changed) {
      std::vector<float> c(_moving->size() * 3), s(_moving->size());
      std::vector<uint8_t> d(_moving->size() * PRS_DESC_BYTES);
      std::vector<uint32_t> nopt(_moving->size());
      for (size_t i = 0; i < _moving->size(); ++i) {
        std::memcpy(&c[i * 3], (*_moving)[i].coordinates(), sizeof(float) * 3);
        std::memcpy(&d[i * PRS_DESC_BYTES], (*_moving)[i].descriptor(), PRS_DESC_BYTES);
        nopt[i] = (*_moving)[i].number_of_optimizations;
      }
      // setupFactor's information scaling by landmark age (aligner_slice_processor_projective.cpp:46-52)
      prs_info_scale_from_nopt(nopt.data(), (int32_t) nopt.size(), s.data());
      if (prs_pcf_set_moving(_h, c.data(), s.data(), d.data(), (int32_t) _moving->size()) < 0)
        throw std::runtime_error("CorrespondenceFinderProjectiveHIP|ERROR: set_moving failed");
      _moving_changed = false;
    }
  }
  ContextPtr _ctx;
  prs_pcf* _h                            = nullptr;
  const FixedType* _fixed                = nullptr;
  const MovingType* _moving              = nullptr;
  CorrespondenceVector* _correspondences = nullptr;
  bool _fixed_changed = false, _moving_changed = false;
  bool _config_changed          = true;  // CF/..projective_base.h:134
  float _local_map_in_sensor[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};
template <typename F, typename M>
using CorrespondenceFinderProjectiveKDTreeHIP = CorrespondenceFinderProjectiveHIP<PRS_SEARCH_KDTREE, F, M>;
template <typename F, typename M>
using CorrespondenceFinderProjectiveSquareHIP = CorrespondenceFinderProjectiveHIP<PRS_SEARCH_SQUARE, F, M>;
template <typename F, typename M>
using CorrespondenceFinderProjectiveCircleHIP = CorrespondenceFinderProjectiveHIP<PRS_SEARCH_CIRCLE, F, M>;
template <typename F, typename M>
using CorrespondenceFinderProjectiveRhombusHIP = CorrespondenceFinderProjectiveHIP<PRS_SEARCH_RHOMBUS, F, M>;
using CorrespondenceFinderProjectiveCircleHIP4D3D =
  CorrespondenceFinderProjectiveCircleHIP<PointIntensityDescriptorVectorCloud<4>, PointIntensityDescriptorVectorCloud<3>>;
using CorrespondenceFinderProjectiveCircleHIP2D3D =
  CorrespondenceFinderProjectiveCircleHIP<PointIntensityDescriptorVectorCloud<2>, PointIntensityDescriptorVectorCloud<3>>;

// ---- triangulator -----------------------------------------------------------------------------------
class TriangulatorRigidStereoHIP {
public:
  using MeasurementType = PointIntensityDescriptorVectorCloud<4>;
  using DestType        = PointIntensityDescriptorVectorCloud<3>;
  explicit TriangulatorRigidStereoHIP(ContextPtr ctx) : _ctx(std::move(ctx)) {}
  PropertyFloat param_minimum_disparity_pixels{1.0f};               // mapping/triangulator_rigid_stereo.h:34-38
  PropertyFloat param_infinity_depth_meters{1.8446743e19f};         // :39-43 sqrt(FLT_MAX)
  ProjectorPinholeHIPPtr param_projector;
  void setDest(DestType* dest_) { _dest = dest_; }
  void setMoving(const MeasurementType* matches_) { _stereo_intensity_matches = matches_; }
  // platform->getTransform(camera_right in camera_left).translation(), mapping/triangulator_rigid_stereo.cpp:103-106
  void setBaselineRightInLeftMeters(float tx, float ty, float tz) {
    _t[0] = tx;
    _t[1] = ty;
    _t[2] = tz;
    _baseline_set = false;
  }
  void initializeBaseline() {
    if (_baseline_set || !param_projector) return;
    const float* K = param_projector->camera_matrix;
    for (int r = 0; r < 3; ++r) _baseline_right_in_left[r] = K[3 * r] * _t[0] + K[3 * r + 1] * _t[1] + K[3 * r + 2] * _t[2];
    _baseline_set = true;
  }
  const float* baselineRigthInLeft() const { return _baseline_right_in_left; }
  const std::vector<size_t>& indicesInvalidated() const { return _indices_invalidated; }
  void compute() {
    if (!_stereo_intensity_matches) {  // mapping/triangulator_rigid_stereo.cpp:9-16: log + return
      std::cerr << "TriangulatorRigidStereo::compute|ERROR: input not set" << std::endl;
      return;
    }
    if (!_dest) {
      std::cerr << "TriangulatorRigidStereo::compute|ERROR: result buffer not set" << std::endl;
      return;
    }
    initializeBaseline();
    const size_t n = _stereo_intensity_matches->size();
    std::vector<float> uvuv(n * 4), xyz(n * 3);
    std::vector<uint8_t> valid(n);
    for (size_t i = 0; i < n; ++i) std::memcpy(&uvuv[i * 4], (*_stereo_intensity_matches)[i].coordinates(), sizeof(float) * 4);
    prs_triangulator_params p;
    const float* K = param_projector->camera_matrix;
    p.fx = K[0];
    p.fy = K[4];
    p.cx = K[2];
    p.cy = K[5];
    p.b_x = _baseline_right_in_left[0];
    p.minimum_disparity_pixels = param_minimum_disparity_pixels.value();
    p.infinity_depth_meters    = param_infinity_depth_meters.value();
    const int rc = prs_triangulate(_ctx->get(), &p, uvuv.data(), (int32_t) n, xyz.data(), valid.data());
    if (rc < 0) throw std::runtime_error(std::string("TriangulatorRigidStereoHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    _dest->clear();
    _dest->resize(n);
    _indices_invalidated.clear();
    for (size_t i = 0; i < n; ++i) {
      PointIntensityDescriptor3f& d = (*_dest)[i];
      d.valid                      = valid[i] != 0;
      std::memcpy(d.coords, &xyz[i * 3], sizeof(float) * 3);
      if (d.valid) {  // descriptor + intensity of the left measurement are kept (:49-50)
        std::memcpy(d.descriptor_row, (*_stereo_intensity_matches)[i].descriptor(), PRS_DESC_BYTES);
        d.intensity_value = (*_stereo_intensity_matches)[i].intensity_value;
      } else {
        _indices_invalidated.push_back(i);
      }
    }
  }

protected:
  ContextPtr _ctx;
  const MeasurementType* _stereo_intensity_matches = nullptr;
  DestType* _dest                                  = nullptr;
  float _t[3]                       = {0, 0, 0};
  float _baseline_right_in_left[3] = {0, 0, 0};
  bool _baseline_set               = false;
  std::vector<size_t> _indices_invalidated;
};

// ---- aligner: MultiAligner3DQR with one projective slice -------------------------------------------
template <typename FinderType_>
class AlignerProjectiveHIP {
public:
  enum Status { Fail = 0, Success = 1 };
  using FixedType  = typename FinderType_::FixedType;
  using MovingType = typename FinderType_::MovingType;
  explicit AlignerProjectiveHIP(ContextPtr ctx) : _ctx(ctx), param_finder(new FinderType_(ctx)) {}
  std::shared_ptr<FinderType_> param_finder;      // slice->param_finder
  PropertyUnsignedInt param_max_iterations{10};   // MultiAligner3DQR
  PropertyUnsignedInt param_min_num_inliers{6};
  PropertyUnsignedInt param_min_num_correspondences{0};
  PropertyFloat param_damping{0.0f};              // IterationAlgorithmGN
  PropertyFloat param_chi_threshold{100.0f * 100.0f};  // RobustifierSaturated (aligner_slice_processor_projective.cpp:18)
  float param_diagonal_info_matrix[3]     = {1, 1, 1};
  bool param_enable_inverse_depth_weighting = false;
  float baseline_left_in_right_pixels[3]    = {0, 0, 0};  // K * t_left_in_right (aligner_slice_processor_projective.cpp:98-104)
  // MultiAligner3DQR flags the RGB-D configurations switch on (configurations/icl.conf:50-64, tum.conf:90-104)
  PropertyBool param_enable_inlier_only_runs{false};
  PropertyBool param_keep_only_inlier_correspondences{false};
  // readings of the un-vendored srrg2_solver arithmetic (include/proslam_hip.h, prs_aligner_params): 0 = the family
  // this library ships; a maintainer whose srrg2_solver does otherwise selects the other reading here (or in the .conf)
  PropertyInt param_robustifier_kernel_weight_form{PRS_KERNEL_WEIGHT_INV_CHI};     // RobustifierSaturated: Omega / chi | Omega * tau / chi
  PropertyFloat param_step_norm_exit{0.f};  // OPT-IN, not a parameter of the reference: leave the loop once the finder has latched and |dx| is below this (0 = off)
  PropertyInt param_damping_form{PRS_DAMPING_DIAG};                                // IterationAlgorithmGN: H + lambda diag(H) | H + lambda I
  PropertyInt param_translation_weight_form{PRS_TRANSLATION_WEIGHT_OFFSET};        // min(0.01 + d / mean, 1) | clamp(d / mean, 0.01, 1)
  // AlignerSliceMotionModel3D (kitti.conf:747-772): prior on movingInFixed around setMotionPriorMean() (identity by default)
  PropertyBool param_enable_motion_model_slice{false};
  float param_motion_model_information[6] = {1, 1, 1, 1, 1, 1};

  // the ...WithSensor slice processors read sensor_in_robot from the Platform (setPlatform,
  // aligner_slice_processor_projective.h:80-83): row-major 4x4; the estimate is then the ROBOT's movingInFixed
  void setSensorInRobot(const float* T16_row_major) {
    std::memcpy(_sensor_in_robot, T16_row_major, sizeof(_sensor_in_robot));
    _with_sensor = true;
  }
  void setMotionPriorMean(const float* T16_row_major) { prs_pcf_set_motion_prior_mean(param_finder->handle(), T16_row_major); }

  void setFixed(const FixedType* fixed_) { param_finder->setFixed(fixed_); _n_fixed = fixed_ ? fixed_->size() : 0; }
  void setMoving(const MovingType* moving_) { param_finder->setMoving(moving_); }
  void setMovingInFixed(const float* T16_row_major) { std::memcpy(_moving_in_fixed, T16_row_major, sizeof(_moving_in_fixed)); }
  const float* movingInFixed() const { return _moving_in_fixed; }
  Status status() const { return _status; }
  const CorrespondenceVector& correspondences() const { return _correspondences; }
  const prs_align_result& result() const { return _result; }

  void compute() {
    prs_aligner_params a;
    std::memset(&a, 0, sizeof(a));
    const prs_projector pr = param_finder->param_projector->raw();
    a.factor_type = FixedType::value_type::Dim;
    a.fx = pr.fx; a.fy = pr.fy; a.cx = pr.cx; a.cy = pr.cy;
    a.image_cols = (float) pr.canvas_cols;
    a.image_rows = (float) pr.canvas_rows;
    for (int i = 0; i < 3; ++i) {
      a.baseline_left_in_right_px[i] = baseline_left_in_right_pixels[i];
      a.diagonal_info[i]             = param_diagonal_info_matrix[i];
    }
    a.chi_threshold                  = param_chi_threshold.value();
    a.enable_inverse_depth_weighting = param_enable_inverse_depth_weighting ? 1 : 0;
    a.mean_disparity                 = -1.0f;  // bindFixed: computed over all fixed points on the device
    a.damping                        = param_damping.value();
    a.max_iterations                 = (int32_t) param_max_iterations.value();
    a.min_num_inliers                = (int32_t) param_min_num_inliers.value();
    a.min_num_correspondences        = (int32_t) param_min_num_correspondences.value();
    a.stop_at_fixed_point            = 1;
    a.enable_inlier_only_runs          = param_enable_inlier_only_runs.value() ? 1 : 0;
    a.keep_only_inlier_correspondences = param_keep_only_inlier_correspondences.value() ? 1 : 0;
    a.with_sensor                      = _with_sensor ? 1 : 0;
    std::memcpy(a.sensor_in_robot, _sensor_in_robot, sizeof(_sensor_in_robot));
    a.kernel_weight_form      = (int32_t) param_robustifier_kernel_weight_form.value();
    a.damping_form            = (int32_t) param_damping_form.value();
    a.step_norm_exit          = param_step_norm_exit.value();
    a.translation_weight_form = (int32_t) param_translation_weight_form.value();
    a.enable_motion_prior = param_enable_motion_model_slice.value() ? 1 : 0;
    for (int i = 0; i < 6; ++i) a.motion_prior_info[i] = param_motion_model_information[i];
    std::vector<prs_corr> out(_n_fixed + 1);
    int32_t n = 0;
    float X[16];
    const int rc = prs_pcf_align(param_finder->handle(), &a, _moving_in_fixed, nullptr, X, out.data(), (int32_t) out.size(), &n, &_result);
    if (rc < 0) throw std::runtime_error(std::string("AlignerProjectiveHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    std::memcpy(_moving_in_fixed, X, sizeof(X));
    _correspondences.assign(reinterpret_cast<Correspondence*>(out.data()), reinterpret_cast<Correspondence*>(out.data()) + n);
    _status = _result.status ? Success : Fail;
  }

protected:
  ContextPtr _ctx;
  size_t _n_fixed = 0;
  float _moving_in_fixed[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float _sensor_in_robot[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  bool _with_sensor          = false;
  Status _status = Fail;
  CorrespondenceVector _correspondences;
  prs_align_result _result;
};

// ---- scene clipper ----------------------------------------------------------------------------------
// SceneClipperProjective3D (mapping/scene_clipper_projective_3d.h:10-43, .cpp:9-67)
class SceneClipperProjective3DHIP {
public:
  using SceneType = PointIntensityDescriptorVectorCloud<3>;
  enum Status { Error = 0, Ready = 1, Successful = 2 };
  explicit SceneClipperProjective3DHIP(ContextPtr ctx) : _ctx(std::move(ctx)), param_projector(new ProjectorPinholeHIP()) {
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(_robot_in_local_map, I, sizeof(I));
    std::memcpy(_sensor_in_robot, I, sizeof(I));
  }
  void setFullScene(const SceneType* full_scene_) { _full_scene = full_scene_; }
  void setClippedSceneInRobot(SceneType* clipped_) { _clipped_scene_in_robot = clipped_; }
  void setRobotInLocalMap(const float* T16) { std::memcpy(_robot_in_local_map, T16, sizeof(_robot_in_local_map)); }
  void setSensorInRobot(const float* T16) { std::memcpy(_sensor_in_robot, T16, sizeof(_sensor_in_robot)); }
  const std::vector<int> globalIndices() const { return _global_indices; }
  Status status() const { return _status; }
  void compute() {
    _status = Error;
    if (!param_projector) throw std::runtime_error("SceneClipperProjective3D::compute|ERROR: missing projector");
    if (!_clipped_scene_in_robot) throw std::runtime_error("SceneClipperProjective3D::compute|ERROR: missing clipped scene");
    if (!_full_scene) throw std::runtime_error("SceneClipperProjective3D::compute|ERROR: missing global scene");
    if (_full_scene->empty()) {  // scene_clipper_projective_3d.cpp:21-28: nothing is cleared
      std::cerr << "SceneClipperProjective3D::compute|WARNING: global scene is empty, no clipping will be performed" << std::endl;
      _status = Ready;
      return;
    }
    const size_t n = _full_scene->size();
    std::vector<float> xyzw(4 * n), out(4 * n);
    std::vector<uint8_t> desc(PRS_DESC_BYTES * n), odesc(PRS_DESC_BYTES * n);
    std::vector<int32_t> idx(n);
    for (size_t i = 0; i < n; ++i) {  // AoS -> SoA gather; w carries the index so the other fields can be copied back
      std::memcpy(&xyzw[4 * i], (*_full_scene)[i].coords, sizeof(float) * 3);
      xyzw[4 * i + 3] = 0.f;
      std::memcpy(&desc[PRS_DESC_BYTES * i], (*_full_scene)[i].descriptor_row, PRS_DESC_BYTES);
    }
    const prs_projector p = param_projector->raw();
    int32_t m             = 0;
    const int rc = prs_scene_clip(_ctx->get(), &p, _robot_in_local_map, _sensor_in_robot, xyzw.data(), desc.data(), (int32_t) n,
                                  out.data(), odesc.data(), idx.data(), (int32_t) n, &m);
    if (rc < 0) throw std::runtime_error(std::string("SceneClipperProjective3DHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    _clipped_scene_in_robot->clear();
    _global_indices.clear();
    _clipped_scene_in_robot->reserve((size_t) m);
    for (int32_t k = 0; k < m; ++k) {
      PointIntensityDescriptor3f q = (*_full_scene)[(size_t) idx[k]];  // intensity, statistics, descriptor travel with the point
      std::memcpy(q.coords, &out[4 * (size_t) k], sizeof(float) * 3);
      _clipped_scene_in_robot->push_back(q);
      _global_indices.push_back(idx[k]);
    }
    if (rc & PRS_WARN_NO_PROJECTION) std::cerr << "SceneClipperProjective3D::compute|WARNING: clipped empty scene" << std::endl;
    _status = Successful;
  }
  ProjectorPinholeHIPPtr param_projector;

protected:
  ContextPtr _ctx;
  const SceneType* _full_scene       = nullptr;
  SceneType* _clipped_scene_in_robot = nullptr;
  float _robot_in_local_map[16];
  float _sensor_in_robot[16];
  std::vector<int> _global_indices;
  Status _status = Error;
};

// IntensityFeatureExtractorBinned_ (sensor_processing/feature_extractors/intensity_feature_extractor_binned.{h,cpp},
// base class intensity_feature_extractor_base.h): same PARAM names, setFeatures() / compute(image); the image is a plain
// 8-bit buffer here where the reference takes a cv::Mat.  Features are (u, v) points with intensity and a 256-bit descriptor.
class IntensityFeatureExtractorBinnedHIP {
public:
  using PointCloudType = PointIntensityDescriptorVectorCloud<2>;
  explicit IntensityFeatureExtractorBinnedHIP(ContextPtr ctx) : _ctx(std::move(ctx)) {}
  PropertyFloat param_detector_threshold{10.f};                  // intensity_feature_extractor_base.h:36-40
  PropertyBool param_enable_non_maximum_suppression{true};       // :48-52
  Property_<int> param_target_number_of_keypoints{500};          // :54-58
  PropertyUnsignedInt param_number_of_detectors_vertical{1};     // intensity_feature_extractor_binned.h:17-22
  PropertyUnsignedInt param_number_of_detectors_horizontal{1};   // :23-28
  // which members of a response class survive the per-region cut: the reference's std::sort order (GCC) by default
  Property_<int> param_selection_order{PRS_SELECT_LIBSTDCXX};
  void setFeatures(PointCloudType* features_) { _features = features_; }
  void compute(const uint8_t* image, int rows, int cols, int pitch) {
    if (!image || rows <= 0 || cols <= 0) throw std::runtime_error("IntensityFeatureExtractor::compute|ERROR: image not set");
    if (!_features) throw std::runtime_error("IntensityFeatureExtractor::compute|ERROR: target feature buffer not set");
    prs_extractor_params p;
    p.detector_threshold             = (int32_t) param_detector_threshold.value();
    p.enable_non_maximum_suppression = param_enable_non_maximum_suppression.value() ? 1 : 0;
    p.target_number_of_keypoints     = param_target_number_of_keypoints.value();
    p.number_of_detectors_vertical   = (int32_t) param_number_of_detectors_vertical.value();
    p.number_of_detectors_horizontal = (int32_t) param_number_of_detectors_horizontal.value();
    p.selection_order                = param_selection_order.value();
    p.max_raw_detections             = 32768;
    const int32_t capacity = 8192;
    std::vector<float> kp(2 * (size_t) capacity), inten((size_t) capacity);
    std::vector<uint8_t> desc(PRS_DESC_BYTES * (size_t) capacity);
    int32_t n    = 0;
    const int rc = prs_extract_features(_ctx->get(), &p, image, rows, cols, pitch, kp.data(), inten.data(), desc.data(), capacity, &n);
    if (rc < 0) throw std::runtime_error(std::string("IntensityFeatureExtractorBinnedHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    _features->clear();
    _features->reserve((size_t) n);
    for (int32_t i = 0; i < n; ++i) {
      PointIntensityDescriptor_<2> q;
      q.coords[0] = kp[2 * (size_t) i];
      q.coords[1] = kp[2 * (size_t) i + 1];
      q.intensity_value = inten[(size_t) i];
      std::memcpy(q.descriptor_row, &desc[PRS_DESC_BYTES * (size_t) i], PRS_DESC_BYTES);
      _features->push_back(q);
    }
  }

protected:
  ContextPtr _ctx;
  PointCloudType* _features = nullptr;
};

// IntensityFeatureExtractorSelective_ (sensor_processing/feature_extractors/intensity_feature_extractor_selective.{h,cpp}, base class
// intensity_feature_extractor_base.h): same PARAM names and defaults, setFeatures() / setProjections(points, radius) /
// setKeypointDetectionMask() / compute(image).  Projections are consumed by one compute() (selective.cpp:175-176), the external
// mask by the next one that does not return early.  Only the GFTT detector is built (detector_type "FAST", the reference's default,
// throws); target_bin_width_pixels must be a whole number of pixels.  The 3D cloud carries (u, v, 0).
template <int Dim_>
class IntensityFeatureExtractorSelectiveHIP_ {
public:
  using PointCloudType = PointIntensityDescriptorVectorCloud<Dim_>;
  explicit IntensityFeatureExtractorSelectiveHIP_(ContextPtr ctx) : _ctx(std::move(ctx)) {}
  Property_<std::string> param_descriptor_type{"ORB-256"};  // intensity_feature_extractor_base.h:24-28
  Property_<std::string> param_detector_type{"FAST"};       // :30-34
  PropertyFloat param_target_bin_width_pixels{10.f};        // :42-46
  Property_<int> param_target_number_of_keypoints{500};     // :54-58
  PropertyBool param_enable_full_distance_to_left{false};   // intensity_feature_extractor_selective.h:17-21
  PropertyBool param_enable_full_distance_to_right{false};  // :23-27
  PropertyBool param_enable_seeding_when_tracking{true};    // :29-33
  void setFeatures(PointCloudType* features_) { _features = features_; }
  void setProjections(const PointCloudType* projections_, const size_t& projection_detection_radius_) {
    _projections = projections_;
    _radius      = projection_detection_radius_;
  }
  // mask: rows x cols bytes (pitch `pitch`), non-zero = detect; seeding mode only.  The caller keeps it alive until compute().
  void setKeypointDetectionMask(const uint8_t* mask, int pitch) {
    _mask       = mask;
    _mask_pitch = pitch;
  }
  void compute(const uint8_t* image, int rows, int cols, int pitch) {
    if (!_features) {
      std::cerr << "IntensityFeatureExtractor::compute|WARNING: target feature buffer not set, ignoring call" << std::endl;
      return;
    }
    if (!image || rows <= 0 || cols <= 0) throw std::runtime_error("IntensityFeatureExtractor::compute|ERROR: image not set");
    prs_selective_extractor_params p;
    std::memset(&p, 0, sizeof(p));
    const std::string& det  = param_detector_type.value();
    const std::string& desc = param_descriptor_type.value();
    if (det == "GFTT") {
      p.detector_type = PRS_DETECTOR_GFTT;
    } else {
      throw std::runtime_error("IntensityFeatureExtractorSelectiveHIP::compute|ERROR: detector type not built: " + det);
    }
    if (desc == "ORB-256") {
      p.descriptor_type = PRS_DESCRIPTOR_ORB_256;
    } else if (desc == "BRIEF-256") {
      p.descriptor_type = PRS_DESCRIPTOR_BRIEF_256;
    } else {
      throw std::runtime_error("IntensityFeatureExtractorSelectiveHIP::compute|ERROR: descriptor type not built: " + desc);
    }
    const float width = param_target_bin_width_pixels.value();
    if (width < 0.f || width != std::floor(width)) {
      throw std::runtime_error("IntensityFeatureExtractorSelectiveHIP::compute|ERROR: target_bin_width_pixels must be a whole number");
    }
    p.target_number_of_keypoints    = param_target_number_of_keypoints.value();
    p.target_bin_width_pixels       = (int32_t) width;
    p.enable_full_distance_to_left  = param_enable_full_distance_to_left.value() ? 1 : 0;
    p.enable_full_distance_to_right = param_enable_full_distance_to_right.value() ? 1 : 0;
    p.enable_seeding_when_tracking  = param_enable_seeding_when_tracking.value() ? 1 : 0;
    p.max_candidates                = 16384;
    const bool tracking = _projections && !_projections->empty();
    std::vector<float> proj;
    if (tracking) {
      proj.reserve(2 * _projections->size());
      for (const auto& q : *_projections) {
        proj.push_back(q.coords[0]);
        proj.push_back(q.coords[1]);
      }
    }
    // the mask has the image's pitch on the device: repack it when the caller's differs
    std::vector<uint8_t> mask;
    const uint8_t* m = nullptr;
    if (!tracking && _mask) {
      mask.resize((size_t) rows * pitch);
      for (int r = 0; r < rows; ++r) std::memcpy(&mask[(size_t) r * pitch], _mask + (size_t) r * _mask_pitch, (size_t) cols);
      m = mask.data();
    }
    const int32_t capacity = 2 * 8192;
    std::vector<float> kp(2 * (size_t) capacity), inten((size_t) capacity);
    std::vector<uint8_t> d(PRS_DESC_BYTES * (size_t) capacity);
    int32_t n    = 0;
    const int rc = prs_extract_features_selective(_ctx->get(), &p, image, rows, cols, pitch, tracking ? proj.data() : nullptr,
                                                  tracking ? (int32_t) _projections->size() : 0, (int32_t) _radius, m, kp.data(),
                                                  inten.data(), d.data(), capacity, &n);
    if (rc < 0) throw std::runtime_error(std::string("IntensityFeatureExtractorSelectiveHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    _features->clear();
    _features->reserve((size_t) n);
    for (int32_t i = 0; i < n; ++i) {
      PointIntensityDescriptor_<Dim_> q;
      std::memset(q.coords, 0, sizeof(q.coords));
      q.coords[0]       = kp[2 * (size_t) i];
      q.coords[1]       = kp[2 * (size_t) i + 1];
      q.intensity_value = inten[(size_t) i];
      std::memcpy(q.descriptor_row, &d[PRS_DESC_BYTES * (size_t) i], PRS_DESC_BYTES);
      _features->push_back(q);
    }
    if (tracking) {
      if (n == 0) std::cerr << "IntensityFeatureExtractorSelective_::computeKeypoints|WARNING: no keypoints detected for projected regions: " << _projections->size();
      _projections = nullptr;  // selective.cpp:175-176: back to seeding for the next call
    } else if (n == 0) {
      std::cerr << "IntensityFeatureExtractorSelective_::computeKeypoints|WARNING: unable to seed keypoints" << std::endl;
      return;  // (the reference returns before clearing the mask here: selective.cpp:193-199)
    }
    _mask = nullptr;
  }

protected:
  ContextPtr _ctx;
  PointCloudType* _features          = nullptr;
  const PointCloudType* _projections = nullptr;
  size_t _radius                     = 0;
  const uint8_t* _mask               = nullptr;
  int _mask_pitch                    = 0;
};
using IntensityFeatureExtractorSelective2DHIP = IntensityFeatureExtractorSelectiveHIP_<2>;
using IntensityFeatureExtractorSelective3DHIP = IntensityFeatureExtractorSelectiveHIP_<3>;

// RawDataPreprocessorMonocularDepth (sensor_processing/raw_data_preprocessor_monocular_depth.{h,cpp}): same PARAM name and
// default, setMeas() / compute(); the intensity and depth images are plain buffers here where the reference takes ImageMessages,
// and the depth type (PRS_DEPTH_U16 = TYPE_16UC1, PRS_DEPTH_F32 = TYPE_32FC1) comes with the depth image as it does there.
// compute() runs the owned binned extractor, then the device depth lookup (prs_depth_measurements): features without depth are
// dropped, the others become (u, v, d) points in order.  status() is Ready, or Error when no feature is left (:131-136); the
// sparse-depth warning goes to std::cerr (:139-145).  An unknown depth type or a keypoint outside the depth image throws.
class RawDataPreprocessorMonocularDepthHIP {
public:
  using MeasurementType = PointIntensityDescriptorVectorCloud<3>;
  enum Status { Error = 0, Ready = 1 };
  explicit RawDataPreprocessorMonocularDepthHIP(ContextPtr ctx) : _ctx(ctx), _extractor(new IntensityFeatureExtractorBinnedHIP(ctx)) {}
  PropertyFloat param_depth_scaling_factor_to_meters{1.0f};  // raw_data_preprocessor_monocular_depth.h:26-30
  IntensityFeatureExtractorBinnedHIP& featureExtractor() { return *_extractor; }  // param_feature_extractor
  void setMeas(MeasurementType* meas_) { _meas = meas_; }
  Status status() const { return _status; }
  // intensity: rows x cols 8-bit (pitch bytes between rows); depth: depth_rows x depth_cols elements of depth_type
  void compute(const uint8_t* intensity, int rows, int cols, int pitch, const void* depth, int depth_rows, int depth_cols, int depth_pitch,
               int depth_type) {
    _status = Error;
    if (!intensity || !depth) throw std::runtime_error("RawDataPreprocessorMonocularDepth::compute|ERROR: measurement not set");
    if (!_meas) throw std::runtime_error("RawDataPreprocessorMonocularDepth::compute|ERROR: destination buffer not set");
    if (rows <= 0 || cols <= 0 || depth_rows <= 0 || depth_cols <= 0) {
      throw std::runtime_error("RawDataPreprocessorMonocularDepth::compute|ERROR: image has zero rows or columns");
    }
    _meas->clear();
    PointIntensityDescriptorVectorCloud<2> features;
    _extractor->setFeatures(&features);
    _extractor->compute(intensity, rows, cols, pitch);
    if (features.empty()) std::cerr << "RawDataPreprocessorMonocularDepth::compute|WARNING: no features found" << std::endl;
    const size_t n = features.size();
    std::vector<float> kp(2 * n + 2), inten(n + 1), uvd(3 * n + 3), inten_out(n + 1);
    std::vector<uint8_t> desc(PRS_DESC_BYTES * (n + 1)), desc_out(PRS_DESC_BYTES * (n + 1));
    for (size_t i = 0; i < n; ++i) {
      kp[2 * i]     = features[i].coords[0];
      kp[2 * i + 1] = features[i].coords[1];
      inten[i]      = features[i].intensity_value;
      std::memcpy(&desc[PRS_DESC_BYTES * i], features[i].descriptor_row, PRS_DESC_BYTES);
    }
    prs_depth_params p;
    p.depth_type                     = depth_type;
    p.depth_scaling_factor_to_meters = param_depth_scaling_factor_to_meters.value();
    int32_t k    = 0;
    const int rc = prs_depth_measurements(_ctx->get(), &p, depth, depth_rows, depth_cols, depth_pitch, kp.data(), inten.data(), desc.data(),
                                          (int32_t) n, uvd.data(), inten_out.data(), desc_out.data(), &k);
    if (rc < 0) throw std::runtime_error(std::string("RawDataPreprocessorMonocularDepthHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    _meas->reserve((size_t) k);
    for (int32_t i = 0; i < k; ++i) {
      PointIntensityDescriptor3f q;
      std::memcpy(q.coords, &uvd[3 * (size_t) i], 3 * sizeof(float));
      q.intensity_value = inten_out[(size_t) i];
      std::memcpy(q.descriptor_row, &desc_out[PRS_DESC_BYTES * (size_t) i], PRS_DESC_BYTES);
      _meas->push_back(q);
    }
    if (rc & PRS_WARN_NO_MATCHES) {
      std::cerr << "RawDataPreprocessorMonocularDepth::compute|WARNING: no adapted measurements generated" << std::endl;
      return;  // _status stays Error (:131-136)
    }
    if (rc & PRS_WARN_SPARSE_DEPTH) {
      std::cerr << "RawDataPreprocessorMonocularDepth::compute|WARNING: high number of points without depth: " << (n - (size_t) k) << "/" << n
                << std::endl;
    }
    _status = Ready;
  }

protected:
  ContextPtr _ctx;
  std::unique_ptr<IntensityFeatureExtractorBinnedHIP> _extractor;
  MeasurementType* _meas = nullptr;
  Status _status         = Error;
};

// MergerRigidStereoTriangulation with LandmarkEstimatorWeightedMean4D3D (mapping/mergers/merger_rigid_stereo_triangulation.h,
// merger_projective.h, landmarks/landmark_estimator_weighted_mean.h): same setters and PARAM names; the scene is mirrored into a
// device-resident map (prs_map) on setScene and read back after compute(), so a caller sees its scene cloud updated in place like
// with the reference object.  Other variants / estimators only differ in the prs_merger_params they fill.
class MergerRigidStereoTriangulationHIP {
public:
  using SceneType       = PointIntensityDescriptorVectorCloud<3>;
  using MeasurementType = PointIntensityDescriptorVectorCloud<4>;
  explicit MergerRigidStereoTriangulationHIP(ContextPtr ctx) : param_projector(new ProjectorPinholeHIP()), _ctx(std::move(ctx)) {
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(_measurement_in_scene, I, sizeof(I));
    std::memcpy(_measurement_in_world, I, sizeof(I));
  }
  ~MergerRigidStereoTriangulationHIP() {
    if (_map) prs_map_destroy(_map);
  }
  PropertyFloat param_maximum_distance_appearance{50.f};       // merger_projective.h:42-46
  PropertyUnsignedInt param_number_of_row_bins{10};            // :47-51
  PropertyUnsignedInt param_number_of_col_bins{30};            // :52-56
  PropertyFloat param_target_merge_ratio{0.5f};                // :57-61
  PropertyBool param_enable_binning{true};
  PropertyUnsignedInt param_target_number_of_merges{100};
  PropertyFloat param_maximum_distance_geometry_meters_squared{1.f};  // landmark_estimator_base.hpp:20-25 (of the landmark estimator)
  PropertyFloat param_minimum_disparity_pixels{1.f};           // triangulator_rigid_stereo.h:34-38 (of the triangulator)
  ProjectorPinholeHIPPtr param_projector;
  void setBaselineRightInLeftPixels(float bx) { _baseline_px = bx; }
  void setScene(SceneType* scene_) {
    _scene         = scene_;
    _scene_changed = true;
  }
  void setMeasurement(const MeasurementType* measurement_) { _measurement = measurement_; }
  void setCorrespondences(const CorrespondenceVector* correspondences_) { _correspondences = correspondences_; }
  void setMeasurementInScene(const float* T16) { std::memcpy(_measurement_in_scene, T16, sizeof(_measurement_in_scene)); }
  void setMeasurementInWorld(const float* T16) { std::memcpy(_measurement_in_world, T16, sizeof(_measurement_in_world)); }
  // pre-sizes the device-resident map (grown in place: landmark states, covariances and counters are kept)
  void reserve(size_t capacity) {
    if (_map && (int32_t) capacity > _capacity) {
      if (prs_map_reserve(_map, (int32_t) capacity) != PRS_OK) {
        throw std::runtime_error(std::string("MergerRigidStereoTriangulationHIP::reserve|ERROR: ") + prs_last_error(_ctx->get()));
      }
      _capacity = (int32_t) capacity;
    }
  }
  size_t numberOfMergedPoints() const { return _n_merged; }
  size_t numberOfAddedPoints() const { return _n_added; }
  void compute() {
    // merger_projective_impl.cpp:12-27
    if (!_scene) throw std::runtime_error("MergerProjective::compute|ERROR: scene not set");
    if (!_measurement) throw std::runtime_error("MergerProjective::compute|ERROR: measurement not set");
    if (!_correspondences) throw std::runtime_error("MergerProjective::compute|ERROR: correspondences not set");
    if (!param_projector) throw std::runtime_error("MergerProjective::compute|ERROR: projector not set");
    // room for this frame's additions.  After the first upload the DEVICE copy of the scene is the master (landmark states in
    // world coordinates, covariances, counters live there), so a map that has to grow is grown in place (prs_map_reserve keeps
    // every array); only setScene() makes the host scene authoritative again.
    int32_t on_device = 0;
    if (_map && !_scene_changed) prs_map_size(_map, &on_device, nullptr);
    const size_t scene_size = _scene_changed ? _scene->size() : (size_t) on_device;
    const int32_t capacity  = (int32_t) (scene_size + _measurement->size() + 1024);
    if (!_map) {
      _capacity    = 2 * capacity;
      const int rc = prs_map_create(_ctx->get(), _capacity, 0, 4096, 8192, &_map);
      if (rc != PRS_OK) throw std::runtime_error(std::string("MergerRigidStereoTriangulationHIP|ERROR: ") + prs_last_error(_ctx->get()));
      _scene_changed = true;
    } else if (capacity > _capacity) {
      _capacity = 2 * capacity;
      if (prs_map_reserve(_map, _capacity) != PRS_OK) {
        throw std::runtime_error(std::string("MergerRigidStereoTriangulationHIP|ERROR: ") + prs_last_error(_ctx->get()));
      }
    }
    if (_scene_changed) {  // upload the scene once; afterwards the device copy is the master
      const size_t n = _scene->size();
      std::vector<float> xyz(3 * n);
      std::vector<uint8_t> desc(PRS_DESC_BYTES * n);
      std::vector<uint32_t> nopt(n);
      for (size_t i = 0; i < n; ++i) {
        std::memcpy(&xyz[3 * i], (*_scene)[i].coords, sizeof(float) * 3);
        std::memcpy(&desc[PRS_DESC_BYTES * i], (*_scene)[i].descriptor_row, PRS_DESC_BYTES);
        nopt[i] = (*_scene)[i].number_of_optimizations;
      }
      prs_map_clear(_map);
      if (prs_map_set_scene(_map, xyz.data(), nullptr, nullptr, desc.data(), nopt.data(), nullptr, (int32_t) n) != PRS_OK) {
        throw std::runtime_error(std::string("MergerRigidStereoTriangulationHIP|ERROR: ") + prs_last_error(_ctx->get()));
      }
      _scene_changed = false;
    }
    prs_merger_params p;
    std::memset(&p, 0, sizeof(p));
    const float* K = param_projector->camera_matrix;
    p.variant                     = PRS_MERGER_STEREO_TRIANGULATION;
    p.enable_binning              = param_enable_binning.value() ? 1 : 0;
    p.number_of_row_bins          = (uint32_t) param_number_of_row_bins.value();
    p.number_of_col_bins          = (uint32_t) param_number_of_col_bins.value();
    p.canvas_rows                 = (int32_t) param_projector->param_canvas_rows.value();
    p.canvas_cols                 = (int32_t) param_projector->param_canvas_cols.value();
    p.maximum_distance_appearance = param_maximum_distance_appearance.value();
    p.target_number_of_merges     = (uint32_t) param_target_number_of_merges.value();
    p.target_merge_ratio          = param_target_merge_ratio.value();
    p.triangulator.fx = K[0];
    p.triangulator.fy = K[4];
    p.triangulator.cx = K[2];
    p.triangulator.cy = K[5];
    p.triangulator.b_x                      = _baseline_px;
    p.triangulator.minimum_disparity_pixels = param_minimum_disparity_pixels.value();
    p.triangulator.infinity_depth_meters    = 1.8446743e19f;
    p.fx = K[0];
    p.fy = K[4];
    p.cx = K[2];
    p.cy = K[5];
    p.estimator.type            = PRS_EST_WEIGHTED_MEAN;
    p.estimator.measurement_dim = 4;
    p.estimator.maximum_distance_geometry_meters_squared = param_maximum_distance_geometry_meters_squared.value();
    const size_t nm = _measurement->size();
    std::vector<float> z(4 * nm);
    std::vector<uint8_t> zd(PRS_DESC_BYTES * nm);
    for (size_t i = 0; i < nm; ++i) {
      std::memcpy(&z[4 * i], (*_measurement)[i].coords, sizeof(float) * 4);
      std::memcpy(&zd[PRS_DESC_BYTES * i], (*_measurement)[i].descriptor_row, PRS_DESC_BYTES);
    }
    static_assert(sizeof(Correspondence) == sizeof(prs_corr), "layout");
    prs_merge_result res;
    const int rc = prs_map_merge(_map, &p, _measurement_in_world, _measurement_in_scene, z.data(), zd.data(), (int32_t) nm,
                                 reinterpret_cast<const prs_corr*>(_correspondences->data()), (int32_t) _correspondences->size(), nullptr, 0, &res);
    if (rc < 0) throw std::runtime_error(std::string("MergerRigidStereoTriangulationHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    if (rc & PRS_WARN_NO_MATCHES) std::cerr << "MergerProjective::compute|WARNING: all merge attempts failed" << std::endl;
    _n_merged = (size_t) res.n_merged;
    _n_added  = (size_t) res.n_added;
    // mirror the scene back: element order intact, new points appended (merger_projective_impl.cpp:230-308)
    int32_t n = 0;
    prs_map_size(_map, &n, nullptr);
    std::vector<float> xyz(3 * (size_t) _capacity);
    std::vector<uint8_t> desc(PRS_DESC_BYTES * (size_t) _capacity);
    std::vector<uint32_t> nopt((size_t) _capacity);
    if (prs_map_get_scene(_map, _capacity, xyz.data(), nullptr, desc.data(), nopt.data(), nullptr, &n) != PRS_OK) {
      throw std::runtime_error(std::string("MergerRigidStereoTriangulationHIP|ERROR: ") + prs_last_error(_ctx->get()));
    }
    _scene->resize((size_t) n);
    for (int32_t i = 0; i < n; ++i) {
      std::memcpy((*_scene)[(size_t) i].coords, &xyz[3 * (size_t) i], sizeof(float) * 3);
      std::memcpy((*_scene)[(size_t) i].descriptor_row, &desc[PRS_DESC_BYTES * (size_t) i], PRS_DESC_BYTES);
      (*_scene)[(size_t) i].number_of_optimizations = nopt[(size_t) i];
    }
  }

protected:
  ContextPtr _ctx;
  prs_map* _map      = nullptr;
  int32_t _capacity  = 0;
  SceneType* _scene  = nullptr;
  bool _scene_changed = true;
  const MeasurementType* _measurement          = nullptr;
  const CorrespondenceVector* _correspondences = nullptr;
  float _measurement_in_scene[16];
  float _measurement_in_world[16];
  float _baseline_px = 0.f;
  size_t _n_merged = 0, _n_added = 0;
};

// ---- closure merger ---------------------------------------------------------------------------------------------------
// MergerCorrespondence_ (srrg2_slam_interfaces, not in the tree: BUILD-DEFINED rule, include/proslam_hip.h "Closure merger"): folds a
// measurement cloud into a scene through given correspondences, in place like the reference object.  PARAM names are the
// reference's; the base class's own defaults are not in the tree, so the values every shipped .conf sets stand in (kitti.conf:446-460),
// the bin counts are merger_projective.h:47-56.  KIND_ selects the measurement: 3D points (the tracker slice's closure_merger) or
// (u, v, d) behind the unprojector (mapping/mergers/merger_correspondence_projective_depth_3d.cpp:7-33).
struct UnprojectorPinholeHIP {
  PropertyUnsignedInt param_canvas_rows{0};
  PropertyUnsignedInt param_canvas_cols{0};
  float camera_matrix[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  void setCameraMatrix(const float* K9) { std::memcpy(camera_matrix, K9, sizeof(camera_matrix)); }
};
using UnprojectorPinholeHIPPtr = std::shared_ptr<UnprojectorPinholeHIP>;

template <int KIND_>
class MergerCorrespondenceHIP_ {
public:
  using SceneType       = PointIntensityDescriptorVectorCloud<3>;
  using MeasurementType = PointIntensityDescriptorVectorCloud<3>;
  explicit MergerCorrespondenceHIP_(ContextPtr ctx) : param_unprojector(new UnprojectorPinholeHIP()), _ctx(std::move(ctx)) {
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(_measurement_in_scene, I, sizeof(I));
  }
  PropertyBool param_enable_binning{true};
  PropertyFloat param_maximum_distance_geometry_squared{0.25f};
  PropertyFloat param_maximum_response{50.f};
  PropertyUnsignedInt param_target_number_of_merges{200};
  PropertyUnsignedInt param_number_of_row_bins{10};
  PropertyUnsignedInt param_number_of_col_bins{30};
  // camera matrix and canvas: the unprojector of the (u, v, d) form; for 3D measurements only the binning projects with them
  UnprojectorPinholeHIPPtr param_unprojector;
  void setScene(SceneType* scene_) { _scene = scene_; }
  void setMeasurement(const MeasurementType* measurement_) { _measurement = measurement_; }
  void setCorrespondences(const CorrespondenceVector* correspondences_) { _correspondences = correspondences_; }
  void setMeasurementInScene(const float* T16) { std::memcpy(_measurement_in_scene, T16, sizeof(_measurement_in_scene)); }
  size_t numberOfMergedPoints() const { return _n_merged; }
  size_t numberOfAddedPoints() const { return _n_added; }
  void compute() {
    if (!_scene) throw std::runtime_error("MergerCorrespondence::compute|ERROR: scene not set");
    if (!_measurement) throw std::runtime_error("MergerCorrespondence::compute|ERROR: measurement not set");
    if (!_correspondences) throw std::runtime_error("MergerCorrespondence::compute|ERROR: correspondences not set");
    if (!param_unprojector) throw std::runtime_error("MergerCorrespondence::compute|ERROR: unprojector not set");
    prs_closure_merger_params p;
    std::memset(&p, 0, sizeof(p));
    const float* K = param_unprojector->camera_matrix;
    p.measurement_kind   = KIND_;
    p.number_of_row_bins = (uint32_t) param_number_of_row_bins.value();
    p.number_of_col_bins = (uint32_t) param_number_of_col_bins.value();
    p.canvas_rows        = (int32_t) param_unprojector->param_canvas_rows.value();
    p.canvas_cols        = (int32_t) param_unprojector->param_canvas_cols.value();
    // (a merger whose canvas was never set cannot bin: the first gtest of the reference leaves it unset, tests/test_mergers.cpp:174-181)
    p.enable_binning = param_enable_binning.value() && p.canvas_rows > 0 && p.canvas_cols > 0 ? 1 : 0;
    p.fx = K[0];
    p.fy = K[4];
    p.cx = K[2];
    p.cy = K[5];
    p.maximum_distance_geometry_squared = param_maximum_distance_geometry_squared.value();
    p.maximum_response                  = param_maximum_response.value();
    p.target_number_of_merges           = (uint32_t) param_target_number_of_merges.value();
    const size_t n = _scene->size(), nm = _measurement->size(), cap = n + nm + 1;
    std::vector<float> xyz(4 * cap, 0.f), z(4 * (nm + 1), 0.f);
    std::vector<uint8_t> desc(PRS_DESC_BYTES * cap, 0), zd(PRS_DESC_BYTES * (nm + 1), 0);
    std::vector<uint32_t> nopt(cap, 0u);
    for (size_t i = 0; i < n; ++i) {
      std::memcpy(&xyz[4 * i], (*_scene)[i].coords, sizeof(float) * 3);
      std::memcpy(&desc[PRS_DESC_BYTES * i], (*_scene)[i].descriptor_row, PRS_DESC_BYTES);
      nopt[i] = (*_scene)[i].number_of_optimizations;
    }
    for (size_t i = 0; i < nm; ++i) {
      std::memcpy(&z[4 * i], (*_measurement)[i].coords, sizeof(float) * 3);
      std::memcpy(&zd[PRS_DESC_BYTES * i], (*_measurement)[i].descriptor_row, PRS_DESC_BYTES);
    }
    int32_t n_points = (int32_t) n;
    prs_merge_result res;
    const int rc = prs_closure_merge(_ctx->get(), &p, (int32_t) cap, &n_points, xyz.data(), desc.data(), nullptr, nullptr, nopt.data(), nullptr,
                                     nullptr, nullptr, z.data(), zd.data(), (int32_t) nm,
                                     reinterpret_cast<const prs_corr*>(_correspondences->data()), (int32_t) _correspondences->size(), 0,
                                     _measurement_in_scene, 0, &res);
    if (rc < 0) throw std::runtime_error(std::string("MergerCorrespondence::compute|ERROR: ") + prs_status_string(rc) + " " + prs_last_error(_ctx->get()));
    _n_merged = (size_t) res.n_merged;
    _n_added  = (size_t) res.n_added;
    // the scene in place: element order intact, new points appended
    _scene->resize((size_t) n_points);
    for (int32_t i = 0; i < n_points; ++i) {
      std::memcpy((*_scene)[(size_t) i].coords, &xyz[4 * (size_t) i], sizeof(float) * 3);
      std::memcpy((*_scene)[(size_t) i].descriptor_row, &desc[PRS_DESC_BYTES * (size_t) i], PRS_DESC_BYTES);
      (*_scene)[(size_t) i].number_of_optimizations = nopt[(size_t) i];
    }
  }

protected:
  ContextPtr _ctx;
  SceneType* _scene                            = nullptr;
  const MeasurementType* _measurement          = nullptr;
  const CorrespondenceVector* _correspondences = nullptr;
  float _measurement_in_scene[16];
  size_t _n_merged = 0, _n_added = 0;
};
using MergerCorrespondencePointIntensityDescriptor3fHIP = MergerCorrespondenceHIP_<PRS_CLOSURE_XYZ>;
using MergerCorrespondenceProjectiveDepth3DHIP          = MergerCorrespondenceHIP_<PRS_CLOSURE_UVD>;

// ---- loop aligner -----------------------------------------------------------------------------------
// MultiAligner3DQR "loop_aligner" with one AlignerSliceProcessor3D (registration/aligner_slice_processor_3d.hpp:7-22): point-to-point
// SE(3) registration of two 3D clouds through given correspondences (SE3Point2PointErrorFactor, Omega = I3), plus the loop
// detector's accept / reject verdict (kitti.conf:966-977).  Defaults: the kitti.conf loop aligner (:380-408, :938-978).
class AlignerSliceProcessor3DHIP {
public:
  enum Status { Fail = 0, Success = 1 };
  enum Robustifier { Clamp = PRS_ROBUSTIFIER_CLAMP, Saturated = PRS_ROBUSTIFIER_SATURATED };
  using CloudType = PointIntensityDescriptorVectorCloud<3>;
  explicit AlignerSliceProcessor3DHIP(ContextPtr ctx) : _ctx(std::move(ctx)) {}
  PropertyInt param_robustifier{Clamp};                  // slice->param_robustifier: RobustifierClamp / RobustifierSaturated
  PropertyFloat param_chi_threshold{3.0f};               // the robustifier's chi_threshold
  PropertyUnsignedInt param_min_num_correspondences{30};  // AlignerSliceProcessor3D
  PropertyUnsignedInt param_max_iterations{100};         // MultiAligner3DQR
  PropertyUnsignedInt param_min_num_inliers{10};
  PropertyFloat param_damping{0.0f};                     // IterationAlgorithmGN
  PropertyUnsignedInt param_relocalize_min_inliers{25};  // MultiLoopDetectorHBST3D / MultiRelocalizer3D verdict
  PropertyFloat param_relocalize_min_inliers_ratio{0.5f};
  PropertyFloat param_relocalize_max_chi_inliers{2.0f};

  void setFixed(const CloudType* fixed_) { _fixed = fixed_; }
  void setMoving(const CloudType* moving_) { _moving = moving_; }
  void setCorrespondences(const CorrespondenceVector* correspondences_) { _correspondences = correspondences_; }
  void setMovingInFixed(const float* T16_row_major) { std::memcpy(_moving_in_fixed, T16_row_major, sizeof(_moving_in_fixed)); }
  const float* movingInFixed() const { return _moving_in_fixed; }
  Status status() const { return _status; }
  bool accepted() const { return _result.accepted != 0; }
  const prs_point_align_result& result() const { return _result; }
  const std::vector<uint8_t>& inliers() const { return _inliers; }  // 1 = inlier at the last linearisation

  void compute() {
    if (!_fixed) throw std::runtime_error("AlignerSliceProcessor3DHIP::compute|ERROR: fixed not set");
    if (!_moving) throw std::runtime_error("AlignerSliceProcessor3DHIP::compute|ERROR: moving not set");
    if (!_correspondences) throw std::runtime_error("AlignerSliceProcessor3DHIP::compute|ERROR: correspondences not set");
    prs_point_align_params p;
    std::memset(&p, 0, sizeof(p));
    p.robustifier                  = (int32_t) param_robustifier.value();
    p.chi_threshold                = param_chi_threshold.value();
    p.damping                      = param_damping.value();
    p.max_iterations               = (int32_t) param_max_iterations.value();
    p.min_num_inliers              = (int32_t) param_min_num_inliers.value();
    p.min_num_correspondences      = (int32_t) param_min_num_correspondences.value();
    p.relocalize_min_inliers       = (int32_t) param_relocalize_min_inliers.value();
    p.relocalize_min_inliers_ratio = param_relocalize_min_inliers_ratio.value();
    p.relocalize_max_chi_inliers   = param_relocalize_max_chi_inliers.value();
    std::vector<float> f(_fixed->size() * 3), m(_moving->size() * 3);
    for (size_t i = 0; i < _fixed->size(); ++i) std::memcpy(&f[3 * i], (*_fixed)[i].coordinates(), 3 * sizeof(float));
    for (size_t i = 0; i < _moving->size(); ++i) std::memcpy(&m[3 * i], (*_moving)[i].coordinates(), 3 * sizeof(float));
    _inliers.assign(_correspondences->size(), 0);
    const int rc = prs_point_align(_ctx->get(), &p, f.data(), (int32_t) _fixed->size(), m.data(), (int32_t) _moving->size(),
                                   reinterpret_cast<const prs_corr*>(_correspondences->data()), (int32_t) _correspondences->size(),
                                   _moving_in_fixed, &_result, _inliers.data());
    if (rc < 0) throw std::runtime_error(std::string("AlignerSliceProcessor3DHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    warn("AlignerSliceProcessor3DHIP::compute", rc);
    _status = _result.status ? Success : Fail;
  }

protected:
  ContextPtr _ctx;
  const CloudType* _fixed                       = nullptr;
  const CloudType* _moving                      = nullptr;
  const CorrespondenceVector* _correspondences = nullptr;
  float _moving_in_fixed[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  Status _status             = Fail;
  prs_point_align_result _result{};
  std::vector<uint8_t> _inliers;
};

// ---- loop detector: candidate search --------------------------------------------------------------
// CorrespondenceFinderHBST_ (correspondence_finder_hbst.cpp:5-127) over the device place database: compute() queries every earlier local
// map, indices() lists the candidates (ascending), correspondences(i) holds candidate i's (query, reference, distance) triples, and
// addPreviousQuery() stores the last query's local map.  SUBSTITUTION: the HBST tree is searched exhaustively (include/proslam_hip.h);
// its leaf size, depth and partitioning parameters do not exist here.  Defaults: kitti.conf:938-978.
template <int Dim_>
class CorrespondenceFinderPlaceHIP {
public:
  using CloudType = PointIntensityDescriptorVectorCloud<Dim_>;
  explicit CorrespondenceFinderPlaceHIP(ContextPtr ctx) : _ctx(std::move(ctx)) {
    const int rc = prs_place_db_create(_ctx->get(), &_db);
    if (rc != PRS_OK) throw std::runtime_error(std::string("CorrespondenceFinderPlaceHIP|ERROR: ") + prs_status_string(rc));
  }
  ~CorrespondenceFinderPlaceHIP() { prs_place_db_destroy(_db); }
  CorrespondenceFinderPlaceHIP(const CorrespondenceFinderPlaceHIP&) = delete;
  CorrespondenceFinderPlaceHIP& operator=(const CorrespondenceFinderPlaceHIP&) = delete;
  PropertyFloat param_maximum_descriptor_distance{25.0f};
  PropertyUnsignedInt param_minimum_age_difference_to_candidates{10};
  PropertyInt param_relocalize_min_inliers{25};
  PropertyInt param_max_candidates{16};  // candidate slots per query (this build: a fixed-size output)

  // the local map's graph identifier and its points (status Valid = point.valid)
  void setCurrentLocalMapAndPoints(int64_t graph_id_, const CloudType* query_local_map_points_) {
    _graph_id = graph_id_;
    _query    = query_local_map_points_;
  }

  void compute() {
    _indices.clear();
    _correspondences.clear();
    if (!_query || _graph_id < 0) throw std::runtime_error("CorrespondenceFinderPlaceHIP::compute|ERROR: no local map set");
    prs_place_params p;
    std::memset(&p, 0, sizeof(p));
    p.maximum_descriptor_distance          = param_maximum_descriptor_distance.value();
    p.minimum_age_difference_to_candidates = param_minimum_age_difference_to_candidates.value();
    p.relocalize_min_inliers               = param_relocalize_min_inliers.value();
    p.max_candidates                       = param_max_candidates.value();
    const size_t n = _query->size();
    _desc.resize(n * PRS_DESC_BYTES);
    _xyz.assign(n * 3, 0.0f);
    _valid.resize(n);
    for (size_t i = 0; i < n; ++i) {
      std::memcpy(&_desc[i * PRS_DESC_BYTES], (*_query)[i].descriptor(), PRS_DESC_BYTES);
      std::memcpy(&_xyz[i * 3], (*_query)[i].coordinates(), (Dim_ < 3 ? Dim_ : 3) * sizeof(float));
      _valid[i] = (*_query)[i].valid ? 1 : 0;
    }
    int32_t maps = 0, rows = 0, big = 0;
    prs_place_db_size(_db, &maps, &rows, &big);
    const int32_t stride = big > 0 ? big : 1;
    std::vector<int32_t> cand((size_t) p.max_candidates), ncorr((size_t) p.max_candidates);
    std::vector<Correspondence> corr((size_t) p.max_candidates * (size_t) stride);
    int32_t nc = 0;
    const int rc = prs_place_query(_db, &p, _graph_id, _desc.data(), _valid.data(), (int32_t) n, cand.data(), &nc,
                                   reinterpret_cast<prs_corr*>(corr.data()), stride, ncorr.data(), nullptr);
    if (rc < 0) throw std::runtime_error(std::string("CorrespondenceFinderPlaceHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    if (rc & PRS_WARN_EMPTY_INPUT) std::cerr << "MultiLoopDetectorHBST::compute|WARNING: query descriptor vector is empty" << std::endl;
    _query_stored = rc & PRS_WARN_EMPTY_INPUT ? false : true;
    for (int32_t k = 0; k < nc; ++k) {
      _indices.push_back((size_t) cand[(size_t) k]);
      const Correspondence* first = corr.data() + (size_t) k * (size_t) stride;
      _correspondences.emplace_back(first, first + ncorr[(size_t) k]);
    }
  }

  // stores the last queried local map (graph id -> the next database index); a graph id already stored is left as it is
  void addPreviousQuery() {
    if (!_query_stored) return;
    _query_stored = false;
    const int rc = prs_place_db_add(_db, _graph_id, _xyz.data(), _desc.data(), _valid.data(), (int32_t) _valid.size());
    if (rc == PRS_ERR_RANGE) return;
    if (rc < 0) throw std::runtime_error(std::string("CorrespondenceFinderPlaceHIP::addPreviousQuery|ERROR: ") + prs_last_error(_ctx->get()));
  }

  const std::vector<size_t>& indices() const { return _indices; }
  // candidate i of indices(): correspondences (fixed = query point, moving = reference point, response = distance)
  CorrespondenceVector correspondences(size_t i) const { return _correspondences.at(i); }

protected:
  ContextPtr _ctx;
  prs_place_db* _db    = nullptr;
  int64_t _graph_id    = -1;
  const CloudType* _query = nullptr;
  bool _query_stored   = false;
  std::vector<uint8_t> _desc, _valid;
  std::vector<float> _xyz;
  std::vector<size_t> _indices;
  std::vector<CorrespondenceVector> _correspondences;
};


// ------------------------------------------------------------------------------------------------
// The global solver of the pose graph: Solver + IterationAlgorithmGN + SimpleTerminationCriteria as MultiGraphSLAM3D's
// `global_solver` uses them (kitti.conf:895-936), over prs_pose_graph_optimize; with param_algorithm = LevenbergMarquardt the
// IterationAlgorithmLM of icl.conf:665-685 / tum.conf:174-194, over prs_pose_graph_optimize_lm.  A graph is handed over as plain arrays: variable i is
// the i-th pose (VariableSE3QuaternionRight, estimate as a row-major 4x4 double), a factor is (from, to, measurement, information)
// (SE3PosePoseGeodesicErrorFactor).  setGraph() copies, compute() optimises, poses() / pose(i) give the estimates back.
class SolverPoseGraphHIP {
public:
  PropertyInt param_max_iterations{10};  // Solver max_iterations
  PropertyFloat param_damping{1e-6f};    // IterationAlgorithmGN damping
  PropertyFloat param_epsilon{1e-3f};    // SimpleTerminationCriteria epsilon
  PropertyInt param_damping_form{PRS_DAMPING_DIAG};
  enum Algorithm { GaussNewton = 0, LevenbergMarquardt = 1 };
  PropertyInt param_algorithm{GaussNewton};      // the class of the Solver's `algorithm`: IterationAlgorithmGN / IterationAlgorithmLM
  PropertyInt param_lm_iterations_max{100};      // IterationAlgorithmLM, used by LevenbergMarquardt only
  PropertyFloat param_step_high{0.666667f};
  PropertyFloat param_step_low{0.333333f};
  PropertyFloat param_tau{1e-5f};
  PropertyFloat param_user_lambda_init{0.f};
  PropertyInt param_variable_damping{1};

  explicit SolverPoseGraphHIP(ContextPtr ctx) : _ctx(std::move(ctx)) {}

  // poses16 [n][16] double, fixed [n] (nonzero = the variable is fixed), from / to [m], measurements16 [m][16] float,
  // information36 [m][36] float or nullptr (identity)
  void setGraph(size_t n, const double* poses16, const uint8_t* fixed, size_t m, const int32_t* from, const int32_t* to,
                const float* measurements16, const float* information36 = nullptr) {
    _poses.assign(poses16, poses16 + 16 * n);
    _fixed.assign(fixed, fixed + n);
    _from.assign(from, from + m);
    _to.assign(to, to + m);
    _z.assign(measurements16, measurements16 + 16 * m);
    _omega.clear();
    if (information36) _omega.assign(information36, information36 + 36 * m);
    _set = true;
  }

  // one closure (or odometry) edge more, e.g. an accepted verdict of the loop detector: measurement = X_from^-1 X_to
  void addFactor(int32_t from, int32_t to, const float* measurement16, const float* information36 = nullptr) {
    if (!_omega.empty() || information36) {
      static const float eye[36] = {1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1};
      if (_omega.empty()) {
        for (size_t k = 0; k < _from.size(); ++k) _omega.insert(_omega.end(), eye, eye + 36);
      }
      const float* o = information36 ? information36 : eye;
      _omega.insert(_omega.end(), o, o + 36);
    }
    _from.push_back(from);
    _to.push_back(to);
    _z.insert(_z.end(), measurement16, measurement16 + 16);
  }

  void compute() {
    if (!_set) throw std::runtime_error("SolverPoseGraphHIP::compute|ERROR: graph not set");
    if (param_algorithm.value() == LevenbergMarquardt) {
      computeLM();
      return;
    }
    if (param_algorithm.value() != GaussNewton) throw std::runtime_error("SolverPoseGraphHIP::compute|ERROR: unknown algorithm");
    prs_pose_graph_params p;
    std::memset(&p, 0, sizeof(p));
    p.damping             = param_damping.value();
    p.damping_form        = param_damping_form.value();
    p.max_iterations      = param_max_iterations.value();
    p.epsilon             = param_epsilon.value();
    p.closure_information = 1.0f;
    _ran_lm               = false;
    const int rc = prs_pose_graph_optimize(_ctx->get(), &p, (int32_t) _fixed.size(), _poses.data(), _fixed.data(), (int32_t) _from.size(),
                                           _from.data(), _to.data(), _z.data(), _omega.empty() ? nullptr : _omega.data(), &_result);
    if (rc < 0) throw std::runtime_error(std::string("SolverPoseGraphHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    warn("SolverPoseGraphHIP::compute", rc);
  }

  size_t size() const { return _fixed.size(); }
  const std::vector<double>& poses() const { return _poses; }
  const double* pose(size_t i) const { return _poses.data() + 16 * i; }
  // of the last compute(), whichever algorithm it ran
  int iterations() const { return _ran_lm ? _lm_result.iterations : _result.iterations; }
  double chi2() const { return _ran_lm ? _lm_result.chi_final : _result.chi_final; }
  const prs_pose_graph_result& result() const { return _result; }         // GaussNewton runs
  const prs_pose_graph_lm_result& resultLM() const { return _lm_result; }  // LevenbergMarquardt runs

protected:
  void computeLM() {
    prs_pose_graph_lm_params p;
    std::memset(&p, 0, sizeof(p));
    p.user_lambda_init  = param_user_lambda_init.value();
    p.tau               = param_tau.value();
    p.step_high         = param_step_high.value();
    p.step_low          = param_step_low.value();
    p.lm_iterations_max = param_lm_iterations_max.value();
    p.variable_damping  = param_variable_damping.value();
    p.max_iterations    = param_max_iterations.value();
    p.epsilon           = param_epsilon.value();
    _ran_lm             = true;
    const int rc = prs_pose_graph_optimize_lm(_ctx->get(), &p, (int32_t) _fixed.size(), _poses.data(), _fixed.data(), (int32_t) _from.size(),
                                              _from.data(), _to.data(), _z.data(), _omega.empty() ? nullptr : _omega.data(), &_lm_result);
    if (rc < 0) throw std::runtime_error(std::string("SolverPoseGraphHIP::compute|ERROR: ") + prs_last_error(_ctx->get()));
    warn("SolverPoseGraphHIP::compute", rc);
  }

  ContextPtr _ctx;
  bool _set = false;
  std::vector<double> _poses;
  std::vector<uint8_t> _fixed;
  std::vector<int32_t> _from, _to;
  std::vector<float> _z, _omega;
  prs_pose_graph_result _result = {};
  prs_pose_graph_lm_result _lm_result = {};
  bool _ran_lm = false;
};

#ifdef PROSLAM_HIP_WITH_HIP_RUNTIME
// ------------------------------------------------------------------------------------------------
// The local-map manager at B = 1: the block of SLAMBenchmark::benchmarkCompute between tracker->align() and tracker->merge()
// (apps/app_benchmark.cpp:100-183) over prs_session_step_batch.  The trajectory log (:107-121), the switch on the tracker's status
// (:123-178), LocalMapSplittingCriterionViewpoint3D's compute() / hasToSplit() and makeNewMap(1) / makeNewMap(0.1) are one call,
// step(); unrollFullTrajectory() (:195-203) is the other.  The session entries take device arrays only, so this adapter owns them
// (one allocation): the session's state, the aligner's three outputs, a local map's coords / desc / counters of `capacity` rows, the
// merger's per-frame inputs and one pose graph.  A caller whose merger runs on the device points it at batch()'s map arrays.
class LocalMapManagerHIP {
public:
  PropertyFloat param_local_map_distance{10.f};                // LocalMapSplittingCriterionViewpoint3D (kitti.conf:549)
  PropertyFloat param_local_map_angle_distance_radians{0.25f}; // (kitti.conf:546)
  PropertyFloat param_split_information{1.f};                  // makeNewMap(1)
  PropertyFloat param_lost_information{0.1f};                  // makeNewMap(0.1)

  LocalMapManagerHIP(ContextPtr ctx, int capacity, int node_stride, int edge_stride, int frame_stride) : _ctx(std::move(ctx)) {
    if (capacity < 1 || node_stride < 1 || edge_stride < 1 || frame_stride < 1) {
      throw std::runtime_error("LocalMapManagerHIP|ERROR: a size below 1");
    }
    std::memset(&_b, 0, sizeof(_b));
    _b.batch = 1, _b.frame_stride = frame_stride, _b.capacity = capacity, _b.node_stride = node_stride, _b.edge_stride = edge_stride;
    size_t end = 0;
    auto take = [&end](size_t bytes) {
      const size_t at = end;
      end += (bytes + 255) / 256 * 256;
      return at;
    };
    const size_t o_pose = take(64), o_prev = take(64), o_pred = take(64), o_slot = take(4), o_cur = take(4), o_nf = take(4),
                 o_fnode = take(4 * (size_t) frame_stride), o_fpose = take(64 * (size_t) frame_stride), o_status = take(4), o_reason = take(4),
                 o_X = take(64), o_res = take(sizeof(prs_align_result)), o_ncorr = take(4), o_coords = take(16 * (size_t) capacity),
                 o_desc = take(32 * (size_t) capacity), o_np = take(4), o_nm = take(4 * (size_t) capacity), o_frame = take(4),
                 o_ncm = take(4), o_miw = take(64), o_mis = take(64), o_gx = take(128 * (size_t) node_stride), o_fixed = take(node_stride),
                 o_nn = take(4), o_from = take(4 * (size_t) edge_stride), o_to = take(4 * (size_t) edge_stride),
                 o_Z = take(64 * (size_t) edge_stride), o_om = take(144 * (size_t) edge_stride), o_ne = take(4),
                 o_traj = take(64 * (size_t) frame_stride);
    _bytes = end;
    if (hipMalloc(&_block, _bytes) != hipSuccess) throw std::runtime_error("LocalMapManagerHIP|ERROR: device allocation failed");
    char* d = static_cast<char*>(_block);
    _b.pose = (float*) (d + o_pose), _b.prev = (float*) (d + o_prev), _b.prediction = (float*) (d + o_pred);
    _b.slot = (int32_t*) (d + o_slot), _b.cur_node = (int32_t*) (d + o_cur), _b.n_frames = (int32_t*) (d + o_nf);
    _b.frame_node = (int32_t*) (d + o_fnode), _b.frame_pose = (float*) (d + o_fpose);
    _b.status = (int32_t*) (d + o_status), _b.reason = (int32_t*) (d + o_reason);
    _b.X = (const float*) (d + o_X), _b.result = (const prs_align_result*) (d + o_res), _b.n_corr = (const int32_t*) (d + o_ncorr);
    _b.coords = (const float*) (d + o_coords), _b.desc = (const uint8_t*) (d + o_desc), _b.n_points = (int32_t*) (d + o_np);
    _b.n_meas = (uint32_t*) (d + o_nm), _b.frame = (int32_t*) (d + o_frame), _b.n_corr_merge = (int32_t*) (d + o_ncm);
    _b.measurement_in_world = (float*) (d + o_miw), _b.measurement_in_scene = (float*) (d + o_mis);
    _b.graph_X = (double*) (d + o_gx), _b.fixed = (uint8_t*) (d + o_fixed), _b.n_nodes = (int32_t*) (d + o_nn);
    _b.from = (int32_t*) (d + o_from), _b.to = (int32_t*) (d + o_to), _b.Z = (float*) (d + o_Z), _b.omega = (float*) (d + o_om);
    _b.n_edges = (int32_t*) (d + o_ne);
    _trajectory = (float*) (d + o_traj);
    reset();
  }
  ~LocalMapManagerHIP() {
    if (_block) (void) hipFree(_block);
  }
  LocalMapManagerHIP(const LocalMapManagerHIP&) = delete;
  LocalMapManagerHIP& operator=(const LocalMapManagerHIP&) = delete;

  // the first local map: the graph holds node 0 alone (identity, fixed); the next step() is frame 0
  void reset() {
    prs_context_synchronize(_ctx->get());
    check(hipMemset(_block, 0, _bytes), "reset");
    static const float eye[16]   = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    static const double eye_d[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    up(_b.pose, eye, 64), up(_b.prev, eye, 64), up(_b.prediction, eye, 64);
    up(_b.graph_X, eye_d, 128);
    const uint8_t one_u8 = 1;
    const int32_t one    = 1;
    up(_b.fixed, &one_u8, 1), up(_b.n_nodes, &one, 4);
  }

  // one frame: `X16` is the aligner's estimate (moving in fixed, relative to the prediction the local map was clipped at),
  // `status` TrackerBase-like (1 = the alignment succeeded), `warnings` the aligner's word (negative = error).  Logs the pose,
  // evaluates the criterion, makes the new map on a split or a loss.  Synchronises; returns the split made (PRS_SESSION_*).
  int step(const float* X16, int status, int warnings, int n_corr = 0) {
    prs_align_result r;
    std::memset(&r, 0, sizeof(r));
    r.status = status, r.warnings = warnings;
    const int32_t nc = n_corr;
    up(const_cast<float*>(_b.X), X16, 64), up(const_cast<prs_align_result*>(_b.result), &r, sizeof(r)), up(const_cast<int32_t*>(_b.n_corr), &nc, 4);
    prs_session_params p;
    std::memset(&p, 0, sizeof(p));
    p.local_map_distance               = param_local_map_distance.value();
    p.local_map_angle_distance_radians = param_local_map_angle_distance_radians.value();
    p.split_information                = param_split_information.value();
    p.lost_information                 = param_lost_information.value();
    const int rc = prs_session_step_batch(_ctx->get(), &p, &_b);
    if (rc < 0) throw std::runtime_error(std::string("LocalMapManagerHIP::step|ERROR: ") + prs_last_error(_ctx->get()));
    prs_context_synchronize(_ctx->get());
    _status = word(_b.status);
    _reason = word(_b.reason);
    if (_status == PRS_ERR_RANGE) throw std::runtime_error("LocalMapManagerHIP::step|ERROR: a counter is out of range");
    if (_status == PRS_ERR_CAPACITY) std::cerr << "LocalMapManagerHIP::step|WARNING: graph or log full, staying in the local map" << std::endl;
    return _reason;
  }

  bool hasToSplit() const { return _reason != PRS_SESSION_NO_SPLIT; }  // of the last step()
  int status() const { return _status; }
  int currentLocalMap() const { return word(_b.cur_node); }            // graph id of the current local map (node index)
  int numLocalMaps() const { return word(_b.n_nodes); }
  int numFrames() const { return word(_b.n_frames); }
  std::vector<float> robotInLocalMap() const { return down<float>(_b.pose, 16); }
  std::vector<float> prediction() const { return down<float>(_b.prediction, 16); }  // where the next frame's clip goes
  // the graph as it stands: estimates double [n][16], factors (from, to, measurement float [m][16], information float [m][36])
  std::vector<double> estimates() const { return down<double>(_b.graph_X, 16 * (size_t) numLocalMaps()); }
  void factors(std::vector<int32_t>& from, std::vector<int32_t>& to, std::vector<float>& measurements16, std::vector<float>& information36) const {
    const size_t m = (size_t) word(_b.n_edges);
    from = down<int32_t>(_b.from, m), to = down<int32_t>(_b.to, m);
    measurements16 = down<float>(_b.Z, 16 * m), information36 = down<float>(_b.omega, 36 * m);
  }
  // (local map of every frame, pose in it) as logged, float [n][16]
  void fullTrajectory(std::vector<int32_t>& local_map, std::vector<float>& poses16) const {
    const size_t n = (size_t) std::min(numFrames(), _b.frame_stride);
    local_map = down<int32_t>(_b.frame_node, n), poses16 = down<float>(_b.frame_pose, 16 * n);
  }
  // global poses float [n][16]: estimate of the frame's local map * the pose in it (unrollFullTrajectory)
  std::vector<float> unrollFullTrajectory() {
    const int rc = prs_session_unroll_batch(_ctx->get(), &_b, _trajectory);
    if (rc < 0) throw std::runtime_error(std::string("LocalMapManagerHIP::unrollFullTrajectory|ERROR: ") + prs_last_error(_ctx->get()));
    prs_context_synchronize(_ctx->get());
    return down<float>(_trajectory, 16 * (size_t) std::min(numFrames(), _b.frame_stride));
  }
  // the device arrays (a device-resident merger reads frame, n_corr_merge and the two poses, and owns coords .. n_meas)
  const prs_session_batch& batch() const { return _b; }

protected:
  static void check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("LocalMapManagerHIP::") + what + "|ERROR: " + hipGetErrorString(e));
  }
  template <class T>
  static void up(T* dst, const void* src, size_t bytes) {
    check(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "upload");
  }
  template <class T>
  static std::vector<T> down(const T* src, size_t count) {
    std::vector<T> out(count);
    if (count) check(hipMemcpy(out.data(), src, count * sizeof(T), hipMemcpyDeviceToHost), "download");
    return out;
  }
  static int word(const int32_t* src) { return down<int32_t>(src, 1)[0]; }

  ContextPtr _ctx;
  prs_session_batch _b;
  void* _block      = nullptr;
  size_t _bytes     = 0;
  float* _trajectory = nullptr;
  int _status = 0, _reason = 0;
};
#endif  // PROSLAM_HIP_WITH_HIP_RUNTIME

}  // namespace proslam_hip
