// ism3d.h — C++ host mirror of the reference's plugin interface for the recognition hot path.
//
// Same class names, parameter names, type strings and error behaviour as vseib/point-cloud-donkey
// (paths relative to /root/reference/src/implicit_shape_model):
//   JSONObject / JSONParameter / Factory<T>      utils/json_object.h:31-103, utils/factory.h:20-53
//   Exception hierarchy                          utils/exception.h:21-88
//   Features + SHOT/CSHOT/FPFH/SHORT_SHOT/SHORT_CSHOT/CoSPAIR/BSHOT/SpinImage/RSD/RIFT/CGF/ESF_LOCAL/USC   features/features.h:31-112, features_shot.cpp, features_cshot.cpp, features_fpfh.cpp, features_short_shot.cpp, features_short_cshot.cpp, features_cospair.cpp, features_bshot.cpp, features_spin_image.cpp, features_rsd.cpp, features_rift.cpp, features_cgf.cpp, features_esf_local.cpp, features_usc.cpp
//   Keypoints + VoxelGrid                        keypoints/keypoints.h:31-86, keypoints_voxel_grid.cpp:30-46
//   ActivationStrategy(KNN), Codebook            activation_strategy/*.h, codebook/codebook.h:50
//   FeatureRanking + KNNActivation/Incremental/Strangeness/NaiveBayes/Uniform   feature_ranking/feature_ranking.h, ranking_*.cpp, ranking_factory.h
//   Voting, VotingMeanShift, Vote, VotingMaximum voting/voting.h:35, voting_mean_shift.cpp, voting_maximum.h:25-88
//   ImplicitShapeModel                           implicit_shape_model.h:82-330
// What differs by design: PCL/Eigen/Boost types are replaced by plain SoA containers, every plugin works on a BATCH of
// objects, and the bodies call the C ABI of libismhip.so (include/ismhip.h) — there is no CPU implementation behind them.
#pragma once
#include <array>
#include <cstdint>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/ismhip.h"
#include "json.h"
#include "boost_archive.h"

namespace ism3d {

// ---- exceptions (utils/exception.h) ----------------------------------------------------------------
class Exception : public std::exception {
public:
    virtual ~Exception() throw() {}
    virtual const char* what() const throw() { return m_message.c_str(); }
protected:
    explicit Exception(std::string m) : m_message(std::move(m)) {}
private:
    std::string m_message;
};
class JSONException : public Exception { public: explicit JSONException(std::string m) : Exception(std::move(m)) {} };
class RuntimeException : public Exception { public: explicit RuntimeException(std::string m) : Exception(std::move(m)) {} };
class BadParamException : public Exception { public: explicit BadParamException(std::string m) : Exception(std::move(m)) {} };
template <typename T>
class BadParamExceptionType : public BadParamException {
public:
    BadParamExceptionType(std::string message, T value) : BadParamException(msg(message, value)) {}
private:
    static std::string msg(std::string m, T v) { std::stringstream s; s << v; if (!s.str().empty()) m += " (Value: " + s.str() + ")"; return m; }
};

// ---- JSON parameters (utils/json_parameter.h, json_parameter_traits.h) -----------------------------
struct JSONParameterBase {
    std::string name;
    virtual ~JSONParameterBase() {}
    virtual void fromJson(const Json* v) = 0;     // nullptr: key missing -> WARN + default (json_parameter_base.cpp:35-45)
    virtual Json toJson() const = 0;
};
template <typename T> struct JSONParameter;
class JSONObject {
public:
    JSONObject();
    virtual ~JSONObject();
    virtual std::string getType() const { return ""; }
    bool writeObject(std::string file);
    bool writeObject(std::string file, std::string fileData);
    bool readObject(std::string file, bool training = false);
    Json configToJson() const;
    bool configFromJson(const Json&);
protected:
    template <typename T> void addParameter(T& param, std::string name, T defaultValue);
    virtual Json iChildConfigsToJson() const { return Json::object(); }
    virtual bool iChildConfigsFromJson(const Json&) { return true; }
    virtual void iSaveData(std::ostream&) const {}
    virtual bool iLoadData(std::istream&) { return true; }
    virtual void iPostInitConfig() {}
    std::string m_output_file_name, m_input_config_file;
private:
    std::vector<JSONParameterBase*> m_params;
};

// typed parameter with the reference's semantics: missing key -> default (+ warning), wrong JSON type -> JSONException
void jsonWarnMissing(const std::string& name);
template <typename T> struct JSONParameterTraits;
template <> struct JSONParameterTraits<bool> {
    static bool ok(const Json& v) { return v.type == Json::Bool; }
    static bool get(const Json& v) { return v.b; }
    static Json put(bool v) { return Json::of(v); }
};
template <> struct JSONParameterTraits<int> {
    static bool ok(const Json& v) { return v.type == Json::Number; }
    static int get(const Json& v) { return (int)v.num; }
    static Json put(int v) { return Json::of(v); }
};
template <> struct JSONParameterTraits<float> {
    static bool ok(const Json& v) { return v.type == Json::Number; }
    static float get(const Json& v) { return (float)v.num; }
    static Json put(float v) { return Json::of((double)v); }
};
template <> struct JSONParameterTraits<double> {
    static bool ok(const Json& v) { return v.type == Json::Number; }
    static double get(const Json& v) { return v.num; }
    static Json put(double v) { return Json::of(v); }
};
template <> struct JSONParameterTraits<std::string> {
    static bool ok(const Json& v) { return v.type == Json::String; }
    static std::string get(const Json& v) { return v.str; }
    static Json put(const std::string& v) { return Json::of(v); }
};
typedef std::array<double, 3> Vec3d;      // Eigen::Vector3d parameters: a JSON array of three numbers (json_parameter_traits.h:107-128)
template <> struct JSONParameterTraits<Vec3d> {
    static bool ok(const Json& v) { return v.type == Json::Array && v.arr.size() == 3 && v.arr[0].type == Json::Number && v.arr[1].type == Json::Number && v.arr[2].type == Json::Number; }
    static Vec3d get(const Json& v) { return Vec3d{{v.arr[0].num, v.arr[1].num, v.arr[2].num}}; }
    static Json put(const Vec3d& v) { Json j = Json::array(); for (double x : v) j.arr.push_back(Json::of(x)); return j; }
};
template <typename T>
struct JSONParameter : JSONParameterBase {
    T& ref; T def;
    JSONParameter(T& r, std::string n, T d) : ref(r), def(d) { name = std::move(n); ref = d; }
    void fromJson(const Json* v) override {
        if (!v) { jsonWarnMissing(name); ref = def; return; }
        if (!JSONParameterTraits<T>::ok(*v)) throw JSONException("invalid type for parameter \"" + name + "\"");
        ref = JSONParameterTraits<T>::get(*v);
    }
    Json toJson() const override { return JSONParameterTraits<T>::put(ref); }
};
template <typename T>
void JSONObject::addParameter(T& param, std::string name, T defaultValue) { m_params.push_back(new JSONParameter<T>(param, std::move(name), defaultValue)); }

// ---- data model -------------------------------------------------------------------------------------
struct PointCloud {          // NaN-free surface with normals (PointXYZRGBNormal split into SoA)
    std::vector<float> x, y, z, nx, ny, nz;
    std::vector<uint32_t> rgba;         // 0x00RRGGBB, empty when the cloud has no colour
    bool organized = false;             // the file was a dense HEIGHT > 1 image: pcl::PointCloud::isOrganized() survives removeNaNFromPointCloud
    size_t size() const { return x.size(); }
    bool empty() const { return x.empty(); }
};
struct KeypointSet { std::vector<float> x, y, z; std::vector<uint32_t> rgba; size_t size() const { return x.size(); } };

struct BoundingBox { std::array<float, 3> position{{0, 0, 0}}; std::array<float, 4> rotQuat{{1, 0, 0, 0}}; std::array<float, 3> size{{0, 0, 0}}; };
struct Vote {                 // voting/voting_maximum.h:25-42
    std::array<float, 3> position; float weight; unsigned classId; unsigned instanceId; int codewordId;
};
struct VotingMaximum {        // voting/voting_maximum.h:51-88
    std::array<float, 3> position{{0, 0, 0}};
    float weight = 0;
    unsigned classId = (unsigned)-1;
    unsigned instanceId = (unsigned)-1;
    float instanceWeight = 0;
    BoundingBox boundingBox;
    int numVotes = 0;
    // the global classifier's answer for this maximum (voting_maximum.h:74-87); Voting.UseGlobalFeatures only
    struct GlobalHypothesis { unsigned classId = 0; float classWeight = 0; unsigned instanceId = 0; float instanceWeight = 0; };
    GlobalHypothesis globalHypothesis;
    // centroid of the region the hypothesis was computed on (detection mode; zeros in single-object mode). The reference keeps ONE
    // roi_centroid written by every maximum inside an OMP loop (voting.cpp:91, 226-229); here every maximum carries its own.
    std::array<float, 3> roiCentroid{{0, 0, 0}};
};

class DeviceSession;          // ctx + device buffers (ism3d.cpp)
struct DeviceFeatures;        // device-resident ISMFeature batch: descriptors, LRFs, keypoints, per-object offsets

// ---- global descriptors (the GlobalFeatures child; features/features_short_shot_global.cpp, features_shot_global.cpp, features_vfh.cpp,
// features_gasd.cpp)
// One row per REGION of the batch's search surface (ismhip_global_short_shot / ismhip_global_shot352 / ismhip_global_vfh /
// ismhip_global_gasd): the whole object in training and
// in single-object mode, a ball round a maximum in detection mode. Any other type of the reference stays a pass-through of its JSON
// (no object is created) and is refused by name only when Voting.UseGlobalFeatures asks for it.
struct GlobalRegions;          // device arrays of a region batch and its outputs (ism3d.cpp)
class GlobalFeatures : public JSONObject {
public:
    virtual ~GlobalFeatures() {}
    virtual int getDescriptorLength() const = 0;
    virtual void describe(DeviceSession& s, GlobalRegions& r) const = 0;     // fills r's outputs for r's regions on s.cloud
    virtual bool needsColor() const { return false; }                        // the batch is uploaded with its colours
    virtual void checkInput(const PointCloud&) const {}                      // refuses a cloud the descriptor cannot describe, on the host
    static const char* builtTypes() { return "SHORT_SHOT_GLOBAL, SHOT_GLOBAL, VFH, GASD, CVFH"; }
    static GlobalFeatures* createIfBuilt(const Json& object);                // nullptr for a type that is not built (or no object)
};
class GlobalFeaturesShortShot : public GlobalFeatures {      // features_short_shot_global.cpp:21-30, 168-249
public:
    GlobalFeaturesShortShot();
    static std::string getTypeStatic() { return "SHORT_SHOT_GLOBAL"; }
    std::string getType() const override { return getTypeStatic(); }
    int getDescriptorLength() const override { return m_r_bins * m_e_bins * m_a_bins; }
    void describe(DeviceSession& s, GlobalRegions& r) const override;
protected:
    void iPostInitConfig() override;                         // configureSphericalGrid
private:
    double m_min_radius; int m_feature_dims; bool m_log_radius; int m_r_bins, m_e_bins, m_a_bins; std::string m_bin_type;
};
class GlobalFeaturesShot : public GlobalFeatures {           // features_shot_global.cpp
public:
    static std::string getTypeStatic() { return "SHOT_GLOBAL"; }
    std::string getType() const override { return getTypeStatic(); }
    int getDescriptorLength() const override { return 352; }
    void describe(DeviceSession& s, GlobalRegions& r) const override;
};
class GlobalFeaturesVFH : public GlobalFeatures {            // features_vfh.cpp:27-70: no parameters, the viewpoint stays (0, 0, 0)
public:
    static std::string getTypeStatic() { return "VFH"; }
    std::string getType() const override { return getTypeStatic(); }
    int getDescriptorLength() const override { return ISMHIP_VFH_DIM; }
    void describe(DeviceSession& s, GlobalRegions& r) const override;    // there is no frame: r.lrf is filled with zeros
};
class GlobalFeaturesGASD : public GlobalFeatures {           // features_gasd.cpp:16-91: pcl::GASDColorEstimation, view direction (0, 0, 1)
public:
    GlobalFeaturesGASD();
    static std::string getTypeStatic() { return "GASD"; }
    std::string getType() const override { return getTypeStatic(); }
    int getDescriptorLength() const override { return m_use_color ? ISMHIP_GASD_DIM : ISMHIP_GASD_SHAPE_DIM; }
    bool needsColor() const override { return m_use_color; }
    void checkInput(const PointCloud& cloud) const override;             // GasdWithColor: a cloud without colours throws
    void describe(DeviceSession& s, GlobalRegions& r) const override;    // the stored rf of a row is zeros, as for VFH
private:
    bool m_use_color;
};
// features_cvfh.cpp: pcl::CVFHEstimation, angle 10 degrees, viewpoint (0, 0, 0). The one type with SEVERAL rows per region, one per smooth
// cluster (GlobalRegions::row_off). The reference has no parameters; the three here default to PCL's metre-scale values and are this
// port's own (a reference configuration behaves as the reference does).
class GlobalFeaturesCVFH : public GlobalFeatures {
public:
    GlobalFeaturesCVFH();
    static std::string getTypeStatic() { return "CVFH"; }
    std::string getType() const override { return getTypeStatic(); }
    int getDescriptorLength() const override { return ISMHIP_VFH_DIM; }
    void describe(DeviceSession& s, GlobalRegions& r) const override;    // compacts the rows: r.desc [r.row_off.back()][308]; rf zeros
private:
    double m_cluster_tolerance, m_normal_radius; int m_min_points;
};
// one stored training row (ISMFeature of voting.cpp:586-613, 660-701)
struct StoredGlobalFeature { unsigned classId = 0, instanceId = 0; float rf[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; std::vector<float> descriptor; float radius = 0; };

// ---- Keypoints (keypoints/keypoints.h) -----------------------------------------------------------------
class Keypoints : public JSONObject {
public:
    virtual ~Keypoints() {}
    KeypointSet operator()(const PointCloud& points) const { return iComputeKeypoints(points); }
protected:
    virtual KeypointSet iComputeKeypoints(const PointCloud& points) const = 0;
};
class KeypointsVoxelGrid : public Keypoints {
public:
    KeypointsVoxelGrid();
    static std::string getTypeStatic() { return "VoxelGrid"; }
    std::string getType() const override { return getTypeStatic(); }
    float getLeafSize() const { return m_leafSize; }
protected:
    KeypointSet iComputeKeypoints(const PointCloud& points) const override;
private:
    float m_leafSize;
};
// keypoints/keypoints_iss3d.cpp:17-72 -> pcl::ISSKeypoint3D without border estimation (ismhip_iss3d_keypoints):
// the reference's parameter names and defaults. Non-positive radii or gammas and a negative MinNeighbors are refused when the
// configuration is read. There is NO host implementation: the detector runs on the batch's search surface on the device
// (ImplicitShapeModel::computeFeatures), iComputeKeypoints(const PointCloud&) throws by name, and ISM3D_HOST_KEYPOINTS=1 -- the switch
// that sends VoxelGrid to its host implementation -- does not apply to ISS3D. Organised clouds are treated as unorganised ones (the
// reference hands PCL the unfiltered cloud there); computeFeatures warns.
class KeypointsISS3D : public Keypoints {
public:
    KeypointsISS3D();
    static std::string getTypeStatic() { return "ISS3D"; }
    std::string getType() const override { return getTypeStatic(); }
    double getSalientRadius() const { return m_salientRadius; }
    double getNonMaxRadius() const { return m_nonMaxRadius; }
    double getGamma21() const { return m_gamma21; }
    double getGamma32() const { return m_gamma32; }
    int getMinNeighbors() const { return m_minNeighbors; }
protected:
    KeypointSet iComputeKeypoints(const PointCloud& points) const override;
    void iPostInitConfig() override;
private:
    double m_salientRadius, m_nonMaxRadius, m_gamma21, m_gamma32;
    int m_minNeighbors;
};

// keypoints/keypoints_sift3d.cpp:17-86 -> pcl::SIFTKeypoint on the cloud's normal curvature, setScales(Radius, 4, 3), minimum contrast 0
// (ismhip_normal_curvature, ismhip_sift3d_keypoints): the reference's one parameter and its default. A Radius that
// is not > 0, or not a number, is refused when the configuration is read. There is NO host implementation: the detector runs on the
// batch's search surface on the device (DeviceSession::finishBatch), iComputeKeypoints(const PointCloud&) throws by name, and
// ISM3D_HOST_KEYPOINTS=1 does not apply. The curvature is always computed there, at the model's NormalRadius, on the NaN-free surface the
// descriptors will see; organised clouds take the same route. The keypoints carry no colour.
class KeypointsSIFT3D : public Keypoints {
public:
    KeypointsSIFT3D();
    static std::string getTypeStatic() { return "SIFT3D"; }
    std::string getType() const override { return getTypeStatic(); }
    float getRadius() const { return m_radius; }
    static constexpr int kOctaves = 4, kScalesPerOctave = 3;     // setScales(m_radius, 4, 3), keypoints_sift3d.cpp:60
protected:
    KeypointSet iComputeKeypoints(const PointCloud& points) const override;
    void iPostInitConfig() override;
private:
    float m_radius;
};

// keypoints/keypoints_voxel_grid_culling.cpp:27-44: the reference's 13 parameter names and defaults (ismhip_principal_curvatures,
// ismhip_culling_scores, ismhip_culling_select). Method and type strings are lower-cased when the configuration is
// read, as the reference lower-cases them before it compares; CombineFilters is case-sensitive. Refused by name there, each with its
// reason: FilterMethodGeometry "gaussian", FilterTypeGeometry "auto", RefineKeypointPosition, a FilterCutoffRatio outside [0, 1), an
// unknown method, type or CombineFilters, a non-positive LeafSize. There is NO host implementation of the culling: the detector runs on
// the batch's search surface on the device (DeviceSession::finishBatch), iComputeKeypoints(const PointCloud&) throws by name, and
// ISM3D_HOST_KEYPOINTS=1 does not apply.
class KeypointsVoxelGridCulling : public Keypoints {
public:
    KeypointsVoxelGridCulling();
    static std::string getTypeStatic() { return "VoxelGridCulling"; }
    std::string getType() const override { return getTypeStatic(); }
    float getLeafSize() const { return m_leafSize; }
    // both methods "none", or training with DisableFilterInTraining: the plain voxel grid (:76-87)
    bool isPlainVoxelGrid(bool is_training) const { return (is_training && m_disable_filter_in_training) || (m_geometry == 0 && m_color == 0); }
    bool needsColor() const { return m_color != 0; }
    int geometryMethod() const { return m_geometry; }      // ISMHIP_CULLING_GEOMETRY_*
    int colorMethod() const { return m_color; }            // ISMHIP_CULLING_COLOR_*
    int geometryType() const { return m_geometry_type; }   // ISMHIP_CULLING_TYPE_*
    int colorType() const { return m_color_type; }
    int combine() const { return m_combine; }              // ISMHIP_CULLING_REQUIRE_*
    float geometryThreshold() const { return m_filter_threshold_geometry; }
    float colorThreshold() const { return m_filter_threshold_color; }
    float maxSimilarColorDistance() const { return m_max_similar_color_distance; }
    float cutoffRatio() const { return m_filter_cutoff_ratio; }
protected:
    KeypointSet iComputeKeypoints(const PointCloud& points) const override;
    void iPostInitConfig() override;
private:
    float m_leafSize;
    std::string m_filter_method_geometry, m_filter_type_geometry, m_filter_method_color, m_filter_type_color, m_combine_filters;
    float m_filter_threshold_geometry, m_filter_threshold_color, m_max_similar_color_distance, m_filter_cutoff_ratio;
    bool m_disable_filter_in_training, m_refine_position;
    int m_geometry = 0, m_color = 0, m_geometry_type = 0, m_color_type = 0, m_combine = 2;
};

// ---- Features (features/features.h) -------------------------------------------------------------------
class Features : public JSONObject {
public:
    Features();
    virtual ~Features() {}
    // Features::operator() (features.cpp:40-116): LRFs -> drop invalid frames -> iComputeDescriptors -> NaN rows removed.
    // Works on the batch resident in the session; returns the device feature batch.
    std::shared_ptr<DeviceFeatures> operator()(DeviceSession& s) const;
    void setNumThreads(int n) { m_numThreads = n; }
    int getNumThreads() const { return m_numThreads; }
    float getReferenceFrameRadius() const { return m_referenceFrameRadius; }
    virtual float getRadius() const = 0;
    virtual int getDescriptorLength() const = 0;
    virtual bool needsColor() const { return false; }
    // refuses an input cloud the descriptor cannot describe, on the host, before any device work (default: every cloud is taken)
    virtual void checkInput(const PointCloud&) const {}
protected:
    void iPostInitConfig() override { checkReferenceFrameType(); }   // what the device does not compute is refused when the config is read
    // ReferenceFrameType (features.cpp:153-179): "SHOT" and "SHOTNA" are built, "BOARD" and "FLARE" refused, anything else a bad parameter
    void checkReferenceFrameType() const;
    // writes descriptors [nkp x D] for every keypoint of the batch (NaN rows for failures, never an error)
    virtual void iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const = 0;
    float m_referenceFrameRadius;
    std::string m_referenceFrameType;
    int m_numThreads;
};
#define ISM3D_FEATURE(NAME, TYPESTR, DIM, COLOR)                                                      \
    class NAME : public Features {                                                                    \
    public:                                                                                           \
        NAME();                                                                                       \
        static std::string getTypeStatic() { return TYPESTR; }                                        \
        std::string getType() const override { return getTypeStatic(); }                              \
        float getRadius() const override { return m_radius; }                                         \
        int getDescriptorLength() const override { return DIM; }                                      \
        bool needsColor() const override { return COLOR; }                                            \
    protected:                                                                                        \
        void iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const override; \
    private:                                                                                          \
        float m_radius;                                                                               \
    };
ISM3D_FEATURE(FeaturesSHOT, "SHOT", 352, false)
ISM3D_FEATURE(FeaturesCSHOT, "CSHOT", 1344, true)
ISM3D_FEATURE(FeaturesFPFH, "FPFH", 33, false)
// features/features_bshot.{h,cpp}: SHOT-352 binarised in groups of four (getBinaryVector :109-157); rows of zeros and ones. The frames and
// centerDist are FeaturesSHOT's. A NaN SHOT row becomes 352 ones and stays in the batch, as in the reference.
ISM3D_FEATURE(FeaturesBSHOT, "BSHOT", ISMHIP_BSHOT_DIM, false)
// features/features_spin_image.{h,cpp}: PCL's spin image (width 8, rectangular, support-angle cosine 0) about the normal of the cloud point
// the keypoint coincides with, 153 floats; a keypoint that is no cloud point gets the zero axis, as in the reference (DESIGN.md section
// 4.15), so the type wants keypoints taken from the cloud (ISS3D). The frames only decide which keypoints stay; centerDist is not set.
ISM3D_FEATURE(FeaturesSpinImage, "SpinImage", ISMHIP_SPIN_IMAGE_DIM, false)
// features/features_usc.{h,cpp} -> pcl::UniqueShapeContext (ismhip_point_density, ismhip_usc): 14 x 14 x 10 bins of
// the Radius ball in PCL's own frame, every point weighted by the bin's volume and the point's density, 1960 floats, not normalised.
// Radius is the one parameter; the minimal radius is Radius / 10 and the frames of the rows are SHOT frames at Radius - 0.1 (0.1 when
// Radius <= 0.1), computed apart from ReferenceFrameType / ReferenceFrameRadius (features_usc.cpp:46-54); the frames kept with the
// features for voting stay the base class's. Rows of this length are searched by ismhip_knn's exact wide scan only: the Threshold
// activation, KNN with K > 16 and a FeatureWeighting other than Uniform are refused when the configuration is read.
ISM3D_FEATURE(FeaturesUSC, "USC", ISMHIP_USC_DIM, false)
// The one value features_usc.cpp leaves to pcl::UniqueShapeContext's constructor: the radius of the point density. 0.1 AS RECALLED from
// PCL 1.10's usc.h (PCL is not part of the reference tree, so the value is unpinned); change it here and in capi.py if PCL says otherwise.
constexpr float USC_POINT_DENSITY_RADIUS = 0.1f;
// features/features_short_shot.{h,cpp}: the generalised Short SHOT. Not an ISM3D_FEATURE: its length follows the spherical grid.
class FeaturesSHORTSHOT : public Features {
public:
    FeaturesSHORTSHOT();
    static std::string getTypeStatic() { return "SHORT_SHOT"; }
    std::string getType() const override { return getTypeStatic(); }
    float getRadius() const override { return m_radius; }
    int getDescriptorLength() const override { return m_feature_dims; }
    float getMinRadius() const;                      // compute_descriptor :88-103, as the float ismhip_short_shot takes
protected:
    void iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const override;
    void iPostInitConfig() override;                 // configureSphericalGrid (:285-366) + what the device refuses
    float m_radius;
    bool m_use_min_radius, m_log_radius;
    double m_min_radius_relative;
    int m_feature_dims, m_r_bins, m_e_bins, m_a_bins;
    std::string m_bin_type;
};
// features/features_short_cshot.{h,cpp}: the Short SHOT followed by a colour histogram on a second spherical grid. The nine shape
// parameters, configureSphericalGrid and the minimum radius are FeaturesSHORTSHOT's (the reference repeats their text, :23-33, :114-132,
// :509-590); ShortColorShotDims and ShortColorShotHistSize are added.
class FeaturesSHORTCSHOT : public FeaturesSHORTSHOT {
public:
    FeaturesSHORTCSHOT();
    static std::string getTypeStatic() { return "SHORT_CSHOT"; }
    std::string getType() const override { return getTypeStatic(); }
    int getDescriptorLength() const override { return m_feature_dims + m_color_feature_dims * m_color_hist_size; }
    bool needsColor() const override { return true; }
    void checkInput(const PointCloud& cloud) const override;   // a cloud without colours throws
protected:
    void iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const override;
    void iPostInitConfig() override;                 // + configureSphericalColorGrid (:592-646) + what the device refuses
private:
    int m_color_feature_dims, m_color_hist_size, m_r_color_bins, m_e_color_bins, m_a_color_bins;
};
// features/features_cospair.{h,cpp} -> third_party/cospair: seven shells around the cloud point nearest to the keypoint, pair features
// and CIELab colours, 378 floats. Levels, bins and colour type are hard-coded in the reference (:37-40); Radius is the one parameter.
// Not an ISM3D_FEATURE: it checks its input cloud.
class FeaturesCospair : public Features {
public:
    FeaturesCospair();
    static std::string getTypeStatic() { return "CoSPAIR"; }
    std::string getType() const override { return getTypeStatic(); }
    float getRadius() const override { return m_radius; }
    int getDescriptorLength() const override { return ISMHIP_COSPAIR_DIM; }
    bool needsColor() const override { return true; }
    void checkInput(const PointCloud& cloud) const override;   // a cloud without colours throws
protected:
    void iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const override;
private:
    float m_radius;
};
// features/features_rsd.{h,cpp} -> PCL's RSDEstimation over every pair of the ball's points (ismhip_rsd): the
// 5 x 5 angle-distance histogram over 300 (25 floats) or, with UseFullRSDHistogram false, the two principal radii (2 floats). The frames
// only decide which keypoints stay. Not an ISM3D_FEATURE: its length follows the switch.
class FeaturesRSD : public Features {
public:
    FeaturesRSD();
    static std::string getTypeStatic() { return "RSD"; }
    std::string getType() const override { return getTypeStatic(); }
    float getRadius() const override { return m_radius; }
    int getDescriptorLength() const override { return m_use_hist ? ISMHIP_RSD_DIM : ISMHIP_RSD_RADII_DIM; }
    bool useFullHistogram() const { return m_use_hist; }
protected:
    void iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const override;
private:
    float m_radius;
    bool m_use_hist;
};
// features/features_rift.{h,cpp} -> PCL's IntensityGradientEstimation and RIFTEstimation (ismhip_intensity_gradients, ismhip_rift, DESIGN.md
// section 4.19): the intensity gradients of the coloured cloud, then per keypoint the 8 x 16 histogram of (distance, gradient angle), 128
// floats. The bin counts are hard-coded in the reference (:38-39); Radius is the one parameter. The frames only decide which keypoints
// stay. Not an ISM3D_FEATURE: it checks its input cloud.
class FeaturesRIFT : public Features {
public:
    FeaturesRIFT();
    static std::string getTypeStatic() { return "RIFT"; }
    std::string getType() const override { return getTypeStatic(); }
    float getRadius() const override { return m_radius; }
    int getDescriptorLength() const override { return ISMHIP_RIFT_DIM; }
    bool needsColor() const override { return true; }
    void checkInput(const PointCloud& cloud) const override;   // a cloud without colours throws
protected:
    void iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const override;
private:
    float m_radius;
};
// features/features_esf_local.{h,cpp} -> PCL's ESFEstimation on the Radius ball of every keypoint (ismhip_esf_local, DESIGN.md section
// 4.21): twenty thousand point triples, their lines traced through a 64^3 occupancy grid of the ball, 640 floats. Radius is the one
// parameter; no normals, no colour and no frame enter the row. The frames only decide which keypoints stay.
class FeaturesESFLocal : public Features {
public:
    FeaturesESFLocal();
    static std::string getTypeStatic() { return "ESF_LOCAL"; }
    std::string getType() const override { return getTypeStatic(); }
    float getRadius() const override { return m_radius; }
    int getDescriptorLength() const override { return ISMHIP_ESF_DIM; }
protected:
    void iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const override;
private:
    float m_radius;
};

// features/features_cgf.{h,cpp} -> third_party/cgf/cgf.cpp and embedding.py (ismhip_keypoint_normals_pca, ismhip_cgf_raw, ismhip_mlp_forward,
// DESIGN.md section 4.20): the 2244-bin spherical histogram of the Radius ball in CGF's own frame (SHOT at 0.75 Radius, negated against a PCA
// normal at 0.1 Radius), embedded by the perceptron of CgfModelFile. Radius is the reference's one parameter; CgfModelFile is this library's
// (the reference hard-codes "embed_model_910000.ckpt" in the working directory and leaves the process to run it): a .cgfw container
// (include/ismhip.h, tools/cgf_weights.py), read when the configuration is read -- the descriptor's length is the file's. The frames of
// ReferenceFrameRadius / ReferenceFrameType only decide which keypoints stay, as for every Features type. Not an ISM3D_FEATURE: its length
// follows the file.
class FeaturesCGF : public Features {
public:
    FeaturesCGF();
    ~FeaturesCGF() override;
    static std::string getTypeStatic() { return "CGF"; }
    std::string getType() const override { return getTypeStatic(); }
    float getRadius() const override { return m_radius; }
    int getDescriptorLength() const override { return m_dim; }
protected:
    void iPostInitConfig() override;                 // + the weights file: every refusal of the loader, and the length
    void iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const override;
private:
    float m_radius;
    std::string m_model_file;
    int m_dim = 0;
    ismhip_cgfw* m_weights = nullptr;
};

// ---- activation strategy + codebook ----------------------------------------------------------------------
class ActivationStrategy : public JSONObject {
public:
    ActivationStrategy();
    virtual ~ActivationStrategy() {}
    void setIsDetection() { m_is_detection = true; }
    bool useDistanceRatio() const { return m_use_distance_ratio; }
    float distanceRatioThreshold() const { return m_distance_ratio_threshold; }
    virtual int getK() const = 0;
    // activates every feature of the batch; writes idx/dist [n x columns] on the device and returns the column count
    virtual int activateKNN(DeviceSession& s, const ismhip_codebook* codewords, const DeviceFeatures& f, int metric, int32_t* idx_out, float* dist_out, const float* desc = nullptr) const = 0;
protected:
    bool m_use_distance_ratio; float m_distance_ratio_threshold; bool m_is_detection = false;
};
class ActivationStrategyKNN : public ActivationStrategy {
public:
    ActivationStrategyKNN();
    static std::string getTypeStatic() { return "KNN"; }
    std::string getType() const override { return getTypeStatic(); }
    int getK() const override { return m_k; }
    // activateKNN for a whole feature batch (activation_strategy_knn.h:41-126): idx/dist [n x K] on the device, exact search
    // (FLANNExactMatch semantics). With UseDistanceRatio at detection time and K == 1 the 2-NN ratio test discards matches
    // (idx -1). Returns K.
    int activateKNN(DeviceSession& s, const ismhip_codebook* codewords, const DeviceFeatures& f, int metric, int32_t* idx_out, float* dist_out, const float* desc = nullptr) const override;
private:
    int m_k;
};
class ActivationStrategyKnnRule : public ActivationStrategy {      // activation_strategy/activation_strategy_knn_rule.h:41-152
public:
    ActivationStrategyKnnRule();
    static std::string getTypeStatic() { return "KNNRule"; }
    std::string getType() const override { return getTypeStatic(); }
    int getK() const override { return m_k; }
    // training: plain 1-NN; detection: 3-NN + class-consistency rules. One column.
    int activateKNN(DeviceSession& s, const ismhip_codebook* codewords, const DeviceFeatures& f, int metric, int32_t* idx_out, float* dist_out, const float* desc = nullptr) const override;
private:
    int m_k;
};

// activation_strategy/activation_strategy_threshold.cpp:18-44: every codeword whose functor value is STRICTLY below Threshold, in
// codebook row order -- any number per feature, zero included. Codebook::activate / castVotes take the list path for it
// (ismhip_knn_threshold -> ismhip_train_activate_lists / ismhip_cast_votes_csr); UseDistanceRatio is inherited and never read.
class ActivationStrategyThreshold : public ActivationStrategy {
public:
    ActivationStrategyThreshold();
    static std::string getTypeStatic() { return "Threshold"; }
    std::string getType() const override { return getTypeStatic(); }
    int getK() const override { return 1; }             // no fixed fan-out (the K cap checks do not apply)
    float getThreshold() const { return m_threshold; }
    // the fixed-column interface does not fit a variable fan-out: throws (the codebook calls the list path instead)
    int activateKNN(DeviceSession& s, const ismhip_codebook* codewords, const DeviceFeatures& f, int metric, int32_t* idx_out, float* dist_out, const float* desc = nullptr) const override;
private:
    float m_threshold;
};

// ---- Clustering (clustering/clustering.h:31-99) ----------------------------------------------------------------------------
// operator() clusters the descriptors of all training features; getClusterCenters / getClusterIndices as in the reference, with
// the centres left on the device (they are the rows of the activation codebook). "None": one cluster per feature, no centre matrix.
struct ClusterCenters;         // device matrix [n x dim] (ism3d.cpp)
class Clustering : public JSONObject {
public:
    Clustering();
    virtual ~Clustering();
    void operator()(DeviceSession& s, const DeviceFeatures& f, int metric) { clear(); process(s, f, metric); }
    virtual void clear();
    bool hasCenters() const { return m_n_centers > 0; }
    int getNumCenters() const { return m_n_centers; }
    const float* getClusterCentersDevice() const;
    const std::vector<int>& getClusterIndices() const { return m_indices; }
protected:
    virtual void process(DeviceSession& s, const DeviceFeatures& f, int metric) = 0;
    std::unique_ptr<ClusterCenters> m_centers;
    int m_n_centers = 0;
    std::vector<int> m_indices;
    std::vector<float> m_distances;            // functor distance of every feature to its centre
};
class ClusteringNone : public Clustering {        // clustering_none.cpp:25-35: every feature is its own centre
public:
    static std::string getTypeStatic() { return "None"; }
    std::string getType() const override { return getTypeStatic(); }
protected:
    void process(DeviceSession& s, const DeviceFeatures& f, int metric) override;
};
class ClusteringKMeans : public Clustering {      // clustering_kmeans.{h,cpp}: Iterations, CentersInit, CbIndex (+ Seed: this build's draws)
protected:
    ClusteringKMeans();
    void cluster(DeviceSession& s, const DeviceFeatures& f, int metric, int clusterCount);
    int m_iterations; std::string m_centersInit; float m_cbIndex; int m_seed;
};
class ClusteringKMeansCount : public ClusteringKMeans {         // clustering_kmeans_count.cpp
public:
    ClusteringKMeansCount();
    static std::string getTypeStatic() { return "KMeansCount"; }
    std::string getType() const override { return getTypeStatic(); }
protected:
    void process(DeviceSession& s, const DeviceFeatures& f, int metric) override;
    int m_clusterCount;
};
class ClusteringKMeansFactor : public ClusteringKMeans {        // clustering_kmeans_factor.cpp
public:
    ClusteringKMeansFactor();
    static std::string getTypeStatic() { return "KMeansFactor"; }
    std::string getType() const override { return getTypeStatic(); }
protected:
    void process(DeviceSession& s, const DeviceFeatures& f, int metric) override;
    float m_clusterFactor;
};
class ClusteringKMeansThumbRule : public ClusteringKMeans {     // clustering_kmeans_thumb_rule.cpp
public:
    static std::string getTypeStatic() { return "KMeansThumbRule"; }
    std::string getType() const override { return getTypeStatic(); }
protected:
    void process(DeviceSession& s, const DeviceFeatures& f, int metric) override;
};
class ClusteringKMeansHartigan : public ClusteringKMeans {      // clustering_kmeans_hartigan.cpp
public:
    ClusteringKMeansHartigan();
    static std::string getTypeStatic() { return "KMeansHartigan"; }
    std::string getType() const override { return getTypeStatic(); }
protected:
    void process(DeviceSession& s, const DeviceFeatures& f, int metric) override;
    int m_maxK;
};

// ---- FeatureRanking (feature_ranking/feature_ranking.h, ranking_factory.h) --------------------------------------------------
// operator() is the reference's (feature_ranking.cpp:37-118) on a class-major feature batch: scores (ismhip_rank_scores), then the
// per-class window of the ranked list (ismhip_rank_select); it returns the keep mask, 1 = the feature stays. All searches are exact
// and chi-square, whatever DistanceType says (feature_ranking.cpp:35). "Similarity" is not built.
class FeatureRanking : public JSONObject {
public:
    FeatureRanking();
    virtual ~FeatureRanking() {}
    // class_offsets: [n_classes + 1] ranges of the classes in f (ascending class ids, empty classes allowed)
    std::vector<uint8_t> operator()(DeviceSession& s, const DeviceFeatures& f, const std::vector<uint32_t>& class_offsets);
    virtual bool ranks() const { return true; }        // false: Uniform, every feature stays and nothing is launched
    float getExtractOffset() const { return m_extract_offset; }
protected:
    void iPostInitConfig() override;                   // the deprecated ExtractFromList -> ExtractOffset (:135-148)
    virtual int deviceType() const = 0;                // ISMHIP_RANK_*
    virtual int incrementType() { return 0; }
    int m_k_search; float m_dist_thresh, m_factor; std::string m_extract_list; float m_extract_offset;
};
class RankingUniform : public FeatureRanking {         // ranking_uniform.cpp
public:
    static std::string getTypeStatic() { return "Uniform"; }
    std::string getType() const override { return getTypeStatic(); }
    bool ranks() const override { return false; }
protected:
    int deviceType() const override { return -1; }
};
class RankingKnnActivation : public FeatureRanking {   // ranking_knn_activation.cpp
public:
    RankingKnnActivation();
    static std::string getTypeStatic() { return "KNNActivation"; }
    std::string getType() const override { return getTypeStatic(); }
protected:
    void iPostInitConfig() override;                   // + UseFeaturePosition true is refused (the training batch carries no centerDist)
    int deviceType() const override { return ISMHIP_RANK_KNN_ACTIVATION; }
    int incrementType() override;                      // :88-95: 0 means 1, anything outside 1 .. 3 becomes 1 with a warning
    bool m_use_feature_position; int m_score_increment_type;
};
#define ISM3D_RANKING(NAME, TYPESTR, DEVTYPE)                                                        \
    class NAME : public FeatureRanking {                                                             \
    public:                                                                                          \
        static std::string getTypeStatic() { return TYPESTR; }                                       \
        std::string getType() const override { return getTypeStatic(); }                             \
    protected:                                                                                       \
        int deviceType() const override { return DEVTYPE; }                                          \
    };
ISM3D_RANKING(RankingIncremental, "Incremental", ISMHIP_RANK_INCREMENTAL)      // ranking_incremental.cpp
ISM3D_RANKING(RankingStrangeness, "Strangeness", ISMHIP_RANK_STRANGENESS)      // ranking_strangeness.cpp
ISM3D_RANKING(RankingNaiveBayes, "NaiveBayes", ISMHIP_RANK_NAIVE_BAYES)        // ranking_naive_bayes.cpp
#undef ISM3D_RANKING

struct CodebookData {          // host copy of what Codebook::iSaveData persists (flattened CodewordDistributions)
    int dim = 0;
    std::vector<float> words, word_weight;
    std::vector<uint32_t> vote_offsets{0};
    std::vector<float> vote_xyz, vote_weight, vote_class_weight, vote_bbox_quat, vote_bbox_size;
    std::vector<uint32_t> vote_class, vote_instance;
    std::vector<uint32_t> word_class;      // Codeword::getClassId per word (empty: class of the word's first vote)
    std::vector<int32_t> word_id;          // Codeword::getId per word, ascending (empty: the row index)
    std::vector<int32_t> word_num_features;// Codeword::getNumFeatures (empty: 1)
    std::vector<float> word_keypoint;      // [n_words*3] Codeword::getKeypoint (empty: 0)
    std::vector<float> class_sigma;
    int numWords() const { return dim ? (int)(words.size() / dim) : 0; }
    // consistency of the arrays with each other (a data file is untrusted input); empty string = fine
    std::string validate() const;
};

class Voting;
class Codebook : public JSONObject {
public:
    Codebook();
    ~Codebook();
    std::string getType() const override { return "Codebook"; }
    // training: Codebook::activate (codebook.cpp:64-368); the codewords are the clustering's centres (one per feature for "None")
    void activate(DeviceSession& s, const DeviceFeatures& f, const std::vector<unsigned>& feat_class, const std::vector<unsigned>& feat_instance,
                  const std::vector<unsigned>& feat_model, const std::vector<std::array<float, 3>>& feat_center,
                  const std::vector<std::array<float, 3>>& feat_bbox_size, int metric, int n_classes, const Clustering& clustering,
                  const std::vector<std::array<float, 4>>* feat_bbox_quat = nullptr);   // nullptr: axis-aligned boxes, (1, 0, 0, 0)
    // detection: Codebook::castVotes (codebook.cpp:403-555): activate every feature, emit the votes into the voting space
    void castVotes(DeviceSession& s, const DeviceFeatures& f, int metric, Voting& voting) const;
    bool isEmpty() const { return m_data.numWords() == 0; }
    int getSize() const { return m_data.numWords(); }
    int getDim() const { return m_data.dim; }
    const CodebookData& data() const { return m_data; }
    void setData(const CodebookData& d) { m_data = d; m_dirty = true; }
    // the codewords are rows of zeros and ones (Features type "BSHOT"): upload() then asks for the binary image of the exact integer search
    void setBinaryWords(bool b) { if (b != m_binary_words) { m_binary_words = b; m_dirty = true; } }
    const ActivationStrategy* getActivationStrategy() const { return m_activationStrategy.get(); }
    void save(BoostBinaryOArchive& oa) const;     // Codebook::iSaveData (codebook.cpp:739-761)
    bool load(BoostBinaryIArchive& ia);           // Codebook::iLoadData (codebook.cpp:763-950)
protected:
    Json iChildConfigsToJson() const override;
    bool iChildConfigsFromJson(const Json&) override;
private:
    void upload(DeviceSession& s) const;
    bool m_useClassWeight, m_useVoteWeight, m_useMatchingWeight, m_useCodewordWeight;
    bool m_use_partial_shot; std::string m_partial_shot_type;
    bool m_use_random_codebook; float m_random_codebook_factor;
    std::unique_ptr<ActivationStrategy> m_activationStrategy;
    CodebookData m_data;
    mutable std::vector<int32_t> m_partial_cols;    // kept descriptor columns when UsePartialShot (empty otherwise)
    mutable bool m_dirty = true;
    bool m_binary_words = false;
    mutable ismhip_codebook* m_dev = nullptr;
    mutable DeviceSession* m_dev_session = nullptr;
};

// ---- Voting (voting/voting.h) ----------------------------------------------------------------------------
class Voting : public JSONObject {
public:
    Voting();
    virtual ~Voting() {}
    // Voting::findMaxima for every object of the batch (voting.cpp:79-328). metric is read with UseGlobalFeatures only (the box of a
    // hypothesis-only maximum comes from the session's search surface).
    std::vector<std::vector<VotingMaximum>> findMaxima(DeviceSession& s, int metric = ISMHIP_METRIC_L2SQ);
    // ---- global verification (voting.cpp:217-298; classifier/global_classifier.cpp) ----
    bool useGlobalFeatures() const { return m_use_global_features; }
    const std::string& globalStrategy() const { return m_global_feature_method; }
    void setGlobalFeatureDescriptor(const GlobalFeatures* g) { m_global_descriptor = g; }
    // Voting::forwardGlobalFeatures (voting.cpp:554-557): class -> one list per training cloud (empty when its row was NaN)
    typedef std::map<unsigned, std::vector<std::vector<StoredGlobalFeature>>> GlobalFeatureMap;
    void forwardGlobalFeatures(const GlobalFeatureMap& g) { m_global_features = g; }
    const GlobalFeatureMap& getGlobalFeatures() const { return m_global_features; }
    // GlobalClassifier::classifyWithKNN (:242-347) on the neighbours of one query, in the search's order
    static VotingMaximum::GlobalHypothesis classifyWithKNN(int k, const unsigned* n_class, const unsigned* n_inst, const float* n_dist, unsigned max_class, bool single_object_mode);
    // the merge sequence of voting.cpp:272-323 on maxima whose weights carry the first normalisation: normalizeWeights (except function
    // 5), mergeGlobalAndLocalHypotheses, sort, erase zero weights, normalizeWeights, MinThreshold, BestK. Pure host code.
    struct MergeParams { int function = 3; float radius = 0, min_threshold = 0; int best_k = -1; float min_svm_score = 0.70f, rate_limit = 0.60f, weight_factor = 1.5f; };
    static void mergeSequence(std::vector<VotingMaximum>& maxima, const MergeParams& p);
    // diagnostics (tests): what the global step of the last findMaxima saw and decided
    struct GlobalDump { int k = 0, dim = 0; std::vector<int32_t> region_obj, region_max; std::vector<uint32_t> n_sel; std::vector<float> centroid, radius, desc;
                        std::vector<int32_t> knn_idx; std::vector<float> knn_dist, hyp_w; std::vector<uint32_t> hyp_id;      // hyp_w / hyp_id: 2 per region
                        std::vector<uint32_t> max_off; std::vector<int32_t> max_cls, max_inst; std::vector<float> max_w, max_iw, max_pos;
                        // rows of region r: row_off[r] .. row_off[r + 1] (one each but for CVFH); desc, knn_idx and knn_dist are per ROW
                        std::vector<uint32_t> row_off;
                        std::vector<float> box; };   // 10 per region: position, size, rotQuat of the box made for an object without maxima, NaN where none was
    const GlobalDump& lastGlobal() const { return m_last_global; }
    void clear();
    bool isSingleObjectMode() const { return m_single_object_mode; }
    bool refineModelRequested() const { return m_refine_model; }   // RansacRefineModel: refused when the config is read
    // Voting::forwardBoxesAndRadii (voting.cpp:496-551): per class (mean object radius, mean median box edge) and their variances
    void forwardBoxesAndRadii(const std::map<unsigned, std::vector<std::array<float, 3>>>& box_sizes, const std::map<unsigned, std::vector<float>>& object_radii);
    const std::map<unsigned, std::pair<float, float>>& getDimensionsMap() const { return m_dimensions_map; }
    const std::map<unsigned, std::pair<float, float>>& getVarianceMap() const { return m_variance_map; }
    void setDimensions(unsigned class_id, float radius, float box, float radius_var, float box_var) { m_dimensions_map[class_id] = {radius, box}; m_variance_map[class_id] = {radius_var, box_var}; }
    void save(BoostBinaryOArchive& oa) const;     // Voting::iSaveData (voting.cpp:559-614)
    bool load(BoostBinaryIArchive& ia);           // Voting::iLoadData (voting.cpp:616-734)
protected:
    // MaximaHandler::getSearchDistForClass (maxima_handler.cpp:509-521) for every class; empty = the configured radius for all
    std::vector<float> searchDistPerClass(float radius, int n_classes) const;
    std::map<unsigned, std::pair<float, float>> m_dimensions_map, m_variance_map;
    friend class Codebook;
    virtual void iFindMaxima(DeviceSession& s, std::vector<std::vector<VotingMaximum>>& out) = 0;
    virtual float mergeRadius() const = 0;                       // MaximaHandler::getRadius(): Bandwidth (mean shift), BinSize[0] / 2 (Hough)
    void verifyWithGlobalFeatures(DeviceSession& s, int metric, std::vector<std::vector<VotingMaximum>>& out);
    // device outputs of ismhip_find_maxima / ismhip_hough3d_maxima -> VotingMaximum lists
    struct MaximaBuffers;                                        // defined in ism3d.cpp (device buffers)
    static bool collectMaxima(DeviceSession& s, MaximaBuffers& b, std::vector<std::vector<VotingMaximum>>& out, bool with_quat);
    // the search both back ends share: P (ismhip_maxima_params / ismhip_hough_params) with the back end's own fields, its two entry points
    template <typename Params, typename Entry, typename RansacEntry>
    void searchMaxima(DeviceSession& s, Params P, Entry entry, RansacEntry ransac_entry, const char* what, std::vector<std::vector<VotingMaximum>>& out) const;
    int singleObjectMaxType() const;                             // ISMHIP_SOM_* from SingleObjectMode / SingleObjectMaxType
    int maxFilter() const;                                       // ISMHIP_MAXFILTER_* from MaxFilterType
    // RANSAC vote filter (voting.cpp:110-127): per-class inlier thresholds (empty = the configured one for all) and the device call's parameters
    std::vector<float> ransacThresholdPerClass(int n_classes) const;
    void fillRansacParams(DeviceSession& s, const std::vector<float>& class_thr, ismhip_ransac_params& R) const;
    float m_minThreshold; int m_minVotesThreshold; int m_bestK; bool m_averageRotation;
    std::string m_radiusType; float m_radiusFactor; std::string m_max_filter_type, m_max_type_param;
    bool m_single_object_mode; bool m_use_global_features; bool m_vote_filtering_with_ransac;
    bool m_refine_model; float m_inlier_threshold; std::string m_inlier_threshold_type;      // RansacRefineModel, RansacInlierThreshold(Type)
    std::string m_global_feature_method; int m_k_global_features, m_merge_function, m_min_points;             // voting.cpp:39-45
    float m_min_svm_score, m_rate_limit, m_weight_factor;
    const GlobalFeatures* m_global_descriptor = nullptr;         // owned by the model
    GlobalFeatureMap m_global_features;
    GlobalDump m_last_global;
};
class VotingHough3D : public Voting {             // voting/voting_hough_3d.{h,cpp}
public:
    VotingHough3D();
    static std::string getTypeStatic() { return "Hough3D"; }
    std::string getType() const override { return getTypeStatic(); }
protected:
    void iFindMaxima(DeviceSession& s, std::vector<std::vector<VotingMaximum>>& out) override;
    float mergeRadius() const override { return (float)(m_binSize[0] / 2); }
private:
    bool m_useInterpolation; Vec3d m_minCoord, m_maxCoord, m_binSize; float m_relThreshold;
};
class VotingMeanShift : public Voting {
public:
    VotingMeanShift();
    static std::string getTypeStatic() { return "MeanShift"; }
    std::string getType() const override { return getTypeStatic(); }
protected:
    void iFindMaxima(DeviceSession& s, std::vector<std::vector<VotingMaximum>>& out) override;
    float mergeRadius() const override { return m_bandwidth; }
private:
    float m_bandwidth, m_threshold; int m_maxIter; std::string m_kernel, m_maxima_suppression_type;
};

// ---- Factory (utils/factory.h) ---------------------------------------------------------------------------
template <typename TClass>
class Factory {
public:
    static TClass* create(const Json& object) {
        if (object.isNull()) return nullptr;
        std::string typeStr;
        if (const Json* t = object.find("Type")) { if (t->type != Json::String) return nullptr; typeStr = t->str; }
        TClass* inst = createByType(typeStr);
        if (!inst || !inst->configFromJson(object)) { delete inst; throw RuntimeException("could not create object of type: \"" + typeStr + "\""); }
        return inst;
    }
private:
    static TClass* createByType(const std::string& type);
};

// ---- ImplicitShapeModel (implicit_shape_model.h:82) -------------------------------------------------------
class ImplicitShapeModel : public JSONObject {
public:
    ImplicitShapeModel();
    ~ImplicitShapeModel();
    std::string getType() const override { return "ImplicitShapeModel"; }

    void clear();
    bool addTrainingModel(const std::string& filename, unsigned class_id, unsigned instance_id);
    bool addTrainingModel(const PointCloud& cloud, unsigned class_id, unsigned instance_id);   // in-memory variant (harness/tests)
    void train();

    std::tuple<std::vector<VotingMaximum>, std::map<std::string, double>> detect(const PointCloud& pointCloud, bool hasNormals = true);
    bool detect(const std::string& filename, std::vector<VotingMaximum>& maxima, std::map<std::string, double>& times);
    // batched fast path (new): descriptors -> kNN -> votes -> maxima stay on the device across many objects
    std::vector<std::vector<VotingMaximum>> detectBatch(const std::vector<const PointCloud*>& clouds);

    const Codebook* getCodebook() const { return m_codebook.get(); }
    // diagnostics (tests): the features of the last train() (which = 0) or detectBatch() (which = 1) and the vote space of the last
    // detectBatch(), copied to the host
    struct FeatureDump { int dim = 0; uint32_t n = 0; std::vector<uint32_t> off; std::vector<float> desc, lrf, kx, ky, kz;
                         std::vector<unsigned> cls, model; std::vector<float> center; };
    struct VoteDump { std::vector<uint32_t> slot_off; std::vector<float> pos, weight; std::vector<int32_t> cls, inst; };
    FeatureDump lastFeatures(int which) const;
    const std::vector<BoundingBox>& lastTrainingBoxes() const { return m_last_boxes; }
    VoteDump lastVotes() const;
    // diagnostics (tests): a timer or counter of the device library's context (ismhip_timer_get); 0 before the first device call
    double deviceTimer(const std::string& name) const;
    const Voting* getVoting() const { return m_voting.get(); }
    Voting* getVoting() { return m_voting.get(); }
    const GlobalFeatures* getGlobalFeatures() const { return m_global_descriptor.get(); }
    const Features* getFeatures() const { return m_feature_descriptor.get(); }
    void setSignalsState(bool) {}
    void setLogging(bool l) { m_logging = l; }
    void setLabels(std::map<unsigned, std::string>& c, std::map<unsigned, std::string>& i, std::map<unsigned, unsigned>& m) { m_class_labels = c; m_instance_labels = i; m_instance_to_class_map = m; }
    std::map<unsigned, std::string> getClassLabels() { return m_class_labels; }
    std::map<unsigned, std::string> getInstanceLabels() { return m_instance_labels; }
    std::map<unsigned, unsigned> getInstanceClassMap() { return m_instance_to_class_map; }
    bool isInstancePrimaryLabel() { return m_instance_labels_primary; }
    const std::map<std::string, double>& getProcessingTimes() const { return m_processing_times; }
    int numClasses() const { return m_n_classes; }
    // test / tooling access to what travels in the data file
    void setCodebookData(const CodebookData& d, int n_classes) { m_codebook->setData(d); m_n_classes = n_classes; }
    void setLabels(const std::vector<std::string>& cls, const std::vector<std::string>& inst, const std::vector<unsigned>& inst_to_class) {
        m_class_labels.clear(); m_instance_labels.clear(); m_instance_to_class_map.clear();
        for (size_t i = 0; i < cls.size(); ++i) m_class_labels[(unsigned)i] = cls[i];
        for (size_t i = 0; i < inst.size(); ++i) { m_instance_labels[(unsigned)i] = inst[i]; m_instance_to_class_map[(unsigned)i] = inst_to_class[i]; }
    }
    std::string getLabel(int which, unsigned id) const { const auto& m = which == 0 ? m_class_labels : m_instance_labels; auto it = m.find(id); return it == m.end() ? std::string() : it->second; }
    bool getDimensions(unsigned class_id, float* out4) const;
    void setDimensions(unsigned class_id, const float* in4);
    void setDevice(int device) { m_device = device; }

    static std::shared_ptr<PointCloud> loadPointCloud(const std::string& file);

protected:
    Json iChildConfigsToJson() const override;
    bool iChildConfigsFromJson(const Json&) override;
    void iSaveData(std::ostream&) const override;
    bool iLoadData(std::istream&) override;
    void iPostInitConfig() override;

private:
    DeviceSession& session();
    int metric() const;
    std::shared_ptr<DeviceFeatures> computeFeatures(const std::vector<const PointCloud*>& clouds, bool is_training);
    // the enabled pre-filters (SOR, ROR, z cut-off) on a batch, in that order; returns `clouds` itself when none is enabled, else
    // pointers to the filtered copies it puts into `store`
    std::vector<const PointCloud*> preFilterClouds(const std::vector<const PointCloud*>& clouds, std::vector<std::unique_ptr<PointCloud>>& store);

    std::string m_distanceType, m_bounding_box_type;
    float m_normal_radius; int m_consistent_normals_method, m_num_threads, m_num_kd_trees;
    bool m_flann_exact_match, m_instance_labels_primary, m_single_object_mode_legacy;
    bool m_use_smoothing, m_use_sor, m_use_ror, m_use_voxel_filtering;
    int m_sor_mean_k, m_ror_min_neighbors;
    float m_sor_stddev_mul, m_ror_radius, m_cutoff_distance_z;
    std::unique_ptr<Codebook> m_codebook;
    std::unique_ptr<Keypoints> m_keypoints_detector;
    std::unique_ptr<Features> m_feature_descriptor;
    std::unique_ptr<Voting> m_voting;
    std::unique_ptr<Clustering> m_clustering;
    std::unique_ptr<FeatureRanking> m_feature_ranking;
    Json m_global_features_cfg;                                  // the GlobalFeatures child as read: written back unchanged
    std::unique_ptr<GlobalFeatures> m_global_descriptor;         // the object of a built type (nullptr: pass-through)
    std::map<unsigned, std::vector<std::shared_ptr<PointCloud>>> m_training_clouds;     // class -> models
    std::map<unsigned, std::vector<unsigned>> m_training_instances;
    std::map<unsigned, std::string> m_class_labels, m_instance_labels;
    std::map<unsigned, unsigned> m_instance_to_class_map;
    std::map<std::string, double> m_processing_times;
    int m_n_classes = 0;
    bool m_logging = true;
    int m_device = 0;
    std::unique_ptr<DeviceSession> m_session;
    std::shared_ptr<DeviceFeatures> m_last_train, m_last_detect;            // for lastFeatures()
    std::vector<unsigned> m_last_fclass, m_last_fmodel; std::vector<float> m_last_fcenter;
    std::vector<BoundingBox> m_last_boxes;                                  // the last train()'s box per training object, in training order
};

// list files of eval_tool (eval_tool/eval_helpers.h:100-177)
struct FileList {
    std::vector<std::string> filenames; std::vector<unsigned> class_labels, instance_labels; std::string mode; bool using_instances = false;
    std::map<std::string, unsigned> class_labels_map, instance_labels_map; std::map<unsigned, std::string> class_labels_rmap, instance_labels_rmap;
    std::map<unsigned, unsigned> instance_to_class_map;
};
FileList parseFileList(const std::string& input_file_name);

}  // namespace ism3d
