/*
 * ismhip.h — C ABI of the MI355X-native implicit_shape_model recognition hot path.
 *
 * This is the drop-in boundary: every entry point replaces one plugin seam of the
 * reference (vseib/point-cloud-donkey, paths relative to /root/reference/src/implicit_shape_model).
 * The reference has no FFI of its own (its seams are C++ virtuals created by Factory<T>,
 * utils/factory.h:24-46), so the functions below are what a maintainer binds from the
 * plugin classes; INTEGRATION.md shows the stubs.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, int status (0 = ok, <0 = error); no exception crosses.
 *   - pointers are DEVICE pointers unless the parameter name ends in _h (host).
 *   - every call takes an ismhip_ctx (device, stream, scratch arena) and is asynchronous on the
 *     ctx stream; outputs are valid after ismhip_sync() or after a stream-ordered consumer.
 *   - one ctx per host thread / GPU; calls on different ctxs are re-entrant.
 *   - object batches: "n_obj" objects are concatenated; X_offsets_h[n_obj+1] gives the element
 *     range of each object in the concatenated arrays (points, keypoints/features, vote slots).
 *   - there is exactly ONE back end (HIP, gfx950). If no GPU is present ismhip_ctx_create fails.
 */
#ifndef ISMHIP_H_
#define ISMHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISMHIP_ABI_VERSION 4

#define ISMHIP_OK               0
#define ISMHIP_ERR_INVALID     -1   /* bad argument (null pointer, negative size, unsupported value) */
#define ISMHIP_ERR_HIP         -2   /* a HIP runtime call failed; see ismhip_last_error */
#define ISMHIP_ERR_NOMEM       -3   /* device allocation failed */
#define ISMHIP_ERR_UNSUPPORTED -4   /* valid in the reference, not built here */
#define ISMHIP_ERR_NODEVICE    -5   /* no gfx950 device visible: the product path has no CPU fallback */

/* distance metric: utils/distance.h:45,65 (FLANN functors; L2 is SQUARED, no sqrt) */
#define ISMHIP_METRIC_L2SQ 0
#define ISMHIP_METRIC_CHI2 1

/* vote weight flags: codebook/codebook.cpp:32-35 */
#define ISMHIP_W_CLASS    1u
#define ISMHIP_W_VOTE     2u
#define ISMHIP_W_MATCHING 4u
#define ISMHIP_W_CODEWORD 8u

/* mean-shift kernel: voting/voting_mean_shift.cpp:378-417 */
#define ISMHIP_KERNEL_GAUSSIAN 0
#define ISMHIP_KERNEL_UNIFORM  1
/* maxima suppression: voting/voting_mean_shift.cpp:99-122 */
#define ISMHIP_SUPPRESS_AVERAGE  0
#define ISMHIP_SUPPRESS_SUPPRESS 1
#define ISMHIP_SUPPRESS_NONE     2
/* inter-class maxima filter: voting/maxima_handler.cpp:272-296 ("Simple" = greedy non-maximum suppression over ALL classes inside
 * the search radius, suppressNeighborMaxima2 :227-268; "Merge" = mergeAndFilterMaxima :298-..., merging the maxima of the SAME class inside the radius first) */
#define ISMHIP_MAXFILTER_NONE   0
#define ISMHIP_MAXFILTER_SIMPLE 1
#define ISMHIP_MAXFILTER_MERGE  2
/* Voting.SingleObjectMaxType in SingleObjectMode (voting_mean_shift.cpp:80, 124-157; maxima_handler.h:45-46): "Default" / "None" (and
 * every type outside single-object mode) run the mean shift; the other three place ONE maximum per class at the cloud centroid */
#define ISMHIP_SOM_MEANSHIFT              0
#define ISMHIP_SOM_BANDWIDTH              1
#define ISMHIP_SOM_MODEL_RADIUS           2
#define ISMHIP_SOM_COMPLETE_VOTING_SPACE  3

#define ISMHIP_SHOT_DIM   352
#define ISMHIP_BSHOT_DIM  352     /* ismhip_bshot352: SHOT-352 binarised in groups of four */
#define ISMHIP_CSHOT_DIM 1344
#define ISMHIP_FPFH_DIM    33
#define ISMHIP_SHORT_SHOT_MAX_DIM 256   /* r_bins * e_bins * a_bins of ismhip_short_shot */
#define ISMHIP_COSPAIR_LEVELS 7     /* concentric shells of ismhip_cospair */
#define ISMHIP_COSPAIR_BINS   9     /* bins per pair feature and per colour channel */
#define ISMHIP_COSPAIR_DIM  378     /* 7 levels x (27 geometry + 27 colour) */
#define ISMHIP_SPIN_IMAGE_WIDTH 8   /* setImageWidth(8), features_spin_image.cpp:67 */
#define ISMHIP_SPIN_IMAGE_DIM 153   /* (8 + 1) * (2 * 8 + 1) */
#define ISMHIP_RSD_DIM 25           /* ismhip_rsd, full_histogram: 5 angle bins x 5 distance bins */
#define ISMHIP_RSD_RADII_DIM 2      /* ismhip_rsd without it: the two principal radii */
#define ISMHIP_RIFT_DISTANCE_BINS 8  /* rift_distance_bins, features_rift.cpp:38 */
#define ISMHIP_RIFT_GRADIENT_BINS 16 /* rift_gradient_bins, :39 */
#define ISMHIP_RIFT_DIM 128         /* 8 * 16 */
#define ISMHIP_VFH_DIM 308         /* ismhip_global_vfh: 4 shape blocks of 45 bins + 128 viewpoint bins */
#define ISMHIP_GASD_DIM 984        /* ismhip_global_gasd with colour: 6^3 shape bins + 4^3 cells x 12 hue bins */
#define ISMHIP_GASD_SHAPE_DIM 512  /* without colour: the 216 shape bins followed by 296 zeros (pcl::GASDSignature512) */
#define ISMHIP_SHORT_CSHOT_MAX_DIM 1344 /* r_bins * e_bins * a_bins + rc_bins * ec_bins * ac_bins * hist_size of ismhip_short_cshot; also the longest row of ismhip_knn_large_k above K = 16, ismhip_knn_threshold, ismhip_knn_binary and ismhip_rank_scores */
#define ISMHIP_KNN_MAX_DIM 2048    /* the longest row of ismhip_codebook_create, ismhip_knn (K <= 16), _ratio, _rule, ismhip_train_activate and ismhip_kmeans */
#define ISMHIP_USC_DIM 1960        /* ismhip_usc: 14 azimuth x 14 elevation x 10 radial bins */
#define ISMHIP_USC_AZIMUTH_BINS 14
#define ISMHIP_USC_ELEVATION_BINS 14
#define ISMHIP_USC_RADIAL_BINS 10

typedef struct ismhip_ctx      ismhip_ctx;
typedef struct ismhip_cloud    ismhip_cloud;
typedef struct ismhip_codebook ismhip_codebook;

/* ---- context ----------------------------------------------------------------------------- */
int  ismhip_abi_version(void);
/* stream: a hipStream_t (as void*) the caller owns, or NULL to let the ctx create its own. */
int  ismhip_ctx_create(int device, void* stream, ismhip_ctx** out);
/* same, but every value of stream is taken literally: NULL is the device's default (null) stream. This is how a host
 * that already owns a stream (e.g. torch.cuda.current_stream()) orders its own work with the library's. */
int  ismhip_ctx_create_on_stream(int device, void* stream, ismhip_ctx** out);
int  ismhip_ctx_destroy(ismhip_ctx* ctx);
/* waits for the context's stream. Also the place where asynchronous caps surface: if find_maxima / hough3d_maxima had to drop
 * maxima since the last call (more than 128 per object and class, or 1024 per object), it returns ISMHIP_ERR_UNSUPPORTED once
 * (message in ismhip_last_error) and clears the condition -- the reference has no such caps, so this is never silent. */
int  ismhip_sync(ismhip_ctx* ctx);
const char* ismhip_last_error(const ismhip_ctx* ctx);
/* per-kernel device timers (hipEvent on the ctx stream). Enable, run, sync, then read.
 * name: "grid","lrf","shot352","cshot1344","fpfh33","short_shot","short_cshot","cospair","bshot","knn","knn_binary","cast_votes","maxima","filter_sor","filter_ror","filter_compact","rank_scores","rank_select","global_short_shot","global_shot352","global_vfh","iss3d_saliency","iss3d_nms","keypoint_normals","spin_image","rsd","culling_pc","culling_scores","culling_select","intensity_gradients","rift","keypoint_normals_pca","cgf_raw","mlp_forward","esf_local"; ismhip_knn_threshold: "knn_threshold" and its
 * parts "knn_threshold_sweep", "knn_threshold_eval", "knn_threshold_exact", "knn_threshold_compact". Returns accumulated
 * milliseconds and launch count since the last reset. "knn_threshold_mfma_launches" is a counter (ms_out = number of radius
 * searches whose candidate sweep ran on the matrix cores), valid without timers; "knn_threshold_overflow_queries" the number of
 * queries of the last such search whose candidate list exceeded the per-query cap and went to the exact scan. */
int  ismhip_timers_enable(ismhip_ctx* ctx, int on);
int  ismhip_timers_reset(ismhip_ctx* ctx);
int  ismhip_timer_get(ismhip_ctx* ctx, const char* name, double* ms_out, int64_t* launches_out);

/* ---- search surface (replaces pcl::search::KdTree built at implicit_shape_model.cpp:823-831) ---
 * Takes the NaN-free surface cloud of n_obj objects as SoA and builds a per-object uniform grid
 * (y/z cell edge = cell_size, x cells three times finer; use 0.4 * min(Radius, ReferenceFrameRadius)) with the points counting-sorted
 * by cell. rgba may be NULL (needed only by cshot1344): packed as PCL does, 0x00RRGGBB. */
int  ismhip_cloud_create(ismhip_ctx* ctx, int n_obj, const uint32_t* pt_offsets_h,
                         const float* x, const float* y, const float* z,
                         const float* nx, const float* ny, const float* nz,
                         const uint32_t* rgba, float cell_size, ismhip_cloud** out);
int  ismhip_cloud_destroy(ismhip_ctx* ctx, ismhip_cloud* cloud);
/* Normals for clouds that come without them: ImplicitShapeModel::computeNormals, ConsistentNormalsMethod 2 (the default,
 * implicit_shape_model.cpp:1014-1018) -> NormalOrientation::processSHOTLRF (utils/normal_orientation.cpp:48-110): a SHOT
 * frame of radius NormalRadius at every point, normal = inverted z axis; NaN where the frame is invalid (< 5 neighbours).
 * The cloud may have been created with any normal arrays (their values are not read before this call); the outputs
 * (device, original point order, may alias the arrays given to ismhip_cloud_create) also replace the cloud's normals. */
int  ismhip_estimate_normals(ismhip_ctx* ctx, ismhip_cloud* cloud, float radius, float* nx_out, float* ny_out, float* nz_out);
/* ConsistentNormalsMethod 0 and 1 (implicit_shape_model.cpp:969-1011) -> pcl::NormalEstimationOMPWithEigVals
 * (third_party/pcl_normal_3d_omp_with_eigenvalues): PCA normal of the NormalRadius neighbourhood (>= 3 points, else NaN), flipped
 * towards the viewpoint. orientation 0: towards (0,0,0) (method 0); 1: away from the object's centroid (method 1). Outputs as
 * ismhip_estimate_normals. */
int  ismhip_estimate_normals_pca(ismhip_ctx* ctx, ismhip_cloud* cloud, float radius, int orientation, float* nx_out, float* ny_out, float* nz_out);
/* ImplicitShapeModel::filterNormals (implicit_shape_model.cpp:1034-1075): the points whose normal holds a NaN leave their cloud, order
 * kept, without the arrays leaving HBM. in / out: device SoA over all objects (out must not alias in; rgba may be NULL in both);
 * pt_offsets_h_out[n_obj+1] (host) receives the new ranges. The call synchronises. */
typedef struct ismhip_point_arrays { float *x, *y, *z, *nx, *ny, *nz; uint32_t* rgba; } ismhip_point_arrays;
int  ismhip_filter_normals(ismhip_ctx* ctx, int n_obj, const uint32_t* pt_offsets_h, const ismhip_point_arrays* in,
                           const ismhip_point_arrays* out, uint32_t* pt_offsets_h_out);
/* ---- point-cloud pre-filters: the first steps of ImplicitShapeModel::computeFeatures (implicit_shape_model.cpp:739-758, :810-821).
 *      PCL is external; the arithmetic is this library's definition, restated from PCL 1.10. Masks are device
 *      uint8_t[n_pts] in the ORIGINAL point order of the cloud, 1 = keep. A point that is not finite in x, y and z is never a
 *      neighbour and is always dropped. Every squared distance is the unfused float (dx*dx + dy*dy) + dz*dz. Results do not depend
 *      on the cell_size the cloud was created with. The filters are chained by the caller: mask -> ismhip_compact_points -> a new
 *      ismhip_cloud over the surviving points -> next filter. */
#define ISMHIP_SOR_MAX_MEAN_K 64
/* pcl::StatisticalOutlierRemoval (:739-748; MeanK, StddevMul :95-98): per finite point the mean_k + 1 smallest squared distances to the
 * finite points of its object (itself included, duplicates count), the smallest dropped, mean_dist = (float)(sum of sqrt((double)d2)
 * in ascending order / mean_k); per object in double mean, var = (sum d^2 - (sum d)^2 / n) / (n - 1), threshold = mean +
 * stddev_mul * sqrt(var), summed in a fixed order; keep iff !(mean_dist > threshold). An object with fewer than mean_k + 1 finite points
 * keeps all of them (threshold +inf, mean_dist NaN). mean_k < 1: ISMHIP_ERR_INVALID; mean_k > ISMHIP_SOR_MAX_MEAN_K is REFUSED with
 * ISMHIP_ERR_UNSUPPORTED (there is no slower path). mean_dist_out: device [n_pts] or NULL (NaN for the non-finite points);
 * threshold_h_out: host [n_obj] or NULL. Timer "filter_sor". The call synchronises. */
int  ismhip_filter_statistical(ismhip_ctx* ctx, const ismhip_cloud* cloud, int mean_k, float stddev_mul, uint8_t* keep_out,
                               float* mean_dist_out, double* threshold_h_out);
/* pcl::RadiusOutlierRemoval, radius-search branch (:749-758; the reference's clouds are is_dense = false :519,:612,:744): count =
 * finite points of the object with d2 < (float)((double)radius * radius), STRICTLY, the point itself included; keep iff
 * count > min_neighbors. count_out: device [n_pts] or NULL; when given it holds the full counts (0 for non-finite points), when NULL a
 * query stops counting once it is kept. Timer "filter_ror". Asynchronous. */
int  ismhip_filter_radius(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, int min_neighbors, uint8_t* keep_out, uint32_t* count_out);
/* pcl::PassThrough on z with limits (0, CutoffDistanceZAxis) (:810-821): keep iff the point is finite and !(z < z_min || z > z_max). */
int  ismhip_filter_passthrough_z(ismhip_ctx* ctx, uint32_t n_pts, const float* x, const float* y, const float* z, float z_min, float z_max,
                                 uint8_t* keep_out);
/* Stable compaction of the point arrays by a keep mask (device uint8_t[n_pts], 1 = keep): as ismhip_filter_normals, with the mask in
 * place of the NaN-normal test. Normals and colours travel with their points. Timer "filter_compact". The call synchronises. */
int  ismhip_compact_points(ismhip_ctx* ctx, int n_obj, const uint32_t* pt_offsets_h, const ismhip_point_arrays* in, const uint8_t* keep,
                           const ismhip_point_arrays* out, uint32_t* pt_offsets_h_out);
/* per-object centroid (features_shot.cpp:45-51) -> centroid_out[n_obj*3] */
int  ismhip_cloud_centroids(ismhip_ctx* ctx, const ismhip_cloud* cloud, float* centroid_out);
/* SingleObjectHelper::getModelRadius (voting/single_object_mode_helper.cpp:15-27): per object the largest distance of a (finite)
 * point from centroid[n_obj*3] (device, e.g. ismhip_cloud_centroids) -> radius_out[n_obj] (device) */
int  ismhip_cloud_radii(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* centroid, float* radius_out);

/* ---- local reference frames: Features::computeSHOTReferenceFrames (features/features.cpp:238-252)
 *      -> pcl::SHOTLocalReferenceFrameEstimationOMP (arithmetic as third_party/pcl_shot_na_lrf/shot_na_lrf.hpp:48-178
 *      with upstream's v.z sign rule). lrf9_out[nkp*9] row-major [x;y;z]; all-NaN when <5 neighbours. */
int  ismhip_shot_lrf(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                     const float* kpx, const float* kpy, const float* kpz,
                     float radius, float* lrf9_out);
/* ReferenceFrameType "SHOTNA": Features::computeSHOTNAReferenceFrames (features/features.cpp:254-279) ->
 * pcl::SHOTNALocalReferenceFrameEstimation::getLocalRF (third_party/pcl_shot_na_lrf/shot_na_lrf.hpp:48-178). The SHOT frame with one
 * change: the sign of z is voted by the NORMALS of all points inside the ball (double(normal) . v3 >= 0; a point that coincides with
 * the keypoint votes too, a NaN normal never counts as plus); a tied vote goes to the five median neighbours by position, as in SHOT.
 * The normals are the ones the cloud holds when this is called: those given to ismhip_cloud_create, or the ones a later
 * ismhip_estimate_normals / ismhip_estimate_normals_pca installed. The x sign counts the valid neighbours only (upstream PCL's loop
 * bound; the reference's loop also reads rows of vij it never wrote). Arguments, output layout, NaN rows and the timer
 * key "lrf" are those of ismhip_shot_lrf. */
int  ismhip_shotna_lrf(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                       const float* kpx, const float* kpy, const float* kpz,
                       float radius, float* lrf9_out);

/* ---- descriptors: FeaturesSHOT::iComputeDescriptors (features/features_shot.cpp:28-81) ------
 * desc_out[nkp*352]; NaN row when LRF non-finite or <5 neighbours. neighbour_count_out may be NULL
 * (else [nkp] number of radius neighbours, the M_k of the roofline model). */
int  ismhip_shot352(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                    const float* kpx, const float* kpy, const float* kpz,
                    const float* lrf9, float radius, float* desc_out, uint32_t* neighbour_count_out);
/* FeaturesBSHOT::getBinaryVector (features/features_bshot.cpp:109-157) on n_rows rows of 352 floats, in groups of four (v0..v3); dst may be
 * src. Every element of dst is 0.0f or 1.0f. Exactly the reference's text: sum = ((v0 + v1) + v2) + v3 in float, unfused; a group with
 * sum == 0 gives 0000; every test is (double)lhs > (double)sum * 0.9 (the literal 0.9 is a double), the lhs of a pair vi + vj and of a
 * triple (vi + vj) + vk in float in the written index order; case B sets the bit of every single element that passes and holds when one
 * bit is set; otherwise case C runs the six pair tests in the order 01, 02, 03, 12, 13, 23, the last one that passes overwriting the
 * result, and holds when two bits are set; otherwise case D runs the triples 012, 013, 023, 123 likewise and holds with three bits;
 * otherwise 1111. The result carries over between the cases as the reference writes it, so two consequences are kept:
 *  - two bits left by case B stand when no pair test passes, and count as case C (possible with negative elements only);
 *  - a group that holds a NaN gives 1111 (sum != 0 is true, every comparison false): a SHOT row that is NaN as a whole becomes 352 ones
 *    and is NOT removed by ismhip_compact_descriptor_rows. Timer "bshot". */
int  ismhip_bshot_binarize(ismhip_ctx* ctx, int n_rows, const float* src, float* dst);
/* FeaturesBSHOT::iComputeDescriptors (features/features_bshot.cpp:40-107): the arguments of ismhip_shot352; desc_out[nkp*352] =
 * ismhip_bshot_binarize of the rows ismhip_shot352 writes on the same inputs (a separate kernel behind k_shot); neighbour_count_out as there. */
int  ismhip_bshot352(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                     const float* kpx, const float* kpy, const float* kpz,
                     const float* lrf9, float radius, float* desc_out, uint32_t* neighbour_count_out);
/* FeaturesCSHOT::iComputeDescriptors (features/features_cshot.cpp:28-103); kp_rgba = keypoint colours */
int  ismhip_cshot1344(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                      const float* kpx, const float* kpy, const float* kpz, const uint32_t* kp_rgba,
                      const float* lrf9, float radius, float* desc_out, uint32_t* neighbour_count_out);
/* FeaturesFPFH::iComputeDescriptors (features/features_fpfh.cpp:27-72) */
int  ismhip_fpfh33(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                   const float* kpx, const float* kpy, const float* kpz,
                   float radius, float* desc_out, uint32_t* neighbour_count_out);
/* FeaturesSHORTSHOT::compute_descriptor (features/features_short_shot.cpp:77-156) with compute_shape_descriptor (:159-243),
 * linear_interpolation (:246-260) and correct_bin (:263-283): the generalised Short SHOT on a spherical grid of r_bins x e_bins x a_bins
 * bins around the keypoint's frame. desc_out[nkp * r_bins*e_bins*a_bins]. Per keypoint with a finite frame [x;y;z]:
 *  - neighbours: d2 < (float)((double)radius * radius), d2 the unfused float (dx*dx + dy*dy) + dz*dz -- the predicate and the
 *    neighbour_count_out of ismhip_shot352; a neighbour with d2 <= 1e-15f (the SQUARED distance, :127) is skipped;
 *  - x_l = (double)((v.x*X.x + v.y*X.y) + v.z*X.z) in float, unfused, in this order (the reference's Eigen Vector4f::dot does not state
 *    its order: this one is the library's definition), likewise y_l, z_l; then in double r = sqrt(x_l^2 + y_l^2 + z_l^2), skipped if
 *    r < (double)min_radius, theta = acos(z_l / r) * 57.29578, phi = atan2(y_l, x_l) * 57.29578 (pcl::rad2deg(double) of PCL 1.10);
 *  - float raw_r = (float)(r_bins * r / (double)radius), or with log_radius (float)((r_bins - 1) * (log(r) - log(min_radius)) /
 *    log(radius / min_radius) + 1); float raw_theta = (float)(e_bins * theta / 180); float raw_phi = (float)(a_bins * (phi + 180) / 360);
 *    primary bins int(raw), r clamped to [0, r_bins - 1], theta and phi from above only; per axis decimals = raw - (int)raw (float),
 *    share f = decimals + 0.5 towards -1 if decimals <= 0.5f, else (1 - decimals) + 0.5 towards +1; a secondary bin exists for an axis
 *    with more than one bin when the corrected neighbour (r, theta clamp; phi wraps) differs from the primary; the primary bin receives
 *    f_r + f_theta + f_phi, the secondary bin of an axis the same sum with that axis' share replaced by 1 - f;
 *    bin index = bin_r + bin_theta * r_bins + bin_phi * r_bins * e_bins;
 *  - the row is divided by its L2 norm (double) and cast to float. ONE contributing neighbour is enough (no five-neighbour rule); none
 *    gives 0 / 0: the row is NaN AS A WHOLE (:143-152), as for a non-finite frame or keypoint (count 0).
 * The caller derives min_radius (:88-103): Radius * ShortShotMinRadius with UseMinRadius, else 0.1 * Radius with ShortShotLogRadius, else 0.
 * Refused: a bin count < 1 or min_radius < 0 (ISMHIP_ERR_INVALID), more than ISMHIP_SHORT_SHOT_MAX_DIM bins (ISMHIP_ERR_UNSUPPORTED),
 * log_radius without 0 < min_radius < radius (ISMHIP_ERR_INVALID: the reference divides by log(radius / 0)-derived zeros). Timer "short_shot". */
int  ismhip_short_shot(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                       const float* kpx, const float* kpy, const float* kpz, const float* lrf9,
                       float radius, float min_radius, int log_radius, int r_bins, int e_bins, int a_bins,
                       float* desc_out, uint32_t* neighbour_count_out);
/* FeaturesSHORTCSHOT::compute_descriptor (features/features_short_cshot.cpp:103-223) with compute_shape_descriptor (:225-310),
 * compute_color_descriptor (:312-429), linear_interpolation (:432-443) and correct_bin (:487-507): the Short SHOT followed by its colour
 * histogram. desc_out[nkp * D], D = r_bins*e_bins*a_bins + rc_bins*ec_bins*ac_bins*hist_size. Per keypoint with a finite frame:
 *  - neighbours, local coordinates, r, theta, phi, the d2 <= 1e-15f and r < min_radius skips: those of ismhip_short_shot, for both parts;
 *  - shape part, bins [0, r_bins*e_bins*a_bins): exactly the row ismhip_short_shot accumulates BEFORE its norm;
 *  - colour part: the raw r / theta / phi values are formed again with the colour grid's bin counts (rc, ec, ac), so a neighbour takes
 *    a second, independent set of primary bins, shares f and secondary bins; float raw_c = (float)(cd * hist_size) with cd the CSHOT
 *    colour distance of ismhip_cshot1344 on normalised CIELab, (|dL| + (|da| + |db|) / 2) / 3 clamped to [0, 1], between the neighbour's
 *    colour and the KEYPOINT's own colour kp_rgba (0x00RRGGBB); bin_c = int(raw_c) clamped from above only, its share and secondary bin
 *    as for theta (clamps); an axis with one bin has no secondary bin; bin index = Ds + bin_c + hist_size * (bin_r + rc_bins *
 *    (bin_theta + ec_bins * bin_phi)); up to five deposits, float sums in this order: primary (f_c + f_r) + f_theta + f_phi; phi's
 *    secondary the same with 1 - f_phi; theta's with 1 - f_theta; r's with 1 - f_r; the secondary COLOUR bin receives
 *    (1 - f_c) + (1 - f_r) + f_theta + f_phi -- with 1 - f_r, not f_r, exactly as the reference writes it (:424): bug-compatible;
 *  - the two parts, shape first, are divided by their JOINT L2 norm (double) and cast to float; no contributing neighbour gives 0 / 0:
 *    the row is NaN AS A WHOLE, as for a non-finite frame or keypoint (count 0).
 * Deviations from the reference's text: the three of ismhip_short_shot (dot-product order, Radius and min_radius as float, 57.29578), and
 * the colour distance is taken in float as in PCL's cshot.hpp and ismhip_cshot1344 (the reference's unqualified fabs pins neither).
 * The caller derives min_radius as for ismhip_short_shot and the colour grid from ShortColorShotDims (configureSphericalColorGrid, :592-646).
 * Refused, never altered: a bin count or hist_size < 1, min_radius negative or not finite, missing colour arrays (cloud made without
 * rgba, or kp_rgba NULL), log_radius without 0 < min_radius < radius (ISMHIP_ERR_INVALID); more than ISMHIP_SHORT_SHOT_MAX_DIM shape
 * bins or a row longer than ISMHIP_SHORT_CSHOT_MAX_DIM (ISMHIP_ERR_UNSUPPORTED). Timer "short_cshot". */
int  ismhip_short_cshot(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                        const float* kpx, const float* kpy, const float* kpz, const uint32_t* kp_rgba, const float* lrf9,
                        float radius, float min_radius, int log_radius, int r_bins, int e_bins, int a_bins,
                        int rc_bins, int ec_bins, int ac_bins, int hist_size, float* desc_out, uint32_t* neighbour_count_out);
/* FeaturesCospair::iComputeDescriptors (features/features_cospair.cpp:28-77) -> COSPAIR::ComputeCOSPAIR (third_party/cospair/cospair.cpp:
 * 18-294) with the parameters the reference hard-codes (7 levels, 9 bins, rgb_type 5 = CIELab, 9 colour bins). desc_out[nkp * 378]: for
 * level l = 1..7 the block at (l - 1) * 54 holds a geometry array (f1 bins 0..8, f2 bins 9..17, f3 bins 18..26) and a colour array (L, a, b
 * likewise). Needs no frame and no keypoint colour; the cloud must have been created with rgba. Per keypoint:
 *  - the centre is the finite cloud point NEAREST to the keypoint (d2 the unfused float (dx*dx + dy*dy) + dz*dz; among equal distances
 *    the lowest original index), however far away; its position and normal are the source of every pair;
 *  - level l owns the points with r2_{l-1} <= d2 < r2_l, d2 to the CENTRE, r2_l = (float)(r_l * r_l), r_l = ((double)l / 7) * (double)radius,
 *    r2_0 = 0; the centre itself is dropped by index (coincident duplicates of it are ordinary level-1 pairs);
 *  - a neighbour whose normal is not finite is skipped and not counted; every other one counts in its level and deposits +1 at
 *    bin_f1, 9 + bin_f2, 18 + bin_f3 of the geometry array: (f1, f2, f3) = PCL 1.10 computePairFeatures(centre, neighbour) in float, all
 *    zero for a degenerate pair; deg_f1 = f1 * 57.29578f + 180, deg = acosf(clamp(f, -1, 1)) * 57.29578f for f2 and f3;
 *    bin = int(floor((double)deg / 40.0)) for f1, / 20.0 for f2 and f3; and +1 at bin_l, 9 + bin_a, 18 + bin_b of the colour array:
 *    (L, a, b) = PCL's RGB2CIELAB of the NEIGHBOUR's colour, l' = (float)(1.0 * L / 100), a' = (float)((a + 86.185) / 184.439),
 *    b' = (float)((b + 107.863) / 202.345) (sums and divisions in double), bin = int(floor((double)x' / (1.0 / 9)));
 *  - an index offset + bin that stays inside [0, 27) is used as it is (a bin 9 of f1, f2, L or a lands on bin 0 of the next feature, as
 *    in the reference); one that leaves the array (undefined in the reference) is clamped to 0 or 26;
 *  - every entry of a level with n pairs becomes ((float)count / (float)n) * (float)l; an empty level stays zero; no final normalisation.
 * A keypoint that is not finite, an object without a finite point and a centre whose normal is not finite give a row that is NaN AS A WHOLE
 * with counts 0. neighbour_count_out[nkp]: the sum of the level pair counts; level_count_out[nkp * 7]; snap_index_out[nkp]: the object-local
 * original index of the centre, 0xffffffff for a NaN row; each may be NULL. Refused with ISMHIP_ERR_INVALID: a missing array or a
 * radius that is not positive ("cospair: bad argument"), a cloud made without rgba ("cospair: colour arrays missing"). Timer "cospair".
 * The per-point colour indices are built by the first call on a cloud and kept with it. */
int  ismhip_cospair(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                    const float* kpx, const float* kpy, const float* kpz, float radius, float* desc_out,
                    uint32_t* neighbour_count_out, uint32_t* level_count_out, uint32_t* snap_index_out);
/* The normal lookup of FeaturesSpinImage::iComputeDescriptors (features/features_spin_image.cpp:36-53): for every keypoint the installed
 * normal of the LOWEST original index among the object's finite points whose three coordinates compare == to the keypoint's -> knx_out,
 * kny_out, knz_out [nkp]; src_index_out[nkp] (may be NULL): that object-local index, -1 when nothing matches. No match (and a keypoint that
 * is not finite) gives the normal (0, 0, 0), the reference's default-constructed pcl::Normal. A matched point's normal is handed over as
 * it is, finite or not (the host filters such points before this step). Only the keypoint's own grid cell is read. Refused with
 * ISMHIP_ERR_INVALID: a missing array ("keypoint_normals: bad argument"). Timer "keypoint_normals". */
int  ismhip_keypoint_normals(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                             const float* kpx, const float* kpy, const float* kpz,
                             float* knx_out, float* kny_out, float* knz_out, int32_t* src_index_out);
/* FeaturesSpinImage::iComputeDescriptors (features/features_spin_image.cpp:28-87) -> PCL 1.10 SpinImageEstimation::computeSiForPoint as
 * :61-69 configure it: rectangular image, support-angle cosine 0 (neighbour normals are never read), min_pts_neighb 0; the reference's
 * image_width is 8 (ISMHIP_SPIN_IMAGE_WIDTH, 153 floats). desc_out[nkp * (w + 1)(2w + 1)], w = image_width: element ia * (2w + 1) + ib is
 * entry (ia, ib) of the image. Per keypoint with centre c and axis n = (ax, ay, az)[k] (every float product and sum unfused, as written):
 *  - neighbours: the finite cloud points with d2 < (float)((double)radius * radius), d = p - c, d2 = (d.x*d.x + d.y*d.y) + d.z*d.z in float;
 *    neighbour_count_out[nkp] (may be NULL) counts them all, the skipped ones too;
 *  - norm = sqrtf(d2); (double)norm < 10 * DBL_EPSILON: skipped; dot = (d.x*n.x + d.y*n.y) + d.z*n.z in float; from here in double:
 *    cos = dot / norm; |cos| > 1 + 10 * FLT_EPSILON (or cos no number): the keypoint's WHOLE row is NaN (PCL throws); else cos clamped to [-1, 1],
 *    beta = norm * cos, alpha = norm * sqrt(1 - cos * cos), bin = (double)radius / w / sqrt(2.0), lim = bin * w; |beta| >= lim or
 *    alpha >= lim: skipped; ib = (int)floor(beta / bin) + w, ia = (int)floor(alpha / bin), a = alpha / bin - ia, b = beta / bin - (ib - w);
 *    deposits (1-a)(1-b), a(1-b), (1-a)b, ab at (ia, ib), (ia+1, ib), (ia, ib+1), (ia+1, ib+1); an entry outside the matrix (reached only
 *    when a quotient rounds up onto w, with a weight of rounding size) is dropped;
 *  - every deposit enters a 64-bit integer bin as round(v * 2^28); S = the integer sum of the bins. More than one neighbour:
 *    row[i] = (float)((double)h_i / (double)S), S == 0 giving the reference's NaN row; otherwise row[i] = (float)(h_i * 2^-28).
 * A ball that holds no point gives a ZERO row and count 0. A keypoint or an axis that is not finite gives a row that is NaN AS A WHOLE
 * and count 0. An axis of (0, 0, 0) -- what ismhip_keypoint_normals returns for a keypoint that is no cloud point -- is used as it is:
 * every cosine is 0 and only column w fills. Two calls give the same bits. Refused: a missing array, a radius that is not positive,
 * image_width < 1 (ISMHIP_ERR_INVALID, "spin_image: bad argument"); image_width > 25, whose rows ismhip_knn would not take
 * (ISMHIP_ERR_UNSUPPORTED). Timer "spin_image". */
int  ismhip_spin_image(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                       const float* kpx, const float* kpy, const float* kpz, const float* ax, const float* ay, const float* az,
                       float radius, int image_width, float* desc_out, uint32_t* neighbour_count_out);
/* ---- Unique Shape Context (Features type "USC", features/features_usc.cpp -> pcl::UniqueShapeContext). PCL is external: the arithmetic
 *      below is THIS library's definition, written from knowledge of PCL 1.10's usc.hpp; parity with PCL is unpinned. */
/* density_out[n_pts] (cloud order): for every finite cloud point the number of finite points of the SAME object with
 * d2 < (float)((double)density_radius * density_radius), d2 = (dx*dx + dy*dy) + dz*dz in float -- the point itself included, so at
 * least 1; 0 for a point that is not finite. Exact and order free: the same bits for any grid cell size. Refused with
 * ISMHIP_ERR_INVALID ("point_density: bad argument"): a missing array, a radius that is not positive or not finite. Timer "point_density". */
int  ismhip_point_density(ismhip_ctx* ctx, const ismhip_cloud* cloud, float density_radius, uint32_t* density_out);
/* The tables of ismhip_usc for (radius, min_radius), computed on the host in double (libm):
 *   edges11[j]  = (float)exp(ln r_min + (j / 10.0) * ln(R / r_min)), j = 0 .. 10  (R = (double)radius, r_min = (double)min_radius)
 *   lut140[j * 14 + k] = 1 / cbrt( (cos th_k - cos th_{k+1}) * (e_{j+1}^3 - e_j^3) / 3 * (2 pi / 14) ),  th_k = k * pi / 14, e_j the
 *   DOUBLE edge before its rounding to float, j the radial and k the elevation bin.
 * Either output may be NULL. Refused (ISMHIP_ERR_INVALID): radius not positive or not finite, min_radius not in (0, radius). */
int  ismhip_usc_tables(float radius, float min_radius, double* lut140_out, float* edges11_out);
/* desc_out[nkp * 1960] (ISMHIP_USC_DIM). Grid: 14 azimuth bins of 360/14 degrees, 14 elevation bins of 180/14 degrees, 10 radial bins
 * with the edges of ismhip_usc_tables; bin index l * 140 + k * 10 + j (l azimuth, k elevation, j radial).
 *  - Frame: x = lrf9[0..2], y = lrf9[3..5], z = lrf9[6..8] of the keypoint (only x and z are read). A frame with a non-finite
 *    component, a keypoint that is not finite or a ball without a point: the WHOLE row NaN, count 0.
 *  - Ball: the finite cloud points of the keypoint's object with d2 < (float)((double)radius * radius), as ismhip_shot352;
 *    neighbour_count_out[nkp] (may be NULL) counts them all, the skipped ones too.
 *  - Per ball point p, v = p - keypoint (float), from here in double on the float inputs: |v|^2 = (v.x^2 + v.y^2) + v.z^2 <= FLT_EPSILON:
 *    skipped. r = sqrt(|v|^2); c = (z.v) / r clamped to [-1, 1], theta = acos(c) in degrees; u = v - (z.v) z; u == 0 (all three
 *    components): phi = 0 -- NAMED DEVIATION, PCL divides by zero there; else phi = atan2(|x cross u|, x.u) in degrees, replaced by
 *    360 - phi when (x cross u).z < 0.
 *    j = the first radial bin whose upper edge e_{j+1} (the float of the table, widened) is not below r; k = the first with
 *    (k + 1) * (180.0 / 14) not below theta; l = the first with (l + 1) * (360.0 / 14) not below phi. So r < r_min falls in j = 0.
 *    A value beyond the last edge takes the LAST bin -- NAMED DEVIATION, PCL's loop leaves it in bin 0.
 *  - Deposit: the integer q_p = (2^32 + n_p / 2) / n_p (64-bit integer division), n_p = max(1, density[p]) the point's density from
 *    ismhip_point_density; a bin holds Q = the sum of its q_p in 64 bits. q_out[nkp * 1960] (may be NULL) receives Q (0 for a NaN row).
 *  - Row: desc[i] = (float)((double)Q_i * 2^-32 * lut140[j * 14 + k]). No float atomics, no normalisation (the reference applies none).
 * The row depends on neither the order of the points nor the grid: two calls give the same bits. A row is NaN throughout or finite
 * throughout, never infinite. Balls of any size are served. Refused (ISMHIP_ERR_INVALID, "usc: bad argument"): a missing array (density
 * included), radius not positive or not finite, min_radius not in (0, radius). Timer "usc". */
int  ismhip_usc(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                const float* kpx, const float* kpy, const float* kpz, const float* lrf9, float radius, float min_radius,
                const uint32_t* density, float* desc_out, uint32_t* neighbour_count_out, unsigned long long* q_out);
/* FeaturesRSD::iComputeDescriptors (features/features_rsd.cpp:29-103) -> PCL 1.10 RSDEstimation::computeFeature / computeRSD as :41-56
 * configure it (5 subdivisions, max_dist = the search radius, plane_radius = Radius), then, for the histogram, normalizeDescriptors
 * (features/features.cpp:282-297). desc_out[nkp * 25] (ISMHIP_RSD_DIM) when full_histogram is not 0, else desc_out[nkp * 2]
 * (ISMHIP_RSD_RADII_DIM). Per keypoint with centre q, R = radius, D = (double)R; every float product and sum unfused, as written:
 *  - neighbours N: the finite cloud points with d2 < (float)(D * D), d = p - q, d2 = (d.x*d.x + d.y*d.y) + d.z*d.z in float, the
 *    keypoint's own cloud point included when it is one; neighbour_count_out[nkp] (may be NULL) = |N|;
 *  - for every unordered pair {i, j} of N, i != j by cloud index (coincident coordinates are still a pair), with normals ni, nj:
 *    c = (ni.x*nj.x + ni.y*nj.y) + ni.z*nj.z and d2 of the two points in float; c or d2 not finite: the pair is skipped;
 *    a = min(|c|, 1), theta = acos((double)a) in [0, pi/2], dist = sqrt((double)d2); dist > D: the pair is neglected;
 *    bd = floor(5 * dist / D), 5 (dist == D) becoming 4; ba = min(4, floor(5 * theta / (pi / 2))); count[ba + 5 * bd] += 1 (Eigen's
 *    column-major histogram(ba, bd)); per distance bin bd, amin[bd] = min a and amax[bd] = max a;
 *  - full_histogram: row[j] = (float)count[j] / 300.0f -- the reference divides by the sum of the INDICES 0..24; counts are uint32;
 *  - otherwise: theta_min[d] = acos(amax[d]), theta_max[d] = acos(amin[d]); bin 0 starts at theta_min = theta_max = 0, a bin without
 *    pairs is left out; in double and in bin order, f_d = (d + 0.5) * D / 5: Amin2 = sum theta_min^2, Amind = sum theta_min * f_d, Amax2
 *    and Amaxd likewise; rmin = Amin2 == 0 ? (float)D : (float)min(Amind / Amin2, D), rmax likewise, each times 1.1f in float; the row is
 *    [smaller, larger], not normalised.
 * |N| = 1: a zero row in either mode. |N| = 0, a keypoint that is not finite or a ball that misses the grid: the row NaN AS A WHOLE,
 * count 0 (PCL gives zeros for an empty neighbourhood). The row is made of integer counts and of minima and maxima only: two calls, any
 * grid cell size and any staging capacity (env ISMHIP_RSD_CAP, 64..256 in steps of 64; default 256) give the same bytes; larger
 * neighbourhoods are tiled, never truncated. Refused with ISMHIP_ERR_INVALID: a missing array, a radius that is not positive and finite
 * ("rsd: bad argument"). Timer "rsd". */
int  ismhip_rsd(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                const float* kpx, const float* kpy, const float* kpz, float radius, int full_histogram,
                float* desc_out, uint32_t* neighbour_count_out);
/* FeaturesESFLocal::iComputeDescriptors (features/features_esf_local.cpp:28-100) -> PCL 1.10 ESFEstimation (computeESF, lci, voxelize9,
 * scale_points_unit_sphere) on the Radius ball of every keypoint: the "ensemble of shape functions", desc_out[nkp * 640] (ISMHIP_ESF_DIM).
 * PCL draws with an unseeded rand(); this is the library's definition (deviations E1-E9). Per keypoint q, float32
 * throughout, every product and sum unfused and in the written order:
 *  1 neighbours N: the finite cloud points with d2 < (float)((double)radius * radius), d2 = (dx*dx + dy*dy) + dz*dz, the keypoint's own
 *    cloud point included; n = |N| -> neighbour_count_out[nkp] (may be NULL); N is indexed 0..n-1 in ASCENDING CLOUD INDEX; any n is
 *    taken: the first 1024 of them (the staging capacity; env ISMHIP_ESF_CAP = 1..1024 lowers it) are read from LDS, the others through
 *    a work list in device memory, never truncated;
 *  2 the row is NaN AS A WHOLE (and its bin counts 0) when n < 3, the keypoint is not finite, the ball misses the object (n = 0), the
 *    scale of step 3 is degenerate or the attempt cap of step 5 is reached;
 *  3 centroid c = (float)((double)q + mean(p - q)), the sum of the (double) differences in 64-bit fixed point, hence free of order;
 *    m = max |p - c|, |v| = sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z) of the float differences; m = 0, m or 32.0f / m not finite: NaN row;
 *    g = (p - c) * (32.0f / m) per coordinate; scale_out[nkp * 4] (may be NULL) = c.x, c.y, c.z, m (NaN where n < 3 or q is not finite);
 *  4 voxel per axis v = g < 0 ? floorf(g) + 32 : ceilf(g) + 31, clamped to 0..63; every point sets the cells v + {-1,0,1}^3 that lie in
 *    the 64^3 bit set;
 *  5 attempt t = 0, 1, 2, ... draws i_k = mulhi32(h(seed, 3t + k), n), k = 0, 1, 2 (mulhi32: the upper half of the 64-bit product) with
 *      h(s, x): v = x * 0x9E3779B1 + s;  v ^= v >> 16;  v *= 0x7FEB352D;  v ^= v >> 15;  v *= 0x846CA68B;  v ^= v >> 16   (mod 2^32)
 *    p1, p2, p3 = g[i_0], g[i_1], g[i_2]; v21 = p2 - p1, v31 = p3 - p1, v23 = p2 - p3; a, b, c = |v21|, |v31|, |v23|;
 *    s = ((a + b) + c) * 0.5f; H = ((s*(s-a))*(s-b))*(s-c). Rejected: two equal indices; H <= 0.001f or not finite; one of
 *    th = (int)floorf(acosf(|u . w|) / (float)(pi/2) * 63.0f + 0.5f) outside 0..63 or NaN, for (u, w) = (v21, v31), (v23, v31), (v23, v21)
 *    each divided by its length. The samples are the first n_samples accepted attempts in order of t; fewer than n_samples among the
 *    attempts t < 8 * n_samples: NaN row;
 *  6 per sample the lines p1 -> p2 (length a), p1 -> p3 (b), p2 -> p3 (c) are walked from voxel to voxel by PCL's lci: a 3-D Bresenham
 *    line whose driving axis is the longest (ties x, then y, then z), L its length in cells; the cells at steps 0 .. max(L, 1) - 1 are
 *    visited (as PCL's loop, the walk stops one step short of the end voxel); visited = max(L, 1), inside = the occupied ones. Line
 *    class: IN if inside >= visited - 1, else OUT if inside <= 7, else MIXED with ratio = (float)inside / (float)visited, which adds to
 *    the ratio block at floorf(ratio * 63.0f + 0.5f). Triangle class over the three lines: OUT if sum inside <= 21, else IN if
 *    sum visited - sum inside < 4, else MIXED. A3: bins th1, th2, th3 of the triangle's class, a third each;
 *  7 after all samples, D3 = sqrtf(sqrtf(H)) goes to bin floorf(D3 / max D3 * 63.0f + 0.5f) of the triangle's class, every line's length d
 *    to bin floorf(d / max d * 63.0f + 0.5f) of the D2 block of the line's class, the maxima over all samples;
 *  8 ten blocks of 64 bins: A3 in, out, mixed (weight 0.5 each), D3 in (0.5), out (0.5), mixed (1), D2 in (0.5), out (2), mixed (2), ratio
 *    (1). In sixths every deposit is an integer: A3 1, D3 3 / 3 / 6, D2 3 / 12 / 12, ratio 6; N_i -> bin_counts_out[nkp * 640] (may be
 *    NULL), row[i] = (float)N_i / (float)sum N.
 * Integer counts, float maxima and fixed-point sums only: two calls, any grid cell size and any staging capacity give the same bytes, and
 * two identical neighbourhoods anywhere in a batch get identical rows. The host layer calls with ISMHIP_ESF_SAMPLES and ISMHIP_ESF_SEED.
 * Refused with ISMHIP_ERR_INVALID ("esf_local: bad argument"): a missing array, a radius that is not positive and finite, n_samples
 * outside 1..65536. Timer "esf_local". */
#define ISMHIP_ESF_DIM 640          /* ismhip_esf_local: 10 blocks of 64 bins */
#define ISMHIP_ESF_SAMPLES 20000    /* PCL's sample_size */
#define ISMHIP_ESF_SEED 0x45534631u /* "ESF1" */
int  ismhip_esf_local(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                      const float* kpx, const float* kpy, const float* kpz, float radius, int n_samples, uint32_t seed,
                      float* desc_out, uint32_t* neighbour_count_out, uint32_t* bin_counts_out, float* scale_out);
/* The dense first half of FeaturesRIFT::iComputeDescriptors (features/features_rift.cpp:29-96): PointCloudXYZRGBtoXYZI (:47-51), then PCL 1.10
 * IntensityGradientEstimation (:53-62) over the Radius ball of every cloud point. This library's definition (deviations D1, D2):
 *  - intensity I = (0.299f*R + 0.587f*G) + 0.114f*B in float, unfused, from the 8-bit channels of the cloud's 0x00RRGGBB colours;
 *  - ball of point i: the finite cloud points with d2 < (float)((double)radius * radius), d2 = (dx*dx + dy*dy) + dz*dz in float, i itself
 *    included; count_out[n_pts] (may be NULL) = cp, 0 for a point that is not finite;
 *  - cp < 3 or a normal that is not finite: (NaN, NaN, NaN); else A = sum (p_j - c)(p_j - c)^T, b = sum (p_j - c)(I_j - m), c and m the
 *    ball's means, from the moments about the query (positions and intensities both), differences and products in double, every term
 *    rounded to a fixed quantum and added as a 64-bit integer: the sums do not depend on the order (D1);
 *  - x = pseudo-inverse of A over the eigenvalues above 1e-12 of the largest (eigen3.h; x = 0 when that is not positive) times b (D2);
 *  - g = x - n (n . x) with the point's normal n, in double; grad_out[n_pts * 3] floats in the cloud's original point order.
 * Two calls and any grid cell size give the same bits. Refused with ISMHIP_ERR_INVALID: a radius that is not positive and finite
 * ("intensity_gradients: bad argument"), a cloud made without rgba ("intensity_gradients: colour arrays missing"), grad_out NULL with
 * points to describe. Timer "intensity_gradients". Asynchronous. */
int  ismhip_intensity_gradients(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, float* grad_out, uint32_t* count_out);
/* The second half (features/features_rift.cpp:66-78 -> PCL 1.10 RIFTEstimation::computeRIFT): desc_out[nkp * n_distance_bins *
 * n_gradient_bins], the reference's 8 x 16 (ISMHIP_RIFT_DISTANCE_BINS, ISMHIP_RIFT_GRADIENT_BINS, 128 floats). grad: the array
 * ismhip_intensity_gradients wrote for this cloud. Per keypoint p0 (the keypoint itself, D5) and ball point j (same ball rule), in float:
 * u = p_j - p0, dist = sqrtf(d2), mag = |g_j|, angle = atan2(|g_j x u|, g_j . u) (D3; 0 when both vanish), d = nd * dist / (radius +
 * FLT_EPSILON), a = ng * angle / ((float)M_PI + FLT_EPSILON); the deposit (1 - |d - d_idx|)(1 - |a - g_idx|) * mag goes to bin
 * g_idx mod ng * nd + d_idx for the d_idx in [0, nd - 1] and the g_idx within 1 of d and a. Deposits enter 64-bit integer bins scaled per
 * object by a power of two above its largest |g|; the row is divided by its L2 norm (double), an all-zero row stays zero. An empty ball,
 * a ball point whose gradient is not finite and a keypoint that is not finite give a row that is NaN AS A WHOLE (D4);
 * neighbour_count_out[nkp] (may be NULL) = the ball's points, 0 for a ball that misses the object. Two calls and any grid cell size give
 * the same bits. Refused with ISMHIP_ERR_INVALID: a radius that is not positive and finite, a bin count below 1 ("rift: bad argument"),
 * a cloud made without rgba ("rift: colour arrays missing"), a missing array with keypoints to describe, offsets that are not monotone;
 * with ISMHIP_ERR_UNSUPPORTED: n_distance_bins * n_gradient_bins > 256. Timer "rift". */
int  ismhip_rift(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                 const float* kpx, const float* kpy, const float* kpz, float radius, int n_distance_bins, int n_gradient_bins,
                 const float* grad, float* desc_out, uint32_t* neighbour_count_out);
/* ---- CGF (features/features_cgf.cpp -> third_party/cgf/cgf.cpp:64-165 and third_party/cgf/embedding.py:103-108) ----------
 * The PCA normal of cgf.cpp:87-94 at every KEYPOINT over the `radius` ball of the cloud: the arithmetic of ismhip_estimate_normals_pca with
 * orientation 0 (FP64 moments about the query, eigen3.h, at least 3 ball points, flipped towards (0,0,0)); NaN for fewer than 3 points, for a
 * keypoint that is not finite and for a ball that misses the object. Writes three arrays of nkp floats. Refused with ISMHIP_ERR_INVALID
 * ("keypoint_normals_pca: bad argument"): a missing array, a radius that is not positive and finite. Timer "keypoint_normals_pca". */
int  ismhip_keypoint_normals_pca(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                                 const float* kpx, const float* kpy, const float* kpz, float radius,
                                 float* knx_out, float* kny_out, float* knz_out);
/* The raw spherical histogram of cgf.cpp:98-161: desc_out[nkp * ISMHIP_CGF_RAW_DIM], bin = bin_r + 17 bin_theta + 187 bin_phi.
 *  - lrf9: the frames of ismhip_shot_lrf at radius_lrf (the caller's 0.75 R); a frame with a NaN in its x axis becomes the identity; else,
 *    with n = (knx, kny, knz)[k] (ismhip_keypoint_normals_pca at 0.1 R), all three axes are negated when (z.x n.x + z.y n.y) + z.z n.z < 0
 *    in float (a NaN normal negates nothing);
 *  - ball: the finite cloud points with d2 < (float)((double)radius * radius), d2 as in every sweep of this library. THE SKIP RULE (cgf.cpp's
 *    loop starts at j = 1 of a distance-sorted list): the ball point with the smallest d2, ties to the lowest original index, is left out
 *    whether or not it coincides with the keypoint; so is every point whose (double)d2 > 1e-15 is false;
 *  - per remaining point: v = p - k in float; x, y, z = (v.x a.x + v.y a.y) + v.z a.z in unfused float against the three axes, widened to
 *    double; r = sqrt(x x + y y + z z), theta = acos(z / r) * 57.29578, phi = atan2(y, x) * 57.29578 (PCL's rad2deg);
 *    bin_r = (int)(16 (ln r - ln rmin) / ln(radius / rmin) + 1) clamped to [0, 16], bin_theta = (int)(11 theta / 180) at most 10,
 *    bin_phi = (int)(12 (phi + 180) / 360) at most 11; an angle that is NaN goes to bin 0;
 *  - row = (float)((double)count / (double)sum); sum == 0 (an empty ball, a ball that misses the object): a row of zeros, as in the
 *    reference. A keypoint that is not finite gives a row that is NaN as a whole. neighbour_count_out[nkp] (may be NULL) = sum.
 * radius and rmin arrive as doubles already rounded by the caller (the reference passes them through std::to_string). Integer counts only:
 * two calls and any grid cell size give the same bytes. Refused with ISMHIP_ERR_INVALID ("cgf_raw: bad argument"): a missing array, radius
 * or rmin not positive and finite, rmin >= radius. Timer "cgf_raw". */
#define ISMHIP_CGF_RADIAL_BINS 17
#define ISMHIP_CGF_POLAR_BINS 11
#define ISMHIP_CGF_AZIMUTH_BINS 12
#define ISMHIP_CGF_RAW_DIM 2244     /* 17 * 11 * 12 */
int  ismhip_cgf_raw(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                    const float* kpx, const float* kpy, const float* kpz, const float* lrf9,
                    const float* knx, const float* kny, const float* knz, double radius, double rmin,
                    float* desc_out, uint32_t* neighbour_count_out);
/* A small perceptron on the exact FP32 matrix cores (mlp.hip): n_layers <= ISMHIP_MLP_MAX_LAYERS layers y = act(x W + b), W[in][out]
 * row-major (TensorFlow's layout), act = ReLU (relu[l] != 0) or the identity; in[0] from 1 to 4096, every out from 1 to 512, in[l] =
 * out[l - 1]. W, b: host arrays, copied. forward maps x[n_rows * in[0]] to y[n_rows * out[last]] (device floats, row-major); odd widths and
 * row counts are padded inside the call. A row's result does not depend on the other rows of the call. Every sum is an FP32 fma chain in a
 * fixed order; bias and ReLU in float; a NaN stays NaN. Refused with ISMHIP_ERR_INVALID ("mlp_create: ..."). Timer "mlp_forward". */
#define ISMHIP_MLP_MAX_LAYERS 8
#define ISMHIP_MLP_MAX_IN 4096
#define ISMHIP_MLP_MAX_OUT 512
typedef struct ismhip_mlp ismhip_mlp;
int  ismhip_mlp_create(ismhip_ctx* ctx, int n_layers, const int* in, const int* out, const int* relu,
                       const float* const* W_h, const float* const* b_h, ismhip_mlp** mlp_out);
int  ismhip_mlp_destroy(ismhip_mlp* mlp);
int  ismhip_mlp_in(const ismhip_mlp* mlp);     /* in[0] */
int  ismhip_mlp_out(const ismhip_mlp* mlp);    /* out[last] */
int  ismhip_mlp_forward(ismhip_ctx* ctx, const ismhip_mlp* mlp, const float* x, size_t n_rows, float* y);
/* The weights container ".cgfw" (little endian): char magic[4] = "CGFW", uint32 version = 1, uint32 n_layers; per layer uint32 in, uint32
 * out, uint32 activation (1 ReLU, 0 identity), float32 W[in][out], float32 b[out]. No device is touched. expect_in > 0: the first layer's
 * `in` must equal it. Refusals (ISMHIP_ERR_INVALID, the reason in err[err_len], each with its name): "cannot open", "wrong magic",
 * "unsupported version", "layer count", "truncated file", "width out of range", "inconsistent widths", "first layer width", "unknown
 * activation", "non-finite weight", "trailing bytes". */
typedef struct ismhip_cgfw ismhip_cgfw;
int  ismhip_cgfw_open(const char* path, int expect_in, ismhip_cgfw** out, char* err, int err_len);
int  ismhip_cgfw_close(ismhip_cgfw* w);
int  ismhip_cgfw_layers(const ismhip_cgfw* w);
int  ismhip_cgfw_layer(const ismhip_cgfw* w, int layer, int* in, int* out, int* relu, const float** W, const float** b);
int  ismhip_mlp_from_cgfw(ismhip_ctx* ctx, const ismhip_cgfw* w, ismhip_mlp** mlp_out);
/* ISMFeature::centerDist (features_shot.cpp:77): |keypoint - centroid(object)| -> out[nkp] */
int  ismhip_center_dist(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h,
                        const float* kpx, const float* kpy, const float* kpz, float* out);

/* ---- global (region) descriptors: the global features of Voting.UseGlobalFeatures. A REGION is (object index, selection centre,
 *      selection radius): region_obj[n_regions] (device int32), region_center[n_regions*3], region_radius[n_regions] (device float).
 *      A NEGATIVE selection radius selects the object's finite points as a whole; otherwise those with d2 < (float)((double)radius *
 *      radius) to the centre, d2 the unfused float (dx*dx + dy*dy) + dz*dz (the rule of every ball sweep of this library). Several
 *      regions may name the same object, in any order; a region whose object index is outside [0, n_obj) selects nothing.
 *      Per region (all outputs device, all written): n_sel_out[n_regions] the number of selected points; centroid_out[n_regions*3] their
 *      centroid (pcl::compute3DCentroid: double sums, one division, cast to float); radius_out[n_regions] the largest distance from that
 *      centroid to a selected point (Features::getCloudRadius, features.cpp:128-151, the arithmetic of ismhip_cloud_radii); lrf9_out
 *      [n_regions*9] the SHOT frame (ismhip_shot_lrf's arithmetic and layout) of ONE keypoint, that centroid, with that radius over the
 *      selected points -- a sign tie goes to the five median neighbours by (distance, original index) whatever the region's size;
 *      desc_out one row per region. For a whole-object region centroid and radius are bit-equal to ismhip_cloud_centroids /
 *      ismhip_cloud_radii. n_sel = 0: NaN centroid, radius 0, NaN frame, NaN row. Fewer than five frame neighbours (selected points
 *      inside the ball (centroid, radius) other than the centroid itself): NaN frame and NaN row. One workgroup per region, no float
 *      atomics: every output is bitwise reproducible. Asynchronous.
 *
 * ismhip_global_short_shot: FeaturesSHORTSHOTGlobal::compute_descriptor (features/features_short_shot_global.cpp:94-165) on the grid of
 * configureSphericalGrid (:168-249; the caller maps ShortShotDims / ShortShotBinType to the three bin counts). desc_out[n_regions * D],
 * D = r_bins * e_bins * a_bins. Every selected point with d2 < (float)((double)R * R) to the centroid (R = radius_out) and (double)d2 >
 * 1e-15: v = p - centroid in float; x_l = (double)((v.x*X.x + v.y*X.y) + v.z*X.z) in float, unfused, in this order (as ismhip_short_shot),
 * likewise y_l, z_l; then in double r = sqrt((x_l^2 + y_l^2) + z_l^2), theta = acos(z_l / r) * 57.29578, phi = atan2(y_l, x_l) * 57.29578;
 * bin_r = int((r_bins * r) / (double)R), or with log_radius int(((r_bins - 1) * (log(r) - log(min_radius))) / log((double)R / min_radius) + 1)
 * -- min_radius is the parameter ShortShotMinRadius ITSELF, an absolute length, and no point is skipped for lying below it;
 * bin_theta = int((e_bins * theta) / 180), bin_phi = int((a_bins * (phi + 180)) / 360); r clamped to [0, r_bins - 1], theta and phi from
 * above only; +1 at bin_r + bin_theta * r_bins + bin_phi * r_bins * e_bins: NO interpolation (this is not ismhip_short_shot's arithmetic).
 * int() of a NaN is taken as INT_MIN (x86-64): bin 0 for r, no count for an angle. The row is count / sqrt(sum count^2) in double, cast
 * to float; no counted point gives 0 / 0, a NaN row. count_out: device [n_regions * D] or NULL, the integer histogram (0 for a NaN frame).
 * Refused as ismhip_short_shot refuses: a bin count < 1 (ISMHIP_ERR_INVALID), more than ISMHIP_SHORT_SHOT_MAX_DIM bins
 * (ISMHIP_ERR_UNSUPPORTED), log_radius without a finite min_radius > 0 (ISMHIP_ERR_INVALID). Timer "global_short_shot". */
int  ismhip_global_short_shot(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                              const float* region_radius, double min_radius, int log_radius, int r_bins, int e_bins, int a_bins,
                              uint32_t* n_sel_out, float* centroid_out, float* radius_out, float* lrf9_out, float* desc_out, uint32_t* count_out);
/* ismhip_global_shot352: FeaturesSHOTGlobal::iComputeDescriptors (features/features_shot_global.cpp:27-99): SHOT-352 at the centroid with
 * descriptor radius and frame radius both R, over the selected points -- the per-neighbour arithmetic, the 2^-28 fixed-point histogram
 * and the normalisation of ismhip_shot352 (the same functions); fewer than five descriptor neighbours: NaN row. desc_out[n_regions*352].
 * Timer "global_shot352". */
int  ismhip_global_shot352(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                           const float* region_radius, uint32_t* n_sel_out, float* centroid_out, float* radius_out, float* lrf9_out, float* desc_out);
/* ismhip_global_vfh: FeaturesVFH::iComputeDescriptors (features/features_vfh.cpp:27-70): pcl::VFHEstimation over the region with
 * setNormalizeBins(true), setNormalizeDistance(false), the size component off and the viewpoint the caller's (the reference leaves PCL's
 * (0, 0, 0)). PCL is external: this is the library's own statement of PCL 1.10 vfh.hpp (DESIGN.md section 4.17 names the deviations).
 * Region, n_sel, centroid c and radius are those of the two entries above, bit for bit on the same regions; there is NO frame.
 * normal_centroid_out[n_regions*3]: nc = (float)(sum / m) per component over the m selected points whose normal is finite, double sums in
 * a fixed order, NOT normalised. m < 2: NaN row. View direction d = viewpoint - c in float, divided by its float norm (a zero norm
 * leaves d = 0). desc_out[n_regions*308] from INTEGER counts (count_out: device [n_regions*308] or NULL):
 *   bins 0..179, four blocks of 45: every selected point p with a finite normal n is evaluated with pcl::computePairFeatures(c, nc, p, n)
 *     in float (the arithmetic of ismhip_fpfh33's exact path); a pair it rejects (f4 == 0 or a zero cross product) deposits nothing here.
 *     From the float features, in double: b1 = floor(45 * ((f1 + M_PI) * dpi)), dpi = (double)(1.0f / (2.0f * (float)M_PI));
 *     b2 = floor(45 * ((f2 + 1.0) * 0.5)); b3 likewise from f3; b4 = floor((double)(f4 * 100.0f) + 0.5), f4 = |p - c| in float (hundredths
 *     of a unit, not normalised); each clamped to [0, 44]; a NaN feature deposits nothing.
 *   bins 180..307, the viewpoint block: every selected point with a finite normal (its pair rejected or not):
 *     floor((((double)(float)dot(n, d) + 1.0) * 0.5) * 128.0) clamped to [0, 127].
 *   row: blocks f1..f3 (float)((double)count * (double)incr), incr = 100.0f / (float)(m - 1) in float; block f4 all zeros unless
 *     fill_size_component (then as f1..f3; its counts are reported either way); viewpoint block (float)((double)count *
 *     (double)(float)(100.0 / (double)m)). One product per bin: order-free, the same bits on every call.
 * n_sel = 0: NaN centroid, radius 0, NaN normal centroid, NaN row. viewpoint: HOST float[3]; a non-finite one is ISMHIP_ERR_INVALID.
 * Otherwise checked as the two entries above. Timer "global_vfh". */
int  ismhip_global_vfh(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                       const float* region_radius, const float viewpoint[3], int fill_size_component, uint32_t* n_sel_out, float* centroid_out,
                       float* radius_out, float* normal_centroid_out, float* desc_out, uint32_t* count_out);
/* ismhip_global_gasd: FeaturesGASD::iComputeDescriptors (features/features_gasd.cpp:25-91): pcl::GASDColorEstimation with its default
 * constructor (shape half-grid 3, colour half-grid 2, 12 hue bins, NO interpolation on either grid) over the region, the view direction
 * the caller's (PCL's default is (0, 0, 1)). PCL is external: this is the library's own statement of PCL 1.10 gasd.hpp (DESIGN.md
 * section 4.22 names the deviations); parity with PCL is not pinned. Region, n_sel, centroid c and radius are those of the three entries
 * above, bit for bit on the same regions. n_sel = 0: NaN centroid, radius 0, NaN frame, NaN row. n_sel < 2: NaN frame and NaN row
 * (PCL's increment 100 / (n - 1) is infinite there). Otherwise, over the selected points p, d = p - c per component in float:
 *   covariance: the six products of d in double, summed in a fixed order, NOT normalised (pcl::computeCovarianceMatrix).
 *   frame (frame9_out[n_regions*9], rows x, y, z; double eigenvectors cast to float): z = eigenvector of the smallest eigenvalue,
 *     negated if z . view_direction > 0; x = eigenvector of the largest; the sign of x (PCL leaves it to its solver) is defined here:
 *     with t = (x.x*d.x + x.y*d.y) + x.z*d.z in float, unfused, x is negated if more selected points have t < 0 than t > 0; on equal
 *     counts x is signed so that its component of largest magnitude (lowest index on a tie) is positive; y = z cross x.
 *   max_coord_out[n_regions]: the float maximum over the points of |t.x|, |t.y|, |t.z|, t = (x . d, y . d, z . d) each as above (PCL
 *     rotates p and c separately and subtracts); NaN with a NaN frame. max_coord = 0 or not finite: NaN row, the frame stays.
 *   bins 0..215, the shape block: per axis coord = (t / max_coord) * 3.0f + 3.0f in float, b = floor(coord); a b outside 0..5 or a NaN on
 *     any axis deposits nothing (PCL's padding cell, which its copy to the output drops: the point that attains +max_coord is lost);
 *     otherwise +1 at (bx*6 + by)*6 + bz.
 *   bins 216..983, the colour block, only with with_color: cells as above with * 2.0f + 2.0f and 0..3; the hue of the point's 8-bit
 *     (r, g, b) -- the caller's rgba at the original index -- as GASDColorEstimation::computeFeature writes it: diff_inv = 1.f /
 *     (float)(max - min); not finite: hue 0; max == r: 60.f * ((float)(g - b) * diff_inv); else max == g: 60.f * (2.f + (float)(b - r) *
 *     diff_inv); else 60.f * (4.f + (float)(r - g) * diff_inv); hue < 0: + 360.f; hb = floor((hue / 360.f) * 12.f) in float, unfused;
 *     hb outside 0..11 deposits nothing; otherwise +1 at 216 + ((cx*4 + cy)*4 + cz)*12 + hb.
 *   row: (float)((double)count * (double)incr), incr = 100.0f / (float)(n_sel - 1): one product per bin, order-free, the same bits on
 *     every call (PCL adds incr once per deposit in float). desc_out and count_out (device uint32 or NULL; 0 for a NaN row) have row
 *     length ISMHIP_GASD_DIM with with_color, else ISMHIP_GASD_SHAPE_DIM: the 216 shape bins followed by 296 zeros.
 * view_direction: HOST float[3]; a non-finite or zero one is ISMHIP_ERR_INVALID, as is with_color on a cloud made without rgba
 * ("global_gasd: colour arrays missing"). Otherwise checked as the entries above. Timer "global_gasd". */
int  ismhip_global_gasd(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                        const float* region_radius, const float view_direction[3], int with_color, uint32_t* n_sel_out, float* centroid_out,
                        float* radius_out, float* frame9_out, float* max_coord_out, float* desc_out, uint32_t* count_out);
/* ismhip_global_cvfh: FeaturesCVFH::iComputeDescriptors (features/features_cvfh.cpp) -> pcl::CVFHEstimation, the clustered viewpoint
 * feature histogram: the one region descriptor with MORE THAN ONE ROW per region, one per smooth cluster. PCL is external: this is the
 * library's own statement of PCL 1.10 cvfh.hpp / vfh.hpp (DESIGN.md section 4.25 names the deviations); parity with PCL is not pinned.
 * Region, n_sel, centroid and radius are those of the entries above, bit for bit on the same regions. "Selected" below: a finite point of
 * the region. features_cvfh.cpp has no parameters (angle 10 degrees, curvature threshold 1.0, which keeps every point; PCL's defaults
 * otherwise: tolerance and normal radius 0.015, 50 points, viewpoint (0, 0, 0)); here they are arguments.
 *   a. clustering normals. normal_radius > 0 and n_sel >= min_points: for every selected point q the PCA normal over the SELECTED points p
 *      with d2(p, q) < (float)((double)normal_radius * normal_radius), q included: v = (double)p - (double)q per component; the three
 *      components and six products, each rounded to the integer grids of csrc/moments.h (2^e2 the power of two above the squared radius,
 *      2^e1 its root; 48 bits, fewer for objects beyond 2^14 points) and added as integers: ORDER FREE. Covariance E[vv^T] - E[v]E[v]^T with
 *      inv = 1.0 / count, the Jacobi solver of ismhip_estimate_normals_pca; the smallest eigenvalue's vector cast to float and negated when
 *      ((vp - q) . n) < 0 in float (method 0 of ismhip_estimate_normals_pca, with the caller's viewpoint). Fewer than three such points: NaN.
 *      Otherwise (normal_radius <= 0, or n_sel < min_points) the clustering normals are the cloud's own.
 *   b. links. Two selected points i != j link iff d2(i, j) < (float)((double)cluster_tolerance * cluster_tolerance), both clustering normals
 *      are finite, and c > cos(angle_threshold), c = ((double)n1.x*n2.x + (double)n1.y*n2.y) + (double)n1.z*n2.z clamped to [-1, 1]
 *      (float components converted to double; cos() once on the host in double). Comparing cosines is acos(c) < angle_threshold without the
 *      acos; the clamp keeps two equal normals whose product rounds past 1 linked (PCL's unclamped acos gives NaN there). Clusters are the
 *      CONNECTED COMPONENTS of that symmetric relation (PCL's region growing yields the same sets: the predicate is pairwise). A component
 *      of at least min_points points is kept; kept clusters are ordered by their smallest ORIGINAL point index (PCL's seed order).
 *      label_out (device uint32 [n_regions * S], S = the cloud's largest object, or NULL): per region and original point index the smallest
 *      original index of the point's component (a selected point with a NaN normal is a component of its own); 0xffffffff for a point that
 *      is not selected, not finite or past the object's end.
 *   c. per kept cluster: centroid = the mean of its points, normal = the mean of its clustering normals, normalised: coordinates and
 *      components rounded to integer grids (coordinates: 2^e above twice the largest |region centroid| component plus the region radius;
 *      normal components: below 4, a longer normal is left out) and added as integers, order free; mean = (double)sum * q / count, cast to
 *      float; the normal divided by its double length first. No cluster kept and n_sel > 0: ONE row (the fallback) from the mean of ALL
 *      selected points and the mean of their FINITE clustering normals (non-finite ones are left out of sum and count), root 0xffffffff,
 *      size n_sel.
 *   d. one row of 308 per kept cluster: ismhip_global_vfh's deposits over ALL selected points of the region with a finite CLOUD normal,
 *      evaluated against the row's centroid and normal, view direction (viewpoint - row centroid) normalised in float, with the distance
 *      block b4 = floor((45.0 * (double)f4) / (double)dmax) clamped to [0, 44], dmax the largest float f4 = |p - row centroid| over those
 *      points (dmax = 0: no deposit). count_out: the integer counts. desc = (float)count / 47278.0f, one division per bin (the reference's
 *      normalizeDescriptors, features/features.cpp:282-297, divides the raw counts by the sum of the bin INDICES).
 *      Fewer than two points with a finite cloud normal, or a row centroid or row normal that is not finite: a NaN row with zero counts
 *      (k_vfh's rule; the host drops a NaN row).
 * Outputs per region: n_sel_out, centroid_out, radius_out as above; n_clusters_out[n_regions] the TRUE number of rows, never clipped by
 * max_rows (0 iff n_sel = 0); rows k < min(n_clusters, max_rows) at slot region * max_rows + k: row_centroid_out[.*3], row_normal_out[.*3],
 * row_size_out[.] (points of the cluster), desc_out[.*308], count_out[.*308] (or NULL). The other slots: NaN, size 0, zero counts. A caller
 * that finds n_clusters > max_rows asks again with a larger capacity. viewpoint: HOST float[3], finite. cluster_tolerance > 0,
 * min_points >= 1, max_rows >= 1, 0 < angle_threshold < pi (the reference: 10.0 / 180.0 * M_PI), else ISMHIP_ERR_INVALID. Integer atomics
 * only: every output is the same bits on every call and for every grid cell size of the cloud. Asynchronous. Timers "global_cvfh" and,
 * inside it, "cvfh_normals", "cvfh_label", "cvfh_stats", "cvfh_rows". */
int  ismhip_global_cvfh(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                        const float* region_radius, const float viewpoint[3], float cluster_tolerance, float normal_radius, int min_points,
                        double angle_threshold, int max_rows, uint32_t* n_sel_out, float* centroid_out, float* radius_out,
                        uint32_t* n_clusters_out, float* row_centroid_out, float* row_normal_out, uint32_t* row_size_out, float* desc_out,
                        uint32_t* count_out, uint32_t* label_out);
/* Diagnostic: the hue bin of ismhip_global_gasd's colour block alone, one thread per colour. rgba: device [n] packed 0x00RRGGBB, bits
 * 24..31 ignored. out: device uint8 [n], the bin 0..11, or 255 where the rule deposits nothing. Asynchronous. Off every hot path. */
int  ismhip_gasd_hue_bins(ismhip_ctx* ctx, int n, const uint32_t* rgba, uint8_t* out);
/* ismhip_region_mvbb: the minimum-volume bounding box of a region, Utils::computeMVBB (utils/utils.cpp:242-293), which is
 * gdiam_approx_mvbb(points, n, 0.0) of libgdiam-1.3: stated here as this library's own arithmetic (DESIGN.md section 4.24 names the
 * deviations and pins the result against the real library's). The region and its finite points are those of the entries above;
 * n_sel_out likewise. A point is its three floats converted to double (utils.cpp:249-257), its INDEX the one inside its object.
 * Everything below is double, unfused, in the written order; dot(a, b) = (a0*b0 + a1*b1) + a2*b2; normalise(v): len = sqrt(dot(v, v)),
 * v / len per component unless len == 0; cross(a, b) = (a1*b2 - a2*b1, -(a0*b2 - a2*b0), a0*b1 - a1*b0). bound(axes): per axis k
 * lo_k / hi_k = the minimum / maximum over the points of dot(p, axis_k); volume = ((hi0 - lo0) * (hi1 - lo1)) * (hi2 - lo2).
 * base(u): gdiam_generate_orthonormal_base (gdiam.cpp:1226-1270) on normalise(u), its case list as written, giving (bx, by).
 *   A (gdiam.cpp:1138-1149, eps 0: exact). Over all pairs i < j: d2 = (dx*dx + dy*dy) + dz*dz of d = p_i - p_j; the pair of largest d2,
 *     ties to the lowest (i, j). d1 = normalise(p_i - p_j).
 *   B (:1151-1169). The same over the projected points p' = p - dot(p, d1) * d1 (per component). With v = p'_i - p'_j of that pair:
 *     q = v - dot(v, d1) * d1, len = sqrt(dot(q, q)); len < 1e-6 (collinear points): (d2, d3) = base(d1); else d2 = q / len,
 *     d3 = normalise(cross(d1, d2)).
 *   C (:1191-1200). best = bound(d1, d2, d3); if bound(identity) has a strictly smaller volume, best = that, with identity axes.
 *   D (gdiam_mvbb_optimize, :2245-2270), rounds r = 0 .. ISMHIP_MVBB_ROUNDS - 1: u = normalise(axis r % 3 of best), (bx, by) = base(u);
 *     every point (x, y) = (dot(p, bx), dot(p, by)). The convex hull of these, STRICT vertices only, counter-clockwise from the lowest
 *     (x, y): monotone chain over the points sorted by (x, y, index), a point that repeats the (x, y) of the one before it skipped,
 *     turn(o, a, b) = (a.x - o.x)*(b.y - o.y) - (a.y - o.y)*(b.x - o.x), a vertex popped while turn <= 0. (The kernel first drops
 *     points inside the polygon of the extremes in eight directions by a margin of 2^-40 M^2, M the larger extent in x and y: a
 *     thousand times the rounding of the test, so no hull vertex is lost.) For every hull edge from vertex a to its successor b:
 *     e = (b - a) / sqrt(ex*ex + ey*ey); over the hull's vertices s = x*e.x + y*e.y and t = y*e.x - x*e.y; area = (max s - min s) *
 *     (max t - min t). The edge of smallest area, ties to the lowest point index of its start vertex. (Equal to the reference's
 *     rotating calipers, :1977-2022, in exact arithmetic; not its tan / atan2 arithmetic.) A hull of one vertex: e = (1, 0).
 *     o1 = normalise((-e.y) * bx + e.x * by) across the edge, o2 = normalise(e.x * bx + e.y * by) along it (the order in which the
 *     reference lifts its rectangle, :2161-2192: it decides which axis a later round takes); cand = bound(u, o1, o2); best = cand if
 *     cand's volume < best's volume * (1 - 2^-36). (The reference asks for strictly smaller. A box that has converged is found again
 *     by later rounds, from either of its two flush hull edges, with a volume that differs in the last bits: there "strictly" is
 *     decided by rounding, in the reference too, and with it the axis order of every later round. An improvement below 1.5e-11 of
 *     the volume is declined instead.)
 *   Output (the reference's axis order, signs and handedness are accidents of its traversal): axes ordered by descending extent
 *     hi - lo, ties to the earlier axis; axes 1 and 2 negated (with their lo / hi) where their component of largest magnitude (lowest
 *     index on a tie) is negative; axis 3 = cross(axis 1, axis 2), its lo / hi negated and swapped if that reverses the old axis 3.
 *     axes9_out: rows = axes. size_out = hi - lo per axis. center_out (world) = (mid0*axis1 + mid1*axis2) + mid2*axis3 per component,
 *     mid = (lo + hi) * 0.5. volume_out (device double [n_regions] or NULL): best's volume. Float outputs are the doubles cast once.
 *   Degenerate: n_sel = 1 or all points coincident (the reference asserts): identity axes, zero size, centre the point, volume 0.
 *     n_sel = 0: NaN centre and axes, zero size, volume 0.
 * trace_out (device int32 [n_regions * ISMHIP_MVBB_TRACE] or NULL): [0, 1] the pair of A, [2, 3] of B, [4] C took the axis-aligned box,
 * [5] B found the points collinear, [6] degenerate, [7] a diagnostic that is no part of the definition: the most points the kernel's
 * pre-filter left in a round (above 768 they went through the work buffer); round r at [8 + 4 r]: taken, hull size, the chosen edge's two point indices.
 * Indices that do not exist are -1. One workgroup per region, a region of any size; no float atomics: the same bits on every call.
 * Checked as the entries above ("region_mvbb: bad argument"). Timer "region_mvbb". Asynchronous. */
#define ISMHIP_MVBB_ROUNDS 10
#define ISMHIP_MVBB_TRACE  48
int  ismhip_region_mvbb(ismhip_ctx* ctx, const ismhip_cloud* cloud, int n_regions, const int32_t* region_obj, const float* region_center,
                        const float* region_radius, uint32_t* n_sel_out, float* center_out /*[n*3], world*/, float* size_out /*[n*3]*/,
                        float* axes9_out /*[n*9], rows = axes*/, double* volume_out /*[n] or NULL*/, int32_t* trace_out /*[n*48] or NULL*/);

/* ---- keypoints (the step in front of the path): KeypointsVoxelGrid::iComputeKeypoints
 *      (keypoints/keypoints_voxel_grid.cpp:30-46) -> pcl::VoxelGrid<PointXYZRGB> with a cubic leaf. Per object the
 *      centroids (xyz, and rgb when rgba is given) of the occupied voxels in ascending voxel index, packed object
 *      after object into kx|ky|kz[|krgba] (device, `capacity` entries; the number of points always suffices);
 *      kp_offsets_h_out[n_obj+1] (host) receives the per-object ranges. Non-finite points are ignored. The call
 *      synchronises. */
int  ismhip_voxel_keypoints(ismhip_ctx* ctx, int n_obj, const uint32_t* pt_offsets_h,
                            const float* x, const float* y, const float* z, const uint32_t* rgba, float leaf,
                            uint32_t capacity, float* kx, float* ky, float* kz, uint32_t* krgba,
                            uint32_t* kp_offsets_h_out);

/* ---- ISS3D keypoints: KeypointsISS3D::iComputeKeypoints (keypoints/keypoints_iss3d.cpp:31-72) -> pcl::ISSKeypoint3D without border
 *      estimation. PCL is external; the arithmetic is this library's definition, restated from PCL 1.10 iss_3d.hpp (DESIGN.md section
 *      4.14). Per object, on the finite points of the cloud; every neighbourhood by the rule of ismhip_filter_radius (unfused float d2,
 *      STRICTLY below (float)((double)r * r), the query included). Results do not depend on the cell_size the cloud was created with,
 *      and are the same bits from run to run.
 * ismhip_iss3d_saliency (keypoints_iss3d.cpp:31-72): per point the scatter matrix C = sum d d^T, d = (double)p_j - (double)p_i over the
 * salient_radius ball (about the query, not divided by the count; all zero with fewer than min_neighbors neighbours), its eigenvalues
 * e1 >= e2 >= e3, and saliency = e3 when all three are finite, e3 >= 0, e2 / e1 < gamma21 and e3 / e2 < gamma32 (double compares, 0 / 0
 * fails), else 0. saliency_out: device double[n_pts] in original point order; eig_out: device double[n_pts * 3] (e1, e2, e3) or NULL;
 * count_out: device uint32[n_pts] neighbour counts or NULL. Non-finite points: all 0. Radii or gammas not > 0, min_neighbors < 0:
 * ISMHIP_ERR_INVALID. Timer "iss3d_saliency". Asynchronous. */
int  ismhip_iss3d_saliency(ismhip_ctx* ctx, const ismhip_cloud* cloud, float salient_radius, double gamma21, double gamma32, int min_neighbors,
                           double* saliency_out, double* eig_out, uint32_t* count_out);
/* ismhip_iss3d_keypoints (keypoints_iss3d.cpp:31-72): the saliency pass, then non-maximum suppression: a point with saliency > 0 is a
 * keypoint iff its non_max_radius ball holds at least min_neighbors points and none with a strictly larger saliency (equal ones both
 * survive). The keypoints are those points themselves, in ascending original index, packed object after object into kx|ky|kz (device,
 * `capacity` entries; the number of points always suffices), krgba (or NULL; the points' colours, 0 for a cloud without) and
 * src_index_out (or NULL; the point's index inside its object); kp_offsets_h_out[n_obj+1] (host) receives the per-object ranges. Empty
 * clouds and objects give empty ranges. Errors as ismhip_iss3d_saliency; capacity too small: ISMHIP_ERR_INVALID, as in
 * ismhip_voxel_keypoints. Timers "iss3d_saliency", "iss3d_nms". The call synchronises. */
int  ismhip_iss3d_keypoints(ismhip_ctx* ctx, const ismhip_cloud* cloud, float salient_radius, float non_max_radius, double gamma21, double gamma32,
                            int min_neighbors, uint32_t capacity, float* kx, float* ky, float* kz, uint32_t* krgba, uint32_t* src_index_out,
                            uint32_t* kp_offsets_h_out);

/* ---- VoxelGridCulling keypoints: KeypointsVoxelGridCulling (keypoints/keypoints_voxel_grid_culling.cpp): the voxel-grid keypoints of
 *      ismhip_voxel_keypoints at LeafSize, a geometry and a colour score per keypoint over its LeafSize ball of the search surface, and the
 *      better-scoring share kept (restated in tests/culling_ref.py). PCL is external: where it decides the
 *      arithmetic (normal curvature, principal curvatures) the definition is this library's own, written from knowledge of PCL 1.10; where
 *      the reference's own source decides it (kpq, colour score, combined score, thresholds, acceptance) the text is followed as written.
 *      Every ball: unfused float d2 STRICTLY below (float)((double)r * r), non-finite points are never neighbours. Every
 *      order-dependent sum is taken on an integer grid: the same bits for any cell_size, lane mapping and run, and an object's results do
 *      not depend on the other objects of the batch.
 * ismhip_principal_curvatures (:136-153 -> pcl::PrincipalCurvaturesEstimation, dense): per surface point i with normal n, over its
 * radius ball N (i included; a neighbour with a non-finite normal is skipped and not counted): v_j = n_j - n (n . n_j) in double from the
 * float normals, c their mean, S = sum (v_j - c)(v_j - c)^T (not divided), eigenvalues l0 <= l1 <= l2; pc1 = (float)(l2 / |N|), pc2 =
 * (float)(l1 / |N|). Normals need not be unit: the grid's scale comes from B (1 + B)^2 >= |v_j|^2, B the object's largest squared normal
 * length (a per-object reduction). pc1_out, pc2_out: device float[n_pts], count_out: device uint32[n_pts] (|N|) or NULL, original point
 * order; a point whose position or own normal is not finite: NaN, NaN, 0. radius not > 0: ISMHIP_ERR_INVALID. Timer "culling_pc".
 * Asynchronous. */
int  ismhip_principal_curvatures(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, float* pc1_out, float* pc2_out, uint32_t* count_out);
#define ISMHIP_CULLING_GEOMETRY_NONE 0
#define ISMHIP_CULLING_GEOMETRY_CURVATURE 1
#define ISMHIP_CULLING_GEOMETRY_KPQ 2
#define ISMHIP_CULLING_COLOR_NONE 0
#define ISMHIP_CULLING_COLOR_DISTANCE 1
/* ismhip_culling_scores (getScoresForKeypoints :280-329): per keypoint k (kx|ky|kz|krgba: device, kp_offsets_h[n_obj+1] host ranges,
 * object o's keypoints on object o of the cloud) one sweep over its `leaf` ball of n points fills
 *   geometry CURVATURE (:156-194 -> pcl::NormalEstimation): n < 3: NaN; else C = sum (p - m)(p - m)^T / n about the neighbours' mean m
 *     (sum d, sum d d^T about the keypoint on the grid, mean correction and eigen-solve in double), e3 its smallest eigenvalue:
 *     (float)|e3 / trace(C)|, 0 when the trace is 0;
 *   geometry KPQ (computeKPQ :441-471, as written): k1 = pc1, k2 = pc2 of the ball's points, K = k1 * k2 in float; max_k1, max_K from
 *     FLT_MIN and min_k2, min_K from FLT_MAX by the comparisons as written (a NaN never updates them); the score, in float, left to right:
 *     (1000.0f / num * num) * sum K + 100.0f * max_K + |100.0f * min_K| + 10 * max_k1 + |10 * min_k2|. sum K on the grid of the object's
 *     largest finite |K|, rounded once to float; NaN when any K is NaN. n = 0: NaN. pc1, pc2: device float[n_pts], original order;
 *   colour DISTANCE (computeColorScore :474-506): the keypoint's colour through RGB -> normalised CIELab is the reference; per ball point
 *     the distance (|dL| + (|da| + |db|) / 2) / 3 in double from the float differences, clamped to [0, 1], as float;
 *     (float)count(distance > max_similar_color_distance) / (float)n; n = 0: NaN. Needs a cloud with colours and krgba.
 * A method NONE leaves its score 0. geo_out, color_out: device float[n_keypoints]; count_out: device uint32 (n) or NULL. A keypoint that
 * is not finite has an empty ball. Errors: ISMHIP_ERR_INVALID. Timer "culling_scores". Asynchronous. */
int  ismhip_culling_scores(ismhip_ctx* ctx, const ismhip_cloud* cloud, const uint32_t* kp_offsets_h, const float* kx, const float* ky, const float* kz,
                           const uint32_t* krgba, float leaf, int geometry_method, int color_method, float max_similar_color_distance,
                           const float* pc1, const float* pc2, float* geo_out, float* color_out, uint32_t* count_out);
#define ISMHIP_CULLING_TYPE_CUTOFF 0
#define ISMHIP_CULLING_TYPE_THRESHOLD 1
#define ISMHIP_CULLING_REQUIRE_ONE 0
#define ISMHIP_CULLING_REQUIRE_BOTH 1
#define ISMHIP_CULLING_REQUIRE_COMBINED_LIST 2
/* ismhip_culling_select (:331-340, computeThresholds :346-432, :204-272): per object, on its score lists g = geo, c = color (device):
 *   combined = (g - gmin) / gmax + (c - cmin) / cmax in float (the division IS by the maximum), gmin / gmax the first smallest / largest
 *     of the object's non-NaN scores (none: +inf / -inf);
 *   a CUTOFF threshold of a method that is on: the element at index min((unsigned)(cutoff_ratio * (float)size), size - 1) of the list in
 *     ascending order, NaN behind +inf, -0 and +0 equal, ties by index; a THRESHOLD type: the given value; the combined threshold exists
 *     only when both methods are on and both types are CUTOFF. Every threshold that is not set stays FLT_MIN, as written;
 *   a test passes iff !(score < threshold) (a NaN score passes); both methods on: combine = REQUIRE_ONE: geo || colour, REQUIRE_BOTH:
 *     geo && colour, REQUIRE_COMBINED_LIST: the combined test; else geo && colour (a method that is off passes).
 * The accepted keypoints go, in their order and with their colours, to kx_out|ky_out|kz_out[|krgba_out] (device, `capacity` entries, must
 * not alias the inputs); kp_offsets_h_out[n_obj+1] (host) receives their ranges. keep_mask_out: device uint8[n_keypoints] or NULL;
 * combined_out: device float[n_keypoints] or NULL; thresholds_out: device float[3 * n_obj] (geometry, colour, combined) or NULL. An
 * object without keypoints gives an empty range (the reference's .at(0) throws there). Objects of any size. cutoff_ratio outside [0, 1),
 * more than `capacity` accepted (nothing written): ISMHIP_ERR_INVALID. Timer "culling_select". The call synchronises. */
int  ismhip_culling_select(ismhip_ctx* ctx, int n_obj, const uint32_t* kp_offsets_h, const float* geo, const float* color, int geometry_on, int color_on,
                           int geometry_type, int color_type, float geometry_threshold, float color_threshold, float cutoff_ratio, int combine,
                           const float* kx, const float* ky, const float* kz, const uint32_t* krgba, uint32_t capacity, float* kx_out, float* ky_out,
                           float* kz_out, uint32_t* krgba_out, uint8_t* keep_mask_out, float* combined_out, float* thresholds_out,
                           uint32_t* kp_offsets_h_out);

/* ---- SIFT3D keypoints: KeypointsSIFT3D::iComputeKeypoints (keypoints/keypoints_sift3d.cpp:24-86) -> pcl::SIFTKeypoint on an XYZI cloud
 *      whose intensity is the normal's curvature, setScales(Radius, 4, 3), setMinimumContrast(0). PCL is external; the arithmetic is this
 *      library's definition, restated from PCL 1.10 sift_keypoint.hpp (tests/sift3d_ref.py). Per object, on finite
 *      points only; every squared distance is the unfused float (dx*dx + dy*dy) + dz*dz. Every order-dependent sum is taken on an integer
 *      grid: the same bits for any cell_size, lane mapping and run.
 * ismhip_normal_curvature: dense, per surface point the CURVATURE geometry score of ismhip_culling_scores with that point as the keypoint
 * and `radius` as the leaf (the same device function): (float)|l0 / trace| over its radius ball, NaN with fewer than 3 ball points.
 * curv_out: device float[n_pts], count_out: device uint32[n_pts] (ball points) or NULL, original point order; a point that is not finite:
 * NaN, 0. radius not > 0: ISMHIP_ERR_INVALID. Timer "normal_curvature". Asynchronous. */
int  ismhip_normal_curvature(ismhip_ctx* ctx, const ismhip_cloud* cloud, float radius, float* curv_out, uint32_t* count_out);
/* ismhip_voxel_downsample_xyzi: one octave's downsampling. Positions exactly those of ismhip_voxel_keypoints on the same input (occupied
 * voxels in ascending voxel index, the 2^-40 fixed-point centroid); ki the mean of the voxel's intensities, summed on an integer grid of
 * its own: round(I * s), s the power of two with s * 2^e = 2^40, 2^e the power of two above the object's largest finite |I|, and
 * ki = (float)((double)sum / s) / (float)count. A point whose position or intensity is not finite is left out. x, y, z, intensity: device
 * float[n_pts]; kx|ky|kz|ki: device, `capacity` entries (the number of points always suffices); kp_offsets_h_out[n_obj+1] (host).
 * Errors as ismhip_voxel_keypoints. Timer "voxel_downsample_xyzi". The call synchronises. */
int  ismhip_voxel_downsample_xyzi(ismhip_ctx* ctx, int n_obj, const uint32_t* pt_offsets_h, const float* x, const float* y, const float* z,
                                  const float* intensity, float leaf, uint32_t capacity, float* kx, float* ky, float* kz, float* ki,
                                  uint32_t* kp_offsets_h_out);
/* ismhip_sift3d_scale_space: the difference-of-Gaussians columns of one octave. scales: host float[n_scales] (the caller's
 * base_scale * powf(2.0f, (i - 1.0f) / nr_scales)), 3 <= n_scales <= 16 else ISMHIP_ERR_INVALID, every scale > 0 and finite.
 * intensity: device float[n_pts], the cloud's original point order. Per point p and scale i, in float: s2 = scales[i] * scales[i],
 * over the cloud's points q with d2 <= 9.0f * s2 (p included, so the denominator is never 0): w = expf((-0.5f * d2) / s2),
 * response_i = (float)(sum (w * I_q) / sum w), both sums on integer grids (terms rounded to 2^(e - bits), 2^e the power of two above the
 * object's largest finite |I| for the numerator and 2 for the denominator, bits = 48 for objects below 2^14 points, one fewer per
 * doubling), the quotient in double; dog[p][i - 1] = response_i - response_{i-1} in float. A neighbour whose intensity is not finite is
 * skipped. dog_out: device float[n_pts * (n_scales - 1)], count_out: device uint32[n_pts] (points within the largest scale's bound) or
 * NULL; a point whose position or intensity is not finite: NaN row, count 0. One sweep of the 3 * scales[n_scales - 1] ball serves all
 * scales. Timer "sift3d_scale_space". Asynchronous. */
int  ismhip_sift3d_scale_space(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* intensity, const float* scales_h, int n_scales,
                               float* dog_out, uint32_t* count_out);
/* ismhip_sift3d_extrema: per point p its k nearest points of its object, itself included, ordered by (d2, index inside the object)
 * ascending -- ties go to the lowest index --, an object of fewer than k finite points uses all of them. For each column c = 1 ..
 * n_cols - 2 with fabsf(v) >= min_contrast, v = dog[p][c] (a NaN never passes): p is a MAXIMUM iff v > dog[q][c'] for every neighbour
 * q != p and c' in {c-1, c, c+1}, and v > dog[p][c-1], v > dog[p][c+1]; a MINIMUM with < throughout. The comparisons are STRICT: a
 * plateau yields neither (a decision of this library). dog: device float[n_pts * n_cols], 3 <= n_cols <= 15; flags_out: device
 * uint8[n_pts * n_cols]: 0 none, 1 minimum, 2 maximum, the border columns always 0; nn_idx_out: device int32[n_pts * k] or NULL, the
 * neighbours' indices inside the object in that order, padded with -1; rows of points that are not finite: 0 / -1.
 * 1 <= k <= ISMHIP_SOR_MAX_MEAN_K; larger k: ISMHIP_ERR_UNSUPPORTED. Timer "sift3d_extrema". Asynchronous. */
int  ismhip_sift3d_extrema(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* dog, int n_cols, int k, float min_contrast,
                           uint8_t* flags_out, int32_t* nn_idx_out);
#define ISMHIP_SIFT3D_MIN_POINTS 25   /* pcl::SIFTKeypoint: an octave below this many points ends the object; also its nr of neighbours */
#define ISMHIP_SIFT3D_MAX_OCTAVES 16
/* ismhip_sift3d_keypoints: the detector. cloud: the surface; intensity: device float[n_pts] in its point order (the reference: the
 * normals' curvature, ismhip_normal_curvature). scale = min_scale; for octave = 0 .. nr_octaves - 1: the current cloud (octave 0: the
 * surface's points with a finite intensity) is downsampled at leaf `scale` (ismhip_voxel_downsample_xyzi); an object left with fewer
 * than ISMHIP_SIFT3D_MIN_POINTS points stops there; on the others the scale space with scales[i] = scale * powf(2.0f, (i - 1.0f) /
 * nr_scales), i = 0 .. nr_scales + 2 (host, float) and the extrema with k = ISMHIP_SIFT3D_MIN_POINTS, on a search grid of cell size
 * 0.4f * (3.0f * scales[nr_scales + 2]) built and freed inside; scale *= 2.0f; the next octave downsamples THIS octave's cloud.
 * Output per object: octave ascending, then the octave's points in voxel order, then the column c ascending; each extremum one
 * keypoint: the octave point's position and scales[c] (kscale_out, or NULL). A position may appear more than once. kx|ky|kz|kscale_out:
 * device, `capacity` entries; kp_offsets_h_out[n_obj+1] (host); octave_sizes_h_out: host uint32[n_obj * nr_octaves] or NULL, the size
 * of the object's cloud at every octave it reached (the one that stopped it included), 0 behind. 1 <= nr_octaves <=
 * ISMHIP_SIFT3D_MAX_OCTAVES, 1 <= nr_scales <= 13, min_scale > 0, min_contrast >= 0 else ISMHIP_ERR_INVALID; more than `capacity`
 * keypoints: ISMHIP_ERR_INVALID, nothing written. Timers of the stages. The call synchronises. */
int  ismhip_sift3d_keypoints(ismhip_ctx* ctx, const ismhip_cloud* cloud, const float* intensity, float min_scale, int nr_octaves, int nr_scales,
                             float min_contrast, uint32_t capacity, float* kx, float* ky, float* kz, float* kscale_out,
                             uint32_t* kp_offsets_h_out, uint32_t* octave_sizes_h_out);

/* ---- feature filtering: Features::operator() drops non-finite LRFs (features.cpp:66-76),
 *      ImplicitShapeModel::removeNaNFeatures drops NaN descriptors (implicit_shape_model.cpp:1276-1308).
 *      Stable stream compaction of rows; keep_offsets_h_out[n_obj+1] (host) receives the new per-object
 *      ranges; src_index_out[nkp] (device) the source row of every kept row. The call synchronises. */
int  ismhip_compact_features(ismhip_ctx* ctx, int n_obj, const uint32_t* kp_offsets_h, int dim,
                             const float* desc, const float* lrf9,
                             const float* kpx, const float* kpy, const float* kpz,
                             float* desc_out, float* lrf9_out,
                             float* kpx_out, float* kpy_out, float* kpz_out,
                             uint32_t* src_index_out, uint32_t* keep_offsets_h_out);

/* The same filter for the descriptor matrices of THIS library: one element per row (desc[k * dim]) is tested instead of the matrix,
 * and when nothing is dropped *all_kept_out = 1, the *_out arrays are NOT written (the caller goes on with its input arrays;
 * src_index_out, if given, is 0..nkp-1) and keep_offsets_h_out = kp_offsets_h. Otherwise exactly as ismhip_compact_features.
 * THE ROW CONTRACT it rests on: a row is finite throughout or NaN throughout (invalid frame, keypoint not finite, empty
 * neighbourhood, zero norm, a NaN input reaching the histogram) -- never a finite first element with a NaN behind it, and never an
 * infinity. It covers the rows of all thirteen local Features entry points: ismhip_shot352 / ismhip_bshot352 / ismhip_cshot1344 /
 * ismhip_short_shot / ismhip_short_cshot / ismhip_fpfh33 / ismhip_cospair / ismhip_spin_image / ismhip_rsd / ismhip_rift /
 * ismhip_esf_local / ismhip_usc / ismhip_cgf_raw followed by ismhip_mlp_forward. Of these, FPFH rescales its three 11-bin blocks
 * independently, and they are NaN together; BSHOT holds no NaN at all (a NaN SHOT row is 352 ones and stays); a NaN raw CGF row gives
 * a NaN output row of the embedding, and only that row. tests/test_gpu_feature_batch.py holds every one of them to the contract on a
 * ragged batch with every kind of special row, and holds this call to ismhip_compact_features on those rows. A descriptor matrix from
 * anywhere else (a file, another library, rows edited by the caller) is filtered with ismhip_compact_features, which reads every
 * element. */
int  ismhip_compact_descriptor_rows(ismhip_ctx* ctx, int n_obj, const uint32_t* kp_offsets_h, int dim,
                                    const float* desc, const float* lrf9,
                                    const float* kpx, const float* kpy, const float* kpz,
                                    float* desc_out, float* lrf9_out,
                                    float* kpx_out, float* kpy_out, float* kpz_out,
                                    uint32_t* src_index_out, uint32_t* keep_offsets_h_out, int* all_kept_out);

/* ---- partial descriptors: Codebook::castVotes with UsePartialShot (codebook/codebook.cpp:416-475, mask :952-1036) keeps the
 *      histograms of some of the 32 SHOT signatures: dst[n_rows * n_cols] = src[:, cols_h] (cols_h host, ascending). */
int  ismhip_gather_columns(ismhip_ctx* ctx, int n_rows, int dim_in, const float* src, int n_cols, const int32_t* cols_h, float* dst);

/* ---- codebook: FlannHelper dataset (utils/flann_helper.cpp:21-70) + CodewordDistribution vote
 *      tables (codebook/codeword_distribution.cpp:73-144) + classSigmas (codebook.cpp:107,159-193).
 *      Rows of words_h are in getCodewords() order (ascending codeword id, codebook.cpp:856-859).
 *      Votes are CSR over words. All inputs are host arrays, copied once; the codebook stays resident. */
int  ismhip_codebook_create(ismhip_ctx* ctx, int n_words, int dim, const float* words_h,
                            const float* word_weight_h,          /* [n_words] Codeword::getWeight, may be NULL (=1) */
                            const uint32_t* vote_offsets_h,      /* [n_words+1] */
                            const float* vote_xyz_h,             /* [n_votes*3] vote in LRF coordinates */
                            const float* vote_weight_h,          /* [n_votes] learned centre weight, NULL = 1 */
                            const float* vote_class_weight_h,    /* [n_votes] statistical weight of the vote's class, NULL = 1 */
                            const uint32_t* vote_class_h,        /* [n_votes] */
                            const uint32_t* vote_instance_h,     /* [n_votes] */
                            const float* vote_bbox_quat_h,       /* [n_votes*4] (w,x,y,z), NULL = identity */
                            const float* vote_bbox_size_h,       /* [n_votes*3], NULL = 0 */
                            int n_classes, const float* class_sigma_h, /* [n_classes] variance per class id */
                            ismhip_codebook** out);
/* Codeword::getClassId per word (codebook/codeword.h:73-75; only meaningful for one-feature codewords). Default when not set:
 * the class of the word's first stored vote. Needed by ismhip_knn_rule only. */
int  ismhip_codebook_set_word_class(ismhip_ctx* ctx, ismhip_codebook* cb, const uint32_t* word_class_h);
/* Codeword::getFeaturePosition per word (codebook/codeword.h; the keypoint the codeword was trained at, Vote::keypoint_training of
 * every vote it casts, voting.cpp:71). word_keypoint_h: host [n_words*3]. Needed by ismhip_vote_keypoints(_csr) only. */
int  ismhip_codebook_set_word_keypoint(ismhip_ctx* ctx, ismhip_codebook* cb, const float* word_keypoint_h);
int  ismhip_codebook_destroy(ismhip_ctx* ctx, ismhip_codebook* cb);
int  ismhip_codebook_max_votes_per_word(const ismhip_codebook* cb);
/* Diagnostic: leading rotated coordinates of the codebook's stage-1 search image (0 = none: the squared-L2 candidate stage runs on
 * all dimensions). Speed only -- every ismhip_knn answer is the exact functor minimum either way. energy_out (may be NULL): share
 * of the codebook's second moment those coordinates hold. */
int  ismhip_codebook_stage1_dims(const ismhip_codebook* cb, float* energy_out);
/* The same for the image the queries whose stage-1 proof failed are searched on again (0: all dimensions). */
int  ismhip_codebook_stage2_dims(const ismhip_codebook* cb, float* energy_out);
/* Diagnostic: the rotated f16 image ismhip_knn makes of a query batch for stage 1 (stage = 1) or stage 2 (stage = 2), as the proofs
 * see it. q: device [nq x dim]. image_out: device [nq x m] f16 bits, row-major (the search's tiled layout undone); qn2_out / qn2h_out:
 * device [nq], |q|^2 of the rows and the sums of squares of the image rows as stored. r_out_h (host [m x dim_pad], may be NULL): the
 * fp32 rotation R the bound refers to. consts_out_h (host [3], may be NULL): the image scale s and the constants of
 * |image / s - R q|_2 <= d_rel |q|_2 + d_abs that the proofs use on this ctx (ISMHIP_KNN_ROTATE_F32 read at its creation).
 * Returns m (0: the codebook has no such image, nothing written) or a negative error. q == NULL or nq == 0: only m, R and the
 * constants. Synchronises. */
int  ismhip_codebook_rotate_probe(ismhip_ctx* ctx, const ismhip_codebook* cb, int stage, int nq, const float* q, uint16_t* image_out,
                                  float* qn2_out, float* qn2h_out, float* r_out_h, float* consts_out_h);
/* Diagnostic: the CIELab conversion every colour feature shares (PCL's RGB2CIELAB through the context's two LUTs, LUT index clamped to
 * 0..3999), one thread per colour. rgba: device [n] packed 0x00RRGGBB, bits 24..31 ignored. out: device [3 n], (L, a, b) per colour as
 * CoSPAIR takes them (L <= 100, |a|, |b| <= 120), or, with normalised != 0, (L / 100, a / 120, b / 120) as CSHOT, SHORT_CSHOT and the
 * culling colour score take them. Asynchronous on the ctx stream. Off every hot path. */
int  ismhip_rgb2lab(ismhip_ctx* ctx, int n, const uint32_t* rgba, int normalised, float* out);

/* The resident integer image of a codebook whose every element is exactly 0.0f or 1.0f (-0.0f counts as 0), e.g. B-SHOT rows
 * (features/features_bshot.cpp:96-99): int8 rows zero-padded to the search kernel's K step (128) and the number of ones per row.
 * ISMHIP_ERR_INVALID, with the codebook unchanged, when any element is something else. ISMHIP_ERR_UNSUPPORTED when the search key does
 * not fit: the key is a SIGNED 32-bit (distance << s) + row with s = ceil(log2(n_words rounded up to 256)), which needs
 * (dim + 2) * 2^s <= 2^31 (at dim 1344: up to 2^20 words). A second call is a no-op. Synchronises. */
int  ismhip_codebook_make_binary(ismhip_ctx* ctx, ismhip_codebook* cb);
/* 1 when the codebook holds that image, else 0 */
int  ismhip_codebook_has_binary(const ismhip_codebook* cb);

/* ---- activation: ActivationStrategyKNN::activateKNN (activation_strategy/activation_strategy_knn.h:41-126)
 *      with FLANNExactMatch semantics (SearchParams(-1)): exact k nearest codewords, ascending distance,
 *      ties -> lowest row. idx_out[nq*k] (row in words, -1 when n_words < k), dist_out[nq*k] = the FLANN
 *      functor value (utils/distance.cpp:33-52), recomputed by direct summation for the winners. */
int  ismhip_knn(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q,
                int k, int32_t* idx_out, float* dist_out);
/* ismhip_knn for 0/1 rows on a codebook with a binary image (ismhip_codebook_make_binary), 1 <= k <= 16. Between such rows both FLANN
 * functors (utils/distance.cpp:33-52) equal the Hamming distance, so there is no metric argument: the answers -- ascending (distance,
 * row), -1 entries with a NaN distance when n_words < k, dist_out = the functor value -- are bit-identical to ismhip_knn's for
 * ISMHIP_METRIC_L2SQ and for ISMHIP_METRIC_CHI2. The float query rows q[nq * dim] are packed on the device inside the call; the search
 * is one exact pass of 8-bit integer matrix-core products with int32 accumulation. ISMHIP_ERR_INVALID: a query element that is not 0 or 1
 * (the outputs are then void), a codebook without the image, k outside 1 .. 16. Any nq >= 0, n_words >= 1, dim >= 1; never falls back to
 * ismhip_knn. Timer "knn_binary"; counter "knn_binary_launches" (ismhip_timer_get, valid without timers): the calls that searched.
 * Synchronises. */
int  ismhip_knn_binary(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* q, int k, int32_t* idx_out, float* dist_out);
#define ISMHIP_KNN_LARGE_K_MAX 1024
/* ActivationStrategyKNN::activateKNN for any K (FLANNExactMatch semantics): the contract of ismhip_knn for
 * 1 <= k <= ISMHIP_KNN_LARGE_K_MAX. idx_out / dist_out device [nq*k]. Synchronises. k <= 16 is ismhip_knn itself. Larger k: squared-L2
 * launches that ismhip_knn_threshold would run on the matrix cores take a certified threshold search there first;
 * chi-square launches only with the environment variable ISMHIP_KNN_LARGE_K_FAST=1 at context creation; every query not certified
 * (all of them with ISMHIP_KNN_LARGE_K_EXACT=1) goes to an exact scan. Counters (ismhip_timer_get, valid without timers): "knn_large_k_certified_queries",
 * "knn_large_k_retry_queries", "knn_large_k_exact_queries" of the last call; timers "knn_large_k" and its parts
 * "knn_large_k_seed", "knn_large_k_sweep", "knn_large_k_eval", "knn_large_k_exact". */
int  ismhip_knn_large_k(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q,
                        int k, int32_t* idx_out, float* dist_out);
/* distance-ratio test of activateKNN (:74-85), k must be 1: needs the 2-NN; idx -> -1 when d1/d2 > threshold */
int  ismhip_knn_ratio(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q,
                      float ratio_threshold, int32_t* idx_out, float* dist_out);

/* ActivationStrategyKnnRule::activateKNN at detection time (activation_strategy/activation_strategy_knn_rule.h:41-152): exact
 * 3-NN, then the class-consistency rules over (c1,c2,c3) with the ratio tests d1/d3 and d1/d2; idx_out[nq] = accepted codeword
 * row (k1 or k2) or -1, dist_out[nq] = its functor distance. (At training time the rule is plain 1-NN: use ismhip_knn.) */
int  ismhip_knn_rule(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q,
                     float ratio_threshold, int32_t* idx_out, float* dist_out);

/* ActivationStrategyThreshold::activate (activation_strategy/activation_strategy_threshold.cpp:27-44): every codeword whose functor
 * value is STRICTLY below threshold, in ascending row order, as a CSR: act_offsets_out[nq+1] (device), idx_out / dist_out (device,
 * `capacity` entries; dist = the functor value, bit-equal to the FLANN functor). *n_act_h_out (host) = the total. The offsets and the
 * total are always written; the lists only when the total fits capacity (0: count only; otherwise grow the buffers and call again).
 * threshold <= 0 (or NaN) gives empty lists. A total of 2^32 or more is refused (ISMHIP_ERR_UNSUPPORTED). The call synchronises. */
int  ismhip_knn_threshold(ismhip_ctx* ctx, const ismhip_codebook* cb, int metric, int nq, const float* q, float threshold,
                          int64_t capacity, uint32_t* act_offsets_out, int32_t* idx_out, float* dist_out, int64_t* n_act_h_out);

/* ---- vote casting: Codebook::castVotes second loop + CodewordDistribution::castVotes/castVote
 *      (codebook.cpp:541-554, codeword_distribution.cpp:73-167), sink = Voting::vote (voting/voting.cpp:58-77).
 *      Vote slot of (feature f, activation j, stored vote v) = (f*k + j)*maxv + v with
 *      maxv = ismhip_codebook_max_votes_per_word; a slot that casts no vote has class = -1.
 *      All outputs are SoA of n_slots = nq*k*maxv entries. */
int  ismhip_cast_votes(ismhip_ctx* ctx, const ismhip_codebook* cb, uint32_t weight_flags,
                       int nq, const float* lrf9, const float* kpx, const float* kpy, const float* kpz,
                       int k, const int32_t* idx, const float* dist,
                       float* vote_pos_out,      /* [n_slots*3] */
                       float* vote_weight_out,   /* [n_slots] */
                       int32_t* vote_class_out,  /* [n_slots], -1 = no vote */
                       int32_t* vote_instance_out,
                       int32_t* vote_codeword_out,
                       float* vote_bbox_quat_out,/* [n_slots*4], may be NULL */
                       float* vote_bbox_size_out /* [n_slots*3], may be NULL */);

/* The same for a variable number of activations per feature (ismhip_knn_threshold): activation a of feature f lies in
 * [act_offsets[f], act_offsets[f+1]) (device, [nq+1]) of idx / dist (device, [n_act]). Vote slot of (activation a, stored vote v) =
 * a*maxv + v (feature-major); all outputs are SoA of n_slots = n_act*maxv entries. */
int  ismhip_cast_votes_csr(ismhip_ctx* ctx, const ismhip_codebook* cb, uint32_t weight_flags,
                           int nq, const float* lrf9, const float* kpx, const float* kpy, const float* kpz,
                           const uint32_t* act_offsets, int64_t n_act, const int32_t* idx, const float* dist,
                           float* vote_pos_out, float* vote_weight_out, int32_t* vote_class_out, int32_t* vote_instance_out,
                           int32_t* vote_codeword_out, float* vote_bbox_quat_out, float* vote_bbox_size_out);

/* The keypoint pair every vote carries (Voting::vote, voting/voting.cpp:58-77: Vote::keypoint = the query keypoint, Vote::keypoint_training
 * = the activated codeword's getFeaturePosition()), in the slot layout of ismhip_cast_votes / ismhip_cast_votes_csr with the same
 * (nq, k, idx) / (act_offsets, n_act, idx). vote_kp_out / vote_kp_train_out: device [n_slots*3]; a slot beyond the codeword's stored
 * votes gets zeros (the weight tests of castVote are not repeated: such a slot has class -1 and is never read). The codebook must
 * hold its training keypoints (ismhip_codebook_set_word_keypoint). Input of the RANSAC vote filter. */
int  ismhip_vote_keypoints(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* kpx, const float* kpy, const float* kpz,
                           int k, const int32_t* idx, float* vote_kp_out, float* vote_kp_train_out);
int  ismhip_vote_keypoints_csr(ismhip_ctx* ctx, const ismhip_codebook* cb, int nq, const float* kpx, const float* kpy, const float* kpz,
                               const uint32_t* act_offsets, int64_t n_act, const int32_t* idx, float* vote_kp_out, float* vote_kp_train_out);

/* ---- RANSAC vote filter: Voting::filterVotesWithRansac (voting/voting.cpp:110-127, 356-433) over
 *      pcl::registration::CorrespondenceRejectorSampleConsensus. PCL is EXTERNAL: the draws (a counter-based hash instead of PCL's
 *      mt19937(12345)), the three-point model in double and the scoring in double are this library's own definitions (DESIGN.md §4.6,
 *      restated in tests/ransac_ref.py; parity with the reference unpinned). PCL's SEQUENTIAL loop is the contract: hypotheses are
 *      evaluated in chunks, the stopping point is found by a scan in index order, ties keep the lowest index.
 *      Cluster c = votes [cluster_offsets_h[c], cluster_offsets_h[c+1]) of src_xyz (training keypoints) / tgt_xyz (scene keypoints)
 *      (device [n*3]); threshold_h[n_clusters] (host): inlier distance of every cluster, <= 0 drops it. A cluster is dropped
 *      (kept_out 0, no inliers) with fewer than 3 votes, without a good sample, with fewer than 3 inliers, or when the best motion
 *      is the identity to 1e-4 (Eigen isIdentity: the reference drops an object seen in its training pose). Outputs (device):
 *      inlier_out[n] 0/1, kept_out / n_inliers_out / best_hypothesis_out / iterations_out [n_clusters] (the last two may be NULL;
 *      iterations = the sequential stopping point), transform_out [n_clusters*16] row-major 4x4 or NULL (identity when dropped).
 *      RansacRefineModel is not built. Synchronises. Counters (ismhip_timer_get, valid without timers, since the last
 *      ismhip_timers_reset): "ransac_clusters", "ransac_clusters_kept", "ransac_hypotheses_needed" (sum of the stopping points),
 *      "ransac_hypotheses_evaluated" (what the chunks ran); timer "ransac_filter". */
int  ismhip_ransac_filter(ismhip_ctx* ctx, int n_clusters, const uint32_t* cluster_offsets_h, const float* src_xyz, const float* tgt_xyz,
                          const float* threshold_h, int max_iterations, unsigned long long seed,
                          uint8_t* inlier_out, int32_t* kept_out, int32_t* n_inliers_out, int32_t* best_hypothesis_out, int32_t* iterations_out,
                          float* transform_out);
/* Diagnostic: exactly hypothesis hypothesis_h[c] of cluster c, whatever its count: valid_out[c] = it had a good sample, inlier_out
 * its inlier mask, n_inliers_out its count, d2_out (device double [n]) the squared residual of every vote, transform_out (device
 * double [n_clusters*12], R row-major then t, or NULL). No identity test, no counters. The parity tests measure the library's d^2
 * against the restatement's with it. Synchronises. */
int  ismhip_ransac_hypothesis(ismhip_ctx* ctx, int n_clusters, const uint32_t* cluster_offsets_h, const float* src_xyz, const float* tgt_xyz,
                              const float* threshold_h, unsigned long long seed, const int32_t* hypothesis_h,
                              uint8_t* inlier_out, int32_t* valid_out, int32_t* n_inliers_out, double* d2_out, double* transform_out);

/* ---- maxima: Voting::findMaxima + VotingMeanShift::iFindMaxima + MaximaHandler
 *      (voting/voting.cpp:79-328,436-462; voting_mean_shift.cpp:39-177,201-481; maxima_handler.cpp:51-157) */
typedef struct ismhip_maxima_params {
    int   n_classes;
    const float* class_bandwidth_h; /* [n_classes] MaximaHandler::getSearchDistForClass; NULL -> bandwidth for all */
    float bandwidth;                /* Voting.Bandwidth */
    float threshold;                /* Voting.Threshold */
    int   max_iter;                 /* Voting.MaxIter */
    int   kernel;                   /* ISMHIP_KERNEL_* */
    int   suppression;              /* ISMHIP_SUPPRESS_* */
    int   min_votes_threshold;      /* Voting.MinVotesThreshold */
    float min_threshold;            /* Voting.MinThreshold (negative = relative to best) */
    int   best_k;                   /* Voting.BestK (<=0: all) */
    int   max_maxima;               /* capacity of the output per object */
    int   max_filter;               /* Voting.MaxFilterType: ISMHIP_MAXFILTER_NONE | _SIMPLE | _MERGE (MaximaHandler::filterMaxima,
                                       maxima_handler.cpp:272-440); not applied in single-object mode: pass NONE there (voting.cpp:262-268) */
    /* ---- ABI 4 (zero-initialise the struct: all of these are optional) */
    const float* vote_bbox_quat;    /* device [n_slots*4] (w,x,y,z), the vote_bbox_quat_out of ismhip_cast_votes: Voting.AverageRotation
                                       (voting.cpp:210-215, Utils::quatWeightedAverage utils.cpp:617-665; see DESIGN.md §7 for the
                                       eigenvector choice); NULL = off */
    float* max_bbox_quat_out;       /* device [n_obj*max_maxima*4]; required iff vote_bbox_quat is given */
    int   single_object_max_type;   /* ISMHIP_SOM_* */
    const float* object_centroid;   /* device [n_obj*3]: ismhip_cloud_centroids of the objects' clouds (ISMHIP_SOM_BANDWIDTH and up) */
    const float* object_radius;     /* device [n_obj]: ismhip_cloud_radii (ISMHIP_SOM_MODEL_RADIUS) */
} ismhip_maxima_params;

/* slot_offsets_h[n_obj+1]: vote-slot range of each object. Outputs per object o, maximum m (sorted by
 * weight, descending): index o*max_maxima + m. n_maxima_out[n_obj]. class_score_out[n_obj*n_classes] =
 * best normalised weight per class (0 when the class has no maximum) — the record the multi-GPU
 * all-gather exchanges.
 * vote_instance: any int32 except INT32_MIN (0x80000000), which marks an empty entry of the per-maximum instance table. A vote
 * carrying it adds its weight to an entry whose key stays empty; another id that claims that entry later inherits the weight, so
 * such a vote can inflate a different instance's sum and change the winner. Negative ids are fine; among equal sums the lowest id
 * AS AN UNSIGNED NUMBER wins (the reference's std::map<unsigned, float>). The same holds for ismhip_hough3d_maxima and the _ransac
 * entries. */
int  ismhip_find_maxima(ismhip_ctx* ctx, int n_obj, const uint32_t* slot_offsets_h,
                        const float* vote_pos, const float* vote_weight, const int32_t* vote_class,
                        const int32_t* vote_instance, const float* vote_bbox_size /* may be NULL */,
                        const ismhip_maxima_params* params,
                        int32_t* n_maxima_out, float* max_pos_out, float* max_weight_out,
                        int32_t* max_class_out, int32_t* max_instance_out, float* max_instance_weight_out,
                        float* max_bbox_size_out /* may be NULL */, int32_t* max_n_votes_out,
                        float* class_score_out);

/* Voting.RansacVoteFiltering (voting.cpp:110-127): every maximum's votes pass the RANSAC vote filter between the mode search and
 * the per-maximum sums (voting.cpp:131-236), which then see the inliers only; MinVotesThreshold is tested before and after; a
 * dropped cluster gives no maximum. The in-place reweighting of ALL votes around a maximum (voting_mean_shift.cpp:161-176) stays
 * before the filter. The cluster's list is its votes in ascending slot order. The instance tally uses the inlier votes' own
 * instance ids (the reference indexes the unfiltered list). */
typedef struct ismhip_ransac_params {
    const float* vote_keypoint;             /* device [n_slots*3]: vote_kp_out of ismhip_vote_keypoints(_csr) (the RANSAC target) */
    const float* vote_keypoint_training;    /* device [n_slots*3]: vote_kp_train_out (the RANSAC source) */
    float inlier_threshold;                 /* Voting.RansacInlierThreshold, already scaled when the type is not "Fixed" */
    const float* class_inlier_threshold_h;  /* [n_classes] per-class threshold (RansacInlierThresholdType "ObjectRadius" /
                                               "BoundingBoxMedian": the factor times m_dimensions_map[class]); NULL -> inlier_threshold */
    int   max_iterations;                   /* corr_rejector.setMaximumIterations: 10000 in the reference */
    unsigned long long seed;                /* of the draws; the same stream for every cluster, as in PCL */
} ismhip_ransac_params;
/* The arguments of ismhip_find_maxima, then the filter's. max_transform_out: device [n_obj*max_maxima*16] or NULL: the 4x4 (row-major,
 * float) of every returned maximum's best hypothesis (the reference discards it); a maximum merged by MaxFilterType "Merge" carries
 * the motion of the maximum whose place it takes. Timer "maxima"; the counters of ismhip_ransac_filter. */
int  ismhip_find_maxima_ransac(ismhip_ctx* ctx, int n_obj, const uint32_t* slot_offsets_h,
                               const float* vote_pos, const float* vote_weight, const int32_t* vote_class,
                               const int32_t* vote_instance, const float* vote_bbox_size /* may be NULL */,
                               const ismhip_maxima_params* params,
                               int32_t* n_maxima_out, float* max_pos_out, float* max_weight_out,
                               int32_t* max_class_out, int32_t* max_instance_out, float* max_instance_weight_out,
                               float* max_bbox_size_out /* may be NULL */, int32_t* max_n_votes_out,
                               float* class_score_out, const ismhip_ransac_params* ransac, float* max_transform_out);

/* ---- training: Codebook::activate (codebook/codebook.cpp:64-368): exact kNN activation of every training feature in the
 *      codebook, class sigma^2 (:94-193), K = 1 clean-up (:201-224), vote = rotateInto(centre - keypoint, LRF)
 *      (codeword_distribution.cpp:37-71), CodewordDistribution::computeWeights (:169-243) and the statistical class weights
 *      term1 * term2 * term3 (:226-368, including m_term3 being keyed by class only).
 *      The codewords are the rows of `codewords` (device [n_codewords * dim]: the cluster centres of ismhip_kmeans,
 *      implicit_shape_model.cpp:445-475), or, with codewords == NULL, the training features themselves (clustering_none.cpp:25-35).
 *      desc / lrf9 / kp* are device arrays of the n training features in CLASS-MAJOR order (classes ascending, models and
 *      features in the order the reference iterates them); feat_*_h are host arrays ([n], centre [n*3] = the model's bounding-box
 *      centre). Outputs are HOST arrays with m = number of codewords: word_src_out[m] (row of `codewords` behind every kept
 *      codeword, ascending = codeword order), vote_offsets_out[m+1] (CSR), vote_feature_out / vote_weight_out /
 *      vote_class_weight_out [n*k], vote_xyz_out[n*k*3], class_sigma_out[n_classes]. The call synchronises.
 *      k <= ISMHIP_KNN_LARGE_K_MAX (k > 16 activates through ismhip_knn_large_k);
 *      a codeword with more than 32768 votes is refused (ISMHIP_ERR_UNSUPPORTED). */
int  ismhip_train_activate(ismhip_ctx* ctx, int metric, int n, int dim, const float* desc, const float* lrf9,
                           const float* kpx, const float* kpy, const float* kpz,
                           const uint32_t* feat_class_h, const uint32_t* feat_model_h, const float* feat_center_h,
                           int n_codewords, const float* codewords /* device, may be NULL */,
                           int k, int clean_up_single_vote, int n_classes,
                           int32_t* n_words_out, uint32_t* word_src_out, uint32_t* vote_offsets_out, uint32_t* vote_feature_out,
                           float* vote_xyz_out, float* vote_weight_out, float* vote_class_weight_out, float* class_sigma_out);

/* Codebook::activate with a variable number of activations per feature (ActivationStrategyThreshold, codebook.cpp:139-142): the
 * activations are given as a CSR, act_offsets (device, [n+1]) into act_idx (device, [n_act], rows of `codewords`, ascending per
 * feature), e.g. from ismhip_knn_threshold. No K = 1 clean-up. The sigma^2 word sample takes whole activation lists of a class's
 * first features while it holds fewer than sqrt(#features) words (:159-160, so it may overshoot); a class whose sample is empty gets
 * 0/0 = NaN, as the reference computes it. Outputs as ismhip_train_activate, sized n_act instead of n*k. */
int  ismhip_train_activate_lists(ismhip_ctx* ctx, int metric, int n, int dim, const float* desc, const float* lrf9,
                                 const float* kpx, const float* kpy, const float* kpz,
                                 const uint32_t* feat_class_h, const uint32_t* feat_model_h, const float* feat_center_h,
                                 int n_codewords, const float* codewords /* device, may be NULL */,
                                 const uint32_t* act_offsets, const int32_t* act_idx, int64_t n_act, int n_classes,
                                 int32_t* n_words_out, uint32_t* word_src_out, uint32_t* vote_offsets_out, uint32_t* vote_feature_out,
                                 float* vote_xyz_out, float* vote_weight_out, float* vote_class_weight_out, float* class_sigma_out);

/* ---- training-side feature ranking ("codebook cleaning"): FeatureRanking::operator() (feature_ranking/feature_ranking.cpp:37-118),
 *      the step of ImplicitShapeModel::train() between feature extraction and clustering (implicit_shape_model.cpp:437-443).
 *      ismhip_rank_scores is iComputeScores of one subclass, ismhip_rank_select is rankFeaturesWithScores +
 *      extractSubsetFromRankedList (feature_ranking.cpp:121-203). Every search is exact (FLANNExactMatch semantics) and uses the
 *      chi-square functor whatever the model's DistanceType says, as the reference's hard-coded flann::ChiSquareDistance does
 *      (feature_ranking.cpp:35). Neighbour lists are in ismhip_knn's (distance, row) order. */
#define ISMHIP_RANK_KNN_ACTIVATION 0   /* ranking_knn_activation.cpp:53-110 (UseFeaturePosition false) */
#define ISMHIP_RANK_INCREMENTAL    1   /* ranking_incremental.cpp:51-84 */
#define ISMHIP_RANK_STRANGENESS    2   /* ranking_strangeness.cpp:58-93 */
#define ISMHIP_RANK_NAIVE_BAYES    3   /* ranking_naive_bayes.cpp:52-79, feature_ranking.cpp:346-363 */
/* desc: device [n*dim], CLASS-MAJOR as in ismhip_train_activate; class_offsets_h: host [n_classes+1], from 0 to n, ascending (empty
 * classes allowed); score_out: device [n]. With m = min(K, n) valid neighbours per query:
 *   KNN_ACTIVATION  K = k_search + 1 in all features; each of the first m - 1 neighbours (the LAST one is dropped, not the self match)
 *                   gets 1 (increment_type 1, and 0 which means 1), 1 / (d + 1) (2) or expf(d) (3) added to its score
 *   INCREMENTAL     the same search; neighbour j < m - 1 gets d_j - d_(j+1)
 *   both are float sums in the reference's sequential order (queries ascending, then rank), without float atomics: two calls give the
 *   same bits
 *   STRANGENESS     per class c the float sum, ascending, of the distances to the feature's k_search nearest rows of class c (fewer in a
 *                   smaller class, 0 for an empty one); score = own-class sum / smallest sum of the other classes
 *   NAIVE_BAYES     num_pos = those of the k_search nearest own-class rows with d < dist_threshold, num_neg = the same count over the
 *                   k_search nearest rows of all other classes together (ties in global row order);
 *                   score = (num_pos / num_current) / ((num_pos + num_neg) / (num_current + num_other)) in float, in that order
 * ISMHIP_ERR_INVALID, with score_out unwritten: an unknown type, k_search < 1, increment_type outside 0 .. 3 (KNN_ACTIVATION), offsets that
 * do not ascend from 0 to n, STRANGENESS with fewer than two non-empty classes (the reference would index past the end).
 * ISMHIP_ERR_UNSUPPORTED: K > ISMHIP_KNN_LARGE_K_MAX, dim > ISMHIP_SHORT_CSHOT_MAX_DIM. K > 16 searches through ismhip_knn_large_k.
 * Timers "rank_scores" (the searches included) and, of it, "rank_score_kernels" (everything after the searches); counter "rank_launches": calls of the two entries that reached the device. Synchronises. */
int  ismhip_rank_scores(ismhip_ctx* ctx, int type, int n, int dim, const float* desc, int n_classes, const uint32_t* class_offsets_h,
                        int k_search, float dist_threshold, int increment_type, float* score_out);
/* Per class of size s: min_index = (float)s * extract_offset clamped at 0, max_index = (float)s * (factor + extract_offset) clamped at
 * s; the feature of ascending rank j is kept iff (float)j >= min_index && (float)j < max_index. The reference sorts with an unstable
 * std::sort on the score alone; here the order is DEFINED: ascending by (score, index within the class), -0 equal to +0, NaN after
 * +inf. score: device [n]; keep_out: device [n], 1 = kept; n_keep_h_out: host [n_classes]. Two order statistics per class by a radix
 * select over the 64-bit key (ordered score bits, index): linear in the class size. ISMHIP_ERR_INVALID, outputs unwritten: offsets
 * that do not ascend from 0 to n. Timer "rank_select". Synchronises. */
int  ismhip_rank_select(ismhip_ctx* ctx, int n, int n_classes, const uint32_t* class_offsets_h, const float* score,
                        float factor, float extract_offset, uint8_t* keep_out, uint32_t* n_keep_h_out);

/* ---- k-means codebook clustering: ClusteringKMeans::cluster (clustering/clustering_kmeans.h:53-131) =
 *      flann::hierarchicalClustering with branching == the cluster count (one level of Lloyd k-means: centre chooser, then
 *      [means -> reassign, ties to the lowest centre -> refill empty clusters] until nothing moves or max_iterations), followed by
 *      the nearest centre of every feature. FLANN is EXTERNAL and draws from rand(): the random draws, the integer form of the
 *      k-means++ sampling and of the means, and the exact final search are this library's own definitions (csrc/kmeans.hip,
 *      restated in oracle/; parity with the reference unpinned). desc: device [n * dim]. n_clusters is clipped to n.
 *      centers_out: device [n_clusters * dim]; assign_out: device [n] (row of centers_out); dist_out: device [n] or NULL (functor
 *      distance to that centre); *n_clusters_out <= n_clusters (fewer when the distinct points run out). Synchronises. */
#define ISMHIP_CENTERS_RANDOM   0
#define ISMHIP_CENTERS_GONZALES 1
#define ISMHIP_CENTERS_KMEANSPP 2
int  ismhip_kmeans(ismhip_ctx* ctx, int metric, int n, int dim, const float* desc, int n_clusters, int max_iterations,
                   int centers_init, unsigned long long seed, float* centers_out, int32_t* assign_out, float* dist_out,
                   int32_t* n_clusters_out, int32_t* iterations_out /* may be NULL */);

/* ---- discrete Hough space: VotingHough3D::iFindMaxima (voting/voting_hough_3d.cpp:33-95) over pcl::recognition::HoughSpace3D
 *      (bins ceil((max-min)/bin) per axis; trilinear voteInt; findMaxima(-RelThreshold): bins >= rel * max with no strictly
 *      greater 26-neighbour, in ascending bin index) followed by the same Voting::findMaxima post-processing as
 *      ismhip_find_maxima (same outputs). The reference makes the bins cubic: edge = 2 * MaximaHandler::getSearchDistForClass,
 *      i.e. BinSize[0] for BinOrBandwidthType "Config" (voting_hough_3d.cpp:46-48). */
typedef struct ismhip_hough_params {
    int   n_classes;
    float min_coord[3];             /* Voting.MinCoord */
    float max_coord[3];             /* Voting.MaxCoord */
    float bin_size;                 /* Voting.BinSize[0] */
    const float* class_bin_h;       /* [n_classes] per-class bin edge; NULL -> bin_size for all */
    int   use_interpolation;        /* Voting.UseInterpolation */
    float rel_threshold;            /* Voting.RelThreshold */
    int   min_votes_threshold;      /* Voting.MinVotesThreshold */
    float min_threshold;            /* Voting.MinThreshold (negative = relative to best) */
    int   best_k;                   /* Voting.BestK (<=0: all) */
    int   max_maxima;               /* capacity of the output per object */
    int   max_filter;               /* as ismhip_maxima_params.max_filter; the radius is bin_size / 2 (voting_hough_3d.cpp:45) */
    /* ---- ABI 4 (zero-initialise the struct) */
    const float* vote_bbox_quat;    /* Voting.AverageRotation, as in ismhip_maxima_params */
    float* max_bbox_quat_out;
} ismhip_hough_params;
int  ismhip_hough3d_maxima(ismhip_ctx* ctx, int n_obj, const uint32_t* slot_offsets_h,
                           const float* vote_pos, const float* vote_weight, const int32_t* vote_class,
                           const int32_t* vote_instance, const float* vote_bbox_size /* may be NULL */,
                           const ismhip_hough_params* params,
                           int32_t* n_maxima_out, float* max_pos_out, float* max_weight_out,
                           int32_t* max_class_out, int32_t* max_instance_out, float* max_instance_weight_out,
                           float* max_bbox_size_out /* may be NULL */, int32_t* max_n_votes_out,
                           float* class_score_out);

/* ismhip_hough3d_maxima with Voting.RansacVoteFiltering: as ismhip_find_maxima_ransac. The voters of a maximum's bin are the cluster;
 * the maximum's position stays the weighted centre of ALL voters (filterVotesWithRansac leaves a cluster's position alone), every
 * other per-maximum sum is taken over the inliers. Timer "hough3d". */
int  ismhip_hough3d_maxima_ransac(ismhip_ctx* ctx, int n_obj, const uint32_t* slot_offsets_h,
                                  const float* vote_pos, const float* vote_weight, const int32_t* vote_class,
                                  const int32_t* vote_instance, const float* vote_bbox_size /* may be NULL */,
                                  const ismhip_hough_params* params,
                                  int32_t* n_maxima_out, float* max_pos_out, float* max_weight_out,
                                  int32_t* max_class_out, int32_t* max_instance_out, float* max_instance_weight_out,
                                  float* max_bbox_size_out /* may be NULL */, int32_t* max_n_votes_out,
                                  float* class_score_out, const ismhip_ransac_params* ransac, float* max_transform_out);

#ifdef __cplusplus
}
#endif
#endif /* ISMHIP_H_ */
