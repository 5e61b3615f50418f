/*
 * colmap_amd_match.h -- C ABI of SIFT descriptor matching: brute-force nearest neighbours between the 128-byte
 * descriptor sets of image pairs, with the ratio test, the distance threshold and the cross check (`colmap
 * exhaustive_matcher`, `sequential_matcher`, `matches_importer`; reference src/colmap).
 *
 * Replaces, for descriptors that are already in memory:
 *   feature/sift.cc:1346-1473   SiftGPUFeatureMatcher (Match, its SetDescriptors reuse of uploaded sets)
 *   feature/sift.cc:967-1004    ComputeSiftDistanceMatrix, DOT_PRODUCT
 *   feature/sift.cc:772-864     FindBestMatchesOneWayBruteForce, FindBestMatchesBruteForce
 *   feature/matcher.h           FeatureMatcherCache, the part that keeps descriptors close to the matcher
 * The reference matches one pair per call. Here a handle keeps descriptor sets resident on the device by image id and
 * one call matches a LIST of pairs in one launch. The device computes the integer products and, for every descriptor of
 * both images of a pair, (idx, best, second): the first column with the largest product, that product, and the largest
 * product once one instance of the best is taken away (0, 0 and idx = -1 where every product is 0). The thresholds
 * (C library acosf), the cross check and the ordering are applied on the host (colmap_amd/csrc/match_plan.h). All
 * device results are integers with one possible value: they depend neither on the batch nor on the position in it.
 * There is no CPU path.
 */
#ifndef COLMAP_AMD_MATCH_H_
#define COLMAP_AMD_MATCH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MATCH_DESCRIPTOR_DIM = 128, MATCH_DEFAULT_MAX_NUM_MATCHES = 32768 };

/* SiftMatchingOptions (feature/sift.h) and TwoViewGeometryOptions::min_num_inliers as the controller applies it to the
 * raw matches (controllers/feature_matching_utils.cc:502-505). */
typedef struct match_options {
  float max_ratio;         /* 0.8 */
  float max_distance;      /* 0.7 */
  int32_t cross_check;     /* 1 */
  int32_t min_num_inliers; /* 15: a shorter result becomes empty; 0 keeps everything */
} match_options;

typedef struct match_pair {
  uint32_t image_id1, image_id2;
} match_pair;

typedef struct match_handle match_handle;

void match_options_init(match_options* options);

/* SiftGPUFeatureMatcher::Create (sift.cc:1351-1390). max_num_matches: descriptors of a set that take part (0 = 32768,
 * FeatureMatchingOptions::max_num_matches); cache_bytes: device bytes the resident descriptor sets may take before the
 * least recently used ones are dropped (0 = 4 GiB; never less than one pair of max_num_matches descriptors). 0 = ok. */
int match_create(int32_t gpu_index, int32_t max_num_matches, size_t cache_bytes, match_handle** handle);

/* The upload half of SiftGPUFeatureMatcher::Match (sift.cc:1420-1447, SetDescriptors) and FeatureMatcherCache::
 * GetDescriptors: puts data[rows][cols] (cols must be 128) on the device under image_id, replacing what was there. Only
 * the first max_num_matches rows take part (a warning goes to stderr, sift.cc:1404-1418). 0 = ok. */
int match_set_descriptors(match_handle* handle, uint32_t image_id, int32_t rows, int32_t cols, const uint8_t* data);

/* 1 when image_id is resident (and marks it as just used), else 0. */
int match_has_descriptors(match_handle* handle, uint32_t image_id);

/* SiftGPUFeatureMatcher::Match (sift.cc:1392-1473) for n pairs in one launch; every image must be resident. The results
 * stay in the handle until the next call. 0 = ok. */
int match_pairs(match_handle* handle, const match_pair* pairs, int32_t n, const match_options* options);

/* FeatureMatches of pair k of the last match_pairs: the count, then a copy of [count][2] uint32 (point2D_idx1,
 * point2D_idx2), ascending in point2D_idx1. 0 = ok. */
int match_num_matches(match_handle* handle, int32_t k, int64_t* count);
int match_copy_matches(match_handle* handle, int32_t k, uint32_t* matches, int64_t capacity);

/* What the device computed for pair k: direction 0 is one row per descriptor of image 1 over the columns of image 2,
 * direction 1 the transposed problem. out[rows][3] = idx, best, second. 0 = ok. */
int match_num_rows(match_handle* handle, int32_t k, int32_t direction, int64_t* rows);
int match_copy_selection(match_handle* handle, int32_t k, int32_t direction, int32_t* out, int64_t capacity);

/* Resident sets, their device bytes, and the sets dropped so far to stay within cache_bytes. */
void match_cache_stats(match_handle* handle, int64_t* entries, int64_t* bytes, int64_t* evictions);

/* Query rows one workgroup owns (the unit of the tile table). */
int match_tile_rows(void);

/* Kernel time (HIP events) and whole time of this thread's last match_pairs, in milliseconds. */
void match_last_timing(double* kernel_ms, double* total_ms);

void match_destroy(match_handle* handle);

const char* match_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* COLMAP_AMD_MATCH_H_ */
