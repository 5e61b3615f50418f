// model_align.hip -- model alignment on gfx950 behind include/colmap_amd_align.h: scoring batches of similarity
// hypotheses against the common observations (or the matched points) of two models, and applying a similarity to points.
// The host side of the search -- layouts, samples, stopping rule, LORANSAC -- is align_plan.h; this file uploads, launches
// and hands that loop a scorer.
//
// Kernels, all geometry in double:
//   align_reproj_score_kernel   ReconstructionAlignmentEstimator::Residuals (estimators/alignment.cc:94-175) for a tile
//                               of kHypTile hypotheses. The plan sorts the records by image and pads every image to whole
//                               waves, so a wave64 holds ONE image: poses and cameras are wave-uniform (scalar loads) and
//                               the wave takes one branch of each camera-model switch. A lane loads its record once -- 10
//                               doubles -- and keeps it in registers while the wave walks the tile; per hypothesis it
//                               evaluates CalculateSquaredReprojectionError (scene/projection.cc:74-91; the angular form
//                               of :46-52 for spherical cameras, DBL_MAX for a missing projection) of the src point in the
//                               tgt image and, where that passes, of the tgt point in the src image. The wave's count is
//                               one __ballot + popcount, written to partial[h][wave].
//   align_reproj_reduce_kernel  inliers[h][image] = sum of the partials of the image's waves, in wave order. Integers.
//   align_position_score_kernel SimilarityTransformEstimator::Residuals + InlierSupportMeasurer::Evaluate: a block of 256
//                               lanes takes a chunk of 1024 points, 4 per lane, held in registers over the tile.
//                               Summation order of residual_sum, a function of N alone: lane l of chunk c adds its
//                               inlier residuals of points 1024 c + l + 256 j, j = 0..3, in that order; a wave adds its 64
//                               lanes by the shuffle-down tree with offsets 32, 16, 8, 4, 2, 1 (lane i += lane i + off);
//                               the block adds its 4 wave sums in wave order; align_position_reduce_kernel adds the chunk
//                               sums of a hypothesis in chunk order, one lane per hypothesis.
//   align_transform_points_kernel  X' = s (R X) + t in place, one lane per point.
// No atomics of any kind. A hypothesis' counts and the bits of its residual sum do not depend on the batch size or on
// its position in the batch: the tile only decides which lanes' loop visits it, never an order of additions.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/colmap_amd_align.h"
#include "align_plan.h"
#include "camera_projection.h"

#define ALIGN_API __attribute__((visibility("default")))

namespace {

namespace ud = camera;
namespace ap = align_plan;

thread_local std::string g_error;
thread_local double g_kernel_ms = 0.0, g_total_ms = 0.0;

using Fail = ap::Fail;
#define ALIGN_HIP(call)                                                                  \
  do {                                                                                   \
    const hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess) throw Fail(std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <typename F>
int Guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / ap::kWave;
constexpr int kHypTile = ALIGN_HYPOTHESIS_TILE;
constexpr int kPointsPerLane = 4;
constexpr int kChunk = kBlock * kPointsPerLane;  // points of one block of the position scorer
constexpr int kRecordDoubles = 10;               // src xyz, tgt xyz, src xy, tgt xy

struct DevCamera {
  int model, width;
  double p[ud::kMaxParams];
};

struct DevImage {  // both sides of a common image
  double src_pose[12], tgt_pose[12];  // cam_from_world as 3x4 [R | t], row-major (Rigid3d::ToMatrix)
  DevCamera src_cam, tgt_cam;
};

struct DevHypothesis {
  double tgt_from_src[12], src_from_tgt[12];  // 3x4 [sR | t] of the Sim3 and of Inverse(Sim3)
};

struct DevSim3 {  // x -> s * (R x) + t
  double R[9], s, t[3];
};

// ---------------------------------------------------------------------------------------------------------------------
// device code
// ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void apply3x4(const double* __restrict__ M, double x, double y, double z, double o[3]) {
  o[0] = M[0] * x + M[1] * y + M[2] * z + M[3];
  o[1] = M[4] * x + M[5] * y + M[6] * z + M[7];
  o[2] = M[8] * x + M[9] * y + M[10] * z + M[11];
}

// the measured pixel's unit bearing for a spherical camera; has = false where CamRayFromImg has no value
struct Ray {
  double x, y, z;
  bool has;
};

// CalculateSquaredReprojectionError(point2D, world_from_other * X, cam_from_world, camera): scene/projection.cc:74-91.
// `ray` is the bearing of the measured pixel, used by spherical cameras only (it does not depend on the hypothesis).
__device__ __forceinline__ double squared_reproj_error(const double* __restrict__ map, const double* __restrict__ pose,
                                                       const DevCamera* __restrict__ cam, int m, double X, double Y, double Z,
                                                       double px, double py, const Ray& ray) {
  double w[3], pc[3];
  apply3x4(map, X, Y, Z, w);
  apply3x4(pose, w[0], w[1], w[2], pc);
  if (ud::is_spherical(m)) {
    double angle = ud::kPi;  // CalculateAngularReprojectionError: pi when the pixel has no ray
    if (ray.has) {
      double nx = pc[0], ny = pc[1], nz = pc[2];
      const double n2 = nx * nx + ny * ny + nz * nz;
      if (n2 > 0.0) {  // Eigen's normalized() leaves the zero vector alone
        const double n = sqrt(n2);
        nx /= n;
        ny /= n;
        nz /= n;
      }
      const double c = ray.x * nx + ray.y * ny + ray.z * nz;
      angle = acos(fmin(fmax(c, -1.0), 1.0));
    }
    const double pixels_per_radian = (double)cam->width / (2.0 * ud::kPi);
    const double pixel_error = angle * pixels_per_radian;
    return pixel_error * pixel_error;
  }
  double qx, qy;
  if (!ud::img_from_cam(m, cam->p, pc[0], pc[1], pc[2], &qx, &qy)) return DBL_MAX;
  const double dx = qx - px, dy = qy - py;
  return dx * dx + dy * dy;
}

__global__ __launch_bounds__(kBlock) void align_reproj_score_kernel(const double* __restrict__ rows, long long num_rows,
                                                                     const int* __restrict__ wave_image,
                                                                     const int* __restrict__ wave_count, int num_waves,
                                                                     const DevImage* __restrict__ images,
                                                                     const DevHypothesis* __restrict__ hyps, int num_hyps,
                                                                     double max_squared_error,
                                                                     unsigned* __restrict__ partial) {
  const int wave = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6);
  if (wave >= num_waves) return;  // the whole wave leaves
  const int lane = threadIdx.x & 63;
  const int img = __builtin_amdgcn_readfirstlane(wave_image[wave]);
  const int count = __builtin_amdgcn_readfirstlane(wave_count[wave]);
  const bool valid = lane < count;
  const long long row = (long long)wave * 64 + lane;  // < num_rows: padding rows exist and hold zeros
  double v[kRecordDoubles];
#pragma unroll
  for (int c = 0; c < kRecordDoubles; ++c) v[c] = rows[(long long)c * num_rows + row];
  const DevImage* __restrict__ im = images + img;
  const int src_model = im->src_cam.model, tgt_model = im->tgt_cam.model;
  Ray src_ray = {0.0, 0.0, 0.0, false}, tgt_ray = {0.0, 0.0, 0.0, false};
  if (ud::is_spherical(src_model)) src_ray.has = ud::cam_ray_from_img(src_model, im->src_cam.p, v[6], v[7], &src_ray.x, &src_ray.y, &src_ray.z);
  if (ud::is_spherical(tgt_model)) tgt_ray.has = ud::cam_ray_from_img(tgt_model, im->tgt_cam.p, v[8], v[9], &tgt_ray.x, &tgt_ray.y, &tgt_ray.z);

  const int h0 = blockIdx.y * kHypTile;
  const int h1 = h0 + kHypTile < num_hyps ? h0 + kHypTile : num_hyps;
  for (int h = h0; h < h1; ++h) {
    const DevHypothesis* __restrict__ H = hyps + h;
    bool inlier = false;
    if (valid) {
      // alignment.cc:141-161: `error > max` leaves, so a NaN error stays, as there
      const double e_tgt = squared_reproj_error(H->tgt_from_src, im->tgt_pose, &im->tgt_cam, tgt_model, v[0], v[1], v[2],
                                                v[8], v[9], tgt_ray);
      if (!(e_tgt > max_squared_error)) {
        const double e_src = squared_reproj_error(H->src_from_tgt, im->src_pose, &im->src_cam, src_model, v[3], v[4], v[5],
                                                  v[6], v[7], src_ray);
        inlier = !(e_src > max_squared_error);
      }
    }
    const unsigned long long votes = __ballot(inlier ? 1 : 0);
    if (lane == 0) partial[(size_t)h * num_waves + wave] = (unsigned)__popcll(votes);
  }
}

__global__ __launch_bounds__(kBlock) void align_reproj_reduce_kernel(const unsigned* __restrict__ partial, int num_waves,
                                                                      const int* __restrict__ image_wave_begin, int num_images,
                                                                      int num_hyps, unsigned* __restrict__ inliers) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)num_hyps * num_images) return;
  const int h = (int)(t / num_images), i = (int)(t % num_images);
  unsigned sum = 0u;
  for (int w = image_wave_begin[i]; w < image_wave_begin[i + 1]; ++w) sum += partial[(size_t)h * num_waves + w];
  inliers[t] = sum;
}

__device__ __forceinline__ void apply_sim3(const DevSim3* __restrict__ S, double x, double y, double z, double o[3]) {
  o[0] = S->s * (S->R[0] * x + S->R[1] * y + S->R[2] * z) + S->t[0];
  o[1] = S->s * (S->R[3] * x + S->R[4] * y + S->R[5] * z) + S->t[1];
  o[2] = S->s * (S->R[6] * x + S->R[7] * y + S->R[8] * z) + S->t[2];
}

// chunk_sum / chunk_count: [num_chunks][num_hyps]
__global__ __launch_bounds__(kBlock) void align_position_score_kernel(const double* __restrict__ src,
                                                                       const double* __restrict__ tgt, int num_points,
                                                                       const DevSim3* __restrict__ sims, int num_hyps,
                                                                       double max_squared_error, double* __restrict__ chunk_sum,
                                                                       unsigned* __restrict__ chunk_count,
                                                                       unsigned char* __restrict__ mask) {
  __shared__ double wave_sum[kHypTile][kWavesPerBlock];
  __shared__ unsigned wave_count[kHypTile][kWavesPerBlock];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  double a[kPointsPerLane][3], b[kPointsPerLane][3];
#pragma unroll
  for (int j = 0; j < kPointsPerLane; ++j) {
    const long long p = base + (long long)kBlock * j;
    const bool in = p < num_points;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a[j][c] = in ? src[3 * p + c] : 0.0;
      b[j][c] = in ? tgt[3 * p + c] : 0.0;
    }
  }
  const int h0 = blockIdx.y * kHypTile;
  const int h1 = h0 + kHypTile < num_hyps ? h0 + kHypTile : num_hyps;
  for (int h = h0; h < h1; ++h) {
    const DevSim3* __restrict__ S = sims + h;
    double sum = 0.0;
    unsigned count = 0u;
#pragma unroll
    for (int j = 0; j < kPointsPerLane; ++j) {
      const long long p = base + (long long)kBlock * j;
      if (p < num_points) {
        double o[3];
        apply_sim3(S, a[j][0], a[j][1], a[j][2], o);
        const double dx = b[j][0] - o[0], dy = b[j][1] - o[1], dz = b[j][2] - o[2];
        const double r = dx * dx + dy * dy + dz * dz;
        const bool inlier = r <= max_squared_error;
        if (inlier) {
          sum += r;
          ++count;
        }
        if (mask) mask[(size_t)h * (size_t)num_points + (size_t)p] = inlier ? 1 : 0;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      sum += __shfl_down(sum, off);
      count += (unsigned)__shfl_down((int)count, off);
    }
    if (lane == 0) {
      wave_sum[h - h0][wave] = sum;
      wave_count[h - h0][wave] = count;
    }
  }
  __syncthreads();
  const int hl = threadIdx.x;
  if (hl < h1 - h0) {
    double sum = wave_sum[hl][0];
    unsigned count = wave_count[hl][0];
    for (int w = 1; w < kWavesPerBlock; ++w) {
      sum += wave_sum[hl][w];
      count += wave_count[hl][w];
    }
    chunk_sum[(size_t)blockIdx.x * num_hyps + h0 + hl] = sum;
    chunk_count[(size_t)blockIdx.x * num_hyps + h0 + hl] = count;
  }
}

__global__ __launch_bounds__(kBlock) void align_position_reduce_kernel(const double* __restrict__ chunk_sum,
                                                                        const unsigned* __restrict__ chunk_count,
                                                                        int num_chunks, int num_hyps,
                                                                        double* __restrict__ residual_sum,
                                                                        long long* __restrict__ num_inliers) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= num_hyps) return;
  double sum = 0.0;
  long long count = 0;
  for (int c = 0; c < num_chunks; ++c) {
    sum += chunk_sum[(size_t)c * num_hyps + h];
    count += (long long)chunk_count[(size_t)c * num_hyps + h];
  }
  residual_sum[h] = sum;
  num_inliers[h] = count;
}

__global__ __launch_bounds__(kBlock) void align_transform_points_kernel(double* __restrict__ points, long long num_points,
                                                                         DevSim3 S) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= num_points) return;
  double* X = points + 3 * p;
  double o[3];
  apply_sim3(&S, X[0], X[1], X[2], o);
  X[0] = o[0];
  X[1] = o[1];
  X[2] = o[2];
}

// ---------------------------------------------------------------------------------------------------------------------
// host code
// ---------------------------------------------------------------------------------------------------------------------

void bind_device(int gpu_index) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw Fail("no HIP device available: model alignment runs on the GPU (there is no CPU path)");
  if (!(gpu_index >= 0 && gpu_index < ndev)) throw Fail("gpu_index " + std::to_string(gpu_index) + " out of range");
  ALIGN_HIP(hipSetDevice(gpu_index));
}

template <typename T>
struct DeviceBuffer {
  T* p = nullptr;
  size_t n = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  void alloc(size_t count) {
    release();
    if (count == 0) return;
    ALIGN_HIP(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
  }
  void reserve(size_t count) {  // scratch: contents are not kept
    if (count > n) alloc(count);
  }
  void upload(const T* host, size_t count) {
    alloc(count);
    if (count) ALIGN_HIP(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
  }
  void download(T* host, size_t count) const {
    if (count && host) ALIGN_HIP(hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DeviceBuffer() { release(); }
};

struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
  Timer() {
    ALIGN_HIP(hipEventCreate(&a));
    ALIGN_HIP(hipEventCreate(&b));
  }
  Timer(const Timer&) = delete;
  Timer& operator=(const Timer&) = delete;
  ~Timer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void start() { ALIGN_HIP(hipEventRecord(a, 0)); }
  double stop() {
    ALIGN_HIP(hipEventRecord(b, 0));
    ALIGN_HIP(hipEventSynchronize(b));
    float ms = 0.0f;
    ALIGN_HIP(hipEventElapsedTime(&ms, a, b));
    return ms;
  }
};

inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + kBlock - 1) / kBlock); }

DevSim3 dev_sim3(const double sim[8]) {
  DevSim3 S;
  ap::sim3_rotation(sim, S.R);
  S.s = sim[0];
  for (int k = 0; k < 3; ++k) S.t[k] = sim[5 + k];
  return S;
}

void pose_matrix(const double pose[7], double M[12]) {
  double R[9];
  colmap_amd::QuatToRot(pose, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) M[4 * r + c] = R[3 * r + c];
    M[4 * r + 3] = pose[4 + r];
  }
}

DevCamera dev_camera(const align_camera& c) {
  DevCamera d;
  d.model = c.model_id;
  d.width = c.width;
  for (int k = 0; k < ud::kMaxParams; ++k) d.p[k] = k < c.num_params ? c.params[k] : 0.0;
  return d;
}

enum Kind { KIND_REPROJ = 1, KIND_POSITIONS = 2 };

}  // namespace

struct align_handle {
  int kind = 0, gpu_index = 0;
  std::unique_ptr<Timer> timer;
  double kernel_ms = 0.0;  // of the running call
  // reprojection
  ap::ReprojLayout layout;
  int num_images = 0, num_waves = 0;
  std::vector<double> src_centers, tgt_centers;  // [num_images][3] projection centres: the samples of the search
  DeviceBuffer<double> d_rows;
  DeviceBuffer<int> d_wave_image, d_wave_count, d_image_wave_begin;
  DeviceBuffer<DevImage> d_images;
  DeviceBuffer<DevHypothesis> d_hyps;
  DeviceBuffer<unsigned> d_partial, d_inliers;
  // positions
  int64_t num_points = 0;
  int num_chunks = 0;
  std::vector<double> src, tgt;  // host copies: the estimator's samples
  DeviceBuffer<double> d_src, d_tgt, d_chunk_sum, d_residual_sum;
  DeviceBuffer<unsigned> d_chunk_count;
  DeviceBuffer<long long> d_num_inliers;
  DeviceBuffer<DevSim3> d_sims;
  DeviceBuffer<unsigned char> d_mask;
};

namespace {

void check_hypotheses(const double* sims, int B) {
  ALIGN_CHECK(B >= 0 && B <= ALIGN_MAX_BATCH, "num_hypotheses must lie in [0, ALIGN_MAX_BATCH]");
  ALIGN_CHECK(B == 0 || sims, "the hypotheses are null (8 doubles each)");
  for (int h = 0; h < B; ++h) ap::check_sim3(sims + 8 * (size_t)h, "hypothesis " + std::to_string(h));
}

// inliers: [B][num_images] host
void reproj_score(align_handle& H, const double* sims, int B, double max_reproj_error, uint32_t* inliers) {
  ALIGN_CHECK(max_reproj_error >= 0.0, "max_reproj_error must not be negative");
  const size_t I = (size_t)H.num_images;
  if (B == 0 || I == 0) return;
  ALIGN_HIP(hipSetDevice(H.gpu_index));
  std::vector<DevHypothesis> hyps((size_t)B);
  for (int h = 0; h < B; ++h) {
    double inv[8];
    ap::sim3_matrix(sims + 8 * (size_t)h, hyps[(size_t)h].tgt_from_src);
    ap::sim3_inverse(sims + 8 * (size_t)h, inv);
    ap::sim3_matrix(inv, hyps[(size_t)h].src_from_tgt);
  }
  H.d_hyps.reserve((size_t)B);
  ALIGN_HIP(hipMemcpy(H.d_hyps.p, hyps.data(), hyps.size() * sizeof(DevHypothesis), hipMemcpyHostToDevice));
  H.d_partial.reserve((size_t)B * (size_t)H.num_waves);
  H.d_inliers.reserve((size_t)B * I);
  H.timer->start();
  if (H.num_waves > 0) {
    const dim3 grid((unsigned)((H.num_waves + kWavesPerBlock - 1) / kWavesPerBlock), (unsigned)((B + kHypTile - 1) / kHypTile));
    hipLaunchKernelGGL(align_reproj_score_kernel, grid, dim3(kBlock), 0, 0, H.d_rows.p, (long long)H.layout.num_rows,
                       H.d_wave_image.p, H.d_wave_count.p, H.num_waves, H.d_images.p, H.d_hyps.p, B,
                       max_reproj_error * max_reproj_error, H.d_partial.p);
    ALIGN_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(align_reproj_reduce_kernel, dim3(blocks_for((size_t)B * I)), dim3(kBlock), 0, 0, H.d_partial.p,
                     H.num_waves, H.d_image_wave_begin.p, H.num_images, B, H.d_inliers.p);
  ALIGN_HIP(hipGetLastError());
  H.kernel_ms += H.timer->stop();
  H.d_inliers.download(inliers, (size_t)B * I);
}

void positions_score(align_handle& H, const double* sims, int B, double max_error, int64_t* num_inliers,
                     double* residual_sum, uint8_t* mask) {
  ALIGN_CHECK(max_error >= 0.0, "max_error must not be negative");
  if (B == 0) return;
  const size_t N = (size_t)H.num_points;
  if (N == 0) {
    for (int h = 0; h < B; ++h) {
      if (num_inliers) num_inliers[h] = 0;
      if (residual_sum) residual_sum[h] = 0.0;
    }
    return;
  }
  ALIGN_CHECK(!mask || (size_t)B * N < ((size_t)1 << 32), "num_hypotheses * num_points of an inlier mask must stay below 2^32");
  ALIGN_HIP(hipSetDevice(H.gpu_index));
  std::vector<DevSim3> dev((size_t)B);
  for (int h = 0; h < B; ++h) dev[(size_t)h] = dev_sim3(sims + 8 * (size_t)h);
  H.d_sims.reserve((size_t)B);
  ALIGN_HIP(hipMemcpy(H.d_sims.p, dev.data(), dev.size() * sizeof(DevSim3), hipMemcpyHostToDevice));
  H.d_chunk_sum.reserve((size_t)H.num_chunks * (size_t)B);
  H.d_chunk_count.reserve((size_t)H.num_chunks * (size_t)B);
  H.d_residual_sum.reserve((size_t)B);
  H.d_num_inliers.reserve((size_t)B);
  if (mask) H.d_mask.reserve((size_t)B * N);
  H.timer->start();
  const dim3 grid((unsigned)H.num_chunks, (unsigned)((B + kHypTile - 1) / kHypTile));
  hipLaunchKernelGGL(align_position_score_kernel, grid, dim3(kBlock), 0, 0, H.d_src.p, H.d_tgt.p, (int)N, H.d_sims.p, B,
                     max_error * max_error, H.d_chunk_sum.p, H.d_chunk_count.p, mask ? H.d_mask.p : nullptr);
  ALIGN_HIP(hipGetLastError());
  hipLaunchKernelGGL(align_position_reduce_kernel, dim3(blocks_for((size_t)B)), dim3(kBlock), 0, 0, H.d_chunk_sum.p,
                     H.d_chunk_count.p, H.num_chunks, B, H.d_residual_sum.p, H.d_num_inliers.p);
  ALIGN_HIP(hipGetLastError());
  H.kernel_ms += H.timer->stop();
  static_assert(sizeof(long long) == sizeof(int64_t), "counts are downloaded as they are");
  H.d_num_inliers.download((long long*)num_inliers, (size_t)B);
  H.d_residual_sum.download(residual_sum, (size_t)B);
  if (mask) H.d_mask.download(mask, (size_t)B * N);
}

// the problems the search loop of align_plan.h runs on

struct ReprojProblem {
  align_handle& H;
  double max_reproj_error, max_residual;
  std::vector<uint32_t> counts;

  size_t num_samples() const { return (size_t)H.num_images; }
  bool estimate(const size_t* idx, size_t n, double sim[8]) {
    return ap::estimate_sim3(H.src_centers.data(), H.tgt_centers.data(), idx, n, sim);
  }
  // InlierSupportMeasurer::Evaluate over the images, in image order
  ap::Support evaluate(const uint32_t* inliers, std::vector<uint8_t>* mask) const {
    ap::Support s;
    s.num_inliers = 0;
    s.residual_sum = 0.0;
    if (mask) mask->assign((size_t)H.num_images, 0);
    for (int i = 0; i < H.num_images; ++i) {
      const double r = ap::reproj_residual(inliers[i], H.layout.common[(size_t)i]);
      if (r <= max_residual) {
        ++s.num_inliers;
        s.residual_sum += r;
        if (mask) (*mask)[(size_t)i] = 1;
      }
    }
    return s;
  }
  void score(const double* sims, int B, ap::Support* supports) {
    counts.resize((size_t)B * (size_t)H.num_images);
    reproj_score(H, sims, B, max_reproj_error, counts.data());
    for (int h = 0; h < B; ++h) supports[h] = evaluate(counts.data() + (size_t)h * (size_t)H.num_images, nullptr);
  }
  void inliers(const double sim[8], std::vector<uint8_t>* mask, ap::Support* s) {
    counts.resize((size_t)H.num_images);
    reproj_score(H, sim, 1, max_reproj_error, counts.data());
    *s = evaluate(counts.data(), mask);
  }
};

struct PositionsProblem {
  align_handle& H;
  double max_error;
  std::vector<int64_t> n;
  std::vector<double> sum;

  size_t num_samples() const { return (size_t)H.num_points; }
  bool estimate(const size_t* idx, size_t count, double sim[8]) {
    return ap::estimate_sim3(H.src.data(), H.tgt.data(), idx, count, sim);
  }
  void score(const double* sims, int B, ap::Support* supports) {
    n.resize((size_t)B);
    sum.resize((size_t)B);
    positions_score(H, sims, B, max_error, n.data(), sum.data(), nullptr);
    for (int h = 0; h < B; ++h) {
      supports[h].num_inliers = (uint64_t)n[(size_t)h];
      supports[h].residual_sum = sum[(size_t)h];
    }
  }
  void inliers(const double sim[8], std::vector<uint8_t>* mask, ap::Support* s) {
    int64_t count = 0;
    double total = 0.0;
    mask->assign((size_t)H.num_points, 0);
    positions_score(H, sim, 1, max_error, &count, &total, mask->data());
    s->num_inliers = (uint64_t)count;
    s->residual_sum = total;
  }
};

void fill_report(const ap::Report& r, align_report* out) {
  out->success = r.success ? 1 : 0;
  out->num_trials = (int64_t)r.num_trials;
  out->num_inliers = (int64_t)r.support.num_inliers;
  out->residual_sum = r.support.residual_sum;
  for (int k = 0; k < 8; ++k) out->model[k] = r.model[(size_t)k];
  if (out->inlier_mask && !r.inlier_mask.empty()) std::memcpy(out->inlier_mask, r.inlier_mask.data(), r.inlier_mask.size());
  out->num_scored = (int64_t)r.num_scored;
  out->num_launches = (int64_t)r.num_launches;
}

struct CallClock {  // kernel and total time of one ABI call
  align_handle* H;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit CallClock(align_handle* h) : H(h) {
    if (H) H->kernel_ms = 0.0;
  }
  void done() {
    g_kernel_ms = H ? H->kernel_ms : 0.0;
    g_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
};

}  // namespace

extern "C" {

ALIGN_API void align_options_init(align_options* o) {
  o->max_error = 8.0;
  o->min_inlier_observations = 0.3;
  o->min_inlier_ratio = 0.1;
  o->confidence = 0.99;
  o->dyn_num_trials_multiplier = 3.0;
  o->min_num_trials = 0;
  o->max_num_trials = INT32_MAX;
  o->random_seed = 0;
  o->batch_size = 0;
}

ALIGN_API int align_reproj_create(const align_reproj_pair* pair, int32_t gpu_index, align_handle** handle) {
  return Guard([&] {
    if (!pair || !handle) throw Fail("null argument");
    *handle = nullptr;
    ap::validate(*pair);
    bind_device(gpu_index);
    CallClock clock(nullptr);
    std::unique_ptr<align_handle> H(new align_handle);
    H->kind = KIND_REPROJ;
    H->gpu_index = gpu_index;
    H->timer.reset(new Timer);
    H->layout = ap::make_layout(*pair);
    H->num_images = pair->num_images;
    H->num_waves = (int)H->layout.wave_image.size();
    const size_t I = (size_t)pair->num_images, rows = (size_t)H->layout.num_rows;
    H->src_centers.resize(3 * I);
    H->tgt_centers.resize(3 * I);
    std::vector<DevImage> images(I);
    for (size_t i = 0; i < I; ++i) {
      const auto cs = ap::projection_center(pair->src_poses + 7 * i), ct = ap::projection_center(pair->tgt_poses + 7 * i);
      for (int k = 0; k < 3; ++k) {
        H->src_centers[3 * i + k] = cs[(size_t)k];
        H->tgt_centers[3 * i + k] = ct[(size_t)k];
      }
      pose_matrix(pair->src_poses + 7 * i, images[i].src_pose);
      pose_matrix(pair->tgt_poses + 7 * i, images[i].tgt_pose);
      images[i].src_cam = dev_camera(pair->src_cameras[i]);
      images[i].tgt_cam = dev_camera(pair->tgt_cameras[i]);
    }
    std::vector<double> soa((size_t)kRecordDoubles * rows, 0.0);
    for (size_t r = 0; r < rows; ++r) {
      const int32_t o = H->layout.order[r];
      if (o < 0) continue;
      for (int c = 0; c < 3; ++c) {
        soa[(size_t)c * rows + r] = pair->rec_src_xyz[3 * (size_t)o + c];
        soa[(size_t)(3 + c) * rows + r] = pair->rec_tgt_xyz[3 * (size_t)o + c];
      }
      for (int c = 0; c < 2; ++c) {
        soa[(size_t)(6 + c) * rows + r] = pair->rec_src_xy[2 * (size_t)o + c];
        soa[(size_t)(8 + c) * rows + r] = pair->rec_tgt_xy[2 * (size_t)o + c];
      }
    }
    H->d_rows.upload(soa.data(), soa.size());
    H->d_wave_image.upload(H->layout.wave_image.data(), H->layout.wave_image.size());
    H->d_wave_count.upload(H->layout.wave_count.data(), H->layout.wave_count.size());
    H->d_image_wave_begin.upload(H->layout.image_wave_begin.data(), H->layout.image_wave_begin.size());
    H->d_images.upload(images.data(), images.size());
    clock.done();
    *handle = H.release();
  });
}

ALIGN_API int align_reproj_score(align_handle* handle, const double* tgt_from_src, int32_t num_hypotheses,
                                 double max_reproj_error, uint32_t* inliers, uint32_t* common) {
  return Guard([&] {
    if (!handle || handle->kind != KIND_REPROJ) throw Fail("not a handle of align_reproj_create");
    check_hypotheses(tgt_from_src, num_hypotheses);
    ALIGN_CHECK(max_reproj_error >= 0.0, "max_reproj_error must not be negative");
    CallClock clock(handle);
    if (common && handle->num_images) std::memcpy(common, handle->layout.common.data(), (size_t)handle->num_images * sizeof(uint32_t));
    if (inliers) reproj_score(*handle, tgt_from_src, num_hypotheses, max_reproj_error, inliers);
    clock.done();
  });
}

ALIGN_API int align_reproj_estimate(align_handle* handle, const align_options* options, align_report* report) {
  return Guard([&] {
    if (!handle || handle->kind != KIND_REPROJ) throw Fail("not a handle of align_reproj_create");
    if (!options || !report) throw Fail("null argument");
    ap::validate_options(*options, true);
    CallClock clock(handle);
    // alignment.cc:310-311: ransac_options.max_error = 1 - min_inlier_observations, squared by LORANSAC (loransac.h:146)
    const double max_error = 1.0 - options->min_inlier_observations;
    ReprojProblem problem{*handle, options->max_error, max_error * max_error, {}};
    fill_report(ap::loransac(problem, *options), report);
    clock.done();
  });
}

ALIGN_API int align_positions_create(const double* src, const double* tgt, int64_t num_points, int32_t gpu_index,
                                     align_handle** handle) {
  return Guard([&] {
    if (!handle) throw Fail("null argument");
    *handle = nullptr;
    ap::validate_positions(src, tgt, num_points);
    bind_device(gpu_index);
    CallClock clock(nullptr);
    std::unique_ptr<align_handle> H(new align_handle);
    H->kind = KIND_POSITIONS;
    H->gpu_index = gpu_index;
    H->timer.reset(new Timer);
    H->num_points = num_points;
    H->num_chunks = (int)((num_points + kChunk - 1) / kChunk);
    H->src.assign(src, src + 3 * (size_t)num_points);
    H->tgt.assign(tgt, tgt + 3 * (size_t)num_points);
    H->d_src.upload(src, 3 * (size_t)num_points);
    H->d_tgt.upload(tgt, 3 * (size_t)num_points);
    clock.done();
    *handle = H.release();
  });
}

ALIGN_API int align_positions_score(align_handle* handle, const double* tgt_from_src, int32_t num_hypotheses, double max_error,
                                    int64_t* num_inliers, double* residual_sum, uint8_t* inlier_mask) {
  return Guard([&] {
    if (!handle || handle->kind != KIND_POSITIONS) throw Fail("not a handle of align_positions_create");
    check_hypotheses(tgt_from_src, num_hypotheses);
    ALIGN_CHECK(max_error >= 0.0, "max_error must not be negative");
    ALIGN_CHECK(num_hypotheses == 0 || (num_inliers && residual_sum), "num_inliers and residual_sum are null");
    CallClock clock(handle);
    positions_score(*handle, tgt_from_src, num_hypotheses, max_error, num_inliers, residual_sum, inlier_mask);
    clock.done();
  });
}

ALIGN_API int align_positions_estimate(align_handle* handle, const align_options* options, align_report* report) {
  return Guard([&] {
    if (!handle || handle->kind != KIND_POSITIONS) throw Fail("not a handle of align_positions_create");
    if (!options || !report) throw Fail("null argument");
    ap::validate_options(*options, false);
    CallClock clock(handle);
    PositionsProblem problem{*handle, options->max_error, {}, {}};
    fill_report(ap::loransac(problem, *options), report);
    clock.done();
  });
}

ALIGN_API void align_destroy(align_handle* handle) { delete handle; }

ALIGN_API int align_hypothesis_tile(void) { return kHypTile; }

ALIGN_API int align_transform_points(double* points, int64_t num_points, const double new_from_old[8], int32_t gpu_index) {
  return Guard([&] {
    ALIGN_CHECK(num_points >= 0, "num_points must not be negative");
    ALIGN_CHECK(num_points < ((int64_t)1 << 31), "num_points must fit a 32-bit index");
    ALIGN_CHECK(num_points == 0 || points, "points is null");
    ALIGN_CHECK(new_from_old != nullptr, "the transform is null (8 doubles)");
    ap::check_sim3(new_from_old, "the transform");
    const auto t0 = std::chrono::steady_clock::now();
    g_kernel_ms = 0.0;
    if (num_points > 0) {
      bind_device(gpu_index);
      DeviceBuffer<double> d;
      d.upload(points, 3 * (size_t)num_points);
      Timer timer;
      timer.start();
      hipLaunchKernelGGL(align_transform_points_kernel, dim3(blocks_for((size_t)num_points)), dim3(kBlock), 0, 0, d.p,
                         (long long)num_points, dev_sim3(new_from_old));
      ALIGN_HIP(hipGetLastError());
      g_kernel_ms = timer.stop();
      d.download(points, 3 * (size_t)num_points);
    }
    g_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  });
}

ALIGN_API void align_last_timing(double* kernel_ms, double* total_ms) {
  if (kernel_ms) *kernel_ms = g_kernel_ms;
  if (total_ms) *total_ms = g_total_ms;
}

ALIGN_API const char* align_last_error(void) { return g_error.c_str(); }

}  // extern "C"
