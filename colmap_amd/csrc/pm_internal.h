// Internal interface between the C-ABI host code (pm_api.cpp) and the gfx950
// kernels (pm_kernels.hip). Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pm_host_plan.h"  // PmParams, the packed-image layout, and what the host decides before any device call
#include "switches.h"

// PmParams::ablate (skip phases of the sweep to time the rest: results are garbage) is only ever non-zero in a
// profiling build (-DCOLMAP_AMD_DIAG_BUILD: pm_api.cpp sets it from a development switch); the kernels keep their three
// scalar tests on it so that the shipped instruction stream is the profiled one.
#define PM_ABLATE(p) ((p).ablate)

namespace colmap_amd {

constexpr int kPmProfSlots = 24; // phase-profile counters per handle (pm_kernels.hip: kProf*, written by pm_sweep_quad_prof_kernel only)

// floats per pixel of PmParams::draws: perturbed depth, perturbed normal, M uniforms (whole float4s)
__host__ __device__ inline int pm_draw_stride(int M) { return 4 + ((M + 3) & ~3); }
// `requested` > 0: the caller's columns per group (PatchMatchOptions::columns_per_group or the development switch)
int pm_pick_columns(int S, int ntaps, int num_samples, bool geom, int radius, int requested);
// dynamic LDS bytes of a four-wave workgroup of the 11 x 11 wave kernels at C columns per wave (pm_debug_wave_lds_bytes)
size_t pm_quad_lds_bytes(int S, int num_samples, int C, bool geom);

// Which kernels a run launches, decided ONCE per run (pm_plan_run) from the common shape of its problems; the launchers
// below only launch what the plan states. Two families, one arithmetic: the 11 x 11 wave kernels (quad; pair = a helper
// wave per column group; quad-prof = the quad kernel with its phase clocks) and the generic kernel of any window.
enum PmFamily { kPmGeneric, kPmQuad, kPmPair, kPmQuadProf };
struct PmRunPlan {
  PmFamily initial_cost;    // kPmGeneric or kPmQuad
  PmFamily sweep;
  bool fp_resource;         // wave kernels: packed images through the problem's buffer resource (else explicit indices).
                            // One flag for the initial cost and every sweep; false = every parameter block of the run
                            // carries fp_base = null (RunBatchAsync)
  bool geom;
  int W, H, C;              // grid geometry: un-rotated image size, columns per group
  int initial_cost_block, sweep_block;     // threads per workgroup
  size_t initial_cost_lds, sweep_lds;      // dynamic LDS bytes
  const char* sweep_name;   // what pm_get_sweep_kernel_name reports

  // The one shape test of the plan: do the 11 x 11 wave kernels serve this shape (window, source count and the
  // four-wave workgroup's LDS budget at C columns per wave)? They read the sweep's random numbers from PmParams::draws:
  // pm_create asks with C = 1, the narrowest shape a run may choose, whether to allocate them.
  static bool wave_kernels_fit(const PmParams& shape, int C, bool geom);
};
// `shape`: the parameter block of any problem of the run, with the run's C and help; `threads`: workgroup size of the
// generic sweep kernel; fp_base_all: every handle of the batch has a buffer-resource base; draws: PmParams::draws is
// allocated. The only reader of COLMAP_AMD_PM_WAVE and COLMAP_AMD_PM_FP_GLOBAL.
PmRunPlan pm_plan_run(const PmParams& shape, bool geom, int threads, bool fp_base_all, bool profile, bool draws);

void pm_launch_build_footprint(const uint8_t* src, uint32_t* fp, int S, int w, int h, hipStream_t st);
void pm_launch_filter_ref(const uint8_t* gray, int W, int H, int radius, int step, float sigma_spatial,
                          float sigma_color, uint8_t* out_img, float* out_sum, float* out_sqsum,
                          hipStream_t st);
void pm_launch_init_state(const PmParams& p, bool random_init, float depth_min, float depth_max,
                          const float* init_depth, const float* init_normal, hipStream_t st);
// `dev_params` is the device array of per-problem parameter blocks the kernel indexes with its batch coordinate.
void pm_launch_initial_cost(const PmRunPlan& plan, const PmParams* dev_params, int batch, hipStream_t st);
// the random numbers of the next sweep launch (wave kernels; no-op when the generic kernel sweeps, it draws in place):
// call before pm_launch_sweep with the same arguments; `rot` = the sweep's direction (PmParams::rot)
void pm_launch_draws(const PmRunPlan& plan, int rot, const PmParams* dev_params, int batch, hipStream_t st);
void pm_launch_sweep(const PmRunPlan& plan, int rot, const PmParams* dev_params, int batch, bool filter_photo,
                     bool filter_geom, hipStream_t st);
void pm_launch_rng_streams(const unsigned long long* seeds, int nseeds, int ndraws, float* out,
                           hipStream_t st);
void pm_launch_extract(const PmParams& p, int sel_off, float* depth, float* normal, float* sel,
                       float* cost, hipStream_t st);

}  // namespace colmap_amd
