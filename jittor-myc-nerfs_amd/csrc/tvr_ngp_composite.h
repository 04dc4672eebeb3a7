// tvr_ngp_composite.h — the per-sample arithmetic of compute_rgbs (calc_rgb.h:2-4, restated in oracle/ngp_oracle.c: ngp_oracle_composite), shared by
// the inference compositor (tvr_ngp.hip: ngp_composite_kernel) and the training compositor and its backward (tvr_ngp_train.hip), so that the three
// walk a ray with the same roundings: fp32, every operation rounded on its own (-ffp-contract=off), the exponentials the hardware's (__expf).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float min_cone_step() { return 1.73205080757f / 1024.0f; }

// the row's dt as the compositor sees it: column 3 of the sampler's row, unwarped
__device__ __forceinline__ float ngp_row_dt(float warped)
{
    const float max_step = min_cone_step() * 16.0f;
    return warped * (max_step - min_cone_step()) + min_cone_step();
}
// alpha = 1 - exp(-sigma dt) with sigma = exp(raw density)
__device__ __forceinline__ float ngp_alpha(float raw, float dt) { return 1.f - __expf(-__expf(raw) * dt); }
// the colour activation
__device__ __forceinline__ float ngp_logistic(float v) { return 1.0f / (1.0f + __expf(-v)); }
