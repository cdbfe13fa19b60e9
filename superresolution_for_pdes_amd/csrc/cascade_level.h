// The statistics and assemble passes of one cascade level as cascade.hip (disjoint tiles, statistics from the next
// level's ground truth) and tiled.hip (overlapping windows, statistics from the level's inputs) both launch them.
// The kernels and the launchers are defined once, in cascade.hip; the public entries check their arguments and
// call them.
#pragma once
#include "common.h"

namespace srpde {

// GlobalNormalization's statistics row and theta-constant flag of E examples: the u columns from u [E][n_u], the
// f / theta columns from f, th [E][n_f].  Every field is reduced over red_blocks(its length) workgroups, so a row
// does not depend on what the other field's length is.  part: E * 3 * red_blocks(n_f) * 2 doubles.  Two launches,
// grid (red_blocks(n_f), 3, E) then E.  The caller has checked every argument; `name` labels a launch error.
int level_stats_launch(const char* name, const double* u, const double* f, const double* th, long long n_u,
                       long long n_f, int E, float* stats, int* theta_const, double* part, hipStream_t stream);

// The U-Net input x [E m^2][3][2 tile][2 tile] of the m x m windows per example whose origin on the coarse grid is
// min(k * stride, S - tile) on either axis (stride == tile, m == S / tile: the disjoint tiles).  One launch.
int level_assemble_launch(const char* name, const double* u_cur, const double* f_next, const double* th_next,
                          const float* stats, int E, int S, int tile, int stride, int m, float* x, hipStream_t stream);

// v * std + mean as an fp32 multiply, then an fp32 add (two roundings, as torch's y * std + mean)
__device__ __forceinline__ float denorm(float v, float std, float mean) {
#pragma clang fp contract(off)
  float r = v * std;
  r = r + mean;
  return r;
}

}  // namespace srpde
