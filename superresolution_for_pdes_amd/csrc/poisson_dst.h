// The sine-transform solve of poisson_dst.hip as other translation units launch it (poisson_div.hip: the
// preconditioner of the divergence-form CG).  The public entries check their arguments and call the same function.
#pragma once
#include "common.h"

namespace srpde {

// u = L^-1 (f / theta) for B problems [B][n][n] fp64, 2 <= n <= 16384; theta == nullptr: u = L^-1 f, no division and
// no field of ones.  plan: S [n][n] then lam [n] (srpde_poisson_dst_plan); ws: srpde_poisson_dst_workspace_size(B, n)
// bytes, unused up to srpde_poisson_dst_lds_max_n().  The caller has checked every argument.  One launch up to that
// n, four above it (u must not alias f there); `name` labels a launch error.
//
// sigma > 0 (finite, theta == nullptr only): u = (L - sigma I)^-1 f.  The eigenvalue scaling h^2 / (lam_i + lam_j)
// becomes 1 / ((lam_i + lam_j) * inv_h2 - sigma), each operation rounded once in this order with no contraction: the
// sum lam_i + lam_j, times inv_h2 = (n - 1)^2, minus sigma, the reciprocal, then the product with the transformed
// field -- applied where the unshifted scaling is (the LDS kernel's second product, the second launch's store above
// the LDS limit).  sigma = 0 launches the unshifted kernels with their arguments: today's bits.
int dst_solve_launch(const char* name, const double* f, const double* theta, double* u, int B, int n, const void* plan,
                     void* ws, hipStream_t stream, double sigma = 0.0);

size_t dst_plan_bytes_for(int n);

// The separable solve with mixed sides: u = (L_bc - sigma I)^-1 f for B problems [B][n][n] fp64, sigma >= 0 (> 0 when
// all four sides are zero-flux), the sides in the plan (srpde_poisson_sep_plan for n and the mask); ws: one [B][n][n]
// field at every n.  Four launches; u must not alias f.  The caller has checked every argument.
int sep_solve_launch(const char* name, const double* f, double* u, int B, int n, const void* plan, void* ws,
                     hipStream_t stream, double sigma);

size_t sep_plan_bytes_for(int n, int bc);

}  // namespace srpde
