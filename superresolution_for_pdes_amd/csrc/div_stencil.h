// The face coefficients of the divergence-form operator  D_theta u = div(theta grad u)  and its face sum, float or
// double (poisson_div.hip: the operator and its CG; relax.hip: its smoother; physics.hip: its loss term), and the
// coefficients' derivative in theta_a with its face sum, the operator's gradient in theta (poisson_div.hip).
//
// For node a with nodal theta_a and neighbour b the face coefficient is
//     arithmetic (HARM false):  c = 0.5 * (ta + tb)
//     harmonic   (HARM true):   c = (2.0 * (ta * tb)) / (ta + tb)
//     b outside the grid:       c = ta, and the value there is 0
// Both means are bit-symmetric in (a, b).  The order of the operations below defines the operator's bits.  The header
// does not set the contraction mode: its functions take the mode in force where it is included, so a file that turns
// contraction off for itself (poisson_div.hip, relax.hip: one rounding per operation) includes it after its pragma.
#pragma once

namespace srpde {

template <bool HARM, typename T>
__device__ __forceinline__ T face_mean(T ta, T tb) {
  return HARM ? (T(2) * (ta * tb)) / (ta + tb) : T(0.5) * (ta + tb);
}

// (cE (vE - v) + cW (vW - v)) + (cS (vS - v) + cN (vN - v)) on halo tiles around v and th (E is +1, S is +pitch);
// has_*: that neighbour is a node of the grid
template <bool HARM, typename T>
__device__ __forceinline__ T face_sum(const T* v, const T* th, int pitch, bool has_w, bool has_e, bool has_n,
                                      bool has_s) {
  const T ta = th[0], vc = v[0];
  const T cE = has_e ? face_mean<HARM>(ta, th[1]) : ta;
  const T cW = has_w ? face_mean<HARM>(ta, th[-1]) : ta;
  const T cS = has_s ? face_mean<HARM>(ta, th[pitch]) : ta;
  const T cN = has_n ? face_mean<HARM>(ta, th[-pitch]) : ta;
  return (cE * (v[1] - vc) + cW * (v[-1] - vc)) + (cS * (v[pitch] - vc) + cN * (v[-pitch] - vc));
}

// face_sum with a boundary pattern: ghost_*: the ghost face on that side of the GRID exists (a Dirichlet side; a
// zero-flux side has none).  A missing ghost face has coefficient 0 where face_sum has ta, every other operation and
// its place are face_sum's: four Dirichlet sides give face_sum's bits.  The halo holds 0 outside the grid, so a
// missing face's term is 0 * (0 - v) = -+0, which changes no sum but an all-zero one's sign.
template <bool HARM, typename T>
__device__ __forceinline__ T face_sum_bc(const T* v, const T* th, int pitch, bool has_w, bool has_e, bool has_n,
                                         bool has_s, bool ghost_w, bool ghost_e, bool ghost_n, bool ghost_s) {
  const T ta = th[0], vc = v[0];
  const T cE = has_e ? face_mean<HARM>(ta, th[1]) : (ghost_e ? ta : T(0));
  const T cW = has_w ? face_mean<HARM>(ta, th[-1]) : (ghost_w ? ta : T(0));
  const T cS = has_s ? face_mean<HARM>(ta, th[pitch]) : (ghost_s ? ta : T(0));
  const T cN = has_n ? face_mean<HARM>(ta, th[-pitch]) : (ghost_n ? ta : T(0));
  return (cE * (v[1] - vc) + cW * (v[-1] - vc)) + (cS * (v[pitch] - vc) + cN * (v[-pitch] - vc));
}

// d face_mean(ta, tb) / d ta: 0.5, or 2 tb^2 / (ta + tb)^2 (towards the ghost ring c = ta and the derivative is 1)
template <bool HARM, typename T>
__device__ __forceinline__ T face_mean_da(T ta, T tb) {
  return HARM ? (T(2) * (tb * tb)) / ((ta + tb) * (ta + tb)) : T(0.5);
}

// The pair gradient of the operator in theta_a, sum over the node's faces of dc/dta (vb - va) (wb - wa), as
// (gE + gW) + (gS + gN) with a face term g = (d * (vb - va)) * (wb - wa); tiles and has_* as for face_sum.  The halo
// holds 0 for v and w outside the grid, so a ghost face gives (1 * (0 - va)) * (0 - wa) = va * wa exactly.
template <bool HARM, typename T>
__device__ __forceinline__ T face_grad_sum(const T* v, const T* w, const T* th, int pitch, bool has_w, bool has_e,
                                           bool has_n, bool has_s) {
  const T ta = th[0], vc = v[0], wc = w[0];
  const T dE = has_e ? face_mean_da<HARM>(ta, th[1]) : T(1);
  const T dW = has_w ? face_mean_da<HARM>(ta, th[-1]) : T(1);
  const T dS = has_s ? face_mean_da<HARM>(ta, th[pitch]) : T(1);
  const T dN = has_n ? face_mean_da<HARM>(ta, th[-pitch]) : T(1);
  return ((dE * (v[1] - vc)) * (w[1] - wc) + (dW * (v[-1] - vc)) * (w[-1] - wc)) +
         ((dS * (v[pitch] - vc)) * (w[pitch] - wc) + (dN * (v[-pitch] - vc)) * (w[-pitch] - wc));
}

// face_grad_sum with a boundary pattern (ghost_* as for face_sum_bc): a missing ghost face has derivative 0 where
// face_grad_sum has 1, every other operation and its place are face_grad_sum's.
template <bool HARM, typename T>
__device__ __forceinline__ T face_grad_sum_bc(const T* v, const T* w, const T* th, int pitch, bool has_w, bool has_e,
                                              bool has_n, bool has_s, bool ghost_w, bool ghost_e, bool ghost_n,
                                              bool ghost_s) {
  const T ta = th[0], vc = v[0], wc = w[0];
  const T dE = has_e ? face_mean_da<HARM>(ta, th[1]) : (ghost_e ? T(1) : T(0));
  const T dW = has_w ? face_mean_da<HARM>(ta, th[-1]) : (ghost_w ? T(1) : T(0));
  const T dS = has_s ? face_mean_da<HARM>(ta, th[pitch]) : (ghost_s ? T(1) : T(0));
  const T dN = has_n ? face_mean_da<HARM>(ta, th[-pitch]) : (ghost_n ? T(1) : T(0));
  return ((dE * (v[1] - vc)) * (w[1] - wc) + (dW * (v[-1] - vc)) * (w[-1] - wc)) +
         ((dS * (v[pitch] - vc)) * (w[pitch] - wc) + (dN * (v[-pitch] - vc)) * (w[-pitch] - wc));
}

}  // namespace srpde
