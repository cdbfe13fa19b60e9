// The face coefficients of the divergence-form operator  D_theta u = div(theta grad u)  and its face sum, float or
// double (poisson_div.hip: the operator and its CG; relax.hip: its smoother; physics.hip: its loss term), and the
// coefficients' derivative in theta_a with its face sum, the operator's gradient in theta (poisson_div.hip).  At the end:
// what boundary data (values beyond Dirichlet sides, fluxes through zero-flux sides) puts into a halo and onto a node.
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
// has_*: that neighbour is a node of the grid; ghost_*: the ghost face on that side of the GRID exists (a Dirichlet
// side; a zero-flux side has none).  A face to a missing neighbour has coefficient ta where its ghost face exists and 0
// where it does not, in the same place of the same sum.  The halo holds 0 outside the grid, so a missing face's term
// is 0 * (0 - v) = -+0, which changes no sum but an all-zero one's sign.
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

// the zero ghost ring: all four ghost faces exist
template <bool HARM, typename T>
__device__ __forceinline__ T face_sum(const T* v, const T* th, int pitch, bool has_w, bool has_e, bool has_n,
                                      bool has_s) {
  return face_sum_bc<HARM>(v, th, pitch, has_w, has_e, has_n, has_s, true, true, true, true);
}

// d face_mean(ta, tb) / d ta: 0.5, or 2 tb^2 / (ta + tb)^2 (towards the ghost ring c = ta and the derivative is 1)
template <bool HARM, typename T>
__device__ __forceinline__ T face_mean_da(T ta, T tb) {
  return HARM ? (T(2) * (tb * tb)) / ((ta + tb) * (ta + tb)) : T(0.5);
}

// The pair gradient of the operator in theta_a, sum over the node's faces of dc/dta (vb - va) (wb - wa), as
// (gE + gW) + (gS + gN) with a face term g = (d * (vb - va)) * (wb - wa); tiles, has_* and ghost_* as for face_sum_bc:
// towards a missing neighbour the derivative is 1 where the ghost face exists and 0 where it does not.  The halo holds
// 0 for v and w outside the grid, so a ghost face gives (1 * (0 - va)) * (0 - wa) = va * wa exactly.
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

// the zero ghost ring: all four ghost faces exist
template <bool HARM, typename T>
__device__ __forceinline__ T face_grad_sum(const T* v, const T* w, const T* th, int pitch, bool has_w, bool has_e,
                                           bool has_n, bool has_s) {
  return face_grad_sum_bc<HARM>(v, w, th, pitch, has_w, has_e, has_n, has_s, true, true, true, true);
}

// ---- Boundary data (the *_bd entries).  bd is one problem's [4][n] doubles, the sides in the mask's order: row 0,
// row n - 1, column 0, column n - 1; entry k of a row side belongs to column k, of a column side to row k.  On a
// Dirichlet side (bit clear) it is the ghost value g beyond the edge node, on a zero-flux side (bit set) the outward
// flux q through the face half a cell beyond it.

// What the halo holds at the out-of-grid position (gy, gx): g where it lies straight beyond an edge node of a Dirichlet
// side, 0.0 everywhere else (beyond a flux side, in the halo's corners, past a ragged tile's grid edge).  Called for
// out-of-grid positions only, so no in-grid halo entry pays for a load of bd.
__device__ __forceinline__ double bd_halo(const double* __restrict__ bd, int gy, int gx, int n, int bc) {
  const bool col = gx >= 0 && gx < n, row = gy >= 0 && gy < n;
  if (col && gy == -1 && !(bc & 1)) return bd[gx];
  if (col && gy == n && !(bc & 2)) return bd[n + gx];
  if (row && gx == -1 && !(bc & 4)) return bd[2 * n + gy];
  if (row && gx == n && !(bc & 8)) return bd[3 * n + gy];
  return 0.0;
}

// node (gy, gx) has at least one ghost face on a flux side
__device__ __forceinline__ bool bd_flux_node(int gy, int gx, int n, int bc) {
  return (gy == 0 && (bc & 1)) || (gy == n - 1 && (bc & 2)) || (gx == 0 && (bc & 4)) || (gx == n - 1 && (bc & 8));
}

// (qE + qW) + (qS + qN) of such a node, an absent term 0.0
__device__ __forceinline__ double bd_flux_sum(const double* __restrict__ bd, int gy, int gx, int n, int bc) {
  const double qN = (gy == 0 && (bc & 1)) ? bd[gx] : 0.0;
  const double qS = (gy == n - 1 && (bc & 2)) ? bd[n + gx] : 0.0;
  const double qW = (gx == 0 && (bc & 4)) ? bd[2 * n + gy] : 0.0;
  const double qE = (gx == n - 1 && (bc & 8)) ? bd[3 * n + gy] : 0.0;
  return (qE + qW) + (qS + qN);
}

// face_sum_bc of the field that is 0.0 on the grid and v's halo outside it: the ghost faces' terms c * (g - 0.0) = c * g
// in their places, 0.0 for a face to a grid node.  With * inv_h2 and the flux term it is b = A_bd 0 of the stop rule.
template <typename T>
__device__ __forceinline__ T face_ghost_sum(const T* v, const T* th, int pitch, bool has_w, bool has_e, bool has_n,
                                            bool has_s, bool ghost_w, bool ghost_e, bool ghost_n, bool ghost_s) {
  const T ta = th[0];
  const T tE = has_e ? T(0) : (ghost_e ? ta : T(0)) * v[1];
  const T tW = has_w ? T(0) : (ghost_w ? ta : T(0)) * v[-1];
  const T tS = has_s ? T(0) : (ghost_s ? ta : T(0)) * v[pitch];
  const T tN = has_n ? T(0) : (ghost_n ? ta : T(0)) * v[-pitch];
  return (tE + tW) + (tS + tN);
}

}  // namespace srpde
