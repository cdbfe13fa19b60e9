// The face coefficients of the divergence-form operator  D_theta u = div(theta grad u)  and its face sum, float or
// double (poisson_div.hip: the operator and its CG; relax.hip: its smoother; physics.hip: its loss term).
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

}  // namespace srpde
