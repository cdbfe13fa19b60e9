// The temporal-blocking geometry shared by the two weighted-Jacobi smoothers (relax.hip: theta * L u = f,
// relax_div.hip: div(theta grad u) = f), so that srpde_pde_relax_sweeps_per_launch() answers for both.
#pragma once
#include <cstdint>

namespace srpde {

constexpr int kRelaxT = 48;                            // output tile
constexpr int kRelaxK = 8;                             // sweeps per launch = halo width
constexpr int kRelaxP = kRelaxT + 2 * kRelaxK;         // patch side
constexpr int kRelaxWaves = 8;
constexpr int kRelaxThreads = 64 * kRelaxWaves;
constexpr int kRelaxR = kRelaxP / kRelaxWaves;         // rows per thread
static_assert(kRelaxP == 64, "one patch column per lane");
static_assert(kRelaxR * kRelaxWaves == kRelaxP && kRelaxR <= 32, "the waves' strips tile the patch");
constexpr int kRelaxMaxN = 16384;

inline bool relax_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
  return p < q + bytes && q < p + bytes;
}

}  // namespace srpde
