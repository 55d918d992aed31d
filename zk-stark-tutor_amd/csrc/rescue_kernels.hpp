// Batched Rescue-Prime on the device (rescue_kernels.hip): one lane per input.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "fe128.hpp"

namespace sg {

constexpr int kRescueBatchMinM = 2, kRescueBatchMaxM = 4;  // state sizes with a kernel instantiation
constexpr unsigned kRescueBatchBlock = 64;                 // one wave per block

// rescue_prime.rs:185-204 for n inputs (canonical, device): trace = false writes out[i] = hash(in[i]);
// trace = true writes the (N + 1) x m trace of input i at out + i (N + 1) m.  consts (device,
// Montgomery): the m x m MDS matrix row-major, then the 2 m N round constants.  m outside
// [kRescueBatchMinM, kRescueBatchMaxM] is hipErrorInvalidValue.
hipError_t launch_rescue_batch(int m, bool trace, const fe* in, uint64_t n, uint32_t N, const fe* consts, fe* out,
                               const fe& r2, hipStream_t s);

}  // namespace sg
