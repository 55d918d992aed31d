// Batched Rescue-Prime (rescue_prime.rs:52-103, 185-204): many independent hashes / traces, one
// lane each.  One hash is a serial chain of N m inverse S-boxes, each a 128-bit exponentiation, so
// a single input stays on the host (sg_rescue_hash); a batch -- RPSSS key generation, trace
// preparation for many signers -- is compute-bound work with no data sharing: no LDS, no barriers,
// the state in registers in Montgomery form, the constants read through lane-uniform addresses.
//
// Products (mont_mul) per hash: N (m (2 + 141) + 2 m^2) + 2 = N m (143 + 2m) + 2 -- the cube, the
// alpha_inv chain of rescue_pow.hpp, two MDS products, and the conversion of the input and the
// output; 7 940 at m = 2, N = 27.  A trace adds m conversions per row.
//
// Launch: one-wave blocks.  A lane's chain has a fixed latency, so throughput comes from the
// number of resident waves alone, and 64-lane blocks let a batch of w waves spread over w SIMDs.
#include <hip/hip_runtime.h>

#include "dev_util.hpp"
#include "profiler.hpp"
#include "rescue_kernels.hpp"
#include "rescue_pow.hpp"

namespace sg {

// Waves per SIMD asked for: 4 at m = 2 (up to 128 VGPRs), 3 at m = 3, 4 (up to 168): a lane runs m
// interleaved chains, each with its own product temporaries, and a cap of 128 registers spills
// them at m >= 3.  Three waves of m >= 3 chains still give a SIMD nine or more independent chains.
// DESIGN.md 8.2 lists VGPRs, scratch (0) and the resulting occupancy of every instantiation.
constexpr int rescue_batch_waves(int m) { return m == 2 ? 4 : 3; }

template <int M, bool TRACE>
__global__ __launch_bounds__(kRescueBatchBlock, rescue_batch_waves(M)) void k_rescue_batch(
    const fe* __restrict__ in, uint64_t n, uint32_t N, const fe* __restrict__ consts, fe* __restrict__ out, fe r2) {
  const uint64_t i = (uint64_t)blockIdx.x * kRescueBatchBlock + threadIdx.x;
  if (i >= n) return;
  const fe one = {{1u, 0u, 0u, 0u}};
  const fe x = ld_fe(in + i);
  fe s[M];
  s[0] = mont_mul(x, r2);
#pragma unroll
  for (int k = 1; k < M; ++k) s[k] = fe_zero();
  fe* rows = out + i * ((uint64_t)N + 1) * M;  // TRACE: [input][row][register]
  if (TRACE) {
    st_fe(rows, x);
#pragma unroll
    for (int k = 1; k < M; ++k) st_fe(rows + k, fe_zero());
  }
  const fe* rc = consts + M * M;
  for (uint32_t r = 0; r < N; ++r) {
    rescue_round<M>(s, consts, rc + (uint64_t)2 * M * r);
    if (TRACE) {
#pragma unroll
      for (int k = 0; k < M; ++k) st_fe(rows + ((uint64_t)r + 1) * M + k, mont_mul(s[k], one));
    }
  }
  if (!TRACE) st_fe(out + i, mont_mul(s[0], one));
}

template <int M>
static void launch_m(bool trace, dim3 grid, hipStream_t s, const fe* in, uint64_t n, uint32_t N, const fe* consts,
                     fe* out, const fe& r2) {
  if (trace) hipLaunchKernelGGL((k_rescue_batch<M, true>), grid, dim3(kRescueBatchBlock), 0, s, in, n, N, consts, out, r2);
  else hipLaunchKernelGGL((k_rescue_batch<M, false>), grid, dim3(kRescueBatchBlock), 0, s, in, n, N, consts, out, r2);
}

hipError_t launch_rescue_batch(int m, bool trace, const fe* in, uint64_t n, uint32_t N, const fe* consts, fe* out,
                               const fe& r2, hipStream_t s) {
  if (!n) return hipSuccess;
  const uint64_t blocks = (n + kRescueBatchBlock - 1) / kRescueBatchBlock;
  if (m < kRescueBatchMinM || m > kRescueBatchMaxM || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  ProfScope ps(trace ? "rescue_trace_batch" : "rescue_hash_batch",
               16 * n * (1 + (trace ? ((uint64_t)N + 1) * (uint64_t)m : 1)), s);
  const dim3 grid((unsigned)blocks);
  switch (m) {
    case 2: launch_m<2>(trace, grid, s, in, n, N, consts, out, r2); break;
    case 3: launch_m<3>(trace, grid, s, in, n, N, consts, out, r2); break;
    default: launch_m<4>(trace, grid, s, in, n, N, consts, out, r2); break;
  }
  return hipGetLastError();
}

}  // namespace sg
