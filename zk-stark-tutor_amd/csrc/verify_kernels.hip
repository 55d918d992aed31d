// gfx950 kernels of the verifier (fri.rs:250-416, stark.rs:565-770): polynomials evaluated at
// the opened points, the transition zerofier's product at those points, and the Merkle
// authentication paths of every opening.  All values are exact: canonical field elements in
// device memory, Montgomery form (x R mod p, R = 2^128) only for multiplicands in registers.
//
// Evaluation and product share one skeleton.  A block owns a chunk of C = B * 32 consecutive
// coefficients (factors); lane t takes those at t, t + B, t + 2B, ... so a wave's loads are
// consecutive 16-byte elements, and every loaded coefficient is used for kEvalPts points held in
// registers.  The lanes' results are combined by a wave shuffle and an LDS step across the four
// waves; a second, small launch combines the chunks.  No atomics, no inter-block waiting.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "dev_util.hpp"
#include "fe128.hpp"
#include "merkle_dev.hpp"
#include "profiler.hpp"
#include "verify.hpp"

namespace sg {

namespace {

constexpr unsigned kWave = 64;
constexpr unsigned kWaves = kEvalBlock / kWave;
constexpr unsigned kMerkleBlock = 64;  // one BLAKE2b state per lane: a wave per block spreads the items over the CUs

template <bool MUL>
__device__ __forceinline__ fe combine(const fe& a, const fe& b) {
  if constexpr (MUL) return mont_mul(a, b);  // Montgomery x Montgomery -> Montgomery
  else return fe_add(a, b);
}

// sum (or Montgomery product) over the block's lanes; the result is valid in lane 0
template <bool MUL>
__device__ __forceinline__ fe block_reduce(fe v, fe* sm) {
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    fe o;
#pragma unroll
    for (int w = 0; w < 4; ++w) o.w[w] = (uint32_t)__shfl_down((int)v.w[w], d, kWave);
    v = combine<MUL>(v, o);
  }
  const unsigned wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  __syncthreads();  // sm may still be read from the previous reduction
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (unsigned w = 1; w < kWaves; ++w) v = combine<MUL>(v, sm[w]);
  }
  return v;
}

// Montgomery(b^e) from Montgomery(b) (e = 0: Montgomery(1))
__device__ __forceinline__ fe mont_pow(fe bm, uint64_t e, const fe& one_m) {
  fe acc = one_m;
  while (e) {
    if (e & 1) acc = mont_mul(acc, bm);
    bm = mont_mul(bm, bm);
    e >>= 1;
  }
  return acc;
}

}  // namespace

// pw[j (B + 1) + t] = Montgomery(x_j^t), t <= B
__global__ __launch_bounds__(kEvalBlock) void k_point_powers(const fe* __restrict__ xs, uint32_t nx,
                                                            fe* __restrict__ pw, fe r2, fe one_m) {
  const uint32_t j = blockIdx.x;
  if (j >= nx) return;
  const fe xm = mont_mul(ld_fe(xs + j), r2);
  for (uint32_t t = threadIdx.x; t <= kEvalBlock; t += kEvalBlock)
    st_fe(pw + (uint64_t)j * (kEvalBlock + 1) + t, mont_pow(xm, t, one_m));
}

// Polynomial::evaluate (field/polynomial.rs) of many polynomials at many points, one chunk per block:
// lane t runs Horner in y = x^B over c[base + t + k B], scales by x^t, the block sums.
__global__ __launch_bounds__(kEvalBlock) void k_eval_points(const EvalPolyRef* __restrict__ polys,
                                                           const uint32_t* __restrict__ cstart, uint32_t npoly,
                                                           const fe* __restrict__ pw, uint32_t nx,
                                                           fe* __restrict__ partial) {
  __shared__ fe sm[kWaves];
  const uint32_t g = blockIdx.x, t = threadIdx.x;
  uint32_t p = 0;
  while (p + 1 < npoly && cstart[p + 1] <= g) ++p;  // uniform: cstart[p] <= g < cstart[p + 1]
  const fe* __restrict__ c = polys[p].c;
  const uint64_t len = polys[p].len;
  const uint64_t base = (uint64_t)(g - cstart[p]) * kEvalChunk;
  const uint32_t j0 = blockIdx.y * kEvalPts;
  fe y[kEvalPts], acc[kEvalPts];
  uint32_t jj[kEvalPts];
#pragma unroll
  for (int q = 0; q < kEvalPts; ++q) {
    jj[q] = j0 + q < nx ? j0 + q : nx - 1;  // a padded point repeats the last one (not stored)
    y[q] = ld_fe(pw + (uint64_t)jj[q] * (kEvalBlock + 1) + kEvalBlock);
    acc[q] = fe_zero();
  }
  // rows of B coefficients this chunk holds (uniform over the block)
  const uint64_t rows64 = (len - base + kEvalBlock - 1) / kEvalBlock;
  const int rows = rows64 < kEvalPerLane ? (int)rows64 : (int)kEvalPerLane;
  for (int k = rows - 1; k >= 0; --k) {
    const uint64_t i = base + (uint64_t)k * kEvalBlock + t;
    const fe cf = i < len ? ld_fe(c + i) : fe_zero();
#pragma unroll
    for (int q = 0; q < kEvalPts; ++q) acc[q] = fe_add(mont_mul(acc[q], y[q]), cf);
  }
#pragma unroll
  for (int q = 0; q < kEvalPts; ++q) {
    const fe xt = ld_fe(pw + (uint64_t)jj[q] * (kEvalBlock + 1) + t);
    const fe r = block_reduce<false>(mont_mul(acc[q], xt), sm);
    if (t == 0 && j0 + q < nx) st_fe(partial + (uint64_t)g * nx + j0 + q, r);
  }
}

// out[p nx + j] = sum_ch partial[(cstart[p] + ch) nx + j] x_j^(C ch)
__global__ __launch_bounds__(kEvalBlock) void k_eval_points_finish(const uint32_t* __restrict__ cstart,
                                                                  const fe* __restrict__ pw, uint32_t nx,
                                                                  const fe* __restrict__ partial,
                                                                  fe* __restrict__ out, fe one_m) {
  __shared__ fe sm[kWaves];
  const uint32_t j = blockIdx.x, p = blockIdx.y;
  const uint32_t c0 = cstart[p], nch = cstart[p + 1] - c0;
  fe xc = ld_fe(pw + (uint64_t)j * (kEvalBlock + 1) + kEvalBlock);  // Montgomery(x^B)
#pragma unroll 1
  for (unsigned s = 1; s < kEvalPerLane; s <<= 1) xc = mont_mul(xc, xc);  // Montgomery(x^C)
  fe acc = fe_zero();
  for (uint32_t ch = threadIdx.x; ch < nch; ch += kEvalBlock)
    acc = fe_add(acc, mont_mul(ld_fe(partial + (uint64_t)(c0 + ch) * nx + j), mont_pow(xc, ch, one_m)));
  const fe r = block_reduce<false>(acc, sm);
  if (threadIdx.x == 0) st_fe(out + (uint64_t)p * nx + j, r);
}

// prod_{r in chunk} (x_j - q^r) per block.  x_j and the running power q^r are held in Montgomery
// form, so their difference is the factor's Montgomery form and every product (lane, wave, block,
// chunks) stays in Montgomery form: no power of R is left to undo (k_bary_prod instead counts the
// R^-1 of each product; here lanes at the ragged end multiply by Montgomery(1) and the count would
// differ per lane).
__global__ __launch_bounds__(kEvalBlock) void k_geo_zerofier_at(GeoZeroArgs a) {
  __shared__ fe sm[kWaves];
  const uint32_t g = blockIdx.x, t = threadIdx.x;
  const uint64_t base = (uint64_t)g * kEvalChunk;
  const uint32_t j0 = blockIdx.y * kEvalPts;
  // q^(base + t)
  const uint64_t e = base + t;
  fe cur = a.one_m;
  for (int i = 0; i < a.nbits; ++i)
    if ((e >> i) & 1) cur = mont_mul(cur, a.sq[i]);
  fe x[kEvalPts], acc[kEvalPts];
#pragma unroll
  for (int q = 0; q < kEvalPts; ++q) {
    x[q] = mont_mul(ld_fe(a.xs + (j0 + q < a.nx ? j0 + q : a.nx - 1)), a.r2);
    acc[q] = a.one_m;
  }
  const uint64_t rows64 = (a.n - base + kEvalBlock - 1) / kEvalBlock;
  const int rows = rows64 < kEvalPerLane ? (int)rows64 : (int)kEvalPerLane;
  for (int k = 0; k < rows; ++k) {
    const bool in = base + (uint64_t)k * kEvalBlock + t < a.n;
#pragma unroll
    for (int q = 0; q < kEvalPts; ++q) acc[q] = mont_mul(acc[q], in ? fe_sub(x[q], cur) : a.one_m);
    cur = mont_mul(cur, a.qB_m);
  }
#pragma unroll
  for (int q = 0; q < kEvalPts; ++q) {
    const fe r = block_reduce<true>(acc[q], sm);
    if (t == 0 && j0 + q < a.nx) st_fe(a.partial + (uint64_t)g * a.nx + j0 + q, r);
  }
}

__global__ __launch_bounds__(kEvalBlock) void k_geo_zerofier_finish(const fe* __restrict__ partial, uint32_t chunks,
                                                                   uint32_t nx, fe* __restrict__ out, fe one_m) {
  __shared__ fe sm[kWaves];
  const uint32_t j = blockIdx.x;
  fe acc = one_m;
  for (uint32_t g = threadIdx.x; g < chunks; g += kEvalBlock) acc = mont_mul(acc, ld_fe(partial + (uint64_t)g * nx + j));
  const fe r = block_reduce<true>(acc, sm);
  if (threadIdx.x == 0) st_fe(out + j, mont_mul(r, fe_make(1, 0)));
}

// MerkleRoot::verify (merkle_root.rs:69-95), one lane per item: the leaf digest from the decimal
// string, then `depth` node hashes with the side chosen by the index bit.
__global__ __launch_bounds__(kMerkleBlock) void k_merkle_verify_batch(
    const uint64_t* __restrict__ roots, const uint64_t* __restrict__ indices, const fe* __restrict__ leaves,
    const uint64_t* __restrict__ paths, uint32_t stride, const uint32_t* __restrict__ depths, uint32_t n,
    uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * kMerkleBlock + threadIdx.x;
  if (i >= n) return;
  uint64_t h[8];
  leaf_hash(ld_fe(leaves + i), h);
  uint32_t depth = depths ? depths[i] : stride;
  if (depth > stride) depth = stride;  // never read past the item's row (the host rejects it first)
  uint64_t idx = indices[i];
  const uint64_t* p = paths + (uint64_t)i * stride * 8;
#pragma unroll 1
  for (uint32_t k = 0; k < depth; ++k) {
    uint64_t s[8], l[8], r[8];
    ld_digest(p + (uint64_t)k * 8, s);
    const bool right = (idx & 1) != 0;  // this node is the right child: the sibling goes first
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      l[w] = right ? s[w] : h[w];
      r[w] = right ? h[w] : s[w];
    }
    blake2b_node(l, r, h);
    idx >>= 1;
  }
  uint64_t rt[8], diff = 0;
  ld_digest(roots + (uint64_t)i * 8, rt);
#pragma unroll
  for (int w = 0; w < 8; ++w) diff |= rt[w] ^ h[w];
  ok[i] = diff == 0 ? 1 : 0;
}

// ------------------------------------------------------------------ launchers

hipError_t launch_point_powers(const fe* xs, uint32_t nx, fe* pw, const fe& r2, const fe& one_m, hipStream_t s) {
  if (!nx) return hipSuccess;
  ProfScope ps("point_powers", 16ull * nx * (kEvalBlock + 2), s);
  hipLaunchKernelGGL(k_point_powers, dim3(nx), dim3(kEvalBlock), 0, s, xs, nx, pw, r2, one_m);
  return hipGetLastError();
}

hipError_t launch_eval_points(const EvalPolyRef* polys, const uint32_t* cstart, uint32_t npoly, uint32_t total_chunks,
                              uint64_t total_coeffs, const fe* pw, uint32_t nx, fe* partial, hipStream_t s) {
  if (!total_chunks || !nx) return hipSuccess;
  const uint32_t groups = (nx + kEvalPts - 1) / kEvalPts;
  // every coefficient once, the chunk partials written
  ProfScope ps("eval_points", 16ull * total_coeffs + 16ull * total_chunks * nx, s);
  hipLaunchKernelGGL(k_eval_points, dim3(total_chunks, groups), dim3(kEvalBlock), 0, s, polys, cstart, npoly, pw, nx,
                     partial);
  return hipGetLastError();
}

hipError_t launch_eval_points_finish(const uint32_t* cstart, uint32_t npoly, const fe* pw, uint32_t nx,
                                     const fe* partial, fe* out, const fe& one_m, hipStream_t s) {
  if (!npoly || !nx) return hipSuccess;
  ProfScope ps("eval_points_finish", 16ull * npoly * nx, s);
  hipLaunchKernelGGL(k_eval_points_finish, dim3(nx, npoly), dim3(kEvalBlock), 0, s, cstart, pw, nx, partial, out,
                     one_m);
  return hipGetLastError();
}

hipError_t launch_geo_zerofier_at(const GeoZeroArgs& a, uint32_t chunks, hipStream_t s) {
  if (!chunks || !a.nx) return hipSuccess;
  const uint32_t groups = (a.nx + kEvalPts - 1) / kEvalPts;
  ProfScope ps("geo_zerofier_at", 16ull * a.nx + 16ull * chunks * a.nx, s);
  hipLaunchKernelGGL(k_geo_zerofier_at, dim3(chunks, groups), dim3(kEvalBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_geo_zerofier_finish(const fe* partial, uint32_t chunks, uint32_t nx, fe* out, const fe& one_m,
                                      hipStream_t s) {
  if (!nx) return hipSuccess;
  ProfScope ps("geo_zerofier_finish", 16ull * chunks * nx + 16ull * nx, s);
  hipLaunchKernelGGL(k_geo_zerofier_finish, dim3(nx), dim3(kEvalBlock), 0, s, partial, chunks, nx, out, one_m);
  return hipGetLastError();
}

hipError_t launch_merkle_verify_batch(const uint64_t* roots, const uint64_t* indices, const fe* leaves,
                                      const uint64_t* paths, uint32_t stride, const uint32_t* depths, uint32_t n,
                                      uint8_t* ok, hipStream_t s) {
  if (!n) return hipSuccess;
  // per item: root, index, leaf, its path row, the flag
  ProfScope ps("merkle_verify_batch", (64ull + 8 + 16 + 64ull * stride + 1) * n, s);
  hipLaunchKernelGGL(k_merkle_verify_batch, dim3((n + kMerkleBlock - 1) / kMerkleBlock), dim3(kMerkleBlock), 0, s,
                     roots, indices, leaves, paths, stride, depths, n, ok);
  return hipGetLastError();
}

}  // namespace sg
