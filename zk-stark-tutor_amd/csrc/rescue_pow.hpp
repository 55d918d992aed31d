// The two S-box exponentiations of Rescue-Prime over p = 1 + 407 * 2^119, shared by the batch kernel
// (rescue_kernels.hip) and the host batch loop (stark.cpp), so the CPU suite covers the chain the
// device runs.  Both exponents are fixed by the field (rescue_prime.rs:120-123):
//   alpha     = 3 (the smallest k >= 3 coprime to p - 1)
//   alpha_inv = inv(p - 3) mod p = 3^-1 mod (p - 1) = (2p - 1) / 3
//             = 180331931428153586757283157844700080811
//             = 135 * 2^120 + (2^121 + 1) / 3      (bits: 1000011110, then 10 x 57, then 1011)
// Everything is in Montgomery form (fe128.hpp mont_mul keeps x*R mod p closed under products) and
// written over M independent state elements with M a compile-time constant: every step runs over
// all M before the next, so the M dependent chains interleave in the instruction stream and no
// array is indexed at run time.
#pragma once
#include "fe128.hpp"

namespace sg {

constexpr uint64_t kRescueAlpha = 3;
constexpr uint64_t kRescueAlphaInvLo = 0xAAAAAAAAAAAAAAABull;  // (2p - 1) / 3, low and high limbs
constexpr uint64_t kRescueAlphaInvHi = 0x87AAAAAAAAAAAAAAull;
// products of one x^alpha_inv (126 squarings + 15 multiplications) and of one x^alpha
constexpr int kRescueAlphaInvProducts = 141;
constexpr int kRescueAlphaProducts = 2;

template <int M>
__host__ __device__ __forceinline__ void rescue_sq_n(fe (&a)[M], int n) {
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int k = 0; k < M; ++k) a[k] = mont_mul(a[k], a[k]);
  }
}

// a = a^(4^b) * c: with D_k = x^((4^k - 1) / 3) (k binary digits "01"), D_(a+b) = D_a^(4^b) * D_b
template <int M>
__host__ __device__ __forceinline__ void rescue_shift_mul(fe (&a)[M], int b, const fe (&c)[M]) {
  rescue_sq_n<M>(a, 2 * b);
#pragma unroll
  for (int k = 0; k < M; ++k) a[k] = mont_mul(a[k], c[k]);
}

// x^3, two products per element
template <int M>
__host__ __device__ __forceinline__ void rescue_pow_alpha(fe (&x)[M]) {
#pragma unroll
  for (int k = 0; k < M; ++k) x[k] = mont_mul(mont_mul(x[k], x[k]), x[k]);
}

// x^alpha_inv.  Square-and-multiply would cost 127 + 64 products; the exponent's period gives an
// addition chain of 126 squarings + 15 multiplications:
//   D_60 by the chain 1, 2, 3, 6, 7, 14, 15, 30, 60 over k           118 squarings, 8 products
//   d2 = D_60^2, z = d2 * D_60 * x = x^(4^60) = x^(2^120)              1 squaring,   2 products
//   lo = d2 * x = x^((2^121 + 1) / 3)                                                1 product
//   z^135 = z^128 * z^4 * z^2 * z                                      7 squarings,  3 products
//   x^alpha_inv = z^135 * lo                                                         1 product
// 0 maps to 0, as the reference's pow does.
template <int M>
__host__ __device__ __forceinline__ void rescue_pow_alpha_inv(fe (&x)[M]) {
  fe d[M], t[M];
#pragma unroll
  for (int k = 0; k < M; ++k) d[k] = x[k];  // D_1
  rescue_shift_mul<M>(d, 1, x);             // D_2
  rescue_shift_mul<M>(d, 1, x);             // D_3
#pragma unroll
  for (int k = 0; k < M; ++k) t[k] = d[k];
  rescue_shift_mul<M>(d, 3, t);             // D_6
  rescue_shift_mul<M>(d, 1, x);             // D_7
#pragma unroll
  for (int k = 0; k < M; ++k) t[k] = d[k];
  rescue_shift_mul<M>(d, 7, t);             // D_14
  rescue_shift_mul<M>(d, 1, x);             // D_15
#pragma unroll
  for (int k = 0; k < M; ++k) t[k] = d[k];
  rescue_shift_mul<M>(d, 15, t);            // D_30
#pragma unroll
  for (int k = 0; k < M; ++k) t[k] = d[k];
  rescue_shift_mul<M>(d, 30, t);            // D_60
#pragma unroll
  for (int k = 0; k < M; ++k) {
    const fe d2 = mont_mul(d[k], d[k]);
    t[k] = mont_mul(d2, x[k]);                   // lo
    d[k] = mont_mul(mont_mul(d2, d[k]), x[k]);   // z
  }
  fe z2[M], z4[M];
#pragma unroll
  for (int k = 0; k < M; ++k) {
    z2[k] = mont_mul(d[k], d[k]);
    z4[k] = mont_mul(z2[k], z2[k]);
    x[k] = z4[k];
  }
  rescue_sq_n<M>(x, 5);  // z^128
#pragma unroll
  for (int k = 0; k < M; ++k)
    x[k] = mont_mul(mont_mul(mont_mul(mont_mul(x[k], z4[k]), z2[k]), d[k]), t[k]);
}

// One round (rescue_prime.rs:52-103) on a Montgomery state: x^alpha, MDS, the first m constants,
// x^alpha_inv, MDS, the second m constants.  mds = m x m row-major, rc = this round's 2m constants,
// both Montgomery.  Products: m (2 + 141) + 2 m^2.
template <int M>
__host__ __device__ __forceinline__ void rescue_round(fe (&s)[M], const fe* __restrict__ mds,
                                                      const fe* __restrict__ rc) {
  fe t[M];
  rescue_pow_alpha<M>(s);
#pragma unroll
  for (int j = 0; j < M; ++j) {
    fe acc = rc[j];
#pragma unroll
    for (int i = 0; i < M; ++i) acc = fe_add(acc, mont_mul(s[i], mds[j * M + i]));
    t[j] = acc;
  }
  rescue_pow_alpha_inv<M>(t);
#pragma unroll
  for (int j = 0; j < M; ++j) {
    fe acc = rc[M + j];
#pragma unroll
    for (int i = 0; i < M; ++i) acc = fe_add(acc, mont_mul(t[i], mds[j * M + i]));
    s[j] = acc;
  }
}

}  // namespace sg
