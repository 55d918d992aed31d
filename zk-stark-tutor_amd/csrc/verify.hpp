// Verifier side (fri.rs:250-416, stark.rs:565-770): the three device evaluations
// (verify_kernels.hip), their host drivers with the plain host loops behind the context
// option "verify_device" = 0, the verifier's view of a proof stream and the deferred
// Merkle-path queue the FRI and STARK verifiers share (verify.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/stark_gpu.h"
#include "context.hpp"
#include "fe128.hpp"

namespace sg {

// ---- kernel shape (sg_verify_kernel_shape reports B and C to the bindings) ----
constexpr unsigned kEvalBlock = 256;                         // B: lanes of a block
constexpr unsigned kEvalPerLane = 32;                        // coefficients (factors) per lane
constexpr unsigned kEvalChunk = kEvalBlock * kEvalPerLane;   // C: coefficients (factors) per block
constexpr int kEvalPts = 4;                                  // points a lane keeps in registers
constexpr int kGeoMaxBits = 40;                              // squarings of q passed to the product kernel (n < 2^38)

struct EvalPolyRef {
  const fe* c;   // device coefficients (canonical)
  uint64_t len;
};

// pw[j (B + 1) + t] = Montgomery(x_j^t), t <= B
hipError_t launch_point_powers(const fe* xs, uint32_t nx, fe* pw, const fe& r2, const fe& one_m, hipStream_t s);
// partial[g nx + j] = sum_{i in chunk g} c_i x_j^(i - base(g)); chunk g of polynomial p: cstart[p] <= g < cstart[p+1]
hipError_t launch_eval_points(const EvalPolyRef* polys, const uint32_t* cstart, uint32_t npoly, uint32_t total_chunks,
                              uint64_t total_coeffs, const fe* pw, uint32_t nx, fe* partial, hipStream_t s);
// out[p nx + j] = sum_ch partial[(cstart[p] + ch) nx + j] x_j^(C ch)
hipError_t launch_eval_points_finish(const uint32_t* cstart, uint32_t npoly, const fe* pw, uint32_t nx,
                                     const fe* partial, fe* out, const fe& one_m, hipStream_t s);
struct GeoZeroArgs {
  fe sq[kGeoMaxBits];  // Montgomery(q^(2^i))
  fe qB_m;             // Montgomery(q^B)
  fe one_m;            // Montgomery(1)
  fe r2;               // R^2 mod p
  uint64_t n;
  const fe* xs;
  uint32_t nx;
  int nbits;           // bits of the largest exponent a lane starts from
  fe* partial;         // [chunks][nx], Montgomery form
};
hipError_t launch_geo_zerofier_at(const GeoZeroArgs& a, uint32_t chunks, hipStream_t s);
// out[j] = prod_g partial[g nx + j] (canonical; 1 for no chunk)
hipError_t launch_geo_zerofier_finish(const fe* partial, uint32_t chunks, uint32_t nx, fe* out, const fe& one_m,
                                      hipStream_t s);
// merkle_root.rs:69-95 per lane: ok[i] = (root_i == the root recomputed from leaf_i along path_i)
hipError_t launch_merkle_verify_batch(const uint64_t* roots, const uint64_t* indices, const fe* leaves,
                                      const uint64_t* paths, uint32_t stride, const uint32_t* depths, uint32_t n,
                                      uint8_t* ok, hipStream_t s);

// ---- host drivers (device kernels, or host loops when ctx->opt.verify_device is off) ----
// out[p nx + j] = polys[p](xs[j]); the coefficient vectors are in device memory, xs / out on the host
void eval_points(sg_ctx* ctx, const std::vector<EvalPolyRef>& polys, const fe* xs, size_t nx, fe* out);
// out[j] = prod_{r < n} (xs[j] - q^r)
void zerofier_geometric_at(sg_ctx* ctx, const fe& q, uint64_t n, const fe* xs, size_t nx, fe* out);
// host arrays; depths == nullptr: every depth = stride.  Throws SG_ERR_INVALID for depth 0 / index >= 2^depth
void merkle_verify_batch(sg_ctx* ctx, const uint8_t* roots, const uint64_t* indices, const fe* leaves,
                         const uint8_t* paths, size_t stride, const uint32_t* depths, size_t n, uint8_t* ok);

// ---- the verifier's proof stream ----
struct VObject {
  uint8_t code = 0;
  const uint8_t* p = nullptr;
  size_t len = 0;
};
struct VStream {
  const sg_verifier_stream* vs;
  VObject pull();                                // SG_ERR_INVALID "Cannot pull, queue is empty" when exhausted
  void fiat_shamir(size_t n, uint8_t* out);
  // typed pulls: SG_ERR_INVALID on another kind (the reference's expect_*), SG_ERR_NONCANONICAL for elements >= p
  std::vector<uint8_t> root();
  std::vector<fe> elements(uint8_t code, const char* what, size_t want);  // want = 0: any count
};

// Merkle openings met while walking a proof in the reference's order.  They are checked together
// (one launch) when the walk ends -- at its end, at the first check the host decides itself, or at
// the first structural error -- and the earliest failure in the reference's order is the verdict.
struct PathQueue {
  struct Item {
    std::vector<uint8_t> root;
    uint64_t index;
    fe leaf;
    std::vector<uint8_t> path;  // depth x 64 bytes
    uint32_t depth;
    bool wellformed;            // 64-byte root and nodes (else the reference's comparison fails)
    std::string msg;            // the rejection text if this opening fails
  };
  std::vector<Item> items;
  // pulls a Path object and queues its check against `root`; SG_ERR_INVALID where the reference
  // panics (an empty path, "Cannot verify invalid index")
  void pull_path(VStream& in, const std::vector<uint8_t>& root, uint64_t index, const fe& leaf, std::string msg);
  // index of the first failing item, -1 if none
  long flush(sg_ctx* ctx);
};

// Runs `walk` (returns 1, or 0 with a rejection text); then the queued openings.  The earliest event
// in the reference's order decides: a failing opening, else the walk's structural error (rethrown),
// else the walk's verdict.
template <class F>
int verify_in_order(sg_ctx* ctx, PathQueue& q, std::string& msg, F&& walk) {
  int verdict = 1;
  std::string m;
  bool failed = false;
  Error pending{0, ""};
  try {
    verdict = walk(m);
  } catch (const Error& e) {
    if (e.code == SG_ERR_HIP || e.code == SG_ERR_NOMEM) throw;
    pending = e;
    failed = true;
  }
  const long bad = q.flush(ctx);
  if (bad >= 0) {
    msg = q.items[(size_t)bad].msg;
    q.items.clear();
    return 0;
  }
  q.items.clear();
  if (failed) throw pending;
  msg = m;
  return verdict;
}

// fri.rs:250-416 up to the queued openings: returns 1, or 0 with `msg` (a check the host decides).
// points receives polynomial_values in push order.
int fri_verify_walk(sg_ctx* ctx, const sg_fri* f, VStream& in, PathQueue& q, const std::string& prefix,
                    std::vector<std::pair<uint64_t, fe>>& points, std::string& msg);

}  // namespace sg
