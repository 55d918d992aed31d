// The verifier's host side: drivers of the three device evaluations (verify_kernels.hip) with
// their plain host loops (context option "verify_device" = 0), the verifier's view of a proof
// stream, FRI::verify (fri.rs:250-416) and the C ABI of all of them.  Stark::verify is in
// stark.cpp, beside the prover whose degree bookkeeping it shares.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_field.hpp"
#include "host_hash.hpp"
#include "internal.hpp"
#include "poly.hpp"
#include "verify.hpp"

namespace sg {

namespace {

fe one_mont() { return to_mont(fe_one()); }

fe get_u128_be(const uint8_t* b) {
  uint64_t hi = 0, lo = 0;
  for (int i = 0; i < 8; ++i) hi = (hi << 8) | b[i];
  for (int i = 8; i < 16; ++i) lo = (lo << 8) | b[i];
  return fe_make(lo, hi);
}

const char* kind_name(uint8_t code) {
  switch (code) {
    case SG_OBJ_ROOT: return "Root";
    case SG_OBJ_CODEWORD: return "Codeword";
    case SG_OBJ_PATH: return "Path";
    case SG_OBJ_LEAFS: return "Leafs";
    default: return "Value";
  }
}

}  // namespace

// ====================================================================== evaluations

void eval_points(sg_ctx* ctx, const std::vector<EvalPolyRef>& polys, const fe* xs, size_t nx, fe* out) {
  const size_t npoly = polys.size();
  if (!npoly || !nx) return;
  if (!ctx->opt.verify_device) {
    // the plain host loop: Horner per polynomial and point (field/polynomial.rs evaluate)
    for (size_t p = 0; p < npoly; ++p) {
      const std::vector<fe> c = dpoly_download(ctx, polys[p].c, polys[p].len);
      for (size_t j = 0; j < nx; ++j) {
        const fe xm = to_mont(xs[j]);
        fe acc = fe_zero();
        for (size_t i = c.size(); i-- > 0;) acc = fe_add(mont_mul(acc, xm), c[i]);
        out[p * nx + j] = acc;
      }
    }
    return;
  }
  SG_REQUIRE(npoly <= 65535 && nx <= 65535 * (size_t)kEvalPts, "too many polynomials or points for one evaluation");
  std::vector<uint32_t> cstart(npoly + 1, 0);
  uint64_t total_coeffs = 0;
  for (size_t p = 0; p < npoly; ++p) {
    const uint64_t ch = (polys[p].len + kEvalChunk - 1) / kEvalChunk;
    SG_REQUIRE((uint64_t)cstart[p] + ch < ((uint64_t)1 << 31), "polynomials too long for one evaluation");
    cstart[p + 1] = cstart[p] + (uint32_t)ch;
    total_coeffs += polys[p].len;
  }
  const uint32_t chunks = cstart[npoly];
  DevBuf d_polys(ctx, npoly * sizeof(EvalPolyRef)), d_cstart(ctx, (npoly + 1) * sizeof(uint32_t));
  DevBuf d_xs(ctx, nx * sizeof(fe)), d_pw(ctx, nx * (kEvalBlock + 1) * sizeof(fe));
  DevBuf d_partial(ctx, std::max<size_t>((size_t)chunks * nx, 1) * sizeof(fe)), d_out(ctx, npoly * nx * sizeof(fe));
  hipStream_t s = ctx->stream;
  SG_HIP(hipMemcpyAsync(d_polys.get(), polys.data(), npoly * sizeof(EvalPolyRef), hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(d_cstart.get(), cstart.data(), (npoly + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(d_xs.get(), xs, nx * sizeof(fe), hipMemcpyHostToDevice, s));
  SG_HIP(launch_point_powers(d_xs.as<fe>(), (uint32_t)nx, d_pw.as<fe>(), fe_r2(), one_mont(), s));
  SG_HIP(launch_eval_points(d_polys.as<EvalPolyRef>(), d_cstart.as<uint32_t>(), (uint32_t)npoly, chunks, total_coeffs,
                            d_pw.as<fe>(), (uint32_t)nx, d_partial.as<fe>(), s));
  SG_HIP(launch_eval_points_finish(d_cstart.as<uint32_t>(), (uint32_t)npoly, d_pw.as<fe>(), (uint32_t)nx,
                                   d_partial.as<fe>(), d_out.as<fe>(), one_mont(), s));
  SG_HIP(hipMemcpyAsync(out, d_out.get(), npoly * nx * sizeof(fe), hipMemcpyDeviceToHost, s));
  host_wait(ctx, s);
}

void zerofier_geometric_at(sg_ctx* ctx, const fe& q, uint64_t n, const fe* xs, size_t nx, fe* out) {
  if (!nx) return;
  if (!ctx->opt.verify_device) {
    // the plain host loop: prod (x - q^r), x, q^r and the accumulator in Montgomery form
    const fe qm = to_mont(q);
    for (size_t j = 0; j < nx; ++j) {
      const fe xm = to_mont(xs[j]);
      fe acc = one_mont(), cur = one_mont();
      for (uint64_t r = 0; r < n; ++r) {
        acc = mont_mul(acc, fe_sub(xm, cur));
        cur = mont_mul(cur, qm);
      }
      out[j] = from_mont(acc);
    }
    return;
  }
  SG_REQUIRE(n < ((uint64_t)1 << (kGeoMaxBits - 2)), "zerofier: too many factors");
  SG_REQUIRE(nx <= 65535 * (size_t)kEvalPts, "too many points for one evaluation");
  const uint32_t chunks = (uint32_t)((n + kEvalChunk - 1) / kEvalChunk);
  DevBuf d_xs(ctx, nx * sizeof(fe)), d_partial(ctx, std::max<size_t>((size_t)chunks * nx, 1) * sizeof(fe));
  DevBuf d_out(ctx, nx * sizeof(fe));
  GeoZeroArgs a;
  fe sq = to_mont(q);
  for (int i = 0; i < kGeoMaxBits; ++i) {
    a.sq[i] = sq;
    sq = mont_mul(sq, sq);
  }
  a.qB_m = a.sq[__builtin_ctz(kEvalBlock)];
  a.one_m = one_mont();
  a.r2 = fe_r2();
  a.n = n;
  a.xs = d_xs.as<fe>();
  a.nx = (uint32_t)nx;
  a.nbits = 64 - __builtin_clzll((unsigned long long)(n + kEvalChunk));
  a.partial = d_partial.as<fe>();
  hipStream_t s = ctx->stream;
  SG_HIP(hipMemcpyAsync(d_xs.get(), xs, nx * sizeof(fe), hipMemcpyHostToDevice, s));
  SG_HIP(launch_geo_zerofier_at(a, chunks, s));
  SG_HIP(launch_geo_zerofier_finish(d_partial.as<fe>(), chunks, (uint32_t)nx, d_out.as<fe>(), one_mont(), s));
  SG_HIP(hipMemcpyAsync(out, d_out.get(), nx * sizeof(fe), hipMemcpyDeviceToHost, s));
  host_wait(ctx, s);
}

void merkle_verify_batch(sg_ctx* ctx, const uint8_t* roots, const uint64_t* indices, const fe* leaves,
                         const uint8_t* paths, size_t stride, const uint32_t* depths, size_t n, uint8_t* ok) {
  for (size_t i = 0; i < n; ++i) {
    const uint32_t d = depths ? depths[i] : (uint32_t)stride;
    SG_REQUIRE(d >= 1 && d <= stride && d < 64, "Merkle path is empty or longer than its row");
    SG_REQUIRE(indices[i] < ((uint64_t)1 << d), "Cannot verify invalid index");
  }
  if (!n) return;
  if (!ctx->opt.verify_device) {
    for (size_t i = 0; i < n; ++i)
      ok[i] = (uint8_t)sg_merkle_verify(roots + 64 * i, indices[i], paths + 64 * stride * i,
                                        depths ? depths[i] : stride, from_fe(leaves[i]));
    return;
  }
  SG_REQUIRE(n < ((size_t)1 << 31) && stride < 64, "too many openings for one batch");
  DevBuf d_roots(ctx, 64 * n), d_idx(ctx, 8 * n), d_leaves(ctx, sizeof(fe) * n), d_paths(ctx, 64 * stride * n);
  DevBuf d_depths(ctx, 4 * n), d_ok(ctx, n);
  hipStream_t s = ctx->stream;
  SG_HIP(hipMemcpyAsync(d_roots.get(), roots, 64 * n, hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(d_idx.get(), indices, 8 * n, hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(d_leaves.get(), leaves, sizeof(fe) * n, hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(d_paths.get(), paths, 64 * stride * n, hipMemcpyHostToDevice, s));
  if (depths) SG_HIP(hipMemcpyAsync(d_depths.get(), depths, 4 * n, hipMemcpyHostToDevice, s));
  SG_HIP(launch_merkle_verify_batch(d_roots.as<uint64_t>(), d_idx.as<uint64_t>(), d_leaves.as<fe>(),
                                    d_paths.as<uint64_t>(), (uint32_t)stride, depths ? d_depths.as<uint32_t>() : nullptr,
                                    (uint32_t)n, d_ok.as<uint8_t>(), s));
  SG_HIP(hipMemcpyAsync(ok, d_ok.get(), n, hipMemcpyDeviceToHost, s));
  host_wait(ctx, s);
}

// ====================================================================== proof stream, verifier side

VObject VStream::pull() {
  VObject o;
  const int rc = vs->pull(vs->user, &o.code, &o.p, &o.len);
  if (rc == SG_ERR_INVALID) throw Error{SG_ERR_INVALID, "Cannot pull, queue is empty"};
  if (rc != 0) throw Error{SG_ERR_CALLBACK, "proof stream pull callback failed"};
  if (o.code > SG_OBJ_VALUE || (o.len && !o.p)) throw Error{SG_ERR_INVALID, "pulled an unknown proof stream object"};
  return o;
}

void VStream::fiat_shamir(size_t n, uint8_t* out) {
  if (vs->fiat_shamir_verifier(vs->user, n, out) != 0)
    throw Error{SG_ERR_CALLBACK, "proof stream fiat_shamir_verifier callback failed"};
}

std::vector<uint8_t> VStream::root() {
  const VObject o = pull();
  if (o.code != SG_OBJ_ROOT) throw Error{SG_ERR_INVALID, "expected StarkProofStreamEnum to be Root"};
  return std::vector<uint8_t>(o.p, o.p + o.len);
}

std::vector<fe> VStream::elements(uint8_t code, const char* what, size_t want) {
  const VObject o = pull();
  if (o.code != code) throw Error{SG_ERR_INVALID, std::string("expected StarkProofStreamEnum to be ") + kind_name(code)};
  if (o.len % 16 != 0 || (want && o.len != 16 * want))
    throw Error{SG_ERR_INVALID, std::string(what) + ": malformed payload"};
  std::vector<fe> v(o.len / 16);
  for (size_t i = 0; i < v.size(); ++i) {
    v[i] = get_u128_be(o.p + 16 * i);
    if (!fe_is_canonical(v[i])) throw Error{SG_ERR_NONCANONICAL, std::string(what) + ": element >= p"};
  }
  return v;
}

void PathQueue::pull_path(VStream& in, const std::vector<uint8_t>& root, uint64_t index, const fe& leaf,
                          std::string msg) {
  const VObject o = in.pull();
  if (o.code != SG_OBJ_PATH) throw Error{SG_ERR_INVALID, "expected StarkProofStreamEnum to be Path"};
  Item it;
  it.root = root;
  it.index = index;
  it.leaf = leaf;
  it.depth = 0;
  it.wellformed = root.size() == 64;
  it.msg = std::move(msg);
  size_t pos = 0;
  while (pos < o.len) {
    if (pos + 8 > o.len) throw Error{SG_ERR_INVALID, "Path: malformed payload"};
    uint64_t sz = 0;
    for (int i = 0; i < 8; ++i) sz = (sz << 8) | o.p[pos + i];
    pos += 8;
    if (sz > o.len - pos) throw Error{SG_ERR_INVALID, "Path: malformed payload"};
    if (sz == 64) it.path.insert(it.path.end(), o.p + pos, o.p + pos + 64);
    else {
      it.wellformed = false;  // a node of another size hashes to another root
      it.path.insert(it.path.end(), 64, 0);
    }
    pos += sz;
    ++it.depth;
  }
  // merkle_root.rs:70-73: assert!(index < (1 << len)), path.get(0).unwrap()
  if (it.depth >= 64 || index >= ((uint64_t)1 << it.depth)) throw Error{SG_ERR_INVALID, "Cannot verify invalid index"};
  if (it.depth == 0) throw Error{SG_ERR_INVALID, "Merkle path is empty"};
  items.push_back(std::move(it));
}

long PathQueue::flush(sg_ctx* ctx) {
  const size_t n = items.size();
  if (!n) return -1;
  size_t stride = 1;
  for (auto& it : items) stride = std::max<size_t>(stride, it.depth);
  // pinned staging would save a copy; the batch is ~100 KB..4 MB and goes up once
  std::vector<uint8_t> roots(64 * n, 0), paths(64 * stride * n, 0), ok(n, 0);
  std::vector<uint64_t> idx(n);
  std::vector<fe> leaves(n);
  std::vector<uint32_t> depths(n);
  for (size_t i = 0; i < n; ++i) {
    const Item& it = items[i];
    if (it.root.size() == 64) memcpy(&roots[64 * i], it.root.data(), 64);
    memcpy(&paths[64 * stride * i], it.path.data(), it.path.size());
    idx[i] = it.index;
    leaves[i] = it.leaf;
    depths[i] = it.depth;
  }
  merkle_verify_batch(ctx, roots.data(), idx.data(), leaves.data(), paths.data(), stride, depths.data(), n, ok.data());
  for (size_t i = 0; i < n; ++i)
    if (!ok[i] || !items[i].wellformed) return (long)i;
  return -1;
}

// ====================================================================== FRI::verify

int fri_verify_walk(sg_ctx* ctx, const sg_fri* f, VStream& in, PathQueue& q, const std::string& prefix,
                    std::vector<std::pair<uint64_t, fe>>& points, std::string& msg) {
  auto reject = [&](const std::string& m) {
    msg = prefix + m;
    return 0;
  };
  const uint64_t N = f->domain_length, c = f->num_colinearity_tests;
  SG_REQUIRE(N && (N & (N - 1)) == 0, "FRI domain length must be a power of two");
  SG_REQUIRE(f->expansion_factor >= 1, "expansion_factor must be at least 1");
  check_canonical(&f->offset, 1, "offset");
  check_canonical(&f->omega, 1, "omega");
  fe omega = to_fe(f->omega), offset = to_fe(f->offset);
  const size_t rounds = fri_num_rounds(f);
  SG_REQUIRE(rounds >= 1, "FRI::verify needs at least one round (roots.last().unwrap())");

  // fri.rs:263-270: the roots, one challenge after each
  std::vector<std::vector<uint8_t>> roots;
  std::vector<fe> alphas;
  uint8_t fs[32];
  for (size_t r = 0; r < rounds; ++r) {
    roots.push_back(in.root());
    in.fiat_shamir(32, fs);
    alphas.push_back(fe_sample(fs, 32));
  }

  // fri.rs:272-328: the last codeword matches its root and is of low degree
  const std::vector<fe> last = in.elements(SG_OBJ_CODEWORD, "last codeword", 0);
  const uint64_t L = last.size();
  SG_REQUIRE(L > 0 && (L & (L - 1)) == 0, "Leafs len must be power of two");
  DPoly d_last = dpoly_upload(ctx, last.data(), L);
  {
    std::unique_ptr<sg_tree> t(build_tree(ctx, d_last.p(), L));
    if (roots.back().size() != 64 || memcmp(t->root, roots.back().data(), 64) != 0)
      return reject("last codeword is not well formed");
  }
  SG_REQUIRE(L >= f->expansion_factor, "attempt to subtract with overflow (last codeword shorter than the expansion factor)");
  const uint64_t degree = L / f->expansion_factor - 1;
  fe last_omega = omega, last_offset = offset;
  for (size_t r = 0; r + 1 < rounds; ++r) {
    last_omega = fe_mul(last_omega, last_omega);
    last_offset = fe_mul(last_offset, last_offset);
  }
  if (!fe_eq(fe_inv(last_omega), fe_pow(last_omega, L - 1))) return reject("omega does not have the right order");
  {
    const int logn = ilog2_exact(L);
    DPoly coeffs = dpoly_alloc(ctx, L), scaled = dpoly_alloc(ctx, L), back = dpoly_alloc(ctx, L), re = dpoly_alloc(ctx, L);
    intt_sized(ctx, last_omega, d_last.p(), logn, coeffs.p());
    dev_scale_pow(ctx, scaled.p(), coeffs.p(), L, fe_inv(last_offset));
    const int64_t pd = dev_degree(ctx, scaled.p(), L);
    if (pd < 0) return reject("Received none instead of polynomial degree");
    if ((uint64_t)pd > degree)
      return reject("last codeword does not correspond to polynomial of low enough degree (it is " +
                    std::to_string(pd) + " but should be <= " + std::to_string(degree) + ")");
    dev_scale_pow(ctx, back.p(), scaled.p(), L, last_offset);
    if (logn == 0) SG_HIP(hipMemcpyAsync(re.p(), back.p(), sizeof(fe), hipMemcpyDeviceToDevice, ctx->stream));
    else ntt_sized(ctx, last_omega, back.p(), L, logn, re.p());
    const std::vector<fe> reeval = dpoly_download(ctx, re.p(), L);
    if (memcmp(reeval.data(), last.data(), L * sizeof(fe)) != 0)
      return reject("re-evaluated codeword does not match original");
  }

  // fri.rs:330-335
  in.fiat_shamir(32, fs);
  std::vector<size_t> top(c);
  sample_indices(fs, 32, N >> 1, N >> (rounds - 1), c, top.data());

  // fri.rs:337-413: per round the colinearity tests (decided here), then the aa / bb / cc openings (queued)
  for (size_t r = 0; r + 1 < rounds; ++r) {
    const uint64_t half = N >> (r + 1);
    const fe omega_half = fe_pow(omega, half);
    std::vector<uint64_t> ic(c);
    std::vector<fe> aa(c), bb(c), cc(c);
    for (size_t s = 0; s < c; ++s) {
      ic[s] = top[s] % half;
      const std::vector<fe> l = in.elements(SG_OBJ_LEAFS, "leafs", 3);
      aa[s] = l[0];
      bb[s] = l[1];
      cc[s] = l[2];
      if (r == 0) {
        points.emplace_back(ic[s], l[0]);
        points.emplace_back(ic[s] + half, l[1]);
      }
      // polynomial.rs:161-177 test_colinearity: the interpolant through the three points has degree
      // exactly 1 -- (cx, cy) on the line through a and b, and that line not constant
      const fe ax = fe_mul(offset, fe_pow(omega, ic[s]));
      const fe bx = fe_mul(ax, omega_half);
      const fe cx = alphas[r];
      SG_REQUIRE(!fe_eq(ax, bx) && !fe_eq(ax, cx) && !fe_eq(bx, cx), "divide by zero");
      const fe lhs = fe_mul(fe_sub(l[1], l[0]), fe_sub(cx, ax));
      const fe rhs = fe_mul(fe_sub(l[2], l[0]), fe_sub(bx, ax));
      if (!fe_eq(lhs, rhs) || fe_eq(l[0], l[1])) return reject("colinearity check failure");
    }
    for (size_t i = 0; i < c; ++i) {
      q.pull_path(in, roots[r], ic[i], aa[i], prefix + "Merkle auth path verification failed for aa");
      q.pull_path(in, roots[r], ic[i] + half, bb[i], prefix + "Merkle auth path verification failed for bb");
      q.pull_path(in, roots[r + 1], ic[i], cc[i], prefix + "Merkle auth path verification failed for cc");
    }
    omega = fe_mul(omega, omega);
    offset = fe_mul(offset, offset);
  }
  return 1;
}

}  // namespace sg

// ====================================================================== C ABI

using namespace sg;

extern "C" void sg_verify_kernel_shape(size_t* block, size_t* chunk) {
  if (block) *block = kEvalBlock;
  if (chunk) *chunk = kEvalChunk;
}

extern "C" int sg_poly_evaluate_points(sg_ctx* ctx, const sg_poly* const* polys, size_t npoly, const sg_fe* xs,
                                       size_t nx, sg_fe* out) {
  return guard(ctx, [&] {
    set_device(ctx);
    SG_REQUIRE((polys || !npoly) && (xs || !nx) && (out || !npoly || !nx), "null argument");
    check_canonical(xs, nx, "point");
    std::vector<EvalPolyRef> refs;
    for (size_t p = 0; p < npoly; ++p) {
      SG_REQUIRE(polys[p], "null polynomial");
      refs.push_back({polys[p]->d.p(), polys[p]->d.len});
    }
    eval_points(ctx, refs, reinterpret_cast<const fe*>(xs), nx, reinterpret_cast<fe*>(out));
  });
}

extern "C" int sg_zerofier_geometric_at(sg_ctx* ctx, sg_fe root, uint64_t n, const sg_fe* xs, size_t nx, sg_fe* out) {
  return guard(ctx, [&] {
    set_device(ctx);
    SG_REQUIRE((xs && out) || !nx, "null argument");
    check_canonical(&root, 1, "root");
    check_canonical(xs, nx, "point");
    zerofier_geometric_at(ctx, to_fe(root), n, reinterpret_cast<const fe*>(xs), nx, reinterpret_cast<fe*>(out));
  });
}

extern "C" int sg_merkle_verify_batch(sg_ctx* ctx, const uint8_t* roots, const uint64_t* indices, const sg_fe* leaves,
                                      const uint8_t* paths, size_t stride, const uint32_t* depths, size_t n,
                                      uint8_t* ok) {
  return guard(ctx, [&] {
    set_device(ctx);
    SG_REQUIRE((roots && indices && leaves && paths && ok) || !n, "null argument");
    check_canonical(leaves, n, "leaf");
    merkle_verify_batch(ctx, roots, indices, reinterpret_cast<const fe*>(leaves), paths, stride, depths, n, ok);
  });
}

namespace {
int stream_pull_cb(void* user, uint8_t* code, const uint8_t** payload, size_t* len) {
  return sg_stream_pull(reinterpret_cast<sg_stream*>(user), code, payload, len);
}
int stream_fsv_cb(void* user, size_t num_bytes, uint8_t* out) {
  return sg_stream_fiat_shamir_verifier(reinterpret_cast<sg_stream*>(user), num_bytes, out);
}
}  // namespace

extern "C" sg_verifier_stream sg_stream_verifier_callbacks(sg_stream* s) {
  sg_verifier_stream vs;
  vs.user = s;
  vs.pull = stream_pull_cb;
  vs.fiat_shamir_verifier = stream_fsv_cb;
  return vs;
}

extern "C" int sg_fri_verify(sg_ctx* ctx, const sg_fri* fri, const sg_verifier_stream* vs, size_t* indices,
                             sg_fe* values) {
  int verdict = 0;
  const int rc = guard(ctx, [&] {
    set_device(ctx);
    SG_REQUIRE(fri && vs && vs->pull && vs->fiat_shamir_verifier, "verifier stream callbacks required");
    VStream in{vs};
    PathQueue q;
    std::vector<std::pair<uint64_t, fe>> points;
    std::string msg;
    // the points read so far are the caller's also when the proof is rejected (the reference's
    // polynomial_values is an out-parameter)
    auto publish = [&] {
      for (size_t i = 0; i < points.size(); ++i) {
        if (indices) indices[i] = (size_t)points[i].first;
        if (values) values[i] = from_fe(points[i].second);
      }
    };
    try {
      verdict = verify_in_order(ctx, q, msg, [&](std::string& m) { return fri_verify_walk(ctx, fri, in, q, "", points, m); });
    } catch (...) {
      publish();
      throw;
    }
    publish();
    ctx->last_error = verdict ? "" : msg;
  });
  return rc < 0 ? rc : verdict;
}
