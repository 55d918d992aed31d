// RPSSS, the Rescue-Prime STARK signature scheme (rpsss.rs): the reference's one application, as
// an object over the library's own entry points.  It owns RescuePrime::new(field, 2, 1, security,
// 27), the Stark over its trace shape and the m transition constraints -- built once here, where
// the reference rebuilds them for every sign and verify (rpsss.rs:46,57) -- and composes
// sg_rescue_trace, sg_stark_prove, sg_stream_deserialize's parser and sg_stark_verify; nothing of
// the prover or the verifier is forked.  The thread_rng draws are explicit inputs.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_field.hpp"
#include "internal.hpp"
#include "transcript.hpp"

using namespace sg;

struct sg_rpsss {
  sg_rescue* rp = nullptr;
  sg_stark* st = nullptr;
  std::vector<sg_mpoly*> tcs;
  size_t m = 0, N = 0, num_randomizers = 0, n_rc = 0;
  ~sg_rpsss() {
    for (sg_mpoly* t : tcs) sg_mpoly_free(t);
    sg_stark_free(st);
    sg_rescue_free(rp);
  }
};

namespace {

constexpr size_t kSeedBytes = 17;  // rpsss.rs:62-66: bytes_per_int of the field + 1

// an inner entry point's failure, with the message it left
void inner(int rc, sg_ctx* ctx) {
  if (rc < 0) throw Error{rc, ctx ? ctx->last_error : host_last_error()};
}

struct StreamDeleter {
  void operator()(sg_stream* s) const { sg_stream_destroy(s); }
};
using StreamPtr = std::unique_ptr<sg_stream, StreamDeleter>;

}  // namespace

extern "C" int sg_rpsss_create(sg_ctx* ctx, size_t expansion_factor, size_t num_colinearity_checks,
                               size_t security_level, size_t transition_constraints_degree, sg_rpsss** out) {
  return guard(ctx, [&] {
    set_device(ctx);  // the constraints are interpolated on the device
    SG_REQUIRE(out, "null argument");
    std::unique_ptr<sg_rpsss> r(new sg_rpsss());
    r->m = 2;
    r->N = 27;
    inner(sg_rescue_create(ctx, r->m, 1, security_level, r->N, &r->rp), ctx);
    inner(sg_stark_create(ctx, expansion_factor, num_colinearity_checks, security_level, r->m, r->N + 1,
                          transition_constraints_degree, &r->st),
          ctx);
    sg_fe omicron;
    uint64_t D = 0;
    inner(sg_stark_params(r->st, &omicron, &D, nullptr, &r->num_randomizers), ctx);
    r->tcs.assign(r->m, nullptr);
    inner(sg_rescue_transition_constraints(ctx, r->rp, omicron, D, r->tcs.data()), ctx);
    uint64_t max_degree = 0;
    inner(sg_stark_max_degree(ctx, r->st, r->tcs.data(), r->tcs.size(), &max_degree), ctx);
    r->n_rc = (size_t)max_degree + 1;
    *out = r.release();
  });
}

extern "C" void sg_rpsss_free(sg_rpsss* r) { delete r; }

extern "C" int sg_rpsss_params(const sg_rpsss* r, size_t* n_trace_randomizers, size_t* n_randomizer_coeffs) {
  if (!r) return SG_ERR_INVALID;
  if (n_trace_randomizers) *n_trace_randomizers = r->num_randomizers * r->m;
  if (n_randomizer_coeffs) *n_randomizer_coeffs = r->n_rc;
  return SG_OK;
}

extern "C" int sg_rpsss_keygen_batch(sg_ctx* ctx, const sg_rpsss* r, const uint8_t* seeds, size_t n, sg_fe* sk,
                                     sg_fe* pk) {
  return guard(ctx, [&] {
    SG_REQUIRE(r && (!n || (seeds && sk && pk)), "null argument");
    for (size_t i = 0; i < n; ++i) sk[i] = from_fe(fe_sample(seeds + kSeedBytes * i, kSeedBytes));
    inner(sg_rescue_hash_batch(ctx, r->rp, sk, n, pk), ctx);
  });
}

extern "C" int sg_rpsss_keygen(sg_ctx* ctx, const sg_rpsss* r, const uint8_t seed[17], sg_fe* sk, sg_fe* pk) {
  return guard(ctx, [&] {
    SG_REQUIRE(r && seed && sk && pk, "null argument");
    *sk = from_fe(fe_sample(seed, kSeedBytes));
    inner(sg_rescue_hash(ctx, r->rp, *sk, pk), ctx);  // one chain: the host
  });
}

extern "C" int sg_rpsss_sign(sg_ctx* ctx, const sg_rpsss* r, sg_fe sk, const uint8_t* document, size_t doc_len,
                             const sg_fe* trace_randomizers, const sg_fe* randomizer_coeffs, size_t n_rc,
                             sg_stream** out) {
  return guard(ctx, [&] {
    set_device(ctx);
    SG_REQUIRE(r && out && (document || !doc_len), "null argument");
    // rpsss.rs:38-49: the trace of sk; its last row's first register is pk = hash(sk)
    std::vector<sg_fe> trace((r->N + 1) * r->m);
    inner(sg_rescue_trace(ctx, r->rp, sk, trace.data()), ctx);
    sg_boundary bnd[2];
    inner(sg_rescue_boundary_constraints(r->rp, trace[r->N * r->m], bnd), ctx);
    StreamPtr s(sg_stream_create_signature(document, doc_len));
    if (!s) throw std::bad_alloc();
    const sg_proof_stream ps = sg_stream_callbacks(s.get());
    inner(sg_stark_prove(ctx, r->st, trace.data(), r->N + 1, r->tcs.data(), r->tcs.size(), bnd, 2,
                         trace_randomizers, randomizer_coeffs, n_rc, &ps),
          ctx);
    *out = s.release();
  });
}

extern "C" int sg_rpsss_verify(sg_ctx* ctx, const sg_rpsss* r, sg_fe pk, const uint8_t* document, size_t doc_len,
                               const uint8_t* signature, size_t sig_len) {
  int verdict = 0;
  const int rc = guard(ctx, [&] {
    set_device(ctx);
    SG_REQUIRE(r && (document || !doc_len) && signature, "null argument");
    // rpsss.rs:51-59: the signature's objects (stark.rs:30-67) behind the document's prefix
    StreamPtr s(sg_stream_create_signature(document, doc_len));
    if (!s) throw std::bad_alloc();
    std::string err;
    SG_REQUIRE(deserialize_stream(signature, sig_len, s->s, err), "malformed signature: " + err);
    sg_boundary bnd[2];
    inner(sg_rescue_boundary_constraints(r->rp, pk, bnd), ctx);
    const sg_verifier_stream vs = sg_stream_verifier_callbacks(s.get());
    verdict = sg_stark_verify(ctx, r->st, r->tcs.data(), r->tcs.size(), bnd, 2, &vs);
    inner(verdict, ctx);
  });
  return rc < 0 ? rc : verdict;
}
