// Sparse R1CS on the device (include/gosnark_hip.h, "R1CS"): upload, and witness -> constraint values -> ax, bx, cx, px.
#include "prove.h"
#include "domain.h"
#include "scan.h"
#include "r1cs_solve.h"
#include "solve_plan.h"

#include <algorithm>

using namespace gs;

// Sparse R1CS + witness -> ax, bx, cx, px = ax * bx - cx: the scalable replacement of the dense
// R1CSToQAP + CombinePolynomials pair (r1csqap.go:161-210).  CombinePolynomials' ax = sum_i w_i alpha_i(x) is the
// interpolant of the values (A w)_j at the nodes j = 1..n, so the m x n coefficient matrices are never formed.
static const char* validate_csr(size_t n, size_t m, const uint32_t* rowptr, const uint32_t* col, const uint64_t* val) {
  if (!rowptr) return "null row_ptr";
  if (rowptr[0] != 0) return "row_ptr[0] must be 0";
  for (size_t r = 0; r < n; ++r) if (rowptr[r + 1] < rowptr[r]) return "row_ptr not monotone";
  const size_t nnz = rowptr[n];
  if (nnz && (!col || !val)) return "null column/value array";
  for (size_t e = 0; e < nnz; ++e) if (col[e] >= m) return "column index out of range";
  return nullptr;
}

static int r1cs_upload_impl(Ctx& c, size_t n, size_t m, const uint32_t* const rp[3], const uint32_t* const cl[3], const uint64_t* const vl[3],
                            R1csObj& o) {
  if (n == 0 || m == 0) return fail(GS_ERR_ARG, "empty R1CS");
  if (n >= (1ull << 26) || m >= (1ull << 31)) return fail(GS_ERR_ARG, "R1CS too large");
  for (int k = 0; k < 3; ++k)
    if (const char* e = validate_csr(n, m, rp[k], cl[k], vl[k])) return fail(GS_ERR_ARG, "R1CS matrix %c: %s", "ABC"[k], e);
  o.n = n; o.m = m;
  for (int k = 0; k < 3; ++k) {
    const size_t nnz = rp[k][n];
    o.nnz[k] = nnz;
    o.rowptr[k].alloc((n + 1) * 4);
    o.col[k].alloc(std::max<size_t>(nnz, 1) * 4);
    o.val[k].alloc(std::max<size_t>(nnz, 1) * 32);
    GS_HIP(hipMemcpyAsync(o.rowptr[k].p, rp[k], (n + 1) * 4, hipMemcpyHostToDevice, c.stream));
    if (nnz) {
      GS_HIP(hipMemcpyAsync(o.col[k].p, cl[k], nnz * 4, hipMemcpyHostToDevice, c.stream));
      GS_HIP(hipMemcpyAsync(o.val[k].p, vl[k], nnz * 32, hipMemcpyHostToDevice, c.stream));
    }
  }
  GS_HIP(hipStreamSynchronize(c.stream));
  return GS_OK;
}

// w (standard form, m elements, device) -> o.vals = [A w | B w | C w] (o.points() each, standard form): the values of ax, bx, cx at the
// nodes 1..n (CombinePolynomials' sum_i w_i alpha_i(x) evaluated there, r1csqap.go:191-210) -- or, for a domain R1CS, at omega^0 ..
// omega^(n-1), followed by the zeros of the empty rows up to 2^k
void gs::r1cs_values_dev(Ctx& c, R1csObj& o, const uint32_t* w_dev) { r1cs_values_into_dev(c, o, w_dev, o.w_mont, o.vals); }
// The same stage into workspaces the caller names (grown here): gs_r1cs_check keeps its own pair, because o.w_mont and o.vals belong to
// the polynomial stage of the proofs in flight on this system.
void gs::r1cs_values_into_dev(Ctx& c, R1csObj& o, const uint32_t* w_dev, DevBuf& w_mont, DevBuf& vals) {
  const size_t n = o.n, m = o.m, np = o.points();
  w_mont.ensure(m * 32); vals.ensure(3 * np * 32);
  GS_HIP(hipMemcpyAsync(w_mont.p, w_dev, m * 32, hipMemcpyDeviceToDevice, c.stream));
  poly_canon_dev(c, w_mont.as<uint32_t>(), m, 1);                                           // w -> Montgomery
  for (int k = 0; k < (o.product ? 2 : 3); ++k) {
    uint32_t* out = vals.as<uint32_t>() + k * np * 8;
    spmv_dev(c, o.rowptr[k].as<uint32_t>(), o.col[k].as<uint32_t>(), o.val[k].as<uint32_t>(), w_mont.as<uint32_t>(), n, m, out);
    if (np > n) GS_HIP(hipMemsetAsync(out + n * 8, 0, (np - n) * 32, c.stream));
  }
  // a product system: [A w | B w | a o b], the third vector by one point-wise kernel (not fused into the first transform pass: that
  // pass is shared with every other caller of ntt_forward_n, and the vector is 32 B per point against the three transforms' 6 passes)
  if (o.product) r1cs_product_dev(c, vals.as<uint32_t>(), np);
}

// w -> o.coef = [ax | bx | cx] (o.points() each) and px_out (o.npx()), canonical standard form
void gs::r1cs_px_dev(Ctx& c, R1csObj& o, const uint32_t* w_dev, uint32_t* px_out) {
  const size_t n = o.points(), npx = o.npx();
  r1cs_values_dev(c, o, w_dev);
  o.coef.ensure(3 * n * 32); o.prod.ensure(npx * 32);
  if (o.domain_log2) domain_coeffs_dev(c, o.vals.as<uint32_t>(), o.domain_log2, 3, o.coef.as<uint32_t>());   // one transform each (domain.h)
  else interpolate_dev(c, o.vals.as<uint32_t>(), n, 3, o.coef.as<uint32_t>());
  uint32_t* A = o.coef.as<uint32_t>();
  uint32_t* B = A + n * 8;
  uint32_t* C = B + n * 8;
  poly_mul_dev(c, A, n, Form::Std, B, n, Form::Std, o.prod.as<uint32_t>());
  poly_addsub_dev(c, o.prod.as<uint32_t>(), npx, C, n, true, px_out);
  poly_canon_dev(c, px_out, npx, 0);
  poly_canon_dev(c, A, 3 * n, 0);
}

extern "C" {

int gs_r1cs_to_px(size_t n, size_t m,
                  const uint32_t* a_rowptr, const uint32_t* a_col, const uint64_t* a_val,
                  const uint32_t* b_rowptr, const uint32_t* b_col, const uint64_t* b_val,
                  const uint32_t* c_rowptr, const uint32_t* c_col, const uint64_t* c_val,
                  const uint64_t* w, uint64_t* ax, uint64_t* bx, uint64_t* cx, uint64_t* px) {
  return guarded([&](Ctx& c) -> int {
    if (!w || !px) return fail(GS_ERR_ARG, "gs_r1cs_to_px: null argument");
    const uint32_t* rp[3] = {a_rowptr, b_rowptr, c_rowptr};
    const uint32_t* cl[3] = {a_col, b_col, c_col};
    const uint64_t* vl[3] = {a_val, b_val, c_val};
    R1csObj o;
    const int rc = r1cs_upload_impl(c, n, m, rp, cl, vl, o);
    if (rc != GS_OK) return rc;
    const size_t npx = 2 * n - 1;
    const uint32_t* dw = upload_tmp(c, prove_state(c).up_w, w, m);
    prove_state(c).up_o.ensure(npx * 32);
    r1cs_px_dev(c, o, dw, prove_state(c).up_o.as<uint32_t>());
    const uint32_t* A = o.coef.as<uint32_t>();
    if (ax) GS_HIP(hipMemcpyAsync(ax, A, n * 32, hipMemcpyDeviceToHost, c.stream));
    if (bx) GS_HIP(hipMemcpyAsync(bx, A + n * 8, n * 32, hipMemcpyDeviceToHost, c.stream));
    if (cx) GS_HIP(hipMemcpyAsync(cx, A + 2 * n * 8, n * 32, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipMemcpyAsync(px, prove_state(c).up_o.p, npx * 32, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    return GS_OK;
  });
}

// The per-circuit / per-proof split of the same computation: the R1CS is uploaded and validated once ...
int gs_r1cs_upload(size_t n, size_t m,
                   const uint32_t* a_rowptr, const uint32_t* a_col, const uint64_t* a_val,
                   const uint32_t* b_rowptr, const uint32_t* b_col, const uint64_t* b_val,
                   const uint32_t* c_rowptr, const uint32_t* c_col, const uint64_t* c_val, gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    if (!out) return fail(GS_ERR_ARG, "gs_r1cs_upload: null output");
    const uint32_t* rp[3] = {a_rowptr, b_rowptr, c_rowptr};
    const uint32_t* cl[3] = {a_col, b_col, c_col};
    const uint64_t* vl[3] = {a_val, b_val, c_val};
    auto o = std::make_unique<R1csObj>();
    const int rc = r1cs_upload_impl(c, n, m, rp, cl, vl, *o);
    if (rc != GS_OK) return rc;
    *out = c.put(std::move(o));
    return GS_OK;
  });
}

// The same system as a QAP over the domain of the 2^log2_domain-th roots of unity (domain.h): what snarkjs / circom keys are built on.
int gs_r1cs_upload_domain(size_t log2_domain, size_t n, size_t m,
                          const uint32_t* a_rowptr, const uint32_t* a_col, const uint64_t* a_val,
                          const uint32_t* b_rowptr, const uint32_t* b_col, const uint64_t* b_val,
                          const uint32_t* c_rowptr, const uint32_t* c_col, const uint64_t* c_val, gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    if (!out) return fail(GS_ERR_ARG, "gs_r1cs_upload_domain: null output");
    if (log2_domain < 1 || log2_domain > (size_t)kDomainMaxLog2)
      return fail(GS_ERR_ARG, "gs_r1cs_upload_domain: log2_domain = %zu, must be 1 .. %d", log2_domain, kDomainMaxLog2);
    if (n > ((size_t)1 << log2_domain))
      return fail(GS_ERR_SHAPE, "gs_r1cs_upload_domain: %zu constraints do not fit the domain of 2^%zu points", n, log2_domain);
    const uint32_t* rp[3] = {a_rowptr, b_rowptr, c_rowptr};
    const uint32_t* cl[3] = {a_col, b_col, c_col};
    const uint64_t* vl[3] = {a_val, b_val, c_val};
    auto o = std::make_unique<R1csObj>();
    const int rc = r1cs_upload_impl(c, n, m, rp, cl, vl, *o);
    if (rc != GS_OK) return rc;
    o->domain_log2 = (int)log2_domain;
    *out = c.put(std::move(o));
    return GS_OK;
  });
}

// ... and every proof only turns its resident witness into the resident px (nothing crosses PCIe).  *px_inout: 0 to create the
// 2n - 1 coefficient vector, or a handle from an earlier call to overwrite.
int gs_r1cs_px(gs_handle hr1cs, gs_handle hw, gs_handle* px_inout) {
  return guarded([&](Ctx& c) -> int {
    R1csObj* o = c.get<R1csObj>(hr1cs, Kind::R1cs);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    if (!o || !w || !px_inout) return fail(GS_ERR_ARG, "gs_r1cs_px: bad handle");
    if (w->n != o->m) return fail(GS_ERR_SHAPE, "len(w) = %zu but the system has %zu variables", w->n, o->m);
    const size_t npx = o->npx();
    Scalars* px = inout_scalars(c, px_inout, npx, "%s: the px handle does not hold 2n - 1 = %zu coefficients", "gs_r1cs_px");
    if (!px) return GS_ERR_ARG;
    // On the stream that carries every proof's polynomial stage: stream order keeps the engine's workspaces consistent, so
    // the px of proof k+1 may be computed while proofs are in flight (it queues behind their H(x), not behind their MSMs).
    StreamScope sc(c, c.aux_stream[1]);
    PhaseTimer t(c.stream);
    r1cs_px_dev(c, *o, w->buf.as<uint32_t>(), px->buf.as<uint32_t>());
    t.stop();
    GS_HIP(hipStreamSynchronize(c.stream));
    if (!c.any_inflight()) reset_timing(c);
    c.timing.poly_ms = t.ms();
    c.timing.total_ms = c.timing.poly_ms;
    return GS_OK;
  }, true, true, hr1cs);
}

// Which constraints does a resident witness break?  All n rows, not the roots of a key's Z; no key needed (include/gosnark_hip.h).
// Runs beside proofs in flight (allow_inflight): on the polynomial stream like gs_r1cs_px -- never the accumulation stream; spmv_dev's
// hand-off list of long rows is shared with the proofs' polynomial stages, and stream order keeps it consistent -- but in workspaces
// of its own (R1csObj::chk_*), since o.vals of a proof in flight is still read after this call was enqueued.  The call waits for its
// own stream position only, so when it returns the device has finished reading w: like every blocking entry point it leaves no read
// mark on the vector (runtime.h, Scalars), and a gs_scalars_update that follows cannot overtake it.
int gs_r1cs_check(gs_handle hr1cs, gs_handle hw, size_t cap, uint64_t* nviolated, uint32_t* rows, uint64_t* values) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_r1cs_check";
    if (!nviolated) return fail(GS_ERR_ARG, "%s: null nviolated", fn);
    if (cap && !rows) return fail(GS_ERR_ARG, "%s: cap = %zu but rows is null", fn, cap);
    R1csObj* o = c.get<R1csObj>(hr1cs, Kind::R1cs);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    if (!o || !w) return fail(GS_ERR_ARG, "%s: bad handle (an R1CS and a scalar vector of the same logical device)", fn);
    if (o->product)
      return fail(GS_ERR_SHAPE, "%s: a .zkey key's system holds A and B only, no C (c = a b by definition): the check needs the three "
                                "matrices of circuit.r1cs (gs_r1cs_upload / gs_r1cs_upload_domain)", fn);
    if (w->n != o->m) return fail(GS_ERR_SHAPE, "len(w) = %zu but the system has %zu variables", w->n, o->m);
    const size_t n = o->n, capd = std::min(cap, n);
    o->chk_pos.ensure((n + 1) * 4);
    o->chk_tiles.ensure((size_t)scan_tiles(n + 1) * 4);
    if (capd) { o->chk_rows.ensure(capd * 4); o->chk_values.ensure(capd * 96); }
    uint32_t* pos = o->chk_pos.as<uint32_t>();
    StreamScope sc(c, c.aux_stream[1]);
    PhaseTimer total(c.stream), tvals(c.stream);
    r1cs_values_into_dev(c, *o, w->buf.as<uint32_t>(), o->chk_w_mont, o->chk_vals);
    tvals.stop();
    PhaseTimer trows(c.stream);
    r1cs_check_rows_dev(c, o->chk_vals.as<uint32_t>(), n, o->points(), pos, o->chk_tiles.as<uint32_t>(), capd, o->chk_rows.as<uint32_t>(),
                        o->chk_values.as<uint32_t>());
    trows.stop();
    uint32_t count = 0;
    GS_HIP(hipMemcpyAsync(&count, pos + n, 4, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    const size_t k = std::min<size_t>(count, capd);           // nothing at and beyond it is written
    if (k) {
      GS_HIP(hipMemcpyAsync(rows, o->chk_rows.p, k * 4, hipMemcpyDeviceToHost, c.stream));
      if (values) GS_HIP(hipMemcpyAsync(values, o->chk_values.p, k * 96, hipMemcpyDeviceToHost, c.stream));
    }
    total.stop();
    GS_HIP(hipStreamSynchronize(c.stream));
    *nviolated = count;
    if (!c.any_inflight()) reset_timing(c);
    c.timing.poly_ms = tvals.ms();
    c.timing.reduce_ms = trows.ms();
    c.timing.total_ms = total.ms();                           // with the result copies: gs_timing has no field for them
    return GS_OK;
  }, true, true, hr1cs);
}

// ---- witnesses solved from the system (include/gosnark_hip.h; solve_plan.h, r1cs_solve.hip) -----------------------------------------
// The plan is made on the host from the system's CSR arrays, which are read back from the device once, here (uploads keep no host
// copy: most systems are never solved).  The arrays are immutable after the upload, so the copies need no ordering against proofs in
// flight; they go on the polynomial stream like everything else of the solver.
int gs_r1cs_solve_plan(gs_handle hr1cs, const uint32_t* input_vars, size_t ninputs, const gs_solve_opts* opts, gs_handle* plan_out,
                       gs_solve_stats* stats) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_r1cs_solve_plan";
    if (!plan_out) return fail(GS_ERR_ARG, "%s: null plan", fn);
    if (ninputs && !input_vars) return fail(GS_ERR_ARG, "%s: ninputs = %zu but input_vars is null", fn, ninputs);
    std::shared_ptr<R1csObj> o = c.share<R1csObj>(hr1cs, Kind::R1cs);
    if (!o) return fail(GS_ERR_ARG, "%s: bad handle (an R1CS)", fn);
    if (o->product)
      return fail(GS_ERR_SHAPE, "%s: a .zkey key's system holds A and B only, no C (c = a b by definition): the solver needs the three "
                                "matrices of circuit.r1cs (gs_r1cs_upload / gs_r1cs_upload_domain)", fn);
    const size_t n = o->n, m = o->m;
    StreamScope sc(c, c.aux_stream[1]);
    std::vector<uint32_t> rp[3], cl[3];
    std::vector<uint64_t> vl[3];
    SolveCsr mat[3];
    for (int k = 0; k < 3; ++k) {
      const size_t nnz = o->nnz[k];
      rp[k].resize(n + 1); cl[k].resize(std::max<size_t>(nnz, 1)); vl[k].resize(std::max<size_t>(nnz, 1) * 4);
      GS_HIP(hipMemcpyAsync(rp[k].data(), o->rowptr[k].p, (n + 1) * 4, hipMemcpyDeviceToHost, c.stream));
      if (nnz) {
        GS_HIP(hipMemcpyAsync(cl[k].data(), o->col[k].p, nnz * 4, hipMemcpyDeviceToHost, c.stream));
        GS_HIP(hipMemcpyAsync(vl[k].data(), o->val[k].p, nnz * 32, hipMemcpyDeviceToHost, c.stream));
      }
      mat[k] = SolveCsr{rp[k].data(), cl[k].data(), vl[k].data()};
    }
    GS_HIP(hipStreamSynchronize(c.stream));
    SolvePlan hp;
    size_t bad = 0;
    switch (plan_solve_levels(mat, n, m, input_vars, ninputs, hp, &bad)) {
      case kSpOk: break;
      case kSpInputRange: return fail(GS_ERR_ARG, "%s: input_vars[%zu] = %u but the system has %zu variables", fn, bad, input_vars[bad], m);
      case kSpInputZero: return fail(GS_ERR_ARG, "%s: input_vars[%zu] = 0: variable 0 is the constant one, not an input", fn, bad);
      case kSpInputTwice: return fail(GS_ERR_ARG, "%s: input_vars[%zu] = %u is listed twice", fn, bad, input_vars[bad]);
    }
    auto p = std::make_unique<SolvePlanObj>();
    p->sys = o;
    p->ninputs = ninputs;
    const size_t ns = p->nsolved = hp.entries.size();
    SolveOptions so;
    if (opts) { so.narrow = opts->narrow; so.run_max_rows = opts->run_max_rows; }
    std::vector<SolveLaunch> launches;
    plan_solve_launches(hp.level_off, so, launches);
    std::vector<uint32_t> targets(ns), forms(ns), elems(ns * 8);
    p->host_rows.resize(ns);
    for (size_t i = 0; i < ns; ++i) {
      p->host_rows[i] = hp.entries[i].row; targets[i] = hp.entries[i].target; forms[i] = hp.entries[i].form;
      memcpy(&elems[i * 8], hp.entries[i].elem, 32);
    }
    p->rows.alloc(ns * 4); p->targets.alloc(ns * 4); p->forms.alloc(ns * 4); p->elems.alloc(ns * 32);
    p->input_vars.alloc(ninputs * 4);
    if (ns) {
      GS_HIP(hipMemcpyAsync(p->rows.p, p->host_rows.data(), ns * 4, hipMemcpyHostToDevice, c.stream));
      GS_HIP(hipMemcpyAsync(p->targets.p, targets.data(), ns * 4, hipMemcpyHostToDevice, c.stream));
      GS_HIP(hipMemcpyAsync(p->forms.p, forms.data(), ns * 4, hipMemcpyHostToDevice, c.stream));
      GS_HIP(hipMemcpyAsync(p->elems.p, elems.data(), ns * 32, hipMemcpyHostToDevice, c.stream));
    }
    if (ninputs) GS_HIP(hipMemcpyAsync(p->input_vars.p, input_vars, ninputs * 4, hipMemcpyHostToDevice, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    gs_solve_stats& st = p->stats;
    st.solved = ns; st.unsolved = hp.unsolved.size(); st.checks = hp.checks; st.stuck = hp.stuck;
    st.levels = hp.level_off.size() - 1; st.launches = launches.size();
    for (const SolveLaunch& l : launches) {
      p->launches.push_back(SolvePlanObj::Launch{l.lo, l.hi, l.run});
      st.wide_launches += !l.run;
    }
    for (size_t l = 0; l + 1 < hp.level_off.size(); ++l) st.widest_level = std::max<uint64_t>(st.widest_level, hp.level_off[l + 1] - hp.level_off[l]);
    p->unsolved = std::move(hp.unsolved);
    if (stats) *stats = st;
    *plan_out = c.put(std::move(p));
    return GS_OK;
  }, true, true, hr1cs);
}

int gs_r1cs_solve_unsolved(gs_handle hplan, size_t cap, uint32_t* vars, uint64_t* count) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_r1cs_solve_unsolved";
    SolvePlanObj* p = c.get<SolvePlanObj>(hplan, Kind::SolvePlan);
    if (!p) return fail(GS_ERR_ARG, "%s: bad handle (a plan of gs_r1cs_solve_plan)", fn);
    if (!count) return fail(GS_ERR_ARG, "%s: null count", fn);
    if (cap && !vars) return fail(GS_ERR_ARG, "%s: cap = %zu but vars is null", fn, cap);
    const size_t k = std::min(cap, p->unsolved.size());
    if (k) memcpy(vars, p->unsolved.data(), k * 4);
    *count = p->unsolved.size();
    return GS_OK;
  }, true, true, hplan);
}

// Runs beside proofs in flight like gs_r1cs_check: on the polynomial stream, in workspaces the plan owns, waiting only for itself.
// The vectors it overwrites may still be read by pipelined operations: the stream first waits for their read marks (runtime.h,
// Scalars), as gs_scalars_update's copy does.  When the call returns the device has finished with every vector, so it leaves no mark.
int gs_r1cs_solve(gs_handle hplan, size_t nwit, const uint64_t* inputs, gs_handle* w_inout, uint64_t* nfailed, uint32_t* first_failed_row) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_r1cs_solve";
    SolvePlanObj* p = c.get<SolvePlanObj>(hplan, Kind::SolvePlan);
    if (!p) return fail(GS_ERR_ARG, "%s: bad handle (a plan of gs_r1cs_solve_plan)", fn);
    if (!nwit || nwit >= (1ull << 31)) return fail(GS_ERR_ARG, "%s: nwit = %zu", fn, nwit);
    if (!w_inout || !nfailed || !first_failed_row || (p->ninputs && !inputs)) return fail(GS_ERR_ARG, "%s: null argument", fn);
    R1csObj& o = *p->sys;
    const size_t m = o.m;
    std::vector<Scalars*> vec(nwit, nullptr);
    for (size_t b = 0; b < nwit; ++b) {
      if (!w_inout[b]) continue;
      vec[b] = c.get<Scalars>(w_inout[b], Kind::Scalars);
      if (!vec[b]) return fail(GS_ERR_ARG, "%s: w_inout[%zu] is not a scalar vector of the plan's logical device", fn, b);
      if (vec[b]->n != m) return fail(GS_ERR_SHAPE, "%s: w_inout[%zu] holds %zu elements but the system has %zu variables", fn, b, vec[b]->n, m);
    }
    {
      std::vector<Scalars*> sorted;
      for (Scalars* s : vec) if (s) sorted.push_back(s);
      std::sort(sorted.begin(), sorted.end());
      if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(GS_ERR_ARG, "%s: a vector is listed twice in w_inout", fn);
    }
    // every allocation before the first handle is given out: a call that fails for memory leaves w_inout as it was
    std::vector<std::unique_ptr<Scalars>> fresh;
    for (size_t b = 0; b < nwit; ++b) {
      if (vec[b]) continue;
      fresh.push_back(std::make_unique<Scalars>());
      fresh.back()->n = m;
      fresh.back()->buf.alloc(m * 32);
      vec[b] = fresh.back().get();
    }
    p->ws_ptrs.ensure(nwit * sizeof(uint32_t*));
    p->ws_fail.ensure(nwit * 8);
    p->ws_inputs.ensure(std::max<size_t>(nwit * p->ninputs, 1) * 32);
    std::vector<uint32_t*> ptrs(nwit);
    for (size_t b = 0; b < nwit; ++b) ptrs[b] = vec[b]->buf.as<uint32_t>();
    std::vector<uint32_t> fail_host(nwit * 2);

    StreamScope sc(c, c.aux_stream[1]);
    for (Scalars* s : vec) for (auto& r : s->reads) GS_HIP(hipStreamWaitEvent(c.stream, r.ev, 0));
    PhaseTimer total(c.stream), th(c.stream);
    GS_HIP(hipMemcpyAsync(p->ws_ptrs.p, ptrs.data(), nwit * sizeof(uint32_t*), hipMemcpyHostToDevice, c.stream));
    if (p->ninputs) GS_HIP(hipMemcpyAsync(p->ws_inputs.p, inputs, nwit * p->ninputs * 32, hipMemcpyHostToDevice, c.stream));
    th.stop();
    uint32_t* const* wtab = p->ws_ptrs.as<uint32_t*>();
    uint32_t* fail_dev = p->ws_fail.as<uint32_t>();
    SolveDev d;
    for (int k = 0; k < 3; ++k) { d.rowptr[k] = o.rowptr[k].as<uint32_t>(); d.col[k] = o.col[k].as<uint32_t>(); d.val[k] = o.val[k].as<uint32_t>(); }
    d.rows = p->rows.as<uint32_t>(); d.targets = p->targets.as<uint32_t>(); d.forms = p->forms.as<uint32_t>(); d.elems = p->elems.as<uint32_t>();
    d.m = (uint32_t)m;
    PhaseTimer tsolve(c.stream);
    solve_begin_dev(c, wtab, nwit, m, p->ws_inputs.as<uint32_t>(), p->input_vars.as<uint32_t>(), p->ninputs, fail_dev);
    for (const SolvePlanObj::Launch& l : p->launches) {
      if (l.run) solve_run_dev(c, d, l.lo, l.hi, wtab, nwit, fail_dev);
      else solve_level_dev(c, d, l.lo, l.hi, wtab, nwit, fail_dev);
    }
    solve_finish_dev(c, wtab, nwit, m);
    tsolve.stop();
    GS_HIP(hipMemcpyAsync(fail_host.data(), fail_dev, nwit * 8, hipMemcpyDeviceToHost, c.stream));
    total.stop();
    GS_HIP(hipStreamSynchronize(c.stream));
    for (size_t b = 0, f = 0; b < nwit; ++b) {
      nfailed[b] = fail_host[2 * b];
      const uint32_t pos = fail_host[2 * b + 1];
      first_failed_row[b] = pos < p->host_rows.size() ? p->host_rows[pos] : 0xffffffffu;
      if (!w_inout[b]) w_inout[b] = c.put(std::move(fresh[f++]));
    }
    if (!c.any_inflight()) reset_timing(c);
    c.timing.h2d_ms = th.ms();
    c.timing.poly_ms = tsolve.ms();
    c.timing.total_ms = total.ms();
    return GS_OK;
  }, true, true, hplan);
}

int gs_solve_abi_sizes(size_t* opts_bytes, size_t* stats_bytes) {
  if (opts_bytes) *opts_bytes = sizeof(gs_solve_opts);
  if (stats_bytes) *stats_bytes = sizeof(gs_solve_stats);
  return GS_OK;
}

}  // extern "C"
