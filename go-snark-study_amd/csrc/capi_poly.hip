// The extern "C" polynomial entry points (include/gosnark_hip.h, "polynomial field"): host operands in, host result out, staged
// through the context's upload buffers.
#include "prove.h"

#include <algorithm>

using namespace gs;

extern "C" {

// ---- polynomial field ------------------------------------------------------------------------------------
int gs_poly_mul(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out) {
  return guarded([&](Ctx& c) -> int {
    if (!a || !b || !out || na == 0 || nb == 0) return fail(GS_ERR_ARG, "gs_poly_mul: empty or null operand");
    if (na + nb > (1ull << 27)) return fail(GS_ERR_ARG, "gs_poly_mul: product too large");
    const uint32_t* da = upload_tmp(c, prove_state(c).up_a, a, na);
    const uint32_t* db = upload_tmp(c, prove_state(c).up_b, b, nb);
    const size_t nr = na + nb - 1;
    prove_state(c).up_o.ensure(nr * 32);
    poly_mul_dev(c, da, na, Form::Std, db, nb, Form::Std, prove_state(c).up_o.as<uint32_t>());
    poly_canon_dev(c, prove_state(c).up_o.as<uint32_t>(), nr, 0);
    download(c, out, prove_state(c).up_o.p, nr);
    return GS_OK;
  });
}

int gs_poly_div(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* quo, uint64_t* rem) {
  return guarded([&](Ctx& c) -> int {
    if (!a || !b || !quo || nb == 0 || na < nb) return fail(GS_ERR_ARG, "gs_poly_div: need len(a) >= len(b) >= 1");
    bool lead_zero = true;
    for (int i = 0; i < 4; ++i) lead_zero = lead_zero && b[4 * (nb - 1) + i] == 0;
    if (lead_zero) return fail(GS_ERR_ARG, "gs_poly_div: leading coefficient of the divisor is zero");
    const uint32_t* da = upload_tmp(c, prove_state(c).up_a, a, na);
    const uint32_t* db = upload_tmp(c, prove_state(c).up_b, b, nb);
    Divisor d;
    divisor_init(c, d, db, nb);
    const size_t nq = na - nb + 1;
    prove_state(c).up_o.ensure((nq + na + nb) * 32);
    uint32_t* q = prove_state(c).up_o.as<uint32_t>();
    poly_quotient_dev(c, d, da, na, q);
    if (rem && nb > 1) {
      // rem = (a - q b) mod x^(nb-1)        (r1csqap.go:70-84 returns the final `rem`)
      uint32_t* qb = q + nq * 8;
      poly_mul_dev(c, q, nq, Form::Std, db, nb, Form::Std, qb);
      uint32_t* rr = qb + (nq + nb - 1) * 8;              // up_o holds nq + (nq + nb - 1) + (nb - 1) <= nq + na + nb elements: no allocation here
      poly_addsub_dev(c, da, nb - 1, qb, nb - 1, true, rr);
      poly_canon_dev(c, rr, nb - 1, 0);
      GS_HIP(hipMemcpyAsync(rem, rr, (nb - 1) * 32, hipMemcpyDeviceToHost, c.stream));
      GS_HIP(hipStreamSynchronize(c.stream));
    }
    poly_canon_dev(c, q, nq, 0);
    download(c, quo, q, nq);
    return GS_OK;
  });
}

static int addsub_api(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out, bool sub) {
  return guarded([&](Ctx& c) -> int {
    if ((na && !a) || (nb && !b) || !out) return fail(GS_ERR_ARG, "null operand");
    const size_t n = std::max(na, nb);
    if (n == 0) return GS_OK;
    const uint32_t* da = upload_tmp(c, prove_state(c).up_a, a, na);
    const uint32_t* db = upload_tmp(c, prove_state(c).up_b, b, nb);
    prove_state(c).up_o.ensure(n * 32);
    poly_addsub_dev(c, da, na, db, nb, sub, prove_state(c).up_o.as<uint32_t>());
    poly_canon_dev(c, prove_state(c).up_o.as<uint32_t>(), n, 0);
    download(c, out, prove_state(c).up_o.p, n);
    return GS_OK;
  });
}
int gs_poly_add(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out) { return addsub_api(a, na, b, nb, out, false); }
int gs_poly_sub(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out) { return addsub_api(a, na, b, nb, out, true); }

int gs_poly_eval(const uint64_t* v, size_t n, const uint64_t x[4], uint64_t out[4]) {
  return guarded([&](Ctx& c) -> int {
    if ((n && !v) || !x || !out) return fail(GS_ERR_ARG, "null operand");
    const uint32_t* dv = upload_tmp(c, prove_state(c).up_a, v, n);
    prove_state(c).up_o.ensure(32);
    poly_eval_dev(c, dv, n, x, prove_state(c).up_o.as<uint32_t>());
    download(c, out, prove_state(c).up_o.p, 1);
    return GS_OK;
  });
}

// PolynomialField.LagrangeInterpolation (r1csqap.go:150-158): n values at the nodes 1..n -> n coefficients.
int gs_lagrange_interpolation(const uint64_t* values, size_t n, uint64_t* coeffs) {
  return guarded([&](Ctx& c) -> int {
    if (n == 0) return GS_OK;
    if (!values || !coeffs) return fail(GS_ERR_ARG, "gs_lagrange_interpolation: null argument");
    if (n >= (1ull << 26)) return fail(GS_ERR_ARG, "gs_lagrange_interpolation: too many nodes");
    const uint32_t* dv = upload_tmp(c, prove_state(c).up_a, values, n);
    prove_state(c).up_o.ensure(n * 32);
    interpolate_dev(c, dv, n, 1, prove_state(c).up_o.as<uint32_t>());
    poly_canon_dev(c, prove_state(c).up_o.as<uint32_t>(), n, 0);
    download(c, coeffs, prove_state(c).up_o.p, n);
    return GS_OK;
  });
}

int gs_zpoly(size_t deg, uint64_t* out) {
  return guarded([&](Ctx& c) -> int {
    if (!out) return fail(GS_ERR_ARG, "gs_zpoly: null output");
    if (deg >= (1ull << 26)) return fail(GS_ERR_ARG, "gs_zpoly: degree too large");
    prove_state(c).up_o.ensure((deg + 1) * 32);
    zpoly_dev(c, deg, prove_state(c).up_o.as<uint32_t>());
    download(c, out, prove_state(c).up_o.p, deg + 1);
    return GS_OK;
  });
}

}  // extern "C"
