// Host-only check of the hierarchical regression holiday's host arithmetic (boom_amd/csrc/ssg_regholiday.h):
// every refusal of rhh_add_refusal and rhh_set_refusal with its text, the Cholesky factor and the inverse
// the hyperparameters are formed with, and the model rhh_model builds.  The expectations are the documented
// rules (include/boom_amd.h at ba_ss_add_hierarchical_regression_holiday) written out as
// literals.  Built with -fsanitize=address,undefined and run by tests/test_ss_hier_regholiday_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../boom_amd/csrc/ssg_regholiday.h"

using namespace boom_amd;

static int failures = 0, checks = 0;
static void expect(bool ok, const char *what, int a = 0, int b = 0) {
  ++checks;
  if (ok) return;
  std::printf("FAIL %s (%d, %d)\n", what, a, b);
  ++failures;
}
static bool same(const char *a, const char *b) { return (!a && !b) || (a && b && std::strcmp(a, b) == 0); }

static std::vector<double> identity(int d, double v = 1.0) {
  std::vector<double> m((size_t)d * d, 0.0);
  for (int i = 0; i < d; ++i) m[(size_t)(i * d + i)] = v;
  return m;
}

int main() {
  const double inf = 1.0 / 0.0, nan = 0.0 / 0.0;
  // ---- the factor and the inverse
  {
    const double A[9] = {4, 2, -2, 2, 10, 2, -2, 2, 6}, want[9] = {2, 0, 0, 1, 3, 0, -1, 1, 2};
    double L[9], V[9];
    expect(rh_cholesky(A, 3, L), "a factor");
    for (int i = 0; i < 9; ++i) expect(L[i] == want[i], "the factor's entries", i);
    expect(rh_spd_inverse(A, 3, V), "an inverse");
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += A[r * 3 + k] * V[k * 3 + c];
        expect(std::fabs(s - (r == c ? 1.0 : 0.0)) < 1e-14, "A A^-1 = I", r, c);
        expect(V[r * 3 + c] == V[c * 3 + r], "the inverse is symmetric to the bit", r, c);
      }
    const double one[1] = {0.25};
    expect(rh_spd_inverse(one, 1, V) && V[0] == 4.0, "1 x 1");
    const double indef[4] = {1, 2, 2, 1}, zero[4] = {1, 1, 1, 1};
    expect(!rh_cholesky(indef, 2, L) && !rh_cholesky(zero, 2, L), "not positive definite");
    expect(!rh_is_spd(indef, 2) && !rh_is_spd(zero, 2), "rh_is_spd: not positive definite");
    const double skew[4] = {2, 0.5, 0.25, 2}, hasnan[4] = {2, nan, nan, 2}, hasinf[4] = {inf, 0, 0, 1};
    expect(!rh_is_spd(skew, 2), "not symmetric");
    expect(!rh_is_spd(hasnan, 2) && !rh_is_spd(hasinf, 2), "not finite");
    const std::vector<double> big = identity(16, 3.0);
    expect(rh_is_spd(big.data(), 16), "16 x 16");
  }
  // ---- the arguments of an add
  {
    std::vector<RhModel> none;
    const int d = 3;
    const double mu0[3] = {0.5, -0.5, 0.25};
    const std::vector<double> S = identity(d, 2.0), G = identity(d, 0.5);
    auto refusal = [&](int H, int w, const double *m, const double *s, const double *g, double wt, const double *c = nullptr,
                       bool has = true, const std::vector<RhModel> *ms = nullptr) {
      return rhh_add_refusal(ms ? *ms : none, has, H, w, m, s, g, wt, c);
    };
    expect(refusal(4, d, mu0, S.data(), G.data(), 4.0) == nullptr, "a plain add");
    expect(same(refusal(4, d, nullptr, S.data(), G.data(), 4.0), "null argument"), "null mean");
    expect(same(refusal(4, d, mu0, nullptr, G.data(), 4.0), "null argument"), "null variance");
    expect(same(refusal(4, d, mu0, S.data(), nullptr, 4.0), "null argument"), "null guess");
    expect(same(refusal(0, d, mu0, S.data(), G.data(), 4.0), "a regression holiday model needs at least one holiday"), "no holiday");
    expect(same(refusal(4, d, mu0, S.data(), G.data(), 4.0, nullptr, false),
                "a regression holiday model goes on a list of state models: add a state model first"), "no state model");
    expect(same(refusal(4, 0, mu0, S.data(), G.data(), 4.0), "a holiday's width must be at least 1"), "width 0");
    const std::vector<double> S17 = identity(17), m17(17, 0.0);
    expect(same(refusal(1, 17, m17.data(), S17.data(), S17.data(), 20.0),
                "the holidays of a hierarchical regression holiday model are at most 16 days wide"), "width 17");
    const std::vector<double> S16 = identity(16), m16(16, 0.0);
    expect(refusal(16, 16, m16.data(), S16.data(), S16.data(), 16.0) == nullptr, "16 x 16: the 256 coefficients");
    expect(same(refusal(17, 16, m16.data(), S16.data(), S16.data(), 16.0), "more than 256 regression holiday coefficients"), "272 coefficients");
    RhModel plain;
    plain.widths = {250};
    const std::vector<RhModel> one(1, plain), four(4, RhModel{});
    expect(same(refusal(3, d, mu0, S.data(), G.data(), 4.0, nullptr, true, &one), "more than 256 regression holiday coefficients"), "250 + 9");
    expect(refusal(2, d, mu0, S.data(), G.data(), 4.0, nullptr, true, &one) == nullptr, "250 + 6");
    expect(same(refusal(3, d, mu0, S.data(), G.data(), 4.0, nullptr, true, &four), "more than 4 regression holiday models"), "a fifth model");
    // the weight: above d - 1
    for (double wt : {2.0, 1.0, 0.0, -1.0})
      expect(same(refusal(4, d, mu0, S.data(), G.data(), wt),
                  "the variance guess weight must exceed the holidays' width less 1 (the Wishart prior's degrees of freedom)"), "the weight");
    expect(refusal(4, d, mu0, S.data(), G.data(), 2.5) == nullptr, "a weight of 2.5 at width 3");
    for (double wt : {inf, nan}) expect(same(refusal(4, d, mu0, S.data(), G.data(), wt), "the variance guess weight must be finite"), "the weight, not finite");
    // not finite, not symmetric, not positive definite
    double mbad[3] = {0.5, nan, 0.25};
    expect(same(refusal(4, d, mbad, S.data(), G.data(), 4.0), "the prior mean of the holidays' mean must be finite"), "mean");
    std::vector<double> bad = S;
    bad[1] = bad[3] = inf;
    const char *const FINITE = "the prior variance of the holidays' mean and the variance guess must be finite";
    expect(same(refusal(4, d, mu0, bad.data(), G.data(), 4.0), FINITE), "variance, not finite");
    expect(same(refusal(4, d, mu0, S.data(), bad.data(), 4.0), FINITE), "guess, not finite");
    bad = S;
    bad[1] = 0.5;
    expect(same(refusal(4, d, mu0, bad.data(), G.data(), 4.0), "the prior variance of the holidays' mean must be symmetric and positive definite"), "variance, not symmetric");
    expect(same(refusal(4, d, mu0, S.data(), bad.data(), 4.0), "the variance guess must be symmetric and positive definite"), "guess, not symmetric");
    bad[0] = bad[1] = bad[3] = bad[4] = 1.0;   // [[1, 1], [1, 1]] in the corner: singular, the second pivot exactly 0
    expect(same(refusal(4, d, mu0, bad.data(), G.data(), 4.0), "the prior variance of the holidays' mean must be symmetric and positive definite"), "variance, singular");
    expect(same(refusal(4, d, mu0, S.data(), bad.data(), 4.0), "the variance guess must be symmetric and positive definite"), "guess, singular");
    std::vector<double> c(12, 0.5);
    expect(refusal(4, d, mu0, S.data(), G.data(), 4.0, c.data()) == nullptr, "coefficients");
    c[11] = nan;
    expect(same(refusal(4, d, mu0, S.data(), G.data(), 4.0, c.data()), "the initial coefficients must be finite"), "coefficients, not finite");
  }
  // ---- the model
  {
    const double mu0[2] = {1.0, -2.0}, S[4] = {4, 0, 0, 16}, G[4] = {1, 0.5, 0.5, 3};
    const double c[6] = {1, 2, 3, 4, 5, 6};
    const RhModel m = rhh_model(3, 2, mu0, S, G, 2.5, c);
    expect(m.hier && m.width == 2 && m.ncoef() == 6 && m.widths.size() == 3 && m.nu0 == 2.5, "the model's shape");
    expect(m.sinv0[0] == 0.25 && m.sinv0[1] == 0.0 && m.sinv0[2] == 0.0 && m.sinv0[3] == 0.0625, "Sigma0^-1");
    expect(m.sinv0mu0[0] == 0.25 && m.sinv0mu0[1] == -0.125, "Sigma0^-1 mu0");
    expect(m.s0[0] == 2.5 && m.s0[1] == 1.25 && m.s0[2] == 1.25 && m.s0[3] == 7.5, "S0 = nu0 x the guess");
    expect(m.initial_mu[0] == 0.0 && m.initial_mu[1] == 0.0, "mu starts at 0");
    expect(m.initial_omega[0] == 1.0 && m.initial_omega[1] == 0.0 && m.initial_omega[2] == 0.0 && m.initial_omega[3] == 1.0, "Omega starts at I");
    for (int i = 0; i < 6; ++i) expect(m.initial[(size_t)i] == c[i], "the initial coefficients", i);
    const RhModel z = rhh_model(3, 2, mu0, S, G, 2.5, nullptr);
    for (int i = 0; i < 6; ++i) expect(z.initial[(size_t)i] == 0.0, "no initial coefficients: 0", i);
    // a setter's arguments
    const double mean[2] = {0.5, 0.5}, prec[4] = {2, 1, 1, 2}, notpd[4] = {1, 2, 2, 1}, skew[4] = {2, 1, 0.5, 2};
    double nf[4] = {2, 1, 1, 1.0 / 0.0}, mnf[2] = {0.0 / 0.0, 0};
    expect(rhh_set_refusal(m, mean, prec) == nullptr, "a setter");
    expect(same(rhh_set_refusal(m, nullptr, prec), "null argument") && same(rhh_set_refusal(m, mean, nullptr), "null argument"), "a setter, null");
    expect(same(rhh_set_refusal(m, mnf, prec), "the mean must be finite"), "a setter, mean");
    expect(same(rhh_set_refusal(m, mean, nf), "the precision must be finite"), "a setter, precision not finite");
    expect(same(rhh_set_refusal(m, mean, notpd), "the precision must be symmetric and positive definite"), "a setter, not positive definite");
    expect(same(rhh_set_refusal(m, mean, skew), "the precision must be symmetric and positive definite"), "a setter, not symmetric");
    RhModel plain;
    plain.widths = {2};
    expect(same(rhh_set_refusal(plain, mean, prec), "not a hierarchical regression holiday model"), "a setter on a plain model");
    // the packing is the plain model's: flat index h d + day
    RhModel k = m;
    k.calendar = {0, 1, -1, 4, 5, 2};
    const uint8_t obs[6] = {1, 1, 1, 0, 1, 1};
    const RhPacked P = rh_pack(std::vector<RhModel>(1, k), 6, obs);
    const double counts[6] = {1, 1, 1, 0, 0, 1};
    for (int i = 0; i < 6; ++i) expect(P.counts[(size_t)i] == counts[i], "counts", i);
    expect(P.steps.size() == 5 && P.table[3 * RH_MAX_MODELS] == 4, "steps and table");
  }
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
