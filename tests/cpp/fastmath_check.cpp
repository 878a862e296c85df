// CPU check of sctl_amd/csrc/fastmath.hpp (the fp64 sincos / exp used by the Helmholtz device kernel) against libm in
// long double (__float128 where a product of two doubles must be exact).  Prints the maximum errors; tests/test_fastmath.py asserts the
// bounds.  Built with g++ -lquadmath (no HIP needed).
#include "../../include/sctl_amd/device/fastmath.hpp"

#include <cmath>
#include <quadmath.h>
#include <cstdio>
#include <cstdlib>

int main() {
  using namespace sctl_amd::fastmath;
  const Coeffs K;
  srand48(1);
  const TabCoeffs T;
  static double table[kTableDoubles];
  for (int t = 0; t < 7; t++) fill_tables(table, t, 7, K);      // any cooperative split fills every entry
  double es = 0, ec = 0, ee = 0, ts = 0, tc = 0, te = 0;
  for (int i = 0; i < 4000000; i++) {
    const double scale = (i % 5 == 0) ? 1.0 : (i % 5 == 1) ? 30.0 : (i % 5 == 2) ? 3000.0 : (i % 5 == 3) ? 1.2e4 : 1.5e6;
    const double x = (drand48() * 2 - 1) * scale;
    double s, c;
    sincos_reduced(x, s, c, K);
    const long double sl = sinl((long double)x), cl = cosl((long double)x);
    es = fmax(es, fabs((double)(s - sl)));
    ec = fmax(ec, fabs((double)(c - cl)));
    const double t = (drand48() * 2 - 1) * ((i % 2) ? 5.0 : 700.0);
    const long double el = expl((long double)t);
    ee = fmax(ee, fabs((double)((exp_fast(t, K) - el) / el)));
    te = fmax(te, fabs((double)((exp_tab(t, T, table) - el) / el)));
    if (fabs(x) <= kSincosTabMaxArg) {
      sincos_tab(x, s, c, T, table);
      ts = fmax(ts, fabs((double)(s - sl)));
      tc = fmax(tc, fabs((double)(c - cl)));
    }
  }
  // the forms with the wavenumber folded in: sincos(kr r), exp(kappa r) against long double of the EXACT product
  double ks = 0, kc = 0, ke = 0;
  bool k_specials = true;
  const double krs[6] = {7.5, 0.013, 250.0, -3.2, 1e-9, 0.0}, kappas[6] = {-0.3, 0.3, -25.0, 1e-3, 40.0, 0.0};
  for (int m = 0; m < 6; m++) {
    TabCoeffsK TK;
    TK.set(krs[m], kappas[m], T);
    const double rmax_s = (krs[m] != 0) ? fmin(kSincosTabMaxArg / fabs(krs[m]), 1e6) : 1e6;
    const double rmax_e = (kappas[m] != 0) ? fmin(700.0 / fabs(kappas[m]), 1e6) : 1e6;   // relative accuracy where the result is a normal number
    for (int i = 0; i < 400000; i++) {
      const double u = drand48(), r = ((i % 3 == 0) ? u * u * u : u) * rmax_s;
      double s, c;
      sincos_tab_k(r, s, c, TK, table);
      const __float128 x = (__float128)krs[m] * (__float128)r;      // the product of two doubles is exact in 113 bits (not in long double's 64)
      ks = fmax(ks, fabs((double)((__float128)s - sinq(x))));
      kc = fmax(kc, fabs((double)((__float128)c - cosq(x))));
      const double re = ((i % 3 == 0) ? u * u * u : u) * rmax_e;
      const __float128 el = expq((__float128)kappas[m] * (__float128)re);
      ke = fmax(ke, fabs((double)(((__float128)exp_tab_k(re, TK, table) - el) / el)));
    }
    double s, c;
    sincos_tab_k(0.0, s, c, TK, table);
    k_specials = k_specials && s == 0.0 && c == 1.0 && exp_tab_k(0.0, TK, table) == 1.0;
    if (krs[m] == 0) { sincos_tab_k(123.456, s, c, TK, table); k_specials = k_specials && s == 0.0 && c == 1.0; }
    if (kappas[m] == 0) k_specials = k_specials && exp_tab_k(123.456, TK, table) == 1.0;
    else {   // beyond the double range, up to the stated limit of the argument: 0 or inf; NaN in -> NaN out
      const double far = 0.9 * kExpTabMaxArg / fabs(kappas[m]), v = exp_tab_k(far, TK, table), w = exp_tab_k(NAN, TK, table);
      k_specials = k_specials && (kappas[m] < 0 ? v == 0.0 : std::isinf(v)) && w != w;
    }
  }
  printf("k_abs_err_sin %.3e\nk_abs_err_cos %.3e\nk_rel_err_exp %.3e\nk_specials %d\n", ks, kc, ke, (int)k_specials);
  // ONE reduction for the whole factor e^{(kappa + i kr) r} (cexp_tab_k): error of D_m (re + i im) relative to |e^{(kappa + i kr) r}|, against
  // 113-bit arithmetic of the exact products; wavenumbers at both ends of the allowed decay ratio, tiny and large kr, kappa of either sign
  {
    static double ctab[kCexpTableDoubles];
    const double ckr[7] = {7.5, 7.5, 0.013, 250.0, 3.2, 1e-9, 40.0}, ckap[7] = {-0.3, 0.0, 0.013 / 4, -62.5, 0.8, 0.0, -1e-3};
    double ce = 0, cre = 0, two = 0;
    bool c_specials = true;
    for (int m = 0; m < 7; m++) {
      c_specials = c_specials && CexpCoeffsK::usable(ckr[m], ckap[m]);
      CexpCoeffsK CK;
      CK.set(ckr[m], ckap[m], T);
      TabCoeffsK TK;                       // the two-reduction form on the same arguments, for comparison
      TK.set(ckr[m], ckap[m], T);
      for (int t = 0; t < 5; t++) fill_cexp_tables(ctab, t, 5, ckr[m], ckap[m], K, T);
      const double rmax = fmin(kCexpMaxPhase / ckr[m], 1e6);
      for (int i = 0; i < 400000; i++) {
        const double u = drand48(), r = ((i % 3 == 0) ? u * u * u : u) * rmax;
        double re, im, dm;
        cexp_tab_k(r, re, im, dm, CK, ctab);
        const __float128 ph = (__float128)ckr[m] * (__float128)r, mag = expq((__float128)ckap[m] * (__float128)r);
        const __float128 er = (__float128)dm * (__float128)re - mag * cosq(ph), ei = (__float128)dm * (__float128)im - mag * sinq(ph);
        ce = fmax(ce, (double)(sqrtq(er * er + ei * ei) / mag));
        {
          double s2, c2;
          sincos_tab_k(r, s2, c2, TK, table);
          const double a2 = exp_tab_k(r, TK, table);
          const __float128 fr = (__float128)(a2 * c2) - mag * cosq(ph), fi = (__float128)(a2 * s2) - mag * sinq(ph);
          two = fmax(two, (double)(sqrtq(fr * fr + fi * fi) / mag));
        }
        if (ckap[m] == 0) {
          cexp_tab_k_real(r, re, im, CK, ctab);
          const __float128 fr = (__float128)re - cosq(ph), fi = (__float128)im - sinq(ph);
          cre = fmax(cre, (double)sqrtq(fr * fr + fi * fi));
        }
      }
      double re, im, dm;
      cexp_tab_k(0.0, re, im, dm, CK, ctab);
      c_specials = c_specials && re == 1.0 && im == 0.0 && dm == 1.0;
    }
    c_specials = c_specials && !CexpCoeffsK::usable(0.0, 0.0) && !CexpCoeffsK::usable(-7.5, 0.1) && !CexpCoeffsK::usable(1.0, 0.26) && !CexpCoeffsK::usable(1.0, -0.26);
    printf("cexp_rel_err %.3e\ncexp_real_abs_err %.3e\ncexp_specials %d\ntwo_reductions_rel_err %.3e\n", ce, cre, (int)c_specials, two);
  }
  // The constants a launch really runs: the kernel hands the distance in as the double C r (C = helmholtz_dist_factor(mode): 2 for mode 1,
  // 0x1.555555p+1 for mode 2, the default) and set_scaled folds C into the reduction step and the polynomial.  Both forms, per C, over the
  // wavenumbers of tests/test_gpu_helmholtz_pairs.py: the argument is the double x = C r, the truth is taken at x / C in 113-bit arithmetic, the
  // measure is the modulus of the complex error relative to |e^{ikr}|, of the EXACT product of the factors a form returns (D_m times the node
  // value, the exponential times sine / cosine: the kernel multiplies them into the amplitude 1/r in its own order, and the roundings of that
  // belong to the per-pair probes on the device).  C = 1 runs through the same loop (the keys *_c1), so the three columns
  // are of one measurement.  The one-reduction form also gets distances within one step h of EVERY period boundary m 2 pi / kr, m = 1 .. 255
  // (m = 255 lies at a phase of 1602, past kCexpMaxPhase but inside the 256 periods the tables hold: the last period factor is read there).
  {
    static double ctab[kCexpTableDoubles];
    const double Cs[3] = {1.0, 2.0, 22369621.0 / 8388608.0};      // the last is 0x1.555555p+1 exactly (C++14 has no hexadecimal literals)
    const char* tag[3] = {"c1", "c2", "c83"};
    // (Re k, Im k); kappa = -Im k.  The first six are usable by the one-reduction form, the last five are its refusals
    const double wkr[11] = {7.5, 7.5, 40.0, 40.0, 900.0, 1e-3, 40.0, -3.0, 0.0, 3.0, 5.0};
    const double wki[11] = {0.3, 0.0, 10.0, -10.0, 5.0, 2e-4, nextafter(10.0, 11.0), 2.5, 0.7, 60.0, -2.0};
    bool edges = true;
    for (int m = 0; m < 11; m++) edges = edges && (CexpCoeffsK::usable(wkr[m], -wki[m]) == (m < 6));
    edges = edges && CexpCoeffsK::usable(40.0, 10.0) && CexpCoeffsK::usable(40.0, -10.0) && !CexpCoeffsK::usable(40.0, nextafter(10.0, 11.0)) &&
            !CexpCoeffsK::usable(40.0, -nextafter(10.0, 11.0)) && !CexpCoeffsK::usable(nextafter(40.0, 39.0), 10.0);
    for (int ic = 0; ic < 3; ic++) {
      const double Cd = Cs[ic];
      const __float128 Cq = (__float128)Cd;
      double one = 0, two = 0, bnd = 0;
      for (int m = 0; m < 11; m++) {
        const double kr = wkr[m], kappa = -wki[m];
        const __float128 krq = (__float128)kr, kapq = (__float128)kappa;
        TabCoeffsK TK;
        TK.set_scaled(kr, kappa, T, Cd);
        // |error| / |e^{ikr}| of the value amp (c + i s) for the argument x = C r
        auto err_of = [&](double x, __float128 re, __float128 im) {
          const __float128 r = (__float128)x / Cq, ph = krq * r, mag = expq(kapq * r);
          const __float128 er = re - mag * cosq(ph), ei = im - mag * sinq(ph);
          return (double)(sqrtq(er * er + ei * ei) / mag);
        };
        auto two_at = [&](double x) {
          double s2, c2;
          sincos_tab_k(x, s2, c2, TK, table);
          const double a2 = exp_tab_k(x, TK, table);
          return err_of(x, (__float128)a2 * (__float128)c2, (__float128)a2 * (__float128)s2);
        };
        double rmax2 = 1e6;
        if (kr != 0) rmax2 = fmin(rmax2, kSincosTabMaxArg / fabs(kr));
        if (kappa != 0) rmax2 = fmin(rmax2, 700.0 / fabs(kappa));        // relative accuracy where the result is a normal number
        for (int i = 0; i < 100000; i++) {
          const double u = drand48(), x = ((i % 3 == 0) ? u * u * u : u) * rmax2 * Cd;
          two = fmax(two, two_at(x));
        }
        if (m >= 6) continue;
        CexpCoeffsK CK;
        CK.set_scaled(kr, kappa, T, Cd);
        for (int t = 0; t < 5; t++) fill_cexp_tables(ctab, t, 5, kr, kappa, K, T);      // the tables do not depend on C
        auto one_at = [&](double x) {
          double re, im, dm;
          cexp_tab_k(x, re, im, dm, CK, ctab);
          double e = err_of(x, (__float128)dm * (__float128)re, (__float128)dm * (__float128)im);
          if (kappa == 0) {
            cexp_tab_k_real(x, re, im, CK, ctab);
            e = fmax(e, err_of(x, re, im));
          }
          return e;
        };
        const double rmax1 = kCexpMaxPhase / kr;
        for (int i = 0; i < 100000; i++) {
          const double u = drand48(), x = ((i % 3 == 0) ? u * u * u : u) * rmax1 * Cd;
          one = fmax(one, one_at(x));
        }
        const double period = 6.283185307179586476925 / kr, h = period / kCexpNodes;
        for (int p = 1; p < kCexpPeriods; p++)
          for (int i = 0; i < 40; i++) {
            const double d = (i == 0) ? 0.0 : (i == 1) ? h : (i == 2) ? -h : (drand48() * 2 - 1) * h;
            bnd = fmax(bnd, one_at((p * period + d) * Cd));
          }
        double re, im, dm, s2, c2;
        cexp_tab_k(0.0, re, im, dm, CK, ctab);
        sincos_tab_k(0.0, s2, c2, TK, table);
        edges = edges && re == 1.0 && im == 0.0 && dm == 1.0 && s2 == 0.0 && c2 == 1.0 && exp_tab_k(0.0, TK, table) == 1.0;
      }
      printf("cexp_rel_err_%s %.3e\ncexp_boundary_rel_err_%s %.3e\ntwo_reductions_rel_err_%s %.3e\n", tag[ic], one, tag[ic], bnd, tag[ic], two);
    }
    printf("scaled_edges %d\n", (int)edges);
  }
  double s1, c1;
  sincos_tab(0.0, s1, c1, T, table);
  const bool tab_specials = exp_tab(-1e9, T, table) == 0.0 && std::isinf(exp_tab(1e9, T, table)) && exp_tab(0.0, T, table) == 1.0 &&
                            exp_tab(NAN, T, table) != exp_tab(NAN, T, table) && s1 == 0.0 && c1 == 1.0;
  printf("tab_abs_err_sin %.3e\ntab_abs_err_cos %.3e\ntab_rel_err_exp %.3e\ntab_specials %d\n", ts, tc, te, (int)tab_specials);
  // specials
  const double z = exp_fast(-1e9, K), big = exp_fast(1e9, K), one = exp_fast(0.0, K), nn = exp_fast(NAN, K);
  double s0, c0;
  sincos_reduced(0.0, s0, c0, K);
  printf("max_abs_err_sin %.3e\nmax_abs_err_cos %.3e\nmax_rel_err_exp %.3e\n", es, ec, ee);
  printf("specials %d\n", (z == 0.0) && std::isinf(big) && (one == 1.0) && (nn != nn) && (s0 == 0.0) && (c0 == 1.0));
  return 0;
}
