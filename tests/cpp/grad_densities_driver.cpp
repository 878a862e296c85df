// GenericKernel::EvalGradDensities through the header-only host surface, for the stresslet (normals: all three outputs), against the sum of EvalGrad
// calls per row.  Also EvalGrad's resizing rule: a wrongly sized output is resized and zeroed, a rightly sized one accumulated into.
//   grad_densities_driver       exit status 0 when every difference is <= 1e-12 of the largest gradient entry
#include <sctl_amd.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace sctl_amd;

static double max_diff(const Vector<double>& a, const Vector<double>& b, double fb, double& amax) {
  double e = 0;
  for (Long i = 0; i < a.Dim(); i++) {
    e = std::fmax(e, std::fabs(a[i] - fb * b[i]));
    amax = std::fmax(amax, std::fabs(b[i]));
  }
  return e;
}

int main() {
  srand48(0);
  const Long Nt = 700, Ns = 450, nd = 5;     // a pass of 4 rows and one row on the form of 2
  const Stokes3D_DxU ker;
  Vector<double> Xt(Nt * 3), Xs(Ns * 3), Xn(Ns * 3);
  Matrix<double> F(nd, Ns * 3), W(nd, Nt * 3);
  for (auto& a : Xt) a = drand48();
  for (auto& a : Xs) a = drand48();
  for (auto& a : Xn) a = drand48() - 0.5;
  for (Long i = 0; i < nd * Ns * 3; i++) F.begin()[i] = drand48() - 0.5;
  for (Long i = 0; i < nd * Nt * 3; i++) W.begin()[i] = drand48() - 0.5;
  Vector<double> gt(5), gs, gn;
  ker.template EvalGradDensities<double>(&gt, &gs, &gn, Xt, Xs, Xn, F, W);       // wrong sizes: resized and zeroed
  if (gt.Dim() != Nt * 3 || gs.Dim() != Ns * 3 || gn.Dim() != Ns * 3) return 1;
  Vector<double> rt, rs, rn;                                                      // the rows one at a time, accumulated
  for (Long m = 0; m < nd; m++) {
    const Vector<double> f(Ns * 3, F[m], false), w(Nt * 3, W[m], false);
    ker.template EvalGrad<double>(&rt, &rs, &rn, Xt, Xs, Xn, f, w);
  }
  double gmax = 0;
  const double err = std::fmax(max_diff(gt, rt, 1, gmax), std::fmax(max_diff(gs, rs, 1, gmax), max_diff(gn, rn, 1, gmax)));
  ker.template EvalGradDensities<double>(&gt, &gs, &gn, Xt, Xs, Xn, F, W);       // right sizes: accumulated into
  double dummy = 0;
  const double acc = std::fmax(max_diff(gt, rt, 2, dummy), std::fmax(max_diff(gs, rs, 2, dummy), max_diff(gn, rn, 2, dummy)));
  std::printf("Stokes3D-DxU %ld x %ld, %ld rows: max |g| %.3e, against the rows one at a time %.3e, after a second call %.3e\n", (long)Nt, (long)Ns, (long)nd,
              gmax, err, acc);
  return (gmax > 0 && err <= 1e-12 * gmax && acc <= 2e-12 * gmax) ? 0 : 1;
}
