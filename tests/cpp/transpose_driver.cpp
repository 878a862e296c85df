// GenericKernel::EvalTranspose through the header-only host surface, checked against Eval by the adjoint identity
//     <w, Eval(f)> == <EvalTranspose(w), f>
// for a kernel with normals and an unsymmetric block (the stresslet) and one with more outputs than inputs (velocity + pressure).  Also Eval's
// resizing rule: a wrongly sized g_src is resized and zeroed, a rightly sized one accumulated into.
//   transpose_driver          (inputs by drand48); exit status 0 when both identities hold to 1e-12 of sum |w_i (A f)_i|
#include <sctl_amd.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace sctl_amd;

template <class Ker> static bool check(const char* name, Long Nt, Long Ns) {
  const Ker ker;
  const Long k0 = Ker::SrcDim(), k1 = Ker::TrgDim(), nd = Ker::NormalDim();
  Vector<double> Xt(Nt * 3), Xs(Ns * 3), Xn(Ns * nd), f(Ns * k0), w(Nt * k1), u, g(7);
  for (auto& a : Xt) a = drand48();
  for (auto& a : Xs) a = drand48();
  for (auto& a : Xn) a = drand48() - 0.5;
  for (auto& a : f) a = drand48() - 0.5;
  for (auto& a : w) a = drand48() - 0.5;
  ker.template Eval<double>(u, Xt, Xs, Xn, f);
  ker.template EvalTranspose<double>(g, Xt, Xs, Xn, w);      // wrong size: resized and zeroed
  if (g.Dim() != Ns * k0) return false;
  long double lhs = 0, rhs = 0, mag = 0;
  for (Long i = 0; i < Nt * k1; i++) { lhs += (long double)w[i] * u[i]; mag += std::fabs((long double)w[i] * u[i]); }
  for (Long i = 0; i < Ns * k0; i++) rhs += (long double)g[i] * f[i];
  Vector<double> g2 = g;
  ker.template EvalTranspose<double>(g2, Xt, Xs, Xn, w);     // right size: accumulated into
  double acc_err = 0, gmax = 0;
  for (Long i = 0; i < Ns * k0; i++) {
    acc_err = std::fmax(acc_err, std::fabs(g2[i] - 2 * g[i]));
    gmax = std::fmax(gmax, std::fabs(g[i]));
  }
  const double diff = (double)std::fabs(lhs - rhs), bound = (double)(1e-12L * mag);
  std::printf("%s %ld x %ld: <w, A f> = %.17g, <A^T w, f> = %.17g, |difference| %.3e (bound %.3e), accumulate error %.3e\n", name, (long)Nt, (long)Ns, (double)lhs,
              (double)rhs, diff, bound, acc_err);
  return diff <= bound && acc_err <= 1e-14 * gmax;
}

int main() {
  srand48(0);
  const bool a = check<Stokes3D_DxU>("Stokes3D-DxU", 3000, 2100);
  const bool b = check<Stokes3D_FxUP>("Stokes3D-FxUP", 700, 5000);
  return (a && b) ? 0 : 1;
}
