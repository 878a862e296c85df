// GenericKernel::EvalListsTranspose through the header-only host surface, checked against a loop of EvalTranspose over the lists: source boxes
// of 5 .. 130 points (packed, one and two owners per lane), each listed with three target ranges that overlap freely (the transposed direction
// asks disjoint-or-identical ranges of the sources only), for a kernel with normals and one with more outputs than inputs.  Also the resizing
// rule: a wrongly sized g_src is resized and zeroed, a rightly sized one accumulated into.
//   lists_transpose_driver          (inputs by drand48); exit status 0 when both kernels agree to rel-L2 1e-12
#include <sctl_amd.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace sctl_amd;

template <class Ker> static bool check(const char* name) {
  const Ker ker;
  const Long k0 = Ker::SrcDim(), k1 = Ker::TrgDim(), nd = Ker::NormalDim();
  const Long box[5] = {5, 40, 64, 130, 20};
  const Long Nt = 400;
  Long Ns = 0;
  Vector<Long> to, tc, so, sc;
  for (int b = 0; b < 5; b++) {
    for (int j = 0; j < 3; j++) {                 // target ranges [37 (b + j), + 70 + 30 j): they overlap
      to.PushBack(37 * (b + j)); tc.PushBack(70 + 30 * j); so.PushBack(Ns); sc.PushBack(box[b]);
    }
    Ns += box[b];
  }
  Vector<double> Xt(Nt * 3), Xs(Ns * 3), Xn(Ns * nd), w(Nt * k1), g(3), ref(Ns * k0);
  for (auto& a : Xt) a = drand48();
  for (auto& a : Xs) a = drand48();
  for (auto& a : Xn) a = drand48() - 0.5;
  for (auto& a : w) a = drand48() - 0.5;
  ker.template EvalListsTranspose<double>(g, Xt, Xs, Xn, w, to, tc, so, sc);      // wrong size: resized and zeroed
  if (g.Dim() != Ns * k0) return false;
  ref.SetZero();
  for (Long l = 0; l < to.Dim(); l++) {           // views into the arrays; a rightly sized result is accumulated into
    Vector<double> gl(sc[l] * k0, ref.begin() + so[l] * k0, false);
    const Vector<double> xt(tc[l] * 3, Xt.begin() + to[l] * 3, false), xs(sc[l] * 3, Xs.begin() + so[l] * 3, false);
    const Vector<double> xn(sc[l] * nd, Xn.begin() + so[l] * nd, false), wl(tc[l] * k1, w.begin() + to[l] * k1, false);
    ker.template EvalTranspose<double>(gl, xt, xs, xn, wl);
  }
  Vector<double> g2 = g;
  ker.template EvalListsTranspose<double>(g2, Xt, Xs, Xn, w, to, tc, so, sc);     // right size: accumulated into
  long double num = 0, den = 0;
  double acc_err = 0, gmax = 0;
  for (Long i = 0; i < Ns * k0; i++) {
    num += ((long double)g[i] - ref[i]) * ((long double)g[i] - ref[i]);
    den += (long double)ref[i] * ref[i];
    acc_err = std::fmax(acc_err, std::fabs(g2[i] - 2 * g[i]));
    gmax = std::fmax(gmax, std::fabs(g[i]));
  }
  const double rel = (double)std::sqrt(num / den);
  std::printf("%s %ld lists, %ld sources: rel-L2 against the loop of EvalTranspose %.3e, accumulate error %.3e\n", name, (long)to.Dim(), (long)Ns, rel, acc_err);
  return den > 0 && rel <= 1e-12 && acc_err <= 1e-14 * gmax;
}

int main() {
  srand48(0);
  const bool a = check<Stokes3D_DxU>("Stokes3D-DxU");
  const bool b = check<Stokes3D_FxUP>("Stokes3D-FxUP");
  return (a && b) ? 0 : 1;
}
