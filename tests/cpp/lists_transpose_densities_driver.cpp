// GenericKernel::EvalListsTransposeDensities through the header-only host surface, checked against a loop of EvalListsTranspose over the rows:
// source boxes of 5 .. 130 points (packed, one and two owners per lane), each listed with three target ranges that overlap freely, nd = 1, 3, 5
// and 9 weight vectors (one row: EvalListsTranspose's own path, bit for bit; a partly filled form; a form and a row left over; two passes), for a
// kernel with normals and one with more outputs than inputs.  Also the resizing rule: a wrongly sized G is resized and zeroed, a rightly sized
// one accumulated into.
//   lists_transpose_densities_driver          (inputs by drand48); exit status 0 when every row agrees to rel-L2 1e-12 and nd == 1 bit for bit
#include <sctl_amd.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace sctl_amd;

template <class Ker> static bool check(const char* name) {
  const Ker ker;
  const Long k0 = Ker::SrcDim(), k1 = Ker::TrgDim(), nn = Ker::NormalDim();
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
  Vector<double> Xt(Nt * 3), Xs(Ns * 3), Xn(Ns * nn);
  for (auto& a : Xt) a = drand48();
  for (auto& a : Xs) a = drand48();
  for (auto& a : Xn) a = drand48() - 0.5;
  bool ok = true;
  const Long nds[4] = {1, 3, 5, 9};
  for (const Long nd : nds) {
    Matrix<double> W(nd, Nt * k1), G(2, 3);
    for (Long i = 0; i < nd * Nt * k1; i++) W.begin()[i] = drand48() - 0.5;
    ker.template EvalListsTransposeDensities<double>(G, Xt, Xs, Xn, W, to, tc, so, sc);      // wrong size: resized and zeroed
    if (G.Dim(0) != nd || G.Dim(1) != Ns * k0) return false;
    Matrix<double> G2 = G;
    ker.template EvalListsTransposeDensities<double>(G2, Xt, Xs, Xn, W, to, tc, so, sc);     // right size: accumulated into
    double worst = 0, acc_err = 0, gmax = 0;
    bool bits = true;
    for (Long m = 0; m < nd; m++) {
      const Vector<double> w(Nt * k1, (Iterator<double>)W[m], false);
      Vector<double> ref;
      ker.template EvalListsTranspose<double>(ref, Xt, Xs, Xn, w, to, tc, so, sc);
      long double num = 0, den = 0;
      for (Long i = 0; i < Ns * k0; i++) {
        num += ((long double)G(m, i) - ref[i]) * ((long double)G(m, i) - ref[i]);
        den += (long double)ref[i] * ref[i];
        bits = bits && G(m, i) == ref[i];
        acc_err = std::fmax(acc_err, std::fabs(G2(m, i) - 2 * G(m, i)));
        gmax = std::fmax(gmax, std::fabs(G(m, i)));
      }
      if (!(den > 0)) return false;
      worst = std::fmax(worst, (double)std::sqrt(num / den));
    }
    std::printf("%s %ld lists, %ld sources, nd %ld: worst row rel-L2 against EvalListsTranspose %.3e, accumulate error %.3e%s\n", name, (long)to.Dim(), (long)Ns,
                (long)nd, worst, acc_err, nd == 1 ? (bits ? ", bit-equal" : ", NOT bit-equal") : "");
    ok = ok && worst <= 1e-12 && acc_err <= 1e-14 * gmax && (nd != 1 || bits);
  }
  Matrix<double> W0(0, Nt * k1), G0(1, 1);        // no rows: a 0 x Ns*SrcDim result, no device work
  ker.template EvalListsTransposeDensities<double>(G0, Xt, Xs, Xn, W0, to, tc, so, sc);
  return ok && G0.Dim(0) == 0 && G0.Dim(1) == Ns * k0;
}

int main() {
  srand48(0);
  const bool a = check<Stokes3D_DxU>("Stokes3D-DxU");
  const bool b = check<Stokes3D_FxUP>("Stokes3D-FxUP");
  return (a && b) ? 0 : 1;
}
