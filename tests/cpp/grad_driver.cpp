// GenericKernel::EvalGrad through the header-only host surface, for the stresslet (normals: all three outputs).  Writes the inputs and the three
// gradients, as raw doubles in the order xt xs xn f w g_trg g_src g_nrm, to the file named on the command line: tests/test_gpu_grad.py runs the Python
// entry on the same inputs and compares.  Also Eval's resizing rule: a wrongly sized output is resized and zeroed, a rightly sized one accumulated
// into, and a null output is left out.
//   grad_driver out.bin       exit status 0 when the rules hold
#include <sctl_amd.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace sctl_amd;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  srand48(0);
  const Long Nt = 700, Ns = 450;
  const Stokes3D_DxU ker;
  Vector<double> Xt(Nt * 3), Xs(Ns * 3), Xn(Ns * 3), f(Ns * 3), w(Nt * 3), gt(5), gs, gn;
  for (auto& a : Xt) a = drand48();
  for (auto& a : Xs) a = drand48();
  for (auto& a : Xn) a = drand48() - 0.5;
  for (auto& a : f) a = drand48() - 0.5;
  for (auto& a : w) a = drand48() - 0.5;
  ker.template EvalGrad<double>(&gt, &gs, &gn, Xt, Xs, Xn, f, w);       // wrong sizes: resized and zeroed
  if (gt.Dim() != Nt * 3 || gs.Dim() != Ns * 3 || gn.Dim() != Ns * 3) return 1;
  Vector<double> gs2 = gs;
  ker.template EvalGrad<double>(nullptr, &gs2, nullptr, Xt, Xs, Xn, f, w);   // right size: accumulated into; the others left out
  double acc_err = 0, gmax = 0;
  for (Long i = 0; i < Ns * 3; i++) {
    acc_err = std::fmax(acc_err, std::fabs(gs2[i] - 2 * gs[i]));
    gmax = std::fmax(gmax, std::fabs(gs[i]));
  }
  std::printf("Stokes3D-DxU %ld x %ld: max |g_src| %.3e, accumulate error %.3e\n", (long)Nt, (long)Ns, gmax, acc_err);
  FILE* fh = std::fopen(argv[1], "wb");
  if (!fh) return 2;
  const Vector<double>* all[8] = {&Xt, &Xs, &Xn, &f, &w, &gt, &gs, &gn};
  for (const Vector<double>* v : all)
    if (std::fwrite(v->begin(), sizeof(double), (size_t)v->Dim(), fh) != (size_t)v->Dim()) return 2;
  std::fclose(fh);
  return (gmax > 0 && acc_err <= 1e-14 * gmax) ? 0 : 1;
}
