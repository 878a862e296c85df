// GenericKernel::EvalJvp through the header-only host surface, for the stresslet (normals: all three tangents).  Writes the inputs, the tangents and
// the result, as raw doubles in the order xt xs xn f dxt dxs dxn du, to the file named on the command line: tests/test_gpu_jvp.py runs the Python
// entry on the same inputs and compares.  Also Eval's resizing rule: a wrongly sized result is resized and zeroed, a rightly sized one accumulated
// into, and a null tangent is a field of zeros.
//   jvp_driver out.bin       exit status 0 when the rules hold
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
  Vector<double> Xt(Nt * 3), Xs(Ns * 3), Xn(Ns * 3), f(Ns * 3), dXt(Nt * 3), dXs(Ns * 3), dXn(Ns * 3), du(5);
  for (auto& a : Xt) a = drand48();
  for (auto& a : Xs) a = drand48();
  for (auto& a : Xn) a = drand48() - 0.5;
  for (auto& a : f) a = drand48() - 0.5;
  for (auto& a : dXt) a = drand48() - 0.5;
  for (auto& a : dXs) a = drand48() - 0.5;
  for (auto& a : dXn) a = drand48() - 0.5;
  ker.template EvalJvp<double>(du, Xt, Xs, Xn, f, &dXt, &dXs, &dXn);       // wrong size: resized and zeroed
  if (du.Dim() != Nt * 3) return 1;
  // right size: accumulated into; the three tangents one at a time add up to the full call (the tangent is linear in them)
  Vector<double> parts(Nt * 3);
  parts.SetZero();
  ker.template EvalJvp<double>(parts, Xt, Xs, Xn, f, &dXt, nullptr, nullptr);
  ker.template EvalJvp<double>(parts, Xt, Xs, Xn, f, nullptr, &dXs, nullptr);
  ker.template EvalJvp<double>(parts, Xt, Xs, Xn, f, nullptr, nullptr, &dXn);
  Vector<double> same = du;
  ker.template EvalJvp<double>(same, Xt, Xs, Xn, f, nullptr, nullptr, nullptr);   // no tangent: nothing is added
  double err = 0, untouched = 0, umax = 0;
  for (Long i = 0; i < Nt * 3; i++) {
    err = std::fmax(err, std::fabs(parts[i] - du[i]));
    untouched = std::fmax(untouched, std::fabs(same[i] - du[i]));
    umax = std::fmax(umax, std::fabs(du[i]));
  }
  std::printf("Stokes3D-DxU %ld x %ld: max |du| %.3e, parts against the whole %.3e\n", (long)Nt, (long)Ns, umax, err);
  FILE* fh = std::fopen(argv[1], "wb");
  if (!fh) return 2;
  const Vector<double>* all[8] = {&Xt, &Xs, &Xn, &f, &dXt, &dXs, &dXn, &du};
  for (const Vector<double>* v : all)
    if (std::fwrite(v->begin(), sizeof(double), (size_t)v->Dim(), fh) != (size_t)v->Dim()) return 2;
  std::fclose(fh);
  return (umax > 0 && err <= 1e-12 * umax && untouched == 0) ? 0 : 1;
}
