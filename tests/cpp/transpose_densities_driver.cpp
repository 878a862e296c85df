// GenericKernel::EvalTransposeDensities through the header-only host surface: nd weight vectors of the velocity + pressure kernel on one geometry.
//   transpose_densities_driver <Nt> <Ns> <nd> <out.bin>      (inputs by drand48 - 0.5 after srand48(0): targets, sources, the nd weight vectors)
// Writes the nd x Ns*3 result (raw doubles), then calls again into the result (the right size: accumulated into) and prints how far that is from twice
// the first, and the largest relative difference of a row from EvalTranspose of that row.
#include <sctl_amd.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace sctl_amd;

int main(int argc, char** argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: transpose_densities_driver <Nt> <Ns> <nd> <out.bin>\n"); return 2; }
  const Long Nt = std::atol(argv[1]), Ns = std::atol(argv[2]), nd = std::atol(argv[3]);
  srand48(0);
  Vector<double> Xt(Nt * 3), Xs(Ns * 3), Xn;
  for (auto& a : Xt) a = drand48() - 0.5;
  for (auto& a : Xs) a = drand48() - 0.5;
  Matrix<double> W(nd, Nt * 4), G(1, 1);                       // G of the wrong size: resized and zeroed
  for (Long i = 0; i < nd * Nt * 4; i++) W.begin()[i] = drand48() - 0.5;
  const Stokes3D_FxUP ker;
  ker.EvalTransposeDensities<double>(G, Xt, Xs, Xn, W);
  SCTL_AMD_ASSERT(G.Dim(0) == nd && G.Dim(1) == Ns * 3);
  std::FILE* fp = std::fopen(argv[4], "wb");
  if (!fp) return 1;
  std::fwrite(G.begin(), sizeof(double), (size_t)(nd * Ns * 3), fp);
  std::fclose(fp);
  double row_err = 0;
  for (Long m = 0; m < nd; m++) {
    Vector<double> w(Nt * 4, (Iterator<double>)W[m], false), g;
    ker.EvalTranspose<double>(g, Xt, Xs, Xn, w);
    double d2 = 0, n2 = 0;
    for (Long i = 0; i < Ns * 3; i++) {
      d2 += (G(m, i) - g[i]) * (G(m, i) - g[i]);
      n2 += g[i] * g[i];
    }
    if (n2 > 0 && std::sqrt(d2 / n2) > row_err) row_err = std::sqrt(d2 / n2);
  }
  Matrix<double> G2 = G;
  ker.EvalTransposeDensities<double>(G2, Xt, Xs, Xn, W);      // the right size: accumulated into
  double acc_err = 0, scale = 0;
  for (Long i = 0; i < nd * Ns * 3; i++) {
    acc_err = std::fmax(acc_err, std::fabs(G2.begin()[i] - 2 * G.begin()[i]));
    scale = std::fmax(scale, std::fabs(G.begin()[i]));
  }
  std::printf("EvalTransposeDensities vs EvalTranspose per row: largest relative difference %.3e; accumulate error %.3e of %.3e\n", row_err, acc_err, scale);
  return (row_err <= 1e-12 && acc_err <= 1e-12 * scale) ? 0 : 1;
}
