// GenericKernel::EvalDensities through the header-only host surface: nd Stokeslet densities on one geometry, then each row through Eval.
//   densities_driver <N> <nd> <out.bin>      (inputs by drand48: targets, sources, the nd densities)
// Writes the nd x N*3 result of EvalDensities followed by the nd rows Eval gives (raw doubles) and prints the largest relative difference.
#include <sctl_amd.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace sctl_amd;

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: densities_driver <N> <nd> <out.bin>\n"); return 2; }
  const Long N = std::atol(argv[1]), nd = std::atol(argv[2]);
  srand48(0);
  Vector<double> Xt(N * 3), Xs(N * 3), Xn;
  for (auto& a : Xt) a = drand48() - 0.5;
  for (auto& a : Xs) a = drand48() - 0.5;
  Matrix<double> F(nd, N * 3), U;
  for (Long i = 0; i < nd * N * 3; i++) F.begin()[i] = drand48() - 0.5;
  const Stokes3D_FxU ker;
  ker.EvalDensities<double>(U, Xt, Xs, Xn, F);
  SCTL_AMD_ASSERT(U.Dim(0) == nd && U.Dim(1) == N * 3);
  Matrix<double> R(nd, N * 3);
  double err = 0;
  for (Long m = 0; m < nd; m++) {
    Vector<double> f(N * 3, (Iterator<double>)F[m], false), u;
    ker.Eval<double>(u, Xt, Xs, Xn, f);
    double d2 = 0, n2 = 0;
    for (Long i = 0; i < N * 3; i++) {
      R(m, i) = u[i];
      d2 += (U(m, i) - u[i]) * (U(m, i) - u[i]);
      n2 += u[i] * u[i];
    }
    if (n2 > 0 && std::sqrt(d2 / n2) > err) err = std::sqrt(d2 / n2);
  }
  std::FILE* fp = std::fopen(argv[3], "wb");
  if (!fp) return 1;
  std::fwrite(&U(0, 0), sizeof(double), (size_t)(nd * N * 3), fp);
  std::fwrite(&R(0, 0), sizeof(double), (size_t)(nd * N * 3), fp);
  std::fclose(fp);
  std::printf("EvalDensities vs Eval per row: largest relative difference %.3e\n", err);
  return 0;
}
