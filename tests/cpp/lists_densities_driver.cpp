// GenericKernel::EvalListsDensities through the header-only host surface: nd Stokeslet densities over the lists of a small tree-like layout (boxes
// of 1 .. 150 points, each against itself and its two neighbours), then each row through EvalLists.
//   lists_densities_driver <nboxes> <nd> <out.bin>      (inputs by drand48)
// Writes the nd x N*3 result of EvalListsDensities followed by the nd rows EvalLists gives (raw doubles); asserts the resize-or-accumulate rule.
#include <sctl_amd.hpp>

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sctl_amd;

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: lists_densities_driver <nboxes> <nd> <out.bin>\n"); return 2; }
  const Long nb = std::atol(argv[1]), nd = std::atol(argv[2]);
  srand48(0);
  std::vector<Long> cnt(nb), off(nb);
  Long N = 0;
  for (Long b = 0; b < nb; b++) { cnt[b] = 1 + (Long)(drand48() * (b % 4 == 0 ? 150 : 20)); off[b] = N; N += cnt[b]; }
  std::vector<Long> to, tc, so, sc;
  for (Long b = 0; b < nb; b++)
    for (Long d = -1; d <= 1; d++) {
      const Long s = b + d;
      if (s < 0 || s >= nb) continue;
      to.push_back(off[b]); tc.push_back(cnt[b]); so.push_back(off[s]); sc.push_back(cnt[s]);
    }
  const Long nl = (Long)to.size();
  Vector<Long> Lto(nl), Ltc(nl), Lso(nl), Lsc(nl);
  for (Long l = 0; l < nl; l++) { Lto[l] = to[l]; Ltc[l] = tc[l]; Lso[l] = so[l]; Lsc[l] = sc[l]; }
  Vector<double> X(N * 3), Xn;                 // the sources ARE the targets: every box meets its own points
  for (auto& a : X) a = drand48() - 0.5;
  Matrix<double> F(nd, N * 3), U;
  for (Long i = 0; i < nd * N * 3; i++) F.begin()[i] = drand48() - 0.5;
  const Stokes3D_FxU ker;
  ker.EvalListsDensities<double>(U, X, X, Xn, F, Lto, Ltc, Lso, Lsc);          // wrong size: resized and zeroed
  SCTL_AMD_ASSERT(U.Dim(0) == nd && U.Dim(1) == N * 3);
  Matrix<double> U2(nd, N * 3);
  for (Long i = 0; i < nd * N * 3; i++) U2.begin()[i] = 0.25;
  ker.EvalListsDensities<double>(U2, X, X, Xn, F, Lto, Ltc, Lso, Lsc);         // right size: accumulated into
  for (Long i = 0; i < nd * N * 3; i++) SCTL_AMD_ASSERT(U2.begin()[i] == 0.25 + U.begin()[i]);
  Matrix<double> R(nd, N * 3);
  for (Long m = 0; m < nd; m++) {
    Vector<double> f(N * 3, (Iterator<double>)F[m], false), u;
    ker.EvalLists<double>(u, X, X, Xn, f, Lto, Ltc, Lso, Lsc);
    for (Long i = 0; i < N * 3; i++) R(m, i) = u[i];
  }
  std::FILE* fp = std::fopen(argv[3], "wb");
  if (!fp) return 1;
  std::fwrite(&U(0, 0), sizeof(double), (size_t)(nd * N * 3), fp);
  std::fwrite(&R(0, 0), sizeof(double), (size_t)(nd * N * 3), fp);
  std::fclose(fp);
  std::printf("%ld points, %ld lists, %ld densities\n", (long)N, (long)nl, (long)nd);
  return 0;
}
