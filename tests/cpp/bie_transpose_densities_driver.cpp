// BoundaryIntegralOp::ComputePotentialTransposeDensities / ComputeFarFieldTransposeDensities / ComputeNearInteracTransposeDensities of
// include/sctl_amd/boundary_integral.hpp on the operator bie_driver builds (same arguments, same drand48 inputs, same element lists: that
// driver's source is included below with its entry points renamed).  F (nd x Dim(0)) and W (nd x Dim(1)): drand48() - 0.5, drawn after the inputs.
//
//   bie_transpose_densities_driver <kernel> <seed> <Nt> <Ns> <nodes_per_elem> <upsample> <dot> <self_targets> <out.bin> <nd> [<rad> [<free_nodes>]]
// Writes G = ComputePotentialTransposeDensities(W) (nd x Dim(0)) to <out.bin> and, per row m, { <W[m], ComputePotentialDensities(F)[m]>, <G[m], F[m]>,
// sum |W_i U_i|, sum |G_j F_j|, rel-L2 of G[m] against ComputePotentialTranspose(W[m]) } to <out.bin>.ip, and checks on the way that the two legs (far,
// then near accumulated) give the fused result to rounding.  The transposed call comes first: an operator with a matrix-free element list aborts there.
#define main bie_driver_main
#define run bie_driver_run
#include "bie_driver.cpp"
#undef main
#undef run

template <class Kernel> int run_transpose(long seed, Long Nt, Long Ns, Long npe, Long ups, bool dot, bool self_trg, const char* out, Long nd, double rad, Long nfree) {
  typedef double Real;
  srand48(seed);
  Vector<Real> xt(Nt * 3), xnt(Nt * 3), xs(Ns * 3), xn(Ns * 3), w(Ns);
  for (auto& a : xt) a = drand48() - 0.5;
  for (auto& a : xnt) a = drand48() - 0.5;
  for (auto& a : xs) a = drand48() - 0.5;
  for (auto& a : xn) a = drand48() - 0.5;
  for (auto& a : w) a = drand48() * 0.01;

  Kernel ker;
  BoundaryIntegralOp<Real, Kernel> op(ker, dot, Comm::Self());
  op.SetAccuracy(1e-10);
  if (rad > 0 && nfree > 0) {
    const Long na = Ns - nfree;
    auto part = [](const Vector<Real>& v, Long off, Long n) { return Vector<Real>(n, (Iterator<Real>)v.begin() + off, false); };
    PatchElemList<Real> A(part(xs, 0, na * 3), part(xn, 0, na * 3), part(w, 0, na), npe, ups, rad);
    op.AddElemList(A, "a_patches");
    op.AddElemList(FreePatchElemList<Real>(part(xs, na * 3, nfree * 3), part(xn, na * 3, nfree * 3), part(w, na, nfree), npe, ups, rad, A.Size()), "b_free");
  } else if (rad > 0) op.AddElemList(PatchElemList<Real>(xs, xn, w, npe, ups, rad), "patches");
  else op.AddElemList(PointElemList<Real>(xs, xn, w, npe, ups), "points");
  if (!self_trg) {
    op.SetTargetCoord(xt);
    if (dot) op.SetTargetNormal(xnt);
  }
  const Long n0 = op.Dim(0), n1 = op.Dim(1);
  Matrix<Real> F(nd, n0), W(nd, n1);
  for (Long m = 0; m < nd; m++)
    for (Long i = 0; i < n0; i++) F[m][i] = drand48() - 0.5;
  for (Long m = 0; m < nd; m++)
    for (Long i = 0; i < n1; i++) W[m][i] = drand48() - 0.5;

  Matrix<Real> G;
  op.ComputePotentialTransposeDensities(G, W);
  SCTL_AMD_ASSERT(G.Dim(0) == nd && G.Dim(1) == n0);
  Matrix<Real> L;
  op.ComputeFarFieldTransposeDensities(L, W);
  op.ComputeNearInteracTransposeDensities(L, W);          // a right-sized matrix is accumulated into
  Real dmax = 0, gmax = 0;
  for (Long m = 0; m < nd; m++)
    for (Long i = 0; i < n0; i++) { dmax = std::max(dmax, std::fabs(G[m][i] - L[m][i])); gmax = std::max(gmax, std::fabs(G[m][i])); }
  SCTL_AMD_ASSERT(dmax <= 1e-13 * gmax);

  Matrix<Real> U;
  op.ComputePotentialDensities(U, F);
  SCTL_AMD_ASSERT(U.Dim(0) == nd && U.Dim(1) == n1);
  Vector<Real> ip(5 * nd);
  ip.SetZero();
  for (Long m = 0; m < nd; m++) {
    Real* r = &ip[5 * m];
    for (Long i = 0; i < n1; i++) { r[0] += W[m][i] * U[m][i]; r[2] += std::fabs(W[m][i] * U[m][i]); }
    for (Long i = 0; i < n0; i++) { r[1] += G[m][i] * F[m][i]; r[3] += std::fabs(G[m][i] * F[m][i]); }
    const Vector<Real> wm(n1, (Iterator<Real>)W[m], false);
    Vector<Real> g1;
    op.ComputePotentialTranspose(g1, wm);
    Real num = 0, den = 0;
    for (Long i = 0; i < n0; i++) { num += (G[m][i] - g1[i]) * (G[m][i] - g1[i]); den += g1[i] * g1[i]; }
    r[4] = std::sqrt(num / den);
    std::cout << "row " << m << " <W,PF>=" << r[0] << " <P^T W,F>=" << r[1] << " vs single " << r[4] << '\n';
  }
  Vector<Real> Gflat(nd * n0, G.begin(), false);
  Gflat.Write(out);
  ip.Write((std::string(out) + ".ip").c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 11) {
    std::cerr << "usage: bie_transpose_densities_driver <kernel> <seed> <Nt> <Ns> <nodes_per_elem> <upsample> <dot> <self_targets> <out.bin> <nd> [<rad> "
                 "[<free_nodes>]]\n";
    return 2;
  }
  const std::string k = argv[1];
  const long seed = std::atol(argv[2]);
  const Long Nt = std::atol(argv[3]), Ns = std::atol(argv[4]), npe = std::atol(argv[5]), ups = std::atol(argv[6]);
  const bool dot = std::atoi(argv[7]) != 0, self_trg = std::atoi(argv[8]) != 0;
  const Long nd = std::atol(argv[10]);
  const double rad = argc > 11 ? std::atof(argv[11]) : 0;
  const Long nfree = argc > 12 ? std::atol(argv[12]) : 0;
  if (k == "Laplace3D-FxU") return run_transpose<Laplace3D_FxU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], nd, rad, nfree);
  if (k == "Laplace3D-DxU") return run_transpose<Laplace3D_DxU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], nd, rad, nfree);
  if (k == "Laplace3D-FxdU") return run_transpose<Laplace3D_FxdU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], nd, rad, nfree);
  if (k == "Stokes3D-FxU") return run_transpose<Stokes3D_FxU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], nd, rad, nfree);
  if (k == "Stokes3D-DxU") return run_transpose<Stokes3D_DxU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], nd, rad, nfree);
  if (k == "Stokes3D-FxT") return run_transpose<Stokes3D_FxT>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], nd, rad, nfree);
  std::cerr << "unknown kernel " << k << '\n';
  return 2;
}
