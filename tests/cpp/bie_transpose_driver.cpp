// BoundaryIntegralOp::ComputePotentialTranspose / ComputeFarFieldTranspose / ComputeNearInteracTranspose of
// include/sctl_amd/boundary_integral.hpp on the operator bie_driver builds (same arguments, same drand48 inputs, same element lists: that
// driver's source is included below with its entry points renamed).  W: drand48() - 0.5 drawn after the density.
//
//   bie_transpose_driver <kernel> <seed> <Nt> <Ns> <nodes_per_elem> <upsample> <dot> <self_targets> <out.bin> [<rad> [<free_nodes>]]
// Writes G = ComputePotentialTranspose(W) to <out.bin> and { <W, ComputePotential(F)>, <G, F>, sum |W_i U_i|, sum |G_j F_j| } to <out.bin>.ip, and
// checks on the way that the two legs (far, then near accumulated) give the fused result to rounding.  The transposed call comes first: an
// operator with a matrix-free element list aborts there.
#define main bie_driver_main
#define run bie_driver_run
#include "bie_driver.cpp"
#undef main
#undef run

template <class Kernel> int run_transpose(long seed, Long Nt, Long Ns, Long npe, Long ups, bool dot, bool self_trg, const char* out, double rad, Long nfree) {
  typedef double Real;
  srand48(seed);
  Vector<Real> xt(Nt * 3), xnt(Nt * 3), xs(Ns * 3), xn(Ns * 3), w(Ns), f(Ns * Kernel::SrcDim());
  for (auto& a : xt) a = drand48() - 0.5;
  for (auto& a : xnt) a = drand48() - 0.5;
  for (auto& a : xs) a = drand48() - 0.5;
  for (auto& a : xn) a = drand48() - 0.5;
  for (auto& a : w) a = drand48() * 0.01;
  for (auto& a : f) a = drand48() - 0.5;

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
  SCTL_AMD_ASSERT(n0 == f.Dim());
  Vector<Real> W(n1);
  for (auto& a : W) a = drand48() - 0.5;

  Vector<Real> G;
  op.ComputePotentialTranspose(G, W);
  SCTL_AMD_ASSERT(G.Dim() == n0);
  Vector<Real> L;
  op.ComputeFarFieldTranspose(L, W);
  op.ComputeNearInteracTranspose(L, W);                   // a right-sized vector is accumulated into
  Real dmax = 0, gmax = 0;
  for (Long i = 0; i < n0; i++) { dmax = std::max(dmax, std::fabs(G[i] - L[i])); gmax = std::max(gmax, std::fabs(G[i])); }
  SCTL_AMD_ASSERT(dmax <= 1e-13 * gmax);

  Vector<Real> U;
  op.ComputePotential(U, f);
  SCTL_AMD_ASSERT(U.Dim() == n1);
  Vector<Real> ip(4);
  ip.SetZero();
  for (Long i = 0; i < n1; i++) { ip[0] += W[i] * U[i]; ip[2] += std::fabs(W[i] * U[i]); }
  for (Long i = 0; i < n0; i++) { ip[1] += G[i] * f[i]; ip[3] += std::fabs(G[i] * f[i]); }
  G.Write(out);
  ip.Write((std::string(out) + ".ip").c_str());
  std::cout << "dim0=" << n0 << " dim1=" << n1 << " <W,PF>=" << ip[0] << " <P^T W,F>=" << ip[1] << '\n';
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 10) {
    std::cerr << "usage: bie_transpose_driver <kernel> <seed> <Nt> <Ns> <nodes_per_elem> <upsample> <dot> <self_targets> <out.bin> [<rad> [<free_nodes>]]\n";
    return 2;
  }
  const std::string k = argv[1];
  const long seed = std::atol(argv[2]);
  const Long Nt = std::atol(argv[3]), Ns = std::atol(argv[4]), npe = std::atol(argv[5]), ups = std::atol(argv[6]);
  const bool dot = std::atoi(argv[7]) != 0, self_trg = std::atoi(argv[8]) != 0;
  const double rad = argc > 10 ? std::atof(argv[10]) : 0;
  const Long nfree = argc > 11 ? std::atol(argv[11]) : 0;
  if (k == "Laplace3D-FxU") return run_transpose<Laplace3D_FxU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], rad, nfree);
  if (k == "Laplace3D-DxU") return run_transpose<Laplace3D_DxU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], rad, nfree);
  if (k == "Laplace3D-FxdU") return run_transpose<Laplace3D_FxdU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], rad, nfree);
  if (k == "Stokes3D-FxU") return run_transpose<Stokes3D_FxU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], rad, nfree);
  if (k == "Stokes3D-DxU") return run_transpose<Stokes3D_DxU>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], rad, nfree);
  if (k == "Stokes3D-FxT") return run_transpose<Stokes3D_FxT>(seed, Nt, Ns, npe, ups, dot, self_trg, argv[9], rad, nfree);
  std::cerr << "unknown kernel " << k << '\n';
  return 2;
}
