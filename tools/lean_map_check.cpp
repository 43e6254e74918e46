// lean_map_check -- host check of the lean patterns of the BDF2 cell map (cell.hpp: MAP_NOPSI_NEG,
// MAP_NOPSI_POS), which the level-split pipelined pass runs on a handle whose source has no
// psi term (Sl == 0).  For random line constants, probed in double and in long double:
//  (1) sizes: map_count 33 / 24 / 16, FMAs 28 / 20 / 13, MAP_FULL's slots the dense walk's;
//  (2) with Sl = +0 or -0 (Sc = 0 lines among them) map_admits accepts both halves' maps and
//      the reflective head map, and every coefficient outside the lean pattern is exactly zero;
//      with Sl != 0 it refuses;
//  (3) one cell: the lean map_apply on the packed lean map is bitwise MAP_FULL's on the live
//      outputs, for finite inputs with zeros and 1e+-300 magnitudes among them;
//  (4) a 64-cell x 8-level strip run the way split_chunk runs it (each cell through the levels
//      in turn, the carried states kept per level, the reflective head cell on the full head
//      map): node outputs and live carried states bitwise equal.
// Host code only; tests/test_lean_map.py builds it under ASan + UBSan.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I radiative-transfer_amd/csrc \
//       tools/lean_map_check.cpp -o /tmp/lean_map_check && /tmp/lean_map_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "cell.hpp"

using namespace rtamd;

namespace {

constexpr int S = SCHEME_BDF2, K = SchemeDim<S>::K, WN = map_count<S>();

std::mt19937_64 rng(20261019);
double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
double mag(double lo, double hi) { return (rng() & 1 ? 1.0 : -1.0) * std::pow(10.0, uni(lo, hi)); }

int fails = 0;
void fail(const char *what) {
  if (fails++ < 10) std::printf("FAIL: %s\n", what);
}

bool same_bits(double a, double b) {
  std::uint64_t x, y;
  std::memcpy(&x, &a, 8);
  std::memcpy(&y, &b, 8);
  return x == y;
}

// a finite input: zeros, huge and tiny magnitudes among ordinary ones
double state_value() {
  switch (rng() % 8) {
    case 0: return 0.0;
    case 1: return -0.0;
    case 2: return mag(290.0, 300.0);
    case 3: return mag(-300.0, -290.0);
    default: return mag(-3.0, 3.0);
  }
}

template <class R>
LineConstT<R> random_line(int kind) {
  LineConstT<R> L;
  for (R &c : L.c) c = R(std::fabs(mag(-6.0, 6.0)));
  L.c[LC_SL] = kind == 0 ? R(0.0) : kind == 1 ? R(-0.0) : R(mag(-6.0, 6.0));
  if (rng() % 4 == 0) L.c[LC_SC] = R(0.0);
  return L;
}

// A line of a real medium (rtsn_lines.hip line_constants: BDF2, tau = dt / 2), whose step is
// stable, for the strips: ct = c tau, sigma = rho kappa, m = |mu|.
template <class R>
LineConstT<R> medium_line(int kind, R &dx) {
  dx = R(std::fabs(mag(-4.0, 0.0)));
  const R ct = dx * R(std::fabs(mag(-2.0, 3.0))), sigma = R(std::fabs(mag(-3.0, 3.0))) / dx;
  const R m = R(uni(0.02, 1.0)), half = R(0.5) * ct * dx;
  LineConstT<R> L{};
  L.c[LC_SC] = rng() % 4 == 0 ? R(0.0) : half * sigma * R(uni(0.1, 10.0));
  L.c[LC_SL] = kind == 0 ? R(0.0) : R(-0.0);
  auto inverse = [](R d, R o, R &i0, R &i1) {
    const R det = d * d + o * o;
    i0 = d / det;
    i1 = o / det;
  };
  {
    const R a = R(1.0) + ct * sigma, b = ct * m;
    L.c[LC_BE_B] = b;
    inverse((a * dx + b) / R(2.0), b / R(2.0), L.c[LC_BE_I0], L.c[LC_BE_I1]);
  }
  {
    const R t = R(0.5) * ct * sigma, A = R(0.5) * m * ct;
    L.c[LC_CN_A] = A;
    L.c[LC_CN_K1] = R(0.5) * ((R(1.0) - t) * dx - A);
    L.c[LC_CN_K2] = R(0.5) * A;
    inverse(R(0.5) * (A + (R(1.0) + t) * dx), A / R(2.0), L.c[LC_CN_I0], L.c[LC_CN_I1]);
  }
  {
    const R t = sigma * ct / R(6.0), Bc = m * (R(2.0) * ct) / R(6.0);
    L.c[LC_BD_BC] = Bc;
    L.c[LC_BD_Q1] = R(0.5) * ((R(1.0) - R(4.0) * t) * dx - R(4.0) * Bc);
    L.c[LC_BD_Q2] = R(2.0) * Bc;
    L.c[LC_BD_Q3] = R(0.5) * (Bc + t * dx);
    L.c[LC_BD_Q4] = R(0.5) * Bc;
    inverse(R(0.5) * ((R(1.0) + t) * dx + Bc), R(0.5) * Bc, L.c[LC_BD_I0], L.c[LC_BD_I1]);
  }
  return L;
}

void check_sizes() {
  static_assert(map_count<S, MAP_FULL>() == 33 && map_count<S, MAP_NOPSI_NEG>() == 24 &&
                    map_count<S, MAP_NOPSI_POS>() == 16,
                "map_count per pattern");
  static_assert(map_fmas<S, MAP_FULL>() == 28 && map_fmas<S, MAP_NOPSI_NEG>() == 20 &&
                    map_fmas<S, MAP_NOPSI_POS>() == 13,
                "FMAs per pattern");
  static_assert(lean_map_rows() == 40, "the two lean maps back to back");
  // MAP_FULL's slots: rows 1 .. K in order, each its structural columns then its constant
  const int deps[K + 1] = {0, 3, 5, 6, 7, 7};
  int n = 0;
  for (int r = 1; r <= K; ++r) {
    int cols = 0;
    for (int c = 0; c < K + 2; ++c) {
      const bool dep = c >= K || (r == 1 ? c == 1 : r == 2 ? c <= 2 : r == 3 ? c <= 3 : true);
      if (dep != map_dep<S>(r, c)) fail("MAP_FULL dependency pattern changed");
      if (!dep) continue;
      if (map_slot<S>(r, c) != n++) fail("MAP_FULL slot changed");
      ++cols;
    }
    if (cols != deps[r]) fail("MAP_FULL row size changed");
    if (map_slot<S>(r, K + 2) != n++) fail("MAP_FULL constant slot changed");
  }
  if (n != 33) fail("MAP_FULL count");
  // BE and CN have one pattern
  if (map_count<SCHEME_BE, MAP_NOPSI_POS>() != map_count<SCHEME_BE>() ||
      map_count<SCHEME_CN, MAP_NOPSI_NEG>() != map_count<SCHEME_CN>())
    fail("BE / CN maps have no lean pattern");
}

// every MAP_FULL coefficient the pattern P drops (its rows' own coefficients aside) is zero
template <int P>
bool dropped_zero(const double *W) {
  for (int r = 1; r <= K; ++r) {
    if (!map_row<S, P>(r)) continue;
    for (int c = 0; c < K + 2; ++c)
      if (map_dep<S>(r, c) && !map_dep<S, P>(r, c) && W[map_slot<S>(r, c)] != 0.0) return false;
  }
  return true;
}

// one cell, full against lean, on the live outputs
template <int P>
void one_cell(const double *W) {
  double Wp[WN];
  map_pack<S, P>(W, Wp);
  double X[K], Xl[K], Xn[K], Xln[K], oi, oo, li, lo;
  const bool zeros = rng() % 16 == 0;
  for (int r = 0; r < K; ++r) {
    X[r] = zeros ? 0.0 : state_value();
    Xl[r] = map_live<S, P>(r) ? X[r] : 0.0;
    Xln[r] = -1.0;
  }
  const double pin = zeros ? 0.0 : state_value(), pout = zeros ? 0.0 : state_value();
  map_apply<S, true>(W, X, pin, pout, Xn, oi, oo);
  map_apply<S, true, false, false, 0, P>(Wp, Xl, pin, pout, Xln, li, lo);
  for (int r = 0; r < K; ++r) {
    if (map_live<S, P>(r) && !same_bits(Xn[r], Xln[r])) fail("one cell: a live row differs");
    if (!map_live<S, P>(r) && Xln[r] != -1.0) fail("one cell: a dropped row was written");
  }
  if (!same_bits(oi, li) || !same_bits(oo, lo)) fail("one cell: node outputs differ");
}

// a strip of cells through T levels, the way split_chunk runs a chunk; Wh: the reflective head
// cell's full map for cell 0 (head_cell), or nullptr
template <int P>
void strip(const double *W, const double *Wh) {
  constexpr int NC = 64, T = 8;
  double Wp[WN];
  map_pack<S, P>(W, Wp);
  double X[T][K], Xl[T][K];
  for (int t = 0; t < T; ++t)
    for (int r = 0; r < K; ++r) {
      X[t][r] = uni(-1.0, 1.0);
      Xl[t][r] = map_live<S, P>(r) ? X[t][r] : 0.0;
    }
  for (int c = 0; c < NC; ++c) {
    const double ein = uni(-1.0, 1.0), eout = uni(-1.0, 1.0);
    double oi = ein, oo = eout, li = ein, lo = eout;
    for (int t = 0; t < T; ++t) {
      double Xn[K], a, e;
      map_apply<S, true>(c == 0 && Wh ? Wh : W, X[t], oi, oo, Xn, a, e);
      for (int r = 0; r < K; ++r) X[t][r] = Xn[r];
      oi = a;
      oo = e;
      if (c == 0 && Wh) {  // the lean roles keep the head cell on the full head map
        map_apply<S, true>(Wh, Xl[t], li, lo, Xn, a, e);
        for (int r = 0; r < K; ++r) Xl[t][r] = Xn[r];
      } else {
        map_apply<S, true, false, false, 0, P>(Wp, Xl[t], li, lo, Xn, a, e);
        for (int r = 0; r < K; ++r)
          if (map_live<S, P>(r)) Xl[t][r] = Xn[r];
      }
      li = a;
      lo = e;
    }
    if (!same_bits(oi, li) || !same_bits(oo, lo)) fail("strip: node outputs differ");
    if (!std::isfinite(oi) || !std::isfinite(oo)) fail("strip: not finite (the comparison needs finite states)");
  }
  for (int t = 0; t < T; ++t)
    for (int r = 0; r < K; ++r)
      if (map_live<S, P>(r) && !same_bits(X[t][r], Xl[t][r])) fail("strip: a live carried state differs");
}

template <class R>
void check(int lines) {
  for (int n = 0; n < lines; ++n) {
    const int kind = n % 3;  // Sl = +0, -0, non-zero
    const LineConstT<R> L = random_line<R>(kind);
    const R hd = R(std::fabs(mag(-6.0, 0.0)));
    double Wneg[WN], Wpos[WN], Wh[WN];
    if (!cell_map<S>(L, hd, true, Wneg) || !cell_map<S>(L, hd, false, Wpos) || !cell_map<S, true>(L, hd, false, Wh)) {
      fail("a map is not of the structural pattern");
      continue;
    }
    if (kind == 2) {
      if (map_admits<S>(Wneg, true) || map_admits<S>(Wpos, false) || map_admits<S>(Wh, false))
        fail("a map with a psi source term was admitted");
      continue;
    }
    if (!map_admits<S>(Wneg, true) || !map_admits<S>(Wpos, false) || !map_admits<S>(Wh, false)) {
      fail("a map without a psi source term was refused");
      continue;
    }
    if (!dropped_zero<MAP_NOPSI_NEG>(Wneg) || !dropped_zero<MAP_NOPSI_POS>(Wpos) || !dropped_zero<MAP_NOPSI_POS>(Wh) ||
        !dropped_zero<MAP_NOPSI_NEG>(Wpos))
      fail("a dropped coefficient is not zero");
    // the mu < 0 lines keep the CN row: H = e2 there
    if (Wneg[map_slot<S>(K - 1, 2)] == 0.0 && Wneg[map_slot<S>(K, 2)] == 0.0) fail("mu < 0: the xh column vanished");
    for (int k = 0; k < 8; ++k) {
      one_cell<MAP_NOPSI_NEG>(Wneg);
      one_cell<MAP_NOPSI_POS>(Wpos);
      one_cell<MAP_NOPSI_NEG>(Wpos);  // (both halves on the 20-FMA pattern)
      one_cell<MAP_NOPSI_POS>(Wh);
    }
  }
  for (int n = 0; n < lines / 10; ++n) {  // strips, on the lines of real media
    R dx;
    const LineConstT<R> L = medium_line<R>(n % 2, dx);
    double Wneg[WN], Wpos[WN], Wh[WN];
    if (!cell_map<S>(L, dx / R(2.0), true, Wneg) || !cell_map<S>(L, dx / R(2.0), false, Wpos) ||
        !cell_map<S, true>(L, dx / R(2.0), false, Wh)) {
      fail("a medium's map is not of the structural pattern");
      continue;
    }
    if (!map_admits<S>(Wneg, true) || !map_admits<S>(Wpos, false) || !map_admits<S>(Wh, false)) {
      fail("a medium's map without a psi source term was refused");
      continue;
    }
    strip<MAP_NOPSI_NEG>(Wneg, nullptr);
    strip<MAP_NOPSI_POS>(Wpos, nullptr);
    strip<MAP_NOPSI_NEG>(Wpos, nullptr);
    strip<MAP_NOPSI_POS>(Wpos, Wh);
  }
}

}  // namespace

int main() {
  const int lines = 3000;
  check_sizes();
  check<double>(lines);
  check<long double>(lines);
  std::printf("%d random lines per format, %d failures\n", lines, fails);
  return fails ? 1 : 0;
}
