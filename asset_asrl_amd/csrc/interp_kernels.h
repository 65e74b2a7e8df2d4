// Trajectory table on the device: the Hermite interpolant of a phase trajectory, evaluated at arbitrary times.
//
// Replaces LGLInterpTable for exact data (/root/reference/src/OptimalControl/LGLInterpTable.h:349-372 loadExactData,
// :480-619 FindBlock / InterpBlockGen, :621-669 InterpBlockDerivGen, :866-926; LGLInterpTable.cpp:4-84 setMethod), the table
// ODEPhaseBase::refineTrajManual / updateMesh / returnTrajRange / returnTrajTable go through (ODEPhaseBase.cpp:673-688).
//
// STAGE 1, once per table (interp_xdot_kernel): the ODE right-hand side at every node row -- each row with its own controls,
// as loadExactData computes it -- and the compact array tb[0..nb] of block start times (tb[nb] = the last node's time) that the
// search of stage 2 reads instead of striding through the trajectory.  Thread <-> node; a workgroup's 64 rows are contiguous in
// memory, so they are read into LDS as one flat, coalesced stream and the 64 result rows leave the same way: a thread reading
// its own row of N doubles from global memory (or writing its n results there) would be a stride-N (stride-n) access, 1/N-th
// of every cache line used per instruction.  LDS rows are padded to an odd number of doubles, so the 32 lanes of a lane group
// reading element i of 32 different rows hit 32 different (64-bit) banks.
//
// STAGE 2, per query time (interp_eval_kernel), a workgroup takes QG = 128 consecutive queries:
//   A  thread <-> query: binary search over tb, s = (tau - t_first) / h, and the 6 * CS basis values phi_i(s), h psi_i(s), ups_i(s)
//      and their tau-derivatives, Horner from constexpr tables, left in LDS (odd row length: conflict-free for the lanes of phase B
//      that read different queries, a broadcast for those that share one);
//   B  thread <-> OUTPUT ELEMENT: the QG output rows are one contiguous run of QG * N doubles, and thread k of the workgroup
//      produces elements k, k + 256, ... of it -- every store instruction of a wave writes 512 contiguous bytes, whatever N is.
//      (Thread <-> query in this phase would write a row of N doubles per lane: a stride-N store, 8 of every 8 N bytes of a line
//      per instruction.)  The loads follow the same pattern: the CS node rows of a block are contiguous, consecutive lanes read
//      consecutive columns of them, and neighbouring queries share or adjoin blocks -- the re-reads are L1 / L2 hits.
// Work per query in phase A is a few hundred flops against (1 + deriv) * N doubles written and ~CS (N + n) read, so the stage is
// bound by memory; the basis values are therefore evaluated in double-double (below), which costs nothing measurable.
//
// Accuracy of the basis: the LGL7 power weights reach 2e3 with alternating signs, the derivative's 1.4e4; plain Horner in
// double leaves ~1e-12 absolute in phi_i' and the tau-derivative is  sum_i X_i phi_i'(s) / h : on a fine mesh (h ~ 1e-2 .. 1e-5)
// that is 1e-10 .. 1e-7 relative to X.  The polynomials are therefore summed by Horner with a double-double accumulator (the
// derivative's coefficients k w_k as exact products) and rounded once; the sums over the nodes are plain fused multiply-adds in a
// fixed order, so results are bitwise repeatable.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_kernels.h"

namespace asset_hip {

// Cardinal_XPower_Weights[i], Cardinal_DXPower_Weights[i] (2 CS coefficients) and Cardinal_UPolyPower_Weights[i] (CS
// coefficients), highest power first (LGLCoeffs.h:44-55, 139-153, 293-392; literals digit for digit).  Trapezoidal uses the
// LGL3 (cubic) table, as the reference does (LGLInterpTable.cpp:8-10).
struct InterpBasis {
  int cs;
  double xw[4][8], dxw[4][8], uw[4][4];
};
// clang-format off
__host__ __device__ constexpr InterpBasis interp_basis(int sch) {
  switch (sch) {
    case 1:
    case 2:
      return {2,
              {{2.0, -3.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0},
               {-2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
               {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
               {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}},
              {{1.0, -2.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0},
               {1.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
               {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
               {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}},
              {{-1.0, 1.0, 0.0, 0.0},
               {1.0, 0.0, 0.0, 0.0},
               {0.0, 0.0, 0.0, 0.0},
               {0.0, 0.0, 0.0, 0.0}}};
    case 3:
      return {3,
              {{24.0, -68.0, 66.0, -23.0, 0.0, 1.0, 0.0, 0.0},
               {0.0, 16.0, -32.0, 16.0, 0.0, 0.0, 0.0, 0.0},
               {-24.0, 52.0, -34.0, 7.0, 0.0, 0.0, 0.0, 0.0},
               {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}},
              {{4.0, -12.0, 13.0, -6.0, 1.0, 0.0, 0.0, 0.0},
               {16.0, -40.0, 32.0, -8.0, 0.0, 0.0, 0.0, 0.0},
               {4.0, -8.0, 5.0, -1.0, 0.0, 0.0, 0.0, 0.0},
               {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}},
              {{2.0, -3.0, 1.0, 0.0},
               {-4.0, 4.0, 0.0, 0.0},
               {2.0, -1.0, 0.0, 0.0},
               {0.0, 0.0, 0.0, 0.0}}};
    default:
      return {4,
              {{322.113192893432, -1262.16647180554, 1953.18722397597, -1497.44073672143, 575.419724269949, -92.112932612382, 0.0, 1.0},
               {-64.79204848488, 361.542466375583, -764.578109564441, 777.477964267544, -383.431222919698, 73.7809503258911, 0.0, 0.0},
               {64.7920484849059, -92.0018730186832, -44.0436705064007, 110.002715108135, -43.8271690468644, 5.07794897890751, 0.0, 0.0},
               {-322.11319289346, 992.625878448649, -1144.56544390514, 609.960057345752, -148.161332303388, 13.2540333075835, 0.0, 0.0}},
              {{26.2862997682608, -105.145199073049, 167.971831917166, -135.907298995812, 58.0483996910198, -12.254033307585, 1.0, 0.0},
               {119.581459799146, -446.567920871157, 645.538793826344, -446.829224641783, 145.40645229346, -17.1295604060043, 0.0, 0.0},
               {119.581459799146, -390.502297722867, 477.341924381445, -267.69702439259, 67.4701675365851, -6.19422960171859, 0.0, 0.0},
               {26.2862997682629, -78.8588993047889, 89.1129326123729, -46.7943663834307, 11.2540333075837, -0.999999999999869, 0.0, 0.0}},
              {{-5.12701665379258, 10.2540333075852, -6.12701665379258, 1.0},
               {10.9353308042859, -18.9665045333251, 8.03117372903925, 0.0},
               {-10.9353308042859, 13.8394878795326, -2.90415707524666, 0.0},
               {5.12701665379258, -5.12701665379258, 1.0, 0.0}}};
  }
}
// clang-format on

struct InterpArgs {
  int nb;                          // blocks; nodes = nb * (cs - 1) + 1
  long long nq;                    // query times
  const double* traj;              // [nodes][N] node rows [x, t, u, p]
  double* xdot;                    // [nodes][n]  ODE right-hand side at every node (written by stage 1, read by stage 2)
  double* tb;                      // [nb + 1]    block start times and the last node's time
  const double* times;             // [nq]
  double* out;                     // [nq][N]
  double* dout;                    // [nq][N] d/dtau of out, or null
  unsigned long long* n_outside;   // += queries outside [tb[0], tb[nb]] (extrapolated from the end blocks), or null
};

// ---- double-double Horner -------------------------------------------------------------------------------------------
// The error-free transformations below need every product and sum rounded as written: device code is compiled with
// -ffp-contract=fast, which turned  r = p + e  into fma(a.h, s, e) and  r - p  into fma(-a.h, s, r)  -- the low part then
// misses the rounding error of p and the result is no better than plain Horner (tests/test_gpu_traj_table_entries.py saw
// exactly plain Horner's error).  Contraction is therefore off inside the three functions; the fused multiply-adds that
// are meant are written as fma().
struct InterpDD {
  double h, l;
};
__device__ inline InterpDD interp_dd_mul(InterpDD a, double s) {   // a * s
#pragma clang fp contract(off)
  const double p = a.h * s;
  const double e = fma(a.l, s, fma(a.h, s, -p));
  const double r = p + e;
  return {r, e - (r - p)};
}
__device__ inline InterpDD interp_dd_add(InterpDD a, double wh, double wl) {   // a + (wh + wl)
#pragma clang fp contract(off)
  const double s = a.h + wh, bb = s - a.h;
  const double e = ((a.h - (s - bb)) + (wh - bb)) + (a.l + wl);
  const double r = s + e;
  return {r, e - (r - s)};
}
// p(s) and dp/ds of the polynomial with coefficients w[0..NC) (highest power first), each rounded once
template <int NC>
__device__ inline void interp_poly(const double* w, double s, double& p, double& dp) {
#pragma clang fp contract(off)
  InterpDD a{w[0], 0.0}, d{0.0, 0.0};
#pragma unroll
  for (int k = 1; k < NC; k++) {
    // derivative: coefficient (NC - k) w[k - 1] of s^(NC - 1 - k), as an exact product
    const double m = double(NC - k), ch = m * w[k - 1], cl = fma(m, w[k - 1], -ch);
    d = interp_dd_add(interp_dd_mul(d, s), ch, cl);
    a = interp_dd_add(interp_dd_mul(a, s), w[k], 0.0);
  }
  p = a.h + a.l;
  dp = d.h + d.l;
}

template <class Ode>
struct InterpRowIn {   // ODE input = one trajectory row, its own controls (loadExactData does not relabel controls)
  const double* row;
  __device__ double y(int i) const { return row[i]; }
  __device__ double lam(int) const { return 0.0; }
};

// ---- stage 1 --------------------------------------------------------------------------------------------------------
template <class Ode, int SCH, bool BLOCKED>
__global__ __launch_bounds__(64) void interp_xdot_kernel(InterpArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, K = interp_basis(SCH).cs - 1;
  constexpr int LDN = N | 1, LDX = n | 1;                                  // odd row lengths (see the head of the file)
  constexpr bool STAGED = size_t(64) * (LDN + LDX) * sizeof(double) <= 48 * 1024;
  __shared__ double srow[STAGED ? 64 * LDN : 1];
  __shared__ double sout[STAGED ? 64 * LDX : 1];
  const long long nodes = (long long)a.nb * K + 1;
  const long long first = (long long)blockIdx.x * 64;
  const int cnt = int(nodes - first < 64 ? nodes - first : 64), t = threadIdx.x;
  if (cnt <= 0) return;
  if constexpr (STAGED) {
    for (int k = t; k < cnt * N; k += 64) srow[(k / N) * LDN + (k % N)] = a.traj[first * N + k];
    __syncthreads();
  }
  if (t < cnt) {
    const double* row = STAGED ? srow + t * LDN : a.traj + (first + t) * N;
    InterpRowIn<Ode> in{row};
    ValueOut<n> out;
    Ode::f(in, out);
    if constexpr (STAGED) {
#pragma unroll
      for (int k = 0; k < n; k++) sout[t * LDX + k] = out.v[k];
    } else {
#pragma unroll
      for (int k = 0; k < n; k++) a.xdot[(first + t) * n + k] = out.v[k];
    }
    const long long j = first + t;
    if (j % K == 0) a.tb[j / K] = row[n];
  }
  if constexpr (STAGED) {
    __syncthreads();
    for (int k = t; k < cnt * n; k += 64) a.xdot[first * n + k] = sout[(k / n) * LDX + (k % n)];
  }
}

// ---- stage 2 --------------------------------------------------------------------------------------------------------
constexpr int INTERP_QG = 128;   // queries per workgroup pass

template <class Ode, int SCH, bool BLOCKED>
__global__ __launch_bounds__(256) void interp_eval_kernel(InterpArgs a) {
  constexpr InterpBasis bs = interp_basis(SCH);                        // compile-time indices: constants in the code
  constexpr int n = Ode::XV, N = Ode::NIN, CS = interp_basis(SCH).cs, K = CS - 1, QG = INTERP_QG;
  constexpr int LD = 1 + 6 * CS;   // [0] time, phi[CS], h psi[CS], ups[CS], phi'/h [CS], psi' [CS], ups'/h [CS]: 13 / 19 / 25 doubles, odd
  __shared__ double sb[QG * LD];
  __shared__ int se[QG];
  const int t = threadIdx.x;
  const long long ngroups = (a.nq + QG - 1) / QG;
  const double t0 = a.tb[0], tf = a.tb[a.nb];
  const double dir = tf > t0 ? 1.0 : -1.0;
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long long q0 = g * QG;
    const int cnt = int(a.nq - q0 < QG ? a.nq - q0 : QG);
    if (t < cnt) {
      const double tau = a.times[q0 + t], dtau = dir * tau;
      // the block: the first one whose end time is not before tau (a tau on an interior boundary belongs to the block it ends);
      // a tau outside the data takes the first / last block
      int lo = 0, hi = a.nb - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (dtau <= dir * a.tb[mid + 1]) hi = mid;
        else lo = mid + 1;
      }
      if (a.n_outside && !(dtau >= dir * t0 && dtau <= dir * tf)) atomicAdd(a.n_outside, 1ull);
      const double tb0 = a.tb[lo], h = a.tb[lo + 1] - tb0, s = (tau - tb0) / h, ih = 1.0 / h;
      double* b = sb + t * LD;
      se[t] = lo;
      b[0] = tb0 + h * s;
#pragma unroll
      for (int i = 0; i < CS; i++) {
        double p, dp, wx[2 * CS], wd[2 * CS], wu[CS];
#pragma unroll
        for (int k = 0; k < 2 * CS; k++) wx[k] = bs.xw[i][k], wd[k] = bs.dxw[i][k];
#pragma unroll
        for (int k = 0; k < CS; k++) wu[k] = bs.uw[i][k];
        interp_poly<2 * CS>(wx, s, p, dp);
        b[1 + i] = p, b[1 + 3 * CS + i] = dp * ih;
        interp_poly<2 * CS>(wd, s, p, dp);
        b[1 + CS + i] = p * h, b[1 + 4 * CS + i] = dp;
        interp_poly<CS>(wu, s, p, dp);
        b[1 + 2 * CS + i] = p, b[1 + 5 * CS + i] = dp * ih;
      }
    }
    __syncthreads();
    const bool deriv = a.dout != nullptr;
    for (int k = t; k < cnt * N; k += 256) {
      const int ql = k / N, c = k - ql * N;
      const double* b = sb + ql * LD;
      const double* x = a.traj + size_t(se[ql]) * K * N + c;
      double v, dv;
      if (c < n) {
        const double* xd = a.xdot + size_t(se[ql]) * K * n + c;
        v = dv = 0.0;
#pragma unroll
        for (int i = 0; i < CS; i++) {
          const double xi = x[i * N], fi = xd[i * n];
          v = fma(fi, b[1 + CS + i], fma(xi, b[1 + i], v));
          if (deriv) dv = fma(fi, b[1 + 4 * CS + i], fma(xi, b[1 + 3 * CS + i], dv));
        }
      } else if (c == n) {
        v = b[0], dv = 1.0;
      } else if (BLOCKED) {   // BlockConstant: the block's first row's controls and parameters, copied (LGLInterpTable.h:608-611)
        v = x[0], dv = 0.0;
      } else {
        v = dv = 0.0;
#pragma unroll
        for (int i = 0; i < CS; i++) {
          const double ui = x[i * N];
          v = fma(ui, b[1 + 2 * CS + i], v);
          if (deriv) dv = fma(ui, b[1 + 5 * CS + i], dv);
        }
      }
      a.out[q0 * N + k] = v;
      if (deriv) a.dout[q0 * N + k] = dv;
    }
    __syncthreads();
  }
}

}  // namespace asset_hip
