// Integrator-based mesh-error estimate of a phase trajectory on the device.
//
// Replaces ODEPhase<DODE>::get_meshinfo_integrator (OptimalControl/ODEPhase.h:592-685 of the reference): the ODE is integrated
// again across every node interval of the trajectory with the Prince-Dormand 8(7) pair (rk_tables.h), the control taken from the
// transcription's own polynomial, and the distance of each integrated state from the next node is the error of that interval.
//
// STAGE 1 (integ_reintegrate_kernel), lane <-> node interval i = 0 .. nodes - 2: the initial-value problem from row i to t_(i+1), a
// restatement of Integrator::integrate_impl and its stepper (Integrators/Integrator.h:536-676, :383-480) -- first step
// 0.9 H / (int(|H / DefStepSize|) + 1), a step that reaches t_(i+1) is shortened to end there, 13 stages K_s = h f(x + sum a_sj K_j,
// t + c_s h), the order-8 solution propagated, the worst |x8 - x7|_k / (AbsTol_k + |x8_k| RelTol_k) drives
// h <- 0.9 h (acc / err)^(1/8) (its ratio clamped to [1 / MaxStepChange, MaxStepChange], |h| to [MinStepSize, MaxStepSize]); a step with
// err > acc is taken again unless h was raised to MinStepSize.  Controls: held at the start row's for ODEs without controls and for
// BlockConstant phases (the reference builds its re-integrator without a controller then, ODEPhase.h:142-162), otherwise the block's
// degree cs - 1 polynomial through its nodes (interp_kernels.h: the uw rows of interp_basis).  ODE parameters stay the start row's.
// One difference from the reference: its block search gives a time on a block boundary to the block that ends there, so the first
// stage of a block's first interval sees the previous block's polynomial at s = 1; here it is this block's at s = 0 -- the shared
// node's control either way, up to rounding.
// What the reference does not have: a cap on the steps of an interval (accepted + rejected, IntegOptions::max_steps).  Its loop does not
// end once h is NaN; a lane here stops at the cap (status 1) or when its step or state stops being finite (status 2, looked at every
// step; also when the interval's own rows are not finite) and reports NaN end states.
//
// Layout: consecutive lanes take consecutive intervals (neighbours need similar step counts; a wave runs as long as its slowest
// lane).  The rows a workgroup needs are contiguous and come into LDS as one flat coalesced stream, the results leave the same way
// (interp_kernels.h, stage 1).  The right-hand side is called at ONE place, inside the stage loop, which is not unrolled: the body of
// a heavy ODE is thousands of instructions.  The stage number is therefore a run-time index, and the 13 stage vectors live in LDS as
// [stage][state][lane]: lane l reads 8 bytes at 8 l + const, all 64 banks once per half wave, no conflict.  That is 13 n 8 bytes per
// lane, so a workgroup (one wave) works with integ_lanes(n) active lanes: 64 up to n = 7, 32 / 16 / 8 beyond.
//
// STAGE 2 (integ_mesh_error_kernel), thread <-> block (ODEPhase.h:630-666): with e[i][k] = |xend_i,k - x_(i+1),k| and max_err their
// maximum (NaN if any is NaN),  mesh_errors[:, b] = sum_j e[start + j] |(t_(j+1) - t_j) / (tf_b - t0_b)|,
// mesh_dist[:, b] = (mesh_errors[:, b] / (|tf_b - t0_b|^(Order+1) max_err))^(1 / (Order+1)),  tsnd[b] = (t0_b - T0) / (TF - T0); the last
// column repeats the one before, and the per-block infinity norms follow mesh_error_kernel's NaN rule.
#pragma once
#include <hip/hip_runtime.h>

#include "interp_kernels.h"
#include "rk_tables.h"

namespace asset_hip {

struct IntegOptions {   // Integrator.h:297-310; the defaults of a phase: asset_hip_mesh_error_integrator
  double def_step, min_step, max_step, max_step_change;
  int adaptive, max_steps;
};
enum IntegStatus { INTEG_OK = 0, INTEG_STEP_LIMIT = 1, INTEG_NONFINITE = 2 };

struct IntegArgs {
  int nb;                        // blocks; nodes = nb*(cs-1) + 1, intervals = nodes - 1
  const double* traj;            // [nodes][N] node rows [x, t, u, p]
  const double* abs_tols;        // [n]
  const double* rel_tols;        // [n]
  IntegOptions opt;
  double* xend;                  // [intervals][n] integrated end states (NaN where status != 0)
  int* steps;                    // [intervals][2] accepted, rejected
  int* status;                   // [intervals]
  double* e;                     // [intervals][n] |xend - next node|
  unsigned long long* max_err;   // bits of max e; zero before stage 1 (non-negative doubles and NaN order as unsigned integers)
  double* tsnd;                  // [nb+1]
  double* errors;                // [nb+1][n]
  double* dist;                  // [nb+1][n]
  double* error_max;             // [nb+1]
  double* dist_max;              // [nb+1]
};

// active lanes of a (one-wave) workgroup: the 13 stage vectors of a lane take 13 n doubles of LDS
__host__ __device__ constexpr int integ_lanes(int n) {
  int l = 64;
  while (l > 1 && size_t(RK_STAGES) * n * l * sizeof(double) > 48 * 1024) l >>= 1;
  return l;
}

template <class Ode>
struct IntegIn {   // ODE input of a stage: the stage's state and time, its controls, the start row's parameters
  const double* x;
  double t;
  const double* u;
  const double* row;
  __device__ double y(int i) const {
    return i < Ode::XV ? x[i] : (i == Ode::XV ? t : (i < Ode::XV + 1 + Ode::UV ? u[i - Ode::XV - 1] : row[i]));
  }
  __device__ double lam(int) const { return 0.0; }
};

__device__ inline bool integ_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }   // false for NaN

template <class Ode, int SCH, bool BLOCKED>
__global__ __launch_bounds__(64) void integ_reintegrate_kernel(IntegArgs a) {
  constexpr InterpBasis bs = interp_basis(SCH);
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, CS = interp_basis(SCH).cs, K = CS - 1, T = n;
  constexpr int L = integ_lanes(n), S = RK_STAGES;
  constexpr bool HELD = UV == 0 || BLOCKED;          // controls held at the start row's
  constexpr int LDN = N | 1, LDX = n | 1;            // odd row lengths: lanes reading one column of different rows do not collide
  constexpr int MAXROWS = L + 2 * K;                 // rows of the workgroup's intervals and of the blocks they lie in
  constexpr bool STAGED = size_t(S) * n * L * 8 + size_t(MAXROWS) * LDN * 8 + 64 * 8 <= 60 * 1024;
  constexpr int RS = STAGED ? LDN : N;               // stride of the rows a lane reads
  static_assert(2 * L * LDX <= S * n * L, "the results are staged in the stage vectors' space");
  __shared__ double sk[S * n * L];                   // [stage][state][lane]; afterwards xend | e rows
  __shared__ double srow[STAGED ? MAXROWS * LDN : 1];
  __shared__ unsigned long long smax[64];
  const long long nint = (long long)a.nb * K;
  const long long i0 = (long long)blockIdx.x * L;
  const int cnt = int(nint - i0 < L ? nint - i0 : L), t = threadIdx.x;
  if (cnt <= 0) return;
  const long long r0 = (i0 / K) * K, r1 = ((i0 + cnt - 1) / K) * K + K;   // first and last row needed (r1 <= nodes - 1: a block's end)
  if constexpr (STAGED) {
    const int nrow = int(r1 - r0 + 1);
    for (int k = t; k < nrow * N; k += 64) srow[(k / N) * LDN + (k % N)] = a.traj[r0 * N + k];
    __syncthreads();
  }
  const bool active = t < cnt;
  double x[n], xn[n];
  int accepted = 0, rejected = 0, status = INTEG_OK;
  unsigned long long emax = 0ull;
  if (active) {
    const long long i = i0 + t, blk = i / K;
    auto rowp = [&](long long r) -> const double* { return STAGED ? srow + (r - r0) * LDN : a.traj + r * N; };
    const double* row = rowp(i);
    const double* next = rowp(i + 1);
    const double* first = rowp(blk * K);             // the block's rows: its control polynomial
    const double tb0 = first[T], hb = first[K * RS + T] - tb0;
    double u[UV > 0 ? UV : 1];
#pragma unroll
    for (int j = 0; j < UV; j++) u[j] = row[n + 1 + j];
    const double t0 = row[T], tf = next[T];
    double tc = t0;
    bool ok = integ_finite(t0) && integ_finite(tf);
#pragma unroll
    for (int k = 0; k < n; k++) {
      x[k] = row[k];
      ok = ok && integ_finite(x[k]) && integ_finite(next[k]);
    }
    const IntegOptions o = a.opt;
    const double H = tf - t0;
    const int numsteps = int(fabs(H / o.def_step)) + 1;
    double h = 0.9 * (H / double(numsteps));
    if (!ok) status = INTEG_NONFINITE;
    bool go = ok;
    while (go) {
      if (accepted + rejected >= o.max_steps) {
        status = INTEG_STEP_LIMIT;
        break;
      }
      // a step that reaches or passes tf ends there; it is the last one if it is accepted
      double tnext = tc + h;
      bool last = false;
      if (H > 0.0 ? (tnext - tf) >= 0.0 : (tnext - tf) <= 0.0) {
        h = tf - tc;
        tnext = tf;
        last = true;
      }
      const double hs = tnext - tc;                  // the stepper's own step (Integrator.h:400-401)
      // ---- the 13 stages: ONE call site of the right-hand side
#pragma unroll 1
      for (int s = 0; s < S; s++) {
        double xs[n];
#pragma unroll
        for (int k = 0; k < n; k++) xs[k] = x[k];
        for (int j = 0; j < s; j++) {
          const double asj = d_rk_tab.a[s - 1][j];
#pragma unroll
          for (int k = 0; k < n; k++) xs[k] += asj * sk[(j * n + k) * L + t];
        }
        const double ts = s == 0 ? tc : tc + d_rk_tab.c[s > 0 ? s - 1 : 0] * hs;
        if constexpr (!HELD) {
          const double sl = (ts - tb0) / hb;
          double ups[CS];
#pragma unroll
          for (int i2 = 0; i2 < CS; i2++) {
            double w[CS], dp;
#pragma unroll
            for (int k = 0; k < CS; k++) w[k] = bs.uw[i2][k];
            interp_poly<CS>(w, sl, ups[i2], dp);
          }
#pragma unroll
          for (int j = 0; j < UV; j++) {
            double v = 0.0;
#pragma unroll
            for (int i2 = 0; i2 < CS; i2++) v = fma(first[i2 * RS + n + 1 + j], ups[i2], v);
            u[j] = v;
          }
        }
        IntegIn<Ode> in{xs, ts, u, row};
        ValueOut<n> out;
        Ode::f(in, out);
#pragma unroll
        for (int k = 0; k < n; k++) sk[(s * n + k) * L + t] = out.v[k] * hs;
      }
      // ---- the two solutions and the controller
      double xe[n];
#pragma unroll
      for (int k = 0; k < n; k++) xn[k] = x[k], xe[k] = x[k];
      for (int s = 0; s < S; s++) {
        const double b = d_rk_tab.b[s], bh = d_rk_tab.bhat[s];
#pragma unroll
        for (int k = 0; k < n; k++) {
          const double ks = sk[(s * n + k) * L + t];
          xn[k] += b * ks;
          xe[k] += bh * ks;
        }
      }
      bool fin = integ_finite(h);
#pragma unroll
      for (int k = 0; k < n; k++) fin = fin && integ_finite(xn[k]);
      if (!fin) {
        status = INTEG_NONFINITE;
        break;
      }
      bool reject = false;
      if (o.adaptive) {
        double worst = -1.0, err = 0.0, acc = 1.0;
#pragma unroll
        for (int k = 0; k < n; k++) {
          const double ek = fabs(xn[k] - xe[k]), ak = a.abs_tols[k] + fabs(xn[k]) * a.rel_tols[k];
          const double q = ek / ak;
          if (q > worst) worst = q, err = ek, acc = ak;      // (the first of equal maxima, as maxCoeff)
        }
        const double hnext = 0.9 * h * pow(acc / err, 1.0 / 8.0);
        if (hnext / h > o.max_step_change) h *= o.max_step_change;
        else if (hnext / h < 1.0 / o.max_step_change) h /= o.max_step_change;
        else h = hnext;
        if (fabs(h) > o.max_step) h = o.max_step * h / fabs(h);
        bool hit_min = false;
        if (fabs(h) < o.min_step) {
          h = o.min_step * h / fabs(h);
          hit_min = true;
        }
        reject = (err - acc) > 0.0 && !hit_min;
      }
      if (reject) {
        rejected++;
        continue;
      }
      accepted++;
#pragma unroll
      for (int k = 0; k < n; k++) x[k] = xn[k];
      tc = tnext;
      if (last) go = false;
    }
  }
  // ---- results: rows of xend and e in the stage vectors' space, once every lane is done with its stage vectors
  __syncthreads();
  double* sx = sk;
  double* se = sk + L * LDX;
  if (active) {
    const double* next = STAGED ? srow + (i0 + t + 1 - r0) * LDN : a.traj + (i0 + t + 1) * N;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int k = 0; k < n; k++) {
      const double xk = status == INTEG_OK ? x[k] : qnan;
      const double ev = fabs(xk - next[k]);
      sx[t * LDX + k] = xk;
      se[t * LDX + k] = ev;
      const unsigned long long bits = (unsigned long long)__double_as_longlong(ev);
      emax = bits > emax ? bits : emax;
    }
    a.steps[(i0 + t) * 2] = accepted;
    a.steps[(i0 + t) * 2 + 1] = rejected;
    a.status[i0 + t] = status;
  }
  smax[t] = emax;
  __syncthreads();
  for (int k = t; k < cnt * n; k += 64) {
    a.xend[i0 * n + k] = sx[(k / n) * LDX + (k % n)];
    a.e[i0 * n + k] = se[(k / n) * LDX + (k % n)];
  }
  if (t == 0) {
    unsigned long long m = 0ull;
    for (int k = 0; k < cnt; k++) m = smax[k] > m ? smax[k] : m;
    atomicMax(a.max_err, m);
  }
}

// thread <-> block (a template only so that every translation unit may hold a copy)
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void integ_mesh_error_kernel(IntegArgs a, int n, int N, int K, double order) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.nb) return;
  const int T = n;
  const long long start = (long long)b * K;
  const double T0 = a.traj[T], TF = a.traj[(long long)a.nb * K * N + T];
  const double t0 = a.traj[start * N + T], tf = a.traj[(start + K) * N + T];
  const double max_err = __longlong_as_double((long long)*a.max_err);
  const double h = fabs(tf - t0), den = pow(h, order + 1.0) * max_err, ipow = 1.0 / (order + 1.0);
  double emax = 0.0, dmax = 0.0;
  for (int k = 0; k < n; k++) {
    double ev = 0.0;
    for (int j = 0; j < K; j++) {
      const double ti = a.traj[(start + j) * N + T], tn = a.traj[(start + j + 1) * N + T];
      ev += a.e[(start + j) * n + k] * fabs((tn - ti) / (tf - t0));
    }
    const double dv = pow(ev / den, ipow);
    a.errors[size_t(b) * n + k] = ev;
    a.dist[size_t(b) * n + k] = dv;
    emax = (fabs(ev) > emax || ev != ev) ? fabs(ev) : emax;
    dmax = (fabs(dv) > dmax || dv != dv) ? fabs(dv) : dmax;
    if (b == a.nb - 1) {
      a.errors[size_t(a.nb) * n + k] = ev;
      a.dist[size_t(a.nb) * n + k] = dv;
    }
  }
  a.tsnd[b] = (t0 - T0) / (TF - T0);
  a.error_max[b] = emax;
  a.dist_max[b] = dmax;
  if (b == a.nb - 1) a.tsnd[a.nb] = 1.0, a.error_max[a.nb] = emax, a.dist_max[a.nb] = dmax;
}

}  // namespace asset_hip
