// Batched propagation of initial-value problems on the device: end states, states at intermediate times, and the derivative of the
// end state with respect to what went in (the state-transition matrix, STM).
//
// Replaces Integrator::integrate_parallel / integrate_dense_parallel / integrate_stm_parallel of the reference (Integrators/
// Integrator.h:1788-1832, 1917-1946, 2071-2130: one host thread per problem) for an integrator WITHOUT a controller: controls and
// parameters are those of the problem's row [x0, t0, u, p], held for the whole propagation (Integrator.h:204-209).
//
// STEP RULE: that of integ_kernels.h (a restatement of Integrator::integrate_impl and its stepper), stated again here so that the
// estimator's kernel keeps its text: first step 0.9 H / (int(|H / DefStepSize|) + 1), H = tf - t0; 13 stages K_s = h f(x + sum a_sj K_j,
// t + c_s h) of the Prince-Dormand 8(7) pair (rk_tables.h), the order-8 solution propagated; the worst |x8 - x7|_k / (AbsTol_k + |x8_k|
// RelTol_k) drives h <- 0.9 h (acc / err)^(1/8), its ratio clamped to [1 / MaxStepChange, MaxStepChange], |h| to [MinStepSize, MaxStepSize];
// a step with err > acc is taken again unless h was raised to MinStepSize; status 1 once accepted + rejected reaches max_steps, 2 when
// the step or a state stops being finite (or the row is not finite); either direction of time.
//
// OUTPUT TIMES (prop_batch_kernel, ns > 1): sample j = 1 .. ns - 1 is the state at t0 + (j H) / (ns - 1) (the last one at tf itself), and
// sample 0 is x0.  Every output time is reached by shortening the step that would reach or pass it -- the rule the step rule applies at
// tf -- so the samples are integrator-accurate, not interpolated; an output time that rounds to the time already reached (|H| / (ns - 1)
// below the spacing of doubles at t0) takes the state as it is, without a step of size 0.  The controller is not restarted there: after an accepted step that
// was shortened from h_full to hit an output time, the next step is the controller's new h or h_full, whichever is larger in size
// (h_full was the step the controller had asked for; without this a sliver in front of an output time would cost a dozen steps of
// growth by MaxStepChange, and a fixed-step propagation would keep the sliver's size for good).  Difference from the reference:
// integrate_dense (Integrator.h:1917-1946) integrates once and interpolates its stored step table, so its end state is the ns = 1 one
// bit for bit; here the shortened steps change the step sequence, and the end state of a dense call agrees with the ns = 1 call to
// the integrator's tolerance, not bitwise.
// tf == t0: every sample is x0, steps 0, 0, status 0.  A lane whose status is not 0 writes NaN to the samples it has not reached.
//
// prop_batch_kernel<Ode>: lane <-> problem.  Layout as integ_reintegrate_kernel: the 13 stage vectors in LDS as [stage][state][lane],
// ONE call site of the right-hand side inside a stage loop that is not unrolled, `lanes` (capi/propagate_plan.h; = integ_lanes(n))
// active lanes per one-wave workgroup.  A wave runs as long as its slowest lane.
//
// prop_stm_kernel<Ode>: lane <-> (problem, column c of S = d x(tf) / d [x0, u, p], C = n + UV + PV columns).  A group of G lanes serves one
// problem and 64 / G problems share a wave (capi/propagate_plan.h).  Every lane of a group integrates the problem's state itself: the
// same instructions on the same data, hence bitwise the same values and the same accept / reject decisions in every lane of the
// group -- no cross-lane operation and no barrier inside the step loop.  Beside the state the lane carries its column through the
// same stages of the same steps: KC_s = h J(X_s) w_s with w_s the lane's direction in ODE-input space (the column's stage value in the
// state slots, 0 for the time, the unit entry of a control or parameter column).  That is the exact derivative of the discrete map
// with the step sequence held fixed -- what Integrator::calculate_jacobian chains step by step (Integrator.h:1317-1349).  The error
// control looks at the state only; the state's stages evaluate Ode::f, as prop_batch_kernel does, so the end states of the two kernels
// are the same bit for bit.  The Jacobian is never stored: Ode::fj hands every entry J(k, i, v) to an accessor that does
// acc[k] = fma(v, w[i], acc[k]) (n + N registers where a stored Jacobian takes n N).  The state's stage vectors are kept once per
// group ([stage][state][group]: every lane of the group writes the same value and reads one address, a broadcast), the column's per
// lane.  When the plan has passes > 1 a lane walks columns c, c + G, .. and integrates the state again in every pass.
//
// prop_stm_jac_kernel<Ode>, thread <-> problem: J[m][n][N + 1] row-major, columns in ODE-input order and the end time,
// [x0 (n) | t0 | u | p | tf] (the reference's IRows + 1 layout, Integrator.h:197).  The x0, u, p columns are S: the DISCRETE map's
// derivative.  The two time columns are the FLOW's: d xf / d tf = f(xf, tf, u, p),  d xf / d t0 = -S_x f(x0, t0, u, p).
// tf == t0 gives S_x = I and zero control and parameter columns.
#pragma once
#include <hip/hip_runtime.h>

#include "integ_kernels.h"

namespace asset_hip {

struct PropArgs {
  long long m;                   // problems
  int ns;                        // samples per problem (batch kernel), >= 1
  int group, lanes, passes;      // capi/propagate_plan.h
  const double* y0;              // [m][N] rows [x0, t0, u, p]
  const double* tf;              // [m]
  const double* abs_tols;        // [n]
  const double* rel_tols;        // [n]
  IntegOptions opt;
  double* xs;                    // batch: [m][ns][n];  stm: [m][n] end states (lane 0 of the group)
  double* xlast;                 // stm: [m][n] end states as the LAST lane of the group holds them (may be null)
  double* S;                     // stm: [m][n][C]
  double* jac;                   // stm: [m][n][N + 1]
  int* steps;                    // [m][2] accepted, rejected
  int* status;                   // [m]
};

extern __shared__ double prop_lds[];

// One step's controller (integ_kernels.h:208-228): updates h, returns whether the step is rejected.
__device__ inline bool prop_controller(const IntegOptions& o, double err, double acc, double& h) {
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
  return (err - acc) > 0.0 && !hit_min;
}

template <class Ode>
__global__ __launch_bounds__(64) void prop_batch_kernel(PropArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, S = RK_STAGES;
  double* sk = prop_lds;                             // [stage][state][lane]
  const int L = a.lanes, t = threadIdx.x;
  const long long i = (long long)blockIdx.x * L + t;
  if (t >= L || i >= a.m) return;                    // (no barrier below: a lane only reads what it wrote)
  const double* row = a.y0 + i * N;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int ns = a.ns;
  double* out = a.xs + i * (long long)ns * n;
  double x[n], xn[n], u[UV > 0 ? UV : 1];
#pragma unroll
  for (int j = 0; j < UV; j++) u[j] = row[n + 1 + j];
  const double t0 = row[n], tf = a.tf[i];
  bool ok = integ_finite(t0) && integ_finite(tf);
#pragma unroll
  for (int k = 0; k < n; k++) {
    x[k] = row[k];
    ok = ok && integ_finite(x[k]);
  }
  if (ns > 1)
    for (int k = 0; k < n; k++) out[k] = x[k];
  const IntegOptions o = a.opt;
  const double H = tf - t0;
  int accepted = 0, rejected = 0, status = ok ? INTEG_OK : INTEG_NONFINITE;
  int j = ns > 1 ? 1 : 0;                            // next sample to write
  if (ok && H == 0.0) {
    for (; j < ns; j++)
      for (int k = 0; k < n; k++) out[j * n + k] = x[k];
  } else if (ok) {
    const int numsteps = int(fabs(H / o.def_step)) + 1;
    double h = 0.9 * (H / double(numsteps)), tc = t0;
    const int nseg = ns > 1 ? ns - 1 : 1;
    for (; j < ns && status == INTEG_OK; j++) {
      const int js = ns > 1 ? j : 1;
      const double tt = js == nseg ? tf : t0 + (double(js) * H) / double(nseg);   // this sample's time
      bool go = tt != tc;                            // (an output time that rounds to the current time: the state, without a step)
      while (go) {
        if (accepted + rejected >= o.max_steps) {
          status = INTEG_STEP_LIMIT;
          break;
        }
        // a step that reaches or passes the output time ends there
        double tnext = tc + h;
        const double hfull = h;
        bool last = false;
        if (H > 0.0 ? (tnext - tt) >= 0.0 : (tnext - tt) <= 0.0) {
          h = tt - tc;
          tnext = tt;
          last = true;
        }
        const double hs = tnext - tc;
        // ---- the 13 stages: ONE call site of the right-hand side
#pragma unroll 1
        for (int s = 0; s < S; s++) {
          double xs[n];
#pragma unroll
          for (int k = 0; k < n; k++) xs[k] = x[k];
          for (int q = 0; q < s; q++) {
            const double asq = d_rk_tab.a[s - 1][q];
#pragma unroll
            for (int k = 0; k < n; k++) xs[k] += asq * sk[(q * n + k) * L + t];
          }
          const double ts = s == 0 ? tc : tc + d_rk_tab.c[s > 0 ? s - 1 : 0] * hs;
          IntegIn<Ode> in{xs, ts, u, row};
          ValueOut<n> fo;
          Ode::f(in, fo);
#pragma unroll
          for (int k = 0; k < n; k++) sk[(s * n + k) * L + t] = fo.v[k] * hs;
        }
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
            if (q > worst) worst = q, err = ek, acc = ak;
          }
          reject = prop_controller(o, err, acc, h);
        }
        if (reject) {
          rejected++;
          continue;
        }
        accepted++;
#pragma unroll
        for (int k = 0; k < n; k++) x[k] = xn[k];
        tc = tnext;
        if (last) {
          if (fabs(h) < fabs(hfull)) h = hfull;      // the controller carries on across an output time
          go = false;
        }
      }
      if (status == INTEG_OK)
        for (int k = 0; k < n; k++) out[j * n + k] = x[k];
    }
    if (status != INTEG_OK) j--;                     // (the loop's increment: sample j was not reached)
  }
  for (; j < ns; j++)                                // samples not reached
    for (int k = 0; k < n; k++) out[j * n + k] = qnan;
  a.steps[i * 2] = accepted;
  a.steps[i * 2 + 1] = rejected;
  a.status[i] = status;
}

// Ode::fj output: the Jacobian contracted with the lane's direction as its entries arrive.  The value is NOT taken from here: the
// state's stages call Ode::f, the body prop_batch_kernel calls, so that the states of the two kernels are the same bit for bit (the f
// and fj bodies of a generated ODE order their operations differently: Reentry's differ by a few units in the last place).
template <int NX, int NIN>
struct JvpOut {
  double acc[NX], w[NIN];
  __device__ void f(int, double) {}
  __device__ void J(int k, int i, double x) { acc[k] = fma(x, w[i], acc[k]); }
};

template <class Ode>
__global__ __launch_bounds__(64) void prop_stm_kernel(PropArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, S = RK_STAGES, C = N - 1;
  const int L = a.lanes, G = a.group, PW = L / G, t = threadIdx.x;
  double* sx = prop_lds;                             // [stage][state][group of the workgroup]
  double* sc = prop_lds + S * n * PW;                // [stage][state][lane]
  const int g = t / G, c0 = t % G;
  const long long i = (long long)blockIdx.x * PW + g;
  if (t >= L || i >= a.m) return;
  const double* row = a.y0 + i * N;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double u[UV > 0 ? UV : 1];
#pragma unroll
  for (int j = 0; j < UV; j++) u[j] = row[n + 1 + j];
  const double t0 = row[n], tf = a.tf[i];
  const IntegOptions o = a.opt;
  const double H = tf - t0;
  for (int pass = 0; pass < a.passes; pass++) {
    const int c = pass * G + c0;                     // this lane's column (c >= C: none; the lane carries zeros)
    double x[n], xn[n], sv[n], svn[n];
    bool ok = integ_finite(t0) && integ_finite(tf);
#pragma unroll
    for (int k = 0; k < n; k++) {
      x[k] = row[k];
      sv[k] = k == c ? 1.0 : 0.0;
      ok = ok && integ_finite(x[k]);
    }
    int accepted = 0, rejected = 0, status = ok ? INTEG_OK : INTEG_NONFINITE;
    if (ok && H != 0.0) {
      const int numsteps = int(fabs(H / o.def_step)) + 1;
      double h = 0.9 * (H / double(numsteps)), tc = t0;
      bool go = true;
      while (go) {
        if (accepted + rejected >= o.max_steps) {
          status = INTEG_STEP_LIMIT;
          break;
        }
        double tnext = tc + h;
        bool last = false;
        if (H > 0.0 ? (tnext - tf) >= 0.0 : (tnext - tf) <= 0.0) {
          h = tf - tc;
          tnext = tf;
          last = true;
        }
        const double hs = tnext - tc;
        // ---- the 13 stages: ONE call site of the right-hand side and one of its Jacobian
#pragma unroll 1
        for (int s = 0; s < S; s++) {
          double xs[n];
          JvpOut<n, N> fo;
#pragma unroll
          for (int k = 0; k < n; k++) xs[k] = x[k], fo.w[k] = sv[k], fo.acc[k] = 0.0;
          for (int q = 0; q < s; q++) {
            const double asq = d_rk_tab.a[s - 1][q];
#pragma unroll
            for (int k = 0; k < n; k++) {
              xs[k] += asq * sx[(q * n + k) * PW + g];
              fo.w[k] += asq * sc[(q * n + k) * L + t];
            }
          }
#pragma unroll
          for (int k = n; k < N; k++) fo.w[k] = (k > n && k - 1 == c) ? 1.0 : 0.0;
          const double ts = s == 0 ? tc : tc + d_rk_tab.c[s > 0 ? s - 1 : 0] * hs;
          IntegIn<Ode> in{xs, ts, u, row};
          ValueOut<n> fv;
          Ode::f(in, fv);
          Ode::fj(in, fo);
#pragma unroll
          for (int k = 0; k < n; k++) {
            sx[(s * n + k) * PW + g] = fv.v[k] * hs;
            sc[(s * n + k) * L + t] = fo.acc[k] * hs;
          }
        }
        double xe[n];
#pragma unroll
        for (int k = 0; k < n; k++) xn[k] = x[k], xe[k] = x[k], svn[k] = sv[k];
        for (int s = 0; s < S; s++) {
          const double b = d_rk_tab.b[s], bh = d_rk_tab.bhat[s];
#pragma unroll
          for (int k = 0; k < n; k++) {
            const double ks = sx[(s * n + k) * PW + g];
            xn[k] += b * ks;
            xe[k] += bh * ks;
            svn[k] += b * sc[(s * n + k) * L + t];
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
            if (q > worst) worst = q, err = ek, acc = ak;
          }
          reject = prop_controller(o, err, acc, h);
        }
        if (reject) {
          rejected++;
          continue;
        }
        accepted++;
#pragma unroll
        for (int k = 0; k < n; k++) x[k] = xn[k], sv[k] = svn[k];
        tc = tnext;
        if (last) go = false;
      }
    }
    const bool good = status == INTEG_OK;
    if (c < C)
      for (int k = 0; k < n; k++) a.S[(i * n + k) * C + c] = good ? sv[k] : qnan;
    if (pass == 0 && c0 == 0) {
      for (int k = 0; k < n; k++) a.xs[i * n + k] = good ? x[k] : qnan;
      a.steps[i * 2] = accepted;
      a.steps[i * 2 + 1] = rejected;
      a.status[i] = status;
    }
    if (pass == 0 && c0 == G - 1 && a.xlast)
      for (int k = 0; k < n; k++) a.xlast[i * n + k] = good ? x[k] : qnan;
  }
}

template <class Ode>
__global__ __launch_bounds__(64) void prop_stm_jac_kernel(PropArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, C = N - 1, LDJ = N + 1;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.m) return;
  const double* row = a.y0 + i * N;
  const double* Sm = a.S + i * n * C;
  double* J = a.jac + i * n * LDJ;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  if (a.status[i] != INTEG_OK) {
    for (int k = 0; k < n * LDJ; k++) J[k] = qnan;
    return;
  }
  double x[n], u[UV > 0 ? UV : 1];
#pragma unroll
  for (int j = 0; j < UV; j++) u[j] = row[n + 1 + j];
  ValueOut<n> f0, ff;
#pragma unroll
  for (int k = 0; k < n; k++) x[k] = row[k];
  {
    IntegIn<Ode> in{x, row[n], u, row};
    Ode::f(in, f0);
  }
#pragma unroll
  for (int k = 0; k < n; k++) x[k] = a.xs[i * n + k];
  {
    IntegIn<Ode> in{x, a.tf[i], u, row};
    Ode::f(in, ff);
  }
  for (int k = 0; k < n; k++) {
    double dt0 = 0.0;
    for (int c = 0; c < n; c++) {
      const double s = Sm[k * C + c];
      J[k * LDJ + c] = s;
      dt0 = fma(s, f0.v[c], dt0);
    }
    J[k * LDJ + n] = -dt0;
    for (int c = n; c < C; c++) J[k * LDJ + c + 1] = Sm[k * C + c];
    J[k * LDJ + N] = ff.v[k];
  }
}

}  // namespace asset_hip
