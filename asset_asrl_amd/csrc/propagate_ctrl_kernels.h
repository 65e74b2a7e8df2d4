// Batched propagation with a controller: the controls of a stage are a feedback law of the stage's own state, time and parameters.
//
// Replaces Integrator::integrate_parallel / integrate_dense_parallel / integrate_stm_parallel of the reference for an integrator WITH
// a controller (Integrators/Integrator.h:96-118, 190-249, 373-381, 398-463): `ode.integrator(def_step, ucon, varlocs)` evaluates
// u = ucon(row[varlocs]) at every Runge-Kutta stage.  The STEP RULE and the OUTPUT TIMES are those of propagate_kernels.h, statement
// for statement; so are the LDS layouts ([stage][state][lane]; in the STM kernel the state's stages once per lane group) and the
// launch plan (capi/propagate_plan.h).
//
// CONTROLLER.  Ctl is a generated functor of the FULL ODE input row [x, t, u, p] (Ctl::NIN == Ode::NIN) with Ctl::XV == Ode::UV outputs:
// the host composes the law with the selection of `varlocs` through the DSL, so which entries of the row the law reads is compile-time
// content of the module -- nothing indexes a register array at run time.  The law does not read the control slots (the host refuses
// a `varlocs` entry inside them), and the u columns of the initial rows are ignored.  The kernels reach the law through two
// functions only, ctrl_value and ctrl_jvp: a controller of another kind (a trajectory's control table) overloads those two for its
// own policy type and leaves the stage loops as they are.
//
// At stage s:  u_s = Ctl(x_s, t_s, ., p),  K_s = h Ode::f(x_s, t_s, u_s, p)  -- one call site of Ctl::f and one of Ode::f inside the stage
// loop, which is not unrolled.  A u_s that is not finite makes the stage, hence the step's result, not finite: status 2, as for a
// state that stops being finite.
//
// prop_ctrl_batch_kernel<Ode, Ctl>: lane <-> problem, as prop_batch_kernel.  Beside xs[m][ns][n] it writes us[m][ns][UV], the law's
// value at every sample's own state and time (Integrator.h:462, :557 -- sample 0 too; NaN where the sample was not reached, and for a
// row that is not finite).
//
// prop_ctrl_stm_kernel<Ode, Ctl>: lane <-> (problem, column c of S = d x(tf) / d [x0, p]).  A controlled problem has no control
// columns to carry: C' = n + PV columns, the plan is propagate_plan(n, 0, PV, m, 1).  The lane's direction in ODE-input space at a stage
// is w = [the column's stage value | 0 | w_u | the unit entry of a parameter column] with w_u = J_Ctl(y_s) w: Ctl::fj hands its entries
// to an accessor that contracts them with w as they arrive, then Ode::fj does the same with the completed w.  Neither Jacobian is
// stored.  That is the exact derivative of the discrete closed-loop map with the step sequence held fixed.  The state's stages
// evaluate Ctl::f and Ode::f -- the bodies the batch kernel calls, on the same data -- so the end states and step counts are those of
// the batch kernel bit for bit, and the same in every lane of a group.
//
// prop_ctrl_jac_kernel<Ode, Ctl>, thread <-> problem: J[m][n][N + 1], columns [x0 | t0 | u | p | tf]; the u columns are exactly zero (the
// closed loop does not read them), the x0 and p columns are S, the time columns the flow's: -S_x f(x0, t0, Ctl(.), p) and
// f(xf, tf, Ctl(.), p).  It also writes uf[m][UV] = Ctl(xf, tf, ., p).  A problem whose status is not 0 gets NaN in both.
#pragma once
#include <hip/hip_runtime.h>

#include "propagate_kernels.h"

namespace asset_hip {

struct PropCtrlArgs {
  long long m;                   // problems
  int ns;                        // samples per problem (batch kernel), >= 1
  int group, lanes, passes;      // capi/propagate_plan.h (STM: of (n, 0, PV))
  const double* y0;              // [m][N] rows [x0, t0, u, p]; the u columns are not read
  const double* tf;              // [m]
  const double* abs_tols;        // [n]
  const double* rel_tols;        // [n]
  IntegOptions opt;
  double* xs;                    // batch: [m][ns][n];  stm: [m][n] end states (lane 0 of the group)
  double* us;                    // batch: [m][ns][UV];  stm: [m][UV] the law at the end state (the assembly kernel)
  double* xlast;                 // stm: [m][n] end states as the LAST lane of the group holds them (may be null)
  double* S;                     // stm: [m][n][C'], C' = n + PV
  double* jac;                   // stm: [m][n][N + 1]
  int* steps;                    // [m][2] accepted, rejected
  int* status;                   // [m]
};

// The law's value at an ODE input row: u[UV].
template <class Ode, class Ctl>
__device__ inline void ctrl_value(const IntegIn<Ode>& in, double* u) {
  static_assert(Ctl::NIN == Ode::NIN, "the controller reads the ODE's input row");
  static_assert(Ctl::XV == Ode::UV && Ode::UV >= 1, "the controller gives the ODE's controls");
  ValueOut<Ode::UV> uo;
  Ctl::f(in, uo);
#pragma unroll
  for (int j = 0; j < Ode::UV; j++) u[j] = uo.v[j];
}

// w_u = J_Ctl(row) w for a direction w[NIN] in ODE-input space: written into w's own control slots, which must hold zeros on entry
// (the law does not read them; its Jacobian's entries there are structural zeros).
template <class Ode, class Ctl>
__device__ inline void ctrl_jvp(const IntegIn<Ode>& in, double* w) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV;
  JvpOut<UV, N> co;
#pragma unroll
  for (int k = 0; k < N; k++) co.w[k] = w[k];
#pragma unroll
  for (int j = 0; j < UV; j++) co.acc[j] = 0.0;
  Ctl::fj(in, co);
#pragma unroll
  for (int j = 0; j < UV; j++) w[n + 1 + j] = co.acc[j];
}

template <class Ode, class Ctl>
__global__ __launch_bounds__(64) void prop_ctrl_batch_kernel(PropCtrlArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, S = RK_STAGES;
  double* sk = prop_lds;                             // [stage][state][lane]
  const int L = a.lanes, t = threadIdx.x;
  const long long i = (long long)blockIdx.x * L + t;
  if (t >= L || i >= a.m) return;                    // (no barrier below: a lane only reads what it wrote)
  const double* row = a.y0 + i * N;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int ns = a.ns;
  double* out = a.xs + i * (long long)ns * n;
  double* uout = a.us + i * (long long)ns * UV;
  double x[n], xn[n], u[UV];
#pragma unroll
  for (int j = 0; j < UV; j++) u[j] = 0.0;
  const double t0 = row[n], tf = a.tf[i];
  bool ok = integ_finite(t0) && integ_finite(tf);
#pragma unroll
  for (int k = 0; k < n; k++) {
    x[k] = row[k];
    ok = ok && integ_finite(x[k]);
  }
  const IntegOptions o = a.opt;
  const double H = tf - t0;
  if (ns > 1 || (ok && H == 0.0)) {                  // the law at the row itself: sample 0, and every sample of an arc of length 0
    if (ok) {
      IntegIn<Ode> in{x, t0, u, row};
      ctrl_value<Ode, Ctl>(in, u);
    }
    if (ns > 1) {
      for (int k = 0; k < n; k++) out[k] = x[k];
      for (int k = 0; k < UV; k++) uout[k] = ok ? u[k] : qnan;
    }
  }
  int accepted = 0, rejected = 0, status = ok ? INTEG_OK : INTEG_NONFINITE;
  int j = ns > 1 ? 1 : 0;                            // next sample to write
  if (ok && H == 0.0) {
    for (; j < ns; j++) {
      for (int k = 0; k < n; k++) out[j * n + k] = x[k];
      for (int k = 0; k < UV; k++) uout[j * UV + k] = u[k];
    }
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
        // ---- the 13 stages: ONE call site of the law and ONE of the right-hand side
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
          ctrl_value<Ode, Ctl>(in, u);
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
      if (status == INTEG_OK) {
        IntegIn<Ode> in{x, tt, u, row};              // the law at the sample's own state and time
        ctrl_value<Ode, Ctl>(in, u);
        for (int k = 0; k < n; k++) out[j * n + k] = x[k];
        for (int k = 0; k < UV; k++) uout[j * UV + k] = u[k];
      }
    }
    if (status != INTEG_OK) j--;                     // (the loop's increment: sample j was not reached)
  }
  for (; j < ns; j++) {                              // samples not reached
    for (int k = 0; k < n; k++) out[j * n + k] = qnan;
    for (int k = 0; k < UV; k++) uout[j * UV + k] = qnan;
  }
  a.steps[i * 2] = accepted;
  a.steps[i * 2 + 1] = rejected;
  a.status[i] = status;
}

template <class Ode, class Ctl>
__global__ __launch_bounds__(64) void prop_ctrl_stm_kernel(PropCtrlArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, PV = Ode::PV, S = RK_STAGES, C = n + PV;
  const int L = a.lanes, G = a.group, PW = L / G, t = threadIdx.x;
  double* sx = prop_lds;                             // [stage][state][group of the workgroup]
  double* sc = prop_lds + S * n * PW;                // [stage][state][lane]
  const int g = t / G, c0 = t % G;
  const long long i = (long long)blockIdx.x * PW + g;
  if (t >= L || i >= a.m) return;
  const double* row = a.y0 + i * N;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  double u[UV];
#pragma unroll
  for (int j = 0; j < UV; j++) u[j] = 0.0;
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
        // ---- the 13 stages: ONE call site of the law, of its Jacobian, of the right-hand side and of its Jacobian
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
          // the time and the control slots 0, the unit entry of a parameter column (column c >= n is parameter c - n)
#pragma unroll
          for (int k = n; k < N; k++) fo.w[k] = (k > n + UV && k - 1 - UV == c) ? 1.0 : 0.0;
          const double ts = s == 0 ? tc : tc + d_rk_tab.c[s > 0 ? s - 1 : 0] * hs;
          IntegIn<Ode> in{xs, ts, u, row};
          ctrl_value<Ode, Ctl>(in, u);
          ctrl_jvp<Ode, Ctl>(in, fo.w);
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

template <class Ode, class Ctl>
__global__ __launch_bounds__(64) void prop_ctrl_jac_kernel(PropCtrlArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, PV = Ode::PV, C = n + PV, LDJ = N + 1;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.m) return;
  const double* row = a.y0 + i * N;
  const double* Sm = a.S + i * n * C;
  double* J = a.jac + i * n * LDJ;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  if (a.status[i] != INTEG_OK) {
    for (int k = 0; k < n * LDJ; k++) J[k] = qnan;
    for (int k = 0; k < UV; k++) a.us[i * UV + k] = qnan;
    return;
  }
  double x[n], u[UV];
#pragma unroll
  for (int j = 0; j < UV; j++) u[j] = 0.0;
  ValueOut<n> f0, ff;
#pragma unroll
  for (int k = 0; k < n; k++) x[k] = row[k];
  {
    IntegIn<Ode> in{x, row[n], u, row};
    ctrl_value<Ode, Ctl>(in, u);
    Ode::f(in, f0);
  }
#pragma unroll
  for (int k = 0; k < n; k++) x[k] = a.xs[i * n + k];
  {
    IntegIn<Ode> in{x, a.tf[i], u, row};
    ctrl_value<Ode, Ctl>(in, u);
    Ode::f(in, ff);
  }
  for (int k = 0; k < UV; k++) a.us[i * UV + k] = u[k];
  for (int k = 0; k < n; k++) {
    double dt0 = 0.0;
    for (int c = 0; c < n; c++) {
      const double s = Sm[k * C + c];
      J[k * LDJ + c] = s;
      dt0 = fma(s, f0.v[c], dt0);
    }
    J[k * LDJ + n] = -dt0;
    for (int c = 0; c < UV; c++) J[k * LDJ + n + 1 + c] = 0.0;
    for (int c = n; c < C; c++) J[k * LDJ + 1 + UV + c] = Sm[k * C + c];
    J[k * LDJ + N] = ff.v[k];
  }
}

}  // namespace asset_hip
