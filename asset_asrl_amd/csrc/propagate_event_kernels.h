// Batched propagation with events: propagate until something happens, and say where it happened.
//
// Replaces the Events overloads of Integrator::integrate / integrate_parallel of the reference (Integrators/Integrator.h:536-730,
// 1047-1159) for an integrator without a controller.  The step rule is prop_batch_kernel's (propagate_kernels.h, ns = 1), statement
// for statement, so that a propagation whose events never stop it ends in the same bits.
//
// EVENTS.  Ev is a generated functor of NE = Ev::XV (1 .. PROP_EVENT_MAX) scalar functions g_j of the ODE's input row [x, t, u, p]
// (Ev::NIN == Ode::NIN), value only: Ev::f(in, out).  direction[j] in {-1, 0, +1} and stop[j] >= 0 are run-time arguments.  After every
// ACCEPTED step from (x_i, t_i) to (x_i+1, t_i+1) (Integrator.h:678-704): event j occurred iff g_j(prev) g_j(next) < 0 and
// (direction == 0 or g_j(next) has the sign of direction) -- a value that is exactly zero at a step end never counts.  All events are
// examined for the step; an occurrence raises ev_count[j]; when an event with stop[j] = k > 0 reaches its k-th occurrence the
// propagation ends AT THE END OF THAT ACCEPTED STEP (Integrator.h:725), t_end = t_i+1, stopped = the lowest such j.
//
// LOCATION.  The reference root-finds on the interpolant of its step table.  Here the root is found on the integrator itself, as the
// dense output reaches its samples: x(theta) is the order-8 result of ONE step of size theta h from the START of the bracketing step,
// theta in (0, 1), and the root of G(theta) = g_j(x(theta), t_i + theta h, u, p) is bracketed by G(0) = g_j(prev), G(1) = g_j(next).
// METHOD: Illinois regula falsi -- the secant point of the bracket, and the function value of an end point that has survived two
// updates in a row is halved; superlinear, and the trial point never leaves the bracket (a trial that rounding puts on or outside an
// end is replaced by the midpoint).  The bracket is kept at all times.  One evaluation of G is one 13-stage step; at most max_iters
// evaluations per occurrence.  Done when |G| < event_tol, or when the bracket's half-width in time is < event_tol: the trial point is
// then the bracket's MIDPOINT, so the stored time is within event_tol of the root of G.  An occurrence that uses up its evaluations
// is stored with ev_conv = 0 (also one whose trial state stops being finite).  Per problem and event the first K = max_locs
// occurrences are located and stored; later ones are detected, counted, and count towards stop (the host refuses stop > K).
// Locating does not disturb the propagation: x, t, h and the step counts of the lane are those of the same problem without events.
//
// prop_event_kernel<Ode, Ev>: lane <-> problem, the LDS layout and `lanes` of prop_batch_kernel ([stage][state][lane],
// capi/propagate_plan.h with stm = 0), no further LDS: a location reuses the stage storage of the step it follows, whose result
// x_i+1 waits in registers.  The lane is a small state machine -- ADVANCE, or LOCATE (event, bracket) -- and every trip through the ONE
// stage loop (ONE call site of Ode::f, not unrolled) serves whichever the lane needs: it differs in the step size only (h, or theta h),
// so lanes that locate and lanes that step run the same instructions, and a location costs its own lane trips (at most NE max_iters
// per accepted step) instead of sending the wave through a second copy of the step.  Behind the stage loop there is ONE call site of
// Ev::f (the events at the trip's end point); a second one evaluates g(x0, t0) before the loop.
// Every loop is bounded: max_steps (accepted + rejected integration steps; location trips are not steps), max_iters per location, NE
// locations per step.  No barrier, no cross-lane operation: a lane reads only what it wrote.
//
// Outputs: xf[m][n] (NaN when status != 0), t_end[m] (tf unless the problem stopped), stopped[m] (-1: ran to tf), ev_count[m][NE],
// ev_rows[m][NE][K][n + 1] (state and time of a located occurrence, NaN where unused), ev_resid[m][NE][K] (G there, NaN where unused),
// ev_conv[m][NE][K] (0 where unused), steps[m][2], status[m] (0, 1, 2 as prop_batch_kernel; a stopped problem has 0).  tf == t0: no
// events, t_end = t0.  A problem whose status is not 0 keeps what it located before it failed.
#pragma once
#include <hip/hip_runtime.h>

#include "propagate_kernels.h"

namespace asset_hip {

constexpr int PROP_EVENT_MAX = 8;

struct PropEventArgs {
  long long m;                   // problems
  int lanes;                     // capi/propagate_plan.h (stm = 0)
  int max_iters, max_locs;       // evaluations of G per occurrence; occurrences stored per problem and event (K)
  double event_tol;
  int direction[PROP_EVENT_MAX], stop[PROP_EVENT_MAX];
  const double* y0;              // [m][N] rows [x0, t0, u, p]
  const double* tf;              // [m]
  const double* abs_tols;        // [n]
  const double* rel_tols;        // [n]
  IntegOptions opt;
  double* xf;                    // [m][n]
  double* t_end;                 // [m]
  int* stopped;                  // [m]
  int* ev_count;                 // [m][NE]
  double* ev_rows;               // [m][NE][K][n + 1]
  double* ev_resid;              // [m][NE][K]
  int* ev_conv;                  // [m][NE][K]
  int* steps;                    // [m][2]
  int* status;                   // [m]
};

// v[j] for a run-time j without indexing a register array
template <int NE, class T>
__device__ inline T prop_event_pick(const T* v, int j) {
  T r = v[0];
#pragma unroll
  for (int q = 1; q < NE; q++) r = q == j ? v[q] : r;
  return r;
}

template <class Ode, class Ev>
__global__ __launch_bounds__(64) void prop_event_kernel(PropEventArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, S = RK_STAGES, NE = Ev::XV;
  static_assert(Ev::NIN == N, "an event function reads the ODE's input row");
  static_assert(NE >= 1 && NE <= PROP_EVENT_MAX, "1 .. PROP_EVENT_MAX events");
  double* sk = prop_lds;                             // [stage][state][lane]
  const int L = a.lanes, t = threadIdx.x;
  const long long i = (long long)blockIdx.x * L + t;
  if (t >= L || i >= a.m) return;                    // (no barrier below: a lane only reads what it wrote)
  const double* row = a.y0 + i * N;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int K = a.max_locs;
  const double tol = a.event_tol;
  double x[n], xn[n], xacc[n], u[UV > 0 ? UV : 1];
#pragma unroll
  for (int j = 0; j < UV; j++) u[j] = row[n + 1 + j];
  const double t0 = row[n], tf = a.tf[i];
  bool ok = integ_finite(t0) && integ_finite(tf);
#pragma unroll
  for (int k = 0; k < n; k++) {
    x[k] = row[k];
    xacc[k] = x[k];
    ok = ok && integ_finite(x[k]);
  }
  const IntegOptions o = a.opt;
  const double H = tf - t0;
  int accepted = 0, rejected = 0, status = ok ? INTEG_OK : INTEG_NONFINITE, stopped = -1;
  int cnt[NE];
#pragma unroll
  for (int q = 0; q < NE; q++) cnt[q] = 0;
  double tc = t0;
  if (ok && H != 0.0) {
    double gp[NE], gn[NE];                           // the events at the start and at the end of the accepted step
    {
      IntegIn<Ode> in{x, t0, u, row};
      ValueOut<NE> g0;
      Ev::f(in, g0);
#pragma unroll
      for (int q = 0; q < NE; q++) gp[q] = g0.v[q], gn[q] = g0.v[q];
    }
    const int numsteps = int(fabs(H / o.def_step)) + 1;
    double h = 0.9 * (H / double(numsteps));
    // the lane's state machine: ADVANCE (locating == false) or LOCATE event ej within the bracket [tha, thb] of the accepted step
    bool locating = false, lastacc = false, final_trial = false;
    unsigned pending = 0;                            // events of the accepted step still to be located (bit q)
    int ej = 0, iters = 0, side = 0;
    double tha = 0.0, thb = 1.0, Ga = 0.0, Gb = 0.0, hbr = 0.0, tacc = t0;
    bool go = true;
    while (go) {
      double tnext = tc, hs;
      bool last = false;
      if (!locating) {
        if (accepted + rejected >= o.max_steps) {
          status = INTEG_STEP_LIMIT;
          break;
        }
        // a step that reaches or passes tf ends there
        tnext = tc + h;
        if (H > 0.0 ? (tnext - tf) >= 0.0 : (tnext - tf) <= 0.0) {
          h = tf - tc;
          tnext = tf;
          last = true;
        }
        hs = tnext - tc;
      } else {
        // the next trial point: the midpoint once the bracket is narrow enough (the last trial), else the secant point
        final_trial = 0.5 * (thb - tha) * fabs(hbr) < tol;
        double th = final_trial ? 0.5 * (tha + thb) : (tha * Gb - thb * Ga) / (Gb - Ga);
        if (!(th > tha && th < thb)) th = 0.5 * (tha + thb);
        hs = th * hbr;
        tnext = th;                                  // (carried to the bracket update below)
      }
      // ---- the 13 stages: ONE call site of the right-hand side, for a step and for a trial point alike
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
      // ---- the events at the trip's end point: ONE call site
      const double tev = locating ? tc + hs : tnext;
      ValueOut<NE> gv;
      {
        IntegIn<Ode> in{xn, tev, u, row};
        Ev::f(in, gv);
      }
      bool commit = false, start = false;
      if (!locating) {
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
        // every event is examined for the accepted step
        pending = 0;
#pragma unroll
        for (int q = 0; q < NE; q++) {
          gn[q] = gv.v[q];
          const int dir = a.direction[q], st = a.stop[q];
          const bool occurred = gp[q] * gn[q] < 0.0 && (dir == 0 || (dir > 0 ? gn[q] > 0.0 : gn[q] < 0.0));
          if (occurred) {
            if (cnt[q] < K) pending |= 1u << q;      // (its slot is cnt[q] - 1 after the increment)
            cnt[q]++;
            if (st > 0 && cnt[q] == st && stopped < 0) stopped = q;
          }
        }
#pragma unroll
        for (int k = 0; k < n; k++) xacc[k] = xn[k];
        hbr = hs, tacc = tnext, lastacc = last;
        if (pending) start = true;
        else commit = true;
      } else {
        const double G = prop_event_pick<NE>(gv.v, ej), th = tnext;
        iters++;
        const bool gfin = fin && integ_finite(G);
        const bool conv = gfin && (final_trial || fabs(G) < tol);
        if (conv || iters >= a.max_iters || !gfin) {
          const long long slot = (i * NE + ej) * (long long)K + (prop_event_pick<NE>(cnt, ej) - 1);
          double* er = a.ev_rows + slot * (n + 1);
#pragma unroll
          for (int k = 0; k < n; k++) er[k] = xn[k];
          er[n] = tev;
          a.ev_resid[slot] = G;
          a.ev_conv[slot] = conv ? 1 : 0;
          pending &= ~(1u << ej);
          if (pending) start = true;
          else commit = true;
        } else if ((G < 0.0) == (Gb < 0.0)) {        // the trial point replaces the end point whose sign it has
          thb = th, Gb = G;
          if (side > 0) Ga *= 0.5;
          side = 1;
        } else {
          tha = th, Ga = G;
          if (side < 0) Gb *= 0.5;
          side = -1;
        }
      }
      if (start) {                                   // the lowest pending event, its bracket the whole accepted step
        locating = true;
        ej = __ffs(int(pending)) - 1;
        tha = 0.0, thb = 1.0, Ga = prop_event_pick<NE>(gp, ej), Gb = prop_event_pick<NE>(gn, ej);
        iters = 0, side = 0;
      }
      if (commit) {                                  // the accepted step becomes the lane's state
        locating = false;
#pragma unroll
        for (int k = 0; k < n; k++) x[k] = xacc[k];
#pragma unroll
        for (int q = 0; q < NE; q++) gp[q] = gn[q];
        tc = tacc;
        if (lastacc || stopped >= 0) go = false;
      }
    }
  }
  const bool good = status == INTEG_OK;
  for (int k = 0; k < n; k++) a.xf[i * n + k] = good ? x[k] : qnan;
  a.t_end[i] = stopped >= 0 ? tc : tf;
  a.stopped[i] = stopped;
#pragma unroll
  for (int q = 0; q < NE; q++) {
    a.ev_count[i * NE + q] = cnt[q];
    for (int s = cnt[q] < K ? cnt[q] : K; s < K; s++) {   // slots never used
      const long long slot = (i * NE + q) * (long long)K + s;
      for (int k = 0; k <= n; k++) a.ev_rows[slot * (n + 1) + k] = qnan;
      a.ev_resid[slot] = qnan;
      a.ev_conv[slot] = 0;
    }
  }
  a.steps[i * 2] = accepted;
  a.steps[i * 2 + 1] = rejected;
  a.status[i] = status;
}

}  // namespace asset_hip
