// Batched propagation with events AND the state-transition matrix: propagate until something happens, say where it happened, and
// give the derivative of every state that is returned -- the end state and the state at every stored occurrence -- with respect to
// what went in.
//
// Replaces the STM + Events overloads of the reference (Integrators/Integrator.h:2076-2082, :2125) for an integrator without a
// controller.  It is prop_event_kernel (propagate_event_kernels.h) run by the lane groups of prop_stm_kernel (propagate_kernels.h):
//
// prop_event_stm_kernel<Ode, Ev>: lane <-> (problem, column c of S = d x / d [x0, u, p]), the launch plan of prop_stm_kernel unchanged
// (capi/propagate_plan.h, stm = 1: group, lanes, passes, problems_per_wg, the same LDS bytes; state stages once per group as
// [stage][state][group], column stages per lane as [stage][state][lane]).  Every lane of a group runs the state machine of
// prop_event_kernel -- ADVANCE, or LOCATE (event, bracket) -- on the problem's state itself, statement for statement: the same
// instructions on the same data, hence the same accept / reject decisions, the same detections, the same brackets and the same trial
// points in every lane of the group.  No barrier, no cross-lane operation, every loop bounded as there.  ONE stage loop, not
// unrolled, with ONE call site of Ode::f and ONE of Ode::fj, serves a step and a trial point alike; ONE call site of Ev::f sits
// behind the loop and one before it.
//
// THE COLUMN rides through every trip exactly as in prop_stm_kernel: KC_s = hs J(X_s) w_s through the JvpOut accessor, the Jacobian
// never stored, the state's stages from Ode::f (so the states are those of prop_event_kernel bit for bit).  An accepted step's
// column waits in registers (svacc) beside xacc until the step is committed; a LOCATE trip carries the column through its theta h
// step from the start of the bracketing step, and the trial point's column is what is stored with the occurrence: the discrete
// derivative of the stored state through the accepted steps up to the bracket's start, then the one theta h step with theta held.
//
// Outputs.  Everything prop_event_kernel writes is written here by lane 0 of the group in pass 0 only.  S[m][n][C] at the end of the
// propagation: every lane with c < C.  ev_S[m][NE][K][n][C] (when the pointer is not null): the column at every stored occurrence --
// for one stored with ev_conv = 0 the column of the trial point whose state was stored -- NaN in unused slots.  With passes > 1 the
// state machine runs again in every pass, as the state does in prop_stm_kernel; S and ev_S columns are written per pass.  A problem
// whose status is not 0 has NaN in xf and S and keeps what it located before it failed.  tf == t0: S is the identity in its x columns
// and zero elsewhere, no events.
//
// prop_event_jac_kernel<Ode, Ev>: thread <-> (problem, item); item 0 is the end of the propagation, items 1 .. NE K the stored
// occurrences (only item 0 when ev_jac is null).  Each item gives J[n][N + 1] in the reference's layout [x0 | t0 | u | p | t]: the x0, u,
// p columns from S or ev_S, d / d t0 = -S_x f(x0, t0, u, p), the last column f at the item's own state and its own time -- t_end for
// item 0 (not tf when the problem stopped), ev_rows[..][n] for an occurrence.  NaN where the item is unused or the status is not 0.
#pragma once
#include <hip/hip_runtime.h>

#include "propagate_event_kernels.h"

namespace asset_hip {

struct PropEventStmArgs {
  long long m;                   // problems
  int group, lanes, passes;      // capi/propagate_plan.h (stm = 1)
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
  double* S;                     // [m][n][C]
  double* ev_S;                  // [m][NE][K][n][C] (null: not wanted)
  double* jac;                   // [m][n][N + 1]
  double* ev_jac;                // [m][NE][K][n][N + 1] (null: not wanted)
  int* steps;                    // [m][2]
  int* status;                   // [m]
};

template <class Ode, class Ev>
__global__ __launch_bounds__(64) void prop_event_stm_kernel(PropEventStmArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, S = RK_STAGES, C = N - 1, NE = Ev::XV;
  static_assert(Ev::NIN == N, "an event function reads the ODE's input row");
  static_assert(NE >= 1 && NE <= PROP_EVENT_MAX, "1 .. PROP_EVENT_MAX events");
  const int L = a.lanes, G = a.group, PW = L / G, t = threadIdx.x;
  double* sx = prop_lds;                             // [stage][state][group of the workgroup]
  double* sc = prop_lds + S * n * PW;                // [stage][state][lane]
  const int g = t / G, c0 = t % G;
  const long long i = (long long)blockIdx.x * PW + g;
  if (t >= L || i >= a.m) return;                    // (no barrier below: a group only reads what it wrote)
  const double* row = a.y0 + i * N;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int K = a.max_locs;
  const double tol = a.event_tol;
  double u[UV > 0 ? UV : 1];
#pragma unroll
  for (int j = 0; j < UV; j++) u[j] = row[n + 1 + j];
  const double t0 = row[n], tf = a.tf[i];
  const IntegOptions o = a.opt;
  const double H = tf - t0;
  for (int pass = 0; pass < a.passes; pass++) {
    const int c = pass * G + c0;                     // this lane's column (c >= C: none; the lane carries zeros)
    const bool writer = pass == 0 && c0 == 0;        // the lane that writes what prop_event_kernel writes
    double* evs = (a.ev_S && c < C) ? a.ev_S + i * NE * (long long)K * n * C + c : nullptr;   // this column of slot 0, event 0
    double x[n], xn[n], xacc[n], sv[n], svn[n], svacc[n];
    bool ok = integ_finite(t0) && integ_finite(tf);
#pragma unroll
    for (int k = 0; k < n; k++) {
      x[k] = row[k];
      xacc[k] = x[k];
      sv[k] = k == c ? 1.0 : 0.0;
      svacc[k] = sv[k];
      ok = ok && integ_finite(x[k]);
    }
    int accepted = 0, rejected = 0, status = ok ? INTEG_OK : INTEG_NONFINITE, stopped = -1;
    int cnt[NE];
#pragma unroll
    for (int q = 0; q < NE; q++) cnt[q] = 0;
    double tc = t0;
    if (ok && H != 0.0) {
      double gp[NE], gn[NE];                         // the events at the start and at the end of the accepted step
      {
        IntegIn<Ode> in{x, t0, u, row};
        ValueOut<NE> g0;
        Ev::f(in, g0);
#pragma unroll
        for (int q = 0; q < NE; q++) gp[q] = g0.v[q], gn[q] = g0.v[q];
      }
      const int numsteps = int(fabs(H / o.def_step)) + 1;
      double h = 0.9 * (H / double(numsteps));
      // the group's state machine: ADVANCE (locating == false) or LOCATE event ej within the bracket [tha, thb] of the accepted step
      bool locating = false, lastacc = false, final_trial = false;
      unsigned pending = 0;                          // events of the accepted step still to be located (bit q)
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
          tnext = th;                                // (carried to the bracket update below)
        }
        // ---- the 13 stages: ONE call site of the right-hand side and one of its Jacobian, for a step and for a trial point alike
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
              if (cnt[q] < K) pending |= 1u << q;    // (its slot is cnt[q] - 1 after the increment)
              cnt[q]++;
              if (st > 0 && cnt[q] == st && stopped < 0) stopped = q;
            }
          }
#pragma unroll
          for (int k = 0; k < n; k++) xacc[k] = xn[k], svacc[k] = svn[k];
          hbr = hs, tacc = tnext, lastacc = last;
          if (pending) start = true;
          else commit = true;
        } else {
          const double Gt = prop_event_pick<NE>(gv.v, ej), th = tnext;
          iters++;
          const bool gfin = fin && integ_finite(Gt);
          const bool conv = gfin && (final_trial || fabs(Gt) < tol);
          if (conv || iters >= a.max_iters || !gfin) {
            const long long slot = (i * NE + ej) * (long long)K + (prop_event_pick<NE>(cnt, ej) - 1);
            if (writer) {
              double* er = a.ev_rows + slot * (n + 1);
#pragma unroll
              for (int k = 0; k < n; k++) er[k] = xn[k];
              er[n] = tev;
              a.ev_resid[slot] = Gt;
              a.ev_conv[slot] = conv ? 1 : 0;
            }
            if (evs) {                               // the trial point's column: this lane's entries of the slot's [n][C]
              double* es = evs + (slot - i * NE * (long long)K) * n * C;
#pragma unroll
              for (int k = 0; k < n; k++) es[k * C] = svn[k];
            }
            pending &= ~(1u << ej);
            if (pending) start = true;
            else commit = true;
          } else if ((Gt < 0.0) == (Gb < 0.0)) {     // the trial point replaces the end point whose sign it has
            thb = th, Gb = Gt;
            if (side > 0) Ga *= 0.5;
            side = 1;
          } else {
            tha = th, Ga = Gt;
            if (side < 0) Gb *= 0.5;
            side = -1;
          }
        }
        if (start) {                                 // the lowest pending event, its bracket the whole accepted step
          locating = true;
          ej = __ffs(int(pending)) - 1;
          tha = 0.0, thb = 1.0, Ga = prop_event_pick<NE>(gp, ej), Gb = prop_event_pick<NE>(gn, ej);
          iters = 0, side = 0;
        }
        if (commit) {                                // the accepted step becomes the group's state, its column the lane's
          locating = false;
#pragma unroll
          for (int k = 0; k < n; k++) x[k] = xacc[k], sv[k] = svacc[k];
#pragma unroll
          for (int q = 0; q < NE; q++) gp[q] = gn[q];
          tc = tacc;
          if (lastacc || stopped >= 0) go = false;
        }
      }
    }
    const bool good = status == INTEG_OK;
    if (c < C)
      for (int k = 0; k < n; k++) a.S[(i * n + k) * C + c] = good ? sv[k] : qnan;
    if (evs) {
#pragma unroll
      for (int q = 0; q < NE; q++)
        for (int s = cnt[q] < K ? cnt[q] : K; s < K; s++) {   // slots never used
          double* es = evs + ((long long)q * K + s) * n * C;
          for (int k = 0; k < n; k++) es[k * C] = qnan;
        }
    }
    if (writer) {
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
  }
}

template <class Ode, class Ev>
__global__ __launch_bounds__(64) void prop_event_jac_kernel(PropEventStmArgs a) {
  constexpr int n = Ode::XV, N = Ode::NIN, UV = Ode::UV, C = N - 1, LDJ = N + 1, NE = Ev::XV;
  const int K = a.max_locs;
  const long long items = a.ev_jac ? 1 + (long long)NE * K : 1;
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= a.m * items) return;
  const long long i = id / items, item = id % items;
  const double* row = a.y0 + i * N;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const long long slot = i * NE * (long long)K + (item - 1);          // (items >= 1)
  const double* Sm = item == 0 ? a.S + i * n * C : a.ev_S + slot * n * C;
  double* J = item == 0 ? a.jac + i * n * LDJ : a.ev_jac + slot * n * LDJ;
  const double* xi = item == 0 ? a.xf + i * n : a.ev_rows + slot * (n + 1);
  bool used = a.status[i] == INTEG_OK;
  if (item > 0) {
    const int q = int((item - 1) / K), s = int((item - 1) % K);
    used = used && s < a.ev_count[i * NE + q];
  }
  if (!used) {
    for (int k = 0; k < n * LDJ; k++) J[k] = qnan;
    return;
  }
  const double ti = item == 0 ? a.t_end[i] : xi[n];
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
  for (int k = 0; k < n; k++) x[k] = xi[k];
  {
    IntegIn<Ode> in{x, ti, u, row};
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
