// nesterov_step.h -- the text every device form of the accelerated-RGD iteration shares: the Nesterov scalars and the
// step tail.  The iteration exists as the two-launch sequence (k_precond<PM_RGD> + k_eval_stats, precond.hip), the
// one-launch form (k_step_fe, step_fused.hip) and the deep-carried form (k_step_fd, step_deep.hip), and their iterates are
// bitwise equal.  For what stands here that holds by construction: one expression each for the recurrence, the scalars of
// the iterations ahead, the books, the look-ahead map and the lane-parallel step of a workgroup's two poses.  (k_precond's
// serial tail and its in-place look-ahead keep their own control flow: they store in place, not into a twin copy, and take
// only the scalars and the map from here.  So do the look-ahead waves of the two one-launch kernels for the poses of the
// other agents: one function for both was built and measured, and k_step_fd lost 0.14 us per launch to it,
// profiles/r19_nesterov_step.md.)
//
// The library is built with -ffp-contract=on, which fuses within one source expression: every expression below is the
// kernels' own, moved whole.
//
// The scalar part compiles for the host too (tests/test_nesterov_host.py): it needs nothing but NestState (dpgo_dev.h; a
// host program declares dpgo::NestState { double gamma, alpha; int iter, pad; } itself before it includes this file).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include "device_math.h"
#include "dpgo_dev.h"
#endif

#ifndef DPGO_HD
#if defined(__HIPCC__)
#define DPGO_HD __host__ __device__ __forceinline__
#else
#define DPGO_HD inline
#endif
#endif

namespace dpgo {

// ------------------------------------------------------------------------------------------------ scalars
// the recurrence: gamma of an iteration from gamma of the one before (Nr: the number of robots)
DPGO_HD double nest_gamma_step(double gamma, double Nr) { return (1.0 + sqrt(1.0 + 4.0 * Nr * Nr * gamma * gamma)) / (2.0 * Nr); }

// does the iteration `ahead` steps behind the one the state describes restart?  A NestState describes iteration k - 1 and
// its iter is pre-increment: iteration k restarts when (iter + 2) % interval == 0.
DPGO_HD bool nest_restart(const NestState &ns, int ahead, int restart_interval) { return ((ns.iter + 2 + ahead) % restart_interval) == 0; }

// the books of one accelerated iteration: gamma and alpha of the next state (iter is the caller's: advance_agent adds its
// own increment)
DPGO_HD void nest_books(NestState &ns, double Nr, int restart_interval) {
  const bool restart = nest_restart(ns, 0, restart_interval);
  if (restart) { ns.gamma = 0; ns.alpha = 0; }
  else {
    ns.gamma = nest_gamma_step(ns.gamma, Nr);
    ns.alpha = 1.0 / (ns.gamma * Nr);
  }
}

// Nesterov scalars of the iterations a launch looks at, from the state BEFORE iteration k: gamma of iteration k, and the
// restart tests and look-ahead alphas of the iterations behind it.  Every wave that needs them derives them from the same
// NestState; a caller that looks fewer steps ahead leaves fields unread.
struct NestAhead {
  bool restart_now, restart_next, restart_next2, restart_next3;
  double nest_gamma, ahead_alpha, ahead2_alpha, ahead3_alpha;
};

DPGO_HD NestAhead nest_ahead(const NestState &ns, int num_robots, int restart_interval) {
  NestAhead o;
  const double Nr = (double)num_robots;
  o.restart_now = nest_restart(ns, 0, restart_interval);
  o.restart_next = nest_restart(ns, 1, restart_interval);
  o.restart_next2 = nest_restart(ns, 2, restart_interval);
  o.restart_next3 = nest_restart(ns, 3, restart_interval);
  o.nest_gamma = o.restart_now ? 0.0 : nest_gamma_step(ns.gamma, Nr);
  const double g2 = nest_gamma_step(o.nest_gamma, Nr);
  o.ahead_alpha = 1.0 / (g2 * Nr);
  const double gamma_next = o.restart_next ? 0.0 : g2;
  const double g3 = nest_gamma_step(gamma_next, Nr);
  o.ahead2_alpha = 1.0 / (g3 * Nr);
  const double gamma_next2 = o.restart_next2 ? 0.0 : g3;
  const double g4 = nest_gamma_step(gamma_next2, Nr);
  o.ahead3_alpha = 1.0 / (g4 * Nr);
  return o;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------ device text
// the look-ahead map of one pose on one lane: y = polar((1 - alpha) x + alpha v)
template <int R>
__device__ __forceinline__ void lookahead_map(const double *x, const double *v, double alpha, double *y) {
#pragma unroll
  for (int i = 0; i < 4 * R; ++i) y[i] = (1.0 - alpha) * x[i] + alpha * v[i];
  polar_inplace<R>(y);
}

// the books of a one-launch iteration (advance_agent, accelerated), lane k for agent k: the next state into the OTHER state
// buffer -- every workgroup of the launch reads nest_src --, then lane 0 publishes the iteration
__device__ __forceinline__ void step_books(TeamDev *team, const NestState *nest_src, NestState *nest_dst, int k, int num_agents,
                                           int sel, int next_sel, int num_robots, int restart_interval) {
  const double Nr = (double)num_robots;
  if (k < num_agents) {
    NestState s2 = nest_src[k];
    nest_books(s2, Nr, restart_interval);
    s2.iter += 1;
    nest_dst[k] = s2;
  }
  if (k == 0) {
    team->iter += 1;
    team->stats_sel = sel;
    team->next_sel = next_sel;
    team->cur_sel = next_sel;
  }
}

// LDS of step_two_poses, declared by the kernel: the reduced product zs, the operands x0 / v0 / y0 / p0 (X, V, Y, XPrev of
// the two poses, [pose][4r]; p0 and tl_rel only where a step leaves statistics), the work rows tl_x / tl_v / tl_y and the
// 16 Gram sums per pose tl_s
struct TwoPoseLds {
  double *zs;
  const double *x0, *v0, *y0, *p0;
  double *tl_x, *tl_v, *tl_y, *tl_s, *tl_rel;
};

// The step of a workgroup's two poses on one wave: one pose on 16 lanes, the pose in LDS (device_math.h, lane-parallel
// forms: bitwise the serial routines) -- the six Gram sums of a QF / polar factor side by side, the entries of a product on
// 3R lanes: tangent projection of the product, step, QF retraction, Nesterov V (or the restart's V = X), the look-ahead
// point of iteration k+1 (or the restart's carry-over), the stores into the other copy of the poses (Xw / Yw) and V.
// What the step leaves behind: `in` -- it stores at all (a launch that only opens a run computes on nothing); `stats` --
// what k_precond's PA_STATS leaves: the snapshot B_X2 the closing statistics evaluate and |X - XPrev|^2 per pose in
// tl_rel (one lane, the serial loop's order; the caller sums the two); `lastat` -- what PA_LA_STATUS leaves: XPrev, and
// |Y' - X|^2 per pose in PART_D.  stamp(7 | 8 | 9): the kernel's trace stamps behind the retraction, V and the look-ahead.
template <int R, class Stamp>
__device__ __forceinline__ void step_two_poses(const AgentDev &ag, double *__restrict__ Xw, double *__restrict__ Yw, const TwoPoseLds &L,
                                               int ln, int npose, int pj0, int pj1, double step, const NestAhead &nn,
                                               bool ahead_opt, bool in, bool stats, bool lastat, Stamp stamp) {
  const bool restart_now = nn.restart_now, restart_next = nn.restart_next;
  const double nest_gamma = nn.nest_gamma, ahead_alpha = nn.ahead_alpha;
  const int lp = ln >> 4, s = ln & 15;
  if (lp < npose) {
    const size_t o = (size_t)(lp ? pj1 : pj0) * 4 * R;
    double *xs = L.tl_x + lp * 4 * R, *vsv = L.tl_v + lp * 4 * R, *ys = L.tl_y + lp * 4 * R, *Ss = L.tl_s + lp * 16;
    double *zz = L.zs + lp * 4 * R;
    const double *x0 = L.x0 + lp * 4 * R, *v0 = L.v0 + lp * 4 * R, *y0 = L.y0 + lp * 4 * R;
    const int i0 = s, i1 = s + 16;  // the (at most two) entries of the pose this lane moves
    const bool h0 = i0 < 4 * R, h1 = i1 < 4 * R;
    tangent_lanes<R>(x0, zz, Ss, s);
    if (h0) xs[i0] = x0[i0] - step * zz[i0];
    if (h1) xs[i1] = x0[i1] - step * zz[i1];
    lanes_sync();
    qf_lanes<R>(xs, Ss, s);
    stamp(7);
    if (stats) {
      if (h0) gp(ag.buf[B_X2])[o + i0] = xs[i0];
      if (h1) gp(ag.buf[B_X2])[o + i1] = xs[i1];
      if (s == 0) {
        const double *p0 = L.p0 + lp * 4 * R;
        double rel = 0;
#pragma unroll
        for (int i = 0; i < 4 * R; ++i) { const double d = xs[i] - p0[i]; rel += d * d; }
        L.tl_rel[lp] = rel;
      }
    }
    if (lastat) {
      if (h0) gp(ag.buf[B_XPREV])[o + i0] = xs[i0];
      if (h1) gp(ag.buf[B_XPREV])[o + i1] = xs[i1];
    }
    const bool reset = restart_now;  // restart iteration: V = Y = X
    if (reset) {
      if (h0) vsv[i0] = xs[i0];
      if (h1) vsv[i1] = xs[i1];
      lanes_sync();
    } else {
      const double gamma = nest_gamma;
      if (h0) vsv[i0] = v0[i0] + gamma * (xs[i0] - y0[i0]);
      if (h1) vsv[i1] = v0[i1] + gamma * (xs[i1] - y0[i1]);
      lanes_sync();
      polar_lanes<R>(vsv, Ss, s);
    }
    stamp(8);
    if (restart_next) {
      if (h0 && in) {
        Xw[o + i0] = xs[i0];
        if (!ahead_opt) { Yw[o + i0] = xs[i0]; vsv[i0] = xs[i0]; }
        else Yw[o + i0] = reset ? xs[i0] : y0[i0];  // (else Y stays: carried into the other copy)
      }
      if (h1 && in) {
        Xw[o + i1] = xs[i1];
        if (!ahead_opt) { Yw[o + i1] = xs[i1]; vsv[i1] = xs[i1]; }
        else Yw[o + i1] = reset ? xs[i1] : y0[i1];
      }
      if (lastat && !ahead_opt && s == 0) gp(ag.part)[PART_D + (lp ? pj1 : pj0)] = 0.0;
    } else {
      if (h0) ys[i0] = (1.0 - ahead_alpha) * xs[i0] + ahead_alpha * vsv[i0];
      if (h1) ys[i1] = (1.0 - ahead_alpha) * xs[i1] + ahead_alpha * vsv[i1];
      lanes_sync();
      polar_lanes<R>(ys, Ss, s);
      stamp(9);
      if (h0 && in) { Yw[o + i0] = ys[i0]; Xw[o + i0] = ys[i0]; }
      if (h1 && in) { Yw[o + i1] = ys[i1]; Xw[o + i1] = ys[i1]; }
      if (lastat && !ahead_opt && s == 0) {  // look-ahead steps leave |Y' - X|^2 per pose
        double rel2 = 0;
#pragma unroll
        for (int i = 0; i < 4 * R; ++i) { const double d = ys[i] - xs[i]; rel2 += d * d; }
        gp(ag.part)[PART_D + (lp ? pj1 : pj0)] = rel2;
      }
    }
    lanes_sync();
    if (h0 && in) ag.buf[B_V][o + i0] = vsv[i0];
    if (h1 && in) ag.buf[B_V][o + i1] = vsv[i1];
  }
}

#endif  // __HIPCC__

}  // namespace dpgo
