// team_run.hip -- the drivers of the team schedule (host code only): which launches make up a run of RBCD iterations.
//   dpgo_team_step_begin / _end      one iteration, split around a neighbour exchange that the caller carries
//   dpgo_team_run / _prepare         runs of the device-resident schedule: one captured graph per window, replayed
//   dpgo_team_run_group / _colored   colour-parallel sweeps
//   dpgo_team_run_simultaneous       lockstep ticks of every local agent
//   dpgo_team_run_peer               the schedule across processes, the UPDATE token on the device
// The launches of ONE iteration and its host-side books are solve.hip's (enqueue_team_iteration, account_iteration); the
// one-launch forms of the pipelined iteration are step_fused.hip and step_deep.hip.
#include "team_internal.h"

using namespace dpgo;
using namespace dpgo_host;

namespace dpgo_host {

void drop_graphs(dpgo_team *t) {
  for (auto &kv : t->graphs) if (kv.second) (void)hipGraphExecDestroy(kv.second);
  t->graphs.clear();
  t->graph_flip.clear();
}

// An in-kernel exchange that timed out (codes: 2 hand-off of the one-launch RTR solve, 3 two-level preconditioner, 4 mailbox
// of the device-side UPDATE token) leaves its code in a pinned word.  Every entry point that has just drained the team's
// stream looks at it, so a time-out is an error at the next host read-back whichever call that is (advisor, round 3: only
// dpgo_team_synchronize did, and the run_peer path never called it).
int check_exchange_error(dpgo_team *t) {
  if (!t->h_bar_err || !*t->h_bar_err) return 0;
  const int code = *t->h_bar_err;
  *t->h_bar_err = 0;
  drop_graphs(t);
  set_err("an in-kernel exchange timed out (code " + std::to_string(code) + ": 2 hand-off of the one-launch RTR solve, 3 two-level "
          "preconditioner, 4 mailbox of the device-side UPDATE token): the iterates since the last successful synchronisation are invalid");
  return DPGO_ERR;
}

// captured runs bake the schedule and the descriptors into their launches: whatever moved those cleared graph_valid
static void revalidate_graphs(dpgo_team *t) { if (!t->graph_valid) { drop_graphs(t); t->graph_valid = true; } }

// the executable graph kept under `key`; if there is none yet, what `body` enqueues on the team's stream is captured,
// instantiated and kept (upload: the first replay then costs what the later ones do)
static int graph_for_key(dpgo_team *t, int key, bool upload, const std::function<int()> &body, hipGraphExec_t *out) {
  auto it = t->graphs.find(key);
  if (it != t->graphs.end()) { *out = it->second; return 0; }
  hipGraph_t g = nullptr;
  HIPC(hipStreamBeginCapture(t->stream, hipStreamCaptureModeThreadLocal));
  const int rc = body();
  HIPC(hipStreamEndCapture(t->stream, &g));
  if (rc) { (void)hipGraphDestroy(g); return rc; }
  hipGraphExec_t ge = nullptr;
  HIPC(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  (void)hipGraphDestroy(g);
  if (upload) (void)hipGraphUpload(ge, t->stream);
  *out = t->graphs[key] = ge;
  return 0;
}

static int agent_at(const dpgo_team *t, int iter) { return t->sched[(size_t)iter % t->sched.size()]; }

// Carried rows of the one-launch iterations (step_fused.hip): launch `rep` of a run of nfe one-launch iterations that starts
// at iteration iter0 finds the row products of its agent formed by launch rep - 1, from the evaluation point launch rep - 2
// left -- which takes the agents of the three iterations to be three different ones (the point is formed while the agent
// rests) and both earlier launches to be part of the same run.  The first two launches of a run form their row products
// themselves.
int fe_carry_flags(dpgo_team *t, int rep, int nfe, int iter0) {
  if (!t->use_fe_carry) return 0;
  auto consumes = [&](int q) {
    if (q < 2 || q >= nfe) return false;
    const int a = agent_at(t, iter0 + q - 2), b = agent_at(t, iter0 + q - 1), c = agent_at(t, iter0 + q);
    if (a == b || a == c || b == c) return false;
    // (the poses of agent c are spread over the workgroups of the launch of agent b)
    const int nblk = precond_nblk(*t->ag[b]);
    if ((t->ag[c]->n + nblk - 1) / nblk > step_fe_carry_max_poses()) return false;
    // (a gradient wave of the launch of agent c finishes 64 public poses and fetches their shared edges, two per lane)
    if (t->ag[c]->npub < 1 || t->ag[c]->npub > 256 || !t->ag[c]->dev.fe_code_ok) return false;  // (no public pose: no table to read)
    for (int g = 0; g < 4; ++g)
      if (t->ag[c]->dev.fe_eptr[g + 1] - t->ag[c]->dev.fe_eptr[g] > 128) return false;
    return true;
  };
  return (consumes(rep) ? FE_CARRY_IN : 0) | (consumes(rep + 1) ? FE_CARRY_W : 0) | (consumes(rep + 2) ? FE_CARRY_Y : 0);
}

// every one-launch iteration of a long run finds carried rows (every three consecutive agents of the schedule differ)
static bool fe_carry_everywhere(dpgo_team *t) {
  const int P = (int)t->sched.size();
  if (P < 3) return false;
  for (int q = 2; q < P + 2; ++q)
    if (!(fe_carry_flags(t, q, 1 << 30, 0) & FE_CARRY_IN)) return false;
  return true;
}

// the one-launch iteration (step_fused.hip) may serve this team: dense agents of fe_min_n (449: where it is faster) .. 512 poses whose rows fit the ELL
// part, few enough public poses / shared edges for its LDS tables, the schedule and the descriptors baked into the
// launches (period <= 8), every neighbour co-resident (the twins of its poses are addressed through the shared-edge table)
bool fused_eval_eligible(dpgo_team *t) {
  const dpgo_params_t &p = t->prm;
  const int P = (int)t->sched.size();
  if (!(t->use_fused_eval && t->bake_sel && t->bake_desc && P >= 1 && P <= 8 && step_fe_supported(p.r) && p.acceleration &&
        p.method == DPGO_METHOD_RGD && p.rgd_use_preconditioner && (int)t->ag.size() <= LOOKAHEAD_MAX_AGENTS &&
        t->h_descs.size() == t->ag.size() && t->precond_of.size() == t->ag.size() && t->peers.empty() && !t->isolated &&
        (int)t->ag.size() == p.num_robots))
    return false;
  // (with carried rows the one-launch form is the faster one at every size it was measured at, 41 .. 500 poses; without them
  // only from about 450 poses up -- profiles/experiments/fe_small.py)
  const int min_n = t->fe_min_n > 0 ? t->fe_min_n : (fe_carry_everywhere(t) ? 32 : 449);
  for (size_t k = 0; k < t->ag.size(); ++k) {
    const int n = t->ag[k]->n;
    if (t->precond_of[k] != DPGO_PRECOND_DENSE || n < min_n || n > 512 || !t->ag[k]->has_soa ||
        t->h_descs[k].nshared > step_fe_max_edges())
      return false;
  }
  return true;
}

// The deep-carried form (step_deep.hip) may serve this team: the private part of every agent's product is formed one launch
// early, its row products two, its evaluation point three -- so every FOUR consecutive agents of the schedule differ; the
// first 24 chunks of every agent's order are private (24 is returned; 0: not this team); an agent's
// public poses fit two waves, its shared edges three edge slots of 64, the head of a launch can stand for its descriptor
// (step_head.h: fields within their widths, work vectors one allocation), and the partial sums have their buffers.
// (The same run as ONE persistent launch was built, measured slower and removed: profiles/r06_deep_carry.md.)
int fe_deep_m0(dpgo_team *t) {
  if (!t->use_fe_deep || !t->use_fe_carry || !fused_eval_eligible(t)) return 0;
  const int P = (int)t->sched.size();
  if (P < 4) return 0;
  for (int q = 0; q < P; ++q)
    for (int u = 1; u < 4; ++u)
      if (t->sched[(size_t)q] == t->sched[(size_t)((q + u) % P)]) return 0;
  int min_priv = 32, nblk_all = 0, total = 0;
  for (auto &a : t->ag) {
    if (a->npub < 1 || a->npub > 128 || !a->dev.fe_code_ok || (int)a->se_host.size() > FE_MAX_EDGES) return 0;
    // (the launches resolve their edges and public poses from the front table, step_front.h: it must be the one built from
    // the descriptors as they were last published)
    if (t->desc_gen == 0 || a->front_gen != t->desc_gen) return 0;
    min_priv = std::min(min_priv, a->dev.fe_npriv);
    nblk_all = std::max(nblk_all, (4 * a->n + 7) / 8);
    total += a->n;
  }
  for (auto &a : t->ag)
    if ((total - a->n + nblk_all - 1) / nblk_all > 64) return 0;
  int m0 = step_fd_pick_m0(min_priv);
  if (const char *e = std::getenv("DPGO_FD_M0")) { const int f = std::atoi(e); if (f > 0 && f <= min_priv && step_fd_pick_m0(f) == f) m0 = f; }  // (experiments)
  if (m0 == 0) return 0;
  for (auto &a : t->ag)
    if (!step_fd_head_ok(a->dev, t->prm.r, m0)) return 0;
  const size_t want = (size_t)2 * nblk_all * t->prm.r * 256;
  if (t->d_fd_pacc.n < want && t->d_fd_pacc.alloc(want)) return 0;
  return m0;
}

// ---- dpgo_team_run.  The schedule, the counters and the Nesterov scalars live on the device, so a window of iterations is
// one fixed launch sequence: captured once and replayed.  What a call runs is decided once ...
struct RunPlan {
  bool graphable;  // preconditioned RGD: windows are captured (anything else: run_eager_iteration)
  bool ls;         // RGD line search: the step is decided once the whole agent's trial costs are known -- its iterations are
                   // the un-fused launch sequence of enqueue_team_iteration, captured as it is
  bool pipelined;  // accelerated, and the look-ahead Nesterov steps fit (a workgroup's share of the other agents' poses in one
                   // wave, one double per pose in PART_D): two launches per iteration, restarts part of the uniform sequence
  bool bake;       // short schedule period: one graph per phase of the schedule, the agent of every iteration baked into its
                   // launches (its descriptor comes from a kernel argument: one dependent round trip less in each prologue)
  bool fe_ok;      // one-launch iterations (step_fused.hip) may serve the mid-run part of a pipelined window
  int fd_m0, P;    // > 0: ... in the deep-carried form (step_deep.hip); the schedule period
};

static RunPlan make_plan(dpgo_team *t) {
  const dpgo_params_t &p = t->prm;
  RunPlan pl{};
  pl.graphable = p.method == DPGO_METHOD_RGD && p.rgd_use_preconditioner;
  pl.ls = p.rgd_line_search != 0;
  pl.pipelined = p.acceleration != 0 && (int)t->ag.size() <= LOOKAHEAD_MAX_AGENTS && !pl.ls;
  int total = 0;
  for (auto &a : t->ag) total += a->n;
  for (auto &a : t->ag) {
    const int nblk = precond_nblk(*a);
    if ((total - a->n + nblk - 1) / nblk > 64 || a->n > MAX_PART * PART_STRIDE) pl.pipelined = false;
  }
  pl.P = (int)t->sched.size();
  pl.bake = t->bake_sel && pl.P >= 1 && pl.P <= 8;
  pl.fe_ok = pl.pipelined && pl.graphable && fused_eval_eligible(t);
  pl.fd_m0 = pl.fe_ok ? fe_deep_m0(t) : 0;
  return pl;
}

// ... and so is every window = one graph: [lead: a restart iteration, un-fused kernels] + B iterations in the plan's form from
// iteration iter0.  Pipelined teams have no lead (restart iterations are ordinary iterations of their sequence).
struct RunWindow {
  bool lead;
  int B, iter0;
  bool fe;    // with one-launch iterations
  int L;      // the last L = min(B, period) steps leave their statistics (X2 snapshot, |X - XPrev|^2: every agent's last block
              // update of the run is among them, and a status query reads it, a9), the look-aheads in front of them XPrev
              // and |Y' - X|^2; nothing reads these values earlier in the run
  int nfe;    // iterations [0, nfe) are one launch each; even: the launches alternate between the two copies of the poses.
              // Round 5's form leaves the last L + 1 to the two-launch sequence; the deep-carried form (deep) leaves their
  bool deep;  // statistics itself (FD_STATS / FD_LASTAT) and hands over only the last iteration, which does not look ahead
};

static RunWindow make_window(const RunPlan &pl, bool lead, int B, int iter0) {
  RunWindow w{};
  w.lead = lead; w.B = B; w.iter0 = iter0;
  w.fe = pl.fe_ok && (pl.fd_m0 > 0 ? B >= 6 : B > pl.P + 2);
  w.L = std::min(B, pl.P);
  w.deep = w.fe && pl.fd_m0 > 0 && ((B - 1) & ~1) >= 4;
  w.nfe = !w.fe ? 0 : (w.deep ? (B - 1) & ~1 : std::max(0, B - w.L - 1) & ~1);
  return w;
}

// one run of nfe deep-carried one-launch iterations from the state k_nest_pre leaves: the points of the first three agents,
// two launches that only produce (the row products of sel(0); then its private partial sums and the row products of
// sel(1)), then the iterations -- each consuming what the three launches before it left
static void enqueue_fe_deep(dpgo_team *t, const LaunchCtx &c, int m0, const RunWindow &w, NestState *nest_own, NestState *const nest_fe[2]) {
  const dpgo_params_t &p = t->prm;
  const int nfe = w.nfe, B = w.B, L = w.L;
  auto sel_at = [&](int rep) { return agent_at(t, w.iter0 + rep); };
  int nblk_all = 0;
  for (auto &a : t->ag) nblk_all = std::max(nblk_all, (4 * a->n + 7) / 8);
  double *pacc[2] = {t->d_fd_pacc.p, t->d_fd_pacc.p + (size_t)nblk_all * p.r * 256};
  const int s0 = sel_at(0), s1 = sel_at(1), s2 = sel_at(2);
  launch_fd_prime(c, s0, s1, s2, t->max_n, p.num_robots, p.restart_interval, nest_own);
  launch_fd_open(c, m0, s0, s1, pacc[0]);
  for (int rep = 0; rep < nfe; ++rep) {
    const int flags = FD_IN | (rep + 1 < nfe ? FD_P : 0) | (rep + 2 < nfe ? FD_W : 0) | (rep + 3 < nfe ? FD_Y : 0) |
                      (rep >= B - L ? FD_STATS : 0) | ((rep + 1 < B && rep + 1 >= B - L) ? FD_LASTAT : 0);
    launch_step_fd(c, m0, sel_at(rep), sel_at(rep + 1), sel_at(rep + 2), sel_at(rep + 3), p.rgd_stepsize, p.num_robots,
                   p.restart_interval, rep == 0 ? nest_own : nest_fe[rep & 1], nest_fe[(rep + 1) & 1], rep & 1, flags,
                   pacc[rep & 1], pacc[(rep + 1) & 1]);
  }
}

// the launches of one window (what its graph captures)
static int enqueue_window(dpgo_team *t, const RunPlan &pl, const RunWindow &w) {
  const dpgo_params_t &p = t->prm;
  const int B = w.B, na = (int)t->ag.size(), mn = t->max_n;
  auto sel_at = [&](int rep) { return pl.bake ? agent_at(t, w.iter0 + rep) : SEL_SCHED; };
  if (w.lead) {
    const int rc = enqueue_team_iteration(t, true, true, SEL_SCHED, PHASE_WHOLE);
    if (rc) return rc;
  }
  if (B > 0 && p.acceleration && pl.pipelined) {
    // pipelined: 2 launches per iteration (see k_eval_stats), restart iterations included.  The Nesterov step of
    // the first iteration is a launch of its own, the last iteration does not look ahead, and its statistics /
    // bookkeeping close the run.
    LaunchCtx c = t->ctx();
    c.bake_desc = pl.bake && t->bake_desc;  // the agent's descriptor by value in the launches that name their agent
    launch_nest_pre(c, SEL_SCHED, -1, na, mn, p.num_robots, p.restart_interval, 1);
    const int L = w.L, nfe = w.nfe;
    NestState *nest_own = t->d_nest_all.p, *nest_fe[2] = {t->d_nest_all.p + na, t->d_nest_all.p + 2 * na};
    if (w.deep) enqueue_fe_deep(t, c, pl.fd_m0, w, nest_own, nest_fe);
    for (int rep = w.deep ? nfe : 0; rep < B; ++rep) {
      if (rep < nfe) {
        // (the one-launch iterations are the ones that leave nothing behind)
        launch_step_fe(c, sel_at(rep), sel_at(rep + 1), p.rgd_stepsize, p.num_robots, p.restart_interval,
                       rep == 0 ? nest_own : nest_fe[rep & 1], nest_fe[(rep + 1) & 1], rep & 1, sel_at(rep + 2),
                       fe_carry_flags(t, rep, nfe, w.iter0));
        continue;
      }
      const int ahead = (rep + 1 < B ? PA_LOOKAHEAD : 0) | ((rep + 1 < B && rep + 1 >= B - L) ? PA_LA_STATUS : 0) | (rep >= B - L ? PA_STATS : 0);
      launch_eval_stats(c, mn, rep == 0, 1, 0, p.num_robots, p.restart_interval, sel_at(rep), SEL_SCHED,
                        (rep == nfe && nfe > 0) ? nest_fe[nfe & 1] : nullptr);
      launch_precond(c, sel_at(rep), mn, PM_RGD_, B_X, B_GF, B_Z, 0, 0, p.rgd_stepsize, 1, p.num_robots, PADV_PIPELINED,
                     p.restart_interval, ahead);
    }
    launch_eval_stats(c, mn, 0, 0, 1, p.num_robots, p.restart_interval, SEL_SCHED, sel_at(B - 1));
  } else if (B > 0 && p.acceleration && !pl.ls) {
    // 3 launches per iteration: [statistics of iteration k-1 + Nesterov step of iteration k] in one
    // heterogeneous kernel, cost/gradient (+ G from the neighbours' Y), preconditioner + RGD step +
    // Nesterov V + bookkeeping
    LaunchCtx c = t->ctx();
    for (int rep = 0; rep < B; ++rep) {
      if (rep == 0) launch_nest_pre(c, SEL_SCHED, -1, na, mn, p.num_robots, p.restart_interval);
      else launch_stats_nest(c, na, mn, p.num_robots, p.restart_interval);
      launch_eval(c, SEL_SCHED, mn, B_X, B_EGRAD, B_GF, PART_C, eval_opts(t, 2, 1, 0));
      launch_precond(c, SEL_SCHED, mn, PM_RGD_, B_X, B_GF, B_Z, 0, 0, p.rgd_stepsize, 1, p.num_robots, PADV_TEAM, p.restart_interval);
    }
    launch_eval(c, SEL_STATS, mn, B_X2, B_EGRAD2, B_GF2, PART_A, eval_opts(t, 0, 0, 0));
  } else {
    for (int rep = 0; rep < B; ++rep) {
      const int rc = enqueue_team_iteration(t, true, false, SEL_SCHED, PHASE_WHOLE, rep + 1 < B);
      if (rc) return rc;
    }
  }
  return 0;
}

// One graph per window shape and -- where the schedule is baked in -- phase of the schedule.  Two instances per key
// alternate, so that a launch never has to wait for the previous replay of the same executable graph.
static int window_graph(dpgo_team *t, const RunPlan &pl, const RunWindow &w, hipGraphExec_t *out) {
  const int phase = pl.bake ? w.iter0 % pl.P : -1;
  const int base = ((((w.lead ? 1 : 0) + 2 * w.B) * 16 + phase + 1) * 2 + (w.fe ? 1 : 0)) * 2;
  const int key = base + (t->graph_flip[base / 2] ^= 1);
  return graph_for_key(t, key, true, [&] { return enqueue_window(t, pl, w); }, out);
}

// the host-side books of a window that has been launched (the team still stands at w.iter0)
static void account_window(dpgo_team *t, const RunPlan &pl, const RunWindow &w) {
  const dpgo_params_t &p = t->prm;
  const int lead = w.lead ? 1 : 0, batch = w.B + lead;
  t->counters[CNT_ONE_LAUNCH] += w.nfe;
  if (w.deep) { t->counters[CNT_CARRIED] += w.nfe; t->counters[CNT_DEEP] += w.nfe; }  // deep-carried: every one of them finds carried rows
  else for (int q = 0; q < w.nfe; ++q) t->counters[CNT_CARRIED] += (fe_carry_flags(t, q, w.nfe, w.iter0) & FE_CARRY_IN) ? 1 : 0;
  // after >= 2 pipelined iterations every agent took its last Nesterov step as a look-ahead (per-pose partials)
  for (auto &a : t->ag) a->rel_src = p.acceleration ? ((pl.pipelined && w.B >= 2) ? REL_POSE_D : REL_TILES_D) : REL_NONE;
  for (int q = 0; q < batch; ++q) {
    const bool is_lead = w.lead && q == 0;
    Agent &a = *t->ag[agent_at(t, w.iter0 + q)];
    // sparse evaluations of the iteration: the gradient and the closing statistics of the two-launch form, the gradient
    // alone in a one-launch iteration (it leaves no statistics); a line-search iteration adds its trial passes
    const int evals = pl.ls ? 2 + (ls_trials(p) + 3) / 4 : ((!is_lead && q - lead < w.nfe) ? 1 : 2);
    count_work(t, a, 1, evals);
    if (is_lead) count_work(t, a, 1, evals);  // the restart iteration solves twice (from Y, then from XPrev)
    // status of this block update: the fused step leaves PART_B[2], the un-fused sequence (restart iteration, line search) tiles
    mark_optimized(t, a, (is_lead || pl.ls) ? REL_TILES_E : REL_FUSED_B, true);
    if (q == batch - 1) {
      a.opt_pending_rgd = true;
      a.rel_src = (w.B > 0 && !pl.ls) ? REL_FUSED_B : REL_TILES_D;  // a lone restart iteration ends with k_status (PART_D tiles)
    }
  }
}

// one iteration of a team whose iterations are not captured (RTR; RGD without the preconditioner), enqueued as it is
static int run_eager_iteration(dpgo_team *t) {
  const int sel = agent_at(t, t->iter);
  for (auto &a : t->ag) a->rel_src = t->prm.acceleration ? REL_TILES_D : REL_NONE;
  const int rc = enqueue_team_iteration(t, false, restart_due(t), sel, PHASE_WHOLE);
  if (rc) return rc;
  // status of the block update: k_status tiles, or -- where the one-launch RTR solve took the iteration's tail --
  // one partial per pose pair in PART_B[2], the fused RGD step's layout
  t->ag[sel]->rel_src = t->last_update_src == REL_FUSED_B ? REL_FUSED_B : REL_TILES_D;
  mark_optimized(t, *t->ag[sel], t->last_update_src, true);
  count_iterations(t, 1, 1);
  return 0;
}

// prepare_only: capture and instantiate every graph a run of `iters` iterations from the current state would replay
// (both alternating instances of each), execute nothing
static int team_run_impl(dpgo_team *t, int iters, bool prepare_only) {
  if (sync_descs(t)) return DPGO_ERR;
  const dpgo_params_t &p = t->prm;
  for (auto &a : t->ag) if (!a->has_X) { set_err("team_run before set_initial"); return DPGO_NOT_READY; }
  const RunPlan pl = make_plan(t);
  if (!pl.graphable) {
    for (int k = 0; k < iters && !prepare_only; ++k) {
      const int rc = run_eager_iteration(t);
      if (rc) return rc;
    }
    return 0;
  }
  revalidate_graphs(t);
  const bool uniform = p.acceleration && pl.pipelined;  // restart iterations are ordinary iterations of the sequence
  int cur_iter = t->iter;
  for (int k = 0; k < iters;) {
    const bool restart = !uniform && p.acceleration && ((cur_iter + 2) % p.restart_interval) == 0;
    // one graph per window: [the restart iteration, if the window opens with one] + the fused iterations up to
    // the next restart iteration
    int fusedn = iters - k - (restart ? 1 : 0);
    if (p.acceleration && !uniform) {
      const int it0 = cur_iter + (restart ? 1 : 0);
      const int to_restart = (p.restart_interval - ((it0 + 2) % p.restart_interval)) % p.restart_interval;
      fusedn = std::min(fusedn, to_restart);
    }
    // (the uniform pipelined sequence pays two extra launches per graph -- the first Nesterov step, the closing
    // statistics -- and six two-launch iterations at its end: longer graphs)
    fusedn = std::max(0, std::min(fusedn, uniform ? dpgo_team::MAX_PIPELINED_GRAPH_ITERS : dpgo_team::MAX_GRAPH_ITERS));
    const RunWindow w = make_window(pl, restart, fusedn, cur_iter);
    const int batch = fusedn + (restart ? 1 : 0);
    hipGraphExec_t ge = nullptr;
    int rc = window_graph(t, pl, w, &ge);
    if (rc) return rc;
    if (prepare_only) {
      rc = window_graph(t, pl, w, &ge);  // the other instance; leaves the alternation where it was
      if (rc) return rc;
    } else {
      ++t->epoch;
      HIPC(hipGraphLaunch(ge, t->stream));
      account_window(t, pl, w);
      count_iterations(t, batch, batch);
    }
    cur_iter += batch;
    k += batch;
  }
  return 0;
}

// one colour class takes its block update -- its members in the same launches -- while `count` iterations of the global
// schedule pass.  global_class (dpgo_team_run_group, the classes of dpgo_team_set_groups): the class may have no member in
// this team, and then no solve is enqueued; what its members moved is asked to be published.
static int enqueue_group_update(dpgo_team *t, const LaunchCtx &c, int g, int count, bool global_class) {
  const dpgo_params_t &p = t->prm;
  const std::vector<int> &mem = t->groups[g];
  const int na = (int)t->ag.size();
  launch_copy(c, SEL_EVERY, -1, na, t->max_n, B_X, B_XPREV, 0);
  if (!(global_class && mem.empty())) {
    const int rc = enqueue_optimize_group(t, g);
    if (rc) return rc;
  }
  launch_status(c, SEL_EVERY, -1, na, t->max_n);
  if (!mem.empty()) {
    LaunchCtx cg = c;
    cg.ny = (int)mem.size();
    int gmn = 0;
    for (int k : mem) gmn = std::max(gmn, t->ag[k]->n);
    launch_status(cg, SEL_GROUP0 - g, -1, cg.ny, gmn, 1);
  }
  launch_advance(c, -1, na, 0, p.num_robots, p.restart_interval, 1, count);
  for (auto &a : t->ag) a->rel_src = REL_TILES_D;
  for (int k : mem) {
    if (global_class) t->ag[k]->publish_requested = true;
    mark_optimized(t, *t->ag[k], REL_TILES_E, true);
  }
  count_iterations(t, count, count);
  return 0;
}

}  // namespace dpgo_host

extern "C" {

int dpgo_team_step_begin(dpgo_team_t *t, int sel_id) {
  if (sync_descs(t)) return DPGO_ERR;
  return enqueue_team_iteration(t, false, restart_due(t), local_or_remote(t, sel_id), PHASE_BEGIN);
}

int dpgo_team_step_end(dpgo_team_t *t, int sel_id) {
  const int sel = local_or_remote(t, sel_id);
  if (sel >= 0 && !neighbor_poses_ready(*t->ag[sel], t->prm.acceleration ? 1 : 0)) { set_err("neighbour poses missing"); return DPGO_NOT_READY; }
  const int rc = enqueue_team_iteration(t, false, restart_due(t), sel, PHASE_END);
  if (rc) return rc;
  account_iteration(t, sel, t->last_update_src);
  return 0;
}

int dpgo_team_run(dpgo_team_t *t, int iters) { return team_run_impl(t, iters, false); }
int dpgo_team_prepare(dpgo_team_t *t, int iters) { return team_run_impl(t, iters, true); }

// one colour class: `count` block updates of the global schedule (count = global size of the class)
int dpgo_team_run_group(dpgo_team_t *t, int g, int count) {
  if (sync_descs(t)) return DPGO_ERR;
  if (t->prm.acceleration) { set_err("colour-parallel sweeps need acceleration = 0"); return DPGO_ERR; }
  if (g < 0 || g >= (int)t->groups.size()) { set_err("bad group"); return DPGO_ERR; }
  LaunchCtx c = t->ctx();
  if (t->ag.empty()) return 0;
  return enqueue_group_update(t, c, g, count, true);
}

int dpgo_team_run_colored(dpgo_team_t *t, int sweeps) {
  if (sync_descs(t)) return DPGO_ERR;
  if (t->prm.acceleration) { set_err("colour-parallel sweeps need acceleration = 0"); return DPGO_ERR; }
  for (auto &a : t->ag) if (!a->has_X) { set_err("run_colored before set_initial"); return DPGO_NOT_READY; }
  LaunchCtx c = t->ctx();
  for (int sw = 0; sw < sweeps; ++sw)
    for (size_t g = 0; g < t->groups.size(); ++g) {
      const int rc = enqueue_group_update(t, c, (int)g, (int)t->groups[g].size(), false);
      if (rc) return rc;
    }
  return 0;
}

// Simultaneous updates: every local agent takes one preconditioned RGD step per tick, all in the same launches
// (blockIdx.y = agent), each from the neighbour poses as they were when the tick began.  This is the deterministic
// instance of the asynchronous (ASAPP) mode in which all Poisson clocks fire together (src/PGOAgentROS.cpp:119-127
// runs the same RGD step from whatever neighbour poses have arrived); one graph replay per call.
int dpgo_team_run_simultaneous(dpgo_team_t *t, int ticks) {
  if (sync_descs(t)) return DPGO_ERR;
  const dpgo_params_t &p = t->prm;
  if (p.method != DPGO_METHOD_RGD || !p.rgd_use_preconditioner || p.acceleration || p.rgd_line_search) {
    set_err("simultaneous updates: preconditioned RGD with the fixed step, without acceleration (the ASAPP configuration)");
    return DPGO_ERR;
  }
  for (auto &a : t->ag) if (!a->has_X) { set_err("run_simultaneous before set_initial"); return DPGO_NOT_READY; }
  const int na = (int)t->ag.size();
  if (na == 0 || ticks <= 0) return 0;
  revalidate_graphs(t);
  LaunchCtx c = t->ctx();
  c.ny = na;
  const int sel = SEL_ALL, mn = t->max_n;  // (= the class t->all_group: the local agents in index order)
  for (int left = ticks; left > 0;) {
    const int B = std::min(left, dpgo_team::MAX_GRAPH_ITERS);
    hipGraphExec_t ge = nullptr;
    const int rc = graph_for_key(t, -(B + 1), false, [&] {  // negative keys: simultaneous-update graphs
      for (int rep = 0; rep < B; ++rep) {
        // XPrev only feeds the status of the LAST tick of a run (|X - XPrev|^2 left by its step kernel): the copy is
        // taken in the last tick of every graph, two launches per tick otherwise
        if (rep == B - 1) launch_copy(c, SEL_EVERY, -1, na, mn, B_X, B_XPREV, 0);
        launch_eval(c, sel, mn, B_X, B_EGRAD, B_GF, PART_C, eval_opts(t, 2, 0, 0));
        // (statistics -- X2 snapshot, |X - XPrev|^2 -- only from the last tick of a graph: nothing reads the others')
        launch_precond(c, sel, mn, PM_RGD_, B_X, B_GF, B_Z, 0, 0, p.rgd_stepsize, 0, p.num_robots, PADV_NONE, p.restart_interval,
                       rep == B - 1 ? 0 : PA_NO_STATS);
      }
      return 0;
    }, &ge);
    if (rc) return rc;
    ++t->epoch;
    HIPC(hipGraphLaunch(ge, t->stream));
    left -= B;
  }
  // f_opt / gradnorm_opt of every agent on the snapshot of its last step, then the counters
  launch_eval(c, sel, mn, B_X2, B_EGRAD2, B_GF2, PART_A, eval_opts(t, 0, 0, 0));
  LaunchCtx c1 = t->ctx();
  launch_advance(c1, -1, na, 0, p.num_robots, p.restart_interval, 1, ticks, ticks * na);
  for (auto &a : t->ag) {
    count_work(t, *a, ticks, ticks + 1);
    a->rel_src = REL_FUSED_B; a->opt_pending_rgd = true; a->publish_requested = true;
    mark_optimized(t, *a, REL_FUSED_B, true);
  }
  count_iterations(t, ticks, ticks * na);
  return 0;
}

// `iters` global iterations in which robot sel_ids[q] holds the token, enqueued without any host synchronisation:
// every process calls this with the same list; neighbours in other processes are read in place (dpgo_team_import_peer)
// and ordered by the mailboxes.  Per iteration k (t->iter), with acceleration:
//   wait   fin[s] >= k         for s = the token holder of k - 1, if it neighbours a local robot from another process
//                              (it has finished reading the Y this process is about to move)
//   P1     iterate(false) part of every local robot (dpgo_team_step_begin)
//   signal ready[a] = k + 1    into the mailbox of the token holder's team, for its local neighbours a
//   wait   ready[b] >= k + 1   for the remote neighbours b of a local token holder
//   P2     the block update (dpgo_team_step_end)
//   signal fin[sel] = k + 1    into the mailboxes of the token holder's remote neighbours
// Without acceleration only block updates move poses: the token holder waits for fin[b] of every remote neighbour's last
// block update (what it reads is final, and nobody still reads what it overwrites).
int dpgo_team_run_peer(dpgo_team_t *t, const int *sel_ids, int iters) {
  if (check_exchange_error(t)) return DPGO_ERR;  // (a time-out of an earlier run that nobody has looked at yet)
  if (sync_descs(t)) return DPGO_ERR;
  if (ensure_mailbox(t)) return DPGO_ERR;
  const dpgo_params_t &p = t->prm;
  const int NR = p.num_robots;
  for (auto &a : t->ag) if (!a->has_X) { set_err("run_peer before set_initial"); return DPGO_NOT_READY; }
  // remote neighbours of every local robot must be readable in place and reachable by mail
  for (auto &a : t->ag)
    for (int b : a->neighbors)
      if (!t->id2local.count(b) && (!t->peers.count(b) || !t->peer_mail.count(b))) {
        set_err("run_peer: neighbour " + std::to_string(b) + " of robot " + std::to_string(a->id) + " was not imported (state + mailbox)");
        return DPGO_ERR;
      }
  auto is_nbr = [](const Agent &a, int b) { return std::binary_search(a.neighbors.begin(), a.neighbors.end(), b); };
  auto flush_waits = [&](MailWaits &w) { launch_mail_wait(t->stream, t->d_mail.p, w, t->h_bar_err); w.count = 0; };
  auto add_wait = [&](MailWaits &w, int index, unsigned long long value) {
    for (int q = 0; q < w.count; ++q) if (w.index[q] == index) { w.value[q] = std::max(w.value[q], value); return; }
    if (w.count == MAIL_MAX) flush_waits(w);
    w.index[w.count] = index; w.value[w.count] = value; ++w.count;
  };
  auto flush_sigs = [&](MailSignals &s) { launch_mail_signal(t->stream, s); s.count = 0; };
  auto add_sig = [&](MailSignals &s, unsigned long long *word, unsigned long long value) {
    for (int q = 0; q < s.count; ++q) if (s.word[q] == word) { s.value[q] = value; return; }
    if (s.count == MAIL_MAX) flush_sigs(s);
    s.word[s.count] = word; s.value[s.count] = value; ++s.count;
  };
  int prev_sel = -1;
  {
    // (the token holder of the iteration in front of this call, if any)
    unsigned long long best = 0;
    for (int b = 0; b < NR; ++b) if (t->last_fin[b] > best) { best = t->last_fin[b]; prev_sel = b; }
    if (best != (unsigned long long)t->iter) prev_sel = -1;
  }
  for (int q = 0; q < iters; ++q) {
    const int sel_id = sel_ids[q];
    if (sel_id < 0 || sel_id >= NR) { set_err("run_peer: bad robot id in the schedule"); return DPGO_ERR; }
    const unsigned long long k = (unsigned long long)t->iter;
    const int sel = local_or_remote(t, sel_id);
    const bool restart = restart_due(t);
    MailWaits w{};
    MailSignals s{};
    if (p.acceleration && prev_sel >= 0 && !t->id2local.count(prev_sel))
      for (auto &a : t->ag) if (is_nbr(*a, prev_sel)) { add_wait(w, NR + prev_sel, k); break; }
    flush_waits(w);
    int rc = enqueue_team_iteration(t, false, restart, sel, PHASE_BEGIN);
    if (rc) return rc;
    if (p.acceleration && sel == SEL_REMOTE)
      for (auto &a : t->ag) if (is_nbr(*a, sel_id)) add_sig(s, t->peer_mail[sel_id] + a->id, k + 1);
    flush_sigs(s);
    if (sel >= 0)
      for (int b : t->ag[sel]->neighbors)
        if (!t->id2local.count(b)) {
          if (p.acceleration) add_wait(w, b, k + 1);
          if (t->last_fin[b] > 0) add_wait(w, NR + b, t->last_fin[b]);
        }
    flush_waits(w);
    rc = enqueue_team_iteration(t, false, restart, sel, PHASE_END);
    if (rc) return rc;
    account_iteration(t, sel, t->last_update_src);
    if (sel >= 0)
      for (int b : t->ag[sel]->neighbors)
        if (!t->id2local.count(b)) add_sig(s, t->peer_mail[b] + NR + sel_id, k + 1);
    flush_sigs(s);
    t->last_fin[sel_id] = k + 1;
    prev_sel = sel_id;
  }
  return DPGO_OK;
}

}  // extern "C"
