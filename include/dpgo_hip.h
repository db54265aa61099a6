/*
 * dpgo_hip.h -- C-ABI of the MI355X-native RBCD hot path (libdpgo_hip.so).
 *
 * This is the drop-in boundary underneath the C++ facade `namespace DPGO` (headers under include/DPGO/) that
 * the ROS wrapper of mit-acl/dpgo_ros subclasses (include/dpgo_ros/PGOAgentROS.h:121
 * `class PGOAgentROS : public PGOAgent`).  Each entry point cites the reference call site it
 * serves (paths relative to /root/reference).  Plain pointers and sizes only; no torch types.
 *
 * Conventions (d = 3, k = 4, r = relaxation rank in [3,8]):
 *   X is r x (4 n) column-major: X[(4*i + c)*r + a]; c<3 -> column c of Y_i, c=3 -> p_i.
 *   A "pose" is the r x 4 block of 4r contiguous doubles (Eigen column-major LiftedPose::getData()).
 *   All arithmetic is fp64 on the device.  Host pointers unless the name says _device.
 * Return codes: 0 = ok, >0 = not available yet (the facade maps to `false`), <0 = fatal (CHECK).
 */
#ifndef DPGO_HIP_H
#define DPGO_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* RelativeSEMeasurement(r1,r2,p1,p2,R,t,kappa,tau) + weight, fixedWeight
 * (src/utils.cpp:109-149; src/PGOAgentROS.cpp:740-745) */
typedef struct {
  int r1, p1, r2, p2;
  double R[9]; /* row-major 3x3 */
  double t[3];
  double kappa, tau, weight;
  int fixed_weight;
  int is_known_inlier;
} dpgo_measurement_t;

enum { DPGO_METHOD_RTR = 0, DPGO_METHOD_RGD = 1 };       /* ROptParameters::ROptMethod */
/* RobustCostParameters::Type, the six names src/PGOAgentROSNode.cpp:178-188 accepts.  Weight functions w(r) of the residual
 * r (dpgo_agent_robust_weight; [UPSTREAM-RECALL] mit-acl/dpgo src/DPGO_robust.cpp, the library is absent from the mount):
 *   L2 1 | L1 1 / r | Huber r < huber_threshold ? 1 : huber_threshold / r | TLS r < tls_threshold ? 1 : 0 |
 *   GM 1 / (1 + r^2)^2 | GNC_TLS Yang et al. RA-L 2020 with the running mu */
enum { DPGO_COST_L2 = 0, DPGO_COST_L1 = 1, DPGO_COST_HUBER = 2, DPGO_COST_TLS = 3, DPGO_COST_GM = 4, DPGO_COST_GNC_TLS = 5 };
enum { DPGO_WAIT_FOR_DATA = 0, DPGO_WAIT_FOR_INITIALIZATION = 1, DPGO_INITIALIZED = 2 }; /* msg/Status.msg:1-3 */
enum { DPGO_WEIGHT_LIBRARY = 0, DPGO_WEIGHT_WRAPPER = 1 }; /* info-matrix vs kappa=1e4,tau=1e2 */
enum { DPGO_OK = 0, DPGO_NOT_READY = 1, DPGO_ERR = -1 };
/* preconditioner of the local solves.  The reference's is a sparse Cholesky solve with Q + shift I.  Two forms
 * of that SAME operator are built here: DENSE, the explicit inverse (N^2 doubles, N = 4 poses; small agents), and
 * TWO_LEVEL, the exact nested-dissection / Schur-complement form (dense inverses of p subdomains + the separator block:
 * 8 MB instead of 32 MB at 500 poses on sphere2500, 0.9 GB instead of 4.2 GB for cubicle as one agent, 4 GB for a
 * 60 000-pose chain) -- equal to round-off.  BLOCK_JACOBI (the inverses of the 4 x 4 diagonal blocks) is NOT the
 * reference's preconditioner: it runs only when asked for (precond_mode 2; restated in the oracle for its own parity
 * tests) or when neither exact form fits the device. */
enum { DPGO_PRECOND_AUTO = 0, DPGO_PRECOND_DENSE = 1, DPGO_PRECOND_BLOCK_JACOBI = 2, DPGO_PRECOND_TWO_LEVEL = 3 };
/* largest pose index dpgo_agent_add_measurements accepts (a dense preconditioner of (4n)^2 doubles is the limit
 * long before this; see dpgo_agent memory guard in DESIGN.md 3) */
#define DPGO_MAX_POSE_INDEX 1000000

/* PGOAgentParameters fields written by src/PGOAgentROSNode.cpp:80-231 */
typedef struct {
  int d, r, num_robots;
  int method;
  double rgd_stepsize;
  int rgd_use_preconditioner;
  int rtr_iterations;
  int rtr_tcg_iterations;
  double gradnorm_tol;
  double rtr_initial_radius;
  double rtr_max_radius;
  double precond_shift;
  int acceleration;
  int restart_interval;
  double rel_change_tol;
  int max_num_iters;
  int robust_cost_type;
  double gnc_barc, gnc_mu_step, gnc_init_mu;
  int robust_opt_num_weight_updates, robust_opt_inner_iters;
  double robust_opt_min_convergence_ratio;
  int weights_as_float32;
  int robust_opt_num_resets;  /* src/PGOAgentROSNode.cpp:213: written by the wrapper, never read by it; its semantics live
                               * in the absent library -> carried, validated (>= 0), no effect */
  int precond_mode;           /* DPGO_PRECOND_*: 0 automatic (dense inverse for small agents, the two-level form where it
                               * streams less than half the dense bytes), 1 dense inverse (error if it does not fit),
                               * 2 block-Jacobi, 3 two-level for every agent */
  int status_every_iterate;   /* 0 (default): relativeChange / readyToTerminate describe the last iterate(true) of the
                               * agent [UPSTREAM-RECALL]; 1: refreshed by every iterate (round-1 behaviour) */
  /* RGD with a backtracking (Armijo) line search on the retraction curve (north_star "RTR/RGD line search"; SURVEY App. B:
   * "a backtracking variant exists" [UPSTREAM-RECALL]; no wrapper call site selects it -- src/PGOAgentROSNode.cpp:86-97
   * writes method, RGD_stepsize, RGD_use_preconditioner only -- so it is off unless asked for).  Trial steps
   * t_j = rgd_stepsize * rgd_ls_shrink^j, j = 0 .. rgd_ls_max_backoffs (at most 7: eight trial points, all evaluated by
   * one pass over Q); the first j with f(Retr_x(-t_j d)) <= f(x) - rgd_ls_sigma t_j <grad f(x), d> is taken; none: x
   * stays put (dpgo_opt_result_t.accepted = 0). */
  int rgd_line_search;
  int rgd_ls_max_backoffs;
  double rgd_ls_shrink;
  double rgd_ls_sigma;
  double tls_threshold;       /* RobustCostParameters::TLSThreshold [UPSTREAM-RECALL: 10]; no wrapper call site writes it */
  double huber_threshold;     /* RobustCostParameters::HuberThreshold [UPSTREAM-RECALL: 3]; likewise */
} dpgo_params_t;

/* mLocalOptResult.{success,fInit,fOpt,gradNormInit,gradNormOpt} (src/PGOAgentROS.cpp:169-172) */
typedef struct {
  int success;
  double f_init, f_opt, gradnorm_init, gradnorm_opt;
  int rtr_outer_iters, tcg_iters_total, hessvec_count, precond_count, accepted;
  int ls_backoffs; /* RGD line search: back-offs before the accepted step */
} dpgo_opt_result_t;

/* PGOAgentStatus(agentID,state,instanceNumber,iterationNumber,readyToTerminate,relativeChange)
 * (src/utils.cpp:262-281; tests/testUtils.cpp:56-65) */
typedef struct {
  int agent_id, state, instance_number, iteration_number, ready_to_terminate;
  double relative_change;
} dpgo_status_t;

void dpgo_default_params(dpgo_params_t *p, int r, int num_robots);
const char *dpgo_last_error(void);

/* ---- dataset input: read_g2o_file (src/PGODatasetPublisherNode.cpp:80),
 *      PGOLogger::loadMeasurements (:168), contiguous partition (:84-135) ---- */
int dpgo_read_g2o(const char *path, int weight_mode, dpgo_measurement_t **out, int *num_poses);
int dpgo_read_measurements_csv(const char *path, int weight_mode, dpgo_measurement_t **out);
/* robust inter-robot frame alignment: n candidate transforms T_world_robot (3x4 column-major
 * each, one per shared loop closure with an initialised neighbour; updateNeighborPoses ->
 * initializeInGlobalFrame, src/PGOAgentROS.cpp:1276, 353-358) -> GNC-TLS rotation averaging (chordal metric,
 * threshold = chord of max_rotation_error_rad) then GNC-TLS translation averaging on the rotation inliers.
 * DPGO_OK, or DPGO_NOT_READY when fewer than min_inliers (robustInitMinInliers, Node.cpp:150) agree.
 * inlier: n flags or NULL.  Host arithmetic only. */
int dpgo_robust_frame_alignment(const double *T_candidates, int n, double max_rotation_error_rad,
                                double max_translation_error, int min_inliers, double *T_out, int *inlier);
/* robust local initialisation (InitializationMethod::GNC_TLS, src/PGOAgentROSNode.cpp:111-112): single-robot
 * GNC-TLS solve on the device with r = d = 3 -- odometry chain as the initial guess and fixed at weight 1,
 * loop closures re-weighted robust_opt_num_weight_updates times, robust_opt_inner_iters RTR iterations
 * per weighting (gnc_*, rtr_*, gradnorm_tol of `gnc` are used; r / num_robots / method / acceleration are
 * overridden).  T_out: 3x4 column-major per pose; weights_out: nm final weights in input order, or NULL. */
int dpgo_robust_local_init(int device, const dpgo_measurement_t *m, int nm, int num_poses, const dpgo_params_t *gnc,
                           double *T_out, double *weights_out);
/* writers (the PGOLogger::logMeasurements / logTrajectory role): the CSV of loadMeasurements
 * (data/tunnels/robot0/measurements.csv:1, weights and inlier flags included so GNC results round-trip), g2o
 * with isotropic information blocks (global index = robot_offsets[robot] + frame; NULL = single robot; T =
 * 3x4 column-major poses or NULL for edges only), and a trajectory CSV "pose_index,qx,qy,qz,qw,tx,ty,tz".
 * Return the number of records written, -1 on I/O failure. */
int dpgo_write_measurements_csv(const char *path, const dpgo_measurement_t *m, int nm);
int dpgo_write_g2o(const char *path, const dpgo_measurement_t *m, int nm, const double *T, int num_poses,
                   const int *robot_offsets);
int dpgo_write_trajectory_csv(const char *path, const double *T, int num_poses);
void dpgo_partition(dpgo_measurement_t *m, int nm, int num_poses, int num_robots, int weight_mode);
void dpgo_free(void *p);
void dpgo_odometry_init(const dpgo_measurement_t *m, int nm, int num_poses, double *T /* 3x4 per pose */);
/* two-stage chordal relaxation on the GPU (dense SPD solves), single-robot numbering; T as above.
 * PGOAgent::initialize() with InitializationMethod::Chordal (src/PGOAgentROS.cpp:348, Node.cpp:106-112) */
int dpgo_chordal_init(int device, const dpgo_measurement_t *m, int nm, int num_poses, double *T);
void dpgo_fixed_stiefel(int r, double *YLift);
void dpgo_lift(const double *T, int num_poses, const double *YLift, int r, double *X);

/* ---- a team = the agents resident on one GPU (one process per GPU) ---- */
typedef struct dpgo_team dpgo_team_t;
/* agent_ids: global robot ids hosted here.  stream: hipStream_t or NULL (library-owned stream). */
dpgo_team_t *dpgo_team_create(int device, const dpgo_params_t *p, int num_local, const int *agent_ids,
                              void *stream);
void dpgo_team_destroy(dpgo_team_t *t);
int dpgo_team_num_local(const dpgo_team_t *t);
void *dpgo_team_stream(dpgo_team_t *t);
int dpgo_team_synchronize(dpgo_team_t *t);

/* PGOAgent::addMeasurement (src/PGOAgentROS.cpp:277,1307).  Measurements not touching `id` are ignored. */
int dpgo_agent_add_measurements(dpgo_team_t *t, int id, const dpgo_measurement_t *m, int count);
int dpgo_agent_num_poses(dpgo_team_t *t, int id);                       /* num_poses() :285 */
int dpgo_agent_num_measurements(dpgo_team_t *t, int id, int *odom, int *priv, int *shared); /* :343-345 */
int dpgo_agent_get_neighbors(dpgo_team_t *t, int id, int *ids);         /* getNeighbors() :663 */
int dpgo_agent_public_pose_ids(dpgo_team_t *t, int id, int nbr, int *frames);
int dpgo_agent_neighbor_pose_ids(dpgo_team_t *t, int id, int nbr, int *frames); /* activeNeighborPublicPoseIDs :1394 */
/* initializeInGlobalFrame-equivalent entry: set the lifted iterate (r x 4n); X->XPrev,Y,V; INITIALIZED */
int dpgo_agent_set_X(dpgo_team_t *t, int id, const double *X);
/* which: 0 X, 1 Y (auxiliary), 2 V, 3 XPrev */
int dpgo_agent_get_X(dpgo_team_t *t, int id, int which, double *X);
/* getSharedPoseDictWithNeighbor / getAuxSharedPoseDictWithNeighbor (:668,:666); order = public_pose_ids */
int dpgo_agent_get_public_poses(dpgo_team_t *t, int id, int nbr, int aux, double *poses);
/* updateNeighborPoses / updateAuxNeighborPoses (:1276,:1278) */
int dpgo_agent_update_neighbor_poses(dpgo_team_t *t, int id, int nbr, int aux, int count,
                                     const int *frames, const double *poses);
/* same exchange with device buffers (packed slab, order = public_pose_ids / neighbor_pose_ids):
 * the RCCL point-to-point payload that replaces msg/PublicPoses.msg (:662-690, :1255-1284) */
int dpgo_agent_pack_public_poses_device(dpgo_team_t *t, int id, int nbr, int aux, double *dev_out);
int dpgo_agent_unpack_neighbor_poses_device(dpgo_team_t *t, int id, int nbr, int aux, const double *dev_in);

int dpgo_agent_iterate(dpgo_team_t *t, int id, int do_optimization);    /* :160 (true), :1185 (false) */
int dpgo_agent_get_status(dpgo_team_t *t, int id, dpgo_status_t *s);     /* getStatus() :616 */
int dpgo_agent_get_opt_result(dpgo_team_t *t, int id, dpgo_opt_result_t *r); /* :169-172 */
int dpgo_agent_iteration_number(dpgo_team_t *t, int id);                 /* iteration_number() :139 */
/* preconditioner the agent actually runs (DPGO_PRECOND_DENSE, _TWO_LEVEL or _BLOCK_JACOBI), after its data matrices
 * were built; <0 on error */
int dpgo_agent_preconditioner(dpgo_team_t *t, int id);
/* diagnostic, out[8]: {mode, subdomains, separator poses, workgroups of an apply, workgroups that own separator poses,
 * bytes one apply streams, bytes of the dense inverse, largest subdomain (poses)} */
int dpgo_agent_preconditioner_info(dpgo_team_t *t, int id, double *out);
/* the dissection behind the two-level form, host arithmetic only (csrc/twolevel_plan.cpp): block-CSR pattern of Q (row j
 * lists the poses coupled to j, diagonal included) -> sub_of[n] (subdomain of a pose, -1 = separator); max_sub <= 0: the
 * subdomain size that streams the fewest bytes.  info[6]: {subdomains, separator poses, workgroups, producer workgroups,
 * bytes per apply, 1 if the automatic mode would pick this form over the dense inverse} */
int dpgo_two_level_plan(int n, const int *rowptr, const int *col, int max_sub, int *sub_of, double *info);
int dpgo_agent_publish_requested(dpgo_team_t *t, int id, int clear);     /* mPublishPublicPosesRequested :109-112 */
int dpgo_agent_set_iteration_number(dpgo_team_t *t, int id, int iteration); /* mIterationNumber = ... (RECOVER, :1196) */

/* ---- QuadraticProblem surface for parity (f, EucGrad, RieGrad, Hessian, PreConditioner) ---- */
int dpgo_agent_build_problem(dpgo_team_t *t, int id, int aux);
int dpgo_agent_eval(dpgo_team_t *t, int id, const double *X, double *f, double *egrad, double *rgrad);
int dpgo_agent_hessvec(dpgo_team_t *t, int id, const double *X, const double *eta, double *out);
int dpgo_agent_precondition(dpgo_team_t *t, int id, const double *X, const double *V, double *out);
/* |z (Q + shift I) - v| / |v| for a fixed pseudo-random v and z = the device's preconditioner apply: how well the operator
 * the kernels run (dense inverse or two-level form) inverts Q + shift I (the reference solves with a Cholesky factor) */
int dpgo_agent_preconditioner_residual(dpgo_team_t *t, int id, double *rel);
int dpgo_agent_get_Q(dpgo_team_t *t, int id, int *rowptr, int *col, double *val); /* returns #blocks */
int dpgo_agent_get_G(dpgo_team_t *t, int id, double *G);

/* ---- lifted SE manifold ops on the device (host in/out), n poses of r x 4 ---- */
int dpgo_project_manifold(dpgo_team_t *t, const double *X, int n, double *out);
int dpgo_tangent_project(dpgo_team_t *t, const double *X, const double *V, int n, double *out);
int dpgo_retract(dpgo_team_t *t, const double *X, const double *eta, int n, double *out);

/* ---- robust path (src/PGOAgentROS.cpp:1218,1049,1050,1341,210,1351; Node.cpp:201) ---- */
int dpgo_agent_compute_residual(dpgo_team_t *t, int id, const dpgo_measurement_t *m, double *residual);
double dpgo_agent_robust_weight(dpgo_team_t *t, int id, double residual);
int dpgo_agent_update_measurement_weights(dpgo_team_t *t, int id);
int dpgo_agent_set_measurement_weight(dpgo_team_t *t, int id, int r1, int p1, int r2, int p2, double w, int fixed);
int dpgo_agent_get_measurements(dpgo_team_t *t, int id, dpgo_measurement_t *out);
/* the same three calls for every stored measurement at once (order of dpgo_agent_get_measurements: odometry,
 * private loop closures, shared loop closures, each in insertion order): one residual launch and one copy per
 * UPDATE_WEIGHT instead of one per loop closure (src/PGOAgentROS.cpp:1049 is called in a loop over all of them).
 * available[k] = 0 where a neighbour pose is missing.  Returns the count. */
int dpgo_agent_compute_residuals(dpgo_team_t *t, int id, double *residuals, int *available);
int dpgo_agent_set_measurement_weights(dpgo_team_t *t, int id, const double *weights, const int *fixed, int count);
/* restart of the Nesterov sequences (V = Y = X, gamma = alpha = 0) that follows a weight update */
int dpgo_agent_reset_acceleration(dpgo_team_t *t, int id);
int dpgo_agent_should_update_weights(dpgo_team_t *t, int id);
int dpgo_agent_clear_data_matrices(dpgo_team_t *t, int id);
double dpgo_error_threshold_at_quantile(double quantile, int dim);

/* ---- synchronous schedule on the device (src/PGOAgentROS.cpp:129-220,443-504,1161-1189):
 *      all agents of the problem live in this team; exchange is device-to-device ---- */
int dpgo_team_set_schedule(dpgo_team_t *t, const int *order, int len);
/* UpdateRule::Uniform (include/dpgo_ros/PGOAgentROS.h:35-41,76; src/PGOAgentROS.cpp:446-463): `length` token holders drawn
 * uniformly with replacement by the wrapper's own recipe (std::discrete_distribution over the robots, std::mt19937) from an
 * engine of the given seed (the wrapper seeds from std::random_device), installed as the schedule; order_out may be NULL */
int dpgo_team_set_uniform_schedule(dpgo_team_t *t, unsigned seed, int length, int *order_out);
int dpgo_team_set_initial(dpgo_team_t *t, const double *T, const double *YLift, const int *offsets);
int dpgo_team_exchange_all(dpgo_team_t *t);
/* run `iters` global RBCD iterations without host synchronisation (RGD: one hipGraph replay each) */
int dpgo_team_run(dpgo_team_t *t, int iters);
/* capture and instantiate, without executing anything, every hipGraph that dpgo_team_run(t, iters) would replay from
 * the current iteration counter (a first run otherwise builds them on the fly: ~0.3 ms per distinct batch size) */
int dpgo_team_prepare(dpgo_team_t *t, int iters);
/* the same iteration split around the neighbour exchange, for teams that hold only part of the agents
 * (one process per GPU): begin = iterate(false) part of every local agent; [exchange]; end = local solve
 * of `sel_id` if it lives here + bookkeeping.  sel_id is a global robot id. */
int dpgo_team_step_begin(dpgo_team_t *t, int sel_id);
int dpgo_team_step_end(dpgo_team_t *t, int sel_id);
/* colour-parallel sweeps: agents without a shared edge take their block update in the same
 * launches; identical to the sequential schedule that visits the colour classes in order (class 0 first,
 * members in id order).  One sweep = one block update of every agent.  Needs acceleration = 0. */
int dpgo_team_get_coloring(dpgo_team_t *t, int *color_of_agent); /* returns the number of classes */
/* simultaneous updates (the ASAPP configuration: preconditioned RGD, no acceleration): every local agent takes
 * one RGD step per tick in the same launches, from the neighbour poses as of the beginning of the tick -- the
 * deterministic instance of the asynchronous mode (src/PGOAgentROS.cpp:119-127) in which all clocks fire together.
 * Each agent's iteration number advances by `ticks`. */
int dpgo_team_run_simultaneous(dpgo_team_t *t, int ticks);
int dpgo_team_run_colored(dpgo_team_t *t, int sweeps);
/* the same with an explicit (global) colouring, one class at a time, for one-process-per-GPU runs */
int dpgo_team_set_groups(dpgo_team_t *t, int num_groups, const int *group_ptr, const int *member_ids);
int dpgo_team_run_group(dpgo_team_t *t, int group, int count);
int dpgo_team_iteration(dpgo_team_t *t);
/* global cost of the concatenated iterate, evaluated on the device */
int dpgo_team_cost(dpgo_team_t *t, double *f);
int dpgo_team_update_weights(dpgo_team_t *t);
/* PGOAgent::shouldTerminate() as the leader (robot 0) evaluates it from the team's statuses
 * (src/PGOAgentROS.cpp:208): 1 terminate, 0 continue, <0 error.  All robots must live in this team. */
int dpgo_team_should_terminate(dpgo_team_t *t);
/* global-optimality certificate (Rosen et al. 2019; the "certifiably correct" of Tian et al.): S(X) = Q - Lambda(X),
 * Lambda = blockdiag_i [[Sym(Y_i^T (X Q)_i,rot), 0], [0, 0]]; X is a global optimum when S(X) is positive semidefinite.
 * The smallest eigenvalue is found by LOBPCG on the device (csrc/certify.hip).  All robots must live in this team and be
 * INITIALIZED (else DPGO_ERR with a message).  Changes no solver state. */
typedef struct {
  double lambda_min;   /* smallest Ritz value found (deflated: min(0, .) on Z-perp) */
  double residual;     /* |S v - lambda v| / |v| of its Ritz vector */
  double norm_bound;   /* the Gershgorin bound s on |S| */
  int certified;       /* 1: converged and lambda_min >= -eta; 0: lambda_min < -eta (v: negative curvature); -1: not converged */
  int iterations, block, deflated;
} dpgo_certificate_t;
/* flags of dpgo_team_certify.  Deflation (default) projects out Z = [rows of X; e_t], e_t = 1 on every translation
 * coordinate (S Z^T = 0 at a critical point); the preconditioner is the block-Jacobi (Q_a + shift I)^-1 by agent (off when
 * an agent has the two-level form, and left out of an iteration whose last Ritz value is below -1e-3 s: far from a
 * critical point it inverts another operator); ETA_RELATIVE: eta is taken relative to s */
enum { DPGO_CERT_NO_DEFLATION = 1, DPGO_CERT_NO_PRECONDITIONER = 2, DPGO_CERT_ETA_RELATIVE = 4 };
/* S(X) V for a K x 4N block in team order (agents by offsets), K in 3..8: the operator itself, for tests */
int dpgo_team_certificate_apply(dpgo_team_t *t, int K, const double *V, double *out);
/* T V for a K x 4N block in team order, K in 3..8: the eigensolver's preconditioner itself, (Q_a + shift I)^-1 by agent
 * from its dense inverse or its 4 x 4 diagonal inverses, for tests.  DPGO_ERR where an agent has the two-level form */
int dpgo_team_certificate_precondition(dpgo_team_t *t, int K, const double *V, double *out);
/* verify the current iterate; v (4N doubles, team order) or NULL.  Converged: |S v - lambda v| <= tol * s; block 0 = r.
 * A block of K vectors needs K dimensions to live in: when 4N - nz < K (nz = the rank of Z, 0 with NO_DEFLATION; teams of
 * one to three poses) the call is refused with DPGO_ERR and a message that names 4N, nz and K -- pass a smaller block, or
 * NO_DEFLATION.  Changes no solver state. */
int dpgo_team_certify(dpgo_team_t *t, double eta, double tol, int max_iters, int block, int flags,
                      dpgo_certificate_t *out, double *v);
/* staircase step, host arithmetic: X (r x 4n) and v (4n) -> the rank r+1 point [X; 0] + alpha [0; v^T],
 * rotation blocks projected back to the Stiefel manifold */
int dpgo_escape_point(const double *X, int r, int num_poses, const double *v, double alpha, double *X_out);
/* SE-Sync rounding of the current iterate (Rosen et al. 2019, Alg. 2; csrc/round.hip): U = the top-3 left singular vectors of
 * the r x 3N rotation block of X; D = diag(1, 1, -1) when more poses have det(U^T Y_i) < 0 than > 0 (a tie keeps U);
 * R_i = the nearest rotation to D U^T Y_i (degenerate blocks completed by a cross product), t_i = D U^T p_i; every pose
 * then relative to the first in team order (T_0 = I, t_0 = 0).  With DPGO_ROUND_REFINE_TRANSLATIONS the translations are
 * re-solved for the rounded rotations (dpgo_translations_given_rotations on the team's measurements, current weights).
 * When the iterate is certified, f_rounded - f_relaxed bounds the suboptimality of T (up to the certificate's eta). */
typedef struct {
  double f_relaxed;      /* 1/2 <Q, X^T X> at the team's iterate */
  double f_rounded;      /* 1/2 <Q, T^T T> of the returned trajectory (the team's Q: current weights) */
  double sigma[8];       /* singular values of the r x 3N rotation block of X, descending; 0 beyond r */
  int r, reflected, refined, num_degenerate;
} dpgo_rounding_t;
enum { DPGO_ROUND_REFINE_TRANSLATIONS = 1 };
/* T = 12 doubles per pose in team order (R column-major, then t), anchored at the first pose.  All robots local and
 * INITIALIZED (the certificate's refusals and messages).  Changes no solver state. */
int dpgo_team_round(dpgo_team_t *t, int flags, double *T, dpgo_rounding_t *out);
/* t minimising sum_e w_e tau_e |t_j - t_i - R_i t~_e|^2 with t_0 = 0, for the rotations already in T (12 doubles per pose,
 * single-robot numbering); translations of T overwritten.  Stage 2 of dpgo_chordal_init, with its two paths in the same
 * cases.  DPGO_ERR with a message when edges of positive weight do not join every pose to pose 0. */
int dpgo_translations_given_rotations(int device, const dpgo_measurement_t *m, int nm, int num_poses, double *T);
/* ---- marginal pose covariances of a trajectory (csrc/covariance.hip) ----
 * T = (R_i, t_i) in team order, the layout dpgo_team_round returns.  Pose i is perturbed by xi_i = (phi_i, delta_i), rotation
 * first:  R_i <- R_i Exp(phi_i) (body frame),  t_i <- t_i + delta_i (world frame).  H = the Hessian at xi = 0 of the team's
 * cost 1/2 <T, T Q> (current weights) in these 6N coordinates; pose 0 (the anchor of dpgo_team_round) is held fixed:
 * H_red = H without its first 6 rows and columns, Sigma = H_red^-1 (the Laplace approximation of the posterior under the
 * cost's own noise model).  H is assembled on the device from S = Q - Lambda(T) (the certificate's operator at rank 3) and
 * inverted there by the blocked fp64 Cholesky of the dense preconditioner: three square matrices of 6(N-1) doubles a side.
 * DPGO_COV_SCHUR (csrc/covariance_schur.hip) computes the same blocks by robot-wise Schur complement: a pose that no shared
 * edge names (edges of weight 0 included) is interior to its robot; the interiors are eliminated one robot at a time and only
 * the Schur complement on the public poses is inverted as a whole.  Exact and deterministic; the device holds three square
 * matrices of order M = max(6 x the largest interior, 6 x the public poses), the separator, and per robot a matrix of
 * 6 |I_a| x 6 s_a doubles (s_a: the robot's public poses) -- bytes = 8 (3 M^2 + (6 |S|)^2 + sum_a 36 |I_a| s_a + max_a 36 |I_a| s_a)
 * for these large buffers, plus the small ones (N poses, P pairs, A robots, b stored blocks of Q, k = 6 max_a s_a):
 *   small = 8 (33 N + A ceil(max_a n_a / 256) + 4 (A + 1) + 72 (N + P)) + 48 k min(P, 65535, 2^23 / (6 k))
 *           + 24 (N + 2 P) + 24 P + 40 b + 4 (A + 1 + 2 N + |S|) + 56 (A + 2 P) + 8192 ceil(M / 32)
 *   (T, T Q, Lambda, scratch, statistics, kept and output blocks; the scratch of pairs between two robots; list entries of 24
 *    bytes; the work list; the maps and the index array 0 .. |S| - 1; a record of 56 bytes per set of the extraction kernels;
 *    the Linv blocks of the inverse.  DESIGN.md 5e). */
#define DPGO_COV_SCHUR 1
typedef struct {
  int n;                 /* 6 (N - 1): the order of H_red */
  double logdet;         /* log det H_red = 2 sum_k log L_kk, summed in index order (DPGO_COV_SCHUR: per factor, the factors
                          * summed on the host in robot order, the separator last) */
  double min_pivot;      /* smallest and largest L_kk^2 of the Cholesky factor (DPGO_COV_SCHUR: over all factors) */
  double max_pivot;
  double seconds_assemble; /* device time (events on the team's stream): Lambda, clearing and filling H_red (every assembly) */
  double seconds_invert;   /* ... Cholesky, triangular inverse, W^T W (DPGO_COV_SCHUR: every factorisation and product) */
} dpgo_covariance_t;
/* cov_diag: the N diagonal 6 x 6 blocks of Sigma, 36 doubles each, row-major, bitwise symmetric (pose 0: zeros);
 * cov_pairs (may be NULL when num_pairs is 0): the blocks Sigma_ab for pairs[2k] = a, pairs[2k + 1] = b (a pair that names
 * pose 0: zeros).  flags: 0 (the dense inverse) or DPGO_COV_SCHUR; any other bit is refused.  All robots local and INITIALIZED.  Refused with DPGO_ERR and a message before any device work:
 * T outside SE(3) (|R^T R - I| or |det R - 1| above 1e-8), a pair index outside [0, N), positive-weight edges that do not
 * join every pose to pose 0, 3 x n^2 x 8 bytes (DPGO_COV_SCHUR: the bytes above; the message names what sets them) above the
 * free device memory.  Refused after the factorisation: a non-positive pivot (T is not a minimum; DPGO_COV_SCHUR names the
 * robot whose interior block, or the separator, and the pose).  A refused call leaves cov_diag / cov_pairs untouched and *res all zero.
 * Changes no solver state; two calls give the same bits. */
int dpgo_team_marginal_covariances(dpgo_team_t *t, const double *T, int flags, int num_pairs, const int *pairs,
                                   double *cov_diag, double *cov_pairs, dpgo_covariance_t *res);
/* ---- the same covariances by nested dissection inside each robot (csrc/covariance_nested.hip; DESIGN.md 5e, "nested") ----
 * DPGO_COV_SCHUR takes its sets from the team alone: one robot has no separator at all, a few robots with large interiors pay
 * a dense inverse of order 6 |I_a| each.  Here a robot whose interior holds more than max_block poses has the pattern of its
 * block-CSR, restricted to the interior, dissected by the plan of the two-level preconditioner (dpgo_two_level_plan with
 * max_sub = max_block): the subdomains become BLOCKS of at most max_block + max_block / 5 poses, the dissection's separator
 * poses are PROMOTED into the robot's part of the separator S (public and promoted poses in team order).  A robot whose
 * interior fits is one block.  Blocks are ordered by robot, then by first pose; N_b = the separator poses coupled to block b,
 * ascending.  C_b = H_bb^-1, W_b = C_b H[b, N_b] (the coupled columns alone), S_c = H_SS - sum_b H[b, N_b]^T W_b (block after
 * block, no atomics), Sigma_SS = S_c^-1; the blocks of Sigma follow as for DPGO_COV_SCHUR with N_b in the place of a robot's
 * public poses, log det sums the blocks in order and the separator last.  Exact and deterministic (two calls: the same bits);
 * when no robot is split the call IS the DPGO_COV_SCHUR call (it delegates: the same bits and messages).
 * Device bytes, with n_b = 6 |I_b|, K_b = 6 |N_b|, s = 6 |S|:
 *   large = 8 (3 s^2  +  sum_b n_b K_b  +  max_b (3 n_b^2 + n_b K_b + K_b^2))
 *           (S_c, the inverse's work matrix and Sigma_SS; every kept W_b; the workspace of the largest block -- H_bb, work, C_b,
 *            B_b, B_b^T W_b.  Blocks are eliminated a batch at a time, batches filled in block order while their workspaces fit
 *            what is left of the free memory, 2 GiB at the most; the request that is checked counts the largest block alone)
 *   small = 8 (33 N + A ceil(max_a n_a / 256) + 4 (blocks + 1) + 72 (N + P)) + 48 max(K_max, 1) c + 24 (2 N + 3 P) + 40 Q
 *           + 232 blocks + 4 (N + sum_b |N_b| + A + 1) + 8192 (ceil(s / 32) + sum_b ceil(n_b / 32))
 *           (N poses, A robots, P pairs, Q stored blocks and shared-edge records, c = min(P, 65535, 2^23 / (6 max(K_max, 1)))
 *            pairs across blocks per launch; 232 bytes of tables per block: one record of 56, three products of 48, two assembly
 *            targets of 16).
 * A request above the free device memory plus the idle pooled buffers is refused before any device work; the message gives
 * both figures, says whether the separator or the batch workspace sets them, and that another max_block changes them. */
#define DPGO_COV_NESTED_DEFAULT_BLOCK 256
/* Host arithmetic only, no device: the sets for a global block-CSR pattern in team order (robot_of non-decreasing from 0
 * without gaps; a pose joined to a pose of another robot is public; pose 0 is fixed).  block_of[num_poses]: the block index,
 * -1 a separator pose, -2 pose 0.  info[6]: blocks, separator poses, promoted poses among them, the largest block (poses),
 * the largest |N_b|, sum_b |N_b|.  max_block <= 0: DPGO_COV_NESTED_DEFAULT_BLOCK.  Either output may be NULL. */
int dpgo_covariance_nested_plan(int num_poses, const int *robot_of, const int *rowptr, const int *col, int max_block,
                                int *block_of, int *info);
/* the same plan from the team's own structure (public: a pose that a shared-edge record names, edges of weight 0 included).
 * block_of: one entry per pose of the team in team order.  All robots local and INITIALIZED. */
int dpgo_team_covariance_nested_plan(dpgo_team_t *t, int max_block, int *block_of, int *info);
/* dpgo_team_marginal_covariances by that plan: the same arguments, outputs and conventions, max_block in the place of flags.
 * The refusals of DPGO_COV_SCHUR carry over (robots missing or not initialised, T outside SE(3), a pair outside [0, N), a
 * weighted graph that is not joined to pose 0, the bytes above); a non-positive pivot names the robot, the block and the pose,
 * or the separator.  A refused call leaves cov_diag / cov_pairs untouched and *res all zero.  Changes no solver state.  There
 * is no call across teams. */
int dpgo_team_marginal_covariances_nested(dpgo_team_t *t, const double *T, int max_block, int num_pairs, const int *pairs,
                                          double *cov_diag, double *cov_pairs, dpgo_covariance_t *res);
/* ---- candidate measurements gated by Mahalanobis distance (csrc/gate.hip) ----
 * A candidate is a dpgo_measurement_t (r1, p1) -> (r2, p2) with R~ (row-major), t~, kappa, tau; weight, fixed_weight and
 * is_known_inlier are ignored: it is a fresh measurement that is not in the graph.  Its endpoints map to the team poses i != j,
 * T_j ~ T_i T~.  With T and Sigma as above (R_i <- R_i Exp(phi_i), t_i <- t_i + delta_i, rotation first, pose 0 fixed):
 *   relative pose   R_ij = R_i^T R_j, t_ij = R_i^T (t_j - t_i), perturbed the same way: R_ij <- R_ij Exp(phi_ij),
 *                   t_ij <- t_ij + delta_ij (delta_ij in frame i)
 *   Jacobians       J_i = [[-R_ij^T, 0], [[t_ij]x, -R_i^T]],  J_j = [[I, 0], [0, R_i^T]]   (6 x 6, rotation first)
 *   sigma_rel       J_i Sigma_ii J_i^T + J_i Sigma_ij J_j^T + J_j Sigma_ij^T J_i^T + J_j Sigma_jj J_j^T, stored as (A + A^T) / 2:
 *                   bitwise symmetric, row-major; an endpoint that is pose 0 has zero blocks and needs no special case
 *   xi              (Log(R~^T R_ij)v, t_ij - t~): theta = atan2(|a|, c) with a the vee of the antisymmetric part and
 *                   c = (tr - 1) / 2; zero in gives zero out; within 0.1 rad of pi the axis comes from the symmetric part, and
 *                   theta = pi gives a finite vector of norm pi
 *   Sigma_meas      diag(I_3 / (2 kappa), I_3 / tau): the inverse Hessian of the candidate's own term
 *                   1/2 (kappa |R_ij - R~|_F^2 + tau |t_ij - t~|^2) of the cost at zero residual
 *   d2              xi^T (sigma_rel + Sigma_meas)^-1 xi by a 6 x 6 Cholesky; a non-positive pivot (garbage blocks) gives +inf.
 * A candidate passes at quantile q when sqrt(d2) <= dpgo_error_threshold_at_quantile(q, 6).
 * The blocks come from the covariance path `method` (max_block: DPGO_GATE_NESTED only, as in
 * dpgo_team_marginal_covariances_nested), asked for the candidates' pairs (i, j), each once; they stay on the device, one
 * kernel forms the outputs, and only xi (6 num), d2 (num) and sigma_rel (36 num) -- those that are not NULL -- come back.
 * With xi == d2 == NULL only the endpoints of cand are read: the relative-covariance query.  Duplicated candidates give
 * identical bits; two calls give the same bits.  Refused with DPGO_ERR and a message before any device work, every output
 * untouched: num <= 0; all three outputs NULL; exactly one of xi and d2 NULL; an unknown method; an endpoint that is not a
 * robot or pose of the team; i == j; and, when xi / d2 are requested, kappa <= 0 or tau <= 0, or R~ outside SO(3) by the
 * 1e-8 rule of T.  Every refusal of the chosen covariance path carries over with its own message (T outside SE(3), a
 * disconnected weighted graph, too little device memory, a non-positive pivot); the outputs are then untouched and *res all
 * zero.  *res: the path's own record.  Changes no solver state.  Across teams: dpgo_team_gate_candidates_across below. */
enum { DPGO_GATE_DENSE = 0, DPGO_GATE_SCHUR = 1, DPGO_GATE_NESTED = 2 };
int dpgo_team_gate_candidates(dpgo_team_t *t, const double *T, int method, int max_block /* NESTED only */,
                              int num, const dpgo_measurement_t *cand,
                              double *xi /* 6 num or NULL */, double *d2 /* num or NULL */,
                              double *sigma_rel /* 36 num or NULL */, dpgo_covariance_t *res);
/* ---- measurements that are in the graph audited by leave-one-out gating (csrc/audit.hip) ----
 * Record k is a dpgo_measurement_t (r1, p1) -> (r2, p2), team poses i != j, with R~ (row-major), t~, kappa, tau and
 * weight = w >= 0: the caller states that this measurement IS in the weighted graph at that weight (w = 0: not in the Hessian);
 * fixed_weight and is_known_inlier are ignored, and the records are taken on trust.  Its own information w W0 is in Sigma, so
 * its innovation is not independent of the estimate and the gate above does not apply; the audit takes the edge out again by
 * the Woodbury identity on the 6 x 6 blocks of its pair.  T, Sigma, the perturbation, R_ij, t_ij, J_i, J_j, sigma_rel, xi and
 * the logarithm are those of dpgo_team_gate_candidates.  Per record:
 *   scaling      s = (sqrt(2 kappa) x 3, sqrt(tau) x 3): diag(s)^2 = Sigma_meas^-1 = W0, the edge's Hessian at zero residual
 *   whitened     z = s o xi,  C_ab = sigma_rel,ab (s_a s_b)  (bitwise symmetric)
 *   matrices     A = I - w C, the redundancy matrix of the edge: PSD in exact arithmetic, singular exactly in the directions
 *                the graph knows through this edge alone;  B = I + (1 - w) C
 *   rho          1 - w tr(C) / 6 in [0, 1], the redundancy number
 *   pmin         A = L L^T; the smallest of the six pivots before the square root (pivots behind a non-positive one do not
 *                count).  The record is testable when pmin > min_redundancy; the error of d2 grows like 1 / pmin
 *   d2           u^T v with u = A^-1 z by both triangular solves and v = B^-1 z by its own Cholesky: to first order in the
 *                residuals, what dpgo_team_gate_candidates would return for this edge had it been taken out of the graph, the
 *                graph solved again and the edge offered as a candidate.  w = 0 is the gate itself, w = 1 the normalised
 *                residual test
 *   xi_loo       u / s elementwise: the innovation the edge would have shown had it been left out
 *   sigma_loo    diag(1 / s) sym(A^-1 C) diag(1 / s), stored (X + X^T) / 2, row-major: (sigma_rel^-1 - w W0)^-1, the relative
 *                covariance of the graph without the edge
 *   failure      an untestable record, or a non-positive pivot of B (garbage blocks): d2 = +inf and xi_loo = 0; an untestable
 *                record also sigma_loo = 0.  A record with d2 = +inf never passes
 * A record passes at quantile q when it is testable and sqrt(d2) <= dpgo_error_threshold_at_quantile(q, 6).
 * The blocks come from the covariance path `method` (max_block: DPGO_GATE_NESTED only), asked for the records' pairs (i, j),
 * each ordered pair once in order of first use; they stay on the device, one kernel forms the outputs, and xi (6 num), xi_loo
 * (6 num), d2, rho, pmin (num each) and, where it is not NULL, sigma_loo (36 num) come back.  Duplicated records give identical
 * bits; two calls give the same bits.  Refused with DPGO_ERR and a message that names the record, before any device work, every
 * output untouched: a NULL among the required arguments (all but sigma_loo); num <= 0; an unknown method; min_redundancy outside
 * (0, 1); an endpoint that is not a robot or pose of the team; i == j; kappa <= 0 or tau <= 0; a non-finite value; a weight that
 * is negative or not finite; R~ outside SO(3) by the 1e-8 rule of T.  Every refusal of the chosen covariance path carries over
 * with its own message; the outputs are then untouched and *res all zero.  *res: the path's own record.  Changes no solver
 * state.  Across teams: dpgo_team_audit_measurements_across below. */
int dpgo_team_audit_measurements(dpgo_team_t *t, const double *T, int method /* DPGO_GATE_* */, int max_block /* NESTED only */,
                                 int num, const dpgo_measurement_t *meas, double min_redundancy,
                                 double *xi /* 6 num */, double *xi_loo /* 6 num */, double *d2 /* num */,
                                 double *rho /* num */, double *pmin /* num */,
                                 double *sigma_loo /* 36 num or NULL */, dpgo_covariance_t *res);
/* ---- a set of candidates gated jointly, each given those already accepted (csrc/gate_joint.hip) ----
 * dpgo_team_gate_candidates tests every candidate against the Sigma of the estimate before any of them is taken.  This call
 * tests a batch of num = K candidates of one team against each other as well.  T, Sigma, the perturbation, R_ij, t_ij, J_i, J_j,
 * xi, the logarithm and Sigma_meas are those of dpgo_team_gate_candidates; candidate k joins the team poses i_k != j_k.  With
 * A the 6 K x 6 N matrix whose row block k holds J_i^k at pose i_k and J_j^k at pose j_k (nothing at pose 0), and R the block
 * diagonal of the Sigma_meas,k:
 *   M              A Sigma A^T + R, of order 6 K, row-major, bitwise symmetric; its diagonal block (k, k) is the S of the gate,
 *                  stored (G + G^T) / 2.  Positive definite because R is, duplicated candidates included
 *   conditional    given an accepted set A: xi_k|A = xi_k - M_kA M_AA^-1 xi_A, S_k|A = M_kk - M_kA M_AA^-1 M_Ak and
 *                  d2_k|A = xi_k|A^T S_k|A^-1 xi_k|A: to first order at this T the innovation and distance that
 *                  dpgo_team_gate_candidates would show for k after the candidates of A had been added to the graph and the
 *                  estimate updated.  A non-positive pivot gives +inf, which is never accepted
 *   order          thr = dpgo_error_threshold_at_quantile(quantile, 6).  DPGO_JOINT_GREEDY: at every step the remaining
 *                  candidate of smallest d2_k|A, the lower index on ties; accepted when d2 <= thr^2, else the call stops and
 *                  everything left is rejected.  DPGO_JOINT_GIVEN: k = 0 .. K - 1 in turn; accepted when d2_k|A <= thr^2,
 *                  else skipped with A left as it is
 *   outputs        xi (6 K), d2 (K): the marginal values, the definitions of dpgo_team_gate_candidates.  xi_cond (6 K),
 *                  d2_cond (K): the conditional values at the moment k was decided; for what the greedy rule rejects at its
 *                  stop, given the final A.  accept (K): 1 or 0.  rank (K): the position in the order of acceptance, -1 when
 *                  rejected.  *num_accepted = |A|.  *d2_joint: the sum of d2_cond over A in the order of acceptance, which is
 *                  xi_A^T M_AA^-1 xi_A.  *logdet_joint = log det M_AA.  The accepted set passes jointly when
 *                  sqrt(d2_joint) <= dpgo_error_threshold_at_quantile(quantile, 6 |A|).  M (36 K^2) may be NULL: it then
 *                  stays on the device.
 * The covariance path `method` (max_block: DPGO_GATE_NESTED only) is asked for every unordered pair of the distinct endpoint
 * poses, sorted; the blocks stay on the device.  One kernel forms xi, d2 and M, then one launch per step of a left-looking
 * block-pivoted Cholesky of M in the order the pivots are taken updates the conditional diagonal blocks, xi_cond and d2_cond
 * (M is only read; the stream order is the only synchronisation), and only the outputs come back.  No floating-point atomics:
 * duplicated candidates have identical marginal bits, and two calls give the same bits.
 * Refused with DPGO_ERR and a message before any device work, every output untouched: every refusal of
 * dpgo_team_gate_candidates for a call with xi and d2 (a NULL among the required arguments -- all but M --, num <= 0, an unknown
 * method, an endpoint that is not a robot or pose of the team, i == j, kappa <= 0 or tau <= 0, R~ outside SO(3)); an unknown
 * order; quantile outside (0, 1); and pair blocks (288 bytes each), M and the factor (288 K^2 bytes each) that do not fit the
 * free device memory, with the bytes named.  Every refusal of the chosen covariance path carries over with its own message;
 * the outputs are then untouched and *res all zero.  *res: the path's own record.  Changes no solver state.  There is no call
 * across teams. */
enum { DPGO_JOINT_GREEDY = 0, DPGO_JOINT_GIVEN = 1 };
int dpgo_team_gate_candidates_jointly(dpgo_team_t *t, const double *T, int method /* DPGO_GATE_* */, int max_block /* NESTED only */,
                                      int num, const dpgo_measurement_t *cand, int order /* DPGO_JOINT_* */, double quantile,
                                      double *xi /* 6 num */, double *d2 /* num */, double *xi_cond /* 6 num */,
                                      double *d2_cond /* num */, int *accept /* num */, int *rank /* num */, int *num_accepted,
                                      double *d2_joint, double *logdet_joint, double *M /* 36 num^2 or NULL */,
                                      dpgo_covariance_t *res);
/* ---- the estimate and its covariances updated for new closures, no re-solve (csrc/linear_update.hip) ----
 * The information-filter update (the EKF update in covariance form) of the whole trajectory for num = K closures of one team
 * taken together, at the estimate T with covariance Sigma: B = Sigma A^T, M = A B + R, dx = -B M^-1 xi,
 * Sigma' = Sigma - B M^-1 B^T, T' = T [+] dx.  (T', Sigma') is what a Gauss-Newton step from T on the graph with the closures
 * added gives, together with the Laplace covariance there (the matrix-inversion lemma: Sigma' = (H + A^T R^-1 A)^-1,
 * dx = -Sigma' A^T R^-1 xi).
 *   T, Sigma, the perturbation, J_i, J_j, xi with no Log-Jacobian, and Sigma_meas are those of dpgo_team_gate_candidates: the
 *                  perturbation is R_p <- R_p Exp(phi_p) in the body frame and t_p <- t_p + delta_p in the world frame, with
 *                  pose 0 fixed.  As in the gate, the weight field of a closure is not read.
 *   A and R        are those of dpgo_team_gate_candidates_jointly.
 *   endpoints      there are K closures on m distinct endpoint poses e_0 < ... < e_{m-1}.
 *   B_p,k          = Sigma_{p,i_k} J_i^k^T + Sigma_{p,j_k} J_j^k^T is a 6 x 6 block, for p = 0 ... N - 1.  Any Sigma block that
 *                  names pose 0 is zero, so B_0 = 0.
 *   M_kl           = J_i^k B_{i_k,l} + J_j^k B_{j_k,l} + delta_kl Sigma_meas,k.  The diagonal blocks are stored symmetrised.  M
 *                  is stored bitwise symmetric: one lane writes a block and its transpose.  The side from which a block is
 *                  formed is chosen by the endpoints, as in the joint gate.
 *   G              = M^-1 comes from the library's dense SPD inverse.
 *   z, U           z = G xi and U = B G.
 *   dx_p           = -B_p z (delta, 6 per pose: phi_p, then delta_p).
 *   xi_post        = R z, which equals xi + A dx.
 *   Sigma'_pp      = Sigma_pp - U_p B_p^T, formed in the upper triangle and mirrored (cov_diag, 36 per pose, row-major).
 *   Sigma'_pq      = Sigma_pq - U_p B_q^T for each requested pair (cov_pairs, 36 per pair of `pairs`, team pose indices).
 *   T'_p           = (R_p Exp(phi_p), t_p + delta_p), by Rodrigues, with the series below a threshold angle (T_new, the layout
 *                  of T).
 *   scalars        d2_joint = xi^T z; logdet_M from the Cholesky factor; logdet_R = sum_k -3 log(2 kappa_k) - 3 log tau_k.
 *                  The information the batch brings is (logdet_M - logdet_R) / 2.
 * Every sum runs in index order with fused multiply-adds and there are no floating-point atomics, so two calls give the same
 * bytes.  The covariance path `method` (max_block: DPGO_GATE_NESTED only) is asked for the rectangular set -- for each
 * endpoint rank a and each pose p the block Sigma_{p, e_a}, N m pair blocks -- and for the caller's pairs behind them; the
 * blocks, B, U, M and G stay on the device and only the outputs come back.
 * Refused with DPGO_ERR and a message that begins "linear_update:", every output untouched: a NULL among the required
 * arguments (all but pairs and cov_pairs when num_pairs is 0), num <= 0, num_pairs < 0, an unknown method, an endpoint that is
 * not a robot or pose of the team, i == j, kappa or tau not positive and finite, R~ outside SO(3) by the 1e-8 rule, a pair
 * index outside [0, N); the N m pair blocks (288 bytes each), B and U (288 N K bytes each) and the three matrices of order 6 K
 * that do not fit the free device memory, or more than INT32_MAX pair blocks, with the bytes named; a non-positive pivot in M,
 * with the pivot block named.  Every refusal of the chosen covariance path carries over with its own message; the outputs are
 * then untouched and *res all zero.  *res: the path's own record.  Changes no solver state.  One team: a split team calls
 * dpgo_team_linear_update_across. */
int dpgo_team_linear_update(dpgo_team_t *t, const double *T, int method /* DPGO_GATE_* */, int max_block, int num,
                            const dpgo_measurement_t *closures, int num_pairs, const int *pairs, double *T_new,
                            double *delta /* 6 N */, double *cov_diag /* 36 N */, double *cov_pairs, double *xi, double *xi_post,
                            double *scalars /* d2_joint, logdet_M, logdet_R */, dpgo_covariance_t *res);
/* ---- the estimate's covariance applied to vectors (csrc/covariance_apply.hip, covariance_apply.h) ----
 * X = Sigma V, which is the solve H_red X_red = V_red on the factors a covariance path holds, without a block of Sigma: the
 * covariance of any linear function of the trajectory, B = Sigma A^T for any set of measurements, a Newton step -Sigma g.
 *   V, X           6 N x num_cols, column-major with leading dimension 6 N.  Rows 6 p .. 6 p + 5 belong to team pose p in the
 *                  perturbation of dpgo_team_marginal_covariances: rotation first and in the body frame, translation in the
 *                  world frame, pose 0 fixed.  Sigma is the full 6 N x 6 N covariance whose rows and columns of pose 0 are
 *                  zero: the six rows of pose 0 of V are not read, those of X are zero bits.
 *   DPGO_GATE_NESTED  on the plan of dpgo_team_covariance_nested_plan at max_block, whether or not a robot is split (this call
 *                  does not delegate to the Schur path: an unsplit plan's blocks are the robots' interiors, and one robot
 *                  below max_block is one block with an empty separator).  With v_b the rows of block b, v_S the separator's:
 *                    u_b = C_b v_b (while C_b is live in its batch),  r_S = v_S - sum_b scatter_{N_b}(W_b^T v_b) (block order),
 *                    x_S = Sigma_SS r_S,  x_b = u_b - W_b x_S[N_b].
 *   DPGO_GATE_DENSE   X_red = G V_red, one product with the explicit inverse.
 *   DPGO_GATE_SCHUR   refused: DPGO_GATE_NESTED with no robot split has the Schur path's sets.
 * The products are 64 x 64 fp64 matrix-core tiles with row maps on the B operand and on C (a row r of a mapped operand is row
 * 6 pose[r / 6] + r mod 6 of V or X), so v_b is read straight out of V and x_b written straight into X.  Every element's sum
 * runs over k in index order; W_b^T v_b goes through a temporary that is subtracted from r_S one launch per block, in block
 * order; no floating-point atomics: two calls give the same bytes.
 * Bytes on the device beside what the path needs for zero pairs:
 *   dense    2 x 8 x 6 N x num_cols (V and X)
 *   nested   8 num_cols (12 N + 6 |S|) (V, X and r_S; x_S is written straight into X) + 8 num_cols K_b per block in the batch
 *            workspace (the temporaries; they are cut into batches with the rest of it) + 64 (3 blocks + 1) of product records
 *            + 4 (sum_b |N_b| + |S|) of row maps.
 * Refused with DPGO_ERR and a message that begins "covariance_apply:", before any device work: a NULL among t, T, V, X, res;
 * num_cols <= 0; an unknown method; DPGO_GATE_SCHUR; V and X that do not fit the free device memory (decided before V is
 * read), with the bytes named; an entry of V outside pose 0's rows that is not finite.  The refusals of the chosen
 * covariance path (T outside SE(3), a weighted graph not joined to pose 0, its bytes with the apply's beside them, a
 * non-positive pivot) carry over in their own words.  A refused call leaves X untouched and *res all zero.  *res: the path's
 * record.  Changes no solver state.  One team: all robots local and INITIALIZED (a split team: the call below). */
int dpgo_team_covariance_apply(dpgo_team_t *t, const double *T, int method /* DPGO_GATE_* */, int max_block /* NESTED only */,
                               int num_cols, const double *V, double *X, dpgo_covariance_t *res);
/* dpgo_team_linear_update on that solve: the same arguments, outputs and refusals, but the covariance path is asked for the
 * caller's own pairs alone (the diagonal blocks are staged anyway) and forms B = Sigma A^T itself, from V = A^T written on the
 * device (J_i^T and J_j^T of closure k in column block k at the rows of its endpoints, pose 0's rows zero).  B is not formed
 * from N m extracted blocks; M onward is computed as in dpgo_team_linear_update on that B.  The sums of B come in another
 * order, so the outputs agree with dpgo_team_linear_update's to round-off, not bitwise; two calls give the same bytes.
 * DPGO_GATE_SCHUR is refused (DPGO_GATE_NESTED with no robot split has the Schur path's sets).  Bytes: the caller's pair
 * blocks, U (288 N K), the three matrices of order 6 K, and dpgo_team_covariance_apply's for num_cols = 6 K. */
int dpgo_team_linear_update_solved(dpgo_team_t *t, const double *T, int method /* DPGO_GATE_* */, int max_block, int num,
                                   const dpgo_measurement_t *closures, int num_pairs, const int *pairs, double *T_new,
                                   double *delta /* 6 N */, double *cov_diag /* 36 N */, double *cov_pairs, double *xi,
                                   double *xi_post, double *scalars /* d2_joint, logdet_M, logdet_R */, dpgo_covariance_t *res);
/* ---- measurements removed or down-weighted in the estimate and its covariances, no re-solve (csrc/linear_removal.hip;
 * DESIGN.md 5l) ----
 * The counterpart of dpgo_team_linear_update for weight taken OUT of the graph.  num = K records of one team are in the
 * weighted graph, record k at records[k].weight = w_k > 0 (taken on trust, as in dpgo_team_audit_measurements), and T is a
 * minimum of that graph.  Their weights drop to new_weight[k] = w'_k with 0 <= w'_k < w_k (NULL: all 0, the edges removed).
 * With dw_k = w_k - w'_k, R_k = Sigma_meas,k / dw_k, A of dpgo_team_gate_candidates_jointly and B = Sigma A^T:
 *   H' = H - A^T R^-1 A,  N = R - A B (of order 6 K: the covariance of the post-fit residuals of the set),
 *   Sigma' = Sigma + B N^-1 B^T,  dx = +B N^-1 xi,  T' = T [+] dx (the retraction of dpgo_team_linear_update),
 *   xi_loo = xi + A dx = R N^-1 xi: the innovations the K records show against the graph without that weight,
 *   d2_joint = xi^T N^-1 xi: twice the drop of the optimal cost, f'(T') = f(T) - d2_joint / 2,
 *   log det H' - log det H = logdet_N - logdet_R, so the information lost is (logdet_R - logdet_N) / 2 >= 0.
 * At K = 1 xi_loo is the audit's; at K = 1, w = 1, w' = 0 d2_joint is the audit's d2, the classical normalised residual; for
 * K > 1 at full weight d2_joint is the joint normalised-residual statistic, chi^2 with 6 K degrees of freedom when the set is
 * sound.  With a fractional dw d2_joint is still the cost the removed weight accounted for, but it is NOT the audit's d2.
 * The work is whitened: s_k = (sqrt(2 kappa_k dw_k) x 3, sqrt(tau_k dw_k) x 3), D = diag(s), B~ = B D, xi~ = D xi and
 * N~ = D N D = I - (D A) B~, stored bitwise symmetric, whose pivots lie in (0, 1] and whose diagonal block is the audit's
 * I - dw C (several records may join one ordered pair of poses with noise that is not proportional: no block off the
 * diagonal is symmetrised); logdet_N = log det N~ + logdet_R, logdet_R = sum_k -3 log(2 kappa_k) - 3 log tau_k - 6 log dw_k.
 *   outputs        T_new, delta (6 N), cov_diag (36 N, bitwise symmetric), cov_pairs (36 per pair of `pairs`): as in
 *                  dpgo_team_linear_update; xi, xi_loo (6 K); pivot_min (K): the smallest Cholesky pivot of record k's own
 *                  block of N~, the audit's pivot_min at weight dw_k; scalars: d2_joint, logdet_N, logdet_R and
 *                  pivot_min_joint, the smallest pivot of the Cholesky factor of N~.  The errors of every output grow like
 *                  1 / pivot_min_joint.  fixed_weight and is_known_inlier are ignored.
 * A set whose removal leaves the graph without another way to some relative pose (a bridge; two edges that form a cut) makes
 * N~ singular.  Refused behind the covariance path, in this order, every output untouched and *res all zero: a record whose
 * pivot_min is not above min_redundancy, the record named; a non-positive pivot of N~, the pivot block named; a
 * pivot_min_joint not above min_redundancy ("the records together leave no redundancy").
 * Refused before any device work with a message that begins "linear_removal:", every output untouched: every refusal of
 * dpgo_team_linear_update; a weight that is not finite and positive; a new_weight that is negative, not finite or not below
 * the weight; min_redundancy outside (0, 1).  Every refusal of the chosen covariance path carries over with its own message.
 * Every sum runs in index order with fused multiply-adds and there are no floating-point atomics: two calls give the same
 * bytes.  Changes no solver state, the team's weights included.  There is no call across teams. */
int dpgo_team_linear_removal(dpgo_team_t *t, const double *T, int method /* DPGO_GATE_* */, int max_block, int num,
                             const dpgo_measurement_t *records, const double *new_weight /* num, or NULL: all 0 */,
                             double min_redundancy, int num_pairs, const int *pairs, double *T_new, double *delta /* 6 N */,
                             double *cov_diag /* 36 N */, double *cov_pairs, double *xi, double *xi_loo, double *pivot_min /* num */,
                             double *scalars /* d2_joint, logdet_N, logdet_R, pivot_min_joint */, dpgo_covariance_t *res);
/* ---- a trajectory refined to a critical point of the SE(3) cost by Newton steps on Sigma (csrc/refine.hip) ----
 * The covariance calls take Sigma = H_red^-1 for the Laplace approximation at a minimum; this call puts T on one.  With
 * g(xi) = f(T [+] xi), the perturbation of dpgo_team_marginal_covariances and pose 0 held fixed, every iteration forms on the
 * device the gradient g = J^T vec(T Q) (six numbers per pose), the cost f as the sum of the measurements' terms and |g|_inf,
 * stops when |g|_inf <= grad_tol, else runs ONE covariance path (method, max_block as in dpgo_team_covariance_apply) whose
 * right-hand side is g, so that X = Sigma g comes from the path's factors, writes the `ladder` trial trajectories
 * T [+] (-2^-l X), l = 0 .. ladder - 1, evaluates their costs in one pass and takes the first l with
 *   f_l <= f - armijo 2^-l g^T X + eps_f,   eps_f = (24 + ceil(measurements / 256)) 2^-53 f
 * (the rounding of the cost's sum, whose terms are not negative).  A polisher, not a solver: H_red must be positive definite
 * at every iterate, and there is no Levenberg shift.
 * status: DPGO_REFINE_CONVERGED |g|_inf <= grad_tol;  DPGO_REFINE_MAX_ITERS;  DPGO_REFINE_INDEFINITE a pivot of the path was
 * not positive at a later iterate: T_out is the last good iterate;  DPGO_REFINE_NO_DESCENT no entry of the ladder passed:
 * T_out is the iterate it started from.
 * T_out: 12 N doubles (may be T).  A T that already meets grad_tol comes back bit for bit with iterations = 0.
 * history: 5 (max_iters + 1) doubles, row k = [f, |g|_inf at iterate k; alpha, decrement g^T Sigma g, the path's smallest pivot
 * of the step taken from it]; what was not computed is NaN.  *res: the record of the last path that succeeded (zero: none ran).
 * Refused with DPGO_ERR and a message that begins "refine:", before any device work, T_out, history untouched and *out, *res
 * zero: a NULL argument; max_iters < 0; ladder outside [1, 32]; grad_tol not positive; armijo outside (0, 1); an unknown
 * method; DPGO_GATE_SCHUR (in the words of dpgo_team_covariance_apply); a pose of T outside SE(3).  A pivot that is not positive
 * at the input T is refused with the path's message behind "refine: "; the other refusals of the path (its bytes, a graph not
 * joined to pose 0) carry over in their own words.  Bytes on the device beside the path's (one column of V and X): 8 x 12 N
 * (ladder + 2) + 8 x 6 N + 128 per measurement.  Fixed-order sums, no floating-point atomics: two calls give the same bytes.
 * Changes no solver state.  One team only: all robots local and INITIALIZED. */
#define DPGO_REFINE_CONVERGED 0
#define DPGO_REFINE_MAX_ITERS 1
#define DPGO_REFINE_INDEFINITE 2
#define DPGO_REFINE_NO_DESCENT 3
typedef struct {
  int status;     /* DPGO_REFINE_* */
  int iterations; /* steps taken */
  double f0, f;   /* the cost at the input and at T_out */
  double grad_inf0, grad_inf;
} dpgo_refine_t;
int dpgo_team_refine(dpgo_team_t *t, const double *T, int method /* DPGO_GATE_* */, int max_block /* NESTED only */, int max_iters,
                     double grad_tol, double armijo, int ladder, double *T_out /* 12 N */, double *history /* 5 (max_iters + 1) */,
                     dpgo_refine_t *out, dpgo_covariance_t *res);
/* ---- the most informative candidate closures under a budget (csrc/select.hip) ----
 * Asked before anything is measured: of num = P proposed pose pairs of one team, which `budget` would tighten the estimate
 * most.  T, Sigma, the perturbation, J_i, J_j and Sigma_meas are those of dpgo_team_gate_candidates, A, R and
 * M = A Sigma A^T + R those of dpgo_team_gate_candidates_jointly.  The Jacobians depend on T alone, so of a record only the two
 * endpoints and the expected noise (kappa, tau) are read: R~, t~ and weight are not.
 *   conditional    given a selected set A: S_k|A = M_kk - M_kA M_AA^-1 M_Ak and
 *                  gain_k|A = (log det S_k|A - log det Sigma_meas,k) / 2, log det Sigma_meas,k = -3 log(2 kappa_k) - 3 log tau_k:
 *                  the mutual information between measurement k and the trajectory once A has been measured, which is
 *                  (log det H' - log det H) / 2 for adding k to the graph that already holds A.  A non-positive pivot gives
 *                  -inf, which is never taken
 *   order          DPGO_JOINT_GREEDY: at every step the open candidate of largest gain_k|A, the lower index on ties;
 *                  DPGO_JOINT_GIVEN: k = 0 .. budget - 1 in turn.  Either way the candidate is taken while gain > min_gain
 *                  (-INFINITY: no threshold) and fewer than `budget` are selected; otherwise the call stops.  The set function
 *                  is monotone submodular, so the greedy value is at least (1 - 1 / e) of the best set of the same size
 *   outputs        gain (P): the marginal gain_k|{}.  gain_cond (P): the gain at the moment k was selected; for the rest, given
 *                  the final set: what is still on the table.  rank (P): the position in the order of selection, -1 when not
 *                  selected.  *num_selected = |A|.  *gain_total: the sum of the gains at selection in selection order, which
 *                  is (log det M_AA - log det R_A) / 2, the information_gain of dpgo_team_linear_update for the same set.
 *                  *logdet_joint = log det M_AA.
 * The covariance path `method` (max_block: DPGO_GATE_NESTED only) is asked for every unordered pair of the distinct endpoint
 * poses, sorted; the blocks stay on the device.  One kernel forms the diagonal blocks and the marginal gains, then one launch
 * per selected candidate -- `budget` launches, not P -- forms the pivot's block column of M on the fly, bit for bit what
 * dpgo_team_gate_candidates_jointly stores there, and updates the conditional blocks and gains by a left-looking block-pivoted
 * Cholesky whose factor has budget x P blocks of 288 bytes.  M is never formed.  Every sum runs in index order with fused
 * multiply-adds and there are no atomics: two calls give the same bytes.
 * Refused with DPGO_ERR and a message that begins "select_candidates:" before any device work, every output untouched: a NULL
 * argument, num <= 0, budget outside [1, num], an unknown method or order, a NaN min_gain, an endpoint that is not a robot or pose
 * of the team, i == j, kappa or tau not positive and finite; and pair blocks, factor and working arrays that do not fit the free
 * device memory, or more than INT32_MAX pair blocks, with the bytes named.  Every refusal of the chosen covariance path
 * carries over with its own message; the outputs are then untouched and *res all zero.  *res: the path's own record.  Changes no
 * solver state.  There is no call across teams. */
int dpgo_team_select_candidates(dpgo_team_t *t, const double *T, int method /* DPGO_GATE_* */, int max_block /* NESTED only */,
                                int num, const dpgo_measurement_t *cand, int order /* DPGO_JOINT_* */, int budget, double min_gain,
                                double *gain /* num */, double *gain_cond /* num */, int *rank /* num */, int *num_selected,
                                double *gain_total, double *logdet_joint, dpgo_covariance_t *res);
/* ---- the pairwise-consistent set of candidates between two teams (csrc/consistency.hip, csrc/max_clique.cpp) ----
 * Pairwise consistency maximisation (Mangelson et al. 2018) for loop closures between two teams that are NOT joined yet, each
 * with a connected weighted graph of its own (they may be the same handle), trajectories T_a and T_b in their own gauges.
 * Candidate k is a dpgo_measurement_t whose (r1, p1) names a pose i_k of team a and (r2, p2) a pose j_k of team b, with R~
 * (row-major), t~, kappa, tau; weight and the flags are ignored.  Z_k ~ (T^a_{i_k})^-1 G T^b_{j_k} for one unknown G common
 * to the true candidates.  For k < l, every pose perturbed as R <- R Exp(phi), t <- t + delta:
 *   segments     A_kl = (T^a_{i_l})^-1 T^a_{i_k},  B_kl = (T^b_{j_k})^-1 T^b_{j_l}, with the covariances sigma_rel(i_l, i_k) and
 *                sigma_rel(j_k, j_l) of dpgo_team_gate_candidates from each team's own covariance path `method` (bit for bit
 *                those blocks); a segment whose two poses coincide is the identity with zero covariance
 *   loop         E_kl = Z_l^-1 A_kl Z_k B_kl, the identity when both candidates are true;  xi = (Log(R_E)v, t_E), the
 *                logarithm of the gate
 *   covariance   S = J_A Sigma_A J_A^T + J_B Sigma_B J_B^T + J_k N_k J_k^T + J_l N_l J_l^T, symmetrised, N = diag(I / (2 kappa),
 *                I / tau), J the Jacobians of the four-factor product.  The correlation between the two segments is dropped:
 *                zero for separate teams; PCM's standing approximation when a and b are the same team
 *   distance     d2[k, l] = d2[l, k] = xi^T S^-1 xi by a 6 x 6 Cholesky (a non-positive pivot gives +inf), d2[k, k] = 0; both
 *                triangles are bitwise equal.  k and l are consistent when d2 <= thr^2, thr =
 *                dpgo_error_threshold_at_quantile(quantile, 6)
 * d2 (num x num, row-major) and adj (num rows of W = ceil(num / 64) words, bit b of word w of row k: k and 64 w + b are
 * consistent; no bit on the diagonal or at or beyond num) may each be NULL.  members receives the ascending indices of a
 * maximum clique of the consistency graph (room for num), *size their number and *proven whether the search finished
 * (dpgo_max_clique with max_nodes).  *res_a / *res_b: each path's own record; a team none of whose segments joins two
 * different poses (num = 1, for one) is not asked, and its record is all zero.  Two calls give the same bits.
 * Refused with DPGO_ERR and a message that names the candidate, before any device work and with every output untouched:
 * num <= 0, a NULL argument, an unknown method, quantile outside (0, 1), max_nodes < 0, teams on different devices, an endpoint
 * that is not a robot or pose of its team, kappa <= 0 or tau <= 0, a non-finite entry, R~ outside SO(3) by the 1e-8 rule, and
 * staged bytes (384 per segment, 12 num^2 and small change) that do not fit the free device memory.  Every refusal of the
 * covariance path of either team carries over with its own message, the outputs untouched.  Changes no solver state of either
 * team.  There is no call across processes. */
int dpgo_team_pairwise_consistency(dpgo_team_t *a, const double *T_a, dpgo_team_t *b, const double *T_b,
                                   int method /* DPGO_GATE_* */, int max_block /* NESTED only */, int num,
                                   const dpgo_measurement_t *cand, double quantile, long long max_nodes,
                                   double *d2 /* num^2 or NULL */, uint64_t *adj /* num W or NULL */, int *members, int *size,
                                   int *proven, dpgo_covariance_t *res_a, dpgo_covariance_t *res_b);
/* A maximum clique of the graph on K vertices whose adjacency matrix is adj: K rows of W = ceil(K / 64) words, bit b of word w
 * of row k set when k and 64 w + b are joined.  Host only.  Exact branch and bound on bitsets with a greedy-colouring bound;
 * the vertices are ordered by degeneracy and the search is seeded by a greedy clique; a larger clique replaces the incumbent
 * only when strictly larger, so the same input gives the same members.  After max_nodes search nodes (0: no limit) it stops
 * and returns the incumbent with *proven = 0, else *proven = 1.  members (room for K): ascending.  Refused: K <= 0, a NULL
 * argument, max_nodes < 0, a matrix that is not symmetric, a set diagonal bit, a set bit at or beyond K. */
int dpgo_max_clique(int K, const uint64_t *adj, long long max_nodes, int *members, int *size, int *proven);
/* ---- certificate and rounding across teams (csrc/certify_across.hip) ----
 * A participant is one team that holds a subset of the robots; owner_rank_of_robot[num_robots] says which participant holds
 * each (the meaning of dpgo_team_attach_comm).  The library does not own the transport: it calls the two functions below,
 * host memory in and out, on the calling thread.  Every participant enters the same calls in the same order.
 *   allgather: every participant passes n doubles; out receives world * n doubles in rank order.
 *   exchange:  send_counts[p] doubles to participant p (send packed in rank order), recv_counts[p] from p into recv (packed
 *              in rank order); both ends know the counts in advance, zero counts included.
 * Both return 0 on success.  A transport that fails or times out makes the calling participant return DPGO_ERR. */
typedef struct {
  void *ctx;
  int rank, world; /* this participant, number of participants */
  int (*allgather)(void *ctx, const double *in, int n, double *out);
  int (*exchange)(void *ctx, const double *send, const long long *send_counts, double *recv, const long long *recv_counts);
} dpgo_transport_t;
/* The three calls of the single team over a split problem.  V / out / v / T hold this team's columns (poses) in team order;
 * every scalar output is bitwise identical on every participant, and one participant holding every robot reproduces
 * dpgo_team_certificate_apply / _certify / _round bit for bit.  The first allgather carries an agreement record (block,
 * r, num_robots, flags, eta, tol, max_iters, the owner table, this team's robots); a disagreement, a robot held by no or two
 * participants, an uninitialised robot anywhere, a participant without robots, or a local failure later on (allocation,
 * device error) makes every participant return DPGO_ERR at the next allgather, with a message that names the rank.
 * Transport calls: certify 2 exchanges + 8 allgathers per LOBPCG iteration that continues (2 + 5 in the last); the set-up
 * and the closing status add a fixed few.  Changes no solver state. */
int dpgo_team_certificate_apply_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, int K,
                                       const double *V, double *out);
int dpgo_team_certify_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, double eta,
                             double tol, int max_iters, int block, int flags, dpgo_certificate_t *out, double *v);
/* anchored at robot 0's first pose; DPGO_ROUND_REFINE_TRANSLATIONS: every participant gathers the owned measurements and
 * the rounded rotations of all and solves the same translation problem (global numbering: robots by id, then poses), then
 * keeps its own poses' translations */
int dpgo_team_round_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, int flags, double *T,
                           dpgo_rounding_t *out);
/* dpgo_team_marginal_covariances over a split team (csrc/covariance_schur.hip): the Schur path is its only
 * method, flags = DPGO_COV_SCHUR.  T and cov_diag: this team's poses in team order.  pairs: poses of the whole problem
 * (robots by id, then poses; pose 0, the fixed one, is robot 0's first pose), the same list on every participant; cov_pairs is
 * complete on every participant.  The agreement record of the calls above also carries num_pairs and a hash of the pair list; a
 * participant whose arguments are invalid (a T outside SE(3), flags) makes every participant refuse.  Then three allgathers:
 * the robots' sizes; per robot its public frames, its diagonal block of the Schur complement, the statistics of its factor and
 * the blocks of H_SS below the diagonal in the rows it holds, together with a failure record (a non-positive pivot with robot,
 * pose and row; a device that is too small); the pair blocks a participant owns and the rows W_a[i,:] of pairs between two
 * robots' interiors.  Every participant inverts the same Schur complement itself.  Every participant returns DPGO_ERR with a
 * message that names the failing rank, and a refused call leaves cov_diag / cov_pairs untouched everywhere.  Every block, log
 * det and pivot equals the single team's DPGO_COV_SCHUR call bit for bit, whatever the split, and the scalars of *res are
 * identical on every participant (seconds_*: this participant's).  The connectivity of the weighted graph is NOT checked
 * here (no participant sees all edges): a graph cut in two ends in a non-positive pivot. */
int dpgo_team_marginal_covariances_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot,
                                          const double *T, int flags, int num_pairs, const int *pairs, double *cov_diag,
                                          double *cov_pairs, dpgo_covariance_t *res);
/* dpgo_team_gate_candidates and dpgo_team_audit_measurements over a split team (csrc/gate.hip, csrc/audit.hip; DESIGN.md 5f,
 * 5h, "across teams"): the step behind dpgo_team_marginal_covariances_across, whose Schur path is the only method.  T: this
 * team's poses in team order.  The records are the same on every participant and their (r1, p1) -> (r2, p2) may name any
 * robot of the problem: a closure between a robot held here and one held elsewhere is the normal case.  All num outputs are
 * complete and identical on every participant, and every bit equals the single team's DPGO_GATE_SCHUR call on the same T and
 * records, whatever the split.  The agreement record carries num and a hash of the records' endpoint ids and their 14 (the
 * audit: 15, with the weight) doubles, of the outputs requested and of min_redundancy: a list that differs on one
 * participant is refused everywhere ("the number of records", "the record list").  The path is asked for the records' pairs
 * of GLOBAL poses, each ordered pair once in order of first use.  Behind its three allgathers comes a fourth, D: per endpoint
 * of the records, sorted by global pose, the 12 doubles of T and the 36 of Sigma_ii from the participant that holds it, zeros
 * from everyone else.  Every participant then holds compact tables (endpoint poses, their diagonal blocks, the pair blocks),
 * runs the single team's kernel on all num records itself, and copies back the per-record outputs: nothing is broadcast.
 * Exactly one allgather more than dpgo_team_marginal_covariances_across with the same pairs.
 * The refusals of the single-team call keep their words (NULL arguments, num <= 0, xi and d2 not together, i == j, kappa <= 0
 * or tau <= 0, a weight that is negative or not finite, R~ outside SO(3), min_redundancy outside (0, 1)); they are decided on
 * the host before any device work, and because the others must not be left waiting they travel in the agreement record: the
 * participant whose argument it was reports the words above, the others "rank q: invalid arguments".  An endpoint outside
 * the problem is refused behind the agreement, in the same words everywhere.  Every refusal of
 * dpgo_team_marginal_covariances_across passes through with its own message.  A refused call leaves every output untouched on
 * every participant and *res all zero.  Changes no solver state. */
int dpgo_team_gate_candidates_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, const double *T,
                                     int num, const dpgo_measurement_t *cand, double *xi /* 6 num or NULL */,
                                     double *d2 /* num or NULL */, double *sigma_rel /* 36 num or NULL */, dpgo_covariance_t *res);
int dpgo_team_audit_measurements_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, const double *T,
                                        int num, const dpgo_measurement_t *meas, double min_redundancy, double *xi /* 6 num */,
                                        double *xi_loo /* 6 num */, double *d2 /* num */, double *rho /* num */, double *pmin /* num */,
                                        double *sigma_loo /* 36 num or NULL */, dpgo_covariance_t *res);
/* dpgo_team_covariance_apply over a team split across participants, on the path of dpgo_team_marginal_covariances_across,
 * whose fixed pose, global numbering and robot-wise sets it has; there is no method: the Schur path is the only one.  Every
 * participant calls.
 *   T              this team's poses in team order, 12 N_loc doubles.
 *   V, X           6 N_loc x num_cols, column-major with leading dimension 6 N_loc; rows 6 p .. 6 p + 5 belong to team pose p.
 *                  On the participant that holds robot 0 the rows of V of the problem's pose 0 are not read and those of X
 *                  are zero bits.  num_cols is the same on every participant.
 * For the robots a held here, in id order, with I_a the interior and S_a the public poses, v_a = V[I_a]:
 *     u_a = C_a v_a (while C_a is live in the robot's step),  r_a = v_{S_a} - W_a^T v_a (no interior pose: r_a = v_{S_a});
 *     r_S = the r_a of every robot of the problem at the robot's place in the global separator (gathered);
 *     x_S = Sigma_SS r_S (on every participant, from identical bytes),  x_a = u_a - W_a x_S[S_a],  X[I_a] = x_a,  X[S_a] = x_S[S_a].
 * The products are the tiles of dpgo_team_covariance_apply with their row maps; one more kernel forms r_a out of V into the
 * robot's rows of r_S and copies x_S[S_a] into X.  No floating-point atomics.  The r_a ride in the record of the path's third
 * allgather (the owned pair blocks, empty here): the call makes exactly the transport calls of
 * dpgo_team_marginal_covariances_across with zero pairs.  Every row of X is the same bits whatever the split, one participant
 * that holds every robot included, and two calls give the same bytes.  It is not bitwise DPGO_GATE_NESTED of the single
 * team's call: the interior inverses take another route.
 * Bytes on the device beside what the path needs for zero pairs: 8 num_cols (12 N_loc + 12 |S| + max_a K_a) (V and X; r_S and
 * x_S on the separator of the whole problem; the temporary W_a^T v_a, K_a = 6 |S_a| over the robots here) + 64 (3 robots + 1)
 * of product records + 4 per public pose here of row maps.  A request above the free memory is refused before V and X are
 * allocated, with the bytes named; the other participants read "rank q: the Schur path does not fit its device".  V and X
 * alone above the free memory are decided before V is read.
 * Refused with DPGO_ERR and a message that begins "covariance_apply_across:", before any device work: a NULL among t, tr,
 * owner_rank_of_robot, T, V, X, res; num_cols <= 0; an entry of V outside pose 0's rows that is not finite (the row, team pose
 * and column named).  Such a refusal travels in the agreement record: its participant reads its own words, the others "rank
 * q: invalid arguments"; a num_cols that differs is refused on all of them, naming "num_cols".  The refusals of
 * dpgo_team_marginal_covariances_across (T outside SE(3), a pivot, memory, measurement sets that differ) carry over in their
 * own words.  A refused call leaves X untouched and *res all zero on every participant, and the transport usable.  *res: the
 * path's record, identical on every participant.  Changes no solver state. */
int dpgo_team_covariance_apply_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot,
                                      const double *T, int num_cols, const double *V, double *X, dpgo_covariance_t *res);
/* ---- dpgo_team_linear_update over a team split across participants (csrc/linear_update.hip; DESIGN.md 5j, "Across teams") ----
 * Collective: every participant calls it with its own team, the same owner table, the same closures and the same pairs.  The
 * closures' (r1, p1) -> (r2, p2) may name any robot of the problem; `pairs` holds poses of the whole problem in the global
 * numbering (robots by id, then poses; pose 0 is robot 0's first).  T, T_new, delta (6 N_loc) and cov_diag (36 N_loc) are this
 * participant's poses in team order; cov_pairs, xi, xi_post, scalars and the scalars of *res are complete and identical on every
 * participant.  The definitions are dpgo_team_linear_update's: B = Sigma A^T, M = A B + R, G = M^-1, z = G xi, U = B G,
 * dx = -B z, Sigma' = Sigma - U B^T, T' = T [+] dx, xi_post = R z; the fixed pose is the PROBLEM's pose 0.
 * With C the distinct poses among the closures' endpoints and the pairs, sorted by global pose:
 *   allgather E    12 doubles of T per compact pose from its holder, zeros from everyone else: the table T_C, identical bytes
 *                  everywhere, from which one lane per closure forms J_i, J_j and writes J^T into column block k of V at the rows
 *                  of the endpoints that are this participant's (pose 0's rows stay zero);
 *   the path       dpgo_team_marginal_covariances_across with `pairs` and that V: B_loc = Sigma V on this participant's rows, the
 *                  local diagonal blocks and the pair blocks;
 *   allgather F    6 x 6 K doubles of B per compact pose from its holder alone, padded to the participant that holds most:
 *                  B_C (6 C x 6 K);
 *   order 6 K      M, its inverse and log det, z, the figures and U_C = B_C G on every participant from identical bytes, by the
 *                  kernels of dpgo_team_linear_update with N := C; U_loc = B_loc G and the reduction over this participant's
 *                  poses; Sigma'_pq = Sigma_pq - U_p B_q^T on the compact tables.
 * Transport calls: those of dpgo_team_marginal_covariances_across with the same pairs and two more allgathers (E and F),
 * whatever K, the pairs and the split; the agreement (num, num_pairs and a hash of the records and the pairs) rides in the
 * path's own record.  For a given problem, T, closures and pairs every output is the same bits whatever the split, one
 * participant that holds every robot included, and two calls give the same bytes; no floating-point atomics.  It is not bitwise
 * the single team's call.
 * Refused with DPGO_ERR and a message that begins "linear_update_across:".  Decided on the host before any device work and
 * carried in the agreement record (its participant reads its own words, the others "rank q: invalid arguments"): a NULL among
 * the required arguments, num <= 0, num_pairs < 0, a closure that joins a pose to itself, kappa or tau not positive and finite,
 * R~ outside SO(3), and V, X, U (288 N_loc K bytes each), the three matrices of order 6 K and the compact tables (at most
 * 2 K + 2 num_pairs poses) above the free device memory, with the bytes named, decided before a record is read.  A NULL t or tr
 * returns at once.  A num or a record or pair list that differs between participants is refused on all of them ("the number of
 * records", "the record list": the hash covers the pairs, so a num_pairs that differs reads as the latter); an endpoint or a pair pose outside the problem in the same words everywhere.  A
 * non-positive pivot of M is refused with the pivot block named, the same on every participant.  The refusals of
 * dpgo_team_marginal_covariances_across (T outside SE(3), a pivot, memory, measurement sets that differ) carry over in their own
 * words.  A refused call leaves every output untouched and *res all zero on every participant, and the transport usable.
 * Changes no solver state. */
int dpgo_team_linear_update_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot,
                                   const double *T /* 12 N_loc */, int num, const dpgo_measurement_t *closures, int num_pairs,
                                   const int *pairs /* GLOBAL poses */, double *T_new /* 12 N_loc */, double *delta /* 6 N_loc */,
                                   double *cov_diag /* 36 N_loc */, double *cov_pairs /* 36 num_pairs */, double *xi,
                                   double *xi_post /* 6 num each */, double *scalars /* d2_joint, logdet_M, logdet_R */,
                                   dpgo_covariance_t *res);
/* ---- dpgo_team_refine over a team split across participants (csrc/refine.hip; DESIGN.md 5n, "Across teams") ----
 * Collective: every participant calls it with its own team and the same owner table, max_iters, grad_tol, armijo and ladder.
 * T, T_out: this participant's 12 N_loc doubles in team order.  history, *out, *res and the status codes are those of
 * dpgo_team_refine and are identical on every participant.  There is no method: a split team has the Schur path alone.
 * The fixed pose is the PROBLEM's pose 0, robot 0's first: on a participant that does not hold robot 0 every local pose moves.
 * Per iterate: E = T Q from the across operator at K = 3 (one exchange of the T halo), the gradient on the local poses, and the
 * cost summed ROBOT BY ROBOT -- a measurement belongs to its own robot, a shared one to the lower robot id, whose copy owns the
 * weight; a robot's terms are summed in the order of its own list, 256 to a workgroup, the workgroups in index order -- so a
 * robot's total depends on nothing but the robot.  The totals are allgathered and added on the host in robot order from 0;
 * |g|_inf is the largest of the participants' (a NaN wins).  The step is X = Sigma g from dpgo_team_covariance_apply_across'
 * path with one column; the rows of X of the remote end points of this participant's shared measurements are read out of
 * x_S = Sigma_SS r_S, which is whole on every participant, so the trial trajectories need no further exchange.  The ladder's
 * costs and g^T X are summed by robot in the same way; the first l with
 *   f_l <= f - armijo 2^-l g^T X + eps_f,   eps_f = (24 + max_a ceil(E_a / 256) + R) 2^-53 f
 * is taken (R robots in the problem, E_a the measurements robot a owns), by every participant from the same bits.
 * Transport calls for k steps: the two agreement allgathers and the closing one; per evaluated iterate (k + 1 of them) one
 * exchange and one allgather; per step the calls of dpgo_team_marginal_covariances_across with zero pairs and one allgather.
 * For a given problem and T every pose of T_out, every entry of history and every scalar are the same bits whatever the split,
 * one participant that holds every robot included; two calls give the same bytes.  It is not bitwise dpgo_team_refine of the
 * joined team (the step comes from the Schur path's sets, the sums run by robot).  A T that meets grad_tol comes back bit for bit
 * with iterations = 0 and no path run.
 * Refused with DPGO_ERR and a message that begins "refine_across:": a NULL argument; max_iters < 0; ladder outside [1, 32];
 * grad_tol not positive; armijo outside (0, 1); a pose of T outside SE(3).  Such a refusal travels in the agreement record: its
 * participant reads its own words, the others "rank q: invalid arguments"; a max_iters, ladder, grad_tol or armijo that differs
 * is refused on all of them ("the participants disagree on ...").  A pivot that is not positive at the input T refuses every
 * participant with the path's message behind "refine: "; at a later iterate the status is DPGO_REFINE_INDEFINITE everywhere.
 * The path's other refusals pass through.  A refused call leaves T_out and history untouched and *out, *res zero, and the
 * transport usable.  Bytes on the device beside the path's, with H the halo poses here: 8 x 12 (N_loc + H) (ladder + 1) +
 * 8 x 6 (2 N_loc + H) + 8 x 12 N_loc + 128 per measurement owned here.  No floating-point atomics.  Changes no solver state. */
int dpgo_team_refine_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, const double *T,
                            int max_iters, double grad_tol, double armijo, int ladder, double *T_out /* 12 N_loc */,
                            double *history /* 5 (max_iters + 1) */, dpgo_refine_t *out, dpgo_covariance_t *res);
/* the synchronous schedule with the leader's decisions (src/PGOAgentROS.cpp:129-220): iterate; after every iteration
 * in which the leader optimized: stop if shouldTerminate() (:208), else an UPDATE_WEIGHT round if
 * shouldUpdateMeasurementWeights() (:210), else pass the token (:213).  Returns the number of iterations executed
 * (<= max_iters) or <0; *terminated / *weight_rounds may be NULL. */
int dpgo_team_run_schedule(dpgo_team_t *t, int max_iters, int *terminated, int *weight_rounds);
/* per-iteration log (createIterationLog / logIteration / logString, src/PGOAgentROS.cpp:853-909): one CSV per
 * local robot, <directory>/dpgo_log_robot<id>.csv, the reference's header and column order -- robot_id, cluster_id,
 * num_active_robots, iteration, num_poses, bytes_received, iter_time_sec, total_time_sec, rel_change -- followed by
 * global_cost; a row after every block update of the robot (:189), the strings UPDATE_WEIGHT (:1217) and TERMINATE (:1042)
 * in every robot's file.  Written by dpgo_team_run_schedule, which runs one iteration per host round trip while a log is
 * open.  directory = NULL closes the files. */
int dpgo_team_set_iteration_log(dpgo_team_t *t, const char *directory);
/* refresh this agent's neighbour slabs from co-resident agents (device-to-device) */
int dpgo_agent_pull_local(dpgo_team_t *t, int id);
/* average HIP-event duration of one launch of a hot kernel on the team stream.
 * which: 0 dense preconditioner apply, 1 cost+gradient SpMM, 2 Hessian-vector SpMM; 9 / 10 / 11 the step kernel of the
 * pipelined sequence back to back / that sequence launched eagerly / its evaluation launches alone; 14 the one-launch
 * iteration (csrc/step_fused.hip) launched eagerly, real iterations (fails where the team cannot take that form) */
int dpgo_team_time_kernel(dpgo_team_t *t, int id, int which, int reps, double *avg_ms, double *algorithmic_bytes);
/* peer access for one-process-per-GPU runs of the asynchronous mode (src/PGOAgentROS.cpp:119-127): a robot's X / Y arrays
 * exported as a 64-byte HIP IPC handle (+ the offsets of X and Y in doubles and its pose count), imported by the
 * processes that hold its neighbours; from then on its public poses are read in place (xGMI peer loads), one-sided:
 * no PublicPoses message, no rendezvous.  The exporting process must outlive the importers' use.  Once a team has imported
 * a peer, dpgo_agent_iterate reads every neighbour that is readable in place (imported or co-resident) from its owner's
 * arrays instead of from what dpgo_agent_update_neighbor_poses last supplied. */
int dpgo_agent_export_state(dpgo_team_t *t, int id, unsigned char *handle64, long long *offset_x, long long *offset_y, int *n);
int dpgo_team_import_peer(dpgo_team_t *t, int robot_id, const unsigned char *handle64, long long offset_x, long long offset_y, int n);
/* The synchronous schedule across processes WITHOUT the host in the loop (the UPDATE token of src/PGOAgentROS.cpp:136-149,
 * 443-504, 1161-1189 on the device): every team exports a mailbox of 64-bit words (IPC handle) that the teams holding its
 * robots' neighbours import (robot_ids: the robots that live in the exporting team); dpgo_team_run_peer then enqueues
 * `iters` global iterations -- robot sel_ids[q] holds the token in the q-th -- with wait / signal kernels around the
 * launches that read a neighbour in place or overwrite what a neighbour was reading.  Every process passes the same
 * list; nothing synchronises with the host; the iterates are those of dpgo_team_step_begin / _end with messages. */
int dpgo_team_export_mailbox(dpgo_team_t *t, unsigned char *handle64);
int dpgo_team_import_mailbox(dpgo_team_t *t, const unsigned char *handle64, const int *robot_ids, int count);
int dpgo_team_run_peer(dpgo_team_t *t, const int *sel_ids, int iters);
/* ---- one process per GPU, the exchange carried by RCCL from inside the library (csrc/rank_exchange.cpp) ----
 * Replaces the ROS transport of this path: PublicPoses messages (msg/PublicPoses.msg:1-8; sent src/PGOAgentROS.cpp:662-690,
 * received :1255-1284) become packed r x 4 fp64 slabs moved by ncclSend / ncclRecv that the library enqueues on the team
 * stream; the staleness gate (:136-149, maxDelayedIterations include/dpgo_ros/PGOAgentROS.h:83) decides which slabs are
 * sent; the UPDATE token (:443-504, 1161-1189) is the list of token holders every rank is handed.
 * RCCL is bound at run time (dlopen librccl.so.1; DPGO_RCCL_LIBRARY overrides): single-GPU users never load it.
 * A communicator is an object of its own because ranks that own no robot (5 robots on 8 GPUs) still take part in its
 * creation and in the reductions.  id128: DPGO_COMM_ID_BYTES bytes obtained on ONE rank and handed to all (any channel). */
#define DPGO_COMM_ID_BYTES 128
typedef struct dpgo_comm dpgo_comm_t;
int dpgo_comm_unique_id(unsigned char *id128);
dpgo_comm_t *dpgo_comm_create(int device, const unsigned char *id128, int rank, int world); /* collective; NULL on error */
void dpgo_comm_destroy(dpgo_comm_t *c);
int dpgo_comm_rank(const dpgo_comm_t *c);
int dpgo_comm_world(const dpgo_comm_t *c);
/* which RCCL was bound: path + version code into out; returns the version code (<0 on error) */
int dpgo_comm_library(char *out, int cap);
/* small collectives (<= 64 doubles, host in/out, synchronous) on `stream` (hipStream_t or NULL) */
int dpgo_comm_allreduce_sum(dpgo_comm_t *c, void *stream, double *inout, int n);
int dpgo_comm_allreduce_max(dpgo_comm_t *c, void *stream, double *inout, int n);
/* owner_rank_of_robot[num_robots]: the rank that holds each robot (every robot of this team must map to the communicator's
 * rank).  max_delayed_iterations: the staleness gate.  loopback (world size 1 only): every neighbour pair -- co-resident
 * ones included -- exchanges through RCCL self-sends and nothing is read in place: the message path end to end on one GPU. */
int dpgo_team_attach_comm(dpgo_team_t *t, dpgo_comm_t *c, const int *owner_rank_of_robot, int max_delayed_iterations, int loopback);
int dpgo_team_detach_comm(dpgo_team_t *t);
/* every neighbour pair that crosses ranks, both directions, X and Y (after set_initial; before a cost evaluation) */
int dpgo_team_exchange_all_ranks(dpgo_team_t *t);
/* `iters` global iterations, robot sel_ids[q] holding the token in the q-th: per iteration the iterate(false) part of every
 * local robot (:1183-1186), the token holder's neighbours' public poses by ncclSend / ncclRecv (one message per pair of
 * ranks), the block update (:160).  Nothing synchronises with the host; every rank that owns a robot passes the same
 * list.  Iterates equal dpgo_team_step_begin / messages / dpgo_team_step_end bit for bit. */
int dpgo_team_run_ranks(dpgo_team_t *t, const int *sel_ids, int iters);
/* the lockstep ASAPP ticks (dpgo_team_run_simultaneous) and the classes of a colour-parallel sweep (dpgo_team_run_group, after
 * dpgo_team_set_groups with the global classes) with their boundary slabs moved by the library in the same way */
int dpgo_team_run_simultaneous_ranks(dpgo_team_t *t, int ticks);
int dpgo_team_run_group_ranks(dpgo_team_t *t, int group, int count);
/* the planning layer of the exchange replayed for ONE rank of a world, host arithmetic only (no device, no RCCL): the full
 * exchange, then `iters` iterations of the token schedule with the staleness gate.  npub[b * num_robots + a] = public poses of
 * robot b that robot a needs (0: not neighbours).  out[(1 + iters) * world * 4]: per batch and peer rank {doubles sent, doubles
 * received, hash of the sent slabs in order, hash of the received slabs in order} -- what rank r sends to p must be what p
 * receives from r (tests/test_rank_plan.py replays every rank of worlds of 2 .. 8). */
int dpgo_rank_plan_simulate(int num_robots, int world, int rank, const int *owner, const int *npub, int acceleration,
                            int max_delayed_iterations, int r, const int *sel_ids, int iters, long long *out);
/* global cost: this team's owned-edge partial sums (t may be NULL on a rank without robots) + a 1-double all-reduce */
int dpgo_comm_global_cost(dpgo_comm_t *c, dpgo_team_t *t, void *stream, double *f);
/* out[4]: point-to-point messages sent / received by this rank, bytes sent / received */
int dpgo_team_comm_counters(dpgo_team_t *t, double *out4);
/* diagnostic: hand-off words of an agent's one-launch RTR solve (rtr_fused.hip; phase stamps in trace builds) */
int dpgo_agent_read_rtr_handoff(dpgo_team_t *t, int id, unsigned long long *out, int n);
/* diagnostic: `n` doubles of an agent's device-side partial-sum scratch (csrc/dpgo_dev.h PART_*) from `offset` */
int dpgo_agent_read_partials(dpgo_team_t *t, int id, int offset, double *out, int n);
/* counters for the roofline report: launches and algorithmic bytes of the dominant kernels ([0] preconditioner applies,
 * [1] their bytes, [2] sparse evaluations, [3] their bytes, [4] iterations); diagnostics of the per-agent API: [5] host
 * microseconds between the launch of a report kernel and the arrival of its sequence word, [6] reports; [7] iterations
 * of dpgo_team_run that took the one-launch form (csrc/step_fused.hip), [8] those of them that found the row products of
 * their agent formed by the previous launch (carried rows), [9] the deep-carried ones (csrc/step_deep.hip); [10] reports
 * of the per-agent API that rode on the last launch of their iterate(true) (k_eval_report) */
int dpgo_team_get_counters(dpgo_team_t *t, double *out, int n);

#ifdef __cplusplus
}
#endif
#endif
