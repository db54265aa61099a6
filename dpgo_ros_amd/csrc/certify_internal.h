// certify_internal.h -- the certificate's device workspace and host helpers (certify.hip), shared with the rounding of a
// certified point (round.hip) and with the calls across teams (certify_across.hip).  The kernels stay in certify.hip;
// Cert's launching methods are defined there.
#pragma once
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "kernel_common.h"
#include "schur_across_plan.h"
#include "team_internal.h"

namespace dpgo {

constexpr int CG_CH = 128;   // columns per workgroup of a Gram launch
constexpr int CG_MAXK = 24;  // most rows of either operand (the 3K-row basis at K = 8)

// OUT = beta OUT + sum_t s_t A_t C_t, one thread per element (column, q).  C_t row-major k_t x ko on the device (null:
// the identity, k_t = ko).  No A_t may alias OUT.
struct CertTerm {
  const double *A;
  const double *C;
  int lda, ka;
  double s;
};
struct CertTerms {
  CertTerm t[3];
  int n;
};

}  // namespace dpgo

namespace dpgo_cert {
using namespace dpgo;
using namespace dpgo_host;

// cyclic Jacobi eigendecomposition of a symmetric n x n matrix (row-major): ascending eigenvalues w, eigenvectors as the
// columns of V (row-major, V[i * n + k] = component i of vector k)
void jacobi_eig(int n, std::vector<double> A, std::vector<double> &w, std::vector<double> &V);

struct Across;

// the certificate's device state for one call
struct Cert {
  dpgo_team_t *t = nullptr;
  Across *x = nullptr;  // across teams (certify_across.hip): halo exchange inside apply, reductions through the transport
  int r = 0, K = 0, na = 0, N = 0, L = 0, max_n = 0, nz = 0;  // nz: rows of the orthonormal deflation basis Zo
  bool deflate = true, precond = true;
  double *Xt = nullptr, *E = nullptr, *lam = nullptr, *Zr = nullptr, *Zo = nullptr;
  double *U[2] = {nullptr, nullptr}, *AU[2] = {nullptr, nullptr}, *T = nullptr, *T2 = nullptr;
  double *part = nullptr, *G = nullptr, *gmax = nullptr;
  int *off = nullptr;
  int gstride = 0, nblk = 0;
  // the eigensolver's Gram sums (gram_agents): chunk k covers the team's columns [chunk0[k], chunkend[k]) of one agent,
  // agent a owns chunks [achunk[a], achunk[a + 1]); atot: per slot, the agents' totals (na x ka kb) of its last Gram
  int nchunk = 0;
  int *achunk = nullptr, *chunk0 = nullptr, *chunkend = nullptr;
  double *atot = nullptr;
  static constexpr int SLOT = CG_MAXK * CG_MAXK;
  // Gram slots: 0 basis x operator, 1 basis x basis, 2 residual x residual, 3 Cholesky failure word (read back together),
  // 4 X^T S X, 5 deflation products, 6 Cholesky coefficients, 7 coefficients from the host
  double *slot(int k) const { return G + (size_t)k * SLOT; }

  int setup(int K_);
  void apply(int k, const double *V, int ldv, double *out, int ldo, bool with_lam);
  void gram(const double *A, int lda, int ka, const double *B, int ldb, int kb, double *out);
  // A^T B into slot(slot_), summed agent by agent: inside an agent in chunks of 128 columns, then the agents' totals in
  // team order.  The order does not depend on which team holds which robot, so a call split across teams (reduce_agents)
  // gives the single team's bits (robots in id order in both)
  void gram_agents(const double *A, int lda, int ka, const double *B, int ldb, int kb, int slot_);
  // across teams: the listed slots (slot, count) of gram_agents summed over all robots in id order (no-op for one team)
  void reduce_agents(std::initializer_list<std::pair<int, int>> parts);
  // out[o] = sum over the nblk partials part[k * m + o], in k order (one workgroup)
  void sum_partials(const double *p, int nblk_, int m, double *out);
  void update(double *out, int ldo, int ko, double beta, std::initializer_list<CertTerm> terms);
  // V <- V - Zo^T (Zo V^T): onto the complement of the deflation basis
  void project(double *V, int ld, int k);
  // rows of V orthonormal: V <- L^-1 V (CholQR) through scratch S (k rows, ld k)
  void cholqr(double *V, int ld, int k, double *S);
  void precondition(const double *V, int ldv, double *out, int ldo);
  // across teams: the listed device arrays summed over the participants in rank order, in place (no-op for one team)
  void reduce(std::initializer_list<std::pair<double *, int>> parts);
  bool halted() const;  // across teams: this participant failed or the collective did -- no more device work
  bool dead() const;  // across teams: the collective found a failure -- every participant returns DPGO_ERR
};

// across teams: the transport, the agreement of the participants, the halo plan and the failure protocol
// (certify_across.hip).  A participant that fails locally sets `bad`: it launches nothing more but keeps to
// the sequence of transport calls up to the next allgather, whose status word makes every participant set `dead`; from
// then on nobody calls the transport and every participant returns DPGO_ERR.
struct Across {
  const dpgo_transport_t *tr = nullptr;
  std::string what;
  int rank = 0, world = 1, num_robots = 0;
  std::vector<int> owner;
  bool bad = false, dead = false, all_precond = true;
  std::string err;
  // global numbering: robots by id, then poses
  std::vector<int> robot_n, robot_holder, robot_lidx;
  std::vector<long long> robot_goff;
  long long nglob = 0;
  // halo plan: this team's public poses per peer (team pose index) and where received poses land (halo slot), both in
  // plan order -- by peer rank, then (sending robot, receiving robot, frame)
  std::vector<int> scol, rdst, hoffs;
  std::vector<long long> sent_p, recv_p;  // poses per peer
  int halo_slots = 0;
  int *d_scol = nullptr, *d_rdst = nullptr, *d_hoff = nullptr;
  double *d_halo = nullptr, *d_send = nullptr, *d_recv = nullptr;
  std::vector<double> hsend, hrecv, hred[2], hall;
  int hflip = 0;
  long long n_allgather = 0, n_exchange = 0;

  // local checks, the agreement record (two allgathers) and the plan; DPGO_ERR on every participant when they disagree.
  // argerr: this participant's arguments are invalid (the others learn it from the record)
  int begin(dpgo_team_t *t, const dpgo_transport_t *tr_, const int *owner_, const char *what_, int op, int K, int flags,
            double eta, double tol, int max_iters, const char *argerr);
  size_t dev_doubles() const { return (size_t)(halo_slots + scol.size() + rdst.size()) * 4 * 8 + 8; }
  size_t dev_ints() const { return scol.size() + rdst.size() + hoffs.size() + 1; }
  // carve the device tables out of d_cert / d_cert_int (behind the caller's part) and upload them
  void place(double *d, int *di, hipStream_t s);
  void note(hipError_t e, int line);
  void fail_local(const std::string &m);
  // the halo of the k-row block V (ld ldv): pack, exchange, unpack.  Returns the device halo ([(4 slot + c) k + b])
  const double *halo_of(Cert &c, int k, const double *V, int ldv);
  // allgather of mine = [status, payload...]: `all` receives world records of that length
  int gather(std::vector<double> &mine, std::vector<double> &all);
  // the listed device arrays summed (or maximised) over the participants in rank order, in place
  int reduce(Cert &c, std::initializer_list<std::pair<double *, int>> parts, bool take_max = false);
  // the slots of Cert::gram_agents: every robot's total from its holder, summed on the host in robot order from 0 -- the
  // single team's order of additions
  int reduce_agents(Cert &c, std::initializer_list<std::pair<int, int>> parts);
  const double *reduced() const { return hred[1 - hflip].data() + 1; }  // the host copy of the last reduce
  int finish();  // the closing status word: DPGO_ERR on every participant when any failed
  int fail();    // set_err(what: err), DPGO_ERR
};

// a HIP step: DPGO_ERR for one team; across teams the error is noted (and the step skipped once this participant has halted)
#define CERT_CK(c, expr)                                \
  do {                                                  \
    if ((c).x) {                                        \
      if (!(c).halted()) (c).x->note((expr), __LINE__); \
    } else {                                            \
      HIPC(expr);                                       \
    }                                                   \
  } while (0)

// every robot local and INITIALIZED, every neighbour inside the team; descriptors synchronised.  `what` prefixes the message.
int check_team(dpgo_team_t *t, const char *what);
// its first half: every robot local and initialized, decided on the host without touching the device
int check_team_local(dpgo_team_t *t, const char *what);

// the rank-3 forms of the certificate's kernels for a trajectory T in the iterate layout (3 x 4N, ld 3; covariance.hip):
// out = T Q (lam null) or T S, one team;  Lambda_i = Sym(R_i^T E_i,rot) into lam (9 per pose), gmax: na x ceil(max_n / 256)
// doubles of scratch (the Gershgorin sums k_cert_lambda leaves)
// across teams: halo ([(4 slot + c) 3 + b], Across::halo_of at k = 3) and hoff (Across::d_hoff), the remote neighbours' poses
void launch_cert_apply3(hipStream_t s, const AgentDev *agents, const int *off, int na, int max_n, const double *V, double *out,
                        const double *lam, const double *halo = nullptr, const int *hoff = nullptr);
void launch_cert_lambda3(hipStream_t s, const AgentDev *agents, const int *off, int na, int max_n, const double *X,
                         const double *E, double *lam, double *gmax);

// the team's measurements with their current weights in team-order pose numbering (robot fields zeroed), each shared
// edge once: the copy of the lower robot, which owns its weight.  offs: pose offsets of the local agents (na + 1)
int team_measurements(dpgo_team_t *t, const std::vector<int> &offs, const char *what, std::vector<dpgo_measurement_t> &mm);

// the LOBPCG of dpgo_team_certify on a Cert whose t (and x, across teams) is set (certify.hip)
int certify_body(Cert &c, double eta, double tol, int max_iters, int K, int flags, dpgo_certificate_t *out, double *v);


// What a covariance path has staged on the device when its last extraction kernel is queued: T (the iterate layout, 12 per
// pose), the N diagonal blocks and behind them the num_pairs pair blocks (36 doubles each, row-major), all ordered on
// `stream`.  The buffers belong to the path and live until the epilogue has returned AND the path has drained the stream.
struct CovStage {
  const double *Td, *diag, *pairs;
  int N, num_pairs;
  hipStream_t stream;
};
// A step behind the staged blocks (gate.hip).  A path that is given one calls run() in the place of its copy of the blocks
// to the host (cov_diag / cov_pairs are then not touched and may be null), and drains the stream afterwards: run() queues
// its kernels and its own copies on stage.stream and does not synchronise.  DPGO_OK, or DPGO_ERR with a message.
struct CovEpilogue {
  virtual int run(const CovStage &stage) = 0;
  virtual ~CovEpilogue() = default;
};
// Sigma applied to vectors inside a covariance path (covariance_apply.h).  A path that is given one allocates V
// and X (6 N x num_cols, column-major, leading dimension 6 N; rows 6 p .. 6 p + 5 belong to team pose p), calls rhs() once
// CovFrame::begin has T on the device -- rhs() queues on `stream` whatever writes every element of V outside pose 0's rows,
// which are not read -- forms X = Sigma V from its own factors without a block of Sigma, and sets X before it runs the
// epilogue: the pointer stays valid as long as the staged blocks do.  Pose 0's rows of X are zero bits.
struct CovApply {
  int num_cols = 0;
  double *X = nullptr;
  double ms_products = 0.0, flops = 0.0;  // the apply's own products, for the caller's DPGO_TIMING line
  virtual int rhs(const double *Td, int N, double *V, hipStream_t stream) = 0;
  virtual ~CovApply() = default;
};

// the device part of dpgo_team_marginal_covariances by the dense inverse (covariance.hip, behind the host-side refusals of
// marginal_covariances_call): DPGO_OK, DPGO_ERR with a message, or k + 1 > 0 when the pivot of row k of the reduced Hessian
// was not positive
int covariance_device(dpgo_team_t *t, const double *T, int num_pairs, const int *pairs, double *cov_diag, double *cov_pairs,
                      dpgo_covariance_t *res, CovEpilogue *epi = nullptr, CovApply *app = nullptr);
// dpgo_team_marginal_covariances / _nested with an epilogue in the place of the copy of the blocks (covariance.hip,
// covariance_nested.hip): the public calls are these with epi = nullptr; with one, cov_diag and cov_pairs may be null
int marginal_covariances_call(dpgo_team_t *t, const double *T, int flags, int num_pairs, const int *pairs, double *cov_diag,
                              double *cov_pairs, dpgo_covariance_t *res, CovEpilogue *epi, CovApply *app = nullptr);
// (with app the nested call runs its own device part on nest_plan_team's plan whether or not a robot is split)
int marginal_covariances_nested_call(dpgo_team_t *t, const double *T, int max_block, int num_pairs, const int *pairs, double *cov_diag,
                                     double *cov_pairs, dpgo_covariance_t *res, CovEpilogue *epi, CovApply *app = nullptr);
// the refusals of the marginal covariances that are decided on the host, shared by its methods (covariance.hip): DPGO_OK, 1 (the
// anchor alone: outputs written), or DPGO_ERR
int covariance_host_checks(dpgo_team_t *t, const double *T, const char *flags_error, int num_pairs, const int *pairs, double *cov_diag,
                           double *cov_pairs, dpgo_covariance_t *res, const char *what, int *num_poses, bool staged = false);
// k_cov_logdet on a Cholesky factor left in A: out[0 .. 2] = 2 sum log L_kk, min L_kk^2, max L_kk^2
int launch_cov_logdet(hipStream_t s, const double *A, int n, double *out);
// the same call by robot-wise Schur complement (covariance_schur.hip; flags = DPGO_COV_SCHUR): DPGO_OK, DPGO_ERR with a message,
// or 1 when a pivot was not positive -- fail[0] the local index of the robot whose interior block failed (-1: the separator),
// fail[1] the team pose of the pivot, fail[2] its row in that factor
int covariance_schur_device(dpgo_team_t *t, const double *T, int num_pairs, const int *pairs, double *cov_diag, double *cov_pairs,
                            dpgo_covariance_t *res, int *fail, CovEpilogue *epi = nullptr);
// ---- the path over a split team (covariance_schur.hip, SchurAcross; DESIGN.md 5e, "across teams")
//
// What the path has on the device of EVERY participant once allgather D has run ("across teams"): compact tables
// over the E sorted distinct endpoint poses of the records and the P listed pairs -- T (12 per endpoint, the iterate layout),
// the E diagonal blocks and the P pair blocks (36 doubles each, row-major), all ordered on `stream`.  An index into them takes
// the place of the team pose of CovStage: the kernels behind a single team's blocks run on them unchanged.
struct AcrossStage {
  const double *Td, *diag, *pairs;
  int E, P;
  hipStream_t stream;
};
// What the path holds when it calls AcrossStep::taken(): T with its halo on the device (N poses of this participant in team
// order, then halo_slots poses, slot hoffs[k] + s the pose np[s] of local robot k; the slots of remote neighbours are filled,
// the others are not read by anyone), x_S = Sigma_SS r_S of the WHOLE problem (6 |S| x num_cols, leading dimension nS: after
// allgather B every participant knows every robot's public frames, so x_S is whole everywhere), and for every halo slot the
// separator pose whose rows 6 q .. 6 q + 5 of x_S are the slot's rows of X (-1: the problem's fixed pose, whose rows are zero,
// or a slot of a neighbour that lives here).  With pairs beside the columns (the first-order update, DESIGN.md 5j "across
// teams") the view also hands the blocks back: diag, the N diagonal blocks of this participant's poses on the device, and
// blocks_h, the host image of those N blocks and behind them the num_pairs pair blocks, complete after allgather C.  All of
// it is ordered on the path's stream and lives until the path has drained it behind taken(); filling it costs no launch and
// no transport call.
struct CovAcrossView {
  const double *Td = nullptr, *xS = nullptr, *diag = nullptr, *blocks_h = nullptr;
  int N = 0, halo_slots = 0, nS = 0, num_pairs = 0;
  std::vector<int> halo_sep;
};
// The ONE hook of the path: what a public call adds to the marginal covariances across teams.  The call fills the agreement
// record before the path starts -- name, op, the two real fields (agree_num, agree_hash) and the integer one (agree_int) of
// Across::begin, so that a record list that differs on one participant is refused everywhere -- with argerr, this participant's
// own refusal, which the others learn from the record, and memerr: its V and X alone exceed the device (V was then not read),
// told as the path's memory refusal.  The step as it stands here is the plain call (op 3; the path fills the number and the
// hash of the caller's pairs).  Every virtual does nothing unless overridden, and then queues no launch and sends no byte:
//   resolve()    behind begin, when the global numbering is known: DPGO_OK, 2: the transport is dead, anything else: a refusal
//                in msg, the same words on every participant.  A step with records fills `pairs` (global pose ids, two per
//                pair), which then take the place of the caller's, and its endpoints;
//   num_cols(), rhs()   Sigma applied to vectors beside the blocks (DESIGN.md 5m "across teams"; 0: none).  The path allocates V
//                and X (6 N x num_cols, N this participant's poses, pose 0 the problem's) and calls rhs() once T is on the
//                device, as CovApply::rhs above;
//   taken()      once X and `view` are set: queues on `stream` whatever reads X; the path drains the stream;
//   exchange()   behind taken(), whether or not this participant still works (x.bad): the step's own allgathers, the same
//                number on every participant, and behind them its device work;
//   endpoints(), run()   a step behind compact tables (the gate, the audit): the records' endpoints, sorted
//                and distinct, make allgather D run; run() queues its uploads, its kernel and the copies of its per-record
//                outputs on stage.stream and does not synchronise; the path drains the stream and closes the protocol.
struct AcrossStep {
  const char *name = "marginal_covariances_across";
  int op = 3, agree_int = 0;
  double agree_num = 0.0, agree_hash = 0.0;
  std::string argerr, memerr;
  std::vector<int> pairs;
  CovAcrossView view;
  double *X = nullptr;
  double ms_products = 0.0, flops = 0.0;  // the apply's own products, for the caller's DPGO_TIMING line
  virtual int resolve(Across & /*x*/, std::string & /*msg*/) { return DPGO_OK; }
  virtual int num_cols() const { return 0; }
  virtual int rhs(const double * /*Td*/, int /*N*/, double * /*V*/, hipStream_t /*stream*/) { return DPGO_OK; }
  virtual int taken(int /*N*/, hipStream_t /*stream*/) { return DPGO_OK; }
  virtual int exchange(Across & /*x*/, hipStream_t /*stream*/) { return DPGO_OK; }
  virtual const std::vector<int> *endpoints() const { return nullptr; }
  virtual int run(const AcrossStage & /*stage*/) { return DPGO_OK; }
  virtual ~AcrossStep() = default;
};
// Sigma applied to vectors with nothing else (op 6: the first real field carries num_cols, the hash is that of no pairs)
struct ApplyStep : AcrossStep {
  int cols;
  explicit ApplyStep(int num_cols_) : cols(num_cols_) {
    name = "covariance_apply_across";
    op = 6;
    agree_num = num_cols_;
    agree_hash = RecordHash().value();
  }
  int num_cols() const override { return cols; }
};

// The call over a split team (dpgo_team_marginal_covariances_across and the five calls that ride on it).  step null: the plain
// call, which writes the N diagonal blocks of this participant's poses to cov_diag and the listed pairs to cov_pairs.  With a
// step the blocks stay with the path (cov_diag and cov_pairs are not touched and may be null) and only res is filled.  res is
// all zero unless the call returns DPGO_OK.
struct SchurAcrossArgs {
  dpgo_team_t *t;
  const dpgo_transport_t *tr;
  const int *owner;  // the owner table: the rank that holds each robot
  const double *T;
  SchurAcrossArgs(dpgo_team_t *team, const dpgo_transport_t *transport, const int *owner_rank_of_robot, const double *T_)
      : t(team), tr(transport), owner(owner_rank_of_robot), T(T_) {}
  int flags = DPGO_COV_SCHUR;
  int num_pairs = 0;
  const int *pairs = nullptr;
  double *cov_diag = nullptr, *cov_pairs = nullptr;
  dpgo_covariance_t *res = nullptr;
  AcrossStep *step = nullptr;
};
int covariance_schur_across(const SchurAcrossArgs &a);

}  // namespace dpgo_cert
