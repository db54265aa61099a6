// certify_across.hip -- the certificate and the rounding of an iterate whose robots are split across teams (one team per
// participant: a process, or a thread driving its own GPU), DESIGN.md 5d.
//
// The operator is local: S(X) V on one agent's columns reads the agent's Q block, its Lambda blocks and the neighbours'
// rows of V at the shared-edge end points -- the public-pose halo, with K rows in place of r.  A halo exchange is one pack
// launch (every peer's poses into one staging buffer, plan order), one call of the transport's `exchange`, one unpack
// launch into the halo (k_cert_apply reads a remote neighbour there).  Everything else of LOBPCG and of the rounding is a
// small Gram matrix, a count or a maximum: reduced on the device in the single team's fixed order (k_cert_gram +
// k_cert_gram_sum), allgathered, summed on the host in rank order and uploaded where the device needs it.  Every host
// decision is taken on those summed bits, so every participant takes the same branch at the same point and makes the same
// transport calls.  One participant that holds every robot reproduces the single team bit for bit: its sums are its own
// values and it has no remote neighbour.
#include <algorithm>
#include <tuple>

#include "certify_internal.h"

namespace dpgo {

// stage[(4 e + c) k + b] = V[(4 scol[e] + c) ld + b]: this team's public poses of the k-row block V, plan order; one lane per
// (pose, row), so that a wave's lanes read and write contiguous rows
__global__ __launch_bounds__(256) void k_xa_pack(const double *__restrict__ V, int ld, int k, const int *__restrict__ scol,
                                                 int ne, double *__restrict__ stage) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ne * k) return;
  const int e = i / k, b = i - e * k;
  const size_t g = (size_t)scol[e];
#pragma unroll
  for (int c = 0; c < 4; ++c) stage[((size_t)4 * e + c) * k + b] = V[(4 * g + c) * ld + b];
}

// halo[(4 rdst[e] + c) k + b] = recv[(4 e + c) k + b]: the received poses into the halo slots of their receivers
__global__ __launch_bounds__(256) void k_xa_unpack(const double *__restrict__ recv, int k, const int *__restrict__ rdst, int ne,
                                                   double *__restrict__ halo) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ne * k) return;
  const int e = i / k, b = i - e * k;
  const size_t s = (size_t)rdst[e];
#pragma unroll
  for (int c = 0; c < 4; ++c) halo[(4 * s + c) * k + b] = recv[((size_t)4 * e + c) * k + b];
}

}  // namespace dpgo

using namespace dpgo;
using namespace dpgo_host;
using namespace dpgo_cert;

namespace {

// FNV-1a over 64-bit words, kept to 52 bits so that a double carries it exactly
struct Fnv {
  unsigned long long h = 1469598103934665603ull;
  void add(long long v) {
    for (int i = 0; i < 8; ++i) {
      h ^= (unsigned long long)(v >> (8 * i)) & 0xffull;
      h *= 1099511628211ull;
    }
  }
  double value() const { return (double)(h & ((1ull << 52) - 1)); }
};

// the agreement header: [0] status word of the allgather, [1] refusal code, [2] its detail, [3] rank, [4] world, then the
// fields every participant must pass alike
enum { XA_OK = 0, XA_ARGS, XA_OWNER_RANGE, XA_NOT_OWNER, XA_NOT_HELD, XA_EMPTY, XA_UNINIT, XA_LOCAL };
constexpr int XA_HDR = 14;
const char *const XA_FIELD[XA_HDR] = {"", "", "", "", "", "the operation", "num_robots", "r", "the block size", "flags",
                                      "eta", "tol", "max_iters", "the owner table"};

std::string refusal(int q, int code, long long detail) {
  const std::string who = "rank " + std::to_string(q) + ": ";
  switch (code) {
    case XA_ARGS: return who + "invalid arguments";
    case XA_OWNER_RANGE: return who + "the owner table names no participant for robot " + std::to_string(detail);
    case XA_NOT_OWNER: return who + "holds robot " + std::to_string(detail) + ", which the owner table gives to another rank";
    case XA_NOT_HELD: return who + "the owner table gives it robot " + std::to_string(detail) + ", which its team does not hold";
    case XA_EMPTY: return who + "holds no robot";
    case XA_UNINIT: return who + "robot " + std::to_string(detail) + " is not initialized";
    default: return who + "local failure";
  }
}

}  // namespace

namespace dpgo_cert {

void Across::note(hipError_t e, int line) {
  if (e == hipSuccess) return;
  (void)hipGetLastError();
  fail_local(std::string(hipGetErrorString(e)) + " @" + std::to_string(line));
}

void Across::fail_local(const std::string &m) {
  if (bad) return;
  bad = true;
  err = "rank " + std::to_string(rank) + ": " + m;
}

int Across::fail() {
  set_err(what + ": " + err);
  return DPGO_ERR;
}

int Across::gather(std::vector<double> &mine, std::vector<double> &all) {
  if (dead) return DPGO_ERR;
  mine[0] = bad ? 1.0 : 0.0;
  const int n = (int)mine.size();
  all.assign((size_t)world * n, 0.0);
  ++n_allgather;
  if (tr->allgather(tr->ctx, mine.data(), n, all.data()) != 0) {
    dead = true;
    if (!bad) err = "rank " + std::to_string(rank) + ": the transport's allgather failed";
    return DPGO_ERR;
  }
  for (int q = 0; q < world; ++q)
    if (all[(size_t)q * n] != 0.0) {
      dead = true;
      if (!bad) err = "rank " + std::to_string(q) + " failed locally (its own error names the cause)";
      return DPGO_ERR;
    }
  return 0;
}

int Across::reduce(Cert &c, std::initializer_list<std::pair<double *, int>> parts, bool take_max) {
  if (dead) return DPGO_ERR;
  size_t m = 0;
  for (auto &p : parts) m += (size_t)p.second;
  const hipStream_t s = c.t->stream;
  // two host images in turn: the upload from one may still be queued while the other is filled (the download in
  // between synchronises the stream)
  std::vector<double> &h = hred[hflip];
  h.assign(1 + m, 0.0);
  if (!bad) {
    size_t o = 1;
    for (auto &p : parts) {
      note(hipMemcpyAsync(h.data() + o, p.first, sizeof(double) * p.second, hipMemcpyDeviceToHost, s), __LINE__);
      o += (size_t)p.second;
    }
    note(hipStreamSynchronize(s), __LINE__);
  }
  if (gather(h, hall)) return DPGO_ERR;
  const size_t n = 1 + m;
  for (size_t o = 1; o < n; ++o) {
    double v = hall[o];
    for (int q = 1; q < world; ++q) v = take_max ? std::max(v, hall[(size_t)q * n + o]) : v + hall[(size_t)q * n + o];
    h[o] = v;
  }
  size_t o = 1;
  for (auto &p : parts) {
    if (!bad) note(hipMemcpyAsync(p.first, h.data() + o, sizeof(double) * p.second, hipMemcpyHostToDevice, s), __LINE__);
    o += (size_t)p.second;
  }
  hflip ^= 1;
  return 0;
}

int Across::reduce_agents(Cert &c, std::initializer_list<std::pair<int, int>> parts) {
  if (dead) return DPGO_ERR;
  size_t m = 0;
  for (auto &p : parts) m += (size_t)p.second;
  const hipStream_t s = c.t->stream;
  const int na = c.na;
  std::vector<double> &h = hred[hflip];  // [status, robot 0's m sums, robot 1's, ...]: zeros for the robots held elsewhere
  h.assign(1 + m * num_robots, 0.0);
  if (!bad) {
    std::vector<double> tot(m * na);
    size_t o = 0;
    for (auto &p : parts) {
      note(hipMemcpyAsync(tot.data() + o * na, c.atot + (size_t)p.first * na * Cert::SLOT, sizeof(double) * p.second * na,
                          hipMemcpyDeviceToHost, s), __LINE__);
      o += (size_t)p.second;
    }
    note(hipStreamSynchronize(s), __LINE__);
    o = 0;
    for (auto &p : parts) {
      for (int k = 0; k < na && !bad; ++k)
        std::copy(tot.begin() + o * na + (size_t)k * p.second, tot.begin() + o * na + (size_t)(k + 1) * p.second,
                  h.begin() + 1 + (size_t)c.t->ag[k]->id * m + o);
      o += (size_t)p.second;
    }
  }
  if (gather(h, hall)) return DPGO_ERR;
  const size_t n = 1 + m * num_robots;
  for (size_t o = 0; o < m; ++o) {
    double v = 0.0;
    for (int i = 0; i < num_robots; ++i) v += hall[(size_t)robot_holder[i] * n + 1 + (size_t)i * m + o];
    h[1 + o] = v;
  }
  size_t o = 1;
  for (auto &p : parts) {
    if (!bad) note(hipMemcpyAsync(c.slot(p.first), h.data() + o, sizeof(double) * p.second, hipMemcpyHostToDevice, s), __LINE__);
    o += (size_t)p.second;
  }
  hflip ^= 1;
  return 0;
}

int Across::finish() {
  std::vector<double> m(1, 0.0);
  if (gather(m, hall)) return fail();
  return 0;
}

const double *Across::halo_of(Cert &c, int k, const double *V, int ldv) {
  if (dead) return nullptr;
  const hipStream_t s = c.t->stream;
  const size_t ns = scol.size(), nr = rdst.size(), w = (size_t)4 * k;
  if (!bad) note(hipStreamSynchronize(s), __LINE__);  // (the previous unpack has read hrecv)
  hsend.assign(ns * w, 0.0);
  hrecv.assign(nr * w, 0.0);
  if (!bad && ns) {
    k_xa_pack<<<(unsigned)((ns * k + 255) / 256), 256, 0, s>>>(V, ldv, k, d_scol, (int)ns, d_send);
    note(hipGetLastError(), __LINE__);
    note(hipMemcpyAsync(hsend.data(), d_send, sizeof(double) * ns * w, hipMemcpyDeviceToHost, s), __LINE__);
    note(hipStreamSynchronize(s), __LINE__);
    if (bad) std::fill(hsend.begin(), hsend.end(), 0.0);
  }
  std::vector<long long> sc(world), rc(world);
  for (int p = 0; p < world; ++p) {
    sc[p] = sent_p[p] * (long long)w;
    rc[p] = recv_p[p] * (long long)w;
  }
  ++n_exchange;
  if (tr->exchange(tr->ctx, hsend.data(), sc.data(), hrecv.data(), rc.data()) != 0) fail_local("the transport's exchange failed");
  if (!bad && nr) {
    note(hipMemcpyAsync(d_recv, hrecv.data(), sizeof(double) * nr * w, hipMemcpyHostToDevice, s), __LINE__);
    k_xa_unpack<<<(unsigned)((nr * k + 255) / 256), 256, 0, s>>>(d_recv, k, d_rdst, (int)nr, d_halo);
    note(hipGetLastError(), __LINE__);
  }
  return d_halo;
}

void Across::place(double *d, int *di, hipStream_t s) {
  d_halo = d;
  d += (size_t)halo_slots * 32;
  d_send = d;
  d += scol.size() * 32;
  d_recv = d;
  d_scol = di;
  di += scol.size();
  d_rdst = di;
  di += rdst.size();
  d_hoff = di;
  if (!scol.empty()) note(hipMemcpyAsync(d_scol, scol.data(), sizeof(int) * scol.size(), hipMemcpyHostToDevice, s), __LINE__);
  if (!rdst.empty()) note(hipMemcpyAsync(d_rdst, rdst.data(), sizeof(int) * rdst.size(), hipMemcpyHostToDevice, s), __LINE__);
  if (!hoffs.empty()) note(hipMemcpyAsync(d_hoff, hoffs.data(), sizeof(int) * hoffs.size(), hipMemcpyHostToDevice, s), __LINE__);
}

int Across::begin(dpgo_team_t *t, const dpgo_transport_t *tr_, const int *owner_, const char *what_, int op, int K, int flags,
                  double eta, double tol, int max_iters, const char *argerr) {
  what = what_;
  if (!t || !tr_ || !tr_->allgather || !tr_->exchange || tr_->world < 1 || tr_->rank < 0 || tr_->rank >= tr_->world) {
    set_err(what + ": null team, or an incomplete transport (allgather, exchange, 0 <= rank < world)");
    return DPGO_ERR;
  }
  tr = tr_;
  rank = tr->rank;
  world = tr->world;
  num_robots = t->prm.num_robots;
  // local checks: refusals travel in the header, so that every participant refuses
  int code = XA_OK;
  long long detail = 0;
  std::string local_msg;
  Fnv oh;
  owner.assign(num_robots, -1);
  if (argerr) {
    code = XA_ARGS;
    local_msg = argerr;
  } else if (!owner_) {
    code = XA_OWNER_RANGE;
  } else {
    for (int i = 0; i < num_robots; ++i) {
      owner[i] = owner_[i];
      oh.add(owner_[i]);
      if (!code && (owner_[i] < 0 || owner_[i] >= world)) { code = XA_OWNER_RANGE; detail = i; }
    }
  }
  if (!code && t->ag.empty()) code = XA_EMPTY;
  if (!code)
    for (auto &a : t->ag)
      if (a->id < 0 || a->id >= num_robots || owner[a->id] != rank) { code = XA_NOT_OWNER; detail = a->id; break; }
  if (!code)
    for (int i = 0; i < num_robots; ++i)
      if (owner[i] == rank && !t->id2local.count(i)) { code = XA_NOT_HELD; detail = i; break; }
  if (!code)
    for (auto &a : t->ag)
      if (a->state != DPGO_INITIALIZED || !a->has_X) { code = XA_UNINIT; detail = a->id; break; }
  if (!code && sync_descs(t)) { code = XA_LOCAL; local_msg = g_err; }
  std::vector<double> h(XA_HDR, 0.0);
  h[1] = code; h[2] = (double)detail; h[3] = rank; h[4] = world;
  h[5] = op; h[6] = num_robots; h[7] = t->prm.r; h[8] = K; h[9] = flags; h[10] = eta; h[11] = tol; h[12] = max_iters;
  h[13] = oh.value();
  if (gather(h, hall)) return fail();
  for (int q = 0; q < world; ++q) {
    const double *hq = hall.data() + (size_t)q * XA_HDR;
    if (hq[1] != XA_OK) {
      err = (q == rank && !local_msg.empty()) ? refusal(q, (int)hq[1], (long long)hq[2]) + " (" + local_msg + ")"
                                               : refusal(q, (int)hq[1], (long long)hq[2]);
      dead = true;
      return fail();
    }
  }
  for (int q = 0; q < world; ++q) {
    const double *hq = hall.data() + (size_t)q * XA_HDR;
    if (hq[3] != q || hq[4] != world) {
      err = "rank " + std::to_string(q) + " reports rank " + std::to_string((long long)hq[3]) + " of " +
            std::to_string((long long)hq[4]) + ": the transport's rank order disagrees";
      dead = true;
      return fail();
    }
    for (int f = 5; f < XA_HDR; ++f)
      if (hq[f] != hall[f]) {
        // (op 3, the covariances: the two real fields carry the number of pairs and the hash of the pair list)
        // (op 4, 5, the gate and the audit: the number of records and the hash of the record list)
        // (op 6, Sigma applied to vectors: the first real field carries num_cols)
        // (op 7, the refinement: flags carries the ladder, the two real fields grad_tol and armijo)
        // (op 8, the update across teams: as 4 and 5; the hash covers the pair list too and the integer field carries num_pairs)
        const bool recs = op == 4 || op == 5 || op == 8;
        const char *name = (op == 8 && f == 12) ? "num_pairs" : (op == 7 && f == 9) ? "ladder" : (op == 7 && f == 10) ? "grad_tol" : (op == 7 && f == 11) ? "armijo"
                           : (op == 6 && f == 10) ? "num_cols" : (op == 3 && f == 10) ? "num_pairs" : (op == 3 && f == 11) ? "the pair list"
                           : (recs && f == 10)  ? "the number of records" : (recs && f == 11) ? "the record list" : XA_FIELD[f];
        err = "the participants disagree on " + std::string(name) + " (rank 0 and rank " + std::to_string(q) + ")";
        dead = true;
        return fail();
      }
  }

  // the halo plan, from this team's own measurements: what it sends to each peer and where what it receives lands.
  // Both ends order a pair's poses by (sending robot, receiving robot, frame); the hashes below check they agree
  const int na = (int)t->ag.size();
  std::vector<int> offs(na + 1, 0);
  for (int k = 0; k < na; ++k) offs[k + 1] = offs[k] + t->ag[k]->n;
  hoffs.assign(na, 0);
  halo_slots = 0;
  for (int k = 0; k < na; ++k) {
    hoffs[k] = halo_slots;
    halo_slots += (int)t->ag[k]->np.size();
  }
  using Ent = std::tuple<int, int, int, int, int>;  // peer, sending robot, receiving robot, frame, column / halo slot
  std::vector<Ent> se, re;
  for (int lb = 0; lb < na; ++lb) {
    const Agent &B = *t->ag[lb];
    for (int a : B.neighbors) {
      if (t->id2local.count(a)) continue;
      for (int f : public_ids(B, a)) se.emplace_back(owner[a], B.id, a, f, offs[lb] + f);
    }
  }
  for (int la = 0; la < na; ++la) {
    const Agent &A = *t->ag[la];
    for (size_t s = 0; s < A.np.size(); ++s) {
      const int b = A.np[s].first;
      if (t->id2local.count(b)) continue;
      re.emplace_back(owner[b], b, A.id, A.np[s].second, hoffs[la] + (int)s);
    }
  }
  std::sort(se.begin(), se.end());
  std::sort(re.begin(), re.end());
  sent_p.assign(world, 0);
  recv_p.assign(world, 0);
  std::vector<Fnv> sh(world), rh(world);
  scol.clear();
  rdst.clear();
  for (const Ent &e : se) {
    const int p = std::get<0>(e);
    ++sent_p[p];
    sh[p].add(std::get<1>(e)); sh[p].add(std::get<2>(e)); sh[p].add(std::get<3>(e));
    scol.push_back(std::get<4>(e));
  }
  for (const Ent &e : re) {
    const int p = std::get<0>(e);
    ++recv_p[p];
    rh[p].add(std::get<1>(e)); rh[p].add(std::get<2>(e)); rh[p].add(std::get<3>(e));
    rdst.push_back(std::get<4>(e));
  }
  // the detail record: [status, per robot (position in this team + 1 or 0, poses), per peer (sent, hash, received, hash),
  // whether every agent here has a raw preconditioner]
  const size_t R0 = 1, P0 = R0 + 2 * (size_t)num_robots, n = P0 + 4 * (size_t)world + 1;
  std::vector<double> d(n, 0.0);
  for (int k = 0; k < na; ++k) {
    d[R0 + 2 * t->ag[k]->id] = k + 1;
    d[R0 + 2 * t->ag[k]->id + 1] = t->ag[k]->n;
  }
  for (int p = 0; p < world; ++p) {
    d[P0 + 4 * p] = (double)sent_p[p];
    d[P0 + 4 * p + 1] = sh[p].value();
    d[P0 + 4 * p + 2] = (double)recv_p[p];
    d[P0 + 4 * p + 3] = rh[p].value();
  }
  bool pc = true;
  for (auto &a : t->ag)
    if (!a->dev.M && !a->dev.Dinv) pc = false;
  d[n - 1] = pc ? 1.0 : 0.0;
  if (gather(d, hall)) return fail();
  robot_n.assign(num_robots, 0);
  robot_holder.assign(num_robots, -1);
  robot_lidx.assign(num_robots, -1);
  for (int q = 0; q < world; ++q) {
    const double *dq = hall.data() + (size_t)q * n;
    if (dq[n - 1] == 0.0) all_precond = false;
    for (int i = 0; i < num_robots; ++i) {
      if (dq[R0 + 2 * i] == 0.0) continue;
      if (robot_holder[i] >= 0) {
        err = "robot " + std::to_string(i) + " is held by rank " + std::to_string(robot_holder[i]) + " and by rank " +
              std::to_string(q);
        dead = true;
        return fail();
      }
      robot_holder[i] = q;
      robot_lidx[i] = (int)dq[R0 + 2 * i] - 1;
      robot_n[i] = (int)dq[R0 + 2 * i + 1];
    }
    for (int p = 0; p < world; ++p) {
      const double *dp = hall.data() + (size_t)p * n;
      if (dq[P0 + 4 * p] != dp[P0 + 4 * q + 2] || dq[P0 + 4 * p + 1] != dp[P0 + 4 * q + 3]) {
        err = "the shared poses of rank " + std::to_string(q) + " and rank " + std::to_string(p) +
              " disagree (their measurement sets differ)";
        dead = true;
        return fail();
      }
    }
  }
  robot_goff.assign(num_robots, 0);
  nglob = 0;
  for (int i = 0; i < num_robots; ++i) {
    if (robot_holder[i] < 0) {
      err = "robot " + std::to_string(i) + " is held by no participant";
      dead = true;
      return fail();
    }
    robot_goff[i] = nglob;
    nglob += robot_n[i];
  }
  return 0;
}

}  // namespace dpgo_cert

extern "C" {

int dpgo_team_certificate_apply_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, int K,
                                       const double *V, double *out) {
  Across x;
  const char *argerr = (!V || !out) ? "null argument" : (K < 3 || K > 8) ? "K must lie in 3..8" : nullptr;
  if (x.begin(t, tr, owner_rank_of_robot, "certificate_apply_across", 0, K, 0, 0.0, 0.0, 0, argerr)) return DPGO_ERR;
  Cert c;
  c.t = t;
  c.x = &x;
  if (c.setup(K)) return DPGO_ERR;
  const size_t bytes = sizeof(double) * (size_t)K * c.L;
  CERT_CK(c, hipMemcpyAsync(c.T, V, bytes, hipMemcpyHostToDevice, t->stream));
  c.apply(K, c.T, K, c.T2, K, true);
  CERT_CK(c, hipGetLastError());
  CERT_CK(c, hipMemcpyAsync(out, c.T2, bytes, hipMemcpyDeviceToHost, t->stream));
  CERT_CK(c, hipStreamSynchronize(t->stream));
  return x.finish() ? DPGO_ERR : DPGO_OK;
}

int dpgo_team_certify_across(dpgo_team_t *t, const dpgo_transport_t *tr, const int *owner_rank_of_robot, double eta,
                             double tol, int max_iters, int block, int flags, dpgo_certificate_t *out, double *v) {
  Across x;
  const int K = block > 0 ? block : (t ? t->prm.r : 0);
  const char *argerr = !out ? "null argument"
                       : (K < 3 || K > 8) ? "the block size must lie in 3..8"
                       : (max_iters < 1 || !(tol > 0) || !(eta >= 0)) ? "max_iters >= 1, tol > 0 and eta >= 0 required"
                                                                      : nullptr;
  if (x.begin(t, tr, owner_rank_of_robot, "certify_across", 1, K, flags, eta, tol, max_iters, argerr)) return DPGO_ERR;
  Cert c;
  c.t = t;
  c.x = &x;
  return certify_body(c, eta, tol, max_iters, K, flags, out, v);
}

}  // extern "C"
