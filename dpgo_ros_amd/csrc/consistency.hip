// consistency.hip -- pairwise consistency maximisation between two teams that are not joined yet.
//
// Candidate k is a measurement Z_k ~ (T^A_{i_k})^-1 G T^B_{j_k} from a pose of team A to a pose of team B, G unknown and common
// to the true candidates.  For k < l the loop E_kl = Z_l^-1 A_kl Z_k B_kl closes through the segments A_kl = (T^A_{i_l})^-1 T^A_{i_k}
// and B_kl = (T^B_{j_k})^-1 T^B_{j_l} of the two teams' own trajectories; its residual is tested against its covariance
// (consistency_block.h), and the largest set of candidates that agree pairwise is a maximum clique (max_clique.cpp).
//   k_segments     behind each team's covariance path (a CovEpilogue): one 48-double record per distinct segment -- R, t and
//                  Sigma_rel, the arithmetic of k_gate<false> (gate_block.h), in a buffer this call owns
//   k_consistency  one wave per (row k, adjacency word w): lane b forms d2 of the ordered pair (min, max) of k and 64 w + b,
//                  writes it, and the wave's ballot is the adjacency word
#include <chrono>
#include <unordered_map>

#include "closure_frame.h"
#include "consistency_block.h"

namespace dpgo {

// One lane per segment, grid-stride: team poses ij[2 s] != ij[2 s + 1], whose pair block is block s of the staged pairs.
__global__ __launch_bounds__(256) void k_segments(const double *__restrict__ T, const double *__restrict__ diag,
                                                  const double *__restrict__ pairs, const int *__restrict__ ij, int num,
                                                  double *__restrict__ rec) {
  for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < (size_t)num; s += (size_t)gridDim.x * 256) {
    const int i = gp(ij)[2 * s], j = gp(ij)[2 * s + 1];
    double M[3][3], tij[3], S[6][6];
    gate_relative(T, diag, pairs, i, j, (int)s, M, tij, S);
    double *out = rec + (size_t)PCM_SEG * s;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) gp(out)[3 * a + b] = M[a][b];
      gp(out)[9 + a] = tij[a];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) gp(out)[12 + 6 * a + b] = S[a][b];
  }
}

// One wave owns one tile: row k and the 64 columns of adjacency word w; the waves stride over the K W tiles.  fp64 in
// registers, no LDS, no atomics, no sum across lanes: a lane writes its own d2 and one lane the wave's ballot, so two calls
// give the same bits, and both triangles come from the same expression of the ordered pair.  seg[p K + q] (p < q) is the
// record of A_pq in rec_a, seg[q K + p] that of B_pq in rec_b, -1 where the two poses coincide.
__global__ __launch_bounds__(256) void k_consistency(const double *__restrict__ cand, const int *__restrict__ seg,
                                                     const double *__restrict__ rec_a, const double *__restrict__ rec_b, int K, int W,
                                                     double thr2, double *__restrict__ d2, unsigned long long *__restrict__ adj) {
  const int lane = threadIdx.x & 63;
  const size_t tiles = (size_t)K * W, nwaves = (size_t)gridDim.x * 4;
  for (size_t tile = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < tiles; tile += nwaves) {
    const int k = (int)(tile / W), w = (int)(tile % W);
    const int l = 64 * w + lane;
    const bool active = l < K && l != k;
    double d = 0.0;
    if (active) {
      const int p = min(k, l), q = max(k, l);
      const int ia = gp(seg)[(size_t)p * K + q], ib = gp(seg)[(size_t)q * K + p];
      d = pcm_pair(cand + (size_t)PCM_CAND * p, cand + (size_t)PCM_CAND * q, rec_a + (size_t)PCM_SEG * max(ia, 0), ia >= 0,
                   rec_b + (size_t)PCM_SEG * max(ib, 0), ib >= 0, nullptr, nullptr);
    }
    if (l < K) gp(d2)[(size_t)k * K + l] = d;
    const unsigned long long word = __ballot(active && d <= thr2);
    if (lane == 0) gp(adj)[tile] = word;
  }
}

}  // namespace dpgo

namespace dpgo_cert {

namespace {

const ClosureCall PCM = {"pairwise_consistency", "candidate"};

// the step behind one team's staged blocks: the segment records into the buffer of the call
struct SegEpilogue : ClosureEpilogue {
  std::vector<int> ij;  // team poses (i, j) of every segment, the pair list handed to the path
  DevBuf<int> d_ij;
  double *rec = nullptr;
  SegEpilogue() : ClosureEpilogue(2) {}
  int run(const CovStage &st) override {
    const size_t n = ij.size() / 2;
    if ((size_t)st.num_pairs != n) {
      set_err("pairwise_consistency: the covariance path staged another number of pair blocks than there are segments");
      return DPGO_ERR;
    }
    for (int g : ij)
      if (g < 0 || g >= st.N) {
        set_err("pairwise_consistency: a segment lies outside the staged blocks");
        return DPGO_ERR;
      }
    hipStream_t s = st.stream;
    if (d_ij.upload(ij, s)) { set_err("pairwise_consistency: device allocation failed (segment list)"); return DPGO_ERR; }
    if (ev.create()) return DPGO_ERR;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 256);
    HIPC(hipEventRecord(ev[0], s));
    k_segments<<<grid, 256, 0, s>>>(st.Td, st.diag, st.pairs, d_ij.p, (int)n, rec);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ev[1], s));
    ran = true;
    return DPGO_OK;
  }
};

}  // namespace

}  // namespace dpgo_cert

using namespace dpgo_cert;

extern "C" int dpgo_team_pairwise_consistency(dpgo_team_t *a, const double *T_a, dpgo_team_t *b, const double *T_b, int method,
                                              int max_block, int num, const dpgo_measurement_t *cand, double quantile,
                                              long long max_nodes, double *d2, uint64_t *adj, int *members, int *size, int *proven,
                                              dpgo_covariance_t *res_a, dpgo_covariance_t *res_b) {
  // ---- the refusals of the call itself: on the host, before any device work, no output touched
  if (!a || !b || !T_a || !T_b || !members || !size || !proven || !res_a || !res_b) return PCM.refuse("null argument");
  if (num <= 0) return PCM.refuse("num must be positive, not " + std::to_string(num));
  if (!cand) return PCM.refuse("null argument");
  if (PCM.check_method(method)) return DPGO_ERR;
  if (!(quantile > 0.0 && quantile < 1.0)) {
    char buf[120];
    std::snprintf(buf, sizeof buf, "quantile must lie inside (0, 1), not %.6g", quantile);
    return PCM.refuse(buf);
  }
  if (max_nodes < 0) return PCM.refuse("max_nodes must not be negative (0: no limit), not " + std::to_string(max_nodes));
  if (check_team_local(a, PCM.name) || check_team_local(b, PCM.name)) return DPGO_ERR;
  if (a->device != b->device)
    return PCM.refuse("the teams are on different devices (" + std::to_string(a->device) + " and " + std::to_string(b->device) + ")");
  const std::vector<int> offs_a = pose_offsets(a), offs_b = pose_offsets(b);
  const size_t K = (size_t)num, W = (K + 63) / 64;
  std::vector<int> pi(K), pj(K);
  std::vector<double> h_cand(dpgo::PCM_CAND * K, 0.0);
  for (int k = 0; k < num; ++k) {
    const dpgo_measurement_t &m = cand[k];
    if (PCM.endpoint(a, offs_a, k, m.r1, m.p1, &pi[k], "A") || PCM.endpoint(b, offs_b, k, m.r2, m.p2, &pj[k], "B") || PCM.check(k, m))
      return DPGO_ERR;
    pack_measurement(m, h_cand.data() + dpgo::PCM_CAND * (size_t)k);
  }
  // ---- the segments: per team the distinct ordered pose pairs in order of first use, and the table of their indices
  SegEpilogue epi_a, epi_b;
  std::vector<int> seg(K * K, -1);
  {
    std::unordered_map<unsigned long long, int> of_a, of_b;
    auto index_of = [](std::unordered_map<unsigned long long, int> &of, std::vector<int> &list, int i, int j) {
      const auto ins = of.insert({((unsigned long long)(unsigned)i << 32) | (unsigned)j, (int)of.size()});
      if (ins.second) { list.push_back(i); list.push_back(j); }
      return ins.first->second;
    };
    for (size_t k = 0; k < K; ++k)
      for (size_t l = k + 1; l < K; ++l) {
        if (pi[l] != pi[k]) seg[k * K + l] = index_of(of_a, epi_a.ij, pi[l], pi[k]);
        if (pj[k] != pj[l]) seg[l * K + k] = index_of(of_b, epi_b.ij, pj[k], pj[l]);
      }
  }
  const size_t na = epi_a.ij.size() / 2, nb = epi_b.ij.size() / 2;
  const double thr = dpgo_error_threshold_at_quantile(quantile, 6), thr2 = thr * thr;
  HIPC(hipSetDevice(a->device));
  const size_t rec_doubles = (size_t)dpgo::PCM_SEG * (std::max<size_t>(na, 1) + std::max<size_t>(nb, 1));
  // what the call itself stages on the device: candidates, segment lists and records, the table, d2 and the adjacency words
  const double staged = 8.0 * ((double)h_cand.size() + (double)rec_doubles + (double)(K * K) + (double)(K * W)) + 4.0 * (double)(K * K) +
                        8.0 * (double)(na + nb);
  {
    size_t free_b = 0, total_b = 0;
    HIPC(hipMemGetInfo(&free_b, &total_b));
    const double avail = (double)free_b + (double)pool_held(a->device);
    if (staged > avail) {
      char buf[300];
      std::snprintf(buf, sizeof buf, "%d candidates with %zu + %zu segments stage %.0f bytes, %.0f are available on the device", num, na,
                    nb, staged, avail);
      return PCM.refuse(buf);
    }
  }
  DevBuf<double> d_cand, d_rec, d_d2;
  DevBuf<int> d_seg;
  DevBuf<unsigned long long> d_adj;
  if (d_cand.alloc(h_cand.size()) || d_rec.alloc(rec_doubles) || d_d2.alloc(K * K) || d_seg.alloc(K * K) || d_adj.alloc(K * W))
    return PCM.refuse("device allocation failed (" + std::to_string(num) + " candidates, " + std::to_string(na + nb) + " segments)");
  epi_a.rec = d_rec.p;
  epi_b.rec = d_rec.p + (size_t)dpgo::PCM_SEG * std::max<size_t>(na, 1);
  // ---- each team's covariance path, with its own refusals and messages; a team that needs no segment is not asked
  dpgo_covariance_t ra, rb;
  std::memset(&ra, 0, sizeof ra);
  std::memset(&rb, 0, sizeof rb);
  Events span_a(2), span_b(2), span_k(2);
  auto path = [&](dpgo_team_t *t, const double *T, SegEpilogue &epi, dpgo_covariance_t *res, Events &span) -> int {
    const int np = (int)(epi.ij.size() / 2);
    if (np == 0) return DPGO_OK;
    if (span.create()) return DPGO_ERR;
    HIPC(hipEventRecord(span[0], t->stream));
    if (const int rc = PCM.path(t, T, method, max_block, np, epi.ij.data(), res, epi)) return rc;
    HIPC(hipEventRecord(span[1], t->stream));
    HIPC(hipStreamSynchronize(t->stream));
    return DPGO_OK;
  };
  if (const int rc = path(a, T_a, epi_a, &ra, span_a)) return rc;
  if (const int rc = path(b, T_b, epi_b, &rb, span_b)) return rc;
  // ---- the K x K statistics and the adjacency words (both paths have drained their streams: the records are complete)
  hipStream_t s = a->stream;
  std::vector<double> h_d2(d2 ? K * K : 0);
  std::vector<uint64_t> h_adj(K * W);
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "adjacency words");
  HIPC(hipMemcpyAsync(d_cand.p, h_cand.data(), sizeof(double) * h_cand.size(), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(d_seg.p, seg.data(), sizeof(int) * seg.size(), hipMemcpyHostToDevice, s));
  if (span_k.create()) return DPGO_ERR;
  HIPC(hipEventRecord(span_k[0], s));
  // at most one workgroup per CU of an MI355X, four tiles in flight each: the waves beyond stride over the rest
  const unsigned grid = (unsigned)std::min<size_t>((K * W + 3) / 4, 256);
  dpgo::k_consistency<<<grid, 256, 0, s>>>(d_cand.p, d_seg.p, epi_a.rec, epi_b.rec, num, (int)W, thr2, d_d2.p, d_adj.p);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(span_k[1], s));
  if (d2) HIPC(hipMemcpyAsync(h_d2.data(), d_d2.p, sizeof(double) * K * K, hipMemcpyDeviceToHost, s));
  HIPC(hipMemcpyAsync(h_adj.data(), d_adj.p, sizeof(uint64_t) * K * W, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  // ---- the largest pairwise-consistent set, on the host
  std::vector<int> mem(K);
  int sz = 0, prv = 0;
  const auto t0 = std::chrono::steady_clock::now();
  if (dpgo_max_clique(num, h_adj.data(), max_nodes, mem.data(), &sz, &prv) != DPGO_OK) return DPGO_ERR;
  const double clique_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  static const bool timing = std::getenv("DPGO_TIMING") != nullptr;
  if (timing) {
    std::fprintf(stderr,
                 "pairwise_consistency: %d candidates, %zu + %zu segments, path A %.3f ms, path B %.3f ms, segment kernels %.3f + %.3f ms, "
                 "k_consistency %.3f ms, clique %.3f ms on the host (%d members, %s), %.0f bytes staged\n",
                 num, na, nb, span_a.ms(), span_b.ms(), epi_a.ev.ms(), epi_b.ev.ms(), span_k.ms(), clique_ms, sz, prv ? "proven" : "not proven",
                 staged);
  }
  if (d2) std::memcpy(d2, h_d2.data(), sizeof(double) * K * K);
  if (adj) std::memcpy(adj, h_adj.data(), sizeof(uint64_t) * K * W);
  std::memcpy(members, mem.data(), sizeof(int) * (size_t)sz);
  *size = sz;
  *proven = prv;
  *res_a = ra;
  *res_b = rb;
  return DPGO_OK;
}

// Not part of the public interface (include/dpgo_hip.h does not declare it): the segment records of one team as the call above
// forms them, for the tests -- rec receives 48 doubles per pair (R row-major, t, Sigma_rel), pairs as in the covariance calls.
extern "C" int dpgo_internal_segment_records(dpgo_team_t *t, const double *T, int method, int max_block, int num_pairs, const int *pairs,
                                             double *rec, dpgo_covariance_t *res) {
  if (!t || !T || !pairs || !rec || !res || num_pairs <= 0) return PCM.refuse("segment_records: null argument or no pairs");
  if (check_team_local(t, "pairwise_consistency")) return DPGO_ERR;
  HIPC(hipSetDevice(t->device));
  SegEpilogue epi;
  epi.ij.assign(pairs, pairs + 2 * (size_t)num_pairs);
  DevBuf<double> d_rec;
  if (d_rec.alloc((size_t)dpgo::PCM_SEG * num_pairs)) return PCM.refuse("segment_records: device allocation failed");
  epi.rec = d_rec.p;
  if (const int rc = PCM.path(t, T, method, max_block, num_pairs, pairs, res, epi)) return rc;
  HIPC(hipMemcpy(rec, d_rec.p, sizeof(double) * dpgo::PCM_SEG * (size_t)num_pairs, hipMemcpyDeviceToHost));
  return DPGO_OK;
}
