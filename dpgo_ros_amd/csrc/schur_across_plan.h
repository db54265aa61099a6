// schur_across_plan.h -- the host-only half of the robot-wise Schur path over a split team (covariance_schur.hip, SchurAcross;
// DESIGN.md 5e, "across teams"): who is public and who is interior, the hash of the agreement record, and the layout of every
// record the path sends -- each written ONCE, so that the side that packs and the side that parses cannot drift apart.  Plain
// functions and structs over std::vector, no HIP include: tests/test_schur_across_plan_host.py compiles this header alone.
//   A  per robot three sizes: its public poses, its interior poses, the cross blocks it holds (a_put, a_take);
//   B  a header of B_HDR doubles, then per robot of the participant in id order (BRobot): the frames of its public poses, its
//      diagonal block of the Schur complement, the four statistics of its factor, its cross blocks of 39 doubles (b_pack,
//      assemble), padded to the longest record (pmax);
//   C  the status word, the pair blocks the participant owns in pair order (pairoff), the rows W_a[i,:] of the pairs of two
//      robots' interiors it holds (rowoff), and with Sigma applied to vectors every robot's r_a (rat), padded to cmax;
//   D  HeldRecord: per compact pose a payload from the participant that holds it, zeros from everyone else.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

namespace dpgo {

// a list entry of the extraction (covariance_extract.h): output block blk, set b (or -1), two indices, one flag
struct CovBlk {
  int blk, b, i, j, f, pad_;
};
// a pair of interior poses of two sets: output block, set and interior index of the left pose, then of the right one
struct CovCross {
  int blk, ba, li, bb, lj, pad_;
};

}  // namespace dpgo

namespace dpgo_cert {
using namespace dpgo;

// FNV-1a over the bytes of what every participant must pass alike, as a double that an allgather carries exactly
struct RecordHash {
  unsigned long long h = 1469598103934665603ull;
  void add(const void *p, size_t bytes) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t k = 0; k < bytes; ++k) { h ^= b[k]; h *= 1099511628211ull; }
  }
  void add(int v) { add(&v, sizeof v); }
  void add(double v) { add(&v, sizeof v); }
  double value() const { return (double)(h & ((1ull << 52) - 1)); }
};

// who is public, who is interior among a team's poses; the fixed pose (team index `zero`, -1: not in this
// team) belongs to neither set
struct SchurPartition {
  int na = 0, N = 0, nS = 0, max_int = 0;
  std::vector<int> offs, robot_of, pos, sep, sep_off;  // pos: index inside the pose's own set; sep: team pose of separator index
  std::vector<char> pub;
  std::vector<std::vector<int>> interior;              // team poses of robot a's interior, in order
};

// "Per compact pose a payload of `width` doubles from its holder, zeros from everyone else", behind the status word: allgather D
// of the path (48: T and the diagonal block of a record's endpoint) and allgather E of the update across teams (12: T).
struct HeldRecord {
  size_t width;
  std::vector<int> holder;  // the rank that holds pose e
  size_t len() const { return 1 + width * holder.size(); }
  double *mine(std::vector<double> &rec, size_t e) const { return rec.data() + 1 + width * e; }
  const double *from(const std::vector<double> &all, size_t e) const { return all.data() + (size_t)holder[e] * len() + 1 + width * e; }
};

struct SchurAcrossPlan {
  // ---- what the agreement left on every participant: robots by id, poses numbered robot after robot
  int rank = 0, world = 1, nr = 0;
  std::vector<int> holder, robot_n, local_of, local_id;  // local_of: robot id -> its index here (-1: held elsewhere), local_id back
  std::vector<long long> goff;
  long long NG = 0;
  std::vector<int> grobot, gframe;  // global pose -> robot, frame

  void init(int rank_, int world_, const std::vector<int> &holder_, const std::vector<int> &robot_n_, const std::vector<int> &local_of_) {
    rank = rank_; world = world_; holder = holder_; robot_n = robot_n_; local_of = local_of_;
    nr = (int)holder.size();
    goff.assign(nr + 1, 0);
    int na = 0;
    for (int i = 0; i < nr; ++i) { goff[i + 1] = goff[i] + robot_n[i]; na += local_of[i] >= 0; }
    NG = goff[nr];
    local_id.assign(na, 0);
    grobot.resize((size_t)NG); gframe.resize((size_t)NG);
    for (int i = 0; i < nr; ++i) {
      if (local_of[i] >= 0) local_id[local_of[i]] = i;
      for (int f = 0; f < robot_n[i]; ++f) { grobot[goff[i] + f] = i; gframe[goff[i] + f] = f; }
    }
  }
  bool here(int g) const { return holder[grobot[g]] == rank; }

  // ---- allgather A: the sizes
  std::vector<int> gs, gc, gsoff;  // per robot: its public poses, its cross blocks, its place in the separator
  int nSp = 0, nS = 0, kmax = 0;       // the separator of the whole problem in poses and in rows; the widest robot part
  size_t a_len() const { return 1 + 3 * (size_t)nr; }
  static void a_put(std::vector<double> &ga, int id, int pub, int interior, int cross) {
    ga[1 + 3 * (size_t)id] = pub; ga[2 + 3 * (size_t)id] = interior; ga[3 + 3 * (size_t)id] = cross;
  }
  void a_take(const std::vector<double> &gall) {
    gs.assign(nr, 0); gc.assign(nr, 0); gsoff.assign(nr + 1, 0);
    kmax = 0;
    for (int i = 0; i < nr; ++i) {
      const double *q = gall.data() + (size_t)holder[i] * a_len();
      gs[i] = (int)q[1 + 3 * i]; gc[i] = (int)q[3 + 3 * i];  // (the interior count travels for the record's sake)
      gsoff[i + 1] = gsoff[i] + gs[i];
      kmax = std::max(kmax, 6 * gs[i]);
    }
    nSp = gsoff[nr]; nS = 6 * nSp;
    // B: every robot's part behind its holder's header, in id order
    std::vector<size_t> plen((size_t)world, (size_t)B_HDR);
    bstart.assign(nr, 0);
    for (int i = 0; i < nr; ++i) { bstart[i] = plen[holder[i]]; plen[holder[i]] += b_robot(i).end; }
    pmax = *std::max_element(plen.begin(), plen.end());
  }

  // ---- allgather B
  enum { B_STATUS = 0, B_CODE, B_ROBOT, B_POSE, B_ROW, B_SPARE, B_HDR };  // the header: status, failure code, robot, pose, row, spare
  enum { B_CROSS = 39 };                                                  // a cross block: row, column robot, column frame, 36 doubles
  struct BRobot { size_t frames, diag, stat, cross, end; };               // where a robot's fields lie behind its start
  BRobot b_robot(int i) const {
    const size_t s = (size_t)gs[i], stat = s + 36 * s * s;
    return {0, s, stat, stat + 4, stat + 4 + (size_t)gc[i] * B_CROSS};
  }
  std::vector<size_t> bstart;  // robot i's start inside its holder's record
  size_t pmax = 0;
  // a block of H_SS below the diagonal in a row the robot holds (the row-owner rule): row among the robot's public poses; the
  // column pose by robot and frame; blk 6 x 6 column-major, H[row pose, column pose]
  struct BCross { int lrow, crobot, cframe; const double *blk; };
  // robot `id` of this participant into its record: frames of its public poses (ascending), its diagonal block (6 s x 6 s
  // column-major), the statistics, its gc[id] cross blocks
  void b_pack(std::vector<double> &gb, int id, const int *frames, const double *diag, const double stat[4], const std::vector<BCross> &cross) const {
    const BRobot f = b_robot(id);
    double *r = gb.data() + bstart[id];
    for (int q = 0; q < gs[id]; ++q) r[f.frames + q] = frames[q];
    if (f.stat > f.diag) std::memcpy(r + f.diag, diag, sizeof(double) * (f.stat - f.diag));
    std::memcpy(r + f.stat, stat, sizeof(double) * 4);
    for (size_t b = 0; b < cross.size() && b < (size_t)gc[id]; ++b) {
      double *c = r + f.cross + B_CROSS * b;
      c[0] = cross[b].lrow; c[1] = cross[b].crobot; c[2] = cross[b].cframe;
      std::memcpy(c + 3, cross[b].blk, sizeof(double) * 36);
    }
  }
  const double *b_header(const std::vector<double> &gall, int q) const { return gall.data() + (size_t)q * pmax; }

  // ---- S_c of the whole problem from the gathered B, the same on every participant
  std::vector<std::vector<int>> pubf;  // per robot the frames of its public poses
  std::vector<double> rstat;           // per robot the statistics of its factor
  std::vector<char> gpub;              // every pose of the problem: its set and its index there
  std::vector<int> gpos;
  // the separator index of a robot's frame, -1 when the robot does not list it as public
  int sep_index(int robot, int frame) const {
    if (robot < 0 || robot >= nr) return -1;
    const auto &v = pubf[robot];
    const auto it = std::lower_bound(v.begin(), v.end(), frame);
    return (it != v.end() && *it == frame) ? gsoff[robot] + (int)(it - v.begin()) : -1;
  }
  // hS (nS x nS, column-major): the diagonal blocks, and every cross block at (row, column) and transposed at (column, row).
  // false: torn -- a cross block names a pose that its robot does not list as public (it is skipped)
  bool assemble(const std::vector<double> &gall, std::vector<double> &hS) {
    pubf.assign(nr, {});
    rstat.assign(4 * (size_t)nr, 0.0);
    hS.assign((size_t)nS * nS, 0.0);
    for (int i = 0; i < nr; ++i) {
      const double *r = b_header(gall, holder[i]) + bstart[i] + b_robot(i).frames;
      pubf[i].resize(gs[i]);
      for (int k = 0; k < gs[i]; ++k) pubf[i][k] = (int)r[k];
    }
    bool whole = true;
    for (int i = 0; i < nr; ++i) {
      const BRobot f = b_robot(i);
      const double *r = b_header(gall, holder[i]) + bstart[i];
      const size_t w = 6 * (size_t)gs[i], so = 6 * (size_t)gsoff[i];
      for (size_t cc = 0; cc < w; ++cc) std::memcpy(hS.data() + (so + cc) * nS + so, r + f.diag + cc * w, sizeof(double) * w);
      for (int k = 0; k < 4; ++k) rstat[4 * i + k] = r[f.stat + k];
      for (int b = 0; b < gc[i]; ++b) {
        const double *c = r + f.cross + (size_t)B_CROSS * b;
        const int lrow = (int)c[0], col = sep_index((int)c[1], (int)c[2]);
        if (col < 0 || lrow < 0 || lrow >= gs[i]) { whole = false; continue; }
        const int row = gsoff[i] + lrow;
        const double *blk = c + 3;
        for (int bb = 0; bb < 6; ++bb)
          for (int aa = 0; aa < 6; ++aa) {
            hS[((size_t)6 * col + bb) * nS + (size_t)6 * row + aa] = blk[6 * bb + aa];
            hS[((size_t)6 * row + aa) * nS + (size_t)6 * col + bb] = blk[6 * bb + aa];
          }
      }
    }
    gpub.assign((size_t)NG, 0);
    gpos.assign((size_t)NG, 0);
    for (int i = 0; i < nr; ++i) {
      for (int k = 0; k < gs[i]; ++k)
        if (pubf[i][k] >= 0 && pubf[i][k] < robot_n[i]) { gpub[goff[i] + pubf[i][k]] = 1; gpos[goff[i] + pubf[i][k]] = gsoff[i] + k; }
      int cnt = 0;
      for (int f = (i == 0 ? 1 : 0); f < robot_n[i]; ++f)
        if (!gpub[goff[i] + f]) gpos[goff[i] + f] = cnt++;
    }
    return whole;
  }

  // ---- the pairs, by case.  A pair with the fixed pose (global pose 0) is zeros and on no list.  Two public poses: everyone
  // reads the block of Sigma_SS (pub_list).  Two interior poses of one robot: its holder owns the pair (keep_list and
  // same_list of that robot, known before the robot's step: its blocks of C_a are kept).  An interior with a public pose, in
  // either order: the holder of the interior pose's robot owns it (is_list; flag 1: the caller's order is (public,
  // interior)).  Interiors of two robots: everyone forms it from the two rows W_a[i,:], W_b[j,:] that their holders send
  // (rows, two per pair in pair order).  A list entry's block is N + k: the pair blocks lie behind the N diagonal ones.
  struct RowReq { int pair, robot, li; };
  std::vector<std::vector<CovBlk>> keep_list, same_list;
  std::vector<CovBlk> pub_list, is_list;
  std::vector<int> pair_owner;  // -1: everyone (or zeros)
  std::vector<RowReq> rows;

  // before allgather B, from this participant's own partition: the kept blocks of its robots
  void same_robot_pairs(const SchurPartition &P, const int *pairs, int num_pairs) {
    keep_list.assign(P.na, {}); same_list.assign(P.na, {});
    for (int k = 0; k < P.na; ++k)
      for (int g : P.interior[k]) keep_list[k].push_back({g, k, P.pos[g], P.pos[g], 0, 0});
    for (int k = 0; k < num_pairs; ++k) {
      const int a = pairs[2 * k], b = pairs[2 * k + 1];
      if (a == 0 || b == 0 || grobot[a] != grobot[b] || !here(a)) continue;
      const int lk = local_of[grobot[a]], la = P.offs[lk] + gframe[a], lb = P.offs[lk] + gframe[b];
      if (P.pub[la] || P.pub[lb]) continue;
      keep_list[lk].push_back({P.N + k, lk, P.pos[la], P.pos[lb], 0, 0});
      same_list[lk].push_back({P.N + k, lk, P.pos[la], P.pos[lb], 0, 0});
    }
  }
  // the number of pairs of two robots' poses, an upper bound of rows.size() / 2 known before allgather B
  size_t two_robot_pairs(const int *pairs, int num_pairs) const {
    size_t n = 0;
    for (int k = 0; k < num_pairs; ++k) n += (pairs[2 * k] && pairs[2 * k + 1] && grobot[pairs[2 * k]] != grobot[pairs[2 * k + 1]]);
    return n;
  }

  // behind assemble(): the other lists and the layout of C.  cols: the columns Sigma is applied to (0: none)
  std::vector<size_t> clen, pairoff, rowoff, rat;  // per rank its length; where an owned pair, a row, a robot's r_a lies in its record
  size_t rows_max = 0, cmax = 0;                   // the longest record without the r_a (what the rows are staged in), and with
  void classify(const SchurPartition &P, const int *pairs, int num_pairs, int cols) {
    pub_list.clear(); is_list.clear(); rows.clear();
    pair_owner.assign(num_pairs, -1);
    for (int k = 0; k < P.na; ++k)
      for (int q = P.sep_off[k]; q < P.sep_off[k + 1]; ++q) {
        const int gsx = gsoff[local_id[k]] + (q - P.sep_off[k]);
        pub_list.push_back({P.sep[q], -1, gsx, gsx, 1, 0});
      }
    for (int k = 0; k < num_pairs; ++k) {
      const int a = pairs[2 * k], b = pairs[2 * k + 1], blk = P.N + k;
      if (a == 0 || b == 0) continue;
      const int ra = grobot[a], rb = grobot[b];
      if (gpub[a] && gpub[b]) pub_list.push_back({blk, -1, gpos[a], gpos[b], 0, 0});
      else if (!gpub[a] && !gpub[b]) {
        if (ra == rb) pair_owner[k] = holder[ra];
        else { rows.push_back({k, ra, gpos[a]}); rows.push_back({k, rb, gpos[b]}); }
      } else if (!gpub[a]) {
        pair_owner[k] = holder[ra];
        if (pair_owner[k] == rank) is_list.push_back({blk, local_of[ra], gpos[a], gpos[b], 0, 0});
      } else {
        pair_owner[k] = holder[rb];
        if (pair_owner[k] == rank) is_list.push_back({blk, local_of[rb], gpos[b], gpos[a], 1, 0});
      }
    }
    clen.assign(world, 1);
    pairoff.assign(num_pairs, 0); rowoff.assign(rows.size(), 0); rat.assign(nr, 0);
    for (int k = 0; k < num_pairs; ++k)
      if (pair_owner[k] >= 0) { pairoff[k] = clen[pair_owner[k]]; clen[pair_owner[k]] += 36; }
    for (size_t r = 0; r < rows.size(); ++r) { rowoff[r] = clen[holder[rows[r].robot]]; clen[holder[rows[r].robot]] += row_len(r); }
    rows_max = *std::max_element(clen.begin(), clen.end());
    for (int i = 0; cols > 0 && i < nr; ++i) { rat[i] = clen[holder[i]]; clen[holder[i]] += (size_t)6 * gs[i] * cols; }
    cmax = *std::max_element(clen.begin(), clen.end());
  }
  size_t row_len(size_t r) const { return 36 * (size_t)gs[rows[r].robot]; }  // W_a[i,:]: 6 x 6 s_a, column-major

  // ---- allgather C.  blocks: the pair blocks in pair order, 36 doubles each; staged: the rows this participant holds, at their
  // places in a record of rows_max doubles; ra: robot id's r_a, 6 s_a x cols
  void c_pack(std::vector<double> &gcv, const double *blocks, const std::vector<double> &staged) const {
    for (size_t k = 0; k < pair_owner.size(); ++k)
      if (pair_owner[k] == rank) std::memcpy(gcv.data() + pairoff[k], blocks + 36 * k, sizeof(double) * 36);
    for (size_t r = 0; r < rows.size(); ++r)
      if (holder[rows[r].robot] == rank) std::memcpy(gcv.data() + rowoff[r], staged.data() + rowoff[r], sizeof(double) * row_len(r));
  }
  void c_pack_ra(std::vector<double> &gcv, int id, const double *ra, int cols) const {
    const size_t len = (size_t)6 * gs[id] * cols;
    if (len > 0) std::memcpy(gcv.data() + rat[id], ra, sizeof(double) * len);
  }
  // the owned pair blocks of every participant into `blocks`; the others stay as they are
  void c_unpack_pairs(const std::vector<double> &gall, double *blocks) const {
    for (size_t k = 0; k < pair_owner.size(); ++k)
      if (pair_owner[k] >= 0) std::memcpy(blocks + 36 * k, gall.data() + (size_t)pair_owner[k] * cmax + pairoff[k], sizeof(double) * 36);
  }
  const double *c_row(const std::vector<double> &gall, size_t r) const { return gall.data() + (size_t)holder[rows[r].robot] * cmax + rowoff[r]; }
  // r_S (nS x cols, column-major) of the whole problem from every robot's r_a
  void c_unpack_rs(const std::vector<double> &gall, int cols, std::vector<double> &hrS) const {
    hrS.assign((size_t)nS * cols, 0.0);
    for (int i = 0; i < nr; ++i) {
      const size_t w = (size_t)6 * gs[i];
      const double *src = gall.data() + (size_t)holder[i] * cmax + rat[i];
      for (int c = 0; c < cols && w > 0; ++c) std::memcpy(hrS.data() + (size_t)c * nS + (size_t)6 * gsoff[i], src + (size_t)c * w, sizeof(double) * w);
    }
  }
};

}  // namespace dpgo_cert
