"""CPU check of csrc/schur_across_plan.h, the record layouts of the robot-wise Schur path over a split team (DESIGN.md 5e,
"across teams"), compiled for the host: a stand-alone program plays every participant of a small split problem in one process
-- it packs each participant's records with the functions the path packs them with, concatenates them as an allgather does and
parses them with the functions the path parses them with.  What comes out is compared here with what numpy builds directly from
the same blocks: S_c of the whole problem byte for byte, the torn verdict, the case of every pair on every rank, the tiling of
allgather C, the per-pose payloads of allgathers D and E, and the hash of the agreement record against its first formula.  The
same program runs once more under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import ROOT

F = np.float64

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "schur_across_plan.h"
using namespace dpgo_cert;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Robot {
  int holder, n;
  std::vector<int> frames;
  std::vector<int> cross;       // lrow, crobot, cframe per block
  std::vector<double> crossblk, diag, stat;
};

// the partition of covariance_schur.hip's schur_partition for the robots rank q holds, in id order
static SchurPartition partition(const std::vector<Robot> &R, int q, std::vector<int> &local_of) {
  SchurPartition P;
  local_of.assign(R.size(), -1);
  std::vector<int> ids;
  for (size_t i = 0; i < R.size(); ++i)
    if (R[i].holder == q) { local_of[i] = (int)ids.size(); ids.push_back((int)i); }
  P.na = (int)ids.size();
  P.offs.assign(P.na + 1, 0);
  for (int k = 0; k < P.na; ++k) P.offs[k + 1] = P.offs[k] + R[ids[k]].n;
  P.N = P.offs[P.na];
  P.robot_of.assign(P.N, 0); P.pub.assign(P.N, 0); P.pos.assign(P.N, 0);
  P.interior.assign(P.na, {});
  P.sep_off.assign(P.na + 1, 0);
  for (int k = 0; k < P.na; ++k) {
    for (int f : R[ids[k]].frames) P.pub[P.offs[k] + f] = 1;
    for (int g = P.offs[k]; g < P.offs[k + 1]; ++g) {
      P.robot_of[g] = k;
      if (ids[k] == 0 && g == P.offs[k]) continue;  // the fixed pose
      if (P.pub[g]) { P.pos[g] = (int)P.sep.size(); P.sep.push_back(g); }
      else { P.pos[g] = (int)P.interior[k].size(); P.interior[k].push_back(g); }
    }
    P.sep_off[k + 1] = (int)P.sep.size();
    P.max_int = std::max(P.max_int, (int)P.interior[k].size());
  }
  P.nS = (int)P.sep.size();
  return P;
}

static double pair_value(int k, int e) { return 1000.0 * k + e + 0.5; }
static double row_value(size_t r, size_t e) { return -(100.0 * (double)r + (double)e + 0.25); }
static double ra_value(int i, int c, size_t j) { return 7.0 * i + 0.125 * c + 1e-3 * (double)j; }

// allgathers D and E: per pose a payload of `width` doubles from its holder (pose 0's is zero with its holder too)
static int held_records(size_t width) {
  const int world = 3;
  const HeldRecord rec{width, {0, 1, 0, 2, 1}};
  const size_t E = rec.holder.size();
  CHECK(rec.len() == 1 + width * E);
  std::vector<double> all;
  for (int q = 0; q < world; ++q) {
    std::vector<double> mine(rec.len(), 0.0);
    for (size_t e = 1; e < E; ++e)
      if (rec.holder[e] == q)
        for (size_t j = 0; j < width; ++j) rec.mine(mine, e)[j] = 10.0 * (double)e + (double)j + 1.0;
    all.insert(all.end(), mine.begin(), mine.end());
  }
  for (size_t e = 0; e < E; ++e)
    for (size_t j = 0; j < width; ++j) {
      CHECK(rec.from(all, e)[j] == (e == 0 ? 0.0 : 10.0 * (double)e + (double)j + 1.0));
      for (int q = 0; q < world; ++q)  // zeros from everyone else
        if (q != rec.holder[e]) CHECK(all[(size_t)q * rec.len() + 1 + width * e + j] == 0.0);
    }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[256];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 256, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  size_t o = 0;
  const int world = (int)in[o++], nr = (int)in[o++], cols = (int)in[o++], np = (int)in[o++], nh = (int)in[o++];
  std::vector<Robot> R(nr);
  for (Robot &r : R) {
    r.holder = (int)in[o++]; r.n = (int)in[o++];
    const int s = (int)in[o++];
    for (int k = 0; k < s; ++k) r.frames.push_back((int)in[o++]);
    const int c = (int)in[o++];
    for (int b = 0; b < c; ++b) {
      for (int k = 0; k < 3; ++k) r.cross.push_back((int)in[o++]);
      r.crossblk.insert(r.crossblk.end(), in.begin() + o, in.begin() + o + 36);
      o += 36;
    }
    r.diag.assign(in.begin() + o, in.begin() + o + 36 * (size_t)s * s); o += 36 * (size_t)s * s;
    r.stat.assign(in.begin() + o, in.begin() + o + 4); o += 4;
  }
  std::vector<int> pairs, hints;
  for (int k = 0; k < 2 * np; ++k) pairs.push_back((int)in[o++]);
  for (int k = 0; k < nh; ++k) hints.push_back((int)in[o++]);
  CHECK(o == in.size());

  std::vector<int> holder, robot_n;
  for (const Robot &r : R) { holder.push_back(r.holder); robot_n.push_back(r.n); }
  std::vector<SchurAcrossPlan> pl(world);
  std::vector<SchurPartition> P(world);
  // ---- allgather A
  std::vector<double> gall;
  for (int q = 0; q < world; ++q) {
    std::vector<int> local_of;
    P[q] = partition(R, q, local_of);
    pl[q].init(q, world, holder, robot_n, local_of);
    std::vector<double> ga(pl[q].a_len(), 0.0);
    for (int i = 0; i < nr; ++i)
      if (holder[i] == q)
        SchurAcrossPlan::a_put(ga, i, (int)R[i].frames.size(), R[i].n - (int)R[i].frames.size() - (i == 0 ? 1 : 0), (int)R[i].cross.size() / 3);
    gall.insert(gall.end(), ga.begin(), ga.end());
  }
  for (int q = 0; q < world; ++q) {
    pl[q].a_take(gall);
    pl[q].same_robot_pairs(P[q], pairs.data(), np);
    CHECK(pl[q].pmax == pl[0].pmax && pl[q].nS == pl[0].nS);
  }
  // ---- allgather B and S_c, the same on every participant
  gall.clear();
  for (int q = 0; q < world; ++q) {
    std::vector<double> gb(pl[q].pmax, 0.0);
    for (int i = 0; i < nr; ++i) {
      if (holder[i] != q) continue;
      std::vector<SchurAcrossPlan::BCross> cross;
      for (size_t b = 0; b < R[i].cross.size() / 3; ++b)
        cross.push_back({R[i].cross[3 * b], R[i].cross[3 * b + 1], R[i].cross[3 * b + 2], R[i].crossblk.data() + 36 * b});
      pl[q].b_pack(gb, i, R[i].frames.data(), R[i].diag.data(), R[i].stat.data(), cross);
    }
    gall.insert(gall.end(), gb.begin(), gb.end());
  }
  std::vector<std::vector<double>> hS(world);
  bool whole = true;
  for (int q = 0; q < world; ++q) {
    const bool w = pl[q].assemble(gall, hS[q]);
    if (q == 0) whole = w;
    CHECK(w == whole && hS[q] == hS[0] && pl[q].pubf == pl[0].pubf && pl[q].rstat == pl[0].rstat && pl[q].gpub == pl[0].gpub &&
          pl[q].gpos == pl[0].gpos);
  }
  // ---- the pair lists and allgather C
  std::vector<double> call;
  for (int q = 0; q < world; ++q) {
    SchurAcrossPlan &p = pl[q];
    p.classify(P[q], pairs.data(), np, cols);
    CHECK(p.pair_owner == pl[0].pair_owner && p.clen == pl[0].clen && p.cmax == pl[0].cmax && p.rows_max == pl[0].rows_max &&
          p.rowoff == pl[0].rowoff && p.pairoff == pl[0].pairoff && p.rat == pl[0].rat && p.rows.size() == pl[0].rows.size());
  }
  for (int q = 0; q < world; ++q) {
    const SchurAcrossPlan &p = pl[q];
    // what rank q sends tiles its record: no overlap, no gap
    std::vector<std::pair<size_t, size_t>> seg = {{0, 1}};
    for (int k = 0; k < np; ++k)
      if (p.pair_owner[k] == q) seg.push_back({p.pairoff[k], 36});
    for (size_t r = 0; r < p.rows.size(); ++r)
      if (holder[p.rows[r].robot] == q) seg.push_back({p.rowoff[r], p.row_len(r)});
    size_t before_ra = 1;
    for (const auto &sg : seg) before_ra = std::max(before_ra, sg.first + sg.second);
    CHECK(before_ra <= p.rows_max);
    for (int i = 0; cols > 0 && i < nr; ++i)
      if (holder[i] == q) seg.push_back({p.rat[i], (size_t)6 * p.gs[i] * cols});
    std::sort(seg.begin(), seg.end());
    size_t at = 0;
    for (const auto &sg : seg) { CHECK(sg.first == at || sg.second == 0); at += sg.second; }
    CHECK(at == p.clen[q] && p.clen[q] <= p.cmax);
    // its pair blocks, its rows and its r_a
    std::vector<double> blocks(36 * (size_t)np, -1.0), staged(p.rows_max, 0.0), gcv(p.cmax, 0.0);
    for (int k = 0; k < np; ++k)
      for (int e = 0; e < 36; ++e) blocks[36 * k + e] = pair_value(k, e) + q;  // (only the owner's are sent)
    for (size_t r = 0; r < p.rows.size(); ++r)
      if (holder[p.rows[r].robot] == q)
        for (size_t e = 0; e < p.row_len(r); ++e) staged[p.rowoff[r] + e] = row_value(r, e);
    p.c_pack(gcv, blocks.data(), staged);
    for (int i = 0; cols > 0 && i < nr; ++i) {
      if (holder[i] != q) continue;
      std::vector<double> ra((size_t)6 * p.gs[i] * cols);
      for (int c = 0; c < cols; ++c)
        for (size_t j = 0; j < (size_t)6 * p.gs[i]; ++j) ra[(size_t)c * 6 * p.gs[i] + j] = ra_value(i, c, j);
      p.c_pack_ra(gcv, i, ra.data(), cols);
    }
    CHECK(gcv[0] == 0.0);  // (the status word is the transport's)
    call.insert(call.end(), gcv.begin(), gcv.end());
  }
  for (int q = 0; q < world; ++q) {
    const SchurAcrossPlan &p = pl[q];
    std::vector<double> blocks(36 * (size_t)np, -1.0);
    p.c_unpack_pairs(call, blocks.data());
    for (int k = 0; k < np; ++k)
      for (int e = 0; e < 36; ++e) CHECK(blocks[36 * k + e] == (p.pair_owner[k] < 0 ? -1.0 : pair_value(k, e) + p.pair_owner[k]));
    for (size_t r = 0; r < p.rows.size(); ++r)
      for (size_t e = 0; e < p.row_len(r); ++e) CHECK(p.c_row(call, r)[e] == row_value(r, e));
    if (cols > 0) {
      std::vector<double> hrS;
      p.c_unpack_rs(call, cols, hrS);
      CHECK(hrS.size() == (size_t)p.nS * cols);
      for (int i = 0; i < nr; ++i)
        for (int c = 0; c < cols; ++c)
          for (size_t j = 0; j < (size_t)6 * p.gs[i]; ++j) CHECK(hrS[(size_t)c * p.nS + (size_t)6 * p.gsoff[i] + j] == ra_value(i, c, j));
    }
  }
  if (held_records(12) || held_records(48)) return 1;
  RecordHash h;
  for (int v : hints) h.add(v);

  // out: whole, nS, hS, the public frames and the statistics of every robot, the hash; per rank and pair: its owner, how often
  // it is on pub_list, same_list, keep_list and is_list (with the flag of that entry) and how many rows it asks for
  std::vector<double> out = {whole ? 1.0 : 0.0, (double)pl[0].nS};
  out.insert(out.end(), hS[0].begin(), hS[0].end());
  for (int i = 0; i < nr; ++i)
    for (int v : pl[0].pubf[i]) out.push_back(v);
  out.insert(out.end(), pl[0].rstat.begin(), pl[0].rstat.end());
  out.push_back(h.value());
  for (int q = 0; q < world; ++q)
    for (int k = 0; k < np; ++k) {
      const SchurAcrossPlan &p = pl[q];
      const int blk = P[q].N + k;
      double cnt[7] = {(double)p.pair_owner[k], 0, 0, 0, 0, -1, 0};
      for (const CovBlk &b : p.pub_list) cnt[1] += b.blk == blk && b.f == 0;
      for (const auto &l : p.same_list)
        for (const CovBlk &b : l) cnt[2] += b.blk == blk;
      for (const auto &l : p.keep_list)
        for (const CovBlk &b : l) cnt[3] += b.blk == blk;
      for (const CovBlk &b : p.is_list)
        if (b.blk == blk) { cnt[4] += 1; cnt[5] = b.f; }
      for (const auto &r : p.rows) cnt[6] += r.pair == k;
      out.insert(out.end(), cnt, cnt + 7);
    }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 5;
  std::fclose(f);
  return 0;
}
"""

INCLUDE = os.path.join(ROOT, "dpgo_ros_amd", "csrc")


def _compile(workdir, flags, name):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = workdir / (name + ".cpp"), workdir / name
    src.write_text(PROGRAM)
    res = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall"] + flags + ["-I", INCLUDE, str(src), "-o", str(exe)], capture_output=True, text=True)
    return exe, res


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("schur_across_plan")


@pytest.fixture(scope="module")
def program(workdir):
    exe, res = _compile(workdir, [], "plan_host")
    assert res.returncode == 0, res.stderr
    assert "warning" not in res.stderr, res.stderr
    return exe


# 3 robots of 4, 3 and 1 poses: global poses 0 .. 3 (0 the fixed one), 4 .. 6, 7
GOFF, SIZES = [0, 4, 7], [4, 3, 1]


def _problem(holder, frames, cross, seed):
    """per robot its holder, the frames of its public poses and its cross blocks (row among its public poses, column robot, column
    frame), with random diagonal blocks, statistics and cross blocks"""
    rng = np.random.default_rng(seed)
    robots = []
    for i in range(3):
        s = len(frames[i])
        robots.append(dict(holder=holder[i], n=SIZES[i], frames=frames[i], cross=cross[i], diag=rng.standard_normal(36 * s * s),
                           stat=np.array([rng.standard_normal(), rng.random(), 1 + rng.random(), float(SIZES[i] - s - (i == 0) > 0)]),
                           blocks=rng.standard_normal((len(cross[i]), 36))))
    return robots


# two participants: every robot has a public pose; rank 1 holds two robots, one of them without an interior pose
SPLIT2 = dict(holder=[0, 1, 1], frames=[[3], [0], [0]], cross=[[], [(0, 0, 3)], [(0, 0, 3), (0, 1, 0)]])
PAIRS2 = [(0, 5), (2, 0), (3, 4), (7, 7), (4, 3), (1, 2), (6, 5), (2, 2), (1, 7), (5, 3), (3, 6), (4, 2), (1, 5), (6, 2)]
# three participants: robot 1 has no public pose, robot 2 (rank 2) no interior pose
SPLIT3 = dict(holder=[0, 1, 2], frames=[[1, 3], [], [0]], cross=[[], [], [(0, 0, 1), (0, 0, 3)]])
PAIRS3 = [(0, 4), (6, 0), (1, 3), (7, 1), (7, 7), (2, 2), (4, 6), (5, 5), (2, 7), (5, 3), (3, 5), (7, 2), (2, 5), (6, 2)]


def _run(exe, workdir, robots, world, cols, pairs, hints=()):
    v = [world, len(robots), cols, len(pairs), len(hints)]
    for r in robots:
        v += [r["holder"], r["n"], len(r["frames"])] + list(r["frames"]) + [len(r["cross"])]
        for c, blk in zip(r["cross"], r["blocks"]):
            v += list(c) + list(blk)
        v += list(r["diag"]) + list(r["stat"])
    v += [p for ab in pairs for p in ab] + list(hints)
    np.array(v, dtype=F).tofile(workdir / "in.bin")
    res = subprocess.run([str(exe), str(workdir / "in.bin"), str(workdir / "out.bin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = np.fromfile(workdir / "out.bin")
    nS, S = int(out[1]), sum(len(r["frames"]) for r in robots)
    assert nS == 6 * S
    sizes = [2, nS * nS, S, 4 * len(robots), 1, 7 * world * len(pairs)]
    assert out.size == sum(sizes)
    head, hS, pubf, rstat, h, cases = np.split(out, np.cumsum(sizes)[:-1])
    return dict(whole=bool(head[0]), hS=hS.reshape(nS, nS).T, pubf=pubf, rstat=rstat.reshape(-1, 4), hash=h[0],
                cases=cases.reshape(world, len(pairs), 7))


def _expected_S(robots, skip=()):
    """S_c built directly from the blocks: robot i's diagonal block at its place in the separator; a cross block H[row pose, column
    pose] (6 x 6 column-major) at (row, column) and its transpose at (column, row)"""
    soff = np.cumsum([0] + [len(r["frames"]) for r in robots])
    S = np.zeros((6 * soff[-1], 6 * soff[-1]))
    for i, r in enumerate(robots):
        w = 6 * len(r["frames"])
        S[6 * soff[i]:6 * soff[i] + w, 6 * soff[i]:6 * soff[i] + w] = r["diag"].reshape(w, w).T
        for b, ((lrow, cr, cf), blk) in enumerate(zip(r["cross"], r["blocks"])):
            if (i, b) in skip:
                continue
            row, col = soff[i] + lrow, soff[cr] + robots[cr]["frames"].index(cf)
            S[6 * row:6 * row + 6, 6 * col:6 * col + 6] = blk.reshape(6, 6).T
            S[6 * col:6 * col + 6, 6 * row:6 * row + 6] = blk.reshape(6, 6)
    return S


def _case_of(robots, a, b):
    """the case of a pair from the problem alone: (name, owner rank or -1)"""
    def where(g):
        i = max(k for k in range(3) if GOFF[k] <= g)
        return i, (g - GOFF[i]) in robots[i]["frames"]
    if a == 0 or b == 0:
        return "fixed", -1
    (ra, pa), (rb, pb) = where(a), where(b)
    if pa and pb:
        return "public", -1
    if not pa and not pb:
        return ("same", robots[ra]["holder"]) if ra == rb else ("cross", -1)
    return ("int_pub", robots[ra]["holder"]) if pb else ("pub_int", robots[rb]["holder"])


def _check_split(got, robots, world, pairs, skip=()):
    S = _expected_S(robots, skip)
    assert got["hS"].tobytes() == S.tobytes(), "S_c differs from the matrix built directly from the blocks"
    assert got["pubf"].tolist() == [f for r in robots for f in r["frames"]]
    assert got["rstat"].tobytes() == np.array([r["stat"] for r in robots]).tobytes()
    seen = set()
    for q in range(world):
        for k, (a, b) in enumerate(pairs):
            name, owner = _case_of(robots, a, b)
            mine = owner == q
            seen.add((name, "here" if mine else "elsewhere" if owner >= 0 else "everyone"))
            want = dict(fixed=[-1, 0, 0, 0, 0, -1, 0], public=[-1, 1, 0, 0, 0, -1, 0], cross=[-1, 0, 0, 0, 0, -1, 2],
                        same=[owner, 0, mine, mine, 0, -1, 0], int_pub=[owner, 0, 0, 0, mine, 0 if mine else -1, 0],
                        pub_int=[owner, 0, 0, 0, mine, 1 if mine else -1, 0])[name]
            assert got["cases"][q, k].tolist() == [float(x) for x in want], (q, k, (a, b), name)
    return seen


@pytest.mark.parametrize("cols", [0, 2])
def test_b_round_trip_pair_cases_and_c_tiling(program, workdir, cols):
    every = {(n, w) for n in ("same", "int_pub", "pub_int") for w in ("here", "elsewhere")} | {(n, "everyone") for n in ("fixed", "public", "cross")}
    for split, world, pairs, seed in ((SPLIT2, 2, PAIRS2, 1), (SPLIT3, 3, PAIRS3, 2)):
        robots = _problem(seed=seed, **split)
        got = _run(program, workdir, robots, world, cols, pairs)
        assert got["whole"]
        assert _check_split(got, robots, world, pairs) == every


TORN = dict(SPLIT2, cross=[[], [(0, 0, 3)], [(0, 0, 2), (0, 1, 0)]])  # robot 2's first block names frame 2 of robot 0: not public


def test_torn_when_a_cross_block_names_a_pose_that_is_not_public(program, workdir):
    robots = _problem(seed=3, **TORN)
    got = _run(program, workdir, robots, 2, 0, PAIRS2)
    assert not got["whole"]
    # (the block is left out, everything else is in its place)
    assert got["hS"].tobytes() == _expected_S(robots, skip={(2, 0)}).tobytes()


def _old_pair_hash(ints):
    """the first formula of the agreement hash of the pairs: FNV-1a over the four bytes of every int, low byte first"""
    h = np.uint64(1469598103934665603)
    with np.errstate(over="ignore"):
        for v in np.asarray(ints, dtype=np.int32).view(np.uint32):
            for i in range(4):
                h ^= np.uint64((int(v) >> (8 * i)) & 0xFF)
                h *= np.uint64(1099511628211)
    return float(int(h) & ((1 << 52) - 1))


@pytest.mark.parametrize("ints", [[], [3, 7], [0, -1, 5, 5, -2147483648, 2147483647, 12, -40, 65536, 255]])
def test_record_hash_over_ints_is_the_first_pair_hash(program, workdir, ints):
    got = _run(program, workdir, _problem(seed=4, **SPLIT2), 2, 0, PAIRS2, hints=ints)
    assert got["hash"] == _old_pair_hash(ints)
    assert _old_pair_hash([]) == float(1469598103934665603 & ((1 << 52) - 1))


def test_the_same_program_under_address_and_undefined_sanitizers(workdir):
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # (the runtimes linked INTO the program where the compiler can: a stand-alone program then starts whatever else the
    # environment loads into every process in front of it)
    exe, res = _compile(workdir, san + ["-static-libasan", "-static-libubsan"], "plan_host_san")
    if res.returncode != 0:
        exe, res = _compile(workdir, san, "plan_host_san")
    if res.returncode != 0:
        assert "asan" in res.stderr or "ubsan" in res.stderr or "sanitize" in res.stderr, res.stderr
        pytest.skip("the sanitizer runtimes are not installed: " + res.stderr.strip().splitlines()[-1])
    for split, world, pairs, seed in ((SPLIT2, 2, PAIRS2, 1), (SPLIT3, 3, PAIRS3, 2)):
        for cols in (0, 2):
            robots = _problem(seed=seed, **split)
            _check_split(_run(exe, workdir, robots, world, cols, pairs, hints=[1, -2, 3, 4]), robots, world, pairs)
    assert not _run(exe, workdir, _problem(seed=3, **TORN), 2, 0, PAIRS2)["whole"]
