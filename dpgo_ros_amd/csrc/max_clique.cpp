// max_clique.cpp -- a maximum clique of a graph given as bitset rows: exact branch and bound on bitsets with a
// greedy-colouring bound (Tomita and Seki's MCQ in San Segundo's bit-parallel form).  The vertices are renumbered by
// degeneracy (the vertex removed last comes first), the incumbent is seeded by a greedy clique in that order, and a larger
// clique replaces it only when strictly larger: the same input gives the same members.  Host only.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "team_internal.h"

namespace {

using dpgo_host::set_err;
typedef std::vector<uint64_t> Bits;

struct Search {
  int K = 0, W = 0;
  std::vector<Bits> adj;  // renumbered
  std::vector<int> best, cur;
  long long nodes = 0, max_nodes = 0;
  bool aborted = false;
  // per depth: the candidate set, the colouring's order and its bounds
  std::vector<Bits> P;
  std::vector<std::vector<int>> order, colour;

  static int first_bit(const Bits &b) {
    for (size_t w = 0; w < b.size(); ++w)
      if (b[w]) return (int)(64 * w) + __builtin_ctzll(b[w]);
    return -1;
  }
  void ensure(size_t depth) {
    while (P.size() <= depth) {
      P.emplace_back(W, 0);
      order.emplace_back();
      colour.emplace_back();
    }
  }
  // the vertices of P[depth] in colour classes: colour[n] bounds the clique number of order[0 .. n]
  void colour_sort(size_t depth) {
    Bits Q = P[depth], U(W);
    std::vector<int> &ord = order[depth], &col = colour[depth];
    ord.clear();
    col.clear();
    int c = 0;
    while (first_bit(Q) >= 0) {
      ++c;
      U = Q;
      int v;
      while ((v = first_bit(U)) >= 0) {
        Q[v >> 6] &= ~(1ull << (v & 63));
        U[v >> 6] &= ~(1ull << (v & 63));
        for (int w = 0; w < W; ++w) U[w] &= ~adj[v][w];
        ord.push_back(v);
        col.push_back(c);
      }
    }
  }
  void expand(size_t depth) {
    if (max_nodes > 0 && nodes >= max_nodes) { aborted = true; return; }
    ++nodes;
    colour_sort(depth);
    ensure(depth + 1);
    for (int n = (int)order[depth].size() - 1; n >= 0; --n) {
      if ((int)cur.size() + colour[depth][n] <= (int)best.size()) return;
      const int v = order[depth][n];
      cur.push_back(v);
      bool any = false;
      for (int w = 0; w < W; ++w) {
        P[depth + 1][w] = P[depth][w] & adj[v][w];
        any = any || P[depth + 1][w];
      }
      if (any) expand(depth + 1);
      else if (cur.size() > best.size()) best = cur;
      cur.pop_back();
      if (aborted) return;
      P[depth][v >> 6] &= ~(1ull << (v & 63));
    }
  }
};

int refuse(const std::string &m) {
  set_err("max_clique: " + m);
  return DPGO_ERR;
}

}  // namespace

extern "C" int dpgo_max_clique(int K, const uint64_t *adj, long long max_nodes, int *members, int *size, int *proven) {
  if (K <= 0) return refuse("K must be positive, not " + std::to_string(K));
  if (!adj || !members || !size || !proven) return refuse("null argument");
  if (max_nodes < 0) return refuse("max_nodes must not be negative (0: no limit), not " + std::to_string(max_nodes));
  const int W = (K + 63) / 64;
  auto bit = [&](int a, int b) { return (adj[(size_t)a * W + (b >> 6)] >> (b & 63)) & 1ull; };
  for (int a = 0; a < K; ++a) {
    if (bit(a, a)) return refuse("the diagonal bit of row " + std::to_string(a) + " is set");
    if (K & 63) {
      const uint64_t beyond = adj[(size_t)a * W + W - 1] >> (K & 63);
      if (beyond) return refuse("row " + std::to_string(a) + " has a bit set at or beyond column K = " + std::to_string(K));
    }
  }
  std::vector<int> deg(K, 0);
  for (int a = 0; a < K; ++a)
    for (int w = 0; w < W; ++w) {
      uint64_t x = adj[(size_t)a * W + w];
      deg[a] += __builtin_popcountll(x);
      while (x) {
        const int b = 64 * w + __builtin_ctzll(x);
        x &= x - 1;
        if (!bit(b, a)) return refuse("the matrix is not symmetric: (" + std::to_string(a) + ", " + std::to_string(b) + ") is set, (" +
                                      std::to_string(b) + ", " + std::to_string(a) + ") is not");
      }
    }
  // degeneracy order: the vertex of least remaining degree (the lowest index among equals) leaves first and is numbered last
  std::vector<int> old_of(K), new_of(K);
  {
    std::vector<char> gone(K, 0);
    for (int n = K - 1; n >= 0; --n) {
      int v = -1;
      for (int a = 0; a < K; ++a)
        if (!gone[a] && (v < 0 || deg[a] < deg[v])) v = a;
      gone[v] = 1;
      old_of[n] = v;
      new_of[v] = n;
      for (int b = 0; b < K; ++b)
        if (!gone[b] && bit(v, b)) --deg[b];
    }
  }
  Search s;
  s.K = K;
  s.W = W;
  s.max_nodes = max_nodes;
  s.adj.assign(K, Bits(W, 0));
  for (int a = 0; a < K; ++a)
    for (int b = 0; b < K; ++b)
      if (bit(a, b)) s.adj[new_of[a]][new_of[b] >> 6] |= 1ull << (new_of[b] & 63);
  // the seed: greedy in the new order
  for (int v = 0; v < K; ++v) {
    bool all = true;
    for (int u : s.best) all = all && ((s.adj[v][u >> 6] >> (u & 63)) & 1ull);
    if (all) s.best.push_back(v);
  }
  s.ensure(0);
  for (int v = 0; v < K; ++v) s.P[0][v >> 6] |= 1ull << (v & 63);
  s.expand(0);
  std::vector<int> out;
  for (int v : s.best) out.push_back(old_of[v]);
  std::sort(out.begin(), out.end());
  std::copy(out.begin(), out.end(), members);
  *size = (int)out.size();
  *proven = s.aborted ? 0 : 1;
  return DPGO_OK;
}
