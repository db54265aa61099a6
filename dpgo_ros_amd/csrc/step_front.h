// step_front.h -- the "front table" of k_step_fd (step_deep.hip): what the launch's first dependent lookups resolve to, per
// agent, formed ONCE on the host where the descriptor is built (assembly.hip) instead of in every launch and workgroup
// behind a cold trip to the launch's argument struct.  None of it changes from launch to launch: it changes when a work
// vector is reallocated, the edge list changes or the rank does -- the events that rebuild the descriptor.
//
// The table sits behind the packed coefficients of the shared edges in the SAME device allocation, at a fixed offset, so
// its address follows from the launch's head alone (step_head.h: fe_coef) and nothing is added to the head:
//
//     fe_coef + 0                       [FD_FRONT_EDGES][16] doubles  the coefficients (the first nshared edges are used)
//     fe_coef + FD_FRONT_OFF_DOUBLES    FdFront
//
//     FdFront::xaddr[p][s]   the address of the neighbour pose of shared edge s as a launch of parity p reads it:
//                            ybase[sa] + (p ? alt * 4r * npose[sa] : 0) + 4r * frame,  (sa, frame) the edge's 16-bit code
//                            (frame | sa << 12) -- what wave 6 formed from AgentDev::fe_code and FeBases in every launch.
//                            FD_FRONT_SLOTS = 3 x 64 slots: one per lane of wave 6's three trips, so the lane indexes it
//                            without a clamp; slots beyond the last edge hold the address of code 0 (agent 0, frame 0: a
//                            pose that exists -- the loads behind the last edge stay unconditional, step_deep.hip)
//     FdFront::pub[q]        public pose q: its local pose, where its row goes in the chunk-ordered vector
//                            (fd_front_pos_off: the chunk's place in the agent's chunk order), its shared edges
//                            [pe0, pe1) -- pub_pose[q], fd_pos_off(fe_ord, pose), pub_ptr[q], pub_ptr[q + 1].  Records
//                            beyond npub are {0, 0, 0, 0}: no edges.
//
// fd_front_build forms the image from the descriptor's own fields (the codes, the bases, the public-pose tables, the chunk
// order) and refuses what the table cannot hold or what would address outside a neighbour's vector.
//
// Compiles for the host too (tests/test_step_front_host.py): nothing here needs a device header.
#pragma once
#include <cstddef>
#include "step_head.h"

namespace dpgo {

constexpr int FD_FRONT_EDGES = FD_HEAD_NSHARED_MAX;  // (= FE_MAX_EDGES, dpgo_dev.h: asserted where both are visible)
constexpr int FD_FRONT_SLOTS = 192;                  // three trips of 64 lanes
constexpr int FD_FRONT_AGENTS = 8;                   // (= LOOKAHEAD_MAX_AGENTS: the 16-bit code holds the agent in 4 bits, 8 have bases)
constexpr int FD_FRONT_FRAMES = 4096;                // the code's 12 bits
constexpr size_t FD_FRONT_OFF_DOUBLES = (size_t)FD_FRONT_EDGES * 16;

struct FdFrontPub {
  int pose, vs_off, pe0, pe1;
};

struct FdFront {
  const double *xaddr[2][FD_FRONT_SLOTS];
  FdFrontPub pub[FD_HEAD_NPUB_MAX];
};

static_assert(sizeof(void *) == 8 && sizeof(FdFrontPub) == 16 && sizeof(FdFront) == 2 * FD_FRONT_SLOTS * 8 + FD_HEAD_NPUB_MAX * 16 &&
                  sizeof(FdFront) % sizeof(double) == 0 && (FD_FRONT_OFF_DOUBLES * sizeof(double)) % 16 == 0,
              "the table is read with 8- and 16-byte loads at fixed offsets behind the coefficients");
static_assert(FD_FRONT_SLOTS >= FD_FRONT_EDGES && FD_FRONT_SLOTS % 64 == 0, "one slot per lane and trip");

// doubles of the whole image: coefficients + table
constexpr size_t FD_FRONT_IMAGE_DOUBLES = FD_FRONT_OFF_DOUBLES + sizeof(FdFront) / sizeof(double);

// the table behind the coefficients at fe_coef
DPGO_HD const FdFront *fd_front_of(const double *fe_coef) { return reinterpret_cast<const FdFront *>(fe_coef + FD_FRONT_OFF_DOUBLES); }

// where pose p of an agent sits in the chunk-ordered layout of its vector at rank r, [place][16 poses][4r]: chunk p / 16 at
// the place it has in the agent's chunk order (the value of step_deep.hip's fd_pos_off<R>)
DPGO_HD int fd_front_pos_off(const unsigned char *ord, int pose, int r) {
  const int ch = pose >> 4;
  int p = 0;
  for (int i = 0; i < 32; ++i) p = ((int)ord[i] == ch) ? i : p;
  return p * 64 * r + (pose & 15) * 4 * r;
}

// the address a launch of parity `parity` reads the pose `code` names at (ybase / npose: the agents' Y arrays and pose counts,
// alt: how many vectors the second copy of the poses sits behind the first)
DPGO_HD const double *fd_front_xaddr(unsigned code, int parity, int r, const double *const *ybase, const int *npose, int alt) {
  const int sa = (int)(code >> 12), sf = (int)(code & 0xfffu);
  return ybase[sa] + (parity ? (size_t)alt * 4 * r * npose[sa] : (size_t)0) + (size_t)sf * 4 * r;
}

// the table of one agent.  code: its edges' 16-bit codes, two per word (AgentDev::fe_code; words beyond the last edge are not
// read); ybase / npose: the first num_agents agents' Y arrays and pose counts (FeBases); n: the agent's own pose count.
// false: the table cannot stand for these tables -- too many edges or public poses, an edge whose code names an agent
// without a base or a frame beyond its agent, a public pose beyond the agent, edge ranges that are not an ascending cover
// of [0, nshared) -- and f is left in an unspecified state.
DPGO_HD bool fd_front_build(FdFront &f, int r, int n, int nshared, const unsigned *code, int num_agents, const double *const *ybase,
                            const int *npose, int alt, int npub, const int *pub_pose, const int *pub_ptr, const unsigned char *ord) {
  if (r < 1 || n < 1 || nshared < 0 || nshared > FD_FRONT_EDGES || npub < 0 || npub > FD_HEAD_NPUB_MAX || num_agents < 1 ||
      num_agents > FD_FRONT_AGENTS || alt < 0 || !ybase[0] || npose[0] < 1)
    return false;
  for (int e = 0; e < nshared; ++e) {
    const unsigned c = (code[e >> 1] >> (16 * (e & 1))) & 0xffffu;
    const int sa = (int)(c >> 12), sf = (int)(c & 0xfffu);
    if (sa >= num_agents || !ybase[sa] || sf >= npose[sa]) return false;
    for (int p = 0; p < 2; ++p) f.xaddr[p][e] = fd_front_xaddr(c, p, r, ybase, npose, alt);
  }
  for (int s = nshared; s < FD_FRONT_SLOTS; ++s)
    for (int p = 0; p < 2; ++p) f.xaddr[p][s] = fd_front_xaddr(0u, p, r, ybase, npose, alt);
  if (npub > 0 && (pub_ptr[0] != 0 || pub_ptr[npub] != nshared)) return false;
  for (int q = 0; q < npub; ++q) {
    if (pub_pose[q] < 0 || pub_pose[q] >= n || pub_ptr[q + 1] < pub_ptr[q]) return false;
    f.pub[q].pose = pub_pose[q];
    f.pub[q].vs_off = fd_front_pos_off(ord, pub_pose[q], r);
    f.pub[q].pe0 = pub_ptr[q];
    f.pub[q].pe1 = pub_ptr[q + 1];
  }
  for (int q = npub; q < FD_HEAD_NPUB_MAX; ++q) f.pub[q] = FdFrontPub{0, 0, 0, 0};
  return true;
}

}  // namespace dpgo
