// step_head.h -- the head of k_step_fd's arguments (step_deep.hip): the thirteen dwords every role of the launch forms its
// FIRST requests from.  Leading kernel arguments that are not by-value structs can be delivered in SGPRs at wave launch
// (step_deep.o is built with -mllvm -amdgpu-kernarg-preload-count=14; at most 14 dwords, a struct ends the run), so
// an address formed from them needs no scalar load -- everything else the launch is told sits behind them in one struct
// (FdArgs), in memory nobody has touched.  What the head holds:
//
//     dwords   argument
//     0-1      buf0      the agent's first work vector.  All NBUF work vectors of an agent are ONE allocation
//                        (assembly.hip: buf[b] = base + 4 r n b), so every buf[b] follows from it and n: fd_head_buf
//     2-3      M         its dense inverse
//     4-5      pacc_in   the partial sums the launch continues
//     6-7      fe_coef   the packed coefficients of its shared edges
//     8        np        n | npub << 16                     (n <= 512: one 2048-row pass; N4 = 4 n, nblk = (N4 + 7) / 8)
//     9        sf        nshared | parity << 8 | flags << 9 (nshared <= 160, flags: the FD_* bits, < 64)
//     10-11    ord       fe_ord[m0 .. 31], one byte each: the chunk ids of the last 32 - m0 <= 8 chunks
//     12       nblk_all  workgroups that take part (the team's largest agent); the grid is the next multiple of 8
//
// The head is a packed COPY of fields of the descriptor: fd_head_build refuses a descriptor it cannot represent (a field
// beyond its width, work vectors that are not one allocation), and a team with such an agent does not take the deep-carried
// form (step_fd_head_ok, next to the other conditions of fe_deep_m0).
//
// Compiles for the host too (tests/test_step_head_host.py): nothing here needs a device header.
#pragma once
#include <cstddef>

#ifndef DPGO_HD
#if defined(__HIPCC__)
#define DPGO_HD __host__ __device__ __forceinline__
#else
#define DPGO_HD inline
#endif
#endif

namespace dpgo {

constexpr int FD_HEAD_DWORDS = 13;
constexpr int FD_HEAD_N_MAX = 512, FD_HEAD_NPUB_MAX = 128, FD_HEAD_NSHARED_MAX = 160, FD_HEAD_FLAGS_MAX = 63;
constexpr int FD_HEAD_ORD_MAX = 8;  // chunk ids the two ord dwords hold

struct FdHead {
  double *buf0;
  const double *M, *pacc_in, *fe_coef;
  unsigned np, sf, ord_lo, ord_hi;
  int nblk_all;
};

DPGO_HD unsigned fd_head_pack_np(int n, int npub) { return (unsigned)n | ((unsigned)npub << 16); }
DPGO_HD int fd_head_n(unsigned np) { return (int)(np & 0xffffu); }
DPGO_HD int fd_head_npub(unsigned np) { return (int)(np >> 16); }

DPGO_HD unsigned fd_head_pack_sf(int nshared, int parity, int flags) { return (unsigned)nshared | ((unsigned)parity << 8) | ((unsigned)flags << 9); }
DPGO_HD int fd_head_nshared(unsigned sf) { return (int)(sf & 0xffu); }
DPGO_HD int fd_head_parity(unsigned sf) { return (int)((sf >> 8) & 1u); }
DPGO_HD int fd_head_flags(unsigned sf) { return (int)(sf >> 9); }

// chunk id of the i-th of the last chunks (fe_ord[m0 + i]), i < 8
DPGO_HD int fd_head_ord(unsigned ord_lo, unsigned ord_hi, int i) { return (int)(((i < 4 ? ord_lo : ord_hi) >> (8 * (i & 3))) & 0xffu); }

// work vector b of an agent of n poses at rank r whose first work vector is buf0
DPGO_HD double *fd_head_buf(double *buf0, int r, int n, int b) { return buf0 + (size_t)4 * r * n * b; }

DPGO_HD bool fd_head_fits(int n, int N4, int npub, int nshared, int parity, int flags, int m0) {
  return n >= 1 && n <= FD_HEAD_N_MAX && N4 == 4 * n && npub >= 0 && npub <= FD_HEAD_NPUB_MAX && nshared >= 0 &&
         nshared <= FD_HEAD_NSHARED_MAX && (parity == 0 || parity == 1) && flags >= 0 && flags <= FD_HEAD_FLAGS_MAX &&
         m0 >= 32 - FD_HEAD_ORD_MAX && m0 <= 32;
}

DPGO_HD bool fd_head_one_allocation(double *const *buf, int nbuf, int r, int n) {
  for (int b = 0; b < nbuf; ++b)
    if (buf[b] != fd_head_buf(buf[0], r, n, b)) return false;
  return true;
}

// the head of a launch for the agent the arguments describe (buf: its nbuf work vectors, ord: its 32 chunk ids);
// false: the head cannot stand for this descriptor, and h is left unset
DPGO_HD bool fd_head_build(FdHead &h, double *const *buf, int nbuf, int r, int n, int N4, int npub, int nshared, const double *M,
                           const double *fe_coef, const unsigned char *ord, int m0, int parity, int flags,
                           const double *pacc_in, int nblk_all) {
  if (!fd_head_fits(n, N4, npub, nshared, parity, flags, m0) || nblk_all < (N4 + 7) / 8 || !fd_head_one_allocation(buf, nbuf, r, n))
    return false;
  h.buf0 = buf[0]; h.M = M; h.pacc_in = pacc_in; h.fe_coef = fe_coef;
  h.np = fd_head_pack_np(n, npub);
  h.sf = fd_head_pack_sf(nshared, parity, flags);
  h.ord_lo = h.ord_hi = 0;
  for (int i = 0; m0 + i < 32; ++i) {
    const unsigned v = (unsigned)ord[m0 + i] << (8 * (i & 3));
    if (i < 4) h.ord_lo |= v; else h.ord_hi |= v;
  }
  h.nblk_all = nblk_all;
  return true;
}

}  // namespace dpgo
