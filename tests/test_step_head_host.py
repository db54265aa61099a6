"""CPU check of csrc/step_head.h, compiled for the host: the packed head of k_step_fd's arguments (the thirteen leading
dwords the deep-carried launch forms its first requests from).  A stand-alone program checks

  * pack -> unpack round trips at the field limits: n = 1 and 512, npub = 0 and 128, nshared = 0 and 160, both parities,
    every flag combination, every chunk id in the two ord dwords;
  * the work vectors derived from the first one and n equal base + 4 r n b for every b;
  * the eligibility check launch_step_fd and fe_deep_m0 rely on (fd_head_build): a descriptor whose work vectors are not one
    allocation is refused, and so is every field beyond its width."""
import os
import shutil
import subprocess

import pytest

from tests.util import ROOT

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "step_head.h"
using namespace dpgo;
static int bad = 0, checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { ++bad; std::printf("failed line %d: %s\n", __LINE__, #c); } } while (0)
constexpr int NBUF = 24;
struct Desc {
  std::vector<double> store;
  double *buf[NBUF];
  unsigned char ord[32];
  int r, n, N4, npub, nshared, m0, parity, flags, nblk_all;
  double M[1], coef[1], pacc[1];
  Desc(int r_, int n_) : store((size_t)4 * r_ * n_ * NBUF + 8), r(r_), n(n_), N4(4 * n_), npub(100), nshared(150), m0(24), parity(1),
                         flags(37), nblk_all((4 * n_ + 7) / 8) {
    for (int b = 0; b < NBUF; ++b) buf[b] = store.data() + (size_t)4 * r * n * b;
    for (int i = 0; i < 32; ++i) ord[i] = (unsigned char)((7 * i + 3) % 32);
  }
  bool build(FdHead &h) const { return fd_head_build(h, buf, NBUF, r, n, N4, npub, nshared, M, coef, ord, m0, parity, flags, pacc, nblk_all); }
};
int main() {
  // ---- round trips at the field limits
  const int ns[] = {1, 2, 499, 512}, npubs[] = {0, 1, 127, FD_HEAD_NPUB_MAX}, nsh[] = {0, 1, 159, FD_HEAD_NSHARED_MAX};
  for (int n : ns) for (int npub : npubs) {
    const unsigned np = fd_head_pack_np(n, npub);
    CHECK(fd_head_n(np) == n && fd_head_npub(np) == npub);
  }
  for (int s : nsh) for (int parity = 0; parity < 2; ++parity) for (int flags = 0; flags <= FD_HEAD_FLAGS_MAX; ++flags) {
    const unsigned sf = fd_head_pack_sf(s, parity, flags);
    CHECK(fd_head_nshared(sf) == s && fd_head_parity(sf) == parity && fd_head_flags(sf) == flags);
  }
  CHECK(FD_HEAD_N_MAX == 512 && FD_HEAD_NSHARED_MAX == 160 && FD_HEAD_DWORDS == 13);
  CHECK(sizeof(void *) == 8 && 4 * FD_HEAD_DWORDS == 4 * sizeof(void *) + 5 * sizeof(int));
  // ---- derived work vectors, chunk ids, the head of a descriptor that fits
  for (int r = 3; r <= 5; ++r) for (int n : ns) {
    Desc d(r, n);
    for (int b = 0; b < NBUF; ++b) CHECK(fd_head_buf(d.buf[0], r, n, b) == d.store.data() + (size_t)4 * r * n * b);
    CHECK(fd_head_one_allocation(d.buf, NBUF, r, n));
    for (int m0 = 24; m0 <= 32; ++m0) {
      d.m0 = m0;
      FdHead h;
      CHECK(d.build(h));
      for (int i = 0; m0 + i < 32; ++i) CHECK(fd_head_ord(h.ord_lo, h.ord_hi, i) == d.ord[m0 + i]);
      CHECK(h.buf0 == d.buf[0] && h.M == d.M && h.fe_coef == d.coef && h.pacc_in == d.pacc && h.nblk_all == d.nblk_all);
      CHECK(fd_head_n(h.np) == n && fd_head_npub(h.np) == d.npub && fd_head_nshared(h.sf) == d.nshared);
      CHECK(fd_head_parity(h.sf) == d.parity && fd_head_flags(h.sf) == d.flags);
    }
  }
  // ---- what the head cannot stand for is refused
  FdHead h;
  for (int b = 1; b < NBUF; ++b) { Desc d(5, 500); d.buf[b] += 1; CHECK(!d.build(h)); }              // not one allocation
  { Desc d(5, 500); std::vector<double> other(16); d.buf[NBUF - 1] = other.data(); CHECK(!d.build(h)); }
  { Desc d(5, 500); d.r = 4; CHECK(!d.build(h)); }                                                    // (one allocation at another rank)
  { Desc d(5, 512); CHECK(d.build(h)); d.n = 513; d.N4 = 4 * 513; d.nblk_all = 257; CHECK(!d.build(h)); }
  { Desc d(5, 500); d.n = 0; d.N4 = 0; CHECK(!d.build(h)); }
  { Desc d(5, 500); d.N4 = 4 * 500 + 4; CHECK(!d.build(h)); }
  { Desc d(5, 500); d.npub = FD_HEAD_NPUB_MAX; CHECK(d.build(h)); d.npub = FD_HEAD_NPUB_MAX + 1; CHECK(!d.build(h)); d.npub = -1; CHECK(!d.build(h)); }
  { Desc d(5, 500); d.nshared = FD_HEAD_NSHARED_MAX; CHECK(d.build(h)); d.nshared = FD_HEAD_NSHARED_MAX + 1; CHECK(!d.build(h)); }
  { Desc d(5, 500); d.flags = FD_HEAD_FLAGS_MAX + 1; CHECK(!d.build(h)); d.flags = -1; CHECK(!d.build(h)); }
  { Desc d(5, 500); d.parity = 2; CHECK(!d.build(h)); }
  { Desc d(5, 500); d.m0 = 23; CHECK(!d.build(h)); d.m0 = 33; CHECK(!d.build(h)); }
  { Desc d(5, 500); d.nblk_all -= 1; CHECK(!d.build(h)); }
  std::printf("%d %d\n", checks, bad);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("step_head_host")
    src, exe = d / "step_head_host.cpp", d / "step_head_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def test_head_round_trips_derives_the_work_vectors_and_refuses_what_it_cannot_hold(program):
    out = subprocess.check_output([program], text=True)
    checks, bad = (int(v) for v in out.strip().splitlines()[-1].split())
    assert checks > 1000
    assert bad == 0, out
