"""CPU check of the scalar part of csrc/nesterov_step.h, compiled for the host: the invariant the carried forms of the
accelerated-RGD iteration (k_step_fe, k_step_fd) depend on -- the Nesterov scalars a launch derives AHEAD from the state
before iteration k (nest_ahead) are, bit for bit, the scalars the books (nest_books, + iter) will produce when the
iterations it looks at arrive.  A stand-alone program walks the states from {gamma = 0, alpha = 0, iter = 0} and compares
at every one of them."""
import os
import shutil
import subprocess

import pytest

from tests.util import ROOT

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
namespace dpgo { struct NestState { double gamma, alpha; int iter; int pad; }; }
#include "nesterov_step.h"
using namespace dpgo;
static NestState books(NestState s, double Nr, int ri) { nest_books(s, Nr, ri); s.iter += 1; return s; }
static bool restarts(const NestState &s, int ri) { return ((s.iter + 2) % ri) == 0; }
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
// argv: num_robots, restart_interval.  Prints "<states> <mismatches>" (and one line per mismatch in front of it).
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const int nr = std::atoi(argv[1]), ri = std::atoi(argv[2]);
  const double Nr = (double)nr;
  NestState s = {0.0, 0.0, 0, 0};
  int bad = 0, states = 0;
  for (int t = 0; t < 3 * ri + 7; ++t, s = books(s, Nr, ri)) {
    ++states;
    const NestAhead a = nest_ahead(s, nr, ri);
    const NestState b1 = books(s, Nr, ri), b2 = books(b1, Nr, ri), b3 = books(b2, Nr, ri), b4 = books(b3, Nr, ri);
    const bool ok[8] = {same(a.nest_gamma, b1.gamma),
                        a.restart_now == restarts(s, ri),
                        a.restart_next == restarts(b1, ri),
                        a.restart_next2 == restarts(b2, ri),
                        a.restart_next3 == restarts(b3, ri),
                        a.restart_next || same(a.ahead_alpha, b2.alpha),
                        a.restart_next2 || same(a.ahead2_alpha, b3.alpha),
                        a.restart_next3 || same(a.ahead3_alpha, b4.alpha)};
    for (int k = 0; k < 8; ++k)
      if (!ok[k]) { ++bad; std::printf("mismatch: state %d (iter %d), check %d\n", t, s.iter, k); }
  }
  std::printf("%d %d\n", states, bad);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("nesterov_host")
    src, exe = d / "nesterov_host.cpp", d / "nesterov_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"),
                           str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("restart_interval", [2, 3, 4, 5, 20, 50])
@pytest.mark.parametrize("num_robots", [1, 2, 5, 8])
def test_scalars_derived_ahead_are_the_scalars_the_books_produce(program, num_robots, restart_interval):
    out = subprocess.check_output([program, str(num_robots), str(restart_interval)], text=True)
    states, bad = (int(v) for v in out.strip().splitlines()[-1].split())
    assert states == 3 * restart_interval + 7
    assert bad == 0, out
