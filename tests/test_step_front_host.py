"""CPU check of csrc/step_front.h, compiled for the host: the front table of k_step_fd (where the neighbour pose of every
shared edge lives for either parity, and one record per public pose: pose, place of its row in the chunk-ordered vector,
edge range), which sits behind the packed coefficients in one image.  A stand-alone program builds the image the way
assembly.hip does -- coefficients, then the table at its fixed offset -- for a case it reads from a file, reads the table
back through fd_front_of and prints it; the formulas are evaluated here in numpy:

    xaddr[p][e]   = ybase[sa] + (p ? alt * 4r * npose[sa] : 0) + 4r * frame        (sa, frame: the edge's 16-bit code)
    xaddr[p][s]   = xaddr of code 0 for the slots behind the last edge (a pose that exists)
    pub[q]        = {pub_pose[q], place(chunk of the pose) * 64r + (pose & 15) * 4r, pub_ptr[q], pub_ptr[q + 1]}

Cases: nshared = 0, 1, 63, 64, 65, 127, 128, 129, 160 (161 refused); npub = 1, 64, 65, 128 (129 refused); neighbours on local
agents 0 and 7 with different pose counts (the alt-copy offset differs per neighbour); frames 0 and n - 1; r = 3, 4, 5; a
chunk order that is not the identity.  Where the sanitizer runtimes are installed the same program is built once more with
-fsanitize=address,undefined and run stand-alone over every case."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import ROOT

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "step_front.h"
using namespace dpgo;
// case file: r n nshared num_agents alt npub / npose[num_agents] / nshared x (agent frame) / pub_pose[npub] / pub_ptr[npub + 1] / ord[32]
int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *fp = std::fopen(argv[1], "r");
  if (!fp) return 2;
  int r, n, nshared, na, alt, npub;
  if (std::fscanf(fp, "%d %d %d %d %d %d", &r, &n, &nshared, &na, &alt, &npub) != 6) return 2;
  std::vector<int> npose(FD_FRONT_AGENTS, 0);
  for (int k = 0; k < na; ++k) if (std::fscanf(fp, "%d", &npose[k]) != 1) return 2;
  std::vector<unsigned> code((nshared + 1) / 2 + 1, 0u);
  for (int e = 0; e < nshared; ++e) {
    int sa, sf;
    if (std::fscanf(fp, "%d %d", &sa, &sf) != 2) return 2;
    code[e >> 1] |= (unsigned)(sf | (sa << 12)) << (16 * (e & 1));
  }
  std::vector<int> pub_pose(npub + 1, 0), pub_ptr(npub + 2, 0);
  for (int q = 0; q < npub; ++q) if (std::fscanf(fp, "%d", &pub_pose[q]) != 1) return 2;
  for (int q = 0; q <= npub; ++q) if (std::fscanf(fp, "%d", &pub_ptr[q]) != 1) return 2;
  unsigned char ord[32];
  for (int i = 0; i < 32; ++i) { int v; if (std::fscanf(fp, "%d", &v) != 1) return 2; ord[i] = (unsigned char)v; }
  std::fclose(fp);
  // every agent's Y array and its second copy `alt` vectors behind it: real memory, so every address formed is one of it
  std::vector<std::vector<double>> store(FD_FRONT_AGENTS);
  const double *ybase[FD_FRONT_AGENTS] = {};
  for (int k = 0; k < na; ++k) { store[k].assign((size_t)(alt + 1) * 4 * r * npose[k] + 1, 0.0); ybase[k] = store[k].data(); }
  // the image as assembly.hip packs it: [FD_FRONT_EDGES][16] coefficients (the first nshared used), the table behind them
  std::vector<double> img(FD_FRONT_IMAGE_DOUBLES, 0.0);
  for (int e = 0; e < nshared && e < FD_FRONT_EDGES; ++e) for (int i = 0; i < 16; ++i) img[(size_t)16 * e + i] = 1000.0 * e + i;
  FdFront ft;
  const bool ok = fd_front_build(ft, r, n, nshared, code.data(), na, ybase, npose.data(), alt, npub, pub_pose.data(), pub_ptr.data(), ord);
  std::printf("%d\n", ok ? 1 : 0);
  if (!ok) return 0;
  std::memcpy(&img[FD_FRONT_OFF_DOUBLES], &ft, sizeof ft);
  const FdFront *f = fd_front_of(img.data());
  for (int p = 0; p < 2; ++p)
    for (int s = 0; s < FD_FRONT_SLOTS; ++s) {
      int who = -1; long long off = -1;
      for (int k = 0; k < na; ++k)
        if (f->xaddr[p][s] >= store[k].data() && f->xaddr[p][s] + 4 * r <= store[k].data() + store[k].size()) { who = k; off = (long long)(f->xaddr[p][s] - store[k].data()); }
      std::printf("%d %lld\n", who, off);
    }
  for (int q = 0; q < FD_HEAD_NPUB_MAX; ++q) std::printf("%d %d %d %d\n", f->pub[q].pose, f->pub[q].vs_off, f->pub[q].pe0, f->pub[q].pe1);
  // the coefficients in front of the table are untouched
  int bad = 0;
  for (int e = 0; e < nshared; ++e) for (int i = 0; i < 16; ++i) bad += img[(size_t)16 * e + i] != 1000.0 * e + i;
  std::printf("%d %d %d %d\n", bad, FD_FRONT_SLOTS, FD_HEAD_NPUB_MAX, (int)FD_FRONT_OFF_DOUBLES);
  return 0;
}
"""

SLOTS, NPUB_MAX, EDGES, ALT = 192, 128, 160, 9
NSHARED = (0, 1, 63, 64, 65, 127, 128, 129, 160)
NPUB = (1, 64, 65, 128)
# private chunks first, the others behind them -- and neither group ascending: any permutation must be honoured
ORD = [(11 * i + 5) % 32 for i in range(32)]


def _case(r, n, nshared, npub, seed):
    rng = np.random.default_rng(seed)
    npose = [512, 499, 3, 1, 4095, 64, 17, 486]  # agents 0 .. 7: different pose counts
    agents = rng.integers(0, 8, nshared)
    frames = np.array([rng.integers(0, npose[a]) for a in agents], dtype=int)
    # neighbours on local agents 0 and 7, frames 0 and n - 1 of each
    fixed = [(0, 0), (0, npose[0] - 1), (7, 0), (7, npose[7] - 1), (4, npose[4] - 1)]
    for e, (a, f) in enumerate(fixed[:nshared]):
        agents[-1 - e], frames[-1 - e] = a, f
    pub_pose = np.sort(rng.choice(np.arange(1, n - 1), size=max(npub - 2, 0), replace=False)) if npub > 2 else np.zeros(0, int)
    pub_pose = np.concatenate([[0], pub_pose, [n - 1]])[:npub] if npub >= 2 else np.array([n - 1][:npub], dtype=int)
    cuts = np.sort(rng.integers(0, nshared + 1, max(npub - 1, 0)))
    pub_ptr = np.concatenate([[0], cuts, [nshared]]).astype(int)
    return dict(r=r, n=n, nshared=nshared, npub=npub, npose=npose, agents=agents, frames=frames, pub_pose=pub_pose.astype(int), pub_ptr=pub_ptr, ord=ORD)


def _write(c, path):
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n" % (c["r"], c["n"], c["nshared"], len(c["npose"]), ALT, c["npub"]))
        f.write(" ".join(str(v) for v in c["npose"]) + "\n")
        for a, fr in zip(c["agents"], c["frames"]):
            f.write("%d %d\n" % (a, fr))
        f.write(" ".join(str(v) for v in c["pub_pose"]) + "\n")
        f.write(" ".join(str(v) for v in c["pub_ptr"]) + "\n")
        f.write(" ".join(str(v) for v in c["ord"]) + "\n")


def _expected(c):
    r, ns = c["r"], c["nshared"]
    npose = np.asarray(c["npose"])
    ag = np.zeros(SLOTS, int)
    fr = np.zeros(SLOTS, int)
    ag[:ns], fr[:ns] = c["agents"], c["frames"]  # (slots behind the last edge: code 0 = agent 0, frame 0)
    x = np.zeros((2, SLOTS, 2), dtype=np.int64)
    for p in range(2):
        x[p, :, 0] = ag
        x[p, :, 1] = p * ALT * 4 * r * npose[ag] + 4 * r * fr
    place = np.zeros(32, int)
    place[np.asarray(c["ord"])] = np.arange(32)
    pub = np.zeros((NPUB_MAX, 4), dtype=np.int64)
    pp = c["pub_pose"]
    pub[: c["npub"], 0] = pp
    pub[: c["npub"], 1] = place[pp >> 4] * 64 * r + (pp & 15) * 4 * r
    pub[: c["npub"], 2] = c["pub_ptr"][:-1]
    pub[: c["npub"], 3] = c["pub_ptr"][1:]
    return x.reshape(-1, 2), pub


def _cases():
    out, seed = [], 0
    for r in (3, 4, 5):
        for ns in NSHARED:
            for npub in NPUB:
                seed += 1
                out.append(_case(r, 512 if (ns + npub) % 2 else 499, ns, npub, seed))
    return out


def _compile(d, flags, name):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = d / (name + ".cpp"), d / name
    src.write_text(PROGRAM)
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "dpgo_ros_amd", "csrc"), str(src), "-o", str(exe)] + flags
    return str(exe), subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("step_front_host")


@pytest.fixture(scope="module")
def program(workdir):
    exe, res = _compile(workdir, [], "step_front_host")
    assert res.returncode == 0, res.stderr
    return exe


def _run(exe, c, path, env=None):
    _write(c, path)
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    return res.stdout.split("\n")


def _check(lines, c):
    assert lines[0] == "1", "refused: r %d nshared %d npub %d" % (c["r"], c["nshared"], c["npub"])
    got_x = np.array([ln.split() for ln in lines[1:1 + 2 * SLOTS]], dtype=np.int64)
    got_pub = np.array([ln.split() for ln in lines[1 + 2 * SLOTS:1 + 2 * SLOTS + NPUB_MAX]], dtype=np.int64)
    x, pub = _expected(c)
    assert np.array_equal(got_x, x), (c["r"], c["nshared"], c["npub"], "xaddr")
    assert np.array_equal(got_pub, pub), (c["r"], c["nshared"], c["npub"], "pub")
    assert lines[1 + 2 * SLOTS + NPUB_MAX].split() == ["0", str(SLOTS), str(NPUB_MAX), str(16 * EDGES)]


def test_image_matches_the_formulas_at_every_slot_edge(program, workdir):
    cases = _cases()
    assert len(cases) == 3 * len(NSHARED) * len(NPUB)
    for c in cases:
        _check(_run(program, c, workdir / "case.txt"), c)


def test_what_the_table_cannot_hold_is_refused(program, workdir):
    ok = _case(5, 499, 160, 128, 7)
    _check(_run(program, ok, workdir / "case.txt"), ok)

    def refused(**kw):
        c = dict(ok)
        c.update(kw)
        return _run(program, c, workdir / "case.txt")[0] == "0"

    c161 = _case(5, 499, 161, 128, 8)
    assert _run(program, c161, workdir / "case.txt")[0] == "0", "161 shared edges"
    c129 = _case(5, 499, 160, 129, 9)
    assert _run(program, c129, workdir / "case.txt")[0] == "0", "129 public poses"
    # an edge whose frame lies beyond its agent, an agent without a base, a public pose beyond the agent, a broken edge cover
    fr = ok["frames"].copy(); fr[0] = ok["npose"][ok["agents"][0]]
    assert refused(frames=fr)
    assert refused(npose=ok["npose"][:7])  # (edges name agent 7)
    pp = ok["pub_pose"].copy(); pp[-1] = 499
    assert refused(pub_pose=pp)
    pt = ok["pub_ptr"].copy(); pt[-1] = 159
    assert refused(pub_ptr=pt)
    pt = ok["pub_ptr"].copy(); pt[0] = 1
    assert refused(pub_ptr=pt)


def test_the_same_program_under_address_and_undefined_sanitizers(workdir):
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # (the runtimes linked INTO the program where the compiler can: a stand-alone program then starts whatever else the
    # environment loads into every process in front of it)
    exe, res = _compile(workdir, san + ["-static-libasan", "-static-libubsan"], "step_front_host_san")
    if res.returncode != 0:
        exe, res = _compile(workdir, san, "step_front_host_san")
    if res.returncode != 0:
        assert "asan" in res.stderr or "ubsan" in res.stderr or "sanitize" in res.stderr, res.stderr
        pytest.skip("the sanitizer runtimes are not installed: " + res.stderr.strip().splitlines()[-1])
    for c in _cases()[::3] + [_case(5, 499, 161, 128, 8), _case(5, 499, 160, 129, 9)]:
        lines = _run(exe, c, workdir / "case_san.txt")
        if c["nshared"] <= EDGES and c["npub"] <= NPUB_MAX:
            _check(lines, c)
        else:
            assert lines[0] == "0"
