"""Host-only check of how csrc/step_deep.hip is built: compiled device-only to assembly with the flags csrc/Makefile uses for
step_deep.o, every instance of k_step_fd must have its head (csrc/step_head.h, FD_HEAD_DWORDS leading dwords) delivered in
SGPRs at wave launch -- the preload length the compiler records -- and spill nothing: the chain waves sit at the register
limit, and a spill is scratch traffic in the memory queue the launch's critical chain waits on.  Reads those metadata
lines of the assembly and nothing else."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

from tests.util import ROOT

CSRC = os.path.join(ROOT, "dpgo_ros_amd", "csrc")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    # the command the Makefile would run for build/step_deep.o (dry run, nothing is built or touched)
    dry = subprocess.check_output(["make", "-C", CSRC, "-n", "-W", "step_deep.hip", "build/step_deep.o", "HIPCC=" + hipcc], text=True)
    line = [ln for ln in dry.splitlines() if "step_deep.hip" in ln and " -c " in ln]
    assert len(line) == 1, dry
    argv = shlex.split(line[0])
    assert "-amdgpu-kernarg-preload-count=14" in argv, argv
    out = tmp_path_factory.mktemp("step_head_build") / "step_deep.s"
    o = argv.index("-o")
    argv[o + 1] = str(out)
    argv[argv.index("-c")] = "-S"
    argv.insert(1, "--cuda-device-only")
    subprocess.check_call(argv, cwd=CSRC, stderr=subprocess.DEVNULL)
    return out.read_text()


def _head_dwords():
    text = open(os.path.join(CSRC, "step_head.h")).read()
    return int(re.search(r"constexpr int FD_HEAD_DWORDS = (\d+);", text).group(1))


def test_every_k_step_fd_instance_preloads_its_head_and_spills_nothing(assembly):
    want = _head_dwords()
    assert 0 < want <= 14
    preload = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S*k_step_fd\S*)\n(.*?)\.end_amdhsa_kernel", assembly, re.S):
        preload[m.group(1)] = int(re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", m.group(2)).group(1))
    spills = {}
    for m in re.finditer(r"\.name:\s+(\S*k_step_fd\S*)\n(.*?)\.wavefront_size:", assembly, re.S):
        spills[m.group(1)] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", m.group(2)).group(1)),
                              int(re.search(r"\.sgpr_spill_count:\s+(\d+)", m.group(2)).group(1)))
    assert len(preload) >= 3 and set(preload) == set(spills), (sorted(preload), sorted(spills))
    for name in sorted(preload):
        print("%s: preload length %d, vgpr spills %d, sgpr spills %d" % (name, preload[name], spills[name][0], spills[name][1]))
    for name in sorted(preload):
        assert preload[name] == want, (name, preload[name], want)
        assert spills[name][0] == 0, (name, "vgpr spills", spills[name][0])
        assert spills[name][1] == 0, (name, "sgpr spills", spills[name][1])
