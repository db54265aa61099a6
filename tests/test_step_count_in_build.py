"""Host-only check that the waves of k_step_fd (csrc/step_deep.hip) which count themselves in at FD_SY_RQ do so behind their
last REQUEST and not behind its data.  step_deep.hip is compiled device-only to assembly with the flags csrc/Makefile uses
for step_deep.o; every role leaves a comment-only marker in front of its first request ("fd_role_entry k") and one in front
of its count ("fd_count_in k", the ds_add_u32 follows).  Between the two the instructions are walked in order and the vector
memory instructions issued so far are counted (k): vmcnt retires in order, so an `s_waitcnt vmcnt(n)` makes the wave wait for
data of its own exactly when n < k -- a BLOCKING wait.

    waves 4-5 (role 4)  no blocking wait
    wave 7    (role 7)  no blocking wait (its look-ahead addresses come from values held in scalar registers, not from a
                        per-agent record: no dependent vector load)
    wave 6    (role 6)  exactly three, each n = k - 1 .. k - 3 over the three address loads the pose requests are formed from
    every role          no s_waitcnt behind the role's last vector memory instruction -- but the one lgkmcnt wait of wave 6 for
                        the scalar loads that touch the argument struct, which it issues there (no vector data: unchanged)
    every instance      no flat_ instruction (one flat access makes the compiler's wait counting give up: vmcnt(0) everywhere)

What the parent of this check had (blocking waits; "behind": of them behind the last request):

    instance   wave 7        wave 6   waves 4-5
    <3, 24>    2, 1 behind   3        3, 1 behind
    <4, 24>    2, 1 behind   3        2, 1 behind
    <5, 24>    2, 1 behind   3        3, 1 behind

(the Nesterov state consumed in front of the count: vmcnt(1) after 47 loads in the chain waves of <5, 24>, vmcnt(20) after 57
in wave 7; ybase / npose of the look-ahead fetched by vector loads from the argument segment: vmcnt(2) after 37; two
write-after-write waits on dead halves of loads in the chain waves: vmcnt(16) after 17, vmcnt(8) after 25.)"""
import os
import re
import shlex
import shutil
import subprocess

import pytest

from tests.util import ROOT

CSRC = os.path.join(ROOT, "dpgo_ros_amd", "csrc")
ROLE_CHAIN, ROLE_POSES, ROLE_COEF = 4, 6, 7
VMEM = re.compile(r"^\s+(global_|buffer_|scratch_|flat_)\w+")


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
    out = tmp_path_factory.mktemp("step_count_in_build") / "step_deep.s"
    o = argv.index("-o")
    argv[o + 1] = str(out)
    argv[argv.index("-c")] = "-S"
    argv.insert(1, "--cuda-device-only")
    subprocess.check_call(argv, cwd=CSRC, stderr=subprocess.DEVNULL)
    return out.read_text()


def instances(text):
    """{mangled name: the lines of the function} of every k_step_fd instance"""
    out = {}
    names = re.findall(r"^\s*\.amdhsa_kernel (\S*k_step_fd\S*)$", text, re.M)
    for name in names:
        start = re.search(r"^%s:.*$" % re.escape(name), text, re.M)
        end = text.index(".amdhsa_kernel " + name)
        assert start and start.end() < end, name
        out[name] = text[start.end():end].splitlines()
    return out


def walk(lines, role):
    """the role's stretch of the function, entry marker to the ds_add_u32 of its count: (k, waits, tail, tail_other) -- vector
    memory instructions issued, every s_waitcnt that names vmcnt as (n, k at the wait), those of them behind the last vector
    memory instruction, the other s_waitcnt (lgkmcnt only: scalar loads, LDS) behind it"""
    ent = [i for i, ln in enumerate(lines) if re.search(r";\s*fd_role_entry %d\b" % role, ln)]
    cnt = [i for i, ln in enumerate(lines) if re.search(r";\s*fd_count_in %d\b" % role, ln)]
    assert len(ent) == 1 and len(cnt) == 1 and ent[0] < cnt[0], (role, ent, cnt)
    # the count itself follows its marker: the stretch ends at it
    add = [i for i in range(cnt[0] + 1, min(cnt[0] + 40, len(lines))) if re.match(r"^\s+ds_add_u32\b", lines[i])]
    assert add, (role, lines[cnt[0]:cnt[0] + 40])
    body = lines[ent[0]:add[0]]
    # one stretch of straight code: no other role's marker inside and no branch back into it (forward branches skip under an
    # empty exec mask), so the order of the text is the order of issue
    assert not any(re.search(r";\s*fd_role_entry ", ln) for ln in body[1:]), role
    assert sum(1 for ln in body if re.search(r";\s*fd_count_in ", ln)) == 1, role
    labels = {}
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            labels[m.group(1)] = i
    for i, ln in enumerate(body):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\w+)", ln)
        if m:
            assert labels.get(m.group(1), len(body)) > i, (role, ln)
    k, waits, others, last = 0, [], [], -1
    for i, ln in enumerate(body):
        if VMEM.match(ln):
            k += 1
            last = i
        m = re.match(r"^\s+s_waitcnt\b(.*)$", ln)
        if m:
            arg = m.group(1).split(";")[0]
            assert re.fullmatch(r"(\s*(vmcnt|lgkmcnt|expcnt)\(\d+\))+\s*", arg), (role, ln)  # (no raw immediate)
            v = re.search(r"vmcnt\((\d+)\)", arg)
            if v:
                waits.append((int(v.group(1)), k, i))
            else:
                others.append((arg.strip(), i))
    tail = [(n, kk) for n, kk, i in waits if i > last]
    tail_other = [a for a, i in others if i > last]
    return k, [(n, kk) for n, kk, i in waits], tail, tail_other


def blocking(waits):
    return [(n, k) for n, k in waits if n < k]


def test_count_ins_wait_for_no_data(assembly):
    inst = instances(assembly)
    assert len(inst) >= 3, sorted(inst)
    report = {}
    for name in sorted(inst):
        for role in (ROLE_CHAIN, ROLE_POSES, ROLE_COEF):
            k, waits, tail, tail_other = walk(inst[name], role)
            report[name, role] = (k, waits, tail, tail_other)
            print("%s role %d: %d requests, vmcnt waits (n, k) %s, blocking %s, behind the last request %s and %s"
                  % (name, role, k, waits, blocking(waits), tail, tail_other))
    for name in sorted(inst):
        flat = [ln for ln in inst[name] if re.match(r"^\s+flat_", ln)]
        assert not flat, (name, flat[:3])
        k, waits, tail, tail_other = report[name, ROLE_CHAIN]
        assert k > 0 and blocking(waits) == [], (name, "waves 4-5", blocking(waits))
        assert tail == [] and tail_other == [], (name, "waves 4-5", tail, tail_other)
        k, waits, tail, tail_other = report[name, ROLE_COEF]
        assert k > 0 and blocking(waits) == [], (name, "wave 7", blocking(waits))
        assert tail == [] and tail_other == [], (name, "wave 7", tail, tail_other)
        k, waits, tail, tail_other = report[name, ROLE_POSES]
        b = blocking(waits)
        # the three address loads are the role's first requests; wait q stands in front of the pose loads of address q and
        # leaves everything requested behind address q in flight: n = k - 1 - q
        assert len(b) == 3 and [n for n, kk in b] == [kk - 1 - q for q, (n, kk) in enumerate(b)], (name, "wave 6", b)
        # (wave 6 touches the argument struct behind its pose requests, as before: one lgkmcnt wait for those scalar loads, no data)
        assert tail == [] and len(tail_other) <= 1, (name, "wave 6", tail, tail_other)
