"""Host-only check of who hands the packed edge coefficients over in k_step_fd (csrc/step_deep.hip) and how.  The four
streamer waves request them as their FIRST loads, in front of the carried rows, write them to LDS behind a counted wait and
count at FD_SY_E; wave 7 no longer touches them.  step_deep.hip is compiled device-only to assembly as
tests/test_step_count_in_build.py does (its helpers are used); the streamers leave two comment-only markers, "fd_role_entry 0"
in front of their first request and "fd_e_count 0" in front of the count of their hand-off (behind the marker only the
election of the counting lane and its ds_add_u32 follow, as behind "fd_count_in k").  On every instance <R, 24>:

    streamers  between the two markers: no branch and no exec-mask save -- a lane beyond the last 16-byte part writes the
               clamped part to that part's own place, so no write is guarded;
               five coefficient loads and the R loads of the carried rows, five ds_write_b128;
               every `s_waitcnt vmcnt(n)` there has n >= R: vmcnt retires in order and the coefficients were requested first,
               so the carried rows stay in flight over the hand-off; the last of them has n == R (all five parts landed);
    wave 7     at least 20 vector memory instructions fewer between its entry and its count-in than the parent of this
               change issued (PARENT_ROLE7, read off the parent's assembly with `walk`: 45 / 50 / 55 at r = 3 / 4 / 5 -- the
               twenty coefficient loads of fd_cf_request among them);
    everywhere one s_barrier (the kernel's head), no flat_ instruction."""
import re

from tests.test_step_count_in_build import ROLE_COEF, VMEM, assembly, instances, walk  # noqa: F401 (assembly: the fixture)

ROLE_STREAM = 0
TRIPS = 5
PARENT_ROLE7 = {3: 45, 4: 50, 5: 55}


def _rank(name):
    m = re.search(r"k_step_fdILi(\d+)ELi(\d+)E", name)
    assert m, name
    return int(m.group(1))


def _m0(name):
    """the instance's count of private chunks, its second template argument"""
    return int(re.search(r"k_step_fdILi(\d+)ELi(\d+)E", name).group(2))


def streamer_stretch(lines):
    ent = [i for i, ln in enumerate(lines) if re.search(r";\s*fd_role_entry %d\b" % ROLE_STREAM, ln)]
    cnt = [i for i, ln in enumerate(lines) if re.search(r";\s*fd_e_count %d\b" % ROLE_STREAM, ln)]
    assert len(ent) == 1 and len(cnt) == 1 and ent[0] < cnt[0], (ent, cnt)
    # the count follows its marker
    assert any(re.match(r"^\s+ds_add_u32\b", ln) for ln in lines[cnt[0] + 1:cnt[0] + 40]), lines[cnt[0]:cnt[0] + 40]
    return lines[ent[0]:cnt[0]]


def test_streamers_hand_the_coefficients_over_without_a_branch(assembly):
    inst = instances(assembly)
    assert len(inst) >= 3, sorted(inst)
    for name in sorted(inst):
        r = _rank(name)
        body = streamer_stretch(inst[name])
        assert not any(re.search(r";\s*fd_role_entry ", ln) for ln in body[1:]), name
        branches = [ln for ln in body if re.match(r"^\s+(s_c?branch|s_setpc|s_\w+_saveexec)", ln)]
        labels = [ln for ln in body if re.match(r"^\.LBB\w+:", ln)]
        k, waits, writes = 0, [], 0
        for ln in body:
            if VMEM.match(ln):
                k += 1
            if re.match(r"^\s+ds_write_b128\b", ln):
                writes += 1
            m = re.match(r"^\s+s_waitcnt\b(.*)$", ln)
            if m:
                arg = m.group(1).split(";")[0]
                assert re.fullmatch(r"(\s*(vmcnt|lgkmcnt|expcnt)\(\d+\))+\s*", arg), (name, ln)  # (no raw immediate)
                v = re.search(r"vmcnt\((\d+)\)", arg)
                if v:
                    waits.append((int(v.group(1)), k))
        print("%s streamers: %d requests, %d ds_write_b128, vmcnt waits (n, k) %s, branches %s" % (name, k, writes, waits, branches))
        assert branches == [] and labels == [], (name, branches, labels)
        assert k == TRIPS + r and writes == TRIPS, (name, k, writes)
        # (waits that stand in front of the role's loads are waits for nothing: k == 0)
        live = [(n, kk) for n, kk in waits if kk > 0]
        assert live and all(n >= r for n, kk in live), (name, waits)
        assert min(n for n, kk in live) == r, (name, waits)


def test_streamers_hand_the_next_vector_over_with_the_stream_in_flight(assembly):
    """the second half of the change, on an instance <r, M0>: between "fd_stream_entry 0" (behind the requests for the rows of
    the next agent's carried gradient, in front of the M0 loads of its M) and "fd_n_count 0" (in front of the count of the
    hand-off N) there is no branch, M0 loads and ceil(M0 * 64 * r / 2 / 256) ds_write_b128, and every vmcnt wait leaves
    the M0 loads of M in flight -- the last with exactly M0; behind it the product waits chunk by chunk, vmcnt(M0 - 1)
    down to vmcnt(0)"""
    inst = instances(assembly)
    for name in sorted(inst):
        r, m0, lines = _rank(name), _m0(name), inst[name]
        ent = [i for i, ln in enumerate(lines) if re.search(r";\s*fd_stream_entry 0\b", ln)]
        cnt = [i for i, ln in enumerate(lines) if re.search(r";\s*fd_n_count 0\b", ln)]
        assert len(ent) == 1 and len(cnt) == 1 and ent[0] < cnt[0], (name, ent, cnt)
        body = lines[ent[0]:cnt[0]]
        assert not [ln for ln in body if re.match(r"^\s+(s_c?branch|s_setpc|s_\w+_saveexec)", ln) or re.match(r"^\.LBB\w+:", ln)], name
        k = sum(1 for ln in body if VMEM.match(ln))
        writes = sum(1 for ln in body if re.match(r"^\s+ds_write_b128\b", ln))
        waits = [int(m.group(1)) for ln in body for m in [re.match(r"^\s+s_waitcnt\b.*vmcnt\((\d+)\)", ln)] if m]
        print("%s streamers, next vector: %d loads of M, %d ds_write_b128, vmcnt waits %s" % (name, k, writes, waits))
        assert k == m0 and writes == (m0 * 64 * r // 2 + 255) // 256, (name, k, writes)
        assert waits and min(waits) == m0, (name, waits)
        # the product behind the hand-off: counted waits down to vmcnt(0), in falling order
        tail = []
        for ln in lines[cnt[0]:]:
            if VMEM.match(ln):
                break
            m = re.match(r"^\s+s_waitcnt\b.*vmcnt\((\d+)\)", ln)
            if m:
                tail.append(int(m.group(1)))
        assert tail == list(range(m0 - 1, -1, -1)), (name, tail)


def test_wave_7_lost_the_coefficient_loads(assembly):
    inst = instances(assembly)
    assert sorted(_rank(name) for name in inst) == sorted(PARENT_ROLE7), sorted(inst)
    for name in sorted(inst):
        k, waits, tail, tail_other = walk(inst[name], ROLE_COEF)
        print("%s wave 7: %d requests in front of its count-in (parent %d)" % (name, k, PARENT_ROLE7[_rank(name)]))
        assert 0 < k <= PARENT_ROLE7[_rank(name)] - 20, (name, k)


def test_no_barrier_added_and_no_flat_access(assembly):
    for name, lines in sorted(instances(assembly).items()):
        assert sum(1 for ln in lines if re.match(r"^\s+s_barrier\b", ln)) == 1, name
        assert not [ln for ln in lines if re.match(r"^\s+flat_", ln)], name
