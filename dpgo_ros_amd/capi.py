"""ctypes binding of libdpgo_hip.so -- the C-ABI declared in include/dpgo_hip.h.

Python-side mirror of the reference interface for this path: the `Agent` class carries the
DPGO::PGOAgent method names the ROS wrapper calls (src/PGOAgentROS.cpp), `Team`
the synchronous schedule of src/PGOAgentROS.cpp:129-220.  There is no CPU fallback: loading fails
loudly when the HIP extension has not been built, and every compute call needs a GPU.
"""
import ctypes as C
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (DPGO_HIP_LIB: an instrumented build of the same library, profiles/experiments/build_variant.sh)
LIB_PATH = os.environ.get("DPGO_HIP_LIB") or os.path.join(_HERE, "libdpgo_hip.so")
_LIB = None


class Measurement(C.Structure):
    _fields_ = [("r1", C.c_int), ("p1", C.c_int), ("r2", C.c_int), ("p2", C.c_int),
                ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("kappa", C.c_double), ("tau", C.c_double), ("weight", C.c_double),
                ("fixed_weight", C.c_int), ("is_known_inlier", C.c_int)]


MEAS_DTYPE = np.dtype([("r1", "<i4"), ("p1", "<i4"), ("r2", "<i4"), ("p2", "<i4"),
                       ("R", "<f8", (9,)), ("t", "<f8", (3,)),
                       ("kappa", "<f8"), ("tau", "<f8"), ("weight", "<f8"),
                       ("fixed_weight", "<i4"), ("is_known_inlier", "<i4")], align=True)
assert MEAS_DTYPE.itemsize == C.sizeof(Measurement)


class Params(C.Structure):
    _fields_ = [("d", C.c_int), ("r", C.c_int), ("num_robots", C.c_int), ("method", C.c_int),
                ("rgd_stepsize", C.c_double), ("rgd_use_preconditioner", C.c_int),
                ("rtr_iterations", C.c_int), ("rtr_tcg_iterations", C.c_int),
                ("gradnorm_tol", C.c_double), ("rtr_initial_radius", C.c_double),
                ("rtr_max_radius", C.c_double), ("precond_shift", C.c_double),
                ("acceleration", C.c_int), ("restart_interval", C.c_int),
                ("rel_change_tol", C.c_double), ("max_num_iters", C.c_int),
                ("robust_cost_type", C.c_int), ("gnc_barc", C.c_double),
                ("gnc_mu_step", C.c_double), ("gnc_init_mu", C.c_double),
                ("robust_opt_num_weight_updates", C.c_int), ("robust_opt_inner_iters", C.c_int),
                ("robust_opt_min_convergence_ratio", C.c_double), ("weights_as_float32", C.c_int),
                ("robust_opt_num_resets", C.c_int), ("precond_mode", C.c_int), ("status_every_iterate", C.c_int),
                ("rgd_line_search", C.c_int), ("rgd_ls_max_backoffs", C.c_int), ("rgd_ls_shrink", C.c_double),
                ("rgd_ls_sigma", C.c_double), ("tls_threshold", C.c_double), ("huber_threshold", C.c_double)]


class OptResult(C.Structure):
    _fields_ = [("success", C.c_int), ("f_init", C.c_double), ("f_opt", C.c_double),
                ("gradnorm_init", C.c_double), ("gradnorm_opt", C.c_double),
                ("rtr_outer_iters", C.c_int), ("tcg_iters_total", C.c_int),
                ("hessvec_count", C.c_int), ("precond_count", C.c_int), ("accepted", C.c_int),
                ("ls_backoffs", C.c_int)]


class Status(C.Structure):
    _fields_ = [("agent_id", C.c_int), ("state", C.c_int), ("instance_number", C.c_int),
                ("iteration_number", C.c_int), ("ready_to_terminate", C.c_int),
                ("relative_change", C.c_double)]


class Certificate(C.Structure):
    _fields_ = [("lambda_min", C.c_double), ("residual", C.c_double), ("norm_bound", C.c_double),
                ("certified", C.c_int), ("iterations", C.c_int), ("block", C.c_int), ("deflated", C.c_int)]

    def __repr__(self):
        return ("Certificate(lambda_min=%.6g, residual=%.3g, norm_bound=%.6g, certified=%d, iterations=%d, block=%d, "
                "deflated=%d)" % (self.lambda_min, self.residual, self.norm_bound, self.certified, self.iterations,
                                  self.block, self.deflated))


class Rounding(C.Structure):
    _fields_ = [("f_relaxed", C.c_double), ("f_rounded", C.c_double), ("sigma", C.c_double * 8),
                ("r", C.c_int), ("reflected", C.c_int), ("refined", C.c_int), ("num_degenerate", C.c_int)]

    def __repr__(self):
        return ("Rounding(f_relaxed=%.12g, f_rounded=%.12g, sigma=[%s], r=%d, reflected=%d, refined=%d, num_degenerate=%d)"
                % (self.f_relaxed, self.f_rounded, ", ".join("%.6g" % x for x in self.sigma[:self.r]), self.r,
                   self.reflected, self.refined, self.num_degenerate))


class Covariance(C.Structure):
    _fields_ = [("n", C.c_int), ("logdet", C.c_double), ("min_pivot", C.c_double), ("max_pivot", C.c_double),
                ("seconds_assemble", C.c_double), ("seconds_invert", C.c_double)]

    def __repr__(self):
        return ("Covariance(n=%d, logdet=%.12g, min_pivot=%.6g, max_pivot=%.6g, seconds_assemble=%.3g, seconds_invert=%.3g)"
                % (self.n, self.logdet, self.min_pivot, self.max_pivot, self.seconds_assemble, self.seconds_invert))


class Refine(C.Structure):
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("f0", C.c_double), ("f", C.c_double), ("grad_inf0", C.c_double),
                ("grad_inf", C.c_double)]


REFINE_STATUS = ("converged", "max_iters", "indefinite", "no_descent")  # DPGO_REFINE_*
METHOD_RTR, METHOD_RGD = 0, 1
COST_L2, COST_L1, COST_HUBER, COST_TLS, COST_GM, COST_GNC_TLS = 0, 1, 2, 3, 4, 5
WEIGHT_LIBRARY, WEIGHT_WRAPPER = 0, 1
OK, NOT_READY, ERR = 0, 1, -1
CERT_NO_DEFLATION, CERT_NO_PRECONDITIONER, CERT_ETA_RELATIVE = 1, 2, 4
ROUND_REFINE_TRANSLATIONS = 1
COV_SCHUR = 1  # DPGO_COV_SCHUR
COV_NESTED_DEFAULT_BLOCK = 256  # DPGO_COV_NESTED_DEFAULT_BLOCK
GATE_DENSE, GATE_SCHUR, GATE_NESTED = 0, 1, 2  # DPGO_GATE_*
JOINT_GREEDY, JOINT_GIVEN = 0, 1  # DPGO_JOINT_*
PRECOND_AUTO, PRECOND_DENSE, PRECOND_BLOCK_JACOBI, PRECOND_TWO_LEVEL = 0, 1, 2, 3

# every symbol include/dpgo_hip.h declares (checked by tests/test_abi.py)
EXPORTS = """dpgo_default_params dpgo_last_error dpgo_read_g2o dpgo_read_measurements_csv dpgo_partition
dpgo_free dpgo_odometry_init dpgo_chordal_init dpgo_fixed_stiefel dpgo_lift dpgo_team_create dpgo_team_destroy
dpgo_team_num_local dpgo_team_stream dpgo_team_synchronize dpgo_agent_add_measurements
dpgo_agent_num_poses dpgo_agent_num_measurements dpgo_agent_get_neighbors dpgo_agent_public_pose_ids
dpgo_agent_neighbor_pose_ids dpgo_agent_set_X dpgo_agent_get_X dpgo_agent_get_public_poses
dpgo_agent_update_neighbor_poses dpgo_agent_pack_public_poses_device
dpgo_agent_unpack_neighbor_poses_device dpgo_agent_iterate dpgo_agent_get_status
dpgo_agent_get_opt_result dpgo_agent_iteration_number dpgo_agent_publish_requested dpgo_agent_set_iteration_number
dpgo_agent_build_problem dpgo_agent_eval dpgo_agent_hessvec dpgo_agent_precondition dpgo_agent_get_Q
dpgo_agent_get_G dpgo_project_manifold dpgo_tangent_project dpgo_retract dpgo_agent_compute_residual
dpgo_agent_robust_weight dpgo_agent_update_measurement_weights dpgo_agent_set_measurement_weight
dpgo_agent_get_measurements dpgo_agent_should_update_weights dpgo_agent_clear_data_matrices
dpgo_error_threshold_at_quantile dpgo_team_set_schedule dpgo_team_set_initial dpgo_team_exchange_all
dpgo_agent_pull_local dpgo_team_time_kernel dpgo_team_run dpgo_team_get_coloring dpgo_team_run_colored dpgo_team_set_groups dpgo_team_run_group dpgo_team_step_begin dpgo_team_step_end dpgo_team_iteration dpgo_team_cost dpgo_team_update_weights dpgo_team_get_counters
dpgo_write_measurements_csv dpgo_write_g2o dpgo_write_trajectory_csv dpgo_robust_frame_alignment dpgo_robust_local_init dpgo_team_run_simultaneous
dpgo_team_should_terminate dpgo_team_run_schedule dpgo_agent_compute_residuals dpgo_agent_set_measurement_weights
dpgo_agent_reset_acceleration dpgo_team_prepare dpgo_agent_read_partials dpgo_agent_preconditioner dpgo_agent_preconditioner_info dpgo_agent_preconditioner_residual dpgo_two_level_plan dpgo_agent_export_state dpgo_team_import_peer dpgo_team_export_mailbox dpgo_team_import_mailbox dpgo_team_run_peer dpgo_agent_read_rtr_handoff
dpgo_comm_unique_id dpgo_comm_create dpgo_comm_destroy dpgo_comm_rank dpgo_comm_world dpgo_comm_library
dpgo_comm_allreduce_sum dpgo_comm_allreduce_max dpgo_team_attach_comm dpgo_team_detach_comm dpgo_team_exchange_all_ranks
dpgo_team_run_ranks dpgo_comm_global_cost dpgo_team_comm_counters dpgo_team_set_iteration_log dpgo_team_run_simultaneous_ranks
dpgo_team_run_group_ranks dpgo_rank_plan_simulate dpgo_team_set_uniform_schedule
dpgo_team_certificate_apply dpgo_team_certificate_precondition dpgo_team_certify dpgo_escape_point dpgo_team_round
dpgo_translations_given_rotations dpgo_team_certificate_apply_across dpgo_team_certify_across dpgo_team_round_across
dpgo_team_marginal_covariances dpgo_team_marginal_covariances_across
dpgo_covariance_nested_plan dpgo_team_covariance_nested_plan dpgo_team_marginal_covariances_nested
dpgo_team_gate_candidates dpgo_team_audit_measurements dpgo_team_pairwise_consistency dpgo_max_clique
dpgo_team_gate_candidates_jointly dpgo_team_linear_update dpgo_team_select_candidates dpgo_team_linear_removal
dpgo_team_gate_candidates_across dpgo_team_audit_measurements_across
dpgo_team_covariance_apply dpgo_team_linear_update_solved dpgo_team_refine dpgo_team_covariance_apply_across
dpgo_team_refine_across dpgo_team_linear_update_across""".split()


class DpgoError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libdpgo_hip.so is missing (%s): build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C dpgo_ros_amd/csrc`; there is no CPU fallback" % LIB_PATH)
        # One HIP runtime per process: torch ships its own libamdhip64 / librccl under /opt/rocm's sonames; loaded AFTER this
        # library (which binds /opt/rocm's) the process holds two runtimes and aborts at exit.  So where torch exists and has
        # not been imported yet, it goes first -- this library then binds to torch's copies through the sonames, whatever the
        # user's import order (DPGO_TORCH_FIRST=0: do not; dpgo_ros_amd.distributed needs torch anyway)
        if "torch" not in sys.modules and os.environ.get("DPGO_TORCH_FIRST", "1") != "0":
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        L.dpgo_last_error.restype = C.c_char_p
        L.dpgo_team_create.restype = C.c_void_p
        L.dpgo_team_stream.restype = C.c_void_p
        L.dpgo_comm_create.restype = C.c_void_p
        L.dpgo_agent_robust_weight.restype = C.c_double
        L.dpgo_error_threshold_at_quantile.restype = C.c_double
        _LIB = L
    return _LIB


def _d(a):
    return a.ctypes.data_as(C.c_void_p)


def two_level_plan(rowptr, col, max_sub=0):
    """the dissection of the two-level preconditioner for a block-CSR pattern (host arithmetic only):
    (sub_of[n] with -1 = separator, info dict)"""
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    n = len(rowptr) - 1
    sub_of = np.zeros(n, dtype=np.int32)
    info = np.zeros(6)
    _chk(lib().dpgo_two_level_plan(n, _d(rowptr), _d(col), int(max_sub), _d(sub_of), _d(info)), "two_level_plan")
    return sub_of, dict(subdomains=int(info[0]), separator_poses=int(info[1]), workgroups=int(info[2]),
                        producer_workgroups=int(info[3]), bytes_per_apply=info[4], worthwhile=bool(info[5]))


def _nested_plan_info(info):
    return dict(blocks=int(info[0]), separator_poses=int(info[1]), promoted_poses=int(info[2]), largest_block=int(info[3]),
                largest_coupling=int(info[4]), coupling_total=int(info[5]))


def covariance_nested_plan(robot_of, rowptr, col, max_block=None):
    """the sets of Team.covariances(method="nested") for a global block-CSR pattern in team order (host arithmetic only):
    (block_of[n] with the block index, -1 = separator pose, -2 = pose 0; info dict).  robot_of[n]: the robot of every pose,
    non-decreasing from 0; a pose joined to a pose of another robot is public.  max_block None: the library's default"""
    robot_of = np.ascontiguousarray(robot_of, dtype=np.int32)
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    n = len(rowptr) - 1
    if len(robot_of) != n:
        raise ValueError("covariance_nested_plan: robot_of holds %d entries, the pattern has %d rows" % (len(robot_of), n))
    block_of = np.zeros(n, dtype=np.int32)
    info = np.zeros(6, dtype=np.int32)
    _chk(lib().dpgo_covariance_nested_plan(n, _d(robot_of), _d(rowptr), _d(col), int(max_block or 0), _d(block_of), _d(info)),
         "covariance_nested_plan")
    return block_of, _nested_plan_info(info)


# ---- transports of the calls across teams (dpgo_transport_t) ----
_ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double))
_EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double),
                        C.POINTER(C.c_longlong))


class TransportStruct(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("rank", C.c_int), ("world", C.c_int), ("allgather", _ALLGATHER),
                ("exchange", _EXCHANGE)]


class Transport:
    """A transport the library calls (dpgo_transport_t): subclasses implement
        allgather(x) -> the world contributions of len(x) doubles each, concatenated in rank order,
        exchange(parts, recv_counts) -> one array per peer rank, recv_counts[p] doubles from p (parts[p] goes to p).
    This object keeps the C structure and its callbacks alive.  A callback that raises makes the library call fail on this
    participant (DPGO_ERR); `calls` counts the calls by kind."""

    def __init__(self, rank, world):
        self.rank, self.world = int(rank), int(world)
        self.calls = {"allgather": 0, "exchange": 0}
        self.error = None
        self._ag = _ALLGATHER(self._c_allgather)
        self._ex = _EXCHANGE(self._c_exchange)
        self.struct = TransportStruct(None, self.rank, self.world, self._ag, self._ex)

    def _c_allgather(self, ctx, inp, n, out):
        try:
            self.calls["allgather"] += 1
            x = np.ctypeslib.as_array(inp, shape=(n,)).copy() if n > 0 else np.zeros(0)
            got = np.ascontiguousarray(self.allgather(x), dtype=np.float64).reshape(-1)
            if got.size != self.world * n:
                raise ValueError("allgather returned %d doubles, expected %d" % (got.size, self.world * n))
            if got.size:
                C.memmove(out, got.ctypes.data, 8 * got.size)
            return 0
        except Exception as e:  # (an exception must not cross the C boundary)
            self.error = e
            return -1

    def _c_exchange(self, ctx, send, send_counts, recv, recv_counts):
        try:
            self.calls["exchange"] += 1
            sc = np.ctypeslib.as_array(send_counts, shape=(self.world,)).astype(np.int64)
            rc = np.ctypeslib.as_array(recv_counts, shape=(self.world,)).astype(np.int64)
            tot = int(sc.sum())
            data = np.ctypeslib.as_array(send, shape=(tot,)).copy() if tot else np.zeros(0)
            parts = np.split(data, np.cumsum(sc)[:-1])
            got = self.exchange(parts, rc)
            flat = [np.ascontiguousarray(g, dtype=np.float64).reshape(-1) for g in got]
            if len(flat) != self.world or any(f.size != int(c) for f, c in zip(flat, rc)):
                raise ValueError("exchange delivered sizes that differ from the counts")
            flat = np.concatenate(flat) if flat else np.zeros(0)
            if flat.size:
                C.memmove(recv, flat.ctypes.data, 8 * flat.size)
            return 0
        except Exception as e:
            self.error = e
            return -1

    def allgather(self, x):
        raise NotImplementedError

    def exchange(self, parts, recv_counts):
        raise NotImplementedError


class _LocalTransport(Transport):
    def __init__(self, group, rank):
        super().__init__(rank, group.world)
        self.group = group

    def allgather(self, x):
        g = self.group
        g.slot[self.rank] = x
        g.wait()
        sizes = {len(s) for s in g.slot}
        out = np.concatenate(g.slot) if len(sizes) == 1 else None
        g.wait()  # (nobody overwrites a slot before every participant has read them all)
        if out is None:
            raise ValueError("allgather: the participants passed different sizes %s" % sorted(sizes))
        return out

    def exchange(self, parts, recv_counts):
        g = self.group
        g.box[self.rank] = parts
        g.wait()
        got = [g.box[q][self.rank] for q in range(self.world)]
        g.wait()
        return got


class LocalGroup:
    """`world` transports for teams driven from threads of one process (one team per GPU, or a problem split on one GPU):
    a barrier with shared buffers.  A participant that leaves the sequence, or a barrier that waits longer than `timeout`
    seconds, breaks the barrier: every participant's call then fails instead of waiting forever."""

    def __init__(self, world, timeout=120.0):
        self.world = int(world)
        self.barrier = threading.Barrier(self.world, timeout=timeout)
        self.slot = [None] * self.world
        self.box = [None] * self.world
        self.transports = [_LocalTransport(self, q) for q in range(self.world)]

    def wait(self):
        self.barrier.wait()

    def abort(self):
        self.barrier.abort()

    def __len__(self):
        return self.world

    def __getitem__(self, q):
        return self.transports[q]

    def __iter__(self):
        return iter(self.transports)

    def run(self, fns, timeout=600.0):
        """call fns[q]() on one thread each (q = rank) and join them within `timeout` seconds: [(result, exception)];
        a thread still running at the end breaks the barrier and raises"""
        res = [(None, None)] * len(fns)

        def body(q):
            try:
                res[q] = (fns[q](), None)
            except Exception as e:
                res[q] = (None, e)
                self.abort()  # (the others fail at their next barrier instead of waiting for this one)

        th = [threading.Thread(target=body, args=(q,), daemon=True) for q in range(len(fns))]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout)
        if any(t.is_alive() for t in th):
            self.abort()
            raise TimeoutError("a participant did not return within %g s" % timeout)
        return res


def _owner_array(owner_of_robot):
    return np.ascontiguousarray(owner_of_robot, dtype=np.int32)


_REC_INTS = ("r1", "p1", "r2", "p2", "fixed_weight", "is_known_inlier")
_REC_DOUBLES = 4 + 9 + 3 + 3 + 2  # a MEAS_DTYPE record as plain doubles, the integers exact


def records_to_doubles(recs):
    """MEAS_DTYPE records as [K, 21] doubles (r1, p1, r2, p2, R, t, kappa, tau, weight, fixed_weight, is_known_inlier): what a
    transport's allgather carries"""
    recs = np.ascontiguousarray(recs, dtype=MEAS_DTYPE).reshape(-1)
    out = np.zeros((len(recs), _REC_DOUBLES))
    for c, f in enumerate(("r1", "p1", "r2", "p2")):
        out[:, c] = recs[f]
    out[:, 4:13], out[:, 13:16] = recs["R"], recs["t"]
    out[:, 16], out[:, 17], out[:, 18] = recs["kappa"], recs["tau"], recs["weight"]
    out[:, 19], out[:, 20] = recs["fixed_weight"], recs["is_known_inlier"]
    return out


def records_from_doubles(x):
    """the inverse of records_to_doubles"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, _REC_DOUBLES)
    recs = np.zeros(len(x), dtype=MEAS_DTYPE)
    for c, f in enumerate(("r1", "p1", "r2", "p2")):
        recs[f] = x[:, c].astype(np.int32)
    recs["R"], recs["t"] = x[:, 4:13], x[:, 13:16]
    recs["kappa"], recs["tau"], recs["weight"] = x[:, 16], x[:, 17], x[:, 18]
    recs["fixed_weight"], recs["is_known_inlier"] = x[:, 19].astype(np.int32), x[:, 20].astype(np.int32)
    return recs


def join_records_by_robot(lists_per_rank, owner_of_robot):
    """One list of MEAS_DTYPE records for the whole problem from the lists of the participants (lists_per_rank[q]: what
    rank q holds, in its own order; owner_of_robot[i]: the rank that holds robot i).  A record belongs to the lower robot of a
    shared edge and to r1 otherwise; the joined list takes, robot after robot in id order, that robot's records from the rank
    that holds it, in the order they have there -- so the weights are the owner's, a copy that the higher robot's rank also
    lists is dropped, and a shared edge that its rank lists twice (both copies) appears once, as the first.  This is
    Team.measurements_once() of a single team that holds every robot."""
    own = np.asarray(owner_of_robot, dtype=np.int64).reshape(-1)
    out = []
    for i in range(len(own)):
        recs = np.ascontiguousarray(lists_per_rank[int(own[i])], dtype=MEAS_DTYPE).reshape(-1)
        key = np.where(recs["r1"] == recs["r2"], recs["r1"], np.minimum(recs["r1"], recs["r2"]))
        seen = set()
        for e in recs[key == i]:
            edge = (int(e["r1"]), int(e["p1"]), int(e["r2"]), int(e["p2"]))
            if e["r1"] != e["r2"] and edge in seen:
                continue
            seen.add(edge)
            out.append(e)
    return np.array(out, dtype=MEAS_DTYPE) if out else np.zeros(0, dtype=MEAS_DTYPE)


def _chk(rc, what):
    if rc < 0:
        raise DpgoError("%s failed: %s" % (what, lib().dpgo_last_error().decode()))
    return rc


def default_params(r=5, num_robots=1, **kw):
    p = Params()
    lib().dpgo_default_params(C.byref(p), r, num_robots)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def read_g2o(path, weight_mode=WEIGHT_LIBRARY):
    out, n = C.c_void_p(), C.c_int()
    nm = lib().dpgo_read_g2o(path.encode(), weight_mode, C.byref(out), C.byref(n))
    if nm < 0:
        raise FileNotFoundError(path)
    raw = C.string_at(out, nm * MEAS_DTYPE.itemsize)
    lib().dpgo_free(out)
    return np.frombuffer(raw, dtype=MEAS_DTYPE).copy(), n.value


def read_csv(path, weight_mode=WEIGHT_LIBRARY):
    out = C.c_void_p()
    nm = lib().dpgo_read_measurements_csv(path.encode(), weight_mode, C.byref(out))
    if nm < 0:
        raise FileNotFoundError(path)
    raw = C.string_at(out, nm * MEAS_DTYPE.itemsize)
    lib().dpgo_free(out)
    return np.frombuffer(raw, dtype=MEAS_DTYPE).copy()


def robust_local_init(m, num_poses, params, device=0):
    """single-robot GNC-TLS solve on the device -> (T [12 n], final weights in input order)"""
    m = np.ascontiguousarray(m)
    T, w = np.zeros(12 * num_poses), np.zeros(len(m))
    _chk(lib().dpgo_robust_local_init(device, _d(m), len(m), num_poses, C.byref(params), _d(T), _d(w)), "robust_local_init")
    return T, w


def robust_frame_alignment(Tc, max_rotation_error_rad=0.5, max_translation_error=1.0, min_inliers=2):
    """Tc: n x 12 candidate transforms (3x4 column-major).  Returns (T, inlier mask) or None when fewer than
    min_inliers candidates agree."""
    Tc = np.ascontiguousarray(Tc, dtype=np.float64).reshape(-1, 12)
    T, inl = np.zeros(12), np.zeros(len(Tc), dtype=np.int32)
    rc = lib().dpgo_robust_frame_alignment(_d(Tc), len(Tc), C.c_double(max_rotation_error_rad),
                                           C.c_double(max_translation_error), min_inliers, _d(T), _d(inl))
    return (T, inl.astype(bool)) if rc == OK else None


def write_csv(path, m):
    """measurement list -> the CSV that read_csv / PGOLogger::loadMeasurements reads (weights included)"""
    m = np.ascontiguousarray(m)
    if lib().dpgo_write_measurements_csv(str(path).encode(), _d(m), len(m)) < 0:
        raise OSError("cannot write %s" % path)


def write_g2o(path, m, T=None, num_poses=0, robot_offsets=None):
    m = np.ascontiguousarray(m)
    Tp = _d(np.ascontiguousarray(T, dtype=np.float64)) if T is not None else None
    off = np.ascontiguousarray(robot_offsets, dtype=np.int32) if robot_offsets is not None else None
    if lib().dpgo_write_g2o(str(path).encode(), _d(m), len(m), Tp, num_poses if T is not None else 0,
                            _d(off) if off is not None else None) < 0:
        raise OSError("cannot write %s" % path)


def write_trajectory_csv(path, T, num_poses):
    T = np.ascontiguousarray(T, dtype=np.float64)
    if lib().dpgo_write_trajectory_csv(str(path).encode(), _d(T), num_poses) < 0:
        raise OSError("cannot write %s" % path)


class IterationLog:
    """per-iteration CSV in the column order of the reference's log (src/PGOAgentROS.cpp:863-864, 883-891),
    followed by the global-cost column the reference does not have."""
    HEADER = ("robot_id, cluster_id, num_active_robots, iteration, num_poses, bytes_received, "
              "iter_time_sec, total_time_sec, rel_change, global_cost \n")

    def __init__(self, path):
        self.f = open(path, "w")
        self.f.write(self.HEADER)

    def log(self, robot_id, cluster_id, num_active_robots, iteration, num_poses, bytes_received, iter_time_sec,
            total_time_sec, rel_change, global_cost=float("nan")):
        self.f.write("%d,%d,%d,%d,%d,%d,%.9g,%.9g,%.17g,%.17g\n" % (robot_id, cluster_id, num_active_robots, iteration,
                                                                     num_poses, bytes_received, iter_time_sec,
                                                                     total_time_sec, rel_change, global_cost))

    def log_string(self, s):  # "TERMINATE", "UPDATE_WEIGHT", ... (src/PGOAgentROS.cpp:896-909)
        self.f.write(s + "\n")

    def close(self):
        self.f.close()


def partition(m, num_poses, num_robots, weight_mode=WEIGHT_LIBRARY):
    m = m.copy()
    lib().dpgo_partition(_d(m), len(m), num_poses, num_robots, weight_mode)
    return m


def odometry_init(m, num_poses):
    T = np.zeros(12 * num_poses)
    lib().dpgo_odometry_init(_d(np.ascontiguousarray(m)), len(m), num_poses, _d(T))
    return T


def chordal_init(m, num_poses, device=0):
    T = np.zeros(12 * num_poses)
    _chk(lib().dpgo_chordal_init(device, _d(np.ascontiguousarray(m)), len(m), num_poses, _d(T)), "chordal_init")
    return T


def translations_given_rotations(m, num_poses, T, device=0):
    """the translations minimising sum_e w_e tau_e |t_j - t_i - R_i t~_e|^2 with t_0 = 0 for the rotations of T (12 doubles
    per pose, single-robot numbering): a copy of T with its translations replaced"""
    out = np.array(T, dtype=np.float64).reshape(-1)
    assert out.size == 12 * num_poses
    _chk(lib().dpgo_translations_given_rotations(device, _d(np.ascontiguousarray(m)), len(m), int(num_poses), _d(out)),
         "translations_given_rotations")
    return out


def fixed_stiefel(r):
    Y = np.zeros(3 * r)
    lib().dpgo_fixed_stiefel(r, _d(Y))
    return Y


def lift(T, num_poses, YLift, r):
    X = np.zeros(r * 4 * num_poses)
    lib().dpgo_lift(_d(np.ascontiguousarray(T)), num_poses, _d(np.ascontiguousarray(YLift)), r, _d(X))
    return X


def escape_point(X, r, num_poses, v, alpha):
    """staircase step (host arithmetic): the rank r+1 point [X; 0] + alpha [0; v^T], rotation blocks projected back to the
    Stiefel manifold.  X: r x 4n in the iterate layout, v: 4n"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    assert X.size == r * 4 * num_poses and v.size == 4 * num_poses
    out = np.zeros((r + 1) * 4 * num_poses)
    _chk(lib().dpgo_escape_point(_d(X), int(r), int(num_poses), _d(v), C.c_double(alpha), _d(out)), "escape_point")
    return out


def error_threshold_at_quantile(q, dim):
    return lib().dpgo_error_threshold_at_quantile(C.c_double(q), dim)


class Agent:
    """One robot's block; method names follow DPGO::PGOAgent as used by PGOAgentROS."""

    def __init__(self, team, agent_id):
        self.team = team
        self.t = team.h
        self.id = agent_id
        self.r = team.r

    # --- structure
    def add_measurements(self, m):
        m = np.ascontiguousarray(m)
        _chk(lib().dpgo_agent_add_measurements(self.t, self.id, _d(m), len(m)), "addMeasurement")

    @property
    def n(self):
        return _chk(lib().dpgo_agent_num_poses(self.t, self.id), "num_poses")

    def _vec(self):
        return np.zeros(self.r * 4 * self.n)

    def _ids(self, fn, *args):
        c = _chk(fn(self.t, self.id, *args, None), fn.__name__)
        out = np.zeros(max(c, 1), dtype=np.int32)
        fn(self.t, self.id, *args, _d(out))
        return out[:c]

    def neighbors(self):
        return self._ids(lib().dpgo_agent_get_neighbors).tolist()

    def public_pose_ids(self, nbr):
        return self._ids(lib().dpgo_agent_public_pose_ids, nbr)

    def neighbor_pose_ids(self, nbr):
        return self._ids(lib().dpgo_agent_neighbor_pose_ids, nbr)

    # --- iterate / state
    def set_X(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert X.size == self.r * 4 * self.n
        _chk(lib().dpgo_agent_set_X(self.t, self.id, _d(X)), "set_X")

    def _get(self, which):
        X = self._vec()
        _chk(lib().dpgo_agent_get_X(self.t, self.id, which, _d(X)), "get_X")
        return X

    def get_X(self):
        return self._get(0)

    def get_Y(self):
        return self._get(1)

    def get_V(self):
        return self._get(2)

    def get_public_poses(self, nbr, aux=False):
        ids = self.public_pose_ids(nbr)
        out = np.zeros(max(len(ids), 1) * 4 * self.r)
        _chk(lib().dpgo_agent_get_public_poses(self.t, self.id, nbr, int(aux), _d(out)), "getSharedPoseDict")
        return ids, out[:len(ids) * 4 * self.r]

    def update_neighbor_poses(self, nbr, frames, poses, aux=False):
        frames = np.ascontiguousarray(frames, dtype=np.int32)
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        _chk(lib().dpgo_agent_update_neighbor_poses(self.t, self.id, nbr, int(aux), len(frames), _d(frames), _d(poses)),
             "updateNeighborPoses")

    def iterate(self, do_opt=True):
        return _chk(lib().dpgo_agent_iterate(self.t, self.id, int(do_opt)), "iterate") == OK

    def status(self):
        s = Status()
        _chk(lib().dpgo_agent_get_status(self.t, self.id, C.byref(s)), "getStatus")
        return s

    def opt_result(self):
        s = OptResult()
        _chk(lib().dpgo_agent_get_opt_result(self.t, self.id, C.byref(s)), "opt_result")
        return s

    def preconditioner(self):
        """1 dense inverse, 3 two-level (both exact), 2 block-Jacobi (on request, or where neither exact form fits)"""
        return _chk(lib().dpgo_agent_preconditioner(self.t, self.id), "preconditioner")

    def preconditioner_residual(self):
        """|z (Q + shift I) - v| / |v| for the operator the kernels apply (fixed pseudo-random v)"""
        rel = C.c_double()
        _chk(lib().dpgo_agent_preconditioner_residual(self.t, self.id, C.byref(rel)), "preconditioner_residual")
        return rel.value

    def preconditioner_info(self):
        out = np.zeros(8)
        _chk(lib().dpgo_agent_preconditioner_info(self.t, self.id, _d(out)), "preconditioner_info")
        return dict(mode=int(out[0]), subdomains=int(out[1]), separator_poses=int(out[2]), workgroups=int(out[3]),
                    producer_workgroups=int(out[4]), bytes_per_apply=out[5], dense_bytes=out[6], largest_subdomain=int(out[7]))

    def publish_requested(self, clear=False):
        return bool(lib().dpgo_agent_publish_requested(self.t, self.id, int(clear)))

    # --- QuadraticProblem surface
    def build_problem(self, aux=False):
        return _chk(lib().dpgo_agent_build_problem(self.t, self.id, int(aux)), "build_problem")

    def eval(self, X):
        f = C.c_double()
        eg, rg = self._vec(), self._vec()
        _chk(lib().dpgo_agent_eval(self.t, self.id, _d(np.ascontiguousarray(X)), C.byref(f), _d(eg), _d(rg)), "eval")
        return f.value, eg, rg

    def hessvec(self, X, eta):
        out = self._vec()
        _chk(lib().dpgo_agent_hessvec(self.t, self.id, _d(np.ascontiguousarray(X)), _d(np.ascontiguousarray(eta)), _d(out)),
             "hessvec")
        return out

    def precondition(self, X, V):
        out = self._vec()
        _chk(lib().dpgo_agent_precondition(self.t, self.id, _d(np.ascontiguousarray(X)), _d(np.ascontiguousarray(V)), _d(out)),
             "precondition")
        return out

    def get_Q(self):
        nb = _chk(lib().dpgo_agent_get_Q(self.t, self.id, None, None, None), "get_Q")
        rowptr = np.zeros(self.n + 1, dtype=np.int32)
        col = np.zeros(nb, dtype=np.int32)
        val = np.zeros(16 * nb)
        lib().dpgo_agent_get_Q(self.t, self.id, _d(rowptr), _d(col), _d(val))
        return rowptr, col, val

    def get_G(self):
        G = self._vec()
        _chk(lib().dpgo_agent_get_G(self.t, self.id, _d(G)), "get_G")
        return G

    # --- robust path
    def measurements(self):
        c = _chk(lib().dpgo_agent_get_measurements(self.t, self.id, None), "measurements")
        m = np.zeros(max(c, 1), dtype=MEAS_DTYPE)
        lib().dpgo_agent_get_measurements(self.t, self.id, _d(m))
        return m[:c]

    def compute_residual(self, meas_row):
        m = np.ascontiguousarray(np.array([meas_row], dtype=MEAS_DTYPE))
        res = C.c_double()
        rc = _chk(lib().dpgo_agent_compute_residual(self.t, self.id, _d(m), C.byref(res)), "computeMeasurementResidual")
        return rc == OK, res.value

    def robust_weight(self, residual):
        return lib().dpgo_agent_robust_weight(self.t, self.id, C.c_double(residual))

    def update_measurement_weights(self):
        _chk(lib().dpgo_agent_update_measurement_weights(self.t, self.id), "updateMeasurementWeights")

    def set_measurement_weight(self, r1, p1, r2, p2, w, fixed=False):
        return lib().dpgo_agent_set_measurement_weight(self.t, self.id, r1, p1, r2, p2, C.c_double(w), int(fixed)) == OK

    def clear_data_matrices(self):
        _chk(lib().dpgo_agent_clear_data_matrices(self.t, self.id), "clearDataMatrices")

    def pull_local(self):
        _chk(lib().dpgo_agent_pull_local(self.t, self.id), "pull_local")

    # --- device-buffer exchange (RCCL payloads)
    def pack_public_poses_device(self, nbr, aux, dev_ptr):
        return _chk(lib().dpgo_agent_pack_public_poses_device(self.t, self.id, nbr, int(aux), C.c_void_p(dev_ptr)), "pack")

    def unpack_neighbor_poses_device(self, nbr, aux, dev_ptr):
        return _chk(lib().dpgo_agent_unpack_neighbor_poses_device(self.t, self.id, nbr, int(aux), C.c_void_p(dev_ptr)), "unpack")


COMM_ID_BYTES = 128


def comm_unique_id():
    """DPGO_COMM_ID_BYTES bytes that name a new RCCL communicator: obtained on ONE rank, handed to every rank (any channel)"""
    b = (C.c_ubyte * COMM_ID_BYTES)()
    _chk(lib().dpgo_comm_unique_id(b), "comm_unique_id")
    return bytes(b)


def comm_library():
    """(path, version code) of the RCCL the library bound at run time"""
    buf = C.create_string_buffer(512)
    v = _chk(lib().dpgo_comm_library(buf, 512), "comm_library")
    return buf.value.decode(), v


def rank_plan_simulate(owner, npub, rank, world, sel_ids, acceleration=1, max_delayed_iterations=0, r=5):
    """the exchange's planning layer replayed for one rank (host arithmetic only): array [1 + iters, world, 4] of
    {doubles sent, doubles received, hash of the sent slabs, hash of the received slabs} per batch and peer rank"""
    owner = np.ascontiguousarray(owner, dtype=np.int32)
    N = len(owner)
    npub = np.ascontiguousarray(npub, dtype=np.int32).reshape(N, N)
    sel = np.ascontiguousarray(sel_ids, dtype=np.int32)
    out = np.zeros((1 + len(sel), world, 4), dtype=np.int64)
    _chk(lib().dpgo_rank_plan_simulate(N, int(world), int(rank), _d(owner), _d(npub), int(acceleration), int(max_delayed_iterations), int(r),
                                       _d(sel), len(sel), _d(out)), "rank_plan_simulate")
    return out


class Comm:
    """RCCL communicator owned by the library (csrc/rank_exchange.cpp): one per process, every rank takes part in its
    creation -- also the ranks that own no robot."""

    def __init__(self, unique_id, rank, world, device=0):
        b = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(unique_id)
        h = lib().dpgo_comm_create(device, b, rank, world)
        if not h:
            raise DpgoError("dpgo_comm_create: " + lib().dpgo_last_error().decode())
        self.h = C.c_void_p(h)
        self.rank, self.world, self.device = rank, world, device

    def allreduce(self, values, op="sum", stream=None):
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        fn = lib().dpgo_comm_allreduce_sum if op == "sum" else lib().dpgo_comm_allreduce_max
        _chk(fn(self.h, C.c_void_p(stream) if stream else None, _d(v), len(v)), "comm_allreduce")
        return v

    def global_cost(self, team=None, stream=None):
        f = C.c_double()
        _chk(lib().dpgo_comm_global_cost(self.h, team.h if team is not None else None, C.c_void_p(stream) if stream else None,
                                         C.byref(f)), "comm_global_cost")
        return f.value

    def close(self):
        if getattr(self, "h", None):
            lib().dpgo_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Team:
    """The agents resident on one GPU.  With every agent of the problem local, `run` executes the
    synchronous RBCD schedule entirely on the device."""

    def __init__(self, params, agent_ids, device=0, stream=None):
        self.params = params
        self.r = params.r
        ids = np.ascontiguousarray(agent_ids, dtype=np.int32)
        h = lib().dpgo_team_create(device, C.byref(params), len(ids), _d(ids), C.c_void_p(stream) if stream else None)
        if not h:
            raise DpgoError("dpgo_team_create: " + lib().dpgo_last_error().decode())
        self.h = C.c_void_p(h)
        self.agents = {int(i): Agent(self, int(i)) for i in ids}
        self.ids = [int(i) for i in ids]

    def close(self):
        if getattr(self, "h", None):
            lib().dpgo_team_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_measurements(cls, meas, params, device=0, local_ids=None, stream=None):
        ids = list(range(params.num_robots)) if local_ids is None else list(local_ids)
        t = cls(params, ids, device=device, stream=stream)
        meas = np.ascontiguousarray(meas)
        for i in ids:
            t.agents[i].add_measurements(meas)
        return t

    def offsets(self):
        off, acc = [], 0
        for i in self.ids:
            off.append(acc)
            acc += self.agents[i].n
        return np.array(off, dtype=np.int32)

    def set_schedule(self, order):
        o = np.ascontiguousarray(order, dtype=np.int32)
        _chk(lib().dpgo_team_set_schedule(self.h, _d(o), len(o)), "set_schedule")

    def set_uniform_schedule(self, seed, length):
        """UpdateRule::Uniform (src/PGOAgentROS.cpp:446-463) with a given seed: draws `length` token holders, installs them as
        the schedule and returns them"""
        order = np.zeros(int(length), dtype=np.int32)
        _chk(lib().dpgo_team_set_uniform_schedule(self.h, C.c_uint(int(seed)), int(length), _d(order)), "set_uniform_schedule")
        return order

    def set_initial(self, T, YLift, offsets=None):
        off = self.offsets() if offsets is None else np.ascontiguousarray(offsets, dtype=np.int32)
        _chk(lib().dpgo_team_set_initial(self.h, _d(np.ascontiguousarray(T)), _d(np.ascontiguousarray(YLift)), _d(off)),
             "set_initial")

    def exchange_all(self):
        _chk(lib().dpgo_team_exchange_all(self.h), "exchange_all")

    def run(self, iters):
        _chk(lib().dpgo_team_run(self.h, iters), "team_run")

    def prepare(self, iters):
        """instantiate the graphs a run of `iters` iterations will replay, executing nothing"""
        _chk(lib().dpgo_team_prepare(self.h, iters), "prepare")

    def coloring(self):
        col = np.zeros(len(self.ids), dtype=np.int32)
        nc = _chk(lib().dpgo_team_get_coloring(self.h, _d(col)), "get_coloring")
        return nc, col

    def export_state(self, agent_id):
        """(64-byte IPC handle, offset of X, offset of Y, poses) of a local agent's arrays, for dpgo_team_import_peer"""
        h = (C.c_ubyte * 64)()
        ox, oy, n = C.c_longlong(), C.c_longlong(), C.c_int()
        _chk(lib().dpgo_agent_export_state(self.h, agent_id, h, C.byref(ox), C.byref(oy), C.byref(n)), "export_state")
        return bytes(h), ox.value, oy.value, n.value

    def import_peer(self, robot_id, handle, off_x, off_y, n):
        """read the public poses of a robot that lives in another process in place (HIP IPC / peer access)"""
        h = (C.c_ubyte * 64).from_buffer_copy(handle)
        _chk(lib().dpgo_team_import_peer(self.h, robot_id, h, C.c_longlong(off_x), C.c_longlong(off_y), n), "import_peer")

    def export_mailbox(self):
        """64-byte IPC handle of this team's mailbox (the device-side UPDATE token, dpgo_team_run_peer)"""
        h = (C.c_ubyte * 64)()
        _chk(lib().dpgo_team_export_mailbox(self.h, h), "export_mailbox")
        return bytes(h)

    def import_mailbox(self, handle, robot_ids):
        h = (C.c_ubyte * 64).from_buffer_copy(handle)
        ids = np.ascontiguousarray(robot_ids, dtype=np.int32)
        _chk(lib().dpgo_team_import_mailbox(self.h, h, _d(ids), len(ids)), "import_mailbox")

    def run_peer(self, sel_ids):
        """len(sel_ids) global iterations, robot sel_ids[q] holding the token in the q-th, enqueued without host
        synchronisation; remote neighbours are read in place and ordered by the device-side mailboxes"""
        ids = np.ascontiguousarray(sel_ids, dtype=np.int32)
        _chk(lib().dpgo_team_run_peer(self.h, _d(ids), len(ids)), "run_peer")

    def attach_comm(self, comm, owner_of_robot, max_delayed_iterations=0, loopback=False):
        """from here on run_ranks / exchange_all_ranks move the public poses between ranks with ncclSend / ncclRecv enqueued
        by the library on the team stream (include/dpgo_hip.h); loopback (world size 1): every pair as a self-send"""
        o = np.ascontiguousarray(owner_of_robot, dtype=np.int32)
        assert len(o) == self.params.num_robots
        _chk(lib().dpgo_team_attach_comm(self.h, comm.h, _d(o), int(max_delayed_iterations), int(bool(loopback))), "attach_comm")
        self._comm = comm  # (keeps the communicator alive as long as the team uses it)

    def detach_comm(self):
        _chk(lib().dpgo_team_detach_comm(self.h), "detach_comm")
        self._comm = None

    def exchange_all_ranks(self):
        _chk(lib().dpgo_team_exchange_all_ranks(self.h), "exchange_all_ranks")

    def run_ranks(self, sel_ids):
        """len(sel_ids) global iterations with robot sel_ids[q] holding the token in the q-th; the exchange is RCCL
        point-to-point inside the library, nothing synchronises with the host"""
        ids = np.ascontiguousarray(sel_ids, dtype=np.int32)
        _chk(lib().dpgo_team_run_ranks(self.h, _d(ids), len(ids)), "run_ranks")

    def run_simultaneous_ranks(self, ticks):
        """lockstep ASAPP ticks with the boundary slabs moved by the library (one batch of ncclSend / ncclRecv per tick)"""
        _chk(lib().dpgo_team_run_simultaneous_ranks(self.h, int(ticks)), "run_simultaneous_ranks")

    def run_group_ranks(self, g, count):
        """one colour class across ranks: members receive what moved, then update at once (set_groups first)"""
        _chk(lib().dpgo_team_run_group_ranks(self.h, int(g), int(count)), "run_group_ranks")

    def comm_counters(self):
        """messages sent / received by this rank and their bytes"""
        out = np.zeros(4)
        _chk(lib().dpgo_team_comm_counters(self.h, _d(out)), "comm_counters")
        return dict(messages_sent=int(out[0]), messages_received=int(out[1]), bytes_sent=out[2], bytes_received=out[3])

    def should_terminate(self):
        """PGOAgent::shouldTerminate() as the leader evaluates it (src/PGOAgentROS.cpp:208)"""
        return bool(_chk(lib().dpgo_team_should_terminate(self.h), "should_terminate"))

    def run_schedule(self, max_iters):
        """the synchronous schedule with the leader's TERMINATE / UPDATE_WEIGHT decisions (src/PGOAgentROS.cpp:206-214);
        returns (iterations executed, terminated, weight-update rounds)"""
        term, rounds = C.c_int(0), C.c_int(0)
        done = _chk(lib().dpgo_team_run_schedule(self.h, int(max_iters), C.byref(term), C.byref(rounds)), "run_schedule")
        return done, bool(term.value), rounds.value

    def set_iteration_log(self, directory):
        """one CSV per local robot in the reference's column order + global_cost (include/dpgo_hip.h); None closes"""
        _chk(lib().dpgo_team_set_iteration_log(self.h, str(directory).encode() if directory is not None else None), "set_iteration_log")

    def run_simultaneous(self, ticks):
        """every agent takes `ticks` RGD steps, all agents per tick in the same launches (ASAPP, clocks in lockstep)"""
        _chk(lib().dpgo_team_run_simultaneous(self.h, ticks), "run_simultaneous")

    def run_colored(self, sweeps):
        _chk(lib().dpgo_team_run_colored(self.h, sweeps), "run_colored")

    def set_groups(self, groups):
        ptr = np.cumsum([0] + [len(g) for g in groups]).astype(np.int32)
        mem = np.array([a for g in groups for a in g], dtype=np.int32)
        _chk(lib().dpgo_team_set_groups(self.h, len(groups), _d(ptr), _d(mem)), "set_groups")

    def run_group(self, g, count):
        _chk(lib().dpgo_team_run_group(self.h, g, count), "run_group")

    def step_begin(self, sel_id):
        _chk(lib().dpgo_team_step_begin(self.h, sel_id), "step_begin")

    def step_end(self, sel_id):
        _chk(lib().dpgo_team_step_end(self.h, sel_id), "step_end")

    def synchronize(self):
        _chk(lib().dpgo_team_synchronize(self.h), "synchronize")

    def iteration(self):
        return lib().dpgo_team_iteration(self.h)

    def cost(self):
        f = C.c_double()
        _chk(lib().dpgo_team_cost(self.h, C.byref(f)), "team_cost")
        return f.value

    def update_weights(self):
        return _chk(lib().dpgo_team_update_weights(self.h), "team_update_weights")

    def counters(self):
        out = np.zeros(11)
        lib().dpgo_team_get_counters(self.h, _d(out), 11)
        return out

    def stream(self):
        return lib().dpgo_team_stream(self.h)

    def time_kernel(self, agent_id, which, reps=200):
        ms, nbytes = C.c_double(), C.c_double()
        _chk(lib().dpgo_team_time_kernel(self.h, agent_id, which, reps, C.byref(ms), C.byref(nbytes)), "time_kernel")
        return ms.value, nbytes.value

    def global_X(self):
        return np.concatenate([self.agents[i].get_X() for i in self.ids])

    def certificate_apply(self, V, transport=None, owner_of_robot=None):
        """S(X) V for a K x 4N block (K in 3..8) in the iterate layout over the team's poses in team order:
        element (b, column 4 g + c) at [(4 g + c) K + b].  With a transport (and the owner table: the participant that
        holds each robot), the team holds part of the robots and V / the result its own columns; every participant calls."""
        N = int(sum(self.agents[i].n for i in self.ids))
        V = np.ascontiguousarray(V, dtype=np.float64).reshape(-1)
        K = V.size // (4 * N)
        assert V.size == K * 4 * N
        out = np.zeros_like(V)
        if transport is None:
            _chk(lib().dpgo_team_certificate_apply(self.h, int(K), _d(V), _d(out)), "certificate_apply")
        else:
            own = _owner_array(owner_of_robot)
            _chk(lib().dpgo_team_certificate_apply_across(self.h, C.byref(transport.struct), _d(own), int(K), _d(V), _d(out)),
                 "certificate_apply_across")
        return out

    def certificate_precondition(self, V):
        """T V for a K x 4N block (K in 3..8) in the layout of certificate_apply: the certificate eigensolver's block-Jacobi
        preconditioner (Q_a + shift I)^-1 by agent (dense inverses or 4 x 4 diagonal inverses), for tests"""
        N = int(sum(self.agents[i].n for i in self.ids))
        V = np.ascontiguousarray(V, dtype=np.float64).reshape(-1)
        K = V.size // (4 * N)
        assert V.size == K * 4 * N
        out = np.zeros_like(V)
        _chk(lib().dpgo_team_certificate_precondition(self.h, int(K), _d(V), _d(out)), "certificate_precondition")
        return out

    def certify(self, eta=1e-6, tol=1e-8, max_iters=1000, block=0, deflate=True, precondition=True, eta_relative=True,
                transport=None, owner_of_robot=None):
        """smallest eigenvalue of the certificate matrix S(X) at the current iterate (LOBPCG on the device).  Returns
        (Certificate, v): certified 1 = converged with lambda_min >= -eta, 0 = lambda_min < -eta (v, 4N doubles in team
        order, is a direction of negative curvature), -1 = not converged.  eta is relative to the bound s on |S| unless
        eta_relative is False; tol always is.  Changes no solver state.  With a transport: the certificate of the iterate
        split across the participants' teams (every participant calls; v holds this team's columns)."""
        N = int(sum(self.agents[i].n for i in self.ids))
        flags = (0 if deflate else CERT_NO_DEFLATION) | (0 if precondition else CERT_NO_PRECONDITIONER) | \
            (CERT_ETA_RELATIVE if eta_relative else 0)
        res, v = Certificate(), np.zeros(4 * N)
        if transport is None:
            _chk(lib().dpgo_team_certify(self.h, C.c_double(eta), C.c_double(tol), int(max_iters), int(block), flags,
                                         C.byref(res), _d(v)), "certify")
        else:
            own = _owner_array(owner_of_robot)
            _chk(lib().dpgo_team_certify_across(self.h, C.byref(transport.struct), _d(own), C.c_double(eta), C.c_double(tol),
                                                int(max_iters), int(block), flags, C.byref(res), _d(v)), "certify_across")
        return res, v

    def round(self, refine_translations=True, transport=None, owner_of_robot=None):
        """SE-Sync rounding of the current iterate: (Rounding, T) with T flat, 12 doubles per pose in team order (the layout
        of chordal_init), anchored at the first pose.  refine_translations: the translations re-solved for the rounded
        rotations with the team's measurements and current weights.  Changes no solver state.  With a transport: the
        rounding of the iterate split across the participants' teams, anchored at robot 0's first pose (T: this team's poses)."""
        N = int(sum(self.agents[i].n for i in self.ids))
        res, T = Rounding(), np.zeros(12 * N)
        flags = ROUND_REFINE_TRANSLATIONS if refine_translations else 0
        if transport is None:
            _chk(lib().dpgo_team_round(self.h, flags, _d(T), C.byref(res)), "round")
        else:
            own = _owner_array(owner_of_robot)
            _chk(lib().dpgo_team_round_across(self.h, C.byref(transport.struct), _d(own), flags, _d(T), C.byref(res)),
                 "round_across")
        return res, T

    def covariance_plan(self, max_block=None):
        """the sets of covariances(method="nested") for this team: (block_of[N] in team order with the block index, -1 = separator
        pose, -2 = pose 0; info dict as capi.covariance_nested_plan).  max_block None: the library's default"""
        N = int(sum(self.agents[i].n for i in self.ids))
        block_of, info = np.zeros(N, dtype=np.int32), np.zeros(6, dtype=np.int32)
        _chk(lib().dpgo_team_covariance_nested_plan(self.h, int(max_block or 0), _d(block_of), _d(info)), "covariance_nested_plan")
        return block_of, _nested_plan_info(info)

    def covariances(self, T=None, pairs=None, method=None, transport=None, owner_of_robot=None):
        """Marginal pose covariances at the trajectory T (12 doubles per pose in team order; None: the rounding of the
        current iterate, self.round()): (Covariance, diag[N, 6, 6], cross[len(pairs), 6, 6]).  Pose i is perturbed by
        (phi, delta), rotation first: R_i <- R_i Exp(phi) (body frame), t_i <- t_i + delta (world frame); pose 0 is held
        fixed (its blocks are zero).  The blocks are those of the inverse of the cost's Hessian at the measurements' current
        weights; cross[k] is the block of the pose pair pairs[k] = (a, b).  method: "dense" (the default of one team) inverts
        the whole reduced Hessian, "schur" eliminates the poses without shared edges robot by robot and inverts only the Schur
        complement on the public poses -- the same blocks to round-off, in a fraction of the memory and time when the robots
        share few poses.  "nested" (one team only; covariances_nested takes its block size) goes one step further: a robot
        whose interior holds more poses than the block size has it dissected into blocks, and the dissection's separator poses
        join the public ones -- what a single robot, or a few robots with large interiors, need.  Raises DpgoError when T is not in SE(3), the weighted graph is disconnected, the matrices do not fit
        the device, or T is not a minimum (a non-positive pivot).  Changes no solver state.
        With a transport (a team split across participants, owner_of_robot as for certify / round): the Schur path is the
        only method ("dense" raises ValueError; the default means "schur").  T and diag are this team's poses in team order,
        pairs name poses of the whole problem (robots by id, then poses; pose 0 is robot 0's first pose), the same list on
        every participant, and cross is complete on every participant; the scalars are identical everywhere."""
        if method not in (None, "dense", "schur", "nested"):
            raise ValueError("covariances: method must be \"dense\", \"schur\" or \"nested\", not %r" % (method,))
        if method == "nested" and transport is not None:
            raise ValueError("covariances: method=\"nested\" has no call across teams (it was given a transport)")
        if method == "nested":
            return self.covariances_nested(T, pairs)
        if transport is not None and method == "dense":
            raise ValueError("covariances: a team split across participants has no dense path (method=\"dense\" with a "
                             "transport)")
        if method is None:
            method = "dense" if transport is None else "schur"
        N = int(sum(self.agents[i].n for i in self.ids))
        if T is None:
            T = (self.round() if transport is None else self.round(transport=transport, owner_of_robot=owner_of_robot))[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("covariances: T holds %d doubles, the team's %d poses need %d" % (T.size, N, 12 * N))
        pr = np.ascontiguousarray(np.zeros((0, 2)) if pairs is None else pairs, dtype=np.int32).reshape(-1, 2)
        res, diag, cross = Covariance(), np.zeros((N, 6, 6)), np.zeros((len(pr), 6, 6))
        flags = COV_SCHUR if method == "schur" else 0
        if transport is None:
            _chk(lib().dpgo_team_marginal_covariances(self.h, _d(T), flags, len(pr), _d(pr) if len(pr) else None, _d(diag),
                                                      _d(cross) if len(pr) else None, C.byref(res)), "marginal_covariances")
        else:
            own = _owner_array(owner_of_robot)
            _chk(lib().dpgo_team_marginal_covariances_across(self.h, C.byref(transport.struct), _d(own), _d(T), flags, len(pr),
                                                             _d(pr) if len(pr) else None, _d(diag),
                                                             _d(cross) if len(pr) else None, C.byref(res)),
                 "marginal_covariances_across")
        return res, diag, cross

    def covariances_nested(self, T=None, pairs=None, max_block=None):
        """covariances(method="nested") with its parameter: max_block, the largest block in poses that a robot's interior is
        left whole at or dissected into (None: the library's default, COV_NESTED_DEFAULT_BLOCK).  The same return value,
        conventions and errors as covariances; when no robot's interior exceeds max_block the call is method="schur", bit for bit."""
        N = int(sum(self.agents[i].n for i in self.ids))
        if T is None:
            T = self.round()[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("covariances: T holds %d doubles, the team's %d poses need %d" % (T.size, N, 12 * N))
        pr = np.ascontiguousarray(np.zeros((0, 2)) if pairs is None else pairs, dtype=np.int32).reshape(-1, 2)
        res, diag, cross = Covariance(), np.zeros((N, 6, 6)), np.zeros((len(pr), 6, 6))
        _chk(lib().dpgo_team_marginal_covariances_nested(self.h, _d(T), int(max_block or 0), len(pr), _d(pr) if len(pr) else None,
                                                         _d(diag), _d(cross) if len(pr) else None, C.byref(res)),
             "marginal_covariances_nested")
        return res, diag, cross

    def covariance_apply(self, V, T=None, method=None, max_block=None, transport=None, owner_of_robot=None):
        """X = Sigma V, the estimate's covariance applied to vectors: the solve H_red X_red = V_red on the factors
        of a covariance path, without a block of Sigma.  V: [6 N, m] (or [6 N]: one column); rows 6 p .. 6 p + 5 belong to team
        pose p in the perturbation of covariances (rotation first, body frame; translation, world frame; pose 0 fixed).  Sigma
        is the full covariance whose rows and columns of pose 0 are zero: pose 0's rows of V are not read, those of X are zero.
        T as in covariances (None: the rounding of the current iterate).  method: "dense" (the default) multiplies by the
        explicit inverse; "nested" eliminates on covariance_plan(max_block)'s sets, split or not; "schur" raises DpgoError
        ("nested" with no robot split has its sets).  Returns (Covariance, X[6 N, m]).  Two calls give the same bytes.  Raises
        DpgoError as covariances does, for a V that is not finite, and for V and X that do not fit the device.  Changes no
        solver state.
        With a transport (a team split across participants, owner_of_robot as for covariances): the Schur path is the only
        one (method None or "schur"; anything else, or a max_block, raises ValueError before any transport call).  T, V and
        X are this team's poses in team order, V [6 N_loc, m] with the same m on every participant; the fixed pose is the
        problem's pose 0, robot 0's first, whose rows are not read and come back zero on the participant that holds it.  T
        None: the rounding across.  Returns (Covariance, X_local); every row is the same bits whatever the split, and the
        scalars are identical on every participant.  A ValueError (V's shape, T's size) is raised on this participant alone
        before the library is called, as in the other calls across teams: the others wait in the agreement record until their
        transport times out, so check shapes before a collective call."""
        if method not in (None, "dense", "schur", "nested"):
            raise ValueError("covariance_apply: method must be \"dense\", \"schur\" or \"nested\", not %r" % (method,))
        N = int(sum(self.agents[i].n for i in self.ids))
        if transport is not None:
            T = self._across_args("covariance_apply", T, method, max_block, transport, owner_of_robot)
        elif T is None:
            T = self.round()[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("covariance_apply: T holds %d doubles, the team's %d poses need %d" % (T.size, N, 12 * N))
        V = np.asarray(V, dtype=np.float64)
        if V.ndim == 1:
            V = V.reshape(-1, 1)
        if V.ndim != 2 or V.shape[0] != 6 * N or V.shape[1] < 1:
            raise ValueError("covariance_apply: V has shape %r, the team's %d poses need [%d, m] with m >= 1" % (V.shape, N, 6 * N))
        Vf = np.asfortranarray(V)
        X = np.zeros(Vf.shape, order="F")
        res = Covariance()
        if transport is not None:
            own = _owner_array(owner_of_robot)
            _chk(lib().dpgo_team_covariance_apply_across(self.h, C.byref(transport.struct), _d(own), _d(T), Vf.shape[1], _d(Vf),
                                                         _d(X), C.byref(res)), "covariance_apply_across")
            return res, X
        code = {None: GATE_DENSE, "dense": GATE_DENSE, "schur": GATE_SCHUR, "nested": GATE_NESTED}[method]
        _chk(lib().dpgo_team_covariance_apply(self.h, _d(T), code, int(max_block or 0), Vf.shape[1], _d(Vf), _d(X), C.byref(res)),
             "covariance_apply")
        return res, X

    def refine(self, T=None, method=None, max_block=None, max_iters=10, grad_tol=1e-8, armijo=1e-4, ladder=8, transport=None,
               owner_of_robot=None):
        """T refined to a critical point of the SE(3) cost by Newton steps on Sigma: what covariances, the gates,
        audit, select_closures, linear_update, linear_removal and covariance_apply assume of their T.  Every iteration forms the
        gradient of g(xi) = f(T [+] xi) (the perturbation of covariances, pose 0 fixed), the cost and |g|_inf on the device,
        stops at |g|_inf <= grad_tol, else takes X = Sigma g from one covariance path (method "dense", the default, or "nested"
        with max_block; "schur" raises DpgoError as in covariance_apply) and the first step length 2^-l, l < ladder, with
        f_l <= f - armijo 2^-l g^T X up to the rounding of the cost's sum.  T as in covariances (None: the rounding of the
        current iterate).  A polisher, not a solver: a T at which the Hessian is not positive definite raises DpgoError with the
        path's message ("not a minimum"); there is no Levenberg shift.  Returns dict(T, status: "converged" | "max_iters" |
        "indefinite" (a later iterate lost positive definiteness: T is the last good one) | "no_descent" (no step length
        passed), iterations, f0, f, grad_inf0, grad_inf, history=dict(f, grad_inf: iterations + 1 entries; alpha, decrement =
        g^T Sigma g, pivot_min: one entry per path that ran, alpha NaN where no step was taken), covariance: the last path's
        record).  A T that meets grad_tol comes back bit for bit with iterations 0.  Two calls give the same bytes.  Changes no
        solver state.
        With a transport (a team split across participants, owner_of_robot as for covariances; DESIGN.md 5n "Across teams"):
        the Schur path across is the only one (method None or "schur"; anything else, or a max_block, raises ValueError before
        any transport call).  T is this team's poses in team order (None: the rounding across) and so is the T returned; the
        fixed pose is the problem's pose 0, robot 0's first.  max_iters, grad_tol, armijo and ladder must be the same on every
        participant.  The cost and g^T X are summed robot by robot and the robots' totals in id order, so every pose, the
        history and the scalars are the same bits whatever the split, and identical on every participant; they are not bitwise
        the single team's.  A ValueError (T's size) is raised on this participant alone before the library is called: check
        shapes before a collective call."""
        if method not in (None, "dense", "schur", "nested"):
            raise ValueError("refine: method must be \"dense\", \"schur\" or \"nested\", not %r" % (method,))
        N = int(sum(self.agents[i].n for i in self.ids))
        if transport is not None:
            T = self._across_args("refine", T, method, max_block, transport, owner_of_robot)
        elif T is None:
            T = self.round()[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("refine: T holds %d doubles, the team's %d poses need %d" % (T.size, N, 12 * N))
        code = {None: GATE_DENSE, "dense": GATE_DENSE, "schur": GATE_SCHUR, "nested": GATE_NESTED}[method]
        rows = max(int(max_iters), 0) + 1
        T_out, hist, out, res = np.zeros(12 * N), np.zeros((rows, 5)), Refine(), Covariance()
        if transport is not None:
            own = _owner_array(owner_of_robot)
            _chk(lib().dpgo_team_refine_across(self.h, C.byref(transport.struct), _d(own), _d(T), int(max_iters),
                                               C.c_double(grad_tol), C.c_double(armijo), int(ladder), _d(T_out), _d(hist),
                                               C.byref(out), C.byref(res)), "refine_across")
        else:
            _chk(lib().dpgo_team_refine(self.h, _d(T), code, int(max_block or 0), int(max_iters), C.c_double(grad_tol),
                                        C.c_double(armijo), int(ladder), _d(T_out), _d(hist), C.byref(out), C.byref(res)),
                 "refine")
        k = out.iterations
        ran = int(np.count_nonzero(~np.isnan(hist[:, 3])))
        return dict(T=T_out, status=REFINE_STATUS[out.status], iterations=k, f0=out.f0, f=out.f, grad_inf0=out.grad_inf0,
                    grad_inf=out.grad_inf,
                    history=dict(f=hist[:k + 1, 0].copy(), grad_inf=hist[:k + 1, 1].copy(), alpha=hist[:ran, 2].copy(),
                                 decrement=hist[:ran, 3].copy(), pivot_min=hist[:ran, 4].copy()),
                    covariance=res)

    @staticmethod
    def _across_check(what, method, max_block):
        """the arguments a per-record call cannot take with a transport: ValueError before any transport call"""
        if method not in (None, "schur"):
            raise ValueError("%s: a team split across participants has the Schur path alone (method=%r with a transport)"
                             % (what, method))
        if max_block is not None:
            raise ValueError("%s: max_block belongs to method=\"nested\", which has no call across teams (it was given a "
                             "transport)" % what)

    def _across_args(self, what, T, method, max_block, transport, owner_of_robot):
        """those checks, and the call's T (None: the rounding across)"""
        self._across_check(what, method, max_block)
        if T is None:
            T = self.round(transport=transport, owner_of_robot=owner_of_robot)[1]
        return T

    def _gate_call(self, what, cand, T, method, max_block, want_innovation, want_sigma, transport=None, owner_of_robot=None):
        if method not in (None, "dense", "schur", "nested"):
            raise ValueError("%s: method must be \"dense\", \"schur\" or \"nested\", not %r" % (what, method))
        N = int(sum(self.agents[i].n for i in self.ids))
        if transport is not None:
            T = self._across_args(what, T, method, max_block, transport, owner_of_robot)
        elif T is None:
            T = self.round()[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("%s: T holds %d doubles, the team's %d poses need %d" % (what, T.size, N, 12 * N))
        cand = np.ascontiguousarray(cand, dtype=MEAS_DTYPE).reshape(-1)
        K = len(cand)
        res = Covariance()
        xi, d2 = (np.zeros((K, 6)), np.zeros(K)) if want_innovation else (None, None)
        sg = np.zeros((K, 6, 6)) if want_sigma else None
        outs = (_d(xi) if want_innovation and K else None, _d(d2) if want_innovation and K else None,
                _d(sg) if want_sigma and K else None)
        if transport is not None:
            own = _owner_array(owner_of_robot)
            _chk(lib().dpgo_team_gate_candidates_across(self.h, C.byref(transport.struct), _d(own), _d(T), K, _d(cand), *outs,
                                                        C.byref(res)), "gate_candidates_across")
            return res, xi, d2, sg
        code = {None: GATE_DENSE, "dense": GATE_DENSE, "schur": GATE_SCHUR, "nested": GATE_NESTED}[method]
        _chk(lib().dpgo_team_gate_candidates(self.h, _d(T), code, int(max_block or 0), K, _d(cand), *outs, C.byref(res)),
             "gate_candidates")
        return res, xi, d2, sg

    def gate(self, candidates, T=None, method=None, max_block=None, quantile=0.99, sigma_rel=False, transport=None,
             owner_of_robot=None):
        """Candidate measurements tested against the estimate's own uncertainty.  candidates: MEAS_DTYPE
        records (r1, p1) -> (r2, p2) with R (row-major), t, kappa, tau, T_j ~ T_i (R, t); weight and the flags are ignored: a
        candidate is a fresh measurement that is not in the graph.  T and method as in covariances (T None: the rounding of
        the current iterate; method None: "dense"); max_block: method="nested" only.  Returns (Covariance, xi[K, 6], d2[K],
        accept[K]) and, with sigma_rel=True, sigma_rel[K, 6, 6] behind them.  xi = (Log(R~^T R_ij), t_ij - t~) is the
        innovation, rotation first; sigma_rel the covariance of the relative pose (R_ij, t_ij) = T_i^-1 T_j under the
        perturbation R_ij <- R_ij Exp(phi), t_ij <- t_ij + delta (delta in frame i); d2 = xi^T (sigma_rel + Sigma_meas)^-1 xi
        with Sigma_meas = diag(I / (2 kappa), I / tau), the cost's own noise model; accept = sqrt(d2) <=
        error_threshold_at_quantile(quantile, 6).  The covariance blocks never leave the device: one kernel behind the
        covariance path forms the outputs.  Raises DpgoError as covariances does, and for a candidate that names a robot or pose
        outside the team, joins a pose to itself, has kappa <= 0 or tau <= 0, or an R outside SO(3).  Changes no solver state.
        With a transport (a team split across participants, owner_of_robot as for covariances): the candidates, the same list
        on every participant, may name any robot of the problem -- a closure between a robot held here and one held elsewhere
        is the normal case; T is this team's poses (None: the rounding across); method None or "schur" (anything else and a
        max_block raise ValueError).  The results are complete and identical on every participant, bit for bit those of the
        single team's method="schur"."""
        res, xi, d2, sg = self._gate_call("gate", candidates, T, method, max_block, True, bool(sigma_rel), transport, owner_of_robot)
        accept = np.sqrt(d2) <= error_threshold_at_quantile(quantile, 6)
        return (res, xi, d2, accept, sg) if sigma_rel else (res, xi, d2, accept)

    def relative_covariances(self, pairs, T=None, method=None, max_block=None, transport=None, owner_of_robot=None):
        """sigma_rel[K, 6, 6] of gate for the pose pairs[k] = (i, j), team-order pose indices with i != j: the covariance of
        the relative pose T_i^-1 T_j.  No measurement is involved; the same bits as gate(..., sigma_rel=True) gives.  With a
        transport (as in gate): pairs are global pose ids (robots by id, then poses), the same list on every participant."""
        pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        if transport is not None:
            return self._relative_across(pr, T, method, max_block, transport, owner_of_robot)
        offs = np.cumsum([0] + [self.agents[i].n for i in self.ids])
        N = int(offs[-1])
        if len(pr) and (pr.min() < 0 or pr.max() >= N):
            raise ValueError("relative_covariances: a pair names a pose outside [0, %d)" % N)
        cand = np.zeros(len(pr), dtype=MEAS_DTYPE)
        ids = np.asarray(self.ids, dtype=np.int64)
        for e, (r, p) in enumerate((("r1", "p1"), ("r2", "p2"))):
            k = np.searchsorted(offs, pr[:, e], side="right") - 1
            cand[r], cand[p] = ids[k], pr[:, e] - offs[k]
        return self._gate_call("relative_covariances", cand, T, method, max_block, False, True)[3]

    def _relative_across(self, pr, T, method, max_block, transport, owner_of_robot):
        self._across_check("relative_covariances", method, max_block)
        # the robots' sizes from every participant (one allgather of num_robots doubles), then (robot, pose) of every global id
        own = _owner_array(owner_of_robot)
        mine = np.zeros(len(own))
        for i in self.ids:
            mine[i] = self.agents[i].n
        sizes = np.asarray(transport.allgather(mine)).reshape(transport.world, len(own))
        n_of = np.array([int(sizes[int(own[i]), i]) for i in range(len(own))], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(n_of)])
        if len(pr) and (pr.min() < 0 or pr.max() >= offs[-1]):
            raise ValueError("relative_covariances: a pair names a pose outside [0, %d)" % offs[-1])
        cand = np.zeros(len(pr), dtype=MEAS_DTYPE)
        for e, (r, p) in enumerate((("r1", "p1"), ("r2", "p2"))):
            k = np.searchsorted(offs, pr[:, e], side="right") - 1
            cand[r], cand[p] = k, pr[:, e] - offs[k]
        return self._gate_call("relative_covariances", cand, T, method, max_block, False, True, transport, owner_of_robot)[3]

    def _joined_records(self, recs, transport, owner_of_robot):
        """the participants' record lists allgathered (lengths first, then the lists padded to the longest) and joined by
        join_records_by_robot: the same global list on every participant"""
        x = records_to_doubles(recs)
        lens = np.asarray(transport.allgather(np.array([float(len(x))]))).reshape(-1).astype(int)
        L = int(lens.max()) if len(lens) else 0
        mine = np.zeros(max(L, 1) * _REC_DOUBLES)
        mine[:x.size] = x.reshape(-1)
        allr = np.asarray(transport.allgather(mine)).reshape(transport.world, -1)
        lists = [records_from_doubles(allr[q, :lens[q] * _REC_DOUBLES]) for q in range(transport.world)]
        return join_records_by_robot(lists, owner_of_robot)

    def zero_weight_measurements(self, transport=None, owner_of_robot=None):
        """the team's measurements whose current weight is 0 (what GNC-TLS has rejected, or set_measurement_weight), in the
        form gate accepts; each shared edge once, as the lower robot's copy (the rule of round's translation refinement).
        With a transport: those of the whole problem, the same list on every participant (join_records_by_robot)"""
        if transport is not None:
            return self._joined_records(self.zero_weight_measurements(), transport, owner_of_robot)
        out = [e for i in self.ids for e in self.agents[i].measurements()
               if e["weight"] == 0.0 and (e["r1"] == e["r2"] or min(int(e["r1"]), int(e["r2"])) == i)]
        return np.array(out, dtype=MEAS_DTYPE) if out else np.zeros(0, dtype=MEAS_DTYPE)

    def measurements_once(self):
        """all of the team's measurements with their current weights, in the form audit accepts; each shared edge once, as the
        lower robot's copy (the rule of zero_weight_measurements)"""
        out = [e for i in self.ids for e in self.agents[i].measurements()
               if e["r1"] == e["r2"] or min(int(e["r1"]), int(e["r2"])) == i]
        return np.array(out, dtype=MEAS_DTYPE) if out else np.zeros(0, dtype=MEAS_DTYPE)

    def audit(self, measurements=None, T=None, method=None, max_block=None, quantile=0.99, min_redundancy=1e-6, sigma_loo=False,
              transport=None, owner_of_robot=None):
        """Measurements that are in the graph tested against the rest of it: leave-one-out gating.
        measurements: MEAS_DTYPE records as in gate, whose weight w >= 0 says at which weight each is in the graph (w = 0: not in
        the Hessian); the flags are ignored and the records are taken on trust.  None: measurements_once(), the team's own
        with their current weights.  T, method and max_block as in gate.  Returns a dict:
            measurements  the records audited,
            xi[K, 6]      the innovation of gate,
            xi_loo[K, 6]  the innovation the edge would have shown had it been left out of the graph,
            d2[K]         to first order in the residuals the d2 gate would return for the edge had it been taken out, the
                          graph solved again and the edge offered as a candidate; +inf where the record is not testable,
            redundancy[K] rho = 1 - w tr(C) / 6 in [0, 1] with C the relative covariance whitened by the edge's own noise,
            pivot_min[K]  the smallest Cholesky pivot of A = I - w C; the error of d2 grows like its reciprocal,
            testable[K]   pivot_min > min_redundancy: the graph knows the relative pose by other ways than this edge,
            accept[K]     testable and sqrt(d2) <= error_threshold_at_quantile(quantile, 6),
            covariance    the Covariance record of the path,
            sigma_loo[K, 6, 6]  with sigma_loo=True: the relative covariance of the graph without the edge (zero where the
                          record is not testable).
        At w = 0 this is gate; at w = 1 the normalised-residual test.  Raises DpgoError as gate does, and for a weight that is
        negative or not finite or a min_redundancy outside (0, 1).  Changes no solver state.
        With a transport (as in gate): the records, the same list on every participant, may name any robot of the problem;
        None: every participant's measurements_once() allgathered and joined in robot order (join_records_by_robot), which is
        the single team's measurements_once().  The results are complete and identical on every participant, bit for bit
        those of the single team's method="schur"."""
        if method not in (None, "dense", "schur", "nested"):
            raise ValueError("audit: method must be \"dense\", \"schur\" or \"nested\", not %r" % (method,))
        N = int(sum(self.agents[i].n for i in self.ids))
        if transport is not None:
            T = self._across_args("audit", T, method, max_block, transport, owner_of_robot)
        elif T is None:
            T = self.round()[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("audit: T holds %d doubles, the team's %d poses need %d" % (T.size, N, 12 * N))
        if measurements is not None:
            meas = measurements
        elif transport is not None:
            meas = self._joined_records(self.measurements_once(), transport, owner_of_robot)
        else:
            meas = self.measurements_once()
        meas = np.ascontiguousarray(meas, dtype=MEAS_DTYPE).reshape(-1)
        K = len(meas)
        res = Covariance()
        xi, xl, d2, rho, pm = np.zeros((K, 6)), np.zeros((K, 6)), np.zeros(K), np.zeros(K), np.zeros(K)
        sg = np.zeros((K, 6, 6)) if sigma_loo else None
        code = {None: GATE_DENSE, "dense": GATE_DENSE, "schur": GATE_SCHUR, "nested": GATE_NESTED}[method]
        p = lambda a: _d(a) if K else None
        if transport is not None:
            own = _owner_array(owner_of_robot)
            _chk(lib().dpgo_team_audit_measurements_across(self.h, C.byref(transport.struct), _d(own), _d(T), K, p(meas),
                                                           C.c_double(min_redundancy), p(xi), p(xl), p(d2), p(rho), p(pm),
                                                           p(sg) if sigma_loo else None, C.byref(res)), "audit_measurements_across")
        else:
            _chk(lib().dpgo_team_audit_measurements(self.h, _d(T), code, int(max_block or 0), K, p(meas), C.c_double(min_redundancy),
                                                    p(xi), p(xl), p(d2), p(rho), p(pm), p(sg) if sigma_loo else None, C.byref(res)),
                 "audit_measurements")
        testable = pm > min_redundancy
        out = dict(measurements=meas, xi=xi, xi_loo=xl, d2=d2, redundancy=rho, pivot_min=pm, testable=testable,
                   accept=testable & (np.sqrt(d2) <= error_threshold_at_quantile(quantile, 6)), covariance=res)
        if sigma_loo:
            out["sigma_loo"] = sg
        return out

    def gate_jointly(self, candidates, T=None, method=None, max_block=None, quantile=0.99, order="greedy", innovation_covariance=False):
        """A set of candidate measurements gated jointly, each given those already accepted.  candidates, T,
        method and max_block as in gate, which tests every candidate against the covariance of the estimate before any of them
        is taken; here M = A Sigma A^T + R is the joint covariance of all K innovations (A: the gate's Jacobians J_i, J_j of
        every candidate in its row block, R: the block diagonal of the Sigma_meas), and candidate k is tested by its innovation
        and covariance conditioned on the accepted set A: xi_k|A = xi_k - M_kA M_AA^-1 xi_A, S_k|A = M_kk - M_kA M_AA^-1 M_Ak,
        d2_k|A = xi_k|A^T S_k|A^-1 xi_k|A -- to first order what gate would show for k once the candidates of A had been added
        to the graph and the estimate updated.  order="greedy": at every step the remaining candidate of smallest d2_k|A (the
        lower index on ties) is accepted if d2 <= error_threshold_at_quantile(quantile, 6)^2, else the call stops and all that
        is left is rejected; order="given": k = 0 .. K - 1 in turn, accepted on the same test or skipped.  Returns a dict:
            candidates     the records gated,
            xi[K, 6], d2[K]  the marginal innovation and distance: gate's,
            xi_cond[K, 6], d2_cond[K]  the conditional values at the moment k was decided (for what the greedy rule rejects at
                           its stop: given the final set),
            accept[K]      bool,
            rank[K]        the position in the order of acceptance, -1 when rejected,
            accepted       the indices of the accepted candidates in the order of acceptance,
            num_accepted, d2_joint (the sum of d2_cond over the accepted set = xi_A^T M_AA^-1 xi_A), logdet_joint (log det M_AA),
            joint_accept   sqrt(d2_joint) <= error_threshold_at_quantile(quantile, 6 num_accepted),
            covariance     the Covariance record of the path,
            M[6 K, 6 K]    with innovation_covariance=True: the joint innovation covariance, bitwise symmetric.
        The covariance blocks, M and the factor stay on the device.  Raises DpgoError as gate does, and for a quantile outside
        (0, 1) or a batch whose blocks, M and factor do not fit the device.  One team only.  Changes no solver state."""
        if method not in (None, "dense", "schur", "nested"):
            raise ValueError("gate_jointly: method must be \"dense\", \"schur\" or \"nested\", not %r" % (method,))
        if order not in ("greedy", "given"):
            raise ValueError("gate_jointly: order must be \"greedy\" or \"given\", not %r" % (order,))
        N = int(sum(self.agents[i].n for i in self.ids))
        if T is None:
            T = self.round()[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("gate_jointly: T holds %d doubles, the team's %d poses need %d" % (T.size, N, 12 * N))
        cand = np.ascontiguousarray(candidates, dtype=MEAS_DTYPE).reshape(-1)
        K = len(cand)
        res = Covariance()
        xi, d2, xc, dc = np.zeros((K, 6)), np.zeros(K), np.zeros((K, 6)), np.zeros(K)
        accept, rank = np.zeros(K, dtype=np.int32), np.full(K, -1, dtype=np.int32)
        nacc, dj, lj = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        M = np.zeros((6 * K, 6 * K)) if innovation_covariance else None
        code = {None: GATE_DENSE, "dense": GATE_DENSE, "schur": GATE_SCHUR, "nested": GATE_NESTED}[method]
        p = lambda a: _d(a) if K else None
        _chk(lib().dpgo_team_gate_candidates_jointly(self.h, _d(T), code, int(max_block or 0), K, p(cand),
                                                     JOINT_GREEDY if order == "greedy" else JOINT_GIVEN, C.c_double(quantile),
                                                     p(xi), p(d2), p(xc), p(dc), p(accept), p(rank), C.byref(nacc), C.byref(dj),
                                                     C.byref(lj), p(M) if innovation_covariance else None, C.byref(res)),
             "gate_candidates_jointly")
        n = int(nacc.value)
        accepted = np.argsort(np.where(rank >= 0, rank, K), kind="stable")[:n]
        out = dict(candidates=cand, xi=xi, d2=d2, xi_cond=xc, d2_cond=dc, accept=accept != 0, rank=rank, accepted=accepted,
                   num_accepted=n, d2_joint=float(dj.value), logdet_joint=float(lj.value),
                   joint_accept=bool(n == 0 or np.sqrt(dj.value) <= error_threshold_at_quantile(quantile, 6 * n)), covariance=res)
        if innovation_covariance:
            out["M"] = M
        return out

    def candidates_from_pairs(self, pairs, kappa, tau):
        """MEAS_DTYPE records for the team-order pose pairs[k] = (i, j), i != j, with no measurement: R = I, t = 0, the expected
        noise kappa and tau (scalars or one per pair) and weight 1 -- what select_closures takes for a pool of proposals.  Robots
        and poses are resolved as relative_covariances resolves them."""
        pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        offs = np.cumsum([0] + [self.agents[i].n for i in self.ids])
        N = int(offs[-1])
        if len(pr) and (pr.min() < 0 or pr.max() >= N):
            raise ValueError("candidates_from_pairs: a pair names a pose outside [0, %d)" % N)
        cand = np.zeros(len(pr), dtype=MEAS_DTYPE)
        ids = np.asarray(self.ids, dtype=np.int64)
        for e, (r, p) in enumerate((("r1", "p1"), ("r2", "p2"))):
            k = np.searchsorted(offs, pr[:, e], side="right") - 1
            cand[r], cand[p] = ids[k], pr[:, e] - offs[k]
        cand["R"] = np.eye(3).reshape(-1)
        cand["kappa"], cand["tau"], cand["weight"] = kappa, tau, 1.0
        return cand

    def select_closures(self, candidates, budget, T=None, method=None, max_block=None, order="greedy", min_gain=None):
        """The most informative of a pool of candidate closures under a budget, chosen before any of them is measured (DESIGN.md
        5k).  candidates: MEAS_DTYPE records of which only the endpoints, kappa and tau are read (candidates_from_pairs builds
        them); T, method and max_block as in gate_jointly, whose M = A Sigma A^T + R this call eliminates without forming it.
        Given the selected set A, gain_k|A = (log det S_k|A - log det Sigma_meas,k) / 2 with S_k|A = M_kk - M_kA M_AA^-1 M_Ak is
        the mutual information between measurement k and the trajectory once A has been measured.  order="greedy": at every
        step the open candidate of largest gain_k|A (the lower index on ties); order="given": k = 0 .. budget - 1 in turn, the
        price of a caller's own plan.  A candidate is taken while its gain exceeds min_gain (None: no threshold) and fewer
        than `budget` are selected; otherwise the call stops.  Returns a dict:
            candidates     the records,
            gain[P]        the marginal gain_k|{},
            gain_cond[P]   the gain at the moment k was selected; for the rest, given the final set: what is still on the table,
            rank[P]        the position in the order of selection, -1 when not selected,
            selected       the indices of the selected candidates in selection order,
            num_selected, gain_total (the sum of gain_cond over `selected` in order = (log det M_AA - log det R_A) / 2, the
                           information_gain of linear_update for the same set), logdet_joint (log det M_AA),
            covariance     the Covariance record of the path.
        Greedy's gain_total is at least (1 - 1 / e) of the best set of the same size.  The covariance blocks and the factor
        (budget x P blocks) stay on the device.  Raises DpgoError as gate does (R and t are not checked), and for a budget outside
        [1, P] or blocks and factor that do not fit the device.  One team only.  Changes no solver state."""
        if method not in (None, "dense", "schur", "nested"):
            raise ValueError("select_closures: method must be \"dense\", \"schur\" or \"nested\", not %r" % (method,))
        if order not in ("greedy", "given"):
            raise ValueError("select_closures: order must be \"greedy\" or \"given\", not %r" % (order,))
        N = int(sum(self.agents[i].n for i in self.ids))
        if T is None:
            T = self.round()[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("select_closures: T holds %d doubles, the team's %d poses need %d" % (T.size, N, 12 * N))
        cand = np.ascontiguousarray(candidates, dtype=MEAS_DTYPE).reshape(-1)
        P = len(cand)
        res = Covariance()
        gain, gc, rank = np.zeros(P), np.zeros(P), np.full(P, -1, dtype=np.int32)
        nsel, gt, lj = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        code = {None: GATE_DENSE, "dense": GATE_DENSE, "schur": GATE_SCHUR, "nested": GATE_NESTED}[method]
        p = lambda a: _d(a) if P else None
        _chk(lib().dpgo_team_select_candidates(self.h, _d(T), code, int(max_block or 0), P, p(cand),
                                               JOINT_GREEDY if order == "greedy" else JOINT_GIVEN, int(budget),
                                               C.c_double(-np.inf if min_gain is None else min_gain), p(gain), p(gc), p(rank),
                                               C.byref(nsel), C.byref(gt), C.byref(lj), C.byref(res)), "select_candidates")
        n = int(nsel.value)
        selected = np.argsort(np.where(rank >= 0, rank, P), kind="stable")[:n]
        return dict(candidates=cand, gain=gain, gain_cond=gc, rank=rank, selected=selected, num_selected=n,
                    gain_total=float(gt.value), logdet_joint=float(lj.value), covariance=res)

    def _linear_arguments(self, name, T, method, pairs):
        """what linear_update and linear_removal (`name`) marshal alike: (T flat and checked against the team's N poses, the
        rounded estimate when None; the method code; pairs as int32[P, 2]; the outputs T', delta, cov_diag and cov_pairs)"""
        if method not in (None, "dense", "schur", "nested"):
            raise ValueError("%s: method must be \"dense\", \"schur\" or \"nested\", not %r" % (name, method))
        N = int(sum(self.agents[i].n for i in self.ids))
        if T is None:
            T = self.round()[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("%s: T holds %d doubles, the team's %d poses need %d" % (name, T.size, N, 12 * N))
        pr = np.ascontiguousarray(np.zeros((0, 2)) if pairs is None else pairs, dtype=np.int32).reshape(-1, 2)
        code = {None: GATE_DENSE, "dense": GATE_DENSE, "schur": GATE_SCHUR, "nested": GATE_NESTED}[method]
        return T, code, pr, (np.zeros(12 * N), np.zeros((N, 6)), np.zeros((N, 6, 6)), np.zeros((len(pr), 6, 6)))

    def linear_update(self, closures, T=None, method=None, max_block=None, pairs=None, columns=None, transport=None,
                      owner_of_robot=None):
        """The estimate and its covariances updated to first order for a set of new closures, without a re-solve (DESIGN.md
        5j): the information-filter update of the whole trajectory.  closures, T, method and max_block as in gate_jointly, whose
        A, R and M = A Sigma A^T + R these are: with B = Sigma A^T, dx = -B M^-1 xi, Sigma' = Sigma - B M^-1 B^T and
        T' = T [+] dx (R_p <- R_p Exp(phi_p), t_p <- t_p + delta_p, pose 0 fixed) -- what a Gauss-Newton step from T on the graph
        with the closures added gives, with the Laplace covariance there.  pairs: team-order pose pairs (a, b) whose blocks
        Sigma'_ab are wanted beside the diagonal ones.  Returns a dict:
            T                T' in the layout of chordal_init (12 doubles per pose in team order),
            delta[N, 6]      dx_p = (phi_p, delta_p),
            cov_diag[N, 6, 6]  the diagonal blocks of Sigma', bitwise symmetric,
            cov_pairs[len(pairs), 6, 6]  the blocks Sigma'_ab,
            xi[K, 6]         the innovations at T: gate's,
            xi_post[K, 6]    R M^-1 xi = xi + A dx: the innovations at T' to first order,
            d2_joint         xi^T M^-1 xi: gate_jointly's for the same set,
            logdet_M, logdet_R, information_gain = (logdet_M - logdet_R) / 2,
            covariance       the Covariance record of the path (of Sigma, not Sigma').
        The covariance blocks, B, M and their products stay on the device.  Raises DpgoError as gate_jointly does, for a pair that
        names a pose outside the team, and for a batch whose blocks and matrices do not fit the device.  One team only.
        Changes no solver state.
        columns: how B = Sigma A^T is formed.  "blocks" (the default) asks the covariance path for the N m blocks
        Sigma_{p, e_a} of the m distinct endpoint poses and multiplies afterwards.  "solve" has the path apply Sigma to A^T on
        its own factors (covariance_apply) and asks it for `pairs` alone: the time no longer grows with the
        blocks extracted.  Under "solve" method is "dense" or "nested" ("schur" raises DpgoError: "nested" with no robot split
        has its sets), and the outputs are NOT bitwise those of "blocks", because the sums of B come in another order; they
        agree to round-off, and two calls of either route give the same bytes.
        With a transport (a team split across participants, owner_of_robot as for covariances; DESIGN.md 5j "Across teams"):
        the solve on the Schur path across is the only route (columns None or "solve", method None or "schur"; "blocks", any
        other method or a max_block raises ValueError before any transport call).  The call is collective: every participant
        passes the same closures, whose (r1, p1) -> (r2, p2) may name any robot of the problem, and the same pairs, which
        name poses of the whole problem (robots by id, then poses; pose 0 is robot 0's first).  T (None: the rounding
        across), and T, delta and cov_diag of the dict, are this team's poses in team order; cov_pairs, xi, xi_post, the
        scalars and the covariance record are complete and identical on every participant.  Every output is the same bits
        whatever the split; it is not bitwise the single team's call.  A ValueError (T's size) is raised on this participant
        alone before the library is called: check shapes before a collective call."""
        if columns not in (None, "blocks", "solve"):
            raise ValueError("linear_update: columns must be \"blocks\" or \"solve\", not %r" % (columns,))
        if transport is not None:
            if columns == "blocks":
                raise ValueError("linear_update: a team split across participants has the solve alone (columns=\"blocks\" with a "
                                 "transport)")
            T = self._across_args("linear_update", T, method, max_block, transport, owner_of_robot)
        T, code, pr, (Tn, dx, diag, cross) = self._linear_arguments("linear_update", T, method, pairs)
        cand = np.ascontiguousarray(closures, dtype=MEAS_DTYPE).reshape(-1)
        K = len(cand)
        res = Covariance()
        xi, xp, sc = np.zeros((K, 6)), np.zeros((K, 6)), np.zeros(3)
        p = lambda a: _d(a) if K else None
        if transport is not None:
            own = _owner_array(owner_of_robot)
            _chk(lib().dpgo_team_linear_update_across(self.h, C.byref(transport.struct), _d(own), _d(T), K, p(cand), len(pr),
                                                      _d(pr) if len(pr) else None, _d(Tn), _d(dx), _d(diag),
                                                      _d(cross) if len(pr) else None, _d(xi), _d(xp), _d(sc), C.byref(res)),
                 "linear_update_across")
        else:
            call = lib().dpgo_team_linear_update_solved if columns == "solve" else lib().dpgo_team_linear_update
            _chk(call(self.h, _d(T), code, int(max_block or 0), K, p(cand), len(pr), _d(pr) if len(pr) else None,
                      _d(Tn), _d(dx), _d(diag), _d(cross) if len(pr) else None, _d(xi), _d(xp), _d(sc),
                      C.byref(res)), "linear_update")
        return dict(T=Tn, delta=dx, cov_diag=diag, cov_pairs=cross, xi=xi, xi_post=xp, d2_joint=float(sc[0]), logdet_M=float(sc[1]),
                    logdet_R=float(sc[2]), information_gain=0.5 * float(sc[1] - sc[2]), covariance=res)

    def linear_removal(self, measurements, new_weight=None, T=None, method=None, max_block=None, pairs=None, min_redundancy=1e-6,
                       quantile=0.99):
        """Measurements that are in the graph removed or down-weighted in the estimate and its covariances, to first order and
        without a re-solve: the counterpart of linear_update for weight taken out of the graph, and the joint
        leave-K-out test audit does not give.  measurements: MEAS_DTYPE records as in audit, whose weight w > 0 says at which
        weight each is in the graph (taken on trust; the flags are ignored).  new_weight[K]: the weights w' they drop to,
        0 <= w' < w; None: all 0, the edges removed.  T must be a minimum of the graph that holds the records; T, method and
        max_block as in gate, pairs as in linear_update.  With dw = w - w', R_k = Sigma_meas,k / dw_k, A of gate_jointly and
        B = Sigma A^T: N = R - A B, dx = +B N^-1 xi, Sigma' = Sigma + B N^-1 B^T, T' = T [+] dx.  Returns a dict:
            measurements, new_weight  the records and the weights they go to,
            T, delta[N, 6], cov_diag[N, 6, 6], cov_pairs[len(pairs), 6, 6]  as in linear_update, of the graph without the weight,
            xi[K, 6]         the innovations at T: gate's,
            xi_loo[K, 6]     R N^-1 xi = xi + A dx: the innovations the records show against the graph without that weight; at
                             K = 1 audit's xi_loo,
            pivot_min[K]     the smallest Cholesky pivot of each record's own block of the whitened N: audit's pivot_min at
                             weight dw,
            d2_joint         xi^T N^-1 xi, twice the drop of the optimal cost.  At K = 1, w = 1, w' = 0 it is audit's d2; for
                             K > 1 at full weight the joint normalised-residual statistic, chi^2 with 6 K degrees of freedom
                             when the set is sound; with a fractional dw it is the cost the removed weight accounted for and
                             NOT audit's d2,
            logdet_N, logdet_R, information_loss = (logdet_R - logdet_N) / 2 = (log det H - log det H') / 2 >= 0,
            pivot_min_joint  the smallest pivot of the factor of the whitened N, in (0, 1]; the errors of every output grow
                             like its reciprocal,
            joint_accept     sqrt(d2_joint) <= error_threshold_at_quantile(quantile, 6 K): the set passes, and its removal is
                             not called for (gate_jointly's use of the threshold),
            covariance       the Covariance record of the path (of Sigma, not Sigma').
        What audit flags goes straight in:
            aud = team.audit(); mm = aud["measurements"]
            bad = mm[aud["testable"] & ~aud["accept"]]
            out = team.linear_removal(bad)            # T', Sigma' and the joint verdict now;
            # then agent.set_measurement_weight(..., 0.0) for each, team.set_initial(out["T"], ...) warm-starts the re-solve
        Raises DpgoError as linear_update does; for a weight that is not finite and positive, a new_weight that is negative, not
        finite or not below its weight, a min_redundancy outside (0, 1); and, behind the covariance path, for a record whose
        pivot_min is not above min_redundancy (a bridge: the record is named), a non-positive pivot of N, or a pivot_min_joint
        not above min_redundancy (the records together leave no redundancy: a cut).  One team only.  Changes no solver state,
        the team's weights included."""
        T, code, pr, (Tn, dx, diag, cross) = self._linear_arguments("linear_removal", T, method, pairs)
        meas = np.ascontiguousarray(measurements, dtype=MEAS_DTYPE).reshape(-1)
        K = len(meas)
        nw = np.zeros(K) if new_weight is None else np.ascontiguousarray(np.broadcast_to(np.asarray(new_weight, dtype=np.float64), (K,)))
        res = Covariance()
        xi, xl, pm, sc = np.zeros((K, 6)), np.zeros((K, 6)), np.zeros(K), np.zeros(4)
        p = lambda a: _d(a) if K else None
        _chk(lib().dpgo_team_linear_removal(self.h, _d(T), code, int(max_block or 0), K, p(meas), p(nw), C.c_double(min_redundancy),
                                            len(pr), _d(pr) if len(pr) else None, _d(Tn), _d(dx), _d(diag),
                                            _d(cross) if len(pr) else None, _d(xi), _d(xl), _d(pm), _d(sc), C.byref(res)),
             "linear_removal")
        d2 = float(sc[0])
        return dict(measurements=meas, new_weight=nw, T=Tn, delta=dx, cov_diag=diag, cov_pairs=cross, xi=xi, xi_loo=xl, pivot_min=pm,
                    d2_joint=d2, logdet_N=float(sc[1]), logdet_R=float(sc[2]), pivot_min_joint=float(sc[3]),
                    information_loss=0.5 * float(sc[2] - sc[1]),
                    joint_accept=bool(np.sqrt(d2) <= error_threshold_at_quantile(quantile, 6 * K)), covariance=res)


def _adjacency_words(adjacency):
    """a bool K x K matrix as K rows of ceil(K / 64) words, bit b of word w of row k = adjacency[k, 64 w + b]"""
    A = np.ascontiguousarray(adjacency, dtype=bool)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("max_clique: the adjacency matrix must be square, not of shape %r" % (A.shape,))
    K = A.shape[0]
    W = (K + 63) // 64
    padded = np.zeros((K, 64 * W), dtype=np.uint8)
    padded[:, :K] = A
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(K, W)


def _adjacency_bools(words, K):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(K, -1), axis=1, bitorder="little")[:, :K].astype(bool)


def max_clique(adjacency, max_nodes=0):
    """(members, proven): the ascending vertices of a maximum clique of the graph with the bool K x K matrix `adjacency`
    (symmetric, zero diagonal), by exact branch and bound on the host; the same input gives the same members.  After
    max_nodes search nodes (0: no limit) the search stops and returns the best clique found with proven = False."""
    words = _adjacency_words(adjacency)
    K = len(words)
    members, size, proven = np.zeros(max(K, 1), dtype=np.int32), C.c_int(0), C.c_int(0)
    _chk(lib().dpgo_max_clique(K, _d(words), C.c_longlong(int(max_nodes)), _d(members), C.byref(size), C.byref(proven)), "max_clique")
    return members[:size.value].copy(), bool(proven.value)


def pairwise_consistency(team_a, team_b, candidates, T_a=None, T_b=None, method=None, max_block=None, quantile=0.99, max_nodes=0):
    """The pairwise-consistent set of candidate loop closures between two teams that are not joined yet (pairwise consistency
    maximisation).  candidates: MEAS_DTYPE records whose (r1, p1) names a pose of team_a and (r2, p2) a pose of
    team_b, with R (row-major), t, kappa, tau; weight and the flags are ignored.  Each team has a connected weighted graph of
    its own (build one single-robot team per robot from its private measurements); they may be the same team.  T_a, T_b: the
    trajectories in the teams' own gauges (None: the rounding of that team's iterate, as in Team.gate); method, max_block: the
    covariance path of both teams, as in Team.gate.  For every two candidates the loop through both and through the two
    teams' own trajectories is tested against its covariance on the device; returns a dict with d2[K, K] (symmetric, zero
    diagonal), consistent (bool [K, K]: d2 <= error_threshold_at_quantile(quantile, 6) ** 2 off the diagonal), inliers (the
    ascending indices of a maximum clique of `consistent`), proven (False when max_nodes > 0 stopped the search) and res_a,
    res_b (each path's Covariance).  Raises DpgoError as Team.covariances does for either team, and for a candidate that names
    a robot or pose outside its team, has kappa <= 0 or tau <= 0, or an R outside SO(3).  Changes no solver state."""
    if method not in (None, "dense", "schur", "nested"):
        raise ValueError("pairwise_consistency: method must be \"dense\", \"schur\" or \"nested\", not %r" % (method,))
    Ts = []
    for team, T in ((team_a, T_a), (team_b, T_b)):
        N = int(sum(team.agents[i].n for i in team.ids))
        if T is None:
            T = team.round()[1]
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
        if T.size != 12 * N:
            raise ValueError("pairwise_consistency: T holds %d doubles, the team's %d poses need %d" % (T.size, N, 12 * N))
        Ts.append(T)
    cand = np.ascontiguousarray(candidates, dtype=MEAS_DTYPE).reshape(-1)
    K = len(cand)
    W = (K + 63) // 64
    d2, words = np.zeros((K, K)), np.zeros((K, max(W, 1)), dtype="<u8")
    members, size, proven = np.zeros(max(K, 1), dtype=np.int32), C.c_int(0), C.c_int(0)
    res_a, res_b = Covariance(), Covariance()
    code = {None: GATE_DENSE, "dense": GATE_DENSE, "schur": GATE_SCHUR, "nested": GATE_NESTED}[method]
    _chk(lib().dpgo_team_pairwise_consistency(team_a.h, _d(Ts[0]), team_b.h, _d(Ts[1]), code, int(max_block or 0), K, _d(cand),
                                              C.c_double(quantile), C.c_longlong(int(max_nodes)), _d(d2), _d(words), _d(members),
                                              C.byref(size), C.byref(proven), C.byref(res_a), C.byref(res_b)),
         "pairwise_consistency")
    return dict(d2=d2, consistent=_adjacency_bools(words, K), inliers=members[:size.value].copy(), proven=bool(proven.value),
                res_a=res_a, res_b=res_b)


def covariance_to_body_frame(cov, T):
    """Blocks of Team.covariances in the convention that perturbs the translation in the body frame as well (GTSAM's Pose3:
    t_i <- t_i + R_i delta'): A Sigma A^T with A_i = blockdiag(I, R_i^T).  cov: diagonal blocks [N, 6, 6] with T the
    trajectory (12 doubles per pose), or cross blocks [K, 6, 6] with T = (T_a, T_b): the trajectories' poses of each pair,
    e.g. (Tm[pairs[:, 0]], Tm[pairs[:, 1]]) for Tm = T.reshape(N, 12)."""
    cov = np.asarray(cov, dtype=np.float64)

    def A_of(Tx):
        R = np.asarray(Tx, dtype=np.float64).reshape(-1, 4, 3)[:, :3, :].transpose(0, 2, 1)  # [pose][b][c]
        A = np.zeros((len(R), 6, 6))
        A[:, :3, :3] = np.eye(3)
        A[:, 3:, 3:] = R.transpose(0, 2, 1)
        return A

    Aa, Ab = (A_of(T[0]), A_of(T[1])) if isinstance(T, tuple) else (A_of(T),) * 2
    if len(Aa) != len(cov) or len(Ab) != len(cov):
        raise ValueError("covariance_to_body_frame: %d blocks, %d / %d poses" % (len(cov), len(Aa), len(Ab)))
    return Aa @ cov @ Ab.transpose(0, 2, 1)


def _params_at_rank(params, r):
    p = Params.from_buffer_copy(params)
    p.r = r
    return p


def riemannian_staircase(meas, params, r0, r_max=8, eta=1e-6, T=None, X0=None, iters=20, first_iters=None, alpha0=None,
                         max_backtracks=30, certify_kw=None, device=0):
    """Riemannian staircase over the team solver: run the team at rank r (`iters` iterations of dpgo_team_run, or
    `first_iters` at r0), certify; when the point is not certified, start rank r + 1 from the escape point
    [X; 0] + alpha [0; v^T] along the certificate's direction v, alpha halved until the cost decreases.  Stops when
    certified or at r_max.  The start is T lifted with the fixed Stiefel matrix (dpgo_team_set_initial), or X0 (rank r0,
    team order).  Returns dict(X=per-agent iterates, r=final rank, ranks=rank path, certificate=last Certificate,
    costs=cost at the end of every rank, escape_costs=[(cost before, cost after)] of every escape)."""
    return _staircase(meas, params, r0, r_max, eta, T, X0, iters, first_iters, alpha0, max_backtracks, certify_kw, device)


def _staircase(meas, params, r0, r_max, eta, T, X0, iters, first_iters, alpha0, max_backtracks, certify_kw, device,
               on_final=None):
    """the staircase loop; on_final(team, out) runs on the final team before it is closed and may add to `out`"""
    certify_kw = dict(certify_kw or {})
    r = r0
    team = Team.from_measurements(meas, _params_at_rank(params, r), device=device)
    try:
        if X0 is not None:
            X0 = np.asarray(X0, dtype=np.float64).reshape(-1)
            ofs = 0
            for i in team.ids:
                n = team.agents[i].n
                team.agents[i].set_X(X0[ofs:ofs + r * 4 * n])
                ofs += r * 4 * n
            team.exchange_all()
        else:
            team.set_initial(T, fixed_stiefel(r))
        ranks, costs, escapes = [r], [], []
        n_it = iters if first_iters is None else first_iters
        while True:
            if n_it > 0:
                team.run(n_it)
            n_it = iters
            f = team.cost()
            costs.append(f)
            cert, v = team.certify(eta=eta, **certify_kw)
            if cert.certified != 0 or r >= r_max:
                Xs = [team.agents[i].get_X() for i in team.ids]
                out = dict(X=Xs, r=r, ranks=ranks, certificate=cert, costs=costs, escape_costs=escapes)
                if on_final is not None:
                    on_final(team, out)
                return out
            Xs = [team.agents[i].get_X() for i in team.ids]
            ns = [team.agents[i].n for i in team.ids]
            team.close()
            team = Team.from_measurements(meas, _params_at_rank(params, r + 1), device=device)
            offs = np.concatenate([[0], np.cumsum(ns)])
            alpha = float(alpha0) if alpha0 is not None else np.sqrt(float(offs[-1]))
            taken = None
            for _ in range(max_backtracks):
                for k, i in enumerate(team.ids):
                    vk = v[4 * offs[k]:4 * offs[k + 1]]
                    team.agents[i].set_X(escape_point(Xs[k], r, ns[k], vk, alpha))
                team.exchange_all()
                f2 = team.cost()
                if f2 < f:
                    taken = f2
                    break
                alpha *= 0.5
            if taken is None:
                raise DpgoError("riemannian_staircase: no step along the escape direction decreased the cost")
            escapes.append((f, taken))
            r += 1
            ranks.append(r)
    finally:
        team.close()


def solve_certified(meas, params, r0=5, r_max=8, eta=1e-6, T=None, X0=None, iters=20, first_iters=None,
                    refine_translations=True, certify_kw=None, device=0, covariances=False, covariance_method="dense",
                    covariance_max_block=None, audit=False, refine=False):
    """End to end: the Riemannian staircase, then the SE-Sync rounding of its final point (Team.round on the final team).
    Returns dict(T=trajectory, 12 doubles per pose in team order anchored at the first pose, r=final rank, ranks,
    certificate, rounding=Rounding, f_relaxed, f_rounded, gap_rel, escape_costs).  gap_rel = (f_rounded - f_relaxed) /
    f_relaxed bounds the relative suboptimality of T (up to the certificate's eta) when the point is certified; it is None
    otherwise.  covariances=True adds covariances=(Covariance, diag[N, 6, 6]): Team.covariances of the final team at T by
    covariance_method ("dense", "schur", or "nested" with covariance_max_block).  audit=True adds audit=Team.audit() of the final
    team at T, its own measurements at their final weights, by the same covariance_method / covariance_max_block.
    refine=True refines the rounded T to a critical point on SE(3) (Team.refine at its defaults, on the dense path or, for
    covariance_method "schur" / "nested", the nested one at covariance_max_block: the Schur path has no apply) and adds refine=its dict; T, the covariances and the audit are then
    taken at the refined T, while rounding and f_rounded stay those of the rounded point."""
    def round_final(team, out):
        out["rounding"], out["T"] = team.round(refine_translations=refine_translations)
        if refine:
            out["refine"] = team.refine(out["T"], method="dense" if covariance_method == "dense" else "nested",
                                        max_block=covariance_max_block)
            out["T"] = out["refine"]["T"]
        if covariances:
            if covariance_method == "nested":
                out["covariances"] = team.covariances_nested(out["T"], max_block=covariance_max_block)[:2]
            else:
                out["covariances"] = team.covariances(out["T"], method=covariance_method)[:2]
        if audit:
            out["audit"] = team.audit(T=out["T"], method=covariance_method, max_block=covariance_max_block)

    out = _staircase(meas, params, r0, r_max, eta, T, X0, iters, first_iters, None, 30, certify_kw, device,
                     on_final=round_final)
    rd, cert = out["rounding"], out["certificate"]
    gap = (rd.f_rounded - rd.f_relaxed) / rd.f_relaxed if cert.certified == 1 else None
    res = dict(T=out["T"], r=out["r"], ranks=out["ranks"], certificate=cert, rounding=rd, f_relaxed=rd.f_relaxed,
               f_rounded=rd.f_rounded, gap_rel=gap, escape_costs=out["escape_costs"])
    if covariances:
        res["covariances"] = out["covariances"]
    if audit:
        res["audit"] = out["audit"]
    if refine:
        res["refine"] = out["refine"]
    return res
