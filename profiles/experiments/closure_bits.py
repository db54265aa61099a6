"""the bit comparison of profiles/r18_closure_frame.md and r28_linear_frame.md: every output of the six calls behind the
covariance paths (Team.gate / relative_covariances, Team.audit, Team.gate_jointly, Team.linear_update, Team.linear_removal,
capi.pairwise_consistency) under the inputs of their own GPU tests -- the three methods, both orders of the joint gate, the update
with and without pairs and on both routes (columns="blocks" and "solve"), the removal at full and fractional weight, duplicated
records, candidates at pose 0, the K = 65 ballot-tile edge.  The Python entry points are wrapped, the seven test files run in this
process, and each call leaves one line: its name and a SHA-256 per output array, the Covariance records without their times.  One process per
library (DPGO_HIP_LIB names the other one); two dumps are compared line by line.
usage: python profiles/experiments/closure_bits.py OUT.json            run the tests, write the dump
       python profiles/experiments/closure_bits.py A.json B.json       -> calls, arrays, arrays that differ"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TESTS = ["test_gpu_gate.py", "test_gpu_gate_joint.py", "test_gpu_audit.py", "test_gpu_linear_update.py", "test_gpu_consistency.py",
         "test_gpu_linear_removal.py", "test_gpu_linear_update_solved.py"]
TIMES = ("seconds",)  # the fields of a Covariance record that are measured, not computed


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    arrays = differ = 0
    if len(A) != len(B):
        print("the dumps hold %d and %d calls" % (len(A), len(B)))
        return 1
    for k, (x, y) in enumerate(zip(A, B)):
        if x["call"] != y["call"] or sorted(x["out"]) != sorted(y["out"]):
            print("call %d: %s against %s" % (k, x["call"], y["call"]))
            return 1
        for name in x["out"]:
            arrays += 1
            if x["out"][name] != y["out"][name]:
                differ += 1
                print("call %d (%s, %s): %s differs" % (k, x["call"], x["args"], name))
    print(json.dumps(dict(calls=len(A), arrays=arrays, arrays_differing=differ)))
    return 1 if differ else 0


if len(sys.argv) == 3:
    sys.exit(compare(sys.argv[1], sys.argv[2]))

import ctypes

import numpy as np
import pytest

from dpgo_ros_amd import capi

calls = []


def digest(v):
    if isinstance(v, np.ndarray):
        return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
    if isinstance(v, ctypes.Structure):
        return hashlib.sha256(repr([(f[0], getattr(v, f[0])) for f in v._fields_ if not f[0].startswith(TIMES)]).encode()).hexdigest()
    return hashlib.sha256(repr(v).encode()).hexdigest()


def record(name, fn):
    def wrapped(*a, **kw):
        out = fn(*a, **kw)
        items = out.items() if isinstance(out, dict) else enumerate(out)
        args = {k: v for k, v in kw.items() if isinstance(v, (str, int, float, bool, type(None)))}
        calls.append(dict(call=name, args=repr(sorted(args.items())), out={str(k): digest(v) for k, v in items if v is not None}))
        return out
    return wrapped


capi.Team._gate_call = record("gate_candidates", capi.Team._gate_call)
capi.Team.audit = record("audit_measurements", capi.Team.audit)
capi.Team.gate_jointly = record("gate_candidates_jointly", capi.Team.gate_jointly)
capi.Team.linear_update = record("linear_update", capi.Team.linear_update)
capi.Team.linear_removal = record("linear_removal", capi.Team.linear_removal)
capi.pairwise_consistency = record("pairwise_consistency", capi.pairwise_consistency)

rc = pytest.main(["-q", "-x", "-p", "no:cacheprovider"] + [os.path.join(ROOT, "tests", f) for f in TESTS])
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
json.dump(calls, open(sys.argv[1], "w"))
sys.stderr.write("%d calls, pytest returned %d, library %s\n" % (len(calls), int(rc), capi.LIB_PATH))
sys.exit(int(rc))
