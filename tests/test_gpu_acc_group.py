"""-m gpu: the accumulation kernels in 64-, 128- and 256-thread workgroups (GS_ACC_GROUP_G1 / GS_ACC_GROUP_G2, csrc/knobs.h; the policy
that chooses when no switch is set is csrc/acc_shape.h, walked on the host by test_acc_shape_host.py).  The switches are read once per
process, so every setting runs in a child process of its own; the sums are compared here with the C oracle's naive MulScalar / Add loop,
computed once.

Shapes.  k_bucket_accumulate runs one thread per chunk of 16 bucket entries, ceil(15 n / 16) + 1 chunk threads for n terms at these
sizes, in grid.x = ceil(threads / group) workgroups whose last one is partial: n = 1, 3, 4 (a handful of threads in one group), 66-69,
134-137 and 271-274 (63-66, 127-130 and 256-258 threads: either side of one full group of each size), 1000 (939 threads: several groups
of every size), one vector of zeros (no entries at all: every thread leaves at `beg >= total`) and one of equal scalars (one heavy
bucket per window, cut into many chunks)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 4, 66, 67, 68, 69, 134, 135, 136, 137, 271, 272, 273, 274, 1000]
NMAX = 1000
N_ZERO, N_EQUAL = 272, 1000
SETTINGS = [(64, 64), (128, 128), (256, 256), (64, 256)]

# The child: every MSM through gs_msm_g1 / gs_msm_g2 (blocking) on both summation routes, the 1000-term ones also as tickets
# (gs_msm_*_begin / gs_msm_end); then three pipelined 2^10-constraint Groth16 proofs in flight at once and the blocking proof.
_CHILD = r"""
import sys, json
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import gosnark_amd
from gosnark_amd import capi, synth, groth16
import gpu_util as U
SIZES, NMAX, N_ZERO, N_EQUAL = %(sizes)r, %(nmax)d, %(nzero)d, %(nequal)d
capi.init(0)
out = {}
for g2 in (False, True):
    fixed = capi.g2_fixed_base if g2 else capi.g1_fixed_base
    bases = fixed(U.rand_scalars_u64(NMAX, 9100 + g2))
    sc = U.rand_scalars_u64(NMAX, 9200 + g2)
    equal = np.repeat(U.rand_scalars_u64(1, 9300 + g2), N_EQUAL, axis=0)
    scal = capi.scalars_upload(sc)
    for policy in ("never", "always"):            # table-free first: `always` builds the array's window table in its first call
        capi.set_table_policy(policy)
        res = {str(n): capi.msm(bases, sc[:n], g2=g2) for n in SIZES}
        res["zero"] = capi.msm(bases, np.zeros((N_ZERO, 4), dtype=np.uint64), g2=g2)
        res["equal"] = capi.msm(bases, equal, g2=g2)
        tickets = [capi.msm_begin(bases, scal, NMAX, g2=g2) for _ in range(3)]
        res["tickets"] = [capi.msm_end(t) for t in tickets]
        out["%%s/%%s" %% ("g2" if g2 else "g1", policy)] = res
capi.set_table_policy("always")
inst = synth.sqchain_setup_instance(1024, 77)
r, s = synth.field_elems(2, 5)
pk = inst.device_pk()
tickets = [groth16.prove_begin(pk, inst.w, inst.px, r, s) for _ in range(3)]
out["pipelined"] = [[p.PiA, p.PiB, p.PiC] for p in (groth16.prove_end(t) for t in tickets)]
p = groth16.prove_resident(pk, inst.w, inst.px, r, s)
out["blocking"] = [p.PiA, p.PiB, p.PiC]
print(json.dumps(out))
"""


def _child(env):
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "sizes": SIZES, "nmax": NMAX, "nzero": N_ZERO, "nequal": N_EQUAL}
    clean = {k: v for k, v in os.environ.items() if k not in ("GS_ACC_GROUP_G1", "GS_ACC_GROUP_G2")}
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(clean, **env), timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


def _listed(x):
    """what json.dumps / json.loads makes of a result: tuples -> lists"""
    return json.loads(json.dumps(x))


@pytest.fixture(scope="module")
def oracle_sums():
    """The expected sums, once: the same bases and scalars as the children make (fixed-base products of seeded scalars), summed by the
    C oracle's naive loop."""
    from gosnark_amd import capi
    import gpu_util as U
    from oracle import c_oracle as C
    capi.init(0)
    threads = min(8, os.cpu_count() or 1)
    want = {}
    for g2 in (False, True):
        fixed, download = (capi.g2_fixed_base, capi.g2_download) if g2 else (capi.g1_fixed_base, capi.g1_download)
        naive, affine = (C.g2_msm_naive, C.g2_affine) if g2 else (C.g1_msm_naive, C.g1_affine)
        bases = fixed(U.rand_scalars_u64(NMAX, 9100 + g2))
        pts = np.asarray(download(bases))
        bases.free()
        sc = U.rand_scalars_u64(NMAX, 9200 + g2)
        equal = np.repeat(U.rand_scalars_u64(1, 9300 + g2), N_EQUAL, axis=0)
        res = {str(n): affine(naive(pts[:n], sc[:n], threads=threads)) for n in SIZES}
        res["zero"] = None
        res["equal"] = affine(naive(pts[:N_EQUAL], equal, threads=threads))
        res["tickets"] = [res[str(NMAX)]] * 3
        want["g2" if g2 else "g1"] = _listed(res)
    return want


@pytest.fixture(scope="module")
def child_256():
    """the 256 / 256 child: its blocking proof is what every other child's proofs must equal"""
    return _child({"GS_ACC_GROUP_G1": "256", "GS_ACC_GROUP_G2": "256"})


def _check(got, oracle_sums, blocking):
    for curve in ("g1", "g2"):
        for policy in ("never", "always"):
            res = got["%s/%s" % (curve, policy)]
            for key, want in oracle_sums[curve].items():
                assert res[key] == want, "%s MSM, table policy %s, case %s differs from the oracle's naive sum" % (curve, policy, key)
    assert got["blocking"] == blocking, "the blocking proof differs from the 256 / 256 child's"
    for i, p in enumerate(got["pipelined"]):
        assert p == blocking, "pipelined proof %d of three in flight differs from the blocking proof of the 256 / 256 child" % i


@pytest.mark.parametrize("g1,g2", SETTINGS, ids=["%d-%d" % s for s in SETTINGS])
def test_forced_group_sizes_sum_what_the_oracle_sums(g1, g2, oracle_sums, child_256):
    """G1 and G2 MSMs at every size above, window tables and table-free, blocking and as tickets, against the oracle; then three
    Groth16 proofs of 2^10 constraints in flight at once, each equal to the blocking proof computed with 256-thread groups."""
    got = child_256 if (g1, g2) == (256, 256) else _child({"GS_ACC_GROUP_G1": str(g1), "GS_ACC_GROUP_G2": str(g2)})
    _check(got, oracle_sums, child_256["blocking"])


def test_values_the_switches_cannot_take_are_ignored(oracle_sums, child_256):
    """100 threads (no multiple of a wave) for G1 and 512 (more than __launch_bounds__ allows) for G2: both switches are ignored -- every
    sum and every proof equals what a child with neither switch set gives, the oracle's sums and the 256 / 256 child's proof."""
    default = _child({})
    got = _child({"GS_ACC_GROUP_G1": "100", "GS_ACC_GROUP_G2": "512"})
    _check(default, oracle_sums, child_256["blocking"])
    assert got == default
