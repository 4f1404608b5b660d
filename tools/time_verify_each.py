"""gs_groth16_verify_each against a loop of gs_groth16_verify and against gs_groth16_verify_batch, timed in one process on one GPU -- dev tool.

    python tools/time_verify_each.py [nproofs = 4096] [profiles/verify_each_timing.txt] ["resource-usage lines of the kernels"]      (overwrites)

nproofs proofs of the committed x^3 + x + 5 key (tests/golden/wasm_groth_x3.json) come from the device prover, each with its own witness
and (r, s).  Two batches: all valid, and the same with ONE proof made invalid (its C moved by the generator).  After a warm-up, REPS
rounds alternate, for each batch,
  * ONE gs_groth16_verify_each call (arguments marshalled beforehand: wall time of the C call) with its device-time split from
    gs_last_timing: h2d_ms = signals, lines and key value, poly_ms = membership of the B_i, plan_ms = vkx, accumulate_ms = Miller loops,
    reduce_ms = final exponentiations; what the wall time has beyond the device time is the host's screening of the 3n points, the
    uploads of the three arrays and the key work,
  * the yardstick, set before any run: gs_groth16_verify in a loop over a sample of SAMPLE of the same proofs, on one core, and
  * gs_groth16_verify_batch on the same proofs (its ratio to the per-proof call is recorded, not bounded).
The bound is the one the batch verifier was held to: per proof the device call takes at most 1/16 of the host loop -- a job on these
machines has 16 CPUs and a caller could spread the host loop over them.
The third argument is copied into the file: the register / LDS / scratch / occupancy figures of the kernels from
hipcc -Rpass-analysis=kernel-resource-usage, which this tool cannot produce itself."""
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi, groth16, utils  # noqa: E402
from oracle import ref_py as O  # noqa: E402

REPS, SAMPLE = 5, 64
nproofs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "verify_each_timing.txt")
resource = sys.argv[3] if len(sys.argv) > 3 else "(not given)"
R = O.R
rng = random.Random(32)
capi.init()

with open(os.path.join(ROOT, "tests", "golden", "wasm_groth_x3.json")) as f:
    rec = json.load(f)
setup = json.loads(rec["setup"])
pk, vk = utils.GrothSetupFromString(setup)
circ = groth16.Circuit(len(O.X3_WITNESS), 1)
al, be, ga, _ = O.PF.R1CSToQAP(O.X3_R1CS_A, O.X3_R1CS_B, O.X3_R1CS_C)
proofs, pubs = [], []
for i in range(nproofs):
    x = 3 + i
    out = x ** 3 + x + 5
    w = [1, out, x, x * x, x ** 3, x ** 3 + x, out, 1]
    proofs.append(groth16.GenerateProofsWithRS(circ, pk, w, O.PF.CombinePolynomials(w, al, be, ga)[3], rng.randrange(1, R), rng.randrange(1, R)))
    pubs.append(out)
BAD = nproofs // 2

g1 = capi.g1_points_to_u64([vk.G1_Alpha])
g2 = capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta])
ic = capi.g1_points_to_u64(vk.IC)
pub = capi.ints_to_u64(pubs)
a = capi.g1_points_to_u64([p.PiA for p in proofs])
b = capi.g2_points_to_u64([p.PiB for p in proofs])
c_good = capi.g1_points_to_u64([p.PiC for p in proofs])
c_bad = c_good.copy()
c_bad[BAD] = capi.g1_points_to_u64([O.G1.Add(proofs[BAD].PiC, O.G1_GEN)])[0]
challenge = capi.ints_to_u64([rng.randrange(2, R)])
key = (capi.ptr64(g1[0]), capi.ptr64(g2[0]), capi.ptr64(g2[1]), capi.ptr64(g2[2]), capi.ptr64(ic), len(vk.IC))
PARTS = ("total_ms", "h2d_ms", "poly_ms", "plan_ms", "accumulate_ms", "reduce_ms")


def each(c, bad):
    ok, nbad = np.zeros(nproofs, dtype=np.intc), ctypes.c_uint64(0)
    t = time.perf_counter()
    capi.call("gs_groth16_verify_each", *key, capi.ptr64(pub), 1, capi.ptr64(a), capi.ptr64(b), capi.ptr64(c), nproofs, ok.ctypes.data_as(capi.intp),
              ctypes.byref(nbad))
    ms = (time.perf_counter() - t) * 1e3
    tm = capi.last_timing()
    assert nbad.value == len(bad) and [i for i in range(nproofs) if not ok[i]] == bad
    return (ms,) + tuple(tm[k] for k in PARTS)


def batch(c, want):
    ok = ctypes.c_int(0)
    t = time.perf_counter()
    capi.call("gs_groth16_verify_batch", *key, capi.ptr64(pub), 1, capi.ptr64(a), capi.ptr64(b), capi.ptr64(c), nproofs, capi.ptr64(challenge), ctypes.byref(ok))
    ms = (time.perf_counter() - t) * 1e3
    assert ok.value == want
    return ms


def host_loop():
    ok = ctypes.c_int(0)
    t = time.perf_counter()
    for i in range(SAMPLE):
        capi.call("gs_groth16_verify", *key, capi.ptr64(pub[i]), 1, capi.ptr64(a[i]), capi.ptr64(b[i]), capi.ptr64(c_good[i]), ctypes.byref(ok))
        assert ok.value == 1
    return (time.perf_counter() - t) * 1e3


rows = {"good": [], "bad": [], "host": [], "batch_good": [], "batch_bad": []}
for rep in range(REPS + 1):                                            # rep 0 warms everything up; the sides alternate
    r = (each(c_good, []), each(c_bad, [BAD]), host_loop(), batch(c_good, 1), batch(c_bad, 0))
    if rep:
        for k, v in zip(rows, r):
            rows[k].append(v)
med = lambda xs: statistics.median(xs)   # noqa: E731
per_host = med(rows["host"]) / SAMPLE
lines = ["gs_groth16_verify_each over %d proofs of the x^3 + x + 5 key against gs_groth16_verify in a loop over %d of them and gs_groth16_verify_batch" % (nproofs, SAMPLE),
         "on the same proofs, one process, alternating, medians of %d after a warm-up of all" % REPS,
         "  host loop   wall %9.2f ms   %8.2f us / proof, one core" % (med(rows["host"]), per_host * 1e3)]
worst = 0.0
for name, label in (("good", "all valid"), ("bad", "one invalid")):
    wall = med([r[0] for r in rows[name]])
    parts = [med([r[1 + k] for r in rows[name]]) for k in range(len(PARTS))]
    ratio = wall / nproofs / per_host
    worst = max(worst, ratio)
    lines += ["  each, %-11s wall %8.2f ms   (%s)   %7.2f us / proof   ratio to the host loop %.4f (1/%.1f)"
              % (label, wall, "  ".join("%.2f" % r[0] for r in rows[name]), wall / nproofs * 1e3, ratio, 1 / ratio),
              "      device %.2f ms: signals, lines and key value up %.2f, membership %.2f, vkx %.2f, Miller %.2f, final exponentiation %.2f;"
              % tuple(parts),
              "      host screening of the 3n points, uploads of A, B, C and key work (wall - device) %.2f" % max(wall - parts[0], 0.0)]
    bw = med(rows["batch_" + name])
    lines.append("      gs_groth16_verify_batch on the same proofs %.2f ms (%s): each / batch = %.2f (recorded, not bounded)"
                 % (bw, "ACCEPT" if name == "good" else "REJECT", wall / bw))
lines += ["  bound, set before any run: time per proof <= 1/16 of the host loop's (0.0625), the worse of the two batches: ratio %.4f (1/%.1f): %s"
          % (worst, 1 / worst, "MET" if worst <= 1 / 16 else "NOT MET"),
          "  kernels, hipcc -Rpass-analysis=kernel-resource-usage: %s" % resource, ""]
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
