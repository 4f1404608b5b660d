"""gs_groth16_verify_batch against a loop of gs_groth16_verify, timed in one process on one GPU -- dev tool.

    python tools/time_verify_batch.py [nproofs = 4096] [profiles/verify_batch_timing.txt] ["resource-usage lines of the kernels"]      (overwrites)

nproofs proofs of the committed x^3 + x + 5 key (tests/golden/wasm_groth_x3.json) come from the device prover, each with its own witness
and (r, s).  After a warm-up of both sides, REPS rounds alternate
  * ONE gs_groth16_verify_batch call over all of them (arguments marshalled beforehand: wall time of the C call), and
  * the yardstick, set before any run: gs_groth16_verify in a loop over a sample of SAMPLE of the same proofs, on one core.
The bound: the batch's wall time per proof is at most 1/16 of the host loop's -- a job on these machines has 16 CPUs and a caller could
spread the host loop over them; the device route is worth having only beyond that.
The stages of the batch call are then repeated as the library calls the batch makes (uploads + gs_g2_subgroup_check, gs_g1_scale_powers,
gs_msm_g1, gs_pairing_product), alternating, with their wall and device times (gs_last_timing); "host tail" is what the batch call's
wall time has beyond the stages: the weights, the public-input sum, the three key pairs of the multi-Miller loop (the one final
exponentiation is inside gs_pairing_product's wall time here).
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "verify_batch_timing.txt")
resource = sys.argv[3] if len(sys.argv) > 3 else "(not given)"
R = O.R
rng = random.Random(31)
capi.init()
lib = capi.load_library()

with open(os.path.join(ROOT, "tests", "golden", "wasm_groth_x3.json")) as f:
    rec = json.load(f)
setup = json.loads(rec["setup"])
pk, vk = utils.GrothSetupFromString(setup)
circ = groth16.Circuit(len(O.X3_WITNESS), 1)
al, be, ga, _ = O.PF.R1CSToQAP(O.X3_R1CS_A, O.X3_R1CS_B, O.X3_R1CS_C)
t0 = time.perf_counter()
proofs, pubs = [], []
for i in range(nproofs):
    x = 3 + i
    out = x ** 3 + x + 5
    w = [1, out, x, x * x, x ** 3, x ** 3 + x, out, 1]
    proofs.append(groth16.GenerateProofsWithRS(circ, pk, w, O.PF.CombinePolynomials(w, al, be, ga)[3], rng.randrange(1, R), rng.randrange(1, R)))
    pubs.append(out)
prove_s = time.perf_counter() - t0

g1 = capi.g1_points_to_u64([vk.G1_Alpha])
g2 = capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta])
ic = capi.g1_points_to_u64(vk.IC)
pub = capi.ints_to_u64(pubs)
a = capi.g1_points_to_u64([p.PiA for p in proofs])
b = capi.g2_points_to_u64([p.PiB for p in proofs])
c = capi.g1_points_to_u64([p.PiC for p in proofs])
s = rng.randrange(2, R)
challenge = capi.ints_to_u64([s])
z = capi.ints_to_u64([pow(s, i, R) for i in range(nproofs)])
key = (capi.ptr64(g1[0]), capi.ptr64(g2[0]), capi.ptr64(g2[1]), capi.ptr64(g2[2]), capi.ptr64(ic), len(vk.IC))


def batch():
    ok = ctypes.c_int(0)
    t = time.perf_counter()
    capi.call("gs_groth16_verify_batch", *key, capi.ptr64(pub), 1, capi.ptr64(a), capi.ptr64(b), capi.ptr64(c), nproofs, capi.ptr64(challenge), ctypes.byref(ok))
    ms = (time.perf_counter() - t) * 1e3
    assert ok.value == 1
    return ms


def host_loop():
    ok = ctypes.c_int(0)
    t = time.perf_counter()
    for i in range(SAMPLE):
        capi.call("gs_groth16_verify", *key, capi.ptr64(pub[i]), 1, capi.ptr64(a[i]), capi.ptr64(b[i]), capi.ptr64(c[i]), ctypes.byref(ok))
        assert ok.value == 1
    return (time.perf_counter() - t) * 1e3


def stages():
    """[(name, wall ms, device ms)] of the library calls the batch makes, in its order."""
    rows = []

    def timed(name, f):
        t = time.perf_counter()
        r = f()
        rows.append((name, (time.perf_counter() - t) * 1e3, capi.last_timing()["total_ms"]))
        return r

    t = time.perf_counter()
    ha, hb, hc = capi.g1_upload(a), capi.g2_upload(b), capi.g1_upload(c)
    up = (time.perf_counter() - t) * 1e3
    assert timed("membership", lambda: capi.g2_subgroup_check(hb)) == (0, None)
    rows[-1] = ("uploads and membership", rows[-1][1] + up, rows[-1][2])
    hna = timed("scale", lambda: capi.g1_scale_powers(ha, 0, nproofs, R - 1, s))
    timed("MSM", lambda: capi.msm(hc, z))
    timed("Miller and product", lambda: capi.pairing_product(hna, 0, hb, 0, nproofs))
    for h in (ha, hb, hc, hna):
        h.free()
    return rows


samples = {"batch": [], "host": []}
stage_rows = []
for rep in range(REPS + 1):                                            # rep 0 warms everything up; the sides alternate
    bm, hm, st = batch(), host_loop(), stages()
    if rep:
        samples["batch"].append(bm)
        samples["host"].append(hm)
        stage_rows.append(st)
batch_ms, host_ms = statistics.median(samples["batch"]), statistics.median(samples["host"])
per_batch, per_host = batch_ms / nproofs, host_ms / SAMPLE
ratio = per_batch / per_host
lines = ["gs_groth16_verify_batch over %d proofs of the x^3 + x + 5 key against gs_groth16_verify in a loop over %d of them, one process," % (nproofs, SAMPLE),
         "alternating, medians of %d after a warm-up of both (the %d proofs took the device prover %.1f s to make)" % (REPS, nproofs, prove_s),
         "  batch      wall %9.2f ms   (%s)   %8.2f us / proof" % (batch_ms, "  ".join("%.2f" % v for v in samples["batch"]), per_batch * 1e3),
         "  host loop  wall %9.2f ms   (%s)   %8.2f us / proof, one core" % (host_ms, "  ".join("%.2f" % v for v in samples["host"]), per_host * 1e3),
         "  bound, set before any run: batch time per proof <= 1/16 of the host loop's (0.0625): ratio %.4f (1/%.1f): %s"
         % (ratio, 1 / ratio, "MET" if ratio <= 1 / 16 else "NOT MET"),
         "  the batch call by stage (the same library calls made one by one; wall / device ms, medians):"]
total_wall = 0.0
for k in range(len(stage_rows[0])):
    wall = statistics.median(r[k][1] for r in stage_rows)
    dev = statistics.median(r[k][2] for r in stage_rows)
    total_wall += wall
    lines.append("    %-24s wall %8.2f   device %8.2f" % (stage_rows[0][k][0], wall, dev))
lines += ["    %-24s wall %8.2f   (batch wall - the stages: weights, public-input sum, the three key pairs)" % ("host tail", max(batch_ms - total_wall, 0.0)),
          "  kernels, hipcc -Rpass-analysis=kernel-resource-usage: %s" % resource, ""]
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
