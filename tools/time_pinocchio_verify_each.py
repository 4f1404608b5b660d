"""gs_pinocchio_verify_each against a loop of gs_pinocchio_verify, and beside gs_groth16_verify_each, timed in one process on one GPU -- dev tool.

    python tools/time_pinocchio_verify_each.py [nproofs = 4096] [profiles/pinocchio_verify_each_timing.txt] ["resource usage of the kernels"]      (overwrites)

nproofs proofs of the committed x^3 + x + 5 Pinocchio key (tests/golden/wasm_pinocchio_x3_setup.json) come from the device prover, each
with its own witness.  Two batches: all valid, and the same with ONE proof made invalid (its PiH moved by the generator: equation 4).
After a warm-up, REPS rounds alternate, for each batch,
  * ONE gs_pinocchio_verify_each call (arguments marshalled beforehand: wall time of the C call) with its device-time split from
    gs_last_timing: h2d_ms = signals and the six prepared lists, poly_ms = membership of the PiB_i, plan_ms = vkx and the two sums,
    accumulate_ms = Miller loops, reduce_ms = final exponentiations; what the wall time has beyond the device time is the host's
    screening of the 8n points, the uploads and the key work,
  * the yardstick, set before any run: gs_pinocchio_verify in a loop over a sample of SAMPLE of the same proofs, on one core, and
  * gs_groth16_verify_each over nproofs proofs of the Groth16 key of the same circuit (the ratio is recorded, not bounded).
The bound is the one the other device verifiers were held to: per proof the device call takes at most 1/16 of the host loop -- a job on
these machines has 16 CPUs and a caller could spread the host loop over them.
The third argument is copied into the file: the register / LDS / scratch figures of the kernels from the code-object metadata, which
this tool cannot produce itself."""
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
from gosnark_amd import capi, groth16, snark, utils  # noqa: E402
from oracle import ref_py as O  # noqa: E402

REPS, SAMPLE = 5, 64
nproofs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "pinocchio_verify_each_timing.txt")
resource = sys.argv[3] if len(sys.argv) > 3 else "(not given)"
R = O.R
rng = random.Random(33)
capi.init()


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.loads(json.load(f)["setup"])


pk, vk = utils.SetupFromString(golden("wasm_pinocchio_x3_setup.json"))
gpk, gvk = utils.GrothSetupFromString(golden("wasm_groth_x3.json"))
circ, gcirc = snark.Circuit(len(O.X3_WITNESS), 1), groth16.Circuit(len(O.X3_WITNESS), 1)
al, be, ga, _ = O.PF.R1CSToQAP(O.X3_R1CS_A, O.X3_R1CS_B, O.X3_R1CS_C)
proofs, gproofs, pubs = [], [], []
for i in range(nproofs):
    x = 3 + i
    out = x ** 3 + x + 5
    w = [1, out, x, x * x, x ** 3, x ** 3 + x, out, 1]
    px = O.PF.CombinePolynomials(w, al, be, ga)[3]
    proofs.append(snark.GenerateProofs(circ, pk, w, px))
    gproofs.append(groth16.GenerateProofsWithRS(gcirc, gpk, w, px, rng.randrange(1, R), rng.randrange(1, R)))
    pubs.append(out)
BAD = nproofs // 2

g1 = capi.g1_points_to_u64([vk.Vkb, vk.G1Kbg])
g2 = capi.g2_points_to_u64([vk.Vka, vk.Vkc, vk.G2Kbg, vk.G2Kg, vk.Vkz])
ic = capi.g1_points_to_u64(vk.IC)
pub = capi.ints_to_u64(pubs)
good = np.ascontiguousarray(np.stack([snark._proof_words(p) for p in proofs]))
bad = good.copy()
bad[BAD, 84:96] = capi.g1_points_to_u64([O.G1.Add(proofs[BAD].PiH, O.G1_GEN)])[0]
key = (capi.ptr64(g2[0]), capi.ptr64(g1[0]), capi.ptr64(g2[1]), capi.ptr64(g1[1]), capi.ptr64(g2[2]), capi.ptr64(g2[3]), capi.ptr64(g2[4]),
       capi.ptr64(ic), len(vk.IC))
gg1 = capi.g1_points_to_u64([gvk.G1_Alpha])
gg2 = capi.g2_points_to_u64([gvk.G2_Beta, gvk.G2_Gamma, gvk.G2_Delta])
gic = capi.g1_points_to_u64(gvk.IC)
ga_, gb_, gc_ = (capi.g1_points_to_u64([p.PiA for p in gproofs]), capi.g2_points_to_u64([p.PiB for p in gproofs]),
                 capi.g1_points_to_u64([p.PiC for p in gproofs]))
gkey = (capi.ptr64(gg1[0]), capi.ptr64(gg2[0]), capi.ptr64(gg2[1]), capi.ptr64(gg2[2]), capi.ptr64(gic), len(gvk.IC))
PARTS = ("total_ms", "h2d_ms", "poly_ms", "plan_ms", "accumulate_ms", "reduce_ms")


def each(words, want_bad):
    ok, failed, nbad = np.zeros(nproofs, dtype=np.intc), np.zeros(nproofs, dtype=np.intc), ctypes.c_uint64(0)
    t = time.perf_counter()
    capi.call("gs_pinocchio_verify_each", *key, capi.ptr64(pub), 1, capi.ptr64(words), nproofs, ok.ctypes.data_as(capi.intp),
              failed.ctypes.data_as(capi.intp), ctypes.byref(nbad))
    ms = (time.perf_counter() - t) * 1e3
    tm = capi.last_timing()
    assert nbad.value == len(want_bad) and [(i, int(failed[i])) for i in range(nproofs) if not ok[i]] == want_bad
    return (ms,) + tuple(tm[k] for k in PARTS)


def groth_each():
    ok, nbad = np.zeros(nproofs, dtype=np.intc), ctypes.c_uint64(0)
    t = time.perf_counter()
    capi.call("gs_groth16_verify_each", *gkey, capi.ptr64(pub), 1, capi.ptr64(ga_), capi.ptr64(gb_), capi.ptr64(gc_), nproofs,
              ok.ctypes.data_as(capi.intp), ctypes.byref(nbad))
    ms = (time.perf_counter() - t) * 1e3
    assert nbad.value == 0
    return ms


def host_loop():
    ok, failed = ctypes.c_int(0), ctypes.c_int(0)
    t = time.perf_counter()
    for i in range(SAMPLE):
        capi.call("gs_pinocchio_verify", *key, capi.ptr64(pub[i]), 1, capi.ptr64(good[i]), ctypes.byref(ok), ctypes.byref(failed))
        assert ok.value == 1
    return (time.perf_counter() - t) * 1e3


rows = {"good": [], "bad": [], "host": [], "groth": []}
for rep in range(REPS + 1):                                            # rep 0 warms everything up; the sides alternate
    r = (each(good, []), each(bad, [(BAD, 4)]), host_loop(), groth_each())
    if rep:
        for k, v in zip(rows, r):
            rows[k].append(v)
med = lambda xs: statistics.median(xs)   # noqa: E731
per_host = med(rows["host"]) / SAMPLE
lines = ["gs_pinocchio_verify_each over %d proofs of the x^3 + x + 5 key against gs_pinocchio_verify in a loop over %d of them, and beside" % (nproofs, SAMPLE),
         "gs_groth16_verify_each over %d Groth16 proofs of the same circuit, one process, alternating, medians of %d after a warm-up of all" % (nproofs, REPS),
         "  host loop   wall %9.2f ms   %8.2f us / proof, one core (the reference quantity, first measured here)" % (med(rows["host"]), per_host * 1e3)]
worst = 0.0
gw = med(rows["groth"])
for name, label in (("good", "all valid"), ("bad", "one invalid")):
    wall = med([r[0] for r in rows[name]])
    parts = [med([r[1 + k] for r in rows[name]]) for k in range(len(PARTS))]
    ratio = wall / nproofs / per_host
    worst = max(worst, ratio)
    lines += ["  each, %-11s wall %8.2f ms   (%s)   %7.2f us / proof   ratio to the host loop %.4f (1/%.1f)"
              % (label, wall, "  ".join("%.2f" % r[0] for r in rows[name]), wall / nproofs * 1e3, ratio, 1 / ratio),
              "      device %.2f ms: signals and lines up %.2f, membership %.2f, vkx and the two sums %.2f, Miller %.2f, final exponentiation %.2f;"
              % tuple(parts),
              "      host screening of the 8n points, uploads, key work and the fold (wall - device) %.2f" % max(wall - parts[0], 0.0),
              "      gs_groth16_verify_each over as many Groth16 proofs %.2f ms: Pinocchio / Groth16 = %.2f (recorded, not bounded; 4 to 5 was guessed)"
              % (gw, wall / gw)]
lines += ["  bound, set before any run: time per proof <= 1/16 of the host loop's (0.0625), the worse of the two batches: ratio %.4f (1/%.1f): %s"
          % (worst, 1 / worst, "MET" if worst <= 1 / 16 else "NOT MET"),
          "  kernels, code-object metadata: %s" % resource, ""]
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
