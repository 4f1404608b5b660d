"""gs_r1cs_check timed on the synthetic sqchain circuit, in one process on one GPU -- dev tool.

    python tools/time_r1cs_check.py [log2 n = 20] [profiles/r1cs_check_timing.txt]      (overwrites)

The circuit is synth.sqchain_setup_instance(2^log2 n): a satisfying witness, and the same witness with one entry in the middle of the
chain replaced (it breaks the constraint that defines the entry and the one that squares it).
1. The check of both witnesses, alternating, REPS times each after a warm-up; device times of gs_last_timing.  Yardstick, set before
   anything was measured, from memory traffic (both phases are bandwidth-bound): flags, prefix sums and gather move at most about 110 B
   per row once; the values stage moves at least 68 B per matrix entry and 96 B per row written, with at least one entry per matrix
   and row.  So reduce_ms <= poly_ms of the same call.
2. Recorded without a yardstick: total_ms of the check beside total_ms of gs_groth16_prove_witness on the same handles; wall time of
   circom.CheckWtns from the two files; the steady three-in-flight rate of gs_groth16_prove_witness_begin / _end with and without a check
   issued before every submit; the device time a bad witness costs through GenerateProofsChecked (the check alone) and through
   gs_groth16_prove_witness (the evaluation-basis route, then the exact route)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi, circom, groth16, r1csqap, synth  # noqa: E402

REPS, STREAM = 5, 24
log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r1cs_check_timing.txt")
n, R = 1 << log2n, capi.R
capi.init()
inst = synth.sqchain_setup_instance(n, 0x5EED)
pk, m = inst.device_pk(), inst.m
dev = r1csqap.DeviceR1CS(*inst.r1cs, m)
bad_host = inst.w_host.copy()
bad_host[n // 2] = capi.ints_to_u64([(capi.u64_to_ints(bad_host[n // 2])[0] + 1) % R])[0]
good, bad = inst.w, capi.scalars_upload(bad_host)
r, s = 3, 4
med = statistics.median
lines = ["gs_r1cs_check on sqchain(2^%d): %d constraints, %d variables, one process, device ms of gs_last_timing," % (log2n, n, m),
         "%d repetitions each after a warm-up" % REPS]

# 1. the check itself
samples = {"satisfying": [], "one entry replaced": []}
counts = {}
for rep in range(REPS + 1):
    for name, h in (("satisfying", good), ("one entry replaced", bad)):
        count, rows, _ = capi.r1cs_check(dev, h, 16)
        t = capi.last_timing()
        counts[name] = (count, rows.tolist())
        if rep:
            samples[name].append((t["poly_ms"], t["reduce_ms"], t["total_ms"]))
assert counts["satisfying"][0] == 0 and counts["one entry replaced"] == (2, [n // 2 - 2, n // 2 - 1]), counts
met = True
for name, v in samples.items():
    poly, red, tot = (med(x[i] for x in v) for i in range(3))
    met = met and red <= poly
    lines.append("  %-20s violated %d   poly_ms (values stage) %7.3f   reduce_ms (flags, scan, gather) %7.3f   total_ms %7.3f   (%s)"
                 % (name, counts[name][0], poly, red, tot, "  ".join("%.3f/%.3f" % (x[0], x[1]) for x in v)))
lines += ["  yardstick: reduce_ms <= poly_ms of the same call: %s" % ("MET" if met else "NOT MET"), ""]
check_total = med(x[2] for x in samples["satisfying"])

# 2a. beside a proof from the same handles
prove = []
for rep in range(REPS + 1):
    groth16.prove_from_witness(pk, dev, good, r, s)
    if rep:
        prove.append(capi.last_timing()["total_ms"])
lines.append("gs_groth16_prove_witness on the same handles: total_ms %.2f (%s); the check is %.1f %% of it"
             % (med(prove), "  ".join("%.2f" % x for x in prove), 100 * check_total / med(prove)))

# 2b. a bad witness: refused by the check, or proved twice
groth16.prove_from_witness(pk, dev, bad, r, s)
bad_prove = []
for rep in range(REPS):
    groth16.prove_from_witness(pk, dev, bad, r, s)
    t = capi.last_timing()
    assert t["fallbacks"] == 1
    bad_prove.append(t["total_ms"])
refused = []
for rep in range(REPS):
    try:
        groth16.GenerateProofsChecked(None, pk, dev, bad_host, r, s)
        raise SystemExit("the bad witness was proved")
    except r1csqap.WitnessError:
        refused.append(capi.last_timing()["total_ms"])
lines.append("a witness that breaks a constraint: gs_groth16_prove_witness (both routes) total_ms %.2f (%s); GenerateProofsChecked refuses it "
             "after %.3f ms of device time (%s)" % (med(bad_prove), "  ".join("%.2f" % x for x in bad_prove), med(refused),
                                                    "  ".join("%.3f" % x for x in refused)))


# 2c. the steady stream, three in flight
def stream(checked):
    tickets, t0 = [], None
    for i in range(STREAM + 3):
        if i == 3:
            t0 = time.perf_counter()                        # the pipeline is full
        if checked:
            assert capi.r1cs_check(dev, good, 16)[0] == 0
        if len(tickets) == 3:
            groth16.prove_end(tickets.pop(0))
        tickets.append(groth16.prove_witness_begin(pk, dev, good, r, s))
    while tickets:
        groth16.prove_end(tickets.pop(0))
    return (time.perf_counter() - t0) * 1e3 / STREAM


stream(False)
rates = {c: [stream(c) for _ in range(3)] for c in (False, True)}
lines.append("stream of %d proofs, three in flight, wall ms per proof: without a check %.2f (%s); with a check before every submit %.2f (%s)"
             % (STREAM, med(rates[False]), "  ".join("%.2f" % x for x in rates[False]), med(rates[True]), "  ".join("%.2f" % x for x in rates[True])))

# 2d. from the two files
work = os.environ.get("TMPDIR", "/tmp")
r1cs_path, wtns_path = os.path.join(work, "r1cs_check_%d.r1cs" % log2n), os.path.join(work, "r1cs_check_%d.wtns" % log2n)
a, b, c = inst.r1cs
terms = lambda mat, j: [(int(mat[1][k]), int.from_bytes(mat[2][k].tobytes(), "little")) for k in range(int(mat[0][j]), int(mat[0][j + 1]))]  # noqa: E731
circom.WriteR1cs(r1cs_path, m, 0, 1, m - 2, [(terms(a, j), terms(b, j), terms(c, j)) for j in range(n)])
circom.WriteWtns(wtns_path, bad_host)
walls = []
for rep in range(3):
    t0 = time.perf_counter()
    report = circom.CheckWtns(r1cs_path, wtns_path)
    walls.append((time.perf_counter() - t0) * 1e3)
    assert report.rows == [n // 2 - 2, n // 2 - 1]
lines.append("circom.CheckWtns from a %.0f MB circuit.r1cs and a %.0f MB witness.wtns: wall %.0f ms (%s): parsing and uploads; %r"
             % (os.path.getsize(r1cs_path) / 1e6, os.path.getsize(wtns_path) / 1e6, med(walls), "  ".join("%.0f" % x for x in walls), report))
os.remove(r1cs_path)
os.remove(wtns_path)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
