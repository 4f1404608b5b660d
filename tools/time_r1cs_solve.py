"""gs_r1cs_solve timed on the synthetic gates and sqchain circuits, in one process on one GPU -- dev tool.

    python tools/time_r1cs_solve.py [log2 n = 20] [profiles/r1cs_solve_timing.txt]      (overwrites)

1. BOUNDED (set before anything was measured): the device time of one solve of synth.gates_r1cs(2^log2 n) against
   gs_groth16_prove_witness on the same handles in the same run: no more than a quarter of the proof.
2. The two figures behind knobs.h's kSolveNarrow / kSolveRunMaxRows: one dependent row in k_solve_run (sqchain 2^16 and 2^12, one
   witness, all in runs) and one launch of a one-row level (the SAME 2^12 chain planned with narrow = 1: every level a launch of its
   own).  The C ABI has no way to enqueue a launch of an empty level, so the gap between two launches on the stream is taken as the
   difference of the two figures on that one chain: the same rows, once with and once without a launch boundary between them.
3. Recorded, not bounded: sqchain 2^log2 n at 1 and 64 witnesses, gates at 16 witnesses, the host time of gs_r1cs_solve_plan, the
   Python loop of synth.gates_r1cs for the same witness.
4. Registers, scratch and LDS of the two kernels: the compiler's own resource remarks for csrc/r1cs_solve.hip, compiled here with the
   library's flags (hipcc -Rpass-analysis=kernel-resource-usage; needs no device)."""
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi, groth16, r1csqap, synth  # noqa: E402

REPS = 3
log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r1cs_solve_timing.txt")
n, R = 1 << log2n, capi.R
med = statistics.median
lines = []


def say(text):
    lines.append(text)
    print(text, flush=True)


def timed_solve(plan, batch, reps=REPS):
    """-> (median poly_ms, median total_ms, handles of the last repetition); one warm-up"""
    poly, total, handles = [], [], None
    for rep in range(reps + 1):
        handles, report = plan.Solve(batch, handles)
        assert report, report
        t = capi.last_timing()
        if rep:
            poly.append(t["poly_ms"])
            total.append(t["total_ms"])
    return med(poly), med(total), handles


capi.init()
say("gs_r1cs_solve, one process, device ms of gs_last_timing (poly_ms = the launches of the solve, total_ms = with the copies), median of %d "
    "after a warm-up" % REPS)

# 1. gates against the proof
t0 = time.perf_counter()
inst = synth.gates_setup_instance(n, 0x5EED)
say("synth.gates_setup_instance(2^%d) (the Python witness loop, the setup, px): wall %.1f s" % (log2n, time.perf_counter() - t0))
t0 = time.perf_counter()
synth.gates_r1cs(n, 0x5EED)
say("synth.gates_r1cs(2^%d) alone, the host witness loop included: wall %.2f s" % (log2n, time.perf_counter() - t0))
pk, m = inst.device_pk(), inst.m
dev = r1csqap.DeviceR1CS(*inst.r1cs, m)
t0 = time.perf_counter()
plan = dev.PlanSolve([1])
say("gs_r1cs_solve_plan(gates 2^%d): wall %.2f s (reading the system back, the plan, the uploads); %r" % (log2n, time.perf_counter() - t0, plan.stats))
x = capi.u64_to_ints(inst.w_host[1:2])[0]
poly1, total1, hs = timed_solve(plan, [[x]])
assert (capi.scalars_download(hs[0]) == inst.w_host).all(), "the solved witness is not the generator's"
prove = []
for rep in range(REPS + 1):
    groth16.prove_from_witness(pk, dev, hs[0], 3, 4)
    if rep:
        prove.append(capi.last_timing()["total_ms"])
say("gates 2^%d, 1 witness: solve poly_ms %.3f total_ms %.3f; gs_groth16_prove_witness on the solved handle total_ms %.2f" % (log2n, poly1, total1, med(prove)))
say("  bound: the solve takes no more than a quarter of the proof: %.3f <= %.3f: %s" % (total1, med(prove) / 4, "MET" if total1 <= med(prove) / 4 else "NOT MET"))
rng_inputs = [[(x + 7 * b) % R] for b in range(16)]
poly16, total16, _ = timed_solve(plan, rng_inputs)
say("gates 2^%d, 16 witnesses: poly_ms %.3f total_ms %.3f = %.3f ms per witness" % (log2n, poly16, total16, total16 / 16))
del plan, hs

# 2. a dependent row, a launch
a, b, c, _ = synth.sqchain_r1cs(1 << 16, 5)
chain = r1csqap.DeviceR1CS(a, b, c, (1 << 16) + 1)
runs = chain.PlanSolve([1], 0, 0)
row_ms, _, _ = timed_solve(runs, [[5]])
rows = runs.stats["solved"]
say("sqchain 2^16, 1 witness, all in runs (%d launches): poly_ms %.2f = %.3f us per dependent row" % (runs.stats["launches"], row_ms, 1e3 * row_ms / rows))
a, b, c, _ = synth.sqchain_r1cs(1 << 12, 5)
small = r1csqap.DeviceR1CS(a, b, c, (1 << 12) + 1)
small_runs = small.PlanSolve([1], 0, 1 << 12)
small_ms, _, _ = timed_solve(small_runs, [[5]])
wide = small.PlanSolve([1], 1, 0)
launch_ms, _, _ = timed_solve(wide, [[5]])
per_launch = 1e3 * launch_ms / wide.stats["launches"]
per_row = 1e3 * small_ms / small_runs.stats["solved"]
say("sqchain 2^12, 1 witness, all in runs (%d launch): poly_ms %.2f = %.3f us per dependent row" % (small_runs.stats["launches"], small_ms, per_row))
say("sqchain 2^12, 1 witness, narrow = 1 (%d one-row launches): poly_ms %.2f = %.3f us per launch; less one row of the same chain: %.3f us "
    "between launches; ratio to a dependent row %.2f" % (wide.stats["launches"], launch_ms, per_launch, per_launch - per_row,
                                                         (per_launch - per_row) / per_row))
say("  rows that keep one run under 50 ms (at the 2^16 figure): %d" % int(50e3 / (1e3 * row_ms / rows)))

# 3. the chain at full size
a, b, c, w = synth.sqchain_r1cs(n, 5)
big = r1csqap.DeviceR1CS(a, b, c, n + 1)
t0 = time.perf_counter()
bp = big.PlanSolve([1])
say("gs_r1cs_solve_plan(sqchain 2^%d): wall %.2f s; %d launches" % (log2n, time.perf_counter() - t0, bp.stats["launches"]))
p1, _, h1 = timed_solve(bp, [[5]], reps=2)
assert (capi.scalars_download(h1[0]) == w).all()
p64, _, _ = timed_solve(bp, [[5 + i] for i in range(64)], reps=2)
say("sqchain 2^%d: 1 witness poly_ms %.1f; 64 witnesses poly_ms %.1f (x %.2f)" % (log2n, p1, p64, p64 / p1))

# 4. what the compiler says about the kernels
csrc = os.path.join(ROOT, "go-snark-study_amd", "csrc")
cc = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Rpass-analysis=kernel-resource-usage",
                     "-c", os.path.join(csrc, "r1cs_solve.hip"), "-o", os.devnull], capture_output=True, text=True)
found = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)",
                   cc.stderr, re.S)
for name, vgprs, scratch, occ, lds in found:
    kernel = re.search(r"k_solve_[a-z]+", name)
    if kernel and kernel.group(0) in ("k_solve_level", "k_solve_run"):
        say("%s: %s VGPRs, scratch %s bytes/lane, LDS %s bytes/block, occupancy %s waves/SIMD (hipcc's kernel-resource-usage remarks, gfx950, -O3)"
            % (kernel.group(0), vgprs, scratch, lds, occ))
if not found:
    say("kernel resources: hipcc gave no remarks (rc %d)" % cc.returncode)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
