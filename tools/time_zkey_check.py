"""SetupFromPtau, VerifyZkey and VerifyPtau on the same files in one process -- dev tool.

    python tools/time_zkey_check.py [k = 20] [profiles/zkey_check_timing.txt]      (appends)

The circuit and the transcript are those of tools/time_setup_ptau.py (same generator, same seed).  Reported: the setup's phases (its
timing=), then circom.VerifyZkey on a fresh upload of the key just written and circom.VerifyPtau on the transcript: the device
milliseconds of gs_groth16_key_check / gs_ptau_check (gs_last_timing: HIP events around the call's device work, and its plan, accumulate,
reduce and scalar phases) and the wall milliseconds of the whole Python call (parsing the three files, uploads, pairings).
The yardstick of the key check is the setup's transforms_ms OF THIS RUN: by operation count the check does about 1/50 of that group work,
and with a margin of 5 for plan building, the G2 sums and the pairings its device time is to be at most a tenth of it."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi, circom  # noqa: E402
from synth_circuit import write_r1cs  # noqa: E402

k, out_path = int(sys.argv[1]) if len(sys.argv) > 1 else 20, sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "zkey_check_timing.txt")
work = os.environ.get("TMPDIR", "/tmp")
r1cs, ptau, zkey = (os.path.join(work, "timing_%d.%s" % (k, e)) for e in ("r1cs", "ptau", "zkey"))
npub, nc, nw = write_r1cs(k, r1cs)
capi.init()
circom.WritePtau(ptau, k, 0x1234567890abcdef1234567890abcdef12345, 0xabcdef0123456789, 0x9876543210fedcba)
t2 = time.perf_counter()
ms = {}
key, system, vk = circom.SetupFromPtau(r1cs, ptau, zkey, timing=ms)
t3 = time.perf_counter()
del key, system, vk
capi.trim()
zt, pt = {}, {}
zrep = circom.VerifyZkey(r1cs, ptau, zkey, timing=zt)
capi.trim()
prep = circom.VerifyPtau(ptau, timing=pt)
phases = lambda t: "plans %.1f, accumulate %.1f, reduce %.1f, scalars %.1f" % (t["plan_ms"], t["accumulate_ms"], t["reduce_ms"], t["poly_ms"])      # noqa: E731
bound = ms["transforms_ms"] / 10
worst = max(("plan_ms", "accumulate_ms", "reduce_ms", "poly_ms"), key=lambda n: zt[n])
lines = ["k = %d: %d constraints, %d signals, nPublic = %d; circuit and transcript of tools/time_setup_ptau.py" % (k, nc, nw, npub),
         "  SetupFromPtau   transforms %10.1f ms   column sums %8.1f ms   (HIP events)   wall %10.1f ms" % (ms["transforms_ms"], ms["colsums_ms"], (t3 - t2) * 1e3),
         "  VerifyZkey      device     %10.1f ms   (%s)   wall %10.1f ms   %s" % (zt["total_ms"], phases(zt), zt["wall_ms"], "accepted" if zrep else "REJECTED: " + ", ".join(zrep.failed)),
         "  VerifyPtau      device     %10.1f ms   (%s)   wall %10.1f ms   %s" % (pt["total_ms"], phases(pt), pt["wall_ms"], "accepted" if prep else "REJECTED: " + ", ".join(prep.failed)),
         "  yardstick: VerifyZkey device <= transforms / 10 = %.1f ms: %s (%.1f x below the transforms)"
         % (bound, "MET" if zt["total_ms"] <= bound else "MISSED, the largest phase is %s" % worst, ms["transforms_ms"] / zt["total_ms"]),
         "  (device = HIP events around the whole call, host folds of the window sums between two sums included; the phases are the MSMs' own events)", ""]
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
for p in (r1cs, ptau, zkey):
    os.remove(p)
