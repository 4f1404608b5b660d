"""gs_g2_subgroup_check against gs_g2_scale_powers, and circom.VerifyPtau with and without membership=True, timed in one process on one
GPU -- dev tool.

    python tools/time_g2_membership.py [power = 20] [profiles/g2_membership_timing.txt] ["resource-usage line of the kernel"]      (overwrites)

1. The tauG2 section of a generated transcript of 2^power (NewPtau + one ContributePtau with random secrets) is uploaded once.  After a
   warm-up of both, gs_g2_subgroup_check and gs_g2_scale_powers (random full-width c, t) alternate over the same points, REPS times each;
   the times are device times (gs_last_timing: HIP events around each call's kernels).  Yardstick, set before the kernel was measured: the
   membership test takes at most 0.5 x the scale's median -- by Fq2 products the scale is 256 doublings, 64 + 14 general additions and an
   inversion, about 3800; the test is 62 doublings, 23 mixed and 3 general additions and 3 psi, about 930 (0.25); a fixed scalar also
   costs no divergence, where the scale pays an addition whenever any lane's nibble is non-zero.
2. circom.VerifyPtau at that power with and without membership=True: wall and device milliseconds, REPS times each after a warm-up.
The third argument is copied into the file: the VGPR / scratch / occupancy figures of k_g2_subgroup from
hipcc -Rpass-analysis=kernel-resource-usage, which this tool cannot produce itself."""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi, circom  # noqa: E402

REPS = 5
power = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "g2_membership_timing.txt")
resource = sys.argv[3] if len(sys.argv) > 3 else "(not given)"
n = 1 << power
R = circom.R
rng = random.Random(21)
capi.init()
work = os.environ.get("TMPDIR", "/tmp")
src, path = os.path.join(work, "membership_new_%d.ptau" % power), os.path.join(work, "membership_%d.ptau" % power)
circom.NewPtau(src, power)
circom.ContributePtau(src, path, *(rng.randrange(1, R) for _ in range(3)))
os.remove(src)
tau2 = capi.g2_upload_affine_mont(circom.ReadPtau(path).tauG2)
c, t = (rng.randrange(R >> 1, R) for _ in range(2))                    # full width: 254 bits


def member():
    verdict = capi.g2_subgroup_check(tau2)
    return capi.last_timing()["total_ms"], verdict


def scale():
    h = capi.g2_scale_powers(tau2, 0, n, c, t)
    ms = capi.last_timing()["total_ms"]
    h.free()
    return ms, None


runs = {"gs_g2_subgroup_check": member, "gs_g2_scale_powers": scale}
samples = {name: [] for name in runs}
verdicts = set()
for rep in range(REPS + 1):                                            # rep 0 warms both up; the calls alternate
    for name, run in runs.items():
        ms, verdict = run()
        if rep:
            samples[name].append(ms)
        if verdict is not None:
            verdicts.add(verdict)
med = {name: statistics.median(v) for name, v in samples.items()}
ratio = med["gs_g2_subgroup_check"] / med["gs_g2_scale_powers"]
lines = ["gs_g2_subgroup_check against gs_g2_scale_powers over the 2^%d tauG2 points of a generated transcript, one process, device ms," % power,
         "alternating, %d repetitions each after a warm-up of both" % REPS]
for name, v in samples.items():
    lines.append("  %-24s median %9.2f ms   (%s)   %.1f ns / point" % (name, med[name], "  ".join("%.2f" % x for x in v), med[name] * 1e6 / n))
lines += ["  verdict of every call: %s" % sorted(verdicts, key=str),
          "  yardstick: membership <= 0.5 x scale: ratio %.3f: %s" % (ratio, "MET" if ratio <= 0.5 else "MISSED"),
          "  k_g2_subgroup, hipcc -Rpass-analysis=kernel-resource-usage: %s" % resource, ""]
tau2.free()

lines.append("circom.VerifyPtau at power %d (a %.0f MB file), %d repetitions each after a warm-up" % (power, os.path.getsize(path) / 1e6, REPS))
for membership in (False, True):
    rows = []
    for rep in range(REPS + 1):
        ms = {}
        t0 = time.perf_counter()
        ok = bool(circom.VerifyPtau(path, seed=rep, timing=ms, membership=membership))
        ms["outer_ms"] = (time.perf_counter() - t0) * 1e3
        assert ok
        if rep:
            rows.append(ms)
    m = lambda key: statistics.median(r.get(key, 0.0) for r in rows)      # noqa: E731
    lines.append("  membership=%-5s  wall %8.1f ms (%s)   gs_ptau_check device %6.2f ms   membership device %7.2f ms"
                 % (membership, m("wall_ms"), "  ".join("%.0f" % r["wall_ms"] for r in rows), m("total_ms"), m("membership_ms")))
lines.append("")
os.remove(path)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
