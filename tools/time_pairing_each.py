"""gs_pairing_each against a loop of gs_pairing, timed in one process on one GPU -- dev tool.

    python tools/time_pairing_each.py [npairs = 4096] [profiles/pairing_each_timing.txt] ["resource-usage lines of the kernels"]      (overwrites)

npairs pairs (a_i G1, b_i G2) with random scalars come from gs_g1_fixed_base / gs_g2_fixed_base.  After a warm-up of both sides, REPS
rounds alternate
  * ONE gs_pairing_each call over all of them, values and flags downloaded (wall time of the C call, and the device times of its two
    kernels from gs_last_timing: accumulate_ms = Miller loops, reduce_ms = final exponentiations),
  * the yardstick, set before any run: gs_pairing in a loop over a sample of SAMPLE of the same pairs, on one core, and
  * gs_pairing_product over the same arrays (one value for all pairs; its ratio to gs_pairing_each is recorded, not bounded).
The bound is the one the batch verifier was held to: per pair the device takes at most 1/16 of the host loop -- a job on these machines
has 16 CPUs and a caller could spread the host loop over them.
The third argument is copied into the file: the register / LDS / scratch / occupancy figures of the kernels from
hipcc -Rpass-analysis=kernel-resource-usage, which this tool cannot produce itself."""
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi  # noqa: E402

REPS, SAMPLE = 5, 64
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
npairs = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "pairing_each_timing.txt")
resource = sys.argv[3] if len(sys.argv) > 3 else "(not given)"
rng = random.Random(41)
capi.init()

g1 = capi.g1_fixed_base(capi.ints_to_u64([rng.randrange(1, R) for _ in range(npairs)]))
g2 = capi.g2_fixed_base(capi.ints_to_u64([rng.randrange(1, R) for _ in range(npairs)]))
p, q = capi.g1_download(g1), capi.g2_download(g2)
assert capi.g2_subgroup_check(g2) == (0, None)


def each():
    t = time.perf_counter()
    vals, one = capi.pairing_each(g1, 0, g2, 0, npairs)
    ms = (time.perf_counter() - t) * 1e3
    tm = capi.last_timing()
    assert not one.any()
    return ms, tm["total_ms"], tm["accumulate_ms"], tm["reduce_ms"], vals


def host_loop(vals):
    out = np.zeros(48, dtype=np.uint64)
    rows = [(np.ascontiguousarray(p[i]), np.ascontiguousarray(q[i])) for i in range(SAMPLE)]
    t = time.perf_counter()
    for i, (a, b) in enumerate(rows):
        capi.call("gs_pairing", capi.ptr64(a), capi.ptr64(b), capi.ptr64(out))
        assert (out == vals[i]).all()
    return (time.perf_counter() - t) * 1e3


def product():
    t = time.perf_counter()
    capi.pairing_product(g1, 0, g2, 0, npairs)
    return (time.perf_counter() - t) * 1e3


rows = []
for rep in range(REPS + 1):                                            # rep 0 warms everything up; the sides alternate
    e = each()
    h = host_loop(e[4])
    pr = product()
    if rep:
        rows.append(e[:4] + (h, pr))
med = [statistics.median(r[k] for r in rows) for k in range(6)]
per_each, per_host = med[0] / npairs, med[4] / SAMPLE
ratio = per_each / per_host
lines = ["gs_pairing_each over %d pairs against gs_pairing in a loop over %d of them (every value compared) and gs_pairing_product over the same" % (npairs, SAMPLE),
         "arrays, one process, alternating, medians of %d after a warm-up of all three" % REPS,
         "  each       wall %9.2f ms   (%s)   %8.2f us / pair" % (med[0], "  ".join("%.2f" % r[0] for r in rows), per_each * 1e3),
         "             device %7.2f ms = Miller loops %.2f ms (%.2f us / pair) + final exponentiations %.2f ms (%.2f us / pair)"
         % (med[1], med[2], med[2] / npairs * 1e3, med[3], med[3] / npairs * 1e3),
         "  host loop  wall %9.2f ms   (%s)   %8.2f us / pair, one core" % (med[4], "  ".join("%.2f" % r[4] for r in rows), per_host * 1e3),
         "  bound, set before any run: time per pair <= 1/16 of the host loop's (0.0625): ratio %.4f (1/%.1f): %s"
         % (ratio, 1 / ratio, "MET" if ratio <= 1 / 16 else "NOT MET"),
         "  product    wall %9.2f ms   (%s)   %8.2f us / pair; each / product = %.2f (recorded, not bounded)"
         % (med[5], "  ".join("%.2f" % r[5] for r in rows), med[5] / npairs * 1e3, med[0] / med[5]),
         "  kernels, hipcc -Rpass-analysis=kernel-resource-usage: %s" % resource, ""]
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
