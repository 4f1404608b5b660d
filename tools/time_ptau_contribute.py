"""gs_g1_scale_powers / gs_g2_scale_powers and circom.ContributePtau, timed in one process on one GPU -- dev tool.

    python tools/time_ptau_contribute.py [log2 points = 20] [power = 20] [profiles/ptau_contribute_timing.txt]      (overwrites)

1. G1 rate against the only way the library had to multiply an array: gs_g1_scale (one scalar for the whole array, binary ladder) over
   the same 2^20 random points with a full-width scalar, in the same process, the calls alternating.  The new call multiplies every point
   by its own scalar c t^i (random full-width c, t).  gs_g1_scale sets no device timing, so both calls are timed by a host clock around
   the blocking call (it ends in a stream synchronise); the new call's device time (gs_last_timing: HIP events around series +
   multiplication) stands beside it.  Yardstick: the new call takes at most 1.10 x gs_g1_scale's time per point, by either clock (10 % =
   the run-to-run and box-to-box spread README.md records for one binary).
2. The G2 figure, recorded only: the library had no G2 scale.
3. The whole contribution at `power`: wall time of circom.ContributePtau on the transcript of ones, its phases (timing=) and the largest
   library_bytes seen, at slabs of 2^18 points and at the default slab (one slab per section up to power 21); gs_trim before each, so
   that the bytes are the contribution's own.
Every figure is the median of REPS repetitions after one warm-up of every shape."""
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
log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
power = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ptau_contribute_timing.txt")
n = 1 << log2n
R = circom.R
rng = random.Random(20)
capi.init()
scalars = capi.ints_to_u64([rng.randrange(1, R) for _ in range(n)])
g1, g2 = capi.g1_fixed_base(scalars), capi.g2_fixed_base(scalars)
del scalars
k, c, t = (rng.randrange(R >> 1, R) for _ in range(3))                 # full width: 254 bits


def timed(fn, *args):
    """-> (wall ms of the blocking call, device ms it reported)"""
    t0 = time.perf_counter()
    h = fn(*args)
    wall = (time.perf_counter() - t0) * 1e3
    dev = capi.last_timing()["total_ms"]
    h.free()
    return wall, dev


# faster and different is not faster: t = 1 gives the bytes of gs_g1_scale at the size that is timed
identical = bool((capi.g1_download_affine_mont(capi.g1_scale_powers(g1, 0, n, k, 1)) == capi.g1_download_affine_mont(capi.g1_scale(g1, k))).all())
runs = {"gs_g1_scale (binary ladder)": lambda: timed(capi.g1_scale, g1, k),
        "gs_g1_scale_powers": lambda: timed(capi.g1_scale_powers, g1, 0, n, c, t),
        "gs_g2_scale_powers": lambda: timed(capi.g2_scale_powers, g2, 0, n, c, t)}
samples = {name: [] for name in runs}
for rep in range(REPS + 1):                                            # rep 0 warms every shape up; the calls alternate
    for name, run in runs.items():
        if rep:
            samples[name].append(run())
        else:
            run()
wall = {name: statistics.median(w for w, _ in v) for name, v in samples.items()}
dev = {name: statistics.median(d for _, d in v) for name, v in samples.items()}
old, new_wall, new_dev = wall["gs_g1_scale (binary ladder)"], wall["gs_g1_scale_powers"], dev["gs_g1_scale_powers"]
met = new_wall <= 1.10 * old and new_dev <= 1.10 * old

lines = ["gs_g1_scale_powers / gs_g2_scale_powers over 2^%d random points, one process, medians of %d after a warm-up of every shape" % (log2n, REPS),
         "  %-30s %10s %10s   %s" % ("call", "wall ms", "device ms", "wall min .. max"),]
for name, v in samples.items():
    lines.append("  %-30s %10.2f %10s   %.2f .. %.2f     (%.1f ns / point)"
                 % (name, wall[name], "-" if "ladder" in name else "%.2f" % dev[name], min(w for w, _ in v), max(w for w, _ in v), wall[name] * 1e6 / n))
lines += ["  yardstick: gs_g1_scale_powers <= 1.10 x gs_g1_scale per point: wall / wall = %.3f, device / wall = %.3f: %s"
          % (new_wall / old, new_dev / old, "MET" if met else "MISSED"),
          "  t = 1 gives the bytes of gs_g1_scale at this size: %s" % ("yes" if identical else "NO"), ""]

# ---- the whole contribution ---------------------------------------------------------------------------------------------------------
g1 = g2 = None
work = os.environ.get("TMPDIR", "/tmp")
src, dst = os.path.join(work, "timing_new_%d.ptau" % power), os.path.join(work, "timing_out_%d.ptau" % power)
t0 = time.perf_counter()
circom.NewPtau(src, power)
new_ms = (time.perf_counter() - t0) * 1e3
lines.append("circom.ContributePtau at power %d: a %.0f MB file (NewPtau wrote it in %.0f ms), medians of %d after one warm-up"
             % (power, os.path.getsize(src) / 1e6, new_ms, REPS))
for slab in (18, 22):
    capi.trim()
    idle = capi.memory_query()["library_bytes"]
    rows = []
    for rep in range(REPS + 1):
        ms = {}
        circom.ContributePtau(src, dst, k, c, t, slab_log2=slab, timing=ms)
        if rep:
            rows.append(ms)
    med = lambda key: statistics.median(r[key] for r in rows)      # noqa: E731
    lines.append("  slab_log2 = %2d (%3d slabs): wall %8.0f ms = parse %.0f + upload %.0f + device %.0f + download %.0f + write %.0f (+ the rest);"
                 "  library_bytes_max %.1f MB (%.1f MB before the first call)"
                 % (slab, rows[0]["slabs"], med("wall_ms"), med("parse_ms"), med("upload_ms"), med("device_ms"), med("download_ms"), med("write_ms"),
                    max(r["library_bytes_max"] for r in rows) / 1e6, idle / 1e6))
lines += ["  (library_bytes_max is read after each slab's multiplication, input and output slab resident, and counts the upload's staging",
          "   scratch of one slab, which the context keeps: a G2 slab of 2^s points is 128 x 2^s bytes, a G1 slab half of that; the series of",
          "   one slab, 32 x 2^s bytes, and the download's conversion buffer of one slab are freed inside their calls)", ""]
for p in (src, dst):
    os.remove(p)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
