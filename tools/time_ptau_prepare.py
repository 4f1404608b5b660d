"""gs_g*_lagrange_levels against the level loop it replaces, and circom.PreparePtau / VerifyPtauPrepared / SetupFromPtau(prepared=True)
timed on one GPU -- dev tool.  Appends to profiles/ptau_prepare_timing.txt (or the path given last); one process per line below.

    python tools/time_ptau_prepare.py levels [REPS = 3] [path]
        The batched call gs_g1_lagrange_levels(P, 0, hi) / gs_g2_... against one gs_g1_lagrange / gs_g2_lagrange call per level
        0 .. hi on the same resident array of 2^hi random points, hi = 12, 16, 20: same process, the two alternating, after a warm-up of
        both; device time = HIP events around each call's device work (gs_last_timing), summed over the loop's calls; the wall clock
        around the blocking calls stands beside it.  At every size the two results are compared byte for byte.
    python tools/time_ptau_prepare.py file POWER [path]
        A transcript of 2^POWER from toxic values (circom.WritePtau): PreparePtau's wall time and phases, VerifyPtauPrepared's device and
        wall time (POWER <= 24), and at POWER = 20 SetupFromPtau() against SetupFromPtau(prepared=True) on tools/time_setup_ptau.py's
        synthetic circuit of 2^20."""
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi, circom  # noqa: E402

mode = sys.argv[1]
DEFAULT = os.path.join(ROOT, "profiles", "ptau_prepare_timing.txt")
lines = []


def levels_mode(reps):
    rng = random.Random(12)
    top = 20
    scalars = capi.ints_to_u64([rng.randrange(1, circom.R) for _ in range(1 << top)])
    lines.append("gs_g*_lagrange_levels(P, 0, hi) against one gs_g*_lagrange call per level 0 .. hi, 2^hi random points, one process, the two")
    lines.append("alternating, medians of %d after a warm-up of both; device ms = HIP events (gs_last_timing), summed over the loop's calls" % reps)
    lines.append("  %-4s %3s %16s %16s %8s   %s" % ("", "hi", "batched dev/wall", "loop dev/wall", "loop/bat", "device min .. max (batched | loop); same bytes"))
    for g2 in (False, True):
        fixed, batched, single, down = ((capi.g2_fixed_base, capi.g2_lagrange_levels, capi.g2_lagrange, capi.g2_download_affine_mont) if g2 else
                                        (capi.g1_fixed_base, capi.g1_lagrange_levels, capi.g1_lagrange, capi.g1_download_affine_mont))
        for hi in (12, 16, 20):
            pts = fixed(scalars[:1 << hi])

            def run_batched(keep=False):
                t0 = time.perf_counter()
                h = batched(pts, 0, hi)
                wall, dev = (time.perf_counter() - t0) * 1e3, capi.last_timing()["total_ms"]
                out = down(h) if keep else None
                h.free()
                return dev, wall, out

            def run_loop(keep=False):
                dev, t0, parts = 0.0, time.perf_counter(), []
                for p in range(hi + 1):
                    h = single(pts, p)
                    dev += capi.last_timing()["total_ms"]
                    if keep:
                        parts.append(down(h))
                    h.free()
                return dev, (time.perf_counter() - t0) * 1e3, parts

            _, _, a = run_batched(True)                                   # the warm-up of both is the comparison of their bytes
            _, _, b = run_loop(True)
            b = np.concatenate([x.reshape(-1) for x in b])
            same = a.size == b.size and bool((a.reshape(-1) == b).all())
            a = b = None
            sb, sl = [], []
            for _ in range(reps):
                sb.append(run_batched()[:2])
                sl.append(run_loop()[:2])
            med = lambda v, i: statistics.median(x[i] for x in v)      # noqa: E731
            lines.append("  %-4s %3d %7.1f /%7.1f %7.1f /%7.1f %7.2fx   %.1f .. %.1f | %.1f .. %.1f; %s"
                         % ("G2" if g2 else "G1", hi, med(sb, 0), med(sb, 1), med(sl, 0), med(sl, 1), med(sl, 0) / med(sb, 0),
                            min(x[0] for x in sb), max(x[0] for x in sb), min(x[0] for x in sl), max(x[0] for x in sl), "yes" if same else "NO"))
            pts.free()
    lines.append("")


def file_mode(power):
    work = os.environ.get("TMPDIR", "/tmp")
    src, dst = os.path.join(work, "timing_%d.ptau" % power), os.path.join(work, "timing_prepared_%d.ptau" % power)
    t0 = time.perf_counter()
    circom.WritePtau(src, power, 0x1234567890abcdef1234567890abcdef12345, 0xabcdef0123456789, 0x9876543210fedcba)
    write_s = time.perf_counter() - t0
    capi.trim()
    ms = {}
    circom.PreparePtau(src, dst, timing=ms)
    lines.append("circom.PreparePtau at power %d (a %.0f MB transcript from toxic values, written in %.1f s: a fixture): %.0f MB out, %d device calls"
                 % (power, os.path.getsize(src) / 1e6, write_s, os.path.getsize(dst) / 1e6, ms["calls"]))
    lines.append("  wall %8.0f ms = parse %.0f + upload %.0f + device %.0f + download %.0f + write %.0f (+ the rest);  library_bytes_max %.1f MB"
                 % (ms["wall_ms"], ms["parse_ms"], ms["upload_ms"], ms["device_ms"], ms["download_ms"], ms["write_ms"], ms["library_bytes_max"] / 1e6))
    if power <= 24:
        vt = {}
        rep = circom.VerifyPtauPrepared(dst, timing=vt)
        lines.append("circom.VerifyPtauPrepared at power %d: %s; device %.0f ms (four checks, HIP events), wall %.0f ms (parse, uploads, checks)"
                     % (power, rep, vt["device_ms"], vt["wall_ms"]))
    if power == 20:
        from synth_circuit import write_r1cs
        r1cs, za, zb = (os.path.join(work, "timing_prepare_20.%s" % e) for e in ("r1cs", "a.zkey", "b.zkey"))
        npub, nc, nw = write_r1cs(power, r1cs)
        rows = []
        for prepared in (False, True):
            capi.trim()
            t = {}
            t0 = time.perf_counter()
            out = circom.SetupFromPtau(r1cs, dst, zb if prepared else za, timing=t, prepared=prepared)
            rows.append(((time.perf_counter() - t0) * 1e3, t))
            out = None
        same = open(za, "rb").read() == open(zb, "rb").read()
        lines.append("SetupFromPtau, synthetic circuit of tools/time_setup_ptau.py: k = 20, %d constraints, %d signals; same .zkey bytes: %s" % (nc, nw, "yes" if same else "NO"))
        for name, (wall, t) in zip(("SetupFromPtau()", "SetupFromPtau(prepared=True)"), rows):
            lines.append("  %-30s wall %8.0f ms: transforms %8.1f ms, column sums %8.1f ms, records + downloads + writing %8.1f ms"
                         % (name, wall, t["transforms_ms"], t["colsums_ms"], t["write_ms"]))
        for p in (r1cs, za, zb):
            os.remove(p)
    lines.append("")
    for p in (src, dst):
        os.remove(p)


capi.init()
if mode == "levels":
    args = sys.argv[2:]
    reps = int(args[0]) if args and args[0].isdigit() else 3
    out_path = args[-1] if args and not args[-1].isdigit() else DEFAULT
    levels_mode(reps)
else:
    out_path = sys.argv[3] if len(sys.argv) > 3 else DEFAULT
    file_mode(int(sys.argv[2]))
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
