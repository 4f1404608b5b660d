"""gs_g1_decompress / gs_g2_decompress against calls over the same points, and groth16.VerifyProofsEachCompressed against VerifyProofsEach,
timed in one process on one GPU -- dev tool.

    python tools/time_decompress.py [power = 20] [nproofs = 4096] [profiles/decompress_timing.txt] ["resource-usage lines of the kernels"]   (overwrites)

Every comparison alternates its two sides in this process, REPS times each after a warm-up of both.  The bounds were set from operation
counts before any run:
1. G1, 2^power points (random multiples of the generator, gs_g1_fixed_base): device time of gs_g1_decompress <= 0.25 x gs_g1_scale over
   the same points (about 330 field products against about 2 900).  gs_g1_scale reports no device time of its own: its figure is the
   host clock around the blocking call, which ends in a synchronise and moves no array between host and device.
2. G2, 2^power points: device time of gs_g2_decompress <= 1.0 x gs_g2_subgroup_check over the same points.
3. nproofs compressed proofs of the x^3 + x + 5 key through VerifyProofsEachCompressed <= 1.25 x VerifyProofsEach on the decompressed
   proofs (wall time of the Python calls, marshalling included on both sides).  DISTINCT proofs from the device prover are repeated to fill
   the batch: the verifier's work per proof does not depend on the proof.
4. Recorded, not bounded: the same proofs decompressed with Python integers (pow), gs_g*_compress at 2^power points.
The last argument is copied into the file: the register / LDS / scratch / occupancy figures of the kernels from
hipcc -Rpass-analysis=kernel-resource-usage, which this tool cannot produce itself."""
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
from gosnark_amd import capi, compressed, groth16, utils  # noqa: E402
from oracle import ref_py as O  # noqa: E402
import point_codec_util as P  # noqa: E402

REPS, DISTINCT = 5, 256
power = int(sys.argv[1]) if len(sys.argv) > 1 else 20
nproofs = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "decompress_timing.txt")
resource = sys.argv[4] if len(sys.argv) > 4 else "(not given)"
n = 1 << power
R = O.R
rng = random.Random(33)
capi.init()
med = statistics.median


def alternate(sides):
    """name -> f() -> ms; rep 0 warms every side up -> name -> [ms] * REPS"""
    samples = {name: [] for name in sides}
    for rep in range(REPS + 1):
        for name, run in sides.items():
            ms = run()
            if rep:
                samples[name].append(ms)
    return samples


def show(name, v, per):
    return "  %-24s median %9.3f ms   (%s)   %.1f ns / point" % (name, med(v), "  ".join("%.3f" % x for x in v), med(v) * 1e6 / per)


def wall(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


lines = []
scalars = np.frombuffer(random.Random(34).randbytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
scalars[:, 3] &= np.uint64((1 << 60) - 1)                                # below r
k = rng.randrange(R >> 1, R)                                             # full width: 254 bits
for g2 in (False, True):
    base = (capi.g2_fixed_base if g2 else capi.g1_fixed_base)(scalars)
    comp, decomp = (capi.g2_compress, capi.g2_decompress) if g2 else (capi.g1_compress, capi.g1_decompress)
    x, flags = comp(base)

    def run_decompress():
        h, ok = decomp(x, flags)
        ms = capi.last_timing()["total_ms"]
        assert ok.all()
        h.free()
        return ms

    def run_decompress_wall():
        return wall(lambda: decomp(x, flags)[0].free())

    def run_compress():
        comp(base)
        return capi.last_timing()["total_ms"]

    if g2:
        def run_other():
            verdict = capi.g2_subgroup_check(base)
            assert verdict == (0, None)
            return capi.last_timing()["total_ms"]
        other, bound = "gs_g2_subgroup_check", 1.0
    else:
        def run_other():
            return wall(lambda: capi.g1_scale(base, k).free())
        other, bound = "gs_g1_scale (host clock)", 0.25
    name = "gs_g2_decompress" if g2 else "gs_g1_decompress"
    s = alternate({name: run_decompress, other: run_other, name + " (host clock)": run_decompress_wall,
                   ("gs_g2_compress" if g2 else "gs_g1_compress"): run_compress})
    ratio = med(s[name]) / med(s[other])
    lines += ["%s against %s over the same 2^%d points, one process, device ms unless marked, alternating, %d repetitions each after a warm-up"
              % (name, other, power, REPS)]
    lines += [show(nm, v, n) for nm, v in s.items()]
    lines += ["  bound, set before any run: %s <= %.2f x %s: ratio %.3f: %s" % (name, bound, other, ratio, "MET" if ratio <= bound else "NOT MET"), ""]
    back, _ = decomp(x, flags)                                           # what was timed gives the array back
    x2, flags2 = comp(back)
    assert np.array_equal(x2, x) and np.array_equal(flags2, flags)
    back.free()
    base.free()
del scalars

# ---- end to end --------------------------------------------------------------------------------------------------------------------
with open(os.path.join(ROOT, "tests", "golden", "wasm_groth_x3.json")) as f:
    rec = json.load(f)
pk, vk = utils.GrothSetupFromString(json.loads(rec["setup"]))
circ = groth16.Circuit(len(O.X3_WITNESS), 1)
al, be, ga, _ = O.PF.R1CSToQAP(O.X3_R1CS_A, O.X3_R1CS_B, O.X3_R1CS_C)
distinct, dpubs = [], []
for i in range(min(DISTINCT, nproofs)):
    v = 3 + i
    out = v ** 3 + v + 5
    w = [1, out, v, v * v, v ** 3, v ** 3 + v, out, 1]
    distinct.append(groth16.GenerateProofsWithRS(circ, pk, w, O.PF.CombinePolynomials(w, al, be, ga)[3], rng.randrange(1, R), rng.randrange(1, R)))
    dpubs.append([out])
proofs = [distinct[i % len(distinct)] for i in range(nproofs)]
pubs = [dpubs[i % len(distinct)] for i in range(nproofs)]
codec = compressed.GNARK
dblobs = compressed.CompressProofs(distinct, codec)
blobs = [dblobs[i % len(distinct)] for i in range(nproofs)]


def run_compressed():
    t = time.perf_counter()
    got = groth16.VerifyProofsEachCompressed(vk, blobs, pubs, codec)
    ms = (time.perf_counter() - t) * 1e3
    assert all(got)
    return ms


def run_plain():
    t = time.perf_counter()
    got = groth16.VerifyProofsEach(vk, proofs, pubs)
    ms = (time.perf_counter() - t) * 1e3
    assert all(got)
    return ms


def run_parts():
    """where the front end's own time goes: the numpy decode, the two device calls (wall; device), the downloads"""
    rows = np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(-1, 128)
    t0 = time.perf_counter()
    d1 = compressed.DecodeG1(np.concatenate([rows[:, :32], rows[:, 96:]]), codec)
    d2 = compressed.DecodeG2(rows[:, 32:96], codec)
    t1 = time.perf_counter()
    h1, _ = capi.g1_decompress(*d1)
    dev1 = capi.last_timing()["total_ms"]
    t2 = time.perf_counter()
    h2, _ = capi.g2_decompress(*d2)
    dev2 = capi.last_timing()["total_ms"]
    t3 = time.perf_counter()
    capi.g1_download(h1)
    capi.g2_download(h2)
    t4 = time.perf_counter()
    return ((t1 - t0) * 1e3, (t2 - t1) * 1e3, dev1, (t3 - t2) * 1e3, dev2, (t4 - t3) * 1e3)


def run_python_ints():
    t = time.perf_counter()
    for b in blobs:
        rows = np.frombuffer(b, dtype=np.uint8)
        (xa, xc), (fa, fc) = compressed.DecodeG1(np.concatenate([rows[:32], rows[96:]]), codec)
        xb, fb = compressed.DecodeG2(rows[32:96], codec)
        va, vb, vc = capi.u64_to_ints(xa)[0], tuple(capi.u64_to_ints(xb)), capi.u64_to_ints(xc)[0]
        assert P.g1_point(va, fa & 1) and P.g2_point(vb, fb[0] & 1) and P.g1_point(vc, fc & 1)
    return (time.perf_counter() - t) * 1e3


s = alternate({"VerifyProofsEachCompressed": run_compressed, "VerifyProofsEach": run_plain})
ratio = med(s["VerifyProofsEachCompressed"]) / med(s["VerifyProofsEach"])
pr = [run_parts() for _ in range(REPS + 1)][1:]
pm = [med([r[i] for r in pr]) for i in range(6)]
py_ms = run_python_ints()
lines += ["groth16.VerifyProofsEachCompressed (%s) against groth16.VerifyProofsEach on the decompressed proofs, %d proofs (%d distinct ones repeated),"
          % (codec.name, nproofs, len(distinct)), "wall ms of the Python calls, alternating, %d repetitions each after a warm-up" % REPS]
lines += ["  %-28s median %9.2f ms   (%s)   %.2f us / proof" % (nm, med(v), "  ".join("%.2f" % x for x in v), med(v) * 1e3 / nproofs) for nm, v in s.items()]
lines += ["  bound, set before any run: compressed <= 1.25 x plain: ratio %.3f: %s" % (ratio, "MET" if ratio <= 1.25 else "NOT MET"),
          "  the front end's own steps: numpy decode %.2f ms; gs_g1_decompress over %d points %.2f ms wall (%.3f device); gs_g2_decompress over %d points"
          % (pm[0], 2 * nproofs, pm[1], pm[2], nproofs),
          "  %.2f ms wall (%.3f device); downloads of the two arrays %.2f ms" % (pm[3], pm[4], pm[5]),
          "  recorded, not bounded: the same %d proofs decompressed with Python integers (pow), one core: %.1f ms (%.1f us / proof)"
          % (nproofs, py_ms, py_ms * 1e3 / nproofs),
          "  kernels, hipcc -Rpass-analysis=kernel-resource-usage: %s" % resource, ""]
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
