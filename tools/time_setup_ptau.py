"""One timed circom.SetupFromPtau of a synthetic circuit -- dev tool.

    python tools/time_setup_ptau.py 16 profiles/setup_ptau_timing.txt      (appends; one process per size)

The circuit is tools/synth_circuit.py's (fan-in 2 per linear combination, 90 % of the coefficients in {1, r - 1}, 5 % below 2^16, 5 % of
251 bits, signal 0 in every row of A), the transcript is written from toxic values with circom.WritePtau.  Reported: the
five transforms and the four column sums by HIP events around each call's device work (SetupFromPtau's timing=), the records, downloads
and file writing by the wall clock, and gs_memory_query's library_bytes sampled between device calls.
GS_TIMING_DRY=1: the host half only (write and parse the circuit, build the records of section 4)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi, circom  # noqa: E402
from synth_circuit import write_r1cs  # noqa: E402

k, out_path = int(sys.argv[1]), sys.argv[2]
work = os.environ.get("TMPDIR", "/tmp")
t0 = time.perf_counter()
r1cs, ptau, zkey = (os.path.join(work, "timing_%d.%s" % (k, e)) for e in ("r1cs", "ptau", "zkey"))
npub, nc, nw = write_r1cs(k, r1cs)
t1 = time.perf_counter()
if os.environ.get("GS_TIMING_DRY"):                      # host half only: parse the file, build the records
    r = circom.ReadR1cs(r1cs)
    rec = circom._setup_records(r)
    print("dry: %d constraints, %d records, k = %d, write %.1f s, parse + records %.1f s" % (r.nConstraints, rec.size, circom._setup_domain_bits(r), t1 - t0, time.perf_counter() - t1))
    os.remove(r1cs)
    sys.exit(0)
capi.init()
circom.WritePtau(ptau, k, 0x1234567890abcdef1234567890abcdef12345, 0xabcdef0123456789, 0x9876543210fedcba)
t2 = time.perf_counter()
base = capi.memory_query()
ms = {}
key, system, vk = circom.SetupFromPtau(r1cs, ptau, zkey, timing=ms)
t3 = time.perf_counter()
mem = capi.memory_query()
m = 1 << k
lines = ["SetupFromPtau, synthetic circuit: k = %d, %d constraints, %d signals, %d records in section 4, nPublic = %d" % (k, nc, nw, ms["nCoefs"], npub),
         "  fan-in 2 per linear combination, 90 %% of the coefficients in {1, r - 1}, 5 % below 2^16, 5 % of 251 bits; signal 0 in every row of A",
         "  transforms (4 x G1, 1 x G2; HIP events)      %10.1f ms   (%d scalar multiplications each: m + (m/2) k)" % (ms["transforms_ms"], m + (m // 2) * k),
         "  column sums (3 x G1, 1 x G2; HIP events)     %10.1f ms" % ms["colsums_ms"],
         "  records, downloads, file writing (wall)      %10.1f ms   (%.1f MB zkey)" % (ms["write_ms"], os.path.getsize(zkey) / 1e6),
         "  SetupFromPtau wall, files parsed to key      %10.1f ms" % ((t3 - t2) * 1e3),
         "  (writing the r1cs %.1f s, the transcript from toxic values %.1f s: fixtures, not part of a setup)" % (t1 - t0, t2 - t1),
         "  device memory (gs_memory_query library_bytes): %.1f MB before, at most %.1f MB between two device calls, %.1f MB after (resident key + product system)"
         % (base["library_bytes"] / 1e6, ms["library_bytes_max"] / 1e6, mem["library_bytes"] / 1e6), ""]
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
for p in (r1cs, ptau, zkey):
    os.remove(p)
