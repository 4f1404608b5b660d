#!/usr/bin/env python
"""Wall time of gs_groth16_pk_derive_eval (the evaluation-basis array of a foreign key, derived on the device) at one size, beside
gs_groth16_pk_derive_quot on the same key and the key's blocking witness proof before and after.

A device setup key of n = 2^log2n constraints is rebuilt from its exported arrays (gs_groth16_pk_create: monomial-basis h array and
nothing else), the array is derived and compared with the one the setup emitted while it knew tau.

    python tools/time_eval_basis_derive.py --log2n 16

Prints one JSON line.  profiles/eval_basis_derive.txt holds the recorded runs; tools/derive_eval_basis.py is the naive cross-check
(n MSMs of n terms) this replaces."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gosnark_amd  # noqa: F401,E402
from gosnark_amd import capi, groth16, r1csqap, synth  # noqa: E402


def export(pk, which, count, words):
    a = np.zeros((count, words), dtype=np.uint64)
    capi.check(capi.load_library().gs_groth16_pk_export(capi.Handle(pk.handle.h), which, capi.ptr64(a), count))
    return a


def rebuilt(pk, m):
    """a key of the exported arrays of `pk` alone, without a trip through Python integers"""
    at, b1, cd = (capi.g1_upload(export(pk, w, m, 12)) for w in (0, 1, 3))
    b2 = capi.g2_upload(export(pk, 2, m, 24))
    pt = capi.g1_upload(export(pk, 4, m - 1, 12))
    singles = np.zeros(84, dtype=np.uint64)
    capi.check(capi.load_library().gs_groth16_pk_export(capi.Handle(pk.handle.h), 5, capi.ptr64(singles), 5))
    v = capi.u64_to_ints(singles)
    g1 = lambda o: (v[o], v[o + 1], v[o + 2])                                           # noqa: E731
    g2 = lambda o: ((v[o], v[o + 1]), (v[o + 2], v[o + 3]), (v[o + 4], v[o + 5]))       # noqa: E731
    return groth16.device_pk_from_handles(at, b1, b2, cd, pt, g1(0), g1(3), g1(6), g2(9), g2(15), export(pk, 6, m - 1, 4), m, 1)


def proof_ms(pk, dev, w, r, s, reps):
    for _ in range(3):
        p = groth16.prove_from_witness(pk, dev, w, r, s)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        p = groth16.prove_from_witness(pk, dev, w, r, s)
        t.append((time.perf_counter() - t0) * 1e3)
    return (p.PiA, p.PiB, p.PiC), statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=12)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    n = 1 << args.log2n
    capi.init(0)
    capi.set_table_policy("always")
    inst = synth.sqchain_setup_instance(n, 0xE7B1 + args.log2n)
    pk = inst.device_pk()
    want = export(pk, 7, n, 12)
    foreign = rebuilt(pk, inst.m)
    dev = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
    r, s = synth.field_elems(2, 0xE7B2)
    ref, _, _, _ = proof_ms(pk, dev, inst.w, r, s, 1)
    before = proof_ms(foreign, dev, inst.w, r, s, args.reps)
    t0 = time.perf_counter()
    groth16.DeriveQuotBasis(foreign)
    quot_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    groth16.DeriveEvalBasis(foreign, n)
    eval_s = time.perf_counter() - t0
    same = bool(np.array_equal(export(foreign, 7, n, 12), want))
    after = proof_ms(foreign, dev, inst.w, r, s, args.reps)
    print(json.dumps({"log2n": args.log2n, "derive_eval_s": round(eval_s, 4), "derive_quot_s": round(quot_s, 4), "equals_setup_array": same,
                      "witness_proof_ms_before": [round(x, 3) for x in before[1:]], "witness_proof_ms_after": [round(x, 3) for x in after[1:]],
                      "median_min_max_of": args.reps, "proofs_equal_setup_key": before[0] == ref and after[0] == ref, "table_policy": "always",
                      "version": capi.version()}))
    return 0 if same and before[0] == ref and after[0] == ref else 1


if __name__ == "__main__":
    sys.exit(main())
