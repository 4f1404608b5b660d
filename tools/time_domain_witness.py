"""Witness -> proof with a key over a power-of-two domain (snarkjs / circom shape), timed beside the node-basis witness route -- dev tool.

    python tools/time_domain_witness.py [log2 of the domain = 20] > profiles/domain_witness.txt

A synthetic instance over the domain 2^k: the squaring chain s_j * s_j = s_(j+1), n = 2^k - 1 constraints with 3 non-zeros per row,
key built from seeded toxic values (scalars here in Python, points by the fixed-base batches).  Three tickets in flight, resident
witnesses, window tables built beforehand; per route the median of 5 repetitions of 10 proofs, with the repetitions' spread:
    domain E   the coset evaluation-basis route (three forward and three inverse transforms of size m, one point-wise kernel)
    domain px  the exact route of the same key (gs_set_eval_basis(0): px by transforms of size 2m, quotient by x^m - 1)
    nodes E    the node-basis evaluation route of a device-built key of the reference's shape at n = 2^k (synth.sqchain_setup_instance)
in ONE process, alternating, and the one-off time of gs_groth16_pk_derive_eval_domain.  The E route and the px route of the domain
key must return the same proof (checked)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gosnark_amd  # noqa: E402,F401
from gosnark_amd import capi, circom, groth16, r1csqap, synth  # noqa: E402

R = groth16.R


def batch_inverse(xs):
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * xs[i] % R
    return out


def domain_chain_instance(k, seed=0x5EED):
    """-> (DevicePk, DeviceDomainR1CS, [witness handles]) of the squaring chain over the domain 2^k"""
    m = 1 << k
    n = m - 1
    nvars = n + 2                                       # one, s_1 (public), s_2 .. s_(n+1)
    tau, alpha, beta, _, delta = synth.field_elems(5, seed)
    w = pow(5, (R - 1) >> k, R)
    xs, x = [], 1
    for _ in range(m):
        xs.append(x)
        x = x * w % R
    zt = (pow(tau, m, R) - 1) % R
    num = zt * pow(m, -1, R) % R
    L = [num * a % R * b % R for a, b in zip(xs, batch_inverse([(tau - a) % R for a in xs]))]      # L_j(tau)
    at = [0] + L[:n] + [0]                              # variable j (1..n) is the operand of row j - 1
    ct = [0, 0] + L[:n]                                 # variable j + 1 its product
    dinv = pow(delta, -1, R)
    cd = [0, 0] + [((beta + alpha) * a + c) % R * dinv % R for a, c in zip(at[2:], ct[2:])]
    hexps, t = [], zt * dinv % R
    for _ in range(m + 1):
        hexps.append(t)
        t = t * tau % R
    g1 = lambda ks: capi.g1_fixed_base(capi.ints_to_u64(ks))                                      # noqa: E731
    one = capi.g1_download(g1([alpha, beta, delta]))
    two = capi.g2_download(capi.g2_fixed_base(capi.ints_to_u64([beta, delta])))
    v1, v2 = capi.u64_to_ints(one), capi.u64_to_ints(two)
    p1 = [(v1[3 * i], v1[3 * i + 1], v1[3 * i + 2]) for i in range(3)]
    p2 = [((v2[6 * i], v2[6 * i + 1]), (v2[6 * i + 2], v2[6 * i + 3]), (v2[6 * i + 4], v2[6 * i + 5])) for i in range(2)]
    dev = groth16.device_pk_from_handles(g1(at), g1(at), capi.g2_fixed_base(capi.ints_to_u64(at)), g1(cd), g1(hexps), p1[0], p1[1], p1[2],
                                         p2[0], p2[1], capi.ints_to_u64([R - 1] + [0] * (m - 1) + [1]), nvars, 1)
    rows_ab = [{j + 1: 1} for j in range(n)]
    rows_c = [{j + 2: 1} for j in range(n)]
    a, c = r1csqap.csr_from_rows(rows_ab), r1csqap.csr_from_rows(rows_c)
    r1cs = circom.DeviceDomainR1CS(k, a, a, c, nvars)
    handles = []
    for x0 in synth.field_elems(4, seed + 1):
        wit = [1, x0]
        for _ in range(n):
            wit.append(wit[-1] * wit[-1] % R)
        handles.append(capi.scalars_upload(capi.ints_to_u64(wit)))
    return dev, r1cs, handles


def stream(dev, r1cs, handles, count, r, s):
    """count proofs through three tickets in flight -> (seconds, last proof)"""
    tickets, last = [], None
    t0 = time.perf_counter()
    for i in range(count):
        if len(tickets) == 3:
            last = groth16.prove_end(tickets.pop(0))
        tickets.append(groth16.prove_witness_begin(dev, r1cs, handles[i % len(handles)], r, s))
    while tickets:
        last = groth16.prove_end(tickets.pop(0))
    return time.perf_counter() - t0, last


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    capi.init()
    print("domain witness timing: domain 2^%d, n = 2^%d - 1 constraints, 3 non-zeros per row; %s" % (k, k, capi.version()))
    dev, r1cs, handles = domain_chain_instance(k)
    t0 = time.perf_counter()
    circom.DeriveEvalBasis(dev, k)
    print("gs_groth16_pk_derive_eval_domain (one-off): %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    node = synth.sqchain_setup_instance(1 << k, 0xBEEF)
    node_key, node_r1cs = node.device_pk(), r1csqap.DeviceR1CS(node.r1cs[0], node.r1cs[1], node.r1cs[2], node.m)
    node_w = [capi.scalars_upload(synth.sqchain_witness(1 << k, x)) for x in synth.field_elems(4, 77)]
    capi.build_tables(dev.handle, 0)
    capi.build_tables(node_key.handle, 0)
    r, s = synth.field_elems(2, 99)
    routes = {"domain E": (dev, r1cs, handles, True), "domain px": (dev, r1cs, handles, False), "nodes E": (node_key, node_r1cs, node_w, True)}
    times = {name: [] for name in routes}
    proofs = {}
    for rep in range(6):                                # repetition 0 warms every route (tables, spectra, workspaces)
        for name, (key, sys_, ws, ev) in routes.items():
            capi.set_eval_basis(ev)
            dt, proof = stream(key, sys_, ws, 10, r, s)
            assert capi.last_timing()["fallbacks"] == 0
            proofs[name] = (proof.PiA, proof.PiB, proof.PiC)
            if rep:
                times[name].append(dt / 10 * 1e3)
    capi.set_eval_basis(True)
    assert proofs["domain E"] == proofs["domain px"], "the two routes of the domain key disagree"
    for name, ts in times.items():
        print("%-10s ms per proof, three in flight: median %.3f   min %.3f   max %.3f   spread %.3f   (5 x 10 proofs)"
              % (name, statistics.median(ts), min(ts), max(ts), max(ts) - min(ts)))
    d, nd = statistics.median(times["domain E"]), statistics.median(times["nodes E"])
    spread = max(max(ts) - min(ts) for ts in (times["domain E"], times["nodes E"]))
    print("domain E vs nodes E: %+.3f ms (%s the run's spread of %.3f ms)" % (d - nd, "within" if d - nd <= spread else "ABOVE", spread))


if __name__ == "__main__":
    main()
