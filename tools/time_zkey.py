"""Load and prove from a circuit.zkey, timed beside the same key in the proving_key.json shape -- dev tool.

    python tools/time_zkey.py [log2 of the domain = 20] > profiles/zkey_route.txt

The instance is tools/time_domain_witness.py's: the squaring chain over the domain 2^k, key from seeded toxic values.  It is written
twice: as circuit.zkey (circom.py's layout: affine Montgomery points, coefficient records, the coset basis E in section 9) and as the
limb container of circom.ProvingKeyToBinary with E inside (what the parent loads with UploadProvingKeyBinary).  Reported:
    load       file -> resident key + R1CS, both forms (different bytes: reported, not compared), and per zkey section the upload
               (staged copy + conversion kernel, or + the CSR build) beside a plain staged copy of the same number of bytes
    per proof  three tickets in flight, resident witnesses, window tables built beforehand (policy `always`), the zkey route (coset-only
               key, product system) and the parent's domain E route (key with hExps, three-matrix system) alternating in ONE process:
               median and min of 5 x 10 proofs after a warm-up.  The zkey route's work is a subset of the other's, so its median may
               exceed the parent's by no more than the parent's own max - min.
Both routes must return the same proof (checked)."""
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import gosnark_amd  # noqa: E402,F401
from gosnark_amd import capi, circom, groth16, r1csqap, synth, utils  # noqa: E402
import time_domain_witness as TDW  # noqa: E402

R, Q = groth16.R, circom.Q
MONT = 1 << 256


def mont_bytes(jac, coords):
    """[n, 3 * coords * 4] uint64 affine Jacobian limbs (x, y, 1 / all zero) -> the n x (2 * coords * 32) bytes of a zkey section"""
    n = jac.shape[0]
    raw = np.ascontiguousarray(jac[:, :2 * coords * 4]).astype("<u8").tobytes()
    out = bytearray(len(raw))
    for i in range(0, len(raw), 32):
        v = int.from_bytes(raw[i:i + 32], "little")
        if v:
            out[i:i + 32] = (v * MONT % Q).to_bytes(32, "little")
    assert len(out) == n * 2 * coords * 32
    return bytes(out)


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    capi.init()
    capi.set_table_policy("always")
    m = 1 << k
    n, nvars = m - 1, m + 1
    print("zkey route timing: domain 2^%d, n = 2^%d - 1 constraints, %d variables; %s" % (k, k, nvars, capi.version()))
    # ---- the instance (tools/time_domain_witness.py's scalars), its points by the fixed-base batches
    tau, alpha, beta, gamma, delta = synth.field_elems(5, 0x5EED)
    w = pow(5, (R - 1) >> k, R)
    xs, x = [], 1
    for _ in range(m):
        xs.append(x)
        x = x * w % R
    zt = (pow(tau, m, R) - 1) % R
    num = zt * pow(m, -1, R) % R
    L = [num * a % R * b % R for a, b in zip(xs, TDW.batch_inverse([(tau - a) % R for a in xs]))]
    at = [0] + L[:n] + [0]
    ct = [0, 0] + L[:n]
    dinv = pow(delta, -1, R)
    cd = [0, 0] + [((beta + alpha) * a + c) % R * dinv % R for a, c in zip(at[2:], ct[2:])]
    hexps, t = [], zt * dinv % R
    for _ in range(m + 1):
        hexps.append(t)
        t = t * tau % R
    g1 = lambda ks: capi.g1_fixed_base(capi.ints_to_u64(ks))                                      # noqa: E731
    h_at, h_cd, h_t = g1(at), g1(cd), g1(hexps)
    h_b2 = capi.g2_fixed_base(capi.ints_to_u64(at))
    p1 = capi.g1_tuples(capi.g1_download(g1([alpha, beta, delta])))
    p2 = capi.g2_tuples(capi.g2_download(capi.g2_fixed_base(capi.ints_to_u64([beta, delta, gamma]))))
    jdev = groth16.device_pk_from_handles(h_at, h_at, h_b2, h_cd, h_t, p1[0], p1[1], p1[2], p2[0], p2[1],
                                          capi.ints_to_u64([R - 1] + [0] * (m - 1) + [1]), nvars, 1)
    t_derive, _ = ms(lambda: circom.DeriveEvalBasis(jdev, k))
    print("gs_groth16_pk_derive_eval_domain (one-off, the parent's key only): %.1f ms" % t_derive)
    rows_ab = [{j + 1: 1} for j in range(n)]
    rows_c = [{j + 2: 1} for j in range(n)]
    csr_a, csr_c = r1csqap.csr_from_rows(rows_ab), r1csqap.csr_from_rows(rows_c)
    handles = []
    for x0 in synth.field_elems(4, 0x5EED + 1):
        wit = [1, x0]
        for _ in range(n):
            wit.append(wit[-1] * wit[-1] % R)
        handles.append(capi.scalars_upload(capi.ints_to_u64(wit)))
    # ---- the two files
    tmp = tempfile.mkdtemp(prefix="zkey_timing_")
    zpath, cpath = os.path.join(tmp, "circuit.zkey"), os.path.join(tmp, "key.bin")
    arr = {"A": capi.g1_download(h_at), "B2": capi.g2_download(h_b2), "C": capi.g1_download(h_cd), "T": capi.g1_download(h_t),
           "E": groth16._scheme.export_array(groth16._S, jdev, groth16.PK_ARRAYS["PowersTauDeltaEval"])}
    a_bytes = mont_bytes(arr["A"], 1)
    one = (MONT % R * MONT % R).to_bytes(32, "little")                     # the coefficient 1, times 2^512
    coefs = b"".join(struct.pack("<III", mat, j, j + 1) + one for mat in (0, 1) for j in range(n))
    head = struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<III", nvars, 1, m)
    head += b"".join(circom.G1ToZkey(p) if g == 1 else circom.G2ToZkey(p) for g, p in ((1, p1[0]), (1, p1[1]), (2, p2[0]), (2, p2[2]), (1, p1[2]), (2, p2[1])))
    body = {1: struct.pack("<I", 1), 2: head, 3: bytes(2 * 64), 4: struct.pack("<I", 2 * n) + coefs, 5: a_bytes, 6: a_bytes, 7: mont_bytes(arr["B2"], 2),
            8: mont_bytes(arr["C"][2:], 1), 9: mont_bytes(arr["E"], 1)}
    with open(zpath, "wb") as f:
        f.write(b"zkey" + struct.pack("<II", 1, len(body)))
        for sid, payload in body.items():
            f.write(struct.pack("<IQ", sid, len(payload)) + payload)
    sec = {"G1.At": arr["A"], "G1.BACGamma": arr["A"], "BACDelta": arr["C"], "PowersTauDelta": arr["T"], "G2.BACGamma": arr["B2"],
           "G1.ABD": capi.g1_points_to_u64(p1), "G2.BD": capi.g2_points_to_u64(p2[:2]), "Domain": np.array([[k, n, 0, 0]], dtype=np.uint64),
           circom.EVAL_SECTION: arr["E"]}
    for name, csr in zip("ABC", (csr_a, csr_a, csr_c)):
        sec["R1CS.%s.rowptr" % name] = csr[0].astype(np.uint64).reshape(-1, 1)
        sec["R1CS.%s.col" % name] = csr[1].astype(np.uint64).reshape(-1, 1)
        sec["R1CS.%s.val" % name] = csr[2].reshape(-1, 4)
    utils.WriteBinary(cpath, utils.PROTO_GROTH16, nvars, 1, sec)
    del arr, sec, body, coefs, a_bytes
    print("files: circuit.zkey %.1f MiB, limb container %.1f MiB" % (os.path.getsize(zpath) / 2 ** 20, os.path.getsize(cpath) / 2 ** 20))
    # ---- load
    for rep in range(3):                                                   # repetition 0 warms the page cache and the staging buffers
        t_c, (cdev, cr1cs) = ms(lambda: circom.UploadProvingKeyBinary(cpath))
        t_z, (zdev, zr1cs) = ms(lambda: circom.UploadZkey(zpath))
        if rep:
            print("load, file -> resident key + R1CS: zkey %.1f ms   limb container (parent) %.1f ms" % (t_z, t_c))
    z = circom.ReadZkey(zpath)
    for name, view, up in (("5 (A)", z.A, capi.g1_upload_affine_mont), ("7 (B2)", z.B2, capi.g2_upload_affine_mont), ("9 (H)", z.H, capi.g1_upload_affine_mont),
                           ("4 (coefficients)", z.coefs, lambda b: circom.DeviceZkeyR1CS(k, nvars, b))):
        plain = np.zeros((view.size + 31) // 32 * 4, dtype=np.uint64).reshape(-1, 4)
        best_up = min(ms(lambda: up(view))[0] for _ in range(3))
        best_copy = min(ms(lambda: capi.scalars_upload(plain))[0] for _ in range(3))
        print("  section %-18s %7.1f MiB: upload %.2f ms, a staged copy of as many bytes %.2f ms" % (name, view.size / 2 ** 20, best_up, best_copy))
    # ---- per proof
    jr1cs = circom.DeviceDomainR1CS(k, csr_a, csr_a, csr_c, nvars)
    capi.build_tables(jdev.handle, 2)
    capi.build_tables(zdev.handle, 2)
    r, s = synth.field_elems(2, 99)
    routes = {"zkey": (zdev, zr1cs), "domain E (parent)": (jdev, jr1cs)}
    times = {name: [] for name in routes}
    proofs = {}
    for rep in range(6):                                                   # repetition 0 warms both routes
        for name, (key, sys_) in routes.items():
            dt, proof = TDW.stream(key, sys_, handles, 10, r, s)
            assert capi.last_timing()["fallbacks"] == 0
            proofs[name] = (proof.PiA, proof.PiB, proof.PiC)
            if rep:
                times[name].append(dt / 10 * 1e3)
    assert proofs["zkey"] == proofs["domain E (parent)"], "the two routes disagree"
    for name, ts in times.items():
        print("%-18s ms per proof, three in flight: median %.3f   min %.3f   max %.3f   (5 x 10 proofs)" % (name, statistics.median(ts), min(ts), max(ts)))
    zt_, pt_ = times["zkey"], times["domain E (parent)"]
    over, allowed = statistics.median(zt_) - statistics.median(pt_), max(pt_) - min(pt_)
    print("zkey vs domain E: %+.3f ms at the median (%s the parent route's own max - min of %.3f ms); same proof" % (over, "within" if over <= allowed else "ABOVE", allowed))
    for p in (zpath, cpath):
        os.remove(p)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
