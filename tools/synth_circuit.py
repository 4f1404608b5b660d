"""The synthetic circuit of the setup and key-check timing tools, written as circuit.r1cs with vectorised numpy: nc = 2^k - 9 constraints
(A w)(B w) = w_new with fan-in 2 per linear combination, 90 % of the coefficients in {1, r - 1}, 5 % below 2^16, 5 % of 251 bits, signal 0
in every row of A, one public input.  The generator is seeded with k: the same k gives the same file."""
import struct

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def write_r1cs(k, path):
    """-> (nPublic, nConstraints, nWires) of the circuit written to `path`; its setup domain is 2^k"""
    rng = np.random.default_rng(k)
    npub, nc = 1, (1 << k) - 2 - 7
    nw = 1 + npub + 1 + nc

    def coefs(n):
        u = rng.random(n)
        v = np.zeros((n, 4), dtype="<u8")
        rm1 = np.frombuffer((R - 1).to_bytes(32, "little"), dtype="<u8")
        v[u < 0.45, 0] = 1
        v[(u >= 0.45) & (u < 0.9)] = rm1
        small = (u >= 0.9) & (u < 0.95)
        v[small, 0] = rng.integers(2, 1 << 16, size=int(small.sum()), dtype=np.uint64)
        wide = u >= 0.95
        w = rng.integers(0, 1 << 62, size=(int(wide.sum()), 4), dtype=np.uint64)
        w[:, 3] &= (1 << 59) - 1
        v[wide] = w
        return v
    term = np.dtype([("wire", "<u4"), ("value", "<u8", (4,))])
    cons = np.dtype([("na", "<u4"), ("a", term, (2,)), ("nb", "<u4"), ("b", term, (2,)), ("nc", "<u4"), ("c", term, (1,))])
    assert cons.itemsize == 192
    body = np.zeros(nc, dtype=cons)
    body["na"], body["nb"], body["nc"] = 2, 2, 1
    new = 2 + npub + np.arange(nc, dtype=np.uint32)
    body["a"]["wire"][:, 0] = 0
    body["a"]["wire"][:, 1] = rng.integers(0, new, dtype=np.uint32)
    body["b"]["wire"][:, 0] = rng.integers(0, new, dtype=np.uint32)
    body["b"]["wire"][:, 1] = rng.integers(0, new, dtype=np.uint32)
    body["c"]["wire"][:, 0] = new
    body["a"]["value"] = coefs(2 * nc).reshape(nc, 2, 4)
    body["b"]["value"] = coefs(2 * nc).reshape(nc, 2, 4)
    body["c"]["value"][:, 0, 0] = 1
    head = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<IIIIQI", nw, 0, npub, 1, nw, nc)
    with open(path, "wb") as f:
        f.write(b"r1cs" + struct.pack("<II", 1, 2))
        f.write(struct.pack("<IQ", 1, len(head)) + head)
        f.write(struct.pack("<IQ", 2, body.nbytes))
        body.tofile(f)
    return npub, nc, nw
