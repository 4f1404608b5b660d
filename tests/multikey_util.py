"""Keys and proofs for the multi-key verifier tests (gs_groth16_verify_each_keys).  Test infrastructure.

x3_batch: proofs of the committed x^3 + x + 5 key (wasm_groth_x3.json) from the device prover, one witness x = 3 + i and one (r, s) per
proof, as tests/test_gpu_verify_each.py builds them (npublic 1).
DlogKey: a key from known discrete logs, alpha G1, beta G2, gamma G2, delta G2, IC_j = ic_j G1, whose valid proofs are A = a G1, B = b G2,
C = ((ab - alpha beta - gamma vkx) / delta) G1 with vkx = ic_0 + sum_j s_j ic_{j+1}.  With delta at infinity the pair (C, delta)
contributes one, C is free and a is solved for instead: a = (alpha beta + gamma vkx) / b; with gamma at infinity the vkx term is gone."""
import random

from gosnark_amd import capi, groth16, utils
import golden_util as GU
from oracle import ref_py as O

R, Q = O.R, O.Q


def g1_mul(k):
    return O.G1.MulScalar(O.G1_GEN, k % R)


def g2_mul(k):
    return O.G2.MulScalar(O.G2_GEN, k % R)


def g1_add(p, q):
    return O.G1.Add(p, q)


def x3_batch(n, seed=78):
    """-> (vk, n valid proofs, their public signal lists); needs an initialised device (the prover)."""
    capi.init()
    rec = GU.load("groth_x3")
    opk = GU.groth_pk(rec["setup"])
    _, vk = utils.GrothSetupFromString(rec["setup"])
    circ = groth16.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = groth16.Pk(BACDelta=opk.BACDelta, Z=opk.Z, G1_Alpha=opk.G1_Alpha, G1_Beta=opk.G1_Beta, G1_Delta=opk.G1_Delta,
                    G1_At=opk.G1_At, G1_BACGamma=opk.G1_BACGamma, G2_Beta=opk.G2_Beta, G2_Delta=opk.G2_Delta,
                    G2_BACGamma=opk.G2_BACGamma, PowersTauDelta=opk.PowersTauDelta)
    al, be, ga, _ = O.PF.R1CSToQAP(O.X3_R1CS_A, O.X3_R1CS_B, O.X3_R1CS_C)
    rng = random.Random(seed)
    proofs, pubs = [], []
    for i in range(n):
        x = 3 + i
        out = x ** 3 + x + 5
        w = [1, out, x, x * x, x ** 3, x ** 3 + x, out, 1]
        px = O.PF.CombinePolynomials(w, al, be, ga)[3]
        proofs.append(groth16.GenerateProofsWithRS(circ, pk, w, px, rng.randrange(1, R), rng.randrange(1, R)))
        pubs.append([out])
    return vk, proofs, pubs


class DlogKey:
    """A verification key whose discrete logs are known, and valid proofs for it."""

    def __init__(self, npublic, seed, delta_infinite=False, gamma_infinite=False):
        self.rng = random.Random(seed)
        self.npublic = npublic
        self.alpha, self.beta, self.gamma, self.delta = (self.rng.randrange(1, R) for _ in range(4))
        self.ics = [self.rng.randrange(1, R) for _ in range(npublic + 1)]
        self.delta_infinite, self.gamma_infinite = delta_infinite, gamma_infinite
        self.vk = groth16.Vk(IC=[g1_mul(k) for k in self.ics], G1_Alpha=g1_mul(self.alpha), G2_Beta=g2_mul(self.beta),
                             G2_Gamma=O.G2_ZERO if gamma_infinite else g2_mul(self.gamma),
                             G2_Delta=O.G2_ZERO if delta_infinite else g2_mul(self.delta))

    def signals(self):
        return [self.rng.choice((0, 1, R - 1, self.rng.randrange(R))) for _ in range(self.npublic)]

    def proof(self, sig=None):
        """-> (a valid groth16.Proof, its signals)"""
        sig = self.signals() if sig is None else list(sig)
        vkx = (self.ics[0] + sum(s * k for s, k in zip(sig, self.ics[1:]))) % R
        rhs = (self.alpha * self.beta + (0 if self.gamma_infinite else self.gamma * vkx)) % R
        a, b = self.rng.randrange(1, R), self.rng.randrange(1, R)
        if self.delta_infinite:
            a, c = rhs * pow(b, R - 2, R) % R, self.rng.randrange(1, R)
        else:
            c = (a * b - rhs) * pow(self.delta, R - 2, R) % R
        return groth16.Proof(g1_mul(a), g2_mul(b), g1_mul(c)), sig

    def proofs(self, n):
        both = [self.proof() for _ in range(n)]
        return [p for p, _ in both], [s for _, s in both]


def tamper(proof, signals, what):
    """One of the four kinds of change of test_exactly_the_tampered_positions_get_false -> (proof, signals).  "public" needs a signal."""
    signals = list(signals)
    if what == "A":
        proof = groth16.Proof(g1_add(proof.PiA, O.G1_GEN), proof.PiB, proof.PiC)
    elif what == "B":
        proof = groth16.Proof(proof.PiA, g2_mul(12345), proof.PiC)
    elif what == "C":
        proof = groth16.Proof(proof.PiA, proof.PiB, g1_add(proof.PiC, O.G1_GEN))
    else:
        signals[0] += 1
    return proof, signals


def host_verdicts(vks, key_of_proof, proofs, signals, only=None):
    """The yardstick: groth16.VerifyProof one proof at a time under the key its label names (for the positions in `only`, or all)."""
    at = range(len(proofs)) if only is None else sorted(only)
    return {i: groth16.VerifyProof(vks[key_of_proof[i]], proofs[i], signals[i]) for i in at}
