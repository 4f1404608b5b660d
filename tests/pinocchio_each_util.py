"""Pinocchio keys and proofs from known discrete logs, for the tests of gs_pinocchio_verify_each (test infrastructure, no test here).

Key:   Vka = k_a G2, Vkb = k_b G1, Vkc = k_c G2, G2Kg = gamma G2, G1Kbg = beta gamma G1, G2Kbg = beta gamma G2, Vkz = z G2, IC_j = u_j G1.
Proof: PiA = a G1, PiAp = k_a a G1, PiB = b G2, PiBp = k_b b G1, PiC = c G1, PiCp = k_c c G1, PiH = ((vkx + a) b - c) / z G1,
       PiKp = beta (vkx + a + b + c) G1, with vkx = u_0 + sum_j s_j u_{j+1}: all five equations of snark.VerifyProof hold."""
from oracle import ref_py as O

R = O.R
NAMES = ("PiA", "PiAp", "PiB", "PiBp", "PiC", "PiCp", "PiH", "PiKp")


def dlog_key(npublic, rng):
    k = {name: rng.randrange(1, R) for name in ("ka", "kb", "kc", "gamma", "beta", "z")}
    k["u"] = [rng.randrange(1, R) for _ in range(npublic + 1)]
    return k


def vkx_of(key, signals):
    return (key["u"][0] + sum(s * u for s, u in zip(signals, key["u"][1:]))) % R


def dlog_proof(key, signals, rng, a=None):
    """The exponents of a valid proof for these signals (any integers: the group law reduces them)."""
    vkx = vkx_of(key, signals)
    a = rng.randrange(1, R) if a is None else a % R
    b, c = rng.randrange(1, R), rng.randrange(1, R)
    return {"PiA": a, "PiAp": key["ka"] * a % R, "PiB": b, "PiBp": key["kb"] * b % R, "PiC": c, "PiCp": key["kc"] * c % R,
            "PiH": ((vkx + a) * b - c) * pow(key["z"], R - 2, R) % R, "PiKp": key["beta"] * (vkx + a + b + c) % R}


def equations(key, proof, signals):
    """The five equations as lists of (exponent in G1, exponent in G2) whose pairing product is one for a valid proof, in the
    device's order of pairs (include/gosnark_hip.h, gs_pinocchio_verify_each)."""
    vkx, bg = vkx_of(key, signals), key["beta"] * key["gamma"] % R
    p = proof
    return [[(p["PiA"], key["ka"]), (-p["PiAp"], 1)],
            [(key["kb"], p["PiB"]), (-p["PiBp"], 1)],
            [(p["PiC"], key["kc"]), (-p["PiCp"], 1)],
            [(vkx + p["PiA"], p["PiB"]), (-p["PiH"], key["z"]), (-p["PiC"], 1)],
            [(bg, p["PiB"]), (vkx + p["PiA"] + p["PiC"], bg), (-p["PiKp"], key["gamma"])]]


def g1(k):
    return O.G1.MulScalar(O.G1_GEN, k % R)


def g2(k):
    return O.G2.MulScalar(O.G2_GEN, k % R)


def vk_points(key):
    bg = key["beta"] * key["gamma"] % R
    return dict(IC=[g1(u) for u in key["u"]], Vka=g2(key["ka"]), Vkb=g1(key["kb"]), Vkc=g2(key["kc"]), G1Kbg=g1(bg), G2Kbg=g2(bg),
                G2Kg=g2(key["gamma"]), Vkz=g2(key["z"]))


def proof_points(proof):
    return {name: (g2 if name == "PiB" else g1)(proof[name]) for name in NAMES}
