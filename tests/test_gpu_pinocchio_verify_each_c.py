"""-m gpu: tests/c/pinocchio_verify_each.c -- a process without Python asks gs_pinocchio_verify_each for a verdict and a failing equation
per proof: the C call sequence of gosnarkhip.PinocchioVerifyEach (go/gosnarkhip/pairing_device.go).  For one mixed batch of 65 the
digits it prints for the device must be the ones it prints for the host loop, and the ones snark.VerifyProofsEachChecks gives."""
import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, snark, utils
import c_util
import golden_util as GU
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
N = 65


def test_pinocchio_verify_each_c_sequence_gives_the_host_verdicts(tmp_path):
    capi.init()
    rec = GU.load("pinocchio_x3_setup")
    opk = GU.pinocchio_pk(rec["setup"])
    _, vk = utils.SetupFromString(rec["setup"])
    circ = snark.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = snark.Pk(G1T=opk.G1T, A=opk.A, B=opk.B, C=opk.C, Kp=opk.Kp, Ap=opk.Ap, Bp=opk.Bp, Cp=opk.Cp, Z=opk.Z)
    proof = snark.GenerateProofs(circ, pk, rec["w"], rec["px"])
    proofs, pubs = [proof] * N, [[35] for _ in range(N)]

    def moved(name):
        return snark.Proof(**{f: (O.G1.Add(getattr(proof, f), O.G1_GEN) if f == name else getattr(proof, f)) for f in snark.Proof.FIELDS})
    want = [0] * N
    for at, name, which in ((0, "PiAp", 1), (31, "PiBp", 2), (63, "PiCp", 3), (64, "PiH", 4), (40, "PiKp", 5)):
        proofs[at], want[at] = moved(name), which
    pubs[17], want[17] = [36], 4
    assert snark.VerifyProofsEachChecks(vk, proofs, pubs) == want
    assert snark.VerifyProofsEach(vk, proofs, pubs) == [w == 0 for w in want]
    head = np.array([len(vk.IC), 1, N], dtype=np.uint64)
    g1, g2 = capi.g1_points_to_u64, capi.g2_points_to_u64
    path = c_util._blob(str(tmp_path / "mixed.bin"), [head, g2([vk.Vka]), g1([vk.Vkb]), g2([vk.Vkc]), g1([vk.G1Kbg]), g2([vk.G2Kbg, vk.G2Kg, vk.Vkz]),
                                                      g1(vk.IC), capi.ints_to_u64([s[0] for s in pubs]),
                                                      np.concatenate([snark._proof_words(p) for p in proofs])])
    out = c_util.build_and_run("pinocchio_verify_each.c", [path], tmp_path)
    digits = "".join(str(w) for w in want)
    assert out == "device: %s (6 rejected)\nhost:   %s\n" % (digits, digits), out
