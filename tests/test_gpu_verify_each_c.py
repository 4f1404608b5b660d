"""-m gpu: tests/c/verify_each.c -- a process without Python asks gs_groth16_verify_each for a verdict per proof: the C call sequence of
gosnarkhip.Groth16VerifyEach (go/gosnarkhip/pairing_device.go).  For one mixed batch of 65 its verdict vector must be the one
groth16.VerifyProofsEach gives, and the host verifier's."""
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16, utils
import c_util
import golden_util as GU
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
N = 65


def test_verify_each_c_sequence_gives_the_python_verdicts(tmp_path):
    capi.init()
    rec = GU.load("groth_x3")
    opk = GU.groth_pk(rec["setup"])
    _, vk = utils.GrothSetupFromString(rec["setup"])
    circ = groth16.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = groth16.Pk(BACDelta=opk.BACDelta, Z=opk.Z, G1_Alpha=opk.G1_Alpha, G1_Beta=opk.G1_Beta, G1_Delta=opk.G1_Delta,
                    G1_At=opk.G1_At, G1_BACGamma=opk.G1_BACGamma, G2_Beta=opk.G2_Beta, G2_Delta=opk.G2_Delta,
                    G2_BACGamma=opk.G2_BACGamma, PowersTauDelta=opk.PowersTauDelta)
    rng = random.Random(12)
    proofs = [groth16.GenerateProofsWithRS(circ, pk, rec["w"], rec["px"], rng.randrange(1, O.R), rng.randrange(1, O.R)) for _ in range(N)]
    pubs = [[35] for _ in range(N)]
    for at in (0, 31, 63):
        proofs[at] = groth16.Proof(proofs[at].PiA, proofs[at].PiB, O.G1.Add(proofs[at].PiC, O.G1_GEN))
    proofs[64] = groth16.Proof(O.G1.Add(proofs[64].PiA, O.G1_GEN), proofs[64].PiB, proofs[64].PiC)
    pubs[17] = [36]
    want = groth16.VerifyProofsEach(vk, proofs, pubs)
    assert want == [i not in (0, 17, 31, 63, 64) for i in range(N)]
    head = np.array([len(vk.IC), 1, N], dtype=np.uint64)
    path = c_util._blob(str(tmp_path / "mixed.bin"), [head, capi.g1_points_to_u64([vk.G1_Alpha]), capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta]),
                                                      capi.g1_points_to_u64(vk.IC), capi.ints_to_u64([s[0] for s in pubs]),
                                                      capi.g1_points_to_u64([p.PiA for p in proofs]), capi.g2_points_to_u64([p.PiB for p in proofs]),
                                                      capi.g1_points_to_u64([p.PiC for p in proofs])])
    out = c_util.build_and_run("verify_each.c", [path], tmp_path)
    bits = "".join("1" if v else "0" for v in want)
    assert out == "device: %s (5 rejected)\nhost:   %s\n" % (bits, bits), out
