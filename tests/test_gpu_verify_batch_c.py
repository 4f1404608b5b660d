"""-m gpu: tests/c/verify_batch.c -- a process without Python verifies a batch of proofs with gs_groth16_verify_batch and multiplies
pairings with gs_pairing_product: the C call sequence of go/gosnarkhip/pairing_device.go.  Its verdicts must be the host verifier's."""
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16, utils
import c_util
import golden_util as GU
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
N = 66


def test_verify_batch_c_sequence_agrees_with_the_host_verifier(tmp_path):
    capi.init()
    rec = GU.load("groth_x3")
    opk = GU.groth_pk(rec["setup"])
    _, vk = utils.GrothSetupFromString(rec["setup"])
    circ = groth16.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = groth16.Pk(BACDelta=opk.BACDelta, Z=opk.Z, G1_Alpha=opk.G1_Alpha, G1_Beta=opk.G1_Beta, G1_Delta=opk.G1_Delta,
                    G1_At=opk.G1_At, G1_BACGamma=opk.G1_BACGamma, G2_Beta=opk.G2_Beta, G2_Delta=opk.G2_Delta,
                    G2_BACGamma=opk.G2_BACGamma, PowersTauDelta=opk.PowersTauDelta)
    rng = random.Random(11)
    proofs = [groth16.GenerateProofsWithRS(circ, pk, rec["w"], rec["px"], rng.randrange(1, O.R), rng.randrange(1, O.R)) for _ in range(N)]

    def blob(name, ps):
        head = np.array([len(vk.IC), 1, len(ps)], dtype=np.uint64)
        return c_util._blob(str(tmp_path / name), [head, capi.g1_points_to_u64([vk.G1_Alpha]), capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta]),
                                                   capi.g1_points_to_u64(vk.IC), capi.ints_to_u64([35] * len(ps)), capi.g1_points_to_u64([p.PiA for p in ps]),
                                                   capi.g2_points_to_u64([p.PiB for p in ps]), capi.g1_points_to_u64([p.PiC for p in ps]),
                                                   capi.ints_to_u64([rng.randrange(2, O.R)])])

    out = c_util.build_and_run("verify_batch.c", [blob("good.bin", proofs)], tmp_path)
    assert out == "batch of 66: ACCEPT; one at a time: 66 accepted\nproduct of 66 pairings: device not one, host not one\n", out
    bad = list(proofs)
    bad[65] = groth16.Proof(bad[65].PiA, bad[65].PiB, O.G1.Add(bad[65].PiC, O.G1_GEN))
    out = c_util.build_and_run("verify_batch.c", [blob("bad.bin", bad)], tmp_path)
    assert out == "batch of 66: REJECT; one at a time: 65 accepted\nproduct of 66 pairings: device not one, host not one\n", out
