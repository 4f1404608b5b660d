"""-m gpu: tests/c/verify_each_keys.c -- a process without Python prepares two verification keys and asks gs_groth16_verify_each_keys for a
verdict per proof: the C call sequence of gosnarkhip.Groth16VkCreate + Groth16VerifyEachKeys (go/gosnarkhip/pairing_device.go).  Two
known-log keys with three public inputs each and three proofs, one of them labelled with the other key: the verdicts must be the host
verifier's, one proof at a time under the key its label names."""
import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16
import c_util
import multikey_util as MK

pytestmark = pytest.mark.gpu


def test_verify_each_keys_c_sequence_gives_the_host_verdicts(tmp_path):
    dlog = [MK.DlogKey(3, 901), MK.DlogKey(3, 902)]
    made = [dlog[0].proof(), dlog[1].proof(), dlog[0].proof()]
    proofs, signals = [p for p, _ in made], [s for _, s in made]
    labels = [0, 1, 1]                                                  # the third proof belongs to key 0
    want = [groth16.VerifyProof(dlog[k].vk, p, s) for k, p, s in zip(labels, proofs, signals)]
    assert want == [True, True, False]
    parts = [np.array([2, 3], dtype=np.uint64)]
    for d in dlog:
        parts += [np.array([len(d.vk.IC)], dtype=np.uint64), capi.g1_points_to_u64([d.vk.G1_Alpha]),
                  capi.g2_points_to_u64([d.vk.G2_Beta, d.vk.G2_Gamma, d.vk.G2_Delta]), capi.g1_points_to_u64(d.vk.IC)]
    parts += [np.array(labels, dtype=np.uint64), capi.ints_to_u64([x for s in signals for x in s]),
              capi.g1_points_to_u64([p.PiA for p in proofs]), capi.g2_points_to_u64([p.PiB for p in proofs]),
              capi.g1_points_to_u64([p.PiC for p in proofs])]
    path = c_util._blob(str(tmp_path / "two_keys.bin"), parts)
    out = c_util.build_and_run("verify_each_keys.c", [path], tmp_path)
    bits = "".join("1" if v else "0" for v in want)
    assert out == "device: %s (1 rejected)\nhost:   %s\n" % (bits, bits), out
