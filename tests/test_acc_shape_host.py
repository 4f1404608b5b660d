"""Host instantiation of the accumulation launches' workgroup-size policy (csrc/acc_shape.h) and of the GS_ACC_GROUP_G1 / _G2
switches' parsing (csrc/knobs.h), compiled for the CPU: tests/host/acc_shape_host_test.hip walks the cross product of the policy's inputs."""
import subprocess

import hostbuild


def test_policy_answers_256_wherever_one_wave_groups_lost_and_a_legal_size_everywhere():
    """2 curves x 13 term counts (0, 1, 2^19 - 1, 2^19, 2^19 + 1, ..., 2^32 - 1) x route x caller x pipelined x no_poly x 6 job counts x
    multi-device = 4992 launches: the answer is 64, 128 or 256 in every one, and 256 for every launch below 2^19 terms, every blocking
    call, every plain MSM, every proof with a polynomial stage and every multi-device call.  A set switch (64 / 128 / 256) goes before
    the policy in every launch; 0 and eleven values it cannot take leave the policy's answer; the switches' text is parsed strictly."""
    exe = hostbuild.build("acc_shape_host_test")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK 4992 cases"), out.stdout + out.stderr
