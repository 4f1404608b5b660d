"""Host instantiation of the slot plan of gs_groth16_verify_each_keys (csrc/verify_plan.h: proofs grouped by key, every key's run padded to
one-wave groups), compiled for the CPU: tests/host/verify_plan_host_test.hip compares it with a plan made the slow way."""
import subprocess

import hostbuild


def test_every_proof_has_one_slot_and_every_group_one_key():
    """Random key_of_proof over random npublic, all proofs on one key (1, 63, 64, 65, 127, 128, 129, 200 of them), one proof per key
    (in order, reversed, shuffled; up to 256 keys), counts 63, 64 and 65 side by side with a key that has none, sorted and interleaved,
    no proofs and no keys: every proof occupies exactly one slot, every group holds one key, the group count is the sum of
    ceil(c_k / 64), the order inside a key is the input order, the signal offsets are the running sums of npublic; a key index past
    the end is refused and named."""
    exe = hostbuild.build("verify_plan_host_test")
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("OK 252 cases, 64 lanes"), run.stdout + run.stderr
