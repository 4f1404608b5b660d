"""-m gpu: gs_groth16_vk_create / gs_groth16_verify_each_keys / groth16.VerifyProofsEachKeys -- a verdict per proof for proofs of many
verification keys in one call, one key per one-wave workgroup.

The yardstick for every verdict is the host verifier groth16.VerifyProof(vk_k, proof, signals), one proof at a time under the key the
proof's label names (pinned to the reference's recorded answers in tests/test_verifier.py); the new call is never compared with itself.
Keys (tests/multikey_util.py): 0 = the committed x^3 + x + 5 key with proofs from the device prover (npublic 1); 1, 2, 3 = known
discrete-log keys with npublic 0, 3 and 3; 4 = a known-log key (npublic 1) with delta at infinity, which puts a per-key skip flag next to
ordinary keys.  All shapes are <= 200 proofs."""
import ctypes
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, compressed, groth16
import membership_util as M
import multikey_util as MK
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R, Q = O.R, O.Q
COUNTS = (1, 65, 64, 2)             # proofs per key in the seam tests: a partial group, a full group plus one, exactly one group


@pytest.fixture(autouse=True)
def _init():
    capi.init()


@pytest.fixture(scope="module")
def zoo():
    """vks[k], keys[k] (prepared), pool[k] = (proofs, signals): valid proofs of key k, each accepted by the host for its own key."""
    capi.init()
    x3_vk, x3_proofs, x3_pubs = MK.x3_batch(66)
    dlog = [MK.DlogKey(0, 700), MK.DlogKey(3, 701), MK.DlogKey(3, 702), MK.DlogKey(1, 703, delta_infinite=True)]
    vks = [x3_vk] + [d.vk for d in dlog]
    pool = [(x3_proofs, x3_pubs)] + [d.proofs(n) for d, n in zip(dlog, (65, 64, 8, 4))]      # as many as the largest set below takes
    for vk, (proofs, sigs) in zip(vks, pool):
        assert all(groth16.VerifyProof(vk, p, s) for p, s in zip(proofs[:2], sigs[:2]))
    assert groth16.VerifyProof(vks[4], *MK.tamper(pool[4][0][0], pool[4][1][0], "C"))       # delta at infinity: C is free, on the host too
    assert not groth16.VerifyProof(vks[4], *MK.tamper(pool[4][0][0], pool[4][1][0], "A"))
    keys = [groth16.PrepareVerificationKey(vk) for vk in vks]
    assert [k.npublic for k in keys] == [1, 0, 3, 3, 1]
    return vks, keys, pool


def seam_set(zoo, which=(0, 1, 2, 4), counts=COUNTS, seed=5):
    """counts[j] proofs of key which[j], interleaved by a fixed permutation (never sorted) -> key_of_proof, proofs, signals, runs: the
    positions of every key's proofs in input order."""
    vks, keys, pool = zoo
    items = [(k, pool[k][0][i], pool[k][1][i]) for k, c in zip(which, counts) for i in range(c)]
    random.Random(seed).shuffle(items)
    kop = [k for k, _, _ in items]
    assert kop != sorted(kop)
    runs = {k: [i for i, kk in enumerate(kop) if kk == k] for k in which}
    return kop, [p for _, p, _ in items], [list(s) for _, _, s in items], runs


def seam_positions(runs):
    """Per key, the positions that land in the first and last slot of every group and at the run's end."""
    spots = set()
    for at in runs.values():
        for g in range(0, len(at), 64):
            spots |= {at[g], at[min(g + 63, len(at) - 1)]}
        spots.add(at[-1])
    return sorted(spots)


def test_group_seams_all_valid(zoo):
    vks, keys, _ = zoo
    kop, proofs, signals, runs = seam_set(zoo)
    assert sorted(len(v) for v in runs.values()) == sorted(COUNTS) and len(proofs) == 132
    assert groth16.VerifyProofsEachKeys(keys, kop, proofs, signals) == [True] * len(proofs)


def test_tampering_at_the_seams(zoo):
    vks, keys, _ = zoo
    kop, base, base_sig, runs = seam_set(zoo)
    spots = seam_positions(runs)
    assert len(spots) == 1 + 3 + 2 + 2                                   # 1: one slot; 65: 0, 63, 64; 64: 0, 63; 2: 0, 1
    kinds = ("A", "B", "C", "public")
    for shift in range(len(kinds)):                                     # every kind of change visits every position
        proofs, signals = list(base), [list(s) for s in base_sig]
        for j, at in enumerate(spots):
            what = kinds[(j + shift) % len(kinds)]
            if what == "public" and not signals[at]:
                what = "A"                                              # a key without public inputs has no signal to change
            proofs[at], signals[at] = MK.tamper(base[at], base_sig[at], what)
        got = groth16.VerifyProofsEachKeys(keys, kop, proofs, signals)
        host = MK.host_verdicts(vks, kop, proofs, signals, only=spots)
        assert sum(1 for v in host.values() if not v) >= len(spots) - 2  # (only a changed C under the infinite delta stays valid)
        for i in range(len(proofs)):
            assert got[i] == (host[i] if i in host else True), (shift, i)


def test_key_confusion(zoo):
    """The test the feature exists for: keys 2 and 3 both take three signals."""
    vks, keys, pool = zoo
    n = 10
    kop = [2, 3] * (n // 2)
    proofs = [pool[k][0][i // 2] for i, k in enumerate(kop)]
    signals = [pool[k][1][i // 2] for i, k in enumerate(kop)]
    assert groth16.VerifyProofsEachKeys(keys, kop, proofs, signals) == [True] * n
    wrong = list(kop)
    wrong[4], wrong[7] = 3, 2                                            # a proof of key 2 labelled 3, a proof of key 3 labelled 2
    host = MK.host_verdicts(vks, wrong, proofs, signals)
    assert [host[i] for i in range(n)] == [i not in (4, 7) for i in range(n)]
    assert groth16.VerifyProofsEachKeys(keys, wrong, proofs, signals) == [host[i] for i in range(n)]
    assert groth16.VerifyProofsEachKeys(keys, kop, proofs, signals) == [True] * n          # relabelled correctly
    swapped = [list(s) for s in signals]
    swapped[0], swapped[2] = signals[2], signals[0]                      # proofs of key 2 with another proof's signals
    host = MK.host_verdicts(vks, kop, proofs, swapped)
    assert not host[0] and not host[2]
    assert groth16.VerifyProofsEachKeys(keys, kop, proofs, swapped) == [host[i] for i in range(n)]


def _raw(keys, kop, proofs, signals, nbad=True):
    flat = [int(x) for s in signals for x in s]
    pub = capi.ints_to_u64(flat) if flat else np.zeros((1, 4), dtype=np.uint64)
    a, b, c = groth16._proof_words(proofs)
    kk = np.array(kop, dtype=np.uint32)
    ok, bad = np.full(len(proofs), 7, dtype=np.intc), ctypes.c_uint64(77)
    rc = capi.load_library().gs_groth16_verify_each_keys(capi.harr(keys), len(keys), capi.ptr32(kk), capi.ptr64(pub), capi.ptr64(a), capi.ptr64(b),
                                                         capi.ptr64(c), len(proofs), ok.ctypes.data_as(capi.intp), ctypes.byref(bad) if nbad else None)
    return rc, [int(x) for x in ok], bad.value


def test_handle_cases(zoo):
    vks, keys, pool = zoo
    proofs = [pool[2][0][0], pool[0][0][0], pool[2][0][1]]
    signals = [pool[2][1][0], pool[0][1][0], pool[2][1][1]]
    # the same handle twice in keys (0 and 2 are the x^3 key), a key with no proofs (1)
    four = [keys[0], keys[3], keys[0], keys[2]]
    assert _raw(four, [3, 2, 3], proofs, signals) == (0, [1, 1, 1], 0)
    assert _raw(four, [3, 0, 3], proofs, signals) == (0, [1, 1, 1], 0)
    assert _raw(four, [3, 0, 3], proofs, signals, nbad=False)[:2] == (0, [1, 1, 1])
    # key_of_proof[i] = nkeys
    assert _raw(four, [3, 4, 3], proofs, signals) == (-3, [7, 7, 7], 77)
    assert b"key_of_proof[1]" in capi.load_library().gs_last_error()
    # a key handle of another kind, and one that never existed
    other = capi.g1_upload(capi.g1_points_to_u64([O.G1_GEN]))
    assert _raw([keys[0], other, keys[0], keys[2]], [3, 0, 3], proofs, signals) == (-3, [7, 7, 7], 77)
    assert b"keys[1]" in capi.load_library().gs_last_error()
    other.free()
    assert _raw([keys[0], 0x00ffffffffffff, keys[0], keys[2]], [3, 0, 3], proofs, signals) == (-3, [7, 7, 7], 77)
    with pytest.raises(ValueError, match="proof 1"):
        groth16.VerifyProofsEachKeys(four, [3, 0, 3], proofs, [signals[0], [], signals[2]])
    assert groth16.VerifyProofsEachKeys(four, [], [], []) == []


def test_bad_proof_points_in_both_strict_settings(zoo):
    vks, keys, _ = zoo
    kop, base, base_sig, runs = seam_set(zoo, which=(0, 2, 3), counts=(66, 5, 3), seed=9)
    x3, k2 = runs[0], runs[2]
    proofs, signals = list(base), [list(s) for s in base_sig]
    off, inf_a, inf_c, tw1, tw2, alias = x3[0], x3[63], x3[64], x3[65], k2[0], k2[4]
    x, y, z = base[off].PiA
    proofs[off] = groth16.Proof((x, (y + 1) % Q, z), base[off].PiB, base[off].PiC)                  # an A off its curve
    proofs[inf_a] = groth16.Proof(O.G1_ZERO, base[inf_a].PiB, base[inf_a].PiC)                      # an infinite A
    proofs[inf_c] = groth16.Proof(base[inf_c].PiA, base[inf_c].PiB, O.G1_ZERO)                      # an infinite C
    outside = (M.twist_points(1)[0], M.complete_add(M.jac(O.G2.Affine(base[tw2].PiB)), M.small_order_point()))
    for at, b in zip((tw1, tw2), outside):                                                          # a B on the twist outside G2
        assert not M.in_subgroup(b)
        proofs[at] = groth16.Proof(base[at].PiA, b, base[at].PiC)
    x, y, z = base[alias].PiA
    proofs[alias] = groth16.Proof((x + Q, y, z), base[alias].PiB, base[alias].PiC)                  # one non-canonical coordinate
    bad = {off, inf_a, inf_c, tw1, tw2}
    lib = capi.load_library()
    for strict in (0, 1):
        try:
            assert lib.gs_verify_set_strict(strict) == 0
            host = MK.host_verdicts(vks, kop, proofs, signals, only=bad | {alias})
            rc, got, nbad = _raw(keys, kop, proofs, signals)
        finally:
            lib.gs_verify_set_strict(0)
        assert all(host[i] is False for i in bad) and host[alias] is (strict == 0)
        assert rc == 0 and got == [int(host.get(i, True)) for i in range(len(proofs))]
        assert nbad == len(bad) + strict


def test_one_key_only_equals_verify_proofs_each(zoo):
    vks, keys, pool = zoo
    d = MK.DlogKey(3, 811)
    proofs, signals = d.proofs(130)
    for at, what in ((0, "A"), (63, "public"), (64, "C"), (65, "B"), (129, "public")):
        proofs[at], signals[at] = MK.tamper(proofs[at], signals[at], what)
    want = [i not in (0, 63, 64, 65, 129) for i in range(130)]
    for i, host in MK.host_verdicts([d.vk], [0] * 130, proofs, signals, only=(0, 63, 64, 65, 129)).items():
        assert host == want[i], i
    assert groth16.VerifyProofsEach(d.vk, proofs, signals) == want
    key = groth16.PrepareVerificationKey(d.vk)
    assert groth16.VerifyProofsEachKeys([key], [0] * 130, proofs, signals) == want
    key.handle.free()


def _vk_create(vk, nic=None):
    g2 = capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta])
    a, ic = capi.g1_points_to_u64([vk.G1_Alpha]), capi.g1_points_to_u64(vk.IC)
    out = capi.Handle(77)
    rc = capi.load_library().gs_groth16_vk_create(capi.ptr64(a), capi.ptr64(g2[0]), capi.ptr64(g2[1]), capi.ptr64(g2[2]), capi.ptr64(ic),
                                                  len(vk.IC) if nic is None else nic, ctypes.byref(out))
    return rc, out.value, capi.load_library().gs_last_error()


def test_key_refusals(zoo):
    vks, _, _ = zoo
    vk = vks[2]
    before = capi.alloc_counters()
    ax, ay, az = vk.G1_Alpha
    bad = groth16.Vk(IC=vk.IC, G1_Alpha=(ax, (ay + 1) % Q, az), G2_Beta=vk.G2_Beta, G2_Gamma=vk.G2_Gamma, G2_Delta=vk.G2_Delta)
    rc, h, msg = _vk_create(bad)
    assert (rc, h) == (-3, 77) and b"alpha" in msg
    ix, iy, iz = vk.IC[2]
    bad = groth16.Vk(IC=[vk.IC[0], vk.IC[1], (ix, (iy + 1) % Q, iz), vk.IC[3]], G1_Alpha=vk.G1_Alpha, G2_Beta=vk.G2_Beta, G2_Gamma=vk.G2_Gamma,
                     G2_Delta=vk.G2_Delta)
    rc, h, msg = _vk_create(bad)
    assert (rc, h) == (-3, 77) and b"IC[2]" in msg
    gx, gy, gz = vk.G2_Gamma
    bad = groth16.Vk(IC=vk.IC, G1_Alpha=vk.G1_Alpha, G2_Beta=vk.G2_Beta, G2_Gamma=(gx, (gy[0], (gy[1] + 1) % Q), gz), G2_Delta=vk.G2_Delta)
    rc, h, msg = _vk_create(bad)
    assert (rc, h) == (-3, 77) and b"gamma" in msg
    rc, h, msg = _vk_create(vk, nic=0)
    assert (rc, h) == (-4, 77)
    with pytest.raises(capi.GosnarkHipError, match="alpha"):
        groth16.PrepareVerificationKey(groth16.Vk(IC=vk.IC, G1_Alpha=(ax, (ay + 1) % Q, az), G2_Beta=vk.G2_Beta, G2_Gamma=vk.G2_Gamma,
                                                  G2_Delta=vk.G2_Delta))
    after = capi.alloc_counters()
    assert after[0] - before[0] == after[1] - before[1]                 # nothing stays allocated on the refusals


def test_lifecycle_memory_is_returned(zoo):
    vks, _, pool = zoo
    capi.trim()
    start = capi.memory_query()["object_bytes"]
    mine = [groth16.PrepareVerificationKey(vk) for vk in vks[1:4]]
    for k, vk in zip(mine, vks[1:4]):
        obj, tab = capi.handle_bytes(k.handle)
        assert obj >= 2 * 102 * 36 * 4 + 48 * 8 + len(vk.IC) * 64 and tab == 0      # the lines as limbs, the Miller value, the IC points
        assert capi.handle_device(k.handle) == 0
    assert capi.memory_query()["object_bytes"] > start
    before = capi.alloc_counters()
    assert groth16.VerifyProofsEachKeys(mine, [1, 0, 2], [pool[2][0][0], pool[1][0][0], pool[3][0][0]],
                                        [pool[2][1][0], pool[1][1][0], pool[3][1][0]]) == [True] * 3
    after = capi.alloc_counters()
    assert after[0] - before[0] == after[1] - before[1]                 # every temporary of the call is freed
    for k in mine:
        k.handle.free()
    capi.trim()
    assert capi.memory_query()["object_bytes"] == start


def test_compressed_proofs_of_many_keys(zoo):
    vks, keys, _ = zoo
    kop, proofs, signals, _ = seam_set(zoo)
    blobs = compressed.CompressProofs(proofs, compressed.GNARK)
    at = 40
    blobs[at] = _undecodable(blobs[at])
    got = groth16.VerifyProofsEachKeysCompressed(keys, kop, blobs, signals, compressed.GNARK)
    assert got == [i != at for i in range(len(proofs))]


def _undecodable(blob):
    """The blob with A replaced by the encoding of an x with no point on the curve (x^3 + 3 is not a square mod q)."""
    x = next(x for x in range(2, 60) if pow(x ** 3 + 3, (Q - 1) // 2, Q) != 1)
    return compressed.EncodeG1(capi.ints_to_u64([x]), [0], compressed.GNARK)[0].tobytes() + bytes(blob[32:])
