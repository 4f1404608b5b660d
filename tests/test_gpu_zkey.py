"""-m gpu: proving from circuit.zkey / witness.wtns -- coset-only keys (gs_groth16_pk_create_domain) and product systems
(gs_r1cs_upload_zkey), the sections uploaded as they lie in the file (gs_g1_upload_affine_mont / gs_g2_upload_affine_mont).

Instances come from tests/circom_util.Instance (keys from toxic values, proofs with closed forms in the generators) and are written
with circom.WriteZkey; the committed fixture tests/golden/zkey_multiplier is the reference's circom-test key converted by
circom.ConvertProvingKey.  Every proof is compared bit for bit with the proof of the same instance through the proving_key.json route."""
import functools
import os
import random
import struct

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, groth16
import circom_util as CU
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R, Q = CU.R, circom.Q
GS_ERR_ARG, GS_ERR_SHAPE = -3, -4
ZFIX = os.path.join(CU.HERE, "golden", "zkey_multiplier")
COSET_ONLY = "coset evaluation basis only"


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)
    capi.set_memory_limit(0)
    yield
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)
    capi.set_memory_limit(0)


def rs_pair(seed):
    rng = random.Random(seed)
    return rng.randrange(R), rng.randrange(R)


# ---- instances as zkey files -----------------------------------------------------------------------------------------------------
def dev_g1(ks):
    """k G for every k, affine Jacobian tuples, by the device's fixed-base batch (checked against the oracle elsewhere)"""
    return capi.g1_tuples(capi.g1_download(capi.g1_fixed_base(CU.u64(ks))))


def dev_g2(ks):
    return capi.g2_tuples(capi.g2_download(capi.g2_fixed_base(CU.u64(ks))))


class ZkeyInstance:
    """An Instance, its parsed-JSON form (circom.ProvingKey), its verification key and its coset evaluation basis (closed form)."""

    def __init__(self, k, n, seed):
        self.inst = inst = CU.Instance(k, n, seed)
        ginv = pow(inst.gamma, -1, R)
        ic = [(inst.beta * inst.at[i] + inst.alpha * inst.bt[i] + inst.ct[i]) * ginv % R for i in range(inst.npublic + 1)]
        s1 = dev_g1([inst.alpha, inst.beta, inst.delta])
        s2 = dev_g2([inst.beta, inst.delta, inst.gamma])
        self.pkj = circom.ProvingKey(inst.nvars, inst.npublic, k, inst.rows_a, inst.rows_b, inst.rows_c, dev_g1(inst.at), dev_g1(inst.bt),
                                     dev_g2(inst.bt), dev_g1(inst.cd), dev_g1(inst.hexps), s1[0], s1[1], s1[2], s2[0], s2[1])
        self.vk = groth16.Vk(IC=dev_g1(ic), G1_Alpha=s1[0], G2_Beta=s2[0], G2_Gamma=s2[2], G2_Delta=s2[1])
        self.e = dev_g1(inst.eval_basis_scalars())

    def write(self, tmp_path, **kw):
        path = str(tmp_path / "circuit.zkey")
        circom.WriteZkey(path, self.pkj, self.vk, self.e, **kw)
        wpath = str(tmp_path / "witness.wtns")
        circom.WriteWtns(wpath, self.inst.w)
        return path, wpath

    def json_route(self):
        """the parent's route: the key with hExps, E derived on the device, the three-matrix domain R1CS"""
        dev, r1cs = self.inst.upload()
        circom.DeriveEvalBasis(dev, self.inst.k)
        return dev, r1cs


@functools.lru_cache(maxsize=None)
def zinst(k, n, seed=1):
    return ZkeyInstance(k, n, seed)


# ---- point import ----------------------------------------------------------------------------------------------------------------
NPTS = 257


@functools.lru_cache(maxsize=None)
def oracle_points():
    """257 multiples of each generator from the oracle (not from the device): (G1 tuples, G2 tuples)"""
    rng = random.Random(77)
    ks = [rng.randrange(1, R) for _ in range(NPTS)]
    g1, g2 = [], []
    for k in ks:
        a, b = C.g1_affine(C.g1_mul_scalar(O.G1_GEN, k)), C.g2_affine(C.g2_mul_scalar(O.G2_GEN, k))
        g1.append((a[0], a[1], 1))
        g2.append((b[0], b[1], (1, 0)))
    return g1, g2


def with_infinities(pts, n, inf):
    pts = list(pts[:n])
    for i in {0, n - 1, n // 2}:
        pts[i] = inf
    return pts


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_points_in_the_file_encoding_arrive_as_the_oracles_points(n):
    g1, g2 = oracle_points()
    p1, p2 = with_infinities(g1, n, circom.G1_INF), with_infinities(g2, n, circom.G2_INF)
    b1 = np.frombuffer(b"x" + b"".join(circom.G1ToZkey(p) for p in p1), dtype=np.uint8)[1:]          # an odd address: any alignment goes
    b2 = np.frombuffer(b"".join(circom.G2ToZkey(p) for p in p2), dtype=np.uint8)
    h1, h2 = capi.g1_upload_affine_mont(b1), capi.g2_upload_affine_mont(b2)
    assert len(h1) == n and len(h2) == n
    zero1, zero2 = (0, 0, 0), ((0, 0), (0, 0), (0, 0))                                                # gs_g*_download's infinity
    assert capi.g1_tuples(capi.g1_download(h1)) == [zero1 if p == circom.G1_INF else p for p in p1]
    assert capi.g2_tuples(capi.g2_download(h2)) == [zero2 if p == circom.G2_INF else p for p in p2]
    # the same points through the Jacobian upload are the same resident bytes' worth: an MSM over either handle agrees
    if n == 65:
        sc = CU.u64([random.Random(5).randrange(R) for _ in range(n)])
        assert capi.msm(h1, sc) == capi.msm(capi.g1_upload(capi.g1_points_to_u64([zero1 if p == circom.G1_INF else p for p in p1])), sc)


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_bad_points_are_refused_with_their_index(group):
    g1, g2 = oracle_points()
    n, at = 65, 41
    pts, enc, upload, size = (g1, circom.G1ToZkey, capi.g1_upload_affine_mont, 64) if group == "g1" else (g2, circom.G2ToZkey, capi.g2_upload_affine_mont, 128)
    good = bytearray(b"".join(enc(p) for p in pts[:n]))
    # a coordinate equal to q
    bad = bytearray(good)
    bad[at * size:at * size + 32] = Q.to_bytes(32, "little")
    with pytest.raises(capi.GosnarkHipError) as e:
        upload(np.frombuffer(bytes(bad), dtype=np.uint8))
    assert e.value.code == GS_ERR_ARG and "index %d" % at in str(e.value) and ">= q" in str(e.value)
    # (x, y + 1): off the curve
    bad = bytearray(good)
    off = at * size + size // 2
    y = int.from_bytes(bad[off:off + 32], "little")
    bad[off:off + 32] = ((y + (1 << 256)) % Q).to_bytes(32, "little")                                   # y + 1 in Montgomery form
    with pytest.raises(capi.GosnarkHipError) as e:
        upload(np.frombuffer(bytes(bad), dtype=np.uint8))
    assert e.value.code == GS_ERR_ARG and "index %d" % at in str(e.value) and "1 of the 65" in str(e.value)
    # two offenders: the first is named
    bad[7 * size:7 * size + 32] = (Q + 5).to_bytes(32, "little")
    with pytest.raises(capi.GosnarkHipError) as e:
        upload(np.frombuffer(bytes(bad), dtype=np.uint8))
    assert "index 7" in str(e.value) and "2 of the 65" in str(e.value)
    assert len(upload(np.frombuffer(bytes(good), dtype=np.uint8))) == n


# ---- coefficient import ----------------------------------------------------------------------------------------------------------
def ntt(v, root):
    """sum_c v_c root^(i c) for every i < len(v) (a power of two), recursive"""
    n = len(v)
    if n == 1:
        return list(v)
    even, odd = ntt(v[0::2], root * root % R), ntt(v[1::2], root * root % R)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = t * odd[i] % R
        out[i], out[i + n // 2] = (even[i] + x) % R, (even[i] - x) % R
        t = t * root % R
    return out


def interpolate(vals, k):
    minv = pow(1 << k, -1, R)
    return [x * minv % R for x in ntt(vals, pow(CU.omega(k), -1, R))]


def product_px(a_vals, b_vals, k):
    """px = a b - c for c = the interpolant of a_j b_j: 2m - 1 coefficients, from the VALUES of A w and B w on the domain"""
    m = 1 << k
    a, b = interpolate(a_vals, k), interpolate(b_vals, k)
    c = interpolate([x * y % R for x, y in zip(a_vals, b_vals)], k)
    w2 = CU.omega(k + 1)
    fa, fb = ntt(a + [0] * m, w2), ntt(b + [0] * m, w2)
    inv2m = pow(2 * m, -1, R)
    ab = [x * inv2m % R for x in ntt([x * y % R for x, y in zip(fa, fb)], pow(w2, -1, R))]
    return [(ab[i] - (c[i] if i < m else 0)) % R for i in range(2 * m - 1)]


def record(mat, row, sig, v):
    return struct.pack("<III", mat, row, sig) + (v % R * pow(2, 512, R) % R).to_bytes(32, "little")


def seam_records(k, nvars, seed):
    """Records of a system over 2^k rows that sit on the seams of the sparse kernels: row 0 empty in both matrices, a row of 513 and (for
    k >= 10) one of 4097 records in A (more records than variables: signals repeat, and repeated records add up), an exact repeat, the
    rest two or three records a row; shuffled.  -> (records, rows_a, rows_b as {signal: summed coefficient})"""
    rng = random.Random(seed)
    m = 1 << k
    rows = ([dict() for _ in range(m)], [dict() for _ in range(m)])
    rec = []

    def put(mat, row, sig, v):
        rec.append(record(mat, row, sig, v))
        rows[mat][row][sig] = (rows[mat][row].get(sig, 0) + v) % R
    long_rows = {1: 513, 2: 4097} if k >= 10 else {1: 513}
    for row in range(1, m):
        for mat in (0, 1):
            count = long_rows.get(row, rng.randrange(2, 4)) if mat == 0 else (512 if row == 1 else rng.randrange(1, 4))
            for _ in range(count):
                put(mat, row, rng.randrange(nvars), rng.randrange(R))
    put(0, m - 1, 3, 7)
    put(0, m - 1, 3, 7)                                              # the same record twice
    put(1, m - 1, nvars - 1, R - 1)
    rng.shuffle(rec)
    return rec, rows[0], rows[1]


@pytest.mark.parametrize("k,nvars", [(3, 40), (10, 700)])
def test_coefficient_records_become_the_csr_of_a_and_b(k, nvars):
    """A w and B w of the device-built CSR against mat_vec, through the one window the ABI has onto them: gs_r1cs_px of the product
    system, px = a b - interpolant(a_j b_j), compared coefficient by coefficient with the same expression on mat_vec's values.  (px is
    blind to one thing only: a constant added to every a_j or every b_j.  Row 0 of both matrices is empty here, and the sparse kernels
    themselves are pinned value by value in test_gpu_r1cs_shapes.py.)"""
    rec, rows_a, rows_b = seam_records(k, nvars, 100 + k)
    assert not rows_a[0] and not rows_b[0] and max(len(r) for r in rows_a) <= nvars
    rng = random.Random(k)
    w = [1] + [rng.randrange(R) for _ in range(nvars - 1)]
    r1cs = circom.DeviceZkeyR1CS(k, nvars, np.frombuffer(b"".join(rec), dtype=np.uint8))
    assert capi.handle_bytes(r1cs.handle)[0] >= len(rec) * 36
    wh = capi.scalars_upload(CU.u64(w))
    got = capi.u64_to_ints(capi.scalars_download(r1cs.ComputePxResident(wh)))
    assert got == product_px(CU.mat_vec(rows_a, w), CU.mat_vec(rows_b, w), k)
    # every other order of the same records gives the same object
    random.Random(9).shuffle(rec)
    again = circom.DeviceZkeyR1CS(k, nvars, np.frombuffer(b"".join(rec), dtype=np.uint8))
    assert capi.u64_to_ints(capi.scalars_download(again.ComputePxResident(wh))) == got


def test_bad_records_are_refused_with_their_index():
    k, nvars = 3, 10
    good = [record(i % 2, i % 8, i % nvars, i + 1) for i in range(300)]
    for at, bad, what in ((17, record(2, 0, 0, 1), "matrix 2"), (250, record(0, 8, 0, 1), "row 8"), (299, record(1, 7, nvars, 1), "signal %d" % nvars)):
        rec = list(good)
        rec[at] = bad
        with pytest.raises(capi.GosnarkHipError) as e:
            circom.DeviceZkeyR1CS(k, nvars, np.frombuffer(b"".join(rec), dtype=np.uint8))
        assert e.value.code == GS_ERR_ARG and "index %d" % at in str(e.value) and what in str(e.value)
    rec = list(good)
    rec[5], rec[200] = record(3, 0, 0, 1), record(0, 9, 0, 1)
    with pytest.raises(capi.GosnarkHipError) as e:
        circom.DeviceZkeyR1CS(k, nvars, np.frombuffer(b"".join(rec), dtype=np.uint8))
    assert "2 of the 300" in str(e.value) and "index 5" in str(e.value)
    for bad_k in (0, 28):
        with pytest.raises(capi.GosnarkHipError) as e:
            circom.DeviceZkeyR1CS(bad_k, nvars, np.frombuffer(b"".join(good), dtype=np.uint8))
        assert e.value.code == GS_ERR_ARG
    empty = circom.DeviceZkeyR1CS(k, nvars, np.zeros(0, dtype=np.uint8))                 # no records: A = B = 0, px = 0
    wh = capi.scalars_upload(CU.u64(list(range(nvars))))
    assert capi.u64_to_ints(capi.scalars_download(empty.ComputePxResident(wh))) == [0] * 15


# ---- proofs ----------------------------------------------------------------------------------------------------------------------
def zkey_proofs(dev, r1cs, w_file, w_ints, r, s):
    """the same proof through every entry point a zkey key has"""
    wh = capi.scalars_upload(CU.u64(w_ints))
    out = {
        "blocking, resident w": groth16.prove_from_witness(dev, r1cs, wh, r, s),
        "blocking, host w": groth16.prove_from_witness_host(dev, r1cs, w_file, r, s),
        "resident ticket": groth16.prove_end(groth16.prove_witness_begin(dev, r1cs, wh, r, s)),
        "host ticket, the memory-mapped .wtns": groth16.prove_end(groth16.prove_witness_host_begin(dev, r1cs, w_file, r, s)),
        "circom.GenerateProofs": circom.GenerateProofs(dev, r1cs, w_file, r, s),
    }
    assert capi.last_timing()["fallbacks"] == 0
    p = groth16.NewProver(None, dev, r1cs)
    for _ in range(4):                                               # more than the three slots
        p.SubmitWithRS(w_file, None, r, s)
    for i in range(4):
        out["streaming Prover %d" % i] = p.Collect()
    p.Close()
    return out


@pytest.mark.parametrize("policy", ["always", "never"])
@pytest.mark.parametrize("k,short", [(1, 0), (3, 3), (10, 3), (11, 5)])
def test_zkey_proofs_equal_the_closed_form_and_the_json_route(tmp_path, policy, k, short):
    capi.set_table_policy(policy)
    zi = zinst(k, (1 << k) - short)
    inst = zi.inst
    path, wpath = zi.write(tmp_path)
    dev, r1cs = circom.UploadZkey(path)
    assert capi.pk_eval_count(dev.handle) == inst.m and capi.pk_quot_count(dev.handle) == 0
    assert groth16.ExportPkArray(dev, "PowersTauDeltaEval") == zi.e
    capi.call("gs_groth16_pk_export", capi.raw(dev), 4, None, 0)                  # PowersTauDelta: no points, and it says so
    one = np.zeros(12, dtype=np.uint64)
    with pytest.raises(capi.GosnarkHipError, match="array has 0 points"):
        capi.call("gs_groth16_pk_export", capi.raw(dev), 4, capi.ptr64(one), 1)
    w_file = circom.ReadWtns(wpath)
    r, s = rs_pair(300 + k)
    jdev, jr1cs = zi.json_route()
    want = groth16.prove_from_witness(jdev, jr1cs, capi.scalars_upload(CU.u64(inst.w)), r, s)
    CU.assert_closed_form(want, inst.expected_scalars(inst.w, r, s))
    for name, got in zkey_proofs(dev, r1cs, w_file, inst.w, r, s).items():
        assert CU.words(got) == CU.words(want), name
    vk = circom.VerificationKeyFromZkey(path)
    public = inst.w[1:1 + inst.npublic]
    assert circom.VerifyFromCircom(vk, want, public) is True
    assert circom.VerifyFromCircom(vk, want, [(public[0] + 1) % R]) is False


@pytest.mark.parametrize("policy", ["always", "never"])
def test_the_committed_fixture_proves_and_verifies(policy):
    capi.set_table_policy(policy)
    pkj = circom.ParseProvingKey(CU.fixture_json("proving_key"))
    w = circom.ParseWitness(CU.fixture_json("witness"))
    vk_json = CU.fixture_json("verification_key")
    zpath, wpath = os.path.join(ZFIX, "circuit.zkey"), os.path.join(ZFIX, "witness.wtns")
    jdev, jr1cs = circom.UploadProvingKey(pkj)
    circom.DeriveEvalBasis(jdev, pkj.domainBits)
    # the committed section 9 is what the device derives from the JSON key's hExps (the file was written on the host)
    assert circom.ReadZkey(zpath).g1("H") == groth16.ExportPkArray(jdev, "PowersTauDeltaEval")
    dev, r1cs = circom.UploadZkey(zpath)
    w_file = circom.ReadWtns(wpath)
    vk = circom.VerificationKeyFromZkey(zpath)
    for r, s in [(0, 0), (1, 0), rs_pair(31), rs_pair(32)]:
        want = circom.GenerateProofs(jdev, jr1cs, w, r, s)
        for name, got in zkey_proofs(dev, r1cs, w_file, w, r, s).items():
            assert CU.words(got) == CU.words(want), (name, r, s)
        assert circom.VerifyFromCircom(vk, want, [33]) is True and circom.VerifyFromCircom(vk_json, want, [33]) is True
        assert circom.VerifyFromCircom(vk, want, [34]) is False


def test_convert_proving_key_reproduces_the_committed_fixture(tmp_path):
    pkj = circom.ParseProvingKey(CU.fixture_json("proving_key"))
    out = str(tmp_path / "converted.zkey")
    circom.ConvertProvingKey(pkj, CU.fixture_json("verification_key"), out)
    assert open(out, "rb").read() == open(os.path.join(ZFIX, "circuit.zkey"), "rb").read()


# ---- cross-products --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,short", [(3, 1), (10, 3)])
def test_either_new_object_pairs_with_the_other_kind(tmp_path, k, short):
    zi = zinst(k, (1 << k) - short)
    inst = zi.inst
    path, _ = zi.write(tmp_path)
    zdev, zr1cs = circom.UploadZkey(path)                            # coset-only key, product system
    jdev, jr1cs = zi.json_route()                                    # key with T (and E), three-matrix system
    wh = capi.scalars_upload(CU.u64(inst.w))
    r, s = rs_pair(400 + k)
    want = groth16.prove_from_witness(jdev, jr1cs, wh, r, s)
    CU.assert_closed_form(want, inst.expected_scalars(inst.w, r, s))
    # a key with T and the product system: the coset route, and after gs_set_eval_basis(0) the px route
    assert CU.words(groth16.prove_from_witness(jdev, zr1cs, wh, r, s)) == CU.words(want)
    via_px, pxh = groth16.prove_from_r1cs(jdev, zr1cs, wh, r, s)
    assert CU.words(via_px) == CU.words(want)
    capi.set_eval_basis(False)
    assert CU.words(groth16.prove_from_witness(jdev, zr1cs, wh, r, s)) == CU.words(want)
    assert CU.words(groth16.prove_end(groth16.prove_witness_host_begin(jdev, zr1cs, inst.w, r, s))) == CU.words(want)
    capi.set_eval_basis(True)
    assert capi.last_timing()["fallbacks"] == 0
    # px of the product system equals px of the three-matrix system on a witness that satisfies it
    assert capi.scalars_download(pxh).tolist() == capi.scalars_download(jr1cs.ComputePxResident(wh)).tolist()
    # a coset-only key and the three-matrix system
    assert CU.words(groth16.prove_from_witness(zdev, jr1cs, wh, r, s)) == CU.words(want)
    assert CU.words(groth16.prove_end(groth16.prove_witness_host_begin(zdev, jr1cs, inst.w, r, s))) == CU.words(want)


# ---- a witness that breaks a constraint ------------------------------------------------------------------------------------------
def test_bad_witness_gives_a_proof_the_verifier_rejects_and_no_fallback():
    zpath, wpath = os.path.join(ZFIX, "circuit.zkey"), os.path.join(ZFIX, "witness.wtns")
    dev, r1cs = circom.UploadZkey(zpath)
    vk = circom.VerificationKeyFromZkey(zpath)
    w = np.array(circom.ReadWtns(wpath))
    r, s = rs_pair(50)
    assert circom.VerifyFromCircom(vk, circom.GenerateProofs(dev, r1cs, w, r, s), [33]) is True
    bad = w.copy()
    bad[len(bad) - 1, 0] += 1
    for proof in (circom.GenerateProofs(dev, r1cs, bad, r, s), groth16.prove_from_witness(dev, r1cs, capi.scalars_upload(bad), r, s)):
        assert capi.last_timing()["fallbacks"] == 0
        assert circom.VerifyFromCircom(vk, proof, [33]) is False
    # the same witness with the three-matrix system on the coset-only key: still no exact route to fall back to, still a proof
    pkj = circom.ParseProvingKey(CU.fixture_json("proving_key"))
    a, b, c = pkj.csr()
    full = circom.DeviceDomainR1CS(pkj.domainBits, a, b, c, pkj.nVars)
    proof = groth16.prove_from_witness(dev, full, capi.scalars_upload(bad), r, s)
    assert capi.last_timing()["fallbacks"] == 0 and circom.VerifyFromCircom(vk, proof, [33]) is False


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def refused(fn, code=GS_ERR_SHAPE, text=COSET_ONLY):
    with pytest.raises(capi.GosnarkHipError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_what_needs_the_monomial_h_array_is_refused_and_the_key_still_proves(tmp_path):
    from gosnark_amd import r1csqap
    k = 3
    zi = zinst(k, 7)
    inst = zi.inst
    path, _ = zi.write(tmp_path)
    dev, r1cs = circom.UploadZkey(path)
    _, jr1cs = zi.json_route()
    wh = capi.scalars_upload(CU.u64(inst.w))
    r, s = rs_pair(60)
    want = groth16.prove_from_witness(dev, r1cs, wh, r, s)
    CU.assert_closed_form(want, inst.expected_scalars(inst.w, r, s))
    px = CU.px_naive(inst.rows_a, inst.rows_b, inst.rows_c, inst.w, k)
    pxh = capi.scalars_upload(CU.u64(px))
    refused(lambda: groth16.prove_resident(dev, wh, pxh, r, s))
    refused(lambda: groth16.prove_end(groth16.prove_begin(dev, wh, pxh, r, s)))
    refused(lambda: groth16.prove_end(groth16.prove_host_begin(dev, inst.w, px, r, s)))
    refused(lambda: groth16.prove_partials(dev, wh, pxh, 0, 1))
    refused(lambda: groth16.prove_from_r1cs(dev, r1cs, wh, r, s))
    refused(lambda: groth16.prove_from_r1cs(dev, jr1cs, wh, r, s))
    capi.set_eval_basis(False)
    refused(lambda: groth16.prove_from_witness(dev, r1cs, wh, r, s))
    refused(lambda: groth16.prove_from_witness_host(dev, r1cs, inst.w, r, s))
    refused(lambda: groth16.prove_witness_begin(dev, r1cs, wh, r, s))
    refused(lambda: groth16.prove_witness_host_begin(dev, jr1cs, inst.w, r, s))
    capi.set_eval_basis(True)
    refused(lambda: groth16.DeriveQuotBasis(dev))
    refused(lambda: groth16.DeriveEvalBasis(dev, inst.m))
    refused(lambda: circom.DeriveEvalBasis(dev, k))
    refused(lambda: groth16.SetQuotBasis(dev, zi.e))
    refused(lambda: groth16.SetEvalBasis(dev, zi.e))
    refused(lambda: groth16.ShardPk(dev, 0, 2))
    # a nodes-1..n system has no route on this key either
    a, b, c = inst.csr()
    refused(lambda: groth16.prove_from_witness(dev, r1csqap.DeviceR1CS(a, b, c, inst.nvars), wh, r, s))
    # the product system is a domain R1CS: refused where every domain R1CS is, with that message
    refused(lambda: groth16.witness_values(dev, r1cs, wh), text="power-of-two domain")
    other = zinst(2, 4)
    odev, _ = circom.UploadZkey(other.write(tmp_path)[0])
    refused(lambda: groth16.prove_from_witness(odev, r1cs, wh, r, s), code=GS_ERR_SHAPE, text="")          # wrong size of key
    # none of this touched the key
    assert capi.pk_eval_count(dev.handle) == inst.m and capi.pk_quot_count(dev.handle) == 0
    assert CU.words(groth16.prove_from_witness(dev, r1cs, wh, r, s)) == CU.words(want)
    assert CU.words(groth16.prove_end(groth16.prove_witness_host_begin(dev, r1cs, inst.w, r, s))) == CU.words(want)


# ---- accounting ------------------------------------------------------------------------------------------------------------------
def test_tables_of_a_coset_only_key_are_counted_built_released_and_evicted(tmp_path):
    k = 10
    zi = zinst(k, (1 << k) - 3)
    inst = zi.inst
    path, _ = zi.write(tmp_path)
    wh = capi.scalars_upload(CU.u64(inst.w))
    r, s = rs_pair(70)
    capi.set_table_policy("never")
    dev, r1cs = circom.UploadZkey(path)
    want = groth16.prove_from_witness(dev, r1cs, wh, r, s)
    obj, tab = capi.handle_bytes(dev.handle)
    # four arrays over w (three G1, one G2) and the m points of E; nothing for the h array it does not have
    assert tab == 0 and obj >= inst.nvars * (3 * 64 + 128) + inst.m * 64
    for route in (1, 2, 0):
        capi.build_tables(dev.handle, route)
    tab = capi.handle_bytes(dev.handle)[1]
    assert tab > 0
    capi.set_table_policy("always")
    assert CU.words(groth16.prove_from_witness(dev, r1cs, wh, r, s)) == CU.words(want) and capi.handle_bytes(dev.handle)[1] == tab
    capi.release_tables(dev.handle)
    assert capi.handle_bytes(dev.handle)[1] == 0
    assert CU.words(groth16.prove_from_witness(dev, r1cs, wh, r, s)) == CU.words(want) and capi.handle_bytes(dev.handle)[1] == tab
    # a second key under a cap that has room for one set of tables: the idle key's tables go
    dev2, r1cs2 = circom.UploadZkey(path)
    base = capi.memory_query()
    capi.set_memory_limit(base["library_bytes"] + tab // 3)
    assert CU.words(groth16.prove_from_witness(dev2, r1cs2, wh, r, s)) == CU.words(want)
    now = capi.memory_query()
    assert now["evictions"] > base["evictions"] and capi.handle_bytes(dev2.handle)[1] == tab and capi.handle_bytes(dev.handle)[1] < tab
    assert CU.words(groth16.prove_from_witness(dev, r1cs, wh, r, s)) == CU.words(want)
    capi.set_memory_limit(0)
