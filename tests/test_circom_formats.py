"""snarkjs / circom files (go-snark-study_amd/circom.py) on the reference's own fixture, externalVerif/circom-test (the multiplier
circuit: 3 * 11 = 33 over a domain of 4 points), copied as data into tests/golden/circom_multiplier/.  No GPU: parsing, the
transposition of polsA/B/C into rows, the proof writer, and the verifier (host code) on the proof snarkjs recorded."""
import gosnark_amd  # noqa: F401
from gosnark_amd import circom
import circom_util as CU

R = CU.R


def test_fixture_parses():
    pk = circom.ParseProvingKey(CU.fixture_json("proving_key"))
    assert (pk.nVars, pk.nPublic, pk.domainBits, pk.domainSize) == (4, 1, 2, 4)
    assert len(pk.A) == len(pk.B1) == len(pk.B2) == len(pk.C) == 4 and len(pk.hExps) == 5          # hExps holds m + 1 points
    assert pk.A[3] == circom.G1_INF and pk.B1[0] == circom.G1_INF and pk.B2[0] == circom.G2_INF      # ["0", "1", "0"]
    assert pk.C[0] == circom.G1_INF and pk.C[1] == circom.G1_INF and pk.C[2][2] == 1                 # null for the public signals
    assert pk.Z() == [R - 1, 0, 0, 0, 1]
    vk = circom.ParseVerificationKey(CU.fixture_json("verification_key"))
    assert len(vk.IC) == 2 and vk.G2_Gamma[2] == (1, 0)
    assert circom.ParseWitness(CU.fixture_json("witness")) == [1, 33, 3, 11]
    assert circom.ParsePublic(CU.fixture_json("public")) == [33]


def test_pols_transpose_to_the_rows_of_the_system():
    """polsX[s][c] is the coefficient of signal s in row c.  The multiplier: row 0 says (-w2) * w3 = -w1, rows 1 and 2 are the rows
    snarkjs adds for the constant and the public signal, row 3 of the domain is empty (and not uploaded)."""
    pk = circom.ParseProvingKey(CU.fixture_json("proving_key"))
    assert pk.rows_a == [{2: R - 1}, {0: 1}, {1: 1}]
    assert pk.rows_b == [{3: 1}, {}, {}]
    assert pk.rows_c == [{1: R - 1}, {}, {}]
    a, b, c = pk.csr()
    assert a[0].tolist() == [0, 1, 2, 3] and a[1].tolist() == [2, 0, 1]
    assert b[0].tolist() == [0, 1, 1, 1] and b[1].tolist() == [3]
    assert c[0].tolist() == [0, 1, 1, 1] and c[1].tolist() == [1]
    from gosnark_amd import capi
    assert capi.u64_to_ints(a[2]) == [R - 1, 1, 1] and capi.u64_to_ints(b[2]) == [1] and capi.u64_to_ints(c[2]) == [R - 1]
    w = [1, 33, 3, 11]
    for ra, rb, rc in zip(pk.rows_a, pk.rows_b, pk.rows_c):
        dot = lambda row: sum(v * w[s] for s, v in row.items()) % R       # noqa: E731
        assert dot(ra) * dot(rb) % R == dot(rc)


def test_proof_json_round_trips():
    j = CU.fixture_json("proof")
    assert circom.ProofToJSON(circom.ParseProof(j)) == j


def test_verifier_accepts_the_recorded_snarkjs_proof_and_rejects_another_statement():
    vk, proof = CU.fixture_json("verification_key"), CU.fixture_json("proof")
    assert circom.VerifyFromCircom(vk, proof, CU.fixture_json("public")) is True
    assert circom.VerifyFromCircom(vk, proof, [34]) is False
