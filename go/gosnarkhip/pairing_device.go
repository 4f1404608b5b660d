package gosnarkhip

/*
#include "gosnark_hip.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"math/big"
	"runtime"
)

// Pairing products on the device, and Groth16 proofs verified in batches.  One proof check is O(1) work and stays on the host
// (Groth16Verify); thousands of proofs under one key are a Miller loop per proof, which the device runs one lane per pair.
// include/gosnark_hip.h has the formulas, the precondition on the G2 points and the soundness bound of the batch check.

// PairingProduct is prod_i e(P[poff+i], Q[qoff+i]) over a resident G1 and a resident G2 array (gs_pairing_product): the value in
// Pairing's encoding (12 x 4 words) and whether it is one.  n = 0 gives one; a pair with an infinite member contributes one.  The Q
// must be in G2 (G2SubgroupCheck on the same handle: the uploads test the curve equation only).  Call sequence = tests/c/verify_batch.c.
func PairingProduct(g1 Handle, poff int, g2 Handle, qoff, n int) (value [48]uint64, isOne bool, err error) {
	var one C.int
	err = call(func() C.int {
		return C.gs_pairing_product(C.gs_handle(g1), C.size_t(poff), C.gs_handle(g2), C.size_t(qoff), C.size_t(n), ptr(value[:]), &one)
	})
	return value, one == 1, err
}

// PairingEach is e(P[poff+i], Q[qoff+i]) for EVERY i < n over a resident G1 and a resident G2 array (gs_pairing_each): Miller loop and
// final exponentiation on the device, one lane per pair.  values holds n x 48 words in Pairing's encoding, each equal to Pairing of
// that pair bit for bit; isOne[i] says whether value i is one.  A pair with an infinite member gives one.  The Q must be in G2
// (G2SubgroupCheck on the same handle).  Call sequence = tests/c/pairing_each.c.
func PairingEach(g1 Handle, poff int, g2 Handle, qoff, n int) (values []uint64, isOne []bool, err error) {
	if n < 0 {
		return nil, nil, errors.New("gosnarkhip: PairingEach: negative count")
	}
	values = make([]uint64, 48*n+48)
	ones := make([]C.int, n+1)
	err = call(func() C.int {
		return C.gs_pairing_each(C.gs_handle(g1), C.size_t(poff), C.gs_handle(g2), C.size_t(qoff), C.size_t(n), ptr(values), &ones[0])
	})
	runtime.KeepAlive(ones)
	if err != nil {
		return nil, nil, err
	}
	isOne = make([]bool, n)
	for i := range isOne {
		isOne[i] = ones[i] == 1
	}
	return values[:48*n], isOne, nil
}

// Groth16BatchProof is one proof of a batch with its public signals.
type Groth16BatchProof struct {
	PiA           [3]*big.Int
	PiB           [3][2]*big.Int
	PiC           [3]*big.Int
	PublicSignals []*big.Int
}

// Groth16VerifyBatch checks many proofs of ONE verification key in one randomised product check (gs_groth16_verify_batch): true iff
// every proof verifies, wrong with probability at most (len(proofs) - 1) / r over a challenge drawn uniformly after the proofs are
// fixed, and only towards true.  The challenge is the caller's randomness (crypto/rand); 0 and 1 mod r are refused.  false does not
// say which proof is bad: Groth16VerifyEach says which.  Needs Init.  Call sequence = tests/c/verify_batch.c.
func Groth16VerifyBatch(vk Groth16VkParts, proofs []Groth16BatchProof, challenge *big.Int, order *big.Int) (bool, error) {
	ic, err := G1Points(vk.IC)
	if err != nil {
		return false, err
	}
	g1, err := G1Points([][3]*big.Int{vk.G1Alpha})
	if err != nil {
		return false, err
	}
	g2, err := G2Points([][3][2]*big.Int{vk.G2Beta, vk.G2Gamma, vk.G2Delta})
	if err != nil {
		return false, err
	}
	npublic := 0
	if len(proofs) > 0 {
		npublic = len(proofs[0].PublicSignals)
	}
	as := make([][3]*big.Int, 0, len(proofs))
	bs := make([][3][2]*big.Int, 0, len(proofs))
	cs := make([][3]*big.Int, 0, len(proofs))
	signals := make([]*big.Int, 0, len(proofs)*npublic)
	for _, p := range proofs {
		if len(p.PublicSignals) != npublic {
			return false, errors.New("gosnarkhip: every proof of one key has the same number of public signals")
		}
		as, bs, cs = append(as, p.PiA), append(bs, p.PiB), append(cs, p.PiC)
		signals = append(signals, p.PublicSignals...)
	}
	a, err := G1Points(as)
	if err != nil {
		return false, err
	}
	b, err := G2Points(bs)
	if err != nil {
		return false, err
	}
	c, err := G1Points(cs)
	if err != nil {
		return false, err
	}
	pub, err := Scalars(signals, order)
	if err != nil {
		return false, err
	}
	ch, err := Scalars([]*big.Int{challenge}, order)
	if err != nil {
		return false, err
	}
	if len(pub) == 0 {
		pub = make([]uint64, 4)
	}
	if len(proofs) == 0 {
		a, b, c = make([]uint64, 12), make([]uint64, 24), make([]uint64, 12)
	}
	var ok C.int
	err = call(func() C.int {
		return C.gs_groth16_verify_batch(ptr(g1[0:]), ptr(g2[0:]), ptr(g2[24:]), ptr(g2[48:]), ptr(ic), C.size_t(len(vk.IC)),
			ptr(pub), C.size_t(npublic), ptr(a), ptr(b), ptr(c), C.size_t(len(proofs)), ptr(ch), &ok)
	})
	runtime.KeepAlive(ic)
	runtime.KeepAlive(g1)
	runtime.KeepAlive(g2)
	runtime.KeepAlive(pub)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	runtime.KeepAlive(c)
	runtime.KeepAlive(ch)
	return ok == 1, err
}

// Groth16VerifyEach gives the verdict of Groth16Verify for EVERY proof of a batch under one verification key, on the device
// (gs_groth16_verify_each): exact and deterministic, no challenge.  A proof with a point off its curve, a B outside the order-r
// subgroup or (under strict mode) a non-canonical encoding gets false and is not an error; a key point off its curve makes every
// verdict false.  Needs Init.  Call sequence = tests/c/verify_each.c.
func Groth16VerifyEach(vk Groth16VkParts, proofs []Groth16BatchProof, order *big.Int) ([]bool, error) {
	if len(proofs) == 0 {
		return []bool{}, nil
	}
	ic, err := G1Points(vk.IC)
	if err != nil {
		return nil, err
	}
	g1, err := G1Points([][3]*big.Int{vk.G1Alpha})
	if err != nil {
		return nil, err
	}
	g2, err := G2Points([][3][2]*big.Int{vk.G2Beta, vk.G2Gamma, vk.G2Delta})
	if err != nil {
		return nil, err
	}
	npublic := len(proofs[0].PublicSignals)
	as := make([][3]*big.Int, 0, len(proofs))
	bs := make([][3][2]*big.Int, 0, len(proofs))
	cs := make([][3]*big.Int, 0, len(proofs))
	signals := make([]*big.Int, 0, len(proofs)*npublic)
	for _, p := range proofs {
		if len(p.PublicSignals) != npublic {
			return nil, errors.New("gosnarkhip: every proof of one key has the same number of public signals")
		}
		as, bs, cs = append(as, p.PiA), append(bs, p.PiB), append(cs, p.PiC)
		signals = append(signals, p.PublicSignals...)
	}
	a, err := G1Points(as)
	if err != nil {
		return nil, err
	}
	b, err := G2Points(bs)
	if err != nil {
		return nil, err
	}
	c, err := G1Points(cs)
	if err != nil {
		return nil, err
	}
	pub, err := Scalars(signals, order)
	if err != nil {
		return nil, err
	}
	if len(pub) == 0 {
		pub = make([]uint64, 4)
	}
	oks := make([]C.int, len(proofs))
	var nbad C.uint64_t
	err = call(func() C.int {
		return C.gs_groth16_verify_each(ptr(g1[0:]), ptr(g2[0:]), ptr(g2[24:]), ptr(g2[48:]), ptr(ic), C.size_t(len(vk.IC)),
			ptr(pub), C.size_t(npublic), ptr(a), ptr(b), ptr(c), C.size_t(len(proofs)), &oks[0], &nbad)
	})
	runtime.KeepAlive(ic)
	runtime.KeepAlive(g1)
	runtime.KeepAlive(g2)
	runtime.KeepAlive(pub)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	runtime.KeepAlive(c)
	runtime.KeepAlive(oks)
	if err != nil {
		return nil, err
	}
	out := make([]bool, len(proofs))
	for i := range out {
		out[i] = oks[i] == 1
	}
	return out, nil
}

// Groth16Vk is a verification key prepared and resident on the device (gs_groth16_vk_create): its IC points, the prepared lines of
// gamma and delta and the Miller value of e(alpha, beta).  NPublic = len(IC) - 1.
type Groth16Vk struct {
	h       Handle
	NPublic int
}

// Handle exposes the raw gs_handle.
func (k *Groth16Vk) Handle() Handle { return k.h }

// Free releases the key's device memory.
func (k *Groth16Vk) Free() error {
	h := k.h
	k.h = 0
	return Free(h)
}

// Groth16VkCreate does once per key what Groth16VerifyEach does per call -- the curve tests of the key, the Miller value of
// e(alpha, beta), the prepared lines of gamma and delta -- and keeps the result on logical device `device` (gs_groth16_vk_create).  A
// key that cannot verify anything (a point off its curve, a G2 point that is not of order r) is refused with an error that names the
// point.  Needs Init.  Call sequence = tests/c/verify_each_keys.c.
func Groth16VkCreate(device int, vk Groth16VkParts) (*Groth16Vk, error) {
	ic, err := G1Points(vk.IC)
	if err != nil {
		return nil, err
	}
	if len(vk.IC) == 0 {
		return nil, errors.New("gosnarkhip: a verification key has at least IC[0]")
	}
	g1, err := G1Points([][3]*big.Int{vk.G1Alpha})
	if err != nil {
		return nil, err
	}
	g2, err := G2Points([][3][2]*big.Int{vk.G2Beta, vk.G2Gamma, vk.G2Delta})
	if err != nil {
		return nil, err
	}
	var h C.gs_handle
	err = onDevice(device, func() C.int {
		return C.gs_groth16_vk_create(ptr(g1[0:]), ptr(g2[0:]), ptr(g2[24:]), ptr(g2[48:]), ptr(ic), C.size_t(len(vk.IC)), &h)
	})
	runtime.KeepAlive(ic)
	runtime.KeepAlive(g1)
	runtime.KeepAlive(g2)
	if err != nil {
		return nil, err
	}
	return &Groth16Vk{h: Handle(h), NPublic: len(vk.IC) - 1}, nil
}

// Groth16VerifyEachKeys gives the verdict of Groth16Verify for every proof of a batch in which each proof names its key: proof i is
// checked under keys[keyOfProof[i]] (gs_groth16_verify_each_keys).  One call costs the latency of one wave's loop however many keys
// it names.  Every proof brings exactly NPublic signals of its key; the same key may appear twice and a key may have no proofs.  The
// keys live on logical device `device`.  A proof with a point off its curve, a B outside the order-r subgroup or (under strict mode) a
// non-canonical encoding gets false and is not an error; a key index out of range is.  Needs Init.  Call sequence =
// tests/c/verify_each_keys.c.
func Groth16VerifyEachKeys(device int, keys []*Groth16Vk, keyOfProof []int, proofs []Groth16BatchProof, order *big.Int) ([]bool, error) {
	if len(keyOfProof) != len(proofs) {
		return nil, errors.New("gosnarkhip: one key index per proof")
	}
	if len(proofs) == 0 {
		return []bool{}, nil
	}
	if len(keys) == 0 {
		return nil, errors.New("gosnarkhip: proofs but no keys")
	}
	hs := make([]C.gs_handle, len(keys))
	for i, k := range keys {
		hs[i] = C.gs_handle(k.h)
	}
	kop := make([]C.uint32_t, len(proofs))
	as := make([][3]*big.Int, 0, len(proofs))
	bs := make([][3][2]*big.Int, 0, len(proofs))
	cs := make([][3]*big.Int, 0, len(proofs))
	signals := make([]*big.Int, 0, len(proofs))
	for i, p := range proofs {
		if keyOfProof[i] < 0 || keyOfProof[i] >= len(keys) {
			return nil, fmt.Errorf("gosnarkhip: proof %d names key %d of %d", i, keyOfProof[i], len(keys))
		}
		if len(p.PublicSignals) != keys[keyOfProof[i]].NPublic {
			return nil, fmt.Errorf("gosnarkhip: proof %d has %d public signals, its key takes %d", i, len(p.PublicSignals), keys[keyOfProof[i]].NPublic)
		}
		kop[i] = C.uint32_t(keyOfProof[i])
		as, bs, cs = append(as, p.PiA), append(bs, p.PiB), append(cs, p.PiC)
		signals = append(signals, p.PublicSignals...)
	}
	a, err := G1Points(as)
	if err != nil {
		return nil, err
	}
	b, err := G2Points(bs)
	if err != nil {
		return nil, err
	}
	c, err := G1Points(cs)
	if err != nil {
		return nil, err
	}
	pub, err := Scalars(signals, order)
	if err != nil {
		return nil, err
	}
	if len(pub) == 0 {
		pub = make([]uint64, 4)
	}
	oks := make([]C.int, len(proofs))
	var nbad C.uint64_t
	err = onDevice(device, func() C.int {
		return C.gs_groth16_verify_each_keys(&hs[0], C.size_t(len(keys)), &kop[0], ptr(pub), ptr(a), ptr(b), ptr(c), C.size_t(len(proofs)), &oks[0], &nbad)
	})
	runtime.KeepAlive(hs)
	runtime.KeepAlive(kop)
	runtime.KeepAlive(pub)
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	runtime.KeepAlive(c)
	runtime.KeepAlive(oks)
	if err != nil {
		return nil, err
	}
	out := make([]bool, len(proofs))
	for i := range out {
		out[i] = oks[i] == 1
	}
	return out, nil
}

// PinocchioBatchProof is one Pinocchio proof of a batch with its public signals.
type PinocchioBatchProof struct {
	Proof         PinocchioProof
	PublicSignals []*big.Int
}

// PinocchioVerifyEach gives the answers of PinocchioVerify for EVERY proof of a batch under one verification key, on the device
// (gs_pinocchio_verify_each): ok[i] is its verdict and failed[i] is 0 or the number (1..5) of the first of the five equations, in the
// reference's order, that does not hold.  Exact and deterministic, no challenge.  A proof with a point off its curve, a PiB outside
// the order-r subgroup or (under strict mode, then with failed 0) a non-canonical encoding gets false and is not an error; a key point
// off its curve fails every equation that uses it.  Needs Init.  Call sequence = tests/c/pinocchio_verify_each.c.
func PinocchioVerifyEach(vk PinocchioVkParts, proofs []PinocchioBatchProof, order *big.Int) (ok []bool, failed []int, err error) {
	if len(proofs) == 0 {
		return []bool{}, []int{}, nil
	}
	g2, err := G2Points([][3][2]*big.Int{vk.Vka, vk.Vkc, vk.G2Kbg, vk.G2Kg, vk.Vkz})
	if err != nil {
		return nil, nil, err
	}
	g1, err := G1Points([][3]*big.Int{vk.Vkb, vk.G1Kbg})
	if err != nil {
		return nil, nil, err
	}
	ic, err := G1Points(vk.IC)
	if err != nil {
		return nil, nil, err
	}
	npublic := len(proofs[0].PublicSignals)
	signals := make([]*big.Int, 0, len(proofs)*npublic)
	words := make([]uint64, 0, 108*len(proofs))
	for _, bp := range proofs {
		if len(bp.PublicSignals) != npublic {
			return nil, nil, errors.New("gosnarkhip: every proof of one key has the same number of public signals")
		}
		signals = append(signals, bp.PublicSignals...)
		p := bp.Proof
		// a proof = PiA, PiAp (12 words each), PiB (24), PiBp, PiC, PiCp, PiH, PiKp (12 each) = 108 words
		pa, err := G1Points([][3]*big.Int{p.PiA, p.PiAp})
		if err != nil {
			return nil, nil, err
		}
		pb, err := G2Points([][3][2]*big.Int{p.PiB})
		if err != nil {
			return nil, nil, err
		}
		pc, err := G1Points([][3]*big.Int{p.PiBp, p.PiC, p.PiCp, p.PiH, p.PiKp})
		if err != nil {
			return nil, nil, err
		}
		words = append(append(append(words, pa...), pb...), pc...)
	}
	pub, err := Scalars(signals, order)
	if err != nil {
		return nil, nil, err
	}
	if len(pub) == 0 {
		pub = make([]uint64, 4)
	}
	oks := make([]C.int, len(proofs))
	fails := make([]C.int, len(proofs))
	var nbad C.uint64_t
	err = call(func() C.int {
		return C.gs_pinocchio_verify_each(ptr(g2[0:]), ptr(g1[0:]), ptr(g2[24:]), ptr(g1[12:]), ptr(g2[48:]), ptr(g2[72:]), ptr(g2[96:]),
			ptr(ic), C.size_t(len(vk.IC)), ptr(pub), C.size_t(npublic), ptr(words), C.size_t(len(proofs)), &oks[0], &fails[0], &nbad)
	})
	runtime.KeepAlive(g1)
	runtime.KeepAlive(g2)
	runtime.KeepAlive(ic)
	runtime.KeepAlive(pub)
	runtime.KeepAlive(words)
	runtime.KeepAlive(oks)
	runtime.KeepAlive(fails)
	if err != nil {
		return nil, nil, err
	}
	ok, failed = make([]bool, len(proofs)), make([]int, len(proofs))
	for i := range ok {
		ok[i], failed[i] = oks[i] == 1, int(fails[i])
	}
	return ok, failed, nil
}
