package gosnarkhip

/*
#include "gosnark_hip.h"
*/
import "C"

import (
	"errors"
	"math/big"
	"runtime"
)

// Keys over a power-of-two domain: what snarkjs / circom produce (proving_key.json: polsA/B/C, A, B1, B2, C, hExps).  The QAP lives on
// the m = 2^k-th roots of unity, omega = 5^((r-1)/m), row c of the system at omega^c, Z = x^m - 1.  Such a key is an ordinary
// Groth16Key (UploadGroth16Key with A, B1, B2, C, hExps and Z = x^m - 1); only the R1CS handle says which QAP is meant, and every
// witness entry point of the key (ProveWitness, ProveWitnessBegin, the host-buffer tickets, ProveR1CS) accepts it.

// UploadR1CSDomain validates A, B, C (constraints x variables, CSR; at most 2^log2Domain constraints) and keeps them resident on
// logical device `device` as a QAP over the domain of 2^log2Domain points (gs_r1cs_upload_domain).
func UploadR1CSDomain(device, log2Domain int, a, b, c CSR, nvars int) (*R1CS, error) {
	n := len(a.RowPtr) - 1
	if n < 1 || len(b.RowPtr) != n+1 || len(c.RowPtr) != n+1 {
		return nil, errors.New("gosnark-hip: A, B, C must have the same number of constraints")
	}
	var h C.gs_handle
	err := onDevice(device, func() C.int {
		return C.gs_r1cs_upload_domain(C.size_t(log2Domain), C.size_t(n), C.size_t(nvars),
			ptr32(a.RowPtr), ptr32(a.Col), ptr(a.Val), ptr32(b.RowPtr), ptr32(b.Col), ptr(b.Val), ptr32(c.RowPtr), ptr32(c.Col), ptr(c.Val), &h)
	})
	runtime.KeepAlive(a)
	runtime.KeepAlive(b)
	runtime.KeepAlive(c)
	if err != nil {
		return nil, err
	}
	return &R1CS{Handle(h), n, nvars}, nil
}

// DeriveEvalBasisDomain computes the coset evaluation-basis array of a key whose Z is x^m - 1, m = 2^log2Domain, from its hExps alone
// -- one transform of size m carried out in the group, once per key -- and attaches it (gs_groth16_pk_derive_eval_domain): witness
// proofs then need three forward and three inverse transforms of size m and no division.
func (k *Groth16Key) DeriveEvalBasisDomain(log2Domain int) error {
	return call(func() C.int { return C.gs_groth16_pk_derive_eval_domain(C.gs_handle(k.h), C.size_t(log2Domain)) })
}

// SetEvalBasisDomain attaches a coset evaluation-basis array read from a key file: 2^log2Domain points, natural order
// (gs_groth16_pk_set_eval_domain).
func (k *Groth16Key) SetEvalBasisDomain(points [][3]*big.Int, log2Domain int) error {
	h, err := UploadG1(DeviceOf(k.h), points)
	if err != nil {
		return err
	}
	defer Free(h)
	return call(func() C.int { return C.gs_groth16_pk_set_eval_domain(C.gs_handle(k.h), C.gs_handle(h), C.size_t(log2Domain)) })
}
