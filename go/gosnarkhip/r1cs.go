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

// CSR is one R1CS matrix (constraints x variables) in compressed sparse rows: what gs_groth16_setup,
// gs_pinocchio_setup and gs_r1cs_upload take instead of the reference's dense [][]*big.Int
// (circuitcompiler/circuit.go:22-26), which is unusable past ~2^10 constraints.
type CSR struct {
	RowPtr []uint32 // n + 1
	Col    []uint32 // nnz
	Val    []uint64 // nnz x 4 words, reduced mod r
}

// CSRFromDense packs circuit.R1CS.A / .B / .C ([constraint][variable]) and returns the variable count.
func CSRFromDense(m [][]*big.Int, order *big.Int) (CSR, int, error) {
	var c CSR
	if len(m) == 0 {
		return c, 0, errors.New("gosnark-hip: empty R1CS matrix")
	}
	nvars := len(m[0])
	c.RowPtr = make([]uint32, len(m)+1)
	t := new(big.Int)
	for j, row := range m {
		if len(row) != nvars {
			return c, 0, errors.New("gosnark-hip: ragged R1CS matrix")
		}
		for k, v := range row {
			if v == nil || v.Sign() == 0 {
				continue
			}
			t.Mod(v, order) // the compiler emits negative coefficients (circuit.go:108-118); Mod is Euclidean
			if t.Sign() == 0 {
				continue
			}
			c.Col = append(c.Col, uint32(k))
			var w [4]uint64
			if err := limbs(w[:], t); err != nil {
				return c, 0, err
			}
			c.Val = append(c.Val, w[:]...)
		}
		c.RowPtr[j+1] = uint32(len(c.Col))
	}
	if len(c.Col) == 0 { // keep the pointers non-nil for cgo
		c.Col = []uint32{0}[:0:1]
		c.Val = make([]uint64, 0, 4)
	}
	return c, nvars, nil
}

// R1CSFromQAP recovers the dense R1CS column values from the reference's dense QAP (alphas[i] = coefficients
// of variable i's polynomial, r1csqap.go:161-188): A[j][i] = alphas[i](j+1), nodes 1..n.  Only used when a
// caller hands GenerateTrustedSetup polynomials without circuit.R1CS; O(m n^2) on the host, which is nothing
// next to the dense QAP the caller already built.
func R1CSFromQAP(polys [][]*big.Int, n int, order *big.Int) [][]*big.Int {
	out := make([][]*big.Int, n)
	for j := range out {
		out[j] = make([]*big.Int, len(polys))
		x := big.NewInt(int64(j + 1))
		for i, p := range polys {
			acc := new(big.Int)
			for k := len(p) - 1; k >= 0; k-- { // Horner
				acc.Mul(acc, x)
				acc.Add(acc, p[k])
				acc.Mod(acc, order)
			}
			out[j][i] = acc
		}
	}
	return out
}

// WitnessViolations is what R1csCheck found: Count of ALL n constraints are violated; Rows holds the first cap of them, 0-based and
// ascending, and Values[i] the canonical (A w)_j, (B w)_j, (C w)_j of j = Rows[i].
type WitnessViolations struct {
	Count  uint64
	Rows   []uint32
	Values [][3]*big.Int
}

// Ok reports whether the witness satisfies every constraint.
func (v WitnessViolations) Ok() bool { return v.Count == 0 }

// R1csCheck names the constraints a resident witness (NVars elements) breaks (gs_r1cs_check): every row of the system, not the roots
// of a key's Z that the prover's own count looks at; no key is needed and nothing is proved.  It runs beside proofs in flight.  cap = 0
// only counts.  A product system (UploadR1CSZkey) is refused: it holds no C.  C call sequence: tests/c/r1cs_check.c.
func R1csCheck(q *R1CS, w Handle, cap int) (WitnessViolations, error) {
	var v WitnessViolations
	if cap < 0 {
		return v, errors.New("gosnark-hip: negative cap")
	}
	rows := make([]uint32, cap)
	vals := make([]uint64, 12*cap)
	var count C.uint64_t
	err := call(func() C.int {
		return C.gs_r1cs_check(C.gs_handle(q.h), C.gs_handle(w), C.size_t(cap), &count, ptr32(rows), ptr(vals))
	})
	runtime.KeepAlive(rows)
	runtime.KeepAlive(vals)
	if err != nil {
		return v, err
	}
	v.Count = uint64(count)
	k := cap
	if v.Count < uint64(cap) {
		k = int(v.Count)
	}
	v.Rows = rows[:k]
	v.Values = make([][3]*big.Int, k)
	for i := range v.Values {
		abc := unpackScalars(vals[12*i : 12*i+12])
		v.Values[i] = [3]*big.Int{abc[0], abc[1], abc[2]}
	}
	return v, nil
}
