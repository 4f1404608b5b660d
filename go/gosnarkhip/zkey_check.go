package gosnarkhip

/*
#include "gosnark_hip.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"unsafe"
)

// Checking a key before trusting it: every array of a Groth16 key is a linear image of the transcript's points, so a random linear
// combination of a section must equal a combination of transcript points whose scalars come out of the circuit (include/gosnark_hip.h,
// "checking a key and a transcript").  About a dozen table-free MSMs, a few scalar transforms and two pairing products -- no transform
// in the group.  The checks prove the key's relation to THIS circuit and THIS transcript, and the transcript's consistency with
// itself; they do not prove who contributed to either.  go-snark-study_amd/circom.py (VerifyZkey, VerifyPtau) reads the files and makes the
// host-side comparisons of the header.

// The checks of CheckKey, in the order of CheckReport.Checks.
var KeyCheckNames = []string{"coefs A", "coefs B", "A", "B1", "B2", "IC", "C", "H"}

// The checks of CheckPtau.
var PtauCheckNames = []string{"g1", "g2", "tau", "tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2"}

// CheckResult is one check: its two points (affine, standard form; G1 in the first 8 words, G2 in all 16; zero at infinity).  The
// coefs checks have no points: Lhs[0] is the number of rows that differ.
type CheckResult struct {
	OK             bool
	LhsG2, RhsG2   bool
	LhsInf, RhsInf bool
	Lhs, Rhs       [16]uint64
}

// CheckReport is what CheckKey / CheckPtau found: Failed has bit i set when Checks[i] did not pass.
type CheckReport struct {
	Failed uint32
	Checks []CheckResult
}

// OK is true only when every check passed.
func (r *CheckReport) OK() bool { return r.Failed == 0 }

// KeyCheckInput names the resident objects of one key check: the key's arrays as they lie in the sections of the .zkey (C is section
// 8: nVars - nPublic - 1 points), the key's own section 4 as a product system (UploadR1CSZkey), the circuit's domain R1CS with the
// public rows appended to A (UploadR1CSDomain), the transcript's sections (TauG1: at least 2m - 1 points, the others m), delta2 as a
// Jacobian triple and the 256-bit challenge, drawn after all of these are fixed.
type KeyCheckInput struct {
	A, B1, B2, IC, C, H                  Handle
	KeySystem, CircuitSystem             *R1CS
	TauG1, TauG2, AlphaTauG1, BetaTauG1  Handle
	Delta2                               []uint64
	Challenge                            []uint64
	Log2Domain, NPublic                  int
}

func checkABI() error {
	var in, rep C.size_t
	C.gs_check_abi_sizes(&in, &rep)
	if uintptr(in) != unsafe.Sizeof(C.gs_key_check_input{}) || uintptr(rep) != unsafe.Sizeof(C.gs_check_report{}) {
		return errors.New("gosnark-hip: the library's gs_key_check_input / gs_check_report differ from this binding's header")
	}
	return nil
}

func reportFromC(rep *C.gs_check_report) *CheckReport {
	out := &CheckReport{Failed: uint32(rep.failed)}
	for i := 0; i < int(rep.nchecks); i++ {
		c := &rep.check[i]
		r := CheckResult{OK: c.ok != 0, LhsG2: c.lhs_g2 != 0, RhsG2: c.rhs_g2 != 0, LhsInf: c.lhs_inf != 0, RhsInf: c.rhs_inf != 0}
		for j := 0; j < 16; j++ {
			r.Lhs[j], r.Rhs[j] = uint64(c.lhs[j]), uint64(c.rhs[j])
		}
		out.Checks = append(out.Checks, r)
	}
	return out
}

// CheckKey runs gs_groth16_key_check: coefs A, coefs B, A, B1, B2, IC, C, H.  Blocking; every sum is table-free and none of the
// handles owns a window table afterwards.
func CheckKey(in *KeyCheckInput) (*CheckReport, error) {
	if len(in.Delta2) != 24 || len(in.Challenge) != 4 {
		return nil, errors.New("gosnark-hip: delta2 is a Jacobian triple of 24 limbs, the challenge four limbs")
	}
	if in.KeySystem == nil || in.CircuitSystem == nil {
		return nil, errors.New("gosnark-hip: CheckKey needs both systems")
	}
	if err := checkABI(); err != nil {
		return nil, err
	}
	var ci C.gs_key_check_input
	ci.a, ci.b1, ci.b2, ci.ic, ci.c, ci.h = C.gs_handle(in.A), C.gs_handle(in.B1), C.gs_handle(in.B2), C.gs_handle(in.IC), C.gs_handle(in.C), C.gs_handle(in.H)
	ci.key_system, ci.circuit_system = C.gs_handle(in.KeySystem.h), C.gs_handle(in.CircuitSystem.h)
	ci.tau_g1, ci.tau_g2 = C.gs_handle(in.TauG1), C.gs_handle(in.TauG2)
	ci.alpha_tau_g1, ci.beta_tau_g1 = C.gs_handle(in.AlphaTauG1), C.gs_handle(in.BetaTauG1)
	for i, v := range in.Delta2 {
		ci.delta2[i] = C.uint64_t(v)
	}
	for i, v := range in.Challenge {
		ci.challenge[i] = C.uint64_t(v)
	}
	ci.log2_domain, ci.npublic = C.uint64_t(in.Log2Domain), C.uint64_t(in.NPublic)
	var rep C.gs_check_report
	if err := call(func() C.int { return C.gs_groth16_key_check(&ci, &rep) }); err != nil {
		return nil, err
	}
	return reportFromC(&rep), nil
}

// CheckPtau runs gs_ptau_check on the first 2^log2N powers of a resident transcript: both generators, one tau in both groups,
// geometric alphaTauG1 / betaTauG1, betaG2 (a Jacobian triple) against betaTauG1[0].
func CheckPtau(tauG1, tauG2, alphaTauG1, betaTauG1 Handle, betaG2 []uint64, log2N int, challenge []uint64) (*CheckReport, error) {
	if len(betaG2) != 24 || len(challenge) != 4 {
		return nil, errors.New("gosnark-hip: betaG2 is a Jacobian triple of 24 limbs, the challenge four limbs")
	}
	if err := checkABI(); err != nil {
		return nil, err
	}
	var rep C.gs_check_report
	err := call(func() C.int {
		return C.gs_ptau_check(C.gs_handle(tauG1), C.gs_handle(tauG2), C.gs_handle(alphaTauG1), C.gs_handle(betaTauG1), ptr(betaG2), C.size_t(log2N),
			ptr(challenge), &rep)
	})
	runtime.KeepAlive(betaG2)
	runtime.KeepAlive(challenge)
	if err != nil {
		return nil, err
	}
	return reportFromC(&rep), nil
}
