package gosnarkhip

/*
#include "gosnark_hip.h"
*/
import "C"

import (
	"errors"
	"runtime"
)

// One phase-1 (powers-of-tau) contribution: a new secret is multiplied into a transcript whose tau nobody knows, on the points.
// go-snark-study_amd/circom.py (NewPtau, ContributePtau) documents the file layout, the streaming in slabs and what is NOT produced (no proof of
// knowledge, no challenge hash: the result is for SetupZkeyArrays / CheckPtau, not for `snarkjs powersoftau verify`).

// ScalePowersG1 gives out[i] = (c t^i mod r) P[off+i] for i < n, c and t as four limbs each, any 256-bit value
// (gs_g1_scale_powers).  t^0 = 1 also for t = 0; t = 1 is a uniform scale.  The series is built on the device.
func ScalePowersG1(bases Handle, off, n int, c, t []uint64) (Handle, error) {
	if len(c) != 4 || len(t) != 4 {
		return 0, errors.New("gosnark-hip: a scalar is four 64-bit limbs")
	}
	var h C.gs_handle
	err := call(func() C.int { return C.gs_g1_scale_powers(C.gs_handle(bases), C.size_t(off), C.size_t(n), ptr(c), ptr(t), &h) })
	runtime.KeepAlive(c)
	runtime.KeepAlive(t)
	return Handle(h), err
}

// ScalePowersG2 is ScalePowersG1 for G2 points (gs_g2_scale_powers).
func ScalePowersG2(bases Handle, off, n int, c, t []uint64) (Handle, error) {
	if len(c) != 4 || len(t) != 4 {
		return 0, errors.New("gosnark-hip: a scalar is four 64-bit limbs")
	}
	var h C.gs_handle
	err := call(func() C.int { return C.gs_g2_scale_powers(C.gs_handle(bases), C.size_t(off), C.size_t(n), ptr(c), ptr(t), &h) })
	runtime.KeepAlive(c)
	runtime.KeepAlive(t)
	return Handle(h), err
}

// PtauArrays are the four array sections of a transcript, resident: tauG1 (2^(power+1) - 1 points), tauG2, alphaTauG1, betaTauG1
// (2^power each).  betaG2 is one point: ScalePowersG2(betaG2, 0, 1, beta, one).
type PtauArrays struct {
	TauG1, TauG2, AlphaTauG1, BetaTauG1 Handle
}

// ContributePtauArrays multiplies (tau, alpha, beta) into whole resident sections: tauG1[i] *= tau^i, tauG2[i] *= tau^i,
// alphaTauG1[i] *= alpha tau^i, betaTauG1[i] *= beta tau^i -> four new arrays; the inputs stay as they are.  n1 points of tauG1 and
// n points of the others are taken.  4 x gs_g*_scale_powers.  Call sequence = tests/c/ptau_contribute.c.  A caller that streams a
// long section in slabs passes c tau^s for the slab that starts at index s (circom.py, ContributePtau).
func ContributePtauArrays(in PtauArrays, n1, n int, tau, alpha, beta []uint64) (*PtauArrays, error) {
	one := []uint64{1, 0, 0, 0}
	var out PtauArrays
	var err error
	fail := func(e error) (*PtauArrays, error) {
		for _, h := range []Handle{out.TauG1, out.TauG2, out.AlphaTauG1, out.BetaTauG1} {
			if h != 0 {
				_ = Free(h)
			}
		}
		return nil, e
	}
	if out.TauG1, err = ScalePowersG1(in.TauG1, 0, n1, one, tau); err != nil {
		return fail(err)
	}
	if out.TauG2, err = ScalePowersG2(in.TauG2, 0, n, one, tau); err != nil {
		return fail(err)
	}
	if out.AlphaTauG1, err = ScalePowersG1(in.AlphaTauG1, 0, n, alpha, tau); err != nil {
		return fail(err)
	}
	if out.BetaTauG1, err = ScalePowersG1(in.BetaTauG1, 0, n, beta, tau); err != nil {
		return fail(err)
	}
	return &out, nil
}

// LagrangeLevelsG1 gives the Lagrange bases of the domains 2^lo .. 2^hi over the first points of a resident section
// (gs_g1_lagrange_levels): 2^(hi+1) - 2^lo points, level p -- LagrangeG1(powers, 0, p, false) of the first 2^p points -- at index
// 2^p - 2^lo.  One launch carries the stage of one span for every level.  An array of exactly 2^hi - 1 points: the missing last point
// of level hi is the point at infinity (tauG1's level power + 1).
func LagrangeLevelsG1(powers Handle, lo, hi int) (Handle, error) {
	var h C.gs_handle
	err := call(func() C.int { return C.gs_g1_lagrange_levels(C.gs_handle(powers), C.size_t(lo), C.size_t(hi), &h) })
	return Handle(h), err
}

// LagrangeLevelsG2 is LagrangeLevelsG1 for G2 points (gs_g2_lagrange_levels).
func LagrangeLevelsG2(powers Handle, lo, hi int) (Handle, error) {
	var h C.gs_handle
	err := call(func() C.int { return C.gs_g2_lagrange_levels(C.gs_handle(powers), C.size_t(lo), C.size_t(hi), &h) })
	return Handle(h), err
}

func resultFromC(c *C.gs_check_result) *CheckResult {
	r := &CheckResult{OK: c.ok != 0, LhsG2: c.lhs_g2 != 0, RhsG2: c.rhs_g2 != 0, LhsInf: c.lhs_inf != 0, RhsInf: c.rhs_inf != 0}
	for j := 0; j < 16; j++ {
		r.Lhs[j], r.Rhs[j] = uint64(c.lhs[j]), uint64(c.rhs[j])
	}
	return r
}

// CheckLagrangeLevelsG1 asks whether the first 2^(hi+1) - 1 points of levels are the levels 0 .. hi of powers
// (gs_g1_lagrange_levels_check): one sum over each array and scalar transforms, nothing is transformed in the group.  The challenge is
// four limbs, not 0 mod r, drawn after both arrays are fixed.  hi <= 25.
func CheckLagrangeLevelsG1(powers, levels Handle, hi int, challenge []uint64) (*CheckResult, error) {
	if len(challenge) != 4 {
		return nil, errors.New("gosnark-hip: the challenge is four limbs")
	}
	var res C.gs_check_result
	err := call(func() C.int {
		return C.gs_g1_lagrange_levels_check(C.gs_handle(powers), C.gs_handle(levels), C.size_t(hi), ptr(challenge), &res)
	})
	runtime.KeepAlive(challenge)
	if err != nil {
		return nil, err
	}
	return resultFromC(&res), nil
}

// CheckLagrangeLevelsG2 is CheckLagrangeLevelsG1 for G2 points (gs_g2_lagrange_levels_check); include/gosnark_hip.h says what the
// bound means in G2.
func CheckLagrangeLevelsG2(powers, levels Handle, hi int, challenge []uint64) (*CheckResult, error) {
	if len(challenge) != 4 {
		return nil, errors.New("gosnark-hip: the challenge is four limbs")
	}
	var res C.gs_check_result
	err := call(func() C.int {
		return C.gs_g2_lagrange_levels_check(C.gs_handle(powers), C.gs_handle(levels), C.size_t(hi), ptr(challenge), &res)
	})
	runtime.KeepAlive(challenge)
	if err != nil {
		return nil, err
	}
	return resultFromC(&res), nil
}

// PreparePtauArrays gives the prepared sections 12 .. 15 of a transcript of 2^power from its resident sections: the levels
// 0 .. power + 1 of tauG1 (2^(power+1) - 1 points in, the padded top level) and 0 .. power of tauG2, alphaTauG1, betaTauG1; the inputs
// stay as they are.  4 x gs_g*_lagrange_levels.  Call sequence = tests/c/ptau_prepare.c.  power <= 26.
func PreparePtauArrays(in PtauArrays, power int) (*PtauArrays, error) {
	var out PtauArrays
	var err error
	fail := func(e error) (*PtauArrays, error) {
		for _, h := range []Handle{out.TauG1, out.TauG2, out.AlphaTauG1, out.BetaTauG1} {
			if h != 0 {
				_ = Free(h)
			}
		}
		return nil, e
	}
	if out.TauG1, err = LagrangeLevelsG1(in.TauG1, 0, power+1); err != nil {
		return fail(err)
	}
	if out.TauG2, err = LagrangeLevelsG2(in.TauG2, 0, power); err != nil {
		return fail(err)
	}
	if out.AlphaTauG1, err = LagrangeLevelsG1(in.AlphaTauG1, 0, power); err != nil {
		return fail(err)
	}
	if out.BetaTauG1, err = LagrangeLevelsG1(in.BetaTauG1, 0, power); err != nil {
		return fail(err)
	}
	return &out, nil
}
