package gosnarkhip

/*
#include "gosnark_hip.h"
*/
import "C"

import (
	"errors"
	"math/big"
	"runtime"
	"unsafe"
)

// SolveStats is gs_solve_stats: what the level plan of a system found.  Solved rows define one variable each; Unsolved variables are
// defined by no row (they are 0 in every witness); Checks are rows that define nothing and whose variables are all known (R1csSolve
// does not examine them: R1csCheck does); Stuck rows hold a variable that stays unsolved.
type SolveStats struct {
	Solved, Unsolved, Checks, Stuck, Levels, Launches, WideLaunches, WidestLevel uint64
}

// SolvePlan is the resident level plan of one system for one list of input variables.  It keeps its system alive on the device.
type SolvePlan struct {
	h       Handle
	NInputs int
	NVars   int
	Stats   SolveStats
}

// NoFailedRow is FirstFailedRow's value for a witness without a zero divisor.
const NoFailedRow = ^uint32(0)

func init() {
	var ob, sb C.size_t
	C.gs_solve_abi_sizes(&ob, &sb)
	if uintptr(ob) != unsafe.Sizeof(C.gs_solve_opts{}) || uintptr(sb) != unsafe.Sizeof(C.gs_solve_stats{}) {
		panic("gosnark-hip: libgosnark_hip.so was built from another revision of gosnark_hip.h (gs_solve_opts / gs_solve_stats)")
	}
}

// R1csSolvePlan plans how the witnesses of q are solved from the values of inputVars (gs_r1cs_solve_plan): once per circuit.  Variable 0
// is the constant one and never an input.  narrow / runMaxRows = 0 take the library's defaults.  A product system (UploadR1CSZkey) is
// refused: it holds no C.  C call sequence: tests/c/r1cs_solve.c.
func R1csSolvePlan(q *R1CS, inputVars []uint32, narrow, runMaxRows uint32) (*SolvePlan, error) {
	opts := C.gs_solve_opts{narrow: C.uint32_t(narrow), run_max_rows: C.uint32_t(runMaxRows)}
	var st C.gs_solve_stats
	var h C.gs_handle
	err := call(func() C.int {
		return C.gs_r1cs_solve_plan(C.gs_handle(q.h), ptr32(inputVars), C.size_t(len(inputVars)), &opts, &h, &st)
	})
	runtime.KeepAlive(inputVars)
	if err != nil {
		return nil, err
	}
	return &SolvePlan{h: Handle(h), NInputs: len(inputVars), NVars: q.NVars, Stats: SolveStats{
		Solved: uint64(st.solved), Unsolved: uint64(st.unsolved), Checks: uint64(st.checks), Stuck: uint64(st.stuck), Levels: uint64(st.levels),
		Launches: uint64(st.launches), WideLaunches: uint64(st.wide_launches), WidestLevel: uint64(st.widest_level)}}, nil
}

// Free releases the plan (and its system, once the system's own handle is gone).
func (p *SolvePlan) Free() error { return Free(p.h) }

// R1csSolveUnsolved lists the variables no row defines, ascending (gs_r1cs_solve_unsolved).
func R1csSolveUnsolved(p *SolvePlan) ([]uint32, error) {
	vars := make([]uint32, p.Stats.Unsolved)
	var count C.uint64_t
	err := call(func() C.int {
		return C.gs_r1cs_solve_unsolved(C.gs_handle(p.h), C.size_t(len(vars)), ptr32(vars), &count)
	})
	runtime.KeepAlive(vars)
	return vars, err
}

// SolveResult is what R1csSolve returns per witness: the resident vector (NVars elements, canonical, unsolved variables 0), how many rows
// met a zero divisor (their target is 0) and the first of them in solve order, or NoFailedRow.
type SolveResult struct {
	W              Handle
	NFailed        uint64
	FirstFailedRow uint32
}

// R1csSolve solves len(inputs) witnesses in one set of launches (gs_r1cs_solve).  inputs[b] holds the plan's NInputs values of witness b,
// any value below 2^256, counted mod r.  into may be nil, or hold per witness 0 (create) or a resident vector of NVars elements to
// overwrite.  It runs beside proofs in flight.  A zero divisor is not an error: look at NFailed.
func R1csSolve(p *SolvePlan, inputs [][]*big.Int, into []Handle) ([]SolveResult, error) {
	nwit := len(inputs)
	if nwit == 0 {
		return nil, errors.New("gosnark-hip: no witness to solve")
	}
	if into != nil && len(into) != nwit {
		return nil, errors.New("gosnark-hip: len(into) != len(inputs)")
	}
	words := make([]uint64, 4*nwit*p.NInputs+4)
	for b, row := range inputs {
		if len(row) != p.NInputs {
			return nil, errors.New("gosnark-hip: a witness does not bring one value per input variable")
		}
		for k, v := range row {
			if v.Sign() < 0 || v.BitLen() > 256 {
				return nil, errors.New("gosnark-hip: input value out of range")
			}
			if err := limbs(words[4*(b*p.NInputs+k):4*(b*p.NInputs+k)+4], v); err != nil {
				return nil, err
			}
		}
	}
	hs := make([]C.gs_handle, nwit)
	for b := range into {
		hs[b] = C.gs_handle(into[b])
	}
	nfailed := make([]uint64, nwit)
	first := make([]uint32, nwit)
	err := call(func() C.int {
		return C.gs_r1cs_solve(C.gs_handle(p.h), C.size_t(nwit), ptr(words), &hs[0], ptr(nfailed), ptr32(first))
	})
	runtime.KeepAlive(words)
	runtime.KeepAlive(nfailed)
	runtime.KeepAlive(first)
	if err != nil {
		return nil, err
	}
	out := make([]SolveResult, nwit)
	for b := range out {
		out[b] = SolveResult{W: Handle(hs[b]), NFailed: nfailed[b], FirstFailedRow: first[b]}
	}
	return out, nil
}
